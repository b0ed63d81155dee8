/*
 * g4d_render.h -- C ABI of libg4d_render.so: an exact-coverage tiled rasterizer for the meshes the model predicts (the picture
 * utils/nr_utils.py:33-81 draws with neural_renderer, plus a depth image and a per-sample face index).
 *
 * Visualisation, not part of the model's ABI: its own header and its own shared object, which links against libg4d_hip.so -- the boundary
 * contract of g4d.h holds unchanged (raw device pointers + sizes + a HIP stream, status codes, ONE error state: g4d_last_error()).
 * Every kernel is enqueued on `stream`; none synchronises, allocates or uses an atomic; all scratch comes through g4d_render_ws_bytes, so a
 * call can be captured in a hipGraph.  Two runs give the same bits, and the bits do not depend on how faces are binned or in which order
 * tiles run.  Every fp32 expression below is written with its order: one rounded operation per sign, nothing fused (-ffp-contract=off);
 * division and square root are the correctly rounded ones.
 *
 * neural_renderer is not available to this project: pixel parity with it is NOT claimed.  The contract is this header's; camera and light
 * follow that library's documented defaults (look-at camera, viewing angle 30 degrees, ambient 0.5 + directional 0.5 along (0, 1, 0)).
 * Deviations by design: coverage is the exact top-left rule on a fixed-point grid instead of a float inside test, both sides of a face are lit
 * (the normal is turned towards the viewer), anti-aliasing is the plain mean of ss x ss samples.  Nothing is clipped (the reference's
 * renderer does not clip either): a face that cannot be drawn is DROPPED, see g4d_render_raster.
 */
#ifndef G4D_RENDER_H
#define G4D_RENDER_H

#include "g4d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Limits: ss in {1, 2, 4} samples per pixel edge; ss * W and ss * H <= G4D_RENDER_MAX_SAMPLES; fixed-point coordinates are drawn while
 * every |x|, |y| < 2^G4D_RENDER_COORD_BITS (every edge function then fits int64 with room to spare: |E| < 2^48). */
#define G4D_RENDER_MAX_SAMPLES 4096
#define G4D_RENDER_SUBSAMPLE_BITS 8
#define G4D_RENDER_COORD_BITS 22
#define G4D_RENDER_TILE 16

/* Faces per chunk of the tile kernel's walk (one box test per lane of a 256-lane workgroup): a measurement / test aid ("one chunk plus one"). */
int g4d_render_chunk(void);

/* Bytes of device scratch g4d_render_raster needs for `frames` x `nf` faces: per (frame, face) an 8-byte sample box and a 96-byte record, per
 * (frame, chunk of faces) an 8-byte box; each of the three arrays rounded up to 16 bytes.  0 for an empty problem; (size_t)-1 for a negative size. */
size_t g4d_render_ws_bytes(int frames, int nf);

/* ---- projection ---------------------------------------------------------------------------------------------------------------------------
 * verts (frames,V,3), or (V,3) shared by all frames when shared_verts != 0.  Camera: eye, at, up, half viewing angle in DEGREES, near > 0.
 * Image: W x H pixels, ss samples per pixel edge; Ws = ss * W, Hs = ss * H samples.
 *
 * On the host, in double (IEEE, no fused operation), once per call:
 *   z = at - eye;  z = z / sqrt((z.x^2 + z.y^2) + z.z^2);   x = up X z;  x = x / sqrt(...);   y = z X x;  y = y / sqrt(...)
 *   with  (a X b).x = a.y * b.z - a.z * b.y  (and cyclic);   s = 1 / tan(half_angle * (pi / 180))
 *   then rounded to fp32: R = rows (x, y, z), s, and hh = 128 * Hs, hw = 128 * Ws (exact).  A zero-length z or x is G4D_EINVAL.
 * Per vertex and frame, in fp32:
 *   d = v - eye;   cam.k = (R[k][0] * d.x + R[k][1] * d.y) + R[k][2] * d.z   for k = x, y, z
 *   q = 1 / cam.z                                                             (the one division)
 *   fx = ((cam.x * q) * s) * hh + hw;     fy = hh - ((cam.y * q) * s) * hh   (one scale, hh, for both axes: square samples)
 *   px = |fx| < 2^30 ? (int)rint(fx) : 2^30   (rint: to nearest, ties to even; a NaN takes the second branch);   py likewise from fy
 *   invz = cam.z >= near ? q : 0              (0 marks a vertex that must not be drawn; NaN compares false)
 * The unit of px, py is 1 / 256 of a sample: sample (i, j) has its centre at (256 i + 128, 256 j + 128); row 0 is the top of the image,
 * +y of the camera.  cam (frames,V,3) or NULL receives the camera-space positions (g4d_render_raster shades from them).
 * px, py, invz are (frames,V) also when the vertices are shared. */
int g4d_render_project_f32(int frames, int v, int shared_verts, const float *verts, float eye_x, float eye_y, float eye_z, float at_x, float at_y,
                           float at_z, float up_x, float up_y, float up_z, float half_angle_deg, float near, int w, int h, int ss, int *px, int *py,
                           float *invz, float *cam, g4d_stream_t stream);

/* ---- rasterization ------------------------------------------------------------------------------------------------------------------------
 * px, py (frames,V) int32 and invz (frames,V) as above (any integers will do: the stage is defined on them); faces (nf,3) int32, shared by
 * all frames.  faces_host: the same array in HOST memory or NULL; when given, every index is checked against [0, V) before any launch
 * (G4D_EINVAL).  Without it the check is the kernel's: a face with an index outside [0, V) is dropped, never read through.
 *
 * A face (i0, i1, i2) is DROPPED (drawn nowhere; documented, not an error) when any of
 *   - an invz of its vertices is not in (0, inf)  (a vertex behind `near`),
 *   - any |px|, |py| of its vertices >= 2^22,
 *   - area2 = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0) == 0                                  (int64).
 * Orientation: area2 < 0 -> vertices 1 and 2 change places and area2 = -area2; winding does not matter, both sides are drawn.
 *
 * Coverage, in exact int64 arithmetic at the sample centre s = (256 i + 128, 256 j + 128):
 *   edge k runs p -> q with (p, q) = (v1, v2), (v2, v0), (v0, v1) for k = 0, 1, 2;   dx = q.x - p.x, dy = q.y - p.y
 *   E_k(s) = dx * (s.y - p.y) - dy * (s.x - p.x)                  (E_0 + E_1 + E_2 = area2 at every s)
 *   edge k OWNS its line when dy < 0 (a left edge) or dy == 0 and dx > 0 (a top edge)
 *   s is covered  <=>  for every k:  E_k(s) > 0, or E_k(s) == 0 and edge k owns its line        (the top-left rule)
 * so a sample on an edge shared by two faces, or on a vertex of a closed fan, belongs to exactly one of them.
 *
 * Depth at a covered sample (fp32; (float) of an int64 rounds to nearest even):
 *   b1 = (float)E_1 / (float)area2,   b2 = (float)E_2 / (float)area2
 *   iz = (iz0 + b1 * (iz1 - iz0)) + b2 * (iz2 - iz0)              (iz0, iz1, iz2: invz of the ORIENTED vertices)
 * Visible face: faces are taken in ascending index; the first covering face is taken, a later one replaces it iff its iz is GREATER.  So the
 * largest iz wins and a tie goes to the lowest index.  face_id (frames,Hs,Ws) int32 = that index or -1; depth (frames,Hs,Ws) = 1 / iz or +inf.
 *
 * Shade, flat per face (cam (frames,V,3) from the projection; NULL: shade = 1, unlit), from the vertices in the caller's order:
 *   n = (c1 - c0) X (c2 - c0);   n = -n if (n.x * c0.x + n.y * c0.y) + n.z * c0.z > 0          (towards the viewer, who sits at the origin)
 *   len = sqrt((n.x^2 + n.y^2) + n.z^2);   cosl = len > 0 ? ((n.x * l.x + n.y * l.y) + n.z * l.z) / len : 0;   cosl = cosl > 0 ? cosl : 0
 *   shade = ambient + directional * cosl            (l = (light_x, light_y, light_z): the light's direction in CAMERA space, taken as given)
 * Colour of a covered sample: albedo * shade per channel, albedo = (1, 1, 1), or face_rgb[face] ((nf,3)), or from vert_rgb ((V,3)) with
 *   b0 = (float)E_0 / (float)area2;  w_k = b_k * iz_k;   albedo = (((w0 * c0 + w1 * c1) + w2 * c2) / iz)   (perspective-correct)
 * (face_rgb and vert_rgb together: G4D_EINVAL).  An uncovered sample has the background colour.
 * image (frames,H,W,3) or NULL: each pixel = (sum of its ss x ss sample colours, rows top to bottom, left to right within a row, added one by
 * one to the first) * (1 / ss^2), the background included.
 *
 * cull != 0: a tile (16 x 16 samples, one workgroup) walks the faces in chunks of g4d_render_chunk(), skips a chunk whose box (the join of
 * its faces' boxes, written by the setup launch) misses it, and keeps of the others the faces whose sample box
 *   [ceil((min x - 128) / 256), floor((max x - 128) / 256)] x [the same in y]  meets it, by an order-preserving compaction; cull == 0: every
 * face that is not dropped.  The box contains every sample a face covers, so both settings give the same bits.
 * kept (frames * ceil(Hs / 16) * ceil(Ws / 16)) int32 or NULL: the number of faces each tile kept (a measurement aid).
 * ws: g4d_render_ws_bytes(frames, nf) bytes, 16-byte aligned; ws_bytes: what the caller allocated (less: G4D_EINVAL).
 * Errors (G4D_EINVAL before any launch): a null pointer, a negative size, ss not in {1, 2, 4}, ss * w or ss * h > 4096, a face index outside
 * [0, v) in faces_host.  frames, nf, w or h == 0 ... an empty problem: returns 0; with nf == 0 the outputs are still written (all background). */
int g4d_render_raster(int frames, int v, int nf, int w, int h, int ss, int cull, const int *px, const int *py, const float *invz, const float *cam,
                      const int *faces, const int *faces_host, const float *face_rgb, const float *vert_rgb, float light_x, float light_y,
                      float light_z, float ambient, float directional, float bg_r, float bg_g, float bg_b, void *ws, size_t ws_bytes, int *face_id,
                      float *depth, float *image, int *kept, g4d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* G4D_RENDER_H */
