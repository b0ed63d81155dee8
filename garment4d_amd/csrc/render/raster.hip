// Exact-coverage tiled rasterizer (include/g4d_render.h is the contract; tests/render_twin.py restates it in numpy).
//   project_kernel : one lane per (frame, vertex): look-at transform, one division, snap to the 1/256-sample grid.
//   setup_kernel   : one lane per (frame, face): orient, three biased edge functions, sample box, the oriented invz, the flat shade -> a 96-byte
//                    record + an 8-byte box (the tile kernel's walk reads the boxes only), and per chunk of 256 faces the join of their boxes.
//   tile_kernel    : one workgroup per (frame, 16 x 16 sample tile), lanes on samples.  Walks the chunks in ascending order, skips a chunk whose
//                    box misses the tile, keeps of the others the faces that meet the tile by a ballot / prefix compaction (order preserved),
//                    stages their records in LDS, tests its samples; then shades the winner and resolves the tile's pixels (ss x ss mean)
//                    through LDS.  Sizes: a 16 x 16 tile is one sample per lane of a 256-lane workgroup and holds whole pixels for ss = 1, 2, 4;
//                    a chunk of 256 is one box test per lane, and its 256 staged records are 24 KB of LDS (6 workgroups per CU).
// No atomics: a sample is owned by one lane, a pixel by one lane.  Nothing depends on the order of tiles.
#include "../g4d_common.h"
#include "../../../include/g4d_render.h"

#include <math.h>

namespace g4d {

constexpr int kTile = G4D_RENDER_TILE, kRThreads = kTile * kTile, kChunk = kRThreads;
constexpr int kCoordLimit = 1 << G4D_RENDER_COORD_BITS;
constexpr int kNoCoord = 1 << 30;

struct alignas(16) FaceRec {   // 96 bytes = 6 x 16
    long long area2;
    long long c[3];      // E_k(s) - (edge k owns its line ? 0 : 1) = c[k] + a[k] * s.x + b[k] * s.y:  covered <=> all three >= 0
    int a[3], b[3];
    float iz[3];         // invz of the oriented vertices
    float shade;
    int vid[3];          // the oriented vertices
    int flags;           // bit 0: drawn; bit 1 + k: edge k does NOT own its line (E_k = biased value + 1)
};
static_assert(sizeof(FaceRec) == 96, "FaceRec is staged as six 16-byte pieces");

struct Camera {
    float r[9], eye[3], s, hh, hw, near;
};

__global__ void __launch_bounds__(256) project_kernel(long long total, int v, int shared, Camera cm, const float *__restrict__ verts, int *__restrict__ px,
                                                      int *__restrict__ py, float *__restrict__ invz, float *__restrict__ cam) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const float *p = verts + (size_t)(shared ? g % v : g) * 3;
    const float dx = p[0] - cm.eye[0], dy = p[1] - cm.eye[1], dz = p[2] - cm.eye[2];
    const float cx = (cm.r[0] * dx + cm.r[1] * dy) + cm.r[2] * dz;
    const float cy = (cm.r[3] * dx + cm.r[4] * dy) + cm.r[5] * dz;
    const float cz = (cm.r[6] * dx + cm.r[7] * dy) + cm.r[8] * dz;
    const float q = 1.0f / cz;
    const float fx = ((cx * q) * cm.s) * cm.hh + cm.hw;
    const float fy = cm.hh - ((cy * q) * cm.s) * cm.hh;
    px[g] = fabsf(fx) < 1073741824.f ? (int)rintf(fx) : kNoCoord;
    py[g] = fabsf(fy) < 1073741824.f ? (int)rintf(fy) : kNoCoord;
    invz[g] = cz >= cm.near ? q : 0.f;
    if (cam) {
        cam[(size_t)g * 3] = cx; cam[(size_t)g * 3 + 1] = cy; cam[(size_t)g * 3 + 2] = cz;
    }
}

struct Shading {
    float l[3], ambient, directional, bg[3];
};

// One workgroup per (frame, chunk of kChunk faces): lane t sets up face chunk * kChunk + t, then the workgroup joins the sample boxes of its
// faces into the chunk's box (a dropped face has the empty box {max, max, min, min}: the identity of the join).
__global__ void __launch_bounds__(kChunk) setup_kernel(int v, int nf, int nchunks, Shading sh, const int *__restrict__ px, const int *__restrict__ py,
                                                       const float *__restrict__ invz, const float *__restrict__ cam, const int *__restrict__ faces,
                                                       short *__restrict__ boxes, short *__restrict__ chunk_boxes, FaceRec *__restrict__ recs) {
    __shared__ int s_box[kChunk / kWave][4];
    const int f = blockIdx.x / nchunks, k = (blockIdx.x - f * nchunks) * kChunk + threadIdx.x;
    const bool live = k < nf;
    const size_t g = (size_t)f * nf + (live ? k : 0);
    int id[3] = {-1, -1, -1};
    if (live)
        for (int e = 0; e < 3; ++e) id[e] = faces[(size_t)k * 3 + e];
    FaceRec r;
    r.area2 = 0;
    r.flags = 0;
    r.shade = 1.f;
    for (int e = 0; e < 3; ++e) {
        r.c[e] = -1; r.a[e] = 0; r.b[e] = 0; r.iz[e] = 0.f; r.vid[e] = 0;
    }
    short box[4] = {32767, 32767, -32768, -32768};
    bool ok = (unsigned)id[0] < (unsigned)v && (unsigned)id[1] < (unsigned)v && (unsigned)id[2] < (unsigned)v;
    if (ok) {
        const size_t base = (size_t)f * v;
        int x[3], y[3];
        float iz[3];
        for (int e = 0; e < 3; ++e) {
            x[e] = px[base + id[e]]; y[e] = py[base + id[e]]; iz[e] = invz[base + id[e]];
            ok = ok && iz[e] > 0.f && iz[e] < INFINITY && x[e] > -kCoordLimit && x[e] < kCoordLimit && y[e] > -kCoordLimit && y[e] < kCoordLimit;
        }
        if (ok) {
            if (cam) {   // from the caller's vertex order
                const float *c0 = cam + (base + id[0]) * 3, *c1 = cam + (base + id[1]) * 3, *c2 = cam + (base + id[2]) * 3;
                const float ux = c1[0] - c0[0], uy = c1[1] - c0[1], uz = c1[2] - c0[2];
                const float wx = c2[0] - c0[0], wy = c2[1] - c0[1], wz = c2[2] - c0[2];
                float nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
                if ((nx * c0[0] + ny * c0[1]) + nz * c0[2] > 0.f) {
                    nx = -nx; ny = -ny; nz = -nz;
                }
                const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
                float cosl = len > 0.f ? ((nx * sh.l[0] + ny * sh.l[1]) + nz * sh.l[2]) / len : 0.f;
                cosl = cosl > 0.f ? cosl : 0.f;
                r.shade = sh.ambient + sh.directional * cosl;
            }
            long long area2 = (long long)(x[1] - x[0]) * (y[2] - y[0]) - (long long)(x[2] - x[0]) * (y[1] - y[0]);
            if (area2 < 0) {
                int t = x[1]; x[1] = x[2]; x[2] = t;
                t = y[1]; y[1] = y[2]; y[2] = t;
                t = id[1]; id[1] = id[2]; id[2] = t;
                const float ft = iz[1]; iz[1] = iz[2]; iz[2] = ft;
                area2 = -area2;
            }
            if (area2 > 0) {
                r.area2 = area2;
                r.flags = 1;
                for (int e = 0; e < 3; ++e) {
                    const int p = (e + 1) % 3, q = (e + 2) % 3;
                    const int dx = x[q] - x[p], dy = y[q] - y[p];
                    const bool owns = dy < 0 || (dy == 0 && dx > 0);
                    r.a[e] = -dy;
                    r.b[e] = dx;
                    r.c[e] = (long long)dy * x[p] - (long long)dx * y[p] - (owns ? 0 : 1);
                    r.flags |= owns ? 0 : (2 << e);
                    r.iz[e] = iz[e];
                    r.vid[e] = id[e];
                }
                const int x0 = min(x[0], min(x[1], x[2])), x1 = max(x[0], max(x[1], x[2]));
                const int y0 = min(y[0], min(y[1], y[2])), y1 = max(y[0], max(y[1], y[2]));
                box[0] = (short)((x0 - 128 + 255) >> 8);   // |x| < 2^22: |sample| <= 2^14, a short holds it
                box[1] = (short)((y0 - 128 + 255) >> 8);
                box[2] = (short)((x1 - 128) >> 8);
                box[3] = (short)((y1 - 128) >> 8);
            }
        }
    }
    if (live) {
        recs[g] = r;
        for (int e = 0; e < 4; ++e) boxes[g * 4 + e] = box[e];
    }
    int lo_x = box[0], lo_y = box[1], hi_x = box[2], hi_y = box[3];
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        lo_x = min(lo_x, __shfl_xor(lo_x, m)); lo_y = min(lo_y, __shfl_xor(lo_y, m));
        hi_x = max(hi_x, __shfl_xor(hi_x, m)); hi_y = max(hi_y, __shfl_xor(hi_y, m));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        int *o = s_box[threadIdx.x / kWave];
        o[0] = lo_x; o[1] = lo_y; o[2] = hi_x; o[3] = hi_y;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        int acc = s_box[0][threadIdx.x];
        for (int wv = 1; wv < kChunk / kWave; ++wv) acc = threadIdx.x < 2 ? min(acc, s_box[wv][threadIdx.x]) : max(acc, s_box[wv][threadIdx.x]);
        chunk_boxes[(size_t)blockIdx.x * 4 + threadIdx.x] = (short)acc;
    }
}

// the true edge functions of record r at the sample centre (sx, sy); returns whether the sample is covered
__device__ __forceinline__ bool edges(const FaceRec &r, int sx, int sy, long long E[3]) {
    long long all = 0;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        E[e] = r.c[e] + (long long)r.a[e] * sx + (long long)r.b[e] * sy;
        all |= E[e];
    }
    return all >= 0;   // no sign bit in any of the three biased values
}

__global__ void __launch_bounds__(kRThreads) tile_kernel(int frames, int nf, int ws_, int hs_, int w, int h, int ss, int cull, Shading sh,
                                                         const short *__restrict__ boxes, const short *__restrict__ chunk_boxes,
                                                         const FaceRec *__restrict__ recs, const float *__restrict__ face_rgb, const float *__restrict__ vert_rgb,
                                                         int *__restrict__ face_id, float *__restrict__ depth, float *__restrict__ image,
                                                         int *__restrict__ kept) {
    __shared__ FaceRec s_rec[kChunk];
    __shared__ int s_list[kChunk];
    const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    const int tiles_x = (ws_ + kTile - 1) / kTile, tiles_y = (hs_ + kTile - 1) / kTile;
    // Frame fastest: consecutive workgroups draw the SAME tile of consecutive frames.  A mesh fills a few tiles of its frame and misses most, in
    // every frame alike; tile-fastest numbering would leave the few busy workgroups of one or two frames alone on the device among hundreds of
    // empty ones, each waiting out its own chain of box loads.  This way the busy tiles come in runs of `frames` and hide each other's latency.
    const int f = blockIdx.x % frames, tile = blockIdx.x / frames;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int i = tx * kTile + (t & (kTile - 1)), j = ty * kTile + t / kTile;
    const int sx = 256 * i + 128, sy = 256 * j + 128;
    const int ti0 = tx * kTile, ti1 = ti0 + kTile - 1, tj0 = ty * kTile, tj1 = tj0 + kTile - 1;
    const short *fbox = boxes + (size_t)f * nf * 4;
    const short *cbox = chunk_boxes + (size_t)f * ((nf + kChunk - 1) / kChunk) * 4;
    const FaceRec *frec = recs + (size_t)f * nf;

    float best_iz = 0.f;
    int best = -1, nkept = 0, fill = 0;
    // the kept faces gathered so far (s_list[0 .. fill), ascending): stage their records and test this lane's sample against each, in order
    auto flush = [&]() {
        __syncthreads();   // every wave's part of the list is written
        for (int piece = t; piece < fill * 6; piece += kRThreads) {
            const int rr = piece / 6, part = piece - rr * 6;
            reinterpret_cast<uint4 *>(s_rec)[piece] = reinterpret_cast<const uint4 *>(frec + s_list[rr])[part];
        }
        __syncthreads();
        for (int rr = 0; rr < fill; ++rr) {
            const FaceRec &r = s_rec[rr];
            long long E[3];
            if (edges(r, sx, sy, E)) {
                const float a2 = (float)r.area2;
                const float b1 = (float)(E[1] + ((r.flags >> 2) & 1)) / a2, b2 = (float)(E[2] + ((r.flags >> 3) & 1)) / a2;
                const float iz = (r.iz[0] + b1 * (r.iz[1] - r.iz[0])) + b2 * (r.iz[2] - r.iz[0]);
                if (best < 0 || iz > best_iz) {
                    best_iz = iz;
                    best = s_list[rr];
                }
            }
        }
        __syncthreads();   // list and records are free again
        fill = 0;
    };
    const int nchunks = (nf + kChunk - 1) / kChunk;
    for (int c0 = 0; c0 < nchunks; c0 += kWave) {
        // The chunks' own boxes first, 64 at a time, one per lane: ONE load latency per 64 chunks (most tiles of a frame meet no chunk at all, and
        // a test per chunk in turn is a chain of dependent loads).  Every wave of the workgroup forms the same mask from the same data, so the
        // walk below -- ascending, like the faces inside a chunk -- is uniform over the workgroup and no lane waits at a barrier the others skip.
        bool meets = c0 + lane < nchunks;
        if (meets && cull) {
            const short4 cb = *reinterpret_cast<const short4 *>(cbox + (size_t)(c0 + lane) * 4);
            meets = cb.x <= ti1 && cb.z >= ti0 && cb.y <= tj1 && cb.w >= tj0;
        }
        for (unsigned long long todo = __ballot(meets); todo; todo &= todo - 1) {
            const int base = (c0 + __ffsll((long long)todo) - 1) * kChunk;
            // Every wave tests ALL boxes of the chunk, four per lane: the four ballots are then known to every wave without an exchange through
            // LDS, and a chunk costs no barrier.  A tile keeps a handful of faces per chunk, so the kept faces of many chunks share one flush.
            unsigned long long mask[kRThreads / kWave];
            int total = 0;
#pragma unroll
            for (int wv = 0; wv < kRThreads / kWave; ++wv) {
                const int k = base + wv * kWave + lane;
                bool keep = false;
                if (k < nf) {
                    const short4 b = *reinterpret_cast<const short4 *>(fbox + (size_t)k * 4);
                    keep = cull ? (b.x <= ti1 && b.z >= ti0 && b.y <= tj1 && b.w >= tj0) : (b.x != 32767);
                }
                mask[wv] = __ballot(keep);
                total += __popcll(mask[wv]);
            }
            if (total == 0) continue;
            if (fill + total > kChunk) flush();
            int off = fill;
            unsigned long long mine = 0;
#pragma unroll
            for (int wv = 0; wv < kRThreads / kWave; ++wv) {
                off += wv < wave ? __popcll(mask[wv]) : 0;
                mine = wv == wave ? mask[wv] : mine;
            }
            if ((mine >> lane) & 1) s_list[off + __popcll(mine & ((1ull << lane) - 1ull))] = base + t;   // this wave's own 64 faces of the chunk
            fill += total;
            nkept += total;
        }
    }
    if (fill) flush();
    if (kept && t == 0) kept[(size_t)f * (tiles_x * tiles_y) + tile] = nkept;

    float col[3] = {sh.bg[0], sh.bg[1], sh.bg[2]};
    if (best >= 0) {
        const FaceRec r = frec[best];
        float alb[3] = {1.f, 1.f, 1.f};
        if (face_rgb) {
            for (int c = 0; c < 3; ++c) alb[c] = face_rgb[(size_t)best * 3 + c];
        } else if (vert_rgb) {
            long long E[3];
            edges(r, sx, sy, E);
            const float a2 = (float)r.area2;
            float wgt[3];
            for (int e = 0; e < 3; ++e) wgt[e] = ((float)(E[e] + ((r.flags >> (1 + e)) & 1)) / a2) * r.iz[e];
            for (int c = 0; c < 3; ++c)
                alb[c] = ((wgt[0] * vert_rgb[(size_t)r.vid[0] * 3 + c] + wgt[1] * vert_rgb[(size_t)r.vid[1] * 3 + c]) +
                          wgt[2] * vert_rgb[(size_t)r.vid[2] * 3 + c]) / best_iz;
        }
        for (int c = 0; c < 3; ++c) col[c] = alb[c] * r.shade;
    }
    if (i < ws_ && j < hs_) {
        const size_t o = ((size_t)f * hs_ + j) * ws_ + i;
        face_id[o] = best;
        depth[o] = best >= 0 ? 1.0f / best_iz : INFINITY;
    }
    if (image) {
        __syncthreads();   // s_rec is free: its first 3 KB hold the tile's sample colours
        float *s_col = reinterpret_cast<float *>(s_rec);
        for (int c = 0; c < 3; ++c) s_col[c * kRThreads + t] = col[c];
        __syncthreads();
        const int ppt = kTile / ss;   // whole pixels: ss divides the tile
        if (t < ppt * ppt) {
            const int pxl = t % ppt, pyl = t / ppt;
            const int X = tx * ppt + pxl, Y = ty * ppt + pyl;
            if (X < w && Y < h) {
                const float inv = 1.0f / (float)(ss * ss);
                for (int c = 0; c < 3; ++c) {
                    float acc = 0.f;
                    for (int sj = 0; sj < ss; ++sj)
                        for (int si = 0; si < ss; ++si) {
                            const float val = s_col[c * kRThreads + (pyl * ss + sj) * kTile + pxl * ss + si];
                            acc = (sj | si) ? acc + val : val;
                        }
                    image[(((size_t)f * h + Y) * w + X) * 3 + c] = acc * inv;
                }
            }
        }
    }
}

static size_t box_bytes(int frames, int nf) { return (((size_t)frames * nf * 8) + 15) & ~(size_t)15; }
static size_t chunk_box_bytes(int frames, int nf) { return (((size_t)frames * ((nf + kChunk - 1) / kChunk) * 8) + 15) & ~(size_t)15; }

static int check_image(const char *who, int w, int h, int ss) {
    G4D_REQUIRE(ss == 1 || ss == 2 || ss == 4, "%s: ss must be 1, 2 or 4 (ss=%d)", who, ss);
    G4D_REQUIRE((long long)ss * w <= G4D_RENDER_MAX_SAMPLES && (long long)ss * h <= G4D_RENDER_MAX_SAMPLES,
                "%s: ss * w and ss * h must be <= %d (w=%d, h=%d, ss=%d)", who, G4D_RENDER_MAX_SAMPLES, w, h, ss);
    return G4D_OK;
}

}  // namespace g4d

using namespace g4d;

extern "C" int g4d_render_chunk(void) { return kChunk; }

extern "C" size_t g4d_render_ws_bytes(int frames, int nf) {
    if (frames < 0 || nf < 0) return (size_t)-1;
    return box_bytes(frames, nf) + chunk_box_bytes(frames, nf) + (size_t)frames * nf * sizeof(FaceRec);
}

extern "C" int g4d_render_project_f32(int frames, int v, int shared_verts, const float *verts, float eye_x, float eye_y, float eye_z, float at_x,
                                      float at_y, float at_z, float up_x, float up_y, float up_z, float half_angle_deg, float near, int w, int h, int ss,
                                      int *px, int *py, float *invz, float *cam, g4d_stream_t stream) {
    G4D_REQUIRE(frames >= 0 && v >= 0 && w >= 0 && h >= 0, "g4d_render_project_f32: negative size");
    if (const int rc = check_image("g4d_render_project_f32", w, h, ss)) return rc;
    G4D_REQUIRE(near > 0.f && half_angle_deg > 0.f && half_angle_deg < 90.f,
                "g4d_render_project_f32: needs near > 0 and a half viewing angle in (0, 90) degrees (near=%g, angle=%g)", (double)near,
                (double)half_angle_deg);
    const double e[3] = {eye_x, eye_y, eye_z}, u[3] = {up_x, up_y, up_z};
    double z[3] = {(double)at_x - e[0], (double)at_y - e[1], (double)at_z - e[2]}, x[3], y[3];
    auto cross = [](const double *a, const double *b, double *o) {
        o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
    };
    auto unit = [](double *a) {
        const double n = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
        if (!(n > 0.0) || !(n < INFINITY)) return false;
        a[0] = a[0] / n; a[1] = a[1] / n; a[2] = a[2] / n;
        return true;
    };
    G4D_REQUIRE(unit(z), "g4d_render_project_f32: eye and at coincide (or are not finite)");
    cross(u, z, x);
    G4D_REQUIRE(unit(x), "g4d_render_project_f32: up is parallel to the viewing direction (or not finite)");
    cross(z, x, y);
    G4D_REQUIRE(unit(y), "g4d_render_project_f32: degenerate camera basis");
    if (frames == 0 || v == 0 || w == 0 || h == 0) return G4D_OK;
    G4D_REQUIRE(verts && px && py && invz, "g4d_render_project_f32: null pointer");
    Camera cm;
    for (int k = 0; k < 3; ++k) {
        cm.r[k] = (float)x[k]; cm.r[3 + k] = (float)y[k]; cm.r[6 + k] = (float)z[k];
        cm.eye[k] = (float)e[k];
    }
    cm.s = (float)(1.0 / tan((double)half_angle_deg * (3.14159265358979323846 / 180.0)));
    cm.hh = 128.f * (float)(ss * h);
    cm.hw = 128.f * (float)(ss * w);
    cm.near = near;
    const long long total = (long long)frames * v;
    G4D_REQUIRE((total + 255) / 256 < (1ll << 31), "g4d_render_project_f32: too large");
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), total, v,
                       shared_verts != 0, cm, verts, px, py, invz, cam);
    return check_launch("g4d_render_project_f32");
}

extern "C" int g4d_render_raster(int frames, int v, int nf, int w, int h, int ss, int cull, const int *px, const int *py, const float *invz,
                                 const float *cam, const int *faces, const int *faces_host, const float *face_rgb, const float *vert_rgb, float light_x,
                                 float light_y, float light_z, float ambient, float directional, float bg_r, float bg_g, float bg_b, void *ws,
                                 size_t ws_bytes, int *face_id, float *depth, float *image, int *kept, g4d_stream_t stream) {
    G4D_REQUIRE(frames >= 0 && v >= 0 && nf >= 0 && w >= 0 && h >= 0, "g4d_render_raster: negative size");
    if (const int rc = check_image("g4d_render_raster", w, h, ss)) return rc;
    G4D_REQUIRE(!(face_rgb && vert_rgb), "g4d_render_raster: give per-face or per-vertex colours, not both");
    if (faces_host)
        for (long long k = 0; k < (long long)nf * 3; ++k)
            G4D_REQUIRE(faces_host[k] >= 0 && faces_host[k] < v, "g4d_render_raster: face index %d of face %lld is outside [0, %d)", faces_host[k],
                        k / 3, v);
    if (frames == 0 || w == 0 || h == 0) return G4D_OK;
    G4D_REQUIRE(face_id && depth, "g4d_render_raster: null pointer");
    G4D_REQUIRE(nf == 0 || (px && py && invz && faces && ws), "g4d_render_raster: null pointer");
    G4D_REQUIRE(nf == 0 || ws_bytes >= g4d_render_ws_bytes(frames, nf), "g4d_render_raster: workspace of %zu bytes, %zu needed", ws_bytes,
                g4d_render_ws_bytes(frames, nf));
    G4D_REQUIRE(nf == 0 || ((uintptr_t)ws & 15) == 0, "g4d_render_raster: workspace must be 16-byte aligned");
    const int ws_ = ss * w, hs_ = ss * h;
    const long long tiles = (long long)((ws_ + kTile - 1) / kTile) * ((hs_ + kTile - 1) / kTile);
    const int nchunks = (nf + kChunk - 1) / kChunk;
    G4D_REQUIRE(tiles * frames < (1ll << 31) && (long long)frames * nchunks < (1ll << 31), "g4d_render_raster: too large");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Shading sh = {{light_x, light_y, light_z}, ambient, directional, {bg_r, bg_g, bg_b}};
    short *boxes = reinterpret_cast<short *>(ws);
    short *chunk_boxes = reinterpret_cast<short *>(reinterpret_cast<char *>(ws) + box_bytes(frames, nf));
    FaceRec *recs = reinterpret_cast<FaceRec *>(reinterpret_cast<char *>(ws) + box_bytes(frames, nf) + chunk_box_bytes(frames, nf));
    if (nf > 0) {
        hipLaunchKernelGGL(setup_kernel, dim3((unsigned)(frames * nchunks)), dim3(kChunk), 0, st, v, nf, nchunks, sh, px, py, invz, cam, faces, boxes,
                           chunk_boxes, recs);
        if (const int rc = check_launch("g4d_render_raster (setup)")) return rc;
    }
    hipLaunchKernelGGL(tile_kernel, dim3((unsigned)(tiles * frames)), dim3(kRThreads), 0, st, frames, nf, ws_, hs_, w, h, ss, cull != 0, sh, boxes, chunk_boxes, recs,
                       face_rgb,
                       vert_rgb, face_id, depth, image, kept);
    return check_launch("g4d_render_raster");
}
