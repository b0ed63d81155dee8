// Virtual depth-sensor scans (include/g4d_scan.h is the contract; tests/scan_twin.py restates it in numpy): the face ids the rasterizer wrote,
// from one or several cameras, become exactly N labelled world-space points per frame.  Three launches, no hit list:
//   count_kernel   : one workgroup per (frame, chunk of kChunk samples), lanes on samples, kPerLane = 4 samples per lane.  A segment is 64 consecutive
//                    samples, one per lane of a wave: its hits are one ballot + popcount.  The four waves' counts meet in LDS -> one count per chunk.
//   offsets_kernel : one workgroup per frame: exclusive scan of the frame's chunk counts, 256 at a time in ascending order with a running
//                    carry (integers: exact in any order) -> one offset per chunk, and count[f] = M_f.
//   select_kernel  : the count launch's grid again.  A hit's rank = chunk offset + hits of the segments before its own + hits of the lanes
//                    before it in its ballot.  From the rank alone the hit decides whether and where it writes (the header's per-hit rule), and
//                    only then unprojects: N points per frame pay for the fetches and divisions, not cams * h * w samples.
// A workgroup of 256 lanes with four samples each instead of 1024 lanes with one: the same 16 ballots per chunk, a quarter of the lanes at
// the barrier, four independent face_id loads in flight per lane.  No atomics: a point is written by the one hit that owns it.
#include "../g4d_common.h"
#include "../../../include/g4d_render.h"
#include "../../../include/g4d_scan.h"

#include <math.h>

namespace g4d {

constexpr int kSThreads = 256, kSWaves = kSThreads / kWave, kSegs = 16, kPerLane = kSegs / kSWaves, kChunk = kSegs * kWave;
constexpr int kCoordLimit = 1 << G4D_RENDER_COORD_BITS;
static_assert(kSegs % kSWaves == 0 && kChunk == kPerLane * kSThreads, "a chunk is kPerLane passes of the workgroup over consecutive samples");

struct ScanShape {
    int frames, cams, v, nf, w, h, nchunks;   // nchunks: chunks per frame
    long long samples;                        // cams * h * w, < 2^31
};

// face id of sample s of frame f (-1 past the end); s = (c * h + i) * w + j, face_id is (cams, frames, h, w)
__device__ __forceinline__ int sample_face(const ScanShape &sh, const int *__restrict__ face_id, int f, long long s) {
    if (s >= sh.samples) return -1;
    const long long hw = (long long)sh.h * sh.w;
    const long long c = s / hw;
    return face_id[((size_t)c * sh.frames + f) * (size_t)hw + (size_t)(s - c * hw)];
}

// The ballots of this wave's kPerLane segments (segment q * kSWaves + wave: samples chunk base + q * kSThreads + t), and this lane's face ids.
__device__ __forceinline__ void chunk_ballots(const ScanShape &sh, const int *__restrict__ face_id, int f, int chunk, int id[kPerLane],
                                              unsigned long long mask[kPerLane]) {
    const long long base = (long long)chunk * kChunk + threadIdx.x;
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) id[q] = sample_face(sh, face_id, f, base + q * kSThreads);
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) mask[q] = __ballot((unsigned)id[q] < (unsigned)sh.nf);
}

__global__ void __launch_bounds__(kSThreads) count_kernel(ScanShape sh, const int *__restrict__ face_id, int *__restrict__ counts) {
    __shared__ int s_cnt[kSWaves];
    const int f = blockIdx.x / sh.nchunks, chunk = blockIdx.x - f * sh.nchunks;
    int id[kPerLane];
    unsigned long long mask[kPerLane];
    chunk_ballots(sh, face_id, f, chunk, id, mask);
    int n = 0;
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) n += __popcll(mask[q]);
    if ((threadIdx.x & (kWave - 1)) == 0) s_cnt[threadIdx.x / kWave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int wv = 0; wv < kSWaves; ++wv) total += s_cnt[wv];
        counts[blockIdx.x] = total;
    }
}

__global__ void __launch_bounds__(kSThreads) offsets_kernel(int nchunks, const int *__restrict__ counts, int *__restrict__ offsets, int *__restrict__ count) {
    __shared__ int s_wave[kSWaves];
    const int f = blockIdx.x, t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    const int *in = counts + (size_t)f * nchunks;
    int *out = offsets + (size_t)f * nchunks;
    int carry = 0;   // hits of the chunks before this pass: < 2^31 like the samples
    for (int c0 = 0; c0 < nchunks; c0 += kSThreads) {
        const int mine = c0 + t < nchunks ? in[c0 + t] : 0;
        int incl = mine;   // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int up = __shfl_up(incl, d);
            incl += lane >= d ? up : 0;
        }
        if (lane == kWave - 1) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, pass = 0;
        for (int wv = 0; wv < kSWaves; ++wv) {
            before += wv < wave ? s_wave[wv] : 0;
            pass += s_wave[wv];
        }
        if (c0 + t < nchunks) out[c0 + t] = carry + before + incl - mine;
        carry += pass;
        __syncthreads();   // s_wave is free again
    }
    if (t == 0) count[f] = carry;
}

__device__ __forceinline__ unsigned mix(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

struct ScanOut {
    float *points;
    int *labels, *face, *sample;
};

__device__ __forceinline__ void write_point(const ScanOut &o, size_t at, float x, float y, float z, int label, int face, int sample) {
    o.points[at * 3] = x; o.points[at * 3 + 1] = y; o.points[at * 3 + 2] = z;
    o.labels[at] = label; o.face[at] = face; o.sample[at] = sample;
}

__global__ void __launch_bounds__(kSThreads) select_kernel(ScanShape sh, int n_points, unsigned seed, const int *__restrict__ px, const int *__restrict__ py,
                                                           const float *__restrict__ invz, const int *__restrict__ face_id, const float *__restrict__ verts,
                                                           const int *__restrict__ faces, const int *__restrict__ face_labels,
                                                           const int *__restrict__ offsets, const int *__restrict__ count, ScanOut o) {
    __shared__ int s_cnt[kSegs];
    const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    const int f = blockIdx.x / sh.nchunks, chunk = blockIdx.x - f * sh.nchunks;
    const long long M = count[f], N = n_points;
    if (M == 0) {   // nothing seen in this frame: its chunks share the fill
        for (long long j = (long long)chunk * kSThreads + t; j < N; j += (long long)sh.nchunks * kSThreads) write_point(o, (size_t)f * N + j, 0.f, 0.f, 0.f, -1, -1, -1);
        return;
    }
    int id[kPerLane];
    unsigned long long mask[kPerLane];
    chunk_ballots(sh, face_id, f, chunk, id, mask);
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < kPerLane; ++q) s_cnt[q * kSWaves + wave] = __popcll(mask[q]);
    __syncthreads();
    const long long first = offsets[blockIdx.x];
    const unsigned fkey = mix(mix(seed) ^ (unsigned)f);
    const long long hw = (long long)sh.h * sh.w;
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
        if (!((mask[q] >> lane) & 1)) continue;
        const int seg = q * kSWaves + wave;
        long long r = first + __popcll(mask[q] & ((1ull << lane) - 1ull));
        for (int g = 0; g < seg; ++g) r += s_cnt[g];
        // the per-hit rule: where this hit writes, j0, j0 + step, ... < N (nowhere: j0 = N)
        long long j0 = r, step = M;
        if (M >= N) {
            j0 = ((r + 1) * N - 1) / M;
            const long long lo = j0 * M / N, hi = (j0 + 1) * M / N;
            if (lo + (long long)(mix(fkey ^ (unsigned)j0) % (unsigned long long)(hi - lo)) != r) j0 = N;
            step = N;
        }
        if (j0 >= N) continue;
        const long long s = (long long)chunk * kChunk + q * kSThreads + t;
        const long long c = s / hw, rest = s - c * hw;
        const int i = (int)(rest / sh.w), j = (int)(rest - (long long)i * sh.w);
        const int face = id[q];
        float p[3] = {0.f, 0.f, 0.f};
        int label = -1, face_out = -1, sample_out = -1;
        int vid[3];
        for (int e = 0; e < 3; ++e) vid[e] = faces[(size_t)face * 3 + e];
        bool ok = (unsigned)vid[0] < (unsigned)sh.v && (unsigned)vid[1] < (unsigned)sh.v && (unsigned)vid[2] < (unsigned)sh.v;
        if (ok) {
            const size_t base = ((size_t)c * sh.frames + f) * sh.v;
            long long x[3], y[3];
            float iz[3];
            for (int e = 0; e < 3; ++e) {
                x[e] = px[base + vid[e]]; y[e] = py[base + vid[e]]; iz[e] = invz[base + vid[e]];
                ok = ok && iz[e] > 0.f && iz[e] < INFINITY && x[e] > -kCoordLimit && x[e] < kCoordLimit && y[e] > -kCoordLimit && y[e] < kCoordLimit;
            }
            long long area2 = ok ? (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0]) : 0;
            if (area2 < 0) {
                long long lt = x[1]; x[1] = x[2]; x[2] = lt;
                lt = y[1]; y[1] = y[2]; y[2] = lt;
                const int it = vid[1]; vid[1] = vid[2]; vid[2] = it;
                const float ft = iz[1]; iz[1] = iz[2]; iz[2] = ft;
                area2 = -area2;
            }
            if (area2 > 0) {
                const long long sx = 256ll * j + 128, sy = 256ll * i + 128;
                const float a2 = (float)area2;
                float b[3], wgt[3];
                for (int e = 0; e < 3; ++e) {
                    const int pp = (e + 1) % 3, qq = (e + 2) % 3;
                    const long long E = (x[qq] - x[pp]) * (sy - y[pp]) - (y[qq] - y[pp]) * (sx - x[pp]);
                    b[e] = (float)E / a2;
                    wgt[e] = b[e] * iz[e];
                }
                const float izs = (iz[0] + b[1] * (iz[1] - iz[0])) + b[2] * (iz[2] - iz[0]);
                const float *v0 = verts + ((size_t)f * sh.v + vid[0]) * 3, *v1 = verts + ((size_t)f * sh.v + vid[1]) * 3,
                            *v2 = verts + ((size_t)f * sh.v + vid[2]) * 3;
                for (int k = 0; k < 3; ++k) p[k] = ((wgt[0] * v0[k] + wgt[1] * v1[k]) + wgt[2] * v2[k]) / izs;
                label = face_labels ? face_labels[face] : 0;
                face_out = face;
                sample_out = (int)s;
            }
        }
        for (long long jj = j0; jj < N; jj += step) write_point(o, (size_t)f * N + jj, p[0], p[1], p[2], label, face_out, sample_out);
    }
}

}  // namespace g4d

using namespace g4d;

extern "C" int g4d_scan_chunk(void) { return kChunk; }

extern "C" size_t g4d_scan_ws_bytes(int frames, int cams, int w, int h) {
    if (frames < 0 || cams < 0 || w < 0 || h < 0) return (size_t)-1;
    if (frames == 0 || cams == 0 || w == 0 || h == 0) return 0;
    const long long rays = (long long)w * h;   // < 2^62; times cams only once it is known to be < 2^31
    if (rays >= (1ll << 31) || rays * cams >= (1ll << 31)) return (size_t)-1;
    return (size_t)frames * (size_t)((rays * cams + kChunk - 1) / kChunk) * 8;
}

extern "C" int g4d_scan_points_f32(int frames, int cams, int v, int nf, int w, int h, const int *px, const int *py, const float *invz, const int *face_id,
                                   const float *verts, const int *faces, const int *face_labels, int n_points, unsigned seed, void *ws, size_t ws_bytes,
                                   float *points, int *labels, int *face, int *sample, int *count, g4d_stream_t stream) {
    G4D_REQUIRE(frames >= 0 && v >= 0 && nf >= 0 && w >= 0 && h >= 0, "g4d_scan_points_f32: negative size");
    G4D_REQUIRE(n_points >= 0, "g4d_scan_points_f32: negative n_points (%d)", n_points);
    G4D_REQUIRE(cams >= 1 && cams <= G4D_SCAN_MAX_CAMS, "g4d_scan_points_f32: cams must be in [1, %d] (cams=%d)", G4D_SCAN_MAX_CAMS, cams);
    G4D_REQUIRE(w <= G4D_SCAN_MAX_SIDE && h <= G4D_SCAN_MAX_SIDE, "g4d_scan_points_f32: w and h must be <= %d (w=%d, h=%d)", G4D_SCAN_MAX_SIDE, w, h);
    const long long samples = (long long)cams * h * w;   // <= 2^33 within the limits above
    G4D_REQUIRE(samples < (1ll << 31), "g4d_scan_points_f32: cams * h * w must be < 2^31 (cams=%d, w=%d, h=%d)", cams, w, h);
    if (frames == 0 || w == 0 || h == 0 || n_points == 0) return G4D_OK;
    G4D_REQUIRE(px && py && invz && face_id && verts && faces && ws && points && labels && face && sample && count, "g4d_scan_points_f32: null pointer");
    const size_t need = g4d_scan_ws_bytes(frames, cams, w, h);
    G4D_REQUIRE(ws_bytes >= need, "g4d_scan_points_f32: workspace of %zu bytes, %zu needed", ws_bytes, need);
    G4D_REQUIRE(((uintptr_t)ws & 15) == 0, "g4d_scan_points_f32: workspace must be 16-byte aligned");
    const long long nchunks = (samples + kChunk - 1) / kChunk;
    G4D_REQUIRE(nchunks * frames < (1ll << 31), "g4d_scan_points_f32: too large (frames * chunks >= 2^31)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const ScanShape sh = {frames, cams, v, nf, w, h, (int)nchunks, samples};
    int *counts = reinterpret_cast<int *>(ws), *offsets = counts + (size_t)frames * nchunks;
    const unsigned grid = (unsigned)(nchunks * frames);
    hipLaunchKernelGGL(count_kernel, dim3(grid), dim3(kSThreads), 0, st, sh, face_id, counts);
    if (const int rc = check_launch("g4d_scan_points_f32 (count)")) return rc;
    hipLaunchKernelGGL(offsets_kernel, dim3((unsigned)frames), dim3(kSThreads), 0, st, (int)nchunks, counts, offsets, count);
    if (const int rc = check_launch("g4d_scan_points_f32 (offsets)")) return rc;
    const ScanOut o = {points, labels, face, sample};
    hipLaunchKernelGGL(select_kernel, dim3(grid), dim3(kSThreads), 0, st, sh, n_points, seed, px, py, invz, face_id, verts, faces, face_labels, offsets, count, o);
    return check_launch("g4d_scan_points_f32");
}
