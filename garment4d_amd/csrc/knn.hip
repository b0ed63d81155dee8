// K nearest neighbours (K <= 256) for the garment skinning of the model around the hot path: the reference calls
// `chamferdist.knn_points(garment_verts, body_verts, K=256 / 64 / 1)` (modules/mesh_encoder.py:321-324;
// chamferdist is an un-vendored dependency, README.md:26, wrapping pytorch3d's KNN: squared L2 distances, the K
// smallest per query, sorted ascending).  Defined here as: the K smallest under (distance, index) lexicographic order,
// distance = ((dx*dx) + dy*dy) + dz*dz in fp32 without fma.  PARITY UNPINNED (the dependency is absent; its tie order
// is implementation-defined), checked against a numpy restatement.
//
// One workgroup (256 threads) per query: distances of all P2 points go to LDS as order-preserving uint32 keys, a 4-pass
// MSB radix select (LDS histogram + wave scan) finds the K-th smallest distance, the points below it plus the
// lowest-index ties are compacted to exactly K 64-bit (distance, index) keys, and a bitonic sort of <= 256 keys puts
// them in order.  ~113 M distance evaluations for 4 x 4096 queries against 6890 points: the selection, not the
// distances, is the work, and it never leaves LDS.
#include "g4d_common.h"

namespace g4d {

constexpr int kKnnMaxK = 256;

// exclusive prefix over 256 histogram bins by one wave (4 bins per lane), returns via LDS arrays
__device__ __forceinline__ void knn_find_bin(const unsigned *hist, unsigned kth, unsigned *out_bin, unsigned *out_before) {
    // called by wave 0 only; lane l owns bins 4l..4l+3
    const int lane = threadIdx.x & 63;
    const unsigned h0 = hist[lane * 4 + 0], h1 = hist[lane * 4 + 1], h2 = hist[lane * 4 + 2], h3 = hist[lane * 4 + 3];
    const unsigned mine = h0 + h1 + h2 + h3;
    unsigned incl = mine;  // inclusive scan over lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    const unsigned excl = incl - mine;
    // the lane whose range [excl, incl) contains kth (0-based rank kth)
    if (kth >= excl && kth < incl) {
        unsigned before = excl;
        int b = 0;
        if (kth >= before + h0) { before += h0; b = 1;
            if (kth >= before + h1) { before += h1; b = 2;
                if (kth >= before + h2) { before += h2; b = 3; } } }
        *out_bin = (unsigned)(lane * 4 + b);
        *out_before = before;
    }
}

template <int FM>
__global__ void __launch_bounds__(256) knn_kernel(int p1, int p2, int K, const float *__restrict__ q_all, const float *__restrict__ x_all,
                                                 float *__restrict__ dist_all, int *__restrict__ idx_all) {
    extern __shared__ __attribute__((aligned(16))) unsigned smem_u[];
    unsigned *dk = smem_u;                                   // [p2] distance keys
    unsigned *hist = dk + ((p2 + 3) & ~3);                   // [256]
    unsigned *ctl = hist + 256;                              // [8] bin, before, counters
    unsigned long long *list = reinterpret_cast<unsigned long long *>(ctl + 8);  // [256] selected keys

    const int t = threadIdx.x;
    const int b = blockIdx.y, q = blockIdx.x;
    const float *x = x_all + (size_t)b * p2 * 3;
    const float *qp = q_all + ((size_t)b * p1 + q) * 3;
    const float qx = qp[0], qy = qp[1], qz = qp[2];

    for (int k = t; k < p2; k += 256) {
        const float dx = qx - x[k * 3 + 0], dy = qy - x[k * 3 + 1], dz = qz - x[k * 3 + 2];
        const float d = dist2<FM>(dx, dy, dz);  // >= +0: the bit pattern orders like the value.  chamferdist / pytorch3d accumulate
                                                // `dist += diff * diff` over the 3 axes: nvcc contracts that loop to the chain shape (FM = 2)
        dk[k] = __float_as_uint(d);
    }
    // ---- radix select: value of the (K-1)-th smallest key (0-based), 8 bits per pass, MSB first
    unsigned prefix = 0, pmask = 0, kth = (unsigned)(K - 1);
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[t] = 0;
        __syncthreads();
        for (int k = t; k < p2; k += 256) {
            const unsigned v = dk[k];
            if ((v & pmask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (t < 64) knn_find_bin(hist, kth, &ctl[0], &ctl[1]);
        __syncthreads();
        prefix |= ctl[0] << shift;
        pmask |= 255u << shift;
        kth -= ctl[1];
        __syncthreads();
    }
    const unsigned thr = prefix;  // K-th smallest distance (bit pattern); kth = rank among the ties that is still needed
    const unsigned need_ties = kth + 1;
    // ---- compact: everything below thr, plus the `need_ties` lowest-index points AT thr
    if (t == 0) { ctl[2] = 0; ctl[3] = 0; }
    __syncthreads();
    // ties first: find the index threshold when there are more ties than needed (rare: exact duplicates of the K-th distance)
    unsigned tie_idx_limit = 0xffffffffu;
    {
        unsigned local = 0;
        for (int k = t; k < p2; k += 256) local += (dk[k] == thr) ? 1u : 0u;
        atomicAdd(&ctl[3], local);
        __syncthreads();
        const unsigned nties = ctl[3];
        __syncthreads();
        if (nties > need_ties) {
            // radix select on the INDEX among the ties: the (need_ties-1)-th smallest index
            unsigned ip = 0, im = 0, ik = need_ties - 1;
            for (int shift = 24; shift >= 0; shift -= 8) {
                hist[t] = 0;
                __syncthreads();
                for (int k = t; k < p2; k += 256)
                    if (dk[k] == thr && ((unsigned)k & im) == ip) atomicAdd(&hist[((unsigned)k >> shift) & 255u], 1u);
                __syncthreads();
                if (t < 64) knn_find_bin(hist, ik, &ctl[0], &ctl[1]);
                __syncthreads();
                ip |= ctl[0] << shift;
                im |= 255u << shift;
                ik -= ctl[1];
                __syncthreads();
            }
            tie_idx_limit = ip;
        }
    }
    for (int k = t; k < p2; k += 256) {
        const unsigned v = dk[k];
        if (v < thr || (v == thr && (unsigned)k <= tie_idx_limit)) {
            const unsigned slot = atomicAdd(&ctl[2], 1u);
            if (slot < (unsigned)kKnnMaxK) list[slot] = ((unsigned long long)v << 32) | (unsigned)k;
        }
    }
    __syncthreads();
    const int cnt = (int)ctl[2];  // == K by construction
    for (int i = cnt + t; i < kKnnMaxK; i += 256) list[i] = ~0ull;  // padding sorts last
    __syncthreads();
    // ---- bitonic sort of 256 64-bit keys (distance, index): 128 compare-exchanges per stage
    for (int kk = 2; kk <= kKnnMaxK; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            if (t < kKnnMaxK / 2) {
                const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int c = a | j;
                const unsigned long long ka = list[a], kc = list[c];
                const bool asc = (a & kk) == 0;
                if ((ka > kc) == asc) { list[a] = kc; list[c] = ka; }
            }
            __syncthreads();
        }
    }
    if (t < K) {
        const unsigned long long key = list[t];
        dist_all[((size_t)b * p1 + q) * K + t] = __uint_as_float((unsigned)(key >> 32));
        idx_all[((size_t)b * p1 + q) * K + t] = (int)(unsigned)key;
    }
}

}  // namespace g4d

extern "C" int g4d_knn_f32(int b, int p1, int p2, int k, const float *queries, const float *points, float *dists, int *idx,
                           g4d_stream_t stream) {
    using namespace g4d;
    G4D_REQUIRE(b >= 0 && p1 >= 0 && p2 >= 0 && k >= 1 && k <= kKnnMaxK, "g4d_knn_f32: need 1 <= K <= %d", kKnnMaxK);
    if (b == 0 || p1 == 0) return G4D_OK;
    G4D_REQUIRE(k <= p2, "g4d_knn_f32: K (%d) > number of points (%d)", k, p2);
    G4D_REQUIRE(queries && points && dists && idx, "g4d_knn_f32: null pointer");
    G4D_REQUIRE(b <= 65535 && p2 <= 32768, "g4d_knn_f32: b <= 65535, p2 <= 32768 (LDS-resident distance keys)");
    const size_t lds = sizeof(unsigned) * (((size_t)p2 + 3) / 4 * 4 + 256 + 8) + sizeof(unsigned long long) * kKnnMaxK;
    if (knn_shape(distance_contraction()) == 0) {
        static unsigned long long attr = 0;  // one bit per device
        if (const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(knn_kernel<0>), 150 * 1024, attr, "g4d_knn_f32")) return rc;
        hipLaunchKernelGGL(knn_kernel<0>, dim3(p1, b), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), p1, p2, k, queries, points, dists, idx);
    } else {
        static unsigned long long attr = 0;
        if (const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(knn_kernel<2>), 150 * 1024, attr, "g4d_knn_f32")) return rc;
        hipLaunchKernelGGL(knn_kernel<2>, dim3(p1, b), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), p1, p2, k, queries, points, dists, idx);
    }
    return check_launch("g4d_knn_f32");
}
