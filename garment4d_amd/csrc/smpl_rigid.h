// The per-joint routines of SMPL's rigid part that more than one file needs (lbs.hip: the forward; smpl/smpl_grad.hip: its adjoint).
//   rodrigues()       lbs.py:312-346, the reference's exact formula
//   wave_sync_lds()   a wave exchanging values with itself through LDS
//   rigid_wave()      one wave, one frame: rotations, joints from betas, local transforms and the kinematic chain, left in LDS.  lbs.hip's
//                     kernels keep their own inline copies of this step (they interleave it with their loads and operand stores); this is
//                     the same sequence of operations as a function, for the adjoint's two per-frame kernels.
#pragma once
#include "g4d_common.h"

namespace g4d {

// lbs.py:312-346  batch_rodrigues: angle = ||r + 1e-8||, dir = r / angle, R = I + sin K + (1 - cos) K K
__device__ __forceinline__ void rodrigues(float rx, float ry, float rz, float *R) {
    const float ax = rx + 1e-8f, ay = ry + 1e-8f, az = rz + 1e-8f;
    const float angle = __fsqrt_rn(ax * ax + ay * ay + az * az);
    const float x = rx / angle, y = ry / angle, z = rz / angle;
    const float s = sinf(angle), c1 = 1.0f - cosf(angle);
    // K = [[0,-z,y],[z,0,-x],[-y,x,0]];  K K = [[-(y2+z2), xy, xz],[xy, -(x2+z2), yz],[xz, yz, -(x2+y2)]]
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z;
    R[0] = 1.0f + c1 * (-(zz + yy));  // row-major 3x3; K K[0][0] = -z*z - y*y (bmm order: (-z)(z) + (y)(-y))
    R[1] = s * (-z) + c1 * xy;
    R[2] = s * y + c1 * xz;
    R[3] = s * z + c1 * xy;
    R[4] = 1.0f + c1 * (-(zz + xx));
    R[5] = s * (-x) + c1 * yz;
    R[6] = s * (-y) + c1 * xz;
    R[7] = s * x + c1 * yz;
    R[8] = 1.0f + c1 * (-(yy + xx));
}

__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// parent of joint i >= 1, kept inside [0, i): a malformed table reads no LDS but the wave's own
__device__ __forceinline__ int chain_parent(const int *__restrict__ parents, int i) { return min(max(parents[i], 0), max(i - 1, 0)); }

// One wave (lane l), frame b, J <= 32 joints whose parents precede them.  On return, visible to the whole wave:
//   R_[j][9] rotations, J_[j][3] rest joints (Jt + Js betas), L_[j][12] local transforms [R | J - J_parent], G_[j][12] chain transforms
//   (lbs.py:362-405; G_[j][3,7,11] are the posed joints).  The arrays are the wave's own LDS.
__device__ __forceinline__ void rigid_wave(int l, int b, int J, int NB, int pose2rot, const float *__restrict__ betas, int betas_bstride,
                                           const float *__restrict__ pose, const float *__restrict__ Jt, const float *__restrict__ Js,
                                           const int *__restrict__ parents, float *R_, float *J_, float *L_, float *G_) {
    if (l < J) {
        float R[9];
        if (pose2rot) {
            const float *pp = pose + ((size_t)b * J + l) * 3;
            rodrigues(pp[0], pp[1], pp[2], R);
        } else {
            const float *pp = pose + ((size_t)b * J + l) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = pp[k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) R_[l * 9 + k] = R[k];
        const float *be = betas + (size_t)b * betas_bstride;
#pragma unroll
        for (int r = 0; r < 3; ++r) {   // J_regressor (v_template + shapedirs beta) = Jt + Js beta  (lbs.py:209 through two model constants)
            float acc = Jt[l * 3 + r];
            for (int k = 0; k < NB; ++k) acc = fmaf(Js[(l * 3 + r) * NB + k], be[k], acc);
            J_[l * 3 + r] = acc;
        }
    }
    wave_sync_lds();
    if (l < J) {  // local transform [R | J - J_parent]  (lbs.py:390-396)
        const int p = chain_parent(parents, l);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            L_[l * 12 + r * 4 + 0] = R_[l * 9 + r * 3 + 0];
            L_[l * 12 + r * 4 + 1] = R_[l * 9 + r * 3 + 1];
            L_[l * 12 + r * 4 + 2] = R_[l * 9 + r * 3 + 2];
            L_[l * 12 + r * 4 + 3] = (l > 0) ? (J_[l * 3 + r] - J_[p * 3 + r]) : J_[l * 3 + r];
        }
    }
    wave_sync_lds();
    if (l < 12) G_[l] = L_[l];
    wave_sync_lds();
    for (int i = 1; i < J; ++i) {  // G_i = G_parent(i) . L_i   (lbs.py:399-405), 4x4 product with implicit [0 0 0 1]
        if (l < 12) {
            const int p = chain_parent(parents, i), r = l >> 2, c = l & 3;
            float acc = G_[p * 12 + r * 4 + 0] * L_[i * 12 + 0 * 4 + c];
            acc = fmaf(G_[p * 12 + r * 4 + 1], L_[i * 12 + 1 * 4 + c], acc);
            acc = fmaf(G_[p * 12 + r * 4 + 2], L_[i * 12 + 2 * 4 + c], acc);
            if (c == 3) acc += G_[p * 12 + r * 4 + 3];
            G_[i * 12 + l] = acc;
        }
        wave_sync_lds();
    }
}

}  // namespace g4d
