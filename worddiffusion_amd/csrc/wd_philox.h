// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011): the counter-based
// generator behind the noise streams (wd_misc.hip) and the training dropout masks (wd_norm.hip, wd_bwd.hip).
//   counter = (e4, tag, row & 0xffffffff, row >> 32)      key = (seed & 0xffffffff, seed >> 32)
// e4: index of a group of four consecutive elements inside one sample; row: the global sample row; tag: the timestep of the step
// kernels, or 0x80000000 | stream id (include/wdiff_hip.h: WD_STREAM_*).
#pragma once
#include "wd_common.h"

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
    const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n1 = lo1, n2 = hi0 ^ c[3] ^ k1, n3 = lo0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// ---- normal draws: Box-Muller on (0,1] uniforms.  Four N(0,1) values for the elements 4 e4 .. 4 e4 + 3 of sample `sample`
// (wd_misc.hip: the step kernels, wd_randn, the posterior; wd_resample.hip: the walk's draws).  Every uniform and the angle is
// exact or a single fp32 product, and no product here feeds a sum: the bits do not depend on the contraction mode of the file.
__device__ __forceinline__ float4 philox_normal4(uint64_t seed, uint64_t sample, uint32_t tag, uint32_t e4) {
    uint32_t c[4] = {e4, tag, (uint32_t)sample, (uint32_t)(sample >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u0 = ((float)(c[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float u1 = ((float)(c[1] >> 8)) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c[2] >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float u3 = ((float)(c[3] >> 8)) * (1.0f / 16777216.0f);
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
    float s0, c0, s1, c1;
    sincosf(6.283185307179586f * u1, &s0, &c0);
    sincosf(6.283185307179586f * u3, &s1, &c1);
    return make_float4(r0 * c0, r0 * s0, r1 * c1, r1 * s1);
}

// ---- training dropout (wd_dropout): the keep decision of the four consecutive elements idx .. idx + 3 of sample `row`,
// idx = token * c + channel (a multiple of 4): one draw, element idx + k is kept iff word k >= thr.
__device__ __forceinline__ uint64_t wd_dropout_row(const wd_dropout& d, int b) {
    return d.row_base + (d.row_base_dev ? *d.row_base_dev : 0ull) + (uint64_t)b;
}
__device__ __forceinline__ void wd_dropout_keep4(const wd_dropout& d, uint64_t row, int token, int c, int ch, bool (&keep)[4]) {
    uint32_t w[4] = {(uint32_t)(((uint64_t)token * (uint32_t)c + (uint32_t)ch) >> 2), d.tag, (uint32_t)row, (uint32_t)(row >> 32)};
    philox4x32_10(w, (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
#pragma unroll
    for (int k = 0; k < 4; ++k) keep[k] = w[k] >= d.thr;
}
// a kernel template takes `const D... d` with D empty (the plain form: same signature, same code as without the feature) or one
// wd_dropout; this hands the body the one there is
struct wd_no_dropout {};
__device__ __forceinline__ wd_no_dropout wd_dropout_of() { return {}; }
__device__ __forceinline__ const wd_dropout& wd_dropout_of(const wd_dropout& d) { return d; }
// keep ? fp32(v * scale) : 0 - the product is rounded on its own: parsed with contraction off, it carries no `contract` flag and
// cannot fuse into an add that follows once inlined (the __fmul_rn intrinsic is an inline function parsed with contraction allowed)
__device__ __forceinline__ float wd_dropout_apply(bool keep, float v, float scale) {
#pragma clang fp contract(off)
    const float p = v * scale;
    return keep ? p : 0.0f;
}
