// Resampling jumps of a known-region call (RePaint, Lugmayr et al. 2022, section 4.2 and algorithm 1): the reverse loop walks a
// table of entries, most of them ordinary sampler steps down the schedule, some of them jumps back UP it.  wd_forward_jump is
// the up entry: it diffuses the whole state forward from the level it is at to a higher one.  wd_walk_randn fills the noise a
// down entry reads (the step's z, the blend's z) so that every VISIT of a level has draws of its own: both kernels key their
// Philox draws by the walk index k, not by the timestep.
#include "wd_common.h"
#include "wd_philox.h"

// The jump is compared bit for bit with its numpy specification (tests/_resample_ref.py): both products and the sum are rounded
// to fp32 on their own - no mul+add contraction anywhere in this translation unit (plain operators, as in wd_misc.hip).
#pragma clang fp contract(off)

namespace {

inline int walk_grid(long total) {
    long g = (total + 255) / 256;
    if (g < 1) g = 1;
    return (int)(g < 2048 ? g : 2048);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the tag of draw `which` of walk entry k: top two bits set, which in bits 26-27, k below them
__device__ __forceinline__ uint32_t walk_tag(int which, int k) {
    return (uint32_t)WD_TAG_WALK | ((uint32_t)which << 26) | ((uint32_t)k & 0x03ffffffu);
}

// x = g1[k] * x + g2[k] * z on the walk index k = *k_dev; z from ``noise`` or the walk's own draw WD_WALK_JUMP of entry k
__global__ void forward_jump_kernel(float* __restrict__ x, int batch, int n4, const float* __restrict__ g1,
                                    const float* __restrict__ g2, const int32_t* __restrict__ k_dev, const float* __restrict__ noise,
                                    uint64_t seed, uint64_t sample_offset) {
    int k = *k_dev;
    if (k < 0) k = 0;  // the tables begin at entry 0
    const float a = g1[k], s = g2[k];
    const uint32_t tag = walk_tag(WD_WALK_JUMP, k);
    const long total = (long)batch * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        float4 z;
        if (noise) z = reinterpret_cast<const float4*>(noise)[i];
        else {
            const int b = (int)(i / n4);
            z = philox_normal4(seed, sample_offset + (uint64_t)b, tag, (uint32_t)(i - (long)b * n4));
        }
        const float4 xv = reinterpret_cast<const float4*>(x)[i];
        float4 o;
        o.x = a * xv.x + s * z.x;
        o.y = a * xv.y + s * z.y;
        o.z = a * xv.z + s * z.z;
        o.w = a * xv.w + s * z.w;
        reinterpret_cast<float4*>(x)[i] = o;
    }
}

// randn_kernel under the walk's tag: draw `which` of entry k = *k_dev
__global__ void walk_randn_kernel(float* __restrict__ out, int batch, int n4, uint64_t seed, uint64_t sample_offset, int which,
                                  const int32_t* __restrict__ k_dev) {
    int k = *k_dev;
    if (k < 0) k = 0;
    const uint32_t tag = walk_tag(which, k);
    const long total = (long)batch * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / n4);
        reinterpret_cast<float4*>(out)[i] = philox_normal4(seed, sample_offset + (uint64_t)b, tag, (uint32_t)(i - (long)b * n4));
    }
}

}  // namespace

extern "C" int wd_forward_jump(float* x, int batch, int n_per_sample, const float* g1, const float* g2, const int32_t* k_dev,
                               const float* noise, uint64_t seed, uint64_t sample_offset, void* stream) {
    if (!x || !g1 || !g2 || !k_dev || batch <= 0 || n_per_sample <= 0 || n_per_sample % 4) return WD_EINVAL;
    if (!aligned16(x) || !aligned16(noise)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(forward_jump_kernel, dim3(walk_grid((long)batch * (n_per_sample / 4))), dim3(256), 0, st, x, batch,
                       n_per_sample / 4, g1, g2, k_dev, noise, seed, sample_offset);
    return wd_check_launch();
}

extern "C" int wd_walk_randn(float* out, int batch, int n_per_sample, uint64_t seed, uint64_t sample_offset, int which,
                             const int32_t* k_dev, void* stream) {
    if (!out || !k_dev || batch <= 0 || n_per_sample <= 0 || n_per_sample % 4 || which < 0 || which > WD_WALK_JUMP) return WD_EINVAL;
    if (!aligned16(out)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(walk_randn_kernel, dim3(walk_grid((long)batch * (n_per_sample / 4))), dim3(256), 0, st, out, batch,
                       n_per_sample / 4, seed, sample_offset, which, k_dev);
    return wd_check_launch();
}
