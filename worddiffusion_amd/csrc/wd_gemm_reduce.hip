// Tap-gather GEMM: the split-K combine launch behind wd_gemm_launch_reduce (wd_gemm_priv.h), for every kernel that cuts K across
// workgroups without tickets (wd_gemm.hip, wd_gemm4.hip, wd_gemmw.hip, wd_gemm_exp.hip).
#include "wd_common.h"
#include "wd_gemm_epi.h"
#include "wd_gemm_priv.h"

namespace {

// out = epilogue(sum of the ksplit partial slabs): one workgroup per BM x BN tile sums the slabs in a fixed order into
// the same fp32 LDS image the in-kernel epilogue uses and then runs that epilogue (statistics included).
template <int BM, int BN>
__global__ void __launch_bounds__(256) wd_gemm_reduce_kernel(const wd_gemm_args a, const int nbn) {
    constexpr int LDE = BN + 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* ep = reinterpret_cast<float*>(smem);
    const int bn_i = blockIdx.x % nbn, bm_i = blockIdx.x / nbn;
    const int m0 = bm_i * BM, n0 = bn_i * BN;
    const int tid = threadIdx.x;
    const long total = (long)a.m * a.n;
    const bool v4 = (a.n & 3) == 0;
    if constexpr (BM == 64 && BN == 40) {
        if (a.gn_gamma) {  // (the host has checked shapes and alignment: wd_gemm)
            wd_gn_tile<40, 256, true>(a, nullptr, ep, m0, n0, tid);
            return;
        }
    }
    {
        // the epilogue's vector path can sum the slabs itself (no LDS image, one barrier less, the slab / residual / row-vector
        // loads of a row in flight together); same conditions as its own `vec` test plus aligned slabs
        const bool direct = v4 && wd_epilogue_vec_ok(a) && (reinterpret_cast<uintptr_t>(a.ws) & 15) == 0 && n0 + BN <= a.n;
        if (direct) {
            wd_gemm_args b = a;
            b.ksplit = 1;
            wd_epilogue_from_image<BM, BN, 256, true>(b, ep, m0, n0, tid, a.ksplit);
            return;
        }
    }
    if (v4) {
        // slab-major with all of the thread's elements in flight per slab: the pass is latency-bound otherwise (one
        // workgroup's worth of loads per CU).  Per element the slabs are still summed in ascending order.
        constexpr int NI = (BM * (BN / 4) + 255) / 256;
        float4 v[NI];
        long off[NI];
#pragma unroll
        for (int ii = 0; ii < NI; ++ii) {
            const int i = tid + ii * 256;
            const int row = i / (BN / 4), c = (i - row * (BN / 4)) * 4;
            const int m = m0 + row, n = n0 + c;
            v[ii] = make_float4(0.f, 0.f, 0.f, 0.f);
            off[ii] = (i < BM * (BN / 4) && m < a.m && n < a.n) ? (long)m * a.n + n : -1;
        }
        for (int sp = 0; sp < a.ksplit; ++sp) {
            const float* slab = a.ws + (long)sp * total;
            float4 q[NI];
#pragma unroll
            for (int ii = 0; ii < NI; ++ii)
                q[ii] = off[ii] >= 0 ? *reinterpret_cast<const float4*>(slab + off[ii]) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int ii = 0; ii < NI; ++ii) {
                v[ii].x += q[ii].x; v[ii].y += q[ii].y; v[ii].z += q[ii].z; v[ii].w += q[ii].w;
            }
        }
#pragma unroll
        for (int ii = 0; ii < NI; ++ii) {
            const int i = tid + ii * 256;
            if (i < BM * (BN / 4)) {
                const int row = i / (BN / 4), c = (i - row * (BN / 4)) * 4;
                *reinterpret_cast<float4*>(ep + row * LDE + c) = v[ii];
            }
        }
    } else {
        for (int i = tid; i < BM * (BN / 4); i += 256) {
            const int row = i / (BN / 4), c = (i - row * (BN / 4)) * 4;
            const int m = m0 + row, n = n0 + c;
            float e[4] = {0.f, 0.f, 0.f, 0.f};
            if (m < a.m && n < a.n)
                for (int sp = 0; sp < a.ksplit; ++sp)
                    for (int j = 0; j < 4 && n + j < a.n; ++j) e[j] += a.ws[(long)sp * total + (long)m * a.n + n + j];
            *reinterpret_cast<float4*>(ep + row * LDE + c) = make_float4(e[0], e[1], e[2], e[3]);
        }
    }
    __syncthreads();
    wd_gemm_args b = a;
    b.ksplit = 1;
    wd_epilogue_from_image<BM, BN, 256>(b, ep, m0, n0, tid);
}

template <int RM, int RN>
int launch_reduce(const wd_gemm_args& a, hipStream_t st) {
    constexpr int rsmem = RM * (RN + 4) * 4 + WD_STAT_SCRATCH;
    static bool rattr = false;
    if (!rattr) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&wd_gemm_reduce_kernel<RM, RN>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, rsmem) != hipSuccess)
            return WD_ELAUNCH;
        rattr = true;
    }
    const int rbn = (a.n + RN - 1) / RN, rbm = (a.m + RM - 1) / RM;
    WdLaunchScope scope(WD_CLS_GEMM_REDUCE, st);
    hipLaunchKernelGGL((wd_gemm_reduce_kernel<RM, RN>), dim3(rbn * rbm), dim3(256), rsmem, st, a, rbn);
    return wd_check_launch();
}

// the combine pass is pure streaming: narrow column tiles so that it fills the chip (whole statistics groups per tile
// when the GroupNorm sums are fused in).  The statistics layout is indexed by chunks of BM rows when a sample has more
// rows than that, so the 64-row tile is only used where it leaves that layout unchanged (samples of <= 64 rows).
// The combine for plain fp32 outputs (no statistics, row vector, activation or planes - every weight-gradient GEMM of the
// training step): a pure stream, one float4 of the output per thread, the slabs summed in ascending order; bias and the
// residual (gradient accumulation) are the only epilogue terms.  Half the time of the tile-shaped combine above.
__global__ void __launch_bounds__(256) wd_gemm_reduce_flat_kernel(const wd_gemm_args a) {
    const long total = (long)a.m * a.n, n4 = a.n >> 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.m * n4) return;
    const long m = i / n4;
    const int n = (int)(i - m * n4) * 4;
    const float* p = a.ws + m * a.n + n;
    float4 v = *reinterpret_cast<const float4*>(p);
    for (int sp = 1; sp < a.ksplit; ++sp) {
        const float4 q = *reinterpret_cast<const float4*>(p + (long)sp * total);
        v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    if (a.bias) {
        const float4 q = *reinterpret_cast<const float4*>(a.bias + n);
        v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    if (a.resid) {
        const float4 q = *reinterpret_cast<const float4*>(a.resid + m * a.resid_ld + n);
        v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    *reinterpret_cast<float4*>(a.out_f32 + m * a.out_ld + n) = v;
}

static bool reduce_flat_ok(const wd_gemm_args& a) {
    return !a.stat_part && !a.rowvec && !a.resid_rows && a.act == WD_ACT_NONE && !a.out_hi && a.out_f32 && (a.n & 3) == 0 &&
           (a.out_ld & 3) == 0 && (!a.resid || (a.resid_ld & 3) == 0) &&
           ((reinterpret_cast<uintptr_t>(a.out_f32) | reinterpret_cast<uintptr_t>(a.bias) | reinterpret_cast<uintptr_t>(a.resid) |
             reinterpret_cast<uintptr_t>(a.ws)) & 15) == 0;
}

int launch_reduce_flat(const wd_gemm_args& a, hipStream_t st) {
    WdLaunchScope scope(WD_CLS_GEMM_REDUCE, st);
    const long items = (long)a.m * (a.n >> 2);
    hipLaunchKernelGGL(wd_gemm_reduce_flat_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, a);
    return wd_check_launch();
}

}  // namespace

int wd_gemm_launch_reduce(const wd_gemm_args& a, hipStream_t st, int bm, int bn) {
    if (reduce_flat_ok(a)) return launch_reduce_flat(a, st);
    const int cpg = a.stat_part ? a.stat_cpg : 1;
    if (bm == 64 && bn == 320) {  // the 64-row tiles of wd_gemmw_kernel: the statistics layout follows 64-row chunks
        if (40 % cpg == 0 && a.n % 40 == 0) return launch_reduce<64, 40>(a, st);
        if (32 % cpg == 0 && a.n % 32 == 0) return launch_reduce<64, 32>(a, st);
        return launch_reduce<64, 64>(a, st);
    }
    const bool half_rows = bm == 128 && (!a.stat_part || (a.hw_out <= 64 && 64 % a.hw_out == 0));
    if (40 % cpg == 0) return half_rows ? launch_reduce<64, 40>(a, st) : launch_reduce<128, 40>(a, st);
    if (32 % cpg == 0) return half_rows ? launch_reduce<64, 32>(a, st) : launch_reduce<128, 32>(a, st);
    switch (bm * 1000 + bn) {  // statistics groups that divide neither 40 nor 32 columns: the GEMM's own tile
        case 128064: return launch_reduce<128, 64>(a, st);
        case 128160: return launch_reduce<128, 160>(a, st);
        case 128128: return launch_reduce<128, 128>(a, st);
        case 64064: return launch_reduce<64, 64>(a, st);
    }
    return WD_EINVAL;
}
