// Tap-gather GEMM: the opt-in kernels that lost their A/B against the defaults (families K_CONV3 and K_V8 of
// wd_gemm_plan.hip).  build.py compiles this file only when the library is built with WDIFF_EXPERIMENTAL=1 (and without the macro it is empty).
// "The kernel above" / "the default kernel" in the comments below: wd_gemm2_kernel, wd_gemm.hip, which also holds the third
// opt-in kernel, wd_gemm3_kernel (K_SLAB), and says why.
#ifdef WDIFF_EXPERIMENTAL
#include "wd_common.h"
#include "wd_gemm_epi.h"
#include "wd_gemm_priv.h"
#include "wd_gemm_tile.h"

namespace {

// ======================================================================================================
// Row-shared-taps kernel for the 3x3 / pad 1 / stride 1 convolutions (w_layout == 2; slab_rows = image width W).
// The per-stage cycle stamps of the kernel above show that a global_load_lds piece costs its wave 100-185 issue cycles while
// LDS reads are in flight, and that the LDS port is the bound: bytes through DMA per MFMA is what counts.  The three taps of
// one kernel row (dy; dx = -1, 0, +1) read the SAME source rows shifted by one token, so their A tile is loaded once: rows
// m0 + dy*W - 1 .. m0 + dy*W + 128 (130 rows + padding to 136, the last one all zero) per (dy, 64-channel chunk), used by three
// stages whose fragment reads go through row index r + dx + 1, or the zero row where the gather table says "padding" (image
// edges, sample boundaries).  K order: (dy, chunk, dx) - the weight tile of a stage is simply addressed at column
// (3*dy + dx + 4... tap)*C + chunk*64 of the ordinary [n][tap*C + c] operand, no re-layout.  DMA pieces per three taps:
// 34 (A) + 120 (W) instead of 96 + 120.  An identity second source (the 1x1 skip of a ResBlock) follows as ordinary stages.
// Tile 128 x 160, 8 waves = 2 K-halves x (2 x 2) waves of 64 x 80 on v_mfma_f32_16x16x32_bf16, the second K-half group one
// stage late (stagger), epilogue shared with the kernel above.
template <int NPASS>
__global__ void __launch_bounds__(512, 1) wd_conv3_kernel(const wd_gemm_args a, const int nbn, const int nbm) {
    constexpr int BM = 128, BN = 160;
    constexpr int NPL = (NPASS == 1) ? 1 : 2;
    constexpr int AR = 136;                 // rows of an A tile (130 used, row 135 = zero row)
    constexpr int A_PL = AR * 128, B_PL = BN * 128;
    constexpr int ABUF = NPL * A_PL, WBUF = NPL * B_PL;
    constexpr int APCS = NPL * (AR / 8), WPCS = NPL * (BN / 8);   // DMA pieces per tile
    constexpr int A_INS = (APCS + 7) / 8, W_INS = (WPCS + 7) / 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sA = smem;                        // [2][NPL][AR][128 B]
    char* sW = smem + 2 * ABUF;             // [2][NPL][BN][128 B]
    int* s_tab = reinterpret_cast<int*>(smem + 2 * ABUF + 2 * WBUF);  // [9][BM] source row of src[0] per tap, -1 = padding

    const int ntile = nbn * nbm;
    const int nwg = ntile * a.ksplit;
    int wg;
    {
        const int bid = blockIdx.x;
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int sidx = wg / ntile;
    wg -= sidx * ntile;
    const int bn_i = wg % nbn, bm_i = wg / nbn;
    const int m0 = bm_i * BM, n0 = bn_i * BN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = wave & 3, kh = wave >> 2;
    const int lrow = lane >> 3, lpos = lane & 7;
    const int Wimg = a.slab_rows;

    {
        const int32_t* g0 = a.src[0].gather;
        const int hw_src0 = a.src[0].hw_src;
        for (int idx = tid; idx < 9 * BM; idx += 512) {
            const int t = idx / BM, row = idx - t * BM;
            const int m = m0 + row;
            int v = -1;
            if (m < a.m) {
                const int b = m / a.hw_out, p = m - b * a.hw_out;
                const int g = g0[t * a.hw_out + p];
                if (g >= 0) v = b * hw_src0 + g;
            }
            s_tab[idx] = v;
        }
    }
    const wd_bf16* zline = reinterpret_cast<const wd_bf16*>(wd_zero_line) + lpos * 8;
    const int C0 = a.src[0].c, nc0 = C0 / 64;
    const int nq0 = 9 * nc0;                              // stages of the convolution
    const int nk_all = a.ktot / 64;                       // + C1 / 64 identity stages
    const int k_begin = (int)((long)nk_all * sidx / a.ksplit), k_end = (int)((long)nk_all * (sidx + 1) / a.ksplit);
    const int nk = k_end - k_begin;
    const long rows_src0 = (long)(a.m / a.hw_out) * a.src[0].hw_src;   // rows of the source planes (== a.m for a 'same' conv)

    // stage state (wave-uniform, advanced incrementally - no divisions in the loop): conv stages run (dy, chunk, dx), then the
    // identity stages; G = group id (one A tile per group), kcol = first weight column of the stage
    struct Stg { int conv, dyi, chunk, dxi, G; long kcol; };
    auto stage_at = [&](int q) {
        Stg t;
        if (q < nq0) {
            t.conv = 1;
            t.dyi = q / (3 * nc0);
            const int rem = q - t.dyi * 3 * nc0;
            t.chunk = rem / 3;
            t.dxi = rem - t.chunk * 3;
            t.G = q / 3;
            t.kcol = (long)(t.dyi * 3 + t.dxi) * C0 + t.chunk * 64;
        } else {
            t.conv = 0; t.dyi = 1; t.chunk = q - nq0; t.dxi = 0;
            t.G = nq0 / 3 + t.chunk;
            t.kcol = (long)9 * C0 + (long)t.chunk * 64;
        }
        return t;
    };
    auto next_of = [&](Stg t) {   // the stage after t
        if (t.conv) {
            if (++t.dxi == 3) {
                t.dxi = 0;
                ++t.G;
                if (++t.chunk == nc0) {
                    t.chunk = 0;
                    if (++t.dyi == 3) { t.conv = 0; t.dyi = 1; }
                }
            }
            t.kcol = t.conv ? (long)(t.dyi * 3 + t.dxi) * C0 + t.chunk * 64 : (long)9 * C0;
        } else {
            ++t.chunk; ++t.G; t.kcol += 64;
        }
        return t;
    };
    // static part of this lane's DMA slots: slot i = piece wave + 8 i -> (plane, 8-row piece)
    int a_j[A_INS];                     // tile row of the A slots
    long a_ro0[A_INS], a_ro1[A_INS];    // tile row * ld + swizzled chunk, for src[0] / src[1]
    long w_off[W_INS];                  // n * ktot + swizzled chunk of the W slots, -1 = zero line
#pragma unroll
    for (int i = 0; i < A_INS; ++i) {
        const int pc = wave + 8 * i, rp = pc % (AR / 8);
        a_j[i] = rp * 8 + lrow;
        const int sw = (lpos ^ ((a_j[i] >> 1) & 7)) * 8;
        a_ro0[i] = (long)a_j[i] * a.src[0].ld + sw;
        a_ro1[i] = a.nsrc > 1 ? (long)a_j[i] * a.src[1].ld + sw : 0;
    }
#pragma unroll
    for (int i = 0; i < W_INS; ++i) {
        const int pc = wave + 8 * i, rp = pc % (BN / 8);
        const int row = rp * 8 + lrow, n = n0 + row;
        w_off[i] = (pc < WPCS && n < a.n) ? (long)n * a.ktot + (lpos ^ ((row >> 1) & 7)) * 8 : -1;
    }
    // source pointer of one DMA slot of the A tile of stage-state t / of its W tile (zero line where there is nothing to load)
    auto ptr_A = [&](const Stg& t, int i) -> const wd_bf16* {
        const int pc = wave + 8 * i;
        const int pl = pc / (AR / 8);
        const long srow0 = t.conv ? (long)m0 + (long)(t.dyi - 1) * Wimg - 1 : (long)m0;   // source row of tile row 0 (uniform)
        const long sr = srow0 + a_j[i];
        const bool ok = pc < APCS && a_j[i] < (t.conv ? 130 : 128) && sr >= 0 && sr < (t.conv ? rows_src0 : (long)a.m);
        const wd_bf16* base = t.conv ? (pl ? a.src[0].lo : a.src[0].hi) + srow0 * a.src[0].ld + t.chunk * 64
                                     : (pl ? a.src[1].lo : a.src[1].hi) + srow0 * a.src[1].ld + t.chunk * 64;
        return ok ? base + (t.conv ? a_ro0[i] : a_ro1[i]) : zline;
    };
    auto ptr_W = [&](long kcol, int i) -> const wd_bf16* {
        const int pc = wave + 8 * i;
        const int pl = pc / (BN / 8);
        return w_off[i] >= 0 ? (pl ? a.w_lo : a.w_hi) + kcol + w_off[i] : zline;
    };
    // issue: destination of slot i is fixed by (wave, i): buffer G & 1 of sA / buffer q & 1 of sW
    auto issue_A = [&](int G, int i, const wd_bf16* src) {
        const int pc = wave + 8 * i;
        if (pc >= APCS) return;
        const int pl = pc / (AR / 8), rp = pc - pl * (AR / 8);
        __builtin_amdgcn_global_load_lds((wd_gbl_ptr)src, (wd_lds_ptr)(sA + (G & 1) * ABUF + pl * A_PL + rp * 1024), 16, 0, 0);
    };
    auto issue_W = [&](int q, int i, const wd_bf16* src) {
        const int pc = wave + 8 * i;
        if (pc >= WPCS) return;
        const int pl = pc / (BN / 8), rp = pc - pl * (BN / 8);
        __builtin_amdgcn_global_load_lds((wd_gbl_ptr)src, (wd_lds_ptr)(sW + (q & 1) * WBUF + pl * B_PL + rp * 1024), 16, 0, 0);
    };
    auto fire_A1 = [&](const Stg& t, int i) { issue_A(t.G, i, ptr_A(t, i)); };
    auto fire_W1 = [&](int q, long kcol, int i) { issue_W(q, i, ptr_W(kcol, i)); };
    // slot of everything stage q+1 (state tn) needs that is not in LDS yet: W slots first, then (new group only) the A slots
    auto prefetch_slot = [&](int q, const Stg& tn, bool newA, int sl) {
        if (sl < W_INS) fire_W1(q + 1, tn.kcol, sl);
        else if (newA) fire_A1(tn, sl - W_INS);
    };
    constexpr int NSL = W_INS + A_INS;

    f32x4 acc[4][5];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < 5; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][t][r] = 0.0f;
    Stg cur = stage_at(k_begin < nk_all ? k_begin : 0);
    if (nk > 0) {
#pragma unroll
        for (int i = 0; i < A_INS; ++i) fire_A1(cur, i);
#pragma unroll
        for (int i = 0; i < W_INS; ++i) fire_W1(k_begin, cur.kcol, i);
    }
    const int l15 = lane & 15, lq = lane >> 4;
    const int r0w = (wq >> 1) * 64, c0w = (wq & 1) * 80;
    const int ch = kh * 4 + lq;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // the gather table is complete
    // which (tap, row) pairs of this lane's four fragment rows are real pixels: bit tap * 4 + i
    unsigned long long vmask = 0ull;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (s_tab[t * BM + r0w + i * 16 + l15] >= 0) vmask |= 1ull << (t * 4 + i);
    bf16x8 xa[4][NPL], xb[5][NPL];
    auto read16 = [&](int q, const Stg& t) {
        const char* ab = sA + (t.G & 1) * ABUF;
        const char* wb = sW + (q & 1) * WBUF;
        const unsigned vm = t.conv ? (unsigned)(vmask >> ((t.dyi * 3 + t.dxi) * 4)) & 15u : 15u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0w + i * 16 + l15;
            const int j = (vm >> i) & 1u ? r + t.dxi : AR - 1;   // (identity stages: dxi = 0, rows beyond M are zero-filled)
            const int ao = lds_off2(j, ch);
#pragma unroll
            for (int p = 0; p < NPL; ++p) xa[i][p] = *reinterpret_cast<const bf16x8*>(ab + p * A_PL + ao);
        }
#pragma unroll
        for (int t5 = 0; t5 < 5; ++t5) {
            const int bo = lds_off2(c0w + t5 * 16 + l15, ch);
#pragma unroll
            for (int p = 0; p < NPL; ++p) xb[t5][p] = *reinterpret_cast<const bf16x8*>(wb + p * B_PL + bo);
        }
    };
    // the products of one stage; `pf`: issue the (pre-computed) DMA slots of stage q+1 between the four row groups - no address
    // arithmetic between the MFMAs, a 16x16x32 MFMA leaves room for about two vector instructions
    const wd_bf16* pw[W_INS];
    const wd_bf16* pa[A_INS];
    auto mfma16 = [&](bool pf, int q, int Gn, bool newA) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                if (NPL == 2) {
                    acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[i][NPL - 1], xb[t][0], acc[i][t], 0, 0, 0);
                    acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[i][0], xb[t][NPL - 1], acc[i][t], 0, 0, 0);
                }
                acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[i][0], xb[t][0], acc[i][t], 0, 0, 0);
            }
            if (pf) {
#pragma unroll
                for (int sl = i * NSL / 4; sl < (i + 1) * NSL / 4; ++sl) {
                    if (sl < W_INS) issue_W(q + 1, sl, pw[sl]);
                    else if (newA) issue_A(Gn, sl - W_INS, pa[sl - W_INS]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    const bool stamp = (a.dbg & WD_DBG_STAMPS) && blockIdx.x == 0 && lane == 0 && a.ws && a.ksplit == 1;
    unsigned long long* sb = reinterpret_cast<unsigned long long*>(a.ws) + (long)wave * nk * 4;
    if (kh == 1) {
        // late group: DMA of the next stage first, then the previous stage's products, then this stage's fragments
        for (int q = k_begin; q < k_end; ++q) {
            if (stamp) sb[(q - k_begin) * 4 + 0] = __builtin_amdgcn_s_memtime();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's LDS-DMA pieces have landed (the fence of
            __syncthreads();                                  // __syncthreads does not have to wait for loads)
            if (stamp) sb[(q - k_begin) * 4 + 1] = __builtin_amdgcn_s_memtime();
            const Stg tn = next_of(cur);
            if (q + 1 < k_end) {
                const bool newA = tn.G != cur.G;
#pragma unroll
                for (int sl = 0; sl < NSL; ++sl) prefetch_slot(q, tn, newA, sl);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (q > k_begin) mfma16(false, q, 0, false);
            __builtin_amdgcn_sched_barrier(0);
            if (stamp) sb[(q - k_begin) * 4 + 2] = __builtin_amdgcn_s_memtime();
            read16(q, cur);
            if (stamp) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                sb[(q - k_begin) * 4 + 3] = __builtin_amdgcn_s_memtime();
            }
            cur = tn;
        }
        if (nk > 0) mfma16(false, 0, 0, false);
    } else {
        for (int q = k_begin; q < k_end; ++q) {
            if (stamp) sb[(q - k_begin) * 4 + 0] = __builtin_amdgcn_s_memtime();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // stage q has landed, the buffers of stage q-1 are free
            if (stamp) sb[(q - k_begin) * 4 + 1] = __builtin_amdgcn_s_memtime();
            const bool more = q + 1 < k_end;
            const Stg tn = next_of(cur);
            const bool newA = more && tn.G != cur.G;
            read16(q, cur);
            if (more) {  // addresses of the next stage's pieces, in the shadow of the fragment reads
#pragma unroll
                for (int i = 0; i < W_INS; ++i) pw[i] = ptr_W(tn.kcol, i);
                if (newA) {
#pragma unroll
                    for (int i = 0; i < A_INS; ++i) pa[i] = ptr_A(tn, i);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (stamp) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                sb[(q - k_begin) * 4 + 2] = __builtin_amdgcn_s_memtime();
            }
            mfma16(more, q, tn.G, newA);
            if (stamp) sb[(q - k_begin) * 4 + 3] = __builtin_amdgcn_s_memtime();
            cur = tn;
        }
    }
    // ---- partial tiles -> fp32 LDS image (the two K-halves summed in a fixed order), then the shared epilogue
    constexpr int LDE = BN + 4;
    float* ep = reinterpret_cast<float*>(smem);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int hh = 0; hh < 2; ++hh) {
        if (kh == hh) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int t = 0; t < 5; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float* pe = ep + (r0w + i * 16 + 4 * lq + r) * LDE + c0w + t * 16 + l15;
                        *pe = (hh == 0) ? acc[i][t][r] : *pe + acc[i][t][r];
                    }
        }
        __syncthreads();
    }
    wd_epilogue_tail<BM, BN, 512>(a, ep, m0, n0, tid, sidx);
}

template <int NPASS>
int launch_conv3(const wd_gemm_args& a, hipStream_t st) {
    constexpr int NPL = (NPASS == 1) ? 1 : 2;
    constexpr int loop_smem = 2 * NPL * (136 + 160) * 128 + 9 * 128 * 4;
    constexpr int red_smem = 128 * (160 + 4) * 4 + WD_STAT_SCRATCH;
    constexpr int smem = loop_smem > red_smem ? loop_smem : red_smem;
    static_assert(smem <= 160 * 1024, "LDS budget");
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&wd_conv3_kernel<NPASS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                smem) != hipSuccess)
            return WD_ELAUNCH;
        attr_done = true;
    }
    const int nbn = (a.n + 159) / 160, nbm = (a.m + 127) / 128;
    {
        WdLaunchScope scope(WD_CLS_GEMM, st, 2.0 * (double)a.m * (double)a.n * (double)a.ktot);
        hipLaunchKernelGGL((wd_conv3_kernel<NPASS>), dim3(nbn * nbm * a.ksplit), dim3(512), smem, st, a, nbn, nbm);
    }
    if (a.ksplit > 1) {
        return wd_gemm_launch_reduce(a, st, 128, 160);
    }
    return wd_check_launch();
}

// ======================================================================================================
// v8: a RING kernel (32-deep stages, four LDS buffers, one raw barrier per stage, counted vmcnt) with the DMA moved to FOUR
// DEDICATED LOADER WAVES (12 waves per workgroup, three per SIMD at <= 168 registers).  Opt-in (WDIFF_GEMM_V8=1): within
// +-5 % of wd_gemm2_kernel on every layer shape (same box: 88-90 vs 85-86 us on the 320 x 3 x 3 convolution at B = 64, 19.9-20.3 vs
// 20.3-20.5 us on the 5-stage 1x1 layers).  What it was built to find out (round 2): with the parts of wd_gemm2_kernel switched off
// one at a time its MFMA, fragment-read and DMA costs ADD instead of overlapping - a wave that issues buffer_load ... lds
// cannot feed the MFMA pipe meanwhile.  Here the eight compute waves (32 x 80 blocks of 2 x 5 tiles of
// v_mfma_f32_16x16x32_bf16, 40 accumulator registers, which pays for TWO fragment sets: the fragments of stage k+1 are read
// while stage k is multiplied, pass-major so that dependent MFMAs are nine apart) only read fragments and multiply; loader
// wave L (one per SIMD) fetches, per stage, A pieces 2L, 2L+1 and W pieces L, L+4 of every plane plus one of the four leftover
// W pieces - nine pieces (five with one plane), so `s_waitcnt vmcnt(9)` at the top of its step leaves exactly the youngest
// stage in flight.  Result of the same switch-off experiment here: the loaders are NOT the limit (compute waves alone: 78 of
// 85 us); the MFMAs alone run at 14 cycles each (near the pipe's 16), but the barrier every 32-deep stage and the fragment
// waits stretch a stage from ~850 to ~1800 cycles - two waves per SIMD that meet at the same barrier cannot cover each other.
// Orders: RAW - the loaders wait for their own pieces of stage k+1, then the barrier every wave passes, then the compute
// waves read that buffer; WAR - the buffer refilled after barrier k held stage k-1, whose fragment reads the compute waves
// consumed (lgkmcnt) before the MFMAs of stage k-1, i.e. before they arrived at barrier k.
template <int NPASS>
__global__ void __launch_bounds__(768, 1) wd_gemm8_kernel(const wd_gemm_args a, const int nbn, const int nbm) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int BM = 128, BN = 160, BKS = 32, NST = 4;
    constexpr int NPL = (NPASS == 1) ? 1 : 2;
    constexpr int A_PL = BM * 64, B_PL = BN * 64;
    constexpr int STAGE = NPL * (A_PL + B_PL);
    constexpr int RING = NST * STAGE;
    constexpr int TAB_OFF = RING;
    constexpr uint32_t WD_OOB = 0x80000000u;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* s_tab = reinterpret_cast<int*>(smem + TAB_OFF);  // [ntaps0][BM] source row of src[0] per tap, -1 = zero row

    const int ntile = nbn * nbm;
    const int nwg = ntile * a.ksplit;
    int wg;
    {
        const int bid = blockIdx.x;
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int sidx = wg / ntile;
    wg -= sidx * ntile;
    const int bn_i = wg % nbn, bm_i = wg / nbn;
    const int m0 = bm_i * BM, n0 = bn_i * BN;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    {
        const int nt0 = a.src[0].ntaps;
        const int32_t* g0 = a.src[0].gather;
        const int hw_src0 = a.src[0].hw_src;
        const int Wimg = a.slab_rows;  // > 0: 3x3 / pad 1 / stride 1 over images Wimg wide: the table is computed
        for (int idx = tid; idx < nt0 * BM; idx += 768) {
            const int t = idx / BM, row = idx - t * BM;
            const int m = m0 + row;
            int v = -1;
            if (m < a.m) {
                if (g0 && Wimg > 0) {
                    const int b = m / a.hw_out, p = m - b * a.hw_out;
                    const int y = p / Wimg, x = p - y * Wimg;
                    const int ky = t / 3, dy = ky - 1, dx = t - ky * 3 - 1;
                    const int sy = y + dy, sx = x + dx;
                    if (sy >= 0 && sy * Wimg < a.hw_out && sx >= 0 && sx < Wimg) v = b * hw_src0 + sy * Wimg + sx;
                } else if (g0) {
                    const int b = m / a.hw_out, p = m - b * a.hw_out;
                    const int g = g0[t * a.hw_out + p];
                    if (g >= 0) v = b * hw_src0 + g;
                } else {
                    v = m;
                }
            }
            s_tab[idx] = v;
        }
    }
    __syncthreads();

    const int nk_all = a.ktot / BKS;
    const int k_begin = (int)((long)nk_all * sidx / a.ksplit), k_end = (int)((long)nk_all * (sidx + 1) / a.ksplit);
    const int nk = k_end - k_begin;

    f32x4 acc[2][5];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 5; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][t][r] = 0.0f;
    const int l15 = lane & 15, lq = lane >> 4;
    const int cw = wave & 7;
    const int r0w = (cw >> 1) * 32, c0w = (cw & 1) * 80;

    if (wave >= 8) {
        // =========================== loader wave L: every DMA piece of the workgroup ===========================
        const int L = wave - 8;
        const int lrow = lane >> 2, lpos = lane & 3;              // a DMA piece = 16 rows x 64 bytes
        const int sw = (lpos ^ ((0 - (lane >> 4)) & 3)) * 8;      // source chunk (elements) that lands at position lpos of row lrow
        auto make_srd = [](const wd_bf16* p) {
            return __builtin_amdgcn_make_buffer_rsrc(const_cast<wd_bf16*>(p), 0, 0x7FFFFFF0, 0x00020000);
        };
        // W pieces L, L + 4 (both planes) and leftover item L: piece 8 + (L >> (NPL - 1)) of plane L & (NPL - 1); one plane: loaders
        // 0, 1 take pieces 8, 9 and loaders 2, 3 re-fetch pieces 8, 9 as well (same bytes to the same place: harmless, and every
        // loader issues the same number of pieces)
        const int x_piece = NPL == 2 ? 8 + (L >> 1) : 8 + (L & 1), x_plane = NPL == 2 ? (L & 1) : 0;
        uint32_t b_voff[3];
        {
            const int pcs[3] = {L, L + 4, x_piece};
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int n = n0 + pcs[i] * 16 + lrow;
                b_voff[i] = n < a.n ? (uint32_t)(((long)n * a.ktot + sw) * 2) : WD_OOB;
            }
        }
        const __amdgpu_buffer_rsrc_t srd_w_hi = make_srd(a.w_hi), srd_w_lo = make_srd(a.w_lo ? a.w_lo : a.w_hi);
        const __amdgpu_buffer_rsrc_t srd_w_x = (x_plane ? srd_w_lo : srd_w_hi);
        int s = 0, tap = 0, kc = 0;
        int cur_ld = a.src[0].ld, cur_cpt = a.src[0].c / BKS, cur_nt = a.src[0].ntaps;
        const wd_bf16* cur_hi = a.src[0].hi;
        const wd_bf16* cur_lo = a.src[0].lo;
        {
            const int cpt = a.src[0].c / BKS, n0st = a.src[0].ntaps * cpt;
            if (k_begin < n0st) {
                tap = k_begin / cpt;
                kc = k_begin - tap * cpt;
            } else {
                s = 1;
                kc = k_begin - n0st;
                cur_hi = a.src[1].hi;
                cur_lo = a.src[1].lo;
                cur_ld = a.src[1].ld;
                cur_cpt = a.src[1].c / BKS;
                cur_nt = a.src[1].ntaps;
            }
        }
        __amdgpu_buffer_rsrc_t srd_a_hi = make_srd(cur_hi), srd_a_lo = make_srd(cur_lo ? cur_lo : cur_hi);
        uint32_t a_voff[2];
        auto locate = [&]() {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = (2 * L + i) * 16 + lrow;
                int r;
                if (s == 0) r = s_tab[tap * BM + row];
                else r = (m0 + row < a.m) ? m0 + row : -1;  // src[1] is an identity source (1x1 skip)
                a_voff[i] = r >= 0 ? (uint32_t)r * (uint32_t)(cur_ld * 2) + (uint32_t)(sw * 2) : WD_OOB;
            }
        };
        locate();
        int soff_a = kc * BKS * 2, soff_b = k_begin * BKS * 2;
        int wr_off = 0;
        auto issue_stage = [&]() {
            char* sbase = smem + wr_off;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_a_hi, (wd_lds_ptr)(sbase + (2 * L + i) * 1024), 16, a_voff[i], soff_a, 0, 0);
                if (NPL == 2)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_a_lo, (wd_lds_ptr)(sbase + A_PL + (2 * L + i) * 1024), 16, a_voff[i],
                                                             soff_a, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_w_hi, (wd_lds_ptr)(sbase + NPL * A_PL + (L + 4 * i) * 1024), 16, b_voff[i],
                                                         soff_b, 0, 0);
                if (NPL == 2)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_w_lo, (wd_lds_ptr)(sbase + NPL * A_PL + B_PL + (L + 4 * i) * 1024), 16,
                                                             b_voff[i], soff_b, 0, 0);
            }
            __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_w_x, (wd_lds_ptr)(sbase + NPL * A_PL + x_plane * B_PL + x_piece * 1024), 16,
                                                     b_voff[2], soff_b, 0, 0);
            // the issue state moves on by one stage
            soff_b += BKS * 2;
            soff_a += BKS * 2;
            wr_off += STAGE;
            if (wr_off == RING) wr_off = 0;
            ++kc;
            if (kc == cur_cpt) {
                kc = 0;
                soff_a = 0;
                ++tap;
                if (tap == cur_nt) {
                    tap = 0;
                    ++s;
                    if (s < a.nsrc) {
                        cur_hi = a.src[1].hi;
                        cur_lo = a.src[1].lo;
                        cur_ld = a.src[1].ld;
                        cur_cpt = a.src[1].c / BKS;
                        cur_nt = a.src[1].ntaps;
                        srd_a_hi = make_srd(cur_hi);
                        srd_a_lo = make_srd(cur_lo ? cur_lo : cur_hi);
                    }
                }
                if (s < a.nsrc) locate();
            }
        };
        auto wait_keep1 = [&]() {  // all but the youngest issued stage have landed
            if (NPL == 2) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        };
        __builtin_amdgcn_s_setprio(2);
        int issued = 0;
        for (; issued < 3 && issued < nk; ++issued) issue_stage();
        if (nk > 0) {  // stage 0 landed
            if (issued >= 2) {
                if (issued == 3) {
                    if (NPL == 2) asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
                } else {
                    wait_keep1();
                }
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
        }
        int kit = 0;
        for (; kit + 3 < nk; ++kit) {  // steady state: stage kit + 1 landed -> barrier -> fetch stage kit + 3
            wait_keep1();
            __builtin_amdgcn_s_barrier();
            issue_stage();
        }
        for (; kit < nk; ++kit) {      // drain: nothing left to fetch
            if (kit + 1 < nk) {
                if (kit + 2 < nk) wait_keep1();
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
        }
    } else {
        // =========================== compute wave: fragments and products only ===========================
        const int ao0 = lds_off16(r0w + l15, lq), bo0 = NPL * A_PL + lds_off16(c0w + l15, lq);
        bf16x8 fa0[2][NPL], fb0[5][NPL], fa1[2][NPL], fb1[5][NPL];
        // (16 rows further down the XOR key of lds_off16 differs - rows r0w + 16 i, c0w + 16 t: (row >> 2) & 3 advances by 4 = 0 mod 4,
        // so the key repeats and a wave's fragments are one lane offset + immediates)
        auto read_a = [&](auto& fa_, const char* base, int i) {
#pragma unroll
            for (int p = 0; p < NPL; ++p) fa_[i][p] = *reinterpret_cast<const bf16x8*>(base + ao0 + p * A_PL + i * 1024);
        };
        auto read_b = [&](auto& fb_, const char* base, int t) {
#pragma unroll
            for (int p = 0; p < NPL; ++p) fb_[t][p] = *reinterpret_cast<const bf16x8*>(base + bo0 + p * B_PL + t * 1024);
        };
        // The three products of a tile (lo*hi, hi*lo, hi*hi) go to the same accumulator: issued back to back each waits for the
        // previous one's result (measured: 30.7 cycles per MFMA in this loop with the DMA switched off, against 16 at the pipe's
        // rate).  So the step runs pass-major: the first product of all ten tiles, then the second, then the third - nine
        // independent MFMAs between two dependent ones; per tile the order of the three products, hence the result, is unchanged.
        auto mfma_pass = [&](auto& fa_, auto& fb_, int pass, int g) {
            const int i = g / 5, t = g % 5;
            if (NPL == 2) {
                if (pass == 0) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_[i][NPL - 1], fb_[t][0], acc[i][t], 0, 0, 0);
                else if (pass == 1) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_[i][0], fb_[t][NPL - 1], acc[i][t], 0, 0, 0);
                else acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_[i][0], fb_[t][0], acc[i][t], 0, 0, 0);
            } else {
                if (pass == 2) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_[i][0], fb_[t][0], acc[i][t], 0, 0, 0);
            }
        };
        if (nk > 0) {
            __builtin_amdgcn_s_barrier();  // stage 0 has landed
#pragma unroll
            for (int i = 0; i < 2; ++i) read_a(fa0, smem, i);
#pragma unroll
            for (int t = 0; t < 5; ++t) read_b(fb0, smem, t);
        }
        int rd_off = STAGE;  // ring offset of the stage whose fragments are read next (stage kit + 1)
        auto step = [&](bool have1, auto& ma, auto& mb, auto& ra, auto& rb) {
            __builtin_amdgcn_s_barrier();
            const char* nb = smem + rd_off;
            // Per-step stamps of this loop (clock64, one compute wave): barrier wait ~100-250 cycles, the first ten MFMAs of the
            // step ~700 (the two compute waves of a SIMD together: 36 cycles per MFMA), the other twenty ~500 (14 per MFMA, the
            // pipe's rate), 1490-1620 cycles per step - whether the 14 fragment reads of the next stage are issued at once, as here,
            // or spread over the step (which costs registers: 168 + spills instead of 159); the loaders wait ~800 cycles per step
            // at the barrier, i.e. they are not the limit.
#pragma unroll
            for (int pass = (NPL == 2 ? 0 : 2); pass < 3; ++pass) {
#pragma unroll
                for (int g = 0; g < 10; ++g) {
                    // the 14 fragment reads of the next stage, two per slot of the first pass (the only pass with one plane)
                    if (have1 && pass == (NPL == 2 ? 0 : 2)) {
                        if (g < 2) read_a(ra, nb, g);
                        else if (g < 7) read_b(rb, nb, g - 2);
                    }
                    mfma_pass(ma, mb, pass, g);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            rd_off += STAGE;
            if (rd_off == RING) rd_off = 0;
        };
        for (int kit = 0; kit < nk; kit += 2) {  // (static roles of the two fragment sets: unrolled by two)
            step(kit + 1 < nk, fa0, fb0, fa1, fb1);
            if (kit + 1 < nk) step(kit + 2 < nk, fa1, fb1, fa0, fb0);
        }
    }

    // ---- epilogue: accumulators -> fp32 LDS image of the tile, then the shared epilogue (all twelve waves)
    constexpr int LDE = BN + 4;
    float* ep = reinterpret_cast<float*>(smem);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (wave < 8) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int t = 0; t < 5; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) ep[(r0w + i * 16 + 4 * lq + r) * LDE + c0w + t * 16 + l15] = acc[i][t][r];
    }
    __syncthreads();
    wd_epilogue_tail<BM, BN, 768>(a, ep, m0, n0, tid, sidx);
#endif
}

template <int NPASS>
int launch8(const wd_gemm_args& a, hipStream_t st) {
    constexpr int NPL = (NPASS == 1) ? 1 : 2;
    constexpr int loop_smem = 4 * NPL * (128 + 160) * 64 + 9 * 128 * 4;
    constexpr int red_smem = 128 * (160 + 4) * 4 + WD_STAT_SCRATCH;
    constexpr int smem = loop_smem > red_smem ? loop_smem : red_smem;
    static_assert(smem <= 160 * 1024, "LDS budget");
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&wd_gemm8_kernel<NPASS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                smem) != hipSuccess)
            return WD_ELAUNCH;
        attr_done = true;
    }
    const int nbn = (a.n + 159) / 160, nbm = (a.m + 127) / 128;
    {
        WdLaunchScope scope(WD_CLS_GEMM, st, 2.0 * (double)a.m * (double)a.n * (double)a.ktot);
        hipLaunchKernelGGL((wd_gemm8_kernel<NPASS>), dim3(nbn * nbm * a.ksplit), dim3(768), smem, st, a, nbn, nbm);
    }
    if (a.ksplit > 1) return wd_gemm_launch_reduce(a, st, 128, 160);
    return wd_check_launch();
}

}  // namespace

int wd_conv3_launch(const wd_gemm_args& a, hipStream_t st) { return a.npass == 3 ? launch_conv3<3>(a, st) : launch_conv3<1>(a, st); }

int wd_gemm8_launch(const wd_gemm_args& a, hipStream_t st) { return a.npass == 3 ? launch8<3>(a, st) : launch8<1>(a, st); }

#endif  // WDIFF_EXPERIMENTAL
