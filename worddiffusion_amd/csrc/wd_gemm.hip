// Tap-gather GEMM, the v1 and v2 kernels (families K_V1, K_V2, K_M16 of wd_gemm_plan.hip; K_PP and K_SLAB in an experimental build) on
// v_mfma_f32_32x32x16_bf16 / v_mfma_f32_16x16x32_bf16 with split-bf16 operands (gfx950).  What wd_gemm computes and which launch
// takes which kernel: wd_gemm_plan.hip; the other kernels: wd_gemm4.hip, wd_gemmw.hip, wd_gemmq.hip, wd_gemm_reduce.hip, wd_gemm_exp.hip.
//
// Why three kernels share this unit.  wd_gemm_kernel and wd_gemm3_kernel<..., KS = 2> call the same instantiations of wd_epilogue_lds
// (wd_gemm_tile.h) as wd_gemm2_kernel, with constants (kh = 0, sidx = 0) where wd_gemm2_kernel passes variables.  In a unit of their
// own every caller of an instantiation passes the same constants, hipcc propagates them into the function before it inlines it, and
// four of the eight wd_gemm_kernel and all six wd_gemm3_kernel<..., 2> instantiations come out with other (equivalent) address
// arithmetic, registers and schedule in their epilogue.  Next to wd_gemm2_kernel they compile to the code they always had, so they
// stay next to it.  (wd_gemm4_kernel, wd_conv3_kernel and wd_gemm8_kernel do not share an instantiation and have units of their own.)
#include "wd_common.h"
#include "wd_gemm_epi.h"
#include "wd_gemm_priv.h"
#include "wd_gemm_tile.h"

namespace {

// v1 (K_V1): the form for K that is no multiple of 64, or WDIFF_GEMM_V1.
// Tile: BM x BN x 32 per stage, 4 waves (256 threads), each wave 32 rows x (BN / WN) columns of 32x32 MFMA
// tiles.  Operands are staged global -> VGPR -> LDS (16-byte chunks, XOR-swizzled so that ds_read_b128 of a
// 32-row fragment is bank-conflict free), double buffered with one barrier per K-step.  npass = 3 issues
// lo*hi + hi*lo + hi*hi per fragment pair (fp32-class result), npass = 1 hi*hi only.
template <int BM, int BN, int NPASS>
__global__ void __launch_bounds__(256, 2) wd_gemm_kernel(const wd_gemm_args a, const int nbn, const int nbm) {
    constexpr int NPL = (NPASS == 1) ? 1 : 2;
    constexpr int WM = BM / 32, WN = 4 / WM;
    constexpr int WCOLS = BN / WN;
    constexpr int TN = WCOLS / 32;
    static_assert(WCOLS % 32 == 0 && WM * WN == 4, "bad tile");
    constexpr int A_CH = BM * 4 / 256;
    constexpr int B_CH = (BN * 4 + 255) / 256;
    constexpr int A_PL = BM * 64;
    constexpr int B_PL = BN * 64;
    constexpr int STAGE = NPL * (A_PL + B_PL);

    extern __shared__ __attribute__((aligned(16))) char smem[];

    // ---- XCD-aware block order: the 8 XCDs each take a contiguous run of logical tiles, so the n-blocks that
    // share one A row-panel (and neighbouring panels that share gather halos) hit the same L2.
    const int nwg = nbn * nbm;
    int wg;
    {
        const int bid = blockIdx.x;
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int bn_i = wg % nbn, bm_i = wg / nbn;
    const int m0 = bm_i * BM, n0 = bn_i * BN;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int ach = tid & 3;

    // ---- per-thread A rows (fixed for the whole K loop)
    int a_row[A_CH], a_b[A_CH], a_p[A_CH];
    bool a_ok[A_CH];
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
        a_row[i] = (tid >> 2) + 64 * i;
        const int m = m0 + a_row[i];
        a_ok[i] = m < a.m;
        a_b[i] = a_ok[i] ? m / a.hw_out : 0;
        a_p[i] = a_ok[i] ? m - a_b[i] * a.hw_out : 0;
    }
    // ---- per-thread W rows
    int b_row[B_CH];
    long b_off[B_CH];
    bool b_ok[B_CH];
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
        b_row[i] = (tid >> 2) + 64 * i;
        const int n = n0 + b_row[i];
        b_ok[i] = (b_row[i] < BN) && (n < a.n);
        b_off[i] = (long)n * a.ktot + ach * 8;
    }

    // ---- K iteration state: (source, tap, channel chunk)
    int s = 0, tap = 0, kc = 0;
    const wd_bf16* cur_hi = a.src[0].hi;
    const wd_bf16* cur_lo = a.src[0].lo;
    const int32_t* cur_g = a.src[0].gather;
    int cur_ld = a.src[0].ld, cur_c = a.src[0].c, cur_nt = a.src[0].ntaps, cur_hw = a.src[0].hw_src;
    long a_off[A_CH];  // element offset of the source row, -1 = zero row

    auto locate = [&]() {
#pragma unroll
        for (int i = 0; i < A_CH; ++i) {
            long off = -1;
            if (a_ok[i]) {
                if (cur_g) {
                    const int g = cur_g[tap * a.hw_out + a_p[i]];
                    if (g >= 0) off = ((long)a_b[i] * cur_hw + g) * cur_ld;
                } else {
                    off = (long)(m0 + a_row[i]) * cur_ld;
                }
            }
            a_off[i] = off;
        }
    };
    locate();

    uint4 ra[NPL][A_CH], rb[NPL][B_CH];
    const uint4 zero4 = make_uint4(0, 0, 0, 0);

    auto gload = [&](int kit) {
#pragma unroll
        for (int i = 0; i < A_CH; ++i) {
            const long o = a_off[i] + kc * BK + ach * 8;
            ra[0][i] = a_off[i] >= 0 ? *reinterpret_cast<const uint4*>(cur_hi + o) : zero4;
            if (NPL == 2) ra[NPL - 1][i] = a_off[i] >= 0 ? *reinterpret_cast<const uint4*>(cur_lo + o) : zero4;
        }
#pragma unroll
        for (int i = 0; i < B_CH; ++i) {
            const long o = b_off[i] + (long)kit * BK;
            rb[0][i] = b_ok[i] ? *reinterpret_cast<const uint4*>(a.w_hi + o) : zero4;
            if (NPL == 2) rb[NPL - 1][i] = b_ok[i] ? *reinterpret_cast<const uint4*>(a.w_lo + o) : zero4;
        }
    };
    auto advance = [&]() {
        ++kc;
        if (kc * BK == cur_c) {
            kc = 0;
            ++tap;
            if (tap == cur_nt) {
                tap = 0;
                ++s;
                if (s < a.nsrc) {
                    cur_hi = a.src[1].hi;
                    cur_lo = a.src[1].lo;
                    cur_g = a.src[1].gather;
                    cur_ld = a.src[1].ld;
                    cur_c = a.src[1].c;
                    cur_nt = a.src[1].ntaps;
                    cur_hw = a.src[1].hw_src;
                }
            }
            if (s < a.nsrc) locate();
        }
    };
    auto lstore = [&](int stage) {
        char* base = smem + stage * STAGE;
#pragma unroll
        for (int p = 0; p < NPL; ++p) {
#pragma unroll
            for (int i = 0; i < A_CH; ++i)
                *reinterpret_cast<uint4*>(base + p * A_PL + lds_off(a_row[i], ach)) = ra[p][i];
#pragma unroll
            for (int i = 0; i < B_CH; ++i)
                if (b_row[i] < BN)
                    *reinterpret_cast<uint4*>(base + NPL * A_PL + p * B_PL + lds_off(b_row[i], ach)) = rb[p][i];
        }
    };

    f32x16 acc[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    const int nk = a.ktot / BK;
    gload(0);
    advance();
    lstore(0);
    __syncthreads();

    const int frow = lane & 31, fhalf = lane >> 5;
    for (int kit = 0; kit < nk; ++kit) {
        const bool more = kit + 1 < nk;
        if (more) {
            gload(kit + 1);
            advance();
        }
        const char* base = smem + (kit & 1) * STAGE;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int ch = kk * 2 + fhalf;
            const int ao = lds_off(wm * 32 + frow, ch);
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(base + ao);
            bf16x8 al;
            if (NPL == 2) al = *reinterpret_cast<const bf16x8*>(base + A_PL + ao);
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                const int bo = NPL * A_PL + lds_off(wn * WCOLS + t * 32 + frow, ch);
                const bf16x8 bh = *reinterpret_cast<const bf16x8*>(base + bo);
                if (NPL == 2) {
                    const bf16x8 bl = *reinterpret_cast<const bf16x8*>(base + B_PL + bo);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[t], 0, 0, 0);
                }
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[t], 0, 0, 0);
            }
        }
        if (more) lstore((kit + 1) & 1);
        __syncthreads();
    }

    wd_epilogue_lds<BM, BN, TN, 256>(a, acc, smem, m0, n0, wm, wn, WCOLS, 0, 1, tid);
}

template <int BM, int BN, int NPASS>
int launch(const wd_gemm_args& a, hipStream_t st) {
    constexpr int NPL = (NPASS == 1) ? 1 : 2;
    constexpr int loop_smem = 2 * NPL * (BM + BN) * 64;
    constexpr int red_smem = BM * (BN + 4) * 4 + WD_STAT_SCRATCH;
    constexpr int smem = loop_smem > red_smem ? loop_smem : red_smem;
    static bool attr_done = false;  // one process = one device, set once per instantiation
    if (!attr_done) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&wd_gemm_kernel<BM, BN, NPASS>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess)
            return WD_ELAUNCH;
        attr_done = true;
    }
    const int nbn = (a.n + BN - 1) / BN, nbm = (a.m + BM - 1) / BM;
    WdLaunchScope scope(WD_CLS_GEMM_OTHER, st, 2.0 * (double)a.m * (double)a.n * (double)a.ktot);
    hipLaunchKernelGGL((wd_gemm_kernel<BM, BN, NPASS>), dim3(nbn * nbm), dim3(256), smem, st, a, nbn, nbm);
    return wd_check_launch();
}

// v2: BK = 64, operands go global -> LDS directly (global_load_lds_dwordx4, no VGPR staging), two LDS stages,
// one barrier per K-step: the loads of step k+1 are in flight while step k is multiplied.  Full 128-byte lines
// per row and plane.  Requires every source's channel count to be a multiple of 64.
// LDS image of a [rows][64] bf16 plane: 128-byte rows, 16-byte chunk c of row r stored at position
// c ^ ((r >> 1) & 7) (conflict-free ds_read_b128 of 32-row fragments); since the DMA writes lane-linear, the swizzle
// is applied to the per-lane SOURCE address (lane l of an 8-row piece lands at row l>>3, position l&7).
// KS = 1: 4 waves, each owns a 32 x (BN / WN) output tile for the whole K range.
// KS = 2: 8 waves; waves 4..7 shadow waves 0..3 on the same output tile but multiply the second half of every
//         64-deep stage (k-steps 2,3), so each SIMD hosts two independent MFMA / ds_read streams that cover each
//         other's LDS latency; the two partial accumulators are summed once through LDS before the epilogue.
// PP (KS = 2 only): "ping-pong" - the second K-half group runs its MFMAs one phase late (on the fragments it read in the
//         previous stage), so that on every SIMD one wave is in its LDS-read phase while the other is in its MFMA phase:
//         the LDS port (192 KB of fragment reads + 74 KB of DMA writes per stage) and the MFMA pipe work concurrently
//         instead of alternately.
// M16 (128 x 160 tile, KS = 2): v_mfma_f32_16x16x32_bf16 with a 64 x 80 wave tile (4 x 5 tiles of 16 x 16) instead of
//         32x32x16 with 32 x 160: the same accumulator registers and MFMA cycles, but 18 instead of 24 ds_read_b128 of
//         fragments per wave and stage - the loop is LDS-port bound (per-stage stamps: tools/gemm_bench.py --stamps).
template <int BM, int BN, int NPASS, int KS, bool PP = false, bool M16 = false>
__global__ void __launch_bounds__(256 * KS, 1) wd_gemm2_kernel(const wd_gemm_args a, const int nbn, const int nbm) {
#if defined(__HIP_DEVICE_COMPILE__)  // (the buffer-resource type and builtins exist in the device pass only)
    static_assert(!M16 || (BM == 128 && BN == 160 && KS == 2 && !PP), "M16 is the 128x160 KS=2 kernel");
    constexpr int NPL = (NPASS == 1) ? 1 : 2;
    constexpr int NW = 4 * KS;
    constexpr int WM = BM / 32, WN = 4 / WM;
    constexpr int WCOLS = BN / WN;
    constexpr int TN = WCOLS / 32;
    static_assert(WCOLS % 32 == 0 && WM * WN == 4, "bad tile");
    constexpr int A_PIECES = BM / 8, B_PIECES = BN / 8;       // 8-row DMA pieces per plane
    constexpr int A_INS = (A_PIECES + NW - 1) / NW, B_INS = (B_PIECES + NW - 1) / NW;
    constexpr int A_PL = BM * 128;
    constexpr int B_PL = BN * 128;
    constexpr int STAGE = NPL * (A_PL + B_PL);
    constexpr int KK_PER = 4 / KS;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* s_tab = reinterpret_cast<int*>(smem + 2 * STAGE);  // [ntaps0][BM] source row of src[0] per tap, -1 = zero row

    const int ntile = nbn * nbm;
    const int nwg = ntile * a.ksplit;
    int wg;
    {
        const int bid = blockIdx.x;
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    // split-K across workgroups: slice `sidx` of the K stages of tile `wg / ksplit`.  The slices of a tile are neighbours in the
    // XCD-contiguous order above, so they normally share an XCD's L2 - where the in-launch combine (wd_epilogue_tail) reads the
    // slabs fastest; a speed choice only, the combine's release / acquire is placement-independent.
    const int sidx = wg % a.ksplit;
    wg /= a.ksplit;
    const int bn_i = wg % nbn, bm_i = wg / nbn;
    const int m0 = bm_i * BM, n0 = bn_i * BN;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = wave & 3, kh = wave >> 2;
    const int wm = wq / WN, wn = wq % WN;
    const int lrow = lane >> 3, lpos = lane & 7;

    // ---- source-row table of src[0] for this row panel (one global gather lookup per (tap, row), done once)
    {
        const int nt0 = a.src[0].ntaps;
        const int32_t* g0 = a.src[0].gather;
        const int hw_src0 = a.src[0].hw_src;
        const int Wimg = a.slab_rows;  // > 0: 3x3 / pad 1 / stride 1 over images Wimg wide (wd_gemm() checked): arithmetic table
        for (int idx = tid; idx < nt0 * BM; idx += 256 * KS) {
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

    // ---- the rows this lane feeds: piece (wave + NW * i) of 8 rows, for A and for W
    int a_sw[A_INS];
#pragma unroll
    for (int i = 0; i < A_INS; ++i) {
        const int row = (wave + NW * i) * 8 + lrow;
        a_sw[i] = (lpos ^ ((row >> 1) & 7)) * 8;  // source chunk (in elements) that lands at position lpos
    }
    // Operands are fetched with buffer_load ... lds: a buffer resource per plane in SGPRs, a per-lane 32-bit byte offset that
    // only changes when the tap does, and the stage's position (channel chunk / K step) in the scalar offset - no per-stage
    // vector address arithmetic at all.  Padding and out-of-range rows carry an offset beyond num_records: the hardware
    // returns zeros for them (raw buffer range check on the vector offset), which replaces the zero-line select.
    // (wd_gemm() rejects operands whose plane does not fit 31-bit byte offsets.)
    constexpr uint32_t WD_OOB = 0x80000000u;
    auto make_srd = [](const wd_bf16* p) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<wd_bf16*>(p), 0, 0x7FFFFFF0, 0x00020000);
    };
    uint32_t b_voff[B_INS];
#pragma unroll
    for (int i = 0; i < B_INS; ++i) {
        const int row = (wave + NW * i) * 8 + lrow;
        const int n = n0 + row;
        b_voff[i] = ((row < BN) && (n < a.n)) ? (uint32_t)(((long)n * a.ktot + (lpos ^ ((row >> 1) & 7)) * 8) * 2) : WD_OOB;
    }
    const __amdgpu_buffer_rsrc_t srd_w_hi = make_srd(a.w_hi), srd_w_lo = make_srd(a.w_lo ? a.w_lo : a.w_hi);

    const int nk_all = a.ktot / BK2;
    const int k_begin = (int)((long)nk_all * sidx / a.ksplit), k_end = (int)((long)nk_all * (sidx + 1) / a.ksplit);
    int s = 0, tap = 0, kc = 0;
    const wd_bf16* cur_hi = a.src[0].hi;
    const wd_bf16* cur_lo = a.src[0].lo;
    int cur_ld = a.src[0].ld, cur_c = a.src[0].c, cur_nt = a.src[0].ntaps;
    {   // (source, tap, chunk) of the first stage of this slice
        const int cpt = a.src[0].c / BK2, n0st = a.src[0].ntaps * cpt;
        if (k_begin < n0st) {
            tap = k_begin / cpt;
            kc = k_begin - tap * cpt;
        } else {
            s = 1;
            kc = k_begin - n0st;
            cur_hi = a.src[1].hi;
            cur_lo = a.src[1].lo;
            cur_ld = a.src[1].ld;
            cur_c = a.src[1].c;
            cur_nt = a.src[1].ntaps;
        }
    }
    __amdgpu_buffer_rsrc_t srd_a_hi = make_srd(cur_hi), srd_a_lo = make_srd(cur_lo ? cur_lo : cur_hi);
    uint32_t a_voff[A_INS];  // byte offset of this lane's chunk of its source row, WD_OOB = zero row

    auto locate = [&]() {
#pragma unroll
        for (int i = 0; i < A_INS; ++i) {
            const int row = (wave + NW * i) * 8 + lrow;
            int r = -1;
            if (row < BM) {
                if (s == 0) r = s_tab[tap * BM + row];
                else r = (m0 + row < a.m) ? m0 + row : -1;  // src[1] is an identity source (1x1 skip)
            }
            a_voff[i] = r >= 0 ? (uint32_t)r * (uint32_t)(cur_ld * 2) + (uint32_t)(a_sw[i] * 2) : WD_OOB;
        }
    };
    locate();

    // One stage = NSLOT DMA pieces for this wave (A hi/lo pieces first, then W hi/lo).  What the next stage needs is captured
    // up front (prep: offsets, scalar offsets, the A resources - advance() may move on to the next tap / source before the
    // pieces are issued), the loads themselves are issued one by one BETWEEN the MFMA groups of the current stage (fire), so
    // that DMA issue hides in the MFMA pipe's shadow instead of preceding it as a burst.
    constexpr int NSLOT = NPL * (A_INS + B_INS);
    uint32_t pva[A_INS];        // captured a_voff of the prepared stage
    int soff_a = 0, soff_b = 0;  // captured scalar byte offsets (channel chunk of A, K step of W)
    __amdgpu_buffer_rsrc_t fa_hi = srd_a_hi, fa_lo = srd_a_lo;
    int pdst[NSLOT];            // wave-uniform LDS byte offset inside the stage, < 0: this wave has no such piece
    auto prep = [&](int kit) {
#pragma unroll
        for (int i = 0; i < A_INS; ++i) {
            const int piece = wave + NW * i;
            pva[i] = a_voff[i];
#pragma unroll
            for (int p = 0; p < NPL; ++p) pdst[i * NPL + p] = piece < A_PIECES ? p * A_PL + piece * 1024 : -1;
        }
#pragma unroll
        for (int i = 0; i < B_INS; ++i) {
            const int piece = wave + NW * i;
#pragma unroll
            for (int p = 0; p < NPL; ++p)
                pdst[A_INS * NPL + i * NPL + p] = piece < B_PIECES ? NPL * A_PL + p * B_PL + piece * 1024 : -1;
        }
        soff_a = kc * BK2 * 2;
        soff_b = kit * BK2 * 2;
        fa_hi = srd_a_hi;
        fa_lo = srd_a_lo;
    };
    auto fire = [&](int sl, char* sbase) {  // sl is a compile-time constant at every call site (unrolled loops)
        if (pdst[sl] < 0) return;
        const int p = sl % NPL;
        if (sl < A_INS * NPL)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(p ? fa_lo : fa_hi, (wd_lds_ptr)(sbase + pdst[sl]), 16, pva[sl / NPL], soff_a, 0, 0);
        else
            __builtin_amdgcn_raw_ptr_buffer_load_lds(p ? srd_w_lo : srd_w_hi, (wd_lds_ptr)(sbase + pdst[sl]), 16,
                                                     b_voff[(sl - A_INS * NPL) / NPL], soff_b, 0, 0);
    };
    // address computation and issue in one go (nothing captured)
    auto prep_fire_all = [&](int kit, char* sbase) {
#pragma unroll
        for (int i = 0; i < A_INS; ++i) {
            const int piece = wave + NW * i;
            if (piece < A_PIECES) {
#pragma unroll
                for (int p = 0; p < NPL; ++p)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(p ? srd_a_lo : srd_a_hi, (wd_lds_ptr)(sbase + p * A_PL + piece * 1024), 16,
                                                             a_voff[i], kc * BK2 * 2, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < B_INS; ++i) {
            const int piece = wave + NW * i;
            if (piece < B_PIECES) {
#pragma unroll
                for (int p = 0; p < NPL; ++p)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(p ? srd_w_lo : srd_w_hi,
                                                             (wd_lds_ptr)(sbase + NPL * A_PL + p * B_PL + piece * 1024), 16, b_voff[i],
                                                             kit * BK2 * 2, 0, 0);
            }
        }
    };
    auto advance = [&]() {
        ++kc;
        if (kc * BK2 == cur_c) {
            kc = 0;
            ++tap;
            if (tap == cur_nt) {
                tap = 0;
                ++s;
                if (s < a.nsrc) {
                    cur_hi = a.src[1].hi;
                    cur_lo = a.src[1].lo;
                    cur_ld = a.src[1].ld;
                    cur_c = a.src[1].c;
                    cur_nt = a.src[1].ntaps;
                    srd_a_hi = make_srd(cur_hi);
                    srd_a_lo = make_srd(cur_lo ? cur_lo : cur_hi);
                }
            }
            if (s < a.nsrc) locate();
        }
    };

    f32x16 acc[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    f32x4 acc16[M16 ? 4 : 1][M16 ? 5 : 1];
#pragma unroll
    for (int i = 0; i < (M16 ? 4 : 1); ++i)
#pragma unroll
        for (int t = 0; t < (M16 ? 5 : 1); ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc16[i][t][r] = 0.0f;

    const int nk = k_end - k_begin;
    if (nk > 0) {
        prep(k_begin);
        advance();
#pragma unroll
        for (int sl = 0; sl < NSLOT; ++sl) fire(sl, smem);
    }

    const int frow = lane & 31, fhalf = lane >> 5;
    constexpr int NGRP = KK_PER * TN;  // MFMA groups (one 32x32 tile x one 16-deep k-step) of this wave per stage
    bf16x8 fa[KK_PER][NPL], fb[KK_PER][TN][NPL];
    auto read_frags = [&](const char* base) {
#pragma unroll
        for (int k2 = 0; k2 < KK_PER; ++k2) {
            const int ch = (kh * KK_PER + k2) * 2 + fhalf;
            const int ao = lds_off2(wm * 32 + frow, ch);
#pragma unroll
            for (int p = 0; p < NPL; ++p) fa[k2][p] = *reinterpret_cast<const bf16x8*>(base + p * A_PL + ao);
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                const int bo = NPL * A_PL + lds_off2(wn * WCOLS + t * 32 + frow, ch);
#pragma unroll
                for (int p = 0; p < NPL; ++p) fb[k2][t][p] = *reinterpret_cast<const bf16x8*>(base + p * B_PL + bo);
            }
        }
    };
    auto mfma_stage = [&](bool more, char* nbase) {
#pragma unroll
        for (int g = 0; g < NGRP; ++g) {
            const int k2 = g / TN, t = g % TN;
            if (NPL == 2) {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[k2][NPL - 1], fb[k2][t][0], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[k2][0], fb[k2][t][NPL - 1], acc[t], 0, 0, 0);
            }
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[k2][0], fb[k2][t][0], acc[t], 0, 0, 0);
            // spread this wave's DMA pieces of the next stage over the MFMA groups
            if (more) {
#pragma unroll
                for (int sl = g * NSLOT / NGRP; sl < (g + 1) * NSLOT / NGRP; ++sl) fire(sl, nbase);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    if constexpr (M16) {
        // wave = (K-half kh, row half wq >> 1, column half wq & 1): 64 rows x 80 columns, one 32-deep k-step per stage
        const int l15 = lane & 15, lq = lane >> 4;
        const int r0w = (wq >> 1) * 64, c0w = (wq & 1) * 80;
        bf16x8 xa[4][NPL], xb[5][NPL];
        auto read16 = [&](const char* base) {
            const int ch = kh * 4 + lq;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ao = lds_off2(r0w + i * 16 + l15, ch);
#pragma unroll
                for (int p = 0; p < NPL; ++p) xa[i][p] = *reinterpret_cast<const bf16x8*>(base + p * A_PL + ao);
            }
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                const int bo = NPL * A_PL + lds_off2(c0w + t * 16 + l15, ch);
#pragma unroll
                for (int p = 0; p < NPL; ++p) xb[t][p] = *reinterpret_cast<const bf16x8*>(base + p * B_PL + bo);
            }
        };
        auto mfma16 = [&](bool more, char* nbase) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    if (NPL == 2) {
                        acc16[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[i][NPL - 1], xb[t][0], acc16[i][t], 0, 0, 0);
                        acc16[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[i][0], xb[t][NPL - 1], acc16[i][t], 0, 0, 0);
                    }
                    acc16[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[i][0], xb[t][0], acc16[i][t], 0, 0, 0);
                }
                if (more) {  // this wave's DMA pieces of the next stage, spread over the four row groups
#pragma unroll
                    for (int sl = i * NSLOT / 4; sl < (i + 1) * NSLOT / 4; ++sl) fire(sl, nbase);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        const bool stamp16 = (a.dbg & WD_DBG_STAMPS) && blockIdx.x == 0 && lane == 0 && a.ws;
        unsigned long long* sb16 = reinterpret_cast<unsigned long long*>(a.ws) + (long)wave * nk * 4;
        if (a.dbg & WD_DBG_STAGGER ? kh == 1 : false) {
            // stagger (a.dbg & WD_DBG_STAGGER): the second K-half group multiplies one stage late, so its LDS reads fall under the
            // first group's MFMAs and vice versa.  It keeps TWO fragment sets and alternates between them, so the reads of
            // stage k never wait for the MFMAs of stage k-1 to have consumed their operands (the loop is unrolled by two to
            // keep the register indices static).
            bf16x8 ya[4][NPL], yb[5][NPL];
            auto read16g = [&](auto& fa_, auto& fb_, const char* base) {
                const int ch = kh * 4 + lq;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ao = lds_off2(r0w + i * 16 + l15, ch);
#pragma unroll
                    for (int p = 0; p < NPL; ++p) fa_[i][p] = *reinterpret_cast<const bf16x8*>(base + p * A_PL + ao);
                }
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    const int bo = NPL * A_PL + lds_off2(c0w + t * 16 + l15, ch);
#pragma unroll
                    for (int p = 0; p < NPL; ++p) fb_[t][p] = *reinterpret_cast<const bf16x8*>(base + p * B_PL + bo);
                }
            };
            auto mfma16g = [&](auto& fa_, auto& fb_) {
    #pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int t = 0; t < 5; ++t) {
                        if (NPL == 2) {
                            acc16[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_[i][NPL - 1], fb_[t][0], acc16[i][t], 0, 0, 0);
                            acc16[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_[i][0], fb_[t][NPL - 1], acc16[i][t], 0, 0, 0);
                        }
                        acc16[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_[i][0], fb_[t][0], acc16[i][t], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                };
            auto half_step = [&](int kit, auto& rd_a, auto& rd_b, auto& mm_a, auto& mm_b) {
                if (stamp16) sb16[kit * 4 + 0] = __builtin_amdgcn_s_memtime();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (stamp16) sb16[kit * 4 + 1] = __builtin_amdgcn_s_memtime();
                const char* base = smem + (kit & 1) * STAGE;
                char* nbase = smem + ((kit + 1) & 1) * STAGE;
                // the late group's DMA of the next stage goes out first (the buffer is free as of this barrier and the pieces
                // then have the whole stage to land), then this stage's fragment reads into the fragment set the MFMAs below do not
                // use, then the previous stage's products: the reads are in flight under them (measured: 3220 cycles per stage
                // against 3460 with the products first and 3570 with a single fragment set)
                if (kit + 1 < nk) {
                    prep_fire_all(k_begin + kit + 1, nbase);
                    advance();
                }
                __builtin_amdgcn_sched_barrier(0);
                read16g(rd_a, rd_b, base);
                __builtin_amdgcn_sched_barrier(0);
                if (stamp16) sb16[kit * 4 + 2] = __builtin_amdgcn_s_memtime();
                if (kit > 0) mfma16g(mm_a, mm_b);
                __builtin_amdgcn_sched_barrier(0);
                if (stamp16) {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    sb16[kit * 4 + 3] = __builtin_amdgcn_s_memtime();
                }
            };
            for (int kit = 0; kit < nk; kit += 2) {
                half_step(kit, xa, xb, ya, yb);
                if (kit + 1 < nk) half_step(kit + 1, ya, yb, xa, xb);
            }
            if (nk > 0) {
                if (nk & 1) mfma16g(xa, xb);
                else mfma16g(ya, yb);
            }
        } else {
            for (int kit = 0; kit < nk; ++kit) {
                if (stamp16) sb16[kit * 4 + 0] = __builtin_amdgcn_s_memtime();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // step kit has landed, the other stage buffer is free
                if (stamp16) sb16[kit * 4 + 1] = __builtin_amdgcn_s_memtime();
                const bool more = kit + 1 < nk;
                const char* base = smem + (kit & 1) * STAGE;
                char* nbase = smem + ((kit + 1) & 1) * STAGE;
                if (more) {
                    prep(k_begin + kit + 1);
                    advance();
                }
                read16(base);
                __builtin_amdgcn_sched_barrier(0);
                if (stamp16) {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    sb16[kit * 4 + 2] = __builtin_amdgcn_s_memtime();
                }
                mfma16(more, nbase);
                if (stamp16) sb16[kit * 4 + 3] = __builtin_amdgcn_s_memtime();
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
                            *pe = (hh == 0) ? acc16[i][t][r] : *pe + acc16[i][t][r];
                        }
            }
            __syncthreads();
        }
        wd_epilogue_tail<BM, BN, 256 * KS>(a, ep, m0, n0, tid, sidx);
        return;
    }
    if (PP && KS == 2 && kh == 1) {
        // late group (its own loop, so that the fragments carried across the barrier do not constrain the early group's
        // register allocation): multiply the fragments of the previous stage while the early group reads this one; only
        // then (fragments dead) compute and issue its share of the next stage's DMA, then read this stage
        const bool stamp_l = (a.dbg & WD_DBG_STAMPS) && blockIdx.x == 0 && lane == 0 && a.ws;
        unsigned long long* sbuf_l = reinterpret_cast<unsigned long long*>(a.ws) + (long)wave * nk * 4;
        for (int kit = 0; kit < nk; ++kit) {
            if (stamp_l) sbuf_l[kit * 4 + 0] = __builtin_amdgcn_s_memtime();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (stamp_l) sbuf_l[kit * 4 + 1] = __builtin_amdgcn_s_memtime();
            const bool more = kit + 1 < nk;
            const char* base = smem + (kit & 1) * STAGE;
            char* nbase = smem + ((kit + 1) & 1) * STAGE;
            if (kit > 0) mfma_stage(false, nbase);
            __builtin_amdgcn_sched_barrier(0);
            if (stamp_l) sbuf_l[kit * 4 + 2] = __builtin_amdgcn_s_memtime();   // (late group: [1..2] = MFMA, [2..3] = DMA + reads)
            if (more) {
                prep(k_begin + kit + 1);
                advance();
#pragma unroll
                for (int sl = 0; sl < NSLOT; ++sl) fire(sl, nbase);
            }
            __builtin_amdgcn_sched_barrier(0);
            read_frags(base);
            if (stamp_l) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                sbuf_l[kit * 4 + 3] = __builtin_amdgcn_s_memtime();
            }
        }
        if (nk > 0) mfma_stage(false, smem);
    } else {
        // (a.dbg & WD_DBG_STAMPS: per-stage cycle stamps of workgroup 0 into a.ws as u64 [wave][stage][4] - tools/gemm_bench.py --stamps)
        const bool stamp = (a.dbg & WD_DBG_STAMPS) && blockIdx.x == 0 && lane == 0 && a.ws;
        unsigned long long* sbuf = reinterpret_cast<unsigned long long*>(a.ws) + (long)wave * nk * 4;
        for (int kit = 0; kit < nk; ++kit) {
            if (stamp) sbuf[kit * 4 + 0] = __builtin_amdgcn_s_memtime();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // step kit has landed, the other stage buffer is free
            if (stamp) sbuf[kit * 4 + 1] = __builtin_amdgcn_s_memtime();
            const bool more = kit + 1 < nk;
            const char* base = smem + (kit & 1) * STAGE;
            char* nbase = smem + ((kit + 1) & 1) * STAGE;
            if (more) {
                prep(k_begin + kit + 1);
                advance();
            }
            read_frags(base);
            __builtin_amdgcn_sched_barrier(0);
            if (stamp) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                sbuf[kit * 4 + 2] = __builtin_amdgcn_s_memtime();
            }
            mfma_stage(more, nbase);
            if (stamp) sbuf[kit * 4 + 3] = __builtin_amdgcn_s_memtime();
        }
    }

    wd_epilogue_lds<BM, BN, TN, 256 * KS>(a, acc, smem, m0, n0, wm, wn, WCOLS, kh, KS, tid, sidx);
#endif
}

template <int BM, int BN, int NPASS, int KS, bool PP = false, bool M16 = false>
int launch2(const wd_gemm_args& a, hipStream_t st) {
    constexpr int NPL = (NPASS == 1) ? 1 : 2;
    constexpr int loop_smem = 2 * NPL * (BM + BN) * 128 + 9 * BM * 4;
    constexpr int red_smem = BM * (BN + 4) * 4 + WD_STAT_SCRATCH;  // fp32 epilogue image (+ statistics scratch) overlays the stages
    constexpr int smem = loop_smem > red_smem ? loop_smem : red_smem;
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&wd_gemm2_kernel<BM, BN, NPASS, KS, PP, M16>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess)
            return WD_ELAUNCH;
        attr_done = true;
    }
    const int nbn = (a.n + BN - 1) / BN, nbm = (a.m + BM - 1) / BM;
    {
        WdLaunchScope scope((BM == 128 && BN == 160) ? WD_CLS_GEMM : WD_CLS_GEMM_OTHER, st,
                            2.0 * (double)a.m * (double)a.n * (double)a.ktot);
        hipLaunchKernelGGL((wd_gemm2_kernel<BM, BN, NPASS, KS, PP, M16>), dim3(nbn * nbm * a.ksplit), dim3(256 * KS), smem, st, a,
                           nbn, nbm);
    }
    if (a.ksplit > 1 && !a.tickets) {
        // the combine pass is pure streaming: narrow column tiles so that it fills the chip (whole statistics groups
        // per tile when the GroupNorm sums are fused in)
        return wd_gemm_launch_reduce(a, st, BM, BN);
    }
    return wd_check_launch();
}

// ---- opt-in forms that lost their A/B against the defaults, compiled with -DWDIFF_EXPERIMENTAL only: the ping-pong
// instantiations of wd_gemm2_kernel (K_PP) and the slab kernel (K_SLAB).  The slab kernel lives here and not in wd_gemm_exp.hip
// for the same reason wd_gemm_kernel does: see the head of this file.
#ifdef WDIFF_EXPERIMENTAL
template <int BM, int BN>
int launch2_pp(const wd_gemm_args& a, hipStream_t st) {
    return a.npass == 3 ? launch2<BM, BN, 3, 2, true>(a, st) : launch2<BM, BN, 1, 2, true>(a, st);
}

// ======================================================================================================
// v3 "slab" kernel: the A operand of a 3x3 convolution is NOT re-fetched per tap.  For a panel of BM output rows
// the union of source rows over all taps is a short contiguous range (a few image rows + halo): that slab is
// DMA'd into LDS once per 32-channel chunk (double buffered, prefetched one chunk ahead) and all nine taps read
// their shifted A fragments from it through a per-(tap,row) LDS table.  Only the weights stream per tap, through
// a 4-deep LDS ring kept full with counted s_waitcnt vmcnt(N) + raw s_barrier (no full drain in the loop).
// Weights are stored in consumption order [chunk][tap][N][32] so that one stage is one contiguous block.
// L2->LDS bytes per MFMA drop ~2.8x against v2; linears (one tap) run through the same code.
constexpr int CK3 = 32;
constexpr int RING3 = 4;

__device__ __forceinline__ void wd_wait_vmcnt(int n) {  // n is wave-uniform
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
        case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
        case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
        case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
        case 13: asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); break;
        case 14: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;
        case 15: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); break;
        case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
        case 17: asm volatile("s_waitcnt vmcnt(17)" ::: "memory"); break;
        case 18: asm volatile("s_waitcnt vmcnt(18)" ::: "memory"); break;
        case 19: asm volatile("s_waitcnt vmcnt(19)" ::: "memory"); break;
        case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;  // stricter than needed, still correct
    }
}

template <int BM, int BN, int NPASS, int SLABR, int KS>
__global__ void __launch_bounds__(256 * KS, 1) wd_gemm3_kernel(const wd_gemm_args a, const int nbn, const int nbm) {
    constexpr int NPL = (NPASS == 1) ? 1 : 2;
    constexpr int NW = 4 * KS, NT = 256 * KS;
    constexpr int WM = BM / 32, WN = 4 / WM;
    constexpr int WCOLS = BN / WN;
    constexpr int TN = WCOLS / 32;
    static_assert(WCOLS % 32 == 0 && WM * WN == 4, "bad tile");
    constexpr int SLAB_PL = (SLABR + 1) * 64;          // one plane of one slab buffer (+ the all-zero row)
    constexpr int SLAB_BUF = NPL * SLAB_PL;
    constexpr int W_PL = BN * 64;
    constexpr int W_SLOT = NPL * W_PL;
    constexpr int OFF_RING = 2 * SLAB_BUF;
    constexpr int OFF_TAB = OFF_RING + RING3 * W_SLOT;
    constexpr int W_PIECES = NPL * (BN / 16);            // 1 KB DMA pieces per W stage
    constexpr int W_INS = (W_PIECES + NW - 1) / NW;
    constexpr int S_PIECES_MAX = NPL * ((SLABR + 15) / 16);
    constexpr int S_INS = (S_PIECES_MAX + NW - 1) / NW;
    constexpr int KK_PER = 2 / KS;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* s_tab = reinterpret_cast<int*>(smem + OFF_TAB);   // [ntaps0][BM] slab-local row, SLABR = zero row
    int* s_misc = s_tab + 9 * BM;                          // [0] = min source row of the panel

    const int nwg = nbn * nbm;
    int wg;
    {
        const int bid = blockIdx.x;
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int bn_i = wg % nbn, bm_i = wg / nbn;
    const int m0 = bm_i * BM, n0 = bn_i * BN;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = wave & 3, kh = wave >> 2;
    const int wm = wq / WN, wn = wq % WN;
    const int prow = lane >> 2, ppos = lane & 3;  // row / 16-byte position of this lane inside a 16-row DMA piece

    const int dbg = a.dbg;  // timing-only ablation switches (tools/gemm_bench.py --dbg), 0 in production
    const int nt0 = a.src[0].ntaps;
    const int c0chunks = a.src[0].c / CK3;
    const int c1chunks = a.nsrc > 1 ? a.src[1].c / CK3 : 0;
    const int nstage = (dbg & 32) ? 0 : c0chunks * nt0 + c1chunks;
    if (dbg & 128) return;

    // ---- table of source rows, panel minimum, zero rows
    if (tid == 0) s_misc[0] = 0x7fffffff;
    for (int i = tid; i < 2 * NPL * 16; i += NT) {  // the zero row of every slab buffer / plane (64 B each)
        const int which = i >> 4, w = i & 15;
        reinterpret_cast<int*>(smem + which * SLAB_PL + SLABR * 64)[w] = 0;
    }
    __syncthreads();
    {
        const int32_t* g0 = a.src[0].gather;
        const int hw_src0 = a.src[0].hw_src;
        int mn = 0x7fffffff;
        for (int idx = tid; idx < nt0 * BM; idx += NT) {
            const int t = idx / BM, row = idx - t * BM;
            const int m = m0 + row;
            int v = -1;
            if (m < a.m) {
                if (g0) {
                    const int b = m / a.hw_out, p = m - b * a.hw_out;
                    const int g = g0[t * a.hw_out + p];
                    if (g >= 0) v = b * hw_src0 + g;
                } else {
                    v = m;
                }
            }
            s_tab[idx] = v;
            if (v >= 0) mn = min(mn, v);
        }
        atomicMin(&s_misc[0], mn);
    }
    __syncthreads();
    const int rlo = s_misc[0];
    for (int idx = tid; idx < nt0 * BM; idx += NT) {
        const int v = s_tab[idx];
        int l = SLABR;
        if (v >= 0 && v - rlo < SLABR) l = v - rlo;  // (span is validated by the host; out-of-span rows read zeros)
        s_tab[idx] = l;
    }
    // rows of src[0] present in the slab: [rlo, rlo + span0); src[1] (identity): [m0, m0 + BM)
    const int span0 = min(SLABR, a.slab_rows);
    const long rows0 = (long)((a.src[0].gather ? (long)((a.m + a.hw_out - 1) / a.hw_out) * a.src[0].hw_src : (long)a.m));
    const wd_bf16* zline = reinterpret_cast<const wd_bf16*>(wd_zero_line) + ppos * 8;

    // DMA bookkeeping (all wave-uniform scalars): `issued` counts this wave's glds; mw0..mw3 are the values of
    // `issued` right after the W stages st, st+1, st+2, st+3 were issued; ms_cur / ms_nxt the same for the slab of
    // the current / next phase.  s_waitcnt vmcnt(issued - mark) == "everything up to that issue has landed".
    int issued = 0;
    int mw0 = 0, mw1 = 0, mw2 = 0, mw3 = 0;
    int ms_cur = 0, ms_nxt = 0;

    // slab of phase ph (source, chunk) -> buffer ph & 1
    auto issue_slab = [&](int ph) {
        const bool s1 = ph >= c0chunks;
        const int chunk = s1 ? ph - c0chunks : ph;
        const wd_bf16* hi = s1 ? a.src[1].hi : a.src[0].hi;
        const wd_bf16* lo = s1 ? a.src[1].lo : a.src[0].lo;
        const int ld = s1 ? a.src[1].ld : a.src[0].ld;
        const long base_row = s1 ? m0 : rlo;
        const int span = s1 ? BM : span0;
        const long row_lim = s1 ? (long)a.m : rows0;
        const int npieces = NPL * ((span + 15) / 16);
        char* sb = smem + (ph & 1) * SLAB_BUF;
#pragma unroll
        for (int i = 0; i < S_INS; ++i) {
            const int piece = wave + NW * i;  // wave-uniform
            if (piece < npieces) {
                const int pl = (NPL == 2) ? (piece & 1) : 0;
                const int rp = (NPL == 2) ? (piece >> 1) : piece;
                const int r = rp * 16 + prow;                       // slab row
                const long gr = base_row + r;
                const wd_bf16* src = (pl ? lo : hi);
                const wd_bf16* ptr = (r < span && gr < row_lim)
                                         ? src + gr * ld + chunk * CK3 + ((ppos ^ ((r >> 2) & 3)) << 3)
                                         : zline;
                __builtin_amdgcn_global_load_lds((wd_gbl_ptr)ptr, (wd_lds_ptr)(sb + pl * SLAB_PL + rp * 1024), 16, 0, 0);
                ++issued;
            }
        }
        ms_nxt = issued;
    };
    // W stage st (consumption order) -> ring slot st % RING3.  Global block st: [N][32] per plane, contiguous.
    auto issue_w = [&](int st) {
        char* rb = smem + OFF_RING + (st % RING3) * W_SLOT;
        const long blk = (long)st * a.n * CK3;
#pragma unroll
        for (int i = 0; i < W_INS; ++i) {
            const int piece = wave + NW * i;
            if (piece < W_PIECES) {
                const int pl = (NPL == 2) ? (piece & 1) : 0;
                const int rp = (NPL == 2) ? (piece >> 1) : piece;
                const int r = rp * 16 + prow;  // row inside the BN tile
                const int n = n0 + r;
                const wd_bf16* src = pl ? a.w_lo : a.w_hi;
                const wd_bf16* ptr = (n < a.n) ? src + blk + (long)n * CK3 + ((ppos ^ ((r >> 2) & 3)) << 3) : zline;
                __builtin_amdgcn_global_load_lds((wd_gbl_ptr)ptr, (wd_lds_ptr)(rb + pl * W_PL + rp * 1024), 16, 0, 0);
                ++issued;
            }
        }
        mw3 = issued;
    };

    f32x16 acc[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    __syncthreads();  // table finalised (also orders the zero-row writes before any fragment read)
    issue_slab(0);
    ms_cur = ms_nxt;
    if (0 < nstage) { issue_w(0); mw0 = mw3; }
    if (1 < nstage) { issue_w(1); mw1 = mw3; }
    if (2 < nstage) { issue_w(2); mw2 = mw3; }

    const int frow = lane & 31, fhalf = lane >> 5;
    const int arow = wm * 32 + frow;
    int ph = 0, tap = 0;       // phase / tap of the current stage
    int ntap_ph = nt0;         // taps in the current phase
    auto next_stage = [&]() {
        mw0 = mw1;
        mw1 = mw2;
        mw2 = mw3;
        if (++tap == ntap_ph) {
            tap = 0;
            ++ph;
            ntap_ph = ph < c0chunks ? nt0 : 1;
            ms_cur = ms_nxt;
        }
    };
    for (int st = 0; st < nstage; ++st) {
        // ---- wait until stage st's weights and its phase's slab have landed (everything younger may stay in flight)
        wd_wait_vmcnt(issued - max(mw0, ms_cur));
        if (!(dbg & 16)) __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // ---- refill: the slot of stage st-1 and (at a phase start) the other slab buffer are free now
        if (tap == 0 && ph + 1 < c0chunks + c1chunks && !(dbg & 8)) issue_slab(ph + 1);
        if (st + RING3 - 1 < nstage && !(dbg & 4)) issue_w(st + RING3 - 1);

        // ---- multiply stage st
        const char* sb = smem + (ph & 1) * SLAB_BUF;
        const char* rb = smem + OFF_RING + (st % RING3) * W_SLOT;
        int idx;
        if (ph < c0chunks) idx = s_tab[tap * BM + arow];
        else idx = (m0 + arow < a.m) ? arow : SLABR;
        const int abase = idx * 64, asw = (idx >> 2) & 3;
        // all fragments of this wave's k-steps first (the MFMAs then drain them behind counted lgkmcnt waits) ...
        bf16x8 fa[KK_PER][NPL], fb[KK_PER][TN][NPL];
        if (dbg & 2) { next_stage(); continue; }
#pragma unroll
        for (int k2 = 0; k2 < KK_PER; ++k2) {
            const int ch = (kh * KK_PER + k2) * 2 + fhalf;
            const int ao = abase + ((ch ^ asw) << 4);
#pragma unroll
            for (int p = 0; p < NPL; ++p) fa[k2][p] = *reinterpret_cast<const bf16x8*>(sb + p * SLAB_PL + ao);
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                const int bo = lds_off(wn * WCOLS + t * 32 + frow, ch);
#pragma unroll
                for (int p = 0; p < NPL; ++p) fb[k2][t][p] = *reinterpret_cast<const bf16x8*>(rb + p * W_PL + bo);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (dbg & 1) {
#pragma unroll
            for (int k2 = 0; k2 < KK_PER; ++k2) {
                asm volatile("" ::"v"(fa[k2][0]), "v"(fa[k2][NPL - 1]));
#pragma unroll
                for (int t = 0; t < TN; ++t) asm volatile("" ::"v"(fb[k2][t][0]), "v"(fb[k2][t][NPL - 1]));
            }
            next_stage();
            continue;
        }
        // ... then the multiply block
#pragma unroll
        for (int k2 = 0; k2 < KK_PER; ++k2) {
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                if (NPL == 2) {
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[k2][NPL - 1], fb[k2][t][0], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[k2][0], fb[k2][t][NPL - 1], acc[t], 0, 0, 0);
                }
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[k2][0], fb[k2][t][0], acc[t], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        next_stage();
    }
    if (dbg & 64) {
        if (acc[0][0] == 123.456f) a.out_f32[0] = acc[0][1];
        return;
    }
    wd_epilogue_lds<BM, BN, TN, NT>(a, acc, smem, m0, n0, wm, wn, WCOLS, kh, KS, tid);
}

template <int BM, int BN, int NPASS, int SLABR, int KS>
int launch3(const wd_gemm_args& a, hipStream_t st) {
    constexpr int NPL = (NPASS == 1) ? 1 : 2;
    constexpr int loop_smem = 2 * NPL * (SLABR + 1) * 64 + RING3 * NPL * BN * 64 + 9 * BM * 4 + 64;
    constexpr int red_smem = BM * (BN + 4) * 4 + WD_STAT_SCRATCH;
    constexpr int smem = loop_smem > red_smem ? loop_smem : red_smem;
    static_assert(smem <= 160 * 1024, "LDS budget");
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&wd_gemm3_kernel<BM, BN, NPASS, SLABR, KS>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess)
            return WD_ELAUNCH;
        attr_done = true;
    }
    const int nbn = (a.n + BN - 1) / BN, nbm = (a.m + BM - 1) / BM;
    WdLaunchScope scope(WD_CLS_GEMM_OTHER, st, 2.0 * (double)a.m * (double)a.n * (double)a.ktot);
    hipLaunchKernelGGL((wd_gemm3_kernel<BM, BN, NPASS, SLABR, KS>), dim3(nbn * nbm), dim3(256 * KS), smem, st, a, nbn,
                       nbm);
    return wd_check_launch();
}

template <int BM, int BN>
int launch3_tile(const wd_gemm_args& a, hipStream_t st, const int ks) {
    const bool p3 = a.npass == 3;
    if (ks == 1) return p3 ? launch3<BM, BN, 3, 192, 1>(a, st) : launch3<BM, BN, 1, 192, 1>(a, st);
    return p3 ? launch3<BM, BN, 3, 192, 2>(a, st) : launch3<BM, BN, 1, 192, 2>(a, st);
}

#else
template <int BM, int BN>
int launch2_pp(const wd_gemm_args&, hipStream_t) { return WD_EINVAL; }  // (the ping-pong form is an experimental build option)
#endif  // WDIFF_EXPERIMENTAL

template <int BM, int BN>
int launch2_tile(const wd_gemm_args& a, hipStream_t st, const int ks, const bool pp) {
    const bool p3 = a.npass == 3;
    if (pp) return launch2_pp<BM, BN>(a, st);
    if (ks == 2) return p3 ? launch2<BM, BN, 3, 2>(a, st) : launch2<BM, BN, 1, 2>(a, st);
    return p3 ? launch2<BM, BN, 3, 1>(a, st) : launch2<BM, BN, 1, 1>(a, st);
}

}  // namespace

int wd_gemm2_launch(const wd_gemm_args& a, hipStream_t st, int ks, bool m16, bool pp) {
    if (m16) {
        if (a.tile != 128160) return WD_EINVAL;
        return a.npass == 3 ? launch2<128, 160, 3, 2, false, true>(a, st) : launch2<128, 160, 1, 2, false, true>(a, st);
    }
    switch (a.tile) {
        case 128064: return launch2_tile<128, 64>(a, st, ks, pp);
        case 128160: return launch2_tile<128, 160>(a, st, ks, pp);
        case 128128: return launch2_tile<128, 128>(a, st, ks, pp);
        case 64064: return launch2_tile<64, 64>(a, st, ks, pp);
    }
    return WD_EINVAL;
}

int wd_gemm1_launch(const wd_gemm_args& a, hipStream_t st) {
    const bool p3 = a.npass == 3;
    switch (a.tile) {
        case 128064: return p3 ? launch<128, 64, 3>(a, st) : launch<128, 64, 1>(a, st);
        case 128160: return p3 ? launch<128, 160, 3>(a, st) : launch<128, 160, 1>(a, st);
        case 128128: return p3 ? launch<128, 128, 3>(a, st) : launch<128, 128, 1>(a, st);
        case 64064: return p3 ? launch<64, 64, 3>(a, st) : launch<64, 64, 1>(a, st);
    }
    return WD_EINVAL;
}

#ifdef WDIFF_EXPERIMENTAL
int wd_gemm3_launch(const wd_gemm_args& a, hipStream_t st, int ks) {
    switch (a.tile) {
        case 128064: return launch3_tile<128, 64>(a, st, ks);
        case 128128: return launch3_tile<128, 128>(a, st, ks);
        case 128160: return launch3_tile<128, 160>(a, st, ks);
    }
    return WD_EINVAL;
}
#endif
