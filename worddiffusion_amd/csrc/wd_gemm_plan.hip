// Tap-gather GEMM on v_mfma_f32_32x32x16_bf16 with split-bf16 operands (gfx950): the host side.
//
//   out[m, n] = act( sum_k A[m, k] W[n, k] + bias[n] + rowvec[m / hw, n] + resid[m, n] )
//
// A is never materialised: for every 3x3 tap (or the single 1x1 "tap") a row of the output tile reads one
// row of a token-major activation plane through a per-position gather table, so same-size 3x3, stride-2 3x3,
// nearest-x2-then-3x3 and 1x1 convolutions, the 1x1 skip projection of a ResBlock (a second source appended
// along K) and plain linears are one kernel.  Replaces nn.Conv2d / nn.Linear of reference unet.py:595,621,632,
// 540,488,364,375,175-183,125,145,1201-1205,611.
//
// This file makes no HIP call and holds no device code: the environment switches, the planner (wd_gemm_resolve: every check and
// every decision of a launch, ending in one launch family) and wd_gemm(), which resolves and then calls that family's launcher
// (wd_gemm_priv.h).  The kernels: wd_gemm.hip (v1, v2 / M16), wd_gemm4.hip (v4), wd_gemmw.hip, wd_gemmq.hip, wd_gemm_reduce.hip
// (split-K combine) and, for the opt-in kernels of a WDIFF_EXPERIMENTAL build, wd_gemm_exp.hip and one block of wd_gemm.hip.
#include <stdint.h>
#include <stdlib.h>

#include "wd_common.h"
#include "wd_gemm_epi.h"
#include "wd_gemm_priv.h"

namespace {

// The environment switches of the GEMM family, each read once per process (WDIFF_GEMM_V1 alone is read per call, in staged_grid).
struct WdGemmSwitches {
    int ks = 2;                               // WDIFF_GEMM_KS: K-halves per workgroup of the v2 kernel; 1 = one, anything else two
    int v4 = 2;                               // WDIFF_GEMM_V4: wd_gemm4_kernel 0 never, 1 wherever legal, 2 when every CU gets two workgroups
    bool m16 = true;                          // WDIFF_GEMM_M16: the 16x16x32 form of the v2 kernel on 128 x 160 tiles
    bool pp = false;                          // WDIFF_GEMM_PP: the ping-pong form of the v2 kernel (experimental build; measured: no gain)
    bool stagger = true;                      // WDIFF_GEMM_STAGGER: K_M16's second K-half group runs one stage late ...
    int stagger_min = 10;                     // WDIFF_GEMM_STAGGER_MIN: ... from this many 64-deep stages per K slice on
    bool fuse_combine = false;                // WDIFF_GEMM_FUSE_COMBINE: the in-launch split-K combine (tickets) instead of the combine launch
    bool arith_tab = true;                    // WDIFF_GEMM_ARITH_TAB: the source-row table of a same-size 3x3 source computed, not looked up
    long ksplit_cap = WD_MAX_KSPLIT;          // WDIFF_KSPLIT_CAP: the finest K cut wd_auto_ksplit takes on long K loops
    bool gemmw_slab = WD_GEMMW_SLAB_DEFAULT;  // WDIFF_GEMMW_SLAB: the slab form of the 64 x 320 kernel where it fits
    bool epi_batch = WD_EPI_BATCH_DEFAULT;    // WDIFF_EPI_BATCH: the batched epilogue of the 64-row tiles where it is legal
    int conv3 = 0;                            // WDIFF_CONV3: wd_conv3_kernel for w_layout 2 (experimental build)
    int v8 = 0;                               // WDIFF_GEMM_V8: 1 = wd_gemm8_kernel wherever legal (experimental build)
};

void env(const char* name, int& v) { if (const char* e = getenv(name)) v = atoi(e); }
void env(const char* name, long& v) { if (const char* e = getenv(name)) v = atol(e); }
void env(const char* name, bool& v) { if (const char* e = getenv(name)) v = atoi(e) != 0; }

const WdGemmSwitches& wd_gemm_switches() {
    static const WdGemmSwitches sw = [] {
        WdGemmSwitches s;
        env("WDIFF_GEMM_KS", s.ks);
        env("WDIFF_GEMM_V4", s.v4);
        env("WDIFF_GEMM_M16", s.m16);
        env("WDIFF_GEMM_PP", s.pp);
        env("WDIFF_GEMM_STAGGER", s.stagger);
        env("WDIFF_GEMM_STAGGER_MIN", s.stagger_min);
        env("WDIFF_GEMM_FUSE_COMBINE", s.fuse_combine);
        env("WDIFF_GEMM_ARITH_TAB", s.arith_tab);
        env("WDIFF_KSPLIT_CAP", s.ksplit_cap);
        env("WDIFF_GEMMW_SLAB", s.gemmw_slab);
        env("WDIFF_EPI_BATCH", s.epi_batch);
        env("WDIFF_CONV3", s.conv3);
        env("WDIFF_GEMM_V8", s.v8);
        return s;
    }();
    return sw;
}

// the launch families of wd_gemm: wd_gemm_resolve picks one, wd_gemm runs it
enum WdKernel {
    K_GEMMQ,  // 64 x 80, all of K inside the workgroup (wd_gemmq_kernel; w_layout 3, tile 64080)
    K_GEMMW,  // weights straight to registers (wd_gemmw_kernel; w_layout 3, tile 64320 or 128160)
    K_V4,     // two co-resident 4-wave workgroups per CU (wd_gemm4_kernel; 128 x 160)
    K_M16,    // the 16x16x32 MFMA form of the v2 kernel (wd_gemm2_kernel<..., M16>; 128 x 160)
    K_V2,     // wd_gemm2_kernel with `ks` K-halves per workgroup
    K_V1,     // wd_gemm_kernel (K not a multiple of 64, or WDIFF_GEMM_V1)
    K_SLAB,   // WDIFF_EXPERIMENTAL: slab-order weights (wd_gemm3_kernel; w_layout 1)
    K_CONV3,  // WDIFF_EXPERIMENTAL: row-shared taps (wd_conv3_kernel)
    K_V8,     // WDIFF_EXPERIMENTAL: ring kernel with loader waves (wd_gemm8_kernel)
    K_PP,     // WDIFF_EXPERIMENTAL: wd_gemm2_kernel<..., PP>
};

struct WdResolved {
    wd_gemm_args a;  // the args as the kernel sees them: tile, ksplit, tickets, slab_rows and the dbg stagger bit resolved
    WdKernel kernel;
    int ks;          // K-halves per workgroup (K_V2, K_SLAB)
};

// what resolve_staged knows of a launch once its grid is fixed
struct WdStaged {
    bool conv3;   // the row-shared-taps kernel was asked for and fits (always false outside an experimental build)
    bool v2ok;    // the v2 / v4 kernels can run it: 64-deep stages, at most nine taps, an identity second source
    bool use_v4;  // tile 128160 and the two-workgroups-per-CU kernel takes it
    int nk64;     // 64-deep K stages
};

bool src1_identity(const wd_gemm_args& a) { return a.nsrc == 1 || (a.src[1].gather == nullptr && a.src[1].ntaps == 1); }

// src[0] is a 3x3 / pad 1 / stride 1 window over images slab_rows wide
bool src0_same3(const wd_gemm_args& a) {
    const wd_src& q0 = a.src[0];
    return q0.ntaps == 9 && q0.gather && a.slab_rows > 0 && q0.hw_src == a.hw_out && a.hw_out % a.slab_rows == 0;
}

}  // namespace

bool wd_want_epi_batch(int32_t& dbg) {
    const bool want = (dbg & WD_EPI_BATCH_OFF) ? false : (dbg & WD_EPI_BATCH_ON) ? true : wd_gemm_switches().epi_batch;
    dbg &= ~(WD_EPI_BATCH_OFF | WD_EPI_BATCH_ON);
    return want;
}

bool wd_want_gemmw_slab(int32_t& dbg) {
    const bool want = (dbg & WD_GEMMW_SLAB_OFF) ? false : (dbg & WD_GEMMW_SLAB_ON) ? true : wd_gemm_switches().gemmw_slab;
    dbg &= ~(WD_GEMMW_SLAB_OFF | WD_GEMMW_SLAB_ON);
    return want;
}

// the K cut wd_gemm picks by itself: fewer than 128 tiles (or exactly 128 on a long K loop) and at least 8 stages of 64
static int wd_auto_ksplit(const int tile, const int m, const int n, const int nk64, const long ws_floats) {
    const int bn = tile % 1000, bm = tile / 1000;
    const long tiles = (long)((m + bm - 1) / bm) * ((n + bn - 1) / bn);
    if (!((tiles < 128 || (tiles == 128 && nk64 >= 32)) && nk64 >= 8)) return 1;
    long sp = 256 / tiles;
    if (sp > nk64 / 4) sp = nk64 / 4;
    // reductions over the token dimension (the weight-gradient GEMMs of the training step: K = 4096 ... 16384 tokens, a handful of
    // output tiles) are cut as finely as it takes to put a workgroup on every CU; the short-K layers of the denoising step keep <= 8
    const long cap = nk64 >= 64 ? wd_gemm_switches().ksplit_cap : 8;
    if (sp > cap) sp = cap;
    while (sp > 1 && sp * m * n > ws_floats) --sp;
    return sp > 1 ? (int)sp : 1;
}

static int wd_auto_tile(const int m, const int n, const int nk64, const bool can_split_base, const long ws_floats) {
    // 128x160 when N allows it (A is re-read only N/160 times), else 128x64; when that leaves most CUs idle either
    // cut K across workgroups (needs a workspace and enough K per slice) or fall back to 64x64 tiles.
    int tile = (n % 160 == 0) ? 128160 : 128064;
    const long tiles = (long)((m + 127) / 128) * ((n + (tile % 1000) - 1) / (tile % 1000));
    const bool can_split = can_split_base && nk64 >= 8 && (long)2 * m * n <= ws_floats;
    if (tiles < 128 && !can_split && m > 64) tile = 64064;
    return tile;
}

// ---- the planner.  wd_gemm_resolve runs the steps below in this order; an earlier step fixes a.tile / a.ksplit / a.tickets for
// the later ones, and every refusal is the same WD_EINVAL.

// Step 1, the options that fix tile and ksplit before anything else looks at them.
static int resolve_options(wd_gemm_args& a) {
    if (a.ksplit < 0 || a.ksplit > WD_MAX_KSPLIT) return WD_EINVAL;
    if (a.w_layout == 3) {
        // fragment-major weights (wd_gemm_pack_w): the 64 x 320 weights-to-registers kernel only
        if (a.n % 80 || a.act == WD_ACT_GEGLU || (a.tile && a.tile != 64320 && a.tile != 128160 && a.tile != 64080) || a.ktot % 64)
            return WD_EINVAL;
        if (a.tile == 0) a.tile = (a.a32 || a.ln_gamma) ? 64320 : 128160;
        if (a.n % (a.tile % 1000)) return WD_EINVAL;
        if (a.tile == 64080) a.ksplit = 1;  // (all of K inside the workgroup: wd_gemmq_kernel; wd_gemmq_applies() is checked later)
    }
    if (a.w_ngroups > 1) {
        // weight groups: the 64 x 320 weights-to-registers kernel only, a tile inside one run of rows, no K cut
        if (a.w_layout != 3 || a.tile != 64320 || a.ksplit > 1 || a.hw_out % (64 * a.w_ngroups) || a.w_group_stride <= 0 || (a.w_group_stride & 7))
            return WD_EINVAL;
        a.ksplit = 1;
    }
    if (a.stat_part) {
        // fused GroupNorm statistics need row panels that tile the samples and whole groups inside a column tile
        if (a.stat_cpg <= 0 || a.n % a.stat_cpg || a.act == WD_ACT_GEGLU) return WD_EINVAL;
        const int bn = (a.tile ? a.tile % 1000 : (a.n % 160 == 0 ? 160 : 64));
        const int bm = (a.tile ? a.tile / 1000 : 128);
        if (!((a.hw_out % bm == 0) || (bm % a.hw_out == 0 && bm / a.hw_out <= WD_STAT_MAXNS))) return WD_EINVAL;
        if ((bm != 128 && a.w_layout != 3) || bn % a.stat_cpg) return WD_EINVAL;
        // vector epilogue only: an odd pitch or a pointer off the 16-byte / 8-byte grid takes the scalar path, which keeps no column sums
        if (!wd_epilogue_vec_ok(a)) return WD_EINVAL;
        if (a.tile == 0) a.tile = bm * 1000 + bn;  // keep 128-row panels (no 64x64 fallback)
    }
    if (a.ksplit > 1 && (!a.ws || a.act == WD_ACT_GEGLU || a.w_layout == 1)) return WD_EINVAL;
    if (a.ln_gamma) {
        // row LayerNorm of the result: the tile must hold whole rows and the epilogue must run in the GEMM launch itself
        if (a.w_layout != 3 || (a.tile && a.tile != 64320) || a.n != 320 || a.ksplit > 1 || !a.ln_beta || !a.out_hi || (a.out_pl_ld & 3) ||
            ((reinterpret_cast<uintptr_t>(a.ln_gamma) | reinterpret_cast<uintptr_t>(a.ln_beta)) & 15) ||
            ((reinterpret_cast<uintptr_t>(a.out_hi) | reinterpret_cast<uintptr_t>(a.out_lo)) & 7) || a.act == WD_ACT_GEGLU)
            return WD_EINVAL;
        a.tile = 64320;
        a.ksplit = 1;
    }
    if (a.gn_gamma) {
        // GroupNorm of the result in the combine launch (wd_reduce_gn_tile): whole (sample, group) blocks per 64 x 40 tile
        if (!a.gn_beta || !a.stat_part || !a.out_hi || (!a.ws && a.tile != 64080) || a.hw_out != 64 || a.m % 64 || a.n % 160 || a.gn_cpg <= 0 ||
            40 % a.gn_cpg || a.stat_cpg <= 0 || a.gn_cpg % a.stat_cpg || a.act != WD_ACT_NONE || a.resid_rows || a.w_layout == 1)
            return WD_EINVAL;
        if (!wd_epilogue_vec_ok(a) ||
            ((reinterpret_cast<uintptr_t>(a.ws) | reinterpret_cast<uintptr_t>(a.gn_gamma) | reinterpret_cast<uintptr_t>(a.gn_beta)) & 15))
            return WD_EINVAL;
        a.tickets = nullptr;  // the norm lives in the combine launch
    }
    if (a.w_layout == 1) {
        a.ksplit = 1;
        a.tickets = nullptr;
    }
    return WD_OK;
}

// Step 2, operands and pitches: the sources add up to ktot, every plane is addressable, every pitch spans its row.
static int check_operands(const wd_gemm_args& a) {
    if (a.nsrc < 1 || a.nsrc > 2 || (a.npass != 1 && a.npass != 3)) return WD_EINVAL;
    if (a.m <= 0 || a.n <= 0 || a.hw_out <= 0 || !a.w_hi || (a.npass == 3 && !a.w_lo)) return WD_EINVAL;
    if (!a.out_f32 && !a.out_hi) return WD_EINVAL;
    long k = 0;
    for (int s = 0; s < a.nsrc; ++s) {
        const wd_src& q = a.src[s];
        if (s == 0 && a.a32) {
            // src[0] staged from the fp32 map with the consumer's GroupNorm: the weights-to-registers kernel, 64-row tiles inside one sample
            if (a.w_layout != 3 || a.npass != 3 || (a.tile && a.tile != 64320) || a.n % 320 || a.hw_out % 64 || !a.a32_part || !a.a32_gamma ||
                !a.a32_beta || a.a32_nchunk <= 0 || a.a32_pcpg <= 0 || a.a32_cpg <= 0 || a.a32_cpg % a.a32_pcpg || q.c % a.a32_cpg ||
                q.c > 1024 || a.a32_ld < q.c || (a.a32_ld & 3) || (reinterpret_cast<uintptr_t>(a.a32) & 15) || q.hw_src <= 0)
                return WD_EINVAL;
        } else if (!q.hi || (a.npass == 3 && !q.lo)) return WD_EINVAL;
        if (q.c <= 0 || q.c % BK || q.ld % 8 || q.ntaps < 1) return WD_EINVAL;
        if (!q.gather && q.ntaps != 1) return WD_EINVAL;
        if (q.gather && q.hw_src <= 0) return WD_EINVAL;
        k += (long)q.ntaps * q.c;
    }
    if (k != a.ktot) return WD_EINVAL;
    {   // the main kernel addresses every operand plane with 31-bit byte offsets (buffer_load ... lds)
        const long lim = 0x7FFFFFF0L;
        if ((long)a.n * a.ktot * 2 >= lim) return WD_EINVAL;
        for (int s = 0; s < a.nsrc; ++s) {
            const wd_src& q = a.src[s];
            const long rows = q.gather ? (long)((a.m + a.hw_out - 1) / a.hw_out) * q.hw_src : (long)a.m;
            if ((s == 0 && a.a32) ? rows * a.a32_ld * 4 >= lim : rows * q.ld * 2 >= lim) return WD_EINVAL;
        }
    }
    if (a.act == WD_ACT_GEGLU && (a.n % 64 || a.tile == 0)) return WD_EINVAL;  // the tile fixes the x|gate packing
    if (a.rowvec && a.rowvec_ld <= 0) return WD_EINVAL;
    if (a.resid && a.resid_ld <= 0) return WD_EINVAL;
    {   // a pitch spans at least the columns the launch touches in a row (a narrower one folds rows onto one another)
        const int nout = a.act == WD_ACT_GEGLU ? a.n / 2 : a.n;
        if ((a.out_f32 && a.out_ld < nout) || (a.out_hi && a.out_pl_ld < nout) || (a.resid && a.resid_ld < nout) ||
            (a.rowvec && a.rowvec_ld < nout))
            return WD_EINVAL;
        for (int s = 0; s < a.nsrc; ++s)
            if (!(s == 0 && a.a32) && a.src[s].ld < a.src[s].c) return WD_EINVAL;
    }
    return WD_OK;
}

// Step 3, w_layout 3 (fragment-major weights): K_GEMMQ on tile 64080, else K_GEMMW.  want_batch: wd_want_epi_batch of the caller's dbg;
// the resolved WD_EPI_BATCH_BIT is set here, for these two families only.
static int resolve_fragment_major(wd_gemm_args& a, const bool want_batch, WdResolved& r) {
    bool ok = a.src[0].ntaps <= 9 && src1_identity(a);
    for (int s = 0; s < a.nsrc; ++s) ok = ok && (a.src[s].c % 64 == 0);
    if (!ok) return WD_EINVAL;
    const wd_src& q0 = a.src[0];
    const bool same3 = src0_same3(a);
    // (slab_rows: the image width of a 3x3 / pad 1 / stride 1 source, as for w_layout 2; tile 64080 also takes the stride-2 table
    // of a Downsample - hw_src == 4 hw_out -, slab_rows then is the OUTPUT width)
    const bool down3 = a.tile == 64080 && q0.ntaps == 9 && q0.gather && a.slab_rows > 0 && q0.hw_src == 4 * a.hw_out;
    if (!same3 && !down3) a.slab_rows = 0;
    a.tickets = nullptr;
    if (a.tile == 64080) {
        if (!wd_gemmq_applies(a)) return WD_EINVAL;
        if (a.gn_gamma && (40 % a.gn_cpg || 80 % a.gn_cpg)) return WD_EINVAL;
        if (want_batch && wd_epilogue_batch_shape(a, 64, 80)) a.dbg |= WD_EPI_BATCH_BIT;
        r.a = a, r.kernel = K_GEMMQ;
        return WD_OK;
    }
    const int nk64 = a.ktot / 64;
    if (a.ksplit == 0) a.ksplit = a.ws ? wd_auto_ksplit(a.tile, a.m, a.n, nk64, a.ws_floats) : 1;
    if (a.ksplit > 1 && (nk64 < a.ksplit || (long)a.ksplit * a.m * a.n > a.ws_floats)) a.ksplit = 1;
    if (a.gn_gamma && a.ksplit <= 1) return WD_EINVAL;
    // the slab form of the 64 x 320 kernel: src[0] a 3x3 / pad 1 / stride 1 source whose 64-row tiles are whole image rows of
    // one sample, given as planes; an optional identity src[1]; no K cut.  Everything else takes the per-tap form.
    // WDIFF_GEMMW_SLAB (default WD_GEMMW_SLAB_DEFAULT) is the switch; dbg WD_GEMMW_SLAB_OFF / _ON override it per call.
    const bool want_slab = wd_want_gemmw_slab(a.dbg);
    const bool fits = a.tile == 64320 && a.npass == 3 && a.ksplit <= 1 && a.w_ngroups <= 1 && !a.a32 && !a.ln_gamma && same3 &&
                      64 % a.slab_rows == 0 && a.hw_out % 64 == 0 && a.m % a.hw_out == 0 && q0.c % 64 == 0 && src1_identity(a);
    if (want_slab && fits) a.dbg |= WD_GEMMW_SLAB_BIT;
    if (want_batch && a.tile == 64320 && wd_epilogue_batch_shape(a, 64, 320)) a.dbg |= WD_EPI_BATCH_BIT;
    r.a = a, r.kernel = K_GEMMW;
    return WD_OK;
}

// Step 4a of the staged kernels, w_layout 2 / 0: the operand layout of 2 is the ordinary one, so it is a hint that ends here.
static int staged_layout(wd_gemm_args& a, const bool conv3) {
    if (a.w_layout == 2) {
        const bool same3 = src0_same3(a);
        if (conv3) a.tile = 128160;
        a.w_layout = 0;
        // generic kernel: slab_rows > 0 now means "src[0] is a 3x3 / pad 1 / stride 1 window over images slab_rows wide" - the
        // source-row table of a panel is then computed, not looked up (saves the dependent global loads of the prologue)
        if (!same3 || !wd_gemm_switches().arith_tab) a.slab_rows = 0;
    } else if (a.w_layout == 0) {
        a.slab_rows = 0;
    } else {
        return WD_EINVAL;
    }
    return WD_OK;
}

// Step 4b, the grid: which kernels can run it at all, the tile, the K cut and whether wd_gemm4_kernel takes it.
static int staged_grid(wd_gemm_args& a, WdStaged& s) {
    s.v2ok = (a.ktot % BK2 == 0) && !getenv("WDIFF_GEMM_V1");
    for (int i = 0; i < a.nsrc; ++i) s.v2ok = s.v2ok && (a.src[i].c % BK2 == 0);
    s.v2ok = s.v2ok && a.src[0].ntaps <= 9 && src1_identity(a);
    s.nk64 = a.ktot / BK2;
    if (a.tile == 0)
        a.tile = wd_auto_tile(a.m, a.n, s.nk64, s.v2ok && a.ws && a.ksplit == 0 && a.act != WD_ACT_GEGLU, a.ws_floats);
    if (a.ksplit == 0) {
        // (half-filled chip - exactly 128 tiles, e.g. batch 32 -: a two-way cut pays on the long-K convolutions only)
        a.ksplit = (s.v2ok && a.ws && a.act != WD_ACT_GEGLU) ? wd_auto_ksplit(a.tile, a.m, a.n, s.nk64, a.ws_floats) : 1;
    }
    if (a.act == WD_ACT_GEGLU && a.n % (a.tile % 1000)) return WD_EINVAL;
    if (a.ksplit > 1 && (!s.v2ok || s.nk64 < a.ksplit || (long)a.ksplit * a.m * a.n > a.ws_floats)) a.ksplit = 1;
    s.use_v4 = false;
    if (a.tile == 128160) {
        // two co-resident 4-wave workgroups per CU for the layers without fused statistics (see wd_gemm4_kernel)
        // WDIFF_GEMM_V4: 0 never, 1 always (where legal), default 2 = when every CU gets at least two workgroups
        const int v4 = wd_gemm_switches().v4;
        const long wgs = (long)((a.m + 127) / 128) * ((a.n + 159) / 160) * a.ksplit;
        s.use_v4 = s.v2ok && !a.stat_part && (v4 == 1 || (v4 == 2 && wgs >= 512) || (a.dbg & WD_DBG_FORCE_V4));
    }
    return WD_OK;
}

// Step 4c, how the K slices are combined: tickets (in the GEMM launch) or the combine launch, which alone can norm the result.
static int staged_combine(wd_gemm_args& a, const WdStaged& s) {
    // in-launch split-K combine (tickets): v2 kernels only, vector epilogue (16-byte aligned everything), whole column tiles
    // Measured on the 4x16-level convolutions (M = 4096, 64 tiles x 4 slices of 80 KB): 46.0 us against 33.8 us for GEMM +
    // combine launch - the slabs of a tile are combined by ONE workgroup (64 busy CUs) behind an agent-scope release /
    // acquire, the combine launch spreads the same bytes over 512 workgroups - so the default is the second launch
    // (the guide's rule: in-launch pays up to a few tens of KB of slabs per tile).  dbg WD_DBG_FORCE_TICKETS forces it (parity tests).
    const bool fuse = wd_gemm_switches().fuse_combine || (a.dbg & WD_DBG_FORCE_TICKETS);
    const int bn = a.tile % 1000, bm = a.tile / 1000;
    const long ntile = (long)((a.m + bm - 1) / bm) * ((a.n + bn - 1) / bn);
    const bool aligned = (a.n & 3) == 0 && a.n % bn == 0 && wd_epilogue_vec_ok(a) && (reinterpret_cast<uintptr_t>(a.ws) & 15) == 0;
    if (!(fuse && a.tickets && a.ksplit > 1 && s.v2ok && !s.use_v4 && !s.conv3 && aligned && ntile <= a.ntickets)) a.tickets = nullptr;
    // the GroupNorm epilogue exists in the combine launch of the 128 x 160 kernels only: anything else is an error, not a skipped norm
    if (a.gn_gamma && !(a.ksplit > 1 && a.tile == 128160 && s.v2ok && !s.use_v4 && !s.conv3)) return WD_EINVAL;
    return WD_OK;
}

// ---- the experimental half: the only code that knows K_SLAB / K_CONV3 / K_V8 / K_PP
#ifdef WDIFF_EXPERIMENTAL
// w_layout 1, slab-order weights: v3 kernel only.  Contract: c % 32 == 0 (check_operands), src[1] identity, slab_rows set.
static int resolve_experimental_slab(wd_gemm_args& a, WdResolved& r) {
    if (a.src[0].ntaps > 9 || a.slab_rows <= 0) return WD_EINVAL;
    if (a.nsrc == 2 && (a.src[1].gather || a.src[1].ntaps != 1)) return WD_EINVAL;
    if (a.tile == 0) a.tile = (a.act == WD_ACT_GEGLU || a.n % 160) ? 128064 : 128160;
    if (a.act == WD_ACT_GEGLU && a.n % (a.tile % 1000)) return WD_EINVAL;
    if (a.slab_rows > 192) return WD_EINVAL;
    if (a.tile != 128064 && a.tile != 128128 && a.tile != 128160) return WD_EINVAL;
    r.a = a, r.kernel = K_SLAB;
    return WD_OK;
}

// w_layout 2, row-shared taps (wd_conv3_kernel): 3x3 / pad 1 / stride 1 over images of width slab_rows, optional identity source.
// A hint: shapes the kernel does not cover take the generic path.  WDIFF_CONV3 asks for it, dbg WD_DBG_FORCE_CONV3 too (parity tests).
static bool experimental_conv3(const wd_gemm_args& a) {
    if (a.w_layout != 2 || !(wd_gemm_switches().conv3 != 0 || (a.dbg & WD_DBG_FORCE_CONV3))) return false;
    return src0_same3(a) && a.src[0].c % 64 == 0 && a.act != WD_ACT_GEGLU && (a.tile == 0 || a.tile == 128160) &&
           (a.nsrc == 1 || (!a.src[1].gather && a.src[1].ntaps == 1 && a.src[1].c % 64 == 0));
}

// `fam` is the default family of a staged launch; the opt-in kernels that were asked for and fit take it over.
static WdKernel resolve_experimental(wd_gemm_args& a, const WdStaged& s, const int ks, const WdKernel fam) {
    if (s.conv3 && s.v2ok) return K_CONV3;
    if (a.tile == 128160 && fam != K_V4) {
        // ring kernel with dedicated loader waves (wd_gemm8_kernel): within +-5 % of the default kernel on every shape; no
        // fused GroupNorm statistics (its 768-thread epilogue would need a larger statistics scratch).  WDIFF_GEMM_V8=1 takes it wherever legal, dbg WD_DBG_FORCE_V8 forces it (parity tests).
        bool v8ok = a.ktot % 32 == 0 && a.src[0].ntaps <= 9 && !a.stat_part && !a.gn_gamma && a.act != WD_ACT_GEGLU && src1_identity(a);
        for (int s8 = 0; s8 < a.nsrc; ++s8) v8ok = v8ok && (a.src[s8].c % 32 == 0);
        if (v8ok && (wd_gemm_switches().v8 == 1 || (a.dbg & WD_DBG_FORCE_V8))) {
            if (a.ksplit > 1 && (a.ktot / 32 < a.ksplit || (long)a.ksplit * a.m * a.n > a.ws_floats)) a.ksplit = 1;
            a.tickets = nullptr;
            return K_V8;
        }
    }
    if (fam == K_V2 && ks == 2 && wd_gemm_switches().pp) return K_PP;  // (measured: no gain)
    return fam;
}
#else
static int resolve_experimental_slab(wd_gemm_args&, WdResolved&) { return WD_EINVAL; }  // (the slab kernel is an experimental build option)
static bool experimental_conv3(const wd_gemm_args&) { return false; }
static WdKernel resolve_experimental(wd_gemm_args&, const WdStaged&, const int, const WdKernel fam) { return fam; }
#endif

// Step 4, the kernels that stage both operands through LDS: K_V4 / K_M16 / K_V2 / K_V1.
static int resolve_staged(wd_gemm_args& a, WdResolved& r) {
    WdStaged s;
    s.conv3 = experimental_conv3(a);
    if (staged_layout(a, s.conv3) != WD_OK || staged_grid(a, s) != WD_OK || staged_combine(a, s) != WD_OK) return WD_EINVAL;
    if (a.tile != 128064 && a.tile != 128160 && a.tile != 128128 && a.tile != 64064) return WD_EINVAL;
    const WdGemmSwitches& sw = wd_gemm_switches();
    const bool m16 = a.tile == 128160 && s.v2ok && r.ks == 2 && sw.m16;
    const WdKernel fam = resolve_experimental(a, s, r.ks, s.use_v4 ? K_V4 : m16 ? K_M16 : s.v2ok ? K_V2 : K_V1);
    // K_M16: the second K-half group runs one stage late (see the kernel); the extra drain phase only pays on long K loops
    if (fam == K_M16 && sw.stagger && s.nk64 / a.ksplit >= sw.stagger_min) a.dbg |= WD_DBG_STAGGER;
    if (fam == K_V1) {
        a.ksplit = 1;
        a.tickets = nullptr;
    }
    r.a = a, r.kernel = fam;
    return WD_OK;
}

// Every check and every decision of wd_gemm, host only (no HIP call): WD_OK and `r` filled, or WD_EINVAL.
static int wd_gemm_resolve(const wd_gemm_args& in, WdResolved& r) {
    wd_gemm_args a = in;
    const bool want_batch = wd_want_epi_batch(a.dbg);
    r.ks = wd_gemm_switches().ks == 1 ? 1 : 2;
    if (resolve_options(a) != WD_OK || check_operands(a) != WD_OK) return WD_EINVAL;
    if (a.w_layout == 3) return resolve_fragment_major(a, want_batch, r);
    if (a.w_layout == 1) return resolve_experimental_slab(a, r);
    return resolve_staged(a, r);
}

extern "C" int wd_gemm_experimental(void) {  // 1: built with -DWDIFF_EXPERIMENTAL (slab / row-shared-taps / ring kernels present)
#ifdef WDIFF_EXPERIMENTAL
    return 1;
#else
    return 0;
#endif
}

extern "C" int wd_gemm_args_bytes(void) { return (int)sizeof(wd_gemm_args); }  // (callers that mirror the struct check their layout)

extern "C" int wd_gemm_auto_ksplit(int m, int n, int ktot, int64_t ws_floats) {
    if (m <= 0 || n <= 0 || ktot <= 0 || ktot % BK2 || ws_floats <= 0) return 1;
    const int nk64 = ktot / BK2;
    return wd_auto_ksplit(wd_auto_tile(m, n, nk64, true, (long)ws_floats), m, n, nk64, (long)ws_floats);
}

extern "C" int wd_gemm_check(const wd_gemm_args* in, wd_gemm_args* out) {
    if (!in) return WD_EINVAL;
    WdResolved r;
    const int rc = wd_gemm_resolve(*in, r);
    if (rc == WD_OK && out) *out = r.a;
    return rc;
}

extern "C" int wd_epilogue_batch_applies(const wd_gemm_args* a, int bm, int bn) {
    return a && bm == 64 && bn > 0 && bn % 4 == 0 && wd_epilogue_batch_ok(*a, bm, bn) ? 1 : 0;
}

extern "C" const char* wd_gemm_check_kernel(const wd_gemm_args* in) {
    if (!in) return nullptr;
    WdResolved r;
    if (wd_gemm_resolve(*in, r) != WD_OK) return nullptr;
    switch (r.kernel) {
        case K_GEMMQ: return "K_GEMMQ";
        case K_GEMMW: return "K_GEMMW";
        case K_V4: return "K_V4";
        case K_M16: return "K_M16";
        case K_V2: return "K_V2";
        case K_V1: return "K_V1";
        case K_SLAB: return "K_SLAB";
        case K_CONV3: return "K_CONV3";
        case K_V8: return "K_V8";
        case K_PP: return "K_PP";
    }
    return nullptr;
}

extern "C" int wd_gemm(const wd_gemm_args* pa, void* stream) {
    if (!pa) return WD_EINVAL;
    WdResolved r;
    const int rc = wd_gemm_resolve(*pa, r);
    if (rc != WD_OK) return rc;
    const wd_gemm_args& a = r.a;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (r.kernel) {
        case K_GEMMQ: return wd_gemmq_launch(a, st);
        case K_GEMMW: return wd_gemmw_launch(a, st);
        case K_V4: return wd_gemm4_launch(a, st);
        case K_M16: return wd_gemm2_launch(a, st, 2, true, false);
        case K_V2: return wd_gemm2_launch(a, st, r.ks, false, false);
        case K_V1: return wd_gemm1_launch(a, st);
#ifdef WDIFF_EXPERIMENTAL
        case K_SLAB: return wd_gemm3_launch(a, st, r.ks);
        case K_CONV3: return wd_conv3_launch(a, st);
        case K_V8: return wd_gemm8_launch(a, st);
        case K_PP: return wd_gemm2_launch(a, st, 2, false, true);
#endif
        default: return WD_EINVAL;
    }
}
