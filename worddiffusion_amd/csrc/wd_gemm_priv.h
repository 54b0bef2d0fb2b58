// Internal links between the translation units of the tap-gather GEMM (not part of the C ABI).  wd_gemm_plan.hip validates and
// resolves a launch (host only) and calls exactly one of the family launchers below; every launcher takes args that
// wd_gemm_resolve has validated and resolved (tile, ksplit, tickets, slab_rows, dbg) and picks its own template instantiation.
#pragma once
#include "wd_common.h"

// K depth of a stage: the v1 / v4 kernels (BK; every source's channel count is a multiple of it) and the v2 kernel (BK2).
constexpr int BK = 32;
constexpr int BK2 = 64;

// wd_gemm.hip: wd_gemm_kernel (K_V1), tiles 128064 / 128160 / 128128 / 64064.
int wd_gemm1_launch(const wd_gemm_args& a, hipStream_t st);
// wd_gemm.hip: wd_gemm2_kernel with `ks` K-halves per workgroup (K_V2), its 16x16x32 form on tile 128160 (m16: K_M16) or its
// ping-pong form (pp: K_PP, experimental build only); the same four tiles.
int wd_gemm2_launch(const wd_gemm_args& a, hipStream_t st, int ks, bool m16, bool pp);
// wd_gemm.hip, a library built with WDIFF_EXPERIMENTAL=1 only: wd_gemm3_kernel (K_SLAB), tiles 128064 / 128128 / 128160.
int wd_gemm3_launch(const wd_gemm_args& a, hipStream_t st, int ks);
// wd_gemm4.hip: wd_gemm4_kernel (K_V4), tile 128160.
int wd_gemm4_launch(const wd_gemm_args& a, hipStream_t st);
// wd_gemmw.hip: the 64 x 320 "weights straight to registers" kernel (K_GEMMW; wd_gemm_args.w_layout == 3).
int wd_gemmw_launch(const wd_gemm_args& a, hipStream_t st);
// wd_gemmq.hip: 64 x 80 tiles, all of K inside the workgroup (K_GEMMQ; wd_gemm_args.tile == 64080: the 3x3 layers over 64-position samples).
bool wd_gemmq_applies(const wd_gemm_args& a);
int wd_gemmq_launch(const wd_gemm_args& a, hipStream_t st);
// wd_gemm_exp.hip (a library built with WDIFF_EXPERIMENTAL=1 only): wd_conv3_kernel (K_CONV3), wd_gemm8_kernel (K_V8).
int wd_conv3_launch(const wd_gemm_args& a, hipStream_t st);
int wd_gemm8_launch(const wd_gemm_args& a, hipStream_t st);
// wd_gemm_reduce.hip: the split-K combine launch for the slabs of a launch with bm x bn tiles (the statistics layout follows bm; bn
// is the combine's own column tile where the statistics groups fit neither 40 nor 32 columns).
int wd_gemm_launch_reduce(const wd_gemm_args& a, hipStream_t st, int bm, int bn);

// wd_gemm_args.dbg (the names: include/wdiff_hip.h), the slab form of the 64 x 320 kernel (the A operand of a 3x3 / pad 1 / stride 1
// source from an LDS slab, see the kernel).  A caller's WD_GEMMW_SLAB_OFF / _ON overrides WDIFF_GEMMW_SLAB for this call (the
// engine's own switch, the parity tests); in the RESOLVED args WD_GEMMW_SLAB_BIT says that the launch takes the slab form -
// wd_gemm_resolve alone decides that.
constexpr bool WD_GEMMW_SLAB_DEFAULT = true;
// wd_gemm_args.dbg / wd_ff_args.dbg, the batched form of the 64-row tile epilogue (wd_epilogue_rows, wd_gemm_epi.h: every row load of a
// thread, one wait, then the rows' arithmetic and stores with no load between them).  A caller's WD_EPI_BATCH_OFF / _ON overrides
// WDIFF_EPI_BATCH for this call; in the RESOLVED args WD_EPI_BATCH_BIT says that the launch's 16-byte epilogue path is the batched form -
// wd_gemm_resolve / wd_ff_fused alone decide that, by wd_epilogue_batch_shape (wd_gemm_epi.h); the kernels ask wd_epilogue_batch_ok.
constexpr bool WD_EPI_BATCH_DEFAULT = true;
// wd_gemm_plan.hip, the one reading of each override rule: what the caller's _OFF / _ON bits in `dbg` and the environment switch
// ask for; both request bits are cleared from `dbg` (the caller sets the resolved _BIT where the form is legal).
bool wd_want_epi_batch(int32_t& dbg);
bool wd_want_gemmw_slab(int32_t& dbg);
