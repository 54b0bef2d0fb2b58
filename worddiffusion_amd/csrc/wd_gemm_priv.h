// Internal links between the translation units of the tap-gather GEMM (not part of the C ABI).
#pragma once
#include "wd_common.h"

// wd_gemmw.hip: the 64 x 320 "weights straight to registers" kernel (wd_gemm_args.w_layout == 3).  `a` has been validated and
// its ksplit resolved by wd_gemm().
int wd_gemmw_launch(const wd_gemm_args& a, hipStream_t st);
// wd_gemm_args.dbg (the names: include/wdiff_hip.h), the slab form of that kernel (the A operand of a 3x3 / pad 1 / stride 1 source from an LDS slab, see the kernel).
// A caller's WD_GEMMW_SLAB_OFF / _ON overrides WDIFF_GEMMW_SLAB for this call (the engine's own switch, the parity tests); in
// the RESOLVED args WD_GEMMW_SLAB_BIT says that the launch takes the slab form - wd_gemm_resolve alone decides that.
constexpr bool WD_GEMMW_SLAB_DEFAULT = true;
// wd_gemm_args.dbg / wd_ff_args.dbg, the batched form of the 64-row tile epilogue (wd_epilogue_rows, wd_gemm_epi.h: every row load of a
// thread, one wait, then the rows' arithmetic and stores with no load between them).  A caller's WD_EPI_BATCH_OFF / _ON overrides
// WDIFF_EPI_BATCH for this call; in the RESOLVED args WD_EPI_BATCH_BIT says that the launch's 16-byte epilogue path is the batched form -
// wd_gemm_resolve / wd_ff_fused alone decide that, by wd_epilogue_batch_shape (wd_gemm_epi.h); the kernels ask wd_epilogue_batch_ok.
constexpr bool WD_EPI_BATCH_DEFAULT = true;
// wd_gemm.hip: the split-K combine launch for slabs of a launch with bm-row tiles (statistics layout follows bm).
int wd_gemm_launch_reduce(const wd_gemm_args& a, hipStream_t st, int bm);
// wd_gemmq.hip: 64 x 80 tiles, all of K inside the workgroup (wd_gemm_args.tile == 64080: the 3x3 layers over 64-position samples).
bool wd_gemmq_applies(const wd_gemm_args& a);
int wd_gemmq_launch(const wd_gemm_args& a, hipStream_t st);
