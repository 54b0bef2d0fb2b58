/*
 * wdiff_hip.h - C ABI of libwdiff_hip.so: the MI355X (gfx950) kernels behind the WordDiffusion UNet
 * denoising hot path.
 *
 * The reference (aniketntnu/WordDiffusion) is pure Python on stock PyTorch and has no FFI of its own
 * (SURVEY.md fact 0.1, section 8b); the boundary a maintainer binds is the Python class surface
 * (worddiffusion_amd.UNetModel / UNetModelPhosc / Diffusion / EMA).  This C ABI is what that Python
 * surface calls (ctypes).  Every entry point:
 *   - takes raw DEVICE pointers, sizes and a hipStream_t (passed as void*); no torch types;
 *   - allocates nothing and takes no ownership; workspaces are passed in;
 *   - returns 0 on success, a negative WD_E* code on a bad argument or a failed launch;
 *   - is asynchronous on the given stream and safe to capture into a hipGraph.
 *
 * Data layout: feature maps are token-major ("NHWC"): row m = b*HW + y*W + x, C contiguous floats.
 * GEMM operands are "split-bf16 planes": two bf16 matrices hi = bf16(x), lo = bf16(x - hi), consumed
 * by v_mfma_f32_32x32x16_bf16 as hi*hi + hi*lo + lo*hi (npass = 3, ~2^-17 relative operand error,
 * fp32 accumulate) or hi*hi only (npass = 1, plain bf16).
 *
 * For each function the reference code it replaces is cited as file:line of /root/reference.
 */
#ifndef WDIFF_HIP_H
#define WDIFF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WD_OK 0
#define WD_EINVAL (-1)  /* bad argument (null pointer, unsupported size) */
#define WD_ELAUNCH (-2) /* hip launch / runtime error */
#define WD_ESTATE (-3)  /* call order error (e.g. graph end without begin) */

#define WD_ACT_NONE 0
#define WD_ACT_SILU 1
#define WD_ACT_GEGLU 2 /* out[:, j] = x_j * gelu_erf(gate_j); weight/bias rows packed per BN-tile as [BN/2 x | BN/2 gates]; tile must be set */

typedef uint16_t wd_bf16;

#define WD_MAX_KSPLIT 64 /* largest wd_gemm_args.ksplit */

/* The bits of wd_gemm_args.dbg / wd_ff_args.dbg / wd_dw_args.dbg a caller may set or a check returns (0 in production; the bits
 * below 0x100 are timing ablations of the experimental slab-order kernel).  FORCE_*: take that kernel form wherever it is legal,
 * whatever the grid size or the environment says (parity tests).  *_OFF / *_ON: override the named environment switch for this
 * call; both are cleared in the args a check returns, where *_BIT says which form the launch takes. */
#define WD_DBG_STAMPS 0x100           /* cycle stamps of workgroup 0 into ws / wd_dw_args.stamps (a library built with WDIFF_STAMPS=1) */
#define WD_DBG_STAGGER 0x200          /* resolved only: the second K-half wave group multiplies one stage late */
#define WD_DBG_FORCE_V4 0x400         /* the two-workgroups-per-CU kernel (wd_gemm4_kernel) */
#define WD_DBG_FORCE_CONV3 0x1000     /* the row-shared-taps kernel for w_layout 2 (wd_conv3_kernel, experimental build) */
#define WD_DBG_FORCE_TICKETS 0x2000   /* the in-launch split-K combine (tickets) */
#define WD_DBG_GEMMW_INSTEP 0x4000    /* timing experiment: the K-half groups of the per-tap 64 x 320 kernel run in step, none a stage late */
#define WD_GEMMW_SLAB_OFF 0x8000      /* WDIFF_GEMMW_SLAB: the 64 x 320 weights-to-registers kernel keeps the per-tap A path ... */
#define WD_GEMMW_SLAB_ON 0x10000      /* ... takes the slab form (3x3 / pad 1 / stride 1 source rows from an LDS slab) where it is legal */
#define WD_GEMMW_SLAB_BIT 0x10000     /* resolved: the launch takes the slab form */
#define WD_EPI_BATCH_OFF 0x20000      /* WDIFF_EPI_BATCH: the 64-row tiles (64320, 64080, wd_ff_fused) keep the row loop of their epilogue ... */
#define WD_EPI_BATCH_ON 0x40000       /* ... take its batched form - a thread's row loads in one round trip, then its stores - where it is legal */
#define WD_EPI_BATCH_BIT 0x40000      /* resolved: the 16-byte path of the launch's epilogue is the batched form */
#define WD_DBG_FORCE_V8 0x80000       /* the ring-of-four kernel with dedicated loader waves (wd_gemm8_kernel) */

/* One A-operand source of the tap-gather GEMM.  K contribution = ntaps * c.
 * Row m of the output (sample b = m / hw_out, position p = m % hw_out) reads, for tap t,
 * source row  b*hw_src + gather[t*hw_out + p]  (all-zero row when that entry is < 0);
 * gather == NULL means the identity (row m, ntaps must be 1). */
typedef struct wd_src {
    const wd_bf16* hi;
    const wd_bf16* lo; /* may be NULL when npass == 1 */
    const int32_t* gather;
    int32_t ld;     /* row pitch of hi/lo in elements, multiple of 8 */
    int32_t c;      /* channels read per tap, multiple of 32 */
    int32_t ntaps;  /* 1 (1x1 / linear) or 9 (3x3) */
    int32_t hw_src; /* rows per sample in the source */
} wd_src;

/* out[m, n] = act( sum_k A[m, k] * W[n, k] + bias[n] + rowvec[m / hw_out, n] + resid[rr(m), n] )
 * with A = [src0 taps | src1 taps] along k.
 * Replaces nn.Conv2d 3x3 / stride-2 / nearest-x2+3x3 / 1x1 and nn.Linear on the path:
 * unet.py:595,621,632 (ResBlock convs + skip), :540 (Downsample), :488-499 (Upsample), :364,375 (proj_in/out),
 * :175-183 (attention projections), :125,145 (GEGLU feed-forward), :1201-1205 (time MLP), :611 (emb_layers).
 * Every operand has a row pitch of its own (wd_src.ld, rowvec_ld, resid_ld, out_ld, out_pl_ld, a32_ld), so each may be a column
 * window of a wider buffer.  A pitch narrower than the columns the launch touches in a row is WD_EINVAL, not a fold of rows onto
 * one another: with n_out = n (n / 2 under WD_ACT_GEGLU), out_ld >= n_out when out_f32 is set, out_pl_ld >= n_out when out_hi is
 * set, resid_ld >= n_out when resid is set, rowvec_ld >= n_out when rowvec is set, and ld >= c for every planes source.  The
 * launch reads and writes nothing outside those windows (rows [0, m), the stated columns): pitch padding and neighbouring rows
 * are never stored to and never reach a stored value or a statistic. */
typedef struct wd_gemm_args {
    wd_src src[2];
    int32_t nsrc;
    int32_t npass; /* 3 = split-bf16 (fp32-class), 1 = bf16 */
    const wd_bf16* w_hi; /* [n][ktot], k contiguous */
    const wd_bf16* w_lo;
    int32_t m, n, ktot;
    int32_t hw_out;       /* rows per sample of the output (1 for per-sample vectors) */
    const float* bias;    /* [n] or NULL */
    const float* rowvec;  /* [m / hw_out][rowvec_ld] or NULL: additive timestep/writer (FiLM) term, unet.py:660-669 */
    int32_t rowvec_ld;
    const float* resid;   /* [rows][resid_ld] or NULL: residual / skip input */
    int32_t resid_ld;
    const int64_t* resid_rows; /* NULL: row m; else row resid_rows[m] (label_emb gather, unet.py:1581) */
    int32_t act;
    float* out_f32;       /* [m][out_ld] or NULL */
    int32_t out_ld;
    wd_bf16* out_hi;      /* split-bf16 planes of the result for the next GEMM, or NULL */
    wd_bf16* out_lo;
    int32_t out_pl_ld;
    int32_t tile;         /* 0 = auto; else BM*1000+BN of a compiled tile (128064, 128128, 128160, 64064; 64320 / 64080 with w_layout 3) */
    int32_t w_layout;     /* 0: w = [n][ktot].  1: "slab order" [stage][n][32], stage = (32-channel chunk, tap) of src0
                           * (chunk-major, tap-minor) followed by the 32-channel chunks of src1: selects the kernel that
                           * keeps the source slab of a BM-row panel resident in LDS (3x3 taps re-read LDS, not L2)
                           * 3: fragment-major weights (wd_gemm_pack_w), loaded straight into registers; tile 64320 or 128160; or tile
                           *    64080 - all of K inside the workgroup, never a K cut: src[0] a 3x3 / pad 1 / stride 1 source over
                           *    64-position samples of width slab_rows (16 or 32; hw_out == hw_src == 64), the stride-2 table of a
                           *    Downsample onto such samples (slab_rows = 16 = the OUTPUT width, hw_src == 256) or an identity source, src[1]
                           *    (optional) an identity source, planes only, npass 3, n % 80 == 0, no activation / row gather / a32 / ln;
                           *    gn_* is then served by the launch itself (n % 160 == 0, 40 % gn_cpg == 0), ws is not needed.
                           *    Statistics (stat_part) are kept per row panel of the tile: nchunk = max(1, hw_out / 64) for the
                           *    64-row tile */
    int32_t slab_rows;    /* w_layout 1: max over 128-row panels of (max - min + 1) gathered source row; <= 192
                           * w_layout 2 or 3: w as for 0 (2) / fragment-major (3), src[0] is a 3x3 / pad 1 / stride 1 convolution (9 taps, its usual
                           * gather table) over images of width slab_rows, src[1] (optional) an identity source: selects the
                           * kernel that loads the A tile of a kernel row once for its three taps when WDIFF_CONV3=1; in every case
                           * it lets the kernel compute the source rows of a panel instead of reading the gather table */
    int32_t ksplit;       /* 1: off.  >1 (at most WD_MAX_KSPLIT): the K range is cut into ksplit slices run by separate workgroups
                           * (fills the chip when m*n is small); partial sums go to ws and are combined in fixed order.  0: automatic
                           * (splits only when ws is given and the tile grid would leave most CUs idle) */
    float* ws;            /* split-K workspace (ksplit * m * n floats are used) or NULL */
    int64_t ws_floats;    /* capacity of ws in floats */
    double* stat_part;    /* NULL, or [m / hw_out][nchunk][n / stat_cpg][2] (sum, sum of squares) of the finished output per
                           * (sample, 128-row chunk, channel group): GroupNorm statistics for the consumer (wd_gn_apply),
                           * nchunk = max(1, hw_out / 128).  Needs 128-row tiles, hw_out | 128 or 128 | hw_out, whole
                           * groups per column tile, the vector epilogue (out_ld, rowvec_ld, resid_ld, out_pl_ld multiples of 4;
                           * bias, rowvec, resid, out_f32 16-byte and out_hi / out_lo 8-byte aligned); not with GEGLU.
                           * Accuracy (every producer of such partials: this epilogue, the combine launch, tile 64080, wd_ff_fused,
                           * wd_conv3x3_in): var = sumsq / n - mean^2 formed from them in double is within ~1e-7 of the variance
                           * of the fp32 values for any mean / std of a group (measured <= 1e-7 up to 256) - no fp32 stage sums
                           * the values or their squares unshifted (csrc/wd_gemm_epi.h, WdStatAcc) */
    int32_t stat_cpg;     /* channels per statistics group */
    int32_t dbg;          /* 0 in production, else WD_DBG_* / WD_GEMMW_SLAB_* / WD_EPI_BATCH_* above.  WD_GEMMW_SLAB_OFF / _ON and
                             WD_EPI_BATCH_OFF / _ON apply to the tiles of w_layout 3 (the slab form: 64320; the batched epilogue:
                             64320 and 64080); in the args wd_gemm_check returns they are cleared and WD_DBG_STAGGER,
                             WD_GEMMW_SLAB_BIT, WD_EPI_BATCH_BIT say what the launch does (a launch whose pitches or addresses
                             keep it off the 16-byte epilogue path runs the element loop either way - wd_epilogue_batch_applies
                             says both) */
    int32_t* tickets;     /* NULL: split-K partials are combined by a second launch.  Else ntickets ints, ALL ZERO before the
                           * call and left all zero by it, not shared with a launch that may run concurrently: one arrival
                           * counter per output tile - the workgroup that finishes a tile's last K slice sums the slices from
                           * ws in ascending slice order and runs the epilogue itself (same bits as the second launch, one
                           * launch less).  Used when the shapes allow it (16-byte aligned operands, n a multiple of the tile) */
    int32_t ntickets;
    /* GroupNorm of the RESULT in the combine launch (nn.GroupNorm of the consumer, unet.py:427-431 / :161-162, + SiLU): when
     * gn_gamma != NULL the planes out_hi / out_lo receive SiLU?((result - mean) * rstd * gn_gamma[col] + gn_beta[col]) with the
     * statistics of (sample, group of gn_cpg channels) instead of the result itself; out_f32 and stat_part are written as
     * usual.  Only where one combine tile holds whole (sample, group) blocks (hw_out == 64, 40 % gn_cpg == 0, stat_part given, no
     * activation) and the launch cuts K or holds all of K (tile 64080); wd_gemm_check says whether a given launch does - anything
     * else returns an error rather than skip the norm. */
    const float* gn_gamma;
    const float* gn_beta;
    float gn_eps;
    int32_t gn_silu;
    int32_t gn_cpg;
    /* GroupNorm of the INPUT while it is staged (w_layout 3, tile 64320, npass 3 only): a32 != NULL makes src[0] the fp32 map
     * a32 [rows][a32_ld] itself (src[0].hi / lo are ignored; c, ntaps, gather, hw_src as usual) and the rows enter the product as
     * SiLU?((x - mean) * rstd * a32_gamma[ch] + a32_beta[ch]) (nn.GroupNorm of the consumer, unet.py:427-431 / :161-162), with
     * the statistics of (sample, group of a32_cpg channels) summed from a32_part [batch][a32_nchunk][c / a32_pcpg][2]
     * (wd_gn_stats' / stat_part's layout; a32_pcpg divides a32_cpg).  Zero padding stays zero.  Needs hw_out % 64 == 0 and
     * hw_src == hw_out's sample grid (a row tile must lie inside one sample), c <= 1024, a32_ld % 4 == 0. */
    const float* a32;
    int32_t a32_ld;
    const double* a32_part;
    int32_t a32_nchunk;
    int32_t a32_pcpg;
    int32_t a32_cpg;
    const float* a32_gamma;
    const float* a32_beta;
    float a32_eps;
    int32_t a32_silu;
    /* LayerNorm of the RESULT's rows in the epilogue (w_layout 3, tile 64320, n == 320, no K cut): ln_gamma != NULL makes
     * out_hi / out_lo receive LayerNorm(result row) * ln_gamma + ln_beta (nn.LayerNorm of the consuming transformer block,
     * unetPhosc.py:241-246 norm1 / norm2 / norm3) instead of the result's own planes; out_f32 is still the result. */
    const float* ln_gamma;
    const float* ln_beta;
    float ln_eps;
    /* Weight groups (w_layout 3, tile 64320, no K cut): w_ngroups > 1 cuts the hw_out rows of every sample into w_ngroups equal
     * runs (each a multiple of 64 rows); run g multiplies with the fragment-major image at w_hi / w_lo + g * w_group_stride
     * elements.  The nearest x2 upsample + 3x3 convolution (Upsample.forward, unet.py:488-499) runs this way as its four output
     * phases (row parity, column parity): a phase reads a 2 x 2 neighbourhood of the SOURCE map with the kernel taps that fall
     * on the same source pixel summed - 4 taps instead of 9; the rows of a sample come out phase-major (wd_gn_apply2's perm_a
     * reads them back in raster order). */
    int32_t w_ngroups;
    int64_t w_group_stride;
} wd_gemm_args;

int wd_gemm(const wd_gemm_args* args, void* stream);

/* What wd_gemm would do with `args`, without launching anything (host only, no HIP call): WD_OK when wd_gemm accepts them, else
 * WD_EINVAL.  On WD_OK and out != NULL, *out receives the args as the kernel sees them (tile, ksplit, tickets, slab_rows resolved).
 * Callers ask this rather than restate the rules above. */
int wd_gemm_check(const wd_gemm_args* args, wd_gemm_args* out);
/* The launch family wd_gemm would run `args` on, by the name csrc/wd_gemm_plan.hip gives it ("K_V1", "K_V2", "K_M16", "K_V4", "K_GEMMW",
 * "K_GEMMQ", ...; a static string), NULL where wd_gemm_check refuses them.  Host only: lets a test pin the kernel a case is about. */
const char* wd_gemm_check_kernel(const wd_gemm_args* args);
/* 1 when a launch of bm x bn tiles over `args` (as wd_gemm_check returns them) runs the batched epilogue: the 16-byte path
 * (pitches % 4, fp32 operands 16-byte and planes 8-byte aligned), no K cut, activation none or SiLU, no ln_gamma / gn_gamma /
 * a32 / resid_rows, m % bm == 0, n % bn == 0, hw_out % bm == 0, pitches below 2^22 elements.  Host only; the rule the kernels ask. */
int wd_epilogue_batch_applies(const wd_gemm_args* args, int bm, int bn);

/* wd_gemm_args.w_layout == 3: the weights of a GEMM with n % 320 == 0, ktot % 64 == 0 in FRAGMENT-MAJOR order - the 16 bytes
 * lane l of a v_mfma_f32_16x16x32_bf16 B fragment holds, W[16 ct + (l & 15)][32 ks + 8 (l >> 4) .. + 8], at byte
 * ((ks * n/16 + ct) * 64 + l) * 16 of the plane - so a wave loads a fragment as one contiguous kilobyte straight into
 * registers and the weights never pass through LDS (64 x 320 tiles, csrc/wd_gemmw.hip; same nn.Conv2d / nn.Linear layers as
 * wd_gemm: unet.py:595,621,632,540,488,364,375,145).  wd_gemm_pack_w converts [n][ktot] planes (lo / out_lo may be NULL). */
int wd_gemm_pack_w(const wd_bf16* hi, const wd_bf16* lo, int n, int ktot, wd_bf16* out_hi, wd_bf16* out_lo, void* stream);

/* The GEGLU feed-forward of a transformer block with its residual in one launch per 64-token panel (csrc/wd_ff.hip):
 *     out = resid + GEGLU(x W1^T + b1) W2^T + b2        FeedForward / GEGLU unet.py:122-149, residual unet.py:343-344
 * x: split-bf16 planes of LayerNorm(norm3) of the tokens, [m][x_ld]; c = 320 channels, inner hidden units (a multiple of 128).
 * w1: wd_gemm_pack_w image of the [2 * inner][c] projection with its rows reordered in blocks of 16 x-rows followed by their 16
 * gate rows (unet.py:128 chunk(2): x = rows [0, inner), gate = rows [inner, 2 inner)); b1 in the same order.  w2: wd_gemm_pack_w
 * image of the [c][inner] output projection.  The hidden activations never leave the chip.  The result goes through the GEMM
 * epilogue: fp32 out_f32 and / or split-bf16 planes out_hi / out_lo, optional GroupNorm statistics (stat_part per 64-row panel:
 * nchunk = max(1, hw_out / 64), as wd_gemm with 64-row tiles).
 * w3 != NULL: the 1x1 proj_out of the SpatialTransformer and its residual ride in the same launch (unet.py:406-412),
 *     out = resid3 + (resid + GEGLU(...) W2^T + b2) W3^T + b3
 * with w3 the wd_gemm_pack_w image of the [c][c] projection; the feed-forward result itself is then not stored.
 * x_in != NULL: the whole SpatialTransformer of the base model (one transformer block, c == inner == 320) in the same launch; the
 *     panel's tokens come from x_in (fp32 [m][x_in_ld], the block input, also resid3) instead of x_hi / x_lo (then unused):
 *         tok  = GroupNorm(x_in) Wpi^T + pi_b               norm (eps gn_eps, no SiLU) + proj_in, unet.py:398-402
 *         tok1 = tok  + attn1(norm2(tok))                   folded cross-attention a (wd_xattn_fold planes mq_a / mot_a, bias xb_a)
 *         tok2 = tok1 + attn2(norm2(tok1))                  folded cross-attention b, unet.py:337-345
 *         x    = norm3(tok2) -> the feed-forward above, resid = tok2 (written to the fp32 scratch tok2 [m][320]; resid ignored)
 *     GroupNorm statistics as wd_gemm_args.a32*: gn_part [batch][gn_nchunk][c / gn_pcpg][2], groups of gn_cpg channels, samples of
 *     hw rows (hw % 64 == 0, m % hw == 0).  pi: wd_gemm_pack_w image of the [320][320] proj_in.  mq_* / mot_*: the per-sample
 *     fragment-major planes of wd_xattn_fold; wd_xattn_supported(320, heads, L).  npass 3 and w3 only.
 * w32_hi != NULL (with w3, npass 3): the folded tail.  No non-linearity separates the two last products, so
 *     out = resid3 + GEGLU(...) W32^T + resid W3^T + b32,   W32 = W3 W2 ([c][inner]),  b32 = W3 b2 + b3   (wd_linear_fold)
 * with w32 the wd_gemm_pack_w image of W32: resid W3^T is formed before the hidden chunks, the chunks add their part on top, and
 * the feed-forward result is never materialised (w2 / b2 / b3 are not read).  With x_in, tok2 may be NULL and is then not written.
 * Without x_in, resid is required. */
typedef struct wd_ff_args {
    const wd_bf16* x_hi;
    const wd_bf16* x_lo;
    int32_t x_ld;
    int32_t m, c, inner;
    const wd_bf16* w1_hi;
    const wd_bf16* w1_lo;
    const float* b1;
    const wd_bf16* w2_hi;
    const wd_bf16* w2_lo;
    const float* b2;
    const float* resid; /* [m][resid_ld] or NULL */
    int32_t resid_ld;
    float* out_f32;
    int32_t out_ld;
    wd_bf16* out_hi;
    wd_bf16* out_lo;
    int32_t out_pl_ld;
    const wd_bf16* w3_hi;
    const wd_bf16* w3_lo;
    const float* b3;
    const float* resid3;
    int32_t resid3_ld;
    double* stat_part;
    int32_t stat_cpg;
    int32_t hw_out;
    int32_t npass;
    const float* x_in;
    int32_t x_in_ld;
    int32_t hw;
    const double* gn_part;
    int32_t gn_nchunk, gn_pcpg, gn_cpg;
    float gn_eps;
    const float* gn_gamma;
    const float* gn_beta;
    const wd_bf16* pi_hi;
    const wd_bf16* pi_lo;
    const float* pi_b;
    const float* ln2_gamma;
    const float* ln2_beta;
    const wd_bf16* mq_a;
    const wd_bf16* mot_a;
    const float* xb_a;
    const wd_bf16* mq_b;
    const wd_bf16* mot_b;
    const float* xb_b;
    const float* ln3_gamma;
    const float* ln3_beta;
    float ln_eps; /* norm2 and norm3 */
    int32_t heads, L;
    float* tok2;
    const wd_bf16* w32_hi; /* folded tail (needs w3, npass 3): see above */
    const wd_bf16* w32_lo;
    const float* b32;
    int32_t dbg; /* 0 in production.  WD_EPI_BATCH_OFF / _ON: the epilogue keeps its row loop / takes the batched form where it is legal,
                    whatever WDIFF_EPI_BATCH says (in the args wd_ff_check returns, WD_EPI_BATCH_BIT = the batched form, as wd_gemm_args.dbg) */
} wd_ff_args;
int wd_ff_fused(const wd_ff_args* args, void* stream);
/* What wd_ff_fused would do with `args`, without launching anything (host only): WD_OK when it accepts them, else WD_EINVAL.  On
 * WD_OK and out != NULL, *out receives the args as the kernel sees them (dbg resolved). */
int wd_ff_check(const wd_ff_args* args, wd_ff_args* out);
int wd_ff_supported(int c, int inner); /* 1 when wd_ff_fused covers the shape */
int wd_ff_args_bytes(void); /* sizeof(wd_ff_args) as this library was built */

/* The number of K slices wd_gemm picks by itself (ksplit = 0, tile = 0) for an m x n x ktot product with a workspace of
 * ws_floats floats and no GEGLU: 1 = no cut.  (What a caller needs to know before it asks for the GroupNorm epilogue.) */
int wd_gemm_auto_ksplit(int m, int n, int ktot, int64_t ws_floats);
/* sizeof(wd_gemm_args) as this library was built: a binding that mirrors the struct (ctypes, cgo, ...) compares its own. */
int wd_gemm_args_bytes(void);
/* 1 when the library was built with -DWDIFF_EXPERIMENTAL: the opt-in GEMM variants that measured slower than the defaults (slab
 * order w_layout 1, the row-shared-taps convolution WDIFF_CONV3, the loader-wave ring WDIFF_GEMM_V8, the ping-pong K-half
 * WDIFF_GEMM_PP) are then compiled in; otherwise w_layout 1 is an error and the other switches are ignored. */
int wd_gemm_experimental(void);

/* GroupNorm statistics, unet.py:427-431 (eps 1e-5) and :161-162 (eps 1e-6).  x: [B*hw][ld] fp32 with c channels in
 * groups of cpg.  Writes per (sample, chunk, group) partial (sum, sumsq) in double: part[((b*nchunk + j)*(c/cpg) + g)*2],
 * nchunk = wd_gn_nchunk(hw).  (wd_gemm can produce the same array in its epilogue: wd_gemm_args.stat_part.)
 * Accuracy: the partials are the sum and the sum of squares of the fp32 values to double rounding (every stage in double; the
 * square of an fp32 value is exact there), so the consumers' var = sumsq / n - mean^2 loses nothing to the producer at any
 * mean / std of a group - tests/test_gpu_norm_offset.py runs it to 256. */
int wd_gn_nchunk(int hw);
int wd_gn_stats(const float* x, int ld, int batch, int hw, int c, int cpg, double* part, void* stream);
/* part[batch][nchunk][ngroups][2] -> out[batch][1][ngroups][2] (fixed-order sum over the chunks): lets wd_gn_apply run with
 * nchunk = 1 where a sample has many chunks (every workgroup of wd_gn_apply folds the chunks itself otherwise). */
int wd_gn_fold_chunks(const double* part, int batch, int nchunk, int ngroups, double* out, void* stream);

/* Normalise (+ optional SiLU) channels [0, c) of x with groups of cpg channels and emit split-bf16 planes
 * out[m][c_off + ch].  `part` holds nchunk partials per sample at a granularity of part_cpg channels (part_cpg | cpg: a
 * 320-channel tensor keeps 10-channel partials that also serve the 20-channel groups of a 640-channel concat norm).
 * gamma/beta are the norm's full affine vectors (indexed at c_off + ch).  raw_hi != NULL: also the un-normalised input
 * as planes for a 1x1 skip convolution (unet.py:632,671). */
int wd_gn_apply(const float* x, int ld, int batch, int hw, int c, int cpg, const double* part, int nchunk, int part_cpg,
                const float* gamma, const float* beta, float eps, int silu,
                wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, int c_off,
                wd_bf16* raw_hi, wd_bf16* raw_lo, void* stream);

/* The same over the channel concat of TWO tensors (the decoder ResBlocks: [h | skip], unet.py:1586-1588 + :427-431) in one
 * launch: source a fills columns [c_off_a, c_off_a + ca) of the planes, source b [c_off_b, c_off_b + cb); gamma / beta are
 * indexed by the concat channel. */
int wd_gn_apply2(const float* xa, int lda, int ca, const double* part_a, int nchunk_a, int part_cpg_a, int c_off_a,
                 const float* xb, int ldb, int cb, const double* part_b, int nchunk_b, int part_cpg_b, int c_off_b,
                 int batch, int hw, int cpg, const float* gamma, const float* beta, float eps, int silu,
                 wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, wd_bf16* raw_hi, wd_bf16* raw_lo, const int32_t* perm_a, void* stream);

/* out[b][o][y][x] (NCHW, o < oc <= 4) = Conv3x3(SiLU?(GroupNorm(x)))[o] + bias[o] in one launch, fp32 VALU: the UNet's last layer
 * (GroupNorm32, SiLU, conv 320 -> 4; unet.py:1453-1458) and any other few-output-channel 3x3 (pad 1, stride 1).
 * x: token-major fp32 [batch*h*w][ld]; part / nchunk / part_cpg: GroupNorm statistics as for wd_gn_apply; weight: the
 * parameter itself, fp32 [oc][c][3][3].  wd_gn_conv3x3_few_supported(c, w, oc): c % 64 == 0, w <= 64, oc <= 4. */
int wd_gn_conv3x3_few_supported(int c, int w, int oc);
int wd_gn_conv3x3_few(const float* x, int ld, int batch, int h, int w, int c, int cpg, const double* part, int nchunk, int part_cpg,
                      const float* gamma, const float* beta, float eps, int silu, const float* weight, const float* bias, int oc,
                      float* out, void* stream);

/* nn.LayerNorm(c, eps) over the last dim (unet.py:314-316), one row per token -> planes. */
int wd_layernorm(const float* x, int ld, int rows, int c, const float* gamma, const float* beta, float eps,
                 wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, void* stream);

/* fp32 -> split planes (optionally through SiLU). */
int wd_split(const float* x, int ld, int rows, int c, int silu, wd_bf16* out_hi, wd_bf16* out_lo, int out_ld,
             void* stream);

/* softmax(q k^T * scale) v per (sample, head): CrossAttention.forward unet.py:185-279 / unetPhosc.py:176-198
 * and Word_Attention unet.py:823-836 (heads = 1, scale = 1).  q: [B*nq][ldq], k/v: [B*nk][ldk/ldv], head h
 * occupies columns [h*d, (h+1)*d).  Output row = b*out_rows + out_row0 + i; fp32 and/or planes. */
int wd_attention(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                 int batch, int heads, int nq, int nk, int d, float scale,
                 float* out_f32, wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, int out_rows, int out_row0,
                 void* stream);

/* Attention over a context that stays fixed for many calls (the PHOSC cross-attention, unetPhosc.py:241-246 over 10 + 769
 * tokens: the same K / V for all 999 steps of a sampling call).  wd_attention_pack_kv converts K / V [batch*nk][ld] (head h in
 * columns [h*d, (h+1)*d)) ONCE into the split-bf16 key-block images the MFMA kernel keeps in LDS
 * (wd_attention_packed_elems(...) bf16 elements, 16-byte aligned; 0 = shape not covered: nk <= 16 or d not in 16..96 step 16);
 * wd_attention_packed is wd_attention reading those images.  Same arithmetic as wd_attention on the same K / V. */
int64_t wd_attention_packed_elems(int batch, int heads, int nk, int d);
int wd_attention_pack_kv(const float* k, int ldk, const float* v, int ldv, int batch, int heads, int nk, int d,
                         wd_bf16* img, void* stream);
int wd_attention_packed(const float* q, int ldq, const wd_bf16* img, int batch, int heads, int nq, int nk, int d,
                        float scale, float* out_f32, wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, int out_rows,
                        int out_row0, void* stream);

/* timestep_embedding, unet.py:96-116: planes[b][0:half] = cos(t_b * freqs), [half:2*half] = sin(...).
 * freqs[half] is the fp32 table exp(-ln(1e4) k / half) computed by the caller with the reference's op order. */
int wd_timestep_embedding(const int64_t* t, int batch, const float* freqs, int half,
                          wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, void* stream);

/* Cross-attention over <= 10 context tokens, folded and fused (CrossAttention of unet.py:164-279 as used by
 * BasicTransformerBlock unet.py:337-345: x + to_out(softmax(to_q(LN(x)) K^T * scale) V)).
 * wd_xattn_fold (once per context): Mq[b][h*L+j][n] = scale * sum_c K[b*L+j][h*d+c] * Wq[h*d+c][n],
 *                                   Mo[b][h*L+j][n] = sum_c V[b*L+j][h*d+c] * Wo[n][h*d+c]   (fp32; wq [heads*d][c], wo [c][heads*d]).
 * wd_xattn_fused (per step): out = x + bias + softmax_heads(LN(x; gamma, beta, eps) . Mq[b]^T) . Mo[b]; when n_hi != NULL also
 * the following LayerNorm (gamma2, beta2, eps2) of `out` as split-bf16 planes.  Shapes: wd_xattn_supported(c, heads, L).
 * mq_pl / mot_pl (2 * 64 * c bf16 per sample each, zero-initialised by the caller, filled by wd_xattn_fold) are the same
 * matrices as split-bf16 MFMA operands, hi plane then lo plane, stored in the order the consuming MFMA reads them (opaque to
 * the caller: only wd_xattn_fold writes them); when given, the two products of wd_xattn_fused run on MFMA (fp32 VALU
 * otherwise). */
int wd_xattn_supported(int c, int heads, int L);
int wd_xattn_fold(const float* k, int ldk, const float* v, int ldv, int batch, int heads, int L, int d, float scale,
                  const float* wq, const float* wo, int c, float* mq, float* mo, wd_bf16* mq_pl, wd_bf16* mot_pl, void* stream);
int wd_xattn_fused(const float* x, int ld, int batch, int hw, int c, const float* gamma, const float* beta, float eps,
                   const float* mq, const float* mo, int heads, int L, const float* bias, float* out, int out_ld,
                   const float* gamma2, const float* beta2, float eps2, wd_bf16* n_hi, wd_bf16* n_lo, int n_ld,
                   const wd_bf16* mq_pl, const wd_bf16* mot_pl, void* stream);

/* Sampling-time tabulation of the FiLM path (time_embed + label_emb + SiLU + every emb_layers, unet.py:1550-1581,609-615):
 * wd_emb_combine writes SiLU(time[t] + label[y_b]) for T consecutive timesteps (time points at the first one) and every
 * sample b as operand planes (row t*B + b; y_b is clamped to [0, num_classes) - the host range-checks it, the reference
 * raises an index error), one wd_gemm then gives the FiLM vectors of those T steps, and wd_select_rows copies the rows of
 * the current step out of the resident chunk: row ((*t_dev) % chunk)*B + b (chunk = T of the table: one table for all steps).
 * label == NULL: the rows are SiLU(time[t]); out_lo == NULL: the hi plane only.
 * WD_EINVAL (nothing launched): wd_emb_combine - a NULL time / out_hi (or y with a label), ted or out_ld not a multiple of 4,
 * out_ld < ted, time / label not 16-byte aligned, out_hi / out_lo not 8-byte aligned;  wd_select_rows - a NULL pointer,
 * row_floats not a multiple of 4, table / out not 16-byte aligned. */
int wd_emb_combine(const float* time, const float* label, const int64_t* y, int num_classes, int T, int B, int ted,
                   wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, void* stream);
int wd_select_rows(const float* table, const int32_t* t_dev, int batch, int64_t row_floats, int chunk, float* out,
                   void* stream);

/* Writer-style interpolation (unet.py:1558-1573): the label row of a sample is the blend (1 - m_b) * label[s1] + m_b * label[s2]
 * of two writers, evaluated in fp32 as two products and one sum.  pairs is int32 (s1, s2) per row, mix is fp32 [B]; ids are
 * clamped to [0, num_classes) - the host range-checks them.
 * wd_emb_combine_mix: wd_emb_combine with that blend as the label term; pairs is [T][B][2] (row t*B + b).  With m_b = 0 / 1 the
 * planes equal wd_emb_combine's for y_b = s1 / s2 bit for bit.
 * wd_label_mix: the blended rows themselves, out fp32 [B][ted], pairs [B][2] (the residual rows of the time_embed.2 GEMM on
 * the path that does not tabulate); WD_EINVAL (nothing launched): a NULL pointer, ted % 4, label / out not 16-byte aligned. */
int wd_emb_combine_mix(const float* time, const float* label, const int32_t* pairs, const float* mix, int num_classes, int T, int B,
                       int ted, wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, void* stream);
int wd_label_mix(const float* label, const int32_t* pairs, const float* mix, int num_classes, int B, int ted, float* out,
                 void* stream);

/* Two chained folded cross-attentions in one launch (attn1 then attn2 of a base-model BasicTransformerBlock, unet.py:337-345;
 * both read LayerNorm parameters of their own, here norm2 twice): out = B(A(x)) with A/B = x + bias + softmax(LN(x).Mq^T).Mo,
 * optionally followed by the next LayerNorm as operand planes.  MFMA form only (planes from wd_xattn_fold). */
int wd_xattn_pair(const float* x, int ld, int batch, int hw, int c, float eps, int heads, int L, const float* gamma_a,
                  const float* beta_a, const wd_bf16* mq_pl_a, const wd_bf16* mot_pl_a, const float* bias_a, const float* gamma_b,
                  const float* beta_b, const wd_bf16* mq_pl_b, const wd_bf16* mot_pl_b, const float* bias_b, float* out, int out_ld,
                  const float* gamma2, const float* beta2, float eps2, wd_bf16* n_hi, wd_bf16* n_lo, int n_ld, void* stream);

/* wd_xattn_pair (or, with mq_pl_b == NULL, the single folded cross-attention a in its MFMA form: gamma_b .. bias_b unused) that
 * also writes its result as raw operand planes r_hi / r_lo [rows][r_ld] (r_lo may be NULL): the A operand of a product that
 * reads it next.  out, n_hi / n_lo are what wd_xattn_pair / wd_xattn_fused write, bit for bit. */
int wd_xattn_planes(const float* x, int ld, int batch, int hw, int c, float eps, int heads, int L, const float* gamma_a,
                    const float* beta_a, const wd_bf16* mq_pl_a, const wd_bf16* mot_pl_a, const float* bias_a, const float* gamma_b,
                    const float* beta_b, const wd_bf16* mq_pl_b, const wd_bf16* mot_pl_b, const float* bias_b, float* out, int out_ld,
                    const float* gamma2, const float* beta2, float eps2, wd_bf16* n_hi, wd_bf16* n_lo, int n_ld, wd_bf16* r_hi,
                    wd_bf16* r_lo, int r_ld, void* stream);

/* Per-character attention maps: the head sum of the softmax of one folded cross-attention (the reference's --attentionMaps 1
 * outputs attn1 / attn2 / attn3, unet.py:203-279 (CrossAttention keeps its softmax), 337-345, 405-410, 1645-1832; :1757 sums the
 * heads).  Per token row r of sample b, with A as in wd_xattn_pair:
 *     xa = x[r] (mq_pl_a == NULL: gamma_a .. bias_a unused)   or   xa = A(x[r]) (the attention before the tapped one)
 *     p[h][j] = softmax_j(LN(xa; gamma_b, beta_b, eps) . Mq_b[b][h*L + j]),   m[j] = sum_h p[h][j]
 *     maps[r][j] = m[j]  (wtab == NULL)   or   maps[r][j] + wtab[*k_dev] * m[j]  (product and sum rounded separately, no fma;
 *                                               *k_dev outside [0, wtab_n) counts as weight 0)
 * The same LayerNorm, planes and MFMA score products as wd_xattn_pair / wd_xattn_planes, so p is what the sampling step itself
 * multiplies with Mo; no output product, Mo_b is not read.  maps is fp32 [batch*hw][maps_ld >= L].  k_dev is a device index
 * (the samplers' step index or timestep), so one captured graph serves every step.  Shapes: wd_xattn_supported(c, heads, L);
 * wtab and k_dev come together. */
int wd_xattn_maps(const float* x, int ld, int batch, int hw, int c, float eps, int heads, int L, const float* gamma_a,
                  const float* beta_a, const wd_bf16* mq_pl_a, const wd_bf16* mot_pl_a, const float* bias_a, const float* gamma_b,
                  const float* beta_b, const wd_bf16* mq_pl_b, float* maps, int maps_ld, const float* wtab, int wtab_n,
                  const int32_t* k_dev, void* stream);

/* Two linear layers with nothing between them as one: w32 [c][ffi] = w3 [c][inner] . w2 [inner][ffi] and b32 [c] = w3 . b2 + b3
 * (b2 / b3 may be NULL: zeros).  fp64 products summed in ascending k and rounded once to fp32; no library GEMM.  The folded tail
 * of wd_ff_fused and the two-source ff2 + proj_out GEMM of the SpatialTransformer read the result (unet.py:145,406-412). */
int wd_linear_fold(const float* w3, const float* w2, const float* b2, const float* b3, int c, int inner, int ffi, float* w32,
                   float* b32, void* stream);

/* nn.Embedding lookup + positional encoding (CharacterEncoder, unet.py:860-872; PE skipped when pe == NULL,
 * unetPhosc.py:726-729): planes[r][:] = table[ids[r]][:] + pe[r % seq_len][:]. ids are int64 or int32, clamped to
 * [0, vocab) (the reference raises an index error); out_lo == NULL: the hi plane only.
 * WD_EINVAL (nothing launched): a NULL ids / table / out_hi, c or out_ld not a multiple of 4, out_ld < c, table / pe not
 * 16-byte aligned, out_hi / out_lo not 8-byte aligned. */
int wd_embed_tokens(const void* ids, int ids_are_i64, int rows, int seq_len, const float* table, int vocab, int c,
                    const float* pe, wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, void* stream);

/* x NCHW [B][cin][h][w] -> im2col planes [B*h*w][kpad], column tap*cin + ci (3x3, pad 1); unet.py:1251. */
int wd_im2col3x3(const float* x, int batch, int cin, int h, int w, wd_bf16* out_hi, wd_bf16* out_lo, int kpad,
                 void* stream);

/* The first layer as a direct fp32 convolution (3x3, pad 1, cin <= 4; unet.py:1251), without im2col planes:
 * out[(b*h*w + p)*ld + o] = bias[o] + sum weight[o][ci][tap] * x[b][ci][..] (fp32 FMAs), weight = the parameter [cout][cin][3][3].
 * part (may be NULL): GroupNorm statistics partials [batch][wd_conv3x3_in_nchunk(h*w)][cout / stat_cpg][2] in fp64 (sum, sum of
 * squares of the fp32 results over 64-token chunks) - the layout wd_gemm's stat_part has for 64-row panels, read by wd_gn_apply.
 * wd_conv3x3_in_supported(cin, h, w, cout): 1 <= cin <= 4, w <= 64, (h + 2) * (w + 2) <= 2048, cout % 4 == 0, cout <= 2048, and
 * the padded sample + the weights within 64 KB of LDS. */
int wd_conv3x3_in_supported(int cin, int h, int w, int cout);
int wd_conv3x3_in_nchunk(int hw);
int wd_conv3x3_in(const float* x, int batch, int cin, int h, int w, const float* weight, const float* bias, int cout, float* out,
                  int ld, double* part, int stat_cpg, void* stream);

/* layout changes at the API edge: NCHW [B][c][hw] <-> token-major [B*hw][ld]. */
int wd_nchw_to_tokens(const float* x, int batch, int c, int hw, float* out, int ld, void* stream);
int wd_tokens_to_nchw(const float* x, int ld, int batch, int c, int hw, float* out, void* stream);

/* One reverse-diffusion update, train.py:229-236, on n elements per sample (any layout):
 *   x = ca[t] * (x - cb[t] * eps) + cs[t] * z,   z = 0 when t <= 1,
 * evaluated with the reference's rounding order (no fma contraction), ca = 1/sqrt(alpha), cb = (1-alpha)/sqrt(1-alpha_hat),
 * cs = sqrt(beta) tabulated by the caller.  t = *t_dev (device int32, so that a captured graph can be replayed).
 * noise != NULL: z is read from it (parity tests); else z ~ N(0,1) from Philox4x32-10 keyed by seed with counter
 * (element/4, t, sample_offset + sample index): a sample's noise does not depend on how the batch is sharded.
 * WD_EINVAL (nothing launched): a NULL required pointer, n_per_sample % 4, x / eps / noise not 16-byte aligned. */
int wd_ddpm_step(float* x, const float* eps, int batch, int n_per_sample, const float* ca, const float* cb,
                 const float* cs, const int32_t* t_dev, const float* noise, uint64_t seed, uint64_t sample_offset,
                 void* stream);

/* wd_ddpm_step on the guided prediction eps = torch.lerp(second, first, scale) (train.py:228), formed as torch forms it:
 * first - (first - second) * (1 - scale) when |scale| >= 0.5, second + scale * (first - second) otherwise.  The update and the
 * Philox stream are wd_ddpm_step's, bit for bit.  eps_out != NULL also receives eps.
 * WD_EINVAL (nothing launched): as wd_ddpm_step, for x / first / second / eps_out / noise. */
int wd_ddpm_step_cfg(float* x, const float* first, const float* second, float scale, float* eps_out, int batch, int n_per_sample,
                     const float* ca, const float* cb, const float* cs, const int32_t* t_dev, const float* noise, uint64_t seed,
                     uint64_t sample_offset, void* stream);

/* *t_dev += delta; t64[b] = *t_dev for b < batch (the int64 timesteps vector the UNet takes, train.py:222). */
int wd_advance_timestep(int32_t* t_dev, int delta, int64_t* t64, int batch, void* stream);

/* One DDIM update (Song et al. 2020, eq. 12) over a subsequence tau of S visited timesteps; k = *k_dev is the index of the
 * current one, t = *t_dev = tau[k] its timestep.  With a = alpha_hat[tau[k]], p = alpha_hat of the predecessor (tau[k+1];
 * alpha_hat[0] after the last entry) and sigma = eta * sqrt((1-p)/(1-a)) * sqrt(1 - a/p), the caller tabulates per k
 *   c1 = sqrt(1-a), c2 = 1/sqrt(a), c3 = sqrt(p), c4 = sqrt(max(1 - p - sigma^2, 0)), c5 = sigma   (fp32 [S] each)
 * and the kernel evaluates, every operation rounded to fp32 on its own and in this order (no fma contraction),
 *   x0 = (x - c1[k] * e) * c2[k];   x = (c3[k] * x0 + c4[k] * e) + c5[k] * z.
 * e = eps, or torch.lerp(second, eps, scale) when second != NULL, bit for bit as torch's device kernel forms it for any
 * weight: fma(-(eps - second), 1 - scale, eps) for |scale| >= 0.5, fma(scale, eps - second, second) below - one rounding
 * each, where wd_ddpm_step_cfg rounds the product and the sum separately (the same value where the product is exact, as
 * at scale = 3).  eps_out != NULL receives e.
 * z: read from noise when given, else the draw wd_ddpm_step makes for (seed, sample_offset + sample index, t) - a sample's
 * noise at timestep t is the DDPM sampler's, whatever the batch size or sharding.  c5[k] == 0 (eta = 0): z is neither read
 * nor drawn and the term is omitted (not multiplied by zero).  WD_EINVAL: a required pointer is NULL, n_per_sample % 4, or
 * x / eps / second / noise / eps_out is not 16-byte aligned. */
int wd_ddim_step(float* x, const float* eps, const float* second, float scale, float* eps_out, int batch, int n_per_sample,
                 const float* c1, const float* c2, const float* c3, const float* c4, const float* c5, const int32_t* k_dev,
                 const int32_t* t_dev, const float* noise, uint64_t seed, uint64_t sample_offset, void* stream);

/* One DPM-Solver++(2M) update (Lu et al. 2022, algorithm 2: the data-prediction multistep solver) over a subsequence tau of S
 * visited timesteps; k = *k_dev is the index of the current one.  With a = alpha_hat[tau[k]], p = alpha_hat of the predecessor
 * (tau[k+1]; alpha_hat[0] after the last entry), lambda(v) = ln(v / (1-v)) / 2 and h_k = lambda(p) - lambda(a), the caller
 * tabulates per k
 *   c1 = sqrt(1-a), c2 = 1/sqrt(a), c3 = sqrt((1-p)/(1-a)), c4 = -sqrt(p) * expm1(-h_k), c5 = h_k / (2 h_{k-1})   (fp32 [S] each)
 * with c5 = 0 where the step is first order (k = 0, the last step, every step at order 1), and the kernel evaluates, every
 * operation rounded to fp32 on its own and in this order (no fma contraction),
 *   x0 = (x - c1[k] * e) * c2[k];
 *   D  = x0,  or  x0 + c5[k] * (x0 - x0_prev)  when c5[k] != 0;
 *   x  = c3[k] * x + c4[k] * D;
 *   x0_prev = x0   (always written).
 * c5[k] == 0: x0_prev is NOT read (the first step sees an uninitialised buffer) and the term is omitted, not multiplied by
 * zero.  e = eps, or torch.lerp(second, eps, scale) when second != NULL, formed as wd_ddim_step forms it; eps_out != NULL
 * receives e.  x0_prev is a caller-owned buffer of x's shape that lives across the steps of one trajectory.
 * WD_EINVAL: a required pointer (x, eps, x0_prev, c1..c5, k_dev) is NULL, n_per_sample % 4, or x / eps / second / eps_out /
 * x0_prev is not 16-byte aligned. */
int wd_dpmpp_step(float* x, const float* eps, const float* second, float scale, float* eps_out, float* x0_prev, int batch,
                  int n_per_sample, const float* c1, const float* c2, const float* c3, const float* c4, const float* c5,
                  const int32_t* k_dev, void* stream);

/* The table-driven wd_advance_timestep: k = min(*k_dev + 1, S - 1); *k_dev = k; *t_dev = tau[k]; t64[b] = tau[k] for b < batch
 * (tau int32 [S]).  After the last visited step k stays at S - 1. */
int wd_next_timestep(int32_t* k_dev, const int32_t* tau, int S, int32_t* t_dev, int64_t* t64, int batch, void* stream);

/* N(0,1) fill with the same Philox stream family (x_T, train.py:217; noise_images eps, train.py:193).
 * WD_EINVAL (nothing launched): out NULL or not 16-byte aligned, n_per_sample % 4. */
int wd_randn(float* out, int batch, int n_per_sample, uint64_t seed, uint64_t sample_offset, uint32_t stream_id,
             void* stream);

/* The tail of AutoencoderKL.encode (train.py:277-278: vae.encode(images).latent_dist.sample() * 0.18215) in one launch:
 * quant_conv (1x1, 2L -> 2L), chunk into mean | logvar, clamp, the posterior draw, the scale and the layout change.
 *   moments_tok  encoder.conv_out's token-major fp32 output [batch*hw][ld], ld >= 2L, columns 0..2L-1 read;
 *   w, bias      quant_conv.weight [2L][2L](x1x1) and .bias [2L], fp32, reference layout - never split into bf16 planes (logvar
 *                goes through exp: a 1e-5 relative error of the split would be multiplied by |logvar| / 2);
 *   mean, logvar NCHW fp32 [batch][L][hw]; logvar is clamped to [-30, 20] (NaN passes, as torch.clamp);
 *   sample       NULL, or NCHW fp32: scale * (mean + exp(0.5 * logvar) * z).
 * Rounding order (plain fp32, no fma contraction anywhere): output o of quant_conv at a position with moments x is
 *   ((w[o][0]*x[0] + w[o][1]*x[1]) + ... + w[o][2L-1]*x[2L-1]) + bias[o]    - products rounded, summed left to right, bias last;
 * the draw is  t0 = 0.5f*logvar; t1 = expf(t0); t2 = t1*z; t3 = mean + t2; sample = scale*t3, each rounded on its own.
 * noise != NULL (needs sample): z is read from it (NCHW, parity tests).  Otherwise z ~ N(0,1) from Philox4x32-10, bit-identical
 * to what wd_randn writes for (batch, L*hw, seed, sample_offset, WD_STREAM_VAE_POSTERIOR): sample i depends on
 * (seed, sample_offset + i) only, not on how a batch is cut into launches.
 * WD_EINVAL (nothing launched): a NULL required pointer, L outside 1..WD_VAE_MAX_LATENT, ld < 2L, L*hw not a multiple of 4,
 * noise without sample, mean / logvar / sample / noise not 16-byte aligned.  Does not allocate or synchronise (capturable). */
#define WD_VAE_MAX_LATENT 8
#define WD_STREAM_VAE_POSTERIOR 3 /* stream ids taken so far: 0 x_T, 1 noise_images eps, 2 the training step's eps, 3 this one; */
#define WD_STREAM_KNOWN 4         /* 4: the per-sample fixed eps of a known-region call (wd_known_blend below), via wd_randn; */
#define WD_STREAM_DROPOUT0 0x100  /* 0x100 + layer: the training dropout mask of ResBlock `layer` (wd_dropout below) */
#define WD_STREAM_LABEL_DROP 5    /* 5: the per-sample writer dropout of a training step (wd_label_rows_keep below) */
int wd_vae_posterior(const float* moments_tok, int ld, const float* w, const float* bias, int batch, int L, int hw, float* mean,
                     float* logvar, float* sample, float scale, const float* noise, uint64_t seed, uint64_t sample_offset,
                     void* stream);

/* The same draw from stored moments (latent_dist.sample() called after encode): mean, logvar (already clamped), sample and
 * noise are fp32 [batch][n_per_sample], n_per_sample % 4 == 0, 16-byte aligned; z as in wd_vae_posterior, bit for bit. */
int wd_posterior_sample(const float* mean, const float* logvar, int batch, int n_per_sample, float* sample, float scale,
                        const float* noise, uint64_t seed, uint64_t sample_offset, void* stream);

/* x_t = sqrt_ah[t_b] * x + sqrt_1m_ah[t_b] * eps  (Diffusion.noise_images, train.py:190-194); the two tables
 * sqrt(alpha_hat) and sqrt(1 - alpha_hat) are tabulated by the caller (fp32, reference op order). */
int wd_noise_images(const float* x, const float* eps, const int64_t* t, const float* sqrt_ah, const float* sqrt_1m_ah,
                    int batch, int n_per_sample, float* out, void* stream);

/* Known-region conditioning (inpainting as in RePaint, Lugmayr et al. 2022): after a sampler's update and BEFORE its timestep
 * advance, x [batch][n_per_sample] is at the level of the predecessor p of the step just taken, read on the device so that a
 * captured graph replays:
 *   tau == NULL (DDPM form):  p = *t_dev - 1;
 *   otherwise, k = *k_dev:    p = tau[k + 1] if k + 1 < S, else 0   (tau int32 [S], the visited timesteps of wd_next_timestep).
 * Where the mask keeps, x is replaced by the known latent x0 noised to that level.  Per element, every operation rounded to
 * fp32 on its own and in this order (no fma contraction):
 *   kv = x0                                   when p == 0: the trajectory ends on the known latent itself, noise-free;
 *   kv = sqrt_ah[p] * x0 + sqrt_1m_ah[p] * z  otherwise - the expression of wd_noise_images, bit for bit;
 *   x  = x (its bits, untouched by arithmetic) where m == 0,  kv where m == 1,  x + m * (kv - x) otherwise.
 * x0, mask (values in [0, 1], 1 = keep) and noise are fp32 [batch][n_per_sample]; the two tables are wd_noise_images'.
 * z: read from noise when given (one fixed eps per sample, or the parity tests); else drawn from Philox4x32-10 keyed by seed
 * with counter (element / 4, WD_TAG_KNOWN | p, sample_offset + sample index) - a tag family of its own, disjoint from the
 * step kernels' bare timestep t (< 2^30) and from the 0x80000000 | stream_id tags of wd_randn, so a step that draws its own
 * noise at level p and this blend never share a draw.  What is drawn for a group of four elements does not depend on the mask;
 * at p == 0 neither noise is read nor anything drawn.
 * WD_EINVAL (nothing launched): x, x0, mask or a table is NULL, n_per_sample % 4, x / x0 / mask / noise not 16-byte aligned,
 * tau given with S < 1 or without k_dev, tau and t_dev both NULL.  Does not allocate or synchronise (capturable). */
#define WD_TAG_KNOWN 0x40000000
int wd_known_blend(float* x, const float* x0, const float* mask, int batch, int n_per_sample, const float* sqrt_ah,
                   const float* sqrt_1m_ah, const int32_t* t_dev, const int32_t* k_dev, const int32_t* tau, int S,
                   const float* noise, uint64_t seed, uint64_t sample_offset, void* stream);

/* Resampling jumps of a known-region call (RePaint, Lugmayr et al. 2022, section 4.2 and algorithm 1).  The reverse loop of a
 * resampled call walks a table of entries: entry k = *k_dev starts from the level tau'[k] (the table wd_next_timestep and
 * wd_known_blend read) and is either a sampler's ordinary step down the schedule or a jump back UP it.
 *
 * wd_forward_jump, the up entry: x [batch][n_per_sample] at the level `from` is diffused forward to the level `to` > from,
 *   x = g1[k] * x + g2[k] * z,   both products and the sum rounded to fp32 on their own (no fma contraction),
 * with g1 = sqrt(Q/A), g2 = sqrt(1 - Q/A), A = alpha_hat[from], Q = alpha_hat[to], tabulated per walk entry by the caller
 * (float64, rounded to fp32 once; fp32 [entries], read at k only).  Kept and free cells are diffused alike.
 *
 * wd_walk_randn: out [batch][n_per_sample] = N(0,1), the noise a down entry's kernels then read through their `noise`
 * argument - `which` = WD_WALK_STEP for the step's z, WD_WALK_BLEND for the z of a wd_known_blend that draws per step.
 *
 * The draw, in both: z is read from `noise` when given (wd_forward_jump), else it comes from Philox4x32-10 keyed by seed with
 * counter (element / 4, WD_TAG_WALK | which << 26 | k, sample_offset + sample index), which = WD_WALK_JUMP for the jump.  k is
 * the WALK INDEX, not the timestep: a level that is visited twice draws afresh on each visit, which the timestep-keyed draws
 * of wd_ddpm_step, wd_ddim_step and wd_known_blend would not.  A row's draws depend on (seed, sample_offset + row, k) only.
 * WD_TAG_WALK is the fourth tag family and the four are disjoint in the tag's top two bits: a bare timestep t < 2^30 has 00,
 * WD_TAG_KNOWN | p (p < 2^30) has 01, 0x80000000 | stream_id (stream ids < 2^30) has 10, and WD_TAG_WALK | which << 26 | k
 * (which <= 2 < 4, k < 2^26, so everything below bit 28) has 11.  The caller keeps k < 2^26; the kernels use k's low 26 bits.
 * WD_EINVAL (nothing launched): a NULL required pointer (x, g1, g2, k_dev; out, k_dev), n_per_sample % 4, x / noise / out not
 * 16-byte aligned, which outside 0 .. 2.  Neither allocates nor synchronises (capturable). */
#define WD_TAG_WALK 0xC0000000
#define WD_WALK_STEP 0
#define WD_WALK_BLEND 1
#define WD_WALK_JUMP 2
int wd_forward_jump(float* x, int batch, int n_per_sample, const float* g1, const float* g2, const int32_t* k_dev,
                    const float* noise, uint64_t seed, uint64_t sample_offset, void* stream);
int wd_walk_randn(float* out, int batch, int n_per_sample, uint64_t seed, uint64_t sample_offset, int which,
                  const int32_t* k_dev, void* stream);

/* Line sampling as overlapping windows (MultiDiffusion, Bar-Tal et al. 2023): a line latent, fp32 [lines][c][h][wl], is denoised
 * as K windows of the model's own width w per line; window k of line s is model batch row b = s * K + k and begins at line
 * column o = offsets[b] (int32 [lines][K], on the device so that a captured graph replays).  A window that does not fit
 * (o < 0 or o + w > wl) is treated as absent; every access is checked against wl and w whatever offsets holds.
 *
 * wd_window_gather, before the forward(s):  win[b][ch][r][j] = line[s][ch][r][o + j] - the bits are copied, no arithmetic; an
 * absent window is written 0.  win is fp32 [lines * K][c][h][w].
 *
 * wd_window_blend, after them: the K predictions of a line averaged into one line-wide prediction with the normalised weights
 * wn, fp32 [lines][K][w] (the caller divides each window's profile by the sum over the windows that cover the column, in float64,
 * and rounds to fp32 once).  Per line element (s, ch, r, J), over the windows k in ascending order that have o <= J < o + w and
 * wn[s][k][J - o] != 0, every product and every sum rounded to fp32 on its own (no fma contraction):
 *   acc = wn * e          for the first such window;
 *   acc = acc + wn * e    for each later one;
 *   line[s][ch][r][J] = acc,  or 0.0f where no window has a weight (the caller refuses such layouts).
 * A window whose weight is 0 at that column is skipped, not multiplied: its prediction is not read there and a NaN in it does
 * not spread.  A single covering window with weight 1 returns its value with its bits, -0.0 included (acc starts from the first
 * product, not from 0).  win1 / line1: NULL together, or the second prediction of a guided step, blended with the same weights
 * into a line buffer of its own in the same launch; line0 is the same either way.
 * One output element per lane in both kernels: offsets are arbitrary, so a window's rows are not 16-byte aligned in general.
 * WD_EINVAL (nothing launched): a NULL required pointer, win1 without line1 or the reverse, K outside 1..WD_WINDOW_MAX, w < 1,
 * wl < w, lines, c or h < 1.  Neither allocates nor synchronises (capturable). */
#define WD_WINDOW_MAX 32
int wd_window_gather(const float* line, const int32_t* offsets, int lines, int K, int c, int h, int w, int wl, float* win,
                     void* stream);
int wd_window_blend(const float* win0, const float* win1, const float* wn, const int32_t* offsets, int lines, int K, int c,
                    int h, int w, int wl, float* line0, float* line1, void* stream);

/* strided device-to-device copy (rows x width_bytes); used to materialise a channel concat (unet.py:1750) only when
 * GroupNorm groups straddle the concat boundary. */
int wd_copy2d(void* dst, int64_t dst_pitch, const void* src, int64_t src_pitch, int64_t width_bytes, int64_t rows,
              void* stream);

/* EMA of weights, train.py:151-159: ema = ema * beta + (1 - beta) * p over one flat fp32 buffer. */
int wd_ema_update(float* ema, const float* p, int64_t n, double beta, void* stream);

/* Multi-tensor fused AdamW (+ EMA of the weights) - the optimiser side of the training step, train.py:290-294,405,146-170.
 * table: device array of ntensor wd_adamw_table_entry records, chunk0 = running sum of ceil(n / wd_adamw_chunk());
 * total_chunks = that sum over all tensors.  Same fp32 op order as torch.optim.AdamW's single-tensor update at `step`
 * (1-based).  ema_mode 0: none, 1: ema = p (the first 2000 steps of the reference), 2: ema = ema*beta + (1-beta)*p. */
typedef struct wd_adamw_table_entry {
    float* p;
    const float* g; /* NULL: the loss does not reach the parameter; AdamW skips it, the EMA still runs */
    float* m;
    float* v;
    float* ema;     /* may be NULL */
    int64_t n;
    int64_t chunk0; /* index of this tensor's first chunk */
} wd_adamw_table_entry;
int wd_adamw_table_entry_bytes(void); /* sizeof(wd_adamw_table_entry) as this library was built */
int wd_adamw_chunk(void);
int wd_adamw_multi(const void* table, int ntensor, int64_t total_chunks, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int64_t step, int ema_mode, double ema_beta, void* stream);

/* wd_adamw_multi on gradients scaled by a factor that lives on the device: every workgroup reads *gscale once and uses
 * g = fp32(table.g[i] * *gscale), the product rounded on its own; everything after that is wd_adamw_multi's op order.  The
 * gradient buffers are not written.  gscale is ctl + 1 of wd_grad_sqnorm_multi for global-norm clipping. */
int wd_adamw_multi_scaled(const void* table, int ntensor, int64_t total_chunks, double lr, double beta1, double beta2,
                          double eps, double weight_decay, int64_t step, int ema_mode, double ema_beta, const float* gscale,
                          void* stream);

/* Global L2 norm of the gradients of a wd_adamw_multi table and the clip coefficient of torch.nn.utils.clip_grad_norm_, on
 * the device (two launches, no atomics, fixed summation order: bit-identical from run to run).  Stage 1: one workgroup per
 * chunk of the table sums (double)g * (double)g in double into partial[chunk] (entries with g == NULL give 0); stage 2: one
 * workgroup adds the total_chunks partials in a fixed order and writes
 *   ctl[0] = (float)sqrt(sum)                               the norm, one rounding of the double sum
 *   ctl[1] = min(1.0f, max_norm / (ctl[0] + 1e-6f))         in fp32; a NaN quotient stays NaN (torch.clamp)
 * max_norm = +inf gives ctl[1] = 1 for every finite norm: the norm is only measured.  partial: total_chunks doubles of
 * scratch; ctl: 2 floats.  WD_EINVAL: a NULL pointer, max_norm <= 0 or NaN. */
int wd_grad_sqnorm_multi(const void* table, int ntensor, int64_t total_chunks, double* partial, float max_norm, float* ctl,
                         void* stream);

/* Row-wise AdamW over a few rows of one embedding table (fitting new writers: DESIGN.md "Fitting new writers").  The row list is
 * a HOST array of nrows distinct ids in [0, vocab), nrows in [1, WD_ROWS_MAX]; it is handed to the kernels by value, so nothing on
 * the device has to outlive the call.  Both entry points return WD_EINVAL, with nothing launched, for: nrows outside
 * [1, WD_ROWS_MAX], a row outside [0, vocab), duplicate rows, c % 4 != 0 (wd_adamw_rows), a NULL required pointer, a table,
 * compact buffer or anchor that is not 16-byte aligned, ld / ema_ld that is not a multiple of 4 floats or < c.
 *
 * wd_row_slots: slots[b] = j where rows[j] == ids[b], else -1 (ids int64 [n], any value; slots int64 [n]).  slots is the `ids`
 * argument of wd_embedding_bwd with vocab = nrows, which gives rows with id -1 no gradient: the gradient of the listed rows lands
 * in a compact fp32 [nrows][c] buffer, in the summation order the full table uses.
 *
 * wd_adamw_rows: one launch updates table[rows[j]][0:c] (row pitch ld floats) for every j.  grad, m, v and the optional anchor
 * are compact [nrows][c]; ema_table (NULL allowed) is a second table of vocab rows, pitch ema_ld, updated at the same rows under
 * ema_mode 0 / 1 / 2 as wd_adamw_multi does; gscale (NULL allowed) is the device scalar of wd_adamw_multi_scaled.  With
 * anchor == NULL the arithmetic is wd_adamw_multi's, in its fp32 op order.  With an anchor the decoupled decay pulls towards it:
 *   p = p - fp32(lr * weight_decay) * (p - a)
 * replaces p = p * fp32(1 - lr * weight_decay); every operation is rounded on its own and no product is contracted.  No row that
 * is not listed is read or written, in either table; every (row, column) cell has one writer. */
#define WD_ROWS_MAX 64
int wd_row_slots(const int64_t* ids, int n, const int* rows, int nrows, int vocab, int64_t* slots, void* stream);
int wd_adamw_rows(float* table, int ld, int c, const int* rows, int nrows, int vocab, const float* grad, float* m, float* v,
                  const float* anchor, float* ema_table, int ema_ld, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int64_t step, int ema_mode, double ema_beta, const float* gscale, void* stream);

/* dst[i] = scale * (overwrite ? src[i] : dst[i] + src[i]) over n fp32 elements, each operation rounded on its own.  With
 * overwrite != 0 dst is never read (it may hold anything, NaN included).  16-byte accesses where dst and src reach a 16-byte
 * boundary at the same element, scalar accesses for the ragged ends (or throughout).  dst and src must not overlap. */
int wd_grad_accumulate(float* dst, const float* src, int64_t n, int overwrite, float scale, void* stream);

/* Table-driven weight repack (one launch refreshes every packed operand after an optimiser step; the reference reads
 * its parameters in place, unet.py forward).  table: device array of nentries wd_repack_entry records (below), one per piece
 * of a packed operand.
 * mode 0: dst[perm_g(n)][t*C + c]   = split(src0[n][c][t])   (forward operand; perm_g = GEGLU x|gate interleave, g=0 none)
 * mode 1: dst[c][t*npad + n]        = split(src0[n][c][t]), 0 for N <= n < npad   (data-gradient operand)
 * mode 2: dstf[perm_g(i)]           = src0[i] (+ src1[i]), i < N   (fp32 vectors)
 * mode 3: mode 0's matrix written fragment-major (the image wd_gemm_pack_w makes of it); dst = the image's base, ld = the matrix's
 *         row count (% 16 == 0), the piece sits at (row_off, col_off); needs C % 32 == 0, T in {1, 9}, even col_off
 * dst pointers are pre-offset to the piece's (row, column) origin; ld = row pitch in elements.  A mode-0/1 piece owns
 * ceil(N or npad / tile) * ceil(C / tile) chunks (tile = wd_repack_tile()), a mode-2 piece ceil(N / wd_repack_vchunk()). */
typedef struct wd_repack_entry {
    const float* src0; /* [N][C][T] (T = 9 for 3x3 kernels, 1 for linears) or a vector of N floats */
    const float* src1; /* NULL, or a second addend (mode 2 only: conv bias + skip bias) */
    void* dst_hi;      /* planes: the bf16 hi plane; mode 2: the fp32 destination */
    void* dst_lo;
    int32_t N, C, T, mode;
    int32_t npad, ld, g, ntile_c; /* ntile_c = ceil(C / tile) */
    int64_t chunk0;    /* index of this piece's first chunk */
    int32_t row_off, col_off; /* mode 3 only */
} wd_repack_entry;
int wd_repack_entry_bytes(void); /* sizeof(wd_repack_entry) as this library was built */
int wd_repack_tile(void);
int wd_repack_vchunk(void);
int wd_repack_multi(const void* table, int nentries, int64_t total_chunks, void* stream);

/* loss = mean((pred - target)^2) (nn.MSELoss, train.py:289; deterministic two-stage sum) and, when grad != NULL,
 * grad = d loss / d pred = 2 (pred - target) / n.  scratch: >= min(1024, ceil(n/256)) doubles. */
int wd_mse_loss(const float* pred, const float* target, int64_t n, float* grad, float* loss, double* scratch,
                int scratch_len, void* stream);

/* Weighted, masked per-sample squared error and its gradient (two launches, no atomics, fixed summation order: the same bits on
 * every run).  pred, target, grad: fp32 [batch][n_per_sample]; mask: NULL, or fp32 [batch][n_per_sample] with values in [0, 1];
 * t: int64 [batch] on the device; weights: NULL (w_b = 1), or fp32 [T] with w_b = weights[t_b].  No product is contracted:
 *   d   = pred - target                                   in fp32
 *   M_b = sum_i (double)m_bi                              (n_per_sample without a mask)
 *   S_b = sum_i (double)m_bi * ((double)d * (double)d)    both sums in double
 *   l_b = (float)(S_b / M_b)                              the UNWEIGHTED masked mean of sample b -> sample_loss[b] (optional)
 *   c_b = (float)(2.0 * (double)w_b / ((double)batch * M_b))
 *   grad = c_b * d without a mask, c_b * (m * d) with one, each product rounded on its own (grad may be NULL)
 *   loss = (float)((sum_b (double)w_b * (S_b / M_b)) / batch), b ascending
 * A sample with M_b == 0 contributes nothing: l_b = 0, its gradient row is 0 (not NaN) and the histogram skips it; otherwise NaN
 * and inf propagate by plain arithmetic.  hist: NULL, or double [nbins][2] = (sum, count), ACCUMULATED INTO: for b ascending,
 * bin = (t_b * nbins) / T in integers, hist[bin][0] += (double)l_b (the rounded fp32 value), hist[bin][1] += 1.
 * scratch: >= 2 * batch doubles.  With weights == NULL and mask == NULL grad is wd_mse_loss's, bit for bit.
 * t outside [0, T) is a precondition (the callers check host timesteps).  The function neither allocates nor synchronises.
 * WD_EINVAL (nothing launched): pred, target, loss or scratch NULL; t NULL or T < 1 with weights or hist; nbins < 1 with hist;
 * batch < 1; n_per_sample < 4 or not a multiple of 4; pred / target / mask / grad not 16-byte aligned. */
int wd_weighted_mse_loss(const float* pred, const float* target, const float* mask, int batch, int n_per_sample,
                         const int64_t* t, const float* weights, int T, float* grad, float* loss, float* sample_loss,
                         double* hist, int nbins, double* scratch, void* stream);

/* CTC loss of nn.CTCLoss(reduction='sum', zero_infinity=True)(log_softmax(logits, 2), ...) (trainModifyCondition.py:73,757-799)
 * and its gradient with respect to the RAW logits (the log-softmax is folded in), forward and backward in one call: two launches,
 * no atomics on floating-point values, fixed summation order (the same bits on every run).  The blank is class 0.
 *   logits      fp32, row (t, b) at logits + (t * batch + b) * ld, C classes per row, ld >= C
 *   targets     int32 (targets_i64 = 0) or int64 (1), sample b at targets + b * tld, tld >= Lmax; may be NULL when Lmax == 0
 *   input_len, target_len  int32 [batch] on the device
 *   dlogits     NULL (loss only) or fp32 in the layout of logits with its own pitch dld >= C; EVERY row t < T of it is written
 *   sample_nll  fp32 [batch]: -log P(target_b | logits_b), unscaled; +inf when no alignment exists
 *   loss        fp32 [1] = (float)((double)scale * sum_b nll_b), b ascending in double, over the samples that count
 *   status      int32 [batch]: 0, or bit 0 input_len outside [1, T], bit 1 target_len outside [0, Lmax], bit 2 an id outside [0, C)
 * With l' the blank-extended target (S = 2 L + 1 states; a target id equal to the blank follows the same recursion, as in torch),
 * p = softmax(logits[t, b, :]) and gamma_t(s) the posterior of state s at time t,
 *   dlogits[t, b, c] = scale * (p[c] - sum over {s : l'_s = c} of gamma_t(s))   for t < input_len[b], 0 for t >= input_len[b].
 * A sample whose nll is not finite (no alignment: zero_infinity) adds nothing to loss and has a zero gradient; so does a sample
 * with status != 0, whose rows and targets are not read beyond what the check itself needs and whose sample_nll is 0.
 * alpha and beta are kept in the log domain in double, so the gradient keeps its relative precision at any T and for logits
 * however peaked.
 * workspace: wd_ctc_workspace_bytes(T, batch, Lmax) bytes (8 * batch * (1 + T * (5 * Lmax + 3)); -1 for sizes outside the range),
 * 8-byte aligned, no initial contents needed.  The function neither allocates nor synchronises (capturable).
 * WD_EINVAL (nothing launched): logits, input_len, target_len, sample_nll, loss, status or workspace NULL; targets NULL or
 * tld < Lmax with Lmax > 0; T outside [1, WD_CTC_MAX_T], C outside [1, WD_CTC_MAX_C], Lmax outside [0, WD_CTC_MAX_L], batch < 1;
 * ld < C, dld < C with dlogits; targets_i64 not 0 or 1; workspace_bytes too small; a pointer not aligned to its element. */
#define WD_CTC_MAX_T 1024
#define WD_CTC_MAX_C 1024
#define WD_CTC_MAX_L 127
int64_t wd_ctc_workspace_bytes(int T, int batch, int Lmax);
int wd_ctc_loss(const float* logits, int ld, int T, int batch, int C, const void* targets, int targets_i64, int tld, int Lmax,
                const int32_t* input_len, const int32_t* target_len, float scale, float* dlogits, int dld, float* sample_nll,
                float* loss, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- backward building blocks (training step, train.py:290: loss.backward()).  Contractions reuse wd_gemm:
 *  d(input)  = wd_gemm over d(output) planes with the mirrored gather table and transposed weights;
 *  d(weight) = wd_gemm over the token dimension, operands = the transposed planes made by wd_transpose_planes. */

/* (weight gradient of nn.Conv2d / nn.Linear, unet.py:595,621,632,540,488,364,375,175-183,125,145,1201-1205,611 under autograd)
 * out[(t*c + ch)][mm] (tap_minor = 0) or out[(ch*ntaps + t)][mm] (tap_minor = 1: the OIHW order of a conv weight)
 *   = in[src(mm, t)][ch] for mm < m (0 beyond, up to mpad): split-bf16 planes [ntaps*c][mpad].
 * in: planes (in_is_f32 = 0; in_lo may be NULL) or one fp32 matrix (in_is_f32 = 1, split on the fly); src = row mm, or
 * through the 3x3 gather table as in wd_gemm (zero row for -1).  mpad >= m and mpad % 4 == 0 (four tokens per store), else
 * WD_EINVAL; gather == NULL requires ntaps == 1.  (The training engine passes a multiple of 64.) */
int wd_transpose_planes(const void* in_hi, const void* in_lo, int in_is_f32, int ld, int c, const int32_t* gather, int ntaps,
                        int hw_out, int hw_src, int m, int mpad, int tap_minor, wd_bf16* out_hi, wd_bf16* out_lo,
                        void* stream);

/* Weight gradient straight from the row-major operand planes - no transposed copies (csrc/wd_dw.hip):
 *   grad[n][ci * ntaps + t] (+)= sum over tokens mm < m of  d[mm][n] * x[src(mm, t)][ci]
 * (the OIHW gradient of nn.Conv2d / nn.Linear under autograd, same layers as wd_transpose_planes above).  d: split-bf16 planes
 * of d(output) [m][d_ld] (wd_dout_prep's row-major planes); x: the layer's input planes [.][x_ld], pointers at the first of the
 * c channels; src = row mm (gather NULL, ntaps 1) or sample * hw_src + gather[t * hw_out + position] (zero row for -1) as in
 * wd_gemm.  The token range is cut into slices run by separate workgroups; their partial tiles go to ws
 * ([nslice][n][ntaps][c] floats) and are combined in fixed order.  Shapes: wd_dw_supported(). */
typedef struct wd_dw_item {   /* one problem of a grouped launch (wd_dw_group): the fields of wd_dw_args that differ between layers */
    const wd_bf16* d_hi;
    const wd_bf16* d_lo;
    const wd_bf16* x_hi;
    const wd_bf16* x_lo;
    float* grad;
    int32_t d_ld, x_ld, grad_ld, accumulate;
} wd_dw_item;
typedef struct wd_dw_args {
    const wd_bf16* d_hi;
    const wd_bf16* d_lo;      /* NULL with npass 1 */
    const wd_bf16* x_hi;
    const wd_bf16* x_lo;      /* NULL with npass 1 */
    const int32_t* gather;    /* [ntaps][hw_out] or NULL */
    float* grad;              /* [n][grad_ld], grad_ld >= c * ntaps */
    float* ws;
    int64_t ws_floats;
    int32_t d_ld, x_ld, grad_ld;
    int32_t ntaps, hw_out, hw_src;
    int32_t m, n, c;
    int32_t npass;            /* 3: hi.hi + hi.lo + lo.hi, 1: hi.hi */
    int32_t accumulate;       /* 1: grad += */
    int32_t nslice;           /* 0: automatic (wd_dw_slices), else <= m / 64 */
    int32_t dbg;              /* 0 in production.  WD_DBG_STAMPS: cycle sums into `stamps` */
    int32_t reserved;
    void* stamps;             /* NULL (debug builds: 16 u64 of cycle sums, see csrc/wd_dw.hip) */
    const wd_dw_item* items;  /* set by wd_dw_group (device memory); callers leave it NULL */
    int32_t nitems;
    int32_t reserved2;
} wd_dw_args;
int wd_dw(const wd_dw_args* a, void* stream);
/* Several layers of the SAME shape (m, n, c, ntaps, hw_out, hw_src, gather, npass as in *a) in one launch: the 1x1 layers of a
 * transformer block have four output tiles each - alone they need 64 token slices of 256 tokens to fill the chip and spend their time
 * in prologue, epilogue and 26 MB of partial tiles; eight of them together run 2048-token slices.  items_host / items_dev: the same
 * nitems (<= 64) records in host memory (checked here) and in device memory (read by the kernel; must stay valid until the launch has
 * run - for a captured graph, as long as the graph).  ws: [nslice][nitems][n][ntaps][c] floats. */
int wd_dw_group(const wd_dw_args* a, const wd_dw_item* items_host, const wd_dw_item* items_dev, int nitems, void* stream);
int wd_dw_group_slices(int m, int n, int c, int ntaps, int nitems);
int wd_dw_item_bytes(void); /* sizeof(wd_dw_item) as this library was built */
int wd_dw_supported(int m, int n, int c, int ntaps, int hw_out); /* m % 64, n % 160, c % 160, hw_out % 64 == 0, hw_out <= 1024 */
int wd_dw_slices(int m, int n, int c, int ntaps);               /* the automatic nslice */
int wd_dw_args_bytes(void); /* sizeof(wd_dw_args) as this library was built */

/* (bias gradients of the layers above; gradient of the FiLM vector emb_out[..., None, None], unet.py:660-661)
 * out[s][col] (+)= scale * sum over rows [s*seg, (s+1)*seg) of x[row][col]; fixed summation order.
 * scratch: ceil(rows/seg) * ceil(seg/128) * c floats (one partial row per 128-row block of a segment); WD_EINVAL when
 * scratch_floats is less.  (bias gradients: seg = rows; FiLM gradient: seg = hw.) */
int wd_colsum(const float* x, int ld, int rows, int c, int seg, float* out, int out_ld, int accumulate, float scale,
              float* scratch, int64_t scratch_floats, void* stream);

/* GroupNorm (+SiLU) backward (unet.py:427-431,594,618 through autograd).  x: the forward input, dz: gradient w.r.t. the
 * normalised(+SiLU) output, columns [dz_off, dz_off + c) of a [B*hw][dz_ld] matrix (channel concat: one call per source);
 * part / nchunk_f / part_cpg: the forward statistics as for wd_gn_apply.
 * pass 1 -> sums[b][chunk][2][c] (chunk < wd_gn_bwd_nchunk(hw)): per-channel sums of dy and dy*xhat; their column sums over
 * (b, chunk) are [d beta | d gamma].  pass 2 -> dx (+= when accumulate). */
int wd_gn_bwd_nchunk(int hw);
int wd_gn_bwd_stats(const float* x, int ld, const float* dz, int dz_ld, int dz_off, int batch, int hw, int c, int cpg,
                    const double* part, int nchunk_f, int part_cpg, const float* gamma, const float* beta, int c_off, float eps,
                    int silu, float* sums, void* stream);
int wd_gn_bwd_apply(const float* x, int ld, const float* dz, int dz_ld, int dz_off, int batch, int hw, int c, int cpg,
                    const double* part, int nchunk_f, int part_cpg, const float* gamma, const float* beta, int c_off, float eps,
                    int silu, const float* sums, float* dx, int dx_ld, int accumulate, void* stream);

/* Both passes in one launch: a workgroup keeps its (sample, 40 channels = whole groups) tile of dy and xhat in LDS, so x and dz are
 * read once.  sums: [b][2][c] (the layout of wd_gn_bwd_stats with one chunk).  Shapes: wd_gn_bwd_fused_supported (40 | c, cpg | 40,
 * the hw x 40 tile pair within LDS: hw <= 448); everything else as wd_gn_bwd_stats / _apply. */
int wd_gn_bwd_fused_supported(int hw, int c, int cpg);
int wd_gn_bwd_fused(const float* x, int ld, const float* dz, int dz_ld, int dz_off, int batch, int hw, int c, int cpg,
                    const double* part, int nchunk_f, int part_cpg, const float* gamma, const float* beta, int c_off, float eps,
                    int silu, float* sums, float* dx, int dx_ld, int accumulate, void* stream);

/* Training dropout (nn.Dropout(p) of ResBlock.out_layers, unet.py:616-623) on the output of a GroupNorm(+SiLU): the mask is a
 * function of (seed, global sample row, layer, position) alone and is never stored - the forward and both backward passes
 * recompute it.  One Philox4x32-10 draw covers four consecutive elements:
 *   counter = (e4, tag, row & 0xffffffff, row >> 32), key = (seed & 0xffffffff, seed >> 32),
 *   idx = token * c + ch (token = y * W + x, ch the channel inside this norm, c its channel count), e4 = idx >> 2, element idx
 *   reads output word idx & 3 and is kept iff word >= thr; row = row_base (+ *row_base_dev) + b;
 *   tag = 0x80000000 | (WD_STREAM_DROPOUT0 + layer); thr = (uint32)(p * 2^32 + 0.5); scale = (float)(1 / (1 - p)).
 * A kept value is one fp32 product v * scale (rounded on its own), a dropped one exactly zero. */
typedef struct {
    uint64_t seed;
    uint64_t row_base;
    const uint64_t* row_base_dev; /* NULL, or added to row_base (read on device) */
    uint32_t tag, thr;
    float scale;
} wd_dropout;
/* Writer-free guidance (classifier-free guidance on the writer; the reference's imgConditioned == 1 branch, unet.py:1578-1579,
 * made per sample): a sample either keeps its label term or runs without it - the term is left out, not multiplied by zero.
 * wd_emb_combine_keep: wd_emb_combine with keep uint8 [B].  Row t*B + b is SiLU(time[t] + label[y_b]) where keep[b] != 0, bit
 * for bit wd_emb_combine's row, and SiLU(time[t]) where keep[b] == 0: bit for bit wd_emb_combine's row on an all-zero label
 * table wherever time holds no exact zero.  keep == NULL: no sample keeps its writer; label and y may then be NULL.
 * wd_label_rows_keep: the writer rows of a batch, out fp32 [B][ted] (16-byte aligned; the residual rows of the time_embed.2 GEMM,
 * as wd_label_mix's): out[b] = label[y_b] bit for bit where sample b keeps its writer, exact zeros where it does not.  The
 * decision is keep_in[b] != 0 (uint8 [B]) when d == NULL.  Otherwise it is drawn: one Philox4x32-10 call with
 *   counter = (0, d->tag, row & 0xffffffff, row >> 32), key = (seed & 0xffffffff, seed >> 32), row = row_base (+ *row_base_dev) + b,
 * kept iff output word 0 >= d->thr; d->scale is ignored.  A training step passes tag = 0x80000000 | WD_STREAM_LABEL_DROP, which
 * no ResBlock mask (0x80000000 | (0x100 + layer)), WD_TAG_KNOWN draw or bare timestep uses.  NULL or: y_eff int64 [B] receives
 * y_b where kept and -1 where dropped (the ids to hand wd_embedding_bwd, which skips ids outside [0, vocab)); keep_out uint8 [B]
 * receives the decision.  y_b is clamped to [0, num_classes) for the read - the host range-checks it.
 * Both: WD_EINVAL (nothing launched) for a NULL required pointer, ted % 4, out_ld % 4 or < ted; they neither allocate nor
 * synchronise (capturable). */
int wd_emb_combine_keep(const float* time, const float* label, const int64_t* y, const uint8_t* keep, int num_classes, int T, int B,
                        int ted, wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, void* stream);
int wd_label_rows_keep(const float* label, const int64_t* y, int num_classes, int B, int ted, const wd_dropout* d,
                       const uint8_t* keep_in, float* out, int64_t* y_eff, uint8_t* keep_out, void* stream);
/* wd_gn_apply with the mask on the normalised(+SiLU) planes (the raw planes carry none). */
int wd_gn_apply_dropout(const float* x, int ld, int batch, int hw, int c, int cpg, const double* part, int nchunk, int part_cpg,
                        const float* gamma, const float* beta, float eps, int silu,
                        wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, int c_off,
                        wd_bf16* raw_hi, wd_bf16* raw_lo, const wd_dropout* d, void* stream);
/* The GroupNorm backward entry points above with dz' = keep ? fp32(dz * scale) : 0 formed as dz is loaded (both passes): bit for
 * bit what they compute from a dz masked beforehand.  WD_EINVAL for d == NULL or c % 4; wd_gn_bwd_fused_supported governs
 * wd_gn_bwd_fused_dropout too. */
int wd_gn_bwd_stats_dropout(const float* x, int ld, const float* dz, int dz_ld, int dz_off, int batch, int hw, int c, int cpg,
                            const double* part, int nchunk_f, int part_cpg, const float* gamma, const float* beta, int c_off, float eps,
                            int silu, float* sums, const wd_dropout* d, void* stream);
int wd_gn_bwd_apply_dropout(const float* x, int ld, const float* dz, int dz_ld, int dz_off, int batch, int hw, int c, int cpg,
                            const double* part, int nchunk_f, int part_cpg, const float* gamma, const float* beta, int c_off, float eps,
                            int silu, const float* sums, float* dx, int dx_ld, int accumulate, const wd_dropout* d, void* stream);
int wd_gn_bwd_fused_dropout(const float* x, int ld, const float* dz, int dz_ld, int dz_off, int batch, int hw, int c, int cpg,
                            const double* part, int nchunk_f, int part_cpg, const float* gamma, const float* beta, int c_off, float eps,
                            int silu, float* sums, float* dx, int dx_ld, int accumulate, const wd_dropout* d, void* stream);

/* LayerNorm backward (nn.LayerNorm of BasicTransformerBlock, unet.py:314-316): dx (+=), and colpart[blk][2][c] (blk < wd_layernorm_bwd_nblk(rows)) whose column sums are
 * [d gamma | d beta]. */
int wd_layernorm_bwd_nblk(int rows);
int wd_layernorm_bwd(const float* x, int ld, const float* dy, int dy_ld, int rows, int c, const float* gamma, float eps,
                     float* dx, int dx_ld, int accumulate, float* colpart, void* stream);

/* softmax-attention backward (CrossAttention.forward unet.py:185-279, Word_Attention :823-836) for nk <= 16 keys: dq[B*nq][lddq]; dkv_part[b][nwg][nk][2][heads*d] = per-workgroup partial
 * sums of (dK, dV) over their tokens (nwg returned; the caller column-sums them). */
/* number of per-workgroup dK/dV partial slabs wd_attention_bwd_small writes per batch element (0 = unsupported shape) */
int wd_attention_bwd_small_nwg(int heads, int nq, int nk, int d);
int wd_attention_bwd_small(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* dout,
                           int ldo, int batch, int heads, int nq, int nk, int d, float scale, float* dq, int lddq,
                           float* dkv_part, int* nwg_out, void* stream);

/* One pass over d(output) [m][n] fp32 (row pitch ld) producing what the layer's backward consumes; each output optional:
 *  pl_*   row-major split planes [m][npad] (columns n..npad-1 zero) - operand of the data-gradient GEMM;
 *  t_*    transposed split planes [n][mpad] (columns m..mpad-1 zero) - operand of the weight-gradient GEMM;
 *  colpart[ceil(mpad/64)][n] column sums of every 64-row block - wd_colsum_finish(colpart, nblk, n, nseg, ...) then sums
 *  nblk consecutive blocks per segment (bias gradient: one segment; FiLM gradient: one segment per sample). */
int wd_dout_prep_rows(void);
int wd_dout_prep(const float* d, int ld, int m, int n, int npad, int mpad, wd_bf16* pl_hi, wd_bf16* pl_lo, wd_bf16* t_hi,
                 wd_bf16* t_lo, float* colpart, void* stream);
/* The same outputs for d(output) of the GEGLU projection (unet.py:125-136 under autograd) WITHOUT materialising it: computed on the
 * fly from the saved pre-activation u = [x | gate] ([m][u_ld]) and the gradient dh [m][dh_ld] of x . gelu(gate); n = npad = 2 inner,
 * inner % 64 == 0.  Replaces wd_geglu_bwd + wd_dout_prep. */
int wd_dout_prep_geglu(const float* u, int u_ld, const float* dh, int dh_ld, int m, int inner, int mpad, wd_bf16* pl_hi, wd_bf16* pl_lo,
                       wd_bf16* t_hi, wd_bf16* t_lo, float* colpart, void* stream);
int wd_colsum_finish(const float* part, int nblk, int c, int nseg, float* out, int out_ld, int accumulate, float scale,
                     void* stream);
/* The same finish for `n` (partials -> gradient) pairs in one launch (nseg = 1 each).  `table` is a device array of
 * wd_colsum_entry records: out[0..c) (+)= scale * sum over k < nblk of part[k * ld + col]; max_c = the widest entry.  Entries of
 * one launch must write distinct `out` ranges.  Used by the training backward for every bias / norm-affine gradient at once
 * (reference: those terms of loss.backward(), train.py:291). */
typedef struct wd_colsum_entry {
    const float* part;
    float* out;
    int32_t nblk, c, ld, accumulate;
    float scale;
    int32_t pad;
} wd_colsum_entry;
int wd_colsum_entry_bytes(void); /* sizeof(wd_colsum_entry) as this library was built */
int wd_colsum_finish_multi(const void* table, int n, int max_c, void* stream);

/* Attention backward (CrossAttention.forward unetPhosc.py:157-198, Word_Attention :696-708) for any number of keys <= 1024
 * (spatial self-attention, the 779-token PHOSC context): recomputes the
 * softmax rows, dq/dk/dv written in place of autograd's (row pitches ldd*; head h owns columns [h*d, (h+1)*d)).
 * scratch: wd_attention_bwd_scratch_floats() floats (P and dS, [batch][heads][nq][nk] each).  Deterministic. */
int64_t wd_attention_bwd_scratch_floats(int batch, int heads, int nq, int nk);
int wd_attention_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* dout, int ldo,
                     int batch, int heads, int nq, int nk, int d, float scale, float* dq, int lddq, float* dk, int lddk,
                     float* dv, int lddv, float* scratch, int64_t scratch_floats, void* stream);

/* dst[i] += src[i] (gradient accumulation where a feature map has several consumers: residual adds, the skip stack
 * of unet.py:1750). 16-byte aligned pointers. */
int wd_add(float* dst, const float* src, int64_t n, void* stream);

/* packed weight gradient [n][tap*c + ch] (row pitch ld >= ntaps*c) -> the parameter's OIHW order [n][ch][tap]. */
int wd_permute_dw(const float* packed, int ld, int n, int c, int ntaps, float* out, void* stream);

/* GEGLU (unet.py:122-135) unfused (training keeps the pre-activation u = [a | g]): h = a * gelu_erf(g) -> planes; du from dh. */
int wd_geglu_fwd(const float* u, int ld, int64_t rows, int inner, wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, void* stream);
int wd_geglu_bwd(const float* u, int ld, const float* dh, int dh_ld, int64_t rows, int inner, float* du, int du_ld,
                 void* stream);
/* nn.SiLU backward (time_embed / emb_layers, unet.py:1201-1205,609): dpre = dact * silu'(pre) */
int wd_silu_bwd(const float* pre, const float* dact, int64_t n, float* dpre, void* stream);
/* backward of F.interpolate(scale_factor=2, mode="nearest") (Upsample.forward, unet.py:497): in [B][2h][2w][c] -> out [B][h][w][c], 2x2 block sums */
int wd_pool2x2_sum(const float* in, int batch, int h, int w, int c, float* out, void* stream);
/* nn.Embedding backward (CharacterEncoder.embedding unet.py:845, label_emb :1245): dtable[v][:] (+)= sum of d[r][:] over rows with ids[r] == v (deterministic);
 * a row whose id lies outside [0, vocab) contributes to no table row: ids of -1 mask rows out (wd_label_rows_keep's y_eff) */
int wd_embedding_bwd(const void* ids, int ids_are_i64, int rows, const float* d, int ld, int vocab, int c, float* dtable,
                     int accumulate, void* stream);

/* ---- The PHOSCnet word recogniser (ResPhoSCNetZSL/modules/models.py:15-80): the streaming stages between its GEMMs
 * (csrc/wd_phoscnet.hip).  The network's nn.ReLU never enters a GEMM epilogue: it lives in the stage that turns one GEMM's fp32
 * result into the next GEMM's split-bf16 operand.  Every stage is a grid-stride loop under the grid cap of the edge kernels
 * (2048 workgroups of 256), launches nothing on WD_EINVAL, calls nothing but the launch (capturable), and takes the 16-byte load /
 * 8-byte plane store path when every pitch is a multiple of 4 elements and every pointer on its 16-byte (fp32) / 8-byte (planes)
 * grid, the element path otherwise - the same values either way. */

/* nn.ReLU (+ nn.MaxPool2d((2, 2), stride 2) when pool == 2; models.py:21-29) of a token-major fp32 map x [batch*h*w][ld_in] with c
 * channels -> split-bf16 planes out [batch*h'*w'][ld_out]: pool 1 keeps h' = h, w' = w; pool 2 has h' = h / 2, w' = w / 2 (floor: a
 * last odd row or column is dropped; h, w >= 2).  Value: m = x (pool 1) or the largest of the four, then v = m > 0 ? m : +0; hi =
 * bf16(v) (round to nearest even), lo = bf16(v - hi) - wd_split's planes bit for bit.  out_lo may be NULL.  Rows of an MLP
 * ([batch][c], nn.Linear + nn.ReLU, models.py:53-58) are h = w = 1. */
int wd_relu_pool_planes(const float* x, int ld_in, int batch, int h, int w, int c, int pool, wd_bf16* out_hi, wd_bf16* out_lo,
                        int ld_out, void* stream);

/* nn.ReLU, then TemporalPyramidPooling(levels) (pyramidpooling.py:88-113, mode "max") of the token-major fp32 map x [batch*h*w][ld]
 * with c channels.  Level L: k = ceil(w / L) columns per bin, pad = k * L - w zero columns of which floor(pad / 2) go on the left;
 * bin j is the maximum of max(x, 0) over all h rows and the padded columns [j * k, (j + 1) * k) (a bin of padding only is 0; a
 * zero column never wins against a ReLU output, so padding only matters there).  Output column of (level i, channel ch, bin j):
 * sum_{i' < i} c * levels[i'] + ch * levels[i] + j - the reference's x.view(num_sample, -1) of an NCHW tensor.  Writes the fp32
 * row out_f32 [batch][ld_out] (may be NULL) and its split planes out_hi / out_lo [batch][ld_pl] (out_hi may be NULL when out_f32 is
 * not; out_lo may be NULL).  levels: nlevels <= WD_TPP_MAX_LEVELS ints on the HOST, each in [1, WD_TPP_MAX_BINS], read before the
 * launch. */
#define WD_TPP_MAX_LEVELS 8
#define WD_TPP_MAX_BINS 16
int wd_tpp_max(const float* x, int ld, int batch, int h, int w, int c, const int32_t* levels, int nlevels, float* out_f32,
               int ld_out, wd_bf16* out_hi, wd_bf16* out_lo, int ld_pl, void* stream);

/* Bilinear resize with half-pixel centres, no antialias: cv2.resize(..., INTER_LINEAR) of the recogniser's inputs
 * (ResPhoSCNetZSL/modules/datasets.py:91) and F.interpolate(mode="bilinear", align_corners=False).  x: batch * c planes of hs rows of
 * pitch ld_in (ws values each); out: batch * c planes of h rows of pitch ld_out (w values each).  bgr != 0: output plane ch of a
 * sample reads source plane c - 1 - ch.  Every operation below is rounded to fp32 on its own (no contraction), in this order:
 *   the source coordinate (y + 0.5) * hs / h - 0.5, clamped at 0, in integers: n = max((2 y + 1) * hs - h, 0); y0 = n / (2 h);
 *   y1 = min(y0 + 1, hs - 1);  ly = (float)(n - y0 * 2 h) / (float)(2 h) - one division of two exact values (a coordinate formed
 *   in fp32 is off by 1.5e-5 of a pixel at the far edge of a 256-pixel image);  the same for x (x0, x1, lx)
 *   top = (1 - lx) * s[y0][x0] + lx * s[y0][x1];  bot = (1 - lx) * s[y1][x0] + lx * s[y1][x1];  out = (1 - ly) * top + ly * bot
 * (same size: ly = lx = 0 and out = s[y][x]). */
int wd_resize_bilinear(const float* x, int ld_in, int batch, int c, int hs, int ws, float* out, int ld_out, int h, int w, int bgr,
                       void* stream);

/* The two heads' activations (models.py:60-61, :72-73) into one PHOSC row: out[b][j] = max(phos[b][j], 0) for j < n_phos (as
 * wd_relu_pool_planes: x > 0 ? x : +0), out[b][n_phos + j] = 1 / (1 + exp(-phoc[b][j])) for j < n_phoc (expf and an IEEE division:
 * within 1e-6 of the exact sigmoid).  phos [batch][ld_phos], phoc [batch][ld_phoc] may be the first columns of zero-padded GEMM
 * outputs; out [batch][ld_out], ld_out >= n_phos + n_phoc. */
int wd_phosc_finish(const float* phos, int ld_phos, int n_phos, const float* phoc, int ld_phoc, int n_phoc, int batch, float* out,
                    int ld_out, void* stream);

/* Zero-shot recognition (ResPhoSCNetZSL/modules/engine.py:130-146): the cosine of every prediction pred [batch][ld_pred] (d values)
 * against every row of table [v][ld_table]: cos = dot / max(|x| * |y|, 1e-8) in fp32, |y| = table_norm[word] (fp32 [v], from the
 * host in fp64 or any other source), |x| summed by the launch.  One workgroup per (sample, block of 64 words), one wave per word.
 * Outputs, each optional: scores [batch][ld_scores]; best_idx [batch] int32 and best_score [batch]: the FIRST maximum (the
 * reference's strict > over its iteration order); target_score [batch] = the score of word target_idx[b] (int32; NaN for an id
 * outside [0, v); target_idx is required with it).  ws: [batch][v] floats, needed only when scores is NULL and one of the other
 * outputs is asked for (WD_EINVAL without it); asking for nothing is WD_EINVAL.  The best / target outputs are a second launch
 * over the scores (one workgroup per sample). */
int wd_phosc_score(const float* pred, int ld_pred, int batch, int d, const float* table, int ld_table, const float* table_norm, int v,
                   float* scores, int ld_scores, int32_t* best_idx, float* best_score, const int32_t* target_idx, float* target_score,
                   float* ws, void* stream);

/* hipGraph capture of a launch sequence (one denoising step) on `stream`. */
int wd_graph_begin(void* stream);
int wd_graph_end(void* stream, void** graph_exec_out);
int wd_graph_launch(void* graph_exec, void* stream);
int wd_graph_destroy(void* graph_exec);

/* per-kernel-class timing with hipEvents recorded on the launch stream (bench.py roofline leg).
 * classes: 0 gemm (the LDS-staged wd_gemm2_kernel<128,160,...>), 1 gn_stats, 2 gn_apply, 3 layernorm, 4 attention, 5 other,
 * 6 gemm with other tile shapes, 7 split-K combine pass, 8 the two-workgroups-per-CU gemm kernel (wd_gemm4_kernel),
 * 9 the weights-to-registers gemm (wd_gemmw_kernel, 64 x 320 / 128 x 160 tiles), 10 the fused feed-forward (wd_ff_kernel),
 * 11 the weight-gradient kernel (wd_dw_kernel), 12 the whole-K kernel of the small maps (wd_gemmq_kernel).
 * wd_prof_collect: gemm_flops = the 2*M*N*K of class 0; wd_prof_collect_flops additionally returns the algorithmic FLOPs
 * (each multiply-add counted once) of every class that declares them (the contraction classes 0, 6, 8, 9, 10, 11, 12). */
#define WD_NCLASS 13
int wd_prof_enable(int on);
int wd_prof_collect(double* ms_per_class, int64_t* launches_per_class, double* gemm_flops); /* syncs */
int wd_prof_collect_flops(double* ms_per_class, int64_t* launches_per_class, double* flops_per_class); /* syncs */

const char* wd_version(void);
int wd_device_info(int* cu_count, int* lds_per_block, char* name, int name_len);

#ifdef __cplusplus
}
#endif
#endif
