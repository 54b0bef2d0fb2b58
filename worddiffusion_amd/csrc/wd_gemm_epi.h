// Epilogue shared by every tap-gather GEMM kernel of libwdiff_hip.so (wd_gemm.hip, wd_gemm4.hip, wd_gemmw.hip, wd_gemmq.hip, wd_gemm_reduce.hip,
// wd_gemm_exp.hip) and by wd_ff.hip: the fp32 LDS image of an
// output tile -> bias / FiLM row vector / residual / activation / operand planes / fused GroupNorm statistics, or the split-K
// partial store.  Replaces the elementwise tails of reference unet.py:660-669 (FiLM add, residual) and :128-136 (GEGLU).
#pragma once
#include "wd_common.h"
#include "wd_gemm_priv.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace {

// ---- epilogue shared by all kernels.  The accumulators of all waves go through an fp32 LDS image of the output
// tile (which also sums the two k-halves of the 8-wave variants); wd_epilogue_from_image then reads float4s row-major
// and does bias / FiLM / residual / activation with 16-byte global loads and stores, and - when the consumer is a
// GroupNorm - reduces per-(sample, group) sum / sum of squares of the finished values in a fixed order, so that the
// statistics pass over the feature map (wd_gn_stats) disappears.
constexpr int WD_STAT_SCRATCH = 40 * 1024;  // LDS behind the epilogue image for the per-thread column sums
constexpr int WD_STAT_MAXNS = 2;          // samples per 128-row panel the fused statistics support (hw_out >= 64)

// Does the epilogue take its 16-byte path for these args: every epilogue pitch a multiple of 4 elements, the fp32 operands on the
// 16-byte grid and the output planes on the 8-byte grid.  The one statement of that rule: the epilogue itself, the combine
// launch and the host checks (wd_gemm_resolve: statistics, gn_*, tickets need this path) all ask here.
__host__ __device__ __forceinline__ bool wd_epilogue_vec_ok(const wd_gemm_args& a) {
    return (((a.out_ld | a.rowvec_ld | a.resid_ld | a.out_pl_ld) & 3) == 0) &&
           (((reinterpret_cast<uintptr_t>(a.bias) | reinterpret_cast<uintptr_t>(a.rowvec) |
              reinterpret_cast<uintptr_t>(a.resid) | reinterpret_cast<uintptr_t>(a.out_f32)) & 15) == 0) &&
           (((reinterpret_cast<uintptr_t>(a.out_hi) | reinterpret_cast<uintptr_t>(a.out_lo)) & 7) == 0);
}

// Does a launch of bm x bn tiles (bm = 64) over these RESOLVED args take the batched epilogue (wd_epilogue_rows below) instead of the
// row loop of wd_epilogue_from_image.  Two parts.  The launch's SHAPE (wd_epilogue_batch_shape): the epilogue inside the GEMM launch
// (no K cut), no activation or SiLU, the result stored as it is (no row LayerNorm, no GroupNorm of the result), planes sources (no
// a32), the residual row of m is row m, every tile whole (m and n multiples of the tile) and inside one sample (no second sample's
// statistics to park), and pitches small enough that a tile's byte offsets from its first element fit 31 bits - wd_gemm_resolve /
// wd_ff_fused set WD_EPI_BATCH_BIT by it: the bit names the form of the launch's 16-byte path.  And the 16-byte path itself
// (wd_epilogue_vec_ok), which depends on the pitches and addresses of a call as it always did: a launch off it runs the element loop
// under either form.  wd_epilogue_batch_ok is both, the one statement of the rule: the kernels ask it before they branch.
constexpr int WD_EPI_BATCH_MAX_LD = 1 << 22;
__host__ __device__ __forceinline__ bool wd_epilogue_batch_shape(const wd_gemm_args& a, const int bm, const int bn) {
    const bool pitches = (!a.out_f32 || a.out_ld < WD_EPI_BATCH_MAX_LD) && (!a.out_hi || a.out_pl_ld < WD_EPI_BATCH_MAX_LD) &&
                         (!a.resid || a.resid_ld < WD_EPI_BATCH_MAX_LD);
    return a.ksplit <= 1 && (a.act == WD_ACT_NONE || a.act == WD_ACT_SILU) && !a.ln_gamma && !a.gn_gamma && !a.a32 && !a.resid_rows &&
           a.m % bm == 0 && a.n % bn == 0 && a.hw_out % bm == 0 && pitches;
}
__host__ __device__ __forceinline__ bool wd_epilogue_batch_ok(const wd_gemm_args& a, const int bm, const int bn) {
    return wd_epilogue_vec_ok(a) && wd_epilogue_batch_shape(a, bm, bn);
}

// Fused GroupNorm statistics, the accuracy rule: a producer's (sum, sum of squares) partials leave var = sumsq / n - mean^2,
// formed in double by the consumers, accurate to ~1e-7 of the variance however far the group's mean is from zero.  (Plain fp32
// sums anywhere are off by 2^-24 of the sum of squares, which that difference multiplies by (mean / std)^2: 2.4e-4 at 64.)
// A thread's rows, the only stage with one step per row, stay in fp32 but are summed as d = v - pivot, the pivot being the first
// value the thread saw in that column of that sample: d is exact for values within a factor two of the pivot (Sterbenz) and of
// the size of the spread, not of the mean, so the fp32 roundings of sum(d) and sum(d^2) are relative to the spread.  wd_stat_finish
// turns them into the plain sums in double (n p + S, n p^2 + 2 p S + Q); every later stage - the LDS hand-over, the sums over a
// group's columns and over the row lanes - is in double.
struct WdStatAcc {
    float4 p, s, q;  // pivot, sum (v - p), sum (v - p)^2
    int n;           // rows summed
};
__device__ __forceinline__ void wd_stat_reset(WdStatAcc& t) {
    t.p = t.s = t.q = make_float4(0.f, 0.f, 0.f, 0.f);
    t.n = 0;
}
__device__ __forceinline__ void wd_stat_add(WdStatAcc& t, const float4& v) {
    if (t.n == 0) t.p = v;
    const float4 d = make_float4(v.x - t.p.x, v.y - t.p.y, v.z - t.p.z, v.w - t.p.w);
    t.s.x += d.x; t.s.y += d.y; t.s.z += d.z; t.s.w += d.w;
    t.q.x += d.x * d.x; t.q.y += d.y * d.y; t.q.z += d.z * d.z; t.q.w += d.w * d.w;
    ++t.n;
}
__device__ __forceinline__ void wd_stat_finish(const WdStatAcc& t, double (&su)[4], double (&sq)[4]) {
    const float p[4] = {t.p.x, t.p.y, t.p.z, t.p.w}, s[4] = {t.s.x, t.s.y, t.s.z, t.s.w}, q[4] = {t.q.x, t.q.y, t.q.z, t.q.w};
    const double n = (double)t.n;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double pj = (double)p[j], sj = (double)s[j];
        su[j] = n * pj + sj;
        sq[j] = n * pj * pj + 2.0 * pj * sj + (double)q[j];
    }
}

// scr[sample][row lane][bn]: (sample, group, row lane) -> the sum over the group's columns, written over the group's first column
template <int NT>
__device__ __forceinline__ void wd_stat_reduce(double* scr, const int ns, const int nrl, const int ngt, const int bn, const int cpg,
                                               const int tid) {
    for (int it = tid; it < ns * ngt * nrl; it += NT) {
        const int l = it % nrl, g = (it / nrl) % ngt, sidx2 = it / (nrl * ngt);
        double* p = scr + (long)(sidx2 * nrl + l) * bn + g * cpg;
        double su = 0.0;
        for (int cc = 0; cc < cpg; ++cc) su += p[cc];
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): every read of this group's span precedes the write-back
        p[0] = su;
    }
}

// The hand-over both epilogue forms end in: `st` holds a thread's column sums of the last sample of the panel (a thread that
// crossed into sample 1 left sample 0's state in `park`), nrl / rl / c / rps are the caller's row-lane geometry.
template <int BM, int BN, int NT>
__device__ __forceinline__ void wd_stat_handover(const wd_gemm_args& a, float* ep, const int m0, const int n0, const int tid,
                                                 const WdStatAcc& st, const int cur_s, const float* park, const int nrl, const int rl,
                                                 const int c, const int rps) {
    constexpr int LDE = BN + 4;
    // ---- GroupNorm partial statistics of the finished tile: (sample in panel, group) = fixed-order sum over the group's
    // columns, then over the row lanes, of the per-thread column sums (host guarantees the vector path, BN % cpg == 0,
    // n % cpg == 0, and that BM and hw_out divide one another).  Everything stays in double: the scratch behind the image
    // holds [quantity][sample][row lane][BN] doubles - the sums and the sums of squares together where that fits (one
    // sample per panel, or 256 threads), else the sums go through it first and the sums of squares second.
    const int ns = BM > a.hw_out ? BM / a.hw_out : 1;
    double ssum[4] = {0.0, 0.0, 0.0, 0.0}, ssq[4] = {0.0, 0.0, 0.0, 0.0};  // the last sample of the panel
    double s0[4] = {0.0, 0.0, 0.0, 0.0}, q0[4] = {0.0, 0.0, 0.0, 0.0};      // sample 0 of two
    if (cur_s == 0 && ns > 1) {
        wd_stat_finish(st, s0, q0);  // this thread never reached sample 1: its running sums are sample 0's
    } else {
        wd_stat_finish(st, ssum, ssq);
        if (cur_s != 0) {  // (only with ns > 1, and then rl < nrl && c < BN: the parked slots are inside the scratch)
            WdStatAcc pv;
            pv.p = *reinterpret_cast<const float4*>(park);
            pv.s = *reinterpret_cast<const float4*>(park + 4);
            pv.q = *reinterpret_cast<const float4*>(park + 2 * nrl * BN);
            pv.n = __float_as_int(park[2 * nrl * BN + 4]);
            wd_stat_finish(pv, s0, q0);
        }
    }
    const int cpg = a.stat_cpg;
    const int ngt = BN / cpg;
    const int nchunk = a.hw_out > BM ? a.hw_out / BM : 1;
    const int ngs = a.n / cpg;  // groups per sample in the statistics array of this tensor
    double* scr = reinterpret_cast<double*>(ep + BM * LDE);  // (BM * LDE * 4 is a multiple of 16)
    const int nq = 2 * ns * nrl * BN * (int)sizeof(double) <= WD_STAT_SCRATCH ? 2 : 1;  // quantities per pass
    for (int q0i = 0; q0i < 2; q0i += nq) {
        if (q0i) __syncthreads();
        if (rl < nrl && c < BN) {
            for (int qq = 0; qq < nq; ++qq) {
                const bool sq = q0i + qq;
                const double* lo = ns > 1 ? (sq ? q0 : s0) : (sq ? ssq : ssum);
                double* o = scr + ((long)(qq * ns) * nrl + rl) * BN + c;
                *reinterpret_cast<double2*>(o) = make_double2(lo[0], lo[1]);
                *reinterpret_cast<double2*>(o + 2) = make_double2(lo[2], lo[3]);
                if (ns > 1) {
                    const double* hi = sq ? ssq : ssum;
                    o += nrl * BN;
                    *reinterpret_cast<double2*>(o) = make_double2(hi[0], hi[1]);
                    *reinterpret_cast<double2*>(o + 2) = make_double2(hi[2], hi[3]);
                }
            }
        }
        __syncthreads();
        wd_stat_reduce<NT>(scr, nq * ns, nrl, ngt, BN, cpg, tid);
        __syncthreads();
        // (quantity, sample, group) -> sum over the row lanes in fixed order
        for (int it = tid; it < nq * ns * ngt; it += NT) {
            const int g = it % ngt, qs = it / ngt, sidx2 = qs % ns, qq = qs / ns;
            const int mrow = m0 + sidx2 * rps;
            if (mrow >= a.m || n0 + g * cpg >= a.n) continue;
            double su = 0.0;
            for (int l = 0; l < nrl; ++l) su += scr[(long)(qs * nrl + l) * BN + g * cpg];
            const int b = mrow / a.hw_out;
            const int chunk = (mrow - b * a.hw_out) / BM;
            a.stat_part[(((long)b * nchunk + chunk) * ngs + n0 / cpg + g) * 2 + q0i + qq] = su;
        }
    }
}

// WS: the tile's values are not in the LDS image but still spread over the split-K slabs of a.ws - the combine pass sums them
// here, row by row in the thread's own (row lane, column quad) pattern, instead of staging the sums through LDS first (the
// statistics scratch behind the image position is used as usual).  Vector path only; the caller checks.
template <int BM, int BN, int NT, bool WS = false>
__device__ __forceinline__ void wd_epilogue_from_image(const wd_gemm_args& a, float* ep, const int m0, const int n0,
                                                       const int tid, const int nslab = 1) {
    constexpr int LDE = BN + 4;  // row pitch in floats (16-byte aligned rows, bank-shifted)
    const bool geglu = a.act == WD_ACT_GEGLU;
    const int ocols = geglu ? BN / 2 : BN;  // output columns of this tile
    const int oc4 = ocols / 4;
    const int nout = geglu ? a.n / 2 : a.n;
    const int no0 = geglu ? n0 / 2 : n0;
    const bool stats = a.stat_part != nullptr;
    // 16-byte path needs aligned rows everywhere; otherwise (odd leading dimensions) one element at a time
    const bool vec = wd_epilogue_vec_ok(a);
    if (!vec) {
        for (int i = tid; i < BM * ocols; i += NT) {
            const int row = i / ocols, c = i - row * ocols;
            const int m = m0 + row, no = no0 + c;
            if (m >= a.m || no >= nout) continue;
            float v;
            if (geglu) {
                const float x = ep[row * LDE + c] + (a.bias ? a.bias[n0 + c] : 0.f);
                const float g = ep[row * LDE + c + BN / 2] + (a.bias ? a.bias[n0 + c + BN / 2] : 0.f);
                v = x * wd_gelu_erf(g);
            } else {
                v = ep[row * LDE + c] + (a.bias ? a.bias[no] : 0.f);
            }
            if (a.rowvec) v += a.rowvec[(long)(m / a.hw_out) * a.rowvec_ld + no];
            if (a.resid) v += a.resid[(a.resid_rows ? (long)a.resid_rows[m] : (long)m) * a.resid_ld + no];
            if (a.act == WD_ACT_SILU) v = wd_silu(v);
            if (stats || a.ln_gamma) ep[row * LDE + c] = v;
            if (a.out_f32) a.out_f32[(long)m * a.out_ld + no] = v;
            if (a.out_hi && !a.ln_gamma) {
                uint32_t hb, lb;
                wd_split1(v, hb, lb);
                a.out_hi[(long)m * a.out_pl_ld + no] = (wd_bf16)hb;
                if (a.out_lo) a.out_lo[(long)m * a.out_pl_ld + no] = (wd_bf16)lb;
            }
        }
    } else {
        // thread -> (row lane, fixed column quad): coalesced rows, and per-thread column sums for the statistics
        const int nrl = NT / oc4;                 // row lanes
        const int rl = tid / oc4, c = (tid - rl * oc4) * 4;
        const int no = no0 + c;
        const int rps = BM > a.hw_out ? a.hw_out : BM;  // rows of one sample inside this panel
        // (with statistics rps is BM or a divisor of it - a power of two - so row / rps is a shift; the FiLM row of m needs m /
        // hw_out: a shift too for power-of-two images, a division otherwise.  A run-time integer division is ~25 instructions,
        // more than the rest of a row's work.)
        const int rps_sh = 31 - __clz(rps);
        const int hw_sh = (a.hw_out & (a.hw_out - 1)) == 0 ? 31 - __clz(a.hw_out) : -1;
        // statistics: a thread's column sums and sums of squares (WdStatAcc) of the sample it is in.  WD_STAT_MAXNS == 2 and rows
        // ascend, so `cur_s` only ever steps from 0 to 1: the finished sample's fp32 state is then parked in this thread's own two
        // slots of the scratch (32 bytes each, read and written by no other thread before the barrier below) - nothing but `st`
        // stays live across the row loop, whose loads in flight need the registers.
        WdStatAcc st;
        wd_stat_reset(st);
        float* park = ep + BM * LDE + 2 * ((long)rl * BN + c);  // slot of sample 0; sample 1's is 2 * nrl * BN floats on
        int cur_s = 0;
        if (rl < nrl && no < nout) {
            float4 bx = make_float4(0, 0, 0, 0), bg = bx;
            if (a.bias) {
                bx = *reinterpret_cast<const float4*>(a.bias + (geglu ? n0 + c : no));
                if (geglu) bg = *reinterpret_cast<const float4*>(a.bias + n0 + c + BN / 2);
            }
            for (int row = rl; row < BM; row += nrl) {
                const int m = m0 + row;
                if (m >= a.m) break;
                float4 v;
                if constexpr (WS) {
                    const float* p = a.ws + (long)m * a.n + n0 + c;
                    const long total = (long)a.m * a.n;
                    v = *reinterpret_cast<const float4*>(p);
                    for (int sp = 1; sp < nslab; ++sp) {
                        const float4 q = *reinterpret_cast<const float4*>(p + (long)sp * total);
                        v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
                    }
                } else {
                    v = *reinterpret_cast<const float4*>(ep + row * LDE + c);
                }
                if (geglu) {  // columns [0, BN/2) of the tile are x, [BN/2, BN) their gates (weights packed that way)
                    const float4 g = *reinterpret_cast<const float4*>(ep + row * LDE + c + BN / 2);
                    const wd_f32x2 h01 = (wd_f32x2{v.x, v.y} + wd_f32x2{bx.x, bx.y}) * wd_gelu_erf2(wd_f32x2{g.x, g.y} + wd_f32x2{bg.x, bg.y});
                    const wd_f32x2 h23 = (wd_f32x2{v.z, v.w} + wd_f32x2{bx.z, bx.w}) * wd_gelu_erf2(wd_f32x2{g.z, g.w} + wd_f32x2{bg.z, bg.w});
                    v = make_float4(h01.x, h01.y, h23.x, h23.y);
                } else {
                    v.x += bx.x; v.y += bx.y; v.z += bx.z; v.w += bx.w;
                }
                if (a.rowvec) {
                    const int bi = hw_sh >= 0 ? m >> hw_sh : m / a.hw_out;
                    const float4 q = *reinterpret_cast<const float4*>(a.rowvec + (long)bi * a.rowvec_ld + no);
                    v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
                }
                if (a.resid) {
                    const long rr = a.resid_rows ? (long)a.resid_rows[m] : (long)m;
                    const float4 q = *reinterpret_cast<const float4*>(a.resid + rr * a.resid_ld + no);
                    v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
                }
                if (a.act == WD_ACT_SILU) {
                    v.x = wd_silu(v.x); v.y = wd_silu(v.y); v.z = wd_silu(v.z); v.w = wd_silu(v.w);
                }
                if (stats) {
                    const int sidx2 = row >> rps_sh;
                    if (sidx2 != cur_s) {  // rows ascend: set the finished sample's column sums aside
                        *reinterpret_cast<float4*>(park) = st.p;
                        *reinterpret_cast<float4*>(park + 4) = st.s;
                        *reinterpret_cast<float4*>(park + 2 * nrl * BN) = st.q;
                        park[2 * nrl * BN + 4] = __int_as_float(st.n);
                        wd_stat_reset(st);
                        cur_s = sidx2;
                    }
                    wd_stat_add(st, v);
                }
                if (a.ln_gamma) {  // the row LayerNorm below reads the finished values back from the image
                    if constexpr (!WS) *reinterpret_cast<float4*>(ep + row * LDE + c) = v;
                }
                if (no + 3 < nout) {
                    if (a.out_f32) *reinterpret_cast<float4*>(a.out_f32 + (long)m * a.out_ld + no) = v;
                    if (a.out_hi && !a.ln_gamma) {
                        uint2 hh, ll;
                        wd_split4(v, hh, ll);
                        *reinterpret_cast<uint2*>(a.out_hi + (long)m * a.out_pl_ld + no) = hh;
                        if (a.out_lo) *reinterpret_cast<uint2*>(a.out_lo + (long)m * a.out_pl_ld + no) = ll;
                    }
                } else {  // ragged right edge (n not a multiple of 4 columns inside this float4)
                    const float e[4] = {v.x, v.y, v.z, v.w};
                    for (int j = 0; j < 4 && no + j < nout; ++j) {
                        if (a.out_f32) a.out_f32[(long)m * a.out_ld + no + j] = e[j];
                        if (a.out_hi) {
                            uint32_t hb, lb;
                            wd_split1(e[j], hb, lb);
                            a.out_hi[(long)m * a.out_pl_ld + no + j] = (wd_bf16)hb;
                            if (a.out_lo) a.out_lo[(long)m * a.out_pl_ld + no + j] = (wd_bf16)lb;
                        }
                    }
                }
            }
        }
        if (stats) wd_stat_handover<BM, BN, NT>(a, ep, m0, n0, tid, st, cur_s, park, nrl, rl, c, rps);
    }
    if (a.ln_gamma) {
        // ---- LayerNorm of every finished row -> the operand planes of the next GEMM (nn.LayerNorm of the transformer block that
        // consumes this tensor, unetPhosc.py:241-246): the tile holds whole rows (BN == n, the host checked), one wave per row,
        // two-pass statistics in registers as wd_layernorm does.  Saves the wd_layernorm launch and its pass over the tensor.
        __syncthreads();
        constexpr int NW = NT / 64;
        const int lane = tid & 63, wv = tid >> 6;
        const bool has0 = lane * 4 < BN, has1 = (64 + lane) * 4 < BN;
        // (a lane's columns are the same for every row: the affine vectors are loaded once, not once per row)
        float4 gq[2], bq[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            gq[h] = bq[h] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (h ? has1 : has0) {
                gq[h] = *reinterpret_cast<const float4*>(a.ln_gamma + (h * 64 + lane) * 4);
                bq[h] = *reinterpret_cast<const float4*>(a.ln_beta + (h * 64 + lane) * 4);
            }
        }
        for (int row = wv; row < BM; row += NW) {
            const int m = m0 + row;
            if (m >= a.m) break;
            const float* rp = ep + row * LDE;
            float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;
            if (has0) x0 = *reinterpret_cast<const float4*>(rp + lane * 4);
            if (has1) x1 = *reinterpret_cast<const float4*>(rp + (64 + lane) * 4);
            const float mean = wd_wave_sum((x0.x + x0.y) + (x0.z + x0.w) + (x1.x + x1.y) + (x1.z + x1.w)) * (1.0f / BN);
            float d = 0.f;
            if (has0) d += (x0.x - mean) * (x0.x - mean) + (x0.y - mean) * (x0.y - mean) + (x0.z - mean) * (x0.z - mean) + (x0.w - mean) * (x0.w - mean);
            if (has1) d += (x1.x - mean) * (x1.x - mean) + (x1.y - mean) * (x1.y - mean) + (x1.z - mean) * (x1.z - mean) + (x1.w - mean) * (x1.w - mean);
            const float rstd = rsqrtf(wd_wave_sum(d) * (1.0f / BN) + a.ln_eps);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (!(h ? has1 : has0)) continue;
                const int c = (h * 64 + lane) * 4;
                const float4 x = h ? x1 : x0;
                const float4 g = gq[h], b = bq[h];
                float4 y;
                y.x = (x.x - mean) * rstd * g.x + b.x; y.y = (x.y - mean) * rstd * g.y + b.y;
                y.z = (x.z - mean) * rstd * g.z + b.z; y.w = (x.w - mean) * rstd * g.w + b.w;
                uint2 hh, ll;
                wd_split4(y, hh, ll);
                *reinterpret_cast<uint2*>(a.out_hi + (long)m * a.out_pl_ld + c) = hh;
                if (a.out_lo) *reinterpret_cast<uint2*>(a.out_lo + (long)m * a.out_pl_ld + c) = ll;
            }
        }
    }
}

// The batched form of the 16-byte path for launches wd_epilogue_batch_ok accepts: the values and the order of the row loop above
// (+ bias, + FiLM row, + residual, SiLU?, the column sums), so the bits of every output are the loop's, but a thread's rows
// rl, rl + NRL, ... are unrolled and go through memory together:
//   (a) every image quad from LDS, the bias and FiLM quads (one sample per tile: one row vector) and every residual row are requested;
//   (b) ONE wait for all of them;
//   (c) the rows in ascending order: arithmetic, then the row's stores - no load and no wait between the first and the last store.
// In the loop every row paid a round trip of its own: vmcnt counts stores as well as loads, and the wait in front of a row's residual
// load also drained the stores of the row before it.
// The run-time flags (bias, rowvec, resid, out_f32, out_hi, out_lo) wrap no memory operation in a branch - hipcc's wait-count pass
// would put the waits back.  Every operand is a buffer descriptor over the tile's own window (based at the
// tile's first element, as long as its last row's last column), of ZERO bytes when the operand is absent: such a load returns
// zeros (added only under the flag, or + 0.0f as the loop adds an absent bias) and such a store is dropped, as are those of a
// thread's rows past the tile (offset WD_EPI_OOB).  The same bounds check keeps a wrong offset from leaving the window.
typedef __attribute__((ext_vector_type(4))) unsigned wd_u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned wd_u32x2;
constexpr uint32_t WD_EPI_OOB = 0x80000000u;

template <int BM, int BN, int NT>
__device__ __forceinline__ void wd_epilogue_rows(const wd_gemm_args& a, float* ep, const int m0, const int n0, const int tid) {
    constexpr int LDE = BN + 4, Q = BN / 4, NRL = NT / Q, KEEP = (BM + NRL - 1) / NRL;
    const int rl = tid / Q, c = (tid - rl * Q) * 4;
    const bool live = rl < NRL;
    const bool planes = a.out_hi != nullptr;
    // a window of BM rows of pitch ld, BN columns of esz bytes, from (m0 + row0, n0) of p
    auto window = [&](const void* p, const long row0, const int ld, const int rows, const int esz) {
        const char* base = reinterpret_cast<const char*>(p) + (row0 * ld + n0) * esz;
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), 0, p ? ((rows - 1) * ld + BN) * esz : 0, 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t s_bias = window(a.bias, 0, 0, 1, 4);
    const __amdgpu_buffer_rsrc_t s_rv = window(a.rowvec, a.rowvec ? m0 / a.hw_out : 0, a.rowvec_ld, 1, 4);
    const __amdgpu_buffer_rsrc_t s_res = window(a.resid, m0, a.resid_ld, BM, 4);
    const __amdgpu_buffer_rsrc_t s_f32 = window(a.out_f32, m0, a.out_ld, BM, 4);
    const __amdgpu_buffer_rsrc_t s_hi = window(a.out_hi, m0, a.out_pl_ld, BM, 2);
    const __amdgpu_buffer_rsrc_t s_lo = window(planes ? a.out_lo : nullptr, m0, a.out_pl_ld, BM, 2);
    auto as_f4 = [](const wd_u32x4 u) { return __builtin_bit_cast(float4, u); };

    // ---- (a) every load
    float4 v[KEEP], r[KEEP];
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
        const int row = rl + k * NRL;
        v[k] = *reinterpret_cast<const float4*>(ep + (row < BM ? row : BM - 1) * LDE + c);  // (a row past the tile: any row, never stored)
    }
    const uint32_t vo_c = live ? (uint32_t)c * 4u : WD_EPI_OOB;
    const float4 bx = as_f4(__builtin_amdgcn_raw_buffer_load_b128(s_bias, vo_c, 0, 0));
    const float4 rv = as_f4(__builtin_amdgcn_raw_buffer_load_b128(s_rv, vo_c, 0, 0));
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
        const int row = rl + k * NRL;
        const uint32_t vo = (live && row < BM) ? ((uint32_t)row * (uint32_t)a.resid_ld + (uint32_t)c) * 4u : WD_EPI_OOB;
        r[k] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(s_res, vo, 0, 0));
    }
    // ---- (b) one wait: vmcnt(0) lgkmcnt(0)
    __builtin_amdgcn_s_waitcnt(0x0070);
    __builtin_amdgcn_sched_barrier(0);
    // ---- (c) the rows
    const bool has_rv = a.rowvec != nullptr, has_res = a.resid != nullptr, silu = a.act == WD_ACT_SILU, stats = a.stat_part != nullptr;
    WdStatAcc st;
    wd_stat_reset(st);
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
        const int row = rl + k * NRL;
        const bool ok = live && row < BM;
        float4 x = v[k];
        x.x += bx.x; x.y += bx.y; x.z += bx.z; x.w += bx.w;
        if (has_rv) {
            x.x += rv.x; x.y += rv.y; x.z += rv.z; x.w += rv.w;
        }
        if (has_res) {
            x.x += r[k].x; x.y += r[k].y; x.z += r[k].z; x.w += r[k].w;
        }
        if (silu) {
            x.x = wd_silu(x.x); x.y = wd_silu(x.y); x.z = wd_silu(x.z); x.w = wd_silu(x.w);
        }
        if (stats && ok) wd_stat_add(st, x);
        uint2 hh = make_uint2(0u, 0u), ll = hh;
        if (planes) wd_split4(x, hh, ll);
        const uint32_t vo_f = ok ? ((uint32_t)row * (uint32_t)a.out_ld + (uint32_t)c) * 4u : WD_EPI_OOB;
        const uint32_t vo_p = ok ? ((uint32_t)row * (uint32_t)a.out_pl_ld + (uint32_t)c) * 2u : WD_EPI_OOB;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(wd_u32x4, x), s_f32, vo_f, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(wd_u32x2, hh), s_hi, vo_p, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(wd_u32x2, ll), s_lo, vo_p, 0, 0);
    }
    // (one sample per tile: nothing parked, the running sums are the panel's)
    if (stats) wd_stat_handover<BM, BN, NT>(a, ep, m0, n0, tid, st, 0, ep, NRL, rl, c, BM);
}

// after the fp32 image of the tile is complete: split-K partial store, or the fused epilogue (BATCH: the kernels whose 64-row tiles
// may take the batched form - wd_gemmw_kernel's 64 x 320, wd_gemmq_kernel's 64 x 80)
template <int BM, int BN, int NT, bool BATCH = false>
__device__ __forceinline__ void wd_epilogue_tail(const wd_gemm_args& a, float* ep, const int m0, const int n0, const int tid,
                                                 const int sidx) {
    constexpr int LDE = BN + 4;
    if constexpr (BATCH) {
        if ((a.dbg & WD_EPI_BATCH_BIT) && wd_epilogue_batch_ok(a, BM, BN)) {
            wd_epilogue_rows<BM, BN, NT>(a, ep, m0, n0, tid);
            return;
        }
    }
    if (a.ksplit > 1) {  // raw partial sums of this K slice -> ws[sidx][m][n]; wd_gemm_reduce applies the epilogue
        float* ws = a.ws + (long)sidx * a.m * a.n;
        const bool v4 = (a.n & 3) == 0;
        for (int i = tid; i < BM * (BN / 4); i += NT) {
            const int row = i / (BN / 4), c = (i - row * (BN / 4)) * 4;
            const int m = m0 + row, n = n0 + c;
            if (m >= a.m || n >= a.n) continue;
            const float4 v = *reinterpret_cast<const float4*>(ep + row * LDE + c);
            if (v4) {
                *reinterpret_cast<float4*>(ws + (long)m * a.n + n) = v;
            } else {
                const float e[4] = {v.x, v.y, v.z, v.w};
                for (int j = 0; j < 4 && n + j < a.n; ++j) ws[(long)m * a.n + n + j] = e[j];
            }
        }
        if (!a.tickets) return;  // a separate wd_gemm_reduce launch combines the slabs
        // ---- in-launch combine (cdna_hip_programming.md section 5 "In-launch split-K reduction", Guideline 16): every slice
        // publishes its slab (all stores drained, barrier, ONE agent-scope release, then a relaxed agent-scope ticket add); the
        // workgroup that draws the last ticket acquires once and sums ALL slabs from the workspace in ascending slice order -
        // the result does not depend on which slice arrived last - inside the ordinary epilogue (bias, FiLM, residual,
        // statistics, planes).  No spinning anywhere: a workgroup that is not last simply ends.  The ticket word is zero
        // before the launch (zero-initialised by the owner, reset here by the last arriver).
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int* s_flag = reinterpret_cast<int*>(ep + BM * LDE);  // first word of the statistics scratch (idle until the epilogue)
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            int* cnt = a.tickets + (m0 / BM) * ((a.n + BN - 1) / BN) + n0 / BN;
            const int old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = old == a.ksplit - 1;
            if (last) {
                __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            *s_flag = last;
        }
        __syncthreads();
        const int is_last = *s_flag;
        __syncthreads();  // (the epilogue reuses the scratch the flag sits in)
        if (!is_last) return;
        wd_gemm_args b = a;
        b.ksplit = 1;
        wd_epilogue_from_image<BM, BN, NT, true>(b, ep, m0, n0, tid, a.ksplit);
        return;
    }
    wd_epilogue_from_image<BM, BN, NT>(a, ep, m0, n0, tid);
}

// Combine + the consumer's GroupNorm for one 64-row x 40-column tile whose rows are ONE sample (hw_out == 64, wd_gemm_args::gn_*):
// the slabs summed in ascending order, bias / FiLM row / residual, the fp32 result, the (sample, group) statistics - written to
// stat_part exactly as the ordinary combine writes them (same summation order) - and SiLU?(GroupNorm(result)) as operand planes.
// A thread's (at most three) rows stay in its registers between the statistics and the normalisation, so the wd_gn_apply
// launch and its pass over the tensor disappear (ten of them on the 4x16 level of the base UNet).
// WS = true: the values are summed from the split-K slabs of a.ws (the combine launch, 64 x 40 tiles of 256 threads); WS = false:
// they are the finished fp32 image `img` (row pitch BN + 4) of a kernel that owns all of K (wd_gemmk_kernel, 64 x 80, 512 threads).
// `ep`: scratch of 2 * NRL * BN + 2 * BN / stat_cpg doubles (16-byte aligned), not overlapping img.
template <int BN, int NT, bool WS>
__device__ __forceinline__ void wd_gn_tile(const wd_gemm_args& a, const float* img, float* ep, const int m0, const int n0, const int tid) {
    constexpr int BM = 64, Q = BN / 4, NRL = NT / Q, KEEP = (BM + NRL - 1) / NRL;
    const int rl = tid / Q, c = (tid - rl * Q) * 4;
    const bool live = rl < NRL;
    const int no = n0 + c;
    const long total = (long)a.m * a.n;
    float4 v[KEEP];
    bool ok[KEEP];
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
        const int row = rl + k * NRL;
        ok[k] = live && row < BM && m0 + row < a.m;
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[k]) v[k] = WS ? *reinterpret_cast<const float4*>(a.ws + (long)(m0 + row) * a.n + no)
                             : *reinterpret_cast<const float4*>(img + row * (BN + 4) + c);
    }
    for (int sp = 1; WS && sp < a.ksplit; ++sp) {
        float4 q[KEEP];
#pragma unroll
        for (int k = 0; k < KEEP; ++k) {
            q[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok[k]) q[k] = *reinterpret_cast<const float4*>(a.ws + (long)sp * total + (long)(m0 + rl + k * NRL) * a.n + no);
        }
#pragma unroll
        for (int k = 0; k < KEEP; ++k) {
            v[k].x += q[k].x; v[k].y += q[k].y; v[k].z += q[k].z; v[k].w += q[k].w;
        }
    }
    float4 bx = make_float4(0.f, 0.f, 0.f, 0.f), rv = bx;
    if (live && a.bias) bx = *reinterpret_cast<const float4*>(a.bias + no);
    if (live && a.rowvec) rv = *reinterpret_cast<const float4*>(a.rowvec + (long)(m0 / a.hw_out) * a.rowvec_ld + no);
    WdStatAcc st;
    wd_stat_reset(st);
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
        if (!ok[k]) continue;
        const long m = m0 + rl + k * NRL;
        v[k].x += bx.x; v[k].y += bx.y; v[k].z += bx.z; v[k].w += bx.w;
        if (a.rowvec) {
            v[k].x += rv.x; v[k].y += rv.y; v[k].z += rv.z; v[k].w += rv.w;
        }
        if (a.resid) {
            const float4 q = *reinterpret_cast<const float4*>(a.resid + m * a.resid_ld + no);
            v[k].x += q.x; v[k].y += q.y; v[k].z += q.z; v[k].w += q.w;
        }
        wd_stat_add(st, v[k]);
        if (a.out_f32) *reinterpret_cast<float4*>(a.out_f32 + m * a.out_ld + no) = v[k];
    }
    double ssum[4], ssq[4];
    wd_stat_finish(st, ssum, ssq);
    // per-thread column sums -> (group, row lane) -> (group): the order and the arithmetic of the ordinary combine (all in double)
    double* scr = reinterpret_cast<double*>(ep);    // [2][NRL][BN]: sums, sums of squares
    double* gs = scr + 2 * NRL * BN;                 // [BN / stat_cpg][2]
    const int cps = a.stat_cpg, ngt = BN / cps;
    if (live) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const double* e = q ? ssq : ssum;
            double* o = scr + (q * NRL + rl) * BN + c;
            *reinterpret_cast<double2*>(o) = make_double2(e[0], e[1]);
            *reinterpret_cast<double2*>(o + 2) = make_double2(e[2], e[3]);
        }
    }
    __syncthreads();
    wd_stat_reduce<NT>(scr, 2, NRL, ngt, BN, cps, tid);
    __syncthreads();
    if (tid < 2 * ngt && n0 + (tid % ngt) * cps < a.n) {
        const int g = tid % ngt, q = tid / ngt;
        double su = 0.0;
        for (int l = 0; l < NRL; ++l) su += scr[(q * NRL + l) * BN + g * cps];
        gs[2 * g + q] = su;
        a.stat_part[((long)(m0 / a.hw_out) * (a.n / cps) + n0 / cps + g) * 2 + q] = su;  // (one chunk per sample: hw_out == BM)
    }
    __syncthreads();
    if (!live) return;
    // the consumer's groups: gn_cpg channels = gn_cpg / stat_cpg statistics groups (wd_gn_apply's arithmetic)
    const int gcp = a.gn_cpg, ratio = gcp / cps;
    float sc[4], sh[4];
    const float4 ga = *reinterpret_cast<const float4*>(a.gn_gamma + no);
    const float4 be = *reinterpret_cast<const float4*>(a.gn_beta + no);
    const float gaa[4] = {ga.x, ga.y, ga.z, ga.w}, bea[4] = {be.x, be.y, be.z, be.w};
    int gprev = -1;
    float mean = 0.f, rstd = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int g = (c + j) / gcp;
        if (g != gprev) {
            double ds = 0.0, dq = 0.0;
            for (int k = 0; k < ratio; ++k) {
                ds += gs[2 * (g * ratio + k)];
                dq += gs[2 * (g * ratio + k) + 1];
            }
            const double n = (double)a.hw_out * gcp;
            const double mu = ds / n;
            double var = dq / n - mu * mu;
            if (var < 0.0) var = 0.0;
            mean = (float)mu;
            rstd = (float)(1.0 / sqrt(var + (double)a.gn_eps));
            gprev = g;
        }
        sc[j] = rstd * gaa[j];
        sh[j] = bea[j] - mean * sc[j];
    }
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
        if (!ok[k]) continue;
        const long m = m0 + rl + k * NRL;
        float4 y;
        y.x = v[k].x * sc[0] + sh[0]; y.y = v[k].y * sc[1] + sh[1]; y.z = v[k].z * sc[2] + sh[2]; y.w = v[k].w * sc[3] + sh[3];
        if (a.gn_silu) {
            y.x = wd_silu(y.x); y.y = wd_silu(y.y); y.z = wd_silu(y.z); y.w = wd_silu(y.w);
        }
        uint2 hh, ll;
        wd_split4(y, hh, ll);
        *reinterpret_cast<uint2*>(a.out_hi + m * a.out_pl_ld + no) = hh;
        if (a.out_lo) *reinterpret_cast<uint2*>(a.out_lo + m * a.out_pl_ld + no) = ll;
    }
}


}  // namespace
