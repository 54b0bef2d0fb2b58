// GroupNorm statistics / apply(+SiLU) -> split-bf16 planes, LayerNorm -> planes, plain split.
// HBM-bound streaming kernels: 16-byte loads, 8-byte plane stores, deterministic reductions (no atomics).
// Reference: GroupNorm32 unet.py:427-431 (eps 1e-5), Normalize unet.py:161-162 (eps 1e-6),
// nn.LayerNorm unet.py:314-316, SiLU unet.py:594,618.
#include "wd_common.h"
#include "wd_philox.h"

namespace {

constexpr int GN_TOK = 32;  // tokens per statistics chunk

// grid (nchunk, batch); block (64 * ceil(c/4/64), 2).  thread x owns channels 4x..4x+3, y splits tokens.
// Every stage is in double: a thread's sums over its tokens (the square of an fp32 value is exact in double), the LDS hand-over,
// the sum over the group's columns.  The partials are the sums of the fp32 values to double rounding, so the consumers'
// var = sumsq / n - mean^2 loses nothing to the producer however far the group's mean is from zero (an fp32 sum of squares is off
// by 2^-24 of itself, (mean / std)^2 times that in the variance).
__global__ void gn_stats_kernel(const float* __restrict__ x, int ld, int hw, int c, int cpg, int nchunk,
                                double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* s_sum = reinterpret_cast<double*>(smem);  // [2][c]
    double* s_sq = s_sum + 2 * c;                     // [2][c]
    const int b = blockIdx.y, j = blockIdx.x;
    const int cx = threadIdx.x * 4;
    const int t0 = j * GN_TOK, t1 = min(hw, t0 + GN_TOK);
    if (cx < c) {
        double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
        const float* base = x + ((long)b * hw) * ld + cx;
        for (int t = t0 + threadIdx.y; t < t1; t += 2) {
            const float4 v = *reinterpret_cast<const float4*>(base + (long)t * ld);
            const double e[4] = {(double)v.x, (double)v.y, (double)v.z, (double)v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s[k] += e[k];
                q[k] = fma(e[k], e[k], q[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s_sum[threadIdx.y * c + cx + k] = s[k];
            s_sq[threadIdx.y * c + cx + k] = q[k];
        }
    }
    __syncthreads();
    const int ng = c / cpg;
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    if (tid < ng) {
        double ds = 0.0, dq = 0.0;
        for (int k = 0; k < cpg; ++k) {
            const int ch = tid * cpg + k;
            ds += s_sum[ch] + s_sum[c + ch];
            dq += s_sq[ch] + s_sq[c + ch];
        }
        double* o = part + (((long)b * nchunk + j) * ng + tid) * 2;
        o[0] = ds;
        o[1] = dq;
    }
}

// grid (ceil(hw / TOK_PER_WG), batch), block 256.  One float4 (4 channels) per thread per step.
constexpr int AP_TOK = 8;
struct GnSrc {  // one source tensor of a GroupNorm over a channel concat: its rows, its statistics, its channel offset in the concat
    const float* x;
    const double* part;
    int ld, c, nchunk, part_cpg, c_off;
    const int32_t* perm;  // NULL, or [hw]: the row (inside its sample) that holds position t - a producer that wrote its rows in another order
};

__device__ __forceinline__ float4 gn_drop4(const wd_dropout& d, uint64_t drow, int token, int c, int ch, float4 y) {
    bool keep[4];
    wd_dropout_keep4(d, drow, token, c, ch, keep);
    return make_float4(wd_dropout_apply(keep[0], y.x, d.scale), wd_dropout_apply(keep[1], y.y, d.scale),
                       wd_dropout_apply(keep[2], y.z, d.scale), wd_dropout_apply(keep[3], y.w, d.scale));
}

// grid (token tiles, batch, sources): blockIdx.z picks the source.
// D: nothing (the plain kernel - its signature and code are those of the kernel without the feature), or one wd_dropout (DROP): the
// training dropout mask (wd_philox.h) on the normalised(+SiLU) value before the split - one draw per float4, the lane's four
// channels being four consecutive elements (c % 4 == 0).
template <typename... D>
__global__ void gn_apply_kernel(const GnSrc s0, const GnSrc s1, int hw, int cpg, const float* __restrict__ gamma,
                                const float* __restrict__ beta, float eps, int silu, wd_bf16* __restrict__ out_hi,
                                wd_bf16* __restrict__ out_lo, int out_ld, wd_bf16* __restrict__ raw_hi,
                                wd_bf16* __restrict__ raw_lo, const D... dd) {
    constexpr bool DROP = sizeof...(D) != 0;
    const auto& d = wd_dropout_of(dd...);
    const GnSrc& sr = blockIdx.z ? s1 : s0;
    const float* __restrict__ x = sr.x;
    const double* __restrict__ part = sr.part;
    const int ld = sr.ld, c = sr.c, nchunk = sr.nchunk, part_cpg = sr.part_cpg, c_off = sr.c_off;
    __shared__ float s_mean[32], s_rstd[32];
    const int b = blockIdx.y;
    const int ng = c / cpg;
    if (threadIdx.x < ng) {
        // the statistics array holds c / part_cpg groups per (sample, chunk); this norm's group = `ratio` of them
        const int ratio = cpg / part_cpg, ngs = c / part_cpg;
        double ds = 0.0, dq = 0.0;
        for (int j = 0; j < nchunk; ++j) {
            const double* p = part + (((long)b * nchunk + j) * ngs + threadIdx.x * ratio) * 2;
            for (int k = 0; k < ratio; ++k) {
                ds += p[2 * k];
                dq += p[2 * k + 1];
            }
        }
        const double n = (double)hw * cpg;
        const double mean = ds / n;
        double var = dq / n - mean * mean;
        if (var < 0.0) var = 0.0;
        s_mean[threadIdx.x] = (float)mean;
        s_rstd[threadIdx.x] = (float)(1.0 / sqrt(var + (double)eps));
    }
    __syncthreads();
    const int c4 = c >> 2;
    const int t0 = blockIdx.x * AP_TOK, nt = min(AP_TOK, hw - t0);
    uint64_t drow = 0;
    if constexpr (DROP) drow = wd_dropout_row(d, b);
    if (c4 <= 256) {
        // thread = (token lane, channel quad): the quad is fixed, so y = v * scale + shift with four per-thread constants each
        // (the group lookups - integer divisions by a run-time cpg - happen once, not per element)
        const int rpp = 256 / c4;  // tokens per pass
        const int tl = threadIdx.x / c4, cx = (threadIdx.x - tl * c4) * 4;
        if (tl >= rpp) return;
        float sc[4], sh[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int g = (cx + j) / cpg;  // the four channels may straddle two groups
            sc[j] = s_rstd[g] * gamma[c_off + cx + j];
            sh[j] = beta[c_off + cx + j] - s_mean[g] * sc[j];
        }
        for (int t = tl; t < nt; t += rpp) {
            const long row = (long)b * hw + t0 + t;
            const long srow = sr.perm ? (long)b * hw + sr.perm[t0 + t] : row;
            const float4 v = *reinterpret_cast<const float4*>(x + srow * ld + cx);
            float4 y = make_float4(v.x * sc[0] + sh[0], v.y * sc[1] + sh[1], v.z * sc[2] + sh[2], v.w * sc[3] + sh[3]);
            if (silu) {
                y.x = wd_silu(y.x); y.y = wd_silu(y.y); y.z = wd_silu(y.z); y.w = wd_silu(y.w);
            }
            if constexpr (DROP) y = gn_drop4(d, drow, t0 + t, c, cx, y);
            uint2 h, l;
            wd_split4(y, h, l);
            const long o = row * out_ld + c_off + cx;
            *reinterpret_cast<uint2*>(out_hi + o) = h;
            if (out_lo) *reinterpret_cast<uint2*>(out_lo + o) = l;
            if (raw_hi) {
                wd_split4(v, h, l);
                *reinterpret_cast<uint2*>(raw_hi + o) = h;
                if (raw_lo) *reinterpret_cast<uint2*>(raw_lo + o) = l;
            }
        }
        return;
    }
    const int total = nt * c4;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int t = i / c4, cx = (i - t * c4) * 4;
        const long row = (long)b * hw + t0 + t;
        const long srow = sr.perm ? (long)b * hw + sr.perm[t0 + t] : row;
        const float4 v = *reinterpret_cast<const float4*>(x + srow * ld + cx);
        float4 y;
        {
            const int g = cx / cpg, g1 = (cx + 1) / cpg, g2 = (cx + 2) / cpg, g3 = (cx + 3) / cpg;
            const float4 ga = *reinterpret_cast<const float4*>(gamma + c_off + cx);
            const float4 be = *reinterpret_cast<const float4*>(beta + c_off + cx);
            const float s0 = s_rstd[g] * ga.x, s1 = s_rstd[g1] * ga.y, s2 = s_rstd[g2] * ga.z, s3 = s_rstd[g3] * ga.w;
            y.x = v.x * s0 + (be.x - s_mean[g] * s0);
            y.y = v.y * s1 + (be.y - s_mean[g1] * s1);
            y.z = v.z * s2 + (be.z - s_mean[g2] * s2);
            y.w = v.w * s3 + (be.w - s_mean[g3] * s3);
        }
        if (silu) {
            y.x = wd_silu(y.x); y.y = wd_silu(y.y); y.z = wd_silu(y.z); y.w = wd_silu(y.w);
        }
        if constexpr (DROP) y = gn_drop4(d, drow, t0 + t, c, cx, y);
        uint2 h, l;
        wd_split4(y, h, l);
        const long o = row * out_ld + c_off + cx;
        *reinterpret_cast<uint2*>(out_hi + o) = h;
        if (out_lo) *reinterpret_cast<uint2*>(out_lo + o) = l;
        if (raw_hi) {
            wd_split4(v, h, l);
            *reinterpret_cast<uint2*>(raw_hi + o) = h;
            if (raw_lo) *reinterpret_cast<uint2*>(raw_lo + o) = l;
        }
    }
}

// one wave per row; c <= 64 * 4 * LN_MAX4
constexpr int LN_MAX4 = 8;
__global__ void layernorm_kernel(const float* __restrict__ x, int ld, int rows, int c, const float* __restrict__ gamma,
                                 const float* __restrict__ beta, float eps, wd_bf16* __restrict__ out_hi,
                                 wd_bf16* __restrict__ out_lo, int out_ld) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int c4 = c >> 2;
    float4 v[LN_MAX4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAX4; ++i) {
        const int f = lane + 64 * i;
        if (f < c4) {
            v[i] = *reinterpret_cast<const float4*>(x + (long)row * ld + f * 4);
            s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        }
    }
    const float mean = wd_wave_sum(s) / (float)c;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAX4; ++i) {
        const int f = lane + 64 * i;
        if (f < c4) {
            const float a = v[i].x - mean, b = v[i].y - mean, cc = v[i].z - mean, d = v[i].w - mean;
            q += (a * a + b * b) + (cc * cc + d * d);
        }
    }
    const float rstd = 1.0f / sqrtf(wd_wave_sum(q) / (float)c + eps);
#pragma unroll
    for (int i = 0; i < LN_MAX4; ++i) {
        const int f = lane + 64 * i;
        if (f < c4) {
            const float4 ga = *reinterpret_cast<const float4*>(gamma + f * 4);
            const float4 be = *reinterpret_cast<const float4*>(beta + f * 4);
            float4 y;
            y.x = (v[i].x - mean) * rstd * ga.x + be.x;
            y.y = (v[i].y - mean) * rstd * ga.y + be.y;
            y.z = (v[i].z - mean) * rstd * ga.z + be.z;
            y.w = (v[i].w - mean) * rstd * ga.w + be.w;
            uint2 h, l;
            wd_split4(y, h, l);
            const long o = (long)row * out_ld + f * 4;
            *reinterpret_cast<uint2*>(out_hi + o) = h;
            if (out_lo) *reinterpret_cast<uint2*>(out_lo + o) = l;
        }
    }
}

__global__ void split_kernel(const float* __restrict__ x, int ld, int rows, int c, int silu,
                             wd_bf16* __restrict__ out_hi, wd_bf16* __restrict__ out_lo, int out_ld) {
    const int c4 = c >> 2;
    const long total = (long)rows * c4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / c4;
        const int cx = (int)(i - r * c4) * 4;
        float4 v = *reinterpret_cast<const float4*>(x + r * ld + cx);
        if (silu) {
            v.x = wd_silu(v.x); v.y = wd_silu(v.y); v.z = wd_silu(v.z); v.w = wd_silu(v.w);
        }
        uint2 h, l;
        wd_split4(v, h, l);
        *reinterpret_cast<uint2*>(out_hi + r * out_ld + cx) = h;
        if (out_lo) *reinterpret_cast<uint2*>(out_lo + r * out_ld + cx) = l;
    }
}

// ---- out[b][o][y][x] = Conv3x3(SiLU(GroupNorm(x)))[o] + bias[o] for a convolution with FEW output channels (<= 4): the UNet's
// last layer (unet.py:1453-1458: GroupNorm32, SiLU, conv 320 -> 4).  As a GEMM it fills 4 of a tile's 64 columns; here one
// workgroup owns a tile of 4 image rows x 16 columns of one sample and walks the channels in chunks of 64: the chunk's 6 x 18 pixel
// tile (halo included, zero outside the image) is normalised + SiLU'd into LDS once, next to the chunk's weights as
// [channel][tap][4], and multiplied in fp32 on the VALU.
// lane = (channel slot s, column x) with x in the low four bits, so the 16 lanes of a DPP row are the 16 columns of the tile.  A
// lane owns the 4 pixels of its column and 2 of the chunk's channels (8 waves x 4 slots x 2 = 64): per channel it reads the six
// rows of its column (8 bytes per row for both channels), takes the left and right neighbours from the neighbouring lanes by DPP
// row shifts - the two lanes at the ends of a row keep the halo column's value instead, the `old` operand of the shift - and reads
// the channel's 9 x 4 weights once into registers for 144 products.  (One pixel per lane needed a weight read per four products.)
// What a chunk needs from global memory - its rows, its weights, gamma and beta - is requested two chunks ahead, into registers,
// so that the latency of a chunk hides under the arithmetic of the two before it.
// grid (batch, ceil(W / 16), ceil(H / 4)), block 512; c % 64 == 0, weights = the parameter [oc][c][3][3].
constexpr int GC_CH = 64;            // channels per chunk
constexpr int GC_PITCH = GC_CH + 4;  // floats per pixel in the tile (shifts the banks from pixel to pixel)
constexpr int GC_TR = 4, GC_TC = 16;  // the tile: rows x columns
constexpr int GC_NT = 512, GC_SLOTS = GC_NT / GC_TC, GC_CPS = GC_CH / GC_SLOTS;  // threads, channel slots, channels per slot and chunk
constexpr int GC_ITEMS = (GC_TR + 2) * (GC_TC + 2) * (GC_CH / 4);                // float4 of a chunk's tile
constexpr int GC_NLD = (GC_ITEMS + GC_NT - 1) / GC_NT;                           // ... per thread (4, the last one partly)
constexpr int GC_NWV = (4 * GC_CH * 9 + GC_NT - 1) / GC_NT;                      // weights of a chunk per thread (5, the last one partly)
constexpr int GC_TILE_FLOATS = (GC_TR + 2) * (GC_TC + 2) * GC_PITCH;
constexpr int GC_RED_FLOATS = GC_SLOTS * GC_TR * GC_TC * 4;  // the partial sums at the end: [slot][pixel][4]
static_assert(GC_CPS == 2, "a lane reads its two channels of a pixel as one float2");

// lane i of a DPP row (16 lanes) gets v of lane i - 1 (shr) / i + 1 (shl); the lane without such a neighbour keeps `old`
__device__ __forceinline__ float gc_from_left(float old, float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), 0x111, 0xf, 0xf, false));
}
__device__ __forceinline__ float gc_from_right(float old, float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), 0x101, 0xf, 0xf, false));
}

__global__ void __launch_bounds__(GC_NT) gn_conv_few_kernel(const float* __restrict__ x, int ld, int H, int W, int c, int cpg, int nchunk,
                                                           int part_cpg, const double* __restrict__ part,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                           int silu, const float* __restrict__ w, const float* __restrict__ bias, int oc,
                                                           float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_t[GC_TILE_FLOATS > GC_RED_FLOATS ? GC_TILE_FLOATS : GC_RED_FLOATS];
    __shared__ __attribute__((aligned(16))) float s_w[GC_CH * 9 * 4];  // [channel][tap][4]: this chunk's weights
    __shared__ float s_mean[32], s_rstd[32];
    // grid.x = batch: consecutive workgroup ids = consecutive samples, so the tiles of one sample - whose halos overlap - are dealt
    // to the same XCD and re-read from its L2
    const int b = blockIdx.x, x0 = blockIdx.y * GC_TC, y0 = blockIdx.z * GC_TR, tid = threadIdx.x;
    const int hw = H * W, ng = c / cpg;
    // what a thread brings in for a chunk: its share of the tile (item i = tid + 512 k -> tile row r, tile column px, channel quad
    // c4 - the same quad for all of them, 512 being a multiple of the 16 quads of a chunk), of the weights, and gamma / beta of its
    // quad.  Two chunks are in flight: chunk i + 2 is requested when chunk i has been written to LDS.
    struct Pre {
        float4 pv[GC_NLD], ga, be;
        float wv[GC_NWV];
    };
    const int cq = (tid & (GC_CH / 4 - 1)) * 4;
    // Every load is unconditional and in bounds - coordinates outside the image are clamped onto it (their values are never used:
    // the tile gets zeros there), a chunk past the last one re-reads the last - so that the requests are straight-line code and
    // the compiler's vmcnt bookkeeping can wait for the older chunk while the newer one is still in flight (a branch around a load
    // makes it wait for everything).
    auto request = [&](Pre& P, int c0w) {
        const int c0 = min(c0w, c - GC_CH);
#pragma unroll
        for (int k = 0; k < GC_NLD; ++k) {
            const int i = tid + GC_NT * k;
            const int r = i / ((GC_TC + 2) * (GC_CH / 4)), rem = i - r * ((GC_TC + 2) * (GC_CH / 4));
            const int px = rem / (GC_CH / 4), c4 = rem - px * (GC_CH / 4);
            const int yy = min(max(y0 + r - 1, 0), H - 1), xx = min(max(x0 + px - 1, 0), W - 1);
            P.pv[k] = *reinterpret_cast<const float4*>(x + ((long)b * hw + (long)yy * W + xx) * ld + c0 + c4 * 4);
        }
#pragma unroll
        for (int k = 0; k < GC_NWV; ++k) {  // weights [o][c0 .. c0+63][9]: contiguous per o
            const int i = min(tid + GC_NT * k, 4 * GC_CH * 9 - 1);
            const int o = i / (GC_CH * 9), rem = i - o * (GC_CH * 9);
            P.wv[k] = w[((long)min(o, oc - 1) * c + c0) * 9 + rem];
        }
        P.ga = make_float4(gamma[c0 + cq], gamma[c0 + cq + 1], gamma[c0 + cq + 2], gamma[c0 + cq + 3]);
        P.be = make_float4(beta[c0 + cq], beta[c0 + cq + 1], beta[c0 + cq + 2], beta[c0 + cq + 3]);
    };
    Pre pa, pb;
    request(pa, 0);
    request(pb, GC_CH);
    // mean and 1 / std of the groups: 16 threads per group fold the chunk partials (one global round trip for up to 16 chunks
    // instead of one per chunk), one thread sums their sixteen terms in order
    {
        double* s_ps = reinterpret_cast<double*>(s_t);  // [16][32][2]
        const int g = tid & 31, jl = tid >> 5;
        if (g < ng) {
            const int ratio = cpg / part_cpg, ngs = c / part_cpg;
            double ds = 0.0, dq = 0.0;
            for (int j = jl; j < nchunk; j += GC_NT / 32) {
                const double* p = part + (((long)b * nchunk + j) * ngs + g * ratio) * 2;
                for (int k = 0; k < ratio; ++k) {
                    ds += p[2 * k];
                    dq += p[2 * k + 1];
                }
            }
            s_ps[(jl * 32 + g) * 2] = ds;
            s_ps[(jl * 32 + g) * 2 + 1] = dq;
        }
        __syncthreads();
        if (tid < ng) {
            double ds = 0.0, dq = 0.0;
            for (int l = 0; l < GC_NT / 32; ++l) {
                ds += s_ps[(l * 32 + tid) * 2];
                dq += s_ps[(l * 32 + tid) * 2 + 1];
            }
            const double n = (double)hw * cpg;
            const double mean = ds / n;
            double var = dq / n - mean * mean;
            if (var < 0.0) var = 0.0;
            s_mean[tid] = (float)mean;
            s_rstd[tid] = (float)(1.0 / sqrt(var + (double)eps));
        }
    }
    __syncthreads();
    const int lx = tid & (GC_TC - 1), slot = tid / GC_TC;
    const bool edge = lx == 0 || lx == GC_TC - 1;
    // this lane's column in tile row 0 (row r is r * 18 pixels on), and the halo column next to it (read by the lanes at the
    // ends of a row only); its channels' weights
    const float* at = s_t + (lx + 1) * GC_PITCH + slot * GC_CPS;
    const float* ah = s_t + (lx == 0 ? 0 : GC_TC + 1) * GC_PITCH + slot * GC_CPS;
    const float* wt = s_w + slot * GC_CPS * 36;
    float acc[GC_TR][4];
#pragma unroll
    for (int r = 0; r < GC_TR; ++r)
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[r][o] = 0.f;
    auto chunk = [&](Pre& P, int c0) {
        // ---- this chunk: weights -> [channel][tap][4] (the slots of o >= oc zero); tile normalised (+ SiLU), zero outside the image
#pragma unroll
        for (int k = 0; k < GC_NWV; ++k) {
            const int i = tid + GC_NT * k;
            const int o = i / (GC_CH * 9), rem = i - o * (GC_CH * 9);  // rem = channel * 9 + tap: the parameter's own order
            if (o < 4) s_w[rem * 4 + o] = o < oc ? P.wv[k] : 0.f;
        }
        float sc[4], sh[4];
        {
            const float ga[4] = {P.ga.x, P.ga.y, P.ga.z, P.ga.w}, be[4] = {P.be.x, P.be.y, P.be.z, P.be.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int g = (c0 + cq + j) / cpg;
                sc[j] = s_rstd[g] * ga[j];
                sh[j] = be[j] - s_mean[g] * sc[j];
            }
        }
#pragma unroll
        for (int k = 0; k < GC_NLD; ++k) {
            const int i = tid + GC_NT * k;
            if (i >= GC_ITEMS) continue;
            const int r = i / ((GC_TC + 2) * (GC_CH / 4)), rem = i - r * ((GC_TC + 2) * (GC_CH / 4));
            const int px = rem / (GC_CH / 4), c4 = rem - px * (GC_CH / 4);
            const int yy = y0 + r - 1, xx = x0 + px - 1;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                const float4 v = P.pv[k];
                o = make_float4(v.x * sc[0] + sh[0], v.y * sc[1] + sh[1], v.z * sc[2] + sh[2], v.w * sc[3] + sh[3]);
                if (silu) {
                    o.x = wd_silu(o.x); o.y = wd_silu(o.y); o.z = wd_silu(o.z); o.w = wd_silu(o.w);
                }
            }
            *reinterpret_cast<float4*>(s_t + (r * (GC_TC + 2) + px) * GC_PITCH + c4 * 4) = o;
        }
        request(P, c0 + 2 * GC_CH);  // in flight while this chunk and the next are multiplied
        __syncthreads();
        // ---- every lane multiplies (a lane outside the image sees zeros and stores nothing): the row shifts need all 64
        float a[GC_TR + 2][3][GC_CPS];  // [tile row][dx][channel of the slot]
#pragma unroll
        for (int r = 0; r < GC_TR + 2; ++r) {
            const float2 ce = *reinterpret_cast<const float2*>(at + r * (GC_TC + 2) * GC_PITCH);
            float2 ha = make_float2(0.f, 0.f);
            if (edge) ha = *reinterpret_cast<const float2*>(ah + r * (GC_TC + 2) * GC_PITCH);
            a[r][1][0] = ce.x; a[r][1][1] = ce.y;
            a[r][0][0] = gc_from_left(ha.x, ce.x); a[r][0][1] = gc_from_left(ha.y, ce.y);
            a[r][2][0] = gc_from_right(ha.x, ce.x); a[r][2][1] = gc_from_right(ha.y, ce.y);
        }
#pragma unroll
        for (int j = 0; j < GC_CPS; ++j)
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float4 w4 = *reinterpret_cast<const float4*>(wt + (j * 9 + t) * 4);
#pragma unroll
                for (int r = 0; r < GC_TR; ++r) {
                    const float v = a[r + t / 3][t % 3][j];
                    acc[r][0] += v * w4.x; acc[r][1] += v * w4.y; acc[r][2] += v * w4.z; acc[r][3] += v * w4.w;
                }
            }
        __syncthreads();
    };
    for (int c0 = 0;; c0 += 2 * GC_CH) {  // (no branch joins behind a request: see there)
        chunk(pa, c0);
        if (c0 + GC_CH >= c) break;
        chunk(pb, c0 + GC_CH);
        if (c0 + 2 * GC_CH >= c) break;
    }
    // ---- sum the channel slots in a fixed order, add the bias, write NCHW
    float* s_red = s_t;  // [slot][tile pixel = r * 16 + x][4]
#pragma unroll
    for (int r = 0; r < GC_TR; ++r)
        *reinterpret_cast<float4*>(s_red + ((slot * GC_TR + r) * GC_TC + lx) * 4) = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
    __syncthreads();
    for (int i = tid; i < GC_TR * GC_TC * oc; i += GC_NT) {
        const int o = i / (GC_TR * GC_TC), p = i - o * (GC_TR * GC_TC);
        const int yy = y0 + p / GC_TC, xx = x0 + p % GC_TC;
        if (yy >= H || xx >= W) continue;
        float v = bias ? bias[o] : 0.f;
        for (int g = 0; g < GC_SLOTS; ++g) v += s_red[(g * GC_TR * GC_TC + p) * 4 + o];
        out[(((long)b * oc + o) * H + yy) * W + xx] = v;
    }
}

// part[b][nchunk][ng][2] -> out[b][1][ng][2]: the chunk sums of a sample folded once (fixed order) instead of by every workgroup
// of wd_gn_apply - at 16384 positions per sample (the VAE decoder's last level) that loop is 128 chunks long.
// grid (batch), block 256 = 4 chunk lanes x 64 (group, sum / sum of squares) columns; ng * 2 <= 64.
__global__ void __launch_bounds__(256) gn_fold_chunks_kernel(const double* __restrict__ part, int nchunk, int ng2,
                                                            double* __restrict__ out) {
    __shared__ double red[4][64];
    const int col = threadIdx.x & 63, lane = threadIdx.x >> 6;
    const long b = blockIdx.x;
    double acc = 0.0;
    if (col < ng2)
        for (int j = lane; j < nchunk; j += 4) acc += part[(b * nchunk + j) * ng2 + col];
    red[lane][col] = acc;
    __syncthreads();
    if (lane == 0 && col < ng2) out[b * ng2 + col] = (red[0][col] + red[1][col]) + (red[2][col] + red[3][col]);
}

}  // namespace

extern "C" int wd_gn_nchunk(int hw) { return (hw + GN_TOK - 1) / GN_TOK; }

extern "C" int wd_gn_fold_chunks(const double* part, int batch, int nchunk, int ngroups, double* out, void* stream) {
    if (!part || !out || batch <= 0 || nchunk <= 0 || ngroups <= 0 || ngroups > 32) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_GNSTATS, st);
    hipLaunchKernelGGL(gn_fold_chunks_kernel, dim3(batch), dim3(256), 0, st, part, nchunk, 2 * ngroups, out);
    return wd_check_launch();
}

extern "C" int wd_gn_stats(const float* x, int ld, int batch, int hw, int c, int cpg, double* part, void* stream) {
    if (!x || !part || batch <= 0 || hw <= 0 || c <= 0 || cpg <= 0) return WD_EINVAL;
    if (c % 4 || ld % 4 || c % cpg || c / cpg > 256 || c > 4096) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nchunk = wd_gn_nchunk(hw);
    const int bx = 64 * ((c / 4 + 63) / 64);
    if (bx * 2 > 1024) return WD_EINVAL;
    WdLaunchScope scope(WD_CLS_GNSTATS, st);
    hipLaunchKernelGGL(gn_stats_kernel, dim3(nchunk, batch), dim3(bx, 2), 4 * c * sizeof(double), st, x, ld, hw, c, cpg,
                       nchunk, part);
    return wd_check_launch();
}

extern "C" int wd_gn_apply(const float* x, int ld, int batch, int hw, int c, int cpg, const double* part, int nchunk,
                           int part_cpg, const float* gamma, const float* beta, float eps, int silu, wd_bf16* out_hi,
                           wd_bf16* out_lo, int out_ld, int c_off, wd_bf16* raw_hi, wd_bf16* raw_lo, void* stream) {
    if (!x || !part || !gamma || !beta || !out_hi || batch <= 0 || hw <= 0 || nchunk <= 0 || part_cpg <= 0) return WD_EINVAL;
    if (c % 4 || ld % 4 || out_ld % 4 || c_off % 4 || c % cpg || c / cpg > 32 || cpg % part_cpg) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_GNAPPLY, st);
    const GnSrc s0 = {x, part, ld, c, nchunk, part_cpg, c_off, nullptr};
    hipLaunchKernelGGL(gn_apply_kernel<>, dim3((hw + AP_TOK - 1) / AP_TOK, batch, 1), dim3(256), 0, st, s0, s0, hw, cpg, gamma, beta, eps,
                       silu, out_hi, out_lo, out_ld, raw_hi, raw_lo);
    return wd_check_launch();
}

extern "C" int wd_gn_apply_dropout(const float* x, int ld, int batch, int hw, int c, int cpg, const double* part, int nchunk,
                                   int part_cpg, const float* gamma, const float* beta, float eps, int silu, wd_bf16* out_hi,
                                   wd_bf16* out_lo, int out_ld, int c_off, wd_bf16* raw_hi, wd_bf16* raw_lo, const wd_dropout* d,
                                   void* stream) {
    if (!x || !part || !gamma || !beta || !out_hi || !d || batch <= 0 || hw <= 0 || c <= 0 || cpg <= 0 || nchunk <= 0 || part_cpg <= 0)
        return WD_EINVAL;
    if (c % 4 || ld % 4 || out_ld % 4 || c_off % 4 || c % cpg || c / cpg > 32 || cpg % part_cpg) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_GNAPPLY, st);
    const GnSrc s0 = {x, part, ld, c, nchunk, part_cpg, c_off, nullptr};
    hipLaunchKernelGGL(gn_apply_kernel<wd_dropout>, dim3((hw + AP_TOK - 1) / AP_TOK, batch, 1), dim3(256), 0, st, s0, s0, hw, cpg, gamma,
                       beta, eps, silu, out_hi, out_lo, out_ld, raw_hi, raw_lo, *d);
    return wd_check_launch();
}

extern "C" int wd_gn_apply2(const float* xa, int lda, int ca, const double* part_a, int nchunk_a, int part_cpg_a, int c_off_a,
                            const float* xb, int ldb, int cb, const double* part_b, int nchunk_b, int part_cpg_b, int c_off_b,
                            int batch, int hw, int cpg, const float* gamma, const float* beta, float eps, int silu,
                            wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, wd_bf16* raw_hi, wd_bf16* raw_lo, const int32_t* perm_a,
                            void* stream) {
    if (!xa || !xb || !part_a || !part_b || !gamma || !beta || !out_hi || batch <= 0 || hw <= 0 || nchunk_a <= 0 || nchunk_b <= 0 ||
        part_cpg_a <= 0 || part_cpg_b <= 0)
        return WD_EINVAL;
    if (ca % 4 || cb % 4 || lda % 4 || ldb % 4 || out_ld % 4 || c_off_a % 4 || c_off_b % 4 || ca % cpg || cb % cpg ||
        ca / cpg > 32 || cb / cpg > 32 || cpg % part_cpg_a || cpg % part_cpg_b)
        return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_GNAPPLY, st);
    const GnSrc s0 = {xa, part_a, lda, ca, nchunk_a, part_cpg_a, c_off_a, perm_a}, s1 = {xb, part_b, ldb, cb, nchunk_b, part_cpg_b, c_off_b, nullptr};
    hipLaunchKernelGGL(gn_apply_kernel<>, dim3((hw + AP_TOK - 1) / AP_TOK, batch, 2), dim3(256), 0, st, s0, s1, hw, cpg, gamma, beta, eps,
                       silu, out_hi, out_lo, out_ld, raw_hi, raw_lo);
    return wd_check_launch();
}

extern "C" int wd_gn_conv3x3_few_supported(int c, int w, int oc) {
    return c > 0 && c % GC_CH == 0 && w > 0 && w <= 64 && oc >= 1 && oc <= 4;
}

extern "C" int wd_gn_conv3x3_few(const float* x, int ld, int batch, int h, int w, int c, int cpg, const double* part, int nchunk,
                                 int part_cpg, const float* gamma, const float* beta, float eps, int silu, const float* weight,
                                 const float* bias, int oc, float* out, void* stream) {
    if (!x || !part || !gamma || !beta || !weight || !out || batch <= 0 || h <= 0 || nchunk <= 0 || part_cpg <= 0) return WD_EINVAL;
    if (!wd_gn_conv3x3_few_supported(c, w, oc) || ld % 4 || cpg <= 0 || c % cpg || c / cpg > 32 || cpg % part_cpg) return WD_EINVAL;
    if ((h + GC_TR - 1) / GC_TR > 65535) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(gn_conv_few_kernel, dim3(batch, (w + GC_TC - 1) / GC_TC, (h + GC_TR - 1) / GC_TR), dim3(GC_NT), 0, st, x, ld, h,
                       w, c, cpg, nchunk, part_cpg, part, gamma, beta, eps, silu, weight, bias, oc, out);
    return wd_check_launch();
}

extern "C" int wd_layernorm(const float* x, int ld, int rows, int c, const float* gamma, const float* beta, float eps,
                            wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, void* stream) {
    if (!x || !gamma || !beta || !out_hi || rows <= 0 || c <= 0) return WD_EINVAL;
    if (c % 4 || ld % 4 || out_ld % 4 || c > 64 * 4 * LN_MAX4) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_LN, st);
    hipLaunchKernelGGL(layernorm_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, x, ld, rows, c, gamma, beta, eps,
                       out_hi, out_lo, out_ld);
    return wd_check_launch();
}

extern "C" int wd_split(const float* x, int ld, int rows, int c, int silu, wd_bf16* out_hi, wd_bf16* out_lo, int out_ld,
                        void* stream) {
    if (!x || !out_hi || rows <= 0 || c <= 0 || c % 4 || ld % 4 || out_ld % 4) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long total = (long)rows * (c / 4);
    const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(split_kernel, dim3(grid), dim3(256), 0, st, x, ld, rows, c, silu, out_hi, out_lo, out_ld);
    return wd_check_launch();
}
