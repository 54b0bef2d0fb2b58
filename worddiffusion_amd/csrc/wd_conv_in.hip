// The UNet's first layer (unet.py:1251: conv 3x3, pad 1, in_channels <= 4 -> model_channels) as a direct fp32 convolution:
// x NCHW [B][cin][H][W] -> token-major fp32 rows [B*H*W][cout] + the GroupNorm statistics partials of the result.
// K = 9 * cin <= 36, so there is nothing to gather or pipeline: the cost is the store of the rows (1280 bytes each at 320
// channels).  One workgroup owns 64 consecutive tokens of one sample - one statistics chunk, the row panel of the GEMM this kernel
// replaces - and stages in LDS the sample (4 KB at 8 x 32) with its zero border, one float4 of input channels per pixel, and the
// weights as [ci * 9 + tap][cout] (read from the parameter in its own order, so the global reads are contiguous).
// thread = (token lane, output-channel quad): the quad's 4 x cin x 9 weights live in registers for the whole kernel (one 16-byte
// LDS read per (ci, tap)), a token costs nine 16-byte LDS reads (the same address across the lanes of a token lane: broadcasts)
// and 36 * cin FMAs, and consecutive lanes store consecutive 16-byte pieces of a token row.
// Statistics: part[b][chunk][cout / cpg][2] (sum, sum of squares) in fp64, the layout of wd_gemm's stat_part with 64-row panels.
// Every term is widened to fp64 before it is added or squared; a thread sums its tokens in order, then one thread per channel
// sums the token lanes and one thread per group the group's channels, each in a fixed order (no atomics: the same bits on every
// launch).
#include "wd_common.h"

namespace {

constexpr int CI_NT = 512;        // threads per workgroup
constexpr int CI_TOK = 64;        // tokens per workgroup = rows per statistics chunk
constexpr int CI_MAX_PIX = 2048;  // (H + 2) * (W + 2) pixels of a padded sample: 32 KB of LDS
constexpr int CI_WBATCH = 12;     // weight loads a thread has in flight while the weights are staged
constexpr int CI_WPAD = 4;        // floats between the weight rows of two (ci, tap): spreads the banks of the transposing writes

// bytes of LDS behind the sample: the weights, reused for the statistics once they are in registers
__host__ __device__ inline size_t ci_scratch_bytes(int cin, int cout, bool stats) {
    const size_t wb = (size_t)cin * 9 * (cout + CI_WPAD) * sizeof(float);
    const size_t sb = stats ? ((size_t)(CI_NT / (cout / 4)) * cout + cout) * 2 * sizeof(double) : 0;
    return wb > sb ? wb : sb;
}

template <int CIN>
__global__ void __launch_bounds__(CI_NT) conv3x3_in_kernel(const float* __restrict__ x, int H, int W, const float* __restrict__ w,
                                                          const float* __restrict__ bias, int cout, float* __restrict__ out, int ld,
                                                          double* __restrict__ part, int cpg) {
    constexpr int K = CIN * 9;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4* s_x = reinterpret_cast<float4*>(smem);                      // [H + 2][W + 2]: channels 0..3 of a pixel (0 from cin on)
    float* s_w = reinterpret_cast<float*>(s_x + (H + 2) * (W + 2));    // [K][cout + CI_WPAD]
    double* s_st = reinterpret_cast<double*>(s_w);                      // later: [token lane][cout][2], then [cout][2]
    const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int hw = H * W, pw = W + 2, wp = cout + CI_WPAD;
    for (int i = tid; i < (H + 2) * pw; i += CI_NT) {
        const int yy = i / pw - 1, xx = i % pw - 1;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) v[ci] = x[(((long)b * CIN + ci) * H + yy) * W + xx];
        }
        s_x[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
    // w[co][ci][tap] = w[co * K + k] -> s_w[k][co], twelve loads of a thread in flight at a time (one load per trip of a plain
    // loop waits a full L2 round trip per element: 23 of them at 320 channels)
    for (int i0 = 0; i0 < cout * K; i0 += CI_NT * CI_WBATCH) {
        float v[CI_WBATCH];
#pragma unroll
        for (int u = 0; u < CI_WBATCH; ++u) v[u] = w[min(i0 + u * CI_NT + tid, cout * K - 1)];
#pragma unroll
        for (int u = 0; u < CI_WBATCH; ++u) {
            const int i = i0 + u * CI_NT + tid, co = i / K, k = i - co * K;
            if (i < cout * K) s_w[k * wp + co] = v[u];
        }
    }
    const int nq = cout >> 2, ntl = CI_NT / nq;  // channel quads, token lanes
    const int tl = tid / nq, q = tid - tl * nq;
    const bool active = tl < ntl;
    __syncthreads();
    float4 wr[K], bs = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) {
#pragma unroll
        for (int k = 0; k < K; ++k) wr[k] = *reinterpret_cast<const float4*>(s_w + k * wp + 4 * q);
        if (bias) bs = make_float4(bias[4 * q], bias[4 * q + 1], bias[4 * q + 2], bias[4 * q + 3]);
    }
    const int t0 = chunk * CI_TOK, nt = min(CI_TOK, hw - t0);
    double su[4] = {0.0, 0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
        for (int t = tl; t < nt; t += ntl) {
            const int p = t0 + t, y = p / W, xx = p - y * W;
            const float4* px = s_x + y * pw + xx;  // the pixel above and to the left: tap (dy, dx) is px[dy * pw + dx]
            float acc[4] = {bs.x, bs.y, bs.z, bs.w};
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const float4 a4 = px[(tap / 3) * pw + tap % 3];
                const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci) {
                    const float4 w4 = wr[ci * 9 + tap];
                    acc[0] += w4.x * a[ci]; acc[1] += w4.y * a[ci]; acc[2] += w4.z * a[ci]; acc[3] += w4.w * a[ci];
                }
            }
            *reinterpret_cast<float4*>(out + ((long)b * hw + p) * ld + 4 * q) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            if (part) {
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const double d = (double)acc[o];
                    su[o] += d;
                    sq[o] += d * d;
                }
            }
        }
    }
    if (!part) return;
    __syncthreads();  // every thread has its weights in registers: their LDS becomes the statistics scratch
    if (active) {
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            s_st[((long)tl * cout + 4 * q + o) * 2] = su[o];
            s_st[((long)tl * cout + 4 * q + o) * 2 + 1] = sq[o];
        }
    }
    __syncthreads();
    double* s_ch = s_st + (long)ntl * cout * 2;  // [cout][2]: a channel's sums over the token lanes
    for (int ch = tid; ch < cout; ch += CI_NT) {
        double ds = 0.0, dq = 0.0;
        for (int l = 0; l < ntl; ++l) {
            ds += s_st[((long)l * cout + ch) * 2];
            dq += s_st[((long)l * cout + ch) * 2 + 1];
        }
        s_ch[2 * ch] = ds;
        s_ch[2 * ch + 1] = dq;
    }
    __syncthreads();
    const int ng = cout / cpg;
    for (int g = tid; g < ng; g += CI_NT) {
        double ds = 0.0, dq = 0.0;
        for (int k = 0; k < cpg; ++k) {
            ds += s_ch[2 * (g * cpg + k)];
            dq += s_ch[2 * (g * cpg + k) + 1];
        }
        double* o = part + (((long)b * gridDim.x + chunk) * ng + g) * 2;
        o[0] = ds;
        o[1] = dq;
    }
}

}  // namespace

extern "C" int wd_conv3x3_in_nchunk(int hw) { return (hw + CI_TOK - 1) / CI_TOK; }

extern "C" int wd_conv3x3_in_supported(int cin, int h, int w, int cout) {
    return cin >= 1 && cin <= 4 && h > 0 && w > 0 && w <= 64 && (long)(h + 2) * (w + 2) <= CI_MAX_PIX && cout >= 4 && cout % 4 == 0 &&
           cout / 4 <= CI_NT && (size_t)(h + 2) * (w + 2) * sizeof(float4) + ci_scratch_bytes(cin, cout, true) <= 64 * 1024;
}

extern "C" int wd_conv3x3_in(const float* x, int batch, int cin, int h, int w, const float* weight, const float* bias, int cout,
                             float* out, int ld, double* part, int stat_cpg, void* stream) {
    if (!x || !weight || !out || batch <= 0 || batch > 65535 || !wd_conv3x3_in_supported(cin, h, w, cout)) return WD_EINVAL;
    if (ld < cout || ld % 4) return WD_EINVAL;
    if (part && (stat_cpg <= 0 || cout % stat_cpg)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t smem = (size_t)(h + 2) * (w + 2) * sizeof(float4) + ci_scratch_bytes(cin, cout, part != nullptr);  // <= 64 KB
    const dim3 grid(wd_conv3x3_in_nchunk(h * w), batch);
    WdLaunchScope scope(WD_CLS_OTHER, st, 2.0 * batch * h * w * (double)cout * 9 * cin);
#define WD_CI_LAUNCH(CIN) \
    hipLaunchKernelGGL(conv3x3_in_kernel<CIN>, grid, dim3(CI_NT), smem, st, x, h, w, weight, bias, cout, out, ld, part, stat_cpg)
    switch (cin) {
        case 1: WD_CI_LAUNCH(1); break;
        case 2: WD_CI_LAUNCH(2); break;
        case 3: WD_CI_LAUNCH(3); break;
        default: WD_CI_LAUNCH(4); break;
    }
#undef WD_CI_LAUNCH
    return wd_check_launch();
}
