// Line sampling (MultiDiffusion, Bar-Tal et al. 2023): a line latent [lines][c][h][wl] is denoised as K overlapping windows of
// the model's own width w.  wd_window_gather cuts the windows out of the line before the forward(s); wd_window_blend averages
// the K predicted noises back into one line-wide prediction, on which the sampler's ordinary update then runs.
#include "wd_common.h"

// The blend is compared bit for bit with its numpy specification (tests/_window_ref.py): every product and every sum is rounded
// to fp32 on its own - no mul+add contraction anywhere in this translation unit (plain operators, as in wd_misc.hip).
#pragma clang fp contract(off)

namespace {

inline int window_grid(long total) {
    long g = (total + 255) / 256;
    if (g < 1) g = 1;
    return (int)(g < 2048 ? g : 2048);
}

// win[b][ch][r][j] = line[s][ch][r][o + j], b = s * K + k, o = offsets[b]: the bits are copied.  One output element per lane
// (o is arbitrary: a window's rows are not 16-byte aligned in general).  A window that does not fit the line (o < 0 or
// o + w > wl) is absent: its rows are written 0 and the line is not read for it.
__global__ void window_gather_kernel(const float* __restrict__ line, const int32_t* __restrict__ offsets, int lines, int K, int c, int h,
                                     int w, int wl, float* __restrict__ win) {
    const long rows = (long)c * h;
    const long total = (long)lines * K * rows * w;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / w;  // (b, ch, r) flattened
        const int j = (int)(i - row * w);
        const long b = row / rows;
        const long cr = row - b * rows;
        const long s = b / K;
        const int o = offsets[b];
        const bool fits = o >= 0 && (long)o + w <= wl;
        win[i] = fits ? line[(s * rows + cr) * wl + o + j] : 0.0f;
    }
}

// Per line element (s, ch, r, J): the windows k = 0 .. K-1 in ascending order with o <= J < o + w (and o + w <= wl, o >= 0) and
// wn[s][k][J - o] != 0; the first sets acc = wn * e, each later one acc = acc + wn * e.  A window whose weight is 0 there is
// skipped - its prediction is not read, so a NaN in it does not spread - and an uncovered column gives 0.0f.  TWO: the second
// prediction of a guided step goes through the same weights into a line buffer of its own.
template <bool TWO>
__global__ void window_blend_kernel(const float* __restrict__ win0, const float* __restrict__ win1, const float* __restrict__ wn,
                                    const int32_t* __restrict__ offsets, int lines, int K, int c, int h, int w, int wl,
                                    float* __restrict__ line0, float* __restrict__ line1) {
    const long rows = (long)c * h;
    const long total = (long)lines * rows * wl;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / wl;  // (s, ch, r) flattened
        const int J = (int)(i - row * wl);
        const long s = row / rows;
        const long cr = row - s * rows;
        float acc0 = 0.0f, acc1 = 0.0f;
        bool first = true;
        for (int k = 0; k < K; ++k) {
            const long b = s * K + k;
            const int o = offsets[b];
            if (o < 0 || (long)o + w > wl || J < o || J >= o + w) continue;
            const float g = wn[b * w + (J - o)];
            if (g == 0.0f) continue;
            const long src = (b * rows + cr) * w + (J - o);
            const float p0 = g * win0[src];
            acc0 = first ? p0 : acc0 + p0;
            if (TWO) {
                const float p1 = g * win1[src];
                acc1 = first ? p1 : acc1 + p1;
            }
            first = false;
        }
        line0[i] = acc0;
        if (TWO) line1[i] = acc1;
    }
}

inline bool window_shape_ok(int lines, int K, int c, int h, int w, int wl) {
    return lines >= 1 && c >= 1 && h >= 1 && K >= 1 && K <= WD_WINDOW_MAX && w >= 1 && wl >= w &&
           (long)lines * K * c * h * (long)w <= 0x7fffffffL && (long)lines * c * h * (long)wl <= 0x7fffffffL;
}

}  // namespace

extern "C" int wd_window_gather(const float* line, const int32_t* offsets, int lines, int K, int c, int h, int w, int wl, float* win,
                                void* stream) {
    if (!line || !offsets || !win || !window_shape_ok(lines, K, c, h, w, wl)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(window_gather_kernel, dim3(window_grid((long)lines * K * c * h * w)), dim3(256), 0, st, line, offsets, lines, K, c,
                       h, w, wl, win);
    return wd_check_launch();
}

extern "C" int wd_window_blend(const float* win0, const float* win1, const float* wn, const int32_t* offsets, int lines, int K, int c,
                               int h, int w, int wl, float* line0, float* line1, void* stream) {
    if (!win0 || !wn || !offsets || !line0 || (win1 == nullptr) != (line1 == nullptr) || !window_shape_ok(lines, K, c, h, w, wl))
        return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    const dim3 grid(window_grid((long)lines * c * h * wl));
    if (win1)
        hipLaunchKernelGGL(window_blend_kernel<true>, grid, dim3(256), 0, st, win0, win1, wn, offsets, lines, K, c, h, w, wl, line0, line1);
    else
        hipLaunchKernelGGL(window_blend_kernel<false>, grid, dim3(256), 0, st, win0, (const float*)nullptr, wn, offsets, lines, K, c, h, w,
                           wl, line0, (float*)nullptr);
    return wd_check_launch();
}
