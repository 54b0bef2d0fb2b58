// The streaming stages of the PHOSCnet word recogniser (ResPhoSCNetZSL/modules/models.py:15-80) between its GEMMs, and the
// zero-shot scoring behind it (modules/engine.py:130-146):
//   wd_relu_pool_planes  nn.ReLU (+ nn.MaxPool2d 2x2 / 2) of a GEMM's fp32 result -> the next GEMM's split-bf16 operand planes
//   wd_tpp_max           nn.ReLU + TemporalPyramidPooling (pyramidpooling.py:88-113) of the last convolution -> the 4096 features
//   wd_resize_bilinear   cv2.resize(INTER_LINEAR) / F.interpolate(bilinear, align_corners=False) of the input images
//   wd_phosc_finish      relu(phos) | sigmoid(phoc) -> the 769-vector
//   wd_phosc_score       cosine of the predictions against a lexicon table, first maximum, score of a given word
// All are memory-bound: plain C++, a grid-stride loop under the grid cap of wd_misc.hip, 16-byte loads and 8-byte plane stores
// where pitches and addresses allow (VEC), the element path otherwise (same values).  No ReLU ever enters wd_gemm's epilogue.
#include "wd_common.h"

// wd_resize_bilinear is compared bit for bit with its numpy specification (tests/_phoscnet_ref.py): every product, sum and
// difference is rounded to fp32 on its own - no mul+add contraction anywhere in this translation unit (plain operators, as in
// wd_misc.hip); the dot products of wd_phosc_score ask for their fused multiply-adds by name (fmaf).
#pragma clang fp contract(off)

namespace {

inline int pn_grid(long total, int block = 256) {  // (wd_misc.hip grid_for: at most 2048 workgroups, the loop strides)
    long g = (total + block - 1) / block;
    if (g < 1) g = 1;
    return (int)(g < 2048 ? g : 2048);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

__device__ __forceinline__ float relu0(float m) { return m > 0.0f ? m : 0.0f; }  // (-0 and everything below: +0)
__device__ __forceinline__ float max_gt(float m, float v) { return v > m ? v : m; }

// ---- ReLU (+ 2x2 / 2 max pool) -> planes ---------------------------------------------------------------------------------
template <bool VEC>
__global__ void relu_pool_kernel(const float* __restrict__ x, int ld_in, int batch, int h, int w, int c, int pool,
                                 wd_bf16* __restrict__ out_hi, wd_bf16* __restrict__ out_lo, int ld_out) {
    constexpr int E = VEC ? 4 : 1;
    const int cq = c / E;
    const int ho = pool == 2 ? h / 2 : h, wo = pool == 2 ? w / 2 : w;
    const long hwo = (long)ho * wo;
    const long total = (long)batch * hwo * cq;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cq;  // output row
        const int cx = (int)(i - r * cq) * E;
        const long b = r / hwo;
        const long p = r - b * hwo;
        const int yo = (int)(p / wo), xo = (int)(p - (long)yo * wo);
        const long src = (b * h + (long)yo * pool) * w + (long)xo * pool;  // source row of the window's first pixel
        const float* s0 = x + src * ld_in + cx;
        if (VEC) {
            float4 v = *reinterpret_cast<const float4*>(s0);
            if (pool == 2) {
                const float4 v1 = *reinterpret_cast<const float4*>(s0 + ld_in);
                const float4 v2 = *reinterpret_cast<const float4*>(s0 + (long)w * ld_in);
                const float4 v3 = *reinterpret_cast<const float4*>(s0 + ((long)w + 1) * ld_in);
                v.x = max_gt(max_gt(max_gt(v.x, v1.x), v2.x), v3.x);
                v.y = max_gt(max_gt(max_gt(v.y, v1.y), v2.y), v3.y);
                v.z = max_gt(max_gt(max_gt(v.z, v1.z), v2.z), v3.z);
                v.w = max_gt(max_gt(max_gt(v.w, v1.w), v2.w), v3.w);
            }
            v.x = relu0(v.x); v.y = relu0(v.y); v.z = relu0(v.z); v.w = relu0(v.w);
            uint2 hv, lv;
            wd_split4(v, hv, lv);
            *reinterpret_cast<uint2*>(out_hi + r * ld_out + cx) = hv;
            if (out_lo) *reinterpret_cast<uint2*>(out_lo + r * ld_out + cx) = lv;
        } else {
            float v = s0[0];
            if (pool == 2) v = max_gt(max_gt(max_gt(v, s0[ld_in]), s0[(long)w * ld_in]), s0[((long)w + 1) * ld_in]);
            v = relu0(v);
            uint32_t hb, lb;
            wd_split1(v, hb, lb);
            out_hi[r * ld_out + cx] = (wd_bf16)hb;
            if (out_lo) out_lo[r * ld_out + cx] = (wd_bf16)lb;
        }
    }
}

// ---- ReLU + temporal pyramid max pooling ---------------------------------------------------------------------------------
struct TppLevels {
    int n;
    int bins[WD_TPP_MAX_LEVELS];
};

// A work item = (sample, bin of some level, run of 64 channel units); a unit is 4 channels (VEC) or 1.  The 256 threads are 64
// units x 4 slices of the bin's h x k window; the slices meet in LDS (a maximum: exact in any order).
template <bool VEC>
__global__ void __launch_bounds__(256) tpp_max_kernel(const float* __restrict__ x, int ld, int batch, int h, int w, int c, TppLevels lv,
                                                       float* __restrict__ out_f32, int ld_out, wd_bf16* __restrict__ out_hi,
                                                       wd_bf16* __restrict__ out_lo, int ld_pl) {
    constexpr int E = VEC ? 4 : 1;
    __shared__ float red[4][64 * E];
    const int units = c / E;
    const int nrun = (units + 63) / 64;
    int nbins = 0;
    for (int i = 0; i < lv.n; ++i) nbins += lv.bins[i];
    const long items = (long)batch * nbins * nrun;
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const int run = (int)(item % nrun);
        const long bb = item / nrun;
        int bin = (int)(bb % nbins);
        const long b = bb / nbins;
        int L = lv.bins[0];
        long off = 0;  // first output column of the level
        for (int i = 0; i < lv.n; ++i) {
            L = lv.bins[i];
            if (bin < L) break;
            bin -= L;
            off += (long)c * L;
        }
        const int k = (w + L - 1) / L;
        const int left = (k * L - w) / 2;
        int x0 = bin * k - left, x1 = x0 + k;  // the bin's columns of the unpadded map
        if (x0 < 0) x0 = 0;
        if (x1 > w) x1 = w;
        const int nv = x1 > x0 ? x1 - x0 : 0;
        const int npos = h * nv;
        const int u = run * 64 + lane;
        float m[E];
        for (int e = 0; e < E; ++e) m[e] = 0.0f;  // (the ReLU's floor; what a bin of padding only yields)
        if (u < units) {
            const float* base = x + (b * h * w) * ld + (long)u * E;
            for (int q = slice; q < npos; q += 4) {
                const int yy = q / nv, xx = x0 + (q - yy * nv);
                const float* s = base + ((long)yy * w + xx) * ld;
                if constexpr (VEC) {
                    const float4 v = *reinterpret_cast<const float4*>(s);
                    m[0] = max_gt(m[0], v.x);
                    m[1] = max_gt(m[1], v.y);
                    m[2] = max_gt(m[2], v.z);
                    m[3] = max_gt(m[3], v.w);
                } else {
                    m[0] = max_gt(m[0], s[0]);
                }
            }
        }
        for (int e = 0; e < E; ++e) red[slice][lane * E + e] = m[e];
        __syncthreads();
        if (slice == 0 && u < units) {
            for (int e = 0; e < E; ++e) {
                float v = red[0][lane * E + e];
                v = max_gt(v, red[1][lane * E + e]);
                v = max_gt(v, red[2][lane * E + e]);
                v = max_gt(v, red[3][lane * E + e]);
                const long o = off + (long)(u * E + e) * L + bin;
                if (out_f32) out_f32[b * ld_out + o] = v;
                if (out_hi) {
                    uint32_t hb, lb;
                    wd_split1(v, hb, lb);
                    out_hi[b * ld_pl + o] = (wd_bf16)hb;
                    if (out_lo) out_lo[b * ld_pl + o] = (wd_bf16)lb;
                }
            }
        }
        __syncthreads();
    }
}

// ---- bilinear resize -----------------------------------------------------------------------------------------------------
struct Tap {
    int i0, i1;
    float l;
};
// source coordinate (dst + 0.5) * nsrc / ndst - 0.5 = n / (2 ndst) with n = (2 dst + 1) nsrc - ndst in integers: the pixel index is
// exact and the weight is ONE fp32 division of two exact integers (a coordinate formed in fp32 is off by half an ulp of 256 at
// the right edge of a 256-pixel image, 1.5e-5 of a pixel)
__device__ __forceinline__ Tap resize_tap(int dst, int ndst, int nsrc) {
    long n = (2L * dst + 1) * nsrc - ndst;
    if (n < 0) n = 0;
    const long den = 2L * ndst;
    const int i0 = (int)(n / den);  // (< nsrc: n < 2 ndst nsrc)
    Tap t;
    t.i0 = i0;
    t.i1 = i0 + 1 < nsrc ? i0 + 1 : nsrc - 1;
    t.l = (float)(n - i0 * den) / (float)den;
    return t;
}
__device__ __forceinline__ float resize_px(const float* __restrict__ r0, const float* __restrict__ r1, const Tap tx, const Tap ty) {
    const float wx = 1.0f - tx.l, wy = 1.0f - ty.l;
    const float top = wx * r0[tx.i0] + tx.l * r0[tx.i1];
    const float bot = wx * r1[tx.i0] + tx.l * r1[tx.i1];
    return wy * top + ty.l * bot;
}

template <bool VEC>
__global__ void resize_kernel(const float* __restrict__ x, int ld_in, int batch, int c, int hs, int ws, float* __restrict__ out,
                              int ld_out, int h, int w, int bgr) {
    constexpr int E = VEC ? 4 : 1;
    const int wq = w / E;
    const long total = (long)batch * c * h * wq;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / wq;  // output row over all planes
        const int xo = (int)(i - row * wq) * E;
        const long plane = row / h;
        const int y = (int)(row - plane * h);
        const long b = plane / c;
        const int ch = (int)(plane - b * c);
        const long splane = b * c + (bgr ? c - 1 - ch : ch);
        const Tap ty = resize_tap(y, h, hs);
        const float* r0 = x + (splane * hs + ty.i0) * ld_in;
        const float* r1 = x + (splane * hs + ty.i1) * ld_in;
        float* o = out + row * ld_out + xo;
        if (VEC) {
            float4 v;
            v.x = resize_px(r0, r1, resize_tap(xo, w, ws), ty);
            v.y = resize_px(r0, r1, resize_tap(xo + 1, w, ws), ty);
            v.z = resize_px(r0, r1, resize_tap(xo + 2, w, ws), ty);
            v.w = resize_px(r0, r1, resize_tap(xo + 3, w, ws), ty);
            *reinterpret_cast<float4*>(o) = v;
        } else {
            o[0] = resize_px(r0, r1, resize_tap(xo, w, ws), ty);
        }
    }
}

// ---- relu(phos) | sigmoid(phoc) ------------------------------------------------------------------------------------------
__global__ void phosc_finish_kernel(const float* __restrict__ phos, int ld_phos, int n_phos, const float* __restrict__ phoc, int ld_phoc,
                                    int n_phoc, int batch, float* __restrict__ out, int ld_out) {
    const int n = n_phos + n_phoc;
    const long total = (long)batch * n;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long b = i / n;
        const int j = (int)(i - b * n);
        float v;
        if (j < n_phos) v = relu0(phos[b * ld_phos + j]);
        else v = 1.0f / (1.0f + expf(-phoc[b * ld_phoc + (j - n_phos)]));
        out[b * ld_out + j] = v;
    }
}

// ---- cosine scores against a lexicon -------------------------------------------------------------------------------------
// A work item = (sample, block of 64 words): the workgroup sums |x|^2 once, then each of its 4 waves takes 16 words, one at a time,
// lanes striding over the row (16 bytes per lane on the VEC path, the d % 4 tail on the first lanes).
template <bool VEC>
__global__ void __launch_bounds__(256) phosc_score_kernel(const float* __restrict__ pred, int ld_pred, int batch, int d,
                                                           const float* __restrict__ table, int ld_table,
                                                           const float* __restrict__ table_norm, int v, float* __restrict__ sc, int ld_sc) {
    __shared__ float part[4];
    const int nblk = (v + 63) / 64;
    const long items = (long)batch * nblk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int d4 = VEC ? d / 4 : 0;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long b = item / nblk;
        const int wb = (int)(item - b * nblk);
        const float* xr = pred + b * ld_pred;
        float s = 0.0f;
        for (int j = threadIdx.x; j < d; j += 256) s = fmaf(xr[j], xr[j], s);
        s = wd_wave_sum(s);
        if (lane == 0) part[wave] = s;
        __syncthreads();
        const float xn = sqrtf((part[0] + part[1]) + (part[2] + part[3]));
        for (int t = 0; t < 16; ++t) {
            const int word = wb * 64 + wave * 16 + t;
            if (word >= v) break;  // (wave-uniform)
            const float* yr = table + (long)word * ld_table;
            float dot = 0.0f;
            if (VEC) {
                for (int q = lane; q < d4; q += 64) {
                    const float4 a = *reinterpret_cast<const float4*>(xr + 4 * q);
                    const float4 y = *reinterpret_cast<const float4*>(yr + 4 * q);
                    dot = fmaf(a.x, y.x, dot);
                    dot = fmaf(a.y, y.y, dot);
                    dot = fmaf(a.z, y.z, dot);
                    dot = fmaf(a.w, y.w, dot);
                }
                const int j = 4 * d4 + lane;
                if (j < d) dot = fmaf(xr[j], yr[j], dot);
            } else {
                for (int j = lane; j < d; j += 64) dot = fmaf(xr[j], yr[j], dot);
            }
            dot = wd_wave_sum(dot);
            if (lane == 0) sc[b * ld_sc + word] = dot / fmaxf(xn * table_norm[word], 1e-8f);
        }
        __syncthreads();  // (part is rewritten by the next item)
    }
}

// first maximum of a sample's scores + the score of its target word: one workgroup per sample
__global__ void __launch_bounds__(256) phosc_best_kernel(const float* __restrict__ sc, int ld_sc, int batch, int v,
                                                          int32_t* __restrict__ best_idx, float* __restrict__ best_score,
                                                          const int32_t* __restrict__ target_idx, float* __restrict__ target_score) {
    __shared__ float bs[256];
    __shared__ int bi[256];
    for (long b = blockIdx.x; b < batch; b += gridDim.x) {
        const float* r = sc + b * ld_sc;
        if (best_idx || best_score) {
            float m = -INFINITY;
            int mi = 0x7fffffff;
            for (int j = threadIdx.x; j < v; j += 256) {
                const float s = r[j];
                if (s > m || mi == 0x7fffffff) m = s, mi = j;  // strict >: the first of equal scores in this thread's stride
            }
            bs[threadIdx.x] = m;
            bi[threadIdx.x] = mi;
            __syncthreads();
            for (int step = 128; step > 0; step >>= 1) {
                if ((int)threadIdx.x < step) {
                    const float m2 = bs[threadIdx.x + step];
                    const int i2 = bi[threadIdx.x + step];
                    const float m1 = bs[threadIdx.x];
                    const int i1 = bi[threadIdx.x];
                    if (i2 != 0x7fffffff && (i1 == 0x7fffffff || m2 > m1 || (m2 == m1 && i2 < i1))) bs[threadIdx.x] = m2, bi[threadIdx.x] = i2;
                }
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                if (best_idx) best_idx[b] = bi[0];
                if (best_score) best_score[b] = bs[0];
            }
            __syncthreads();
        }
        if (target_score && threadIdx.x == 0) {
            const int t = target_idx[b];
            target_score[b] = (t >= 0 && t < v) ? r[t] : __uint_as_float(0x7fc00000u);
        }
    }
}

}  // namespace

extern "C" int wd_relu_pool_planes(const float* x, int ld_in, int batch, int h, int w, int c, int pool, wd_bf16* out_hi, wd_bf16* out_lo,
                                   int ld_out, void* stream) {
    if (!x || !out_hi || batch <= 0 || h <= 0 || w <= 0 || c <= 0 || (pool != 1 && pool != 2)) return WD_EINVAL;
    if (pool == 2 && (h < 2 || w < 2)) return WD_EINVAL;
    if (ld_in < c || ld_out < c) return WD_EINVAL;
    const int ho = pool == 2 ? h / 2 : h, wo = pool == 2 ? w / 2 : w;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool vec = c % 4 == 0 && ld_in % 4 == 0 && ld_out % 4 == 0 && al16(x) && al8(out_hi) && al8(out_lo);
    const long total = (long)batch * ho * wo * (vec ? c / 4 : c);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    if (vec)
        hipLaunchKernelGGL(relu_pool_kernel<true>, dim3(pn_grid(total)), dim3(256), 0, st, x, ld_in, batch, h, w, c, pool, out_hi, out_lo,
                           ld_out);
    else
        hipLaunchKernelGGL(relu_pool_kernel<false>, dim3(pn_grid(total)), dim3(256), 0, st, x, ld_in, batch, h, w, c, pool, out_hi, out_lo,
                           ld_out);
    return wd_check_launch();
}

extern "C" int wd_tpp_max(const float* x, int ld, int batch, int h, int w, int c, const int32_t* levels, int nlevels, float* out_f32,
                          int ld_out, wd_bf16* out_hi, wd_bf16* out_lo, int ld_pl, void* stream) {
    if (!x || !levels || (!out_f32 && !out_hi) || (out_lo && !out_hi) || batch <= 0 || h <= 0 || w <= 0 || c <= 0 || ld < c) return WD_EINVAL;
    if (nlevels < 1 || nlevels > WD_TPP_MAX_LEVELS) return WD_EINVAL;
    TppLevels lv;
    lv.n = nlevels;
    long nbins = 0;
    for (int i = 0; i < WD_TPP_MAX_LEVELS; ++i) {
        lv.bins[i] = i < nlevels ? levels[i] : 0;
        if (i < nlevels && (levels[i] < 1 || levels[i] > WD_TPP_MAX_BINS)) return WD_EINVAL;
        nbins += lv.bins[i];
    }
    const long ncol = nbins * c;
    if ((out_f32 && ld_out < ncol) || (out_hi && ld_pl < ncol)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool vec = c % 4 == 0 && ld % 4 == 0 && al16(x);
    const int units = vec ? c / 4 : c;
    const long items = (long)batch * nbins * ((units + 63) / 64);
    const int grid = (int)(items < 2048 ? items : 2048);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    if (vec)
        hipLaunchKernelGGL(tpp_max_kernel<true>, dim3(grid), dim3(256), 0, st, x, ld, batch, h, w, c, lv, out_f32, ld_out, out_hi, out_lo,
                           ld_pl);
    else
        hipLaunchKernelGGL(tpp_max_kernel<false>, dim3(grid), dim3(256), 0, st, x, ld, batch, h, w, c, lv, out_f32, ld_out, out_hi, out_lo,
                           ld_pl);
    return wd_check_launch();
}

extern "C" int wd_resize_bilinear(const float* x, int ld_in, int batch, int c, int hs, int ws, float* out, int ld_out, int h, int w,
                                  int bgr, void* stream) {
    if (!x || !out || batch <= 0 || c <= 0 || hs <= 0 || ws <= 0 || h <= 0 || w <= 0 || ld_in < ws || ld_out < w) return WD_EINVAL;
    if (hs >= (1 << 23) || ws >= (1 << 23) || h >= (1 << 23) || w >= (1 << 23)) return WD_EINVAL;  // (2 * size is exact in fp32)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool vec = w % 4 == 0 && ld_out % 4 == 0 && al16(out);
    const long total = (long)batch * c * h * (vec ? w / 4 : w);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    if (vec)
        hipLaunchKernelGGL(resize_kernel<true>, dim3(pn_grid(total)), dim3(256), 0, st, x, ld_in, batch, c, hs, ws, out, ld_out, h, w, bgr);
    else
        hipLaunchKernelGGL(resize_kernel<false>, dim3(pn_grid(total)), dim3(256), 0, st, x, ld_in, batch, c, hs, ws, out, ld_out, h, w, bgr);
    return wd_check_launch();
}

extern "C" int wd_phosc_finish(const float* phos, int ld_phos, int n_phos, const float* phoc, int ld_phoc, int n_phoc, int batch,
                               float* out, int ld_out, void* stream) {
    if (!phos || !phoc || !out || batch <= 0 || n_phos <= 0 || n_phoc <= 0) return WD_EINVAL;
    if (ld_phos < n_phos || ld_phoc < n_phoc || ld_out < n_phos + n_phoc) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(phosc_finish_kernel, dim3(pn_grid((long)batch * (n_phos + n_phoc))), dim3(256), 0, st, phos, ld_phos, n_phos, phoc,
                       ld_phoc, n_phoc, batch, out, ld_out);
    return wd_check_launch();
}

extern "C" int wd_phosc_score(const float* pred, int ld_pred, int batch, int d, const float* table, int ld_table, const float* table_norm,
                              int v, float* scores, int ld_scores, int32_t* best_idx, float* best_score, const int32_t* target_idx,
                              float* target_score, float* ws, void* stream) {
    if (!pred || !table || !table_norm || batch <= 0 || d <= 0 || v <= 0 || ld_pred < d || ld_table < d) return WD_EINVAL;
    const bool second = best_idx || best_score || target_score;
    if (!scores && !second) return WD_EINVAL;
    if (target_score && !target_idx) return WD_EINVAL;
    if (scores && ld_scores < v) return WD_EINVAL;
    if (!scores && !ws) return WD_EINVAL;
    float* sc = scores ? scores : ws;
    const int ld_sc = scores ? ld_scores : v;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool vec = ld_pred % 4 == 0 && ld_table % 4 == 0 && al16(pred) && al16(table);
    const long items = (long)batch * ((v + 63) / 64);
    const int grid = (int)(items < 2048 ? items : 2048);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    if (vec)
        hipLaunchKernelGGL(phosc_score_kernel<true>, dim3(grid), dim3(256), 0, st, pred, ld_pred, batch, d, table, ld_table, table_norm, v,
                           sc, ld_sc);
    else
        hipLaunchKernelGGL(phosc_score_kernel<false>, dim3(grid), dim3(256), 0, st, pred, ld_pred, batch, d, table, ld_table, table_norm, v,
                           sc, ld_sc);
    int rc = wd_check_launch();
    if (rc != WD_OK || !second) return rc;
    hipLaunchKernelGGL(phosc_best_kernel, dim3(batch < 2048 ? batch : 2048), dim3(256), 0, st, sc, ld_sc, batch, v, best_idx, best_score,
                       target_idx, target_score);
    return wd_check_launch();
}
