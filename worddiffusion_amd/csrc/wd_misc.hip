// Small kernels at the edges of the UNet forward and the DDPM loop around it.
// Reference: timestep_embedding unet.py:96-116; CharacterEncoder embedding + PE unet.py:860-872;
// first conv unet.py:1251; Diffusion.sampling update train.py:229-236; noise_images train.py:190-194;
// EMA train.py:151-159.
#include "wd_common.h"
#include "wd_philox.h"

// The DDPM update, noise_images and the EMA are compared bit-for-bit with the reference's unfused fp32 torch ops:
// no mul+add contraction anywhere in this translation unit.  (Plain operators are used on purpose: the header
// intrinsics __fmul_rn/__fadd_rn are inline functions parsed with contraction allowed and fuse after inlining.)
#pragma clang fp contract(off)

namespace {

__global__ void temb_kernel(const int64_t* __restrict__ t, int batch, const float* __restrict__ freqs, int half,
                            wd_bf16* __restrict__ out_hi, wd_bf16* __restrict__ out_lo, int out_ld) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch * half) return;
    const int b = i / half, kx = i - b * half;
    const float arg = (float)t[b] * freqs[kx];
    const float c = cosf(arg), s = sinf(arg);
    uint32_t h, l;
    wd_split1(c, h, l);
    out_hi[(long)b * out_ld + kx] = (wd_bf16)h;
    if (out_lo) out_lo[(long)b * out_ld + kx] = (wd_bf16)l;
    wd_split1(s, h, l);
    out_hi[(long)b * out_ld + half + kx] = (wd_bf16)h;
    if (out_lo) out_lo[(long)b * out_ld + half + kx] = (wd_bf16)l;
}

__global__ void embed_kernel(const void* __restrict__ ids, int i64, int rows, int seq_len,
                             const float* __restrict__ table, int vocab, int c, const float* __restrict__ pe,
                             wd_bf16* __restrict__ out_hi, wd_bf16* __restrict__ out_lo, int out_ld) {
    const int c4 = c >> 2;
    const long total = (long)rows * c4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int r = (int)(i / c4), cx = (int)(i - (long)r * c4) * 4;
        long id = i64 ? (long)reinterpret_cast<const int64_t*>(ids)[r] : (long)reinterpret_cast<const int32_t*>(ids)[r];
        if (id < 0) id = 0;
        if (id >= vocab) id = vocab - 1;  // the reference would raise; never hit with valid ids
        float4 v = *reinterpret_cast<const float4*>(table + id * c + cx);
        if (pe) {
            const float4 p = *reinterpret_cast<const float4*>(pe + (long)(r % seq_len) * c + cx);
            v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
        uint2 h, l;
        wd_split4(v, h, l);
        *reinterpret_cast<uint2*>(out_hi + (long)r * out_ld + cx) = h;
        if (out_lo) *reinterpret_cast<uint2*>(out_lo + (long)r * out_ld + cx) = l;
    }
}

__global__ void im2col_kernel(const float* __restrict__ x, int batch, int cin, int h, int w,
                              wd_bf16* __restrict__ out_hi, wd_bf16* __restrict__ out_lo, int kpad) {
    const long total = (long)batch * h * w * kpad;
    const int hw = h * w;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / kpad;
        const int col = (int)(i - row * kpad);
        float v = 0.0f;
        if (col < 9 * cin) {
            const int tap = col / cin, ci = col - tap * cin;
            const int b = (int)(row / hw), p = (int)(row - (long)b * hw);
            const int yy = p / w + tap / 3 - 1, xx = p % w + tap % 3 - 1;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w) v = x[(((long)b * cin + ci) * h + yy) * w + xx];
        }
        uint32_t hb, lb;
        wd_split1(v, hb, lb);
        out_hi[i] = (wd_bf16)hb;
        if (out_lo) out_lo[i] = (wd_bf16)lb;
    }
}

__global__ void nchw_to_tok_kernel(const float* __restrict__ x, int batch, int c, int hw, float* __restrict__ out,
                                   int ld) {
    const long total = (long)batch * c * hw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / c;  // iterate output-major: row = b*hw + p, channel fastest
        const int ch = (int)(i - row * c);
        const int b = (int)(row / hw), p = (int)(row - (long)b * hw);
        out[row * ld + ch] = x[((long)b * c + ch) * hw + p];
    }
}

__global__ void tok_to_nchw_kernel(const float* __restrict__ x, int ld, int batch, int c, int hw,
                                   float* __restrict__ out) {
    const long total = (long)batch * c * hw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int p = (int)(i % hw);
        const long bc = i / hw;
        const int ch = (int)(bc % c), b = (int)(bc / c);
        out[i] = x[((long)b * hw + p) * ld + ch];
    }
}

// ---- normal draws from Philox4x32-10: philox_normal4 (wd_philox.h) -----------------------------------
// x = ca[t] * (x - cb[t] * eps) + cs[t] * z  with the reference's rounding order (no contraction)
__global__ void ddpm_step_kernel(float* __restrict__ x, const float* __restrict__ eps, int batch, int n4,
                                 const float* __restrict__ ca, const float* __restrict__ cb,
                                 const float* __restrict__ cs, const int32_t* __restrict__ t_dev,
                                 const float* __restrict__ noise, uint64_t seed, uint64_t sample_offset) {
    const int t = *t_dev;
    const float a = ca[t], bb = cb[t], s = cs[t];
    const long total = (long)batch * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / n4);
        const uint32_t e4 = (uint32_t)(i - (long)b * n4);
        float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t > 1) {
            if (noise) z = reinterpret_cast<const float4*>(noise)[i];
            else z = philox_normal4(seed, sample_offset + (uint64_t)b, (uint32_t)t, e4);
        }
        const float4 xv = reinterpret_cast<const float4*>(x)[i];
        const float4 ev = reinterpret_cast<const float4*>(eps)[i];
        float4 o;
        o.x = a * (xv.x - bb * ev.x) + s * z.x;
        o.y = a * (xv.y - bb * ev.y) + s * z.y;
        o.z = a * (xv.z - bb * ev.z) + s * z.z;
        o.w = a * (xv.w - bb * ev.w) + s * z.w;
        reinterpret_cast<float4*>(x)[i] = o;
    }
}

__global__ void advance_kernel(int32_t* t_dev, int delta, int64_t* t64, int batch) {
    __shared__ int tn;
    if (threadIdx.x == 0) {
        tn = *t_dev + delta;
        if (tn < 0) tn = 0;  // index 0 of the schedule is never used (train.py:221); never step below it
    }
    __syncthreads();
    const int v = tn;
    for (int b = threadIdx.x; b < batch; b += blockDim.x) t64[b] = (int64_t)v;
    __syncthreads();
    if (threadIdx.x == 0) *t_dev = v;
}

__global__ void randn_kernel(float* __restrict__ out, int batch, int n4, uint64_t seed, uint64_t sample_offset,
                             uint32_t tag) {
    const long total = (long)batch * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / n4);
        reinterpret_cast<float4*>(out)[i] =
            philox_normal4(seed, sample_offset + (uint64_t)b, tag, (uint32_t)(i - (long)b * n4));
    }
}

__global__ void noise_images_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                    const int64_t* __restrict__ t, const float* __restrict__ sa_tab,
                                    const float* __restrict__ sb_tab, int batch, int n, float* __restrict__ out) {
    const long total = (long)batch * n;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / n);
        const float sa = sa_tab[t[b]], sb = sb_tab[t[b]];
        out[i] = sa * x[i] + sb * eps[i];
    }
}

// python evaluates (1 - self.beta) in double; torch then multiplies the fp32 tensor by the fp32-rounded scalar
__global__ void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n, float beta, float omb) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        ema[i] = ema[i] * beta + omb * p[i];
}

inline int grid_for(long total, int block = 256, int cap = 2048) {
    long g = (total + block - 1) / block;
    if (g < 1) g = 1;
    return (int)(g < cap ? g : cap);
}

// emb rows for every (timestep, sample): SiLU(time[t] + label[y_b]) as operand planes (unet.py:1550-1581 followed by the
// SiLU that opens every emb_layers, unet.py:609) - lets the sampler tabulate the FiLM vectors of all steps in one GEMM
__global__ void emb_combine_kernel(const float* __restrict__ time, const float* __restrict__ label, const int64_t* __restrict__ y,
                                   int num_classes, int T, int B, int ted, wd_bf16* __restrict__ out_hi,
                                   wd_bf16* __restrict__ out_lo, int out_ld) {
    const int t4 = ted >> 2;
    const long total = (long)T * B * t4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / t4;
        const int cx = (int)(i - row * t4) * 4;
        const int t = (int)(row / B), b = (int)(row - (long)t * B);
        float4 v = *reinterpret_cast<const float4*>(time + (long)t * ted + cx);
        if (label) {
            long yb = y[b];  // range-checked on the host (engine.check_ids); clamped here so that a stale id can never read
            yb = yb < 0 ? 0 : (yb >= num_classes ? num_classes - 1 : yb);  // past the table
            const float4 l = *reinterpret_cast<const float4*>(label + yb * ted + cx);
            v.x += l.x; v.y += l.y; v.z += l.z; v.w += l.w;
        }
        v.x = wd_silu(v.x); v.y = wd_silu(v.y); v.z = wd_silu(v.z); v.w = wd_silu(v.w);
        uint2 hi, lo;
        wd_split4(v, hi, lo);
        *reinterpret_cast<uint2*>(out_hi + row * out_ld + cx) = hi;
        if (out_lo) *reinterpret_cast<uint2*>(out_lo + row * out_ld + cx) = lo;
    }
}
// out[b][:] = table[((*t_dev) % chunk) * B + b][:]  (the rows of the current timestep inside the resident chunk of `chunk`
// timesteps; t_dev lives on the device so the launch replays)
__global__ void select_rows_kernel(const float* __restrict__ table, const int32_t* __restrict__ t_dev, int B, long row4,
                                   int chunk, float* __restrict__ out) {
    const long base = (long)((*t_dev) % chunk) * B * row4;
    const long total = (long)B * row4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
        reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(table)[base + i];
}

// ---- writer-style interpolation (unet.py:1558-1573) ----------------------------------------------------------------------
// y = (1 - m) * label[s1] + m * label[s2] with the reference's fp32 op order: two products, one sum (no contraction in this
// file).  Ids are range-checked on the host and clamped here, as in emb_combine_kernel.
__device__ __forceinline__ float4 label_mix4(const float* __restrict__ label, const int32_t* __restrict__ pair, int num_classes,
                                             int ted, int cx, float m) {
    int s1 = pair[0], s2 = pair[1];
    s1 = s1 < 0 ? 0 : (s1 >= num_classes ? num_classes - 1 : s1);
    s2 = s2 < 0 ? 0 : (s2 >= num_classes ? num_classes - 1 : s2);
    const float4 a = *reinterpret_cast<const float4*>(label + (long)s1 * ted + cx);
    const float4 b = *reinterpret_cast<const float4*>(label + (long)s2 * ted + cx);
    const float om = 1.0f - m;
    return make_float4(om * a.x + m * b.x, om * a.y + m * b.y, om * a.z + m * b.z, om * a.w + m * b.w);
}

// emb_combine_kernel with the label row replaced by the blend of the pair of (t, b): row t*B + b
__global__ void emb_combine_mix_kernel(const float* __restrict__ time, const float* __restrict__ label,
                                       const int32_t* __restrict__ pairs, const float* __restrict__ mix, int num_classes, int T, int B,
                                       int ted, wd_bf16* __restrict__ out_hi, wd_bf16* __restrict__ out_lo, int out_ld) {
    const int t4 = ted >> 2;
    const long total = (long)T * B * t4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / t4;
        const int cx = (int)(i - row * t4) * 4;
        const int t = (int)(row / B), b = (int)(row - (long)t * B);
        float4 v = *reinterpret_cast<const float4*>(time + (long)t * ted + cx);
        const float4 l = label_mix4(label, pairs + 2 * row, num_classes, ted, cx, mix[b]);
        v.x += l.x; v.y += l.y; v.z += l.z; v.w += l.w;
        v.x = wd_silu(v.x); v.y = wd_silu(v.y); v.z = wd_silu(v.z); v.w = wd_silu(v.w);
        uint2 hi, lo;
        wd_split4(v, hi, lo);
        *reinterpret_cast<uint2*>(out_hi + row * out_ld + cx) = hi;
        if (out_lo) *reinterpret_cast<uint2*>(out_lo + row * out_ld + cx) = lo;
    }
}

__global__ void label_mix_kernel(const float* __restrict__ label, const int32_t* __restrict__ pairs, const float* __restrict__ mix,
                                 int num_classes, int B, int ted, float* __restrict__ out) {
    const int t4 = ted >> 2;
    const long total = (long)B * t4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / t4), cx = (int)(i - (long)b * t4) * 4;
        *reinterpret_cast<float4*>(out + (long)b * ted + cx) = label_mix4(label, pairs + 2 * b, num_classes, ted, cx, mix[b]);
    }
}

// ---- writer-free guidance ---------------------------------------------------------------------------------------------------
// emb_combine_kernel with the label term per sample: where keep[b] == 0 (or keep == NULL) the row is SiLU(time[t]) - the term is
// left out, not multiplied by zero (the reference's imgConditioned == 1 branch, unet.py:1578-1579).  Kept rows run
// emb_combine_kernel's operations in its order.
__global__ void emb_combine_keep_kernel(const float* __restrict__ time, const float* __restrict__ label, const int64_t* __restrict__ y,
                                        const uint8_t* __restrict__ keep, int num_classes, int T, int B, int ted,
                                        wd_bf16* __restrict__ out_hi, wd_bf16* __restrict__ out_lo, int out_ld) {
    const int t4 = ted >> 2;
    const long total = (long)T * B * t4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / t4;
        const int cx = (int)(i - row * t4) * 4;
        const int t = (int)(row / B), b = (int)(row - (long)t * B);
        float4 v = *reinterpret_cast<const float4*>(time + (long)t * ted + cx);
        if (keep && keep[b]) {
            long yb = y[b];
            yb = yb < 0 ? 0 : (yb >= num_classes ? num_classes - 1 : yb);
            const float4 l = *reinterpret_cast<const float4*>(label + yb * ted + cx);
            v.x += l.x; v.y += l.y; v.z += l.z; v.w += l.w;
        }
        v.x = wd_silu(v.x); v.y = wd_silu(v.y); v.z = wd_silu(v.z); v.w = wd_silu(v.w);
        uint2 hi, lo;
        wd_split4(v, hi, lo);
        *reinterpret_cast<uint2*>(out_hi + row * out_ld + cx) = hi;
        if (out_lo) *reinterpret_cast<uint2*>(out_lo + row * out_ld + cx) = lo;
    }
}

// out[b][:] = label[y_b][:] where sample b keeps its writer, zeros where it does not.  The decision is keep_in[b], or (DRAW) word 0
// of one Philox4x32-10 call with counter (0, d.tag, row) >= d.thr, row the global sample row of wd_dropout_row: every lane of a
// row recomputes it, the lane of the row's first four columns also writes y_eff[b] (y_b, or -1 when dropped) and keep_out[b].
template <bool DRAW>
__global__ void label_rows_keep_kernel(const float* __restrict__ label, const int64_t* __restrict__ y, int num_classes, int B, int ted,
                                       const wd_dropout d, const uint8_t* __restrict__ keep_in, float* __restrict__ out,
                                       int64_t* __restrict__ y_eff, uint8_t* __restrict__ keep_out) {
    const int t4 = ted >> 2;
    const long total = (long)B * t4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / t4), cx = (int)(i - (long)b * t4) * 4;
        bool keep;
        if constexpr (DRAW) {
            const uint64_t row = wd_dropout_row(d, b);
            uint32_t w[4] = {0u, d.tag, (uint32_t)row, (uint32_t)(row >> 32)};
            philox4x32_10(w, (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
            keep = w[0] >= d.thr;
        } else {
            keep = keep_in[b] != 0;
        }
        const long yb = y[b];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (keep) {
            const long yc = yb < 0 ? 0 : (yb >= num_classes ? num_classes - 1 : yb);  // range-checked on the host, as above
            v = *reinterpret_cast<const float4*>(label + yc * ted + cx);
        }
        *reinterpret_cast<float4*>(out + (long)b * ted + cx) = v;
        if (cx == 0) {
            if (y_eff) y_eff[b] = keep ? (int64_t)yb : (int64_t)-1;
            if (keep_out) keep_out[b] = keep ? 1 : 0;
        }
    }
}

// torch.lerp(second, first, s) as ATen evaluates it: the weight >= 0.5 form is first - (first - second) * (1 - s)
__device__ __forceinline__ float lerp_cfg(float first, float second, float s, float oms, bool high) {
    const float d = first - second;
    return high ? first - d * oms : second + s * d;
}

// ddpm_step_kernel on eps = lerp(second, first, scale)
__global__ void ddpm_step_cfg_kernel(float* __restrict__ x, const float* __restrict__ first, const float* __restrict__ second,
                                     float scale, float* __restrict__ eps_out, int batch, int n4, const float* __restrict__ ca,
                                     const float* __restrict__ cb, const float* __restrict__ cs, const int32_t* __restrict__ t_dev,
                                     const float* __restrict__ noise, uint64_t seed, uint64_t sample_offset) {
    const int t = *t_dev;
    const float a = ca[t], bb = cb[t], s = cs[t];
    const float oms = 1.0f - scale;
    const bool high = fabsf(scale) >= 0.5f;
    const long total = (long)batch * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / n4);
        const uint32_t e4 = (uint32_t)(i - (long)b * n4);
        float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t > 1) {
            if (noise) z = reinterpret_cast<const float4*>(noise)[i];
            else z = philox_normal4(seed, sample_offset + (uint64_t)b, (uint32_t)t, e4);
        }
        const float4 xv = reinterpret_cast<const float4*>(x)[i];
        const float4 fv = reinterpret_cast<const float4*>(first)[i];
        const float4 sv = reinterpret_cast<const float4*>(second)[i];
        float4 ev;
        ev.x = lerp_cfg(fv.x, sv.x, scale, oms, high);
        ev.y = lerp_cfg(fv.y, sv.y, scale, oms, high);
        ev.z = lerp_cfg(fv.z, sv.z, scale, oms, high);
        ev.w = lerp_cfg(fv.w, sv.w, scale, oms, high);
        if (eps_out) reinterpret_cast<float4*>(eps_out)[i] = ev;
        float4 o;
        o.x = a * (xv.x - bb * ev.x) + s * z.x;
        o.y = a * (xv.y - bb * ev.y) + s * z.y;
        o.z = a * (xv.z - bb * ev.z) + s * z.z;
        o.w = a * (xv.w - bb * ev.w) + s * z.w;
        reinterpret_cast<float4*>(x)[i] = o;
    }
}

// torch.lerp(second, first, s) bit for bit for any weight: torch's device kernel is compiled with contraction, so both of its
// forms, ``second + s * (first - second)`` below 0.5 and ``first - (first - second) * (1 - s)`` from 0.5 on, are ONE fused
// multiply-add.  lerp_cfg rounds the product and the sum separately, which is the same value only where the product is exact
// (s = 3 and s = 0.25 are such weights: 1 - s = -2 and s are powers of two).  The fma is spelled out: this file compiles with
// contraction off.
__device__ __forceinline__ float lerp_guided(float first, float second, float s, float oms, bool high) {
    const float d = first - second;
    return high ? __builtin_fmaf(-d, oms, first) : __builtin_fmaf(s, d, second);
}

// DDIM update (Song et al. 2020, eq. 12) on the step index k = *k_dev of the visited-timestep tables:
//   x0 = (x - c1[k] * e) * c2[k];  x = (c3[k] * x0 + c4[k] * e) + c5[k] * z,  every operation rounded on its own;
// e = eps, or lerp_guided(eps, second, scale) when second != NULL.  c5[k] == 0: no z is read or drawn and the term is omitted.
__global__ void ddim_step_kernel(float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ second, float scale,
                                 float* __restrict__ eps_out, int batch, int n4, const float* __restrict__ c1,
                                 const float* __restrict__ c2, const float* __restrict__ c3, const float* __restrict__ c4,
                                 const float* __restrict__ c5, const int32_t* __restrict__ k_dev, const int32_t* __restrict__ t_dev,
                                 const float* __restrict__ noise, uint64_t seed, uint64_t sample_offset) {
    const int k = *k_dev;
    const int t = *t_dev;
    const float a1 = c1[k], a2 = c2[k], a3 = c3[k], a4 = c4[k], sg = c5[k];
    const float oms = 1.0f - scale;
    const bool high = fabsf(scale) >= 0.5f;
    const long total = (long)batch * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const float4 xv = reinterpret_cast<const float4*>(x)[i];
        float4 ev = reinterpret_cast<const float4*>(eps)[i];
        if (second) {
            const float4 sv = reinterpret_cast<const float4*>(second)[i];
            ev.x = lerp_guided(ev.x, sv.x, scale, oms, high);
            ev.y = lerp_guided(ev.y, sv.y, scale, oms, high);
            ev.z = lerp_guided(ev.z, sv.z, scale, oms, high);
            ev.w = lerp_guided(ev.w, sv.w, scale, oms, high);
        }
        if (eps_out) reinterpret_cast<float4*>(eps_out)[i] = ev;
        float4 o;
        o.x = a3 * ((xv.x - a1 * ev.x) * a2) + a4 * ev.x;
        o.y = a3 * ((xv.y - a1 * ev.y) * a2) + a4 * ev.y;
        o.z = a3 * ((xv.z - a1 * ev.z) * a2) + a4 * ev.z;
        o.w = a3 * ((xv.w - a1 * ev.w) * a2) + a4 * ev.w;
        if (sg != 0.0f) {
            float4 z;
            if (noise) z = reinterpret_cast<const float4*>(noise)[i];
            else {
                const int b = (int)(i / n4);
                z = philox_normal4(seed, sample_offset + (uint64_t)b, (uint32_t)t, (uint32_t)(i - (long)b * n4));
            }
            o.x = o.x + sg * z.x;
            o.y = o.y + sg * z.y;
            o.z = o.z + sg * z.z;
            o.w = o.w + sg * z.w;
        }
        reinterpret_cast<float4*>(x)[i] = o;
    }
}

// DPM-Solver++(2M) update (Lu et al. 2022, algorithm 2) on the step index k = *k_dev of the visited-timestep tables:
//   x0 = (x - c1[k] * e) * c2[k];  D = x0, or x0 + c5[k] * (x0 - x0_prev) when c5[k] != 0;  x = c3[k] * x + c4[k] * D;
//   x0_prev = x0,  every operation rounded on its own.  e as in ddim_step_kernel.  c5[k] == 0: x0_prev is written, not read.
__global__ void dpmpp_step_kernel(float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ second, float scale,
                                  float* __restrict__ eps_out, float* __restrict__ x0_prev, int batch, int n4,
                                  const float* __restrict__ c1, const float* __restrict__ c2, const float* __restrict__ c3,
                                  const float* __restrict__ c4, const float* __restrict__ c5, const int32_t* __restrict__ k_dev) {
    const int k = *k_dev;
    const float a1 = c1[k], a2 = c2[k], a3 = c3[k], a4 = c4[k], r = c5[k];
    const float oms = 1.0f - scale;
    const bool high = fabsf(scale) >= 0.5f;
    const long total = (long)batch * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const float4 xv = reinterpret_cast<const float4*>(x)[i];
        float4 ev = reinterpret_cast<const float4*>(eps)[i];
        if (second) {
            const float4 sv = reinterpret_cast<const float4*>(second)[i];
            ev.x = lerp_guided(ev.x, sv.x, scale, oms, high);
            ev.y = lerp_guided(ev.y, sv.y, scale, oms, high);
            ev.z = lerp_guided(ev.z, sv.z, scale, oms, high);
            ev.w = lerp_guided(ev.w, sv.w, scale, oms, high);
        }
        if (eps_out) reinterpret_cast<float4*>(eps_out)[i] = ev;
        float4 x0;
        x0.x = (xv.x - a1 * ev.x) * a2;
        x0.y = (xv.y - a1 * ev.y) * a2;
        x0.z = (xv.z - a1 * ev.z) * a2;
        x0.w = (xv.w - a1 * ev.w) * a2;
        float4 d = x0;
        if (r != 0.0f) {
            const float4 pv = reinterpret_cast<const float4*>(x0_prev)[i];
            d.x = x0.x + r * (x0.x - pv.x);
            d.y = x0.y + r * (x0.y - pv.y);
            d.z = x0.z + r * (x0.z - pv.z);
            d.w = x0.w + r * (x0.w - pv.w);
        }
        reinterpret_cast<float4*>(x0_prev)[i] = x0;
        float4 o;
        o.x = a3 * xv.x + a4 * d.x;
        o.y = a3 * xv.y + a4 * d.y;
        o.z = a3 * xv.z + a4 * d.z;
        o.w = a3 * xv.w + a4 * d.w;
        reinterpret_cast<float4*>(x)[i] = o;
    }
}

// advance_kernel over a table of visited timesteps: k <- min(k + 1, S - 1), t <- tau[k]
__global__ void next_timestep_kernel(int32_t* k_dev, const int32_t* __restrict__ tau, int S, int32_t* t_dev, int64_t* t64,
                                     int batch) {
    __shared__ int kn, tn;
    if (threadIdx.x == 0) {
        int k = *k_dev + 1;
        if (k > S - 1) k = S - 1;  // the last visited step stays current: nothing is read past the tables
        if (k < 0) k = 0;
        kn = k;
        tn = tau[k];
    }
    __syncthreads();
    const int v = tn;
    for (int b = threadIdx.x; b < batch; b += blockDim.x) t64[b] = (int64_t)v;
    __syncthreads();
    if (threadIdx.x == 0) {
        *k_dev = kn;
        *t_dev = v;
    }
}

// Known-region blend after a sampler's update, before its timestep advance: x is at the level of the predecessor p
// (*t_dev - 1, or tau[*k_dev + 1], 0 after the last entry), and where the mask m keeps, it is replaced by the known latent x0
// noised to that level:  kv = x0 at p == 0, else sa[p] * x0 + sb[p] * z (the expression of noise_images_kernel);
//   x = x (m == 0, the bits it had),  kv (m == 1),  x + m * (kv - x) otherwise,  every operation rounded on its own.
// z from ``noise`` or from the Philox stream under the tag WD_TAG_KNOWN | p; neither is touched at p == 0, and what is drawn
// for a group of four does not depend on its mask.
__global__ void known_blend_kernel(float* __restrict__ x, const float* __restrict__ x0, const float* __restrict__ mask, int batch,
                                   int n4, const float* __restrict__ sa_tab, const float* __restrict__ sb_tab,
                                   const int32_t* __restrict__ t_dev, const int32_t* __restrict__ k_dev,
                                   const int32_t* __restrict__ tau, int S, const float* __restrict__ noise, uint64_t seed,
                                   uint64_t sample_offset) {
    int p;
    if (tau) {
        const int k = *k_dev;
        p = (k >= -1 && k + 1 < S) ? tau[k + 1] : 0;
    } else {
        p = *t_dev - 1;
    }
    if (p < 0) p = 0;  // index 0 of the schedule is the last level there is
    const float sa = sa_tab[p], sb = sb_tab[p];
    const long total = (long)batch * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const float4 xv = reinterpret_cast<const float4*>(x)[i];
        const float4 m = reinterpret_cast<const float4*>(mask)[i];
        float4 kv = reinterpret_cast<const float4*>(x0)[i];
        if (p != 0) {
            float4 z;
            if (noise) z = reinterpret_cast<const float4*>(noise)[i];
            else {
                const int b = (int)(i / n4);
                z = philox_normal4(seed, sample_offset + (uint64_t)b, (uint32_t)WD_TAG_KNOWN | (uint32_t)p, (uint32_t)(i - (long)b * n4));
            }
            kv.x = sa * kv.x + sb * z.x;
            kv.y = sa * kv.y + sb * z.y;
            kv.z = sa * kv.z + sb * z.z;
            kv.w = sa * kv.w + sb * z.w;
        }
        float4 o;
        o.x = m.x == 0.0f ? xv.x : (m.x == 1.0f ? kv.x : xv.x + m.x * (kv.x - xv.x));
        o.y = m.y == 0.0f ? xv.y : (m.y == 1.0f ? kv.y : xv.y + m.y * (kv.y - xv.y));
        o.z = m.z == 0.0f ? xv.z : (m.z == 1.0f ? kv.z : xv.z + m.z * (kv.z - xv.z));
        o.w = m.w == 0.0f ? xv.w : (m.w == 1.0f ? kv.w : xv.w + m.w * (kv.w - xv.w));
        reinterpret_cast<float4*>(x)[i] = o;
    }
}

// ---- AutoencoderKL posterior (DiagonalGaussianDistribution of the encoder's moments) --------------------------------
// One draw for four consecutive elements of a sample, shared by both kernels below:
//   sample = scale * (mean + exp(0.5 * logvar) * z), every operation rounded on its own (no contraction in this file);
// z from ``noise`` (float4 index i4 of the whole batch) or from the Philox stream of wd_randn under WD_STREAM_VAE_POSTERIOR.
__device__ __forceinline__ float4 posterior_draw4(const float4 m, const float4 lv, float scale, const float* __restrict__ noise,
                                                  long i4, uint64_t seed, uint64_t sample, uint32_t e4) {
    const float4 z = noise ? reinterpret_cast<const float4*>(noise)[i4]
                           : philox_normal4(seed, sample, 0x80000000u | (uint32_t)WD_STREAM_VAE_POSTERIOR, e4);
    float4 o;
    o.x = scale * (m.x + expf(0.5f * lv.x) * z.x);
    o.y = scale * (m.y + expf(0.5f * lv.y) * z.y);
    o.z = scale * (m.z + expf(0.5f * lv.z) * z.z);
    o.w = scale * (m.w + expf(0.5f * lv.w) * z.w);
    return o;
}

constexpr int kVaeMaxK = 2 * WD_VAE_MAX_LATENT;

// quant_conv output o at one position: ((w[o][0] x[0] + w[o][1] x[1]) + ... + w[o][K-1] x[K-1]) + bias[o], plain fp32
__device__ __forceinline__ float quant_dot(const float* __restrict__ w, const float (&x)[kVaeMaxK], int K2, float bias) {
    float acc = w[0] * x[0];
#pragma unroll
    for (int k = 1; k < kVaeMaxK; ++k)
        if (k < K2) acc = acc + w[k] * x[k];
    return acc + bias;
}

__device__ __forceinline__ float clamp_logvar(float v) { return v < -30.0f ? -30.0f : (v > 20.0f ? 20.0f : v); }  // NaN passes, as torch.clamp

__device__ __forceinline__ void load_moments(const float* __restrict__ row, int K2, int vec, float (&x)[kVaeMaxK]) {
    if (vec) {  // K2 % 4 == 0, rows 16-byte aligned
#pragma unroll
        for (int k = 0; k < kVaeMaxK; k += 4)
            if (k < K2) {
                const float4 v = *reinterpret_cast<const float4*>(row + k);
                x[k] = v.x; x[k + 1] = v.y; x[k + 2] = v.z; x[k + 3] = v.w;
            }
    } else {
#pragma unroll
        for (int k = 0; k < kVaeMaxK; ++k)
            if (k < K2) x[k] = row[k];
    }
}

// hw % 4 == 0: one thread owns four consecutive positions of a sample: it reads their token rows once and writes, per latent
// channel, one float4 of mean / logvar / sample (consecutive threads -> consecutive float4s of a channel plane).
__global__ void vae_posterior_rows_kernel(const float* __restrict__ moments, int ld, int vec, const float* __restrict__ w,
                                          const float* __restrict__ bias, int batch, int L, int hw, float* __restrict__ mean,
                                          float* __restrict__ logvar, float* __restrict__ sample, float scale,
                                          const float* __restrict__ noise, uint64_t seed, uint64_t sample_offset) {
    const int K2 = 2 * L, hw4 = hw >> 2;
    const long total = (long)batch * hw4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / hw4), p0 = (int)(i - (long)b * hw4) * 4;
        float x[4][kVaeMaxK];
#pragma unroll
        for (int j = 0; j < 4; ++j) load_moments(moments + ((long)b * hw + p0 + j) * ld, K2, vec, x[j]);
#pragma unroll
        for (int l = 0; l < WD_VAE_MAX_LATENT; ++l) {
            if (l >= L) break;
            const float* wm = w + l * K2;
            const float* wv = w + (L + l) * K2;
            const float bm = bias[l], bv = bias[L + l];
            const float4 m = make_float4(quant_dot(wm, x[0], K2, bm), quant_dot(wm, x[1], K2, bm), quant_dot(wm, x[2], K2, bm),
                                         quant_dot(wm, x[3], K2, bm));
            const float4 lv = make_float4(clamp_logvar(quant_dot(wv, x[0], K2, bv)), clamp_logvar(quant_dot(wv, x[1], K2, bv)),
                                          clamp_logvar(quant_dot(wv, x[2], K2, bv)), clamp_logvar(quant_dot(wv, x[3], K2, bv)));
            const uint32_t e4 = (uint32_t)(((long)l * hw + p0) >> 2);
            const long o4 = (long)b * ((long)L * hw4) + e4;
            reinterpret_cast<float4*>(mean)[o4] = m;
            reinterpret_cast<float4*>(logvar)[o4] = lv;
            if (sample)
                reinterpret_cast<float4*>(sample)[o4] = posterior_draw4(m, lv, scale, noise, o4, seed, sample_offset + (uint64_t)b, e4);
        }
    }
}

// any hw with L * hw % 4 == 0: one thread per float4 of the NCHW output; its four elements may lie in two channel planes, so
// each one finds its own (channel, position) and reads that position's token row (the rows stay in cache: a map of odd size is small).
__global__ void vae_posterior_flat_kernel(const float* __restrict__ moments, int ld, int vec, const float* __restrict__ w,
                                          const float* __restrict__ bias, int batch, int L, int hw, float* __restrict__ mean,
                                          float* __restrict__ logvar, float* __restrict__ sample, float scale,
                                          const float* __restrict__ noise, uint64_t seed, uint64_t sample_offset) {
    const int K2 = 2 * L, n4 = (L * hw) >> 2;
    const long total = (long)batch * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / n4);
        const uint32_t e4 = (uint32_t)(i - (long)b * n4);
        float mv[4], lvv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = (int)e4 * 4 + j, l = idx / hw, p = idx - l * hw;
            float x[kVaeMaxK];
            load_moments(moments + ((long)b * hw + p) * ld, K2, vec, x);
            mv[j] = quant_dot(w + l * K2, x, K2, bias[l]);
            lvv[j] = clamp_logvar(quant_dot(w + (L + l) * K2, x, K2, bias[L + l]));
        }
        const float4 m = make_float4(mv[0], mv[1], mv[2], mv[3]), lv = make_float4(lvv[0], lvv[1], lvv[2], lvv[3]);
        reinterpret_cast<float4*>(mean)[i] = m;
        reinterpret_cast<float4*>(logvar)[i] = lv;
        if (sample) reinterpret_cast<float4*>(sample)[i] = posterior_draw4(m, lv, scale, noise, i, seed, sample_offset + (uint64_t)b, e4);
    }
}

__global__ void posterior_sample_kernel(const float* __restrict__ mean, const float* __restrict__ logvar, int batch, int n4,
                                        float* __restrict__ sample, float scale, const float* __restrict__ noise, uint64_t seed,
                                        uint64_t sample_offset) {
    const long total = (long)batch * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / n4);
        reinterpret_cast<float4*>(sample)[i] =
            posterior_draw4(reinterpret_cast<const float4*>(mean)[i], reinterpret_cast<const float4*>(logvar)[i], scale, noise, i, seed,
                            sample_offset + (uint64_t)b, (uint32_t)(i - (long)b * n4));
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

extern "C" int wd_timestep_embedding(const int64_t* t, int batch, const float* freqs, int half, wd_bf16* out_hi,
                                     wd_bf16* out_lo, int out_ld, void* stream) {
    if (!t || !freqs || !out_hi || batch <= 0 || half <= 0 || out_ld < 2 * half) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(temb_kernel, dim3((batch * half + 255) / 256), dim3(256), 0, st, t, batch, freqs, half, out_hi,
                       out_lo, out_ld);
    return wd_check_launch();
}

extern "C" int wd_embed_tokens(const void* ids, int ids_are_i64, int rows, int seq_len, const float* table, int vocab,
                               int c, const float* pe, wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, void* stream) {
    if (!ids || !table || !out_hi || rows <= 0 || seq_len <= 0 || vocab <= 0 || c <= 0 || c % 4 || out_ld % 4 || out_ld < c)
        return WD_EINVAL;
    if (!aligned16(table) || !aligned16(pe) || !aligned8(out_hi) || !aligned8(out_lo)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(embed_kernel, dim3(grid_for((long)rows * (c / 4))), dim3(256), 0, st, ids, ids_are_i64, rows,
                       seq_len, table, vocab, c, pe, out_hi, out_lo, out_ld);
    return wd_check_launch();
}

extern "C" int wd_im2col3x3(const float* x, int batch, int cin, int h, int w, wd_bf16* out_hi, wd_bf16* out_lo,
                            int kpad, void* stream) {
    if (!x || !out_hi || batch <= 0 || cin <= 0 || h <= 0 || w <= 0 || kpad < 9 * cin || kpad % 32) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(im2col_kernel, dim3(grid_for((long)batch * h * w * kpad)), dim3(256), 0, st, x, batch, cin, h, w,
                       out_hi, out_lo, kpad);
    return wd_check_launch();
}

extern "C" int wd_nchw_to_tokens(const float* x, int batch, int c, int hw, float* out, int ld, void* stream) {
    if (!x || !out || batch <= 0 || c <= 0 || hw <= 0 || ld < c) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(nchw_to_tok_kernel, dim3(grid_for((long)batch * c * hw)), dim3(256), 0, st, x, batch, c, hw, out,
                       ld);
    return wd_check_launch();
}

extern "C" int wd_tokens_to_nchw(const float* x, int ld, int batch, int c, int hw, float* out, void* stream) {
    if (!x || !out || batch <= 0 || c <= 0 || hw <= 0 || ld < c) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(tok_to_nchw_kernel, dim3(grid_for((long)batch * c * hw)), dim3(256), 0, st, x, ld, batch, c, hw,
                       out);
    return wd_check_launch();
}

extern "C" int wd_ddpm_step(float* x, const float* eps, int batch, int n_per_sample, const float* ca, const float* cb,
                            const float* cs, const int32_t* t_dev, const float* noise, uint64_t seed,
                            uint64_t sample_offset, void* stream) {
    if (!x || !eps || !ca || !cb || !cs || !t_dev || batch <= 0 || n_per_sample <= 0 || n_per_sample % 4)
        return WD_EINVAL;
    if (!aligned16(x) || !aligned16(eps) || !aligned16(noise)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(ddpm_step_kernel, dim3(grid_for((long)batch * (n_per_sample / 4))), dim3(256), 0, st, x, eps,
                       batch, n_per_sample / 4, ca, cb, cs, t_dev, noise, seed, sample_offset);
    return wd_check_launch();
}

extern "C" int wd_advance_timestep(int32_t* t_dev, int delta, int64_t* t64, int batch, void* stream) {
    if (!t_dev || !t64 || batch <= 0) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(256), 0, st, t_dev, delta, t64, batch);
    return wd_check_launch();
}

extern "C" int wd_randn(float* out, int batch, int n_per_sample, uint64_t seed, uint64_t sample_offset,
                        uint32_t stream_id, void* stream) {
    if (!out || batch <= 0 || n_per_sample <= 0 || n_per_sample % 4 || !aligned16(out)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(randn_kernel, dim3(grid_for((long)batch * (n_per_sample / 4))), dim3(256), 0, st, out, batch,
                       n_per_sample / 4, seed, sample_offset, 0x80000000u | stream_id);
    return wd_check_launch();
}

extern "C" int wd_noise_images(const float* x, const float* eps, const int64_t* t, const float* sqrt_ah,
                               const float* sqrt_1m_ah, int batch, int n_per_sample, float* out, void* stream) {
    if (!x || !eps || !t || !sqrt_ah || !sqrt_1m_ah || !out || batch <= 0 || n_per_sample <= 0) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(noise_images_kernel, dim3(grid_for((long)batch * n_per_sample)), dim3(256), 0, st, x, eps, t,
                       sqrt_ah, sqrt_1m_ah, batch, n_per_sample, out);
    return wd_check_launch();
}

extern "C" int wd_copy2d(void* dst, int64_t dst_pitch, const void* src, int64_t src_pitch, int64_t width_bytes,
                         int64_t rows, void* stream) {
    if (!dst || !src || width_bytes <= 0 || rows <= 0 || dst_pitch < width_bytes || src_pitch < width_bytes)
        return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    return hipMemcpy2DAsync(dst, (size_t)dst_pitch, src, (size_t)src_pitch, (size_t)width_bytes, (size_t)rows,
                            hipMemcpyDeviceToDevice, st) == hipSuccess
               ? WD_OK
               : WD_ELAUNCH;
}

extern "C" int wd_ema_update(float* ema, const float* p, int64_t n, double beta, void* stream) {
    if (!ema || !p || n <= 0) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(ema_kernel, dim3(grid_for(n)), dim3(256), 0, st, ema, p, n, (float)beta,
                       (float)(1.0 - beta));
    return wd_check_launch();
}

extern "C" int wd_emb_combine(const float* time, const float* label, const int64_t* y, int num_classes, int T, int B, int ted,
                              wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, void* stream) {
    if (!time || !out_hi || T <= 0 || B <= 0 || ted <= 0 || ted % 4 || out_ld % 4 || out_ld < ted ||
        (label && (!y || num_classes <= 0)))
        return WD_EINVAL;
    if (!aligned16(time) || !aligned16(label) || !aligned8(out_hi) || !aligned8(out_lo)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(emb_combine_kernel, dim3(grid_for((long)T * B * (ted / 4))), dim3(256), 0, st, time, label, y, num_classes, T,
                       B, ted, out_hi, out_lo, out_ld);
    return wd_check_launch();
}

extern "C" int wd_select_rows(const float* table, const int32_t* t_dev, int batch, int64_t row_floats, int chunk, float* out,
                              void* stream) {
    if (!table || !t_dev || !out || batch <= 0 || row_floats <= 0 || row_floats % 4 || chunk <= 0) return WD_EINVAL;
    if (!aligned16(table) || !aligned16(out)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(select_rows_kernel, dim3(grid_for((long)batch * (row_floats / 4))), dim3(256), 0, st, table, t_dev, batch,
                       (long)(row_floats / 4), chunk, out);
    return wd_check_launch();
}

extern "C" int wd_emb_combine_mix(const float* time, const float* label, const int32_t* pairs, const float* mix, int num_classes,
                                  int T, int B, int ted, wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, void* stream) {
    if (!time || !label || !pairs || !mix || !out_hi || num_classes <= 0 || T <= 0 || B <= 0 || ted <= 0 || ted % 4 || out_ld % 4 ||
        out_ld < ted)
        return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(emb_combine_mix_kernel, dim3(grid_for((long)T * B * (ted / 4))), dim3(256), 0, st, time, label, pairs, mix,
                       num_classes, T, B, ted, out_hi, out_lo, out_ld);
    return wd_check_launch();
}

extern "C" int wd_label_mix(const float* label, const int32_t* pairs, const float* mix, int num_classes, int B, int ted, float* out,
                            void* stream) {
    if (!label || !pairs || !mix || !out || num_classes <= 0 || B <= 0 || ted <= 0 || ted % 4) return WD_EINVAL;
    if (!aligned16(label) || !aligned16(out)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(label_mix_kernel, dim3(grid_for((long)B * (ted / 4))), dim3(256), 0, st, label, pairs, mix, num_classes, B, ted,
                       out);
    return wd_check_launch();
}

extern "C" int wd_emb_combine_keep(const float* time, const float* label, const int64_t* y, const uint8_t* keep, int num_classes, int T,
                                   int B, int ted, wd_bf16* out_hi, wd_bf16* out_lo, int out_ld, void* stream) {
    if (!time || !out_hi || T <= 0 || B <= 0 || ted <= 0 || ted % 4 || out_ld % 4 || out_ld < ted ||
        (keep && (!label || !y || num_classes <= 0)))
        return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(emb_combine_keep_kernel, dim3(grid_for((long)T * B * (ted / 4))), dim3(256), 0, st, time, label, y, keep,
                       num_classes, T, B, ted, out_hi, out_lo, out_ld);
    return wd_check_launch();
}

extern "C" int wd_label_rows_keep(const float* label, const int64_t* y, int num_classes, int B, int ted, const wd_dropout* d,
                                  const uint8_t* keep_in, float* out, int64_t* y_eff, uint8_t* keep_out, void* stream) {
    if (!label || !y || !out || num_classes <= 0 || B <= 0 || ted <= 0 || ted % 4 || (!d && !keep_in) || ((uintptr_t)out & 15))
        return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    const dim3 grid(grid_for((long)B * (ted / 4)));
    if (d)
        hipLaunchKernelGGL(label_rows_keep_kernel<true>, grid, dim3(256), 0, st, label, y, num_classes, B, ted, *d, keep_in, out, y_eff,
                           keep_out);
    else
        hipLaunchKernelGGL(label_rows_keep_kernel<false>, grid, dim3(256), 0, st, label, y, num_classes, B, ted, wd_dropout{}, keep_in,
                           out, y_eff, keep_out);
    return wd_check_launch();
}

extern "C" int wd_ddpm_step_cfg(float* x, const float* first, const float* second, float scale, float* eps_out, int batch,
                                int n_per_sample, const float* ca, const float* cb, const float* cs, const int32_t* t_dev,
                                const float* noise, uint64_t seed, uint64_t sample_offset, void* stream) {
    if (!x || !first || !second || !ca || !cb || !cs || !t_dev || batch <= 0 || n_per_sample <= 0 || n_per_sample % 4)
        return WD_EINVAL;
    if (!aligned16(x) || !aligned16(first) || !aligned16(second) || !aligned16(eps_out) || !aligned16(noise)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(ddpm_step_cfg_kernel, dim3(grid_for((long)batch * (n_per_sample / 4))), dim3(256), 0, st, x, first, second,
                       scale, eps_out, batch, n_per_sample / 4, ca, cb, cs, t_dev, noise, seed, sample_offset);
    return wd_check_launch();
}

extern "C" int wd_ddim_step(float* x, const float* eps, const float* second, float scale, float* eps_out, int batch, int n_per_sample,
                            const float* c1, const float* c2, const float* c3, const float* c4, const float* c5,
                            const int32_t* k_dev, const int32_t* t_dev, const float* noise, uint64_t seed, uint64_t sample_offset,
                            void* stream) {
    if (!x || !eps || !c1 || !c2 || !c3 || !c4 || !c5 || !k_dev || !t_dev || batch <= 0 || n_per_sample <= 0 || n_per_sample % 4)
        return WD_EINVAL;
    if (!aligned16(x) || !aligned16(eps) || !aligned16(second) || !aligned16(noise) || !aligned16(eps_out)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(ddim_step_kernel, dim3(grid_for((long)batch * (n_per_sample / 4))), dim3(256), 0, st, x, eps, second, scale,
                       eps_out, batch, n_per_sample / 4, c1, c2, c3, c4, c5, k_dev, t_dev, noise, seed, sample_offset);
    return wd_check_launch();
}

extern "C" int wd_dpmpp_step(float* x, const float* eps, const float* second, float scale, float* eps_out, float* x0_prev, int batch,
                             int n_per_sample, const float* c1, const float* c2, const float* c3, const float* c4, const float* c5,
                             const int32_t* k_dev, void* stream) {
    if (!x || !eps || !x0_prev || !c1 || !c2 || !c3 || !c4 || !c5 || !k_dev || batch <= 0 || n_per_sample <= 0 || n_per_sample % 4)
        return WD_EINVAL;
    if (!aligned16(x) || !aligned16(eps) || !aligned16(second) || !aligned16(eps_out) || !aligned16(x0_prev)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(dpmpp_step_kernel, dim3(grid_for((long)batch * (n_per_sample / 4))), dim3(256), 0, st, x, eps, second, scale,
                       eps_out, x0_prev, batch, n_per_sample / 4, c1, c2, c3, c4, c5, k_dev);
    return wd_check_launch();
}

extern "C" int wd_next_timestep(int32_t* k_dev, const int32_t* tau, int S, int32_t* t_dev, int64_t* t64, int batch, void* stream) {
    if (!k_dev || !tau || !t_dev || !t64 || S <= 0 || batch <= 0) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(next_timestep_kernel, dim3(1), dim3(256), 0, st, k_dev, tau, S, t_dev, t64, batch);
    return wd_check_launch();
}

extern "C" int wd_known_blend(float* x, const float* x0, const float* mask, int batch, int n_per_sample, const float* sqrt_ah,
                              const float* sqrt_1m_ah, const int32_t* t_dev, const int32_t* k_dev, const int32_t* tau, int S,
                              const float* noise, uint64_t seed, uint64_t sample_offset, void* stream) {
    if (!x || !x0 || !mask || !sqrt_ah || !sqrt_1m_ah || batch <= 0 || n_per_sample <= 0 || n_per_sample % 4) return WD_EINVAL;
    if (tau ? (S < 1 || !k_dev) : !t_dev) return WD_EINVAL;
    if (!aligned16(x) || !aligned16(x0) || !aligned16(mask) || !aligned16(noise)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(known_blend_kernel, dim3(grid_for((long)batch * (n_per_sample / 4))), dim3(256), 0, st, x, x0, mask, batch,
                       n_per_sample / 4, sqrt_ah, sqrt_1m_ah, t_dev, k_dev, tau, S, noise, seed, sample_offset);
    return wd_check_launch();
}

extern "C" int wd_vae_posterior(const float* moments_tok, int ld, const float* w, const float* bias, int batch, int L, int hw,
                                float* mean, float* logvar, float* sample, float scale, const float* noise, uint64_t seed,
                                uint64_t sample_offset, void* stream) {
    if (!moments_tok || !w || !bias || !mean || !logvar || batch <= 0 || hw <= 0 || L < 1 || L > WD_VAE_MAX_LATENT || ld < 2 * L ||
        ((long)L * hw) % 4 || (long)L * hw > 0x7fffffffL || (noise && !sample))
        return WD_EINVAL;
    if (!aligned16(mean) || !aligned16(logvar) || !aligned16(sample) || !aligned16(noise)) return WD_EINVAL;
    const int vec = (L % 2 == 0) && (ld % 4 == 0) && aligned16(moments_tok);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    if (hw % 4 == 0)
        hipLaunchKernelGGL(vae_posterior_rows_kernel, dim3(grid_for((long)batch * (hw / 4))), dim3(256), 0, st, moments_tok, ld, vec, w,
                           bias, batch, L, hw, mean, logvar, sample, scale, noise, seed, sample_offset);
    else
        hipLaunchKernelGGL(vae_posterior_flat_kernel, dim3(grid_for((long)batch * (L * hw / 4))), dim3(256), 0, st, moments_tok, ld, vec,
                           w, bias, batch, L, hw, mean, logvar, sample, scale, noise, seed, sample_offset);
    return wd_check_launch();
}

extern "C" int wd_posterior_sample(const float* mean, const float* logvar, int batch, int n_per_sample, float* sample, float scale,
                                   const float* noise, uint64_t seed, uint64_t sample_offset, void* stream) {
    if (!mean || !logvar || !sample || batch <= 0 || n_per_sample <= 0 || n_per_sample % 4) return WD_EINVAL;
    if (!aligned16(mean) || !aligned16(logvar) || !aligned16(sample) || !aligned16(noise)) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(posterior_sample_kernel, dim3(grid_for((long)batch * (n_per_sample / 4))), dim3(256), 0, st, mean, logvar, batch,
                       n_per_sample / 4, sample, scale, noise, seed, sample_offset);
    return wd_check_launch();
}
