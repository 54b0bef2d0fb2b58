// Optimiser side of the training step (SURVEY.md row a-T): MSE loss + its gradient, multi-tensor fused AdamW with the
// EMA of the weights folded in.  Reference: nn.MSELoss()(noise, predicted_noise) train.py:289; optim.AdamW(lr=1e-4)
// train.py:405 (torch defaults betas (0.9, 0.999), eps 1e-8, weight_decay 0.01); EMA.step_ema train.py:146-170, which
// the reference runs as ~260 x 3 separate elementwise launches per step.  Arithmetic follows torch's single-tensor
// AdamW op order in fp32 (no contraction) so that updates are comparable bit-for-bit up to the division rounding.
#include "wd_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CHUNK = 8192;  // elements per workgroup

// which tensor owns chunk c (binary search over the running chunk0 sums; adamw_multi_kernel keeps its own copy of the loop -
// through this helper the compiler swaps the operands of one scalar add, and that kernel's code is to stay what it was)
__device__ __forceinline__ int chunk_owner(const wd_adamw_table_entry* __restrict__ tab, int ntensor, int64_t c) {
    int lo = 0, hi = ntensor - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].chunk0 <= c) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// GS is empty (wd_adamw_multi: the plain kernel, its signature and code as they were) or one `const float*` (wd_adamw_multi_scaled):
// a device-resident factor every gradient is multiplied by as it is loaded, the product rounded on its own.
template <typename... GS>
__global__ void adamw_multi_kernel(const wd_adamw_table_entry* __restrict__ tab, int ntensor, float decay, float omb1, float b2,
                                   float omb2, float step_size, float bc2_sqrt, float eps, int ema_mode, float ema_b,
                                   float ema_omb, const GS... gscale) {
    // binary search: which tensor owns chunk blockIdx.x
    int lo = 0, hi = ntensor - 1;
    const int64_t c = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].chunk0 <= c) lo = mid;
        else hi = mid - 1;
    }
    const wd_adamw_table_entry t = tab[lo];
    const int64_t base = (c - t.chunk0) * CHUNK;
    const int64_t end = base + CHUNK < t.n ? base + CHUNK : t.n;
    if (!t.g) {
        // a parameter the loss does not reach (grad None in the reference: AdamW skips it, train.py:293); EMA still runs
        if (t.ema && ema_mode)
            for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x)
                t.ema[i] = ema_mode == 1 ? t.p[i] : t.ema[i] * ema_b + ema_omb * t.p[i];
        return;
    }
    float gs = 1.0f;
    if constexpr (sizeof...(GS) > 0) gs = *(gscale, ...);  // one read per workgroup (uniform)
    for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
        float g = t.g[i];
        if constexpr (sizeof...(GS) > 0) g = g * gs;  // the clipped gradient, as torch's grad.mul_(clip_coef) leaves it
        float p = t.p[i] * decay;                 // param.mul_(1 - lr * weight_decay)
        float m = t.m[i];
        m = m + omb1 * (g - m);                   // exp_avg.lerp_(grad, 1 - beta1)
        float v = t.v[i] * b2;                    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        v = v + (omb2 * g) * g;
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        p = p + (-step_size * m) / denom;         // param.addcdiv_(exp_avg, denom, value=-step_size)
        t.p[i] = p;
        t.m[i] = m;
        t.v[i] = v;
        if (t.ema) {
            if (ema_mode == 1) t.ema[i] = p;                                  // warm-up: plain copy (train.py:161-170)
            else if (ema_mode == 2) t.ema[i] = t.ema[i] * ema_b + ema_omb * p;  // old * beta + (1 - beta) * new
        }
    }
}

// deterministic two-stage sum of (a - b)^2; stage 1 also writes d loss / d pred = 2 (pred - target) / n
__global__ void mse_stage1(const float* __restrict__ pred, const float* __restrict__ target, int64_t n, float scale,
                           float* __restrict__ grad, double* __restrict__ partial) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float d = pred[i] - target[i];
        acc += (double)(d * d);
        if (grad) grad[i] = scale * d;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
__global__ void mse_stage2(const double* __restrict__ partial, int nb, int64_t n, float* __restrict__ loss) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < nb; ++i) s += partial[i];
        *loss = (float)(s / (double)n);
    }
}

// ---- global gradient norm (clip_grad_norm_) and gradient accumulation: streaming passes over the flat gradient arena ----------
// Sum of squares of one chunk of one tensor in double, one partial per workgroup.  16-byte loads where the address allows: a
// scalar head up to the first 16-byte boundary of g + base, float4 body, scalar tail.  Every lane's order is fixed by (address,
// length) alone and the LDS tree is fixed, so the partial is the same bits on every run.
__global__ __launch_bounds__(256) void grad_sqnorm_stage1(const wd_adamw_table_entry* __restrict__ tab, int ntensor,
                                                          double* __restrict__ partial) {
    __shared__ double sh[256];
    const int64_t c = blockIdx.x;
    const wd_adamw_table_entry t = tab[chunk_owner(tab, ntensor, c)];
    double acc = 0.0;
    if (t.g) {
        const int64_t base = (c - t.chunk0) * CHUNK;
        const int len = (int)(base + CHUNK < t.n ? CHUNK : t.n - base);
        const float* __restrict__ g = t.g + base;
        int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(g) & 15u)) & 15u) >> 2);
        if (head > len) head = len;
        const int nvec = (len - head) >> 2;
        if ((int)threadIdx.x < head) {
            const double x = (double)g[threadIdx.x];
            acc += x * x;
        }
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + head);
        for (int i = threadIdx.x; i < nvec; i += 256) {
            const float4 q = g4[i];
            acc += (double)q.x * (double)q.x;
            acc += (double)q.y * (double)q.y;
            acc += (double)q.z * (double)q.z;
            acc += (double)q.w * (double)q.w;
        }
        const int tail0 = head + (nvec << 2);
        if (tail0 + (int)threadIdx.x < len) {
            const double x = (double)g[tail0 + threadIdx.x];
            acc += x * x;
        }
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[c] = sh[0];
}

// One workgroup: lane l adds partials l, l + 256, ... in index order, then the same LDS tree.  ctl[0] = the norm, ctl[1] = the
// clip coefficient of torch.nn.utils.clip_grad_norm_, formed in fp32: clamp(max_norm / (norm + 1e-6), max = 1).  torch.clamp
// passes NaN on, so a NaN quotient (a NaN norm, or inf / inf) stays NaN here too.
__global__ __launch_bounds__(256) void grad_sqnorm_stage2(const double* __restrict__ partial, int64_t n, float max_norm,
                                                          float* __restrict__ ctl) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) acc += partial[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(sh[0]);
        const float q = max_norm / (norm + 1e-6f);
        ctl[0] = norm;
        ctl[1] = q != q ? q : fminf(1.0f, q);
    }
}

// dst = scale * (OVERWRITE ? src : dst + src); n4 float4s from 16-byte aligned pointers
template <bool OVERWRITE>
__global__ __launch_bounds__(256) void grad_accumulate_vec(float4* __restrict__ dst, const float4* __restrict__ src, int64_t n4,
                                                           float scale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 s = src[i];
        if (!OVERWRITE) {
            const float4 d = dst[i];
            s.x = d.x + s.x;
            s.y = d.y + s.y;
            s.z = d.z + s.z;
            s.w = d.w + s.w;
        }
        s.x = scale * s.x;
        s.y = scale * s.y;
        s.z = scale * s.z;
        s.w = scale * s.w;
        dst[i] = s;
    }
}
// the ragged ends (and everything, when dst and src are not aligned alike): elements [0, head) and [tail0, n)
template <bool OVERWRITE>
__global__ __launch_bounds__(256) void grad_accumulate_scalar(float* __restrict__ dst, const float* __restrict__ src, int64_t head,
                                                              int64_t tail0, int64_t n, float scale) {
    const int64_t cnt = head + (n - tail0);
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < cnt; j += (int64_t)gridDim.x * 256) {
        const int64_t i = j < head ? j : tail0 + (j - head);
        const float s = src[i];
        dst[i] = scale * (OVERWRITE ? s : dst[i] + s);
    }
}

// ---- weighted, masked per-sample squared error (wd_weighted_mse_loss; specification in include/wdiff_hip.h) --------------------
// Stage 1: one workgroup per sample.  With a mask the gradient scale needs M_b = sum(m) first, so the mask row is summed in a
// pass of its own (the main pass reads it again from L2; a sample is 4 KB at the training shape).  Every lane's order is fixed by
// n_per_sample alone and the LDS tree is fixed, so S_b and M_b are the same bits on every run.  out2[b] = S_b, out2[batch + b] = M_b.
template <bool MASKED>
__global__ __launch_bounds__(256) void wmse_stage1(const float* __restrict__ pred, const float* __restrict__ target,
                                                   const float* __restrict__ mask, int batch, int n4,
                                                   const int64_t* __restrict__ t, const float* __restrict__ weights,
                                                   float* __restrict__ grad, double* __restrict__ out2) {
    __shared__ double sh[256];
    const int b = blockIdx.x;
    const int64_t row = (int64_t)b * n4;
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(pred) + row;
    const float4* __restrict__ e4 = reinterpret_cast<const float4*>(target) + row;
    const float4* __restrict__ m4 = MASKED ? reinterpret_cast<const float4*>(mask) + row : nullptr;
    float4* __restrict__ g4 = grad ? reinterpret_cast<float4*>(grad) + row : nullptr;
    double M = 4.0 * (double)n4;
    if constexpr (MASKED) {
        double acc = 0.0;
        for (int i = threadIdx.x; i < n4; i += 256) {
            const float4 m = m4[i];
            acc += (double)m.x;
            acc += (double)m.y;
            acc += (double)m.z;
            acc += (double)m.w;
        }
        sh[threadIdx.x] = acc;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
            __syncthreads();
        }
        M = sh[0];
        __syncthreads();  // (sh is reused below)
    }
    const float w = weights ? weights[t[b]] : 1.0f;
    // M == 0: the sample has no cell to learn from; its gradient row is 0 whatever pred holds
    const bool live = M != 0.0;
    const float c = live ? (float)(2.0 * (double)w / ((double)batch * M)) : 0.0f;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const float4 p = p4[i], e = e4[i];
        float4 d;
        d.x = p.x - e.x;
        d.y = p.y - e.y;
        d.z = p.z - e.z;
        d.w = p.w - e.w;
        if constexpr (MASKED) {
            const float4 m = m4[i];
            acc += (double)m.x * ((double)d.x * (double)d.x);
            acc += (double)m.y * ((double)d.y * (double)d.y);
            acc += (double)m.z * ((double)d.z * (double)d.z);
            acc += (double)m.w * ((double)d.w * (double)d.w);
            d.x = m.x * d.x;
            d.y = m.y * d.y;
            d.z = m.z * d.z;
            d.w = m.w * d.w;
        } else {
            acc += (double)d.x * (double)d.x;
            acc += (double)d.y * (double)d.y;
            acc += (double)d.z * (double)d.z;
            acc += (double)d.w * (double)d.w;
        }
        if (g4) {
            float4 g;
            g.x = live ? c * d.x : 0.0f;
            g.y = live ? c * d.y : 0.0f;
            g.z = live ? c * d.z : 0.0f;
            g.w = live ? c * d.w : 0.0f;
            g4[i] = g;
        }
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out2[b] = sh[0];
        out2[batch + b] = M;
    }
}

// Stage 2: one workgroup, 256 samples at a time.  Lane l forms sample base + l's mean, weighted term and bin; then lane 0 adds the
// terms with b ascending, and lane j updates the bins j, j + 256, ... each walking the samples with b ascending - the bins do not
// interact, so this is the recurrence "for b ascending: hist[bin_b] += (l_b, 1)" of the specification.
__global__ __launch_bounds__(256) void wmse_stage2(const double* __restrict__ in2, int batch, const int64_t* __restrict__ t,
                                                   const float* __restrict__ weights, int T, float* __restrict__ loss,
                                                   float* __restrict__ sample_loss, double* __restrict__ hist, int nbins) {
    __shared__ double term[256];
    __shared__ float mean[256];
    __shared__ int bin[256];  // -1: the sample has M_b == 0 and is skipped
    double total = 0.0;
    for (int base = 0; base < batch; base += 256) {
        const int b = base + threadIdx.x;
        const int cnt = batch - base < 256 ? batch - base : 256;
        if (b < batch) {
            const double S = in2[b], M = in2[batch + b];
            const bool live = M != 0.0;
            const double q = live ? S / M : 0.0;
            const float l = (float)q;
            int64_t tb = 0;
            if (weights || hist) tb = t[b];
            const float w = weights ? weights[tb] : 1.0f;
            term[threadIdx.x] = (double)w * q;
            mean[threadIdx.x] = l;
            bin[threadIdx.x] = !live ? -1 : hist ? (int)((tb * (int64_t)nbins) / (int64_t)T) : 0;
            if (sample_loss) sample_loss[b] = l;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < cnt; ++i)
                if (bin[i] >= 0) total += term[i];
        if (hist)
            for (int k = threadIdx.x; k < nbins; k += 256) {
                double s = hist[2 * (int64_t)k], c = hist[2 * (int64_t)k + 1];
                bool hit = false;
                for (int i = 0; i < cnt; ++i)
                    if (bin[i] == k) {
                        s += (double)mean[i];
                        c += 1.0;
                        hit = true;
                    }
                if (hit) {
                    hist[2 * (int64_t)k] = s;
                    hist[2 * (int64_t)k + 1] = c;
                }
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(total / (double)batch);
}

// ---- row-wise AdamW over a few rows of one embedding table (wd_adamw_rows; specification in include/wdiff_hip.h) ---------------
// The row list travels in the kernel arguments.  wd_adamw_multi's op order per element; with an anchor the decay step is
// p - lrwd * (p - a).  One thread per float4 of one listed row: blockIdx.y is the slot.
struct row_list {
    int row[WD_ROWS_MAX];
};
__device__ __forceinline__ float adamw_row_elem(float p, float g, float& m, float& v, bool anchored, float a, float gs, bool scaled,
                                                float decay, float lrwd, float omb1, float b2, float omb2, float step_size,
                                                float bc2_sqrt, float eps) {
    if (scaled) g = g * gs;
    if (anchored) p = p - lrwd * (p - a);
    else p = p * decay;
    m = m + omb1 * (g - m);
    v = v * b2;
    v = v + (omb2 * g) * g;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    return p + (-step_size * m) / denom;
}
__global__ __launch_bounds__(256) void adamw_rows_kernel(float* __restrict__ table, int ld, int c4, const row_list rows,
                                                         const float* __restrict__ grad, float* __restrict__ m,
                                                         float* __restrict__ v, const float* __restrict__ anchor,
                                                         float* __restrict__ ema_table, int ema_ld, float decay, float lrwd,
                                                         float omb1, float b2, float omb2, float step_size, float bc2_sqrt,
                                                         float eps, int ema_mode, float ema_b, float ema_omb,
                                                         const float* __restrict__ gscale) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= c4) return;
    const int64_t row = rows.row[j];
    const int64_t ci = (int64_t)j * c4 + i;  // float4 index into the compact buffers
    float4* __restrict__ p4 = reinterpret_cast<float4*>(table + row * ld) + i;
    const float gs = gscale ? *gscale : 1.0f;
    const bool scaled = gscale != nullptr, anchored = anchor != nullptr;
    float4 p = *p4, mm = reinterpret_cast<float4*>(m)[ci], vv = reinterpret_cast<float4*>(v)[ci];
    const float4 g = reinterpret_cast<const float4*>(grad)[ci];
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (anchored) a = reinterpret_cast<const float4*>(anchor)[ci];
    p.x = adamw_row_elem(p.x, g.x, mm.x, vv.x, anchored, a.x, gs, scaled, decay, lrwd, omb1, b2, omb2, step_size, bc2_sqrt, eps);
    p.y = adamw_row_elem(p.y, g.y, mm.y, vv.y, anchored, a.y, gs, scaled, decay, lrwd, omb1, b2, omb2, step_size, bc2_sqrt, eps);
    p.z = adamw_row_elem(p.z, g.z, mm.z, vv.z, anchored, a.z, gs, scaled, decay, lrwd, omb1, b2, omb2, step_size, bc2_sqrt, eps);
    p.w = adamw_row_elem(p.w, g.w, mm.w, vv.w, anchored, a.w, gs, scaled, decay, lrwd, omb1, b2, omb2, step_size, bc2_sqrt, eps);
    *p4 = p;
    reinterpret_cast<float4*>(m)[ci] = mm;
    reinterpret_cast<float4*>(v)[ci] = vv;
    if (ema_table && ema_mode) {
        float4* __restrict__ e4 = reinterpret_cast<float4*>(ema_table + row * ema_ld) + i;
        if (ema_mode == 1) {
            *e4 = p;  // warm-up: plain copy
        } else {
            float4 e = *e4;
            e.x = e.x * ema_b + ema_omb * p.x;
            e.y = e.y * ema_b + ema_omb * p.y;
            e.z = e.z * ema_b + ema_omb * p.z;
            e.w = e.w * ema_b + ema_omb * p.w;
            *e4 = e;
        }
    }
}

}  // namespace

extern "C" int wd_adamw_table_entry_bytes(void) { return (int)sizeof(wd_adamw_table_entry); }
extern "C" int wd_adamw_chunk(void) { return CHUNK; }

extern "C" int wd_adamw_multi(const void* table, int ntensor, int64_t total_chunks, double lr, double beta1, double beta2,
                              double eps, double weight_decay, int64_t step, int ema_mode, double ema_beta, void* stream) {
    if (!table || ntensor <= 0 || total_chunks <= 0 || step <= 0 || ema_mode < 0 || ema_mode > 2) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // the scalars exactly as torch forms them (python doubles), then rounded once to fp32
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const float decay = (float)(1.0 - lr * weight_decay), omb1 = (float)(1.0 - beta1), b2 = (float)beta2,
                omb2 = (float)(1.0 - beta2), step_size = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(adamw_multi_kernel<>, dim3((unsigned)total_chunks), dim3(256), 0, st,
                       reinterpret_cast<const wd_adamw_table_entry*>(table), ntensor, decay, omb1, b2, omb2, step_size, bc2_sqrt,
                       (float)eps, ema_mode, (float)ema_beta, (float)(1.0 - ema_beta));
    return wd_check_launch();
}

extern "C" int wd_adamw_multi_scaled(const void* table, int ntensor, int64_t total_chunks, double lr, double beta1, double beta2,
                                     double eps, double weight_decay, int64_t step, int ema_mode, double ema_beta,
                                     const float* gscale, void* stream) {
    if (!table || !gscale || ntensor <= 0 || total_chunks <= 0 || step <= 0 || ema_mode < 0 || ema_mode > 2) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const float decay = (float)(1.0 - lr * weight_decay), omb1 = (float)(1.0 - beta1), b2 = (float)beta2,
                omb2 = (float)(1.0 - beta2), step_size = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(adamw_multi_kernel<const float*>, dim3((unsigned)total_chunks), dim3(256), 0, st,
                       reinterpret_cast<const wd_adamw_table_entry*>(table), ntensor, decay, omb1, b2, omb2, step_size, bc2_sqrt,
                       (float)eps, ema_mode, (float)ema_beta, (float)(1.0 - ema_beta), gscale);
    return wd_check_launch();
}

extern "C" int wd_grad_sqnorm_multi(const void* table, int ntensor, int64_t total_chunks, double* partial, float max_norm,
                                    float* ctl, void* stream) {
    if (!table || !partial || !ctl || ntensor <= 0 || total_chunks <= 0 || total_chunks > 0x7fffffff || !(max_norm > 0.0f))
        return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(grad_sqnorm_stage1, dim3((unsigned)total_chunks), dim3(256), 0, st,
                       reinterpret_cast<const wd_adamw_table_entry*>(table), ntensor, partial);
    hipLaunchKernelGGL(grad_sqnorm_stage2, dim3(1), dim3(256), 0, st, partial, total_chunks, max_norm, ctl);
    return wd_check_launch();
}

extern "C" int wd_grad_accumulate(float* dst, const float* src, int64_t n, int overwrite, float scale, void* stream) {
    if (!dst || !src || n <= 0) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uintptr_t da = reinterpret_cast<uintptr_t>(dst), sa = reinterpret_cast<uintptr_t>(src);
    if ((da & 3u) || (sa & 3u)) return WD_EINVAL;
    // float4 body where dst and src reach a 16-byte boundary at the same element; scalar head and tail (or everything)
    int64_t head = n, n4 = 0;
    if ((da & 15u) == (sa & 15u)) {
        head = (int64_t)(((16u - (unsigned)(da & 15u)) & 15u) >> 2);
        if (head > n) head = n;
        n4 = (n - head) >> 2;
    }
    const int64_t tail0 = head + 4 * n4, nscalar = head + (n - tail0);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    if (n4 > 0) {
        const int64_t want = (n4 + 255) / 256;
        const unsigned nb = (unsigned)(want < 8192 ? want : 8192);
        if (overwrite)
            hipLaunchKernelGGL(grad_accumulate_vec<true>, dim3(nb), dim3(256), 0, st, reinterpret_cast<float4*>(dst + head),
                               reinterpret_cast<const float4*>(src + head), n4, scale);
        else
            hipLaunchKernelGGL(grad_accumulate_vec<false>, dim3(nb), dim3(256), 0, st, reinterpret_cast<float4*>(dst + head),
                               reinterpret_cast<const float4*>(src + head), n4, scale);
    }
    if (nscalar > 0) {
        const int64_t want = (nscalar + 255) / 256;
        const unsigned nb = (unsigned)(want < 8192 ? want : 8192);
        if (overwrite)
            hipLaunchKernelGGL(grad_accumulate_scalar<true>, dim3(nb), dim3(256), 0, st, dst, src, head, tail0, n, scale);
        else
            hipLaunchKernelGGL(grad_accumulate_scalar<false>, dim3(nb), dim3(256), 0, st, dst, src, head, tail0, n, scale);
    }
    return wd_check_launch();
}

extern "C" int wd_mse_loss(const float* pred, const float* target, int64_t n, float* grad, float* loss, double* scratch,
                           int scratch_len, void* stream) {
    if (!pred || !target || !loss || !scratch || n <= 0 || scratch_len < 1) return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int nb = (int)((n + 255) / 256 < scratch_len ? (n + 255) / 256 : scratch_len);
    if (nb > 1024) nb = 1024;
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(mse_stage1, dim3(nb), dim3(256), 0, st, pred, target, n, (float)(2.0 / (double)n), grad, scratch);
    hipLaunchKernelGGL(mse_stage2, dim3(1), dim3(64), 0, st, scratch, nb, n, loss);
    return wd_check_launch();
}

extern "C" int wd_weighted_mse_loss(const float* pred, const float* target, const float* mask, int batch, int n_per_sample,
                                    const int64_t* t, const float* weights, int T, float* grad, float* loss, float* sample_loss,
                                    double* hist, int nbins, double* scratch, void* stream) {
    if (!pred || !target || !loss || !scratch || batch < 1 || n_per_sample < 4 || (n_per_sample & 3)) return WD_EINVAL;
    if ((weights || hist) && (!t || T < 1)) return WD_EINVAL;
    if (hist && nbins < 1) return WD_EINVAL;
    if ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(mask) |
         reinterpret_cast<uintptr_t>(grad)) & 15u)
        return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    const int n4 = n_per_sample >> 2;
    if (mask)
        hipLaunchKernelGGL(wmse_stage1<true>, dim3((unsigned)batch), dim3(256), 0, st, pred, target, mask, batch, n4, t, weights,
                           grad, scratch);
    else
        hipLaunchKernelGGL(wmse_stage1<false>, dim3((unsigned)batch), dim3(256), 0, st, pred, target, mask, batch, n4, t, weights,
                           grad, scratch);
    hipLaunchKernelGGL(wmse_stage2, dim3(1), dim3(256), 0, st, scratch, batch, t, weights, T, loss, sample_loss, hist, nbins);
    return wd_check_launch();
}

extern "C" int wd_adamw_rows(float* table, int ld, int c, const int* rows, int nrows, int vocab, const float* grad, float* m,
                             float* v, const float* anchor, float* ema_table, int ema_ld, double lr, double beta1, double beta2,
                             double eps, double weight_decay, int64_t step, int ema_mode, double ema_beta, const float* gscale,
                             void* stream) {
    if (!table || !rows || !grad || !m || !v || nrows < 1 || nrows > WD_ROWS_MAX || vocab < 1 || c < 4 || (c & 3) || ld < c ||
        (ld & 3) || step <= 0 || ema_mode < 0 || ema_mode > 2)
        return WD_EINVAL;
    if (ema_table && (ema_ld < c || (ema_ld & 3))) return WD_EINVAL;
    if ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(m) |
         reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(anchor) | reinterpret_cast<uintptr_t>(ema_table)) & 15u)
        return WD_EINVAL;
    if (reinterpret_cast<uintptr_t>(gscale) & 3u) return WD_EINVAL;
    row_list rl;
    for (int j = 0; j < nrows; ++j) {
        if (rows[j] < 0 || rows[j] >= vocab) return WD_EINVAL;
        for (int k = 0; k < j; ++k)
            if (rows[k] == rows[j]) return WD_EINVAL;
        rl.row[j] = rows[j];
    }
    for (int j = nrows; j < WD_ROWS_MAX; ++j) rl.row[j] = 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // the scalars as wd_adamw_multi forms them (doubles, rounded once to fp32)
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const float decay = (float)(1.0 - lr * weight_decay), lrwd = (float)(lr * weight_decay), omb1 = (float)(1.0 - beta1),
                b2 = (float)beta2, omb2 = (float)(1.0 - beta2), step_size = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    const int c4 = c >> 2;
    WdLaunchScope scope(WD_CLS_OTHER, st);
    hipLaunchKernelGGL(adamw_rows_kernel, dim3((unsigned)((c4 + 255) / 256), (unsigned)nrows), dim3(256), 0, st, table, ld, c4, rl,
                       grad, m, v, anchor, ema_table, ema_ld, decay, lrwd, omb1, b2, omb2, step_size, bc2_sqrt, (float)eps,
                       ema_mode, (float)ema_beta, (float)(1.0 - ema_beta), gscale);
    return wd_check_launch();
}
