// wd_ctc_loss: log-softmax + CTC loss, forward and gradient with respect to the raw logits, in one call (specification in
// include/wdiff_hip.h; DESIGN.md section 9 "CTC loss").  gfx950 only.
//
// One workgroup of 512 threads per sample.  alpha and beta are kept in the LOG domain, in DOUBLE.  (An fp32 log-space recursion -
// what torch runs - loses the gradient at T = 256: log-probabilities near -900 have an fp32 ulp of 6e-5, and that is exponentiated;
// in double the ulp there is 1e-13.  The scaled linear-domain recursion was tried first and is not enough: with peaked logits the
// mass of alpha_t and the mass of beta_t sit on different states, and the states that carry the posterior fall below double's
// range in either one.)
//
//   phase 0  waves share the rows t < input_len: lse_t = logsumexp of the row (max in fp32, sum and log in double), then the
//            log-probabilities E[t][k] = x[t][lab_k] - lse_t of the blank (k = 0) and of target j (k = 1 + j)
//   phase 1  the even waves run alpha forwards, the odd waves run beta backwards (torch's convention: beta holds the emission of
//            its own state), one state per thread, one barrier per step for both; every step's values go to the workspace
//   phase 2  nll = -logaddexp of the two final states; feasibility
//   phase 3  waves share the rows again: w(s) = exp(alpha + beta - lp + nll), the posterior of state s, then every class sums the
//            states that carry it in a fixed order (the blank: a butterfly over the even states; any other: a walk over the targets
//            with that id, ascending), g = scale (p - share)
// Nothing is accumulated atomically: the same bits on every run.
#include "wd_common.h"

#define CTC_THREADS 512
#define CTC_SMAX (2 * WD_CTC_MAX_L + 1)  // 255 states at most: one per thread of a direction
#define CTC_CHUNK 16                     // steps of the recursion per memory round trip (even)
#define CTC_SP 260                       // a step buffer: 256 slots + 2 slots of -inf on the side the recursion reaches over

__device__ __forceinline__ double ctc_wave_sum(double v) {  // xor butterfly: a + b == b + a, so all 64 lanes end with the same bits
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// log(e^a + e^b + e^c) for values that are finite or -inf.  The largest of the three contributes e^0 = 1 whichever it is, so only
// the other two are exponentiated: three double transcendentals per call, which is what a step of the recursion costs.
__device__ __forceinline__ double ctc_lse3(double a, double b, double c) {
    const double p = fmax(a, b), q = fmin(a, b);
    const double hi = fmax(p, c), r = fmin(p, c);  // {hi, q, r} = {a, b, c}
    if (hi == -INFINITY) return -INFINITY;
    return hi + log1p(exp(q - hi) + exp(r - hi));
}
__device__ __forceinline__ float ctc_wave_max(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// doubles of workspace: [batch] nll, then per sample E [T][Lmax + 1], A (log alpha) [T][2 Lmax + 1], Bt (log beta) [T][2 Lmax + 1]
static inline int64_t ctc_sample_doubles(int T, int Lmax) { return (int64_t)T * (5 * (int64_t)Lmax + 3); }

template <bool I64>
__global__ __launch_bounds__(CTC_THREADS) void ctc_sample_kernel(const float* __restrict__ logits, int ld, int T, int batch, int C,
                                                                 const void* __restrict__ targets, int tld, int Lmax,
                                                                 const int32_t* __restrict__ input_len,
                                                                 const int32_t* __restrict__ target_len, float scale,
                                                                 float* __restrict__ dlogits, int dld, float* __restrict__ sample_nll,
                                                                 int32_t* __restrict__ status, double* ws,
                                                                 int64_t sample_doubles) {
    __shared__ double lse[WD_CTC_MAX_T];    // phase 0 -> phase 3
    __shared__ double abuf[2][CTC_SP];      // log alpha_t(s) at [s + 2]; [0], [1] stay -inf
    __shared__ double bbuf[2][CTC_SP];      // log beta_t(s) at [s]; [S ..] are -inf
    __shared__ double wbuf[8][CTC_SMAX + 1];
    __shared__ int tgt[WD_CTC_MAX_L + 1];
    __shared__ int nxt[WD_CTC_MAX_L + 1];   // next target position with the same id, -1 at the end
    __shared__ int head[WD_CTC_MAX_C];      // first target position that carries class c, -1 for none
    __shared__ int bad;
    __shared__ double nll_sh;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Tin = input_len[b], L = target_len[b];
    if (tid == 0) bad = 0;
    for (int c = tid; c < C; c += CTC_THREADS) head[c] = -1;
    __syncthreads();
    int mybad = 0;
    if (Tin < 1 || Tin > T) mybad |= 1;
    if (L < 0 || L > Lmax) mybad |= 2;
    if (!(mybad & 2)) {
        for (int j = tid; j < L; j += CTC_THREADS) {
            const int64_t id = I64 ? reinterpret_cast<const int64_t*>(targets)[(int64_t)b * tld + j]
                                   : (int64_t) reinterpret_cast<const int32_t*>(targets)[(int64_t)b * tld + j];
            if (id < 0 || id >= C) mybad |= 4;
            tgt[j] = (int)(id < 0 || id >= C ? 0 : id);
        }
    }
    if (mybad) atomicOr(&bad, mybad);
    __syncthreads();
    const int badall = bad;
    const int64_t row0 = b;  // row (t, b) of logits / dlogits is t * batch + b
    if (badall) {
        if (tid == 0) {
            status[b] = badall;
            sample_nll[b] = 0.0f;
            ws[b] = 0.0;
        }
        if (dlogits)
            for (int t = wave; t < T; t += 8)
                for (int c = lane; c < C; c += 64) dlogits[((int64_t)t * batch + row0) * dld + c] = 0.0f;
        return;
    }
    const int S = 2 * L + 1;
    double* E = ws + batch + (int64_t)b * sample_doubles;
    double* A = E + (int64_t)T * (Lmax + 1);
    double* Bt = A + (int64_t)T * (2 * Lmax + 1);
    const int ldE = Lmax + 1, ldS = 2 * Lmax + 1;

    if (tid == 0) {  // the targets of every class, ascending: L <= 127 steps
        status[b] = 0;
        for (int j = L - 1; j >= 0; --j) {
            nxt[j] = head[tgt[j]];
            head[tgt[j]] = j;
        }
    }
    for (int i = tid; i < 2 * CTC_SP; i += CTC_THREADS) {
        (&abuf[0][0])[i] = -INFINITY;
        (&bbuf[0][0])[i] = -INFINITY;
    }

    // ---- phase 0: lse_t and the log-probabilities of the target's classes ---------------------------------------------------
    for (int t = wave; t < Tin; t += 8) {
        const float* __restrict__ x = logits + ((int64_t)t * batch + row0) * ld;
        float m = -INFINITY;
        for (int c = lane; c < C; c += 64) m = fmaxf(m, x[c]);
        m = ctc_wave_max(m);
        double sum = 0.0;
        for (int c = lane; c < C; c += 64) sum += exp((double)x[c] - (double)m);
        sum = ctc_wave_sum(sum);
        const double l = (double)m + log(sum);
        if (lane == 0) lse[t] = l;
        for (int k = lane; k <= L; k += 64) E[(int64_t)t * ldE + k] = (double)x[k ? tgt[k - 1] : 0] - l;
    }
    __syncthreads();

    // ---- phase 1: alpha and beta, one state per thread ---------------------------------------------------------------------
    // even waves carry alpha, odd waves beta: the first wave of each - often the only ones with a live state - then sit on
    // different SIMDs of the CU (waves of a workgroup go to the SIMDs in turn), and a wave without a live state skips the arithmetic
    const bool is_alpha = !(wave & 1);
    const int s = (wave >> 1) * 64 + lane;
    const bool wave_live = (wave >> 1) * 64 < S;
    const bool live = s < S;
    const int ek = (s & 1) ? 1 + (s >> 1) : 0;  // the emission column of state s
    const int lab = live ? ((s & 1) ? tgt[s >> 1] : 0) : -1;
    // the transition that skips a state: from s - 2 (alpha) / to s + 2 (beta), when the two labels differ
    bool skip = false;
    if (is_alpha) {
        if (live && s >= 2 && ((s & 1) ? tgt[(s - 2) >> 1] : 0) != lab) skip = true;
    } else {
        if (live && s + 2 < S && ((s & 1) ? tgt[(s + 2) >> 1] : 0) != lab) skip = true;
    }
    // t = 0 for alpha: states 0 and 1; t = Tin - 1 for beta: states S - 1 and S - 2
    const int t_first = is_alpha ? 0 : Tin - 1;
    double* mine = is_alpha ? A : Bt;
    double v = -INFINITY;
    if (live && (is_alpha ? s < 2 : s >= S - 2)) v = E[(int64_t)t_first * ldE + ek];
    // CTC_CHUNK steps at a time: the chunk's log-probabilities are loaded and its results stored together, so the barrier of a
    // step (which waits for every outstanding global access of the wave) finds none - one memory round trip per chunk, not per step
    for (int i0 = 0; i0 < Tin; i0 += CTC_CHUNK) {
        double lpn[CTC_CHUNK], hist[CTC_CHUNK];
#pragma unroll
        for (int j = 0; j < CTC_CHUNK; ++j) {
            const int i = i0 + j;
            const int tn = is_alpha ? i + 1 : Tin - 2 - i;  // the step computed after step i's barrier
            lpn[j] = (live && i + 1 < Tin) ? E[(int64_t)tn * ldE + ek] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < CTC_CHUNK; ++j) {
            const int i = i0 + j, par = j & 1;  // (CTC_CHUNK is even: the parity of j is the parity of i)
            if (i < Tin) {                      // (uniform over the workgroup)
                hist[j] = v;
                if (is_alpha)
                    abuf[par][s + 2] = v;
                else
                    bbuf[par][s] = v;
                __syncthreads();
                if (wave_live && i + 1 < Tin) {
                    const double n1 = is_alpha ? abuf[par][s + 1] : bbuf[par][s + 1];
                    const double n2 = skip ? (is_alpha ? abuf[par][s] : bbuf[par][s + 2]) : -INFINITY;
                    v = live ? ctc_lse3(v, n1, n2) + lpn[j] : -INFINITY;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CTC_CHUNK; ++j) {
            const int i = i0 + j;
            const int t = is_alpha ? i : Tin - 1 - i;  // the step hist[j] belongs to
            if (live && i < Tin) mine[(int64_t)t * ldS + s] = hist[j];
        }
    }
    __syncthreads();

    // ---- phase 2: nll = -logaddexp(log alpha_{Tin-1}(S-1), log alpha_{Tin-1}(S-2)) ------------------------------------------
    if (tid == 0) {
        const double* al = A + (int64_t)(Tin - 1) * ldS;
        const double nll = -ctc_lse3(al[S - 1], S > 1 ? al[S - 2] : -INFINITY, -INFINITY);
        nll_sh = nll;
        sample_nll[b] = (float)nll;
        ws[b] = nll;
    }
    __syncthreads();
    if (!dlogits) return;
    const double nll = nll_sh;
    const bool feasible = nll == nll && nll != INFINITY && nll != -INFINITY;
    const double dscale = (double)scale;

    // ---- phase 3: the gradient, eight rows per round ---------------------------------------------------------------------
    for (int t0 = 0; t0 < T; t0 += 8) {
        const int t = t0 + wave;
        const bool row_live = feasible && t < Tin;
        double z0 = 0.0;
        if (row_live) {
            for (int k = lane; k < S; k += 64) {
                const double lpk = E[(int64_t)t * ldE + ((k & 1) ? 1 + (k >> 1) : 0)];
                const double w = exp((A[(int64_t)t * ldS + k] + Bt[(int64_t)t * ldS + k]) - lpk + nll);  // (-inf -> 0)
                wbuf[wave][k] = w;
                if (!(k & 1)) z0 += w;
            }
            z0 = ctc_wave_sum(z0);
        }
        __syncthreads();
        if (t < T) {
            float* __restrict__ g = dlogits + ((int64_t)t * batch + row0) * dld;
            if (row_live) {
                const float* __restrict__ x = logits + ((int64_t)t * batch + row0) * ld;
                const double l = lse[t];
                for (int c = lane; c < C; c += 64) {
                    double share = c == 0 ? z0 : 0.0;
                    for (int j = head[c]; j >= 0; j = nxt[j]) share += wbuf[wave][2 * j + 1];
                    g[c] = (float)(dscale * (exp((double)x[c] - l) - share));
                }
            } else {
                for (int c = lane; c < C; c += 64) g[c] = 0.0f;
            }
        }
        __syncthreads();
    }
}

// loss = scale * sum_b nll_b over the valid samples whose nll is finite, b ascending, in double, rounded once
__global__ void ctc_reduce_kernel(const double* __restrict__ nll, const int32_t* __restrict__ status, int batch, float scale,
                                  float* __restrict__ loss) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double acc = 0.0;
        for (int b = 0; b < batch; ++b) {
            const double v = nll[b];
            if (status[b] == 0 && v == v && v != INFINITY && v != -INFINITY) acc += v;
        }
        loss[0] = (float)((double)scale * acc);
    }
}

extern "C" int64_t wd_ctc_workspace_bytes(int T, int batch, int Lmax) {
    if (T < 1 || T > WD_CTC_MAX_T || batch < 1 || Lmax < 0 || Lmax > WD_CTC_MAX_L) return -1;
    return 8 * ((int64_t)batch + (int64_t)batch * ctc_sample_doubles(T, Lmax));
}

extern "C" int wd_ctc_loss(const float* logits, int ld, int T, int batch, int C, const void* targets, int targets_i64, int tld,
                           int Lmax, const int32_t* input_len, const int32_t* target_len, float scale, float* dlogits, int dld,
                           float* sample_nll, float* loss, int32_t* status, void* workspace, int64_t workspace_bytes,
                           void* stream) {
    if (!logits || !input_len || !target_len || !sample_nll || !loss || !status || !workspace) return WD_EINVAL;
    if (T < 1 || T > WD_CTC_MAX_T || batch < 1 || C < 1 || C > WD_CTC_MAX_C || Lmax < 0 || Lmax > WD_CTC_MAX_L) return WD_EINVAL;
    if (ld < C || (dlogits && dld < C)) return WD_EINVAL;
    if (Lmax > 0 && (!targets || tld < Lmax)) return WD_EINVAL;
    if (targets_i64 != 0 && targets_i64 != 1) return WD_EINVAL;
    if (workspace_bytes < wd_ctc_workspace_bytes(T, batch, Lmax)) return WD_EINVAL;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) || (reinterpret_cast<uintptr_t>(targets) & (targets_i64 ? 7u : 3u)) ||
        ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(dlogits) | reinterpret_cast<uintptr_t>(sample_nll) |
          reinterpret_cast<uintptr_t>(loss) | reinterpret_cast<uintptr_t>(status) | reinterpret_cast<uintptr_t>(input_len) |
          reinterpret_cast<uintptr_t>(target_len)) & 3u))
        return WD_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WdLaunchScope scope(WD_CLS_OTHER, st);
    double* ws = reinterpret_cast<double*>(workspace);
    const int64_t sd = ctc_sample_doubles(T, Lmax);
    if (targets_i64)
        hipLaunchKernelGGL(ctc_sample_kernel<true>, dim3((unsigned)batch), dim3(CTC_THREADS), 0, st, logits, ld, T, batch, C, targets,
                           tld, Lmax, input_len, target_len, scale, dlogits, dld, sample_nll, status, ws, sd);
    else
        hipLaunchKernelGGL(ctc_sample_kernel<false>, dim3((unsigned)batch), dim3(CTC_THREADS), 0, st, logits, ld, T, batch, C, targets,
                           tld, Lmax, input_len, target_len, scale, dlogits, dld, sample_nll, status, ws, sd);
    hipLaunchKernelGGL(ctc_reduce_kernel, dim3(1), dim3(64), 0, st, ws, status, batch, scale, loss);
    return wd_check_launch();
}
