// The tail of a transformer block in ONE launch per 64-token panel (gfx950):
//
//     h   = GEGLU(LN3(x) W1^T + b1)              FeedForward / GEGLU, reference unet.py:122-149 (unetPhosc.py:103-130)
//     x'  = x + h W2^T + b2                      BasicTransformerBlock residual, unet.py:343-344
//     out = x_in + x' Wo^T + bo   (optional)     SpatialTransformer.proj_out + residual, unet.py:406-412
//
// As three wd_gemm launches the hidden activations made a round trip through HBM as split-bf16 planes (84 MB written and read
// per layer at 64 x 8 x 32 tokens), the 2048 five-stage tiles of the first projection paid a prologue and an epilogue each, and
// the two short-K products that follow are bound by their own activation traffic.  Here a workgroup keeps its 64 normalised
// token rows resident in LDS (80 KB as split-bf16 planes), walks the hidden dimension in chunks of 128 units and never stores
// h: per chunk the 8 waves each own 16 hidden units (one x tile + one gate tile of v_mfma_f32_16x16x32_bf16, so x and gate of
// an element sit in the same lane and register), GEGLU runs on the accumulators, h goes to a 32 KB LDS image as the A operand
// of the second product, whose 64 x 320 result stays in 80 accumulator registers per wave (2 K-halves x 4 column groups, as
// in wd_gemmw_kernel) over all chunks.  Every weight is read exactly once per workgroup, straight from its FRAGMENT-MAJOR image
// (wd_gemm_pack_w) into the MFMA operand registers through a ring of six two-load groups (12 KB per wave in flight).
//
// FRONT: the panel also goes through the head of its SpatialTransformer first (base model, one block, unet.py:398-402,337-345):
// GroupNorm of the fp32 block input applied while it is staged into the resident rows, proj_in through the same ring (the
// K-half x column-group product of proj_out), both folded cross-attentions (wd_xattn.hip's arithmetic on 64 tokens instead of
// 16) and norm3 straight into the resident rows - every step is token-local and a 64-token panel of the 8 x 32 level lies in one
// sample, so the three launches of the chain and their three fp32 / plane round trips through HBM become phases of this one.
//
// FOLD (wd_ff_args.w32_*, with PROJ): nothing non-linear lies between the second product and proj_out, so
//     out = x_in + h (Wo W2)^T + x Wo^T + (Wo b2 + bo)
// with W32 = Wo W2 and b32 derived once per weight refresh (wd_linear_fold).  x Wo^T goes into the accumulators BEFORE the chunk
// loop - x is then still at hand: in the front's registers, or read from `resid` - the chunk loop adds h W32^T on top, and one
// K-half sum and the epilogue finish.  x' is never formed: no fp32 scratch of x (21 MB written, read back and written back per
// launch at 64 x 8 x 32), no in-place plane split over the image, one K-half sum instead of two; the multiply-adds are the same.
#include "wd_gemm_epi.h"

namespace {

constexpr int FNT = 512;
constexpr int FBM = 64;
constexpr int FC = 320;          // token width (model_channels of every reference configuration that reaches this kernel)
constexpr int FCH = 128;         // hidden units per chunk
constexpr int FRING = 6;         // weight-fragment groups in flight per wave
constexpr int F_MAX_INNER = 2048; // hidden width the LDS copy of b1 leaves room for (144 KB of rows and h images + 8 bytes per unit)
constexpr int FGRP = 30;         // groups per chunk: 10 k-steps x (x, gate) + 2 k-steps x 5 column tiles
constexpr uint32_t F_OOB = 0x80000000u;

typedef __attribute__((ext_vector_type(4))) unsigned f_u32x4;

__device__ __forceinline__ int f_lds_off(int row, int ch) { return row * 128 + ((ch ^ ((row >> 1) & 7)) << 4); }

// The GEMM epilogue of the launch's last product as wd_gemm_args: the bias and residual of its tail (plain: b2 + resid; proj_out: b3 +
// resid3; folded: b32 + resid3), the outputs, the statistics.  Host and device build it here, so wd_ff_fused asks
// wd_epilogue_batch_ok about the args the kernel will run.
__host__ __device__ __forceinline__ wd_gemm_args ff_epi_args(const wd_ff_args& a, const bool proj, const bool fold) {
    wd_gemm_args e = {};
    e.m = a.m;
    e.n = FC;
    e.hw_out = a.hw_out > 0 ? a.hw_out : 1;
    e.act = WD_ACT_NONE;
    e.out_f32 = a.out_f32;
    e.out_ld = a.out_ld;
    e.out_hi = a.out_hi;
    e.out_lo = a.out_lo;
    e.out_pl_ld = a.out_pl_ld;
    e.ksplit = 1;
    e.stat_part = a.stat_part;
    e.stat_cpg = a.stat_cpg;
    e.bias = !proj ? a.b2 : fold ? a.b32 : a.b3;
    e.resid = proj ? a.resid3 : a.resid;
    e.resid_ld = proj ? a.resid3_ld : a.resid_ld;
    e.dbg = a.dbg;
    return e;
}

// the finished 64 x 320 image -> the outputs: the batched form where wd_ff_fused resolved it (wd_ff_args.dbg), else the row loop
__device__ __forceinline__ void ff_epilogue(const wd_gemm_args& e, float* ep, const int m0, const int tid) {
    if ((e.dbg & WD_EPI_BATCH_BIT) && wd_epilogue_batch_ok(e, FBM, FC)) wd_epilogue_rows<FBM, FC, FNT>(e, ep, m0, 0, tid);
    else wd_epilogue_from_image<FBM, FC, FNT>(e, ep, m0, 0, tid);
}

template <int NPASS, bool PROJ, bool FRONT, bool FOLD>
__global__ void __launch_bounds__(FNT, 1) wd_ff_kernel(const wd_ff_args a) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(!FRONT || (NPASS == 3 && PROJ), "the transformer front needs split-bf16 operands and the proj_out tail");
    static_assert(!FOLD || (NPASS == 3 && PROJ), "the folded tail is the proj_out tail in split-bf16");
    constexpr int NPL = (NPASS == 1) ? 1 : 2;
    constexpr int SLAB = 2 * FBM * 128;            // one 64-deep K slab of 64 rows, both planes (plane stride FBM * 128)
    constexpr int A_BYTES = 5 * SLAB;              // the resident token rows: 320 channels
    constexpr int H_BYTES = 2 * SLAB;              // one h image: 128 hidden units
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* s_a = smem;
    char* s_h = smem + A_BYTES;                    // two h images
    float* s_b1 = reinterpret_cast<float*>(smem + A_BYTES + 2 * H_BYTES);   // b1 (2 * inner floats): a global load of the bias inside
    //                                                 the chunk loop drains the weight ring once per chunk (vmcnt counts in order)

    const int m0 = blockIdx.x * FBM;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kh = wave >> 2, cg = wave & 3;
    const int l15 = lane & 15, lq = lane >> 4;
    const int nchunk = a.inner / FCH;

    auto make_srd = [](const wd_bf16* p) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<wd_bf16*>(p), 0, 0x7FFFFFF0, 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t srd1_hi = make_srd(a.w1_hi), srd1_lo = make_srd(a.w1_lo ? a.w1_lo : a.w1_hi);
    // (FOLD: the second product runs against W32 = W3 W2, and W3 meets tok2 BEFORE the chunk loop - see the header of the file)
    const __amdgpu_buffer_rsrc_t srd2_hi = make_srd(FOLD ? a.w32_hi : a.w2_hi),
                                 srd2_lo = make_srd(FOLD ? a.w32_lo : a.w2_lo ? a.w2_lo : a.w2_hi);
    const __amdgpu_buffer_rsrc_t srd3_hi = make_srd(PROJ ? a.w3_hi : a.w2_hi), srd3_lo = make_srd(PROJ ? (a.w3_lo ? a.w3_lo : a.w3_hi) : a.w2_hi);
    const uint32_t lane16 = lane * 16;
    const int nct1 = (2 * a.inner) >> 4;          // column tiles of W1 (x / gate tiles alternate: wd_ff_fused's packing)

    // ---- the weight stream: group G of chunk j -> (descriptor, byte offset) of its two kilobytes (hi, lo)
    //   g < 20: first product, k-step g >> 1, tile (g & 1: x | gate) of this wave's 16 hidden units
    //   g >= 20: second product, k-step 4 j + 2 kh + (g - 20) / 5 of W2, column tile 5 cg + (g - 20) % 5
    bf16x8 ring[FRING][NPL];
    auto issue = [&](const int slot, const int g, const int j) {  // slot, g compile-time; j run-time (uniform)
        const bool live = j < nchunk;
        const uint32_t vo = live ? lane16 : F_OOB;
        if (PROJ && !FOLD && g < FRING) {
            // the first groups of "chunk nchunk" are the first groups of the proj_out product (k-step 2 (g / 5) + kh, tile g % 5): ONE
            // pair of loads with the descriptor and offset selected - a load inside a run-time branch makes hipcc's wait-count pass
            // assume it may not have been issued, every such branch lowers the vmcnt it dares to wait for by two, and the six of
            // them at the end of a chunk drained the ring once per chunk
            const uint32_t so3 = (uint32_t)(((2 * (g / 5) + kh) * (FC / 16) + 5 * cg + g % 5) * 1024);
            const uint32_t so1 = (uint32_t)(((g >> 1) * nct1 + 2 * (j * 8 + wave) + (g & 1)) * 1024);
            const uint32_t so = live ? so1 : so3;
#pragma unroll
            for (int p = 0; p < NPL; ++p) {
                const __amdgpu_buffer_rsrc_t srd = live ? (p ? srd1_lo : srd1_hi) : (p ? srd3_lo : srd3_hi);
                ring[slot][p] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(srd, lane16, so, 0));
            }
        } else if (g < 20) {
            const uint32_t so = (uint32_t)(((g >> 1) * nct1 + 2 * (j * 8 + wave) + (g & 1)) * 1024);
#pragma unroll
            for (int p = 0; p < NPL; ++p)
                ring[slot][p] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(p ? srd1_lo : srd1_hi, vo, live ? so : 0u, 0));
        } else {
            const int q = (g - 20) / 5, t = (g - 20) % 5;
            const uint32_t so = (uint32_t)(((4 * j + 2 * kh + q) * (FC / 16) + 5 * cg + t) * 1024);
#pragma unroll
            for (int p = 0; p < NPL; ++p)
                ring[slot][p] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(p ? srd2_lo : srd2_hi, vo, live ? so : 0u, 0));
        }
    };
    f32x4 acc2[4][5];
    bf16x8 xa[4][NPL];
    auto read_frags = [&](const char* slab_base, const int half) {  // the four row tiles of k-step `half` (0 / 1) of a 64-deep slab
        const int ch = half * 4 + lq;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ao = f_lds_off(i * 16 + l15, ch);
#pragma unroll
            for (int p = 0; p < NPL; ++p) xa[i][p] = *reinterpret_cast<const bf16x8*>(slab_base + p * (FBM * 128) + ao);
        }
    };
    auto mfma12 = [&](f32x4 (&acc)[4], const bf16x8 (&w)[NPL]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (NPL == 2) {
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[i][NPL - 1], w[0], acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[i][0], w[NPL - 1], acc[i], 0, 0, 0);
            }
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[i][0], w[0], acc[i], 0, 0, 0);
        }
    };
    // the first product with the operands swapped: the A and B fragments of v_mfma_f32_16x16x32_bf16 have the same form (lane & 15 =
    // row or column, lane >> 4 = k group), so the same registers serve, every dot product sums the same terms in the same order, and
    // only the accumulator comes out transposed: lane (l15, lq), register r = hidden unit 4 lq + r of token 16 i + l15 - four
    // K-neighbours of the second product in one lane
    auto mfma12_t = [&](f32x4 (&acc)[4], const bf16x8 (&w)[NPL]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (NPL == 2) {
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[0], xa[i][NPL - 1], acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[NPL - 1], xa[i][0], acc[i], 0, 0, 0);
            }
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[0], xa[i][0], acc[i], 0, 0, 0);
        }
    };
    constexpr int LDE = FC + 4;
    float* ep = reinterpret_cast<float*>(smem);   // [FBM][LDE] fp32 image of a finished product (over s_a and 1 KB of s_h)
    auto ksum_to_image = [&]() {  // the two K-halves of acc2 summed in a fixed order through the fp32 image (callers: barrier first)
        for (int hh = 0; hh < 2; ++hh) {
            if (kh == hh) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int t = 0; t < 5; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float* pe = ep + (i * 16 + 4 * lq + r) * LDE + cg * 80 + t * 16 + l15;
                            *pe = (hh == 0) ? acc2[i][t][r] : *pe + acc2[i][t][r];
                        }
            }
            __syncthreads();
        }
    };

    // ---- FOLD: acc2 = tok2 W3^T from the tok2 planes in the resident rows (K = 320 as ten k-steps, K-half kh takes the k-steps
    // 2 q + kh, as proj_in), BEFORE the chunk loop adds h W32^T on top.  Group g rides in ring slot (g + 5) % 6, so that the 25th
    // leaves the ring where chunk 0 expects it: the last six refills are chunk 0's first groups.
    auto issue_w3 = [&](const int slot, const int g) {
        const uint32_t so = (uint32_t)(((2 * (g / 5) + kh) * (FC / 16) + 5 * cg + g % 5) * 1024);
#pragma unroll
        for (int p = 0; p < NPL; ++p)
            ring[slot][p] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(p ? srd3_lo : srd3_hi, lane16, so, 0));
    };
    // the groups of the slabs [q0, q1), whose planes start at `slabs` (callers: the first FRING groups requested, the planes
    // complete and a barrier passed)
    auto fold_product = [&](const int q0, const int q1, const char* slabs) {
        if (q0 == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int t = 0; t < 5; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc2[i][t][r] = 0.0f;
        }
#pragma unroll
        for (int g = 0; g < 25; ++g) {
            const int q = g / 5, t = g % 5;
            if (q < q0 || q >= q1) continue;
            if (t == 0) read_frags(slabs + (q - q0) * SLAB, kh);
            {
                f32x4 col[4] = {acc2[0][t], acc2[1][t], acc2[2][t], acc2[3][t]};
                mfma12(col, ring[(g + 5) % FRING]);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc2[i][t] = col[i];
            }
            if (g + FRING < 25) issue_w3((g + 5) % FRING, g + FRING);
            else issue((g + 5) % FRING, g + FRING - 25, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    if constexpr (FRONT) {
        // ================= the transformer front: GroupNorm + proj_in, attn1, attn2, norm3 -> the resident rows =================
        constexpr int SP = 65, PP = 72, KS32 = FC / 32;
        const int b = m0 / a.hw;                                   // (hw % 64 == 0: the panel is one sample)
        const int HJ = a.heads * a.L;                              // (<= 40: the (head, key) tiles 0..2 of 16 carry data)
        char* fr = s_h + 4096;                                     // (s_h[0, 1024) lies under the fp32 image)
        float* s_aff = reinterpret_cast<float*>(fr);               // [FC][2] GroupNorm scale / shift of the sample (staging only)
        float* sS = reinterpret_cast<float*>(fr);                  // [FBM][SP] scores
        wd_bf16* sP = reinterpret_cast<wd_bf16*>(fr + FBM * SP * 4);  // [2][FBM][PP] probability planes, padding columns 0
        // the per-channel vectors of the phases below, staged once: 7 x FC floats behind the front's scratch, inside the second h
        // image (which the chunk loop first writes in chunk 1, long after norm3 has read them)
        float* s_vec = reinterpret_cast<float*>(s_h + (FOLD ? 49152 : 40960));  // (FOLD: 48 KB of tok2 planes lie in front of them)
        const float* s_pib = s_vec;
        const float* s_ln2g = s_vec + FC, * s_ln2b = s_vec + 2 * FC, * s_ln3g = s_vec + 3 * FC, * s_ln3b = s_vec + 4 * FC;
        const float* s_xba = s_vec + 5 * FC, * s_xbb = s_vec + 6 * FC;
        // ---- every request of the prologue goes out before anything waits: the panel's input rows (thread: row, 8 channels of
        // each slab), the first proj_in groups into the ring, the staged vectors and b1 - none depends on the GroupNorm table
        const int arow = tid >> 3, ach = tid & 7;
        float4 xv[5][2];
        {
            const float* xrow = a.x_in + (long)(m0 + arow) * a.x_in_ld + ach * 8;
#pragma unroll
            for (int sl = 0; sl < 5; ++sl) {
                xv[sl][0] = *reinterpret_cast<const float4*>(xrow + sl * 64);
                xv[sl][1] = *reinterpret_cast<const float4*>(xrow + sl * 64 + 4);
            }
        }
        const __amdgpu_buffer_rsrc_t srdp_hi = make_srd(a.pi_hi), srdp_lo = make_srd(a.pi_lo);
        auto issue_pi = [&](const int slot, const int g) {  // proj_in group g: k-step 2 (g / 5) + kh, column tile 5 cg + g % 5
            const uint32_t so = (uint32_t)(((2 * (g / 5) + kh) * (FC / 16) + 5 * cg + g % 5) * 1024);
#pragma unroll
            for (int p = 0; p < NPL; ++p)
                ring[slot][p] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(p ? srdp_lo : srdp_hi, lane16, so, 0));
        };
#pragma unroll
        for (int g = 0; g < FRING; ++g) issue_pi(g, g);
        // (wave v < 7 takes vector v: FC / 4 = 80 float4s, lane: its own and 64 + lane % 16, the same value from four lanes)
        const int sv = wave < 7 ? wave : 6;
        const float* vsrc = sv == 0 ? a.pi_b : sv == 1 ? a.ln2_gamma : sv == 2 ? a.ln2_beta : sv == 3 ? a.ln3_gamma : sv == 4 ? a.ln3_beta
                            : sv == 5 ? a.xb_a : a.xb_b;
        const float4 vst0 = *reinterpret_cast<const float4*>(vsrc + lane * 4);
        const float4 vst1 = *reinterpret_cast<const float4*>(vsrc + (64 + l15) * 4);
        constexpr int NB1 = 2 * F_MAX_INNER / FNT;                 // b1: units past 2 * inner (or all, without a bias) read as 0
        float b1v[NB1];
        {
            const __amdgpu_buffer_rsrc_t sb1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.b1), 0, a.b1 ? 2 * a.inner * 4 : 0, 0x00020000);
#pragma unroll
            for (int k = 0; k < NB1; ++k)
                b1v[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(sb1, (uint32_t)(tid + k * FNT) * 4u, 0, 0));
        }
        __builtin_amdgcn_sched_barrier(0);
        for (int e = tid; e < FBM * PP; e += FNT) reinterpret_cast<uint32_t*>(sP)[e] = 0u;
        // ---- GroupNorm (affine folded per channel) from the producer's partials, as wd_gemmw_kernel<..., A32>
        {
            const int ngp = FC / a.gn_pcpg, ratio = a.gn_cpg / a.gn_pcpg;
            for (int c = tid; c < FC; c += FNT) {
                const int g = c / a.gn_cpg;
                const float gam = a.gn_gamma[c], bet = a.gn_beta[c];
                // the partials of the group, k outer and chunk inner as wd_gemmw_kernel sums them, but requested eight at a time
                // (a term past the end re-reads the batch's first and is not added): one wait per batch, not one per term
                double su = 0.0, sq = 0.0;
                const int nterm = ratio * a.gn_nchunk;
                int k = 0, ck = 0;
                for (int t0 = 0; t0 < nterm; t0 += 8) {
                    const int k0 = k, ck0 = ck;
                    double2 pv[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const bool live = t0 + u < nterm;
                        const int kk = live ? k : k0, cc = live ? ck : ck0;
                        pv[u] = *reinterpret_cast<const double2*>(a.gn_part + (((long)b * a.gn_nchunk + cc) * ngp + g * ratio + kk) * 2);
                        if (++ck == a.gn_nchunk) {
                            ck = 0;
                            ++k;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (t0 + u < nterm) {
                            su += pv[u].x;
                            sq += pv[u].y;
                        }
                }
                const double n = (double)a.hw * a.gn_cpg;
                const double mu = su / n;
                double var = sq / n - mu * mu;
                if (var < 0.0) var = 0.0;
                const float rstd = (float)(1.0 / sqrt(var + (double)a.gn_eps));
                const float sc = rstd * gam;
                s_aff[2 * c] = sc;
                s_aff[2 * c + 1] = bet - (float)mu * sc;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (wave < 7) {
            *reinterpret_cast<float4*>(s_vec + sv * FC + lane * 4) = vst0;
            *reinterpret_cast<float4*>(s_vec + sv * FC + (64 + l15) * 4) = vst1;
        }
#pragma unroll
        for (int k = 0; k < NB1; ++k)
            if (tid + k * FNT < 2 * a.inner) s_b1[tid + k * FNT] = b1v[k];
        __syncthreads();
        // ---- y = x * scale + shift -> split-bf16 planes of the resident rows
#pragma unroll
        for (int sl = 0; sl < 5; ++sl) {
            const float4* tab = reinterpret_cast<const float4*>(s_aff + 2 * (sl * 64 + ach * 8));  // (sc0 sh0 sc1 sh1) ...
            const float4 t0 = tab[0], t1 = tab[1], t2 = tab[2], t3 = tab[3];
            const float4 x0 = xv[sl][0], x1 = xv[sl][1];
            float4 y0, y1;
            y0.x = x0.x * t0.x + t0.y; y0.y = x0.y * t0.z + t0.w; y0.z = x0.z * t1.x + t1.y; y0.w = x0.w * t1.z + t1.w;
            y1.x = x1.x * t2.x + t2.y; y1.y = x1.y * t2.z + t2.w; y1.z = x1.z * t3.x + t3.y; y1.w = x1.w * t3.z + t3.w;
            uint2 h0, l0, h1, l1;
            wd_split4(y0, h0, l0);
            wd_split4(y1, h1, l1);
            char* dst = s_a + sl * SLAB + f_lds_off(arow, ach);
            *reinterpret_cast<f_u32x4*>(dst) = f_u32x4{h0.x, h0.y, h1.x, h1.y};
            *reinterpret_cast<f_u32x4*>(dst + FBM * 128) = f_u32x4{l0.x, l0.y, l1.x, l1.y};
        }
        __syncthreads();
        // ---- tok = rows Wpi^T: K = 320 as ten k-steps, K-half kh takes the k-steps 2 q + kh (wd_gemmw_kernel's order)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < 5; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc2[i][t][r] = 0.0f;
#pragma unroll
        for (int g = 0; g < 25; ++g) {
            const int q = g / 5, t = g % 5;
            if (t == 0) read_frags(s_a + q * SLAB, kh);
            {
                f32x4 col[4] = {acc2[0][t], acc2[1][t], acc2[2][t], acc2[3][t]};
                mfma12(col, ring[g % FRING]);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc2[i][t] = col[i];
            }
            if (g + FRING < 25) issue_pi(g % FRING, g + FRING);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        ksum_to_image();
        // ---- the rows as quarter-wave rows (xattn16_kernel's layout): wave w holds rows 8 w + 4 pp + lq, lane l15 the float4
        // columns l15 + 16 i; tok = image + bias
        float4 xr[2][5];
#pragma unroll
        for (int pp = 0; pp < 2; ++pp)
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int n = (l15 + 16 * i) * 4, row = wave * 8 + pp * 4 + lq;
                const float4 v = *reinterpret_cast<const float4*>(ep + row * LDE + n);
                const float4 bx = *reinterpret_cast<const float4*>(s_pib + n);
                xr[pp][i] = make_float4(v.x + bx.x, v.y + bx.y, v.z + bx.z, v.w + bx.w);
            }
        __syncthreads();  // the image is read: the planes go over it
        // LayerNorm of the quarter-wave rows -> split-bf16 planes of the resident rows
        auto ln_rows = [&](const float* gamma, const float* beta) {
#pragma unroll
            for (int pp = 0; pp < 2; ++pp) {
                const int row = wave * 8 + pp * 4 + lq;
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < 5; ++i) s += (xr[pp][i].x + xr[pp][i].y) + (xr[pp][i].z + xr[pp][i].w);
                const float mean = wd_row16_sum(s) / (float)FC;
                float q = 0.f;
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const float a0 = xr[pp][i].x - mean, a1 = xr[pp][i].y - mean, a2 = xr[pp][i].z - mean, a3 = xr[pp][i].w - mean;
                    q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
                }
                const float rstd = 1.0f / sqrtf(wd_row16_sum(q) / (float)FC + a.ln_eps);
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const int n = (l15 + 16 * i) * 4;
                    const float4 ga = *reinterpret_cast<const float4*>(gamma + n);
                    const float4 be = *reinterpret_cast<const float4*>(beta + n);
                    const float4 x = xr[pp][i];
                    float4 o;
                    o.x = (x.x - mean) * rstd * ga.x + be.x; o.y = (x.y - mean) * rstd * ga.y + be.y;
                    o.z = (x.z - mean) * rstd * ga.z + be.z; o.w = (x.w - mean) * rstd * ga.w + be.w;
                    uint2 hi, lo;
                    wd_split4(o, hi, lo);
                    char* d = s_a + (n >> 6) * SLAB + f_lds_off(row, (n & 63) >> 3) + (n & 7) * 2;
                    *reinterpret_cast<uint2*>(d) = hi;
                    *reinterpret_cast<uint2*>(d + FBM * 128) = lo;
                }
            }
        };
        // ---- the two folded cross-attentions (wd_xattn.hip): wave w takes (head, key) tile w & 3 of the scores and the column
        // group w & 3 of the output, both for the row tiles 2 (w >> 2) and 2 (w >> 2) + 1
        const int ht = wave & 3, rp = wave >> 2;
        const long pq = 64L * FC;                                  // elements of one plane of one sample's folded matrix
        // the score operand depends only on the sample and the attention: requested a phase ahead (attention 1: here, acc2 is
        // dead; attention 2: after attention 1's output product, when mh / ml are dead), it lands under the LayerNorm
        bf16x8 bh[KS32], bl[KS32];
        auto issue_mq = [&](const wd_bf16* mq) {
            const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(const_cast<wd_bf16*>(mq + (long)b * 2 * pq), 0,
                                                                                (int)(2 * pq * 2), 0x00020000);
            const uint32_t vo = ht * 16 + l15 < HJ ? lane16 : F_OOB;
#pragma unroll
            for (int ks = 0; ks < KS32; ++ks) {
                bh[ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rq, vo, (uint32_t)((ht * KS32 + ks) << 10), 0));
                bl[ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rq, vo, (uint32_t)(((ht * KS32 + ks) << 10) + pq * 2), 0));
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        issue_mq(a.mq_a);
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const wd_bf16* mot = ps == 0 ? a.mot_a : a.mot_b;
            const float* xb = ps == 0 ? s_xba : s_xbb;
            ln_rows(s_ln2g, s_ln2b);  // (norm2 for both attentions, unet.py:337-345)
            __syncthreads();
            // ---- scores S[token][hj] = LN(x) . Mq^T, three split products in independent accumulators
            if (ht * 16 < HJ) {
                f32x4 a_lh[2], a_hl[2], a_hh[2];
#pragma unroll
                for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                    for (int r = 0; r < 4; ++r) a_lh[ri][r] = a_hl[ri][r] = a_hh[ri][r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS32; ++ks)
#pragma unroll
                    for (int ri = 0; ri < 2; ++ri) {
                        const char* ap = s_a + (ks >> 1) * SLAB + f_lds_off((2 * rp + ri) * 16 + l15, (ks & 1) * 4 + lq);
                        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(ap);
                        const bf16x8 al = *reinterpret_cast<const bf16x8*>(ap + FBM * 128);
                        a_lh[ri] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[ks], a_lh[ri], 0, 0, 0);
                        a_hl[ri] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[ks], a_hl[ri], 0, 0, 0);
                        a_hh[ri] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[ks], a_hh[ri], 0, 0, 0);
                    }
#pragma unroll
                for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        sS[((2 * rp + ri) * 16 + 4 * lq + r) * SP + ht * 16 + l15] = (a_lh[ri][r] + a_hl[ri][r]) + a_hh[ri][r];
            }
            __builtin_amdgcn_sched_barrier(0);
            // the operand of the output product does not depend on the softmax: requested now, it lands during the softmax
            bf16x8 mh[2][5], ml[2][5];
            {
                const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(const_cast<wd_bf16*>(mot + (long)b * 2 * pq), 0,
                                                                                    (int)(2 * pq * 2), 0x00020000);
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const uint32_t vo = ks * 32 + lq * 8 < HJ ? lane16 : F_OOB;
#pragma unroll
                    for (int t = 0; t < 5; ++t) {  // block (column tile, ks) = ((5 cg + t) 2 + ks) KB
                        const uint32_t so = (uint32_t)((((5 * cg + t) * 2 + ks) << 10));
                        mh[ks][t] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rm, vo, so, 0));
                        ml[ks][t] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rm, vo, so + (uint32_t)(pq * 2), 0));
                    }
                }
            }
            __syncthreads();
            // ---- softmax per (token, head) -> probability planes
            for (int idx = tid; idx < FBM * a.heads; idx += FNT) {
                const int t = idx / a.heads, h = idx - t * a.heads;
                const float* pr = sS + t * SP + h * a.L;
                wd_bf16* ph = sP + t * PP + h * a.L;
                // the first 10 keys stay in registers, each exponential evaluated once (a key past L re-reads the last one: no
                // effect on the maximum, not added, not stored); the sums run in key order as before
                float ex[10];
#pragma unroll
                for (int j = 0; j < 10; ++j) ex[j] = pr[j < a.L ? j : a.L - 1];
                float mx = -3.4e38f;
#pragma unroll
                for (int j = 0; j < 10; ++j) mx = fmaxf(mx, ex[j]);
                for (int j = 10; j < a.L; ++j) mx = fmaxf(mx, pr[j]);
                float sum = 0.f;
#pragma unroll
                for (int j = 0; j < 10; ++j) {
                    ex[j] = __expf(ex[j] - mx);
                    sum += j < a.L ? ex[j] : 0.f;
                }
                for (int j = 10; j < a.L; ++j) sum += __expf(pr[j] - mx);
                const float inv = __fdividef(1.f, sum);
#pragma unroll
                for (int j = 0; j < 10; ++j)
                    if (j < a.L) {
                        uint32_t hi, lo;
                        wd_split1(ex[j] * inv, hi, lo);
                        ph[j] = (wd_bf16)hi;
                        ph[FBM * PP + j] = (wd_bf16)lo;
                    }
                for (int j = 10; j < a.L; ++j) {
                    uint32_t hi, lo;
                    wd_split1(__expf(pr[j] - mx) * inv, hi, lo);
                    ph[j] = (wd_bf16)hi;
                    ph[FBM * PP + j] = (wd_bf16)lo;
                }
            }
            __syncthreads();
            // ---- output image O[token][n] = P . Mo (the token planes are dead: every wave passed the barrier after the scores)
            {
                f32x4 o[2][5];
#pragma unroll
                for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                    for (int t = 0; t < 5; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) o[ri][t][r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int ri = 0; ri < 2; ++ri) {
                        const wd_bf16* ap = sP + ((2 * rp + ri) * 16 + l15) * PP + lq * 8 + ks * 32;
                        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(ap);
                        const bf16x8 al = *reinterpret_cast<const bf16x8*>(ap + FBM * PP);
#pragma unroll
                        for (int t = 0; t < 5; ++t) o[ri][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, mh[ks][t], o[ri][t], 0, 0, 0);
#pragma unroll
                        for (int t = 0; t < 5; ++t) o[ri][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, ml[ks][t], o[ri][t], 0, 0, 0);
#pragma unroll
                        for (int t = 0; t < 5; ++t) o[ri][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, mh[ks][t], o[ri][t], 0, 0, 0);
                    }
#pragma unroll
                for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                    for (int t = 0; t < 5; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) ep[((2 * rp + ri) * 16 + 4 * lq + r) * LDE + (5 * cg + t) * 16 + l15] = o[ri][t][r];
            }
            // mh / ml / o are dead: the second attention's score operand, or (the ring is free since proj_in) the first groups of
            // chunk 0, which land under the residual add, the tok2 stores and norm3
            if (ps == 0) {
                issue_mq(a.mq_b);
            } else {
#pragma unroll
                for (int g = 0; g < FRING; ++g) {
                    if (FOLD) issue_w3((g + 5) % FRING, g);
                    else issue(g, g, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
            // ---- + bias + residual (the rows are still in registers)
#pragma unroll
            for (int pp = 0; pp < 2; ++pp)
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const int n = (l15 + 16 * i) * 4, row = wave * 8 + pp * 4 + lq;
                    const float4 bi = *reinterpret_cast<const float4*>(xb + n);
                    const float4 at = *reinterpret_cast<const float4*>(ep + row * LDE + n);
                    const float4 x = xr[pp][i];
                    xr[pp][i] = make_float4(at.x + bi.x + x.x, at.y + bi.y + x.y, at.z + bi.z + x.z, at.w + bi.w + x.w);
                }
            __syncthreads();  // the image is read: the next planes go over it
        }
        // ---- tok2 -> its scratch (the residual of the feed-forward, read back by this same wave in the x' step), norm3 -> the
        // resident rows
        if constexpr (!FOLD) {
#pragma unroll
            for (int pp = 0; pp < 2; ++pp)
#pragma unroll
                for (int i = 0; i < 5; ++i)
                    *reinterpret_cast<float4*>(a.tok2 + (long)(m0 + wave * 8 + pp * 4 + lq) * FC + (l15 + 16 * i) * 4) = xr[pp][i];
        } else {
            // tok2 is not stored (a.tok2, for debugging: buffer stores that a NULL pointer turns into out-of-range ones - no branch
            // around memory operations while the ring is in flight).  The product needs acc2, the ring and the fragments, with the
            // rows beside them the kernel spills: the rows wait in the resident rows' LDS (free until norm3; thread-private float4s,
            // [.][tid] so that a wave's accesses are contiguous) and their planes go through the h images, slabs 0-2 then 3-4
            const __amdgpu_buffer_rsrc_t st2 = __builtin_amdgcn_make_buffer_rsrc(a.tok2, 0, a.tok2 ? 0x7FFFFFF0 : 0, 0x00020000);
            float4* park = reinterpret_cast<float4*>(s_a);
            auto planes = [&](const int pp, const int i, const int i0) {
                const int n = (l15 + 16 * i) * 4, row = wave * 8 + pp * 4 + lq;
                uint2 hi, lo;
                wd_split4(xr[pp][i], hi, lo);
                char* d = s_h + (i - i0) * SLAB + f_lds_off(row, (n & 63) >> 3) + (n & 7) * 2;
                *reinterpret_cast<uint2*>(d) = hi;
                *reinterpret_cast<uint2*>(d + FBM * 128) = lo;
            };
#pragma unroll
            for (int pp = 0; pp < 2; ++pp)
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const int n = (l15 + 16 * i) * 4, row = wave * 8 + pp * 4 + lq;
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(f_u32x4, xr[pp][i]), st2, (uint32_t)(((m0 + row) * FC + n) * 4), 0, 0);
                    park[(pp * 5 + i) * FNT + tid] = xr[pp][i];
                    if (i < 3) planes(pp, i, 0);
                }
            __syncthreads();
            fold_product(0, 3, s_h);
            __syncthreads();  // every fragment read of the slabs 0-2 is done: 3-4 go over them
#pragma unroll
            for (int pp = 0; pp < 2; ++pp)
#pragma unroll
                for (int i = 3; i < 5; ++i) {
                    xr[pp][i] = park[(pp * 5 + i) * FNT + tid];
                    planes(pp, i, 3);
                }
            __syncthreads();
            fold_product(3, 5, s_h);
#pragma unroll
            for (int pp = 0; pp < 2; ++pp)
#pragma unroll
                for (int i = 0; i < 5; ++i) xr[pp][i] = park[(pp * 5 + i) * FNT + tid];
            __syncthreads();  // every row is back in its registers: norm3 goes over them
        }
        ln_rows(s_ln3g, s_ln3b);
    } else {
    // the first FRING groups go out before anything else (they have the whole prologue to land)
#pragma unroll
    for (int g = 0; g < FRING; ++g) {
        if (FOLD) issue_w3((g + 5) % FRING, g);
        else issue(g, g, 0);
    }
    if constexpr (FOLD) {
        // ---- tok2 (a.resid, fp32) -> split-bf16 planes in the resident rows, its product with W3, and only then the norm3 rows
        const int arow = tid >> 3, ach = tid & 7;
        const bool rok = m0 + arow < a.m;
        const float* xrow = a.resid + (long)(rok ? m0 + arow : 0) * a.resid_ld + ach * 8;
        float4 xv[5][2];
#pragma unroll
        for (int sl = 0; sl < 5; ++sl) {
            xv[sl][0] = *reinterpret_cast<const float4*>(xrow + sl * 64);
            xv[sl][1] = *reinterpret_cast<const float4*>(xrow + sl * 64 + 4);
        }
#pragma unroll
        for (int sl = 0; sl < 5; ++sl) {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            uint2 h0, l0, h1, l1;
            wd_split4(rok ? xv[sl][0] : z, h0, l0);
            wd_split4(rok ? xv[sl][1] : z, h1, l1);
            char* dst = s_a + sl * SLAB + f_lds_off(arow, ach);
            *reinterpret_cast<f_u32x4*>(dst) = f_u32x4{h0.x, h0.y, h1.x, h1.y};
            *reinterpret_cast<f_u32x4*>(dst + FBM * 128) = f_u32x4{l0.x, l0.y, l1.x, l1.y};
        }
        __syncthreads();
        fold_product(0, 5, s_a);
        __syncthreads();  // every fragment read of the tok2 planes is done: the norm3 rows go over them
    }

    // ---- the token rows: global planes -> LDS (5 slabs x 2 planes, 16-byte chunks, the GEMM stage image)
    {
        const __amdgpu_buffer_rsrc_t sx_hi = make_srd(a.x_hi), sx_lo = make_srd(a.x_lo ? a.x_lo : a.x_hi);
        const int arow = tid >> 3, ach = tid & 7;
        const uint32_t vo = (m0 + arow < a.m) ? (uint32_t)(m0 + arow) * (uint32_t)(a.x_ld * 2) + (uint32_t)(ach * 16) : F_OOB;
        f_u32x4 v[5][NPL];
#pragma unroll
        for (int sl = 0; sl < 5; ++sl)
#pragma unroll
            for (int p = 0; p < NPL; ++p) v[sl][p] = __builtin_amdgcn_raw_buffer_load_b128(p ? sx_lo : sx_hi, vo, sl * 128, 0);
        const int dst = f_lds_off(arow, ach);
#pragma unroll
        for (int sl = 0; sl < 5; ++sl)
#pragma unroll
            for (int p = 0; p < NPL; ++p) *reinterpret_cast<f_u32x4*>(s_a + sl * SLAB + p * (FBM * 128) + dst) = v[sl][p];
        for (int i = tid; i < 2 * a.inner; i += FNT) s_b1[i] = a.b1 ? a.b1[i] : 0.0f;
    }
    }
    __syncthreads();

    if constexpr (!FOLD) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < 5; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc2[i][t][r] = 0.0f;
    }

    // bias of this wave's hidden units (x and gate) changes per chunk: read inside the loop
    for (int j = 0; j < nchunk; ++j) {
        char* hbuf = s_h + (j & 1) * H_BYTES;
        // ---- first product: 16 hidden units (x tile, gate tile) x 64 tokens, K = 320
        f32x4 ax[4], ag[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ax[i][r] = 0.0f;
                ag[i][r] = 0.0f;
            }
#pragma unroll
        for (int g = 0; g < 20; ++g) {
            if ((g & 1) == 0) read_frags(s_a + (g >> 2) * SLAB, (g >> 1) & 1);
            if (g & 1) mfma12_t(ag, ring[g % FRING]);
            else mfma12_t(ax, ring[g % FRING]);
            // the slot is free: group g + FRING of this chunk, or of the next
            if (g + FRING < FGRP) issue(g % FRING, g + FRING, j);
            else issue(g % FRING, g + FRING - FGRP, j + 1);
            __builtin_amdgcn_sched_barrier(0);  // (else hipcc sinks the loads to just before their use: no ring left)
        }
        // ---- GEGLU on the transposed accumulators (x and gate of an element share lane and register; a lane's four registers are
        // the hidden units 4 lq .. 4 lq + 3 of one token), two values at a time, h -> LDS as split-bf16 planes: the four units are
        // eight contiguous bytes of the token's K row in each plane
        {
            const float* pb = s_b1 + (j * 8 + wave) * 32 + 4 * lq;  // biases of the x units; their gates: + 16
            const float4 bx = *reinterpret_cast<const float4*>(pb), bg = *reinterpret_cast<const float4*>(pb + 16);
            const wd_f32x2 bx01 = {bx.x, bx.y}, bx23 = {bx.z, bx.w}, bg01 = {bg.x, bg.y}, bg23 = {bg.z, bg.w};
            char* hq = hbuf + (wave >> 2) * SLAB + (lq & 1) * 8;
            const int ch = (wave & 3) * 2 + (lq >> 1);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const wd_f32x2 h01 = (wd_f32x2{ax[i][0], ax[i][1]} + bx01) * wd_gelu_erf2(wd_f32x2{ag[i][0], ag[i][1]} + bg01);
                const wd_f32x2 h23 = (wd_f32x2{ax[i][2], ax[i][3]} + bx23) * wd_gelu_erf2(wd_f32x2{ag[i][2], ag[i][3]} + bg23);
                uint2 hb, lb;
                wd_split4(make_float4(h01.x, h01.y, h23.x, h23.y), hb, lb);
                char* p = hq + f_lds_off(i * 16 + l15, ch);
                *reinterpret_cast<uint2*>(p) = hb;
                if (NPL == 2) *reinterpret_cast<uint2*>(p + FBM * 128) = lb;
            }
        }
        __syncthreads();  // h(j) complete; (the other h image was last read before the previous barrier)
        // ---- second product: this wave's K-half (two k-steps of the chunk) x its 80 output columns
#pragma unroll
        for (int g = 20; g < FGRP; ++g) {
            const int q = (g - 20) / 5, t = (g - 20) % 5;
            if (t == 0) read_frags(hbuf + kh * SLAB, q);
            {
                f32x4 col[4] = {acc2[0][t], acc2[1][t], acc2[2][t], acc2[3][t]};
                mfma12(col, ring[g % FRING]);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc2[i][t] = col[i];
            }
            if (g + FRING < FGRP) issue(g % FRING, g + FRING, j);
            else issue(g % FRING, g + FRING - FGRP, j + 1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- the two K-halves summed in a fixed order through the fp32 image, then the shared GEMM epilogue (+ b2, + x, planes / fp32)
    __syncthreads();
    ksum_to_image();
    const wd_gemm_args e = ff_epi_args(a, PROJ, FOLD);
    if constexpr (!PROJ) {
        ff_epilogue(e, ep, m0, tid);  // + b2, + resid
    } else if constexpr (FOLD) {
        ff_epilogue(e, ep, m0, tid);  // the image already is tok2 W3^T + h (W3 W2)^T: + b32 = W3 b2 + b3, + x_in
    } else {
        // ---- x' = image + b2 + x -> split-bf16 planes IN PLACE (a row's 320 floats = 1296 bytes with the pitch; its planes take
        // 2 x 640): wave w converts rows 8 w .. 8 w + 7, every read of those rows before the first write (same wave, in order)
        constexpr int ROWB = LDE * 4;
        const float* resid = FRONT ? a.tok2 : a.resid;
        const int resid_ld = FRONT ? FC : a.resid_ld;
        // (FRONT: this wave's own tok2 stores, long done - but a store and a later load are not ordered by the counters alone)
        if (FRONT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        {
            float4 v[10];
#pragma unroll
            for (int it = 0; it < 10; ++it) {
                const int idx = it * 64 + lane, row = wave * 8 + idx / 80, c = (idx % 80) * 4;
                const int m = m0 + row;
                float4 x = *reinterpret_cast<const float4*>(ep + row * LDE + c);
                if (a.b2) {
                    const float4 q = *reinterpret_cast<const float4*>(a.b2 + c);
                    x.x += q.x; x.y += q.y; x.z += q.z; x.w += q.w;
                }
                if (resid && m < a.m) {
                    const float4 q = *reinterpret_cast<const float4*>(resid + (long)m * resid_ld + c);
                    x.x += q.x; x.y += q.y; x.z += q.z; x.w += q.w;
                }
                v[it] = x;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int it = 0; it < 10; ++it) {
                const int idx = it * 64 + lane, row = wave * 8 + idx / 80, c = (idx % 80) * 4;
                uint2 hh, ll;
                wd_split4(v[it], hh, ll);
                char* rowp = reinterpret_cast<char*>(ep) + row * ROWB;
                *reinterpret_cast<uint2*>(rowp + c * 2) = hh;
                if (NPL == 2) *reinterpret_cast<uint2*>(rowp + 640 + c * 2) = ll;
            }
        }
        __syncthreads();
        // ---- out = x' Wo^T: K = 320 as ten k-steps, K-half kh takes the k-steps 2 q + kh; 25 groups through the same ring
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < 5; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc2[i][t][r] = 0.0f;
#pragma unroll
        for (int g = 0; g < 25; ++g) {
            const int q = g / 5, t = g % 5;
            if (t == 0) {
                const int ks = 2 * q + kh;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const char* rp = reinterpret_cast<const char*>(ep) + (i * 16 + l15) * ROWB + (ks * 4 + lq) * 16;
#pragma unroll
                    for (int p = 0; p < NPL; ++p) xa[i][p] = *reinterpret_cast<const bf16x8*>(rp + p * 640);
                }
            }
            {
                f32x4 col[4] = {acc2[0][t], acc2[1][t], acc2[2][t], acc2[3][t]};
                mfma12(col, ring[g % FRING]);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc2[i][t] = col[i];
            }
            if (g + FRING < 25) {
                const int g2 = g + FRING;
                const uint32_t so3 = (uint32_t)(((2 * (g2 / 5) + kh) * (FC / 16) + 5 * cg + g2 % 5) * 1024);
#pragma unroll
                for (int p = 0; p < NPL; ++p)
                    ring[g % FRING][p] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(p ? srd3_lo : srd3_hi, lane16, so3, 0));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();  // every fragment read of the planes is done: the image goes over them
        ksum_to_image();
        ff_epilogue(e, ep, m0, tid);  // + b3, + resid3
    }
#endif
}

template <int NPASS, bool PROJ, bool FRONT = false, bool FOLD = false>
int launch_ff(const wd_ff_args& a, hipStream_t st) {
    constexpr int max_smem = 5 * 2 * FBM * 128 + 2 * 2 * 2 * FBM * 128 + 2 * F_MAX_INNER * 4;  // token rows + two h images + b1
    constexpr int red_smem = FBM * (FC + 4) * 4 + WD_STAT_SCRATCH;
    static_assert(max_smem <= 160 * 1024 && red_smem <= max_smem, "LDS budget");
    const int loop_smem = max_smem - 2 * (F_MAX_INNER - a.inner) * 4;
    const int smem = loop_smem > red_smem ? loop_smem : red_smem;
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&wd_ff_kernel<NPASS, PROJ, FRONT, FOLD>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                max_smem) != hipSuccess)
            return WD_ELAUNCH;
        attr_done = true;
    }
    const int nb = (a.m + FBM - 1) / FBM;
    // (FRONT: + proj_in and the two folded attentions, scores and output: 2 x 2 (heads L) c multiply-adds per token)
    const double fl = 2.0 * (double)a.m * (3.0 * (double)a.inner * FC + (PROJ ? (double)FC * FC : 0.0) +
                                           (FRONT ? (double)FC * FC + 4.0 * a.heads * a.L * FC : 0.0));
    WdLaunchScope scope(WD_CLS_FF, st, fl);
    hipLaunchKernelGGL((wd_ff_kernel<NPASS, PROJ, FRONT, FOLD>), dim3(nb), dim3(FNT), smem, st, a);
    return wd_check_launch();
}

}  // namespace

extern "C" int wd_ff_args_bytes(void) { return (int)sizeof(wd_ff_args); }

extern "C" int wd_ff_supported(int c, int inner) { return (c == FC && inner > 0 && inner % FCH == 0 && inner <= F_MAX_INNER) ? 1 : 0; }

// Every check and decision of wd_ff_fused, host only (no HIP call): WD_OK and `a` = the args as the kernel sees them (dbg resolved:
// WD_EPI_BATCH_BIT alone says which epilogue form runs), or WD_EINVAL.
static int wd_ff_resolve(const wd_ff_args& in, wd_ff_args& a) {
    a = in;
    if (!wd_ff_supported(a.c, a.inner) || a.m <= 0 || (a.npass != 1 && a.npass != 3)) return WD_EINVAL;
    const bool front = a.x_in != nullptr;
    if (!a.w1_hi || !a.w2_hi || (a.npass == 3 && (!a.w1_lo || !a.w2_lo))) return WD_EINVAL;
    if (!front && (!a.x_hi || (a.npass == 3 && !a.x_lo) || a.x_ld % 8 || a.x_ld < a.c)) return WD_EINVAL;
    if (!a.out_f32 && !a.out_hi) return WD_EINVAL;
    if ((a.out_ld | a.resid_ld | a.out_pl_ld) & 3) return WD_EINVAL;  // the vector epilogue
    if (a.resid && a.resid_ld <= 0) return WD_EINVAL;
    if ((long)a.m * a.x_ld * 2 >= 0x7FFFFFF0L || (long)2 * a.inner * a.c * 2 >= 0x7FFFFFF0L) return WD_EINVAL;
    const bool proj = a.w3_hi != nullptr;
    const bool fold = a.w32_hi != nullptr;
    if (fold && (!proj || a.npass != 3 || !a.w32_lo || !a.b32 || (!front && !a.resid) || (long)a.m * FC * 4 >= 0x7FFFFFF0L))
        return WD_EINVAL;
    if (proj && ((a.npass == 3 && !a.w3_lo) || (a.resid3 && (a.resid3_ld <= 0 || (a.resid3_ld & 3))))) return WD_EINVAL;
    if (a.stat_part && (a.stat_cpg <= 0 || FC % a.stat_cpg || a.hw_out <= 0 || !(a.hw_out % FBM == 0 || FBM % a.hw_out == 0) ||
                        (FBM > a.hw_out && FBM / a.hw_out > WD_STAT_MAXNS)))
        return WD_EINVAL;
    if (front) {
        if (a.npass != 3 || !proj || a.x_in_ld < a.c || a.x_in_ld % 4 || a.hw <= 0 || a.hw % FBM || a.m % a.hw) return WD_EINVAL;
        if (!a.gn_part || a.gn_nchunk <= 0 || a.gn_pcpg <= 0 || a.gn_cpg <= 0 || a.gn_cpg % a.gn_pcpg || FC % a.gn_cpg ||
            !a.gn_gamma || !a.gn_beta)
            return WD_EINVAL;
        if (!a.pi_hi || !a.pi_lo || !a.pi_b || !a.ln2_gamma || !a.ln2_beta || !a.ln3_gamma || !a.ln3_beta || (!a.tok2 && !fold)) return WD_EINVAL;
        if (!a.mq_a || !a.mot_a || !a.xb_a || !a.mq_b || !a.mot_b || !a.xb_b || !wd_xattn_supported(a.c, a.heads, a.L)) return WD_EINVAL;
    }
    {
        // the batched epilogue (wd_epilogue_rows): WDIFF_EPI_BATCH (default WD_EPI_BATCH_DEFAULT) is the switch, dbg WD_EPI_BATCH_OFF /
        // _ON override it per call (wd_want_epi_batch, shared with wd_gemm); wd_epilogue_batch_ok says where it is legal
        if (wd_want_epi_batch(a.dbg) && wd_epilogue_batch_shape(ff_epi_args(a, proj, fold), FBM, FC)) a.dbg |= WD_EPI_BATCH_BIT;
    }
    return WD_OK;
}

extern "C" int wd_ff_check(const wd_ff_args* in, wd_ff_args* out) {
    if (!in) return WD_EINVAL;
    wd_ff_args a;
    const int rc = wd_ff_resolve(*in, a);
    if (rc == WD_OK && out) *out = a;
    return rc;
}

extern "C" int wd_ff_fused(const wd_ff_args* pa, void* stream) {
    if (!pa) return WD_EINVAL;
    wd_ff_args a;
    const int rc = wd_ff_resolve(*pa, a);
    if (rc != WD_OK) return rc;
    const bool front = a.x_in != nullptr, proj = a.w3_hi != nullptr, fold = a.w32_hi != nullptr;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (fold) return front ? launch_ff<3, true, true, true>(a, st) : launch_ff<3, true, false, true>(a, st);
    if (front) return launch_ff<3, true, true>(a, st);
    if (proj) return a.npass == 3 ? launch_ff<3, true>(a, st) : launch_ff<1, true>(a, st);
    return a.npass == 3 ? launch_ff<3, false>(a, st) : launch_ff<1, false>(a, st);
}
