// Interpolation Consistency Training (ICT): device Beta(a, a) mix factors, the per-sample mixup of the unlabeled
// batch and the loss tail whose consistency target is the mix of two teacher softmaxes.
//
// Replaces (reference code/train_interpolation_consistency_training_2D.py:157-188, _3D.py:146-177,
// _2D_ViT.py:198-229):
//   lam = np.random.beta(ict_alpha, ict_alpha, size=(L // 2, 1, 1, 1[, 1]))                      -> mis_beta_sample
//   x0, x1 = unlabeled[:L // 2], unlabeled[L // 2:]
//   input = cat([volume[:L], x0 * (1.0 - lam) + x1 * lam])                                        -> mis_ict_mix
//   target = softmax(ema(x0)) * (1.0 - lam) + softmax(ema(x1)) * lam
//   loss = 0.5 * (CE + Dice)(student[:L], label[:L]) + w * mean((softmax(student[L:]) - target)**2)  -> mis_ict_tail
//
// The tail has the two-pass structure of loss_tail.hip: pass 1 -> fixed-order partial sums per workgroup (double in
// the last stage), one-workgroup finalize -> scalars and gradient coefficients, pass 2 -> dlogits.  The mixed
// target is formed in registers from the two teacher logit tensors and never materialised.
#include "tail.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Beta(a, a) = X / (X + Y), X, Y ~ Gamma(a): Marsaglia-Tsang for Gamma(a + 1 >= 1), boosted to Gamma(a) by U^(1/a) when
// a < 1.  Everything stays in the log domain: at a = 0.2 the boost U^5 underflows fp32 and X / (X + Y) becomes 0 / 0.
// One lane per factor; Philox counters (factor, gamma << 24 | attempt, salt, iter) under the key (seed): a replayed
// step draws new factors every iteration with no host involvement.  At most ICT_MAX_TRIES attempts per gamma (the
// acceptance rate is > 0.95 for every shape parameter); a lane that exhausts them returns the mode d of Gamma(a + 1).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int ICT_MAX_TRIES = 64;

__device__ __forceinline__ double u01_open(uint32_t r) {          // uniform in (0, 1): never 0, never 1
    return ((double)(r >> 8) + 0.5) * (1.0 / 16777216.0);
}

__device__ double log_gamma_draw(double a, uint32_t m, uint32_t g, uint32_t salt, uint32_t it, uint32_t k0,
                                 uint32_t k1) {
    const double ab = a < 1.0 ? a + 1.0 : a;
    const double d = ab - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double lg = log(d);                                             // fallback: the mode of Gamma(ab)
    for (int t = 0; t < ICT_MAX_TRIES; ++t) {
        uint32_t r[4];
        mis_philox4(m, (g << 24) | (uint32_t)t, salt, it, k0, k1, r);
        const double u1 = u01_open(r[0]), u2 = u01_open(r[1]);
        const double x = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
        const double v0 = 1.0 + c * x;
        if (v0 <= 0.0) continue;
        const double v = v0 * v0 * v0;
        const double u = u01_open(r[2]);
        if (log(u) < 0.5 * x * x + d - d * v + d * log(v)) {
            lg = log(d) + log(v);
            break;
        }
    }
    if (a < 1.0) {                                                  // Gamma(a) = Gamma(a + 1) * U^(1/a)
        uint32_t r[4];
        mis_philox4(m, (g << 24) | 0xFFFFFFu, salt, it, k0, k1, r);
        lg += log(u01_open(r[0])) / a;
    }
    return lg;
}

__global__ __launch_bounds__(256) void beta_sample_kernel(float* __restrict__ lam, int M, double a, uint32_t salt,
                                                          const MisStepState* __restrict__ st) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const uint64_t seed = st->seed;
    const uint32_t it = (uint32_t)st->iter_num;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ (uint32_t)((uint64_t)st->iter_num >> 32);
    const double lx = log_gamma_draw(a, (uint32_t)m, 0u, salt, it, k0, k1);
    const double ly = log_gamma_draw(a, (uint32_t)m, 1u, salt, it, k0, k1);
    lam[m] = (float)(1.0 / (1.0 + exp(ly - lx)));                  // X / (X + Y), in [0, 1] for every finite lx, ly
}

// ---------------------------------------------------------------------------------------------------------------------
// out[r] = x[r] for r < L;  out[L + m] = x[L + m] * (1 - lam[m]) + x[L + M + m] * lam[m]  (n floats per sample)
// The reference's three rounded fp32 operations in its order, no contraction (this file is compiled with
// -ffp-contract=off, see the Makefile): bit-identical to the torch expression.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float mix1(float a, float b, float l) {
    return __fadd_rn(__fmul_rn(a, __fsub_rn(1.0f, l)), __fmul_rn(b, l));
}

__global__ __launch_bounds__(256) void ict_mix4_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                       const float* __restrict__ lam, int L, int M, long long n) {
    const long long units = n >> 2, total = (long long)(L + M) * units;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / units);
        const long long q = (i - (long long)r * units) * 4;
        float4 o;
        if (r < L) {
            o = *reinterpret_cast<const float4*>(x + (long long)r * n + q);
        } else {
            const int m = r - L;
            const float l = lam[m];
            const float4 a = *reinterpret_cast<const float4*>(x + (long long)(L + m) * n + q);
            const float4 b = *reinterpret_cast<const float4*>(x + (long long)(L + M + m) * n + q);
            o = make_float4(mix1(a.x, b.x, l), mix1(a.y, b.y, l), mix1(a.z, b.z, l), mix1(a.w, b.w, l));
        }
        *reinterpret_cast<float4*>(out + (long long)r * n + q) = o;
    }
}

__global__ __launch_bounds__(256) void ict_mix1_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                       const float* __restrict__ lam, int L, int M, long long n) {
    const long long total = (long long)(L + M) * n;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / n);
        const long long q = i - (long long)r * n;
        out[i] = r < L ? x[i] : mix1(x[(long long)r * n + q], x[(long long)(r + M) * n + q], lam[r - L]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// loss tail
// ---------------------------------------------------------------------------------------------------------------------
struct IArgs {
    const float* s; long long s_bs;      // student logits [L + M][C][S]
    const float* t0; long long t0_bs;    // teacher logits of x0 [M][C][S]
    const float* t1; long long t1_bs;    // teacher logits of x1 [M][C][S]
    const float* lam;                    // [M]
    const void* label; int label_bytes;  // [L][S], uint8 or int64
    int L, M, C;
    long long S;
};

// the mixed teacher target of 4 consecutive voxels of unlabeled sample m, channel-major q[j][c]
template <int C>
__device__ __forceinline__ void mixed_target(const IArgs& a, int m, long long u, float (&q)[4][C]) {
    const float* __restrict__ b0 = a.t0 + (long long)m * a.t0_bs + u * 4;
    const float* __restrict__ b1 = a.t1 + (long long)m * a.t1_bs + u * 4;
    float z0[4][C], z1[4][C];
    mis_tail_load4<C>(b0, a.S, z0);
    mis_tail_load4<C>(b1, a.S, z1);
    const float l = a.lam[m];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float p0[C], p1[C], lse;
        mis_tail_softmax<C>(z0[j], p0, lse);
        mis_tail_softmax<C>(z1[j], p1, lse);
#pragma unroll
        for (int c = 0; c < C; ++c) q[j][c] = mix1(p0[c], p1[c], l);
    }
}

// partial layout per block: [0]=ce_sum, [1]=squared-error sum, [2+3c+0]=I_c, [2+3c+1]=Y_c, [2+3c+2]=Z_c
constexpr int NPART = 2 + 3 * MIS_MAXC;

template <int C>
__global__ __launch_bounds__(256) void ict_pass1_kernel(const IArgs a, float* __restrict__ part) {
    __shared__ float red[4 * NPART];
    float v[NPART];
#pragma unroll
    for (int i = 0; i < NPART; ++i) v[i] = 0.f;
    const long long units = a.S >> 2, total = (long long)(a.L + a.M) * units;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / units);
        const long long u = i - (long long)b * units;
        const float* __restrict__ sb = a.s + (long long)b * a.s_bs + u * 4;
        float z[4][C];
        mis_tail_load4<C>(sb, a.S, z);
        if (b < a.L) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float p[C], lse;
                mis_tail_softmax<C>(z[j], p, lse);
                const int y = mis_tail_label(a.label, a.label_bytes, (long long)b * a.S + u * 4 + j);
                mis_tail_labeled_sums<C>(z[j], p, lse, y, v[0], v + 2);
            }
        } else {
            float q[4][C];
            mixed_target<C>(a, b - a.L, u, q);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float p[C], lse;
                mis_tail_softmax<C>(z[j], p, lse);
#pragma unroll
                for (int c = 0; c < C; ++c) { const float d = p[c] - q[j][c]; v[1] += d * d; }
            }
        }
    }
    mis_block_sum<NPART>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NPART; ++i) part[(long long)blockIdx.x * NPART + i] = v[i];
    }
}

// out[0]=loss out[1]=loss_ce out[2]=loss_dice out[3]=consistency_loss out[4]=consistency_weight
// out[5..5+C) = class-wise dice score (the layout of mis_loss_tail)
// coef[0]=ce scale, coef[1]=mse scale, coef[2+2c]=a_c, coef[3+2c]=b_c   (see pass 2)
struct IFinalArgs {
    const float* part; int blocks; int C; int L; int M; long long S;
    float cons_weight; const MisStepState* st; float loss_scale;
    float* out; float* coef;
};

__global__ __launch_bounds__(256) void ict_final_kernel(const IFinalArgs a) {
    __shared__ double tot[NPART];
    mis_tail_reduce_parts(a.part, a.blocks, NPART, 2 + 3 * a.C, tot);
    if (threadIdx.x != 0) return;
    const double nlab = (double)a.L * (double)a.S;
    const double nun = (double)a.M * (double)a.C * (double)a.S;
    const float w = a.st ? a.st->cons_weight : a.cons_weight;
    const float gate = a.st ? a.st->cons_gate : 1.f;
    const double ce = a.L > 0 ? tot[0] / nlab : 0.0;
    const double mse = (a.M > 0 && gate != 0.f) ? tot[1] / nun : 0.0;
    double dice = 0.0;
    for (int c = 0; c < a.C; ++c) {
        double dl, ac, bc;
        mis_tail_dice_coef(tot[2 + 3 * c], tot[3 + 3 * c], tot[4 + 3 * c], 0.5 * a.loss_scale, a.C, dl, ac, bc);
        dice += dl;
        a.out[5 + c] = (float)(1.0 - dl);
        a.coef[2 + 2 * c] = (float)ac;
        a.coef[3 + 2 * c] = (float)bc;
    }
    dice = a.L > 0 ? dice / a.C : 0.0;
    a.out[0] = (float)(0.5 * (dice + ce) + (double)w * mse);
    a.out[1] = (float)ce; a.out[2] = (float)dice; a.out[3] = (float)mse; a.out[4] = w;
    a.coef[0] = a.L > 0 ? (float)(a.loss_scale * 0.5 / nlab) : 0.f;
    a.coef[1] = (a.M > 0 && gate != 0.f) ? (float)(a.loss_scale * (double)w * 2.0 / nun) : 0.f;
}

// dlogit_j = p_j * (g_j - sum_c g_c p_c) [+ CE term], g = dLoss/dp
template <int C>
__global__ __launch_bounds__(256) void ict_pass2_kernel(const IArgs a, const float* __restrict__ coef,
                                                        float* __restrict__ ds, long long ds_bs) {
    const float kce = coef[0], kmse = coef[1];
    float ac[C], bc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { ac[c] = coef[2 + 2 * c]; bc[c] = coef[3 + 2 * c]; }
    const long long units = a.S >> 2, total = (long long)(a.L + a.M) * units;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / units);
        const long long u = i - (long long)b * units;
        const float* __restrict__ sb = a.s + (long long)b * a.s_bs + u * 4;
        float z[4][C], o[4][C];
        mis_tail_load4<C>(sb, a.S, z);
        if (b < a.L) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float p[C], lse;
                mis_tail_softmax<C>(z[j], p, lse);
                const int y = mis_tail_label(a.label, a.label_bytes, (long long)b * a.S + u * 4 + j);
                // not mis_tail_labeled_grad: its fmaf would fuse a product that this file, built without contraction, rounds
                float g[C], dot = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    g[c] = bc[c] * p[c] + (c == y ? ac[c] : 0.f);
                    dot += g[c] * p[c];
                }
#pragma unroll
                for (int c = 0; c < C; ++c)
                    o[j][c] = p[c] * (g[c] - dot) + kce * (p[c] - (c == y ? 1.f : 0.f));
            }
        } else {
            float q[4][C];
            mixed_target<C>(a, b - a.L, u, q);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float p[C], g[C], lse;
                mis_tail_softmax<C>(z[j], p, lse);
                float dot = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) { g[c] = kmse * (p[c] - q[j][c]); dot += g[c] * p[c]; }
#pragma unroll
                for (int c = 0; c < C; ++c) o[j][c] = p[c] * (g[c] - dot);
            }
        }
        mis_tail_store4<C>(ds + (long long)b * ds_bs + u * 4, a.S, o);
    }
}

int nblocks(long long B, long long S) { return mis_tail_blocks(B * (S >> 2)); }

}  // namespace

extern "C" int mis_beta_sample(float* lam, int M, double alpha, unsigned salt, const MisStepState* state,
                               hipStream_t stream) {
    if (!lam || !state || M <= 0 || !(alpha > 0.0)) return MIS_ERR_ARG;
    hipLaunchKernelGGL(beta_sample_kernel, dim3((unsigned)mis_cdiv(M, 256)), dim3(256), 0, stream, lam, M, alpha,
                       (uint32_t)salt, state);
    return mis_launch_status();
}

extern "C" int mis_ict_mix(const float* x, float* out, const float* lam, int L, int M, long long n,
                           hipStream_t stream) {
    if (!x || !out || !lam || L < 0 || M <= 0 || n <= 0) return MIS_ERR_ARG;
    const bool vec = n % 4 == 0 && mis_aligned16(x) && mis_aligned16(out);
    const long long work = (long long)(L + M) * (vec ? n >> 2 : n);
    long long nb = mis_cdiv(work, 256);
    if (nb > 4096) nb = 4096;
    if (vec)
        hipLaunchKernelGGL(ict_mix4_kernel, dim3((unsigned)nb), dim3(256), 0, stream, x, out, lam, L, M, n);
    else
        hipLaunchKernelGGL(ict_mix1_kernel, dim3((unsigned)nb), dim3(256), 0, stream, x, out, lam, L, M, n);
    return mis_launch_status();
}

extern "C" long long mis_ict_tail_workspace_bytes(int B, int C, long long S) {
    if (B <= 0 || C <= 0 || S <= 0) return MIS_ERR_ARG;
    return ((long long)nblocks(B, S) * NPART + 2 + 2 * MIS_MAXC) * (long long)sizeof(float);
}

// student: [L + M][C][S]; teacher0 / teacher1: [M][C][S]; out >= 5 + C floats (device).  dlogits may be nullptr.
extern "C" int mis_ict_tail(const float* student, long long s_bs, const float* teacher0, long long t0_bs,
                            const float* teacher1, long long t1_bs, const float* lam, const void* label,
                            int label_bytes, int L, int M, int C, long long S, float cons_weight,
                            const MisStepState* state, float loss_scale, float* out, float* dlogits, long long d_bs,
                            void* workspace, long long workspace_bytes, hipStream_t stream) {
    if (!student || !out || !workspace || L < 0 || M < 0 || L + M <= 0 || C <= 0 || S <= 0) return MIS_ERR_ARG;
    if (L > 0 && !label) return MIS_ERR_ARG;
    if (M > 0 && (!teacher0 || !teacher1 || !lam)) return MIS_ERR_ARG;
    if (label_bytes != 1 && label_bytes != 8) return MIS_ERR_ARG;
    if (C != 2 && C != 3 && C != 4) return MIS_ERR_UNSUPPORTED;
    if (S % 4 || s_bs % 4 || !mis_aligned16(student)) return MIS_ERR_UNSUPPORTED;
    if (s_bs < (long long)C * S) return MIS_ERR_ARG;
    if (M > 0 && (t0_bs % 4 || t1_bs % 4 || !mis_aligned16(teacher0) || !mis_aligned16(teacher1))) return MIS_ERR_UNSUPPORTED;
    if (M > 0 && (t0_bs < (long long)C * S || t1_bs < (long long)C * S)) return MIS_ERR_ARG;
    if (dlogits && (d_bs % 4 || !mis_aligned16(dlogits) || d_bs < (long long)C * S)) return MIS_ERR_UNSUPPORTED;
    if (workspace_bytes < mis_ict_tail_workspace_bytes(L + M, C, S)) return MIS_ERR_WORKSPACE;
    IArgs a{student, s_bs, teacher0, t0_bs, teacher1, t1_bs, lam, label, label_bytes, L, M, C, S};
    const int nb = nblocks(L + M, S);
    float* part = reinterpret_cast<float*>(workspace);
    float* coef = part + (long long)nb * NPART;
    MIS_DISPATCH_C(C, ict_pass1_kernel, nb, stream, a, part)
    IFinalArgs f{part, nb, C, L, M, S, cons_weight, state, loss_scale, out, coef};
    hipLaunchKernelGGL(ict_final_kernel, dim3(1), dim3(256), 0, stream, f);
    if (dlogits) MIS_DISPATCH_C(C, ict_pass2_kernel, nb, stream, a, coef, dlogits, d_bs)
    return mis_launch_status();
}
