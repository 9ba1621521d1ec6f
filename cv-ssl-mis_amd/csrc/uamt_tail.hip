// Uncertainty-aware Mean Teacher (UA-MT): the MC-dropout mean prediction and the uncertainty-masked
// consistency loss tail.
//
// Replaces (reference code/train_uncertainty_aware_mean_teacher_3D.py:148-179,
// code/train_uncertainty_aware_mean_teacher_2D.py:161-191):
//   preds = softmax(teacher(repeat(unlabeled, 2) + noise_i)) for i in 0..3          -> T = 8 predictions
//   preds = mean over T ; uncertainty = -sum_c preds * log(preds + 1e-6)
//   consistency_dist = (softmax(student[L:]) - softmax(teacher(unlabeled + noise)))**2   (losses.softmax_mse_loss)
//   threshold = (0.75 + 0.25 * sigmoid_rampup(iter_num, max_iterations)) * ln 2
//   mask = uncertainty < threshold
//   consistency_loss = sum(mask * consistency_dist) / (2 * sum(mask) + 1e-16)
//   loss = 0.5 * (CE + Dice)(labeled) + consistency_weight * consistency_loss ; loss.backward()
//
// HBM-bound, same two-pass structure as loss_tail.hip: pass 1 -> partial sums per workgroup (fixed-order
// tree, double in the last stage), one-workgroup finalize -> scalars and gradient coefficients, pass 2 ->
// dlogits.  The T softmax tensors and the uncertainty map are never materialised: each MC pass is folded
// into one running mean-probability buffer as soon as its logits exist.
#include "tail.h"

namespace {

// acc[u][c][s] = (first ? 0 : acc) + scale * sum_r softmax(logits[r*U + u])[c][s]     (R repeats in the batch)
template <int C>
__global__ __launch_bounds__(256) void softmax_mean_kernel(const float* __restrict__ logits, long long l_bs,
                                                           float* __restrict__ acc, long long a_bs, int U, int R,
                                                           long long S, float scale, int first) {
    const long long units = S >> 2, total = (long long)U * units;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int u = (int)(i / units);
        const long long q = i - (long long)u * units;
        float m[4][C];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < C; ++c) m[j][c] = 0.f;
        for (int r = 0; r < R; ++r) {
            const float* __restrict__ lb = logits + (long long)(r * U + u) * l_bs + q * 4;
            float z[4][C];
            mis_tail_load4<C>(lb, S, z);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float p[C], lse;
                mis_tail_softmax<C>(z[j], p, lse);
#pragma unroll
                for (int c = 0; c < C; ++c) m[j][c] += p[c];
            }
        }
        float* __restrict__ ab = acc + (long long)u * a_bs + q * 4;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float4 o = make_float4(scale * m[0][c], scale * m[1][c], scale * m[2][c], scale * m[3][c]);
            if (!first) {
                const float4 prev = *reinterpret_cast<const float4*>(ab + (long long)c * S);
                o.x += prev.x; o.y += prev.y; o.z += prev.z; o.w += prev.w;
            }
            *reinterpret_cast<float4*>(ab + (long long)c * S) = o;
        }
    }
}

struct UArgs {
    const float* s; long long s_bs;      // student logits [B][C][S]
    const float* t; long long t_bs;      // teacher logits [B-L][C][S] (the single noised pass)
    const float* pm; long long pm_bs;    // mean MC-dropout probabilities [B-L][C][S]
    const void* label; int label_bytes;
    int B, L, C;
    long long S;
    const MisStepState* st;
    double max_iterations;
    long long iter_num;                  // used when st == nullptr
};

// threshold of this step, as the reference computes it (float64, then compared in float32)
__device__ __forceinline__ float uamt_threshold(const UArgs& a) {
    const double it = (double)(a.st ? a.st->iter_num : a.iter_num);
    double cur = it < 0.0 ? 0.0 : (it > a.max_iterations ? a.max_iterations : it);
    const double phase = 1.0 - cur / a.max_iterations;
    const double ramp = a.max_iterations == 0.0 ? 1.0 : exp(-5.0 * phase * phase);   // ramps.sigmoid_rampup
    return (float)((0.75 + 0.25 * ramp) * 0.6931471805599453);
}

__device__ __forceinline__ float entropy_c(const float* pm, int C) {
    float e = 0.f;
    for (int c = 0; c < C; ++c) e += pm[c] * logf(pm[c] + 1e-6f);
    return -1.0f * e;
}

// partial layout per block: [0]=ce_sum, [1]=masked sq-diff sum, [2]=mask count, [3+3c..]=I_c, Y_c, Z_c
constexpr int NPART = 3 + 3 * MIS_MAXC;

template <int C>
__global__ __launch_bounds__(256) void uamt_pass1_kernel(const UArgs a, float* __restrict__ part) {
    __shared__ float red[4 * NPART];
    __shared__ float s_thr;
    if (threadIdx.x == 0) s_thr = uamt_threshold(a);
    __syncthreads();
    const float thr = s_thr;
    float v[NPART];
#pragma unroll
    for (int i = 0; i < NPART; ++i) v[i] = 0.f;
    const long long units = a.S >> 2, total = (long long)a.B * units;
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
                mis_tail_labeled_sums<C>(z[j], p, lse, y, v[0], v + 3);
            }
        } else {
            const float* __restrict__ tb = a.t + (long long)(b - a.L) * a.t_bs + u * 4;
            const float* __restrict__ mb = a.pm + (long long)(b - a.L) * a.pm_bs + u * 4;
            float zt[4][C], pm[4][C];
            mis_tail_load4<C>(tb, a.S, zt);
            mis_tail_load4<C>(mb, a.S, pm);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (entropy_c(pm[j], C) < thr) {
                    float p[C], q[C], lse;
                    mis_tail_softmax<C>(z[j], p, lse);
                    mis_tail_softmax<C>(zt[j], q, lse);
#pragma unroll
                    for (int c = 0; c < C; ++c) { const float d = p[c] - q[c]; v[1] += d * d; }
                    v[2] += 1.f;
                }
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
// out[5..5+C) = class-wise dice score, out[5+C] = number of unmasked voxels, out[6+C] = threshold
// coef[0]=ce scale, coef[1]=masked-mse scale, coef[2+2c]=a_c, coef[3+2c]=b_c
struct UFinalArgs {
    const float* part; int blocks; int C; int L; long long S;
    float cons_weight; const MisStepState* st; float loss_scale; float thr_dbg;
    float* out; float* coef;
};

__global__ __launch_bounds__(256) void uamt_final_kernel(const UFinalArgs a, const UArgs ua) {
    __shared__ double tot[NPART];
    mis_tail_reduce_parts(a.part, a.blocks, NPART, 3 + 3 * a.C, tot);
    if (threadIdx.x != 0) return;
    const double nlab = (double)a.L * (double)a.S;
    const float w = a.st ? a.st->cons_weight : a.cons_weight;
    const double ce = a.L > 0 ? tot[0] / nlab : 0.0;
    // float32 arithmetic of the reference: sum(mask*dist) / (2*sum(mask) + 1e-16)
    const double den = 2.0 * tot[2] + 1e-16;
    const double cons = tot[1] / den;
    double dice = 0.0;
    for (int c = 0; c < a.C; ++c) {
        double dl, ac, bc;
        mis_tail_dice_coef(tot[3 + 3 * c], tot[4 + 3 * c], tot[5 + 3 * c], 0.5 * a.loss_scale, a.C, dl, ac, bc);
        dice += dl;
        a.out[5 + c] = (float)(1.0 - dl);
        a.coef[2 + 2 * c] = (float)ac;
        a.coef[3 + 2 * c] = (float)bc;
    }
    dice = a.L > 0 ? dice / a.C : 0.0;
    a.out[0] = (float)(0.5 * (dice + ce) + (double)w * cons);
    a.out[1] = (float)ce; a.out[2] = (float)dice; a.out[3] = (float)cons; a.out[4] = w;
    a.out[5 + a.C] = (float)tot[2];
    a.out[6 + a.C] = uamt_threshold(ua);
    a.coef[0] = a.L > 0 ? (float)(a.loss_scale * 0.5 / nlab) : 0.f;
    a.coef[1] = (float)(a.loss_scale * (double)w * 2.0 / den);
}

template <int C>
__global__ __launch_bounds__(256) void uamt_pass2_kernel(const UArgs a, const float* __restrict__ coef,
                                                         float* __restrict__ ds, long long ds_bs) {
    __shared__ float s_thr;
    if (threadIdx.x == 0) s_thr = uamt_threshold(a);
    __syncthreads();
    const float thr = s_thr;
    const float kce = coef[0], kmse = coef[1];
    float ac[C], bc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { ac[c] = coef[2 + 2 * c]; bc[c] = coef[3 + 2 * c]; }
    const long long units = a.S >> 2, total = (long long)a.B * units;
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
                mis_tail_labeled_grad<C>(p, y, kce, ac, bc, o[j]);
            }
        } else {
            const float* __restrict__ tb = a.t + (long long)(b - a.L) * a.t_bs + u * 4;
            const float* __restrict__ mb = a.pm + (long long)(b - a.L) * a.pm_bs + u * 4;
            float zt[4][C], pm[4][C];
            mis_tail_load4<C>(tb, a.S, zt);
            mis_tail_load4<C>(mb, a.S, pm);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool keep = entropy_c(pm[j], C) < thr;
                float p[C], q[C], g[C], lse;
                mis_tail_softmax<C>(z[j], p, lse);
                mis_tail_softmax<C>(zt[j], q, lse);
                float dot = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) { g[c] = keep ? kmse * (p[c] - q[c]) : 0.f; dot += g[c] * p[c]; }
#pragma unroll
                for (int c = 0; c < C; ++c) o[j][c] = p[c] * (g[c] - dot);
            }
        }
        mis_tail_store4<C>(ds + (long long)b * ds_bs + u * 4, a.S, o);
    }
}

int nblocks(long long B, long long S) { return mis_tail_blocks(B * (S >> 2)); }

}  // namespace

extern "C" int mis_softmax_mean_accumulate(const float* logits, long long l_bs, float* acc, long long a_bs, int U,
                                           int R, int C, long long S, float scale, int first, hipStream_t stream) {
    if (!logits || !acc || U <= 0 || R <= 0 || C <= 0 || S <= 0) return MIS_ERR_ARG;
    if (C != 2 && C != 3 && C != 4) return MIS_ERR_UNSUPPORTED;
    if (S % 4 || l_bs % 4 || a_bs % 4 || !mis_aligned16(logits) || !mis_aligned16(acc)) return MIS_ERR_UNSUPPORTED;
    if (l_bs < (long long)C * S || a_bs < (long long)C * S) return MIS_ERR_ARG;
    const int nb = nblocks(U, S);
    MIS_DISPATCH_C(C, softmax_mean_kernel, nb, stream, logits, l_bs, acc, a_bs, U, R, S, scale, first)
    return mis_launch_status();
}

extern "C" long long mis_uamt_tail_workspace_bytes(int B, int C, long long S) {
    if (B <= 0 || C <= 0 || S <= 0) return MIS_ERR_ARG;
    return ((long long)nblocks(B, S) * NPART + 2 + 2 * MIS_MAXC) * (long long)sizeof(float);
}

// out: >= 7 + C floats (device).  dlogits may be nullptr (forward only).
extern "C" int mis_uamt_tail(const float* student, long long s_bs, const float* teacher, long long t_bs,
                             const float* mean_probs, long long mp_bs, const void* label, int label_bytes, int B,
                             int L, int C, long long S, float cons_weight, const MisStepState* state,
                             long long iter_num, double max_iterations, float loss_scale, float* out,
                             float* dlogits, long long d_bs, void* workspace, long long workspace_bytes,
                             hipStream_t stream) {
    if (!student || !teacher || !mean_probs || !out || !workspace || B <= 0 || L < 0 || L >= B || C <= 0 || S <= 0)
        return MIS_ERR_ARG;
    if (L > 0 && !label) return MIS_ERR_ARG;
    if (label_bytes != 1 && label_bytes != 8) return MIS_ERR_ARG;
    if (C != 2 && C != 3 && C != 4) return MIS_ERR_UNSUPPORTED;
    if (S % 4 || s_bs % 4 || t_bs % 4 || mp_bs % 4 || !mis_aligned16(student) || !mis_aligned16(teacher) || !mis_aligned16(mean_probs))
        return MIS_ERR_UNSUPPORTED;
    if (dlogits && (d_bs % 4 || !mis_aligned16(dlogits))) return MIS_ERR_UNSUPPORTED;
    if (workspace_bytes < mis_uamt_tail_workspace_bytes(B, C, S)) return MIS_ERR_WORKSPACE;
    UArgs a{student, s_bs, teacher, t_bs, mean_probs, mp_bs, label, label_bytes, B, L, C, S, state, max_iterations,
            iter_num};
    const int nb = nblocks(B, S);
    float* part = reinterpret_cast<float*>(workspace);
    float* coef = part + (long long)nb * NPART;
    MIS_DISPATCH_C(C, uamt_pass1_kernel, nb, stream, a, part)
    UFinalArgs f{part, nb, C, L, S, cons_weight, state, loss_scale, 0.f, out, coef};
    hipLaunchKernelGGL(uamt_final_kernel, dim3(1), dim3(256), 0, stream, f, a);
    if (dlogits) MIS_DISPATCH_C(C, uamt_pass2_kernel, nb, stream, a, coef, dlogits, d_bs)
    return mis_launch_status();
}
