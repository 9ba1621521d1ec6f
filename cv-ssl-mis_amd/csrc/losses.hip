// Stand-alone loss operators of the reference's utils.losses surface (the fused training step uses
// loss_tail.hip instead; these back the drop-in ``losses.DiceLoss`` / ``losses.softmax_mse_loss``
// modules so scripts that call them directly also stay on the device) and the EMA-only update.
//
// Replaces (reference):
//   losses.DiceLoss(n_classes)(probs, target)          code/utils/losses.py:165-201
//   losses.softmax_mse_loss(input_logits, target_logits)   code/utils/losses.py:74-91
//   update_ema_variables(model, ema_model, alpha, step)     code/train_mean_teacher_2D.py:124-128
#include "tail.h"

namespace {

constexpr int NP3 = 3 * MIS_MAXC;

// partial[block][3c + {0,1,2}] = (sum p_c*[y==c], sum [y==c], sum p_c^2)
__global__ __launch_bounds__(256) void dice_partial_kernel(const float* __restrict__ p, long long p_bs,
                                                           const void* __restrict__ label, int label_bytes, int B,
                                                           int C, long long S, float* __restrict__ part) {
    __shared__ float red[4 * NP3];
    float v[NP3];
#pragma unroll
    for (int i = 0; i < NP3; ++i) v[i] = 0.f;
    const long long total = (long long)B * S;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / S);
        const long long s = i - (long long)b * S;
        const int y = mis_tail_label(label, label_bytes, i);
        const float* __restrict__ pb = p + (long long)b * p_bs + s;
#pragma unroll
        for (int c = 0; c < MIS_MAXC; ++c) {
            if (c < C) {
                const float pc = pb[(long long)c * S];
                if (c == y) { v[3 * c] += pc; v[3 * c + 1] += 1.f; }
                v[3 * c + 2] += pc * pc;
            }
        }
    }
    mis_block_sum<NP3>(v, red);
    if (threadIdx.x == 0)
        for (int i = 0; i < NP3; ++i) part[(long long)blockIdx.x * NP3 + i] = v[i];
}

// out[0] = loss, out[1+c] = class-wise dice score; coef[2c] = a_c, coef[2c+1] = b_c with
// dLoss/dp_c = a_c*[y==c] + b_c*p_c
__global__ __launch_bounds__(256) void dice_final_kernel(const float* __restrict__ part, int blocks, int C,
                                                         const float* __restrict__ weight, float* out, float* coef) {
    __shared__ double tot[NP3];
    mis_tail_reduce_parts(part, blocks, NP3, 3 * C, tot);
    if (threadIdx.x != 0) return;
    double loss = 0.0;
    for (int c = 0; c < C; ++c) {
        const double I = tot[3 * c], Y = tot[3 * c + 1], Z = tot[3 * c + 2];
        const double num = 2.0 * I + 1e-5, den = Z + Y + 1e-5;
        const double wc = weight ? (double)weight[c] : 1.0;
        loss += wc * (1.0 - num / den);
        out[1 + c] = (float)(num / den);
        coef[2 * c] = (float)(wc * (-2.0 / den) / C);
        coef[2 * c + 1] = (float)(wc * (2.0 * num / (den * den)) / C);
    }
    out[0] = (float)(loss / C);
}

__global__ __launch_bounds__(256) void dice_bwd_kernel(const float* __restrict__ p, long long p_bs,
                                                       const void* __restrict__ label, int label_bytes, int B,
                                                       int C, long long S, const float* __restrict__ coef,
                                                       const float* __restrict__ gout, float* __restrict__ dp,
                                                       long long d_bs) {
    const float g = gout[0];
    const long long total = (long long)B * S;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / S);
        const long long s = i - (long long)b * S;
        const int y = mis_tail_label(label, label_bytes, i);
        for (int c = 0; c < C; ++c) {
            const float pc = p[(long long)b * p_bs + (long long)c * S + s];
            dp[(long long)b * d_bs + (long long)c * S + s] = g * (coef[2 * c + 1] * pc + (c == y ? coef[2 * c] : 0.f));
        }
    }
}

__device__ __forceinline__ void softmax_n(const float* z, int C, float* p) {
    float mx = z[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
    float sum = 0.f;
    for (int c = 0; c < C; ++c) { p[c] = expf(z[c] - mx); sum += p[c]; }
    const float inv = 1.f / sum;
    for (int c = 0; c < C; ++c) p[c] *= inv;
}

// mode 0: out = (softmax(a) - softmax(b))^2 ; mode 1: out = d/da given gout (elementwise upstream)
__global__ __launch_bounds__(256) void softmax_mse_kernel(const float* __restrict__ a, long long a_bs,
                                                          const float* __restrict__ b, long long b_bs,
                                                          const float* __restrict__ gout, long long g_bs,
                                                          float* __restrict__ out, long long o_bs, int B, int C,
                                                          long long S, int mode) {
    const long long total = (long long)B * S;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int n = (int)(i / S);
        const long long s = i - (long long)n * S;
        float za[MIS_MAXC], zb[MIS_MAXC], p[MIS_MAXC], q[MIS_MAXC];
        for (int c = 0; c < C; ++c) {
            za[c] = a[(long long)n * a_bs + (long long)c * S + s];
            zb[c] = b[(long long)n * b_bs + (long long)c * S + s];
        }
        softmax_n(za, C, p);
        softmax_n(zb, C, q);
        if (mode == 0) {
            for (int c = 0; c < C; ++c) {
                const float d = p[c] - q[c];
                out[(long long)n * o_bs + (long long)c * S + s] = d * d;
            }
        } else {
            float h[MIS_MAXC], dot = 0.f;
            for (int c = 0; c < C; ++c) {
                h[c] = 2.f * gout[(long long)n * g_bs + (long long)c * S + s] * (p[c] - q[c]);
                dot += h[c] * p[c];
            }
            for (int c = 0; c < C; ++c) out[(long long)n * o_bs + (long long)c * S + s] = p[c] * (h[c] - dot);
        }
    }
}

__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, long long n,
                                                  float alpha) {
    const float om = 1.f - alpha;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        ema[i] = ema[i] * alpha + om * p[i];
}

int nblocks(long long total) {
    long long b = mis_cdiv(total, 256 * 4);
    if (b > 1024) b = 1024;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace

extern "C" long long mis_dice_workspace_bytes(int B, int C, long long S) {
    if (B <= 0 || C <= 0 || C > MIS_MAXC || S <= 0) return MIS_ERR_ARG;
    return ((long long)nblocks((long long)B * S) * NP3 + 2 * MIS_MAXC) * (long long)sizeof(float);
}

// probs [B][C][S], label [B][S] (u8 or i64), weight [C] or NULL.  out: 1 + C floats (device).
// The workspace keeps the per-class coefficients mis_dice_loss_bwd needs.
extern "C" int mis_dice_loss_fwd(const float* probs, long long p_bs, const void* label, int label_bytes, int B,
                                 int C, long long S, const float* weight, float* out, void* workspace,
                                 long long workspace_bytes, hipStream_t stream) {
    if (!probs || !label || !out || !workspace || B <= 0 || C <= 0 || C > MIS_MAXC || S <= 0) return MIS_ERR_ARG;
    if (label_bytes != 1 && label_bytes != 8) return MIS_ERR_ARG;
    if (workspace_bytes < mis_dice_workspace_bytes(B, C, S)) return MIS_ERR_WORKSPACE;
    const int nb = nblocks((long long)B * S);
    float* part = reinterpret_cast<float*>(workspace);
    float* coef = part + (long long)nb * NP3;
    hipLaunchKernelGGL(dice_partial_kernel, dim3(nb), dim3(256), 0, stream, probs, p_bs, label, label_bytes, B, C, S,
                       part);
    hipLaunchKernelGGL(dice_final_kernel, dim3(1), dim3(256), 0, stream, part, nb, C, weight, out, coef);
    return mis_launch_status();
}

extern "C" int mis_dice_loss_bwd(const float* probs, long long p_bs, const void* label, int label_bytes, int B,
                                 int C, long long S, const void* workspace, const float* grad_out, float* dprobs,
                                 long long d_bs, hipStream_t stream) {
    if (!probs || !label || !workspace || !grad_out || !dprobs || B <= 0 || C <= 0 || C > MIS_MAXC || S <= 0)
        return MIS_ERR_ARG;
    const int nb = nblocks((long long)B * S);
    const float* coef = reinterpret_cast<const float*>(workspace) + (long long)nb * NP3;
    hipLaunchKernelGGL(dice_bwd_kernel, dim3(nb), dim3(256), 0, stream, probs, p_bs, label, label_bytes, B, C, S,
                       coef, grad_out, dprobs, d_bs);
    return mis_launch_status();
}

extern "C" int mis_softmax_mse(const float* input_logits, long long a_bs, const float* target_logits,
                               long long b_bs, const float* grad_out, long long g_bs, float* out, long long o_bs,
                               int B, int C, long long S, int backward, hipStream_t stream) {
    if (!input_logits || !target_logits || !out || B <= 0 || C <= 0 || C > MIS_MAXC || S <= 0) return MIS_ERR_ARG;
    if (backward && !grad_out) return MIS_ERR_ARG;
    hipLaunchKernelGGL(softmax_mse_kernel, dim3(nblocks((long long)B * S)), dim3(256), 0, stream, input_logits, a_bs,
                       target_logits, b_bs, grad_out, g_bs, out, o_bs, B, C, S, backward ? 1 : 0);
    return mis_launch_status();
}

extern "C" int mis_ema_update(float* ema_param, const float* param, long long n, float alpha, hipStream_t stream) {
    if (!ema_param || !param || n <= 0) return MIS_ERR_ARG;
    hipLaunchKernelGGL(ema_kernel, dim3(nblocks(n)), dim3(256), 0, stream, ema_param, param, n, alpha);
    return mis_launch_status();
}
