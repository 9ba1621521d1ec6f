// Contrastive cross teaching (reference code/train_Contrastive_Cross_CNN_2D.py:212-283 and its _CNN_ViT_ twin): the fused
// loss tail of one student and the device-side schedule of these two scripts.
//
// Replaces, per student m (other student o), one step of
//   loss_m  = 0.5 * (CE(z_m[:L], y) + Dice(softmax z_m[:L], y))                                   :220-223
//   ps_m    = Dice(softmax z_m[L:], argmax z_o[L:])                                               :225-233
//   loss    = 2 * (loss_1 + loss_2) + 0.5 * (Lc_l + Lc_u) + 1.25 * w * (ps_1 + ps_2)              :261
//   loss.backward()
// where Lc_l / Lc_u reach z_1 through the frozen classifier / projector heads (mis_patch_nce + the heads' data gradients,
// already weighted by 0.5).  The tail writes dlogits = d(2 loss_m + 1.25 w ps_m)/dz_m and adds the heads' input gradients
// on the rows that have one IN THE SAME STORE, so the [B][C][S] gradient is written once and never read back.  The script's
// factors 2 / 1.25 (/ 1 for the already weighted head gradients) are arguments, passed from ONE place:
// mis_hip.step.ContrastiveCrossTrainer.SCALES.
//
// Three stages, like every tail (tail.h): pass 1 leaves 1 + 6C fixed-order partial sums per workgroup, a one-workgroup
// finalize sums them in double and writes the scalars and the Dice coefficients, pass 2 re-reads the logits and writes
// dlogits.  One voxel per thread and iteration (any S, any batch stride >= C * S), channel planes read coalesced.
#include "tail.h"
#include "../../include/mis_hip_contrastive.h"      // the declarations of this file's entry points

namespace {

struct CcArgs {
    const float* s; long long s_bs;      // own logits [B][C][S]
    const float* o; long long o_bs;      // the other student's logits [B][C][S]
    const void* label; int label_bytes;  // [L][S]
    int B, L;
    long long S;
    const float* el; long long el_bs;    // classifier input gradient [L/2][C][S] (rows 0, 2, ... of the labeled half) or null
    const float* eu; long long eu_bs;    // projector input gradient [B-L][C][S] or null
    float extra_scale;
};

// partial layout per workgroup (stride 1 + 6C): [0] = ce_sum, [1 + 3c ..] = labeled (I, Y, Z), [1 + 3C + 3c ..] = pseudo (I, Y, Z)
template <int C>
__device__ __forceinline__ int cc_label(const CcArgs& a, int b, long long sidx) {
    if (b < a.L) return mis_tail_label(a.label, a.label_bytes, (long long)b * a.S + sidx);
    float zo[C];
#pragma unroll
    for (int c = 0; c < C; ++c) zo[c] = a.o[(long long)b * a.o_bs + (long long)c * a.S + sidx];
    return mis_tail_argmax<C>(zo);
}

template <int C>
__global__ __launch_bounds__(256) void cc_pass1_kernel(const CcArgs a, float* __restrict__ part) {
    constexpr int NP = 1 + 6 * C;
    __shared__ float red[4 * NP];
    float v[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) v[i] = 0.f;
    const long long total = (long long)a.B * a.S;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / a.S);
        const long long sidx = i - (long long)b * a.S;
        float z[C], p[C], lse;
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = a.s[(long long)b * a.s_bs + (long long)c * a.S + sidx];
        mis_tail_softmax<C>(z, p, lse);
        const int y = cc_label<C>(a, b, sidx);
        const bool lab = b < a.L;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const bool hit = c == y;
            if (lab) {
                if (hit) { v[0] += lse - z[c]; v[1 + 3 * c] += p[c]; v[1 + 3 * c + 1] += 1.f; }
                v[1 + 3 * c + 2] += p[c] * p[c];
            } else {
                if (hit) { v[1 + 3 * C + 3 * c] += p[c]; v[1 + 3 * C + 3 * c + 1] += 1.f; }
                v[1 + 3 * C + 3 * c + 2] += p[c] * p[c];
            }
        }
    }
    mis_block_sum<NP>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NP; ++i) part[(long long)blockIdx.x * NP + i] = v[i];
    }
}

// coef[0] = CE scale, coef[1 + 2c] = a_c, coef[2 + 2c] = b_c (labeled), coef[1 + 2C + 2c], coef[2 + 2C + 2c] (pseudo)
struct CcFinalArgs {
    const float* part; int blocks; int C; int L; int Bu; long long S;
    float sup_scale, pseudo_scale, cons_weight; const MisStepState* st; float* out; float* coef;
};

__global__ __launch_bounds__(256) void cc_final_kernel(const CcFinalArgs a) {
    __shared__ double tot[1 + 6 * MIS_MAXC];
    const int C = a.C, NP = 1 + 6 * C;
    mis_tail_reduce_parts(a.part, a.blocks, NP, NP, tot);
    if (threadIdx.x != 0) return;
    const float w = a.st ? a.st->cons_weight : a.cons_weight;
    const double ks = 0.5 * (double)a.sup_scale;              // d out[0] / d ce = d out[0] / d dice
    const double ku = (double)a.pseudo_scale * (double)w;     // d out[0] / d ps
    const double nlab = (double)a.L * (double)a.S;
    const double ce = tot[0] / nlab;
    double dice_l = 0.0, dice_u = 0.0;
    for (int c = 0; c < C; ++c) {
        for (int half = 0; half < 2; ++half) {
            const int o = 1 + half * 3 * C + 3 * c;
            double dl, ac, bc;
            mis_tail_dice_coef(tot[o], tot[o + 1], tot[o + 2], half == 0 ? ks : ku, C, dl, ac, bc);
            (half == 0 ? dice_l : dice_u) += dl;
            a.coef[1 + half * 2 * C + 2 * c] = (float)ac;
            a.coef[2 + half * 2 * C + 2 * c] = (float)bc;
        }
    }
    dice_l /= C;
    dice_u = a.Bu > 0 ? dice_u / C : 0.0;
    a.out[0] = (float)(ks * (ce + dice_l) + ku * dice_u);
    a.out[1] = (float)ce; a.out[2] = (float)dice_l; a.out[3] = (float)dice_u; a.out[4] = w;
    a.out[5] = (float)(0.5 * (ce + dice_l) + (double)w * dice_u);
    a.coef[0] = (float)(ks / nlab);
}

template <int C>
__global__ __launch_bounds__(256) void cc_pass2_kernel(const CcArgs a, const float* __restrict__ coef,
                                                       float* __restrict__ ds, long long ds_bs) {
    const float kce = coef[0];
    const long long total = (long long)a.B * a.S;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / a.S);
        const long long sidx = i - (long long)b * a.S;
        float z[C], p[C], g[C], lse;
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = a.s[(long long)b * a.s_bs + (long long)c * a.S + sidx];
        mis_tail_softmax<C>(z, p, lse);
        const int y = cc_label<C>(a, b, sidx);
        const bool lab = b < a.L;
        const int off = lab ? 0 : 2 * C;
        // the head gradient of this row, if it has one: the classifier saw the labeled rows 0, 2, ..., the projector every
        // unlabeled row
        const float* __restrict__ e = nullptr;
        if (lab) { if (a.el && (b & 1) == 0) e = a.el + (long long)(b >> 1) * a.el_bs + sidx; }
        else if (a.eu) e = a.eu + (long long)(b - a.L) * a.eu_bs + sidx;
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            g[c] = coef[2 + off + 2 * c] * p[c] + (c == y ? coef[1 + off + 2 * c] : 0.f);
            dot += g[c] * p[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float d = p[c] * (g[c] - dot);
            if (lab) d += kce * (p[c] - (c == y ? 1.f : 0.f));
            if (e) d += a.extra_scale * e[(long long)c * a.S];
            ds[(long long)b * ds_bs + (long long)c * a.S + sidx] = d;
        }
    }
}

int cc_blocks(long long B, long long S) { return mis_tail_blocks(B * S); }

// lr / cons_weight of the step that runs at iteration st->iter_num (see the header for the rule and its source lines)
struct CcSched { double base_lr, max_iterations, consistency, rampup; long long iters_per_epoch; };

__device__ void cc_fill_schedule(MisStepState* st, const CcSched& a) {
    const long long k = st->iter_num;
    double lr = a.base_lr;
    if (k >= 1) {
        const double it = (double)(k - 1);       // the script computes lr_ before iter_num += 1
        double f;
        if (it / a.max_iterations > 0.5) {
            f = 1.0 - (it - a.max_iterations * 0.5) / a.max_iterations * 0.5;
            lr = 0.0001;
        } else {
            f = 1.0 - it / a.max_iterations;
        }
        if (f < 0.0) f = 0.0;
        lr *= pow(f, 0.9);
    }
    st->lr = (float)lr;
    st->ema_alpha = 0.f;                         // min(1 - 1 / (k + 1), ema_decay = 0): no teacher in this method
    const double epoch = (double)(k / a.iters_per_epoch);
    double ramp = 1.0;
    if (epoch < a.rampup) {
        const double p = 1.0 - (epoch > 0.0 ? epoch : 0.0) / a.rampup;
        ramp = exp(-p * p * 5.0);
    }
    st->cons_weight = (float)(a.consistency * ramp);
    st->cons_gate = 1.f;
}

__global__ void cc_step_init_kernel(MisStepState* st, unsigned long long seed, long long iter_num, CcSched a) {
    st->seed = seed; st->offset = (unsigned long long)iter_num; st->iter_num = iter_num;
    cc_fill_schedule(st, a);
}

__global__ void cc_step_advance_kernel(MisStepState* st, CcSched a) {
    st->iter_num += 1; st->offset += 1;
    cc_fill_schedule(st, a);
}

}  // namespace

extern "C" long long mis_contrastive_cross_tail_workspace_bytes(int B, int C, long long S) {
    if (B <= 0 || C <= 0 || C > MIS_MAXC || S <= 0) return MIS_ERR_ARG;
    return ((long long)cc_blocks(B, S) * (1 + 6 * C) + 1 + 4 * C) * (long long)sizeof(float);
}

extern "C" int mis_contrastive_cross_tail(const float* own, long long s_bs, const float* other, long long o_bs,
                                          const void* label, int label_bytes, int B, int L, int C, long long S,
                                          float sup_scale, float pseudo_scale, float cons_weight,
                                          const MisStepState* state, const float* extra_l, long long el_bs,
                                          const float* extra_u, long long eu_bs, float extra_scale, float* out,
                                          float* dlogits, long long d_bs, void* workspace, long long workspace_bytes,
                                          hipStream_t stream) {
    if (!own || !out || !workspace || !label || B <= 0 || C <= 0 || S <= 0) return MIS_ERR_ARG;
    if (L < 2 || L > B || (L & 1)) return MIS_ERR_ARG;          // the classifier pairs rows 0::2 of one student with 1::2 of the other
    if (label_bytes != 1 && label_bytes != 8) return MIS_ERR_ARG;
    if (C != 2 && C != 3 && C != 4) return MIS_ERR_UNSUPPORTED;
    const long long plane = (long long)C * S;
    if (s_bs < plane || (B > L && (!other || o_bs < plane))) return MIS_ERR_ARG;
    if (dlogits && d_bs < plane) return MIS_ERR_ARG;
    if ((extra_l || extra_u) && !dlogits) return MIS_ERR_ARG;
    if ((extra_l && el_bs < plane) || (extra_u && eu_bs < plane)) return MIS_ERR_ARG;
    if (workspace_bytes < mis_contrastive_cross_tail_workspace_bytes(B, C, S)) return MIS_ERR_WORKSPACE;
    const int blocks = cc_blocks(B, S);
    CcArgs a{own, s_bs, other, o_bs, label, label_bytes, B, L, S, extra_l, el_bs, B > L ? extra_u : nullptr, eu_bs,
             extra_scale};
    float* part = reinterpret_cast<float*>(workspace);
    float* coef = part + (long long)blocks * (1 + 6 * C);
    MIS_DISPATCH_C(C, cc_pass1_kernel, blocks, stream, a, part)
    CcFinalArgs f{part, blocks, C, L, B - L, S, sup_scale, pseudo_scale, cons_weight, state, out, coef};
    hipLaunchKernelGGL(cc_final_kernel, dim3(1), dim3(256), 0, stream, f);
    if (dlogits) MIS_DISPATCH_C(C, cc_pass2_kernel, blocks, stream, a, coef, dlogits, d_bs)
    return mis_launch_status();
}

extern "C" int mis_contrastive_step_init(MisStepState* state, unsigned long long seed, long long iter_num, double base_lr,
                                         double max_iterations, double consistency, double rampup,
                                         long long iters_per_epoch, hipStream_t stream) {
    if (!state || !(max_iterations > 0) || iters_per_epoch <= 0 || !(rampup >= 0) || iter_num < 0) return MIS_ERR_ARG;
    CcSched a{base_lr, max_iterations, consistency, rampup, iters_per_epoch};
    hipLaunchKernelGGL(cc_step_init_kernel, dim3(1), dim3(1), 0, stream, state, seed, iter_num, a);
    return mis_launch_status();
}

extern "C" int mis_contrastive_step_advance(MisStepState* state, double base_lr, double max_iterations, double consistency,
                                            double rampup, long long iters_per_epoch, hipStream_t stream) {
    if (!state || !(max_iterations > 0) || iters_per_epoch <= 0 || !(rampup >= 0)) return MIS_ERR_ARG;
    CcSched a{base_lr, max_iterations, consistency, rampup, iters_per_epoch};
    hipLaunchKernelGGL(cc_step_advance_kernel, dim3(1), dim3(1), 0, stream, state, a);
    return mis_launch_status();
}
