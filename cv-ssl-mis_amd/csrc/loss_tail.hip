// Fused loss tail of the Mean-Teacher step: channel softmax + cross-entropy +
// Dice on the labeled half, softmax-MSE consistency on the unlabeled half, and
// the gradient of the total loss w.r.t. the student logits.
//
// Replaces (reference, one step of train_mean_teacher_2D.py:213-229 /
// train_mean_teacher_3D.py:142-158):
//   outputs_soft = torch.softmax(outputs, dim=1)
//   ema_output_soft = torch.softmax(ema_output, dim=1)
//   loss_ce   = CrossEntropyLoss()(outputs[:L], label[:L])
//   loss_dice = losses.DiceLoss(C)(outputs_soft[:L], label[:L].unsqueeze(1))   (code/utils/losses.py:165-201)
//   consistency_loss = mean((outputs_soft[L:] - ema_output_soft)**2)
//   loss = 0.5*(loss_dice + loss_ce) + consistency_weight * consistency_loss ; loss.backward()
//
// HBM-bound: pass 1 reads the logits once and produces 2 + 3C partial sums per
// workgroup (fixed-order tree, double in the last stage, no atomics and no
// per-class host sync -- the reference does C .item() syncs, losses.py:199);
// a one-workgroup finalize turns them into the four scalars and the per-class
// Dice coefficients; pass 2 re-reads the logits and writes dlogits.  The
// softmax tensors are never materialised in HBM.
#include "tail.h"

namespace {

struct TailArgs {
    const float* s; long long s_bs;      // student logits [B][C][S]
    const float* t; long long t_bs;      // teacher logits [B-L][C][S]
    const void* label;                   // [L][S], uint8 or int64
    int label_bytes;                     // 1 or 8
    int B, L, C;
    long long S;
    int blocks;                          // pass-1 grid size
};

// partial layout per block: [0]=ce_sum, [1]=mse_sum, [2+3c+0]=I_c, [2+3c+1]=Y_c, [2+3c+2]=Z_c
constexpr int NPART = 2 + 3 * MIS_MAXC;

template <int C>
__global__ __launch_bounds__(256) void tail_pass1_kernel(const TailArgs a, float* __restrict__ part) {
    __shared__ float red[4 * NPART];
    float v[NPART];
#pragma unroll
    for (int i = 0; i < NPART; ++i) v[i] = 0.f;
    const long long units = a.S >> 2;
    const long long total = (long long)a.B * units;
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
            const float* __restrict__ tb = a.t + (long long)(b - a.L) * a.t_bs + u * 4;
            float zt[4][C];
            mis_tail_load4<C>(tb, a.S, zt);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float p[C], q[C], lse;
                mis_tail_softmax<C>(z[j], p, lse);
                mis_tail_softmax<C>(zt[j], q, lse);
#pragma unroll
                for (int c = 0; c < C; ++c) { const float d = p[c] - q[c]; v[1] += d * d; }
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
// out[5..5+C) = class-wise dice score (1 - dice loss), as the reference collects them
// coef[0]=ce scale, coef[1]=mse scale, coef[2+2c]=a_c, coef[3+2c]=b_c   (see pass 2)
struct FinalArgs {
    const float* part; int blocks; int C; int L; int Bu; long long S;
    float cons_weight; const MisStepState* st; float loss_scale;
    float* out; float* coef;
};

__global__ __launch_bounds__(256) void tail_final_kernel(const FinalArgs a) {
    __shared__ double tot[NPART];
    mis_tail_reduce_parts(a.part, a.blocks, NPART, 2 + 3 * a.C, tot);
    if (threadIdx.x != 0) return;
    const double nlab = (double)a.L * (double)a.S;
    const double nun = (double)a.Bu * (double)a.C * (double)a.S;
    const float w = a.st ? a.st->cons_weight : a.cons_weight;
    const float gate = a.st ? a.st->cons_gate : 1.f;
    const double ce = a.L > 0 ? tot[0] / nlab : 0.0;
    const double mse = (a.Bu > 0 && gate != 0.f) ? tot[1] / nun : 0.0;
    double dice = 0.0;
    for (int c = 0; c < a.C; ++c) {
        double dl, ac, bc;   // d(0.5 * dice_mean)/dp_c = a_c*[y==c] + b_c*p_c
        mis_tail_dice_coef(tot[2 + 3 * c], tot[3 + 3 * c], tot[4 + 3 * c], 0.5 * a.loss_scale, a.C, dl, ac, bc);
        dice += dl;
        a.out[5 + c] = (float)(1.0 - dl);
        a.coef[2 + 2 * c] = (float)ac;
        a.coef[3 + 2 * c] = (float)bc;
    }
    dice = a.L > 0 ? dice / a.C : 0.0;
    const double loss = 0.5 * (dice + ce) + (double)w * mse;
    a.out[0] = (float)loss; a.out[1] = (float)ce; a.out[2] = (float)dice; a.out[3] = (float)mse;
    a.out[4] = w;
    a.coef[0] = a.L > 0 ? (float)(a.loss_scale * 0.5 / nlab) : 0.f;
    a.coef[1] = (a.Bu > 0 && gate != 0.f) ? (float)(a.loss_scale * (double)w * 2.0 / nun) : 0.f;
}

// dlogit_j = p_j * (g_j - sum_c g_c p_c) [+ CE term], g = dLoss/dp
template <int C>
__global__ __launch_bounds__(256) void tail_pass2_kernel(const TailArgs a, const float* __restrict__ coef,
                                                         float* __restrict__ ds, long long ds_bs) {
    const float kce = coef[0], kmse = coef[1];
    float ac[C], bc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { ac[c] = coef[2 + 2 * c]; bc[c] = coef[3 + 2 * c]; }
    const long long units = a.S >> 2;
    const long long total = (long long)a.B * units;
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
            float zt[4][C];
            mis_tail_load4<C>(tb, a.S, zt);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float p[C], q[C], g[C], lse;
                mis_tail_softmax<C>(z[j], p, lse);
                mis_tail_softmax<C>(zt[j], q, lse);
                float dot = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) { g[c] = kmse * (p[c] - q[c]); dot += g[c] * p[c]; }
#pragma unroll
                for (int c = 0; c < C; ++c) o[j][c] = p[c] * (g[c] - dot);
            }
        }
        mis_tail_store4<C>(ds + (long long)b * ds_bs + u * 4, a.S, o);
    }
}

int pass1_blocks(long long B, long long S) { return mis_tail_blocks(B * (S >> 2)); }

}  // namespace

extern "C" long long mis_loss_tail_workspace_bytes(int B, int C, long long S) {
    if (B <= 0 || C <= 0 || S <= 0) return MIS_ERR_ARG;
    return ((long long)pass1_blocks(B, S) * NPART + 2 + 2 * MIS_MAXC) * (long long)sizeof(float);
}

// out: >= 5 + C floats (device).  dlogits may be nullptr (forward only).
extern "C" int mis_loss_tail(const float* student, long long s_bs, const float* teacher, long long t_bs,
                             const void* label, int label_bytes, int B, int L, int C, long long S,
                             float cons_weight, const MisStepState* state, float loss_scale, float* out,
                             float* dlogits, long long d_bs, void* workspace, long long workspace_bytes,
                             hipStream_t stream) {
    if (!student || !out || !workspace || B <= 0 || L < 0 || L > B || C <= 0 || S <= 0) return MIS_ERR_ARG;
    if (L > 0 && !label) return MIS_ERR_ARG;
    if (B > L && !teacher) return MIS_ERR_ARG;
    if (label_bytes != 1 && label_bytes != 8) return MIS_ERR_ARG;
    if (C != 2 && C != 3 && C != 4) return MIS_ERR_UNSUPPORTED;
    if (S % 4 != 0 || s_bs % 4 != 0 || !mis_aligned16(student)) return MIS_ERR_UNSUPPORTED;
    if (teacher && (t_bs % 4 != 0 || !mis_aligned16(teacher))) return MIS_ERR_UNSUPPORTED;
    if (dlogits && (d_bs % 4 != 0 || !mis_aligned16(dlogits))) return MIS_ERR_UNSUPPORTED;
    if (workspace_bytes < mis_loss_tail_workspace_bytes(B, C, S)) return MIS_ERR_WORKSPACE;
    TailArgs a{student, s_bs, teacher, t_bs, label, label_bytes, B, L, C, S, pass1_blocks(B, S)};
    float* part = reinterpret_cast<float*>(workspace);
    float* coef = part + (long long)a.blocks * NPART;
    MIS_DISPATCH_C(C, tail_pass1_kernel, a.blocks, stream, a, part)
    FinalArgs f{part, a.blocks, C, L, B - L, S, cons_weight, state, loss_scale, out, coef};
    hipLaunchKernelGGL(tail_final_kernel, dim3(1), dim3(256), 0, stream, f);
    if (dlogits) MIS_DISPATCH_C(C, tail_pass2_kernel, a.blocks, stream, a, coef, dlogits, d_bs)
    return mis_launch_status();
}

// =====================================================================================================
// Cross-teaching loss tail (reference code/train_cross_teaching_between_cnn_transformer_2D.py:221-245):
//   loss_m = 0.5 * (CE(out_m[:L], y) + Dice(softmax(out_m)[:L], y))
//          + w * Dice(softmax(out_m)[L:], argmax(out_other[L:]))          (pseudo labels, detached)
// Same three-stage structure as the Mean-Teacher tail; the pseudo label of a voxel is the arg-max of the
// OTHER network's logits (softmax is monotone; first maximum wins like torch.argmax), computed on the fly.
// =====================================================================================================
namespace {

struct CrossArgs {
    const float* s; long long s_bs;      // own logits [B][C][S]
    const float* o; long long o_bs;      // other network's logits [B][C][S]
    const void* label; int label_bytes;  // [L][S]
    int B, L, C;
    long long S;
    int blocks;
    int pseudo_ce;                       // 1: pseudo-supervision is CE (CPS), 0: Dice (cross teaching)
    const float* t; long long t_bs;      // optional EMA-teacher logits [B-L][C][S] (train_cnn_meet_vit_2D.py), else null
};

// partial layout per block: [0]=ce_sum, [1]=pseudo-label ce_sum (pseudo_ce) or squared-error sum against the
// teacher's softmax (t != null; the two are exclusive), then 3C labeled (I,Y,Z), then 3C pseudo (I,Y,Z)
constexpr int NPARTX = 2 + 6 * MIS_MAXC;

template <int C>
__global__ __launch_bounds__(256) void cross_pass1_kernel(const CrossArgs a, float* __restrict__ part) {
    __shared__ float red[4 * NPARTX];
    float v[NPARTX];
#pragma unroll
    for (int i = 0; i < NPARTX; ++i) v[i] = 0.f;
    const long long total = (long long)a.B * a.S;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / a.S);
        const long long sidx = i - (long long)b * a.S;
        float z[C], p[C], lse;
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = a.s[(long long)b * a.s_bs + (long long)c * a.S + sidx];
        mis_tail_softmax<C>(z, p, lse);
        int y;
        if (b < a.L) {
            y = mis_tail_label(a.label, a.label_bytes, (long long)b * a.S + sidx);
        } else {
            float zo[C];
#pragma unroll
            for (int c = 0; c < C; ++c) zo[c] = a.o[(long long)b * a.o_bs + (long long)c * a.S + sidx];
            y = mis_tail_argmax<C>(zo);
        }
        // not mis_tail_labeled_sums: through it the pseudo-labeled half compiles to other fp32 code (its CE term is conditional)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const bool hit = c == y;
            if (b < a.L) {
                if (hit) { v[0] += lse - z[c]; v[2 + 3 * c] += p[c]; v[2 + 3 * c + 1] += 1.f; }
                v[2 + 3 * c + 2] += p[c] * p[c];
            } else {
                if (hit) {
                    v[2 + 3 * MIS_MAXC + 3 * c] += p[c]; v[2 + 3 * MIS_MAXC + 3 * c + 1] += 1.f;
                    if (a.pseudo_ce) v[1] += lse - z[c];
                }
                v[2 + 3 * MIS_MAXC + 3 * c + 2] += p[c] * p[c];
            }
        }
        if (b >= a.L && a.t) {
            float zt[C], q[C], lt;
#pragma unroll
            for (int c = 0; c < C; ++c) zt[c] = a.t[(long long)(b - a.L) * a.t_bs + (long long)c * a.S + sidx];
            mis_tail_softmax<C>(zt, q, lt);
#pragma unroll
            for (int c = 0; c < C; ++c) v[1] += (p[c] - q[c]) * (p[c] - q[c]);
        }
    }
    mis_block_sum<NPARTX>(v, red);
    if (threadIdx.x == 0)
        for (int i = 0; i < NPARTX; ++i) part[(long long)blockIdx.x * NPARTX + i] = v[i];
}

// out[0]=loss_m out[1]=ce out[2]=dice_sup out[3]=pseudo_dice out[4]=w; with a teacher also out[5]=mse out[6]=w_mt
// coef[0]=ce scale, coef[1+2c]=a_c, coef[2+2c]=b_c (labeled), coef[1+2C+2c], coef[2+2C+2c] (pseudo)
struct CrossFinalArgs {
    const float* part; int blocks; int C; int L; int Bu; long long S;
    float cons_weight; const MisStepState* st; float* out; float* coef; int pseudo_ce;
    int has_teacher; float mt_weight;
};

__global__ __launch_bounds__(256) void cross_final_kernel(const CrossFinalArgs a) {
    __shared__ double tot[NPARTX];
    mis_tail_reduce_parts(a.part, a.blocks, NPARTX, NPARTX, tot);
    if (threadIdx.x != 0) return;
    const float w = a.st ? a.st->cons_weight : a.cons_weight;
    const double nlab = (double)a.L * (double)a.S;
    const double ce = a.L > 0 ? tot[0] / nlab : 0.0;
    double dice_l = 0.0, dice_u = 0.0;
    for (int c = 0; c < a.C; ++c) {
        for (int half = 0; half < 2; ++half) {
            const int o = 2 + half * 3 * MIS_MAXC + 3 * c;
            const double scale = half == 0 ? 0.5 : (double)w;          // d loss / d dice_mean
            double dl, ac, bc;
            mis_tail_dice_coef(tot[o], tot[o + 1], tot[o + 2], scale, a.C, dl, ac, bc);
            (half == 0 ? dice_l : dice_u) += dl;
            a.coef[1 + half * 2 * a.C + 2 * c] = (float)ac;
            a.coef[2 + half * 2 * a.C + 2 * c] = (float)bc;
        }
    }
    dice_l = a.L > 0 ? dice_l / a.C : 0.0;
    dice_u = a.Bu > 0 ? dice_u / a.C : 0.0;
    const double nun = (double)a.Bu * (double)a.S;
    // CPS (train_cross_pseudo_supervision_{2D,3D}.py): the pseudo-supervision term is a cross-entropy
    const double pseudo = a.pseudo_ce ? (a.Bu > 0 ? tot[1] / nun : 0.0) : dice_u;
    a.out[0] = (float)(0.5 * (ce + dice_l) + (double)w * pseudo);
    a.out[1] = (float)ce; a.out[2] = (float)dice_l; a.out[3] = (float)pseudo; a.out[4] = w;
    a.coef[0] = a.L > 0 ? (float)(0.5 / nlab) : 0.f;
    a.coef[4 * MIS_MAXC] = (a.pseudo_ce && a.Bu > 0) ? (float)((double)w / nun) : 0.f;
    a.coef[4 * MIS_MAXC + 1] = 0.f;
    if (a.has_teacher) {   // + w_mt * mean((softmax(own[L:]) - softmax(teacher))^2), train_cnn_meet_vit_2D.py:326-333
        const double mse = a.Bu > 0 ? tot[1] / (nun * a.C) : 0.0;
        a.out[0] = (float)(0.5 * (ce + dice_l) + (double)w * pseudo + (double)a.mt_weight * mse);
        a.out[5] = (float)mse; a.out[6] = a.mt_weight;
        a.coef[4 * MIS_MAXC + 1] = a.Bu > 0 ? (float)(2.0 * (double)a.mt_weight / (nun * a.C)) : 0.f;
    }
}

template <int C>
__global__ __launch_bounds__(256) void cross_pass2_kernel(const CrossArgs a, const float* __restrict__ coef,
                                                          float* __restrict__ ds, long long ds_bs) {
    const float kce = coef[0], kce_u = coef[4 * MIS_MAXC], kmse = coef[4 * MIS_MAXC + 1];
    const long long total = (long long)a.B * a.S;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / a.S);
        const long long sidx = i - (long long)b * a.S;
        float z[C], p[C], g[C], lse;
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = a.s[(long long)b * a.s_bs + (long long)c * a.S + sidx];
        mis_tail_softmax<C>(z, p, lse);
        int y;
        const bool lab = b < a.L;
        if (lab) {
            y = mis_tail_label(a.label, a.label_bytes, (long long)b * a.S + sidx);
        } else {
            float zo[C];
#pragma unroll
            for (int c = 0; c < C; ++c) zo[c] = a.o[(long long)b * a.o_bs + (long long)c * a.S + sidx];
            y = mis_tail_argmax<C>(zo);
        }
        const int off = lab ? 0 : 2 * C;
        float q[C];
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = p[c];
        if (!lab && a.t) {
            float zt[C], lt;
#pragma unroll
            for (int c = 0; c < C; ++c) zt[c] = a.t[(long long)(b - a.L) * a.t_bs + (long long)c * a.S + sidx];
            mis_tail_softmax<C>(zt, q, lt);
        }
        // not mis_tail_labeled_grad: one expression serves the labeled, the pseudo-labeled and the teacher term
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            g[c] = (!lab && a.pseudo_ce) ? 0.f : coef[2 + off + 2 * c] * p[c] + (c == y ? coef[1 + off + 2 * c] : 0.f);
            g[c] += kmse * (p[c] - q[c]);     // zero without a teacher (q == p) and on the labeled half
            dot += g[c] * p[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float d = p[c] * (g[c] - dot);
            if (lab) d += kce * (p[c] - (c == y ? 1.f : 0.f));
            else if (a.pseudo_ce) d = kce_u * (p[c] - (c == y ? 1.f : 0.f));
            ds[(long long)b * ds_bs + (long long)c * a.S + sidx] = d;
        }
    }
}

int cross_blocks(long long B, long long S) { return mis_tail_blocks(B * S); }

}  // namespace

extern "C" long long mis_cross_teaching_tail_workspace_bytes(int B, int C, long long S) {
    if (B <= 0 || C <= 0 || S <= 0) return MIS_ERR_ARG;
    return ((long long)cross_blocks(B, S) * NPARTX + 2 + 4 * MIS_MAXC) * (long long)sizeof(float);
}

// out: >= 5 floats (device): loss_m, loss_ce, loss_dice, pseudo_supervision, consistency_weight
// pseudo_ce = 0: Dice against the other network's arg-max (cross teaching); 1: cross-entropy (CPS,
// code/train_cross_pseudo_supervision_3D.py:168-175, _2D.py:187-194)
//
// mis_cross_pseudo_mt_tail: the same plus a Mean-Teacher consistency term against an EMA teacher's logits on the
// unlabeled half (reference code/train_cnn_meet_vit_2D.py:300-337):
//   loss_m = 0.5*(CE + Dice) + cons_weight * Dice(softmax(own)[L:], argmax(other[L:])) + mt_weight * mean((softmax(own)[L:] - softmax(teacher))^2)
// (the script's factor 7 and its ``iter_num < 1000`` gate are folded into the two weights by the caller);
// out needs >= 7 floats: [.., 5] = consistency (MSE) loss, [6] = mt_weight.  Dice pseudo-supervision only.
extern "C" int mis_cross_pseudo_mt_tail(const float* own, long long s_bs, const float* other, long long o_bs,
                                        const float* teacher, long long t_bs, const void* label, int label_bytes,
                                        int B, int L, int C, long long S, float cons_weight, float mt_weight,
                                        const MisStepState* state, int pseudo_ce, float* out, float* dlogits,
                                        long long d_bs, void* workspace, long long workspace_bytes,
                                        hipStream_t stream) {
    if (!own || !out || !workspace || B <= 0 || L < 0 || L > B || C <= 0 || S <= 0) return MIS_ERR_ARG;
    if (teacher && pseudo_ce) return MIS_ERR_UNSUPPORTED;
    if ((L > 0 && !label) || (B > L && !other)) return MIS_ERR_ARG;
    if (label_bytes != 1 && label_bytes != 8) return MIS_ERR_ARG;
    if (C != 2 && C != 3 && C != 4) return MIS_ERR_UNSUPPORTED;
    if (workspace_bytes < mis_cross_teaching_tail_workspace_bytes(B, C, S)) return MIS_ERR_WORKSPACE;
    CrossArgs a{own, s_bs, other, o_bs, label, label_bytes, B, L, C, S, cross_blocks(B, S), pseudo_ce ? 1 : 0,
                B > L ? teacher : nullptr, t_bs};
    float* part = reinterpret_cast<float*>(workspace);
    float* coef = part + (long long)a.blocks * NPARTX;
    MIS_DISPATCH_C(C, cross_pass1_kernel, a.blocks, stream, a, part)
    CrossFinalArgs f{part, a.blocks, C, L, B - L, S, cons_weight, state, out, coef, a.pseudo_ce, a.t ? 1 : 0, mt_weight};
    hipLaunchKernelGGL(cross_final_kernel, dim3(1), dim3(256), 0, stream, f);
    if (dlogits) MIS_DISPATCH_C(C, cross_pass2_kernel, a.blocks, stream, a, coef, dlogits, d_bs)
    return mis_launch_status();
}

extern "C" int mis_cross_pseudo_tail(const float* own, long long s_bs, const float* other, long long o_bs,
                                     const void* label, int label_bytes, int B, int L, int C, long long S,
                                     float cons_weight, const MisStepState* state, int pseudo_ce, float* out,
                                     float* dlogits, long long d_bs, void* workspace, long long workspace_bytes,
                                     hipStream_t stream) {
    return mis_cross_pseudo_mt_tail(own, s_bs, other, o_bs, nullptr, 0, label, label_bytes, B, L, C, S, cons_weight, 0.f,
                                    state, pseudo_ce, out, dlogits, d_bs, workspace, workspace_bytes, stream);
}

extern "C" int mis_cross_teaching_tail(const float* own, long long s_bs, const float* other, long long o_bs,
                                       const void* label, int label_bytes, int B, int L, int C, long long S,
                                       float cons_weight, const MisStepState* state, float* out, float* dlogits,
                                       long long d_bs, void* workspace, long long workspace_bytes,
                                       hipStream_t stream) {
    return mis_cross_pseudo_tail(own, s_bs, other, o_bs, label, label_bytes, B, L, C, S, cons_weight, state, 0, out,
                                 dlogits, d_bs, workspace, workspace_bytes, stream);
}
