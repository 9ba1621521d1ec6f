/* C ABI of libmis_hip.so, contrastive cross teaching (csrc/contrastive.hip): a header of its own beside mis_hip.h, with the
 * same conventions (device pointers, fp32, the stream last, 0 or MIS_ERR_* returned, deterministic results) and the types
 * of mis_hip.h.  The definitions are compiled against these declarations, and mis_hip/lib.py reads the ctypes prototypes
 * from this text (lib.EXTRA_HEADERS), exactly as it does for mis_hip.h. */
#ifndef MIS_HIP_CONTRASTIVE_H
#define MIS_HIP_CONTRASTIVE_H

#include "mis_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Contrastive cross teaching (code/train_Contrastive_Cross_CNN_2D.py:212-283, _CNN_ViT_2D.py the same with a Swin student).
 * mis_contrastive_cross_tail: one student's share of
 *     loss = 2 * (sup_1 + sup_2) + 0.5 * (Lc_l + Lc_u) + 1.25 * w * (ps_1 + ps_2)                              (:261)
 *   own / other = logits [B][C][S] of this student and of the other one, label [L][S] (uint8: label_bytes 1, int64: 8):
 *     ce    = CE(own[:L], label),  dice = Dice(softmax own[:L], label)
 *     ps    = Dice(softmax own[L:], argmax other[L:])          (first maximum wins; pseudo labels detached)
 *     out[0] = sup_scale * 0.5 * (ce + dice) + pseudo_scale * w * ps
 *   with w = state->cons_weight when `state` is given, else cons_weight.  The script's factors are the caller's
 *   sup_scale = 2, pseudo_scale = 1.25, extra_scale = 1 (the 0.5 of the contrastive terms is folded into mis_patch_nce's
 *   grad_scale, so that the head gradients arrive already weighted).
 *   out (>= 6 floats): out[0], ce, dice, ps, w, and out[5] = 0.5 * (ce + dice) + w * ps, the script's model{1,2}_loss (:257).
 *   dlogits [B][C][S] (may be NULL: scalars only) = d out[0] / d own, plus, in the same pass, the gradients that reach the
 *   logits through the frozen heads: extra_l [L/2][C][S] belongs to the labeled rows 0, 2, 4, ... (the classifier saw
 *   own[:L][0::2]), extra_u [B-L][C][S] to the unlabeled rows (the projector saw own[L:]):
 *     dlogits[row] = tail gradient + extra_scale * extra[row]    on those rows, the tail gradient alone on the others.
 *   Either may be NULL (both NULL: the second student, which receives no contrastive gradient).  Every element of dlogits
 *   is written exactly once; fixed-order partial sums, double in the last stage, no atomics.
 *   MIS_ERR_ARG unless 2 <= L <= B, L even, S > 0, label_bytes in {1, 8}, every batch stride >= C * S, the pointers that
 *   the geometry needs are given and extra_* come with dlogits; C outside {2, 3, 4}: MIS_ERR_UNSUPPORTED; a workspace
 *   below mis_contrastive_cross_tail_workspace_bytes: MIS_ERR_WORKSPACE.  Nothing is launched in any of these cases.
 * mis_contrastive_step_init / _advance: the schedule of these two scripts on MisStepState (mis_step_init / mis_step_advance
 *   are the Mean-Teacher one).  For the step that runs at iteration k = state->iter_num:
 *     lr          = base_lr                                                         k == 0
 *                 = 1e-4 * (1 - (i - 0.5 * max) / max * 0.5) ** 0.9                 i / max > 0.5, i = k - 1   (:274-276,
 *                 = base_lr * (1 - i / max) ** 0.9                                  otherwise           literal precedence)
 *     cons_weight = consistency * ramp_up_function(k // iters_per_epoch, rampup)    (:107-110, utils/ramps.py:30-46)
 *   ema_alpha as mis_step_advance writes it with ema_decay = 0 (unused: no teacher), cons_gate = 1.  Computed in double,
 *   stored as float.  _advance adds 1 to iter_num and to the RNG offset first.
 *   MIS_ERR_ARG unless state, max_iterations > 0, iters_per_epoch > 0, rampup >= 0. */
long long mis_contrastive_cross_tail_workspace_bytes(int B, int C, long long S);
int mis_contrastive_cross_tail(const float* own, long long s_bs, const float* other, long long o_bs, const void* label,
                               int label_bytes, int B, int L, int C, long long S, float sup_scale, float pseudo_scale,
                               float cons_weight, const MisStepState* state, const float* extra_l, long long el_bs,
                               const float* extra_u, long long eu_bs, float extra_scale, float* out, float* dlogits,
                               long long d_bs, void* workspace, long long workspace_bytes, mis_stream_t stream);
int mis_contrastive_step_init(MisStepState* state, unsigned long long seed, long long iter_num, double base_lr,
                              double max_iterations, double consistency, double rampup, long long iters_per_epoch,
                              mis_stream_t stream);
int mis_contrastive_step_advance(MisStepState* state, double base_lr, double max_iterations, double consistency,
                                 double rampup, long long iters_per_epoch, mis_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
