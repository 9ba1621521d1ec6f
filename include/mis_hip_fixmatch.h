/* C ABI of libmis_hip.so, FixMatch family (csrc/fixmatch.hip): a header of its own beside mis_hip.h, with the same
 * conventions (device pointers, fp32, the stream last, 0 or MIS_ERR_* returned, deterministic results) and the types of
 * mis_hip.h.  The definitions are compiled against these declarations, and mis_hip/lib.py reads the ctypes prototypes from
 * this text (lib.EXTRA_HEADERS), exactly as it does for mis_hip.h. */
#ifndef MIS_HIP_FIXMATCH_H
#define MIS_HIP_FIXMATCH_H

#include "mis_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* FixMatch with complementary learning (code/train_Fixmatch_CNN_2D.py:132-166, :259-288; dataloaders/dataset.py:99-107).
 * mis_color_jitter: y = ColorJitter(0.8, 0.8, 0.8, 0.2)(x) for one-channel float images x [B][1][S] (saturation and hue
 *   leave one channel unchanged): per image, in the order `order` says, brightness clamp(beta * x, 0, 1) and contrast
 *   clamp(gamma * x + (1 - gamma) * mean(x), 0, 1), mean(x) of the image as it stands then.  params ([B][3] floats: beta,
 *   gamma, order; order 0 = brightness first) gives the factors, or, when NULL, they are drawn on the device: beta, gamma
 *   ~ U[0.2, 1.8], order a fair bit, Philox4x32-10 keyed by (state->seed, state->iter_num, salt, sample).  drawn ([B][3],
 *   may be NULL) receives the factors used.  The mean is a fixed-order sum over 4096-pixel chunks, whatever the grid.
 * mis_fixmatch_tail: weak / strong = logits [B][C][S] of ONE network on the weak and the strong batch, pw / ps their
 *   softmaxes; label [L][S].  With pseudo = argmax_c(pw_c * [(pw_c - min pw) / max pw > conf_thresh]) on rows >= L and
 *   comp = argmin_c pw_c on all rows (first extremum wins, both detached):
 *     sup   = CE(weak[:L], label) + Dice(pw[:L], label)
 *     a     = mean_{b,c}(1 - H_bc / ln S),  H_bc = -sum_s q log(clamp(q, 2^-23, 1 - 2^-23)),  q = ps[b,c,:] / sum_s ps[b,c,s]
 *     unsup = CE(strong[L:], pseudo) + Dice(ps[L:], pseudo) + a^2 * CE(1 - ps, comp)
 *     loss  = sup + w * unsup,   w = state->cons_weight when `state` is given, else cons_weight (no gate)
 *   out (>= 10 floats): loss, sup_ce, sup_dice, unsup, w, ce_u, dice_u, ce_comp, a, share of the unlabeled pixels where the
 *   mask kept a class.  d_weak / d_strong = dloss/dlogits (a is differentiated through; d_weak rows >= L are written as
 *   zeros); either may be NULL.  pseudo ([B-L][S]) / comp ([B][S]): the decisions as uint8 maps, may be NULL.
 *   MIS_ERR_ARG unless 1 <= L < B and S > 1; C outside {2, 3, 4}: MIS_ERR_UNSUPPORTED.  float4 path when S % 4 == 0 and
 *   every pointer / batch stride is 16-byte aligned, scalar path otherwise. */
long long mis_color_jitter_workspace_bytes(int B, long long S);
int mis_color_jitter(const float* x, long long x_bs, float* y, long long y_bs, int B, long long S, const float* params,
                     const MisStepState* state, unsigned salt, float* drawn, void* workspace, long long workspace_bytes,
                     mis_stream_t stream);
long long mis_fixmatch_tail_workspace_bytes(int B, int C, long long S);
int mis_fixmatch_tail(const float* weak, long long w_bs, const float* strong, long long s_bs, const void* label,
                      int label_bytes, int B, int L, int C, long long S, float conf_thresh, float cons_weight,
                      const MisStepState* state, float* out, float* d_weak, long long dw_bs, float* d_strong,
                      long long ds_bs, unsigned char* pseudo, unsigned char* comp, void* workspace,
                      long long workspace_bytes, mis_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
