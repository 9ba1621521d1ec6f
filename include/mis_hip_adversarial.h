/* C ABI of libmis_hip.so, adversarial training of the 3-D nets (csrc/adversarial.hip): the discriminator's kernel-4 /
 * stride-2 convolutions, its pool + linear + cross-entropy head, the segmenter's loss tail and Adam.  A header of its own
 * beside mis_hip.h, with the same conventions (device pointers, fp32, NCDHW with free batch strides, the stream last, 0 or
 * MIS_ERR_* returned before anything is launched, run-to-run bit-identical results, no floating-point atomics) and the types
 * of mis_hip.h.  The definitions are compiled against these declarations, and mis_hip/lib.py reads the ctypes prototypes
 * from this text (lib.EXTRA_HEADERS).
 *
 * Reference: code/networks/discriminator.py:6-55 (FC3DDiscriminator), code/train_adversarial_network_3D.py:129-175. */
#ifndef MIS_HIP_ADVERSARIAL_H
#define MIS_HIP_ADVERSARIAL_H

#include "mis_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nn.Dropout3d(p): scale[n * C + c] = 0 or 1 / (1 - p), one Bernoulli draw per (n, c) from Philox(state->seed,
 * state->offset, salt, n * C + c) -- the draw of mis_norm_act_fwd's channel mode.  The convolutions below take the array
 * (forward, data gradient and weight gradient read the same decision); a parity test writes the array itself. */
int mis_channel_dropout_scale(float* scale, int N, int C, float p, unsigned salt, const MisStepState* state,
                              mis_stream_t stream);

/* nn.Conv3d(Cin, Cout, kernel_size = 4, stride = 2, padding = 1) on v_mfma_f32_16x16x4_f32, with the discriminator's
 * epilogue:   y = drop(leaky_relu(bias + bias2 + conv(in), slope)).
 *
 * (D, H, W) is the INPUT extent, even and >= 2 per axis (odd: MIS_ERR_UNSUPPORTED); y is [N][Cout][D/2][H/2][W/2].  The
 * input has Cin = Cl + Cx channels: the first Cl are read as softmax over the Cl channels of `logits` [N][Cl][D][H][W]
 * (never written to memory; Cl <= 4, Cl = 0 and logits = NULL: none), the last Cx are read from x [N][Cx][D][H][W] as they
 * lie (Cx = 0 and x = NULL: none).  The filter is given in the same two parts, torch layout: w_l [Cout][Cl][4][4][4],
 * w_x [Cout][Cx][4][4][4] (FC3DDiscriminator's conv0 + conv1 in one pass, bias and bias2 their two biases; either bias may be
 * NULL).  slope = 1 is no activation; drop_scale [N][Cout] or NULL.  Any Cin, Cout >= 1.
 *
 * Few output voxels and a long contraction (the deep layers): the input channels are cut into slices, every slice leaves its
 * partial sums in `workspace` (>= mis_conv_k4s2_fwd_workspace_bytes, which may be 0) and a second launch adds them in slice
 * order and applies the epilogue.
 *
 * mis_conv_k4s2_dgrad: dx [N][Cin][D][H][W] = the gradient at the convolution's input (all Cin channels as plain channels,
 *   w [Cout][Cin][4][4][4]; the first layer passes conv0's filter and gets the gradient at the softmax output) for the
 *   gradient dy at the ACTIVATED output: dy is multiplied on the load path by the activation's derivative, recovered from
 *   the sign of the stored output y (slope > 0; y = NULL: no activation), and by drop_scale (NULL: none).
 * mis_conv_k4s2_wgrad: dw_l / dw_x (+)= the filter gradient in the two parts of the forward, dbias / dbias2 [Cout] (+)= the
 *   bias gradient (NULL: not wanted; both receive the same sum).  Partial sums over slices of the output voxels go to
 *   `workspace` (>= mis_conv_k4s2_wgrad_workspace_bytes) and are added in slice order.
 *
 * MIS_ERR_ARG: a NULL pointer the call needs, a count or extent <= 0, a batch stride below C * S, slope <= 0.
 * MIS_ERR_UNSUPPORTED: an odd extent, Cl > 4, N * (D/2) * (H/2) * (W/2) >= 2^31.  MIS_ERR_WORKSPACE: workspace too small. */
long long mis_conv_k4s2_fwd_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W);
int mis_conv_k4s2_fwd(const float* x, long long x_bs, int Cx, const float* logits, long long l_bs, int Cl, const float* w_x,
                      const float* w_l, const float* bias, const float* bias2, float* y, long long y_bs, int N, int Cout,
                      int D, int H, int W, float slope, const float* drop_scale, float* workspace,
                      long long workspace_bytes, mis_stream_t stream);
int mis_conv_k4s2_dgrad(const float* dy, long long dy_bs, const float* y, long long y_bs, float slope,
                        const float* drop_scale, const float* w, float* dx, long long dx_bs, int N, int Cin, int Cout,
                        int D, int H, int W, mis_stream_t stream);
long long mis_conv_k4s2_wgrad_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W);
int mis_conv_k4s2_wgrad(const float* x, long long x_bs, int Cx, const float* logits, long long l_bs, int Cl,
                        const float* dy, long long dy_bs, const float* y, long long y_bs, float slope,
                        const float* drop_scale, float* dw_x, float* dw_l, float* dbias, float* dbias2, int N, int Cout,
                        int D, int H, int W, int accumulate, float* workspace, long long workspace_bytes,
                        mis_stream_t stream);

/* The discriminator's head: a [N][C][D][H][W] (the activated conv4 output) -> AvgPool3d(pool) -> flatten ->
 * Linear(C, K) (w [K][C], b [K]) -> cross_entropy(logits, target), mean over the N samples; target [N] int32 in [0, K).
 * The pool window must equal the feature's extent (else MIS_ERR_UNSUPPORTED), K <= 8.
 * mis_adv_head_fwd writes loss[0], logits [N][K] and keeps the pooled features and d loss / d logits in `workspace`
 * (>= mis_adv_head_workspace_bytes); mis_adv_head_bwd reads that workspace and writes da [N][C][D][H][W] (the gradient at a;
 * NULL: not wanted), dw [K][C] and db [K] (+)= (NULL: not wanted). */
long long mis_adv_head_workspace_bytes(int N, int C, int K);
int mis_adv_head_fwd(const float* a, long long a_bs, const float* w, const float* b, const int* target, float* loss,
                     float* logits, int N, int C, int K, int D, int H, int W, int pool_d, int pool_h, int pool_w,
                     float* workspace, long long workspace_bytes, mis_stream_t stream);
int mis_adv_head_bwd(const float* w, float* da, long long da_bs, float* dw, float* db, int accumulate, int N, int C, int K,
                     int D, int H, int W, const float* workspace, long long workspace_bytes, mis_stream_t stream);

/* The segmenter's loss tail of the adversarial step (train_adversarial_network_3D.py:137-150):
 *   loss = 0.5 * (CE + Dice)(logits[:L], label) + w * cons_loss,   w = state->cons_weight (state == NULL: cons_weight),
 * cons_loss[0] = the discriminator's cross-entropy on the unlabeled samples (mis_adv_head_fwd's loss, on the device) and
 * dmap [B - L][C][S] its gradient at softmax(logits[L:]) (mis_conv_k4s2_dgrad of the first layer).
 * out (>= 5 + C floats): loss, loss_ce, loss_dice, cons_loss, w, class-wise dice.  dlogits [B][C][S] (NULL: forward only) =
 * loss_scale * (the supervised gradient on the labeled samples; w * (softmax Jacobian)^T dmap on the unlabeled ones), one
 * pass.  C in {2, 3, 4}, any S >= 1.  B == L: dmap and cons_loss may be NULL. */
long long mis_adversarial_tail_workspace_bytes(int B, int C, long long S);
int mis_adversarial_tail(const float* logits, long long s_bs, const void* label, int label_bytes, const float* dmap,
                         long long dm_bs, const float* cons_loss, int B, int L, int C, long long S, float cons_weight,
                         const MisStepState* state, float loss_scale, float* out, float* dlogits, long long d_bs,
                         void* workspace, long long workspace_bytes, mis_stream_t stream);

/* torch.optim.Adam (no weight decay, no amsgrad, bias-corrected) on flat fp32 buffers of n elements.  adam_state: 16 bytes
 * on the device (int64 step count, then 1 - beta1^step and 1 - beta2^step as floats): mis_adam_step first advances the count
 * and the corrections there, so a recorded launch replays as the next step.  mis_adam_init sets the count (0: fresh). */
int mis_adam_init(void* adam_state, long long step, mis_stream_t stream);
int mis_adam_step(float* param, const float* grad, float* m, float* v, long long n, float lr, float beta1, float beta2,
                  float eps, void* adam_state, mis_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
