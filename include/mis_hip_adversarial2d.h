/* C ABI of libmis_hip.so, adversarial training of the 2-D nets (csrc/adversarial2d.hip): the 2-D discriminator's kernel-4 /
 * stride-2 convolutions and its windowed pool + linear + cross-entropy head.  A header of its own beside mis_hip.h, with the
 * conventions of mis_hip_adversarial.h (device pointers, fp32, NCHW with free batch strides, the stream last, 0 or MIS_ERR_*
 * returned before anything is launched, run-to-run bit-identical results, no floating-point atomics) and the types of
 * mis_hip.h.  The definitions are compiled against these declarations, and mis_hip/lib.py reads the ctypes prototypes from
 * this text (lib.EXTRA_HEADERS).  The dropout decision, the segmenter's loss tail and Adam are dimension-free and stay where
 * they are: mis_channel_dropout_scale, mis_adversarial_tail, mis_adam_init, mis_adam_step (mis_hip_adversarial.h).
 *
 * Reference: code/networks/discriminator.py:58-100 (FCDiscriminator), code/train_adversarial_network_2D.py. */
#ifndef MIS_HIP_ADVERSARIAL2D_H
#define MIS_HIP_ADVERSARIAL2D_H

#include "mis_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nn.Conv2d(Cin, Cout, kernel_size = 4, stride = 2, padding = 1) on v_mfma_f32_16x16x4_f32, with the discriminator's
 * epilogue:   y = drop(leaky_relu(bias + bias2 + conv(in), slope)).
 *
 * (H, W) is the INPUT extent, even and >= 2 per axis (odd: MIS_ERR_UNSUPPORTED); y is [N][Cout][H/2][W/2].  The input has
 * Cin = Cl + Cx channels: the first Cl are read as softmax over the Cl channels of `logits` [N][Cl][H][W] (never written to
 * memory; Cl <= 4, Cl = 0 and logits = NULL: none), the last Cx are read from x [N][Cx][H][W] as they lie (Cx = 0 and
 * x = NULL: none).  The filter is given in the same two parts, torch layout: w_l [Cout][Cl][4][4], w_x [Cout][Cx][4][4]
 * (FCDiscriminator's conv0 + conv1 in one pass, bias and bias2 their two biases; either bias may be NULL).  slope = 1 is no
 * activation; drop_scale [N][Cout] or NULL.  Any Cin, Cout >= 1.
 *
 * Whole input row segments are staged in LDS with 16-byte loads where W, the batch strides and the pointers are multiples
 * of 4 floats (else element by element, same result); the next stage is loaded while the current one is multiplied.
 *
 * Few output pixels and a long contraction (the deep layers): the input channels are cut into slices, every slice leaves its
 * partial sums in `workspace` (>= mis_conv2d_k4s2_fwd_workspace_bytes, which may be 0) and a second launch adds them in slice
 * order and applies the epilogue.
 *
 * mis_conv2d_k4s2_dgrad: dx [N][Cin][H][W] = the gradient at the convolution's input (all Cin channels as plain channels,
 *   w [Cout][Cin][4][4]; the first layer passes conv0's filter and gets the gradient at the softmax output) for the gradient
 *   dy at the ACTIVATED output: dy is multiplied on the load path by the activation's derivative, recovered from the sign of
 *   the stored output y (slope > 0; y = NULL: no activation), and by drop_scale (NULL: none).  Cin <= 4 (the `map`
 *   gradient) runs a form of its own: pixels on the MFMA's rows, (channel, parity class) on its 16 columns.
 * mis_conv2d_k4s2_wgrad: dw_l / dw_x (+)= the filter gradient in the two parts of the forward, dbias / dbias2 [Cout] (+)= the
 *   bias gradient (NULL: not wanted; both receive the same sum).  Partial sums over slices of the output pixels go to
 *   `workspace` (>= mis_conv2d_k4s2_wgrad_workspace_bytes, never 0) and are added in slice order.
 *
 * MIS_ERR_ARG: a NULL pointer the call needs, a count or extent <= 0, a batch stride below C * S, slope <= 0.
 * MIS_ERR_UNSUPPORTED: an odd extent, Cl > 4, N * Cout * (H/2) * (W/2) >= 2^31, more than 65535 (sample, slice) pairs.
 * MIS_ERR_WORKSPACE: workspace too small. */
long long mis_conv2d_k4s2_fwd_workspace_bytes(int N, int Cin, int Cout, int H, int W);
int mis_conv2d_k4s2_fwd(const float* x, long long x_bs, int Cx, const float* logits, long long l_bs, int Cl,
                        const float* w_x, const float* w_l, const float* bias, const float* bias2, float* y, long long y_bs,
                        int N, int Cout, int H, int W, float slope, const float* drop_scale, float* workspace,
                        long long workspace_bytes, mis_stream_t stream);
int mis_conv2d_k4s2_dgrad(const float* dy, long long dy_bs, const float* y, long long y_bs, float slope,
                          const float* drop_scale, const float* w, float* dx, long long dx_bs, int N, int Cin, int Cout,
                          int H, int W, mis_stream_t stream);
long long mis_conv2d_k4s2_wgrad_workspace_bytes(int N, int Cin, int Cout, int H, int W);
int mis_conv2d_k4s2_wgrad(const float* x, long long x_bs, int Cx, const float* logits, long long l_bs, int Cl,
                          const float* dy, long long dy_bs, const float* y, long long y_bs, float slope,
                          const float* drop_scale, float* dw_x, float* dw_l, float* dbias, float* dbias2, int N, int Cout,
                          int H, int W, int accumulate, float* workspace, long long workspace_bytes, mis_stream_t stream);

/* The 2-D discriminator's head: a [N][C][H][W] (the activated conv4 output) -> AvgPool2d((pool_h, pool_w)) (stride = window,
 * floor mode: nwh = H / pool_h by nww = W / pool_w windows, the remainder rows and columns are not read) -> flatten, feature
 * index c * (nwh * nww) + wy * nww + wx -> Linear(C * nwh * nww, K) (w [K][C * nwh * nww], b [K] or NULL) ->
 * cross_entropy(logits, target), mean over the N samples; target [N] int32 in [0, K).  K <= 8, fixed summation order.
 * mis_adv_head2d_fwd writes loss[0], logits [N][K] and keeps the pooled features and d loss / d logits in `workspace`
 * (>= mis_adv_head2d_workspace_bytes); mis_adv_head2d_bwd reads that workspace and writes da [N][C][H][W] (the gradient at a,
 * ZERO in the remainder rows and columns; NULL: not wanted), dw and db (+)= (NULL: not wanted).
 * MIS_ERR_ARG also: a window <= 0.  MIS_ERR_UNSUPPORTED: K > 8, N > 65535, a window larger than the feature (no window). */
long long mis_adv_head2d_workspace_bytes(int N, int C, int K, int H, int W, int pool_h, int pool_w);
int mis_adv_head2d_fwd(const float* a, long long a_bs, const float* w, const float* b, const int* target, float* loss,
                       float* logits, int N, int C, int K, int H, int W, int pool_h, int pool_w, float* workspace,
                       long long workspace_bytes, mis_stream_t stream);
int mis_adv_head2d_bwd(const float* w, float* da, long long da_bs, float* dw, float* db, int accumulate, int N, int C, int K,
                       int H, int W, int pool_h, int pool_w, const float* workspace, long long workspace_bytes,
                       mis_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
