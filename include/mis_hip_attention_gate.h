/* C ABI of libmis_hip.so, grid attention gates of the 3-D Attention U-Net and trilinear up-sampling by an integer factor
 * (csrc/attention_gate.hip): a header of its own beside mis_hip.h, with the same conventions (device pointers, fp32, NCDHW with
 * dense (C, D, H, W) and free batch strides `*_bs` in floats, so any operand may be a channel slice of a wider buffer; the
 * stream last; 0 or MIS_ERR_* returned; deterministic results: no floating-point atomics, partial sums added in a fixed order).
 * The definitions are compiled against these declarations, and mis_hip/lib.py reads the ctypes prototypes from this text
 * (lib.EXTRA_HEADERS), exactly as it does for mis_hip.h.
 *
 * Reference: GridAttentionBlock3D._concatenation (code/networks/grid_attention_layer.py:84-107) as MultiAttentionBlock uses it
 * (code/networks/attention_unet.py:113-136): G gates stacked along channels read the same skip tensor x and the same gating
 * signal.  Ci = inter_channels; the coarse grid is d x h x w, the fine grid D x H x W = 2d x 2h x 2w.
 *
 *   att[n][g][u]     = sigmoid(psi_b[g] + sum_i psi_w[g][i] * relu(theta[n][g Ci + i][u] + phi[n][g Ci + i][u]))
 *   y[n][g C + c][v] = up2(att[n][g])(v) * x[n][c][v]
 *
 * up2 = trilinear x2, align_corners=False, neighbours clamped at the edges (a coarse extent of 1 replicates), on all three
 * axes -- also when d == 1, unlike mis_upsample2_fwd, whose D == 1 selects the 2-D form.
 *
 * mis_attn_gate_map_fwd:   theta, phi [N][G Ci][d][h][w]; psi_w [G][Ci], psi_b [G] contiguous; att [N][G][d][h][w].
 * mis_attn_gate_apply_fwd: x [N][C][D][H][W] is read once for all G gates; y [N][G C][D][H][W].
 * mis_attn_gate_apply_bwd: dx[n][c][v] (+)= sum_g up2(att_g)(v) dy[n][g C + c][v]  (accumulate != 0 adds: x has other readers);
 *   datt [N][G][d][h][w] = the adjoint of up2 applied to sum_c dy * x, always written.  dy and x are read once: the channel sums
 *   go to a fine-resolution [N][G][D][H][W] scratch in `workspace` (>= mis_attn_gate_apply_bwd_workspace_bytes), 1 / C of the
 *   traffic, which a second launch gathers to the coarse grid.
 * mis_attn_gate_map_bwd:   with dpre = datt * att * (1 - att):
 *     df[n][g Ci + i][u] = psi_w[g][i] * dpre[n][g][u] * [theta + phi > 0]      (the gradient at theta AND at phi), written;
 *     dpsi_w[g][i] (+)= sum_{n,u} relu(theta + phi) * dpre,   dpsi_b[g] (+)= sum_{n,u} dpre    (accumulate != 0 adds);
 *     dphi_b[g Ci + i] (+)= sum_{n,u} df, the bias gradient of the phi convolution (df is its output gradient), or NULL: the
 *     launch has every df value in a register, a separate channel sum would read df again.
 *   Per-workgroup partial sums go to `workspace` (>= mis_attn_gate_map_bwd_workspace_bytes) and a second launch adds them in a
 *   fixed order.
 * mis_upsample_int_fwd / _bwd: y [N][K][s d][s h][s w] = trilinear up-sampling of x [N][K][d][h][w] by scale s in {2, 4, 8} per
 *   axis, align_corners=False (source coordinate (dst + 0.5) / s - 0.5 clamped below at 0, neighbours clamped at the edge), and
 *   its exact adjoint in gather form: dx[u] (+)= the weighted sum of the (2s)^3 outputs that read u.
 *
 * MIS_ERR_ARG: a NULL pointer the call needs, N, G, C, Ci, K or an extent <= 0, a batch stride below the operand's C * D * H * W.
 * MIS_ERR_UNSUPPORTED, with nothing launched: (D, H, W) != (2d, 2h, 2w); a scale outside {2, 4, 8}; G > 4; a fine volume of
 * 2^31 voxels or more.  MIS_ERR_WORKSPACE: workspace too small.  The *_workspace_bytes queries return a negative MIS_ERR_* for a
 * geometry the launch would refuse. */
#ifndef MIS_HIP_ATTENTION_GATE_H
#define MIS_HIP_ATTENTION_GATE_H

#include "mis_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int mis_attn_gate_map_fwd(const float* theta, long long theta_bs, const float* phi, long long phi_bs, const float* psi_w,
                          const float* psi_b, float* att, long long att_bs, int N, int G, int Ci, int d, int h, int w,
                          mis_stream_t stream);
int mis_attn_gate_apply_fwd(const float* x, long long x_bs, const float* att, long long att_bs, float* y, long long y_bs, int N,
                            int G, int C, int D, int H, int W, int d, int h, int w, mis_stream_t stream);
long long mis_attn_gate_apply_bwd_workspace_bytes(int N, int G, int D, int H, int W);
int mis_attn_gate_apply_bwd(const float* dy, long long dy_bs, const float* x, long long x_bs, const float* att, long long att_bs,
                            float* dx, long long dx_bs, float* datt, long long datt_bs, void* workspace,
                            long long workspace_bytes, int N, int G, int C, int D, int H, int W, int d, int h, int w,
                            int accumulate, mis_stream_t stream);
long long mis_attn_gate_map_bwd_workspace_bytes(int N, int G, int Ci, int d, int h, int w);
int mis_attn_gate_map_bwd(const float* datt, long long datt_bs, const float* att, long long att_bs, const float* theta,
                          long long theta_bs, const float* phi, long long phi_bs, const float* psi_w, float* df, long long df_bs,
                          float* dpsi_w, float* dpsi_b, float* dphi_b, void* workspace, long long workspace_bytes, int N, int G,
                          int Ci, int d, int h, int w, int accumulate, mis_stream_t stream);
int mis_upsample_int_fwd(const float* x, long long x_bs, float* y, long long y_bs, int N, int K, int d, int h, int w, int scale,
                         mis_stream_t stream);
int mis_upsample_int_bwd(const float* dy, long long dy_bs, float* dx, long long dx_bs, int N, int K, int d, int h, int w,
                         int scale, int accumulate, mis_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
