/* C ABI of libmis_hip.so, dilated 3x3 convolutions (csrc/conv_dilated.hip): a header of its own beside mis_hip.h, with the
 * same conventions (device pointers, fp32, NCHW with free batch strides, the stream last, 0 or MIS_ERR_* returned,
 * deterministic results) and the types of mis_hip.h.  The definitions are compiled against these declarations, and
 * mis_hip/lib.py reads the ctypes prototypes from this text (lib.EXTRA_HEADERS), exactly as it does for mis_hip.h. */
#ifndef MIS_HIP_DILATED_H
#define MIS_HIP_DILATED_H

#include "mis_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nn.Conv2d(Cin, Cout, kernel_size=3, dilation=d, padding=d), stride 1, d in {2, 4, 8, 16} (PNet2D's blocks 2..5, reference
 * code/networks/pnet.py:26-29): forward, data gradient and weight gradient on v_mfma_f32_16x16x4_f32.  Every H, W >= 1 is
 * served (also H or W < d: the taps that fall wholly into the padding contribute exact zeros).  x, y, dy, dx are
 * [N][C][H][W] with dense (C, H, W) and a batch stride >= C * H * W floats: channel slices of wider buffers are fine.
 *
 * mis_conv_dilated_fwd:   y = bias + conv(x);  wp = mis_conv_pack_weights(w, ..., taps = 9, mode 0), bias [Cout] or NULL.
 * mis_conv_dilated_dgrad: dx = the gradient of that convolution at its input for the output gradient dy [N][Cout][H][W];
 *   wpd = the same weights packed with mode 1 (flipped taps, transposed channels).  It is the forward launch on (dy, wpd)
 *   with the channel counts exchanged and no bias.
 * mis_conv_dilated_wgrad: dw[Cout][Cin][9] (+)= sum over images and pixels of dy * shifted x.  Partial sums go to
 *   `workspace` (>= mis_conv_dilated_wgrad_workspace_bytes) and are added in a fixed order: run-to-run bit-identical.
 *   accumulate != 0 adds to dw instead of overwriting it.
 * *_kernel_name: the kernel instantiation that serves the geometry, as a profiler prints it (minus the anonymous
 *   namespace).
 *
 * MIS_ERR_ARG: a NULL pointer that the call needs, a size <= 0, a batch stride below C * H * W.  MIS_ERR_UNSUPPORTED, with
 * nothing launched: a dilation outside {2, 4, 8, 16} (dilation 1 is mis_conv_fwd / mis_conv_wgrad), a packed filter that is
 * not 16-byte aligned, or an image beyond the 32-bit buffer descriptors, (max(Cin, Cout) + 32) * H * W * 4 >= 2^30 bytes
 * (the limit mis_conv_fwd documents).  MIS_ERR_WORKSPACE: workspace too small. */
int mis_conv_dilated_fwd(const float* x, long long x_bs, const float* wp, const float* bias, float* y, long long y_bs, int N,
                         int Cin, int Cout, int H, int W, int dilation, mis_stream_t stream);
int mis_conv_dilated_dgrad(const float* dy, long long dy_bs, const float* wpd, float* dx, long long dx_bs, int N, int Cin,
                           int Cout, int H, int W, int dilation, mis_stream_t stream);
long long mis_conv_dilated_wgrad_workspace_bytes(int N, int Cin, int Cout, int H, int W, int dilation);
int mis_conv_dilated_wgrad(const float* x, long long x_bs, const float* dy, long long dy_bs, float* dw, float* workspace,
                           long long workspace_bytes, int N, int Cin, int Cout, int H, int W, int dilation, int accumulate,
                           mis_stream_t stream);
int mis_conv_dilated_fwd_kernel_name(int N, int Cin, int Cout, int H, int W, int dilation, char* name, int name_len);
int mis_conv_dilated_dgrad_kernel_name(int N, int Cin, int Cout, int H, int W, int dilation, char* name, int name_len);
int mis_conv_dilated_wgrad_kernel_name(int N, int Cin, int Cout, int H, int W, int dilation, char* name, int name_len);

#ifdef __cplusplus
}
#endif

#endif
