"""The convolution kernels (csrc/conv_fwd.hip, conv_wino.hip, conv_wino2d.hip, conv_wgrad.hip, conv_wgrad_cin1.hip,
conv_wino_wgrad.hip, conv_wino2d_wgrad.hip, conv_k2s2.hip, conv1x1_gemm.hip, with pack.hip in front of them) against the float64
oracle of tests/conv_oracle.py, in units of fp32 noise.  tests/test_kernels_gpu.py and tests/test_wino_gpu.py hold the geometry
(boxes, rings, ragged blocks, refusals) at 2e-4 of the tensor's largest value on zero-mean uniform inputs; this file holds the
PRECISION, per output channel, on what the networks feed: the output of a norm + ReLU (non-negative, half zeros) with channel
scales over three decades, gradients with channel scales over three decades, an input with a mean of four standard deviations,
and the uniform class for comparison.

Every output is pre-filled with NaN and must come back finite.  The primary class of a shape (relu_scaled x, scaled dy) runs on
channel slices of wider buffers (NaN around an input, a sentinel around an output, which must survive), the further classes on
dense tensors.  Every case asserts which kernel served each of its tensors (the *_kernel_name entry points, conv_wino_select,
mis_conv3d_wino_fwd_splits, ops.DISPATCH), so the matrix cannot drift onto another kernel.  Each weight gradient is also
accumulated onto a non-zero dw.

The rule, per tensor, in both measures of conv_oracle.measure (max: the worst channel's largest error over that channel's
largest reference value; rms: over the whole tensor), with no per-case K:

    err_hip <= max(K * e32, FLOOR[kind]),    K = 6

e32 = error of torch's fp32 CPU operators on the same bits against float64; for a tensor a Winograd kernel serves, the larger of
that and of conv_oracle.winograd32 (plain fp32 F(2, 3) per axis), which tests/test_conv_oracle_cpu.py holds to <= 3 x e32 on
every k = 3 case of the matrix (measured <= 2.8; one 4 x 4 case, which no Winograd kernel serves, is excepted there by name at 3.4): K = 6
is that margin twice.  FLOOR = the largest e32 of the matrix per kind (recomputed there).
The statistics of the split forward (wino_split_reduce_kernel + mis_norm_stats_finalize) are held to the ``stat`` rule of
tests/test_norm_edges_gpu.py with its conditioning factor for fp32 partials.

Measured on an MI355X (this file's own run; `MIS_CONV_STATS=<file>` writes every figure as JSON).  ratio = HIP / max(e32, FLOOR / K):
the error in units of fp32 noise, the gate is at 6.  72 cases (71 pass, one xfails on its one known entry), 10 s wall (the long weight gradient of 8 x 64 x 24^3: 2.6 s, of
which 2.2 s are the CPU references; every other case under 0.9 s).

    kernel (as the library names it; /n = contraction slices)            kind e32 (max measure)    HIP max   ratio  HIP rms   ratio  worst case (max measure)
    conv_fwd_kernel<Cfg<3, 3, 3, 2, 4, 16, 16, 4, 2>>                     y    2.7e-07 .. 1.0e-06  7.65e-07  1.11  1.70e-07  0.68  direct-ragged/relu_scaled
    conv_fwd_kernel<Cfg<3, 3, 3, 2, 4, 16, 16, 4, 2>>                     dx   2.0e-07 .. 2.6e-07  4.13e-07  1.66  1.74e-07  0.95  direct-ragged/offset
    conv_fwd_kernel<Cfg<3, 3, 3, 2, 8, 8, 16, 4, 2>>  (beside the split)  y    5.2e-07 .. 1.4e-06  7.66e-07  1.02  2.28e-07  0.74  split4-6/relu_scaled
    conv_fwd_kernel<Cfg<3, 3, 3, 4, 8, 16, 16, 4, 8>>                     dx   1.9e-07 .. 1.9e-07  9.09e-07  4.77  3.51e-07  1.92  direct-cin1/relu_scaled
    conv_fwd_kernel<Cfg<1, 1, 1, 4, 8, 16, 16, 16, 8>>                    y    2.0e-07 .. 2.0e-07  7.34e-08  0.29  2.42e-08  0.10  direct-cout2-k1/relu_scaled
    conv_fwd_kernel<Cfg<1, 1, 1, 4, 8, 16, 16, 16, 8>>                    dx   5.3e-08 .. 5.3e-08  5.29e-08  0.29  2.53e-08  0.14  direct-cout2-k1/relu_scaled
    conv_fwd_kernel<Cfg<1, 3, 3, 1, 16, 16, 32, 8, 4>>  (the 4 x 4 level) y    3.8e-07 .. 1.2e-06  2.26e-06  5.93  5.13e-07  2.05  direct2d-4x4-256/relu_scaled
    conv_fwd_kernel<Cfg<1, 3, 3, 1, 16, 16, 32, 8, 4>>  (over the gate)   dx   4.3e-07 .. 5.7e-07  2.84e-06  6.55  7.99e-07  3.93  direct2d-4x4-128/offset
    conv_fwd_kernel<Cfg<1, 1, 1, 1, 16, 16, 32, 16, 4>> + pixel shuffle   y    1.5e-07 .. 4.2e-07  4.18e-07  1.00  1.17e-07  0.47  up2d/uniform
    conv_fwd_kernel<Cfg<1, 1, 1, 1, 16, 16, 32, 16, 4>> + pixel shuffle   dx   3.4e-07 .. 4.6e-07  1.13e-06  3.02  3.84e-07  2.09  up2d-4x4/relu_scaled
    conv_fwd_cin1_kernel<3>                                               y    8.8e-08 .. 8.8e-08  8.78e-08  0.35  2.32e-08  0.09  direct-cin1/relu_scaled
    conv_fwd_cin1_kernel<1>                                               y    1.2e-07 .. 1.2e-07  1.18e-07  0.47  2.76e-08  0.11  direct2d-cin1/relu_scaled
    conv_small_cout_kernel                                                y    8.6e-08 .. 8.6e-08  5.91e-08  0.24  2.32e-08  0.09  direct2d-cout2/relu_scaled
    conv_small_cout_kernel                                                dx   2.1e-07 .. 3.5e-07  2.98e-07  0.85  1.90e-07  0.96  direct2d-cin1/relu_scaled
    wino_fwd_kernel<WinoCfg<1, 1, 16, 2, 2, 1, 1, 4, 0, 0>, false>        y    2.9e-07 .. 5.6e-07  2.87e-07  0.92  2.02e-07  0.81  wino-v0/relu
    wino_fwd_kernel<WinoCfg<1, 1, 16, 2, 2, 1, 1, 4, 0, 0>, false>        dx   2.5e-07 .. 3.4e-07  3.92e-07  1.14  2.25e-07  1.01  wino-v0/offset
    wino_fwd_kernel<WinoCfg<1, 2, 8, 2, 2, 1, 1, 4, 0, 0>, false>         y    7.1e-07 .. 7.1e-07  2.60e-07  0.37  9.77e-08  0.39  wino-v1/relu_scaled
    wino_fwd_kernel<WinoCfg<1, 2, 8, 2, 2, 1, 1, 4, 0, 0>, false>         dx   6.4e-07 .. 6.4e-07  4.43e-07  0.69  2.63e-07  0.80  wino-v1/relu_scaled
    wino_fwd_kernel<WinoCfg<1, 4, 4, 4, 1, 1, 1, 4, 1, 0>, false>         y    4.7e-07 .. 6.8e-07  4.03e-07  0.80  1.59e-07  0.63  wino-v2/relu_scaled
    wino_fwd_kernel<WinoCfg<1, 4, 4, 4, 1, 1, 1, 4, 1, 0>, false>         dx   5.1e-07 .. 5.1e-07  4.37e-07  0.86  2.66e-07  1.00  wino-v2/relu_scaled
    wino_fwd_kernel<WinoCfg<1, 4, 4, 4, 1, 1, 1, 4, 1, 0>, false> /2      y    7.5e-07 .. 7.5e-07  6.23e-07  0.83  3.03e-07  0.74  split2-6/relu_scaled
    wino_fwd_kernel<WinoCfg<1, 4, 4, 4, 1, 1, 1, 4, 1, 0>, false> /2      dx   7.9e-07 .. 7.9e-07  4.18e-07  0.53  2.94e-07  0.74  wino-v2-partial-boxes/relu_scaled
    wino_fwd_kernel<WinoCfg<1, 4, 4, 4, 1, 1, 1, 4, 1, 0>, false> /4      y    7.0e-07 .. 1.4e-06  8.89e-07  0.85  3.62e-07  0.76  split4-6/relu_scaled
    wino_fwd_kernel<WinoCfg<1, 4, 4, 4, 1, 1, 1, 4, 1, 0>, false> /4      dx   6.8e-07 .. 9.0e-07  6.01e-07  0.89  3.99e-07  0.81  split2-6/relu_scaled
    wino_fwd_kernel<WinoCfg<3, 3, 6, 1, 1, 1, 1, 4, 1, 1>, false>         y    7.4e-07 .. 7.4e-07  2.89e-07  0.39  1.11e-07  0.44  wino-v3/relu_scaled
    wino_fwd_kernel<WinoCfg<3, 3, 6, 1, 1, 1, 1, 4, 1, 1>, false> /2      y    8.0e-07 .. 8.0e-07  5.35e-07  0.67  3.00e-07  0.75  split2-12/relu_scaled
    wino_fwd_kernel<WinoCfg<3, 3, 6, 1, 1, 1, 1, 4, 1, 1>, false> /2      dx   9.0e-07 .. 9.0e-07  5.33e-07  0.59  3.60e-07  0.72  split2-12/relu_scaled
    wino_fwd_kernel<WinoCfg<3, 3, 6, 1, 1, 1, 1, 4, 1, 1>, false> /4      dx   6.5e-07 .. 6.5e-07  3.44e-07  0.53  2.63e-07  0.60  wino-v3/relu_scaled
    wino2d_fwd_kernel<W2Cfg<8, 8, 1, 3>>                                  y    5.3e-07 .. 5.3e-07  5.21e-07  0.98  4.01e-08  0.16  wino2d-v0/relu_scaled
    wino2d_fwd_kernel<W2Cfg<8, 8, 1, 3>>                                  dx   3.5e-07 .. 8.1e-07  3.33e-07  0.84  2.04e-07  0.98  wino2d-v1/uniform
    wino2d_fwd_kernel<W2Cfg<8, 8, 2, 3>>                                  y    3.7e-07 .. 6.9e-07  3.65e-07  0.77  1.30e-07  0.52  wino2d-v1/relu
    wino2d_fwd_kernel<W2Cfg<4, 16, 1, 3>>                                 y    4.1e-07 .. 4.1e-07  2.92e-07  0.72  5.94e-08  0.24  wino2d-v2/relu_scaled
    wino2d_fwd_kernel<W2Cfg<4, 16, 1, 3>>                                 dx   4.6e-07 .. 4.9e-07  3.22e-07  0.69  1.92e-07  0.89  wino2d-v3/relu_scaled
    wino2d_fwd_kernel<W2Cfg<4, 16, 2, 3>>                                 y    4.4e-07 .. 4.4e-07  3.25e-07  0.74  5.03e-08  0.20  wino2d-v3/relu_scaled
    conv_wgrad_kernel<WCfg<3, 3, 3, 2, 12, 8, 1> >                        dw   2.3e-07 .. 2.3e-06  3.41e-07  0.14  1.90e-07  0.08  direct-ragged/offset
    conv_wgrad_kernel<WCfg<3, 3, 3, 2, 6, 8, 1> >  (the 6^3 level)        dw   8.0e-07 .. 2.0e-06  8.98e-07  0.36  1.71e-07  0.07  split4-6/offset
    conv_wgrad_kernel<WCfg<3, 3, 3, 4, 8, 8, 1> >                         dw   2.5e-06 .. 3.2e-06  3.13e-07  0.10  1.66e-07  0.07  wino-v2-partial-boxes/relu_scaled
    conv_wgrad_kernel<WCfg<1, 3, 3, 1, 16, 16, 1> >                       dw   2.2e-07 .. 1.2e-06  2.39e-07  0.10  1.34e-07  0.05  direct2d-4x4-128/offset
    conv_wgrad_kernel<WCfg<1, 3, 3, 1, 8, 32, 1> >                        dw   7.8e-07 .. 8.2e-07  1.47e-07  0.06  1.31e-07  0.05  direct2d-cout2/relu_scaled
    conv_wgrad_kernel<WCfg<1, 1, 1, 2, 8, 16, 1> >                        dw   6.6e-07 .. 6.8e-07  2.71e-07  0.11  1.77e-07  0.07  direct-cout2-k1/relu_scaled
    conv_wgrad_kernel<WCfg<1, 1, 1, 1, 16, 16, 1> > + pixel shuffle       dw   2.1e-07 .. 8.2e-07  2.60e-07  0.10  1.15e-07  0.05  up2d/offset
    wgrad_cin1_kernel<3, false>                                           dw   2.4e-07 .. 4.8e-07  3.17e-07  0.13  2.08e-07  0.08  direct-cin1/relu_scaled
    wgrad_cin1_kernel<1, false>                                           dw   6.0e-07 .. 1.1e-06  3.48e-07  0.14  2.12e-07  0.08  direct2d-cin1/relu_scaled
    wino_wgrad_kernel<WgCfg<2, 2, 8, 1> >             (select = 1)        dw   3.6e-07 .. 5.5e-07  4.41e-07  0.18  1.90e-07  0.08  wgrad-wino-v1/relu_scaled
    wino_wgrad_kernel<WgCfg<4, 2, 4, 0> >             (2)                 dw   5.1e-07 .. 6.1e-07  3.10e-07  0.12  1.48e-07  0.06  wino-v2/relu_scaled
    wino_wgrad_ring_kernel<WrCfg<2, 16, 1> >          (3; 24 x 24 x 96)   dw   4.0e-07 .. 8.4e-06  4.74e-07  0.19  2.48e-07  0.09  wino-v0/offset
    wino_wgrad_ring_kernel<WrCfg<4, 8, 1> >           (4)                 dw   4.7e-07 .. 9.0e-07  4.04e-07  0.16  2.39e-07  0.10  wino-v1/relu_scaled
    wino_wgrad_flat_kernel<12, 12>                    (5)                 dw   8.5e-07 .. 3.3e-06  6.97e-07  0.28  3.09e-07  0.12  wgrad-wino-v5/relu_scaled
    wino_wgrad_ring3_kernel<Wr3Cfg<4, 12> >           (6; 8 x 64 x 24^3)  dw   7.2e-07 .. 1.4e-05  1.11e-06  0.13  5.31e-07  0.13  wgrad-wino-v6/relu_scaled
    wino2d_wgrad_kernel<Wg2Cfg<1, 4, 8> >                                 dw   4.7e-07 .. 1.6e-06  3.07e-07  0.12  1.30e-07  0.05  wgrad-wino2d/relu_scaled
    wino2d_wgrad_kernel<Wg2Cfg<2, 4, 8> >                                 dw   6.9e-07 .. 1.5e-06  4.40e-07  0.18  1.45e-07  0.06  wino2d-v1/relu_scaled
    wino2d_wgrad_kernel<Wg2Cfg<1, 2, 16> >                                dw   1.4e-06 .. 1.4e-06  3.13e-07  0.13  1.80e-07  0.07  wino2d-v2/relu_scaled
    wino2d_wgrad_kernel<Wg2Cfg<2, 2, 16> >                                dw   4.4e-06 .. 4.4e-06  2.72e-07  0.06  1.67e-07  0.07  wino2d-v3/relu_scaled
    k2s2_down_kernel<16, 32>  (Conv3d forward, ConvTranspose3d dx)        y    3.6e-07 .. 8.0e-07  7.72e-07  1.30  2.18e-07  0.87  k2s2-down/uniform
    k2s2_down_kernel<16, 32>                                              dx   4.8e-07 .. 4.8e-07  4.57e-07  0.95  1.72e-07  0.87  k2s2-up/relu_scaled
    k2s2_down_kernel<32, 64>                                              y    3.5e-07 .. 3.5e-07  7.91e-07  2.29  1.24e-07  0.49  k2s2-down-32x64/relu_scaled
    k2s2_down_kernel<32, 64>                                              dx   6.2e-07 .. 6.2e-07  7.67e-07  1.24  2.88e-07  1.26  k2s2-up-64x32/relu_scaled
    k2s2_up_kernel<32, 16>  (ConvTranspose3d forward, Conv3d dx)          y    2.4e-07 .. 2.4e-07  2.45e-07  0.98  2.86e-08  0.11  k2s2-up/relu_scaled
    k2s2_up_kernel<32, 16>                                                dx   1.8e-07 .. 3.3e-07  3.33e-07  1.00  1.18e-07  0.64  k2s2-down/uniform
    k2s2_up_kernel<64, 32>                                                y    2.5e-07 .. 2.5e-07  2.45e-07  0.98  3.24e-08  0.13  k2s2-up-64x32/relu_scaled
    k2s2_up_kernel<64, 32>                                                dx   4.4e-07 .. 4.4e-07  4.36e-07  1.00  1.49e-07  0.81  k2s2-down-32x64/relu_scaled
    k2s2_wgrad_kernel<16, 32, 1, 4>  (16 x 1-voxel lane groups)           dw   8.5e-07 .. 3.5e-06  5.53e-07  0.16  1.61e-07  0.06  k2s2-down/offset
    k2s2_wgrad_kernel<32, 64, 3, 2>  (8 x 2)                              dw   3.1e-07 .. 5.0e-07  3.56e-07  0.14  1.31e-07  0.05  k2s2-up-64x32/relu_scaled
    conv1x1_gemm                                                          y    3.1e-07 .. 8.8e-07  8.78e-07  1.00  1.56e-07  0.62  gemm1x1-ragged/uniform
    conv1x1_gemm                                                          dx   4.5e-07 .. 5.8e-07  5.83e-07  1.00  2.16e-07  1.00  gemm1x1-ragged/uniform
    conv1x1_wgrad                                                         dw   2.5e-07 .. 1.8e-06  1.84e-06  0.74  2.38e-07  0.10  gemm1x1-ragged/offset
    wino_split_reduce_kernel + norm_stats_finalize                        mean 6.6e-09 .. 1.9e-07  2.34e-07  0.89 of its tolerance (split4-6/offset, per sample)
    wino_split_reduce_kernel + norm_stats_finalize                        rstd 1.1e-08 .. 2.2e-07  7.64e-07  0.60 of its tolerance (split2-12/relu_scaled, per sample; factor 5.3)

    Every kernel is within 2.3 x fp32 noise except the direct kernel where it still accumulates in one fmaf chain: the 16-channel
    4 x 8 x 16-tile configuration on the data gradient of the first layer (4.8 x over 16 x 27 products), the 1x1 convolution
    under the 2-D transposed convolution (3.0 x over 512 channels) and the 2-D 3x3 configuration at the 4 x 4 level (3.3 .. 6.6 x
    over 128 .. 256 channels x 9 taps), which holds the one tensor over the gate (OVER_THE_GATE below: open, not settled).
    The weight gradients sit far below their gate because FLOOR[dw] is torch's own fp32 sum over 8 x 24^3 voxels (1.4e-5); in
    absolute terms every HIP weight gradient is at 1.5e-7 .. 1.8e-6, the long contractions at 4.7e-7 and 1.1e-6 where torch's fp32
    is at 8.4e-6 and 1.4e-5.

The split forward beside the direct kernel and the algorithm (y, same operands, same process; max / rms):

    case (N x Cin -> Cout at size, slices)     e32 (torch fp32)      winograd32            HIP split             HIP direct (before -> after folding)
    split2-6/relu_scaled  8 x 128->256 6^3 /2  6.8e-07 / 2.1e-07     7.5e-07 / 4.1e-07     6.2e-07 / 3.0e-07     2.5e-06 / 6.1e-07 -> 4.7e-07 / 1.4e-07
    split4-6/uniform      4 x 256->256 6^3 /4  7.2e-07 / 3.3e-07     8.0e-07 / 4.9e-07     5.9e-07 / 3.6e-07     4.0e-06 / 1.3e-06 -> 4.3e-07 / 2.2e-07
    split4-6/relu                              5.2e-07 / 2.4e-07     7.0e-07 / 4.3e-07     5.9e-07 / 3.2e-07     4.0e-06 / 9.1e-07 -> 4.8e-07 / 1.9e-07
    split4-6/relu_scaled                       5.4e-07 / 2.3e-07     7.2e-07 / 4.3e-07     6.1e-07 / 3.3e-07     3.6e-06 / 8.5e-07 -> 5.5e-07 / 1.8e-07
    split4-6/offset                            1.4e-06 / 3.5e-07     1.2e-06 / 3.2e-07     8.9e-07 / 2.5e-07     5.7e-06 / 1.3e-06 -> 7.7e-07 / 2.3e-07
    split2-12/relu_scaled 4 x 128->128 12^3 /2 5.8e-07 / 2.3e-07     8.0e-07 / 4.0e-07     5.4e-07 / 3.0e-07     2.5e-06 / 7.0e-07 -> 4.0e-07 / 1.6e-07

    The split-contraction Winograd forward is at 0.6 .. 1.1 x (max) / 0.7 .. 1.4 x (rms) torch's fp32 and below the plain fp32
    algorithm in every case: it does not round
    "10 x coarser than the direct form".  What this file found instead is the DIRECT kernel: conv_fwd_kernel accumulated all
    Cin * taps products of an output in one MFMA fmaf chain, and at the deep levels (256 channels x 27 taps) that chain was at
    4 .. 7.7 x fp32 noise -- over the gate on split4-6/relu (7.7) and relu_scaled (6.7) beside the split, on the data gradient of
    direct-ragged/uniform (6.8) and of direct2d-4x4-128/offset (6.6).  The small-tile 3x3x3 configurations (NT <= 4: the deep
    levels) now restart the accumulators with every chunk of CI_B channels and fold them into a second set (conv_fwd.hip, FOLD);
    their figures above are after that change, 1.0 .. 1.7 x.  The 2-D configurations were measured folded too (the 4 x 4 level at
    1.0 .. 1.8 x) and keep the single chain for the reason given at OVER_THE_GATE.
"""
import functools

import pytest
import torch

import conv_oracle as co
import norm_oracle as no
import oracle_kit as kit
from oracle_kit import NAN, kernel_name as _name

pytestmark = pytest.mark.gpu

K = 6.0
FLOOR = {"y": 1.5e-6,       # largest e32 of the matrix: 1.44e-6 (split4-6/offset, max: 256 x 27 products of a mean-4 input)
         "dx": 1.1e-6,      # 1.08e-6 (gemm1x1-wide, max: a contraction over 1024 channels)
         "dw": 1.5e-5}      # 1.40e-5 (wgrad-long-v6, max: torch's fp32 sum over 8 x 24^3 voxels; the short cases sit at 3e-7 .. 8e-7)
# The one tensor left over the gate: the data gradient of 128 -> 256 at 4 x 4 by conv_fwd_kernel<Cfg<1, 3, 3, 1, 16, 16, 32, 8, 4>>,
# worst channel at 6.55 x e32 (2.84e-6 against 4.35e-7; rms 3.9 x).  Cause: one fmaf chain over 256 x 9 products.  Folding
# per-chunk accumulators as the 3x3x3 small-tile configurations do brings the whole 4 x 4 level to 1.0 .. 1.8 x (measured), but it
# also moves the one ill-conditioned tensor of unet2d_deconv_64_masks (test_parity_gpu.py::F64_K_CASE) from 7.2 to 7.9 x its
# reference's noise, 1.008 of that test's K = 8 tolerance.  OPEN, not settled: the 2-D configurations keep the coarser single chain
# only until that tensor's distance is explained; direct2d-4x4-256 y sits at 5.93 for the same reason.
# Strict and narrow (oracle_kit.Gate.done): the case xfails only when exactly these (tensor, measure) entries are over the gate -- every
# other tensor, the kernel names, the finite and sentinel checks of the case still fail it, and so does this entry passing.
OVER_THE_GATE = {"direct2d-4x4-128/offset": {("dx", "max")}}
LEAD, TRAIL = 1, 2            # channels of the wider buffer before / after a slice
_in, _out = functools.partial(kit.place, lead=LEAD, trail=TRAIL), functools.partial(kit.Out, lead=LEAD, trail=TRAIL)
STATS = []        # (group, case, label, kind, measure, e32, hip, kernel)
STAT_ROWS = []    # (case, "in" / "bn", "mean" / "rstd", e32, hip, hip / tolerance, largest conditioning factor)
TRIPLE = []       # (case, measure, e32 direct form, winograd32, HIP split, HIP direct)


def _ops():
    from mis_hip import ops
    return ops


def _lib():
    from mis_hip import lib
    return lib.load()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if not STATS:
        return
    for (kernel, kind, m), r in kit.worst_rows(((kernel, kind, m), f"{cid} {label}", e32, ehip, max(e32, FLOOR[kind] / K))
                                               for group, cid, label, kind, m, e32, ehip, kernel in STATS):
        print(f"\n[conv edges] {kernel:62s} {kind:2s} {m:3s} e32 {r['lo']:.1e} .. {r['hi']:.1e}  hip max {r['hip']:.2e}  "
              f"worst hip/max(e32, floor/K) {r['ratio']:.2f} ({r['at']})", end="")
    for key in ("mean", "rstd"):
        sel = [r for r in STAT_ROWS if r[2] == key]
        if sel:
            w = max(sel, key=lambda r: r[5])
            print(f"\n[conv edges] wino_split_reduce_kernel + norm_stats_finalize {key:4s} e32 {min(r[3] for r in sel):.1e} .. "
                  f"{max(r[3] for r in sel):.1e}  hip max {max(r[4] for r in sel):.2e}  worst hip/tolerance {w[5]:.2f} ({w[0]} {w[1]}, "
                  f"factor {w[6]:.1f})", end="")
    for cid, m, e32, ew, split, direct in TRIPLE:
        print(f"\n[conv edges] triple {cid:24s} {m:3s} e32 {e32:.2e}  winograd32 {ew:.2e}  HIP split {split:.2e}  HIP direct {direct:.2e}",
              end="")
    print()
    kit.report(STATS, "MIS_CONV_STATS", {"stats": STATS, "split_statistics": STAT_ROWS, "triple": TRIPLE})


# ---------------------------------------------------------------------------------------------------------------------
# which kernel serves a case (host-side queries of the library: nothing is launched)
# ---------------------------------------------------------------------------------------------------------------------
def _served_fwd(N, Cin, Cout, D, H, W, k):
    """(wino variant or -1, kernel name, contraction slices) of the forward launch for this geometry."""
    ops, L = _ops(), _lib()
    v = ops.conv_wino_select(N, Cin, Cout, D, H, W, k)
    if v >= ops.WINO2D:
        return v, _name(L.mis_conv2d_wino_kernel_name, v - ops.WINO2D), 1
    if v >= 0:
        return v, _name(L.mis_conv3d_wino_kernel_name, v), int(L.mis_conv3d_wino_fwd_splits(N, Cin, Cout, D, H, W, v))
    return v, _name(L.mis_conv_fwd_kernel_name, N, Cin, Cout, D, H, W, *k), 1


def _served_wgrad(N, Cin, Cout, D, H, W, k):
    L = _lib()
    if tuple(k) == co.K3:
        v = int(L.mis_conv3d_wino_wgrad_select(N, Cin, Cout, D, H, W))
        if v >= 0:
            return _name(L.mis_conv3d_wino_wgrad_kernel_name, v)
    if tuple(k) == co.K2D and D == 1:
        v = int(L.mis_conv2d_wino_wgrad_select(N, Cin, Cout, H, W))
        if v >= 0:
            return _name(L.mis_conv2d_wino_wgrad_kernel_name, v)
    return _name(L.mis_conv_wgrad_kernel_name, N, Cin, Cout, D, H, W, *k)


def served(spec):
    """{fwd: (name, slices), dgrad: (name, slices), wgrad: name} as the library reports them for a 'conv' case."""
    N, Cin, Cout, D, H, W = spec["shape"]
    k = spec["k"]
    f, d = _served_fwd(N, Cin, Cout, D, H, W, k), _served_fwd(N, Cout, Cin, D, H, W, k)
    return {"fwd": f[1:], "dgrad": d[1:], "wgrad": _served_wgrad(N, Cin, Cout, D, H, W, k)}


# ---------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------
class _Check:
    def __init__(self, name):
        self.name = name
        self.c = co.case(name)
        self.group = self.c["group"]
        self.r64, self.e32, self.ew = co.references(name)
        self.gate = kit.Gate(K, FLOOR, OVER_THE_GATE, STATS)

    def __call__(self, kind, got, kernel, label="", ref=None, e32=None, judged=co.MEASURES):
        return self.gate.tensor(self.name, label or kind, kind, got, self.r64[kind] if ref is None else ref,
                                lambda g, r: co.measure(g, r, co.dim_of(self.c, kind)),
                                {ms: co.yardstick(self.name, kind, ms) if e32 is None else e32[ms] for ms in judged},
                                (self.group, self.name), (kernel,))

    def done(self):
        self.gate.done(self.name)


def _layout(c):
    """The primary class of a shape runs on channel slices of wider buffers, the further classes on dense tensors."""
    return "slice" if c["xcls"] == "relu_scaled" else "dense"


def _dw_accumulate(chk, kernel, launch, shape):
    """``launch(dw, accumulate)`` onto a non-zero dw: the sum is held to the same rule (e32: fp32 torch's dw added in fp32)."""
    c = chk.c
    r64 = chk.r64["dw"]
    d0 = r64.flip(1 - co.dw_dim(c)).float()              # the output channels keep their own scale
    dw = d0.clone().reshape(shape).cuda()
    launch(dw, True)
    r32 = co.reference32(c)["dw"]
    e32 = co.measure((d0 + r32.float()).double(), r64 + d0.double(), co.dw_dim(c))
    if co.served_by_winograd(c, "dw"):
        e32 = {m: max(e32[m], chk.ew["dw"][m]) for m in co.MEASURES}
    chk("dw", dw, kernel, "dw+=", ref=r64 + d0.double(), e32=e32)


def _run_conv(name):
    """y, dx, dw of one 'conv' case of the matrix, each by the kernel the matrix names."""
    ops = _ops()
    chk = _Check(name)
    c = chk.c
    N, Cin, Cout, D, H, W = c["shape"]
    k = c["k"]
    lay = _layout(c)
    got = served(c)
    for key in ("fwd", "dgrad", "wgrad"):
        if key in c:
            assert got[key] == c[key], (name, key, got[key], c[key])
    xv, dyv = _in(c["x"], lay), _in(c["dy"], lay)
    wd, bd = c["w"].cuda(), c["b"].cuda()
    out = {}
    keep, ops.DISPATCH = ops.DISPATCH, set()
    try:
        if "y" in c["kinds"]:
            v = ops.conv_wino_select(N, Cin, Cout, D, H, W, k)
            y = _out((N, Cout, D, H, W), lay)
            ops.conv_fwd(xv, ops.conv_pack(wd, ops.conv_wino_pack_mode(v, False) if v >= 0 else 0), bd, y.v, Cin, Cout, k, wino=v)
            assert (f"wino_fwd_split:v{v}@{W}" in ops.DISPATCH) == (got["fwd"][1] > 1)
            chk("y", y.v, got["fwd"][0] + (f" /{got['fwd'][1]}" if got["fwd"][1] > 1 else ""))
            assert y.untouched()
            out.update(v=v, y=y)
        if "dx" in c["kinds"]:
            vb = ops.conv_wino_select(N, Cout, Cin, D, H, W, k)
            dx = _out((N, Cin, D, H, W), lay)
            ops.conv_fwd(dyv, ops.conv_pack(wd, ops.conv_wino_pack_mode(vb, True) if vb >= 0 else 1), None, dx.v, Cout, Cin, k,
                         wino=vb)
            chk("dx", dx.v, got["dgrad"][0] + (f" /{got['dgrad'][1]}" if got["dgrad"][1] > 1 else ""))
            assert dx.untouched()
        if "dw" in c["kinds"]:
            dw = torch.full(tuple(c["w"].shape), NAN, device="cuda")
            ops.conv_wgrad(xv, dyv, dw, k)
            chk("dw", dw, got["wgrad"])
            tags = set(ops.DISPATCH)
            _dw_accumulate(chk, got["wgrad"], lambda t, acc: ops.conv_wgrad(xv, dyv, t, k, accumulate=acc), tuple(c["w"].shape))
            assert any(t.startswith("wino_wgrad:") for t in tags) == got["wgrad"].startswith("wino_wgrad")
    finally:
        ops.DISPATCH = keep
    return chk, xv, wd, bd, out


@pytest.mark.parametrize("name", co.names("fwd3d"))
def test_forward_and_data_gradient_3d(name):
    """The direct kernels (generic ragged, cin1<3>, k = 1 with Cout = 2) and the four Winograd variants (whole and partly
    filled boxes); the data gradient is the same launch on dy with pack mode 1 / 5; dw of the same operands rides along."""
    _run_conv(name)[0].done()


@pytest.mark.parametrize("name", co.names("fwd2d"))
def test_forward_and_data_gradient_2d(name):
    """The four conv_wino2d variants, cin1<1>, the 4x4x1-MFMA kernel for Cout <= 4, and the 4 x 4 level of the 2-D UNet."""
    _run_conv(name)[0].done()


@pytest.mark.parametrize("name", co.names("wgrad"))
def test_weight_gradient(name):
    """The direct weight gradient, every value of mis_conv3d_wino_wgrad_select at its smallest shape, conv_wino2d_wgrad, and
    one long contraction per 3-D ring kernel; each also accumulating onto a non-zero dw."""
    _run_conv(name)[0].done()


@pytest.mark.parametrize("name", co.names("split"))
def test_split_contraction(name):
    """The split-contraction Winograd forward (2 and 4 slices at 6^3, 2 at 12^3) with bias, against the oracle; then with the
    fused statistics out of wino_split_reduce_kernel + mis_norm_stats_finalize (the ``stat`` rule of test_norm_edges_gpu.py
    with its factor for fp32 partials); then the direct kernel on the same operands in the same process: HIP split, HIP direct
    and winograd32 side by side."""
    ops = _ops()
    chk, xv, wd, bd, out = _run_conv(name)
    c, r64 = chk.c, chk.r64
    N, Cin, Cout, D, H, W = c["shape"]
    k, v = c["k"], out["v"]
    kernel = c["fwd"][0] + f" /{c['fwd'][1]}"
    assert c["fwd"][1] > 1
    wp = ops.conv_pack(wd, 4)
    T = ops.conv_stat_tiles(N, Cin, Cout, D, H, W, k, wino=v)
    assert T > 0
    y32 = co.reference32(c)["y"].float()
    for per_sample in (True, False):
        kind = "in" if per_sample else "bn"
        G = N * Cout if per_sample else Cout
        part = torch.full((Cout * N * T, 2), NAN, device="cuda")
        y = _out((N, Cout, D, H, W), _layout(c))
        ops.conv_fwd(xv, wp, bd, y.v, Cin, Cout, k, stat=(part, *((T, Cout * T) if per_sample else (N * T, T))), wino=v)
        chk("y", y.v, kernel, "y+stat")
        assert y.untouched() and torch.isfinite(part).all()
        mean, rstd = torch.full((G,), NAN, device="cuda"), torch.full((G,), NAN, device="cuda")
        ops.norm_stats_finalize(part, N, Cout, D * H * W, T, per_sample, 1e-5, mean, rstd)
        m64, var64, rstd64 = (no.flat(t, kind) for t in no.stats64(r64["y"], kind))
        m32, _, rstd32 = (no.flat(t, kind) for t in no.stats64(y32, kind))      # statistics of fp32 torch's y
        factor = no.finalize_factor(m64, var64)
        for key, g, ref, r32, each in (("mean", mean, m64, m32, False), ("rstd", rstd, rstd64, rstd32, True)):
            e32 = no.rel(r32, ref, each)
            tol = max(no.K * e32, no.FLOOR_STAT)
            err = (g.cpu().double() - ref).abs()
            scale = ref.abs() if each else ref.abs().max()
            lim = tol * scale * (factor if each else 1.0)
            worst = (err / lim).max().item()
            print(f"[split {name}] {kind} {key:5s} e32 {e32:.2e} hip/tolerance {worst:.2f} factor max {factor.max().item():.1f}")
            STAT_ROWS.append((name, kind, key, e32, (err / scale).max().item(), worst, factor.max().item()))
            if not worst <= 1.0:
                chk.gate.bad.append((kind, key, f"e32 {e32:.3e}", f"hip/tolerance {worst:.3f}"))
    yd = _out((N, Cout, D, H, W), "dense")
    ops.conv_fwd(xv, ops.conv_pack(wd, 0), bd, yd.v, Cin, Cout, k)
    md = chk("y", yd.v, _served_direct(c), "y direct", e32=chk.e32["y"])
    ms = chk("y", out["y"].v, "", judged=())        # the figures alone, judged above
    for m in co.MEASURES:
        TRIPLE.append((name, m, chk.e32["y"][m], chk.ew["y"][m], ms[m], md[m]))
    chk.done()


def _served_direct(c):
    N, Cin, Cout, D, H, W = c["shape"]
    return _name(_lib().mis_conv_fwd_kernel_name, N, Cin, Cout, D, H, W, *c["k"])


# ---------------------------------------------------------------------------------------------------------------------
# kernel 2 / stride 2, 1x1 GEMM, 2-D transposed convolution
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", co.names("k2s2"))
def test_kernel2_stride2(name):
    """conv_k2s2.hip in place: Conv3d(k2s2) (down: y, up: dx) and ConvTranspose3d(k2s2) (up: y, down: dx) with the shared
    weight-gradient kernel: both channel pairs ((16, 32) and (32, 64): every template of the three kernels), whole and ragged
    16-voxel tiles, the weight gradient on 16 x 1 (Wo % 16 == 0) and on 8 x 2-voxel lane groups."""
    ops = _ops()
    chk = _Check(name)
    c = chk.c
    N, Cin, Cout, D, H, W = c["shape"]
    lay = _layout(c)
    down = c["op"] == "down"
    coarse = (D // 2, H // 2, W // 2) if down else (D, H, W)
    cf, cc = (Cin, Cout) if down else (Cout, Cin)          # channels on the fine / coarse side
    assert ops.conv_k2s2_eligible(cf, cc, coarse, False) and ops.conv_k2s2_eligible(cc, cf, coarse, True)
    assert ops.conv_k2s2_wgrad_eligible(cf, cc, coarse)
    xv, dyv = _in(c["x"], lay), _in(c["dy"], lay)
    w2, bd = c["w"].cuda().reshape(cc, cf * 8), c["b"].cuda()
    y, dx = _out(co.out_shape(c), lay), _out(tuple(c["x"].shape), lay)
    fwd, bwd = (ops.conv_k2s2_down, ops.conv_k2s2_up) if down else (ops.conv_k2s2_up, ops.conv_k2s2_down)
    keep, ops.DISPATCH = ops.DISPATCH, set()
    try:
        fwd(xv, w2, bd, y.v)
        bwd(dyv, w2, None, dx.v)
        assert ops.conv_k2s2_up_output_ok(y.v if not down else dx.v)
        assert ops.conv_k2s2_wgrad_operands_ok(*((dyv, xv) if down else (xv, dyv)))
        dw = torch.full((cc * cf * 8,), NAN, device="cuda")
        wg = lambda t, acc: ops.conv_k2s2_wgrad(*((dyv, xv) if down else (xv, dyv)), t.view(-1), accumulate=acc)
        wg(dw, False)
        assert ops.DISPATCH == {f"k2s2_down:{cf}x{cc}@{coarse[0]}", f"k2s2_up:{cc}x{cf}@{coarse[0]}", f"k2s2_wgrad:{cf}x{cc}@{coarse[0]}"}
    finally:
        ops.DISPATCH = keep
    gpr = 4 if coarse[2] % 16 == 0 else 2               # as mis_conv_k2s2_wgrad picks its instantiation
    xt = coarse[2] // (4 * gpr)
    kd, ku = f"k2s2_down_kernel<{cf}, {cc}>", f"k2s2_up_kernel<{cc}, {cf}>"
    kw = f"k2s2_wgrad_kernel<{cf}, {cc}, {3 if xt % 3 == 0 else 2 if xt % 2 == 0 else 1}, {gpr}>"
    chk("y", y.v, kd if down else ku)
    chk("dx", dx.v, ku if down else kd)
    chk("dw", dw, kw)
    assert y.untouched() and dx.untouched()
    _dw_accumulate(chk, kw, wg, (cc * cf * 8,))
    chk.done()


@pytest.mark.parametrize("name", co.names("gemm"))
def test_conv1x1_gemm(name):
    """conv1x1_gemm.hip: the forward and the data gradient as batched (split-K) GEMMs, the weight gradient by mis_conv1x1_wgrad;
    ragged tiles, a long contraction cut into slices, many output channels."""
    ops = _ops()
    chk = _Check(name)
    c = chk.c
    N, Cin, Cout, D, H, W = c["shape"]
    lay = _layout(c)
    xv, dyv = _in(c["x"], lay), _in(c["dy"], lay)
    w2 = c["w"].cuda().reshape(Cout, Cin)
    y, dx = _out((N, Cout, D, H, W), lay), _out((N, Cin, D, H, W), lay)
    assert ops.conv1x1_gemm_eligible(xv, y.v, Cin, Cout) and ops.conv1x1_gemm_eligible(dyv, dx.v, Cout, Cin)
    assert ops.conv1x1_wgrad_eligible(dyv, xv)
    keep, ops.DISPATCH = ops.DISPATCH, set()
    try:
        ops.conv1x1_gemm(xv, w2.t().contiguous(), c["b"].cuda(), y.v)
        ops.conv1x1_gemm(dyv, w2, None, dx.v)
        dw = torch.full((Cout, Cin), NAN, device="cuda")
        wg = lambda t, acc: ops.conv1x1_wgrad(dyv, xv, t.view(Cout, Cin), accumulate=acc)
        wg(dw, False)
        assert ops.DISPATCH == {f"conv1x1_gemm:{Cin}x{Cout}@{W}", f"conv1x1_gemm:{Cout}x{Cin}@{W}", f"conv1x1_wgrad:{Cout}x{Cin}@{W}"}
    finally:
        ops.DISPATCH = keep
    chk("y", y.v, "conv1x1_gemm")
    chk("dx", dx.v, "conv1x1_gemm")
    chk("dw", dw, "conv1x1_wgrad")
    assert y.untouched() and dx.untouched()
    _dw_accumulate(chk, "conv1x1_wgrad", wg, (Cout, Cin))
    chk.done()


@pytest.mark.parametrize("name", co.names("up2d"))
def test_transposed_convolution_2d(name):
    """nn.ConvTranspose2d(k = 2, stride = 2) as mis_hip.plan.UpConv2dOp: 1x1 MFMA convolution + pixel shuffle, its gradients by
    the direct weight-gradient and 1x1 kernels; the output is a channel slice of a wider buffer."""
    from mis_hip.plan import Act, UpConv2dOp, _PRef
    ops = _ops()
    chk = _Check(name)
    c = chk.c
    N, Cin, Cout, D, H, W = c["shape"]
    xa = Act(tensor=c["x"].cuda().contiguous())
    cat = Act((N, Cout + 8, 1, 2 * H, 2 * W))
    cat.t.fill_(NAN)
    ya = cat.slice(8, Cout)
    w4 = c["w"][:, :, 0].contiguous()
    wref = _PRef(w4.cuda(), torch.full_like(w4, NAN, device="cuda"))
    bref = _PRef(c["b"].cuda(), torch.full_like(c["b"], NAN, device="cuda"))
    op = UpConv2dOp(xa, ya, wref, bref, bias_grad=True)
    keep, ops.DISPATCH = ops.DISPATCH, set()
    try:
        op.fwd(None)
        assert torch.isnan(cat.t[:, :8]).all()
        cat.grad().fill_(NAN)
        ya.grad().copy_(c["dy"].cuda())
        op.bwd(None)
        assert f"direct_wgrad:k111@{W}" in ops.DISPATCH
    finally:
        ops.DISPATCH = keep
    L = _lib()
    kf = _name(L.mis_conv_fwd_kernel_name, N, Cin, 4 * Cout, 1, H, W, 1, 1, 1)
    kb = _name(L.mis_conv_fwd_kernel_name, N, 4 * Cout, Cin, 1, H, W, 1, 1, 1)
    kw = _name(L.mis_conv_wgrad_kernel_name, N, Cin, 4 * Cout, 1, H, W, 1, 1, 1)
    chk("y", ya.t, kf + " + shuffle")
    chk("dx", xa.grad(), kb + " + shuffle")
    chk("dw", wref.grad, kw + " + shuffle")
    chk.done()


# ---------------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["direct-ragged/relu_scaled", "wino-v1/relu_scaled", "wino-v2/relu_scaled", "split2-6/relu_scaled",
                                  "wino2d-v1/relu_scaled", "direct2d-4x4-128/relu_scaled"])
def test_exact_zeros(name):
    """An all-zero input channel: exactly zero in that channel's slice of dw.  An all-zero dy channel: exactly zero in its row
    of dw, and dx does not depend on that channel's filter.  Zero weights: y is the bias, bit for bit.  A stale LDS row or
    a cross-channel leak is non-zero here, whatever its size."""
    ops = _ops()
    c = co.case(name)
    N, Cin, Cout, D, H, W = c["shape"]
    k = c["k"]
    zi, zo = Cin // 2 + 1, Cout - 2
    x, dy = c["x"].clone(), c["dy"].clone()
    x[:, zi] = 0.0
    dy[:, zo] = 0.0
    xv, dyv, wd, bd = _in(x, "slice"), _in(dy, "slice"), c["w"].cuda(), c["b"].cuda()
    dw = torch.full(tuple(c["w"].shape), NAN, device="cuda")
    ops.conv_wgrad(xv, dyv, dw, k)
    assert torch.isfinite(dw).all() and (dw[:, zi] == 0).all() and (dw[zo] == 0).all()
    live = torch.ones(Cout, Cin, dtype=torch.bool)
    live[:, zi], live[zo] = False, False
    assert (dw.cpu().flatten(2).abs().amax(2)[live] > 0).all()
    vb = ops.conv_wino_select(N, Cout, Cin, D, H, W, k)
    mode = ops.conv_wino_pack_mode(vb, True) if vb >= 0 else 1
    w2 = wd.clone()
    w2[zo] = wd[zo].flip(0) * 37.0 + 1.0
    dxs = []
    for wt in (wd, w2):
        dx = _out((N, Cin, D, H, W), "slice")
        ops.conv_fwd(dyv, ops.conv_pack(wt, mode), None, dx.v, Cout, Cin, k, wino=vb)
        assert dx.untouched()
        dxs.append(dx.v.clone())
    assert torch.isfinite(dxs[0]).all() and torch.equal(dxs[0], dxs[1])
    v = ops.conv_wino_select(N, Cin, Cout, D, H, W, k)
    assert co.SPECS[c["id"]]["fwd"] == served(c)["fwd"]
    y = _out((N, Cout, D, H, W), "slice")
    ops.conv_fwd(_in(c["x"], "slice"), ops.conv_pack(torch.zeros_like(wd), ops.conv_wino_pack_mode(v, False) if v >= 0 else 0),
                 bd, y.v, Cin, Cout, k, wino=v)
    assert y.untouched() and torch.equal(y.v, bd.reshape(1, -1, 1, 1, 1).expand_as(y.v))
