"""Tensor-level wrappers over the C-ABI kernels (one Python function per entry point).

Activation tensors are 5-D ``[N, C, D, H, W]`` fp32 (2-D images use ``D == 1``) whose
channel/spatial dims are dense and whose batch stride is free (``>= C*D*H*W``), so
channel slices of a concatenated skip buffer are valid inputs and outputs.
Every function launches on torch's current stream and returns nothing (outputs are
caller-allocated), mirroring the C signatures in ``include/mis_hip.h``.
"""
import ctypes as _ctypes
import os as _os

import torch

from . import lib as _l

_scratch = {}


def _geom(t):
    """(N, C, D, H, W, S, batch_stride) of a 5-D activation view; validates density."""
    if t.dim() != 5 or t.dtype != torch.float32:
        raise RuntimeError(f"expected 5-D fp32 [N,C,D,H,W], got {tuple(t.shape)} {t.dtype}")
    _l.require_gpu(t)
    N, C, D, H, W = t.shape
    S = D * H * W
    st = t.stride()
    if C > 1 and st[1] != S or (D > 1 and st[2] != H * W) or (H > 1 and st[3] != W) or (W > 1 and st[4] != 1):
        raise RuntimeError(f"activation view must be dense in (C,D,H,W); strides {st} shape {tuple(t.shape)}")
    bs = st[0] if N > 1 else max(st[0], C * S)
    if bs < C * S:
        bs = C * S
    return N, C, D, H, W, S, bs


_scratch_retired = []


def scratch(nbytes, key="default"):
    """Grow-only device scratch buffer (bytes) for kernel workspaces, per device, key and stream."""
    # keyed by stream too: student and teacher forwards may run concurrently on two streams (step.py)
    k = (torch.cuda.current_device(), key, torch.cuda.current_stream().cuda_stream)
    buf = _scratch.get(k)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            # a captured hipGraph may hold raw pointers into the buffer being outgrown (an eager validation forward
            # between replays can need more workspace than the training step did): never hand it back to the allocator
            _scratch_retired.append(buf)
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device="cuda")
        _scratch[k] = buf
    return buf


# ---------------------------------------------------------------- convolution
def conv_pack(weight, mode, out=None):
    """Repack ``weight [Cout,Cin,*k]`` for conv_fwd (mode 0) or the data gradient (mode 1)."""
    L = _l.load()
    Cout, Cin = weight.shape[0], weight.shape[1]
    taps = weight[0, 0].numel()
    n = L.mis_conv_packed_floats(Cout, Cin, taps, mode)
    if n < 0:
        _l.check(n, "mis_conv_packed_floats")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=weight.device)
    assert out.numel() >= n and weight.is_contiguous()
    _l.check(L.mis_conv_pack_weights(_l.ptr(weight), _l.ptr(out), Cout, Cin, taps, mode, _l.stream_ptr()),
             "mis_conv_pack_weights")
    return out


class PackBatch:
    """All weight re-layouts of a network in one launch (``mis_conv_pack_batch``).  ``jobs``: list of
    (weight tensor [Cout,Cin,*k], packed buffer, mode); the device job table is built once."""

    def __init__(self, jobs):
        L = _l.load()
        nb = L.mis_conv_pack_job_bytes()
        host = (_ctypes.c_char * (nb * len(jobs)))()
        start = 0
        for i, (w, wp, mode) in enumerate(jobs):
            assert w.is_contiguous() and wp.is_contiguous()
            Cout, Cin = w.shape[0], w.shape[1]
            n = L.mis_conv_pack_job(_ctypes.byref(host, i * nb), _l.ptr(w), _l.ptr(wp), Cout, Cin, w[0, 0].numel(),
                                    mode, start)
            if n < 0:
                _l.check(n, "mis_conv_pack_job")
            assert wp.numel() >= n
            start += n
        self.n, self.total = len(jobs), start
        self.keep = jobs      # the table holds raw pointers into these tensors
        self.table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()

    def run(self):
        L = _l.load()
        _l.check(L.mis_conv_pack_batch(_l.ptr(self.table), self.n, self.total, _l.stream_ptr()), "mis_conv_pack_batch")


def conv_pack_raw(w, Cout, Cin, taps, mode, out=None):
    """Pack a weight buffer with explicit geometry (modes 2/3: 1x1 weight stored input-major [Cin][Cout])."""
    L = _l.load()
    n = L.mis_conv_packed_floats(Cout, Cin, taps, mode)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=w.device)
    assert out.numel() >= n and w.is_contiguous() and w.numel() == Cout * Cin * taps
    _l.check(L.mis_conv_pack_weights(_l.ptr(w), _l.ptr(out), Cout, Cin, taps, mode, _l.stream_ptr()),
             "mis_conv_pack_weights")
    return out


def space_to_depth2(src, dst, fine_shape, to_depth, bias=None, accumulate=False):
    """fine [N,C,D,H,W] <-> coarse [N,8C,D/2,H/2,W/2]; ``fine_shape`` = (N,C,D,H,W) of the fine tensor."""
    L = _l.load()
    N, C, D, H, W = fine_shape
    sbs, dbs = _geom(src)[6], _geom(dst)[6]
    _l.check(L.mis_space_to_depth2(_l.ptr(src), sbs, _l.ptr(dst), dbs, _l.ptr(bias), N, C, D, H, W, int(to_depth),
                                   int(accumulate), _l.stream_ptr()), "mis_space_to_depth2")


def space_to_depth2d(src, dst, fine_shape, to_depth, bias=None, accumulate=False):
    """2-D: fine [N,C,1,H,W] <-> coarse [N,4C,1,H/2,W/2]; ``fine_shape`` = (N,C,1,H,W) of the fine tensor."""
    L = _l.load()
    N, C, D, H, W = fine_shape
    assert D == 1
    sbs, dbs = _geom(src)[6], _geom(dst)[6]
    _l.check(L.mis_space_to_depth2d(_l.ptr(src), sbs, _l.ptr(dst), dbs, _l.ptr(bias), N, C, H, W, int(to_depth),
                                    int(accumulate), _l.stream_ptr()), "mis_space_to_depth2d")


def conv_k2s2_eligible(cin, cout, coarse, up):
    """(cin, cout) and the COARSE (Do, Ho, Wo) the in-place kernel-2 / stride-2 kernels serve (conv_k2s2.hip)."""
    return K2S2 and bool(_l.load().mis_conv_k2s2_eligible(int(cin), int(cout), *[int(v) for v in coarse], int(up)))


def conv_k2s2_wgrad_eligible(cf, cc, coarse):
    return K2S2 and bool(_l.load().mis_conv_k2s2_wgrad_eligible(int(cf), int(cc), *[int(v) for v in coarse]))


# When set to a set(), the ops below add a short tag of the path they dispatched (tests assert that the full-batch
# instantiations -- in-place kernel-2 / stride-2 kernels, Winograd weight-gradient variants -- are the ones that ran).
DISPATCH = None


def _tag(name):
    if DISPATCH is not None:
        DISPATCH.add(name)


def conv_k2s2_up_output_ok(y):
    """mis_conv_k2s2_up stores float2 pairs: the fine output (possibly a channel-slice view) must start on 8 bytes with an
    even batch stride (the kernel returns MIS_ERR_UNSUPPORTED otherwise)."""
    return y.data_ptr() % 8 == 0 and _geom(y)[6] % 2 == 0


def conv_k2s2_wgrad_operands_ok(coarse, fine):
    """mis_conv_k2s2_wgrad reads float4 rows: both operands on 16 bytes, batch strides multiples of 4 floats."""
    return (coarse.data_ptr() % 16 == 0 and fine.data_ptr() % 16 == 0 and _geom(coarse)[6] % 4 == 0
            and _geom(fine)[6] % 4 == 0)


def conv_k2s2_wgrad(coarse, fine, dw, accumulate=False):
    """dw[cc][cf*8 + tap] (+)= sum coarse[n][cc][v] * fine[n][cf][2v + tap] (mis_conv_k2s2_wgrad): the parameter gradient of
    Conv3d(k2s2) (coarse = dy, fine = x) and of ConvTranspose3d(k2s2) (coarse = x, fine = dy), in the parameter's layout."""
    L = _l.load()
    N, CC, Do, Ho, Wo, _, cbs = _geom(coarse)
    _, CF, _, _, _, _, fbs = _geom(fine)
    assert dw.is_contiguous() and dw.numel() == CC * CF * 8
    ws = scratch(L.mis_conv_k2s2_wgrad_workspace_bytes(CF, CC), "wgrad")
    _tag(f"k2s2_wgrad:{CF}x{CC}@{Do}")
    _l.check(L.mis_conv_k2s2_wgrad(_l.ptr(coarse), cbs, _l.ptr(fine), fbs, _l.ptr(dw), N, CF, CC, Do, Ho, Wo,
                                   int(accumulate), _l.ptr(ws), ws.numel(), _l.stream_ptr()), "mis_conv_k2s2_wgrad")


def conv_k2s2_down(x, w, bias, y, accumulate=False):
    """y (coarse) (+)= bias + sum w[co][ci*8 + tap] x[ci][2v + tap]: Conv3d(k2s2) forward / ConvTranspose3d(k2s2) dX."""
    L = _l.load()
    N, Cin, _, _, _, _, xbs = _geom(x)
    _, Cout, Do, Ho, Wo, _, ybs = _geom(y)
    assert w.is_contiguous() and w.numel() == Cin * Cout * 8
    _tag(f"k2s2_down:{Cin}x{Cout}@{Do}")
    _l.check(L.mis_conv_k2s2_down(_l.ptr(x), xbs, _l.ptr(w), _l.ptr(bias), _l.ptr(y), ybs, N, Cin, Cout, Do, Ho, Wo,
                                  int(accumulate), _l.stream_ptr()), "mis_conv_k2s2_down")


def conv_k2s2_up(x, w, bias, y, accumulate=False):
    """y (fine) (+)= bias + sum w[ci][co*8 + tap] x[ci][v]: ConvTranspose3d(k2s2) forward / Conv3d(k2s2) dX."""
    L = _l.load()
    N, Cin, Do, Ho, Wo, _, xbs = _geom(x)
    _, Cout, _, _, _, _, ybs = _geom(y)
    assert w.is_contiguous() and w.numel() == Cin * Cout * 8
    _tag(f"k2s2_up:{Cin}x{Cout}@{Do}")
    _l.check(L.mis_conv_k2s2_up(_l.ptr(x), xbs, _l.ptr(w), _l.ptr(bias), _l.ptr(y), ybs, N, Cin, Cout, Do, Ho, Wo,
                                int(accumulate), _l.stream_ptr()), "mis_conv_k2s2_up")


def add(a, b, out):
    """out = a (+ b if b is not None) on [N,C,D,H,W] views."""
    L = _l.load()
    N, C, D, H, W, S, abs_ = _geom(a)
    bbs = _geom(b)[6] if b is not None else 0
    obs = _geom(out)[6]
    _l.check(L.mis_add(_l.ptr(a), abs_, _l.ptr(b), bbs, _l.ptr(out), obs, N, C, S, _l.stream_ptr()), "mis_add")


def _ksize(k):
    if len(k) == 2:
        return 1, k[0], k[1]
    return tuple(k)


K2S2 = _os.environ.get("MIS_K2S2", "1") != "0"      # kernel-2 / stride-2 (de)convolutions in place (conv_k2s2.hip)
WINO = int(_os.environ.get("MIS_WINO", "3"))      # bit 0: Winograd form of the 3x3x3 convolutions, bit 1: of the 3x3 ones
# diagnostics (numerics studies, tests/test_parity_gpu.py): the 3-D forward / data gradient resp. weight gradient alone on the
# direct kernels, and the smallest volume edge W the 3-D Winograd kernels are used for
WINO_FWD = _os.environ.get("MIS_WINO_FWD", "1") != "0"
WINO_WGRAD = _os.environ.get("MIS_WINO_WGRAD", "1") != "0"
WINO_MIN_W = int(_os.environ.get("MIS_WINO_MIN_W", "0"))


WINO2D = 10       # ids >= WINO2D: variant id - WINO2D of the 2-D kernels (conv_wino2d.hip); below: 3-D (conv_wino.hip)


# 1x1x1 convolutions of small volumes with many channels (the space-to-depth form of V-Net's deep kernel-2 / stride-2 layers):
# batched GEMM instead of the spatially tiled direct kernel (conv1x1_gemm.hip).  MIS_CONV1X1_GEMM=0 switches it off
CONV1X1_GEMM = _os.environ.get("MIS_CONV1X1_GEMM", "1") != "0"
CONV1X1_GEMM_MAX_S = int(_os.environ.get("MIS_CONV1X1_GEMM_MAX_S", "4096"))


def conv1x1_gemm_eligible(x, y, cin, cout):
    """x / y: 5-D NCDHW views with dense (C, D, H, W); few voxels, many channels, sizes the GEMM's float4 rows need."""
    if not CONV1X1_GEMM:
        return False
    try:
        _, _, _, _, _, S, xbs = _geom(x)
        _, _, _, _, _, _, ybs = _geom(y)
    except RuntimeError:
        return False
    return (S <= CONV1X1_GEMM_MAX_S and S % 4 == 0 and cout % 4 == 0 and cin >= 64 and xbs % 4 == 0 and ybs % 4 == 0 and
            x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0)


def conv1x1_gemm(x, wt, bias, y, accumulate=False):
    """y[n][co][s] (+)= bias[co] + sum_ci wt[ci][co] x[n][ci][s] (mis_conv1x1_gemm); ``wt`` = the weights [Cin][Cout]."""
    L = _l.load()
    N, Cin, D, H, W, S, xbs = _geom(x)
    _, Cout, _, _, _, _, ybs = _geom(y)
    assert wt.dim() == 2 and wt.shape == (Cin, Cout) and wt.stride(1) == 1, (wt.shape, Cin, Cout)
    nb = L.mis_conv1x1_gemm_workspace_bytes(N, Cin, Cout, S)
    if nb < 0:
        _l.check(nb, "mis_conv1x1_gemm_workspace_bytes")
    ws = scratch(nb, "conv1x1") if nb > 0 else None
    _tag(f"conv1x1_gemm:{Cin}x{Cout}@{W}")
    _l.check(L.mis_conv1x1_gemm(_l.ptr(x), xbs, _l.ptr(wt), wt.stride(0), _l.ptr(bias), _l.ptr(y), ybs, N, Cin, Cout, S,
                                int(accumulate), _l.ptr(ws), nb, _l.stream_ptr()), "mis_conv1x1_gemm")


def conv1x1_wgrad_eligible(a, b):
    """a / b: the two 5-D NCDHW operands of the weight gradient (same N, D, H, W)."""
    if not CONV1X1_GEMM:
        return False
    try:
        _, _, _, _, _, S, abs_ = _geom(a)
        _, _, _, _, _, _, bbs = _geom(b)
    except RuntimeError:
        return False
    return (S <= CONV1X1_GEMM_MAX_S and S % 4 == 0 and abs_ % 4 == 0 and bbs % 4 == 0 and a.data_ptr() % 16 == 0 and
            b.data_ptr() % 16 == 0 and min(a.shape[1], b.shape[1]) >= 64)


def conv1x1_wgrad(a, b, dw, accumulate=False):
    """dw[M][Nc] (+)= sum_{image, voxel} a[.][m][s] * b[.][n][s] (mis_conv1x1_wgrad); dw: a 2-D view [a channels][b channels]."""
    L = _l.load()
    N, M, D, H, W, S, abs_ = _geom(a)
    _, Nc, _, _, _, _, bbs = _geom(b)
    assert dw.dim() == 2 and dw.shape == (M, Nc) and dw.stride(1) == 1, (dw.shape, M, Nc)
    nb = L.mis_conv1x1_wgrad_workspace_bytes(N, M, Nc, S)
    if nb < 0:
        _l.check(nb, "mis_conv1x1_wgrad_workspace_bytes")
    ws = scratch(nb, "conv1x1_wgrad")
    _tag(f"conv1x1_wgrad:{M}x{Nc}@{W}")
    _l.check(L.mis_conv1x1_wgrad(_l.ptr(a), abs_, _l.ptr(b), bbs, _l.ptr(dw), dw.stride(0), N, M, Nc, S, int(accumulate),
                                 _l.ptr(ws), nb, _l.stream_ptr()), "mis_conv1x1_wgrad")


def conv_wino_select(N, Cin, Cout, D, H, W, ksize, dilation=1):
    """Winograd variant serving this convolution (mis_conv3d_wino_select / mis_conv2d_wino_select), or -1: use the
    direct kernel.  A dilated convolution has no Winograd form here: -1."""
    if not WINO or dilation != 1:
        return -1
    k = _ksize(ksize)
    if k == (3, 3, 3) and (WINO & 1):
        if not WINO_FWD or W < WINO_MIN_W:
            return -1
        return int(_l.load().mis_conv3d_wino_select(N, Cin, Cout, D, H, W))
    if k == (1, 3, 3) and D == 1 and (WINO & 2):
        v = int(_l.load().mis_conv2d_wino_select(N, Cin, Cout, H, W))
        return v + WINO2D if v >= 0 else -1
    return -1


def conv_wino_pack_mode(wino, dgrad):
    """Pack mode of the transformed filter for this variant (4 / 5: 3x3x3, 6 / 7: 3x3; forward / data gradient)."""
    return (6 if wino >= WINO2D else 4) + (1 if dgrad else 0)


def conv_stat_tiles(N, Cin, Cout, D, H, W, ksize, wino=-1):
    """Partial-statistics tiles per image of the fused conv+stats form for this geometry (0: not eligible)."""
    kd, kh, kw = _ksize(ksize)
    if wino >= WINO2D:
        t = _l.load().mis_conv2d_wino_stat_tiles(H, W, wino - WINO2D)
    elif wino >= 0:
        t = _l.load().mis_conv3d_wino_stat_tiles(D, H, W, wino)
    else:
        t = _l.load().mis_conv_fwd_stat_tiles(N, Cin, Cout, D, H, W, kd, kh, kw)
    if t < 0:
        _l.check(t, "mis_conv_fwd_stat_tiles")
    return int(t)


def norm_stats_finalize(part, N, C, S, tiles, per_sample, eps, mean, rstd, running_mean=None, running_var=None,
                        num_batches=None, momentum=0.1):
    L = _l.load()
    _l.check(L.mis_norm_stats_finalize(_l.ptr(part), N, C, S, tiles, int(per_sample), eps, _l.ptr(mean), _l.ptr(rstd),
                                       _l.ptr(running_mean), _l.ptr(running_var), _l.ptr(num_batches), momentum,
                                       _l.stream_ptr()), "mis_norm_stats_finalize")


def conv_fwd(x, wp, bias, y, Cin, Cout, ksize, stat=None, wino=-1):
    """y = conv(x) with packed weights ``wp``; stride 1, 'same' zero padding, k in {1,3}.
    ``stat = (buffer, stride_channel, stride_image)``: also emit the per-tile (sum, sumsq) of y (mis_conv_fwd_stats).
    ``wino >= 0``: ``wp`` is the Winograd-transformed filter (pack mode 4 / 5) and that variant of
    mis_conv3d_wino_fwd runs."""
    L = _l.load()
    N, Cx, D, H, W, S, xbs = _geom(x)
    Ny, Cy, Dy, Hy, Wy, _, ybs = _geom(y)
    assert Cx == Cin and Cy == Cout and (N, D, H, W) == (Ny, Dy, Hy, Wy)
    kd, kh, kw = _ksize(ksize)
    prof = PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    if wino >= WINO2D:
        st = stat if stat is not None else (None, 0, 0)
        _l.check(L.mis_conv2d_wino_fwd(_l.ptr(x), xbs, _l.ptr(wp), _l.ptr(bias), _l.ptr(y), ybs, N, Cin, Cout, H, W,
                                       _l.ptr(st[0]), st[1], st[2], wino - WINO2D, _l.stream_ptr()), "mis_conv2d_wino_fwd")
    elif wino >= 0:
        st = stat if stat is not None else (None, 0, 0)
        # few boxes (the 6^3 level, half batches at 12^3): the contraction is cut into slices, partials in scratch
        nb = L.mis_conv3d_wino_fwd_workspace_bytes(N, Cin, Cout, D, H, W, wino)
        if nb < 0:
            _l.check(nb, "mis_conv3d_wino_fwd_workspace_bytes")
        ws = scratch(nb, "wino_fwd") if nb > 0 else None
        if ws is not None:
            _tag(f"wino_fwd_split:v{wino}@{W}")
        _l.check(L.mis_conv3d_wino_fwd_ws(_l.ptr(x), xbs, _l.ptr(wp), _l.ptr(bias), _l.ptr(y), ybs, N, Cin, Cout, D, H, W,
                                          _l.ptr(st[0]), st[1], st[2], wino, _l.ptr(ws), nb, _l.stream_ptr()),
                 "mis_conv3d_wino_fwd_ws")
    elif stat is not None:
        _l.check(L.mis_conv_fwd_stats(_l.ptr(x), xbs, _l.ptr(wp), _l.ptr(bias), _l.ptr(y), ybs, N, Cin, Cout, D, H, W,
                                      kd, kh, kw, _l.ptr(stat[0]), stat[1], stat[2], _l.stream_ptr()),
                 "mis_conv_fwd_stats")
    else:
        _l.check(L.mis_conv_fwd(_l.ptr(x), xbs, _l.ptr(wp), _l.ptr(bias), _l.ptr(y), ybs, N, Cin, Cout, D, H, W,
                                kd, kh, kw, _l.stream_ptr()), "mis_conv_fwd")
    if prof is not None:
        e1.record()
        buf = _ctypes.create_string_buffer(128)
        if wino >= WINO2D:
            L.mis_conv2d_wino_kernel_name(wino - WINO2D, buf, 128)
        elif wino >= 0:
            L.mis_conv3d_wino_kernel_name(wino, buf, 128)
        else:
            L.mis_conv_fwd_kernel_name(N, Cin, Cout, D, H, W, kd, kh, kw, buf, 128)
        prof.append((buf.value.decode(), 2.0 * N * Cout * Cin * kd * kh * kw * S, e0, e1,
                     4.0 * (N * (Cin + Cout) * S + Cout * Cin * kd * kh * kw)))


# When set to a list, conv_fwd brackets every launch with HIP events on the launch stream and appends
# (kernel name, algorithmic FLOPs, start event, end event, algorithmic bytes = operands read once + result written once):
# bench.py's live roofline measurement.
PROFILE = None


def conv_dgrad_norm(dy, wpd, da, Cin, Cout, xn, mean, slope, part, wino):
    """The Winograd data gradient ``da = dgrad(dy)`` (``wpd``: pack mode 5) with the first stage of the backward of the
    InstanceNorm + (Leaky)ReLU that produced the conv's input from ``xn`` in its epilogue (mis_conv3d_wino_dgrad_norm):
    ``part [N*Cout*tiles, 2]`` receives (sum dz, sum dz * xn) per (n, channel, tile).  ``Cin`` / ``Cout``: channels of
    dy / da.  Returns the number of tiles per image."""
    L = _l.load()
    N, C, D, H, W, S, dbs = _geom(dy)
    _, _, _, _, _, _, abs_ = _geom(da)
    _, _, _, _, _, _, xbs = _geom(xn)
    assert C == Cin and da.shape[1] == Cout and xn.shape[1] == Cout
    tiles = int(L.mis_conv3d_wino_stat_tiles(D, H, W, wino))
    assert part.numel() >= N * Cout * tiles * 2
    prof = PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _l.check(L.mis_conv3d_wino_dgrad_norm(_l.ptr(dy), dbs, _l.ptr(wpd), _l.ptr(da), abs_, N, Cin, Cout, D, H, W,
                                          _l.ptr(xn), xbs, _l.ptr(mean), float(slope), _l.ptr(part), tiles, Cout * tiles,
                                          wino, _l.stream_ptr()), "mis_conv3d_wino_dgrad_norm")
    if prof is not None:
        e1.record()
        buf = _ctypes.create_string_buffer(128)
        L.mis_conv3d_wino_kernel_name(wino, buf, 128)
        prof.append((buf.value.decode().replace(", false>", ", true>"), 2.0 * N * Cout * Cin * 27 * S, e0, e1,
                     4.0 * (N * (Cin + 2 * Cout) * S + Cout * Cin * 27)))     # + the norm input it reads
    return tiles


def norm_act_bwd_tiles(x, da, dx, mean, rstd, slope, part, tiles, sums):
    """Second stage + apply pass of the InstanceNorm + (Leaky)ReLU backward from conv_dgrad_norm's partials; ``dx`` may
    be None (only ``sums`` is wanted: the first layer's weight gradient forms dx itself)."""
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    _, _, _, _, _, _, dabs = _geom(da)
    dxbs = _geom(dx)[6] if dx is not None else 0
    _l.check(L.mis_norm_act_bwd_tiles(_l.ptr(x), xbs, _l.ptr(da), dabs, _l.ptr(dx), dxbs, N, C, S, _l.ptr(mean),
                                      _l.ptr(rstd), float(slope), _l.ptr(part), int(tiles), _l.ptr(sums),
                                      _l.stream_ptr()), "mis_norm_act_bwd_tiles")


def conv_wgrad(x, dy, dw, ksize, accumulate=False):
    """dw[Cout,Cin,*k] (+)= sum_n,p dy * shifted x."""
    L = _l.load()
    N, Cin, D, H, W, S, xbs = _geom(x)
    _, Cout, _, _, _, _, dbs = _geom(dy)
    kd, kh, kw = _ksize(ksize)
    assert dw.is_contiguous() and dw.numel() == Cout * Cin * kd * kh * kw
    prof = PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    name = _conv_wgrad_launch(L, x, dy, dw, N, Cin, Cout, D, H, W, xbs, dbs, kd, kh, kw, accumulate)
    if prof is not None:       # bench.py's live roofline: the weight gradients count towards the executed step flops
        e1.record()
        prof.append((name, 2.0 * N * Cout * Cin * kd * kh * kw * S, e0, e1,
                     4.0 * (N * (Cin + Cout) * S + Cout * Cin * kd * kh * kw)))


def _conv_wgrad_launch(L, x, dy, dw, N, Cin, Cout, D, H, W, xbs, dbs, kd, kh, kw, accumulate):
    # 3x3x3 on large volumes: the Winograd F(2^3, 3^3) form (conv_wino_wgrad.hip), 3.375x fewer matrix-pipe flops
    wino = int(L.mis_conv3d_wino_wgrad_select(N, Cin, Cout, D, H, W)) if ((WINO & 1) and WINO_WGRAD and W >= WINO_MIN_W and
                                                                          (kd, kh, kw) == (3, 3, 3)) else -1
    if wino >= 0 and xbs % 4 == 0 and dbs % 4 == 0 and x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0:
        nb = L.mis_conv3d_wino_wgrad_workspace_bytes(N, Cin, Cout, D, H, W, wino)
        if nb < 0:
            _l.check(nb, "mis_conv3d_wino_wgrad_workspace_bytes")
        ws = scratch(nb, "wgrad")
        _tag(f"wino_wgrad:v{wino}@{W}")
        _l.check(L.mis_conv3d_wino_wgrad(_l.ptr(x), xbs, _l.ptr(dy), dbs, _l.ptr(dw), _l.ptr(ws), ws.numel(), N, Cin,
                                         Cout, D, H, W, int(accumulate), wino, _l.stream_ptr()), "mis_conv3d_wino_wgrad")
        buf = _ctypes.create_string_buffer(96)
        _l.check(L.mis_conv3d_wino_wgrad_kernel_name(wino, buf, 96), "mis_conv3d_wino_wgrad_kernel_name")
        return buf.value.decode()
    wino2 = int(L.mis_conv2d_wino_wgrad_select(N, Cin, Cout, H, W)) if ((WINO & 2) and (kd, kh, kw) == (1, 3, 3) and D == 1) else -1
    if wino2 >= 0 and xbs % 4 == 0 and dbs % 4 == 0 and x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0:
        nb = L.mis_conv2d_wino_wgrad_workspace_bytes(N, Cin, Cout, H, W, wino2)
        if nb < 0:
            _l.check(nb, "mis_conv2d_wino_wgrad_workspace_bytes")
        ws = scratch(nb, "wgrad")
        _l.check(L.mis_conv2d_wino_wgrad(_l.ptr(x), xbs, _l.ptr(dy), dbs, _l.ptr(dw), _l.ptr(ws), ws.numel(), N, Cin, Cout,
                                         H, W, int(accumulate), wino2, _l.stream_ptr()), "mis_conv2d_wino_wgrad")
        buf = _ctypes.create_string_buffer(96)
        _l.check(L.mis_conv2d_wino_wgrad_kernel_name(wino2, buf, 96), "mis_conv2d_wino_wgrad_kernel_name")
        return buf.value.decode()
    nb = L.mis_conv_wgrad_workspace_bytes(N, Cin, Cout, D, H, W, kd, kh, kw)
    if nb < 0:
        _l.check(nb, "mis_conv_wgrad_workspace_bytes")
    ws = scratch(nb, "wgrad")
    _tag(f"direct_wgrad:k{kd}{kh}{kw}@{W}")
    _l.check(L.mis_conv_wgrad(_l.ptr(x), xbs, _l.ptr(dy), dbs, _l.ptr(dw), _l.ptr(ws), ws.numel(), N, Cin, Cout,
                              D, H, W, kd, kh, kw, int(accumulate), _l.stream_ptr()), "mis_conv_wgrad")
    buf = _ctypes.create_string_buffer(96)
    _l.check(L.mis_conv_wgrad_kernel_name(N, Cin, Cout, D, H, W, kd, kh, kw, buf, 96), "mis_conv_wgrad_kernel_name")
    return buf.value.decode()


# ------------------------------------------------------- dilated 3x3 convolution (conv_dilated.hip, mis_hip_dilated.h)
def _dilated_geom(x, y):
    N, Cx, D, H, W, S, xbs = _geom(x)
    Ny, Cy, Dy, Hy, Wy, _, ybs = _geom(y)
    if D != 1 or (N, D, H, W) != (Ny, Dy, Hy, Wy):
        raise RuntimeError(f"dilated convolution: 2-D tensors of one geometry expected, got {tuple(x.shape)} {tuple(y.shape)}")
    return N, Cx, Cy, H, W, xbs, ybs


def _dilated_name(fn, N, Cin, Cout, H, W, dilation):
    buf = _ctypes.create_string_buffer(128)
    _l.check(getattr(_l.load(), fn)(N, Cin, Cout, H, W, int(dilation), buf, 128), fn)
    return buf.value.decode()


def conv_dilated_fwd_kernel_name(N, Cin, Cout, H, W, dilation):
    return _dilated_name("mis_conv_dilated_fwd_kernel_name", N, Cin, Cout, H, W, dilation)


def conv_dilated_dgrad_kernel_name(N, Cin, Cout, H, W, dilation):
    return _dilated_name("mis_conv_dilated_dgrad_kernel_name", N, Cin, Cout, H, W, dilation)


def conv_dilated_wgrad_kernel_name(N, Cin, Cout, H, W, dilation):
    return _dilated_name("mis_conv_dilated_wgrad_kernel_name", N, Cin, Cout, H, W, dilation)


def conv_dilated_fwd(x, wp, bias, y, dilation, dgrad=False):
    """y = bias + conv3x3(x, dilation = padding = ``dilation``) with packed weights ``wp`` (mode 0, taps = 9).
    ``dgrad``: ``x`` is the output gradient, ``wp`` the mode-1 pack and ``y`` receives the input gradient (no bias)."""
    L = _l.load()
    N, Cx, Cy, H, W, xbs, ybs = _dilated_geom(x, y)
    prof = PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    if dgrad:
        assert bias is None
        _l.check(L.mis_conv_dilated_dgrad(_l.ptr(x), xbs, _l.ptr(wp), _l.ptr(y), ybs, N, Cy, Cx, H, W, int(dilation),
                                          _l.stream_ptr()), "mis_conv_dilated_dgrad")
    else:
        _l.check(L.mis_conv_dilated_fwd(_l.ptr(x), xbs, _l.ptr(wp), _l.ptr(bias), _l.ptr(y), ybs, N, Cx, Cy, H, W,
                                        int(dilation), _l.stream_ptr()), "mis_conv_dilated_fwd")
    if prof is not None:
        e1.record()
        prof.append((conv_dilated_fwd_kernel_name(N, Cx, Cy, H, W, dilation), 2.0 * N * Cy * Cx * 9 * H * W, e0, e1,
                     4.0 * (N * (Cx + Cy) * H * W + Cy * Cx * 9)))


def conv_dilated_wgrad(x, dy, dw, dilation, accumulate=False):
    """dw[Cout,Cin,3,3] (+)= the weight gradient of the dilated convolution; deterministic."""
    L = _l.load()
    N, Cin, Cout, H, W, xbs, dbs = _dilated_geom(x, dy)
    assert dw.is_contiguous() and dw.numel() == Cout * Cin * 9
    nb = L.mis_conv_dilated_wgrad_workspace_bytes(N, Cin, Cout, H, W, int(dilation))
    if nb < 0:
        _l.check(nb, "mis_conv_dilated_wgrad_workspace_bytes")
    ws = scratch(nb, "wgrad")
    prof = PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _tag(f"dilated_wgrad:d{dilation}@{W}")
    _l.check(L.mis_conv_dilated_wgrad(_l.ptr(x), xbs, _l.ptr(dy), dbs, _l.ptr(dw), _l.ptr(ws), ws.numel(), N, Cin, Cout, H, W,
                                      int(dilation), int(accumulate), _l.stream_ptr()), "mis_conv_dilated_wgrad")
    if prof is not None:
        e1.record()
        prof.append((conv_dilated_wgrad_kernel_name(N, Cin, Cout, H, W, dilation), 2.0 * N * Cout * Cin * 9 * H * W, e0, e1,
                     4.0 * (N * (Cin + Cout) * H * W + Cout * Cin * 9)))


# ------------------------------------------------------- norm + act + dropout
def norm_stats(x, per_sample, eps, mean, rstd, running_mean=None, running_var=None, num_batches=None,
               momentum=0.1):
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    nb = L.mis_norm_workspace_bytes(N, C, S, int(per_sample))
    ws = scratch(nb, "norm")
    _l.check(L.mis_norm_stats(_l.ptr(x), xbs, N, C, S, int(per_sample), eps, _l.ptr(mean), _l.ptr(rstd),
                              _l.ptr(running_mean), _l.ptr(running_var), _l.ptr(num_batches), momentum,
                              _l.ptr(ws), ws.numel(), _l.stream_ptr()), "mis_norm_stats")


def channel_sum(x, out, accumulate=False):
    """out[c] (+)= sum_{n,s} x[n,c,s]  (conv bias gradient)."""
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    nb = L.mis_norm_workspace_bytes(N, C, S, 0)
    ws = scratch(nb, "norm")
    _l.check(L.mis_channel_sum(_l.ptr(x), xbs, N, C, S, _l.ptr(out), int(accumulate), _l.ptr(ws), ws.numel(),
                               _l.stream_ptr()), "mis_channel_sum")


def norm_stats_from_running(running_mean, running_var, eps, mean, rstd):
    L = _l.load()
    _l.check(L.mis_norm_stats_from_running(_l.ptr(running_mean), _l.ptr(running_var), eps, _l.ptr(mean),
                                           _l.ptr(rstd), running_mean.numel(), _l.stream_ptr()),
             "mis_norm_stats_from_running")


def norm_act_fwd(x, y, per_sample, mean, rstd, gamma, beta, slope, drop_p=0.0, drop_salt=0, state=None,
                 drop_mask=None, cg=1):
    """``cg``: channels per statistics group of a per-sample norm (1 InstanceNorm, C/16 GroupNorm(16))."""
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    _, _, _, _, _, _, ybs = _geom(y)
    _l.check(L.mis_norm_act_fwd_g(_l.ptr(x), xbs, _l.ptr(y), ybs, N, C, S, int(per_sample), int(cg), _l.ptr(mean),
                                  _l.ptr(rstd), _l.ptr(gamma), _l.ptr(beta), slope, drop_p, drop_salt,
                                  _l.ptr(state), _l.ptr(drop_mask), _l.stream_ptr()), "mis_norm_act_fwd_g")


def norm_act_bwd(x, da, dx, per_sample, mean, rstd, gamma, beta, slope, drop_p=0.0, drop_salt=0, state=None,
                 drop_mask=None, dgamma=None, dbeta=None, accumulate_affine=False, cg=1, no_norm=False):
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    _, _, _, _, _, _, dabs = _geom(da)
    _, _, _, _, _, _, dxbs = _geom(dx)
    nb = L.mis_norm_workspace_bytes(N, C, S, int(per_sample))
    ws = scratch(nb, "norm")
    _l.check(L.mis_norm_act_bwd_g(_l.ptr(x), xbs, _l.ptr(da), dabs, _l.ptr(dx), dxbs, N, C, S, int(per_sample),
                                  int(cg), int(no_norm), _l.ptr(mean), _l.ptr(rstd), _l.ptr(gamma), _l.ptr(beta),
                                  slope, drop_p, drop_salt, _l.ptr(state), _l.ptr(drop_mask), _l.ptr(dgamma),
                                  _l.ptr(dbeta), int(accumulate_affine), _l.ptr(ws), ws.numel(), _l.stream_ptr()),
             "mis_norm_act_bwd_g")


def norm_res_act_fwd(x, res, y, per_sample, mean, rstd, gamma, beta, slope, post=False):
    """y = act(norm(x) + res) in one pass (mis_norm_res_act_fwd); ``post``: y = act(norm(x)) + res."""
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    rbs, ybs = _geom(res)[6], _geom(y)[6]
    _l.check(L.mis_norm_res_act_fwd(_l.ptr(x), xbs, _l.ptr(res), rbs, _l.ptr(y), ybs, N, C, S, int(per_sample),
                                    _l.ptr(mean), _l.ptr(rstd), _l.ptr(gamma), _l.ptr(beta), slope, int(post),
                                    _l.stream_ptr()), "mis_norm_res_act_fwd")


def norm_res_act_bwd(x, res, dy, dx, dres, accumulate_dres, per_sample, mean, rstd, gamma, beta, slope, dgamma=None,
                     dbeta=None, accumulate_affine=False, post=False):
    """Backward of norm_res_act_fwd: dres (+)= dz, dx = norm backward of dz, dz = dy * act'(norm(x) + res)."""
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    rbs, dybs, dxbs, drbs = _geom(res)[6], _geom(dy)[6], _geom(dx)[6], _geom(dres)[6]
    ws = scratch(L.mis_norm_workspace_bytes(N, C, S, int(per_sample)), "norm")
    _l.check(L.mis_norm_res_act_bwd(_l.ptr(x), xbs, _l.ptr(res), rbs, _l.ptr(dy), dybs, _l.ptr(dx), dxbs, _l.ptr(dres),
                                    drbs, int(accumulate_dres), N, C, S, int(per_sample), _l.ptr(mean), _l.ptr(rstd),
                                    _l.ptr(gamma), _l.ptr(beta), slope, _l.ptr(dgamma), _l.ptr(dbeta),
                                    int(accumulate_affine), int(post), _l.ptr(ws), ws.numel(), _l.stream_ptr()),
             "mis_norm_res_act_bwd")


def norm_act_fwd_pool(x, y, pooled, idx, per_sample, mean, rstd, gamma, beta, slope, drop_p=0.0, drop_salt=0, state=None,
                      drop_mask=None, cg=1):
    """norm_act_fwd and the 2x max-pool of its output (pooled, idx as maxpool2_fwd writes them) in one pass."""
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    _, _, _, _, _, _, ybs = _geom(y)
    _, _, _, _, _, _, pbs = _geom(pooled)
    _l.check(L.mis_norm_act_fwd_pool(_l.ptr(x), xbs, _l.ptr(y), ybs, _l.ptr(pooled), pbs, _l.ptr(idx), N, C, D, H, W,
                                     int(per_sample), int(cg), _l.ptr(mean), _l.ptr(rstd), _l.ptr(gamma), _l.ptr(beta),
                                     slope, drop_p, drop_salt, _l.ptr(state), _l.ptr(drop_mask), _l.stream_ptr()),
             "mis_norm_act_fwd_pool")


def norm_act_bwd_pool(x, da, dpool, idx, dx, per_sample, mean, rstd, gamma, beta, slope, drop_p=0.0, drop_salt=0,
                      state=None, drop_mask=None, dgamma=None, dbeta=None, accumulate_affine=False, cg=1):
    """norm_act_bwd of an activation that also feeds a 2x max-pool: incoming gradient = da (None: no other consumer) +
    the pool's backward of dpool through the argmax codes idx, added on the load path (no maxpool2_bwd pass)."""
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    dabs = _geom(da)[6] if da is not None else 0
    _, _, _, _, _, _, dpbs = _geom(dpool)
    _, _, _, _, _, _, dxbs = _geom(dx)
    ws = scratch(L.mis_norm_workspace_bytes(N, C, S, int(per_sample)), "norm")
    _l.check(L.mis_norm_act_bwd_pool(_l.ptr(x), xbs, _l.ptr(da), dabs, _l.ptr(dpool), dpbs, _l.ptr(idx), _l.ptr(dx), dxbs,
                                     N, C, D, H, W, int(per_sample), int(cg), _l.ptr(mean), _l.ptr(rstd), _l.ptr(gamma),
                                     _l.ptr(beta), slope, drop_p, drop_salt, _l.ptr(state), _l.ptr(drop_mask),
                                     _l.ptr(dgamma), _l.ptr(dbeta), int(accumulate_affine), _l.ptr(ws), ws.numel(),
                                     _l.stream_ptr()), "mis_norm_act_bwd_pool")


def norm_act_bwd_sums(x, da, per_sample, mean, rstd, gamma, beta, slope, sums, dgamma=None, dbeta=None,
                      accumulate_affine=False):
    """The reduction half of norm_act_bwd: sums[group] = (mean dz, mean dz*xhat) (+ dgamma / dbeta); no dropout."""
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    _, _, _, _, _, _, dabs = _geom(da)
    ws = scratch(L.mis_norm_workspace_bytes(N, C, S, int(per_sample)), "norm")
    _l.check(L.mis_norm_act_bwd_sums(_l.ptr(x), xbs, _l.ptr(da), dabs, N, C, S, int(per_sample), _l.ptr(mean),
                                     _l.ptr(rstd), _l.ptr(gamma), _l.ptr(beta), slope, _l.ptr(sums), _l.ptr(dgamma),
                                     _l.ptr(dbeta), int(accumulate_affine), _l.ptr(ws), ws.numel(), _l.stream_ptr()),
             "mis_norm_act_bwd_sums")


def conv_wgrad_cin1_norm_eligible(N, Cout, D, H, W):
    return bool(_l.load().mis_conv_wgrad_cin1_norm_eligible(N, Cout, D, H, W))


def conv_wgrad_cin1_norm(x, da, y, per_sample, mean, rstd, gamma, beta, sums, slope, dw, accumulate=False):
    """dw of the first layer Conv3d(1 -> 16, 3) from the gradient at the activation after its norm + (Leaky)ReLU."""
    L = _l.load()
    N, Cin, D, H, W, S, xbs = _geom(x)
    _, _, _, _, _, _, dabs = _geom(da)
    _, Cout, _, _, _, _, ybs = _geom(y)
    nb = L.mis_conv_wgrad_workspace_bytes(N, Cin, Cout, D, H, W, 1 if D == 1 else 3, 3, 3)
    if nb < 0:
        _l.check(nb, "mis_conv_wgrad_workspace_bytes")
    ws = scratch(nb, "wgrad")
    _l.check(L.mis_conv_wgrad_cin1_norm(_l.ptr(x), xbs, _l.ptr(da), dabs, _l.ptr(y), ybs, N, D, H, W, int(per_sample),
                                        _l.ptr(mean), _l.ptr(rstd), _l.ptr(gamma), _l.ptr(beta), _l.ptr(sums), slope,
                                        _l.ptr(dw), _l.ptr(ws), ws.numel(), int(accumulate), _l.stream_ptr()),
             "mis_conv_wgrad_cin1_norm")


def norm_head_eligible(C, K, per_sample, gamma, beta, cg=1, no_norm=False):
    """norm + act + dropout + 1x1x1 classifier as one pass (mis_norm_head_*): C == 16, K in 2..4, one statistics group per
    channel, InstanceNorm only without affine."""
    return bool(_l.load().mis_norm_head_eligible(C, K)) and cg == 1 and not no_norm and not (
        per_sample and (gamma is not None or beta is not None))


def norm_head_fwd(x, logits, per_sample, mean, rstd, gamma, beta, slope, w, b, drop_p=0.0, drop_salt=0, state=None,
                  drop_mask=None):
    """logits = W . drop(act(norm(x))) + b without storing the activation (w: [K, C] view of the 1x1x1 conv weight)."""
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    _, K, _, _, _, _, lbs = _geom(logits)
    _l.check(L.mis_norm_head_fwd(_l.ptr(x), xbs, N, C, S, int(per_sample), _l.ptr(mean), _l.ptr(rstd), _l.ptr(gamma),
                                 _l.ptr(beta), slope, drop_p, drop_salt, _l.ptr(state), _l.ptr(drop_mask), _l.ptr(w),
                                 _l.ptr(b), K, _l.ptr(logits), lbs, _l.stream_ptr()), "mis_norm_head_fwd")


def norm_head_bwd(x, dlogits, dx, per_sample, mean, rstd, gamma, beta, slope, w, dw, db, drop_p=0.0, drop_salt=0,
                  state=None, drop_mask=None, dgamma=None, dbeta=None, accumulate_affine=False, accumulate_w=False):
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    _, K, _, _, _, _, dlbs = _geom(dlogits)
    _, _, _, _, _, _, dxbs = _geom(dx)
    nb = L.mis_norm_head_workspace_bytes(N, C, S, int(per_sample), K)
    ws = scratch(nb, "norm")
    _l.check(L.mis_norm_head_bwd(_l.ptr(x), xbs, _l.ptr(dlogits), dlbs, _l.ptr(dx), dxbs, N, C, S, int(per_sample),
                                 _l.ptr(mean), _l.ptr(rstd), _l.ptr(gamma), _l.ptr(beta), slope, drop_p, drop_salt,
                                 _l.ptr(state), _l.ptr(drop_mask), _l.ptr(w), K, _l.ptr(dgamma), _l.ptr(dbeta),
                                 int(accumulate_affine), _l.ptr(dw), _l.ptr(db), int(accumulate_w), _l.ptr(ws),
                                 ws.numel(), _l.stream_ptr()), "mis_norm_head_bwd")


def group_norm_stats(x, cg, eps, mean, rstd):
    """(mean, rstd) per (n, group of ``cg`` consecutive channels): the groups are contiguous in NCDHW, so this is the
    InstanceNorm statistics kernel on the [N, C/cg, cg*S] view of the same memory."""
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    G = C // cg
    nb = L.mis_norm_workspace_bytes(N, G, cg * S, 1)
    ws = scratch(nb, "norm")
    _l.check(L.mis_norm_stats(_l.ptr(x), xbs, N, G, cg * S, 1, eps, _l.ptr(mean), _l.ptr(rstd), None, None, None,
                              0.0, _l.ptr(ws), ws.numel(), _l.stream_ptr()), "mis_norm_stats")


# ------------------------------------------------------------ pool / upsample
def maxpool2_fwd(x, y, idx):
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    _, _, _, _, _, _, ybs = _geom(y)
    _l.check(L.mis_maxpool2_fwd(_l.ptr(x), xbs, _l.ptr(y), ybs, _l.ptr(idx), N, C, D, H, W, _l.stream_ptr()),
             "mis_maxpool2_fwd")


def maxpool2_bwd(dy, idx, dx, accumulate=False):
    L = _l.load()
    N, C, D, H, W, S, dxbs = _geom(dx)
    _, _, _, _, _, _, dybs = _geom(dy)
    _l.check(L.mis_maxpool2_bwd(_l.ptr(dy), dybs, _l.ptr(idx), _l.ptr(dx), dxbs, N, C, D, H, W, int(accumulate),
                                _l.stream_ptr()), "mis_maxpool2_bwd")


def upsample2_fwd(x, y, align_corners):
    L = _l.load()
    N, C, D, H, W, S, xbs = _geom(x)
    _, _, _, _, _, _, ybs = _geom(y)
    _l.check(L.mis_upsample2_fwd(_l.ptr(x), xbs, _l.ptr(y), ybs, N, C, D, H, W, int(align_corners),
                                 _l.stream_ptr()), "mis_upsample2_fwd")


def upsample2_bwd(dy, dx, align_corners, accumulate=False):
    L = _l.load()
    N, C, D, H, W, S, dxbs = _geom(dx)
    _, _, _, _, _, _, dybs = _geom(dy)
    _l.check(L.mis_upsample2_bwd(_l.ptr(dy), dybs, _l.ptr(dx), dxbs, N, C, D, H, W, int(align_corners),
                                 int(accumulate), _l.stream_ptr()), "mis_upsample2_bwd")


# ------------------------------------------------------------------ loss tail
def loss_tail(student, teacher, label, labeled_bs, out, dlogits=None, cons_weight=0.0, state=None,
              loss_scale=1.0):
    """Fused softmax/CE/Dice/consistency.  ``out``: >= 5+C floats:
    [loss, loss_ce, loss_dice, consistency_loss, consistency_weight, class-wise dice...]."""
    L = _l.load()
    B, C, D, H, W, S, sbs = _geom(student)
    tbs = 0
    if teacher is not None:
        Bt, Ct, _, _, _, St, tbs = _geom(teacher)
        assert Bt == B - labeled_bs and Ct == C and St == S
    if label is not None:
        _l.require_gpu(label)
        assert label.is_contiguous() and label.dtype in (torch.uint8, torch.int64)
        assert label.numel() >= labeled_bs * S
    lb = 1 if (label is None or label.dtype == torch.uint8) else 8
    dbs = 0
    if dlogits is not None:
        dbs = _geom(dlogits)[6]
    nb = L.mis_loss_tail_workspace_bytes(B, C, S)
    ws = scratch(nb, "tail")
    _l.check(L.mis_loss_tail(_l.ptr(student), sbs, _l.ptr(teacher), tbs, _l.ptr(label), lb, B, labeled_bs, C, S,
                             cons_weight, _l.ptr(state), loss_scale, _l.ptr(out), _l.ptr(dlogits), dbs,
                             _l.ptr(ws), ws.numel(), _l.stream_ptr()), "mis_loss_tail")


def softmax_mean_accumulate(logits, acc, repeats, scale, first):
    """acc[u] (+)= scale * sum_r softmax(logits[r*U + u]) over the channel dim (UA-MT MC-dropout mean)."""
    L = _l.load()
    Bl, C, D, H, W, S, lbs = _geom(logits)
    U, Ca, _, _, _, Sa, abs_ = _geom(acc)
    assert Bl == repeats * U and Ca == C and Sa == S
    _l.check(L.mis_softmax_mean_accumulate(_l.ptr(logits), lbs, _l.ptr(acc), abs_, U, repeats, C, S, scale,
                                           int(first), _l.stream_ptr()), "mis_softmax_mean_accumulate")


def uamt_tail(student, teacher, mean_probs, label, labeled_bs, out, max_iterations, dlogits=None, cons_weight=0.0,
              state=None, iter_num=0, loss_scale=1.0):
    """UA-MT loss tail.  ``out`` (>= 7+C floats): [loss, loss_ce, loss_dice, consistency_loss, consistency_weight,
    class-wise dice..., #unmasked voxels, threshold]."""
    L = _l.load()
    B, C, D, H, W, S, sbs = _geom(student)
    Bt, Ct, _, _, _, St, tbs = _geom(teacher)
    Bm, Cm, _, _, _, Sm, mbs = _geom(mean_probs)
    assert Bt == Bm == B - labeled_bs and Ct == Cm == C and St == Sm == S
    _l.require_gpu(label)
    assert label.is_contiguous() and label.dtype in (torch.uint8, torch.int64) and label.numel() >= labeled_bs * S
    lb = 1 if label.dtype == torch.uint8 else 8
    dbs = _geom(dlogits)[6] if dlogits is not None else 0
    nb = L.mis_uamt_tail_workspace_bytes(B, C, S)
    ws = scratch(nb, "tail")
    _l.check(L.mis_uamt_tail(_l.ptr(student), sbs, _l.ptr(teacher), tbs, _l.ptr(mean_probs), mbs, _l.ptr(label), lb,
                             B, labeled_bs, C, S, cons_weight, _l.ptr(state), int(iter_num), float(max_iterations),
                             loss_scale, _l.ptr(out), _l.ptr(dlogits), dbs, _l.ptr(ws), ws.numel(),
                             _l.stream_ptr()), "mis_uamt_tail")


ICT_BETA_SALT = 0x1C7BE7A0


def beta_sample(lam, alpha, state, salt=ICT_BETA_SALT):
    """lam[m] ~ Beta(alpha, alpha) on the device, keyed by (seed, iter_num) of ``state`` and ``salt`` (ICT mix factors,
    reference np.random.beta(ict_alpha, ict_alpha, size=(L // 2, 1, 1, 1)))."""
    L = _l.load()
    _l.require_gpu(lam, state)
    assert lam.dtype == torch.float32 and lam.is_contiguous() and lam.numel() > 0
    if not float(alpha) > 0.0:
        raise ValueError(f"Beta(alpha, alpha) needs alpha > 0, got {alpha}")
    _l.check(L.mis_beta_sample(_l.ptr(lam), lam.numel(), float(alpha), int(salt) & 0xFFFFFFFF, _l.ptr(state),
                               _l.stream_ptr()), "mis_beta_sample")


def ict_mix(x, lam, labeled_bs, out):
    """out[:L] = x[:L]; out[L + m] = x[L + m] * (1 - lam[m]) + x[L + M + m] * lam[m] with M = lam.numel() and
    x.shape[0] == L + 2M (ICT input of the student, bit-identical to the torch expression)."""
    L = _l.load()
    _l.require_gpu(x, lam, out)
    M = lam.numel()
    assert x.dtype == out.dtype == lam.dtype == torch.float32
    assert x.is_contiguous() and out.is_contiguous() and lam.is_contiguous()
    assert x.shape[0] == labeled_bs + 2 * M and out.shape[0] == labeled_bs + M
    assert tuple(x.shape[1:]) == tuple(out.shape[1:])
    n = x[0].numel()
    _l.check(L.mis_ict_mix(_l.ptr(x), _l.ptr(out), _l.ptr(lam), labeled_bs, M, n, _l.stream_ptr()), "mis_ict_mix")


def ict_tail(student, teacher0, teacher1, lam, label, labeled_bs, out, dlogits=None, cons_weight=0.0, state=None,
             loss_scale=1.0):
    """ICT loss tail: 0.5*(CE+Dice) on student[:L] + w * mean((softmax(student[L:]) - target)^2), target =
    softmax(teacher0) * (1 - lam) + softmax(teacher1) * lam.  ``out`` (>= 5+C floats): the layout of loss_tail."""
    L = _l.load()
    B, C, D, H, W, S, sbs = _geom(student)
    M = B - labeled_bs
    B0, C0, _, _, _, S0, t0bs = _geom(teacher0)
    B1, C1, _, _, _, S1, t1bs = _geom(teacher1)
    assert B0 == B1 == M and C0 == C1 == C and S0 == S1 == S
    _l.require_gpu(lam, label)
    assert lam.dtype == torch.float32 and lam.is_contiguous() and lam.numel() == M
    assert label.is_contiguous() and label.dtype in (torch.uint8, torch.int64) and label.numel() >= labeled_bs * S
    lb = 1 if label.dtype == torch.uint8 else 8
    dbs = _geom(dlogits)[6] if dlogits is not None else 0
    ws = scratch(L.mis_ict_tail_workspace_bytes(B, C, S), "tail")
    _l.check(L.mis_ict_tail(_l.ptr(student), sbs, _l.ptr(teacher0), t0bs, _l.ptr(teacher1), t1bs, _l.ptr(lam),
                            _l.ptr(label), lb, labeled_bs, M, C, S, cons_weight, _l.ptr(state), loss_scale,
                            _l.ptr(out), _l.ptr(dlogits), dbs, _l.ptr(ws), ws.numel(), _l.stream_ptr()),
             "mis_ict_tail")


def _sched_args(sched, k):
    if sched is None:
        if int(k) < 0:
            raise ValueError("rotation k < 0 reads sched[state.iter_num]: a schedule and a step state are needed")
        return None, 0
    _l.require_gpu(sched)
    assert sched.dtype == torch.int32 and sched.is_contiguous() and sched.numel() > 0
    return _l.ptr(sched), sched.numel()


def rot90(x, out, k=-1, sched=None, state=None):
    """out = torch.rot90(x, k, [2, 3]) for x [N, C, H, W] (free batch stride, dense planes: e.g. ``volume[L:]``),
    bit-identical.  ``k`` < 0: read on the device, ``sched[state.iter_num]`` (deep co-training's rotation per iteration)."""
    L = _l.load()
    _l.require_gpu(x, out, state)
    if x.dim() != 4 or out.dim() != 4 or x.dtype != torch.float32 or out.dtype != torch.float32:
        raise RuntimeError(f"rot90 takes fp32 [N,C,H,W] tensors, got {tuple(x.shape)} / {tuple(out.shape)}")
    N, C, H, W = x.shape
    assert x[0].is_contiguous() and out.is_contiguous()
    want = (N, C, W, H) if int(k) >= 0 and int(k) % 2 else (N, C, H, W)
    if tuple(out.shape) != want:
        raise RuntimeError(f"rot90: output {tuple(out.shape)}, expected {want}")
    sp, ns = _sched_args(sched, k)
    in_bs = x.stride(0) if N > 1 else C * H * W
    _l.check(L.mis_rot90(_l.ptr(x), in_bs, _l.ptr(out), C * H * W, N, C, H, W, sp, ns, _l.ptr(state), int(k),
                         _l.stream_ptr()), "mis_rot90")


def dct_tail(logits_a, logits_r, label, labeled_bs, out, dA=None, dR=None, k=-1, sched=None, state=None,
             cons_weight=0.0, loss_scale=1.0):
    """Deep co-training loss tail over pass A (the batch, [L+U,C,1,H,W]) and pass R (the rotated unlabeled part,
    [U,C,1,H,W]).  ``out`` (>= 6+C floats): [loss, loss_ce, loss_dice, consistency_loss, consistency_weight, k,
    class-wise dice...]; ``dA`` / ``dR``: the logits gradients of both passes (both or neither)."""
    L = _l.load()
    B, C, D, H, W, S, abs_ = _geom(logits_a)
    U, Cr, Dr, Hr, Wr, _, rbs = _geom(logits_r)
    assert D == Dr == 1 and Cr == C and (Hr, Wr) == (H, W) and U == B - labeled_bs
    _l.require_gpu(label, state)
    assert label.is_contiguous() and label.dtype in (torch.uint8, torch.int64) and label.numel() >= labeled_bs * S
    lb = 1 if label.dtype == torch.uint8 else 8
    dabs = _geom(dA)[6] if dA is not None else 0
    drbs = _geom(dR)[6] if dR is not None else 0
    sp, ns = _sched_args(sched, k)
    ws = scratch(L.mis_dct_tail_workspace_bytes(labeled_bs, U, C, H, W), "tail")
    _l.check(L.mis_dct_tail(_l.ptr(logits_a), abs_, _l.ptr(logits_r), rbs, _l.ptr(label), lb, labeled_bs, U, C, H, W,
                            sp, ns, _l.ptr(state), int(k), cons_weight, loss_scale, _l.ptr(out), _l.ptr(dA), dabs,
                            _l.ptr(dR), drbs, _l.ptr(ws), ws.numel(), _l.stream_ptr()), "mis_dct_tail")


def grad_combine(dst, src, accumulate):
    """dst = src, or dst += src with ``accumulate`` (flat gradient buffers; a launch, so it lands on a launch tape)."""
    L = _l.load()
    _l.require_gpu(dst, src)
    assert dst.dtype == src.dtype == torch.float32 and dst.is_contiguous() and src.is_contiguous()
    assert dst.numel() == src.numel()
    _l.check(L.mis_grad_combine(_l.ptr(dst), _l.ptr(src), dst.numel(), int(bool(accumulate)), _l.stream_ptr()),
             "mis_grad_combine")


FIXMATCH_JITTER_SALT = 0xF1A7C401
FIXMATCH_OUT = ("loss", "sup_ce", "sup_dice", "unsup", "consistency_weight", "ce_u", "dice_u", "ce_comp", "as_weight",
                "masked_in_fraction")


def color_jitter(x, out, params=None, state=None, drawn=None, salt=FIXMATCH_JITTER_SALT):
    """out = ColorJitter(0.8, 0.8, 0.8, 0.2)(x) for one-channel images x [B, 1, ...] (free batch stride, dense planes):
    brightness and contrast per image, in the order of that image.  ``params`` ([B, 3] fp32: beta, gamma, order; order 0 =
    brightness first) gives the factors; without it they are drawn on the device from ``state`` (seed, iter_num) under
    ``salt``.  ``drawn`` ([B, 3] fp32) receives the factors used."""
    L = _l.load()
    _l.require_gpu(x, out, params, state, drawn)
    if x.dtype != torch.float32 or out.dtype != torch.float32 or x.dim() < 3 or x.shape[1] != 1:
        raise RuntimeError(f"color_jitter takes fp32 [B,1,...] images, got {tuple(x.shape)} {x.dtype}")
    B = x.shape[0]
    assert tuple(out.shape) == tuple(x.shape) and x[0].is_contiguous() and out[0].is_contiguous()
    S = x[0].numel()
    for t in (params, drawn):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == 3 * B)
    if params is None and state is None:
        raise ValueError("color_jitter needs the factors (params) or a step state to draw them from")
    xbs = x.stride(0) if B > 1 else S
    ybs = out.stride(0) if B > 1 else S
    ws = scratch(L.mis_color_jitter_workspace_bytes(B, S), "jitter")
    _l.check(L.mis_color_jitter(_l.ptr(x), xbs, _l.ptr(out), ybs, B, S, _l.ptr(params), _l.ptr(state),
                                int(salt) & 0xFFFFFFFF, _l.ptr(drawn), _l.ptr(ws), ws.numel(), _l.stream_ptr()),
             "mis_color_jitter")


def fixmatch_tail(weak, strong, label, labeled_bs, out, d_weak=None, d_strong=None, conf_thresh=0.8, cons_weight=0.0,
                  state=None, pseudo=None, comp=None):
    """FixMatch loss tail over the logits of one network on the weak and on the strong batch (both [B,C,D,H,W]).
    ``out`` (>= 10 floats): FIXMATCH_OUT.  ``d_weak`` / ``d_strong``: the logits gradients (either may be None).
    ``pseudo`` ([B-L, S] uint8) / ``comp`` ([B, S] uint8) receive the kernel's pseudo and complementary labels."""
    L = _l.load()
    B, C, D, H, W, S, wbs = _geom(weak)
    Bs, Cs, _, _, _, Ss, sbs = _geom(strong)
    assert (Bs, Cs, Ss) == (B, C, S)
    _l.require_gpu(label, state, out, pseudo, comp)
    assert label.is_contiguous() and label.dtype in (torch.uint8, torch.int64) and label.numel() >= labeled_bs * S
    lb = 1 if label.dtype == torch.uint8 else 8
    assert out.dtype == torch.float32 and out.numel() >= len(FIXMATCH_OUT)
    dwbs = _geom(d_weak)[6] if d_weak is not None else 0
    dsbs = _geom(d_strong)[6] if d_strong is not None else 0
    for t, n in ((pseudo, (B - labeled_bs) * S), (comp, B * S)):
        assert t is None or (t.dtype == torch.uint8 and t.is_contiguous() and t.numel() == n)
    ws = scratch(max(L.mis_fixmatch_tail_workspace_bytes(B, C, S), 0), "tail")
    _l.check(L.mis_fixmatch_tail(_l.ptr(weak), wbs, _l.ptr(strong), sbs, _l.ptr(label), lb, B, labeled_bs, C, S,
                                 float(conf_thresh), cons_weight, _l.ptr(state), _l.ptr(out), _l.ptr(d_weak), dwbs,
                                 _l.ptr(d_strong), dsbs, _l.ptr(pseudo), _l.ptr(comp), _l.ptr(ws), ws.numel(),
                                 _l.stream_ptr()), "mis_fixmatch_tail")


def cross_teaching_tail(own, other, label, labeled_bs, out, dlogits=None, cons_weight=0.0, state=None,
                        pseudo_ce=False, teacher=None, mt_weight=0.0):
    """0.5*(CE+Dice) on the labeled half + w * Dice (``pseudo_ce``: cross-entropy, CPS) against the other network's
    arg-max pseudo labels.  ``out`` (>= 5 floats): [loss_m, loss_ce, loss_dice, pseudo_supervision, consistency_weight].
    ``teacher`` (EMA-teacher logits of the unlabeled half): + mt_weight * softmax-MSE consistency, out[5:7] =
    [consistency_loss, mt_weight] (reference code/train_cnn_meet_vit_2D.py:300-337)."""
    L = _l.load()
    B, C, D, H, W, S, sbs = _geom(own)
    Bo, Co, _, _, _, So, obs = _geom(other)
    assert (Bo, Co, So) == (B, C, S)
    if teacher is not None:
        Bt, Ct, _, _, _, St, tbs = _geom(teacher)
        assert (Bt, Ct, St) == (B - labeled_bs, C, S)
        _l.require_gpu(label)
        assert label.is_contiguous() and label.dtype in (torch.uint8, torch.int64) and label.numel() >= labeled_bs * S
        ws = scratch(L.mis_cross_teaching_tail_workspace_bytes(B, C, S), "tail")
        _l.check(L.mis_cross_pseudo_mt_tail(_l.ptr(own), sbs, _l.ptr(other), obs, _l.ptr(teacher), tbs, _l.ptr(label),
                                            1 if label.dtype == torch.uint8 else 8, B, labeled_bs, C, S, cons_weight,
                                            mt_weight, _l.ptr(state), int(bool(pseudo_ce)), _l.ptr(out),
                                            _l.ptr(dlogits), _geom(dlogits)[6] if dlogits is not None else 0,
                                            _l.ptr(ws), ws.numel(), _l.stream_ptr()), "mis_cross_pseudo_mt_tail")
        return
    _l.require_gpu(label)
    assert label.is_contiguous() and label.dtype in (torch.uint8, torch.int64) and label.numel() >= labeled_bs * S
    lb = 1 if label.dtype == torch.uint8 else 8
    dbs = _geom(dlogits)[6] if dlogits is not None else 0
    ws = scratch(L.mis_cross_teaching_tail_workspace_bytes(B, C, S), "tail")
    _l.check(L.mis_cross_pseudo_tail(_l.ptr(own), sbs, _l.ptr(other), obs, _l.ptr(label), lb, B, labeled_bs, C,
                                     S, cons_weight, _l.ptr(state), int(bool(pseudo_ce)), _l.ptr(out),
                                     _l.ptr(dlogits), dbs, _l.ptr(ws), ws.numel(), _l.stream_ptr()),
             "mis_cross_pseudo_tail")


def triple_view_tail(z1, z2, z3, label, labeled_bs, outs, dlogits=None, cons_weight=0.0, state=None):
    """Triple-view loss tail of three students' logits [B,C,D,H,W]: for each, 0.5*(CE+Dice) on the labeled half + w * Dice
    against the arg-max pseudo labels of EACH of the other two on the unlabeled half (reference
    code/train_tripleview_2D(demo).py:290-335).  ``outs``: three buffers of >= 6 floats, [loss_m, loss_ce, loss_dice,
    pseudo_supervision_a, consistency_weight, pseudo_supervision_b]; ``dlogits``: three gradient buffers or None."""
    L = _l.load()
    B, C, D, H, W, S, bs1 = _geom(z1)
    bss = [bs1]
    for z in (z2, z3):
        Bo, Co, _, _, _, So, bs = _geom(z)
        assert (Bo, Co, So) == (B, C, S)
        bss.append(bs)
    assert len(outs) == 3 and all(o.dtype == torch.float32 and o.numel() >= 6 for o in outs)
    _l.require_gpu(label, state, *outs)
    assert label.is_contiguous() and label.dtype in (torch.uint8, torch.int64) and label.numel() >= labeled_bs * S
    lb = 1 if label.dtype == torch.uint8 else 8
    if dlogits is None:
        dlogits, dbs = (None, None, None), (0, 0, 0)
    else:
        assert len(dlogits) == 3
        dg = [_geom(d) for d in dlogits]
        assert all((g[0], g[1], g[5]) == (B, C, S) for g in dg)
        dbs = [g[6] for g in dg]
    ws = scratch(L.mis_triple_view_tail_workspace_bytes(B, C, S), "tail")
    _l.check(L.mis_triple_view_tail(_l.ptr(z1), bss[0], _l.ptr(z2), bss[1], _l.ptr(z3), bss[2], _l.ptr(label), lb, B,
                                    labeled_bs, C, S, cons_weight, _l.ptr(state), _l.ptr(outs[0]), _l.ptr(outs[1]),
                                    _l.ptr(outs[2]), _l.ptr(dlogits[0]), dbs[0], _l.ptr(dlogits[1]), dbs[1],
                                    _l.ptr(dlogits[2]), dbs[2], _l.ptr(ws), ws.numel(), _l.stream_ptr()),
             "mis_triple_view_tail")


PATCH_NCE_DIMS = (16, 32)     # feature dims mis_patch_nce is built for (the reference's projector and classifier heads)


def _geom_features(t):
    """(B, d, N, batch_stride) of a fp32 feature view [B, d, *spatial]: dense in (d, spatial), free batch stride."""
    if t.dim() < 3 or t.dtype != torch.float32:
        raise RuntimeError(f"expected fp32 [B, d, *spatial], got {tuple(t.shape)} {t.dtype}")
    _l.require_gpu(t)
    B, d = t.shape[0], t.shape[1]
    N = 1
    for n in t.shape[2:]:
        N *= n
    if B < 1 or d < 1 or N < 1:
        raise RuntimeError(f"empty feature tensor {tuple(t.shape)}")
    want = 1
    for size, stride in zip(reversed(t.shape[1:]), reversed(t.stride()[1:])):
        if size > 1 and stride != want:
            raise RuntimeError(f"feature view must be dense in (d, spatial); strides {t.stride()} shape {tuple(t.shape)}")
        want *= size
    bs = t.stride(0) if B > 1 else d * N
    if bs < d * N:
        raise RuntimeError(f"batch stride {bs} of a feature view overlaps its samples ({d} x {N})")
    return B, d, N, bs


def patch_nce(feat_q, feat_k, out, dfeat=None, temperature=0.07, grad_scale=1.0):
    """Pixel-wise contrastive loss of ``feat_q`` against the detached ``feat_k`` (both ``[B, d, *spatial]``, d in
    ``PATCH_NCE_DIMS``; reference code/utils/losses.py:283-337): ``out`` (>= 3 floats) = [loss, mean s_ii, mean
    logsumexp_j s_ij]; ``dfeat``: ``grad_scale * d loss / d feat_q`` with respect to the raw features, or None for the
    loss alone.  One flash-style pass: no [B, N, N] tensor, the workspace is linear in B * N * d."""
    L = _l.load()
    B, d, N, qbs = _geom_features(feat_q)
    Bk, dk, Nk, kbs = _geom_features(feat_k)
    assert (Bk, dk, Nk) == (B, d, N), (tuple(feat_q.shape), tuple(feat_k.shape))
    if d not in PATCH_NCE_DIMS:
        raise RuntimeError(f"patch_nce: feature dim {d} is not supported (supported dims: {PATCH_NCE_DIMS})")
    _l.require_gpu(out)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= 3
    dbs = 0
    if dfeat is not None:
        Bd, dd, Nd, dbs = _geom_features(dfeat)
        assert (Bd, dd, Nd) == (B, d, N), (tuple(feat_q.shape), tuple(dfeat.shape))
    nb = L.mis_patch_nce_workspace_bytes(B, d, N)
    if nb < 0:
        _l.check(nb, "mis_patch_nce_workspace_bytes")
    ws = scratch(nb, "patch_nce")
    _l.check(L.mis_patch_nce(_l.ptr(feat_q), qbs, _l.ptr(feat_k), kbs, B, d, N, float(temperature), float(grad_scale),
                             _l.ptr(out), _l.ptr(dfeat), dbs, _l.ptr(ws), ws.numel(), _l.stream_ptr()), "mis_patch_nce")


CONTRASTIVE_OUT = ("weighted_loss", "loss_ce", "loss_dice", "pseudo_supervision", "consistency_weight", "model_loss")


def contrastive_cross_tail(own, other, label, labeled_bs, out, dlogits=None, extra_l=None, extra_u=None, sup_scale=2.0,
                           pseudo_scale=1.25, extra_scale=1.0, cons_weight=0.0, state=None):
    """One student's loss tail of contrastive cross teaching (mis_contrastive_cross_tail): ``out`` (>= 6 floats,
    CONTRASTIVE_OUT) with out[0] = sup_scale * 0.5 * (CE + Dice) + pseudo_scale * w * Dice(own[L:], argmax other[L:]);
    ``dlogits`` = d out[0] / d own + extra_scale * the head gradients ``extra_l`` ([L/2, C, ...]: labeled rows 0, 2, ...)
    and ``extra_u`` ([B-L, C, ...]: the unlabeled rows), each optional, added in the pass that writes dlogits."""
    L = _l.load()
    B, C, D, H, W, S, sbs = _geom(own)
    Bo, Co, _, _, _, So, obs = _geom(other)
    assert (Bo, Co, So) == (B, C, S)
    _l.require_gpu(label, state, out)
    assert label.is_contiguous() and label.dtype in (torch.uint8, torch.int64) and label.numel() >= labeled_bs * S
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= len(CONTRASTIVE_OUT)
    lb = 1 if label.dtype == torch.uint8 else 8
    dbs = elbs = eubs = 0
    if dlogits is not None:
        Bd, Cd, _, _, _, Sd, dbs = _geom(dlogits)
        assert (Bd, Cd, Sd) == (B, C, S)
    if extra_l is not None:
        Be, Ce, _, _, _, Se, elbs = _geom(extra_l)
        assert (2 * Be, Ce, Se) == (labeled_bs, C, S), (tuple(extra_l.shape), labeled_bs)
    if extra_u is not None:
        Be, Ce, _, _, _, Se, eubs = _geom(extra_u)
        assert (Be, Ce, Se) == (B - labeled_bs, C, S), (tuple(extra_u.shape), B - labeled_bs)
    ws = scratch(max(L.mis_contrastive_cross_tail_workspace_bytes(B, C, S), 0), "tail")
    _l.check(L.mis_contrastive_cross_tail(_l.ptr(own), sbs, _l.ptr(other), obs, _l.ptr(label), lb, B, labeled_bs, C, S,
                                          float(sup_scale), float(pseudo_scale), float(cons_weight), _l.ptr(state),
                                          _l.ptr(extra_l), elbs, _l.ptr(extra_u), eubs, float(extra_scale), _l.ptr(out),
                                          _l.ptr(dlogits), dbs, _l.ptr(ws), ws.numel(), _l.stream_ptr()),
             "mis_contrastive_cross_tail")


def contrastive_step_init(state, seed, iter_num, base_lr, max_iterations, consistency, rampup, iters_per_epoch):
    L = _l.load()
    _l.check(L.mis_contrastive_step_init(_l.ptr(state), seed, iter_num, base_lr, float(max_iterations), consistency,
                                         float(rampup), int(iters_per_epoch), _l.stream_ptr()),
             "mis_contrastive_step_init")


def contrastive_step_advance(state, base_lr, max_iterations, consistency, rampup, iters_per_epoch):
    L = _l.load()
    _l.check(L.mis_contrastive_step_advance(_l.ptr(state), base_lr, float(max_iterations), consistency, float(rampup),
                                            int(iters_per_epoch), _l.stream_ptr()), "mis_contrastive_step_advance")


def contrastive_schedule(k, base_lr, max_iterations, consistency, rampup, iters_per_epoch):
    """Host restatement of the device schedule: (lr, consistency weight) of the step that runs at iteration ``k``
    (reference code/train_Contrastive_Cross_CNN_2D.py:107-110, :274-278; the lr of step k was computed after step k - 1
    from iter_num = k - 1, before the increment)."""
    import math
    lr = float(base_lr)
    if k >= 1:
        it = k - 1
        if it / max_iterations > 0.5:
            lr = 0.0001 * max(1.0 - (it - max_iterations * 0.5) / max_iterations * 0.5, 0.0) ** 0.9
        else:
            lr = base_lr * max(1.0 - it / max_iterations, 0.0) ** 0.9
    epoch = k // iters_per_epoch
    ramp = 1.0
    if epoch < rampup:
        p = 1.0 - max(0.0, float(epoch)) / float(rampup)
        ramp = math.exp(-p * p * 5.0)
    return lr, consistency * ramp


# ------------------------------------------------------------ optimizer / rng
def sgd_ema_step(param, grad, momentum_buf, ema_param, lr=0.0, momentum=0.9, weight_decay=1e-4, ema_alpha=0.99,
                 grad_scale=1.0, state=None):
    L = _l.load()
    _l.require_gpu(param, grad, momentum_buf, ema_param)
    n = param.numel()
    assert grad.numel() == n and momentum_buf.numel() == n and (ema_param is None or ema_param.numel() == n)
    _l.check(L.mis_sgd_ema_step(_l.ptr(param), _l.ptr(grad), _l.ptr(momentum_buf), _l.ptr(ema_param), n, lr,
                                momentum, weight_decay, ema_alpha, grad_scale, _l.ptr(state), _l.stream_ptr()),
             "mis_sgd_ema_step")


def teacher_noise(x, y, state, sigma=0.1, clamp_abs=0.2, salt=0x7EAC4E5):
    L = _l.load()
    _l.require_gpu(x, y, state)
    assert x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel()
    _l.check(L.mis_teacher_noise(_l.ptr(x), _l.ptr(y), x.numel(), sigma, clamp_abs, salt, _l.ptr(state),
                                 _l.stream_ptr()), "mis_teacher_noise")


def new_step_state():
    return torch.zeros(_l.STEP_STATE_BYTES, dtype=torch.uint8, device="cuda")


def step_init(state, seed, iter_num, base_lr, max_iterations, ema_decay, consistency, rampup, ramp_div=150,
              cons_start_iter=0, lr_post_increment=False):
    L = _l.load()
    _l.check(L.mis_step_init(_l.ptr(state), seed, iter_num, base_lr, float(max_iterations), ema_decay, consistency,
                             rampup, ramp_div, cons_start_iter, int(lr_post_increment), _l.stream_ptr()),
             "mis_step_init")


def step_advance(state, base_lr, max_iterations, ema_decay, consistency, rampup, ramp_div=150, cons_start_iter=0,
                 lr_post_increment=False):
    L = _l.load()
    _l.check(L.mis_step_advance(_l.ptr(state), base_lr, float(max_iterations), ema_decay, consistency, rampup,
                                ramp_div, cons_start_iter, int(lr_post_increment), _l.stream_ptr()),
             "mis_step_advance")


def read_step_state(state):
    """Host copy of the device step state (one small D2H; not used inside the hot loop)."""
    import struct
    raw = bytes(state.cpu().numpy().tobytes())
    seed, offset, it, lr, alpha, w, gate = struct.unpack("<QQqffff", raw[:40])
    return dict(seed=seed, offset=offset, iter_num=it, lr=lr, ema_alpha=alpha, cons_weight=w, cons_gate=gate)


def argmax_channels(x, out):
    L = _l.load()
    B, C, D, H, W, S, xbs = _geom(x)
    assert out.dtype == torch.uint8 and out.numel() == B * S
    _l.check(L.mis_argmax_channels(_l.ptr(x), xbs, _l.ptr(out), B, C, S, _l.stream_ptr()), "mis_argmax_channels")


# ---------------------------------------------------------------- validation metrics
def _label_geom(*maps):
    """(ndim, D, H, W) of uint8 label maps of one shape, [D, H, W] or [H, W]; the wrapper refuses anything it would have to copy."""
    _l.require_gpu(*maps)
    first = maps[0]
    for t in maps:
        if t.dtype != torch.uint8:
            raise RuntimeError(f"label maps must be uint8, got {t.dtype}")
        if not t.is_contiguous():
            raise RuntimeError("label maps must be contiguous")
        if t.shape != first.shape:
            raise RuntimeError(f"label maps differ in shape: {tuple(first.shape)} vs {tuple(t.shape)}")
    if first.dim() not in (2, 3) or first.numel() == 0:
        raise RuntimeError(f"expected a non-empty [D,H,W] or [H,W] label map, got {tuple(first.shape)}")
    D, H, W = (1,) * (3 - first.dim()) + tuple(first.shape)
    return first.dim(), D, H, W


def _surface_workspace(L, D, H, W):
    nbytes = L.mis_surface_metrics_workspace_bytes(D, H, W)
    if nbytes < 0:
        _l.check(nbytes, "mis_surface_metrics_workspace_bytes")
    return scratch(nbytes, "surface_metrics"), nbytes


def surface_metrics(pred_u8, gt_u8, cls):
    """The result record of ``mis_surface_metrics`` (int64 [12] on the device; fields in include/mis_hip.h) for the masks
    ``pred == cls`` / ``gt == cls`` (``cls = -1``: label > 0).  Nothing is synchronised: the caller reads the record when it wants
    it (utils.metrics.device_scores)."""
    L = _l.load()
    ndim, D, H, W = _label_geom(pred_u8, gt_u8)
    ws, nbytes = _surface_workspace(L, D, H, W)
    out = torch.empty(_l.SURFACE_RECORD_WORDS, dtype=torch.int64, device=pred_u8.device)
    _l.check(L.mis_surface_metrics(_l.ptr(pred_u8), _l.ptr(gt_u8), int(cls), ndim, D, H, W, _l.ptr(out), _l.ptr(ws), nbytes,
                                   _l.stream_ptr()), "mis_surface_metrics")
    return out


def sq_edt(seeds_u8):
    """Exact squared Euclidean distance (int32) of every voxel to the nearest non-zero voxel of ``seeds_u8``."""
    L = _l.load()
    ndim, D, H, W = _label_geom(seeds_u8)
    ws, nbytes = _surface_workspace(L, D, H, W)
    out = torch.empty(seeds_u8.shape, dtype=torch.int32, device=seeds_u8.device)
    _l.check(L.mis_sq_edt(_l.ptr(seeds_u8), ndim, D, H, W, _l.ptr(out), _l.ptr(ws), nbytes, _l.stream_ptr()), "mis_sq_edt")
    return out


# ------------------------------------------------- grid attention gates, integer up-sampling (csrc/attention_gate.hip)
def _gate_geom(x, att, wide):
    """(N, G, C, D, H, W, d, h, w, x_bs, att_bs, wide_bs): ``x`` [N,C,D,H,W], ``att`` [N,G,d,h,w], ``wide`` [N,G*C,D,H,W]."""
    N, C, D, H, W, _, xbs = _geom(x)
    Na, G, d, h, w, _, abs_ = _geom(att)
    Nw, GC, Dw, Hw, Ww, _, wbs = _geom(wide)
    if Na != N or Nw != N or GC != G * C or (Dw, Hw, Ww) != (D, H, W):
        raise RuntimeError(f"attention gate: x {tuple(x.shape)}, att {tuple(att.shape)} and the gated tensor "
                           f"{tuple(wide.shape)} do not belong together (MIS_ERR_ARG)")
    return N, G, C, D, H, W, d, h, w, xbs, abs_, wbs


def attn_gate_map_fwd(theta, phi, psi_w, psi_b, att):
    """att[N,G,d,h,w] = sigmoid(psi_b[g] + sum_i psi_w[g,i] relu(theta + phi)[N, g Ci + i]); psi_w [G,Ci], psi_b [G] contiguous."""
    L = _l.load()
    N, GCi, d, h, w, _, tbs = _geom(theta)
    Np, GCp, dp, hp, wp_, _, pbs = _geom(phi)
    Na, G, da, ha, wa, _, abs_ = _geom(att)
    if (Np, GCp, dp, hp, wp_) != (N, GCi, d, h, w) or (Na, da, ha, wa) != (N, d, h, w) or GCi % G or psi_b.numel() != G \
            or psi_w.numel() != GCi or not psi_w.is_contiguous() or not psi_b.is_contiguous():
        raise RuntimeError(f"attention gate map: theta {tuple(theta.shape)}, phi {tuple(phi.shape)}, att {tuple(att.shape)}, "
                           f"psi {tuple(psi_w.shape)} / {tuple(psi_b.shape)} do not belong together (MIS_ERR_ARG)")
    _l.check(L.mis_attn_gate_map_fwd(_l.ptr(theta), tbs, _l.ptr(phi), pbs, _l.ptr(psi_w), _l.ptr(psi_b), _l.ptr(att), abs_, N, G,
                                     GCi // G, d, h, w, _l.stream_ptr()), "mis_attn_gate_map_fwd")


def attn_gate_map_bwd(datt, att, theta, phi, psi_w, df, dpsi_w, dpsi_b, dphi_b=None, accumulate=False):
    """df[N,G*Ci,d,h,w] = psi_w dpre [theta + phi > 0] with dpre = datt att (1 - att); dpsi_w (+)= sum relu(theta + phi) dpre,
    dpsi_b (+)= sum dpre, dphi_b[G*Ci] (+)= sum df (the phi convolution's bias gradient; None: not wanted).  Deterministic."""
    L = _l.load()
    N, GCi, d, h, w, _, tbs = _geom(theta)
    pbs, fbs = _geom(phi)[6], _geom(df)[6]
    Na, G, da, ha, wa, _, abs_ = _geom(att)
    dbs = _geom(datt)[6]
    if (tuple(phi.shape) != tuple(theta.shape) or tuple(df.shape) != tuple(theta.shape) or tuple(datt.shape) != tuple(att.shape)
            or (Na, da, ha, wa) != (N, d, h, w) or GCi % G or psi_w.numel() != GCi or dpsi_w.numel() != GCi
            or dpsi_b.numel() != G or not (psi_w.is_contiguous() and dpsi_w.is_contiguous() and dpsi_b.is_contiguous())
            or (dphi_b is not None and (dphi_b.numel() != GCi or not dphi_b.is_contiguous()))):
        raise RuntimeError(f"attention gate map backward: theta {tuple(theta.shape)}, att {tuple(att.shape)}, datt "
                           f"{tuple(datt.shape)}, df {tuple(df.shape)} do not belong together (MIS_ERR_ARG)")
    nb = L.mis_attn_gate_map_bwd_workspace_bytes(N, G, GCi // G, d, h, w)
    if nb < 0:
        _l.check(nb, "mis_attn_gate_map_bwd_workspace_bytes")
    ws = scratch(nb, "attn_gate")
    _l.check(L.mis_attn_gate_map_bwd(_l.ptr(datt), dbs, _l.ptr(att), abs_, _l.ptr(theta), tbs, _l.ptr(phi), pbs, _l.ptr(psi_w),
                                     _l.ptr(df), fbs, _l.ptr(dpsi_w), _l.ptr(dpsi_b), _l.ptr(dphi_b), _l.ptr(ws), ws.numel(), N, G,
                                     GCi // G, d, h, w, int(accumulate), _l.stream_ptr()), "mis_attn_gate_map_bwd")


def attn_gate_apply_fwd(x, att, y):
    """y[N, g C + c] = up2(att[N, g]) * x[N, c]: trilinear x2 (align_corners=False) of the attention maps, x read once."""
    L = _l.load()
    N, G, C, D, H, W, d, h, w, xbs, abs_, ybs = _gate_geom(x, att, y)
    _l.check(L.mis_attn_gate_apply_fwd(_l.ptr(x), xbs, _l.ptr(att), abs_, _l.ptr(y), ybs, N, G, C, D, H, W, d, h, w,
                                       _l.stream_ptr()), "mis_attn_gate_apply_fwd")


def attn_gate_apply_bwd(dy, x, att, dx, datt, accumulate=False):
    """dx (+)= sum_g up2(att_g) dy_g;  datt = up2^T(sum_c dy x).  dy and x are read once."""
    L = _l.load()
    N, G, C, D, H, W, d, h, w, xbs, abs_, dybs = _gate_geom(x, att, dy)
    if tuple(dx.shape) != tuple(x.shape) or tuple(datt.shape) != tuple(att.shape):
        raise RuntimeError(f"attention gate backward: dx {tuple(dx.shape)} / datt {tuple(datt.shape)} do not match x "
                           f"{tuple(x.shape)} / att {tuple(att.shape)} (MIS_ERR_ARG)")
    dxbs, dabs = _geom(dx)[6], _geom(datt)[6]
    nb = L.mis_attn_gate_apply_bwd_workspace_bytes(N, G, D, H, W)
    if nb < 0:
        _l.check(nb, "mis_attn_gate_apply_bwd_workspace_bytes")
    ws = scratch(nb, "attn_gate")
    _l.check(L.mis_attn_gate_apply_bwd(_l.ptr(dy), dybs, _l.ptr(x), xbs, _l.ptr(att), abs_, _l.ptr(dx), dxbs, _l.ptr(datt), dabs,
                                       _l.ptr(ws), ws.numel(), N, G, C, D, H, W, d, h, w, int(accumulate), _l.stream_ptr()),
             "mis_attn_gate_apply_bwd")


def _up_int_geom(coarse, fine, scale):
    N, K, d, h, w, _, cbs = _geom(coarse)
    Nf, Kf, D, H, W, _, fbs = _geom(fine)
    if (Nf, Kf) != (N, K) or (D, H, W) != (scale * d, scale * h, scale * w):
        raise RuntimeError(f"upsample x{scale}: {tuple(coarse.shape)} and {tuple(fine.shape)} do not belong together "
                           "(MIS_ERR_ARG)")
    return N, K, d, h, w, cbs, fbs


def upsample_int_fwd(x, y, scale):
    """y = trilinear up-sampling of x by ``scale`` in {2, 4, 8} per axis, align_corners=False."""
    L = _l.load()
    N, K, d, h, w, xbs, ybs = _up_int_geom(x, y, int(scale))
    _l.check(L.mis_upsample_int_fwd(_l.ptr(x), xbs, _l.ptr(y), ybs, N, K, d, h, w, int(scale), _l.stream_ptr()),
             "mis_upsample_int_fwd")


def upsample_int_bwd(dy, dx, scale, accumulate=False):
    """dx (+)= the adjoint of upsample_int_fwd applied to dy (gather form: deterministic)."""
    L = _l.load()
    N, K, d, h, w, dxbs, dybs = _up_int_geom(dx, dy, int(scale))
    _l.check(L.mis_upsample_int_bwd(_l.ptr(dy), dybs, _l.ptr(dx), dxbs, N, K, d, h, w, int(scale), int(accumulate),
                                    _l.stream_ptr()), "mis_upsample_int_bwd")


# ------------------------------------------------------- adversarial training (csrc/adversarial.hip)
ADAM_STATE_BYTES = 16      # int64 step, float 1 - beta1^step, float 1 - beta2^step


def channel_dropout_scale(scale, p, salt, state):
    """scale[N, C] = nn.Dropout3d(p)'s factor per (sample, channel): 0 or 1 / (1 - p), drawn from ``state``."""
    L = _l.load()
    _l.require_gpu(scale)
    assert scale.dim() == 2 and scale.is_contiguous() and scale.dtype == torch.float32
    _l.check(L.mis_channel_dropout_scale(_l.ptr(scale), scale.shape[0], scale.shape[1], float(p), int(salt), _l.ptr(state),
                                         _l.stream_ptr()), "mis_channel_dropout_scale")


def _k4s2_in(x, logits):
    """Geometry of the two-part input of a kernel-4 / stride-2 convolution: (N, D, H, W, x_bs, Cx, l_bs, Cl)."""
    N = D = H = W = None
    xbs = lbs = Cx = Cl = 0
    if logits is not None:
        N, Cl, D, H, W, _, lbs = _geom(logits)
    if x is not None:
        Nx, Cx, Dx, Hx, Wx, _, xbs = _geom(x)
        if N is not None and (Nx, Dx, Hx, Wx) != (N, D, H, W):
            raise RuntimeError(f"conv_k4s2: {tuple(x.shape)} and {tuple(logits.shape)} do not belong together (MIS_ERR_ARG)")
        N, D, H, W = Nx, Dx, Hx, Wx
    if N is None:
        raise RuntimeError("conv_k4s2: no input (MIS_ERR_ARG)")
    return N, D, H, W, xbs, Cx, lbs, Cl


def _k4s2_out(t, N, D, H, W, what):
    No, Co, Do, Ho, Wo, _, bs = _geom(t)
    if (No, 2 * Do, 2 * Ho, 2 * Wo) != (N, D, H, W):
        raise RuntimeError(f"conv_k4s2: {what} {tuple(t.shape)} does not belong to an input of {(N, D, H, W)} (MIS_ERR_ARG)")
    return Co, bs


def conv_k4s2_fwd(x, logits, w_x, w_l, bias, bias2, y, slope=0.2, drop_scale=None):
    """y = drop(leaky_relu(bias + bias2 + Conv3d(k=4, s=2, p=1)(cat(softmax(logits), x)), slope)).  ``logits`` / ``w_l``: the
    channels read through a softmax and their filter (None: none); ``x`` / ``w_x``: the plain ones (None: none)."""
    L = _l.load()
    N, D, H, W, xbs, Cx, lbs, Cl = _k4s2_in(x, logits)
    Cout, ybs = _k4s2_out(y, N, D, H, W, "y")
    assert (w_x is None or (w_x.is_contiguous() and w_x.numel() == Cout * Cx * 64))
    assert (w_l is None or (w_l.is_contiguous() and w_l.numel() == Cout * Cl * 64))
    nb = L.mis_conv_k4s2_fwd_workspace_bytes(N, Cx + Cl, Cout, D, H, W)
    if nb < 0:
        _l.check(nb, "mis_conv_k4s2_fwd_workspace_bytes")
    ws = scratch(nb, "k4s2")
    _l.check(L.mis_conv_k4s2_fwd(_l.ptr(x), xbs, Cx, _l.ptr(logits), lbs, Cl, _l.ptr(w_x), _l.ptr(w_l), _l.ptr(bias),
                                 _l.ptr(bias2), _l.ptr(y), ybs, N, Cout, D, H, W, float(slope), _l.ptr(drop_scale),
                                 _l.ptr(ws), ws.numel(), _l.stream_ptr()), "mis_conv_k4s2_fwd")


def conv_k4s2_dgrad(dy, y, w, dx, slope=0.2, drop_scale=None):
    """dx = the gradient at the input of the convolution with filter ``w`` [Cout, Cin, 4, 4, 4] for the gradient ``dy`` at its
    activated output ``y`` (None: the plain convolution's gradient)."""
    L = _l.load()
    N, Cin, D, H, W, _, dxbs = _geom(dx)
    Cout, dybs = _k4s2_out(dy, N, D, H, W, "dy")
    ybs = _k4s2_out(y, N, D, H, W, "y")[1] if y is not None else 0
    assert w.is_contiguous() and w.numel() == Cout * Cin * 64
    _l.check(L.mis_conv_k4s2_dgrad(_l.ptr(dy), dybs, _l.ptr(y), ybs, float(slope), _l.ptr(drop_scale), _l.ptr(w), _l.ptr(dx),
                                   dxbs, N, Cin, Cout, D, H, W, _l.stream_ptr()), "mis_conv_k4s2_dgrad")


def conv_k4s2_wgrad(x, logits, dy, y, dw_x, dw_l, dbias=None, dbias2=None, slope=0.2, drop_scale=None, accumulate=False):
    """dw_l / dw_x (+)= the filter gradient in the two parts of conv_k4s2_fwd's input, dbias / dbias2 (+)= the bias gradient;
    deterministic."""
    L = _l.load()
    N, D, H, W, xbs, Cx, lbs, Cl = _k4s2_in(x, logits)
    Cout, dybs = _k4s2_out(dy, N, D, H, W, "dy")
    ybs = _k4s2_out(y, N, D, H, W, "y")[1] if y is not None else 0
    assert (dw_x is None or (dw_x.is_contiguous() and dw_x.numel() == Cout * Cx * 64))
    assert (dw_l is None or (dw_l.is_contiguous() and dw_l.numel() == Cout * Cl * 64))
    nb = L.mis_conv_k4s2_wgrad_workspace_bytes(N, Cx + Cl, Cout, D, H, W)
    if nb < 0:
        _l.check(nb, "mis_conv_k4s2_wgrad_workspace_bytes")
    ws = scratch(nb, "k4s2")
    _l.check(L.mis_conv_k4s2_wgrad(_l.ptr(x), xbs, Cx, _l.ptr(logits), lbs, Cl, _l.ptr(dy), dybs, _l.ptr(y), ybs, float(slope),
                                   _l.ptr(drop_scale), _l.ptr(dw_x), _l.ptr(dw_l), _l.ptr(dbias), _l.ptr(dbias2), N, Cout,
                                   D, H, W, int(accumulate), _l.ptr(ws), ws.numel(), _l.stream_ptr()), "mis_conv_k4s2_wgrad")


def adv_head_workspace(N, C, K):
    """The buffer adv_head_fwd leaves the pooled features and d loss / d logits in for adv_head_bwd."""
    L = _l.load()
    nb = L.mis_adv_head_workspace_bytes(N, C, K)
    if nb < 0:
        _l.check(nb, "mis_adv_head_workspace_bytes")
    return torch.empty(nb // 4, dtype=torch.float32, device="cuda")


def adv_head_fwd(a, w, b, target, loss, logits, ws, pool=None):
    """loss[0] = cross_entropy(Linear(avg_pool(a)), target), logits [N, K]; ``pool`` defaults to the feature's extent."""
    L = _l.load()
    N, C, D, H, W, _, abs_ = _geom(a)
    K = w.shape[0]
    pool = (D, H, W) if pool is None else tuple(int(p) for p in pool)
    assert w.is_contiguous() and w.numel() == K * C and target.dtype == torch.int32 and target.numel() == N
    assert logits.is_contiguous() and logits.numel() == N * K
    _l.require_gpu(w, target, loss, logits, ws)
    _l.check(L.mis_adv_head_fwd(_l.ptr(a), abs_, _l.ptr(w), _l.ptr(b), _l.ptr(target), _l.ptr(loss), _l.ptr(logits), N, C, K,
                                D, H, W, pool[0], pool[1], pool[2], _l.ptr(ws), ws.numel() * 4, _l.stream_ptr()),
             "mis_adv_head_fwd")


def adv_head_bwd(w, da, dw, db, ws, shape=None, accumulate=False):
    """da (None: not wanted; then ``shape`` = the feature's (N, C, D, H, W)), dw [K, C], db [K] (+)= the head's gradients."""
    L = _l.load()
    if da is not None:
        N, C, D, H, W, _, dabs = _geom(da)
    else:
        N, C, D, H, W = shape
        dabs = 0
    K = w.shape[0]
    _l.check(L.mis_adv_head_bwd(_l.ptr(w), _l.ptr(da), dabs, _l.ptr(dw), _l.ptr(db), int(accumulate), N, C, K, D, H, W,
                                _l.ptr(ws), ws.numel() * 4, _l.stream_ptr()), "mis_adv_head_bwd")


def adversarial_tail(logits, label, labeled_bs, dmap, cons_loss, out, dlogits=None, cons_weight=0.0, state=None,
                     loss_scale=1.0):
    """0.5 * (CE + Dice) on the labeled samples + w * cons_loss; dlogits: the supervised gradient on the labeled samples,
    w * (softmax Jacobian)^T dmap on the unlabeled ones.  ``out`` (>= 5 + C floats): [loss, loss_ce, loss_dice,
    consistency_loss, consistency_weight, class-wise dice...]."""
    L = _l.load()
    B, C, D, H, W, S, sbs = _geom(logits)
    mbs = 0
    if dmap is not None:
        Bm, Cm, _, _, _, Sm, mbs = _geom(dmap)
        assert Bm == B - labeled_bs and Cm == C and Sm == S
    if label is not None:
        _l.require_gpu(label)
        assert label.is_contiguous() and label.dtype in (torch.uint8, torch.int64)
        assert label.numel() >= labeled_bs * S
    lb = 1 if (label is None or label.dtype == torch.uint8) else 8
    dbs = _geom(dlogits)[6] if dlogits is not None else 0
    nb = L.mis_adversarial_tail_workspace_bytes(B, C, S)
    if nb < 0:
        _l.check(nb, "mis_adversarial_tail_workspace_bytes")
    ws = scratch(nb, "tail")
    _l.check(L.mis_adversarial_tail(_l.ptr(logits), sbs, _l.ptr(label), lb, _l.ptr(dmap), mbs, _l.ptr(cons_loss), B,
                                    labeled_bs, C, S, cons_weight, _l.ptr(state), loss_scale, _l.ptr(out), _l.ptr(dlogits),
                                    dbs, _l.ptr(ws), ws.numel(), _l.stream_ptr()), "mis_adversarial_tail")


def adam_init(adam_state, step=0):
    """Set the device-resident step count of an Adam state (a 16-byte buffer)."""
    L = _l.load()
    _l.require_gpu(adam_state)
    assert adam_state.numel() * adam_state.element_size() >= ADAM_STATE_BYTES
    _l.check(L.mis_adam_init(_l.ptr(adam_state), int(step), _l.stream_ptr()), "mis_adam_init")


def adam_step(param, grad, m, v, adam_state, lr, betas=(0.9, 0.999), eps=1e-8):
    """One torch.optim.Adam step (no weight decay) on flat fp32 buffers; the step count advances on the device."""
    L = _l.load()
    _l.require_gpu(param, grad, m, v, adam_state)
    n = param.numel()
    assert grad.numel() == n and m.numel() == n and v.numel() == n
    _l.check(L.mis_adam_step(_l.ptr(param), _l.ptr(grad), _l.ptr(m), _l.ptr(v), n, float(lr), float(betas[0]),
                             float(betas[1]), float(eps), _l.ptr(adam_state), _l.stream_ptr()), "mis_adam_step")
