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
    if not t.is_cuda:
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


def _view(t):
    """The (pointer, batch stride) operand of an activation view that may be absent: (NULL, 0)."""
    return (t, _geom(t)[6]) if t is not None else (None, 0)


def _label(label, n, optional=False):
    """The (pointer, bytes per label) operand of a label map: uint8 or int64, contiguous, at least ``n`` labels."""
    if label is None and optional:
        return None, 1
    _l.require_gpu(label)
    assert label.is_contiguous() and label.dtype in (torch.uint8, torch.int64) and label.numel() >= n
    return label, 1 if label.dtype == torch.uint8 else 8


def _ws(key, query, *args, optional=False, exact=False):
    """The (pointer, byte count) operand of a kernel workspace: the scratch buffer ``key`` of this stream, grown to what the
    ``*_workspace_bytes`` entry point ``query`` asks for these arguments (an error code raises).  The count is the buffer's
    (never below 1 MiB), with ``exact`` the queried one; with ``optional`` a size of 0 gives (NULL, 0), for entry points to
    which a workspace means "the contraction is split"."""
    nb = _l.query(query, *args)
    if optional and nb == 0:
        return None, 0
    buf = scratch(nb, key)
    return buf, nb if exact else buf.numel()


# When set to a list, the convolution and GEMM wrappers bracket every launch with HIP events on the launch stream and append
# (kernel name, algorithmic FLOPs, start event, end event, algorithmic bytes = operands read once + result written once):
# bench.py's live roofline measurement.
PROFILE = None


def _prof_begin():
    """Opens a row of the roofline list (None: not measuring)."""
    prof = PROFILE
    if prof is None:
        return None
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    e0.record()
    return prof, e0, e1


def _prof_end(row, name, flops, nbytes):
    """Closes it after the launch: ``name`` is a thunk (a ``kernel_name`` query), so nothing is asked when nothing is measured."""
    if row is not None:
        prof, e0, e1 = row
        e1.record()
        prof.append((name(), flops, e0, e1, nbytes))


class JobTable:
    """Many small jobs of one kind in one launch: the device table of job records is built once (it holds raw pointers into the
    jobs' tensors, which ``keep`` keeps alive), ``run()`` launches it.  A subclass names the three entry points and fills one
    record: ``fill(slot, job, first)`` returns the work units of the job, ``first`` being the units of the jobs before it."""
    JOB_BYTES = BATCH = None

    def __init__(self, jobs):
        nb = _l.query(self.JOB_BYTES)
        host = (_ctypes.c_char * (nb * len(jobs)))()
        first = 0
        for i, job in enumerate(jobs):
            first += self.fill(_ctypes.byref(host, i * nb), job, first)
        self.n, self.units, self.keep = len(jobs), first, list(jobs)
        self.table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()

    def run(self):
        _l.launch(self.BATCH, self.table, self.n, self.units)


# ---------------------------------------------------------------- convolution
def conv_pack(weight, mode, out=None):
    """Repack ``weight [Cout,Cin,*k]`` for conv_fwd (mode 0) or the data gradient (mode 1)."""
    Cout, Cin = weight.shape[0], weight.shape[1]
    taps = weight[0, 0].numel()
    n = _l.query("mis_conv_packed_floats", Cout, Cin, taps, mode)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=weight.device)
    assert out.numel() >= n and weight.is_contiguous()
    _l.launch("mis_conv_pack_weights", weight, out, Cout, Cin, taps, mode)
    return out


class PackBatch(JobTable):
    """All weight re-layouts of a network in one launch (``mis_conv_pack_batch``).  ``jobs``: list of
    (weight tensor [Cout,Cin,*k], packed buffer, mode); the device job table is built once."""
    JOB_BYTES, BATCH = "mis_conv_pack_job_bytes", "mis_conv_pack_batch"

    def fill(self, slot, job, first):
        w, wp, mode = job
        assert w.is_contiguous() and wp.is_contiguous()
        n = _l.query("mis_conv_pack_job", slot, w, wp, w.shape[0], w.shape[1], w[0, 0].numel(), mode, first)
        assert wp.numel() >= n
        return n


def conv_pack_raw(w, Cout, Cin, taps, mode, out=None):
    """Pack a weight buffer with explicit geometry (modes 2/3: 1x1 weight stored input-major [Cin][Cout])."""
    n = _l.query("mis_conv_packed_floats", Cout, Cin, taps, mode)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=w.device)
    assert out.numel() >= n and w.is_contiguous() and w.numel() == Cout * Cin * taps
    _l.launch("mis_conv_pack_weights", w, out, Cout, Cin, taps, mode)
    return out


def space_to_depth2(src, dst, fine_shape, to_depth, bias=None, accumulate=False):
    """fine [N,C,D,H,W] <-> coarse [N,8C,D/2,H/2,W/2]; ``fine_shape`` = (N,C,D,H,W) of the fine tensor."""
    N, C, D, H, W = fine_shape
    _l.launch("mis_space_to_depth2", _view(src), _view(dst), bias, N, C, D, H, W, int(to_depth), int(accumulate))


def space_to_depth2d(src, dst, fine_shape, to_depth, bias=None, accumulate=False):
    """2-D: fine [N,C,1,H,W] <-> coarse [N,4C,1,H/2,W/2]; ``fine_shape`` = (N,C,1,H,W) of the fine tensor."""
    N, C, D, H, W = fine_shape
    assert D == 1
    _l.launch("mis_space_to_depth2d", _view(src), _view(dst), bias, N, C, H, W, int(to_depth), int(accumulate))


def conv_k2s2_eligible(cin, cout, coarse, up):
    """(cin, cout) and the COARSE (Do, Ho, Wo) the in-place kernel-2 / stride-2 kernels serve (conv_k2s2.hip)."""
    return bool(_l.query("mis_conv_k2s2_eligible", int(cin), int(cout), *[int(v) for v in coarse], int(up)))


def conv_k2s2_wgrad_eligible(cf, cc, coarse):
    return bool(_l.query("mis_conv_k2s2_wgrad_eligible", int(cf), int(cc), *[int(v) for v in coarse]))


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
    N, CC, Do, Ho, Wo, _, cbs = _geom(coarse)
    _, CF, _, _, _, _, fbs = _geom(fine)
    assert dw.is_contiguous() and dw.numel() == CC * CF * 8
    ws = _ws("wgrad", "mis_conv_k2s2_wgrad_workspace_bytes", CF, CC)
    _tag(f"k2s2_wgrad:{CF}x{CC}@{Do}")
    _l.launch("mis_conv_k2s2_wgrad", coarse, cbs, fine, fbs, dw, N, CF, CC, Do, Ho, Wo, int(accumulate), ws)


def conv_k2s2_down(x, w, bias, y, accumulate=False):
    """y (coarse) (+)= bias + sum w[co][ci*8 + tap] x[ci][2v + tap]: Conv3d(k2s2) forward / ConvTranspose3d(k2s2) dX."""
    N, Cin, _, _, _, _, xbs = _geom(x)
    _, Cout, Do, Ho, Wo, _, ybs = _geom(y)
    assert w.is_contiguous() and w.numel() == Cin * Cout * 8
    _tag(f"k2s2_down:{Cin}x{Cout}@{Do}")
    _l.launch("mis_conv_k2s2_down", x, xbs, w, bias, y, ybs, N, Cin, Cout, Do, Ho, Wo, int(accumulate))


def conv_k2s2_up(x, w, bias, y, accumulate=False):
    """y (fine) (+)= bias + sum w[ci][co*8 + tap] x[ci][v]: ConvTranspose3d(k2s2) forward / Conv3d(k2s2) dX."""
    N, Cin, Do, Ho, Wo, _, xbs = _geom(x)
    _, Cout, _, _, _, _, ybs = _geom(y)
    assert w.is_contiguous() and w.numel() == Cin * Cout * 8
    _tag(f"k2s2_up:{Cin}x{Cout}@{Do}")
    _l.launch("mis_conv_k2s2_up", x, xbs, w, bias, y, ybs, N, Cin, Cout, Do, Ho, Wo, int(accumulate))


def add(a, b, out):
    """out = a (+ b if b is not None) on [N,C,D,H,W] views."""
    N, C, D, H, W, S, abs_ = _geom(a)
    _l.launch("mis_add", a, abs_, _view(b), _view(out), N, C, S)


def _ksize(k):
    if len(k) == 2:
        return 1, k[0], k[1]
    return tuple(k)


WINO = int(_os.environ.get("MIS_WINO", "3"))      # bit 0: Winograd form of the 3x3x3 convolutions, bit 1: of the 3x3 ones
# diagnostics (numerics studies, tests/test_parity_gpu.py): the 3-D forward / data gradient resp. weight gradient alone on the
# direct kernels, and the smallest volume edge W the 3-D Winograd kernels are used for
WINO_FWD = _os.environ.get("MIS_WINO_FWD", "1") != "0"
WINO_WGRAD = _os.environ.get("MIS_WINO_WGRAD", "1") != "0"
WINO_MIN_W = int(_os.environ.get("MIS_WINO_MIN_W", "0"))


WINO2D = 10       # ids >= WINO2D: variant id - WINO2D of the 2-D kernels (conv_wino2d.hip); below: 3-D (conv_wino.hip)


# 1x1x1 convolutions of small volumes with many channels (the space-to-depth form of V-Net's deep kernel-2 / stride-2 layers):
# batched GEMM instead of the spatially tiled direct kernel (conv1x1_gemm.hip), up to this many voxels
CONV1X1_GEMM_MAX_S = 4096


def conv1x1_gemm_eligible(x, y, cin, cout):
    """x / y: 5-D NCDHW views with dense (C, D, H, W); few voxels, many channels, sizes the GEMM's float4 rows need."""
    try:
        _, _, _, _, _, S, xbs = _geom(x)
        _, _, _, _, _, _, ybs = _geom(y)
    except RuntimeError:
        return False
    return (S <= CONV1X1_GEMM_MAX_S and S % 4 == 0 and cout % 4 == 0 and cin >= 64 and xbs % 4 == 0 and ybs % 4 == 0 and
            x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0)


def conv1x1_gemm(x, wt, bias, y, accumulate=False):
    """y[n][co][s] (+)= bias[co] + sum_ci wt[ci][co] x[n][ci][s] (mis_conv1x1_gemm); ``wt`` = the weights [Cin][Cout]."""
    N, Cin, D, H, W, S, xbs = _geom(x)
    _, Cout, _, _, _, _, ybs = _geom(y)
    assert wt.dim() == 2 and wt.shape == (Cin, Cout) and wt.stride(1) == 1, (wt.shape, Cin, Cout)
    ws = _ws("conv1x1", "mis_conv1x1_gemm_workspace_bytes", N, Cin, Cout, S, optional=True, exact=True)
    _tag(f"conv1x1_gemm:{Cin}x{Cout}@{W}")
    _l.launch("mis_conv1x1_gemm", x, xbs, wt, wt.stride(0), bias, y, ybs, N, Cin, Cout, S, int(accumulate), ws)


def conv1x1_wgrad_eligible(a, b):
    """a / b: the two 5-D NCDHW operands of the weight gradient (same N, D, H, W)."""
    try:
        _, _, _, _, _, S, abs_ = _geom(a)
        _, _, _, _, _, _, bbs = _geom(b)
    except RuntimeError:
        return False
    return (S <= CONV1X1_GEMM_MAX_S and S % 4 == 0 and abs_ % 4 == 0 and bbs % 4 == 0 and a.data_ptr() % 16 == 0 and
            b.data_ptr() % 16 == 0 and min(a.shape[1], b.shape[1]) >= 64)


def conv1x1_wgrad(a, b, dw, accumulate=False):
    """dw[M][Nc] (+)= sum_{image, voxel} a[.][m][s] * b[.][n][s] (mis_conv1x1_wgrad); dw: a 2-D view [a channels][b channels]."""
    N, M, D, H, W, S, abs_ = _geom(a)
    _, Nc, _, _, _, _, bbs = _geom(b)
    assert dw.dim() == 2 and dw.shape == (M, Nc) and dw.stride(1) == 1, (dw.shape, M, Nc)
    ws = _ws("conv1x1_wgrad", "mis_conv1x1_wgrad_workspace_bytes", N, M, Nc, S, exact=True)
    _tag(f"conv1x1_wgrad:{M}x{Nc}@{W}")
    _l.launch("mis_conv1x1_wgrad", a, abs_, b, bbs, dw, dw.stride(0), N, M, Nc, S, int(accumulate), ws)


def conv_wino_select(N, Cin, Cout, D, H, W, ksize, dilation=1):
    """Winograd variant serving this convolution (mis_conv3d_wino_select / mis_conv2d_wino_select), or -1: use the
    direct kernel.  A dilated convolution has no Winograd form here: -1."""
    if not WINO or dilation != 1:
        return -1
    k = _ksize(ksize)
    if k == (3, 3, 3) and (WINO & 1):
        if not WINO_FWD or W < WINO_MIN_W:
            return -1
        return _l.select("mis_conv3d_wino_select", N, Cin, Cout, D, H, W)
    if k == (1, 3, 3) and D == 1 and (WINO & 2):
        v = _l.select("mis_conv2d_wino_select", N, Cin, Cout, H, W)
        return v + WINO2D if v >= 0 else -1
    return -1


def conv_wino_pack_mode(wino, dgrad):
    """Pack mode of the transformed filter for this variant (4 / 5: 3x3x3, 6 / 7: 3x3; forward / data gradient)."""
    return (6 if wino >= WINO2D else 4) + (1 if dgrad else 0)


def conv_stat_tiles(N, Cin, Cout, D, H, W, ksize, wino=-1):
    """Partial-statistics tiles per image of the fused conv+stats form for this geometry (0: not eligible)."""
    kd, kh, kw = _ksize(ksize)
    if wino >= WINO2D:
        return _l.query("mis_conv2d_wino_stat_tiles", H, W, wino - WINO2D)
    if wino >= 0:
        return _l.query("mis_conv3d_wino_stat_tiles", D, H, W, wino)
    return _l.query("mis_conv_fwd_stat_tiles", N, Cin, Cout, D, H, W, kd, kh, kw)


def norm_stats_finalize(part, N, C, S, tiles, per_sample, eps, mean, rstd, running_mean=None, running_var=None,
                        num_batches=None, momentum=0.1):
    _l.launch("mis_norm_stats_finalize", part, N, C, S, tiles, int(per_sample), eps, mean, rstd, running_mean, running_var,
              num_batches, momentum)


def conv_fwd(x, wp, bias, y, Cin, Cout, ksize, stat=None, wino=-1):
    """y = conv(x) with packed weights ``wp``; stride 1, 'same' zero padding, k in {1,3}.
    ``stat = (buffer, stride_channel, stride_image)``: also emit the per-tile (sum, sumsq) of y (mis_conv_fwd_stats).
    ``wino >= 0``: ``wp`` is the Winograd-transformed filter (pack mode 4 / 5) and that variant of
    mis_conv3d_wino_fwd runs."""
    N, Cx, D, H, W, S, xbs = _geom(x)
    Ny, Cy, Dy, Hy, Wy, _, ybs = _geom(y)
    assert Cx == Cin and Cy == Cout and (N, D, H, W) == (Ny, Dy, Hy, Wy)
    kd, kh, kw = _ksize(ksize)
    prof = _prof_begin()
    if wino >= WINO2D:
        name = ("mis_conv2d_wino_kernel_name", wino - WINO2D)
        _l.launch("mis_conv2d_wino_fwd", x, xbs, wp, bias, y, ybs, N, Cin, Cout, H, W, stat or (None, 0, 0), wino - WINO2D)
    elif wino >= 0:
        name = ("mis_conv3d_wino_kernel_name", wino)
        # few boxes (the 6^3 level, half batches at 12^3): the contraction is cut into slices, partials in scratch
        ws = _ws("wino_fwd", "mis_conv3d_wino_fwd_workspace_bytes", N, Cin, Cout, D, H, W, wino, optional=True, exact=True)
        if ws[0] is not None:
            _tag(f"wino_fwd_split:v{wino}@{W}")
        _l.launch("mis_conv3d_wino_fwd_ws", x, xbs, wp, bias, y, ybs, N, Cin, Cout, D, H, W, stat or (None, 0, 0), wino, ws)
    else:
        name = ("mis_conv_fwd_kernel_name", N, Cin, Cout, D, H, W, kd, kh, kw)
        if stat is not None:
            _l.launch("mis_conv_fwd_stats", x, xbs, wp, bias, y, ybs, N, Cin, Cout, D, H, W, kd, kh, kw, stat)
        else:
            _l.launch("mis_conv_fwd", x, xbs, wp, bias, y, ybs, N, Cin, Cout, D, H, W, kd, kh, kw)
    if prof is not None:
        _prof_end(prof, lambda: _l.kernel_name(*name), 2.0 * N * Cout * Cin * kd * kh * kw * S,
                  4.0 * (N * (Cin + Cout) * S + Cout * Cin * kd * kh * kw))


def conv_dgrad_norm(dy, wpd, da, Cin, Cout, xn, mean, slope, part, wino):
    """The Winograd data gradient ``da = dgrad(dy)`` (``wpd``: pack mode 5) with the first stage of the backward of the
    InstanceNorm + (Leaky)ReLU that produced the conv's input from ``xn`` in its epilogue (mis_conv3d_wino_dgrad_norm):
    ``part [N*Cout*tiles, 2]`` receives (sum dz, sum dz * xn) per (n, channel, tile).  ``Cin`` / ``Cout``: channels of
    dy / da.  Returns the number of tiles per image."""
    N, C, D, H, W, S, dbs = _geom(dy)
    da_v, xn_v = _view(da), _view(xn)
    assert C == Cin and da.shape[1] == Cout and xn.shape[1] == Cout
    tiles = _l.query("mis_conv3d_wino_stat_tiles", D, H, W, wino)
    assert part.numel() >= N * Cout * tiles * 2
    prof = _prof_begin()
    _l.launch("mis_conv3d_wino_dgrad_norm", dy, dbs, wpd, da_v, N, Cin, Cout, D, H, W, xn_v, mean, float(slope), part,
              tiles, Cout * tiles, wino)
    if prof is not None:
        _prof_end(prof, lambda: _l.kernel_name("mis_conv3d_wino_kernel_name", wino).replace(", false>", ", true>"),
                  2.0 * N * Cout * Cin * 27 * S, 4.0 * (N * (Cin + 2 * Cout) * S + Cout * Cin * 27))     # + the norm input it reads
    return tiles


def norm_act_bwd_tiles(x, da, dx, mean, rstd, slope, part, tiles, sums):
    """Second stage + apply pass of the InstanceNorm + (Leaky)ReLU backward from conv_dgrad_norm's partials; ``dx`` may
    be None (only ``sums`` is wanted: the first layer's weight gradient forms dx itself)."""
    N, C, D, H, W, S, xbs = _geom(x)
    _l.launch("mis_norm_act_bwd_tiles", x, xbs, _view(da), _view(dx), N, C, S, mean, rstd, float(slope), part, int(tiles), sums)


def conv_wgrad(x, dy, dw, ksize, accumulate=False):
    """dw[Cout,Cin,*k] (+)= sum_n,p dy * shifted x."""
    N, Cin, D, H, W, S, xbs = _geom(x)
    _, Cout, _, _, _, _, dbs = _geom(dy)
    kd, kh, kw = _ksize(ksize)
    assert dw.is_contiguous() and dw.numel() == Cout * Cin * kd * kh * kw
    prof = _prof_begin()
    name = _conv_wgrad_launch(x, dy, dw, N, Cin, Cout, D, H, W, xbs, dbs, kd, kh, kw, accumulate)
    # bench.py's live roofline: the weight gradients count towards the executed step flops
    if prof is not None:
        _prof_end(prof, lambda: _l.kernel_name(*name), 2.0 * N * Cout * Cin * kd * kh * kw * S,
                  4.0 * (N * (Cin + Cout) * S + Cout * Cin * kd * kh * kw))


def _conv_wgrad_launch(x, dy, dw, N, Cin, Cout, D, H, W, xbs, dbs, kd, kh, kw, accumulate):
    """Launches the weight gradient; returns the ``kernel_name`` query of what it ran."""
    aligned = xbs % 4 == 0 and dbs % 4 == 0 and x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0
    # 3x3x3 on large volumes: the Winograd F(2^3, 3^3) form (conv_wino_wgrad.hip), 3.375x fewer matrix-pipe flops
    wino = -1
    if (WINO & 1) and WINO_WGRAD and W >= WINO_MIN_W and (kd, kh, kw) == (3, 3, 3):
        wino = _l.select("mis_conv3d_wino_wgrad_select", N, Cin, Cout, D, H, W)
    if wino >= 0 and aligned:
        ws = _ws("wgrad", "mis_conv3d_wino_wgrad_workspace_bytes", N, Cin, Cout, D, H, W, wino)
        _tag(f"wino_wgrad:v{wino}@{W}")
        _l.launch("mis_conv3d_wino_wgrad", x, xbs, dy, dbs, dw, ws, N, Cin, Cout, D, H, W, int(accumulate), wino)
        return "mis_conv3d_wino_wgrad_kernel_name", wino
    wino2 = -1
    if (WINO & 2) and (kd, kh, kw) == (1, 3, 3) and D == 1:
        wino2 = _l.select("mis_conv2d_wino_wgrad_select", N, Cin, Cout, H, W)
    if wino2 >= 0 and aligned:
        ws = _ws("wgrad", "mis_conv2d_wino_wgrad_workspace_bytes", N, Cin, Cout, H, W, wino2)
        _l.launch("mis_conv2d_wino_wgrad", x, xbs, dy, dbs, dw, ws, N, Cin, Cout, H, W, int(accumulate), wino2)
        return "mis_conv2d_wino_wgrad_kernel_name", wino2
    ws = _ws("wgrad", "mis_conv_wgrad_workspace_bytes", N, Cin, Cout, D, H, W, kd, kh, kw)
    _tag(f"direct_wgrad:k{kd}{kh}{kw}@{W}")
    _l.launch("mis_conv_wgrad", x, xbs, dy, dbs, dw, ws, N, Cin, Cout, D, H, W, kd, kh, kw, int(accumulate))
    return "mis_conv_wgrad_kernel_name", N, Cin, Cout, D, H, W, kd, kh, kw


# ------------------------------------------------------- dilated 3x3 convolution (conv_dilated.hip, mis_hip_dilated.h)
def _dilated_geom(x, y):
    N, Cx, D, H, W, S, xbs = _geom(x)
    Ny, Cy, Dy, Hy, Wy, _, ybs = _geom(y)
    if D != 1 or (N, D, H, W) != (Ny, Dy, Hy, Wy):
        raise RuntimeError(f"dilated convolution: 2-D tensors of one geometry expected, got {tuple(x.shape)} {tuple(y.shape)}")
    return N, Cx, Cy, H, W, xbs, ybs


def conv_dilated_fwd_kernel_name(N, Cin, Cout, H, W, dilation):
    return _l.kernel_name("mis_conv_dilated_fwd_kernel_name", N, Cin, Cout, H, W, int(dilation))


def conv_dilated_dgrad_kernel_name(N, Cin, Cout, H, W, dilation):
    return _l.kernel_name("mis_conv_dilated_dgrad_kernel_name", N, Cin, Cout, H, W, int(dilation))


def conv_dilated_wgrad_kernel_name(N, Cin, Cout, H, W, dilation):
    return _l.kernel_name("mis_conv_dilated_wgrad_kernel_name", N, Cin, Cout, H, W, int(dilation))


def conv_dilated_fwd(x, wp, bias, y, dilation, dgrad=False):
    """y = bias + conv3x3(x, dilation = padding = ``dilation``) with packed weights ``wp`` (mode 0, taps = 9).
    ``dgrad``: ``x`` is the output gradient, ``wp`` the mode-1 pack and ``y`` receives the input gradient (no bias)."""
    N, Cx, Cy, H, W, xbs, ybs = _dilated_geom(x, y)
    prof = _prof_begin()
    if dgrad:
        assert bias is None
        _l.launch("mis_conv_dilated_dgrad", x, xbs, wp, y, ybs, N, Cy, Cx, H, W, int(dilation))
    else:
        _l.launch("mis_conv_dilated_fwd", x, xbs, wp, bias, y, ybs, N, Cx, Cy, H, W, int(dilation))
    if prof is not None:
        _prof_end(prof, lambda: conv_dilated_fwd_kernel_name(N, Cx, Cy, H, W, dilation), 2.0 * N * Cy * Cx * 9 * H * W,
                  4.0 * (N * (Cx + Cy) * H * W + Cy * Cx * 9))


def conv_dilated_wgrad(x, dy, dw, dilation, accumulate=False):
    """dw[Cout,Cin,3,3] (+)= the weight gradient of the dilated convolution; deterministic."""
    N, Cin, Cout, H, W, xbs, dbs = _dilated_geom(x, dy)
    assert dw.is_contiguous() and dw.numel() == Cout * Cin * 9
    ws = _ws("wgrad", "mis_conv_dilated_wgrad_workspace_bytes", N, Cin, Cout, H, W, int(dilation))
    prof = _prof_begin()
    _tag(f"dilated_wgrad:d{dilation}@{W}")
    _l.launch("mis_conv_dilated_wgrad", x, xbs, dy, dbs, dw, ws, N, Cin, Cout, H, W, int(dilation), int(accumulate))
    if prof is not None:
        _prof_end(prof, lambda: conv_dilated_wgrad_kernel_name(N, Cin, Cout, H, W, dilation), 2.0 * N * Cout * Cin * 9 * H * W,
                  4.0 * (N * (Cin + Cout) * H * W + Cout * Cin * 9))


# ------------------------------------------------------- norm + act + dropout
def norm_stats(x, per_sample, eps, mean, rstd, running_mean=None, running_var=None, num_batches=None,
               momentum=0.1):
    N, C, D, H, W, S, xbs = _geom(x)
    ws = _ws("norm", "mis_norm_workspace_bytes", N, C, S, int(per_sample))
    _l.launch("mis_norm_stats", x, xbs, N, C, S, int(per_sample), eps, mean, rstd, running_mean, running_var, num_batches,
              momentum, ws)


def channel_sum(x, out, accumulate=False):
    """out[c] (+)= sum_{n,s} x[n,c,s]  (conv bias gradient)."""
    N, C, D, H, W, S, xbs = _geom(x)
    ws = _ws("norm", "mis_norm_workspace_bytes", N, C, S, 0)
    _l.launch("mis_channel_sum", x, xbs, N, C, S, out, int(accumulate), ws)


def norm_stats_from_running(running_mean, running_var, eps, mean, rstd):
    _l.launch("mis_norm_stats_from_running", running_mean, running_var, eps, mean, rstd, running_mean.numel())


def norm_act_fwd(x, y, per_sample, mean, rstd, gamma, beta, slope, drop_p=0.0, drop_salt=0, state=None,
                 drop_mask=None, cg=1):
    """``cg``: channels per statistics group of a per-sample norm (1 InstanceNorm, C/16 GroupNorm(16))."""
    N, C, D, H, W, S, xbs = _geom(x)
    _l.launch("mis_norm_act_fwd_g", x, xbs, _view(y), N, C, S, int(per_sample), int(cg), mean, rstd, gamma, beta, slope, drop_p,
              drop_salt, state, drop_mask)


def norm_act_bwd(x, da, dx, per_sample, mean, rstd, gamma, beta, slope, drop_p=0.0, drop_salt=0, state=None,
                 drop_mask=None, dgamma=None, dbeta=None, accumulate_affine=False, cg=1, no_norm=False):
    N, C, D, H, W, S, xbs = _geom(x)
    ws = _ws("norm", "mis_norm_workspace_bytes", N, C, S, int(per_sample))
    _l.launch("mis_norm_act_bwd_g", x, xbs, _view(da), _view(dx), N, C, S, int(per_sample), int(cg), int(no_norm), mean, rstd,
              gamma, beta, slope, drop_p, drop_salt, state, drop_mask, dgamma, dbeta, int(accumulate_affine), ws)


def norm_res_act_fwd(x, res, y, per_sample, mean, rstd, gamma, beta, slope, post=False):
    """y = act(norm(x) + res) in one pass (mis_norm_res_act_fwd); ``post``: y = act(norm(x)) + res."""
    N, C, D, H, W, S, xbs = _geom(x)
    _l.launch("mis_norm_res_act_fwd", x, xbs, _view(res), _view(y), N, C, S, int(per_sample), mean, rstd, gamma, beta, slope,
              int(post))


def norm_res_act_bwd(x, res, dy, dx, dres, accumulate_dres, per_sample, mean, rstd, gamma, beta, slope, dgamma=None,
                     dbeta=None, accumulate_affine=False, post=False):
    """Backward of norm_res_act_fwd: dres (+)= dz, dx = norm backward of dz, dz = dy * act'(norm(x) + res)."""
    N, C, D, H, W, S, xbs = _geom(x)
    ws = _ws("norm", "mis_norm_workspace_bytes", N, C, S, int(per_sample))
    _l.launch("mis_norm_res_act_bwd", x, xbs, _view(res), _view(dy), _view(dx), _view(dres), int(accumulate_dres), N, C, S,
              int(per_sample), mean, rstd, gamma, beta, slope, dgamma, dbeta, int(accumulate_affine), int(post), ws)


def norm_act_fwd_pool(x, y, pooled, idx, per_sample, mean, rstd, gamma, beta, slope, drop_p=0.0, drop_salt=0, state=None,
                      drop_mask=None, cg=1):
    """norm_act_fwd and the 2x max-pool of its output (pooled, idx as maxpool2_fwd writes them) in one pass."""
    N, C, D, H, W, S, xbs = _geom(x)
    _l.launch("mis_norm_act_fwd_pool", x, xbs, _view(y), _view(pooled), idx, N, C, D, H, W, int(per_sample), int(cg), mean, rstd,
              gamma, beta, slope, drop_p, drop_salt, state, drop_mask)


def norm_act_bwd_pool(x, da, dpool, idx, dx, per_sample, mean, rstd, gamma, beta, slope, drop_p=0.0, drop_salt=0,
                      state=None, drop_mask=None, dgamma=None, dbeta=None, accumulate_affine=False, cg=1):
    """norm_act_bwd of an activation that also feeds a 2x max-pool: incoming gradient = da (None: no other consumer) +
    the pool's backward of dpool through the argmax codes idx, added on the load path (no maxpool2_bwd pass)."""
    N, C, D, H, W, S, xbs = _geom(x)
    ws = _ws("norm", "mis_norm_workspace_bytes", N, C, S, int(per_sample))
    _l.launch("mis_norm_act_bwd_pool", x, xbs, _view(da), _view(dpool), idx, _view(dx), N, C, D, H, W, int(per_sample), int(cg),
              mean, rstd, gamma, beta, slope, drop_p, drop_salt, state, drop_mask, dgamma, dbeta, int(accumulate_affine), ws)


def norm_act_bwd_sums(x, da, per_sample, mean, rstd, gamma, beta, slope, sums, dgamma=None, dbeta=None,
                      accumulate_affine=False):
    """The reduction half of norm_act_bwd: sums[group] = (mean dz, mean dz*xhat) (+ dgamma / dbeta); no dropout."""
    N, C, D, H, W, S, xbs = _geom(x)
    ws = _ws("norm", "mis_norm_workspace_bytes", N, C, S, int(per_sample))
    _l.launch("mis_norm_act_bwd_sums", x, xbs, _view(da), N, C, S, int(per_sample), mean, rstd, gamma, beta, slope, sums, dgamma,
              dbeta, int(accumulate_affine), ws)


def conv_wgrad_cin1_norm_eligible(N, Cout, D, H, W):
    return bool(_l.query("mis_conv_wgrad_cin1_norm_eligible", N, Cout, D, H, W))


def conv_wgrad_cin1_norm(x, da, y, per_sample, mean, rstd, gamma, beta, sums, slope, dw, accumulate=False):
    """dw of the first layer Conv3d(1 -> 16, 3) from the gradient at the activation after its norm + (Leaky)ReLU."""
    N, Cin, D, H, W, S, xbs = _geom(x)
    _, Cout, _, _, _, _, ybs = _geom(y)
    ws = _ws("wgrad", "mis_conv_wgrad_workspace_bytes", N, Cin, Cout, D, H, W, 1 if D == 1 else 3, 3, 3)
    _l.launch("mis_conv_wgrad_cin1_norm", x, xbs, _view(da), y, ybs, N, D, H, W, int(per_sample), mean, rstd, gamma, beta, sums,
              slope, dw, ws, int(accumulate))


def norm_head_eligible(C, K, per_sample, gamma, beta, cg=1, no_norm=False):
    """norm + act + dropout + 1x1x1 classifier as one pass (mis_norm_head_*): C == 16, K in 2..4, one statistics group per
    channel, InstanceNorm only without affine."""
    return bool(_l.query("mis_norm_head_eligible", C, K)) and cg == 1 and not no_norm and not (
        per_sample and (gamma is not None or beta is not None))


def norm_head_bits(x):
    """The buffer of a head's dropout decisions (``bits`` of norm_head_fwd / _bwd): one 64-bit word per 4 voxels of a sample."""
    N, C, D, H, W, S, _ = _geom(x)
    return torch.empty(N * (S // 4), dtype=torch.int64, device=x.device)


def norm_head_fwd(x, logits, per_sample, mean, rstd, gamma, beta, slope, w, b, drop_p=0.0, drop_salt=0, state=None,
                  drop_mask=None, bits=None):
    """logits = W . drop(act(norm(x))) + b without storing the activation (w: [K, C] view of the 1x1x1 conv weight).
    ``bits`` (norm_head_bits): the Philox dropout decisions are stored there for norm_head_bwd."""
    N, C, D, H, W, S, xbs = _geom(x)
    _, K, _, _, _, _, lbs = _geom(logits)
    assert bits is None or (bits.dtype == torch.int64 and bits.is_contiguous() and bits.numel() >= N * (S // 4))
    _l.launch("mis_norm_head_fwd", x, xbs, N, C, S, int(per_sample), mean, rstd, gamma, beta, slope, drop_p, drop_salt, state,
              drop_mask, w, b, K, logits, lbs, bits)


def norm_head_bwd(x, dlogits, dx, per_sample, mean, rstd, gamma, beta, slope, w, dw, db, drop_p=0.0, drop_salt=0,
                  state=None, drop_mask=None, dgamma=None, dbeta=None, accumulate_affine=False, accumulate_w=False, bits=None):
    """``bits``: what norm_head_fwd stored for this x, seed, offset and salt; read in place of drawing the mask again."""
    N, C, D, H, W, S, xbs = _geom(x)
    _, K, _, _, _, _, dlbs = _geom(dlogits)
    ws = _ws("norm", "mis_norm_head_workspace_bytes", N, C, S, int(per_sample), K)
    assert bits is None or (bits.dtype == torch.int64 and bits.is_contiguous() and bits.numel() >= N * (S // 4))
    _l.launch("mis_norm_head_bwd", x, xbs, dlogits, dlbs, _view(dx), N, C, S, int(per_sample), mean, rstd, gamma, beta, slope,
              drop_p, drop_salt, state, drop_mask, w, K, dgamma, dbeta, int(accumulate_affine), dw, db, int(accumulate_w), bits,
              ws)


def group_norm_stats(x, cg, eps, mean, rstd):
    """(mean, rstd) per (n, group of ``cg`` consecutive channels): the groups are contiguous in NCDHW, so this is the
    InstanceNorm statistics kernel on the [N, C/cg, cg*S] view of the same memory."""
    N, C, D, H, W, S, xbs = _geom(x)
    G = C // cg
    ws = _ws("norm", "mis_norm_workspace_bytes", N, G, cg * S, 1)
    _l.launch("mis_norm_stats", x, xbs, N, G, cg * S, 1, eps, mean, rstd, None, None, None, 0.0, ws)


# ------------------------------------------------------------ pool / upsample
def maxpool2_fwd(x, y, idx):
    N, C, D, H, W, S, xbs = _geom(x)
    _l.launch("mis_maxpool2_fwd", x, xbs, _view(y), idx, N, C, D, H, W)


def maxpool2_bwd(dy, idx, dx, accumulate=False):
    N, C, D, H, W, S, dxbs = _geom(dx)
    _l.launch("mis_maxpool2_bwd", _view(dy), idx, dx, dxbs, N, C, D, H, W, int(accumulate))


def upsample2_fwd(x, y, align_corners):
    N, C, D, H, W, S, xbs = _geom(x)
    _l.launch("mis_upsample2_fwd", x, xbs, _view(y), N, C, D, H, W, int(align_corners))


def upsample2_bwd(dy, dx, align_corners, accumulate=False):
    N, C, D, H, W, S, dxbs = _geom(dx)
    _l.launch("mis_upsample2_bwd", _view(dy), dx, dxbs, N, C, D, H, W, int(align_corners), int(accumulate))


# ------------------------------------------------------------------ loss tail
def loss_tail(student, teacher, label, labeled_bs, out, dlogits=None, cons_weight=0.0, state=None,
              loss_scale=1.0):
    """Fused softmax/CE/Dice/consistency.  ``out``: >= 5+C floats:
    [loss, loss_ce, loss_dice, consistency_loss, consistency_weight, class-wise dice...]."""
    B, C, D, H, W, S, sbs = _geom(student)
    tbs = 0
    if teacher is not None:
        Bt, Ct, _, _, _, St, tbs = _geom(teacher)
        assert Bt == B - labeled_bs and Ct == C and St == S
    ws = _ws("tail", "mis_loss_tail_workspace_bytes", B, C, S)
    _l.launch("mis_loss_tail", student, sbs, teacher, tbs, _label(label, labeled_bs * S, optional=True), B, labeled_bs, C, S,
              cons_weight, state, loss_scale, out, _view(dlogits), ws)


def softmax_mean_accumulate(logits, acc, repeats, scale, first):
    """acc[u] (+)= scale * sum_r softmax(logits[r*U + u]) over the channel dim (UA-MT MC-dropout mean)."""
    Bl, C, D, H, W, S, lbs = _geom(logits)
    U, Ca, _, _, _, Sa, abs_ = _geom(acc)
    assert Bl == repeats * U and Ca == C and Sa == S
    _l.launch("mis_softmax_mean_accumulate", logits, lbs, acc, abs_, U, repeats, C, S, scale, int(first))


def uamt_tail(student, teacher, mean_probs, label, labeled_bs, out, max_iterations, dlogits=None, cons_weight=0.0,
              state=None, iter_num=0, loss_scale=1.0):
    """UA-MT loss tail.  ``out`` (>= 7+C floats): [loss, loss_ce, loss_dice, consistency_loss, consistency_weight,
    class-wise dice..., #unmasked voxels, threshold]."""
    B, C, D, H, W, S, sbs = _geom(student)
    Bt, Ct, _, _, _, St, tbs = _geom(teacher)
    Bm, Cm, _, _, _, Sm, mbs = _geom(mean_probs)
    assert Bt == Bm == B - labeled_bs and Ct == Cm == C and St == Sm == S
    ws = _ws("tail", "mis_uamt_tail_workspace_bytes", B, C, S)
    _l.launch("mis_uamt_tail", student, sbs, teacher, tbs, mean_probs, mbs, _label(label, labeled_bs * S), B, labeled_bs, C, S,
              cons_weight, state, int(iter_num), float(max_iterations), loss_scale, out, _view(dlogits), ws)


ICT_BETA_SALT = 0x1C7BE7A0


def beta_sample(lam, alpha, state, salt=ICT_BETA_SALT):
    """lam[m] ~ Beta(alpha, alpha) on the device, keyed by (seed, iter_num) of ``state`` and ``salt`` (ICT mix factors,
    reference np.random.beta(ict_alpha, ict_alpha, size=(L // 2, 1, 1, 1)))."""
    _l.require_gpu(lam, state)
    assert lam.dtype == torch.float32 and lam.is_contiguous() and lam.numel() > 0
    if not float(alpha) > 0.0:
        raise ValueError(f"Beta(alpha, alpha) needs alpha > 0, got {alpha}")
    _l.launch("mis_beta_sample", lam, lam.numel(), float(alpha), int(salt) & 0xFFFFFFFF, state)


def ict_mix(x, lam, labeled_bs, out):
    """out[:L] = x[:L]; out[L + m] = x[L + m] * (1 - lam[m]) + x[L + M + m] * lam[m] with M = lam.numel() and
    x.shape[0] == L + 2M (ICT input of the student, bit-identical to the torch expression)."""
    _l.require_gpu(x, lam, out)
    M = lam.numel()
    assert x.dtype == out.dtype == lam.dtype == torch.float32
    assert x.is_contiguous() and out.is_contiguous() and lam.is_contiguous()
    assert x.shape[0] == labeled_bs + 2 * M and out.shape[0] == labeled_bs + M
    assert tuple(x.shape[1:]) == tuple(out.shape[1:])
    n = x[0].numel()
    _l.launch("mis_ict_mix", x, out, lam, labeled_bs, M, n)


def ict_tail(student, teacher0, teacher1, lam, label, labeled_bs, out, dlogits=None, cons_weight=0.0, state=None,
             loss_scale=1.0):
    """ICT loss tail: 0.5*(CE+Dice) on student[:L] + w * mean((softmax(student[L:]) - target)^2), target =
    softmax(teacher0) * (1 - lam) + softmax(teacher1) * lam.  ``out`` (>= 5+C floats): the layout of loss_tail."""
    B, C, D, H, W, S, sbs = _geom(student)
    M = B - labeled_bs
    B0, C0, _, _, _, S0, t0bs = _geom(teacher0)
    B1, C1, _, _, _, S1, t1bs = _geom(teacher1)
    assert B0 == B1 == M and C0 == C1 == C and S0 == S1 == S
    _l.require_gpu(lam)
    assert lam.dtype == torch.float32 and lam.is_contiguous() and lam.numel() == M
    ws = _ws("tail", "mis_ict_tail_workspace_bytes", B, C, S)
    _l.launch("mis_ict_tail", student, sbs, teacher0, t0bs, teacher1, t1bs, lam, _label(label, labeled_bs * S), labeled_bs, M,
              C, S, cons_weight, state, loss_scale, out, _view(dlogits), ws)


def _sched_args(sched, k):
    if sched is None:
        if int(k) < 0:
            raise ValueError("rotation k < 0 reads sched[state.iter_num]: a schedule and a step state are needed")
        return None, 0
    _l.require_gpu(sched)
    assert sched.dtype == torch.int32 and sched.is_contiguous() and sched.numel() > 0
    return sched, sched.numel()


def rot90(x, out, k=-1, sched=None, state=None):
    """out = torch.rot90(x, k, [2, 3]) for x [N, C, H, W] (free batch stride, dense planes: e.g. ``volume[L:]``),
    bit-identical.  ``k`` < 0: read on the device, ``sched[state.iter_num]`` (deep co-training's rotation per iteration)."""
    _l.require_gpu(x, out, state)
    if x.dim() != 4 or out.dim() != 4 or x.dtype != torch.float32 or out.dtype != torch.float32:
        raise RuntimeError(f"rot90 takes fp32 [N,C,H,W] tensors, got {tuple(x.shape)} / {tuple(out.shape)}")
    N, C, H, W = x.shape
    assert x[0].is_contiguous() and out.is_contiguous()
    want = (N, C, W, H) if int(k) >= 0 and int(k) % 2 else (N, C, H, W)
    if tuple(out.shape) != want:
        raise RuntimeError(f"rot90: output {tuple(out.shape)}, expected {want}")
    in_bs = x.stride(0) if N > 1 else C * H * W
    _l.launch("mis_rot90", x, in_bs, out, C * H * W, N, C, H, W, _sched_args(sched, k), state, int(k))


def dct_tail(logits_a, logits_r, label, labeled_bs, out, dA=None, dR=None, k=-1, sched=None, state=None,
             cons_weight=0.0, loss_scale=1.0):
    """Deep co-training loss tail over pass A (the batch, [L+U,C,1,H,W]) and pass R (the rotated unlabeled part,
    [U,C,1,H,W]).  ``out`` (>= 6+C floats): [loss, loss_ce, loss_dice, consistency_loss, consistency_weight, k,
    class-wise dice...]; ``dA`` / ``dR``: the logits gradients of both passes (both or neither)."""
    B, C, D, H, W, S, abs_ = _geom(logits_a)
    U, Cr, Dr, Hr, Wr, _, rbs = _geom(logits_r)
    assert D == Dr == 1 and Cr == C and (Hr, Wr) == (H, W) and U == B - labeled_bs
    _l.require_gpu(state)
    ws = _ws("tail", "mis_dct_tail_workspace_bytes", labeled_bs, U, C, H, W)
    _l.launch("mis_dct_tail", logits_a, abs_, logits_r, rbs, _label(label, labeled_bs * S), labeled_bs, U, C, H, W,
              _sched_args(sched, k), state, int(k), cons_weight, loss_scale, out, _view(dA), _view(dR), ws)


def grad_combine(dst, src, accumulate):
    """dst = src, or dst += src with ``accumulate`` (flat gradient buffers; a launch, so it lands on a launch tape)."""
    _l.require_gpu(dst, src)
    assert dst.dtype == src.dtype == torch.float32 and dst.is_contiguous() and src.is_contiguous()
    assert dst.numel() == src.numel()
    _l.launch("mis_grad_combine", dst, src, dst.numel(), int(bool(accumulate)))


FIXMATCH_JITTER_SALT = 0xF1A7C401
FIXMATCH_OUT = ("loss", "sup_ce", "sup_dice", "unsup", "consistency_weight", "ce_u", "dice_u", "ce_comp", "as_weight",
                "masked_in_fraction")


def color_jitter(x, out, params=None, state=None, drawn=None, salt=FIXMATCH_JITTER_SALT):
    """out = ColorJitter(0.8, 0.8, 0.8, 0.2)(x) for one-channel images x [B, 1, ...] (free batch stride, dense planes):
    brightness and contrast per image, in the order of that image.  ``params`` ([B, 3] fp32: beta, gamma, order; order 0 =
    brightness first) gives the factors; without it they are drawn on the device from ``state`` (seed, iter_num) under
    ``salt``.  ``drawn`` ([B, 3] fp32) receives the factors used."""
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
    ws = _ws("jitter", "mis_color_jitter_workspace_bytes", B, S)
    _l.launch("mis_color_jitter", x, xbs, out, ybs, B, S, params, state, int(salt) & 0xFFFFFFFF, drawn, ws)


def fixmatch_tail(weak, strong, label, labeled_bs, out, d_weak=None, d_strong=None, conf_thresh=0.8, cons_weight=0.0,
                  state=None, pseudo=None, comp=None):
    """FixMatch loss tail over the logits of one network on the weak and on the strong batch (both [B,C,D,H,W]).
    ``out`` (>= 10 floats): FIXMATCH_OUT.  ``d_weak`` / ``d_strong``: the logits gradients (either may be None).
    ``pseudo`` ([B-L, S] uint8) / ``comp`` ([B, S] uint8) receive the kernel's pseudo and complementary labels."""
    B, C, D, H, W, S, wbs = _geom(weak)
    Bs, Cs, _, _, _, Ss, sbs = _geom(strong)
    assert (Bs, Cs, Ss) == (B, C, S)
    _l.require_gpu(state, out, pseudo, comp)
    assert out.dtype == torch.float32 and out.numel() >= len(FIXMATCH_OUT)
    for t, n in ((pseudo, (B - labeled_bs) * S), (comp, B * S)):
        assert t is None or (t.dtype == torch.uint8 and t.is_contiguous() and t.numel() == n)
    ws = _ws("tail", "mis_fixmatch_tail_workspace_bytes", B, C, S)
    _l.launch("mis_fixmatch_tail", weak, wbs, strong, sbs, _label(label, labeled_bs * S), B, labeled_bs, C, S,
              float(conf_thresh), cons_weight, state, out, _view(d_weak), _view(d_strong), pseudo, comp, ws)


def cross_teaching_tail(own, other, label, labeled_bs, out, dlogits=None, cons_weight=0.0, state=None,
                        pseudo_ce=False, teacher=None, mt_weight=0.0):
    """0.5*(CE+Dice) on the labeled half + w * Dice (``pseudo_ce``: cross-entropy, CPS) against the other network's
    arg-max pseudo labels.  ``out`` (>= 5 floats): [loss_m, loss_ce, loss_dice, pseudo_supervision, consistency_weight].
    ``teacher`` (EMA-teacher logits of the unlabeled half): + mt_weight * softmax-MSE consistency, out[5:7] =
    [consistency_loss, mt_weight] (reference code/train_cnn_meet_vit_2D.py:300-337)."""
    B, C, D, H, W, S, sbs = _geom(own)
    Bo, Co, _, _, _, So, obs = _geom(other)
    assert (Bo, Co, So) == (B, C, S)
    if teacher is not None:
        Bt, Ct, _, _, _, St, tbs = _geom(teacher)
        assert (Bt, Ct, St) == (B - labeled_bs, C, S)
    lab, dl = _label(label, labeled_bs * S), _view(dlogits)
    ws = _ws("tail", "mis_cross_teaching_tail_workspace_bytes", B, C, S)
    if teacher is not None:
        _l.launch("mis_cross_pseudo_mt_tail", own, sbs, other, obs, teacher, tbs, lab, B, labeled_bs, C, S, cons_weight,
                  mt_weight, state, int(bool(pseudo_ce)), out, dl, ws)
    else:
        _l.launch("mis_cross_pseudo_tail", own, sbs, other, obs, lab, B, labeled_bs, C, S, cons_weight, state,
                  int(bool(pseudo_ce)), out, dl, ws)


def triple_view_tail(z1, z2, z3, label, labeled_bs, outs, dlogits=None, cons_weight=0.0, state=None):
    """Triple-view loss tail of three students' logits [B,C,D,H,W]: for each, 0.5*(CE+Dice) on the labeled half + w * Dice
    against the arg-max pseudo labels of EACH of the other two on the unlabeled half (reference
    code/train_tripleview_2D(demo).py:290-335).  ``outs``: three buffers of >= 6 floats, [loss_m, loss_ce, loss_dice,
    pseudo_supervision_a, consistency_weight, pseudo_supervision_b]; ``dlogits``: three gradient buffers or None."""
    B, C, D, H, W, S, bs1 = _geom(z1)
    assert len(outs) == 3 and all(o.dtype == torch.float32 and o.numel() >= 6 for o in outs)
    _l.require_gpu(state, *outs)
    if dlogits is None:
        dlogits = (None, None, None)
    assert len(dlogits) == 3
    views = []                                  # z2, z3, then the three gradients: (pointer, batch stride) each
    for t in (z2, z3) + tuple(dlogits):
        if t is not None:
            g = _geom(t)
            assert (g[0], g[1], g[5]) == (B, C, S)
        views.append((t, g[6]) if t is not None else (None, 0))
    ws = _ws("tail", "mis_triple_view_tail_workspace_bytes", B, C, S)
    _l.launch("mis_triple_view_tail", z1, bs1, views[0], views[1], _label(label, labeled_bs * S), B, labeled_bs, C, S,
              cons_weight, state, outs[0], outs[1], outs[2], views[2], views[3], views[4], ws)


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
    ws = _ws("patch_nce", "mis_patch_nce_workspace_bytes", B, d, N)
    _l.launch("mis_patch_nce", feat_q, qbs, feat_k, kbs, B, d, N, float(temperature), float(grad_scale), out, dfeat, dbs, ws)


CONTRASTIVE_OUT = ("weighted_loss", "loss_ce", "loss_dice", "pseudo_supervision", "consistency_weight", "model_loss")


def contrastive_cross_tail(own, other, label, labeled_bs, out, dlogits=None, extra_l=None, extra_u=None, sup_scale=2.0,
                           pseudo_scale=1.25, extra_scale=1.0, cons_weight=0.0, state=None):
    """One student's loss tail of contrastive cross teaching (mis_contrastive_cross_tail): ``out`` (>= 6 floats,
    CONTRASTIVE_OUT) with out[0] = sup_scale * 0.5 * (CE + Dice) + pseudo_scale * w * Dice(own[L:], argmax other[L:]);
    ``dlogits`` = d out[0] / d own + extra_scale * the head gradients ``extra_l`` ([L/2, C, ...]: labeled rows 0, 2, ...)
    and ``extra_u`` ([B-L, C, ...]: the unlabeled rows), each optional, added in the pass that writes dlogits."""
    B, C, D, H, W, S, sbs = _geom(own)
    Bo, Co, _, _, _, So, obs = _geom(other)
    assert (Bo, Co, So) == (B, C, S)
    _l.require_gpu(state, out)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= len(CONTRASTIVE_OUT)
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
    ws = _ws("tail", "mis_contrastive_cross_tail_workspace_bytes", B, C, S)
    _l.launch("mis_contrastive_cross_tail", own, sbs, other, obs, _label(label, labeled_bs * S), B, labeled_bs, C, S,
              float(sup_scale), float(pseudo_scale), float(cons_weight), state, extra_l, elbs, extra_u, eubs,
              float(extra_scale), out, dlogits, dbs, ws)


def contrastive_step_init(state, seed, iter_num, base_lr, max_iterations, consistency, rampup, iters_per_epoch):
    _l.launch("mis_contrastive_step_init", state, seed, iter_num, base_lr, float(max_iterations), consistency, float(rampup),
              int(iters_per_epoch))


def contrastive_step_advance(state, base_lr, max_iterations, consistency, rampup, iters_per_epoch):
    _l.launch("mis_contrastive_step_advance", state, base_lr, float(max_iterations), consistency, float(rampup),
              int(iters_per_epoch))


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
    _l.require_gpu(param, grad, momentum_buf, ema_param)
    n = param.numel()
    assert grad.numel() == n and momentum_buf.numel() == n and (ema_param is None or ema_param.numel() == n)
    _l.launch("mis_sgd_ema_step", param, grad, momentum_buf, ema_param, n, lr, momentum, weight_decay, ema_alpha, grad_scale,
              state)


def teacher_noise(x, y, state, sigma=0.1, clamp_abs=0.2, salt=0x7EAC4E5):
    _l.require_gpu(x, y, state)
    assert x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel()
    _l.launch("mis_teacher_noise", x, y, x.numel(), sigma, clamp_abs, salt, state)


def new_step_state():
    return torch.zeros(_l.STEP_STATE_BYTES, dtype=torch.uint8, device="cuda")


def step_init(state, seed, iter_num, base_lr, max_iterations, ema_decay, consistency, rampup, ramp_div=150,
              cons_start_iter=0, lr_post_increment=False):
    _l.launch("mis_step_init", state, seed, iter_num, base_lr, float(max_iterations), ema_decay, consistency, rampup, ramp_div,
              cons_start_iter, int(lr_post_increment))


def step_advance(state, base_lr, max_iterations, ema_decay, consistency, rampup, ramp_div=150, cons_start_iter=0,
                 lr_post_increment=False):
    _l.launch("mis_step_advance", state, base_lr, float(max_iterations), ema_decay, consistency, rampup, ramp_div,
              cons_start_iter, int(lr_post_increment))


def read_step_state(state):
    """Host copy of the device step state (one small D2H; not used inside the hot loop)."""
    import struct
    raw = bytes(state.cpu().numpy().tobytes())
    seed, offset, it, lr, alpha, w, gate = struct.unpack("<QQqffff", raw[:40])
    return dict(seed=seed, offset=offset, iter_num=it, lr=lr, ema_alpha=alpha, cons_weight=w, cons_gate=gate)


def argmax_channels(x, out):
    B, C, D, H, W, S, xbs = _geom(x)
    assert out.dtype == torch.uint8 and out.numel() == B * S
    _l.launch("mis_argmax_channels", x, xbs, out, B, C, S)


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


def surface_metrics(pred_u8, gt_u8, cls):
    """The result record of ``mis_surface_metrics`` (int64 [12] on the device; fields in include/mis_hip.h) for the masks
    ``pred == cls`` / ``gt == cls`` (``cls = -1``: label > 0).  Nothing is synchronised: the caller reads the record when it wants
    it (utils.metrics.device_scores)."""
    ndim, D, H, W = _label_geom(pred_u8, gt_u8)
    ws = _ws("surface_metrics", "mis_surface_metrics_workspace_bytes", D, H, W, exact=True)
    out = torch.empty(_l.SURFACE_RECORD_WORDS, dtype=torch.int64, device=pred_u8.device)
    _l.launch("mis_surface_metrics", pred_u8, gt_u8, int(cls), ndim, D, H, W, out, ws)
    return out


def sq_edt(seeds_u8):
    """Exact squared Euclidean distance (int32) of every voxel to the nearest non-zero voxel of ``seeds_u8``."""
    ndim, D, H, W = _label_geom(seeds_u8)
    ws = _ws("surface_metrics", "mis_surface_metrics_workspace_bytes", D, H, W, exact=True)
    out = torch.empty(seeds_u8.shape, dtype=torch.int32, device=seeds_u8.device)
    _l.launch("mis_sq_edt", seeds_u8, ndim, D, H, W, out, ws)
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
    N, GCi, d, h, w, _, tbs = _geom(theta)
    Np, GCp, dp, hp, wp_, _, pbs = _geom(phi)
    Na, G, da, ha, wa, _, abs_ = _geom(att)
    if (Np, GCp, dp, hp, wp_) != (N, GCi, d, h, w) or (Na, da, ha, wa) != (N, d, h, w) or GCi % G or psi_b.numel() != G \
            or psi_w.numel() != GCi or not psi_w.is_contiguous() or not psi_b.is_contiguous():
        raise RuntimeError(f"attention gate map: theta {tuple(theta.shape)}, phi {tuple(phi.shape)}, att {tuple(att.shape)}, "
                           f"psi {tuple(psi_w.shape)} / {tuple(psi_b.shape)} do not belong together (MIS_ERR_ARG)")
    _l.launch("mis_attn_gate_map_fwd", theta, tbs, phi, pbs, psi_w, psi_b, att, abs_, N, G, GCi // G, d, h, w)


def attn_gate_map_bwd(datt, att, theta, phi, psi_w, df, dpsi_w, dpsi_b, dphi_b=None, accumulate=False):
    """df[N,G*Ci,d,h,w] = psi_w dpre [theta + phi > 0] with dpre = datt att (1 - att); dpsi_w (+)= sum relu(theta + phi) dpre,
    dpsi_b (+)= sum dpre, dphi_b[G*Ci] (+)= sum df (the phi convolution's bias gradient; None: not wanted).  Deterministic."""
    N, GCi, d, h, w, _, tbs = _geom(theta)
    phi_v, df_v = _view(phi), _view(df)
    Na, G, da, ha, wa, _, abs_ = _geom(att)
    datt_v = _view(datt)
    if (tuple(phi.shape) != tuple(theta.shape) or tuple(df.shape) != tuple(theta.shape) or tuple(datt.shape) != tuple(att.shape)
            or (Na, da, ha, wa) != (N, d, h, w) or GCi % G or psi_w.numel() != GCi or dpsi_w.numel() != GCi
            or dpsi_b.numel() != G or not (psi_w.is_contiguous() and dpsi_w.is_contiguous() and dpsi_b.is_contiguous())
            or (dphi_b is not None and (dphi_b.numel() != GCi or not dphi_b.is_contiguous()))):
        raise RuntimeError(f"attention gate map backward: theta {tuple(theta.shape)}, att {tuple(att.shape)}, datt "
                           f"{tuple(datt.shape)}, df {tuple(df.shape)} do not belong together (MIS_ERR_ARG)")
    ws = _ws("attn_gate", "mis_attn_gate_map_bwd_workspace_bytes", N, G, GCi // G, d, h, w)
    _l.launch("mis_attn_gate_map_bwd", datt_v, att, abs_, theta, tbs, phi_v, psi_w, df_v, dpsi_w, dpsi_b, dphi_b,
              ws, N, G, GCi // G, d, h, w, int(accumulate))


def attn_gate_apply_fwd(x, att, y):
    """y[N, g C + c] = up2(att[N, g]) * x[N, c]: trilinear x2 (align_corners=False) of the attention maps, x read once."""
    N, G, C, D, H, W, d, h, w, xbs, abs_, ybs = _gate_geom(x, att, y)
    _l.launch("mis_attn_gate_apply_fwd", x, xbs, att, abs_, y, ybs, N, G, C, D, H, W, d, h, w)


def attn_gate_apply_bwd(dy, x, att, dx, datt, accumulate=False):
    """dx (+)= sum_g up2(att_g) dy_g;  datt = up2^T(sum_c dy x).  dy and x are read once."""
    N, G, C, D, H, W, d, h, w, xbs, abs_, dybs = _gate_geom(x, att, dy)
    if tuple(dx.shape) != tuple(x.shape) or tuple(datt.shape) != tuple(att.shape):
        raise RuntimeError(f"attention gate backward: dx {tuple(dx.shape)} / datt {tuple(datt.shape)} do not match x "
                           f"{tuple(x.shape)} / att {tuple(att.shape)} (MIS_ERR_ARG)")
    dx_v, datt_v = _view(dx), _view(datt)
    ws = _ws("attn_gate", "mis_attn_gate_apply_bwd_workspace_bytes", N, G, D, H, W)
    _l.launch("mis_attn_gate_apply_bwd", dy, dybs, x, xbs, att, abs_, dx_v, datt_v, ws, N, G, C, D, H, W,
              d, h, w, int(accumulate))


def _up_int_geom(coarse, fine, scale):
    N, K, d, h, w, _, cbs = _geom(coarse)
    Nf, Kf, D, H, W, _, fbs = _geom(fine)
    if (Nf, Kf) != (N, K) or (D, H, W) != (scale * d, scale * h, scale * w):
        raise RuntimeError(f"upsample x{scale}: {tuple(coarse.shape)} and {tuple(fine.shape)} do not belong together "
                           "(MIS_ERR_ARG)")
    return N, K, d, h, w, cbs, fbs


def upsample_int_fwd(x, y, scale):
    """y = trilinear up-sampling of x by ``scale`` in {2, 4, 8} per axis, align_corners=False."""
    N, K, d, h, w, xbs, ybs = _up_int_geom(x, y, int(scale))
    _l.launch("mis_upsample_int_fwd", x, xbs, y, ybs, N, K, d, h, w, int(scale))


def upsample_int_bwd(dy, dx, scale, accumulate=False):
    """dx (+)= the adjoint of upsample_int_fwd applied to dy (gather form: deterministic)."""
    N, K, d, h, w, dxbs, dybs = _up_int_geom(dx, dy, int(scale))
    _l.launch("mis_upsample_int_bwd", dy, dybs, dx, dxbs, N, K, d, h, w, int(scale), int(accumulate))


# ------------------------------------------------------- adversarial training (csrc/adversarial.hip, csrc/adversarial2d.hip)
ADAM_STATE_BYTES = 16      # int64 step, float 1 - beta1^step, float 1 - beta2^step


def channel_dropout_scale(scale, p, salt, state):
    """scale[N, C] = nn.Dropout3d(p)'s factor per (sample, channel): 0 or 1 / (1 - p), drawn from ``state``."""
    _l.require_gpu(scale)
    assert scale.dim() == 2 and scale.is_contiguous() and scale.dtype == torch.float32
    _l.launch("mis_channel_dropout_scale", scale, scale.shape[0], scale.shape[1], float(p), int(salt), state)


# The kernel-4 / stride-2 convolutions and the head exist per dimension (mis_conv_k4s2_* / mis_adv_head_* in adversarial.hip,
# mis_conv2d_k4s2_* / mis_adv_head2d_* in adversarial2d.hip); one wrapper each picks the family from the geometry.
_K4S2 = {2: "conv2d_k4s2", 3: "conv_k4s2"}


def _k4s2_geom(t, nd=None):
    """(N, C, spatial extents, batch stride) of ``[N, C, H, W]``, ``[N, C, 1, H, W]`` (the view a 2-D HipNet hands out) or
    ``[N, C, D, H, W]``.  ``nd`` None, for an input: a 4-D tensor or D == 1 is 2-D, which is unambiguous because the 3-D entry
    points refuse an odd D.  An output-side tensor passes its input's ``nd``: the 3-D output of D == 2 has D == 1."""
    N, C, D, H, W, _, bs = _geom(t.unsqueeze(2) if t.dim() == 4 else t)
    if nd is None:
        nd = 2 if D == 1 else 3
    if nd == 2 and D != 1:
        raise RuntimeError(f"expected a 2-D activation [N,C,H,W] or [N,C,1,H,W], got {tuple(t.shape)} (MIS_ERR_ARG)")
    return N, C, (D, H, W)[3 - nd:], bs


def _k4s2_in(x, logits):
    """Geometry of the two-part input of a kernel-4 / stride-2 convolution: (N, spatial, x_bs, Cx, l_bs, Cl)."""
    geo = None
    xbs = lbs = Cx = Cl = 0
    if logits is not None:
        N, Cl, sp, lbs = _k4s2_geom(logits)
        geo = (N, sp)
    if x is not None:
        N, Cx, sp, xbs = _k4s2_geom(x)
        if geo is not None and geo != (N, sp):
            raise RuntimeError(f"{_K4S2[len(sp)]}: {tuple(x.shape)} and {tuple(logits.shape)} do not belong together "
                               "(MIS_ERR_ARG)")
        geo = (N, sp)
    if geo is None:
        raise RuntimeError("conv_k4s2: no input (MIS_ERR_ARG)")
    return (*geo, xbs, Cx, lbs, Cl)


def _k4s2_out(t, N, spatial, what):
    """(channels, (tensor, batch stride)) of an output-side tensor of a kernel-4 / stride-2 convolution of that input; ``t`` None
    (where the entry point takes NULL): (0, (NULL, 0))."""
    if t is None:
        return 0, (None, 0)
    No, Co, so, bs = _k4s2_geom(t, len(spatial))
    if (No, tuple(2 * e for e in so)) != (N, spatial):
        raise RuntimeError(f"{_K4S2[len(spatial)]}: {what} {tuple(t.shape)} does not belong to an input of {(N, *spatial)} "
                           "(MIS_ERR_ARG)")
    return Co, (t, bs)


def conv_k4s2_fwd(x, logits, w_x, w_l, bias, bias2, y, slope=0.2, drop_scale=None):
    """y = drop(leaky_relu(bias + bias2 + Conv{2,3}d(k=4, s=2, p=1)(cat(softmax(logits), x)), slope)).  ``logits`` / ``w_l``: the
    channels read through a softmax and their filter (None: none); ``x`` / ``w_x``: the plain ones (None: none)."""
    N, sp, xbs, Cx, lbs, Cl = _k4s2_in(x, logits)
    Cout, y_v = _k4s2_out(y, N, sp, "y")
    taps, entry = 4 ** len(sp), "mis_" + _K4S2[len(sp)]
    assert (w_x is None or (w_x.is_contiguous() and w_x.numel() == Cout * Cx * taps))
    assert (w_l is None or (w_l.is_contiguous() and w_l.numel() == Cout * Cl * taps))
    ws = _ws("k4s2", entry + "_fwd_workspace_bytes", N, Cx + Cl, Cout, *sp)
    _l.launch(entry + "_fwd", x, xbs, Cx, logits, lbs, Cl, w_x, w_l, bias, bias2, y_v, N, Cout, *sp, float(slope), drop_scale,
              ws)


def conv_k4s2_dgrad(dy, y, w, dx, slope=0.2, drop_scale=None):
    """dx = the gradient at the input of the convolution with filter ``w`` [Cout, Cin, (4,) 4, 4] for the gradient ``dy`` at its
    activated output ``y`` (None: the plain convolution's gradient)."""
    N, Cin, sp, dxbs = _k4s2_geom(dx)
    Cout, dy_v = _k4s2_out(dy, N, sp, "dy")
    y_v = _k4s2_out(y, N, sp, "y")[1]
    assert w.is_contiguous() and w.numel() == Cout * Cin * 4 ** len(sp)
    _l.launch("mis_" + _K4S2[len(sp)] + "_dgrad", dy_v, y_v, float(slope), drop_scale, w, dx, dxbs, N, Cin, Cout, *sp)


def conv_k4s2_wgrad(x, logits, dy, y, dw_x, dw_l, dbias=None, dbias2=None, slope=0.2, drop_scale=None, accumulate=False):
    """dw_l / dw_x (+)= the filter gradient in the two parts of conv_k4s2_fwd's input, dbias / dbias2 (+)= the bias gradient;
    deterministic."""
    N, sp, xbs, Cx, lbs, Cl = _k4s2_in(x, logits)
    Cout, dy_v = _k4s2_out(dy, N, sp, "dy")
    y_v = _k4s2_out(y, N, sp, "y")[1]
    taps, entry = 4 ** len(sp), "mis_" + _K4S2[len(sp)]
    assert (dw_x is None or (dw_x.is_contiguous() and dw_x.numel() == Cout * Cx * taps))
    assert (dw_l is None or (dw_l.is_contiguous() and dw_l.numel() == Cout * Cl * taps))
    ws = _ws("k4s2", entry + "_wgrad_workspace_bytes", N, Cx + Cl, Cout, *sp)
    _l.launch(entry + "_wgrad", x, xbs, Cx, logits, lbs, Cl, dy_v, y_v, float(slope), drop_scale, dw_x, dw_l, dbias, dbias2, N,
              Cout, *sp, int(accumulate), ws)


# The head's family is its window's: ``pool`` of two is AvgPool2d in floor mode (any number of windows, flattened), ``pool`` of
# three or None is AvgPool3d over the whole feature, the one window the 3-D entry points take.
def adv_head_workspace(N, C, K, H=None, W=None, pool=None):
    """The buffer adv_head_fwd leaves the pooled features and d loss / d logits in for adv_head_bwd; the 2-D head's depends on
    the feature's extent ``H``, ``W`` and the ``pool`` of two."""
    if pool is None:
        nb = _l.query("mis_adv_head_workspace_bytes", N, C, K)
    else:
        nb = _l.query("mis_adv_head2d_workspace_bytes", N, C, K, H, W, int(pool[0]), int(pool[1]))
    return torch.empty(nb // 4, dtype=torch.float32, device="cuda")


def adv_head_fwd(a, w, b, target, loss, logits, ws, pool=None):
    """loss[0] = cross_entropy(Linear(flatten(avg_pool(a))), target), logits [N, K]; ``pool`` defaults to the 3-D feature's
    extent."""
    nd = 2 if pool is not None and len(pool) == 2 else 3
    N, C, ext, abs_ = _k4s2_geom(a, nd)
    pool = ext if pool is None else tuple(int(p) for p in pool)
    K = w.shape[0]
    F = C * (ext[0] // pool[0]) * (ext[1] // pool[1]) if nd == 2 else C
    assert w.is_contiguous() and w.numel() == K * F and target.dtype == torch.int32 and target.numel() == N
    assert logits.is_contiguous() and logits.numel() == N * K
    _l.require_gpu(w, target, loss, logits, ws)
    _l.launch("mis_adv_head2d_fwd" if nd == 2 else "mis_adv_head_fwd", a, abs_, w, b, target, loss, logits, N, C, K, *ext, *pool,
              ws, ws.numel() * 4)


def adv_head_bwd(w, da, dw, db, ws, pool=None, shape=None, accumulate=False):
    """da (None: not wanted; then ``shape`` = the feature's (N, C, extents...)), dw [K, F], db [K] (+)= the head's gradients;
    under a ``pool`` of two da is zero in the rows and columns the floor-mode windows leave out."""
    nd = 2 if pool is not None and len(pool) == 2 else 3
    if da is None:
        (N, C, *ext), da_v = shape, (None, 0)
    else:
        N, C, ext, dabs = _k4s2_geom(da, nd)
        da_v = (da, dabs)
    K = w.shape[0]
    win = (int(pool[0]), int(pool[1])) if nd == 2 else ()
    _l.launch("mis_adv_head2d_bwd" if nd == 2 else "mis_adv_head_bwd", w, da_v, dw, db, int(accumulate), N, C, K, *ext, *win, ws,
              ws.numel() * 4)


# the 2-D names: the same functions
conv2d_k4s2_fwd, conv2d_k4s2_dgrad, conv2d_k4s2_wgrad = conv_k4s2_fwd, conv_k4s2_dgrad, conv_k4s2_wgrad
adv_head2d_workspace, adv_head2d_fwd, adv_head2d_bwd = adv_head_workspace, adv_head_fwd, adv_head_bwd


def adversarial_tail(logits, label, labeled_bs, dmap, cons_loss, out, dlogits=None, cons_weight=0.0, state=None,
                     loss_scale=1.0):
    """0.5 * (CE + Dice) on the labeled samples + w * cons_loss; dlogits: the supervised gradient on the labeled samples,
    w * (softmax Jacobian)^T dmap on the unlabeled ones.  ``out`` (>= 5 + C floats): [loss, loss_ce, loss_dice,
    consistency_loss, consistency_weight, class-wise dice...]."""
    B, C, D, H, W, S, sbs = _geom(logits)
    mbs = 0
    if dmap is not None:
        Bm, Cm, _, _, _, Sm, mbs = _geom(dmap)
        assert Bm == B - labeled_bs and Cm == C and Sm == S
    ws = _ws("tail", "mis_adversarial_tail_workspace_bytes", B, C, S)
    _l.launch("mis_adversarial_tail", logits, sbs, _label(label, labeled_bs * S, optional=True), dmap, mbs, cons_loss, B,
              labeled_bs, C, S, cons_weight, state, loss_scale, out, _view(dlogits), ws)


def adam_init(adam_state, step=0):
    """Set the device-resident step count of an Adam state (a 16-byte buffer)."""
    _l.require_gpu(adam_state)
    assert adam_state.numel() * adam_state.element_size() >= ADAM_STATE_BYTES
    _l.launch("mis_adam_init", adam_state, int(step))


def adam_step(param, grad, m, v, adam_state, lr, betas=(0.9, 0.999), eps=1e-8):
    """One torch.optim.Adam step (no weight decay) on flat fp32 buffers; the step count advances on the device."""
    _l.require_gpu(param, grad, m, v, adam_state)
    n = param.numel()
    assert grad.numel() == n and m.numel() == n and v.numel() == n
    _l.launch("mis_adam_step", param, grad, m, v, n, float(lr), float(betas[0]), float(betas[1]), float(eps), adam_state)
