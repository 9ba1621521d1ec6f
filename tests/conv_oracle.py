"""float64 reference of the convolution kernels (csrc/conv_fwd.hip, conv_wino*.hip, conv_wgrad*.hip, conv_k2s2.hip,
conv1x1_gemm.hip, pack.hip) and the case matrix of tests/test_conv_edges_gpu.py.

CPU only, pure torch.  Every case exists four times:

  reference64(c)   y, dx, dw through torch's float64 convolution and autograd;
  plain64(c)       the same as a sum over the filter taps of shifted slices, einsum over the channels -- no convolution
                   operator, so that tests/test_conv_oracle_cpu.py can hold the two forms to each other;
  reference32(c)   the same through torch's float32 CPU operators (one thread: the summation order, and with it the last
                   digits, would follow the thread count).  Its distance to reference64 is ``e32``, the yardstick;
  winograd32(c)    a plain fp32 F(2, 3) per axis (F(2x2, 3x3) / F(2x2x2, 3x3x3)) of the k = 3 cases: filter transform in
                   double, rounded once; input and output transforms and the contraction (BLAS) in fp32.  It states what the
                   ALGORITHM costs in fp32 -- no boxes, no LDS layout, no contraction slices.  With dtype=float64 it is
                   exact and is held to reference64.

Tensors are [N, C, D, H, W] (2-D: D == 1, filter [.., .., 1, k, k]).  A case ``c`` is a dict of CPU fp32 tensors and
settings made by ``case(id)``; inputs are generated in float64 from a seed derived from the id and rounded to fp32 once.

Input classes (x): uniform U(-1, 1); relu max(N(0,1), 0); relu_scaled the same times a per-channel 10^-U(0,3); offset
4 + N(0,1).  Gradient classes (dy): uniform; scaled N(0,1) times a per-channel 10^-U(0,3).  Weights U(-0.2, 0.2), bias U(-1, 1).

measure(got, ref64, dim) gives two figures per tensor: ``max`` = the largest |error| of a channel over that channel's largest
|reference|, worst channel (channel = ``dim``: 1 for y and dx, the OUTPUT channel's dimension for dw), and ``rms`` =
rms(error) / rms(reference); plus ``zero_ok``: a channel whose reference is exactly zero is exactly zero in ``got``.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

from oracle_kit import ceil2, one_thread          # noqa: F401  (ceil2 re-exported: other files round their floors with it)

F64, F32 = torch.float64, torch.float32
KINDS = ("y", "dx", "dw")
MEASURES = ("max", "rms")
X_CLASSES = ("uniform", "relu", "relu_scaled", "offset")
DY_CLASSES = ("uniform", "scaled")
DY_OF = {"uniform": "uniform", "relu": "scaled", "relu_scaled": "scaled", "offset": "scaled"}     # the dy class an x class runs with


# ---------------------------------------------------------------------------------------------------------------------
# measures
# ---------------------------------------------------------------------------------------------------------------------
def measure(got, ref, dim=1):
    got, ref = got.detach().double().reshape(ref.shape), ref.double()
    other = [d for d in range(ref.dim()) if d != dim]
    err = (got - ref).abs()
    cmax = ref.abs().amax(other)
    live = cmax > 0
    zero_ok = bool((got.abs().amax(other)[~live] == 0).all())
    emax = (err.amax(other)[live] / cmax[live]).max().item() if live.any() else 0.0
    rms = ref.pow(2).mean().sqrt().item()
    return {"max": emax, "rms": err.pow(2).mean().sqrt().item() / rms if rms > 0 else 0.0, "zero_ok": zero_ok}


def dw_dim(c):
    """The dimension of the output channel in the parameter (ConvTranspose: [Cin, Cout, ...])."""
    return 1 if c["op"] == "up" else 0


def dim_of(c, kind):
    return dw_dim(c) if kind == "dw" else 1


# ---------------------------------------------------------------------------------------------------------------------
# the operation in torch (float64 / float32) and as a plain sum over the taps
# ---------------------------------------------------------------------------------------------------------------------
def _torch_op(c, x, w, b):
    k = c["k"]
    if c["op"] == "conv":
        if k[0] == 1 and x.shape[2] == 1:            # Conv2d
            return F.conv2d(x[:, :, 0], w[:, :, 0], b, padding=(k[1] // 2, k[2] // 2)).unsqueeze(2)
        return F.conv3d(x, w, b, padding=tuple(v // 2 for v in k))
    if c["op"] == "down":
        return F.conv3d(x, w, b, stride=2)
    if k[0] == 1:                                    # ConvTranspose2d
        return F.conv_transpose2d(x[:, :, 0], w[:, :, 0], b, stride=2).unsqueeze(2)
    return F.conv_transpose3d(x, w, b, stride=2)


def reference_torch(c, dtype):
    x = c["x"].to(dtype, copy=True).requires_grad_(True)          # copies: the case's own tensors stay plain leaves
    w = c["w"].to(dtype, copy=True).requires_grad_(True)
    y = _torch_op(c, x, w, c["b"].to(dtype))
    y.backward(c["dy"].to(dtype))
    return {"y": y.detach().double(), "dx": x.grad.double(), "dw": w.grad.double()}


def reference64(c):
    return reference_torch(c, F64)


def reference32(c):
    return one_thread(reference_torch, c, F32)


def _taps(k):
    return [(a, b, d) for a in range(k[0]) for b in range(k[1]) for d in range(k[2])]


def plain64(c, kinds=KINDS):
    """y, dx, dw (those of ``kinds``) in float64 without a convolution operator."""
    x, w, b, dy = c["x"].double(), c["w"].double(), c["b"].double(), c["dy"].double()
    k = c["k"]
    N, _, D, H, W = x.shape
    op = c["op"]
    y = b.reshape(1, -1, 1, 1, 1).expand(N, -1, *dy.shape[2:]).clone()
    dx, dw = torch.zeros_like(x), torch.zeros_like(w)
    p = [v // 2 for v in k]
    xp = F.pad(x, (p[2], p[2], p[1], p[1], p[0], p[0]))
    gp = F.pad(dy, (p[2], p[2], p[1], p[1], p[0], p[0]))
    for a, e, d in _taps(k):
        if op == "conv":              # 'same': tap (a, e, d) reads x shifted by the tap, dx the gradient shifted the other way
            xs = xp[:, :, a:a + D, e:e + H, d:d + W]
            gs = gp[:, :, k[0] - 1 - a:k[0] - 1 - a + D, k[1] - 1 - e:k[1] - 1 - e + H, k[2] - 1 - d:k[2] - 1 - d + W]
            yv, dxv, ein = y, dx, ("oc,ncdhw->nodhw", "nodhw,ncdhw->oc", "oc,nodhw->ncdhw")
        elif op == "down":            # stride 2: tap = the position inside a 2 x 2 x 2 window of x
            xs, gs = x[:, :, a::2, e::2, d::2], dy
            yv, dxv, ein = y, dx[:, :, a::2, e::2, d::2], ("oc,ncdhw->nodhw", "nodhw,ncdhw->oc", "oc,nodhw->ncdhw")
        else:                         # transposed: tap = the position inside a window of y; the parameter is [Cin, Cout, ...]
            xs, gs = x, dy[:, :, a::k[0], e::k[1], d::k[2]]
            yv, dxv, ein = y[:, :, a::k[0], e::k[1], d::k[2]], dx, ("co,ncdhw->nodhw", "nodhw,ncdhw->co", "co,nodhw->ncdhw")
        if "y" in kinds:
            yv += torch.einsum(ein[0], w[:, :, a, e, d], xs)
        if "dw" in kinds:
            dw[:, :, a, e, d] = torch.einsum(ein[1], gs if op == "up" else dy, xs)
        if "dx" in kinds:
            dxv += torch.einsum(ein[2], w[:, :, a, e, d], gs)
    return {kk: v for kk, v in (("y", y), ("dx", dx), ("dw", dw)) if kk in kinds}


# ---------------------------------------------------------------------------------------------------------------------
# plain Winograd F(2, 3) per axis
# ---------------------------------------------------------------------------------------------------------------------
def _bt(t, ax):
    """B^T d = (d0 - d2, d1 + d2, d2 - d1, d1 - d3): the 4 inputs of a tile."""
    d0, d1, d2, d3 = t.unbind(ax)
    return torch.stack((d0 - d2, d1 + d2, d2 - d1, d1 - d3), ax)


def _at(t, ax):
    """A^T m = (m0 + m1 + m2, m1 - m2 - m3): the 2 outputs of a tile."""
    m0, m1, m2, m3 = t.unbind(ax)
    return torch.stack((m0 + m1 + m2, m1 - m2 - m3), ax)


def _a(t, ax):
    """A y = (y0, y0 + y1, y0 - y1, -y1)."""
    y0, y1 = t.unbind(ax)
    return torch.stack((y0, y0 + y1, y0 - y1, -y1), ax)


def _g(t, ax):
    """G g = (g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2)."""
    g0, g1, g2 = t.unbind(ax)
    return torch.stack((g0, (g0 + g1 + g2) * 0.5, (g0 - g1 + g2) * 0.5, g2), ax)


def _gt(t, ax):
    """G^T m = (m0 + (m1 + m2) / 2, (m1 - m2) / 2, (m1 + m2) / 2 + m3)."""
    m0, m1, m2, m3 = t.unbind(ax)
    return torch.stack((m0 + (m1 + m2) * 0.5, (m1 - m2) * 0.5, (m1 + m2) * 0.5 + m3), ax)


def _input_tiles(x, k):
    """[N, C, tiles, points]: B^T d B of the overlapping 4-wide patches (stride 2) along every axis with k = 3."""
    pad = []
    for ax in (2, 1, 0):
        pad += [k[ax] // 2, k[ax] // 2]
    t = F.pad(x, pad)
    for ax in range(3):
        t = t.unfold(2 + ax, 4, 2) if k[ax] == 3 else t.unfold(2 + ax, 1, 1)
    for ax in range(3):                              # [N, C, tD, tH, tW, pD, pH, pW]
        if k[ax] == 3:
            t = _bt(t, 5 + ax)
    return t.reshape(t.shape[0], t.shape[1], -1, t.shape[5] * t.shape[6] * t.shape[7]), tuple(t.shape[2:5])


def _filter_points(w, k, dtype):
    """[O, C, points]: G g G^T in double, rounded to ``dtype`` once."""
    u = w.double()
    for ax in range(3):
        if k[ax] == 3:
            u = _g(u, 2 + ax)
    return u.reshape(u.shape[0], u.shape[1], -1).to(dtype)


def _wino_conv(x, w, k, dtype):
    N, C = x.shape[:2]
    O = w.shape[0]
    v, tiles = _input_tiles(x.to(dtype), k)                      # [N, C, T, P]
    u = _filter_points(w, k, dtype)                              # [O, C, P]
    T, P = v.shape[2], v.shape[3]
    m = torch.bmm(u.permute(2, 0, 1), v.permute(3, 1, 0, 2).reshape(P, C, N * T))      # [P, O, N * T]
    pts = [4 if k[ax] == 3 else 1 for ax in range(3)]
    m = m.reshape(*pts, O, N, *tiles).permute(4, 3, 5, 6, 7, 0, 1, 2)                   # [N, O, tD, tH, tW, pD, pH, pW]
    for ax in range(3):
        if k[ax] == 3:
            m = _at(m, 5 + ax)
    m = m.permute(0, 1, 2, 5, 3, 6, 4, 7)                        # [N, O, tD, oD, tH, oH, tW, oW]
    return m.reshape(N, O, m.shape[2] * m.shape[3], m.shape[4] * m.shape[5], m.shape[6] * m.shape[7])


def _wino_wgrad(x, dy, k, dtype):
    N, C = x.shape[:2]
    O = dy.shape[1]
    v, tiles = _input_tiles(x.to(dtype), k)                      # [N, C, T, P]
    T, P = v.shape[2], v.shape[3]
    outs = [2 if k[ax] == 3 else 1 for ax in range(3)]
    g = dy.to(dtype).reshape(N, O, tiles[0], outs[0], tiles[1], outs[1], tiles[2], outs[2]).permute(0, 1, 2, 4, 6, 3, 5, 7)
    for ax in range(3):
        if k[ax] == 3:
            g = _a(g, 5 + ax)
    g = g.reshape(N, O, T, P)
    m = torch.bmm(g.permute(3, 1, 0, 2).reshape(P, O, N * T), v.permute(3, 0, 2, 1).reshape(P, N * T, C))       # [P, O, C]
    pts = [4 if k[ax] == 3 else 1 for ax in range(3)]
    m = m.reshape(*pts, O, C).permute(3, 4, 0, 1, 2)
    for ax in range(3):
        if k[ax] == 3:
            m = _gt(m, 2 + ax)
    return m


def winograd_eligible(c):
    k = c["k"]
    return c["op"] == "conv" and 3 in k and all(kk == 1 or (kk == 3 and s % 2 == 0) for kk, s in zip(k, c["shape"][3:]))


def winograd(c, dtype=F32, kinds=KINDS):
    """y, dx, dw (those of ``kinds``) of a k = 3 'same' convolution by F(2, 3) per axis in ``dtype``."""
    assert winograd_eligible(c)
    k = c["k"]
    out = {}
    if "y" in kinds:
        out["y"] = _wino_conv(c["x"], c["w"], k, dtype) + c["b"].to(dtype).reshape(1, -1, 1, 1, 1)
    if "dx" in kinds:
        out["dx"] = _wino_conv(c["dy"], c["w"].flip(2, 3, 4).transpose(0, 1), k, dtype)
    if "dw" in kinds:
        out["dw"] = _wino_wgrad(c["x"], c["dy"], k, dtype)
    return {kk: v.double() for kk, v in out.items()}


def winograd32(c, kinds=KINDS):
    return winograd(c, F32, kinds)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(zlib.crc32(seed.encode()))


def make_x(cls, shape, g):
    C = shape[1]
    rn = torch.randn(shape, generator=g, dtype=F64)
    sc = 10.0 ** (-3.0 * torch.rand(C, generator=g, dtype=F64)).reshape(1, C, 1, 1, 1)
    if cls == "uniform":
        return torch.rand(shape, generator=g, dtype=F64) * 2 - 1
    if cls == "relu":
        return rn.clamp_min(0)
    if cls == "relu_scaled":
        return rn.clamp_min(0) * sc
    if cls == "offset":
        return 4.0 + rn
    if cls == "scaled":
        return rn * sc
    raise KeyError(cls)


def out_shape(spec):
    N, Cin, Cout, D, H, W = spec["shape"]
    if spec["op"] == "conv":
        return (N, Cout, D, H, W)
    if spec["op"] == "down":
        return (N, Cout, D // 2, H // 2, W // 2)
    k = spec["k"]
    return (N, Cout, D * k[0], H * k[1], W * k[2])


def make_case(cid, spec, xcls):
    N, Cin, Cout, D, H, W = spec["shape"]
    k = spec["k"]
    g = _gen(f"{cid}/{xcls}")
    x = make_x(xcls, (N, Cin, D, H, W), g)
    dy = make_x(DY_OF[xcls], out_shape(spec), g)
    wshape = (Cin, Cout) + tuple(k) if spec["op"] == "up" else (Cout, Cin) + tuple(k)
    w = (torch.rand(wshape, generator=g, dtype=F64) * 2 - 1) * 0.2
    b = torch.rand(Cout, generator=g, dtype=F64) * 2 - 1
    return dict(spec, id=cid, xcls=xcls, x=x.float(), dy=dy.float(), w=w.float(), b=b.float())


# ---------------------------------------------------------------------------------------------------------------------
# the case matrix: id -> operation, shape (N, Cin, Cout, D, H, W) of the INPUT, filter, input classes, expected kernels
#   fwd / dgrad: (kernel name, contraction slices)  -- names as mis_conv_fwd_kernel_name / mis_conv3d_wino_kernel_name /
#                mis_conv2d_wino_kernel_name print them;  wgrad: name of mis_conv*_wgrad_kernel_name
# ---------------------------------------------------------------------------------------------------------------------
# The names below are the strings the library's *_kernel_name entry points return, which follow the compiler's own spelling of
# the instantiation (as a profiler prints it: "Cfg<...>>" here, "WgCfg<...> >" there).  A toolchain that spells them differently
# changes those entry points' answers and these tables together; run tests/test_conv_edges_gpu.py::served over SPECS to regenerate.
ALL = X_CLASSES
ONE = ("relu_scaled",)
W3 = {0: "wino_fwd_kernel<WinoCfg<1, 1, 16, 2, 2, 1, 1, 4, 0, 0>, false>", 1: "wino_fwd_kernel<WinoCfg<1, 2, 8, 2, 2, 1, 1, 4, 0, 0>, false>",
      2: "wino_fwd_kernel<WinoCfg<1, 4, 4, 4, 1, 1, 1, 4, 1, 0>, false>", 3: "wino_fwd_kernel<WinoCfg<3, 3, 6, 1, 1, 1, 1, 4, 1, 1>, false>"}
W2 = {0: "wino2d_fwd_kernel<W2Cfg<8, 8, 1, 3>>", 1: "wino2d_fwd_kernel<W2Cfg<8, 8, 2, 3>>", 2: "wino2d_fwd_kernel<W2Cfg<4, 16, 1, 3>>",
      3: "wino2d_fwd_kernel<W2Cfg<4, 16, 2, 3>>"}
WG = {1: "wino_wgrad_kernel<WgCfg<2, 2, 8, 1> >", 2: "wino_wgrad_kernel<WgCfg<4, 2, 4, 0> >", 3: "wino_wgrad_ring_kernel<WrCfg<2, 16, 1> >",
      4: "wino_wgrad_ring_kernel<WrCfg<4, 8, 1> >", 5: "wino_wgrad_flat_kernel<12, 12>", 6: "wino_wgrad_ring3_kernel<Wr3Cfg<4, 12> >"}


def _cfg(*v):
    return "conv_fwd_kernel<Cfg<" + ", ".join(map(str, v)) + ">>"


def _wcfg(*v):
    return "conv_wgrad_kernel<WCfg<" + ", ".join(map(str, v)) + "> >"


K3, K2D, K1 = (3, 3, 3), (1, 3, 3), (1, 1, 1)
SPECS = {}


def _spec(group, cid, op, shape, k, classes=ONE, kinds=KINDS, **kernels):
    assert cid not in SPECS, cid
    SPECS[cid] = dict(group=group, op=op, shape=shape, k=k, classes=classes, kinds=kinds, **kernels)


# forward and data gradient, 3-D (the weight gradient of the same operands rides along)
_spec("fwd3d", "direct-ragged", "conv", (1, 20, 24, 4, 10, 12), K3, ALL, fwd=(_cfg(3, 3, 3, 2, 4, 16, 16, 4, 2), 1),
      dgrad=(_cfg(3, 3, 3, 2, 4, 16, 16, 4, 2), 1), wgrad=_wcfg(3, 3, 3, 2, 12, 8, 1))
_spec("fwd3d", "direct-cin1", "conv", (1, 1, 16, 8, 16, 32), K3, fwd=("conv_fwd_cin1_kernel<3>", 1),
      dgrad=(_cfg(3, 3, 3, 4, 8, 16, 16, 4, 8), 1), wgrad="wgrad_cin1_kernel<3, false>")
_spec("fwd3d", "direct-cout2-k1", "conv", (1, 16, 2, 16, 16, 16), K1, fwd=(_cfg(1, 1, 1, 4, 8, 16, 16, 16, 8), 1),
      dgrad=(_cfg(1, 1, 1, 4, 8, 16, 16, 16, 8), 1), wgrad=_wcfg(1, 1, 1, 2, 8, 16, 1))
_spec("fwd3d", "wino-v0", "conv", (1, 16, 16, 4, 4, 32), K3, ALL, fwd=(W3[0], 1), dgrad=(W3[0], 1), wgrad=WG[3])
_spec("fwd3d", "wino-v1", "conv", (2, 16, 32, 4, 8, 16), K3, fwd=(W3[1], 1), dgrad=(W3[1], 1), wgrad=WG[4])
_spec("fwd3d", "wino-v2", "conv", (1, 32, 32, 8, 8, 8), K3, fwd=(W3[2], 1), dgrad=(W3[2], 1), wgrad=WG[2])
_spec("fwd3d", "wino-v2-partial-boxes", "conv", (8, 32, 64, 12, 8, 20), K3, fwd=(W3[2], 1), dgrad=(W3[2], 2),
      wgrad=_wcfg(3, 3, 3, 4, 8, 8, 1))
_spec("fwd3d", "wino-v3", "conv", (4, 32, 128, 18, 6, 12), K3, fwd=(W3[3], 1), dgrad=(W3[3], 4),
      wgrad=_wcfg(3, 3, 3, 2, 12, 8, 1))
_spec("split", "split2-6", "conv", (8, 128, 256, 6, 6, 6), K3, fwd=(W3[2], 2), dgrad=(W3[2], 4),
      wgrad=_wcfg(3, 3, 3, 2, 6, 8, 1))
_spec("split", "split4-6", "conv", (4, 256, 256, 6, 6, 6), K3, ALL, fwd=(W3[2], 4), dgrad=(W3[2], 4),
      wgrad=_wcfg(3, 3, 3, 2, 6, 8, 1))
_spec("split", "split2-12", "conv", (4, 128, 128, 12, 12, 12), K3, fwd=(W3[3], 2), dgrad=(W3[3], 2), wgrad=WG[5])
# forward and data gradient, 2-D
_spec("fwd2d", "wino2d-v0", "conv", (2, 16, 16, 1, 48, 48), K2D, fwd=(W2[0], 1), dgrad=(W2[0], 1),
      wgrad="wino2d_wgrad_kernel<Wg2Cfg<1, 4, 8> >")
_spec("fwd2d", "wino2d-v1", "conv", (2, 16, 32, 1, 16, 16), K2D, ALL, fwd=(W2[1], 1), dgrad=(W2[0], 1),
      wgrad="wino2d_wgrad_kernel<Wg2Cfg<2, 4, 8> >")
_spec("fwd2d", "wino2d-v2", "conv", (2, 16, 16, 1, 24, 32), K2D, fwd=(W2[2], 1), dgrad=(W2[2], 1),
      wgrad="wino2d_wgrad_kernel<Wg2Cfg<1, 2, 16> >")
_spec("fwd2d", "wino2d-v3", "conv", (2, 16, 32, 1, 64, 64), K2D, fwd=(W2[3], 1), dgrad=(W2[2], 1),
      wgrad="wino2d_wgrad_kernel<Wg2Cfg<2, 2, 16> >")
_spec("fwd2d", "direct2d-cin1", "conv", (2, 1, 16, 1, 32, 32), K2D, fwd=("conv_fwd_cin1_kernel<1>", 1),
      dgrad=("conv_small_cout_kernel", 1), wgrad="wgrad_cin1_kernel<1, false>")
_spec("fwd2d", "direct2d-cout2", "conv", (2, 4, 2, 1, 16, 130), K2D, fwd=("conv_small_cout_kernel", 1),
      dgrad=("conv_small_cout_kernel", 1), wgrad=_wcfg(1, 3, 3, 1, 8, 32, 1))
_spec("fwd2d", "direct2d-4x4-128", "conv", (4, 128, 256, 1, 4, 4), K2D, ALL, fwd=(_cfg(1, 3, 3, 1, 16, 16, 32, 8, 4), 1),
      dgrad=(_cfg(1, 3, 3, 1, 16, 16, 32, 8, 4), 1), wgrad=_wcfg(1, 3, 3, 1, 16, 16, 1))
_spec("fwd2d", "direct2d-4x4-256", "conv", (4, 256, 256, 1, 4, 4), K2D, fwd=(_cfg(1, 3, 3, 1, 16, 16, 32, 8, 4), 1),
      dgrad=(_cfg(1, 3, 3, 1, 16, 16, 32, 8, 4), 1), wgrad=_wcfg(1, 3, 3, 1, 16, 16, 1))
# weight gradient alone
_spec("wgrad", "wgrad-direct2d", "conv", (2, 16, 16, 1, 28, 28), K2D, kinds=("dw",), wgrad=_wcfg(1, 3, 3, 1, 16, 16, 1))
_spec("wgrad", "wgrad-wino-v1", "conv", (1, 16, 16, 4, 4, 16), K3, ALL, kinds=("dw",), wgrad=WG[1])
_spec("wgrad", "wgrad-wino-v2", "conv", (2, 32, 16, 8, 4, 8), K3, kinds=("dw",), wgrad=WG[2])
_spec("wgrad", "wgrad-wino-v3", "conv", (1, 16, 16, 2, 4, 32), K3, kinds=("dw",), wgrad=WG[3])
_spec("wgrad", "wgrad-wino-v4", "conv", (1, 16, 16, 2, 8, 16), K3, kinds=("dw",), wgrad=WG[4])
_spec("wgrad", "wgrad-wino-v5", "conv", (2, 16, 32, 4, 12, 12), K3, kinds=("dw",), wgrad=WG[5])
_spec("wgrad", "wgrad-wino-v6", "conv", (1, 16, 16, 2, 8, 24), K3, kinds=("dw",), wgrad=WG[6])
_spec("wgrad", "wgrad-wino2d", "conv", (1, 16, 16, 1, 8, 16), K2D, kinds=("dw",), wgrad="wino2d_wgrad_kernel<Wg2Cfg<1, 4, 8> >")
_spec("wgrad", "wgrad-long-v3", "conv", (2, 16, 16, 24, 24, 96), K3, kinds=("dw",), wgrad=WG[3])
_spec("wgrad", "wgrad-long-v6", "conv", (8, 64, 64, 24, 24, 24), K3, kinds=("dw",), wgrad=WG[6])
# kernel 2 / stride 2, 1x1 GEMM, 2-D transposed convolution (shape = the op's INPUT)
_spec("k2s2", "k2s2-down", "down", (2, 16, 32, 8, 32, 32), (2, 2, 2), ALL)
_spec("k2s2", "k2s2-down-ragged", "down", (2, 16, 32, 4, 40, 32), (2, 2, 2))
_spec("k2s2", "k2s2-up", "up", (2, 32, 16, 4, 16, 16), (2, 2, 2))
# the 32 <-> 64 templates (a contraction over 256 terms) at a coarse 3 x 18 x 24: ragged 16-voxel tiles, and Wo % 16 != 0 puts the
# weight gradient on its 8 x 2-voxel lane groups
_spec("k2s2", "k2s2-down-32x64", "down", (1, 32, 64, 6, 36, 48), (2, 2, 2))
_spec("k2s2", "k2s2-up-64x32", "up", (1, 64, 32, 3, 18, 24), (2, 2, 2))
_spec("gemm", "gemm1x1-ragged", "conv", (3, 72, 100, 5, 6, 4), K1, ALL)
_spec("gemm", "gemm1x1-splitk", "conv", (8, 1024, 256, 6, 6, 6), K1)
_spec("gemm", "gemm1x1-wide", "conv", (4, 256, 1024, 6, 6, 6), K1)
_spec("up2d", "up2d", "up", (3, 32, 16, 1, 8, 12), (1, 2, 2), ALL)
_spec("up2d", "up2d-4x4", "up", (2, 256, 128, 1, 4, 4), (1, 2, 2))


def spec_of(name):
    """The matrix entry of a case name (``id/class``): what does not need the tensors."""
    return SPECS[name.split("/")[0]]


def names(group=None):
    return [f"{cid}/{cls}" for cid, s in SPECS.items() if group in (None, s["group"]) for cls in s["classes"]]


@functools.lru_cache(maxsize=None)
def case(name):
    cid, cls = name.split("/")
    return make_case(cid, SPECS[cid], cls)


def served_by_winograd(c, kind):
    """Whether the expected kernel of this tensor is a Winograd kernel (then e32 is the larger of reference32's and winograd32's)."""
    if "fwd" not in c and "wgrad" not in c:
        return False
    name = c.get("wgrad") if kind == "dw" else (c.get("fwd" if kind == "y" else "dgrad") or (None,))[0]
    return bool(name) and name.startswith("wino")


@functools.lru_cache(maxsize=None)
def references(name):
    """(float64 reference, e32, winograd32's error or None) of a matrix case; e32 / ew: {kind: {measure: value}}.
    Computed once, never modified."""
    c = case(name)
    r64 = reference64(c)
    r32 = reference32(c)
    e32 = {k: measure(r32[k], r64[k], dim_of(c, k)) for k in KINDS}
    ew = None
    if winograd_eligible(c):
        w32 = winograd32(c, c["kinds"])
        ew = {k: measure(w32[k], r64[k], dim_of(c, k)) for k in c["kinds"]}
    return r64, e32, ew


def yardstick(name, kind, m):
    """The e32 the rule uses for one tensor and measure."""
    c = case(name)
    _, e32, ew = references(name)
    v = e32[kind][m]
    if ew is not None and served_by_winograd(c, kind):
        v = max(v, ew[kind][m])
    return v

