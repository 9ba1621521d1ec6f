"""float64 reference of the dilated 3x3 convolution kernels (csrc/conv_dilated.hip) and the case matrix of
tests/test_conv_dilated_gpu.py.

CPU only, pure torch, built on tests/conv_oracle.py: the same input classes (``conv_oracle.make_x``), the same measures
(``conv_oracle.measure``), the same tensor layout ([N, C, 1, H, W], filter [Cout, Cin, 1, 3, 3]).  Every case exists three times:

  reference64(c)   y, dx, dw through ``F.conv2d(dilation=d, padding=d)`` in float64 and autograd;
  plain64(c)       the same as a sum over the nine taps of shifted slices, einsum over the channels -- no convolution operator
                   (tests/test_pnet_cpu.py holds the two forms to each other at 1e-12);
  reference32(c)   the same through torch's float32 CPU operators on one thread.  Its distance to reference64 is ``e32``, the
                   yardstick of the GPU test's rule  err_hip <= max(K * e32, FLOOR[kind]),  K = 6.

FLOOR = the largest e32 of the matrix per kind of tensor (either measure), rounded up to two digits (``conv_oracle.ceil2``);
tests/test_pnet_cpu.py recomputes it.

The matrix holds the smallest shapes at which the kernels' two address maps (phase rows, haloed dense columns) can be wrong.
"""
import functools

import torch
import torch.nn.functional as F

import conv_oracle as co
from oracle_kit import one_thread

F64, F32 = torch.float64, torch.float32
KINDS, MEASURES = co.KINDS, co.MEASURES
K = 6.0
FLOOR = {"y": 1.2e-6,       # largest e32 of the matrix: 1.16e-6 (few-px-d16/offset, max: 64 x 9 products of a mean-4 input)
         "dx": 5.4e-7,      # 5.32e-7 (small-phase-d8/relu_scaled, max)
         "dw": 1.9e-6}      # 1.80e-6 (even-d2/relu_scaled, max: torch's fp32 sum over 2 x 32 x 32 pixels)

ALL3 = ("relu_scaled", "uniform", "offset")
ONE = ("relu_scaled",)
SPECS = {}


def _spec(cid, shape, d, classes=ONE, layout="dense"):
    """shape = (N, Cin, Cout, H, W)."""
    N, Cin, Cout, H, W = shape
    SPECS[cid] = dict(group="dilated", op="conv", shape=(N, Cin, Cout, 1, H, W), k=(1, 3, 3), dil=d, classes=classes,
                      kinds=KINDS, layout=layout)


_spec("even-d2", (2, 16, 32, 32, 32), 2)                 # phases of exactly one tile
_spec("ragged-d4", (1, 10, 20, 37, 50), 4, ALL3)         # H, W no multiples of d or of the tile; Cin % 4, Cout % 16 != 0
_spec("small-phase-d8", (1, 64, 64, 56, 56), 8)          # 7 rows per phase, full PNet width
_spec("few-px-d16", (2, 64, 64, 32, 48), 16, ALL3)       # 2 rows per phase
_spec("below-d-d16", (1, 8, 8, 8, 24), 16)               # H < d: only the centre row of taps lands inside
_spec("odd-d16", (3, 8, 8, 40, 24), 16)                  # the PNet golden's geometry
_spec("slices-d4", (2, 16, 16, 24, 40), 4, layout="slice")     # PNet's concat layout: every operand a channel slice
# beside the issue's matrix: the paths it does not reach -- the 16 x 32 forward tiles of W >= 128 (at d = 16 with chunks of 4
# channels), two chunks of input channels on them, and the 16 x 16 weight-gradient tiles of W < 32 below d = 16
_spec("wide-d16", (1, 8, 16, 20, 136), 16)
_spec("wide-d2", (1, 12, 32, 18, 130), 2)
_spec("narrow-d2", (1, 4, 16, 9, 12), 2)


def names():
    return [f"{cid}/{cls}" for cid, s in SPECS.items() for cls in s["classes"]]


@functools.lru_cache(maxsize=None)
def case(name):
    cid, cls = name.split("/")
    return co.make_case(cid, SPECS[cid], cls)


def reference_torch(c, dtype):
    d = c["dil"]
    x = c["x"].to(dtype, copy=True).requires_grad_(True)
    w = c["w"].to(dtype, copy=True).requires_grad_(True)
    y = F.conv2d(x[:, :, 0], w[:, :, 0], c["b"].to(dtype), dilation=d, padding=d).unsqueeze(2)
    y.backward(c["dy"].to(dtype))
    return {"y": y.detach().double(), "dx": x.grad.double(), "dw": w.grad.double()}


def reference64(c):
    return reference_torch(c, F64)


def reference32(c):
    return one_thread(reference_torch, c, F32)


def plain64(c):
    """y, dx, dw in float64 as sums over the nine taps: tap (a, e) reads x shifted by ((a - 1) d, (e - 1) d), dx reads the
    gradient shifted the other way."""
    x, w, b, dy = c["x"].double(), c["w"].double(), c["b"].double(), c["dy"].double()
    d = c["dil"]
    N, _, _, H, W = x.shape
    y = b.reshape(1, -1, 1, 1, 1).expand(N, -1, 1, H, W).clone()
    dx, dw = torch.zeros_like(x), torch.zeros_like(w)
    xp, gp = F.pad(x, (d, d, d, d)), F.pad(dy, (d, d, d, d))
    for a in range(3):
        for e in range(3):
            xs = xp[:, :, :, a * d:a * d + H, e * d:e * d + W]
            gs = gp[:, :, :, (2 - a) * d:(2 - a) * d + H, (2 - e) * d:(2 - e) * d + W]
            y += torch.einsum("oc,ncdhw->nodhw", w[:, :, 0, a, e], xs)
            dw[:, :, 0, a, e] = torch.einsum("nodhw,ncdhw->oc", dy, xs)
            dx += torch.einsum("oc,nodhw->ncdhw", w[:, :, 0, a, e], gs)
    return {"y": y, "dx": dx, "dw": dw}


@functools.lru_cache(maxsize=None)
def references(name):
    """(float64 reference, reference32, e32 = {kind: {measure: value}}) of a matrix case.  Computed once, never modified."""
    c = case(name)
    r64, r32 = reference64(c), reference32(c)
    return r64, r32, {k: co.measure(r32[k], r64[k], co.dim_of(c, k)) for k in KINDS}
