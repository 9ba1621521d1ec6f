"""The dilated 3x3 convolution kernels (csrc/conv_dilated.hip: forward, data gradient, weight gradient) against the float64
oracle of tests/dilated_oracle.py, in units of fp32 noise -- the rule of tests/test_conv_edges_gpu.py, unchanged:

    err_hip <= max(K * e32, FLOOR[kind]),    K = 6

per tensor and per measure of conv_oracle.measure (max: the worst channel's largest error over that channel's largest
reference value; rms: over the whole tensor); e32 = torch's fp32 CPU result on the same bits against float64, FLOOR = the
largest e32 of the matrix per kind (dilated_oracle.FLOOR, recomputed by tests/test_pnet_cpu.py).  A channel whose reference is
exactly zero must be exactly zero.

Every output is pre-filled with NaN and must come back finite, every case asserts the kernel that served each tensor (the
*_kernel_name entry points), every weight gradient is also accumulated onto a non-zero dw and run twice (bit-identical).
``slices-d4`` is PNet's concat layout: x a channel slice of a wider buffer with NaN around it, y and dx slices with a sentinel
around them, which must survive.

Measured on an MI355X (this file's own run; ``MIS_DILATED_STATS=<file>`` writes every figure as JSON).  ratio = HIP / max(e32,
FLOOR / K): the error in units of fp32 noise, the gate is at 6.  16 cases + 2, all pass, 4 s wall.

    kernel (as the library names it)                       kind e32 (max measure)    HIP max   ratio  HIP rms   ratio  worst case (max measure)
    conv_dilated_fwd_kernel<DCfg<2, 16, 16, 16, 8, 4>>     y    6.2e-08 .. 6.2e-08  6.50e-08  0.33  2.45e-08  0.12  narrow-d2/relu_scaled
    conv_dilated_fwd_kernel<DCfg<2, 16, 16, 16, 8, 4>>     dx   1.6e-07 .. 4.7e-07  2.93e-07  1.38  1.60e-07  1.34  narrow-d2/relu_scaled
    conv_dilated_fwd_kernel<DCfg<2, 16, 16, 32, 8, 4>>     y    5.5e-07 .. 5.5e-07  3.99e-07  0.73  4.62e-08  0.23  even-d2/relu_scaled
    conv_dilated_fwd_kernel<DCfg<2, 16, 32, 32, 8, 8>>     y    2.9e-07 .. 2.9e-07  3.64e-07  1.27  6.22e-08  0.31  wide-d2/relu_scaled
    conv_dilated_fwd_kernel<DCfg<2, 16, 32, 16, 8, 8>>     dx   4.7e-07 .. 4.7e-07  6.82e-07  1.46  3.08e-07  1.51  wide-d2/relu_scaled
    conv_dilated_fwd_kernel<DCfg<4, 16, 16, 32, 8, 4>>     y    2.4e-07 .. 5.6e-07  5.82e-07  1.03  1.41e-07  0.70  ragged-d4/offset
    conv_dilated_fwd_kernel<DCfg<4, 16, 16, 16, 8, 4>>     y    2.9e-07 .. 2.9e-07  2.27e-07  0.79  4.72e-08  0.24  slices-d4/relu_scaled
    conv_dilated_fwd_kernel<DCfg<4, 16, 16, 16, 8, 4>>     dx   1.7e-07 .. 4.6e-07  3.64e-07  2.17  1.42e-07  1.41  ragged-d4/uniform
    conv_dilated_fwd_kernel<DCfg<8, 16, 16, 32, 8, 4>>     y    3.6e-07 .. 3.6e-07  2.68e-07  0.74  8.51e-08  0.43  small-phase-d8/relu_scaled
    conv_dilated_fwd_kernel<DCfg<8, 16, 16, 32, 8, 4>>     dx   5.3e-07 .. 5.3e-07  2.94e-07  0.55  1.33e-07  0.66  small-phase-d8/relu_scaled
    conv_dilated_fwd_kernel<DCfg<16, 16, 16, 32, 8, 4>>    y    3.6e-07 .. 1.2e-06  4.45e-07  0.65  1.25e-07  0.58  few-px-d16/relu_scaled
    conv_dilated_fwd_kernel<DCfg<16, 16, 16, 32, 8, 4>>    dx   3.4e-07 .. 4.6e-07  3.11e-07  0.83  1.28e-07  0.77  few-px-d16/offset
    conv_dilated_fwd_kernel<DCfg<16, 16, 16, 16, 8, 4>>    y    5.6e-08 .. 1.8e-07  1.83e-07  0.91  4.19e-08  0.21  odd-d16/relu_scaled
    conv_dilated_fwd_kernel<DCfg<16, 16, 16, 16, 8, 4>>    dx   8.1e-08 .. 2.2e-07  3.69e-07  1.65  1.28e-07  1.11  odd-d16/relu_scaled
    conv_dilated_fwd_kernel<DCfg<16, 16, 32, 16, 4, 8>>    y    1.8e-07 .. 1.8e-07  1.09e-07  0.54  2.25e-08  0.11  wide-d16/relu_scaled
    conv_dilated_fwd_kernel<DCfg<16, 16, 32, 16, 4, 8>>    dx   1.3e-07 .. 1.3e-07  2.72e-07  2.16  1.14e-07  1.26  wide-d16/relu_scaled
    conv_dilated_wgrad_kernel<DWCfg<2, 16, 16>>            dw   2.2e-07 .. 2.6e-07  2.12e-07  0.67  7.83e-08  0.25  narrow-d2/relu_scaled dw+=
    conv_dilated_wgrad_kernel<DWCfg<2, 8, 32>>             dw   6.4e-07 .. 1.8e-06  3.78e-07  0.57  1.25e-07  0.38  wide-d2/relu_scaled dw+=
    conv_dilated_wgrad_kernel<DWCfg<4, 8, 32>>             dw   2.5e-07 .. 1.1e-06  5.44e-07  0.88  1.56e-07  0.49  ragged-d4/offset dw+=
    conv_dilated_wgrad_kernel<DWCfg<8, 8, 32>>             dw   1.7e-06 .. 1.7e-06  2.87e-07  0.17  1.33e-07  0.21  small-phase-d8/relu_scaled
    conv_dilated_wgrad_kernel<DWCfg<16, 8, 32>>            dw   4.3e-07 .. 1.4e-06  5.24e-07  0.54  1.22e-07  0.38  few-px-d16/uniform dw+=
    conv_dilated_wgrad_kernel<DWCfg<16, 16, 16>>           dw   2.3e-07 .. 2.8e-07  3.20e-07  1.01  9.93e-08  0.31  below-d-d16/relu_scaled dw+=

    Every tensor is within 2.2 x fp32 noise; no entry is over the gate (OVER_THE_GATE is empty).  The highest ratios are data
    gradients onto few channels (8 .. 16 products per tap), where torch's own fp32 error is at 1e-7 and the floor decides.
"""
import ctypes
import functools

import pytest
import torch

import conv_oracle as co
import dilated_oracle as do
import oracle_kit as kit
from oracle_kit import NAN

pytestmark = pytest.mark.gpu

K, FLOOR = do.K, do.FLOOR
# A tensor over the gate is a finding, named here with its measured ratio: {case: {(kind, measure)}}.  Strict: the case xfails
# only when exactly these entries are over the gate.
OVER_THE_GATE = {}
LEAD, TRAIL = 1, 2            # channels of the wider buffer before / after a slice
_in, _out = functools.partial(kit.place, lead=LEAD, trail=TRAIL), functools.partial(kit.Out, lead=LEAD, trail=TRAIL)
STATS = []        # (case, label, kind, measure, e32, hip, kernel)


def _f(d, ty, tx, cob, cib, nt):
    return f"conv_dilated_fwd_kernel<DCfg<{d}, {ty}, {tx}, {cob}, {cib}, {nt}>>"


def _w(d, ty, tx):
    return f"conv_dilated_wgrad_kernel<DWCfg<{d}, {ty}, {tx}>>"


# the kernel that serves each tensor of a case: (y, dx, dw)
SERVED = {
    "even-d2": (_f(2, 16, 16, 32, 8, 4), _f(2, 16, 16, 16, 8, 4), _w(2, 8, 32)),
    "ragged-d4": (_f(4, 16, 16, 32, 8, 4), _f(4, 16, 16, 16, 8, 4), _w(4, 8, 32)),
    "small-phase-d8": (_f(8, 16, 16, 32, 8, 4), _f(8, 16, 16, 32, 8, 4), _w(8, 8, 32)),
    "few-px-d16": (_f(16, 16, 16, 32, 8, 4), _f(16, 16, 16, 32, 8, 4), _w(16, 8, 32)),
    "below-d-d16": (_f(16, 16, 16, 16, 8, 4), _f(16, 16, 16, 16, 8, 4), _w(16, 16, 16)),
    "odd-d16": (_f(16, 16, 16, 16, 8, 4), _f(16, 16, 16, 16, 8, 4), _w(16, 16, 16)),
    "slices-d4": (_f(4, 16, 16, 16, 8, 4), _f(4, 16, 16, 16, 8, 4), _w(4, 8, 32)),
    "wide-d16": (_f(16, 16, 32, 16, 4, 8), _f(16, 16, 32, 16, 4, 8), _w(16, 8, 32)),
    "wide-d2": (_f(2, 16, 32, 32, 8, 8), _f(2, 16, 32, 16, 8, 8), _w(2, 8, 32)),
    "narrow-d2": (_f(2, 16, 16, 16, 8, 4), _f(2, 16, 16, 16, 8, 4), _w(2, 16, 16)),
}


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
                                               for cid, label, kind, m, e32, ehip, kernel in STATS):
        print(f"\n[dilated] {kernel:56s} {kind:2s} {m:3s} e32 {r['lo']:.1e} .. {r['hi']:.1e}  hip max {r['hip']:.2e}  "
              f"worst hip/max(e32, floor/K) {r['ratio']:.2f} ({r['at']})", end="")
    print()
    kit.report(STATS, "MIS_DILATED_STATS", {"stats": STATS})


class _Check:
    def __init__(self, name):
        self.name = name
        self.c = do.case(name)
        self.r64, self.r32, self.e32 = do.references(name)
        self.gate = kit.Gate(K, FLOOR, OVER_THE_GATE, STATS)

    def __call__(self, kind, got, kernel, label="", ref=None, e32=None):
        e32 = self.e32[kind] if e32 is None else e32
        self.gate.tensor(self.name, label or kind, kind, got, self.r64[kind] if ref is None else ref,
                         lambda g, r: co.measure(g, r, co.dim_of(self.c, kind)), {ms: e32[ms] for ms in co.MEASURES},
                         (self.name,), (kernel,), width=5)

    def done(self):
        self.gate.done(self.name)


@pytest.mark.parametrize("name", do.names())
def test_forward_data_gradient_weight_gradient(name):
    ops = _ops()
    chk = _Check(name)
    c = chk.c
    N, Cin, Cout, _, H, W = c["shape"]
    d, lay = c["dil"], c["layout"]
    ky, kdx, kdw = SERVED[c["id"]]
    assert ops.conv_dilated_fwd_kernel_name(N, Cin, Cout, H, W, d) == ky
    assert ops.conv_dilated_dgrad_kernel_name(N, Cin, Cout, H, W, d) == kdx
    assert ops.conv_dilated_wgrad_kernel_name(N, Cin, Cout, H, W, d) == kdw
    xv, dyv = _in(c["x"], lay), _in(c["dy"], lay)
    wd, bd = c["w"].cuda(), c["b"].cuda()
    keep, ops.DISPATCH = ops.DISPATCH, set()
    try:
        y = _out((N, Cout, 1, H, W), lay)
        ops.conv_dilated_fwd(xv, ops.conv_pack(wd, 0), bd, y.v, d)
        chk("y", y.v, ky)
        assert y.untouched()
        dx = _out((N, Cin, 1, H, W), lay)
        ops.conv_dilated_fwd(dyv, ops.conv_pack(wd, 1), None, dx.v, d, dgrad=True)
        chk("dx", dx.v, kdx)
        assert dx.untouched()
        dw = torch.full(tuple(c["w"].shape), NAN, device="cuda")
        ops.conv_dilated_wgrad(xv, dyv, dw, d)
        chk("dw", dw, kdw)
        again = torch.full(tuple(c["w"].shape), NAN, device="cuda")
        ops.conv_dilated_wgrad(xv, dyv, again, d)
        assert torch.equal(dw, again), (name, "the weight gradient is not run-to-run bit-identical")
        assert ops.DISPATCH == {f"dilated_wgrad:d{d}@{W}"}
        # accumulated onto a non-zero dw (e32: fp32 torch's dw added in fp32)
        r64 = chk.r64["dw"]
        d0 = r64.flip(1).float()                 # the output channels keep their own scale
        acc = d0.clone().cuda()
        ops.conv_dilated_wgrad(xv, dyv, acc, d, accumulate=True)
        e32 = co.measure((d0 + chk.r32["dw"].float()).double(), r64 + d0.double(), 0)
        chk("dw", acc, kdw, "dw+=", ref=r64 + d0.double(), e32=e32)
    finally:
        ops.DISPATCH = keep
    chk.done()


def test_tap_rows_in_the_padding_add_exact_zeros():
    """H < d: the rows y - d and y + d of every output row lie in the padding, so y is the centre tap row's convolution and the
    filter's outer rows get an exactly zero gradient."""
    ops = _ops()
    c = do.case("below-d-d16/relu_scaled")
    N, Cin, Cout, _, H, W = c["shape"]
    d = c["dil"]
    xv, dyv, wd, bd = c["x"].cuda(), c["dy"].cuda(), c["w"].cuda(), c["b"].cuda()
    w2 = wd.clone()
    w2[:, :, :, 0] = wd[:, :, :, 2] * 3.0 + 1.0
    w2[:, :, :, 2] = -wd[:, :, :, 0]
    ys = []
    for wt in (wd, w2):
        y = torch.full((N, Cout, 1, H, W), NAN, device="cuda")
        ops.conv_dilated_fwd(xv, ops.conv_pack(wt, 0), bd, y, d)
        ys.append(y)
    assert torch.isfinite(ys[0]).all() and torch.equal(ys[0], ys[1])
    dw = torch.full(tuple(wd.shape), NAN, device="cuda")
    ops.conv_dilated_wgrad(xv, dyv, dw, d)
    assert (dw[:, :, :, 0] == 0).all() and (dw[:, :, :, 2] == 0).all() and (dw[:, :, :, 1].abs() > 0).any()


def test_unserved_geometry_is_refused_not_launched():
    """An image beyond the 32-bit buffer descriptors, a dilation outside {2, 4, 8, 16}: MIS_ERR_UNSUPPORTED from the argument
    checks of every entry point.  The pointers are those of small live tensors; nothing is launched."""
    L = _lib()
    from mis_hip import lib
    t = torch.zeros(1024, device="cuda")
    p = ctypes.c_void_p(t.data_ptr())
    buf = ctypes.create_string_buffer(128)
    big = (1, 64, 64, 16384, 16384)            # (64 + 32) * 2^28 * 4 bytes >= 2^30
    S = big[3] * big[4]
    for geom, d in ((big, 2), (big, 16), ((1, 8, 8, 16, 16), 1), ((1, 8, 8, 16, 16), 3), ((1, 8, 8, 16, 16), 32)):
        N, Cin, Cout, H, W = geom
        bs = max(Cin, Cout) * H * W
        assert L.mis_conv_dilated_wgrad_workspace_bytes(N, Cin, Cout, H, W, d) == -2
        assert L.mis_conv_dilated_fwd_kernel_name(N, Cin, Cout, H, W, d, buf, 128) == -2
        assert L.mis_conv_dilated_dgrad_kernel_name(N, Cin, Cout, H, W, d, buf, 128) == -2
        assert L.mis_conv_dilated_wgrad_kernel_name(N, Cin, Cout, H, W, d, buf, 128) == -2
        assert L.mis_conv_dilated_fwd(p, bs, p, None, p, bs, N, Cin, Cout, H, W, d, lib.stream_ptr()) == -2
        assert L.mis_conv_dilated_dgrad(p, bs, p, p, bs, N, Cin, Cout, H, W, d, lib.stream_ptr()) == -2
        assert L.mis_conv_dilated_wgrad(p, bs, p, bs, p, p, 4096, N, Cin, Cout, H, W, d, 0, lib.stream_ptr()) == -2
    assert S * 96 * 4 >= 1 << 30
    torch.cuda.synchronize()
    assert (t == 0).all()
