"""The adversarial kernels (csrc/adversarial.hip) against the float64 oracle of tests/adversarial_oracle.py, in units of fp32
noise -- the rule of tests/test_conv_edges_gpu.py, unchanged:

    err_hip <= max(K * e32, FLOOR[kind]),    K = 6

per tensor and per measure of conv_oracle.measure (max: the worst channel's largest error over that channel's largest
reference value; rms: over the whole tensor); e32 = torch's fp32 CPU result (one thread) on the same bits against float64,
FLOOR = the largest e32 of the matrix per kind (adversarial_oracle.FLOOR, recomputed by tests/test_adversarial_cpu.py).  The
head, the tail and Adam are held to the same rule with their own e32 and the floor of the kind they end in (y for
activations, losses and logits, dx for data gradients, dw for parameter gradients and parameters).

Every output is pre-filled with NaN and must come back finite; every kernel runs twice and must give identical bits.  The
chains (ndf = 64 at 16^3, ndf = 8 at 96^3) are held to the oracle evaluated with the activation decisions and dropout masks
the HIP forward produced, and those decisions may differ from the float64 forward's only inside the margin
(adversarial_oracle.MARGIN of a channel's largest pre-activation; at most UNDECIDED_CAP of the elements lie inside it).

Measured on an MI355X (this file's own run; ``MIS_ADVERSARIAL_STATS=<file>`` writes every figure as JSON).  ratio = HIP /
max(e32, FLOOR / K): the error in units of fp32 noise, the gate is at 6.  55 cases, all pass, 10 s wall.

    group  tensor               e32 (max measure)     HIP max   ratio  HIP rms   ratio  worst case (max measure)
    conv   db                   0.0e+00 .. 2.0e-07  3.09e-07  2.42  2.44e-07  2.03  cube-1-4/relu_scaled
    conv   dw                   2.0e-08 .. 7.1e-07  6.34e-07  1.00  1.41e-07  1.04  thin/relu_scaled
    conv   dw+=                 1.0e-08 .. 5.1e-07  3.59e-07  1.00  9.10e-08  0.76  sliced/uniform
    conv   dx                   3.5e-08 .. 3.5e-06  3.87e-06  4.98  8.99e-07  2.19  wide-n3/uniform
    conv   y                    4.7e-08 .. 2.0e-06  1.55e-06  1.43  2.44e-07  0.64  cube-3-8/uniform
    act    act db               7.2e-08 .. 2.1e-07  1.09e-07  0.92  1.19e-07  1.01  act:ragged/relu_scaled
    act    act dw               1.9e-07 .. 4.2e-07  3.30e-07  1.00  1.40e-07  0.76  act:sliced/uniform
    act    act dx               1.4e-07 .. 1.4e-06  2.40e-06  4.62  5.67e-07  1.29  act:wide-n3/uniform
    act    act y                5.3e-07 .. 2.1e-06  1.71e-06  0.81  2.45e-07  0.62  act:sliced/uniform
    first  db0                  1.5e-07 .. 3.1e-07  1.07e-07  0.66  1.09e-07  0.57  first:(2, 4, 1, 64, 2, 12, 4)
    first  db1                  1.5e-07 .. 3.1e-07  1.07e-07  0.66  1.09e-07  0.57  first:(2, 4, 1, 64, 2, 12, 4)
    first  dmap                 1.3e-07 .. 3.5e-07  5.84e-07  2.03  2.70e-07  1.08  first:(1, 3, 2, 20, 12, 12, 12)
    first  dw0                  1.9e-07 .. 5.9e-07  2.73e-07  1.39  1.52e-07  0.81  first:(2, 4, 1, 64, 2, 12, 4)
    first  dw1                  2.0e-07 .. 5.9e-07  2.57e-07  0.99  1.30e-07  0.82  first:(2, 4, 1, 64, 2, 12, 4)
    first  y                    3.4e-07 .. 3.9e-07  5.11e-07  1.46  1.97e-07  0.56  first:(1, 3, 2, 20, 12, 12, 12)
    head   head da              1.4e-07 .. 5.6e-05  8.06e-05  2.22  1.09e-07  0.43  head:2x64x(1, 1, 1)
    head   head db              1.4e-09 .. 2.6e-07  6.43e-07  5.43  4.54e-07  3.84  head:3x20x(2, 3, 1)
    head   head dw              6.5e-08 .. 2.2e-07  1.77e-07  1.50  1.20e-07  1.01  head:1x37x(3, 5, 7)
    head   head logits          3.5e-08 .. 6.3e-07  2.36e-07  0.38  5.81e-08  0.17  head:3x20x(2, 3, 1)
    head   head loss            1.2e-08 .. 1.9e-07  2.04e-07  0.58  2.04e-07  0.58  head:1x37x(3, 5, 7)
    tail   tail dlogits         1.3e-07 .. 1.9e-07  1.57e-07  0.63  7.20e-08  0.29  tail:4,2,2,(4, 6, 10),0.0
    tail   tail out             1.7e-08 .. 7.3e-08  4.51e-08  0.13  4.59e-08  0.13  tail:3,1,3,(2, 3, 5),0.1
    adam   adam step+0          1.3e-04 .. 1.4e-03  1.38e-03  1.00  2.69e-04  1.00  adam:1,1
    adam   adam step+1          7.8e-05 .. 1.1e-03  1.15e-03  1.00  2.42e-04  1.00  adam:1,1
    chain  chain act0           7.2e-07 .. 8.8e-07  9.52e-07  1.08  2.63e-07  0.75  chain:8@96
    chain  chain act1           1.2e-06 .. 1.4e-06  1.47e-06  1.19  5.04e-07  1.29  chain:8@96
    chain  chain act2           1.6e-06 .. 2.7e-06  2.09e-06  1.28  6.70e-07  0.99  chain:8@96
    chain  chain act3           2.1e-06 .. 1.1e-05  3.86e-05  3.52  6.84e-07  0.89  chain:64@16
    chain  chain dclassifier.bias 1.8e-07 .. 1.2e-06  1.54e-06  1.97  1.54e-06  1.74  chain:8@96
    chain  chain dclassifier.weight 2.0e-07 .. 7.7e-07  8.43e-07  1.09  6.81e-07  1.22  chain:8@96
    chain  chain dconv0.bias    8.1e-07 .. 3.0e-06  1.03e-06  1.28  1.09e-06  1.27  chain:64@16
    chain  chain dconv0.weight  1.6e-06 .. 3.2e-05  3.95e-06  1.35  9.96e-07  1.26  chain:64@16
    chain  chain dconv1.bias    8.1e-07 .. 3.0e-06  1.03e-06  1.28  1.09e-06  1.27  chain:64@16
    chain  chain dconv1.weight  1.6e-06 .. 2.5e-05  4.87e-06  1.00  8.71e-07  1.13  chain:64@16
    chain  chain dconv2.bias    4.7e-07 .. 6.2e-07  8.92e-07  1.44  8.45e-07  1.46  chain:64@16
    chain  chain dconv2.weight  1.3e-06 .. 1.9e-06  2.59e-06  1.37  8.04e-07  1.28  chain:64@16
    chain  chain dconv3.bias    6.0e-07 .. 9.6e-07  6.78e-07  1.13  5.49e-07  1.17  chain:64@16
    chain  chain dconv3.weight  1.9e-06 .. 3.1e-06  2.86e-06  1.03  6.35e-07  1.03  chain:64@16
    chain  chain dconv4.bias    4.3e-07 .. 6.8e-06  4.14e-07  0.97  5.78e-07  1.39  chain:64@16
    chain  chain dconv4.weight  1.2e-06 .. 1.5e-05  2.91e-05  1.93  5.59e-07  0.99  chain:64@16
    chain  chain dmap           4.3e-07 .. 6.5e-07  9.44e-07  1.58  9.01e-07  1.37  chain:8@96
    chain  chain logits         5.5e-07 .. 7.7e-07  6.89e-07  1.05  4.74e-07  1.28  chain:8@96
    chain  chain loss           5.5e-08 .. 3.4e-07  3.38e-07  0.97  3.38e-07  0.97  chain:8@96

    Every tensor is within 5.4 x fp32 noise; no entry is over the gate (OVER_THE_GATE is empty).  The highest ratios are the
    head's bias gradient (a sum of N <= 4 numbers that nearly cancel: 6e-7 absolute against a floor of 7.1e-7) and data gradients
    onto few channels, where torch's own fp32 error is at 1e-7 and the floor decides.  The Adam rows measure the UPDATE
    (parameter - initial parameter): both fp32 evaluations round the parameter itself, which is 1e-3 of an update of 1e-4.
"""
import functools

import pytest
import torch

import adversarial_oracle as ao
import oracle_kit as kit
from oracle_kit import NAN, nan as _nan, one_thread as _one_thread

pytestmark = pytest.mark.gpu

K, FLOOR = ao.K, ao.FLOOR
# A tensor over the gate is a finding, named here with its measured ratio: {case: {(label, measure)}}.
OVER_THE_GATE = {}
LEAD, TRAIL = 1, 2            # channels of the wider buffer before / after a slice
_in, _out = functools.partial(kit.place, lead=LEAD, trail=TRAIL), functools.partial(kit.Out, lead=LEAD, trail=TRAIL)
_checker = functools.partial(ao.Check, floor=FLOOR, over_the_gate=OVER_THE_GATE)      # rows go to ao.STATS
STATS = ao.STATS   # (case, label, kind, measure, e32, hip); tests/test_adversarial_gpu.py adds its golden's rows
F64 = torch.float64


def _ops():
    from mis_hip import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if STATS:
        ao.print_report("adversarial", STATS, FLOOR)
        kit.report(STATS, "MIS_ADVERSARIAL_STATS", {"stats": STATS})


# ---------------------------------------------------------------------------------------------------------------------
# the convolution alone: y, dx, dw, dw accumulated, db
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ao.names())
def test_conv_forward_data_gradient_weight_gradient(name):
    ops = _ops()
    chk = _checker(name)
    c = ao.case(name)
    r64, r32, _ = ao.references(name)
    N, Cin, Cout, D, H, W = c["shape"]
    lay = c["layout"]
    osh = (N, Cout, D // 2, H // 2, W // 2)
    xv, dyv = _in(c["x"], lay), _in(c["dy"], lay)
    wd, bd = c["w"].cuda(), c["b"].cuda()
    ys = []
    for _ in range(2):
        y = _out(osh, lay)
        ops.conv_k4s2_fwd(xv, None, wd, None, bd, None, y.v, slope=1.0)
        assert y.untouched()
        ys.append(y.v)
    chk("y", "y", ys[0], r64["y"], r32["y"])
    assert torch.equal(ys[0], ys[1]), (name, "the forward is not run-to-run bit-identical")
    dxs = []
    for _ in range(2):
        dx = _out((N, Cin, D, H, W), lay)
        ops.conv_k4s2_dgrad(dyv, None, wd, dx.v, slope=1.0)
        assert dx.untouched()
        dxs.append(dx.v)
    chk("dx", "dx", dxs[0], r64["dx"], r32["dx"])
    assert torch.equal(dxs[0], dxs[1]), (name, "the data gradient is not run-to-run bit-identical")
    dws, dbs = [], []
    for _ in range(2):
        dw, db = _nan(*c["w"].shape), _nan(Cout)
        ops.conv_k4s2_wgrad(xv, None, dyv, None, dw, None, dbias=db, slope=1.0)
        dws.append(dw)
        dbs.append(db)
    chk("dw", "dw", dws[0], r64["dw"], r32["dw"], 0)
    db64 = c["dy"].double().sum((0, 2, 3, 4))
    chk("db", "dw", dbs[0], db64, _one_thread(lambda: c["dy"].sum((0, 2, 3, 4))))
    assert torch.equal(dws[0], dws[1]) and torch.equal(dbs[0], dbs[1]), (name, "the weight gradient is not bit-identical")
    # accumulated onto a non-zero dw (e32: fp32 torch's dw added in fp32)
    d0 = r64["dw"].flip(1).float()
    acc = d0.clone().cuda()
    ops.conv_k4s2_wgrad(xv, None, dyv, None, acc, None, slope=1.0, accumulate=True)
    chk("dw+=", "dw", acc, r64["dw"] + d0.double(), d0 + r32["dw"].float(), 0)
    chk.done()


def _scale_pattern(N, C):
    """Dropout3d scales [N, C]: 0 or 2, both values in every sample (C > 1), channel 0 dropped in every sample."""
    n = torch.arange(N).reshape(N, 1)
    c = torch.arange(C).reshape(1, C)
    s = (((n * 3 + c * 5) % 7) % 2 == 1).float() * 2.0
    s[:, 0] = 0.0
    if C > 1:
        s[:, 1] = 2.0
    return s


@pytest.mark.parametrize("name", ["cube-3-8/uniform", "ragged/relu_scaled", "wide-n3/uniform", "sliced/uniform"])
def test_activation_and_dropout_epilogue(name):
    """LeakyReLU(0.2) + channel dropout in the forward's epilogue, and their derivative recovered from the stored output in
    both gradients.  The decisions are compared where the float64 pre-activation is outside the margin; the values are
    held to the oracle evaluated on the decisions the kernel took."""
    ops = _ops()
    chk = _checker("act:" + name)
    c = ao.case(name)
    r64, r32, _ = ao.references(name)
    N, Cin, Cout, D, H, W = c["shape"]
    scale = _scale_pattern(N, Cout)
    xv, dyv, wd, bd, sd = c["x"].cuda(), c["dy"].cuda(), c["w"].cuda(), c["b"].cuda(), scale.cuda()
    y = _nan(N, Cout, D // 2, H // 2, W // 2)
    ops.conv_k4s2_fwd(xv, None, wd, None, bd, None, y, slope=ao.SLOPE, drop_scale=sd)
    yc = y.cpu()
    kept = (scale > 0).reshape(N, Cout, 1, 1, 1).expand_as(yc)
    assert (yc[~kept] == 0).all(), "a dropped (n, c) volume is not exactly zero"
    pre64 = r64["y"]
    dec = ao.decided(pre64)
    assert 1.0 - dec.double().mean().item() <= ao.UNDECIDED_CAP
    signs = yc > 0
    assert torch.equal(signs[kept & dec], (pre64 > 0)[kept & dec]), "an activation decision outside the margin differs"
    signs = torch.where(kept, signs, pre64 > 0)           # a dropped volume keeps no decision; its gradient is zero anyway
    chk("act y", "y", y, ao.act_drop(pre64, ao.SLOPE, scale, signs), ao.act_drop(r32["y"].float(), ao.SLOPE, scale, signs))

    def back(dtype):
        x = c["x"].to(dtype).requires_grad_(True)
        w = c["w"].to(dtype).requires_grad_(True)
        b = c["b"].to(dtype).requires_grad_(True)
        ao.act_drop(ao.conv(x, w, b), ao.SLOPE, scale, signs).backward(c["dy"].to(dtype))
        return x.grad, w.grad, b.grad
    g64, g32 = back(F64), _one_thread(lambda: back(torch.float32))
    dx, dw, db = _nan(N, Cin, D, H, W), _nan(*c["w"].shape), _nan(Cout)
    ops.conv_k4s2_dgrad(dyv, y, wd, dx, slope=ao.SLOPE, drop_scale=sd)
    ops.conv_k4s2_wgrad(xv, None, dyv, y, dw, None, dbias=db, slope=ao.SLOPE, drop_scale=sd)
    chk("act dx", "dx", dx, g64[0], g32[0])
    chk("act dw", "dw", dw, g64[1], g32[1], 0)
    chk("act db", "dw", db, g64[2], g32[2])
    assert (dw[0] == 0).all() and db[0] == 0, "channel 0 is dropped in every sample: its gradients are exactly zero"
    chk.done()


@pytest.mark.parametrize("shape", [(3, 2, 1, 8, 4, 6, 10), (1, 3, 2, 20, 12, 12, 12), (2, 4, 1, 64, 2, 12, 4)])
def test_first_layer_reads_softmax_of_logits(shape):
    """conv0(softmax(logits)) + conv1(image) as one convolution: forward, the two filter gradients and the two bias gradients
    written separately, and the gradient at the softmax output."""
    ops = _ops()
    N, Cl, Cx, Cout, D, H, W = shape
    chk = _checker(f"first:{shape}")
    g = torch.Generator().manual_seed(sum(shape))
    lg = (torch.randn(N, Cl, D, H, W, generator=g, dtype=F64) * 2).float()
    im = torch.randn(N, Cx, D, H, W, generator=g, dtype=F64).float()
    w0 = ((torch.rand(Cout, Cl, 4, 4, 4, generator=g, dtype=F64) * 2 - 1) * 0.2).float()
    w1 = ((torch.rand(Cout, Cx, 4, 4, 4, generator=g, dtype=F64) * 2 - 1) * 0.2).float()
    b0, b1 = [(torch.rand(Cout, generator=g, dtype=F64) * 2 - 1).float() for _ in range(2)]
    dy = torch.randn(N, Cout, D // 2, H // 2, W // 2, generator=g, dtype=F64).float()

    def ref(dtype):
        p = torch.softmax(lg.to(dtype), 1).requires_grad_(True)
        ws = [t.to(dtype).requires_grad_(True) for t in (w0, w1, b0, b1)]
        y = ao.conv(p, ws[0], ws[2]) + ao.conv(im.to(dtype), ws[1], ws[3])
        y.backward(dy.to(dtype))
        return [y.detach(), p.grad] + [t.grad for t in ws]
    r64, r32 = ref(F64), _one_thread(lambda: ref(torch.float32))
    lgd, imd, dyd = lg.cuda(), im.cuda(), dy.cuda()
    y = _nan(*dy.shape)
    ops.conv_k4s2_fwd(imd, lgd, w1.cuda(), w0.cuda(), b1.cuda(), b0.cuda(), y, slope=1.0)
    chk("y", "y", y, r64[0], r32[0])
    dmap = _nan(N, Cl, D, H, W)
    ops.conv_k4s2_dgrad(dyd, None, w0.cuda(), dmap, slope=1.0)
    chk("dmap", "dx", dmap, r64[1], r32[1])
    outs = []
    for _ in range(2):
        dw0, dw1, db0, db1 = _nan(*w0.shape), _nan(*w1.shape), _nan(Cout), _nan(Cout)
        ops.conv_k4s2_wgrad(imd, lgd, dyd, None, dw1, dw0, dbias=db1, dbias2=db0, slope=1.0)
        outs.append((dw0, dw1, db0, db1))
    for label, got, i in (("dw0", outs[0][0], 2), ("dw1", outs[0][1], 3), ("db0", outs[0][2], 4), ("db1", outs[0][3], 5)):
        chk(label, "dw", got, r64[i], r32[i], 0)
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    chk.done()


# ---------------------------------------------------------------------------------------------------------------------
# dropout decision, head, tail, Adam
# ---------------------------------------------------------------------------------------------------------------------
def _state(seed=7, it=3):
    from mis_hip import lib
    st = torch.zeros(lib.STEP_STATE_BYTES, dtype=torch.uint8, device="cuda")
    L = lib.load()
    lib.check(L.mis_step_init(lib.ptr(st), seed, it, 0.01, 30000.0, 0.99, 0.1, 40.0, 150, 0, 0, lib.stream_ptr()), "mis_step_init")
    return st


def test_channel_dropout_scale_is_a_bernoulli_draw_per_channel_from_the_step_state():
    ops = _ops()
    s = [_nan(64, 512) for _ in range(3)]
    ops.channel_dropout_scale(s[0], 0.5, 0x80000001, _state(7, 3))
    ops.channel_dropout_scale(s[1], 0.5, 0x80000001, _state(7, 3))
    ops.channel_dropout_scale(s[2], 0.5, 0x80000001, _state(7, 4))
    assert torch.equal(s[0], s[1]) and not torch.equal(s[0], s[2])
    assert ((s[0] == 0) | (s[0] == 2)).all()
    assert abs((s[0] == 0).float().mean().item() - 0.5) < 0.02          # 32768 draws: sigma = 0.0028


HEAD_CASES = [(1, 4, (1, 1, 1)), (3, 20, (2, 3, 1)), (2, 64, (1, 1, 1)), (4, 512, (6, 6, 6)), (1, 37, (3, 5, 7))]


@pytest.mark.parametrize("N,C,ext", HEAD_CASES)
def test_head_pool_linear_cross_entropy(N, C, ext):
    ops = _ops()
    chk = _checker(f"head:{N}x{C}x{ext}")
    g = torch.Generator().manual_seed(N * 1000 + C)
    a = torch.randn(N, C, *ext, generator=g, dtype=F64).float()
    w = (torch.randn(2, C, generator=g, dtype=F64) / C ** 0.5).float()
    b = torch.randn(2, generator=g, dtype=F64).float()
    target = (torch.arange(N) < (N + 1) // 2).int()
    r64, r32 = ao.head(a, w, b, target), _one_thread(lambda: ao.head(a, w, b, target, torch.float32))
    outs = []
    for _ in range(2):
        ws = ops.adv_head_workspace(N, C, 2)
        loss, logits, da, dw, db = _nan(1), _nan(N, 2), _nan(N, C, *ext), _nan(2, C), _nan(2)
        ops.adv_head_fwd(a.cuda(), w.cuda(), b.cuda(), target.cuda(), loss, logits, ws, ext)
        ops.adv_head_bwd(w.cuda(), da, dw, db, ws)
        outs.append((loss, logits, da, dw, db))
    for i, (label, kind) in enumerate((("loss", "y"), ("logits", "y"), ("da", "dx"), ("dw", "dw"), ("db", "dw"))):
        key = label
        chk("head " + label, kind, outs[0][i], r64[key].reshape(outs[0][i].shape), r32[key].reshape(outs[0][i].shape),
            0 if label in ("logits", "dw") else 1)
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    from mis_hip import lib
    L = lib.load()
    p = lib.ptr(outs[0][2])
    assert L.mis_adv_head_fwd(p, C * ext[0] * ext[1] * ext[2], p, p, p, p, p, N, C, 2, *ext, ext[0] + 1, ext[1], ext[2], p, 1 << 20,
                              lib.stream_ptr()) == -2, "a pool window that is not the feature's extent is refused"
    chk.done()


TAIL_CASES = [(2, 1, 2, (3, 5, 7), 0.1), (4, 2, 2, (8, 8, 8), 0.05), (3, 1, 3, (2, 3, 5), 0.1), (3, 2, 4, (4, 4, 6), 1.0),
              (4, 2, 2, (4, 6, 10), 0.0)]


@pytest.mark.parametrize("B,L,C,ext,w", TAIL_CASES)
def test_adversarial_tail(B, L, C, ext, w):
    ops = _ops()
    chk = _checker(f"tail:{B},{L},{C},{ext},{w}")
    g = torch.Generator().manual_seed(B * 100 + L * 10 + C)
    lg = (torch.randn(B, C, *ext, generator=g, dtype=F64) * 2).float()
    lab = torch.randint(0, C, (B,) + ext, generator=g).to(torch.uint8)
    dmap = (torch.randn(B - L, C, *ext, generator=g, dtype=F64) * 1e-3).float()
    cons = torch.tensor([0.6931], dtype=torch.float32)
    o64, g64 = ao.tail(lg, lab, L, dmap, cons.item(), w)
    o32, g32 = _one_thread(lambda: ao.tail(lg, lab, L, dmap, cons.item(), w, dtype=torch.float32))
    outs = []
    for labd in (lab.cuda(), lab.long().cuda()):
        out, dl = _nan(5 + C), _nan(B, C, *ext)
        ops.adversarial_tail(lg.cuda(), labd, L, dmap.cuda(), cons.cuda(), out, dl, cons_weight=w)
        outs.append((out, dl))
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    chk("tail out", "y", outs[0][0], o64, o32)
    if w == 0.0:
        assert (outs[0][1][L:] == 0).all(), "consistency weight 0: the unlabeled samples get an exactly zero gradient"
    chk("tail dlogits", "dx", outs[0][1], g64, g32)
    chk.done()


@pytest.mark.parametrize("n", [1, 255, 4097])
@pytest.mark.parametrize("first", [1, 1000])
def test_adam_step(n, first):
    """Steps ``first`` and ``first + 1`` (1 and 2: the fresh state; 1000: the bias correction far along)."""
    ops = _ops()
    chk = _checker(f"adam:{n},{first}")
    g = torch.Generator().manual_seed(n + first)
    p0 = torch.randn(n, generator=g, dtype=F64).float()
    grads = [(torch.randn(n, generator=g, dtype=F64) * 10.0 ** (-2 * i)).float() for i in range(2)]
    r64 = ao.adam(p0, grads, 1e-4, first_step=first)
    r32 = _one_thread(lambda: ao.adam(p0, grads, 1e-4, dtype=torch.float32, first_step=first))
    runs = []
    for _ in range(2):
        p, m, v = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        st = torch.zeros(2, dtype=torch.int64, device="cuda")
        ops.adam_init(st, first - 1)
        after = []
        for gr in grads:
            ops.adam_step(p, gr.cuda(), m, v, st, 1e-4, (0.9, 0.99), 1e-8)
            after.append(p.clone())
        assert st.cpu()[0].item() == first + 1
        runs.append(after)
    for i in range(2):
        # the update is what is tested: the parameter itself hides it below its own rounding
        chk(f"adam step+{i}", "dw", runs[0][i].cpu().double() - p0.double(), r64[i] - p0.double(), r32[i].double() - p0.double())
        assert torch.equal(runs[0][i], runs[1][i])
    chk.done()


def test_adam_with_an_all_zero_gradient_leaves_the_parameters_unchanged():
    ops = _ops()
    for n in (1, 255, 4097):
        p0 = torch.randn(n, device="cuda")
        p, m, v = p0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        st = torch.zeros(2, dtype=torch.int64, device="cuda")
        ops.adam_init(st, 0)
        for _ in range(2):
            ops.adam_step(p, torch.zeros(n, device="cuda"), m, v, st, 1e-4, (0.9, 0.99), 1e-8)
        assert torch.equal(p, p0) and (m == 0).all() and (v == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the whole chain
# ---------------------------------------------------------------------------------------------------------------------
def _chain_inputs(N, C, size, ndf, seed):
    g = torch.Generator().manual_seed(seed)
    if size == 96:
        vol, lg, _ = ao.golden_inputs(N, C, size)
    else:
        vol = torch.randn(N, 1, size, size, size, generator=g, dtype=F64).float()
        lg = (torch.randn(N, C, size, size, size, generator=g, dtype=F64) * 2).float()
    sd = {}
    for key, shape in ao.disc_shapes(C, ndf, 1).items():
        fan_in = 1
        for s in shape[1:]:
            fan_in *= s
        # He-like amplitudes keep the activations of all five layers at order one; the biases move the decisions off zero
        sd[key] = (torch.randn(shape, generator=g, dtype=F64) * (1.6 / max(fan_in, 4) ** 0.5 if len(shape) > 1 else 0.1)).float()
    return vol, lg, sd


@pytest.mark.parametrize("ndf,size,pool", [(64, 16, (1, 1, 1)), (8, 96, (6, 6, 6))])
def test_whole_chain_against_the_oracle_on_the_decisions_it_took(ndf, size, pool):
    from networks.discriminator import FC3DDiscriminator
    N, C = 3 if size == 16 else 2, 2
    chk = _checker(f"chain:{ndf}@{size}")
    vol, lg, sd = _chain_inputs(N, C, size, ndf, ndf + size)
    masks = ao.golden_masks(ndf, N)
    target = (torch.arange(N) < (N + 1) // 2).int()
    dan = FC3DDiscriminator(C, ndf, 1, pool=pool)
    dan.load_state_dict(sd)
    dan.train()
    dan.drop_masks = [m.float().cuda() for m in masks]
    lgd, vold, td = lg.cuda(), vol.cuda(), target.cuda()
    runs = []
    for _ in range(2):
        for _, gv in dan.named_flat(dan.flat_grad):      # the padding words between the parameters stay zero
            gv.fill_(NAN)
        dan.loss_forward(lgd, vold, td)
        dan.loss_backward(params=True, dmap=True)
        runs.append([dan.loss_buffer().clone(), dan.logits_buffer().clone(), dan.dmap_buffer().clone(), dan.flat_grad.clone()]
                    + [a.clone() for a in dan.activations()])
    assert all(torch.equal(x, y) for x, y in zip(*runs)), "the chain is not run-to-run bit-identical"
    acts = [a.cpu() for a in runs[0][4:]]
    probs = torch.softmax(lg.double(), 1)
    free = ao.disc_step(sd, probs, vol, target, masks, pool)                 # the float64 forward's own decisions
    signs, kept = [], []
    for i, (a, pre) in enumerate(zip(acts, free["pres"])):
        kept.append((masks[i] > 0).reshape(N, -1, 1, 1, 1).expand_as(a) if i < 3 else torch.ones_like(a, dtype=torch.bool))
        signs.append(torch.where(kept[i], a > 0, pre > 0))     # a dropped volume keeps no decision; its gradient is zero anyway
    r64 = ao.disc_step(sd, probs, vol, target, masks, pool, signs=signs)
    r32 = _one_thread(lambda: ao.disc_step(sd, probs, vol, target, masks, pool, signs=signs, dtype=torch.float32))
    # the decisions differ from the float64 forward's only inside the margin (of the forward they belong to: r64's)
    for i, pre in enumerate(r64["pres"]):
        live = ao.decided(pre) & kept[i]
        assert torch.equal(signs[i][live], (pre > 0)[live]), f"layer {i}: a decision outside the margin differs"
        assert (acts[i][~kept[i]] == 0).all(), f"layer {i}: a dropped volume is not exactly zero"
    chk("chain loss", "y", runs[0][0], r64["loss"], r32["loss"])
    chk("chain logits", "y", runs[0][1], r64["logits"], r32["logits"], 0)
    for i in range(4):
        chk(f"chain act{i}", "y", acts[i], r64["acts"][i], r32["acts"][i])
    chk("chain dmap", "dx", runs[0][2], r64["dmap"], r32["dmap"])
    for key, gview in dan.named_flat(runs[0][3]):
        chk("chain d" + key, "dw", gview, r64["grads"][key], r32["grads"][key], 0)
    chk.done()
