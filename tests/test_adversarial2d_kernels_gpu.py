"""The 2-D adversarial kernels (csrc/adversarial2d.hip) against the float64 oracle of tests/adversarial2d_oracle.py, in units of
fp32 noise -- the rule of tests/test_adversarial_kernels_gpu.py, unchanged:

    err_hip <= max(K * e32, FLOOR[kind]),    K = 6

per tensor and per measure of conv_oracle.measure; e32 = torch's fp32 CPU result (one thread) on the same bits against float64,
FLOOR = the largest e32 of the matrix per kind (adversarial2d_oracle.FLOOR, recomputed by tests/test_adversarial2d_cpu.py).
The head is held to the same rule with its own e32 and the floor of the kind it ends in (y for losses and logits, dx for da,
dw for parameter gradients).

Every output is pre-filled with NaN and must come back finite; every kernel runs twice and must give identical bits.  The
chains (ndf = 8 at 80 x 80 with pool 2, ndf = 64 at 32 x 32 with pool 1) are held to the oracle evaluated with the activation
decisions the HIP forward took, and those decisions may differ from the float64 forward's only inside the margin
(adversarial_oracle.MARGIN of a channel's largest pre-activation; at most UNDECIDED_CAP of the elements lie inside it, which
tests/test_adversarial2d_cpu.py checks for these inputs).

Measured on an MI355X (this file's own run; ``MIS_ADVERSARIAL2D_STATS=<file>`` writes every figure as JSON).  ratio = HIP /
max(e32, FLOOR / K): the error in units of fp32 noise, the gate is at 6.

    group  tensor                  e32 (max measure)     HIP max   ratio  HIP rms   ratio  worst case (max measure)
    act    act db                  7.8e-08 .. 2.5e-07  1.51e-07  0.75  1.51e-07  0.76  act:tiles-vec/relu_scaled
    act    act dw                  2.3e-07 .. 4.9e-07  2.13e-07  0.75  1.93e-07  0.62  act:sliced/uniform
    act    act dx                  1.0e-07 .. 3.3e-07  6.30e-07  2.00  1.95e-07  1.38  act:c20-64/relu_scaled
    act    act y                   1.0e-07 .. 1.2e-06  1.11e-06  1.25  2.65e-07  1.03  act:ragged-20x12/uniform
    chain  chain act0              2.8e-07 .. 3.4e-07  4.65e-07  1.37  1.15e-07  0.49  chain:64@32
    chain  chain act1              9.9e-07 .. 1.6e-06  1.81e-06  1.11  3.04e-07  1.05  chain:64@32
    chain  chain act2              9.3e-07 .. 1.6e-06  1.98e-06  1.27  3.74e-07  1.10  chain:64@32
    chain  chain act3              1.2e-06 .. 2.6e-06  2.26e-06  1.22  4.24e-07  1.04  chain:8@80
    chain  chain dclassifier.bias  6.2e-06 .. 1.4e-05  6.72e-06  0.82  6.72e-06  0.93  chain:8@80
    chain  chain dclassifier.weight 2.8e-07 .. 5.2e-07  5.10e-07  1.41  4.95e-07  1.12  chain:8@80
    chain  chain dconv0.bias       8.3e-07 .. 1.6e-06  8.63e-07  1.04  8.74e-07  1.04  chain:64@32
    chain  chain dconv0.weight     3.1e-06 .. 6.8e-06  2.75e-06  0.89  9.32e-07  1.14  chain:64@32
    chain  chain dconv1.bias       8.3e-07 .. 1.6e-06  8.63e-07  1.04  8.74e-07  1.04  chain:64@32
    chain  chain dconv1.weight     6.2e-06 .. 9.0e-06  9.54e-06  1.07  8.71e-07  1.13  chain:64@32
    chain  chain dconv2.bias       3.0e-07 .. 4.0e-07  5.73e-07  1.93  7.98e-07  1.62  chain:64@32
    chain  chain dconv2.weight     1.7e-06 .. 1.8e-06  3.16e-06  1.75  8.37e-07  1.56  chain:64@32
    chain  chain dconv3.bias       3.1e-07 .. 3.5e-07  5.06e-07  1.46  7.52e-07  1.75  chain:64@32
    chain  chain dconv3.weight     9.4e-07 .. 1.8e-06  2.40e-06  1.34  7.76e-07  1.52  chain:64@32
    chain  chain dconv4.bias       2.0e-07 .. 3.8e-07  2.65e-07  1.00  1.93e-07  0.59  chain:64@32
    chain  chain dconv4.weight     6.8e-07 .. 1.2e-06  9.82e-07  1.12  4.05e-07  1.00  chain:8@80
    chain  chain dmap              2.7e-07 .. 6.9e-07  1.11e-06  1.76  9.43e-07  1.59  chain:8@80
    chain  chain logits            2.1e-07 .. 5.6e-07  7.33e-07  1.30  5.90e-07  1.06  chain:64@32
    chain  chain loss              4.8e-08 .. 4.8e-08  4.80e-08  0.21  4.80e-08  0.21  chain:64@32
    conv   db                      0.0e+00 .. 1.7e-07  2.07e-07  1.04  1.74e-07  0.87  ragged-20x12/relu_scaled
    conv   dw                      2.5e-08 .. 1.2e-06  5.56e-07  1.23  1.03e-07  0.51  wide/relu_scaled
    conv   dw+=                    1.3e-08 .. 1.1e-06  3.32e-07  1.02  8.28e-08  0.41  wide/relu_scaled
    conv   dx                      1.4e-08 .. 8.4e-07  1.14e-06  3.05  3.93e-07  1.44  ragged-20x12/uniform
    conv   y                       2.1e-08 .. 1.4e-06  1.16e-06  1.97  3.09e-07  1.25  views-wide/relu_scaled
    first  db0                     1.1e-07 .. 7.7e-07  1.16e-07  0.44  9.52e-08  0.37  first:(1, 3, 2, 20, 12, 12)
    first  db1                     1.1e-07 .. 7.7e-07  1.16e-07  0.44  9.52e-08  0.37  first:(1, 3, 2, 20, 12, 12)
    first  dmap                    1.1e-07 .. 2.7e-07  3.48e-07  2.00  2.59e-07  1.29  first:(1, 3, 2, 20, 12, 12)
    first  dw0                     2.9e-07 .. 8.4e-07  2.52e-07  0.81  1.50e-07  0.44  first:(1, 3, 2, 20, 12, 12)
    first  dw1                     1.7e-07 .. 7.0e-07  2.95e-07  0.77  1.36e-07  0.44  first:(1, 3, 2, 20, 12, 12)
    first  y                       1.7e-07 .. 2.4e-07  2.62e-07  1.12  8.29e-08  0.36  first:(3, 2, 1, 8, 6, 10)
    head   head da                 9.2e-08 .. 2.0e-07  4.30e-07  2.20  6.81e-08  0.48  head:3x37x(5, 5)/(2, 2)
    head   head db                 4.8e-09 .. 3.3e-07  1.58e-07  0.79  1.17e-07  0.59  head:3x20x(2, 5)/(1, 2)
    head   head dw                 3.7e-08 .. 1.5e-07  1.61e-07  0.81  9.28e-08  0.46  head:1x37x(16, 14)/(7, 7)
    head   head logits             2.8e-08 .. 7.5e-08  6.82e-08  0.29  5.12e-08  0.22  head:3x20x(2, 5)/(1, 2)
    head   head loss               3.0e-09 .. 7.1e-08  5.28e-08  0.23  5.28e-08  0.23  head:3x20x(16, 16)/(7, 7)

    41 cases with figures (42 tests), all pass, 4 s of test time.  Every tensor is within 3.1 x fp32 noise; no entry is over the
    gate (OVER_THE_GATE is empty).  The highest ratios are data gradients onto few channels (ragged-20x12: 3 channels, the `map`
    form), where torch's own fp32 error is at 1e-7 and the floor decides.
"""
import functools

import pytest
import torch

import adversarial2d_oracle as ao
import oracle_kit as kit
from oracle_kit import NAN, nan as _nan

pytestmark = pytest.mark.gpu

K, FLOOR = ao.K, ao.FLOOR
# A tensor over the gate is a finding, named here with its measured ratio; the gate itself stays where it is and the test fails.
OVER_THE_GATE = {}
LEAD, TRAIL = 1, 2            # channels of the wider buffer before / after a slice
_in, _out = functools.partial(kit.place, lead=LEAD, trail=TRAIL), functools.partial(kit.Out, lead=LEAD, trail=TRAIL)
STATS = []        # (case, label, kind, measure, e32, hip)
_checker = functools.partial(ao.Check, floor=FLOOR, stats=STATS, over_the_gate=OVER_THE_GATE, width=22)
F64 = torch.float64


def _ops():
    from mis_hip import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if STATS:
        ao.print_report("adversarial2d", STATS, FLOOR, width=22)
        kit.report(STATS, "MIS_ADVERSARIAL2D_STATS", {"stats": STATS})


# ---------------------------------------------------------------------------------------------------------------------
# the convolution alone: y, dx, dw, dw accumulated, db
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ao.names())
def test_conv_forward_data_gradient_weight_gradient(name):
    ops = _ops()
    chk = _checker(name)
    c = ao.case(name)
    r64, r32, _ = ao.references(name)
    N, Cin, Cout, H, W = c["shape"]
    lay = c["layout"]
    osh = (N, Cout, H // 2, W // 2)
    xv, dyv = _in(c["x"], lay), _in(c["dy"], lay)
    wd, bd = c["w"].cuda(), c["b"].cuda()
    ys = []
    for _ in range(2):
        y = _out(osh, lay)
        ops.conv2d_k4s2_fwd(xv, None, wd, None, bd, None, y.v, slope=1.0)
        assert y.untouched()
        ys.append(y.v)
    chk("y", "y", ys[0], r64["y"], r32["y"])
    assert torch.equal(ys[0], ys[1]), (name, "the forward is not run-to-run bit-identical")
    dxs = []
    for _ in range(2):
        dx = _out((N, Cin, H, W), lay)
        ops.conv2d_k4s2_dgrad(dyv, None, wd, dx.v, slope=1.0)
        assert dx.untouched()
        dxs.append(dx.v)
    chk("dx", "dx", dxs[0], r64["dx"], r32["dx"])
    assert torch.equal(dxs[0], dxs[1]), (name, "the data gradient is not run-to-run bit-identical")
    dws, dbs = [], []
    for _ in range(2):
        dw, db = _nan(*c["w"].shape), _nan(Cout)
        ops.conv2d_k4s2_wgrad(xv, None, dyv, None, dw, None, dbias=db, slope=1.0)
        dws.append(dw)
        dbs.append(db)
    chk("dw", "dw", dws[0], r64["dw"], r32["dw"], 0)
    db64 = c["dy"].double().sum((0, 2, 3))
    chk("db", "dw", dbs[0], db64, ao.one_thread(lambda: c["dy"].sum((0, 2, 3))))
    assert torch.equal(dws[0], dws[1]) and torch.equal(dbs[0], dbs[1]), (name, "the weight gradient is not bit-identical")
    # accumulated onto a non-zero dw (e32: fp32 torch's dw added in fp32)
    d0 = r64["dw"].flip(1).float()
    acc = d0.clone().cuda()
    ops.conv2d_k4s2_wgrad(xv, None, dyv, None, acc, None, slope=1.0, accumulate=True)
    chk("dw+=", "dw", acc, r64["dw"] + d0.double(), d0 + r32["dw"].float(), 0)
    chk.done()


def test_the_case_matrix_slices_the_forward_and_the_weight_gradient():
    """The contraction of "sliced" is cut in the forward (a workspace is asked for), that of "tiles-vec" is not; the weight
    gradient of "tiles-vec" (15 pixel tiles) is cut: its workspace holds more than the bias partials (at most 64 per channel)."""
    from mis_hip import lib
    assert lib.query("mis_conv2d_k4s2_fwd_workspace_bytes", *ao.SPECS["sliced"]["shape"]) > 0
    assert lib.query("mis_conv2d_k4s2_fwd_workspace_bytes", *ao.SPECS["tiles-vec"]["shape"]) == 0
    N, Cin, Cout, H, W = ao.SPECS["tiles-vec"]["shape"]
    assert lib.query("mis_conv2d_k4s2_wgrad_workspace_bytes", N, Cin, Cout, H, W) >= (2 * Cout * Cin * 16 + Cout) * 4


def _scale_pattern(N, C):
    """Dropout2d scales [N, C]: 0 or 2, both values in every sample (C > 1), channel 0 dropped in every sample."""
    n = torch.arange(N).reshape(N, 1)
    c = torch.arange(C).reshape(1, C)
    s = (((n * 3 + c * 5) % 7) % 2 == 1).float() * 2.0
    s[:, 0] = 0.0
    if C > 1:
        s[:, 1] = 2.0
    return s


@pytest.mark.parametrize("name", ["ragged-20x12/uniform", "c20-64/relu_scaled", "tiles-vec/relu_scaled", "sliced/uniform"])
def test_activation_and_dropout_epilogue(name):
    """LeakyReLU(0.2) + channel dropout in the forward's epilogue, and their derivative recovered from the stored output in
    both gradients.  The decisions are compared where the float64 pre-activation is outside the margin; the values are
    held to the oracle evaluated on the decisions the kernel took."""
    ops = _ops()
    chk = _checker("act:" + name)
    c = ao.case(name)
    r64, r32, _ = ao.references(name)
    N, Cin, Cout, H, W = c["shape"]
    scale = _scale_pattern(N, Cout)
    xv, dyv, wd, bd, sd = c["x"].cuda(), c["dy"].cuda(), c["w"].cuda(), c["b"].cuda(), scale.cuda()
    y = _nan(N, Cout, H // 2, W // 2)
    ops.conv2d_k4s2_fwd(xv, None, wd, None, bd, None, y, slope=ao.SLOPE, drop_scale=sd)
    yc = y.cpu()
    kept = (scale > 0).reshape(N, Cout, 1, 1).expand_as(yc)
    assert (yc[~kept] == 0).all(), "a dropped (n, c) plane is not exactly zero"
    pre64 = r64["y"]
    dec = ao.decided(pre64)
    signs = yc > 0
    assert torch.equal(signs[kept & dec], (pre64 > 0)[kept & dec]), "an activation decision outside the margin differs"
    signs = torch.where(kept, signs, pre64 > 0)           # a dropped plane keeps no decision; its gradient is zero anyway
    chk("act y", "y", y, ao.act_drop(pre64, ao.SLOPE, scale, signs), ao.act_drop(r32["y"].float(), ao.SLOPE, scale, signs))

    def back(dtype):
        x = c["x"].to(dtype).requires_grad_(True)
        w = c["w"].to(dtype).requires_grad_(True)
        b = c["b"].to(dtype).requires_grad_(True)
        ao.act_drop(ao.conv(x, w, b), ao.SLOPE, scale, signs).backward(c["dy"].to(dtype))
        return x.grad, w.grad, b.grad
    g64, g32 = back(F64), ao.one_thread(lambda: back(torch.float32))
    dx, dw, db = _nan(N, Cin, H, W), _nan(*c["w"].shape), _nan(Cout)
    ops.conv2d_k4s2_dgrad(dyv, y, wd, dx, slope=ao.SLOPE, drop_scale=sd)
    ops.conv2d_k4s2_wgrad(xv, None, dyv, y, dw, None, dbias=db, slope=ao.SLOPE, drop_scale=sd)
    chk("act dx", "dx", dx, g64[0], g32[0])
    chk("act dw", "dw", dw, g64[1], g32[1], 0)
    chk("act db", "dw", db, g64[2], g32[2])
    assert (dw[0] == 0).all() and db[0] == 0, "channel 0 is dropped in every sample: its gradients are exactly zero"
    chk.done()


# (N, Cl, Cx, Cout, H, W): the last one takes the 16-byte row path with the script's channel counts
@pytest.mark.parametrize("shape", [(3, 2, 1, 8, 6, 10), (1, 3, 2, 20, 12, 12), (2, 4, 1, 64, 12, 4), (2, 4, 1, 17, 24, 40)])
def test_first_layer_reads_softmax_of_logits(shape):
    """conv0(softmax(logits)) + conv1(image) as one convolution: forward, the two filter gradients and the two bias gradients
    written separately, and the gradient at the softmax output (the `map` gradient, Cin <= 4); 4-D and [N, C, 1, H, W] views."""
    ops = _ops()
    N, Cl, Cx, Cout, H, W = shape
    chk = _checker(f"first:{shape}")
    g = torch.Generator().manual_seed(sum(shape))
    lg = (torch.randn(N, Cl, H, W, generator=g, dtype=F64) * 2).float()
    im = torch.randn(N, Cx, H, W, generator=g, dtype=F64).float()
    w0 = ((torch.rand(Cout, Cl, 4, 4, generator=g, dtype=F64) * 2 - 1) * 0.2).float()
    w1 = ((torch.rand(Cout, Cx, 4, 4, generator=g, dtype=F64) * 2 - 1) * 0.2).float()
    b0, b1 = [(torch.rand(Cout, generator=g, dtype=F64) * 2 - 1).float() for _ in range(2)]
    dy = torch.randn(N, Cout, H // 2, W // 2, generator=g, dtype=F64).float()

    def ref(dtype):
        p = torch.softmax(lg.to(dtype), 1).requires_grad_(True)
        ws = [t.to(dtype).requires_grad_(True) for t in (w0, w1, b0, b1)]
        y = ao.conv(p, ws[0], ws[2]) + ao.conv(im.to(dtype), ws[1], ws[3])
        y.backward(dy.to(dtype))
        return [y.detach(), p.grad] + [t.grad for t in ws]
    r64, r32 = ref(F64), ao.one_thread(lambda: ref(torch.float32))
    lgd, imd, dyd = lg.cuda().unsqueeze(2), im.cuda(), dy.cuda()       # the logits as a 2-D HipNet hands them out
    y = _nan(*dy.shape)
    ops.conv2d_k4s2_fwd(imd, lgd, w1.cuda(), w0.cuda(), b1.cuda(), b0.cuda(), y, slope=1.0)
    chk("y", "y", y, r64[0], r32[0])
    dmaps = []
    for _ in range(2):
        dmap = _nan(N, Cl, 1, H, W)
        ops.conv2d_k4s2_dgrad(dyd, None, w0.cuda(), dmap, slope=1.0)
        dmaps.append(dmap)
    chk("dmap", "dx", dmaps[0], r64[1], r32[1])
    assert torch.equal(*dmaps)
    outs = []
    for _ in range(2):
        dw0, dw1, db0, db1 = _nan(*w0.shape), _nan(*w1.shape), _nan(Cout), _nan(Cout)
        ops.conv2d_k4s2_wgrad(imd, lgd, dyd, None, dw1, dw0, dbias=db1, dbias2=db0, slope=1.0)
        outs.append((dw0, dw1, db0, db1))
    for label, got, i in (("dw0", outs[0][0], 2), ("dw1", outs[0][1], 3), ("db0", outs[0][2], 4), ("db1", outs[0][3], 5)):
        chk(label, "dw", got, r64[i], r32[i], 0)
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    chk.done()


# ---------------------------------------------------------------------------------------------------------------------
# the head
# ---------------------------------------------------------------------------------------------------------------------
# (N, C, (H, W), (pool_h, pool_w))
HEAD_CASES = [(1, 20, (2, 2), (1, 1)), (3, 37, (5, 5), (2, 2)), (3, 20, (16, 16), (7, 7)), (1, 37, (14, 14), (7, 7)),
              (3, 20, (2, 5), (1, 2)), (1, 37, (16, 14), (7, 7))]


@pytest.mark.parametrize("N,C,ext,pool", HEAD_CASES)
def test_head_windowed_pool_linear_cross_entropy(N, C, ext, pool):
    ops = _ops()
    chk = _checker(f"head:{N}x{C}x{ext}/{pool}")
    g = torch.Generator().manual_seed(N * 1000 + C + ext[0])
    nwh, nww = ext[0] // pool[0], ext[1] // pool[1]
    Fe = C * nwh * nww
    a = torch.randn(N, C, *ext, generator=g, dtype=F64).float()
    w = (torch.randn(2, Fe, generator=g, dtype=F64) / Fe ** 0.5).float()
    b = torch.randn(2, generator=g, dtype=F64).float()
    target = (torch.arange(N) < (N + 1) // 2).int()
    r64 = ao.head2d(a, w, b, target, pool)
    r32 = ao.one_thread(lambda: ao.head2d(a, w, b, target, pool, torch.float32))
    outs = []
    for _ in range(2):
        ws = ops.adv_head2d_workspace(N, C, 2, *ext, pool)
        loss, logits, da, dw, db = _nan(1), _nan(N, 2), _nan(N, C, *ext), _nan(2, Fe), _nan(2)
        ops.adv_head2d_fwd(a.cuda(), w.cuda(), b.cuda(), target.cuda(), loss, logits, ws, pool)
        ops.adv_head2d_bwd(w.cuda(), da, dw, db, ws, pool)
        outs.append((loss, logits, da, dw, db))
    for i, (label, kind) in enumerate((("loss", "y"), ("logits", "y"), ("da", "dx"), ("dw", "dw"), ("db", "dw"))):
        chk("head " + label, kind, outs[0][i], r64[label].reshape(outs[0][i].shape), r32[label].reshape(outs[0][i].shape),
            0 if label in ("logits", "dw") else 1)
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    da = outs[0][2]
    assert (da[:, :, nwh * pool[0]:] == 0).all() and (da[:, :, :, nww * pool[1]:] == 0).all(), \
        "the rows and columns the floor-mode windows leave out receive an exactly zero gradient"
    assert (da[:, :, :nwh * pool[0], :nww * pool[1]] != 0).all()
    chk.done()


# ---------------------------------------------------------------------------------------------------------------------
# the whole chain
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ao.CHAINS))
def test_whole_chain_against_the_oracle_on_the_decisions_it_took(name):
    from networks.discriminator_2d import FCDiscriminator
    ndf, H, W, pool, N, _, _ = ao.CHAINS[name]
    C = ao.CHAIN_CLASSES
    chk = _checker(f"chain:{name}")
    img, lg, sd, masks, target, pool = ao.chain_inputs(name)
    dan = FCDiscriminator(C, ndf, 1, pool=pool)
    dan.load_state_dict(sd)
    dan.train()
    dan.drop_masks = [m.float().cuda() for m in masks]
    lgd, imgd, td = lg.cuda(), img.cuda(), target.cuda()
    runs = []
    for _ in range(2):
        for _, gv in dan.named_flat(dan.flat_grad):      # the padding words between the parameters stay zero
            gv.fill_(NAN)
        dan.loss_forward(lgd, imgd, td)
        dan.loss_backward(params=True, dmap=True)
        runs.append([dan.loss_buffer().clone(), dan.logits_buffer().clone(), dan.dmap_buffer().clone(), dan.flat_grad.clone()]
                    + [a.clone() for a in dan.activations()])
    assert all(torch.equal(x, y) for x, y in zip(*runs)), "the chain is not run-to-run bit-identical"
    acts = [a.cpu().reshape(a.shape[0], a.shape[1], a.shape[-2], a.shape[-1]) for a in runs[0][4:]]
    probs = torch.softmax(lg.double(), 1)
    free = ao.disc_step(sd, probs, img, target, masks, pool)                 # the float64 forward's own decisions
    signs, kept = {}, {}
    for i in ao.ACTIVATED:
        a, pre = acts[i], free["pres"][i]
        drops = ao.LAYER_ACT[i][1]
        kept[i] = (masks[i - 1] > 0).reshape(N, -1, 1, 1).expand_as(a) if drops else torch.ones_like(a, dtype=torch.bool)
        signs[i] = torch.where(kept[i], a > 0, pre > 0)        # a dropped plane keeps no decision; its gradient is zero anyway
    r64 = ao.disc_step(sd, probs, img, target, masks, pool, signs=signs)
    r32 = ao.one_thread(lambda: ao.disc_step(sd, probs, img, target, masks, pool, signs=signs, dtype=torch.float32))
    # the decisions differ from the float64 forward's only inside the margin (of the forward they belong to: r64's)
    for i in ao.ACTIVATED:
        pre = r64["pres"][i]
        live = ao.decided(pre) & kept[i]
        assert torch.equal(signs[i][live], (pre > 0)[live]), f"layer {i}: a decision outside the margin differs"
        assert (acts[i][~kept[i]] == 0).all(), f"layer {i}: a dropped plane is not exactly zero"
    chk("chain loss", "y", runs[0][0], r64["loss"], r32["loss"])
    chk("chain logits", "y", runs[0][1], r64["logits"], r32["logits"], 0)
    for i in range(4):
        chk(f"chain act{i}", "y", acts[i], r64["acts"][i], r32["acts"][i])
    chk("chain dmap", "dx", runs[0][2], r64["dmap"], r32["dmap"])
    for key, gview in dan.named_flat(runs[0][3]):
        chk("chain d" + key, "dw", gview, r64["grads"][key], r32["grads"][key], 0)
    chk.done()
