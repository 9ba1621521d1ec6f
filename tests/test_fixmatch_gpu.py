"""FixMatch on the GPU: mis_fixmatch_tail over the edge matrix of tests/fixmatch_oracle.py, mis_color_jitter, and
FixMatchTrainer (three steps against the oracle and a torch restatement of the update, tape against eager, the batch rule,
the command line, two gloo ranks against one process).

The tail.  Quantised-logit cases (multiples of 0.25: exact ties, first wins on both sides; test_fixmatch_cpu.py asserts a
relative margin >= 1e-3 on every mask and clamp comparison of these very inputs) must reproduce the float64 decisions in
every pixel.  Continuous-logit cases are arbitrated: the kernel's pseudo / comp maps must equal the float64 decisions
wherever the float64 margin exceeds 1e-5, may differ in at most 8 pixels below it, and the values are compared against the
oracle evaluated AT the kernel's decisions.  Tolerance (the convention of tests/test_loss_tails_gpu.py), per scalar and
per gradient tensor:

    |hip - f64|_max <= max(6 * e32, FLOOR) * |f64|_max

e32 = fp32 CPU torch.autograd of the literal reference expression against the float64 oracle, same case and quantity;
FLOOR = the largest e32 over the matrix (fixmatch_oracle.FLOOR_SCALAR / FLOOR_TENSOR, held to the measurement by
test_fixmatch_cpu.py).  A reference of exactly 0 (d_weak on the unlabeled rows, masked_in_fraction when nothing passes) is
met exactly.

Measured on an MI355X (this file's own run; MIS_FIXMATCH_STATS=<file> writes every figure, profiles/fixmatch_tail_stats.json):

    quantity   e32 (fp32 torch vs float64)   HIP vs float64 (max)   worst HIP / max(e32, floor)   worst HIP / e32
    scalar     5.5e-8   .. 1.05e-6           1.39e-7                0.13                          (floor governs)
    tensor     1.1e-8   .. 3.38e-7           3.38e-7                0.99                          1.45

    FLOOR_SCALAR = 1.1e-6 (largest scalar e32: 1.05e-6, C2-u8-part-B4-L2-offset-float-quant),
    FLOOR_TENSOR = 3.4e-7 (largest tensor e32: 3.38e-7, d_weak of C4-i64-2d-B4-L2-strided-float-quant).
    57 cases.  Every scalar is below 1.4e-7, an eighth of the scalar floor (the adaptive weight is summed as ln S - H, in
    double from the workgroup partials on); every gradient tensor is within 1.45 x its own e32 and below the tensor floor
    (K = 6 is never needed).
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

import fixmatch_oracle as fo
import oracle_kit as kit
from oracle_kit import NAN, same_bits as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")
TOL_LOGIT = 1e-3            # of tests/test_dct_gpu.py
TOL_LOSS = 1e-3
PAD = 8
STATS = []


def _ops():
    from mis_hip import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if STATS:
        worst = {k: max((r[k] for r in STATS), default=0.0) for k in ("e32_scalar", "hip_scalar", "e32_tensor", "hip_tensor")}
        kit.report(STATS, "MIS_FIXMATCH_STATS", dict(floor_scalar=fo.FLOOR_SCALAR, floor_tensor=fo.FLOOR_TENSOR, K=fo.K,
                                                     worst=worst, cases=STATS), indent=1)


# ---------------------------------------------------------------------------------------------------------------------
# device placement and the kernel call
# ---------------------------------------------------------------------------------------------------------------------
def _place(t, layout, like=None):
    """(buffer, view) of a CPU tensor [n, C, 1, H, W] (or of NaNs shaped ``like``): dense, batch-strided, two rows into a
    strided buffer, or one float into a buffer of odd row width (4-byte aligned only: the scalar path)."""
    src = like if t is None else t
    n, row = src.shape[0], src[0].numel()
    if layout == "shift1":
        buf = torch.full((n * (row + 1) + 1,), NAN, device="cuda")
        view = buf[1:].view(n, row + 1)[:, :row]
        if t is not None:
            view.copy_(t.reshape(n, row).cuda())
        view = view.view(src.shape)
        assert view.data_ptr() == buf.data_ptr() + 4
        return buf, view
    return kit.place_rows(t, layout, PAD, like)


def _untouched_outside(buf, view):
    if buf.dim() == 2:
        return kit.untouched_outside(buf, view)
    rest = buf.clone()
    n, row = view.shape[0], view[0].numel()
    rest[1:].view(n, row + 1)[:, :row].fill_(NAN)
    return bool(torch.isnan(rest).all())


def _state():
    ops = _ops()
    st = ops.new_step_state()
    ops.step_init(st, 1, 500, 0.01, 1000, 0.99, fo.W, 0.0, 150, 0)      # rampup 0: cons_weight = (float)W
    return st


def _launch(c, x, layout, wmode, grads=(True, True), maps=True):
    ops = _ops()
    zw, zs, lab = x
    B, C, L = c["B"], c["C"], c["L"]
    S = zw[0, 0].numel()
    vw, vs = _place(zw, layout)[1], _place(zs, layout)[1]
    out = torch.full((16,), NAN, device="cuda")
    dw = _place(None, layout, like=zw) if grads[0] else None
    ds = _place(None, layout, like=zs) if grads[1] else None
    pseudo = torch.full(((B - L) * S,), 255, dtype=torch.uint8, device="cuda") if maps else None
    comp = torch.full((B * S,), 255, dtype=torch.uint8, device="cuda") if maps else None
    ops.scratch(1, "tail").view(torch.float32).fill_(NAN)
    wkw = dict(cons_weight=fo.W) if wmode == "float" else dict(state=_state())
    ops.fixmatch_tail(vw, vs, lab.cuda(), L, out, d_weak=dw and dw[1], d_strong=ds and ds[1], conf_thresh=fo.TAU,
                      pseudo=pseudo, comp=comp, **wkw)
    torch.cuda.synchronize()
    return out, dw, ds, pseudo, comp


@pytest.mark.parametrize("c", fo.matrix(), ids=fo.cid)
def test_fixmatch_tail_matches_float64(c):
    x = fo.inputs(c)
    zw, zs, lab = x
    B, C, L = c["B"], c["C"], c["L"]
    S = zw[0, 0].numel()
    w32 = float(torch.tensor(fo.W, dtype=torch.float32))
    out, dw, ds, pseudo, comp = _launch(c, x, c["layout"], c["wmode"])
    # every element written once and nothing else
    assert torch.isfinite(out[:10]).all() and torch.isnan(out[10:]).all(), out
    for buf, view in (dw, ds):
        assert torch.isfinite(view).all() and _untouched_outside(buf, view)
    pseudo, comp = pseudo.cpu().long().view(B - L, S), comp.cpu().long().view(B, S)
    assert pseudo.max() < C and comp.max() < C
    # the decisions
    p64, k64, _ = fo.decisions(zw, fo.TAU)
    if c["content"] != "cont":
        assert torch.equal(pseudo, p64[L:]) and torch.equal(comp, k64)
        inj = {}
    else:
        pm, km = fo.decision_margins(zw, fo.TAU)
        dp, dk = pseudo != p64[L:], comp != k64
        assert not (dp & (pm[L:] > 1e-5)).any() and not (dk & (km > 1e-5)).any()
        assert int(dp.sum()) + int(dk.sum()) <= 8
        inj = dict(pseudo=pseudo, comp=comp)
    ref = fo.fixmatch_tail(zw, zs, lab, L, fo.TAU, w32, **inj)
    es, ew, et = fo.e32(c, zw, zs, lab, ref, **inj)
    got = out[:10].cpu().double()
    hs = fo.scalar_rels(got, ref[0])
    print(f"\n[fixmatch tail] {fo.cid(c)}: scalars e32 {max(es):.2e} hip {max(hs):.2e}", end="")
    row = dict(case=fo.cid(c), e32_scalar=max(es), hip_scalar=max(hs))
    for i in range(10):
        if ref[0][i].item() == 0:
            assert got[i].item() == 0, (i, got[i].item())
        else:
            assert hs[i] <= max(fo.K * es[i], fo.FLOOR_SCALAR), (ops_name(i), got[i].item(), ref[0][i].item(), hs[i], es[i])
    assert got[4].item() == w32
    gw, gs = dw[1].cpu().double(), ds[1].cpu().double()
    assert torch.equal(gw[L:], torch.zeros_like(gw[L:]))                      # exactly 0: no gradient through the decisions
    hw, ht = fo.rel(gw, ref[1]), fo.rel(gs, ref[2])
    print(f"  d_weak e32 {ew:.2e} hip {hw:.2e}  d_strong e32 {et:.2e} hip {ht:.2e}", end="")
    row.update(e32_tensor=max(ew, et), hip_tensor=max(hw, ht), e32_d_weak=ew, hip_d_weak=hw, e32_d_strong=et, hip_d_strong=ht)
    STATS.append(row)
    assert hw <= max(fo.K * ew, fo.FLOOR_TENSOR), (hw, ew)
    assert ht <= max(fo.K * et, fo.FLOOR_TENSOR), (ht, et)
    # bit-reproducible
    out2, dw2, ds2, p2, k2 = _launch(c, x, c["layout"], c["wmode"])
    assert _same(out, out2) and _same(dw[0], dw2[0]) and _same(ds[0], ds2[0])
    # forward only, and one gradient alone: the same scalars, the same gradient
    out3 = _launch(c, x, c["layout"], c["wmode"], grads=(False, False), maps=False)[0]
    assert _same(out, out3)
    if c["layout"] == "dense":
        out4, _, ds4, _, _ = _launch(c, x, "dense", c["wmode"], grads=(False, True), maps=False)
        assert _same(out, out4) and _same(ds[0], ds4[0])
    # only addresses differ between a strided / offset view and the dense tensor (shift1 takes the scalar path instead of
    # the float4 one: other partial sums, the same tolerance)
    if c["layout"] in ("strided", "offset"):
        outd, dwd, dsd, _, _ = _launch(c, x, "dense", c["wmode"])
        assert _same(out, outd) and torch.equal(dw[1], dwd[1]) and torch.equal(ds[1], dsd[1])
    # the weight from the device state == the weight from the float argument
    if c["wmode"] == "state":
        outf, dwf, dsf, _, _ = _launch(c, x, c["layout"], "float")
        assert _same(out, outf) and _same(dw[0], dwf[0]) and _same(ds[0], dsf[0])


def ops_name(i):
    return _ops().FIXMATCH_OUT[i]


def test_fixmatch_tail_refuses_bad_geometry_without_launching():
    from mis_hip import lib
    ops = _ops()
    L = lib.load()
    B, C, S = 4, 3, 64
    zw, zs = torch.randn((B, C, S), device="cuda"), torch.randn((B, C, S), device="cuda")
    lab = torch.zeros((B, S), dtype=torch.uint8, device="cuda")
    out = torch.full((16,), NAN, device="cuda")
    d = torch.full((B, C, S), NAN, device="cuda")
    ws = ops.scratch(L.mis_fixmatch_tail_workspace_bytes(B, C, S), "tail")

    def call(B=B, Lb=2, C=C, S=S, lb=1, wsb=None):
        return L.mis_fixmatch_tail(lib.ptr(zw), C * S, lib.ptr(zs), C * S, lib.ptr(lab), lb, B, Lb, C, S, 0.8, 0.1, None,
                                   lib.ptr(out), lib.ptr(d), C * S, lib.ptr(d), C * S, None, None, lib.ptr(ws),
                                   ws.numel() if wsb is None else wsb, lib.stream_ptr())

    assert call(Lb=0) == -1 and call(Lb=B) == -1 and call(Lb=B + 1) == -1      # MIS_ERR_ARG unless 1 <= L < B
    assert call(S=1) == -1                                                        # ln 1 = 0
    assert call(lb=4) == -1
    assert call(C=5, S=32) == -2 and call(C=1, S=64) == -2                       # MIS_ERR_UNSUPPORTED
    assert call(wsb=64) == -4                                                     # MIS_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(d).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out[:10]).all()


# ---------------------------------------------------------------------------------------------------------------------
# colour jitter
# ---------------------------------------------------------------------------------------------------------------------
FACTORS = [(b, g, o) for o in (0, 1) for b in (0.2, 1.0, 1.8) for g in (0.2, 1.0, 1.8)]


@pytest.mark.parametrize("shape", [(64, 64), (7, 9), (70, 70), (67, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("content", ["unit", "saturating", "constant"])
def test_color_jitter_matches_float64_formula(shape, content):
    ops = _ops()
    g = torch.Generator().manual_seed(shape[0] * 100 + len(content))
    B = len(FACTORS)
    if content == "unit":
        x = torch.rand((B, 1) + shape, generator=g)
    elif content == "saturating":                      # values outside [0, 1] and factors that push inside ones out
        x = torch.rand((B, 1) + shape, generator=g) * 3 - 1
    else:
        x = torch.tensor([0.0, 0.5, 1.0]).repeat(B // 3).view(B, 1, 1, 1).expand((B, 1) + shape).contiguous()
    params = torch.tensor(FACTORS, dtype=torch.float32)
    ref = fo.color_jitter(x, params)
    y32 = fo.color_jitter(x, params, torch.float32)
    for view in ("dense", "strided"):
        if view == "dense":
            xd = x.cuda()
        else:
            base = torch.full((B + 1, x[0].numel() + 4), NAN, device="cuda")
            xd = base[1:, :x[0].numel()].view(x.shape)
            xd.copy_(x.cuda())
        out = torch.full(x.shape, NAN, device="cuda")
        drawn = torch.full((B, 3), NAN, device="cuda")
        ops.color_jitter(xd, out, params=params.cuda(), drawn=drawn)
        out2 = torch.full(x.shape, NAN, device="cuda")
        ops.color_jitter(xd, out2, params=params.cuda())
        torch.cuda.synchronize()
        assert _same(out, out2) and torch.equal(drawn.cpu(), params)
        assert out.min().item() >= 0 and out.max().item() <= 1
        for b in range(B):
            e32 = fo.rel(y32[b], ref[b])
            hip = fo.rel(out[b].cpu(), ref[b])
            if ref[b].abs().max().item() == 0:
                assert out[b].abs().max().item() == 0
            else:
                assert hip <= max(fo.K * e32, fo.FLOOR_TENSOR), (view, FACTORS[b], hip, e32)
    if content == "saturating":
        assert ((ref == 0) | (ref == 1)).double().mean().item() > 0.2       # the clamp bites


def test_color_jitter_device_draws():
    ops = _ops()
    B, shape = 64, (32, 32)
    x = torch.rand((B, 1) + shape, generator=torch.Generator().manual_seed(5))
    xd = x.cuda()

    def draw(seed, it):
        st = ops.new_step_state()
        ops.step_init(st, seed, it, 0.01, 30000, 0.99, 0.1, 200.0)
        out = torch.full(x.shape, NAN, device="cuda")
        drawn = torch.full((B, 3), NAN, device="cuda")
        ops.color_jitter(xd, out, state=st, drawn=drawn)
        torch.cuda.synchronize()
        return out, drawn.cpu()

    out, f = draw(1337, 10)
    assert (f[:, :2] >= 0.2).all() and (f[:, :2] <= 1.8).all()
    assert set(f[:, 2].tolist()) == {0.0, 1.0}                              # both orders occur
    assert f[:, 0].unique().numel() == B and f[:, 1].unique().numel() == B  # different across samples
    assert 0.6 < f[:, 0].mean().item() < 1.4 and f[:, 0].min().item() < 0.5 and f[:, 0].max().item() > 1.5
    out_b, f_b = draw(1337, 10)
    assert _same(out, out_b) and torch.equal(f, f_b)                        # reproducible from (seed, iteration)
    _, f_next = draw(1337, 11)
    _, f_seed = draw(1338, 10)
    assert not torch.equal(f, f_next) and not torch.equal(f, f_seed)        # fresh per iteration and per seed
    assert (f[:, 0] != f_next[:, 0]).all()
    ref = fo.color_jitter(x, f)                                             # the image is jittered by the factors reported
    assert fo.rel(out.cpu(), ref) <= max(fo.K * fo.rel(fo.color_jitter(x, f, torch.float32), ref), fo.FLOOR_TENSOR)


# ---------------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------------
IT0 = 1200
CFG = dict(base_lr=0.01, max_iterations=30000, ema_decay=0.99, consistency=0.1, consistency_rampup=200.0)


def _nets():
    from networks.net_factory import net_factory
    from oracle import filler
    from oracle.nets import OracleUNet2D
    sd = filler.fill_state_dict(OracleUNet2D(1, 4).new_state())
    model, ema = net_factory("unet", 1, 4), net_factory("unet", 1, 4)
    model.load_state_dict(sd)
    ema.load_state_dict(sd)
    model.train()
    ema.train()
    model.dropout_enabled = ema.dropout_enabled = False
    return model, ema


def _batch():
    from oracle import filler
    return filler.image((4, 1, 64, 64), "volume").cuda(), filler.labels((4, 64, 64), 4, torch.uint8).cuda()


def test_fixmatch_step_matches_oracle_and_torch_update():
    from mis_hip.step import FixMatchTrainer
    ops = _ops()
    model, ema = _nets()
    vol, lab = _batch()
    tr = FixMatchTrainer(model, ema, labeled_bs=2, num_classes=4, iter_num=IT0, **CFG)
    jit = torch.tensor([[1.3, 0.7, 0], [0.5, 1.6, 1], [1.8, 0.2, 1], [0.9, 1.1, 0]])
    shape5 = (4, 1, 1, 64, 64)
    for i in range(3):
        it = IT0 + i
        st0 = ops.read_step_state(tr.state)
        lr_prev, alpha, w = fo.schedule(it - 1, CFG["base_lr"], CFG["max_iterations"], CFG["ema_decay"], CFG["consistency"],
                                        CFG["consistency_rampup"])[0], *fo.schedule(it, 0.01, 30000, 0.99, 0.1, 200.0)[1:]
        assert st0["iter_num"] == it and abs(st0["lr"] - lr_prev) <= 1e-9 and abs(st0["ema_alpha"] - alpha) <= 1e-7
        assert abs(st0["cons_weight"] - w) <= 1e-8
        p0, m0, e0 = model.flat_param.clone(), tr.momentum_buf.clone(), ema.flat_param.clone()
        out = tr.step(vol, lab, jitter=jit)
        torch.cuda.synchronize()
        assert tr._tape is None                                              # injected factors keep the step eager
        strong = fo.color_jitter(vol.cpu(), jit)
        assert fo.rel(tr._strong_in.cpu(), strong) <= 1e-6 and torch.equal(tr.jitter_factors.cpu(), jit)
        pw, ps = model.plan_for(shape5), model.plan_for(shape5, slot=1)
        zw, zs = pw.out.t.detach().clone(), ps.out.t.detach().clone()
        gw, gs = pw.out.grad().detach().clone(), ps.out.grad().detach().clone()
        # the kernel's own decisions on these logits (continuous: arbitrated, as in the tail tests)
        pm = torch.empty(2 * 4096, dtype=torch.uint8, device="cuda")
        cm = torch.empty(4 * 4096, dtype=torch.uint8, device="cuda")
        chk = torch.zeros(16, device="cuda")
        ops.fixmatch_tail(zw, zs, lab[:2].contiguous(), 2, chk, conf_thresh=0.8, cons_weight=st0["cons_weight"], pseudo=pm,
                          comp=cm)
        assert _same(chk[:10], out[:10])
        p64, k64, _ = fo.decisions(zw.cpu(), 0.8)
        pmar, kmar = fo.decision_margins(zw.cpu(), 0.8)
        pm, cm = pm.cpu().long().view(2, 4096), cm.cpu().long().view(4, 4096)
        assert not ((pm != p64[2:]) & (pmar[2:] > 1e-5)).any() and not ((cm != k64) & (kmar > 1e-5)).any()
        ref, rw, rs = fo.fixmatch_tail(zw.cpu(), zs.cpu(), lab[:2].cpu(), 2, 0.8, st0["cons_weight"], pseudo=pm, comp=cm)
        got = tr.losses()
        for j, k in enumerate(ops.FIXMATCH_OUT):
            assert abs(got[k] - ref[j].item()) <= TOL_LOSS * max(1.0, abs(ref[j].item())), (i, k, got[k], ref[j].item())
        assert (gw.cpu().double() - rw).abs().max().item() <= TOL_LOGIT * rw.abs().max().item()
        assert (gs.cpu().double() - rs).abs().max().item() <= TOL_LOGIT * rs.abs().max().item()
        assert torch.equal(gw[2:], torch.zeros_like(gw[2:]))
        # SGD (momentum 0.9, wd 1e-4), EMA and the schedule: a plain torch restatement on the step's summed gradient
        g = model.flat_grad.double()
        assert torch.isfinite(g).all() and not torch.equal(model.flat_grad, tr._stash)       # both passes are in it
        m1 = 0.9 * m0.double() + (g + 1e-4 * p0.double())
        p1 = p0.double() - st0["lr"] * m1
        e1 = alpha * e0.double() + (1 - alpha) * p1
        scale = p0.abs().max().item()
        assert (tr.momentum_buf.double() - m1).abs().max().item() <= 1e-6 * max(m1.abs().max().item(), 1e-3)
        assert (model.flat_param.double() - p1).abs().max().item() <= 1e-6 * scale
        assert (ema.flat_param.double() - e1).abs().max().item() <= 1e-6 * scale
        st1 = ops.read_step_state(tr.state)
        assert st1["iter_num"] == it + 1 and tr.iter_num == it + 1
        assert abs(st1["lr"] - fo.schedule(it, 0.01, 30000, 0.99, 0.1, 200.0)[0]) <= 1e-9
    sd = model.state_dict()
    assert all(int(sd[n]) == 6 for n in sd if n.endswith("num_batches_tracked"))       # two train-mode passes per step


def _run(steps, use_tape, seed=7):
    from mis_hip.step import FixMatchTrainer
    model, ema = _nets()
    model.dropout_enabled = True
    vol, lab = _batch()
    tr = FixMatchTrainer(model, ema, labeled_bs=2, num_classes=4, seed=seed, iter_num=IT0, use_tape=use_tape, **CFG)
    outs, factors = [], []
    for i in range(steps):
        tr.step(vol if i % 2 == 0 else vol.flip(0).contiguous(), lab)
        outs.append(tr.out.clone())
        factors.append(tr.jitter_factors.clone())
    torch.cuda.synchronize()
    return dict(out=torch.stack(outs), factors=torch.stack(factors), param=model.flat_param.clone(), ema=ema.flat_param.clone(),
                bufs=[b.clone() for b in model.buffers()], tape=tr._tape is not None)


def test_fixmatch_tape_and_eager_are_bit_identical_and_factors_are_fresh():
    taped, eager, again = _run(5, True), _run(5, False), _run(5, True)
    assert taped["tape"] and not eager["tape"]
    for r in (eager, again):
        assert torch.equal(taped["out"], r["out"]) and torch.equal(taped["param"], r["param"])
        assert torch.equal(taped["ema"], r["ema"]) and torch.equal(taped["factors"], r["factors"])
        assert all(torch.equal(a, b) for a, b in zip(taped["bufs"], r["bufs"]))
    f = taped["factors"]                                   # steps 4 and 5 are replays: drawn on the device per iteration
    for i in range(5):
        for j in range(i + 1, 5):
            assert (f[i, :, :2] != f[j, :, :2]).all(), (i, j)
    assert (f[:, :, :2] >= 0.2).all() and (f[:, :, :2] <= 1.8).all()
    assert torch.isfinite(taped["out"][:, :10]).all() and (taped["out"][:, 7] > 0).all()
    assert not torch.equal(_run(1, True, seed=8)["factors"], f[:1])


def test_fixmatch_trainer_rejects_bad_batch_before_launch():
    from mis_hip.step import FixMatchTrainer
    model, ema = _nets()
    tr = FixMatchTrainer(model, ema, labeled_bs=2, num_classes=4)
    before = model.flat_param.clone()
    z = lambda *s: torch.zeros(s, device="cuda")
    lab = torch.zeros((4, 32, 32), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        tr.step(z(2, 1, 32, 32), lab[:2])                                   # labeled_bs == batch_size
    with pytest.raises(ValueError):
        tr.step(z(4, 2, 32, 32), lab)                                       # one channel
    with pytest.raises(ValueError):
        tr.step(z(4, 1, 32, 32), lab, jitter=z(3, 3))
    with pytest.raises(ValueError):
        tr.step(z(4, 1, 32, 32), lab, strong=z(4, 1, 32, 16))
    with pytest.raises(ValueError):
        tr.step(z(4, 1, 32, 32), lab, strong=z(4, 1, 32, 32), jitter=z(4, 3))
    torch.cuda.synchronize()
    assert torch.equal(before, model.flat_param) and tr.iter_num == 0
    # an injected strong batch is used as it is
    vol, lab = _batch()
    strong = (vol * 0.5).contiguous()
    tr.step(vol, lab, strong=strong)
    torch.cuda.synchronize()
    assert tr._strong_in is None and torch.isfinite(tr.out[:10]).all()


def test_weak_strong_augment_item_transform():
    import numpy as np
    from dataloaders.dataset import WeakStrongAugment
    rng = np.random.RandomState(0)
    image, label = rng.rand(40, 52).astype(np.float32), rng.randint(0, 4, (40, 52)).astype(np.uint8)
    np.random.seed(21)
    torch.manual_seed(21)
    s = WeakStrongAugment((32, 32))({"image": image, "label": label})
    np.random.seed(21)
    k, axis = np.random.randint(0, 4), np.random.randint(0, 2)
    torch.manual_seed(21)
    beta, gamma, order = WeakStrongAugment.draw_jitter()
    from scipy.ndimage import zoom
    img_r, lab_r = zoom(image, (32 / 40, 32 / 52), order=0), zoom(label, (32 / 40, 32 / 52), order=0)
    weak = np.flip(np.rot90(img_r, k), axis=axis).copy()
    lab_w = np.flip(np.rot90(lab_r, k), axis=axis).copy()
    assert np.array_equal(s["image"].cpu().numpy()[0], img_r) and np.array_equal(s["image_weak"].cpu().numpy()[0], weak)
    assert np.array_equal(s["label_aug"].cpu().numpy(), lab_w) and s["label_aug"].dtype == torch.uint8
    ref = fo.color_jitter(torch.from_numpy(weak)[None, None], torch.tensor([[beta, gamma, order]], dtype=torch.float32))
    assert fo.rel(s["image_strong"].cpu()[None], ref) <= 1e-6 and tuple(s["image_strong"].shape) == (1, 32, 32)


# ---------------------------------------------------------------------------------------------------------------------
# data parallel: two gloo ranks on the same batch == one process
# ---------------------------------------------------------------------------------------------------------------------
def _fm_worker(rank, world, store, out_dir):
    for p in (PKG, ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=world)
    from networks.net_factory import net_factory
    from mis_hip.step import FixMatchTrainer
    torch.manual_seed(5)
    m, e = net_factory("unet", 1, 4), net_factory("unet", 1, 4)
    e.load_state_dict(m.state_dict())
    m.train()
    e.train()
    g = torch.Generator(device="cuda").manual_seed(100)          # the same batch on every rank
    vol = torch.rand((4, 1, 64, 64), generator=g, device="cuda")
    lab = torch.randint(0, 4, (4, 64, 64), generator=g, device="cuda").to(torch.uint8)
    tr = FixMatchTrainer(m, e, labeled_bs=2, num_classes=4, iter_num=1000, seed=7)
    for _ in range(4):                                           # the fourth step is a replay of the tape
        tr.step(vol, lab)
    torch.cuda.synchronize()
    torch.save(dict(param=m.flat_param.cpu(), ema=e.flat_param.cpu(), tape=tr._tape is not None),
               os.path.join(out_dir, f"fm_{world}_{rank}.pt"))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_fixmatch_two_gloo_ranks_match_one_process(tmp_path):
    mp.spawn(_fm_worker, args=(1, None, str(tmp_path)), nprocs=1, join=True)
    mp.spawn(_fm_worker, args=(2, str(tmp_path / "gloo_store"), str(tmp_path)), nprocs=2, join=True)
    r = {k: torch.load(os.path.join(tmp_path, f"fm_{k}.pt")) for k in ("1_0", "2_0", "2_1")}
    assert all(v["tape"] for v in r.values())
    # the summed buffer is exchanged once: (g + g) / 2 == g bit for bit
    for key in ("param", "ema"):
        assert torch.equal(r["2_0"][key], r["2_1"][key]) and torch.equal(r["2_0"][key], r["1_0"][key])


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
def test_fixmatch_cli_runs(tmp_path):
    work = tmp_path / "code"
    work.mkdir()
    cmd = [sys.executable, os.path.join(PKG, "train_Fixmatch_CNN_2D.py"), "--root_path", str(tmp_path / "no_data"), "--exp",
           "fm_cli", "--max_iterations", "1", "--batch_size", "4", "--labeled_bs", "2", "--patch_size", "64", "64"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run(cmd, cwd=work, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Training Finished!" in r.stdout and "iteration 1 : model loss :" in r.stdout + r.stderr
    snap = tmp_path / "model" / "fm_cli_14" / "unet"
    ck = torch.load(str(snap / "unet_best_model.pth"))
    assert sorted(ck) == ["epoch", "loss", "optimizer_state_dict", "state_dict"]
    assert ck["optimizer_state_dict"]["iter_num"] == 1
    from networks.net_factory import net_factory
    a, b = net_factory("unet", 1, 4), net_factory("unet", 1, 4)
    a.load_state_dict(ck["state_dict"])
    b.load_state_dict(ck)                      # the wrapped form, as test_2D_fully.py hands it over
    assert torch.equal(a.flat_param, b.flat_param) and all(torch.equal(x, y) for x, y in zip(a.buffers(), b.buffers()))
    with pytest.raises(RuntimeError):          # any other dictionary is still refused
        b.load_state_dict({"epoch": 1, "state_dict": ck["state_dict"]})
    scal = (snap / "scalars.csv").read_text()
    for tag in ("1,lr,", "1,consistency_weight/consistency_weight,", "1,loss/model_loss,"):
        assert tag in scal
