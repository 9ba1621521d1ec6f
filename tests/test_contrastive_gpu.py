"""Contrastive cross teaching on the GPU: the frozen projector / classifier heads, mis_contrastive_cross_tail, the device
schedule, ContrastiveCrossTrainer (eager, taped, with the Swin student, data parallel) and the two command lines, all
against the float64 numpy oracle of tests/contrastive_oracle.py (held to the real reference by tests/test_contrastive_cpu.py).

Gates.  Tail and step scalars / logits gradients (the convention of tests/test_fixmatch_gpu.py):

    |hip - f64|max <= max(6 * e32, FLOOR) * |f64|max

e32 = the fp32 CPU torch evaluation of the literal reference expression against float64, same case and quantity; FLOOR =
the largest e32 over the tail's matrix (contrastive_oracle.FLOOR_SCALAR / FLOOR_TENSOR, measured on the CPU and held to
that measurement by test_contrastive_cpu.py).  Heads: the same form with e32 = fp32 torch operators against the float64
oracle and the floor 2^-23, one fp32 unit in the last place of the largest entry.  ReLU and max-pool decisions: a GPU pass
arbitrates its own near-ties (the float64 gradient is evaluated on the branch the pass took), and may differ from float64
only where float64 is within 1e-5 of the boundary, at most 8 times.  Flat gradients: the per-tensor envelope of
tests/test_cross_teaching_gpu.py, (6 * e32 + 2e-3) * |ref|max + 5e-4 * (largest gradient entry of the network), float64
and fp32 both on the LeakyReLU branches the pass took (_score_flat_grads).

MIS_CONTRASTIVE_STATS=<file> writes every figure of the tail matrix (profiles/contrastive_tail_stats.json).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import contrastive_oracle as co
import oracle_kit as kit
import patch_nce_oracle as pno
from oracle_kit import NAN, same_bits as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")
PAD = 8
ULP = 2.0 ** -23
STATS = []
HEADS = ("classifier_1", "classifier_2", "projector_1", "projector_2")


def _ops():
    from mis_hip import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if STATS:
        worst = {k: max((r[k] for r in STATS), default=0.0) for k in ("e32_scalar", "hip_scalar", "e32_tensor", "hip_tensor")}
        kit.report(STATS, "MIS_CONTRASTIVE_STATS", dict(floor_scalar=co.FLOOR_SCALAR, floor_tensor=co.FLOOR_TENSOR, K=co.K,
                                                        worst=worst, cases=STATS), indent=1)


def _np_sd(net):
    return {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}


# ---------------------------------------------------------------------------------------------------------------------
# heads
# ---------------------------------------------------------------------------------------------------------------------
def _head(kind, seed, plain=False):
    """A head with non-trivial BatchNorm affine parameters and running buffers (loaded through load_state_dict)."""
    from networks.net_factory import net_factory
    torch.manual_seed(seed)
    h = net_factory(kind)
    if not plain:
        g = torch.Generator().manual_seed(seed + 1)
        sd = h.state_dict()
        for k in sd:
            if k.endswith("bn.weight"):
                sd[k] = 1.0 + 0.3 * torch.randn(sd[k].shape, generator=g)
            elif k.endswith("bn.bias"):
                sd[k] = 0.2 * torch.randn(sd[k].shape, generator=g)
            elif k.endswith("running_mean"):
                sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
            elif k.endswith("running_var"):
                sd[k] = 1.0 + 0.2 * torch.rand(sd[k].shape, generator=g)
        h.load_state_dict(sd)
    h.train()
    return h


def _plan_ops(head):
    plan = head._last[0]
    norms = [op for op in plan.ops if type(op).__name__ == "NormActOp"]
    pools = [op for op in plan.ops if type(op).__name__ == "MaxPoolOp"]
    return plan, norms, pools


def _gpu_decisions(head):
    _, norms, pools = _plan_ops(head)
    out = []
    for n, p in zip(norms, pools):
        N, C, _, H, W = n.y.shape
        out.append(((n.y.t[:, :, 0] > 0).cpu().numpy(), p.idx.view(N, C, H // 2, W // 2).cpu().numpy().astype(np.int64)))
    return out


def _gate(hip, e32, floor=ULP):
    return hip <= max(co.K * e32, floor)


HEAD_CASES = [(k, s) for k in ("projector", "classifier") for s in ((2, 4, 32, 32), (3, 4, 16, 48), (1, 4, 224, 224))]


@pytest.mark.parametrize("kind,shape", HEAD_CASES, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in HEAD_CASES])
def test_head_matches_float64(kind, shape):
    blocks, final = (2, False) if kind == "projector" else (3, True)
    head = _head(kind, 11)
    sd0 = _np_sd(head)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=g) * 2.0
    xd = x.cuda()
    feat = head.forward_raw(xd).clone()
    plan, norms, pools = _plan_ops(head)
    # the geometry decides the pool path: fused into the normalisation's forward only where W % 8 == 0
    assert [p.fwd_fused for p in pools] == [(shape[3] >> i) % 8 == 0 for i in range(blocks)]
    assert all(p.fused_into is not None for p in pools)
    dfeat = torch.randn(feat.shape, generator=g)
    head.logits_grad_buffer().copy_(dfeat.cuda())
    head.backward_raw()
    gin = head.input_grad_buffer().clone()
    torch.cuda.synchronize()
    assert tuple(gin.shape) == (shape[0], shape[1], 1) + shape[2:] and torch.isfinite(gin).all()
    assert not head.flat_grad.any()                                               # frozen: no parameter gradient is written
    # float64 oracle; the pass's own ReLU / max-pool decisions arbitrate the gradient
    f64, cache = co.head_forward(sd0, x.numpy(), blocks, final)
    dec = _gpu_decisions(head)
    flips = co.check_decisions(cache, dec)
    g64 = co.head_input_grad(dfeat[:, :, 0].numpy(), cache, dec)
    f32, st32, after32, g32 = co.head_torch(sd0, x.numpy(), blocks, final, torch.float32, co.decisions_of(cache),
                                            dfeat[:, :, 0].numpy())
    g64_own = co.head_input_grad(dfeat[:, :, 0].numpy(), cache)
    e_f, e_g = co.rel(f32, f64), co.rel(g32, g64_own)
    h_f, h_g = co.rel(feat[:, :, 0].cpu(), f64), co.rel(gin[:, :, 0].cpu(), g64)
    print(f"\n[head] {kind} {shape}: features e32 {e_f:.2e} hip {h_f:.2e}; input gradient e32 {e_g:.2e} hip {h_g:.2e}; "
          f"decisions that differ from float64: {flips}", end="")
    assert _gate(h_f, e_f), (h_f, e_f)
    assert _gate(h_g, e_g), (h_g, e_g)
    # batch statistics and the running buffers after one train-mode pass
    after = co.running_after(sd0, cache)
    sd1 = _np_sd(head)
    for i, (n, c) in enumerate(zip(norms, cache["blocks"]), start=1):
        std = np.sqrt(c["stats"]["var"])
        scale = (std + np.abs(c["stats"]["mean"])).max()
        h_m = np.abs(n.mean.cpu().numpy() - c["stats"]["mean"]).max() / scale
        e_m = np.abs(st32[i - 1][0].numpy() - c["stats"]["mean"]).max() / scale
        h_r, e_r = co.rel(n.rstd.cpu(), c["rstd"]), co.rel(st32[i - 1][1], c["rstd"])
        assert _gate(h_m, e_m) and _gate(h_r, e_r), (i, h_m, e_m, h_r, e_r)
        for k in ("running_mean", "running_var"):
            key = f"conv_{i}.bn.{k}"
            assert _gate(co.rel(sd1[key], after[key]), co.rel(after32[key], after[key])), key
        assert int(sd1[f"conv_{i}.bn.num_batches_tracked"]) == 1
    for k in sd0:                                                               # nothing else moved
        if "running" not in k and "num_batches" not in k:
            assert np.array_equal(sd0[k], sd1[k]), k
    # a batch-strided view is bound as it is and gives the same bits as the dense tensor
    if shape[0] > 1:
        big = torch.full((2 * shape[0],) + shape[1:], NAN, device="cuda")
        big[0::2] = xd
        assert _same(head.forward_raw(big[0::2]), feat)
        assert plan.inp.t.data_ptr() == big.data_ptr()


def test_frozen_head_launches_no_weight_gradient_and_packs_once():
    from mis_hip import lib
    x = torch.randn((2, 4, 32, 32), device="cuda")

    def names(head, passes=1):
        head.forward_raw(x)                                                      # plans and buffers settle
        head.logits_grad_buffer().fill_(0.25)
        head.backward_raw()
        tape = lib.LaunchTape()
        with tape.recording():
            for _ in range(passes):
                head.forward_raw(x)
                head.backward_raw()
        torch.cuda.synchronize()
        return [getattr(fn, "__name__", "") for fn, _ in tape.items]

    for kind in ("classifier", "projector"):
        frozen = names(_head(kind, 5), passes=2)
        assert frozen and all(n.startswith("mis_") or n.startswith("hip") for n in frozen)
        assert not [n for n in frozen if "wgrad" in n or "channel_sum" in n or "pack" in n], frozen
        assert sum("conv" in n for n in frozen) >= 2 * 2 * (2 if kind == "projector" else 3)      # forward + data gradient
        live = _head(kind, 5)
        live.frozen = False                                                      # the same head with weight gradients on
        assert live.weights_version == 1
        thawed = names(live)
        assert [n for n in thawed if "wgrad" in n] and [n for n in thawed if "pack" in n]
        assert live.flat_grad.any()
    # a load makes the frozen head pack again, once
    h = _head("projector", 5)
    first = h.forward_raw(x).clone()
    sd = h.state_dict()
    sd["conv_1.conv.weight"] = sd["conv_1.conv.weight"] * 2.0
    h.load_state_dict(sd)
    assert not _same(h.forward_raw(x), first)


# ---------------------------------------------------------------------------------------------------------------------
# the tail
# ---------------------------------------------------------------------------------------------------------------------
def _state(w):
    ops = _ops()
    st = ops.new_step_state()
    ops.contrastive_step_init(st, 1, 500, 0.01, 1000, w, 0.0, 10)               # rampup 0: cons_weight = (float)w
    return st


def _launch(c, x, layout, wmode="float", grad=True):
    ops = _ops()
    own, other, label, el, eu = x
    vo, vt = kit.place_rows(own, layout, PAD)[1], kit.place_rows(other, layout, PAD)[1]
    ve = [None if e is None else kit.place_rows(e, layout, PAD)[1] for e in (el, eu)]
    out = torch.full((16,), NAN, device="cuda")
    d = kit.place_rows(None, layout, PAD, like=own) if grad else None
    ops.scratch(1, "tail").view(torch.float32).fill_(NAN)
    wkw = dict(cons_weight=c["w"]) if wmode == "float" else dict(state=_state(c["w"]))
    ops.contrastive_cross_tail(vo, vt, label.cuda(), c["L"], out, dlogits=d and d[1], extra_l=ve[0], extra_u=ve[1], **wkw)
    torch.cuda.synchronize()
    return out, d


@pytest.mark.parametrize("c", co.matrix(), ids=co.cid)
def test_contrastive_tail_matches_float64(c):
    x, out64, d64, es, et = co.reference_case(c)
    L = c["L"]
    out, d = _launch(c, x, c["layout"])
    assert torch.isfinite(out[:6]).all() and torch.isnan(out[6:]).all(), out           # six scalars and nothing else
    buf, view = d
    assert torch.isfinite(view).all() and kit.untouched_outside(buf, view)                # every element once, nothing else
    got = out[:6].cpu().double()
    hs = co.scalar_rels(got, out64)
    ht = co.rel(view.cpu(), d64)
    print(f"\n[contrastive tail] {co.cid(c)}: scalars e32 {max(es):.2e} hip {max(hs):.2e}  dlogits e32 {et:.2e} hip {ht:.2e}",
          end="")
    STATS.append(dict(case=co.cid(c), e32_scalar=max(es), hip_scalar=max(hs), e32_tensor=et, hip_tensor=ht,
                      e32_scalars=es, hip_scalars=hs))
    for i in range(6):
        if out64[i] == 0:
            assert got[i].item() == 0, (i, got[i].item())
        else:
            assert hs[i] <= max(co.K * es[i], co.FLOOR_SCALAR), (_ops().CONTRASTIVE_OUT[i], got[i].item(), out64[i], hs[i], es[i])
    assert got[4].item() == float(torch.tensor(c["w"], dtype=torch.float32))
    assert ht <= max(co.K * et, co.FLOOR_TENSOR), (ht, et)
    # the rows without a head gradient carry the tail gradient alone: the same bits as a launch without extras
    if c["extra"]:
        plain = _launch(c, x[:3] + (None, None), c["layout"])
        assert _same(out, plain[0])
        assert torch.equal(view[1:L:2], plain[1][1][1:L:2])
        assert not torch.equal(view[0:L:2], plain[1][1][0:L:2])
        if c["B"] > L:
            assert not torch.equal(view[L:], plain[1][1][L:])
    if c["w"] == 0 and not c["extra"]:
        assert not view[L:].any()                                                  # w = 0: no pseudo-label gradient
    # bit-reproducible; scalars alone; addresses only; the weight from the device state
    out2, d2 = _launch(c, x, c["layout"])
    assert _same(out, out2) and _same(buf, d2[0])
    if not c["extra"]:
        assert _same(out, _launch(c, x, c["layout"], grad=False)[0])
    if c["layout"] != "dense":
        outd, dd = _launch(c, x, "dense")
        assert _same(out, outd) and torch.equal(view, dd[1])
    outs, ds = _launch(c, x, c["layout"], wmode="state")
    assert _same(out, outs) and _same(buf, ds[0])


def test_contrastive_tail_refuses_bad_geometry_without_launching():
    from mis_hip import lib
    ops = _ops()
    L = lib.load()
    B, C, S = 6, 4, 64
    z = torch.randn((B, C, S), device="cuda")
    lab = torch.zeros((B, S), dtype=torch.uint8, device="cuda")
    out = torch.full((16,), NAN, device="cuda")
    d = torch.full((B, C, S), NAN, device="cuda")
    ws = ops.scratch(L.mis_contrastive_cross_tail_workspace_bytes(B, C, S), "tail")
    P = lib.ptr

    def call(own=z, other=z, label=lab, lb=1, B=B, Lb=4, C=C, S=S, bs=C * S, el=None, eu=None, o=out, dl=d, w=ws, wsb=None):
        return L.mis_contrastive_cross_tail(P(own), bs, P(other), bs, P(label), lb, B, Lb, C, S, 2.0, 1.25, 0.1, None,
                                            P(el), bs, P(eu), bs, 1.0, P(o), P(dl), bs, P(w),
                                            ws.numel() if wsb is None else wsb, lib.stream_ptr())

    assert call(Lb=3) == -1 and call(Lb=5) == -1 and call(Lb=0) == -1 and call(Lb=8) == -1      # odd L, L < 2, L > B
    assert call(own=None) == -1 and call(other=None) == -1 and call(label=None) == -1 and call(o=None) == -1
    assert call(w=None) == -1 and call(el=z, dl=None) == -1 and call(eu=z, dl=None) == -1
    assert call(lb=4) == -1 and call(S=0) == -1 and call(bs=C * S - 1) == -1
    assert call(C=5, S=32) == -2 and call(C=1) == -2                                              # MIS_ERR_UNSUPPORTED
    assert call(wsb=64) == -4                                                                     # MIS_ERR_WORKSPACE
    assert L.mis_contrastive_cross_tail_workspace_bytes(B, 9, S) == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(d).all()
    assert call() == 0 and call(Lb=6, other=None) == 0                                            # L = B needs no other
    torch.cuda.synchronize()
    assert torch.isfinite(out[:6]).all() and torch.isfinite(d).all()
    from mis_hip.step import ContrastiveCrossTrainer
    with pytest.raises(ValueError):                                                # an odd labeled_bs: before any launch
        ContrastiveCrossTrainer(None, None, None, None, None, None, labeled_bs=3, num_classes=4, iters_per_epoch=2)


# ---------------------------------------------------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------------------------------------------------
SCHED = dict(base_lr=0.01, max_iterations=8, consistency=0.1, rampup=3, iters_per_epoch=2)


def test_schedule_kernel_follows_the_host_restatement():
    ops = _ops()
    st = ops.new_step_state()
    ops.contrastive_step_init(st, 9, 0, **SCHED)
    lit = co.literal_schedule(8, 0.01, 8, 0.1, 3, 2)
    for k in range(9):
        s = ops.read_step_state(st)
        lr, w = ops.contrastive_schedule(k, **SCHED)
        assert s["iter_num"] == k and s["offset"] == k and s["seed"] == 9 and s["cons_gate"] == 1.0
        assert s["lr"] == float(np.float32(lr)) or abs(s["lr"] - lr) <= 2 ** -23 * lr, (k, s["lr"], lr)
        assert s["cons_weight"] == float(np.float32(w)) or abs(s["cons_weight"] - w) <= 2 ** -23 * w, (k, s["cons_weight"], w)
        if k < 8:
            assert (lr, w) == lit[k]
        ops.contrastive_step_advance(st, **SCHED)
    # started in the middle of a run: the same state as advancing to it
    st2 = ops.new_step_state()
    ops.contrastive_step_init(st2, 9, 6, **SCHED)
    for _ in range(3):
        ops.contrastive_step_advance(st2, **SCHED)
    assert torch.equal(st, st2)


# ---------------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------------
def _students(seed=0, filler_sd=True):
    from networks.net_factory import net_factory
    from oracle import filler
    from oracle.nets import OracleUNet2D
    torch.manual_seed(seed)
    nets, sds = [], []
    for m in range(2):
        net = net_factory("unet", 1, 4)
        if filler_sd:
            sd = filler.fill_state_dict({f"m{m}." + k: v.clone() for k, v in OracleUNet2D(1, 4).new_state().items()})
            sd = {k.split(".", 1)[1]: v for k, v in sd.items()}
            net.load_state_dict(sd)
            sds.append(sd)
        net.train()
        net.dropout_enabled = False
        nets.append(net)
    return nets, sds


def _heads(seed=20):
    return [_head(k, seed + i, plain=True) for i, k in enumerate(("classifier", "classifier", "projector", "projector"))]


def _batch(B=6, hw=32):
    from oracle import filler
    return filler.image((B, 1, hw, hw), "volume").cuda(), filler.labels((B, hw, hw), 4, torch.uint8).cuda()


def _whole_step_e32(z1, z2, label, L, w, heads_sd, r):
    """fp32 CPU torch evaluation of the whole loss at these logits (float64 decisions in the heads): the e32 of every
    scalar of ``losses()`` and of both logits gradients, against the float64 result ``r``."""
    f32 = torch.float32
    c = co.SCALES["contrastive"]
    t1, t2 = torch.from_numpy(z1).float(), torch.from_numpy(z2).float()
    spec = [("classifier_1", z1[:L][0::2], 3, True), ("classifier_2", z2[:L][1::2], 3, True),
            ("projector_1", z1[L:], 2, False), ("projector_2", z2[L:], 2, False)]
    feats = {n: co.head_torch(heads_sd[n], x, b, f, f32, co.decisions_of(r["caches"][n]))[0] for n, x, b, f in spec}
    ol, gl = pno.loss_and_grad(feats["classifier_1"], feats["classifier_2"], dtype=f32, grad_scale=c)
    ou, gu = pno.loss_and_grad(feats["projector_1"], feats["projector_2"], dtype=f32, grad_scale=c)
    el = co.head_torch(heads_sd["classifier_1"], z1[:L][0::2], 3, True, f32, co.decisions_of(r["caches"]["classifier_1"]),
                       gl.numpy())[3]
    eu = co.head_torch(heads_sd["projector_1"], z1[L:], 2, False, f32, co.decisions_of(r["caches"]["projector_1"]),
                       gu.numpy())[3]
    lab = torch.from_numpy(label)
    o1, d1 = co.tail_torch(t1.unsqueeze(2), t2.unsqueeze(2), lab, L, w, f32, el.unsqueeze(2), eu.unsqueeze(2))
    o2, d2 = co.tail_torch(t2.unsqueeze(2), t1.unsqueeze(2), lab, L, w, f32)
    s32 = dict(loss=(o1[0] + o2[0] + c * (ol[0] + ou[0])).item(), model1_loss=o1[5].item(), model2_loss=o2[5].item(),
               con_loss=(ol[0] + ou[0]).item(), c_loss_l=ol[0].item(), c_loss_u=ou[0].item())
    s64 = dict(loss=r["loss"], model1_loss=r["model1_loss"], model2_loss=r["model2_loss"], con_loss=r["Lc_l"] + r["Lc_u"],
               c_loss_l=r["Lc_l"], c_loss_u=r["Lc_u"])
    e = {k: abs(s32[k] - s64[k]) / abs(s64[k]) for k in s64}
    return e, s64, co.rel(d1[:, :, 0], r["dz1"]), co.rel(d2[:, :, 0], r["dz2"])


def _gpu_signs(net):
    """the branch every LeakyReLU of the network's last pass took, per normalisation op in plan order == the oracle's order"""
    return [(op.y.t[:, :, 0] > 0).cpu() for op in net._last[0].ops if type(op).__name__ == "NormActOp"]


def _flat_grads(sd, volume, dlogits, dtype, signs=None, keep=()):
    """Per-parameter gradients of a UNet for a given logits gradient: the oracle network under autograd in ``dtype``.
    ``signs``: every LeakyReLU takes the branch a pass took (oracle.nets.PRE_ACT); where that is not the branch of this
    evaluation the pre-activation x becomes x - 2 * x.detach(): the value changes sides, d/dx stays +1, so the unit gets the
    other branch's slope and nothing else changes.  (Multiplying x by -1 instead, as tests/test_parity_gpu.py's
    _flipped_solutions does, also negates the derivative: the reversed unit then contributes -slope, and the solution moves
    AWAY from an implementation that took that branch by as much as it should move towards it.)  ``keep``: (site, index)
    of units left on this evaluation's own branch.  Returns (gradients, logits, [(site, index, margin)] of the reversals)."""
    from oracle import nets
    net = nets.OracleUNet2D(1, 4)
    work = {n: (t.detach().to(dtype).clone().requires_grad_(True) if net.is_param(n) else t.detach().clone().to(
        dtype if t.is_floating_point() else t.dtype)) for n, t in sd.items()}
    state, found = dict(i=0), []

    def hook(x):
        i = state["i"]
        state["i"] += 1
        v = x.detach()
        diff = (v > 0) != signs[i]
        if not diff.any():
            return x
        idx = diff.flatten().nonzero().flatten().tolist()
        found.extend((i, j, float(v.flatten()[j].abs() / v.abs().max())) for j in idx)
        for j in idx:
            if (i, j) in keep:
                diff.view(-1)[j] = False
        return torch.where(diff, x - 2 * v, x)

    nets.PRE_ACT = hook if signs is not None else None
    try:
        out = net.forward(work, volume.to(dtype), training=True, drop="off")
    finally:
        nets.PRE_ACT = None
    assert signs is None or state["i"] == len(signs)
    names = [n for n in work if net.is_param(n)]
    grads = torch.autograd.grad(out, [work[n] for n in names], torch.as_tensor(dlogits).to(dtype))
    return dict(zip(names, grads)), out.detach(), found


def _score_flat_grads(net, sd, volume, dlogits, signs):
    """Worst (error / tolerance) of the network's flat gradient per tensor, by the gate of tests/test_cross_teaching_gpu.py:
    tolerance (6 * e32 + 2e-3) * |ref|max + 5e-4 * (largest gradient entry), e32 = the oracle network in fp32 against
    float64.  Six images of 32 x 32 put pre-activations within fp32 rounding of zero (margins of 1e-7 .. 1e-6 of their
    layer's maximum), and one such LeakyReLU on the other branch moves whole decoder tensors by several per cent of their
    maximum: any fp32 implementation lands on either side (the oracle network in fp32 does under a 6e-8 perturbation of the
    input).  So the float64 and the fp32 evaluation take the branches the GPU pass took (``signs``), which may differ from
    float64's own only at pre-activations float64 has within 1e-5 of zero, at most 6 of them.  The kernels' backward forms
    the sign again from x, in another order of operations than the forward: if the forward's branches do not fit, the
    subsets of those few units left on float64's branch are evaluated too, exactly, and EVERY tensor is held to the normal
    tolerance against ONE of these solutions."""
    import itertools
    names = [n for n, _ in net.named_flat(net.flat_grad)]
    hip = {n: g.cpu().double() for n, g in net.named_flat(net.flat_grad)}

    def score(keep):
        g64, _, found = _flat_grads(sd, volume, dlogits, torch.float64, signs, keep)
        g32 = _flat_grads(sd, volume, dlogits, torch.float32, signs, keep)[0]
        gscale = max(float(g.abs().max()) for g in g64.values())
        rows = []
        for n in names:
            e32 = co.rel(g32[n], g64[n])
            tol = (co.K * e32 + 2e-3) * float(g64[n].abs().max()) + 5e-4 * gscale
            rows.append(((hip[n] - g64[n]).abs().max().item() / tol, n, e32))
        return max(rows), found

    worst, found = score(())
    assert len(found) <= 6 and all(m <= 1e-5 for _, _, m in found), found
    kept = ()
    if worst[0] > 1.0:
        units = [(i, j) for i, j, _ in found]
        for k in range(1, len(units) + 1):
            for keep in itertools.combinations(units, k):
                w = score(frozenset(keep))[0]
                if w[0] < worst[0]:
                    worst, kept = w, keep
            if worst[0] <= 1.0:
                break
    return worst, found, kept


def test_step_matches_oracle_and_torch_update():
    """Two UNets at [6, 1, 32, 32], L = 4, dropout off, one eager step: scalars, both logits gradients, the SGD update, the
    untouched heads and the flat gradients per tensor."""
    from mis_hip.step import ContrastiveCrossTrainer
    ops = _ops()
    L = 4
    (m1, m2), sds = _students()
    heads = _heads()
    heads_sd = {n: _np_sd(h) for n, h in zip(HEADS, heads)}
    vol, lab = _batch()
    cfg = dict(base_lr=0.01, max_iterations=30000, consistency=0.1, consistency_rampup=200.0)
    tr = ContrastiveCrossTrainer(m1, m2, *heads, labeled_bs=L, num_classes=4, iters_per_epoch=3, iter_num=300,
                                 use_tape=False, **cfg)
    st0 = ops.read_step_state(tr.state)
    lr0, w0 = ops.contrastive_schedule(300, 0.01, 30000, 0.1, 200.0, 3)
    assert st0["iter_num"] == 300 and abs(st0["lr"] - lr0) <= 1e-9 and abs(st0["cons_weight"] - w0) <= 1e-9
    p0 = [m.flat_param.clone() for m in (m1, m2)]
    hp0 = [h.flat_param.clone() for h in heads]
    tr.step(vol, lab)
    torch.cuda.synchronize()
    got = tr.losses()
    z = [m._last[0].out.t[:, :, 0].detach().cpu().double().numpy() for m in (m1, m2)]
    dz = [m.logits_grad_buffer()[:, :, 0].detach().cpu().double() for m in (m1, m2)]
    w = st0["cons_weight"]
    r = co.loss_and_grads(z[0], z[1], lab[:L].cpu().numpy(), L, w, heads_sd)
    # the query-side heads' own ReLU / max-pool decisions arbitrate the gradient that reaches student 1
    dec = {"classifier_1": _gpu_decisions(heads[0]), "projector_1": _gpu_decisions(heads[2])}
    for n, d in dec.items():
        co.check_decisions(r["caches"][n], d)
    own = co.loss_and_grads(z[0], z[1], lab[:L].cpu().numpy(), L, w, heads_sd, decisions=dec)
    e, s64, e_d1, e_d2 = _whole_step_e32(z[0], z[1], lab[:L].cpu().numpy(), L, w, heads_sd, r)
    r["dz1"] = own["dz1"]
    for k in s64:
        h = abs(got[k] - s64[k]) / abs(s64[k])
        print(f"\n[step] {k}: f64 {s64[k]:.9f} hip {got[k]:.9f} rel {h:.2e} e32 {e[k]:.2e}", end="")
        assert h <= max(co.K * e[k], co.FLOOR_SCALAR), (k, got[k], s64[k], h, e[k])
    assert got["consistency_weight"] == w and abs(got["lr"] - ops.contrastive_schedule(301, 0.01, 30000, 0.1, 200.0, 3)[0]) <= 1e-9
    for m, (ed, key) in enumerate(((e_d1, "dz1"), (e_d2, "dz2"))):
        h = co.rel(dz[m], r[key])
        print(f"\n[step] {key}: hip {h:.2e} e32 {ed:.2e}", end="")
        assert h <= max(co.K * ed, co.FLOOR_TENSOR), (key, h, ed)
    # only student 1 carries the head gradients: its rows 1 and 3 and all of student 2 are the tail gradient alone
    chk = torch.zeros(16, device="cuda")
    d2 = torch.empty_like(m2.logits_grad_buffer())
    ops.contrastive_cross_tail(m2._last[0].out.t, m1._last[0].out.t, lab[:L].contiguous(), L, chk, dlogits=d2, cons_weight=w)
    assert _same(d2, m2.logits_grad_buffer()) and _same(chk[:6], tr.out2[:6])
    # SGD (momentum 0.9, wd 1e-4) on the kernel's own gradients; the heads never move
    for m, (net, mom) in enumerate(((m1, tr.mom1), (m2, tr.mom2))):
        g = net.flat_grad.double()
        mo = g + 1e-4 * p0[m].double()
        p1 = p0[m].double() - st0["lr"] * mo
        assert (mom.double() - mo).abs().max().item() <= 1e-6 * max(mo.abs().max().item(), 1e-3)
        assert (net.flat_param.double() - p1).abs().max().item() <= 1e-6 * p0[m].abs().max().item()
    for h, before in zip(heads, hp0):
        assert torch.equal(h.flat_param, before) and not h.flat_grad.any()
        assert all(int(v) == 1 for k, v in h.state_dict().items() if k.endswith("num_batches_tracked"))
    st1 = ops.read_step_state(tr.state)
    assert st1["iter_num"] == 301 and tr.iter_num == 301
    # flat gradients: per tensor, against the oracle network fed the oracle's logits gradient
    for m, net in enumerate((m1, m2)):
        lg = _flat_grads(sds[m], vol.cpu(), r[f"dz{m + 1}"], torch.float64)[1]
        assert (torch.from_numpy(z[m]) - lg).abs().max().item() <= 1e-3
        worst, found, kept = _score_flat_grads(net, sds[m], vol.cpu(), r[f"dz{m + 1}"], _gpu_signs(net))
        print(f"\n[step] model{m + 1} flat gradient: worst error / tolerance {worst[0]:.3f} at {worst[1]} (e32 {worst[2]:.2e}); "
              f"LeakyReLU branches the pass took against float64's: {len(found)} (margins {['%.1e' % x for _, _, x in found]})"
              + (f", {len(kept)} of them left on float64's branch" if kept else ""), end="")
        assert worst[0] <= 1.0, (m, worst, found, kept)


def _run_steps(steps, use_tape, seed=7):
    from mis_hip.step import ContrastiveCrossTrainer
    (m1, m2), _ = _students(seed=3, filler_sd=False)
    m1.dropout_enabled = m2.dropout_enabled = True
    heads = _heads()
    vol, lab = _batch()
    tr = ContrastiveCrossTrainer(m1, m2, *heads, labeled_bs=4, num_classes=4, iters_per_epoch=2, base_lr=0.01,
                                 max_iterations=8, consistency=0.1, consistency_rampup=3, seed=seed, use_tape=use_tape)
    outs, states = [], []
    for i in range(steps):
        tr.step(vol if i % 2 == 0 else vol.flip(0).contiguous(), lab)
        outs.append(torch.cat([tr.out1[:6], tr.out2[:6], tr.out_cl[:3], tr.out_cu[:3]]).clone())
        states.append(tr.state.clone())
    torch.cuda.synchronize()
    nets = [m1, m2] + heads
    return dict(out=torch.stack(outs), state=torch.stack(states), params=[n.flat_param.clone() for n in nets],
                bufs=[b.clone() for n in nets for b in n.buffers()], tape=tr._tape is not None,
                sched=[_ops().read_step_state(s) for s in states])


def test_tape_and_eager_are_bit_identical_across_epochs_and_the_lr_switch():
    taped, eager = _run_steps(8, True), _run_steps(8, False)
    assert taped["tape"] and not eager["tape"]
    assert torch.equal(taped["out"], eager["out"]) and torch.equal(taped["state"], eager["state"])
    assert all(torch.equal(a, b) for a, b in zip(taped["params"], eager["params"]))
    assert all(torch.equal(a, b) for a, b in zip(taped["bufs"], eager["bufs"]))
    assert torch.isfinite(taped["out"]).all()
    # the replayed steps (4 .. 8) saw the schedule move: an epoch boundary every second step, the 1e-4 rule from step 7 on
    for k, s in enumerate(taped["sched"], start=1):
        lr, w = _ops().contrastive_schedule(k, **SCHED)
        assert s["iter_num"] == k and abs(s["lr"] - lr) <= 1e-6 * lr and abs(s["cons_weight"] - w) <= 1e-6 * w
    ws = taped["out"][:, 4]
    assert ws[0] == ws[1] != ws[2] and ws[4] != ws[3] and ws[6] == ws[7]
    assert taped["sched"][4]["lr"] > 1e-3 > 1.1e-4 > taped["sched"][5]["lr"]


def test_step_with_the_swin_student():
    """UNet + SwinUnet at the geometry of tests/test_cross_teaching_gpu.py (224 x 224, the lite configuration): the step
    runs and its scalars equal the oracle's on its own logits.  (Not pinned against a real-reference golden.)"""
    from config import lite_config
    from mis_hip.step import ContrastiveCrossTrainer
    from networks.net_factory import net_factory
    from networks.vision_transformer import SwinUnet
    ops = _ops()
    torch.manual_seed(1)
    m1 = net_factory("unet", 1, 4)
    m2 = SwinUnet(lite_config(), img_size=224, num_classes=4)
    for m in (m1, m2):
        m.train()
        m.dropout_enabled = False
    heads = _heads()
    heads_sd = {n: _np_sd(h) for n, h in zip(HEADS, heads)}
    vol, lab = _batch(B=3, hw=224)
    L = 2
    tr = ContrastiveCrossTrainer(m1, m2, *heads, labeled_bs=L, num_classes=4, iters_per_epoch=5, iter_num=50, use_tape=False)
    w = ops.read_step_state(tr.state)["cons_weight"]
    tr.step(vol, lab)
    torch.cuda.synchronize()
    got = tr.losses()
    assert all(np.isfinite(v) for v in got.values()), got
    z = [m._last[0].out.t[:, :, 0].detach().cpu().double().numpy() for m in (m1, m2)]
    r = co.loss_and_grads(z[0], z[1], lab[:L].cpu().numpy(), L, w, heads_sd)
    e, s64, e_d1, e_d2 = _whole_step_e32(z[0], z[1], lab[:L].cpu().numpy(), L, w, heads_sd, r)
    for k in s64:
        h = abs(got[k] - s64[k]) / abs(s64[k])
        print(f"\n[swin step] {k}: f64 {s64[k]:.9f} hip {got[k]:.9f} rel {h:.2e} e32 {e[k]:.2e}", end="")
        assert h <= max(co.K * e[k], co.FLOOR_SCALAR), (k, got[k], s64[k], h, e[k])
    assert torch.isfinite(m1.flat_grad).all() and torch.isfinite(m2.flat_grad).all() and m2.flat_grad.any()


# ---------------------------------------------------------------------------------------------------------------------
# data parallel: two gloo ranks on the same batch == one process
# ---------------------------------------------------------------------------------------------------------------------
def _cc_worker(rank, world, store, out_dir):
    for p in (PKG, ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=world)
    from networks.net_factory import net_factory
    from mis_hip.step import ContrastiveCrossTrainer
    torch.manual_seed(5)
    m1, m2 = net_factory("unet", 1, 4), net_factory("unet", 1, 4)
    torch.manual_seed(9 + rank)                                  # rank 1's heads start elsewhere: the broadcast must fix that
    heads = [net_factory(k) for k in ("classifier", "classifier", "projector", "projector")]
    for n in [m1, m2] + heads:
        n.train()
    g = torch.Generator(device="cuda").manual_seed(100)          # the same batch on every rank
    vol = torch.rand((6, 1, 32, 32), generator=g, device="cuda")
    lab = torch.randint(0, 4, (6, 32, 32), generator=g, device="cuda").to(torch.uint8)
    tr = ContrastiveCrossTrainer(m1, m2, *heads, labeled_bs=4, num_classes=4, iters_per_epoch=2, max_iterations=8,
                                 consistency_rampup=3, seed=7)
    for _ in range(4):                                           # the fourth step is a replay of the tape
        tr.step(vol, lab)
    torch.cuda.synchronize()
    torch.save(dict(p1=m1.flat_param.cpu(), p2=m2.flat_param.cpu(), heads=[h.flat_param.cpu() for h in heads],
                    out=torch.cat([tr.out1[:6], tr.out_cl[:1], tr.out_cu[:1]]).cpu(), tape=tr._tape is not None),
               os.path.join(out_dir, f"cc_{world}_{rank}.pt"))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_gloo_ranks_match_one_process(tmp_path):
    mp.spawn(_cc_worker, args=(1, None, str(tmp_path)), nprocs=1, join=True)
    mp.spawn(_cc_worker, args=(2, str(tmp_path / "gloo_store"), str(tmp_path)), nprocs=2, join=True)
    r = {k: torch.load(os.path.join(tmp_path, f"cc_{k}.pt")) for k in ("1_0", "2_0", "2_1")}
    assert all(v["tape"] for v in r.values())
    for key in ("p1", "p2", "out"):                              # (g + g) / 2 == g bit for bit
        assert torch.equal(r["2_0"][key], r["2_1"][key]) and torch.equal(r["2_0"][key], r["1_0"][key]), key
    for a, b, c in zip(r["1_0"]["heads"], r["2_0"]["heads"], r["2_1"]["heads"]):
        assert torch.equal(a, b) and torch.equal(a, c)


# ---------------------------------------------------------------------------------------------------------------------
# command lines
# ---------------------------------------------------------------------------------------------------------------------
def _cli(script, tmp_path, extra):
    work = tmp_path / "code"
    work.mkdir(exist_ok=True)
    cmd = [sys.executable, os.path.join(PKG, script), "--root_path", str(tmp_path / "no_data"), "--exp", "cc_cli",
           "--max_iterations", "4", "--zip", "--amp-opt-level", "O0", "--tag", "t"] + extra
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run(cmd, cwd=work, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Training Finished!" in r.stdout and "itr 4, loss " in r.stdout + r.stderr
    return work, env


def test_cnn_cli_trains_and_its_checkpoint_loads(tmp_path):
    work, env = _cli("train_Contrastive_Cross_CNN_2D.py", tmp_path, ["--batch_size", "6", "--labeled_bs", "4",
                                                                      "--patch_size", "32", "32"])
    snap = tmp_path / "model" / "cc_cli_14_labeled" / "unet"
    scal = (snap / "scalars.csv").read_text()
    for tag in ("4,lr,", "4,consistency_weight/consistency_weight,", "4,loss/model1_loss,", "4,loss/model2_loss,",
                "4,loss/c_loss_u,"):
        assert tag in scal, tag
    from networks.net_factory import net_factory
    for i in (1, 2):
        net_factory("unet", 1, 4).load_state_dict(torch.load(str(snap / f"unet_best_model{i}.pth")))
    # the inference command line reads ``{model}_best_model.pth``: hand it student 1, as a user of the reference would
    rng = np.random.default_rng(0)
    acdc = tmp_path / "data" / "ACDC"
    (acdc / "data").mkdir(parents=True)
    np.savez(acdc / "data" / "patient001_frame01.npz", image=rng.random((2, 40, 48)).astype(np.float32),
             label=rng.integers(0, 4, (2, 40, 48)).astype(np.uint8))
    (acdc / "test.list").write_text("patient001_frame01.h5\n")
    os.replace(snap / "unet_best_model1.pth", snap / "unet_best_model.pth")
    r = subprocess.run([sys.executable, os.path.join(PKG, "test_2D_fully.py"), "--root_path", str(acdc), "--exp", "cc_cli",
                        "--labeled_num", "14"], cwd=work, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    dice = eval(r.stdout.strip().splitlines()[-1])
    assert len(dice) == 3
    # an odd --labeled_bs is refused before any device work
    bad = subprocess.run([sys.executable, os.path.join(PKG, "train_Contrastive_Cross_CNN_2D.py"), "--batch_size", "6",
                          "--labeled_bs", "3"], cwd=work, env=env, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "even labeled_bs" in bad.stderr


def test_cnn_vit_cli_trains(tmp_path):
    _cli("train_Contrastive_Cross_CNN_ViT_2D.py", tmp_path, ["--batch_size", "3", "--labeled_bs", "2"])
    snap = tmp_path / "model" / "cc_cli_14_labeled" / "unet"
    assert (snap / "unet_best_model1.pth").exists() and (snap / "unet_best_model2.pth").exists()
    from networks.net_factory import net_factory
    net_factory("ViT_Seg", 1, 4).load_state_dict(torch.load(str(snap / "unet_best_model2.pth")))
