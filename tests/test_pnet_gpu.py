"""PNet2D (networks/pnet.py, ``--model pnet``) on the device against the golden of the real reference
(tests/golden/pnet_40x24.npz) and the float64 oracle (tests/pnet_oracle.py), with the constants of tests/test_parity_gpu.py:

    logits:        |hip - f64|max <= F64_LOGIT
    per gradient:  |g_hip - g64|max <= max(F64_K * e32, F64_REL) * |g64|max + F64_ABS * (largest |g64| of the net)
    all gradients: median of (HIP relative error / e32) <= F64_MEDIAN_RATIO   (tensors above 1e-4 of the largest gradient)
    running buffers: the ``stat`` rule of tests/test_norm_edges_gpu.py, max(K * e32, FLOOR["stat"]) of the tensor's largest value

e32 = the reference's own fp32 (one thread) against float64, stored in the golden per tensor.  The golden's geometry
[3, 1, 40, 24] gives the dilated layers 3- and 2-row phases at d = 16 and ragged ones at d = 8.
"""
import os

import numpy as np
import pytest
import torch

import pnet_oracle as po
import norm_oracle as no
from net_gate import F64_LOGIT, check_grads as _check_grads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [1, 2, 4, 8, 16]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "pnet_40x24.npz"))


def _sd(z):
    return {str(k): torch.from_numpy(z[f"sd/{k}"]) for k in z["keys"]}


def _model(z):
    from networks.pnet import PNet2D
    m = PNet2D(1, 4, 8, RATIOS).cuda()
    m.load_state_dict(_sd(z))
    return m


def test_train_mode_forward_backward_and_eval_forward_match_the_reference(gold):
    m = _model(gold)
    m.train()
    m.dropout_enabled = False
    x = torch.from_numpy(gold["x"].astype(np.float32)).cuda()
    dl = torch.from_numpy(gold["dlogits"].astype(np.float32)).cuda()
    m.flat_grad.fill_(float("nan"))
    # the biases in front of a BatchNorm have an exactly zero gradient that no launch writes: the flat buffer keeps its zeros
    for n, g in m.named_flat(m.flat_grad):
        if ".conv" in n and n.startswith("block") and n.endswith("bias"):
            g.zero_()
    logits = m.forward_raw(x)
    assert tuple(logits.shape) == (3, 4, 1, 40, 24)
    err = float((logits[:, :, 0].cpu().double() - torch.from_numpy(gold["logits"])).abs().max())
    print(f"[pnet] train logits: |hip - f64|max {err:.2e} (reference fp32: {float(gold['e32_logits']):.2e} relative)")
    assert err <= F64_LOGIT, err
    m.backward_raw(dl.unsqueeze(2).contiguous())
    torch.cuda.synchronize()
    params = [str(k) for k in gold["keys"] if po.is_param(str(k))]
    _check_grads(m, {k: torch.from_numpy(gold[f"grad/{k}"]) for k in params}, {k: float(gold[f"e32/{k}"]) for k in params}, "pnet golden")
    sd = m.state_dict()
    for k in (str(k) for k in gold["keys"] if not po.is_param(str(k))):
        ref = torch.from_numpy(gold[f"after/{k}"])
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(ref) == 1
            continue
        tol = max(no.K * float(gold[f"e32_after/{k}"]), no.FLOOR_STAT)
        e = float((sd[k].cpu().double() - ref).abs().max() / ref.abs().max())
        assert e <= tol, (k, e, tol)
    m.eval()
    ev = m.forward_raw(x, no_backward=True)
    err = float((ev[:, :, 0].cpu().double() - torch.from_numpy(gold["eval_logits"])).abs().max())
    print(f"[pnet] eval logits: |hip - f64|max {err:.2e}")
    assert err <= F64_LOGIT, err


def test_dilated_layers_run_on_the_dilated_kernels_and_take_no_dense_fusion(gold):
    from mis_hip.plan import ConvOp, NormActOp
    m = _model(gold)
    plan = m.plan_for((3, 1, 1, 40, 24))
    convs = [op for op in plan.ops if type(op) is ConvOp]
    assert [op.dilation for op in convs] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 1, 1, 1, 1]
    assert [op.ksize for op in convs] == [(3, 3)] * 10 + [(1, 1)] * 4
    assert not convs[0].need_dx and all(op.need_dx for op in convs[1:])
    for op in convs:
        if op.dilation > 1:
            assert op.wino_f == -1 and op.wino_b == -1 and op.stat is None and op.norm_bwd is None and op.dgrad_norm is None
            assert op.fused_into is None
            norm = plan.ops[plan.ops.index(op) + 1]
            assert type(norm) is NormActOp and norm.x is op.y and norm.fused is None and norm.sums is None
    # the concatenation never runs: the second activation of every block is a channel slice of one buffer
    outs = [plan.ops[plan.ops.index(convs[2 * k + 1]) + 1].y for k in range(5)]
    assert all(o.parent is outs[0].parent and o.c0 == 8 * k for k, o in enumerate(outs))
    assert convs[10].x is outs[0].parent and tuple(convs[10].x.shape) == (3, 40, 1, 40, 24)
    from networks.pnet import PNet2D
    with pytest.raises(RuntimeError):
        PNet2D(1, 4, 8, RATIOS).cuda().forward_raw(torch.zeros(2, 2, 16, 16, device="cuda"))
    with pytest.raises(RuntimeError):
        m.plan_for((2, 1, 4, 16, 16))


def test_fixed_channel_dropout_masks_match_the_oracle(gold):
    m = _model(gold)
    m.train()
    x = torch.from_numpy(gold["x"].astype(np.float32)).cuda()
    dl = torch.from_numpy(gold["dlogits"].astype(np.float32)).cuda()
    plan = m.plan_for((3, 1, 1, 40, 24))
    sites = plan.drop_sites()
    assert len(sites) == 2
    shapes = [plan.drop_site_shape(s) for s in sites]
    assert shapes == [(3, 16, 1, 40, 24), (3, 8, 1, 40, 24)]
    g = torch.Generator().manual_seed(3)
    masks = [(torch.rand((s[0], s[1], 1, 1, 1), generator=g) >= 0.3).float() / 0.7 for s in shapes]
    assert all(0 < float((mk == 0).float().mean()) < 1 for mk in masks)
    m.drop_masks = {s: mk.expand(sh).contiguous().cuda() for s, mk, sh in zip(sites, masks, shapes)}
    logits = m.forward_raw(x)
    m.backward_raw(dl.unsqueeze(2).contiguous())
    torch.cuda.synchronize()
    r = po.run({k: v.double() for k, v in _sd(gold).items()}, gold["x"].astype(np.float64), gold["dlogits"].astype(np.float64),
               train=True, masks=[mk[:, :, 0].double() for mk in masks])
    err = float((logits[:, :, 0].cpu().double() - r["logits"]).abs().max())
    assert err <= F64_LOGIT, err
    # e32 of the masked pass is not in the golden: the p = 0 pass's (same layers, same tensors) stands in
    params = [str(k) for k in gold["keys"] if po.is_param(str(k))]
    _check_grads(m, r["grads"], {k: float(gold[f"e32/{k}"]) for k in params}, "pnet masks")


def test_philox_dropout_zeroes_or_scales_whole_feature_maps(gold):
    from mis_hip import ops
    m = _model(gold)
    m.train()
    m.step_state = ops.new_step_state()
    ops.step_init(m.step_state, 11, 0, 0.01, 100, 0.99, 0.1, 200.0)
    x = torch.from_numpy(gold["x"].astype(np.float32)).cuda()
    m.forward_raw(x)
    plan = m.plan_for((3, 1, 1, 40, 24))
    drops = [op for op in plan.ops if getattr(op, "drop_p", 0) > 0]
    assert len(drops) == 2 and all(op.drop3d and op.no_norm for op in drops)
    seen = set()
    for op in drops:
        pre = torch.nn.functional.leaky_relu(op.x.t, 0.01)
        ratio = (op.y.t / pre)[pre.abs() > 1e-20]
        maps = (op.y.t.flatten(2).abs().amax(2) == 0)              # [N, C]: whole feature maps dropped
        live = op.y.t[~maps]
        assert torch.allclose(live, pre[~maps] / 0.7, rtol=1e-6, atol=0)
        assert (ratio.abs() < 1e-30).logical_or((ratio - 1 / 0.7).abs() < 1e-5).all()
        seen.add(bool(maps.any()))
        seen.add(not bool(maps.all()))
    assert seen == {True}


def test_product_width_from_the_factory(gold):
    from networks.net_factory import net_factory
    from networks.pnet import PNet2D
    m = net_factory("pnet", 1, 4)
    assert isinstance(m, PNet2D) and m.num_filters == 64 and m.ratios == RATIOS
    sd = m.state_dict()
    spec = PNet2D.spec(1, 4, 64)
    assert list(sd.keys()) == [n for n, _ in spec] == [str(k) for k in gold["keys"]]      # the fixture's key list, at F = 64
    assert [tuple(v.shape) for v in sd.values()] == [tuple(s) for _, s in spec]
    m.eval()
    y = m(torch.randn(2, 1, 48, 40, device="cuda"))
    assert tuple(y.shape) == (2, 4, 48, 40) and torch.isfinite(y).all()


def _trainer(tape, sd0):
    from mis_hip.step import MeanTeacherTrainer
    from networks.pnet import PNet2D
    m, e = PNet2D(1, 4, 8, RATIOS).cuda(), PNet2D(1, 4, 8, RATIOS).cuda()
    m.load_state_dict(sd0)
    e.load_state_dict(sd0)
    m.train()
    e.train()
    return MeanTeacherTrainer(m, e, labeled_bs=2, num_classes=4, cons_start_iter=0, seed=5, iter_num=1200, use_tape=tape), m, e


def test_taped_mean_teacher_step_is_bit_identical_to_eager_and_records_the_dilated_launches(gold):
    """Student and EMA teacher are PNets at [4, 1, 32, 32], L = 2: an eager and a taped trainer from identical state; the third
    step is the one the taped trainer records, the two after it are replays."""
    sd0 = _sd(gold)
    g = torch.Generator().manual_seed(7)
    batches = [(torch.rand((4, 1, 32, 32), generator=g).cuda(), torch.randint(0, 4, (4, 32, 32), generator=g).to(torch.uint8).cuda())
               for _ in range(5)]
    res = []
    for tape in (False, True):
        tr, m, e = _trainer(tape, sd0)
        losses = []
        for i, (v, l) in enumerate(batches):
            tr.step(v, l)
            losses.append(tr.out.clone())
            if i == 2:
                torch.cuda.synchronize()
                res.append([m.flat_param.clone(), e.flat_param.clone(), tr.momentum_buf.clone()])
        torch.cuda.synchronize()
        assert torch.isfinite(torch.stack(losses)).all()
        res[-1] += [torch.stack(losses), m.flat_param.clone(), e.flat_param.clone(), tr.momentum_buf.clone()]
        if tape:
            names = [getattr(fn, "__name__", "") for fn, _ in tr._tape.items]
            # per recorded step: 8 dilated forwards of the student + 8 of the teacher, 8 data and 8 weight gradients
            assert names.count("mis_conv_dilated_fwd") == 16, names.count("mis_conv_dilated_fwd")
            assert names.count("mis_conv_dilated_dgrad") == 8 and names.count("mis_conv_dilated_wgrad") == 8
    for a, b in zip(*res):
        assert torch.equal(a, b)
