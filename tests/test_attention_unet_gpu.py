"""Attention U-Net (networks/attention_unet.py, ``--model attention_unet``) on the device against the golden of the real
reference (tests/golden/attention_unet_32x16x48.npz) and the float64 oracle (tests/attention_unet_oracle.py), under the rules of
tests/test_pnet_gpu.py with the constants of tests/test_parity_gpu.py:

    logits:        |hip - f64|max <= F64_LOGIT
    per gradient:  |g_hip - g64|max <= max(F64_K * e32, F64_REL) * |g64|max + F64_ABS * (largest |g64| of the net)
    all gradients: median of (HIP relative error / e32) <= F64_MEDIAN_RATIO   (tensors above 1e-4 of the largest gradient)
    running buffers: the ``stat`` rule of tests/test_norm_edges_gpu.py, max(K * e32, FLOOR["stat"]) of the tensor's largest value

e32 = the reference's own fp32 (one thread) against float64, stored in the golden per tensor.  The golden holds the float64
logits at 512 positions (its size cap); they are compared there, and the full tensors with the oracle, which
tests/test_attention_unet_cpu.py pins to the golden at 1e-10.  The geometry [2, 1, 32, 16, 48] puts a coarse extent of 1 into
the level-4 gate (centre 2 x 1 x 3) and an up-sampling by 8 from 4 x 2 x 6 into dsv4.
"""
import os

import numpy as np
import pytest
import torch

import attention_unet_oracle as ao
import norm_oracle as no
from net_gate import F64_LOGIT, check_grads as _check_grads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 1, 32, 16, 48)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "attention_unet_32x16x48.npz"))


@pytest.fixture(scope="module")
def oracle(gold):
    """the float64 oracle's full logits, train mode and -- with the golden's buffers afterwards -- eval mode"""
    sd = _sd(gold)
    x = gold["x"].astype(np.float64)
    train = ao.run(sd, x, train=True)["logits"]
    sd.update({k: torch.from_numpy(gold[f"after/{k}"]) for k in sd if not ao.is_param(k)})
    return train, ao.run(sd, x, train=False)["logits"]


def _sd(z):
    return {str(k): torch.from_numpy(z[f"sd/{k}"]) for k in z["keys"]}


def _model(z):
    from networks.attention_unet import Attention_UNet
    m = Attention_UNet(feature_scale=64, n_classes=2, in_channels=1).cuda()
    m.load_state_dict(_sd(z))
    return m


def _zero_gradient_biases(keys):
    """the biases in front of a normalisation: their gradient is exactly zero and no launch writes it"""
    return [k for k in keys if k.endswith(".bias") and (".conv1.0." in k or ".conv2.0." in k or ".W.0." in k or ".combine_gates.0." in k)]


def test_train_mode_forward_backward_and_eval_forward_match_the_reference(gold, oracle):
    m = _model(gold)
    m.train()
    x = torch.from_numpy(gold["x"].astype(np.float32)).cuda()
    dl = torch.from_numpy(gold["dlogits"].astype(np.float32)).cuda()
    params = [str(k) for k in gold["keys"] if ao.is_param(str(k))]
    zero = set(_zero_gradient_biases(params))
    assert len(zero) == 18 + 1 + 6 + 3
    m.flat_grad.fill_(float("nan"))
    for n, g in m.named_flat(m.flat_grad):      # the flat buffer keeps its zeros where no launch writes
        if n in zero:
            g.zero_()
    idx = torch.from_numpy(gold["logits_idx"])
    logits = m.forward_raw(x)
    assert tuple(logits.shape) == (2, 2, 32, 16, 48)
    got = logits.cpu().double()
    err = float((got.reshape(-1)[idx] - torch.from_numpy(gold["logits"])).abs().max())
    full = float((got - oracle[0]).abs().max())
    print(f"[attention_unet] train logits: |hip - f64|max {err:.2e} at the golden's positions, {full:.2e} over the tensor "
          f"(reference fp32: {float(gold['e32_logits']):.2e} relative)")
    assert err <= F64_LOGIT and full <= F64_LOGIT, (err, full)
    m.backward_raw(dl.contiguous())
    torch.cuda.synchronize()
    e32 = dict(zip(params, (float(v) for v in gold["e32"])))
    _check_grads(m, {k: torch.from_numpy(gold[f"grad/{k}"]) for k in params}, e32, "pnet attention_unet golden")
    sd = m.state_dict()
    buffers = [str(k) for k in gold["keys"] if not ao.is_param(str(k))]
    e32_after = dict(zip([k for k in buffers if not k.endswith("num_batches_tracked")], (float(v) for v in gold["e32_after"])))
    for k in buffers:
        ref = torch.from_numpy(gold[f"after/{k}"])
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(ref) == 1
            continue
        tol = max(no.K * e32_after[k], no.FLOOR_STAT)
        e = float((sd[k].cpu().double() - ref).abs().max() / ref.abs().max())
        assert e <= tol, (k, e, tol)
    m.eval()
    ev = m.forward_raw(x, no_backward=True).cpu().double()
    err = float((ev.reshape(-1)[idx] - torch.from_numpy(gold["eval_logits"])).abs().max())
    full = float((ev - oracle[1]).abs().max())
    print(f"[attention_unet] eval logits: |hip - f64|max {err:.2e} at the golden's positions, {full:.2e} over the tensor")
    assert err <= F64_LOGIT and full <= F64_LOGIT, (err, full)


def _conv_flags(plan):
    from mis_hip.plan import ConvOp, NormActOp
    convs = [op for op in plan.ops if type(op) is ConvOp and op.ksize == (3, 3, 3)]
    flags = []
    for op in convs:
        norm = plan.ops[plan.ops.index(op) + 1]
        assert type(norm) is NormActOp and norm.x is op.y and norm.per_sample
        flags.append((op.cin, op.cout, op.wino_f, op.wino_b, op.stat is not None, op.norm_bwd is not None,
                      op.dgrad_norm is not None, norm.fused is not None, norm.sums is not None, norm.pool is not None,
                      norm.ext_part is not None))
    return flags


def test_product_width_from_the_factory(gold):
    from mis_hip.plan import DownConvOp, GateApplyOp, GateMapOp, UpsampleOp
    from networks.attention_unet import Attention_UNet
    from networks.net_factory_3d import net_factory_3d
    m = net_factory_3d("attention_unet", 1, 2)
    assert isinstance(m, Attention_UNet) and m.filters == [16, 32, 64, 128, 256]
    sd = m.state_dict()
    spec = Attention_UNet.spec(4, 2, 1)
    assert list(sd.keys()) == [n for n, _ in spec] == [str(k) for k in gold["keys"]]      # the fixture's key list, at width 16
    assert [tuple(v.shape) for v in sd.values()] == [tuple(s) for _, s in spec]
    m.train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn((1, 1, 16, 16, 16), generator=g).cuda()
    m.flat_grad.fill_(float("nan"))
    y = m.forward_raw(x)
    assert tuple(y.shape) == (1, 2, 16, 16, 16) and bool(torch.isfinite(y).all())
    m.backward_raw(torch.randn((1, 2, 16, 16, 16), generator=g).cuda())
    torch.cuda.synchronize()
    zero = set(_zero_gradient_biases([n for n, _ in spec]))
    for n, gr in m.named_flat(m.flat_grad):
        assert n in zero or bool(torch.isfinite(gr).all()), n
    plan = m.plan_for((1, 1, 16, 16, 16))
    maps = [op for op in plan.ops if type(op) is GateMapOp]
    applies = [op for op in plan.ops if type(op) is GateApplyOp]
    assert [tuple(op.att.shape) for op in maps] == [(1, 2, 1, 1, 1), (1, 2, 2, 2, 2), (1, 2, 4, 4, 4)]        # levels 4, 3, 2
    assert [op.Ci for op in maps] == [128, 64, 32] and all(op.G == 2 for op in maps)
    assert [tuple(op.y.shape) for op in applies] == [(1, 256, 2, 2, 2), (1, 128, 4, 4, 4), (1, 64, 8, 8, 8)]
    assert all(a.att is mp.att for a, mp in zip(applies, maps))
    thetas = [op for op in plan.ops if type(op) is DownConvOp]
    assert len(thetas) == 6 and all(op.b is None and op.y.parent is mp.theta for op, mp in zip(thetas, [mp for mp in maps for _ in (0, 1)]))
    assert sorted(op.scale for op in plan.ops if type(op) is UpsampleOp) == [2, 2, 2, 2, 2, 4, 8]
    # the skip of every gated level has four readers, the gated skip lands in the decoder's concat buffer
    for a in applies:
        assert sum(1 for op in plan.ops if getattr(op, "x", None) is a.x) == 4
    # unet_3D's fusions on the UnetConv3 blocks: the same 18 convolutions with the same decisions
    u = net_factory_3d("unet_3D", 1, 2)
    u.dropout_enabled = False
    u.forward_raw(x)
    want, got = _conv_flags(u.plan_for((1, 1, 16, 16, 16))), _conv_flags(plan)
    assert len(got) == 18 and got == want
    with pytest.raises(RuntimeError):
        m.forward_raw(torch.zeros(1, 1, 16, 16, 24, device="cuda"))
    with pytest.raises(RuntimeError):
        m.forward_raw(torch.zeros(1, 2, 16, 16, 16, device="cuda"))


def test_the_fusions_of_the_training_geometry_are_unet_3ds(gold):
    """At a geometry where unet_3D's fusions switch on (64^3: epilogue statistics, data-gradient / norm, the pool inside the norm
    backward, the fused first layer) the UnetConv3 blocks of the two nets take the same decisions.  Plans only: nothing runs."""
    from networks.net_factory_3d import net_factory_3d
    m, u = net_factory_3d("attention_unet", 1, 2), net_factory_3d("unet_3D", 1, 2)
    pm, pu = m.plan_for((2, 1, 64, 64, 64)), u.plan_for((2, 1, 64, 64, 64))
    for p in (pm, pu):
        p._fuse_head()
        p._fuse_dgrad_norm()
    got, want = _conv_flags(pm), _conv_flags(pu)
    print([f[4:] for f in got])
    assert got == want and any(any(f[4:]) for f in got)


def _trainer(tape, sd0):
    from mis_hip.step import MeanTeacherTrainer
    from networks.attention_unet import Attention_UNet
    m, e = (Attention_UNet(feature_scale=64, n_classes=2, in_channels=1).cuda() for _ in (0, 1))
    m.load_state_dict(sd0)
    e.load_state_dict(sd0)
    m.train()
    e.train()
    return MeanTeacherTrainer(m, e, labeled_bs=2, num_classes=2, cons_start_iter=0, seed=5, iter_num=1200, use_tape=tape), m, e


def test_taped_mean_teacher_step_is_bit_identical_to_eager_and_records_the_gate_launches(gold):
    """Student and EMA teacher at [2 + 2, 1, 16, 16, 16]: an eager and a taped trainer from identical state; the third step is
    the one the taped trainer records, the two after it are replays."""
    sd0 = _sd(gold)
    g = torch.Generator().manual_seed(7)
    batches = [(torch.rand((4, 1, 16, 16, 16), generator=g).cuda(),
                torch.randint(0, 2, (4, 16, 16, 16), generator=g).to(torch.uint8).cuda()) for _ in range(5)]
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
            # per recorded step, three gated levels: student + teacher forward, the student's backward; a map launch per gate
            assert names.count("mis_attn_gate_apply_fwd") == 6 and names.count("mis_attn_gate_apply_bwd") == 3
            assert names.count("mis_attn_gate_map_fwd") == 12 and names.count("mis_attn_gate_map_bwd") == 6
            # dsv4 and dsv3 (x8, x4) and the centre's depth-1 doubling
            assert names.count("mis_upsample_int_fwd") == 6 and names.count("mis_upsample_int_bwd") == 3
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_load_state_dict_of_the_references_state_dict_round_trips(gold):
    m = _model(gold)
    sd0, sd = _sd(gold), m.state_dict()
    assert list(sd.keys()) == list(sd0.keys()) and len(sd) == 141
    for k, v in sd0.items():
        assert sd[k].dtype == v.dtype and torch.equal(sd[k].cpu(), v), k
    # the parameters live in the flat buffer, in the reference's order
    off = 0
    for k, v in sd0.items():
        if ao.is_param(k):
            assert torch.equal(m.flat_param[off:off + v.numel()].cpu(), v.reshape(-1)), k
            off += (v.numel() + 3) // 4 * 4
    assert off == m.flat_param.numel()
