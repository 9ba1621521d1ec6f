"""The 2-D adversarial step (mis_hip.step.AdversarialTrainer with networks/discriminator_2d.py) on the GPU: ``unet`` and ``pnet``
at [2 + 2, 1, 32, 32] with FCDiscriminator(4, ndf=8, pool=(1, 1)), ``ViT_Seg`` at [2 + 2, 1, 224, 224] with the reference's
pool.  The kernels themselves are held to the float64 oracle in tests/test_adversarial2d_kernels_gpu.py; here the step is held
to those ops bit for bit (what the student receives, what Adam and SGD do, eager against taped, run against run)."""
import numpy as np
import pytest
import torch

import adversarial2d_oracle as ao

pytestmark = pytest.mark.gpu

B, L, C, NDF = 4, 2, 4, 8
KW = dict(labeled_bs=L, num_classes=C, base_lr=0.01, dan_lr=1e-4, max_iterations=100, consistency=0.1,
          consistency_rampup=1.0, seed=11)       # rampup 1: the consistency weight is 0.1 * exp(-5) > 0 from iteration 0


def _ops():
    from mis_hip import ops
    return ops


def _nets(kind, seed=5):
    from networks.discriminator_2d import FCDiscriminator
    torch.manual_seed(seed)
    if kind == "ViT_Seg":
        from config import lite_config
        from networks.vision_transformer import SwinUnet
        model = SwinUnet(lite_config(), img_size=224, num_classes=C)
        dan = FCDiscriminator(C, ndf=NDF)
    else:
        from networks.net_factory import net_factory
        model = net_factory(kind, 1, C)
        dan = FCDiscriminator(C, ndf=NDF, pool=(1, 1))
    return model.train(), dan.train()


_BATCHES = {}


def _batch(kind):
    size = 224 if kind == "ViT_Seg" else 32
    if size not in _BATCHES:
        img, _, lab = ao.golden_inputs(B, C, size, size)
        _BATCHES[size] = (img.cuda(), lab.cuda())
    return _BATCHES[size]


def _run(kind, steps, use_tape):
    """``steps`` steps from the seeded start; returns what the comparisons need (host copies)."""
    from mis_hip.step import AdversarialTrainer
    model, dan = _nets(kind)
    tr = AdversarialTrainer(model, dan, use_tape=use_tape, **KW)
    outs = []
    for _ in range(steps):
        tr.step(*_batch(kind))
        outs.append((tr.out.clone(), tr.dan_out.clone()))
    torch.cuda.synchronize()
    res = dict(model=model.flat_param.cpu(), dan=dan.flat_param.cpu(), m=tr.adam_m.cpu(), v=tr.adam_v.cpu(),
               step=int(tr.adam_state[0].item()), outs=[(a.cpu(), b.cpu()) for a, b in outs], taped=tr._tape is not None)
    del tr, model, dan
    torch.cuda.empty_cache()
    return res


def _same(a, b):
    return (torch.equal(a["model"], b["model"]) and torch.equal(a["dan"], b["dan"]) and torch.equal(a["m"], b["m"])
            and torch.equal(a["v"], b["v"]) and a["step"] == b["step"]
            and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a["outs"], b["outs"])))


@pytest.mark.parametrize("kind", ["unet", "pnet"])
def test_one_step_is_its_separately_tested_pieces_bit_for_bit(kind):
    from mis_hip.step import AdversarialTrainer
    from networks.discriminator_2d import FCDiscriminator
    ops = _ops()
    volume, label = _batch(kind)
    model, dan = _nets(kind)
    tr = AdversarialTrainer(model, dan, use_tape=False, **KW)
    with pytest.raises(ValueError, match="2-D"):
        tr.step(volume.unsqueeze(2), label)
    sd0 = {k: v.detach().clone() for k, v in dan.state_dict().items()}
    p0, state0 = model.flat_param.clone(), tr.state.clone()
    SENT = 123.0
    for _, gv in dan.named_flat(dan.flat_grad):      # not the padding words between the parameters: Adam reads those too
        gv.fill_(SENT)
    seen = []
    inner = dan.loss_forward

    def spy(logits, image, target):
        if logits.shape[0] == B:       # phase B begins: what phase A left of the discriminator
            seen.append((dan.flat_param.clone(), dan.flat_grad.clone(), tr.adam_m.clone(), tr.adam_v.clone(),
                         tr.adam_state.clone(), model.training, dan.training))
        return inner(logits, image, target)
    dan.loss_forward = spy
    tr.step(volume, label)
    torch.cuda.synchronize()
    # phase A leaves the discriminator's parameters, gradients and Adam state untouched
    fp, fg, am, av, ast, m_train, d_train = seen[0]
    ref = FCDiscriminator(C, ndf=NDF, pool=(1, 1))
    ref.load_state_dict(sd0)
    assert torch.equal(fp, ref.flat_param) and all((gv == SENT).all() for _, gv in dan.named_flat(fg))
    assert (am == 0).all() and (av == 0).all() and ast[0].item() == 0
    assert m_train and d_train
    # ---- the student's logits gradient: the tail on the trainer's own logits and the discriminator branch of the ops
    plan = tr.pass_a[0]
    a_logits = plan.out.t
    assert tuple(a_logits.shape) == (B, C, 1, 32, 32)
    ref.eval()
    ref.loss_forward(a_logits[L:], volume[L:], torch.ones(B - L, dtype=torch.int32, device="cuda"))
    ref.loss_backward(params=False, dmap=True)
    out = torch.full((16,), float("nan"), device="cuda")
    want = torch.full_like(a_logits, float("nan"))
    ops.adversarial_tail(a_logits, label[:L].contiguous(), L, ref.dmap_buffer(), ref.loss_buffer(), out, dlogits=want,
                         state=state0)
    got = model.logits_grad_buffer(tr.pass_a)
    assert torch.equal(got, want) and torch.isfinite(got).all() and got[L:].abs().max() > 0
    assert torch.equal(out[:5 + C], tr.out[:5 + C])
    # ---- the student's parameters: the existing SGD path on its gradient
    p, mom = p0.clone(), torch.zeros_like(p0)
    ops.sgd_ema_step(p, model.flat_grad, mom, None, momentum=0.9, weight_decay=1e-4, grad_scale=1.0, state=state0)
    assert torch.equal(p, model.flat_param) and torch.equal(mom, tr.momentum_buf)
    # ---- the discriminator's parameters: mis_adam_step on the ops' gradients (phase B read the updated student's logits)
    b_logits = model._last[0].out.t
    assert model._last[0] is not plan
    ref.train()
    ref.drop_masks = [s.clone() for s in dan._cur[0]["scale"]]
    assert len(ref.drop_masks) == 2 and all(((s == 0) | (s == 2)).all() for s in ref.drop_masks)
    ref.loss_forward(b_logits, volume, (torch.arange(B) < L).int().cuda())
    ref.loss_backward(params=True, dmap=False)
    assert torch.equal(ref.loss_buffer(), tr.dan_out) and torch.equal(ref.flat_grad, dan.flat_grad)
    m, v, st = torch.zeros_like(ref.flat_param), torch.zeros_like(ref.flat_param), torch.zeros(2, dtype=torch.int64, device="cuda")
    ops.adam_init(st, 0)
    ops.adam_step(ref.flat_param, ref.flat_grad, m, v, st, 1e-4, (0.9, 0.99), 1e-8)
    assert torch.equal(ref.flat_param, dan.flat_param) and torch.equal(m, tr.adam_m) and torch.equal(v, tr.adam_v)
    assert not torch.equal(dan.flat_param, fp) and tr.adam_state[0].item() == 1
    s = tr.losses()
    assert abs(s["consistency_weight"] - 0.1 * np.exp(-5.0)) < 1e-7 and s["DAN_loss"] > 0 and s["consistency_loss"] > 0


@pytest.mark.parametrize("kind", ["unet", "pnet"])
def test_taped_replay_and_a_second_seeded_run_equal_the_eager_run_bit_for_bit(kind):
    eager = _run(kind, 4, use_tape=False)
    taped = _run(kind, 4, use_tape=True)           # two eager steps, the recorded one, one replay
    assert taped["taped"] and not eager["taped"]
    assert _same(eager, taped), "the taped step differs from the eager one"
    again = _run(kind, 4, use_tape=True)
    assert _same(taped, again), "two seeded runs of four steps differ"
    assert eager["step"] == 4 and all(torch.isfinite(o[0][:5]).all() for o in eager["outs"])
    assert not torch.equal(eager["outs"][0][1], eager["outs"][3][1]), "the discriminator does not move"


def test_vit_seg_taped_step_equals_the_eager_step():
    """SwinUnet through both phases: the second, ``no_backward``, ``slot=1`` forward runs on a SwinPlan of its own, and the
    reference's AvgPool2d((7, 7)) pools the 14 x 14 that conv4 leaves of 224 x 224 exactly."""
    eager = _run("ViT_Seg", 4, use_tape=False)
    taped = _run("ViT_Seg", 4, use_tape=True)      # two eager steps, the recorded one, one replay
    assert taped["taped"] and _same(eager, taped)
    assert eager["step"] == 4 and all(torch.isfinite(o[0][:5]).all() and torch.isfinite(o[1]).all() for o in eager["outs"])


def test_an_extent_that_does_not_leave_two_by_two_windows_is_refused_by_name():
    from networks.discriminator_2d import FCDiscriminator
    dan = FCDiscriminator(C, ndf=NDF)
    lg, img = torch.zeros(1, C, 32, 32, device="cuda"), torch.zeros(1, 1, 32, 32, device="cuda")
    with pytest.raises(RuntimeError, match="2 x 2 of an input of 32 x 32"):
        dan.loss_forward(lg, img, torch.zeros(1, dtype=torch.int32, device="cuda"))


def test_checkpoint_round_trip_restores_the_discriminator_and_adam(tmp_path):
    from mis_hip.step import AdversarialTrainer
    model, dan = _nets("unet")
    tr = AdversarialTrainer(model, dan, use_tape=False, **KW)
    tr.step(*_batch("unet"))
    tr.step(*_batch("unet"))
    path = str(tmp_path / "DAN_iter_2.pth")
    torch.save(tr.dan_checkpoint(), path)
    ck = torch.load(path)
    assert sorted(ck) == ["adam_m", "adam_step", "adam_v", "state_dict"] and list(ck["state_dict"]) == list(ao.DISC_KEYS)
    assert ck["adam_step"] == 2 and tuple(ck["state_dict"]["classifier.weight"].shape) == (2, 32 * NDF)
    model2, dan2 = _nets("unet", seed=6)
    tr2 = AdversarialTrainer(model2, dan2, use_tape=False, **KW)
    assert not torch.equal(dan2.flat_param, dan.flat_param)
    tr2.load_dan_checkpoint(ck)
    torch.cuda.synchronize()
    assert torch.equal(dan2.flat_param, dan.flat_param) and torch.equal(tr2.adam_m, tr.adam_m)
    assert torch.equal(tr2.adam_v, tr.adam_v) and tr2.adam_state[0].item() == 2
