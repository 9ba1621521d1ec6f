"""Interpolation Consistency Training: the HIP path through ICTTrainer and the three mis_ict_* / mis_beta_sample
operators, against the golden vectors of the real reference (scripts/gen_golden_ict.py,
code/train_interpolation_consistency_training_{2D,3D,2D_ViT}.py), the CPU restatement (tests/ict_oracle.py) and
torch on the GPU.  Tolerances as in test_uamt_gpu.py: 1e-3 on logits / losses, the measured fp32 envelope on
gradients."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")
GOLD = os.path.join(ROOT, "tests", "golden")
TOL_LOGIT = 1e-3
TOL_LOSS = 1e-3


def _sample_idx(numel):
    return np.unique(np.linspace(0, numel - 1, 64).astype(np.int64))


def _nets(kind, C):
    from oracle.nets import OracleUNet2D, OracleUNet3D
    if kind == "swin":
        from networks.net_factory import net_factory
        from oracle.swin import OracleSwinUnet
        return OracleSwinUnet(C), (lambda: net_factory("ViT_Seg", 1, C)), torch.uint8
    if kind == "unet2d":
        from networks.net_factory import net_factory
        return OracleUNet2D(1, C), (lambda: net_factory("unet", 1, C)), torch.uint8
    from networks.net_factory_3d import net_factory_3d
    return OracleUNet3D(C, 1), (lambda: net_factory_3d("unet_3D", 1, C)), torch.int64


@pytest.mark.parametrize("name", ["ict_unet2d_64", "ict_unet3d_64", "ict_swin_224"])
def test_ict_step_matches_reference_golden_and_oracle(name):
    from ict_oracle import ict_step
    from mis_hip.step import ICTTrainer
    from oracle import filler

    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    kind, cfg, it = meta["kind"], meta["cfg"], meta["iters"][0]
    C, L, B = cfg["num_classes"], cfg["labeled_bs"], cfg["batch_size"]
    M, sp = L // 2, tuple(cfg["spatial"])
    onet, make, ldt = _nets(kind, C)
    sd0 = filler.fill_state_dict(onet.new_state())
    tsd0 = filler.fill_state_dict({"t." + k: v.clone() for k, v in onet.new_state().items()})
    tsd0 = {k[2:]: v for k, v in tsd0.items()}
    volume = filler.image((B, 1) + sp, "volume")
    label = filler.labels((B,) + sp, C, ldt)
    pre = f"it{it}_"
    lam = torch.from_numpy(z[pre + "mix_factors"])

    model, ema = make(), make()
    for p in ema.parameters():
        p.detach_()
    model.train(); ema.train()
    model.dropout_enabled = ema.dropout_enabled = False
    model.load_state_dict(sd0)
    ema.load_state_dict(tsd0)
    tr = ICTTrainer(model, ema, labeled_bs=L, num_classes=C, base_lr=cfg["base_lr"],
                    max_iterations=cfg["max_iterations"], ema_decay=cfg["ema_decay"], consistency=cfg["consistency"],
                    consistency_rampup=cfg["rampup"], iter_num=it)
    mom = {}
    for n, v in model.named_flat(tr.momentum_buf):
        m = filler.uniform(v.shape, "mom." + n, -0.01, 0.01)
        v.copy_(m)
        mom[n] = m.clone()
    tr.step(volume.cuda(), label.cuda(), mix_factors=lam.cuda())
    got = tr.losses()
    assert torch.equal(tr.mix_factors.cpu(), lam)

    # ---- (a) golden vectors from the real reference ----
    for k in ("loss", "loss_ce", "loss_dice", "consistency_loss"):
        assert abs(got[k] - float(z[pre + k])) <= TOL_LOSS, (k, got[k], float(z[pre + k]))
    assert abs(got["consistency_weight"] - float(z[pre + "consistency_weight"])) <= 1e-6
    assert got["consistency_weight"] > 0
    shape5 = lambda n: (n, 1, 1) + sp if len(sp) == 2 else (n, 1) + sp
    s_logits = model._last[0].out.t
    t0, t1 = ema.plan_for(shape5(M)).out.t, ema.plan_for(shape5(M), slot=1).out.t
    for t, key in ((s_logits, "logits_"), (t0, "teacher_logits0_"), (t1, "teacher_logits1_")):
        flat = t.detach().double().cpu().flatten()
        np.testing.assert_allclose(flat[_sample_idx(flat.numel())].numpy(), z[pre + key + "samples"], rtol=0,
                                   atol=TOL_LOGIT * max(1.0, float(np.abs(z[pre + key + "samples"]).max())))
    env = 6.0 * z[pre + "grad_relerr32"] + 2e-3
    gn = np.array([float(g.double().norm()) for _, g in model.named_flat(model.flat_grad)])
    ref_gn, gn64 = z[pre + "grad_norms"], z[pre + "grad_norms64"]
    assert np.all(np.abs(gn - ref_gn) <= env * np.maximum(ref_gn, gn64) + 1e-5 * ref_gn.max()), \
        list(zip(gn, ref_gn, gn64))
    msd, esd = model.state_dict(), ema.state_dict()
    if pre + "teacher_buf_sum" in z.files:      # BatchNorm running statistics after 1 (student) / 2 (teacher) forwards
        bufs = [n for n in msd if n.endswith("running_mean") or n.endswith("running_var")]
        np.testing.assert_allclose(np.array([float(msd[n].double().sum()) for n in bufs]), z[pre + "student_buf_sum"],
                                   rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(np.array([float(esd[n].double().sum()) for n in bufs]), z[pre + "teacher_buf_sum"],
                                   rtol=1e-4, atol=1e-3)
    nbt = [n for n in esd if n.endswith("num_batches_tracked")]
    assert all(int(esd[n]) == 2 for n in nbt) and all(int(msd[n]) == 1 for n in nbt)

    # ---- (b) the CPU restatement run here ----
    student = {k: v.clone() for k, v in sd0.items()}
    teacher = {k: v.clone() for k, v in tsd0.items()}
    orc = ict_step(onet, student, teacher, mom, volume, label, lam, it, labeled_bs=L, num_classes=C,
                   base_lr=cfg["base_lr"], max_iterations=cfg["max_iterations"], ema_decay=cfg["ema_decay"],
                   consistency=cfg["consistency"], rampup=cfg["rampup"], drop_student="off", drop_teacher="off")
    for k in ("loss", "loss_ce", "loss_dice", "consistency_loss"):
        assert abs(got[k] - orc[k]) <= TOL_LOSS, (k, got[k], orc[k])
    assert torch.equal(tr._mix_in.cpu().reshape(orc["mixed"].shape), orc["mixed"])
    assert (s_logits.cpu().reshape(orc["logits"].shape) - orc["logits"]).abs().max().item() <= TOL_LOGIT
    for t, key in ((t0, "teacher_logits0"), (t1, "teacher_logits1")):
        scale = max(1.0, float(orc[key].abs().max()))
        assert (t.cpu().reshape(orc[key].shape) - orc[key]).abs().max().item() <= TOL_LOGIT * scale, key
    gscale = max(float(g.abs().max()) for g in orc["grads"].values())
    gmax = z[pre + "grad_max64"]
    for i, (n, g) in enumerate(model.named_flat(model.flat_grad)):
        tol_g = env[i] * max(float(orc["grads"][n].abs().max()), gmax[i]) + 5e-4 * gscale
        err = (g.cpu() - orc["grads"][n]).abs().max().item()
        assert err <= tol_g, (n, err, tol_g)
    lr = float(z[pre + "lr"])
    for i, (n, v) in enumerate(model.named_flat(model.flat_param)):
        tol_g = env[i] * gmax[i] + 1e-5 * gscale
        assert (v.cpu() - student[n]).abs().max().item() <= 1e-6 + lr * tol_g, n


# ---------------------------------------------------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------------------------------------------------
def _torch_ict_loss(s, t0, t1, lam, label, L, C, w):
    """The reference's loss expression (train_interpolation_consistency_training_2D.py:168-184) in float64: the shared
    loss-tail oracle (tests/loss_tail_oracle.py)."""
    from loss_tail_oracle import ict_tail
    out, grad = ict_tail(s, t0, t1, lam, label, L, w)
    return dict(loss=out[0].item(), loss_ce=out[1].item(), loss_dice=out[2].item(), consistency_loss=out[3].item()), grad


@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("spatial", [(32, 48), (8, 12, 16)])
@pytest.mark.parametrize("ldt", [torch.uint8, torch.int64])
def test_ict_tail_matches_torch_autograd(C, spatial, ldt):
    from mis_hip import ops
    g = torch.Generator().manual_seed(C * 100 + len(spatial) * 10 + (ldt == torch.uint8))
    L, M = 3, 2
    S = int(np.prod(spatial))
    pad = 8            # non-trivial batch strides: every tensor is a view of rows [.., C * S + pad]

    def strided(n):
        base = torch.randn((n, C * S + pad), generator=g) * 3.0
        return base.cuda(), base[:, :C * S].reshape((n, C) + spatial)

    sb, s = strided(L + M)
    t0b, t0 = strided(M)
    t1b, t1 = strided(M)
    lam = torch.tensor([0.3, 0.85], dtype=torch.float32)
    label = torch.randint(0, C, (L,) + spatial, generator=g).to(ldt)
    w, scale = 0.37, 2.5
    ref, ref_grad = _torch_ict_loss(s, t0, t1, lam, label, L, C, w)

    def view5(b, n):
        v = b[:, :C * S].reshape((n, C) + spatial)
        return v.unsqueeze(2) if len(spatial) == 2 else v

    dl_base = torch.full((L + M, C * S + pad), float("nan"), device="cuda")
    outs = []
    for _ in range(2):
        out = torch.zeros(16, device="cuda")
        ops.ict_tail(view5(sb, L + M), view5(t0b, M), view5(t1b, M), lam.cuda(), label.cuda(), L, out,
                     dlogits=view5(dl_base, L + M), cons_weight=w, loss_scale=scale)
        outs.append((out.clone(), dl_base.clone()))
    bits = lambda t: t.view(torch.int32)                  # the NaN padding compares equal bit for bit
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1]))
    o = outs[0][0].cpu().double()
    for i, k in enumerate(("loss", "loss_ce", "loss_dice", "consistency_loss")):
        assert abs(o[i].item() - ref[k]) <= 1e-5 * max(abs(ref[k]), 1e-3), (k, o[i].item(), ref[k])
    assert abs(o[4].item() - w) <= 1e-7
    dl = outs[0][1].cpu()
    assert torch.isnan(dl[:, C * S:]).all()                          # the padding of every row is untouched
    got = dl[:, :C * S].reshape((L + M, C) + spatial).double()
    assert (got - scale * ref_grad).abs().max().item() <= 1e-6 * scale


def test_ict_mix_is_bit_identical_to_torch():
    from mis_hip import ops
    g = torch.Generator().manual_seed(5)
    for shape, L in (((8, 1, 64, 64), 4), ((4, 1, 20, 24, 28), 2), ((4, 3, 7, 9), 2)):   # float4 and scalar paths
        M = L // 2
        x = (torch.randn(shape, generator=g) * 100).cuda()
        lam = torch.rand(M, generator=g).cuda()
        out = torch.full((L + M,) + shape[1:], float("nan"), device="cuda")
        ops.ict_mix(x, lam, L, out)
        f = lam.reshape((M,) + (1,) * (len(shape) - 1))
        ref = torch.cat([x[:L], x[L:L + M] * (1.0 - f) + x[L + M:] * f], dim=0)
        assert torch.equal(out[:L], x[:L])
        assert torch.equal(out, ref), (shape, (out - ref).abs().max().item())


def _ks_float32(lam, alpha):
    """Exact sup-distance between the empirical law of float32 draws and the law of round-to-float32(Beta(alpha, alpha)).

    scipy's kstest assumes continuous data.  The factors are float32, in the reference too (``torch.tensor(
    np.random.beta(...), dtype=torch.float)``), and at alpha = 0.2 about 1.6 % of the mass lies within 3e-8 of 1 and
    rounds to exactly 1.0: those ties alone give kstest a statistic of ~0.016, for numpy's own generator as well.  Here
    every distinct value v carries the probability of its rounding cell, F(mid(v, next(v))) - F(mid(prev(v), v))."""
    from scipy import stats
    v, cnt = np.unique(lam.numpy(), return_counts=True)
    Fn = np.cumsum(cnt) / lam.numel()
    up = np.nextafter(v, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(v, np.float32(-np.inf)).astype(np.float64)
    hi = np.where(v >= 1, 1.0, (v.astype(np.float64) + up) / 2)
    lo = np.where(v <= 0, 0.0, (v.astype(np.float64) + dn) / 2)
    F = stats.beta(alpha, alpha).cdf
    return max(np.abs(Fn - F(hi)).max(), np.abs(Fn - cnt / lam.numel() - F(lo)).max())


@pytest.mark.parametrize("alpha", [0.2, 1.0, 2.0])
def test_beta_sampler_distribution_and_reproducibility(alpha):
    from scipy import stats
    from mis_hip import ops
    n = 65536

    def draw(seed, it):
        st = ops.new_step_state()
        ops.step_init(st, seed, it, 0.01, 30000, 0.99, 0.1, 200.0)
        lam = torch.empty(n, device="cuda")
        ops.beta_sample(lam, alpha, st)
        return lam.cpu()

    a = draw(1337, 10)
    assert torch.isfinite(a).all() and (a >= 0).all() and (a <= 1).all()
    assert _ks_float32(a, alpha) <= 0.011
    if alpha >= 1.0:         # no mass piles up at 1.0: the continuous test applies as it is
        assert stats.kstest(a.double().numpy(), stats.beta(alpha, alpha).cdf).statistic <= 0.011
    assert torch.equal(a, draw(1337, 10))
    assert not torch.equal(a, draw(1337, 11))
    assert not torch.equal(a, draw(1338, 10))


# ---------------------------------------------------------------------------------------------------------------------
# the trainer: tape, determinism, device factors
# ---------------------------------------------------------------------------------------------------------------------
def _run_ict(steps, use_tape, seed=7):
    from networks.net_factory import net_factory
    from mis_hip.step import ICTTrainer
    from oracle import filler
    from oracle.nets import OracleUNet2D
    sd0 = filler.fill_state_dict(OracleUNet2D(1, 4).new_state())
    vol = filler.image((8, 1, 32, 32), "volume").cuda()
    lab = filler.labels((8, 32, 32), 4, torch.uint8).cuda()
    m, e = net_factory("unet", 1, 4), net_factory("unet", 1, 4)
    m.load_state_dict(sd0); e.load_state_dict(sd0)
    tr = ICTTrainer(m, e, labeled_bs=4, num_classes=4, seed=seed, iter_num=1200, use_tape=use_tape)
    losses, factors = [], []
    for i in range(steps):
        tr.step(vol if i % 2 == 0 else vol.flip(0).contiguous(), lab)
        losses.append(tr.out.clone())
        factors.append(tr.mix_factors.clone())
    torch.cuda.synchronize()
    return dict(losses=torch.stack(losses), factors=torch.stack(factors), param=m.flat_param.clone(),
                ema=e.flat_param.clone(), bufs=[b.clone() for b in list(m.buffers()) + list(e.buffers())],
                tape=tr._tape is not None)


def test_ict_tape_and_eager_steps_are_bit_identical_and_seeded():
    taped = _run_ict(4, True)
    eager = _run_ict(4, False)
    again = _run_ict(4, True)
    assert taped["tape"] and not eager["tape"]
    for r in (eager, again):
        for k in ("losses", "factors", "param", "ema"):
            assert torch.equal(taped[k], r[k]), k
        assert all(torch.equal(a, b) for a, b in zip(taped["bufs"], r["bufs"]))
    f = taped["factors"]
    assert torch.isfinite(taped["losses"][:, :5]).all()
    assert ((f >= 0) & (f <= 1)).all() and not torch.equal(f[0], f[1])     # new factors every step, from the device
    other = _run_ict(2, True, seed=8)
    assert not torch.equal(other["factors"][0], f[0])


def test_ict_trainer_rejects_bad_batch_before_launch():
    from networks.net_factory import net_factory
    from mis_hip.step import ICTTrainer
    m, e = net_factory("unet", 1, 4), net_factory("unet", 1, 4)
    tr = ICTTrainer(m, e, labeled_bs=2, num_classes=4)
    before = m.flat_param.clone()
    with pytest.raises(ValueError):
        tr.step(torch.zeros((5, 1, 32, 32), device="cuda"), torch.zeros((5, 32, 32), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        tr.step(torch.zeros((4, 1, 32, 32), device="cuda"), torch.zeros((4, 32, 32), dtype=torch.uint8, device="cuda"),
                mix_factors=torch.zeros(2, device="cuda"))
    assert torch.equal(before, m.flat_param) and tr.iter_num == 0


# ---------------------------------------------------------------------------------------------------------------------
# command lines
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("script,extra", [
    ("train_interpolation_consistency_training_2D.py", ["--patch_size", "64", "64"]),
    ("train_interpolation_consistency_training_3D.py", ["--patch_size", "32", "32", "32"]),
    ("train_interpolation_consistency_training_2D_ViT.py", ["--patch_size", "224", "224"]),
])
def test_ict_cli_runs(script, extra, tmp_path):
    work = tmp_path / "code"
    work.mkdir()
    cmd = [sys.executable, os.path.join(PKG, script), "--root_path", str(tmp_path / "no_data"), "--exp", "ict_cli",
           "--max_iterations", "3", "--batch_size", "4", "--labeled_bs", "2"] + extra
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run(cmd, cwd=work, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Training Finished!" in r.stdout
    assert "iteration 3 : loss :" in r.stdout + r.stderr
