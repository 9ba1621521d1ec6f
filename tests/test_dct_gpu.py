"""Deep co-training: the HIP path through DeepCoTrainingTrainer and the mis_rot90 / mis_dct_tail / mis_grad_combine
operators, against torch on the GPU, torch autograd in float64 and the golden vectors of the real reference
(scripts/gen_golden_dct.py, code/train_deep_co_training_2D{,_ViT}.py).  Tolerances as in test_ict_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")
GOLD = os.path.join(ROOT, "tests", "golden")
TOL_LOGIT = 1e-3
TOL_LOSS = 1e-3


def _sample_idx(numel):
    return np.unique(np.linspace(0, numel - 1, 64).astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("n", [36, 100, 224, 256])
def test_rot90_is_bit_identical_to_torch(C, n):
    from mis_hip import ops
    g = torch.Generator().manual_seed(n * 10 + C)
    vol = (torch.randn((5, C, n, n), generator=g) * 100).cuda()
    unl = vol[2:]                                              # the batch-strided view volume[L:]
    base = torch.randn((3, C * n * n + 12), generator=g).cuda()
    padded = base[:, :C * n * n].view(3, C, n, n)              # batch stride C*n*n + 12
    for x in (unl, padded):
        for k in range(4):
            out = torch.full((3, C, n, n), float("nan"), device="cuda")
            ops.rot90(x, out, k=k)
            assert torch.equal(out, torch.rot90(x, k, [2, 3])), k
    # k read on the device: sched[state.iter_num]
    st = ops.new_step_state()
    sched = torch.tensor([0, 1, 2, 3, 1, 3], dtype=torch.int32, device="cuda")
    for it in range(6):
        ops.step_init(st, 1, it, 0.01, 30000, 0.0, 0.1, 200.0)
        out = torch.full((3, C, n, n), float("nan"), device="cuda")
        ops.rot90(unl, out, sched=sched, state=st)
        assert torch.equal(out, torch.rot90(unl, int(sched[it]), [2, 3])), it


def test_rot90_non_square_even_k_only():
    from mis_hip import ops
    x = torch.randn((2, 1, 36, 100), device="cuda")
    for k in (0, 2):
        out = torch.empty_like(x)
        ops.rot90(x, out, k=k)
        assert torch.equal(out, torch.rot90(x, k, [2, 3]))
    with pytest.raises(RuntimeError):
        ops.rot90(x, torch.empty((2, 1, 100, 36), device="cuda"), k=1)


def _torch_dct_loss(a, r, label, L, C, k, w):
    """The reference's loss expression (train_deep_co_training_2D.py:148-158) in float64: the shared loss-tail oracle
    (tests/loss_tail_oracle.py)."""
    from loss_tail_oracle import dct_tail
    out, da, dr = dct_tail(a, r, label, L, k, w)
    return dict(loss=out[0].item(), loss_ce=out[1].item(), loss_dice=out[2].item(), consistency_loss=out[3].item()), da, dr


@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("n", [36, 64])
@pytest.mark.parametrize("ldt", [torch.uint8, torch.int64])
def test_dct_tail_matches_torch_autograd(C, n, ldt):
    from mis_hip import ops
    g = torch.Generator().manual_seed(C * 100 + n + (ldt == torch.uint8))
    L, U, S, pad = 3, 2, n * n, 8      # every tensor is a view of rows [.., C * S + pad]: non-trivial batch strides

    def strided(rows, fill=None):
        base = torch.randn((rows, C * S + pad), generator=g) * 3.0 if fill is None else torch.full((rows, C * S + pad), fill)
        return base.cuda()

    def view5(b, rows):
        return b[:, :C * S].reshape(rows, C, 1, n, n)

    ab, rb = strided(L + U), strided(U)
    a4, r4 = view5(ab, L + U)[:, :, 0].cpu(), view5(rb, U)[:, :, 0].cpu()
    label = torch.randint(0, C, (L, n, n), generator=g).to(ldt)
    w, scale = 0.37, 2.5
    for k in range(4):
        ref, ref_da, ref_dr = _torch_dct_loss(a4, r4, label, L, C, k, w)
        outs = []
        for _ in range(2):
            out = torch.zeros(16, device="cuda")
            da, dr = strided(L + U, float("nan")), strided(U, float("nan"))
            ops.dct_tail(view5(ab, L + U), view5(rb, U), label.cuda(), L, out, dA=view5(da, L + U), dR=view5(dr, U), k=k,
                         cons_weight=w, loss_scale=scale)
            outs.append((out.clone(), da.clone(), dr.clone()))
        bits = lambda t: t.view(torch.int32)
        for i in range(3):
            assert torch.equal(bits(outs[0][i]), bits(outs[1][i])), (k, i)        # bit-reproducible
        o = outs[0][0].cpu().double()
        for i, key in enumerate(("loss", "loss_ce", "loss_dice", "consistency_loss")):
            assert abs(o[i].item() - ref[key]) <= 1e-5 * max(abs(ref[key]), 1e-3), (k, key, o[i].item(), ref[key])
        assert abs(o[4].item() - w) <= 1e-7 and int(o[5].item()) == k
        for got, want, rows in ((outs[0][1], ref_da, L + U), (outs[0][2], ref_dr, U)):
            got = got.cpu()
            assert torch.isnan(got[:, C * S:]).all()                           # the padding of every row is untouched
            got = got[:, :C * S].reshape(rows, C, n, n).double()
            assert (got - scale * want).abs().max().item() <= 1e-6 * scale, k


def test_grad_combine_copies_and_adds():
    from mis_hip import ops
    for n in (4096, 1001):                     # float4 and scalar paths
        a, b = torch.randn(n, device="cuda"), torch.randn(n, device="cuda")
        d = torch.empty_like(a)
        ops.grad_combine(d, a, accumulate=False)
        assert torch.equal(d, a)
        ops.grad_combine(d, b, accumulate=True)
        assert torch.equal(d, a + b)


# ---------------------------------------------------------------------------------------------------------------------
# the step against the reference goldens
# ---------------------------------------------------------------------------------------------------------------------
def _make(kind, C):
    from networks.net_factory import net_factory
    if kind == "swin":
        from oracle.swin import OracleSwinUnet
        return OracleSwinUnet(C), (lambda: net_factory("ViT_Seg", 1, C))
    from oracle.nets import OracleUNet2D
    return OracleUNet2D(1, C), (lambda: net_factory("unet", 1, C))


@pytest.mark.parametrize("name", ["dct_unet2d_64", "dct_swin_224"])
def test_dct_step_matches_reference_golden(name):
    from mis_hip.step import DeepCoTrainingTrainer
    from oracle import filler
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    kind, cfg = meta["kind"], meta["cfg"]
    C, L, B = cfg["num_classes"], cfg["labeled_bs"], cfg["batch_size"]
    sp = tuple(cfg["spatial"])
    onet, make = _make(kind, C)
    volume = filler.image((B, 1) + sp, "volume").cuda()
    label = filler.labels((B,) + sp, C, torch.uint8).cuda()
    for it in meta["iters"]:
        pre = f"it{it}_"
        k = int(z[pre + "rot_k"])
        model = make()
        model.train()
        model.dropout_enabled = False
        model.load_state_dict(filler.fill_state_dict(onet.new_state()))
        tr = DeepCoTrainingTrainer(model, labeled_bs=L, num_classes=C, base_lr=cfg["base_lr"],
                                   max_iterations=cfg["max_iterations"], consistency=cfg["consistency"],
                                   consistency_rampup=cfg["rampup"], iter_num=it)
        for n, v in model.named_flat(tr.momentum_buf):
            v.copy_(filler.uniform(v.shape, "mom." + n, -0.01, 0.01))
        tr.step(volume, label, rot_k=k)
        got = tr.losses()
        assert got["rot_k"] == k
        assert torch.equal(tr._rot_in, torch.rot90(volume[L:], k, [2, 3]))
        for key in ("loss", "loss_ce", "loss_dice", "consistency_loss"):
            assert abs(got[key] - float(z[pre + key])) <= TOL_LOSS, (it, key, got[key], float(z[pre + key]))
        assert abs(got["consistency_weight"] - float(z[pre + "consistency_weight"])) <= 1e-6
        shape_a = (B, 1, 1) + sp
        logits = {"logits_": model.plan_for(shape_a).out.t, "rot_logits_": model.plan_for((B - L,) + shape_a[1:], slot=1).out.t}
        for key, t in logits.items():
            flat = t.detach().double().cpu().flatten()
            ref = z[pre + key + "samples"]
            np.testing.assert_allclose(flat[_sample_idx(flat.numel())].numpy(), ref, rtol=0,
                                       atol=TOL_LOGIT * max(1.0, float(np.abs(ref).max())))
        # the optimizer's gradient: the sum over BOTH passes (one pass alone misses the consistency half of the other)
        env = 6.0 * z[pre + "grad_relerr32"] + 2e-3
        gn = np.array([float(g.double().norm()) for _, g in model.named_flat(model.flat_grad)])
        ref_gn, gn64 = z[pre + "grad_norms"], z[pre + "grad_norms64"]
        assert np.all(np.abs(gn - ref_gn) <= env * np.maximum(ref_gn, gn64) + 1e-5 * ref_gn.max()), \
            list(zip(gn, ref_gn, gn64))
        absum = np.array([float(v.double().abs().sum()) for _, v in model.named_flat(model.flat_param)])
        np.testing.assert_allclose(absum, z[pre + "param_abssum"], rtol=1e-5, atol=1e-6)
        sd = model.state_dict()
        if pre + "buf_sum" in z.files:          # BatchNorm running statistics after the double update
            bufs = [n for n in sd if n.endswith("running_mean") or n.endswith("running_var")]
            np.testing.assert_allclose(np.array([float(sd[n].double().sum()) for n in bufs]), z[pre + "buf_sum"],
                                       rtol=1e-4, atol=1e-4)
            assert all(int(sd[n]) == 2 for n in sd if n.endswith("num_batches_tracked"))


# ---------------------------------------------------------------------------------------------------------------------
# the trainer: tape, determinism, device k
# ---------------------------------------------------------------------------------------------------------------------
IT0 = 1200


def _run_dct(steps, use_tape, seed=7):
    from networks.net_factory import net_factory
    from mis_hip.step import DeepCoTrainingTrainer
    from oracle import filler
    from oracle.nets import OracleUNet2D
    m = net_factory("unet", 1, 4)
    m.load_state_dict(filler.fill_state_dict(OracleUNet2D(1, 4).new_state()))
    m.train()
    vol = filler.image((8, 1, 32, 32), "volume").cuda()
    lab = filler.labels((8, 32, 32), 4, torch.uint8).cuda()
    tr = DeepCoTrainingTrainer(m, labeled_bs=4, num_classes=4, seed=seed, iter_num=IT0, use_tape=use_tape)
    outs = []
    for i in range(steps):
        tr.step(vol if i % 2 == 0 else vol.flip(0).contiguous(), lab)
        outs.append(tr.out.clone())
    torch.cuda.synchronize()
    return dict(out=torch.stack(outs), param=m.flat_param.clone(), bufs=[b.clone() for b in m.buffers()],
                tape=tr._tape is not None, sched=tr.schedule.cpu())


def test_dct_tape_and_eager_are_bit_identical_and_k_follows_the_schedule():
    from mis_hip.step import rotation_schedule
    taped = _run_dct(5, True)
    eager = _run_dct(5, False)
    again = _run_dct(5, True)
    assert taped["tape"] and not eager["tape"]
    for r in (eager, again):
        assert torch.equal(taped["out"], r["out"]) and torch.equal(taped["param"], r["param"])
        assert all(torch.equal(a, b) for a, b in zip(taped["bufs"], r["bufs"]))
    ks = taped["out"][:, 5].long().tolist()
    want = rotation_schedule(7, 30000)[IT0:IT0 + 5]
    assert ks == want and len(set(want)) > 1            # steps 4 and 5 are replays: k is read on the device
    assert taped["sched"].tolist() == rotation_schedule(7, 30000)
    assert torch.isfinite(taped["out"][:, :5]).all() and (taped["out"][:, 3] > 0).all()
    other = _run_dct(2, True, seed=8)
    assert other["out"][:, 5].long().tolist() == rotation_schedule(8, 30000)[IT0:IT0 + 2]


def test_dct_trainer_rejects_bad_batch_before_launch():
    from networks.net_factory import net_factory
    from mis_hip.step import DeepCoTrainingTrainer
    m = net_factory("unet", 1, 4)
    tr = DeepCoTrainingTrainer(m, labeled_bs=2, num_classes=4)
    before = m.flat_param.clone()
    with pytest.raises(ValueError):
        tr.step(torch.zeros((2, 1, 32, 32), device="cuda"), torch.zeros((2, 32, 32), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        tr.step(torch.zeros((4, 1, 32, 64), device="cuda"), torch.zeros((4, 32, 64), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        tr.step(torch.zeros((4, 1, 32, 32), device="cuda"), torch.zeros((4, 32, 32), dtype=torch.uint8, device="cuda"),
                rot_k=4)
    torch.cuda.synchronize()
    assert torch.equal(before, m.flat_param) and tr.iter_num == 0


# ---------------------------------------------------------------------------------------------------------------------
# data parallel: two gloo ranks on the same batch == one process
# ---------------------------------------------------------------------------------------------------------------------
def _dct_worker(rank, world, store, out_dir):
    for p in (PKG, ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    if world > 1:
        # a file rendezvous: no TCP port is reserved and handed over, so nothing else on the host can take it meanwhile
        dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=world)
    from networks.net_factory import net_factory
    from mis_hip.step import DeepCoTrainingTrainer
    torch.manual_seed(5)
    m = net_factory("unet", 1, 4)
    m.train()
    g = torch.Generator(device="cuda").manual_seed(100)          # the same batch on every rank
    vol = torch.rand((4, 1, 64, 64), generator=g, device="cuda")
    lab = torch.randint(0, 4, (4, 64, 64), generator=g, device="cuda").to(torch.uint8)
    tr = DeepCoTrainingTrainer(m, labeled_bs=2, num_classes=4, iter_num=1000, seed=7)
    for _ in range(4):                                           # the fourth step is a replay of the tape
        tr.step(vol, lab)
    torch.cuda.synchronize()
    torch.save(dict(param=m.flat_param.cpu(), tape=tr._tape is not None), os.path.join(out_dir, f"dct_{world}_{rank}.pt"))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_dct_two_gloo_ranks_match_one_process(tmp_path):
    mp.spawn(_dct_worker, args=(1, None, str(tmp_path)), nprocs=1, join=True)
    mp.spawn(_dct_worker, args=(2, str(tmp_path / "gloo_store"), str(tmp_path)), nprocs=2, join=True)
    r = {k: torch.load(os.path.join(tmp_path, f"dct_{k}.pt")) for k in ("1_0", "2_0", "2_1")}
    assert all(v["tape"] for v in r.values())
    # the summed buffer is exchanged once: (g + g) / 2 == g bit for bit
    assert torch.equal(r["2_0"]["param"], r["2_1"]["param"]) and torch.equal(r["2_0"]["param"], r["1_0"]["param"])


# ---------------------------------------------------------------------------------------------------------------------
# command lines
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("script,extra", [
    ("train_deep_co_training_2D.py", ["--patch_size", "64", "64"]),
    ("train_deep_co_training_2D_ViT.py", ["--patch_size", "224", "224"]),
])
def test_dct_cli_runs(script, extra, tmp_path):
    work = tmp_path / "code"
    work.mkdir()
    cmd = [sys.executable, os.path.join(PKG, script), "--root_path", str(tmp_path / "no_data"), "--exp", "dct_cli",
           "--max_iterations", "3", "--batch_size", "4", "--labeled_bs", "2"] + extra
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run(cmd, cwd=work, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Training Finished!" in r.stdout
    assert "iteration 3 : loss :" in r.stdout + r.stderr
