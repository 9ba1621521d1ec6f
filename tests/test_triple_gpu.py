"""TripleViewTrainer on HIP: a step at cross_224's geometry (UNet, UNet, SwinUnet) against the golden vector of the real
reference and the CPU oracle; taped == eager; MIS_TWO_STREAM=0 (a child process) == the default; two ranks on one GPU; the
refusals."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _sample_idx(numel):
    return np.unique(np.linspace(0, numel - 1, 64).astype(np.int64))


def lr_next(k, cfg):
    """learning rate in effect for step k under the post-increment rule"""
    return cfg["base_lr"] * (1.0 - k / cfg["max_iterations"]) ** 0.9


def test_triple_view_step_matches_reference_and_oracle():
    from config import lite_config
    from mis_hip import ops
    from mis_hip.step import TripleViewTrainer
    from networks.net_factory import net_factory
    from networks.vision_transformer import SwinUnet
    from oracle import filler
    from oracle.nets import OracleUNet2D
    from oracle.swin import OracleSwinUnet
    from triple_oracle import triple_view_step

    z = np.load(os.path.join(GOLD, "triple_224.npz"))
    meta = json.loads(str(z["meta"]))
    cfg, it, kinds = meta["cfg"], meta["iters"][0], meta["kinds"]
    C, L = cfg["num_classes"], cfg["labeled_bs"]
    nets = [OracleUNet2D(1, C) if k == "unet2d" else OracleSwinUnet(C) for k in kinds]
    sds = []
    for m, onet in enumerate(nets):
        sd = filler.fill_state_dict({f"m{m}." + k: v.clone() for k, v in onet.new_state().items()})
        sds.append({k.split(".", 1)[1]: v for k, v in sd.items()})
    B, sp = cfg["batch_size"], tuple(cfg["spatial"])
    volume = filler.image((B, 1) + sp, "volume")
    label = filler.labels((B,) + sp, C, torch.uint8)
    models = [net_factory("unet", 1, C) if k == "unet2d" else SwinUnet(lite_config(), img_size=224, num_classes=C)
              for k in kinds]
    for m in range(3):
        models[m].load_state_dict(sds[m])
        models[m].train()
        models[m].dropout_enabled = False
    tr = TripleViewTrainer(*models, labeled_bs=L, num_classes=C, base_lr=cfg["base_lr"],
                           max_iterations=cfg["max_iterations"], consistency=cfg["consistency"],
                           consistency_rampup=cfg["rampup"], iter_num=it)
    moms = []
    for m, buf in enumerate((tr.mom1, tr.mom2, tr.mom3)):
        mm = {}
        for n, v in models[m].named_flat(buf):
            t = filler.uniform(v.shape, f"mom{m}." + n, -0.01, 0.01)
            v.copy_(t)
            mm[n] = t.clone()
        moms.append(mm)
    outs = tr.step(volume.cuda(), label.cuda())
    assert len(outs) == 3 and outs[2] is tr.out3
    got = tr.losses()
    pre = f"it{it}_"
    # ---- golden (real reference) ----
    for i in (1, 2, 3):
        assert abs(got[f"model{i}_loss"] - float(z[pre + f"model{i}_loss"])) <= 2e-4
        assert abs(0.5 * (got[f"loss{i}_ce"] + got[f"loss{i}_dice"]) - float(z[pre + f"loss{i}_ce_dice"])) <= 2e-4
        assert abs(got[f"pseudo_supervision{i}a"] - float(z[pre + f"pseudo{i}a"])) <= 2e-4
        assert abs(got[f"pseudo_supervision{i}b"] - float(z[pre + f"pseudo{i}b"])) <= 2e-4
    assert abs(got["loss"] - sum(float(z[pre + f"model{i}_loss"]) for i in (1, 2, 3))) <= 6e-4
    assert got["consistency_weight"] > 0
    assert abs(got["consistency_weight"] - float(z[pre + "consistency_weight"])) <= 1e-6
    st = ops.read_step_state(tr.state)
    assert st["iter_num"] == it + 1 and tr.iter_num == it + 1
    for m in range(3):
        lg = models[m]._last[0].out.t.detach().double().cpu().flatten()
        np.testing.assert_allclose(lg[_sample_idx(lg.numel())].numpy(), z[pre + f"logits{m + 1}_samples"], rtol=0,
                                   atol=1e-3)
        gn = np.array([float(g.double().norm()) for _, g in models[m].named_flat(models[m].flat_grad)])
        ref_gn, gn64 = z[pre + f"grad_norms{m + 1}"], z[pre + f"grad_norms64_{m + 1}"]
        env = 6.0 * z[pre + f"grad_relerr32_{m + 1}"] + 2e-3
        assert np.all(np.abs(gn - ref_gn) <= env * np.maximum(ref_gn, gn64) + 1e-5 * ref_gn.max())
    # ---- oracle, full tensors ----
    osd = [{k: v.clone() for k, v in sd.items()} for sd in sds]
    r = triple_view_step(nets, osd, moms, volume, label, it, labeled_bs=L, num_classes=C, base_lr=cfg["base_lr"],
                         max_iterations=cfg["max_iterations"], consistency=cfg["consistency"], rampup=cfg["rampup"])
    lr = r["lr"]
    assert abs(lr - float(z[pre + "lr"])) <= 1e-9
    assert abs(st["lr"] - lr_next(it + 1, cfg)) <= 1e-9 + 1e-6 * lr        # post-increment: the next step's rate
    for m in range(3):
        lg = models[m]._last[0].out.t.cpu().reshape(r[f"logits{m + 1}"].shape)
        assert (lg - r[f"logits{m + 1}"]).abs().max().item() <= 1e-3
        env = 6.0 * z[pre + f"grad_relerr32_{m + 1}"] + 2e-3
        gmax = z[pre + f"grad_max64_{m + 1}"]
        gscale = max(float(g.abs().max()) for g in r["grads"][m].values())
        for i, (n, g) in enumerate(models[m].named_flat(models[m].flat_grad)):
            ref = r["grads"][m][n]
            tol = env[i] * max(float(ref.abs().max()), gmax[i]) + 5e-4 * gscale
            assert (g.cpu() - ref).abs().max().item() <= tol, (m, n)
        for i, (n, v) in enumerate(models[m].named_flat(models[m].flat_param)):
            tol = env[i] * gmax[i] + 1e-5 * gscale
            assert (v.cpu() - osd[m][n]).abs().max().item() <= 1e-6 + lr * tol, (m, n)


# ---------------------------------------------------------------------------------------------------------------------
# three unet students at 64 x 64, B = 4, L = 2, dropout off: tape, stream switch
# ---------------------------------------------------------------------------------------------------------------------
def _three_unets(tape, steps=5):
    """Five steps of three UNets from three different filler states; returns [outs of every step, params, momenta] and the
    trainer."""
    from mis_hip.step import TripleViewTrainer
    from networks.net_factory import net_factory
    from oracle import filler
    from oracle.nets import OracleUNet2D
    C = 4
    models = []
    for m in range(3):
        sd = filler.fill_state_dict({f"m{m}." + k: v.clone() for k, v in OracleUNet2D(1, C).new_state().items()})
        net = net_factory("unet", 1, C)
        net.load_state_dict({k.split(".", 1)[1]: v for k, v in sd.items()})
        net.train()
        net.dropout_enabled = False
        models.append(net)
    tr = TripleViewTrainer(*models, labeled_bs=2, num_classes=C, seed=11, iter_num=1500, use_tape=tape)
    g = torch.Generator().manual_seed(3)
    outs = []
    for _ in range(steps):                                  # fresh input tensors every step
        v = torch.rand((4, 1, 64, 64), generator=g).cuda()
        l = torch.randint(0, C, (4, 64, 64), generator=g).to(torch.uint8).cuda()
        outs.append(torch.cat(tr.step(v, l)).clone())
    torch.cuda.synchronize()
    res = [torch.stack(outs)] + [m.flat_param.clone() for m in models] + [b.clone() for b in (tr.mom1, tr.mom2, tr.mom3)]
    return res, tr


def test_taped_triple_view_step_is_bit_identical_to_eager():
    eager, tr_e = _three_unets(False)
    taped, tr_t = _three_unets(True)
    assert tr_e._tape is None
    assert tr_t._tape is not None and len(tr_t._tape) > 50             # steps 4 and 5 were replays
    assert torch.isfinite(eager[0]).all() and (eager[0][:, 4] > 0).all()          # w > 0: the pseudo terms are live
    assert len(set(eager[0][:, 0].tolist())) == 5                      # the loss moves from step to step
    for a, b in zip(eager, taped):
        assert torch.equal(a, b)


def _child(path):
    from mis_hip import step
    assert not step.TWO_STREAM
    res, tr = _three_unets(False)
    torch.save([t.cpu() for t in res], path)


def test_one_stream_in_a_child_process_is_bit_identical_to_two_streams(tmp_path):
    from mis_hip import step
    assert step.TWO_STREAM
    here, _ = _three_unets(False)
    path = str(tmp_path / "one_stream.pt")
    env = dict(os.environ, MIS_TWO_STREAM="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--one-stream-child", path], env=env, check=True, timeout=300)
    there = torch.load(path)
    assert len(here) == len(there) == 7
    for a, b in zip(here, there):
        assert torch.equal(a.cpu(), b)


# ---------------------------------------------------------------------------------------------------------------------
# two ranks on one GPU (gloo)
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    for p in (os.path.join(ROOT, "cv-ssl-mis_amd"), ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    from mis_hip.step import TripleViewTrainer
    from networks.net_factory import net_factory
    torch.manual_seed(5)                                   # identical initial weights on both ranks
    C = 4
    models = [net_factory("unet", 1, C) for _ in range(3)]
    for m in models:
        m.train()
        m.dropout_enabled = False
    tr = TripleViewTrainer(*models, labeled_bs=1, num_classes=C, iter_num=1000, seed=7)
    assert tr.world == world
    g = torch.Generator(device="cuda").manual_seed(100 + rank)          # a different shard per rank
    vol = torch.rand((2, 1, 64, 64), generator=g, device="cuda")
    lab = torch.randint(0, C, (2, 64, 64), generator=g, device="cuda").to(torch.uint8)
    for _ in range(3):
        tr.step(vol, lab)
    torch.cuda.synchronize()
    torch.save(dict(params=[m.flat_param.cpu() for m in models], losses=tr.losses()),
               os.path.join(out_dir, f"triple_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_on_one_gpu_exchange_three_gradients(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(os.path.join(tmp_path, f"triple_{k}.pt")) for k in range(world)]
    for m in range(3):
        assert torch.equal(r[0]["params"][m], r[1]["params"][m]), f"ranks diverged in student {m + 1}"
        assert r[0]["losses"][f"model{m + 1}_loss"] != r[1]["losses"][f"model{m + 1}_loss"]      # the shards really differ
    assert not torch.equal(r[0]["params"][0], r[0]["params"][1])        # the students do not collapse into one


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_triple_view_trainer_refusals():
    from mis_hip.step import TripleViewTrainer
    from networks.net_factory import net_factory
    models = [net_factory("unet", 1, 4) for _ in range(3)]
    for m in models:
        m.train()
    tr = TripleViewTrainer(*models, labeled_bs=2, num_classes=4, use_tape=False)
    vol = torch.rand((4, 1, 64, 64), device="cuda")
    lab = torch.zeros((4, 64, 64), dtype=torch.uint8, device="cuda")
    before = [m.flat_param.clone() for m in models]
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        tr.step(vol[:, 0], lab)                            # wrong rank: [B, H, W]
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        tr.step(vol.unsqueeze(2), lab)                     # wrong rank: [B, C, 1, H, W]
    with pytest.raises(ValueError, match="labeled_bs < batch_size"):
        tr.step(vol[:2], lab[:2])                          # no unlabeled sample
    models[1].eval()
    with pytest.raises(RuntimeError, match="train mode"):
        tr.step(vol, lab)
    assert tr.TRAIN_MODE and "train mode" in tr.TRAIN_MODE
    models[1].train()
    torch.cuda.synchronize()
    assert tr.iter_num == 0 and all(torch.equal(a, m.flat_param) for a, m in zip(before, models))
    assert (tr.out1 == 0).all() and (tr.out2 == 0).all() and (tr.out3 == 0).all()        # nothing was launched
    tr.step(vol, lab)                                      # and the trainer still works
    assert tr.iter_num == 1 and tr.losses()["loss"] > 0


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--one-stream-child":
    for p in (os.path.join(ROOT, "cv-ssl-mis_amd"), ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    _child(sys.argv[2])
