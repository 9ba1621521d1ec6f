"""Deep co-training, CPU side: the restatement tests/dct_oracle.dct_step against the golden vectors of the real reference
(scripts/gen_golden_dct.py), the rotation schedule, the batch / patch rules and the command-line surface of the two
drop-ins.  No GPU is touched."""
import json
import os
import random

import numpy as np
import pytest
import torch

from dct_oracle import REF_FLAGS_VIT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# flag names of code/train_deep_co_training_2D.py and _2D_ViT.py
REF_FLAGS_2D = ["--root_path", "--exp", "--model", "--max_iterations", "--batch_size", "--deterministic", "--base_lr",
                "--patch_size", "--seed", "--num_classes", "--labeled_bs", "--labeled_num", "--ema_decay",
                "--consistency_type", "--consistency", "--consistency_rampup"]
REF_DEFAULTS = {
    "2D": dict(exp="ACDC/Deep_Co_Training", batch_size=24, labeled_bs=12, labeled_num=3, patch_size=[256, 256],
               model="unet", root_path="../data/ACDC", num_classes=4),
    "2D_ViT": dict(exp="ACDC/Deep_Co_Training_ViT", batch_size=24, labeled_bs=7, labeled_num=7, patch_size=[224, 224],
                   model="unet", root_path="../data/ACDC", num_classes=4,
                   cfg="../code/configs/swin_tiny_patch4_window7_224_lite.yaml"),
}
CASES = ["dct_unet2d_64", "dct_swin_224"]


def _script(which):
    import importlib
    return importlib.import_module("train_deep_co_training_" + which)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-6))


@pytest.mark.parametrize("name", CASES)
def test_dct_oracle_reproduces_reference_golden(name):
    from dct_oracle import dct_step
    from oracle import filler
    from oracle.nets import OracleUNet2D
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    assert float(z["oracle_vs_reference_worst_rel"]) <= 1e-5
    meta = json.loads(str(z["meta"]))
    kind, cfg = meta["kind"], meta["cfg"]
    assert meta["method"] == "dct"
    C, L, B = cfg["num_classes"], cfg["labeled_bs"], cfg["batch_size"]
    sp = tuple(cfg["spatial"])
    if kind == "swin":
        from oracle.swin import OracleSwinUnet
        onet = OracleSwinUnet(C)
    else:
        onet = OracleUNet2D(1, C)
    volume = filler.image((B, 1) + sp, "volume")
    label = filler.labels((B,) + sp, C, torch.uint8)
    ks = [int(z[f"it{it}_rot_k"]) for it in meta["iters"]]
    assert any(k % 2 for k in ks) and len(set(ks)) >= 2          # an odd (transposing) rotation and at least two k
    for it, k in zip(meta["iters"], ks):
        student = filler.fill_state_dict(onet.new_state())
        mom = {n: filler.uniform(student[n].shape, "mom." + n, -0.01, 0.01) for n in student if onet.is_param(n)}
        pre = f"it{it}_"
        orc = dct_step(onet, student, mom, volume, label, k, it, labeled_bs=L, num_classes=C, base_lr=cfg["base_lr"],
                       max_iterations=cfg["max_iterations"], consistency=cfg["consistency"], rampup=cfg["rampup"],
                       drop="off")
        assert orc["consistency_weight"] > 0 and orc["consistency_loss"] > 0
        for key in ("loss", "loss_ce", "loss_dice", "consistency_loss", "consistency_weight", "lr"):
            assert _rel(orc[key], float(z[pre + key])) <= 1e-5, (it, key, orc[key], float(z[pre + key]))
        for key in ("logits", "rot_logits"):
            flat = orc[key].double().flatten()
            idx = np.unique(np.linspace(0, flat.numel() - 1, 64).astype(np.int64))
            assert _rel(flat[idx].numpy(), z[pre + key + "_samples"]) <= 1e-5, (it, key)
            assert _rel(float(flat.sum()), float(z[pre + key + "_sum"])) <= 1e-4, (it, key)
        gn = np.array([float(g.double().norm()) for g in orc["grads"].values()])
        assert np.all(np.abs(gn - z[pre + "grad_norms"]) <= 2e-4 * z[pre + "grad_norms"].max() +
                      6.0 * z[pre + "grad_relerr32"] * z[pre + "grad_norms"])
        params = [n for n in student if onet.is_param(n)]
        assert _rel([float(student[n].double().abs().sum()) for n in params], z[pre + "param_abssum"]) <= 1e-5
        if pre + "buf_sum" in z.files:         # BatchNorm: running statistics updated by both forwards
            bufs = [n for n in student if n.endswith("running_mean") or n.endswith("running_var")]
            assert _rel([float(student[n].double().sum()) for n in bufs], z[pre + "buf_sum"]) <= 1e-5
            nbt = [n for n in student if n.endswith("num_batches_tracked")]
            assert nbt and all(int(student[n]) == 2 for n in nbt)


@pytest.mark.parametrize("seed,n", [(1337, 30000), (7, 5), (1338, 1)])
def test_rotation_schedule_is_the_reference_draw_sequence(seed, n):
    from mis_hip.step import rotation_schedule
    random.seed(seed)              # the reference: random.seed(args.seed), then one randrange per iteration
    assert rotation_schedule(seed, n) == [random.randrange(0, 4) for _ in range(n)]
    assert set(rotation_schedule(seed, 400)) == {0, 1, 2, 3}


@pytest.mark.parametrize("B,L,patch", [(4, 4, [64, 64]), (4, 5, [64, 64]), (4, 0, [64, 64]), (4, 2, [64, 96]),
                                       (24, 12, [256, 224])])
def test_dct_rejects_bad_batch_or_patch_before_any_gpu_call(B, L, patch):
    from mis_hip.step import dct_split
    with pytest.raises(ValueError):
        dct_split(B, L, patch)
    for which in ("2D", "2D_ViT"):
        with pytest.raises(ValueError):
            _script(which).main(["--batch_size", str(B), "--labeled_bs", str(L), "--patch_size"] + [str(p) for p in patch])


def test_dct_batch_rule_accepts():
    from mis_hip.step import dct_split
    assert dct_split(24, 12, [256, 256]) == 12 and dct_split(24, 7, (224, 224)) == 17 and dct_split(2, 1) == 1


@pytest.mark.parametrize("which,flags", [("2D", REF_FLAGS_2D), ("2D_ViT", REF_FLAGS_VIT)])
def test_dct_cli_flags_match_reference(which, flags):
    p = _script(which).parser
    ours = [s for a in p._actions for s in a.option_strings if s not in ("-h", "--help")]
    assert sorted(ours) == sorted(flags)
    args = p.parse_args([])
    for k, v in REF_DEFAULTS[which].items():
        assert getattr(args, k) == v, (k, getattr(args, k), v)
    for k, v in dict(max_iterations=30000, deterministic=1, base_lr=0.01, seed=1337, ema_decay=0.99,
                     consistency_type="mse", consistency=0.1, consistency_rampup=200.0).items():
        assert getattr(args, k) == v, k
    assert p.parse_args(["--patch_size", "32", "32"]).patch_size == [32, 32]


def test_dct_c_abi_is_declared():
    import re
    from mis_hip import lib
    header = open(os.path.join(ROOT, "include", "mis_hip.h")).read()
    names = {"mis_rot90", "mis_dct_tail", "mis_dct_tail_workspace_bytes", "mis_grad_combine"}
    assert names <= set(re.findall(r"\b(mis_[a-z0-9_]+)\s*\(", header))
    assert names <= set(lib.PROTOTYPES)
    L = lib.load()
    assert L.mis_dct_tail_workspace_bytes(12, 12, 4, 256, 256) > 0
    # argument validation happens before any launch
    assert L.mis_rot90(None, 0, None, 0, 1, 1, 4, 4, None, 0, None, 0, None) == -1
    assert L.mis_grad_combine(None, None, 4, 0, None) == -1
    assert L.mis_dct_tail(None, 0, None, 0, None, 1, 1, 1, 2, 4, 4, None, 0, None, 0, 0.0, 1.0, None, None, 0, None, 0,
                          None, 0, None) == -1
