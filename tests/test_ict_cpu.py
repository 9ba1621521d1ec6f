"""Interpolation Consistency Training, CPU side: the restatement tests/ict_oracle.ict_step against the golden vectors
of the real reference (scripts/gen_golden_ict.py), the batch-shape rule and the command-line surface of the three
drop-ins.  No GPU is touched."""
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# flag names of code/train_interpolation_consistency_training_{2D,3D,2D_ViT}.py
REF_FLAGS_2D = ["--root_path", "--exp", "--model", "--max_iterations", "--batch_size", "--deterministic", "--base_lr",
                "--patch_size", "--seed", "--num_classes", "--labeled_bs", "--labeled_num", "--ict_alpha",
                "--ema_decay", "--consistency_type", "--consistency", "--consistency_rampup"]
REF_FLAGS_3D = ["--root_path", "--exp", "--model", "--max_iterations", "--batch_size", "--deterministic", "--base_lr",
                "--patch_size", "--seed", "--labeled_bs", "--labeled_num", "--total_labeled_num", "--ict_alpha",
                "--ema_decay", "--consistency_type", "--consistency", "--consistency_rampup"]
REF_FLAGS_VIT = ["--root_path", "--exp", "--model", "--max_iterations", "--batch_size", "--deterministic", "--base_lr",
                 "--patch_size", "--seed", "--num_classes", "--cfg", "--opts", "--zip", "--cache-mode", "--resume",
                 "--accumulation-steps", "--use-checkpoint", "--amp-opt-level", "--tag", "--eval", "--throughput",
                 "--labeled_bs", "--labeled_num", "--ict_alpha", "--ema_decay", "--consistency_type", "--consistency",
                 "--consistency_rampup"]
# defaults that differ between the three scripts
REF_DEFAULTS = {
    "2D": dict(exp="ACDC/Interpolation_Consistency_Training", batch_size=24, labeled_bs=12, labeled_num=300,
               patch_size=[256, 256], model="unet", root_path="../data/ACDC"),
    "3D": dict(exp="BraTS2019_Interpolation_Consistency_Training", batch_size=4, labeled_bs=2, labeled_num=14,
               total_labeled_num=140, patch_size=[96, 96, 96], model="unet_3D", root_path="../data/BraTS2019"),
    "2D_ViT": dict(exp="ACDC/Interpolation_Consistency_Training_ViT", batch_size=24, labeled_bs=12, labeled_num=7,
                   patch_size=[224, 224], model="unet", root_path="../data/ACDC"),
}
CASES = ["ict_unet2d_64", "ict_unet3d_64", "ict_swin_224"]


def _script(which):
    import importlib
    return importlib.import_module("train_interpolation_consistency_training_" + which)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-6))


@pytest.mark.parametrize("name", CASES)
def test_ict_oracle_reproduces_reference_golden(name):
    from ict_oracle import ict_step
    from oracle import filler
    from oracle.nets import OracleUNet2D, OracleUNet3D
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    assert float(z["oracle_vs_reference_worst_rel"]) <= 1e-5
    meta = json.loads(str(z["meta"]))
    kind, cfg, it = meta["kind"], meta["cfg"], meta["iters"][0]
    assert meta["method"] == "ict"
    C, L, B = cfg["num_classes"], cfg["labeled_bs"], cfg["batch_size"]
    sp = tuple(cfg["spatial"])
    if kind == "swin":
        from oracle.swin import OracleSwinUnet
        onet = OracleSwinUnet(C)
    else:
        onet = OracleUNet2D(1, C) if kind == "unet2d" else OracleUNet3D(C, 1)
    student = filler.fill_state_dict(onet.new_state())
    teacher = filler.fill_state_dict({"t." + k: v.clone() for k, v in onet.new_state().items()})
    teacher = {k[2:]: v for k, v in teacher.items()}
    mom = {n: filler.uniform(student[n].shape, "mom." + n, -0.01, 0.01) for n in student if onet.is_param(n)}
    volume = filler.image((B, 1) + sp, "volume")
    label = filler.labels((B,) + sp, C, torch.int64 if kind == "unet3d" else torch.uint8)
    pre = f"it{it}_"
    lam = torch.from_numpy(z[pre + "mix_factors"])
    assert lam.numel() == L // 2 and not torch.any(lam == 0.5)
    orc = ict_step(onet, student, teacher, mom, volume, label, lam, it, labeled_bs=L, num_classes=C,
                   base_lr=cfg["base_lr"], max_iterations=cfg["max_iterations"], ema_decay=cfg["ema_decay"],
                   consistency=cfg["consistency"], rampup=cfg["rampup"], drop_student="off", drop_teacher="off")
    assert orc["consistency_weight"] > 0
    for k in ("loss", "loss_ce", "loss_dice", "consistency_loss", "consistency_weight", "lr"):
        assert _rel(orc[k], float(z[pre + k])) <= 1e-5, (k, orc[k], float(z[pre + k]))
    for key in ("logits", "teacher_logits0", "teacher_logits1"):
        flat = orc[key].double().flatten()
        idx = np.unique(np.linspace(0, flat.numel() - 1, 64).astype(np.int64))
        assert _rel(flat[idx].numpy(), z[pre + key + "_samples"]) <= 1e-5, key
        assert _rel(float(flat.sum()), float(z[pre + key + "_sum"])) <= 1e-4, key
    gn = np.array([float(g.double().norm()) for g in orc["grads"].values()])
    assert np.all(np.abs(gn - z[pre + "grad_norms"]) <= 2e-4 * z[pre + "grad_norms"].max() +
                  6.0 * z[pre + "grad_relerr32"] * z[pre + "grad_norms"])
    if pre + "teacher_buf_sum" in z.files:         # BatchNorm: two teacher forwards, one student forward
        bufs = [n for n in student if n.endswith("running_mean") or n.endswith("running_var")]
        assert _rel([float(student[n].double().sum()) for n in bufs], z[pre + "student_buf_sum"]) <= 1e-5
        assert _rel([float(teacher[n].double().sum()) for n in bufs], z[pre + "teacher_buf_sum"]) <= 1e-5
        nbt = [n for n in teacher if n.endswith("num_batches_tracked")]
        assert nbt and all(int(teacher[n]) == 2 for n in nbt) and all(int(student[n]) == 1 for n in nbt)


@pytest.mark.parametrize("B,L", [(5, 2), (6, 2), (3, 2), (4, 1), (2, 1), (8, 5), (0, 0)])
def test_ict_batch_rule_rejects_before_any_gpu_call(B, L):
    from ict_oracle import ict_split as oracle_split
    from mis_hip.step import ict_split
    with pytest.raises(ValueError):
        ict_split(B, L)
    with pytest.raises(ValueError):
        oracle_split(B, L)
    # the command lines apply the rule before any network or device state exists
    with pytest.raises(ValueError):
        _script("2D").main(["--batch_size", str(B), "--labeled_bs", str(L)])
    with pytest.raises(ValueError):
        _script("3D").main(["--batch_size", str(B), "--labeled_bs", str(L)])


@pytest.mark.parametrize("B,L,M", [(4, 2, 1), (8, 4, 2), (24, 12, 6), (5, 3, 1), (9, 5, 2)])
def test_ict_batch_rule_accepts(B, L, M):
    from ict_oracle import ict_split as oracle_split
    from mis_hip.step import ict_split
    assert ict_split(B, L) == oracle_split(B, L) == M


@pytest.mark.parametrize("which,flags", [("2D", REF_FLAGS_2D), ("3D", REF_FLAGS_3D), ("2D_ViT", REF_FLAGS_VIT)])
def test_ict_cli_flags_match_reference(which, flags):
    p = _script(which).parser
    ours = [s for a in p._actions for s in a.option_strings if s not in ("-h", "--help")]
    assert sorted(ours) == sorted(flags)
    args = p.parse_args([])
    for k, v in REF_DEFAULTS[which].items():
        assert getattr(args, k) == v, (k, getattr(args, k), v)
    for k, v in dict(max_iterations=30000, deterministic=1, base_lr=0.01, seed=1337, ema_decay=0.99,
                     consistency_type="mse", consistency=0.1, consistency_rampup=200.0).items():
        assert getattr(args, k) == v, k
    # --ict_alpha: a float (the reference's type=int cannot parse its own default from a shell)
    assert args.ict_alpha == 0.2
    assert p.parse_args(["--ict_alpha", "0.5"]).ict_alpha == 0.5
    n = 3 if which == "3D" else 2
    assert p.parse_args(["--patch_size"] + ["32"] * n).patch_size == [32] * n


def test_ict_c_abi_is_declared():
    import re
    from mis_hip import lib
    header = open(os.path.join(ROOT, "include", "mis_hip.h")).read()
    names = {"mis_beta_sample", "mis_ict_mix", "mis_ict_tail", "mis_ict_tail_workspace_bytes"}
    assert names <= set(re.findall(r"\b(mis_[a-z0-9_]+)\s*\(", header))
    assert names <= set(lib.PROTOTYPES)
    L = lib.load()
    assert L.mis_ict_tail_workspace_bytes(8, 2, 96 ** 3) > 0
    # argument validation happens before any launch
    assert L.mis_ict_mix(None, None, None, 2, 1, 16, None) == -1
    assert L.mis_beta_sample(None, 4, 0.2, 0, None, None) == -1
    assert L.mis_ict_tail(None, 0, None, 0, None, 0, None, None, 1, 2, 1, 2, 16, 0.0, None, 1.0, None, None, 0, None,
                          0, None) == -1
