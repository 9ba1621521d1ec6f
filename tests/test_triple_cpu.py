"""Triple-view training, CPU side: the restatement tests/triple_oracle.triple_view_step against the golden vector of the real
reference (scripts/gen_golden_triple.py), the float64 tail reference against plain autograd of the reference's formula, the
batch rule and the command-line surface of the drop-in, and the C ABI's declarations.  No GPU is touched."""
import json
import os
import re

import numpy as np
import pytest
import torch

from dct_oracle import REF_FLAGS_VIT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# code/train_tripleview_2D(demo).py:43-103
REF_DEFAULTS = dict(exp="ACDC/Triple_View", batch_size=16, labeled_bs=8, labeled_num=7, patch_size=[224, 224], model="unet",
                    root_path="../data/ACDC", num_classes=4, cfg="../code/configs/swin_tiny_patch4_window7_224_lite.yaml")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-6))


def test_triple_oracle_reproduces_reference_golden():
    from oracle import filler
    from oracle.nets import OracleUNet2D
    from oracle.swin import OracleSwinUnet
    from triple_oracle import triple_view_step
    z = np.load(os.path.join(GOLD, "triple_224.npz"), allow_pickle=False)
    assert float(z["oracle_vs_reference_worst_rel"]) <= 1e-5
    meta = json.loads(str(z["meta"]))
    cross = json.loads(str(np.load(os.path.join(GOLD, "cross_224.npz"), allow_pickle=False)["meta"]))
    assert meta["method"] == "triple_view" and meta["kinds"] == ["unet2d", "unet2d", "swin"]
    assert meta["cfg"] == cross["cfg"] and meta["iters"] == cross["iters"]      # cross_224's geometry, classes, iteration
    cfg, it = meta["cfg"], meta["iters"][0]
    C, L, B, sp = cfg["num_classes"], cfg["labeled_bs"], cfg["batch_size"], tuple(cfg["spatial"])
    nets = [OracleUNet2D(1, C) if k == "unet2d" else OracleSwinUnet(C) for k in meta["kinds"]]
    sds, moms = [], []
    for m, onet in enumerate(nets):
        sd = filler.fill_state_dict({f"m{m}." + k: v.clone() for k, v in onet.new_state().items()})
        sds.append({k.split(".", 1)[1]: v for k, v in sd.items()})
        moms.append({n: filler.uniform(sds[m][n].shape, f"mom{m}." + n, -0.01, 0.01) for n in sds[m] if onet.is_param(n)})
    volume = filler.image((B, 1) + sp, "volume")
    label = filler.labels((B,) + sp, C, torch.uint8)
    r = triple_view_step(nets, sds, moms, volume, label, it, labeled_bs=L, num_classes=C, base_lr=cfg["base_lr"],
                         max_iterations=cfg["max_iterations"], consistency=cfg["consistency"], rampup=cfg["rampup"])
    pre = f"it{it}_"
    assert r["consistency_weight"] > 0
    assert _rel(r["consistency_weight"], float(z[pre + "consistency_weight"])) <= 1e-5
    assert _rel(r["lr"], float(z[pre + "lr"])) <= 1e-5
    assert abs(r["loss"] - sum(r[f"model{i}_loss"] for i in (1, 2, 3))) <= 1e-6
    for m in range(3):
        i = m + 1
        ce, dl, pa, pb = r["parts"][m]
        assert pa > 0 and pb > 0 and pa != pb
        assert _rel(r[f"model{i}_loss"], float(z[pre + f"model{i}_loss"])) <= 1e-5
        assert _rel(0.5 * (ce + dl), float(z[pre + f"loss{i}_ce_dice"])) <= 1e-5
        assert _rel(pa, float(z[pre + f"pseudo{i}a"])) <= 1e-5 and _rel(pb, float(z[pre + f"pseudo{i}b"])) <= 1e-5
        flat = r[f"logits{i}"].double().flatten()
        idx = np.unique(np.linspace(0, flat.numel() - 1, 64).astype(np.int64))
        assert _rel(flat[idx].numpy(), z[pre + f"logits{i}_samples"]) <= 1e-5
        assert _rel(float(flat.sum()), float(z[pre + f"logits{i}_sum"])) <= 1e-4
        gn = np.array([float(g.double().norm()) for g in r["grads"][m].values()])
        ref_gn = z[pre + f"grad_norms{i}"]
        assert np.all(np.abs(gn - ref_gn) <= 2e-4 * ref_gn.max() + 6.0 * z[pre + f"grad_relerr32_{i}"] * ref_gn)
        params = [n for n in sds[m] if nets[m].is_param(n)]
        assert _rel([float(sds[m][n].double().abs().sum()) for n in params], z[pre + f"param_abssum{i}"]) <= 1e-5


@pytest.mark.parametrize("B,L", [(6, 3), (5, 1), (4, 4), (3, 0)])
def test_tail_oracle_is_the_reference_formula(B, L):
    """tests/triple_oracle.triple_view_tail (float64) == autograd through oracle.losses.dice_loss / F.cross_entropy written
    as the reference writes it (:299-334), with no student's gradient seeing another student's loss."""
    import torch.nn.functional as F
    from oracle.losses import dice_loss
    from triple_oracle import PEERS, triple_view_tail
    g = torch.Generator().manual_seed(B * 10 + L)
    C, sp, w = 3, (1, 6, 10), 0.37
    zs = [torch.randn((B, C) + sp, generator=g) * 3.0 for _ in range(3)]
    label = torch.randint(0, C, (L,) + sp, generator=g).to(torch.uint8)
    outs, grads = triple_view_tail(*zs, label, L, w)
    leaves = [z.double().requires_grad_(True) for z in zs]
    soft = [torch.softmax(z, 1) for z in leaves]
    pseudo = [torch.argmax(s[L:].detach(), 1) for s in soft]
    total = 0.0
    for m in range(3):
        sup = 0.5 * (F.cross_entropy(leaves[m][:L], label.long()) + dice_loss(soft[m][:L], label.unsqueeze(1), C)) if L else 0.0
        ps = [dice_loss(soft[m][L:], pseudo[j].unsqueeze(1), C) if B > L else torch.zeros((), dtype=torch.float64)
              for j in PEERS[m]]
        loss = sup + w * ps[0] + w * ps[1]
        total = total + loss
        assert abs(float(loss) - outs[m][0].item()) <= 1e-12
        assert abs(float(ps[0]) - outs[m][3].item()) <= 1e-12 and abs(float(ps[1]) - outs[m][5].item()) <= 1e-12
        assert outs[m][4].item() == w and outs[m].numel() == 6
    ref = torch.autograd.grad(total, leaves)       # the reference's single backward of loss1 + loss2 + loss3
    for m in range(3):
        assert (grads[m] - ref[m]).abs().max().item() <= 1e-12


def test_triple_cli_flags_match_reference():
    import train_tripleview_2D as script
    p = script.parser
    ours = [s for a in p._actions for s in a.option_strings if s not in ("-h", "--help")]
    assert sorted(ours) == sorted(REF_FLAGS_VIT)
    args = p.parse_args([])
    for k, v in REF_DEFAULTS.items():
        assert getattr(args, k) == v, (k, getattr(args, k), v)
    for k, v in dict(max_iterations=30000, deterministic=1, base_lr=0.01, seed=1337, ema_decay=0.99,
                     consistency_type="mse", consistency=0.1, consistency_rampup=200.0).items():
        assert getattr(args, k) == v, k
    assert p.parse_args(["--patch_size", "32", "32"]).patch_size == [32, 32]


@pytest.mark.parametrize("B,L", [(4, 4), (4, 5), (4, 0), (16, 16)])
def test_triple_rejects_bad_batch_split_before_any_gpu_call(B, L):
    import train_tripleview_2D as script
    from mis_hip.step import triple_split
    with pytest.raises(ValueError):
        triple_split(B, L)
    with pytest.raises(ValueError):
        script.main(["--batch_size", str(B), "--labeled_bs", str(L)])


def test_triple_batch_rule_accepts():
    from mis_hip.step import triple_split
    assert triple_split(16, 8) == 8 and triple_split(2, 1) == 1 and triple_split(24, 7) == 17


def test_triple_c_abi_is_declared():
    from mis_hip import lib
    header = open(os.path.join(ROOT, "include", "mis_hip.h")).read()
    names = {"mis_triple_view_tail", "mis_triple_view_tail_workspace_bytes"}
    assert names <= set(re.findall(r"\b(mis_[a-z0-9_]+)\s*\(", header))
    assert names <= set(lib.PROTOTYPES)
    assert "train_tripleview_2D(demo).py" in header            # the prototypes cite the reference lines they replace
    L = lib.load()
    small, big = L.mis_triple_view_tail_workspace_bytes(2, 4, 224 * 224), L.mis_triple_view_tail_workspace_bytes(16, 4, 224 * 224)
    assert 0 < small < big
    assert L.mis_triple_view_tail_workspace_bytes(0, 4, 64) == -1 and L.mis_triple_view_tail_workspace_bytes(2, 5, 64) == -2
    # argument validation happens before any launch
    null = lambda C: L.mis_triple_view_tail(None, 0, None, 0, None, 0, None, 1, 2, 1, C, 64, 0.1, None, None, None, None,
                                            None, 0, None, 0, None, 0, None, 0, None)
    assert null(4) == -1 and null(5) == -1


def test_trainer_skeleton_names_three_students():
    """_Step names (mom1, out1) .. (mom3, out3) for three students and keeps the one- and two-student names."""
    import inspect
    from mis_hip import step
    sig = inspect.signature(step.TripleViewTrainer.__init__)
    assert list(sig.parameters)[1:4] == ["model1", "model2", "model3"]
    for k in ("labeled_bs", "num_classes", "base_lr", "max_iterations", "consistency", "consistency_rampup", "seed",
              "iter_num", "momentum", "weight_decay", "process_group", "use_tape"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert "TripleViewTrainer" in step.__doc__
