"""FixMatch, CPU side: the float64 oracle of tests/fixmatch_oracle.py against torch.autograd of the literal reference
expression (code/train_Fixmatch_CNN_2D.py:132-166, :259-288), the margins of the discrete decisions of every case of the
GPU edge matrix, the schedule, the batch rule, the augmentation's draw order, the command-line surface and the checkpoint
shape.  No GPU is touched."""
import os
import types

import numpy as np
import pytest
import torch

import fixmatch_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# flag names of code/train_Fixmatch_CNN_2D.py:41-68
REF_FLAGS = ["--root_path", "--exp", "--model", "--max_iterations", "--batch_size", "--deterministic", "--base_lr",
             "--patch_size", "--seed", "--num_classes", "--load", "--conf_thresh", "--labeled_bs", "--labeled_num",
             "--ema_decay", "--consistency_type", "--consistency", "--consistency_rampup"]
SMALL = [c for c in fo.matrix() if not c["shape"].startswith("cap")]
_E32 = {}


def _w32():
    return float(torch.tensor(fo.W, dtype=torch.float32))


def _case_e32(c):
    """e32 of one case, computed once (the float64 side at its own decisions; they are the fp32 ones on quantised logits)."""
    key = fo.cid(c)
    if key not in _E32:
        zw, zs, lab = fo.inputs(c)
        ref = fo.fixmatch_tail(zw, zs, lab, c["L"], fo.TAU, _w32())
        inj = {}
        if c["content"] == "cont":
            p, k, _ = fo.decisions(zw, fo.TAU)
            inj = dict(pseudo=p[c["L"]:], comp=k)
        _E32[key] = fo.e32(c, zw, zs, lab, ref, **inj)
    return _E32[key]


@pytest.mark.parametrize("c", SMALL, ids=fo.cid)
def test_oracle_matches_autograd_of_the_reference_expression_in_float64(c):
    zw, zs, lab = fo.inputs(c)
    eps = torch.finfo(torch.float64).eps          # what Categorical clamps with in float64
    o, gw, gs = fo.fixmatch_tail(zw, zs, lab, c["L"], fo.TAU, fo.W, eps=eps)
    o2, gw2, gs2 = fo.reference_autograd(zw, zs, lab, c["L"], fo.TAU, fo.W, torch.float64)
    assert max(fo.scalar_rels(o, o2)) <= 1e-10
    assert fo.rel(gw, gw2) <= 1e-10 and fo.rel(gs, gs2) <= 1e-10
    assert torch.equal(gw[c["L"]:], torch.zeros_like(gw[c["L"]:])) and torch.equal(gw2[c["L"]:], torch.zeros_like(gw2[c["L"]:]))


def test_the_clamp_is_the_float32_one():
    """fp32 autograd follows the oracle with eps = 2^-23, not the one with float64's eps: the clamp is part of the loss."""
    c = fo.case(C=4, content="clamp")
    zw, zs, lab = fo.inputs(c)
    share, _ = fo.clamped_share(zs)
    assert share > 0.15
    o32, _, gs32 = fo.reference_autograd(zw, zs, lab, c["L"], fo.TAU, fo.W, torch.float32)
    near, _, gnear = fo.fixmatch_tail(zw, zs, lab, c["L"], fo.TAU, fo.W, eps=fo.EPS32)
    far, _, gfar = fo.fixmatch_tail(zw, zs, lab, c["L"], fo.TAU, fo.W, eps=torch.finfo(torch.float64).eps)
    # The clamped q are tiny and enter d_strong times their own ps, so the clamp moves the weight by ~5e-6 and the gradient
    # by ~1.5e-6 of its largest entry: small, but several times what separates fp32 torch from the oracle with its clamp.
    e_a, d_a = abs(o32[8].item() - near[8].item()), abs(far[8].item() - near[8].item())
    e_g, d_g = fo.rel(gs32, gnear), fo.rel(gfar, gnear)
    print(f"as_weight: fp32 vs eps 2^-23 {e_a:.2e}, eps float64 vs eps 2^-23 {d_a:.2e}; d_strong: {e_g:.2e}, {d_g:.2e}")
    assert d_a >= 4 * e_a and d_g >= 4 * e_g and e_g <= 1e-6


def test_floors_are_the_largest_e32_of_the_matrix():
    worst_s, worst_t = 0.0, 0.0
    for c in fo.matrix():
        es, ew, et = _case_e32(c)
        worst_s, worst_t = max(worst_s, max(es)), max(worst_t, ew, et)
    print(f"largest e32: scalar {worst_s:.3e}, tensor {worst_t:.3e}")
    # (10 % of slack either way: the order of torch's CPU reductions depends on the number of threads)
    assert worst_s <= 1.1 * fo.FLOOR_SCALAR and fo.FLOOR_SCALAR <= 1.25 * worst_s, worst_s
    assert worst_t <= 1.1 * fo.FLOOR_TENSOR and fo.FLOOR_TENSOR <= 1.25 * worst_t, worst_t


@pytest.mark.parametrize("c", fo.matrix(), ids=fo.cid)
def test_case_margins(c):
    """What the GPU tests assume of their inputs.  Quantised logits: every mask comparison, every arg-max / arg-min gap and
    every q-against-clamp comparison has a float64 relative margin >= 1e-3 (exact ties are resolved first-wins on both sides),
    and fp32 torch takes the float64 decisions everywhere.  Continuous logits: fp32 torch differs from float64 in at most 8
    pixels, all of margin <= 1e-5."""
    zw, zs, lab = fo.inputs(c)
    L = c["L"]
    pm, km = fo.decision_margins(zw, fo.TAU)
    p64, k64, _ = fo.decisions(zw, fo.TAU)
    p32, k32, _ = fo.decisions(zw, fo.TAU, torch.float32)
    if c["content"] != "cont":
        assert fo.clamp_margin(zs) >= 1e-3
        assert pm[L:].min().item() >= 1e-3 and km.min().item() >= 1e-3
        assert torch.equal(p32[L:], p64[L:]) and torch.equal(k32, k64)
    else:
        assert fo.clamp_margin(zs) >= 1e-5
        dp, dk = p32[L:] != p64[L:], k32 != k64
        assert int(dp.sum()) + int(dk.sum()) <= 8
        assert not (dp & (pm[L:] > 1e-5)).any() and not (dk & (km > 1e-5)).any()
    # the planted contents are what they claim
    share, peaks = fo.clamped_share(zs)
    passed = fo.decisions(zw, fo.TAU)[2][L:]
    if c["content"] == "nomask":
        assert not passed.any() and not p64[L:].any()
    if c["content"] == "allmask":
        assert passed.all()
    if c["content"] == "clamp":
        assert share > 0.15
    if c["content"] == "peak":
        assert peaks == c["B"]
    if c["content"] == "sat":
        ps = torch.softmax(zs.float().flatten(2), 1)
        assert (ps == 1).float().mean().item() > 0.1 and ps.min().item() > 0      # saturated, nothing underflows
    if c["content"] == "missing":
        assert not (lab == c["C"] - 1).any()


def test_jitter_formula():
    x = torch.tensor([[[0.0, 0.25, 0.5, 1.0]]], dtype=torch.float64).repeat(3, 1, 1)
    p = torch.tensor([[1.5, 1.0, 0], [1.0, 0.5, 1], [1.8, 1.8, 0]])
    y = fo.color_jitter(x, p)
    assert torch.allclose(y[0], torch.tensor([0.0, 0.375, 0.75, 1.0], dtype=torch.float64))
    assert torch.allclose(y[1], 0.5 * x[1] + 0.5 * x[1].mean())
    b = (1.8 * x[2]).clamp(0, 1)
    want = (float(p[2, 1]) * b + (1 - float(p[2, 1])) * b.mean()).clamp(0, 1)
    assert torch.allclose(y[2], want)


def test_schedule():
    lr, alpha, w = fo.schedule(0, 0.01, 30000, 0.99, 0.1, 200.0)
    assert lr == 0.01 and alpha == 0.0 and abs(w - 0.1 * np.exp(-5.0)) < 1e-15
    lr, alpha, w = fo.schedule(1200, 0.01, 30000, 0.99, 0.1, 200.0)
    assert abs(lr - 0.01 * (1 - 1200 / 30000) ** 0.9) < 1e-15 and alpha == 0.99
    assert abs(w - 0.1 * np.exp(-5.0 * (1 - 8 / 200.0) ** 2)) < 1e-15        # 1200 // 150 = 8: no iter < 1000 gate
    assert fo.schedule(29999, 0.01, 30000, 0.99, 0.1, 200.0)[2] == pytest.approx(0.1 * np.exp(-5.0 * (1 - 199 / 200) ** 2))
    from utils import ramps
    for it in (0, 149, 150, 4500, 30000, 45000):
        assert fo.schedule(it, 0.01, 60000, 0.99, 0.1, 200.0)[2] == pytest.approx(0.1 * ramps.sigmoid_rampup(it // 150, 200.0))


@pytest.mark.parametrize("B,L", [(4, 0), (4, 4), (2, 3), (0, 0), (1, 1)])
def test_fixmatch_split_rejects(B, L):
    from mis_hip.step import fixmatch_split
    import train_Fixmatch_CNN_2D as cli
    with pytest.raises(ValueError):
        fixmatch_split(B, L)
    with pytest.raises(ValueError):           # the command line applies the rule before any network or device state exists
        cli.main(["--batch_size", str(B), "--labeled_bs", str(L)])


def test_fixmatch_split_accepts():
    from mis_hip.step import fixmatch_split
    assert fixmatch_split(24, 12) == 12 and fixmatch_split(2, 1) == 1 and fixmatch_split(5, 4) == 1


def test_weak_strong_draw_order():
    from dataloaders.dataset import AUG2D_DTYPE, WeakStrongAugment, _RotFlip
    pool = types.SimpleNamespace(shapes=[(8, 8)] * 3, offsets=[0, 64, 128])
    np.random.seed(11)
    recs = np.zeros(3, AUG2D_DTYPE)
    gen = _RotFlip((8, 8))
    for i in range(3):
        gen.fill(recs[i], pool, i)
    np.random.seed(11)
    want = [(np.random.randint(0, 4), np.random.randint(0, 2)) for _ in range(3)]     # dataset.py:80, :82 per item
    assert [(int(r["k"]), int(r["axis"])) for r in recs] == want and all(int(r["mode"]) == 1 for r in recs)
    assert [int(r["img_off"]) for r in recs] == [0, 64, 128]
    # the jitter draw consumes torch's generator like ColorJitter.get_params: randperm(4), then four uniforms
    torch.manual_seed(3)
    got = [WeakStrongAugment.draw_jitter() for _ in range(4)]
    torch.manual_seed(3)
    for beta, gamma, order in got:
        idx = torch.randperm(4).tolist()
        u = [float(torch.empty(1).uniform_(lo, hi)) for lo, hi in ((0.2, 1.8), (0.2, 1.8), (0.2, 1.8), (-0.2, 0.2))]
        assert (beta, gamma) == (u[0], u[1]) and order == int(idx.index(1) < idx.index(0))
        assert 0.2 <= beta <= 1.8 and 0.2 <= gamma <= 1.8


def test_cli_flags_match_reference():
    import train_Fixmatch_CNN_2D as cli
    p = cli.parser
    ours = [s for a in p._actions for s in a.option_strings if s not in ("-h", "--help")]
    assert sorted(ours) == sorted(REF_FLAGS)
    args = p.parse_args([])
    for k, v in dict(root_path="../data/ACDC", exp="ACDC/FixMatch_standard_augs", model="unet", max_iterations=30000,
                     batch_size=24, deterministic=1, base_lr=0.01, patch_size=[256, 256], seed=1337, num_classes=4,
                     load=False, conf_thresh=0.8, labeled_bs=12, labeled_num=14, ema_decay=0.99, consistency_type="mse",
                     consistency=0.1, consistency_rampup=200.0).items():
        assert getattr(args, k) == v, k
    assert p.parse_args(["--patch_size", "64", "32"]).patch_size == [64, 32]
    assert p.parse_args(["--load"]).load is True


def test_checkpoint_round_trip(tmp_path):
    from mis_hip import train_common as tc
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(1, 2, 3), torch.nn.BatchNorm2d(2))
    trainer = types.SimpleNamespace(momentum_buf=torch.randn(37), iter_num=6000)
    for n in (3000, 6000, 200):
        tc.save_checkpoint(4, model, trainer, 0.625, str(tmp_path / f"model_iter_{n}.pth"))
    tc.save_checkpoint(4, model, trainer, 0.625, str(tmp_path / "model_iter_400_dice_0.81.pth"))
    (tmp_path / "unet_best_model.pth").write_bytes(b"")
    assert tc.newest_checkpoint(str(tmp_path)) == str(tmp_path / "model_iter_6000.pth")
    assert tc.newest_checkpoint(str(tmp_path / "missing")) is None
    ck = torch.load(str(tmp_path / "model_iter_6000.pth"))
    assert sorted(ck) == ["epoch", "loss", "optimizer_state_dict", "state_dict"]       # util.save_checkpoint's keys
    assert ck["loss"].item() == 0.625                                                     # util.load_checkpoint calls .item()
    other = torch.nn.Sequential(torch.nn.Conv2d(1, 2, 3), torch.nn.BatchNorm2d(2))
    epoch, it, mom, loss = tc.load_checkpoint(str(tmp_path / "model_iter_6000.pth"), other)
    assert (epoch, it, loss) == (4, 6000, 0.625) and torch.equal(mom, trainer.momentum_buf)
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), other.state_dict().values()))


def test_c_abi_is_declared_and_refuses_bad_geometry_before_launch():
    import re
    from mis_hip import lib
    header = open(os.path.join(ROOT, "include", "mis_hip_fixmatch.h")).read()
    names = {"mis_color_jitter", "mis_color_jitter_workspace_bytes", "mis_fixmatch_tail", "mis_fixmatch_tail_workspace_bytes"}
    declared = set(re.findall(r"\b(mis_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    assert declared == names == set(lib.EXTRA_PROTOTYPES["mis_hip_fixmatch.h"]) and not names & set(lib.PROTOTYPES)
    import ctypes
    P, I, LL, F, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_uint
    protos = lib.EXTRA_PROTOTYPES["mis_hip_fixmatch.h"]
    assert protos["mis_color_jitter"] == (I, [P, LL, P, LL, I, LL, P, P, U, P, P, LL, P])
    assert protos["mis_fixmatch_tail"] == (I, [P, LL, P, LL, P, I, I, I, I, LL, F, F, P, P, P, LL, P, LL, P, P, P, LL, P])
    assert protos["mis_fixmatch_tail_workspace_bytes"] == (LL, [I, I, LL])
    L = lib.load()
    assert L.mis_fixmatch_tail_workspace_bytes(24, 4, 256 * 256) > 0 and L.mis_color_jitter_workspace_bytes(24, 65536) == 24 * 16 * 4
    assert L.mis_fixmatch_tail_workspace_bytes(0, 4, 16) == -1 and L.mis_color_jitter_workspace_bytes(2, 0) == -1
    assert L.mis_color_jitter(None, 0, None, 0, 2, 16, None, None, 0, None, None, 0, None) == -1
    assert L.mis_fixmatch_tail(None, 0, None, 0, None, 1, 4, 2, 4, 16, 0.8, 0.1, None, None, None, 0, None, 0, None, None,
                               None, 0, None) == -1
