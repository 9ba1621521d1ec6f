"""CPU suite: the oracle against the committed golden vectors of the real reference, the host-side
schedule logic, and the C-ABI surface (library loads, exports every declared symbol).  No GPU needed.
"""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def _sample_idx(numel):
    return np.unique(np.linspace(0, numel - 1, 64).astype(np.int64))


@pytest.mark.parametrize("name", ["unet2d_64_dropoff", "unet2d_64_masks", "unet2d_deconv_64_masks", "unet3d_64_dropoff",
                                  "unet3d_64_masks", "vnet_64_masks", "vnet_gn_64_masks"])
def test_oracle_reproduces_reference_goldens(name):
    """oracle.step on the fixture inputs == numbers the real reference produced (gen_golden.py)."""
    from oracle import filler
    from oracle.nets import OracleUNet2D, OracleUNet3D, OracleVNet
    from oracle.step import mean_teacher_step
    z, meta = _load(name)
    kind, cfg, iters, mode = meta["kind"], meta["cfg"], meta["iters"], meta["drop_mode"]
    C, L = cfg["num_classes"], cfg["labeled_bs"]
    onet = {"unet2d": lambda: OracleUNet2D(1, C), "unet2d_deconv": lambda: OracleUNet2D(1, C, bilinear=False), "unet3d": lambda: OracleUNet3D(C, 1),
            "vnet": lambda: OracleVNet(C, 1),
            "vnet_groupnorm": lambda: OracleVNet(C, 1, normalization="groupnorm")}[kind]()
    sd0 = filler.fill_state_dict(onet.new_state())
    tsd0 = filler.fill_state_dict({"t." + k: v.clone() for k, v in onet.new_state().items()})
    tsd0 = {k[2:]: v for k, v in tsd0.items()}
    B, sp = cfg["batch_size"], tuple(cfg["spatial"])
    volume = filler.image((B, 1) + sp, "volume")
    label = filler.labels((B,) + sp, C, torch.uint8 if kind.startswith("unet2d") else torch.int64)
    noise = filler.noise((B - L, 1) + sp, "noise")
    if "eval_logits_samples" in z.files:
        lg = onet.forward({k: v.clone() for k, v in sd0.items()}, volume, training=False).double().flatten()
        np.testing.assert_allclose(lg[_sample_idx(lg.numel())].numpy(), z["eval_logits_samples"], rtol=0, atol=2e-5)
    in_shape, t_shape = tuple(volume.shape), (B - L,) + tuple(volume.shape[1:])
    if mode == "off":
        ds = dt = "off"
    else:
        ds = {s: filler.drop_mask(shape, p, f"drop_s{s}") for s, p, shape in onet.drop_sites(in_shape)}
        dt = {s: filler.drop_mask(shape, p, f"drop_t{s}") for s, p, shape in onet.drop_sites(t_shape)}
    pnames = [n for n in sd0 if onet.is_param(n)]
    for it in iters[:1] if kind == "unet3d" else iters:       # keep the CPU suite short
        student = {k: v.clone() for k, v in sd0.items()}
        teacher = {k: v.clone() for k, v in tsd0.items()}
        mom = {} if it == 0 else {n: filler.uniform(student[n].shape, "mom." + n, -0.01, 0.01) for n in pnames}
        r = mean_teacher_step(onet, student, teacher, mom, volume, label, noise, it, labeled_bs=L, num_classes=C,
                              base_lr=cfg["base_lr"], max_iterations=cfg["max_iterations"],
                              ema_decay=cfg["ema_decay"], consistency=cfg["consistency"], rampup=cfg["rampup"],
                              cons_start_iter=cfg["cons_start_iter"], drop_student=ds, drop_teacher=dt)
        pre = f"it{it}_"
        for k in ("loss", "loss_ce", "loss_dice", "consistency_loss", "consistency_weight", "lr"):
            assert abs(r[k] - float(z[pre + k])) <= 1e-5, (k, r[k], float(z[pre + k]))
        lg = r["logits"].double().flatten()
        np.testing.assert_allclose(lg[_sample_idx(lg.numel())].numpy(), z[pre + "logits_samples"], rtol=0, atol=2e-5)
        gn = np.array([float(r["grads"][n].double().norm()) for n in pnames])
        # a conv bias in front of a normalisation has a zero gradient (float64: ~1e-15); its fp32 norm in the golden is the
        # reference's rounding noise, which depends on the CPU's summation order (thread count, ISA).  For those tensors --
        # float64 norm below the reference's own fp32 error -- the oracle must be within that error of the golden
        ref, ref64 = z[pre + "grad_norms"], z[pre + "grad_norms64"]
        floor = np.where(ref64 < np.abs(ref - ref64), np.abs(ref - ref64), 0.0)
        tol = 1e-3 * ref + np.maximum(1e-6 * ref.max(), floor)
        bad = np.abs(gn - ref) > tol
        assert not bad.any(), [(n, a, b, t) for n, a, b, t, f in zip(pnames, gn, ref, tol, bad) if f]
        sabs = np.array([float(student[n].double().abs().sum()) for n in pnames])
        np.testing.assert_allclose(sabs, z[pre + "student_abssum"], rtol=1e-5, atol=1e-6)
        tabs = np.array([float(teacher[n].double().abs().sum()) for n in pnames])
        np.testing.assert_allclose(tabs, z[pre + "teacher_abssum"], rtol=1e-5, atol=1e-6)


def test_medpy_free_metrics_known_answers():
    """utils/metrics.py restates medpy.metric.binary.dc / hd95 (the reference's validation metrics, val_2D.py:7-15):
    closed-form cases."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "cv-ssl-mis_amd"))
    from utils import metrics
    a = np.zeros((20, 20, 20), bool); a[5:10, 5:10, 5:10] = True
    b = np.zeros((20, 20, 20), bool); b[5:10, 5:10, 8:13] = True            # same cube shifted by 3 along z
    assert metrics.dc(a, a) == 1.0 and metrics.dc(a, ~a) == 0.0
    assert abs(metrics.dc(a, b) - 2 * 50 / 250) < 1e-12                     # overlap 5*5*2 voxels of 125 + 125
    assert metrics.hd95(a, a) == 0.0
    # every surface voxel of the shifted cube is at most 3 away from the other surface, the far faces exactly 3
    assert metrics.hd95(a, b) == 3.0
    assert metrics.hd95(a, b, voxelspacing=(1.0, 1.0, 2.0)) == 6.0
    sq = np.zeros((16, 16), bool); sq[4:8, 4:8] = True
    pt = np.zeros((16, 16), bool); pt[4, 12] = True
    assert abs(metrics.hd95(pt, sq) - metrics.hd95(sq, pt)) < 1e-12         # symmetric by construction
    assert metrics.dc(np.zeros(4, bool), np.zeros(4, bool)) == 0.0
    with pytest.raises(RuntimeError):
        metrics.hd95(np.zeros((4, 4), bool), sq)
    # asd / ravd (the 3-D inference CLI's extra columns, code/test_3D_util.py:147-152)
    a10 = np.zeros((20, 20), bool); a10[5:15, 5:15] = True
    b10 = np.zeros((20, 20), bool); b10[5:15, 7:17] = True          # the same square shifted by 2 columns
    half = np.zeros((20, 20), bool); half[5:15, 5:10] = True
    assert metrics.asd(a10, a10) == 0.0 and metrics.asd(a10, b10) == pytest.approx(1.0)
    assert metrics.ravd(a10, b10) == 0.0 and metrics.ravd(half, a10) == pytest.approx(-0.5)
    with pytest.raises(RuntimeError):
        metrics.ravd(a10, np.zeros((20, 20), bool))


def test_uamt_oracle_reproduces_reference_golden():
    """oracle.step.uamt_step == numbers the reference's UA-MT loop produced (gen_golden.run_uamt_case)."""
    from oracle import filler
    from oracle.nets import OracleUNet2D
    from oracle.step import uamt_step, uamt_threshold
    z, meta = _load("uamt_unet2d_64")
    cfg, it = meta["cfg"], meta["iters"][0]
    C, L, B, sp = cfg["num_classes"], cfg["labeled_bs"], cfg["batch_size"], tuple(cfg["spatial"])
    onet = OracleUNet2D(1, C)
    sd0 = filler.fill_state_dict(onet.new_state())
    tsd0 = filler.fill_state_dict({"t." + k: v.clone() for k, v in onet.new_state().items()})
    tsd0 = {k[2:]: v for k, v in tsd0.items()}
    tsd0["decoder.out_conv.weight"] = tsd0["decoder.out_conv.weight"] * cfg["teacher_head_scale"]
    volume = filler.image((B, 1) + sp, "volume")
    label = filler.labels((B,) + sp, C, torch.uint8)
    noise = filler.noise((B - L, 1) + sp, "noise")
    mc = [filler.noise((2 * (B - L), 1) + sp, f"mc_noise{i}") for i in range(4)]
    mom = {n: filler.uniform(sd0[n].shape, "mom." + n, -0.01, 0.01) for n in sd0 if onet.is_param(n)}
    r = uamt_step(onet, sd0, tsd0, mom, volume, label, noise, mc, it, labeled_bs=L, num_classes=C,
                  base_lr=cfg["base_lr"], max_iterations=cfg["max_iterations"], ema_decay=cfg["ema_decay"],
                  consistency=cfg["consistency"], rampup=cfg["rampup"], drop_student="off", drop_teacher="off")
    pre = f"it{it}_"
    for k in ("loss", "loss_ce", "loss_dice", "consistency_loss", "consistency_weight", "lr", "threshold"):
        assert abs(r[k] - float(z[pre + k])) <= 1e-5, (k, r[k], float(z[pre + k]))
    assert abs(r["unmasked"] - float(z[pre + "unmasked"])) <= 2
    assert abs(uamt_threshold(0, 30000) - 0.75 * math.log(2) - 0.25 * math.exp(-5.0) * math.log(2)) < 1e-12
    assert all(int(v) == 5 for k, v in tsd0.items() if k.endswith("num_batches_tracked"))


def test_swin_oracle_reproduces_reference_golden_and_keys():
    """OracleSwinUnet == numbers the real reference SwinUnet produced; state_dict keys/shapes == reference dump."""
    from oracle import filler
    from oracle.step import mean_teacher_step
    from oracle.swin import OracleSwinUnet
    z, meta = _load("swin_224_masks")
    cfg, it = meta["cfg"], meta["iters"][0]
    C, L = cfg["num_classes"], cfg["labeled_bs"]
    onet = OracleSwinUnet(C)
    sd0 = filler.fill_state_dict(onet.new_state())
    lines = [ln.split() for ln in open(os.path.join(GOLD, "swinunet_state_dict_keys.txt")).read().splitlines()[1:]]
    ref_keys = [ln[0] for ln in lines]
    assert ref_keys == list(sd0.keys())
    for ln in lines:
        shape = tuple(int(v) for v in re.findall(r"\d+", " ".join(ln[1:-1])))
        assert tuple(sd0[ln[0]].shape) == shape, ln
    assert sum(v.numel() for k, v in sd0.items() if onet.is_param(k)) == 27168420
    tsd0 = filler.fill_state_dict({"t." + k: v.clone() for k, v in onet.new_state().items()})
    tsd0 = {k[2:]: v for k, v in tsd0.items()}
    B, sp = cfg["batch_size"], tuple(cfg["spatial"])
    volume = filler.image((B, 1) + sp, "volume")
    label = filler.labels((B,) + sp, C, torch.uint8)
    noise = filler.noise((B - L, 1) + sp, "noise")
    ds = {s: filler.drop_mask(shape, p, f"drop_s{s}") for s, p, shape in onet.drop_sites((B,))}
    dt = {s: filler.drop_mask(shape, p, f"drop_t{s}") for s, p, shape in onet.drop_sites((B - L,))}
    pnames = [n for n in sd0 if onet.is_param(n)]
    mom = {n: filler.uniform(sd0[n].shape, "mom." + n, -0.01, 0.01) for n in pnames}
    student = {k: v.clone() for k, v in sd0.items()}
    r = mean_teacher_step(onet, student, tsd0, mom, volume, label, noise, it, labeled_bs=L, num_classes=C,
                          cons_start_iter=cfg["cons_start_iter"], drop_student=ds, drop_teacher=dt)
    pre = f"it{it}_"
    for k in ("loss", "loss_ce", "loss_dice", "consistency_loss"):
        assert abs(r[k] - float(z[pre + k])) <= 1e-5, (k, r[k], float(z[pre + k]))
    gn = np.array([float(r["grads"][n].double().norm()) for n in pnames])
    np.testing.assert_allclose(gn, z[pre + "grad_norms"], rtol=1e-3, atol=1e-6 * z[pre + "grad_norms"].max())


def _cnnvit_inputs(cfg):
    from oracle import filler
    from oracle.nets import OracleUNet2D
    from oracle.swin import OracleSwinUnet
    C, L, B, sp = cfg["num_classes"], cfg["labeled_bs"], cfg["batch_size"], tuple(cfg["spatial"])
    nets = [OracleUNet2D(1, C), OracleSwinUnet(C), OracleSwinUnet(C)]
    sds = []
    for m, onet in enumerate(nets):
        sd = filler.fill_state_dict({f"m{m}." + k: v.clone() for k, v in onet.new_state().items()})
        sds.append({k.split(".", 1)[1]: v for k, v in sd.items()})
    volume = filler.image((B, 1) + sp, "volume")
    label = filler.labels((B,) + sp, C, torch.uint8)
    noise = filler.noise((B - L, 1) + sp, "noise")
    moms = [{n: filler.uniform(sds[m][n].shape, f"mom{m}." + n, -0.01, 0.01) for n in sds[m] if nets[m].is_param(n)}
            for m in range(2)]
    return nets, sds, moms, volume, label, noise


def test_cnn_meet_vit_oracle_reproduces_reference_golden():
    """oracle.step.cnn_meet_vit_step == numbers the reference's train_cnn_meet_vit_2D loop produced
    (gen_golden.run_cnnvit_case): UNet student, SwinUnet student, EMA SwinUnet teacher."""
    from oracle.step import cnn_meet_vit_step, cnn_meet_vit_weights
    z, meta = _load("cnnvit_224")
    cfg, it = meta["cfg"], meta["iters"][0]
    nets, sds, moms, volume, label, noise = _cnnvit_inputs(cfg)
    r = cnn_meet_vit_step(nets[0], nets[1], sds[0], sds[1], sds[2], moms[0], moms[1], volume, label, noise, it,
                          labeled_bs=cfg["labeled_bs"], num_classes=cfg["num_classes"], base_lr=cfg["base_lr"],
                          max_iterations=cfg["max_iterations"], ema_decay=cfg["ema_decay"],
                          consistency=cfg["consistency"], rampup=cfg["rampup"], drop1="off", drop2="off", drop_t="off")
    pre = f"it{it}_"
    for k in ("model1_loss", "model2_loss", "lr", "ema_alpha"):
        assert abs(r[k] - float(z[pre + k])) <= 1e-5, (k, r[k], float(z[pre + k]))
    for m in range(2):
        assert abs(r["parts"][m][2] - float(z[pre + f"pseudo{m + 1}"])) <= 1e-5
        assert abs(r["parts"][m][3] - float(z[pre + f"cons{m + 1}"])) <= 1e-6
        pn = [n for n in sds[m] if nets[m].is_param(n)]
        gn = np.array([float(r["grads"][m][n].double().norm()) for n in pn])
        ref = z[pre + f"grad_norms{m + 1}"]
        np.testing.assert_allclose(gn, ref, rtol=1e-3, atol=1e-6 * ref.max())
        ab = np.array([float(sds[m][n].double().abs().sum()) for n in pn])
        np.testing.assert_allclose(ab, z[pre + f"param_abssum{m + 1}"], rtol=1e-6)
    tn = [n for n in sds[2] if nets[2].is_param(n)]
    np.testing.assert_allclose(np.array([float(sds[2][n].double().abs().sum()) for n in tn]), z[pre + "teacher_abssum"],
                               rtol=1e-6)
    assert abs(r["mt_weight"] - float(z[pre + "weight"])) <= 1e-12 and abs(r["pseudo_weight"] - 7 * r["mt_weight"]) < 1e-12
    # schedule: linear ramp in iter//150 over 200 "epochs"; the mean-teacher term is gated at iteration 1000
    assert cnn_meet_vit_weights(999) == (pytest.approx(7 * 0.1 * 6 / 200), 0.0)
    assert cnn_meet_vit_weights(1000) == (pytest.approx(7 * 0.1 * 6 / 200), pytest.approx(0.1 * 6 / 200))
    assert cnn_meet_vit_weights(10 ** 6) == (pytest.approx(0.7), pytest.approx(0.1))


def test_goldens_record_oracle_pin():
    for f in sorted(os.listdir(GOLD)):
        if not f.endswith(".npz"):
            continue
        z = np.load(os.path.join(GOLD, f))
        if f in ("swin_load_from.npz", "val2d.npz", "val3d.npz", "sampler.npz", "cnnvit_infer.npz"):
            continue        # the reference function's / class's own result is the vector and the product is compared with it
                            # directly -- no oracle in between (checkpoint key mapping; oracle/gen_golden_io.py)
        assert float(z["oracle_vs_reference_worst_rel"]) <= 1e-5, f


def test_schedules_match_reference_formulas():
    """oracle.losses / oracle.step host arithmetic vs closed forms (ramps.py:20-27, train_*2D.py:119-128,234-236)."""
    from oracle.losses import consistency_weight, sigmoid_rampup
    from oracle.step import ema_alpha, lr_for_step
    assert sigmoid_rampup(0, 200.0) == pytest.approx(math.exp(-5.0))
    assert sigmoid_rampup(200, 200.0) == 1.0 and sigmoid_rampup(1e9, 200.0) == 1.0
    assert sigmoid_rampup(5, 0) == 1.0
    assert consistency_weight(29999) == pytest.approx(0.1 * math.exp(-5.0 * (1 - 199 / 200) ** 2))
    assert consistency_weight(149) == consistency_weight(0)
    assert lr_for_step(0, 0.01, 30000) == 0.01
    assert lr_for_step(1, 0.01, 30000) == 0.01
    assert lr_for_step(2, 0.01, 30000) == pytest.approx(0.01 * (1 - 1 / 30000) ** 0.9)
    assert lr_for_step(2, 0.01, 30000, post_increment=True) == pytest.approx(0.01 * (1 - 2 / 30000) ** 0.9)
    assert ema_alpha(0, 0.99) == 0.0 and ema_alpha(9, 0.99) == pytest.approx(0.9) and ema_alpha(1000, 0.99) == 0.99


def test_dice_loss_edge_cases():
    from oracle.losses import dice_loss
    p = torch.zeros(1, 2, 4, 4)
    p[:, 0] = 1.0
    t = torch.zeros(1, 1, 4, 4, dtype=torch.long)
    # perfect prediction of class 0, class 1 absent everywhere: both per-class terms are ~0
    assert float(dice_loss(p, t, 2)) == pytest.approx(0.0, abs=1e-6)
    with pytest.raises(AssertionError, match="predict & target shape do not match"):
        dice_loss(torch.zeros(1, 3, 4, 4), t, 2)


def test_c_abi_library_exports_every_declared_symbol():
    """include/mis_hip.h <-> libmis_hip.so <-> ctypes prototypes: the library is compiled against the header and lib.PROTOTYPES
    is parsed from it; here the parse is held to hand-written expectations that cover every mapped type (no compute calls)."""
    import ctypes
    from mis_hip import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "mis_hip.h")).read()
    # names come from declarations only: the same regex as before, but on the text without its comments
    declared = set(re.findall(r"\b(mis_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    assert declared, "no declarations parsed from include/mis_hip.h"
    assert declared == set(lib.PROTOTYPES), declared ^ set(lib.PROTOTYPES)
    assert len(declared) == 189
    for name in declared:
        assert hasattr(L, name), name
    P, CH, I, LL, ULL = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong
    U, F, D = ctypes.c_uint, ctypes.c_float, ctypes.c_double
    expected = {
        "mis_abi_version": (I, []),                                                  # (void)
        "mis_step_init": (I, [P, ULL, LL, D, D, D, D, D, LL, LL, I, P]),            # unsigned long long, double, long long
        "mis_uamt_tail": (I, [P, LL, P, LL, P, LL, P, I, I, I, I, LL, F, P, LL, D, F, P, P, LL, P, LL, P]),   # double by float
        "mis_beta_sample": (I, [P, I, D, U, P, P]),                                  # unsigned, const MisStepState*
        "mis_conv_fwd_kernel_name": (I, [I] * 9 + [CH, I]),                          # char*
        "mis_surface_metrics": (I, [P, P, I, I, I, I, I, P, P, LL, P]),              # const unsigned char*
        "mis_debug_wgrad_prof": (I, [P]),                                            # unsigned long long*
        "mis_win3d_gather": (I, [P, P] + [I] * 12 + [P]),                            # twelve ints in a row
        "mis_conv_packed_floats": (LL, [I, I, I, I]),                                # long long result
    }
    for name, (res, args) in expected.items():
        assert lib.PROTOTYPES[name] == (res, args), (name, lib.PROTOTYPES[name])
        assert getattr(L, name).restype is res and list(getattr(L, name).argtypes or []) == args, name
    assert L.mis_abi_version() == 1
    assert L.mis_conv_cin_pad(1) == 4 and L.mis_conv_cout_pad(2) == 16
    assert L.mis_conv_packed_floats(16, 48, 27, 0) == 48 * 27 * 16
    assert L.mis_conv_packed_floats(16, 48, 27, 1) == 16 * 27 * 48
    assert L.mis_norm_workspace_bytes(8, 16, 96 ** 3, 1) > 0
    assert L.mis_loss_tail_workspace_bytes(8, 2, 96 ** 3) > 0
    assert L.mis_conv_wgrad_workspace_bytes(8, 48, 16, 96, 96, 96, 3, 3, 3) > 0
    # argument validation happens before any launch
    assert L.mis_conv_fwd(None, 0, None, None, None, 0, 1, 1, 1, 1, 1, 1, 3, 3, 3, None) == -1


def test_c_abi_header_compiles_alone():
    """include/mis_hip.h is self-contained C and C++: the host compiler takes it with no HIP header in sight."""
    import shutil
    import subprocess
    if shutil.which("cc") is None:
        pytest.skip("no host C compiler (cc) on this machine")
    path = os.path.join(ROOT, "include", "mis_hip.h")
    for cc, lang in (("cc", "c"), (shutil.which("c++") and "c++" or "cc", "c++")):
        r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-x", lang, path], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (lang, r.stderr)


_EP_FIELD = {"nt": 2, "nt_short": 1, "nt_rega": 1, "nt_rega_res": 0}      # where a kernel name carries its epilogue


def _name_group(names):
    """The answers of one name query for epilogues 0, 1, ..: one string when they agree (an ``e`` in the epilogue's place: answer
    i carries epilogue i), else the answers joined by ``/``."""
    def generic(i, s):
        family, _, rest = s.partition("<")
        fields, j = rest.rstrip(">").split(","), _EP_FIELD.get(family)
        if j is None or j >= len(fields) or fields[j] != str(i):
            return None
        return family + "<" + ",".join(fields[:j] + ["e"] + fields[j + 1:]) + ">"
    forms = {generic(i, s) for i, s in enumerate(names)}
    if len(forms) == 1 and None not in forms:
        return forms.pop()
    return names[0] if len(set(names)) == 1 else "/".join(names)


def _gemm_dispatch_row(L, mask, M, N, K):
    """One line of tests/golden/gemm_dispatch.txt: what every dispatch query of csrc/gemm.hip answers for (mask, M, N, K).
    Kernel names without ``gemm_`` / ``_kernel`` / blanks, a status code where a query refuses; then the byte counts."""
    import ctypes
    buf = ctypes.create_string_buffer(96)

    def name(fn, *args):
        st = fn(*args, buf, 96)
        return buf.value.decode().replace("gemm_", "").replace("_kernel", "").replace(" ", "") if st == 0 else str(st)
    nt = _name_group([name(L.mis_gemm_nt_kernel_name, M, N, K, e) for e in range(4)])
    split = _name_group([name(L.mis_gemm_nt_split_kernel_name, M, N, K, e) for e in range(5)])
    staged = _name_group([name(L.mis_gemm_nt_split_layout_kernel_name, M, N, K, e, 0) for e in range(5)])
    natural = _name_group([name(L.mis_gemm_nt_split_layout_kernel_name, M, N, K, e, 1) for e in range(6)])
    # dW = dy[K, M]^T . x[K, N]: operands on 16-byte boundaries, then 4 bytes off them
    tn = "/".join(name(L.mis_gemm_tn_kernel_name, 4096 + o, M, 8192 + o, N, 12288 + o, N, M, N, K) for o in (0, 4))
    nbytes = [L.mis_gemm_workspace_bytes(M, N, K, 0), L.mis_gemm_workspace_bytes(M, N, K, 1), L.mis_gemm_dw_workspace_bytes(M, N, K),
              L.mis_gemm_nt_split_workspace_bytes(M, N, K), L.mis_gemm_nt_split_natural(M, N, K), L.mis_gemm_split_bytes(N, K)]
    return f"{mask} {M} {N} {K}|{nt}|{split}|{staged if staged != split else '='}|{natural}|{tn}|" + " ".join(str(int(b)) for b in nbytes)


def test_gemm_dispatch_matches_the_recorded_table():
    """tests/golden/gemm_dispatch.txt was recorded from the library BEFORE its host dispatch became one plan per launch: every
    kernel-name and workspace query for the Linear shapes of SwinUnet (224 x 224, batches 2 / 24 / 48), of UNETR's ViT and of
    the GEMM tests, under precision masks 0 and 7.  The queries print the plan the launcher runs, so a tile rule, threshold or
    slice count that moves shows here, without a GPU.  mis_gemm_expand_kernel_name is newer than the table: pinned by hand."""
    import ctypes
    from mis_hip import lib
    L = lib.load()
    rows = [r for r in open(os.path.join(GOLD, "gemm_dispatch.txt")).read().splitlines() if r and not r.startswith("#")]
    assert len(rows) > 300
    buf = ctypes.create_string_buffer(96)

    def expand(B, H, W, K, P, c, ln_head, planes):
        st = L.mis_gemm_expand_kernel_name(B, H, W, K, P, c, ln_head, planes, buf, 96)
        return buf.value.decode() if st == 0 else st
    prev = L.mis_gemm_set_split_precision(-1)
    try:
        for want in rows:
            mask, M, N, K = (int(v) for v in want.split("|")[0].split())
            L.mis_gemm_set_split_precision(mask)
            assert _gemm_dispatch_row(L, mask, M, N, K) == want
        for mask, p in ((0, 0), (7, 1)):
            L.mis_gemm_set_split_precision(mask)
            # FinalPatchExpand_X4 at 24 images: the pixel-shuffle store keeps it off the short-contraction kernel, whose name the
            # profile row used to carry; on staged planes K < 97 stays with the fp32-B path; (1, 1) / (0, 2): no such entry point
            assert expand(24, 56, 56, 96, 4, 96, 0, 0) == f"gemm_nt_kernel<64, 128, 0, {p}, 4>"
            assert expand(24, 56, 56, 96, 4, 96, 1, 0) == f"gemm_nt_kernel<64, 96, 4, {p}, 4>"
            assert expand(24, 56, 56, 96, 4, 96, 0, 1) == -2 and expand(24, 56, 56, 96, 4, 96, 1, 1) == -2 and expand(24, 56, 56, 96, 4, 96, 0, 2) == -2
            natural = L.mis_gemm_nt_split_natural(24 * 56 * 56, 16 * 96, 96)
            assert natural == (1 if mask else 0)
            assert expand(24, 56, 56, 96, 4, 96, 1, 2) == ("gemm_nt_rega_res_kernel<4>" if natural else -2)
            assert expand(24, 56, 56, 192, 4, 96, 1, 2) == -2           # K > 96: the panel does not stay resident
            # PatchExpand of the decoder (P = 2) on staged planes: the launch mis_gemm_nt_split_kernel_name names
            assert L.mis_gemm_nt_split_kernel_name(24 * 28 * 28, 384, 192, 0, buf, 96) == 0
            staged = buf.value.decode()
            assert expand(24, 28, 28, 192, 2, 96, 0, 1) == staged and staged.startswith("gemm_nt_kernel<")
            assert expand(24, 28, 28, 192, 2, 100, 0, 0) == -2 and expand(0, 28, 28, 192, 2, 96, 0, 0) == -1
    finally:
        L.mis_gemm_set_split_precision(prev)


def test_c_abi_header_parser_refuses_what_it_does_not_know():
    """lib.parse_header never guesses: an unknown type, a struct by value, a variadic or function-pointer parameter raise and
    name the declaration; a declaration broken over lines around a comment with '(' and ';' in it parses."""
    import ctypes
    from mis_hip.lib import parse_header
    ok = parse_header("#define X 1\ntypedef void* mis_stream_t;\ntypedef struct S { int a, b; } S;\n"
                      "long long mis_three_lines(const float* x, /* batch stride (elements); may be 0 */\n"
                      "        long long x_bs,\n        unsigned int n, mis_stream_t stream);\nint mis_none(void);\n")
    assert ok == {"mis_three_lines": (ctypes.c_longlong, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_uint, ctypes.c_void_p]),
                  "mis_none": (ctypes.c_int, [])}
    for bad in ("int mis_bad_scalar(short n);", "int mis_bad_struct(MisAug2D rec, int n);", "int mis_bad_dots(int n, ...);",
                "int mis_bad_callback(int (*cb)(int), int n);", "int mis_bad_unnamed(long long);",
                "int mis_bad_pointee(const MisAug2D* rec);", "size_t mis_bad_result(int n);",
                "int mis_bad_twice(int n); int mis_bad_twice(int n);", "int mis_bad_field; int mis_fine(int n);"):
        with pytest.raises(ValueError, match=r"mis_bad_\w+"):
            parse_header(bad)


def test_product_path_refuses_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from networks.net_factory import net_factory
    from networks.net_factory_3d import net_factory_3d
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net_factory("unet", 1, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net_factory_3d("unet_3D", 1, 2)
    assert net_factory("does_not_exist", 1, 4) is None        # reference behaviour: unknown key -> None
    with pytest.raises(NotImplementedError):
        net_factory("unet_cct", 1, 4)


def test_product_path_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "cv-ssl-mis_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(d, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), os.path.join(d, f)


def test_unetr_oracle_runs_and_has_the_documented_keys():
    """oracle/unetr.py (parity unpinned: MONAI is not vendored in the reference) -- shape / key sanity on CPU."""
    from oracle.unetr import OracleUNETR
    o = OracleUNETR(2, img_size=(32, 32, 32))
    sd = o.new_state()
    keys = list(sd)
    assert keys[0] == "vit.patch_embedding.position_embeddings" and keys[-1] == "out.conv.conv.bias"
    assert "vit.blocks.11.attn.qkv.weight" in sd and "encoder2.blocks.1.1.conv2.conv.weight" in sd
    assert "decoder2.conv_block.conv3.conv.weight" in sd and "encoder1.layer.conv3.conv.weight" in sd
    g = torch.Generator().manual_seed(0)
    for v in sd.values():
        if v.dim() >= 2:
            v.copy_(torch.randn(v.shape, generator=g) * 0.05)
    y = o.forward(sd, torch.rand(1, 1, 32, 32, 32, generator=g), training=False)
    assert y.shape == (1, 2, 32, 32, 32) and torch.isfinite(y).all()
    assert sum(v.numel() for v in OracleUNETR(2).new_state().values()) > 90e6     # the 96^3 network: ~92.8 M parameters


def test_swinunetr_oracle_runs_and_has_the_documented_properties():
    """oracle/swinunetr.py (parity unpinned: MONAI is not vendored in the reference) on CPU: MONAI's parameter names and
    count (62.19 M for feature_size 48), the published structural facts of the restated algorithm (relative-position index,
    27 shift regions, window clipping, the v0.9 merging order with its two duplicated slices), a finite forward."""
    from oracle.swinunetr import (MERGE_OFFSETS, OracleSwinUNETR, region_ids, relative_position_index, window_geometry,
                                  window_partition, window_reverse)
    o = OracleSwinUNETR(2)
    sd = o.new_state()
    keys = list(sd)
    assert keys[0] == "swinViT.patch_embed.proj.weight" and keys[-1] == "out.conv.conv.bias"
    assert "swinViT.layers4.0.blocks.1.attn.relative_position_bias_table" in sd
    assert "swinViT.layers1.0.downsample.reduction.weight" in sd and "encoder10.layer.conv2.conv.weight" in sd
    assert "decoder1.conv_block.conv3.conv.weight" in sd and "encoder2.layer.conv3.conv.weight" not in sd
    assert sum(v.numel() for v in sd.values()) == 62186708
    idx = relative_position_index()
    assert idx.shape == (343, 343) and int(idx.min()) == 0 and int(idx.max()) == 13 ** 3 - 1
    assert int(idx[0, 0]) == int(idx[342, 342]) == (13 ** 3 - 1) // 2        # zero offset = the table's centre
    assert window_geometry((4, 4, 4)) == ((4, 4, 4), (0, 0, 0)) and window_geometry((32, 16, 8)) == ((7, 7, 7), (3, 3, 3))
    r = region_ids((14, 14, 14), (7, 7, 7), (3, 3, 3))
    assert r.shape == (8, 343) and r.unique().numel() == 27
    x = torch.arange(2 * 14 * 14 * 14 * 3, dtype=torch.float32).view(2, 14, 14, 14, 3)
    assert torch.equal(window_reverse(window_partition(x, (7, 7, 7)), (7, 7, 7), (2, 14, 14, 14)), x)
    assert MERGE_OFFSETS[2] == MERGE_OFFSETS[5] and MERGE_OFFSETS[3] == MERGE_OFFSETS[6]      # the v0.9 duplicates
    assert (1, 1, 0) not in MERGE_OFFSETS and (0, 1, 1) not in MERGE_OFFSETS
    g = torch.Generator().manual_seed(0)
    for k, v in sd.items():
        if v.dim() >= 2:
            v.copy_(torch.randn(v.shape, generator=g) * 0.05)
    y = o.forward(sd, torch.rand(1, 1, 32, 32, 64, generator=g), training=False)
    assert y.shape == (1, 2, 32, 32, 64) and torch.isfinite(y).all()
    with pytest.raises(ValueError):
        o.forward(sd, torch.rand(1, 1, 48, 64, 64), training=False)


def _brute_surface(mask):
    """Surface voxels by definition: object voxels with at least one face neighbour outside the object (or the volume)."""
    m = np.pad(mask, 1)
    inner = np.ones_like(m)
    for ax in range(m.ndim):
        inner &= np.roll(m, 1, ax) & np.roll(m, -1, ax)
    return (m & ~inner)[tuple(slice(1, -1) for _ in range(m.ndim))]


@pytest.mark.parametrize("shape,spacing,seed", [((12, 14), None, 0), ((9, 10, 11), None, 1), ((8, 9, 10), (1.0, 0.5, 2.0), 2),
                                                ((16, 16), (0.7, 1.3), 3)])
def test_surface_metrics_against_brute_force(shape, spacing, seed):
    """hd95 / asd of utils/metrics.py (medpy's published algorithm: erosion surfaces + Euclidean distance transform)
    against an independent brute-force evaluation of the definition (explicit surface voxels, all pairwise distances)
    on random blobs.  medpy itself is not installed: this is the strongest pin available for these metrics here."""
    from utils import metrics
    rng = np.random.default_rng(seed)

    def blob():
        z = rng.random(shape)
        for ax in range(len(shape)):          # smooth a little so that the objects have interiors
            z = (z + np.roll(z, 1, ax) + np.roll(z, -1, ax)) / 3
        m = z > np.quantile(z, 0.6)
        m[tuple(s // 2 for s in shape)] = True
        return m

    a, b = blob(), blob()
    sp = np.ones(len(shape)) if spacing is None else np.asarray(spacing)

    def directed(x, y):
        sx, sy = np.argwhere(_brute_surface(x)) * sp, np.argwhere(_brute_surface(y)) * sp
        d = np.sqrt(((sx[:, None, :] - sy[None, :, :]) ** 2).sum(-1))
        return d.min(1)

    d_ab, d_ba = directed(a, b), directed(b, a)
    np.testing.assert_allclose(metrics.hd95(a, b, voxelspacing=spacing), np.percentile(np.hstack((d_ab, d_ba)), 95),
                               rtol=0, atol=1e-9)
    np.testing.assert_allclose(metrics.asd(a, b, voxelspacing=spacing), d_ab.mean(), rtol=0, atol=1e-9)
    np.testing.assert_allclose(metrics.asd(b, a, voxelspacing=spacing), d_ba.mean(), rtol=0, atol=1e-9)
    inter = np.count_nonzero(a & b)
    assert abs(metrics.dc(a, b) - 2.0 * inter / (a.sum() + b.sum())) < 1e-12
    assert abs(metrics.ravd(a, b) - (a.sum() - b.sum()) / b.sum()) < 1e-12


@pytest.mark.timeout(900)
def test_no_packed_fp32_op_takes_low_src0_and_high_other_source():
    """gfx950 erratum (round 5): a v_pk_add / v_pk_mul / v_pk_fma_f32 whose LOW lane reads the low half of src0 and the HIGH half of
    another register returns wrong values while a foreign wave on the same SIMD runs bf16 MFMAs (scripts/ubench/pk_hazard.hip).
    scripts/check_pk_opsel.py disassembles the built library: neither the inline asm nor hipcc's own packing may contain it."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_pk_opsel", os.path.join(ROOT, "scripts", "check_pk_opsel.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = ["	v_pk_add_f32 v[0:1], v[2:3], v[4:5] op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1]",
             "	v_pk_add_f32 v[0:1], v[2:3], v[2:3] op_sel:[0,1] op_sel_hi:[0,1]",
             "	v_pk_add_f32 v[0:1], v[2:3], v[4:5] op_sel:[1,0] op_sel_hi:[1,1] neg_lo:[1,0] neg_hi:[0,1]",
             "	v_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[6:7] op_sel:[0,0,1] op_sel_hi:[1,1,1]"]
    assert mod.scan_text(lines) == [lines[0].strip(), lines[3].strip()]            # the scanner itself
    found, n_pk, n_obj = mod.scan_library(os.path.join(ROOT, "cv-ssl-mis_amd", "mis_hip", "libmis_hip.so"))
    assert n_obj >= 20 and n_pk > 1000
    assert not found, found[:10]


def test_no_mfma_reads_an_inline_asm_valu_result_too_early():
    """hipcc does not insert wait states between an inline-asm vector instruction and an MFMA that reads its result (round 4: a
    hoisted MFMA two instructions behind the packed add producing its B operand gave wrong weight gradients on lanes 48 - 63).
    scripts/check_mfma_hazard.py compiles the kernels that mix the two to gfx950 ISA and looks for such pairs."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_mfma_hazard", os.path.join(ROOT, "scripts", "check_mfma_hazard.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main([]) == 0
