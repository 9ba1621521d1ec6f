"""Generate tests/golden/ict_*.npz from the REAL reference modules, and pin the CPU restatement against them.

Run in the build container only (it needs the reference checkout, which never travels to the GPU machine):

    python scripts/gen_golden_ict.py [ict_unet2d_64 ict_unet3d_64 ict_swin_224]

For every case it (1) runs the reference's own networks, utils.losses.DiceLoss and utils.ramps around a restatement of
the ICT loop body of code/train_interpolation_consistency_training_{2D,3D,2D_ViT}.py (the scripts parse arguments at
import time and cannot be imported), with the Beta mix factors injected instead of np.random.beta, (2) runs
tests/ict_oracle.ict_step on identical filler inputs, (3) asserts they agree to <= 1e-5 (relative to scale) and
(4) stores the REFERENCE numbers.  Fixtures are data only: scalars, checksums and sampled values.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))     # ict_oracle; the product package stays off the path (its
                                                    # `networks` would shadow the reference's namespace package)

from oracle import filler  # noqa: E402
from oracle.gen_golden import (CFG2D, CFG3D, GOLD, REF, _install_timm_shim, build_reference,  # noqa: E402
                               rel_close, set_reference_dropout, tensor_summary)
from oracle.nets import OracleUNet2D, OracleUNet3D  # noqa: E402

FACTORS = [0.3, 0.85]


def reference_ict_step(model, ema_model, optimizer, volume, label, lam, iter_num, cfg):
    """Loop body of train_interpolation_consistency_training_2D.py:150-190 around the reference modules (model,
    ema_model, utils.losses.DiceLoss, utils.ramps), with the mix factors injected."""
    from utils import losses, ramps
    L, C = cfg["labeled_bs"], cfg["num_classes"]
    dice = losses.DiceLoss(C)
    ce = torch.nn.CrossEntropyLoss()
    unlabeled_volume_batch = volume[L:]
    labeled_volume_batch = volume[:L]
    ict_mix_factors = lam.reshape((L // 2,) + (1,) * (volume.dim() - 1)).to(volume.dtype)
    ux0 = unlabeled_volume_batch[0:L // 2, ...]
    ux1 = unlabeled_volume_batch[L // 2:, ...]
    batch_ux_mixed = ux0 * (1.0 - ict_mix_factors) + ux1 * ict_mix_factors
    input_volume_batch = torch.cat([labeled_volume_batch, batch_ux_mixed], dim=0)
    outputs = model(input_volume_batch)
    outputs_soft = torch.softmax(outputs, dim=1)
    with torch.no_grad():
        t0 = ema_model(ux0)
        t1 = ema_model(ux1)
        batch_pred_mixed = torch.softmax(t0, dim=1) * (1.0 - ict_mix_factors) + \
            torch.softmax(t1, dim=1) * ict_mix_factors
    loss_ce = ce(outputs[:L], label[:L].long())
    loss_dice = dice(outputs_soft[:L], label[:L].unsqueeze(1))
    supervised = 0.5 * (loss_dice + loss_ce)
    w = cfg["consistency"] * ramps.sigmoid_rampup(iter_num // 150, cfg["rampup"])
    cons = torch.mean((outputs_soft[L:] - batch_pred_mixed) ** 2)
    loss = supervised + w * cons
    optimizer.zero_grad()
    loss.backward()
    grads = [p.grad.detach().clone() for p in model.parameters()]
    lr_used = optimizer.param_groups[0]["lr"]
    optimizer.step()
    alpha = min(1 - 1 / (iter_num + 1), cfg["ema_decay"])
    for ema_p, p in zip(ema_model.parameters(), model.parameters()):
        ema_p.data.mul_(alpha).add_(p.data, alpha=1 - alpha)
    return dict(loss=float(loss), loss_ce=float(loss_ce), loss_dice=float(loss_dice), consistency_loss=float(cons),
                consistency_weight=w, lr=lr_used, mixed=input_volume_batch.detach(), logits=outputs.detach(),
                teacher_logits0=t0.detach(), teacher_logits1=t1.detach(), grads=grads)


def run_ict_case(name, kind, cfg, it):
    from ict_oracle import ict_step
    torch.manual_seed(0)
    cfg = {k: v for k, v in cfg.items() if k != "cons_start_iter"}       # ICT has no iter_num < 1000 gate
    C, L, B = cfg["num_classes"], cfg["labeled_bs"], cfg["batch_size"]
    M = L // 2
    if kind == "swin":
        from oracle.swin import OracleSwinUnet
        onet = OracleSwinUnet(C)
    else:
        onet = OracleUNet2D(1, C) if kind == "unet2d" else OracleUNet3D(C, 1)
    model, ema_model = build_reference(kind, 1, C), build_reference(kind, 1, C)
    for p in ema_model.parameters():
        p.detach_()
    sd0 = filler.fill_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    tsd0 = filler.fill_state_dict({"t." + k: v.clone() for k, v in model.state_dict().items()})
    tsd0 = {k[2:]: v for k, v in tsd0.items()}
    model.load_state_dict(sd0)
    ema_model.load_state_dict(tsd0)
    model.train(); ema_model.train()
    set_reference_dropout(model, kind, "off", None)
    set_reference_dropout(ema_model, kind, "off", None)
    sp = tuple(cfg["spatial"])
    volume = filler.image((B, 1) + sp, "volume")
    label = filler.labels((B,) + sp, C, torch.int64 if kind == "unet3d" else torch.uint8)
    lam = torch.tensor(cfg["mix_factors"], dtype=torch.float32)
    assert lam.numel() == M
    optimizer = torch.optim.SGD(model.parameters(), lr=cfg["base_lr"], momentum=0.9, weight_decay=0.0001)
    for n, p in model.named_parameters():
        optimizer.state[p]["momentum_buffer"] = filler.uniform(p.shape, "mom." + n, -0.01, 0.01)
    lr_prev = cfg["base_lr"] * (1.0 - (it - 1) / cfg["max_iterations"]) ** 0.9
    for g in optimizer.param_groups:
        g["lr"] = lr_prev
    ref = reference_ict_step(model, ema_model, optimizer, volume, label, lam, it, cfg)
    student = {k: v.clone() for k, v in sd0.items()}
    teacher = {k: v.clone() for k, v in tsd0.items()}
    mom = {n: filler.uniform(student[n].shape, "mom." + n, -0.01, 0.01) for n in student if onet.is_param(n)}
    orc = ict_step(onet, student, teacher, mom, volume, label, lam, it, labeled_bs=L, num_classes=C,
                   base_lr=cfg["base_lr"], max_iterations=cfg["max_iterations"], ema_decay=cfg["ema_decay"],
                   consistency=cfg["consistency"], rampup=cfg["rampup"], drop_student="off", drop_teacher="off")
    assert ref["consistency_weight"] > 0.0, "the fixture must exercise the consistency term"
    worst = 0.0
    for k in ("loss", "loss_ce", "loss_dice", "consistency_loss", "consistency_weight", "lr"):
        worst = max(worst, rel_close(orc[k], ref[k], 1e-5, f"{name} {k}"))
    assert torch.equal(orc["mixed"], ref["mixed"]), "mixed student input differs"
    for k in ("logits", "teacher_logits0", "teacher_logits1"):
        worst = max(worst, rel_close(orc[k], ref[k], 1e-5, f"{name} {k}"))
    pnames = [n for n, _ in model.named_parameters()]
    for n, g in zip(pnames, ref["grads"]):
        rel_close(orc["grads"][n], g, 2e-4, f"{name} grad {n}")
    ref_sd, ref_tsd = model.state_dict(), ema_model.state_dict()
    for n in ref_sd:
        if n.endswith("num_batches_tracked"):
            assert int(ref_sd[n]) == int(student[n]) == 1 and int(ref_tsd[n]) == int(teacher[n]) == 2
            continue
        worst = max(worst, rel_close(student[n], ref_sd[n], 1e-5, f"{name} post-SGD {n}"))
        worst = max(worst, rel_close(teacher[n], ref_tsd[n], 1e-5, f"{name} post-EMA {n}"))
    # float64 run of the same loop: the reference's own fp32 rounding noise per gradient tensor
    m64, e64 = build_reference(kind, 1, C).double(), build_reference(kind, 1, C).double()
    m64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd0.items()})
    e64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in tsd0.items()})
    m64.train(); e64.train()
    set_reference_dropout(m64, kind, "off", None)
    set_reference_dropout(e64, kind, "off", None)
    g64 = reference_ict_step(m64, e64, torch.optim.SGD(m64.parameters(), lr=0.0), volume.double(), label,
                             lam.double(), it, cfg)["grads"]
    out = dict(meta=json.dumps(dict(name=name, kind=kind, cfg=cfg, iters=[it], drop_mode="off", method="ict")))
    pre = f"it{it}_"
    for k in ("loss", "loss_ce", "loss_dice", "consistency_loss", "consistency_weight", "lr"):
        out[pre + k] = np.float64(ref[k])
    out[pre + "mix_factors"] = lam.numpy().astype(np.float32)
    for key, t in (("logits_", ref["logits"]), ("teacher_logits0_", ref["teacher_logits0"]),
                   ("teacher_logits1_", ref["teacher_logits1"])):
        for k, v in tensor_summary(t).items():
            out[pre + key + k] = np.asarray(v)
    out[pre + "grad_norms"] = np.array([float(g.double().norm()) for g in ref["grads"]])
    out[pre + "grad_norms64"] = np.array([float(g.norm()) for g in g64])
    out[pre + "grad_max64"] = np.array([float(g.abs().max()) for g in g64])
    out[pre + "grad_relerr32"] = np.array([float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))
                                           for a, b in zip(ref["grads"], g64)])
    out[pre + "student_abssum"] = np.array([float(ref_sd[n].double().abs().sum()) for n in pnames])
    out[pre + "teacher_abssum"] = np.array([float(ref_tsd[n].double().abs().sum()) for n in pnames])
    bufs = [n for n in ref_sd if n.endswith("running_mean") or n.endswith("running_var")]
    if bufs:
        out[pre + "student_buf_sum"] = np.array([float(ref_sd[n].double().sum()) for n in bufs])
        out[pre + "teacher_buf_sum"] = np.array([float(ref_tsd[n].double().sum()) for n in bufs])
    out["oracle_vs_reference_worst_rel"] = np.float64(worst)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(f"{name}: loss {ref['loss']:.6f} cons {ref['consistency_loss']:.3e} w {ref['consistency_weight']:.4f}; "
          f"oracle vs reference worst rel err {worst:.2e}; wrote {name}.npz")


CASES = [
    # 2-D UNet (BatchNorm): 4 + 4, so M = 2 and each teacher half sees two samples
    ("ict_unet2d_64", "unet2d", dict(CFG2D, batch_size=8, labeled_bs=4, spatial=[64, 64], mix_factors=FACTORS), 24000),
    # unet_3D (InstanceNorm): 2 + 2, M = 1; 64^3 keeps 4^3 voxels per channel at the deepest level
    ("ict_unet3d_64", "unet3d", dict(CFG3D, batch_size=4, labeled_bs=2, spatial=[64, 64, 64],
                                     mix_factors=FACTORS[:1]), 24000),
    # the ViT script (train_interpolation_consistency_training_2D_ViT.py): two SwinUnets at 224 x 224, 2 + 2
    ("ict_swin_224", "swin", dict(CFG2D, batch_size=4, labeled_bs=2, spatial=[224, 224], mix_factors=FACTORS[:1]),
     24000),
]


def main():
    torch.set_num_threads(8)
    only = set(sys.argv[1:])
    sys.path.insert(0, REF)
    for name, kind, cfg, it in CASES:
        if only and name not in only:
            continue
        if kind == "swin":
            _install_timm_shim()
        run_ict_case(name, kind, cfg, it)


if __name__ == "__main__":
    main()
