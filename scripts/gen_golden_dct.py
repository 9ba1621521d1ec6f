"""Generate tests/golden/dct_*.npz from the REAL reference modules, and pin the CPU restatement against them.

Run in the build container only (it needs the reference checkout, which never travels to the GPU machine):

    python scripts/gen_golden_dct.py [dct_unet2d_64 dct_swin_224]

For every case it (1) runs the reference's own network, utils.losses.DiceLoss and utils.ramps around a restatement of the
deep co-training loop body of code/train_deep_co_training_2D.py:134-167 (_2D_ViT.py:172-205; the scripts parse arguments
at import time and cannot be imported) for one step at each of several (iteration, rotation count) pairs from the same weights, k injected instead of
random.randrange(0, 4), dropout off, (2) runs tests/dct_oracle.dct_step on identical filler inputs, (3) asserts they agree
to <= 1e-5 (relative to scale) and (4) stores the REFERENCE numbers of every iteration.  Fixtures are data only: scalars,
checksums and sampled values.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))     # dct_oracle; the product package stays off the path (its
                                                    # `networks` would shadow the reference's namespace package)

from oracle import filler  # noqa: E402
from oracle.gen_golden import (CFG2D, GOLD, REF, _install_timm_shim, build_reference,  # noqa: E402
                               rel_close, set_reference_dropout, tensor_summary)
from oracle.nets import OracleUNet2D  # noqa: E402


def reference_dct_step(model, optimizer, volume, label, rot_k, iter_num, cfg):
    """Loop body of train_deep_co_training_2D.py:134-167 around the reference modules, with rot_times injected."""
    from torch.nn.modules.loss import CrossEntropyLoss
    from utils import losses, ramps
    L, C = cfg["labeled_bs"], cfg["num_classes"]
    ce_loss, dice_loss = CrossEntropyLoss(), losses.DiceLoss(C)
    unlabeled_volume_batch = volume[L:]
    outputs = model(volume)
    outputs_soft = torch.softmax(outputs, dim=1)
    rotated_unlabeled_volume_batch = torch.rot90(unlabeled_volume_batch, rot_k, [2, 3])
    unlabeled_rot_outputs = model(rotated_unlabeled_volume_batch)
    unlabeled_rot_outputs_soft = torch.softmax(unlabeled_rot_outputs, dim=1)
    loss_ce = ce_loss(outputs[:L], label[:][:L].long())
    loss_dice = dice_loss(outputs_soft[:L], label[:L].unsqueeze(1))
    supervised_loss = 0.5 * (loss_dice + loss_ce)
    w = cfg["consistency"] * ramps.sigmoid_rampup(iter_num // 150, cfg["rampup"])
    consistency_loss = 0.5 * (torch.mean((unlabeled_rot_outputs_soft.detach() - torch.rot90(
        outputs_soft[L:], rot_k, [2, 3])) ** 2) + torch.mean((unlabeled_rot_outputs_soft - torch.rot90(
            outputs_soft[L:].detach(), rot_k, [2, 3])) ** 2))
    loss = supervised_loss + w * consistency_loss
    optimizer.zero_grad()
    loss.backward()
    grads = [p.grad.detach().clone() for p in model.parameters()]
    lr_used = optimizer.param_groups[0]["lr"]
    optimizer.step()
    for g in optimizer.param_groups:                        # :163-165, iter_num before its increment
        g["lr"] = cfg["base_lr"] * (1.0 - iter_num / cfg["max_iterations"]) ** 0.9
    return dict(loss=float(loss), loss_ce=float(loss_ce), loss_dice=float(loss_dice),
                consistency_loss=float(consistency_loss), consistency_weight=w, lr=lr_used, logits=outputs.detach(),
                rot_logits=unlabeled_rot_outputs.detach(), grads=grads)


def _sgd(model, cfg, it, dtype):
    opt = torch.optim.SGD(model.parameters(), lr=cfg["base_lr"], momentum=0.9, weight_decay=0.0001)
    for n, p in model.named_parameters():
        opt.state[p]["momentum_buffer"] = filler.uniform(p.shape, "mom." + n, -0.01, 0.01).to(dtype)
    for g in opt.param_groups:
        g["lr"] = cfg["base_lr"] * (1.0 - (it - 1) / cfg["max_iterations"]) ** 0.9
    return opt


def run_dct_case(name, kind, cfg, it0):
    from dct_oracle import dct_step
    torch.manual_seed(0)
    cfg = {k: v for k, v in cfg.items() if k != "cons_start_iter"}       # no iter_num < 1000 gate in these scripts
    C, L, B = cfg["num_classes"], cfg["labeled_bs"], cfg["batch_size"]
    if kind == "swin":
        from oracle.swin import OracleSwinUnet
        onet = OracleSwinUnet(C)
    else:
        onet = OracleUNet2D(1, C)
    sp = tuple(cfg["spatial"])
    volume = filler.image((B, 1) + sp, "volume")
    label = filler.labels((B,) + sp, C, torch.uint8)
    iters = [it0 + s for s in range(len(cfg["rot_ks"]))]
    out = dict(meta=json.dumps(dict(name=name, kind=kind, cfg=cfg, iters=iters, drop_mode="off", method="dct")))
    worst = 0.0
    for it, k in zip(iters, cfg["rot_ks"]):
        # every iteration is one step from the same filled weights and momentum (only the iteration number and k differ)
        model = build_reference(kind, 1, C)
        sd0 = filler.fill_state_dict({kk: v.clone() for kk, v in model.state_dict().items()})
        model.load_state_dict(sd0)
        model.train()
        set_reference_dropout(model, kind, "off", None)
        m64 = build_reference(kind, 1, C).double()          # float64 run of the same loop: the fp32 rounding envelope
        m64.load_state_dict({kk: (v.double() if v.is_floating_point() else v) for kk, v in sd0.items()})
        m64.train()
        set_reference_dropout(m64, kind, "off", None)
        opt, opt64 = _sgd(model, cfg, it, torch.float32), _sgd(m64, cfg, it, torch.float64)
        student = {kk: v.clone() for kk, v in sd0.items()}
        mom = {n: filler.uniform(student[n].shape, "mom." + n, -0.01, 0.01) for n in student if onet.is_param(n)}
        pnames = [n for n, _ in model.named_parameters()]
        ref = reference_dct_step(model, opt, volume, label, k, it, cfg)
        g64 = reference_dct_step(m64, opt64, volume.double(), label, k, it, cfg)["grads"]
        orc = dct_step(onet, student, mom, volume, label, k, it, labeled_bs=L, num_classes=C, base_lr=cfg["base_lr"],
                       max_iterations=cfg["max_iterations"], consistency=cfg["consistency"], rampup=cfg["rampup"],
                       drop="off")
        assert ref["consistency_weight"] > 0.0, "the fixture must exercise the consistency term"
        for key in ("loss", "loss_ce", "loss_dice", "consistency_loss", "consistency_weight", "lr"):
            worst = max(worst, rel_close(orc[key], ref[key], 1e-5, f"{name} it{it} {key}"))
        for key in ("logits", "rot_logits"):
            worst = max(worst, rel_close(orc[key], ref[key], 1e-5, f"{name} it{it} {key}"))
        for n, g in zip(pnames, ref["grads"]):
            if g.abs().max() > 1e-6:
                rel_close(orc["grads"][n], g, 2e-4, f"{name} it{it} grad {n}")
            else:               # conv biases in front of a BatchNorm: 0 up to rounding in both
                assert (orc["grads"][n] - g).abs().max() <= 1e-6, f"{name} it{it} grad {n}"
        ref_sd = model.state_dict()
        for n in ref_sd:
            if n.endswith("num_batches_tracked"):
                assert int(ref_sd[n]) == int(student[n]) == 2
                continue
            worst = max(worst, rel_close(student[n], ref_sd[n], 1e-5, f"{name} it{it} post-SGD {n}"))
        pre = f"it{it}_"
        for key in ("loss", "loss_ce", "loss_dice", "consistency_loss", "consistency_weight", "lr"):
            out[pre + key] = np.float64(ref[key])
        out[pre + "rot_k"] = np.int64(k)
        for key, t in (("logits_", ref["logits"]), ("rot_logits_", ref["rot_logits"])):
            for kk, v in tensor_summary(t).items():
                out[pre + key + kk] = np.asarray(v)
        out[pre + "grad_norms"] = np.array([float(g.double().norm()) for g in ref["grads"]])
        out[pre + "grad_norms64"] = np.array([float(g.norm()) for g in g64])
        out[pre + "grad_max64"] = np.array([float(g.abs().max()) for g in g64])
        out[pre + "grad_relerr32"] = np.array([float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))
                                               for a, b in zip(ref["grads"], g64)])
        out[pre + "param_abssum"] = np.array([float(ref_sd[n].double().abs().sum()) for n in pnames])
        bufs = [n for n in ref_sd if n.endswith("running_mean") or n.endswith("running_var")]
        if bufs:
            out[pre + "buf_sum"] = np.array([float(ref_sd[n].double().sum()) for n in bufs])
        print(f"{name} it{it} k={k}: loss {ref['loss']:.6f} cons {ref['consistency_loss']:.3e} "
              f"w {ref['consistency_weight']:.4f}")
    out["oracle_vs_reference_worst_rel"] = np.float64(worst)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(f"{name}: oracle vs reference worst rel err {worst:.2e}; wrote {name}.npz")


CASES = [
    # 2-D UNet (BatchNorm, running statistics updated twice per step): 4 + 4; k = 1, 2, 3 on three consecutive steps
    ("dct_unet2d_64", "unet2d", dict(CFG2D, batch_size=8, labeled_bs=4, spatial=[64, 64], rot_ks=[1, 2, 3]), 24000),
    # the ViT script: SwinUnet at 224 x 224, 2 + 2; an odd and an even k
    ("dct_swin_224", "swin", dict(CFG2D, batch_size=4, labeled_bs=2, spatial=[224, 224], rot_ks=[3, 2]), 24000),
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
        run_dct_case(name, kind, cfg, it)


if __name__ == "__main__":
    main()
