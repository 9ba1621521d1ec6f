"""Generate tests/golden/triple_224.npz from the REAL reference modules, and pin the CPU restatement against them.

Run in the build container only (it needs the reference checkout, which never travels to the GPU machine):

    python scripts/gen_golden_triple.py

It (1) runs the reference's own UNet (twice), SwinUnet, utils.losses.DiceLoss and utils.ramps around a restatement of the
triple-view loop body of code/train_tripleview_2D(demo).py:290-354 (the script parses arguments at import time and cannot
be imported) for one step, dropout off, (2) runs tests/triple_oracle.triple_view_step on identical filler inputs, (3) asserts
they agree to <= 1e-5 (relative to scale) and (4) stores the REFERENCE numbers.  The fixture is data only: scalars, checksums
and sampled values, with the fields of cross_224.npz for three models.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))     # triple_oracle; the product package stays off the path (its
                                                    # `networks` would shadow the reference's namespace package)

from oracle import filler  # noqa: E402
from oracle.gen_golden import (CFG2D, GOLD, REF, _install_timm_shim, build_reference, make_inputs,  # noqa: E402
                               rel_close, set_reference_dropout, tensor_summary)
from oracle.nets import OracleUNet2D  # noqa: E402

KINDS = ("unet2d", "unet2d", "swin")
PEERS = ((1, 2), (0, 2), (0, 1))


def reference_triple_losses(outs, label, L, C, w):
    """Lines 290-335 around the reference's DiceLoss: (model losses, supervised losses, [(1a, 1b), (2a, 2b), (3a, 3b)])."""
    from torch.nn.modules.loss import CrossEntropyLoss
    from utils import losses
    ce_loss, dice_loss = CrossEntropyLoss(), losses.DiceLoss(C)
    soft = [torch.softmax(o, dim=1) for o in outs]
    sup = [0.5 * (ce_loss(o[:L], label[:L].long()) + dice_loss(s[:L], label[:L].unsqueeze(1))) for o, s in zip(outs, soft)]
    pseudo = [torch.argmax(s[L:].detach(), dim=1, keepdim=False) for s in soft]
    ps = [(dice_loss(soft[m][L:], pseudo[a].unsqueeze(1)), dice_loss(soft[m][L:], pseudo[b].unsqueeze(1)))
          for m, (a, b) in enumerate(PEERS)]
    model_losses = [sup[m] + w * ps[m][0] + w * ps[m][1] for m in range(3)]
    return model_losses, sup, ps


def run_triple_case(name, cfg, it):
    from oracle.swin import OracleSwinUnet
    from triple_oracle import triple_view_step
    from utils import ramps as ref_ramps
    torch.manual_seed(0)
    C, L = cfg["num_classes"], cfg["labeled_bs"]
    nets = [OracleUNet2D(1, C) if k == "unet2d" else OracleSwinUnet(C) for k in KINDS]
    models = [build_reference(k, 1, C) for k in KINDS]
    sds = []
    for m, (onet, model) in enumerate(zip(nets, models)):
        sd = filler.fill_state_dict({f"m{m}." + k: v.clone() for k, v in model.state_dict().items()})
        sd = {k.split(".", 1)[1]: v for k, v in sd.items()}
        assert list(sd.keys()) == [s[0] for s in onet.spec()]
        model.load_state_dict(sd)
        model.train()
        set_reference_dropout(model, KINDS[m], "off", None)
        sds.append(sd)
    volume, label, _ = make_inputs("swin", cfg)
    # ---- reference loop body ----
    opts = [torch.optim.SGD(m.parameters(), lr=cfg["base_lr"], momentum=0.9, weight_decay=0.0001) for m in models]
    lr_prev = cfg["base_lr"] * (1.0 - it / cfg["max_iterations"]) ** 0.9      # set after step it-1, before its increment
    for m, opt in enumerate(opts):
        for n, p in models[m].named_parameters():
            opt.state[p]["momentum_buffer"] = filler.uniform(p.shape, f"mom{m}." + n, -0.01, 0.01)
        for g in opt.param_groups:
            g["lr"] = lr_prev
    outs = [model(volume) for model in models]
    w = cfg["consistency"] * ref_ramps.sigmoid_rampup(it // 150, cfg["rampup"])
    mloss, sup, ps = reference_triple_losses(outs, label, L, C, w)
    assert w > 0 and all(float(t) > 0 for pair in ps for t in pair), "the fixture must exercise all six pseudo terms"
    for opt in opts:
        opt.zero_grad()
    (mloss[0] + mloss[1] + mloss[2]).backward()
    rgrads = [[p.grad.detach().clone() for p in m.parameters()] for m in models]
    for opt in opts:
        opt.step()
    # ---- oracle ----
    osd = [{k: v.clone() for k, v in sd.items()} for sd in sds]
    moms = [{n: filler.uniform(osd[m][n].shape, f"mom{m}." + n, -0.01, 0.01) for n in osd[m] if nets[m].is_param(n)}
            for m in range(3)]
    r = triple_view_step(nets, osd, moms, volume, label, it, labeled_bs=L, num_classes=C, base_lr=cfg["base_lr"],
                         max_iterations=cfg["max_iterations"], consistency=cfg["consistency"], rampup=cfg["rampup"])
    worst = max(rel_close(r["lr"], lr_prev, 1e-5, f"{name} lr"), rel_close(r["consistency_weight"], w, 1e-5, f"{name} w"))
    for m in range(3):
        worst = max(worst, rel_close(r[f"model{m + 1}_loss"], float(mloss[m]), 1e-5, f"{name} model{m + 1}_loss"))
        worst = max(worst, rel_close(r[f"logits{m + 1}"], outs[m].detach(), 1e-5, f"{name} logits{m + 1}"))
        worst = max(worst, rel_close(r["parts"][m][2], float(ps[m][0]), 1e-5, f"{name} pseudo{m + 1}a"))
        worst = max(worst, rel_close(r["parts"][m][3], float(ps[m][1]), 1e-5, f"{name} pseudo{m + 1}b"))
        ref_sd = models[m].state_dict()
        for (n, _), g in zip(models[m].named_parameters(), rgrads[m]):
            rel_close(r["grads"][m][n], g, 2e-4, f"{name} grad m{m} {n}")
            rel_close(osd[m][n], ref_sd[n], 1e-5, f"{name} post-SGD m{m} {n}")
    # ---- float64 run of the same loop: the fp32 rounding envelope of the gradients ----
    m64 = [build_reference(k, 1, C).double() for k in KINDS]
    for m in range(3):
        m64[m].load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sds[m].items()})
        m64[m].train()
        set_reference_dropout(m64[m], KINDS[m], "off", None)
    l64, _, _ = reference_triple_losses([m(volume.double()) for m in m64], label, L, C, w)
    (l64[0] + l64[1] + l64[2]).backward()
    out = dict(meta=json.dumps(dict(name=name, kind="triple", cfg=cfg, iters=[it], drop_mode="off", kinds=list(KINDS),
                                    method="triple_view")))
    pre = f"it{it}_"
    out[pre + "consistency_weight"], out[pre + "lr"] = np.float64(w), np.float64(lr_prev)
    for m in range(3):
        i = m + 1
        out[pre + f"model{i}_loss"] = np.float64(float(mloss[m]))
        out[pre + f"loss{i}_ce_dice"] = np.float64(float(sup[m]))
        out[pre + f"pseudo{i}a"], out[pre + f"pseudo{i}b"] = np.float64(float(ps[m][0])), np.float64(float(ps[m][1]))
        for k, v in tensor_summary(outs[m]).items():
            out[pre + f"logits{i}_{k}"] = np.asarray(v)
        g64 = [p.grad for p in m64[m].parameters()]
        out[pre + f"grad_norms{i}"] = np.array([float(g.double().norm()) for g in rgrads[m]])
        out[pre + f"grad_norms64_{i}"] = np.array([float(g.norm()) for g in g64])
        out[pre + f"grad_max64_{i}"] = np.array([float(g.abs().max()) for g in g64])
        out[pre + f"grad_relerr32_{i}"] = np.array(
            [float((a.double() - b).abs().max() / (b.abs().max() + 1e-300)) for a, b in zip(rgrads[m], g64)])
        sdm = models[m].state_dict()
        pn = [n for n, _ in models[m].named_parameters()]
        out[pre + f"param_abssum{i}"] = np.array([float(sdm[n].double().abs().sum()) for n in pn])
    out["oracle_vs_reference_worst_rel"] = np.float64(worst)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(f"{name}: w {w:.5f} pseudo terms {[round(float(t), 5) for pair in ps for t in pair]}; "
          f"oracle vs reference worst rel err {worst:.2e}; wrote {name}.npz")


def main():
    torch.set_num_threads(8)
    sys.path.insert(0, REF)
    _install_timm_shim()
    # batch geometry, classes and iteration of cross_224's meta
    run_triple_case("triple_224", dict(CFG2D, batch_size=2, labeled_bs=1, spatial=[224, 224]), 1300)


if __name__ == "__main__":
    main()
