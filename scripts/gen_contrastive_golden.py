#!/usr/bin/env python
"""Writes tests/golden/contrastive_cross.npz: one contrastive cross-teaching loss evaluation by the REAL reference.

    python scripts/gen_contrastive_golden.py --reference /path/to/the/reference/checkout

Run on a development machine that has the reference checkout; CPU only, float64, train mode.  The reference's own
``projectors`` / ``classifier`` (code/networks/projector.py), ``DiceLoss``, ``ConLoss`` and ``contrastive_loss_sup`` (the
definition in force, the second one of code/utils/losses.py) are loaded from their files and called; this script only
builds the inputs, spells the loss lines of code/train_Contrastive_Cross_CNN_2D.py:212-261 around those calls, and stores
data: inputs, the heads' state dicts, every head output, the loss terms, and d loss / d z1, d loss / d z2 from autograd.
The gradients are stored at every 7th element plus their sums (1e-10 on both pins the tensor; the file stays small).

Inputs: logits z1, z2 [6, 4, 32, 32], L = 4, multiples of 1/256 (exact in float16, which is how they are stored), scaled so
that every class wins pixels, and built so that no arg-max sits on a tie: class c carries the fraction c/256 below the
1/64 grid of the rest, so two logits of one pixel differ by at least 1/256.  Both facts are asserted below.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, C, L, H, W_ = 6, 4, 4, 32, 32
WEIGHT = 0.043
STRIDE = 7


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _logits(rng):
    z = np.clip(np.round(rng.standard_normal((B, C, H, W_)) * 2.5 * 64) / 64, -7, 7)
    z = z + np.arange(C).reshape(1, C, 1, 1) / 256.0
    assert np.array_equal(z.astype(np.float16).astype(np.float64), z)
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (the directory that holds code/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "contrastive_cross.npz"))
    a = ap.parse_args()
    proj = _load(os.path.join(a.reference, "code", "networks", "projector.py"), "ref_projector")
    losses = _load(os.path.join(a.reference, "code", "utils", "losses.py"), "ref_losses")

    torch.manual_seed(20)
    heads = dict(classifier_1=proj.classifier(), classifier_2=proj.classifier(), projector_1=proj.projectors(),
                 projector_2=proj.projectors())
    store = {}
    for name, h in heads.items():
        sd = h.state_dict()
        store[f"keys/{name}"] = np.array(list(sd.keys()))
        for k, v in sd.items():
            store[f"sd/{name}/{k}"] = v.numpy().copy()
        h.double().train()

    rng = np.random.default_rng(20)
    z1n, z2n = _logits(rng), _logits(rng)
    label = rng.integers(0, C, (L, H, W_)).astype(np.uint8)
    for z in (z1n, z2n):
        s = np.sort(z, axis=1)
        assert (s[:, -1] - s[:, -2]).min() >= 1.0 / 256 - 1e-12, "an arg-max sits on a tie"
        assert set(np.unique(z.argmax(axis=1))) == set(range(C)), "a class wins no pixel"
    assert set(np.unique(label)) == set(range(C))

    outputs1 = torch.from_numpy(z1n).requires_grad_(True)
    outputs2 = torch.from_numpy(z2n).requires_grad_(True)
    label_batch = torch.from_numpy(label)
    w = WEIGHT
    ce_loss = torch.nn.CrossEntropyLoss()
    dice_loss = losses.DiceLoss(C)
    con_u, con_l = losses.ConLoss(), losses.contrastive_loss_sup()

    soft1, soft2 = torch.softmax(outputs1, dim=1), torch.softmax(outputs2, dim=1)
    sup, ps = [], []
    for out, soft, other in ((outputs1, soft1, soft2), (outputs2, soft2, soft1)):
        sup.append(0.5 * (ce_loss(out[:L], label_batch[:L].long()) + dice_loss(soft[:L], label_batch[:L].unsqueeze(1))))
        pseudo = torch.argmax(other[L:].detach(), dim=1, keepdim=False)
        ps.append(dice_loss(soft[L:], pseudo.unsqueeze(1)))
    feat_l_q = heads["classifier_1"](outputs1[:L][0::2])
    feat_l_k = heads["classifier_2"](outputs2[:L][1::2])
    lc_l = con_l(feat_l_q, feat_l_k)
    feat_q = heads["projector_1"](outputs1[L:])
    feat_k = heads["projector_2"](outputs2[L:])
    lc_u = con_u(feat_q, feat_k)
    loss = 2 * (sup[0] + sup[1]) + 0.5 * (lc_l + lc_u) + 1.25 * (w * ps[0] + w * ps[1])
    loss.backward()

    # the buffers the reference's BatchNorm layers hold after this one train-mode forward
    for name, h in heads.items():
        for k, v in h.state_dict().items():
            if "running" in k or "num_batches" in k:
                store[f"after/{name}/{k}"] = v.numpy().copy()

    g1, g2 = outputs1.grad.numpy(), outputs2.grad.numpy()
    store.update(z1=z1n.astype(np.float16), z2=z2n.astype(np.float16), label=label, w=np.float64(w), L=np.int64(L),
                 feat_l_q=feat_l_q.detach().numpy(), feat_l_k=feat_l_k.detach().numpy(), feat_q=feat_q.detach().numpy(),
                 feat_k=feat_k.detach().numpy(), Lc_l=lc_l.item(), Lc_u=lc_u.item(), sup_1=sup[0].item(),
                 sup_2=sup[1].item(), ps_1=ps[0].item(), ps_2=ps[1].item(), loss=loss.item(),
                 model1_loss=(sup[0] + w * ps[0]).item(), model2_loss=(sup[1] + w * ps[1]).item(),
                 grad_stride=np.int64(STRIDE), dz1_samples=g1.reshape(-1)[::STRIDE].copy(),
                 dz2_samples=g2.reshape(-1)[::STRIDE].copy(), dz1_sum=g1.sum(), dz2_sum=g2.sum(),
                 dz1_abs_sum=np.abs(g1).sum(), dz2_abs_sum=np.abs(g2).sum(),
                 dz1_row_abs_sum=np.abs(g1).sum(axis=(1, 2, 3)), dz2_row_abs_sum=np.abs(g2).sum(axis=(1, 2, 3)))
    # the pin every golden records (tests/test_oracle_cpu.py): the project's float64 oracle on these inputs against the
    # reference's result, worst relative deviation over the loss terms, the head outputs and the sampled gradients
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import contrastive_oracle as co
    hs = {n: {k[len(f"sd/{n}/"):]: v for k, v in store.items() if k.startswith(f"sd/{n}/")} for n in heads}
    r = co.loss_and_grads(z1n, z2n, label, L, w, hs)
    worst = max(abs(r[k] - float(store[k])) / abs(float(store[k])) for k in ("loss", "Lc_l", "Lc_u", "sup_1", "sup_2", "ps_1", "ps_2"))
    for k in ("feat_l_q", "feat_l_k", "feat_q", "feat_k"):
        worst = max(worst, float(np.abs(r[k] - store[k]).max() / np.abs(store[k]).max()))
    for k, g in (("dz1", g1), ("dz2", g2)):
        worst = max(worst, float(np.abs(r[k] - g).max() / np.abs(g).max()))
    assert worst <= 1e-10, worst
    store["oracle_vs_reference_worst_rel"] = np.float64(worst)
    np.savez_compressed(a.out, **store)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes; loss {loss.item():.12f} Lc_l {lc_l.item():.6f} Lc_u {lc_u.item():.6f}")
    sys.stdout.flush()


if __name__ == "__main__":
    main()
