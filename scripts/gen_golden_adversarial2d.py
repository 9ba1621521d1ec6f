#!/usr/bin/env python
"""Writes tests/golden/adversarial_2d.npz: the discriminator's side of one iteration of the reference's
train_adversarial_network_2D.py, computed with the REAL reference FCDiscriminator in float64.

    python scripts/gen_golden_adversarial2d.py --reference /path/to/the/reference/checkout

Run on a development machine that has the reference checkout; CPU only.  The reference's own ``FCDiscriminator``
(code/networks/discriminator.py:58-100) is imported from the checkout and called as ``FCDiscriminator(4, ndf=4)`` on
256 x 224 images, N = 2 labeled + 2 unlabeled: conv4 leaves 16 x 14, so the reference's own ``AvgPool2d((7, 7))`` pools one
axis 16 -> 2 with a dropped remainder and the other 14 -> 2 exactly.  The inputs -- image, the student's logits, the
parameters, the two Dropout2d masks -- are closed-form functions of the index (tests/adversarial2d_oracle.py: golden_inputs,
golden_state_dict, golden_masks) that this script and the tests both evaluate; the file stores results only:

  a_logits, a_loss      phase A: DAN.eval(), DAN(softmax(outputs)[2:], image[2:]) and its cross-entropy against 1
  dmap_lattice, dmap_sums   the gradient of that loss at softmax(outputs)[2:]: its values at every 12th pixel per axis from 5
                        (adversarial2d_oracle.lattice) and its sums per (sample, channel)
  b_logits, b_loss      phase B: DAN.train() with the masks injected in place of nn.Dropout2d's draw,
                        DAN(softmax(outputs), image) and its cross-entropy against [1, 1, 0, 0]
  grad/<key>            float64: d b_loss / d parameter, all twelve
  delta1/<key>, delta2/<key>   float32: parameter - initial parameter after one and after two steps of
                        torch.optim.Adam(lr=1e-4, betas=(0.9, 0.99)) on that batch (the second step repeats phase B with the
                        updated parameters and the same masks)
  oracle_vs_reference_worst_rel   the project's float64 oracle on the same inputs against all of the above

The segmenter is not part of the fixture: its logits are an input here (both phases read the same ones).
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NDF, B, L, C, H, W = 4, 4, 2, 4, 256, 224
LR, BETAS = 1e-4, (0.9, 0.99)


class InjectedDropout(torch.nn.Module):
    """Stands in for the reference's ``self.dropout``: the k-th call of a forward multiplies by the k-th mask."""

    def __init__(self, masks):
        super().__init__()
        self.masks, self.calls = masks, 0

    def forward(self, x):
        m = self.masks[self.calls % len(self.masks)]
        self.calls += 1
        return x * m.reshape(m.shape[0], m.shape[1], 1, 1)


def _rel(a, b):
    return float((torch.as_tensor(a).double() - b.double()).abs().max() / b.double().abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (the directory that holds code/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "adversarial_2d.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.reference, "code"))
    from networks.discriminator import FCDiscriminator
    sys.path.pop(0)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import adversarial2d_oracle as ao

    img, logits, _ = ao.golden_inputs(B, C, H, W)
    sd0 = ao.golden_state_dict(C, NDF, 1)
    masks = ao.golden_masks(NDF, B)
    dan = FCDiscriminator(C, ndf=NDF).double()
    # AvgPool2d has no parameters: the reference registers it after the classifier, the state_dict order is unaffected
    assert list(dan.state_dict()) == list(sd0) == list(ao.DISC_KEYS)
    dan.load_state_dict({k: v.double() for k, v in sd0.items()})
    img64 = img.double()
    target = torch.tensor([1] * L + [0] * (B - L))

    # phase A
    dan.eval()
    probs = torch.softmax(logits.double(), 1).requires_grad_(True)
    a_logits = dan(probs[L:], img64[L:])
    a_loss = F.cross_entropy(a_logits, target[:L].long())
    (dmap,) = torch.autograd.grad(a_loss, [probs])
    dmap = dmap[L:]
    store = {"a_logits": a_logits.detach().numpy(), "a_loss": a_loss.detach().numpy(),
             "dmap_lattice": ao.lattice(dmap).numpy().copy(), "dmap_sums": dmap.sum((2, 3)).numpy()}

    # phase B, twice
    dan.train()
    dan.dropout = InjectedDropout(masks)
    opt = torch.optim.Adam(dan.parameters(), lr=LR, betas=BETAS)
    probs = probs.detach()
    deltas = []
    for step in range(2):
        b_logits = dan(probs, img64)
        b_loss = F.cross_entropy(b_logits, target.long())
        opt.zero_grad()
        b_loss.backward()
        if step == 0:
            store.update(b_logits=b_logits.detach().numpy(), b_loss=b_loss.detach().numpy())
            grads = {k: p.grad.detach().clone() for k, p in dan.named_parameters()}
        opt.step()
        deltas.append({k: (p.detach() - sd0[k].double()) for k, p in dan.named_parameters()})
    for k, g in grads.items():
        store[f"grad/{k}"] = g.numpy()
        store[f"delta1/{k}"] = deltas[0][k].numpy().astype(np.float32)
        store[f"delta2/{k}"] = deltas[1][k].numpy().astype(np.float32)

    # the pin every golden records: the project's float64 oracle on these inputs against the reference's results
    ra = ao.disc_step(sd0, torch.softmax(logits.double(), 1)[L:], img[L:], target[:L], None)
    rb = ao.disc_step(sd0, torch.softmax(logits.double(), 1), img, target, masks)
    worst = max(_rel(ra["logits"], a_logits.detach()), _rel(ra["loss"], a_loss.detach()), _rel(ra["dmap"], dmap),
                _rel(rb["logits"], torch.from_numpy(store["b_logits"])), _rel(rb["loss"], torch.from_numpy(store["b_loss"])))
    for k, g in grads.items():
        worst = max(worst, _rel(rb["grads"][k], g))
    assert worst <= 1e-10, worst
    store["oracle_vs_reference_worst_rel"] = np.float64(worst)
    np.savez_compressed(a.out, **store)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes; a_loss {float(a_loss.detach()):.6f} b_loss {float(store['b_loss']):.6f}; "
          f"oracle vs reference {worst:.2e}")


if __name__ == "__main__":
    main()
