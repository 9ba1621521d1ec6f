"""Generate tests/golden/patch_nce.npz from the REAL reference losses, and pin the CPU restatement against them.

Run in the build container only (it needs the reference checkout, which never travels to the GPU machine):

    python scripts/gen_golden_patch_nce.py

It imports the reference's utils/losses.py by path, evaluates ``ConLoss`` and ``contrastive_loss_sup`` (the definition in
force, :479-531) in float64 on the CPU on a few tiny cases, asserts that both classes agree and that both forms of
tests/patch_nce_oracle.py reproduce them (<= 1e-13; the worst figure is stored), and stores inputs, loss and
d loss / d feat_q of every case.  The fixture is data only.  No test runs this script.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.gen_golden import GOLD, REF  # noqa: E402

import patch_nce_oracle as pno  # noqa: E402

T = 0.07


def _cases():
    g = torch.Generator().manual_seed(20240607)
    signed_q = torch.randn(2, 16, 6, 6, generator=g, dtype=torch.float64)
    signed_k = torch.randn(2, 16, 6, 6, generator=g, dtype=torch.float64)
    relu_q = torch.relu(torch.randn(2, 32, 4, 4, generator=g, dtype=torch.float64))
    relu_k = torch.relu(torch.randn(2, 32, 4, 4, generator=g, dtype=torch.float64))
    relu_q[0, :, 1, 2] = 0          # one all-zero q vector
    relu_k[1, :, 3, 0] = 0          # one all-zero k vector
    one_q = torch.randn(1, 16, 1, 1, generator=g, dtype=torch.float64)
    one_k = torch.randn(1, 16, 1, 1, generator=g, dtype=torch.float64)
    return {"signed_2x16x6x6": (signed_q, signed_k), "relu_zero_2x32x4x4": (relu_q, relu_k), "one_1x16x1x1": (one_q, one_k)}


def main():
    spec = importlib.util.spec_from_file_location("reference_losses", os.path.join(REF, "utils", "losses.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    store = {"names": np.array(sorted(_cases())), "temperature": np.float64(T)}
    worst = 0.0
    for name, (fq, fk) in _cases().items():
        got = []
        for cls in (ref.ConLoss, ref.contrastive_loss_sup):
            q = fq.clone().requires_grad_(True)
            k = fk.clone().requires_grad_(True)
            loss = cls(temperature=T)(q, k)
            loss.backward()
            assert k.grad is None
            got.append((loss.detach(), q.grad.detach()))
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), name
        loss, grad = got[0]
        out, ograd = pno.loss_and_grad(fq, fk, T)
        scale = max(grad.abs().max().item(), 1e-300)
        for what, a, b, s in (("materialised", pno.materialised_loss(fq, fk, T), loss, max(abs(loss.item()), 1.0)),
                              ("rows", pno.rows_loss(fq, fk, T), loss, max(abs(loss.item()), 1.0)), ("grad", ograd, grad, scale)):
            err = (a - b).abs().max().item() / s
            assert err <= 1e-13, (name, what, err)
            worst = max(worst, err)
        store[name + ".feat_q"], store[name + ".feat_k"] = fq.numpy(), fk.numpy()
        store[name + ".loss"], store[name + ".grad"] = loss.numpy(), grad.numpy()                    # ConLoss
        store[name + ".loss_sup"] = got[1][0].numpy()              # contrastive_loss_sup (its gradient: equal, asserted above)
        print(f"{name}: loss {loss.item():.15g}  |grad|max {grad.abs().max().item():.6g}")
    store["oracle_vs_reference_worst_rel"] = np.float64(worst)      # read by test_goldens_record_oracle_pin
    path = os.path.join(GOLD, "patch_nce.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
