#!/usr/bin/env python
"""Writes tests/golden/pnet_40x24.npz: one train-mode forward + backward and one eval-mode forward of the REAL reference PNet2D.

    python scripts/gen_golden_pnet.py --reference /path/to/the/reference/checkout

Run on a development machine that has the reference checkout; CPU only.  The reference's own ``PNet2D``
(code/networks/pnet.py) is loaded from its file and called as ``PNet2D(1, 4, 8, [1, 2, 4, 8, 16])`` (8 filters: 7 964
parameters); this script only builds the inputs and stores data:

  keys, sd/<key>        the fp32 initial state_dict in its order: torch's default initialisation under a fixed seed, the
                        BatchNorm affine parameters moved off (1, 0) by float16-exact amounts so that their gradients matter
  x [3, 1, 40, 24]      float16-exact input: at d = 16 a phase has 3 or 2 rows, at d = 8 the phases are ragged too
  dlogits               float16-exact gradient at the logits
  logits, grad/<key>    float64, train mode, both Dropout2d at p = 0: logits and d sum(logits * dlogits) / d parameter
  after/<key>           the BatchNorm running buffers after that forward
  eval_logits           the eval-mode logits computed afterwards with those buffers
  e32/<key>, e32_after/<key>, e32_logits, e32_eval_logits
                        the reference's own fp32 (one thread) against float64: max |fp32 - fp64| / max |fp64| per tensor
  grad_floor            1e-4 of the net's largest |gradient|: the denominator's lower bound for the gradients that are zero in
                        exact arithmetic (the biases of the convolutions in front of a BatchNorm)
"""
import argparse
import copy
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, CIN, NCLS, F, H, W = 3, 1, 4, 8, 40, 24
RATIOS = [1, 2, 4, 8, 16]
# of the net's largest gradient: the scale of a gradient that is exactly zero in exact arithmetic (the threshold below which
# tests/test_parity_gpu.py leaves a tensor out of its noise ratios)
GRAD_FLOOR = 1e-4


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _f16_exact(a):
    assert np.array_equal(a.astype(np.float16).astype(np.float64), a)
    return a


def _run(net, x, dlogits):
    """train-mode forward + backward, then the eval-mode forward with the updated buffers"""
    net.train()
    net.out.drop1.p = net.out.drop2.p = 0.0
    net.zero_grad()
    logits = net(x)
    (logits * dlogits).sum().backward()
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    after = {k: v.detach().clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
    net.eval()
    with torch.no_grad():
        ev = net(x)
    return logits.detach(), grads, after, ev


def _rel(a, b, floor=0.0):
    """max |a - b| / max |b|; ``floor`` bounds the denominator from below for a tensor that is zero in exact arithmetic (the
    bias of a convolution in front of a BatchNorm: its float64 gradient is rounding noise of 1e-16 with no scale of its own)"""
    return float((a.double() - b).abs().max() / max(float(b.abs().max()), floor))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (the directory that holds code/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pnet_40x24.npz"))
    a = ap.parse_args()
    ref = _load(os.path.join(a.reference, "code", "networks", "pnet.py"), "ref_pnet")

    torch.manual_seed(23)
    net = ref.PNet2D(CIN, NCLS, F, RATIOS)
    rng = np.random.default_rng(23)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if ".in1." in k or ".in2." in k:
                delta = _f16_exact(np.round(rng.uniform(-0.25, 0.25, p.shape) * 256) / 256)
                p.add_(torch.from_numpy(delta).float())
    sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    xn = _f16_exact(np.clip(np.round(rng.standard_normal((N, CIN, H, W)) * 64) / 64, -4, 4))
    dn = _f16_exact(np.round(rng.standard_normal((N, NCLS, H, W)) * 64) / 4096)

    n64 = copy.deepcopy(net).double()
    logits, grads, after, ev = _run(n64, torch.from_numpy(xn), torch.from_numpy(dn))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        l32, g32, after32, ev32 = _run(copy.deepcopy(net), torch.from_numpy(xn).float(), torch.from_numpy(dn).float())
    finally:
        torch.set_num_threads(threads)

    store = {"keys": np.array(list(sd0.keys())), "x": xn.astype(np.float16), "dlogits": dn.astype(np.float16),
             "logits": logits.numpy(), "eval_logits": ev.numpy(), "e32_logits": np.float64(_rel(l32, logits)),
             "e32_eval_logits": np.float64(_rel(ev32, ev))}
    for k, v in sd0.items():
        store[f"sd/{k}"] = v.numpy().copy()
    gfloor = GRAD_FLOOR * max(float(g.abs().max()) for g in grads.values())
    store["grad_floor"] = np.float64(gfloor)
    for k, g in grads.items():
        store[f"grad/{k}"] = g.numpy()
        store[f"e32/{k}"] = np.float64(_rel(g32[k], g, gfloor))
    for k, v in after.items():
        store[f"after/{k}"] = v.numpy()
        if "num_batches" not in k:
            store[f"e32_after/{k}"] = np.float64(_rel(after32[k], v))

    # the pin every golden records: the project's float64 oracle on these inputs against the reference's result
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pnet_oracle as po
    r = po.run(sd0, xn, dn, train=True)
    worst = _rel(r["logits"], logits)
    for k, g in grads.items():
        worst = max(worst, _rel(r["grads"][k], g, gfloor))
    for k, v in after.items():
        if "num_batches" not in k:
            worst = max(worst, _rel(r["after"][k], v))
    sd1 = dict(sd0)
    sd1.update(after)
    worst = max(worst, _rel(po.run(sd1, xn, train=False)["logits"], ev))
    assert worst <= 1e-10, worst
    store["oracle_vs_reference_worst_rel"] = np.float64(worst)
    np.savez_compressed(a.out, **store)
    nparam = sum(p.numel() for p in net.parameters())
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes; {nparam} parameters; oracle vs reference {worst:.2e}; "
          f"e32 logits {store['e32_logits']:.2e}, gradients {min(float(store[f'e32/{k}']) for k in grads):.2e} .. "
          f"{max(float(store[f'e32/{k}']) for k in grads):.2e}")


if __name__ == "__main__":
    main()
