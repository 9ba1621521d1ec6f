#!/usr/bin/env python
"""Writes tests/golden/attention_unet_32x16x48.npz: one train-mode forward + backward and one eval-mode forward of the REAL
reference Attention_UNet.

    python scripts/gen_golden_attention_unet.py --reference /path/to/the/reference/checkout

Run on a development machine that has the reference checkout; CPU only.  The reference's own ``Attention_UNet``
(code/networks/attention_unet.py) is imported from the checkout and called as ``Attention_UNet(feature_scale=64, n_classes=2,
in_channels=1)`` (filters 1, 2, 4, 8, 16: 25 628 parameters); this script only builds the inputs and stores data:

  keys, sd/<key>        the fp32 initial state_dict in its order: the reference's kaiming initialisation under a fixed seed, the
                        BatchNorm affine parameters moved off (1, 0) by float16-exact amounts so that their gradients matter
  x [2, 1, 32, 16, 48]  float16-exact input: the centre is 2 x 1 x 3 (a coarse extent of 1 in the level-4 gate), dsv4 is
                        up-sampled by 8 from 4 x 2 x 6
  dlogits               float16-exact gradient at the logits
  grad/<key>            float64, train mode: d sum(logits * dlogits) / d parameter
  after/<key>           the BatchNorm running buffers after that forward
  logits_idx, logits, eval_logits
                        float64 train-mode logits and the eval-mode logits computed afterwards with those buffers, at LOGIT_POINTS
                        flat positions of the [2, 2, 32, 16, 48] tensor (the eight corners of every (image, class) volume and a
                        seeded draw): the two full tensors in float64 are 1.5 MB, the file has to stay under 400 KB, and every
                        voxel of the logits already reaches the stored gradients through dlogits.  The tests compare full logits
                        with tests/attention_unet_oracle.py, which this file pins at these positions
  e32, e32_after, e32_logits, e32_eval_logits
                        the reference's own fp32 (one thread) against float64: max |fp32 - fp64| / max |fp64| per tensor (the
                        logits' over the full tensors).  ``e32`` is one vector over the parameters and ``e32_after`` one over the
                        running_mean / running_var buffers, both in the order of ``keys`` (an archive member per scalar costs
                        250 bytes of headers: 45 KB for the 189 of them)
  grad_floor            1e-4 of the net's largest |gradient|: the denominator's lower bound for the gradients that are zero in
                        exact arithmetic (the biases of the convolutions in front of a normalisation)
"""
import argparse
import copy
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, CIN, NCLS, FEATURE_SCALE, D, H, W = 2, 1, 2, 64, 32, 16, 48
GRAD_FLOOR = 1e-4
LOGIT_POINTS = 512


def _f16_exact(a):
    assert np.array_equal(a.astype(np.float16).astype(np.float64), a)
    return a


def _run(net, x, dlogits):
    """train-mode forward + backward, then the eval-mode forward with the updated buffers"""
    net.train()
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
    return float((a.double() - b).abs().max() / max(float(b.abs().max()), floor))


def logit_points(rng):
    """flat indices into [N, NCLS, D, H, W]: the corners of every volume, then a seeded draw without repetition"""
    idx = [np.ravel_multi_index((n, c, z, y, x), (N, NCLS, D, H, W)) for n in range(N) for c in range(NCLS)
           for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)]
    rest = np.setdiff1d(np.arange(N * NCLS * D * H * W), idx)
    return np.sort(np.concatenate([idx, rng.choice(rest, LOGIT_POINTS - len(idx), replace=False)])).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (the directory that holds code/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "attention_unet_32x16x48.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.reference, "code"))
    warnings.filterwarnings("ignore")            # the reference calls F.upsample / F.sigmoid
    from networks.attention_unet import Attention_UNet
    sys.path.pop(0)

    torch.manual_seed(29)
    net = Attention_UNet(feature_scale=FEATURE_SCALE, n_classes=NCLS, in_channels=CIN)
    rng = np.random.default_rng(29)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if ".W.1." in k or ".combine_gates.1." in k:
                delta = _f16_exact(np.round(rng.uniform(-0.25, 0.25, p.shape) * 256) / 256)
                p.add_(torch.from_numpy(delta).float())
    sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    # few distinct values (steps of 1/2 resp. 1/64): the two arrays compress to a fraction of their 16 bits per voxel
    xn = _f16_exact(np.clip(np.round(rng.standard_normal((N, CIN, D, H, W)) * 2) / 2, -3, 3))
    dn = _f16_exact(np.clip(np.round(rng.standard_normal((N, NCLS, D, H, W)) * 0.8), -2, 2) / 64)

    n64 = copy.deepcopy(net).double()
    logits, grads, after, ev = _run(n64, torch.from_numpy(xn), torch.from_numpy(dn))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        l32, g32, after32, ev32 = _run(copy.deepcopy(net), torch.from_numpy(xn).float(), torch.from_numpy(dn).float())
    finally:
        torch.set_num_threads(threads)
    assert all(float(g.abs().max()) > 0 for g in grads.values())

    idx = logit_points(rng)
    store = {"keys": np.array(list(sd0.keys())), "x": xn.astype(np.float16), "dlogits": dn.astype(np.float16),
             "logits_idx": idx, "logits": logits.numpy().reshape(-1)[idx], "eval_logits": ev.numpy().reshape(-1)[idx],
             "e32_logits": np.float64(_rel(l32, logits)), "e32_eval_logits": np.float64(_rel(ev32, ev))}
    for k, v in sd0.items():
        store[f"sd/{k}"] = v.numpy().copy()
    gfloor = GRAD_FLOOR * max(float(g.abs().max()) for g in grads.values())
    store["grad_floor"] = np.float64(gfloor)
    for k, g in grads.items():
        store[f"grad/{k}"] = g.numpy()
    for k, v in after.items():
        store[f"after/{k}"] = v.numpy()
    store["e32"] = np.array([_rel(g32[k], g, gfloor) for k, g in grads.items()])
    store["e32_after"] = np.array([_rel(after32[k], v) for k, v in after.items() if "num_batches" not in k])
    assert list(grads) == [k for k in sd0 if k in grads] and list(after) == [k for k in sd0 if k in after]

    # the pin every golden records: the project's float64 oracle on these inputs against the reference's result (full tensors)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import attention_unet_oracle as ao
    r = ao.run(sd0, xn, dn, train=True)
    worst = _rel(r["logits"], logits)
    for k, g in grads.items():
        worst = max(worst, _rel(r["grads"][k], g, gfloor))
    for k, v in after.items():
        if "num_batches" not in k:
            worst = max(worst, _rel(r["after"][k], v))
    sd1 = dict(sd0)
    sd1.update(after)
    worst = max(worst, _rel(ao.run(sd1, xn, train=False)["logits"], ev))
    assert worst <= 1e-10, worst
    store["oracle_vs_reference_worst_rel"] = np.float64(worst)
    np.savez_compressed(a.out, **store)
    nparam = sum(p.numel() for p in net.parameters())
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes; {nparam} parameters; oracle vs reference {worst:.2e}; "
          f"e32 logits {store['e32_logits']:.2e}, gradients {store['e32'].min():.2e} .. {store['e32'].max():.2e}")


if __name__ == "__main__":
    main()
