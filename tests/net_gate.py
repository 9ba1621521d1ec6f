"""The net-level float64 gate (tests/test_parity_gpu.py motivates it; tests/test_pnet_gpu.py and
tests/test_attention_unet_gpu.py hold their nets to the same rule).  Per tensor:
|g_hip - g_f64|_max <= max(F64_K * e32, F64_REL) * |g_f64|_max + F64_ABS * (largest |g_f64| of the net), e32 = the reference's
own fp32-vs-fp64 relative error of that tensor; over all tensors the median of (HIP relative error / e32) <= F64_MEDIAN_RATIO."""
import numpy as np
import torch

F64_K, F64_REL, F64_ABS = 6.0, 2e-3, 1e-4
F64_LOGIT = 5e-4
F64_MEDIAN_RATIO = 2.0


def check_grads(model, ref, e32, label):
    """the per-tensor rule and the median ratio; ``ref`` / ``e32``: {parameter: float64 gradient / the reference's fp32 noise}"""
    hip = {n: g.cpu().double() for n, g in model.named_flat(model.flat_grad)}
    assert set(hip) == set(ref)
    gscale = max(float(g.abs().max()) for g in ref.values())
    ratios, worst, rel = [], (0.0, ""), (0.0, "")
    for n, g in ref.items():
        assert torch.isfinite(hip[n]).all(), n
        gmax = float(g.abs().max())
        err = float((hip[n] - g).abs().max())
        tol = max(F64_K * e32[n], F64_REL) * gmax + F64_ABS * gscale
        worst = max(worst, (err / tol, n))
        if gmax > 1e-4 * gscale:            # test_parity_gpu.py's ratio, with its 1e-3 lower bound on e32
            ratios.append((err / gmax) / max(e32[n], 1e-3))
            rel = max(rel, (err / gmax, n))
    print(f"[{label}] worst gradient error / tolerance {worst[0]:.2e} at {worst[1]}; largest relative error {rel[0]:.2e} at "
          f"{rel[1]} (reference fp32: {e32[rel[1]]:.2e}); HIP error / max(e32, 1e-3): median {np.median(ratios):.2e}, "
          f"max {max(ratios):.2e}")
    assert worst[0] <= 1.0, worst
    assert np.median(ratios) <= F64_MEDIAN_RATIO, np.median(ratios)
