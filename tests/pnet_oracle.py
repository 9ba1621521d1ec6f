"""float64 restatement of PNet2D (networks/pnet.py; reference code/networks/pnet.py) in plain torch, for the tests.

CPU only.  ``run(sd, x, dlogits, ...)`` evaluates one forward (train or eval mode) on a state dict with the reference's keys
and, given ``dlogits``, the gradient of ``sum(logits * dlogits)`` at every parameter by autograd.  BatchNorm is written out
(batch mean and biased variance in train mode, running buffers updated with momentum 0.1 and the unbiased variance; the
running buffers in eval mode), LeakyReLU has slope 0.01, and the two Dropout2d layers of the output block take explicit
per-channel SCALE masks ``[N, C, 1, 1]`` (0 or 1 / (1 - p), what ``model.drop_masks`` takes expanded) or are off (``None``).

tests/test_pnet_cpu.py holds this text to tests/golden/pnet_40x24.npz (the reference's own PNet2D in float64) at 1e-10.
"""
import torch
import torch.nn.functional as F

F64 = torch.float64
RATIOS = (1, 2, 4, 8, 16)
SLOPE, EPS, MOMENTUM = 0.01, 1e-5, 0.1


def is_param(name):
    return not (name.endswith("running_mean") or name.endswith("running_var") or name.endswith("num_batches_tracked"))


def _bn(x, p, prefix, train, after):
    g, b = p[f"{prefix}.weight"], p[f"{prefix}.bias"]
    if train:
        n = x.numel() // x.shape[1]
        mean = x.mean((0, 2, 3))
        var = ((x - mean.reshape(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
        after[f"{prefix}.running_mean"] = (1 - MOMENTUM) * p[f"{prefix}.running_mean"] + MOMENTUM * mean.detach()
        after[f"{prefix}.running_var"] = (1 - MOMENTUM) * p[f"{prefix}.running_var"] + MOMENTUM * var.detach() * n / (n - 1)
        after[f"{prefix}.num_batches_tracked"] = p[f"{prefix}.num_batches_tracked"] + 1
    else:
        mean, var = p[f"{prefix}.running_mean"], p[f"{prefix}.running_var"]
    xn = (x - mean.reshape(1, -1, 1, 1)) / torch.sqrt(var.reshape(1, -1, 1, 1) + EPS)
    return xn * g.reshape(1, -1, 1, 1) + b.reshape(1, -1, 1, 1)


def run(sd, x, dlogits=None, train=True, masks=None, ratios=RATIOS):
    """``sd``: {key: tensor / array}; ``x`` [N, C, H, W]; ``masks``: None or the two scale masks (drop1, drop2).
    Returns {"logits", "grads": {parameter: gradient} (with dlogits), "after": {running buffer: value} (train mode)}."""
    p = {}
    for k, v in sd.items():
        t = torch.as_tensor(v)
        p[k] = t.to(F64).clone().requires_grad_(True) if is_param(k) else t.clone().to(F64 if t.is_floating_point() else t.dtype)
    after = {}
    h = torch.as_tensor(x).to(F64)
    outs = []
    for k in range(1, 6):
        r = ratios[k - 1]
        for conv, bn in (("conv1", "in1"), ("conv2", "in2")):
            h = F.conv2d(h, p[f"block{k}.{conv}.weight"], p[f"block{k}.{conv}.bias"], dilation=r, padding=r)
            h = F.leaky_relu(_bn(h, p, f"block{k}.{bn}", train, after), SLOPE)
        outs.append(h)
    h = torch.cat(outs, 1)
    h = F.leaky_relu(F.conv2d(h, p["catblock.conv1.weight"], p["catblock.conv1.bias"]), SLOPE)
    h = F.leaky_relu(F.conv2d(h, p["catblock.conv2.weight"], p["catblock.conv2.bias"]), SLOPE)
    if masks is not None:
        h = h * torch.as_tensor(masks[0]).to(F64)
    h = F.leaky_relu(F.conv2d(h, p["out.conv1.weight"], p["out.conv1.bias"]), SLOPE)
    if masks is not None:
        h = h * torch.as_tensor(masks[1]).to(F64)
    logits = F.conv2d(h, p["out.conv2.weight"], p["out.conv2.bias"])
    res = {"logits": logits.detach(), "after": after}
    if dlogits is not None:
        names = [k for k in p if is_param(k)]
        grads = torch.autograd.grad(logits, [p[k] for k in names], torch.as_tensor(dlogits).to(F64))
        res["grads"] = dict(zip(names, grads))
    return res
