"""float64 restatement of the Attention U-Net (networks/attention_unet.py; reference code/networks/attention_unet.py with
grid_attention_layer.py and utils.py) in plain torch, for the tests.  CPU only.

Written out here, not taken from torch: the trilinear up-sampling by an integer factor (``up_matrix``: the per-axis weight
matrix of PyTorch's align_corners=False rule, ``upsample_int`` / ``upsample_int_adjoint``), the grid attention gate in the
stacked form the kernels compute (``gate_map``, ``gate_apply``) and the gate's gradients as formulas (``gate_apply_bwd``,
``gate_map_bwd``), InstanceNorm and BatchNorm (batch statistics and the running-buffer update in train mode, the running
buffers in eval mode).  ``run(sd, x, dlogits, train)`` evaluates the net on a state dict with the reference's keys and, given
``dlogits``, the gradient of ``sum(logits * dlogits)`` at every parameter by autograd through those expressions.

``reference32``: the same quantities from torch's own fp32 CPU operators (F.interpolate, F.conv3d, torch.sigmoid, autograd):
the e32 of the kernel tests' tolerance rule.

tests/test_attention_unet_cpu.py holds this text to tests/golden/attention_unet_32x16x48.npz (the reference's own net in
float64) at 1e-10, the up-sampling to F.interpolate and the gradient formulas to autograd.
"""
import torch
import torch.nn.functional as F

F64 = torch.float64
EPS, MOMENTUM = 1e-5, 0.1
# the kernel tests keep every theta + phi this many fp32 ulps (of the larger operand) away from the ReLU kink, so that the
# fp32 sum and the float64 sum fall on the same side (tests/norm_oracle.py: KINK_ULPS)
KINK_ULPS = 64


def is_param(name):
    return not (name.endswith("running_mean") or name.endswith("running_var") or name.endswith("num_batches_tracked"))


# ------------------------------------------------------------------------------------------------ up-sampling
def up_matrix(n, s, dtype=F64):
    """[s n, n]: row o holds the weights with which output o reads the n input cells (align_corners=False: source coordinate
    (o + 0.5) / s - 0.5 clamped below at 0, the upper neighbour clamped at n - 1)."""
    m = torch.zeros(s * n, n, dtype=dtype)
    for o in range(s * n):
        src = max((o + 0.5) / s - 0.5, 0.0)
        i0 = min(int(src), n - 1)
        i1 = min(i0 + 1, n - 1)
        l1 = src - i0
        m[o, i0] += 1.0 - l1
        m[o, i1] += l1
    return m


def upsample_int(x, s):
    """[N, K, d, h, w] -> [N, K, s d, s h, s w]"""
    mz, my, mx = (up_matrix(n, s, x.dtype) for n in x.shape[2:])
    return torch.einsum("zd,yh,xw,nkdhw->nkzyx", mz, my, mx, x)


def upsample_int_adjoint(b, s):
    """[N, K, s d, s h, s w] -> [N, K, d, h, w]: the transpose of upsample_int"""
    mz, my, mx = (up_matrix(n // s, s, b.dtype) for n in b.shape[2:])
    return torch.einsum("zd,yh,xw,nkzyx->nkdhw", mz, my, mx, b)


# ------------------------------------------------------------------------------------------------ the gate
def gate_map(theta, phi, psi_w, psi_b):
    """theta, phi [N, G Ci, d, h, w]; psi_w [G, Ci]; psi_b [G] -> att [N, G, d, h, w]"""
    G, Ci = psi_w.shape
    f = torch.relu(theta + phi).reshape(theta.shape[0], G, Ci, *theta.shape[2:])
    return torch.sigmoid((f * psi_w.reshape(1, G, Ci, 1, 1, 1)).sum(2) + psi_b.reshape(1, G, 1, 1, 1))


def gate_apply(x, att):
    """x [N, C, 2d, 2h, 2w]; att [N, G, d, h, w] -> y [N, G C, ...], y[:, g C + c] = up2(att[:, g]) x[:, c]"""
    a = upsample_int(att, 2)
    return (a.unsqueeze(2) * x.unsqueeze(1)).reshape(x.shape[0], -1, *x.shape[2:])


def gate_apply_bwd(dy, x, att):
    """-> (dx, datt)"""
    N, C = x.shape[:2]
    G = att.shape[1]
    dy = dy.reshape(N, G, C, *x.shape[2:])
    dx = (upsample_int(att, 2).unsqueeze(2) * dy).sum(1)
    return dx, upsample_int_adjoint((dy * x.unsqueeze(1)).sum(2), 2)


def gate_map_bwd(datt, att, theta, phi, psi_w):
    """-> (df, dpsi_w, dpsi_b); df is the gradient at theta and at phi"""
    G, Ci = psi_w.shape
    N, sp = theta.shape[0], theta.shape[2:]
    dpre = datt * att * (1 - att)
    f = (theta + phi).reshape(N, G, Ci, *sp)
    df = psi_w.reshape(1, G, Ci, 1, 1, 1) * dpre.unsqueeze(2) * (f > 0)
    dw = (torch.relu(f) * dpre.unsqueeze(2)).sum((0, 3, 4, 5))
    return df.reshape(theta.shape), dw, dpre.sum((0, 2, 3, 4))


class reference32:
    """torch's own fp32 CPU operators on the same cases (inputs are converted to fp32)."""

    @staticmethod
    def _f(*ts):
        return [torch.as_tensor(t).float() for t in ts]

    @staticmethod
    def upsample_int(x, s):
        return F.interpolate(torch.as_tensor(x).float(), scale_factor=s, mode="trilinear", align_corners=False)

    @staticmethod
    def upsample_int_adjoint(b, s):
        b = torch.as_tensor(b).float()
        x = torch.zeros(b.shape[0], b.shape[1], *(n // s for n in b.shape[2:]), requires_grad=True)
        y = F.interpolate(x, scale_factor=s, mode="trilinear", align_corners=False)
        return torch.autograd.grad(y, x, b)[0]

    @staticmethod
    def gate_map(theta, phi, psi_w, psi_b):
        theta, phi, psi_w, psi_b = reference32._f(theta, phi, psi_w, psi_b)
        G, Ci = psi_w.shape
        f = F.relu(theta + phi)
        return torch.cat([torch.sigmoid(F.conv3d(f[:, g * Ci:(g + 1) * Ci], psi_w[g].reshape(1, Ci, 1, 1, 1), psi_b[g:g + 1]))
                          for g in range(G)], 1)

    @staticmethod
    def gate_apply(x, att):
        x, att = reference32._f(x, att)
        up = F.interpolate(att, size=x.shape[2:], mode="trilinear", align_corners=False)
        return torch.cat([up[:, g:g + 1].expand_as(x) * x for g in range(att.shape[1])], 1)

    @staticmethod
    def gate_apply_bwd(dy, x, att):
        dy, x, att = reference32._f(dy, x, att)
        x.requires_grad_(True)
        att.requires_grad_(True)
        return torch.autograd.grad(reference32.gate_apply(x, att), [x, att], dy)

    @staticmethod
    def gate_map_bwd(datt, att, theta, phi, psi_w):
        datt, theta, phi, psi_w = reference32._f(datt, theta, phi, psi_w)
        psi_b = torch.zeros(psi_w.shape[0])         # the gradients do not depend on the bias once att is given ...
        for t in (theta, psi_w, psi_b):
            t.requires_grad_(True)
        G, Ci = psi_w.shape
        f = F.relu(theta + phi)
        pre = torch.cat([F.conv3d(f[:, g * Ci:(g + 1) * Ci], psi_w[g].reshape(1, Ci, 1, 1, 1), psi_b[g:g + 1]) for g in range(G)], 1)
        a = torch.as_tensor(att).float()            # ... so the sigmoid's derivative is taken at the given maps
        return torch.autograd.grad(pre, [theta, psi_w, psi_b], datt * a * (1 - a))


# ------------------------------------------------------------------------------------------------ the net
def _inorm(x):
    mean = x.mean((2, 3, 4), keepdim=True)
    var = ((x - mean) ** 2).mean((2, 3, 4), keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS)


def _bn(x, p, prefix, train, after):
    g, b = p[f"{prefix}.weight"], p[f"{prefix}.bias"]
    sh = (1, -1, 1, 1, 1)
    if train:
        n = x.numel() // x.shape[1]
        mean = x.mean((0, 2, 3, 4))
        var = ((x - mean.reshape(sh)) ** 2).mean((0, 2, 3, 4))
        after[f"{prefix}.running_mean"] = (1 - MOMENTUM) * p[f"{prefix}.running_mean"] + MOMENTUM * mean.detach()
        after[f"{prefix}.running_var"] = (1 - MOMENTUM) * p[f"{prefix}.running_var"] + MOMENTUM * var.detach() * n / (n - 1)
        after[f"{prefix}.num_batches_tracked"] = p[f"{prefix}.num_batches_tracked"] + 1
    else:
        mean, var = p[f"{prefix}.running_mean"], p[f"{prefix}.running_var"]
    return (x - mean.reshape(sh)) / torch.sqrt(var.reshape(sh) + EPS) * g.reshape(sh) + b.reshape(sh)


def _unetconv(h, p, prefix):
    for sub in ("conv1", "conv2"):
        h = torch.relu(_inorm(F.conv3d(h, p[f"{prefix}.{sub}.0.weight"], p[f"{prefix}.{sub}.0.bias"], padding=1)))
    return h


def _attention(p, prefix, x, g, train, after):
    gates = [f"{prefix}.gate_block_{k}" for k in (1, 2)]
    theta = torch.cat([F.conv3d(x, p[f"{q}.theta.weight"], stride=2) for q in gates], 1)
    phi = torch.cat([F.conv3d(g, p[f"{q}.phi.weight"], p[f"{q}.phi.bias"]) for q in gates], 1)
    assert theta.shape == phi.shape          # the reference's F.upsample(phi_g, size=theta_x.size()[2:]) is an identity
    C = x.shape[1]
    att = gate_map(theta, phi, torch.stack([p[f"{q}.psi.weight"].reshape(C) for q in gates]),
                   torch.cat([p[f"{q}.psi.bias"] for q in gates]))
    y = gate_apply(x, att)
    wy = torch.cat([_bn(F.conv3d(y[:, k * C:(k + 1) * C], p[f"{q}.W.0.weight"], p[f"{q}.W.0.bias"]), p, f"{q}.W.1", train, after)
                    for k, q in enumerate(gates)], 1)
    h = F.conv3d(wy, p[f"{prefix}.combine_gates.0.weight"], p[f"{prefix}.combine_gates.0.bias"])
    return torch.relu(_bn(h, p, f"{prefix}.combine_gates.1", train, after))


def run(sd, x, dlogits=None, train=True, dtype=F64):
    """``sd``: {key: tensor / array} with the reference's keys; ``x`` [N, C, D, H, W] with D, H, W multiples of 16.
    Returns {"logits", "grads": {parameter: gradient} (with dlogits), "after": {running buffer: value} (train mode)}."""
    p = {}
    for k, v in sd.items():
        t = torch.as_tensor(v)
        p[k] = t.to(dtype).clone().requires_grad_(True) if is_param(k) else t.clone().to(dtype if t.is_floating_point() else t.dtype)
    after = {}
    h = torch.as_tensor(x).to(dtype)
    enc = []
    for name in ("conv1", "conv2", "conv3", "conv4"):
        h = _unetconv(h, p, name)
        enc.append(h)
        h = F.max_pool3d(h, 2)
    center = _unetconv(h, p, "center")
    g = torch.relu(_inorm(F.conv3d(center, p["gating.conv1.0.weight"], p["gating.conv1.0.bias"])))
    h, heads = center, []
    for lvl in (4, 3, 2, 1):
        skip = enc[lvl - 1] if lvl == 1 else _attention(p, f"attentionblock{lvl}", enc[lvl - 1], g, train, after)
        h = g = _unetconv(torch.cat([skip, upsample_int(h, 2)], 1), p, f"up_concat{lvl}.conv")
        if lvl > 1:
            heads.append(upsample_int(F.conv3d(h, p[f"dsv{lvl}.dsv.0.weight"], p[f"dsv{lvl}.dsv.0.bias"]), 1 << (lvl - 1)))
        else:
            heads.append(F.conv3d(h, p["dsv1.weight"], p["dsv1.bias"]))
    logits = F.conv3d(torch.cat(heads[::-1], 1), p["final.weight"], p["final.bias"])
    res = {"logits": logits.detach(), "after": after}
    if dlogits is not None:
        names = [k for k in p if is_param(k)]
        grads = torch.autograd.grad(logits, [p[k] for k in names], torch.as_tensor(dlogits).to(dtype))
        res["grads"] = dict(zip(names, grads))
    return res
