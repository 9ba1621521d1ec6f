"""The case matrix of tests/test_attention_gate_gpu.py: seeded inputs, the float64 oracle's outputs
(tests/attention_unet_oracle.py) and e32 -- torch's own fp32 CPU operators against float64 -- per output tensor.  CPU only;
tests/test_attention_unet_cpu.py recomputes the GPU test's FLOOR constants from it.

Inputs: theta and phi are multiples of 1/64 in (-4, 4) whose sum is never zero, so every theta + phi is exact in fp32 and at
least MARGIN = 1/64 (2^16 fp32 ulps of 4) from the ReLU kink; psi weights are scaled by 1 / sqrt(Ci), and every case asserts
its psi pre-activations within +-8.  Attention maps are drawn from (0.05, 0.95), everything else is standard normal.
"""
import itertools

import torch

import attention_unet_oracle as ao

F64 = torch.float64
MARGIN = 1.0 / 64
PRE_MAX = 8.0
N, G = 2, 2
MAP_CASES = [(ci, grid) for ci in (1, 3, 32, 128) for grid in ((1, 1, 1), (2, 1, 3), (3, 5, 7))] + [(4, (24, 24, 24))]
APPLY_CASES = [(c, grid) for c in (1, 5, 32) for grid in ((1, 1, 1), (2, 1, 3), (3, 5, 8))]     # fine W = 2, 6: scalar; 16: float4
UP_CASES = list(itertools.product((2, 4, 8), (2, 4), ((1, 1, 1), (2, 1, 3), (4, 2, 6))))
# the kind of quantity of every output (one FLOOR each): attention maps, gated / up-sampled activations, data gradients,
# parameter sums, and the up-sampling adjoint (a sum over up to 16^3 outputs per cell: a scale of its own)
KIND_OF = {"att": "att", "y": "act", "dx": "dx", "datt": "dx", "df": "dx", "dpsi_w": "sum", "dpsi_b": "sum", "dphi_b": "sum", "up": "act",
           "upT": "upT"}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rel(a, b):
    """max |a - b| / max |b|"""
    return float((a.double() - b).abs().max() / b.abs().max())


def map_case(ci, grid):
    g = _gen(1000 + 17 * ci + sum(grid))
    sh = (N, G * ci) + tuple(grid)
    theta = torch.randint(-255, 256, sh, generator=g).to(F64) / 64
    phi = torch.randint(-255, 256, sh, generator=g).to(F64) / 64
    phi = torch.where(theta + phi == 0, phi + MARGIN, phi)
    assert float((theta + phi).abs().min()) >= MARGIN
    psi_w = torch.randn((G, ci), generator=g, dtype=F64) / (2.0 * ci ** 0.5)
    psi_b = torch.randn((G,), generator=g, dtype=F64) / 2
    datt = torch.randn((N, G) + tuple(grid), generator=g, dtype=F64)
    # what the parameter gradients hold before an accumulating call
    base = dict(dw0=torch.randn((G, ci), generator=g, dtype=F64), db0=torch.randn((G,), generator=g, dtype=F64),
                dp0=torch.randn((G * ci,), generator=g, dtype=F64))
    pre = (torch.relu(theta + phi).reshape(N, G, ci, *grid) * psi_w.reshape(1, G, ci, 1, 1, 1)).sum(2) + psi_b.reshape(1, G, 1, 1, 1)
    assert float(pre.abs().max()) <= PRE_MAX, float(pre.abs().max())
    att = ao.gate_map(theta, phi, psi_w, psi_b)
    df, dw, db = ao.gate_map_bwd(datt, att, theta, phi, psi_w)
    a32 = ao.reference32.gate_map(theta, phi, psi_w, psi_b)
    # the backward's e32 from the float64 maps rounded to fp32: what the kernel is given
    df32, dw32, db32 = ao.reference32.gate_map_bwd(datt, att, theta, phi, psi_w)
    dphi = df.sum((0, 2, 3, 4))           # the bias gradient of the phi convolution, whose output gradient df is
    return {"in": dict(theta=theta, phi=phi, psi_w=psi_w, psi_b=psi_b, datt=datt, **base), "att": att, "df": df, "dpsi_w": dw, "dpsi_b": db,
            "dphi_b": dphi,
            "e32": {"att": rel(a32, att), "df": rel(df32, df), "dpsi_w": rel(dw32, dw), "dpsi_b": rel(db32, db),
                    "dphi_b": rel(df32.sum((0, 2, 3, 4)), dphi)}}


def apply_case(c, grid):
    g = _gen(2000 + 31 * c + sum(grid))
    fine = tuple(2 * n for n in grid)
    x = torch.randn((N, c) + fine, generator=g, dtype=F64)
    att = 0.05 + 0.9 * torch.rand((N, G) + tuple(grid), generator=g, dtype=F64)
    dy = torch.randn((N, G * c) + fine, generator=g, dtype=F64)
    dx0 = torch.randn((N, c) + fine, generator=g, dtype=F64)          # what dx holds before an accumulating call
    y = ao.gate_apply(x, att)
    dx, datt = ao.gate_apply_bwd(dy, x, att)
    y32 = ao.reference32.gate_apply(x, att)
    dx32, datt32 = ao.reference32.gate_apply_bwd(dy, x, att)
    return {"in": dict(x=x, att=att, dy=dy, dx0=dx0), "y": y, "dx": dx, "datt": datt,
            "e32": {"y": rel(y32, y), "dx": rel(dx32, dx), "datt": rel(datt32, datt)}}


def up_case(s, k, grid):
    g = _gen(3000 + 7 * s + k + sum(grid))
    fine = tuple(s * n for n in grid)
    x = torch.randn((N, k) + tuple(grid), generator=g, dtype=F64)
    dy = torch.randn((N, k) + fine, generator=g, dtype=F64)
    dx0 = torch.randn((N, k) + tuple(grid), generator=g, dtype=F64)
    up, upT = ao.upsample_int(x, s), ao.upsample_int_adjoint(dy, s)
    return {"in": dict(x=x, dy=dy, dx0=dx0), "up": up, "upT": upT,
            "e32": {"up": rel(ao.reference32.upsample_int(x, s), up), "upT": rel(ao.reference32.upsample_int_adjoint(dy, s), upT)}}


def all_cases():
    """(label, case) over the whole matrix"""
    for ci, grid in MAP_CASES:
        yield f"map-Ci{ci}-{'x'.join(map(str, grid))}", map_case(ci, grid)
    for c, grid in APPLY_CASES:
        yield f"apply-C{c}-{'x'.join(map(str, grid))}", apply_case(c, grid)
    for s, k, grid in UP_CASES:
        yield f"up{s}-K{k}-{'x'.join(map(str, grid))}", up_case(s, k, grid)


def floors():
    """{kind: (largest e32 of the matrix, label, output)}"""
    worst = {}
    for label, c in all_cases():
        for out, e in c["e32"].items():
            if e > worst.get(KIND_OF[out], (-1.0,))[0]:
                worst[KIND_OF[out]] = (e, label, out)
    return worst
