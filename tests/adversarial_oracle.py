"""float64 reference of the adversarial kernels (csrc/adversarial.hip) and the case matrix of
tests/test_adversarial_kernels_gpu.py.  CPU only, plain torch, built on tests/conv_oracle.py (input classes, measures) and
tests/loss_tail_oracle.py (CE + Dice).

  Convolution  nn.Conv3d(k = 4, s = 2, p = 1): reference64 / reference32 through F.conv3d and autograd; plain64 the same as a
               sum over the 64 taps of strided slices, einsum over the channels -- no convolution operator.  e32 = the
               distance of reference32 (one thread) to reference64: the yardstick of  err_hip <= max(K e32, FLOOR[kind]).
  Epilogue     act_drop: leaky_relu(pre, slope) * scale[n, c]; ``signs`` replaces the activation's own decision pre > 0 by a
               given one (the float64-arbiter rule: a chain is compared with the oracle evaluated on the decisions the
               kernels took; decided_share says how many pre-activations lie outside the margin inside which fp32 and
               float64 may decide differently).
  Discriminator  FC3DDiscriminator (reference code/networks/discriminator.py:6-55) as a function of a state_dict:
               disc_forward, disc_step (loss, logits, parameter gradients, gradient at the ``map`` input).
  Head, tail, Adam   head, tail (train_adversarial_network_3D.py:137-150), adam (torch.optim.Adam in float64).
  Golden inputs      golden_inputs / golden_state_dict: closed-form functions of the index that both
               scripts/gen_golden_adversarial.py and the tests evaluate; the fixture stores results only.
"""
import functools
import math

import torch
import torch.nn.functional as F

import conv_oracle as co
import loss_tail_oracle as lto
import oracle_kit as kit

F64, F32 = torch.float64, torch.float32
KINDS, MEASURES = co.KINDS, co.MEASURES
K = 6.0
SLOPE = 0.2
MARGIN = 1e-4          # a decision counts where |pre| exceeds this share of its channel's largest |pre|
UNDECIDED_CAP = 1e-3   # at most this share of the elements may lie inside the margin
# the largest e32 of the matrix per kind (either measure), rounded up to two digits; tests/test_adversarial_cpu.py recomputes it
FLOOR = {"y": 2.1e-6,       # 2.04e-6 (sliced/uniform, max: a contraction over 16384 products)
         "dx": 1.5e-6,      # 1.45e-6 (sliced/offset, max)
         "dw": 7.1e-7}      # 7.09e-7 (wide-n3/offset, max)

ALL = co.X_CLASSES
ONE = ("relu_scaled",)
SPECS = {}


def _spec(cid, shape, classes=ONE, layout="dense"):
    """shape = (N, Cin, Cout, D, H, W) of the INPUT."""
    SPECS[cid] = dict(group="k4s2", op="down", shape=shape, k=(4, 4, 4), classes=classes, kinds=KINDS, layout=layout)


_spec("all-padding", (1, 1, 4, 2, 2, 2), ALL)            # one output voxel: every window touches the padding on both sides
_spec("all-padding-n3", (3, 5, 20, 2, 2, 2))
_spec("ragged", (3, 3, 8, 4, 6, 10), ALL)                # 30 output voxels: a ragged column tile that crosses samples
_spec("thin", (1, 5, 20, 2, 12, 4))                      # Do = 1, Cout over one 16-row tile
_spec("cube-1-4", (3, 1, 4, 12, 12, 12))                 # 648 columns: more than one workgroup, the 16-row tiles
_spec("cube-3-8", (1, 3, 8, 12, 12, 12), ALL)
_spec("cube-5-20", (3, 5, 20, 12, 12, 12))               # 64-row tiles with 44 dead rows
_spec("wide", (1, 64, 128, 12, 12, 12))                  # two row blocks, 64 chunks of the contraction
_spec("wide-n3", (3, 64, 128, 4, 6, 10), ALL)
_spec("sliced", (1, 256, 512, 4, 4, 4), ALL)             # 8 columns, K = 16384: the contraction is cut into slices
_spec("sliced-n3", (3, 256, 512, 4, 4, 4))
_spec("views", (3, 3, 8, 4, 6, 10), layout="slice")      # every operand a channel slice of a wider buffer
_spec("views-wide", (1, 64, 128, 2, 12, 4), layout="slice")


def names():
    return [f"{cid}/{cls}" for cid, s in SPECS.items() for cls in s["classes"]]


@functools.lru_cache(maxsize=None)
def case(name):
    cid, cls = name.split("/")
    return co.make_case(cid, SPECS[cid], cls)


def conv(x, w, b=None):
    return F.conv3d(x, w, b, stride=2, padding=1)


def reference_torch(c, dtype):
    x = c["x"].to(dtype, copy=True).requires_grad_(True)
    w = c["w"].to(dtype, copy=True).requires_grad_(True)
    y = conv(x, w, c["b"].to(dtype))
    y.backward(c["dy"].to(dtype))
    return {"y": y.detach().double(), "dx": x.grad.double(), "dw": w.grad.double()}


def reference64(c):
    return reference_torch(c, F64)


def reference32(c):
    return kit.one_thread(reference_torch, c, F32)


def plain64(c):
    """y, dx, dw in float64 as sums over the 64 taps: tap (a, e, d) reads the padded input at 2 o + (a, e, d)."""
    x, w, b, dy = c["x"].double(), c["w"].double(), c["b"].double(), c["dy"].double()
    N, _, D, H, W = x.shape
    y = b.reshape(1, -1, 1, 1, 1).expand(N, -1, D // 2, H // 2, W // 2).clone()
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    dxp, dw = torch.zeros_like(xp), torch.zeros_like(w)
    for a in range(4):
        for e in range(4):
            for d in range(4):
                sl = (slice(None), slice(None), slice(a, a + D, 2), slice(e, e + H, 2), slice(d, d + W, 2))
                y += torch.einsum("oc,ncdhw->nodhw", w[:, :, a, e, d], xp[sl])
                dw[:, :, a, e, d] = torch.einsum("nodhw,ncdhw->oc", dy, xp[sl])
                dxp[sl] += torch.einsum("oc,nodhw->ncdhw", w[:, :, a, e, d], dy)
    return {"y": y, "dx": dxp[:, :, 1:-1, 1:-1, 1:-1], "dw": dw}


@functools.lru_cache(maxsize=None)
def references(name):
    """(float64 reference, reference32, e32 = {kind: {measure: value}}) of a matrix case.  Computed once, never modified."""
    c = case(name)
    r64, r32 = reference64(c), reference32(c)
    return r64, r32, {k: co.measure(r32[k], r64[k], co.dim_of(c, k)) for k in KINDS}


# ---------------------------------------------------------------------------------------------------------------------
# activation + channel dropout
# ---------------------------------------------------------------------------------------------------------------------
def act_drop(pre, slope=SLOPE, scale=None, signs=None):
    """leaky_relu(pre, slope) * scale[n, c]; ``signs`` (bool, pre's shape): the decisions to use instead of pre > 0."""
    pos = (pre > 0) if signs is None else signs
    a = torch.where(pos, pre, pre * slope)
    if scale is not None:
        a = a * scale.to(pre.dtype).reshape(scale.shape[0], scale.shape[1], *([1] * (pre.dim() - 2)))
    return a


def decided(pre64):
    """bool, pre's shape: |pre| exceeds MARGIN of its channel's largest |pre| (channel = dim 1, over batch and space)."""
    other = [d for d in range(pre64.dim()) if d != 1]
    return pre64.abs() > MARGIN * pre64.abs().amax(other, keepdim=True)


def undecided_share(pre64):
    return 1.0 - decided(pre64).double().mean().item()


# ---------------------------------------------------------------------------------------------------------------------
# the discriminator
# ---------------------------------------------------------------------------------------------------------------------
DISC_KEYS = ("conv0.weight", "conv0.bias", "conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight",
             "conv3.bias", "conv4.weight", "conv4.bias", "classifier.weight", "classifier.bias")


def disc_shapes(num_classes, ndf=64, n_channel=1):
    """The reference's twelve state_dict entries, in its order."""
    k = (4, 4, 4)
    return {"conv0.weight": (ndf, num_classes) + k, "conv0.bias": (ndf,), "conv1.weight": (ndf, n_channel) + k,
            "conv1.bias": (ndf,), "conv2.weight": (2 * ndf, ndf) + k, "conv2.bias": (2 * ndf,),
            "conv3.weight": (4 * ndf, 2 * ndf) + k, "conv3.bias": (4 * ndf,), "conv4.weight": (8 * ndf, 4 * ndf) + k,
            "conv4.bias": (8 * ndf,), "classifier.weight": (2, 8 * ndf), "classifier.bias": (2,)}


def disc_forward(sd, probs, image, masks=None, pool=(6, 6, 6), slope=SLOPE, signs=None, conv_fn=conv):
    """FC3DDiscriminator.forward(map = probs, image) with the parameters ``sd``.  masks: three [N, C] dropout scale arrays
    (None: eval mode); signs: four bool tensors, the activation decisions to use.  Returns (logits, [a0, a2, a3, a4] the stored
    activated outputs, [pre0, pre2, pre3, pre4])."""
    acts, pres = [], []
    pre = conv_fn(probs, sd["conv0.weight"], sd["conv0.bias"]) + conv_fn(image, sd["conv1.weight"], sd["conv1.bias"])
    for i, key in enumerate((None, "conv2", "conv3", "conv4")):
        if key is not None:
            pre = conv_fn(acts[-1], sd[key + ".weight"], sd[key + ".bias"])
        pres.append(pre)
        scale = masks[i] if (masks is not None and i < 3) else None
        acts.append(act_drop(pre, slope, scale, None if signs is None else signs[i]))
    a4 = acts[-1]
    assert tuple(a4.shape[2:]) == tuple(pool), (tuple(a4.shape), pool)
    pooled = a4.mean((2, 3, 4))
    return pooled @ sd["classifier.weight"].t() + sd["classifier.bias"], acts, pres


def disc_step(sd, probs, image, target, masks=None, pool=(6, 6, 6), signs=None, dtype=F64):
    """One forward + backward of cross_entropy(D(probs, image), target): dict(loss, logits, grads {key: tensor}, dmap = the
    gradient at probs, acts, pres)."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    m = probs.detach().to(dtype).clone().requires_grad_(True)
    logits, acts, pres = disc_forward(p, m, image.to(dtype), masks, pool, signs=signs)
    loss = F.cross_entropy(logits, target.long())
    loss.backward()
    return dict(loss=loss.detach(), logits=logits.detach(), grads={k: v.grad for k, v in p.items()}, dmap=m.grad,
                acts=[a.detach() for a in acts], pres=[a.detach() for a in pres])


def head(a, w, b, target, dtype=F64):
    """AvgPool over the whole feature -> Linear -> cross_entropy: dict(loss, logits, da, dw, db)."""
    a = a.detach().to(dtype).clone().requires_grad_(True)
    w = w.detach().to(dtype).clone().requires_grad_(True)
    b = b.detach().to(dtype).clone().requires_grad_(True)
    logits = a.mean((2, 3, 4)) @ w.t() + b
    loss = F.cross_entropy(logits, target.long())
    loss.backward()
    return dict(loss=loss.detach(), logits=logits.detach(), da=a.grad, dw=w.grad, db=b.grad)


def tail(logits, label, L, dmap, cons_loss, w, loss_scale=1.0, dtype=F64):
    """out = [loss, ce, dice, consistency, w, C class-wise dice] and dlogits of
    0.5 * (CE + Dice)(logits[:L], label) + w * cons_loss, where cons_loss is a function of softmax(logits[L:]) whose
    gradient there is dmap: the unlabeled samples receive w * (softmax Jacobian)^T dmap."""
    s = logits.detach().to(dtype).clone().requires_grad_(True)
    B, C = s.shape[:2]
    ce, dice, scores = lto._supervised(s, label, L, C)
    sup = 0.5 * (ce + dice)
    proxy = sup + (w * (torch.softmax(s[L:], 1) * dmap.to(dtype)).sum() if B > L else 0.0)
    (g,) = torch.autograd.grad(proxy * loss_scale, [s])
    cons = float(cons_loss) if B > L else 0.0
    return lto._out(sup.detach() + w * cons, ce, dice, cons, w, scores), g


def adam(p0, grads, lr, betas=(0.9, 0.99), eps=1e-8, dtype=F64, first_step=1):
    """The parameter after each of the steps with gradients ``grads`` (a list), torch.optim.Adam; first_step > 1 starts from a
    state whose step count is first_step - 1 with zero moments (what mis_adam_init leaves)."""
    p = p0.detach().to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    if first_step > 1:
        opt.state[p] = dict(step=torch.tensor(float(first_step - 1)), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
    out = []
    for g in grads:
        p.grad = g.detach().to(dtype).clone()
        opt.step()
        out.append(p.detach().clone())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# closed-form inputs of the golden iteration
# ---------------------------------------------------------------------------------------------------------------------
def _grid(shape):
    return torch.meshgrid(*[torch.arange(s, dtype=F64) for s in shape], indexing="ij")


def golden_inputs(B=4, C=2, size=96):
    """volume [B, 1, size^3], the student's logits [B, C, size^3] (both float32, functions of the index) and labels
    [B, size^3] uint8."""
    n, d, h, w = _grid((B, size, size, size))
    vol = torch.sin(0.37 * d + 0.23 * h - 0.11 * w + 1.3 * n) * torch.cos(0.05 * (d + h + w)) + 0.1 * n
    lg = [1.5 * torch.sin(0.19 * d - 0.31 * h + 0.07 * w + 0.9 * n + 2.1 * c) + 0.5 * torch.cos(0.13 * w * (c + 1) + 0.4 * d)
          for c in range(C)]
    lab = ((d // 8 + h // 12 + w // 16 + n) % C).to(torch.uint8)
    return vol.unsqueeze(1).float(), torch.stack(lg, 1).float(), lab


def golden_state_dict(num_classes=2, ndf=4, n_channel=1):
    """float32 parameters as a function of the index: amplitude 1.5 / sqrt(fan_in), a different frequency per entry."""
    sd = {}
    for i, (key, shape) in enumerate(disc_shapes(num_classes, ndf, n_channel).items()):
        n = math.prod(shape)
        fan_in = math.prod(shape[1:]) if len(shape) > 1 else 16
        idx = torch.arange(n, dtype=F64)
        sd[key] = (1.5 / math.sqrt(fan_in) * torch.sin(idx * (0.7 + 0.13 * i) + 0.3 * i)).reshape(shape).float()
    return sd


def golden_masks(ndf=4, N=4):
    """The three Dropout3d scale arrays [N, C] of phase B: 0 or 2, a fixed pattern with both values in every sample."""
    out = []
    for i, C in enumerate((ndf, 2 * ndf, 4 * ndf)):
        n, c = _grid((N, C))
        out.append((((n * 3 + c * 5 + i) % 7) % 2 == 0).double() * 2.0)
    return out


GOLDEN_LATTICE = 12     # the map gradient is stored at every 12th voxel per axis, offset 5


def lattice(t):
    return t[..., 5::GOLDEN_LATTICE, 5::GOLDEN_LATTICE, 5::GOLDEN_LATTICE]


# ---------------------------------------------------------------------------------------------------------------------
# the gate of the adversarial GPU tests (3-D kernels, 2-D kernels, the golden iteration)
# ---------------------------------------------------------------------------------------------------------------------
STATS = []        # every figure of the 3-D tests: (case, label, kind, measure, e32, hip)


class Check:
    """The gate on one tensor: got against ref64, e32 from the fp32 evaluation r32 of the same expression."""

    def __init__(self, name, floor=FLOOR, stats=STATS, over_the_gate=None, width=14):
        self.name, self.width = name, width
        self.gate = kit.Gate(K, floor, over_the_gate, stats)

    def __call__(self, label, kind, got, ref, r32, dim=1):
        ref = ref.detach().double()
        got, r32 = got.detach().cpu().double().reshape(ref.shape), r32.detach().double().reshape(ref.shape)
        if ref.dim() < 2:
            got, ref, r32, dim = got.reshape(1, -1), ref.reshape(1, -1), r32.reshape(1, -1), 0
        e = co.measure(r32, ref, dim)
        self.gate.tensor(self.name, label, kind, got, ref, lambda g, r: co.measure(g, r, dim), {ms: e[ms] for ms in co.MEASURES},
                         (self.name,), width=self.width)

    def done(self):
        self.gate.done(self.name)


def print_report(prefix, stats, floor, width=14):
    """Worst ratio per (group, tensor, measure) of the rows a test file collected."""
    for (group, label, m), r in kit.worst_rows(((cid.split(":")[0] if ":" in cid else "conv", label, m), cid, e32, ehip,
                                                max(e32, floor[kind] / K)) for cid, label, kind, m, e32, ehip in stats):
        print(f"\n[{prefix}] {group:8s} {label:{width}s} {m:3s} e32 {r['lo']:.1e} .. {r['hi']:.1e}  hip max {r['hip']:.2e}  "
              f"worst hip/max(e32, floor/K) {r['ratio']:.2f} ({r['at']})", end="")
    print()
