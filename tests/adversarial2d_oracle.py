"""float64 reference of the 2-D adversarial kernels (csrc/adversarial2d.hip) and the case matrix of
tests/test_adversarial2d_kernels_gpu.py.  CPU only, plain torch.  What is dimension-free comes from
tests/adversarial_oracle.py (act_drop, decided, undecided_share, tail, adam, K, MARGIN, UNDECIDED_CAP).

  Convolution  nn.Conv2d(k = 4, s = 2, p = 1): reference64 / reference32 through F.conv2d and autograd; plain64 the same as a
               sum over the 16 taps of strided slices, einsum over the channels -- no convolution operator.  e32 = the
               distance of reference32 (one thread) to reference64: the yardstick of  err_hip <= max(K e32, FLOOR[kind]).
  Discriminator  FCDiscriminator (reference code/networks/discriminator.py:58-100) as a function of a state_dict, in the
               reference's 2-D order: no activation and no dropout after conv0 + conv1, LeakyReLU(0.2) after conv2, conv3,
               conv4, Dropout2d after conv2 and conv3, AvgPool2d(pool) in floor mode, flatten, Linear(32 ndf, 2).
  Head         head2d: AvgPool2d(pool) -> flatten -> Linear -> cross_entropy.
  Inputs       golden_inputs / golden_state_dict / golden_masks: closed-form functions of the index that both
               scripts/gen_golden_adversarial2d.py and the tests evaluate; chain_params: the chain tests' parameters under
               torch's default uniform law (seeded) or the sine pattern.
"""
import functools
import math

import torch
import torch.nn.functional as F

import conv_oracle as co
from oracle_kit import one_thread          # noqa: F401  (re-exported: the tests evaluate their fp32 forms under it)
from adversarial_oracle import K, MARGIN, Check, print_report, UNDECIDED_CAP, SLOPE, act_drop, adam, decided, tail, undecided_share  # noqa: F401

F64, F32 = torch.float64, torch.float32
KINDS, MEASURES = co.KINDS, co.MEASURES
# the largest e32 of the matrix per kind (either measure), rounded up to two digits; tests/test_adversarial2d_cpu.py recomputes it
FLOOR = {"y": 1.4e-6,       # 1.39e-6 (c20-64/offset, max)
         "dx": 8.5e-7,      # 8.42e-7 (views-wide/relu_scaled, max)
         "dw": 1.2e-6}      # 1.16e-6 (c20-64/offset, max)

ALL = co.X_CLASSES
ONE = ("relu_scaled",)
SPECS = {}


def _spec(cid, shape, classes=ONE, layout="dense"):
    """shape = (N, Cin, Cout, H, W) of the INPUT."""
    SPECS[cid] = dict(shape=shape, classes=classes, layout=layout)


_spec("all-padding", (1, 1, 4, 2, 2), ALL)               # one output pixel: all taps but four lie in the padding
_spec("all-padding-n3", (3, 5, 20, 2, 2))
_spec("row", (3, 5, 20, 2, 12))                          # 2 x W: one output row
_spec("col", (3, 3, 8, 10, 2))                           # H x 2: one output column
_spec("c1-1", (3, 1, 1, 8, 8))                           # one channel in, one out; 16-byte rows on both sides
_spec("ragged-20x12", (3, 3, 17, 20, 12), ALL)           # 10 x 6 outputs: no multiple of a tile side; Cout over one MFMA tile
_spec("ragged-6x70", (1, 5, 4, 6, 70))                   # 35 output columns: three column tiles, rows of no 16-byte multiple
_spec("c20-64", (3, 20, 64, 20, 12), ALL)                # five channel chunks, a full 64-row block
_spec("tiles-vec", (1, 4, 8, 40, 72))                    # 20 x 36 outputs: 3 x 3 tiles, 16-byte row segments throughout
_spec("wide", (1, 64, 128, 12, 12))                      # two blocks of output channels, 16 chunks of the contraction
_spec("sliced", (2, 256, 64, 8, 8), ALL)                 # 4 x 4 outputs, K = 4096: the forward's contraction is cut into slices
_spec("views", (3, 3, 8, 6, 10), layout="slice")         # every operand a channel slice of a wider buffer
_spec("views-wide", (1, 64, 128, 12, 8), layout="slice")


def names():
    return [f"{cid}/{cls}" for cid, s in SPECS.items() for cls in s["classes"]]


@functools.lru_cache(maxsize=None)
def case(name):
    """x [N, Cin, H, W], dy [N, Cout, H/2, W/2], w [Cout, Cin, 4, 4], b [Cout]: conv_oracle's input classes, float32."""
    cid, cls = name.split("/")
    s = SPECS[cid]
    N, Cin, Cout, H, W = s["shape"]
    g = co._gen(f"adv2d/{cid}/{cls}")
    x = co.make_x(cls, (N, Cin, 1, H, W), g)[:, :, 0]
    dy = co.make_x(co.DY_OF[cls], (N, Cout, 1, H // 2, W // 2), g)[:, :, 0]
    w = (torch.rand((Cout, Cin, 4, 4), generator=g, dtype=F64) * 2 - 1) * 0.2
    b = torch.rand(Cout, generator=g, dtype=F64) * 2 - 1
    return dict(s, id=cid, xcls=cls, x=x.float().contiguous(), dy=dy.float().contiguous(), w=w.float(), b=b.float())


def conv(x, w, b=None):
    return F.conv2d(x, w, b, stride=2, padding=1)


def conv_taps(x, w, b=None):
    """conv as a sum over the 16 taps of strided slices of the padded input: no convolution operator (autograd works)."""
    N, _, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    y = 0.0
    for a in range(4):
        for e in range(4):
            y = y + torch.einsum("oc,nchw->nohw", w[:, :, a, e], xp[:, :, a:a + H:2, e:e + W:2])
    return y if b is None else y + b.reshape(1, -1, 1, 1)


def reference_torch(c, dtype, conv_fn=conv):
    x = c["x"].to(dtype, copy=True).requires_grad_(True)
    w = c["w"].to(dtype, copy=True).requires_grad_(True)
    y = conv_fn(x, w, c["b"].to(dtype))
    y.backward(c["dy"].to(dtype))
    return {"y": y.detach().double(), "dx": x.grad.double(), "dw": w.grad.double()}


def reference64(c):
    return reference_torch(c, F64)


def reference32(c):
    return one_thread(lambda: reference_torch(c, F32))


def plain64(c):
    """y, dx, dw in float64 as explicit sums over the 16 taps (forward and both gradients written out, no autograd)."""
    x, w, b, dy = c["x"].double(), c["w"].double(), c["b"].double(), c["dy"].double()
    N, _, H, W = x.shape
    y = b.reshape(1, -1, 1, 1).expand(N, -1, H // 2, W // 2).clone()
    xp = F.pad(x, (1, 1, 1, 1))
    dxp, dw = torch.zeros_like(xp), torch.zeros_like(w)
    for a in range(4):
        for e in range(4):
            sl = (slice(None), slice(None), slice(a, a + H, 2), slice(e, e + W, 2))
            y += torch.einsum("oc,nchw->nohw", w[:, :, a, e], xp[sl])
            dw[:, :, a, e] = torch.einsum("nohw,nchw->oc", dy, xp[sl])
            dxp[sl] += torch.einsum("oc,nohw->nchw", w[:, :, a, e], dy)
    return {"y": y, "dx": dxp[:, :, 1:-1, 1:-1], "dw": dw}


def dim_of(kind):
    return 0 if kind == "dw" else 1


@functools.lru_cache(maxsize=None)
def references(name):
    """(float64 reference, reference32, e32 = {kind: {measure: value}}) of a matrix case.  Computed once, never modified."""
    c = case(name)
    r64, r32 = reference64(c), reference32(c)
    return r64, r32, {k: co.measure(r32[k], r64[k], dim_of(k)) for k in KINDS}


# ---------------------------------------------------------------------------------------------------------------------
# the discriminator
# ---------------------------------------------------------------------------------------------------------------------
DISC_KEYS = ("conv0.weight", "conv0.bias", "conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight",
             "conv3.bias", "conv4.weight", "conv4.bias", "classifier.weight", "classifier.bias")
# (slope, dropout) after conv0 + conv1, conv2, conv3, conv4
LAYER_ACT = ((1.0, False), (SLOPE, True), (SLOPE, True), (SLOPE, False))
ACTIVATED = (1, 2, 3)       # the layers whose stored output carries a decision


def disc_shapes(num_classes, ndf=64, n_channel=1):
    """The reference's twelve state_dict entries, in its order."""
    k = (4, 4)
    return {"conv0.weight": (ndf, num_classes) + k, "conv0.bias": (ndf,), "conv1.weight": (ndf, n_channel) + k,
            "conv1.bias": (ndf,), "conv2.weight": (2 * ndf, ndf) + k, "conv2.bias": (2 * ndf,),
            "conv3.weight": (4 * ndf, 2 * ndf) + k, "conv3.bias": (4 * ndf,), "conv4.weight": (8 * ndf, 4 * ndf) + k,
            "conv4.bias": (8 * ndf,), "classifier.weight": (2, 32 * ndf), "classifier.bias": (2,)}


def pool_flatten(a, pool):
    """AvgPool2d(pool) (stride = window, floor mode) and the flatten, by reshaping: no pooling operator."""
    N, C, H, W = a.shape
    nh, nw = H // pool[0], W // pool[1]
    a = a[:, :, :nh * pool[0], :nw * pool[1]].reshape(N, C, nh, pool[0], nw, pool[1])
    return a.mean((3, 5)).reshape(N, C * nh * nw)


def disc_forward(sd, probs, image, masks=None, pool=(7, 7), signs=None, conv_fn=conv):
    """FCDiscriminator.forward(map = probs, feature = image) with the parameters ``sd``.  masks: two [N, C] dropout scale arrays,
    after conv2 and conv3 (None: eval mode); signs: {layer index: bool tensor}, the activation decisions to use.  Returns
    (logits, [a0, a2, a3, a4] the stored outputs, [pre0, pre2, pre3, pre4])."""
    acts, pres = [], []
    pre = conv_fn(probs, sd["conv0.weight"], sd["conv0.bias"]) + conv_fn(image, sd["conv1.weight"], sd["conv1.bias"])
    for i, key in enumerate((None, "conv2", "conv3", "conv4")):
        if key is not None:
            pre = conv_fn(acts[-1], sd[key + ".weight"], sd[key + ".bias"])
        pres.append(pre)
        slope, drops = LAYER_ACT[i]
        scale = masks[i - 1] if (masks is not None and drops) else None
        acts.append(act_drop(pre, slope, scale, None if (signs is None or slope == 1.0) else signs[i]))
    return pool_flatten(acts[-1], pool) @ sd["classifier.weight"].t() + sd["classifier.bias"], acts, pres


def disc_step(sd, probs, image, target, masks=None, pool=(7, 7), signs=None, dtype=F64):
    """One forward + backward of cross_entropy(D(probs, image), target): dict(loss, logits, grads {key: tensor}, dmap = the
    gradient at probs, acts, pres)."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    m = probs.detach().to(dtype).clone().requires_grad_(True)
    logits, acts, pres = disc_forward(p, m, image.to(dtype), masks, pool, signs=signs)
    loss = F.cross_entropy(logits, target.long())
    loss.backward()
    return dict(loss=loss.detach(), logits=logits.detach(), grads={k: v.grad for k, v in p.items()}, dmap=m.grad,
                acts=[a.detach() for a in acts], pres=[a.detach() for a in pres])


def head2d(a, w, b, target, pool, dtype=F64):
    """AvgPool2d(pool) -> flatten -> Linear -> cross_entropy: dict(loss, logits, da, dw, db)."""
    a = a.detach().to(dtype).clone().requires_grad_(True)
    w = w.detach().to(dtype).clone().requires_grad_(True)
    b = b.detach().to(dtype).clone().requires_grad_(True)
    logits = pool_flatten(a, pool) @ w.t() + b
    loss = F.cross_entropy(logits, target.long())
    loss.backward()
    return dict(loss=loss.detach(), logits=logits.detach(), da=a.grad, dw=w.grad, db=b.grad)


# ---------------------------------------------------------------------------------------------------------------------
# closed-form inputs
# ---------------------------------------------------------------------------------------------------------------------
def _grid(shape):
    return torch.meshgrid(*[torch.arange(s, dtype=F64) for s in shape], indexing="ij")


def golden_inputs(B=4, C=4, H=256, W=224):
    """image [B, 1, H, W], the student's logits [B, C, H, W] (both float32, functions of the index) and labels [B, H, W] uint8."""
    n, h, w = _grid((B, H, W))
    img = torch.sin(0.23 * h - 0.11 * w + 1.3 * n) * torch.cos(0.05 * (h + w)) + 0.1 * n
    lg = [1.5 * torch.sin(-0.31 * h + 0.07 * w + 0.9 * n + 2.1 * c) + 0.5 * torch.cos(0.13 * w * (c + 1) + 0.4 * h)
          for c in range(C)]
    lab = ((h // 12 + w // 16 + n) % C).to(torch.uint8)
    return img.unsqueeze(1).float(), torch.stack(lg, 1).float(), lab


def golden_state_dict(num_classes=4, ndf=4, n_channel=1):
    """float32 parameters as a function of the index: amplitude 1.5 / sqrt(fan_in), a different frequency per entry."""
    sd = {}
    for i, (key, shape) in enumerate(disc_shapes(num_classes, ndf, n_channel).items()):
        n = math.prod(shape)
        fan_in = math.prod(shape[1:]) if len(shape) > 1 else 16
        idx = torch.arange(n, dtype=F64)
        sd[key] = (1.5 / math.sqrt(fan_in) * torch.sin(idx * (0.7 + 0.13 * i) + 0.3 * i)).reshape(shape).float()
    return sd


def uniform_state_dict(num_classes, ndf, n_channel=1, seed=0):
    """float32 parameters under torch's default law of Conv2d / Linear: U(+-1/sqrt(fan_in)) for weight and bias."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    shapes = disc_shapes(num_classes, ndf, n_channel)
    for key, shape in shapes.items():
        wshape = shapes[key.replace(".bias", ".weight")]
        bound = 1.0 / math.sqrt(math.prod(wshape[1:]))
        sd[key] = ((torch.rand(shape, generator=g, dtype=F64) * 2 - 1) * bound).float()
    return sd


def golden_masks(ndf=4, N=4):
    """The two Dropout2d scale arrays [N, C] (after conv2 and conv3): 0 or 2, a fixed pattern with both values in every sample."""
    out = []
    for i, C in enumerate((2 * ndf, 4 * ndf)):
        n, c = _grid((N, C))
        out.append((((n * 3 + c * 5 + i) % 7) % 2 == 0).double() * 2.0)
    return out


# The chains of tests/test_adversarial2d_kernels_gpu.py: (ndf, H, W, pool, N, parameter law, seed).  The seeds were picked on the
# CPU so that every activated layer's float64 pre-activation keeps undecided_share <= UNDECIDED_CAP
# (tests/test_adversarial2d_cpu.py checks exactly that; a tensor under ~2000 elements sits one element away from the cap).
CHAINS = {"8@80": (8, 80, 80, (2, 2), 4, "uniform", 0),
          "64@32": (64, 32, 32, (1, 1), 4, "uniform", 0)}
CHAIN_CLASSES = 4


def chain_inputs(name, law=None, seed=None):
    """(image, logits, state_dict, masks, target, pool) of a chain."""
    ndf, H, W, pool, N, law0, seed0 = CHAINS[name]
    law, seed = law or law0, seed0 if seed is None else seed
    img, lg, _ = golden_inputs(N, CHAIN_CLASSES, H, W)
    sd = uniform_state_dict(CHAIN_CLASSES, ndf, 1, seed) if law == "uniform" else golden_state_dict(CHAIN_CLASSES, ndf, 1)
    target = (torch.arange(N) < (N + 1) // 2).int()
    return img, lg, sd, golden_masks(ndf, N), target, pool


GOLDEN_LATTICE = 12     # the map gradient is stored at every 12th pixel per axis, offset 5


def lattice(t):
    return t[..., 5::GOLDEN_LATTICE, 5::GOLDEN_LATTICE]
