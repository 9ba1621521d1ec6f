"""Float64 restatement of the FixMatch loss tail (reference code/train_Fixmatch_CNN_2D.py:132-166, :259-288) with closed-form
gradients, the literal reference expression for torch.autograd to differentiate, the decision margins the GPU tests
assert on, and the colour-jitter formula.  CPU only; shared by test_fixmatch_cpu.py and test_fixmatch_gpu.py.

Logits are ``[B, C, S]`` (any trailing shape is flattened), labels ``[L, S]``.  ``out`` has the layout of mis_fixmatch_tail:
[loss, sup_ce, sup_dice, unsup, w, ce_u, dice_u, ce_comp, as_weight, masked_in_fraction]."""
import math

import torch

EPS32 = 2.0 ** -23            # torch.finfo(torch.float32).eps: the clamp of Categorical(probs=...) in the reference's dtype
SMOOTH = 1e-5


def _flat(z, dtype):
    return z.detach().to(dtype).reshape(z.shape[0], z.shape[1], -1)


def decisions(zw, tau, dtype=torch.float64):
    """(pseudo [B, S], comp [B, S], passed [B, S]) of weak logits: the mask ((p - min) / max > tau), argmax of the masked
    softmax and argmin of the softmax, first extremum wins; ``passed``: the mask kept any class."""
    pw = torch.softmax(_flat(zw, dtype), 1)
    mn, mx = pw.min(1, keepdim=True)[0], pw.max(1, keepdim=True)[0]
    mask = ((pw - mn) / mx) > tau
    return torch.argmax(pw * mask.to(dtype), 1), torch.argmin(pw, 1), mask.any(1)


def decision_margins(zw, tau):
    """Per pixel, in float64: (pseudo margin, comp margin).  Pseudo: the smallest relative distance of a mask comparison,
    |n_c - tau| / tau, and the relative gap between the two largest masked values when they differ (an exact tie is resolved
    first-wins on both sides and has no margin to keep).  Comp: the relative gap between the two smallest softmax values,
    likewise."""
    pw = torch.softmax(_flat(zw, torch.float64), 1)
    mn, mx = pw.min(1, keepdim=True)[0], pw.max(1, keepdim=True)[0]
    n = (pw - mn) / mx
    m_mask = ((n - tau).abs() / tau).min(1)[0]
    top = torch.sort(pw * (n > tau).double(), 1, descending=True)[0]
    gap = (top[:, 0] - top[:, 1]) / top[:, 0].clamp(min=1e-300)
    gap = torch.where((top[:, 0] == top[:, 1]) | (top[:, 0] == 0), torch.ones_like(gap), gap)
    low = torch.sort(pw, 1)[0]
    cgap = (low[:, 1] - low[:, 0]) / low[:, 1]
    cgap = torch.where(low[:, 1] == low[:, 0], torch.ones_like(cgap), cgap)
    return torch.minimum(m_mask, gap), cgap


def clamp_margin(zs, eps=EPS32):
    """The smallest relative distance, over every (b, c, s), of q = ps / sum_s ps from the two clamp bounds: |q / eps - 1| and
    |(1 - q) / eps - 1| (1 - q as the sum of the other pixels' q: no cancellation), in float64."""
    ps = torch.softmax(_flat(zs, torch.float64), 1)
    A = ps.sum(2, keepdim=True)
    q = ps / A
    one_minus = (A - ps) / A
    return min((q / eps - 1).abs().min().item(), (one_minus / eps - 1).abs().min().item())


def clamped_share(zs, eps=EPS32):
    """(share of (b, c, s) with q < eps, number with q > 1 - eps), float64."""
    ps = torch.softmax(_flat(zs, torch.float64), 1)
    A = ps.sum(2, keepdim=True)
    return ((ps / A) < eps).double().mean().item(), int((((A - ps) / A) < eps).sum())


def _dice(p, y, C):
    """(loss, dloss/dp) of losses.DiceLoss(C) (code/utils/losses.py:165-201) on probabilities p [n, C, S], labels y [n, S]."""
    t = torch.nn.functional.one_hot(y.long(), C).permute(0, 2, 1).to(p.dtype)
    inter, ys, zs = (p * t).sum((0, 2)), (t * t).sum((0, 2)), (p * p).sum((0, 2))
    num, den = 2 * inter + SMOOTH, zs + ys + SMOOTH
    loss = (1 - num / den).mean()
    g = (-2 * t / den[None, :, None] + 2 * p * (num / den ** 2)[None, :, None]) / C
    return loss, g


def _ce(z, y):
    """(mean cross-entropy, dloss/dz) of logits z [n, C, S] against labels y [n, S]."""
    lse = torch.logsumexp(z, 1)
    zy = torch.gather(z, 1, y.long().unsqueeze(1)).squeeze(1)
    n = y.numel()
    g = torch.softmax(z, 1)
    g = g - torch.nn.functional.one_hot(y.long(), z.shape[1]).permute(0, 2, 1).to(z.dtype)
    return (lse - zy).mean(), g / n


def _through_softmax(p, g):
    return p * (g - (g * p).sum(1, keepdim=True))


def fixmatch_tail(zw, zs, label, L, tau, w, eps=EPS32, dtype=torch.float64, pseudo=None, comp=None):
    """(out [10], d_weak, d_strong) in ``dtype`` (gradients shaped like the logits).  ``pseudo`` ([B - L, S]) / ``comp``
    ([B, S]) replace the oracle's own decisions (the arbiter form of the continuous-logit tests)."""
    shape = zw.shape
    zw, zs = _flat(zw, dtype), _flat(zs, dtype)
    B, C, S = zw.shape
    label = label.reshape(L, S).long()
    pw, ps = torch.softmax(zw, 1), torch.softmax(zs, 1)
    own_pseudo, own_comp, passed = decisions(zw, tau, dtype)
    pseudo = own_pseudo[L:] if pseudo is None else pseudo.reshape(B - L, S).long()
    comp = own_comp if comp is None else comp.reshape(B, S).long()
    # supervised
    sup_ce, g_ce = _ce(zw[:L], label)
    sup_dice, g_dp = _dice(pw[:L], label, C)
    d_weak = torch.zeros_like(zw)
    d_weak[:L] = g_ce + _through_softmax(pw[:L], g_dp)
    # pseudo-label terms on the strong pass
    ce_u, g_ceu = _ce(zs[L:], pseudo)
    dice_u, g_du = _dice(ps[L:], pseudo, C)
    # complementary cross-entropy: logits 1 - ps
    ce_comp, g_x = _ce(1 - ps, comp)
    # adaptive weight
    A = ps.sum(2, keepdim=True)
    q = ps / A
    lq = torch.log(q.clamp(eps, 1 - eps))
    H = -(q * lq).sum(2)
    norm = B * C * math.log(S)
    a = 1 - H.sum() / norm
    fp = -lq - ((q >= eps) & (q <= 1 - eps)).to(dtype)
    T = (q * fp).sum(2, keepdim=True)
    da_dps = -(fp - T) / (norm * A)
    unsup = ce_u + dice_u + a * a * ce_comp
    loss = sup_ce + sup_dice + w * unsup
    g_ps = w * (-a * a * g_x + 2 * a * ce_comp * da_dps)
    g_ps[L:] += w * g_du
    d_strong = _through_softmax(ps, g_ps)
    d_strong[L:] += w * g_ceu
    out = torch.stack([loss, sup_ce, sup_dice, unsup, torch.tensor(w, dtype=dtype), ce_u, dice_u, ce_comp, a,
                       passed[L:].to(dtype).mean()])
    return out, d_weak.reshape(shape), d_strong.reshape(shape)


def reference_autograd(zw, zs, label, L, tau, w, dtype, pseudo=None, comp=None):
    """The literal reference expression (train_Fixmatch_CNN_2D.py:132-166, :259-288) in ``dtype`` under torch.autograd:
    Categorical(probs=...).entropy(), CrossEntropyLoss and the DiceLoss of code/utils/losses.py written out.  Returns the same
    triple as ``fixmatch_tail``.  ``pseudo`` / ``comp`` replace the expression's own (detached) label maps."""
    from torch.distributions import Categorical
    shape = zw.shape
    B, C = shape[0], shape[1]
    outputs_weak = _flat(zw, dtype).requires_grad_(True)
    outputs_strong = _flat(zs, dtype).requires_grad_(True)
    S = outputs_weak.shape[2]
    label = label.reshape(L, S)
    ce_loss = torch.nn.CrossEntropyLoss()

    def dice_loss(inputs, target):                       # losses.DiceLoss.forward, weight None, softmax False
        target = torch.cat([(target == i).to(dtype) for i in range(C)], dim=1)
        loss = 0.0
        for i in range(C):
            score, tgt = inputs[:, i], target[:, i]
            intersect = torch.sum(score * tgt)
            y_sum = torch.sum(tgt * tgt)
            z_sum = torch.sum(score * score)
            loss = loss + (1 - (2 * intersect + SMOOTH) / (z_sum + y_sum + SMOOTH))
        return loss / C

    def normalize(tensor):
        min_val = tensor.min(1, keepdim=True)[0]
        max_val = tensor.max(1, keepdim=True)[0]
        return (tensor - min_val) / max_val

    outputs_weak_soft = torch.softmax(outputs_weak, dim=1)
    outputs_strong_soft = torch.softmax(outputs_strong, dim=1)
    pseudo_mask = (normalize(outputs_weak_soft) > tau).to(dtype)
    outputs_weak_masked = outputs_weak_soft * pseudo_mask
    pseudo_outputs = torch.argmax(outputs_weak_masked[L:].detach(), dim=1, keepdim=False)
    if pseudo is not None:
        pseudo_outputs = pseudo.reshape(B - L, S).long()
    sup_ce = ce_loss(outputs_weak[:L], label.long())
    sup_dice = dice_loss(outputs_weak_soft[:L], label.unsqueeze(1))
    il_output = torch.reshape(outputs_strong_soft, (B, C, S))
    # validate_args: the simplex check of the normalised rows is a tolerance test (1e-6) that long fp32 rows can miss; it
    # does not enter the arithmetic
    as_weight = torch.mean(1 - (Categorical(probs=il_output, validate_args=False).entropy() / math.log(S)))
    comp_labels = torch.argmin(outputs_weak_soft.detach(), dim=1, keepdim=False)
    if comp is not None:
        comp_labels = comp.reshape(B, S).long()
    ce_comp = ce_loss(torch.add(torch.negative(outputs_strong_soft), 1), comp_labels)
    comp_loss = as_weight * ce_comp
    ce_u = ce_loss(outputs_strong[L:], pseudo_outputs)
    dice_u = dice_loss(outputs_strong_soft[L:], pseudo_outputs.unsqueeze(1))
    unsup_loss = ce_u + dice_u + as_weight * comp_loss
    loss = sup_ce + sup_dice + w * unsup_loss
    loss.backward()
    out = torch.stack([loss, sup_ce, sup_dice, unsup_loss, torch.tensor(w, dtype=dtype), ce_u, dice_u, ce_comp, as_weight,
                       pseudo_mask[L:].amax(1).mean()]).detach()
    return out, outputs_weak.grad.reshape(shape), outputs_strong.grad.reshape(shape)


def color_jitter(x, params, dtype=torch.float64):
    """ColorJitter(0.8, 0.8, 0.8, 0.2) on one-channel images x [B, 1, ...] with given factors ``params`` [B, 3] = (beta,
    gamma, order): torchvision's F.adjust_brightness is _blend(img, 0, beta) = clamp(beta * img, 0, 1), F.adjust_contrast is
    _blend(img, mean(img), gamma) = clamp(gamma * img + (1 - gamma) * mean(img), 0, 1); F.adjust_saturation and F.adjust_hue
    return a one-channel image unchanged.  order 0: brightness then contrast, 1: contrast then brightness."""
    x = x.to(dtype)
    B = x.shape[0]
    out = torch.empty_like(x)
    for b in range(B):
        beta, gamma, order = float(params[b, 0]), float(params[b, 1]), int(params[b, 2])
        img = x[b]
        for op in ((0, 1) if order == 0 else (1, 0)):
            if op == 0:
                img = (beta * img).clamp(0, 1)
            else:
                img = (gamma * img + (1 - gamma) * img.mean()).clamp(0, 1)
        out[b] = img
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the edge matrix of the tail (inputs are built on the CPU; test_fixmatch_cpu.py checks their margins, test_fixmatch_gpu.py
# runs the kernel on them)
# ---------------------------------------------------------------------------------------------------------------------
TAU = 0.8
W = 0.37
# "cap" / "capvec": one workgroup per sample past the cap of 2048 / B workgroups per sample (256 work items each) on the
# scalar path (odd S) and on the float4 path
SHAPES = {"2d": (32, 48), "part": (40, 52), "odd": (7, 9), "cap": (5, 52429), "capvec": (4, 262145)}
# added to a case's seed where the first draw leaves some q = ps / A within 1e-3 (relative) of a clamp bound
SEED_BUMP = {"C3-u8-2d-B4-L2-dense-float-quant": 2, "C4-u8-2d-B4-L2-dense-float-quant": 2,
             "C4-i64-2d-B4-L2-dense-float-quant": 14, "C3-u8-2d-B5-L1-dense-float-quant": 3,
             "C4-u8-2d-B5-L4-dense-float-quant": 3, "C2-u8-part-B4-L2-offset-float-quant": 1,
             "C4-i64-2d-B4-L2-strided-float-quant": 2, "C4-u8-part-B4-L2-offset-float-quant": 1,
             "C4-u8-2d-B4-L2-shift1-float-quant": 15, "C3-u8-2d-B4-L2-dense-float-missing": 2,
             "C4-i64-part-B4-L2-dense-float-missing": 4, "C4-u8-2d-B4-L2-dense-float-sat": 2,
             "C4-u8-2d-B4-L2-dense-float-allmask": 3, "C4-u8-2d-B4-L2-dense-float-clamp": 25}


def case(**kw):
    c = dict(C=3, ldt="u8", shape="2d", B=4, L=2, layout="dense", wmode="float", content="quant")
    c.update(kw)
    return c


def cid(c):
    return "-".join(f"{k}{c[k]}" if k in ("C", "B", "L") else str(c[k])
                    for k in ("C", "ldt", "shape", "B", "L", "layout", "wmode", "content"))


def matrix():
    cs = [case(C=C, ldt=ldt, shape=shape) for C in (2, 3, 4) for ldt in ("u8", "i64") for shape in ("2d", "part", "odd")]
    cs += [case(B=5, L=1), case(B=5, L=4, C=4), case(B=5, L=1, C=2, shape="odd"), case(B=3, L=2, shape="part", ldt="i64")]
    for C in (2, 3, 4):
        cs += [case(C=C, layout="strided", ldt="i64"), case(C=C, layout="offset", shape="part"),
               case(C=C, layout="shift1")]
    cs += [case(wmode="state"), case(C=4, wmode="state", layout="strided", shape="part"), case(C=2, wmode="state", shape="odd")]
    cs += [case(C=3, content="missing"), case(C=4, content="missing", ldt="i64", shape="part")]
    for C in (2, 3, 4):
        cs += [case(C=C, content=k) for k in ("sat", "nomask", "allmask", "clamp", "peak")]
    cs += [case(C=2, shape="cap", B=2, L=1), case(C=2, shape="capvec", B=2, L=1, ldt="i64")]
    cs += [case(C=2, content="cont"), case(C=3, content="cont", shape="part", ldt="i64"),
           case(C=4, content="cont", shape="odd"), case(C=4, content="cont", layout="strided", wmode="state")]
    return cs


def quantise(z):
    return torch.round(z * 4) / 4          # multiples of 0.25: ties are exact, no threshold can be approached


def inputs(c):
    """(zw, zs [B, C, 1, H, W] fp32, label [L, H, W]) of one case."""
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(("fixmatch" + cid(c)).encode()) + SEED_BUMP.get(cid(c), 0))
    C, B, L, sp = c["C"], c["B"], c["L"], SHAPES[c["shape"]]
    S = sp[0] * sp[1]
    content = c["content"]
    # "sat": most softmaxes round to exactly 1 and 0 + tiny in fp32 (a gap of 17 does that), but no gap exceeds 80: past 87
    # fp32 softmax underflows to 0 and creates arg-min ties that float64 does not have
    r = lambda: (torch.randn((B, C, S), generator=g) * 25).clamp(-40, 40) if content == "sat" else \
        torch.randn((B, C, S), generator=g) * 3.0
    zw, zs = r(), r()
    label = torch.randint(0, C, (L, S), generator=g)
    if content == "missing":
        label[label == C - 1] = 0
    if content == "nomask":                # (max - min) / max = 1 - e^-(range) <= 1 - e^-1.5 = 0.777 < tau: nothing passes
        zw = torch.randint(0, 7, (B, C, S), generator=g).float() * 0.25
    if content == "allmask":               # one class 3.5 above a spread of at most 1.5: 1 - e^-2 = 0.865 > tau everywhere
        zw = torch.randint(0, 7, (B, C, S), generator=g).float() * 0.25
        top = torch.randint(0, C, (B, 1, S), generator=g)
        zw.scatter_add_(1, top, torch.full((B, 1, S), 3.5))
    if content == "clamp":                 # class C-1: e^-12 on three quarters of the pixels, ordinary on the rest:
        sel = torch.rand((B, S), generator=g) < 0.75      # A ~ S / 4C, q ~ e^-12 / A < 2^-23 on the planted pixels
        zs[:, C - 1][sel] = -12.0
    if content == "peak":                  # class 0 holds its whole mass in one pixel: q > 1 - 2^-23 there
        zs[:, 0] = -30.0
        zs[:, 1:] = zs[:, 1:].clamp(-3, 3)
        at = torch.randint(0, S, (B,), generator=g)
        zs[torch.arange(B), 0, at] = 10.0
    if content != "cont":
        zw, zs = quantise(zw), quantise(zs)
    label = label.to(torch.uint8 if c["ldt"] == "u8" else torch.int64)
    return zw.reshape((B, C, 1) + sp), zs.reshape((B, C, 1) + sp), label.reshape((L,) + sp)


# ---------------------------------------------------------------------------------------------------------------------
# tolerance of the GPU tests (the convention of tests/test_loss_tails_gpu.py) and the schedule
# ---------------------------------------------------------------------------------------------------------------------
K = 6.0
# the largest e32 (fp32 torch.autograd of the literal expression against the float64 oracle) over matrix(), per scalar and
# per gradient tensor, measured by test_fixmatch_cpu.py::test_floors_are_the_largest_e32_of_the_matrix, which holds them
# to that measurement: 1.05e-6 (a scalar of C2-u8-part-B4-L2-offset-float-quant) and 3.38e-7
FLOOR_SCALAR = 1.1e-6
FLOOR_TENSOR = 3.4e-7


def rel(a, ref):
    m = ref.abs().max().item()
    return (a.double() - ref).abs().max().item() / m if m > 0 else (a.double() - ref).abs().max().item()


def scalar_rels(out, ref):
    """Relative error of every scalar of ``out`` against ``ref`` (absolute where the reference is exactly 0)."""
    return [abs(out[i].item() - ref[i].item()) / abs(ref[i].item()) if ref[i].item() != 0 else abs(out[i].item())
            for i in range(ref.numel())]


def e32(c, zw, zs, label, ref, pseudo=None, comp=None):
    """(scalar e32 list, d_weak e32, d_strong e32) of one case: the literal expression under fp32 torch.autograd on the CPU
    against the float64 triple ``ref``.  Continuous-logit cases pass the decisions the float64 side used."""
    o, gw, gs = reference_autograd(zw, zs, label, c["L"], TAU, float(torch.tensor(W, dtype=torch.float32)),
                                   torch.float32, pseudo=pseudo, comp=comp)
    return scalar_rels(o.double(), ref[0]), rel(gw, ref[1]), rel(gs, ref[2])


def schedule(it, base_lr, max_iterations, ema_decay, consistency, rampup):
    """(lr after the step, EMA alpha of the step, consistency weight of the step) at iteration ``it`` as the reference
    computes them (train_Fixmatch_CNN_2D.py:102-111, :270, :297): the weight from ``it // 150``, alpha =
    min(1 - 1 / (it + 1), decay), lr = base_lr * (1 - it / max) ** 0.9 with ``it`` before its increment."""
    epoch = it // 150
    if rampup == 0:
        ramp = 1.0
    else:
        cur = min(max(float(epoch), 0.0), rampup)
        ramp = math.exp(-5.0 * (1.0 - cur / rampup) ** 2)
    return base_lr * (1.0 - it / max_iterations) ** 0.9, min(1 - 1 / (it + 1), ema_decay), consistency * ramp
