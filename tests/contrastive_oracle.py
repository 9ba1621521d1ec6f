"""Reference arithmetic of contrastive cross teaching (reference code/train_Contrastive_Cross_CNN_2D.py:212-261): the
frozen heads (networks/projector.py:50-92), the two pixel-wise contrastive losses (utils/losses.py:283-337, :479-531), the
supervised / pseudo-label terms and the gradient of the whole loss at both students' logits.

Everything that arbitrates is float64 numpy written from the formulas, with its backward by hand -- no autograd, nothing
shared with the kernels or with torch's operators: tests/golden/contrastive_cross.npz (the REAL reference's modules under
float64 autograd, scripts/gen_contrastive_golden.py) holds it to 1e-10 in tests/test_contrastive_cpu.py, and it then
arbitrates the GPU tests.  ``tail_torch`` is the other thing here: one student's share of the loss as the literal torch
expression, under autograd in a chosen dtype; its fp32 evaluation against float64 is e32, the yardstick of the tail's gate.

Gate of the tail (the convention of tests/test_fixmatch_gpu.py):  |hip - f64|max <= max(K * e32, FLOOR) * |f64|max.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS_BN = 1e-5
MOMENTUM_BN = 0.1
TEMPERATURE = 0.07
SCALES = dict(sup=2.0, contrastive=0.5, pseudo=1.25)          # reference :261


# ---------------------------------------------------------------------------------------------------------------------
# the heads: conv 3x3 -> BatchNorm (batch statistics) -> ReLU -> MaxPool 2, forward and input gradient
# ---------------------------------------------------------------------------------------------------------------------
def conv2d(x, w, b):
    """'same' cross-correlation, odd square kernel: x [N, Ci, H, W], w [Co, Ci, k, k], b [Co]."""
    k = w.shape[2]
    p = k // 2
    N, _, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))
    y = np.zeros((N, w.shape[0], H, W))
    for i in range(k):
        for j in range(k):
            y += np.einsum("nchw,oc->nohw", xp[:, :, i:i + H, j:j + W], w[:, :, i, j])
    return y + b[None, :, None, None]


def conv2d_dx(dy, w):
    """dx[n, c, h, w] = sum_{o, i, j} dy[n, o, h + p - i, w + p - j] w[o, c, i, j]"""
    k = w.shape[2]
    p = k // 2
    N, _, H, W = dy.shape
    dp = np.pad(dy, ((0, 0), (0, 0), (p, p), (p, p)))
    dx = np.zeros((N, w.shape[1], H, W))
    for i in range(k):
        for j in range(k):
            dx += np.einsum("nohw,oc->nchw", dp[:, :, 2 * p - i:2 * p - i + H, 2 * p - j:2 * p - j + W], w[:, :, i, j])
    return dx


def _block_fwd(x, sd, pre):
    t = conv2d(x, sd[pre + ".conv.weight"], sd[pre + ".conv.bias"])
    n = t.shape[0] * t.shape[2] * t.shape[3]
    mean = t.mean(axis=(0, 2, 3))
    var = t.var(axis=(0, 2, 3))                                 # biased: what normalises
    rstd = 1.0 / np.sqrt(var + EPS_BN)
    xhat = (t - mean[None, :, None, None]) * rstd[None, :, None, None]
    z = xhat * sd[pre + ".bn.weight"][None, :, None, None] + sd[pre + ".bn.bias"][None, :, None, None]
    a = np.maximum(z, 0.0)
    N, C, H, W = a.shape
    win = a.reshape(N, C, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
    arg = win.argmax(axis=4)                                    # first maximum of the window, row-major
    y = np.take_along_axis(win, arg[..., None], axis=4)[..., 0]
    stats = dict(mean=mean, var=var, var_unbiased=var * n / max(n - 1, 1))
    top = np.sort(win, axis=4)
    return y, dict(xhat=xhat, rstd=rstd, a=a, arg=arg, stats=stats, pre=z, gap=top[..., 3] - top[..., 2])


def _block_bwd(dy, sd, pre, c, decision=None):
    """``decision`` = (ReLU mask [N, C, H, W], window position [N, C, H/2, W/2]) replaces the float64 decisions: the gradient
    is then the exact one of the branch those decisions select (a GPU pass arbitrates its own near-ties)."""
    N, C, H, W = c["a"].shape
    mask, arg = (c["a"] > 0, c["arg"]) if decision is None else decision        # ReLU: derivative 0 at 0
    dwin = np.zeros((N, C, H // 2, W // 2, 4))
    np.put_along_axis(dwin, np.asarray(arg, dtype=np.int64)[..., None], dy[..., None], axis=4)
    da = dwin.reshape(N, C, H // 2, W // 2, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, H, W)
    dz = da * mask
    dxhat = dz * sd[pre + ".bn.weight"][None, :, None, None]
    m1 = dxhat.mean(axis=(0, 2, 3), keepdims=True)
    m2 = (dxhat * c["xhat"]).mean(axis=(0, 2, 3), keepdims=True)
    dt = c["rstd"][None, :, None, None] * (dxhat - m1 - c["xhat"] * m2)
    return conv2d_dx(dt, sd[pre + ".conv.weight"])


def head_forward(sd, x, blocks, final):
    """(features, cache): ``blocks`` = 2 projector / 3 classifier; ``final``: the classifier's 1x1 convolution."""
    sd = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    caches = []
    y = np.asarray(x, dtype=np.float64)
    for i in range(1, blocks + 1):
        y, c = _block_fwd(y, sd, f"conv_{i}")
        caches.append(c)
    if final:
        y = conv2d(y, sd["final.weight"], sd["final.bias"])
    return y, dict(sd=sd, blocks=caches, final=final)


def head_input_grad(dfeat, cache, decisions=None):
    """``decisions``: per block, see _block_bwd."""
    sd, d = cache["sd"], np.asarray(dfeat, dtype=np.float64)
    if cache["final"]:
        d = conv2d_dx(d, sd["final.weight"])
    for i in range(len(cache["blocks"]), 0, -1):
        d = _block_bwd(d, sd, f"conv_{i}", cache["blocks"][i - 1], None if decisions is None else decisions[i - 1])
    return d


def decisions_of(cache):
    """the float64 decisions, per block: (ReLU mask, window position)"""
    return [(c["a"] > 0, c["arg"]) for c in cache["blocks"]]


def check_decisions(cache, decisions, margin=1e-5, most=8):
    """A pass's own decisions may differ from the float64 ones only where float64 itself is within ``margin`` of the
    boundary (a pre-activation that close to 0, a window whose two largest values are that close), and at most ``most``
    times; a window position only matters where its value survives the ReLU."""
    n = 0
    for c, (mask, arg) in zip(cache["blocks"], decisions):
        dm = np.asarray(mask, dtype=bool) != (c["a"] > 0)
        assert not (dm & (np.abs(c["pre"]) > margin)).any()
        y = np.take_along_axis(
            c["a"].reshape(c["a"].shape[0], c["a"].shape[1], c["a"].shape[2] // 2, 2, c["a"].shape[3] // 2, 2)
            .transpose(0, 1, 2, 4, 3, 5).reshape(c["arg"].shape + (4,)), c["arg"][..., None], axis=4)[..., 0]
        da = (np.asarray(arg, dtype=np.int64) != c["arg"]) & (y > 0)
        assert not (da & (c["gap"] > margin)).any()
        n += int(dm.sum()) + int(da.sum())
    assert n <= most, n
    return n


def head_torch(sd, x, blocks, final, dtype, decisions, dfeat=None):
    """The head as torch operators in ``dtype`` with the given decisions: (features, batch statistics per block, BatchNorm
    buffers after the pass, input gradient for ``dfeat``).  fp32 against the float64 oracle is the e32 of the heads' gates."""
    t64 = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    xin = t64(x).clone().requires_grad_(True)
    y, stats, after = xin, [], {}
    for i in range(1, blocks + 1):
        pre = f"conv_{i}"
        t = F.conv2d(y, t64(sd[pre + ".conv.weight"]), t64(sd[pre + ".conv.bias"]), padding=1)
        rm, rv = t64(sd[pre + ".bn.running_mean"]).clone(), t64(sd[pre + ".bn.running_var"]).clone()
        stats.append((t.detach().mean(dim=(0, 2, 3)), 1.0 / torch.sqrt(t.detach().var(dim=(0, 2, 3), unbiased=False) + EPS_BN)))
        t = F.batch_norm(t, rm, rv, t64(sd[pre + ".bn.weight"]), t64(sd[pre + ".bn.bias"]), True, MOMENTUM_BN, EPS_BN)
        after[pre + ".bn.running_mean"], after[pre + ".bn.running_var"] = rm, rv
        mask, arg = decisions[i - 1]
        a = t * torch.as_tensor(np.asarray(mask)).to(dtype)
        N, C, H, W = a.shape
        win = a.reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
        y = win.gather(4, torch.as_tensor(np.asarray(arg, dtype=np.int64))[..., None])[..., 0]
    if final:
        y = F.conv2d(y, t64(sd["final.weight"]), t64(sd["final.bias"]))
    g = None
    if dfeat is not None:
        g, = torch.autograd.grad(y, xin, t64(dfeat))
    return y.detach(), stats, after, g


def running_after(sd, cache, passes=1):
    """The BatchNorm buffers after ``passes`` train-mode forwards on the input of ``cache`` (momentum 0.1, unbiased variance)."""
    out = {}
    for i, c in enumerate(cache["blocks"], start=1):
        rm = np.asarray(sd[f"conv_{i}.bn.running_mean"], dtype=np.float64)
        rv = np.asarray(sd[f"conv_{i}.bn.running_var"], dtype=np.float64)
        for _ in range(passes):
            rm = (1 - MOMENTUM_BN) * rm + MOMENTUM_BN * c["stats"]["mean"]
            rv = (1 - MOMENTUM_BN) * rv + MOMENTUM_BN * c["stats"]["var_unbiased"]
        out[f"conv_{i}.bn.running_mean"], out[f"conv_{i}.bn.running_var"] = rm, rv
        out[f"conv_{i}.bn.num_batches_tracked"] = int(np.asarray(sd[f"conv_{i}.bn.num_batches_tracked"])) + passes
    return out


def classifier_forward(sd, x):
    return head_forward(sd, x, 3, True)


def projector_forward(sd, x):
    return head_forward(sd, x, 2, False)


# ---------------------------------------------------------------------------------------------------------------------
# the pixel-wise contrastive loss (ConLoss == contrastive_loss_sup, the definition in force) and its gradient at feat_q
# ---------------------------------------------------------------------------------------------------------------------
def _l1_pixels(feat):
    B, d = feat.shape[0], feat.shape[1]
    v = feat.reshape(B, d, -1).transpose(0, 2, 1)               # [B, N, d]
    n = np.maximum(np.abs(v).sum(axis=2, keepdims=True), 1e-12) # F.normalize(p = 1): x / max(||x||_1, eps)
    return v, n


def patch_nce(feat_q, feat_k, temperature=TEMPERATURE):
    """(loss, d loss / d feat_q): loss = mean_i (logsumexp_j s_ij - s_ii), s_ij = q^_i . k^_j / T over the pixels of one sample
    (the positive column plus the diagonal-masked negatives of the reference are the row {s_ij : all j})."""
    q, nq = _l1_pixels(np.asarray(feat_q, dtype=np.float64))
    k, nk = _l1_pixels(np.asarray(feat_k, dtype=np.float64))
    qn, kn = q / nq, k / nk
    B, N, d = qn.shape
    s = np.einsum("bid,bjd->bij", qn, kn) / temperature
    mx = s.max(axis=2, keepdims=True)
    e = np.exp(s - mx)
    z = e.sum(axis=2, keepdims=True)
    lse = (mx + np.log(z))[..., 0]
    pos = np.einsum("bii->bi", s)
    loss = (lse - pos).mean()
    soft = e / z
    dqn = (np.einsum("bij,bjd->bid", soft, kn) - kn) / (temperature * B * N)
    # through q^ = q / max(||q||_1, eps): the norm's derivative is sign(q), and 0 where the clamp holds
    live = (np.abs(q).sum(axis=2, keepdims=True) > 1e-12)
    dq = dqn / nq - live * np.sign(q) * (dqn * q).sum(axis=2, keepdims=True) / (nq * nq)
    return loss, dq.transpose(0, 2, 1).reshape(np.asarray(feat_q).shape)


# ---------------------------------------------------------------------------------------------------------------------
# CE + Dice + pseudo-label Dice of one student, and their gradient at its logits
# ---------------------------------------------------------------------------------------------------------------------
def _softmax(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _dice(p, onehot):
    """(mean over classes of 1 - (2 I + s) / (Z + Y + s), its gradient at p); sums over batch and pixels (losses.py:165-201)"""
    C = p.shape[1]
    ax = (0,) + tuple(range(2, p.ndim))
    smooth = 1e-5
    I, Y, Z = (p * onehot).sum(axis=ax), onehot.sum(axis=ax), (p * p).sum(axis=ax)
    num, den = 2 * I + smooth, Z + Y + smooth
    sh = (1, C) + (1,) * (p.ndim - 2)
    grad = (-2 * onehot / den.reshape(sh) + 2 * p * (num / (den * den)).reshape(sh)) / C
    return (1 - num / den).mean(), grad


def _through_softmax(p, g):
    return p * (g - (g * p).sum(axis=1, keepdims=True))


def _onehot(y, C):
    return np.moveaxis(np.eye(C)[np.asarray(y, dtype=np.int64)], -1, 1)


def student_tail(own, other, label, L, w, sup_scale=SCALES["sup"], pseudo_scale=SCALES["pseudo"], extra_l=None,
                 extra_u=None, extra_scale=1.0):
    """One student's tail, the layout of mis_contrastive_cross_tail: (out [6], dlogits).  own / other [B, C, *sp], label
    [L, *sp]; extra_l [L/2, C, *sp] is added on the labeled rows 0, 2, ..., extra_u [B-L, C, *sp] on the unlabeled rows."""
    own, other = np.asarray(own, dtype=np.float64), np.asarray(other, dtype=np.float64)
    B, C = own.shape[0], own.shape[1]
    p = _softmax(own)
    oh = _onehot(label[:L], C)
    nlab = oh.size / C
    ce = -(np.log(p[:L]) * oh).sum() / nlab
    dice, gd = _dice(p[:L], oh)
    d = np.zeros_like(own)
    ks = 0.5 * sup_scale
    d[:L] = ks * ((p[:L] - oh) / nlab + _through_softmax(p[:L], gd))
    ps = 0.0
    if B > L:
        ohu = _onehot(other[L:].argmax(axis=1), C)              # first maximum wins, as torch.argmax
        ps, gu = _dice(p[L:], ohu)
        d[L:] = pseudo_scale * w * _through_softmax(p[L:], gu)
        if extra_u is not None:
            d[L:] += extra_scale * np.asarray(extra_u, dtype=np.float64)
    if extra_l is not None:
        d[0:L:2] += extra_scale * np.asarray(extra_l, dtype=np.float64)
    out = np.array([ks * (ce + dice) + pseudo_scale * w * ps, ce, dice, ps, w, 0.5 * (ce + dice) + w * ps])
    return out, d


def argmax_margin(z):
    """smallest gap between the two largest logits over all pixels"""
    s = np.sort(np.asarray(z, dtype=np.float64), axis=1)
    return float((s[:, -1] - s[:, -2]).min())


# ---------------------------------------------------------------------------------------------------------------------
# the whole step at the logits
# ---------------------------------------------------------------------------------------------------------------------
def loss_and_grads(z1, z2, label, L, w, heads, decisions=None):
    """``heads``: state dicts (name -> array) under "classifier_1", "classifier_2", "projector_1", "projector_2".
    Returns the scalars of :220-261, every head output, and d loss / d z1, d loss / d z2.  ``decisions``: the ReLU /
    max-pool decisions of a pass under "classifier_1" / "projector_1" (head_input_grad), for the backward only."""
    z1, z2 = np.asarray(z1, dtype=np.float64), np.asarray(z2, dtype=np.float64)
    c = SCALES["contrastive"]
    fq_l, cq_l = classifier_forward(heads["classifier_1"], z1[:L][0::2])
    fk_l, ck_l = classifier_forward(heads["classifier_2"], z2[:L][1::2])
    fq_u, cq_u = projector_forward(heads["projector_1"], z1[L:])
    fk_u, ck_u = projector_forward(heads["projector_2"], z2[L:])
    lc_l, dq_l = patch_nce(fq_l, fk_l)
    lc_u, dq_u = patch_nce(fq_u, fk_u)
    dec = decisions or {}
    e_l = head_input_grad(c * dq_l, cq_l, dec.get("classifier_1"))
    e_u = head_input_grad(c * dq_u, cq_u, dec.get("projector_1"))
    o1, d1 = student_tail(z1, z2, label, L, w, extra_l=e_l, extra_u=e_u)
    o2, d2 = student_tail(z2, z1, label, L, w)
    return dict(loss=o1[0] + o2[0] + c * (lc_l + lc_u), Lc_l=lc_l, Lc_u=lc_u, sup_1=0.5 * (o1[1] + o1[2]),
                sup_2=0.5 * (o2[1] + o2[2]), ps_1=o1[3], ps_2=o2[3], model1_loss=o1[5], model2_loss=o2[5], out1=o1, out2=o2,
                feat_l_q=fq_l, feat_l_k=fk_l, feat_q=fq_u, feat_k=fk_u, dz1=d1, dz2=d2, extra_l=e_l, extra_u=e_u,
                caches=dict(classifier_1=cq_l, classifier_2=ck_l, projector_1=cq_u, projector_2=ck_u))


# ---------------------------------------------------------------------------------------------------------------------
# the schedule: the literal Python of the script (:107-110, :196-218, :274-284)
# ---------------------------------------------------------------------------------------------------------------------
def literal_schedule(steps, base_lr, max_iterations, consistency, rampup, iters_per_epoch):
    """[(lr the step ran with, consistency weight of the step)] for iterations 0 .. steps - 1, by running the script's own
    statements in its own order, the local ``base_lr`` reassigned as the script reassigns it."""
    def ramp_up_function(epoch, epoch_with_max_rampup=80):
        if epoch < epoch_with_max_rampup:
            p = max(0.0, float(epoch)) / float(epoch_with_max_rampup)
            p = 1.0 - p
            return math.exp(-p * p * 5.0)
        else:
            return 1.0

    rows, iter_num, lr_ = [], 0, base_lr
    for epoch_num in range(steps // iters_per_epoch + 1):
        for _ in range(iters_per_epoch):
            if iter_num >= steps:
                break
            consistency_weight = consistency * ramp_up_function(epoch_num, rampup)
            rows.append((lr_, consistency_weight))               # optimizer.step() runs with the lr_ set one iteration ago
            if iter_num / max_iterations > 0.5:
                base_lr = 0.0001
                lr_ = base_lr * (1.0 - (iter_num-max_iterations*0.5) / max_iterations*0.5) ** 0.9
            else:
                lr_ = base_lr * (1.0 - iter_num / max_iterations) ** 0.9
            iter_num = iter_num + 1
    return rows


# ---------------------------------------------------------------------------------------------------------------------
# the tail's case matrix, its literal torch expression, and the gate
# ---------------------------------------------------------------------------------------------------------------------
K = 6.0
# the largest e32 (fp32 torch.autograd of the literal expression against float64) over matrix(), scalars and gradient
# tensors: measured by tests/test_contrastive_cpu.py::test_floors_are_the_largest_e32_of_the_matrix, which holds them to
# that measurement: 1.647e-7 (a scalar) and 2.140e-7 (a gradient tensor), rounded up at the second digit
FLOOR_SCALAR = 1.7e-7
FLOOR_TENSOR = 2.2e-7
W = 0.0625


def matrix():
    """C x label type x batch layout, then the edges: S off the workgroup's chunk (1024 voxels) and off 4, no head
    gradients (student 2), w = 0, a class absent from the labels, L = B, L = 2, more than one workgroup."""
    cases = []
    for C in (2, 3, 4):
        for lt in ("u8", "i64"):
            for layout in ("dense", "strided"):
                cases.append(dict(C=C, lt=lt, layout=layout, B=6, L=4, sp=(9, 13), extra=True, w=W, absent=False))
    base = dict(C=4, lt="u8", layout="dense", B=6, L=4, sp=(9, 13), extra=True, w=W, absent=False)
    cases += [dict(base, extra=False), dict(base, w=0.0), dict(base, absent=True), dict(base, B=4, L=4),
              dict(base, B=5, L=2, layout="offset"), dict(base, sp=(33, 37), lt="i64"), dict(base, sp=(1, 5), C=3),
              dict(base, extra=False, w=0.0, C=2, layout="strided")]
    return cases


def cid(c):
    return (f"C{c['C']}-{c['lt']}-{c['layout']}-B{c['B']}-L{c['L']}-{c['sp'][0]}x{c['sp'][1]}-"
            f"{'extra' if c['extra'] else 'noextra'}-w{c['w']:g}{'-absent' if c['absent'] else ''}")


def inputs(c):
    """(own, other, label, extra_l, extra_u) as CPU torch tensors, fp32 data: logits scaled so that every class wins pixels."""
    g = torch.Generator().manual_seed(1000 + sum(map(ord, cid(c))))
    B, C, L, sp = c["B"], c["C"], c["L"], c["sp"]
    own = (torch.randn((B, C, 1) + sp, generator=g) * 2.0).float()
    other = (torch.randn((B, C, 1) + sp, generator=g) * 2.0).float()
    hi = C - 1 if c["absent"] else C
    label = torch.randint(0, hi, (L,) + sp, generator=g).to(torch.uint8 if c["lt"] == "u8" else torch.int64)
    extra_l = extra_u = None
    if c["extra"]:
        extra_l = (torch.randn((L // 2, C, 1) + sp, generator=g) * 1e-3).float()
        if B > L:
            extra_u = (torch.randn((B - L, C, 1) + sp, generator=g) * 1e-3).float()
    return own, other, label, extra_l, extra_u


def tail_torch(own, other, label, L, w, dtype, extra_l=None, extra_u=None, sup_scale=SCALES["sup"],
               pseudo_scale=SCALES["pseudo"], extra_scale=1.0):
    """The literal expression of :213-233, :257, :261 for one student under torch.autograd in ``dtype``: (out [6], dlogits).
    The head gradients enter as the linear term whose gradient they are."""
    z = own.to(dtype).clone().requires_grad_(True)
    zo = other.to(dtype)
    B, C = z.shape[0], z.shape[1]
    soft, soft_o = torch.softmax(z, dim=1), torch.softmax(zo, dim=1)

    def dice_loss(score, target):
        tot = 0.0
        for i in range(C):
            t = (target == i).to(dtype)
            s = score[:, i]
            tot = tot + (1 - (2 * torch.sum(s * t) + 1e-5) / (torch.sum(s * s) + torch.sum(t * t) + 1e-5))
        return tot / C

    ce = F.cross_entropy(z[:L].reshape(L, C, -1), label[:L].long().reshape(L, -1))
    dice = dice_loss(soft[:L], label[:L].reshape(soft[:L, 0].shape))
    ps = torch.zeros((), dtype=dtype)
    if B > L:
        ps = dice_loss(soft[L:], torch.argmax(soft_o[L:].detach(), dim=1))
    wt = torch.tensor(w, dtype=dtype)
    loss = sup_scale * 0.5 * (ce + dice) + pseudo_scale * wt * ps
    total = loss
    if extra_l is not None:
        total = total + extra_scale * (z[:L][0::2] * extra_l.to(dtype)).sum()
    if extra_u is not None:
        total = total + extra_scale * (z[L:] * extra_u.to(dtype)).sum()
    total.backward()
    out = torch.stack([loss.detach(), ce.detach(), dice.detach(), ps.detach(), wt, 0.5 * (ce + dice).detach() + wt * ps.detach()])
    return out, z.grad.detach()


def rel(a, ref):
    """|a - ref|max / |ref|max (0 when ref is all zero and a equals it)"""
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    scale = ref.abs().max().item()
    err = (a - ref).abs().max().item()
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


def scalar_rels(got, ref):
    return [rel(got[i], ref[i]) for i in range(len(ref))]


def reference_case(c):
    """(inputs, float64 out [6], float64 dlogits, scalar e32 list, tensor e32) of one case of the matrix."""
    x = inputs(c)
    own, other, label, el, eu = x
    w32 = float(torch.tensor(c["w"], dtype=torch.float32))
    sq = lambda t: None if t is None else t.squeeze(2).numpy()
    out64, d64 = student_tail(sq(own), sq(other), label.numpy(), c["L"], w32, extra_l=sq(el), extra_u=sq(eu))
    o32, d32 = tail_torch(own, other, label, c["L"], w32, torch.float32, el, eu)
    return x, out64, d64.reshape(own.shape), scalar_rels(o32, out64), rel(d32, d64.reshape(own.shape))
