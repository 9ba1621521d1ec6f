"""One float64 autograd reference for the whole family of fused loss tails (mis_loss_tail, mis_cross_*_tail,
mis_uamt_tail, mis_softmax_mean_accumulate, mis_ict_tail, mis_dct_tail).

Written from the formulas of include/mis_hip.h and oracle/losses.py: plain torch on the CPU, ``float64`` throughout,
gradients by autograd.  Every function returns the scalars in the layout of its kernel's ``out`` vector (a float64
tensor) and d(loss * loss_scale)/d(logits).  ``dtype=torch.float32`` evaluates the same expression in fp32: the
distance of that evaluation from the float64 one is the yardstick of the GPU tests' tolerance (e32).

Shared pieces: sup = 0.5 * (CE + Dice) over the first L samples; Dice per class over all L*S voxels,
1 - (2 I + 1e-5) / (Z + Y + 1e-5), averaged over the classes; class-wise dice score = 1 - dice_loss_c.
"""
import math

import torch
import torch.nn.functional as F

SMOOTH = 1e-5
LN2 = 0.6931471805599453


def argmax_first(x, dim=1):
    """Index of the FIRST maximum along ``dim`` (a later value wins only when strictly greater; -0.0 == +0.0)."""
    best = x.select(dim, 0).clone()
    idx = torch.zeros(best.shape, dtype=torch.int64)
    for c in range(1, x.shape[dim]):
        v = x.select(dim, c)
        m = v > best
        idx[m] = c
        best = torch.where(m, v, best)
    return idx


def dice_score_per_class(probs, target, C):
    """[C] dice scores (2 I + 1e-5) / (Z + Y + 1e-5); probs [N, C, ...], target [N, ...] integer; sums over batch and
    space.  The score is formed directly, not as 1 - (1 - score): for a class that never occurs it is ~1e-9, which the
    double subtraction would round away in the fp32 evaluation."""
    out = []
    for c in range(C):
        p = probs[:, c]
        t = (target == c).to(probs.dtype)
        out.append((2 * torch.sum(p * t) + SMOOTH) / (torch.sum(p * p) + torch.sum(t) + SMOOTH))
    return torch.stack(out)


def dice_per_class(probs, target, C):
    """[C] dice losses 1 - score."""
    return 1 - dice_score_per_class(probs, target, C)


def _leaf(x, dtype):
    return x.detach().to(dtype).clone().requires_grad_(True)


def _supervised(logits, label, L, C):
    """(ce, dice, [C] class-wise dice scores) of the first L samples; all zero / one without labeled samples."""
    zero = logits.sum() * 0
    if L == 0:
        return zero, zero, torch.ones(C, dtype=logits.dtype)
    lab = label[:L].long()
    ce = F.cross_entropy(logits[:L], lab)
    score = dice_score_per_class(torch.softmax(logits[:L], 1), lab, C)
    return ce, (1 - score).mean(), score


def _grad(loss, leaf, loss_scale):
    (g,) = torch.autograd.grad(loss * loss_scale, [leaf], allow_unused=True)
    return torch.zeros_like(leaf) if g is None else g


def _out(*vals):
    flat = []
    for v in vals:
        if torch.is_tensor(v):
            flat.extend(v.detach().double().reshape(-1).tolist())
        else:
            flat.append(float(v))
    return torch.tensor(flat, dtype=torch.float64)


def mean_teacher_tail(student, teacher, label, L, w, gate=1.0, loss_scale=1.0, dtype=torch.float64):
    """out = [loss, ce, dice, consistency, w, C class-wise dice]; + w * gate * mean((softmax(s[L:]) - softmax(t))^2)."""
    s = _leaf(student, dtype)
    loss, ce, dice, cons, scores = mean_teacher_loss(s, teacher, label, L, w, gate)
    return _out(loss, ce, dice, cons, w, scores), _grad(loss, s, loss_scale)


def mean_teacher_loss(s, teacher, label, L, w, gate=1.0):
    """The differentiable expression behind mean_teacher_tail: (loss, ce, dice, consistency, scores) of logits ``s``."""
    B, C = s.shape[:2]
    ce, dice, scores = _supervised(s, label, L, C)
    cons = s.sum() * 0
    if B > L and gate != 0:
        cons = torch.mean((torch.softmax(s[L:], 1) - torch.softmax(teacher.to(s.dtype), 1)) ** 2)
    return 0.5 * (ce + dice) + w * cons, ce, dice, cons, scores


def cross_tail(own, other, label, L, w, pseudo_ce=False, teacher=None, mt_weight=0.0, loss_scale=1.0,
               dtype=torch.float64):
    """out = [loss, ce, dice, pseudo_supervision, w] (+ [mse, mt_weight] with a teacher); the pseudo labels are the
    first-maximum arg-max of the other network's logits on the unlabeled rows."""
    s = _leaf(own, dtype)
    loss, ce, dice, pseudo, mse = cross_loss(s, other, label, L, w, pseudo_ce, teacher, mt_weight)
    if teacher is None:
        return _out(loss, ce, dice, pseudo, w), _grad(loss, s, loss_scale)
    return _out(loss, ce, dice, pseudo, w, mse, mt_weight), _grad(loss, s, loss_scale)


def cross_loss(s, other, label, L, w, pseudo_ce=False, teacher=None, mt_weight=0.0):
    """The differentiable expression behind cross_tail: (loss, ce, dice, pseudo_supervision, mse) of logits ``s``."""
    B, C = s.shape[:2]
    ce, dice, _ = _supervised(s, label, L, C)
    pseudo = s.sum() * 0
    mse = s.sum() * 0
    if B > L:
        y = argmax_first(other[L:], 1)
        if pseudo_ce:
            pseudo = F.cross_entropy(s[L:], y)
        else:
            pseudo = dice_per_class(torch.softmax(s[L:], 1), y, C).mean()
        if teacher is not None:
            mse = torch.mean((torch.softmax(s[L:], 1) - torch.softmax(teacher.to(s.dtype), 1)) ** 2)
    loss = 0.5 * (ce + dice) + w * pseudo
    if teacher is not None:
        loss = loss + mt_weight * mse
    return loss, ce, dice, pseudo, mse


def uamt_threshold(iter_num, max_iterations):
    cur = min(max(float(iter_num), 0.0), float(max_iterations))
    ramp = 1.0 if max_iterations == 0 else math.exp(-5.0 * (1.0 - cur / max_iterations) ** 2)
    return (0.75 + 0.25 * ramp) * LN2


def uamt_entropy(mean_probs):
    """float64 entropy of the exact values of ``mean_probs`` (an fp32 tensor): -sum_c pm * log(pm + 1e-6)."""
    pm = mean_probs.double()
    return -(pm * torch.log(pm + 1e-6)).sum(1)


def uamt_undecided(mean_probs, thr, band=1e-5):
    """Voxels whose entropy lies within ``band`` of the threshold: an fp32 kernel may decide them either way."""
    return (uamt_entropy(mean_probs) - thr).abs() < band


def uamt_mean_probs(U, C, spatial, thr, generator, scale=3.0, passes=8):
    """fp32 mean of ``passes`` correlated MC-dropout-like softmaxes [U, C, *spatial]; every voxel within 1e-5 of the
    threshold is replaced by a clearly decided near-one-hot row, so that the mask is the same in any precision."""
    base = torch.randn((U, C) + tuple(spatial), generator=generator) * scale
    pm = torch.zeros_like(base)
    for _ in range(passes):
        pm += torch.softmax(base + torch.randn(base.shape, generator=generator) * (0.5 * scale), 1) / passes
    und = uamt_undecided(pm, thr).unsqueeze(1).expand_as(pm)
    hot = torch.full_like(pm, 1e-3)
    hot[:, 0] = 1.0 - (C - 1) * 1e-3
    return torch.where(und, hot, pm).float()


def uamt_tail(student, teacher, mean_probs, label, L, w, iter_num, max_iterations, loss_scale=1.0,
              dtype=torch.float64):
    """out = [loss, ce, dice, consistency, w, C class-wise dice, mask count, thr]; consistency =
    sum(mask * (softmax(s[L:]) - softmax(t))^2) / (2 * sum(mask) + 1e-16), mask = entropy(mean_probs) < thr."""
    s = _leaf(student, dtype)
    loss, ce, dice, cons, scores, count, thr = uamt_loss(s, teacher, mean_probs, label, L, w, iter_num, max_iterations)
    return _out(loss, ce, dice, cons, w, scores, count, thr), _grad(loss, s, loss_scale)


def uamt_loss(s, teacher, mean_probs, label, L, w, iter_num, max_iterations):
    """The differentiable expression behind uamt_tail: (loss, ce, dice, consistency, scores, mask count, thr)."""
    C = s.shape[1]
    ce, dice, scores = _supervised(s, label, L, C)
    thr = uamt_threshold(iter_num, max_iterations)
    pm = mean_probs.to(s.dtype)
    mask = (-(pm * torch.log(pm + 1e-6)).sum(1, keepdim=True) < thr).to(s.dtype)
    dist = (torch.softmax(s[L:], 1) - torch.softmax(teacher.to(s.dtype), 1)) ** 2
    cons = torch.sum(mask * dist) / (2 * torch.sum(mask) + 1e-16)
    return 0.5 * (ce + dice) + w * cons, ce, dice, cons, scores, mask.sum(), thr


def ict_tail(student, teacher0, teacher1, lam, label, L, w, gate=1.0, loss_scale=1.0, dtype=torch.float64):
    """out = [loss, ce, dice, consistency, w, C class-wise dice]; target = softmax(t0) * (1 - lam) + softmax(t1) * lam."""
    s = _leaf(student, dtype)
    loss, ce, dice, cons, scores = ict_loss(s, teacher0, teacher1, lam, label, L, w, gate)
    return _out(loss, ce, dice, cons, w, scores), _grad(loss, s, loss_scale)


def ict_loss(s, teacher0, teacher1, lam, label, L, w, gate=1.0):
    """The differentiable expression behind ict_tail: (loss, ce, dice, consistency, scores) of logits ``s``."""
    B, C = s.shape[:2]
    ce, dice, scores = _supervised(s, label, L, C)
    cons = s.sum() * 0
    if B > L and gate != 0:
        l = lam.to(s.dtype).reshape((-1,) + (1,) * (s.dim() - 1))
        target = torch.softmax(teacher0.to(s.dtype), 1) * (1.0 - l) + torch.softmax(teacher1.to(s.dtype), 1) * l
        cons = torch.mean((torch.softmax(s[L:], 1) - target) ** 2)
    return 0.5 * (ce + dice) + w * cons, ce, dice, cons, scores


def dct_tail(logits_a, logits_r, label, L, k, w, gate=1.0, loss_scale=1.0, dtype=torch.float64):
    """Deep co-training over pass A [L+U, C, H, W] and pass R [U, C, H, W]: out = [loss, ce, dice, consistency, w, k,
    C class-wise dice]; consistency = 0.5 * (mean((Q.detach() - rot P)^2) + mean((Q - rot P.detach())^2)).
    Returns (out, dA, dR)."""
    a, r = _leaf(logits_a, dtype), _leaf(logits_r, dtype)
    loss, ce, dice, cons, scores = dct_loss(a, r, label, L, k, w, gate)
    ga, gr = torch.autograd.grad(loss * loss_scale, [a, r], allow_unused=True)
    ga = torch.zeros_like(a) if ga is None else ga
    gr = torch.zeros_like(r) if gr is None else gr
    return _out(loss, ce, dice, cons, w, k, scores), ga, gr


def dct_loss(a, r, label, L, k, w, gate=1.0):
    """The differentiable expression behind dct_tail: (loss, ce, dice, consistency, scores) of both passes' logits."""
    C = a.shape[1]
    ce, dice, scores = _supervised(a, label, L, C)
    cons = a.sum() * 0
    if gate != 0:
        q = torch.softmax(r, 1)
        rp = torch.rot90(torch.softmax(a[L:], 1), k, [2, 3])
        cons = 0.5 * (torch.mean((q.detach() - rp) ** 2) + torch.mean((q - rp.detach()) ** 2))
    return 0.5 * (ce + dice) + w * cons, ce, dice, cons, scores


def softmax_mean_accumulate(logits, acc, repeats, scale, first, dtype=torch.float64):
    """acc[u] = (0 if first else acc[u]) + scale * sum_r softmax(logits[r * U + u]); returns the new acc."""
    U = logits.shape[0] // repeats
    p = torch.softmax(logits.to(dtype), 1).reshape((repeats, U) + tuple(logits.shape[1:])).sum(0)
    prev = torch.zeros_like(p) if first else acc.to(dtype)
    return prev + scale * p
