"""Triple-view training restated on torch CPU: the loop body (reference code/train_tripleview_2D(demo).py:290-354) over
the oracle networks, and the float64 autograd reference of its loss tail (mis_triple_view_tail).

Three students; student m is supervised on the labeled half and, on the unlabeled half, by the arg-max pseudo labels of
the other two (a, b), ascending: loss_m = 0.5 * (CE + Dice)(z_m[:L], y) + w * Dice(p_m[L:], y_a) + w * Dice(p_m[L:], y_b).
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

import loss_tail_oracle as lto
from oracle.losses import consistency_weight, dice_loss
from oracle.step import lr_for_step

PEERS = ((1, 2), (0, 2), (0, 1))


def triple_view_loss(zs, label, L, w, m):
    """The differentiable expression of student ``m``: (loss, ce, dice, pseudo_a, pseudo_b); ``zs``: the three logits, of
    which only zs[m] carries a gradient (the others are read through their arg-max)."""
    s = zs[m]
    B, C = s.shape[:2]
    ce, dice, _ = lto._supervised(s, label, L, C)
    ps = [s.sum() * 0, s.sum() * 0]
    if B > L:
        soft = torch.softmax(s[L:], 1)
        for k, j in enumerate(PEERS[m]):
            y = lto.argmax_first(zs[j][L:].detach(), 1)
            ps[k] = lto.dice_per_class(soft, y, C).mean()
    return 0.5 * (ce + dice) + w * ps[0] + w * ps[1], ce, dice, ps[0], ps[1]


def triple_view_tail(z1, z2, z3, label, L, w, dtype=torch.float64):
    """([out_1, out_2, out_3], [g_1, g_2, g_3]): out_m = [loss_m, ce, dice, pseudo_supervision_a, w, pseudo_supervision_b]
    (float64 tensors), g_m = d loss_m / d z_m.  The arg-max runs on the operands as given (fp32 values are exact in
    either dtype, so the pseudo labels do not depend on ``dtype``)."""
    zs = [lto._leaf(z, dtype) for z in (z1, z2, z3)]
    outs, grads = [], []
    for m in range(3):
        loss, ce, dice, pa, pb = triple_view_loss(zs, label, L, w, m)
        outs.append(lto._out(loss, ce, dice, pa, w, pb))
        grads.append(lto._grad(loss, zs[m], 1.0))
    return outs, grads


def triple_view_step(nets, sds, moms, volume, label, iter_num, *, labeled_bs, num_classes, base_lr=0.01,
                     max_iterations=30000, consistency=0.1, rampup=200.0, sgd_momentum=0.9, weight_decay=1e-4,
                     drops=("off", "off", "off"), apply_update=True):
    """One iteration over three oracle networks (``nets``), their state dicts (``sds``, mutated in place) and SGD momentum
    dicts (``moms``): three forwards, the six pseudo-supervision terms, one backward of loss1 + loss2 + loss3, three SGD
    steps; the learning rate in effect is the one computed before the previous increment of iter_num (:346-347)."""
    L = labeled_bs
    works, outs = [], []
    for net, sd, drop in zip(nets, sds, drops):
        work = OrderedDict((n, t.detach().clone().requires_grad_(True)) if net.is_param(n) else (n, t)
                           for n, t in sd.items())
        works.append(work)
        outs.append(net.forward(work, volume, training=True, drop=drop))
    soft = [torch.softmax(o, dim=1) for o in outs]
    pseudo = [torch.argmax(s[L:].detach(), dim=1, keepdim=False) for s in soft]
    w = consistency_weight(iter_num, consistency, rampup)
    losses, parts = [], []
    for m in range(3):
        ce = F.cross_entropy(outs[m][:L], label[:L].long())
        dl = dice_loss(soft[m][:L], label[:L].unsqueeze(1), num_classes)
        a, b = PEERS[m]
        pa = dice_loss(soft[m][L:], pseudo[a].unsqueeze(1), num_classes)
        pb = dice_loss(soft[m][L:], pseudo[b].unsqueeze(1), num_classes)
        losses.append(0.5 * (ce + dl) + w * pa + w * pb)
        parts.append((float(ce.detach()), float(dl.detach()), float(pa.detach()), float(pb.detach())))
    loss = losses[0] + losses[1] + losses[2]
    plist = [(m, n) for m, net in enumerate(nets) for n in works[m] if net.is_param(n)]
    grads = torch.autograd.grad(loss, [works[m][n] for m, n in plist])
    g = [OrderedDict(), OrderedDict(), OrderedDict()]
    for (m, n), gr in zip(plist, grads):
        g[m][n] = gr
    lr = lr_for_step(iter_num, base_lr, max_iterations, post_increment=True)
    if apply_update:
        with torch.no_grad():
            for sd, mom, gm in zip(sds, moms, g):
                for n, gr in gm.items():
                    d = gr + weight_decay * sd[n]
                    if n in mom:
                        mom[n].mul_(sgd_momentum).add_(d)
                    else:
                        mom[n] = d.clone()
                    sd[n].sub_(lr * mom[n])
    r = dict(loss=float(loss.detach()), parts=parts, consistency_weight=w, lr=lr, grads=g)
    for m in range(3):
        r[f"model{m + 1}_loss"] = float(losses[m].detach())
        r[f"logits{m + 1}"] = outs[m].detach()
    return r
