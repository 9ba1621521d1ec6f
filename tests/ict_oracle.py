"""CPU restatement of one Interpolation Consistency Training iteration, for the ICT tests and golden generator.

Restates the loop body of code/train_interpolation_consistency_training_2D.py:150-190 (_3D.py:140-182,
_2D_ViT.py:190-235) on torch CPU fp32 with the oracle networks (oracle.nets / oracle.swin), the oracle losses and the
SGD / EMA / poly-LR rules of oracle.step.  The mix factors are an input (the reference draws them with
np.random.beta).  The teacher runs two train-mode forwards, on x0 and on x1: its BatchNorm running statistics are
updated twice, as in the reference.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle.losses import consistency_weight, dice_loss
from oracle.step import ema_alpha, lr_for_step


def ict_split(batch_size, labeled_bs):
    """M = labeled_bs // 2; ValueError unless labeled_bs >= 2 and the batch holds labeled_bs + 2M samples (the rule
    of mis_hip.step.ict_split, restated here so that the reference-side generator needs no product package)."""
    B, L = int(batch_size), int(labeled_bs)
    if L < 2:
        raise ValueError(f"ICT needs labeled_bs >= 2, got {L}")
    M = L // 2
    if B - L != 2 * M:
        raise ValueError(f"ICT needs batch_size - labeled_bs == {2 * M}, got batch_size={B}, labeled_bs={L}")
    return M


def ict_step(net, student, teacher, momentum, volume, label, mix_factors, iter_num, *, labeled_bs, num_classes,
             base_lr=0.01, max_iterations=30000, ema_decay=0.99, consistency=0.1, rampup=200.0, sgd_momentum=0.9,
             weight_decay=1e-4, drop_student=None, drop_teacher=None, apply_update=True):
    """One ICT iteration.  ``student``/``teacher``: state dicts (mutated in place), ``momentum``: SGD buffers (mutated;
    missing entries = first step), ``mix_factors``: the M = labeled_bs // 2 factors (any shape with M elements)."""
    L = labeled_bs
    M = ict_split(volume.shape[0], L)
    lam = mix_factors.reshape((M,) + (1,) * (volume.dim() - 1)).float()
    params = [n for n in student if net.is_param(n)]
    work = OrderedDict((n, t.detach().clone().requires_grad_(True)) if n in params else (n, t)
                       for n, t in student.items())
    x0, x1 = volume[L:L + M], volume[L + M:]
    mixed = x0 * (1.0 - lam) + x1 * lam
    inputs = torch.cat([volume[:L], mixed], dim=0)
    outputs = net.forward(work, inputs, training=True, drop=drop_student)
    outputs_soft = torch.softmax(outputs, dim=1)
    with torch.no_grad():
        t0 = net.forward(teacher, x0, training=True, drop=drop_teacher)
        t1 = net.forward(teacher, x1, training=True, drop=drop_teacher)
        target = torch.softmax(t0, dim=1) * (1.0 - lam) + torch.softmax(t1, dim=1) * lam
    loss_ce = F.cross_entropy(outputs[:L], label[:L].long())
    loss_dice = dice_loss(outputs_soft[:L], label[:L].unsqueeze(1), num_classes)
    supervised = 0.5 * (loss_dice + loss_ce)
    w = consistency_weight(iter_num, consistency, rampup)
    cons = torch.mean((outputs_soft[L:] - target) ** 2)
    loss = supervised + w * cons
    grads = torch.autograd.grad(loss, [work[n] for n in params], allow_unused=True)
    grads = OrderedDict((n, g if g is not None else torch.zeros_like(work[n])) for n, g in zip(params, grads))
    lr = lr_for_step(iter_num, base_lr, max_iterations)
    alpha = ema_alpha(iter_num, ema_decay)
    if apply_update:
        with torch.no_grad():
            for n in params:
                d = grads[n] + weight_decay * student[n]
                if n in momentum:
                    momentum[n].mul_(sgd_momentum).add_(d)
                else:
                    momentum[n] = d.clone()
                student[n].sub_(lr * momentum[n])
                teacher[n].mul_(alpha).add_(student[n], alpha=1 - alpha)
    return dict(loss=float(loss.detach()), loss_ce=float(loss_ce.detach()), loss_dice=float(loss_dice.detach()),
                consistency_loss=float(cons.detach()), consistency_weight=w, lr=lr, ema_alpha=alpha,
                mixed=inputs.detach(), logits=outputs.detach(), teacher_logits0=t0.detach(),
                teacher_logits1=t1.detach(), grads=grads)
