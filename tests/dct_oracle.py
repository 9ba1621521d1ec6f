"""CPU restatement of one deep co-training iteration, for the deep co-training tests and golden generator.

Restates the loop body of code/train_deep_co_training_2D.py:134-167 (_2D_ViT.py:172-205) on torch CPU fp32 with the
oracle networks (oracle.nets / oracle.swin), the oracle losses and the poly-LR rule of oracle.step.  The rotation count is
an input (the reference draws it with random.randrange(0, 4)).  The one network runs two train-mode forwards, on the batch
and on its rotated unlabeled part: BatchNorm running statistics are updated twice, and autograd sums the gradient of both.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle.losses import consistency_weight, dice_loss
from oracle.step import lr_for_step

# flag names of code/train_deep_co_training_2D_ViT.py; the triple-view script takes the same ones (tests/test_triple_cpu.py)
REF_FLAGS_VIT = ["--root_path", "--exp", "--model", "--max_iterations", "--batch_size", "--deterministic", "--base_lr",
                 "--patch_size", "--seed", "--num_classes", "--cfg", "--opts", "--zip", "--cache-mode", "--resume",
                 "--accumulation-steps", "--use-checkpoint", "--amp-opt-level", "--tag", "--eval", "--throughput",
                 "--labeled_bs", "--labeled_num", "--ema_decay", "--consistency_type", "--consistency",
                 "--consistency_rampup"]


def dct_step(net, student, momentum, volume, label, rot_k, iter_num, *, labeled_bs, num_classes, base_lr=0.01,
             max_iterations=30000, consistency=0.1, rampup=200.0, sgd_momentum=0.9, weight_decay=1e-4, drop=None,
             apply_update=True):
    """One deep co-training iteration.  ``student``: state dict (mutated in place: SGD and the running statistics),
    ``momentum``: SGD buffers (mutated; missing entries = first step)."""
    L = labeled_bs
    params = [n for n in student if net.is_param(n)]
    work = OrderedDict((n, t.detach().clone().requires_grad_(True)) if n in params else (n, t)
                       for n, t in student.items())
    outputs = net.forward(work, volume, training=True, drop=drop)
    outputs_soft = torch.softmax(outputs, dim=1)
    rotated = torch.rot90(volume[L:], rot_k, [2, 3])
    rot_outputs = net.forward(work, rotated, training=True, drop=drop)
    rot_soft = torch.softmax(rot_outputs, dim=1)
    loss_ce = F.cross_entropy(outputs[:L], label[:L].long())
    loss_dice = dice_loss(outputs_soft[:L], label[:L].unsqueeze(1), num_classes)
    supervised = 0.5 * (loss_dice + loss_ce)
    w = consistency_weight(iter_num, consistency, rampup)
    rot_p = torch.rot90(outputs_soft[L:], rot_k, [2, 3])
    cons = 0.5 * (torch.mean((rot_soft.detach() - rot_p) ** 2) + torch.mean((rot_soft - rot_p.detach()) ** 2))
    loss = supervised + w * cons
    grads = torch.autograd.grad(loss, [work[n] for n in params], allow_unused=True)
    grads = OrderedDict((n, g if g is not None else torch.zeros_like(work[n])) for n, g in zip(params, grads))
    lr = lr_for_step(iter_num, base_lr, max_iterations)
    if apply_update:
        with torch.no_grad():
            for n in params:
                d = grads[n] + weight_decay * student[n]
                if n in momentum:
                    momentum[n].mul_(sgd_momentum).add_(d)
                else:
                    momentum[n] = d.clone()
                student[n].sub_(lr * momentum[n])
    return dict(loss=float(loss.detach()), loss_ce=float(loss_ce.detach()), loss_dice=float(loss_dice.detach()),
                consistency_loss=float(cons.detach()), consistency_weight=w, lr=lr, rotated=rotated,
                logits=outputs.detach(), rot_logits=rot_outputs.detach(), grads=grads)
