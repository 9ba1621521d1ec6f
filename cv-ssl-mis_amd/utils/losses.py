"""``utils.losses`` surface of the reference on HIP kernels (code/utils/losses.py).

The two losses on the Mean-Teacher hot path, ``DiceLoss`` (:165-201) and ``softmax_mse_loss`` (:74-91), and the
pixel-wise contrastive loss of the contrastive trainers, ``ConLoss`` (:283-337) / ``contrastive_loss_sup`` (:479-531).
All are autograd-aware and run on the device through the C-ABI (``mis_dice_loss_*`` / ``mis_softmax_mse`` /
``mis_patch_nce``); there is no CPU implementation here.  The fused training step (``mis_hip.step``) does not call
these -- it uses the single-pass fused loss tail instead.
"""
import torch
import torch.nn as nn

from mis_hip import lib as _l
from mis_hip import ops as _ops


def _as3(t):
    """[B, C, *spatial] -> (B, C, S, batch stride) for dense-in-(C,S) tensors."""
    _l.require_gpu(t)
    if t.dtype != torch.float32:
        raise RuntimeError("expected fp32")
    t = t if t.is_contiguous() else t.contiguous()
    B, C = t.shape[0], t.shape[1]
    S = t[0, 0].numel()
    return t, B, C, S, C * S


class _DiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, probs, label, weight):
        probs, B, C, S, bs = _as3(probs)
        label = label.contiguous()
        lb = 1 if label.dtype == torch.uint8 else 8
        if label.dtype not in (torch.uint8, torch.int64):
            label, lb = label.long(), 8
        ws = torch.empty(_l.query("mis_dice_workspace_bytes", B, C, S), dtype=torch.uint8, device=probs.device)
        out = torch.empty(1 + C, dtype=torch.float32, device=probs.device)
        _l.launch("mis_dice_loss_fwd", probs, bs, label, lb, B, C, S, weight, out, ws, ws.numel())
        ctx.save_for_backward(probs, label, ws)
        ctx.geo = (B, C, S, bs, lb)
        return out[0], out[1:]

    @staticmethod
    def backward(ctx, gloss, _gdice):
        probs, label, ws = ctx.saved_tensors
        B, C, S, bs, lb = ctx.geo
        dp = torch.empty_like(probs)
        g = gloss.reshape(1).contiguous().float()
        _l.launch("mis_dice_loss_bwd", probs, bs, label, lb, B, C, S, ws, g, dp, bs)
        return dp, None, None


class DiceLoss(nn.Module):
    """Drop-in for ``losses.DiceLoss`` (code/utils/losses.py:165-201)."""

    def __init__(self, n_classes):
        super().__init__()
        self.n_classes = n_classes

    def forward(self, inputs, target, weight=None, softmax=False):
        if softmax:
            inputs = torch.softmax(inputs, dim=1)
        # reference: assert inputs.size() == one-hot(target).size()  (:194)
        assert inputs.shape[1] == self.n_classes and tuple(inputs.shape[2:]) == tuple(target.shape[2:]) and \
            target.shape[1] == 1 and inputs.shape[0] == target.shape[0], 'predict & target shape do not match'
        w = None
        if weight is not None:
            w = torch.as_tensor(weight, dtype=torch.float32, device=inputs.device)
        loss, _class_wise_dice = _DiceFn.apply(inputs, target[:, 0], w)
        return loss


class _SoftmaxMseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, B, C, S, bs = _as3(a)
        b, _, _, _, _ = _as3(b)
        out = torch.empty_like(a)
        _l.launch("mis_softmax_mse", a, bs, b, bs, None, 0, out, bs, B, C, S, 0)
        ctx.save_for_backward(a, b)
        ctx.geo = (B, C, S, bs)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        B, C, S, bs = ctx.geo
        g = g.contiguous()
        da = torch.empty_like(a)
        _l.launch("mis_softmax_mse", a, bs, b, bs, g, bs, da, bs, B, C, S, 1)
        return da, None   # "Sends gradients to inputs but not the targets" (losses.py:79)


def softmax_mse_loss(input_logits, target_logits, sigmoid=False):
    """Un-reduced (softmax(input) - softmax(target))**2  (code/utils/losses.py:74-91)."""
    assert input_logits.size() == target_logits.size()
    if sigmoid:
        raise NotImplementedError("sigmoid=True is not on the Mean-Teacher hot path")
    return _SoftmaxMseFn.apply(input_logits, target_logits.detach())


class _PatchNceFn(torch.autograd.Function):
    """One ``mis_patch_nce`` call in the forward: the loss and d loss / d feat_q come from the same walk over the keys, so
    the backward only scales the kept gradient by the upstream scalar."""

    @staticmethod
    def forward(ctx, feat_q, feat_k, temperature):
        out = torch.empty(3, dtype=torch.float32, device=feat_q.device)
        dfeat = torch.empty_like(feat_q) if ctx.needs_input_grad[0] else None
        _ops.patch_nce(feat_q, feat_k, out, dfeat=dfeat, temperature=temperature)
        ctx.save_for_backward(dfeat)
        return out[0].clone()

    @staticmethod
    def backward(ctx, gloss):
        dfeat, = ctx.saved_tensors
        # feat_k is detached in the reference (:308); dfeat is None when only feat_k asked for a gradient
        return (None if dfeat is None else dfeat * gloss), None, None


def _patch_nce_loss(feat_q, feat_k, temperature):
    assert feat_q.size() == feat_k.size(), (feat_q.size(), feat_k.size())
    _l.require_gpu(feat_q, feat_k)
    if feat_q.dtype != torch.float32 or feat_k.dtype != torch.float32 or feat_q.dim() < 3 or \
            feat_q.shape[1] not in _ops.PATCH_NCE_DIMS:
        raise RuntimeError(f"contrastive loss: expected fp32 [B, d, *spatial] features with d in {_ops.PATCH_NCE_DIMS} "
                           f"(supported dims), got {tuple(feat_q.shape)} {feat_q.dtype} / {feat_k.dtype}")
    return _PatchNceFn.apply(feat_q.contiguous(), feat_k.detach().contiguous(), float(temperature))


class ConLoss(nn.Module):
    """Drop-in for ``losses.ConLoss`` (code/utils/losses.py:283-337): PatchNCE over every pixel pair of one sample's
    feature map, the negatives of a pixel being the other pixels of the same sample.  No [B, N, N] tensor is built."""

    def __init__(self, temperature=0.07, base_temperature=0.07):
        super().__init__()
        self.temperature = temperature
        self.base_temperature = base_temperature      # kept for the signature: the reference never reads it

    def forward(self, feat_q, feat_k):
        return _patch_nce_loss(feat_q, feat_k, self.temperature)


class contrastive_loss_sup(ConLoss):
    """Drop-in for ``losses.contrastive_loss_sup`` (code/utils/losses.py:479-531, the definition in force): the same
    arithmetic as ``ConLoss``."""


def update_ema_variables(model, ema_model, alpha, global_step):
    """reference train_mean_teacher_2D.py:124-128 -- one flat kernel instead of 2 launches per tensor."""
    alpha = min(1 - 1 / (global_step + 1), alpha)
    _l.launch("mis_ema_update", ema_model.flat_param, model.flat_param, model.flat_param.numel(), alpha)
