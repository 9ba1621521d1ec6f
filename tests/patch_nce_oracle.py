"""Reference arithmetic of the pixel-wise contrastive (PatchNCE) loss behind mis_patch_nce, utils.losses.ConLoss and
utils.losses.contrastive_loss_sup (reference code/utils/losses.py:283-337 and :479-531, the same arithmetic twice).

Plain torch (the tests evaluate it on the CPU; scripts/patch_nce_bench.py times the materialised form on the device), two
forms of one loss:

  materialised   the reference's own sequence: F.normalize(p = 1), the positive column by a batched [1, d] x [d, 1]
                 product, the [B, N, N] negatives by bmm with the diagonal filled with -inf, the concatenation divided by
                 the temperature, cross-entropy against column 0.
  rows           loss = mean_i (logsumexp_j s_ij - s_ii) with s_ij = q^_i . k^_j / T: the positive column plus the
                 diagonal-masked negatives are exactly the row {s_ij : all j}.  This is what the kernel computes.

Both take ``dtype``: float64 is the arbiter of the tests, float32 evaluates the same expression in fp32 and its distance
from the float64 evaluation is the yardstick of the GPU tests' tolerance (e32).  The gradient always comes from autograd
of the materialised form.  feat_k is detached, as in the reference.
"""
import torch
import torch.nn.functional as F


def _pixels(feat, dtype):
    """[B, d, *spatial] -> L1-normalised pixel vectors [B, N, d] (reference :304-307)."""
    B, d = feat.shape[0], feat.shape[1]
    return F.normalize(feat.to(dtype).reshape(B, d, -1).permute(0, 2, 1), dim=-1, p=1)


def materialised_loss(feat_q, feat_k, temperature=0.07, dtype=torch.float64):
    """The loss as the reference builds it (:299-337); differentiable in feat_q."""
    assert feat_q.size() == feat_k.size(), (feat_q.size(), feat_k.size())
    B, d = feat_q.shape[0], feat_q.shape[1]
    q = _pixels(feat_q, dtype)
    k = _pixels(feat_k, dtype).detach()
    l_pos = torch.bmm(q.reshape(-1, 1, d), k.reshape(-1, d, 1)).view(-1, 1)
    N = q.size(1)
    l_neg = torch.bmm(q, k.transpose(2, 1))
    l_neg = l_neg.masked_fill(torch.eye(N, dtype=torch.bool, device=q.device)[None, :, :], -float("inf")).view(-1, N)
    out = torch.cat((l_pos, l_neg), dim=1) / temperature
    return F.cross_entropy(out, torch.zeros(out.size(0), dtype=torch.long, device=q.device))


def rows_terms(feat_q, feat_k, temperature=0.07, dtype=torch.float64):
    """(loss, mean_i s_ii, mean_i logsumexp_j s_ij) of the row form: the layout of mis_patch_nce's ``out``."""
    assert feat_q.size() == feat_k.size(), (feat_q.size(), feat_k.size())
    q = _pixels(feat_q, dtype)
    k = _pixels(feat_k, dtype).detach()
    s = torch.bmm(q, k.transpose(2, 1)) / temperature
    lse = torch.logsumexp(s, dim=2)
    pos = torch.diagonal(s, dim1=1, dim2=2)
    return torch.stack([(lse - pos).mean(), pos.mean(), lse.mean()])


def rows_loss(feat_q, feat_k, temperature=0.07, dtype=torch.float64):
    return rows_terms(feat_q, feat_k, temperature, dtype)[0]


def loss_and_grad(feat_q, feat_k, temperature=0.07, dtype=torch.float64, grad_scale=1.0):
    """(out [3], grad_scale * d loss / d feat_q in feat_q's shape), both in ``dtype``.  out is the layout of
    mis_patch_nce's scalars: the loss and its gradient (autograd) from the materialised form, the two means the
    materialised form never forms (mean s_ii, mean logsumexp) from the row form."""
    fq = feat_q.detach().to(dtype).clone().requires_grad_(True)
    loss = materialised_loss(fq, feat_k, temperature, dtype)
    (loss * grad_scale).backward()
    with torch.no_grad():
        out = rows_terms(feat_q, feat_k, temperature, dtype)
        out[0] = loss.detach()
    return out, fq.grad.detach()
