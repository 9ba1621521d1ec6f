"""FixMatch on an MI355X: the fused loss tail against the same loss and gradient written with torch ops, the colour
jitter, and the full ``unet`` step, all in this process on one GPU.

    python scripts/fixmatch_bench.py [--iters 200] [--steps 20] [--warmup 5] [--out profiles/fixmatch_bench.json]

Shapes: logits [24, 4, 256, 256], labeled_bs 12 (the reference's default batch).  Times are device-event times per call
over ``--iters`` back-to-back calls after a warm-up (the step: a host clock around ``--steps`` steps ending in a device
synchronise).  The torch version is the literal reference expression (tests/fixmatch_oracle.reference_autograd's
arithmetic: softmax, the min-max mask, CrossEntropyLoss, DiceLoss, ``Categorical(probs=...).entropy()``) on the device in
fp32 with ``loss.backward()`` to both logits tensors.

Byte floor of the tail (the passes DESIGN.md lists; N = B * C * S logits of 4 bytes, labels 1 byte):
    pass 1 reads 2N (weak + strong) + the labels, pass 2 reads N (strong), the gradient pass reads 2N + the labels and
    writes 2N: 7N * 4 bytes + 2 * L * S.  ``floor_us`` is that over the 8.0 TB/s HBM3E peak; ``fraction_of_floor`` =
    floor_us / measured.  Partials and per-sample sums are KBs and are left out.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

B, L, C, H, W = 24, 12, 4, 256, 256
HBM_PEAK = 8.0e12


def event_us(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def torch_tail(zw, zs, label, tau, w):
    """The reference's loss (train_Fixmatch_CNN_2D.py:132-166, :259-288) with torch ops; returns the loss tensor."""
    import torch
    from torch.distributions import Categorical
    S = H * W
    ce = torch.nn.CrossEntropyLoss()

    def dice(p, t):
        loss = 0.0
        for i in range(C):
            ti = (t == i).float()
            pi = p[:, i]
            loss = loss + (1 - (2 * torch.sum(pi * ti) + 1e-5) / (torch.sum(pi * pi) + torch.sum(ti * ti) + 1e-5))
        return loss / C

    pw, ps = torch.softmax(zw, 1), torch.softmax(zs, 1)
    n = (pw - pw.min(1, keepdim=True)[0]) / pw.max(1, keepdim=True)[0]
    pseudo = torch.argmax((pw * (n > tau).float())[L:].detach(), dim=1)
    sup = ce(zw[:L], label.long()) + dice(pw[:L], label)
    a = torch.mean(1 - Categorical(probs=ps.reshape(B, C, S), validate_args=False).entropy() / math.log(S))
    comp = torch.argmin(pw.detach(), dim=1)
    comp_loss = a * ce(1 - ps, comp)
    unsup = ce(zs[L:], pseudo) + dice(ps[L:], pseudo) + a * comp_loss
    return sup + w * unsup


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixmatch_bench.json"))
    a = ap.parse_args()
    import torch
    from mis_hip import lib, ops
    from mis_hip.step import FixMatchTrainer
    from networks.net_factory import net_factory
    assert torch.cuda.is_available(), "fixmatch_bench.py measures on the GPU; there is no CPU path"
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    zw = torch.randn((B, C, 1, H, W), generator=g, device="cuda") * 3
    zs = torch.randn((B, C, 1, H, W), generator=g, device="cuda") * 3
    label = torch.randint(0, C, (L, H, W), generator=g, device="cuda").to(torch.uint8)
    vol = torch.rand((B, 1, H, W), generator=g, device="cuda")
    lab = torch.randint(0, C, (B, H, W), generator=g, device="cuda").to(torch.uint8)
    out = torch.zeros(16, device="cuda")
    dw, ds = torch.empty_like(zw), torch.empty_like(zs)
    w, tau = 0.05, 0.8

    def taped(call):
        """The call as a launch tape (what a training step replays): the host then costs a ctypes call per launch and the
        events time the device, not Python."""
        call()
        tape = lib.LaunchTape()
        with tape.recording():
            call()
        return tape.replay

    tail_us = event_us(taped(lambda: ops.fixmatch_tail(zw, zs, label, L, out, d_weak=dw, d_strong=ds, conf_thresh=tau,
                                                       cons_weight=w)), a.iters, a.warmup)
    fwd_us = event_us(taped(lambda: ops.fixmatch_tail(zw, zs, label, L, out, conf_thresh=tau, cons_weight=w)), a.iters,
                      a.warmup)

    zw4 = zw[:, :, 0].clone().requires_grad_(True)
    zs4 = zs[:, :, 0].clone().requires_grad_(True)

    def torch_call():
        zw4.grad = zs4.grad = None
        torch_tail(zw4, zs4, label, tau, w).backward()

    torch_us = event_us(torch_call, max(a.iters // 10, 5), 2)
    # same loss, same gradients (continuous logits: the few pixels fp32 decides differently stay below this bound)
    loss_t = torch_tail(zw4, zs4, label, tau, w).item()
    ops.fixmatch_tail(zw, zs, label, L, out, d_weak=dw, d_strong=ds, conf_thresh=tau, cons_weight=w)
    agree = dict(loss_hip=out[0].item(), loss_torch=loss_t,
                 d_strong_rel=((ds[:, :, 0] - zs4.grad).abs().max() / zs4.grad.abs().max()).item(),
                 d_weak_rel=((dw[:, :, 0] - zw4.grad).abs().max() / zw4.grad.abs().max()).item())

    strong = torch.empty_like(vol)
    params = torch.tensor([[1.3, 0.7, b % 2] for b in range(B)], dtype=torch.float32, device="cuda")
    jitter_us = event_us(taped(lambda: ops.color_jitter(vol, strong, params=params)), a.iters, a.warmup)

    model, ema = net_factory("unet", 1, C), net_factory("unet", 1, C)
    model.train()
    ema.train()
    tr = FixMatchTrainer(model, ema, labeled_bs=L, num_classes=C, iter_num=1000, max_iterations=30000)
    for _ in range(a.warmup):
        tr.step(vol, lab)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        tr.step(vol, lab)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / a.steps

    N = B * C * H * W
    tail_bytes = 7 * N * 4 + 2 * L * H * W
    floor_us = tail_bytes / HBM_PEAK * 1e6
    jitter_bytes = 3 * B * H * W * 4           # the sum pass reads the batch, the apply pass reads and writes it
    res = dict(metric="fixmatch", shape=[B, C, H, W], labeled_bs=L, iters=a.iters,
               tail=dict(us=round(tail_us, 2), forward_only_us=round(fwd_us, 2), bytes=tail_bytes, floor_us=round(floor_us, 2),
                         fraction_of_floor=round(floor_us / tail_us, 4), launches=6),
               torch_ops=dict(us=round(torch_us, 2), over_tail=round(torch_us / tail_us, 2)),
               agreement=agree,
               jitter=dict(us=round(jitter_us, 2), bytes=jitter_bytes, floor_us=round(jitter_bytes / HBM_PEAK * 1e6, 2),
                           fraction_of_floor=round(jitter_bytes / HBM_PEAK * 1e6 / jitter_us, 4), launches=2),
               step=dict(model="unet", ms_per_step=round(step_ms, 3), samples_per_s=round(B * 1e3 / step_ms, 2),
                         steps=a.steps, taped=tr._tape is not None, loss=tr.losses()["loss"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
