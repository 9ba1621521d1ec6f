"""Triple-view step time against the cross-teaching step on the same batch, and the joint loss tail against the three
two-network tails it replaces.

    python scripts/triple_bench.py [--steps 10] [--warmup 4] [--no-kernels]

Prints ONE JSON line: ms per step of TripleViewTrainer (unet, unet, SwinUnet; 224 x 224, 8 + 8) and of CrossTeachingTrainer
(unet, SwinUnet) on the same synthetic batch, both measured in this process, and -- from a separate child run of this script
under ``rocprofv3 --kernel-trace --stats`` -- the device time per call of mis_triple_view_tail (pass 1, finalize, pass 2)
and of three mis_cross_pseudo_tail calls on the same logits (own, peer) = (1, 2), (2, 3), (3, 1): the cheapest thing the
existing kernels could do for three students, half of an exact composition.  The child alternates the two forms call by call
after a warm-up of each, so both see the same clocks and the same cache state (the 16 x 4 x 224 x 224 operands, 77 MB with
the gradients, stay resident in the 256 MB Infinity Cache for both).
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SP, B, L, C = (224, 224), 16, 8, 4
KERNELS = {           # kernel-name prefix -> reported operator
    "triple_pass1_kernel": "mis_triple_view_tail", "triple_final_kernel": "mis_triple_view_tail",
    "triple_pass2_kernel": "mis_triple_view_tail",
    "cross_pass1_kernel": "three_mis_cross_pseudo_tail", "cross_final_kernel": "three_mis_cross_pseudo_tail",
    "cross_pass2_kernel": "three_mis_cross_pseudo_tail",
}


def _batch():
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    vol = torch.rand((B, 1) + SP, generator=g, device="cuda")
    lab = torch.randint(0, C, (B,) + SP, generator=g, device="cuda").to(torch.uint8)
    return vol, lab


def time_trainer(kind, steps, warmup):
    import torch
    from config import lite_config
    from mis_hip.step import CrossTeachingTrainer, TripleViewTrainer
    from networks.net_factory import net_factory
    from networks.vision_transformer import SwinUnet
    vol, lab = _batch()
    unet = lambda: net_factory("unet", 1, C)
    swin = lambda: SwinUnet(lite_config(), img_size=SP[0], num_classes=C)
    models = [unet(), unet(), swin()] if kind == "triple" else [unet(), swin()]
    for m in models:
        m.train()
    cls = TripleViewTrainer if kind == "triple" else CrossTeachingTrainer
    tr = cls(*models, labeled_bs=L, num_classes=C, iter_num=1000, max_iterations=30000)
    for _ in range(warmup):                 # two eager steps, the recording, one replay
        tr.step(vol, lab)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(vol, lab)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    loss = tr.losses()["loss"]
    del tr, models
    torch.cuda.empty_cache()
    return dict(ms_per_step=round(ms, 3), samples_per_s=round(B * 1e3 / ms, 2), loss=loss)


def tail_child(reps):
    """``reps`` + 1 joint tails and ``reps`` + 1 triples of two-network tails on the same tensors, alternating."""
    import torch
    from mis_hip import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    zs = [torch.randn((B, C, 1) + SP, generator=g, device="cuda") * 3.0 for _ in range(3)]
    ds = [torch.empty_like(z) for z in zs]
    lab = torch.randint(0, C, (L, 1) + SP, generator=g, device="cuda").to(torch.uint8)
    outs = [torch.zeros(16, device="cuda") for _ in range(3)]
    for _ in range(reps + 1):
        ops.triple_view_tail(zs[0], zs[1], zs[2], lab, L, outs, dlogits=ds, cons_weight=0.05)
        for m in range(3):
            ops.cross_teaching_tail(zs[m], zs[(m + 1) % 3], lab, L, outs[m], dlogits=ds[m], cons_weight=0.05)
    torch.cuda.synchronize()


def kernel_times(reps, timeout):
    """Re-run this script under rocprofv3 (kernel trace); device us per call per operator."""
    out = tempfile.mkdtemp(prefix="triple_bench_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--kernel-child", "--steps", str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            return dict(error=f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}")
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return dict(error="no kernel trace written")
        per = {}
        for path in traces:
            for row in csv.DictReader(open(path)):
                name = re.sub(r"\(anonymous namespace\)::", "", row["Kernel_Name"])
                name = re.sub(r"^void ", "", name)
                for pre, op in KERNELS.items():
                    if name.startswith(pre):
                        t0, t1 = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                        per.setdefault((op, pre), []).append((t0, (t1 - t0) / 1e3))
        # the first call of each form is the warm-up: drop its launches (1 per kernel for the joint tail, 3 for the calls)
        res, tot = {}, {}
        for (op, pre), ts in sorted(per.items()):
            k = 1 if op == "mis_triple_view_tail" else 3
            ts = [dt for _, dt in sorted(ts)][k:]
            us = sum(ts) / reps
            res[pre + "_us"] = round(us, 2)
            tot[op] = tot.get(op, 0.0) + us
        for op, us in tot.items():
            res[op + "_us_per_step"] = round(us, 2)
        if len(tot) == 2:
            res["joint_over_three_calls"] = round(tot["mis_triple_view_tail"] / tot["three_mis_cross_pseudo_tail"], 4)
        res["shape"] = dict(B=B, L=L, C=C, S=SP[0] * SP[1], reps=reps)
        return res
    except subprocess.TimeoutExpired:
        return dict(error=f"rocprofv3 run exceeded {timeout} s")
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--kernel-timeout", type=int, default=300)
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    if a.kernel_child:
        tail_child(a.steps)
        return
    res = dict(metric="triple_view_vs_cross_teaching_step", steps=a.steps, warmup=a.warmup, batch_size=B, labeled_bs=L,
               spatial=list(SP))
    res["triple_view"] = time_trainer("triple", a.steps, a.warmup)
    res["cross_teaching"] = time_trainer("cross", a.steps, a.warmup)
    res["triple_over_cross"] = round(res["triple_view"]["ms_per_step"] / res["cross_teaching"]["ms_per_step"], 4)
    if not a.no_kernels:
        res["kernels"] = kernel_times(a.kernel_reps, a.kernel_timeout)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
