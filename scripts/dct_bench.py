"""Deep co-training step time against the Mean-Teacher step on the same batch.

    python scripts/dct_bench.py [--steps 10] [--warmup 3] [--configs unet2d_256,swin_224] [--no-kernels]

Prints ONE JSON line: per configuration the deep co-training and the MT step (ms per step, samples per second counting the
B samples drawn per step), both measured in this process on the same synthetic batch, and -- from a separate child run of
this script under ``rocprofv3 --kernel-trace --stats`` on the unet2d_256 configuration -- the device time per step of the
deep co-training operators (mis_dct_tail = labeled pass 1, consistency pass 1, finalize, labeled pass 2, consistency
pass 2; mis_rot90; mis_grad_combine, two per step) and of mis_loss_tail of the MT step.
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

# name: (factory, spatial, batch_size, labeled_bs, num_classes) -- the reference's default batches
CONFIGS = {
    "unet2d_256": ("unet", (256, 256), 24, 12, 4),
    "swin_224": ("ViT_Seg", (224, 224), 24, 7, 4),
}
KERNELS = {           # kernel-name prefix -> reported operator
    "dct_lab1_kernel": "mis_dct_tail", "dct_cons_kernel": "mis_dct_tail", "dct_final_kernel": "mis_dct_tail",
    "dct_lab2_kernel": "mis_dct_tail", "rot90_kernel": "mis_rot90", "grad_combine4_kernel": "mis_grad_combine",
    "grad_combine1_kernel": "mis_grad_combine",
    "tail_pass1_kernel": "mis_loss_tail", "tail_final_kernel": "mis_loss_tail", "tail_pass2_kernel": "mis_loss_tail",
}


def time_trainer(kind, cfg, steps, warmup):
    import torch
    from networks.net_factory import net_factory
    from mis_hip.step import DeepCoTrainingTrainer, MeanTeacherTrainer
    factory, sp, B, L, C = cfg
    g = torch.Generator(device="cuda").manual_seed(0)
    vol = torch.rand((B, 1) + sp, generator=g, device="cuda")
    lab = torch.randint(0, C, (B,) + sp, generator=g, device="cuda").to(torch.uint8)
    model = net_factory(factory, 1, C)
    model.train()
    if kind == "dct":
        tr = DeepCoTrainingTrainer(model, labeled_bs=L, num_classes=C, iter_num=1000, max_iterations=30000)
    else:
        ema = net_factory(factory, 1, C)
        for p in ema.parameters():
            p.detach_()
        ema.train()
        tr = MeanTeacherTrainer(model, ema, labeled_bs=L, num_classes=C, iter_num=1000, max_iterations=30000)
    for _ in range(warmup):
        tr.step(vol, lab)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(vol, lab)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    loss = tr.losses()["loss"]
    del tr, model
    torch.cuda.empty_cache()
    return dict(ms_per_step=round(ms, 3), samples_per_s=round(B * 1e3 / ms, 2), loss=loss)


def kernel_times(steps, timeout):
    """Re-run this script under rocprofv3 (kernel trace) for unet2d_256; device us per step per operator."""
    out = tempfile.mkdtemp(prefix="dct_bench_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--kernel-child", "--steps", str(steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            return dict(error=f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}")
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return dict(error="no kernel trace written")
        tot, step_us = {}, {"dct": 0.0, "mt": 0.0}
        for path in traces:
            for row in csv.DictReader(open(path)):
                name = re.sub(r"\(anonymous namespace\)::", "", row["Kernel_Name"])
                name = re.sub(r"^void ", "", name)
                for pre, op in KERNELS.items():
                    if name.startswith(pre):
                        dt = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
                        tot[op] = tot.get(op, 0.0) + dt
        # the child runs `steps` deep co-training steps and `steps` MT steps after one warm-up step of each
        res = {op + "_us_per_step": round(t / (steps + 1), 2) for op, t in sorted(tot.items())}
        res["config"] = "unet2d_256"
        return res
    except subprocess.TimeoutExpired:
        return dict(error=f"rocprofv3 run exceeded {timeout} s")
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--kernel-timeout", type=int, default=600)
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    if a.kernel_child:
        for kind in ("dct", "mt"):
            time_trainer(kind, CONFIGS["unet2d_256"], a.steps, 1)
        return
    res = dict(metric="dct_vs_mt_step", steps=a.steps, warmup=a.warmup, configs={})
    for name in a.configs.split(","):
        cfg = CONFIGS[name]
        dct = time_trainer("dct", cfg, a.steps, a.warmup)
        mt = time_trainer("mt", cfg, a.steps, a.warmup)
        res["configs"][name] = dict(batch_size=cfg[2], labeled_bs=cfg[3], dct=dct, mt=mt,
                                    dct_over_mt=round(dct["ms_per_step"] / mt["ms_per_step"], 4))
    if not a.no_kernels:
        res["kernels"] = kernel_times(min(a.steps, 5), a.kernel_timeout)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
