"""mis_patch_nce, forward plus gradient, against the same loss written with torch.bmm and cross_entropy (the materialised
fp32 form of tests/patch_nce_oracle.py with autograd) on the same GPU in the same process, at the three geometries of the
reference's contrastive trainers: the projector output at 256^2 [12, 16, 64, 64] and at 224^2 [12, 16, 56, 56], the
classifier output [6, 32, 32, 32].

    python scripts/patch_nce_bench.py [--reps 30] [--warmup 5] [--out profiles/patch_nce_bench.json] [--no-kernels]

Prints ONE JSON line (and writes it to --out).  Per geometry: ms per call of both forms from device events, the two forms
alternating call by call after a warm-up of each so that both see the same clocks; peak device memory each form adds on
top of its inputs (torch.cuda.max_memory_allocated; the HIP form's is its workspace plus the gradient tensor, the
materialised form's the [B, N, N] logits, their concatenation, the softmax and their gradients); the agreement of the two
forms' loss and gradient; and -- from a separate child run under ``rocprofv3 --kernel-trace`` -- the device time of the
four kernels of mis_patch_nce with the achieved fp32 MFMA rate of the row walk (4 B N^2 d FLOP: B N^2 d multiply-adds
each for the score product and for P.K^).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")
for p in (PKG, ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# ascending workspace: the grow-only scratch buffer is allocated anew inside each geometry's measured window
GEOMETRIES = ((6, 32, 32, 32), (12, 16, 56, 56), (12, 16, 64, 64))
T = 0.07
KERNELS = ("pnce_prep_kernel", "pnce_rows_kernel", "pnce_epilogue_kernel", "pnce_final_kernel")


def _features(shape):
    import torch
    g = torch.Generator(device="cuda").manual_seed(shape[0] * 1000 + shape[2])
    # what the projector / classifier heads end in: conv, BatchNorm, ReLU, max-pool
    return (torch.relu(torch.randn(shape, generator=g, device="cuda")),
            torch.relu(torch.randn(shape, generator=g, device="cuda")))


def _hip_call(fq, fk, out, dq):
    from mis_hip import ops
    ops.patch_nce(fq, fk, out, dfeat=dq, temperature=T)


def _torch_call(fq, fk):
    import torch
    import patch_nce_oracle as pno
    q = fq.detach().requires_grad_(True)
    loss = pno.materialised_loss(q, fk, T, torch.float32)
    loss.backward()
    return loss.detach(), q.grad


def bench_geometry(shape, reps, warmup):
    import torch
    from mis_hip import lib
    B, d = shape[0], shape[1]
    N = shape[2] * shape[3]
    fq, fk = _features(shape)
    out = torch.zeros(3, device="cuda")
    torch.cuda.synchronize()

    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    dq = torch.empty_like(fq)
    _hip_call(fq, fk, out, dq)
    torch.cuda.synchronize()
    hip_peak = torch.cuda.max_memory_allocated() - base

    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss_t, grad_t = _torch_call(fq, fk)
    torch.cuda.synchronize()
    torch_peak = torch.cuda.max_memory_allocated() - base

    loss_diff = abs(out[0].item() - loss_t.item()) / abs(loss_t.item())
    grad_diff = ((dq - grad_t).abs().max() / grad_t.abs().max()).item()
    del loss_t, grad_t

    for _ in range(warmup):
        _hip_call(fq, fk, out, dq)
        _torch_call(fq, fk)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e0, e1, e2 in ev:
        e0.record()
        _hip_call(fq, fk, out, dq)
        e1.record()
        _torch_call(fq, fk)
        e2.record()
    torch.cuda.synchronize()
    hip_ms = sorted(e0.elapsed_time(e1) for e0, e1, _ in ev)
    torch_ms = sorted(e1.elapsed_time(e2) for _, e1, e2 in ev)
    med = lambda v: v[len(v) // 2]
    L = lib.load()
    return dict(shape=list(shape), N=N, reps=reps,
                hip_ms=round(med(hip_ms), 4), hip_ms_min=round(hip_ms[0], 4), hip_ms_max=round(hip_ms[-1], 4),
                torch_ms=round(med(torch_ms), 4), torch_ms_min=round(torch_ms[0], 4), torch_ms_max=round(torch_ms[-1], 4),
                torch_over_hip=round(med(torch_ms) / med(hip_ms), 2),
                workspace_bytes=int(L.mis_patch_nce_workspace_bytes(B, d, N)), hip_peak_bytes=int(hip_peak),
                torch_peak_bytes=int(torch_peak), logits_bytes=B * N * N * 4,
                loss=out[0].item(), loss_rel_diff=loss_diff, grad_rel_diff=grad_diff)


def kernel_child(reps):
    import torch
    for shape in GEOMETRIES:
        fq, fk = _features(shape)
        out, dq = torch.zeros(3, device="cuda"), torch.empty_like(fq)
        for _ in range(reps + 1):
            _hip_call(fq, fk, out, dq)
        torch.cuda.synchronize()


def kernel_times(reps, timeout):
    """Re-run this script under rocprofv3 (kernel trace): device us per call of each kernel, per geometry."""
    tmp = tempfile.mkdtemp(prefix="patch_nce_bench_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--kernel-child", "--reps", str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            return dict(error=f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}")
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = re.sub(r"^void ", "", re.sub(r"\(anonymous namespace\)::", "", row["Kernel_Name"]))
                for k in KERNELS:
                    if name.startswith(k):
                        t0, t1 = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                        rows.append((t0, k, (t1 - t0) / 1e3))
        rows.sort()
        per_call = len(KERNELS)
        if len(rows) != per_call * (reps + 1) * len(GEOMETRIES):
            return dict(error=f"{len(rows)} kernel records, expected {per_call * (reps + 1) * len(GEOMETRIES)}")
        res = {}
        for gi, shape in enumerate(GEOMETRIES):
            mine = rows[gi * per_call * (reps + 1):(gi + 1) * per_call * (reps + 1)][per_call:]      # first call: warm-up
            us = {k: sum(dt for _, kk, dt in mine if kk == k) / reps for k in KERNELS}
            B, d, N = shape[0], shape[1], shape[2] * shape[3]
            flop = 4.0 * B * N * N * d
            res["x".join(map(str, shape))] = dict(
                {k + "_us": round(v, 2) for k, v in us.items()}, total_us=round(sum(us.values()), 2),
                rows_flop=flop, rows_tflops=round(flop / us["pnce_rows_kernel"] / 1e6, 2), exps=B * N * N)
        return res
    except subprocess.TimeoutExpired:
        return dict(error=f"rocprofv3 run exceeded {timeout} s")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--kernel-timeout", type=int, default=240)
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("patch_nce_bench.py needs an MI355X: there is nothing to time on the CPU")
    torch.cuda.set_device(0)
    if a.kernel_child:
        kernel_child(a.reps)
        return
    res = dict(metric="patch_nce_fwd_grad_vs_materialised_torch", temperature=T, device=torch.cuda.get_device_name(0),
               geometries=[bench_geometry(s, a.reps, a.warmup) for s in GEOMETRIES])
    res["hip_faster_everywhere"] = all(g["hip_ms"] < g["torch_ms"] for g in res["geometries"])
    if not a.no_kernels:
        res["kernels"] = kernel_times(a.kernel_reps, a.kernel_timeout)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
