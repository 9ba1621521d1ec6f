"""PNet2D on the device: the dilated 3x3 layers beside the dense 3x3 layer of the same shape, and one Mean-Teacher step.

    python scripts/pnet_bench.py [--reps 20] [--windows 3] [--steps 10] [--warmup 4] [--no-step] [--no-kernels]
                                 [--out profiles/pnet_bench.json]

A host-side driver: it runs GPU work only when invoked, needs a device (no fallback) and reads nothing outside the checkout.
Writes one JSON file (and prints it as one line):

  layers   for [24, 64, 256, 256] and [24, 64, 224, 224], 64 -> 64 channels: device-event time of the forward, the data gradient
           and the weight gradient for d = 2, 4, 8, 16 (csrc/conv_dilated.hip), and of the d = 1 layer of that shape on the
           direct kernel (what MIS_WINO=0 selects) and on the Winograd kernel.  Each figure is the median over ``windows``
           windows of ``reps`` back-to-back launches, the variants alternating inside a window's round; executed fp32-MFMA
           TF = 2 * N * Cout * Cin * 9 * H * W / time (the flops of the direct form, also for the Winograd rows).
           ``ratio_to_direct`` = dilated / direct time.  The direct d = 1 kernel is the yardstick: same flops, same LDS image
           but for the halo, code this work did not change.  ``byte_account`` holds, per d, what the dilated tile moves more
           than the dense one, computed from the tile shapes: the rows a launch executes per image row (each phase's rows
           are cut into tiles of their own: 224 / 16 = 14 rows fill a 16-row tile to 7/8), haloed-tile floats gathered by
           LDS-DMA per output pixel, LDS operand reads per MFMA pair; the stores are the dense kernel's (float2 runs of a row).
  step     one MeanTeacherTrainer step with ``net_factory("pnet", 1, 4)`` at the defaults of train_mean_teacher_2D.py (batch 24,
           12 labeled, 256 x 256, 4 classes): ms per step and images / s (host clock around ``steps`` steps ending in a
           synchronise, after ``warmup`` steps), and the host's enqueue time of a taped step (host clock around step() alone).
  kernels  from a child run of this script under ``rocprofv3 --kernel-trace --stats``: device time per step by kernel family
           and its share of the summed kernel time -- dilated convolutions, dense 3x3, 1x1 convolutions, normalisation /
           activation, the rest.  Kernels of two streams overlap, so the shares are of device work, not of wall time.
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(24, 64, 256, 256), (24, 64, 224, 224)]
DILATIONS = (2, 4, 8, 16)
STEP_CFG = dict(batch_size=24, labeled_bs=12, patch=(256, 256), num_classes=4)     # train_mean_teacher_2D.py defaults
FAMILIES = (("dilated", ("conv_dilated_",)),
            ("conv1x1", ("conv_fwd_kernel<Cfg<1, 1, 1", "conv_wgrad_kernel<WCfg<1, 1, 1", "conv1x1_")),
            ("dense3x3", ("conv_fwd_kernel<Cfg<1, 3, 3", "conv_wgrad_kernel<WCfg<1, 3, 3", "wino2d_", "conv_small_cout", "conv_fwd_cin1",
                          "wgrad_cin1", "conv_wgrad_reduce")),
            ("norm_act", ("apply_fwd", "apply_bwd", "bwd_partial", "bwd_final", "bwd_small", "stats_", "channel_sum", "running_to_stats",
                          "head_")))


def _rows_executed(H, d, ty):
    """tile rows x TY a launch executes per image row: the phases' rows are cut into tiles of TY, each phase on its own"""
    nphase, tiles = min(d, H), -(-(-(-H // d)) // ty)
    return nphase * tiles * ty / H


def byte_account(d, H, W):
    """What a dilated forward tile moves beside the dense 3x3 tile of the same TY x TX pixels, and the rows a launch executes per
    image row (forward TY = 16, weight gradient TY = 8 for W >= 32, else 16) -- from the tile shapes alone."""
    ty, tx = 16, (32 if W >= 128 else 16)
    wty = 8 if W >= 32 else 16
    dense, dil = (ty + 2) * (tx + 2), (ty + 2) * (tx + 2 * d)
    return dict(tile=[ty, tx],
                rows_executed_per_image_row=dict(fwd_dense=round(_rows_executed(H, 1, ty), 3), fwd_dilated=round(_rows_executed(H, d, ty), 3),
                                                 wgrad_dense=round(_rows_executed(H, 1, wty), 3),
                                                 wgrad_dilated=round(_rows_executed(H, d, wty), 3)),
                dma_floats_per_pixel_dense=round(dense / (ty * tx), 3), dma_floats_per_pixel_dilated=round(dil / (ty * tx), 3),
                dma_ratio=round(dil / dense, 3), dma_gather="consecutive floats of a row (whole cache lines), as the dense kernel",
                lds_b64_reads_per_tap_row_and_pair=dict(dense=2, dilated=3), store="float2 runs of an image row, as the dense kernel",
                input_channels_per_chunk=dict(dense=8, dilated=4 if (d == 16 and tx == 32) else 8))


def _time_variants(variants, reps, windows):
    """{name: median ms per launch}; every window times each variant once, in turn (``reps`` launches back to back), so that a
    drift of the machine's clocks or load falls on all of them alike."""
    import torch
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in variants}
    for _ in range(windows):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            got[name].append(e0.elapsed_time(e1) / reps)
    return {k: statistics.median(v) for k, v in got.items()}, {k: [round(x, 4) for x in v] for k, v in got.items()}


def layers(reps, windows):
    import ctypes

    import torch
    from mis_hip import lib, ops
    L = lib.load()
    out = []
    for N, C, H, W in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randn((N, C, 1, H, W), generator=g, device="cuda").clamp_min(0)
        dy = torch.randn((N, C, 1, H, W), generator=g, device="cuda")
        y = torch.empty_like(x)
        w = (torch.rand((C, C, 1, 3, 3), generator=g, device="cuda") * 2 - 1) * 0.2
        b = torch.zeros(C, device="cuda")
        dw = torch.empty_like(w)
        wp0, wp1 = ops.conv_pack(w, 0), ops.conv_pack(w, 1)
        flops = 2.0 * N * C * C * 9 * H * W
        k = (1, 3, 3)
        v = ops.conv_wino_select(N, C, C, 1, H, W, k)
        variants, names = {}, {}

        def direct_wgrad():
            keep, ops.WINO = ops.WINO, 0            # what MIS_WINO=0 selects
            try:
                ops.conv_wgrad(x, dy, dw, k)
            finally:
                ops.WINO = keep
        variants["d1_direct/fwd"] = lambda: ops.conv_fwd(x, wp0, b, y, C, C, k, wino=-1)
        variants["d1_direct/dgrad"] = lambda: ops.conv_fwd(dy, wp1, None, y, C, C, k, wino=-1)
        variants["d1_direct/wgrad"] = direct_wgrad
        buf = ctypes.create_string_buffer(128)
        L.mis_conv_fwd_kernel_name(N, C, C, 1, H, W, 1, 3, 3, buf, 128)
        names["d1_direct/fwd"] = names["d1_direct/dgrad"] = buf.value.decode()
        L.mis_conv_wgrad_kernel_name(N, C, C, 1, H, W, 1, 3, 3, buf, 128)
        names["d1_direct/wgrad"] = buf.value.decode()
        if v >= 0:
            wq0 = ops.conv_pack(w, ops.conv_wino_pack_mode(v, False))
            wq1 = ops.conv_pack(w, ops.conv_wino_pack_mode(v, True))
            variants["d1_winograd/fwd"] = lambda: ops.conv_fwd(x, wq0, b, y, C, C, k, wino=v)
            variants["d1_winograd/dgrad"] = lambda: ops.conv_fwd(dy, wq1, None, y, C, C, k, wino=v)
            variants["d1_winograd/wgrad"] = lambda: ops.conv_wgrad(x, dy, dw, k)
            L.mis_conv2d_wino_kernel_name(v - ops.WINO2D, buf, 128)
            names["d1_winograd/fwd"] = names["d1_winograd/dgrad"] = buf.value.decode()
            v2 = int(L.mis_conv2d_wino_wgrad_select(N, C, C, H, W))
            if v2 >= 0:
                L.mis_conv2d_wino_wgrad_kernel_name(v2, buf, 128)
                names["d1_winograd/wgrad"] = buf.value.decode()
            else:
                names["d1_winograd/wgrad"] = names["d1_direct/wgrad"] + " (no Winograd weight gradient for this shape)"
        for d in DILATIONS:
            variants[f"d{d}/fwd"] = lambda d=d: ops.conv_dilated_fwd(x, wp0, b, y, d)
            variants[f"d{d}/dgrad"] = lambda d=d: ops.conv_dilated_fwd(dy, wp1, None, y, d, dgrad=True)
            variants[f"d{d}/wgrad"] = lambda d=d: ops.conv_dilated_wgrad(x, dy, dw, d)
            names[f"d{d}/fwd"] = ops.conv_dilated_fwd_kernel_name(N, C, C, H, W, d)
            names[f"d{d}/dgrad"] = ops.conv_dilated_dgrad_kernel_name(N, C, C, H, W, d)
            names[f"d{d}/wgrad"] = ops.conv_dilated_wgrad_kernel_name(N, C, C, H, W, d)
        ms, windows_ms = _time_variants(variants, reps, windows)
        rows = {}
        for key, t in ms.items():
            layer, kind = key.split("/")
            r = rows.setdefault(layer, {})
            r[kind] = dict(ms=round(t, 4), tf=round(flops / t / 1e9, 2), kernel=names[key], windows_ms=windows_ms[key])
        for d in DILATIONS:
            r = rows[f"d{d}"]
            r["ratio_to_direct"] = {kind: round(ms[f"d{d}/{kind}"] / ms[f"d1_direct/{kind}"], 3) for kind in ("fwd", "dgrad", "wgrad")}
            if "d1_winograd/fwd" in ms:
                r["ratio_to_winograd"] = {kind: round(ms[f"d{d}/{kind}"] / ms[f"d1_winograd/{kind}"], 3)
                                          for kind in ("fwd", "dgrad", "wgrad")}
            r["byte_account"] = byte_account(d, H, W)
        out.append(dict(shape=[N, C, H, W], cin=C, cout=C, gflop_per_launch=round(flops / 1e9, 2), layers=rows))
        del x, dy, y
        torch.cuda.empty_cache()
    return out


def _trainer(use_tape):
    import torch
    from mis_hip.step import MeanTeacherTrainer
    from networks.net_factory import net_factory
    B, L, sp, C = STEP_CFG["batch_size"], STEP_CFG["labeled_bs"], STEP_CFG["patch"], STEP_CFG["num_classes"]
    g = torch.Generator(device="cuda").manual_seed(0)
    vol = torch.rand((B, 1) + sp, generator=g, device="cuda")
    lab = torch.randint(0, C, (B,) + sp, generator=g, device="cuda").to(torch.uint8)
    model, ema = net_factory("pnet", 1, C), net_factory("pnet", 1, C)
    for p in ema.parameters():
        p.detach_()
    model.train()
    ema.train()
    return MeanTeacherTrainer(model, ema, labeled_bs=L, num_classes=C, iter_num=1000, max_iterations=30000, use_tape=use_tape), vol, lab


def step(steps, warmup):
    import torch
    tr, vol, lab = _trainer(True)
    for _ in range(max(warmup, 4)):          # two eager steps, the recorded one, one replay
        tr.step(vol, lab)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(vol, lab)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    enq = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.step(vol, lab)
        enq.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    B = STEP_CFG["batch_size"]
    return dict(config=dict(STEP_CFG, model="pnet", trainer="MeanTeacherTrainer"), ms_per_step=round(ms, 3),
                images_per_s=round(B * 1e3 / ms, 2), host_enqueue_ms_taped=round(statistics.median(enq), 3),
                tape_launches=len(tr._tape) if tr._tape is not None else None, loss=tr.losses()["loss"],
                peak_memory_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))


def kernel_shares(steps, timeout):
    """Re-run this script under rocprofv3 (kernel trace); device ms per step and share of the summed kernel time per family."""
    out = tempfile.mkdtemp(prefix="pnet_bench_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--kernel-child", "--steps", str(steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            return dict(error=f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}")
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return dict(error="no kernel trace written")
        tot = {}
        for path in traces:
            for row in csv.DictReader(open(path)):
                name = re.sub(r"\(anonymous namespace\)::", "", row["Kernel_Name"])
                name = re.sub(r"^void ", "", name)
                fam = next((f for f, pres in FAMILIES if any(name.startswith(p) for p in pres)), "other")
                tot[fam] = tot.get(fam, 0.0) + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6
        total = sum(tot.values())
        n = steps + 4                            # the child runs 4 warm-up steps and `steps` timed ones
        return dict(steps_in_trace=n, device_ms_per_step={f: round(t / n, 3) for f, t in sorted(tot.items())},
                    share_of_kernel_time={f: round(t / total, 4) for f, t in sorted(tot.items())},
                    kernel_ms_per_step=round(total / n, 3))
    except subprocess.TimeoutExpired:
        return dict(error=f"rocprofv3 run exceeded {timeout} s")
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--kernel-timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnet_bench.json"))
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pnet_bench.py measures on the device: no GPU found (there is no CPU fallback, nothing is estimated)")
    torch.cuda.set_device(0)
    if a.kernel_child:
        tr, vol, lab = _trainer(True)
        for _ in range(4 + a.steps):
            tr.step(vol, lab)
        torch.cuda.synchronize()
        return
    res = dict(metric="pnet_dilated_layers_and_step", device=torch.cuda.get_device_name(0), reps=a.reps, windows=a.windows,
               steps=a.steps, warmup=a.warmup)
    if not a.no_layers:
        res["layers"] = layers(a.reps, a.windows)
    if not a.no_step:
        res["step"] = step(a.steps, a.warmup)
    if not a.no_kernels:
        res["kernels"] = kernel_shares(min(a.steps, 4), a.kernel_timeout)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
