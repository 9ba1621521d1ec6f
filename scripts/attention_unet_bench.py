"""Attention U-Net on the device: one Mean-Teacher step beside unet_3D's on the same batch, the gate kernels of the three
gated levels against their byte floors and against the same expression in torch ops, and the integer up-sampling.

    python scripts/attention_unet_bench.py [--reps 20] [--windows 3] [--steps 10] [--warmup 4] [--no-step] [--no-kernels]
                                           [--no-gates] [--out profiles/attention_unet_bench.json]

A host-side driver: it runs GPU work only when invoked, needs a device (no fallback) and reads nothing outside the checkout.
Writes one JSON file (and prints it as one line):

  step     MeanTeacherTrainer steps of ``net_factory_3d("attention_unet", 1, 2)`` and of ``net_factory_3d("unet_3D", 1, 2)`` at
           bench.py's north-star batch ([4 + 4, 1, 96, 96, 96], 2 classes), the two trainers alternating window by window in
           one process: ms per step and volumes / s (host clock around ``steps`` taped steps ending in a synchronise, after
           ``warmup`` steps), the difference, and the host's enqueue time of a taped step (host clock around step() alone).
  kernels  from a child run of this script under ``rocprofv3 --kernel-trace --stats``: device time per attention_unet step by
           kernel family and its share of the summed kernel time -- the gate kernels, the up-sampling of the heads, 1x1x1
           convolutions (the gates' theta / phi / W / combine, the gating signal, the heads and ``final`` together: the trace
           has no layer names), 3x3x3 convolutions, normalisation / activation, the rest.  Kernels of two streams overlap, so
           the shares are of device work, not of wall time.
  gates    for each gated level of that batch (fine 48^3 / 24^3 / 12^3, C = 32 / 64 / 128, N = 8, G = 2): device-event time of
           mis_attn_gate_apply_fwd / _bwd and of the two per-gate launches of mis_attn_gate_map_fwd / _bwd, the bytes each must
           move (computed here from the shapes: every operand once), that floor at 8 TB/s -- the project's convention -- and
           the achieved fraction; beside them the same expression in torch ops on the same device (F.interpolate, expand, mul,
           autograd), timed the same way.  Each figure is the median over ``windows`` windows of ``reps`` launches.
  heads    the deep-supervision ops of one plan at that batch -- the dsv4 / dsv3 / dsv2 1x1x1 convolutions and their up-sampling
           by 8 / 4 / 2, dsv1 and ``final`` at 96^3 -- run on their own, on one stream: device-event time of their forwards and
           of their backwards (data, weight and bias gradients), and what that is per step (two forwards: student and teacher, one
           backward) beside the step time.  What a head that never materialises the [N, 4 n_classes, 96^3] buffer could save is
           bounded by it.
  upsample mis_upsample_int_fwd / _bwd at s = 4 (24^3 -> 96^3) and s = 8 (12^3 -> 96^3), N = 8, K = 2, into / out of a slice
           of the [8, 8, 96^3] head buffer, against their byte floors.
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

STEP_CFG = dict(shape=(8, 1, 96, 96, 96), labeled_bs=4, num_classes=2)      # bench.py's "unet3d" workload
HBM_TBS = 8.0
LEVELS = [(32, 48), (64, 24), (128, 12)]                                    # (C = Ci, fine edge) of levels 2, 3, 4
FAMILIES = (("gate", ("gate_map_", "gate_apply_")),
            ("upsample_int", ("upsample_int_",)),
            ("conv1x1", ("conv_fwd_kernel<Cfg<1, 1, 1", "conv_wgrad_kernel<WCfg<1, 1, 1", "conv1x1_", "conv_k2s2", "space_to_depth",
                         "conv_small_cout")),
            ("conv3x3x3", ("conv_fwd_kernel<Cfg<3", "conv_wgrad_kernel<WCfg<3", "wino", "conv_fwd_cin1", "wgrad_cin1", "conv_wgrad_reduce",
                           "pack_")),
            ("norm_act", ("apply_fwd", "apply_bwd", "bwd_partial", "bwd_final", "bwd_small", "stats_", "channel_sum", "running_to_stats",
                          "head_", "bwd_tiles", "norm_")),
            ("pool_upsample2", ("maxpool", "upsample_tri2", "upsample_fwd", "upsample_bwd")))


def _time_variants(variants, reps, windows):
    """{name: median ms per call}; every window times each variant once, in turn (``reps`` calls back to back), so that a drift
    of the machine's clocks or load falls on all of them alike."""
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
    return {k: statistics.median(v) for k, v in got.items()}


def _row(ms, nbytes):
    floor_ms = nbytes / (HBM_TBS * 1e12) * 1e3
    return dict(ms=round(ms, 4), mbytes=round(nbytes / 1e6, 2), floor_ms_at_8tbs=round(floor_ms, 4),
                fraction_of_floor=round(floor_ms / ms, 3), tb_per_s=round(nbytes / ms / 1e9, 3))


def gates(reps, windows):
    import torch
    import torch.nn.functional as F
    from mis_hip import ops
    N, G = STEP_CFG["shape"][0], 2
    out = []
    for C, e in LEVELS:
        g = torch.Generator(device="cuda").manual_seed(C)
        fine, coarse = (e, e, e), (e // 2,) * 3
        S, s = e ** 3, (e // 2) ** 3
        x = torch.randn((N, C) + fine, generator=g, device="cuda")
        dy = torch.randn((N, G * C) + fine, generator=g, device="cuda")
        y, dx = torch.empty_like(dy), torch.empty_like(x)
        theta = torch.randn((N, G * C) + coarse, generator=g, device="cuda")
        phi = torch.randn((N, G * C) + coarse, generator=g, device="cuda")
        df = torch.empty_like(theta)
        psi_w = torch.randn((G, C), generator=g, device="cuda") / C ** 0.5
        psi_b = torch.zeros(G, device="cuda")
        dw, db, dp = torch.empty_like(psi_w), torch.empty_like(psi_b), torch.empty(G * C, device="cuda")
        att = torch.rand((N, G) + coarse, generator=g, device="cuda")
        datt = torch.randn((N, G) + coarse, generator=g, device="cuda")
        sl = [(slice(k * C, (k + 1) * C), slice(k, k + 1)) for k in range(G)]

        def map_fwd():              # the plan's form: one launch per gate (the gates' psi are not adjacent in the flat buffer)
            for c, a in sl:
                ops.attn_gate_map_fwd(theta[:, c], phi[:, c], psi_w[a], psi_b[a], att[:, a])

        def map_bwd():
            for k, (c, a) in enumerate(sl):
                ops.attn_gate_map_bwd(datt[:, a], att[:, a], theta[:, c], phi[:, c], psi_w[a], df[:, c], dw[k], db[a], dp[c])

        xt, at = x.clone().requires_grad_(True), att.clone().requires_grad_(True)

        def torch_apply_fwd():
            up = F.interpolate(at, size=fine, mode="trilinear", align_corners=False)
            return torch.cat([up[:, k:k + 1].expand_as(xt) * xt for k in range(G)], 1)

        def torch_apply_fwd_nograd():
            with torch.no_grad():
                torch_apply_fwd()
        yt = torch_apply_fwd()

        def torch_apply_bwd():
            torch.autograd.grad(yt, [xt, at], dy, retain_graph=True)
        tt, pt, wt, bt = (t.clone().requires_grad_(True) for t in (theta, phi, psi_w, psi_b))

        def torch_map_fwd():
            f = F.relu(tt + pt)
            return torch.cat([torch.sigmoid(F.conv3d(f[:, c], wt[a].reshape(1, C, 1, 1, 1), bt[a])) for c, a in sl], 1)

        def torch_map_fwd_nograd():
            with torch.no_grad():
                torch_map_fwd()
        mt = torch_map_fwd()

        def torch_map_bwd():
            torch.autograd.grad(mt, [tt, pt, wt, bt], datt, retain_graph=True)
        ms = _time_variants({"apply_fwd": lambda: ops.attn_gate_apply_fwd(x, att, y),
                             "apply_bwd": lambda: ops.attn_gate_apply_bwd(dy, x, att, dx, datt),
                             "map_fwd": map_fwd, "map_bwd": map_bwd,
                             "torch/apply_fwd": torch_apply_fwd_nograd, "torch/apply_bwd": torch_apply_bwd,
                             "torch/map_fwd": torch_map_fwd_nograd, "torch/map_bwd": torch_map_bwd}, reps, windows)
        nbytes = {"apply_fwd": 4 * N * (C * S + G * s + G * C * S),                       # x, att; y
                  "apply_bwd": 4 * N * (G * C * S + C * S + G * s + C * S + G * s),       # dy, x, att; dx, datt
                  "map_fwd": 4 * N * (2 * G * C * s + G * s),                             # theta, phi; att
                  "map_bwd": 4 * N * (2 * G * s + 2 * G * C * s + G * C * s)}             # datt, att, theta, phi; df
        rows = {k: dict(_row(ms[k], nbytes[k]), torch_ms=round(ms["torch/" + k], 4), torch_over_hip=round(ms["torch/" + k] / ms[k], 2))
                for k in nbytes}
        out.append(dict(level_fine=list(fine), C=C, Ci=C, N=N, G=G, x_mbytes=round(4 * N * C * S / 1e6, 1), kernels=rows))
        del x, dy, y, dx, xt, yt
        torch.cuda.empty_cache()
    return out


def upsample(reps, windows):
    import torch
    from mis_hip import ops
    N, K, E = STEP_CFG["shape"][0], STEP_CFG["num_classes"], STEP_CFG["shape"][2]
    wide, gwide = torch.empty((N, 4 * K, E, E, E), device="cuda"), torch.randn((N, 4 * K, E, E, E), device="cuda")
    out = {}
    for s in (4, 8):
        e = E // s
        x, dx = torch.randn((N, K, e, e, e), device="cuda"), torch.empty((N, K, e, e, e), device="cuda")
        y, dy = wide[:, K:2 * K], gwide[:, K:2 * K]
        ms = _time_variants({"fwd": lambda: ops.upsample_int_fwd(x, y, s), "bwd": lambda: ops.upsample_int_bwd(dy, dx, s)}, reps,
                            windows)
        nb = 4 * N * K * (E ** 3 + e ** 3)
        out[f"s{s}"] = dict(coarse=[e, e, e], fwd=_row(ms["fwd"], nb), bwd=_row(ms["bwd"], nb))
    return out


def heads(reps, windows, step_ms=None):
    import torch
    from mis_hip.plan import ConvOp, UpsampleOp
    from networks.net_factory_3d import net_factory_3d
    shape, C = STEP_CFG["shape"], STEP_CFG["num_classes"]
    m = net_factory_3d("attention_unet", 1, C)
    m.train()
    g = torch.Generator(device="cuda").manual_seed(0)
    m.forward_raw(torch.rand(shape, generator=g, device="cuda"))
    m.backward_raw(torch.randn((shape[0], C) + shape[2:], generator=g, device="cuda"))
    torch.cuda.synchronize()
    plan, ctx = m._last
    ctx.wgrad_stream = None                     # the one-stream form of every backward: the events see all of it
    final = plan.ops[-1]
    buf = final.x                               # [N, 4 n_classes, D, H, W]: dsv1 .. dsv4 side by side
    ups = [op for op in plan.ops if type(op) is UpsampleOp and op.y._root() is buf]
    convs = [op for op in plan.ops if type(op) is ConvOp and (op.y._root() is buf or any(op.y is u.x for u in ups))]
    ops_ = [op for op in plan.ops if op in ups or op in convs] + [final]
    assert len(ups) == 3 and len(convs) == 4

    def fwd():
        for op in ops_:
            op.fwd(ctx)

    def bwd():
        for a in plan.acts:                     # as at the start of a backward walk: the heads' inputs are not written yet
            a.reset()
        for op in reversed(ops_):
            op.bwd(ctx)
    ms = _time_variants({"fwd": fwd, "bwd": bwd}, reps, windows)
    per_step = 2 * ms["fwd"] + ms["bwd"]
    res = dict(ops=[type(op).__name__ + (f"(x{op.scale})" if type(op) is UpsampleOp else f"({op.cin}->{op.cout})") for op in ops_],
               fwd_ms=round(ms["fwd"], 4), bwd_ms=round(ms["bwd"], 4), per_step_ms_two_forwards_one_backward=round(per_step, 4),
               buffer_mbytes=round(buf.t.numel() * 4 / 1e6, 1))
    if step_ms:
        res["fraction_of_step_time_if_serial"] = round(per_step / step_ms, 4)
    return res


def _trainer(model_key):
    import torch
    from mis_hip.step import MeanTeacherTrainer
    from networks.net_factory_3d import net_factory_3d
    shape, L, C = STEP_CFG["shape"], STEP_CFG["labeled_bs"], STEP_CFG["num_classes"]
    g = torch.Generator(device="cuda").manual_seed(0)
    vol = torch.rand(shape, generator=g, device="cuda")
    lab = torch.randint(0, C, (shape[0],) + shape[2:], generator=g, device="cuda")
    model, ema = net_factory_3d(model_key, 1, C), net_factory_3d(model_key, 1, C)
    for p in ema.parameters():
        p.detach_()
    model.train()
    ema.train()
    return MeanTeacherTrainer(model, ema, labeled_bs=L, num_classes=C, cons_start_iter=0, seed=1337, iter_num=1000, use_tape=True), vol, lab


def step(steps, warmup, windows):
    import torch
    trainers = {k: _trainer(k) for k in ("attention_unet", "unet_3D")}
    for tr, vol, lab in trainers.values():
        for _ in range(max(warmup, 4)):          # two eager steps, the recorded one, one replay
            tr.step(vol, lab)
    torch.cuda.synchronize()
    got = {k: [] for k in trainers}
    for _ in range(windows):
        for k, (tr, vol, lab) in trainers.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(vol, lab)
            torch.cuda.synchronize()
            got[k].append((time.perf_counter() - t0) * 1e3 / steps)
    res = {}
    for k, (tr, vol, lab) in trainers.items():
        enq = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.step(vol, lab)
            enq.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        ms = statistics.median(got[k])
        res[k] = dict(ms_per_step=round(ms, 3), windows_ms=[round(v, 3) for v in got[k]],
                      volumes_per_s=round(STEP_CFG["shape"][0] * 1e3 / ms, 2), host_enqueue_ms_taped=round(statistics.median(enq), 3),
                      tape_launches=len(tr._tape) if tr._tape is not None else None, loss=tr.losses()["loss"])
    res["config"] = dict(STEP_CFG, trainer="MeanTeacherTrainer", taped=True)
    res["attention_minus_unet_ms"] = round(res["attention_unet"]["ms_per_step"] - res["unet_3D"]["ms_per_step"], 3)
    res["peak_memory_gib_both_trainers"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    return res


def kernel_shares(steps, timeout):
    """Re-run this script under rocprofv3 (kernel trace); device ms per step and share of the summed kernel time per family."""
    out = tempfile.mkdtemp(prefix="attention_unet_bench_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--kernel-child", "--steps", str(steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            return dict(error=f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}")
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return dict(error="no kernel trace written")
        tot, names = {}, {}
        for path in traces:
            for row in csv.DictReader(open(path)):
                name = re.sub(r"\(anonymous namespace\)::", "", row["Kernel_Name"])
                name = re.sub(r"^void ", "", name)
                fam = next((f for f, pres in FAMILIES if any(p in name for p in pres)), "other")
                t = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6
                tot[fam] = tot.get(fam, 0.0) + t
                if fam in ("gate", "upsample_int", "other"):
                    key = name.split("(")[0][:60]
                    names[key] = names.get(key, 0.0) + t
        total = sum(tot.values())
        n = steps + 4                            # the child runs 4 warm-up steps and `steps` timed ones
        return dict(steps_in_trace=n, device_ms_per_step={f: round(t / n, 3) for f, t in sorted(tot.items())},
                    share_of_kernel_time={f: round(t / total, 4) for f, t in sorted(tot.items())},
                    kernel_ms_per_step=round(total / n, 3),
                    gate_upsample_and_other_kernels_ms_per_step={k: round(t / n, 4) for k, t in sorted(names.items(), key=lambda kv: -kv[1])[:16]})
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
    ap.add_argument("--no-gates", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--kernel-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_unet_bench.json"))
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("attention_unet_bench.py measures on the device: no GPU found (there is no CPU fallback, nothing is estimated)")
    torch.cuda.set_device(0)
    if a.kernel_child:
        tr, vol, lab = _trainer("attention_unet")
        for _ in range(4 + a.steps):
            tr.step(vol, lab)
        torch.cuda.synchronize()
        return
    res = dict(metric="attention_unet_step_gates_and_upsampling", device=torch.cuda.get_device_name(0), reps=a.reps,
               windows=a.windows, steps=a.steps, warmup=a.warmup, hbm_tb_per_s_convention=HBM_TBS)
    if not a.no_gates:
        res["gates"] = gates(a.reps, a.windows)
        res["upsample"] = upsample(a.reps, a.windows)
    if not a.no_step:
        res["step"] = step(a.steps, a.warmup, a.windows)
    if not a.no_gates:
        res["heads"] = heads(a.reps, a.windows, res.get("step", {}).get("attention_unet", {}).get("ms_per_step"))
    if not a.no_kernels:
        res["kernels"] = kernel_shares(min(a.steps, 4), a.kernel_timeout)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
