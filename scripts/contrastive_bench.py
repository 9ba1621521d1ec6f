"""What contrastive cross teaching costs on top of cross teaching, and where.

    python scripts/contrastive_bench.py [--steps 10] [--rounds 5] [--no-kernels] [--out profiles/contrastive_bench.json]

Prints ONE JSON line (and writes it to ``--out``).  Geometry: two UNets, [24, 1, 224, 224], L = 12, 4 classes.

  steps     ms per step of ContrastiveCrossTrainer and of CrossTeachingTrainer (Dice pseudo-supervision) on the same batch, in
            this process, both taped, measured alternately (``--rounds`` windows of ``--steps`` steps each, host clock around a
            device synchronise); their difference is the cost of the whole contrastive branch: four heads, two patch-NCE
            calls, two head backwards, the wider tail.
  kernels   device time from three child runs of this script under ``rocprofv3 --kernel-trace --stats`` on fixed logits:
            "branch"  the contrastive branch as the step issues it (4 head forwards, 2 mis_patch_nce, 2 head backwards, the two
                      tails), split per kernel family; alternating with it, the composition the existing kernels offer for
                      student 1: mis_cross_pseudo_tail + two separate gradient adds (mis_add over the rows that have a head
                      gradient).  The new tail's time is set against its byte floor at 8 TB/s: per pass the own logits, the
                      other student's unlabeled logits and the labels read once, in pass 2 also the head gradients read and
                      the logits gradient written once.
            "frozen" / "thawed"  the two query-side heads, forward + backward, as the trainer runs them (frozen: data gradient
                      only, filters packed once) and with weight, bias and affine gradients on.
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

SP, B, L, C = (224, 224), 24, 12, 4
FAMILIES = [("tail", r"^cc_"), ("cross_tail", r"^cross_"), ("add", r"^add_kernel"), ("patch_nce", r"^pnce_"),
            ("head_wgrad", r"wgrad|channel_sum"), ("head_pack", r"^pack_"), ("head_conv", r"^conv_|^wino"),
            ("head_norm_pool", r"^stats_|^apply_|^bwd_|^maxpool")]


def _batch():
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    vol = torch.rand((B, 1) + SP, generator=g, device="cuda")
    lab = torch.randint(0, C, (B,) + SP, generator=g, device="cuda").to(torch.uint8)
    return vol, lab


def _heads():
    from networks.net_factory import net_factory
    hs = [net_factory(k) for k in ("classifier", "classifier", "projector", "projector")]
    for h in hs:
        h.train()
    return hs


def time_steps(steps, rounds, warmup):
    import torch
    from mis_hip.step import ContrastiveCrossTrainer, CrossTeachingTrainer
    from networks.net_factory import net_factory
    vol, lab = _batch()
    torch.manual_seed(0)

    def unets():
        ms = [net_factory("unet", 1, C), net_factory("unet", 1, C)]
        for m in ms:
            m.train()
        return ms

    trainers = dict(
        contrastive=ContrastiveCrossTrainer(*unets(), *_heads(), labeled_bs=L, num_classes=C, iters_per_epoch=100,
                                            iter_num=1000, max_iterations=30000),
        cross_teaching=CrossTeachingTrainer(*unets(), labeled_bs=L, num_classes=C, iter_num=1000, max_iterations=30000))
    for tr in trainers.values():                 # two eager steps, the recording, replays
        for _ in range(warmup):
            tr.step(vol, lab)
    torch.cuda.synchronize()
    ms = {k: [] for k in trainers}
    for _ in range(rounds):
        for k, tr in trainers.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(vol, lab)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
    res = {}
    for k, v in ms.items():
        v = sorted(v)
        res[k] = dict(ms_per_step=round(v[len(v) // 2], 3), min=round(v[0], 3), max=round(v[-1], 3),
                      samples_per_s=round(B * 1e3 / v[len(v) // 2], 1), taped=trainers[k]._tape is not None,
                      launches_per_step=len(trainers[k]._tape) if trainers[k]._tape is not None else None)
    res["losses"] = {k: round(v, 6) for k, v in trainers["contrastive"].losses().items()}
    d = res["contrastive"]["ms_per_step"] - res["cross_teaching"]["ms_per_step"]
    res["contrastive_branch_ms"] = round(d, 3)
    res["contrastive_over_cross"] = round(res["contrastive"]["ms_per_step"] / res["cross_teaching"]["ms_per_step"], 4)
    return res


def kernel_child(mode, reps):
    import torch
    from mis_hip import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    z1 = torch.randn((B, C, 1) + SP, generator=g, device="cuda") * 3.0
    z2 = torch.randn((B, C, 1) + SP, generator=g, device="cuda") * 3.0
    lab = torch.randint(0, C, (L,) + SP, generator=g, device="cuda").to(torch.uint8)
    cls1, cls2, prj1, prj2 = _heads()
    v1, v2 = z1.squeeze(2), z2.squeeze(2)
    if mode in ("frozen", "thawed"):
        for h in (cls1, prj1):
            h.frozen = mode == "frozen"
        for _ in range(reps + 1):
            for h, x in ((cls1, v1[:L][0::2]), (prj1, v1[L:])):
                h.forward_raw(x)
                if _ == 0:
                    h.logits_grad_buffer().normal_(generator=g)
                h.backward_raw()
        torch.cuda.synchronize()
        return
    outs = [torch.zeros(16, device="cuda") for _ in range(4)]
    d1, d2 = torch.empty_like(z1), torch.empty_like(z2)
    for _ in range(reps + 1):
        k_l, k_u = cls2.forward_raw(v2[:L][1::2], no_backward=True), prj2.forward_raw(v2[L:], no_backward=True)
        q_l, q_u = cls1.forward_raw(v1[:L][0::2]), prj1.forward_raw(v1[L:])
        ops.patch_nce(q_l, k_l, outs[2], dfeat=cls1.logits_grad_buffer(), grad_scale=0.5)
        ops.patch_nce(q_u, k_u, outs[3], dfeat=prj1.logits_grad_buffer(), grad_scale=0.5)
        cls1.backward_raw()
        prj1.backward_raw()
        e_l, e_u = cls1.input_grad_buffer(), prj1.input_grad_buffer()
        ops.contrastive_cross_tail(z1, z2, lab, L, outs[0], dlogits=d1, extra_l=e_l, extra_u=e_u, cons_weight=0.05)
        ops.contrastive_cross_tail(z2, z1, lab, L, outs[1], dlogits=d2, cons_weight=0.05)
        # what the existing kernels offer for student 1: the cross-teaching tail, then two read-modify-writes of the rows
        # that have a head gradient
        ops.cross_teaching_tail(z1, z2, lab, L, outs[0], dlogits=d1, cons_weight=0.05)
        ops.add(d1[:L][0::2], e_l, d1[:L][0::2])
        ops.add(d1[L:], e_u, d1[L:])
    torch.cuda.synchronize()


def tail_floor_us(extras):
    S = SP[0] * SP[1]
    own, other, label, grad = B * C * S * 4, (B - L) * C * S * 4, L * S, B * C * S * 4
    extra = ((L // 2) + (B - L)) * C * S * 4 if extras else 0
    nbytes = (own + other + label) + (own + other + label + extra + grad)
    return nbytes, nbytes / 8e12 * 1e6


def kernel_times(mode, reps, timeout):
    """This script again under rocprofv3 (kernel trace): device us per repetition and kernel family, the first repetition
    (warm-up: code objects, plans, the one filter pack of a frozen head) dropped by its launch count."""
    out = tempfile.mkdtemp(prefix="contrastive_bench_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--kernel-child", mode, "--steps", str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            return dict(error=f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}")
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return dict(error="no kernel trace written")
        rows = []
        for path in traces:
            for row in csv.DictReader(open(path)):
                name = re.sub(r"\(anonymous namespace\)::", "", row["Kernel_Name"])
                name = re.sub(r"^void ", "", name)
                rows.append((int(row["Start_Timestamp"]), name, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
        rows.sort()
        # repetitions are delimited by the family that opens them; everything before the second opening is the warm-up
        fam_of = lambda n: next((f for f, pat in FAMILIES if re.search(pat, n)), None)
        tagged = [(fam_of(n), n, us) for _, n, us in rows if fam_of(n)]
        per_rep = len(tagged) // (reps + 1)
        steady = tagged[len(tagged) - per_rep * reps:]
        res, launches, names = {}, {}, {}
        for f, n, us in steady:
            res[f] = res.get(f, 0.0) + us / reps
            launches[f] = launches.get(f, 0) + 1
            names.setdefault(f, set()).add(n.split("(")[0][:60])
        return dict(us_per_rep={f: round(v, 2) for f, v in res.items()}, total_us=round(sum(res.values()), 2),
                    launches_per_rep={f: round(v / reps, 2) for f, v in launches.items()},
                    kernels={f: sorted(v) for f, v in names.items()}, reps=reps)
    except subprocess.TimeoutExpired:
        return dict(error=f"rocprofv3 run exceeded {timeout} s")
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--kernel-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("contrastive_bench.py measures on an MI355X; no GPU is visible")
    torch.cuda.set_device(0)
    if a.kernel_child:
        kernel_child(a.kernel_child, a.steps)
        return
    res = dict(metric="contrastive_cross_vs_cross_teaching_step", steps=a.steps, rounds=a.rounds, warmup=a.warmup,
               batch_size=B, labeled_bs=L, spatial=list(SP), num_classes=C)
    res["steps_ms"] = time_steps(a.steps, a.rounds, a.warmup)
    if not a.no_kernels:
        k = {m: kernel_times(m, a.kernel_reps, a.kernel_timeout) for m in ("branch", "frozen", "thawed")}
        res["kernels"] = k
        br = k["branch"].get("us_per_rep")
        if br:
            nb1, fl1 = tail_floor_us(True)
            nb2, fl2 = tail_floor_us(False)
            tail = br.get("tail", 0.0)
            res["tail"] = dict(both_students_us=tail, floor_bytes=nb1 + nb2, floor_us_at_8TBps=round(fl1 + fl2, 2),
                               over_floor=round(tail / (fl1 + fl2), 2) if tail else None,
                               cross_tail_plus_adds_us=round(br.get("cross_tail", 0.0) + br.get("add", 0.0), 2),
                               note="tail = students 1 and 2; cross_tail + add = student 1 alone with the existing kernels")
            heads = sum(v for f, v in br.items() if f.startswith("head_"))
            res["branch_split_us"] = dict(heads=round(heads, 2), patch_nce=br.get("patch_nce", 0.0), tail=tail)
        fz, th = k["frozen"].get("total_us"), k["thawed"].get("total_us")
        if fz and th:
            res["query_heads_fwd_bwd_us"] = dict(frozen=fz, with_weight_gradients=th, frozen_over_thawed=round(fz / th, 4))
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
