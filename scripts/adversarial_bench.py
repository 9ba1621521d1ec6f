"""Adversarial training on the device, 3-D (``--dim 3``, the default) or 2-D (``--dim 2``): one AdversarialTrainer step beside
a supervised-only step of the same segmenter on the same batch, and every discriminator kernel against the fp32 MFMA peak and
against the same layer in torch.nn.functional.conv3d / conv2d.

    python scripts/adversarial_bench.py [--dim {2,3}] [--reps 5] [--windows 3] [--steps 6] [--ndf 64] [--no-step]
                                        [--no-kernels] [--models ...] [--out profiles/adversarial{,2d}_bench.json]

A host-side driver: it runs GPU work only when invoked, needs a device (no fallback) and reads nothing outside the checkout.
``DIMS`` holds what a dimension sets: the batch ([2 + 2, 1, 96, 96, 96] with ``FC3DDiscriminator(2, ndf)`` under unet_3D;
[12 + 12, 1, S, S] with ``FCDiscriminator(4, ndf)`` under ``unet`` at 256 x 256 and ``ViT_Seg`` at 224 x 224), the models, the
names of its result fields.  Writes one JSON file (and prints it as one line):

  step     ``AdversarialTrainer(model, discriminator)`` at the dimension's batch, taped, and a supervised-only step of the same
           model on the same batch (forward, mis_loss_tail with all samples labeled, backward, SGD; recorded on a launch tape
           too), alternating window by window in one process: ms per step and volumes or images / s (host clock around
           ``steps`` steps ending in a synchronise), the difference, the host's enqueue time of a taped adversarial step and
           its launch count.  2-D: one such entry per model, and the supervised tape's launch count.
  kernels  device-event time of every discriminator launch of phase B (all N samples: four forwards -- conv0 and conv1 are
           one --, three data gradients, four weight gradients), of phase A's ``map`` gradient (the unlabeled half), the head,
           the tail and Adam, each the median over ``windows`` windows of ``reps`` launches; for the convolutions the executed
           multiply-adds (2 N Cout Cin taps So, taps = 4^dim), the TF/s they ran at and that as a fraction of the 157.3 TF fp32
           MFMA peak; beside each the same operation through torch.nn.functional.conv{2,3}d / torch.autograd.grad on the same
           device in the same run, timed the same way.  2-D: at 256 x 256.
  chain    the sums: our phase-B discriminator convolutions against torch's.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_TF = 157.3
NOTE = "torch's first-layer forward includes the softmax and the concatenation it needs; ours reads the logits"
# per dimension: batch, edge per model (the first model's is the kernels'), label type of a step, and what its JSON calls things.
# ``map_torch``: the samples torch's map gradient is timed on; ``nested``: one step entry per model, with the 2-D-only fields
DIMS = {
    3: dict(batch=4, labeled_bs=2, num_classes=2, size=dict(unet_3D=96), labels="int64", map_torch="all", nested=False,
            metric="adversarial_step_and_discriminator_kernels", out="adversarial_bench.json", rate=("volumes_per_s", 2),
            supervised="supervised_unet_3D", note=NOTE),
    2: dict(batch=24, labeled_bs=12, num_classes=4, size=dict(unet=256, ViT_Seg=224), labels="uint8", map_torch="unlabeled",
            nested=True, metric="adversarial2d_step_and_discriminator_kernels", out="adversarial2d_bench.json",
            rate=("images_per_s", 1), supervised="supervised",
            note=NOTE + "; torch's map gradient is formed at all 5 input channels"),
}


def _discriminator(dim, C, ndf):
    if dim == 3:
        from networks.discriminator import FC3DDiscriminator
        return FC3DDiscriminator(C, ndf=ndf).train()
    from networks.discriminator_2d import FCDiscriminator
    return FCDiscriminator(C, ndf=ndf).train()


def _model(name, C):
    if name == "ViT_Seg":
        from config import lite_config
        from networks.vision_transformer import SwinUnet
        return SwinUnet(lite_config(), img_size=224, num_classes=C).train()
    if name == "unet_3D":
        from networks.net_factory_3d import net_factory_3d
        return net_factory_3d(name, 1, C).train()
    from networks.net_factory import net_factory
    return net_factory(name, 1, C).train()


def _time_variants(variants, reps, windows):
    """{name: median ms per call}; every window times each variant once, in turn (``reps`` calls back to back)."""
    import torch
    for fn in variants.values():
        for _ in range(2):
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


def kernels(dim, ndf, reps, windows):
    import torch
    import torch.nn.functional as F
    from mis_hip import ops
    cfg = DIMS[dim]
    N, C, L, E = cfg["batch"], cfg["num_classes"], cfg["labeled_bs"], next(iter(cfg["size"].values()))
    conv, taps, ext = (F.conv2d, F.conv3d)[dim - 2], 4 ** dim, (E,) * dim
    g = torch.Generator(device="cuda").manual_seed(0)
    vol = torch.rand((N, 1) + ext, generator=g, device="cuda")
    logits = torch.randn((N, C) + ext, generator=g, device="cuda")
    lab = torch.randint(0, C, (N,) + ext, generator=g, device="cuda")
    dan = _discriminator(dim, C, ndf)
    cin = [C + 1, ndf, 2 * ndf, 4 * ndf]
    cout = [ndf, 2 * ndf, 4 * ndf, 8 * ndf]
    dan.drop_masks = [(torch.rand(N, c, generator=g, device="cuda") < 0.5).float() * 2
                      for c, (_, drop) in zip(cout, dan.LAYER_ACT) if drop]
    target = (torch.arange(N) < L).int().cuda()
    dan.loss_forward(logits, vol, target)
    dan.loss_backward(params=True, dmap=True)
    torch.cuda.synchronize()
    b = dan._cur[0]
    a, gr, sc = b["act"], b["grad"], dan._cur[3]
    slope = [s for s, _ in dan.LAYER_ACT]
    y = [a[i] if slope[i] != 1.0 else None for i in range(4)]       # a layer without an activation hands no output on
    P = dan.P
    names = ["conv0+1", "conv2", "conv3", "conv4"]
    wkeys = [None, "conv2", "conv3", "conv4"]
    variants, flops = {}, {}
    ins = [None] + a[:3]
    # torch operands: the same tensors; softmax + concatenation + one convolution for the first layer
    tw = [torch.cat([P("conv0.weight").data, P("conv1.weight").data], 1).clone().requires_grad_(True)] + \
         [P(k + ".weight").data.clone().requires_grad_(True) for k in wkeys[1:]]
    tb = [(P("conv0.bias").data + P("conv1.bias").data).clone()] + [P(k + ".bias").data.clone() for k in wkeys[1:]]

    def torch_in(i):
        x = torch.cat([torch.softmax(logits, 1), vol], 1) if i == 0 else ins[i]
        return x.detach().clone().requires_grad_(True)
    tx = [torch_in(i) for i in range(4)]
    ty = [conv(tx[i], tw[i], tb[i], stride=2, padding=1) for i in range(4)]
    dmap = f"dgrad/conv0 (map, N={N - L})"
    for i in range(4):
        So = (E >> (i + 1)) ** dim
        fl = 2.0 * N * cout[i] * cin[i] * taps * So
        n = names[i]
        if i == 0:
            variants[f"fwd/{n}"] = lambda: ops.conv_k4s2_fwd(vol, logits, P("conv1.weight").data, P("conv0.weight").data,
                                                             P("conv1.bias").data, P("conv0.bias").data, a[0], slope[0], sc[0])
            variants[f"wgrad/{n}"] = lambda: ops.conv_k4s2_wgrad(vol, logits, gr[0], y[0], P("conv1.weight").grad,
                                                                 P("conv0.weight").grad, P("conv1.bias").grad,
                                                                 P("conv0.bias").grad, slope[0], sc[0])
            y0_u, sc0_u = (None if t is None else t[L:] for t in (y[0], sc[0]))
            variants[dmap] = lambda: ops.conv_k4s2_dgrad(gr[0][L:], y0_u, P("conv0.weight").data, b["dmap"][L:], slope[0], sc0_u)
            flops[dmap] = 2.0 * (N - L) * cout[0] * C * taps * So
            variants[f"torch/fwd/{n}"] = lambda: conv(torch.cat([torch.softmax(logits, 1), vol], 1), tw[0], tb[0], stride=2,
                                                      padding=1)
        else:
            k = wkeys[i]
            variants[f"fwd/{n}"] = lambda i=i, k=k: ops.conv_k4s2_fwd(a[i - 1], None, P(k + ".weight").data, None,
                                                                      P(k + ".bias").data, None, a[i], slope[i], sc[i])
            variants[f"wgrad/{n}"] = lambda i=i, k=k: ops.conv_k4s2_wgrad(a[i - 1], None, gr[i], y[i], P(k + ".weight").grad,
                                                                          None, P(k + ".bias").grad, None, slope[i], sc[i])
            variants[f"dgrad/{n}"] = lambda i=i, k=k: ops.conv_k4s2_dgrad(gr[i], y[i], P(k + ".weight").data, gr[i - 1],
                                                                          slope[i], sc[i])
            flops[f"dgrad/{n}"] = fl
            variants[f"torch/fwd/{n}"] = lambda i=i: conv(tx[i].detach(), tw[i].detach(), tb[i], stride=2, padding=1)
            variants[f"torch/dgrad/{n}"] = lambda i=i: torch.autograd.grad(ty[i], [tx[i]], gr[i], retain_graph=True)
        flops[f"fwd/{n}"] = flops[f"wgrad/{n}"] = fl
        variants[f"torch/wgrad/{n}"] = lambda i=i: torch.autograd.grad(ty[i], [tw[i]], gr[i], retain_graph=True)
    # torch's map gradient: the gradient at every input channel of the first layer, on all samples or on the unlabeled ones
    if cfg["map_torch"] == "all":
        txm, tym, gm = tx[0], ty[0], gr[0]
    else:
        txm = tx[0][L:].detach().clone().requires_grad_(True)
        tym, gm = conv(txm, tw[0], tb[0], stride=2, padding=1), gr[0][L:]
    variants["torch/" + dmap] = lambda: torch.autograd.grad(tym, [txm], gm, retain_graph=True)
    ws = b["head"]
    cw, cb = P("classifier.weight"), P("classifier.bias")
    variants["head_fwd"] = lambda: ops.adv_head_fwd(a[3], cw.data, cb.data, target, b["loss"], b["logits"], ws, dan.pool)
    variants["head_bwd"] = lambda: ops.adv_head_bwd(cw.data, gr[3], cw.grad, cb.grad, ws, dan.pool)
    lg5 = logits if dim == 3 else logits.unsqueeze(2)
    out, dl = torch.zeros(16, device="cuda"), torch.empty_like(lg5)
    variants["tail"] = lambda: ops.adversarial_tail(lg5, lab[:L].contiguous(), L, b["dmap"][L:], b["loss"], out, dl, cons_weight=0.1)
    m, v, st = torch.zeros_like(dan.flat_param), torch.zeros_like(dan.flat_param), torch.zeros(2, dtype=torch.int64, device="cuda")
    ops.adam_init(st, 0)
    variants["adam"] = lambda: ops.adam_step(dan.flat_param, dan.flat_grad, m, v, st, 1e-4, (0.9, 0.99), 1e-8)
    with torch.no_grad():
        fwd_only = {k: f for k, f in variants.items() if "torch/fwd" in k}
        ms = _time_variants(fwd_only, reps, windows)
    ms.update(_time_variants({k: f for k, f in variants.items() if k not in fwd_only}, reps, windows))
    rows = {}
    for k in variants:
        if k.startswith("torch/"):
            continue
        row = dict(ms=round(ms[k], 4))
        if k in flops:
            tf = flops[k] / ms[k] / 1e9
            row.update(gflop=round(flops[k] / 1e9, 2), tf_per_s=round(tf, 2), fraction_of_fp32_mfma_peak=round(tf / PEAK_TF, 4))
        t = ms.get("torch/" + k)
        if t is not None:
            row.update(torch_ms=round(t, 4), torch_over_hip=round(t / ms[k], 2), slower_than_torch=bool(ms[k] > t))
        rows[k] = row
    convs = [k for k in rows if "/" in k]
    ours = sum(rows[k]["ms"] for k in convs if "map" not in k)
    theirs = sum(rows[k]["torch_ms"] for k in convs if "map" not in k)
    chain = dict(phase_b_convolutions_ms=round(ours, 3), torch_ms=round(theirs, 3), torch_over_hip=round(theirs / ours, 2),
                 phase_b_gflop=round(sum(flops[k] for k in convs if "map" not in k) / 1e9, 1), note=cfg["note"])
    return dict(ndf=ndf, N=N, **(dict(extent=E) if cfg["nested"] else {}), kernels=rows, chain=chain)


def step(dim, name, ndf, steps, windows):
    import torch
    from mis_hip import lib, ops
    from mis_hip.step import AdversarialTrainer
    cfg = DIMS[dim]
    N, L, C, E = cfg["batch"], cfg["labeled_bs"], cfg["num_classes"], cfg["size"][name]
    shape = (N, 1) + (E,) * dim
    g = torch.Generator(device="cuda").manual_seed(0)
    vol = torch.rand(shape, generator=g, device="cuda")
    lab = torch.randint(0, C, (N,) + shape[2:], generator=g, device="cuda").to(getattr(torch, cfg["labels"]))
    tr = AdversarialTrainer(_model(name, C), _discriminator(dim, C, ndf), labeled_bs=L, num_classes=C, seed=1337, iter_num=1000,
                            use_tape=True)
    sup = _model(name, C)
    state = ops.new_step_state()
    hyper = dict(base_lr=0.01, max_iterations=30000.0, ema_decay=0.0, consistency=0.1, rampup=200.0)
    ops.step_init(state, 1337, 1000, **hyper)
    sup.step_state, sup.rng_stream = state, 1
    mom, out = torch.zeros_like(sup.flat_param), torch.zeros(16, device="cuda")

    def sup_step():
        s = sup.forward_raw(vol)
        ops.loss_tail(s, None, lab, N, out, dlogits=sup.logits_grad_buffer(), state=state)
        sup.backward_raw()
        ops.sgd_ema_step(sup.flat_param, sup.flat_grad, mom, None, state=state)
        ops.step_advance(state, **hyper)
    for _ in range(4):
        tr.step(vol, lab)
    for _ in range(2):
        sup_step()
    tape = lib.LaunchTape()
    with tape.recording():
        sup_step()
    torch.cuda.synchronize()
    runs = {"adversarial": lambda: tr.step(vol, lab), cfg["supervised"]: tape.replay}
    got = {k: [] for k in runs}
    for _ in range(windows):
        for k, fn in runs.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            got[k].append((time.perf_counter() - t0) * 1e3 / steps)
    enq = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.step(vol, lab)
        enq.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    res = {}
    rate, digits = cfg["rate"]
    for k in runs:
        ms = statistics.median(got[k])
        res[k] = {"ms_per_step": round(ms, 3), "windows_ms": [round(v, 3) for v in got[k]], rate: round(N * 1e3 / ms, digits)}
    res["adversarial"].update(host_enqueue_ms_taped=round(statistics.median(enq), 3), tape_launches=len(tr._tape), **tr.losses())
    if cfg["nested"]:
        res[cfg["supervised"]]["tape_launches"] = len(tape)
    res["adversarial_minus_supervised_ms"] = round(res["adversarial"]["ms_per_step"] - res[cfg["supervised"]]["ms_per_step"], 3)
    res["config"] = dict(shape=shape, labeled_bs=L, num_classes=C, ndf=ndf, model=name, taped=True)
    res["peak_memory_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=3, choices=sorted(DIMS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--ndf", type=int, default=64)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--models", nargs="+", help="the dimension's segmenters to step (default: all of them)")
    ap.add_argument("--out", help="default: profiles/adversarial_bench.json, for --dim 2 profiles/adversarial2d_bench.json")
    a = ap.parse_args()
    cfg = DIMS[a.dim]
    models = a.models or list(cfg["size"])
    if set(models) - set(cfg["size"]):
        ap.error(f"--models for --dim {a.dim}: {', '.join(cfg['size'])}")
    out_path = a.out or os.path.join(ROOT, "profiles", cfg["out"])
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("adversarial_bench.py measures on the device: no GPU found (there is no CPU fallback, nothing is estimated)")
    torch.cuda.set_device(0)
    res = dict(metric=cfg["metric"], device=torch.cuda.get_device_name(0), reps=a.reps, windows=a.windows, steps=a.steps,
               fp32_mfma_peak_tf=PEAK_TF)
    if not a.no_kernels:
        res["discriminator"] = kernels(a.dim, a.ndf, a.reps, a.windows)
        torch.cuda.empty_cache()
    if not a.no_step:
        res["step"] = {}
        for name in models:
            res["step"][name] = step(a.dim, name, a.ndf, a.steps, a.windows)
            torch.cuda.empty_cache()
        if not cfg["nested"]:
            (res["step"],) = res["step"].values()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
