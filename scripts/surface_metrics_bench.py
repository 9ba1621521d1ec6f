"""Validation metrics, device against host: writes profiles/surface_metrics_bench.json.

Per shape (BraTS-sized 155 x 240 x 240, ACDC-sized 10 x 256 x 216; seeded ellipsoid masks):
  device_ms   one ``ops.surface_metrics`` call (device events, after warm-up, repeats for a window of >= 0.3 s)
  host_ms     ``metrics.hd95`` + ``metrics.dc`` on the same masks on this node's CPU (best of ``--host_repeats``)
  and whether the device's dc / hd95 / hd equal the host's (they must).
Then the wall time of one ``val_3D.test_all_case`` over a synthetic 4-case list (unet_3D, 2 classes, patch 96^3, stride 64:
test_3D.py's setting) with MIS_DEVICE_METRICS=0 and =1, alternating in the same run.  Needs an MI355X: no fallback.

    python scripts/surface_metrics_bench.py [--out profiles/surface_metrics_bench.json] [--rounds 2]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cv-ssl-mis_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(155, 240, 240), (10, 256, 216)]


def ellipsoid(shape, centre, radii):
    grids = np.meshgrid(*[np.arange(e, dtype=np.float64) for e in shape], indexing="ij")
    return sum(((g - c * e) / (r * e)) ** 2 for g, c, r, e in zip(grids, centre, radii, shape)) <= 1.0


def masks(shape, seed):
    rng = np.random.default_rng(seed)
    jitter = lambda v, s: tuple(x + s * (rng.random() - 0.5) for x in v)
    pred = ellipsoid(shape, jitter((0.5, 0.5, 0.5), 0.06), jitter((0.33, 0.3, 0.27), 0.04))
    gt = ellipsoid(shape, jitter((0.5, 0.5, 0.5), 0.06), jitter((0.33, 0.3, 0.27), 0.04))
    return pred.astype(np.uint8), gt.astype(np.uint8)


def time_device(fn, window=0.3):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 1
    while True:
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        ms = start.elapsed_time(stop)
        if ms >= window * 1e3:
            return ms / reps, reps
        reps = max(reps * 2, int(reps * window * 1.2e3 / max(ms, 1e-3)) + 1)


def bench_shape(shape, host_repeats):
    from mis_hip import ops
    from utils import metrics
    pred, gt = masks(shape, 1234)
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    device_ms, reps = time_device(lambda: ops.surface_metrics(dp, dg, 1))
    s = metrics.device_scores(dp, dg, 1)
    host_ms, host = [], None
    for _ in range(host_repeats):
        t0 = time.perf_counter()
        host = (metrics.hd95(pred == 1, gt == 1), metrics.dc(pred == 1, gt == 1))
        host_ms.append((time.perf_counter() - t0) * 1e3)
    return dict(shape=list(shape), device_ms=device_ms, device_repeats=reps, host_hd95_dc_ms=min(host_ms),
                host_repeats=host_repeats, hd95=host[0], dc=host[1], surface_voxels=s.counts["sa"] + s.counts["sb"],
                equal=bool(s.hd95 == host[0] and s.dc == host[1] and s.hd == metrics.hd(pred == 1, gt == 1)))


def bench_validation(rounds):
    import val_3D
    from networks.net_factory_3d import net_factory_3d
    from oracle import filler
    net = net_factory_3d("unet_3D", 1, 2)
    sd = filler.fill_state_dict(net.state_dict())
    sd["final.weight"] = sd["final.weight"] * 40.0                 # both classes predicted
    net.load_state_dict(sd)
    net.eval()
    shape = SHAPES[0]
    walls = {"0": [], "1": []}
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "data"))
        names = ["case_%d" % i for i in range(4)]
        for i, name in enumerate(names):
            _, gt = masks(shape, 77 + i)
            np.savez(os.path.join(tmp, "data", name + ".npz"), image=filler.image((1, 1) + shape, name)[0, 0].numpy(), label=gt)
        with open(os.path.join(tmp, "val.list"), "w") as f:
            f.write("\n".join(names) + "\n")
        run = lambda: val_3D.test_all_case(net, tmp, test_list="val.list", num_classes=2, patch_size=(96, 96, 96), stride_xy=64,
                                           stride_z=64)
        os.environ["MIS_DEVICE_METRICS"] = "1"
        run()                                                       # warm-up: plans, code objects, scratch
        for _ in range(rounds):
            for flag in ("0", "1"):
                os.environ["MIS_DEVICE_METRICS"] = flag
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                results[flag] = run()
                torch.cuda.synchronize()
                walls[flag].append(time.perf_counter() - t0)
    os.environ.pop("MIS_DEVICE_METRICS", None)
    return dict(cases=4, shape=list(shape), patch=[96, 96, 96], stride=64, rounds=rounds,
                wall_s_host_metrics=walls["0"], wall_s_device_metrics=walls["1"],
                equal=bool(np.array_equal(results["0"], results["1"])), mean_dice_hd95=results["1"].tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_metrics_bench.json"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--host_repeats", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface_metrics_bench.py needs an MI355X")
    out = dict(device=torch.cuda.get_device_name(0), host_cpus=os.cpu_count(), torch_threads=torch.get_num_threads(),
               shapes=[bench_shape(s, args.host_repeats) for s in SHAPES], validation=bench_validation(args.rounds))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
