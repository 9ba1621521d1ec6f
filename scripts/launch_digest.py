#!/usr/bin/env python
"""Digest of the launches a training step issues, argument for argument: the check that a change to the Python layer above
the C ABI (mis_hip/lib.py, ops.py, tops.py, the plans, the trainers) left every launch as it was.

For each configuration the trainer is built with the tape off, two steps run eagerly (plans, scratch buffers and job tables
settle) and the third runs under ``lib.LaunchTape().recording()``.  Every entry of ``tape.items`` is written in a canonical form
that does not depend on where the allocator put things or on how the wrapper spelled an argument:

* a C-ABI launch: the function's name and its arguments, each read through the function's ``argtypes`` -- a pointer is ``null``
  or ``p<k>+<a>`` (k: the order in which that address first appeared in the log, a: the address modulo 16, which the kernels'
  vector paths depend on), whether it was passed as an int or as a ``c_void_p``; a float is ``float.hex``; an int is itself;
  the stream is ``s<k>``;
* a HIP event record / wait: its name, events and streams by order of appearance;
* a Python callback (the gradient exchange): its name.

One line per configuration: name, number of entries, sha256 of the log.  Two commits agree when every line is equal
(``--dump DIR`` keeps the logs themselves for a diff).  ``--host-cost`` instead times the host side of 20 eager SwinUnet
steps (no tape, no synchronisation inside the loop)."""
import argparse
import ctypes
import hashlib
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cv-ssl-mis_amd"))

import torch  # noqa: E402

from mis_hip import lib, ops, step  # noqa: E402

L, U, C = 2, 2, 4          # labeled + unlabeled samples of a batch, classes of the 2-D nets
EDGE_2D = 64               # the smallest input of the 2-D CNNs' plans
EDGE_SWIN = 224            # patch 4 x 32 (four stages) x window 7: the one size the lite SwinUnet configuration takes
EDGE_3D = 32               # the smallest edge at which unet_3D / VNet reach the Winograd and the kernel-2 / stride-2 kernels


def _nets_2d(key, n):
    from networks.net_factory import net_factory
    return [net_factory(key, 1, C) for _ in range(n)]


def _nets_3d(key, n):
    from networks.net_factory_3d import net_factory_3d
    return [net_factory_3d(key, 1, 2) for _ in range(n)]


def _batch_2d(edge):
    g = torch.Generator().manual_seed(1)
    return (torch.rand((L + U, 1, edge, edge), generator=g).cuda(),
            torch.randint(0, C, (L + U, edge, edge), generator=g).to(torch.uint8).cuda())


def _batch_3d(edge):
    g = torch.Generator().manual_seed(1)
    return (torch.rand((L + U, 1, edge, edge, edge), generator=g).cuda(),
            torch.randint(0, 2, (L + U, edge, edge, edge), generator=g).cuda())


def _mean_teacher(nets, classes):
    return step.MeanTeacherTrainer(*nets, labeled_bs=L, num_classes=classes, iter_num=1200, seed=7, use_tape=False)


def _contrastive():
    heads = _nets_2d("classifier", 2) + _nets_2d("projector", 2)
    return step.ContrastiveCrossTrainer(*_nets_2d("unet", 2), *heads, labeled_bs=L, num_classes=C, iters_per_epoch=10,
                                        iter_num=1200, seed=7, use_tape=False)


def _adversarial():
    from networks.discriminator import FC3DDiscriminator
    dan = FC3DDiscriminator(num_classes=2, pool=(EDGE_3D // 16,) * 3)
    return step.AdversarialTrainer(_nets_3d("unet_3D", 1)[0], dan, labeled_bs=L, num_classes=2, iter_num=1200, seed=7,
                                   use_tape=False)


def _adversarial_2d():
    from networks.discriminator_2d import FCDiscriminator
    dan = FCDiscriminator(num_classes=C, ndf=8, pool=(1, 1))
    return step.AdversarialTrainer(_nets_2d("unet", 1)[0], dan, labeled_bs=L, num_classes=C, iter_num=1200, seed=7,
                                   use_tape=False)


def _simple(cls, n, **kw):
    return lambda: cls(*_nets_2d("unet", n), labeled_bs=L, num_classes=C, iter_num=1200, seed=7, use_tape=False, **kw)


# name -> (trainer factory, batch factory, dispatch tags that must appear)
CONFIGS = {
    "mt/unet": (lambda: _mean_teacher(_nets_2d("unet", 2), C), lambda: _batch_2d(EDGE_2D), ()),
    "mt/pnet": (lambda: _mean_teacher(_nets_2d("pnet", 2), C), lambda: _batch_2d(EDGE_2D), ("dilated_wgrad",)),
    "mt/ViT_Seg": (lambda: _mean_teacher(_nets_2d("ViT_Seg", 2), C), lambda: _batch_2d(EDGE_SWIN), ()),
    "mt/unet_3D": (lambda: _mean_teacher(_nets_3d("unet_3D", 2), 2), lambda: _batch_3d(EDGE_3D), ("wino_wgrad",)),
    "mt/vnet": (lambda: _mean_teacher(_nets_3d("vnet", 2), 2), lambda: _batch_3d(EDGE_3D),
                ("wino_wgrad", "k2s2_down", "k2s2_up", "k2s2_wgrad")),
    "mt/attention_unet": (lambda: _mean_teacher(_nets_3d("attention_unet", 2), 2), lambda: _batch_3d(EDGE_3D), ()),
    "mt/unetr": (lambda: _mean_teacher(_nets_3d("unetr", 2), 2), lambda: _batch_3d(96), ()),
    "mt/swinunetr": (lambda: _mean_teacher(_nets_3d("swinunetr", 2), 2), lambda: _batch_3d(64), ()),
    "uamt/unet": (_simple(step.UAMTTrainer, 2), lambda: _batch_2d(EDGE_2D), ()),
    "ict/unet": (_simple(step.ICTTrainer, 2), lambda: _batch_2d(EDGE_2D), ()),
    "fixmatch/unet": (_simple(step.FixMatchTrainer, 2), lambda: _batch_2d(EDGE_2D), ()),
    "dct/unet": (_simple(step.DeepCoTrainingTrainer, 1), lambda: _batch_2d(EDGE_2D), ()),
    "cross_teaching/unet": (_simple(step.CrossTeachingTrainer, 2), lambda: _batch_2d(EDGE_2D), ()),
    "cross_teaching_ce/unet": (_simple(step.CrossTeachingTrainer, 2, pseudo_ce=True), lambda: _batch_2d(EDGE_2D), ()),
    "contrastive/unet": (_contrastive, lambda: _batch_2d(EDGE_2D), ()),
    "cnn_meet_vit/unet": (_simple(step.CnnMeetVitTrainer, 3), lambda: _batch_2d(EDGE_2D), ()),
    "triple_view/unet": (_simple(step.TripleViewTrainer, 3), lambda: _batch_2d(EDGE_2D), ()),
    "adversarial/unet_3D": (_adversarial, lambda: _batch_3d(EDGE_3D), ()),
    "adversarial/unet": (_adversarial_2d, lambda: _batch_2d(32), ()),       # conv4 leaves 2 x 2: four windows of (1, 1)
}


class _Names:
    """Things by the order of their first appearance."""

    def __init__(self, prefix):
        self.prefix, self.seen = prefix, {}

    def __call__(self, key):
        return f"{self.prefix}{self.seen.setdefault(key, len(self.seen))}"


def _address(v):
    if v is None or isinstance(v, int):
        return v or 0
    if isinstance(v, ctypes.c_void_p):
        return v.value or 0
    return None             # a byref() of a host variable


def canonical(items):
    """The log of a tape, one line per entry."""
    ptrs, handles, lines = _Names("p"), _Names("h"), []
    for fn, args in items:
        name = getattr(fn, "__name__", str(fn))
        argtypes = getattr(fn, "argtypes", None)
        if argtypes is None:                                # a Python callback of the gradient exchange
            lines.append(f"py {name}")
            continue
        assert len(argtypes) == len(args), (name, len(argtypes), len(args))
        out = []
        for i, (kind, v) in enumerate(zip(argtypes, args)):
            if name.startswith("hip") and kind is ctypes.c_void_p:
                out.append(handles(_address(v)))            # an event or a stream
            elif isinstance(v, lib.StreamPtr):
                assert i == len(args) - 1, name
                out.append("s" + handles(_address(v)))
            elif kind is ctypes.c_void_p:
                a = _address(v)
                out.append("hostref" if a is None else "null" if a == 0 else f"{ptrs(a)}+{a % 16}")
            elif kind in (ctypes.c_float, ctypes.c_double):
                out.append(float(getattr(v, "value", v)).hex())
            else:
                out.append(str(int(getattr(v, "value", v))))
        lines.append(f"{name}({', '.join(out)})")
    return lines


def record(make_trainer, make_batch):
    """tape.items of the third step of a fresh trainer, and the dispatch tags of that step."""
    getattr(ops, "_scratch", {}).clear()    # grow-only workspaces pass their size: every configuration starts from none
    trainer = make_trainer()
    volume, label = make_batch()
    for _ in range(2):
        trainer.step(volume, label)
    tape = lib.LaunchTape()
    ops.DISPATCH = set()
    try:
        with tape.recording():
            trainer.step(volume, label)
    finally:
        tags, ops.DISPATCH = ops.DISPATCH, None
    torch.cuda.synchronize()
    return tape, tags


def host_cost(steps=20):
    """Wall time of enqueueing ``steps`` eager steps of the SwinUnet configuration."""
    make_trainer, make_batch, _ = CONFIGS["mt/ViT_Seg"]
    trainer = make_trainer()
    volume, label = make_batch()
    for _ in range(3):
        trainer.step(volume, label)
    best = None
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            trainer.step(volume, label)
        dt = time.perf_counter() - t0
        torch.cuda.synchronize()
        best = dt if best is None else min(best, dt)
        print(f"host_cost: {steps} eager mt/ViT_Seg steps enqueued in {dt * 1e3:.2f} ms")
    print(f"host_cost_best_ms {best * 1e3:.2f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--only", nargs="*", help="configurations to run (default: all)")
    ap.add_argument("--dump", help="directory to write the canonical logs to")
    ap.add_argument("--host-cost", action="store_true", help="time the host side of eager SwinUnet steps instead")
    ap.add_argument("--time-limit", type=int, default=900, help="seconds for the whole run")
    args = ap.parse_args()
    signal.alarm(args.time_limit)           # one limit for the whole script: SIGALRM ends it
    if args.host_cost:
        host_cost()
        return 0
    bad = 0
    for name in args.only or CONFIGS:
        make_trainer, make_batch, want = CONFIGS[name]
        t0 = time.perf_counter()
        tape, tags = record(make_trainer, make_batch)
        lines = canonical(tape.items)
        missing = [w for w in want if not any(t.startswith(w) for t in tags)]
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            with open(os.path.join(args.dump, name.replace("/", "_") + ".log"), "w") as f:
                f.write("\n".join(lines) + "\n")
        digest = hashlib.sha256("\n".join(lines).encode()).hexdigest()
        print(f"{name:24s} {len(lines):5d} {digest}" + (f"  MISSING {missing}" if missing else ""), flush=True)
        print(f"  ({name}: {time.perf_counter() - t0:.1f} s)", file=sys.stderr, flush=True)
        bad += bool(missing)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
