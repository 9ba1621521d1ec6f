"""Device validation metrics, host side: numpy's percentile rule restated over two order statistics, the decoding of the
device's result record into medpy's scores (the record is emulated here with numpy/scipy, field by field as
include/mis_hip.h defines it), and the C ABI's declarations.  No GPU is touched."""
import math
import os
import re
import struct

import numpy as np
import pytest
import torch
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_percentile_from_order_stats_is_numpys_percentile_exactly():
    """>= 10 000 seeded multisets of sqrt(int) values, n = 1 .. 60: equality, not closeness; both branches of numpy's
    interpolation are exercised with d_lo != d_hi."""
    from utils.metrics import percentile_from_order_stats
    rng = np.random.default_rng(20260)
    low_branch = high_branch = 0
    for trial in range(12000):
        n = int(rng.integers(1, 61))
        top = int(rng.choice([3, 30, 3000, 300000]))
        x = np.sqrt(rng.integers(0, top, n).astype(np.float64))
        s = np.sort(x)
        lo = math.floor(0.95 * (n - 1))
        hi = min(lo + 1, n - 1)
        got = percentile_from_order_stats(float(s[lo]), float(s[hi]), n, 95)
        want = float(np.percentile(x, 95))
        assert got == want, (trial, n, got, want)
        g = 0.95 * (n - 1) - lo
        if s[lo] != s[hi]:
            low_branch += g < 0.5
            high_branch += g >= 0.5
    assert low_branch > 100 and high_branch > 100, (low_branch, high_branch)


def test_percentile_from_order_stats_other_q():
    from utils.metrics import percentile_from_order_stats
    rng = np.random.default_rng(7)
    for q in (0, 50, 95, 100):
        for n in (1, 2, 7, 20):
            x = np.sqrt(rng.integers(0, 500, n).astype(np.float64))
            s = np.sort(x)
            lo = math.floor(q / 100 * (n - 1))
            assert percentile_from_order_stats(float(s[lo]), float(s[min(lo + 1, n - 1)]), n, q) == float(np.percentile(x, q))


def emulated_record(pred, gt, cls):
    """The 12-field record of mis_surface_metrics from numpy/scipy (a CPU tensor)."""
    a, b = (pred > 0, gt > 0) if cls < 0 else (pred == cls, gt == cls)
    fp = generate_binary_structure(a.ndim, 1)
    sa, sb = a ^ binary_erosion(a, structure=fp), b ^ binary_erosion(b, structure=fp)
    rec = [int(a.sum()), int(b.sum()), int((a & b).sum()), int(sa.sum()), int(sb.sum())]
    valid = rec[0] > 0 and rec[1] > 0
    mx, sums, sq_lo, sq_hi = [-1, -1], [0.0, 0.0], -1, -1
    if valid:
        ab = np.rint(distance_transform_edt(~sb)[sa] ** 2).astype(np.int64)       # dA -> dB
        ba = np.rint(distance_transform_edt(~sa)[sb] ** 2).astype(np.int64)
        for k, v in enumerate((ab, ba)):
            bins = np.bincount(v)
            mx[k] = int(v.max())
            sums[k] = float(sum(int(c) * math.sqrt(q) for q, c in enumerate(bins) if c))
        u = np.sort(np.concatenate((ab, ba)))
        lo = math.floor(0.95 * (len(u) - 1))
        sq_lo, sq_hi = int(u[lo]), int(u[min(lo + 1, len(u) - 1)])
    raw = struct.pack("<7q2d3q", *rec, mx[0], mx[1], sums[0], sums[1], sq_lo, sq_hi, int(valid))
    return torch.frombuffer(bytearray(raw), dtype=torch.int64)


@pytest.mark.parametrize("shape", [(5, 9, 11), (1, 12, 13), (14, 17)])
def test_scores_decode_the_record_to_the_host_functions_values(shape):
    from utils import metrics
    rng = np.random.default_rng(3)
    pred = (rng.random(shape) < 0.2).astype(np.uint8) * rng.integers(1, 4, shape).astype(np.uint8)
    gt = (rng.random(shape) < 0.6).astype(np.uint8) * rng.integers(1, 4, shape).astype(np.uint8)
    for cls in (-1, 1, 2, 3):
        a, b = (pred > 0, gt > 0) if cls < 0 else (pred == cls, gt == cls)
        s = metrics.SurfaceScores(record=emulated_record(pred, gt, cls))
        assert s.dc == metrics.dc(a, b) and s.ravd == metrics.ravd(a, b)
        assert s.hd95 == metrics.hd95(a, b) and s.hd == metrics.hd(a, b)
        for got, want, n in ((s.asd, metrics.asd(a, b), s.counts["sa"]), (s.asd_rev, metrics.asd(b, a), s.counts["sb"])):
            assert abs(got - want) <= 2 * n * 2.0 ** -53 * want
        assert s.counts == metrics._host_counts(a, b)


def test_scores_raise_like_the_host_functions_on_empty_masks():
    from utils import metrics
    full = np.ones((4, 5, 6), np.uint8)
    none = np.zeros((4, 5, 6), np.uint8)
    for pred, gt in ((none, full), (full, none), (none, none)):
        s = metrics.SurfaceScores(record=emulated_record(pred, gt, 1))
        assert s.dc == metrics.dc(pred == 1, gt == 1) == 0.0
        for name, host in (("hd95", metrics.hd95), ("hd", metrics.hd), ("asd", metrics.asd)):
            with pytest.raises(RuntimeError) as want:
                host(pred == 1, gt == 1)
            with pytest.raises(RuntimeError) as got:
                getattr(s, name)
            assert str(got.value) == str(want.value)
        with pytest.raises(RuntimeError) as want:
            metrics.asd(gt == 1, pred == 1)
        with pytest.raises(RuntimeError) as got:
            s.asd_rev
        assert str(got.value) == str(want.value)
        if gt.any():
            assert s.ravd == metrics.ravd(pred == 1, gt == 1)
        else:
            with pytest.raises(RuntimeError, match="second supplied array"):
                s.ravd


def test_host_fallback_scores_and_switch(monkeypatch):
    from utils import metrics
    rng = np.random.default_rng(5)
    a, b = rng.random((3, 6, 7)) < 0.4, rng.random((3, 6, 7)) < 0.5
    s = metrics.SurfaceScores(host=(a, b))
    assert (s.dc, s.hd95, s.hd, s.asd, s.asd_rev, s.ravd) == (metrics.dc(a, b), metrics.hd95(a, b), metrics.hd(a, b),
                                                               metrics.asd(a, b), metrics.asd(b, a), metrics.ravd(a, b))
    assert not metrics.device_supported((1025, 4, 4)) and not metrics.device_supported((2, 2, 2, 2))
    assert metrics.device_supported((1024, 1, 3)) and metrics.device_supported((9, 9)) and not metrics.device_supported((7,))
    monkeypatch.delenv("MIS_DEVICE_METRICS", raising=False)
    assert metrics.device_metrics_enabled()
    monkeypatch.setenv("MIS_DEVICE_METRICS", "0")
    assert not metrics.device_metrics_enabled()


def test_surface_metrics_c_abi_is_declared():
    from mis_hip import lib
    header = open(os.path.join(ROOT, "include", "mis_hip.h")).read()
    names = {"mis_surface_metrics_workspace_bytes", "mis_surface_metrics", "mis_sq_edt"}
    assert names <= set(re.findall(r"\b(mis_[a-z0-9_]+)\s*\(", header))
    assert names <= set(lib.PROTOTYPES)
    for cite in ("code/val_2D.py:7-15", "code/val_3D.py:82-88", "code/test_3D_util.py:147-152", "code/test_CNNVIT.py:33-39"):
        assert cite in header, cite                      # the prototypes cite the reference lines they replace
    L = lib.load()
    small, big = L.mis_surface_metrics_workspace_bytes(1, 8, 8), L.mis_surface_metrics_workspace_bytes(155, 240, 240)
    assert 0 < small < big
    assert L.mis_surface_metrics_workspace_bytes(1025, 8, 8) == -2 and L.mis_surface_metrics_workspace_bytes(0, 8, 8) == -1
    # argument validation happens before any launch
    assert L.mis_surface_metrics(None, None, 1, 3, 4, 4, 4, None, None, 0, None) == -1
    assert L.mis_sq_edt(None, 3, 4, 4, 4, None, None, 0, None) == -1


def test_label_maps_the_device_cannot_take_are_refused_before_any_upload():
    from utils.metrics import device_label_map
    ok = np.ones((3, 4), np.float32)
    bad = [ok * 0.5, ok * 256, -ok, ok * np.nan, np.full((3, 4), 300, np.int64), np.full((3, 4), -1, np.int8),
           np.zeros((1025, 2), np.uint8), np.zeros((2, 2, 2, 2), np.uint8), np.zeros((3, 4), np.complex64),
           torch.full((2, 2), -1), torch.full((2, 2), 1.5)]
    for arr in bad:
        assert device_label_map(arr) is None
