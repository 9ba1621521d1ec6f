"""Device validation metrics (csrc/surface_metrics.hip) against the host path: scipy's exact EDT voxel by voxel, and
utils/metrics.py (dc / hd95 / hd / asd / ravd) for the scores -- EQUALITY, because every number involved is an integer or a
correctly rounded sqrt of one; only asd (a float64 sum taken in another order) gets a bound, the worst-case rounding of two
sums of n non-negative terms.  The reference is always the host code, never the code under test."""
import math
import os

import numpy as np
import pytest
import torch
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the smallest shapes at which the line passes can go wrong: odd extents; D = 1 in 3-D mode with a row longer than a workgroup;
# rows longer than one wave; a long outermost axis; a plain cube; two 2-D maps ...
# ... and the longest line the kernels take on each axis: 64 KiB of LDS per axis-pass tile, all 16 ballot chunks of the row pass
SHAPES = [(3, 5, 7), (1, 33, 257), (7, 65, 130), (260, 6, 5), (16, 16, 16), (40, 300), (13, 9),
          (1024, 2, 3), (2, 1024, 3), (2, 3, 1024)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _rng(shape, salt):
    return np.random.default_rng(1000 * salt + sum((i + 1) * e for i, e in enumerate(shape)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


# ---------------------------------------------------------------------------------------------------------------- sq_edt
@pytest.mark.parametrize("kind", ["dense", "sparse", "corner"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_sq_edt_is_scipys_edt_squared(shape, kind):
    from mis_hip import ops
    rng = _rng(shape, 1)
    if kind == "corner":
        seeds = np.zeros(shape, bool)
        seeds[(-1,) * len(shape)] = True
    else:
        seeds = rng.random(shape) < (0.5 if kind == "dense" else 0.02)
        seeds.flat[int(rng.integers(seeds.size))] = True                       # never empty
    want = np.rint(distance_transform_edt(~seeds) ** 2).astype(np.int64)
    got = ops.sq_edt(_dev(seeds))
    assert got.dtype == torch.int32 and tuple(got.shape) == shape
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)


# ---------------------------------------------------------------------------------------------------------------- scores
def _masks(shape, case):
    """(pred, gt) uint8 label maps with labels in {0, 1}."""
    rng = _rng(shape, 2)
    r = lambda p: (rng.random(shape) < p).astype(np.uint8)
    if case == "rand05":
        return r(0.5), r(0.5)
    if case == "rand02":
        return r(0.2), r(0.6)
    if case == "rand08":
        return r(0.8), r(0.8)
    if case == "identical":
        m = r(0.5)
        return m, m.copy()
    if case == "full":                       # the surface of a full mask is the array's shell
        return np.ones(shape, np.uint8), r(0.5)
    if case == "corners":                    # one voxel against the far corner: the last histogram bin
        a, b = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
        a[(0,) * len(shape)] = 1
        b[(-1,) * len(shape)] = 1
        return a, b
    if case == "faces":                      # both masks touch every face of the array
        a, b = r(0.3), r(0.3)
        for ax in range(len(shape)):
            for m, frac in ((a, 0.5), (b, 0.7)):
                for end in (0, -1):
                    sl = [slice(None)] * len(shape)
                    sl[ax] = end
                    face = m[tuple(sl)]
                    face |= (rng.random(face.shape) < frac).astype(np.uint8)
                    face.flat[0] = 1
        return a, b
    raise KeyError(case)


CASES = ["rand05", "rand02", "rand08", "identical", "full", "corners", "faces"]


def _host(a, b):
    """Host reference of one mask pair: counts with scipy's erosion, scores with utils/metrics.py."""
    from utils import metrics
    fp = generate_binary_structure(a.ndim, 1)
    sa, sb = a ^ binary_erosion(a, structure=fp), b ^ binary_erosion(b, structure=fp)
    counts = dict(a=int(a.sum()), b=int(b.sum()), ab=int((a & b).sum()), sa=int(sa.sum()), sb=int(sb.sum()))
    return counts, dict(dc=metrics.dc(a, b), hd95=metrics.hd95(a, b), hd=metrics.hd(a, b), ravd=metrics.ravd(a, b),
                        asd=metrics.asd(a, b), asd_rev=metrics.asd(b, a))


def _check_scores(pred, gt, cls):
    from utils import metrics
    a, b = (pred > 0, gt > 0) if cls < 0 else (pred == cls, gt == cls)
    counts, want = _host(a, b)
    s = metrics.device_scores(_dev(pred), _dev(gt), cls)
    assert s.counts == counts
    for k in ("dc", "hd95", "hd", "ravd"):
        got = getattr(s, k)
        print(k, got, want[k])
        assert type(got) is type(want[k])
        assert got == want[k], (k, got, want[k])
    for k, n in (("asd", counts["sa"]), ("asd_rev", counts["sb"])):
        got, bound = getattr(s, k), 2 * n * 2.0 ** -53 * want[k]
        print(k, got, want[k], abs(got - want[k]), bound)
        assert abs(got - want[k]) <= bound, (k, got, want[k], bound)
    return s


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_device_scores_equal_the_host_scores(shape, case):
    pred, gt = _masks(shape, case)
    s = _check_scores(pred, gt, 1)
    if case == "identical":
        assert s.hd95 == 0.0 and s.hd == 0.0 and s.asd == 0.0 and s.dc == 1.0
    if case == "corners":
        assert s.hd == math.sqrt(sum((e - 1) ** 2 for e in shape))
    if case == "full":
        inner = np.zeros(shape, bool)
        inner[tuple(slice(1, -1) for _ in shape)] = True
        shell = int((~inner).sum()) if len(shape) == 2 or shape[0] > 1 else int(np.prod(shape))
        assert s.counts["sa"] == shell


# (shape, seed) of density 0.2 / 0.6 masks whose 95th percentile falls BETWEEN two different distances (found by a host search;
# most random masks have d_lo == d_hi, which would leave the interpolation untested), with g on both sides of 0.5
INTERPOLATING = [((3, 5, 7), 4), ((3, 5, 7), 15), ((13, 9), 2), ((13, 9), 4), ((40, 300), 185)]


def test_union_order_statistics_differ():
    """d_lo != d_hi is asserted from the HOST distances, both branches of numpy's interpolation occur, and the device's hd95 is
    the host's in each case."""
    from utils import metrics
    below = above = 0
    for shape, seed in INTERPOLATING:
        rng = np.random.default_rng(seed)
        pred, gt = (rng.random(shape) < 0.2).astype(np.uint8), (rng.random(shape) < 0.6).astype(np.uint8)
        a, b = pred == 1, gt == 1
        u = np.sort(np.hstack((metrics._surface_distances(a, b), metrics._surface_distances(b, a))))
        lo = math.floor(0.95 * (len(u) - 1))
        assert u[lo] != u[lo + 1], (shape, seed)
        g = 0.95 * (len(u) - 1) - lo
        below += g < 0.5
        above += g >= 0.5
        _check_scores(pred, gt, 1)
    assert below and above


@pytest.mark.parametrize("shape", [(7, 65, 130), (16, 16, 16), (40, 300)], ids=["7x65x130", "16x16x16", "40x300"])
def test_multiclass_label_maps(shape):
    rng = _rng(shape, 3)
    pred = (rng.integers(0, 4, shape) * (rng.random(shape) < 0.7)).astype(np.uint8)
    gt = (rng.integers(0, 4, shape) * (rng.random(shape) < 0.6)).astype(np.uint8)
    for cls in (1, 2, 3, -1):
        _check_scores(pred, gt, cls)


@pytest.mark.parametrize("shape", [(3, 5, 7), (16, 16, 16), (13, 9)], ids=["3x5x7", "16x16x16", "13x9"])
def test_class_absent_from_one_map(shape):
    from utils import metrics
    rng = _rng(shape, 4)
    has = rng.integers(0, 3, shape).astype(np.uint8)              # labels 0, 1, 2
    lacks = np.where(has == 2, 0, has).astype(np.uint8)           # no label 2
    for pred, gt in ((has, lacks), (lacks, has), (lacks, lacks)):
        a, b = pred == 2, gt == 2
        s = metrics.device_scores(_dev(pred), _dev(gt), 2)
        assert s.dc == metrics.dc(a, b) == 0.0
        assert s.counts["a"] == int(a.sum()) and s.counts["b"] == int(b.sum())
        for name, host in (("hd95", metrics.hd95), ("hd", metrics.hd), ("asd", metrics.asd)):
            with pytest.raises(RuntimeError) as want:
                host(a, b)
            with pytest.raises(RuntimeError) as got:
                getattr(s, name)
            assert str(got.value) == str(want.value)


# ---------------------------------------------------------------------------------------- ordering and argument checks
def test_repeated_and_side_stream_calls_give_the_same_record():
    from mis_hip import ops
    pred, gt = (_dev(m) for m in _masks((7, 65, 130), "rand02"))
    first = ops.surface_metrics(pred, gt, 1).cpu()
    second = ops.surface_metrics(pred, gt, 1).cpu()
    assert torch.equal(first, second) and int(first[11]) == 1
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rec = ops.surface_metrics(pred, gt, 1)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(rec.cpu(), first)


def test_unsupported_extent_workspace_and_wrapper_refusals():
    from mis_hip import lib, ops
    from utils import metrics
    L = lib.load()
    rng = np.random.default_rng(9)
    pred, gt = (rng.random((1025, 3, 2)) < 0.5).astype(np.uint8), (rng.random((1025, 3, 2)) < 0.5).astype(np.uint8)
    dp, dg = _dev(pred), _dev(gt)
    out = torch.zeros(12, dtype=torch.int64, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    st = L.mis_surface_metrics(lib.ptr(dp), lib.ptr(dg), 1, 3, 1025, 3, 2, lib.ptr(out), lib.ptr(ws), ws.numel(), lib.stream_ptr())
    assert st == -2                                                        # MIS_ERR_UNSUPPORTED
    assert L.mis_sq_edt(lib.ptr(dp), 3, 1025, 3, 2, lib.ptr(out), lib.ptr(ws), ws.numel(), lib.stream_ptr()) == -2
    assert L.mis_surface_metrics(lib.ptr(dp), lib.ptr(dg), 1, 4, 5, 3, 2, lib.ptr(out), lib.ptr(ws), ws.numel(),
                                 lib.stream_ptr()) == -2                   # ndim outside {2, 3}
    with pytest.raises(RuntimeError, match="MIS_ERR_UNSUPPORTED"):
        ops.surface_metrics(dp, dg, 1)
    s = metrics.device_scores(dp, dg, 1)                                   # falls back to the host functions
    assert s.hd95 == metrics.hd95(pred == 1, gt == 1) and s.dc == metrics.dc(pred == 1, gt == 1)
    assert s.asd == metrics.asd(pred == 1, gt == 1) and s.hd == metrics.hd(pred == 1, gt == 1)
    # a workspace that is too small
    need = L.mis_surface_metrics_workspace_bytes(4, 5, 6)
    small = _dev(np.ones((4, 5, 6)))
    assert L.mis_surface_metrics(lib.ptr(small), lib.ptr(small), 1, 3, 4, 5, 6, lib.ptr(out), lib.ptr(ws), need - 1,
                                 lib.stream_ptr()) == -4                   # MIS_ERR_WORKSPACE
    edt = torch.zeros(4 * 5 * 6, dtype=torch.int32, device="cuda")
    assert L.mis_sq_edt(lib.ptr(small), 3, 4, 5, 6, lib.ptr(edt), lib.ptr(ws), need - 1, lib.stream_ptr()) == -4
    assert L.mis_surface_metrics(lib.ptr(small), lib.ptr(small), 1, 2, 4, 5, 6, lib.ptr(out), lib.ptr(ws), need,
                                 lib.stream_ptr()) == -1                   # ndim 2 with D != 1
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0                                       # a refused call launches nothing
    # the wrapper refuses what it would have to convert or copy
    ok = _dev(np.ones((4, 6, 8)))
    for bad in (ok.to(torch.int32), ok.float(), ok[:, :, ::2], ok.transpose(0, 2), ok.cpu()):
        with pytest.raises(RuntimeError):
            ops.surface_metrics(bad, bad, 1)
        with pytest.raises(RuntimeError):
            ops.sq_edt(bad)
    with pytest.raises(RuntimeError):
        ops.surface_metrics(ok, ok[:2].contiguous(), 1)


# --------------------------------------------------------------------------------------------------------------- callers
def _no_scipy_edt(monkeypatch):
    """The host distance transform raises: whatever still succeeds did not use it."""
    import scipy.ndimage
    from utils import metrics

    def refuse(*a, **k):
        raise AssertionError("the host distance transform ran on the device path")
    monkeypatch.setattr(scipy.ndimage, "distance_transform_edt", refuse)
    monkeypatch.setattr(metrics, "distance_transform_edt", refuse)


def test_val_2d_scores_on_the_device(monkeypatch):
    import val_2D
    from networks.net_factory import net_factory
    from oracle import filler
    g = np.load(os.path.join(GOLD, "val2d.npz"))
    C, shape = 4, (3, 40, 50)
    net = net_factory("unet", 1, C)
    sd = filler.fill_state_dict(net.state_dict())
    sd["decoder.out_conv.weight"] = sd["decoder.out_conv.weight"] * float(g["weight_scale"])     # several classes predicted
    sd["decoder.out_conv.bias"] = torch.from_numpy(g["out_bias"]).to(sd["decoder.out_conv.bias"])
    net.load_state_dict(sd)
    image = filler.image((1,) + shape, "valimg")
    label = filler.labels((1,) + shape, C, torch.uint8)
    monkeypatch.setenv("MIS_DEVICE_METRICS", "0")
    net.train()
    host = val_2D.test_single_volume(image, label, net, C, patch_size=[64, 64])
    assert net.training
    monkeypatch.delenv("MIS_DEVICE_METRICS")
    with monkeypatch.context() as m:
        _no_scipy_edt(m)
        dev = val_2D.test_single_volume(image, label, net, C, patch_size=[64, 64])
        assert net.training
        net.eval()
        again = val_2D.test_single_volume(image, label, net, C, patch_size=[64, 64])
        assert not net.training
    print(host, dev)
    assert dev == host and again == host and len(host) == C - 1
    assert [type(v) for pair in dev for v in pair] == [type(v) for pair in host for v in pair]
    assert any(h[1] > 0 for h in host), "degenerate prediction: no surface distance was scored"


def test_val_3d_scores_on_the_device(monkeypatch, tmp_path):
    import val_3D
    from networks.net_factory_3d import net_factory_3d
    from oracle import filler
    g = np.load(os.path.join(GOLD, "val3d.npz"))
    net = net_factory_3d("unet_3D", 1, 2)
    sd = filler.fill_state_dict(net.state_dict())
    sd["final.weight"] = sd["final.weight"] * float(g["weight_scale"])                           # both classes predicted
    net.load_state_dict(sd)
    (tmp_path / "data").mkdir()
    for name, shape in (("case_a", (70, 80, 66)), ("case_b", (66, 72, 70))):
        lab = np.zeros(shape, np.uint8)
        lab[10:50, 20:60, 5:40] = 1
        lab[30:60, 10:30, 30:60] = 1
        np.savez(tmp_path / "data" / (name + ".npz"), image=filler.image((1, 1) + shape, name)[0, 0].numpy(), label=lab)
    (tmp_path / "val.list").write_text("case_a\ncase_b\n")
    run = lambda **kw: val_3D.test_all_case(net, str(tmp_path), test_list="val.list", num_classes=2, patch_size=(64, 64, 64),
                                            stride_xy=32, stride_z=32, **kw)
    monkeypatch.setenv("MIS_DEVICE_METRICS", "0")
    net.train()
    host = run()
    assert net.training
    monkeypatch.delenv("MIS_DEVICE_METRICS")
    with monkeypatch.context() as m:
        _no_scipy_edt(m)
        dev = run()
        assert net.training
        net.eval()
        sums, n = run(shard=(1, 2))
        assert not net.training
    print(host, dev)
    assert host.shape == dev.shape == (1, 2) and dev.dtype == host.dtype
    assert np.array_equal(dev, host) and host[0, 0] > 0 and host[0, 1] > 0
    assert n == 1 and sums.shape == (1, 2)


def test_label_maps_of_any_integral_dtype_reach_the_device():
    """Labels stored as float with integral values (some h5 / npz datasets do) take the device path like integer ones."""
    from utils import metrics
    lab = np.random.default_rng(11).integers(0, 4, (5, 6, 7))
    for arr in (lab.astype(np.float32), lab.astype(np.float64), lab.astype(np.int64), lab.astype(np.uint8), lab > 0,
                torch.from_numpy(lab.astype(np.float32)), torch.from_numpy(lab.astype(np.int16))):
        t = metrics.device_label_map(arr)
        assert t is not None and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
        assert np.array_equal(t.cpu().numpy(), np.asarray(arr).astype(np.uint8))
