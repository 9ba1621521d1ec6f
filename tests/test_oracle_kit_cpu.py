"""The harness of the float64-oracle GPU tests (tests/oracle_kit.py), held to its own contract on the CPU: a placement that
lost its guards, a gate that let a figure through or a ``bad`` list nobody asserted would make a whole GPU file pass silently."""
import json
import math

import pytest
import torch

import oracle_kit as kit

CPU = "cpu"
LEAD, TRAIL = 3, 5


def _t(*shape):
    return torch.arange(1.0, 1.0 + math.prod(shape)).reshape(shape)


# place / Out
@pytest.mark.parametrize("shape", [(2, 3, 4), (5, 7)])
def test_place_slice_is_the_input_inside_nan(shape):
    t = _t(*shape)
    v = kit.place(t, "slice", LEAD, TRAIL, device=CPU)
    assert torch.equal(v, t) and tuple(v.shape) == shape
    assert v.storage_offset() == LEAD * v.stride(1)
    assert v.data_ptr() == v.untyped_storage().data_ptr() + LEAD * v.stride(1) * 4
    buf = torch.empty(0).set_(v.untyped_storage()).reshape((shape[0], LEAD + shape[1] + TRAIL) + shape[2:])
    assert torch.isnan(buf[:, :LEAD]).all() and torch.isnan(buf[:, LEAD + shape[1]:]).all()
    assert int(torch.isnan(buf).sum()) == buf.numel() - t.numel()
    d = kit.place(t, "dense", LEAD, TRAIL, device=CPU)                        # dense: a copy; None passes through
    assert torch.equal(d, t) and d.is_contiguous() and d.data_ptr() != t.data_ptr()
    assert kit.place(None, "slice", LEAD, TRAIL, device=CPU) is None


@pytest.mark.parametrize("layout", ["dense", "slice"])
def test_place_rows_behind_are_nan_in_the_same_allocation(layout):
    t = _t(5, 7)
    v = kit.place(t, layout, LEAD, TRAIL, rows_behind=2, device=CPU)
    lead, trail = (LEAD, TRAIL) if layout == "slice" else (0, 0)
    assert torch.equal(v, t)
    buf = torch.empty(0).set_(v.untyped_storage()).reshape(5 + 2, lead + 7 + trail)
    assert torch.isnan(buf[5:]).all() and int(torch.isnan(buf).sum()) == buf.numel() - t.numel()
    assert v.data_ptr() == v.untyped_storage().data_ptr() + lead * 4 and v.stride(0) == lead + 7 + trail


@pytest.mark.parametrize("shape", [(2, 3, 4), (5, 7)])
def test_out_slice_guards(shape):
    o = kit.Out(shape, "slice", LEAD, TRAIL, device=CPU)
    assert tuple(o.v.shape) == shape and torch.isnan(o.v).all()
    assert o.v.data_ptr() == o.buf.data_ptr() + LEAD * o.buf.stride(1) * 4
    assert int((o.buf == kit.SENT).sum()) == o.buf.numel() - o.v.numel()
    assert o.untouched()
    o.v.fill_(1.0)                                   # writing the view itself is what a kernel is for
    assert o.untouched()
    d = kit.Out(shape, "dense", LEAD, TRAIL, device=CPU)
    assert d.buf is None and torch.isnan(d.v).all() and d.untouched() and d.v.zero_() is d.v and d.untouched()
    o.buf[0, LEAD - 1].view(-1)[-1] = 0.0            # one write into the lead guard
    assert not o.untouched()
    o = kit.Out(shape, "slice", LEAD, TRAIL, device=CPU)
    o.buf[-1, LEAD + shape[1]].view(-1)[0] = float("nan")      # one write into the trail guard
    assert not o.untouched()


def test_out_fill_and_nan():
    f = _t(2, 3, 4).double()
    o = kit.Out((2, 3, 4), "slice", LEAD, TRAIL, fill=f, device=CPU)
    assert torch.equal(o.v, f.float()) and o.untouched()
    assert kit.nan(2, 3, device=CPU).isnan().all()


# place_rows / logical
@pytest.mark.parametrize("layout,off,pad", [("dense", 0, 0), ("strided", 0, 8), ("offset", 2, 8)])
def test_place_rows(layout, off, pad):
    t = _t(3, 2, 1, 4, 5)
    buf, view = kit.place_rows(t, layout, 8, device=CPU)
    row = 2 * 4 * 5
    assert tuple(buf.shape) == (3 + off, row + pad) and torch.equal(view, t)
    assert view.data_ptr() == buf.data_ptr() + off * (row + pad) * 4 and view.stride(0) == row + pad
    assert torch.equal(kit.logical(buf, view), t.reshape(3, row))
    assert kit.untouched_outside(buf, view) and int(torch.isnan(buf).sum()) == buf.numel() - t.numel()
    view[1, 1, 0, 2, 3] = -5.0                        # the view aliases the buffer
    assert kit.logical(buf, view)[1, 20 + 2 * 5 + 3] == -5.0 and kit.untouched_outside(buf, view)
    if layout != "dense":
        buf[-1, -1] = 0.0                             # one write into the padding
        assert not kit.untouched_outside(buf, view)
    nbuf, nview = kit.place_rows(None, layout, 8, like=t, device=CPU)
    assert tuple(nview.shape) == tuple(t.shape) and torch.isnan(nbuf).all()


def test_place_rows_refuses_a_layout_it_cannot_serve_as_a_view():
    """Every layout it knows is a row slice of one buffer, taken with .view(), which never copies; anything else (fixmatch's
    ``shift1``, patch_nce's ``dstride``) would need another buffer and raises instead of falling back to a padded copy."""
    for layout in ("shift1", "dstride", "slice"):
        with pytest.raises(ValueError):
            kit.place_rows(_t(3, 4), layout, 8, device=CPU)


# Gate
K, FLOOR = 6.0, {"y": 1e-6, "dw": 5e-6}


def test_gate_boundary_floor_factor_and_rows():
    stats = []
    g = kit.Gate(K, FLOOR, stats=stats)
    e32 = 1e-6
    tol = g.judge("c", "y", "y", "max", e32, K * e32)
    assert tol == K * e32 and g.bad == []                          # hip == tol passes
    g.judge("c", "y", "y", "rms", e32, math.nextafter(K * e32, math.inf))
    assert [(b[0], b[1]) for b in g.bad] == [("y", "rms")]         # the next float above it does not
    g.bad.clear()
    assert g.judge("c", "dw", "dw", "max", 1e-8, 5e-6) == 5e-6 and g.bad == []      # K * e32 < floor: the floor decides
    g.judge("c", "dw", "dw", "max", 1e-8, math.nextafter(5e-6, math.inf))
    g.judge("c", "y", "y", "max", 1e-8, 5e-6)                      # ... the floor of its own kind: 5e-6 > FLOOR["y"]
    assert [(b[0], b[1]) for b in g.bad] == [("dw", "max"), ("y", "max")]
    g.bad.clear()
    assert g.judge("c", "y", "y", "max", e32, 17 * K * e32, factor=17.0) == K * e32 * 17.0 and g.bad == []
    g.judge("c", "y", "y", "max", e32, 17 * K * e32, factor=16.0)
    assert len(g.bad) == 1
    g.bad.clear()
    g.judge("c", "y", "y", "max", e32, float("nan"))               # a NaN figure fails
    assert len(g.bad) == 1
    g.bad.clear()
    g.judge("c", "y", "y", "max", e32, 0.0, ok=False)              # the verdict of an element-wise measure
    g.judge("c", "y", "y", "max", e32, 1.0, ok=True, row=("mine",))
    assert [(b[0], b[1]) for b in g.bad] == [("y", "max")]
    assert len(stats) == 10 and stats[0] == ("c", "y", "y", "max", e32, K * e32) and stats[-1] == ("mine",)
    with pytest.raises(KeyError):
        g.judge("c", "y", "no such kind", "max", e32, 0.0)


def test_gate_finite_zero_ok_and_tensor():
    stats = []
    g = kit.Gate(K, FLOOR, stats=stats)
    g.finite(torch.ones(3), "x")
    g.zero_ok(torch.tensor(True), "x")
    with pytest.raises(AssertionError, match="exactly 0"):
        g.zero_ok(False, "x")
    ref = torch.tensor([[1.0, 0.0], [2.0, 0.0]], dtype=torch.float64)
    measure = lambda got, r: {"max": kit.rel(got, r), "rms": 0.0, "zero_ok": bool((got[r == 0] == 0).all())}
    for v in (float("inf"), float("nan")):
        with pytest.raises(AssertionError, match="not finite"):
            g.finite(torch.tensor([1.0, v]), "x")
        with pytest.raises(AssertionError, match="not finite"):
            g.tensor("c", "y", "y", torch.tensor([1.0, 0.0, v, 0.0]), ref, measure, {"max": 1e-6}, ("c",))
    with pytest.raises(AssertionError, match="exactly 0"):
        g.tensor("c", "y", "y", torch.tensor([1.0, 1e-30, 2.0, 0.0]), ref, measure, {"max": 1e-6}, ("c",))
    assert stats == [] and g.bad == []
    m = g.tensor("c", "y+", "y", torch.tensor([1.0, 0.0, 2.5, 0.0]), ref, measure, {"max": 1e-6, "rms": 1e-7}, ("grp", "c"), ("k<1>",))
    assert m["max"] == 0.25 and [(b[0], b[1], b[-1]) for b in g.bad] == [("y+", "max", "k<1>")]
    assert stats == [("grp", "c", "y+", "y", "max", 1e-6, 0.25, "k<1>"), ("grp", "c", "y+", "y", "rms", 1e-7, 0.0, "k<1>")]
    assert g.tensor("c", "y", "y", ref.float(), ref, measure, {}, ())["max"] == 0.0 and len(stats) == 2     # measured, not judged


def test_gate_done_is_strict():
    g = kit.Gate(K, FLOOR)
    g.judge("c", "y", "y", "max", 1e-6, 1e-6)
    g.done("c")                                                    # nothing over the gate
    g.judge("c", "y", "y", "max", 1e-6, 1.0)
    with pytest.raises(AssertionError):
        g.done("c")                                                # a non-empty bad list
    known = {"c": {("dx", "max")}}

    def run(case, dx, y):
        g = kit.Gate(K, FLOOR, known, [])
        g.judge(case, "dx", "y", "max", 1e-6, dx)
        g.judge(case, "dx", "y", "rms", 1e-6, 1e-6)
        g.judge(case, "y", "y", "max", 1e-6, y)
        g.done(case, sync=False)

    with pytest.raises(pytest.xfail.Exception):
        run("c", 1.0, 1e-6)                                        # exactly the known entry is over: xfail
    with pytest.raises(AssertionError, match="expected over the gate"):
        run("c", 1e-6, 1e-6)                                       # the known entry passes
    with pytest.raises(AssertionError, match="expected over the gate"):
        run("c", 1.0, 1.0)                                         # a further entry is over as well
    with pytest.raises(AssertionError):
        run("another case", 1.0, 1e-6)                             # known for another case only
    run("another case", 1e-6, 1e-6)


# report, one_thread, the small helpers
def test_report(tmp_path, monkeypatch):
    stats = [("a", 1.5e-7, 2.0), ("b", 0.0, 1.0)]
    monkeypatch.delenv("MIS_KIT_TEST_STATS", raising=False)
    kit.report(stats, "MIS_KIT_TEST_STATS")
    assert list(tmp_path.iterdir()) == []
    path = tmp_path / "stats.json"
    monkeypatch.setenv("MIS_KIT_TEST_STATS", str(path))
    kit.report(stats, "MIS_KIT_TEST_STATS")
    assert json.loads(path.read_text()) == [list(r) for r in stats]
    payload = {"stats": stats, "triple": [], "K": 6.0}
    kit.report(stats, "MIS_KIT_TEST_STATS", payload)
    assert path.read_text() == json.dumps(payload)


def test_one_thread_restores_the_thread_count():
    before = torch.get_num_threads()
    torch.set_num_threads(2)
    try:
        assert kit.one_thread(lambda a, b=0: (torch.get_num_threads(), a + b), 1, b=2) == (1, 3)
        assert torch.get_num_threads() == 2

        def boom():
            raise KeyError("boom")
        with pytest.raises(KeyError):
            kit.one_thread(boom)
        assert torch.get_num_threads() == 2
    finally:
        torch.set_num_threads(before)


def test_worst_rows():
    rows = kit.worst_rows([("b", "c1", 1e-7, 3e-7, 1e-7), ("a", "c2", 2e-7, 1e-7, 2e-7), ("b", "c3", 4e-8, 2e-7, 4e-8),
                           ("b", "c4", 0.0, 5e-7, 0.0)])
    assert [k for k, _ in rows] == ["a", "b"]
    assert rows[1][1] == dict(lo=0.0, hi=1e-7, hip=5e-7, ratio=2e-7 / 4e-8, at="c3") and rows[0][1]["ratio"] == 0.5


def test_bits_rel_ceil2_kernel_name():
    a = torch.tensor([0.0, 1.0, float("nan")])
    assert kit.same_bits(a, a.clone()) and not kit.same_bits(a, torch.tensor([-0.0, 1.0, float("nan")]))
    assert kit.same_bits(_t(4, 6)[:, :3], _t(4, 6)[:, :3].contiguous())
    ref = torch.tensor([1.0, -4.0], dtype=torch.float64)
    assert kit.rel(torch.tensor([1.0, -3.0]), ref) == 0.25
    assert kit.rel(torch.ones(2), torch.zeros(2, dtype=torch.float64)) == 0.0
    assert kit.ceil2(1.11e-7) == 1.2e-7 and kit.ceil2(1.2e-7) == 1.2e-7 and kit.ceil2(0.0) == 0.0

    def query(n, buf, size):
        buf.value = b"kernel<%d>" % n if size >= 16 else b""
        return 0 if n else -2
    assert kit.kernel_name(query, 7) == "kernel<7>" and kit.kernel_name(query, 7, size=8) == ""
    with pytest.raises(AssertionError):
        kit.kernel_name(query, 0)
