"""mis_triple_view_tail against the float64 reference of tests/triple_oracle.py, over the edge matrix of the "cross" tail in
test_loss_tails_gpu.py: C in {2, 3, 4} x uint8 / int64 labels x 2-D / 3-D / partly filled last workgroup, odd S, one case
past the 2048-workgroup cap, the splits (6,3) (5,1) (4,4) (3,0), dense / batch-strided / offset views (applied to a
different one of the three students from case to case, and to all three), the weight by float argument and by device step
state (no gate: gate 0 must change nothing), a class that never occurs, saturated logits, and planted exact arg-max ties in
each peer in turn and in two peers at once (the first maximum must win: three quarters of the pseudo labels depend on it).

Tolerance: that file's rule, unchanged.  Per compared scalar (18 per case) and per gradient tensor (3 per case):

    |hip - f64|_max <= max(K * e32, FLOOR) * |f64|_max,    K = 6

e32 = relative error of the fp32 CPU evaluation of the same oracle expression against its float64 evaluation, for the
same case and quantity.  FLOOR = the largest e32 over this matrix for that kind of quantity, computed on the CPU from the
oracle alone (``python tests/test_triple_tail_gpu.py`` prints them; no kernel takes part).  A reference of exactly 0 (no
labeled or no unlabeled rows) must be met exactly.  No case is skipped or excluded.

    FLOOR_SCALAR = 2.2e-7 (largest scalar e32: 2.10e-7, C2 saturated), FLOOR_TENSOR = 3.6e-7 (largest tensor e32: 3.57e-7,
    C3 with ties planted in students 1 and 3)

Measured on an MI355X (this file's own run):

    quantity  e32 (fp32 torch vs float64)   HIP vs float64 (max)   worst HIP / e32
    scalar    2.88e-10 .. 2.10e-7           7.47e-8                4.27  (C2, L = 0, 3-D)
    tensor    1.28e-7  .. 3.57e-7           3.57e-7                1.21  (C3, 3-D)

    Every tensor sits within 1.21 x its own e32 and every scalar below 7.5e-8, under the scalar floor.  47 cases, 4 s wall.
"""
import zlib

import pytest
import torch

import loss_tail_oracle as lto
import triple_oracle as tvo
import oracle_kit as kit
from loss_tail_cases import K, PAD, SHAPES, W, plant_ties as _plant_ties, state as _state
from oracle_kit import NAN

pytestmark = pytest.mark.gpu

FLOOR = {"scalar": 2.2e-7,      # largest scalar e32 of the matrix: 2.10e-7
         "tensor": 3.6e-7}      # largest tensor e32 of the matrix: 3.57e-7
N_OUT = 6
STATS = []


def _ops():
    from mis_hip import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for kind, r in kit.worst_rows((kind, cid, e32, ehip, e32) for cid, kind, e32, ehip in STATS):
        print(f"\n[triple tail] {kind:7s} e32 {r['lo']:.2e} .. {r['hi']:.2e}  hip max {r['hip']:.2e}  worst hip/e32 "
              f"{r['ratio']:.2f} ({r['at']})", end="")
    print()
    kit.report(STATS, "MIS_TRIPLE_TAIL_STATS")


# ---------------------------------------------------------------------------------------------------------------------
# the case matrix
# ---------------------------------------------------------------------------------------------------------------------
def _case(**kw):
    # which: the students whose logits and gradient live in the strided / offset layout; ties: the students with planted ties
    c = dict(C=3, ldt="u8", shape="2d", B=6, L=3, layout="dense", which=(0,), wmode="float", content="rand", ties=(), it=500)
    c.update(kw)
    return c


def _cid(c):
    return "-".join([f"C{c['C']}", c["ldt"], c["shape"], f"B{c['B']}", f"L{c['L']}",
                     c["layout"] + ("" if c["layout"] == "dense" else "".join(str(m + 1) for m in c["which"])),
                     c["wmode"], c["content"] + "".join(str(m + 1) for m in c["ties"])])


def _cases():
    cs = []
    for C in (2, 3, 4):
        for ldt in ("u8", "i64"):
            for shape in ("2d", "3d", "part"):
                cs.append(_case(C=C, ldt=ldt, shape=shape))
    cs += [_case(C=C, shape="odd", ldt=ldt) for C, ldt in ((2, "u8"), (3, "i64"), (4, "u8"))]
    cs += [_case(B=5, L=1, shape="3d"), _case(B=4, L=4, shape="3d", C=4), _case(B=3, L=0, shape="3d", C=2)]
    for C in (2, 3, 4):
        cs += [_case(C=C, layout="strided", ldt="i64", which=(C - 2,)),
               _case(C=C, layout="offset", shape="part", which=((C - 1) % 3,))]
    cs += [_case(layout="strided", which=(0, 1, 2), shape="odd"), _case(C=4, layout="offset", which=(0, 1, 2), shape="3d")]
    cs += [_case(wmode="state1"), _case(wmode="state0"),
           _case(C=4, wmode="state1", layout="strided", shape="3d", which=(1,))]
    cs += [_case(C=3, content="missing"), _case(C=4, content="missing", ldt="i64", shape="3d")]
    cs += [_case(C=C, content="sat") for C in (2, 3, 4)]
    cs.append(_case(C=2, shape="bigscalar", B=3, L=1))
    cs += [_case(C=2, content="ties", shape="2d", ties=(0,)), _case(C=3, content="ties", shape="odd", ties=(1,)),
           _case(C=4, content="ties", shape="3d", ties=(2,)), _case(C=3, content="ties", shape="2d", ties=(0, 2)),
           _case(C=4, content="ties", shape="part", ties=(0, 1), B=5, L=1)]
    return cs


def _matrix():
    return [pytest.param(c, id=_cid(c)) for c in _cases()]


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
def _inputs(c):
    g = torch.Generator().manual_seed(zlib.crc32(("triple" + _cid(c)).encode()))
    C, B, L, sp = c["C"], c["B"], c["L"], SHAPES[c["shape"]]
    mag = 60.0 if c["content"] == "sat" else 3.0
    label = torch.randint(0, C, (L,) + sp, generator=g)
    if c["content"] == "missing":
        label[label == C - 1] = 0
    label = label.to(torch.uint8 if c["ldt"] == "u8" else torch.int64)
    zs = [torch.randn((B, C) + sp, generator=g) * mag for _ in range(3)]
    for j in c["ties"]:
        zs[j][L:] = _plant_ties(zs[j][L:].clone(), C)
        want = lto.argmax_first(zs[j][L:], 1)
        assert torch.equal(want, torch.argmax(zs[j][L:], 1))
        flat = want.reshape(B - L, -1)
        assert (flat[:, 0::4] == 0).all() and (flat[:, 1::4] == 0).all() and (flat[:, 2::4] == 0).all()
    return dict(label=label, zs=zs)


def _references(c, x):
    w = float(torch.tensor(W, dtype=torch.float32))            # the fp32 value the kernel receives
    o64, g64 = tvo.triple_view_tail(*x["zs"], x["label"], c["L"], w)
    o32, g32 = tvo.triple_view_tail(*x["zs"], x["label"], c["L"], w, dtype=torch.float32)
    return o64, g64, [o.double() for o in o32], [g.double() for g in g32]


def _e32(c):
    """(largest scalar e32, largest tensor e32) of one case: the oracle alone."""
    x = _inputs(c)
    o64, g64, o32, g32 = _references(c, x)
    es = max(abs(a[i].item() - r[i].item()) / abs(r[i].item())
             for a, r in zip(o32, o64) for i in (0, 1, 2, 3, 5) if r[i].item() != 0.0)
    et = max(kit.rel(a, r) for a, r in zip(g32, g64))
    return es, et


# ---------------------------------------------------------------------------------------------------------------------
# the kernel call
# ---------------------------------------------------------------------------------------------------------------------
def _launch(c, x, layout, wmode, with_grad=True):
    """One call through mis_hip.ops with NaN-filled outs / dlogits / workspace; returns (outs, [(buffer, view)] * 3)."""
    ops = _ops()
    lay = [layout if m in c["which"] else "dense" for m in range(3)]
    views = [kit.place_rows(z, lay[m], PAD)[1] for m, z in enumerate(x["zs"])]
    label = x["label"].cuda()
    outs = [torch.full((16,), NAN, device="cuda") for _ in range(3)]
    grads = [kit.place_rows(None, lay[m], PAD, like=x["zs"][m]) for m in range(3)] if with_grad else []
    ops.scratch(1, "tail").view(torch.float32).fill_(NAN)
    wkw = dict(cons_weight=W) if wmode == "float" else dict(state=_state(c, wmode == "state1"))
    ops.triple_view_tail(views[0], views[1], views[2], label, c["L"], outs,
                         dlogits=[g[1] for g in grads] if with_grad else None, **wkw)
    torch.cuda.synchronize()
    return outs, grads


def _same(outs, grads, outs2, grads2):
    return (all(kit.same_bits(a, b) for a, b in zip(outs, outs2)) and
            all(kit.same_bits(a[0], b[0]) for a, b in zip(grads, grads2)))


@pytest.mark.parametrize("c", _matrix())
def test_triple_view_tail(c):
    x = _inputs(c)
    L, B = c["L"], c["B"]
    o64, g64, o32, g32 = _references(c, x)
    outs, grads = _launch(c, x, c["layout"], c["wmode"])
    # every element written once and nothing else
    for out in outs:
        assert torch.isfinite(out[:N_OUT]).all() and torch.isnan(out[N_OUT:]).all(), out
    for buf, view in grads:
        assert torch.isfinite(view).all() and kit.untouched_outside(buf, view)
    # bit-reproducible
    assert _same(outs, grads, *_launch(c, x, c["layout"], c["wmode"]))
    # forward only (dlogits=None): the same scalars
    outs3, _ = _launch(c, x, c["layout"], c["wmode"], with_grad=False)
    assert all(kit.same_bits(a, b) for a, b in zip(outs, outs3))
    # only addresses differ between a strided / offset view and the dense tensor
    if c["layout"] != "dense":
        outsd, gradsd = _launch(c, x, "dense", c["wmode"])
        assert all(kit.same_bits(a, b) for a, b in zip(outs, outsd))
        assert all(torch.equal(a[1], b[1]) for a, b in zip(grads, gradsd))
    # the weight from the device state == the weight from the float argument; there is no gate
    if c["wmode"] != "float":
        assert _same(outs, grads, *_launch(c, x, c["layout"], "float"))
    cid = _cid(c)
    w32 = torch.tensor(W, dtype=torch.float32)
    gate = kit.Gate(K, FLOOR, stats=STATS)
    for m in range(3):
        o = outs[m].cpu()
        assert kit.same_bits(o[4], w32)
        for i in (0, 1, 2, 3, 5):
            hip, ref = o[i].double().item(), o64[m][i].item()
            if ref == 0.0:
                assert hip == 0.0, (m, i, hip)
                continue
            e32, ehip = abs(o32[m][i].item() - ref) / abs(ref), abs(hip - ref) / abs(ref)
            gate.judge(cid, f"out{m + 1}[{i}]", "scalar", "max", e32, ehip, row=(cid, "scalar", e32, ehip), extra=(hip, ref))
            print(f"[triple {cid}] out{m + 1}[{i}] f64 {ref:.9e} hip {hip:.9e} e32 {e32:.2e} hip {ehip:.2e}")
        got, ref = grads[m][1].cpu().double(), g64[m]
        assert ref.abs().max().item() > 0
        e32, ehip = kit.rel(g32[m], ref), kit.rel(got, ref)
        gate.judge(cid, f"grad{m + 1}", "tensor", "max", e32, ehip, row=(cid, "tensor", e32, ehip))
        print(f"[triple {cid}] grad{m + 1} |f64|max {ref.abs().max().item():.3e} e32 {e32:.2e} hip {ehip:.2e}")
        if L == 0:
            assert o64[m][1].item() == 0.0 and o64[m][2].item() == 0.0
        if L == B:
            assert o64[m][3].item() == 0.0 and o64[m][5].item() == 0.0
    gate.done(cid)
    if 0 < L < B:
        # the two pseudo terms of a student come from different peers
        assert all(outs[m][3].item() != outs[m][5].item() for m in range(3))


def test_triple_view_tail_refusals():
    """Nothing is launched: five classes, one missing gradient buffer, a short workspace."""
    ops = _ops()
    from mis_hip import lib as _l
    sp = (1, 8, 12)
    out = [torch.full((16,), NAN, device="cuda") for _ in range(3)]
    label = torch.zeros((2,) + sp, dtype=torch.uint8, device="cuda")
    z5 = [torch.randn((4, 5) + sp, device="cuda") for _ in range(3)]
    d5 = [torch.full((4, 5) + sp, NAN, device="cuda") for _ in range(3)]
    with pytest.raises(RuntimeError, match="MIS_ERR_UNSUPPORTED"):
        ops.triple_view_tail(*z5, label, 2, out, dlogits=d5, cons_weight=W)
    z = [torch.randn((4, 3) + sp, device="cuda") for _ in range(3)]
    d = [torch.full((4, 3) + sp, NAN, device="cuda") for _ in range(3)]
    L = _l.load()
    S, row = 96, 3 * 96
    ws = ops.scratch(L.mis_triple_view_tail_workspace_bytes(4, 3, S), "tail")
    args = lambda dl, nbytes: (_l.ptr(z[0]), row, _l.ptr(z[1]), row, _l.ptr(z[2]), row, _l.ptr(label), 1, 4, 2, 3, S, W, None,
                               _l.ptr(out[0]), _l.ptr(out[1]), _l.ptr(out[2]), _l.ptr(dl[0]), row, _l.ptr(dl[1]), row,
                               _l.ptr(dl[2]), row, _l.ptr(ws), nbytes, _l.stream_ptr())
    assert L.mis_triple_view_tail(*args([d[0], None, d[2]], ws.numel())) == -1
    assert L.mis_triple_view_tail(*args(d, L.mis_triple_view_tail_workspace_bytes(4, 3, S) - 4)) == -4
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in out) and all(torch.isnan(t).all() for t in d + d5)


if __name__ == "__main__":      # the floors: the oracle alone, on the CPU
    worst_s = worst_t = 0.0
    for case in _cases():
        e_s, e_t = _e32(case)
        print(f"{_cid(case):60s} e32 scalar {e_s:.3e} tensor {e_t:.3e}")
        worst_s, worst_t = max(worst_s, e_s), max(worst_t, e_t)
    print(f"largest e32: scalar {worst_s:.3e} tensor {worst_t:.3e}")
