"""Every fused loss tail against the float64 reference of tests/loss_tail_oracle.py, over one edge matrix: C in {2, 3, 4},
uint8 / int64 labels, 2-D / 3-D / partly filled last workgroup / past the 2048-workgroup cap / odd S (scalar tail), the
labeled / unlabeled splits including L == B and L == 0, dense / batch-strided / offset views, the weight by float argument
and by device step state (gate on and off), loss_scale, a class that never occurs, saturated logits and planted arg-max ties.

Tolerance (the float64 arbiter of test_parity_gpu.py, F64_K = 6), per compared scalar and per gradient tensor:

    |hip - f64|_max <= max(K * e32, FLOOR) * |f64|_max,    K = 6

e32 = relative error of the fp32 CPU evaluation of the same oracle expression against its float64 evaluation, for the
same case and quantity.  FLOOR = the largest e32 seen over the whole matrix for that kind of quantity (one for scalars,
one for tensors): no case is held tighter than fp32 torch itself manages on the hardest case.  A reference of exactly 0
(gated-off consistency, no unlabeled rows, everything masked out) must be met exactly.

Measured on an MI355X (this file's own run; `MIS_TAIL_STATS=<file>` writes every figure as JSON):

    tail     quantity  e32 (fp32 torch vs float64)   HIP vs float64 (max)   worst HIP / e32
    mt       scalar    0        .. 1.78e-7           1.15e-7                46.6  (e32 = 1.5e-9 there; floor)
    mt       tensor    1.20e-7  .. 5.04e-7           5.61e-7                1.13
    cross    scalar    4.9e-12  .. 2.04e-7           1.16e-7                5.46
    cross    tensor    1.17e-7  .. 3.59e-7           3.59e-7                1.22
    uamt     scalar    0        .. 2.25e-7           1.11e-7                18.0  (floor)
    uamt     tensor    1.30e-7  .. 6.34e-7           6.34e-7                1.16
    ict      scalar    0        .. 2.52e-7           9.85e-8                11.3  (floor)
    ict      tensor    1.28e-7  .. 4.62e-7           4.30e-7                1.29
    dct      scalar    1.9e-11  .. 1.85e-7           1.37e-7                4572  (e32 = 1.9e-11 there; floor)
    dct      tensor    1.26e-7  .. 7.69e-7           8.04e-7                1.30
    softmax_mean_accumulate    1.02e-7  .. 1.36e-7   1.36e-7                1.19

    FLOOR_SCALAR = 2.6e-7 (largest scalar e32: 2.52e-7, ict), FLOOR_TENSOR = 7.7e-7 (largest tensor e32: 7.69e-7, dct).
    "cross" covers the three forms (Dice / CE pseudo-supervision / with the EMA teacher).  Every tensor sits within 1.3 x its
    own e32 (K = 6 is never needed); every scalar is below 1.4e-7, under the scalar floor: the scalar ratios above 6 are
    cases where the fp32 evaluation happens to round to the float64 value (e32 << 2^-24), which the floor is for.
    304 cases, 8 s wall.

The gate: mis_loss_tail, mis_ict_tail and mis_dct_tail read cons_gate of the step state (gate 0: consistency_loss reads 0,
out[4] still the weight, zero gradient on the unlabeled rows).  The cross and UA-MT tails take only cons_weight from the
state (include/mis_hip.h: their callers fold any gate into the weights); for them gate 0 must change nothing.
mis_cross_*_tail has no loss_scale argument, mis_dct_tail is 2-D only (odd rotations need square planes) and needs L, U > 0.
"""
import functools
import zlib

import pytest
import torch

import loss_tail_oracle as lto
from loss_tail_cases import K, MAX_IT, PAD, SHAPES, W, plant_ties as _plant_ties, state as _state
import oracle_kit as kit
from oracle_kit import NAN

pytestmark = pytest.mark.gpu

FLOOR = {"scalar": 2.6e-7,      # largest scalar e32 of the matrix: 2.52e-7 (ict)
         "tensor": 7.7e-7}      # largest tensor e32 of the matrix: 7.69e-7 (dct)
W_MT = 0.11
N_OUT = {"mt": lambda C: 5 + C, "cross": lambda C: 5, "cross_ce": lambda C: 5, "cross_mt": lambda C: 7,
         "uamt": lambda C: 7 + C, "ict": lambda C: 5 + C, "dct": lambda C: 6 + C}
GATED = ("mt", "ict", "dct")
STATS = []


def _ops():
    from mis_hip import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if not STATS:
        return
    for (tail, kind), r in kit.worst_rows(((tail.split("_")[0], kind), cid, e32, ehip, e32) for tail, cid, kind, e32, ehip in STATS):
        print(f"\n[loss tails] {tail:6s} {kind:7s} e32 {r['lo']:.2e} .. {r['hi']:.2e}  hip max {r['hip']:.2e}  "
              f"worst hip/e32 {r['ratio']:.2f} ({r['at']})", end="")
    print()
    kit.report(STATS, "MIS_TAIL_STATS")


# ---------------------------------------------------------------------------------------------------------------------
# the case matrix
# ---------------------------------------------------------------------------------------------------------------------
def _case(**kw):
    c = dict(C=3, ldt="u8", shape="2d", B=6, L=3, layout="dense", wmode="float", scale=1.0, content="rand", it=500)
    c.update(kw)
    return c


def _cid(c):
    return "-".join(f"{k}{c[k]}" if k in ("C", "B", "L", "it") else str(c[k])
                    for k in ("C", "ldt", "shape", "B", "L", "layout", "wmode", "scale", "content", "it"))


def _matrix(tail):
    vec = not tail.startswith("cross")
    scaled = vec                                            # mis_cross_*_tail has no loss_scale
    cs = []
    for C in (2, 3, 4):
        for ldt in ("u8", "i64"):
            for shape in ("2d", "3d", "part"):
                cs.append(_case(C=C, ldt=ldt, shape=shape))
    if not vec:
        cs += [_case(C=C, shape="odd", ldt=ldt) for C, ldt in ((2, "u8"), (3, "i64"), (4, "u8"))]
    cs += [_case(B=5, L=1, shape="3d"), _case(B=4, L=4, shape="3d", C=4), _case(B=3, L=0, shape="3d", C=2)]
    for C in (2, 3, 4):
        cs += [_case(C=C, layout="strided", ldt="i64"), _case(C=C, layout="offset", shape="part")]
    cs += [_case(wmode="state1"), _case(wmode="state0"), _case(C=4, wmode="state1", layout="strided", shape="3d")]
    if scaled:
        cs += [_case(C=2, scale=0.25), _case(C=4, scale=0.25, wmode="state1", layout="offset", shape="3d")]
    cs += [_case(C=3, content="missing"), _case(C=4, content="missing", ldt="i64", shape="3d")]
    cs += [_case(C=C, content="sat") for C in (2, 3, 4)]
    if tail in ("mt", "uamt"):
        cs.append(_case(C=2, shape="bigvec", B=3, L=1))
    if tail == "cross":
        cs.append(_case(C=2, shape="bigscalar", B=3, L=1))
        cs += [_case(C=C, content="ties", shape=s) for C, s in ((2, "2d"), (3, "odd"), (4, "3d"))]
    if tail == "cross_ce":
        cs += [_case(C=C, content="ties", shape=s) for C, s in ((2, "odd"), (3, "2d"), (4, "part"))]
    if tail == "uamt":                                      # L < B is required (the L == B refusal has its own test)
        cs = [c for c in cs if c["L"] < c["B"]]
        cs += [_case(C=2, it=0), _case(C=2, it=MAX_IT), _case(C=3, it=0), _case(C=3, it=MAX_IT), _case(C=4, it=0),
               _case(C=4, it=MAX_IT, ldt="i64"), _case(C=3, it=0, content="allout"),
               _case(C=4, it=MAX_IT, content="allout", layout="strided")]
    if tail == "ict":
        cs = [c for c in cs if c["L"] < c["B"]]
    if tail == "dct":                                       # 2-D, L > 0 and U > 0; odd rotations on the square plane
        cs = [dict(c, shape="sq") if c["shape"] == "3d" else c for c in cs if 0 < c["L"] < c["B"]]
    if tail in ("cross_ce", "cross_mt"):                    # same kernels as "cross": every C, one shape per label type
        cs = [c for c in cs if c["shape"] != "3d" or c["content"] != "rand" or c["layout"] != "dense"
              or c["wmode"] != "float" or (c["B"], c["L"]) != (6, 3)]
    if tail == "cross_mt":                                  # the teacher term needs unlabeled rows
        cs = [c for c in cs if c["L"] < c["B"]]
    return [pytest.param(c, id=_cid(c)) for c in cs]


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
def _inputs(tail, c):
    """CPU fp32 operands of one case: logits operands by name (``ops``: name -> [n, C, D, H, W]), label, extras."""
    g = torch.Generator().manual_seed(zlib.crc32((tail + _cid(c)).encode()))
    C, B, L, sp = c["C"], c["B"], c["L"], SHAPES[c["shape"]]
    U = B - L
    mag = 60.0 if c["content"] == "sat" else 3.0
    r = lambda n: torch.randn((n, C) + sp, generator=g) * mag
    label = torch.randint(0, C, (L,) + sp, generator=g)
    if c["content"] == "missing":
        label[label == C - 1] = 0
    label = label.to(torch.uint8 if c["ldt"] == "u8" else torch.int64)
    x = dict(label=label, ops={"s": r(B)})
    if tail == "mt":
        x["ops"]["t"] = r(U) if U else None
    elif tail.startswith("cross"):
        x["ops"]["o"] = r(B)
        if c["content"] == "ties" and U:
            x["ops"]["o"][L:] = _plant_ties(x["ops"]["o"][L:].clone(), C)
        if tail == "cross_mt":
            x["ops"]["t"] = r(U)
    elif tail == "uamt":
        x["ops"]["t"] = r(U)
        thr = lto.uamt_threshold(c["it"], MAX_IT)
        if c["content"] == "allout":                        # uniform rows: entropy ln C >= ln 3 > thr for C >= 3
            assert C >= 3
            x["ops"]["pm"] = torch.full((U, C) + sp, 1.0 / C)
        else:
            x["ops"]["pm"] = lto.uamt_mean_probs(U, C, sp, thr, g)
        # the condition of the mask: NO voxel within fp32 rounding of the threshold, checked before any kernel runs
        assert not lto.uamt_undecided(x["ops"]["pm"], thr).any()
    elif tail == "ict":
        x["ops"]["t0"], x["ops"]["t1"] = r(U), r(U)
        x["lam"] = torch.rand(U, generator=g)
    elif tail == "dct":
        x["ops"]["r"] = r(U)
        x["k"] = (zlib.crc32(_cid(c).encode()) % 4) if sp[1] == sp[2] else 2 * (zlib.crc32(_cid(c).encode()) % 2)
    return x


def _oracle(tail, c, x, dtype, gate):
    """(out, [gradients]) of the reference in ``dtype``; the weight is the fp32 value the kernel receives."""
    o, L, lab = x["ops"], c["L"], x["label"]
    w = float(torch.tensor(W, dtype=torch.float32))
    if tail == "mt":
        out, g = lto.mean_teacher_tail(o["s"], o["t"], lab, L, w, gate, c["scale"], dtype)
    elif tail in ("cross", "cross_ce"):
        out, g = lto.cross_tail(o["s"], o["o"], lab, L, w, pseudo_ce=tail == "cross_ce", dtype=dtype)
    elif tail == "cross_mt":
        out, g = lto.cross_tail(o["s"], o["o"], lab, L, w, teacher=o["t"],
                                mt_weight=float(torch.tensor(W_MT, dtype=torch.float32)), dtype=dtype)
    elif tail == "uamt":
        out, g = lto.uamt_tail(o["s"], o["t"], o["pm"], lab, L, w, c["it"], MAX_IT, c["scale"], dtype)
    elif tail == "ict":
        out, g = lto.ict_tail(o["s"], o["t0"], o["t1"], x["lam"], lab, L, w, gate, c["scale"], dtype)
    else:
        out, ga, gr = lto.dct_tail(o["s"][:, :, 0], o["r"][:, :, 0], lab[:, 0], L, x["k"], w, gate, c["scale"], dtype)
        return out, [ga.unsqueeze(2), gr.unsqueeze(2)]
    return out, [g]


def _references(tail, c, x, gate=1.0):
    o64, g64 = _oracle(tail, c, x, torch.float64, gate)
    o32, g32 = _oracle(tail, c, x, torch.float32, gate)
    return o64, g64, o32.double(), [g.double() for g in g32]


# ---------------------------------------------------------------------------------------------------------------------
# device placement and the kernel call
# ---------------------------------------------------------------------------------------------------------------------
_place = functools.partial(kit.place_rows, pad=PAD)      # (buffer, 5-D view) of a CPU tensor [n, C, D, H, W], or of NaNs


GRAD_OF = {"dct": ("s", "r")}


def _launch(tail, c, x, layout, wmode, with_grad=True):
    """One call through mis_hip.ops with NaN-filled out / dlogits / workspace; returns (out, [(buffer, view)])."""
    ops = _ops()
    views = {k: (None if t is None else _place(t, layout)[1]) for k, t in x["ops"].items()}
    label = x["label"].cuda()
    L = c["L"]
    out = torch.full((16,), NAN, device="cuda")
    grads = [_place(None, layout, like=x["ops"][k]) for k in GRAD_OF.get(tail, ("s",))] if with_grad else []
    d = [g[1] for g in grads] or [None, None]
    ops.scratch(1, "tail").view(torch.float32).fill_(NAN)
    wkw = dict(cons_weight=W) if wmode == "float" else dict(state=_state(c, wmode == "state1"))
    if tail == "mt":
        ops.loss_tail(views["s"], views["t"], label if L else None, L, out, d[0], loss_scale=c["scale"], **wkw)
    elif tail in ("cross", "cross_ce"):
        ops.cross_teaching_tail(views["s"], views["o"], label, L, out, d[0], pseudo_ce=tail == "cross_ce", **wkw)
    elif tail == "cross_mt":
        ops.cross_teaching_tail(views["s"], views["o"], label, L, out, d[0], teacher=views["t"], mt_weight=W_MT, **wkw)
    elif tail == "uamt":
        ops.uamt_tail(views["s"], views["t"], views["pm"], label, L, out, MAX_IT, d[0], iter_num=c["it"],
                      loss_scale=c["scale"], **wkw)
    elif tail == "ict":
        ops.ict_tail(views["s"], views["t0"], views["t1"], x["lam"].cuda(), label, L, out, d[0], loss_scale=c["scale"],
                     **wkw)
    else:
        ops.dct_tail(views["s"], views["r"], label, L, out, dA=d[0], dR=d[1], k=x["k"], loss_scale=c["scale"], **wkw)
    torch.cuda.synchronize()
    return out, grads


# ---------------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------------
def _check(tail, c):
    x = _inputs(tail, c)
    C, L, B = c["C"], c["L"], c["B"]
    n_out = N_OUT[tail](C)
    gate = 0.0 if (c["wmode"] == "state0" and tail in GATED) else 1.0
    o64, g64, o32, g32 = _references(tail, c, x, gate)
    assert o64.numel() == n_out

    out, grads = _launch(tail, c, x, c["layout"], c["wmode"])
    # every element written once and nothing else: results finite, padding / tail of out still NaN
    assert torch.isfinite(out[:n_out]).all() and torch.isnan(out[n_out:]).all(), out
    for buf, view in grads:
        assert torch.isfinite(view).all() and kit.untouched_outside(buf, view)
    # bit-reproducible
    out2, grads2 = _launch(tail, c, x, c["layout"], c["wmode"])
    assert kit.same_bits(out, out2) and all(kit.same_bits(a[0], b[0]) for a, b in zip(grads, grads2))
    # forward only: the same scalars
    out3, _ = _launch(tail, c, x, c["layout"], c["wmode"], with_grad=False)
    assert kit.same_bits(out, out3)
    # only addresses differ between a strided / offset view and the dense tensor
    if c["layout"] != "dense":
        outd, gradsd = _launch(tail, c, x, "dense", c["wmode"])
        assert kit.same_bits(out, outd) and all(torch.equal(a[1], b[1]) for a, b in zip(grads, gradsd))
    # the weight from the device state == the weight from the float argument
    if c["wmode"] != "float" and gate == 1.0:
        outf, gradsf = _launch(tail, c, x, c["layout"], "float")
        assert kit.same_bits(out, outf) and all(kit.same_bits(a[0], b[0]) for a, b in zip(grads, gradsf))
    o = out.cpu()
    assert kit.same_bits(o[4], torch.tensor(W, dtype=torch.float32))
    if gate == 0.0:
        assert o[3].item() == 0.0
        for (buf, view), rows in zip(grads, (slice(L, None), slice(None))):       # dct: dA[L:] and all of dR
            assert (view[rows] == 0).all()
        if L:
            assert grads[0][1][:L].abs().max().item() > 0

    exact = {4: float(torch.tensor(W, dtype=torch.float32))}
    if tail == "dct":
        exact[5] = float(x["k"])
    if tail == "cross_mt":
        exact[6] = float(torch.tensor(W_MT, dtype=torch.float32))
    if tail == "uamt":
        exact[5 + C] = o64[5 + C].item()                                             # the mask count, exactly
        exact[6 + C] = float(torch.tensor(o64[6 + C].item(), dtype=torch.float32))  # thr rounded to fp32
        total = (B - L) * x["ops"]["s"][0, 0].numel()
        if c["content"] == "allout":
            assert o64[5 + C].item() == 0 and o64[3].item() == 0.0
        elif c["content"] != "sat":
            assert 0 < o64[5 + C].item() <= total
    cid = _cid(c)
    gate = kit.Gate(K, FLOOR, stats=STATS)
    for i in range(n_out):
        hip, ref = o[i].double().item(), o64[i].item()
        if i in exact:
            assert hip == exact[i], (i, hip, exact[i])
            continue
        if ref == 0.0:
            assert hip == 0.0, (i, hip)
            continue
        e32, ehip = abs(o32[i].item() - ref) / abs(ref), abs(hip - ref) / abs(ref)
        gate.judge(cid, f"out[{i}]", "scalar", "max", e32, ehip, row=(tail, cid, "scalar", e32, ehip), extra=(hip, ref))
        print(f"[{tail} {cid}] out[{i}] f64 {ref:.9e} hip {hip:.9e} e32 {e32:.2e} hip {ehip:.2e}")
    for (buf, view), ref, r32 in zip(grads, g64, g32):
        got = view.cpu().double()
        if ref.abs().max().item() == 0.0:
            assert (got == 0).all()
            continue
        e32, ehip = kit.rel(r32, ref), kit.rel(got, ref)
        gate.judge(cid, "grad", "tensor", "max", e32, ehip, row=(tail, cid, "tensor", e32, ehip), extra=(tuple(ref.shape),))
        print(f"[{tail} {cid}] grad |f64|max {ref.abs().max().item():.3e} e32 {e32:.2e} hip {ehip:.2e}")
    gate.done(cid)
    return x, out, grads, o64, g64


@pytest.mark.parametrize("c", _matrix("mt"))
def test_mean_teacher_tail(c):
    _check("mt", c)


@pytest.mark.parametrize("c", _matrix("cross"))
def test_cross_teaching_tail(c):
    x, out, grads, o64, g64 = _check("cross", c)
    if c["wmode"] == "state0":                  # the cross tails take the weight only: the gate changes nothing
        out1, grads1 = _launch("cross", c, x, c["layout"], "state1")
        assert kit.same_bits(out, out1) and kit.same_bits(grads[0][0], grads1[0][0])


@pytest.mark.parametrize("c", _matrix("cross_ce"))
def test_cross_pseudo_supervision_tail(c):
    x, out, grads, o64, g64 = _check("cross_ce", c)
    L = c["L"]
    if c["B"] > L and c["content"] != "sat":
        # d/dlogit of w * CE is w/N * (p - onehot(y)): the one negative channel of an unlabeled voxel IS the pseudo
        # label the kernel chose -- on the planted ties too, where only "first maximum wins" matches
        # (read where the own softmax is not saturated to an exact fp32 1.0 / 0.0, which carries no sign)
        want = lto.argmax_first(x["ops"]["o"][L:], 1)
        got = grads[0][1][L:].cpu()
        live = torch.softmax(x["ops"]["s"][L:].double(), 1).max(1).values < 1 - 1e-4
        assert live.float().mean().item() > 0.9
        assert ((got < 0).sum(1) == 1)[live].all()
        assert torch.equal(torch.argmin(got, 1)[live], want[live])
        assert torch.equal(want, torch.argmax(x["ops"]["o"][L:], 1))


@pytest.mark.parametrize("c", _matrix("cross_mt"))
def test_cnn_meets_vit_tail(c):
    x, out, grads, o64, g64 = _check("cross_mt", c)
    # mt_weight never reaches a labeled row: those rows equal the rows of the call without a teacher, bit for bit
    _, plain = _launch("cross", c, dict(x, ops={k: v for k, v in x["ops"].items() if k != "t"}), c["layout"], c["wmode"])
    L = c["L"]
    assert torch.equal(grads[0][1][:L], plain[0][1][:L])
    assert not torch.equal(grads[0][1][L:], plain[0][1][L:])


@pytest.mark.parametrize("c", _matrix("uamt"))
def test_uamt_tail(c):
    x, out, grads, o64, g64 = _check("uamt", c)
    L, C = c["L"], c["C"]
    keep = (lto.uamt_entropy(x["ops"]["pm"]) < lto.uamt_threshold(c["it"], MAX_IT)).unsqueeze(1)
    got = grads[0][1][L:].cpu()
    # the mask of pass 2 is the mask of pass 1: no gradient on a masked-out voxel
    assert (got[~keep.expand_as(got)] == 0).all()
    if c["content"] == "allout":
        assert out[3].item() == 0.0 and (got == 0).all()
    if c["wmode"] == "state0":                  # UA-MT takes weight and iteration from the state, not the gate
        out1, grads1 = _launch("uamt", c, x, c["layout"], "state1")
        assert kit.same_bits(out, out1) and kit.same_bits(grads[0][0], grads1[0][0])


@pytest.mark.parametrize("c", _matrix("ict"))
def test_ict_tail(c):
    _check("ict", c)


@pytest.mark.parametrize("c", _matrix("dct"))
def test_dct_tail(c):
    _check("dct", c)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: nothing is launched
# ---------------------------------------------------------------------------------------------------------------------
def _dense5(n, C, sp, fill=None):
    t = torch.randn((n, C) + sp, device="cuda") if fill is None else torch.full((n, C) + sp, fill, device="cuda")
    return t


def _misaligned(n, C, sp, fill=0.5):
    row = C * sp[0] * sp[1] * sp[2]
    base = torch.full((n * row + 4,), fill, device="cuda")
    v = base[1:1 + n * row].view((n, C) + sp)
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("tail", ["mt", "uamt", "ict", "dct", "sma"])
@pytest.mark.parametrize("how", ["S%4", "misaligned"])
def test_vectorised_tails_refuse_what_float4_cannot_address(tail, how):
    ops = _ops()
    C, B, L = 3, 4, 2
    sp = (1, 7, 9) if how == "S%4" else (1, 8, 12)
    mk = (lambda n: _dense5(n, C, sp)) if how == "S%4" else (lambda n: _misaligned(n, C, sp))
    label = torch.zeros((L,) + sp, dtype=torch.uint8, device="cuda")
    out = torch.full((16,), NAN, device="cuda")
    d = _dense5(B, C, sp, NAN)
    dr = _dense5(B - L, C, sp, NAN)
    acc = _dense5(B - L, C, sp, NAN)
    with pytest.raises(RuntimeError, match="MIS_ERR_UNSUPPORTED"):
        if tail == "mt":
            ops.loss_tail(mk(B), mk(B - L), label, L, out, d, cons_weight=W)
        elif tail == "uamt":
            ops.uamt_tail(mk(B), mk(B - L), mk(B - L), label, L, out, MAX_IT, d, cons_weight=W)
        elif tail == "ict":
            ops.ict_tail(mk(B), mk(B - L), mk(B - L), torch.rand(B - L, device="cuda"), label, L, out, d, cons_weight=W)
        elif tail == "dct":
            ops.dct_tail(mk(B), mk(B - L), label, L, out, dA=d, dR=dr, k=0, cons_weight=W)
        else:
            ops.softmax_mean_accumulate(mk(B), acc, 2, 0.125, True)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(d).all() and torch.isnan(dr).all() and torch.isnan(acc).all()


def test_uamt_tail_needs_unlabeled_rows():
    ops = _ops()
    C, B, sp = 3, 3, (1, 8, 12)
    empty = torch.empty((0, C) + sp, device="cuda")
    out = torch.full((16,), NAN, device="cuda")
    d = _dense5(B, C, sp, NAN)
    with pytest.raises(RuntimeError, match="MIS_ERR_ARG"):
        ops.uamt_tail(_dense5(B, C, sp), empty, empty, torch.zeros((B,) + sp, dtype=torch.uint8, device="cuda"), B, out,
                      MAX_IT, d, cons_weight=W)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(d).all()


# ---------------------------------------------------------------------------------------------------------------------
# arg-max of the channels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("shape", ["2d", "odd", "part"])
def test_argmax_channels_first_maximum_wins(C, shape):
    ops = _ops()
    sp = SHAPES[shape]
    g = torch.Generator().manual_seed(C * 7 + len(shape))
    x = _plant_ties(torch.randn((5, C) + sp, generator=g) * 3.0, C)
    want = torch.argmax(x, 1)
    assert torch.equal(want, lto.argmax_first(x, 1))
    assert (want.reshape(5, -1)[:, 0::4] == 0).all() and (want.reshape(5, -1)[:, 2::4] == 0).all()
    for layout in ("dense", "strided", "offset"):
        buf, view = _place(x, layout)
        out = torch.full((5,) + sp, 255, dtype=torch.uint8, device="cuda")
        ops.argmax_channels(view, out)
        assert torch.equal(out.cpu().long(), want), layout
        assert buf.isnan().sum().item() == buf.numel() - x.numel()


def test_argmax_channels_refuses_five_classes():
    ops = _ops()
    out = torch.full((2, 1, 8, 8), 255, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="MIS_ERR_UNSUPPORTED"):
        ops.argmax_channels(torch.randn((2, 5, 1, 8, 8), device="cuda"), out)
    torch.cuda.synchronize()
    assert (out == 255).all()


# ---------------------------------------------------------------------------------------------------------------------
# the MC-dropout mean prediction, alone and chained into the UA-MT tail
# ---------------------------------------------------------------------------------------------------------------------
def _accumulate(C, U, R, sp, layout, g, passes=4, scale=0.125):
    """Four calls (first, then three accumulations) as the UA-MT step issues them; returns the device buffer / view of
    acc and the float64 / fp32 references."""
    ops = _ops()
    abuf, aview = _place(None, layout, like=torch.empty((U, C) + sp))
    a64 = a32 = None
    base = torch.randn((U, C) + sp, generator=g) * 3.0      # correlated passes: one prediction under dropout-like noise
    for i in range(passes):
        z = base.repeat((R,) + (1,) * (base.dim() - 1)) + torch.randn((R * U, C) + sp, generator=g) * 1.5
        zbuf, zview = _place(z, layout)
        ops.softmax_mean_accumulate(zview, aview, R, scale, i == 0)
        a64 = lto.softmax_mean_accumulate(z, a64, R, scale, i == 0)
        a32 = lto.softmax_mean_accumulate(z, a32, R, scale, i == 0, dtype=torch.float32)
    torch.cuda.synchronize()
    return abuf, aview, a64, a32.double()


@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("U", [1, 3])
@pytest.mark.parametrize("R", [1, 2, 8])
def test_softmax_mean_accumulate(C, U, R):
    sp = SHAPES["part"] if U == 1 else SHAPES["3d"]
    results = {}
    for layout in ("dense", "strided", "offset"):
        g = torch.Generator().manual_seed(C * 100 + U * 10 + R)
        abuf, aview, a64, a32 = _accumulate(C, U, R, sp, layout, g)
        assert torch.isfinite(aview).all()
        rest = abuf.clone()
        kit.logical(rest, aview).fill_(NAN)
        assert torch.isnan(rest).all()                      # the first call overwrites NaNs; the padding is untouched
        results[layout] = aview.cpu()
        e32, ehip = kit.rel(a32, a64), kit.rel(results[layout].double(), a64)
        STATS.append(("sma", f"C{C}-U{U}-R{R}-{layout}", "tensor", e32, ehip))
        print(f"[sma C{C} U{U} R{R} {layout}] e32 {e32:.2e} hip {ehip:.2e}")
        assert ehip <= max(K * e32, FLOOR["tensor"]), (layout, e32, ehip)
    assert torch.equal(results["dense"], results["strided"]) and torch.equal(results["dense"], results["offset"])


@pytest.mark.parametrize("C,it", [(2, 500), (3, MAX_IT), (4, 0)])
def test_mean_prediction_chained_into_uamt_tail(C, it):
    """softmax_mean_accumulate -> uamt_tail as UAMTTrainer chains them: T = 4 x 2 MC passes folded into one buffer, which is
    the tail's mean_probs operand in place (a batch-strided view)."""
    ops = _ops()
    U, R, L, sp = 2, 2, 2, SHAPES["3d"]
    thr = lto.uamt_threshold(it, MAX_IT)
    g = torch.Generator().manual_seed(C * 31 + it)
    abuf, aview, a64, _ = _accumulate(C, U, R, sp, "strided", g)
    pm = aview.cpu()
    # the kernel's own fp32 mean, exact values: voxels it leaves within fp32 rounding of the threshold are made clearly
    # decided (near-one-hot) IN the buffer -- none is excluded from the comparison -- and the set is empty before the tail runs
    und = lto.uamt_undecided(pm, thr).unsqueeze(1).expand_as(pm)
    hot = torch.full_like(pm, 1e-3)
    hot[:, 0] = 1.0 - (C - 1) * 1e-3
    pm = torch.where(und, hot, pm)
    assert int(und.sum()) <= 0.01 * und.numel()
    aview.copy_(pm.cuda())
    assert not lto.uamt_undecided(aview.cpu(), thr).any()
    keep = lto.uamt_entropy(pm) < thr
    assert 0 < int(keep.sum()) < keep.numel()
    s = torch.randn((L + U, C) + sp, generator=g) * 3.0
    t = torch.randn((U, C) + sp, generator=g) * 3.0
    label = torch.randint(0, C, (L,) + sp, generator=g).to(torch.uint8)
    out = torch.full((16,), NAN, device="cuda")
    dbuf, dview = _place(None, "strided", like=s)
    ops.uamt_tail(s.cuda(), t.cuda(), aview, label.cuda(), L, out, MAX_IT, dview, cons_weight=W, iter_num=it)
    w32 = float(torch.tensor(W, dtype=torch.float32))
    o64, g64 = lto.uamt_tail(s, t, pm, label, L, w32, it, MAX_IT)
    o32, g32 = lto.uamt_tail(s, t, pm, label, L, w32, it, MAX_IT, dtype=torch.float32)
    o = out.cpu().double()
    assert o[5 + C].item() == float(keep.sum()) == o64[5 + C].item()
    for i in (0, 1, 2, 3):
        e32, ehip = abs(o32[i].item() - o64[i].item()) / abs(o64[i].item()), abs(o[i].item() - o64[i].item()) / abs(o64[i].item())
        assert ehip <= max(K * e32, FLOOR["scalar"]), (i, e32, ehip)
    e32, ehip = kit.rel(g32.double(), g64), kit.rel(dview.cpu().double(), g64)
    assert ehip <= max(K * e32, FLOOR["tensor"]), (e32, ehip)
    assert (dview[L:].cpu()[~keep.unsqueeze(1).expand(-1, C, -1, -1, -1)] == 0).all()
