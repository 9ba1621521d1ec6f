"""mis_patch_nce (through ops.patch_nce), utils.losses.ConLoss / contrastive_loss_sup and the launch tape against the float64
oracle of tests/patch_nce_oracle.py.

The matrix (d in {16, 32} x B in {1, 3} throughout the geometry sweep):
  N        1, 2 (no / one negative); 15, 16, 17 (one MFMA tile and its two boundaries); 63 = 7 x 9 and 100 = 10 x 10 (no
           multiple of 16; 63 one short of a 64-key step, 100 a partly masked second step); 784 = 28^2; 1040 = 65 tiles of
           16 (one past a 64-wide key step); 3136 = 56^2 (many workgroups per sample).
  content  signed normal; ReLU'd (sparse, non-negative); one all-zero q vector; one all-zero k vector; a whole sample of
           zeros; signed one-hot (s at +-1/T or 0); feat_q == feat_k; inputs scaled by 1e3 and by 1e-3 -- each at
           T in {0.07, 0.01, 1.0} (at T = 0.01 the one-hot rows hold exp(100) ratios: no fixed shift survives), at N = 100
           and 63, and the one-hot / zero-vector ones again at N = 1040 where the running maximum moves between key steps.
  layout   dense; batch-strided views of a larger buffer; a base pointer offset by one float; dfeat_q with its own batch
           stride -- every view inside NaN guards that must stay untouched.
  plus     grad_scale = 0.37, loss-only == loss-with-gradient (bits), two calls == (bits), the modules, the tape.

Tolerance (the float64 arbiter of tests/test_loss_tails_gpu.py, K = 6), per scalar of ``out`` and per gradient tensor:

    |hip - f64|_max <= max(K * e32, FLOOR) * |f64|_max

e32 = relative error of the fp32 CPU evaluation of the oracle's materialised form (the two means of the row form) against
the float64 evaluation, same case and quantity; FLOOR = the largest e32 over this file's matrix, measured on the CPU
before any GPU run.  One floor for the gradient tensors, FLOOR_TENSOR = 1.2e-6 (largest e32 1.15e-6, d32-B3-N63-same-T0.01).
The three scalars do not share one: pooled, the floor would be the 1.83e-4 of mean_i s_ii (d16-B1-N17-signed: a mean of
17 signed scores that cancels to 2e-4 of their size) and would let the loss drift by as much.  Each scalar is held to the
largest e32 of its own kind, none above the pooled figure: loss 2.0e-7 (1.92e-7, d32-B3-N63-same-T0.01), mean_i logsumexp
3.0e-7 (2.999e-7, d16-B3-N1-signed), mean_i s_ii 1.9e-4.

A float64 value of exactly 0 must be met exactly: a scalar (the loss at N = 1), a gradient tensor, and every pixel whose
float64 gradient is 0 in all d channels (N = 1; the rows of a sample of zeros inside a batch that is not) -- the zeros
the formula gives.  A single element that float64 brings to 0 is not held to it: in the one-hot cases hundreds of
elements are +-1 entries times equal probabilities that happen to cancel in a sum over the keys, and the fp32 evaluation
of the oracle itself leaves 14 .. 664 of them non-zero per case (it is exactly 0 on every all-channel row).

Measured on an MI355X (this file's own run; `MIS_PATCH_NCE_STATS=<file>` writes every figure as JSON):

    quantity   e32 (fp32 torch vs float64)   HIP vs float64 (max)   worst HIP / e32
    loss       0        .. 1.92e-7           1.02e-7                13.1  (e32 = 4.9e-9 there, HIP 6.4e-8; floor)
    mean s_ii  0        .. 1.83e-4           2.44e-4                416   (e32 = 1.5e-10 there, HIP 6.2e-8; floor)
    mean lse   3.1e-10  .. 3.00e-7           3.00e-7                8.9   (e32 = 1.2e-8 there, HIP 1.06e-7; floor)
    gradient   0        .. 1.15e-6           2.58e-6                3.12  (d16-B3-N100-same-T0.01: e32 8.3e-7)

    The loss never leaves 1.1e-7.  The scalar ratios above 6 are cases where the fp32 evaluation happens to round to the
    float64 value, which the floors are for; the 2.44e-4 of mean s_ii is the cancelling mean at N = 17 (e32 1.83e-4 there:
    1.3 x).  The gradient's worst cases are two at T = 0.01, where the scores reach 100 and an fp32 ulp of a score is 8e-6
    (3.1 x and 3.0 x the fp32 torch evaluation), and the one-hot rows at T = 1 (2.75 x); every other tensor is within 2.1 x.
    147 tests, 546 compared quantities, 7 s wall.
"""
import functools
import zlib

import pytest
import torch

import oracle_kit as kit
import patch_nce_oracle as pno

pytestmark = pytest.mark.gpu

K = 6.0
FLOOR = {"loss": 2.0e-7, "mean_sii": 1.9e-4, "mean_lse": 3.0e-7,      # largest e32 of each scalar over the matrix
         "grad": 1.2e-6}                                              # largest tensor e32: 1.15e-6

NS = (1, 2, 15, 16, 17, 63, 100, 784, 1040, 3136)
CONTENTS = ("signed", "relu", "zero_q", "zero_k", "zero_sample", "onehot", "same", "x1e3", "x1e-3")
TS = (0.07, 0.01, 1.0)
LAYOUTS = ("dense", "strided", "offset", "dstride")
STATS = []


def _ops():
    from mis_hip import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if not STATS:
        return
    for kind in ("scalar", "tensor"):
        rows = [s for s in STATS if s[1] == kind]
        e32s = [s[2] for s in rows]
        worst = max(rows, key=lambda s: s[3] / s[2] if s[2] > 0 else 0.0)
        print(f"\n[patch_nce] {kind:6s} e32 {min(e32s):.2e} .. {max(e32s):.2e}  hip max {max(s[3] for s in rows):.2e}  "
              f"worst hip/e32 {worst[3] / worst[2] if worst[2] > 0 else 0.0:.2f} ({worst[0]}: e32 {worst[2]:.2e})", end="")
    print()
    kit.report(STATS, "MIS_PATCH_NCE_STATS")


# ---------------------------------------------------------------------------------------------------------------------
# the case matrix
# ---------------------------------------------------------------------------------------------------------------------
def _case(**kw):
    c = dict(d=16, B=3, N=100, content="signed", T=0.07, layout="dense", gs=1.0)
    c.update(kw)
    return c


def _cid(c):
    return f"d{c['d']}-B{c['B']}-N{c['N']}-{c['content']}-T{c['T']}-{c['layout']}-gs{c['gs']}"


def _matrix():
    cs = [_case(d=d, B=B, N=N) for d in (16, 32) for B in (1, 3) for N in NS]
    for d, N in ((16, 100), (32, 63)):
        cs += [_case(d=d, N=N, content=ct, T=T) for ct in CONTENTS for T in TS if not (ct == "signed" and T == 0.07)]
    cs += [_case(d=d, B=B, N=1040, content=ct, T=T) for d, B in ((16, 1), (32, 3)) for ct in ("onehot", "zero_q", "zero_k")
           for T in (0.07, 0.01)]
    cs += [_case(d=d, B=B, N=N, layout=lay) for d, B in ((16, 3), (32, 3), (32, 1)) for N in (17, 100, 1040)
           for lay in LAYOUTS[1:]]
    cs += [_case(gs=0.37), _case(d=32, N=784, gs=0.37, content="relu", layout="dstride")]
    seen, out = set(), []
    for c in cs:
        if _cid(c) not in seen:
            seen.add(_cid(c))
            out.append(c)
    return out


def _inputs(c):
    """(feat_q, feat_k) [B, d, N] fp32 on the CPU, from a seed of the case's geometry and content."""
    d, B, N, ct = c["d"], c["B"], c["N"], c["content"]
    g = torch.Generator().manual_seed(zlib.crc32(f"{d}-{B}-{N}-{ct}".encode()))
    fq, fk = torch.randn(B, d, N, generator=g), torch.randn(B, d, N, generator=g)
    if ct in ("relu", "zero_q", "zero_k", "zero_sample"):
        fq, fk = torch.relu(fq), torch.relu(fk)
    if ct == "zero_q":
        fq[B - 1, :, N // 2] = 0
    elif ct == "zero_k":
        fk[0, :, N // 3] = 0
    elif ct == "zero_sample":
        fq[B - 1], fk[B - 1] = 0, 0
    elif ct == "onehot":
        def hot(x):
            ch = torch.randint(0, d, (B, 1, N), generator=g)
            return torch.zeros_like(x).scatter_(1, ch, x.gather(1, ch))      # one signed entry per pixel
        fq, fk = hot(fq), hot(fk)
    elif ct == "same":
        fk = fq.clone()
    elif ct == "x1e3":
        fq, fk = fq * 1e3, fk * 1e3
    elif ct == "x1e-3":
        fq, fk = fq * 1e-3, fk * 1e-3
    return fq, fk


def _rel(a, b):
    """|a - b|_max / |b|_max (0 when b is all zero and a equals it)."""
    scale = b.abs().max().item()
    err = (a.double() - b).abs().max().item()
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


@functools.lru_cache(maxsize=None)
def _reference(d, B, N, content, T, gs):
    """Computed once per (geometry, content, T, grad_scale) and shared by every test and layout that needs it:
    (feat_q, feat_k, out64 [3], grad64, e32 of the three scalars, e32 of the gradient)."""
    fq, fk = _inputs(dict(d=d, B=B, N=N, content=content))
    out64, g64 = pno.loss_and_grad(fq, fk, T, torch.float64, gs)
    out32, g32 = pno.loss_and_grad(fq, fk, T, torch.float32, gs)
    e32s = [_rel(out32[i], out64[i]) for i in range(3)]
    return fq, fk, out64, g64, e32s, _rel(g32, g64)


def _ref(c):
    return _reference(c["d"], c["B"], c["N"], c["content"], c["T"], c["gs"])


def _check(cid, out, grad, ref, scalars=("loss", "mean_sii", "mean_lse")):
    """The arbiter, on host copies of the kernel's results; ``out`` holds the named scalars in the kernel's order."""
    _, _, out64, g64, e32s, e32g = ref
    out, grad = out.cpu(), grad.cpu()
    gate = kit.Gate(K, FLOOR, stats=STATS)
    for i, name in enumerate(scalars):
        want, got = out64[i].item(), float(out[i])
        err = abs(got - want) / abs(want) if want != 0 else (0.0 if got == 0 else float("inf"))
        gate.judge(cid, name, name, "max", e32s[i], err, row=(cid + ":" + name, "scalar", e32s[i], err))
        print(f"{cid} {name}: f64 {want:.9g} hip {got:.9g} err {err:.3e} e32 {e32s[i]:.3e}")
    errg = _rel(grad, g64)
    gate.judge(cid, "grad", "grad", "max", e32g, errg, row=(cid + ":grad", "tensor", e32g, errg))
    print(f"{cid} grad: |f64|max {g64.abs().max().item():.6g} err {errg:.3e} e32 {e32g:.3e}")
    rows0 = (g64 == 0).all(dim=1, keepdim=True).expand_as(g64)      # pixels the formula gives no gradient at all
    nz = int(torch.count_nonzero(grad[rows0]))
    assert not nz, (cid, "gradient elements of pixels that must be exactly 0", nz)
    gate.done(cid)


POISON = float("nan")


def _place(x, layout, pad):
    """A device copy of x [B, d, N] as a view with the layout, inside a NaN-filled buffer: (view, buffer)."""
    B, d, N = x.shape
    if layout == "dense":
        buf = torch.full((B * d * N + 2 * pad,), POISON, device="cuda")
        view = buf[pad:pad + B * d * N].view(B, d, N)
    elif layout == "offset":                       # base pointer one float past the allocation's alignment
        buf = torch.full((1 + B * d * N + pad,), POISON, device="cuda")
        view = buf[1:1 + B * d * N].view(B, d, N)
    else:                                          # batch stride d * N + pad: odd, so the planes lose every alignment
        buf = torch.full((B, d * N + pad), POISON, device="cuda")
        view = buf[:, :d * N].view(B, d, N)
    view.copy_(x)
    return view, buf


def _run(c, with_grad=True):
    """One ops.patch_nce call of the case: (out [5] with two poison cells behind the three scalars, dfeat view or None, the
    buffers whose guard cells must still be NaN, with the views inside them)."""
    fq, fk = _ref(c)[:2]
    lay = c["layout"]
    in_lay = lay if lay in ("strided", "offset") else "dense"
    q, qbuf = _place(fq, in_lay, 7)
    k, kbuf = _place(fk, in_lay, 5)
    dq = dbuf = None
    if with_grad:
        dq, dbuf = _place(torch.full_like(fq, POISON), "strided" if lay in ("strided", "dstride") else in_lay, 3)
    out = torch.full((5,), POISON, device="cuda")
    _ops().patch_nce(q, k, out, dfeat=dq, temperature=c["T"], grad_scale=c["gs"])
    torch.cuda.synchronize()
    return out, dq, ((qbuf, q, fq), (kbuf, k, fk), (dbuf, dq, None))


def _assert_guards(cid, out, bufs):
    """Inputs unchanged, every cell outside the views still NaN, every cell of out[:3] and dfeat_q written."""
    assert torch.isnan(out[3:]).all() and torch.isfinite(out[:3]).all(), (cid, out)
    for buf, view, src in bufs:
        if buf is None:
            continue
        if src is not None:
            assert torch.equal(view.cpu(), src), cid
        else:
            assert torch.isfinite(view).all(), (cid, "dfeat_q has cells the kernel did not write")
        inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
        span = torch.arange(view[0].numel(), device="cuda")
        first = (view.data_ptr() - buf.data_ptr()) // 4
        for b in range(view.shape[0]):
            inside[first + b * (view.stride(0) if view.shape[0] > 1 else 0) + span] = True
        assert torch.isnan(buf.reshape(-1)[~inside]).all(), (cid, "a write outside B x d x N")
        assert int((~inside).sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI through ops.patch_nce
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _matrix(), ids=_cid)
def test_patch_nce_matches_the_float64_oracle(c):
    out, dq, bufs = _run(c)
    _assert_guards(_cid(c), out, bufs)
    _check(_cid(c), out[:3], dq, _ref(c))


@pytest.mark.parametrize("c", [_case(d=16, B=1, N=1), _case(d=32, B=3, N=1)], ids=_cid)
def test_a_single_pixel_gives_exactly_zero(c):
    out, dq, _ = _run(c)
    assert out[0].item() == 0.0 and torch.count_nonzero(dq) == 0
    assert out[1].item() == out[2].item()


@pytest.mark.parametrize("c", [_case(d=16, B=3, N=17), _case(d=32, B=3, N=100, content="onehot", T=0.01),
                               _case(d=16, B=1, N=1040, content="relu"), _case(d=32, B=3, N=3136, layout="strided")],
                         ids=_cid)
def test_loss_only_call_and_repeated_calls_are_bit_identical(c):
    out, dq, _ = _run(c)
    lo, none, bufs = _run(c, with_grad=False)
    assert none is None
    _assert_guards(_cid(c), lo, bufs)
    assert torch.equal(out[:3], lo[:3]), (out, lo)
    out2, dq2, _ = _run(c)
    assert torch.equal(out[:3], out2[:3]) and torch.equal(dq, dq2)


def test_refusals():
    ops = _ops()
    out = torch.zeros(3, device="cuda")
    q = torch.randn(2, 24, 10, device="cuda")
    with pytest.raises(RuntimeError, match="supported dims"):
        ops.patch_nce(q, q.clone(), out)
    q = torch.randn(2, 16, 10, device="cuda")
    with pytest.raises(AssertionError):
        ops.patch_nce(q, torch.randn(2, 16, 11, device="cuda"), out)
    with pytest.raises(RuntimeError, match="dense"):
        ops.patch_nce(torch.randn(2, 10, 16, device="cuda").permute(0, 2, 1), q, out)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.patch_nce(q.double(), q.double(), out)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.patch_nce(q.cpu(), q.cpu(), out)


# ---------------------------------------------------------------------------------------------------------------------
# the modules
# ---------------------------------------------------------------------------------------------------------------------
def _module_case(d, B, H, W):
    c = _case(d=d, B=B, N=H * W, gs=0.5)
    return c, _ref(c)


@pytest.mark.parametrize("cls", ["ConLoss", "contrastive_loss_sup"])
@pytest.mark.parametrize("d,B,H,W", [(16, 3, 10, 10), (32, 1, 7, 9)])
def test_modules_forward_and_backward(cls, d, B, H, W):
    from utils import losses
    c, ref = _module_case(d, B, H, W)
    fq = ref[0].view(B, d, H, W).cuda().requires_grad_(True)
    fk = ref[1].view(B, d, H, W).cuda().requires_grad_(True)
    loss = getattr(losses, cls)()(fq, fk)
    assert loss.dim() == 0
    (0.5 * loss).backward()
    torch.cuda.synchronize()
    assert fk.grad is None
    _check(f"{cls}-{_cid(c)}", loss.detach().reshape(1), fq.grad.reshape(B, d, H * W), ref, scalars=("loss",))


def test_modules_take_a_non_contiguous_feat_q_and_another_temperature():
    from utils import losses
    d, B, H, W = 16, 3, 10, 10
    c = _case(d=d, B=B, N=H * W, T=1.0, gs=0.5)
    ref = _ref(c)
    base = ref[0].view(B, d, H, W).permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)      # channels last
    fq = base.permute(0, 3, 1, 2)
    assert not fq.is_contiguous()
    loss = losses.ConLoss(temperature=1.0)(fq, ref[1].view(B, d, H, W).cuda())
    (0.5 * loss).backward()
    torch.cuda.synchronize()
    _check("ConLoss-noncontig-" + _cid(c), loss.detach().reshape(1), base.grad.permute(0, 3, 1, 2).reshape(B, d, H * W), ref,
           scalars=("loss",))
    with torch.no_grad():                                  # no gradient asked for: the loss-only call, same bits
        assert torch.equal(losses.ConLoss(temperature=1.0)(fq.detach(), ref[1].view(B, d, H, W).cuda()), loss.detach())


def test_modules_refuse_what_the_kernel_is_not_built_for():
    from utils import losses
    crit = losses.ConLoss()
    with pytest.raises(RuntimeError, match=r"supported dims"):
        crit(torch.randn(2, 24, 4, 4, device="cuda"), torch.randn(2, 24, 4, 4, device="cuda"))
    with pytest.raises(RuntimeError, match=r"supported dims"):
        crit(torch.randn(2, 16, 4, 4, device="cuda").double(), torch.randn(2, 16, 4, 4, device="cuda").double())
    with pytest.raises(AssertionError):
        crit(torch.randn(2, 16, 4, 4, device="cuda"), torch.randn(2, 16, 4, 5, device="cuda"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(torch.randn(2, 16, 4, 4), torch.randn(2, 16, 4, 4))


# ---------------------------------------------------------------------------------------------------------------------
# the launch tape
# ---------------------------------------------------------------------------------------------------------------------
def test_a_taped_call_replays_bit_identically_on_new_contents():
    from mis_hip import lib
    ops = _ops()
    a, b = _case(d=32, B=3, N=1040), _case(d=32, B=3, N=1040, content="relu", gs=0.37)
    fq, fk = (t.cuda() for t in _ref(a)[:2])
    out, dq = torch.zeros(3, device="cuda"), torch.zeros_like(fq)
    tape = lib.LaunchTape()
    with tape.recording():
        ops.patch_nce(fq, fk, out, dfeat=dq, grad_scale=0.37)
    assert len(tape) == 1
    fq.copy_(_ref(b)[0])
    fk.copy_(_ref(b)[1])
    out.fill_(POISON)
    dq.fill_(POISON)
    tape.replay()
    torch.cuda.synchronize()
    out_e, dq_e = torch.zeros(3, device="cuda"), torch.zeros_like(fq)
    ops.patch_nce(fq, fk, out_e, dfeat=dq_e, grad_scale=0.37)
    torch.cuda.synchronize()
    assert torch.equal(out, out_e) and torch.equal(dq, dq_e)
    _check("tape-" + _cid(b), out, dq, _ref(b))
