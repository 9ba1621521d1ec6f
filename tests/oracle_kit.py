"""The kit of the float64-oracle GPU tests: where an operand is placed, the gate a figure passes, the report that is left.

A test of this family holds a kernel's result to a float64 reference in units of fp32 noise: e32 is the error of an fp32
evaluation of the same expression on the machine that runs the test, and the result may be off by max(K * e32, FLOOR[kind]).
What is the same in every such file lives here; the measure, K, FLOOR with their provenance and the case matrix stay with the
kernel family.  Nothing here needs a GPU at import, and every function takes ``device`` so that
tests/test_oracle_kit_cpu.py runs the same code on the CPU.
"""
import ctypes
import json
import math
import os

import pytest
import torch

NAN = float("nan")
SENT = -777.0


def nan(*shape, device="cuda"):
    return torch.full(shape, NAN, device=device)


# ---------------------------------------------------------------------------------------------------------------------
# placement
# ---------------------------------------------------------------------------------------------------------------------
def place(t, layout, lead, trail, rows_behind=0, device="cuda"):
    """Device copy of an input [N, C, ...] (channels) or [rows][cols] (columns): ``dense``, or as the ``slice``
    [:, lead:lead + C] of a wider NaN-filled buffer; ``rows_behind``: NaN rows behind the last one in the same allocation."""
    if t is None:
        return None
    if layout == "dense" and not rows_behind:
        return t.to(device, copy=True)
    if layout == "dense":
        lead = trail = 0
    N, C = t.shape[:2]
    buf = torch.full((N + rows_behind, lead + C + trail) + tuple(t.shape[2:]), NAN, device=device)
    v = buf[:N, lead:lead + C]
    v.copy_(t)
    assert v.data_ptr() == buf.data_ptr() + lead * buf.stride(1) * buf.element_size()
    return v


class Out:
    """A NaN-filled output (``v``, or ``fill``: what an accumulating call finds): dense, or the slice [:, lead:lead + C] of
    a wider sentinel-filled buffer ``buf``."""

    def __init__(self, shape, layout, lead, trail, fill=None, device="cuda"):
        shape = tuple(shape)
        self.lead = lead
        if layout == "dense":
            self.buf = None
            self.v = nan(*shape, device=device)
        else:
            self.buf = torch.full((shape[0], lead + shape[1] + trail) + shape[2:], SENT, device=device)
            self.v = self.buf[:, lead:lead + shape[1]]
            self.v.fill_(NAN)
            assert self.v.data_ptr() == self.buf.data_ptr() + lead * self.buf.stride(1) * self.buf.element_size()
        if fill is not None:
            self.v.copy_(fill)

    def untouched(self):
        """Every element of the buffer outside the view still holds the sentinel."""
        end = self.lead + self.v.shape[1]
        return self.buf is None or bool((self.buf[:, :self.lead] == SENT).all() and (self.buf[:, end:] == SENT).all())


def place_rows(t, layout, pad, like=None, device="cuda"):
    """(buffer, view) of a tensor [n, ...] (or of NaNs shaped ``like``) whose batch rows lie in a NaN-filled [n, row] buffer:
    ``dense``, ``strided`` (batch stride row + pad) or ``offset`` (strided, two rows into the buffer)."""
    if layout not in ("dense", "strided", "offset"):
        raise ValueError(f"place_rows: no layout {layout!r}")
    src = like if t is None else t
    n, row = src.shape[0], src[0].numel()
    off = 2 if layout == "offset" else 0
    width = row + (0 if layout == "dense" else pad)
    buf = torch.full((n + off, width), NAN, device=device)
    if t is not None:
        buf[off:, :row] = t.reshape(n, row)
    view = buf[off:, :row].view(src.shape)                  # a view: raises if it would have to copy
    assert view.data_ptr() == buf.data_ptr() + off * width * buf.element_size()
    return buf, view


def logical(buf, view):
    """The region of ``buf`` (or of a clone of it) that ``view`` covers."""
    n, row = view.shape[0], view[0].numel()
    return buf[buf.shape[0] - n:, :row]


def untouched_outside(buf, view):
    """Everything in ``buf`` outside ``view`` is still NaN."""
    rest = buf.clone()
    logical(rest, view).fill_(NAN)
    return bool(torch.isnan(rest).all())


# ---------------------------------------------------------------------------------------------------------------------
# the gate
# ---------------------------------------------------------------------------------------------------------------------
class Gate:
    """tol = max(K * e32, floor[kind]) * factor on every figure of one case; ``stats`` gets one row per figure.
    ``over_the_gate``: {case: {(label, measure)}}, the figures known to sit over the gate (strict: see ``done``)."""

    def __init__(self, K, floor, over_the_gate=None, stats=None):
        self.K, self.floor = K, floor
        self.over_the_gate = over_the_gate or {}
        self.stats = [] if stats is None else stats
        self.bad = []

    def finite(self, got, what):
        assert bool(torch.isfinite(got).all()), (what, "not finite")

    def zero_ok(self, flag, what):
        assert bool(flag), (what, "a reference of exactly 0 is not met exactly")

    def judge(self, case, label, kind, measure, e32, hip, factor=1.0, row=None, ok=None, extra=()):
        """One figure ``hip`` of tensor ``label`` against its tolerance, which is returned.  ``row``: what ``stats`` gets
        instead of (case, label, kind, measure, e32, hip); ``ok``: the verdict of a measure that is not one figure (it
        compared element by element against this tolerance); ``extra``: appended to the entry of a figure over the gate."""
        tol = max(self.K * e32, self.floor[kind]) * factor
        self.stats.append((case, label, kind, measure, e32, hip) if row is None else row)
        if not (hip <= tol if ok is None else ok):          # a NaN figure is over the gate
            self.bad.append((label, measure, f"e32 {e32:.3e}", f"hip {hip:.3e}", f"tol {tol:.3e}") + tuple(extra))
        return tol

    def tensor(self, case, label, kind, got, ref, measure, e32, prefix, extra=(), width=8):
        """``got`` against ``ref`` under ``measure`` (-> {"zero_ok": ..., name: figure}): finite, exact zeros, then judge()
        for every measure named in ``e32`` ({name: yardstick}); the rows are prefix + (label, kind, name, e32, hip) + extra."""
        got = got.detach().cpu().double().reshape(ref.shape)
        self.finite(got, (case, label))
        m = measure(got, ref)
        self.zero_ok(m["zero_ok"], (case, label))
        for ms, e in e32.items():
            tol = self.judge(case, label, kind, ms, e, m[ms], extra=extra, row=tuple(prefix) + (label, kind, ms, e, m[ms]) + tuple(extra))
            print(f"[{' '.join(prefix)}] {label:{width}s} {ms:3s} e32 {e:.2e} hip {m[ms]:.2e} ratio "
                  f"{m[ms] / max(e, self.floor[kind] / self.K):.2f} tol {tol:.2e}  {' '.join(extra)}")
        return m

    def done(self, case, sync=True):
        """Strict and narrow: a case named in ``over_the_gate`` xfails only when exactly the named (label, measure) entries
        are over the gate -- one more, one fewer or the named entry passing fail it; every other case has none over."""
        if sync and torch.cuda.is_available():
            torch.cuda.synchronize()
        bad, self.bad = self.bad, []
        known = self.over_the_gate.get(case)
        if known:
            assert {(b[0], b[1]) for b in bad} == known, (case, "expected over the gate", known, "found", bad)
            pytest.xfail(f"{case}: {bad}")
        assert not bad, (case, bad)


def worst_rows(figures):
    """[(key, {lo, hi: the e32 range; hip: the largest; ratio: the worst hip / unit; at: where})] of (key, at, e32, hip, unit):
    what the files' report tables print per key."""
    rows = {}
    for key, at, e32, hip, unit in figures:
        r = rows.setdefault(key, dict(lo=1e9, hi=0.0, ratio=0.0, hip=0.0, at=""))
        r["lo"], r["hi"], r["hip"] = min(r["lo"], e32), max(r["hi"], e32), max(r["hip"], hip)
        ratio = hip / unit if unit > 0 else 0.0
        if ratio > r["ratio"]:
            r["ratio"], r["at"] = ratio, at
    return sorted(rows.items())


def report(stats, env, payload=None, indent=None):
    """``payload`` (default: ``stats``) as JSON into the file the environment variable ``env`` names, if it names one."""
    path = os.environ.get(env)
    if path:
        with open(path, "w") as f:
            json.dump(stats if payload is None else payload, f, indent=indent)


# ---------------------------------------------------------------------------------------------------------------------
# odds and ends
# ---------------------------------------------------------------------------------------------------------------------
def one_thread(fn, *args, **kw):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # the summation order, and with it the last digits, would follow the thread count
    try:
        return fn(*args, **kw)
    finally:
        torch.set_num_threads(threads)


def kernel_name(query, *args, size=128):
    """What a ``*_kernel_name`` query of the library (the function, or its name) prints for these arguments: host side only."""
    if isinstance(query, str):
        from mis_hip import lib
        query = getattr(lib.load(), query)
    buf = ctypes.create_string_buffer(size)
    st = query(*args, buf, size)
    assert st == 0, (query, args, st)
    return buf.value.decode()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def rel(a, ref):
    """|a - ref|_max / |ref|_max; 0 where the reference is all zero."""
    m = ref.abs().max().item()
    return (a.double() - ref).abs().max().item() / m if m > 0 else 0.0


def ceil2(v):
    """v rounded up to two significant digits (how the FLOOR constants are written)."""
    if v <= 0:
        return 0.0
    e = math.floor(math.log10(v)) - 1
    return float(f"{math.ceil(v / 10 ** e - 1e-9) * 10 ** e:.1e}")
