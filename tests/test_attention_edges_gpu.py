"""The attention kernels (csrc/attention.hip + attention_impl.inc, csrc/attention_full.hip, csrc/swin3d.hip) against the float64
oracle of tests/attention_oracle.py, in units of fp32 noise.  tests/test_token_kernels_gpu.py, tests/test_unetr_gpu.py and
tests/test_swin3d_gpu.py hold the geometry at 1e-4 .. 2e-5 of the tensor's largest value on zero-mean uniform inputs, where every
softmax row is flat; this file holds the PRECISION per channel, and the semantics those inputs cannot see: rows near one-hot with
channel scales over three decades and exactly-zero channels (peaked), logits around 90 that need the row maximum (offset), and
cross-region pairs that compete with same-region pairs so that the ADDITIVE -100 of the shift mask differs from an exclusion
by O(1) (mask_competes).

Every output is pre-filled with NaN and must come back finite.  The primary class of a shape (peaked) runs on column slices of
wider buffers (NaN around an input, a sentinel around an output, which must survive), the further classes on dense tensors.
Every 2-D case asserts which kernels served it (mis_window_attention_path: the function the launchers themselves decide
through).  Each backward runs twice (bit-identical) and once more accumulating onto a non-zero table gradient (base + gradient
to the rounding of one fp32 add); the 3-D and the full backward consume the out / stats their HIP forward wrote.

The rule, per tensor, in both measures of attention_oracle.measure (max: the worst column's largest error over that column's
largest reference value; rms: over the whole tensor), with no per-case K:

    err_hip <= max(K * e32, FLOOR[kind]),    K = 6

e32 = the larger of two fp32 errors against float64 on the same bits: torch's fp32 CPU operators, and a plain fp32 loop in the
kernels' order of operations (attention_oracle.plain32).  tests/test_attention_oracle_cpu.py holds the two within 3 x of each
other (one tensor excepted there by name at 3.1): K = 6 is that margin twice.  FLOOR = the largest e32 of the matrix per kind
(recomputed there).

Paths: the 2-D matrix runs under set_split_precision(0) (fp32 MFMA) and (7) (bf16x3 MFMA); the vector-pipe kernels run through
their production condition (qkv a column slice of one NaN-filled buffer of >= 2^31 bytes; the split backward must refuse it)
and, in a child process with MIS_ATTN_VALU=1, through the chunked backward (23 samples in chunks of 2, the last one ragged).

Measured on an MI355X (this file's own run; `MIS_ATTN_STATS=<file>` writes every figure as JSON).  ratio = HIP / max(e32, FLOOR / K):
the error in units of fp32 noise, the gate is at 6.  46 tests over 32 cases, all pass, none over the gate, 9.5 s wall (the child
process of the chunked backward: 6 s, most of it its own start and the CPU references of 18032 tokens; every other test under 1 s).

    kernel                                                                            kind   e32 (max measure)    HIP max   ratio  HIP rms   ratio  worst case (max measure)
    ws7 attn_fwd_mfma_kernel<0>                        (fp32 MFMA)                    out    3.9e-07 .. 7.2e-06  9.50e-06  1.33  2.54e-06  1.00  w7-2x14x14x3-s3/mask_competes
    ws7 attn_bwd_mfma_kernel<0> + attn_dtable_sum_kernel                              dqkv   4.6e-07 .. 1.9e-05  1.61e-05  0.86  4.24e-06  0.46  w7-2x14x14x3-s3/offset
    ws7 attn_bwd_mfma_kernel<0> + attn_dtable_sum_kernel                              dtable 2.5e-07 .. 5.3e-06  8.12e-06  1.53  5.66e-06  1.15  w7-2x14x14x3-s3/offset
    ws7 attn_fwd_mfma_kernel<1>                        (bf16x3 MFMA)                  out    3.9e-07 .. 7.2e-06  4.73e-06  0.96  1.53e-06  0.60  w7-1x14x14x1-s6/peaked
    ws7 attn_bwd_mfma_kernel<1> + attn_dtable_sum_kernel                              dqkv   4.6e-07 .. 1.9e-05  1.01e-05  0.56  2.02e-06  0.22  w7-2x14x14x3-s3/mask_competes
    ws7 attn_bwd_mfma_kernel<1> + attn_dtable_sum_kernel                              dtable 2.5e-07 .. 5.3e-06  3.53e-06  0.79  2.12e-06  0.65  w7-3x14x21x2-s3/peaked
    ws8 attn_fwd_mfma_kernel<0>                                                       out    4.3e-07 .. 8.1e-06  8.71e-06  1.30  2.45e-06  1.00  w8-1x8x8x6-s0/peaked
    ws8 attn_bwd_mfma_kernel<0> + attn_dtable_sum_kernel                              dqkv   5.3e-07 .. 1.9e-05  1.41e-05  0.75  3.58e-06  0.39  w8-1x16x24x2-s4/offset
    ws8 attn_bwd_mfma_kernel<0> + attn_dtable_sum_kernel                              dtable 2.7e-07 .. 6.1e-06  7.45e-06  1.21  5.06e-06  1.01  w8-1x16x24x2-s4/offset
    ws8 attn_fwd_mfma_kernel<1>                                                       out    4.3e-07 .. 8.1e-06  5.09e-06  0.63  1.37e-06  0.56  w8-1x16x24x2-s4/mask_competes
    ws8 attn_bwd_mfma_kernel<1> + attn_dtable_sum_kernel                              dqkv   5.3e-07 .. 1.9e-05  8.79e-06  0.47  1.86e-06  0.20  w8-1x16x24x2-s4/offset
    ws8 attn_bwd_mfma_kernel<1> + attn_dtable_sum_kernel                              dtable 2.7e-07 .. 6.1e-06  3.09e-06  0.61  2.41e-06  0.59  w8-1x16x24x2-s4/peaked
    ws7 attn_fwd_kernel                                (2.1 GB buffer: vector pipe)   out    2.2e-06 .. 2.2e-06  1.61e-06  0.73  3.04e-07  0.22  w7-2x14x14x3-s3/peaked
    ws7 attn_bwd_kernel + attn_ds_reduce_kernel + attn_dtable_kernel                  dqkv   2.9e-06 .. 2.9e-06  2.66e-06  0.29  3.43e-07  0.04  w7-2x14x14x3-s3/peaked
    ws7 attn_bwd_kernel + attn_ds_reduce_kernel + attn_dtable_kernel                  dtable 1.8e-06 .. 1.8e-06  1.28e-06  0.71  7.50e-07  0.73  w7-2x14x14x3-s3/peaked
    ws8 attn_fwd_kernel                                (2.1 GB buffer)                out    2.5e-06 .. 2.5e-06  1.49e-06  0.59  3.63e-07  0.26  w8-1x16x16x3-s4/peaked
    ws8 attn_bwd_kernel + attn_ds_reduce_kernel + attn_dtable_kernel                  dqkv   5.1e-06 .. 5.1e-06  2.68e-06  0.29  3.90e-07  0.04  w8-1x16x16x3-s4/peaked
    ws8 attn_bwd_kernel + attn_ds_reduce_kernel + attn_dtable_kernel                  dtable 1.3e-06 .. 1.3e-06  1.12e-06  0.89  7.10e-07  0.69  w8-1x16x16x3-s4/peaked
    ws7 attn_fwd_kernel                                (MIS_ATTN_VALU, chunks of 2)   out    2.4e-06 .. 2.4e-06  1.75e-06  0.72  3.35e-07  0.24  w7-23x28x28x3-s3/peaked
    ws7 attn_bwd_kernel + attn_ds_reduce_kernel + attn_dtable_kernel                  dqkv   3.7e-06 .. 3.7e-06  4.29e-06  0.47  3.75e-07  0.04  w7-23x28x28x3-s3/peaked
    ws7 attn_bwd_kernel + attn_ds_reduce_kernel + attn_dtable_kernel                  dtable 1.6e-06 .. 1.6e-06  1.02e-06  0.64  7.81e-07  0.68  w7-23x28x28x3-s3/peaked
    full_attn_fwd_kernel                                                              out    0.0e+00 .. 8.3e-06  8.34e-06  1.06  1.40e-06  0.99  full-43x9x12/peaked
    full_attn_bwd_kernel<false> + <true>                                              dqkv   0.0e+00 .. 5.5e-05  5.43e-05  1.00  8.82e-06  0.96  full-2x70x3/offset
    attn3d_fwd_kernel                                                                 out    3.8e-07 .. 6.6e-06  5.74e-06  0.87  1.60e-06  0.79  w3d-2x8x8x8x3-s/mask_competes
    attn3d_bwd_q_kernel + attn3d_bwd_kv_kernel + attn3d_table_reduce_kernel           dqkv   6.4e-07 .. 2.4e-05  3.74e-05  1.54  2.05e-06  0.22  w3d-2x8x8x8x3-s/offset
    attn3d_bwd_q_kernel + attn3d_bwd_kv_kernel + attn3d_table_reduce_kernel           dtable 5.0e-07 .. 4.5e-06  4.67e-06  1.43  3.55e-06  1.03  w3d-2x8x8x8x3-s/peaked

    (e32 is computed on the machine that runs the test: the CPU beside the MI355X puts plain32's dqkv of w3d-2x8x8x8x3-s/offset at
    2.4e-5, another CPU's BLAS at 3.5e-5.)  Every kernel is within 1.6 x fp32 noise on every tensor; no kernel had to change.  The
    candidates the matrix was built to catch are not findings: __expf and the rescaling branch of the 3-D running maximum stay
    below torch's fp32 on out (0.87 x) -- the 1.54 on its dqkv is delta = dO . O from the rounded output against a mean-4 v, which
    the plain fp32 loop in the same order shows on the CPU (3.1 x torch's fp32 there); the bf16x3 form, which splits P and dS
    into pieces after the softmax, is CLOSER to float64 than the fp32-MFMA form on all six of its rows in both measures
    (0.20 .. 0.96 against 0.39 .. 1.53).

Scratch builds, not committed (run once against this file and the three older attention tests): a library whose mask EXCLUDES
cross-region pairs fails exactly the five mask_competes cases here (out off by 2.0 against a gate of 4.3e-5) and passes every
older test; a library whose 2-D bf16x3 products lose one third-order piece (a.h * b.l) fails all thirteen bf16x3 cases here
(w7-2x14x14x3-s3/peaked out: 1.07e-4 against 1.3e-5) and passes every older test.
"""
import ctypes
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import attention_oracle as ao
import oracle_kit as kit
from oracle_kit import NAN

pytestmark = pytest.mark.gpu

K = 6.0
FLOOR = {"out": 8.3e-6,      # largest e32 of the matrix: 8.27e-6 (full-2x70x3/offset, max: 70 keys of a mean-4 v at logits near 128)
         "dqkv": 5.5e-5,     # 5.46e-5 (full-2x70x3/offset, max: dS = P (dP - delta) cancels against a mean-4 v)
         "dtable": 6.2e-6}   # 6.13e-6 (w8-1x16x24x2-s4/offset, max)
# {case: {(label, measure)}}: tensors known to sit over the gate, by name, each with its measured figure in a comment.  Strict
# and narrow as in tests/test_conv_edges_gpu.py: the case xfails only when exactly these entries are over the gate.
OVER_THE_GATE = {}
LEAD, TRAIL = 4, 8            # columns of the wider buffer before / after a slice (16-byte aligned, row strides % 4 == 0)
_in, _out = functools.partial(kit.place, lead=LEAD, trail=TRAIL), functools.partial(kit.Out, lead=LEAD, trail=TRAIL)
STATS = []                    # (group, case, label, kind, measure, e32, hip, kernel)
KERNELS_2D = {"mfma_f32": ("attn_fwd_mfma_kernel<0>", "attn_bwd_mfma_kernel<0> + attn_dtable_sum_kernel"),
              "mfma_bf16x3": ("attn_fwd_mfma_kernel<1>", "attn_bwd_mfma_kernel<1> + attn_dtable_sum_kernel"),
              "valu": ("attn_fwd_kernel", "attn_bwd_kernel + attn_ds_reduce_kernel + attn_dtable_kernel")}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")


def _tops():
    from mis_hip import tops
    return tops


def _print_report():
    for (kernel, kind, m), r in kit.worst_rows(((kernel, kind, m), f"{cid} {label}", e32, ehip, max(e32, FLOOR[kind] / K))
                                               for group, cid, label, kind, m, e32, ehip, kernel in STATS):
        print(f"\n[attention edges] {kernel:74s} {kind:6s} {m:3s} e32 {r['lo']:.1e} .. {r['hi']:.1e}  hip max {r['hip']:.2e}  "
              f"worst hip/max(e32, floor/K) {r['ratio']:.2f} ({r['at']})", end="")
    print()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if not STATS:
        return
    _print_report()
    kit.report(STATS, "MIS_ATTN_STATS", {"stats": STATS})


# ---------------------------------------------------------------------------------------------------------------------
# buffers and comparison
# ---------------------------------------------------------------------------------------------------------------------
class _Check:
    def __init__(self, group, name):
        self.group, self.name = group, name
        self.c = ao.case(name)
        self.z = ao.sizes(self.c)
        self.r64 = ao.references(name)[0]
        self.gate = kit.Gate(K, FLOOR, OVER_THE_GATE, STATS)

    def __call__(self, kind, got, kernel, label="", ref=None, e32=None):
        return self.gate.tensor(self.name, label or kind, kind, got, self.r64[kind] if ref is None else ref, ao.measure,
                                {ms: ao.yardstick(self.name, kind, ms) if e32 is None else e32[ms] for ms in ao.MEASURES},
                                (self.group, self.name), (kernel,), width=10)

    def accumulated(self, dt, launch):
        """``launch(dtable, accumulate=True)`` onto a non-zero table gradient: base + the gradient ``dt`` of the plain launch (held
        to the oracle already) to the rounding of ONE fp32 add -- the kernels add their rounded sum to what is there."""
        base = self.r64["dtable"].flip(0).float().cuda() * 0.5 + 0.25
        acc = base.clone()
        launch(acc, True)
        want = base.double() + dt.double()
        err = (acc.double() - want).abs()
        assert bool((err <= 2.0 ** -24 * want.abs()).all()), (self.name, "accumulate_table", err.max().item())

    def done(self):
        self.gate.done(self.name)


def _layout(c):
    return "slice" if c["cls"] == "peaked" else "dense"


# ---------------------------------------------------------------------------------------------------------------------
# 2-D window attention
# ---------------------------------------------------------------------------------------------------------------------
def _run_win2d(group, name, expect, qkv_view=None, split_refused=False):
    """Forward, backward (twice), backward accumulating, each asserting its path.  qkv_view: a device view to use as qkv (the
    fallback's slice of a huge buffer) instead of the case's layout."""
    tops = _tops()
    chk = _Check(group, name)
    c, z = chk.c, chk.z
    B, H, W, nH, shift, ws = c["shape"]
    T, C, scale = z["T"], z["C"], z["scale"]
    lay = "dense" if qkv_view is not None else _layout(c)
    qkv = qkv_view if qkv_view is not None else _in(c["qkv"], lay)
    dout, table = _in(c["dout"], lay), c["table"].cuda()
    kf, kb = (f"ws{ws} {k}" for k in KERNELS_2D[expect])
    out = _out((T, C), lay)
    assert tops.window_attention_path(B, H, W, nH, qkv, out.v, window=ws) == expect
    tops.window_attention_fwd(qkv, out.v, table, B, H, W, nH, shift, scale, window=ws)
    chk("out", out.v, kf)
    assert out.untouched()

    def bwd(dq, dt, accumulate=False):
        assert tops.window_attention_path(B, H, W, nH, qkv, dout, dq, window=ws) == expect
        tops.window_attention_bwd(qkv, dout, dq, table, dt, B, H, W, nH, shift, scale, accumulate_table=accumulate, window=ws)

    dq, dq2 = _out((T, 3 * C), lay), _out((T, 3 * C), lay)
    dt, dt2 = torch.full_like(table, NAN), torch.full_like(table, NAN)
    bwd(dq.v, dt)
    chk("dqkv", dq.v, kb)
    chk("dtable", dt, kb)
    bwd(dq2.v, dt2)
    assert torch.equal(dq.v, dq2.v) and torch.equal(dt, dt2), (name, "the backward is not deterministic")
    assert dq.untouched() and dq2.untouched()
    dq3 = _out((T, 3 * C), lay)
    chk.accumulated(dt, lambda t, acc: bwd(dq3.v, t, acc))
    assert torch.equal(dq.v, dq3.v)
    partials = tops.window_attention_table_partials(B, H, W, nH, window=ws)
    if split_refused:
        # the split form cannot serve buffers the MFMA kernels cannot index: its second half does not see the strides
        wsp = tops.window_attention_workspace(B, H, W, nH, window=ws)
        dq4 = torch.full((T, 3 * C), NAN, device="cuda")
        with pytest.raises(RuntimeError, match="MIS_ERR_UNSUPPORTED"):
            tops.window_attention_bwd_parts(qkv, dout, dq4, table, wsp, B, H, W, nH, shift, scale, window=ws)
        torch.cuda.synchronize()
        assert torch.isnan(dq4).all()
    return chk, partials


@pytest.mark.parametrize("mask,expect", [(0, "mfma_f32"), (7, "mfma_bf16x3")])
@pytest.mark.parametrize("name", ao.names("win2d"))
def test_window_attention_2d(name, mask, expect):
    """The MFMA kernels of both window sizes in both arithmetics: a ragged group of waves (3 units), shifts 0 / 1 / 3 / 4 / 6,
    one and several windows per image, every input class on one shifted shape per window size."""
    tops = _tops()
    prev = tops.set_split_precision(mask)
    try:
        chk, partials = _run_win2d("win2d", name, expect)
        B, H, W, nH, shift, ws = chk.c["shape"]
        assert partials == (B * (H // ws) * (W // ws), (2 * ws - 1) ** 2 * nH)
        chk.done()
    finally:
        tops.set_split_precision(prev)


@pytest.mark.parametrize("name", ao.names("fallback"))
def test_window_attention_2d_vector_pipe_fallback(name):
    """attn_fwd_kernel / attn_bwd_kernel / attn_ds_reduce_kernel / attn_dtable_kernel through the condition production reaches
    them by: qkv is the column slice [:, :3C] of ONE buffer whose row stride is the smallest multiple of 4 with
    B*H*W*ld*4 >= 2^31 (2.1 GB, NaN-filled, allocated here and freed afterwards); out, dout and dqkv are dense."""
    c, z = ao.case(name), ao.sizes(ao.spec_of(name))
    T, C = z["T"], z["C"]
    ld = -(-(1 << 29) // T)
    ld += -ld % 4
    assert T * ld * 4 >= 1 << 31 > T * (ld - 4) * 4
    big, view = torch.full((T, ld), NAN, device="cuda"), None
    try:
        view = big[:, :3 * C]
        view.copy_(c["qkv"].cuda())
        assert view.stride(0) == ld
        chk, partials = _run_win2d("fallback", name, "valu", qkv_view=view, split_refused=True)
        assert partials is not None            # the shape query sees no buffer: it describes the MFMA layout of small launches
        assert bool(torch.isnan(big[:, 3 * C:3 * C + 64]).all())
        chk.done()
    finally:
        del big, view
        torch.cuda.empty_cache()


def _valu_child(name):
    """Runs in a process of its own with MIS_ATTN_VALU set (read once per process): the chunked vector-pipe backward."""
    assert os.environ.get("MIS_ATTN_VALU")
    from mis_hip import lib
    tops = _tops()
    c = ao.case(name)
    B, H, W, nH, shift, ws = c["shape"]
    chunks = -(-B // 2)           # bwd_chunk picks 2: 1104 units -> two rounds of 552 waves; the last chunk holds one sample
    want = (chunks * (H // ws) * (W // ws) + 1) * nH * (ws * ws) ** 2 * 4
    assert int(lib.load().mis_window_attention_workspace_bytes_ws(B, H, W, nH, ws)) == want
    chk, partials = _run_win2d("valu", name, "valu")
    assert partials is None, "window_attention_table_partials must refuse (MIS_ERR_UNSUPPORTED) under MIS_ATTN_VALU"
    rows, cols = ctypes.c_longlong(0), ctypes.c_int(0)
    assert lib.load().mis_window_attention_table_partials(B, H, W, nH, ws, ctypes.byref(rows), ctypes.byref(cols)) == -2
    print("STATS " + json.dumps(STATS))
    chk.done()


@pytest.mark.parametrize("name", ao.names("valu"))
def test_window_attention_2d_chunked_vector_pipe_backward(name):
    """MIS_ATTN_VALU=1 in a fresh child process: (23, 28, 28, 3, 3, 7) is 1104 units, bwd_chunk picks 2 samples per wave and
    the last chunk is ragged (23 = 11 * 2 + 1).  The child asserts the path, the workspace of 12 chunks, the refusal of
    window_attention_table_partials, and holds out / dqkv / dtable to this file's gate."""
    env = dict(os.environ, MIS_ATTN_VALU="1",
               PYTHONPATH=os.pathsep.join([PKG, ROOT, os.path.dirname(os.path.abspath(__file__)), os.environ.get("PYTHONPATH", "")]))
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--valu-child", name]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    print(r.stdout[-6000:])
    for line in r.stdout.splitlines():
        if line.startswith("STATS "):
            STATS.extend(tuple(row) for row in json.loads(line[6:]))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert any(s[0] == "valu" and s[3] == "dtable" for s in STATS)


# ---------------------------------------------------------------------------------------------------------------------
# full attention (UNETR)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ao.names("full"))
def test_full_attention(name):
    """N = 1, 64, 65 (the edge of a 64-key pass), 256 (the most the kernel takes); row chunks shorter than a workgroup's 8
    waves, ragged last chunks, and one chunk of more rows than tokens (B * nH >= 512); the backward reads the statistics the
    forward kept."""
    tops = _tops()
    chk = _Check("full", name)
    c, z = chk.c, chk.z
    B, N, nH = c["shape"]
    T, C, scale = z["T"], z["C"], z["scale"]
    lay = _layout(c)
    qkv, dout = _in(c["qkv"], lay), _in(c["dout"], lay)
    out = _out((T, C), lay)
    stats = torch.full((B * nH * N * 2,), NAN, device="cuda")
    tops.full_attention_fwd(qkv, out.v, stats, B, N, nH, scale)
    chk("out", out.v, "full_attn_fwd_kernel")
    assert out.untouched() and torch.isfinite(stats).all()
    dq, dq2 = _out((T, 3 * C), lay), _out((T, 3 * C), lay)
    tops.full_attention_bwd(qkv, dout, dq.v, stats, B, N, nH, scale)
    chk("dqkv", dq.v, "full_attn_bwd_kernel<false> + <true>")
    tops.full_attention_bwd(qkv, dout, dq2.v, stats, B, N, nH, scale)
    assert torch.equal(dq.v, dq2.v), (name, "the backward is not deterministic")
    assert dq.untouched() and dq2.untouched()
    chk.done()


# ---------------------------------------------------------------------------------------------------------------------
# 3-D window attention (SwinUNETR)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ao.names("win3d"))
def test_window_attention_3d(name):
    """Clipped 4^3 windows without a mask, 7^3 windows with the shift mask (every class), a padded volume whose padding tokens
    are ordinary keys, and 27 windows x 6 heads; the one-pass running maximum of the forward meets keys in every order of
    magnitude; the backward consumes the out and stats the HIP forward wrote."""
    tops = _tops()
    chk = _Check("win3d", name)
    c, z = chk.c, chk.z
    nH, n, nW, BW, T, C = z["nH"], z["n"], z["nW"], z["G"], z["T"], z["C"]
    lay = _layout(c)
    region = None
    if z["shifted"]:
        from oracle.swinunetr import region_ids
        region = region_ids(z["pdims"], z["win"], z["shift"]).to(torch.int32).contiguous().cuda()
    qkv, dout, table = _in(c["qkv"], lay), _in(c["dout"], lay), c["table"].cuda()
    out = _out((T, C), lay)
    stats = torch.full((BW * nH * n * 2,), NAN, device="cuda")
    tops.win3d_attn_fwd(qkv, out.v, stats, table, region, BW, nW, n, nH)
    chk("out", out.v, "attn3d_fwd_kernel")
    assert out.untouched() and torch.isfinite(stats).all()
    kb = "attn3d_bwd_q_kernel + attn3d_bwd_kv_kernel + attn3d_table_reduce_kernel"

    def bwd(dq, dt, accumulate=False):
        tops.win3d_attn_bwd(qkv, out.v, dout, dq, stats, table, region, dt, BW, nW, n, nH, accumulate_table=accumulate)

    dq, dq2, dq3 = (_out((T, 3 * C), lay) for _ in range(3))
    dt, dt2 = torch.full_like(table, NAN), torch.full_like(table, NAN)
    bwd(dq.v, dt)
    chk("dqkv", dq.v, kb)
    chk("dtable", dt, kb)
    bwd(dq2.v, dt2)
    assert torch.equal(dq.v, dq2.v) and torch.equal(dt, dt2), (name, "the backward is not deterministic")
    chk.accumulated(dt, lambda t, acc: bwd(dq3.v, t, acc))
    assert torch.equal(dq.v, dq3.v)
    assert dq.untouched() and dq2.untouched() and dq3.untouched()
    chk.done()


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--valu-child", sys.argv
    _valu_child(sys.argv[2])
