"""tests/token_oracle.py checked on the CPU: the two float64 forms of every case small enough to loop against each other, the
measures, the input classes, the FLOOR constants of tests/test_token_edges_gpu.py, the 3 x margin between the two fp32
yardsticks that makes K = 6 a gate with a stated distance, the GELU polynomial of csrc/common.h against its own documented
bounds -- and the condition that gives the GPU file its point: on every bf16x3 case of its matrix the six-product bf16x3 scheme,
evaluated exactly, sits at or below e32, and the same scheme with ONE third-order piece product left out sits over the gate."""
import pytest
import torch

import token_oracle as to

YARD_MARGIN = 3.0
# {case: {(tensor, measure): measured larger / smaller}}: the two fp32 yardsticks more than 3 x apart, by name with the figure.
# The rule takes the larger of the two, so an entry only widens that tensor's own gate.  Both are the data gradient of rows whose
# mean is 100 standard deviations: torch's layer_norm backward against the hand-written one on the two-pass statistics.
YARD_OVER = {"ln-50x2048/offset": {("dx", "max"): 3.04}, "lnhead-2x77x128x3/offset": {("dx", "max"): 3.39, ("dx", "rms"): 3.13},
             # torch's fp32 matmul over 20000 rows on ANOTHER CPU's BLAS (the one beside the MI355X): 5.5e-7 / 6.6e-7 against the
             # 157 chains of 128 rows at 1.5e-7 / 2.1e-7; 2.3 on the BLAS this matrix was first measured with.  Only the upper end
             # of an entry is asserted, as in tests/test_attention_oracle_cpu.py.
             "tn-20000x96x288/act_scaled": {("dW", "max"): 3.69}, "tn-20000x96x288/offset": {("dW", "max"): 3.22}}
# The column sums (dgamma, dbeta, mis_colsum; kinds sum / hsum) are excepted as a KIND, not by name: their two yardsticks are
# apart by construction.  torch's fp32 sum down a column carries the rounding of one long fp32 accumulation (3137 rows: 2.5e-6);
# the kernels' order -- one fp32 partial per slab of 8 rows, the partials summed in double -- is all but exact (1e-8): measured
# up to 250 x apart on the offset class.  For them only the direction that matters is asserted: the kernels' order is never more
# than 3 x WORSE than torch's.  e32 is the larger of the two, so the gate of a sum is a gate on torch's fp32 sum.  (hsum, the
# affine gradients behind the output head: sums that cancel, each element on its own scale -- the figure of either yardstick is
# that of its unluckiest element, 3.1 x apart either way round; nothing is asserted between them.)
SUM_KINDS = ("sum", "hsum")


@pytest.mark.parametrize("name", [n for n in to.names() if to.small(n)])
def test_the_two_float64_forms_agree(name):
    c = to.case(name)
    r64 = to.references(name)[0]
    l64 = to.loop64(c)
    assert set(r64) == set(l64)
    for k in r64:
        assert r64[k].dtype == torch.float64 and r64[k].shape == l64[k].shape, k
        m = to.measure_of(k, l64[k], r64[k])
        # (sums of 10^4 float64 terms in another order: 1e-12 of a column's largest value; a column that is exactly zero in
        # one form is exactly zero in the other)
        assert m["max"] <= 1e-11 and m["rms"] <= 1e-12 and m["zero_ok"], (k, m)


def test_measure_sees_a_wrong_quiet_channel_and_a_touched_zero_channel():
    ref = torch.ones(6, 3, dtype=torch.float64)
    ref[:, 1] *= 1e-3
    ref[:, 2] = 0.0
    got = ref.clone()
    got[:, 1] *= 2.0                                     # entirely wrong, 1e-3 of the tensor's maximum
    m = to.measure_of("C", got, ref)
    assert m["max"] == pytest.approx(1.0) and m["rms"] < 1e-3 and m["zero_ok"]
    assert to.measure_of("dW", got.t(), ref.t())["max"] == pytest.approx(1.0)          # rows of dW are the output channels
    got = ref.clone()
    got[4, 2] = 1e-30
    assert not to.measure_of("C", got, ref)["zero_ok"]
    v = torch.tensor([1.0, 1e-3, 0.0], dtype=torch.float64)
    w = v.clone()
    w[1] *= 1.5
    assert to.measure_of("db", w, v)["max"] == pytest.approx(0.5)                       # every element on its own scale
    assert to.measure_of("rstd", w, v)["max"] == pytest.approx(0.5)
    assert to.measure_of("mean", w, v)["max"] == pytest.approx(5e-4)                    # mean: the tensor's largest value


def test_reduce_order_and_slices_follow_the_library():
    parts = [torch.full((1,), float(3 ** i)) for i in range(19)]
    want = 0.0
    lanes = [sum(3.0 ** k for k in range(kl, 19, 8)) for kl in range(8)]
    for s in lanes:
        want += s
    assert to.reduce_order(parts).item() == pytest.approx(want)
    assert to.slice_len(1000, 3) == 352 and to.slice_len(3072, 12) == 256 and to.slice_len(96, 1) == 96
    assert to.case("nt-98x768x3072/uniform")["slices"] > 1 and to.case("nt-300x200x1000/uniform")["slices"] > 1
    assert to.case("nt-200x96x48/uniform")["slices"] == 1 and to.case("tn-20000x96x288/uniform")["slices"] > 8
    assert to.slab_rows(50) == 8 and to.slab_rows(3137) % 8 == 0
    a, w = to.case("nt-300x200x1000/uniform")["A"], to.case("nt-300x200x1000/uniform")["W"]
    one, three = to.chain32(a, w, 1), to.chain32(a, w, 3)
    assert not torch.equal(one, three) and torch.allclose(one, three, rtol=1e-4, atol=1e-5)


def test_input_classes_are_what_they_claim():
    u, s, o = (to.case(f"nt-777x200x104/{cls}") for cls in to.CLASSES)
    assert u["A"].abs().max() <= 1 and u["ep"] and s["ep"] and not o["ep"]
    A, W = s["A"], s["W"]
    assert (A >= 0).all() and 0.4 < (A == 0).float().mean() < 0.6                      # an activation: half of it exactly zero
    live = A.amax(0) > 0
    assert (~live).sum() == 1 and A.amax(0)[live].max() / A.amax(0)[live].min() > 300   # K-channel scales over three decades
    wl = W.abs().amax(1)
    assert (wl == 0).sum() == 1 and wl[wl > 0].max() / wl[wl > 0].min() > 300 and (s["bias"][wl == 0] == 0).all()
    r64 = to.references("nt-777x200x104/act_scaled")[0]
    assert (r64["C"][:, wl == 0] == 0).all() and (r64["gelu"][:, wl == 0] == 0).all()
    assert 3.9 < o["A"].mean() < 4.1
    x = to.case("ln-50x96/offset")["x"].double()
    ratio = (x.mean(1) / x.std(1, unbiased=False).clamp(min=1e-300))
    const = x.std(1) == 0
    assert const.sum() == 3 and (ratio[~const] > 60).all()                             # row mean = 100 std
    var = x.var(1, unbiased=False)[~const]
    assert var.min() < 0.5 * to.EPS and var.max() > 1e6 * to.EPS                       # eps dominates / vanishes
    g = to.case("ln-50x96/act_scaled")
    assert (g["gamma"] == 0).sum() == 1 and (g["beta"][g["gamma"] == 0] == 0).all()
    for name in ("ln-50x96/offset", "ln-50x2048/act_scaled", "tn-3137x100x36/act_scaled", "lnhead-2x77x36x4/offset"):
        r64 = to.references(name)[0]
        for k in ("db", "dgamma", "dbeta", "sum"):
            if k in r64:                                  # no bias / affine gradient is a sum that cancels to nothing
                v = r64[k][r64[k] != 0].abs()
                assert v.min() > 1e-3 * v.median(), (name, k, v.min().item(), v.median().item())
    e = to.case("expandln-1x20x12x4x96x96x2/offset")
    tok = to.references("expandln-1x20x12x4x96x96x2/offset")[0]["tok"]
    assert (tok.mean(1).abs() > 3 * tok.std(1)).all()                                  # row mean far from zero
    assert e["ln"] and not to.case("expand-2x7x7x2x96x192x0/uniform")["ln"]


def test_floor_constants_are_the_largest_e32_of_the_matrix():
    """FLOOR of the GPU test = the largest e32 (either measure, the larger of the two yardsticks) per kind of tensor over the
    matrix, rounded up to two digits.  Both yardsticks run on one thread; the written constants may sit at most 10 % below /
    20 % above what this machine finds."""
    import test_token_edges_gpu as gpu
    worst = {}
    for name in to.names():
        e32 = to.references(name)[1]
        for k, by in e32.items():
            for m in to.MEASURES:
                if by[m] > worst.get(to.KIND_OF[k], (0.0,))[0]:
                    worst[to.KIND_OF[k]] = (by[m], name, k, m)
    print(worst, {k: to.ceil2(v[0]) for k, v in worst.items()})
    assert set(worst) == set(gpu.FLOOR) == set(to.KINDS)
    for k, (e, name, key, m) in worst.items():
        assert 0.8 * gpu.FLOOR[k] <= e <= 1.1 * gpu.FLOOR[k], (k, e, gpu.FLOOR[k], name, key, m)
    assert gpu.K == 6.0


@pytest.mark.parametrize("name", to.names())
def test_the_two_fp32_yardsticks_are_within_three_times_of_each_other(name):
    """Every tensor, both measures, either way round; a case listed in YARD_OVER must exceed the margin where it says and holds
    everywhere else.  K of the GPU test is that margin twice."""
    import test_token_edges_gpu as gpu
    _, _, ea, eb = to.references(name)
    over = YARD_OVER.get(name, {})
    for k in ea:
        for m in to.MEASURES:
            a, b = ea[k][m], eb[k][m]
            if a == 0.0 and b == 0.0:
                continue
            ratio = max(a, b) / max(min(a, b), 1e-300)
            print(f"{name} {k} {m}: torch fp32 {a:.2e} kernel order {b:.2e} ratio {ratio:.2f}")
            if to.KIND_OF[k] in SUM_KINDS and to.spec_of(name)["op"] != "tn":
                assert to.KIND_OF[k] == "hsum" or b <= YARD_MARGIN * a, (name, k, m, a, b)
            elif (k, m) in over:
                assert ratio <= 1.2 * over[(k, m)], (name, k, m, ratio)
            else:
                assert ratio <= YARD_MARGIN, (name, k, m, a, b)
    assert gpu.K == 2 * YARD_MARGIN


BF3_GROUPS = ("nt", "planes", "rega", "resln", "tn", "tnreg", "dwparts", "expand", "expandln", "expandln_rega")


@pytest.mark.parametrize("name", to.names(*BF3_GROUPS))
def test_the_gate_sees_a_lost_piece_product_and_passes_the_full_scheme(name):
    """The six-product bf16x3 scheme evaluated exactly is at or below e32 in both measures; the same with a.h * b.l, a.l * b.h
    or a.m * b.m left out is over the FULL gate max(6 e32, FLOOR) in at least one measure."""
    import test_token_edges_gpu as gpu
    c = to.case(name)
    key = to.GEMM_TENSOR[c["op"]]
    ref = to.references(name)[0][key]
    products = to.bf16x3_products(c)
    full = to.measure_of(key, to.bf16x3(c, None, products)[key], ref)
    gate = {m: max(gpu.K * to.yardstick(name, key, m), gpu.FLOOR[to.KIND_OF[key]]) for m in to.MEASURES}
    print(f"{name} {key}: e32 {to.yardstick(name, key, 'max'):.2e} / {to.yardstick(name, key, 'rms'):.2e}  "
          f"six products {full['max']:.2e} / {full['rms']:.2e}  gate {gate['max']:.2e} / {gate['rms']:.2e}")
    assert full["zero_ok"]
    for m in to.MEASURES:
        assert full[m] <= to.yardstick(name, key, m), (name, m, full[m])
    for drop in ("hl", "lh", "mm"):
        d = to.measure_of(key, to.bf16x3(c, drop, products)[key], ref)
        print(f"    without {drop}: {d['max']:.2e} / {d['rms']:.2e}  ({d['max'] / gate['max']:.1f} / {d['rms'] / gate['rms']:.1f} x the gate)")
        assert any(d[m] > gate[m] for m in to.MEASURES), (name, drop, d, gate)


def test_split3_is_exact_and_truncating():
    x = to.case("nt-200x96x48/offset")["A"]
    h, m, l = to.split3(x)
    assert torch.equal(h + m + l, x.double())                               # 24 bits in 8 + 8 + 8: nothing is lost
    for p in (h, m, l):
        assert torch.equal(p.float().view(torch.int32) & 0xFFFF, torch.zeros_like(x, dtype=torch.int32))      # bf16 values
    assert (h.abs() <= x.double().abs()).all() and (m * x.double() >= 0).all()                                # truncation


def test_matrix_holds_every_kernel_family_and_bracket():
    groups = {s["group"] for s in to.SPECS.values()}
    assert groups == {"nt", "short0", "planes", "rega", "resln", "tn", "tnreg", "dwparts", "expand", "expandln", "expandln_rega",
                      "ln", "lnhead", "head", "colsum"}
    widths = sorted({s["shape"][1] for s in to.SPECS.values() if s["group"] == "ln"})
    assert widths == [96, 100, 192, 384, 516, 768, 1024, 1536, 2048]
    for lo, hi in ((0, 128), (128, 256), (256, 512), (512, 768), (768, 1024), (1024, 1536), (1536, 1 << 30)):
        assert any(lo < C <= hi for C in widths), (lo, hi)                   # one width per bracket of mis_layernorm_fwd / _bwd
    assert {s["shape"][0] for s in to.SPECS.values() if s["group"] == "ln"} == {50, 3137}
    assert {s["shape"][2] for s in to.SPECS.values() if s["group"] == "lnhead"} == {36, 96, 128}
    assert sum(s["ep"] for s in to.SPECS.values()) == 5
    assert to.case("ln-50x96/offset") is to.case("ln-50x96/offset")          # built once, shared


# ---------------------------------------------------------------------------------------------------------------------
# GELU
# ---------------------------------------------------------------------------------------------------------------------
def test_gelu_grid_covers_the_range_and_the_sign_switch():
    x = to.gelu_grid()
    assert x.min() == -13 and x.max() == 13 and (x == 0).sum() >= 2
    assert (x.abs() < 1e-30).sum() > 10 and ((x != 0) & (x.abs() < 2.0 ** -126)).sum() >= 4        # +-tiny, denormals
    assert ((x > 0) & (x < 1e-6)).any() and ((x < 0) & (x > -1e-6)).any()                          # both sides of the switch


def test_gelu_polynomial_as_written_meets_its_documented_bounds():
    """The eight coefficients and the 0.3 of csrc/common.h, evaluated in float64 on the grid: |Phi error| <= 2e-7 and
    |gelu error| <= 4e-7 everywhere on [-13, 13] -- the coefficients are pinned here without a GPU.  (The fp32 evaluation adds
    its roundings; the GPU test holds the kernel.)"""
    x = to.gelu_grid()
    g64, d64 = to.gelu64(x)
    cdf, g, d = to.gelu_poly64(x)
    xd = x.double()
    phi = 0.5 * torch.erfc(-xd * 0.5 ** 0.5)
    e_phi, e_g = (cdf - phi).abs().max().item(), (g - g64).abs().max().item()
    tail = (xd <= -1) & (g64.abs() >= 2.0 ** -126)
    e_rel = ((g - g64).abs()[tail] / g64.abs()[tail]).max().item()
    print(f"polynomial in float64: |Phi error| {e_phi:.2e}  |gelu error| {e_g:.2e}  relative error of the negative tail {e_rel:.2e}  "
          f"|gelu' error| {(d - d64).abs().max().item():.2e}")
    assert e_phi <= to.GELU_PHI_BOUND and e_g <= to.GELU_BOUND
    import test_token_edges_gpu as gpu
    assert e_rel <= gpu.GELU_TAIL_POLY


def test_gelu_yardstick_is_torch_fp32_and_the_documented_bound():
    x = to.gelu_grid()
    g64, d64 = to.gelu64(x)
    g32, d32 = to.gelu32(x)
    m, md = to.gelu_measure(g32, g64, x), to.gelu_measure(d32, d64, x)
    print("torch fp32 gelu", m, "gelu'", md)
    assert m["max"] <= to.GELU_BOUND and md["max"] <= to.GELU_BOUND           # the erf form is within the documented bound ...
    assert m["tail"] > 0.5                                                    # ... and has no digit left in the negative tail
