"""tests/conv_oracle.py checked on the CPU: the two float64 forms of every case against each other (torch's convolution with
autograd / a plain sum over the taps), the plain Winograd form in float64 against them, the FLOOR constants of
tests/test_conv_edges_gpu.py (the largest e32 of the matrix per kind of tensor), and the margin that makes K = 6 a gate with a
stated distance: on every case a Winograd kernel serves, the fp32 Winograd ALGORITHM is within 3 x the direct form's fp32 error."""
import pytest
import torch

import conv_oracle as co

WINO_MARGIN = 3.0


def _rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


@pytest.mark.parametrize("name", co.names())
def test_the_two_float64_forms_agree(name):
    c = co.case(name)
    r64 = co.references(name)[0]
    p64 = co.plain64(c, c["kinds"])
    for k in c["kinds"]:
        assert r64[k].dtype == torch.float64 and r64[k].shape == p64[k].shape
        assert _rel(p64[k], r64[k]) <= 1e-12, (k, _rel(p64[k], r64[k]))
        m = co.measure(p64[k], r64[k], co.dim_of(c, k))
        assert m["max"] <= 1e-12 and m["rms"] <= 1e-12 and m["zero_ok"]


@pytest.mark.parametrize("name", [n for n in co.names() if co.winograd_eligible(co.spec_of(n))])
def test_winograd_form_is_exact_in_float64(name):
    c = co.case(name)
    r64 = co.references(name)[0]
    w64 = co.winograd(c, torch.float64, c["kinds"])
    for k in c["kinds"]:
        m = co.measure(w64[k], r64[k], co.dim_of(c, k))
        assert m["max"] <= 1e-12 and m["rms"] <= 1e-12, (k, m)


WINO_CASES = [n for n in co.names() if co.winograd_eligible(co.spec_of(n))]
# Cases where the fp32 ALGORITHM itself is more than 3 x the direct form's error (a finding about F(2, 3) at that shape, not
# about a kernel): taken out of the Winograd half of the matrix by name, {(kind, measure): measured winograd32 / e32}.  No
# Winograd kernel serves them (conv_wino_select refuses 4 x 4 images), and served_by_winograd must say so.
WINO_OVER = {"direct2d-4x4-256/relu_scaled": {("y", "max"): 3.44, ("dx", "max"): 3.45}}      # 4 x 256 -> 256 at 4 x 4: 4 tiles per image


@pytest.mark.parametrize("name", WINO_CASES)
def test_winograd32_is_within_three_times_the_direct_form(name):
    """On every Winograd-eligible case (k = 3, even sizes), every compared tensor, both measures: winograd32 <= 3 x e32.  A case
    listed in WINO_OVER must exceed 3 where it says, must not be served by a Winograd kernel, and holds everywhere else."""
    import test_conv_edges_gpu as gpu
    c = co.case(name)
    _, e32, ew = co.references(name)
    assert ew is not None
    over = WINO_OVER.get(name, {})
    for k in c["kinds"]:
        for m in co.MEASURES:
            ratio = ew[k][m] / e32[k][m]
            print(f"{name} {k} {m}: e32 {e32[k][m]:.2e} winograd32 {ew[k][m]:.2e} ratio {ratio:.2f}")
            if (k, m) in over:
                assert ratio > WINO_MARGIN and not co.served_by_winograd(c, k), (name, k, m, ratio)
            else:
                assert ratio <= WINO_MARGIN, (name, k, m, ew[k][m], e32[k][m])
    assert gpu.K == 2 * WINO_MARGIN


def test_floor_constants_are_the_largest_e32_of_the_matrix():
    """FLOOR of the GPU test = the largest e32 (either measure) per kind of tensor over the tensors the matrix compares, rounded
    up to two digits.  reference32 runs on one thread, so the figures do not follow the machine's core count; the written
    constants may sit at most 10 % below / 20 % above what this machine finds."""
    import test_conv_edges_gpu as gpu
    worst = {}
    for name in co.names():
        c = co.case(name)
        e32 = co.references(name)[1]
        for k in c["kinds"]:
            for m in co.MEASURES:
                if e32[k][m] > worst.get(k, (0.0,))[0]:
                    worst[k] = (e32[k][m], name, m)
    print(worst, {k: co.ceil2(v[0]) for k, v in worst.items()})
    assert set(worst) == set(gpu.FLOOR) == set(co.KINDS)
    for k, (e, name, m) in worst.items():
        assert 0.8 * gpu.FLOOR[k] <= e <= 1.1 * gpu.FLOOR[k], (k, e, gpu.FLOOR[k], name, m)
    assert gpu.K == 6.0


def test_measure_sees_a_wrong_quiet_channel_and_a_touched_zero_channel():
    ref = torch.ones(2, 3, 1, 4, 4, dtype=torch.float64)
    ref[:, 1] *= 1e-3
    ref[:, 2] = 0.0
    got = ref.clone()
    got[:, 1] *= 2.0                                     # entirely wrong, 1e-3 of the tensor's maximum
    m = co.measure(got, ref)
    assert m["max"] == pytest.approx(1.0) and m["rms"] < 1e-3 and m["zero_ok"]
    got = ref.clone()
    got[0, 2, 0, 0, 0] = 1e-30
    assert not co.measure(got, ref)["zero_ok"]
    w = torch.ones(3, 2, 1, 3, 3, dtype=torch.float64)
    w[:, 1] *= 1e-3
    g = w.clone()
    g[:, 1] *= 2.0
    assert co.measure(g, w, 1)["max"] == pytest.approx(1.0) and co.measure(g, w, 0)["max"] == pytest.approx(1e-3, rel=1e-6)


def test_input_classes_and_matrix():
    """The classes are what they claim (half zeros, channel scales over three decades, a mean of four standard deviations) and
    every family of the issue is in the matrix with all four classes once."""
    c = co.case("wino-v2-partial-boxes/relu_scaled")
    x = c["x"]
    assert 0.45 < (x == 0).float().mean().item() < 0.55 and (x >= 0).all()
    amax = x.amax((0, 2, 3, 4))
    assert amax.max().item() / amax.min().item() > 100
    dmax = c["dy"].abs().amax((0, 2, 3, 4))
    assert dmax.max().item() / dmax.min().item() > 100 and (c["dy"] < 0).any()
    o = co.case("wino-v0/offset")["x"]
    assert 3.5 < o.mean().item() < 4.5 and 0.8 < o.std().item() < 1.2
    u = co.case("wino-v0/uniform")
    assert u["x"].abs().max().item() <= 1 and u["dy"].abs().max().item() <= 1 and u["w"].abs().max().item() <= 0.2
    for group in ("fwd3d", "split", "fwd2d", "wgrad", "k2s2", "gemm", "up2d"):
        assert any(co.SPECS[n.split("/")[0]]["classes"] == co.X_CLASSES for n in co.names(group)), group
    assert {co.SPECS[n.split("/")[0]]["fwd"][1] for n in co.names("split")} == {2, 4}
    assert {s["wgrad"] for s in co.SPECS.values() if s["group"] == "wgrad"} >= set(co.WG.values())
    k2 = [co.SPECS[n.split("/")[0]] for n in co.names("k2s2")]
    assert {(s["op"], s["shape"][1], s["shape"][2]) for s in k2} == {("down", 16, 32), ("down", 32, 64), ("up", 32, 16), ("up", 64, 32)}
    wo = {(s["shape"][5] // 2 if s["op"] == "down" else s["shape"][5]) % 16 == 0 for s in k2}
    assert wo == {True, False}                                           # both lane-group forms of the k2s2 weight gradient
    assert co.case("wino-v0/uniform") is co.case("wino-v0/uniform")       # built once, shared
