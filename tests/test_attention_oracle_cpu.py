"""tests/attention_oracle.py checked on the CPU: the two float64 forms of every case against each other (torch's operators with
autograd over roll / partition; an explicit loop over windows and heads with the backward by hand over integer formulas), the
measures, the input classes, why ``mask_competes`` exists (an exclusion instead of the additive -100 is invisible on the uniform
class and O(1) there), the FLOOR constants of tests/test_attention_edges_gpu.py, and the margin that makes K = 6 a gate with a
stated distance: the two fp32 yardsticks (torch's fp32 operators / the kernels' order of operations in plain fp32) are within
3 x of each other on every tensor of the matrix but one, named below."""
import pytest
import torch

import attention_oracle as ao

# The two fp32 yardsticks against each other, either way round: measured <= 1.34 on every tensor of the matrix (out 1.33, dqkv 1.22,
# dtable 1.34) but one, which is at 3.12 -- so the largest measured factor is 3.12 and K = 6 is NOT twice it.  As
# tests/test_conv_oracle_cpu.py does for its one entry beyond 3, the margin stays at 3 (K = 6 is fixed for both families) and the
# one tensor is excepted by name with its figure:
YARD_MARGIN = 3.0
# {(kind, measure): measured larger / smaller}.  delta = dO . O from the ROUNDED output (the 3-D kernels' order) instead of
# sum P dP costs the data gradient of a mean-4 v that much: 3.5e-5 against 1.1e-5.  The rule takes the larger of the two, so the
# entry only widens that tensor's own gate.
YARD_OVER = {"w3d-2x8x8x8x3-s/offset": {("dqkv", "max"): 3.12}}


@pytest.mark.parametrize("name", ao.names())
def test_the_two_float64_forms_agree(name):
    c = ao.case(name)
    r64 = ao.references(name)[0]
    p64 = ao.plain(c)
    assert set(r64) == set(p64) == set(ao.kinds_of(c))
    for k in r64:
        assert r64[k].dtype == torch.float64 and r64[k].shape == p64[k].shape
        m = ao.measure(p64[k], r64[k])
        assert m["max"] <= 1e-12 and m["rms"] <= 1e-12 and m["zero_ok"], (k, m)
        assert (p64[k] - r64[k]).abs().max().item() <= 1e-12 * max(r64[k].abs().max().item(), 1e-300), k


@pytest.mark.parametrize("name", [n for n in ao.names() if ao.sizes(ao.spec_of(n))["shifted"]])
def test_geometry_formulas_agree_with_roll_and_partition(name):
    """Token rows, table indices and region ids of the two forms are the same integers (the float64 agreement above could not
    tell two regions apart on an input where the mask decides nothing)."""
    spec = ao.spec_of(name)
    perm, index, region = ao.torch_geometry(spec)
    perm2, index2, region2, codes = ao.plain_geometry(spec)
    assert (perm is None and perm2 is None) or torch.equal(perm, perm2)
    assert torch.equal(index, index2)
    same, same2 = region[:, :, None] == region[:, None, :], region2[:, :, None] == region2[:, None, :]
    assert torch.equal(same, same2) and codes.shape == region.shape
    assert (~same).any()


def test_measure_sees_a_wrong_quiet_channel_and_a_touched_zero_channel():
    ref = torch.ones(6, 3, dtype=torch.float64)
    ref[:, 1] *= 1e-3
    ref[:, 2] = 0.0
    got = ref.clone()
    got[:, 1] *= 2.0                                     # entirely wrong, 1e-3 of the tensor's maximum
    m = ao.measure(got, ref)
    assert m["max"] == pytest.approx(1.0) and m["rms"] < 1e-3 and m["zero_ok"]
    got = ref.clone()
    got[4, 2] = 1e-30
    assert not ao.measure(got, ref)["zero_ok"]
    assert ao.measure(ref, ref) == {"max": 0.0, "rms": 0.0, "zero_ok": True}


def _logits(c):
    """Unmasked, table-free logits [G, nH, n, n] in float64 (form of reference_torch)."""
    z = ao.sizes(c)
    perm = ao.torch_geometry(c)[0]
    x = c["qkv"].double()
    x = x if perm is None else x[perm.reshape(-1)]
    xw = x.reshape(z["G"], z["n"], 3, z["nH"], z["hd"]).permute(2, 0, 3, 1, 4)
    return (xw[0] * z["scale"]) @ xw[1].transpose(-2, -1)


@pytest.mark.parametrize("cid", ["w7-2x14x14x3-s3", "full-2x70x3", "w3d-2x8x8x8x3-s"])
def test_input_classes_are_what_they_claim(cid):
    z = ao.sizes(ao.SPECS[cid])
    C, hd, T = z["C"], z["hd"], z["T"]
    u = ao.case(f"{cid}/uniform")
    lim = 0.7 if u["family"] == "full" else 1.5
    assert u["qkv"].abs().max().item() <= lim and u["dout"].abs().max().item() <= 1
    assert _logits(u).std().item() < 1.0                                         # flat softmax rows
    p = ao.case(f"{cid}/peaked")
    lg = _logits(p)
    assert 8.0 < lg.std().item() < 12.0
    top = torch.softmax(lg, -1).amax(-1)
    assert top.median().item() > 0.8                                              # rows near one-hot
    zv, zd = ao.zero_channels(z)
    v, d = p["qkv"][:, 2 * C:], p["dout"]
    for t, zc in ((v, zv), (d, zd)):
        amax = t.abs().amax(0)
        assert (amax[zc] == 0).all() and len(zc) == z["nH"] and len({c // hd for c in zc}) == z["nH"]
        live = torch.ones(C, dtype=torch.bool)
        live[zc] = False
        assert amax[live].max().item() / amax[live].min().item() > 300            # three decades of channel scales
    assert (p["qkv"][[1, T - 2], :C] == 0).all() and (p["qkv"][[0, 2], :C] != 0).any()
    o = ao.case(f"{cid}/offset")
    qk = o["qkv"][:, :2 * C]
    assert 3.9 < qk.mean().item() < 4.1 and 0.9 < qk.std().item() < 1.1
    lg = _logits(o)
    want = 16 * hd * z["scale"]
    assert 0.9 * want < lg.mean().item() < 1.1 * want and lg.max().item() > want + 10
    if hd >= 32:
        assert lg.max().item() > 89                                                # exp overflows fp32 without the maximum
    for cls in ao.spec_of(f"{cid}/x")["classes"]:
        c = ao.case(f"{cid}/{cls}")
        r32 = ao.reference32(c)
        assert all(torch.isfinite(t).all() for t in r32.values()), cls            # every class stays finite in fp32
    if z["shifted"]:
        m = ao.case(f"{cid}/mask_competes")
        lg = _logits(m)
        _, _, region, codes = ao.plain_geometry(m)
        sgn = (1 - 2 * (codes % 2)).double()
        opp = (sgn[:, :, None] * sgn[:, None, :] < 0).repeat(z["B"], 1, 1).unsqueeze(1).expand_as(lg)
        gap = lg[opp].mean().item() - lg[~opp].mean().item()
        assert 95 < gap < 105, gap                                                # 100 apart before the mask, level after it


@pytest.mark.parametrize("name", [n for n in ao.names() if n.endswith(("/mask_competes", "/uniform")) and ao.sizes(ao.spec_of(n))["shifted"]])
def test_only_mask_competes_tells_the_additive_mask_from_an_exclusion(name):
    """In float64: excluding cross-region pairs instead of adding -100 changes nothing at all on the uniform class (exp(-100)
    of a flat row is below half an ulp of the sum) and more than 0.1 of a channel's largest value on mask_competes."""
    c = ao.case(name)
    r64 = ao.references(name)[0]
    hard = ao.reference_torch(c, torch.float64, hard_mask=True)
    for k in r64:
        d = ao.measure(hard[k], r64[k])["max"]
        print(name, k, d)
        if c["cls"] == "uniform":
            assert d == 0.0, (k, d)
        else:
            assert d > 0.1, (k, d)


def test_floor_constants_are_the_largest_e32_of_the_matrix():
    """FLOOR of the GPU test = the largest e32 (either measure, the larger of the two yardsticks) per kind of tensor over the
    matrix, rounded up to two digits.  Both yardsticks run on one thread, so the figures do not follow the machine's core
    count; the written constants may sit at most 10 % below / 20 % above what this machine finds."""
    import test_attention_edges_gpu as gpu
    worst = {}
    for name in ao.names():
        for k in ao.kinds_of(ao.spec_of(name)):
            for m in ao.MEASURES:
                e = ao.yardstick(name, k, m)
                if e > worst.get(k, (0.0,))[0]:
                    worst[k] = (e, name, m)
    print(worst, {k: ao.ceil2(v[0]) for k, v in worst.items()})
    assert set(worst) == set(gpu.FLOOR) == set(ao.KINDS)
    for k, (e, name, m) in worst.items():
        assert 0.8 * gpu.FLOOR[k] <= e <= 1.1 * gpu.FLOOR[k], (k, e, gpu.FLOOR[k], name, m)
    assert gpu.K == 6.0


@pytest.mark.parametrize("name", ao.names())
def test_the_two_fp32_yardsticks_are_within_three_times_of_each_other(name):
    """Every tensor, both measures, either way round; a case listed in YARD_OVER must exceed the margin where it says and holds
    everywhere else.  K of the GPU test is that margin twice."""
    import test_attention_edges_gpu as gpu
    _, ea, eb = ao.references(name)
    over = YARD_OVER.get(name, {})
    for k in ea:
        for m in ao.MEASURES:
            a, b = ea[k][m], eb[k][m]
            if a == 0.0 and b == 0.0:
                continue
            ratio = max(a, b) / min(a, b)
            print(f"{name} {k} {m}: torch fp32 {a:.2e} kernel order {b:.2e} ratio {ratio:.2f}")
            if (k, m) in over:                 # (2.2 on another CPU's BLAS: only the upper end is asserted)
                assert ratio <= 1.2 * over[(k, m)], (name, k, m, ratio)
            else:
                assert ratio <= YARD_MARGIN, (name, k, m, a, b)
    assert gpu.K == 2 * YARD_MARGIN


def test_matrix_holds_every_family_and_path():
    groups = {g for s in ao.SPECS.values() for g in s["groups"]}
    assert groups == {"win2d", "fallback", "valu", "full", "win3d"}
    for g in ("win2d", "win3d"):
        assert any(s["classes"] == ao.CLASSES and ao.sizes(s)["shifted"] for s in ao.SPECS.values() if s["groups"][0] == g), g
    assert any(s["classes"] == ao.NOMASK for s in ao.SPECS.values() if s["family"] == "full")
    assert {s["shape"][5] for s in ao.SPECS.values() if s["family"] == "win2d"} == {7, 8}
    full = [s["shape"] for s in ao.SPECS.values() if s["family"] == "full"]
    assert {sh[1] for sh in full} >= {1, 64, 65, 256} and any(sh[0] * sh[2] >= 512 for sh in full)
    assert ao.names("valu") == ["w7-23x28x28x3-s3/peaked"]
    assert ao.names("fallback") == ["w7-2x14x14x3-s3/peaked", "w8-1x16x16x3-s4/peaked"]
    assert ao.case("full-3x27x2/peaked") is ao.case("full-3x27x2/peaked")        # built once, shared
