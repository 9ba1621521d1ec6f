"""tests/norm_oracle.py checked on the CPU: the float64 closed forms against float64 autograd over torch's own ops, the two
input conditions of every generated case (kink margin, pool ties), and the FLOOR constants of
tests/test_norm_edges_gpu.py, which are the largest e32 of the matrix per kind of quantity."""
import pytest
import torch
import torch.nn.functional as F

import norm_oracle as no

# a few cases of each kind: every norm, scalar path, special channels at every ratio, residual forms, pool 2-D / 3-D, dropout
CLOSED_FORM_CASES = ["bn-S4100-N3-C5", "in-S4100-N3-C5", "in-S4100-N1-C16", "gn-S4100-N3-C16", "bn-S16388-N3-C2", "gn-S4-N1-C2",
                     "bn-S27", "in-S2", "in-S3", "none-S125", "bn-ratio32-special", "in-ratio4-special", "gn-ratio32-special",
                     "gn-ratio0-special", "bn-ratio4", "in-ratio32", "gn-ratio4",
                     "bn-momentum0.3", "bn-pre", "bn-post", "in-pre", "in-post", "bn-2x3x1x2x8-p0.3", "in-2x2x2x4x16-p0.3",
                     "bn-1x2x6x10x24-p0.0", "in-1x2x1x514x8-p0.0", "bn-S16388", "in-S1024", "gn"]


@pytest.mark.parametrize("name", CLOSED_FORM_CASES)
def test_closed_forms_equal_float64_autograd(name):
    c = no.case(name)
    r64 = no.reference64(c)
    ag = no.reference_torch(c, r64.get("codes"), torch.float64)
    assert set(ag) >= {"y", "dx"}
    for k, v in ag.items():
        assert no.rel(v, r64[k].reshape(v.shape)) <= 1e-12, (k, no.rel(v, r64[k].reshape(v.shape)))
    if c["dpool"] is not None:
        # torch's max-pool takes the first maximum too: its indices are the oracle's codes, the planted exact ties included
        y = r64["y"]
        D, H, W = y.shape[2:]
        _, ind = F.max_pool3d(y, 2, return_indices=True) if D > 1 else F.max_pool2d(y[:, :, 0], 2, return_indices=True)
        ind = ind.reshape(r64["codes"].shape)
        d, h, w = ind // (H * W), (ind // W) % H, ind % W
        assert torch.equal(((d % 2) * 4 + (h % 2) * 2 + (w % 2)).to(torch.uint8), r64["codes"])
        # and the scatter is the pool's own backward
        yy = y.clone().requires_grad_(True)
        (F.max_pool3d(yy, 2) if D > 1 else F.max_pool2d(yy[:, :, 0], 2).unsqueeze(2)).backward(c["dpool"].double())
        assert torch.equal(yy.grad, no.unpool(c["dpool"].double(), r64["codes"], y.shape))


def test_running_statistics_closed_form():
    c = no.case("bn-momentum0.3")
    r64 = no.reference64(c)
    x = c["x"].double()
    rm, rv = c["rm"].double(), c["rv"].double()
    F.batch_norm(x, rm, rv, None, None, True, no.f32(0.3), no.EPS)
    assert no.rel(rm, r64["run_mean"]) <= 1e-12 and no.rel(rv, r64["run_var"]) <= 1e-12
    assert not torch.equal(rm.float(), c["rm"]) and (c["rm"] != 0).all() and (c["rv"] != 1).all()


@pytest.mark.parametrize("per_sample", [False, True])
def test_tile_partials_add_up_to_the_statistics(per_sample):
    c = no.case("bn-np1029-N3" if not per_sample else "in-np257-ratio4")
    N, C, D, H, W = c["x"].shape
    T = no.SPECS[c["name"]]["tiles"]
    part = no.tile_partials(c["x"], T, per_sample)
    assert part.dtype == torch.float32 and tuple(part.shape) == ((N * C, T, 2) if per_sample else (C, N * T, 2))
    kind = "in" if per_sample else "bn"
    m, var, _ = no.stats64(c["x"], kind)
    E = no.group_elems(c["x"].shape, kind)
    s = part.double().sum(1)
    mean = s[:, 0] / E
    assert no.rel(mean, no.flat(m, kind)) <= 1e-6
    assert no.rel(s[:, 1] / E - mean ** 2, no.flat(var, kind)) <= 1e-6 * (1 + (m ** 2 / var).max().item())
    # the layouts: partial t of image n of channel c
    n, ch, t = N - 1, C - 1, T - 1
    tile = c["x"][n, ch].double().reshape(T, -1)[t]
    got = part[n * C + ch, t] if per_sample else part[ch, n * T + t]
    assert got[0] == tile.sum().float() and got[1] == (tile * tile).sum().float()


@pytest.mark.parametrize("name", list(no.SPECS))
def test_every_case_meets_its_input_conditions(name):
    c = no.case(name)
    n = c["x"].numel()
    assert c["nudged"] <= no.NUDGE_CAP * n, (c["nudged"], n)
    assert no.undecided(c) == 0
    assert torch.isfinite(c["x"]).all()
    spec = no.SPECS[name]
    if spec.get("special"):
        cg = c["cg"]
        assert (c["x"][:, :cg] == no.CONST).all() and c["gamma"][cg] < 0 and c["gamma"][cg + 1] == 0 and c["beta"][cg + 1] != 0
        assert (no.reference64(c)["var"].reshape(c["x"].shape[0] if c["kind"] != "bn" else 1, -1)[:, 0] == 0).all()
    if spec.get("ratio", 0) >= 4:
        r64 = no.reference64(c)
        ratio = (r64["mean"].abs() * (r64["var"] + 1e-30).rsqrt())[r64["var"] > 0]
        assert ((ratio - spec["ratio"]).abs() <= 0.1 * spec["ratio"]).all(), ratio
    if c["dpool"] is not None:
        r64 = no.references(name)[0]
        assert r64["near"].float().mean().item() <= no.TIE_CAP
        if c["slope"] == 0.0 and (c["drop_p"] > 0 or c["x"].shape[2] == 1):     # ReLU: all-zero windows are exact ties
            w = no._windows(r64["y"])
            assert ((w == 0).all(-1) & (r64["codes"] == 0)).any()


def test_floor_constants_are_the_largest_e32_of_the_matrix():
    """FLOOR_* of the GPU test = the largest e32 per kind of quantity, rounded up to two digits.  The fp32 sums of torch's
    CPU kernels depend on the thread count and the vector width in their last digits: one thread here, and the written
    constants may sit at most 10 % below / 20 % above what this machine finds."""
    import test_norm_edges_gpu as gpu
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        worst = {}
        for name in no.SPECS:
            c = no.case(name)
            r64 = no.reference64(c)
            r32 = no.reference32(c, r64.get("codes"))
            for k, v in r32.items():
                e = no.rel(v, r64[k], k in no.EACH)
                if e > worst.get(no.KIND_OF[k], (0.0,))[0]:
                    worst[no.KIND_OF[k]] = (e, name, k)
        for name, k, e in no.extra_e32():
            if e > worst[no.KIND_OF[k]][0]:
                worst[no.KIND_OF[k]] = (e, name, k)
    finally:
        torch.set_num_threads(threads)
    print(worst)
    assert set(worst) == set(gpu.FLOOR) == {"stat", "act", "dx", "sum"}
    for kind, (e, name, k) in worst.items():
        assert 0.8 * gpu.FLOOR[kind] <= e <= 1.1 * gpu.FLOOR[kind], (kind, e, gpu.FLOOR[kind], name, k)
    assert gpu.K == 6.0


def test_matrix_covers_what_the_kernels_branch_on():
    S_of = lambda n: no.case(n)["x"][0, 0].numel()
    geo = no.names("geometry")
    for kind in ("bn", "in", "gn"):
        assert {S_of(n) for n in geo if n.startswith(kind)} >= {4, 1024, 4100, 16384, 16388, 49156}
        assert {no.case(n)["x"].shape[0] for n in geo if n.startswith(kind)} == {1, 3}
    assert 524292 in {S_of(n) for n in geo}
    assert {S_of(n) for n in no.names("scalar")} == {2, 3, 6, 27, 125, 1001}
    nps = {int(n.split("np")[1].split("-")[0]) for n in no.names("finalize")}
    assert nps == {1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1029}
