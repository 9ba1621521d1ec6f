"""The Attention U-Net and its gate / up-sampling kernels, the part that needs no GPU: the float64 oracle
(tests/attention_unet_oracle.py) against the golden of the real reference (tests/golden/attention_unet_32x16x48.npz,
scripts/gen_golden_attention_unet.py), the oracle's integer up-sampling against F.interpolate and its adjoint identity, the
gate's gradient formulas against autograd, the FLOOR constants of tests/test_attention_gate_gpu.py, the state_dict surface, the
factory key and the C ABI of the new entry points."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")
for p in (PKG, ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import attention_gate_cases as ac  # noqa: E402
import attention_unet_oracle as ao  # noqa: E402

TOL = 1e-10
GOLDEN = os.path.join(ROOT, "tests", "golden", "attention_unet_32x16x48.npz")
SIZE_CAP = 400 * 1000


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def golden_sd(z, prefix="sd/"):
    return {str(k): z[prefix + str(k)] for k in z["keys"] if prefix + str(k) in z.files}


def _rel(a, b, floor=0.0):
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


def test_oracle_reproduces_the_reference(gold):
    """Train-mode logits, every parameter gradient and the running buffers, then the eval-mode logits with those buffers, all to
    1e-10 relative.  The golden holds the logits at ``logits_idx`` (the corners of every volume and a seeded draw: the full
    float64 tensors do not fit its size cap); the generator held the full tensors to the same bound before it wrote the file
    (``oracle_vs_reference_worst_rel``).  A gradient that is zero in exact arithmetic is measured against ``grad_floor``."""
    sd = golden_sd(gold)
    x, dl = gold["x"].astype(np.float64), gold["dlogits"].astype(np.float64)
    assert x.shape == (2, 1, 32, 16, 48) and dl.shape == (2, 2, 32, 16, 48)
    idx = gold["logits_idx"]
    assert len(idx) == 512 and {0, dl.size - 1} <= set(idx.tolist())
    r = ao.run(sd, x, dl, train=True)
    assert _rel(r["logits"].reshape(-1)[idx], gold["logits"]) <= TOL
    floor = float(gold["grad_floor"])
    params = [k for k in sd if ao.is_param(k)]
    assert len(sd) == 141 and len(params) == 114 and sum(sd[k].size for k in params) == 25628
    assert gold["e32"].shape == (len(params),)
    for k in params:
        assert float(np.abs(gold[f"grad/{k}"]).max()) > 0, k
        assert _rel(r["grads"][k], gold[f"grad/{k}"], floor) <= TOL, k
    buffers = [k for k in sd if not ao.is_param(k)]
    assert len(buffers) == 27 and gold["e32_after"].shape == (18,)
    for k in buffers:
        if k.endswith("num_batches_tracked"):
            assert int(r["after"][k]) == int(gold[f"after/{k}"]) == 1
        else:
            assert _rel(r["after"][k], gold[f"after/{k}"]) <= TOL, k
    sd1 = dict(sd)
    sd1.update({k: gold[f"after/{k}"] for k in buffers})
    assert _rel(ao.run(sd1, x, train=False)["logits"].reshape(-1)[idx], gold["eval_logits"]) <= TOL
    assert float(gold["oracle_vs_reference_worst_rel"]) <= TOL


def test_golden_is_under_its_size_cap_and_holds_data_only(gold):
    assert os.path.getsize(GOLDEN) < SIZE_CAP, os.path.getsize(GOLDEN)
    assert all(gold[k].dtype.kind in "fiU" for k in gold.files)
    assert gold["x"].dtype == gold["dlogits"].dtype == np.float16 and gold["logits"].dtype == np.float64


@pytest.mark.parametrize("s", [2, 4, 8])
@pytest.mark.parametrize("grid", [(1, 1, 1), (2, 1, 3), (1, 4, 1), (4, 2, 6), (3, 5, 7)])
def test_integer_upsampling_is_torchs_trilinear_and_its_adjoint_is_exact(s, grid):
    g = torch.Generator().manual_seed(s * 100 + sum(grid))
    a = torch.randn((2, 3) + grid, generator=g, dtype=torch.float64)
    b = torch.randn((2, 3) + tuple(s * n for n in grid), generator=g, dtype=torch.float64)
    up = ao.upsample_int(a, s)
    assert float((up - F.interpolate(a, scale_factor=s, mode="trilinear", align_corners=False)).abs().max()) <= 1e-14
    lhs, rhs = float((up * b).sum()), float((a * ao.upsample_int_adjoint(b, s)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (lhs, rhs)
    m = ao.up_matrix(grid[2], s)
    assert float((m.sum(1) - 1).abs().max()) <= 1e-15 and int((m != 0).sum(1).max()) <= 2     # s fixed weight pairs per axis
    if grid == (1, 1, 1):
        assert torch.equal(up, a.expand_as(up))               # an extent of 1 replicates


def test_two_x2_passes_are_not_one_x4_pass():
    a = torch.arange(4.0, dtype=torch.float64).reshape(1, 1, 1, 1, 4) ** 2
    assert float((ao.upsample_int(ao.upsample_int(a, 2), 2) - ao.upsample_int(a, 4)).abs().max()) > 1e-2


def test_gate_gradient_formulas_are_autograds():
    for ci, grid in [(3, (2, 1, 3)), (32, (3, 5, 7))]:
        c = ac.map_case(ci, grid)
        i = {k: v.clone().requires_grad_(True) for k, v in c["in"].items() if k in ("theta", "phi", "psi_w", "psi_b")}
        got = torch.autograd.grad(ao.gate_map(i["theta"], i["phi"], i["psi_w"], i["psi_b"]),
                                  [i["theta"], i["phi"], i["psi_w"], i["psi_b"]], c["in"]["datt"])
        for g, want in zip(got, (c["df"], c["df"], c["dpsi_w"], c["dpsi_b"])):
            assert _rel(g, want) <= 1e-13
    for ch, grid in [(5, (2, 1, 3)), (1, (1, 1, 1))]:
        c = ac.apply_case(ch, grid)
        x, att = (c["in"][k].clone().requires_grad_(True) for k in ("x", "att"))
        gx, ga = torch.autograd.grad(ao.gate_apply(x, att), [x, att], c["in"]["dy"])
        assert _rel(gx, c["dx"]) <= 1e-13 and _rel(ga, c["datt"]) <= 1e-13
        # the reference's expression: the map up-sampled to x's size, expanded over the channels
        up = F.interpolate(c["in"]["att"], size=x.shape[2:], mode="trilinear", align_corners=False)
        want = torch.cat([up[:, g:g + 1].expand_as(x) * x for g in range(2)], 1)
        assert _rel(c["y"], want.detach()) <= 1e-14


def test_case_matrix_is_the_issues_and_keeps_its_input_conditions():
    assert sorted({ci for ci, _ in ac.MAP_CASES}) == [1, 3, 4, 32, 128] and (4, (24, 24, 24)) in ac.MAP_CASES
    assert {g for ci, g in ac.MAP_CASES if ci != 4} == {(1, 1, 1), (2, 1, 3), (3, 5, 7)}
    assert {c for c, _ in ac.APPLY_CASES} == {1, 5, 32} and {g for _, g in ac.APPLY_CASES} == {(1, 1, 1), (2, 1, 3), (3, 5, 8)}
    assert {(s, k) for s, k, _ in ac.UP_CASES} == {(s, k) for s in (2, 4, 8) for k in (2, 4)}
    assert {g for _, _, g in ac.UP_CASES} == {(1, 1, 1), (2, 1, 3), (4, 2, 6)}
    assert ac.N == 2 and ac.G == 2
    c = ac.map_case(128, (3, 5, 7))         # map_case itself asserts the kink margin and the +-8 bound of every case
    f = (c["in"]["theta"] + c["in"]["phi"])
    assert float(f.abs().min()) >= ac.MARGIN and torch.equal(f.float().double(), f)      # exact in fp32
    assert 0 < float((f > 0).double().mean()) < 1


def test_floor_constants_are_the_largest_e32_of_the_matrix():
    """FLOOR of the GPU kernel test = the largest e32 per kind of quantity over the matrix, rounded up to two digits.  The fp32
    sums of torch's CPU kernels depend on the thread count and the vector width in their last digits: one thread here, and the
    written constants may sit at most 10 % below / 20 % above what this machine finds (tests/test_norm_oracle_cpu.py)."""
    import test_attention_gate_gpu as gpu
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        worst = ac.floors()
    finally:
        torch.set_num_threads(threads)
    print(worst)
    assert set(worst) == set(gpu.FLOOR) == set(ac.KIND_OF.values())
    for kind, (e, label, out) in worst.items():
        assert 0.8 * gpu.FLOOR[kind] <= e <= 1.1 * gpu.FLOOR[kind], (kind, e, gpu.FLOOR[kind], label, out)
    import test_norm_edges_gpu as ne
    assert gpu.K == ne.K == 6.0


def test_state_dict_surface_matches_the_reference(gold):
    from networks.attention_unet import Attention_UNet
    spec = Attention_UNet.spec(64, 2, 1)
    assert [n for n, _ in spec] == [str(k) for k in gold["keys"]] and len(spec) == 141
    for n, shape in spec:
        assert tuple(gold[f"sd/{n}"].shape) == tuple(shape), n
    wide = dict(Attention_UNet.spec(4, 2, 1))
    assert wide["conv1.conv1.0.weight"] == (16, 1, 3, 3, 3) and wide["center.conv2.0.weight"] == (256, 256, 3, 3, 3)
    assert wide["attentionblock2.gate_block_1.theta.weight"] == (32, 32, 2, 2, 2)
    assert "attentionblock2.gate_block_1.theta.bias" not in wide
    assert wide["attentionblock4.gate_block_2.phi.weight"] == (128, 256, 1, 1, 1)
    assert wide["attentionblock3.gate_block_1.psi.weight"] == (1, 64, 1, 1, 1)
    assert wide["attentionblock3.combine_gates.0.weight"] == (64, 128, 1, 1, 1)
    assert wide["dsv4.dsv.0.weight"] == (2, 128, 1, 1, 1) and wide["final.weight"] == (2, 8, 1, 1, 1)


def test_net_factory_3d_serves_attention_unet():
    import networks.net_factory_3d as nf
    assert "attention_unet" not in nf._OUT_OF_SCOPE and "voxresnet" in nf._OUT_OF_SCOPE and "nnUNet" in nf._OUT_OF_SCOPE
    with pytest.raises(NotImplementedError):
        nf.net_factory_3d("voxresnet", 1, 2)
    if not torch.cuda.is_available():      # with a device the factory builds the network: tests/test_attention_unet_gpu.py
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            nf.net_factory_3d("attention_unet", 1, 2)
    from networks.attention_unet import Attention_UNet
    for kw in (dict(nonlocal_mode="concatenation_debug"), dict(attention_dsample=(1, 1, 1)), dict(is_batchnorm=False)):
        with pytest.raises(NotImplementedError):
            Attention_UNet(n_classes=2, in_channels=1, **kw)


def test_c_abi_is_declared_and_refuses_bad_arguments_before_launch():
    from mis_hip import lib
    header = open(os.path.join(ROOT, "include", "mis_hip_attention_gate.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    declared = set(re.findall(r"\b(mis_\w+)\s*\(", code))
    names = {"mis_attn_gate_map_fwd", "mis_attn_gate_map_bwd", "mis_attn_gate_map_bwd_workspace_bytes", "mis_attn_gate_apply_fwd",
             "mis_attn_gate_apply_bwd", "mis_attn_gate_apply_bwd_workspace_bytes", "mis_upsample_int_fwd", "mis_upsample_int_bwd"}
    assert "mis_hip_attention_gate.h" in lib.EXTRA_HEADERS
    protos = lib.EXTRA_PROTOTYPES["mis_hip_attention_gate.h"]
    assert declared == names == set(protos) and not names & set(lib.PROTOTYPES)
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert protos["mis_attn_gate_map_fwd"] == (I, [P, LL, P, LL, P, P, P, LL, I, I, I, I, I, I, P])
    assert protos["mis_attn_gate_apply_fwd"] == (I, [P, LL, P, LL, P, LL] + [I] * 9 + [P])
    assert protos["mis_attn_gate_apply_bwd_workspace_bytes"] == (LL, [I] * 5)
    assert protos["mis_attn_gate_apply_bwd"] == (I, [P, LL, P, LL, P, LL, P, LL, P, LL, P, LL] + [I] * 10 + [P])
    assert protos["mis_attn_gate_map_bwd_workspace_bytes"] == (LL, [I] * 6)
    assert protos["mis_attn_gate_map_bwd"] == (I, [P, LL, P, LL, P, LL, P, LL, P, P, LL, P, P, P, P, LL] + [I] * 7 + [P])
    assert protos["mis_upsample_int_fwd"] == (I, [P, LL, P, LL, I, I, I, I, I, I, P])
    assert protos["mis_upsample_int_bwd"] == (I, [P, LL, P, LL, I, I, I, I, I, I, I, P])
    L = lib.load()
    for n in names:
        assert hasattr(L, n), n                       # the built library exports each of them
    # the workspace queries: sizes from the shapes, refusals as negative codes (no device needed)
    assert L.mis_attn_gate_apply_bwd_workspace_bytes(8, 2, 48, 48, 48) == 8 * 2 * 48 ** 3 * 4
    assert L.mis_attn_gate_apply_bwd_workspace_bytes(8, 2, 47, 48, 48) == -2
    assert L.mis_attn_gate_apply_bwd_workspace_bytes(8, 5, 48, 48, 48) == -2
    assert L.mis_attn_gate_apply_bwd_workspace_bytes(0, 2, 48, 48, 48) == -1
    assert L.mis_attn_gate_map_bwd_workspace_bytes(2, 2, 4, 24, 24, 24) == (2 * 4 + 2) * 14 * 8      # 27 648 pairs in 14 chunks
    assert L.mis_attn_gate_map_bwd_workspace_bytes(2, 2, 0, 24, 24, 24) == -1
    # refused before anything is touched: null pointers and non-positive sizes
    assert L.mis_attn_gate_map_fwd(None, 0, None, 0, None, None, None, 0, 2, 2, 4, 2, 2, 2, None) == -1
    assert L.mis_attn_gate_apply_fwd(None, 0, None, 0, None, 0, 2, 2, 4, 4, 4, 4, 2, 2, 2, None) == -1
    assert L.mis_upsample_int_fwd(None, 0, None, 0, 2, 2, 2, 2, 2, 4, None) == -1
    assert L.mis_upsample_int_bwd(None, 0, None, 0, 2, 2, 2, 2, 2, 4, 0, None) == -1
