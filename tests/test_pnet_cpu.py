"""PNet2D and the dilated convolution, the part that needs no GPU: the float64 net oracle (tests/pnet_oracle.py) against the
golden of the real reference (tests/golden/pnet_40x24.npz, scripts/gen_golden_pnet.py), the two float64 forms of the op oracle
(tests/dilated_oracle.py) against each other, the FLOOR constants of the GPU gate, the network's state_dict surface, the
factory key and the C ABI of the new entry points."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cv-ssl-mis_amd")
for p in (PKG, ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_oracle as co  # noqa: E402
import dilated_oracle as do  # noqa: E402
import pnet_oracle as po  # noqa: E402

TOL = 1e-10


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "pnet_40x24.npz"))


def golden_sd(z, prefix="sd/"):
    return {str(k): z[prefix + str(k)] for k in z["keys"] if prefix + str(k) in z.files}


def _rel(a, b, floor=0.0):
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


def test_oracle_reproduces_the_reference(gold):
    """Train-mode logits, every parameter gradient and the running buffers, then the eval-mode logits with those buffers, all to
    1e-10 relative.  A gradient that is zero in exact arithmetic (the bias of a convolution in front of a BatchNorm: 1e-16 of
    rounding noise in the reference's float64) has no scale of its own and is measured against the golden's ``grad_floor``,
    1e-4 of the net's largest gradient."""
    sd = golden_sd(gold)
    x, dl = gold["x"].astype(np.float64), gold["dlogits"].astype(np.float64)
    r = po.run(sd, x, dl, train=True)
    assert _rel(r["logits"], gold["logits"]) <= TOL
    floor = float(gold["grad_floor"])
    params = [k for k in sd if po.is_param(k)]
    assert len(params) == 48 and sum(sd[k].size for k in params) == 7964
    for k in params:
        assert _rel(r["grads"][k], gold[f"grad/{k}"], floor) <= TOL, k
    buffers = [k for k in sd if not po.is_param(k)]
    assert len(buffers) == 30
    for k in buffers:
        if k.endswith("num_batches_tracked"):
            assert int(r["after"][k]) == int(gold[f"after/{k}"]) == 1
        else:
            assert _rel(r["after"][k], gold[f"after/{k}"]) <= TOL, k
    sd1 = dict(sd)
    sd1.update({k: gold[f"after/{k}"] for k in buffers})
    assert _rel(po.run(sd1, x, train=False)["logits"], gold["eval_logits"]) <= TOL
    assert float(gold["oracle_vs_reference_worst_rel"]) <= TOL


def test_oracle_dropout_masks_scale_whole_feature_maps(gold):
    """An all-ones mask pair is the p = 0 forward; zeroing one channel of drop2's mask equals zeroing that column of out.conv2."""
    sd = golden_sd(gold)
    x = gold["x"].astype(np.float64)
    N = x.shape[0]
    ones = (np.ones((N, 16, 1, 1)), np.ones((N, 8, 1, 1)))
    base = po.run(sd, x, train=True)["logits"]
    assert torch.equal(po.run(sd, x, train=True, masks=ones)["logits"], base)
    m2 = ones[1].copy()
    m2[:, 3] = 0.0
    sd2 = dict(sd)
    w = sd["out.conv2.weight"].copy()
    w[:, 3] = 0.0
    sd2["out.conv2.weight"] = w
    assert _rel(po.run(sd, x, train=True, masks=(ones[0], m2))["logits"], po.run(sd2, x, train=True)["logits"]) <= 1e-14


@pytest.mark.parametrize("name", do.names())
def test_plain_tap_sum_equals_torch_dilated_convolution(name):
    c = do.case(name)
    r64, p64 = do.references(name)[0], do.plain64(c)
    for k in do.KINDS:
        assert _rel(p64[k], r64[k]) <= 1e-12, (name, k)


def test_matrix_covers_what_the_issue_lists():
    want = {"even-d2": ((2, 16, 32, 1, 32, 32), 2, 1), "ragged-d4": ((1, 10, 20, 1, 37, 50), 4, 3),
            "small-phase-d8": ((1, 64, 64, 1, 56, 56), 8, 1), "few-px-d16": ((2, 64, 64, 1, 32, 48), 16, 3),
            "below-d-d16": ((1, 8, 8, 1, 8, 24), 16, 1), "odd-d16": ((3, 8, 8, 1, 40, 24), 16, 1),
            "slices-d4": ((2, 16, 16, 1, 24, 40), 4, 1)}
    for cid, (shape, d, nclasses) in want.items():
        s = do.SPECS[cid]
        assert (s["shape"], s["dil"], len(s["classes"])) == (shape, d, nclasses), cid
        assert s["classes"][0] == "relu_scaled"
    assert do.SPECS["slices-d4"]["layout"] == "slice"
    assert set(do.SPECS["ragged-d4"]["classes"]) == set(do.SPECS["few-px-d16"]["classes"]) == {"relu_scaled", "uniform", "offset"}


def test_floor_constants_are_the_largest_e32_of_the_matrix():
    """FLOOR = the largest e32 (either measure) per kind of tensor over the matrix, rounded up to two digits with
    conv_oracle.ceil2.  reference32 runs on one thread; as in tests/test_conv_oracle_cpu.py the written constants may sit at
    most 10 % below / 20 % above what this machine finds."""
    worst = {}
    for name in do.names():
        e32 = do.references(name)[2]
        for k in do.KINDS:
            for m in do.MEASURES:
                if e32[k][m] > worst.get(k, (0.0,))[0]:
                    worst[k] = (e32[k][m], name, m)
    print(worst, {k: co.ceil2(v[0]) for k, v in worst.items()})
    assert set(worst) == set(do.FLOOR) == set(do.KINDS)
    for k, (e, name, m) in worst.items():
        assert 0.8 * do.FLOOR[k] <= e <= 1.1 * do.FLOOR[k], (k, e, do.FLOOR[k], name, m)
        assert do.FLOOR[k] == co.ceil2(do.FLOOR[k])
    assert do.K == 6.0


def test_state_dict_surface_matches_the_reference(gold):
    from networks.pnet import PNet2D
    spec = PNet2D.spec(1, 4, 8, [1, 2, 4, 8, 16])
    assert [n for n, _ in spec] == [str(k) for k in gold["keys"]]
    for n, shape in spec:
        assert tuple(gold[f"sd/{n}"].shape) == tuple(shape), n
    wide = dict(PNet2D.spec(1, 4, 64))
    assert wide["block1.conv1.weight"] == (64, 1, 3, 3) and wide["block5.conv2.weight"] == (64, 64, 3, 3)
    assert wide["catblock.conv1.weight"] == (320, 320, 1, 1) and wide["catblock.conv2.weight"] == (128, 320, 1, 1)
    assert wide["out.conv1.weight"] == (64, 128, 1, 1) and wide["out.conv2.weight"] == (4, 64, 1, 1)


def test_net_factory_serves_pnet():
    import networks.net_factory as nf
    assert "pnet" not in nf._OUT_OF_SCOPE and "unet_cct" in nf._OUT_OF_SCOPE
    with pytest.raises(NotImplementedError):
        nf.net_factory("unet_cct", 1, 4)
    if not torch.cuda.is_available():      # with a device the factory builds the network: tests/test_pnet_gpu.py
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            nf.net_factory("pnet", 1, 4)


def test_c_abi_is_declared_and_refuses_bad_arguments_before_launch():
    from mis_hip import lib
    header = open(os.path.join(ROOT, "include", "mis_hip_dilated.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    declared = set(re.findall(r"\b(mis_\w+)\s*\(", code))
    names = {"mis_conv_dilated_fwd", "mis_conv_dilated_dgrad", "mis_conv_dilated_wgrad", "mis_conv_dilated_wgrad_workspace_bytes",
             "mis_conv_dilated_fwd_kernel_name", "mis_conv_dilated_dgrad_kernel_name", "mis_conv_dilated_wgrad_kernel_name"}
    assert "mis_hip_dilated.h" in lib.EXTRA_HEADERS
    protos = lib.EXTRA_PROTOTYPES["mis_hip_dilated.h"]
    assert declared == names == set(protos) and not names & set(lib.PROTOTYPES)
    P, I, LL, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_char_p
    assert protos["mis_conv_dilated_fwd"] == (I, [P, LL, P, P, P, LL, I, I, I, I, I, I, P])
    assert protos["mis_conv_dilated_dgrad"] == (I, [P, LL, P, P, LL, I, I, I, I, I, I, P])
    assert protos["mis_conv_dilated_wgrad"] == (I, [P, LL, P, LL, P, P, LL, I, I, I, I, I, I, I, P])
    assert protos["mis_conv_dilated_wgrad_workspace_bytes"] == (LL, [I, I, I, I, I, I])
    assert protos["mis_conv_dilated_fwd_kernel_name"] == (I, [I, I, I, I, I, I, S, I])
    L = lib.load()
    for n in names:
        assert hasattr(L, n), n                       # the built library exports each of them
    buf = ctypes.create_string_buffer(128)
    assert L.mis_conv_dilated_fwd_kernel_name(24, 64, 64, 256, 256, 16, buf, 128) == 0
    assert buf.value.decode() == "conv_dilated_fwd_kernel<DCfg<16, 16, 32, 32, 4, 8>>"
    assert L.mis_conv_dilated_wgrad_kernel_name(24, 64, 64, 256, 256, 2, buf, 128) == 0
    assert buf.value.decode() == "conv_dilated_wgrad_kernel<DWCfg<2, 8, 32>>"
    assert L.mis_conv_dilated_wgrad_workspace_bytes(24, 64, 64, 256, 256, 8) > 0
    # refused before anything is touched (no device needed to see that): null pointers, sizes, dilations and images the
    # kernels do not serve
    assert L.mis_conv_dilated_fwd(None, 0, None, None, None, 0, 1, 8, 8, 16, 16, 2, None) == -1
    assert L.mis_conv_dilated_dgrad(None, 0, None, None, 0, 1, 8, 8, 16, 16, 2, None) == -1
    assert L.mis_conv_dilated_wgrad(None, 0, None, 0, None, None, 0, 1, 8, 8, 16, 16, 2, 0, None) == -1
    assert L.mis_conv_dilated_wgrad_workspace_bytes(0, 8, 8, 16, 16, 2) == -1
    for d in (1, 3, 32):
        assert L.mis_conv_dilated_wgrad_workspace_bytes(1, 8, 8, 16, 16, d) == -2
        assert L.mis_conv_dilated_fwd_kernel_name(1, 8, 8, 16, 16, d, buf, 128) == -2
    assert L.mis_conv_dilated_wgrad_workspace_bytes(1, 64, 64, 16384, 16384, 2) == -2
    assert L.mis_conv_dilated_fwd_kernel_name(1, 64, 64, 16384, 16384, 2, buf, 128) == -2
