"""What of the 2-D adversarial feature can be held without a GPU: the C ABI (header, exports, refusals before any launch), the
float64 oracle of tests/adversarial2d_oracle.py against the REAL reference discriminator (tests/golden/adversarial_2d.npz,
scripts/gen_golden_adversarial2d.py) and against itself (convolution operator vs a plain sum over the taps), the constants the
GPU tests take from it (FLOOR, the undecided share of every chain input), the discriminator's state_dict, the stub that stays
in networks.discriminator, and both command lines."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adversarial2d_oracle as ao
import conv_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "adversarial_2d.npz")
NAMES = {"mis_conv2d_k4s2_fwd_workspace_bytes", "mis_conv2d_k4s2_fwd", "mis_conv2d_k4s2_dgrad",
         "mis_conv2d_k4s2_wgrad_workspace_bytes", "mis_conv2d_k4s2_wgrad", "mis_adv_head2d_workspace_bytes",
         "mis_adv_head2d_fwd", "mis_adv_head2d_bwd"}


def test_header_parses_and_every_exported_symbol_is_declared():
    from mis_hip import lib
    header = open(os.path.join(ROOT, "include", "mis_hip_adversarial2d.h")).read()
    declared = set(re.findall(r"\b(mis_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    assert "mis_hip_adversarial2d.h" in lib.EXTRA_HEADERS
    protos = lib.EXTRA_PROTOTYPES["mis_hip_adversarial2d.h"]
    assert declared == NAMES == set(protos) == set(lib.parse_header(header)) and not NAMES & set(lib.PROTOTYPES)
    source = open(os.path.join(ROOT, "cv-ssl-mis_amd", "csrc", "adversarial2d.hip")).read()
    defined = set(re.findall(r'^extern "C" [\w \*]+?\b(mis_\w+)\s*\(', source, flags=re.M))
    assert defined == NAMES, (defined ^ NAMES)
    make = open(os.path.join(ROOT, "cv-ssl-mis_amd", "csrc", "Makefile")).read()
    assert "adversarial2d.hip" in make and "adversarial2d.o: ../../include/mis_hip_adversarial2d.h" in make
    P, I, LL, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    assert protos["mis_conv2d_k4s2_fwd"] == (I, [P, LL, I, P, LL, I, P, P, P, P, P, LL, I, I, I, I, F, P, P, LL, P])
    assert protos["mis_conv2d_k4s2_dgrad"] == (I, [P, LL, P, LL, F, P, P, P, LL, I, I, I, I, I, P])
    assert protos["mis_adv_head2d_fwd"] == (I, [P, LL, P, P, P, P, P, I, I, I, I, I, I, I, P, LL, P])
    L = lib.load()
    for n in NAMES:
        assert hasattr(L, n), n
    # the 3-D head is untouched: it still refuses every window but the whole feature
    p = ctypes.c_void_p(0x1000)
    assert L.mis_adv_head_fwd(p, 64 * 4, p, p, p, p, p, 1, 64, 2, 1, 2, 2, 1, 1, 1, p, 1 << 20, None) == -2


def test_entry_points_refuse_bad_arguments_before_launching():
    """NULL pointers, extents <= 0, odd extents, Cl > 4, short workspaces, a head geometry that leaves no window: the status
    comes back from the argument checks (no device is needed; the non-NULL pointers below are never dereferenced)."""
    from mis_hip import lib
    L = lib.load()
    p = ctypes.c_void_p(0x1000)
    ARG, UNS, WS = -1, -2, -4
    S, So = 6 * 10, 3 * 5

    def fwd(x=p, w=p, y=p, N=1, Cout=8, H=6, W=10, slope=0.2, ws=p, wsb=1 << 30, Cx=3, xbs=3 * S):
        return L.mis_conv2d_k4s2_fwd(x, xbs, Cx, None, 0, 0, w, None, None, None, y, Cout * (H // 2) * (W // 2), N, Cout, H, W,
                                     slope, None, ws, wsb, None)

    def dgrad(dy=p, w=p, dx=p, N=1, Cin=3, Cout=8, H=6, W=10):
        return L.mis_conv2d_k4s2_dgrad(dy, Cout * So, None, 0, 0.2, None, w, dx, Cin * S, N, Cin, Cout, H, W, None)

    def wgrad(x=p, dy=p, dw=p, N=1, Cout=8, H=6, W=10, ws=p, wsb=1 << 30):
        return L.mis_conv2d_k4s2_wgrad(x, 3 * S, 3, None, 0, 0, dy, Cout * So, None, 0, 0.2, None, dw, None, None, None, N, Cout,
                                       H, W, 0, ws, wsb, None)
    for call in (fwd, dgrad, wgrad):
        for kw in (dict(N=0), dict(Cout=0), dict(H=-2), dict(W=0)):
            assert call(**kw) == ARG, (call.__name__, kw)
        for kw in (dict(H=7), dict(W=1), dict(H=3, W=3)):
            assert call(**kw) == UNS, (call.__name__, kw)
    assert fwd(x=None) == ARG and fwd(w=None) == ARG and fwd(y=None) == ARG and fwd(slope=0.0) == ARG and fwd(xbs=S) == ARG
    assert dgrad(dy=None) == ARG and dgrad(w=None) == ARG and dgrad(dx=None) == ARG and dgrad(Cin=0) == ARG
    assert wgrad(x=None) == ARG and wgrad(dy=None) == ARG and wgrad(dw=None) == ARG
    # five softmax-read channels
    assert L.mis_conv2d_k4s2_fwd(p, 5 * S, 0, p, 5 * S, 5, None, p, None, None, p, 8 * So, 1, 8, 6, 10, 0.2, None, p, 1 << 30,
                                 None) == UNS
    # the workspace queries agree with the entry points: a sliced forward and every weight gradient refuse a short one
    need = L.mis_conv2d_k4s2_fwd_workspace_bytes(2, 256, 64, 8, 8)
    assert need > 0 and L.mis_conv2d_k4s2_fwd_workspace_bytes(24, 5, 64, 256, 256) == 0
    big = dict(N=2, Cout=64, H=8, W=8, Cx=256, xbs=256 * 64)
    assert fwd(**big, wsb=need - 1) == WS and fwd(**big, ws=None, wsb=need) == WS
    need = L.mis_conv2d_k4s2_wgrad_workspace_bytes(1, 3, 8, 6, 10)
    assert need > 0 and wgrad(wsb=need - 1) == WS and wgrad(ws=None) == WS
    for q in (L.mis_conv2d_k4s2_fwd_workspace_bytes, L.mis_conv2d_k4s2_wgrad_workspace_bytes):
        assert q(0, 3, 8, 6, 10) == ARG and q(1, 0, 8, 6, 10) == ARG and q(1, 3, 8, 5, 10) == UNS
    # head: 512 channels of 16 x 16 under AvgPool2d((7, 7)) -> 2 x 2 windows -> 2048 features
    hb = L.mis_adv_head2d_workspace_bytes(4, 512, 2, 16, 16, 7, 7)
    assert hb == (4 * 2048 + 4 * 2 + 4) * 4 and L.mis_adv_head2d_workspace_bytes(4, 512, 2, 14, 14, 7, 7) == hb
    assert L.mis_adv_head2d_workspace_bytes(0, 512, 2, 16, 16, 7, 7) == ARG
    assert L.mis_adv_head2d_workspace_bytes(4, 512, 2, 16, 16, 0, 7) == ARG
    assert L.mis_adv_head2d_workspace_bytes(4, 512, 2, 6, 16, 7, 7) == UNS          # no window fits 6 rows

    def head(a=p, N=4, ext=(16, 16), pool=(7, 7), wsb=hb, K=2):
        return L.mis_adv_head2d_fwd(a, 512 * ext[0] * ext[1], p, p, p, p, p, N, 512, K, *ext, *pool, p, wsb, None)
    assert head(a=None) == ARG and head(N=0) == ARG and head(pool=(0, 7)) == ARG
    assert head(ext=(16, 6)) == UNS and head(K=9) == UNS and head(wsb=hb - 1) == WS
    assert L.mis_adv_head2d_bwd(None, p, 512 * 256, p, p, 0, 4, 512, 2, 16, 16, 7, 7, p, hb, None) == ARG
    assert L.mis_adv_head2d_bwd(p, p, 512 * 256, p, p, 0, 4, 512, 2, 16, 16, 7, 7, p, hb - 1, None) == WS
    assert L.mis_adv_head2d_bwd(p, p, 512 * 256, p, p, 0, 4, 512, 2, 16, 16, 17, 7, p, hb, None) == UNS


def test_discriminator_spec_stub_and_command_lines_are_the_references():
    from networks.discriminator import FCDiscriminator as Stub
    from networks.discriminator_2d import FCDiscriminator
    spec = FCDiscriminator.spec(4)
    assert [k for k, _ in spec] == list(ao.DISC_KEYS) and dict(spec) == ao.disc_shapes(4, 64, 1)
    assert dict(FCDiscriminator.spec(3, ndf=8, n_channel=2))["conv1.weight"] == (8, 2, 4, 4)
    assert dict(spec)["conv4.weight"] == (512, 256, 4, 4) and dict(spec)["classifier.weight"] == (2, 2048)
    assert FCDiscriminator.ndim_spatial == 2
    with pytest.raises(NotImplementedError, match="networks.discriminator_2d"):
        Stub(4)
    common = dict(root_path='../data/ACDC', model='unet', max_iterations=30000, batch_size=24, deterministic=1, base_lr=0.01,
                  DAN_lr=0.0001, seed=1337, num_classes=4, labeled_bs=12, ema_decay=0.99, consistency_type="mse",
                  consistency=0.1, consistency_rampup=200.0)
    import train_adversarial_network_2D as t
    assert vars(t.parser.parse_args([])) == dict(common, exp='ACDC/Adversarial_Network', patch_size=[256, 256], labeled_num=3)
    assert t.parser.parse_args(["--patch_size", "224", "224"]).patch_size == [224, 224]
    import train_adversarial_network_2D_ViT as tv
    swin = {"cfg": "../code/configs/swin_tiny_patch4_window7_224_lite.yaml", "opts": None, "zip": False, "cache_mode": "part",
            "resume": None, "accumulation_steps": None, "use_checkpoint": False, "amp_opt_level": "O1", "tag": None,
            "eval": False, "throughput": False}
    assert vars(tv.parser.parse_args([])) == dict(common, **swin, exp='ACDC/Adversarial_Network_ViT', patch_size=[224, 224],
                                                  labeled_num=7)
    from mis_hip import ops
    for name in ("conv2d_k4s2_fwd", "conv2d_k4s2_dgrad", "conv2d_k4s2_wgrad", "adv_head2d_fwd", "adv_head2d_bwd",
                 "adv_head2d_workspace"):
        assert callable(getattr(ops, name)), name


def test_plain_sum_over_the_taps_agrees_with_the_convolution_operator():
    for name in ("all-padding/offset", "ragged-20x12/uniform", "row/relu_scaled", "col/relu_scaled", "views/relu_scaled"):
        c = ao.case(name)
        plain, r64 = ao.plain64(c), ao.references(name)[0]
        taps = ao.reference_torch(c, torch.float64, ao.conv_taps)
        for k in ao.KINDS:
            for other in (plain[k], taps[k]):
                assert (other - r64[k]).abs().max().item() <= 3e-15 * max(r64[k].abs().max().item(), 1.0), (name, k)
    # the same through the whole discriminator: disc_forward on a convolution that uses no convolution operator
    sd = {k: v.double() for k, v in ao.golden_state_dict(4, 2, 1).items()}
    g = torch.Generator().manual_seed(5)
    probs = torch.softmax(torch.randn(2, 4, 32, 80, generator=g, dtype=torch.float64), 1)
    img = torch.randn(2, 1, 32, 80, generator=g, dtype=torch.float64)
    a = ao.disc_forward(sd, probs, img, pool=(1, 2))[0]
    b = ao.disc_forward(sd, probs, img, pool=(1, 2), conv_fn=ao.conv_taps)[0]
    assert a.shape == (2, 2) and (a - b).abs().max().item() <= 1e-14


def test_floor_is_the_largest_e32_of_the_matrix_and_the_margin_leaves_few_decisions_out():
    worst = {k: 0.0 for k in ao.KINDS}
    for name in ao.names():
        _, _, e32 = ao.references(name)
        for k in ao.KINDS:
            worst[k] = max(worst[k], max(e32[k][m] for m in ao.MEASURES))
    assert {k: co.ceil2(v) for k, v in worst.items()} == ao.FLOOR, worst
    # the epilogue cases of tests/test_adversarial2d_kernels_gpu.py: the oracle's own undecided share stays under the cap
    for name in ("ragged-20x12/uniform", "c20-64/relu_scaled", "tiles-vec/relu_scaled", "sliced/uniform"):
        assert ao.undecided_share(ao.references(name)[0]["y"]) <= ao.UNDECIDED_CAP, name


@pytest.mark.parametrize("name", list(ao.CHAINS))
@pytest.mark.parametrize("law", ["uniform", "sine"])
def test_every_chain_input_keeps_the_undecided_share_under_the_cap(name, law):
    """A condition of the chain tests, not a measurement: in float64, at every activated layer, at most UNDECIDED_CAP of the
    pre-activations lie inside the margin -- under the parameters the GPU test uses and under the other law as well."""
    img, lg, sd, masks, target, pool = ao.chain_inputs(name, law)
    probs = torch.softmax(lg.double(), 1)
    _, _, pres = ao.disc_forward({k: v.double() for k, v in sd.items()}, probs, img.double(), masks, pool)
    for i in ao.ACTIVATED:
        assert ao.undecided_share(pres[i]) <= ao.UNDECIDED_CAP, (name, law, i, ao.undecided_share(pres[i]))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def golden_runs():
    """The oracle on the golden's closed-form inputs: phase A, phase B and the two Adam steps.  Computed once."""
    img, logits, _ = ao.golden_inputs(4, 4, 256, 224)
    sd0 = ao.golden_state_dict(4, 4, 1)
    masks = ao.golden_masks(4, 4)
    probs = torch.softmax(logits.double(), 1)
    target = torch.tensor([1, 1, 0, 0])
    ra = ao.disc_step(sd0, probs[2:], img[2:], target[:2], None)
    rb = ao.disc_step(sd0, probs, img, target, masks)
    sd1 = {k: ao.adam(sd0[k], [rb["grads"][k]], 1e-4)[0] for k in sd0}
    rb2 = ao.disc_step(sd1, probs, img, target, masks)
    return sd0, ra, rb, sd1, rb2


def test_oracle_reproduces_the_reference_iteration(golden, golden_runs):
    sd0, ra, rb, sd1, rb2 = golden_runs
    assert float(golden["oracle_vs_reference_worst_rel"]) <= 1e-10
    assert os.path.getsize(GOLDEN) <= 548021            # no larger than tests/golden/adversarial_3d.npz

    def rel(a, b):
        b = torch.from_numpy(np.asarray(b)).double()
        return ((torch.as_tensor(a).double().reshape(b.shape) - b).abs().max() / b.abs().max()).item()
    # conv4 leaves 16 x 14: one axis pools with a dropped remainder, the other exactly
    assert tuple(ra["acts"][3].shape[2:]) == (16, 14)
    assert rel(ra["logits"], golden["a_logits"]) <= 1e-11 and rel(ra["loss"], golden["a_loss"]) <= 1e-12
    assert rel(ao.lattice(ra["dmap"]), golden["dmap_lattice"]) <= 1e-10
    assert rel(ra["dmap"].sum((2, 3)), golden["dmap_sums"]) <= 1e-9
    assert rel(rb["logits"], golden["b_logits"]) <= 1e-11 and rel(rb["loss"], golden["b_loss"]) <= 1e-12
    assert sorted(k[5:] for k in golden.files if k.startswith("grad/")) == sorted(ao.DISC_KEYS)
    for k in ao.DISC_KEYS:
        assert rel(rb["grads"][k], golden["grad/" + k]) <= 1e-10, k
        # the stored updates are float32: 6e-8 of their size
        assert rel(sd1[k] - sd0[k].double(), golden["delta1/" + k]) <= 2e-7, k
        two = ao.adam(sd0[k], [rb["grads"][k], rb2["grads"][k]], 1e-4)[1]
        assert rel(two - sd0[k].double(), golden["delta2/" + k]) <= 2e-7, k


def test_head_oracle_is_the_reference_expression():
    g = torch.Generator().manual_seed(3)
    for ext, pool in (((16, 14), (7, 7)), ((5, 5), (2, 2)), ((2, 5), (1, 2))):
        a = torch.randn(3, 8, *ext, generator=g, dtype=torch.float64)
        nf = 8 * (ext[0] // pool[0]) * (ext[1] // pool[1])
        w, b = torch.randn(2, nf, generator=g, dtype=torch.float64), torch.randn(2, generator=g, dtype=torch.float64)
        target = torch.tensor([1, 0, 1])
        h = ao.head2d(a, w, b, target, pool)
        lin = torch.nn.Linear(nf, 2).double()
        lin.weight.data.copy_(w)
        lin.bias.data.copy_(b)
        x = a.clone().requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(lin(torch.nn.AvgPool2d(pool)(x).view(3, -1)), target)
        loss.backward()
        assert torch.allclose(h["loss"], loss.detach(), rtol=1e-13) and torch.allclose(h["da"], x.grad, rtol=1e-12, atol=1e-16)
        assert torch.allclose(h["dw"], lin.weight.grad, rtol=1e-12) and torch.allclose(h["db"], lin.bias.grad, rtol=1e-12)
        assert (h["da"][:, :, ext[0] // pool[0] * pool[0]:] == 0).all()
