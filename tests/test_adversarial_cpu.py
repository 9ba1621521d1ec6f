"""What of the adversarial feature can be held without a GPU: the C ABI (header, exports, refusals before any launch), the
float64 oracle of tests/adversarial_oracle.py against the REAL reference discriminator (tests/golden/adversarial_3d.npz,
scripts/gen_golden_adversarial.py) and against itself (convolution operator vs a plain sum over the taps), the constants the
GPU tests take from it (FLOOR, the undecided share), the discriminator's state_dict and the command line."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adversarial_oracle as ao
import conv_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "adversarial_3d.npz")
NAMES = {"mis_channel_dropout_scale", "mis_conv_k4s2_fwd_workspace_bytes", "mis_conv_k4s2_fwd", "mis_conv_k4s2_dgrad",
         "mis_conv_k4s2_wgrad_workspace_bytes", "mis_conv_k4s2_wgrad", "mis_adv_head_workspace_bytes", "mis_adv_head_fwd",
         "mis_adv_head_bwd", "mis_adversarial_tail_workspace_bytes", "mis_adversarial_tail", "mis_adam_init", "mis_adam_step"}


def test_header_parses_and_every_exported_symbol_is_declared():
    from mis_hip import lib
    header = open(os.path.join(ROOT, "include", "mis_hip_adversarial.h")).read()
    declared = set(re.findall(r"\b(mis_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    assert "mis_hip_adversarial.h" in lib.EXTRA_HEADERS
    protos = lib.EXTRA_PROTOTYPES["mis_hip_adversarial.h"]
    assert declared == NAMES == set(protos) == set(lib.parse_header(header)) and not NAMES & set(lib.PROTOTYPES)
    source = open(os.path.join(ROOT, "cv-ssl-mis_amd", "csrc", "adversarial.hip")).read()
    defined = set(re.findall(r'^extern "C" [\w \*]+?\b(mis_\w+)\s*\(', source, flags=re.M))
    assert defined == NAMES, (defined ^ NAMES)
    assert "adversarial.hip" in open(os.path.join(ROOT, "cv-ssl-mis_amd", "csrc", "Makefile")).read()
    P, I, LL, F, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_uint
    assert protos["mis_conv_k4s2_fwd"] == (I, [P, LL, I, P, LL, I, P, P, P, P, P, LL, I, I, I, I, I, F, P, P, LL, P])
    assert protos["mis_conv_k4s2_dgrad"] == (I, [P, LL, P, LL, F, P, P, P, LL, I, I, I, I, I, I, P])
    assert protos["mis_adam_step"] == (I, [P, P, P, P, LL, F, F, F, F, P, P])
    assert protos["mis_channel_dropout_scale"] == (I, [P, I, I, F, U, P, P])
    L = lib.load()
    for n in NAMES:
        assert hasattr(L, n), n


def test_entry_points_refuse_bad_arguments_before_launching():
    """NULL pointers, extents <= 0, odd extents, short workspaces: the status comes back from the argument checks (no device
    is needed to see that; the non-NULL pointers below are never dereferenced)."""
    from mis_hip import lib
    L = lib.load()
    p = ctypes.c_void_p(0x1000)
    ARG, UNS, WS = -1, -2, -4
    geo = (1, 8, 4, 6, 10)                       # N, Cout, D, H, W
    S, So = 4 * 6 * 10, 2 * 3 * 5

    def fwd(x=p, w=p, y=p, N=1, Cout=8, D=4, H=6, W=10, slope=0.2, ws=p, wsb=1 << 30, Cx=3, xbs=3 * S):
        return L.mis_conv_k4s2_fwd(x, xbs, Cx, None, 0, 0, w, None, None, None, y, Cout * (D // 2) * (H // 2) * (W // 2), N, Cout,
                                   D, H, W, slope, None, ws, wsb, None)

    def dgrad(dy=p, w=p, dx=p, N=1, Cin=3, Cout=8, D=4, H=6, W=10):
        return L.mis_conv_k4s2_dgrad(dy, Cout * So, None, 0, 0.2, None, w, dx, Cin * S, N, Cin, Cout, D, H, W, None)

    def wgrad(x=p, dy=p, dw=p, N=1, Cout=8, D=4, H=6, W=10, ws=p, wsb=1 << 30):
        return L.mis_conv_k4s2_wgrad(x, 3 * S, 3, None, 0, 0, dy, Cout * So, None, 0, 0.2, None, dw, None, None, None, N, Cout,
                                     D, H, W, 0, ws, wsb, None)
    for call in (fwd, dgrad, wgrad):
        for kw in (dict(N=0), dict(Cout=0), dict(D=0), dict(H=-2), dict(W=0)):
            assert call(**kw) == ARG, (call.__name__, kw)
        for kw in (dict(D=5), dict(H=7), dict(W=1), dict(D=3, H=3, W=3)):
            assert call(**kw) == UNS, (call.__name__, kw)
    assert fwd(x=None) == ARG and fwd(w=None) == ARG and fwd(y=None) == ARG and fwd(slope=0.0) == ARG and fwd(xbs=S) == ARG
    assert dgrad(dy=None) == ARG and dgrad(w=None) == ARG and dgrad(dx=None) == ARG and dgrad(Cin=0) == ARG
    assert wgrad(x=None) == ARG and wgrad(dy=None) == ARG and wgrad(dw=None) == ARG
    assert L.mis_conv_k4s2_fwd(p, 5 * S, 0, p, 5 * S, 5, None, p, None, None, p, 8 * So, *geo, 0.2, None, p, 1 << 30, None) == UNS
    # the workspace queries agree with the entry points: a sliced forward and a sliced weight gradient refuse a short one
    need = L.mis_conv_k4s2_fwd_workspace_bytes(1, 256, 512, 4, 4, 4)
    assert need > 0 and L.mis_conv_k4s2_fwd_workspace_bytes(4, 1, 64, 96, 96, 96) == 0
    big = dict(N=1, Cout=512, D=4, H=4, W=4, Cx=256, xbs=256 * 64)
    assert fwd(**big, wsb=need - 1) == WS and fwd(**big, ws=None, wsb=need) == WS
    need = L.mis_conv_k4s2_wgrad_workspace_bytes(1, 3, 8, 4, 6, 10)
    assert need >= 0 and L.mis_conv_k4s2_wgrad_workspace_bytes(4, 3, 64, 96, 96, 96) > 0
    assert L.mis_conv_k4s2_wgrad(p, 3 * 96 ** 3, 3, None, 0, 0, p, 64 * 48 ** 3, None, 0, 0.2, None, p, None, None, None, 4, 64,
                                 96, 96, 96, 0, p, 16, None) == WS
    for q in (L.mis_conv_k4s2_fwd_workspace_bytes, L.mis_conv_k4s2_wgrad_workspace_bytes):
        assert q(0, 3, 8, 4, 6, 10) == ARG and q(1, 0, 8, 4, 6, 10) == ARG and q(1, 3, 8, 4, 5, 10) == UNS
    assert L.mis_channel_dropout_scale(None, 2, 4, 0.5, 1, p, None) == ARG
    assert L.mis_channel_dropout_scale(p, 2, 4, 1.0, 1, p, None) == ARG and L.mis_channel_dropout_scale(p, 0, 4, 0.5, 1, p, None) == ARG
    # head
    hb = L.mis_adv_head_workspace_bytes(4, 512, 2)
    assert hb == (4 * 512 + 4 * 2 + 4) * 4 and L.mis_adv_head_workspace_bytes(0, 512, 2) == ARG
    head = lambda a=p, N=4, pool=(6, 6, 6), wsb=hb, K=2: L.mis_adv_head_fwd(a, 512 * 216, p, p, p, p, p, N, 512, K, 6, 6, 6, *pool,
                                                                            p, wsb, None)
    assert head(a=None) == ARG and head(N=0) == ARG and head(pool=(0, 6, 6)) == ARG
    assert head(pool=(3, 6, 6)) == UNS and head(K=9) == UNS and head(wsb=hb - 1) == WS
    assert L.mis_adv_head_bwd(None, p, 512 * 216, p, p, 0, 4, 512, 2, 6, 6, 6, p, hb, None) == ARG
    assert L.mis_adv_head_bwd(p, p, 512 * 216, p, p, 0, 4, 512, 2, 6, 6, 6, p, hb - 1, None) == WS
    # tail
    tb = L.mis_adversarial_tail_workspace_bytes(4, 2, 96 ** 3)
    assert tb > 0 and L.mis_adversarial_tail_workspace_bytes(4, 2, 0) == ARG
    tail = lambda s=p, dmap=p, B=4, Lb=2, C=2, Sv=64, wsb=tb: L.mis_adversarial_tail(s, C * Sv, p, 1, dmap, C * Sv, p, B, Lb, C, Sv,
                                                                                   0.1, None, 1.0, p, p, C * Sv, p, wsb, None)
    assert tail(s=None) == ARG and tail(dmap=None) == ARG and tail(Lb=5) == ARG and tail(Sv=0) == ARG
    assert tail(C=5) == UNS and tail(wsb=8) == WS
    # Adam
    assert L.mis_adam_init(None, 0, None) == ARG and L.mis_adam_init(p, -1, None) == ARG
    assert L.mis_adam_step(None, p, p, p, 4, 1e-4, 0.9, 0.99, 1e-8, p, None) == ARG
    assert L.mis_adam_step(p, p, p, p, 0, 1e-4, 0.9, 0.99, 1e-8, p, None) == ARG
    assert L.mis_adam_step(p, p, p, p, 4, 1e-4, 1.0, 0.99, 1e-8, p, None) == ARG
    assert L.mis_adam_step(p, p, p, p, 4, 1e-4, 0.9, 0.99, 1e-8, None, None) == ARG


def test_discriminator_spec_and_command_line_are_the_references():
    from networks.discriminator import FC3DDiscriminator, FCDiscriminator
    spec = FC3DDiscriminator.spec(2)
    assert [k for k, _ in spec] == list(ao.DISC_KEYS) and dict(spec) == ao.disc_shapes(2, 64, 1)
    assert dict(FC3DDiscriminator.spec(3, ndf=8, n_channel=2))["conv1.weight"] == (8, 2, 4, 4, 4)
    assert dict(spec)["conv4.weight"] == (512, 256, 4, 4, 4) and dict(spec)["classifier.weight"] == (2, 512)
    with pytest.raises(NotImplementedError):
        FCDiscriminator(2)
    import train_adversarial_network_3D as t
    d = vars(t.parser.parse_args([]))
    assert d == dict(root_path='../data/BraTS2019', exp='BraTs2019_Adversarial_Network', model='unet_3D', max_iterations=30000,
                     batch_size=4, deterministic=1, base_lr=0.01, DAN_lr=0.0001, patch_size=[96, 96, 96], seed=1337,
                     labeled_bs=2, labeled_num=25, ema_decay=0.99, consistency_type="mse", consistency=0.1,
                     consistency_rampup=200.0)
    from mis_hip import step, train_common
    assert hasattr(step, "AdversarialTrainer") and hasattr(train_common, "run_adversarial")


def test_both_discriminators_declare_their_layer_law_on_one_body():
    import adversarial2d_oracle as ao2
    from networks.discriminator import SLOPE, FC3DDiscriminator, _K4S2Discriminator
    from networks.discriminator_2d import FCDiscriminator
    assert FCDiscriminator.LAYER_ACT == ao2.LAYER_ACT
    assert SLOPE == ao.SLOPE and FC3DDiscriminator.LAYER_ACT == ((SLOPE, True),) * 3 + ((SLOPE, False),)
    for cls in (FC3DDiscriminator, FCDiscriminator):
        assert cls.loss_forward is _K4S2Discriminator.loss_forward and cls.loss_backward is _K4S2Discriminator.loss_backward
        assert cls._static is _K4S2Discriminator._static


def test_plain_sum_over_the_taps_agrees_with_the_convolution_operator():
    for name in ("all-padding/offset", "ragged/uniform", "thin/relu_scaled", "cube-5-20/relu_scaled", "views/relu_scaled"):
        c = ao.case(name)
        plain, r64 = ao.plain64(c), ao.references(name)[0]
        for k in ao.KINDS:
            assert (plain[k] - r64[k]).abs().max().item() <= 3e-15 * max(r64[k].abs().max().item(), 1.0), (name, k)
    # the same through the whole discriminator: disc_forward on a convolution that uses no convolution operator
    sd = {k: v.double() for k, v in ao.golden_state_dict(2, 2, 1).items()}
    g = torch.Generator().manual_seed(5)
    probs = torch.softmax(torch.randn(1, 2, 16, 16, 16, generator=g, dtype=torch.float64), 1)
    img = torch.randn(1, 1, 16, 16, 16, generator=g, dtype=torch.float64)

    def plain_conv(x, w, b):
        c = dict(x=x, w=w, b=b, dy=torch.zeros(x.shape[0], w.shape[0], *[s // 2 for s in x.shape[2:]], dtype=torch.float64))
        return ao.plain64(c)["y"]
    a = ao.disc_forward(sd, probs, img, pool=(1, 1, 1))[0]
    b = ao.disc_forward(sd, probs, img, pool=(1, 1, 1), conv_fn=plain_conv)[0]
    assert (a - b).abs().max().item() <= 1e-14


def test_floor_is_the_largest_e32_of_the_matrix_and_the_margin_leaves_few_decisions_out():
    worst = {k: 0.0 for k in ao.KINDS}
    for name in ao.names():
        _, _, e32 = ao.references(name)
        for k in ao.KINDS:
            worst[k] = max(worst[k], max(e32[k][m] for m in ao.MEASURES))
    assert {k: co.ceil2(v) for k, v in worst.items()} == ao.FLOOR, worst
    # the epilogue cases of tests/test_adversarial_kernels_gpu.py: the oracle's own undecided share stays under the cap
    for name in ("cube-3-8/uniform", "ragged/relu_scaled", "wide-n3/uniform", "sliced/uniform"):
        assert ao.undecided_share(ao.references(name)[0]["y"]) <= ao.UNDECIDED_CAP, name


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def golden_runs():
    """The oracle on the golden's closed-form inputs: phase A, phase B and the two Adam steps.  Computed once."""
    vol, logits, _ = ao.golden_inputs(4, 2, 96)
    sd0 = ao.golden_state_dict(2, 4, 1)
    masks = ao.golden_masks(4, 4)
    probs = torch.softmax(logits.double(), 1)
    target = torch.tensor([1, 1, 0, 0])
    ra = ao.disc_step(sd0, probs[2:], vol[2:], target[:2], None)
    rb = ao.disc_step(sd0, probs, vol, target, masks)
    sd1 = {k: ao.adam(sd0[k], [rb["grads"][k]], 1e-4)[0] for k in sd0}
    rb2 = ao.disc_step(sd1, probs, vol, target, masks)
    return sd0, ra, rb, sd1, rb2


def test_oracle_reproduces_the_reference_iteration(golden, golden_runs):
    sd0, ra, rb, sd1, rb2 = golden_runs
    assert float(golden["oracle_vs_reference_worst_rel"]) <= 1e-10

    def rel(a, b):
        b = torch.from_numpy(np.asarray(b)).double()
        return ((torch.as_tensor(a).double().reshape(b.shape) - b).abs().max() / b.abs().max()).item()
    assert rel(ra["logits"], golden["a_logits"]) <= 1e-11 and rel(ra["loss"], golden["a_loss"]) <= 1e-12
    assert rel(ao.lattice(ra["dmap"]), golden["dmap_lattice"]) <= 1e-10
    assert rel(ra["dmap"].sum((2, 3, 4)), golden["dmap_sums"]) <= 1e-9
    assert rel(rb["logits"], golden["b_logits"]) <= 1e-11 and rel(rb["loss"], golden["b_loss"]) <= 1e-12
    assert sorted(k[5:] for k in golden.files if k.startswith("grad/")) == sorted(ao.DISC_KEYS)
    for k in ao.DISC_KEYS:
        assert rel(rb["grads"][k], golden["grad/" + k]) <= 1e-10, k
        # the stored updates are float32: 6e-8 of their size
        assert rel(sd1[k] - sd0[k].double(), golden["delta1/" + k]) <= 2e-7, k
        two = ao.adam(sd0[k], [rb["grads"][k], rb2["grads"][k]], 1e-4)[1]
        assert rel(two - sd0[k].double(), golden["delta2/" + k]) <= 2e-7, k


def test_head_tail_and_adam_oracles_are_the_reference_expressions():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(3, 8, 2, 3, 1, generator=g, dtype=torch.float64)
    w, b = torch.randn(2, 8, generator=g, dtype=torch.float64), torch.randn(2, generator=g, dtype=torch.float64)
    target = torch.tensor([1, 0, 1])
    h = ao.head(a, w, b, target)
    lin = torch.nn.Linear(8, 2).double()
    lin.weight.data.copy_(w)
    lin.bias.data.copy_(b)
    x = a.clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(lin(torch.nn.AvgPool3d((2, 3, 1))(x).view(3, -1)), target)
    loss.backward()
    assert torch.allclose(h["loss"], loss.detach(), rtol=1e-13) and torch.allclose(h["da"], x.grad, rtol=1e-12, atol=1e-16)
    assert torch.allclose(h["dw"], lin.weight.grad, rtol=1e-12) and torch.allclose(h["db"], lin.bias.grad, rtol=1e-12)
    # tail: the unlabeled gradient is w * d cons / d logits for ANY cons whose gradient at softmax(logits[L:]) is dmap
    lg = torch.randn(3, 2, 2, 3, 5, generator=g, dtype=torch.float64)
    lab = torch.randint(0, 2, (3, 2, 3, 5), generator=g).to(torch.uint8)
    q = torch.randn(2, 2, 2, 3, 5, generator=g, dtype=torch.float64)
    s = lg.clone().requires_grad_(True)
    cons = (torch.softmax(s[1:], 1) ** 2 * q).sum()
    (want,) = torch.autograd.grad(0.3 * cons, [s])
    dmap = (2 * torch.softmax(lg[1:], 1) * q)
    out, got = ao.tail(lg, lab, 1, dmap, cons.item(), 0.3)
    assert torch.allclose(got[1:], want[1:], rtol=1e-12, atol=1e-16) and abs(out[3].item() - cons.item()) < 1e-15
    assert abs(out[0].item() - (0.5 * (out[1] + out[2]) + 0.3 * cons).item()) < 1e-14
    # Adam from a state at step 999 is torch's own 1000th step
    p = torch.nn.Parameter(torch.randn(7, generator=g, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=1e-4, betas=(0.9, 0.99))
    p0 = p.detach().clone()
    gr = torch.randn(7, generator=g, dtype=torch.float64)
    p.grad = gr.clone()
    opt.step()
    assert torch.equal(ao.adam(p0, [gr], 1e-4)[0], p.detach())
