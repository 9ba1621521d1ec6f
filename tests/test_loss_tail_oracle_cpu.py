"""The float64 loss-tail reference (tests/loss_tail_oracle.py) is itself checked here, without a GPU: against the oracle
losses that test_oracle_cpu.py pins to the upstream goldens, against itself across the five tails, and by gradcheck."""
import pytest
import torch

import loss_tail_oracle as lto

S8 = (2, 4)            # S = 8
W = 0.37


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _inputs(C, B=4, L=2, spatial=(4, 6), seed=0):
    g = _gen(seed)
    r = lambda n: torch.randn((n, C) + tuple(spatial), generator=g) * 3.0
    label = torch.randint(0, C, (L,) + tuple(spatial), generator=g)
    return dict(s=r(B), t=r(B - L), t1=r(B - L), other=r(B), label=label, lam=torch.rand(B - L, generator=g),
                r=r(B - L), g=g)


@pytest.mark.parametrize("C", [2, 3, 4])
def test_dice_and_softmax_mse_agree_with_the_oracle_losses(C):
    from oracle.losses import dice_loss, softmax_mse
    x = _inputs(C, spatial=(3, 4, 5), seed=C)
    L = 2
    s64 = x["s"].double()
    probs = torch.softmax(s64[:L], 1)
    want_dice = dice_loss(probs, x["label"].unsqueeze(1), C)
    want_mse = softmax_mse(s64[L:], x["t"].double()).mean()
    per_class = lto.dice_per_class(probs, x["label"], C)
    assert abs(per_class.mean().item() - want_dice.item()) <= 1e-14
    out, _ = lto.mean_teacher_tail(x["s"], x["t"], x["label"], L, W)
    assert abs(out[2].item() - want_dice.item()) <= 1e-14
    assert abs(out[3].item() - want_mse.item()) <= 1e-15
    assert torch.allclose(out[5:5 + C], 1 - per_class, rtol=0, atol=1e-15)
    assert abs(out[0].item() - (0.5 * (out[1] + out[2]) + W * out[3]).item()) <= 1e-15


@pytest.mark.parametrize("C", [2, 3, 4])
def test_all_tails_share_the_supervised_part(C):
    x = _inputs(C, spatial=(6, 6), seed=10 + C)
    L = 2
    pm = lto.uamt_mean_probs(2, C, (6, 6), lto.uamt_threshold(50, 100), x["g"])
    outs = [lto.mean_teacher_tail(x["s"], x["t"], x["label"], L, 0.0)[0],
            lto.cross_tail(x["s"], x["other"], x["label"], L, 0.0)[0],
            lto.cross_tail(x["s"], x["other"], x["label"], L, 0.0, pseudo_ce=True)[0],
            lto.uamt_tail(x["s"], x["t"], pm, x["label"], L, 0.0, 50, 100)[0],
            lto.ict_tail(x["s"], x["t"], x["t1"], x["lam"], x["label"], L, 0.0)[0],
            lto.dct_tail(x["s"], x["r"], x["label"], L, 1, 0.0)[0]]
    for o in outs[1:]:
        assert torch.equal(o[:3], outs[0][:3])
    assert outs[0][0].item() == 0.5 * (outs[0][1] + outs[0][2]).item()


def test_cross_tail_without_teacher_equals_zero_mt_weight():
    x = _inputs(3, seed=5)
    a, ga = lto.cross_tail(x["s"], x["other"], x["label"], 2, W)
    b, gb = lto.cross_tail(x["s"], x["other"], x["label"], 2, W, teacher=x["t"], mt_weight=0.0)
    assert torch.equal(a, b[:5]) and torch.equal(ga, gb) and b[6].item() == 0.0 and b[5].item() > 0
    c, gc = lto.cross_tail(x["s"], x["other"], x["label"], 2, W, teacher=x["t"], mt_weight=0.2)
    assert abs(c[0].item() - (a[0] + 0.2 * c[5]).item()) <= 1e-15 and not torch.equal(ga, gc)
    assert torch.equal(gc[:2], ga[:2])                        # the teacher term never reaches a labeled row


def test_gates_splits_and_loss_scale():
    x = _inputs(3, seed=6)
    o1, g1 = lto.mean_teacher_tail(x["s"], x["t"], x["label"], 2, W, loss_scale=1.0)
    o2, g2 = lto.mean_teacher_tail(x["s"], x["t"], x["label"], 2, W, loss_scale=0.25)
    assert torch.equal(o1, o2) and torch.allclose(g2, 0.25 * g1, rtol=1e-15, atol=0)
    o0, g0 = lto.mean_teacher_tail(x["s"], x["t"], x["label"], 2, W, gate=0.0)
    assert o0[3].item() == 0.0 and o0[4].item() == W and (g0[2:] == 0).all() and torch.equal(g0[:2], g1[:2])
    ob, gb = lto.mean_teacher_tail(x["s"][:2], None, x["label"], 2, W)                # L == B
    assert torch.equal(ob[1:3], o1[1:3]) and ob[3].item() == 0.0 and torch.equal(gb, g1[:2])
    oz, gz = lto.mean_teacher_tail(x["s"][2:], x["t"], None, 0, W)                    # L == 0
    assert oz[1].item() == 0.0 and oz[2].item() == 0.0 and (oz[5:] == 1).all() and oz[3].item() == o1[3].item()
    for f32, f64 in zip(lto.mean_teacher_tail(x["s"], x["t"], x["label"], 2, W, dtype=torch.float32), (o1, g1)):
        assert f32.double().sub(f64).abs().max().item() <= 1e-5 * f64.abs().max().item()
    assert lto.mean_teacher_tail(x["s"], x["t"], x["label"], 2, W, dtype=torch.float32)[1].dtype == torch.float32


@pytest.mark.parametrize("C", [2, 3, 4])
def test_gradcheck_on_every_tail(C):
    x = _inputs(C, B=3, L=1, spatial=S8, seed=20 + C)
    d = lambda k: x[k].double()
    L, lab = 1, x["label"]
    thr = lto.uamt_threshold(30, 100)
    pm = lto.uamt_mean_probs(2, C, S8, thr, x["g"])
    assert 0 < int((lto.uamt_entropy(pm) < thr).sum()) < pm.numel() // C
    fns = {
        "mean_teacher": lambda s: lto.mean_teacher_loss(s, d("t"), lab, L, W)[0],
        "cross_dice": lambda s: lto.cross_loss(s, x["other"], lab, L, W)[0],
        "cross_ce": lambda s: lto.cross_loss(s, x["other"], lab, L, W, pseudo_ce=True)[0],
        "cross_mt": lambda s: lto.cross_loss(s, x["other"], lab, L, W, teacher=d("t"), mt_weight=0.2)[0],
        "uamt": lambda s: lto.uamt_loss(s, d("t"), pm, lab, L, W, 30, 100)[0],
        "ict": lambda s: lto.ict_loss(s, d("t"), d("t1"), x["lam"], lab, L, W)[0],
    }
    for name, fn in fns.items():
        s = d("s").clone().requires_grad_(True)
        assert torch.autograd.gradcheck(fn, (s,), eps=1e-6, atol=1e-7, rtol=1e-5), name
    # deep co-training stops the gradient on one side of each half: its analytic gradient is that of the expression
    # with the detached operands held constant, which is what the finite difference sees when they are precomputed
    sq = (2, C, 4, 4)
    g = x["g"]
    a0, r0 = torch.randn((3, C, 4, 4), generator=g).double() * 3, torch.randn(sq, generator=g).double() * 3
    lab4 = torch.randint(0, C, (1, 4, 4), generator=g)
    for k in range(4):
        _, ga, gr = lto.dct_tail(a0, r0, lab4, 1, k, W)
        qc = torch.softmax(r0, 1)
        rpc = torch.rot90(torch.softmax(a0[1:], 1), k, [2, 3])

        def frozen(a, r):
            sup = lto.mean_teacher_loss(a[:1], None, lab4, 1, 0.0)[0]
            q, rp = torch.softmax(r, 1), torch.rot90(torch.softmax(a[1:], 1), k, [2, 3])
            return sup + W * 0.5 * (torch.mean((qc - rp) ** 2) + torch.mean((q - rpc) ** 2))

        a, r = a0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
        assert torch.autograd.gradcheck(frozen, (a, r), eps=1e-6, atol=1e-7, rtol=1e-5), k
        fa, fr = torch.autograd.grad(frozen(a, r), [a, r])
        assert torch.allclose(fa, ga, rtol=1e-12, atol=1e-15) and torch.allclose(fr, gr, rtol=1e-12, atol=1e-15)


def test_argmax_first_takes_the_first_maximum():
    x = torch.full((2, 4, 5), 1.5)
    assert (lto.argmax_first(x) == 0).all()
    x = torch.tensor([[1.0, -2.0, 1.0, 0.5], [-0.0, 0.0, -1.0, -1.0], [0.0, -0.0, -1.0, -1.0], [0.1, 0.3, 0.3, 0.2]])
    assert lto.argmax_first(x).tolist() == [0, 0, 0, 1]
    r = torch.randn((3, 4, 50), generator=_gen(1))
    r[:, 2, ::3] = r[:, 0, ::3]
    assert torch.equal(lto.argmax_first(r), torch.argmax(r, 1))


@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("frac", [0.0, 0.5, 1.0])
def test_uamt_builder_leaves_no_undecided_voxel(C, frac):
    max_it = 1000
    thr = lto.uamt_threshold(int(frac * max_it), max_it)
    pm = lto.uamt_mean_probs(3, C, (16, 16, 16), thr, _gen(C * 10 + int(frac * 2)))
    assert pm.dtype == torch.float32 and not lto.uamt_undecided(pm, thr).any()
    assert (pm.double().sum(1) - 1).abs().max().item() <= 1e-6 and (pm > 0).all()
    h64 = lto.uamt_entropy(pm)
    h32 = -(pm * torch.log(pm + 1e-6)).sum(1)
    assert torch.equal(h64 < thr, h32 < thr)                 # the same mask in either precision
    assert (h64 < thr).any()


def test_uamt_mask_all_out_and_threshold():
    import math
    assert abs(lto.uamt_threshold(100, 100) - math.log(2.0)) < 1e-16
    assert abs(lto.uamt_threshold(0, 100) - (0.75 + 0.25 * math.exp(-5.0)) * lto.LN2) < 1e-16
    x = _inputs(3, seed=9)
    pm = torch.full((2, 3, 4, 6), 1.0 / 3.0)
    out, g = lto.uamt_tail(x["s"], x["t"], pm, x["label"], 2, W, 0, 100)
    assert out[3].item() == 0.0 and out[8].item() == 0.0 and (g[2:] == 0).all() and g[:2].abs().max() > 0


def test_softmax_mean_accumulate_is_the_mean_prediction():
    g = _gen(3)
    U, R, C = 3, 2, 4
    passes = [torch.randn((R * U, C, 4, 4), generator=g) * 3 for _ in range(4)]
    acc = None
    for i, z in enumerate(passes):
        acc = lto.softmax_mean_accumulate(z, acc, R, 1.0 / 8, first=(i == 0))
    want = torch.stack([torch.softmax(z.double(), 1).reshape(R, U, C, 4, 4) for z in passes]).sum((0, 1)) / 8
    assert torch.allclose(acc, want, rtol=0, atol=1e-15) and (acc.sum(1) - 1).abs().max().item() < 1e-14
