"""The pixel-wise contrastive loss without a GPU: tests/patch_nce_oracle.py against the numbers the reference's own ConLoss
and contrastive_loss_sup gave (tests/golden/patch_nce.npz, written by scripts/gen_golden_patch_nce.py), and the argument
contract of mis_patch_nce, which is checked before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import patch_nce_oracle as pno

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patch_nce.npz")
MIS_ERR_ARG, MIS_ERR_UNSUPPORTED, MIS_ERR_WORKSPACE = -1, -2, -4


def _golden():
    z = np.load(GOLD)
    T = float(z["temperature"])
    return [(str(n), torch.from_numpy(z[f"{n}.feat_q"]), torch.from_numpy(z[f"{n}.feat_k"]),
             torch.from_numpy(z[f"{n}.loss"]), torch.from_numpy(z[f"{n}.grad"]), T) for n in z["names"]]


def test_golden_holds_the_cases_the_oracle_is_pinned_on():
    cases = {n: (tuple(fq.shape), fq, fk) for n, fq, fk, _, _, _ in _golden()}
    assert {s for s, _, _ in cases.values()} == {(2, 16, 6, 6), (2, 32, 4, 4), (1, 16, 1, 1)}
    _, fq, fk = cases["relu_zero_2x32x4x4"]
    assert fq.min() >= 0 and fk.min() >= 0
    assert int((fq.abs().sum(1) == 0).sum()) == 1 and int((fk.abs().sum(1) == 0).sum()) == 1
    assert cases["signed_2x16x6x6"][1].min() < 0
    assert os.path.getsize(GOLD) < 100 * 1024


@pytest.mark.parametrize("form", ["materialised", "rows"])
def test_both_oracle_forms_reproduce_the_reference_in_float64(form):
    fn = pno.materialised_loss if form == "materialised" else pno.rows_loss
    for name, fq, fk, loss, grad, T in _golden():
        q = fq.clone().requires_grad_(True)
        got = fn(q, fk, T)
        got.backward()
        assert abs(got.item() - loss.item()) <= 1e-13 * max(abs(loss.item()), 1.0), (name, got.item(), loss.item())
        scale = grad.abs().max().item()
        assert (q.grad - grad).abs().max().item() <= 1e-13 * scale, name
        if scale == 0:
            assert torch.count_nonzero(q.grad) == 0


def test_both_reference_classes_gave_the_same_numbers():
    z = np.load(GOLD)
    for n in z["names"]:
        assert np.array_equal(z[f"{n}.loss"], z[f"{n}.loss_sup"]), n      # the generator asserts the gradients equal too


def test_loss_and_grad_returns_the_kernels_layout():
    for name, fq, fk, loss, grad, T in _golden():
        out, g = pno.loss_and_grad(fq, fk, T, grad_scale=0.37)
        assert out.shape == (3,) and g.shape == fq.shape
        assert abs(out[0].item() - loss.item()) <= 1e-13 * max(abs(loss.item()), 1.0)
        assert abs((out[2] - out[1]).item() - out[0].item()) <= 1e-12 * max(abs(out[2].item()), 1.0)
        assert (g - 0.37 * grad).abs().max().item() <= 1e-13 * max(grad.abs().max().item(), 1e-300)


def test_a_single_pixel_has_no_negatives_loss_and_gradient_are_exactly_zero():
    g = torch.Generator().manual_seed(3)
    for dtype in (torch.float64, torch.float32):
        fq, fk = torch.randn(3, 16, 1, 1, generator=g), torch.randn(3, 16, 1, 1, generator=g)
        out, grad = pno.loss_and_grad(fq, fk, 0.07, dtype)
        assert out[0].item() == 0.0 and torch.count_nonzero(grad) == 0
        assert pno.materialised_loss(fq, fk, 0.07, dtype).item() == 0.0


def test_the_normalisation_makes_the_loss_scale_invariant_and_k_carries_no_gradient():
    g = torch.Generator().manual_seed(4)
    fq, fk = torch.randn(2, 16, 5, 3, generator=g).double(), torch.randn(2, 16, 5, 3, generator=g).double()
    base = pno.rows_loss(fq, fk).item()
    for s in (1e3, 1e-3):
        assert abs(pno.rows_loss(fq * s, fk * s).item() - base) <= 1e-12 * base
    k = fk.clone().requires_grad_(True)
    pno.materialised_loss(fq.clone().requires_grad_(True), k).backward()
    assert k.grad is None


def test_c_abi_checks_its_arguments_before_any_launch():
    from mis_hip import lib
    L = lib.load()
    B, d, N = 12, 16, 4096
    nb = L.mis_patch_nce_workspace_bytes(B, d, N)
    assert nb > 0
    # linear in N: at most 64 bytes per feature element (the materialised logits alone would be 12 * 4096^2 * 4 = 805 MB)
    assert nb <= 64 * B * N * d
    assert L.mis_patch_nce_workspace_bytes(B, 32, 2 * N) <= 64 * B * 2 * N * 32
    assert L.mis_patch_nce_workspace_bytes(B, 24, N) == MIS_ERR_UNSUPPORTED
    assert L.mis_patch_nce_workspace_bytes(0, d, N) == MIS_ERR_ARG

    host = (ctypes.c_float * 64)()            # never dereferenced: every call below is refused before a launch
    p = ctypes.cast(host, ctypes.c_void_p)

    def call(fq=p, fk=p, B=B, d=d, N=N, T=0.07, out=p, ws=p, nbytes=nb, q_bs=None):
        bs = d * N if q_bs is None else q_bs
        return L.mis_patch_nce(fq, bs, fk, d * N, B, d, N, T, 1.0, out, None, 0, ws, nbytes, None)

    assert call(fq=None) == MIS_ERR_ARG and call(fk=None) == MIS_ERR_ARG
    assert call(out=None) == MIS_ERR_ARG and call(ws=None) == MIS_ERR_ARG
    assert call(B=0) == MIS_ERR_ARG and call(N=0) == MIS_ERR_ARG and call(d=0) == MIS_ERR_ARG
    assert call(T=0.0) == MIS_ERR_ARG and call(q_bs=0) == MIS_ERR_ARG
    assert call(d=24) == MIS_ERR_UNSUPPORTED
    assert call(nbytes=nb - 1) == MIS_ERR_WORKSPACE and call(nbytes=0) == MIS_ERR_WORKSPACE
