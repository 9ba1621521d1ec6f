"""The hand-offs between streaming kernels of the 3-D UNet that no longer go through HBM, each held to the launches it
replaces -- exactly: these kernels move, select and re-use values, they must not round differently.

  1. mis_norm_act_fwd_pool on a 3-D volume (apply_fwd_pool3d_kernel) == mis_norm_act_fwd_g + mis_maxpool2_fwd:
     activation (written into a channel slice of a wider buffer), pooled tensor, argmax codes.
  2. mis_norm_head_fwd / _bwd with the stored dropout words (drop_bits) == the same pair drawing them three times:
     logits, dx, dw, db, the partial sums in the workspace, dgamma / dbeta; an explicit mask makes the buffer inert.
  Plan level: one unet_3D Mean-Teacher step at 2 x 1 x 32^3 with both switches on and off, eager and through a recorded
  and replayed tape step: logits, flat gradient and losses equal bit for bit.

Comparisons are torch.equal with NaNs compared by position."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

N, C = 2, 3


def _ops():
    from mis_hip import ops
    return ops


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float().cuda()


def _same(a, b, what):
    """Exact equality; NaNs must stand at the same positions."""
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.is_floating_point():
        na, nb = a.isnan(), b.isnan()
        assert torch.equal(na, nb), (what, "NaN positions")
        assert torch.equal(a.masked_fill(na, 0.0), b.masked_fill(nb, 0.0)), (what, (a - b).abs().nan_to_num(0.0).max().item())
    else:
        assert torch.equal(a, b), what


def _state(seed=1337):
    ops = _ops()
    st = ops.new_step_state()
    ops.step_init(st, seed, 3, 0.01, 30000, 0.99, 0.1, 200.0)
    return st


def _norm_kind(kind, seed):
    """(per_sample, cg, mean, rstd, gamma, beta) of InstanceNorm, a BatchNorm-style per-channel norm with affine, GroupNorm with
    one group of 3 channels and affine.  The statistics are inputs of the kernels under test: any finite values serve."""
    G = {"in": N * C, "bn": C, "gn": N}[kind]
    mean = _rand(G, seed=seed, scale=0.3)
    rstd = _rand(G, seed=seed + 1).abs() + 0.5
    gamma = beta = None
    if kind != "in":
        gamma, beta = _rand(C, seed=seed + 2) + 1.0, _rand(C, seed=seed + 3, scale=0.2)
    return kind != "bn", 3 if kind == "gn" else 1, mean, rstd, gamma, beta


# ---------------------------------------------------------------------------------------------------------- part 1
def _pool_inputs(D, H, W):
    """name -> x: the maximum of window i at window position i % 8 (all eight positions occur); one window of four equal maxima
    among ties of the clamped negatives; one NaN."""
    base = _rand(N, C, D, H, W, seed=D * 100 + W)
    win = base.view(N, C, D // 2, 2, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(-1, 8)
    pos = torch.arange(win.shape[0], device="cuda") % 8
    boosted = win.clone()
    boosted[torch.arange(win.shape[0], device="cuda"), pos] = 9.0 + pos.float()
    every = boosted.view(N, C, D // 2, H // 2, W // 2, 2, 2, 2).permute(0, 1, 2, 5, 3, 6, 4, 7).reshape(N, C, D, H, W).contiguous()
    ties = base.clone()
    ties[1, 2, 0, 0:2, 2:4] = 7.5          # dz = 0: (dy, dx) all four equal -> code 0; the plane above stays below them
    nan = base.clone()
    nan[0, 1, 1, 1, 5] = float("nan")
    return {"every": every, "ties": ties, "nan": nan}


@pytest.mark.parametrize("kind", ["in", "bn", "gn"])
@pytest.mark.parametrize("geom", [(2, 2, 8), (4, 6, 12), (6, 4, 24)])
def test_pool3d_in_the_apply_pass_equals_apply_then_pool(geom, kind):
    ops = _ops()
    D, H, W = geom
    per_sample, cg, mean, rstd, gamma, beta = _norm_kind(kind, seed=7)
    st = _state()
    So = (D // 2, H // 2, W // 2)
    for (name, x), slope, p in itertools.product(_pool_inputs(D, H, W).items(), (0.0, 0.01), (0.3, 0.0)):
        what = (geom, kind, name, slope, p)
        wide_ref, wide = torch.zeros(N, C + 2, D, H, W, device="cuda"), torch.zeros(N, C + 2, D, H, W, device="cuda")
        y_ref, y = wide_ref[:, 1:1 + C], wide[:, 1:1 + C]
        pooled_ref, pooled = torch.empty(N, C, *So, device="cuda"), torch.empty(N, C, *So, device="cuda")
        idx_ref = torch.full((pooled.numel(),), 255, dtype=torch.uint8, device="cuda")
        idx = idx_ref.clone()
        drop = dict(drop_p=p, drop_salt=5, state=st if p > 0 else None)
        ops.norm_act_fwd(x, y_ref, per_sample, mean, rstd, gamma, beta, slope, cg=cg, **drop)
        ops.maxpool2_fwd(y_ref, pooled_ref, idx_ref)
        ops.norm_act_fwd_pool(x, y, pooled, idx, per_sample, mean, rstd, gamma, beta, slope, cg=cg, **drop)
        _same(wide, wide_ref, what + ("activation",))          # the slice, and nothing beside it
        _same(pooled, pooled_ref, what + ("pooled",))
        _same(idx, idx_ref, what + ("argmax codes",))
        # a forward nobody differentiates passes no code buffer
        wide2, pooled2 = torch.zeros_like(wide), torch.empty_like(pooled)
        ops.norm_act_fwd_pool(x, wide2[:, 1:1 + C], pooled2, None, per_sample, mean, rstd, gamma, beta, slope, cg=cg, **drop)
        _same(wide2, wide_ref, what + ("activation, no codes",))
        _same(pooled2, pooled_ref, what + ("pooled, no codes",))
        if kind == "in" and name == "ties" and p == 0.0:        # a monotone map of x: the four equal maxima stay the maxima
            assert idx_ref.view(N, C, *So)[1, 2, 0, 0, 1].item() == 0, what      # ... and the first of them wins


def test_pool3d_every_window_position_wins_somewhere():
    """The input of the case above really puts a maximum at each of the eight window positions."""
    ops = _ops()
    D, H, W = 2, 2, 8
    x = _pool_inputs(D, H, W)["every"]
    mean, rstd = torch.zeros(N * C, device="cuda"), torch.ones(N * C, device="cuda")
    y, pooled = torch.empty_like(x), torch.empty(N, C, 1, 1, 4, device="cuda")
    idx = torch.empty(pooled.numel(), dtype=torch.uint8, device="cuda")
    ops.norm_act_fwd_pool(x, y, pooled, idx, True, mean, rstd, None, None, 0.0)
    assert sorted(set(idx.tolist())) == list(range(8))
    assert torch.equal(idx.cpu(), torch.arange(idx.numel()).to(torch.uint8) % 8)


# ---------------------------------------------------------------------------------------------------------- part 2
def _head_run(ops, x, dl, w, b, per_sample, mean, rstd, gamma, beta, K, p, st, mask, bits):
    """Forward + backward of the fused head; every tensor it writes, the workspace's partial sums included."""
    Nn, Cc = x.shape[:2]
    S = x[0, 0].numel()
    logits = torch.empty(Nn, K, *x.shape[2:], device="cuda")
    drop = dict(drop_p=p, drop_salt=9, state=st if p > 0 else None, drop_mask=mask)
    ops.norm_head_fwd(x, logits, per_sample, mean, rstd, gamma, beta, 0.01, w, b, bits=bits, **drop)
    dx = torch.empty_like(x)
    dw, db = torch.empty(K, Cc, device="cuda"), torch.empty(K, device="cuda")
    dg = db_ = None
    if gamma is not None:
        dg, db_ = torch.empty(Cc, device="cuda"), torch.empty(Cc, device="cuda")
    from mis_hip import lib
    nb = lib.query("mis_norm_head_workspace_bytes", Nn, Cc, S, int(per_sample), K)
    ops.scratch(nb, "norm").zero_()
    ops.norm_head_bwd(x, dl, dx, per_sample, mean, rstd, gamma, beta, 0.01, w, dw, db, dgamma=dg, dbeta=db_, bits=bits, **drop)
    part = ops.scratch(nb, "norm")[:nb].clone().view(torch.float32)
    out = dict(logits=logits, dx=dx, dw=dw, db=db, partial_sums=part)
    if dg is not None:
        out.update(dgamma=dg, dbeta=db_)
    return out


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("sp", [(4, 4, 8), (6, 6, 12)])
def test_head_with_stored_dropout_bits_equals_head_drawing_them(sp, K):
    ops = _ops()
    Cc = 16
    x = _rand(N, Cc, *sp, seed=41, scale=2.0)
    dl = _rand(N, K, *sp, seed=42)
    w, b = _rand(K, Cc, seed=43, scale=0.5), _rand(K, seed=44)
    st = _state(seed=99)
    S = sp[0] * sp[1] * sp[2]
    for kind, p in itertools.product(("in", "bn"), (0.3, 0.0)):
        per_sample = kind == "in"
        G = N * Cc if per_sample else Cc
        mean, rstd = _rand(G, seed=45, scale=0.3), _rand(G, seed=46).abs() + 0.5
        gamma, beta = (None, None) if per_sample else (_rand(Cc, seed=47) + 1.0, _rand(Cc, seed=48, scale=0.2))
        args = (ops, x, dl, w, b, per_sample, mean, rstd, gamma, beta, K, p, st)
        ref = _head_run(*args, mask=None, bits=None)
        bits = ops.norm_head_bits(x)
        bits.fill_(0x5555)
        got = _head_run(*args, mask=None, bits=bits)
        for k in ref:
            _same(got[k], ref[k], (sp, K, kind, p, k))
        # the words are one keep bit per element: their density is the keep rate, exactly 1 with dropout off
        kept = sum(int(((bits >> i) & 1).sum()) for i in range(64))
        if p == 0.0:
            assert kept == N * S * Cc
        else:
            assert abs(kept / (N * S * Cc) - (1 - p)) < 0.05
            assert (ref["logits"] != _head_run(*args[:-2], 0.0, st, mask=None, bits=None)["logits"]).any()
        # an explicit mask: the buffer is neither written nor read
        g = torch.Generator().manual_seed(50)
        mask = ((torch.rand(N, Cc, *sp, generator=g) >= 0.3).float() / 0.7).cuda()
        ref_m = _head_run(*args[:-2], 0.3, st, mask=mask, bits=None)
        junk = torch.zeros_like(bits)
        got_m = _head_run(*args[:-2], 0.3, st, mask=mask, bits=junk)
        for k in ref_m:
            _same(got_m[k], ref_m[k], (sp, K, kind, "mask", k))
        assert not junk.any()


# ------------------------------------------------------------------------------------------------------ plan level
SWITCHES = ("FUSE_POOL_FWD_3D", "HEAD_DROP_BITS")


def _unet3d_steps(on, use_tape, steps):
    from mis_hip import plan as plan_mod
    from mis_hip.step import MeanTeacherTrainer
    from networks.net_factory_3d import net_factory_3d
    from oracle import filler
    keep = {s: getattr(plan_mod, s) for s in SWITCHES}
    for s in SWITCHES:
        setattr(plan_mod, s, on)
    try:
        torch.manual_seed(5)
        sd0 = {k: v.clone() for k, v in net_factory_3d("unet_3D", 1, 2).state_dict().items()}
        m, e = net_factory_3d("unet_3D", 1, 2), net_factory_3d("unet_3D", 1, 2)
        m.load_state_dict(sd0); e.load_state_dict(sd0)
        vol = filler.image((2, 1, 32, 32, 32), "volume").cuda()
        lab = filler.labels((2, 32, 32, 32), 2, torch.int64).cuda()
        tr = MeanTeacherTrainer(m, e, labeled_bs=1, num_classes=2, cons_start_iter=0, seed=11, iter_num=1500, use_tape=use_tape)
        for _ in range(steps):
            tr.step(vol, lab)
        torch.cuda.synchronize()
        ops_ = [op for p in m._plans.values() for op in p.ops]
        fused = dict(pool=sum(1 for op in ops_ if getattr(op, "fwd_fused", False)),
                     bits=sum(1 for op in ops_ if getattr(op, "_bits", None) is not None))
        assert tr._tape is not None if use_tape else tr._tape is None
        return tr.losses(), m._last[0].out.t.clone(), m.flat_grad.clone(), m.flat_param.clone(), fused
    finally:
        for s in SWITCHES:
            setattr(plan_mod, s, keep[s])


@pytest.mark.parametrize("use_tape", [False, True])
def test_unet3d_step_is_bit_identical_with_and_without_the_handoffs(use_tape):
    """Eager: one forward and backward.  Taped: two eager steps, the recorded one and a replayed one -- four updates, so every
    one of them has to agree exactly for the last to."""
    steps = 4 if use_tape else 1
    l1, y1, g1, p1, f1 = _unet3d_steps(True, use_tape, steps)
    l0, y0, g0, p0, f0 = _unet3d_steps(False, use_tape, steps)
    assert f1 == dict(pool=4, bits=1) and f0 == dict(pool=0, bits=0), (f1, f0)
    assert l1 == l0, (l1, l0)
    _same(y1, y0, "logits")
    _same(g1, g0, "flat gradient")
    _same(p1, p0, "parameters")
