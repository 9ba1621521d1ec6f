"""The Winograd forward's two LDS-traffic changes leave every result bit where it was (csrc/conv_wino.hip).

* resident filter: a 16 -> 16 launch at the 96^3 level (variant 0) fetches its transformed filter once per workgroup instead
  of once per box (ResidentFilter), in the forward and in the data gradient with the norm-backward partials;
* variant 3 (6 x 6 x 12 boxes, the 12^3 level) fetches its halo rows as 16-byte groups instead of single dwords.

Both change only how bytes reach LDS, so the outputs and the statistics partials are held to the bits the parent commit
produced: tests/golden/wino_resident_digests.json holds the SHA-256 of every result array of every case below, written by
scripts/gen_golden_wino_resident.py on the commit before the change (the arrays themselves are up to 7 MB; a digest of the
bytes is equal exactly when torch.equal holds).  Where a path without the new mode still exists -- the 16 -> 32 launch
streams its filter, and each of its 16-channel blocks is the 16 -> 16 convolution on that weight slice -- the output is also
compared with torch.equal against it.

Replaces nothing new: nn.Conv3d(k=3, pad=1) of UnetConv3 / UnetUp3_CT (reference code/networks/utils.py:99-123)."""
import hashlib
import json
import os
import zlib

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wino_resident_digests.json")
K3 = (3, 3, 3)


def _rand(cid, what, *shape, scale=1.0):
    g = torch.Generator().manual_seed(zlib.crc32(f"{cid}/{what}".encode()))
    return ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float()


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


# resident filter: (N, D, H, W), Cin = Cout = 16.  One box; 8 boxes over 8 workgroups, two images; 384 boxes over 256 workgroups:
# workgroups that walk two boxes (the filter has to survive the second box's DMAs), runs that end at an image boundary
RF_GEOMETRIES = {"one-box": (1, 4, 4, 32), "eight-boxes": (2, 8, 8, 32), "walk": (3, 32, 32, 64)}
# variant 3: (D, H, W) x Cin x Cout x N; Cin = 128 with few boxes is cut into contraction slices (N = 1 on one 6 x 6 x 12 volume: 4)
V3_CASES = {f"v3-{d}x{h}x12-ci{ci}-co{co}-n{n}": (n, ci, co, d, h, 12)
            for d, h in ((6, 6), (12, 12)) for ci in (32, 128) for co in (16, 128) for n in (1, 8)}


def run_resident_filter(ops, cid):
    """{name: result} of the forward (with bias; with and without statistics) and of the data gradient with the norm partials."""
    N, D, H, W = RF_GEOMETRIES[cid]
    C = 16
    x, w, b = _rand(cid, "x", N, C, D, H, W).cuda(), _rand(cid, "w", C, C, 3, 3, 3, scale=0.2).cuda(), _rand(cid, "b", C).cuda()
    T = ops.conv_stat_tiles(N, C, C, D, H, W, K3, wino=0)
    out = {}
    y = torch.full((N, C, D, H, W), float("nan"), device="cuda")
    part = torch.full((C * N * T, 2), float("nan"), device="cuda")
    ops.conv_fwd(x, ops.conv_pack(w, 4), b, y, C, C, K3, stat=(part, T, C * T), wino=0)
    out["y_stat"], out["stat"] = y, part
    y2 = torch.full_like(y, float("nan"))
    ops.conv_fwd(x, ops.conv_pack(w, 4), b, y2, C, C, K3, wino=0)
    out["y"] = y2
    y3 = torch.full_like(y, float("nan"))
    ops.conv_fwd(x, ops.conv_pack(w, 4), None, y3, C, C, K3, wino=0)
    out["y_nobias"] = y3
    # the NB entry: dy -> da with (sum dz, sum dz * xn) per run of boxes; thresholds per (n, channel)
    xn, thr = _rand(cid, "xn", N, C, D, H, W).cuda(), _rand(cid, "thr", N * C, scale=0.3).cuda()
    da = torch.full((N, C, D, H, W), float("nan"), device="cuda")
    npart = torch.full((N * C * T, 2), float("nan"), device="cuda")
    assert ops.conv_dgrad_norm(x, ops.conv_pack(w, 5), da, C, C, xn, thr, 0.01, npart, 0) == T
    out["da"], out["norm_part"] = da, npart
    torch.cuda.synchronize()
    return out


def run_variant3(ops, cid):
    N, Cin, Cout, D, H, W = V3_CASES[cid]
    x, w, b = _rand(cid, "x", N, Cin, D, H, W).cuda(), _rand(cid, "w", Cout, Cin, 3, 3, 3, scale=0.1).cuda(), _rand(cid, "b", Cout).cuda()
    wp = ops.conv_pack(w, 4)
    T = ops.conv_stat_tiles(N, Cin, Cout, D, H, W, K3, wino=3)
    y = torch.full((N, Cout, D, H, W), float("nan"), device="cuda")
    part = torch.full((Cout * N * T, 2), float("nan"), device="cuda")
    ops.conv_fwd(x, wp, b, y, Cin, Cout, K3, stat=(part, T, Cout * T), wino=3)
    y2 = torch.full_like(y, float("nan"))
    ops.conv_fwd(x, wp, b, y2, Cin, Cout, K3, wino=3)
    torch.cuda.synchronize()
    return {"y_stat": y, "stat": part, "y": y2}


def run_case(ops, cid):
    return run_resident_filter(ops, cid) if cid in RF_GEOMETRIES else run_variant3(ops, cid)


def wino_launch(variant, Cin, Cout):
    """MIS_WINO_LAUNCH of include/mis_hip.h."""
    return variant | Cin << 4 | Cout << 16


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _ops():
    from mis_hip import ops
    return ops


def _check(cid, out):
    want = _golden()[cid]
    assert set(want) == set(out), (cid, sorted(want), sorted(out))
    for name, t in out.items():
        assert bool(torch.isfinite(t).all()), (cid, name, "not finite")
        assert digest(t) == want[name], (cid, name, "differs from the bits of the commit before the change")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(RF_GEOMETRIES))
def test_resident_filter_bits(cid):
    from mis_hip import lib
    ops = _ops()
    N, D, H, W = RF_GEOMETRIES[cid]
    resident = lambda Cout: "ResidentFilter<" in lib.kernel_name("mis_conv3d_wino_kernel_name", wino_launch(0, 16, Cout))
    assert ops.conv_wino_select(N, 16, 16, D, H, W, K3) == 0 and resident(16)
    out = run_resident_filter(ops, cid)
    assert torch.equal(out["y"], out["y_stat"])
    _check(cid, out)
    # the streamed path that still exists: 16 -> 32 (two channel groups); its blocks are the 16 -> 16 convolutions on the slices
    assert not resident(32)
    x, b = _rand(cid, "x", N, 16, D, H, W).cuda(), _rand(cid, "b", 16).cuda()
    w = torch.cat([_rand(cid, "w", 16, 16, 3, 3, 3, scale=0.2), _rand(cid, "w-other", 16, 16, 3, 3, 3, scale=0.2)]).cuda()
    y32 = torch.full((N, 32, D, H, W), float("nan"), device="cuda")
    ops.conv_fwd(x, ops.conv_pack(w, 4), torch.cat([b, b]), y32, 16, 32, K3, wino=0)
    assert torch.equal(y32[:, :16], out["y"])
    # data gradient: the plain launch on dy with the transposed filter, 32 output channels (streamed), first block
    da32 = torch.full((N, 32, D, H, W), float("nan"), device="cuda")
    wd = torch.cat([_rand(cid, "w", 16, 16, 3, 3, 3, scale=0.2), _rand(cid, "w-other", 16, 16, 3, 3, 3, scale=0.2)], dim=1).cuda()
    ops.conv_fwd(x, ops.conv_pack(wd, 5), None, da32, 16, 32, K3, wino=0)
    assert torch.equal(da32[:, :16], out["da"])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(V3_CASES))
def test_variant3_sixteen_byte_rows_bits(cid):
    ops = _ops()
    out = run_variant3(ops, cid)
    assert torch.equal(out["y"], out["y_stat"])
    _check(cid, out)


def test_split_cases_are_split():
    """The variant-3 cases with few boxes and 128 input channels run the split form (host-side query)."""
    from mis_hip import lib
    L = lib.load()
    assert L.mis_conv3d_wino_fwd_splits(1, 128, 16, 6, 6, 12, 3) == 4 and L.mis_conv3d_wino_fwd_splits(1, 128, 128, 12, 12, 12, 3) == 4
    assert L.mis_conv3d_wino_fwd_splits(8, 128, 128, 12, 12, 12, 3) == 1 and L.mis_conv3d_wino_fwd_splits(1, 32, 16, 6, 6, 12, 3) == 1


def test_filter_mode_of_the_network_layers():
    """Which launches keep their filter resident, for the 3x3x3 layer shapes of unet_3D (16 .. 256 filters), V-Net and UNETR's
    decoder at 4 + 4 volumes of 96^3: only 16 -> 16 on variant 0 (unet_3D conv1.conv2 and up_concat1.conv2, V-Net's and UNETR's
    16-channel 96^3 layers; forward and data gradient); every other launch streams its filter, under the name it had."""
    from mis_hip import lib
    L = lib.load()
    name = lambda v, Cin=0, Cout=0: lib.kernel_name("mis_conv3d_wino_kernel_name", wino_launch(v, Cin, Cout))
    v0 = "WinoCfg<1, 1, 16, 2, 2, 1, 1, 4, 0, 0>"
    # (Cin, Cout, S): unet_3D encoder / decoder (forward and data-gradient directions), V-Net stages, UNETR decoder blocks
    unet3d = [(16, 16, 96), (48, 16, 96), (16, 48, 96), (16, 32, 48), (32, 16, 48), (32, 32, 48), (96, 32, 48), (32, 96, 48),
              (32, 64, 24), (64, 32, 24), (64, 64, 24), (192, 64, 24), (64, 192, 24), (64, 128, 12), (128, 64, 12), (128, 128, 12),
              (384, 128, 12), (128, 384, 12), (128, 256, 6), (256, 128, 6), (256, 256, 6)]
    vnet = [(16, 16, 96), (32, 32, 48), (64, 64, 24), (128, 128, 12), (256, 256, 6)]
    unetr = [(16, 16, 96), (32, 16, 96), (16, 32, 96), (32, 32, 48), (64, 32, 48), (64, 64, 24), (128, 64, 24), (128, 128, 12)]
    seen = set()
    for Cin, Cout, S in unet3d + vnet + unetr:
        for N in (4, 8):
            v = L.mis_conv3d_wino_select(N, Cin, Cout, S, S, S)
            if v < 0:
                continue
            kn = name(v, Cin, Cout)
            resident = v == 0 and Cin == 16 and Cout == 16
            assert kn.startswith("wino_fwd_kernel<") and kn.endswith(", false>")
            assert kn == (f"wino_fwd_kernel<ResidentFilter<{v0} >, false>" if resident else name(v)), (Cin, Cout, S, v, kn)
            seen.add((v, resident))
    assert seen == {(0, True), (0, False), (1, False), (2, False), (3, False)}
    # the rule is the filter's size alone: four chunks of input channels, one block of 16 output channels, variant 0
    assert "ResidentFilter" not in name(1, 16, 16) and "ResidentFilter" not in name(0, 24, 16) and "ResidentFilter" not in name(0, 16, 32)
    assert name(0) == f"wino_fwd_kernel<{v0}, false>" and name(3) == "wino_fwd_kernel<WinoCfg<3, 3, 6, 1, 1, 1, 1, 4, 1, 1>, false>"
