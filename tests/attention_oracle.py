"""float64 reference of the attention kernels (csrc/attention.hip + attention_impl.inc: SwinUnet's 2-D window attention, windows
7 and 8; csrc/attention_full.hip: UNETR's full attention; csrc/swin3d.hip: SwinUNETR's 3-D window attention) and the case
matrix of tests/test_attention_edges_gpu.py.

CPU only, pure torch.  The three operators are one operation on different token groupings:

    out = softmax((q * scale) k^T + table[index] + mask) v        per (group of n tokens, head)

  win2d   qkv [B*H*W][3*nH*32] in natural token order; a group is a (shifted) ws x ws window, found through the cyclic shift and
          the window partition; table [(2 ws - 1)^2][nH]; mask = -100 ADDED (not an exclusion) where two tokens of a window lie
          in different regions of the shifted image
  full    qkv [B*N][3*nH*64]; a group is a sample; no table, no mask
  win3d   qkv [BW*n][3*nH*16] already in window order; table [13^3][nH] through the [:n, :n] block of the 7^3 window's
          relative-position index; the same additive mask from oracle/swinunetr.py's region ids

Every case exists four times:

  reference64(c)   out, dqkv, dtable through torch's matmul / softmax and autograd in float64, the grouping through torch.roll and
                   view / permute as the networks' own code does it (tests/test_token_kernels_gpu.py::_ref_window_attention,
                   tests/test_swin3d_gpu.py::_attn_ref);
  plain(c)         the same as an explicit loop over groups and heads: token rows, region codes and table indices from integer
                   formulas, max / exp / sum spelled out, and the backward by hand (dV = P^T dO, dP = dO V^T,
                   dS = P (dP - delta), dQ = scale dS K, dK = dS^T (scale Q), dtable = index_add of dS);
                   tests/test_attention_oracle_cpu.py holds the two float64 forms to each other;
  reference32(c)   reference64's operators in float32 on one thread: yardstick (a);
  plain32(c)       plain() in float32 in the order the kernels use: scores, maximum, exp, sum, normalisation (3-D: after the
                   P V product, by 1 / l), and the backward recomputing P from the kept (max, sum), delta = sum P dP (3-D:
                   dO . O from the rounded output), the table gradient as one fp32 partial per (group, head) summed over the
                   groups in double: yardstick (b).
  e32 = the larger of the two distances to reference64.  It plays the role conv_oracle.winograd32 plays for the convolutions.

Tensors: out [T][C], dqkv [T][3 C], dtable [rows][nH]; measure(got, ref, 1) (conv_oracle.measure): ``max`` = the worst column's
largest |error| over that column's largest |reference| (column = channel for out and dqkv, head for dtable), ``rms`` over the
whole tensor, ``zero_ok`` = a column whose reference is exactly zero is exactly zero.

Input classes (q / k / v / table / dout), generated in float64 from a seed derived from the case's name and rounded to fp32 once:
  uniform        U(-1.5, 1.5) (full attention: 0.7) / table U(-0.5, 0.5) / dout U(-1, 1): what the older tests feed;
  peaked         q, k = sqrt(10) N(0, 1): logit standard deviation 10, rows near one-hot; v and dout N(0, 1) times channel scales
                 over three decades (a permuted logspace(-3, 0)); one v channel and one dout channel per head exactly zero; rows
                 1 and T - 2 of q exactly zero (their softmax is the softmax of the table alone); table N(0, 1);
  offset         q, k = 4 + N(0, 1): logits around 16 * hd * scale (90 at head dimension 32) -- exp overflows fp32 without
                 the maximum; v = (4 + N(0, 1)) * channel scale; dout as peaked; table 0.5 N(0, 1);
  mask_competes  (shifted cases) uniform, plus -a s u on q and +a s u on k in every head: s = (-1)^(sum of the per-axis region
                 codes) of the token, u the constant unit vector, a^2 * scale = 50.  Tokens of adjacent regions then sit 100
                 above same-region pairs before the mask and level with them after it: an exclusion instead of the
                 addition changes out and dqkv by O(1).
"""
import functools
import zlib

import torch

from oracle_kit import one_thread as _one_thread
from conv_oracle import ceil2, measure          # noqa: F401  (re-exported: the same measures as the convolutions)

F64, F32 = torch.float64, torch.float32
KINDS = ("out", "dqkv", "dtable")
MEASURES = ("max", "rms")
CLASSES = ("uniform", "peaked", "offset", "mask_competes")
HEAD_DIM = {"win2d": 32, "full": 64, "win3d": 16}
MASK_GAP = 50.0          # a^2 * scale of mask_competes


def kinds_of(c):
    return KINDS[:2] if c["family"] == "full" else KINDS


# ---------------------------------------------------------------------------------------------------------------------
# geometry: sizes, and the grouping twice (through torch's roll / view / permute; through integer formulas)
# ---------------------------------------------------------------------------------------------------------------------
def sizes(spec):
    """What follows from a matrix entry without any tensor."""
    fam = spec["family"]
    hd = HEAD_DIM[fam]
    s = dict(hd=hd, scale=hd ** -0.5)
    if fam == "win2d":
        B, H, W, nH, shift, ws = spec["shape"]
        s.update(B=B, nH=nH, n=ws * ws, nW=(H // ws) * (W // ws), shifted=shift > 0, rows=(2 * ws - 1) ** 2)
    elif fam == "full":
        B, N, nH = spec["shape"]
        s.update(B=B, nH=nH, n=N, nW=1, shifted=False, rows=0)
    else:
        from oracle.swinunetr import window_geometry
        B, dims, nH, shifted = spec["shape"]
        win, shift = window_geometry(dims)
        assert all(shift) or not any(shift)
        if not shifted:
            shift = (0, 0, 0)
        pdims = tuple(-(-d // w) * w for d, w in zip(dims, win))
        s.update(B=B, nH=nH, n=win[0] * win[1] * win[2], nW=(pdims[0] // win[0]) * (pdims[1] // win[1]) * (pdims[2] // win[2]),
                 shifted=any(shift), rows=13 ** 3, win=win, shift=shift, pdims=pdims)
    s["G"] = s["B"] * s["nW"]
    s["T"] = s["G"] * s["n"]
    s["C"] = s["nH"] * hd
    return s


def torch_geometry(spec):
    """(perm [G][n] token row of every group member or None, index [n][n] or None, region [nW][n] or None) the way the
    networks' code finds them: torch.roll + window partition of the token numbers, the img_mask slices, meshgrid."""
    fam, z = spec["family"], sizes(spec)
    if fam == "full":
        return None, None, None
    if fam == "win3d":
        from oracle.swinunetr import region_ids, relative_position_index
        n = z["n"]
        region = region_ids(z["pdims"], z["win"], z["shift"]).long() if z["shifted"] else None
        return None, relative_position_index()[:n, :n].contiguous(), region
    B, H, W, nH, shift, ws = spec["shape"]
    n = ws * ws
    ar = torch.arange(B * H * W).view(B, H, W)
    if shift:
        ar = torch.roll(ar, shifts=(-shift, -shift), dims=(1, 2))
    perm = ar.view(B, H // ws, ws, W // ws, ws).permute(0, 1, 3, 2, 4).reshape(-1, n)
    coords = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0) + ws - 1
    index = rel[:, :, 0] * (2 * ws - 1) + rel[:, :, 1]
    region = None
    if shift:
        img = torch.zeros(1, H, W, 1)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for ws_ in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img[:, hs, ws_, :] = cnt
                cnt += 1
        region = img.view(1, H // ws, ws, W // ws, ws, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, n).long()
    return perm, index, region


def _code(p, L, ws, shift):
    """Region code of position p of the SHIFTED axis of length L: 0 below L - ws, 1 up to L - shift, 2 beyond."""
    return (p >= L - ws).long() + (p >= L - shift).long()


def plain_geometry(spec):
    """The same three, and the per-axis region code sum [nW][n] (or None), from integer formulas alone."""
    fam, z = spec["family"], sizes(spec)
    if fam == "full":
        return None, None, None, None
    t = torch.arange(z["n"])
    w = torch.arange(z["nW"])[:, None]
    if fam == "win2d":
        B, H, W, nH, shift, ws = spec["shape"]
        nWx = W // ws
        iy, ix = t // ws, t % ws
        sy, sx = (w // nWx) * ws + iy, (w % nWx) * ws + ix                       # shifted-image coordinates [nW][n]
        b = torch.arange(B)[:, None, None]
        perm = ((b * H + (sy + shift) % H) * W + (sx + shift) % W).reshape(-1, z["n"])
        index = (iy[:, None] - iy[None, :] + ws - 1) * (2 * ws - 1) + (ix[:, None] - ix[None, :] + ws - 1)
        if not shift:
            return perm, index, None, None
        cy, cx = _code(sy, H, ws, shift), _code(sx, W, ws, shift)
        return perm, index, cy * 3 + cx, cy + cx
    win, shift, pd = z["win"], z["shift"], z["pdims"]
    tz, ty, tx = t // 49, (t // 7) % 7, t % 7                                    # the [:n, :n] block of the 7^3 window's index
    index = (tz[:, None] - tz[None, :] + 6) * 169 + (ty[:, None] - ty[None, :] + 6) * 13 + (tx[:, None] - tx[None, :] + 6)
    if not z["shifted"]:
        return None, index, None, None
    nwh, nww = pd[1] // win[1], pd[2] // win[2]
    pz = (w // (nwh * nww)) * win[0] + t // (win[1] * win[2])
    py = ((w // nww) % nwh) * win[1] + (t // win[2]) % win[1]
    px = (w % nww) * win[2] + t % win[2]
    cz, cy, cx = (_code(p, pd[a], win[a], shift[a]) for a, p in enumerate((pz, py, px)))
    return None, index, cz * 9 + cy * 3 + cx, cz + cy + cx


# ---------------------------------------------------------------------------------------------------------------------
# the operation through torch's operators and autograd (float64 / float32)
# ---------------------------------------------------------------------------------------------------------------------
def reference_torch(c, dtype, hard_mask=False):
    """out, dqkv, dtable in ``dtype``.  hard_mask: cross-region pairs are EXCLUDED (-inf) instead of lowered by 100 -- what the
    reference does NOT do; only tests/test_attention_oracle_cpu.py asks for it, to show which inputs tell the two apart."""
    z = sizes(c)
    perm, index, region = torch_geometry(c)
    G, n, nH, hd, C, nW = z["G"], z["n"], z["nH"], z["hd"], z["C"], z["nW"]
    qkv = c["qkv"].to(dtype, copy=True).requires_grad_(True)
    table = c["table"].to(dtype, copy=True).requires_grad_(True) if c["table"] is not None else None
    x = qkv if perm is None else qkv[perm.reshape(-1)]
    xw = x.reshape(G, n, 3, nH, hd).permute(2, 0, 3, 1, 4)
    q, k, v = xw[0] * z["scale"], xw[1], xw[2]
    attn = q @ k.transpose(-2, -1)
    if table is not None:
        attn = attn + table[index.reshape(-1)].view(n, n, nH).permute(2, 0, 1).unsqueeze(0)
    if region is not None:
        am = region.unsqueeze(1) - region.unsqueeze(2)
        am = torch.zeros(am.shape, dtype=dtype).masked_fill(am != 0, float("-inf") if hard_mask else -100.0)
        attn = (attn.view(G // nW, nW, nH, n, n) + am.unsqueeze(1).unsqueeze(0)).view(-1, nH, n, n)
    attn = attn.softmax(-1)
    o = (attn @ v).transpose(1, 2).reshape(G * n, C)
    if perm is not None:
        inv = torch.empty(G * n, dtype=torch.long)
        inv[perm.reshape(-1)] = torch.arange(G * n)
        o = o[inv]
    o.backward(c["dout"].to(dtype))
    r = {"out": o.detach().double(), "dqkv": qkv.grad.double()}
    if table is not None:
        r["dtable"] = table.grad.double()
    return r


def reference64(c):
    return reference_torch(c, F64)


def reference32(c):
    return _one_thread(reference_torch, c, F32)


# ---------------------------------------------------------------------------------------------------------------------
# the operation as a loop over groups and heads, the backward by hand
# ---------------------------------------------------------------------------------------------------------------------
def plain(c, dtype=F64, kernel_order=False):
    """kernel_order: the order of operations the kernels use where it differs from the textbook's (module docstring)."""
    z = sizes(c)
    perm, index, region, _ = plain_geometry(c)
    G, n, nH, hd, C, nW, scale = z["G"], z["n"], z["nH"], z["hd"], z["C"], z["nW"], z["scale"]
    late = kernel_order and c["family"] == "win3d"
    qkv, dout = c["qkv"].to(dtype), c["dout"].to(dtype)
    table = c["table"].to(dtype) if c["table"] is not None else None
    out, dqkv = torch.zeros(G * n, C, dtype=dtype), torch.zeros(G * n, 3 * C, dtype=dtype)
    dtable = torch.zeros(z["rows"], nH, dtype=F64) if table is not None else None
    flat = index.reshape(-1) if index is not None else None
    for g in range(G):
        rows = perm[g] if perm is not None else torch.arange(g * n, (g + 1) * n)
        x, do = qkv[rows], dout[rows]
        pen = None
        if region is not None:
            r = region[g % nW]
            pen = torch.where(r[:, None] != r[None, :], -100.0, 0.0).to(dtype)
        dx = torch.zeros(n, 3 * C, dtype=dtype)
        og = torch.zeros(n, C, dtype=dtype)
        for h in range(nH):
            col = slice(h * hd, (h + 1) * hd)
            q, k, v, d = x[:, col] * scale, x[:, C + h * hd:C + (h + 1) * hd], x[:, 2 * C + h * hd:2 * C + (h + 1) * hd], do[:, col]
            s = q @ k.t()
            if table is not None:
                s = s + table[:, h][index]
            if pen is not None:
                s = s + pen
            m = s.max(1, keepdim=True).values
            e = torch.exp(s - m)
            l = e.sum(1, keepdim=True)
            if late:
                inv = 1.0 / l
                o = (e @ v) * inv
                p = torch.exp(s - m) * inv                 # the backward's P, from the kept (max, sum)
            elif kernel_order:
                p = e * (1.0 / l)
                o = p @ v
                if c["family"] == "full":
                    p = torch.exp(s - m) / l
            else:
                p = e / l
                o = p @ v
            dp = d @ v.t()
            delta = (d * o).sum(1, keepdim=True) if late else (p * dp).sum(1, keepdim=True)
            ds = p * (dp - delta)
            og[:, col] = o
            dx[:, col] = (ds @ k) * scale
            dx[:, C + h * hd:C + (h + 1) * hd] = ds.t() @ q
            dx[:, 2 * C + h * hd:2 * C + (h + 1) * hd] = p.t() @ d
            if dtable is not None:        # one partial table per (group, head) in ``dtype``, summed over the groups in double
                dtable[:, h] += torch.zeros(z["rows"], dtype=dtype).index_add_(0, flat, ds.reshape(-1)).double()
        out[rows], dqkv[rows] = og, dx
    r = {"out": out.double(), "dqkv": dqkv.double()}
    if dtable is not None:
        r["dtable"] = dtable.double()
    return r


def plain32(c):
    return _one_thread(plain, c, F32, True)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(zlib.crc32(seed.encode()))


def channel_scales(C, g):
    """A permuted logspace(-3, 0) over the C channels."""
    return torch.logspace(-3, 0, C, dtype=F64)[torch.randperm(C, generator=g)]


def zero_channels(z):
    """(v channels, dout channels) that are exactly zero in the peaked and offset classes: one per head each."""
    hd = z["hd"]
    return ([h * hd + (5 * h + 3) % hd for h in range(z["nH"])], [h * hd + (7 * h + 11) % hd for h in range(z["nH"])])


def token_signs(spec):
    """(-1)^(sum of the per-axis region codes) per row of qkv (natural token order in 2-D, window order in 3-D)."""
    z = sizes(spec)
    perm, _, _, codes = plain_geometry(spec)
    s = (1 - 2 * (codes % 2)).to(F64).repeat(z["B"], 1).reshape(-1)            # [G * n] in window order
    if perm is None:
        return s
    nat = torch.empty_like(s)
    nat[perm.reshape(-1)] = s
    return nat


def make_case(cid, spec, cls):
    z = sizes(spec)
    T, C, hd = z["T"], z["C"], z["hd"]
    g = _gen(f"{cid}/{cls}")
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=F64)
    un = lambda *shape: torch.rand(*shape, generator=g, dtype=F64) * 2 - 1
    if cls in ("uniform", "mask_competes"):
        qkv = un(T, 3 * C) * (0.7 if spec["family"] == "full" else 1.5)
        table, dout = un(max(z["rows"], 1), z["nH"]) * 0.5, un(T, C)
        if cls == "mask_competes":
            assert z["shifted"], cid
            a = (MASK_GAP / z["scale"]) ** 0.5 / hd ** 0.5                     # a * u, u = 1 / sqrt(hd) in every dimension
            s = token_signs(spec)[:, None]
            qkv[:, :C] -= a * s
            qkv[:, C:2 * C] += a * s
    else:
        sv, sd = channel_scales(C, g), channel_scales(C, g)
        zv, zd = zero_channels(z)
        sv[zv], sd[zd] = 0.0, 0.0
        if cls == "peaked":
            qkv = torch.cat((rn(T, 2 * C) * 10 ** 0.5, rn(T, C) * sv), 1)
            table = rn(max(z["rows"], 1), z["nH"])
            if T >= 4:
                qkv[[1, T - 2], :C] = 0.0
        elif cls == "offset":
            qkv = torch.cat((4 + rn(T, 2 * C), (4 + rn(T, C)) * sv), 1)
            table = rn(max(z["rows"], 1), z["nH"]) * 0.5
        else:
            raise KeyError(cls)
        dout = rn(T, C) * sd
    return dict(spec, id=cid, cls=cls, qkv=qkv.float(), dout=dout.float(), table=table.float() if z["rows"] else None)


# ---------------------------------------------------------------------------------------------------------------------
# the case matrix: the smallest shapes that reach each code path
#   win2d (B, H, W, nH, shift, ws)    full (B, N, nH)    win3d (B, dims, nH, shifted)
# groups: what tests/test_attention_edges_gpu.py runs a case as -- "win2d" under both precision masks, "fallback" as a column
# slice of a buffer beyond 2^31 bytes (the vector-pipe kernels through their real condition), "valu" in a child process with
# MIS_ATTN_VALU set (the chunked backward), "full", "win3d"
# ---------------------------------------------------------------------------------------------------------------------
ALL = CLASSES
NOMASK = CLASSES[:3]
ONE = ("peaked",)
SPECS = {}


def _spec(groups, cid, family, shape, classes=ONE):
    assert cid not in SPECS, cid
    SPECS[cid] = dict(groups=groups, family=family, shape=shape, classes=classes)


_spec(("win2d",), "w7-1x7x7x3-s0", "win2d", (1, 7, 7, 3, 0, 7))                    # 3 units: a ragged group of 4 waves
_spec(("win2d", "fallback"), "w7-2x14x14x3-s3", "win2d", (2, 14, 14, 3, 3, 7), ALL)
_spec(("win2d",), "w7-3x14x21x2-s3", "win2d", (3, 14, 21, 2, 3, 7))
_spec(("win2d",), "w8-1x8x8x6-s0", "win2d", (1, 8, 8, 6, 0, 8))
_spec(("win2d",), "w8-1x16x24x2-s4", "win2d", (1, 16, 24, 2, 4, 8), ALL)
_spec(("win2d",), "w7-1x14x14x1-s1", "win2d", (1, 14, 14, 1, 1, 7))                # geometry_ok accepts every 0 <= shift < ws
_spec(("win2d",), "w7-1x14x14x1-s6", "win2d", (1, 14, 14, 1, 6, 7))
_spec(("fallback",), "w8-1x16x16x3-s4", "win2d", (1, 16, 16, 3, 4, 8))
_spec(("valu",), "w7-23x28x28x3-s3", "win2d", (23, 28, 28, 3, 3, 7))               # 1104 units: bwd_chunk = 2, 23 = 11 * 2 + 1
_spec(("full",), "full-1x1x1", "full", (1, 1, 1))
_spec(("full",), "full-1x64x1", "full", (1, 64, 1))
_spec(("full",), "full-1x65x2", "full", (1, 65, 2))
_spec(("full",), "full-3x27x2", "full", (3, 27, 2))
_spec(("full",), "full-2x70x3", "full", (2, 70, 3), NOMASK)
_spec(("full",), "full-1x256x1", "full", (1, 256, 1))
_spec(("full",), "full-2x216x12", "full", (2, 216, 12))
_spec(("full",), "full-43x9x12", "full", (43, 9, 12))                              # B * nH >= 512: one row chunk, rows > N
_spec(("win3d",), "w3d-2x4x4x4x6", "win3d", (2, (4, 4, 4), 6, False))
_spec(("win3d",), "w3d-2x8x8x8x3-s", "win3d", (2, (8, 8, 8), 3, True), ALL)
_spec(("win3d",), "w3d-1x9x8x10x3-s", "win3d", (1, (9, 8, 10), 3, True))           # padded tokens are ordinary keys
_spec(("win3d",), "w3d-1x16x16x16x6-s", "win3d", (1, (16, 16, 16), 6, True))


def spec_of(name):
    return SPECS[name.split("/")[0]]


def names(group=None):
    """Case names ``id/class``.  A group beyond a case's first runs its primary class only."""
    out = []
    for cid, s in SPECS.items():
        if group is None or group == s["groups"][0]:
            out += [f"{cid}/{cls}" for cls in s["classes"]]
        elif group in s["groups"]:
            out.append(f"{cid}/peaked")
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    cid, cls = name.split("/")
    return make_case(cid, SPECS[cid], cls)


@functools.lru_cache(maxsize=None)
def references(name):
    """(float64 reference, error of reference32, error of plain32) of a matrix case; errors: {kind: {measure: value}}.
    Computed once, never modified."""
    c = case(name)
    r64 = reference64(c)
    r32, p32 = reference32(c), plain32(c)
    return r64, {k: measure(r32[k], r64[k]) for k in r64}, {k: measure(p32[k], r64[k]) for k in r64}


def yardstick(name, kind, m):
    """The e32 the rule uses for one tensor and measure: the larger of the two fp32 forms' errors."""
    _, ea, eb = references(name)
    return max(ea[kind][m], eb[kind][m])
