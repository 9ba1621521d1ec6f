"""float64 reference of the Linear path of the transformer nets -- the matrix-pipe GEMMs of csrc/gemm.hip (NT: forward and dX,
TN: dW and db, their fused epilogues, the pixel-shuffle store and the fused LayerNorm tails) and the LayerNorm, head, GELU and
column-sum kernels of csrc/token_ops.hip -- and the case matrix of tests/test_token_edges_gpu.py.

CPU only, pure torch; the library is asked (host functions, no GPU) only for what the plain fp32 form must follow: the k slices of
a split contraction and the row slabs of the column reductions.

Operations (``op`` of a case) and their tensors:
  nt       C = A W^T + bias [M][N]; with ``ep``: gelu = gelu(C), gelu_bwd = (A W^T) gelu'(E1), res = E1 + s[row // rps] C
  tn       dW = dY^T X [Cout][Cin], db = dY.sum(0)                                   (nn.Linear's parameter gradients)
  resln    X = E1 + s[row // rps] (A W^T + bias), Y = LayerNorm(X) g + b, mean, rstd  (mis_gemm_nt_residual_ln, N = 96)
  expand   tok = pixel shuffle of x W^T [B H P W P][c]; with ``ln``: mean, rstd of LayerNorm(tok), logits = head(LayerNorm(tok))
  ln       y, mean, rstd, dx, dgamma, dbeta of nn.LayerNorm(C)
  lnhead   logits [B][NC][S] = head(LayerNorm(x)), mean, rstd, dx, dgamma_h, dbeta_h, dw   (the head's dy = W^T dlogits is what it
           is: its affine gradients are sums that do cancel, so they are a kind of their own, ``hsum``, beside ``sum``)
  head     logits, dx, dw of the bias-free 1x1 output convolution
  colsum   sum = x.sum(0)
GELU (exact erf form) has its own grid and references at the end of the file.

Every case exists as:
  reference64(c)   matmul, layer_norm, gelu and autograd of torch in float64;
  loop64(c)        (small cases) the same as explicit float64 loops over k / over rows, backward by hand;
                   tests/test_token_oracle_cpu.py holds the two to each other;
  reference32(c)   reference64's operators in fp32 on one thread: yardstick (a);
  plain32(c)       fp32 in the kernels' order: yardstick (b).  GEMM: fp32 products in ONE sequential chain over k -- for a split
                   contraction one chain per k slice, the slices summed in gemm_reduce_kernel's order (8 lanes take slices
                   kl, kl + 8, ..., then lane 0 adds the other seven in turn); the slice count comes from
                   mis_gemm_workspace_bytes / mis_gemm_nt_split_workspace_bytes / mis_gemm_dw_workspace_bytes and the slice
                   length is that count's share of K rounded up to the k-step of 32.  LayerNorm: two-pass mean, centred sum of
                   squares, 1 / sqrtf; the backward by hand; the affine gradients as one fp32 partial per row slab
                   (mis_colreduce_slabs) summed in double.  The head forms reuse the two-pass LayerNorm under fp32 autograd.
  e32 = the larger of the two distances to reference64 (yardstick()).
  bf16x3(c, drop)  the GEMM tensor of the case through the truncating split x = h + m + l (8 + 8 + 8 bits) of both operands and
                   the six piece products hh + hm + mh + hl + lh + mm, every product and sum in float64: the SCHEME restated, not
                   the device code.  ``drop`` leaves one piece product out (A's piece first: "hl" = a.h * b.l).  It exists to
                   show on the CPU that the gate sees a lost third-order product (tests/test_token_oracle_cpu.py).

Measures (conv_oracle.measure): ``max`` = the worst column's largest |error| over that column's largest |reference|, ``rms`` over
the whole tensor, ``zero_ok`` = a column whose reference is exactly zero is exactly zero.  Column = output channel for C, X, tok,
y, Y, dx, logits (class); row of dW for dW / dw; every element its own column for db, dgamma, dbeta, sum.  mean / rstd follow the
``stat`` rule of tests/test_norm_edges_gpu.py: mean against the tensor's largest |mean|, rstd each row on its own scale; the
LayerNorms here are two-pass on the data itself (no fp32 partials of a one-pass variance), so no conditioning factor applies.

Input classes, generated in float64 from a seed derived from the case's name and rounded to fp32 once:
  uniform      A, x U(-1, 1) (LayerNorm: U(-2, 2) + 0.5); W U(-1, 1) / sqrt(K); bias U(-1, 1): what the older tests feed;
  act_scaled   A is an activation: relu(N(0, 1)) (half of it exactly zero, the rest non-negative) times K-channel scales from a
               permuted logspace(-3, 0), one K channel exactly zero; W's rows N(0, 1) / sqrt(K) times a permuted logspace(-3, 0)
               along N, one output channel of W and its bias exactly zero (so is that column of C); dY likewise over its columns.
               LayerNorm: x and gamma with channel scales over three decades, one channel of gamma and beta exactly zero;
  offset       A = 4 + N(0, 1).  LayerNorm: x = row scale * (100 + N(0, 1)): row mean = 100 std, row scales cycle through
               logspace(-3, 3) (eps dominates the variance of some rows and vanishes in others), rows 1, M // 2, M - 2 constant.
               The fused tails: weight rows around 0.05 against A of mean 4: the row mean after the residual add / of the expanded
               token is far from zero.  (The residual E1 of resln is N(0, 1) on the scale of the GEMM's own columns: were it the
               larger part of X, a GEMM 100 x too noisy would pass X's gate -- the CPU sensitivity test showed exactly that.)
  dy of the LayerNorm cases = U(-1, 1) + 0.25 + 0.5 sign(xhat), dY of the tn cases has a column mean of a quarter of its scale: no
  affine or bias gradient of those is a sum that cancels to nothing (dgamma sits 0.7 sqrt(M) standard deviations of its noise
  from zero), so the per-element measure of db / dgamma / dbeta is a measure of the sum.
"""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

from oracle_kit import one_thread as _one_thread
from conv_oracle import ceil2, measure          # noqa: F401  (re-exported: the same measures as the convolutions)

F64, F32 = torch.float64, torch.float32
MEASURES = ("max", "rms")
CLASSES = ("uniform", "act_scaled", "offset")
PRIMARY = "act_scaled"
EPS = 1e-5
BK = 32                       # k-step of the staged GEMM kernels: a k slice is a whole number of them
KIND_OF = {"C": "C", "gelu": "ep", "gelu_bwd": "ep", "res": "ep", "X": "C", "tok": "C", "y": "y", "Y": "y", "logits": "logits",
           "dx": "dx", "dW": "dW", "dw": "dW", "db": "sum", "dgamma": "sum", "dbeta": "sum", "sum": "sum", "dgamma_h": "hsum", "dbeta_h": "hsum", "mean": "stat",
           "rstd": "stat"}
KINDS = ("C", "ep", "y", "logits", "dx", "dW", "sum", "hsum", "stat")
ROWS_ARE_COLUMNS = ("dW", "dw")                   # measure(.., dim 0)
EACH = ("db", "dgamma", "dbeta", "sum", "dgamma_h", "dbeta_h", "rstd")   # every element on its own scale
GEMM_TENSOR = {"nt": "C", "tn": "dW", "resln": "X", "expand": "tok"}


def measure_of(key, got, ref):
    """The measures of one tensor under the rules of the module docstring."""
    got, ref = got.detach().double().reshape(ref.shape), ref.double()
    if key in EACH:
        return measure(got.reshape(1, -1), ref.reshape(1, -1), 1)
    if key == "mean":
        m = measure(got.reshape(-1, 1), ref.reshape(-1, 1), 1)
        return m
    if ref.dim() == 3:                            # logits [B][NC][S]: column = class
        return measure(got, ref, 1)
    return measure(got, ref, 0 if key in ROWS_ARE_COLUMNS else 1)


def _lib():
    from mis_hip import lib
    return lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# what the plain fp32 form takes from the library
# ---------------------------------------------------------------------------------------------------------------------
def nt_slices(M, N, K, planes=False):
    L = _lib()
    nb = L.mis_gemm_nt_split_workspace_bytes(M, N, K) if planes else L.mis_gemm_workspace_bytes(M, N, K, 0)
    return max(1, int(nb) // (M * N * 4))


def dw_slices(Cout, Cin, T):
    return max(1, int(_lib().mis_gemm_dw_workspace_bytes(Cout, Cin, T)) // (Cout * (Cin + 1) * 4))


def slab_rows(M):
    """Rows per slab of the column reductions: the smallest multiple of 8 that gives mis_colreduce_slabs(M) slabs."""
    slabs = int(_lib().mis_colreduce_slabs(M))
    r = 8
    while -(-M // r) != slabs:
        r += 8
        assert r <= M + 8, (M, slabs)
    return r


def slice_len(K, slices):
    return K if slices <= 1 else -(-(-(-K // slices)) // BK) * BK


# ---------------------------------------------------------------------------------------------------------------------
# fp32 in the kernels' order
# ---------------------------------------------------------------------------------------------------------------------
def reduce_order(parts):
    """gemm_reduce_kernel: lane kl sums slices kl, kl + 8, ... in turn; lane 0 then adds lanes 1 .. 7 in turn."""
    if len(parts) == 1:
        return parts[0]
    lanes = []
    for kl in range(min(8, len(parts))):
        s = parts[kl].clone()
        for k in range(kl + 8, len(parts), 8):
            s += parts[k]
        lanes.append(s)
    s = lanes[0]
    for t in lanes[1:]:
        s = s + t
    return s


def chain32(a, w, slices=1, rows=4096):
    """[M][N] = a [M][K] . w [N][K]^T in fp32: one sequential chain of rounded products per k slice, slices in reduce_order."""
    M, K = a.shape
    kc = slice_len(K, slices)
    wt = w.t().contiguous()
    out = torch.empty(M, w.shape[0], dtype=F32)
    for r0 in range(0, M, rows):
        at = a[r0:r0 + rows].t().contiguous()
        parts = []
        for k0 in range(0, K, kc):
            acc = torch.zeros(at.shape[1], w.shape[0], dtype=F32)
            for k in range(k0, min(K, k0 + kc)):
                acc.addcmul_(at[k][:, None], wt[k][None, :])
            parts.append(acc)
        out[r0:r0 + rows] = reduce_order(parts)
    return out


def colchain32(x, slices=1):
    """Column sums of x [T][C] in fp32: a sequential chain over the rows of a slice, slices in reduce_order."""
    T = x.shape[0]
    kc = slice_len(T, slices)
    parts = []
    for k0 in range(0, T, kc):
        acc = torch.zeros(x.shape[1], dtype=F32)
        for t in range(k0, min(T, k0 + kc)):
            acc += x[t]
        parts.append(acc)
    return reduce_order(parts)


def slab_sum(v, M):
    """Column sums of v [M][C] (fp32) as one fp32 partial per row slab, the partials summed in double."""
    R = slab_rows(M)
    pad = -M % R
    if pad:
        v = torch.cat((v, torch.zeros(pad, v.shape[1], dtype=v.dtype)))
    return v.view(-1, R, v.shape[1]).sum(1).double().sum(0)


def gelu_t(x):
    return 0.5 * x * (1 + torch.erf(x * (0.5 ** 0.5)))


def gelu_grad_t(x):
    return 0.5 * (1 + torch.erf(x * (0.5 ** 0.5))) + x * torch.exp(-0.5 * x * x) * (0.5 / math.pi) ** 0.5


def ln_two_pass(x, g, b):
    """(y, mean, rstd, xhat) in x's dtype: mean, then the centred sum of squares, then 1 / sqrt."""
    C = x.shape[1]
    mean = x.sum(1) / C
    a = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((a * a).sum(1) / C + EPS)
    xhat = a * rstd[:, None]
    return xhat * g + b, mean, rstd, xhat


def ln_backward(xhat, rstd, g, dy):
    """dx and the un-summed affine terms of LayerNorm's backward by hand, in the operands' dtype."""
    gdy = dy * g
    c1 = (gdy * xhat).mean(1, keepdim=True)
    c2 = gdy.mean(1, keepdim=True)
    return rstd[:, None] * (gdy - c2 - xhat * c1), dy * xhat, dy


def shuffle(e, B, H, W, P, c):
    """'b h w (p1 p2 c) -> b (h p1) (w p2) c' on token rows."""
    return e.view(B, H, W, P, P, c).permute(0, 1, 3, 2, 4, 5).reshape(B * H * P * W * P, c)


# ---------------------------------------------------------------------------------------------------------------------
# the operations: torch's operators (float64 / float32) or the kernels' order (fp32)
# ---------------------------------------------------------------------------------------------------------------------
def _scale_rows(c, dtype):
    return c["rowscale"].to(dtype).repeat_interleave(c["rps"])[:c["A"].shape[0], None]


def evaluate(c, dtype, kernel_order=False):
    op = c["op"]
    t = lambda k: c[k].to(dtype)
    if kernel_order:
        assert dtype == F32
        mm = lambda a, w: chain32(a, w, c.get("slices", 1))
        ln = ln_two_pass
    else:
        mm = lambda a, w: a @ w.t()
        ln = lambda x, g, b: (F.layer_norm(x, (x.shape[1],), g, b, EPS),) + ln_two_pass(x, g, b)[1:]
    r = {}
    if op == "nt":
        v = mm(t("A"), t("W"))
        r["C"] = v + t("bias")
        if c["ep"]:
            r["gelu"] = gelu_t(r["C"]) if kernel_order else F.gelu(r["C"])
            r["gelu_bwd"] = v * gelu_grad_t(t("E1"))
            r["res"] = t("E1") + _scale_rows(c, dtype) * r["C"]
    elif op == "tn":
        if kernel_order:
            r["dW"] = chain32(t("dY").t(), t("X").t(), c["slices"], rows=1 << 30)
            r["db"] = colchain32(t("dY"), c["slices"])
        else:
            r["dW"] = t("dY").t() @ t("X")
            r["db"] = t("dY").sum(0)
    elif op == "resln":
        r["X"] = t("E1") + _scale_rows(c, dtype) * (mm(t("A"), t("W")) + t("bias"))
        r["Y"], r["mean"], r["rstd"], _ = ln(r["X"], t("gamma"), t("beta"))
    elif op == "expand":
        B, H, W, P, cc = c["geom"]
        r["tok"] = shuffle(mm(t("A"), t("W")), B, H, W, P, cc)
        if c["ln"]:
            y, r["mean"], r["rstd"], _ = ln(r["tok"], t("gamma"), t("beta"))
            r["logits"] = (y @ t("hw").t()).view(B, H * P * W * P, -1).permute(0, 2, 1).contiguous()
    elif op == "ln":
        x, g, b, dy = t("x"), t("gamma"), t("beta"), t("dy")
        if kernel_order:
            r["y"], r["mean"], r["rstd"], xhat = ln_two_pass(x, g, b)
            r["dx"], pg, pb = ln_backward(xhat, r["rstd"], g, dy)
            r["dgamma"], r["dbeta"] = slab_sum(pg, x.shape[0]), slab_sum(pb, x.shape[0])
        else:
            x, g, b = (v.clone().requires_grad_(True) for v in (x, g, b))
            r["y"] = F.layer_norm(x, (x.shape[1],), g, b, EPS)
            r["y"].backward(dy)
            _, r["mean"], r["rstd"], _ = ln_two_pass(x.detach(), g.detach(), b.detach())
            r["dx"], r["dgamma"], r["dbeta"] = x.grad, g.grad, b.grad
    elif op in ("lnhead", "head"):
        B, S, C, NC = c["geom"]
        x, w = (t(k).clone().requires_grad_(True) for k in ("x", "hw"))
        if op == "lnhead":
            g, b = (t(k).clone().requires_grad_(True) for k in ("gamma", "beta"))
            y, r["mean"], r["rstd"], _ = ln(x, g, b)
            r["mean"], r["rstd"] = r["mean"].detach(), r["rstd"].detach()
        else:
            y = x
        lg = (y @ w.t()).view(B, S, NC).permute(0, 2, 1)
        lg.backward(t("dl"))
        r["logits"], r["dx"], r["dw"] = lg.detach().contiguous(), x.grad, w.grad
        if op == "lnhead":
            r["dgamma_h"], r["dbeta_h"] = g.grad, b.grad
    elif op == "colsum":
        r["sum"] = slab_sum(t("x"), c["x"].shape[0]) if kernel_order else t("x").sum(0)
    else:
        raise KeyError(op)
    return {k: v.detach().double() for k, v in r.items()}


def reference64(c):
    return evaluate(c, F64)


def reference32(c):
    return _one_thread(evaluate, c, F32)


def plain32(c):
    return _one_thread(evaluate, c, F32, True)


def loop64(c):
    """reference64 as explicit float64 loops: sums over k / over rows spelled out, LayerNorm's backward by hand."""
    op = c["op"]
    d = lambda k: c[k].double()

    def mm(a, w):
        acc = torch.zeros(a.shape[0], w.shape[0], dtype=F64)
        for k in range(a.shape[1]):
            acc += a[:, k:k + 1] * w[:, k][None, :]
        return acc
    r = {}
    if op == "nt":
        v = mm(d("A"), d("W"))
        r["C"] = v + d("bias")
        if c["ep"]:
            r["gelu"] = gelu_t(r["C"])
            r["gelu_bwd"] = v * gelu_grad_t(d("E1"))
            r["res"] = d("E1") + _scale_rows(c, F64) * r["C"]
    elif op == "tn":
        r["dW"] = mm(d("dY").t(), d("X").t())
        r["db"] = torch.stack([d("dY")[:, j].sum() for j in range(c["dY"].shape[1])])
    elif op == "resln":
        r["X"] = d("E1") + _scale_rows(c, F64) * (mm(d("A"), d("W")) + d("bias"))
        r["Y"], r["mean"], r["rstd"], _ = ln_two_pass(r["X"], d("gamma"), d("beta"))
    elif op == "expand":
        B, H, W, P, cc = c["geom"]
        e = mm(d("A"), d("W"))
        tok = torch.empty(B * H * P * W * P, cc, dtype=F64)
        for m in range(B * H * W):
            b, h, w = m // (H * W), (m // W) % H, m % W
            for p1 in range(P):
                for p2 in range(P):
                    tok[(b * H * P + h * P + p1) * W * P + w * P + p2] = e[m, (p1 * P + p2) * cc:(p1 * P + p2 + 1) * cc]
        r["tok"] = tok
        if c["ln"]:
            y, r["mean"], r["rstd"], _ = ln_two_pass(tok, d("gamma"), d("beta"))
            r["logits"] = torch.stack([(y * d("hw")[n]).sum(1).view(B, -1) for n in range(c["hw"].shape[0])], 1)
    elif op == "ln":
        r["y"], r["mean"], r["rstd"], xhat = ln_two_pass(d("x"), d("gamma"), d("beta"))
        r["dx"], pg, pb = ln_backward(xhat, r["rstd"], d("gamma"), d("dy"))
        r["dgamma"], r["dbeta"] = pg.sum(0), pb.sum(0)
    elif op in ("lnhead", "head"):
        B, S, C, NC = c["geom"]
        x, w = d("x"), d("hw")
        if op == "lnhead":
            y, r["mean"], r["rstd"], xhat = ln_two_pass(x, d("gamma"), d("beta"))
        else:
            y = x
        r["logits"] = torch.stack([(y * w[n]).sum(1).view(B, S) for n in range(NC)], 1)
        dl = d("dl").permute(0, 2, 1).reshape(B * S, NC)
        r["dw"] = torch.stack([(dl[:, n:n + 1] * y).sum(0) for n in range(NC)])
        dy = sum(dl[:, n:n + 1] * w[n][None, :] for n in range(NC))
        if op == "lnhead":
            r["dx"], pg, pb = ln_backward(xhat, r["rstd"], d("gamma"), dy)
            r["dgamma_h"], r["dbeta_h"] = pg.sum(0), pb.sum(0)
        else:
            r["dx"] = dy
    elif op == "colsum":
        r["sum"] = torch.stack([d("x")[:, j].sum() for j in range(c["x"].shape[1])])
    return r


# ---------------------------------------------------------------------------------------------------------------------
# the bf16x3 scheme, restated in float64
# ---------------------------------------------------------------------------------------------------------------------
def split3(x):
    """fp32 -> (h, m, l) in float64: each piece the value truncated to bf16's 8 significant bits, both remainders exact."""
    def trunc(v):
        return (v.contiguous().view(torch.int32) & -65536).view(F32)
    h = trunc(x)
    r1 = x - h
    m = trunc(r1)
    l = trunc(r1 - m)
    assert torch.equal(h.double() + m.double() + (r1 - m).double(), x.double())
    return h.double(), m.double(), l.double()


PIECE_PRODUCTS = ("hh", "hm", "mh", "hl", "lh", "mm")


def bf16x3_operands(c):
    """(a [M][K], b [N][K]) of the case's GEMM as fp32."""
    return (c["dY"].t().contiguous(), c["X"].t().contiguous()) if c["op"] == "tn" else (c["A"], c["W"])


def bf16x3_products(c):
    a, b = bf16x3_operands(c)
    pa, pb = dict(zip("hml", split3(a))), dict(zip("hml", split3(b)))
    return {p: pa[p[0]] @ pb[p[1]].t() for p in PIECE_PRODUCTS}


def bf16x3(c, drop=None, products=None):
    """The GEMM tensor of the case ({name: tensor}) through the six piece products, ``drop`` left out."""
    products = bf16x3_products(c) if products is None else products
    v = sum(products[p] for p in PIECE_PRODUCTS if p != drop)
    op = c["op"]
    if op == "nt":
        v = v + c["bias"].double()
    elif op == "resln":
        v = c["E1"].double() + _scale_rows(c, F64) * (v + c["bias"].double())
    elif op == "expand":
        v = shuffle(v, *c["geom"])
    return {GEMM_TENSOR[op]: v}


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(zlib.crc32(seed.encode()))


def decades(n, g):
    """A permuted logspace(-3, 0) over n channels."""
    return torch.logspace(-3, 0, n, dtype=F64)[torch.randperm(n, generator=g)]


def zero_channel(n, salt):
    return (5 * salt + 3) % n


def make_case(cid, spec, cls):
    g = _gen(f"{cid}/{cls}")
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    un = lambda *s: torch.rand(*s, generator=g, dtype=F64) * 2 - 1
    op, shape = spec["op"], spec["shape"]
    c = dict(spec, id=cid, cls=cls)
    # the fused epilogues stay off the offset class: its columns deep in GELU's negative tail leave the fp32 erf form of the
    # yardsticks no digit (1 + erf cancels: e32 of gelu(C) 2.5e-2 there), and a gate built on that would hold nothing
    c["ep"] = spec["ep"] and cls != "offset"

    def operands(M, N, K):
        """A [M][K], W [N][K], bias [N] of an NT GEMM."""
        if cls == "uniform":
            return un(M, K), un(N, K) * K ** -0.5, un(N)
        if cls == "offset":
            return 4 + rn(M, K), un(N, K) * K ** -0.5, un(N)
        sa, sw = decades(K, g), decades(N, g)
        sa[zero_channel(K, 1)] = 0.0
        sw[zero_channel(N, 2)] = 0.0
        return torch.relu(rn(M, K)) * sa, rn(N, K) * K ** -0.5 * sw[:, None], un(N) * sw

    def ln_rows(M, C):
        """x [M][C], gamma, beta of a LayerNorm."""
        gam, bet = 1 + 0.2 * un(C), 0.1 * un(C)
        if cls == "uniform":
            return un(M, C) * 2 + 0.5, gam, bet
        if cls == "act_scaled":
            sg = decades(C, g)
            sg[zero_channel(C, 3)] = 0.0
            return rn(M, C) * decades(C, g), gam * sg, bet * (sg > 0)
        rs = torch.logspace(-3, 3, 7, dtype=F64)[torch.arange(M) % 7]
        x = rs[:, None] * (100 + rn(M, C))
        if M >= 4:
            x[[1, M // 2, M - 2]] = 3.25
        return x, gam, bet

    if op == "nt":
        M, N, K = shape
        c["A"], c["W"], c["bias"] = operands(M, N, K)
        if c["ep"]:
            c["E1"] = rn(M, N) * 1.5
            c["rps"] = -(-M // 3)
            c["rowscale"] = torch.tensor([1.25, 0.0, 0.5], dtype=F64)
        c["slices"] = nt_slices(M, N, K, spec.get("planes", False))
    elif op == "tn":
        T, Cout, Cin = shape
        c["X"], dY, _ = operands(T, Cout, Cin)
        if cls == "act_scaled":
            sy = decades(Cout, g)
            sy[zero_channel(Cout, 4)] = 0.0
            c["dY"] = (rn(T, Cout) + 0.25) * sy
        else:
            c["dY"] = (rn(T, Cout) if cls == "offset" else un(T, Cout)) + 0.25
        c["slices"] = dw_slices(Cout, Cin, T)
    elif op == "resln":
        M, N, K = shape
        c["A"], c["W"], c["bias"] = operands(M, N, K)
        if cls == "offset":            # the GEMM itself carries the row mean: 0.2 K, some 8 .. 14 standard deviations of the row
            c["W"] = 0.05 + 0.1 * un(N, K)
        c["E1"] = rn(M, N) * (0.5 * c["W"].abs().amax(1) * K ** 0.5 if cls == PRIMARY else 1.0)
        c["rps"] = -(-M // 3)
        c["rowscale"] = torch.tensor([1.25, 0.0, 0.5], dtype=F64)
        c["gamma"], c["beta"] = 1.5 + un(N), un(N)
    elif op == "expand":
        B, H, W, P, cc, K, NC = shape
        c["geom"] = (B, H, W, P, cc)
        c["A"], c["W"], _ = operands(B * H * W, P * P * cc, K)
        if cls == "offset":
            c["W"] = 0.05 + 0.1 * un(P * P * cc, K)
        c["ln"] = NC > 0
        if NC:
            c["gamma"], c["beta"], c["hw"] = 1 + 0.2 * un(cc), 0.1 * un(cc), 0.3 * un(NC, cc)
    elif op == "ln":
        M, C = shape
        c["x"], c["gamma"], c["beta"] = ln_rows(M, C)
        x32 = c["x"].float().double()
        c["dy"] = un(M, C) + 0.25 + 0.5 * torch.sign(ln_two_pass(x32, torch.ones(C, dtype=F64), torch.zeros(C, dtype=F64))[3])
    elif op in ("lnhead", "head"):
        B, S, C, NC = shape
        c["geom"] = shape
        c["x"], c["gamma"], c["beta"] = ln_rows(B * S, C)
        c["hw"], c["dl"] = 0.3 * un(NC, C), un(B, NC, S)
        if op == "head":
            del c["gamma"], c["beta"]
    elif op == "colsum":
        M, C = shape
        c["x"] = ln_rows(M, C)[0]
    else:
        raise KeyError(op)
    for k, v in c.items():
        if torch.is_tensor(v) and v.dtype == F64:
            c[k] = v.float()
    return c


# ---------------------------------------------------------------------------------------------------------------------
# the case matrix: the smallest shapes the dispatch rules of gemm.hip and token_ops.hip admit for each kernel
#   nt / resln (M, N, K)   tn (T, Cout, Cin)   expand (B, H, W, P, c, K, NC)   ln / colsum (M, C)   lnhead / head (B, S, C, NC)
# group: what tests/test_token_edges_gpu.py runs a case as.  ``ep``: the fused epilogues run on it too.
# Shapes of 10^4 rows and more run their primary class only (the float64 reference of each is a second or two).
# ---------------------------------------------------------------------------------------------------------------------
ALL = CLASSES
ONE = (PRIMARY,)
TAIL = (PRIMARY, "offset")
SPECS = {}


def _spec(group, op, shape, classes=ONE, **kw):
    cid = f"{group}-" + "x".join(str(s) for s in shape)
    assert cid not in SPECS, cid
    SPECS[cid] = dict(group=group, op=op, shape=shape, classes=classes, ep=kw.pop("ep", False), **kw)


# gemm_nt_kernel 64 x 96 / 64 x 128 on fp32 B, both arithmetics: K % 32 != 0, ragged M and N tiles, N off the tile widths
_spec("nt", "nt", (200, 96, 48), ALL)
_spec("nt", "nt", (130, 1536, 96))
_spec("nt", "nt", (777, 200, 104), ALL, ep=True)
# ... split over K + gemm_reduce_kernel: 12 slices of 256; 3 slices of 352 with a ragged last one (296)
_spec("nt", "nt", (98, 768, 3072), ALL)
_spec("nt", "nt", (300, 200, 1000), ALL, ep=True)
# gemm_nt_short_kernel<96 / 128>: ragged last 64-row tile; K = 192 only in the fp32 form (bf16x3: the general kernel)
_spec("nt", "nt", (32801, 288, 96), ep=True)
_spec("short0", "nt", (33000, 384, 192))
# pre-split planes, 64 x 96 tiles (zero-padded planes beyond K = 100) and the 128 x 128 tiles of the "wide" rule
_spec("planes", "nt", (777, 576, 192), ALL, planes=True)
_spec("planes", "nt", (300, 192, 100), ALL, planes=True)
_spec("planes", "nt", (4000, 1536, 384), planes=True)
_spec("planes", "nt", (98, 768, 3072), planes=True)
# register-A kernels on natural-order planes: the walking one (K off 32, N == 96 rule) and the resident-panel one (K <= 96)
_spec("rega", "nt", (30001, 384, 100), ep=True, planes=True)
_spec("rega", "nt", (65570, 96, 384), planes=True)
_spec("rega", "nt", (65570, 96, 96), ep=True, planes=True)
_spec("rega", "nt", (30001, 288, 96), planes=True)
_spec("resln", "resln", (65570, 96, 96), TAIL)
_spec("resln", "resln", (65570, 96, 288), TAIL)
# gemm_tn_kernel<96 / 128> + split-K, db; gemm_tn_reg_kernel (widths % 96 == 0)
_spec("tn", "tn", (3137, 100, 36), ALL)
_spec("tn", "tn", (20000, 96, 288), ALL)
_spec("tnreg", "tn", (1001, 192, 96), ALL)
_spec("tnreg", "tn", (2054, 192, 96))
_spec("dwparts", "tn", (4100, 96, 192))
# pixel-shuffle store and the fused LayerNorm + head tails
_spec("expand", "expand", (2, 7, 7, 2, 96, 192, 0), ALL)
_spec("expandln", "expand", (1, 20, 12, 4, 96, 96, 2), TAIL)
_spec("expandln_rega", "expand", (10, 56, 56, 4, 96, 96, 3), TAIL)
# LayerNorm: one width per bracket of mis_layernorm_fwd / _bwd (<= 128, 256, 512, 768, 1024, 1536, beyond) + idle-lane widths
for _C in (96, 100, 192, 384, 516, 768, 1024, 1536, 2048):
    _spec("ln", "ln", (50, _C), ALL)
    _spec("ln", "ln", (3137, _C), ("offset",))
for _C in (36, 96, 128):
    _spec("lnhead", "lnhead", (2, 77, _C, 4 if _C != 128 else 3), ALL)
_spec("lnhead", "lnhead", (3, 1000, 96, 2), ("offset",))
_spec("head", "head", (2, 196, 96, 4), ALL)
_spec("colsum", "colsum", (1, 96), ("uniform",))
_spec("colsum", "colsum", (1882, 100), ALL)


def spec_of(name):
    return SPECS[name.split("/")[0]]


def names(*groups):
    """Case names ``id/class`` of the groups (all groups when none is given)."""
    return [f"{cid}/{cls}" for cid, s in SPECS.items() if not groups or s["group"] in groups for cls in s["classes"]]


def small(name):
    """Small enough for loop64 (and for every class of the CPU checks)."""
    s = spec_of(name)
    n = 1
    for v in s["shape"]:
        n *= max(v, 1)
    return n <= 6e8 and s["group"] not in ("expandln_rega",)


@functools.lru_cache(maxsize=4)
def case(name):
    cid, cls = name.split("/")
    return make_case(cid, SPECS[cid], cls)


@functools.lru_cache(maxsize=4)
def references(name):
    """(float64 reference, {tensor: {measure: e32}}) of a matrix case.  Computed once per run of consecutive uses (the large
    cases are too many to keep all at once), never modified."""
    c = case(name)
    r64 = reference64(c)
    r32, p32 = reference32(c), plain32(c)
    ea = {k: measure_of(k, r32[k], r64[k]) for k in r64}
    eb = {k: measure_of(k, p32[k], r64[k]) for k in r64}
    return r64, {k: {m: max(ea[k][m], eb[k][m]) for m in MEASURES} for k in r64}, ea, eb


def yardstick(name, key, m):
    return references(name)[1][key][m]


# ---------------------------------------------------------------------------------------------------------------------
# GELU: x on a grid over [-13, 13]
# ---------------------------------------------------------------------------------------------------------------------
# the fit of csrc/common.h (mis_gelu_parts): Phi(-a) = u(a) t P(t), t = 1 / (1 + GELU_T a), u = exp(-a^2 / 2); highest power first
GELU_T = 0.3
GELU_P = (3.664988946e-02, -1.611761927e-01, 2.130432014e-01, -5.969779766e-02, 1.316696142e-01, 9.899286856e-02,
          1.208983674e-01, 1.196200560e-01)
GELU_PHI_BOUND = 2e-7         # documented there: |Phi error| in fp32
GELU_BOUND = 4e-7             # and |gelu error| at |x| = 13


def gelu_grid():
    """fp32 x: 8001 even steps over [-13, 13], every binade's edge down to the smallest normal on both sides of the sign switch
    of cdf (x < 0 ? e : 1 - e), +-0, and denormals."""
    tiny = torch.tensor([2.0 ** -e for e in range(0, 127, 3)] + [2.0 ** -126, 2.0 ** -140, 2.0 ** -149], dtype=F64)
    x = torch.cat((torch.linspace(-13, 13, 8001, dtype=F64), tiny, -tiny, torch.tensor([0.0, -0.0, 13.0, -13.0], dtype=F64)))
    return torch.cat((x, x.new_zeros(-x.numel() % 4))).float()          # (whole float4: mis_gelu's contract)


def gelu64(x):
    """(gelu, gelu') in float64; the negative tail through erfc, which keeps its digits."""
    x = x.double()
    phi = 0.5 * torch.erfc(-x * 0.5 ** 0.5)
    return x * phi, phi + x * torch.exp(-0.5 * x * x) * (0.5 / math.pi) ** 0.5


def gelu32(x):
    """torch's fp32 erf form and its derivative through autograd."""
    x = x.float().clone().requires_grad_(True)
    y = F.gelu(x)
    y.backward(torch.ones_like(y))
    return y.detach().double(), x.grad.double()


def gelu_poly64(x):
    """(cdf, gelu, gelu') of the polynomial as written in common.h, evaluated in float64."""
    x = x.double()
    t = 1.0 / (1.0 + GELU_T * x.abs())
    p = torch.full_like(x, GELU_P[0])
    for coef in GELU_P[1:]:
        p = p * t + coef
    u = torch.exp(-0.5 * x * x)
    e = p * t * u
    cdf = torch.where(x < 0, e, 1 - e)
    return cdf, x * cdf, cdf + x * u * (0.5 / math.pi) ** 0.5


def gelu_measure(got, ref, x):
    """max: the largest |error| over max(1, |x|) (the documented bounds are absolute in Phi: |x| times that in gelu); rms: over
    the grid; tail: the largest RELATIVE error over x <= -1 where the reference is a normal fp32 number."""
    got, ref, x = got.double(), ref.double(), x.double()
    err = (got - ref).abs()
    tail = (x <= -1) & (ref.abs() >= 2.0 ** -126)
    return {"max": (err / x.abs().clamp(min=1)).max().item(), "rms": (err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item(),
            "tail": (err[tail] / ref[tail].abs()).max().item(), "zero_ok": bool((got[ref == 0] == 0).all())}
