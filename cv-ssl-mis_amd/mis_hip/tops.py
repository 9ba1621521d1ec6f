"""Tensor-level wrappers of the token-major C-ABI kernels (SwinUnet): GEMM, LayerNorm, GELU,
residual+DropPath, token re-arrangements, patch im2col, output head, window attention.

Token tensors are 2-D ``[rows, C]`` fp32 views with a dense last dim and a free row stride (``ld``),
so column slices of a wider buffer (the decoder's concat) are valid operands.
"""
import ctypes
import os

import torch

from . import lib as _l
from .ops import JobTable, _prof_begin, _prof_end, _ws

# B operands (weights) of the NT GEMMs pre-split into their bf16 pieces once per step (mis_gemm_nt_split); 0: split per tile
PRESPLIT = os.environ.get("MIS_GEMM_PRESPLIT", "1") != "0"


def _mat(t):
    """(rows, cols, ld) of a 2-D row-major view."""
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RuntimeError(f"expected 2-D fp32 row-major view, got {tuple(t.shape)} strides {t.stride()}")
    if not t.is_cuda:
        _l.require_gpu(t)
    return t.shape[0], t.shape[1], (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def _ld(t):
    """The (pointer, row stride) operand of a token matrix that may be absent: (NULL, 0)."""
    return (t, _mat(t)[2]) if t is not None else (None, 0)


# (``L``, the library object, is not used: the parameter stays because tests/test_token_*_gpu.py call these two with one)
def _nt_name(L, M, N, K, epilogue):
    """NT instantiation mis_gemm / mis_gemm_ex pick (the library's ``*_kernel_name`` entry points print the plan the launcher
    itself runs)."""
    return _l.kernel_name("mis_gemm_nt_kernel_name", M, N, K, epilogue)


def _tn_name(L, A, lda, B, ldb, C, ldc, M, N, K):
    """TN kernel mis_gemm(trans) / mis_gemm_dw pick for these operands."""
    return _l.kernel_name("mis_gemm_tn_kernel_name", A, lda, B, ldb, C, ldc, M, N, K)


class SplitB:
    """The B operand of an NT GEMM cut into its three bf16 piece planes (``mis_gemm_split_b``): ``src`` [N, K] dense fp32 (an
    nn.Linear weight or its transpose); ``t`` the planes.  ``refresh()`` after the weights changed; a ``SplitBatch`` refreshes
    every SplitB of a network in one launch."""

    def __init__(self, src, rows=None):
        """``rows``: the token rows M of the GEMM these planes serve -- decides the element order inside a K = 32 block
        (``natural``: the register-A kernel's, mis_gemm_nt_split_natural; None: the staged kernels' order)."""
        N, K, ldb = _mat(src)
        self.src, self.N, self.K, self.ldb = src, N, K, ldb
        self.natural = bool(rows) and bool(_l.query("mis_gemm_nt_split_natural", int(rows), N, K))
        self.rows = rows
        self.t = torch.empty(_l.query("mis_gemm_split_bytes", N, K), dtype=torch.uint8, device="cuda")

    def refresh(self):
        _l.launch("mis_gemm_split_b_layout", self.src, self.ldb, self.N, self.K, self.t, int(self.natural))
        return self


class SplitBatch(JobTable):
    """``refresh()`` of many SplitB in one launch (``mis_gemm_split_batch``); the device job table is built once."""
    JOB_BYTES, BATCH = "mis_gemm_split_job_bytes", "mis_gemm_split_batch"

    def fill(self, slot, sb, first):
        return _l.query("mis_gemm_split_job_layout", slot, sb.src, sb.ldb, sb.N, sb.K, sb.t, first, int(sb.natural))


def split_active():
    """Pre-split B operands are used when the NT GEMMs run as bf16x3 products (``MIS_GEMM_PRESPLIT=0``: never)."""
    return PRESPLIT and bool(set_split_precision(-1) & 1)


def _nt_split(A, b3, C, bias=None, accumulate=False, epilogue=0, E1=None, C2=None, rowscale=None, rows_per_scale=1, ex=None):
    """mis_gemm_nt_split; False: outside what it covers (the caller runs the fp32-B entry point)."""
    M, K, lda = _mat(A)
    N = b3.N
    assert K == b3.K, (A.shape, b3.N, b3.K)
    if ex is None and C is None:       # EP_GELU_FWD without the pre-activation (a forward nobody differentiates)
        assert epilogue == EP_GELU_FWD and C2 is not None
        ldc, eH, eW, eP, ec = N, 0, 0, 0, 0
    elif ex is None:
        Mc, Nc, ldc = _mat(C)
        assert (Mc, Nc) == (M, N), (C.shape, M, N)
        eH = eW = eP = ec = 0
    else:
        eH, eW, eP, ec = ex
        ldc = N
    ws = _ws("gemm", "mis_gemm_nt_split_workspace_bytes", M, N, K, optional=True)
    prof = _prof_begin()
    if b3.natural and b3.rows != M:
        raise RuntimeError(f"natural-order planes were cut for {b3.rows} token rows, the GEMM has {M}")
    if not _l.try_launch("mis_gemm_nt_split_layout", A, lda, b3.t, C, ldc, bias, M, N, K, int(accumulate), int(epilogue), _ld(E1),
                         _ld(C2), rowscale, int(rows_per_scale), eH, eW, eP, ec, ws, int(b3.natural)):
        if b3.natural:
            raise RuntimeError("natural-order planes, but the register-A kernel refuses this call (the staged kernels cannot read them)")
        return False
    _prof_end(prof, lambda: _l.kernel_name("mis_gemm_nt_split_layout_kernel_name", M, N, K, int(epilogue), int(b3.natural)),
              2.0 * M * N * K, 4.0 * (M * K + M * N) + 6.0 * N * K)
    return True


def gemm(A, B, C, bias=None, trans=False, accumulate=False, b3=None):
    """trans=False: C[M,N] (+)= A[M,K] @ B[N,K]^T (+ bias);  trans=True: C[M,N] (+)= A[K,M]^T @ B[K,N].
    ``b3``: B pre-split (SplitB, current): used when the NT GEMMs run as bf16x3 products."""
    if b3 is not None and not trans and split_active() and _nt_split(A, b3, C, bias=bias, accumulate=accumulate):
        return
    if not trans:
        M, K, lda = _mat(A)
        N, K2, ldb = _mat(B)
    else:
        K, M, lda = _mat(A)
        K2, N, ldb = _mat(B)
    Mc, Nc, ldc = _mat(C)
    assert K == K2 and (Mc, Nc) == (M, N), (A.shape, B.shape, C.shape, trans)
    ws = _ws("gemm", "mis_gemm_workspace_bytes", M, N, K, int(trans), optional=True)
    prof = _prof_begin()
    _l.launch("mis_gemm", A, lda, B, ldb, C, ldc, bias, M, N, K, int(trans), int(accumulate), ws)
    _prof_end(prof, lambda: _tn_name(None, A, lda, B, ldb, C, ldc, M, N, K) if trans else _nt_name(None, M, N, K, 0),
              2.0 * M * N * K, 4.0 * (M * K + N * K + M * N))


def set_split_precision(mask):
    """Arithmetic of the nn.Linear GEMMs (mis_gemm_set_split_precision): bit 0 forward + dX, bit 1 dW as bf16x3 products
    (exact 3-way bf16 split of the fp32 operands, fp32 accumulation); 0 = fp32 MFMA.  Returns the previous mask; < 0 queries."""
    return int(_l.load().mis_gemm_set_split_precision(int(mask)))


def gemm_dw(dy, x, dW, db, accumulate=False):
    """dW[M,N] (+)= dy[K,M]^T @ x[K,N] and db[M] (+)= dy.sum(0) in one pass over dy (mis_gemm_dw)."""
    K, M, lddy = _mat(dy)
    K2, N, ldx = _mat(x)
    Mc, Nc, ldw = _mat(dW)
    assert K == K2 and (Mc, Nc) == (M, N) and db.numel() == M and db.is_contiguous(), (dy.shape, x.shape, dW.shape)
    ws = _ws("gemm", "mis_gemm_dw_workspace_bytes", M, N, K, optional=True)
    prof = _prof_begin()
    _l.launch("mis_gemm_dw", dy, lddy, x, ldx, dW, ldw, db, M, N, K, int(accumulate), ws)
    _prof_end(prof, lambda: _tn_name(None, dy, lddy, x, ldx, dW, ldw, M, N, K), 2.0 * M * N * K, 4.0 * (M * K + N * K + M * N))


def gemm_dw_parts(dy, x, dW, db, ws, accumulate=False):
    """``gemm_dw`` without its finishing launch (mis_gemm_dw_parts): returns the number of k-slices whose partials now sit in the
    caller's workspace ``ws`` (fp32: ``slices`` matrices [M, N], then ``slices`` rows [M] when ``db`` is given) -- 0: the
    contraction was not split and dW / db are complete.  ``db`` may be None (bias-free Linear)."""
    K, M, lddy = _mat(dy)
    K2, N, ldx = _mat(x)
    Mc, Nc, ldw = _mat(dW)
    assert K == K2 and (Mc, Nc) == (M, N) and (db is None or (db.numel() == M and db.is_contiguous())), (dy.shape, x.shape, dW.shape)
    prof = _prof_begin()
    slices = ctypes.c_int(0)
    _l.launch("mis_gemm_dw_parts", dy, lddy, x, ldx, dW, ldw, db, M, N, K, int(accumulate), ws,
              ws.numel() * ws.element_size() if ws is not None else 0, ctypes.byref(slices))
    _prof_end(prof, lambda: _tn_name(None, dy, lddy, x, ldx, dW, ldw, M, N, K), 2.0 * M * N * K, 4.0 * (M * K + N * K + M * N))
    return slices.value


def gemm_dw_workspace(M, N, K):
    """A workspace of the caller's own for gemm_dw_parts (None: this shape is never split)."""
    nb = _l.query("mis_gemm_dw_workspace_bytes", M, N, K)
    return torch.empty(nb // 4, dtype=torch.float32, device="cuda") if nb > 0 else None


class ColsumJob:
    """One finishing column sum ``out_a[c] (+)= sum_s part[s][c]`` (``pairs``: part is float2, .x -> out_a, .y -> out_b) for a
    ``ColsumBatch`` (mis_colsum_job).  ``part`` is a tensor whose storage holds the partial rows, ``offset`` floats into it."""

    def __init__(self, part, offset, stride, slabs, C, pairs, out_a, out_b=None, accumulate=False):
        """``pairs``: False / 0 float partial rows, True / 1 float2 (``.x -> out_a, .y -> out_b``), 2 the k-slices of a split GEMM
        (fp32 sums in the order of the GEMM's own reduction kernel: bit-identical to ``gemm_dw``)."""
        self.part, self.offset, self.stride, self.slabs, self.C, self.pairs = part, int(offset), int(stride), int(slabs), int(C), int(pairs)
        self.out_a, self.out_b, self.accumulate = out_a, out_b, bool(accumulate)
        for o in (out_a, out_b):
            assert o is None or (o.is_contiguous() and o.numel() >= C and o.dtype == torch.float32)
        self.bytes = self.slabs * self.C * (8 if self.pairs == 1 else 4)

    def part_ptr(self):
        return self.part.data_ptr() + 4 * self.offset


class ColsumBatch(JobTable):
    """Many ColsumJob in one launch (``mis_colsum_batch``); the device job table is built once and holds raw pointers."""
    JOB_BYTES, BATCH = "mis_colsum_job_bytes", "mis_colsum_batch"

    def fill(self, slot, j, first):
        return _l.query("mis_colsum_job", slot, j.part_ptr(), j.stride, j.slabs, j.C, int(j.pairs), j.out_a, j.out_b,
                        int(j.accumulate), first)


def colreduce_slabs(M):
    return _l.query("mis_colreduce_slabs", M)


def window_attention_table_partials(B, H, W, nH, window=7):
    """(rows, cols) of the bias-table partials ``window_attention_bwd_parts`` leaves at the start of its workspace, or None when
    the vector-pipe kernels (dS-block partials) are selected."""
    rows, cols = ctypes.c_longlong(0), ctypes.c_int(0)
    if not _l.supported("mis_window_attention_table_partials", B, H, W, nH, window, ctypes.byref(rows), ctypes.byref(cols)):
        return None
    return rows.value, cols.value


EP_GELU_FWD, EP_GELU_BWD, EP_RESIDUAL = 1, 2, 3


def gemm_ex(A, B, C, epilogue, bias=None, E1=None, C2=None, rowscale=None, rows_per_scale=1, b3=None):
    """C = epilogue(A[M,K] @ B[N,K]^T + bias) (mis_gemm_ex): EP_GELU_FWD also writes C2 = gelu(.), EP_GELU_BWD multiplies
    by gelu'(E1), EP_RESIDUAL gives E1 + rowscale[row // rows_per_scale] * (.).  Returns False when the shape is
    outside the fused form (the caller then runs the un-fused ops)."""
    if b3 is not None and split_active() and _nt_split(A, b3, C, bias=bias, epilogue=epilogue, E1=E1, C2=C2, rowscale=rowscale,
                                                     rows_per_scale=rows_per_scale):
        return True
    M, K, lda = _mat(A)
    N, K2, ldb = _mat(B)
    if C is None:          # EP_GELU_FWD only: the pre-activation is not kept (a forward nobody differentiates)
        assert epilogue == EP_GELU_FWD
        Mc, Nc, ldc = M, N, N
    else:
        Mc, Nc, ldc = _mat(C)
    assert K == K2 and (Mc, Nc) == (M, N)
    ws = _ws("gemm", "mis_gemm_workspace_bytes", M, N, K, 0, optional=True)
    prof = _prof_begin()
    if not _l.try_launch("mis_gemm_ex", A, lda, B, ldb, C, ldc, bias, M, N, K, int(epilogue), _ld(E1), _ld(C2), rowscale,
                         int(rows_per_scale), ws):
        return False
    # (split-K shapes run the plain instantiation + the reduce kernel, and that is the label)
    _prof_end(prof, lambda: _nt_name(None, M, N, K, epilogue), 2.0 * M * N * K, 4.0 * (M * K + N * K + M * N))
    return True


def gemm_residual_ln(A, b3, X, E1, gamma, beta, Y, mean, rstd, bias=None, rowscale=None, rows_per_scale=1, eps=1e-5):
    """X = E1 + rowscale[row // rows_per_scale] * (A @ W^T + bias) and Y = LayerNorm(X) * gamma + beta (mean / rstd kept) in one
    launch (mis_gemm_nt_residual_ln: the register-A kernels, 96 channels).  False: outside what it covers."""
    if b3 is None or not b3.natural or not split_active():
        return False
    M, K, lda = _mat(A)
    Mx, N, ldx = _mat(X)
    e1_v, y_v = _ld(E1), _ld(Y)
    if N != 96 or b3.N != 96 or b3.K != K or Mx != M or b3.rows != M:
        return False
    prof = _prof_begin()
    if not _l.try_launch("mis_gemm_nt_residual_ln", A, lda, b3.t, bias, M, N, K, e1_v, rowscale, int(rows_per_scale), X, ldx,
                         gamma, beta, eps, y_v, mean, rstd):
        return False
    _prof_end(prof, lambda: _l.kernel_name("mis_gemm_nt_split_layout_kernel_name", M, N, K, 5, 1), 2.0 * M * N * K,
              4.0 * (M * K + 3 * M * N) + 6.0 * N * K)
    return True


def droppath_table(table, p_dev, salt_dev, nsites, B, state):
    _l.launch("mis_droppath_table", table, p_dev, salt_dev, nsites, B, state)


def gemm_expand(x, w, out, B, H, W, P, c, b3=None):
    """out[(b, h*P+p1, w*P+p2)][c] = (x @ w^T) pixel-shuffled; returns False when the fused form does not cover the
    shape (the caller then runs gemm + token_rearrange)."""
    if b3 is not None and not b3.natural and split_active():      # (natural-order planes: only the register-A kernels read them)
        assert out.is_contiguous() and out.numel() == B * H * W * P * P * c
        if _nt_split(x, b3, out, ex=(H, W, P, c)):
            return True
    M, K, lda = _mat(x)
    N, K2, ldb = _mat(w)
    assert K == K2 and M == B * H * W and N == P * P * c and out.is_contiguous() and out.numel() == M * N
    prof = _prof_begin()
    if not _l.try_launch("mis_gemm_expand", x, lda, w, ldb, out, B, H, W, K, P, c):       # shape outside the fused form
        return False
    _prof_end(prof, lambda: _l.kernel_name("mis_gemm_expand_kernel_name", B, H, W, K, P, c, 0, 0), 2.0 * M * N * K,
              4.0 * (M * K + N * K + M * N))
    return True


def gemm_expand_ln_head(x, w, out, B, H, W, P, c, gamma, beta, head_w, mean, rstd, logits5, eps=1e-5, b3=None):
    """FinalPatchExpand_X4's Linear + pixel shuffle + LayerNorm + output head in one launch (mis_gemm_expand_ln_head):
    ``out`` [B H P W P, c] (None: the expanded tokens are not kept), mean / rstd per expanded token, logits5 [B, NC, 1, H P, W P].
    ``b3``: the expand weight's planes in the natural order (SplitB(rows=M)): the persistent register-A kernel
    (mis_gemm_expand_ln_head_split).  False: outside the fused form."""
    M, K, lda = _mat(x)
    N, K2, ldb = _mat(w)
    NC = logits5.shape[1]
    assert K == K2 and M == B * H * W and N == P * P * c and (out is None or (out.is_contiguous() and out.numel() == M * N))
    assert mean.numel() == M * P * P and rstd.numel() == M * P * P and tuple(head_w.shape) == (NC, c) and head_w.is_contiguous()
    prof = _prof_begin()
    tail = (B, H, W, K, P, c, gamma, beta, head_w, NC, eps, mean, rstd, logits5, logits5.stride(0))
    if b3 is not None and b3.natural and b3.rows == M and split_active() and \
            _l.try_launch("mis_gemm_expand_ln_head_split", x, lda, b3.t, out, tail):
        _prof_end(prof, lambda: _l.kernel_name("mis_gemm_expand_kernel_name", B, H, W, K, P, c, 1, 2), 2.0 * M * N * K,
                  4.0 * (M * K + (M * N if out is not None else 0)) + 6.0 * N * K)
        return True
    if not _l.try_launch("mis_gemm_expand_ln_head", x, lda, w, ldb, out, tail):
        return False
    _prof_end(prof, lambda: _l.kernel_name("mis_gemm_expand_kernel_name", B, H, W, K, P, c, 1, 0), 2.0 * M * N * K,
              4.0 * (M * K + N * K + (M * N if out is not None else 0)))
    return True


def transpose(src, dst):
    """dst[c][r] = src[r][c]."""
    R, Cc, lds = _mat(src)
    _l.launch("mis_transpose", src, lds, _ld(dst), R, Cc)


# ---------------------------------------------------------------- SwinUNETR encoder (csrc/swin3d.hip)
def win3d_gather(src, dst, B, dims, C, win, shift, inverse=False):
    """windows [B*nW, n, C] <- tokens [B*D*H*W, C] (zero padding to multiples of the window, cyclic shift); ``inverse``:
    tokens <- windows.  Each direction is the other's gradient."""
    D, H, W = dims
    _l.launch("mis_win3d_gather", src, dst, B, D, H, W, C, win[0], win[1], win[2], shift[0], shift[1], shift[2], int(inverse))


def win3d_windows(B, dims, win):
    return _l.query("mis_win3d_windows", B, dims[0], dims[1], dims[2], win[0], win[1], win[2])


def merge3d(src, dst, B, dims, C, inverse=False):
    """merged [B*D/2*H/2*W/2, 8C] <- tokens [B*D*H*W, C] in MONAI's v0.9 "merging" order; ``inverse``: token gradient."""
    _l.launch("mis_merge3d", src, dst, B, dims[0], dims[1], dims[2], C, int(inverse))


def win3d_attn_fwd(qkv, out, stats, table, region, BW, nW, n, nH):
    _l.launch("mis_win3d_attn_fwd", qkv, qkv.stride(0), out, out.stride(0), stats, table, region, BW, nW, n, nH)


def win3d_attn_bwd(qkv, out, dout, dqkv, stats, table, region, dtable, BW, nW, n, nH, accumulate_table=False):
    ws = _ws("attn3d", "mis_win3d_attn_workspace_bytes", BW, n, nH)
    _l.launch("mis_win3d_attn_bwd", qkv, qkv.stride(0), out, dout, dout.stride(0), dqkv, dqkv.stride(0), stats, table, region,
              dtable, int(accumulate_table), BW, nW, n, nH, ws)


class TransposeBatch(JobTable):
    """All weight transposes of a network's backward in one launch (``mis_transpose_batch``).  ``jobs``: list of
    (src [R, C] dense, dst [C, R] dense); the device job table is built once (it holds raw pointers into the tensors)."""
    JOB_BYTES, BATCH = "mis_transpose_job_bytes", "mis_transpose_batch"

    def fill(self, slot, job, first):
        src, dst = job
        R, Cc = src.shape
        assert src.is_contiguous() and dst.is_contiguous() and tuple(dst.shape) == (Cc, R)
        return _l.query("mis_transpose_job", slot, src, dst, R, Cc, first)


def layernorm_fwd(x, y, gamma, beta, mean, rstd, eps=1e-5):
    M, C, ldx = _mat(x)
    _l.launch("mis_layernorm_fwd", x, ldx, _ld(y), gamma, beta, mean, rstd, M, C, eps)


def layernorm_bwd(x, dy, dx, gamma, mean, rstd, dgamma, dbeta, accumulate_dx=False, accumulate_affine=False):
    M, C, ldx = _mat(x)
    ws = _ws("colreduce", "mis_colreduce_workspace_bytes", M, C)
    _l.launch("mis_layernorm_bwd", x, ldx, _ld(dy), _ld(dx), gamma, mean, rstd, dgamma, dbeta, M, C, int(accumulate_dx),
              int(accumulate_affine), ws)


def layernorm_bwd_parts(x, dy, dx, gamma, mean, rstd, ws, accumulate_dx=False):
    """dx and the affine partials into the caller's workspace ``ws`` (``colreduce_workspace``); ``layernorm_bwd_final`` finishes."""
    M, C, ldx = _mat(x)
    _l.launch("mis_layernorm_bwd_parts", x, ldx, _ld(dy), _ld(dx), gamma, mean, rstd, M, C, int(accumulate_dx), ws,
              ws.numel())


def layernorm_bwd_residual_parts(x, dy, gin, d_shortcut, d_branch, gamma, mean, rstd, ws, rowscale=None, rows_per_scale=1,
                                 accumulate_shortcut=False):
    """LayerNorm backward + the backward of the residual add that produced its input (mis_layernorm_bwd_residual_parts);
    False: outside the fused form (C > 1536)."""
    M, C, ldx = _mat(x)
    return _l.try_launch("mis_layernorm_bwd_residual_parts", x, ldx, _ld(dy), _ld(gin), _ld(d_shortcut), int(accumulate_shortcut),
                         _ld(d_branch), rowscale, int(rows_per_scale), gamma, mean, rstd, M, C, ws, ws.numel())


def layernorm_bwd_final(ws, M, C, dgamma, dbeta, accumulate_affine=False):
    _l.launch("mis_layernorm_bwd_final", ws, ws.numel(), M, C, dgamma, dbeta, int(accumulate_affine))


def colreduce_workspace(M, C):
    """A workspace of the caller's own for layernorm_bwd_parts / _final (the shared scratch is reused by the next call)."""
    return torch.empty(_l.query("mis_colreduce_workspace_bytes", M, C), dtype=torch.uint8, device="cuda")


def colsum(x, out, accumulate=False):
    M, C, ldx = _mat(x)
    ws = _ws("colreduce", "mis_colreduce_workspace_bytes", M, C)
    _l.launch("mis_colsum", x, ldx, M, C, out, int(accumulate), ws)


def gelu(x, out, dy=None):
    """dy None: out = gelu(x); else out = dy * gelu'(x).  Dense, same numel."""
    assert x.is_contiguous() and out.is_contiguous() and (dy is None or dy.is_contiguous())
    _l.launch("mis_gelu", x, dy, out, x.numel(), int(dy is not None))


def residual_fwd(a, y, out, rows_per_sample, drop_p=0.0, salt=0, state=None, scale_override=None):
    M, C, lda = _mat(a)
    _l.launch("mis_residual_droppath", a, lda, _ld(y), _ld(out), None, 0, M, C, rows_per_sample, drop_p, salt, state,
              scale_override, 0)


def residual_bwd(dout, d_shortcut, d_branch, rows_per_sample, drop_p=0.0, salt=0, state=None,
                 scale_override=None, accumulate_shortcut=False):
    """d_shortcut (may be None) (+)= dout; d_branch = s_b * dout."""
    mode = 2 if accumulate_shortcut else 1
    M, C, lda = _mat(dout)
    _l.launch("mis_residual_droppath", dout, lda, None, 0, _ld(d_shortcut), _ld(d_branch), M, C, rows_per_sample, drop_p, salt,
              state, scale_override, mode)


def token_rearrange(src, dst, B, H, W, C, P, mode, inverse=False):
    _l.launch("mis_token_rearrange", _ld(src), _ld(dst), B, H, W, C, P, mode, int(inverse))


def patch_im2col(x4, out, in_chans):
    """x4 [B,1|in_chans,H,W] (dense C,H,W) -> out [B*H/4*W/4, in_chans*16]; a single channel is repeated."""
    B, Cs, H, W = x4.shape
    assert x4.stride(3) == 1 and x4.stride(2) == W and (Cs == 1 or x4.stride(1) == H * W)
    _l.launch("mis_patch_im2col_c", x4, x4.stride(0), out, B, H, W, in_chans, Cs)


def head_fwd(x, w, logits5):
    """x [B*S, K] tokens, w [NC, K] -> logits [B, NC, 1, H, W]."""
    M, K, ldx = _mat(x)
    B, NC = logits5.shape[0], logits5.shape[1]
    S = M // B
    _l.launch("mis_head_fwd", x, ldx, w, logits5, logits5.stride(0), B, S, K, NC)


def ln_head_fwd(x, gamma, beta, w, mean, rstd, logits5, eps=1e-5):
    """logits [B, NC, 1, H, W] = head(LayerNorm(x)) in one pass over x [B*S, C] (mis_ln_head_fwd); False when the shape
    is outside the fused form."""
    M, C, ldx = _mat(x)
    B, NC = logits5.shape[0], logits5.shape[1]
    if C % 4 or C > 128 or not 2 <= NC <= 4 or M % B:
        return False
    _l.launch("mis_ln_head_fwd", x, ldx, gamma, beta, w, mean, rstd, logits5, logits5.stride(0), B, M // B, C, NC, eps)
    return True


def ln_head_bwd(x, gamma, beta, w, mean, rstd, dlogits5, dx, dgamma, dbeta, dw, accumulate_dx=False, unshuffle=None):
    """``unshuffle = (H, W, P)``: ``x`` rows are the tokens of the pixel-shuffled (H P) x (W P) grid and ``dx`` is the gradient of
    the expand Linear's OUTPUT [B H W, P P C]: the rows are stored through the inverse shuffle (mis_ln_head_bwd_unshuffle)."""
    M, C, ldx = _mat(x)
    _, _, lddx = _mat(dx)
    B, NC = dlogits5.shape[0], dlogits5.shape[1]
    ws = _ws("head", "mis_ln_head_workspace_bytes", M, C, NC)
    if unshuffle is not None:
        H, W, P = unshuffle
        assert M == B * H * P * W * P and dx.shape[0] == B * H * W and dx.shape[1] == P * P * C, (M, dx.shape, unshuffle)
        _l.launch("mis_ln_head_bwd_unshuffle", x, ldx, gamma, beta, w, mean, rstd, dlogits5, dlogits5.stride(0), dx, lddx,
                  int(accumulate_dx), dgamma, dbeta, dw, 0, B, H, W, P, C, NC, ws)
        return
    _l.launch("mis_ln_head_bwd", x, ldx, gamma, beta, w, mean, rstd, dlogits5, dlogits5.stride(0), dx, lddx, int(accumulate_dx),
              dgamma, dbeta, dw, 0, B, M // B, C, NC, ws)


def head_bwd(x, w, dlogits5, dx, dw, accumulate_dw=False):
    M, K, ldx = _mat(x)
    B, NC = dlogits5.shape[0], dlogits5.shape[1]
    S = M // B
    ws = _ws("head", "mis_head_workspace_bytes", K, NC)
    _l.launch("mis_head_bwd", x, ldx, w, dlogits5, dlogits5.stride(0), _ld(dx), dw, int(accumulate_dw), B, S, K, NC, ws)


def window_attention_fwd(qkv, out, table, B, H, W, nH, shift, scale, window=7):
    _l.launch("mis_window_attention_fwd_ws", _ld(qkv), _ld(out), table, B, H, W, nH, shift, scale, window)


def window_attention_bwd(qkv, dout, dqkv, table, dtable, B, H, W, nH, shift, scale, accumulate_table=False, window=7):
    ws = _ws("attn", "mis_window_attention_workspace_bytes_ws", B, H, W, nH, window)
    _l.launch("mis_window_attention_bwd_ws", _ld(qkv), _ld(dout), _ld(dqkv), table, dtable, int(accumulate_table), B, H, W, nH,
              shift, scale, window, ws)


ATTN_PATHS = ("mfma_f32", "mfma_bf16x3", "valu")


def window_attention_path(B, H, W, nH, *buffers, window=7):
    """Which kernels serve a window-attention launch over these token buffers (none: the table-gradient half / the shape
    queries): one of ATTN_PATHS, as the launchers themselves decide it (mis_window_attention_path)."""
    ldmax = max((_mat(t)[2] for t in buffers), default=0)
    return ATTN_PATHS[_l.query("mis_window_attention_path", B, H, W, nH, ldmax, window)]


def window_attention_workspace(B, H, W, nH, window=7):
    nb = _l.query("mis_window_attention_workspace_bytes_ws", B, H, W, nH, window)
    return torch.empty(nb, dtype=torch.uint8, device="cuda")


def window_attention_bwd_parts(qkv, dout, dqkv, table, ws, B, H, W, nH, shift, scale, window=7):
    _l.launch("mis_window_attention_bwd_parts_ws", _ld(qkv), _ld(dout), _ld(dqkv), table, B, H, W, nH, shift, scale, window,
              ws, ws.numel())


def window_attention_dtable(ws, dtable, B, H, W, nH, accumulate_table=False, window=7):
    _l.launch("mis_window_attention_dtable_ws", ws, ws.numel(), dtable, int(accumulate_table), B, H, W, nH, window)


# ---------------------------------------------------------------- UNETR (full attention, 3-D patch embedding)
def full_attention_fwd(qkv, out, stats, B, N, nH, scale):
    _l.launch("mis_full_attention_fwd", _ld(qkv), _ld(out), stats, B, N, nH, scale)


def full_attention_bwd(qkv, dout, dqkv, stats, B, N, nH, scale):
    ws = _ws("attn", "mis_full_attention_workspace_bytes", B, N, nH)
    _l.launch("mis_full_attention_bwd", _ld(qkv), _ld(dout), _ld(dqkv), stats, B, N, nH, scale, ws)


def patch3d_im2col(x5, out, P):
    """x5 [B,1,H,W,D] -> out [B*(H/P)(W/P)(D/P), P^3] (einops 'b c (h p1) (w p2) (d p3) -> b (h w d) (p1 p2 p3 c)')."""
    B, C, H, W, D = x5.shape
    assert C == 1 and x5.stride(4) == 1 and x5.stride(3) == D and x5.stride(2) == W * D
    _l.launch("mis_patch3d_im2col", x5, x5.stride(0), out, B, H, W, D, P)


def add_rowcycle(x, pos, out, L_rows):
    M, C, ldx = _mat(x)
    assert pos.is_contiguous() and pos.numel() == L_rows * C
    _l.launch("mis_add_rowcycle", x, ldx, pos, _ld(out), M, C, L_rows)


def sum_rowcycle(dy, dpos, L_rows):
    M, C, ld = _mat(dy)
    assert dpos.is_contiguous() and dpos.numel() == L_rows * C
    _l.launch("mis_sum_rowcycle", dy, ld, dpos, M, C, L_rows)
