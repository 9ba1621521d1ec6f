// Deep co-training (rotation consistency): the rotation of the unlabeled batch, the loss tail over the logits of the
// two student passes, and the sum of the two passes' weight gradients.
//
// Replaces (reference code/train_deep_co_training_2D.py:136-158, _2D_ViT.py:174-196):
//   rot_times = random.randrange(0, 4)                                                    -> sched[state->iter_num]
//   rotated_unlabeled_volume_batch = torch.rot90(unlabeled_volume_batch, rot_times, [2,3])  -> mis_rot90
//   P = softmax(outputs[L:]), Q = softmax(model(rotated))
//   loss = 0.5 * (CE + Dice)(outputs[:L], label)
//        + w * 0.5 * (mean((Q.detach() - rot(P))^2) + mean((Q - rot(P).detach())^2))      -> mis_dct_tail
//   loss.backward() through both forwards of one network (autograd sums the two uses)     -> mis_grad_combine
//
// k is read on the device (sched[state->iter_num]) so that a replayed step rotates by its own iteration's k.
// torch.rot90(x, k, [2,3]) writes out[i][j] = in[src(i, j)] with
//   k = 0: (i, j)    k = 1: (j, W-1-i)    k = 2: (H-1-i, W-1-j)    k = 3: (H-1-j, i)
// and out is [W][H] for odd k.  For odd k that is a transpose: the source of an output tile is a tile of the input
// whose rows are the output's columns, so both kernels below stage a tile in LDS (rows padded by one float: 64
// four-byte banks) and read and write global memory row by row.
#include "tail.h"

namespace {

__device__ __forceinline__ int dct_k(const int* __restrict__ sched, long long n, const MisStepState* __restrict__ st,
                                     int k_override) {
    if (k_override >= 0) return k_override & 3;
    long long it = st->iter_num;
    if (it < 0) it = 0;
    if (it >= n) it = n - 1;              // past the schedule (the reference stops at max_iterations): its last entry
    return sched[it] & 3;
}

// source pixel of output pixel (i, j); H x W = the SOURCE geometry
__device__ __forceinline__ void rot_src(int k, int H, int W, int i, int j, int& si, int& sj) {
    switch (k) {
        case 0: si = i; sj = j; break;
        case 1: si = j; sj = W - 1 - i; break;
        case 2: si = H - 1 - i; sj = W - 1 - j; break;
        default: si = H - 1 - j; sj = i; break;
    }
}

// the source rectangle (origin ar0, ac0; ah x aw) of the output tile [ti, ti + th) x [tj, tj + tw)
__device__ __forceinline__ void rot_region(int k, int H, int W, int ti, int tj, int th, int tw, int& ar0, int& ac0,
                                           int& ah, int& aw) {
    switch (k) {
        case 0: ar0 = ti; ac0 = tj; ah = th; aw = tw; break;
        case 1: ar0 = tj; ac0 = W - ti - th; ah = tw; aw = th; break;
        case 2: ar0 = H - ti - th; ac0 = W - tj - tw; ah = th; aw = tw; break;
        default: ar0 = H - tj - tw; ac0 = ti; ah = tw; aw = th; break;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// rot90: one 64 x 64 output tile of one (sample, channel) plane per workgroup
// ---------------------------------------------------------------------------------------------------------------------
constexpr int RT = 64;

__global__ __launch_bounds__(256) void rot90_kernel(const float* __restrict__ in, long long in_bs, float* __restrict__ out,
                                                    long long out_bs, int C, int H, int W, int tiles_x, int tiles_y,
                                                    const int* __restrict__ sched, long long n_sched,
                                                    const MisStepState* __restrict__ st, int k_override) {
    __shared__ float t[RT][RT + 1];
    const int k = dct_k(sched, n_sched, st, k_override);
    const int Ho = (k & 1) ? W : H, Wo = (k & 1) ? H : W;
    const int tile = blockIdx.x % (tiles_x * tiles_y), plane = blockIdx.x / (tiles_x * tiles_y);
    const int n = plane / C, c = plane - n * C;
    const int ti = (tile / tiles_x) * RT, tj = (tile % tiles_x) * RT;
    const int th = min(RT, Ho - ti), tw = min(RT, Wo - tj);
    int ar0, ac0, ah, aw;
    rot_region(k, H, W, ti, tj, th, tw, ar0, ac0, ah, aw);
    const float* __restrict__ src = in + (long long)n * in_bs + (long long)c * H * W;
    const int lane = threadIdx.x & 63;
    for (int r = threadIdx.x >> 6; r < ah; r += 4)
        if (lane < aw) t[r][lane] = src[(long long)(ar0 + r) * W + ac0 + lane];
    __syncthreads();
    float* __restrict__ dst = out + (long long)n * out_bs + (long long)c * Ho * Wo;
    for (int i = threadIdx.x >> 6; i < th; i += 4) {
        if (lane < tw) {
            int si, sj;
            rot_src(k, H, W, ti + i, tj + lane, si, sj);
            dst[(long long)(ti + i) * Wo + tj + lane] = t[si - ar0][sj - ac0];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// loss tail
// ---------------------------------------------------------------------------------------------------------------------
struct DArgs {
    const float* a; long long a_bs;      // pass A logits [L + U][C][H][W]
    const float* r; long long r_bs;      // pass R logits [U][C][H][W] (square when k is odd)
    const void* label; int label_bytes;  // [L][H][W], uint8 or int64
    int L, U, C, H, W;
    const int* sched; long long n_sched; const MisStepState* st; int k_override;
};

// ---- labeled rows of pass A: CE + Dice (the labeled branch of the ICT / Mean-Teacher tails) ----
// partial layout per block: [0] = ce_sum, [1+3c] = I_c, [2+3c] = Y_c, [3+3c] = Z_c
constexpr int NPL = 1 + 3 * MIS_MAXC;

template <int C>
__global__ __launch_bounds__(256) void dct_lab1_kernel(const DArgs a, float* __restrict__ part) {
    __shared__ float red[4 * NPL];
    float v[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) v[i] = 0.f;
    const long long S = (long long)a.H * a.W, units = S >> 2, total = (long long)a.L * units;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / units);
        const long long u = i - (long long)b * units;
        const float* __restrict__ sb = a.a + (long long)b * a.a_bs + u * 4;
        float z[4][C];
        mis_tail_load4<C>(sb, S, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float p[C], lse;
            mis_tail_softmax<C>(z[j], p, lse);
            const int y = mis_tail_label(a.label, a.label_bytes, (long long)b * S + u * 4 + j);
            mis_tail_labeled_sums<C>(z[j], p, lse, y, v[0], v + 1);
        }
    }
    mis_block_sum<NPL>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NPL; ++i) part[(long long)blockIdx.x * NPL + i] = v[i];
    }
}

template <int C>
__global__ __launch_bounds__(256) void dct_lab2_kernel(const DArgs a, const float* __restrict__ coef,
                                                       float* __restrict__ da, long long da_bs) {
    const float kce = coef[0];
    float ac[C], bc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { ac[c] = coef[2 + 2 * c]; bc[c] = coef[3 + 2 * c]; }
    const long long S = (long long)a.H * a.W, units = S >> 2, total = (long long)a.L * units;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / units);
        const long long u = i - (long long)b * units;
        const float* __restrict__ sb = a.a + (long long)b * a.a_bs + u * 4;
        float z[4][C], o[4][C];
        mis_tail_load4<C>(sb, S, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float p[C], lse;
            mis_tail_softmax<C>(z[j], p, lse);
            const int y = mis_tail_label(a.label, a.label_bytes, (long long)b * S + u * 4 + j);
            mis_tail_labeled_grad<C>(p, y, kce, ac, bc, o[j]);
        }
        mis_tail_store4<C>(da + (long long)b * da_bs + u * 4, S, o);
    }
}

// ---- the consistency term: one 32 x 32 tile of R pixels of one unlabeled sample per workgroup, paired with its source
// tile in A.  Every channel of the A tile is staged in LDS at once (C x 32 x 33 floats; a 64 x 64 tile of four channels
// would be 66 KB): the reads of A and the writes of dA go row by row ----
constexpr int CT = 32;

template <int C, bool GRAD>
__global__ __launch_bounds__(256) void dct_cons_kernel(const DArgs a, int tiles_x, int tiles_y,
                                                       const float* __restrict__ coef, float* __restrict__ part,
                                                       float* __restrict__ da, long long da_bs, float* __restrict__ dr,
                                                       long long dr_bs) {
    __shared__ float t[C][CT][CT + 1];
    __shared__ float red[4];
    const int k = dct_k(a.sched, a.n_sched, a.st, a.k_override);
    const int H = a.H, W = a.W;
    const long long S = (long long)H * W;
    const int tile = blockIdx.x % (tiles_x * tiles_y), u = blockIdx.x / (tiles_x * tiles_y);
    const int ti = (tile / tiles_x) * CT, tj = (tile % tiles_x) * CT;
    const int th = min(CT, H - ti), tw = min(CT, W - tj);
    int ar0, ac0, ah, aw;
    rot_region(k, H, W, ti, tj, th, tw, ar0, ac0, ah, aw);
    const int col = threadIdx.x & 31, row0 = threadIdx.x >> 5;      // 8 rows of 32 per round, 4 rounds
    const float* __restrict__ ab = a.a + (long long)(a.L + u) * a.a_bs;
#pragma unroll
    for (int c = 0; c < C; ++c)
        for (int r = row0; r < ah; r += 8)
            if (col < aw) t[c][r][col] = ab[(long long)c * S + (long long)(ar0 + r) * W + ac0 + col];
    __syncthreads();
    const float* __restrict__ rb = a.r + (long long)u * a.r_bs;
    const float kc = GRAD ? coef[1] : 0.f;
    float acc = 0.f;
    float gA[4][C];
    int sl[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = row0 + 8 * q;
        sl[q][0] = -1;
        sl[q][1] = 0;
        if (i >= th || col >= tw) continue;
        int si, sj;
        rot_src(k, H, W, ti + i, tj + col, si, sj);
        si -= ar0; sj -= ac0;
        sl[q][0] = si; sl[q][1] = sj;
        float zr[C], za[C], Q[C], P[C], lse;
        const long long off = (long long)(ti + i) * W + tj + col;
#pragma unroll
        for (int c = 0; c < C; ++c) { zr[c] = rb[(long long)c * S + off]; za[c] = t[c][si][sj]; }
        mis_tail_softmax<C>(zr, Q, lse);
        mis_tail_softmax<C>(za, P, lse);
        if (!GRAD) {
#pragma unroll
            for (int c = 0; c < C; ++c) { const float d = Q[c] - P[c]; acc += d * d; }
        } else {
            // dL/dQ = kc (Q - rot P), dL/d(rot P) = kc (rot P - Q); dlogit_c = p_c (g_c - sum_j g_j p_j)
            float d[C], dq = 0.f, dp = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                d[c] = kc * (Q[c] - P[c]);
                dq += d[c] * Q[c];
                dp += d[c] * P[c];
            }
            float* __restrict__ ob = dr + (long long)u * dr_bs + off;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                ob[(long long)c * S] = Q[c] * (d[c] - dq);
                gA[q][c] = P[c] * (dp - d[c]);
            }
        }
    }
    if (!GRAD) {
        acc = mis_wave_sum(acc);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        return;
    }
    __syncthreads();                    // every read of the staged logits is done: the tile takes dA now
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (sl[q][0] < 0) continue;
#pragma unroll
        for (int c = 0; c < C; ++c) t[c][sl[q][0]][sl[q][1]] = gA[q][c];
    }
    __syncthreads();
    float* __restrict__ ob = da + (long long)(a.L + u) * da_bs;
#pragma unroll
    for (int c = 0; c < C; ++c)
        for (int r = row0; r < ah; r += 8)
            if (col < aw) ob[(long long)c * S + (long long)(ar0 + r) * W + ac0 + col] = t[c][r][col];
}

// the two forms of the consistency kernel under names that MIS_DISPATCH_C can instantiate with the class count alone
template <int C> constexpr auto dct_cons_sum = dct_cons_kernel<C, false>;
template <int C> constexpr auto dct_cons_grad = dct_cons_kernel<C, true>;

// out[0]=loss out[1]=loss_ce out[2]=loss_dice out[3]=consistency_loss out[4]=consistency_weight out[5]=k
// out[6..6+C) = class-wise dice score
// coef[0]=ce scale, coef[1]=consistency scale, coef[2+2c]=a_c, coef[3+2c]=b_c   (see dct_lab2_kernel)
struct DFinalArgs {
    const float* part_l; int blocks_l; const float* part_c; int blocks_c;
    DArgs a; float cons_weight; float loss_scale;
    float* out; float* coef;
};

__global__ __launch_bounds__(256) void dct_final_kernel(const DFinalArgs f) {
    __shared__ double tot[NPL + 1];
    const int C = f.a.C;
    mis_tail_reduce_parts(f.part_l, f.blocks_l, NPL, 1 + 3 * C, tot);      // 1 + 3C labeled sums,
    mis_tail_reduce_parts(f.part_c, f.blocks_c, 1, 1, tot + 1 + 3 * C);    // then the squared-error sum
    if (threadIdx.x != 0) return;
    const DArgs& a = f.a;
    const double S = (double)a.H * (double)a.W;
    const double nlab = (double)a.L * S;
    const double nun = (double)a.U * (double)C * S;
    const float w = a.st ? a.st->cons_weight : f.cons_weight;
    const float gate = a.st ? a.st->cons_gate : 1.f;
    const double wl = gate != 0.f ? (double)w : 0.0;
    const double ce = tot[0] / nlab;
    const double mse = gate != 0.f ? tot[1 + 3 * C] / nun : 0.0;   // gated off: reads 0, like mis_loss_tail / mis_ict_tail
    double dice = 0.0;
    for (int c = 0; c < C; ++c) {
        double dl, ac, bc;
        mis_tail_dice_coef(tot[1 + 3 * c], tot[2 + 3 * c], tot[3 + 3 * c], 0.5 * f.loss_scale, C, dl, ac, bc);
        dice += dl;
        f.out[6 + c] = (float)(1.0 - dl);
        f.coef[2 + 2 * c] = (float)ac;
        f.coef[3 + 2 * c] = (float)bc;
    }
    dice /= C;
    f.out[0] = (float)(0.5 * (dice + ce) + wl * mse);
    f.out[1] = (float)ce; f.out[2] = (float)dice; f.out[3] = (float)mse; f.out[4] = w;
    f.out[5] = (float)dct_k(a.sched, a.n_sched, a.st, a.k_override);
    f.coef[0] = (float)(f.loss_scale * 0.5 / nlab);
    f.coef[1] = (float)(f.loss_scale * wl / nun);
}

int lab_blocks(long long L, long long S) { return mis_tail_blocks(L * (S >> 2)); }

// ---------------------------------------------------------------------------------------------------------------------
// gradient sum over the flat buffer
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grad_combine4_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                            long long n4, int accumulate) {
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        float4 s = reinterpret_cast<const float4*>(src)[i];
        if (accumulate) {
            const float4 d = reinterpret_cast<const float4*>(dst)[i];
            s = make_float4(d.x + s.x, d.y + s.y, d.z + s.z, d.w + s.w);
        }
        reinterpret_cast<float4*>(dst)[i] = s;
    }
}

__global__ __launch_bounds__(256) void grad_combine1_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                            long long n, int accumulate) {
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        dst[i] = accumulate ? dst[i] + src[i] : src[i];
}

}  // namespace

extern "C" int mis_rot90(const float* in, long long in_bs, float* out, long long out_bs, int N, int C, int H, int W,
                         const int* sched, long long n_sched, const MisStepState* state, int k_override,
                         hipStream_t stream) {
    if (!in || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0) return MIS_ERR_ARG;
    if (k_override < 0 && (!sched || n_sched <= 0 || !state)) return MIS_ERR_ARG;
    if (k_override > 3) return MIS_ERR_ARG;
    // the output of an odd k is W x H: unless k is known to be even, the plane must be square
    if (H != W && (k_override < 0 || (k_override & 1))) return MIS_ERR_ARG;
    const long long plane = (long long)H * W;
    if (in_bs < (long long)C * plane || out_bs < (long long)C * plane) return MIS_ERR_ARG;
    const int tx = (int)mis_cdiv(W, RT), ty = (int)mis_cdiv(H, RT);
    const long long nb = (long long)tx * ty * N * C;
    if (nb > 0x7FFFFFFFLL) return MIS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(rot90_kernel, dim3((unsigned)nb), dim3(256), 0, stream, in, in_bs, out, out_bs, C, H, W, tx, ty,
                       sched, n_sched, state, k_override);
    return mis_launch_status();
}

extern "C" long long mis_dct_tail_workspace_bytes(int L, int U, int C, int H, int W) {
    if (L <= 0 || U <= 0 || C <= 0 || H <= 0 || W <= 0) return MIS_ERR_ARG;
    const long long nbc = (long long)U * mis_cdiv(H, CT) * mis_cdiv(W, CT);
    return ((long long)lab_blocks(L, (long long)H * W) * NPL + nbc + 2 + 2 * MIS_MAXC) * (long long)sizeof(float);
}

// logits_a: [L + U][C][H][W]; logits_r: [U][C][H][W]; out >= 6 + C floats (device).  dA and dR may both be nullptr.
extern "C" int mis_dct_tail(const float* logits_a, long long a_bs, const float* logits_r, long long r_bs,
                            const void* label, int label_bytes, int L, int U, int C, int H, int W, const int* sched,
                            long long n_sched, const MisStepState* state, int k_override, float cons_weight,
                            float loss_scale, float* out, float* dA, long long dA_bs, float* dR, long long dR_bs,
                            void* workspace, long long workspace_bytes, hipStream_t stream) {
    if (!logits_a || !logits_r || !label || !out || !workspace || L <= 0 || U <= 0 || C <= 0 || H <= 0 || W <= 0)
        return MIS_ERR_ARG;
    if (label_bytes != 1 && label_bytes != 8) return MIS_ERR_ARG;
    if (k_override < 0 && (!sched || n_sched <= 0 || !state)) return MIS_ERR_ARG;
    if (k_override > 3) return MIS_ERR_ARG;
    if (H != W && (k_override < 0 || (k_override & 1))) return MIS_ERR_ARG;
    if ((dA == nullptr) != (dR == nullptr)) return MIS_ERR_ARG;
    if (C != 2 && C != 3 && C != 4) return MIS_ERR_UNSUPPORTED;
    const long long S = (long long)H * W;
    if (S % 4 || a_bs % 4 || !mis_aligned16(logits_a)) return MIS_ERR_UNSUPPORTED;
    if (a_bs < (long long)C * S || r_bs < (long long)C * S) return MIS_ERR_ARG;
    if (dA && (dA_bs % 4 || !mis_aligned16(dA) || dA_bs < (long long)C * S || dR_bs < (long long)C * S)) return MIS_ERR_UNSUPPORTED;
    if (workspace_bytes < mis_dct_tail_workspace_bytes(L, U, C, H, W)) return MIS_ERR_WORKSPACE;
    DArgs a{logits_a, a_bs, logits_r, r_bs, label, label_bytes, L, U, C, H, W, sched, n_sched, state, k_override};
    const int nbl = lab_blocks(L, S);
    const int tx = (int)mis_cdiv(W, CT), ty = (int)mis_cdiv(H, CT);
    const int nbc = U * tx * ty;
    float* part_l = reinterpret_cast<float*>(workspace);
    float* part_c = part_l + (long long)nbl * NPL;
    float* coef = part_c + nbc;
    const float* ccoef = coef;
    float* no_f = nullptr;
    MIS_DISPATCH_C(C, dct_lab1_kernel, nbl, stream, a, part_l)
    MIS_DISPATCH_C(C, dct_cons_sum, nbc, stream, a, tx, ty, ccoef, part_c, no_f, 0LL, no_f, 0LL)
    DFinalArgs f{part_l, nbl, part_c, nbc, a, cons_weight, loss_scale, out, coef};
    hipLaunchKernelGGL(dct_final_kernel, dim3(1), dim3(256), 0, stream, f);
    if (dA) {
        MIS_DISPATCH_C(C, dct_lab2_kernel, nbl, stream, a, ccoef, dA, dA_bs)
        MIS_DISPATCH_C(C, dct_cons_grad, nbc, stream, a, tx, ty, ccoef, no_f, dA, dA_bs, dR, dR_bs)
    }
    return mis_launch_status();
}

extern "C" int mis_grad_combine(float* dst, const float* src, long long n, int accumulate, hipStream_t stream) {
    if (!dst || !src || n <= 0) return MIS_ERR_ARG;
    const bool vec = n % 4 == 0 && mis_aligned16(dst) && mis_aligned16(src);
    long long nb = mis_cdiv(vec ? n >> 2 : n, 256);
    if (nb > 4096) nb = 4096;
    if (vec)
        hipLaunchKernelGGL(grad_combine4_kernel, dim3((unsigned)nb), dim3(256), 0, stream, dst, src, n >> 2, accumulate);
    else
        hipLaunchKernelGGL(grad_combine1_kernel, dim3((unsigned)nb), dim3(256), 0, stream, dst, src, n, accumulate);
    return mis_launch_status();
}
