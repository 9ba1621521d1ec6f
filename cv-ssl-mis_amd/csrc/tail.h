// Building blocks shared by the fused loss tails (loss_tail.hip, uamt_tail.hip, ict.hip, dct.hip, triple_tail.hip, fixmatch.hip) and
// the stand-alone Dice operator (losses.hip).  Every tail has the same three stages: pass 1 leaves fixed-order partial
// sums per workgroup, a one-workgroup finalize sums them in double and writes the scalars and the per-class Dice
// gradient coefficients, pass 2 writes dlogits.  What is here is the half every tail shares, CE + Dice on the labeled
// samples, and the plumbing round it; the unlabeled halves stay in their own files.  Only __forceinline__ device code
// and static inline host code: no kernels, no state.
#pragma once
#include "common.h"

#define MIS_MAXC 8   // bound of the per-class partial-sum and coefficient layouts

// [.][S] labels, uint8 (bytes == 1) or int64 (bytes == 8)
__device__ __forceinline__ int mis_tail_label(const void* lab, int bytes, long long i) {
    return bytes == 1 ? (int)reinterpret_cast<const unsigned char*>(lab)[i]
                      : (int)reinterpret_cast<const long long*>(lab)[i];
}

// softmax over the C logits of one voxel, in registers; lse = log sum exp z
template <int C>
__device__ __forceinline__ void mis_tail_softmax(const float (&z)[C], float (&p)[C], float& lse) {
    float mx = z[0];
#pragma unroll
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { p[c] = expf(z[c] - mx); sum += p[c]; }
    const float inv = 1.f / sum;
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] *= inv;
    lse = mx + logf(sum);
}

// first maximum wins, as torch.argmax (softmax is monotone: the arg-max of the logits is the pseudo label)
template <int C>
__device__ __forceinline__ int mis_tail_argmax(const float (&z)[C]) {
    float best = z[0];
    int y = 0;
#pragma unroll
    for (int c = 1; c < C; ++c)
        if (z[c] > best) { best = z[c]; y = c; }
    return y;
}

// four consecutive voxels of the C channel planes at base (plane stride S): one float4 per class, z[voxel][class]
template <int C>
__device__ __forceinline__ void mis_tail_load4(const float* __restrict__ base, long long S, float (&z)[4][C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float4 q = *reinterpret_cast<const float4*>(base + (long long)c * S);
        z[0][c] = q.x; z[1][c] = q.y; z[2][c] = q.z; z[3][c] = q.w;
    }
}

template <int C>
__device__ __forceinline__ void mis_tail_store4(float* __restrict__ base, long long S, const float (&o)[4][C]) {
#pragma unroll
    for (int c = 0; c < C; ++c)
        *reinterpret_cast<float4*>(base + (long long)c * S) = make_float4(o[0][c], o[1][c], o[2][c], o[3][c]);
}

// Pass 1 of one labeled voxel with p = softmax(z) and label y: ce += -log p_y, and the Dice sums of every class at
// iyz[3c + {0, 1, 2}] = (I_c += p_c [y == c], Y_c += [y == c], Z_c += p_c^2).
template <int C>
__device__ __forceinline__ void mis_tail_labeled_sums(const float (&z)[C], const float (&p)[C], float lse, int y,
                                                      float& ce, float* iyz) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (c == y) { ce += lse - z[c]; iyz[3 * c] += p[c]; iyz[3 * c + 1] += 1.f; }
        iyz[3 * c + 2] += p[c] * p[c];
    }
}

// Pass 2 of one labeled voxel: with g_c = dDice/dp_c = b_c p_c + [y == c] a_c (mis_tail_dice_coef),
// dlogit_c = p_c (g_c - sum_j g_j p_j) + kce (p_c - [y == c]).  The sum has two products and the compiler may fuse
// either into the add; the fmaf says which: the CE product is rounded, the Dice product is fused.
template <int C>
__device__ __forceinline__ void mis_tail_labeled_grad(const float (&p)[C], int y, float kce, const float (&ac)[C],
                                                      const float (&bc)[C], float (&o)[C]) {
    float g[C], dot = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        g[c] = bc[c] * p[c] + (c == y ? ac[c] : 0.f);
        dot += g[c] * p[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = fmaf(p[c], g[c] - dot, kce * (p[c] - (c == y ? 1.f : 0.f)));
}

// Finalize, all 256 threads of the one workgroup: tot[i] = sum over the workgroups b of part[b * stride + i], i < n, in
// double and in a fixed order.  tot is in shared memory and is valid for every thread when this returns.
__device__ __forceinline__ void mis_tail_reduce_parts(const float* __restrict__ part, int blocks, int stride, int n,
                                                      double* tot) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = 0; i < n; ++i) {
        double s = 0.0;
        for (int b = threadIdx.x; b < blocks; b += 256) s += part[(long long)b * stride + i];
        s = mis_wave_sum_d(s);
        __syncthreads();
        if (lane == 0) red[wave] = s;
        __syncthreads();
        if (threadIdx.x == 0) tot[i] = (red[0] + red[1]) + (red[2] + red[3]);
    }
    __syncthreads();
}

// One class of the Dice loss (reference losses.py:165-201) from its three sums: dl = 1 - (2I + smooth) / (Z + Y + smooth)
// and the coefficients of d(scale * mean_c dl_c)/dp_c = a [y == c] + b p_c.
__device__ __forceinline__ void mis_tail_dice_coef(double I, double Y, double Z, double scale, int C, double& dl,
                                                   double& a, double& b) {
    const double smooth = 1e-5;
    const double num = 2.0 * I + smooth, den = Z + Y + smooth;
    dl = 1.0 - num / den;
    const double s2 = 2.0 * scale;
    a = s2 * (-1.0 / C) / den;
    b = s2 * (1.0 / C) * num / (den * den);
}

// grid of a streaming pass over `items` work items: four per thread of 256, at most 2048 workgroups
static inline int mis_tail_blocks(long long items) {
    long long b = mis_cdiv(items, 256 * 4);
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (int)b;
}

static inline bool mis_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// launch KERNEL<C> (256 threads per workgroup) for the class counts the tails are built for
#define MIS_DISPATCH_C(C, KERNEL, grid, stream, ...)                                                             \
    switch (C) {                                                                                                 \
        case 2: hipLaunchKernelGGL(KERNEL<2>, dim3(grid), dim3(256), 0, stream, __VA_ARGS__); break;             \
        case 3: hipLaunchKernelGGL(KERNEL<3>, dim3(grid), dim3(256), 0, stream, __VA_ARGS__); break;             \
        case 4: hipLaunchKernelGGL(KERNEL<4>, dim3(grid), dim3(256), 0, stream, __VA_ARGS__); break;             \
    }
