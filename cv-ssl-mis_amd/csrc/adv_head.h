// The part of the discriminator's head that does not know the pool: Linear(C, K) -> cross-entropy on pooled features
// [N][C], and the Linear's weight gradient.  Shared by the 3-D head (adversarial.hip: one window, the whole feature) and
// the 2-D head (adversarial2d.hip: floor-mode windows, C = channels x windows).
#pragma once
#include "common.h"

namespace {

constexpr int MAXK = 8;

// one workgroup: logits, per-sample cross-entropy and d loss / d logits, then the mean in sample order
__global__ __launch_bounds__(256) void head_final_kernel(const float* __restrict__ pooled, const float* __restrict__ w,
                                                        const float* __restrict__ b, const int* __restrict__ target, int N,
                                                        int C, int K, float* __restrict__ logits, float* __restrict__ dlogits,
                                                        float* __restrict__ per_sample, float* __restrict__ loss) {
    __shared__ float red[4 * MAXK];
    for (int n = 0; n < N; ++n) {
        float v[MAXK];
#pragma unroll
        for (int k = 0; k < MAXK; ++k) {
            v[k] = 0.f;
            if (k < K)
                for (int c = threadIdx.x; c < C; c += 256) v[k] += w[(long long)k * C + c] * pooled[(long long)n * C + c];
        }
        mis_block_sum<MAXK>(v, red);
        if (threadIdx.x == 0) {
            float z[MAXK], mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < MAXK; ++k)
                if (k < K) {
                    z[k] = v[k] + (b ? b[k] : 0.f);
                    logits[n * K + k] = z[k];
                    mx = fmaxf(mx, z[k]);
                }
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < MAXK; ++k)
                if (k < K) sum += expf(z[k] - mx);
            const float lse = mx + logf(sum);
            const int y = target[n];
#pragma unroll
            for (int k = 0; k < MAXK; ++k)
                if (k < K) {
                    dlogits[n * K + k] = (expf(z[k] - lse) - (k == y ? 1.f : 0.f)) / (float)N;
                    if (k == y) per_sample[n] = lse - z[k];
                }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += per_sample[n];
        loss[0] = s / (float)N;
    }
}

// dw[k][c] (+)= sum_n dlogits[n][k] pooled[n][c],  db[k] (+)= sum_n dlogits[n][k]   (sample order)
__global__ __launch_bounds__(256) void head_bwd_dw_kernel(const float* __restrict__ pooled, const float* __restrict__ dlogits,
                                                         int N, int C, int K, float* __restrict__ dw, float* __restrict__ db,
                                                         int accumulate) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (dw && e < K * C) {
        const int k = e / C, c = e - k * C;
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += dlogits[n * K + k] * pooled[(long long)n * C + c];
        dw[e] = accumulate ? dw[e] + s : s;
    }
    if (db && e < K) {
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += dlogits[n * K + e];
        db[e] = accumulate ? db[e] + s : s;
    }
}

}  // namespace
