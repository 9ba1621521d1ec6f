// What the 3-D and the 2-D discriminator files (adversarial.hip, adversarial2d.hip) share: the host's check of the two-part
// input of a first layer and the grid of a streaming pass, and the part of the head that does not know the pool: Linear(C, K) ->
// cross-entropy on pooled features [N][C], and the Linear's weight gradient (3-D: one window, the whole feature; 2-D:
// floor-mode windows, C = channels x windows).
// Not here, on purpose: the softmax on the load path, G = dy * act'(y) * drop and the forward epilogue read alike in both files,
// but behind one inline function the 3-D kernels compiled to other code (same registers, same results) that measured 0.5 - 1.3 %
// slower.  The tile loaders and MFMA loops are different designs (element gather against staged rows).
#pragma once
#include "common.h"

namespace {

constexpr int MAXCL = 4;      // channels a first layer can read through the softmax
constexpr int MAXK = 8;

// the two-part input of a first layer: Cx plain channels and Cl softmax-read ones of S elements each
inline int adv_xsrc_check(const float* x, long long x_bs, int Cx, const float* logits, long long l_bs, int Cl, long long S) {
    if (Cx < 0 || Cl < 0 || Cx + Cl <= 0) return MIS_ERR_ARG;
    if ((Cx > 0 && !x) || (Cl > 0 && !logits)) return MIS_ERR_ARG;
    if ((Cx > 0 && x_bs < Cx * S) || (Cl > 0 && l_bs < Cl * S)) return MIS_ERR_ARG;
    if (Cl > MAXCL) return MIS_ERR_UNSUPPORTED;
    return MIS_OK;
}

// workgroups of 256 threads of a grid-stride pass over ``items``
inline unsigned stream_grid(long long items) {
    long long b = mis_cdiv(items, 256);
    if (b > 2048) b = 2048;
    return (unsigned)(b < 1 ? 1 : b);
}

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
