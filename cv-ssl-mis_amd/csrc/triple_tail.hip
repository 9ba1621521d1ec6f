// Fused loss tail of triple-view training: three students, one pass over each student's logits.
//
// Replaces (reference, one step of train_tripleview_2D(demo).py:290-335), with p_m = softmax(z_m):
//   loss_m   = 0.5 * (ce_loss(z_m[:L], y) + dice_loss(p_m[:L], y))                                     (:299-304)
//   pseudo_j = argmax(p_j[L:].detach())                                                                (:307-312)
//   model_m_loss = loss_m + w * dice_loss(p_m[L:], pseudo_a) + w * dice_loss(p_m[L:], pseudo_b)        (:314-334)
// (a, b) = the other two students in ascending index, w = consistency * sigmoid_rampup(iter_num // 150).
// The pseudo labels are detached: dlogits_m is the gradient of model_m_loss alone.
//
// The three stages of loss_tail.hip: pass 1 reads every logit of the three students once and leaves 3 + 19C partial
// sums per workgroup (fixed-order tree, no atomics); one workgroup sums them in double and writes the scalars and
// the gradient coefficients; pass 2 reads the logits again and writes the three gradients.  What the students share
// is summed once: the labeled class counts Y_c, the pseudo-label counts Y_{j,c} of each peer, and the unlabeled
// Z_{m,c} = sum p_m,c^2 that both pseudo terms of student m divide by.
#include "tail.h"

namespace {

struct TripleArgs {
    const float* z[3]; long long zbs[3];     // logits [B][C][S] of the three students
    const void* label; int label_bytes;      // [L][S], uint8 or int64
    int B, L;
    long long S;
};

// the two peers of student m, ascending: the reference's ...1a/1b, 2a/2b, 3a/3b
__host__ __device__ constexpr int peer_of(int m, int k) { return m == 0 ? 1 + k : (m == 1 ? 2 * k : k); }

// partial layout per block, NP(C) = 3 + 19C floats:
//   [m]                                ce sum of student m
//   labeled   LY + c                   Y_c            (shared)
//             LI + m*C + c             I_{m,c} = sum p_m,c [y == c]
//             LZ + m*C + c             Z_{m,c} = sum p_m,c^2
//   unlabeled UY + j*C + c             Y_{j,c} = #[argmax z_j == c]
//             UZ + m*C + c             Z_{m,c}
//             UI + (2m+k)*C + c        I_{m,k,c} = sum p_m,c [argmax z_peer(m,k) == c]
__host__ __device__ constexpr int np_of(int C) { return 3 + 19 * C; }
#define TV_LY(C) (3)
#define TV_LI(C) (3 + (C))
#define TV_LZ(C) (3 + 4 * (C))
#define TV_UY(C) (3 + 7 * (C))
#define TV_UZ(C) (3 + 10 * (C))
#define TV_UI(C) (3 + 13 * (C))

// coefficient layout per student, NK(C) = 1 + 5C floats (see pass 2):
//   [0] ce scale; labeled a_c at 1 + c, b_c at 1 + C + c; pseudo a_{k,c} at 1 + 2C + k*C + c, b_c at 1 + 4C + c
__host__ __device__ constexpr int nk_of(int C) { return 1 + 5 * C; }

// mis_block_sum (the same tree, the same bits) with a scheduling fence after every eight values: left alone, the scheduler
// interleaves the 6 x NV independent cross-lane steps of up to 79 values and runs the kernel out of registers.
template <int NV>
__device__ __forceinline__ void tv_block_sum(float (&v)[NV], float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = mis_wave_sum(v[i]);
        if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) red[wave * NV + i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = ((red[i] + red[NV + i]) + red[2 * NV + i]) + red[3 * NV + i];
    }
}

template <int C>
__global__ __launch_bounds__(256) void triple_pass1_kernel(const TripleArgs a, float* __restrict__ part) {
    constexpr int NP = np_of(C);
    __shared__ float red[4 * NP];
    float v[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) v[i] = 0.f;
    const long long total = (long long)a.B * a.S;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / a.S);
        const long long sidx = i - (long long)b * a.S;
        float z[3][C], p[3][C], lse[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
#pragma unroll
            for (int c = 0; c < C; ++c) z[m][c] = a.z[m][(long long)b * a.zbs[m] + (long long)c * a.S + sidx];
            mis_tail_softmax<C>(z[m], p[m], lse[m]);
        }
        if (b < a.L) {
            const int y = mis_tail_label(a.label, a.label_bytes, (long long)b * a.S + sidx);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                // selects, not branches: the accumulators stay in registers on one straight-line path (and Y_c is shared
                // by the three students), so not the branching mis_tail_labeled_sums
                const float hit = c == y ? 1.f : 0.f;
                v[TV_LY(C) + c] += hit;
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    v[m] += hit * (lse[m] - z[m][c]);
                    v[TV_LI(C) + m * C + c] += hit * p[m][c];
                    v[TV_LZ(C) + m * C + c] += p[m][c] * p[m][c];
                }
            }
        } else {
            float hot[3][C];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int y = mis_tail_argmax<C>(z[j]);
#pragma unroll
                for (int c = 0; c < C; ++c) hot[j][c] = y == c ? 1.f : 0.f;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    v[TV_UY(C) + m * C + c] += hot[m][c];
                    v[TV_UZ(C) + m * C + c] += p[m][c] * p[m][c];
#pragma unroll
                    for (int k = 0; k < 2; ++k) v[TV_UI(C) + (2 * m + k) * C + c] += hot[peer_of(m, k)][c] * p[m][c];
                }
            }
        }
    }
    tv_block_sum<NP>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NP; ++i) part[(long long)blockIdx.x * NP + i] = v[i];
    }
}

struct TripleFinalArgs {
    const float* part; int blocks; int C; int L; int Bu; long long S;
    float cons_weight; const MisStepState* st;
    float* out[3]; float* coef;
};

constexpr int TV_MAXNP = np_of(4);

// out_m: [0] loss_m, [1] ce, [2] dice, [3] pseudo_supervision_a, [4] w, [5] pseudo_supervision_b
__global__ __launch_bounds__(256) void triple_final_kernel(const TripleFinalArgs a) {
    __shared__ double tot[TV_MAXNP];
    const int C = a.C, NP = np_of(C);
    mis_tail_reduce_parts(a.part, a.blocks, NP, NP, tot);
    if (threadIdx.x != 0) return;
    const float w = a.st ? a.st->cons_weight : a.cons_weight;
    const double nlab = (double)a.L * (double)a.S;
    for (int m = 0; m < 3; ++m) {
        float* coef = a.coef + m * nk_of(C);
        const double ce = a.L > 0 ? tot[m] / nlab : 0.0;
        double dice_l = 0.0, dice_u[2] = {0.0, 0.0};
        for (int c = 0; c < C; ++c) {
            // d(scale * dice_mean)/dp_c = a_c * [y == c] + b_c * p_c
            double dl, ac, bc;
            mis_tail_dice_coef(tot[TV_LI(C) + m * C + c], tot[TV_LY(C) + c], tot[TV_LZ(C) + m * C + c], 0.5, C, dl, ac, bc);
            dice_l += dl;
            coef[1 + c] = (float)ac;
            coef[1 + C + c] = (float)bc;
            double bu = 0.0;
            for (int k = 0; k < 2; ++k) {
                mis_tail_dice_coef(tot[TV_UI(C) + (2 * m + k) * C + c], tot[TV_UY(C) + peer_of(m, k) * C + c],
                                   tot[TV_UZ(C) + m * C + c], (double)w, C, dl, ac, bc);
                dice_u[k] += dl;
                coef[1 + 2 * C + k * C + c] = (float)ac;
                bu += bc;
            }
            coef[1 + 4 * C + c] = (float)bu;
        }
        dice_l = a.L > 0 ? dice_l / C : 0.0;
        const double ps_a = a.Bu > 0 ? dice_u[0] / C : 0.0, ps_b = a.Bu > 0 ? dice_u[1] / C : 0.0;
        float* out = a.out[m];
        out[0] = (float)(0.5 * (ce + dice_l) + (double)w * ps_a + (double)w * ps_b);
        out[1] = (float)ce; out[2] = (float)dice_l; out[3] = (float)ps_a; out[4] = w; out[5] = (float)ps_b;
        coef[0] = a.L > 0 ? (float)(0.5 / nlab) : 0.f;
    }
}

struct TripleGradArgs { float* d[3]; long long dbs[3]; };

// dlogit_j = p_j * (g_j - sum_c g_c p_c) [+ CE term], g = dLoss_m/dp
template <int C>
__global__ __launch_bounds__(256) void triple_pass2_kernel(const TripleArgs a, const float* __restrict__ coef,
                                                           const TripleGradArgs d) {
    constexpr int NK = nk_of(C);
    const long long total = (long long)a.B * a.S;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / a.S);
        const long long sidx = i - (long long)b * a.S;
        float z[3][C], p[3][C], lse;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
#pragma unroll
            for (int c = 0; c < C; ++c) z[m][c] = a.z[m][(long long)b * a.zbs[m] + (long long)c * a.S + sidx];
            mis_tail_softmax<C>(z[m], p[m], lse);
        }
        const bool lab = b < a.L;
        int y[3] = {0, 0, 0};
        if (lab) {
            y[0] = mis_tail_label(a.label, a.label_bytes, (long long)b * a.S + sidx);
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) y[j] = mis_tail_argmax<C>(z[j]);
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const float* __restrict__ k = coef + m * NK;
            // not mis_tail_labeled_grad: g takes the labeled or the two pseudo-label terms, then one shared tail
            float g[C], dot = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (lab) {
                    g[c] = k[1 + C + c] * p[m][c] + (c == y[0] ? k[1 + c] : 0.f);
                } else {
                    g[c] = k[1 + 4 * C + c] * p[m][c] + (c == y[peer_of(m, 0)] ? k[1 + 2 * C + c] : 0.f) +
                           (c == y[peer_of(m, 1)] ? k[1 + 3 * C + c] : 0.f);
                }
                dot += g[c] * p[m][c];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float o = p[m][c] * (g[c] - dot);
                if (lab) o += k[0] * (p[m][c] - (c == y[0] ? 1.f : 0.f));
                d.d[m][(long long)b * d.dbs[m] + (long long)c * a.S + sidx] = o;
            }
        }
    }
}

int triple_blocks(long long B, long long S) { return mis_tail_blocks(B * S); }

}  // namespace

extern "C" long long mis_triple_view_tail_workspace_bytes(int B, int C, long long S) {
    if (B <= 0 || S <= 0) return MIS_ERR_ARG;
    if (C != 2 && C != 3 && C != 4) return MIS_ERR_UNSUPPORTED;
    return ((long long)triple_blocks(B, S) * np_of(C) + 3 * nk_of(C)) * (long long)sizeof(float);
}

// out1..3: >= 6 floats each (device).  d1..3: all three or none (forward only).
extern "C" int mis_triple_view_tail(const float* z1, long long z1_bs, const float* z2, long long z2_bs, const float* z3,
                                    long long z3_bs, const void* label, int label_bytes, int B, int L, int C,
                                    long long S, float cons_weight, const MisStepState* state, float* out1, float* out2,
                                    float* out3, float* d1, long long d1_bs, float* d2, long long d2_bs, float* d3,
                                    long long d3_bs, void* workspace, long long workspace_bytes, hipStream_t stream) {
    if (!z1 || !z2 || !z3 || !out1 || !out2 || !out3 || !workspace || B <= 0 || L < 0 || L > B || C <= 0 || S <= 0)
        return MIS_ERR_ARG;
    if (L > 0 && !label) return MIS_ERR_ARG;
    if (label_bytes != 1 && label_bytes != 8) return MIS_ERR_ARG;
    const int nd = (d1 != nullptr) + (d2 != nullptr) + (d3 != nullptr);
    if (nd != 0 && nd != 3) return MIS_ERR_ARG;
    if (C != 2 && C != 3 && C != 4) return MIS_ERR_UNSUPPORTED;
    const long long row = (long long)C * S;
    if (B > 1 && (z1_bs < row || z2_bs < row || z3_bs < row)) return MIS_ERR_ARG;
    if (nd && B > 1 && (d1_bs < row || d2_bs < row || d3_bs < row)) return MIS_ERR_ARG;
    if (workspace_bytes < mis_triple_view_tail_workspace_bytes(B, C, S)) return MIS_ERR_WORKSPACE;
    const TripleArgs a{{z1, z2, z3}, {z1_bs, z2_bs, z3_bs}, label, label_bytes, B, L, S};
    const int blocks = triple_blocks(B, S);
    float* part = reinterpret_cast<float*>(workspace);
    float* coef = part + (long long)blocks * np_of(C);
    MIS_DISPATCH_C(C, triple_pass1_kernel, blocks, stream, a, part)
    const TripleFinalArgs f{part, blocks, C, L, B - L, S, cons_weight, state, {out1, out2, out3}, coef};
    hipLaunchKernelGGL(triple_final_kernel, dim3(1), dim3(256), 0, stream, f);
    if (nd) {
        const TripleGradArgs d{{d1, d2, d3}, {d1_bs, d2_bs, d3_bs}};
        MIS_DISPATCH_C(C, triple_pass2_kernel, blocks, stream, a, coef, d)
    }
    return mis_launch_status();
}
