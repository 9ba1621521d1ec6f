// FixMatch with complementary ("negative") learning: the strong augmentation of the weak batch and the loss tail over the
// logits of one network on the weak and on the strong batch.
//
// Replaces (reference code/train_Fixmatch_CNN_2D.py:132-166, :259-288; code/dataloaders/dataset.py:99-107, :228):
//   image_strong = ColorJitter(0.8, 0.8, 0.8, 0.2)(image_weak)                                  -> mis_color_jitter
//   pw = softmax(model(weak)), ps = softmax(model(strong))
//   pseudo = argmax(pw * (((pw - min pw) / max pw) > conf_thresh))[L:]            (detached)
//   comp   = argmin(pw)                                                           (detached)
//   sup    = CE(zw[:L], y) + Dice(pw[:L], y)
//   a      = mean_{b,c}(1 - Categorical(probs = ps[b, c, :]).entropy() / ln S)    (not detached)
//   unsup  = CE(zs[L:], pseudo) + Dice(ps[L:], pseudo) + a * (a * CE(1 - ps, comp))
//   loss   = sup + w * unsup                                                                     -> mis_fixmatch_tail
//
// The entropy of q = ps[b, c, :] / A[b, c] needs A[b, c] = sum_s ps[b, c, s] first, so the tail has one pass more than its
// siblings: pass 1 (A and every sum that does not need A) -> per-sample sums, A among them -> pass 2 (entropy sums) ->
// per-sample sums -> one-workgroup finalize in double -> gradient pass.  A workgroup of a streaming pass works on ONE
// sample (workgroup = sample * nbs + j), so the per-sample sums are the fixed-order sums of that sample's nbs partials.
// No atomics: reruns are bit-identical.
#include "tail.h"
#include "../../include/mis_hip_fixmatch.h"      // the declarations of this file's entry points

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// colour jitter of a one-channel float image: torchvision's saturation and hue adjustments return such an image unchanged,
// what is left of ColorJitter is, in a random order,
//   brightness  F.adjust_brightness = _blend(img, 0, beta):          clamp(beta * x, 0, 1)
//   contrast    F.adjust_contrast   = _blend(img, mean(img), gamma): clamp(gamma * x + (1 - gamma) * mean(x), 0, 1)
// with mean(x) the mean of the image as it stands when contrast is applied.  The mean is a two-level sum whose shape is fixed
// by JCH alone: one workgroup sums one chunk of JCH consecutive pixels (same tree for every chunk), the apply kernel sums
// the image's chunk sums in double.  Neither order depends on the grid, and an image is worked on by S / JCH workgroups.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int JCH = 4096;            // pixels per chunk: 16 per thread
constexpr float J_LO = 0.2f, J_HI = 1.8f;

struct JArgs {
    const float* x; long long x_bs;
    float* y; long long y_bs;
    long long S; int nch;
    const float* params;             // [B][3] = (beta, gamma, order) or nullptr: drawn from st
    const MisStepState* st; uint32_t salt;
    float* drawn;                    // [B][3] (may be nullptr): the factors this call used
};

// order 0: brightness then contrast; order 1: contrast then brightness
__device__ __forceinline__ void jitter_factors(const JArgs& a, int b, float& beta, float& gamma, int& order) {
    if (a.params) {
        beta = a.params[3 * b]; gamma = a.params[3 * b + 1]; order = a.params[3 * b + 2] != 0.f;
        return;
    }
    // Philox counters (sample, 0, salt, iter) under the key (seed): a replayed step draws new factors every iteration
    const uint64_t seed = a.st->seed;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ (uint32_t)((uint64_t)a.st->iter_num >> 32);
    uint32_t r[4];
    mis_philox4((uint32_t)b, 0u, a.salt, (uint32_t)a.st->iter_num, k0, k1, r);
    beta = fminf(J_LO + (J_HI - J_LO) * mis_u01(r[0]), J_HI);
    gamma = fminf(J_LO + (J_HI - J_LO) * mis_u01(r[1]), J_HI);
    order = (int)(r[2] & 1u);
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// the pixel index of this thread's i-th item in chunk k: V consecutive pixels (V = 4: one float4), 16 / V items per thread
template <int V>
__device__ __forceinline__ long long jitter_px(int k, int i) {
    return ((long long)k * (JCH / V) + threadIdx.x + 256 * i) * V;
}

template <int V>
__global__ __launch_bounds__(256) void jitter_sum_kernel(const JArgs a, float* __restrict__ part) {
    __shared__ float red[4];
    const int b = blockIdx.x / a.nch, k = blockIdx.x - b * a.nch;
    float beta, gamma;
    int order;
    jitter_factors(a, b, beta, gamma, order);
    const float* __restrict__ xb = a.x + (long long)b * a.x_bs;
    float s[1] = {0.f};
#pragma unroll
    for (int i = 0; i < 16 / V; ++i) {
        const long long px = jitter_px<V>(k, i);
        if (px >= a.S) continue;
        float v[V];
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(xb + px);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = xb[px];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) s[0] += order ? v[j] : clamp01(beta * v[j]);
    }
    mis_block_sum<1>(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

template <int V>
__global__ __launch_bounds__(256) void jitter_apply_kernel(const JArgs a, const float* __restrict__ part) {
    __shared__ double tot[1];
    const int b = blockIdx.x / a.nch, k = blockIdx.x - b * a.nch;
    float beta, gamma;
    int order;
    jitter_factors(a, b, beta, gamma, order);
    mis_tail_reduce_parts(part + (long long)b * a.nch, a.nch, 1, 1, tot);
    const float m = (float)(tot[0] / (double)a.S);
    if (k == 0 && threadIdx.x == 0 && a.drawn) {
        a.drawn[3 * b] = beta; a.drawn[3 * b + 1] = gamma; a.drawn[3 * b + 2] = (float)order;
    }
    const float* __restrict__ xb = a.x + (long long)b * a.x_bs;
    float* __restrict__ yb = a.y + (long long)b * a.y_bs;
    const float off = (1.f - gamma) * m;
#pragma unroll
    for (int i = 0; i < 16 / V; ++i) {
        const long long px = jitter_px<V>(k, i);
        if (px >= a.S) continue;
        float v[V];
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(xb + px);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = xb[px];
        }
#pragma unroll
        for (int j = 0; j < V; ++j)
            v[j] = order ? clamp01(beta * clamp01(gamma * v[j] + off)) : clamp01(gamma * clamp01(beta * v[j]) + off);
        if constexpr (V == 4)
            *reinterpret_cast<float4*>(yb + px) = make_float4(v[0], v[1], v[2], v[3]);
        else
            yb[px] = v[0];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// loss tail
// ---------------------------------------------------------------------------------------------------------------------
struct FArgs {
    const float* zw; long long w_bs;     // weak logits [B][C][S]
    const float* zs; long long s_bs;     // strong logits [B][C][S]
    const void* label; int label_bytes;  // [L][S], uint8 or int64
    int B, L;
    long long S;
    float tau;
    int nbs;                             // workgroups per sample
};

// Block-wide sum of NV values per thread (256 threads), result in thread 0: mis_block_sum with the wave step done by
// mis_group_sum (four DPP adds, one swizzle, one bpermute per value instead of six bpermutes): pass 1 sums 4 + 7C values
// per workgroup for one float4 of pixels per thread (measured: 10 us of a 124 us tail at [24, 4, 256, 256]).  Fixed tree.
template <int NV>
__device__ __forceinline__ void fm_block_sum(float (&v)[NV], float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = mis_group_sum<64>(v[i]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) red[wave * NV + i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = (red[i] + red[NV + i]) + (red[2 * NV + i] + red[3 * NV + i]);
    }
}

constexpr float FM_EPS = 1.1920928955078125e-07f;        // 2^-23: torch.finfo(torch.float32).eps, the clamp of Categorical

// V consecutive pixels of the C channel planes at base: z[pixel][class]
template <int C, int V>
__device__ __forceinline__ void fm_load(const float* __restrict__ base, long long S, float (&z)[V][C]) {
    if constexpr (V == 4) {
        mis_tail_load4<C>(base, S, z);
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) z[0][c] = base[(long long)c * S];
    }
}

template <int C, int V>
__device__ __forceinline__ void fm_store(float* __restrict__ base, long long S, const float (&o)[V][C]) {
    if constexpr (V == 4) {
        mis_tail_store4<C>(base, S, o);
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) base[(long long)c * S] = o[0][c];
    }
}

// The decisions of one pixel from its weak softmax, the reference's fp32 expressions: the mask ((p - min) / max > tau), the
// pseudo label argmax(p * mask) and the complementary label argmin(p); first extremum wins, as torch.argmax / torch.argmin.
template <int C>
__device__ __forceinline__ void fm_decide(const float (&p)[C], float tau, int& pseudo, int& comp, bool& any) {
    float mn = p[0], mx = p[0];
    comp = 0;
#pragma unroll
    for (int c = 1; c < C; ++c) {
        if (p[c] < mn) { mn = p[c]; comp = c; }
        mx = fmaxf(mx, p[c]);
    }
    float best = 0.f;
    pseudo = 0;
    any = false;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const bool in = (p[c] - mn) / mx > tau;
        const float v = in ? p[c] : 0.f;
        any = any || in;
        if (c == 0) best = v;
        else if (v > best) { best = v; pseudo = c; }
    }
}

// cross-entropy whose "logits" are x = 1 - p (all in [0, 1]: no shift needed): returns logsumexp(x) - x_y and e = softmax(x)
template <int C>
__device__ __forceinline__ float fm_comp_ce(const float (&p)[C], int y, float (&e)[C]) {
    float sum = 0.f, xy = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float x = 1.f - p[c];
        e[c] = expf(x);
        sum += e[c];
        if (c == y) xy = x;
    }
    const float inv = 1.f / sum;
#pragma unroll
    for (int c = 0; c < C; ++c) e[c] *= inv;
    return logf(sum) - xy;
}

// partial layout of pass 1 per workgroup, NP1 = 4 + 7C floats:
//   [0] ce_sup  [1 + 3c ..] (I, Y, Z)_c labeled   [1 + 3C] ce_u  [2 + 3C + 3c ..] (I, Y, Z)_c pseudo-labeled
//   [2 + 6C] ce_comp  [3 + 6C] pixels the mask kept a class of  [4 + 6C + c] A_c
template <int C, int V>
__global__ __launch_bounds__(256) void fm_pass1_kernel(const FArgs a, float* __restrict__ part,
                                                       unsigned char* __restrict__ pseudo_map,
                                                       unsigned char* __restrict__ comp_map) {
    constexpr int NP = 4 + 7 * C;
    __shared__ float red[4 * NP];
    float v[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) v[i] = 0.f;
    const int b = blockIdx.x / a.nbs, j0 = blockIdx.x - b * a.nbs;
    const long long units = a.S / V;
    const float* __restrict__ wb = a.zw + (long long)b * a.w_bs;
    const float* __restrict__ sb = a.zs + (long long)b * a.s_bs;
    for (long long u = j0 * 256LL + threadIdx.x; u < units; u += (long long)a.nbs * 256) {
        const long long px = u * V;
        float zw[V][C], zs[V][C];
        fm_load<C, V>(wb + px, a.S, zw);
        fm_load<C, V>(sb + px, a.S, zs);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float pw[C], ps[C], e[C], lw, ls;
            mis_tail_softmax<C>(zw[j], pw, lw);
            mis_tail_softmax<C>(zs[j], ps, ls);
            int yp, yc;
            bool any;
            fm_decide<C>(pw, a.tau, yp, yc, any);
            if (b < a.L) {
                const int y = mis_tail_label(a.label, a.label_bytes, (long long)b * a.S + px + j);
                mis_tail_labeled_sums<C>(zw[j], pw, lw, y, v[0], v + 1);
            } else {
                mis_tail_labeled_sums<C>(zs[j], ps, ls, yp, v[1 + 3 * C], v + 2 + 3 * C);
                v[3 + 6 * C] += any ? 1.f : 0.f;
                if (pseudo_map) pseudo_map[(long long)(b - a.L) * a.S + px + j] = (unsigned char)yp;
            }
            v[2 + 6 * C] += fm_comp_ce<C>(ps, yc, e);
            if (comp_map) comp_map[(long long)b * a.S + px + j] = (unsigned char)yc;
#pragma unroll
            for (int c = 0; c < C; ++c) v[4 + 6 * C + c] += ps[c];
        }
    }
    fm_block_sum<NP>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NP; ++i) part[(long long)blockIdx.x * NP + i] = v[i];
    }
}

// Column sums of `rows` rows of n <= 32 values (row stride n), all 256 threads of the workgroup: lane pair (i, r) = (thread
// % 32, thread / 32) adds rows r, r + 8, .. of column i in double -- a row is one coalesced read, the loads of a thread are
// independent -- and the eight row lanes are added in a fixed order.  tot[i], i < n, is valid for every thread on return.
// (mis_tail_reduce_parts takes a turn of the whole workgroup per column: 32 columns of 1536 partial rows were 44 us.)
template <typename T>
__device__ __forceinline__ void fm_column_sums(const T* __restrict__ src, int rows, int n, double* tot) {
    __shared__ double sm[8][32];
    const int i = threadIdx.x & 31, r = threadIdx.x >> 5;
    double s = 0.0;
    if (i < n) {
#pragma unroll 8
        for (int row = r; row < rows; row += 8) s += (double)src[(long long)row * n + i];
    }
    __syncthreads();                      // a previous call's readers are done with sm
    sm[r][i] = s;
    __syncthreads();
    if ((int)threadIdx.x < n) {
        const int t = threadIdx.x;
        tot[t] = ((sm[0][t] + sm[1][t]) + (sm[2][t] + sm[3][t])) + ((sm[4][t] + sm[5][t]) + (sm[6][t] + sm[7][t]));
    }
    __syncthreads();
}

// dst[b][i] = sum over the nbs workgroups j of sample b of part[(b * nbs + j) * n + i], i < n: one workgroup per sample, in
// double (kept in double: A rounded to fp32 would shift every q = ps / A of its (sample, class) the same way)
__global__ __launch_bounds__(256) void fm_rows_kernel(const float* __restrict__ part, int nbs, int n,
                                                      double* __restrict__ dst) {
    __shared__ double tot[32];
    const int b = blockIdx.x;
    fm_column_sums(part + (long long)b * nbs * n, nbs, n, tot);
    if ((int)threadIdx.x < n) dst[(long long)b * n + threadIdx.x] = tot[threadIdx.x];
}

// f(q) = -q log(clamp(q, eps, 1 - eps)): Categorical(probs = q).entropy() is H = sum_s f(q_s), and the adaptive weight needs
// 1 - H / ln S with H / ln S close to 1.  Summing H in fp32 and subtracting loses what is left: the rounding of the few
// distinct values a softmax takes does not average out over the pixels (measured: 1.7e-6 in the weight where fp32 torch
// is at 5e-8).  With sum_s q_s = 1 the difference is summed directly, ln S - H = sum_s q log(S clamp(q)) =: K: every term
// is O(q), S clamp(q) is one rounding away from exact and the logarithm is taken near 1.
// lsq = log(S clamp(q)); in = [eps <= q <= 1 - eps] (the clamp passes a gradient inside its bounds, both included, as
// torch.clamp), so f'(q) = -log clamp(q) - in = ln S - lsq - in.
__device__ __forceinline__ void fm_entropy_terms(float q, float Sf, float& lsq, float& in) {
    lsq = logf(Sf * fminf(fmaxf(q, FM_EPS), 1.f - FM_EPS));
    in = (q >= FM_EPS && q <= 1.f - FM_EPS) ? 1.f : 0.f;
}

// partial layout of pass 2 per workgroup, 2C floats: [c] K_c = sum q lsq,  [C + c] R_c = sum q in
template <int C, int V>
__global__ __launch_bounds__(256) void fm_pass2_kernel(const FArgs a, const double* __restrict__ samp1,
                                                       float* __restrict__ part) {
    constexpr int NP = 2 * C;
    __shared__ float red[4 * NP];
    float v[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) v[i] = 0.f;
    const int b = blockIdx.x / a.nbs, j0 = blockIdx.x - b * a.nbs;
    double rA[C];
#pragma unroll
    for (int c = 0; c < C; ++c) rA[c] = 1.0 / samp1[b * (4 + 7 * C) + 4 + 6 * C + c];
    const long long units = a.S / V;
    const float Sf = (float)a.S;
    const float* __restrict__ sb = a.zs + (long long)b * a.s_bs;
    for (long long u = j0 * 256LL + threadIdx.x; u < units; u += (long long)a.nbs * 256) {
        float zs[V][C];
        fm_load<C, V>(sb + u * V, a.S, zs);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float ps[C], ls;
            mis_tail_softmax<C>(zs[j], ps, ls);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float q = (float)((double)ps[c] * rA[c]);
                float lsq, in;
                fm_entropy_terms(q, Sf, lsq, in);
                v[c] += q * lsq;
                v[C + c] += q * in;
            }
        }
    }
    fm_block_sum<NP>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NP; ++i) part[(long long)blockIdx.x * NP + i] = v[i];
    }
}

// out[0]=loss [1]=sup_ce [2]=sup_dice [3]=unsup [4]=w [5]=ce_u [6]=dice_u [7]=ce_comp [8]=as_weight [9]=masked-in fraction
// coef[0]=labeled CE scale, [1]=pseudo-label CE scale, [2]=complementary CE scale, [3]=entropy scale,
// coef[4 + 2c], [5 + 2c] = a_c, b_c of the labeled Dice, coef[4 + 2 MIS_MAXC + 2c], [.. + 1] = of the pseudo-label Dice
constexpr int FM_NCOEF = 4 + 4 * MIS_MAXC;

struct FFinalArgs {
    const double* samp1; const double* samp2;       // the per-sample sums of pass 1 [B][4 + 7C] and of pass 2 [B][2C]
    int B, L, C; long long S;
    float cons_weight; const MisStepState* st;
    float* out; float* coef;
};

__global__ __launch_bounds__(256) void fm_final_kernel(const FFinalArgs f) {
    __shared__ double tot[32 + 2 * MIS_MAXC];
    const int C = f.C;
    fm_column_sums(f.samp1, f.B, 4 + 7 * C, tot);                           // (the A columns are summed too, and not used)
    fm_column_sums(f.samp2, f.B, 2 * C, tot + 32);                          // K_c summed over every sample
    if (threadIdx.x != 0) return;
    const double S = (double)f.S;
    const double nlab = (double)f.L * S, nun = (double)(f.B - f.L) * S, nall = (double)f.B * S;
    const double w = f.st ? (double)f.st->cons_weight : (double)f.cons_weight;
    const double ce_sup = tot[0] / nlab, ce_u = tot[1 + 3 * C] / nun, ce_comp = tot[2 + 6 * C] / nall;
    double dice_sup = 0.0, dice_u = 0.0, ksum = 0.0;
    for (int c = 0; c < C; ++c) {
        double dl, ac, bc;
        mis_tail_dice_coef(tot[1 + 3 * c], tot[2 + 3 * c], tot[3 + 3 * c], 1.0, C, dl, ac, bc);
        dice_sup += dl;
        f.coef[4 + 2 * c] = (float)ac;
        f.coef[5 + 2 * c] = (float)bc;
        mis_tail_dice_coef(tot[2 + 3 * C + 3 * c], tot[3 + 3 * C + 3 * c], tot[4 + 3 * C + 3 * c], w, C, dl, ac, bc);
        dice_u += dl;
        f.coef[4 + 2 * MIS_MAXC + 2 * c] = (float)ac;
        f.coef[5 + 2 * MIS_MAXC + 2 * c] = (float)bc;
        ksum += tot[32 + c];
    }
    dice_sup /= C;
    dice_u /= C;
    const double norm = (double)f.B * C * log(S);
    const double as = ksum / norm;                             // mean_{b,c} (1 - H_bc / ln S) = mean K_bc / ln S
    const double unsup = ce_u + dice_u + as * as * ce_comp;
    f.out[0] = (float)(ce_sup + dice_sup + w * unsup);
    f.out[1] = (float)ce_sup; f.out[2] = (float)dice_sup; f.out[3] = (float)unsup; f.out[4] = (float)w;
    f.out[5] = (float)ce_u; f.out[6] = (float)dice_u; f.out[7] = (float)ce_comp; f.out[8] = (float)as;
    f.out[9] = (float)(tot[3 + 6 * C] / nun);
    f.coef[0] = (float)(1.0 / nlab);
    f.coef[1] = (float)(w / nun);
    f.coef[2] = (float)(w * as * as / nall);
    f.coef[3] = (float)(-2.0 * w * as * ce_comp / norm);       // dloss/da * da/dH_bc
}

// d_weak: the supervised gradient on the labeled rows, zeros on the others (mask and both label maps are detached).
// d_strong = ps_c (g_c - sum_j g_j ps_j) [+ CE term], g = dloss/dps:
//   complementary CE:  -k2 (softmax(1 - ps)_c - [c == comp])
//   adaptive weight:    k3 (f'(q_c) - T_bc) / A_bc,  f'(q) - T = (K_bc + R_bc) - lsq - in   (T_bc = sum_s q f'(q))
//   rows >= L:          the pseudo-label Dice (b_c ps_c + [pseudo == c] a_c) and CE k1 (ps_c - [c == pseudo])
template <int C, int V>
__global__ __launch_bounds__(256) void fm_grad_kernel(const FArgs a, const float* __restrict__ coef,
                                                      const double* __restrict__ samp1, const double* __restrict__ samp2,
                                                      float* __restrict__ dw, long long dw_bs, float* __restrict__ ds,
                                                      long long ds_bs) {
    const float k0 = coef[0], k1 = coef[1], k2 = coef[2], k3 = coef[3];
    float al[C], bl[C], au[C], bu[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        al[c] = coef[4 + 2 * c]; bl[c] = coef[5 + 2 * c];
        au[c] = coef[4 + 2 * MIS_MAXC + 2 * c]; bu[c] = coef[5 + 2 * MIS_MAXC + 2 * c];
    }
    const int b = blockIdx.x / a.nbs, j0 = blockIdx.x - b * a.nbs;
    double rA[C];
    float rAf[C], T[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        rA[c] = 1.0 / samp1[b * (4 + 7 * C) + 4 + 6 * C + c]; rAf[c] = (float)rA[c];
        T[c] = (float)(samp2[b * 2 * C + c] + samp2[b * 2 * C + C + c]);
    }
    const long long units = a.S / V;
    const float Sf = (float)a.S;
    const float* __restrict__ wb = a.zw + (long long)b * a.w_bs;
    const float* __restrict__ sb = a.zs + (long long)b * a.s_bs;
    for (long long u = j0 * 256LL + threadIdx.x; u < units; u += (long long)a.nbs * 256) {
        const long long px = u * V;
        float zw[V][C], zs[V][C], ow[V][C], os[V][C];
        fm_load<C, V>(wb + px, a.S, zw);
        fm_load<C, V>(sb + px, a.S, zs);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float pw[C], ps[C], e[C], lw, ls;
            mis_tail_softmax<C>(zw[j], pw, lw);
            mis_tail_softmax<C>(zs[j], ps, ls);
            int yp, yc;
            bool any;
            fm_decide<C>(pw, a.tau, yp, yc, any);
            if (b < a.L) {
                const int y = mis_tail_label(a.label, a.label_bytes, (long long)b * a.S + px + j);
                mis_tail_labeled_grad<C>(pw, y, k0, al, bl, ow[j]);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) ow[j][c] = 0.f;
            }
            fm_comp_ce<C>(ps, yc, e);
            float g[C], dot = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float lsq, in;
                fm_entropy_terms((float)((double)ps[c] * rA[c]), Sf, lsq, in);
                g[c] = k3 * (T[c] - lsq - in) * rAf[c] - k2 * (e[c] - (c == yc ? 1.f : 0.f));
                if (b >= a.L) g[c] += bu[c] * ps[c] + (c == yp ? au[c] : 0.f);
                dot += g[c] * ps[c];
            }
            const float kce = b >= a.L ? k1 : 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) os[j][c] = fmaf(ps[c], g[c] - dot, kce * (ps[c] - (c == yp ? 1.f : 0.f)));
        }
        if (dw) fm_store<C, V>(dw + (long long)b * dw_bs + px, a.S, ow);
        if (ds) fm_store<C, V>(ds + (long long)b * ds_bs + px, a.S, os);
    }
}

// workgroups per sample of the streaming passes: one unit (V pixels) per thread, at most 2048 workgroups in all
int fm_nbs(int B, long long units) {
    long long nbs = mis_cdiv(units, 256), cap = 2048 / B;
    if (cap < 1) cap = 1;
    if (nbs > cap) nbs = cap;
    if (nbs < 1) nbs = 1;
    return (int)nbs;
}

template <int C> constexpr auto fm_pass1_vec = fm_pass1_kernel<C, 4>;
template <int C> constexpr auto fm_pass1_one = fm_pass1_kernel<C, 1>;
template <int C> constexpr auto fm_pass2_vec = fm_pass2_kernel<C, 4>;
template <int C> constexpr auto fm_pass2_one = fm_pass2_kernel<C, 1>;
template <int C> constexpr auto fm_grad_vec = fm_grad_kernel<C, 4>;
template <int C> constexpr auto fm_grad_one = fm_grad_kernel<C, 1>;

}  // namespace

extern "C" long long mis_color_jitter_workspace_bytes(int B, long long S) {
    if (B <= 0 || S <= 0) return MIS_ERR_ARG;
    return (long long)B * mis_cdiv(S, JCH) * (long long)sizeof(float);
}

// x: [B][1][S] weak images (batch stride x_bs), y: the strong images.  params ([B][3] floats: beta, gamma, order; order 0 =
// brightness first) or, when it is nullptr, a draw keyed by (state->seed, state->iter_num, salt).
extern "C" int mis_color_jitter(const float* x, long long x_bs, float* y, long long y_bs, int B, long long S,
                                const float* params, const MisStepState* state, unsigned salt, float* drawn,
                                void* workspace, long long workspace_bytes, hipStream_t stream) {
    if (!x || !y || !workspace || B <= 0 || S <= 0 || x_bs < S || y_bs < S) return MIS_ERR_ARG;
    if (!params && !state) return MIS_ERR_ARG;
    const long long nch = mis_cdiv(S, JCH), nb = nch * B;
    if (nb > 0x7FFFFFFFLL) return MIS_ERR_UNSUPPORTED;
    if (workspace_bytes < mis_color_jitter_workspace_bytes(B, S)) return MIS_ERR_WORKSPACE;
    const bool vec = S % 4 == 0 && x_bs % 4 == 0 && y_bs % 4 == 0 && mis_aligned16(x) && mis_aligned16(y);
    JArgs a{x, x_bs, y, y_bs, S, (int)nch, params, state, (uint32_t)salt, drawn};
    float* part = reinterpret_cast<float*>(workspace);
    const float* cpart = part;
    if (vec) {
        hipLaunchKernelGGL(jitter_sum_kernel<4>, dim3((unsigned)nb), dim3(256), 0, stream, a, part);
        hipLaunchKernelGGL(jitter_apply_kernel<4>, dim3((unsigned)nb), dim3(256), 0, stream, a, cpart);
    } else {
        hipLaunchKernelGGL(jitter_sum_kernel<1>, dim3((unsigned)nb), dim3(256), 0, stream, a, part);
        hipLaunchKernelGGL(jitter_apply_kernel<1>, dim3((unsigned)nb), dim3(256), 0, stream, a, cpart);
    }
    return mis_launch_status();
}

extern "C" long long mis_fixmatch_tail_workspace_bytes(int B, int C, long long S) {
    if (B <= 0 || C <= 0 || C > MIS_MAXC || S <= 0) return MIS_ERR_ARG;
    const long long blocks = (long long)B * fm_nbs(B, S);            // the scalar path has the most workgroups
    // per-sample sums [B][4 + 9C] in double, partials [blocks][4 + 9C], coefficients
    return (long long)B * (4 + 9 * C) * (long long)sizeof(double) + (blocks * (4 + 9 * C) + FM_NCOEF) * (long long)sizeof(float);
}

// weak / strong: [B][C][S] logits of one network; label: [L][S]; out >= 10 floats (device).  d_weak / d_strong: either
// may be nullptr.  pseudo ([B - L][S]) / comp ([B][S]): the decision maps, uint8, may be nullptr.
extern "C" int mis_fixmatch_tail(const float* weak, long long w_bs, const float* strong, long long s_bs,
                                 const void* label, int label_bytes, int B, int L, int C, long long S, float conf_thresh,
                                 float cons_weight, const MisStepState* state, float* out, float* d_weak,
                                 long long dw_bs, float* d_strong, long long ds_bs, unsigned char* pseudo,
                                 unsigned char* comp, void* workspace, long long workspace_bytes, hipStream_t stream) {
    if (!weak || !strong || !label || !out || !workspace || C <= 0) return MIS_ERR_ARG;
    if (!(1 <= L && L < B) || S <= 1) return MIS_ERR_ARG;
    if (label_bytes != 1 && label_bytes != 8) return MIS_ERR_ARG;
    if (C != 2 && C != 3 && C != 4) return MIS_ERR_UNSUPPORTED;
    const long long plane = (long long)C * S;
    if (w_bs < plane || s_bs < plane || (d_weak && dw_bs < plane) || (d_strong && ds_bs < plane)) return MIS_ERR_ARG;
    if (workspace_bytes < mis_fixmatch_tail_workspace_bytes(B, C, S)) return MIS_ERR_WORKSPACE;
    const bool vec = S % 4 == 0 && w_bs % 4 == 0 && s_bs % 4 == 0 && mis_aligned16(weak) && mis_aligned16(strong) &&
                     (!d_weak || (dw_bs % 4 == 0 && mis_aligned16(d_weak))) &&
                     (!d_strong || (ds_bs % 4 == 0 && mis_aligned16(d_strong)));
    const int nbs = fm_nbs(B, vec ? S >> 2 : S);
    const int blocks = B * nbs;
    FArgs a{weak, w_bs, strong, s_bs, label, label_bytes, B, L, S, conf_thresh, nbs};
    if ((uintptr_t)workspace & 7) return MIS_ERR_ARG;
    const int np1 = 4 + 7 * C, np2 = 2 * C;
    double* samp1 = reinterpret_cast<double*>(workspace);
    double* samp2 = samp1 + (long long)B * np1;
    float* part1 = reinterpret_cast<float*>(samp2 + (long long)B * np2);
    float* part2 = part1 + (long long)blocks * np1;
    float* coef = part2 + (long long)blocks * np2;
    const float *cpart1 = part1, *cpart2 = part2, *ccoef = coef;
    const double *csamp1 = samp1, *csamp2 = samp2;
    if (vec) {
        MIS_DISPATCH_C(C, fm_pass1_vec, blocks, stream, a, part1, pseudo, comp)
    } else {
        MIS_DISPATCH_C(C, fm_pass1_one, blocks, stream, a, part1, pseudo, comp)
    }
    hipLaunchKernelGGL(fm_rows_kernel, dim3(B), dim3(256), 0, stream, cpart1, nbs, np1, samp1);
    if (vec) {
        MIS_DISPATCH_C(C, fm_pass2_vec, blocks, stream, a, csamp1, part2)
    } else {
        MIS_DISPATCH_C(C, fm_pass2_one, blocks, stream, a, csamp1, part2)
    }
    hipLaunchKernelGGL(fm_rows_kernel, dim3(B), dim3(256), 0, stream, cpart2, nbs, np2, samp2);
    FFinalArgs f{csamp1, csamp2, B, L, C, S, cons_weight, state, out, coef};
    hipLaunchKernelGGL(fm_final_kernel, dim3(1), dim3(256), 0, stream, f);
    if (d_weak || d_strong) {
        if (vec) {
            MIS_DISPATCH_C(C, fm_grad_vec, blocks, stream, a, ccoef, csamp1, csamp2, d_weak, dw_bs, d_strong, ds_bs)
        } else {
            MIS_DISPATCH_C(C, fm_grad_one, blocks, stream, a, ccoef, csamp1, csamp2, d_weak, dw_bs, d_strong, ds_bs)
        }
    }
    return mis_launch_status();
}
