// Pixel-wise contrastive (PatchNCE) loss of the reference's contrastive trainers, forward and gradient, without an N x N
// object in memory.
//
// Replaces (reference):
//   losses.ConLoss(temperature)(feat_q, feat_k)                code/utils/losses.py:283-337
//   losses.contrastive_loss_sup(temperature)(feat_q, feat_k)   code/utils/losses.py:479-531 (the same arithmetic)
//
// With q^_i = f_i / max(|f_i|_1, 1e-12), k^_j likewise (detached) and s_ij = q^_i . k^_j / T inside one sample, the
// reference's positive column plus its diagonal-masked negatives are the whole row {s_ij : j}, so
//   loss = mean_i ( logsumexp_j s_ij - s_ii ),    d loss / d q^_i = (softmax_j(s_i.) K^ - k^_i) / (B N T):
// attention with V = K^, read off at the diagonal.  Four launches:
//   prep      L1-normalises both inputs once: q^/T and k^ pixel-major [B][Np][d] (the operands of the score product),
//             k^ channel-major [B][d][Np] (the operand of P.K^); Np = N rounded up to 64, the padding is zeros.
//   rows      one wave per 16 query rows walks the keys 64 at a time on v_mfma_f32_16x16x4_f32.  The score product is
//             swapped, S^T = K^ Q^^T: a lane then holds 16 scores of ONE query (column lane & 15; keys 16t + 4(lane >> 4)
//             + r), the online softmax needs two cross-lane steps per 64 keys, and the probabilities are already the B
//             operand of O^T += K^^T P^T (k index = lane >> 4 on both sides, so step (t, r) contracts the keys
//             16t + 4g + r, which is component r of one float4 of the channel-major k^).  Every operand is a float4 load
//             from the workspace (L2-resident: one sample's k^ is N d 4 bytes); no LDS, no barrier.  The wave that meets
//             its own diagonal tile keeps s_ii from the same accumulator the row statistics see, so logsumexp - s_ii is
//             exactly 0 where it must be (N = 1).
//   epilogue  per row: the loss terms as fixed-order per-workgroup partials, and the backward of the normalisation,
//             df = (dq^ - sign(f) (dq^ . q^)) / max(|f|_1, 1e-12), written channel-major.
//   finalize  one workgroup sums the partials in double (mis_tail_reduce_parts).
// No atomics anywhere: run-to-run identical.
#include "tail.h"

namespace {

constexpr float PN_EPS = 1e-12f;                 // F.normalize's eps
constexpr float PN_LOG2E = 1.4426950408889634f;
constexpr int PN_KEYS = 64;                      // keys per step of the row walk = granularity of the padding
constexpr long long PN_MAX_N = 1LL << 22;        // the row kernels index one sample's planes with 32-bit ints

static inline long long pn_pad(long long N) { return mis_cdiv(N, PN_KEYS) * PN_KEYS; }

struct PnLayout {
    long long plane;    // floats of one [B][Np][d] image
    long long rows;     // floats of one [B][Np] vector
    int epi_blocks;     // workgroups of the epilogue = partials
    long long floats;
};

static inline PnLayout pn_layout(int B, int d, long long N) {
    PnLayout l;
    const long long Np = pn_pad(N);
    l.plane = (long long)B * Np * d;
    l.rows = (long long)B * Np;
    l.epi_blocks = (int)(B * mis_cdiv(N, 256));
    l.floats = 4 * l.plane + 2 * l.rows + 3LL * l.epi_blocks;
    return l;
}

// grid (Np / 256 rounded up, B, 2): z == 0 normalises feat_q (times 1 / T), z == 1 feat_k
template <int D>
__global__ __launch_bounds__(256) void pnce_prep_kernel(const float* __restrict__ fq, long long q_bs,
                                                        const float* __restrict__ fk, long long k_bs, int N, int Np,
                                                        float inv_t, float* __restrict__ qT, float* __restrict__ kT,
                                                        float* __restrict__ kC) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Np) return;
    const int b = blockIdx.y;
    const bool is_k = blockIdx.z != 0;
    const float* __restrict__ src = is_k ? fk + (long long)b * k_bs : fq + (long long)b * q_bs;
    float v[D];
    float n1 = 0.f;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        v[c] = p < N ? src[(long long)c * N + p] : 0.f;
        n1 += fabsf(v[c]);
    }
    const float den = fmaxf(n1, PN_EPS);
    const float post = is_k ? 1.f : inv_t;
#pragma unroll
    for (int c = 0; c < D; ++c) v[c] = v[c] / den * post;
    float* __restrict__ dst = (is_k ? kT : qT) + ((long long)b * Np + p) * D;
#pragma unroll
    for (int c = 0; c < D; c += 4) *reinterpret_cast<float4*>(dst + c) = make_float4(v[c], v[c + 1], v[c + 2], v[c + 3]);
    if (is_k) {
#pragma unroll
        for (int c = 0; c < D; ++c) kC[((long long)b * D + c) * Np + p] = v[c];
    }
}

__device__ __forceinline__ float pn_xor16(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), (0x10 << 10) | 0x1F));
}

// One wave per 16 query rows; blockDim.x / 64 waves per workgroup, all independent.  The 1-D grid is padded to a multiple
// of 8 and remapped so that the workgroups of one sample share an XCD's L2.
template <int D, bool GRAD>
__global__ __launch_bounds__(256) void pnce_rows_kernel(const float* __restrict__ qT, const float* __restrict__ kT,
                                                        const float* __restrict__ kC, float* __restrict__ oC,
                                                        float* __restrict__ lse, float* __restrict__ sii, int N, int Np,
                                                        int tiles, int wgs_per_sample, int wgs, int wgs_padded) {
    constexpr int KS = D / 4;     // MFMA k-steps of a score tile; lane group g owns the channels g * KS .. g * KS + KS - 1
    constexpr int OT = D / 16;    // 16-channel tiles of O^T
    const unsigned wg = mis_xcd_remap(blockIdx.x, wgs_padded);
    if (wg >= (unsigned)wgs) return;
    const int b = wg / wgs_per_sample;
    const int tile = (wg - b * wgs_per_sample) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (tile >= tiles) return;
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const int q0 = tile * 16;
    const float* __restrict__ qTb = qT + (long long)b * Np * D;
    const float* __restrict__ kTb = kT + (long long)b * Np * D;
    const float* __restrict__ kCb = kC + (long long)b * D * Np;

    float qv[KS];
#pragma unroll
    for (int i = 0; i < KS; i += 4) {
        const float4 t4 = *reinterpret_cast<const float4*>(qTb + (long long)(q0 + j) * D + g * KS + i);
        qv[i] = t4.x; qv[i + 1] = t4.y; qv[i + 2] = t4.z; qv[i + 3] = t4.w;
    }

    f32x4 o[OT];
#pragma unroll
    for (int c = 0; c < OT; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f, diag = 0.f;
    const int diag_kb = q0 & ~(PN_KEYS - 1);

    for (int kb = 0; kb < Np; kb += PN_KEYS) {
        // S^T tile t: rows = keys kb + 16t .. + 15, columns = the 16 queries
        f32x4 s[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float kv[KS];
#pragma unroll
            for (int i = 0; i < KS; i += 4) {
                const float4 t4 = *reinterpret_cast<const float4*>(kTb + (long long)(kb + 16 * t + j) * D + g * KS + i);
                kv[i] = t4.x; kv[i + 1] = t4.y; kv[i + 2] = t4.z; kv[i + 3] = t4.w;
            }
            s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < KS; ++i) s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[i], qv[i], s[t], 0, 0, 0);
        }
        if (kb + PN_KEYS > N) {      // the padded keys: out of the softmax
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kb + 16 * t + 4 * g + r >= N) s[t][r] = -INFINITY;
        }
        if (kb == diag_kb) {         // this wave's own pixels are among these keys
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kb + 16 * t + 4 * g + r == q0 + j) diag = s[t][r];
        }
        float tmax = s[0][0];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) tmax = fmaxf(tmax, s[t][r]);
        tmax = fmaxf(tmax, pn_xor16(tmax));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m, tmax);     // finite: key kb < N is in every step
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * PN_LOG2E);
        m = mn;
        float psum = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f((s[t][r] - mn) * PN_LOG2E);
                s[t][r] = p;
                psum += p;
            }
        l = fmaf(l, alpha, psum);
        if (GRAD) {
#pragma unroll
            for (int c = 0; c < OT; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[c][r] *= alpha;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int c = 0; c < OT; ++c) {
                    // O^T[channel 16c + j][query] += sum over g of k^[channel][key kb + 16t + 4g + r] P[key][query]
                    const float4 ka = *reinterpret_cast<const float4*>(kCb + (long long)(16 * c + j) * Np + kb + 16 * t + 4 * g);
                    o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka.x, s[t][0], o[c], 0, 0, 0);
                    o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka.y, s[t][1], o[c], 0, 0, 0);
                    o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka.z, s[t][2], o[c], 0, 0, 0);
                    o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka.w, s[t][3], o[c], 0, 0, 0);
                }
        }
    }

    // the four lane groups of a query: (l0 + l1) + (l2 + l3) in every one of them; diag is non-zero in one group only
    l += pn_xor16(l);
    l += __shfl_xor(l, 32, 64);
    diag += pn_xor16(diag);
    diag += __shfl_xor(diag, 32, 64);
    if (g == 0 && q0 + j < N) {
        lse[(long long)b * Np + q0 + j] = m + logf(l);
        sii[(long long)b * Np + q0 + j] = diag;
    }
    if (GRAD) {
        // lane holds O^T[channel 16c + 4g + r][query q0 + j]; rows >= N land in the padding
        float* __restrict__ oCb = oC + (long long)b * D * Np;
#pragma unroll
        for (int c = 0; c < OT; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) oCb[(long long)(16 * c + 4 * g + r) * Np + q0 + j] = o[c][r] / l;
    }
}

// grid (N / 256 rounded up, B): the loss terms of 256 rows as one partial, and dfeat_q when asked for
template <int D>
__global__ __launch_bounds__(256) void pnce_epilogue_kernel(const float* __restrict__ fq, long long q_bs, int N, int Np,
                                                            const float* __restrict__ kC, const float* __restrict__ oC,
                                                            const float* __restrict__ lse, const float* __restrict__ sii,
                                                            float coef, float* __restrict__ dq, long long dq_bs,
                                                            float* __restrict__ part) {
    __shared__ double red[4 * 3];
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    double v[3] = {0.0, 0.0, 0.0};
    if (p < N) {
        const float ls = lse[(long long)b * Np + p], sd = sii[(long long)b * Np + p];
        v[0] = (double)(ls - sd);
        v[1] = (double)sd;
        v[2] = (double)ls;
        if (dq != nullptr) {
            const float* __restrict__ src = fq + (long long)b * q_bs + p;
            float f[D], gq[D];
            float n1 = 0.f;
#pragma unroll
            for (int c = 0; c < D; ++c) {
                f[c] = src[(long long)c * N];
                n1 += fabsf(f[c]);
            }
            const float den = fmaxf(n1, PN_EPS);
            float dot = 0.f;
#pragma unroll
            for (int c = 0; c < D; ++c) {
                const long long at = ((long long)b * D + c) * Np + p;
                gq[c] = coef * (oC[at] - kC[at]);
                dot = fmaf(gq[c], f[c] / den, dot);
            }
            if (!(n1 >= PN_EPS)) dot = 0.f;      // the clamp passes no gradient to the norm below eps
            float* __restrict__ dst = dq + (long long)b * dq_bs + p;
#pragma unroll
            for (int c = 0; c < D; ++c) {
                const float sg = f[c] > 0.f ? 1.f : (f[c] < 0.f ? -1.f : 0.f);
                dst[(long long)c * N] = (gq[c] - sg * dot) / den;
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = mis_wave_sum_d(v[i]);
    if (lane == 0)
        for (int i = 0; i < 3; ++i) red[wave * 3 + i] = v[i];
    __syncthreads();
    if (threadIdx.x < 3) {
        const int i = threadIdx.x;
        part[((long long)blockIdx.y * gridDim.x + blockIdx.x) * 3 + i] =
            (float)((red[i] + red[3 + i]) + (red[6 + i] + red[9 + i]));
    }
}

// out = [loss, mean_i s_ii, mean_i logsumexp_j s_ij]
__global__ __launch_bounds__(256) void pnce_final_kernel(const float* __restrict__ part, int blocks, double inv_rows,
                                                         float* __restrict__ out) {
    __shared__ double tot[3];
    mis_tail_reduce_parts(part, blocks, 3, 3, tot);
    if (threadIdx.x < 3) out[threadIdx.x] = (float)(tot[threadIdx.x] * inv_rows);
}

// CUs of the current device, asked once (every device of a process is the same part)
static int pn_cu_count() {
    static std::atomic<int> cached{0};
    int n = cached.load(std::memory_order_relaxed);
    if (n > 0) return n;
    int dev = 0;
    n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
        return 256;
    cached.store(n, std::memory_order_relaxed);
    return n;
}

template <int D>
int pn_launch(const float* fq, long long q_bs, const float* fk, long long k_bs, int B, int N, float temperature,
              float grad_scale, float* out, float* dq, long long dq_bs, float* ws, hipStream_t stream) {
    const PnLayout lay = pn_layout(B, D, N);
    const int Np = (int)pn_pad(N);
    float* qT = ws;
    float* kT = qT + lay.plane;
    float* kC = kT + lay.plane;
    float* oC = kC + lay.plane;
    float* lse = oC + lay.plane;
    float* sii = lse + lay.rows;
    float* part = sii + lay.rows;

    hipLaunchKernelGGL((pnce_prep_kernel<D>), dim3((unsigned)mis_cdiv(Np, 256), B, 2), dim3(256), 0, stream, fq, q_bs, fk,
                       k_bs, N, Np, (float)(1.0 / (double)temperature), qT, kT, kC);

    // as attention_full.hip sizes its grid: fewer rows per workgroup until the launch covers the CUs, where B * N allows
    const int cus = pn_cu_count();
    const int tiles = (int)mis_cdiv(N, 16);
    int waves = 4;
    while (waves > 1 && (long long)B * mis_cdiv(tiles, waves) < cus) waves >>= 1;
    const int wgs_per_sample = (int)mis_cdiv(tiles, waves);
    const int wgs = B * wgs_per_sample;
    const int wgs_padded = (int)mis_cdiv(wgs, MIS_NUM_XCD) * MIS_NUM_XCD;
    if (dq != nullptr)
        hipLaunchKernelGGL((pnce_rows_kernel<D, true>), dim3(wgs_padded), dim3(64 * waves), 0, stream, qT, kT, kC, oC, lse,
                           sii, N, Np, tiles, wgs_per_sample, wgs, wgs_padded);
    else
        hipLaunchKernelGGL((pnce_rows_kernel<D, false>), dim3(wgs_padded), dim3(64 * waves), 0, stream, qT, kT, kC, oC, lse,
                           sii, N, Np, tiles, wgs_per_sample, wgs, wgs_padded);

    const float coef = (float)((double)grad_scale / ((double)B * (double)N * (double)temperature));
    hipLaunchKernelGGL((pnce_epilogue_kernel<D>), dim3((unsigned)mis_cdiv(N, 256), B), dim3(256), 0, stream, fq, q_bs, N, Np,
                       kC, oC, lse, sii, coef, dq, dq_bs, part);
    hipLaunchKernelGGL(pnce_final_kernel, dim3(1), dim3(256), 0, stream, part, lay.epi_blocks,
                       1.0 / ((double)B * (double)N), out);
    return mis_launch_status();
}

static inline int pn_check_geometry(int B, int d, long long N) {
    if (B <= 0 || d <= 0 || N <= 0) return MIS_ERR_ARG;
    if (d != 16 && d != 32) return MIS_ERR_UNSUPPORTED;
    if (N > PN_MAX_N || B > 65535) return MIS_ERR_UNSUPPORTED;
    return MIS_OK;
}

}  // namespace

extern "C" long long mis_patch_nce_workspace_bytes(int B, int d, long long N) {
    const int st = pn_check_geometry(B, d, N);
    if (st != MIS_OK) return st;
    return pn_layout(B, d, N).floats * 4 + 16;      // 16: the images are aligned to 16 bytes inside the caller's buffer
}

extern "C" int mis_patch_nce(const float* feat_q, long long q_bs, const float* feat_k, long long k_bs, int B, int d,
                             long long N, float temperature, float grad_scale, float* out, float* dfeat_q, long long dq_bs,
                             void* workspace, long long workspace_bytes, hipStream_t stream) {
    if (!feat_q || !feat_k || !out || !workspace) return MIS_ERR_ARG;
    if (B <= 0 || d <= 0 || N <= 0 || !(temperature > 0.f)) return MIS_ERR_ARG;
    if (q_bs < (long long)d * N || k_bs < (long long)d * N || (dfeat_q && dq_bs < (long long)d * N)) return MIS_ERR_ARG;
    const int st = pn_check_geometry(B, d, N);
    if (st != MIS_OK) return st;
    if (workspace_bytes < mis_patch_nce_workspace_bytes(B, d, N)) return MIS_ERR_WORKSPACE;
    float* ws = reinterpret_cast<float*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
    if (d == 16)
        return pn_launch<16>(feat_q, q_bs, feat_k, k_bs, B, (int)N, temperature, grad_scale, out, dfeat_q, dq_bs, ws, stream);
    return pn_launch<32>(feat_q, q_bs, feat_k, k_bs, B, (int)N, temperature, grad_scale, out, dfeat_q, dq_bs, ws, stream);
}
