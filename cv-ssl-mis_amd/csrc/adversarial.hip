// Adversarial training of the 3-D nets: the discriminator's convolutions, its head, the segmenter's loss tail, Adam.
//
// Replaces (reference code/networks/discriminator.py:6-55 FC3DDiscriminator, code/train_adversarial_network_3D.py:129-175):
//   nn.Conv3d(Cin, Cout, kernel_size=4, stride=2, padding=1) -> LeakyReLU(0.2) -> Dropout3d(0.5), forward and backward
//   conv0(softmax(outputs)) + conv1(volume)            as ONE convolution whose first channels are read through a softmax
//   AvgPool3d -> Linear(8 ndf, 2) -> F.cross_entropy    forward and backward
//   0.5 * (CE + Dice) + w * consistency_loss ; backward to the student's logits through the softmax
//   torch.optim.Adam(lr, betas=(0.9, 0.99))
//
// The convolution is an implicit GEMM on v_mfma_f32_16x16x4_f32 in three forms that share their tile loaders:
//   forward  y [co][col]          = sum_{ci, tap} w[co][ci][tap] * X[ci, tap][col]         M = Cout, K = 64 Cin
//   dgrad    dx[ci][col of class] = sum_{co, t}   w[co][ci][tap(class, t)] * G[co, t][col]  M = Cin, K = 8 Cout, 8 classes
//   wgrad    dw[co][ci][tap]      = sum_col       G[co][col] * X[ci, tap][col]              M = Cout, N = 64 taps of one ci
// col = (n, od, oh, ow) runs over the output voxels of ALL samples (the deep layers have 216 voxels per sample: the batch
// fills the tiles); X[ci, tap][col] = in[n][ci][2 od - 1 + kd][2 oh - 1 + kh][2 ow - 1 + kw] or 0 in the padding, gathered on
// the load path (the first Cl channels: softmax of the logits, computed where it is read); G = dy * act'(y) * drop, also
// on the load path.  dgrad: an input voxel of parity class (pd, ph, pw) is reached by the 8 taps kd = 1 - pd + 2 td, .. from
// od = jd + pd - td, .. -- each class is a dense kernel-2 convolution of G.
// A workgroup (4 waves) owns a 64 x 64 tile (16 x 64 when M <= 16), stages a chunk of 64 contraction indices of both
// operands in LDS (A rows 68 floats apart, B rows 80: the four k rows of an operand read fall on distinct banks) and each
// wave runs 2 x 2 MFMA tiles over it.  Single-buffered.
// Long contractions with few tiles are cut into slices (forward: over ci; wgrad: over col), one partial tile per slice
// in the workspace, added in slice order by a second launch that also applies the epilogue: no atomics, bit-identical.
#include "tail.h"
#include "adv_common.h"
#include "../../include/mis_hip_adversarial.h"

namespace {

constexpr int NT = 256;
constexpr int LDA = 68;
constexpr int LDX = 80;

// ------------------------------------------------------------------------------------------------ operand sources
struct XSrc {
    const float* x; long long x_bs; int Cx;       // plain channels
    const float* lg; long long l_bs; int Cl;      // softmax-read channels (the first Cl of the convolution's input)
    int D, H, W;
};

// in[n][ci][id][ih][iw], zero outside
__device__ __forceinline__ float adv_load_x(const XSrc& s, int n, int ci, int id, int ih, int iw) {
    if ((unsigned)id >= (unsigned)s.D || (unsigned)ih >= (unsigned)s.H || (unsigned)iw >= (unsigned)s.W) return 0.f;
    const long long S = (long long)s.D * s.H * s.W;
    const long long off = ((long long)id * s.H + ih) * s.W + iw;
    if (ci >= s.Cl) return s.x[(long long)n * s.x_bs + (long long)(ci - s.Cl) * S + off];
    const float* __restrict__ z = s.lg + (long long)n * s.l_bs + off;
    float v[MAXCL], mx = z[0];
    v[0] = mx;
#pragma unroll
    for (int c = 1; c < MAXCL; ++c) {
        v[c] = c < s.Cl ? z[(long long)c * S] : -INFINITY;
        mx = fmaxf(mx, v[c]);
    }
    float sum = 0.f, mine = 0.f;
#pragma unroll
    for (int c = 0; c < MAXCL; ++c) {
        const float e = c < s.Cl ? expf(v[c] - mx) : 0.f;
        sum += e;
        if (c == ci) mine = e;
    }
    return mine * (1.f / sum);
}

struct GSrc {
    const float* dy; long long dy_bs;
    const float* y; long long y_bs;               // the stored activated output (NULL: no activation)
    float slope;
    const float* drop;                            // [N][Cout] or NULL
    int Cout;
};

// dy * act'(y) * drop at (n, co, voxel v of So)
__device__ __forceinline__ float adv_load_g(const GSrc& g, int n, int co, long long So, long long v) {
    float d = g.dy[(long long)n * g.dy_bs + (long long)co * So + v];
    if (g.y) d = g.y[(long long)n * g.y_bs + (long long)co * So + v] > 0.f ? d : d * g.slope;
    if (g.drop) d *= g.drop[(long long)n * g.Cout + co];
    return d;
}

struct Geo {
    int N, Do, Ho, Wo;                            // output (coarse) extent
    long long So, cols;                           // Do * Ho * Wo, N * So
};

__device__ __forceinline__ void adv_col(const Geo& g, long long col, int& n, int& od, int& oh, int& ow) {
    n = (int)(col / g.So);
    const int v = (int)(col - (long long)n * g.So);
    const int hw = g.Ho * g.Wo;
    od = v / hw;
    const int r = v - od * hw;
    oh = r / g.Wo;
    ow = r - oh * g.Wo;
}

// The MFMA loop over one staged chunk of 64 contraction indices: wave tiles (rt[i], ct[j]) of 16 x 16.
template <int TM, int TN>
__device__ __forceinline__ void adv_mma_chunk(const float* lA, const float* lB, const int (&rt)[TM], const int (&ct)[TN],
                                              int kq, int nl, f32x4 (&acc)[TM][TN]) {
#pragma unroll 4
    for (int k0 = 0; k0 < 64; k0 += 4) {
        float av[TM], bv[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) av[i] = lA[(rt[i] * 16 + nl) * LDA + k0 + kq];
#pragma unroll
        for (int j = 0; j < TN; ++j) bv[j] = lB[(k0 + kq) * LDX + ct[j] * 16 + nl];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
}

// wave -> tiles.  BM = 64: waves 2 x 2, each 2 x 2 tiles.  BM = 16: one row tile, wave w owns column tile w.
template <int BM> struct WaveTiles;
template <> struct WaveTiles<64> {
    static constexpr int TM = 2, TN = 2;
    __device__ static void get(int wave, int (&rt)[2], int (&ct)[2]) {
        rt[0] = (wave >> 1) * 2; rt[1] = rt[0] + 1;
        ct[0] = (wave & 1) * 2; ct[1] = ct[0] + 1;
    }
};
template <> struct WaveTiles<16> {
    static constexpr int TM = 1, TN = 1;
    __device__ static void get(int wave, int (&rt)[1], int (&ct)[1]) { rt[0] = 0; ct[0] = wave; }
};

// ------------------------------------------------------------------------------------------------ forward
struct FwdArgs {
    XSrc s;
    const float* w_l; const float* w_x;
    int Cout, Cin;
    Geo g;
    int slices, ci_per;
    float* part;                                  // slices > 1: [slice][Cout][cols]
    const float* bias; const float* bias2;
    float slope;
    const float* drop;
    float* y; long long y_bs;
};

__device__ __forceinline__ void adv_fwd_store(const FwdArgs& a, float v, int co, long long col) {
    const int n = (int)(col / a.g.So);
    const long long vox = col - (long long)n * a.g.So;
    if (a.bias) v += a.bias[co];
    if (a.bias2) v += a.bias2[co];
    v = v > 0.f ? v : v * a.slope;
    if (a.drop) v *= a.drop[(long long)n * a.Cout + co];
    a.y[(long long)n * a.y_bs + (long long)co * a.g.So + vox] = v;
}

template <int BM>
__global__ __launch_bounds__(NT) void k4s2_fwd_kernel(const FwdArgs a) {
    __shared__ float lA[BM * LDA];
    __shared__ float lX[64 * LDX];
    using WT = WaveTiles<BM>;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, kq = lane >> 4, nl = lane & 15;
    const long long col0 = (long long)blockIdx.x * 64;
    const int co0 = blockIdx.y * BM, slice = blockIdx.z;
    const long long gcol = col0 + lane;
    const bool cvalid = gcol < a.g.cols;
    int n = 0, od = 0, oh = 0, ow = 0;
    if (cvalid) adv_col(a.g, gcol, n, od, oh, ow);
    int rt[WT::TM], ct[WT::TN];
    WT::get(wave, rt, ct);
    f32x4 acc[WT::TM][WT::TN];
#pragma unroll
    for (int i = 0; i < WT::TM; ++i)
#pragma unroll
        for (int j = 0; j < WT::TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int c_begin = slice * a.ci_per, c_end = min(a.Cin, c_begin + a.ci_per);
    for (int ci = c_begin; ci < c_end; ++ci) {
        __syncthreads();
        const bool soft = ci < a.s.Cl;
        const float* __restrict__ wsrc = soft ? a.w_l + (long long)ci * 64 : a.w_x + (long long)(ci - a.s.Cl) * 64;
        const long long wrow = (long long)(soft ? a.s.Cl : a.s.Cx) * 64;
        for (int i = t; i < BM * 64; i += NT) {
            const int m = i >> 6, kk = i & 63, co = co0 + m;
            lA[m * LDA + kk] = co < a.Cout ? wsrc[(long long)co * wrow + kk] : 0.f;
        }
        // tap = wave + 4 j: kw = wave, kh = j & 3, kd = j >> 2
#pragma unroll
        for (int j = 0; j < 16; ++j)
            lX[(wave + 4 * j) * LDX + lane] =
                cvalid ? adv_load_x(a.s, n, ci, 2 * od - 1 + (j >> 2), 2 * oh - 1 + (j & 3), 2 * ow - 1 + wave) : 0.f;
        __syncthreads();
        adv_mma_chunk<WT::TM, WT::TN>(lA, lX, rt, ct, kq, nl, acc);
    }
#pragma unroll
    for (int i = 0; i < WT::TM; ++i)
#pragma unroll
        for (int j = 0; j < WT::TN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int co = co0 + rt[i] * 16 + kq * 4 + q;
                const long long col = col0 + ct[j] * 16 + nl;
                if (co < a.Cout && col < a.g.cols) {
                    if (a.slices > 1) a.part[((long long)slice * a.Cout + co) * a.g.cols + col] = acc[i][j][q];
                    else adv_fwd_store(a, acc[i][j][q], co, col);
                }
            }
}

__global__ __launch_bounds__(NT) void k4s2_fwd_reduce_kernel(const FwdArgs a) {
    const long long total = (long long)a.Cout * a.g.cols;
    for (long long e = blockIdx.x * (long long)NT + threadIdx.x; e < total; e += (long long)gridDim.x * NT) {
        float s = 0.f;
        for (int k = 0; k < a.slices; ++k) s += a.part[(long long)k * total + e];
        const int co = (int)(e / a.g.cols);
        adv_fwd_store(a, s, co, e - (long long)co * a.g.cols);
    }
}

// ------------------------------------------------------------------------------------------------ data gradient
struct DgArgs {
    GSrc gs;
    const float* w;                               // [Cout][Cin][64]
    int Cout, Cin;
    Geo g;                                        // the coarse extent = the extent of one parity class of dx
    float* dx; long long dx_bs;
};

template <int BM>
__global__ __launch_bounds__(NT) void k4s2_dgrad_kernel(const DgArgs a) {
    __shared__ float lA[BM * LDA];
    __shared__ float lG[64 * LDX];
    using WT = WaveTiles<BM>;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, kq = lane >> 4, nl = lane & 15;
    const long long col0 = (long long)blockIdx.x * 64;
    const int ci0 = blockIdx.y * BM;
    const int pd = blockIdx.z >> 2, ph = (blockIdx.z >> 1) & 1, pw = blockIdx.z & 1;
    const long long gcol = col0 + lane;
    const bool cvalid = gcol < a.g.cols;
    int n = 0, jd = 0, jh = 0, jw = 0;
    if (cvalid) adv_col(a.g, gcol, n, jd, jh, jw);
    // kk = co_l * 8 + td * 4 + th * 2 + tw = wave + 4 j: tw = wave & 1, th = wave >> 1, td = j & 1, co_l = j >> 1
    const int oh = jh + ph - (wave >> 1), ow = jw + pw - (wave & 1);
    const bool hw_ok = cvalid && (unsigned)oh < (unsigned)a.g.Ho && (unsigned)ow < (unsigned)a.g.Wo;
    int rt[WT::TM], ct[WT::TN];
    WT::get(wave, rt, ct);
    f32x4 acc[WT::TM][WT::TN];
#pragma unroll
    for (int i = 0; i < WT::TM; ++i)
#pragma unroll
        for (int j = 0; j < WT::TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int cb = 0; cb < a.Cout; cb += 8) {
        __syncthreads();
        for (int i = t; i < BM * 64; i += NT) {
            const int m = i >> 6, kk = i & 63, ci = ci0 + m, co = cb + (kk >> 3);
            const int kd = 1 - pd + 2 * ((kk >> 2) & 1), kh = 1 - ph + 2 * ((kk >> 1) & 1), kw = 1 - pw + 2 * (kk & 1);
            lA[m * LDA + kk] = (ci < a.Cin && co < a.Cout) ? a.w[((long long)co * a.Cin + ci) * 64 + kd * 16 + kh * 4 + kw] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int co = cb + (j >> 1), od = jd + pd - (j & 1);
            const bool ok = hw_ok && co < a.Cout && (unsigned)od < (unsigned)a.g.Do;
            lG[(wave + 4 * j) * LDX + lane] =
                ok ? adv_load_g(a.gs, n, co, a.g.So, ((long long)od * a.g.Ho + oh) * a.g.Wo + ow) : 0.f;
        }
        __syncthreads();
        adv_mma_chunk<WT::TM, WT::TN>(lA, lG, rt, ct, kq, nl, acc);
    }
    const int H = 2 * a.g.Ho, W = 2 * a.g.Wo;
    const long long S = 8 * a.g.So;
#pragma unroll
    for (int j = 0; j < WT::TN; ++j) {
        const long long col = col0 + ct[j] * 16 + nl;
        if (col >= a.g.cols) continue;
        int sn, sd, sh, sw;
        adv_col(a.g, col, sn, sd, sh, sw);
        float* __restrict__ dst = a.dx + (long long)sn * a.dx_bs + ((long long)(2 * sd + pd) * H + 2 * sh + ph) * W + 2 * sw + pw;
#pragma unroll
        for (int i = 0; i < WT::TM; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ci = ci0 + rt[i] * 16 + kq * 4 + q;
                if (ci < a.Cin) dst[(long long)ci * S] = acc[i][j][q];
            }
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct WgArgs {
    XSrc s;
    GSrc gs;
    int Cout, Cin;
    Geo g;
    int slices;
    long long cols_per;                           // columns per slice, a multiple of 64
    float* dw_l; float* dw_x;
    float* part;                                  // slices > 1: [slice][Cout][Cin * 64]
    int accumulate;
};

__device__ __forceinline__ float* adv_dw_ptr(const WgArgs& a, int co, int ci, int tap) {
    return ci < a.s.Cl ? a.dw_l + ((long long)co * a.s.Cl + ci) * 64 + tap
                       : a.dw_x + ((long long)co * a.s.Cx + (ci - a.s.Cl)) * 64 + tap;
}

__global__ __launch_bounds__(NT) void k4s2_wgrad_kernel(const WgArgs a) {
    __shared__ float lA[64 * LDA];
    __shared__ float lX[64 * LDX];
    __shared__ int4 lc[64];
    using WT = WaveTiles<64>;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, kq = lane >> 4, nl = lane & 15;
    const int ci = blockIdx.x, co0 = blockIdx.y * 64, slice = blockIdx.z;
    const long long c_begin = (long long)slice * a.cols_per;
    const long long c_end = c_begin + a.cols_per < a.g.cols ? c_begin + a.cols_per : a.g.cols;
    const int kd = lane >> 4, kh = (lane >> 2) & 3, kw = lane & 3;      // this thread's tap of the X tile
    int rt[2], ct[2];
    WT::get(wave, rt, ct);
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long long c0 = c_begin; c0 < c_end; c0 += 64) {
        __syncthreads();
        if (t < 64) {
            int4 c = make_int4(-1, 0, 0, 0);
            if (c0 + t < c_end) adv_col(a.g, c0 + t, c.x, c.y, c.z, c.w);
            lc[t] = c;
        }
        __syncthreads();
        // A[m = co][kk = column]
        {
            const int4 c = lc[lane];
            const long long v = ((long long)c.y * a.g.Ho + c.z) * a.g.Wo + c.w;
#pragma unroll 4
            for (int r = 0; r < 16; ++r) {
                const int m = wave + 4 * r, co = co0 + m;
                lA[m * LDA + lane] = (c.x >= 0 && co < a.Cout) ? adv_load_g(a.gs, c.x, co, a.g.So, v) : 0.f;
            }
        }
        // B[kk = column][tap]
#pragma unroll 4
        for (int j = 0; j < 16; ++j) {
            const int4 c = lc[wave + 4 * j];
            lX[(wave + 4 * j) * LDX + lane] =
                c.x >= 0 ? adv_load_x(a.s, c.x, ci, 2 * c.y - 1 + kd, 2 * c.z - 1 + kh, 2 * c.w - 1 + kw) : 0.f;
        }
        __syncthreads();
        adv_mma_chunk<2, 2>(lA, lX, rt, ct, kq, nl, acc);
    }
    const long long total = (long long)a.Cout * a.Cin * 64;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int co = co0 + rt[i] * 16 + kq * 4 + q, tap = ct[j] * 16 + nl;
                if (co >= a.Cout) continue;
                if (a.slices > 1) {
                    a.part[(long long)slice * total + ((long long)co * a.Cin + ci) * 64 + tap] = acc[i][j][q];
                } else {
                    float* p = adv_dw_ptr(a, co, ci, tap);
                    *p = a.accumulate ? *p + acc[i][j][q] : acc[i][j][q];
                }
            }
}

__global__ __launch_bounds__(NT) void k4s2_wgrad_reduce_kernel(const WgArgs a) {
    const long long total = (long long)a.Cout * a.Cin * 64;
    for (long long e = blockIdx.x * (long long)NT + threadIdx.x; e < total; e += (long long)gridDim.x * NT) {
        float s = 0.f;
        for (int k = 0; k < a.slices; ++k) s += a.part[(long long)k * total + e];
        const int tap = (int)(e & 63);
        const long long r = e >> 6;
        const int co = (int)(r / a.Cin), ci = (int)(r - (long long)co * a.Cin);
        float* p = adv_dw_ptr(a, co, ci, tap);
        *p = a.accumulate ? *p + s : s;
    }
}

// dbias[co] (+)= sum over (n, voxel) of G: one workgroup per channel, a fixed tree
__global__ __launch_bounds__(NT) void k4s2_dbias_kernel(const GSrc gs, const Geo g, float* dbias, float* dbias2, int accumulate) {
    __shared__ float red[4];
    const int co = blockIdx.x;
    float v[1] = {0.f};
    for (long long col = threadIdx.x; col < g.cols; col += NT) {
        const int n = (int)(col / g.So);
        v[0] += adv_load_g(gs, n, co, g.So, col - (long long)n * g.So);
    }
    mis_block_sum<1>(v, red);
    if (threadIdx.x == 0) {
        if (dbias) dbias[co] = accumulate ? dbias[co] + v[0] : v[0];
        if (dbias2) dbias2[co] = accumulate ? dbias2[co] + v[0] : v[0];
    }
}

// ------------------------------------------------------------------------------------------------ dropout decision
__global__ __launch_bounds__(NT) void channel_dropout_kernel(float* scale, int total, float p, unsigned salt,
                                                             const MisStepState* __restrict__ st) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const unsigned long long seed = st->seed, off = st->offset;
    uint32_t r[4];
    mis_philox4((uint32_t)i, 0x3D0D3D0Du, salt, (uint32_t)off, (uint32_t)seed, (uint32_t)(seed >> 32) ^ (uint32_t)(off >> 32), r);
    scale[i] = mis_u01(r[0]) >= p ? 1.f / (1.f - p) : 0.f;
}

// ------------------------------------------------------------------------------------------------ host side of the convolutions
bool even_ok(int D, int H, int W) { return !(D & 1) && !(H & 1) && !(W & 1); }

int geo_check(int N, int Cout, int D, int H, int W, Geo& g) {
    if (N <= 0 || Cout <= 0 || D <= 0 || H <= 0 || W <= 0) return MIS_ERR_ARG;
    if (!even_ok(D, H, W)) return MIS_ERR_UNSUPPORTED;
    g.N = N; g.Do = D / 2; g.Ho = H / 2; g.Wo = W / 2;
    g.So = (long long)g.Do * g.Ho * g.Wo;
    g.cols = g.So * N;
    if (g.cols >= (1LL << 31) || g.So * 8 >= (1LL << 31)) return MIS_ERR_UNSUPPORTED;
    return MIS_OK;
}

int fwd_slices(int Cin, int Cout, const Geo& g) {
    const long long tiles = mis_cdiv(Cout, Cout <= 16 ? 16 : 64) * mis_cdiv(g.cols, 64);
    if (tiles >= 256 || Cin < 8) return 1;
    long long s = 512 / tiles;
    if (s > Cin / 4) s = Cin / 4;      // at least four channels (256 contraction indices) per slice
    return s < 1 ? 1 : (int)s;
}

void wgrad_slices(int Cin, int Cout, const Geo& g, int& slices, long long& cols_per) {
    const long long tiles = (long long)Cin * mis_cdiv(Cout, 64), chunks = mis_cdiv(g.cols, 64);
    long long s = mis_cdiv(1024, tiles);
    if (s > 512) s = 512;
    if (s > chunks) s = chunks;
    const long long per = mis_cdiv(chunks, s);
    slices = (int)mis_cdiv(chunks, per);
    cols_per = per * 64;
}

}  // namespace

extern "C" int mis_channel_dropout_scale(float* scale, int N, int C, float p, unsigned salt, const MisStepState* state,
                                         hipStream_t stream) {
    if (!scale || !state || N <= 0 || C <= 0 || !(p >= 0.f) || !(p < 1.f)) return MIS_ERR_ARG;
    if ((long long)N * C >= (1LL << 31)) return MIS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(channel_dropout_kernel, dim3((unsigned)mis_cdiv((long long)N * C, NT)), dim3(NT), 0, stream, scale,
                       N * C, p, salt, state);
    return mis_launch_status();
}

extern "C" long long mis_conv_k4s2_fwd_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W) {
    Geo g;
    if (Cin <= 0) return MIS_ERR_ARG;
    const int st = geo_check(N, Cout, D, H, W, g);
    if (st) return st;
    const int s = fwd_slices(Cin, Cout, g);
    return s > 1 ? (long long)s * Cout * g.cols * 4 : 0;
}

extern "C" int mis_conv_k4s2_fwd(const float* x, long long x_bs, int Cx, const float* logits, long long l_bs, int Cl,
                                 const float* w_x, const float* w_l, const float* bias, const float* bias2, float* y,
                                 long long y_bs, int N, int Cout, int D, int H, int W, float slope, const float* drop_scale,
                                 float* workspace, long long workspace_bytes, hipStream_t stream) {
    Geo g;
    int st = geo_check(N, Cout, D, H, W, g);
    if (st) return st;
    st = adv_xsrc_check(x, x_bs, Cx, logits, l_bs, Cl, (long long)D * H * W);
    if (st) return st;
    if (!y || (Cx > 0 && !w_x) || (Cl > 0 && !w_l) || !(slope > 0.f) || y_bs < Cout * g.So) return MIS_ERR_ARG;
    const int Cin = Cx + Cl;
    const int slices = fwd_slices(Cin, Cout, g);
    if (slices > 1 && (!workspace || workspace_bytes < (long long)slices * Cout * g.cols * 4)) return MIS_ERR_WORKSPACE;
    FwdArgs a{{x, x_bs, Cx, logits, l_bs, Cl, D, H, W}, w_l, w_x, Cout, Cin, g, slices, (int)mis_cdiv(Cin, slices),
              workspace, bias, bias2, slope, drop_scale, y, y_bs};
    a.slices = (int)mis_cdiv(Cin, a.ci_per);
    const int bm = Cout <= 16 ? 16 : 64;
    const dim3 grid((unsigned)mis_cdiv(g.cols, 64), (unsigned)mis_cdiv(Cout, bm), (unsigned)a.slices);
    if (bm == 16) hipLaunchKernelGGL(k4s2_fwd_kernel<16>, grid, dim3(NT), 0, stream, a);
    else hipLaunchKernelGGL(k4s2_fwd_kernel<64>, grid, dim3(NT), 0, stream, a);
    st = mis_launch_status();
    if (st || a.slices == 1) return st;
    hipLaunchKernelGGL(k4s2_fwd_reduce_kernel, dim3(stream_grid((long long)Cout * g.cols)), dim3(NT), 0, stream, a);
    return mis_launch_status();
}

extern "C" int mis_conv_k4s2_dgrad(const float* dy, long long dy_bs, const float* y, long long y_bs, float slope,
                                   const float* drop_scale, const float* w, float* dx, long long dx_bs, int N, int Cin,
                                   int Cout, int D, int H, int W, hipStream_t stream) {
    Geo g;
    const int st = geo_check(N, Cout, D, H, W, g);
    if (st) return st;
    if (!dy || !w || !dx || Cin <= 0 || !(slope > 0.f)) return MIS_ERR_ARG;
    if (dy_bs < Cout * g.So || (y && y_bs < Cout * g.So) || dx_bs < Cin * g.So * 8) return MIS_ERR_ARG;
    DgArgs a{{dy, dy_bs, y, y_bs, slope, drop_scale, Cout}, w, Cout, Cin, g, dx, dx_bs};
    const int bm = Cin <= 16 ? 16 : 64;
    const dim3 grid((unsigned)mis_cdiv(g.cols, 64), (unsigned)mis_cdiv(Cin, bm), 8);
    if (bm == 16) hipLaunchKernelGGL(k4s2_dgrad_kernel<16>, grid, dim3(NT), 0, stream, a);
    else hipLaunchKernelGGL(k4s2_dgrad_kernel<64>, grid, dim3(NT), 0, stream, a);
    return mis_launch_status();
}

extern "C" long long mis_conv_k4s2_wgrad_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W) {
    Geo g;
    if (Cin <= 0) return MIS_ERR_ARG;
    const int st = geo_check(N, Cout, D, H, W, g);
    if (st) return st;
    int slices;
    long long per;
    wgrad_slices(Cin, Cout, g, slices, per);
    return slices > 1 ? (long long)slices * Cout * Cin * 64 * 4 : 0;
}

extern "C" int mis_conv_k4s2_wgrad(const float* x, long long x_bs, int Cx, const float* logits, long long l_bs, int Cl,
                                   const float* dy, long long dy_bs, const float* y, long long y_bs, float slope,
                                   const float* drop_scale, float* dw_x, float* dw_l, float* dbias, float* dbias2, int N,
                                   int Cout, int D, int H, int W, int accumulate, float* workspace,
                                   long long workspace_bytes, hipStream_t stream) {
    Geo g;
    int st = geo_check(N, Cout, D, H, W, g);
    if (st) return st;
    st = adv_xsrc_check(x, x_bs, Cx, logits, l_bs, Cl, (long long)D * H * W);
    if (st) return st;
    if (!dy || (Cx > 0 && !dw_x) || (Cl > 0 && !dw_l) || !(slope > 0.f)) return MIS_ERR_ARG;
    if (dy_bs < Cout * g.So || (y && y_bs < Cout * g.So)) return MIS_ERR_ARG;
    const int Cin = Cx + Cl;
    int slices;
    long long per;
    wgrad_slices(Cin, Cout, g, slices, per);
    if (slices > 1 && (!workspace || workspace_bytes < (long long)slices * Cout * Cin * 64 * 4)) return MIS_ERR_WORKSPACE;
    WgArgs a{{x, x_bs, Cx, logits, l_bs, Cl, D, H, W}, {dy, dy_bs, y, y_bs, slope, drop_scale, Cout}, Cout, Cin, g, slices,
             per, dw_l, dw_x, workspace, accumulate};
    hipLaunchKernelGGL(k4s2_wgrad_kernel, dim3((unsigned)Cin, (unsigned)mis_cdiv(Cout, 64), (unsigned)slices), dim3(NT), 0,
                       stream, a);
    st = mis_launch_status();
    if (st) return st;
    if (slices > 1) {
        hipLaunchKernelGGL(k4s2_wgrad_reduce_kernel, dim3(stream_grid((long long)Cout * Cin * 64)), dim3(NT), 0, stream, a);
        st = mis_launch_status();
        if (st) return st;
    }
    if (dbias || dbias2) {
        hipLaunchKernelGGL(k4s2_dbias_kernel, dim3((unsigned)Cout), dim3(NT), 0, stream, a.gs, g, dbias, dbias2, accumulate);
        st = mis_launch_status();
    }
    return st;
}

// =====================================================================================================
// Head: AvgPool3d over the whole feature -> Linear(C, K) -> cross-entropy, mean over the samples.
// workspace: pooled [N][C], dlogits [N][K], per-sample loss [N]
// =====================================================================================================
namespace {

// one workgroup per (n, 4 channels): wave w sums channel c0 + w over the P voxels in a fixed order
__global__ __launch_bounds__(NT) void head_pool_kernel(const float* __restrict__ a, long long a_bs, int C, long long P,
                                                       float* __restrict__ pooled) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6), n = blockIdx.y;
    if (c >= C) return;
    const float* __restrict__ src = a + (long long)n * a_bs + (long long)c * P;
    float s = 0.f;
    for (long long i = lane; i < P; i += 64) s += src[i];
    s = mis_wave_sum(s);
    if (lane == 0) pooled[(long long)n * C + c] = s / (float)P;
}

// da[n][c][:] = (sum_k dlogits[n][k] w[k][c]) / P
__global__ __launch_bounds__(NT) void head_bwd_da_kernel(const float* __restrict__ w, const float* __restrict__ dlogits,
                                                         int C, int K, long long P, float* __restrict__ da, long long da_bs) {
    const int c = blockIdx.x, n = blockIdx.y;
    float g = 0.f;
    for (int k = 0; k < K; ++k) g += dlogits[n * K + k] * w[(long long)k * C + c];
    g /= (float)P;
    float* __restrict__ dst = da + (long long)n * da_bs + (long long)c * P;
    for (long long i = threadIdx.x; i < P; i += NT) dst[i] = g;
}

int head_check(int N, int C, int K, int D, int H, int W) {
    if (N <= 0 || C <= 0 || K <= 0 || D <= 0 || H <= 0 || W <= 0) return MIS_ERR_ARG;
    if (K > MAXK || N > 65535) return MIS_ERR_UNSUPPORTED;
    return MIS_OK;
}

}  // namespace

extern "C" long long mis_adv_head_workspace_bytes(int N, int C, int K) {
    if (N <= 0 || C <= 0 || K <= 0) return MIS_ERR_ARG;
    return ((long long)N * C + (long long)N * K + N) * 4;
}

extern "C" int mis_adv_head_fwd(const float* a, long long a_bs, const float* w, const float* b, const int* target,
                                float* loss, float* logits, int N, int C, int K, int D, int H, int W, int pool_d,
                                int pool_h, int pool_w, float* workspace, long long workspace_bytes, hipStream_t stream) {
    const int st = head_check(N, C, K, D, H, W);
    if (st) return st;
    if (pool_d <= 0 || pool_h <= 0 || pool_w <= 0) return MIS_ERR_ARG;
    const long long P = (long long)D * H * W;
    if (!a || !w || !target || !loss || !logits || !workspace || a_bs < C * P) return MIS_ERR_ARG;
    if (pool_d != D || pool_h != H || pool_w != W) return MIS_ERR_UNSUPPORTED;
    if (workspace_bytes < mis_adv_head_workspace_bytes(N, C, K)) return MIS_ERR_WORKSPACE;
    float* pooled = workspace;
    float* dlogits = pooled + (long long)N * C;
    float* per_sample = dlogits + (long long)N * K;
    hipLaunchKernelGGL(head_pool_kernel, dim3((unsigned)mis_cdiv(C, 4), (unsigned)N), dim3(NT), 0, stream, a, a_bs, C, P, pooled);
    hipLaunchKernelGGL(head_final_kernel, dim3(1), dim3(NT), 0, stream, pooled, w, b, target, N, C, K, logits, dlogits,
                       per_sample, loss);
    return mis_launch_status();
}

extern "C" int mis_adv_head_bwd(const float* w, float* da, long long da_bs, float* dw, float* db, int accumulate, int N,
                                int C, int K, int D, int H, int W, const float* workspace, long long workspace_bytes,
                                hipStream_t stream) {
    const int st = head_check(N, C, K, D, H, W);
    if (st) return st;
    const long long P = (long long)D * H * W;
    if (!w || !workspace || (da && da_bs < C * P)) return MIS_ERR_ARG;
    if (workspace_bytes < mis_adv_head_workspace_bytes(N, C, K)) return MIS_ERR_WORKSPACE;
    const float* pooled = workspace;
    const float* dlogits = pooled + (long long)N * C;
    if (da)
        hipLaunchKernelGGL(head_bwd_da_kernel, dim3((unsigned)C, (unsigned)N), dim3(NT), 0, stream, w, dlogits, C, K, P, da, da_bs);
    if (dw || db)
        hipLaunchKernelGGL(head_bwd_dw_kernel, dim3((unsigned)mis_cdiv((long long)K * C, NT)), dim3(NT), 0, stream, pooled,
                           dlogits, N, C, K, dw, db, accumulate);
    return mis_launch_status();
}

// =====================================================================================================
// The segmenter's tail: the three stages of tail.h's tails.  Pass 1 sums CE and the Dice sums over the labeled samples,
// the finalize writes the scalars and the Dice coefficients, pass 2 writes dlogits: the supervised gradient on the labeled
// samples, w * p_c (dmap_c - sum_j dmap_j p_j) on the unlabeled ones.
// =====================================================================================================
namespace {

struct AdvTailArgs {
    const float* s; long long s_bs;
    const void* label; int label_bytes;
    const float* dmap; long long dm_bs;
    int B, L, C;
    long long S;
    int blocks;
};

constexpr int NPART = 1 + 3 * MIS_MAXC;      // [0] = ce sum, [1 + 3c ..] = I_c, Y_c, Z_c

template <int C>
__global__ __launch_bounds__(256) void adv_tail_pass1_kernel(const AdvTailArgs a, float* __restrict__ part) {
    __shared__ float red[4 * NPART];
    float v[NPART];
#pragma unroll
    for (int i = 0; i < NPART; ++i) v[i] = 0.f;
    const long long total = (long long)a.L * a.S;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / a.S);
        const long long sidx = i - (long long)b * a.S;
        float z[C], p[C], lse;
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = a.s[(long long)b * a.s_bs + (long long)c * a.S + sidx];
        mis_tail_softmax<C>(z, p, lse);
        mis_tail_labeled_sums<C>(z, p, lse, mis_tail_label(a.label, a.label_bytes, i), v[0], v + 1);
    }
    mis_block_sum<NPART>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NPART; ++i) part[(long long)blockIdx.x * NPART + i] = v[i];
    }
}

// coef[0] = ce scale, coef[1] = loss_scale * w, coef[2 + 2c] = a_c, coef[3 + 2c] = b_c
struct AdvFinalArgs {
    const float* part; int blocks; int C; int L; int Bu; long long S;
    float cons_weight; const MisStepState* st; const float* cons_loss; float loss_scale;
    float* out; float* coef;
};

__global__ __launch_bounds__(256) void adv_tail_final_kernel(const AdvFinalArgs a) {
    __shared__ double tot[NPART];
    mis_tail_reduce_parts(a.part, a.blocks, NPART, 1 + 3 * a.C, tot);
    if (threadIdx.x != 0) return;
    const double nlab = (double)a.L * (double)a.S;
    const float w = a.st ? a.st->cons_weight : a.cons_weight;
    const double ce = a.L > 0 ? tot[0] / nlab : 0.0;
    const double cons = (a.Bu > 0 && a.cons_loss) ? (double)a.cons_loss[0] : 0.0;
    double dice = 0.0;
    for (int c = 0; c < a.C; ++c) {
        double dl, ac, bc;
        mis_tail_dice_coef(tot[1 + 3 * c], tot[2 + 3 * c], tot[3 + 3 * c], 0.5 * a.loss_scale, a.C, dl, ac, bc);
        dice += dl;
        a.out[5 + c] = (float)(1.0 - dl);
        a.coef[2 + 2 * c] = (float)ac;
        a.coef[3 + 2 * c] = (float)bc;
    }
    dice = a.L > 0 ? dice / a.C : 0.0;
    a.out[0] = (float)(0.5 * (dice + ce) + (double)w * cons);
    a.out[1] = (float)ce; a.out[2] = (float)dice; a.out[3] = (float)cons; a.out[4] = w;
    a.coef[0] = a.L > 0 ? (float)(a.loss_scale * 0.5 / nlab) : 0.f;
    a.coef[1] = a.loss_scale * w;
}

template <int C>
__global__ __launch_bounds__(256) void adv_tail_pass2_kernel(const AdvTailArgs a, const float* __restrict__ coef,
                                                             float* __restrict__ ds, long long ds_bs) {
    const float kce = coef[0], kw = coef[1];
    float ac[C], bc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { ac[c] = coef[2 + 2 * c]; bc[c] = coef[3 + 2 * c]; }
    const long long total = (long long)a.B * a.S;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / a.S);
        const long long sidx = i - (long long)b * a.S;
        float z[C], p[C], o[C], lse;
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = a.s[(long long)b * a.s_bs + (long long)c * a.S + sidx];
        mis_tail_softmax<C>(z, p, lse);
        if (b < a.L) {
            mis_tail_labeled_grad<C>(p, mis_tail_label(a.label, a.label_bytes, i), kce, ac, bc, o);
        } else {
            float g[C], dot = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                g[c] = kw * a.dmap[(long long)(b - a.L) * a.dm_bs + (long long)c * a.S + sidx];
                dot += g[c] * p[c];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = p[c] * (g[c] - dot);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) ds[(long long)b * ds_bs + (long long)c * a.S + sidx] = o[c];
    }
}

int adv_tail_blocks(long long B, long long S) { return mis_tail_blocks(B * S); }

}  // namespace

extern "C" long long mis_adversarial_tail_workspace_bytes(int B, int C, long long S) {
    if (B <= 0 || C <= 0 || S <= 0) return MIS_ERR_ARG;
    return ((long long)adv_tail_blocks(B, S) * NPART + 2 + 2 * MIS_MAXC) * (long long)sizeof(float);
}

extern "C" int mis_adversarial_tail(const float* logits, long long s_bs, const void* label, int label_bytes,
                                    const float* dmap, long long dm_bs, const float* cons_loss, int B, int L, int C,
                                    long long S, float cons_weight, const MisStepState* state, float loss_scale, float* out,
                                    float* dlogits, long long d_bs, void* workspace, long long workspace_bytes,
                                    hipStream_t stream) {
    if (!logits || !out || !workspace || B <= 0 || L < 0 || L > B || C <= 0 || S <= 0) return MIS_ERR_ARG;
    if (L > 0 && !label) return MIS_ERR_ARG;
    if (B > L && (!dmap || !cons_loss)) return MIS_ERR_ARG;
    if (label_bytes != 1 && label_bytes != 8) return MIS_ERR_ARG;
    if (s_bs < C * S || (B > L && dm_bs < C * S) || (dlogits && d_bs < C * S)) return MIS_ERR_ARG;
    if (C != 2 && C != 3 && C != 4) return MIS_ERR_UNSUPPORTED;
    if (workspace_bytes < mis_adversarial_tail_workspace_bytes(B, C, S)) return MIS_ERR_WORKSPACE;
    AdvTailArgs a{logits, s_bs, label, label_bytes, dmap, dm_bs, B, L, C, S, adv_tail_blocks(B, S)};
    float* part = reinterpret_cast<float*>(workspace);
    float* coef = part + (long long)a.blocks * NPART;
    MIS_DISPATCH_C(C, adv_tail_pass1_kernel, a.blocks, stream, a, part)
    AdvFinalArgs f{part, a.blocks, C, L, B - L, S, cons_weight, state, cons_loss, loss_scale, out, coef};
    hipLaunchKernelGGL(adv_tail_final_kernel, dim3(1), dim3(256), 0, stream, f);
    if (dlogits) MIS_DISPATCH_C(C, adv_tail_pass2_kernel, a.blocks, stream, a, coef, dlogits, d_bs)
    return mis_launch_status();
}

// =====================================================================================================
// Adam
// =====================================================================================================
namespace {

struct AdamState { long long step; float bc1, bc2; };
static_assert(sizeof(AdamState) == 16, "AdamState layout");

// the corrections belong to a step taken: mis_adam_step writes them before it reads them
__global__ void adam_init_kernel(AdamState* st, long long step) {
    st->step = step;
    st->bc1 = 0.f;
    st->bc2 = 0.f;
}

__global__ void adam_advance_kernel(AdamState* st, float beta1, float beta2) {
    const long long step = st->step + 1;
    st->step = step;
    st->bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    st->bc2 = (float)(1.0 - pow((double)beta2, (double)step));
}

// torch.optim.Adam's single-tensor form: m.lerp_(g, 1 - b1); v = v * b2 + (1 - b2) g g;
// p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
__global__ __launch_bounds__(NT) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, long long n, float lr, float beta1, float beta2,
                                                  float eps, const AdamState* __restrict__ st) {
    const float step_size = lr / st->bc1, rs2 = sqrtf(st->bc2);
    const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
        const float gi = g[i];
        const float mi = m[i] + (gi - m[i]) * omb1;
        const float vi = v[i] * beta2 + omb2 * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] = p[i] - step_size * (mi / (sqrtf(vi) / rs2 + eps));
    }
}

}  // namespace

extern "C" int mis_adam_init(void* adam_state, long long step, hipStream_t stream) {
    if (!adam_state || step < 0) return MIS_ERR_ARG;
    hipLaunchKernelGGL(adam_init_kernel, dim3(1), dim3(1), 0, stream, reinterpret_cast<AdamState*>(adam_state), step);
    return mis_launch_status();
}

extern "C" int mis_adam_step(float* param, const float* grad, float* m, float* v, long long n, float lr, float beta1,
                             float beta2, float eps, void* adam_state, hipStream_t stream) {
    if (!param || !grad || !m || !v || !adam_state || n <= 0) return MIS_ERR_ARG;
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f)) return MIS_ERR_ARG;
    AdamState* st = reinterpret_cast<AdamState*>(adam_state);
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, stream, st, beta1, beta2);
    hipLaunchKernelGGL(adam_kernel, dim3(stream_grid(n)), dim3(NT), 0, stream, param, grad, m, v, n, lr, beta1, beta2, eps, st);
    return mis_launch_status();
}
