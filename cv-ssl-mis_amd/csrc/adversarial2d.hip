// Adversarial training of the 2-D nets: the discriminator's kernel-4 / stride-2 convolutions and its windowed head.
//
// Replaces (reference code/networks/discriminator.py:58-100 FCDiscriminator, code/train_adversarial_network_2D.py):
//   nn.Conv2d(Cin, Cout, kernel_size=4, stride=2, padding=1) -> LeakyReLU(0.2) -> Dropout2d(0.5), forward and backward
//   conv0(softmax(outputs)) + conv1(image)             as ONE convolution whose first channels are read through a softmax
//   AvgPool2d((7, 7)) -> flatten -> Linear(32 ndf, 2) -> F.cross_entropy    forward and backward
//
// The convolution is an implicit GEMM on v_mfma_f32_16x16x4_f32 in three forms ("Adversarial training, 2-D"):
//   forward  y [co][pixel]            = sum_{ci, ky, kx} w[co][ci][ky][kx] * in[ci][2 oy - 1 + ky][2 ox - 1 + kx]     K = 16 Cin
//   dgrad    dx[ci][pixel of class]   = sum_{co, ty, tx} w[co][ci][1 - ph + 2 ty][1 - pw + 2 tx] * G[co][jy + ph - ty][jx + pw - tx]
//                                       four parity classes (ph, pw), each a dense kernel-2 convolution of G,             K = 4 Cout
//   wgrad    dw[co][ci][tap]          = sum_{n, oy, ox} G[co][oy][ox] * in[ci][2 oy - 1 + ky][2 ox - 1 + kx]    16 taps x 8 ci = 128 columns
// G = dy * act'(y) * drop.  Unlike the 3-D kernels (adversarial.hip) nothing is gathered element by element: a workgroup owns
// a rectangle of output pixels of ONE sample and stages the input ROWS that rectangle needs -- whole row segments, 16-byte
// loads, bounds per row and per segment -- and the MFMA operand reads walk those rows at stride 2 (forward, wgrad) or 1
// (dgrad).  Neighbouring output rows share their input rows in LDS (rows 2 oy - 1 .. 2 oy + 2 overlap by two).
//
// LDS banks.  One MFMA step contracts 4 indices; lane = (kq = lane / 16, nl = lane % 16) reads A[row nl][k0 + kq] and
// B[k0 + kq][column nl], ds_read_b32, served as lanes 0-31 and 32-63, bank = dword address mod 32.
//   forward: the 4 indices of a step are the 4 column taps kx = kq of one (ci, ky); the 16 columns are 16 consecutive ox of one
//            output row: address = row base + 2 nl + kq + 3.  Lanes 0-31 (kq 0, 1) read 32 consecutive dwords, lanes 32-63
//            the next but two: the stride-2 walk fills the banks by itself, for any row pitch (XP = 40, a multiple of 4 for
//            the 16-byte stores).
//   wgrad:   the 4 indices are 4 consecutive ox of one output row, the 16 columns the taps (ky, kx) of one ci:
//            address = ky * XP + 2 kq + kx (+ base).  XP = 40 = 8 mod 32 puts the four ky rows 8 banks apart, 2 kq + kx spans 6:
//            distinct addresses on distinct banks, equal addresses broadcast.
//   dgrad:   the 4 indices are the taps (ty, tx) of one co, the 16 columns 16 consecutive jx: lanes 0-31 read one row at
//            nl + const and nl + const - 1: consecutive dwords.
//   A side (weights, or G for wgrad): rows LDA = 66 = 2 mod 32 apart: row nl, k = kq + const -> bank 2 nl + kq: distinct.
//   map gradient: A = G[co = kq][row][nl + const], planes 240 = 16 mod 32 apart; B = W'[co = kq][shift][column nl], planes
//            144 = 16 mod 32 apart: 16 + 16 distinct banks either way.
// Double buffering: two LDS buffers per operand; the loads of stage i + 1 are issued into registers before the MFMAs of stage i
// and written to the other buffer after them: one barrier per stage.
// Long contractions with few tiles are cut into slices (forward: over ci; wgrad: over pixel tiles), one partial tile per slice
// in the workspace, added in slice order by a second launch that also applies the epilogue: no atomics, bit-identical.
#include "tail.h"
#include "adv_common.h"
#include "../../include/mis_hip_adversarial2d.h"

#include <cstdint>

namespace {

constexpr int NT = 256;
constexpr int LDA = 66;       // A rows (64 contraction indices + 2)
constexpr int XP = 40;        // staged input row: columns 2 ox0 - 4 .. 2 ox0 + 35 of a 16-wide output tile
constexpr int XSEG = XP / 4;
constexpr int GP = 24;        // staged G row (dgrad): columns jx0 - 4 .. jx0 + 19
constexpr int GSEG = GP / 4;
constexpr int GROWS = 10;     // rows jy0 - 1 .. jy0 + 8 of an 8-row tile

// ------------------------------------------------------------------------------------------------ row loads
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__device__ __forceinline__ float4 ld4(const float* __restrict__ p, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

// columns c0 .. c0 + 3 of a row of W floats, zero outside [0, W).  vec: the row and c0 are 16-byte aligned and W % 4 == 0, so
// a segment lies inside or outside as a whole; otherwise element by element.
__device__ __forceinline__ float4 ld_row4(const float* __restrict__ row, int c0, int W, bool vec) {
    if (c0 + 4 <= 0 || c0 >= W) return zero4();
    if (c0 >= 0 && c0 + 4 <= W) return ld4(row + c0, vec);
    float4 v = zero4();
    if ((unsigned)c0 < (unsigned)W) v.x = row[c0];
    if ((unsigned)(c0 + 1) < (unsigned)W) v.y = row[c0 + 1];
    if ((unsigned)(c0 + 2) < (unsigned)W) v.z = row[c0 + 2];
    if ((unsigned)(c0 + 3) < (unsigned)W) v.w = row[c0 + 3];
    return v;
}

__device__ __forceinline__ float comp(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// ------------------------------------------------------------------------------------------------ the input operand
// The convolution's input channels in chunks of 4: chunk 0 holds the Cl softmax-read channels (when Cl > 0), the following
// ones the plain channels four by four.
struct XSrc {
    const float* x; long long x_bs; int Cx;
    const float* lg; long long l_bs; int Cl;
    int H, W;
    int xvec, lvec;
};

__device__ __host__ __forceinline__ int x_nsoft(const XSrc& s) { return s.Cl > 0 ? 1 : 0; }
__device__ __host__ __forceinline__ int x_chunks(const XSrc& s) { return x_nsoft(s) + (s.Cx + 3) / 4; }

// Stage loads of a [4 channels][NR rows][XP] input tile: rows iy0 .. iy0 + NR - 1, columns ix0 .. ix0 + XP - 1 (ix0 % 4 == 0).
template <int NR>
__device__ __forceinline__ void x_load(const XSrc& s, int n, int chunk, int iy0, int ix0, float4 (&r)[4]) {
    const int t = threadIdx.x;
    const long long HW = (long long)s.H * s.W;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = zero4();
    if (chunk < x_nsoft(s)) {
        static_assert(NR * XSEG <= NT, "one softmax item per thread");
        if (t < NR * XSEG) {
            const int row = t / XSEG, seg = t - row * XSEG, iy = iy0 + row;
            if ((unsigned)iy < (unsigned)s.H) {
                const float* __restrict__ p = s.lg + (long long)n * s.l_bs + (long long)iy * s.W;
#pragma unroll
                for (int c = 0; c < MAXCL; ++c)
                    if (c < s.Cl) r[c] = ld_row4(p + (long long)c * HW, ix0 + 4 * seg, s.W, s.lvec);
            }
        }
    } else {
        constexpr int ITEMS = 4 * NR * XSEG, NI = (ITEMS + NT - 1) / NT;
        static_assert(NI <= 4, "prefetch registers");
        const int c0 = (chunk - x_nsoft(s)) * 4;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int idx = t + NT * i;
            if (idx < ITEMS) {
                const int seg = idx % XSEG, rr = idx / XSEG, row = rr % NR, ci = c0 + rr / NR, iy = iy0 + row;
                if (ci < s.Cx && (unsigned)iy < (unsigned)s.H)
                    r[i] = ld_row4(s.x + (long long)n * s.x_bs + (long long)ci * HW + (long long)iy * s.W, ix0 + 4 * seg, s.W,
                                   s.xvec);
            }
        }
    }
}

template <int NR>
__device__ __forceinline__ void x_store(const XSrc& s, int chunk, int iy0, int ix0, const float4 (&r)[4], float* lX) {
    const int t = threadIdx.x;
    if (chunk < x_nsoft(s)) {
        if (t < NR * XSEG) {
            const int row = t / XSEG, seg = t - row * XSEG, iy = iy0 + row;
            float o[MAXCL][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int col = ix0 + 4 * seg + e;
                const bool in = (unsigned)iy < (unsigned)s.H && (unsigned)col < (unsigned)s.W;
                float v[MAXCL], mx = comp(r[0], e);
                v[0] = mx;
#pragma unroll
                for (int c = 1; c < MAXCL; ++c) {
                    v[c] = c < s.Cl ? comp(r[c], e) : -INFINITY;
                    mx = fmaxf(mx, v[c]);
                }
                float sum = 0.f;
#pragma unroll
                for (int c = 0; c < MAXCL; ++c) {
                    v[c] = c < s.Cl ? expf(v[c] - mx) : 0.f;
                    sum += v[c];
                }
                const float inv = 1.f / sum;
#pragma unroll
                for (int c = 0; c < MAXCL; ++c) o[c][e] = in ? v[c] * inv : 0.f;      // the padding is zero, not softmax(0)
            }
#pragma unroll
            for (int c = 0; c < MAXCL; ++c)
                *reinterpret_cast<float4*>(lX + (c * NR + row) * XP + seg * 4) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
        }
    } else {
        constexpr int ITEMS = 4 * NR * XSEG, NI = (ITEMS + NT - 1) / NT;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int idx = t + NT * i;
            if (idx < ITEMS) *reinterpret_cast<float4*>(lX + (idx / XSEG) * XP + (idx % XSEG) * 4) = r[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------ the gradient operand
struct GSrc {
    const float* dy; long long dy_bs;
    const float* y; long long y_bs;               // the stored activated output (NULL: no activation)
    float slope;
    const float* drop;                            // [N][Cout] or NULL
    int Cout, Ho, Wo;
    int vec;
};

__device__ __forceinline__ float g_one(float d, float yv, bool has_y, float slope, float scale) {
    if (has_y) d = yv > 0.f ? d : d * slope;
    return d * scale;
}

__device__ __forceinline__ float4 g_four(const float4& d, const float4& yv, bool has_y, float slope, float scale) {
    return make_float4(g_one(d.x, yv.x, has_y, slope, scale), g_one(d.y, yv.y, has_y, slope, scale),
                       g_one(d.z, yv.z, has_y, slope, scale), g_one(d.w, yv.w, has_y, slope, scale));
}

__device__ __forceinline__ float g_scale(const GSrc& g, int n, int co) {
    return (g.drop && co < g.Cout) ? g.drop[(long long)n * g.Cout + co] : 1.f;
}

// dgrad's G tile [16 co][GROWS][GP]: channels cb .., rows gy0 .., columns gx0 .. (gx0 % 4 == 0): 960 segments, 4 per thread
constexpr int GD_ITEMS = 16 * GROWS * GSEG, GD_NI = (GD_ITEMS + NT - 1) / NT;

__device__ __forceinline__ void gd_load(const GSrc& g, int n, int cb, int gy0, int gx0, float4 (&d)[GD_NI], float4 (&yv)[GD_NI]) {
    const long long So = (long long)g.Ho * g.Wo;
#pragma unroll
    for (int i = 0; i < GD_NI; ++i) {
        d[i] = zero4();
        yv[i] = zero4();
        const int idx = threadIdx.x + NT * i;
        if (idx < GD_ITEMS) {
            const int seg = idx % GSEG, rr = idx / GSEG, row = rr % GROWS, co = cb + rr / GROWS, gy = gy0 + row;
            if (co < g.Cout && (unsigned)gy < (unsigned)g.Ho) {
                const long long off = (long long)co * So + (long long)gy * g.Wo;
                d[i] = ld_row4(g.dy + (long long)n * g.dy_bs + off, gx0 + 4 * seg, g.Wo, g.vec);
                if (g.y) yv[i] = ld_row4(g.y + (long long)n * g.y_bs + off, gx0 + 4 * seg, g.Wo, g.vec);
            }
        }
    }
}

__device__ __forceinline__ void gd_store(const GSrc& g, int n, int cb, const float4 (&d)[GD_NI], const float4 (&yv)[GD_NI],
                                         float* lG) {
#pragma unroll
    for (int i = 0; i < GD_NI; ++i) {
        const int idx = threadIdx.x + NT * i;
        if (idx < GD_ITEMS) {
            const int co = cb + idx / (GSEG * GROWS);
            *reinterpret_cast<float4*>(lG + (idx / GSEG) * GP + (idx % GSEG) * 4) =
                g_four(d[i], yv[i], g.y != nullptr, g.slope, g_scale(g, n, co));
        }
    }
}

// ------------------------------------------------------------------------------------------------ forward
// A workgroup: 64 output channels x (8 output rows x 16 output columns) of one sample; wave = (channel half, row half), each
// 2 x 4 MFMA tiles (a column tile = one output row).  Stage = 4 input channels = 64 contraction indices.
constexpr int F_TR = 8, F_NR = 2 * F_TR + 2;

struct FwdArgs {
    XSrc s;
    const float* w_l; const float* w_x;
    int wvec;
    int N, Cout;
    int Ho, Wo, tiles_x;
    int slices, chunks_per;
    float* part;                                  // slices > 1: [slice][N][Cout][Ho * Wo]
    const float* bias; const float* bias2;
    float slope;
    const float* drop;
    float* y; long long y_bs;
};

__device__ __forceinline__ void fwd_store(const FwdArgs& a, float v, int n, int co, long long pix) {
    if (a.bias) v += a.bias[co];
    if (a.bias2) v += a.bias2[co];
    v = v > 0.f ? v : v * a.slope;
    if (a.drop) v *= a.drop[(long long)n * a.Cout + co];
    a.y[(long long)n * a.y_bs + (long long)co * a.Ho * a.Wo + pix] = v;
}

// the filter rows of one chunk: lA[m][cl * 16 + tap], 4 segments of 4 taps per (m, cl): 1024 segments, 4 per thread
__device__ __forceinline__ void fw_load(const FwdArgs& a, int chunk, int co0, float4 (&r)[4]) {
    const bool soft = chunk < x_nsoft(a.s);
    const float* __restrict__ w = soft ? a.w_l : a.w_x;
    const int Cp = soft ? a.s.Cl : a.s.Cx, c0 = soft ? 0 : (chunk - x_nsoft(a.s)) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = threadIdx.x + NT * i, q = idx & 3, cl = (idx >> 2) & 3, co = co0 + (idx >> 4);
        r[i] = (co < a.Cout && c0 + cl < Cp) ? ld4(w + ((long long)co * Cp + c0 + cl) * 16 + q * 4, a.wvec) : zero4();
    }
}

__device__ __forceinline__ void fw_store(const float4 (&r)[4], float* lA) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = threadIdx.x + NT * i;
        float* p = lA + (idx >> 4) * LDA + (idx & 15) * 4;           // LDA is even: 8-byte stores
        *reinterpret_cast<float2*>(p) = make_float2(r[i].x, r[i].y);
        *reinterpret_cast<float2*>(p + 2) = make_float2(r[i].z, r[i].w);
    }
}

__global__ __launch_bounds__(NT) void conv2d_k4s2_fwd_kernel(const FwdArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 64 * LDA + 2 * 4 * F_NR * XP];
    float* lA = lds;
    float* lX = lds + 2 * 64 * LDA;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, kq = lane >> 4, nl = lane & 15;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int oy0 = ty * F_TR, ox0 = tx * 16, co0 = blockIdx.y * 64;
    const int n = blockIdx.z / a.slices, slice = blockIdx.z - n * a.slices;
    const int iy0 = 2 * oy0 - 1, ix0 = 2 * ox0 - 4;
    const int rt0 = (wave >> 1) * 2, r0 = (wave & 1) * 4;
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nch = x_chunks(a.s);
    const int c_begin = slice * a.chunks_per, c_end = min(nch, c_begin + a.chunks_per);
    float4 ra[4], rx[4];
    if (c_begin < c_end) {
        fw_load(a, c_begin, co0, ra);
        x_load<F_NR>(a.s, n, c_begin, iy0, ix0, rx);
        fw_store(ra, lA);
        x_store<F_NR>(a.s, c_begin, iy0, ix0, rx, lX);
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const int cur = (c - c_begin) & 1;
        const bool more = c + 1 < c_end;
        if (more) {
            fw_load(a, c + 1, co0, ra);
            x_load<F_NR>(a.s, n, c + 1, iy0, ix0, rx);
        }
        const float* A = lA + cur * 64 * LDA + (rt0 * 16 + nl) * LDA + kq;
        const float* X = lX + cur * 4 * F_NR * XP + 2 * r0 * XP + 2 * nl + kq + 3;
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {                                   // k = cl * 4 + ky
            const float a0 = A[k * 4], a1 = A[16 * LDA + k * 4];
            const float* xr = X + ((k >> 2) * F_NR + (k & 3)) * XP;
            float b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = xr[2 * j * XP];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b[j], acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b[j], acc[1][j], 0, 0, 0);
            }
        }
        if (more) {
            fw_store(ra, lA + (cur ^ 1) * 64 * LDA);
            x_store<F_NR>(a.s, c + 1, iy0, ix0, rx, lX + (cur ^ 1) * 4 * F_NR * XP);
        }
        __syncthreads();
    }
    const long long So = (long long)a.Ho * a.Wo;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int oy = oy0 + r0 + j, ox = ox0 + nl;
        if (oy >= a.Ho || ox >= a.Wo) continue;
        const long long pix = (long long)oy * a.Wo + ox;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int co = co0 + (rt0 + i) * 16 + kq * 4 + q;
                if (co >= a.Cout) continue;
                if (a.slices > 1) a.part[(((long long)slice * a.N + n) * a.Cout + co) * So + pix] = acc[i][j][q];
                else fwd_store(a, acc[i][j][q], n, co, pix);
            }
    }
}

__global__ __launch_bounds__(NT) void conv2d_k4s2_fwd_reduce_kernel(const FwdArgs a) {
    const long long So = (long long)a.Ho * a.Wo, total = (long long)a.N * a.Cout * So;
    for (long long e = blockIdx.x * (long long)NT + threadIdx.x; e < total; e += (long long)gridDim.x * NT) {
        float s = 0.f;
        for (int k = 0; k < a.slices; ++k) s += a.part[(long long)k * total + e];
        const long long nc = e / So;
        const int n = (int)(nc / a.Cout);
        fwd_store(a, s, n, (int)(nc - (long long)n * a.Cout), e - nc * So);
    }
}

// ------------------------------------------------------------------------------------------------ data gradient
// A workgroup: 64 input channels x (8 x 16 pixels of one parity class) of one sample.  Stage = 16 output channels = 64
// contraction indices (co, ty, tx).
struct DgArgs {
    GSrc gs;
    const float* w;                               // [Cout][Cin][16]
    int wvec;
    int Cout, Cin;
    int tiles_x;
    float* dx; long long dx_bs;
};

// lA[m = ci][co_l * 4 + ty * 2 + tx]: one filter row (ky) of 4 taps per item, two of them kept: 2048 items, 8 per thread
__device__ __forceinline__ void dw_load(const DgArgs& a, int cb, int ci0, int ph, float4 (&r)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int idx = threadIdx.x + NT * i, ci = ci0 + (idx & 63), ty = (idx >> 6) & 1, co = cb + (idx >> 7);
        r[i] = (ci < a.Cin && co < a.Cout) ? ld4(a.w + ((long long)co * a.Cin + ci) * 16 + (1 - ph + 2 * ty) * 4, a.wvec) : zero4();
    }
}

__device__ __forceinline__ void dw_store(const float4 (&r)[8], int pw, float* lA) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int idx = threadIdx.x + NT * i;
        // kx = 1 - pw + 2 tx
        *reinterpret_cast<float2*>(lA + (idx & 63) * LDA + (idx >> 7) * 4 + ((idx >> 6) & 1) * 2) =
            pw ? make_float2(r[i].x, r[i].z) : make_float2(r[i].y, r[i].w);
    }
}

__global__ __launch_bounds__(NT) void conv2d_k4s2_dgrad_kernel(const DgArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 64 * LDA + 2 * 16 * GROWS * GP];
    float* lA = lds;
    float* lG = lds + 2 * 64 * LDA;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, kq = lane >> 4, nl = lane & 15;
    const int ty_ = blockIdx.x / a.tiles_x, tx_ = blockIdx.x - ty_ * a.tiles_x;
    const int jy0 = ty_ * 8, jx0 = tx_ * 16, ci0 = blockIdx.y * 64;
    const int n = blockIdx.z >> 2, ph = (blockIdx.z >> 1) & 1, pw = blockIdx.z & 1;
    const int rt0 = (wave >> 1) * 2, r0 = (wave & 1) * 4;
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 ra[8], rd[GD_NI], ry[GD_NI];
    dw_load(a, 0, ci0, ph, ra);
    gd_load(a.gs, n, 0, jy0 - 1, jx0 - 4, rd, ry);
    dw_store(ra, pw, lA);
    gd_store(a.gs, n, 0, rd, ry, lG);
    __syncthreads();
    int cur = 0;
    for (int cb = 0; cb < a.Cout; cb += 16, cur ^= 1) {
        const bool more = cb + 16 < a.Cout;
        if (more) {
            dw_load(a, cb + 16, ci0, ph, ra);
            gd_load(a.gs, n, cb + 16, jy0 - 1, jx0 - 4, rd, ry);
        }
        const float* A = lA + cur * 64 * LDA + (rt0 * 16 + nl) * LDA + kq;
        // row jy + ph - ty of the tile is jy - jy0 + 1 + ph - ty, column jx + pw - tx is jx - jx0 + 4 + pw - tx
        const float* G = lG + cur * 16 * GROWS * GP + (r0 + 1 + ph - (kq >> 1)) * GP + nl + 4 + pw - (kq & 1);
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {                                   // k = co_l
            const float a0 = A[k * 4], a1 = A[16 * LDA + k * 4];
            float b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = G[(k * GROWS + j) * GP];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b[j], acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b[j], acc[1][j], 0, 0, 0);
            }
        }
        if (more) {
            dw_store(ra, pw, lA + (cur ^ 1) * 64 * LDA);
            gd_store(a.gs, n, cb + 16, rd, ry, lG + (cur ^ 1) * 16 * GROWS * GP);
        }
        __syncthreads();
    }
    const int W = 2 * a.gs.Wo;
    const long long S = 4LL * a.gs.Ho * a.gs.Wo;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int jy = jy0 + r0 + j, jx = jx0 + nl;
        if (jy >= a.gs.Ho || jx >= a.gs.Wo) continue;
        float* __restrict__ dst = a.dx + (long long)n * a.dx_bs + (long long)(2 * jy + ph) * W + 2 * jx + pw;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ci = ci0 + (rt0 + i) * 16 + kq * 4 + q;
                if (ci < a.Cin) dst[(long long)ci * S] = acc[i][j][q];
            }
    }
}

// The `map` gradient, Cin <= 4.  With channels on the MFMA's rows a 16-row tile would carry 4 useful rows.  Here the rows are
// 16 consecutive pixels jx of one row jy of the coarse grid, the 16 columns are (ci, ph, pw) -- 4 channels x 4 parity
// classes, all useful at Cin = 4 -- and the contraction runs over (co, shift) with the 9 shifts (oy, ox) in {-1, 0, 1}^2 of G:
//   dx[ci][2 jy + ph][2 jx + pw] = sum_{co, oy, ox} G[co][jy + oy][jx + ox] * W'[co][oy, ox][ci, ph, pw],
//   W' = w[co][ci][1 + ph - 2 oy][1 + pw - 2 ox] where ph - oy and pw - ox are in {0, 1}, else 0  (4 of the 9 shifts per class).
// 4 / 9 of the MFMA work is useful instead of 4 / 16, and G is staged once for all four classes.
constexpr int WS_PLANE = 9 * 16;

__device__ __forceinline__ void sw_load(const DgArgs& a, int cb, float (&r)[9]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int idx = threadIdx.x + NT * i, col = idx & 15, s = (idx >> 4) % 9, co = cb + idx / WS_PLANE;
        const int ci = col >> 2, ph = (col >> 1) & 1, pw = col & 1, ty = ph - (s / 3 - 1), tx = pw - (s % 3 - 1);
        const bool ok = (unsigned)ty < 2u && (unsigned)tx < 2u && ci < a.Cin && co < a.Cout;
        r[i] = ok ? a.w[((long long)co * a.Cin + ci) * 16 + (1 - ph + 2 * ty) * 4 + 1 - pw + 2 * tx] : 0.f;
    }
}

__global__ __launch_bounds__(NT) void conv2d_k4s2_dgrad_map_kernel(const DgArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 16 * WS_PLANE + 2 * 16 * GROWS * GP];
    float* lW = lds;
    float* lG = lds + 2 * 16 * WS_PLANE;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, kq = lane >> 4, nl = lane & 15;
    const int ty_ = blockIdx.x / a.tiles_x, tx_ = blockIdx.x - ty_ * a.tiles_x;
    const int jy0 = ty_ * 8, jx0 = tx_ * 16, n = blockIdx.z;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    float rw[9];
    float4 rd[GD_NI], ry[GD_NI];
    sw_load(a, 0, rw);
    gd_load(a.gs, n, 0, jy0 - 1, jx0 - 4, rd, ry);
#pragma unroll
    for (int i = 0; i < 9; ++i) lW[t + NT * i] = rw[i];
    gd_store(a.gs, n, 0, rd, ry, lG);
    __syncthreads();
    int cur = 0;
    for (int cb = 0; cb < a.Cout; cb += 16, cur ^= 1) {
        const bool more = cb + 16 < a.Cout;
        if (more) {
            sw_load(a, cb + 16, rw);
            gd_load(a.gs, n, cb + 16, jy0 - 1, jx0 - 4, rd, ry);
        }
        const float* Wp = lW + cur * 16 * WS_PLANE + kq * WS_PLANE + nl;
        const float* G = lG + cur * 16 * GROWS * GP + kq * GROWS * GP + (2 * wave + 1) * GP + nl + 4;
#pragma unroll
        for (int cg = 0; cg < 4; ++cg)
#pragma unroll
            for (int s = 0; s < 9; ++s) {
                const float b = Wp[cg * 4 * WS_PLANE + s * 16];
                const float* g = G + cg * 4 * GROWS * GP + (s / 3 - 1) * GP + (s % 3 - 1);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[0], b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[GP], b, acc[1], 0, 0, 0);
            }
        if (more) {
#pragma unroll
            for (int i = 0; i < 9; ++i) lW[(cur ^ 1) * 16 * WS_PLANE + t + NT * i] = rw[i];
            gd_store(a.gs, n, cb + 16, rd, ry, lG + (cur ^ 1) * 16 * GROWS * GP);
        }
        __syncthreads();
    }
    const int W = 2 * a.gs.Wo, ci = nl >> 2, ph = (nl >> 1) & 1, pw = nl & 1;
    const long long S = 4LL * a.gs.Ho * a.gs.Wo;
    if (ci >= a.Cin) return;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int jy = jy0 + 2 * wave + i;
        if (jy >= a.gs.Ho) continue;
        float* __restrict__ dst = a.dx + (long long)n * a.dx_bs + (long long)ci * S + (long long)(2 * jy + ph) * W + pw;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int jx = jx0 + kq * 4 + q;
            if (jx < a.gs.Wo) dst[2 * jx] = acc[i][q];
        }
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// A workgroup: 64 output channels x (two chunks of 4 input channels x 16 taps = 128 columns) over a slice of the pixel tiles
// (n, 4 output rows, 16 output columns).  Stage = one pixel tile = 64 contraction indices.  G is the large operand (64 rows of
// dy and y per stage against 8 short input planes): every pair of chunks reads it once, so the columns are as wide as the
// accumulators and 64 KiB of LDS allow.  The workgroups of the first pair also sum the rows of G they stage -- the bias
// gradient -- so that G is not read a second time for it.
constexpr int W_TR = 4, W_NR = 2 * W_TR + 2, W_NC = 2;

struct WgArgs {
    XSrc s;
    GSrc gs;
    int N, Cout, Cin;
    int tiles_x, tiles_y;
    int slices;
    long long tiles_per;
    float* dw_l; float* dw_x;
    // one row of `row` floats per slice: the filter partials [Cout][Cin][16] (slices > 1 only; boff of them), then the
    // bias gradient's partial sums [Cout]
    float* part; long long row, boff;
    float* dbias; float* dbias2;                  // both NULL: not wanted
    int accumulate;
};

__device__ __forceinline__ float* wg_dw_ptr(const WgArgs& a, int co, int ci, int tap) {
    return ci < a.s.Cl ? a.dw_l + ((long long)co * a.s.Cl + ci) * 16 + tap
                       : a.dw_x + ((long long)co * a.s.Cx + (ci - a.s.Cl)) * 16 + tap;
}

__device__ __forceinline__ void wg_tile(const WgArgs& a, long long tile, int& n, int& oy0, int& ox0) {
    const int per = a.tiles_x * a.tiles_y;
    n = (int)(tile / per);
    const int r = (int)(tile - (long long)n * per), ty = r / a.tiles_x;
    oy0 = ty * W_TR;
    ox0 = (r - ty * a.tiles_x) * 16;
}

// lG[m = co][oy_l * 16 + ox_l]: 64 x 4 rows x 4 segments = 1024 segments, 4 per thread
__device__ __forceinline__ void wgg_load(const GSrc& g, int n, int co0, int oy0, int ox0, float4 (&d)[4], float4 (&yv)[4]) {
    const long long So = (long long)g.Ho * g.Wo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        d[i] = zero4();
        yv[i] = zero4();
        const int idx = threadIdx.x + NT * i, seg = idx & 3, oy = oy0 + ((idx >> 2) & 3), co = co0 + (idx >> 4);
        if (co < g.Cout && oy < g.Ho) {
            const long long off = (long long)co * So + (long long)oy * g.Wo;
            d[i] = ld_row4(g.dy + (long long)n * g.dy_bs + off, ox0 + 4 * seg, g.Wo, g.vec);
            if (g.y) yv[i] = ld_row4(g.y + (long long)n * g.y_bs + off, ox0 + 4 * seg, g.Wo, g.vec);
        }
    }
}

// bsum[i] collects this thread's share of the row sums: row (threadIdx.x >> 4) + 16 i, one of its 16 segments
__device__ __forceinline__ void wgg_store(const GSrc& g, int n, int co0, const float4 (&d)[4], const float4 (&yv)[4], float* lG,
                                          float (&bsum)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = threadIdx.x + NT * i;
        const float4 v = g_four(d[i], yv[i], g.y != nullptr, g.slope, g_scale(g, n, co0 + (idx >> 4)));
        float* p = lG + (idx >> 4) * LDA + (idx & 15) * 4;
        *reinterpret_cast<float2*>(p) = make_float2(v.x, v.y);
        *reinterpret_cast<float2*>(p + 2) = make_float2(v.z, v.w);
        bsum[i] += (v.x + v.y) + (v.z + v.w);
    }
}

__global__ __launch_bounds__(NT) void conv2d_k4s2_wgrad_kernel(const WgArgs a) {
    constexpr int XT = 4 * W_NR * XP;                                    // one chunk's input tile
    __shared__ __attribute__((aligned(16))) float lds[2 * 64 * LDA + 2 * W_NC * XT];
    float* lG = lds;
    float* lX = lds + 2 * 64 * LDA;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, kq = lane >> 4, nl = lane & 15;
    const int chunk0 = blockIdx.x * W_NC, co0 = blockIdx.y * 64, slice = blockIdx.z;
    const long long ntiles = (long long)a.N * a.tiles_x * a.tiles_y;
    const long long t_begin = (long long)slice * a.tiles_per;
    const long long t_end = t_begin + a.tiles_per < ntiles ? t_begin + a.tiles_per : ntiles;
    const int rt0 = (wave >> 1) * 2, wc = wave & 1;                      // this wave's rows, and its chunk of the pair
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
    float4 rd[4], ry[4], rx[W_NC][4];
    int n, oy0, ox0;
    if (t_begin < t_end) {
        wg_tile(a, t_begin, n, oy0, ox0);
        wgg_load(a.gs, n, co0, oy0, ox0, rd, ry);
#pragma unroll
        for (int c = 0; c < W_NC; ++c) x_load<W_NR>(a.s, n, chunk0 + c, 2 * oy0 - 1, 2 * ox0 - 4, rx[c]);
        wgg_store(a.gs, n, co0, rd, ry, lG, bsum);
#pragma unroll
        for (int c = 0; c < W_NC; ++c) x_store<W_NR>(a.s, chunk0 + c, 2 * oy0 - 1, 2 * ox0 - 4, rx[c], lX + c * XT);
    }
    __syncthreads();
    for (long long tile = t_begin; tile < t_end; ++tile) {
        const int cur = (int)(tile - t_begin) & 1;
        const bool more = tile + 1 < t_end;
        if (more) {
            wg_tile(a, tile + 1, n, oy0, ox0);
            wgg_load(a.gs, n, co0, oy0, ox0, rd, ry);
#pragma unroll
            for (int c = 0; c < W_NC; ++c) x_load<W_NR>(a.s, n, chunk0 + c, 2 * oy0 - 1, 2 * ox0 - 4, rx[c]);
        }
        const float* A = lG + cur * 64 * LDA + (rt0 * 16 + nl) * LDA + kq;
        // column nl = tap (ky, kx) of channel j of this wave's chunk; contraction index = pixel (oy_l, ox_l = 4 oxq + kq)
        const float* X = lX + (cur * W_NC + wc) * XT + (nl >> 2) * XP + 2 * kq + (nl & 3) + 3;
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {                                   // k = oy_l * 4 + oxq
            const float a0 = A[k * 4], a1 = A[16 * LDA + k * 4];
            const float* xr = X + 2 * (k >> 2) * XP + 8 * (k & 3);
            float b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = xr[j * W_NR * XP];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b[j], acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b[j], acc[1][j], 0, 0, 0);
            }
        }
        if (more) {
            wgg_store(a.gs, n, co0, rd, ry, lG + (cur ^ 1) * 64 * LDA, bsum);
#pragma unroll
            for (int c = 0; c < W_NC; ++c)
                x_store<W_NR>(a.s, chunk0 + c, 2 * oy0 - 1, 2 * ox0 - 4, rx[c], lX + ((cur ^ 1) * W_NC + c) * XT);
        }
        __syncthreads();
    }
    // the bias gradient's share of this slice: the 16 threads of a row add their sums in a fixed tree
    if ((a.dbias || a.dbias2) && blockIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v = bsum[i];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            const int co = co0 + (t >> 4) + 16 * i;
            if ((t & 15) == 0 && co < a.Cout) a.part[(long long)slice * a.row + a.boff + co] = v;
        }
    }
    const int chunk = chunk0 + wc;
    if (chunk >= x_chunks(a.s)) return;
    const bool soft = chunk < x_nsoft(a.s);
    const int cbase = soft ? 0 : a.s.Cl + (chunk - x_nsoft(a.s)) * 4, cend = soft ? a.s.Cl : a.Cin;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = cbase + j;
        if (ci >= cend) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int co = co0 + (rt0 + i) * 16 + kq * 4 + q;
                if (co >= a.Cout) continue;
                if (a.slices > 1) {
                    a.part[(long long)slice * a.row + ((long long)co * a.Cin + ci) * 16 + nl] = acc[i][j][q];
                } else {
                    float* p = wg_dw_ptr(a, co, ci, nl);
                    *p = a.accumulate ? *p + acc[i][j][q] : acc[i][j][q];
                }
            }
    }
}

// Adds the slices' rows in a fixed order and writes dw (+)= and dbias (+)=.  A workgroup owns 64 consecutive elements of the
// row; its four waves each add every fourth slice (loads unrolled: 512 slices one after the other are 512 memory latencies),
// then the four sums are added in wave order.
__global__ __launch_bounds__(NT) void conv2d_k4s2_wgrad_reduce_kernel(const WgArgs a) {
    __shared__ float red[4][64];
    const int q = threadIdx.x >> 6, l = threadIdx.x & 63;
    const long long e = blockIdx.x * 64LL + l;
    float s = 0.f;
    if (e < a.row) {
        const float* __restrict__ p = a.part + e;
#pragma unroll 8
        for (int k = q; k < a.slices; k += 4) s += p[(long long)k * a.row];
    }
    red[q][l] = s;
    __syncthreads();
    if (q != 0 || e >= a.row) return;
    s = ((red[0][l] + red[1][l]) + red[2][l]) + red[3][l];
    if (e < a.boff) {
        const long long r = e >> 4;
        const int co = (int)(r / a.Cin);
        float* p = wg_dw_ptr(a, co, (int)(r - (long long)co * a.Cin), (int)(e & 15));
        *p = a.accumulate ? *p + s : s;
    } else {
        const int co = (int)(e - a.boff);
        if (a.dbias) a.dbias[co] = a.accumulate ? a.dbias[co] + s : s;
        if (a.dbias2) a.dbias2[co] = a.accumulate ? a.dbias2[co] + s : s;
    }
}

// ------------------------------------------------------------------------------------------------ host side of the convolutions
struct Geo { int N, Ho, Wo; long long So; };

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int geo_check(int N, int Cout, int H, int W, Geo& g) {
    if (N <= 0 || Cout <= 0 || H <= 0 || W <= 0) return MIS_ERR_ARG;
    if ((H & 1) || (W & 1)) return MIS_ERR_UNSUPPORTED;
    g.N = N; g.Ho = H / 2; g.Wo = W / 2;
    g.So = (long long)g.Ho * g.Wo;
    if (g.So * N * Cout >= (1LL << 31) || N > 16383) return MIS_ERR_UNSUPPORTED;
    return MIS_OK;
}

int xsrc_make(const float* x, long long x_bs, int Cx, const float* logits, long long l_bs, int Cl, int H, int W, XSrc& s) {
    const int st = adv_xsrc_check(x, x_bs, Cx, logits, l_bs, Cl, (long long)H * W);
    if (st != MIS_OK) return st;
    s = XSrc{x, x_bs, Cx, logits, l_bs, Cl, H, W, (W % 4 == 0 && x_bs % 4 == 0 && al16(x)) ? 1 : 0,
             (W % 4 == 0 && l_bs % 4 == 0 && al16(logits)) ? 1 : 0};
    return MIS_OK;
}

GSrc gsrc_make(const float* dy, long long dy_bs, const float* y, long long y_bs, float slope, const float* drop, int Cout,
               const Geo& g) {
    const bool vec = g.Wo % 4 == 0 && dy_bs % 4 == 0 && al16(dy) && (!y || (y_bs % 4 == 0 && al16(y)));
    return GSrc{dy, dy_bs, y, y_bs, slope, drop, Cout, g.Ho, g.Wo, vec ? 1 : 0};
}

long long fwd_tiles(const Geo& g) { return mis_cdiv(g.Ho, F_TR) * mis_cdiv(g.Wo, 16); }

// slices of the forward's input-channel chunks: only when the tiles leave most CUs idle, at least 4 chunks (256 indices) each
int fwd_slices(int chunks, int Cout, const Geo& g) {
    const long long tiles = mis_cdiv(Cout, 64) * fwd_tiles(g) * g.N;
    if (tiles >= 256 || chunks < 8) return 1;
    long long s = 512 / tiles;
    if (s > chunks / 4) s = chunks / 4;
    if (s * g.N > 65535) s = 65535 / g.N;
    return s < 1 ? 1 : (int)s;
}

void wgrad_slices(int chunks, int Cout, const Geo& g, int& slices, long long& tiles_per) {
    const long long tiles = mis_cdiv(chunks, W_NC) * mis_cdiv(Cout, 64);
    const long long ptiles = (long long)g.N * mis_cdiv(g.Ho, W_TR) * mis_cdiv(g.Wo, 16);
    long long s = mis_cdiv(1024, tiles);
    if (s > 512) s = 512;
    if (s > ptiles) s = ptiles;
    tiles_per = mis_cdiv(ptiles, s);
    slices = (int)mis_cdiv(ptiles, tiles_per);
}

}  // namespace

extern "C" long long mis_conv2d_k4s2_fwd_workspace_bytes(int N, int Cin, int Cout, int H, int W) {
    Geo g;
    if (Cin <= 0) return MIS_ERR_ARG;
    const int st = geo_check(N, Cout, H, W, g);
    if (st) return st;
    // the split of Cin into softmax-read and plain channels moves the chunk count by at most one: take the larger
    const int s = fwd_slices((int)mis_cdiv(Cin, 4) + 1, Cout, g);
    return s > 1 ? (long long)s * N * Cout * g.So * 4 : 0;
}

extern "C" int mis_conv2d_k4s2_fwd(const float* x, long long x_bs, int Cx, const float* logits, long long l_bs, int Cl,
                                   const float* w_x, const float* w_l, const float* bias, const float* bias2, float* y,
                                   long long y_bs, int N, int Cout, int H, int W, float slope, const float* drop_scale,
                                   float* workspace, long long workspace_bytes, hipStream_t stream) {
    Geo g;
    int st = geo_check(N, Cout, H, W, g);
    if (st) return st;
    FwdArgs a{};
    st = xsrc_make(x, x_bs, Cx, logits, l_bs, Cl, H, W, a.s);
    if (st) return st;
    if (!y || (Cx > 0 && !w_x) || (Cl > 0 && !w_l) || !(slope > 0.f) || y_bs < Cout * g.So) return MIS_ERR_ARG;
    const int chunks = x_chunks(a.s);
    int slices = fwd_slices(chunks, Cout, g);
    const int per = (int)mis_cdiv(chunks, slices);
    slices = (int)mis_cdiv(chunks, per);
    if (slices > 1 && (!workspace || workspace_bytes < (long long)slices * N * Cout * g.So * 4)) return MIS_ERR_WORKSPACE;
    a.w_l = w_l; a.w_x = w_x;
    a.wvec = (!w_l || al16(w_l)) && (!w_x || al16(w_x));
    a.N = N; a.Cout = Cout; a.Ho = g.Ho; a.Wo = g.Wo; a.tiles_x = (int)mis_cdiv(g.Wo, 16);
    a.slices = slices; a.chunks_per = per; a.part = workspace;
    a.bias = bias; a.bias2 = bias2; a.slope = slope; a.drop = drop_scale; a.y = y; a.y_bs = y_bs;
    const dim3 grid((unsigned)fwd_tiles(g), (unsigned)mis_cdiv(Cout, 64), (unsigned)(N * slices));
    hipLaunchKernelGGL(conv2d_k4s2_fwd_kernel, grid, dim3(NT), 0, stream, a);
    st = mis_launch_status();
    if (st || slices == 1) return st;
    hipLaunchKernelGGL(conv2d_k4s2_fwd_reduce_kernel, dim3(stream_grid((long long)N * Cout * g.So)), dim3(NT), 0, stream, a);
    return mis_launch_status();
}

extern "C" int mis_conv2d_k4s2_dgrad(const float* dy, long long dy_bs, const float* y, long long y_bs, float slope,
                                     const float* drop_scale, const float* w, float* dx, long long dx_bs, int N, int Cin,
                                     int Cout, int H, int W, hipStream_t stream) {
    Geo g;
    const int st = geo_check(N, Cout, H, W, g);
    if (st) return st;
    if (!dy || !w || !dx || Cin <= 0 || !(slope > 0.f)) return MIS_ERR_ARG;
    if (dy_bs < Cout * g.So || (y && y_bs < Cout * g.So) || dx_bs < Cin * g.So * 4) return MIS_ERR_ARG;
    DgArgs a{gsrc_make(dy, dy_bs, y, y_bs, slope, drop_scale, Cout, g), w, al16(w) ? 1 : 0, Cout, Cin, (int)mis_cdiv(g.Wo, 16),
             dx, dx_bs};
    const unsigned tiles = (unsigned)(mis_cdiv(g.Ho, 8) * mis_cdiv(g.Wo, 16));
    if (Cin <= 4)
        hipLaunchKernelGGL(conv2d_k4s2_dgrad_map_kernel, dim3(tiles, 1, (unsigned)N), dim3(NT), 0, stream, a);
    else
        hipLaunchKernelGGL(conv2d_k4s2_dgrad_kernel, dim3(tiles, (unsigned)mis_cdiv(Cin, 64), (unsigned)(4 * N)), dim3(NT), 0,
                           stream, a);
    return mis_launch_status();
}

extern "C" long long mis_conv2d_k4s2_wgrad_workspace_bytes(int N, int Cin, int Cout, int H, int W) {
    Geo g;
    if (Cin <= 0) return MIS_ERR_ARG;
    const int st = geo_check(N, Cout, H, W, g);
    if (st) return st;
    // the slice count falls as the chunk count grows: the smallest chunk count bounds it
    int slices;
    long long per;
    wgrad_slices((int)mis_cdiv(Cin, 4), Cout, g, slices, per);
    return (long long)slices * ((slices > 1 ? (long long)Cout * Cin * 16 : 0) + Cout) * 4;      // + the bias partials
}

extern "C" int mis_conv2d_k4s2_wgrad(const float* x, long long x_bs, int Cx, const float* logits, long long l_bs, int Cl,
                                     const float* dy, long long dy_bs, const float* y, long long y_bs, float slope,
                                     const float* drop_scale, float* dw_x, float* dw_l, float* dbias, float* dbias2, int N,
                                     int Cout, int H, int W, int accumulate, float* workspace, long long workspace_bytes,
                                     hipStream_t stream) {
    Geo g;
    int st = geo_check(N, Cout, H, W, g);
    if (st) return st;
    WgArgs a{};
    st = xsrc_make(x, x_bs, Cx, logits, l_bs, Cl, H, W, a.s);
    if (st) return st;
    if (!dy || (Cx > 0 && !dw_x) || (Cl > 0 && !dw_l) || !(slope > 0.f)) return MIS_ERR_ARG;
    if (dy_bs < Cout * g.So || (y && y_bs < Cout * g.So)) return MIS_ERR_ARG;
    const int Cin = Cx + Cl, chunks = x_chunks(a.s);
    int slices;
    long long per;
    wgrad_slices(chunks, Cout, g, slices, per);
    a.boff = slices > 1 ? (long long)Cout * Cin * 16 : 0;
    a.row = a.boff + Cout;
    if (!workspace || workspace_bytes < slices * a.row * 4) return MIS_ERR_WORKSPACE;
    a.gs = gsrc_make(dy, dy_bs, y, y_bs, slope, drop_scale, Cout, g);
    a.N = N; a.Cout = Cout; a.Cin = Cin;
    a.tiles_x = (int)mis_cdiv(g.Wo, 16); a.tiles_y = (int)mis_cdiv(g.Ho, W_TR);
    a.slices = slices; a.tiles_per = per;
    a.dw_l = dw_l; a.dw_x = dw_x; a.part = workspace; a.accumulate = accumulate;
    a.dbias = dbias; a.dbias2 = dbias2;
    hipLaunchKernelGGL(conv2d_k4s2_wgrad_kernel,
                       dim3((unsigned)mis_cdiv(chunks, W_NC), (unsigned)mis_cdiv(Cout, 64), (unsigned)slices), dim3(NT), 0, stream, a);
    st = mis_launch_status();
    if (st) return st;
    if (slices > 1 || dbias || dbias2) {
        // slices == 1: the filter gradient is written already (boff = 0), the row holds the bias sums alone;
        // without a bias gradient its elements at the end of the row are left out
        const long long count = (dbias || dbias2) ? a.row : a.boff;
        hipLaunchKernelGGL(conv2d_k4s2_wgrad_reduce_kernel, dim3((unsigned)mis_cdiv(count, 64)), dim3(NT), 0, stream, a);
        st = mis_launch_status();
    }
    return st;
}

// =====================================================================================================
// Head: AvgPool2d((ph, pw)), stride = window, floor mode -> flatten -> Linear(C nwh nww, K) -> cross-entropy, mean over the
// samples.  workspace: pooled [N][F], dlogits [N][K], per-sample loss [N], F = C * nwh * nww.  The Linear and the
// cross-entropy are adv_common.h's, on F features.
// =====================================================================================================
namespace {

struct HeadGeo { int nwh, nww, F; };

// one wave per pooled feature: lane i sums window elements i, i + 64, .. in order, then the wave tree
__global__ __launch_bounds__(NT) void head2d_pool_kernel(const float* __restrict__ a, long long a_bs, int C, int H, int W,
                                                         int ph, int pw, int nwh, int nww, float* __restrict__ pooled) {
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6), n = blockIdx.y, nw = nwh * nww;
    if (f >= C * nw) return;
    const int c = f / nw, wi = f - c * nw, wy = wi / nww, wx = wi - wy * nww;
    const float* __restrict__ src = a + (long long)n * a_bs + ((long long)c * H + (long long)wy * ph) * W + (long long)wx * pw;
    float s = 0.f;
    for (int i = lane; i < ph * pw; i += 64) s += src[(long long)(i / pw) * W + i % pw];
    s = mis_wave_sum(s);
    if (lane == 0) pooled[(long long)n * C * nw + f] = s / (float)(ph * pw);
}

// da[n][c][y][x] = (sum_k dlogits[n][k] w[k][feature of (c, y / ph, x / pw)]) / (ph pw) inside the windows, 0 in the remainder
__global__ __launch_bounds__(NT) void head2d_bwd_da_kernel(const float* __restrict__ w, const float* __restrict__ dlogits, int C,
                                                           int K, int H, int W, int ph, int pw, int nwh, int nww,
                                                           float* __restrict__ da, long long da_bs) {
    const int c = blockIdx.x, n = blockIdx.y, nw = nwh * nww, F = C * nw;
    float* __restrict__ dst = da + (long long)n * da_bs + (long long)c * H * W;
    const float inv = 1.f / (float)(ph * pw);
    for (int i = threadIdx.x; i < H * W; i += NT) {
        const int yy = i / W, xx = i - yy * W, wy = yy / ph, wx = xx / pw;
        float g = 0.f;
        if (wy < nwh && wx < nww) {
            const int f = c * nw + wy * nww + wx;
            for (int k = 0; k < K; ++k) g += dlogits[n * K + k] * w[(long long)k * F + f];
            g *= inv;
        }
        dst[i] = g;
    }
}

int head2d_check(int N, int C, int K, int H, int W, int ph, int pw, HeadGeo& g) {
    if (N <= 0 || C <= 0 || K <= 0 || H <= 0 || W <= 0 || ph <= 0 || pw <= 0) return MIS_ERR_ARG;
    if (K > MAXK || N > 65535 || ph > H || pw > W) return MIS_ERR_UNSUPPORTED;
    g.nwh = H / ph; g.nww = W / pw;
    const long long F = (long long)C * g.nwh * g.nww;
    if (F * N >= (1LL << 31) || (long long)H * W >= (1LL << 31) || C > 65535 * 4) return MIS_ERR_UNSUPPORTED;
    g.F = (int)F;
    return MIS_OK;
}

}  // namespace

extern "C" long long mis_adv_head2d_workspace_bytes(int N, int C, int K, int H, int W, int pool_h, int pool_w) {
    HeadGeo g;
    const int st = head2d_check(N, C, K, H, W, pool_h, pool_w, g);
    if (st) return st;
    return ((long long)N * g.F + (long long)N * K + N) * 4;
}

extern "C" int mis_adv_head2d_fwd(const float* a, long long a_bs, const float* w, const float* b, const int* target,
                                  float* loss, float* logits, int N, int C, int K, int H, int W, int pool_h, int pool_w,
                                  float* workspace, long long workspace_bytes, hipStream_t stream) {
    HeadGeo g;
    const int st = head2d_check(N, C, K, H, W, pool_h, pool_w, g);
    if (st) return st;
    if (!a || !w || !target || !loss || !logits || !workspace || a_bs < (long long)C * H * W) return MIS_ERR_ARG;
    if (workspace_bytes < mis_adv_head2d_workspace_bytes(N, C, K, H, W, pool_h, pool_w)) return MIS_ERR_WORKSPACE;
    float* pooled = workspace;
    float* dlogits = pooled + (long long)N * g.F;
    float* per_sample = dlogits + (long long)N * K;
    hipLaunchKernelGGL(head2d_pool_kernel, dim3((unsigned)mis_cdiv(g.F, 4), (unsigned)N), dim3(NT), 0, stream, a, a_bs, C, H, W,
                       pool_h, pool_w, g.nwh, g.nww, pooled);
    hipLaunchKernelGGL(head_final_kernel, dim3(1), dim3(NT), 0, stream, pooled, w, b, target, N, g.F, K, logits, dlogits,
                       per_sample, loss);
    return mis_launch_status();
}

extern "C" int mis_adv_head2d_bwd(const float* w, float* da, long long da_bs, float* dw, float* db, int accumulate, int N,
                                  int C, int K, int H, int W, int pool_h, int pool_w, const float* workspace,
                                  long long workspace_bytes, hipStream_t stream) {
    HeadGeo g;
    const int st = head2d_check(N, C, K, H, W, pool_h, pool_w, g);
    if (st) return st;
    if (!w || !workspace || (da && da_bs < (long long)C * H * W)) return MIS_ERR_ARG;
    if (workspace_bytes < mis_adv_head2d_workspace_bytes(N, C, K, H, W, pool_h, pool_w)) return MIS_ERR_WORKSPACE;
    const float* pooled = workspace;
    const float* dlogits = pooled + (long long)N * g.F;
    if (da)
        hipLaunchKernelGGL(head2d_bwd_da_kernel, dim3((unsigned)C, (unsigned)N), dim3(NT), 0, stream, w, dlogits, C, K, H, W,
                           pool_h, pool_w, g.nwh, g.nww, da, da_bs);
    if (dw || db)
        hipLaunchKernelGGL(head_bwd_dw_kernel, dim3((unsigned)mis_cdiv((long long)K * g.F, NT)), dim3(NT), 0, stream, pooled,
                           dlogits, N, g.F, K, dw, db, accumulate);
    return mis_launch_status();
}
