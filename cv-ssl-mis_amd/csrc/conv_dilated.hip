// Dilated 3x3 convolution: forward, data gradient (the forward on flipped/transposed packed weights) and weight gradient.
//
// Replaces: nn.Conv2d(k=3, dilation=d, padding=d), d in {2, 4, 8, 16}   (reference code/networks/pnet.py:26-29, the
//           blocks 2..5 of PNet2D) and its autograd backward.  d = 1 stays on conv_fwd.hip / conv_wgrad.hip.
//
// Identity: a 3x3 convolution with dilation d and padding d touches, for an output pixel (y, x), only the rows y - d, y,
// y + d and the columns x - d, x, x + d.  The rows of one phase ry = y mod d therefore form an independent problem, and
// within it the rows y + (ky - 1) d are NEIGHBOURS: a tile of TY phase rows needs TY + 2 haloed phase rows, as the dense
// 3x3 kernel does.  The kernels decompose in y only.  Along x the tile stays dense (TX consecutive pixels, halo d on either
// side) and the three taps of a row are read from LDS d floats apart.  What that buys over the full (ry, rx) phase view:
//   * every DMA piece gathers consecutive floats of a row (whole cache lines), not floats d apart;
//   * the epilogue is the dense kernel's: (even, odd) pixel pairs as one float2, 128 contiguous bytes per channel per 16
//     lanes, where a lane of the (ry, rx) view would store single floats d apart;
// and what it costs: HX = TX + 2 d haloed columns instead of TX + 2 (LDS and DMA bytes x 1.06 / 1.18 / 1.41 / 1.88 for
// d = 2 / 4 / 8 / 16 at TX = 32), and three 8-byte LDS reads per tap row and pixel pair instead of two (d is even, so the
// float2 at pixel 2j + kx d holds tap kx of the even and of the odd pixel).  The MFMA loop, the operand maps, the LDS
// channel stride rule, the double-buffered LDS-DMA staging and the packed-weight layout are those of conv_fwd.hip.
//
// MFMA 16x16x4 f32 operand maps (forward):
//   A[i = lane&15][k = lane>>4]   -> weight  w[co0 + i][ci0 + k][tap]
//   B[k = lane>>4][j = lane&15]   -> input   x[ci0 + k][pixel(j) shifted by tap]
//   D[row = (lane>>4)*4 + r][col = lane&15]  -> y[co0 + row][pixel(col)]
// Weight gradient: M = 16 output channels, N = 16 input channels, K = pixels, one accumulator per tap, split-K over
// the (image, phase, tile) list with a fixed-order second pass -- conv_wgrad.hip with the same two address maps changed.
#include "common.h"
#include "../../include/mis_hip_dilated.h"
#include <stdio.h>

namespace {

using namespace mis_dma;   // LDS-DMA helpers (common.h)

struct DilFwdArgs {
    const float* x; long long x_bs;
    const float* wp;      // packed [Cin_pad4][9][Cout_pad16]
    const float* bias;    // [Cout] or nullptr
    float* y; long long y_bs;
    int N, Cin, Cout, Cin_pad, Cout_pad, H, W;
    int nphase, tiles_y, tiles_x, co_blocks;   // nphase = min(d, H): a phase without rows gets no workgroup
    unsigned n_blocks, n_blocks_padded;
    int st2;  // 1: output rows may be stored as aligned float2 (W even, 8-byte aligned rows)
};

template <int DIL_, int TY_, int TX_, int CO_B_, int CI_B_, int NT_>
struct DCfg {
    static constexpr int DIL = DIL_, TY = TY_, TX = TX_, CO_B = CO_B_, CI_B = CI_B_, NT = NT_;
    static constexpr int TAPS = 9;
    static constexpr int HY = TY + 2, HX = TX + 2 * DIL;   // haloed tile: phase rows x dense columns
    static constexpr int CS_RAW = HY * HX;
    static constexpr int NCH = (CS_RAW + 63) / 64;   // 64-dword DMA pieces per channel
    static constexpr int CS = NCH * 64 + 32;         // channel stride == 32 (mod 64), see conv_fwd.hip
    static constexpr int NP = NT / 2, M = CO_B / 16, PIX = TY * TX;
    static constexpr int IN_FLOATS = CI_B * CS;
    static constexpr int W_FLOATS = CI_B * TAPS * CO_B;
    static constexpr int W_PIECES = (W_FLOATS + 255) / 256;   // 1 KiB DMA pieces (64 lanes x 16 B)
    static constexpr int WPW = (W_PIECES + 3) / 4;            // pieces per wave
    static constexpr int STAGE = IN_FLOATS + W_PIECES * 256;  // floats per stage buffer
    static constexpr int LDS_BYTES = 2 * STAGE * 4;
    static constexpr int CPW = CI_B / 4;                      // input channels per wave
    static_assert(DIL % 2 == 0, "tap kx of an (even, odd) pixel pair is one aligned float2");
    static_assert(PIX == 64 * NT, "tile must hold 4 waves x NT x 16 pixels");
    static_assert(NT % 2 == 0 && TX % 2 == 0 && HX % 2 == 0, "even/odd pixel pairing needs even rows");
    static_assert(CO_B % 16 == 0 && CI_B % 4 == 0, "MFMA 16x16x4 granularity");
    static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
    static_assert(STAGE % 2 == 0, "float2 addressing of the stage buffers");
};

extern __shared__ __attribute__((aligned(16))) float mis_dil_lds[];

template <class C>
__global__ __launch_bounds__(256) void conv_dilated_fwd_kernel(const DilFwdArgs a) {
    float* const lds = mis_dil_lds;

    const unsigned L = mis_xcd_remap(blockIdx.x, a.n_blocks_padded);
    if (L >= a.n_blocks) return;
    unsigned t = L;
    const int cob = t % a.co_blocks; t /= a.co_blocks;
    const int tx = t % a.tiles_x;    t /= a.tiles_x;
    const int ty = t % a.tiles_y;    t /= a.tiles_y;
    const int ph = t % a.nphase;     t /= a.nphase;
    const int n = t;
    // phase row r of phase ph is image row ph + r * DIL; this tile owns phase rows [r0, r0 + TY)
    const int r0 = ty * C::TY, x0 = tx * C::TX, co0 = cob * C::CO_B;
    if (ph + r0 * C::DIL >= a.H) return;   // the phases' row counts differ by one: an empty last tile (whole workgroup)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lk = lane >> 4, lj = lane & 15;
    const long long S = (long long)a.H * a.W;
    const unsigned s_bytes = (unsigned)S * 4u;

    // buffer descriptors (raw, stride 0): x of this image [Cin][S], packed weights [Cin_pad][9][Cout_pad]
    const i32x4 rx = make_rsrc(a.x + (long long)n * a.x_bs, (unsigned)a.Cin * s_bytes);
    const i32x4 rw = make_rsrc(a.wp, (unsigned)a.Cin_pad * C::TAPS * a.Cout_pad * 4u);
    const unsigned lds0 = lds_addr(lds);

    // per-lane source byte offsets of this lane's element of every DMA piece (chunk-invariant):
    // piece p of a channel = halo elements [64p, 64p+64) of s_in[ci][hy][hx]; halo row hy is image row
    // ph + (r0 + hy - 1) * DIL, halo column hx is image column x0 + hx - DIL.  Outside the image: zeros (range check).
    unsigned voff[C::NCH];
#pragma unroll
    for (int p = 0; p < C::NCH; ++p) {
        const int e = p * 64 + lane;
        const int hy = e / C::HX, hx = e - hy * C::HX;
        const int gy = ph + (r0 + hy - 1) * C::DIL, gx = x0 + hx - C::DIL;
        const bool ok = e < C::CS_RAW && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
        voff[p] = ok ? (unsigned)(gy * a.W + gx) * 4u : OOB;
    }
    // weights: piece j = 64 float4 of s_w[ci][tap][co]; rows of CO_B floats, Cout_pad apart in HBM
    unsigned wvoff[C::WPW];
#pragma unroll
    for (int i = 0; i < C::WPW; ++i) {
        constexpr int VPR = C::CO_B / 4;
        const int e = (wave + 4 * i) * 64 + lane;
        const int row = e / VPR, q = e - row * VPR;
        const bool ok = e < C::W_FLOATS / 4 && co0 + q * 4 < a.Cout_pad;
        wvoff[i] = ok ? (unsigned)(row * a.Cout_pad + co0 + q * 4) * 4u : OOB;
    }

    auto stage = [&](int buf, int c0) {
        const unsigned st = lds0 + (unsigned)buf * (C::STAGE * 4);   // LDS byte address of the stage buffer
#pragma unroll
        for (int i = 0; i < C::CPW; ++i) {
            const int ci = wave + 4 * i;
            const unsigned cbase = (unsigned)(c0 + ci) * s_bytes;   // >= num_records for c >= Cin -> zeros
#pragma unroll
            for (int p = 0; p < C::NCH; ++p)
                dma_dword(st + (unsigned)(ci * C::CS + p * 64) * 4u, voff[p] + cbase, rx);
        }
        const unsigned wbase = (unsigned)c0 * (unsigned)(C::TAPS * 4) * (unsigned)a.Cout_pad;
#pragma unroll
        for (int i = 0; i < C::WPW; ++i) {
            const int j = wave + 4 * i;
            if (j < C::W_PIECES) dma_dwordx4(st + (unsigned)(C::IN_FLOATS + j * 256) * 4u, wvoff[i] + wbase, rw);
        }
    };

    // Pixel groups in even/odd pairs as in conv_fwd.hip: pair q of this wave covers 32 consecutive tile pixels, the even
    // MFMA column j is pixel 2j, the odd one pixel 2j+1.  po2[q]: per-lane offset (float2 units) of the pair's even pixel
    // in the haloed tile at tap (0, 0), incl. the k-lane channel.
    int po2[C::NP];
#pragma unroll
    for (int q = 0; q < C::NP; ++q) {
        const int p = (wave * C::NP + q) * 32 + 2 * lj;
        const int px = p % C::TX, py = p / C::TX;
        po2[q] = (py * C::HX + px + lk * C::CS) >> 1;
    }
    const int woff = C::IN_FLOATS + lk * C::TAPS * C::CO_B + lj;   // A operand: weights [ci][tap][co]

    f32x4 acc[C::M][C::NT];
#pragma unroll
    for (int m = 0; m < C::M; ++m)
#pragma unroll
        for (int i = 0; i < C::NT; ++i) acc[m][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Operands of one ky tap row: B = 3 x NP float2 (tap kx of the pair at + kx * DIL floats), A = 3 x M.  The operands of
    // row r+1 are fetched from LDS before the MFMAs of row r are issued (register double buffer).
    struct RowOps { float2 b[3][C::NP]; float av[3][C::M]; };
    constexpr int T = (C::CI_B / 4) * 3;   // tap rows per chunk (all CI_B channels: those >= Cin_pad hold zeros)

    auto compute = [&](const float* st) {
        const float2* __restrict__ s_in2 = reinterpret_cast<const float2*>(st);
        auto fetch = [&](RowOps& o, int t) {
            const int cq = t / 3, ky = t % 3;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
                for (int q = 0; q < C::NP; ++q)
                    o.b[kx][q] = s_in2[po2[q] + cq * 2 * C::CS + ((ky * C::HX + kx * C::DIL) >> 1)];
#pragma unroll
                for (int m = 0; m < C::M; ++m)
                    o.av[kx][m] = st[woff + cq * 4 * C::TAPS * C::CO_B + (ky * 3 + kx) * C::CO_B + m * 16];
            }
        };
        RowOps ops[2];
        fetch(ops[0], 0);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (t + 1 < T) fetch(ops[(t + 1) & 1], t + 1);
            __builtin_amdgcn_sched_barrier(0);   // keep the LDS reads of row t+1 ahead of the MFMAs of row t
            const RowOps& cur = ops[t & 1];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
                for (int q = 0; q < C::NP; ++q) {
#pragma unroll
                    for (int m = 0; m < C::M; ++m) {
                        acc[m][2 * q] =
                            __builtin_amdgcn_mfma_f32_16x16x4f32(cur.av[kx][m], cur.b[kx][q].x, acc[m][2 * q], 0, 0, 0);
                        acc[m][2 * q + 1] =
                            __builtin_amdgcn_mfma_f32_16x16x4f32(cur.av[kx][m], cur.b[kx][q].y, acc[m][2 * q + 1], 0, 0, 0);
                    }
                }
            }
        }
    };

    // ---- software pipeline over chunks of CI_B input channels: DMA(k+1) || MFMA(k) ----
    // The small-tile configurations hold 32 accumulator registers and can afford a second set (conv_fwd.hip's rule for its
    // small tiles): `acc` restarts with every chunk (CI_B * 9 products) and is folded into `tot`, which shortens the fp32
    // fmaf chain of a 64-channel layer from 576 to 72 products + 8 additions.
    constexpr bool FOLD = C::NT <= 4;
    f32x4 tot[FOLD ? C::M : 1][FOLD ? C::NT : 1];
    if constexpr (FOLD) {
#pragma unroll
        for (int m = 0; m < C::M; ++m)
#pragma unroll
            for (int i = 0; i < C::NT; ++i) tot[m][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int nchunks = (a.Cin_pad + C::CI_B - 1) / C::CI_B;
    stage(0, 0);
    dma_wait();
    __syncthreads();   // chunk 0 has landed for every wave
    for (int k = 0; k < nchunks; ++k) {
        if (k + 1 < nchunks) stage((k + 1) & 1, (k + 1) * C::CI_B);
        compute(lds + (k & 1) * C::STAGE);
        if constexpr (FOLD) {
#pragma unroll
            for (int m = 0; m < C::M; ++m)
#pragma unroll
                for (int i = 0; i < C::NT; ++i) {
                    tot[m][i] += acc[m][i];
                    acc[m][i] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
        }
        dma_wait();
        __syncthreads();   // chunk k+1 landed in the other buffer and every wave is done reading chunk k
    }
    if constexpr (FOLD) {
#pragma unroll
        for (int m = 0; m < C::M; ++m)
#pragma unroll
            for (int i = 0; i < C::NT; ++i) acc[m][i] = tot[m][i];
    }

    // ---- epilogue: bias + store.  D: row = lk*4 + r -> channel, col = lj -> pixel pair (2j, 2j+1) of one image row ----
    // Fast path (tile and channel block fully inside, float2-aligned rows): one buffer_store_dwordx2 per (pair, channel),
    // the channel in the scalar offset.  The descriptor covers this block's CO_B channels of the image.
    if (a.st2 && ph + (r0 + C::TY - 1) * C::DIL < a.H && x0 + C::TX <= a.W && co0 + C::CO_B <= a.Cout) {
        const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(a.y + (long long)n * a.y_bs + (long long)co0 * S), 0, (int)((unsigned)C::CO_B * s_bytes), 0x00020000);
        float bv[C::M][4];
#pragma unroll
        for (int m = 0; m < C::M; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) bv[m][r] = a.bias ? a.bias[co0 + m * 16 + lk * 4 + r] : 0.f;
        const unsigned lane_c = (unsigned)(lk * 4) * s_bytes;
#pragma unroll
        for (int q = 0; q < C::NP; ++q) {
            const int p = (wave * C::NP + q) * 32 + 2 * lj;
            const int px = p % C::TX, py = p / C::TX;
            const unsigned vo = lane_c + (unsigned)((ph + (r0 + py) * C::DIL) * a.W + x0 + px) * 4u;
#pragma unroll
            for (int m = 0; m < C::M; ++m) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    typedef float f32x2 __attribute__((ext_vector_type(2)));
                    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                    const f32x2 v = {acc[m][2 * q][r] + bv[m][r], acc[m][2 * q + 1][r] + bv[m][r]};
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), ry, (int)vo,
                                                          (int)((unsigned)(m * 16 + r) * s_bytes), 0);
                }
            }
        }
        return;
    }
    float* __restrict__ yout = a.y + (long long)n * a.y_bs;
#pragma unroll
    for (int q = 0; q < C::NP; ++q) {
        const int p = (wave * C::NP + q) * 32 + 2 * lj;
        const int px = p % C::TX, py = p / C::TX;
        const int gy = ph + (r0 + py) * C::DIL, gx = x0 + px;
        const bool row_ok = gy < a.H;
        const long long sp = (long long)gy * a.W + gx;
#pragma unroll
        for (int m = 0; m < C::M; ++m) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + m * 16 + lk * 4 + r;
                if (row_ok && co < a.Cout) {
                    const float bv = a.bias ? a.bias[co] : 0.f;
                    const float ve = acc[m][2 * q][r] + bv, vo = acc[m][2 * q + 1][r] + bv;
                    float* dst = yout + (long long)co * S + sp;
                    if (a.st2 && gx + 1 < a.W) {
                        *reinterpret_cast<float2*>(dst) = make_float2(ve, vo);
                    } else {
                        if (gx < a.W) dst[0] = ve;
                        if (gx + 1 < a.W) dst[1] = vo;
                    }
                }
            }
        }
    }
}

template <class C>
int launch_fwd(DilFwdArgs a, hipStream_t stream) {
    a.nphase = a.H < C::DIL ? a.H : C::DIL;
    a.tiles_y = (int)mis_cdiv(mis_cdiv(a.H, C::DIL), C::TY);   // of the longest phase
    a.tiles_x = (int)mis_cdiv(a.W, C::TX);
    a.co_blocks = (int)mis_cdiv(a.Cout_pad, C::CO_B);
    const long long nb = (long long)a.N * a.nphase * a.tiles_y * a.tiles_x * a.co_blocks;
    if (nb <= 0 || nb > 0x7fffffffLL) return MIS_ERR_ARG;
    a.n_blocks = (unsigned)nb;
    a.n_blocks_padded = (unsigned)(mis_cdiv(nb, MIS_NUM_XCD) * MIS_NUM_XCD);
    static std::atomic<unsigned long long> attr_done{0};   // per instantiation, one bit per device
    if (mis_set_lds_attr(reinterpret_cast<const void*>(&conv_dilated_fwd_kernel<C>), C::LDS_BYTES, attr_done) != MIS_OK)
        return MIS_ERR_LAUNCH;
    hipLaunchKernelGGL(conv_dilated_fwd_kernel<C>, dim3(a.n_blocks_padded), dim3(256), C::LDS_BYTES, stream, a);
    return mis_launch_status();
}

// One table for launch and for the profiling label, so both always agree.  Tiles as the dense 3x3 kernel picks them
// (16 x 32 for the large images, 16 x 16 below); at d = 16 the 16 x 32 tile's haloed rows are 64 floats wide, so its
// chunk is 4 channels instead of 8 to keep two stage buffers within the LDS of two workgroups per CU.
template <int DIL>
int dispatch_fwd_d(const DilFwdArgs& a, hipStream_t stream, char* name, int name_len) {
#define MIS_DF(TY, TX, COB, CIB, NT)                                                                              \
    do {                                                                                                          \
        if (name) {                                                                                               \
            snprintf(name, name_len, "conv_dilated_fwd_kernel<DCfg<%d, %d, %d, %d, %d, %d>>", DIL, TY, TX, COB, CIB, NT); \
            return MIS_OK;                                                                                        \
        }                                                                                                         \
        return launch_fwd<DCfg<DIL, TY, TX, COB, CIB, NT>>(a, stream);                                            \
    } while (0)
    const bool wide = a.Cout_pad % 32 == 0;
    constexpr int CIB = DIL == 16 ? 4 : 8;
    if (a.W >= 128) {
        if (wide) MIS_DF(16, 32, 32, CIB, 8); else MIS_DF(16, 32, 16, CIB, 8);
    } else {
        if (wide) MIS_DF(16, 16, 32, 8, 4); else MIS_DF(16, 16, 16, 8, 4);
    }
#undef MIS_DF
}

int dispatch_fwd(const DilFwdArgs& a, int d, hipStream_t stream, char* name, int name_len) {
    switch (d) {
        case 2: return dispatch_fwd_d<2>(a, stream, name, name_len);
        case 4: return dispatch_fwd_d<4>(a, stream, name, name_len);
        case 8: return dispatch_fwd_d<8>(a, stream, name, name_len);
        case 16: return dispatch_fwd_d<16>(a, stream, name, name_len);
    }
    return MIS_ERR_UNSUPPORTED;
}

bool dil_ok(int d) { return d == 2 || d == 4 || d == 8 || d == 16; }

// the DMA descriptors address one image's channels with 32-bit byte offsets (the limit of mis_conv_fwd)
bool geom_ok(int c, int H, int W) { return ((long long)c + 32) * ((long long)H * W) * 4 < (1LL << 30); }

DilFwdArgs make_fwd_args(const float* x, long long x_bs, const float* wp, const float* bias, float* y, long long y_bs,
                         int N, int Cin, int Cout, int H, int W) {
    DilFwdArgs a{};
    a.x = x; a.x_bs = x_bs; a.wp = wp; a.bias = bias; a.y = y; a.y_bs = y_bs;
    a.N = N; a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W;
    a.Cin_pad = mis_conv_cin_pad(Cin);
    a.Cout_pad = mis_conv_cout_pad(Cout);
    a.st2 = (W % 2 == 0 && y_bs % 2 == 0 && ((uintptr_t)y & 7) == 0) ? 1 : 0;
    return a;
}

// ---------------------------------------------------------------------------------------------------------
// Weight gradient.  dw[co][ci][ky][kx] = sum_{n, y, x} dy[n][co][y][x] * x[n][ci][y + (ky-1) d][x + (kx-1) d].
// A pixel tile is TY rows of one phase x TX dense columns of one image; the list of tiles (image, phase, tile row, tile
// column) is walked split-K by the workgroups of a (co-tile, ci-tile) pair, exactly as conv_wgrad.hip walks its own.
// ---------------------------------------------------------------------------------------------------------
struct DilWgradArgs {
    const float* x; long long x_bs;
    const float* dy; long long dy_bs;
    float* ws;  // [KS][pairs][9][256]
    int N, Cin, Cout, H, W;
    int nphase, tiles_y, tiles_x, tiles_total;
    int ci_tiles, pairs, KS;
    unsigned n_blocks_padded;
};

template <int DIL_, int TY_, int TX_>
struct DWCfg {
    static constexpr int DIL = DIL_, TY = TY_, TX = TX_, TAPS = 9;
    static constexpr int HY = TY + 2, HX = TX + 2 * DIL;
    static constexpr int XS_RAW = HY * HX, PIX = TY * TX;
    static constexpr int NCHX = (XS_RAW + 63) / 64, NCHD = (PIX + 63) / 64;   // 64-dword DMA pieces / channel
    static constexpr int XS = NCHX * 64 + 4, DS = NCHD * 64 + 4;             // 4 * odd: conflict-free 8-byte reads
    static constexpr int X_FLOATS = 16 * XS, DY_FLOATS = 16 * DS;
    static constexpr int STAGE = X_FLOATS + DY_FLOATS;
    static constexpr int RED_FLOATS = TAPS * 256;
    static constexpr int LDS_FLOATS = STAGE > RED_FLOATS ? STAGE : RED_FLOATS;
    static constexpr int LDS_BYTES = LDS_FLOATS * 4;
    static_assert(DIL % 2 == 0 && TX % 8 == 0 && PIX % 32 == 0 && HX % 2 == 0, "even/odd pixel-quad pairs");
    static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
};

template <class C>
__global__ __launch_bounds__(256) void conv_dilated_wgrad_kernel(const DilWgradArgs a) {
    float* const smem = mis_dil_lds;

    const unsigned L = mis_xcd_remap(blockIdx.x, a.n_blocks_padded);
    if (L >= (unsigned)(a.pairs * a.KS)) return;
    const int pair = L % a.pairs, ks = L / a.pairs;
    const int mt = pair / a.ci_tiles, jt = pair % a.ci_tiles;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lk = lane >> 4, lj = lane & 15;
    const unsigned s_bytes = (unsigned)(a.H * a.W) * 4u;
    const unsigned lds0 = lds_addr(smem);
    const int ci0 = jt * 16, co0 = mt * 16;

    f32x4 acc[C::TAPS];
#pragma unroll
    for (int t = 0; t < C::TAPS; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // DMA of pixel tile `tile`: wave w brings channels w, w+4, w+8, w+12 of both operands.  Rows beyond the phase and
    // columns beyond the image deliver zeros (range check): such pixels add exact zeros to every tap.
    auto issue = [&](int tile) {
        int t = tile;
        const int tx = t % a.tiles_x; t /= a.tiles_x;
        const int ty = t % a.tiles_y; t /= a.tiles_y;
        const int ph = t % a.nphase;  t /= a.nphase;
        const int n = t;
        const int r0 = ty * C::TY, x0 = tx * C::TX;
        const i32x4 rx = make_rsrc(a.x + (long long)n * a.x_bs, (unsigned)a.Cin * s_bytes);
        const i32x4 rd = make_rsrc(a.dy + (long long)n * a.dy_bs, (unsigned)a.Cout * s_bytes);
#pragma unroll
        for (int p = 0; p < C::NCHX; ++p) {
            const int e = p * 64 + lane;
            const int hy = e / C::HX, hx = e - hy * C::HX;
            const int gy = ph + (r0 + hy - 1) * C::DIL, gx = x0 + hx - C::DIL;
            const bool ok = e < C::XS_RAW && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
            const unsigned vo = ok ? (unsigned)(gy * a.W + gx) * 4u : OOB;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = wave + 4 * i;   // channel >= Cin: beyond num_records -> zeros
                dma_dword(lds0 + (unsigned)(c * C::XS + p * 64) * 4u, vo + (unsigned)(ci0 + c) * s_bytes, rx);
            }
        }
#pragma unroll
        for (int p = 0; p < C::NCHD; ++p) {
            const int e = p * 64 + lane;
            const int px = e % C::TX, py = e / C::TX;
            const int gy = ph + (r0 + py) * C::DIL, gx = x0 + px;
            const bool ok = e < C::PIX && gy < a.H && gx < a.W;
            const unsigned vo = ok ? (unsigned)(gy * a.W + gx) * 4u : OOB;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = wave + 4 * i;
                dma_dword(lds0 + (unsigned)(C::X_FLOATS + c * C::DS + p * 64) * 4u, vo + (unsigned)(co0 + c) * s_bytes, rd);
            }
        }
    };

    // 8 consecutive pixels per step = an "even" K-quad (pixels p0+2k) and an "odd" one (p0+2k+1): one 8-byte LDS read at
    // pixel p0 + 2k + kx * DIL holds tap kx of both quads.
    auto compute = [&](const float* st) {
        const float2* __restrict__ s_x2 = reinterpret_cast<const float2*>(st);
        const float2* __restrict__ s_dy2 = reinterpret_cast<const float2*>(st + C::X_FLOATS);
        for (int g = wave; g < C::PIX / 8; g += 4) {
            const int p0 = g * 8;
            const int px0 = p0 % C::TX, py = p0 / C::TX;
            const float2 av = s_dy2[(lj * C::DS + p0 + 2 * lk) >> 1];
            const int xb2 = (lj * C::XS + py * C::HX + px0 + 2 * lk) >> 1;
            float be[C::TAPS], bo[C::TAPS];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float2 r = s_x2[xb2 + ((ky * C::HX + kx * C::DIL) >> 1)];
                    be[ky * 3 + kx] = r.x;
                    bo[ky * 3 + kx] = r.y;
                }
#pragma unroll
            for (int tap = 0; tap < C::TAPS; ++tap)
                acc[tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, be[tap], acc[tap], 0, 0, 0);
#pragma unroll
            for (int tap = 0; tap < C::TAPS; ++tap)
                acc[tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bo[tap], acc[tap], 0, 0, 0);
        }
    };

    for (int tile = ks; tile < a.tiles_total; tile += a.KS) {
        __syncthreads();   // previous tile fully consumed
        issue(tile);
        dma_wait();
        __syncthreads();
        compute(smem);
    }

    // ---- combine the 4 waves through LDS (wave 0 accumulates, fixed order), then write the partial ----
#pragma unroll 1
    for (int w = 1; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < C::TAPS; ++t) *reinterpret_cast<f32x4*>(&smem[(t * 64 + lane) * 4]) = acc[t];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int t = 0; t < C::TAPS; ++t) acc[t] += *reinterpret_cast<const f32x4*>(&smem[(t * 64 + lane) * 4]);
        }
    }
    if (wave == 0) {
        float* __restrict__ out = a.ws + ((long long)ks * a.pairs + pair) * (C::TAPS * 256);
#pragma unroll
        for (int t = 0; t < C::TAPS; ++t) *reinterpret_cast<f32x4*>(&out[(t * 64 + lane) * 4]) = acc[t];
    }
}

struct DilWredArgs {
    const float* ws;
    float* dw;  // [Cout][Cin][9]
    int Cin, Cout, ci_tiles, pairs, KS, accumulate;
};

// One workgroup of 16 waves per (channel-tile pair, tap): wave w sums the partial tiles k = w, w+16, ... as coalesced
// float4 rows, the 16 wave sums are combined through LDS in a fixed order, and lane l writes its four dw entries
// (co = 16*mt + 4*(l>>4) + r, ci = 16*jt + (l&15)).  The second pass of conv_wgrad.hip.
constexpr int RED_WAVES = 16;

__global__ __launch_bounds__(64 * RED_WAVES) void conv_dilated_wgrad_reduce_kernel(const DilWredArgs a) {
    __shared__ f32x4 red[RED_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pair = blockIdx.x / 9, tap = blockIdx.x - pair * 9;
    const float* __restrict__ base = a.ws + ((long long)pair * 9 + tap) * 256 + lane * 4;
    const long long stride = (long long)a.pairs * 9 * 256;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int k = wave; k < a.KS; k += RED_WAVES) s += *reinterpret_cast<const f32x4*>(base + k * stride);
    red[wave][lane] = s;
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < RED_WAVES; ++w) s += red[w][lane];
    const int mt = pair / a.ci_tiles, jt = pair - mt * a.ci_tiles;
    const int ci = jt * 16 + (lane & 15);
    if (ci >= a.Cin) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int co = mt * 16 + (lane >> 4) * 4 + r;
        if (co < a.Cout) {
            float* p = a.dw + ((long long)co * a.Cin + ci) * 9 + tap;
            *p = a.accumulate ? *p + s[r] : s[r];
        }
    }
}

// Split-K factor: conv_wgrad.hip's cost model (rounds x (tiles per workgroup + fixed cost)), a pure function of its
// arguments, so the workspace query and the launch always agree.
int pick_ks(int pairs, int tiles_total, int slots) {
    const int E = 3;
    int kmax = tiles_total < 2048 ? tiles_total : 2048;
    if (kmax < 1) kmax = 1;
    long long best_t = -1;
    int best = 1;
    for (int ks = 1; ks <= kmax; ++ks) {
        const long long rounds = ((long long)pairs * ks + slots - 1) / slots;
        const long long t = rounds * ((tiles_total + ks - 1) / ks + E);
        if (best_t < 0 || t < best_t) { best_t = t; best = ks; }
    }
    return best;
}

template <class C>
bool fill_tiles(DilWgradArgs& a) {
    a.nphase = a.H < C::DIL ? a.H : C::DIL;
    a.tiles_y = (int)mis_cdiv(mis_cdiv(a.H, C::DIL), C::TY);
    a.tiles_x = (int)mis_cdiv(a.W, C::TX);
    const long long total = (long long)a.N * a.nphase * a.tiles_y * a.tiles_x;
    if (total <= 0 || total > 0x7fffffffLL) return false;
    a.tiles_total = (int)total;
    const int by_lds = (160 * 1024) / C::LDS_BYTES;
    const int per_cu = by_lds < 5 ? (by_lds < 1 ? 1 : by_lds) : 5;   // registers: 9 accumulators + operands
    a.KS = pick_ks(a.pairs, a.tiles_total, 256 * per_cu);
    return true;
}

template <class C>
int run_wgrad(DilWgradArgs a, float* dw, long long ws_bytes, int accumulate, hipStream_t stream, long long* out_ws,
              const char* label, const char** out_name) {
    if (out_name) { *out_name = label; return MIS_OK; }
    if (!fill_tiles<C>(a)) return MIS_ERR_ARG;
    const long long need = (long long)a.KS * a.pairs * C::TAPS * 256 * 4;
    if (out_ws) { *out_ws = need; return MIS_OK; }
    if (need > ws_bytes) return MIS_ERR_WORKSPACE;
    static std::atomic<unsigned long long> attr_done{0};   // per instantiation, one bit per device
    if (mis_set_lds_attr(reinterpret_cast<const void*>(&conv_dilated_wgrad_kernel<C>), C::LDS_BYTES, attr_done) != MIS_OK)
        return MIS_ERR_LAUNCH;
    a.n_blocks_padded = (unsigned)(mis_cdiv((long long)a.pairs * a.KS, MIS_NUM_XCD) * MIS_NUM_XCD);
    hipLaunchKernelGGL(conv_dilated_wgrad_kernel<C>, dim3(a.n_blocks_padded), dim3(256), C::LDS_BYTES, stream, a);
    int st = mis_launch_status();
    if (st) return st;
    DilWredArgs r{a.ws, dw, a.Cin, a.Cout, a.ci_tiles, a.pairs, a.KS, accumulate};
    hipLaunchKernelGGL(conv_dilated_wgrad_reduce_kernel, dim3((unsigned)(a.pairs * 9)), dim3(64 * RED_WAVES), 0, stream, r);
    return mis_launch_status();
}

// mode: out_name set -> label; out_ws set -> workspace bytes; else run
int dispatch_wgrad(const DilWgradArgs& a, int d, float* dw, long long ws_bytes, int accumulate, hipStream_t stream,
                   long long* out_ws, const char** out_name) {
#define MIS_DW(DIL, TY, TX) \
    return run_wgrad<DWCfg<DIL, TY, TX>>(a, dw, ws_bytes, accumulate, stream, out_ws, \
                                         "conv_dilated_wgrad_kernel<DWCfg<" #DIL ", " #TY ", " #TX ">>", out_name)
    const bool big = a.W >= 32;   // the dense kernel's rule: 8 x 32 tiles, 16 x 16 for the narrow images
    switch (d) {
        case 2: if (big) MIS_DW(2, 8, 32); else MIS_DW(2, 16, 16);
        case 4: if (big) MIS_DW(4, 8, 32); else MIS_DW(4, 16, 16);
        case 8: if (big) MIS_DW(8, 8, 32); else MIS_DW(8, 16, 16);
        case 16: if (big) MIS_DW(16, 8, 32); else MIS_DW(16, 16, 16);
    }
#undef MIS_DW
    return MIS_ERR_UNSUPPORTED;
}

DilWgradArgs make_wgrad_args(const float* x, long long x_bs, const float* dy, long long dy_bs, float* ws, int N, int Cin,
                             int Cout, int H, int W) {
    DilWgradArgs a{};
    a.x = x; a.x_bs = x_bs; a.dy = dy; a.dy_bs = dy_bs; a.ws = ws;
    a.N = N; a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W;
    a.ci_tiles = (Cin + 15) / 16;
    a.pairs = ((Cout + 15) / 16) * a.ci_tiles;
    return a;
}

int fwd_entry(const float* x, long long x_bs, const float* wp, const float* bias, float* y, long long y_bs, int N, int Cin,
              int Cout, int H, int W, int d, hipStream_t stream) {
    if (!x || !wp || !y || N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return MIS_ERR_ARG;
    if (!dil_ok(d) || !geom_ok(Cin > Cout ? Cin : Cout, H, W) || ((uintptr_t)wp & 15) != 0) return MIS_ERR_UNSUPPORTED;
    const long long S = (long long)H * W;
    if (x_bs < (long long)Cin * S || y_bs < (long long)Cout * S) return MIS_ERR_ARG;
    return dispatch_fwd(make_fwd_args(x, x_bs, wp, bias, y, y_bs, N, Cin, Cout, H, W), d, stream, nullptr, 0);
}

int fwd_name(int N, int Cin, int Cout, int H, int W, int d, char* name, int name_len) {
    if (!name || name_len <= 0 || N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return MIS_ERR_ARG;
    if (!dil_ok(d) || !geom_ok(Cin > Cout ? Cin : Cout, H, W)) return MIS_ERR_UNSUPPORTED;
    return dispatch_fwd(make_fwd_args(nullptr, 0, nullptr, nullptr, nullptr, 0, N, Cin, Cout, H, W), d, nullptr, name,
                        name_len);
}

}  // namespace

extern "C" int mis_conv_dilated_fwd(const float* x, long long x_bs, const float* wp, const float* bias, float* y,
                                    long long y_bs, int N, int Cin, int Cout, int H, int W, int dilation,
                                    hipStream_t stream) {
    return fwd_entry(x, x_bs, wp, bias, y, y_bs, N, Cin, Cout, H, W, dilation, stream);
}

// the forward launch on (dy, mode-1 pack): Cout channels in, Cin channels out
extern "C" int mis_conv_dilated_dgrad(const float* dy, long long dy_bs, const float* wpd, float* dx, long long dx_bs, int N,
                                      int Cin, int Cout, int H, int W, int dilation, hipStream_t stream) {
    return fwd_entry(dy, dy_bs, wpd, nullptr, dx, dx_bs, N, Cout, Cin, H, W, dilation, stream);
}

extern "C" int mis_conv_dilated_fwd_kernel_name(int N, int Cin, int Cout, int H, int W, int dilation, char* name,
                                                int name_len) {
    return fwd_name(N, Cin, Cout, H, W, dilation, name, name_len);
}

extern "C" int mis_conv_dilated_dgrad_kernel_name(int N, int Cin, int Cout, int H, int W, int dilation, char* name,
                                                  int name_len) {
    return fwd_name(N, Cout, Cin, H, W, dilation, name, name_len);
}

extern "C" long long mis_conv_dilated_wgrad_workspace_bytes(int N, int Cin, int Cout, int H, int W, int dilation) {
    if (N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return MIS_ERR_ARG;
    if (!dil_ok(dilation) || !geom_ok(Cin > Cout ? Cin : Cout, H, W)) return MIS_ERR_UNSUPPORTED;
    long long out = 0;
    const int st = dispatch_wgrad(make_wgrad_args(nullptr, 0, nullptr, 0, nullptr, N, Cin, Cout, H, W), dilation, nullptr, 0,
                                  0, nullptr, &out, nullptr);
    return st ? st : out;
}

extern "C" int mis_conv_dilated_wgrad_kernel_name(int N, int Cin, int Cout, int H, int W, int dilation, char* name,
                                                  int name_len) {
    if (!name || name_len <= 0 || N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return MIS_ERR_ARG;
    if (!dil_ok(dilation) || !geom_ok(Cin > Cout ? Cin : Cout, H, W)) return MIS_ERR_UNSUPPORTED;
    const char* n = nullptr;
    const int st = dispatch_wgrad(make_wgrad_args(nullptr, 0, nullptr, 0, nullptr, N, Cin, Cout, H, W), dilation, nullptr, 0,
                                  0, nullptr, nullptr, &n);
    if (st) return st;
    snprintf(name, name_len, "%s", n);
    return MIS_OK;
}

extern "C" int mis_conv_dilated_wgrad(const float* x, long long x_bs, const float* dy, long long dy_bs, float* dw,
                                      float* workspace, long long workspace_bytes, int N, int Cin, int Cout, int H, int W,
                                      int dilation, int accumulate, hipStream_t stream) {
    if (!x || !dy || !dw || !workspace || N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return MIS_ERR_ARG;
    if (!dil_ok(dilation) || !geom_ok(Cin > Cout ? Cin : Cout, H, W)) return MIS_ERR_UNSUPPORTED;
    const long long S = (long long)H * W;
    if (x_bs < (long long)Cin * S || dy_bs < (long long)Cout * S) return MIS_ERR_ARG;
    return dispatch_wgrad(make_wgrad_args(x, x_bs, dy, dy_bs, workspace, N, Cin, Cout, H, W), dilation, dw, workspace_bytes,
                          accumulate, stream, nullptr, nullptr);
}
