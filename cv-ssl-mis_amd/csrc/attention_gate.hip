// Grid attention gates of the 3-D Attention U-Net (reference code/networks/grid_attention_layer.py:84-107 as
// MultiAttentionBlock uses it, code/networks/attention_unet.py:113-136) and trilinear up-sampling by 2 / 4 / 8 with its adjoint
// (the deep-supervision heads, code/networks/utils.py:455-462).  The ABI and the formulas: include/mis_hip_attention_gate.h.
//
// All of it is memory-bound.  The fine-resolution operands (x, y, dy, dx, the up-sampled outputs) move as float4 along W when
// W % 4 == 0 and the pointers / batch strides allow it, one float per thread otherwise; the coarse attention maps are read
// through the caches (8 taps per fine voxel, 1 / C of the fine traffic).  Sums run in a fixed order: over channels inside a
// thread, over a footprint inside a wave (xor tree), over workgroup partials in a second launch.  No atomics.
#include "common.h"
#include "../../include/mis_hip_attention_gate.h"

namespace {

constexpr int MAXG = 4;          // gates per launch the register arrays hold (the net uses 2)

// cells i0 <= i1 and the weight l1 of i1 that output index o reads on an axis of n cells up-sampled by 1 / inv_s
// (align_corners=False: source coordinate (o + 0.5) / s - 0.5, clamped below at 0; exact in fp32, s is a power of two)
__device__ __forceinline__ void up_src(int o, int n, float inv_s, int& i0, int& i1, float& l1) {
    const float src = fmaxf(((float)o + 0.5f) * inv_s - 0.5f, 0.f);
    i0 = min((int)src, n - 1);
    i1 = min(i0 + 1, n - 1);
    l1 = src - (float)i0;
}

// weight with which output o (of no) reads cell i (of n): 0 outside the volume
__device__ __forceinline__ float up_weight(int o, int i, int n, int no, float inv_s) {
    if (o < 0 || o >= no) return 0.f;
    int i0, i1;
    float l1;
    up_src(o, n, inv_s, i0, i1, l1);
    return (i0 == i ? 1.f - l1 : 0.f) + (i1 == i ? l1 : 0.f);
}

// trilinear value of the coarse volume a[d][h][w] at V consecutive fine cells (oz, oy, ox0 ..)
template <int V>
__device__ __forceinline__ void up_values(const float* __restrict__ a, int h, int w, int z0, int z1, float lz, int y0, int y1,
                                          float ly, int ox0, float inv_s, float (&out)[V]) {
    const float* __restrict__ r00 = a + (z0 * h + y0) * w;
    const float* __restrict__ r01 = a + (z0 * h + y1) * w;
    const float* __restrict__ r10 = a + (z1 * h + y0) * w;
    const float* __restrict__ r11 = a + (z1 * h + y1) * w;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        int x0, x1;
        float lx;
        up_src(ox0 + j, w, inv_s, x0, x1, lx);
        const float v00 = r00[x0] + lx * (r00[x1] - r00[x0]);
        const float v01 = r01[x0] + lx * (r01[x1] - r01[x0]);
        const float v10 = r10[x0] + lx * (r10[x1] - r10[x0]);
        const float v11 = r11[x0] + lx * (r11[x1] - r11[x0]);
        const float v0 = v00 + ly * (v01 - v00);
        const float v1 = v10 + ly * (v11 - v10);
        out[j] = v0 + lz * (v1 - v0);
    }
}

template <int V> struct Vec;
template <> struct Vec<1> {
    static __device__ __forceinline__ void load(const float* p, float (&v)[1]) { v[0] = *p; }
    static __device__ __forceinline__ void store(float* p, const float (&v)[1]) { *p = v[0]; }
};
template <> struct Vec<4> {
    static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4]) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    }
};

// ------------------------------------------------------------------------------------------------ gate map
struct MapArgs {
    const float *theta, *phi, *psi_w, *psi_b;
    float* att;
    long long theta_bs, phi_bs, att_bs;
    int G, Ci, s;
};

// one thread per (n, g, coarse voxel): the 1x1x1 psi convolution over relu(theta + phi), then the sigmoid
__global__ __launch_bounds__(256) void gate_map_fwd_kernel(const MapArgs a) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= a.s) return;
    const int g = blockIdx.y, n = blockIdx.z;
    const long long ch = (long long)g * a.Ci * a.s + u;
    const float* __restrict__ t = a.theta + (long long)n * a.theta_bs + ch;
    const float* __restrict__ p = a.phi + (long long)n * a.phi_bs + ch;
    const float* __restrict__ wv = a.psi_w + g * a.Ci;
    float acc = a.psi_b[g];
#pragma unroll 4
    for (int i = 0; i < a.Ci; ++i) acc = fmaf(wv[i], fmaxf(t[(long long)i * a.s] + p[(long long)i * a.s], 0.f), acc);
    a.att[(long long)n * a.att_bs + (long long)g * a.s + u] = 1.f / (1.f + expf(-acc));
}

struct MapBwdArgs {
    const float *datt, *att, *theta, *phi, *psi_w;
    float *df;
    float2* part;
    long long datt_bs, att_bs, theta_bs, phi_bs, df_bs;
    int G, Ci, s, total, nchunks;       // total = N * s
};

constexpr int MB_EPB = 2048;     // (image, voxel) pairs per workgroup of the map backward

// workgroup = (chunk of (image, voxel) pairs, row): rows 0 .. G Ci - 1 are the channels (g, i) -- df of the channel and the
// partial sums of dpsi_w[g][i] and of df itself (the bias gradient of the phi convolution) -- rows G Ci .. G Ci + G - 1 the
// partial sums of dpsi_b[g]
__global__ __launch_bounds__(256) void gate_map_bwd_kernel(const MapBwdArgs a) {
    __shared__ float red[8];
    const int row = blockIdx.y, chunk = blockIdx.x;
    const bool bias_row = row >= a.G * a.Ci;
    const int g = bias_row ? row - a.G * a.Ci : row / a.Ci;
    const float wv = bias_row ? 0.f : a.psi_w[row];
    float acc[2] = {0.f, 0.f};
#pragma unroll 2
    for (int k = 0; k < MB_EPB / 256; ++k) {
        const int e = chunk * MB_EPB + k * 256 + (int)threadIdx.x;
        if (e >= a.total) break;
        const int n = e / a.s, u = e - n * a.s;
        const float av = a.att[(long long)n * a.att_bs + (long long)g * a.s + u];
        const float dp = a.datt[(long long)n * a.datt_bs + (long long)g * a.s + u] * av * (1.f - av);
        if (bias_row) {
            acc[0] += dp;
        } else {
            const long long ch = (long long)row * a.s + u;
            const float f = a.theta[(long long)n * a.theta_bs + ch] + a.phi[(long long)n * a.phi_bs + ch];
            const float d = f > 0.f ? wv * dp : 0.f;
            a.df[(long long)n * a.df_bs + ch] = d;
            acc[1] += d;
            if (f > 0.f) acc[0] = fmaf(f, dp, acc[0]);
        }
    }
    mis_block_sum<2>(acc, red);
    if (threadIdx.x == 0) a.part[(long long)row * a.nchunks + chunk] = make_float2(acc[0], acc[1]);
}

// one wave per row: lane-strided sums over the chunks, then the wave's xor tree
__global__ __launch_bounds__(64) void gate_map_bwd_final_kernel(const float2* __restrict__ part, int nchunks, int n_w,
                                                                float* dpsi_w, float* dpsi_b, float* dphi_b, int accumulate) {
    const int row = blockIdx.x;
    float s = 0.f, t = 0.f;
    for (int c = threadIdx.x; c < nchunks; c += 64) {
        const float2 v = part[(long long)row * nchunks + c];
        s += v.x;
        t += v.y;
    }
    s = mis_wave_sum(s);
    t = mis_wave_sum(t);
    if (threadIdx.x == 0) {
        float* o = row < n_w ? dpsi_w + row : dpsi_b + (row - n_w);
        *o = accumulate ? *o + s : s;
        if (dphi_b && row < n_w) dphi_b[row] = accumulate ? dphi_b[row] + t : t;
    }
}

// ------------------------------------------------------------------------------------------------ gate apply
struct ApplyArgs {
    const float *x, *att, *dy;
    float *y, *dx, *sc;
    long long x_bs, att_bs, y_bs, dy_bs, dx_bs;
    int G, C, D, H, W, d, h, w, accumulate;
};

// the G up-sampled attention values at this thread's V fine cells; false: the thread has no cell
template <int V>
__device__ __forceinline__ bool gate_cells(const ApplyArgs& a, int n, long long& off, float (&aw)[MAXG][V]) {
    const int WQ = a.W / V;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= a.D * a.H * WQ) return false;
    const int xq = q % WQ, r = q / WQ;
    const int oy = r % a.H, oz = r / a.H;
    off = ((long long)oz * a.H + oy) * a.W + xq * V;
    int z0, z1, y0, y1;
    float lz, ly;
    up_src(oz, a.d, 0.5f, z0, z1, lz);
    up_src(oy, a.h, 0.5f, y0, y1, ly);
    const int s = a.d * a.h * a.w;
#pragma unroll
    for (int g = 0; g < MAXG; ++g)
        if (g < a.G)
            up_values<V>(a.att + (long long)n * a.att_bs + (long long)g * s, a.h, a.w, z0, z1, lz, y0, y1, ly, xq * V, 0.5f,
                         aw[g]);
    return true;
}

// thread = V fine cells x a run of `cc` channels: x is read once, the G products are written
template <int V>
__global__ __launch_bounds__(256) void gate_apply_fwd_kernel(const ApplyArgs a, int cc) {
    const int n = blockIdx.z;
    long long off;
    float aw[MAXG][V];
    if (!gate_cells<V>(a, n, off, aw)) return;
    const long long S = (long long)a.D * a.H * a.W;
    const int c0 = blockIdx.y * cc, c1 = min(c0 + cc, a.C);
    const float* __restrict__ xb = a.x + (long long)n * a.x_bs + off;
    float* __restrict__ yb = a.y + (long long)n * a.y_bs + off;
    for (int c = c0; c < c1; ++c) {
        float xv[V], o[V];
        Vec<V>::load(xb + c * S, xv);
#pragma unroll
        for (int g = 0; g < MAXG; ++g) {
            if (g < a.G) {
#pragma unroll
                for (int j = 0; j < V; ++j) o[j] = aw[g][j] * xv[j];
                Vec<V>::store(yb + ((long long)g * a.C + c) * S, o);
            }
        }
    }
}

// thread = V fine cells x all channels: dy and x are read once; dx (+)= sum_g a_g dy_g, and the channel sums of dy_g * x go to
// the fine-resolution scratch sc[N][G][D][H][W]
template <int V>
__global__ __launch_bounds__(256) void gate_apply_bwd_kernel(const ApplyArgs a) {
    const int n = blockIdx.z;
    long long off;
    float aw[MAXG][V];
    if (!gate_cells<V>(a, n, off, aw)) return;
    const long long S = (long long)a.D * a.H * a.W;
    const float* __restrict__ xb = a.x + (long long)n * a.x_bs + off;
    const float* __restrict__ dyb = a.dy + (long long)n * a.dy_bs + off;
    float* __restrict__ dxb = a.dx + (long long)n * a.dx_bs + off;
    float sg[MAXG][V];
#pragma unroll
    for (int g = 0; g < MAXG; ++g)
#pragma unroll
        for (int j = 0; j < V; ++j) sg[g][j] = 0.f;
    for (int c = 0; c < a.C; ++c) {
        float xv[V], dv[V];
        Vec<V>::load(xb + c * S, xv);
#pragma unroll
        for (int j = 0; j < V; ++j) dv[j] = 0.f;
#pragma unroll
        for (int g = 0; g < MAXG; ++g) {
            if (g < a.G) {
                float t[V];
                Vec<V>::load(dyb + ((long long)g * a.C + c) * S, t);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    dv[j] = fmaf(aw[g][j], t[j], dv[j]);
                    sg[g][j] = fmaf(t[j], xv[j], sg[g][j]);
                }
            }
        }
        if (a.accumulate) {
            float old[V];
            Vec<V>::load(dxb + c * S, old);
#pragma unroll
            for (int j = 0; j < V; ++j) dv[j] += old[j];
        }
        Vec<V>::store(dxb + c * S, dv);
    }
    float* __restrict__ sb = a.sc + ((long long)n * a.G) * S + off;
#pragma unroll
    for (int g = 0; g < MAXG; ++g)
        if (g < a.G) Vec<V>::store(sb + g * S, sg[g]);
}

// ------------------------------------------------------------------------------------------------ integer up-sampling
struct UpArgs {
    const float* x;
    float* y;
    long long x_bs, y_bs;
    int K, d, h, w, Do, Ho, Wo;
    float inv_s;
};

// thread = V consecutive outputs along W of one (n, k) volume; x is the small coarse tensor (cached)
template <int V>
__global__ __launch_bounds__(256) void upsample_int_fwd_kernel(const UpArgs a) {
    const int WQ = a.Wo / V;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= a.Do * a.Ho * WQ) return;
    const int k = blockIdx.y, n = blockIdx.z;
    const int xq = q % WQ, r = q / WQ;
    const int oy = r % a.Ho, oz = r / a.Ho;
    int z0, z1, y0, y1;
    float lz, ly;
    up_src(oz, a.d, a.inv_s, z0, z1, lz);
    up_src(oy, a.h, a.inv_s, y0, y1, ly);
    float o[V];
    up_values<V>(a.x + (long long)n * a.x_bs + (long long)k * (a.d * a.h * a.w), a.h, a.w, z0, z1, lz, y0, y1, ly, xq * V,
                 a.inv_s, o);
    Vec<V>::store(a.y + (long long)n * a.y_bs + (long long)k * ((long long)a.Do * a.Ho * a.Wo) +
                  ((long long)oz * a.Ho + oy) * a.Wo + xq * V, o);
}


struct UpBwdArgs {
    const float* dy;
    float* dx;
    long long dy_bs, dx_bs, cells;                 // cells = N * K * d * h * w
    int K, d, h, w, Do, Ho, Wo, ls, accumulate;    // ls = log2(2 * scale)
    float inv_s;
};

// The adjoint in gather form: one wave per coarse cell.  Cell i is read by outputs among s i - s / 2 .. s i + 3 s / 2 - 1 on each
// axis (2s candidates; the weight function is zero for the ones that do not read it, and outside the volume): the (2s)^3
// candidates are spread over the 64 lanes with x fastest (2s divides 64: a lane keeps its x), then summed by the xor tree.
__global__ __launch_bounds__(256) void upsample_int_bwd_kernel(const UpBwdArgs a) {
    const long long cell = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= a.cells) return;                 // whole waves leave: the tree below sees 64 live lanes
    const int lane = threadIdx.x & 63;
    const int T = 1 << a.ls, mask = T - 1, s = T >> 1;
    long long t = cell;
    const int ix = (int)(t % a.w); t /= a.w;
    const int iy = (int)(t % a.h); t /= a.h;
    const int iz = (int)(t % a.d); t /= a.d;
    const int k = (int)(t % a.K);
    const int n = (int)(t / a.K);
    const float* __restrict__ db = a.dy + (long long)n * a.dy_bs + (long long)k * ((long long)a.Do * a.Ho * a.Wo);
    const int bx = s * ix - (s >> 1), by = s * iy - (s >> 1), bz = s * iz - (s >> 1);
    const int ox = bx + (lane & mask);
    const float wx = up_weight(ox, ix, a.w, a.Wo, a.inv_s);
    float acc = 0.f;
    for (int r = lane >> a.ls; r < T * T; r += 64 >> a.ls) {
        const int oy = by + (r & mask), oz = bz + (r >> a.ls);
        const float wzy = up_weight(oz, iz, a.d, a.Do, a.inv_s) * up_weight(oy, iy, a.h, a.Ho, a.inv_s);
        if (wzy * wx != 0.f) acc = fmaf(wzy * wx, db[((long long)oz * a.Ho + oy) * a.Wo + ox], acc);   // zero weight: maybe outside
    }
    acc = mis_wave_sum(acc);
    if (lane == 0) {
        float* o = a.dx + (long long)n * a.dx_bs + (long long)k * (a.d * a.h * a.w) + (iz * a.h + iy) * a.w + ix;
        *o = a.accumulate ? *o + acc : acc;
    }
}

bool aligned4(const void* p, long long bs) { return !((uintptr_t)p & 15) && !(bs & 3); }

// extents > 0, fine volume below 2^31 voxels; s = coarse voxels
bool coarse_ok(int d, int h, int w, int scale, long long& s) {
    if (d <= 0 || h <= 0 || w <= 0) return false;
    s = (long long)d * h * w;
    return s * scale * scale * scale < (1LL << 31);
}

int launch_up_bwd(const float* dy, long long dy_bs, float* dx, long long dx_bs, int N, int K, int d, int h, int w, int scale,
                  int accumulate, hipStream_t stream) {
    const long long cells = (long long)N * K * d * h * w;
    if (mis_cdiv(cells, 4) > 0x7fffffffLL) return MIS_ERR_UNSUPPORTED;
    UpBwdArgs a{dy, dx, dy_bs, dx_bs, cells, K, d, h, w, scale * d, scale * h, scale * w, scale == 2 ? 2 : scale == 4 ? 3 : 4,
                accumulate, 1.f / (float)scale};
    hipLaunchKernelGGL(upsample_int_bwd_kernel, dim3((unsigned)mis_cdiv(cells, 4)), dim3(256), 0, stream, a);
    return mis_launch_status();
}

}  // namespace

extern "C" int mis_attn_gate_map_fwd(const float* theta, long long theta_bs, const float* phi, long long phi_bs,
                                     const float* psi_w, const float* psi_b, float* att, long long att_bs, int N, int G, int Ci,
                                     int d, int h, int w, hipStream_t stream) {
    long long s;
    if (!theta || !phi || !psi_w || !psi_b || !att || N <= 0 || G <= 0 || Ci <= 0 || d <= 0 || h <= 0 || w <= 0)
        return MIS_ERR_ARG;
    if (!coarse_ok(d, h, w, 2, s) || G > MAXG || N > 65535) return MIS_ERR_UNSUPPORTED;
    if (theta_bs < (long long)G * Ci * s || phi_bs < (long long)G * Ci * s || att_bs < G * s) return MIS_ERR_ARG;
    MapArgs a{theta, phi, psi_w, psi_b, att, theta_bs, phi_bs, att_bs, G, Ci, (int)s};
    hipLaunchKernelGGL(gate_map_fwd_kernel, dim3((unsigned)mis_cdiv(s, 256), G, N), dim3(256), 0, stream, a);
    return mis_launch_status();
}

extern "C" long long mis_attn_gate_map_bwd_workspace_bytes(int N, int G, int Ci, int d, int h, int w) {
    long long s;
    if (N <= 0 || G <= 0 || Ci <= 0 || d <= 0 || h <= 0 || w <= 0) return MIS_ERR_ARG;
    if (!coarse_ok(d, h, w, 2, s) || G > MAXG || N * s >= (1LL << 31) || (long long)G * Ci + G > 65535)
        return MIS_ERR_UNSUPPORTED;
    return ((long long)G * Ci + G) * mis_cdiv(N * s, MB_EPB) * 8;
}

extern "C" int mis_attn_gate_map_bwd(const float* datt, long long datt_bs, const float* att, long long att_bs,
                                     const float* theta, long long theta_bs, const float* phi, long long phi_bs,
                                     const float* psi_w, float* df, long long df_bs, float* dpsi_w, float* dpsi_b,
                                     float* dphi_b, void* workspace, long long workspace_bytes, int N, int G, int Ci, int d, int h, int w,
                                     int accumulate, hipStream_t stream) {
    if (!datt || !att || !theta || !phi || !psi_w || !df || !dpsi_w || !dpsi_b) return MIS_ERR_ARG;
    const long long need = mis_attn_gate_map_bwd_workspace_bytes(N, G, Ci, d, h, w);
    if (need < 0) return (int)need;
    const long long s = (long long)d * h * w;
    if (theta_bs < (long long)G * Ci * s || phi_bs < (long long)G * Ci * s || df_bs < (long long)G * Ci * s || att_bs < G * s ||
        datt_bs < G * s)
        return MIS_ERR_ARG;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need) return MIS_ERR_WORKSPACE;
    const int rows = G * Ci + G, nchunks = (int)mis_cdiv(N * s, MB_EPB);
    MapBwdArgs a{datt, att, theta, phi, psi_w, df, (float2*)workspace, datt_bs, att_bs, theta_bs, phi_bs, df_bs, G, Ci, (int)s,
                 (int)(N * s), nchunks};
    hipLaunchKernelGGL(gate_map_bwd_kernel, dim3(nchunks, rows), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(gate_map_bwd_final_kernel, dim3(rows), dim3(64), 0, stream, (const float2*)workspace, nchunks, G * Ci,
                       dpsi_w, dpsi_b, dphi_b, accumulate);
    return mis_launch_status();
}

static int apply_geometry(int N, int G, int C, int D, int H, int W, int d, int h, int w, long long& S) {
    long long s;
    if (N <= 0 || G <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || d <= 0 || h <= 0 || w <= 0) return MIS_ERR_ARG;
    if (D != 2 * d || H != 2 * h || W != 2 * w || !coarse_ok(d, h, w, 2, s) || G > MAXG || N > 65535 || C > 65535)
        return MIS_ERR_UNSUPPORTED;
    S = 8 * s;
    return MIS_OK;
}

extern "C" int mis_attn_gate_apply_fwd(const float* x, long long x_bs, const float* att, long long att_bs, float* y,
                                       long long y_bs, int N, int G, int C, int D, int H, int W, int d, int h, int w,
                                       hipStream_t stream) {
    long long S;
    if (!x || !att || !y) return MIS_ERR_ARG;
    const int st = apply_geometry(N, G, C, D, H, W, d, h, w, S);
    if (st != MIS_OK) return st;
    if (x_bs < C * S || y_bs < (long long)G * C * S || att_bs < G * (S / 8)) return MIS_ERR_ARG;
    ApplyArgs a{x, att, nullptr, y, nullptr, nullptr, x_bs, att_bs, y_bs, 0, 0, G, C, D, H, W, d, h, w, 0};
    // a run of 8 channels per thread: the 8 G attention taps of a thread are spread over 8 loads and 8 G stores of x / y
    const int cc = 8;
    if (W % 4 == 0 && aligned4(x, x_bs) && aligned4(y, y_bs))
        hipLaunchKernelGGL(gate_apply_fwd_kernel<4>, dim3((unsigned)mis_cdiv(S / 4, 256), (unsigned)mis_cdiv(C, cc), N),
                           dim3(256), 0, stream, a, cc);
    else
        hipLaunchKernelGGL(gate_apply_fwd_kernel<1>, dim3((unsigned)mis_cdiv(S, 256), (unsigned)mis_cdiv(C, cc), N), dim3(256),
                           0, stream, a, cc);
    return mis_launch_status();
}

extern "C" long long mis_attn_gate_apply_bwd_workspace_bytes(int N, int G, int D, int H, int W) {
    long long s;
    if (N <= 0 || G <= 0 || D <= 0 || H <= 0 || W <= 0) return MIS_ERR_ARG;
    if ((D | H | W) & 1 || !coarse_ok(D / 2, H / 2, W / 2, 2, s) || G > MAXG) return MIS_ERR_UNSUPPORTED;
    return (long long)N * G * 8 * s * 4;
}

extern "C" int mis_attn_gate_apply_bwd(const float* dy, long long dy_bs, const float* x, long long x_bs, const float* att,
                                       long long att_bs, float* dx, long long dx_bs, float* datt, long long datt_bs,
                                       void* workspace, long long workspace_bytes, int N, int G, int C, int D, int H, int W,
                                       int d, int h, int w, int accumulate, hipStream_t stream) {
    long long S;
    if (!dy || !x || !att || !dx || !datt) return MIS_ERR_ARG;
    const int st = apply_geometry(N, G, C, D, H, W, d, h, w, S);
    if (st != MIS_OK) return st;
    if (x_bs < C * S || dx_bs < C * S || dy_bs < (long long)G * C * S || att_bs < G * (S / 8) || datt_bs < G * (S / 8))
        return MIS_ERR_ARG;
    if (!workspace || workspace_bytes < (long long)N * G * S * 4) return MIS_ERR_WORKSPACE;
    ApplyArgs a{x, att, dy, nullptr, dx, (float*)workspace, x_bs, att_bs, 0, dy_bs, dx_bs, G, C, D, H, W, d, h, w, accumulate};
    if (W % 4 == 0 && aligned4(x, x_bs) && aligned4(dy, dy_bs) && aligned4(dx, dx_bs) && aligned4(workspace, 0))
        hipLaunchKernelGGL(gate_apply_bwd_kernel<4>, dim3((unsigned)mis_cdiv(S / 4, 256), 1, N), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(gate_apply_bwd_kernel<1>, dim3((unsigned)mis_cdiv(S, 256), 1, N), dim3(256), 0, stream, a);
    const int e = mis_launch_status();
    if (e != MIS_OK) return e;
    return launch_up_bwd((const float*)workspace, G * S, datt, datt_bs, N, G, d, h, w, 2, 0, stream);
}

extern "C" int mis_upsample_int_fwd(const float* x, long long x_bs, float* y, long long y_bs, int N, int K, int d, int h, int w,
                                    int scale, hipStream_t stream) {
    long long s;
    if (!x || !y || N <= 0 || K <= 0 || d <= 0 || h <= 0 || w <= 0) return MIS_ERR_ARG;
    if ((scale != 2 && scale != 4 && scale != 8) || !coarse_ok(d, h, w, scale, s) || N > 65535 || K > 65535)
        return MIS_ERR_UNSUPPORTED;
    const long long So = s * scale * scale * scale;
    if (x_bs < K * s || y_bs < K * So) return MIS_ERR_ARG;
    UpArgs a{x, y, x_bs, y_bs, K, d, h, w, scale * d, scale * h, scale * w, 1.f / (float)scale};
    if (a.Wo % 4 == 0 && aligned4(y, y_bs))
        hipLaunchKernelGGL(upsample_int_fwd_kernel<4>, dim3((unsigned)mis_cdiv(So / 4, 256), K, N), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(upsample_int_fwd_kernel<1>, dim3((unsigned)mis_cdiv(So, 256), K, N), dim3(256), 0, stream, a);
    return mis_launch_status();
}

extern "C" int mis_upsample_int_bwd(const float* dy, long long dy_bs, float* dx, long long dx_bs, int N, int K, int d, int h,
                                    int w, int scale, int accumulate, hipStream_t stream) {
    long long s;
    if (!dy || !dx || N <= 0 || K <= 0 || d <= 0 || h <= 0 || w <= 0) return MIS_ERR_ARG;
    if ((scale != 2 && scale != 4 && scale != 8) || !coarse_ok(d, h, w, scale, s)) return MIS_ERR_UNSUPPORTED;
    if (dx_bs < K * s || dy_bs < K * s * scale * scale * scale) return MIS_ERR_ARG;
    return launch_up_bwd(dy, dy_bs, dx, dx_bs, N, K, d, h, w, scale, accumulate, stream);
}
