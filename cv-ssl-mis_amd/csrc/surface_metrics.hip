// Surface-distance validation metrics on the device: everything medpy's hd95 / hd / asd / dc / ravd need of a (prediction, ground
// truth) pair of label maps, in integers (the reference's scoring functions: code/val_2D.py:7-15, code/val_3D.py:82-88,
// code/test_3D_util.py:147-152, code/test_CNNVIT.py:33-39; host restatement and oracle: utils/metrics.py; bound callers:
// val_2D.test_single_volume, val_3D.test_all_case).
//
//   surface_counts_kernel   masks A = (pred == cls), B = (gt == cls) (cls < 0: label > 0); surface = mask voxel with a face
//                           neighbour outside the mask or outside the array (binary_erosion, connectivity 1, border_value 0);
//                           |A|, |B|, |A & B|, |dA|, |dB| by block reduction + one integer atomic per count and workgroup
//   edt_row_kernel          innermost axis: distance to the nearest seed of the line (uint16; 0xFFFF = no seed in the line)
//   edt_axis_kernel         every further axis: out[i] = min_j g[j] + (i - j)^2, the line tile in LDS (exact squared EDT,
//                           separable); the last pass either writes int32 (mis_sq_edt) or bins the values at the OTHER mask's
//                           surface voxels into hist[direction][sq] with integer atomics (order-independent)
//   finalize_kernel         one workgroup, fixed order: largest occupied bin and sum count * sqrt(sq) per direction, the two
//                           order statistics of the union that numpy's 95th percentile interpolates between
//
// Every value is an integer (or, for the asd sums, a double sum in a fixed order), so the result is run-to-run identical and the
// host can reproduce medpy's numbers bit for bit from it.  No float atomics, no MFMA.
#include "common.h"

namespace {

constexpr int SM_MAX_EXTENT = 1024;
// "no seed" sentinel: three axis passes add at most (1023 + 63)^2 each (rows past the line end are computed and dropped),
// 2^28 + 3 * 1086^2 < 2^31
constexpr int SM_INF = 1 << 28;
constexpr int SM_TW = 16;            // adjacent lines per workgroup of an axis pass (one 64-byte int32 segment per line element)
constexpr int SM_ROWS = 16;          // 256 threads = SM_ROWS line positions x SM_TW lines
constexpr int SM_R = 4;              // line positions per thread: one LDS read feeds SM_R candidates
constexpr int SM_FIN_THREADS = 1024;

struct SmLayout {
    long long counts, hist, surf, g1, g2, total;   // byte offsets; counts + hist are the prefix that is cleared
    long long nbins;
};

inline long long sm_align(long long v) { return (v + 255) & ~255ll; }

inline SmLayout sm_layout(int D, int H, int W) {
    SmLayout l;
    const long long N = (long long)D * H * W;
    l.nbins = (long long)(D - 1) * (D - 1) + (long long)(H - 1) * (H - 1) + (long long)(W - 1) * (W - 1) + 1;
    l.counts = 0;
    l.hist = 256;
    l.surf = sm_align(l.hist + 2 * l.nbins * 4);
    l.g1 = sm_align(l.surf + 2 * N);
    l.g2 = sm_align(l.g1 + 2 * N * 2);
    l.total = sm_align(l.g2 + 2 * N * 4);
    return l;
}

__device__ __forceinline__ bool sm_in(unsigned char v, int cls) { return cls < 0 ? v > 0 : (int)v == cls; }

// ---- surface flags + the five counts ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void surface_counts_kernel(const unsigned char* __restrict__ pred,
                                                            const unsigned char* __restrict__ gt, int cls, int ndim, int D,
                                                            int H, int W, unsigned char* __restrict__ surf,
                                                            unsigned long long* __restrict__ counts) {
    const long long N = (long long)D * H * W, HW = (long long)H * W;
    unsigned c[5] = {0u, 0u, 0u, 0u, 0u};          // a grid-stride thread sees < 2^32 voxels
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < N; idx += (long long)gridDim.x * 256) {
        const int w = (int)(idx % W), h = (int)((idx / W) % H), d = (int)(idx / HW);
        const bool a = sm_in(pred[idx], cls), b = sm_in(gt[idx], cls);
        bool sa = false, sb = false;
        if (a || b) {
            // a face neighbour outside the array counts as outside the mask
            bool ia = true, ib = true;
            if (w > 0) { ia &= sm_in(pred[idx - 1], cls); ib &= sm_in(gt[idx - 1], cls); } else ia = ib = false;
            if (w < W - 1) { ia &= sm_in(pred[idx + 1], cls); ib &= sm_in(gt[idx + 1], cls); } else ia = ib = false;
            if (h > 0) { ia &= sm_in(pred[idx - W], cls); ib &= sm_in(gt[idx - W], cls); } else ia = ib = false;
            if (h < H - 1) { ia &= sm_in(pred[idx + W], cls); ib &= sm_in(gt[idx + W], cls); } else ia = ib = false;
            if (ndim == 3) {
                if (d > 0) { ia &= sm_in(pred[idx - HW], cls); ib &= sm_in(gt[idx - HW], cls); } else ia = ib = false;
                if (d < D - 1) { ia &= sm_in(pred[idx + HW], cls); ib &= sm_in(gt[idx + HW], cls); } else ia = ib = false;
            }
            sa = a && !ia;
            sb = b && !ib;
        }
        surf[idx] = sa;
        surf[N + idx] = sb;
        c[0] += a; c[1] += b; c[2] += a && b; c[3] += sa; c[4] += sb;
    }
    __shared__ unsigned red[4][5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o, 64);
        if (lane == 0) red[wave][k] = c[k];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const unsigned long long s = (unsigned long long)red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] +
                                     red[3][threadIdx.x];
        if (s) atomicAdd(&counts[threadIdx.x], s);
    }
}

// ---- innermost axis: one wave per line, the line's seeds as 64-bit ballots -------------------------------------------------
__global__ __launch_bounds__(256) void edt_row_kernel(const unsigned char* __restrict__ seeds, long long N,
                                                     unsigned short* __restrict__ g1, int W, long long nlines) {
    __shared__ unsigned long long masks[4][SM_MAX_EXTENT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long line = (long long)blockIdx.x * 4 + wave;
    const bool live = line < nlines;
    const int nch = (W + 63) >> 6;
    const unsigned char* src = seeds + (long long)blockIdx.y * N + (live ? line : 0) * W;
    for (int c = 0; c < nch; ++c) {
        const int x = c * 64 + lane;
        const bool s = live && x < W && src[x] != 0;
        const unsigned long long m = __ballot(s);
        if (lane == 0) masks[wave][c] = m;
    }
    __syncthreads();
    if (!live) return;
    unsigned short* dst = g1 + (long long)blockIdx.y * N + line * W;
    int prev = -1;                                   // last seed in the chunks before c
    for (int c = 0; c < nch; ++c) {
        const unsigned long long m = masks[wave][c];
        const int x = c * 64 + lane;
        int best = 0xFFFF;
        const unsigned long long lo = m & (~0ull >> (63 - lane));     // seeds at or left of the lane
        if (lo) best = lane - (63 - __clzll((long long)lo));
        else if (prev >= 0) best = x - prev;
        const unsigned long long hi = m >> lane;                      // seeds at or right of the lane
        if (hi) {
            best = min(best, __ffsll((long long)hi) - 1);
        } else {
            for (int c2 = c + 1; c2 < nch; ++c2) {                    // first seed of a later chunk
                const unsigned long long m2 = masks[wave][c2];
                if (m2) {
                    best = min(best, c2 * 64 + __ffsll((long long)m2) - 1 - x);
                    break;
                }
            }
        }
        if (x < W) dst[x] = (unsigned short)best;
        if (m) prev = c * 64 + 63 - __clzll((long long)m);
    }
}

__device__ __forceinline__ int sm_load(const unsigned short* p) {
    const int v = *p;
    return v == 0xFFFF ? SM_INF : v * v;
}
__device__ __forceinline__ int sm_load(const int* p) { return *p; }

// ---- a further axis: lines of n elements `stride` apart; a workgroup owns SM_TW adjacent lines (consecutive in memory) -----
// blockIdx.x = outer * wtiles + tile, blockIdx.y = which transform (seed set).  HIST: bin the values at the surface voxels of
// the other seed set (transform k measures the direction 1 - k: A -> B is the transform of dB read at dA) and write nothing;
// else write int32, `none_value` where the lines so far hold no seed (SM_INF between passes, INT32_MAX in mis_sq_edt's result).
template <typename TIn, bool HIST>
__global__ __launch_bounds__(256) void edt_axis_kernel(const TIn* __restrict__ gin, long long N, int n, long long stride,
                                                      long long outer_stride, int W, int* __restrict__ gout,
                                                      int none_value, const unsigned char* __restrict__ surf,
                                                      unsigned* __restrict__ hist, long long nbins) {
    extern __shared__ __attribute__((aligned(16))) int sm_line[];       // [n][SM_TW]
    const int wtiles = (W + SM_TW - 1) / SM_TW;
    const int w0 = (int)(blockIdx.x % wtiles) * SM_TW;
    const long long base = (long long)(blockIdx.x / wtiles) * outer_stride + w0;
    const int k = blockIdx.y;
    gin += (long long)k * N;
    const int wl = threadIdx.x % SM_TW, il = threadIdx.x / SM_TW;
    const bool col = w0 + wl < W;
    for (int j = il; j < n; j += SM_ROWS) sm_line[j * SM_TW + wl] = col ? sm_load(gin + base + j * stride + wl) : SM_INF;
    __syncthreads();
    if (!col) return;
    for (int i0 = il; i0 < n; i0 += SM_ROWS * SM_R) {
        bool need[SM_R];
        bool any = false;
#pragma unroll
        for (int r = 0; r < SM_R; ++r) {
            const int i = i0 + r * SM_ROWS;
            need[r] = i < n;
            if (HIST && need[r]) need[r] = surf[(long long)(1 - k) * N + base + i * stride + wl] != 0;
            any |= need[r];
        }
        if (!any) continue;
        int best[SM_R];
#pragma unroll
        for (int r = 0; r < SM_R; ++r) best[r] = 0x7FFFFFFF;
        for (int j = 0; j < n; ++j) {
            const int g = sm_line[j * SM_TW + wl];
#pragma unroll
            for (int r = 0; r < SM_R; ++r) {
                const int dlt = i0 + r * SM_ROWS - j;                  // |dlt| < 2^11: the 24-bit multiply is exact
                best[r] = min(best[r], __mul24(dlt, dlt) + g);
            }
        }
#pragma unroll
        for (int r = 0; r < SM_R; ++r) {
            if (!need[r]) continue;
            const long long idx = base + (long long)(i0 + r * SM_ROWS) * stride + wl;
            if (HIST) {
                if (best[r] < SM_INF && best[r] < nbins) atomicAdd(&hist[(long long)(1 - k) * nbins + best[r]], 1u);
            } else {
                gout[(long long)k * N + idx] = best[r] < SM_INF ? best[r] : none_value;
            }
        }
    }
}

// ---- one workgroup over the two histograms, fixed order --------------------------------------------------------------------
// thread t owns the bins [t * chunk, (t + 1) * chunk); thread 0 combines the 1024 partials in ascending order
__global__ __launch_bounds__(SM_FIN_THREADS) void finalize_kernel(const unsigned long long* __restrict__ counts,
                                                                 const unsigned* __restrict__ hist, long long nbins,
                                                                 long long* __restrict__ out) {
    __shared__ double s_sum[2][SM_FIN_THREADS];
    __shared__ long long s_max[2][SM_FIN_THREADS];
    __shared__ unsigned long long s_cnt[SM_FIN_THREADS];
    const int t = threadIdx.x;
    const long long chunk = (nbins + SM_FIN_THREADS - 1) / SM_FIN_THREADS;
    const long long b0 = min((long long)t * chunk, nbins), b1 = min(b0 + chunk, nbins);
    const bool valid = counts[0] > 0 && counts[1] > 0;
    unsigned long long cnt = 0;
    for (int dir = 0; dir < 2; ++dir) {
        double sum = 0.0;
        long long mx = -1;
        if (valid) {
            for (long long b = b0; b < b1; ++b) {
                const unsigned c = hist[dir * nbins + b];
                if (c) {
                    sum += (double)c * sqrt((double)b);
                    mx = b;
                    cnt += c;
                }
            }
        }
        s_sum[dir][t] = sum;
        s_max[dir][t] = mx;
    }
    s_cnt[t] = cnt;
    __syncthreads();
    if (t != 0) return;
    for (int k = 0; k < 5; ++k) out[k] = (long long)counts[k];
    long long sq[2] = {-1, -1};
    for (int dir = 0; dir < 2; ++dir) {
        double sum = 0.0;
        long long mx = -1;
        for (int u = 0; u < SM_FIN_THREADS; ++u) {
            sum += s_sum[dir][u];
            if (s_max[dir][u] >= 0) mx = s_max[dir][u];
        }
        out[5 + dir] = mx;
        out[7 + dir] = __double_as_longlong(sum);
    }
    if (valid) {
        // numpy's linear percentile: virtual index (n - 1) * 0.95 as ONE float64 product, floor, next index clipped
        const long long n = (long long)(counts[3] + counts[4]);
        const long long lo = (long long)floor((double)(n - 1) * 0.95);
        const long long pos[2] = {lo, min(lo + 1, n - 1)};
        for (int q = 0; q < 2; ++q) {
            unsigned long long before = 0;
            for (int u = 0; u < SM_FIN_THREADS && sq[q] < 0; ++u) {
                if (before + s_cnt[u] > (unsigned long long)pos[q]) {
                    const long long c0 = min((long long)u * chunk, nbins), c1 = min(c0 + chunk, nbins);
                    for (long long b = c0; b < c1; ++b) {
                        before += (unsigned long long)hist[b] + hist[nbins + b];
                        if (before > (unsigned long long)pos[q]) {
                            sq[q] = b;
                            break;
                        }
                    }
                    break;
                }
                before += s_cnt[u];
            }
        }
    }
    out[9] = sq[0];
    out[10] = sq[1];
    out[11] = valid ? 1 : 0;
}

int sm_check_shape(int ndim, int D, int H, int W) {
    if (D <= 0 || H <= 0 || W <= 0) return MIS_ERR_ARG;
    if (ndim != 2 && ndim != 3) return MIS_ERR_UNSUPPORTED;
    if (ndim == 2 && D != 1) return MIS_ERR_ARG;
    if (D > SM_MAX_EXTENT || H > SM_MAX_EXTENT || W > SM_MAX_EXTENT) return MIS_ERR_UNSUPPORTED;
    return MIS_OK;
}

// row pass + H pass of `nsets` seed sets ([nsets][N] uint8) -> g2 ([nsets][N] int32: squared distance within the d-plane)
int sm_plane_passes(const unsigned char* seeds, int nsets, int D, int H, int W, unsigned short* g1, int* g2,
                    hipStream_t stream) {
    const long long N = (long long)D * H * W, nlines = (long long)D * H;
    hipLaunchKernelGGL(edt_row_kernel, dim3((unsigned)mis_cdiv(nlines, 4), nsets), dim3(256), 0, stream, seeds, N, g1, W,
                       nlines);
    const int wtiles = (W + SM_TW - 1) / SM_TW;
    hipLaunchKernelGGL((edt_axis_kernel<unsigned short, false>), dim3((unsigned)(D * wtiles), nsets), dim3(256),
                       (size_t)H * SM_TW * sizeof(int), stream, (const unsigned short*)g1, N, H, (long long)W,
                       (long long)H * W, W, g2, SM_INF, (const unsigned char*)nullptr, (unsigned*)nullptr, 0ll);
    return mis_launch_status();
}

}  // namespace

extern "C" long long mis_surface_metrics_workspace_bytes(int D, int H, int W) {
    if (D <= 0 || H <= 0 || W <= 0) return MIS_ERR_ARG;
    if (D > SM_MAX_EXTENT || H > SM_MAX_EXTENT || W > SM_MAX_EXTENT) return MIS_ERR_UNSUPPORTED;
    return sm_layout(D, H, W).total;
}

extern "C" int mis_surface_metrics(const unsigned char* pred, const unsigned char* gt, int cls, int ndim, int D, int H, int W,
                                   void* out, void* workspace, long long workspace_bytes, hipStream_t stream) {
    if (!pred || !gt || !out || !workspace || cls < -1 || cls > 255) return MIS_ERR_ARG;
    const int st = sm_check_shape(ndim, D, H, W);
    if (st != MIS_OK) return st;
    const SmLayout l = sm_layout(D, H, W);
    if (workspace_bytes < l.total) return MIS_ERR_WORKSPACE;
    char* ws = (char*)workspace;
    unsigned long long* counts = (unsigned long long*)(ws + l.counts);
    unsigned* hist = (unsigned*)(ws + l.hist);
    unsigned char* surf = (unsigned char*)(ws + l.surf);
    unsigned short* g1 = (unsigned short*)(ws + l.g1);
    int* g2 = (int*)(ws + l.g2);
    const long long N = (long long)D * H * W;
    if (hipMemsetAsync(ws, 0, (size_t)(l.hist + 2 * l.nbins * 4), stream) != hipSuccess) return MIS_ERR_LAUNCH;
    const unsigned grid = (unsigned)min(mis_cdiv(N, 256), 256ll * 16);
    hipLaunchKernelGGL(surface_counts_kernel, dim3(grid), dim3(256), 0, stream, pred, gt, cls, ndim, D, H, W, surf, counts);
    if (sm_plane_passes(surf, 2, D, H, W, g1, g2, stream) != MIS_OK) return MIS_ERR_LAUNCH;
    const int wtiles = (W + SM_TW - 1) / SM_TW;
    hipLaunchKernelGGL((edt_axis_kernel<int, true>), dim3((unsigned)(H * wtiles), 2), dim3(256), (size_t)D * SM_TW * sizeof(int),
                       stream, (const int*)g2, N, D, (long long)H * W, (long long)W, W, (int*)nullptr,
                       SM_INF, (const unsigned char*)surf, hist, l.nbins);
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(SM_FIN_THREADS), 0, stream, (const unsigned long long*)counts,
                       (const unsigned*)hist, l.nbins, (long long*)out);
    return mis_launch_status();
}

extern "C" int mis_sq_edt(const unsigned char* seeds, int ndim, int D, int H, int W, int* out, void* workspace,
                          long long workspace_bytes, hipStream_t stream) {
    if (!seeds || !out || !workspace) return MIS_ERR_ARG;
    const int st = sm_check_shape(ndim, D, H, W);
    if (st != MIS_OK) return st;
    const SmLayout l = sm_layout(D, H, W);
    if (workspace_bytes < l.total) return MIS_ERR_WORKSPACE;
    char* ws = (char*)workspace;
    unsigned short* g1 = (unsigned short*)(ws + l.g1);
    int* g2 = (int*)(ws + l.g2);
    const long long N = (long long)D * H * W;
    if (sm_plane_passes(seeds, 1, D, H, W, g1, g2, stream) != MIS_OK) return MIS_ERR_LAUNCH;
    const int wtiles = (W + SM_TW - 1) / SM_TW;
    hipLaunchKernelGGL((edt_axis_kernel<int, false>), dim3((unsigned)(H * wtiles), 1), dim3(256), (size_t)D * SM_TW * sizeof(int),
                       stream, (const int*)g2, N, D, (long long)H * W, (long long)W, W, out, 0x7FFFFFFF,
                       (const unsigned char*)nullptr, (unsigned*)nullptr, 0ll);
    return mis_launch_status();
}
