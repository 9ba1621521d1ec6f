// Window-attention kernels for ONE window size, compiled once per size by attention.hip
// (#define MIS_ATTN_WS / MIS_ATTN_NS, then #include): the window size fixes register layouts, LDS sizes and loop
// trip counts, so it is a compile-time constant.  See attention.hip for the design notes.
namespace MIS_ATTN_NS {

constexpr int WS = MIS_ATTN_WS, NTOK = WS * WS, HD = 32;
constexpr int NBIAS = (2 * WS - 1) * (2 * WS - 1);      // relative-position-bias table rows: 169 (window 7), 225 (8)
constexpr int NBPAD = (NBIAS + 15) / 16 * 16;
static_assert(NTOK <= 64, "one wave covers a window: at most 64 tokens");

struct AttnArgs {
    const float* qkv; long long ldq;      // [B*H*W][3*C] natural token order
    float* out; long long ldo;            // [B*H*W][C]
    const float* table;                   // relative_position_bias_table [169][nH]
    int B, H, W, nH, shift;
    float scale;
};

// region id of the reference's img_mask slices (0,-ws), (-ws,-shift), (-shift,None)  (:219-224)
__device__ __forceinline__ int region(int s, int n, int shift) { return s < n - WS ? 0 : (s < n - shift ? 1 : 2); }

// unit decode shared by forward and backward
struct Unit {
    int b, wy, wx, h, tok, iy, ix, rid;
    bool active;
};

__device__ __forceinline__ Unit decode(long long u, int lane, int B, int H, int W, int nH, int shift) {
    Unit r;
    const int nWx = W / WS, nWy = H / WS;
    r.h = (int)(u % nH); u /= nH;
    r.wx = (int)(u % nWx); u /= nWx;
    r.wy = (int)(u % nWy);
    r.b = (int)(u / nWy);
    r.active = lane < NTOK;
    const int i = r.active ? lane : 0;
    r.iy = i / WS; r.ix = i - r.iy * WS;
    const int sy = r.wy * WS + r.iy, sx = r.wx * WS + r.ix;     // coordinates in the shifted image
    r.rid = shift > 0 ? region(sy, H, shift) * 3 + region(sx, W, shift) : 0;
    const int y = (sy + shift) % H, x = (sx + shift) % W;       // natural coordinates
    r.tok = (r.b * H + y) * W + x;
    return r;
}

// 4 waves per workgroup, one unit each.  LDS per wave: K[49][32], V[49][32], bias[169], rid[49]
constexpr int LDS_PER_WAVE = 2 * NTOK * HD + NBPAD + 64;

__global__ __launch_bounds__(256) void attn_fwd_kernel(const AttnArgs a, long long units) {
    __shared__ __attribute__((aligned(16))) float smem[4 * LDS_PER_WAVE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long u = blockIdx.x * 4LL + wave;
    if (u >= units) return;
    float* sk = smem + wave * LDS_PER_WAVE;
    float* sv = sk + NTOK * HD;
    float* sb = sv + NTOK * HD;
    int* srid = reinterpret_cast<int*>(sb + NBPAD);
    const Unit t = decode(u, lane, a.B, a.H, a.W, a.nH, a.shift);
    const int C = a.nH * HD;
    const float* __restrict__ row = a.qkv + (long long)t.tok * a.ldq + t.h * HD;
    float q[HD];
    if (t.active) {
#pragma unroll
        for (int e = 0; e < HD; e += 4) {
            const float4 vq = *reinterpret_cast<const float4*>(row + e);
            q[e] = vq.x * a.scale; q[e + 1] = vq.y * a.scale; q[e + 2] = vq.z * a.scale; q[e + 3] = vq.w * a.scale;
            *reinterpret_cast<float4*>(sk + lane * HD + e) = *reinterpret_cast<const float4*>(row + C + e);
            *reinterpret_cast<float4*>(sv + lane * HD + e) = *reinterpret_cast<const float4*>(row + 2 * C + e);
        }
        srid[lane] = t.rid;
    }
    for (int i = lane; i < NBIAS; i += 64) sb[i] = a.table[i * a.nH + t.h];
    __builtin_amdgcn_s_waitcnt(0);   // LDS writes of this wave complete (single wave: no barrier needed)
    __builtin_amdgcn_wave_barrier();
    if (!t.active) return;

    float s[NTOK];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < NTOK; ++j) {
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < HD; e += 4) {
            const float4 kk = *reinterpret_cast<const float4*>(sk + j * HD + e);
            acc += (q[e] * kk.x + q[e + 1] * kk.y) + (q[e + 2] * kk.z + q[e + 3] * kk.w);
        }
        const int jy = j / WS, jx = j - jy * WS;
        acc += sb[(t.iy - jy + WS - 1) * (2 * WS - 1) + (t.ix - jx + WS - 1)];
        if (a.shift > 0 && srid[j] != t.rid) acc += -100.f;
        s[j] = acc;
        mx = fmaxf(mx, acc);
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NTOK; ++j) { s[j] = expf(s[j] - mx); sum += s[j]; }
    const float inv = 1.f / sum;
    float o[HD];
#pragma unroll
    for (int e = 0; e < HD; ++e) o[e] = 0.f;
#pragma unroll
    for (int j = 0; j < NTOK; ++j) {
        const float p = s[j] * inv;
#pragma unroll
        for (int e = 0; e < HD; e += 4) {
            const float4 vv = *reinterpret_cast<const float4*>(sv + j * HD + e);
            o[e] += p * vv.x; o[e + 1] += p * vv.y; o[e + 2] += p * vv.z; o[e + 3] += p * vv.w;
        }
    }
    float* __restrict__ orow = a.out + (long long)t.tok * a.ldo + t.h * HD;
#pragma unroll
    for (int e = 0; e < HD; e += 4) *reinterpret_cast<float4*>(orow + e) = make_float4(o[e], o[e + 1], o[e + 2], o[e + 3]);
}

// ---------------------------------------------------------------------------------------------------
// MFMA form (v_mfma_f32_16x16x4_f32, exact fp32): the 49-token window is padded to 64 = 4 tiles of 16.
// One wave per (sample, window, head), NO LDS for the operands: every operand is loaded from global memory
// straight into the register layout the matrix instruction wants --
//   "L1" rows-on-lanes   X1[t][s]     = X[16t + lane%16][8*(lane/16) + s]        (two float4 loads per tile)
//        A or B operand of a product that contracts over the 32 head dims: step s of lane group g supplies
//        dim 8g+s (the contraction index may be permuted freely as long as A and B agree);
//   "L2" rows-on-groups  X2[t][i][nt] = X[16t + 4*(lane/16) + i][16nt + lane%16]  (64-byte row segments)
//        B operand of a product that contracts over tokens, matching the accumulator layout
//        D[4*(lane/16) + i][lane%16] of the previous product used as its A operand (A = D^T).
// Forward: S^T = K Q^T (keys on accumulator rows) -> + bias/mask, softmax over the accumulator rows (in-lane over
// 16 values, then two cross-group shuffles) -> O = P V with A = (S^T)^T straight from the accumulators.
// ---------------------------------------------------------------------------------------------------
struct WinGeo {
    int b, wy, wx, h;
};

__device__ __forceinline__ WinGeo decode_window(long long u, int H, int W, int nH) {
    WinGeo r;
    const int nWx = W / WS, nWy = H / WS;
    r.h = (int)(u % nH); u /= nH;
    r.wx = (int)(u % nWx); u /= nWx;
    r.wy = (int)(u % nWy);
    r.b = (int)(u / nWy);
    return r;
}

// Per-wave LDS row table (64 entries, rows >= 49 alias row 0 and are masked by the callers):
//   srow[r]  = natural token offset of window row r inside its image ((y*W + x), cyclic shift folded in)
//   smeta[r] = (iy*13 + ix) | mask-region id << 8   (relative-position index arithmetic / shift mask :216-238)
__device__ __forceinline__ void fill_row_table(int wy, int wx, int lane, int H, int W, int shift, int* srow, int* smeta) {
    const int r = lane < NTOK ? lane : 0;
    const int iy = r / WS, ix = r - iy * WS;
    const int sy = wy * WS + iy, sx = wx * WS + ix;
    const int rid = shift > 0 ? region(sy, H, shift) * 3 + region(sx, W, shift) : 0;
    srow[lane] = ((sy + shift) % H) * W + (sx + shift) % W;
    smeta[lane] = (iy * (2 * WS - 1) + ix) | (rid << 8);
}

// L1 load: rows 16t + lane%16 (zero for rows >= 49), dims 8*(lane/16) .. +7, optionally scaled.
// Element offsets are 32-bit (the host checks that the buffers are < 2^31 bytes).
__device__ __forceinline__ void load_l1(const float* __restrict__ base, int tb, const int* srow, int ld, int col0,
                                        int lane, float scale, float (*dst)[8]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        const int r = 16 * t + (lane & 15);
        if (r < NTOK) {
            const float* p = base + ((tb + srow[r]) * ld + col0 + 8 * (lane >> 4));
            a = *reinterpret_cast<const float4*>(p);
            b = *reinterpret_cast<const float4*>(p + 4);
        }
        dst[t][0] = a.x * scale; dst[t][1] = a.y * scale; dst[t][2] = a.z * scale; dst[t][3] = a.w * scale;
        dst[t][4] = b.x * scale; dst[t][5] = b.y * scale; dst[t][6] = b.z * scale; dst[t][7] = b.w * scale;
    }
}

// L2 load: rows 16t + 4*(lane/16) + i (zero for rows >= 49), dims 16nt + lane%16
__device__ __forceinline__ void load_l2(const float* __restrict__ base, int tb, const int* srow, int ld, int col0,
                                        int lane, float scale, float (*dst)[4][2]) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // column tile nt of lane lj is head dimension 2 lj + nt (any assignment of the 32 dimensions to (lj, nt) gives the same
            // products; the stores use the same one): one 8-byte access per lane, 128 contiguous bytes per row and instruction
            const int r = 16 * t + 4 * (lane >> 4) + i;
            const int e = (tb + srow[r]) * ld + col0 + 2 * (lane & 15);
            const float2 v = r < NTOK ? *reinterpret_cast<const float2*>(base + e) : make_float2(0.f, 0.f);
            dst[t][i][0] = v.x * scale;
            dst[t][i][1] = v.y * scale;
        }
}

// store an accumulator tile set D[t][nt] (rows 16t + 4*(lane/16) + i, dims 16nt + lane%16) to token rows
__device__ __forceinline__ void store_l2(float* __restrict__ base, int tb, const int* srow, int ld, int col0, int lane,
                                         float scale, const f32x4 (*acc)[2]) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 16 * t + 4 * (lane >> 4) + i;
            if (r < NTOK) {
                const int e = (tb + srow[r]) * ld + col0 + 2 * (lane & 15);
                *reinterpret_cast<float2*>(base + e) = make_float2(acc[t][0][i] * scale, acc[t][1][i] * scale);
            }
        }
}

// reductions over the 16 lanes of a DPP row (all lanes end up with the result): quad swaps, then the two mirrors --
// vector-pipe data movement instead of ds_bpermute round trips through the LDS crossbar
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<0xB1>(v);     // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);     // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);    // row_half_mirror
    v += dpp_mov<0x140>(v);    // row_mirror
    return v;
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    v = fmaxf(v, dpp_mov<0x141>(v));
    v = fmaxf(v, dpp_mov<0x140>(v));
    return v;
}

constexpr int BIAS_OFF = (WS - 1) * (2 * WS - 1) + (WS - 1);     // 84

// 4 waves per workgroup, one unit each; LDS per wave: the head's 169 biases + the row table.
// PREC = 1: the same products as bf16x3 split products (common.h): the L1 layout IS the v_mfma_f32_16x16x32_bf16 operand of a
// product over the 32 head dims (8 dims per lane), and for a product over tokens the 8 elements of a lane are the two
// accumulator tiles (t = 2T, 2T + 1) x 4 rows of a 32-token block -- the same tokens for the A (accumulators) and B (L2) side.
// three waves per SIMD (<= 170 registers; the allocator's own choice is 144 + 64 accumulation registers = two): a unit is one
// load -> products -> softmax -> products -> store chain, and what hides its latencies is the other resident waves
// (scripts/attn_bench.py: 64.8 -> 59.1 us at 9216 units, 38.7 -> 35.3 at 4608)
template <int PREC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void attn_fwd_mfma_kernel(const AttnArgs a, long long units) {
    __shared__ float sbias[4][NBPAD];
    __shared__ int stab[4][128];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lj = lane & 15, g = lane >> 4;
    const long long u = blockIdx.x * 4LL + wave;
    if (u >= units) return;
    const WinGeo w = decode_window(u, a.H, a.W, a.nH);
    float* sb = sbias[wave];
    int* srow = stab[wave];
    int* smeta = srow + 64;
    for (int i = lane; i < NBIAS; i += 64) sb[i] = a.table[i * a.nH + w.h];
    fill_row_table(w.wy, w.wx, lane, a.H, a.W, a.shift, srow, smeta);
    __builtin_amdgcn_wave_barrier();
    const int C = a.nH * HD, col = w.h * HD, ldq = (int)a.ldq;
    const int tb = w.b * a.H * a.W;
    // S^T[key = 16mt + 4g + i][query = 16qt + lj]
    f32x4 st[4][4];
    {
        float q1[4][8], k1[4][8];
        load_l1(a.qkv, tb, srow, ldq, col, lane, a.scale, q1);
        load_l1(a.qkv, tb, srow, ldq, C + col, lane, 1.f, k1);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int qt = 0; qt < 4; ++qt) st[mt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (PREC == 1) {
            MisBf3 kb[4], qb[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                kb[t] = mis_bf3_from8(k1[t][0], k1[t][1], k1[t][2], k1[t][3], k1[t][4], k1[t][5], k1[t][6], k1[t][7]);
                qb[t] = mis_bf3_from8(q1[t][0], q1[t][1], q1[t][2], q1[t][3], q1[t][4], q1[t][5], q1[t][6], q1[t][7]);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int qt = 0; qt < 4; ++qt) st[mt][qt] = mis_bf3_dot(kb[mt], qb[qt], st[mt][qt]);
        } else {
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int qt = 0; qt < 4; ++qt)
                        st[mt][qt] = __builtin_amdgcn_mfma_f32_16x16x4f32(k1[mt][s], q1[qt][s], st[mt][qt], 0, 0, 0);
        }
    }
    float v2[4][4][2];
    load_l2(a.qkv, tb, srow, ldq, 2 * C + col, lane, 1.f, v2);     // in flight during the softmax
    int mk[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) mk[e] = smeta[16 * (e >> 2) + 4 * g + (e & 3)];
    // bias + mask, softmax over keys (accumulator rows) per query column
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
        const int mq = smeta[16 * qt + lj];
        float mx = -INFINITY;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = -INFINITY;
                if (16 * mt + 4 * g + i < NTOK) {
                    v = st[mt][qt][i] + sb[(mq & 255) - (mk[4 * mt + i] & 255) + BIAS_OFF];
                    if (a.shift > 0 && (mk[4 * mt + i] >> 8) != (mq >> 8)) v += -100.f;
                }
                st[mt][qt][i] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float e = expf(st[mt][qt][i] - mx);
                st[mt][qt][i] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.f / sum;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) st[mt][qt][i] *= inv;
    }
    // O[query = 16qt + 4g + i'][dim = 16nt + lj] = sum_key P[query][key] V[key][dim]
    f32x4 o[4][2];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) o[qt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (PREC == 1) {
#pragma unroll
        for (int T = 0; T < 2; ++T) {
            MisBf3 vb[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
                vb[nt] = mis_bf3_from8(v2[2 * T][0][nt], v2[2 * T][1][nt], v2[2 * T][2][nt], v2[2 * T][3][nt],
                                       v2[2 * T + 1][0][nt], v2[2 * T + 1][1][nt], v2[2 * T + 1][2][nt], v2[2 * T + 1][3][nt]);
#pragma unroll
            for (int qt = 0; qt < 4; ++qt) {
                const MisBf3 pb = mis_bf3_from8(st[2 * T][qt][0], st[2 * T][qt][1], st[2 * T][qt][2], st[2 * T][qt][3],
                                                st[2 * T + 1][qt][0], st[2 * T + 1][qt][1], st[2 * T + 1][qt][2], st[2 * T + 1][qt][3]);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) o[qt][nt] = mis_bf3_dot(pb, vb[nt], o[qt][nt]);
            }
        }
    } else {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int qt = 0; qt < 4; ++qt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        o[qt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(st[mt][qt][i], v2[mt][i][nt], o[qt][nt], 0, 0, 0);
    }
    store_l2(a.out, tb, srow, (int)a.ldo, col, lane, 1.f, o);
}

struct AttnBwdArgs {
    const float* qkv; long long ldq;
    const float* dout; long long ldo;     // gradient of the attention output [B*H*W][C]
    float* dqkv; long long lddq;          // [B*H*W][3*C]
    const float* table;
    float* dS_part;                       // [chunks][nWy*nWx][nH][49*49] partial sums of dS over a batch chunk
    int B, H, W, nH, shift, chunk;        // chunk = samples per workgroup
    float scale;
};

// one wave per (batch chunk, window, head): loops over the samples of the chunk, accumulating dS for
// the relative-position-bias gradient.  LDS per wave: K,V,dO [49][32] each + one [49][49] matrix; the scaled Q rows
// (needed row-wise only by the last phase) are written over V once V is dead: 29 KiB -> 5 waves per CU instead of 4.
constexpr int BWD_LDS = 3 * NTOK * HD + NTOK * NTOK + NBPAD + 64;

__global__ __launch_bounds__(64) void attn_bwd_kernel(const AttnBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[BWD_LDS];
    const int lane = threadIdx.x;
    float* sk = smem;
    float* sv = sk + NTOK * HD;
    float* sq = sv;                       // aliases V: filled after phase 1b (V's last use)
    float* sdo = sv + NTOK * HD;
    float* sm = sdo + NTOK * HD;          // [49][49]: first P, then dS
    float* sb = sm + NTOK * NTOK;
    int* srid = reinterpret_cast<int*>(sb + NBPAD);
    const int nWx = a.W / WS, nWy = a.H / WS;
    int u = blockIdx.x;
    const int h = u % a.nH; u /= a.nH;
    const int w = u % (nWx * nWy);
    const int ck = u / (nWx * nWy);
    const int C = a.nH * HD;
    for (int i = lane; i < NBIAS; i += 64) sb[i] = a.table[i * a.nH + h];
    float dsacc[NTOK];
#pragma unroll
    for (int j = 0; j < NTOK; ++j) dsacc[j] = 0.f;

    const int b0 = ck * a.chunk;
    const int b1 = b0 + a.chunk < a.B ? b0 + a.chunk : a.B;
    for (int b = b0; b < b1; ++b) {
        const long long unit = ((long long)b * nWy * nWx + w) * a.nH + h;
        const Unit t = decode(unit, lane, a.B, a.H, a.W, a.nH, a.shift);
        __builtin_amdgcn_wave_barrier();
        const float* __restrict__ row = a.qkv + (long long)t.tok * a.ldq + h * HD;
        const float* __restrict__ drow = a.dout + (long long)t.tok * a.ldo + h * HD;
        float q[HD], dOi[HD];
        if (t.active) {
#pragma unroll
            for (int e = 0; e < HD; e += 4) {
                const float4 vq = *reinterpret_cast<const float4*>(row + e);
                q[e] = vq.x * a.scale; q[e + 1] = vq.y * a.scale; q[e + 2] = vq.z * a.scale; q[e + 3] = vq.w * a.scale;
                *reinterpret_cast<float4*>(sk + lane * HD + e) = *reinterpret_cast<const float4*>(row + C + e);
                *reinterpret_cast<float4*>(sv + lane * HD + e) = *reinterpret_cast<const float4*>(row + 2 * C + e);
                const float4 vd = *reinterpret_cast<const float4*>(drow + e);
                dOi[e] = vd.x; dOi[e + 1] = vd.y; dOi[e + 2] = vd.z; dOi[e + 3] = vd.w;
                *reinterpret_cast<float4*>(sdo + lane * HD + e) = vd;
            }
            srid[lane] = t.rid;
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();

        // ---- phase 1 (lane = query row i): P row, dP row, dS row, dq ----
        float p[NTOK];
        if (t.active) {
            float mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < NTOK; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int e = 0; e < HD; e += 4) {
                    const float4 kk = *reinterpret_cast<const float4*>(sk + j * HD + e);
                    acc += (q[e] * kk.x + q[e + 1] * kk.y) + (q[e + 2] * kk.z + q[e + 3] * kk.w);
                }
                const int jy = j / WS, jx = j - jy * WS;
                acc += sb[(t.iy - jy + WS - 1) * (2 * WS - 1) + (t.ix - jx + WS - 1)];
                if (a.shift > 0 && srid[j] != t.rid) acc += -100.f;
                p[j] = acc;
                mx = fmaxf(mx, acc);
            }
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < NTOK; ++j) { p[j] = expf(p[j] - mx); sum += p[j]; }
            const float inv = 1.f / sum;
#pragma unroll
            for (int j = 0; j < NTOK; ++j) { p[j] *= inv; sm[lane * NTOK + j] = p[j]; }
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        // ---- phase 2a (lane = key row j): dV_j = sum_i P[i][j] dO_i ----
        float* __restrict__ dqrow = a.dqkv + (long long)t.tok * a.lddq + h * HD;
        if (t.active) {
            float dv[HD];
#pragma unroll
            for (int e = 0; e < HD; ++e) dv[e] = 0.f;
            for (int i = 0; i < NTOK; ++i) {
                const float pij = sm[i * NTOK + lane];
#pragma unroll
                for (int e = 0; e < HD; e += 4) {
                    const float4 d = *reinterpret_cast<const float4*>(sdo + i * HD + e);
                    dv[e] += pij * d.x; dv[e + 1] += pij * d.y; dv[e + 2] += pij * d.z; dv[e + 3] += pij * d.w;
                }
            }
#pragma unroll
            for (int e = 0; e < HD; e += 4)
                *reinterpret_cast<float4*>(dqrow + 2 * C + e) = make_float4(dv[e], dv[e + 1], dv[e + 2], dv[e + 3]);
        }
        __builtin_amdgcn_wave_barrier();
        // ---- phase 1b: dS row (overwrites P in LDS), dq ----
        if (t.active) {
            float dot = 0.f;
            float dp[NTOK];
#pragma unroll
            for (int j = 0; j < NTOK; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int e = 0; e < HD; e += 4) {
                    const float4 vv = *reinterpret_cast<const float4*>(sv + j * HD + e);
                    acc += (dOi[e] * vv.x + dOi[e + 1] * vv.y) + (dOi[e + 2] * vv.z + dOi[e + 3] * vv.w);
                }
                dp[j] = acc;
                dot += acc * p[j];
            }
            float dq[HD];
#pragma unroll
            for (int e = 0; e < HD; ++e) dq[e] = 0.f;
#pragma unroll
            for (int j = 0; j < NTOK; ++j) {
                const float ds = p[j] * (dp[j] - dot);
                sm[lane * NTOK + j] = ds;
                dsacc[j] += ds;
#pragma unroll
                for (int e = 0; e < HD; e += 4) {
                    const float4 kk = *reinterpret_cast<const float4*>(sk + j * HD + e);
                    dq[e] += ds * kk.x; dq[e + 1] += ds * kk.y; dq[e + 2] += ds * kk.z; dq[e + 3] += ds * kk.w;
                }
            }
#pragma unroll
            for (int e = 0; e < HD; e += 4)
                *reinterpret_cast<float4*>(dqrow + e) = make_float4(dq[e] * a.scale, dq[e + 1] * a.scale,
                                                                   dq[e + 2] * a.scale, dq[e + 3] * a.scale);
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();       // every lane is done reading V
        if (t.active) {
#pragma unroll
            for (int e = 0; e < HD; e += 4)
                *reinterpret_cast<float4*>(sq + lane * HD + e) = make_float4(q[e], q[e + 1], q[e + 2], q[e + 3]);
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        // ---- phase 2b (lane = key row j): dK_j = sum_i dS[i][j] * (scale*q_i) ----
        if (t.active) {
            float dk[HD];
#pragma unroll
            for (int e = 0; e < HD; ++e) dk[e] = 0.f;
            for (int i = 0; i < NTOK; ++i) {
                const float ds = sm[i * NTOK + lane];
#pragma unroll
                for (int e = 0; e < HD; e += 4) {
                    const float4 qq = *reinterpret_cast<const float4*>(sq + i * HD + e);
                    dk[e] += ds * qq.x; dk[e + 1] += ds * qq.y; dk[e + 2] += ds * qq.z; dk[e + 3] += ds * qq.w;
                }
            }
#pragma unroll
            for (int e = 0; e < HD; e += 4)
                *reinterpret_cast<float4*>(dqrow + C + e) = make_float4(dk[e], dk[e + 1], dk[e + 2], dk[e + 3]);
        }
    }
    // partial of dS summed over this chunk's samples: [ck][w][h][i][j]
    if (lane < NTOK) {
        float* __restrict__ o = a.dS_part + (((long long)ck * nWy * nWx + w) * a.nH + h) * (NTOK * NTOK) + lane * NTOK;
#pragma unroll
        for (int j = 0; j < NTOK; ++j) o[j] = dsacc[j];
    }
}

// MFMA backward (layouts: see attn_fwd_mfma_kernel).  Queries sit on the accumulator rows here:
//   S = Q K^T, dP = dO V^T                    (contract over head dims, L1 operands)
//   P = softmax(S + bias + mask), dS = P o (dP - rowsum(P o dP))   (row reductions = 16-lane shuffles)
//   dV = P^T dO, dK = dS^T (scale Q)          (contract over queries: A = accumulators transposed, B = L2 operands)
//   dQ = scale * dS K                         (contracts over keys = the accumulators' lane axis: dS goes through a
//                                              [64][68] LDS tile once and comes back as a rows-on-lanes A operand)
// One wave per (sample, window, head) (the host passes chunk == 1): dS also goes out as this unit's partial of the
// bias-table gradient.  Summing dS over several samples in accumulators (first version) cost 64 registers and with
// them the second wave per SIMD; per-unit partials + the coalesced attn_ds_reduce_kernel are faster (stage-1
// backward 300 -> 262 us) although they move 88 MB more.
constexpr int DS_LD = 68;

// Relative-position-bias gradient of ONE unit inside the backward kernel (round 6): dtable[dy][dx] = sum of dS[i][j] over the
// (query i, key j) pairs with iy - jy = dy, ix - jx = dx (reference ...sys.py:99-102, :131 through autograd's index_add).  dS sits
// in the wave's LDS tile for the dQ product anyway, and the index is separable:
//   stage 1   R[iy][jy][dx] = sum_jx dS[(iy, jx + dx)][(jy, jx)]     lane = (iy, jy): WS^2 lanes, 2 WS - 1 sums of <= WS terms with
//                                                                    compile-time bounds and immediate LDS offsets (WS^2 reads)
//   stage 2   dtable[dy][dx] = sum_jy R[jy + dy][jy][dx]             lane = table entries lane, lane + 64, ...: <= WS terms each
// (a first version dealt whole table entries to lanes: run-time loop bounds, dependent LDS reads, +10 us per launch).  Stage 1
// accumulates over the samples of a wave's chunk in registers; stage 2 runs once, through the then dead dS tile.  The unit
// writes NBIAS floats instead of its NTOK x NTOK dS block -- 0.7 instead of 9.6 KB -- and the reduction over the units reads
// that much less (attn_ds_reduce_kernel is gone from this path).
constexpr int ND = 2 * WS - 1;
__device__ __forceinline__ void dtable_stage1(const float* sds, int lane, float (&racc)[ND]) {
    if (lane >= WS * WS) return;
    const int iy = lane / WS, jy = lane - iy * WS;
    const float* base = sds + iy * WS * DS_LD + jy * WS;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        constexpr int W1 = WS - 1;
        const int dx = d - W1;
        float s = 0.f;
#pragma unroll
        for (int jx = 0; jx < WS; ++jx)
            if (jx + dx >= 0 && jx + dx < WS) s += base[(jx + dx) * DS_LD + jx];      // (resolved at compile time)
        racc[d] += s;
    }
}
// R through `tile` (>= WS^2 * ND floats: the dead dS tile), then this unit's table partial: out[idx * stride]
__device__ __forceinline__ void dtable_stage2(float* tile, int lane, const float (&racc)[ND], float* out, int stride) {
    __builtin_amdgcn_wave_barrier();
    if (lane < WS * WS) {
#pragma unroll
        for (int d = 0; d < ND; ++d) tile[lane * ND + d] = racc[d];
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int e = 0; e < (NBIAS + 63) / 64; ++e) {
        const int idx = lane + 64 * e;
        if (idx >= NBIAS) break;
        const int dy = idx / ND - (WS - 1), d = idx - (idx / ND) * ND;
        float s = 0.f;
#pragma unroll
        for (int jy = 0; jy < WS; ++jy) {
            const int iy = jy + dy;
            const bool ok = iy >= 0 && iy < WS;
            const float v = tile[((ok ? iy : 0) * WS + jy) * ND + d];
            s += ok ? v : 0.f;
        }
        out[idx * stride] = s;
    }
}
static_assert(WS * WS * ND <= 64 * DS_LD, "R fits the dS tile");

template <int PREC>
__global__ __launch_bounds__(64, 2) void attn_bwd_mfma_kernel(const AttnBwdArgs a) {
    __shared__ float sb[NBPAD];
    __shared__ int srow[64], smeta[64];
    __shared__ __attribute__((aligned(16))) float sds[64 * DS_LD];
    const int lane = threadIdx.x, lj = lane & 15, g = lane >> 4;
    const int nWx = a.W / WS, nWy = a.H / WS;
    int u = blockIdx.x;
    const int h = u % a.nH; u /= a.nH;
    const int wdw = u % (nWx * nWy);
    const int ck = u / (nWx * nWy);
    const int C = a.nH * HD, col = h * HD;
    const int ldq = (int)a.ldq, ldo = (int)a.ldo, lddq = (int)a.lddq;
    for (int i = lane; i < NBIAS; i += 64) sb[i] = a.table[i * a.nH + h];
    fill_row_table(wdw / nWx, wdw % nWx, lane, a.H, a.W, a.shift, srow, smeta);
    __builtin_amdgcn_wave_barrier();
    // this unit's partial of the bias-table gradient: row (ck, w) of a [chunks * windows][NBIAS][nH] matrix
    float* __restrict__ opart = a.dS_part + ((long long)ck * nWy * nWx + wdw) * (NBIAS * a.nH) + h;
    float racc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) racc[d] = 0.f;

    const int b0 = ck * a.chunk;
    const int b1 = b0 + a.chunk < a.B ? b0 + a.chunk : a.B;
    for (int b = b0; b < b1; ++b) {
        const int tb = b * a.H * a.W;
        f32x4 p[4][4], ds[4][4];
        {
            float q1[4][8], k1[4][8];
            load_l1(a.qkv, tb, srow, ldq, col, lane, a.scale, q1);
            load_l1(a.qkv, tb, srow, ldq, C + col, lane, 1.f, k1);
#pragma unroll
            for (int qt = 0; qt < 4; ++qt)
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) p[qt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (PREC == 1) {
                MisBf3 qb[4];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    qb[t] = mis_bf3_from8(q1[t][0], q1[t][1], q1[t][2], q1[t][3], q1[t][4], q1[t][5], q1[t][6], q1[t][7]);
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    const MisBf3 kb = mis_bf3_from8(k1[kt][0], k1[kt][1], k1[kt][2], k1[kt][3], k1[kt][4], k1[kt][5], k1[kt][6], k1[kt][7]);
#pragma unroll
                    for (int qt = 0; qt < 4; ++qt) p[qt][kt] = mis_bf3_dot(qb[qt], kb, p[qt][kt]);
                }
            } else {
#pragma unroll
                for (int s = 0; s < 8; ++s)
#pragma unroll
                    for (int qt = 0; qt < 4; ++qt)
#pragma unroll
                        for (int kt = 0; kt < 4; ++kt)
                            p[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(q1[qt][s], k1[kt][s], p[qt][kt], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            float do1[4][8], v1[4][8];
            load_l1(a.dout, tb, srow, ldo, col, lane, 1.f, do1);
            load_l1(a.qkv, tb, srow, ldq, 2 * C + col, lane, 1.f, v1);
#pragma unroll
            for (int qt = 0; qt < 4; ++qt)
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) ds[qt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (PREC == 1) {
                MisBf3 db[4];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    db[t] = mis_bf3_from8(do1[t][0], do1[t][1], do1[t][2], do1[t][3], do1[t][4], do1[t][5], do1[t][6], do1[t][7]);
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    const MisBf3 vb = mis_bf3_from8(v1[kt][0], v1[kt][1], v1[kt][2], v1[kt][3], v1[kt][4], v1[kt][5], v1[kt][6], v1[kt][7]);
#pragma unroll
                    for (int qt = 0; qt < 4; ++qt) ds[qt][kt] = mis_bf3_dot(db[qt], vb, ds[qt][kt]);
                }
            } else {
#pragma unroll
                for (int s = 0; s < 8; ++s)
#pragma unroll
                    for (int qt = 0; qt < 4; ++qt)
#pragma unroll
                        for (int kt = 0; kt < 4; ++kt)
                            ds[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(do1[qt][s], v1[kt][s], ds[qt][kt], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // softmax rows (query = 16qt + 4g + i; keys = 16kt + lj across the 16 lanes of a group), dS
        int mk[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) mk[kt] = smeta[16 * kt + lj];
#pragma unroll
        for (int qt = 0; qt < 4; ++qt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int mq = smeta[16 * qt + 4 * g + i];
                float mx = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    float v = -INFINITY;
                    if (16 * kt + lj < NTOK) {
                        v = p[qt][kt][i] + sb[(mq & 255) - (mk[kt] & 255) + BIAS_OFF];
                        if (a.shift > 0 && (mk[kt] >> 8) != (mq >> 8)) v += -100.f;
                    }
                    p[qt][kt][i] = v;
                    mx = fmaxf(mx, v);
                }
                mx = row16_max(mx);
                float sum = 0.f;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    const float e = expf(p[qt][kt][i] - mx);
                    p[qt][kt][i] = e;
                    sum += e;
                }
                sum = row16_sum(sum);
                const float inv = 1.f / sum;
                float dot = 0.f;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    p[qt][kt][i] *= inv;
                    dot += p[qt][kt][i] * ds[qt][kt][i];
                }
                dot = row16_sum(dot);
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    const float d = p[qt][kt][i] * (ds[qt][kt][i] - dot);
                    ds[qt][kt][i] = d;
                    sds[(16 * qt + 4 * g + i) * DS_LD + 16 * kt + lj] = d;
                }
            }
        __builtin_amdgcn_sched_barrier(0);
        // dV[key = 16kt + 4g + i'][dim] = sum_query P[query][key] dO[query][dim]
        {
            float x2[4][4][2];
            load_l2(a.dout, tb, srow, ldo, col, lane, 1.f, x2);
            f32x4 acc[4][2];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[kt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (PREC == 1) {
#pragma unroll
                for (int T = 0; T < 2; ++T) {
                    MisBf3 xb[2];
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        xb[nt] = mis_bf3_from8(x2[2 * T][0][nt], x2[2 * T][1][nt], x2[2 * T][2][nt], x2[2 * T][3][nt],
                                               x2[2 * T + 1][0][nt], x2[2 * T + 1][1][nt], x2[2 * T + 1][2][nt], x2[2 * T + 1][3][nt]);
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt) {
                        const MisBf3 ab = mis_bf3_from8(p[2 * T][kt][0], p[2 * T][kt][1], p[2 * T][kt][2], p[2 * T][kt][3],
                                                        p[2 * T + 1][kt][0], p[2 * T + 1][kt][1], p[2 * T + 1][kt][2], p[2 * T + 1][kt][3]);
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) acc[kt][nt] = mis_bf3_dot(ab, xb[nt], acc[kt][nt]);
                    }
                }
            } else {
#pragma unroll
                for (int qt = 0; qt < 4; ++qt)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                            for (int nt = 0; nt < 2; ++nt)
                                acc[kt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[qt][kt][i], x2[qt][i][nt], acc[kt][nt], 0, 0, 0);
            }
            store_l2(a.dqkv, tb, srow, lddq, 2 * C + col, lane, 1.f, acc);
        }
        __builtin_amdgcn_sched_barrier(0);
        // dK[key][dim] = sum_query dS[query][key] (scale * Q[query][dim])
        {
            float x2[4][4][2];
            load_l2(a.qkv, tb, srow, ldq, col, lane, a.scale, x2);
            f32x4 acc[4][2];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[kt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (PREC == 1) {
#pragma unroll
                for (int T = 0; T < 2; ++T) {
                    MisBf3 xb[2];
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        xb[nt] = mis_bf3_from8(x2[2 * T][0][nt], x2[2 * T][1][nt], x2[2 * T][2][nt], x2[2 * T][3][nt],
                                               x2[2 * T + 1][0][nt], x2[2 * T + 1][1][nt], x2[2 * T + 1][2][nt], x2[2 * T + 1][3][nt]);
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt) {
                        const MisBf3 ab = mis_bf3_from8(ds[2 * T][kt][0], ds[2 * T][kt][1], ds[2 * T][kt][2], ds[2 * T][kt][3],
                                                        ds[2 * T + 1][kt][0], ds[2 * T + 1][kt][1], ds[2 * T + 1][kt][2], ds[2 * T + 1][kt][3]);
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) acc[kt][nt] = mis_bf3_dot(ab, xb[nt], acc[kt][nt]);
                    }
                }
            } else {
#pragma unroll
                for (int qt = 0; qt < 4; ++qt)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                            for (int nt = 0; nt < 2; ++nt)
                                acc[kt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[qt][kt][i], x2[qt][i][nt], acc[kt][nt], 0, 0, 0);
            }
            store_l2(a.dqkv, tb, srow, lddq, C + col, lane, 1.f, acc);
        }
        __builtin_amdgcn_sched_barrier(0);
        // dQ[query = 16qt + 4g + i'][dim] = scale * sum_key dS[query][key] K[key][dim]; A rows from the LDS tile
        __builtin_amdgcn_wave_barrier();
        {
            f32x4 acc[4][2];
#pragma unroll
            for (int qt = 0; qt < 4; ++qt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[qt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (PREC == 1) {
                // keys 32 T + 8 g + e, e = 0 .. 7: eight consecutive columns of the dS tile in LDS (A) and eight K rows (B)
#pragma unroll
                for (int T = 0; T < 2; ++T) {
                    float kv[8][2];
#pragma unroll
                    for (int e8 = 0; e8 < 8; ++e8) {
                        const int r = 32 * T + 8 * g + e8;
                        const int e = (tb + srow[r & 63]) * ldq + C + col + 2 * lj;      // dimensions 2 lj, 2 lj + 1 (as load_l2)
                        const float2 v = r < NTOK ? *reinterpret_cast<const float2*>(a.qkv + e) : make_float2(0.f, 0.f);
                        kv[e8][0] = v.x;
                        kv[e8][1] = v.y;
                    }
                    MisBf3 kb[2];
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        kb[nt] = mis_bf3_from8(kv[0][nt], kv[1][nt], kv[2][nt], kv[3][nt], kv[4][nt], kv[5][nt], kv[6][nt], kv[7][nt]);
#pragma unroll
                    for (int qt = 0; qt < 4; ++qt) {
                        const float4 a0 = *reinterpret_cast<const float4*>(&sds[(16 * qt + lj) * DS_LD + 32 * T + 8 * g]);
                        const float4 a1 = *reinterpret_cast<const float4*>(&sds[(16 * qt + lj) * DS_LD + 32 * T + 8 * g + 4]);
                        const MisBf3 ab = mis_bf3_from8(a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w);
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) acc[qt][nt] = mis_bf3_dot(ab, kb[nt], acc[qt][nt]);
                    }
                }
            } else {
#pragma unroll
                for (int st = 0; st < (NTOK + 3) / 4; ++st) {
                    float kb[2];
                    const int r = 4 * st + g;
                    const int e = (tb + srow[r]) * ldq + C + col + 2 * lj;
                    const float2 v = r < NTOK ? *reinterpret_cast<const float2*>(a.qkv + e) : make_float2(0.f, 0.f);
                    kb[0] = v.x;
                    kb[1] = v.y;
    #pragma unroll
                    for (int qt = 0; qt < 4; ++qt) {
                        const float av = sds[(16 * qt + lj) * DS_LD + 4 * st + g];
    #pragma unroll
                        for (int nt = 0; nt < 2; ++nt)
                            acc[qt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, kb[nt], acc[qt][nt], 0, 0, 0);
                    }
                }
            }
            store_l2(a.dqkv, tb, srow, lddq, col, lane, a.scale, acc);
        }
        dtable_stage1(sds, lane, racc);            // the tile still holds this sample's dS
        __builtin_amdgcn_wave_barrier();
    }
    dtable_stage2(sds, lane, racc, opart, a.nH);
}

// Bias-table gradient, stage 1: dsum[h][e] = sum over the partial blocks of part[p][h][e], e < 49*49.
// grid = (ceil(2401/64), nH); block = 64 consecutive e (coalesced 256-byte rows) x 16 partial lanes, double
// accumulators, fixed-order tree over the lanes.
__global__ __launch_bounds__(1024) void attn_ds_reduce_kernel(const float* __restrict__ part, int nparts, int nH,
                                                              float* __restrict__ dsum) {
    __shared__ double red[1024];
    const int el = threadIdx.x & 63, pl = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + el, h = blockIdx.y;
    const long long stride = (long long)nH * (NTOK * NTOK);
    double s = 0.0;
    if (e < NTOK * NTOK) {
        const float* __restrict__ m = part + (long long)h * (NTOK * NTOK) + e;
        int p = pl;
        for (; p + 48 < nparts; p += 64) {
            const float v0 = m[p * stride], v1 = m[(p + 16) * stride], v2 = m[(p + 32) * stride], v3 = m[(p + 48) * stride];
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; p < nparts; p += 16) s += m[p * stride];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (pl == 0 && e < NTOK * NTOK) {
#pragma unroll
        for (int j = 1; j < 16; ++j) s += red[j * 64 + el];
        dsum[(long long)h * (NTOK * NTOK) + e] = (float)s;
    }
}

// stage 2: dtable[idx][h] (+)= sum of dsum[h][(i, j)] over the <= 49 pairs with relative-position index idx
__global__ __launch_bounds__(256) void attn_dtable_kernel(const float* __restrict__ dsum, int nH,
                                                          float* __restrict__ dtable, int accumulate) {
    const int o = blockIdx.x * 256 + threadIdx.x;              // idx*nH + h
    if (o >= NBIAS * nH) return;
    const int idx = o / nH, h = o - idx * nH;
    const int dy = idx / (2 * WS - 1) - (WS - 1), dx = idx % (2 * WS - 1) - (WS - 1);
    const float* __restrict__ m = dsum + (long long)h * (NTOK * NTOK);
    double s = 0.0;
    for (int jy = 0; jy < WS; ++jy) {
        const int iy = jy + dy;
        if (iy < 0 || iy >= WS) continue;
        for (int jx = 0; jx < WS; ++jx) {
            const int ix = jx + dx;
            if (ix < 0 || ix >= WS) continue;
            s += m[(iy * WS + ix) * NTOK + jy * WS + jx];
        }
    }
    dtable[o] = accumulate ? dtable[o] + (float)s : (float)s;
}

// MFMA path: dtable[c] (+)= sum over the (image, window) rows of part[row][c], c = idx * nH + h (the units wrote their table
// partials in the gradient's own layout).  32 columns x 32 row lanes, double accumulators, fixed order.
__global__ __launch_bounds__(1024) void attn_dtable_sum_kernel(const float* __restrict__ part, int rows, int ncol,
                                                               float* __restrict__ dtable, int accumulate) {
    __shared__ double red[1024];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + cl;
    double s = 0.0;
    if (col < ncol) {
        int r = rl;
        for (; r + 224 < rows; r += 256) {
            float p[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) p[j] = part[(long long)(r + 32 * j) * ncol + col];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += p[j];
        }
        for (; r < rows; r += 32) s += part[(long long)r * ncol + col];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (rl == 0 && col < ncol) {
#pragma unroll
        for (int k = 1; k < 32; ++k) s += red[k * 32 + cl];
        dtable[col] = accumulate ? dtable[col] + (float)s : (float)s;
    }
}

int geometry_ok(int B, int H, int W, int nH, int shift) {
    if (B <= 0 || H <= 0 || W <= 0 || nH <= 0) return MIS_ERR_ARG;
    if (H % WS || W % WS || shift < 0 || shift >= WS) return MIS_ERR_UNSUPPORTED;
    return MIS_OK;
}

// samples per backward wave (its dS partial is accumulated over them): the count in 1..8 that needs the fewest
// rounds of the 1024 resident waves (one per SIMD) times samples per round -- e.g. 48 images at 56^2: 3 (3072 waves =
// exactly three rounds) instead of 4 (2304 waves: the third round would run a quarter full); ties go to the larger
// count (fewer partials for the bias-gradient reduction)
bool use_valu();

int bwd_chunk(int B, int H, int W, int nH) {
    if (!use_valu()) return 1;      // the MFMA kernel writes one dS partial per unit (see its header)
    const long long per_sample = (long long)(H / WS) * (W / WS) * nH;
    int best = 1;
    long long best_cost = -1;
    for (int c = 1; c <= 8 && c <= B; ++c) {
        const long long waves = mis_cdiv(B, c) * per_sample;
        const long long cost = mis_cdiv(waves, 1024) * c;
        if (best_cost < 0 || cost <= best_cost) { best = c; best_cost = cost; }
    }
    return best;
}

// MIS_ATTN_VALU=1 selects the first-generation vector-pipe kernels (kept for A/B measurements)
bool use_valu() {
    static const bool v = getenv("MIS_ATTN_VALU") != nullptr;
    return v;
}

// Which kernels serve a launch, decided HERE and nowhere else: the forward and backward launchers, the layout of the backward's
// table partials (window_attention_table_partials) and the label mis_window_attention_path gives a test all read this function,
// so they cannot diverge.  ldmax = the largest row stride (in floats) among the launch's token buffers; 0 = no buffer (the
// table-gradient half on its own, the shape queries).
//
// Why < 2^31 BYTES is sufficient for the MFMA kernels' 32-bit indices: every global access there is base + e with an int element
// offset e = (tb + srow[r]) * ld + col0 + d (load_l1 / load_l2 / store_l2 and the dQ operand loads).  tb + srow[r] is a token
// number < B*H*W (srow holds valid tokens in all 64 entries: rows >= NTOK alias row 0, and their offset is formed although
// never dereferenced), col0 + d < ld for any buffer that holds its columns, so 0 <= e < B*H*W*ld <= B*H*W*ldmax < 2^29 elements:
// no intermediate of the int arithmetic leaves [0, 2^31), and the scaling to bytes happens in the 64-bit pointer addition.  The
// bound is four times tighter than the arithmetic needs; it is the documented condition and stays.  The partial-table and dS
// offsets are 64-bit in both generations.
enum { ATTN_PATH_MFMA_F32 = 0, ATTN_PATH_MFMA_BF3 = 1, ATTN_PATH_VALU = 2 };

int attn_path(int B, int H, int W, long long ldmax) {
    const bool small = (long long)B * H * W * ldmax * 4 < (1LL << 31);
    if (use_valu() || !small) return ATTN_PATH_VALU;
    return (mis_split_precision_mask() & 4) ? ATTN_PATH_MFMA_BF3 : ATTN_PATH_MFMA_F32;
}

// the label: ATTN_PATH_* for this geometry and stride, or a negative MIS_ERR_*
int window_attention_path(int B, int H, int W, int nH, long long ldmax) {
    if (B <= 0 || H <= 0 || W <= 0 || nH <= 0 || ldmax < 0) return MIS_ERR_ARG;
    if (H % WS || W % WS) return MIS_ERR_UNSUPPORTED;
    return attn_path(B, H, W, ldmax);
}


int window_attention_fwd(const float* qkv, long long ldq, float* out, long long ldo,
                                        const float* bias_table, int B, int H, int W, int nH, int shift, float scale,
                                        hipStream_t stream) {
    int st = geometry_ok(B, H, W, nH, shift);
    if (st) return st;
    if (!qkv || !out || !bias_table) return MIS_ERR_ARG;
    if (ldq % 4 || ldo % 4 || ((uintptr_t)qkv & 15) || ((uintptr_t)out & 15)) return MIS_ERR_UNSUPPORTED;
    AttnArgs a{qkv, ldq, out, ldo, bias_table, B, H, W, nH, shift, scale};
    const long long units = (long long)B * (H / WS) * (W / WS) * nH;
    const int path = attn_path(B, H, W, ldq > ldo ? ldq : ldo);
    if (path == ATTN_PATH_VALU)
        hipLaunchKernelGGL(attn_fwd_kernel, dim3((unsigned)mis_cdiv(units, 4)), dim3(256), 0, stream, a, units);
    else if (path == ATTN_PATH_MFMA_BF3)
        hipLaunchKernelGGL(attn_fwd_mfma_kernel<1>, dim3((unsigned)mis_cdiv(units, 4)), dim3(256), 0, stream, a, units);
    else
        hipLaunchKernelGGL(attn_fwd_mfma_kernel<0>, dim3((unsigned)mis_cdiv(units, 4)), dim3(256), 0, stream, a, units);
    return mis_launch_status();
}

long long window_attention_workspace_bytes(int B, int H, int W, int nH) {
    if (B <= 0 || H <= 0 || W <= 0 || nH <= 0 || H % WS || W % WS) return MIS_ERR_ARG;
    // dS partials [chunks * windows][nH][49*49] + their sum over the partials [nH][49*49]
    return (mis_cdiv(B, bwd_chunk(B, H, W, nH)) * (H / WS) * (W / WS) + 1) * nH * (long long)(NTOK * NTOK) * 4;
}

int window_attention_bwd(const float* qkv, long long ldq, const float* dout, long long ldo,
                                        float* dqkv, long long lddq, const float* bias_table, float* dbias_table,
                                        int accumulate_table, int B, int H, int W, int nH, int shift, float scale,
                                        void* workspace, long long workspace_bytes, hipStream_t stream, int phases = 3) {
    // phases: 1 = the data gradient and the per-unit dS partials (into `workspace`), 2 = the bias-table gradient from the
    // partials; the two halves may run on different streams as long as 2 is ordered behind 1 and the workspace is theirs
    int st = geometry_ok(B, H, W, nH, shift);
    if (st) return st;
    if (!workspace || ((phases & 1) && (!qkv || !dout || !dqkv || !bias_table)) || ((phases & 2) && !dbias_table))
        return MIS_ERR_ARG;
    if ((phases & 1) && (ldq % 4 || ldo % 4 || lddq % 4)) return MIS_ERR_UNSUPPORTED;
    if (workspace_bytes < window_attention_workspace_bytes(B, H, W, nH)) return MIS_ERR_WORKSPACE;
    AttnBwdArgs a{qkv, ldq, dout, ldo, dqkv, lddq, bias_table, reinterpret_cast<float*>(workspace),
                  B, H, W, nH, shift, bwd_chunk(B, H, W, nH), scale};
    const int chunks = (int)mis_cdiv(B, a.chunk);
    const int nW = (H / WS) * (W / WS);
    long long ldmax = ldq > ldo ? ldq : ldo;
    if (lddq > ldmax) ldmax = lddq;
    // (the table-gradient half on its own has no token buffer: ldmax = 0)
    const int path = attn_path(B, H, W, ldmax);
    // the split form is refused where the buffers, not MIS_ATTN_VALU, put the launch on the vector pipe: the half that forms the
    // table gradient does not see the strides and would read MFMA-layout partials (use the one-call form)
    if (phases != 3 && path == ATTN_PATH_VALU && !use_valu()) return MIS_ERR_UNSUPPORTED;
    if (phases & 1) {
        if (path == ATTN_PATH_VALU)
            hipLaunchKernelGGL(attn_bwd_kernel, dim3(chunks * nW * nH), dim3(64), 0, stream, a);
        else if (path == ATTN_PATH_MFMA_BF3)
            hipLaunchKernelGGL(attn_bwd_mfma_kernel<1>, dim3(chunks * nW * nH), dim3(64), 0, stream, a);
        else
            hipLaunchKernelGGL(attn_bwd_mfma_kernel<0>, dim3(chunks * nW * nH), dim3(64), 0, stream, a);
    }
    if (phases & 2) {
        // the layout of the partials follows the kernel of phase 1: the same `path` in the one-call form, and in the split form
        // the refusal above leaves only MIS_ATTN_VALU to select the vector pipe, which both halves see
        if (path == ATTN_PATH_VALU) {
            float* dsum = a.dS_part + (long long)chunks * nW * nH * (NTOK * NTOK);
            hipLaunchKernelGGL(attn_ds_reduce_kernel, dim3((NTOK * NTOK + 63) / 64, nH), dim3(1024), 0, stream, a.dS_part,
                               chunks * nW, nH, dsum);
            hipLaunchKernelGGL(attn_dtable_kernel, dim3((NBIAS * nH + 255) / 256), dim3(256), 0, stream, dsum, nH, dbias_table,
                               accumulate_table);
        } else {
            hipLaunchKernelGGL(attn_dtable_sum_kernel, dim3((NBIAS * nH + 31) / 32), dim3(1024), 0, stream, a.dS_part, chunks * nW,
                               NBIAS * nH, dbias_table, accumulate_table);
        }
    }
    return mis_launch_status();
}

// rows x cols of the table partials the MFMA backward leaves in its workspace (float [rows][cols], cols = NBIAS * nH in the
// gradient's own order): the callers that sum them in a batch (mis_colsum_batch).  MIS_ERR_UNSUPPORTED: the vector-pipe kernels
// are selected (MIS_ATTN_VALU), whose workspace holds dS blocks.
int window_attention_table_partials(int B, int H, int W, int nH, long long* rows, int* cols) {
    if (B <= 0 || H <= 0 || W <= 0 || nH <= 0 || H % WS || W % WS || !rows || !cols) return MIS_ERR_ARG;
    if (attn_path(B, H, W, 0) == ATTN_PATH_VALU) return MIS_ERR_UNSUPPORTED;
    *rows = mis_cdiv(B, bwd_chunk(B, H, W, nH)) * (H / WS) * (W / WS);
    *cols = NBIAS * nH;
    return MIS_OK;
}

}  // namespace MIS_ATTN_NS
