// Input pipeline on the device: the training set lives in HBM (288 GB hold every ACDC slice / BraTS volume many
// times over) and a batch is ONE gather launch that applies the reference's per-sample augmentation while it
// copies -- no host-side numpy/scipy work, no H2D of pixels in the hot loop (only B small parameter records).
//
// Replaces (reference code/dataloaders/dataset.py, code/dataloaders/brats2019.py):
//   RandomGenerator.__call__          dataset.py:406-425   (random_rot_flip | random_rotate, then zoom to patch_size)
//   random_rot_flip                   dataset.py:79-89     np.rot90(k) + np.flip(axis)
//   random_rotate                     dataset.py:92-96     scipy.ndimage.rotate(angle, order=0, reshape=False)
//   scipy.ndimage.zoom(order=0)       dataset.py:419-420   (scipy 1.15: ni_interpolation.c NI_ZoomShift)
//   RandomRotFlip / RandomCrop / ToTensor   brats2019.py:84-147,196-208
//
// All transforms are nearest-neighbour gathers, so their composition is a gather too: for an output pixel the
// kernel walks the index maps backwards (zoom -> rotate | flip+rot90 -> source).  The coordinate arithmetic
// restates scipy's C code operation for operation in IEEE double without contraction, so the selected source pixel
// is the one scipy selects, ties and "one ulp outside -> constant 0" cases included:
//   zoom:    cc = kk * ((in-1)/(out-1));  outside if cc < 0 || cc > in-1;  src = floor(cc + 0.5)
//   rotate:  cc_i = offset_i + o_0*m_i0 + o_1*m_i1 (left to right);  same outside rule and rounding
// Random draws stay on the host (the reference's `random` / `np.random` call order) and arrive as parameters.
#include "common.h"

namespace {

// source index of element (y, x) of flip(rot90(src, k), axis); src is H x W
__device__ __forceinline__ void undo_rotflip(int k, int axis, int H, int W, int y, int x, int& sy, int& sx) {
    const int Ht = (k & 1) ? W : H, Wt = (k & 1) ? H : W;
    if (axis == 0) y = Ht - 1 - y; else x = Wt - 1 - x;
    switch (k & 3) {
        case 0: sy = y; sx = x; break;
        case 1: sy = x; sx = W - 1 - y; break;
        case 2: sy = H - 1 - y; sx = W - 1 - x; break;
        default: sy = H - 1 - x; sx = y; break;
    }
}

// scipy zoom(order=0, mode='constant', grid_mode=False): output index kk of n_out -> input index of n_in, -1 = outside
__device__ __forceinline__ int zoom_src(int kk, int n_in, int n_out) {
    const double z = n_out > 1 ? __ddiv_rn((double)(n_in - 1), (double)(n_out - 1)) : 1.0;
    const double cc = __dmul_rn((double)kk, z);
    if (cc < 0.0 || cc > (double)(n_in - 1)) return -1;
    return (int)floor(__dadd_rn(cc, 0.5));
}

// grid = (ceil(out_w*out_h / 256), B)
__global__ __launch_bounds__(256) void augment2d_kernel(const float* __restrict__ img_pool,
                                                        const unsigned char* __restrict__ lab_pool,
                                                        const MisAug2D* __restrict__ params, int out_h, int out_w,
                                                        float* __restrict__ image_out,
                                                        unsigned char* __restrict__ label_out) {
    const MisAug2D p = params[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= out_h * out_w) return;
    const int oy = i / out_w, ox = i - oy * out_w;
    const bool swap = p.mode == 1 && (p.k & 1);
    const int Ht = swap ? p.W : p.H, Wt = swap ? p.H : p.W;
    const int y1 = zoom_src(oy, Ht, out_h), x1 = zoom_src(ox, Wt, out_w);
    int sy = -1, sx = -1;
    if (y1 >= 0 && x1 >= 0) {
        if (p.mode == 0) {
            sy = y1; sx = x1;
        } else if (p.mode == 1) {
            undo_rotflip(p.k, p.axis, p.H, p.W, y1, x1, sy, sx);
        } else {
            const double c0 = __dadd_rn(__dadd_rn(p.off0, __dmul_rn((double)y1, p.m00)), __dmul_rn((double)x1, p.m01));
            const double c1 = __dadd_rn(__dadd_rn(p.off1, __dmul_rn((double)y1, p.m10)), __dmul_rn((double)x1, p.m11));
            if (!(c0 < 0.0 || c0 > (double)(p.H - 1) || c1 < 0.0 || c1 > (double)(p.W - 1))) {
                sy = (int)floor(__dadd_rn(c0, 0.5));
                sx = (int)floor(__dadd_rn(c1, 0.5));
            }
        }
    }
    const long long o = (long long)blockIdx.y * out_h * out_w + i;
    const bool in = sy >= 0;
    const long long s = (long long)sy * p.W + sx;
    image_out[o] = in ? img_pool[p.img_off + s] : 0.f;
    if (label_out) label_out[o] = (in && lab_pool) ? lab_pool[p.lab_off + s] : (unsigned char)0;
}

// grid = (ceil(p0*p1*p2 / 256), B); innermost output dim == innermost source dim (coalesced both ways)
__global__ __launch_bounds__(256) void crop_rotflip3d_kernel(const float* __restrict__ img_pool,
                                                             const unsigned char* __restrict__ lab_pool,
                                                             const MisCrop3D* __restrict__ params, int p0, int p1, int p2,
                                                             float* __restrict__ image_out, void* __restrict__ label_out,
                                                             int label_bytes) {
    const MisCrop3D p = params[blockIdx.y];
    const long long n = (long long)p0 * p1 * p2;
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    const int l = (int)(i % p2);
    const int j = (int)((i / p2) % p1);
    const int a = (int)(i / ((long long)p1 * p2));
    const int t0 = a + p.o0, t1 = j + p.o1, t2 = l + p.o2;
    const int T0 = (p.k & 1) ? p.d1 : p.d0, T1 = (p.k & 1) ? p.d0 : p.d1;
    const bool in = t0 >= 0 && t0 < T0 && t1 >= 0 && t1 < T1 && t2 >= 0 && t2 < p.d2;
    long long s = 0;
    if (in) {
        int s0, s1;
        undo_rotflip(p.k, p.axis, p.d0, p.d1, t0, t1, s0, s1);
        s = ((long long)s0 * p.d1 + s1) * p.d2 + t2;
    }
    const long long o = (long long)blockIdx.y * n + i;
    image_out[o] = in ? img_pool[p.img_off + s] : 0.f;
    if (label_out) {
        const unsigned char v = (in && lab_pool) ? lab_pool[p.lab_off + s] : (unsigned char)0;
        if (label_bytes == 1) reinterpret_cast<unsigned char*>(label_out)[o] = v;
        else reinterpret_cast<long long*>(label_out)[o] = (long long)v;
    }
}

}  // namespace

extern "C" int mis_augment2d(const float* img_pool, const unsigned char* lab_pool, const void* params, int B,
                             int out_h, int out_w, float* image_out, unsigned char* label_out, hipStream_t stream) {
    static_assert(sizeof(MisAug2D) == 88, "MisAug2D layout");
    if (!img_pool || !params || !image_out || B <= 0 || out_h <= 0 || out_w <= 0) return MIS_ERR_ARG;
    if (label_out && !lab_pool) return MIS_ERR_ARG;
    hipLaunchKernelGGL(augment2d_kernel, dim3((unsigned)mis_cdiv((long long)out_h * out_w, 256), B), dim3(256), 0, stream,
                       img_pool, lab_pool, reinterpret_cast<const MisAug2D*>(params), out_h, out_w, image_out, label_out);
    return mis_launch_status();
}

extern "C" int mis_crop_rotflip3d(const float* img_pool, const unsigned char* lab_pool, const void* params, int B,
                                  int p0, int p1, int p2, float* image_out, void* label_out, int label_bytes,
                                  hipStream_t stream) {
    static_assert(sizeof(MisCrop3D) == 48, "MisCrop3D layout");
    if (!img_pool || !params || !image_out || B <= 0 || p0 <= 0 || p1 <= 0 || p2 <= 0) return MIS_ERR_ARG;
    if (label_out && (!lab_pool || (label_bytes != 1 && label_bytes != 8))) return MIS_ERR_ARG;
    hipLaunchKernelGGL(crop_rotflip3d_kernel, dim3((unsigned)mis_cdiv((long long)p0 * p1 * p2, 256), B), dim3(256), 0,
                       stream, img_pool, lab_pool, reinterpret_cast<const MisCrop3D*>(params), p0, p1, p2, image_out,
                       label_out, label_bytes);
    return mis_launch_status();
}
