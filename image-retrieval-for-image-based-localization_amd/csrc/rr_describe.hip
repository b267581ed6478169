// librr.so — keypoint description: local-affine-frame patches, the dominant gradient orientation of
// a patch, the SIFT descriptor of a patch, and the three fused into one kernel per keypoint.
// Replaces extract_patches_simple with generate_patch_grid_from_normalized_LAF of
// cirtorch/features/laf.py:260-308 (F.affine_grid + F.grid_sample), make_upright of laf.py:112-134,
// PatchDominantGradientOrientation.forward and LAFOrienter.forward of
// cirtorch/features/orientation.py:56-105,122-150 (SpatialGradient of cirtorch/filters/sobel.py) and
// SIFTDescriptor.forward of cirtorch/features/siftdesc.py:78-129 (spatial_gradient 'diff',
// get_gaussian_kernel2d of cirtorch/filters/kernels.py:529-551, get_sift_pooling_kernel of
// siftdesc.py:11-18); with them the descriptor half of the host-side cv2 SIFT of
// cirtorch/datasets/localFeatures/utils.py:56-99.
//
// Everything is float64 on float32 values, every sum has one fixed order, each output is rounded
// once to float32, no atomic touches a floating-point value, nothing waits for the host, and this
// file is compiled without floating-point contraction, so a phase gives the same bits in every
// kernel that inlines it.  One block of 256 threads works on one patch; the phases, all in LDS:
//
//   sample     pixel (i, j) of the patch of frame A: u = (2 j + 1) / ps - 1, v = (2 i + 1) / ps - 1,
//              sx = ((a00 u + a01 v) + a02) - 0.5, sy likewise, clamped to the image, bilinear blend
//              of floor and min(floor + 1, size - 1), rounded to float32 (a patch IS float32 in the
//              reference's chain).  A frame with a non-finite entry gives a zero patch.
//   orient     Sobel / 8 gradients at clamped patch coordinates, mag = sqrt((dx^2 + dy^2) + 1e-8),
//              ori = atan2(dy, dx + 1e-8) + 2 pi, o = nb (ori + pi) / (2 pi), soft-binned into nb bins,
//              (bin b owned by the 256 / nb lanes b, b + nb, ..., each adding every (256 / nb)-th
//              pixel in ascending order, the partial sums added in lane order), the mean over the
//              patch, circular smoothing with the float32 values of
//              [0.33, 0.34, 0.33], argmax (ties to the lower index), angle = -(2 pi idx / nb - pi).
//              pi is the float32 value the reference's geometry/conversions.py:29 holds.
//   sift       central differences / 2, mag = sqrt((gx^2 + gy^2) + 1e-10) G(y, x), ori =
//              atan2(gy, gx + 1e-10) + 2 pi, o = nb ori / (2 pi); per pixel the bin b0 and the two
//              weights (1 - w1) mag, w1 mag stay in LDS.  Output (a, cy, cx) is owned by P fixed
//              lanes (P a power of two, P dim <= 256): lane p walks the rows of the ksize x ksize
//              window ascending and in each row the columns kx = p, p + P, ...; the P partial sums
//              are added in ascending p.  Then the two L2 normalisations around the clamp and
//              RootSIFT; the sums of a norm are per thread ascending, a butterfly over the wave and
//              the four waves in order.
//              G is the outer product, in float32, of the 1-D Gaussian of sigma = ps / sqrt 2 (each
//              weight computed in float64 and rounded to float32); the pooling kernel holds the
//              float32 values (xc[ky] xc[kx]) / (ksize / 2)^2 of get_sift_pooling_kernel.
//
// Bin sums by fixed lanes instead of atomics are what makes a descriptor a function of its patch
// alone: not of the batch, the slot, the launch or the run.
#include "rr_internal.h"

#include <math.h>

#pragma clang fp contract(off)

namespace rr {

namespace {

constexpr int Q_TB = 256;                     // threads per patch
constexpr int Q_MINPS = 8, Q_MAXPS = 64;
constexpr int Q_MAXANG = 16, Q_MAXSP = 8;     // SIFT bins
constexpr int Q_MAXOBINS = 64;                // orientation bins
constexpr long long Q_MAXPIX = 1ll << 31;
constexpr long long Q_MAXBLOCKS = (1ll << 24) - 1;   // one block of 256 threads each: a grid holds fewer than 2^32 threads
constexpr double Q_PI = (double)3.14159265358979323846f;   // the float32 value, as the reference's pi tensor

__device__ __forceinline__ int qclampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <bool U8> __device__ __forceinline__ double q_load(const void* x, long long i) {
    if constexpr (U8)  // IEEE division: the same float as torch's x.float() / 255
        return (double)((float)reinterpret_cast<const unsigned char*>(x)[i] / 255.f);
    else
        return (double)reinterpret_cast<const float*>(x)[i];
}

// one plane (or, gray, three planes hw apart reduced on the fly) of an image
template <bool U8> __device__ __forceinline__ double q_pixel(const void* src, long long hw, long long o, int gray) {
    if (gray) return (0.299 * q_load<U8>(src, o) + 0.587 * q_load<U8>(src, hw + o)) + 0.114 * q_load<U8>(src, 2 * hw + o);
    return q_load<U8>(src, o);
}

struct Frame {
    float a00, a01, a02, a10, a11, a12;
    __device__ __forceinline__ bool finite() const {
        return isfinite(a00) && isfinite(a01) && isfinite(a02) && isfinite(a10) && isfinite(a11) && isfinite(a12);
    }
};

// pixel i = row * ps + col of the patch of frame f
template <bool U8>
__device__ __forceinline__ float q_sample(const void* src, long long hw, int h, int w, int gray, const Frame& f, bool ok,
                                          int ps, int i) {
    if (!ok) return 0.f;
    const int r = i / ps, c = i - r * ps;
    const double u = (double)(2 * c + 1) / (double)ps - 1.0, v = (double)(2 * r + 1) / (double)ps - 1.0;
    double sx = (((double)f.a00 * u + (double)f.a01 * v) + (double)f.a02) - 0.5;
    double sy = (((double)f.a10 * u + (double)f.a11 * v) + (double)f.a12) - 0.5;
    sx = sx < 0.0 ? 0.0 : (sx > (double)(w - 1) ? (double)(w - 1) : sx);
    sy = sy < 0.0 ? 0.0 : (sy > (double)(h - 1) ? (double)(h - 1) : sy);
    const int x0 = (int)floor(sx), y0 = (int)floor(sy);
    const int x1 = x0 + 1 < w ? x0 + 1 : w - 1, y1 = y0 + 1 < h ? y0 + 1 : h - 1;
    const double fx = sx - (double)x0, fy = sy - (double)y0;
    const double p00 = q_pixel<U8>(src, hw, (long long)y0 * w + x0, gray), p01 = q_pixel<U8>(src, hw, (long long)y0 * w + x1, gray);
    const double p10 = q_pixel<U8>(src, hw, (long long)y1 * w + x0, gray), p11 = q_pixel<U8>(src, hw, (long long)y1 * w + x1, gray);
    const double val = ((p00 * ((1.0 - fx) * (1.0 - fy)) + p01 * (fx * (1.0 - fy))) + p10 * ((1.0 - fx) * fy)) + p11 * (fx * fy);
    return (float)val;
}

// The block's LDS, carved from one dynamic allocation (lds_bytes below).
struct Lds {
    double* w0;      // [ps ps]   (1 - w1) mag of the pixel's lower bin
    double* w1;      // [ps ps]   w1 mag of the bin above it
    double* part;    // [max(dim, 256)] partial sums of the owning lanes
    double* vals;    // [max(dim, 64)]  bin sums, histogram, descriptor
    double* red;     // [8]       wave sums of a block reduction, the angle
    float* patch;    // [ps ps]
    int* b0;         // [ps ps]
    float* pk;       // [ksize ksize] pooling kernel
    float* g1;       // [ps]      1-D Gaussian
};

__host__ __device__ inline int q_npart(int dim) { return dim > 256 ? dim : 256; }
__host__ __device__ inline int q_nvals(int dim) { return dim > Q_MAXOBINS ? dim : Q_MAXOBINS; }

__host__ __device__ inline size_t lds_bytes(int ps, int dim, int ksize) {
    const size_t n = (size_t)ps * ps;
    return n * 16 + ((size_t)q_npart(dim) + q_nvals(dim) + 8) * 8 + n * 8 + (size_t)ksize * ksize * 4 + (size_t)ps * 4;
}

__device__ __forceinline__ Lds carve(unsigned char* base, int ps, int dim, int ksize) {
    const size_t n = (size_t)ps * ps;
    Lds L;
    L.w0 = reinterpret_cast<double*>(base);
    L.w1 = L.w0 + n;
    L.part = L.w1 + n;
    L.vals = L.part + q_npart(dim);
    L.red = L.vals + q_nvals(dim);
    L.patch = reinterpret_cast<float*>(L.red + 8);
    L.b0 = reinterpret_cast<int*>(L.patch + n);
    L.pk = reinterpret_cast<float*>(L.b0 + n);
    L.g1 = L.pk + (size_t)ksize * ksize;
    return L;
}

// sum of one value per thread in a fixed order: butterfly over the wave, the four waves ascending
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum_d(v);
    __syncthreads();   // the previous reduction's reads of red are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// soft bin of an orientation: o >= 0
__device__ __forceinline__ void soft_bin(double o, double mag, int nb, int i, const Lds& L) {
    const double f = floor(o), w1 = o - f;
    int b = (int)fmod(f, (double)nb);
    if (!(b >= 0 && b < nb)) b = 0;   // a NaN patch: any bin, the sums are NaN anyway
    L.b0[i] = b;
    L.w0[i] = (1.0 - w1) * mag;
    L.w1[i] = w1 * mag;
}

// what pixel i gives to bin a
__device__ __forceinline__ double bin_value(const Lds& L, int i, int a, int nb) {
    const int b = L.b0[i], b1 = b + 1 == nb ? 0 : b + 1;
    return (b == a ? L.w0[i] : 0.0) + (b1 == a ? L.w1[i] : 0.0);
}
// the same for the orientation histogram: false when the pixel gives nothing (its share is +0, so
// skipping it changes no bit of a sum).  With 36 bins, 2 of them hit, a lane skips 17 pixels of 18
// without reading a weight; in the pooling (8 bins) the skip gained nothing, so the
// pooling uses bin_value.
__device__ __forceinline__ bool bin_share(const Lds& L, int i, int a, int nb, double& c) {
    const int b = L.b0[i], b1 = b + 1 == nb ? 0 : b + 1;
    if (b != a && b1 != a) return false;
    c = (b == a ? L.w0[i] : 0.0) + (b1 == a ? L.w1[i] : 0.0);
    return true;
}

// The dominant gradient orientation of L.patch; the angle (float32) is returned to every thread.
__device__ float orient_phase(const Lds& L, int ps, int nb) {
    const int tid = threadIdx.x, n = ps * ps;
    for (int i = tid; i < n; i += Q_TB) {
        const int y = i / ps, x = i - y * ps;
        const int y0 = qclampi(y - 1, ps - 1) * ps, y1 = y * ps, y2 = qclampi(y + 1, ps - 1) * ps;
        const int x0 = qclampi(x - 1, ps - 1), x2 = qclampi(x + 1, ps - 1);
        const double a00 = L.patch[y0 + x0], a01 = L.patch[y0 + x], a02 = L.patch[y0 + x2];
        const double a10 = L.patch[y1 + x0], a12 = L.patch[y1 + x2];
        const double a20 = L.patch[y2 + x0], a21 = L.patch[y2 + x], a22 = L.patch[y2 + x2];
        const double dx = ((a02 - a00) + 2.0 * (a12 - a10) + (a22 - a20)) * 0.125;
        const double dy = ((a20 - a00) + 2.0 * (a21 - a01) + (a22 - a02)) * 0.125;
        const double mag = sqrt((dx * dx + dy * dy) + 1e-8);
        const double ori = atan2(dy, dx + 1e-8) + 2.0 * Q_PI;
        soft_bin(((double)nb * (ori + Q_PI)) / (2.0 * Q_PI), mag, nb, i, L);
    }
    __syncthreads();
    // bin b is owned by the P = 256 / nb lanes b, b + nb, ...: lane (b, p) adds the pixels p, p + P, ...
    // in ascending order, the P partial sums are added in ascending p.  The lanes of one part read
    // the same pixel (a broadcast), consecutive parts consecutive pixels.
    const int P = Q_TB / nb, bin = tid % nb, part = tid / nb;
    if (part < P) {
        double s = 0.0, c;
        for (int i = part; i < n; i += P)
            if (bin_share(L, i, bin, nb, c)) s += c;
        L.part[part * nb + bin] = s;
    }
    __syncthreads();
    if (tid < nb) {
        double t = 0.0;
        for (int p = 0; p < P; ++p) t += L.part[p * nb + tid];
        L.vals[tid] = t / (double)n;
    }
    __syncthreads();
    if (tid == 0) {
        const double k0 = (double)0.33f, k1 = (double)0.34f;
        int best = 0;
        double bv = 0.0;
        for (int i = 0; i < nb; ++i) {
            const double v = (k0 * L.vals[(i + nb - 1) % nb] + k1 * L.vals[i]) + k0 * L.vals[(i + 1) % nb];
            if (i == 0 || v > bv) { bv = v; best = i; }
        }
        L.red[4] = (double)(float)(-(((2.0 * Q_PI) * (double)best) / (double)nb - Q_PI));
    }
    __syncthreads();
    return (float)L.red[4];
}

struct SiftArgs {
    int ps, nb, ns, ksize, stride, pad, rootsift;
    double clipval;
};

// The SIFT descriptor of L.patch -> out[dim] (global).
__device__ void sift_phase(const Lds& L, const SiftArgs& a, float* __restrict__ out) {
    const int tid = threadIdx.x, ps = a.ps, n = ps * ps, nb = a.nb, ns = a.ns, ksize = a.ksize;
    const int dim = nb * ns * ns;
    // tables: the 1-D Gaussian (exp in part, then normalised) and the pooling kernel
    if (tid < ps) {
        const double x = (double)(tid - ps / 2) + ((ps & 1) ? 0.0 : 0.5);
        L.part[tid] = exp(-(x * x) / ((double)ps * (double)ps));   // 2 sigma^2 = ps^2
    }
    {
        const float ks2 = (float)ksize * 0.5f;
        for (int i = tid; i < ksize * ksize; i += Q_TB) {
            const int ky = i / ksize, kx = i - ky * ksize;
            const float xa = ks2 - fabsf(((float)ky + 0.5f) - ks2), xb = ks2 - fabsf(((float)kx + 0.5f) - ks2);
            L.pk[i] = (xa * xb) / (ks2 * ks2);
        }
    }
    __syncthreads();
    if (tid < ps) {
        double s = 0.0;
        for (int i = 0; i < ps; ++i) s += L.part[i];
        L.g1[tid] = (float)(L.part[tid] / s);
    }
    __syncthreads();
    for (int i = tid; i < n; i += Q_TB) {
        const int y = i / ps, x = i - y * ps;
        const double gx = ((double)L.patch[y * ps + qclampi(x + 1, ps - 1)] - (double)L.patch[y * ps + qclampi(x - 1, ps - 1)]) * 0.5;
        const double gy = ((double)L.patch[qclampi(y + 1, ps - 1) * ps + x] - (double)L.patch[qclampi(y - 1, ps - 1) * ps + x]) * 0.5;
        const double mag = sqrt((gx * gx + gy * gy) + 1e-10) * (double)(L.g1[y] * L.g1[x]);
        const double ori = atan2(gy, gx + 1e-10) + 2.0 * Q_PI;
        soft_bin(((double)nb * ori) / (2.0 * Q_PI), mag, nb, i, L);
    }
    __syncthreads();
    // pooling: P lanes per output, consecutive lanes = the parts of one output, then the angular bins of one cell
    int P = 1;
    while (P * 2 * dim <= Q_TB && P < 16) P <<= 1;
    for (int idx = tid; idx < dim * P; idx += Q_TB) {
        const int o = idx / P, part = idx - o * P;
        const int ang = o % nb, cell = o / nb, cy = cell / ns, cx = cell - cy * ns;
        const int ybase = cy * a.stride - a.pad, xbase = cx * a.stride - a.pad;
        double s = 0.0;
        for (int ky = 0; ky < ksize; ++ky) {
            const int y = ybase + ky;
            if (y < 0 || y >= ps) continue;   // zeros outside the patch
            for (int kx = part; kx < ksize; kx += P) {
                const int x = xbase + kx;
                if (x < 0 || x >= ps) continue;
                s += (double)L.pk[ky * ksize + kx] * bin_value(L, y * ps + x, ang, nb);
            }
        }
        L.part[idx] = s;
    }
    __syncthreads();
    for (int o = tid; o < dim; o += Q_TB) {
        double t = 0.0;
        for (int p = 0; p < P; ++p) t += L.part[o * P + p];
        L.vals[(o % nb) * ns * ns + o / nb] = t;
    }
    __syncthreads();
    // L2 normalise, clamp, L2 normalise, RootSIFT; every thread keeps its own elements
    double s = 0.0;
    for (int o = tid; o < dim; o += Q_TB) s += L.vals[o] * L.vals[o];
    double nrm = sqrt(block_sum(s, L.red));
    nrm = nrm < 1e-12 ? 1e-12 : nrm;
    s = 0.0;
    for (int o = tid; o < dim; o += Q_TB) {
        double v = L.vals[o] / nrm;
        v = v < 0.0 ? 0.0 : (v > a.clipval ? a.clipval : v);
        L.vals[o] = v;
        s += v * v;
    }
    nrm = sqrt(block_sum(s, L.red));
    nrm = nrm < 1e-12 ? 1e-12 : nrm;
    s = 0.0;
    for (int o = tid; o < dim; o += Q_TB) {
        const double v = L.vals[o] / nrm;
        L.vals[o] = v;
        s += fabs(v);
    }
    if (a.rootsift) {
        double l1 = block_sum(s, L.red);
        l1 = l1 < 1e-12 ? 1e-12 : l1;
        for (int o = tid; o < dim; o += Q_TB) out[o] = (float)sqrt(L.vals[o] / l1 + 1e-10);
    } else {
        for (int o = tid; o < dim; o += Q_TB) out[o] = (float)L.vals[o];
    }
}

extern __shared__ __attribute__((aligned(16))) unsigned char q_lds[];

// one block per (patch, channel): out [n][npts][co][ps][ps]
template <bool U8>
__global__ void __launch_bounds__(Q_TB) k_extract(const void* __restrict__ x, int c, int h, int w, int gray,
                                                  const float* __restrict__ lafs, int npts, int ps, float* __restrict__ out) {
    const int co = gray ? 1 : c;
    const long long slot = (long long)blockIdx.x / co;   // image * npts + point
    const int ch = (int)((long long)blockIdx.x - slot * co);
    const long long img = slot / npts, hw = (long long)h * w;
    const long long plane = img * c + ch;
    const void* src = U8 ? (const void*)(reinterpret_cast<const unsigned char*>(x) + plane * hw)
                         : (const void*)(reinterpret_cast<const float*>(x) + plane * hw);
    const float* fp = lafs + slot * 6;
    const Frame f{fp[0], fp[1], fp[2], fp[3], fp[4], fp[5]};
    const bool ok = f.finite();
    float* dst = out + (long long)blockIdx.x * ps * ps;
    for (int i = threadIdx.x; i < ps * ps; i += Q_TB) dst[i] = q_sample<U8>(src, hw, h, w, gray, f, ok, ps, i);
}

__global__ void __launch_bounds__(Q_TB) k_orient(const float* __restrict__ patches, int ps, int nb, float* __restrict__ angle) {
    const Lds L = carve(q_lds, ps, 1, 1);
    const float* src = patches + (long long)blockIdx.x * ps * ps;
    for (int i = threadIdx.x; i < ps * ps; i += Q_TB) L.patch[i] = src[i];
    __syncthreads();
    const float a = orient_phase(L, ps, nb);
    if (threadIdx.x == 0) angle[blockIdx.x] = a;
}

__global__ void __launch_bounds__(Q_TB) k_sift(const float* __restrict__ patches, SiftArgs a, float* __restrict__ out) {
    const int dim = a.nb * a.ns * a.ns;
    const Lds L = carve(q_lds, a.ps, dim, a.ksize);
    const float* src = patches + (long long)blockIdx.x * a.ps * a.ps;
    for (int i = threadIdx.x; i < a.ps * a.ps; i += Q_TB) L.patch[i] = src[i];
    __syncthreads();
    sift_phase(L, a, out + (long long)blockIdx.x * dim);
}

// the upright frame of make_upright (laf.py:112-134; get_laf_scale's eps 1e-10, its own 1e-9), float64
__device__ __forceinline__ void q_upright(const Frame& f, double& u00, double& u10, double& u11) {
    const double a00 = f.a00, a01 = f.a01, a10 = f.a10, a11 = f.a11;
    const double det = sqrt(fabs((a00 * a11 - a10 * a01) + 1e-10));
    const double b2a2 = sqrt(a01 * a01 + a00 * a00) + 1e-9;
    u00 = det * (b2a2 / det);
    u10 = det * ((a11 * a01 + a10 * a00) / (b2a2 * det));
    u11 = det * (det / b2a2);
}

// one block per keypoint slot
template <bool U8>
__global__ void __launch_bounds__(Q_TB) k_describe(const void* __restrict__ x, int c, int h, int w, const float* __restrict__ kpts,
                                                   const int* __restrict__ count, int npts, double scale,
                                                   const float* __restrict__ lafs, int orient, int obins, SiftArgs a,
                                                   float* __restrict__ desc, float* __restrict__ angles,
                                                   float* __restrict__ lafs_out) {
    const int tid = threadIdx.x, dim = a.nb * a.ns * a.ns, ps = a.ps;
    const long long slot = blockIdx.x, img = slot / npts;
    const int pt = (int)(slot - img * npts);
    float* dst = desc + slot * dim;
    Frame f;
    if (lafs) {
        const float* fp = lafs + slot * 6;
        f = Frame{fp[0], fp[1], fp[2], fp[3], fp[4], fp[5]};
    } else {
        f = Frame{(float)scale, 0.f, kpts[slot * 2], 0.f, (float)scale, kpts[slot * 2 + 1]};
    }
    if ((count && pt >= count[img]) || (f.a02 == -1.f && f.a12 == -1.f)) {   // block-uniform
        for (int o = tid; o < dim; o += Q_TB) dst[o] = 0.f;
        if (tid == 0 && angles) angles[slot] = 0.f;
        if (tid < 6 && lafs_out) lafs_out[slot * 6 + tid] = 0.f;
        return;
    }
    const Lds L = carve(q_lds, ps, dim, a.ksize);
    const long long hw = (long long)h * w;
    const int gray = c == 3;
    const void* src = U8 ? (const void*)(reinterpret_cast<const unsigned char*>(x) + img * c * hw)
                         : (const void*)(reinterpret_cast<const float*>(x) + img * c * hw);
    float ang = 0.f;
    if (orient) {
        if (lafs) {
            double u00, u10, u11;
            q_upright(f, u00, u10, u11);
            f.a00 = (float)u00; f.a01 = 0.f; f.a10 = (float)u10; f.a11 = (float)u11;
        }
        // the upright frame IS its float32 rounding: the patch is sampled from it and it is what turns
        const double u00 = (double)f.a00, u10 = (double)f.a10, u11 = (double)f.a11;
        const bool ok = f.finite();
        for (int i = tid; i < ps * ps; i += Q_TB) L.patch[i] = q_sample<U8>(src, hw, h, w, gray, f, ok, ps, i);
        __syncthreads();
        ang = orient_phase(L, ps, obins);
        // upright . [[cos, sin], [-sin, cos]] (LAFOrienter's product), rounded once to float32
        const double cs = cos((double)ang), sn = sin((double)ang);
        f.a00 = (float)(u00 * cs);
        f.a01 = (float)(u00 * sn);
        f.a10 = (float)(u10 * cs - u11 * sn);
        f.a11 = (float)(u10 * sn + u11 * cs);
    }
    {
        const bool ok = f.finite();
        for (int i = tid; i < ps * ps; i += Q_TB) L.patch[i] = q_sample<U8>(src, hw, h, w, gray, f, ok, ps, i);
    }
    __syncthreads();
    if (tid == 0 && angles) angles[slot] = ang;
    if (tid == 0 && lafs_out) {
        float* o = lafs_out + slot * 6;
        o[0] = f.a00; o[1] = f.a01; o[2] = f.a02; o[3] = f.a10; o[4] = f.a11; o[5] = f.a12;
    }
    sift_phase(L, a, dst);
}

// ---------------------------------------------------------------- host
constexpr size_t Q_WS = 256;   // no patch, gradient or plane lives in memory: the workspace is a formality

bool q_pixels_ok(long long a, long long b, long long c, long long d) {
    long long p = 1;
    for (long long f : {a, b, c, d}) {
        if (f > 0 && p > Q_MAXPIX / f) return false;
        p *= f;
    }
    return p <= Q_MAXPIX;
}

// the reference's compatibility rule (get_sift_bin_ksize_stride_pad, siftdesc.py:21-37)
bool sift_geometry(int ps, int ns, int& ksize, int& stride, int& pad) {
    ksize = 2 * (int)((double)ps / (double)(ns + 1));
    stride = ps / ns;
    pad = ksize / 4;
    if (ksize < 1) return false;
    const int t = ps + 2 * pad - (ksize - 1) - 1;
    const int out = (t >= 0 ? t / stride : -((-t + stride - 1) / stride)) + 1;   // floor division
    return out == ns;
}

int check_sift(const std::string& w, int ps, int nb, int ns, double clipval, SiftArgs& a) {
    if (ps < Q_MINPS || ps > Q_MAXPS) return fail(RR_EINVAL, w + ": patch size outside [8, 64]");
    if (nb < 1 || nb > Q_MAXANG) return fail(RR_EINVAL, w + ": num_ang_bins outside [1, 16]");
    if (ns < 1 || ns > Q_MAXSP) return fail(RR_EINVAL, w + ": num_spatial_bins outside [1, 8]");
    if (!std::isfinite(clipval)) return fail(RR_EINVAL, w + ": clipval must be finite");
    a.ps = ps; a.nb = nb; a.ns = ns; a.clipval = clipval;
    if (!sift_geometry(ps, ns, a.ksize, a.stride, a.pad))
        return fail(RR_EINVAL, w + ": patch size is incompatible with the number of spatial bins");
    return RR_OK;
}

int check_image(const std::string& w, const void* x, int n, int c, int h, int wd) {
    if (n < 0 || c < 1) return fail(RR_EINVAL, w + ": negative n or c < 1");
    if (h < 1 || wd < 1) return fail(RR_EINVAL, w + ": h and w must be positive");
    if (!q_pixels_ok(n, c, h, wd)) return fail(RR_EINVAL, w + ": more than 2^31 pixels");
    if (n > 0 && !x) return fail(RR_EINVAL, w + ": null input");
    return RR_OK;
}

// LDS above 64 KiB has to be asked for; returns 0 or an error code
template <typename K> int want_lds(K kernel, size_t bytes, const std::string& w) {
    if (bytes <= 65536) return RR_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(RR_EHIP, w + ": cannot reserve the patch's LDS");
    }
    return RR_OK;
}

}  // namespace

}  // namespace rr

using namespace rr;

extern "C" {

size_t rr_describe_workspace_bytes(int n, int npts, int ps, int num_ang_bins, int num_spatial_bins) {
    (void)n; (void)npts; (void)ps; (void)num_ang_bins; (void)num_spatial_bins;
    return Q_WS;
}

int rr_extract_patches(const void* x, int n, int c, int h, int w, int u8, int gray, const float* lafs, int npts, int ps,
                       float* out, void* stream) {
    const std::string nm("rr_extract_patches");
    int rc = check_image(nm, x, n, c, h, w);
    if (rc) return rc;
    if (gray != 0 && gray != 1) return fail(RR_EINVAL, nm + ": gray must be 0 or 1");
    if (gray && c != 3) return fail(RR_EINVAL, nm + ": gray needs c == 3");
    if (npts < 0) return fail(RR_EINVAL, nm + ": negative npts");
    if (ps < Q_MINPS || ps > Q_MAXPS) return fail(RR_EINVAL, nm + ": patch size outside [8, 64]");
    const long long blocks = (long long)n * npts * (gray ? 1 : c);
    if (blocks > Q_MAXBLOCKS) return fail(RR_EINVAL, nm + ": more than 2^24 - 1 patches");
    if (blocks > 0 && (!lafs || !out)) return fail(RR_EINVAL, nm + ": null frames or output");
    if (blocks == 0) return RR_OK;
    if (u8)
        hipLaunchKernelGGL(k_extract<true>, dim3((unsigned)blocks), dim3(Q_TB), 0, as_stream(stream), x, c, h, w, gray, lafs, npts, ps, out);
    else
        hipLaunchKernelGGL(k_extract<false>, dim3((unsigned)blocks), dim3(Q_TB), 0, as_stream(stream), x, c, h, w, gray, lafs, npts, ps, out);
    return check_launch("rr_extract_patches");
}

int rr_patch_orientation(const float* patches, long long B, int ps, int num_ang_bins, float* angle, void* stream) {
    const std::string nm("rr_patch_orientation");
    if (B < 0 || B > Q_MAXBLOCKS) return fail(RR_EINVAL, nm + ": patch count outside [0, 2^24)");
    if (ps < Q_MINPS || ps > Q_MAXPS) return fail(RR_EINVAL, nm + ": patch size outside [8, 64]");
    if (num_ang_bins < 1 || num_ang_bins > Q_MAXOBINS) return fail(RR_EINVAL, nm + ": num_ang_bins outside [1, 64]");
    if (B > 0 && (!patches || !angle)) return fail(RR_EINVAL, nm + ": null input or output");
    if (B == 0) return RR_OK;
    const size_t lds = lds_bytes(ps, 1, 1);
    int rc = want_lds(k_orient, lds, nm);
    if (rc) return rc;
    hipLaunchKernelGGL(k_orient, dim3((unsigned)B), dim3(Q_TB), lds, as_stream(stream), patches, ps, num_ang_bins, angle);
    return check_launch("rr_patch_orientation");
}

int rr_sift_describe(const float* patches, long long B, int ps, int num_ang_bins, int num_spatial_bins, int rootsift,
                     double clipval, float* out, void* stream) {
    const std::string nm("rr_sift_describe");
    if (B < 0 || B > Q_MAXBLOCKS) return fail(RR_EINVAL, nm + ": patch count outside [0, 2^24)");
    SiftArgs a;
    int rc = check_sift(nm, ps, num_ang_bins, num_spatial_bins, clipval, a);
    if (rc) return rc;
    a.rootsift = rootsift != 0;
    if (B > 0 && (!patches || !out)) return fail(RR_EINVAL, nm + ": null input or output");
    if (B == 0) return RR_OK;
    const size_t lds = lds_bytes(ps, a.nb * a.ns * a.ns, a.ksize);
    rc = want_lds(k_sift, lds, nm);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sift, dim3((unsigned)B), dim3(Q_TB), lds, as_stream(stream), patches, a, out);
    return check_launch("rr_sift_describe");
}

int rr_describe_keypoints(const void* x, int n, int c, int h, int w, int u8, const float* kpts, const int* count, int npts,
                          double scale, const float* lafs, int orient, int orient_bins, int ps, int num_ang_bins,
                          int num_spatial_bins, int rootsift, double clipval, float* desc, float* angles, float* lafs_out,
                          void* workspace, size_t workspace_bytes, void* stream) {
    const std::string nm("rr_describe_keypoints");
    if (c != 1 && c != 3) return fail(RR_EINVAL, nm + ": c must be 1 or 3");
    int rc = check_image(nm, x, n, c, h, w);
    if (rc) return rc;
    if (npts < 0) return fail(RR_EINVAL, nm + ": negative npts");
    if (orient != 0 && orient != 1) return fail(RR_EINVAL, nm + ": orient must be 0 or 1");
    if (orient && (orient_bins < 1 || orient_bins > Q_MAXOBINS)) return fail(RR_EINVAL, nm + ": orient_bins outside [1, 64]");
    if (!lafs && !(std::isfinite(scale) && scale > 0.0)) return fail(RR_EINVAL, nm + ": scale must be positive and finite");
    SiftArgs a;
    rc = check_sift(nm, ps, num_ang_bins, num_spatial_bins, clipval, a);
    if (rc) return rc;
    a.rootsift = rootsift != 0;
    const long long blocks = (long long)n * npts;
    if (blocks > Q_MAXBLOCKS) return fail(RR_EINVAL, nm + ": more than 2^24 - 1 keypoint slots");
    if (blocks > 0 && ((!kpts && !lafs) || !desc)) return fail(RR_EINVAL, nm + ": null keypoints or output");
    if (!workspace || workspace_bytes < Q_WS) return fail(RR_ENOSPACE, nm + ": workspace too small");
    if (blocks == 0) return RR_OK;
    const size_t lds = lds_bytes(ps, a.nb * a.ns * a.ns, a.ksize);
    if (u8) {
        rc = want_lds(k_describe<true>, lds, nm);
        if (rc) return rc;
        hipLaunchKernelGGL(k_describe<true>, dim3((unsigned)blocks), dim3(Q_TB), lds, as_stream(stream), x, c, h, w, kpts, count, npts,
                           scale, lafs, orient, orient_bins, a, desc, angles, lafs_out);
    } else {
        rc = want_lds(k_describe<false>, lds, nm);
        if (rc) return rc;
        hipLaunchKernelGGL(k_describe<false>, dim3((unsigned)blocks), dim3(Q_TB), lds, as_stream(stream), x, c, h, w, kpts, count, npts,
                           scale, lafs, orient, orient_bins, a, desc, angles, lafs_out);
    }
    return check_launch("rr_describe_keypoints");
}

}  // extern "C"
