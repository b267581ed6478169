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
// The patch pyramid (pyrdown of cirtorch/geometry/transform/pyramid.py:161-196 and
// extract_patches_from_pyramid of laf.py:311-360): level l + 1 is level l under the 5 x 5 binomial
// blur (reflect padding by 2) and the bilinear halving, which together are one separable 6-tap pass
// [1, 5, 10, 10, 5, 1] / 32 at stride 2 on the plane reflect-padded by 2.  k_pyrdown: one block of
// 256 threads per output tile of 32 x 16; the 68 x 36 input tile goes to LDS once as doubles, even
// and odd columns apart, so that the pass along x reads consecutive doubles (8-byte reads, no bank
// conflict), its result stays in LDS and the pass along y reads that: a level is read once apart
// from the halos, the next is written once, no half-filtered plane exists in memory.  A frame of
// scale s is sampled from level max(0, floor(log2(2 s / ps) + 0.5)), clamped to the last level
// whose smaller side is at least ps, after the frame is renormalised to the level's size.
//
// Bin sums by fixed lanes instead of atomics are what makes a descriptor a function of its patch
// alone: not of the batch, the slot, the launch or the run.
//
// Affine shape (PatchAffineShapeEstimator.forward and LAFAffineShapeEstimator.forward of
// cirtorch/features/affine_shape.py:36-69,91-119, ellipse_to_laf of laf.py:137-177), below the
// describer's kernels and on its helpers: the moments of the Gaussian-weighted Sobel gradients of a
// patch, summed by lane-owned pixels and block_sum; the degenerate rule on the raw moments, then the
// normalisation; the closed-form inverse of the ellipse's square root; and k_laf_shape, one block per
// frame from the upright frame's pyramid patch (LDS) to the rescaled frame.
#include "rr_internal.h"
#include "rr_workspace.h"

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
template <bool U8, typename F>
__device__ __forceinline__ float q_sample(const void* src, long long hw, int h, int w, int gray, const F& f, bool ok,
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

// ---- pyramid levels
struct FrameD { double a00, a01, a02, a10, a11, a12; };

// the level of a frame (laf.py:327-329): max(0, floor(log2(2 s / ps) + 0.5)), s = sqrt(|det + 1e-10|)
__device__ __forceinline__ int q_level(const Frame& f, int ps) {
    const double s = sqrt(fabs(((double)f.a00 * (double)f.a11 - (double)f.a10 * (double)f.a01) + 1e-10));
    const double t = floor(log2((2.0 * s) / (double)ps) + 0.5);
    return t >= 1.0 ? (t > 62.0 ? 62 : (int)t) : 0;   // a NaN: level 0
}

// Patch of frame f -> dst[ps ps] (LDS or global), from the level of f: level 0 is the image (src0),
// level l >= 1 the float32 plane pl of `planes` planes per level in pyr (levels 1 .. last back to
// back, level l of size (h >> l) x (w >> l)); a level past `last` is sampled from `last`.  The frame
// on a level (normalize_laf / denormalize_laf of laf.py:219-257): the centre times (w_l / w, h_l / h),
// the 2 x 2 part times min(h_l, w_l) / min(h, w), float64.  Returns the unclamped level.
template <bool U8>
__device__ __forceinline__ int q_patch(float* __restrict__ dst, const void* src0, long long hw, int h, int w, int gray,
                                       const float* __restrict__ pyr, long long planes, long long pl, int last,
                                       const Frame& f, int ps) {
    const bool ok = f.finite();
    const int lv = ok ? q_level(f, ps) : 0;
    const int l = lv < last ? lv : last;
    if (l <= 0) {
        for (int i = threadIdx.x; i < ps * ps; i += Q_TB) dst[i] = q_sample<U8>(src0, hw, h, w, gray, f, ok, ps, i);
        return lv;
    }
    long long off = 0;
    for (int k = 1; k < l; ++k) off += planes * ((long long)(h >> k) * (long long)(w >> k));
    const int hl = h >> l, wl = w >> l;
    const float* src = pyr + off + pl * ((long long)hl * wl);
    const double m = (double)(hl < wl ? hl : wl) / (double)(h < w ? h : w);
    const double rx = (double)wl / (double)w, ry = (double)hl / (double)h;
    const FrameD g{(double)f.a00 * m, (double)f.a01 * m, (double)f.a02 * rx, (double)f.a10 * m, (double)f.a11 * m, (double)f.a12 * ry};
    for (int i = threadIdx.x; i < ps * ps; i += Q_TB) dst[i] = q_sample<false>(src, 0, hl, wl, 0, g, ok, ps, i);
    return lv;
}

constexpr int P_T = 32, P_TY = 16;       // output tile: 32 wide, 16 tall (28 KiB of LDS: five blocks per CU)
constexpr int P_IN = 2 * P_T + 4;       // input tile with its halo: 68 columns
constexpr int P_INY = 2 * P_TY + 4;     // and 36 rows
constexpr int P_HALF = P_IN / 2;        // even (or odd) columns of an input row: 34

// out[i][j] = sum_a sum_b c6[a] c6[b] xpad[2 i + a][2 j + b], c6 = [1, 5, 10, 10, 5, 1] / 32, xpad the plane
// reflect-padded by 2; along x then along y, each sum in ascending tap order.  One block per tile of
// one plane; gray: the input plane is three planes hw apart reduced on the fly (level 1 of a colour image).
template <bool U8>
__global__ void __launch_bounds__(Q_TB) k_pyrdown(const void* __restrict__ x, int h, int w, int gray, unsigned tiles_x,
                                                  unsigned tiles, float* __restrict__ out) {
    __shared__ double tile[P_INY * P_IN];   // row ly: the even columns, then the odd columns
    __shared__ double mid[P_INY * P_T];     // filtered along x
    const int tid = threadIdx.x;
    const int h2 = h >> 1, w2 = w >> 1;
    const unsigned pl = blockIdx.x / tiles, t = blockIdx.x - pl * tiles;
    const int oy0 = (int)(t / tiles_x) * P_TY, ox0 = (int)(t % tiles_x) * P_T;
    const long long hw = (long long)h * w;
    const long long base = (long long)pl * (gray ? 3 * hw : hw);
#pragma unroll 4
    for (int i = tid; i < P_INY * P_IN; i += Q_TB) {
        const int ly = i / P_IN, r = i - ly * P_IN;
        const int odd = r >= P_HALF, lx = 2 * (r - odd * P_HALF) + odd;
        const long long o = base + (long long)reflect_clampi(2 * oy0 - 2 + ly, h) * w + reflect_clampi(2 * ox0 - 2 + lx, w);
        tile[i] = q_pixel<U8>(x, hw, o, gray);
    }
    __syncthreads();
    const double c0 = 1.0 / 32.0, c1 = 5.0 / 32.0, c2 = 10.0 / 32.0;
    for (int i = tid; i < P_INY * P_T; i += Q_TB) {
        const int ly = i / P_T, ox = i - ly * P_T;
        const double* e = tile + ly * P_IN + ox;
        const double* o = e + P_HALF;
        mid[i] = ((((c0 * e[0] + c1 * o[0]) + c2 * e[1]) + c2 * o[1]) + c1 * e[2]) + c0 * o[2];
    }
    __syncthreads();
    for (int i = tid; i < P_TY * P_T; i += Q_TB) {
        const int oy = i / P_T, ox = i - oy * P_T;
        const int gy = oy0 + oy, gx = ox0 + ox;
        if (gy >= h2 || gx >= w2) continue;
        const double* c = mid + (2 * oy) * P_T + ox;
        const double v = ((((c0 * c[0] + c1 * c[P_T]) + c2 * c[2 * P_T]) + c2 * c[3 * P_T]) + c1 * c[4 * P_T]) + c0 * c[5 * P_T];
        out[(long long)pl * ((long long)h2 * w2) + (long long)gy * w2 + gx] = (float)v;
    }
}

__global__ void k_clear_flag(int* flag) { *flag = 0; }

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
        const int y0 = clampi(y - 1, ps - 1) * ps, y1 = y * ps, y2 = clampi(y + 1, ps - 1) * ps;
        const int x0 = clampi(x - 1, ps - 1), x2 = clampi(x + 1, ps - 1);
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
        const double gx = ((double)L.patch[y * ps + clampi(x + 1, ps - 1)] - (double)L.patch[y * ps + clampi(x - 1, ps - 1)]) * 0.5;
        const double gy = ((double)L.patch[clampi(y + 1, ps - 1) * ps + x] - (double)L.patch[clampi(y - 1, ps - 1) * ps + x]) * 0.5;
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

// the same from the frame's pyramid level; levels_out [n npts] (the unclamped level) and flag may be null
template <bool U8>
__global__ void __launch_bounds__(Q_TB) k_extract_pyr(const void* __restrict__ x, int c, int h, int w, int gray,
                                                      const float* __restrict__ pyr, long long planes, int last,
                                                      const float* __restrict__ lafs, int npts, int ps, float* __restrict__ out,
                                                      int* __restrict__ levels_out, int* __restrict__ flag) {
    const int co = gray ? 1 : c;
    const long long slot = (long long)blockIdx.x / co;
    const int ch = (int)((long long)blockIdx.x - slot * co);
    const long long img = slot / npts, hw = (long long)h * w;
    const long long plane = img * c + ch;
    const void* src = U8 ? (const void*)(reinterpret_cast<const unsigned char*>(x) + plane * hw)
                         : (const void*)(reinterpret_cast<const float*>(x) + plane * hw);
    const float* fp = lafs + slot * 6;
    const Frame f{fp[0], fp[1], fp[2], fp[3], fp[4], fp[5]};
    const int lv = q_patch<U8>(out + (long long)blockIdx.x * ps * ps, src, hw, h, w, gray, pyr, planes, img * co + ch, last, f, ps);
    if (threadIdx.x == 0 && ch == 0) {
        if (levels_out) levels_out[slot] = lv;
        if (flag && lv > last) *flag = 1;   // every writer stores the same value
    }
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

// one block per keypoint slot.  PYR: every patch comes from the pyramid level of the frame it is
// sampled from (q_patch; pyr holds levels 1 .. last of the n gray planes), which is what keeps the
// chain through rr_extract_patches_pyramid bit-identical; without PYR pyr, n and last are unused.
template <bool U8, bool PYR>
__global__ void __launch_bounds__(Q_TB) k_describe(const void* __restrict__ x, int c, int h, int w, const float* __restrict__ kpts,
                                                   const int* __restrict__ count, int npts, double scale,
                                                   const float* __restrict__ lafs, int orient, int obins, SiftArgs a,
                                                   float* __restrict__ desc, float* __restrict__ angles,
                                                   float* __restrict__ lafs_out, const float* __restrict__ pyr, int n, int last) {
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
        if constexpr (PYR) {
            q_patch<U8>(L.patch, src, hw, h, w, gray, pyr, n, img, last, f, ps);
        } else {
            const bool ok = f.finite();
            for (int i = tid; i < ps * ps; i += Q_TB) L.patch[i] = q_sample<U8>(src, hw, h, w, gray, f, ok, ps, i);
        }
        __syncthreads();
        ang = orient_phase(L, ps, obins);
        // upright . [[cos, sin], [-sin, cos]] (LAFOrienter's product), rounded once to float32
        const double cs = cos((double)ang), sn = sin((double)ang);
        f.a00 = (float)(u00 * cs);
        f.a01 = (float)(u00 * sn);
        f.a10 = (float)(u10 * cs - u11 * sn);
        f.a11 = (float)(u10 * sn + u11 * cs);
    }
    if constexpr (PYR) {
        q_patch<U8>(L.patch, src, hw, h, w, gray, pyr, n, img, last, f, ps);
    } else {
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

// ---- affine shape (PatchAffineShapeEstimator, ellipse_to_laf, LAFAffineShapeEstimator)
// The block's LDS of the shape kernels: 832 bytes of tables and the patch (4 ps^2: 16 KiB at ps 64).
struct ShapeLds {
    double* scratch;   // [64] the unnormalised 1-D Gaussian
    double* red;       // [8]  wave sums of a block reduction
    float* g1;         // [64] 1-D Gaussian
    float* patch;      // [ps ps]
};

__host__ __device__ inline size_t shape_lds_bytes(int ps) { return (64 + 8) * 8 + 64 * 4 + (size_t)ps * ps * 4; }

__device__ __forceinline__ ShapeLds shape_carve(unsigned char* base) {
    ShapeLds L;
    L.scratch = reinterpret_cast<double*>(base);
    L.red = L.scratch + 64;
    L.g1 = reinterpret_cast<float*>(L.red + 8);
    L.patch = L.g1 + 64;
    return L;
}

// g1 of sift_phase, by its expressions in its order (the same bits): the window of both is
// get_gaussian_kernel2d((ps, ps), (sigma, sigma), True), sigma = ps / sqrt 2
__device__ __forceinline__ void gauss_table(const ShapeLds& L, int ps) {
    const int tid = threadIdx.x;
    if (tid < ps) {
        const double x = (double)(tid - ps / 2) + ((ps & 1) ? 0.0 : 0.5);
        L.scratch[tid] = exp(-(x * x) / ((double)ps * (double)ps));   // 2 sigma^2 = ps^2
    }
    __syncthreads();
    if (tid < ps) {
        double s = 0.0;
        for (int i = 0; i < ps; ++i) s += L.scratch[i];
        L.g1[tid] = (float)(L.scratch[tid] / s);
    }
    __syncthreads();
}

// The normalised second-moment matrix (a, b, c) of L.patch, float32, returned to every thread.
// Lane t owns the pixels t, t + 256, ... and adds their gx^2, gx gy, gy^2 in ascending order; the 256
// sums are combined by block_sum: a butterfly over the wave, the four waves ascending.
__device__ void shape_phase(const ShapeLds& L, int ps, double eps, float& fa, float& fb, float& fc) {
    const int n = ps * ps;
    double sa = 0.0, sb = 0.0, sc = 0.0;
    for (int i = threadIdx.x; i < n; i += Q_TB) {
        const int y = i / ps, x = i - y * ps;
        const int y0 = clampi(y - 1, ps - 1) * ps, y1 = y * ps, y2 = clampi(y + 1, ps - 1) * ps;
        const int x0 = clampi(x - 1, ps - 1), x2 = clampi(x + 1, ps - 1);
        const double a00 = L.patch[y0 + x0], a01 = L.patch[y0 + x], a02 = L.patch[y0 + x2];
        const double a10 = L.patch[y1 + x0], a12 = L.patch[y1 + x2];
        const double a20 = L.patch[y2 + x0], a21 = L.patch[y2 + x], a22 = L.patch[y2 + x2];
        const double dx = ((a02 - a00) + 2.0 * (a12 - a10) + (a22 - a20)) * 0.125;
        const double dy = ((a20 - a00) + 2.0 * (a21 - a01) + (a22 - a02)) * 0.125;
        const double g = (double)(L.g1[y] * L.g1[x]);
        const double gx = dx * g, gy = dy * g;   // the weight on the gradients: squared in the moments
        sa += gx * gx;
        sb += gx * gy;
        sc += gy * gy;
    }
    double a = block_sum(sa, L.red) / (double)n;
    double b = block_sum(sb, L.red) / (double)n;
    double c = block_sum(sc, L.red) / (double)n;
    if ((a < eps) + (b < eps) + (c < eps) >= 2) { a = 1.0; b = 0.0; c = 1.0; }   // before the normalisation
    double m = a;
    if (b > m || b != b) m = b;
    if (c > m || c != c) m = c;
    fa = (float)(a / m);
    fb = (float)(b / m);
    fc = (float)(c / m);
}

// ellipse (x, y, a, b, c) -> frame o[6]
__device__ __forceinline__ void q_ellipse(float x, float y, float a, float b, float c, float* o) {
    const double a11 = sqrt(fabs((double)a)), a22 = sqrt(fabs((double)c));
    const double d = a11 + a22;
    const double a21 = (double)b / (d < 1e-9 ? 1e-9 : d);
    o[0] = (float)(1.0 / a11);
    o[1] = 0.f;
    o[2] = x;
    o[3] = (float)(0.0 - a21 / (a11 * a22));
    o[4] = (float)(1.0 / a22);
    o[5] = y;
}

__device__ __forceinline__ double q_scale(double a00, double a01, double a10, double a11) {
    return sqrt(fabs((a00 * a11 - a10 * a01) + 1e-10));
}

__global__ void __launch_bounds__(Q_TB) k_patch_shape(const float* __restrict__ patches, int ps, double eps, float* __restrict__ out) {
    const ShapeLds L = shape_carve(q_lds);
    const float* src = patches + (long long)blockIdx.x * ps * ps;
    for (int i = threadIdx.x; i < ps * ps; i += Q_TB) L.patch[i] = src[i];
    gauss_table(L, ps);
    float a, b, c;
    shape_phase(L, ps, eps, a, b, c);
    if (threadIdx.x == 0) {
        float* o = out + (long long)blockIdx.x * 3;
        o[0] = a; o[1] = b; o[2] = c;
    }
}

__global__ void __launch_bounds__(Q_TB) k_ellipse_to_laf(const float* __restrict__ ells, long long B, float* __restrict__ lafs) {
    const long long i = (long long)blockIdx.x * Q_TB + threadIdx.x;
    if (i >= B) return;
    const float* e = ells + i * 5;
    float o[6];
    q_ellipse(e[0], e[1], e[2], e[3], e[4], o);
    for (int k = 0; k < 6; ++k) lafs[i * 6 + k] = o[k];
}

// one block per keypoint slot: upright frame -> its pyramid patch (LDS) -> shape -> ellipse frame of
// the input frame's scale.  lafs_out may be lafs: a block reads its own frame before it writes it.
template <bool U8>
__global__ void __launch_bounds__(Q_TB) k_laf_shape(const void* __restrict__ x, int c, int h, int w, const float* lafs,
                                                    const int* __restrict__ count, int npts, int ps, double eps, float* lafs_out,
                                                    const float* __restrict__ pyr, int n, int last) {
    const int tid = threadIdx.x;
    const long long slot = blockIdx.x, img = slot / npts;
    const int pt = (int)(slot - img * npts);
    const float* fp = lafs + slot * 6;
    const Frame f{fp[0], fp[1], fp[2], fp[3], fp[4], fp[5]};
    if ((count && pt >= count[img]) || (f.a02 == -1.f && f.a12 == -1.f) || !f.finite()) {   // block-uniform
        __syncthreads();   // every thread has read the frame (lafs_out may be lafs)
        if (tid < 6) lafs_out[slot * 6 + tid] = 0.f;
        return;
    }
    const ShapeLds L = shape_carve(q_lds);
    const long long hw = (long long)h * w;
    const void* src = U8 ? (const void*)(reinterpret_cast<const unsigned char*>(x) + img * c * hw)
                         : (const void*)(reinterpret_cast<const float*>(x) + img * c * hw);
    double u00, u10, u11;
    q_upright(f, u00, u10, u11);
    const Frame u{(float)u00, 0.f, f.a02, (float)u10, (float)u11, f.a12};
    q_patch<U8>(L.patch, src, hw, h, w, c == 3, pyr, n, img, last, u, ps);
    gauss_table(L, ps);
    float a, b, cc;
    shape_phase(L, ps, eps, a, b, cc);   // its barriers are also between the reads of lafs and the write below
    if (tid == 0) {
        float e[6];
        q_ellipse(f.a02, f.a12, a, b, cc, e);
        const double s0 = q_scale(f.a00, f.a01, f.a10, f.a11), s1 = q_scale(e[0], e[1], e[3], e[4]);
        const double r = s0 / s1;
        float* o = lafs_out + slot * 6;
        o[0] = (float)((double)e[0] * r); o[1] = (float)((double)e[1] * r); o[2] = f.a02;
        o[3] = (float)((double)e[3] * r); o[4] = (float)((double)e[4] * r); o[5] = f.a12;
    }
}

// ---------------------------------------------------------------- host
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

// bytes of levels 1 .. last of n c planes of h x w (level l is (h >> l) x (w >> l): floor(h / 2) repeated),
// last = the largest l with min(h_l, w_l) >= ps, 0 when there is none or an argument is out of range
size_t pyramid_bytes(int n, int c, int h, int w, int ps, int& last) {
    last = 0;
    if (n < 1 || c < 1 || h < 1 || w < 1 || ps < Q_MINPS || ps > Q_MAXPS || !q_pixels_ok(n, c, h, w)) return 0;
    size_t px = 0;
    for (int l = 1; l < 31 && ((h >> l) < (w >> l) ? (h >> l) : (w >> l)) >= ps; ++l) {
        px += (size_t)(h >> l) * (size_t)(w >> l);
        last = l;
    }
    return px * (size_t)n * (size_t)c * sizeof(float);
}

// one level: planes of h x w (gray: planes images of three channels) -> planes of (h / 2) x (w / 2)
int launch_pyrdown(const std::string& nm, const void* x, long long planes, int h, int w, bool u8, bool gray, float* out,
                   hipStream_t s) {
    const int h2 = h >> 1, w2 = w >> 1;
    const unsigned tiles_x = (unsigned)((w2 + P_T - 1) / P_T), tiles = tiles_x * (unsigned)((h2 + P_TY - 1) / P_TY);
    const long long blocks = planes * (long long)tiles;
    if (blocks > Q_MAXBLOCKS) return fail(RR_EINVAL, nm + ": more than 2^24 - 1 output tiles");
    if (u8)
        hipLaunchKernelGGL(k_pyrdown<true>, dim3((unsigned)blocks), dim3(Q_TB), 0, s, x, h, w, (int)gray, tiles_x, tiles, out);
    else
        hipLaunchKernelGGL(k_pyrdown<false>, dim3((unsigned)blocks), dim3(Q_TB), 0, s, x, h, w, (int)gray, tiles_x, tiles, out);
    return RR_OK;
}

// levels 1 .. last into pyr, back to back; level 1 reads the image, level l + 1 reads level l
int build_pyramid(const std::string& nm, const void* x, int n, int c, int h, int w, bool u8, bool gray, int last, float* pyr,
                  hipStream_t s) {
    const long long planes = (long long)n * (gray ? 1 : c);
    const void* src = x;
    float* dst = pyr;
    for (int l = 1; l <= last; ++l) {
        const int rc = launch_pyrdown(nm, src, planes, h >> (l - 1), w >> (l - 1), l == 1 && u8, l == 1 && gray, dst, s);
        if (rc) return rc;
        src = dst;
        dst += planes * ((long long)(h >> l) * (long long)(w >> l));
    }
    return RR_OK;
}

// the describe entries and rr_laf_affine_shape: no patch, gradient or plane lives in memory, only
// (pyramid) the gray levels 1 .. last, first in the workspace
struct DescribeWs {
    float* pyr;
    int last;
};

DescribeWs layout(Arena& a, bool pyramid, int n, int h, int w, int ps) {
    int last = 0;
    const size_t bytes = pyramid ? pyramid_bytes(n, 1, h, w, ps, last) : 0;
    return {a.take<float>(bytes / sizeof(float)), last};
}

}  // namespace

}  // namespace rr

using namespace rr;

extern "C" {

size_t rr_describe_workspace_bytes(int n, int npts, int ps, int num_ang_bins, int num_spatial_bins) {
    (void)npts; (void)num_ang_bins; (void)num_spatial_bins;
    return measured(layout, false, n, 0, 0, ps);
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

// both describe entries: pyramid = the levels are built at the start of the workspace first
static int describe(const std::string& nm, bool pyramid, const void* x, int n, int c, int h, int w, int u8, const float* kpts,
                    const int* count, int npts, double scale, const float* lafs, int orient, int orient_bins, int ps,
                    int num_ang_bins, int num_spatial_bins, int rootsift, double clipval, float* desc, float* angles,
                    float* lafs_out, void* workspace, size_t workspace_bytes, void* stream) {
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
    Arena arena(workspace, workspace_bytes);
    const auto [pyr, last] = layout(arena, pyramid, n, h, w, ps);
    if (!workspace || !arena.fits()) return fail(RR_ENOSPACE, nm + ": workspace too small");
    if (blocks == 0) return RR_OK;
    if (last > 0) {
        rc = build_pyramid(nm, x, n, c, h, w, u8 != 0, c == 3, last, pyr, as_stream(stream));
        if (rc) return rc;
    }
    const size_t lds = lds_bytes(ps, a.nb * a.ns * a.ns, a.ksize);
    const dim3 grid((unsigned)blocks), block(Q_TB);
#define RR_DESCRIBE(U8, PYR)                                                                                          \
    do {                                                                                                              \
        rc = want_lds(k_describe<U8, PYR>, lds, nm);                                                                  \
        if (rc) return rc;                                                                                            \
        hipLaunchKernelGGL((k_describe<U8, PYR>), grid, block, lds, as_stream(stream), x, c, h, w, kpts, count, npts, \
                           scale, lafs, orient, orient_bins, a, desc, angles, lafs_out, pyr, n, last);               \
    } while (0)
    if (pyramid) {
        if (u8) RR_DESCRIBE(true, true); else RR_DESCRIBE(false, true);
    } else {
        if (u8) RR_DESCRIBE(true, false); else RR_DESCRIBE(false, false);
    }
#undef RR_DESCRIBE
    return check_launch(nm.c_str());
}

int rr_describe_keypoints(const void* x, int n, int c, int h, int w, int u8, const float* kpts, const int* count, int npts,
                          double scale, const float* lafs, int orient, int orient_bins, int ps, int num_ang_bins,
                          int num_spatial_bins, int rootsift, double clipval, float* desc, float* angles, float* lafs_out,
                          void* workspace, size_t workspace_bytes, void* stream) {
    return describe("rr_describe_keypoints", false, x, n, c, h, w, u8, kpts, count, npts, scale, lafs, orient, orient_bins, ps,
                    num_ang_bins, num_spatial_bins, rootsift, clipval, desc, angles, lafs_out, workspace, workspace_bytes, stream);
}

size_t rr_describe_pyramid_workspace_bytes(int n, int c, int h, int w, int npts, int ps, int num_ang_bins, int num_spatial_bins) {
    (void)c; (void)npts; (void)num_ang_bins; (void)num_spatial_bins;
    return measured(layout, true, n, h, w, ps);
}

int rr_describe_keypoints_pyramid(const void* x, int n, int c, int h, int w, int u8, const float* kpts, const int* count,
                                  int npts, double scale, const float* lafs, int orient, int orient_bins, int ps,
                                  int num_ang_bins, int num_spatial_bins, int rootsift, double clipval, float* desc,
                                  float* angles, float* lafs_out, void* workspace, size_t workspace_bytes, void* stream) {
    return describe("rr_describe_keypoints_pyramid", true, x, n, c, h, w, u8, kpts, count, npts, scale, lafs, orient, orient_bins,
                    ps, num_ang_bins, num_spatial_bins, rootsift, clipval, desc, angles, lafs_out, workspace, workspace_bytes,
                    stream);
}

size_t rr_patch_pyramid_bytes(int n, int c, int h, int w, int ps, int* last_level) {
    int last = 0;
    const size_t b = pyramid_bytes(n, c, h, w, ps, last);
    if (last_level) *last_level = last;
    return b;
}

int rr_pyrdown(const float* x, int n, int c, int h, int w, float* out, void* stream) {
    const std::string nm("rr_pyrdown");
    int rc = check_image(nm, x, n, c, h, w);
    if (rc) return rc;
    if (h < 3 || w < 3) return fail(RR_EINVAL, nm + ": h and w must be at least 3 (reflect padding by 2)");
    if (n > 0 && !out) return fail(RR_EINVAL, nm + ": null output");
    if (n == 0) return RR_OK;
    rc = launch_pyrdown(nm, x, (long long)n * c, h, w, false, false, out, as_stream(stream));
    return rc ? rc : check_launch("rr_pyrdown");
}

int rr_patch_pyramid(const void* x, int n, int c, int h, int w, int u8, int gray, int ps, float* pyr, size_t pyr_bytes,
                     void* stream) {
    const std::string nm("rr_patch_pyramid");
    int rc = check_image(nm, x, n, c, h, w);
    if (rc) return rc;
    if (gray != 0 && gray != 1) return fail(RR_EINVAL, nm + ": gray must be 0 or 1");
    if (gray && c != 3) return fail(RR_EINVAL, nm + ": gray needs c == 3");
    if (ps < Q_MINPS || ps > Q_MAXPS) return fail(RR_EINVAL, nm + ": patch size outside [8, 64]");
    int last = 0;
    const size_t need = pyramid_bytes(n, gray ? 1 : c, h, w, ps, last);
    if (need > 0 && !pyr) return fail(RR_EINVAL, nm + ": null pyramid buffer");
    if (pyr_bytes < need) return fail(RR_ENOSPACE, nm + ": pyramid buffer too small");
    if (need == 0) return RR_OK;
    rc = build_pyramid(nm, x, n, c, h, w, u8 != 0, gray != 0, last, pyr, as_stream(stream));
    return rc ? rc : check_launch("rr_patch_pyramid");
}

int rr_extract_patches_pyramid(const void* x, int n, int c, int h, int w, int u8, int gray, const float* pyr, const float* lafs,
                               int npts, int ps, float* out, int* levels_out, int* beyond_flag, void* stream) {
    const std::string nm("rr_extract_patches_pyramid");
    int rc = check_image(nm, x, n, c, h, w);
    if (rc) return rc;
    if (gray != 0 && gray != 1) return fail(RR_EINVAL, nm + ": gray must be 0 or 1");
    if (gray && c != 3) return fail(RR_EINVAL, nm + ": gray needs c == 3");
    if (npts < 0) return fail(RR_EINVAL, nm + ": negative npts");
    if (ps < Q_MINPS || ps > Q_MAXPS) return fail(RR_EINVAL, nm + ": patch size outside [8, 64]");
    const int co = gray ? 1 : c;
    const long long blocks = (long long)n * npts * co;
    if (blocks > Q_MAXBLOCKS) return fail(RR_EINVAL, nm + ": more than 2^24 - 1 patches");
    if (blocks > 0 && (!lafs || !out)) return fail(RR_EINVAL, nm + ": null frames or output");
    int last = 0;
    const size_t need = pyramid_bytes(n, co, h, w, ps, last);
    if (blocks > 0 && need > 0 && !pyr) return fail(RR_EINVAL, nm + ": null pyramid buffer");
    if (blocks == 0 && !beyond_flag) return RR_OK;
    hipStream_t s = as_stream(stream);
    // the flag is reset by a kernel, not hipMemsetAsync (captured memset nodes: DESIGN.md §4, kNN)
    if (beyond_flag) hipLaunchKernelGGL(k_clear_flag, dim3(1), dim3(1), 0, s, beyond_flag);
    if (blocks > 0) {
        const long long planes = (long long)n * co;
        if (u8)
            hipLaunchKernelGGL(k_extract_pyr<true>, dim3((unsigned)blocks), dim3(Q_TB), 0, s, x, c, h, w, gray, pyr, planes, last, lafs,
                               npts, ps, out, levels_out, beyond_flag);
        else
            hipLaunchKernelGGL(k_extract_pyr<false>, dim3((unsigned)blocks), dim3(Q_TB), 0, s, x, c, h, w, gray, pyr, planes, last, lafs,
                               npts, ps, out, levels_out, beyond_flag);
    }
    return check_launch("rr_extract_patches_pyramid");
}

int rr_patch_affine_shape(const float* patches, long long B, int ps, double eps, float* out, void* stream) {
    const std::string nm("rr_patch_affine_shape");
    if (B < 0 || B > Q_MAXBLOCKS) return fail(RR_EINVAL, nm + ": patch count outside [0, 2^24)");
    if (ps < Q_MINPS || ps > Q_MAXPS) return fail(RR_EINVAL, nm + ": patch size outside [8, 64]");
    if (!std::isfinite(eps)) return fail(RR_EINVAL, nm + ": eps must be finite");
    if (B > 0 && (!patches || !out)) return fail(RR_EINVAL, nm + ": null input or output");
    if (B == 0) return RR_OK;
    hipLaunchKernelGGL(k_patch_shape, dim3((unsigned)B), dim3(Q_TB), shape_lds_bytes(ps), as_stream(stream), patches, ps, eps, out);
    return check_launch("rr_patch_affine_shape");
}

int rr_ellipse_to_laf(const float* ells, long long B, float* lafs, void* stream) {
    const std::string nm("rr_ellipse_to_laf");
    if (B < 0 || B > Q_MAXBLOCKS) return fail(RR_EINVAL, nm + ": ellipse count outside [0, 2^24)");
    if (B > 0 && (!ells || !lafs)) return fail(RR_EINVAL, nm + ": null input or output");
    if (B == 0) return RR_OK;
    hipLaunchKernelGGL(k_ellipse_to_laf, dim3((unsigned)((B + Q_TB - 1) / Q_TB)), dim3(Q_TB), 0, as_stream(stream), ells, B, lafs);
    return check_launch("rr_ellipse_to_laf");
}

size_t rr_laf_affine_shape_workspace_bytes(int n, int c, int h, int w, int npts, int ps) {
    (void)c; (void)npts;
    return measured(layout, true, n, h, w, ps);
}

int rr_laf_affine_shape(const void* x, int n, int c, int h, int w, int u8, const float* lafs, const int* count, int npts, int ps,
                        double eps, float* lafs_out, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string nm("rr_laf_affine_shape");
    if (c != 1 && c != 3) return fail(RR_EINVAL, nm + ": c must be 1 or 3");
    int rc = check_image(nm, x, n, c, h, w);
    if (rc) return rc;
    if (npts < 0) return fail(RR_EINVAL, nm + ": negative npts");
    if (ps < Q_MINPS || ps > Q_MAXPS) return fail(RR_EINVAL, nm + ": patch size outside [8, 64]");
    if (!std::isfinite(eps)) return fail(RR_EINVAL, nm + ": eps must be finite");
    const long long blocks = (long long)n * npts;
    if (blocks > Q_MAXBLOCKS) return fail(RR_EINVAL, nm + ": more than 2^24 - 1 keypoint slots");
    if (blocks > 0 && (!lafs || !lafs_out)) return fail(RR_EINVAL, nm + ": null frames or output");
    Arena arena(workspace, workspace_bytes);
    const auto [pyr, last] = layout(arena, true, n, h, w, ps);
    if (!workspace || !arena.fits()) return fail(RR_ENOSPACE, nm + ": workspace too small");
    if (blocks == 0) return RR_OK;
    if (last > 0) {
        rc = build_pyramid(nm, x, n, c, h, w, u8 != 0, c == 3, last, pyr, as_stream(stream));
        if (rc) return rc;
    }
    const size_t lds = shape_lds_bytes(ps);
    if (u8)
        hipLaunchKernelGGL(k_laf_shape<true>, dim3((unsigned)blocks), dim3(Q_TB), lds, as_stream(stream), x, c, h, w, lafs, count,
                           npts, ps, eps, lafs_out, pyr, n, last);
    else
        hipLaunchKernelGGL(k_laf_shape<false>, dim3((unsigned)blocks), dim3(Q_TB), lds, as_stream(stream), x, c, h, w, lafs, count,
                           npts, ps, eps, lafs_out, pyr, n, last);
    return check_launch("rr_laf_affine_shape");
}

}  // extern "C"
