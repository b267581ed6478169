// librr.so — scale-space keypoint detection: Gaussian blur, the scale pyramid, the difference of
// Gaussians, strict 3-D extrema with a quadratic sub-voxel refinement, local affine frames and the
// best N frames per image over all octaves.
// Replaces, on the device, gaussian_blur2d of cirtorch/filters/gaussian.py:8-16 (filter2D of
// cirtorch/filters/filter.py:34-77, get_gaussian_kernel1d of cirtorch/filters/kernels.py:26-35,481-492),
// ScalePyramid.forward of cirtorch/geometry/transform/pyramid.py:30-158, dog_response of
// cirtorch/features/responses.py:106-115, nms3d(x, (3, 3, 3)) of cirtorch/features/nms.py:70-108,
// conv_quad_interp3d of cirtorch/geometry/subpix/spatial_soft_argmax.py:348-411 (spatial_gradient3d of
// cirtorch/filters/sobel.py:48-78) and ScaleSpaceDetector.detect of
// cirtorch/features/scale_space_detector.py:85-161 (laf_is_inside_image, normalize_laf and
// denormalize_laf of cirtorch/features/laf.py).  include/rr.h states every rule.
//
// Everything is float64 on float32 values, every sum has one fixed order, each stored value is
// rounded once, no atomic touches a floating-point value and nothing waits for the host.  The kernels:
//
//   k_blur      one block of 256 threads per T x T tile of one plane (T = 32, or 16 for more than 43
//               taps).  The tile and a halo of ksize / 2 at reflected coordinates go to LDS as
//               doubles, the blur along x of every tile row and halo row goes to a second LDS array,
//               the blur along y reads that: a plane is read once apart from the halos and written
//               once, the x-blurred plane never exists in memory.  The taps are kernel arguments.
//               Rows of 32 (or two rows of 16) consecutive doubles per 32-lane group: every LDS read
//               is 8 bytes wide and free of bank conflicts (the 16-wide tile pads its row stride to
//               16 mod 32 doubles).
//               The pyramid keeps its working levels in float64 (three rotating planes per image in
//               the workspace): a level is blurred from the unrounded previous level, and each
//               float32 level handed out is rounded once from it.
//   k_down      the even pixels of a working level: the next octave's first level.
//   k_dog       level[l + 1] - level[l].
//   k_extrema   the dense form: mask, offsets and refined value of every voxel of a volume.
//   k_ss_candidates  one thread per voxel of one octave: the strict-extremum test, the refinement,
//               the frame and its inside test; the 64-bit key (orderable bits of the refined value
//               << 32 | ~(octave base + voxel index)) of a kept frame is collected in LDS and the
//               block appends its keys to the image's list with one integer atomic.
//   k_ss_select one block of 1024 threads per image: select_sorted (rr_select.h) on the image's keys
//               of all octaves, then the refinement and the frame of each selected voxel again --
//               the same device function on the same values gives the same bits -- written as LAF,
//               score; the slots past count hold a zero frame and 0.
#include "rr_internal.h"
#include "rr_select.h"
#include "rr_workspace.h"

#include <math.h>

#pragma clang fp contract(off)

namespace rr {

namespace {

constexpr int S_TB = 256;
constexpr int S_MAXK = 63;           // taps
constexpr int S_MAXLEVELS = 8;       // levels per octave doubling of sigma
constexpr int S_MAXL = S_MAXLEVELS + 3;
constexpr int S_MAXO = 16;           // octaves
constexpr long long S_MAXPIX = 1ll << 31;

struct Taps { float t[S_MAXK]; };

// reflect_clampi: |overshoot| < size for every coordinate an in-map output reads; coordinates that
// only outputs outside the map read are clamped
// IN: 0 float32, 1 uint8 (/ 255 in IEEE float32), 2 float64
template <int IN> __device__ __forceinline__ double load_in(const void* x, long long i) {
    if constexpr (IN == 1)
        return (double)((float)reinterpret_cast<const unsigned char*>(x)[i] / 255.f);
    else if constexpr (IN == 2)
        return reinterpret_cast<const double*>(x)[i];
    else
        return (double)reinterpret_cast<const float*>(x)[i];
}

template <int IN>
__global__ void __launch_bounds__(S_TB) k_blur(const void* __restrict__ x, int h, int w, int gray, Taps taps, int ks, int T,
                                               int stride, unsigned tiles_x, unsigned tiles, long long in_ps, long long outf_ps,
                                               long long outd_ps, float* __restrict__ outf, double* __restrict__ outd) {
    extern __shared__ __align__(16) double s_lds[];
    const int tid = threadIdx.x;
    const int p = ks / 2, side = T + 2 * p;
    double* tile = s_lds;                       // [side][stride], origin (ty0 - p, tx0 - p)
    double* mid = s_lds + (size_t)side * stride;   // [side][T]: blurred along x
    const unsigned pl = blockIdx.x / tiles, t = blockIdx.x - pl * tiles;
    const int ty0 = (int)(t / tiles_x) * T, tx0 = (int)(t % tiles_x) * T;
    const long long hw = (long long)h * w;
    const long long src = (long long)pl * in_ps;   // plane strides in elements: in_ps, outf_ps, outd_ps

    for (int i = tid; i < side * side; i += S_TB) {
        const int ly = i / side, lx = i - ly * side;
        const long long o = src + (long long)reflect_clampi(ty0 - p + ly, h) * w + reflect_clampi(tx0 - p + lx, w);
        double v;
        if (gray)
            v = (0.299 * load_in<IN>(x, o) + 0.587 * load_in<IN>(x, hw + o)) + 0.114 * load_in<IN>(x, 2 * hw + o);
        else
            v = load_in<IN>(x, o);
        tile[ly * stride + lx] = v;
    }
    __syncthreads();
    for (int i = tid; i < side * T; i += S_TB) {
        const int ly = i / T, ox = i - ly * T;
        const double* row = tile + ly * stride + ox;
        double a = 0.0;
        for (int d = 0; d < ks; ++d) a += (double)taps.t[d] * row[d];
        mid[ly * T + ox] = a;
    }
    __syncthreads();
    for (int i = tid; i < T * T; i += S_TB) {
        const int oy = i / T, ox = i - oy * T;
        const int gy = ty0 + oy, gx = tx0 + ox;
        if (gy >= h || gx >= w) continue;
        double a = 0.0;
        for (int d = 0; d < ks; ++d) a += (double)taps.t[d] * mid[(oy + d) * T + ox];
        const long long o = (long long)gy * w + gx;
        if (outf) outf[(long long)pl * outf_ps + o] = (float)a;
        if (outd) outd[(long long)pl * outd_ps + o] = a;
    }
}

__global__ void __launch_bounds__(S_TB) k_down(const double* __restrict__ x, int h, int w, int h2, int w2, long long total,
                                               long long outf_ps, double* __restrict__ outd, float* __restrict__ outf) {
    const long long i = (long long)blockIdx.x * S_TB + threadIdx.x;
    if (i >= total) return;
    const long long hw2 = (long long)h2 * w2;
    const long long pl = i / hw2;
    const int r = (int)(i - pl * hw2), y = r / w2, xx = r - y * w2;
    const double v = x[pl * ((long long)h * w) + (long long)(2 * y) * w + 2 * xx];
    outd[i] = v;
    outf[pl * outf_ps + r] = (float)v;
}

struct SigTab { float s[S_MAXL]; };

__global__ void __launch_bounds__(S_TB) k_fill_sigmas(float* __restrict__ out, int n, int L, SigTab tab) {
    const int i = blockIdx.x * S_TB + threadIdx.x;
    if (i < n * L) out[i] = tab.s[i % L];
}

// out[b][l] = x[b][l + 1] - x[b][l], l < L - 1; planes of image b start at b * istride / b * ostride
__global__ void __launch_bounds__(S_TB) k_dog(const float* __restrict__ x, int L, long long hw, long long istride,
                                              long long ostride, long long total, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * S_TB + threadIdx.x;
    if (i >= total) return;
    const long long per = (long long)(L - 1) * hw;
    const long long b = i / per, r = i - b * per;
    out[b * ostride + r] = x[b * istride + r + hw] - x[b * istride + r];
}

// ---------------------------------------------------------------- extrema
// sin and cos of the float32 values linspace(0, 2 pi, 11), as float32: the boundary points of
// laf_to_boundary_points(laf, 12) after the centre
__device__ const double S_SIN[11] = {0x0.0p+0, 0x1.2cf23p-1, 0x1.e6f0e2p-1, 0x1.e6f0ep-1, 0x1.2cf22ep-1, -0x1.777a5cp-24,
                                     -0x1.2cf234p-1, -0x1.e6f0ep-1, -0x1.e6f0ep-1, -0x1.2cf226p-1, 0x1.777a5cp-23};
__device__ const double S_COS[11] = {0x1.0p+0, 0x1.9e377ap-1, 0x1.3c6ef2p-2, -0x1.3c6ef6p-2, -0x1.9e377ap-1, -0x1.0p+0,
                                     -0x1.9e3778p-1, -0x1.3c6efap-2, 0x1.3c6efcp-2, 0x1.9e3782p-1, 0x1.0p+0};

// +1: a strict maximum, -1 (minima only): a strict minimum, 0: neither.  v: one image's [D][h][w].
__device__ __forceinline__ int ss_peak(const float* __restrict__ v, int D, int h, int w, int d, int y, int x, int minima) {
    // a clamped neighbour of a face voxel is the voxel itself, which fails the strict comparison
    if (d < 1 || y < 1 || x < 1 || d > D - 2 || y > h - 2 || x > w - 2) return 0;
    const long long hw = (long long)h * w;
    const float* c = v + d * hw + (long long)y * w + x;
    const float cv = *c;
    float sg;
    if (cv > 0.f) sg = 1.f;
    else if (minima && -cv > 0.f) sg = -1.f;
    else return 0;   // 0 and NaN
    const float m = sg * cv;
    for (int dd = -1; dd <= 1; ++dd)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx)
                if ((dd | dy | dx) != 0 && !(m > sg * c[dd * hw + dy * w + dx])) return 0;
    return sg > 0.f ? 1 : -1;
}

// x = -H^-1 b by elimination with partial pivoting; false for a singular or non-finite system
__device__ __forceinline__ bool ss_solve3(double A[3][3], double b[3], double x[3]) {
    for (int c = 0; c < 3; ++c) {
        int pv = c;
        for (int r = c + 1; r < 3; ++r)
            if (fabs(A[r][c]) > fabs(A[pv][c])) pv = r;
        if (!(fabs(A[pv][c]) > 0.0)) return false;
        if (pv != c) {
            for (int k = 0; k < 3; ++k) { const double t = A[c][k]; A[c][k] = A[pv][k]; A[pv][k] = t; }
            const double t = b[c]; b[c] = b[pv]; b[pv] = t;
        }
        for (int r = c + 1; r < 3; ++r) {
            const double f = A[r][c] / A[c][c];
            for (int k = c; k < 3; ++k) A[r][k] -= f * A[c][k];
            b[r] -= f * b[c];
        }
    }
    x[2] = b[2] / A[2][2];
    x[1] = (b[1] - A[1][2] * x[2]) / A[1][1];
    x[0] = ((b[0] - A[0][1] * x[1]) - A[0][2] * x[2]) / A[0][0];
    for (int k = 0; k < 3; ++k) {
        x[k] = -x[k];
        if (!(fabs(x[k]) <= 1.7976931348623157e308)) return false;
    }
    return true;
}

// The refinement of an interior voxel of sg * v: off = (ox, oy, os), the refined value.
__device__ __forceinline__ double ss_refine(const float* __restrict__ v, int h, int w, int d, int y, int x, double sg,
                                            double off[3]) {
    const long long hw = (long long)h * w;
    const float* c = v + d * hw + (long long)y * w + x;
#define SP(dd, dy, dx) (sg * (double)c[(dd) * hw + (dy) * w + (dx)])
    const double cv = SP(0, 0, 0);
    double b[3] = {0.5 * (SP(0, 0, 1) - SP(0, 0, -1)), 0.5 * (SP(0, 1, 0) - SP(0, -1, 0)), 0.5 * (SP(-1, 0, 0) - SP(1, 0, 0))};
    const double g[3] = {b[0], b[1], b[2]};
    const double dxx = (SP(0, 0, -1) + SP(0, 0, 1)) - 2.0 * cv;
    const double dyy = (SP(0, -1, 0) + SP(0, 1, 0)) - 2.0 * cv;
    const double dss = (SP(-1, 0, 0) + SP(1, 0, 0)) - 2.0 * cv;
    const double dxy = 0.25 * (((SP(0, -1, -1) - SP(0, -1, 1)) - SP(0, 1, -1)) + SP(0, 1, 1));
    const double dys = 0.25 * (((SP(-1, 1, 0) - SP(-1, -1, 0)) + SP(1, -1, 0)) - SP(1, 1, 0));
    const double dxs = 0.25 * (((SP(-1, 0, 1) - SP(-1, 0, -1)) + SP(1, 0, -1)) - SP(1, 0, 1));
#undef SP
    double A[3][3] = {{dxx, dxy, dxs}, {dxy, dyy, dys}, {dxs, dys, dss}};
    bool ok = ss_solve3(A, b, off);
    if (ok)
        for (int k = 0; k < 3; ++k)
            if (fabs(off[k]) > 0.7) ok = false;
    if (!ok) off[0] = off[1] = off[2] = 0.0;
    return cv + 0.5 * ((g[0] * off[0] + g[1] * off[1]) + g[2] * off[2]);
}

struct Frame { double a, cx, cy; };   // [[a, 0, cx], [0, a, cy]] in octave pixels

// the frame of a refined voxel and whether its 12 boundary points lie within [0, w] x [0, h]
__device__ __forceinline__ bool ss_frame(int h, int w, int d, int y, int x, const double off[3], double first_sigma,
                                         int levels, double mr, Frame& f) {
    const double s = (double)d + off[2];
    f.a = mr * (first_sigma * exp2(s / (double)levels));
    f.cx = (double)x + off[0];
    f.cy = (double)y + off[1];
    bool in = f.cx >= 0.0 && f.cx <= (double)w && f.cy >= 0.0 && f.cy <= (double)h;
    for (int i = 0; i < 11; ++i) {
        const double px = f.a * S_SIN[i] + f.cx, py = f.a * S_COS[i] + f.cy;
        in = in && px >= 0.0 && px <= (double)w && py >= 0.0 && py <= (double)h;
    }
    return in;
}

__global__ void __launch_bounds__(S_TB) k_extrema(const float* __restrict__ x, int D, int h, int w, int minima, long long total,
                                                  unsigned char* __restrict__ mask, float* __restrict__ offs,
                                                  float* __restrict__ val) {
    const long long i = (long long)blockIdx.x * S_TB + threadIdx.x;
    if (i >= total) return;
    const long long hw = (long long)h * w, vol = (long long)D * hw;
    const long long b = i / vol, r = i - b * vol;
    const int d = (int)(r / hw), q = (int)(r - d * hw), y = q / w, xx = q - y * w;
    const float* v = x + b * vol;
    const int pk = ss_peak(v, D, h, w, d, y, xx, minima);
    double off[3] = {0.0, 0.0, 0.0};
    float value = v[r];
    if (pk) value = (float)ss_refine(v, h, w, d, y, xx, (double)pk, off);
    mask[i] = pk > 0 ? 1 : (pk < 0 ? 2 : 0);
    val[i] = value;
    // channels (ds, dx, dy): the order of the coordinates (d, x, y)
    offs[b * 3 * vol + r] = (float)off[2];
    offs[b * 3 * vol + vol + r] = (float)off[0];
    offs[b * 3 * vol + 2 * vol + r] = (float)off[1];
}

struct CandLds3 {
    unsigned long long key[S_TB];
    int n, base;
};

// One octave: x is image 0's [D][h][w] of it, image b's starts istride floats later.
__global__ void __launch_bounds__(S_TB) k_ss_candidates(const float* __restrict__ x, long long istride, int D, int h, int w,
                                                        int minima, double first_sigma, int levels, double mr, uint32_t gbase,
                                                        unsigned blocks_per_image, long long cap,
                                                        unsigned long long* __restrict__ keys, int* __restrict__ cnt) {
    __shared__ CandLds3 L;
    const int tid = threadIdx.x;
    const unsigned b = blockIdx.x / blocks_per_image, blk = blockIdx.x - b * blocks_per_image;
    const long long hw = (long long)h * w, vol = (long long)D * hw;
    const long long r = (long long)blk * S_TB + tid;
    if (tid == 0) L.n = 0;
    __syncthreads();
    if (r < vol) {
        const int d = (int)(r / hw), q = (int)(r - d * hw), y = q / w, xx = q - y * w;
        const float* v = x + b * istride;
        const int pk = ss_peak(v, D, h, w, d, y, xx, minima);
        if (pk) {
            double off[3];
            Frame f;
            const float value = (float)ss_refine(v, h, w, d, y, xx, (double)pk, off);
            if (ss_frame(h, w, d, y, xx, off, first_sigma, levels, mr, f)) {
                const int pos = atomicAdd(&L.n, 1);
                L.key[pos] = ((unsigned long long)score_key(value) << 32) | (unsigned long long)(0xffffffffu - (gbase + (uint32_t)r));
            }
        }
    }
    __syncthreads();
    const int nb = L.n;
    if (tid == 0) L.base = nb ? atomicAdd(cnt + b, nb) : 0;
    __syncthreads();
    const long long base = L.base;
    if (tid < nb && base + tid < cap) keys[b * cap + base + tid] = L.key[tid];   // always: cap bounds the strict extrema
}

struct SelOct {
    const float* p;        // image 0's volume of this octave
    long long istride;
    int D, h, w;
    uint32_t base;
    double first_sigma;
};
struct SelTab {
    int n_oct;
    SelOct o[S_MAXO];
};

__global__ void __launch_bounds__(D_SEL_TB) k_ss_select(const unsigned long long* __restrict__ keys, const int* __restrict__ cnt,
                                                        long long cap, SelTab tab, int levels, double mr, int H, int W, int num,
                                                        float* __restrict__ lafs, float* __restrict__ scores,
                                                        int* __restrict__ count) {
    __shared__ SelLds L;
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const long long m = cnt[b] < cap ? cnt[b] : cap;
    const int want = select_sorted(L, keys + (long long)b * cap, m, num);
    float* lf = lafs + (long long)b * num * 6;
    float* sc = scores + (long long)b * num;
    const double minHW = (double)(H < W ? H : W);
    for (int i = tid; i < num; i += D_SEL_TB) {
        float fa = 0.f, fx = 0.f, fy = 0.f, fs = 0.f;
        if (i < want) {
            const unsigned long long k = L.sel[i];
            const uint32_t gid = 0xffffffffu - (uint32_t)k;
            int oi = 0;
            while (oi + 1 < tab.n_oct && gid >= tab.o[oi + 1].base) ++oi;
            const SelOct& o = tab.o[oi];
            const uint32_t r = gid - o.base;
            const uint32_t hw = (uint32_t)o.h * (uint32_t)o.w;
            const int d = (int)(r / hw), q = (int)(r - (uint32_t)d * hw), y = q / o.w, x = q - y * o.w;
            const float* v = o.p + (long long)b * o.istride;
            const double sg = v[r] > 0.f ? 1.0 : -1.0;
            double off[3];
            Frame f;
            ss_refine(v, o.h, o.w, d, y, x, sg, off);
            ss_frame(o.h, o.w, d, y, x, off, o.first_sigma, levels, mr, f);
            // normalize_laf on the octave, denormalize_laf on the image
            const double mo = (double)(o.h < o.w ? o.h : o.w);
            fa = (float)((f.a / mo) * minHW);
            fx = (float)((f.cx * (1.0 / (double)o.w)) * (double)W);
            fy = (float)((f.cy * (1.0 / (double)o.h)) * (double)H);
            fs = key_score((uint32_t)(k >> 32));
        }
        lf[6 * i] = fa; lf[6 * i + 1] = 0.f; lf[6 * i + 2] = fx;
        lf[6 * i + 3] = 0.f; lf[6 * i + 4] = fa; lf[6 * i + 5] = fy;
        sc[i] = fs;
    }
    if (tid == 0) count[b] = want;
}


// ---------------------------------------------------------------- host

// the float32 values of get_gaussian_kernel1d(ks, sigma): each exp in float64, the sum ascending, the
// quotient rounded to float32
void make_taps(int ks, double sigma, Taps& t) {
    double e[S_MAXK], s = 0.0;
    for (int i = 0; i < ks; ++i) {
        const double x = (double)(i - ks / 2);
        e[i] = exp(-(x * x) / (2.0 * sigma * sigma));
        s += e[i];
    }
    for (int i = 0; i < S_MAXK; ++i) t.t[i] = i < ks ? (float)(e[i] / s) : 0.f;
}

int check_blur(const std::string& nm, long long planes, int h, int w, int ks, double sigma) {
    if (planes < 0) return fail(RR_EINVAL, nm + ": negative plane count");
    if (h < 1 || w < 1) return fail(RR_EINVAL, nm + ": h and w must be positive");
    if (ks < 1 || ks > S_MAXK || ks % 2 == 0) return fail(RR_EINVAL, nm + ": ksize must be odd and in [1, 63]");
    if (ks / 2 >= (h < w ? h : w)) return fail(RR_EINVAL, nm + ": ksize / 2 must be below min(h, w) (reflect padding)");
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(RR_EINVAL, nm + ": sigma must be positive and finite");
    if (planes > 0 && planes > S_MAXPIX / ((long long)h * w)) return fail(RR_EINVAL, nm + ": more than 2^31 pixels");
    return RR_OK;
}

// in_kind: 0 float32, 1 uint8, 2 float64; (planes, h, w) checked by the caller
int launch_blur(const void* x, int in_kind, int gray, long long planes, int h, int w, int ks, double sigma, long long outf_ps,
                float* outf, double* outd, hipStream_t s, const char* what) {
    const long long hw = (long long)h * w, in_ps = gray ? 3 * hw : hw;
    Taps taps;
    if (ks == 1) {   // a copy (and the conversions)
        for (int i = 0; i < S_MAXK; ++i) taps.t[i] = i == 0 ? 1.f : 0.f;
    } else {
        make_taps(ks, sigma, taps);
    }
    const int p = ks / 2;
    const int T = p <= 21 ? 32 : 16;
    const int side = T + 2 * p;
    const int stride = T == 32 ? side : ((side + 15) / 32) * 32 + 16;   // >= side, 16 mod 32
    const size_t lds = ((size_t)side * stride + (size_t)side * T) * sizeof(double);   // at most 63.4 KiB
    const unsigned tiles_x = (unsigned)((w + T - 1) / T), tiles = tiles_x * (unsigned)((h + T - 1) / T);
    if (planes * (long long)tiles > 0x7fffffffll) return fail(RR_EINVAL, std::string(what) + ": more than 2^31 - 1 tiles");
    const dim3 grid((unsigned)(planes * tiles)), block(S_TB);
    if (in_kind == 1)
        hipLaunchKernelGGL(k_blur<1>, grid, block, lds, s, x, h, w, gray, taps, ks, T, stride, tiles_x, tiles, in_ps, outf_ps, hw, outf, outd);
    else if (in_kind == 2)
        hipLaunchKernelGGL(k_blur<2>, grid, block, lds, s, x, h, w, gray, taps, ks, T, stride, tiles_x, tiles, in_ps, outf_ps, hw, outf, outd);
    else
        hipLaunchKernelGGL(k_blur<0>, grid, block, lds, s, x, h, w, gray, taps, ks, T, stride, tiles_x, tiles, in_ps, outf_ps, hw, outf, outd);
    return check_launch(what);
}

struct OctPlan {
    int h, w;
    long long off;                 // floats from the start of the pyramid buffer
    double first_sigma;
    double lvl_sigma[S_MAXL];      // the sigma of each level
    double blur_sigma[S_MAXL];     // level l is level l - 1 blurred by this, l >= 1
    int ks[S_MAXL];
};
struct Plan {
    int n_oct, L;
    double s0;                     // blur of the first level (ks0 == 0: none)
    int ks0;
    OctPlan o[S_MAXO];
    long long total;               // floats of the pyramid buffer
};

int kernel_size(double sigma) {
    int ks = (int)(2.0 * 4.0 * sigma + 1.0);
    return ks % 2 == 0 ? ks + 1 : ks;
}

// ScalePyramid's host arithmetic, pyramid.py:62-158.  0 or an error code.
int make_plan(const std::string& nm, int n, int c, int h, int w, int levels, double sigma, int min_size, Plan& P) {
    if (n < 0) return fail(RR_EINVAL, nm + ": negative n");
    if (c != 1 && c != 3) return fail(RR_EINVAL, nm + ": c must be 1 or 3");
    if (h < 1 || w < 1) return fail(RR_EINVAL, nm + ": h and w must be positive");
    if (levels < 1 || levels > S_MAXLEVELS) return fail(RR_EINVAL, nm + ": levels outside [1, 8]");
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(RR_EINVAL, nm + ": sigma must be positive and finite");
    if (min_size < 1) return fail(RR_EINVAL, nm + ": min_size must be positive");
    const int L = levels + 3;
    if (n > 0 && ((long long)n * c > S_MAXPIX / ((long long)h * w) || (long long)n * L > S_MAXPIX / ((long long)h * w)))
        return fail(RR_EINVAL, nm + ": more than 2^31 pixels");
    const double step = pow(2.0, 1.0 / (double)levels);
    P.L = L;
    P.n_oct = 0;
    P.total = 0;
    double cur = 0.5;
    P.ks0 = 0;
    P.s0 = 0.0;
    if (sigma > cur) {
        P.s0 = sqrt(sigma * sigma - cur * cur);
        if (P.s0 < 0.01) P.s0 = 0.01;
        P.ks0 = kernel_size(P.s0);
        cur = sigma;
        if (P.ks0 > S_MAXK) return fail(RR_EINVAL, nm + ": a blur of more than 63 taps");
        if (P.ks0 / 2 >= (h < w ? h : w)) return fail(RR_EINVAL, nm + ": h or w too small for the reflect padding of the first level");
    }
    int oh = h, ow = w;
    for (;;) {
        if (P.n_oct == S_MAXO) return fail(RR_EINVAL, nm + ": more than 16 octaves");
        OctPlan& o = P.o[P.n_oct++];
        o.h = oh; o.w = ow; o.off = P.total;
        o.first_sigma = cur;
        o.lvl_sigma[0] = cur; o.blur_sigma[0] = 0.0; o.ks[0] = 0;
        for (int l = 1; l < L; ++l) {
            const double s = cur * sqrt(step * step - 1.0);
            int ks = kernel_size(s);
            const int mn = oh < ow ? oh : ow;
            if (ks > mn) ks = mn;              // the reference's cap is part of the rule
            if (ks % 2 == 0) ks += 1;
            if (ks > S_MAXK) return fail(RR_EINVAL, nm + ": a blur of more than 63 taps");
            if (ks / 2 >= mn) return fail(RR_EINVAL, nm + ": an octave too small for its reflect padding");
            cur *= step;
            o.blur_sigma[l] = s; o.ks[l] = ks; o.lvl_sigma[l] = cur;
        }
        P.total += (long long)((((size_t)n * L * oh * ow) + 63) & ~(size_t)63);
        oh = oh / 2; ow = ow / 2;
        cur = sigma;
        if ((oh < ow ? oh : ow) <= min_size) break;
    }
    return RR_OK;
}

// the caller's output buffer of rr_scale_pyramid
size_t pyr_out_bytes(const Plan& P) { return ((size_t)P.total * 4 + 255) / 256 * 256; }

struct PyrWs {
    double* buf[3];   // working planes [n][h][w]
};

PyrWs pyr_layout(Arena& a, int n, int h, int w) {
    const size_t plane = (size_t)n * h * w;
    return {{a.take<double>(plane), a.take<double>(plane), a.take<double>(plane)}};
}

int launch_pyramid(const void* x, int n, int c, int h, int w, int u8, const Plan& P, float* out, const PyrWs& ws,
                   hipStream_t s, const char* what) {
    double* const* buf = ws.buf;
    int rot = 0;   // level l of the current octave lives in buf[(rot + l) % 3]
    // the float32 levels of an octave are [n][L][h][w] (plane stride L h w per image), the working planes [n][h][w]
    int rc = launch_blur(x, u8 ? 1 : 0, c == 3, n, h, w, P.ks0 ? P.ks0 : 1, P.ks0 ? P.s0 : 1.0, (long long)P.L * h * w,
                         out + P.o[0].off, buf[0], s, what);
    if (rc) return rc;
    for (int oi = 0; oi < P.n_oct; ++oi) {
        const OctPlan& o = P.o[oi];
        const long long plane = (long long)o.h * o.w;
        for (int l = 1; l < P.L; ++l) {
            rc = launch_blur(buf[(rot + l - 1) % 3], 2, 0, n, o.h, o.w, o.ks[l], o.blur_sigma[l], P.L * plane,
                             out + o.off + l * plane, buf[(rot + l) % 3], s, what);
            if (rc) return rc;
        }
        if (oi + 1 == P.n_oct) break;
        const OctPlan& nx = P.o[oi + 1];
        const int keep = (rot + P.L - 3) % 3, to = (keep + 1) % 3;
        const long long total = (long long)n * nx.h * nx.w;
        hipLaunchKernelGGL(k_down, dim3((unsigned)((total + S_TB - 1) / S_TB)), dim3(S_TB), 0, s, buf[keep], o.h, o.w, nx.h, nx.w,
                           total, (long long)P.L * nx.h * nx.w, buf[to], out + nx.off);
        rc = check_launch(what);
        if (rc) return rc;
        rot = to;
    }
    return RR_OK;
}

// ceil(D / 2) ceil(h / 2) ceil(w / 2) maxima and as many minima per octave
long long cand_cap(const Plan& P) {
    long long c = 0;
    for (int i = 0; i < P.n_oct; ++i)
        c += 2ll * ((P.L - 1 + 1) / 2) * ((P.o[i].h + 1) / 2) * ((P.o[i].w + 1) / 2);
    return c;
}

struct SelectWs {
    unsigned long long* keys;   // cand_cap candidate keys per image
    int* cnt;
};

SelectWs select_layout(Arena& a, int n, const Plan& P) {
    return {a.take<unsigned long long>((size_t)n * (size_t)cand_cap(P)), a.take<int>((size_t)n)};
}

struct DetectWs {
    float* pyr;    // first: _ops.detect_scale_space(return_pyramid=True) reads it at the aligned start
    PyrWs pw;
    float* sig;
    float* resp;   // the pyramid's layout
    SelectWs sel;
};

DetectWs detect_layout(Arena& a, int n, int h, int w, const Plan& P) {
    return {a.take<float>((size_t)P.total), pyr_layout(a, n, h, w), a.take<float>((size_t)n * P.L),
            a.take<float>((size_t)P.total), select_layout(a, n, P)};
}

int check_select(const std::string& nm, int n, const Plan& P, int minima, double mr, int num) {
    if (minima != 0 && minima != 1) return fail(RR_EINVAL, nm + ": minima must be 0 or 1");
    if (!(mr > 0.0) || !std::isfinite(mr)) return fail(RR_EINVAL, nm + ": mr_size must be positive and finite");
    if (num < 1 || num > D_MAXNUM) return fail(RR_EINVAL, nm + ": num outside [1, 8192]");
    long long vox = 0;
    for (int i = 0; i < P.n_oct; ++i) vox += (long long)(P.L - 1) * P.o[i].h * P.o[i].w;
    if (vox > 0xffffffffll) return fail(RR_EINVAL, nm + ": more than 2^32 - 1 voxels per image");
    return RR_OK;
}

// resp: the pyramid's layout; the first L - 1 planes of every image and octave are the volume
int launch_select(const float* resp, int n, int H, int W, const Plan& P, int levels, int minima, double mr, int num,
                  float* lafs, float* scores, int* count, const SelectWs& ws, hipStream_t s, const char* what) {
    const long long cap = cand_cap(P);
    hipLaunchKernelGGL(k_reset_counts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ws.cnt, n);
    int rc = check_launch(what);
    if (rc) return rc;
    SelTab tab;
    tab.n_oct = P.n_oct;
    uint32_t base = 0;
    const int D = P.L - 1;
    for (int i = 0; i < P.n_oct; ++i) {
        const OctPlan& o = P.o[i];
        const long long hw = (long long)o.h * o.w, vol = D * hw;
        tab.o[i] = SelOct{resp + o.off, (long long)P.L * hw, D, o.h, o.w, base, o.first_sigma};
        const unsigned bpi = (unsigned)((vol + S_TB - 1) / S_TB);
        if ((long long)bpi * n > 0x7fffffffll) return fail(RR_EINVAL, std::string(what) + ": more than 2^31 - 1 blocks");
        hipLaunchKernelGGL(k_ss_candidates, dim3(bpi * (unsigned)n), dim3(S_TB), 0, s, resp + o.off, (long long)P.L * hw, D, o.h,
                           o.w, minima, o.first_sigma, levels, mr, base, bpi, cap, ws.keys, ws.cnt);
        rc = check_launch(what);
        if (rc) return rc;
        base += (uint32_t)vol;
    }
    hipLaunchKernelGGL(k_ss_select, dim3((unsigned)n), dim3(D_SEL_TB), 0, s, ws.keys, ws.cnt, cap, tab, levels, mr, H, W, num, lafs,
                       scores, count);
    return check_launch(what);
}

}  // namespace

}  // namespace rr

using namespace rr;

extern "C" {

int rr_gaussian_blur(const float* x, long long planes, int h, int w, int ksize, double sigma, float* out, void* stream) {
    const std::string nm("rr_gaussian_blur");
    int rc = check_blur(nm, planes, h, w, ksize, sigma);
    if (rc) return rc;
    if (planes > 0 && (!x || !out)) return fail(RR_EINVAL, nm + ": null input or output");
    if (planes == 0) return RR_OK;
    return launch_blur(x, 0, 0, planes, h, w, ksize, sigma, (long long)h * w, out, nullptr, as_stream(stream), "rr_gaussian_blur");
}

int rr_scale_pyramid_bytes(int n, int c, int h, int w, int levels, double sigma, int min_size, size_t* out_bytes,
                           size_t* workspace_bytes) {
    Plan P;
    int rc = make_plan("rr_scale_pyramid_bytes", n, c, h, w, levels, sigma, min_size, P);
    if (rc) return rc;
    if (out_bytes) *out_bytes = pyr_out_bytes(P);
    if (workspace_bytes) *workspace_bytes = measured(pyr_layout, n, h, w);
    return RR_OK;
}

int rr_scale_pyramid(const void* x, int n, int c, int h, int w, int u8, int levels, double sigma, int min_size, float* out,
                     size_t out_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string nm("rr_scale_pyramid");
    Plan P;
    int rc = make_plan(nm, n, c, h, w, levels, sigma, min_size, P);
    if (rc) return rc;
    if (n > 0 && (!x || !out)) return fail(RR_EINVAL, nm + ": null input or output");
    if (out_bytes < pyr_out_bytes(P)) return fail(RR_ENOSPACE, nm + ": output buffer too small");
    Arena arena(workspace, workspace_bytes);
    const PyrWs ws = pyr_layout(arena, n, h, w);
    if (!workspace || !arena.fits()) return fail(RR_ENOSPACE, nm + ": workspace too small");
    if (n == 0) return RR_OK;
    return launch_pyramid(x, n, c, h, w, u8 != 0, P, out, ws, as_stream(stream), "rr_scale_pyramid");
}

int rr_dog_response(const float* levels, int n, int L, int h, int w, float* out, void* stream) {
    const std::string nm("rr_dog_response");
    if (n < 0) return fail(RR_EINVAL, nm + ": negative n");
    if (L < 2 || h < 1 || w < 1) return fail(RR_EINVAL, nm + ": L must be at least 2, h and w positive");
    if (n > 0 && (long long)n * L > S_MAXPIX / ((long long)h * w)) return fail(RR_EINVAL, nm + ": more than 2^31 pixels");
    if (n > 0 && (!levels || !out)) return fail(RR_EINVAL, nm + ": null input or output");
    if (n == 0) return RR_OK;
    const long long hw = (long long)h * w, total = (long long)n * (L - 1) * hw;
    hipLaunchKernelGGL(k_dog, dim3((unsigned)((total + S_TB - 1) / S_TB)), dim3(S_TB), 0, as_stream(stream), levels, L, hw, L * hw,
                       (L - 1) * hw, total, out);
    return check_launch("rr_dog_response");
}

int rr_scale_space_extrema(const float* x, int n, int D, int h, int w, int minima, unsigned char* mask, float* offsets,
                           float* values, void* stream) {
    const std::string nm("rr_scale_space_extrema");
    if (n < 0) return fail(RR_EINVAL, nm + ": negative n");
    if (D < 1 || h < 1 || w < 1) return fail(RR_EINVAL, nm + ": D, h and w must be positive");
    if (minima != 0 && minima != 1) return fail(RR_EINVAL, nm + ": minima must be 0 or 1");
    if (n > 0 && (long long)n * D > S_MAXPIX / ((long long)h * w)) return fail(RR_EINVAL, nm + ": more than 2^31 voxels");
    if (n > 0 && (!x || !mask || !offsets || !values)) return fail(RR_EINVAL, nm + ": null input or output");
    if (n == 0) return RR_OK;
    const long long total = (long long)n * D * h * w;
    hipLaunchKernelGGL(k_extrema, dim3((unsigned)((total + S_TB - 1) / S_TB)), dim3(S_TB), 0, as_stream(stream), x, D, h, w, minima,
                       total, mask, offsets, values);
    return check_launch("rr_scale_space_extrema");
}

size_t rr_detect_scale_space_workspace_bytes(int n, int c, int h, int w, int levels, double sigma, int min_size) {
    Plan P;
    if (make_plan("rr_detect_scale_space_workspace_bytes", n, c, h, w, levels, sigma, min_size, P)) return 0;
    return measured(detect_layout, n, h, w, P);
}

int rr_scale_space_select(const float* resp, int n, int h, int w, int levels, double sigma, int min_size, int minima,
                          double mr_size, int num, float* lafs, float* scores, int* count, void* workspace,
                          size_t workspace_bytes, void* stream) {
    const std::string nm("rr_scale_space_select");
    Plan P;
    int rc = make_plan(nm, n, 1, h, w, levels, sigma, min_size, P);
    if (rc) return rc;
    rc = check_select(nm, n, P, minima, mr_size, num);
    if (rc) return rc;
    if (n > 0 && (!resp || !lafs || !scores || !count)) return fail(RR_EINVAL, nm + ": null input or output");
    Arena arena(workspace, workspace_bytes);
    const SelectWs ws = select_layout(arena, n, P);
    if (!workspace || !arena.fits()) return fail(RR_ENOSPACE, nm + ": workspace too small");
    if (n == 0) return RR_OK;
    return launch_select(resp, n, h, w, P, levels, minima, mr_size, num, lafs, scores, count, ws, as_stream(stream),
                         "rr_scale_space_select");
}

int rr_detect_scale_space(const void* x, int n, int c, int h, int w, int u8, int levels, double sigma, int min_size, int kind,
                          double k, int minima, double mr_size, int num, float* lafs, float* scores, int* count,
                          void* workspace, size_t workspace_bytes, void* stream) {
    const std::string nm("rr_detect_scale_space");
    Plan P;
    int rc = make_plan(nm, n, c, h, w, levels, sigma, min_size, P);
    if (rc) return rc;
    if (kind != RR_RESP_HARRIS && kind != RR_RESP_GFTT && kind != RR_RESP_HESSIAN && kind != RR_RESP_DOG)
        return fail(RR_EINVAL, nm + ": unknown kind");
    if (kind == RR_RESP_HARRIS && !std::isfinite(k)) return fail(RR_EINVAL, nm + ": k must be finite");
    if (kind != RR_RESP_DOG)
        for (int i = 0; i < P.n_oct; ++i)
            if (P.o[i].h < 4 || P.o[i].w < 4) return fail(RR_EINVAL, nm + ": an octave below 4 pixels (the responses need 4)");
    rc = check_select(nm, n, P, minima, mr_size, num);
    if (rc) return rc;
    if (n > 0 && (!x || !lafs || !scores || !count)) return fail(RR_EINVAL, nm + ": null input or output");
    Arena arena(workspace, workspace_bytes);
    const auto [pyr, pw, sig, resp, sel] = detect_layout(arena, n, h, w, P);
    if (!workspace || !arena.fits()) return fail(RR_ENOSPACE, nm + ": workspace too small");
    if (n == 0) return RR_OK;
    hipStream_t s = as_stream(stream);
    rc = launch_pyramid(x, n, c, h, w, u8 != 0, P, pyr, pw, s, "rr_detect_scale_space");
    if (rc) return rc;
    for (int i = 0; i < P.n_oct; ++i) {
        const OctPlan& o = P.o[i];
        const long long hw = (long long)o.h * o.w;
        if (kind == RR_RESP_DOG) {
            const long long total = (long long)n * (P.L - 1) * hw;
            hipLaunchKernelGGL(k_dog, dim3((unsigned)((total + S_TB - 1) / S_TB)), dim3(S_TB), 0, s, pyr + o.off, P.L, hw, P.L * hw,
                               P.L * hw, total, resp + o.off);
            rc = check_launch("rr_detect_scale_space");
        } else {
            SigTab tab;
            for (int l = 0; l < S_MAXL; ++l) tab.s[l] = l < P.L ? (float)o.lvl_sigma[l] : 0.f;
            hipLaunchKernelGGL(k_fill_sigmas, dim3((unsigned)((n * P.L + S_TB - 1) / S_TB)), dim3(S_TB), 0, s, sig, n, P.L, tab);
            rc = check_launch("rr_detect_scale_space");
            if (rc) return rc;
            rc = rr_response(pyr + o.off, n * P.L, 1, o.h, o.w, 0, 0, kind, k, sig, resp + o.off, stream);
        }
        if (rc) return rc;
    }
    return launch_select(resp, n, h, w, P, levels, minima, mr_size, num, lafs, scores, count, sel, s, "rr_detect_scale_space");
}

}  // extern "C"
