// librr.so — keypoint detection: corner / blob responses, 2-D non-maxima suppression and the
// selection of the best N local maxima per image.
// Replaces, on the device and without one intermediate plane in memory, harris_response,
// gftt_response and hessian_response of cirtorch/features/responses.py:8-103 (on spatial_gradient of
// cirtorch/filters/sobel.py:12-45, gaussian_blur2d of cirtorch/filters/gaussian.py:8-16 and filter2D
// of cirtorch/filters/filter.py:34-77), rgb_to_grayscale of cirtorch/enhance/color/gray.py:7-25,
// nms2d of cirtorch/features/nms.py:29-67,111-116 and the torch.topk(x * mask) that follows it; with
// them the host-side cv2 SIFT detector of cirtorch/datasets/localFeatures/utils.py:56-99.
//
// Everything is float64 on float32 (or uint8 / 255 in IEEE float32) pixels, every sum has one fixed
// order, each score is rounded once to float32, no atomic touches a floating-point value and nothing
// waits for the host.  The kernels:
//
//   k_response  one block of 256 threads per 32 x 32 tile of one output plane.  With p(y, x) the
//               pixel at clamped coordinates (replicate padding) -- for gray = 1 the value
//               (0.299 r + 0.587 g) + 0.114 b --
//                 dx = ((p(y-1,x+1) - p(y-1,x-1)) + 2 (p(y,x+1) - p(y,x-1)) + (p(y+1,x+1) - p(y+1,x-1))) / 8
//                 dy = ((p(y+1,x-1) - p(y-1,x-1)) + 2 (p(y+1,x) - p(y-1,x)) + (p(y+1,x+1) - p(y-1,x+1))) / 8
//               (the 3 x 3 Sobel pair as a correlation), the structure tensor
//                 A = G * dx^2,  B = G * dy^2,  C = G * (dx dy)
//               with G the separable 7 x 7 Gaussian of sigma 1 -- columns first, then rows, taps in
//               ascending offset, weights the float32 values of get_gaussian_kernel1d(7, 1.0) -- on
//               reflected coordinates (-i reads i, h - 1 + i reads h - 1 - i), det = A B - C C,
//               tr = A + B and
//                 Harris   det - k tr^2
//                 GFTT     0.5 (tr - sqrt(|tr^2 - 4 det|))
//               Hessian: the 5 x 5 second-order Sobel kernels as correlations over clamped
//               coordinates, rows then columns ascending, dxx = S_xx / 64, dyy = S_yy / 64,
//               dxy = S_xy w36 with w36 the float32 value of 1 / 36 (what the reference's normalised
//               kernel holds), score dxx dyy - dxy^2.  The score times sigma^4 = (s s)(s s) of the
//               image when sigmas are given.
//               LDS: the pixel tile with a halo of 4 (2 for Hessian) as 40 x 40 doubles, the two
//               gradients on 38 x 38, the three column-blurred products on 38 x 32 (they share the
//               pixel tile's space): 52 KiB, three blocks per CU.  The image is read once apart from
//               the halos, the score written once; no gradient, product or blurred plane is in memory.
//   k_nms       one block per 64 x 32 tile of a score plane (tile and halo in LDS): a pixel is kept when the value is greater than 0 and than
//               every other position of the ks x ks window at clamped coordinates (a clamped
//               neighbour that lands on the centre counts, so no pixel on the map's edge is kept; NaN
//               is never kept).  The comparison with 0 is the reference's: the centre filter of
//               _get_nms_kernel2d is all zeros, so its maximum over the "other" positions includes 0.
//   k_candidates the same test plus score > min_score and the border margin, one block per 64 x 32
//               tile of an image (tile and halo in LDS); a kept pixel's 64-bit key (orderable score bits
//               << 32 | ~index) is collected in LDS and the block appends its keys to the image's
//               list with one integer atomic.  Keys are unique per image, so the order of the list
//               is immaterial.  (k_reset_counts zeroes the per-image counters first.)
//   k_select    one block of 1024 threads per image: a radix select, 8 bits a pass from the top (it stops
//               at the first pass after which every key sharing the settled bits is wanted), finds
//               the num-th largest key, the keys at or above it are gathered into LDS, sorted by a bitonic network
//               (score descending, index ascending) and written as (x, y), score; the slots past
//               count hold (-1, -1) and 0.
//
// No two 8-neighbours are both strict maxima, so an image has at most ceil(h/2) ceil(w/2)
// candidates: the lists are sized by that bound and cannot overflow.  A score depends on the pixels
// of its window only: not on n, the tile, the launch or the run.
#include "rr_internal.h"
#include "rr_select.h"
#include "rr_workspace.h"

#include <math.h>

namespace rr {

namespace {

constexpr int D_TB = 256;          // threads of k_response
constexpr int D_T = 32;            // tile side
constexpr int D_G = D_T + 6;       // gradient slots per side (the blur reaches 3)
constexpr int D_I = D_T + 8;       // pixel slots per side (the gradient reaches 1 more)
constexpr int D_CW = 64, D_CH = 32; // tile of k_candidates
constexpr int D_CR = 4;            // the largest window radius (ks = 9)
constexpr long long D_MAXPIX = 1ll << 31;

// float32 values of get_gaussian_kernel1d(7, 1.0)
__device__ const double D_GW[7] = {0x1.228634p-8, 0x1.ba69e8p-5, 0x1.efb0bp-3, 0x1.98a0a2p-2,
                                   0x1.efb0bp-3, 0x1.ba69e8p-5, 0x1.228634p-8};

// 5 x 5 second-order Sobel kernels (gyy is gxx transposed)
__device__ const double D_GXX[5][5] = {{-1, 0, 2, 0, -1}, {-4, 0, 8, 0, -4}, {-6, 0, 12, 0, -6}, {-4, 0, 8, 0, -4}, {-1, 0, 2, 0, -1}};
__device__ const double D_GXY[5][5] = {{-1, -2, 0, 2, 1}, {-2, -4, 0, 4, 2}, {0, 0, 0, 0, 0}, {2, 4, 0, -4, -2}, {1, 2, 0, -2, -1}};

// reflect padding without the edge sample; |overshoot| <= 3 < size
__device__ __forceinline__ int reflecti(int v, int size) { return v < 0 ? -v : (v >= size ? 2 * size - 2 - v : v); }

template <bool U8> __device__ __forceinline__ double load_px(const void* x, long long i) {
    if constexpr (U8)  // IEEE division: the same float as torch's x.float() / 255
        return (double)((float)reinterpret_cast<const unsigned char*>(x)[i] / 255.f);
    else
        return (double)reinterpret_cast<const float*>(x)[i];
}

struct RespLds {
    union {
        double img[D_I * D_I];        // pixel tile, origin (ty0 - halo, tx0 - halo)
        double hb[3][D_G][D_T];       // column-blurred dx^2, dy^2, dx dy (rows: gradient slots)
    };
    double gx[D_G][D_G];              // origin (ty0 - 3, tx0 - 3)
    double gy[D_G][D_G];
};

template <bool U8>
__global__ void __launch_bounds__(D_TB, 3) k_response(const void* __restrict__ x, int c, int h, int w, int gray, int kind,
                                                      double kh, const float* __restrict__ sigmas, int tiles_x,
                                                      int tiles_y, float* __restrict__ out) {
    __shared__ RespLds L;
    const int tid = threadIdx.x;
    const long long tiles = (long long)tiles_x * tiles_y;
    const long long plane = (long long)blockIdx.x / tiles;   // output plane
    const int tile = (int)((long long)blockIdx.x - plane * tiles);
    const int ty0 = (tile / tiles_x) * D_T, tx0 = (tile % tiles_x) * D_T;
    const long long hw = (long long)h * w;
    const long long img_index = gray ? plane : plane / c;
    const void* src = U8 ? (const void*)(reinterpret_cast<const unsigned char*>(x) + (gray ? plane * 3 : plane) * hw)
                         : (const void*)(reinterpret_cast<const float*>(x) + (gray ? plane * 3 : plane) * hw);
    const int halo = kind == RR_RESP_HESSIAN ? 2 : 4;
    const int side = D_T + 2 * halo;

    // pixel tile at clamped coordinates
    for (int i = tid; i < side * side; i += D_TB) {
        const int ly = i / side, lx = i - ly * side;
        const long long o = (long long)clampi(ty0 - halo + ly, h - 1) * w + clampi(tx0 - halo + lx, w - 1);
        double v;
        if (gray)
            v = (0.299 * load_px<U8>(src, o) + 0.587 * load_px<U8>(src, hw + o)) + 0.114 * load_px<U8>(src, 2 * hw + o);
        else
            v = load_px<U8>(src, o);
        L.img[ly * side + lx] = v;
    }
    __syncthreads();

    double s4 = 1.0;
    if (sigmas) {
        const double s = (double)sigmas[img_index];
        s4 = (s * s) * (s * s);
    }
    float* dst = out + plane * hw;

    if (kind == RR_RESP_HESSIAN) {
        const double w36 = (double)(1.0f / 36.0f);
        for (int i = tid; i < D_T * D_T; i += D_TB) {
            const int oy = i / D_T, ox = i - oy * D_T;
            const int gy = ty0 + oy, gx = tx0 + ox;
            if (gy >= h || gx >= w) continue;
            double sxx = 0.0, sxy = 0.0, syy = 0.0;
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                // slot of the clamped coordinate: the tile holds every coordinate within 2 of it
                const int ry = clampi(gy + r - 2, h - 1) - (ty0 - 2);
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    const int rx = clampi(gx + q - 2, w - 1) - (tx0 - 2);
                    const double p = L.img[ry * side + rx];
                    if (D_GXX[r][q] != 0.0) sxx += D_GXX[r][q] * p;
                    if (D_GXY[r][q] != 0.0) sxy += D_GXY[r][q] * p;
                    if (D_GXX[q][r] != 0.0) syy += D_GXX[q][r] * p;
                }
            }
            const double dxx = sxx * (1.0 / 64.0), dyy = syy * (1.0 / 64.0), dxy = sxy * w36;
            double sc = dxx * dyy - dxy * dxy;
            if (sigmas) sc *= s4;
            dst[(long long)gy * w + gx] = (float)sc;
        }
        return;
    }

    // gradients of the in-map slots (the blur reads the others through their reflection)
    for (int i = tid; i < D_G * D_G; i += D_TB) {
        const int sy = i / D_G, sx = i - sy * D_G;
        const int gy = ty0 - 3 + sy, gx = tx0 - 3 + sx;
        double dx = 0.0, dy = 0.0;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
            const int y0 = clampi(gy - 1, h - 1) - (ty0 - 4), y1 = gy - (ty0 - 4), y2 = clampi(gy + 1, h - 1) - (ty0 - 4);
            const int x0 = clampi(gx - 1, w - 1) - (tx0 - 4), x1 = gx - (tx0 - 4), x2 = clampi(gx + 1, w - 1) - (tx0 - 4);
            const double a00 = L.img[y0 * D_I + x0], a01 = L.img[y0 * D_I + x1], a02 = L.img[y0 * D_I + x2];
            const double a10 = L.img[y1 * D_I + x0], a12 = L.img[y1 * D_I + x2];
            const double a20 = L.img[y2 * D_I + x0], a21 = L.img[y2 * D_I + x1], a22 = L.img[y2 * D_I + x2];
            dx = ((a02 - a00) + 2.0 * (a12 - a10) + (a22 - a20)) * 0.125;
            dy = ((a20 - a00) + 2.0 * (a21 - a01) + (a22 - a02)) * 0.125;
        }
        L.gx[sy][sx] = dx;
        L.gy[sy][sx] = dy;
    }
    __syncthreads();   // every read of img is done: hb may overwrite it

    // blur along x: in-map gradient rows x the tile's in-map columns
    for (int i = tid; i < D_G * D_T; i += D_TB) {
        const int sy = i / D_T, ox = i - sy * D_T;
        const int gy = ty0 - 3 + sy, gx = tx0 + ox;
        double a = 0.0, b = 0.0, cc = 0.0;
        if (gy >= 0 && gy < h && gx < w) {
#pragma unroll
            for (int d = 0; d < 7; ++d) {
                const int sx = reflecti(gx + d - 3, w) - (tx0 - 3);
                const double vx = L.gx[sy][sx], vy = L.gy[sy][sx];
                a += D_GW[d] * (vx * vx);
                b += D_GW[d] * (vy * vy);
                cc += D_GW[d] * (vx * vy);
            }
        }
        L.hb[0][sy][ox] = a;
        L.hb[1][sy][ox] = b;
        L.hb[2][sy][ox] = cc;
    }
    __syncthreads();

    // blur along y, score
    for (int i = tid; i < D_T * D_T; i += D_TB) {
        const int oy = i / D_T, ox = i - oy * D_T;
        const int gy = ty0 + oy, gx = tx0 + ox;
        if (gy >= h || gx >= w) continue;
        double a = 0.0, b = 0.0, cc = 0.0;
#pragma unroll
        for (int d = 0; d < 7; ++d) {
            const int sy = reflecti(gy + d - 3, h) - (ty0 - 3);
            a += D_GW[d] * L.hb[0][sy][ox];
            b += D_GW[d] * L.hb[1][sy][ox];
            cc += D_GW[d] * L.hb[2][sy][ox];
        }
        const double det = a * b - cc * cc, tr = a + b;
        double sc;
        if (kind == RR_RESP_HARRIS)
            sc = det - kh * (tr * tr);
        else
            sc = 0.5 * (tr - sqrt(fabs(tr * tr - 4.0 * det)));
        if (sigmas) sc *= s4;
        dst[(long long)gy * w + gx] = (float)sc;
    }
}

// The NMS rule through LDS (k_nms and k_candidates): a D_CW x D_CH tile of a plane and a halo of the
// window radius r = ks / 2 at clamped coordinates, so a clamped neighbour that lands on the centre is
// a copy of it and fails the strict comparison; every comparison reads LDS.  (An early-exit
// neighbour loop on global memory is a chain of dependent L2 latencies: 3.3 ms against under 1 ms
// for the candidate pass of 128 images of 768 x 1024.)
typedef float PeakTile[D_CH + 2 * D_CR][D_CW + 2 * D_CR];

__device__ __forceinline__ void load_peak_tile(PeakTile& t, const float* __restrict__ p, int h, int w, int ty0, int tx0, int r) {
    const int sw = D_CW + 2 * r, sh = D_CH + 2 * r;
    for (int i = threadIdx.x; i < sw * sh; i += 256) {
        const int ly = i / sw, lx = i - ly * sw;
        t[ly][lx] = p[(long long)clampi(ty0 - r + ly, h - 1) * w + clampi(tx0 - r + lx, w - 1)];
    }
}

// pixel (oy, ox) of the tile: greater than 0 and than every other position of its window (NaN never)
__device__ __forceinline__ bool tile_peak(const PeakTile& t, int oy, int ox, int r) {
    const float v = t[oy + r][ox + r];
    if (!(v > 0.f)) return false;
    for (int dy = 0; dy <= 2 * r; ++dy)
        for (int dx = 0; dx <= 2 * r; ++dx)
            if ((dy != r || dx != r) && !(v > t[oy + dy][ox + dx])) return false;
    return true;
}

__global__ void __launch_bounds__(256) k_nms(const float* __restrict__ x, int h, int w, int r, unsigned tiles_x,
                                            unsigned tiles, unsigned char* __restrict__ mask, float* __restrict__ y) {
    __shared__ PeakTile T;
    const unsigned pl = blockIdx.x / tiles, tile = blockIdx.x - pl * tiles;
    const int ty0 = (int)(tile / tiles_x) * D_CH, tx0 = (int)(tile % tiles_x) * D_CW;
    const long long off = pl * ((long long)h * w);
    load_peak_tile(T, x + off, h, w, ty0, tx0, r);
    __syncthreads();
    for (int j = threadIdx.x; j < D_CW * D_CH; j += 256) {
        const int oy = j / D_CW, ox = j - oy * D_CW;
        const int py = ty0 + oy, px = tx0 + ox;
        if (py >= h || px >= w) continue;
        const bool keep = tile_peak(T, oy, ox, r);
        const long long i = off + (long long)py * w + px;
        if (mask)
            mask[i] = keep ? 1 : 0;
        else
            y[i] = T[oy + r][ox + r] * (keep ? 1.f : 0.f);   // x * mask, as the reference multiplies (NaN stays NaN)
    }
}


// One block per tile of an image.  No two 8-neighbours are both kept, so a tile holds at most
// D_CW D_CH / 4 candidates: they are collected in LDS and appended with ONE global atomic per block
// (per-candidate atomics on the image's counter serialise: the blocks in flight all work on one or
// two images; 9 ms against 1.5 ms for the selection stage of 128 images).
struct CandLds {
    PeakTile t;
    unsigned long long key[D_CW * D_CH / 4];
    int n, base;
};

__global__ void __launch_bounds__(256) k_candidates(const float* __restrict__ x, int h, int w, int r, float min_score,
                                                   int border, long long cap, unsigned tiles_x, unsigned tiles,
                                                   unsigned long long* __restrict__ keys, int* __restrict__ cnt) {
    __shared__ CandLds L;
    const int tid = threadIdx.x;
    const unsigned b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int ty0 = (int)(tile / tiles_x) * D_CH, tx0 = (int)(tile % tiles_x) * D_CW;
    const float* p = x + b * ((long long)h * w);
    if (tid == 0) L.n = 0;
    load_peak_tile(L.t, p, h, w, ty0, tx0, r);
    __syncthreads();
    for (int j = tid; j < D_CW * D_CH; j += 256) {
        const int oy = j / D_CW, ox = j - oy * D_CW;
        const int py = ty0 + oy, px = tx0 + ox;
        if (py >= h - border || px >= w - border || py < border || px < border) continue;   // outside the map too
        const float v = L.t[oy + r][ox + r];
        const bool keep = v > min_score && tile_peak(L.t, oy, ox, r);
        if (keep) {
            const int pos = atomicAdd(&L.n, 1);
            if (pos < D_CW * D_CH / 4)   // always
                L.key[pos] = ((unsigned long long)score_key(v) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)(py * w + px));
        }
    }
    __syncthreads();
    const int nb = L.n < D_CW * D_CH / 4 ? L.n : D_CW * D_CH / 4;
    if (tid == 0) L.base = nb ? atomicAdd(cnt + b, nb) : 0;
    __syncthreads();
    const long long base = L.base;
    for (int j = tid; j < nb; j += 256)
        if (base + j < cap) keys[b * cap + base + j] = L.key[j];   // always: cap is the bound on strict maxima
}

__global__ void __launch_bounds__(D_SEL_TB) k_select(const unsigned long long* __restrict__ keys, const int* __restrict__ cnt,
                                                     long long cap, int w, int num, float* __restrict__ kpts,
                                                     float* __restrict__ scores, int* __restrict__ count) {
    __shared__ SelLds L;
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const long long m = cnt[b] < cap ? cnt[b] : cap;
    const int want = select_sorted(L, keys + (long long)b * cap, m, num);
    float* kp = kpts + (long long)b * num * 2;
    float* sc = scores + (long long)b * num;
    for (int i = tid; i < num; i += D_SEL_TB) {
        float fx = -1.f, fy = -1.f, fs = 0.f;
        if (i < want) {
            const unsigned long long k = L.sel[i];
            const uint32_t o = 0xffffffffu - (uint32_t)k;
            fx = (float)(o % (uint32_t)w);
            fy = (float)(o / (uint32_t)w);
            fs = key_score((uint32_t)(k >> 32));
        }
        kp[2 * i] = fx;
        kp[2 * i + 1] = fy;
        sc[i] = fs;
    }
    if (tid == 0) count[b] = want;
}

// ---------------------------------------------------------------- host
long long cand_cap(int h, int w) { return (long long)((h + 1) / 2) * ((w + 1) / 2); }

struct DetectWs {
    float* map;                  // the score map of rr_detect_keypoints without score_map
    unsigned long long* keys;    // cand_cap candidate keys per image
    int* cnt;
};

// (the selected keys live in LDS: num takes no room)
DetectWs layout(Arena& a, int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return {};
    return {a.take<float>((size_t)n * h * w), a.take<unsigned long long>((size_t)n * (size_t)cand_cap(h, w)),
            a.take<int>((size_t)n)};
}

// a b c d <= 2^31 without overflow (all factors >= 0)
bool pixels_ok(long long a, long long b, long long c, long long d) {
    long long p = 1;
    for (long long f : {a, b, c, d}) {
        if (f > 0 && p > D_MAXPIX / f) return false;
        p *= f;
    }
    return p <= D_MAXPIX;
}

bool ks_ok(int ks) { return ks == 3 || ks == 5 || ks == 7 || ks == 9; }

// argument checks shared by rr_response and rr_detect_keypoints; 0 or an error code
int check_response(const std::string& w, const void* x, int n, int c, int h, int wd, int gray, int kind, double k) {
    if (n < 0 || c < 1) return fail(RR_EINVAL, w + ": negative n or c < 1");
    if (h < 4 || wd < 4) return fail(RR_EINVAL, w + ": h and w must be at least 4");
    if (gray != 0 && gray != 1) return fail(RR_EINVAL, w + ": gray must be 0 or 1");
    if (gray && c != 3) return fail(RR_EINVAL, w + ": gray needs c == 3");
    if (kind != RR_RESP_HARRIS && kind != RR_RESP_GFTT && kind != RR_RESP_HESSIAN) return fail(RR_EINVAL, w + ": unknown kind");
    if (kind == RR_RESP_HARRIS && !std::isfinite(k)) return fail(RR_EINVAL, w + ": k must be finite");
    if (!pixels_ok(n, c, h, wd)) return fail(RR_EINVAL, w + ": more than 2^31 pixels");
    if (n > 0 && !x) return fail(RR_EINVAL, w + ": null input");
    return RR_OK;
}

int launch_response(const void* x, int n, int c, int h, int w, int u8, int gray, int kind, double k, const float* sigmas,
                    float* out, hipStream_t s, const char* what) {
    const int tx = (w + D_T - 1) / D_T, ty = (h + D_T - 1) / D_T;
    const long long blocks = (long long)n * (gray ? 1 : c) * tx * ty;   // <= 2^31 / 16 + edges: fits unsigned
    if (u8)
        hipLaunchKernelGGL(k_response<true>, dim3((unsigned)blocks), dim3(D_TB), 0, s, x, c, h, w, gray, kind, k, sigmas, tx, ty, out);
    else
        hipLaunchKernelGGL(k_response<false>, dim3((unsigned)blocks), dim3(D_TB), 0, s, x, c, h, w, gray, kind, k, sigmas, tx, ty, out);
    return check_launch(what);
}

int check_select(const std::string& w, int n, int h, int wd, int ks, int num, float min_score, int border) {
    if (n < 0) return fail(RR_EINVAL, w + ": negative n");
    if (h < 1 || wd < 1) return fail(RR_EINVAL, w + ": h and w must be positive");
    if (!ks_ok(ks)) return fail(RR_EINVAL, w + ": ks must be 3, 5, 7 or 9");
    if (num < 1 || num > D_MAXNUM) return fail(RR_EINVAL, w + ": num outside [1, 8192]");
    if (border < 0) return fail(RR_EINVAL, w + ": negative border");
    if (std::isnan(min_score)) return fail(RR_EINVAL, w + ": min_score is NaN");
    if (!pixels_ok(n, 1, h, wd)) return fail(RR_EINVAL, w + ": more than 2^31 pixels");
    return RR_OK;
}

int launch_select(const float* score, int n, int h, int w, int ks, int num, float min_score, int border, float* kpts,
                  float* scores, int* count, const DetectWs& ws, hipStream_t s, const char* what) {
    const long long cap = cand_cap(h, w);
    // the counters are reset by a kernel, not hipMemsetAsync (captured memset nodes: DESIGN.md §4, kNN)
    hipLaunchKernelGGL(k_reset_counts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ws.cnt, n);
    int rc = check_launch(what);
    if (rc) return rc;
    const unsigned tiles_x = (unsigned)((w + D_CW - 1) / D_CW), tiles = tiles_x * (unsigned)((h + D_CH - 1) / D_CH);
    hipLaunchKernelGGL(k_candidates, dim3((unsigned)n * tiles), dim3(256), 0, s, score, h, w, ks / 2, min_score, border, cap,
                       tiles_x, tiles, ws.keys, ws.cnt);
    rc = check_launch(what);
    if (rc) return rc;
    hipLaunchKernelGGL(k_select, dim3((unsigned)n), dim3(D_SEL_TB), 0, s, ws.keys, ws.cnt, cap, w, num, kpts, scores, count);
    return check_launch(what);
}

}  // namespace

}  // namespace rr

using namespace rr;

extern "C" {

size_t rr_detect_workspace_bytes(int n, int h, int w, int num) {
    (void)num;
    return measured(layout, n, h, w);
}

int rr_response(const void* x, int n, int c, int h, int w, int u8, int gray, int kind, double k, const float* sigmas,
                float* out, void* stream) {
    const std::string nm("rr_response");
    int rc = check_response(nm, x, n, c, h, w, gray, kind, k);
    if (rc) return rc;
    if (n > 0 && !out) return fail(RR_EINVAL, nm + ": null output");
    if (n == 0) return RR_OK;
    return launch_response(x, n, c, h, w, u8 != 0, gray, kind, k, sigmas, out, as_stream(stream), "rr_response");
}

int rr_nms2d(const float* x, long long planes, int h, int w, int ks, int mask_only, void* out, void* stream) {
    const std::string nm("rr_nms2d");
    if (planes < 0) return fail(RR_EINVAL, nm + ": negative plane count");
    if (h < 1 || w < 1) return fail(RR_EINVAL, nm + ": h and w must be positive");
    if (!ks_ok(ks)) return fail(RR_EINVAL, nm + ": ks must be 3, 5, 7 or 9");
    if (!pixels_ok(planes, 1, h, w)) return fail(RR_EINVAL, nm + ": more than 2^31 pixels");
    if (planes > 0 && (!x || !out)) return fail(RR_EINVAL, nm + ": null input or output");
    if (planes == 0) return RR_OK;
    const unsigned tiles_x = (unsigned)((w + D_CW - 1) / D_CW), tiles = tiles_x * (unsigned)((h + D_CH - 1) / D_CH);
    if (planes * tiles > 0x7fffffffll) return fail(RR_EINVAL, nm + ": more than 2^31 - 1 tiles");   // before anything is enqueued
    hipLaunchKernelGGL(k_nms, dim3((unsigned)planes * tiles), dim3(256), 0, as_stream(stream), x, h, w, ks / 2, tiles_x, tiles,
                       mask_only ? reinterpret_cast<unsigned char*>(out) : nullptr,
                       mask_only ? nullptr : reinterpret_cast<float*>(out));
    return check_launch("rr_nms2d");
}

int rr_select_keypoints(const float* score, int n, int h, int w, int ks, int num, float min_score, int border, float* kpts,
                        float* scores, int* count, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string nm("rr_select_keypoints");
    int rc = check_select(nm, n, h, w, ks, num, min_score, border);
    if (rc) return rc;
    if (n > 0 && (!score || !kpts || !scores || !count)) return fail(RR_EINVAL, nm + ": null input or output");
    Arena arena(workspace, workspace_bytes);
    const DetectWs ws = layout(arena, n, h, w);
    if (!workspace || !arena.fits()) return fail(RR_ENOSPACE, nm + ": workspace too small");
    if (n == 0) return RR_OK;
    return launch_select(score, n, h, w, ks, num, min_score, border, kpts, scores, count, ws, as_stream(stream),
                         "rr_select_keypoints");
}

int rr_detect_keypoints(const void* x, int n, int c, int h, int w, int u8, int kind, double k, const float* sigmas, int ks,
                        int num, float min_score, int border, float* kpts, float* scores, int* count, float* score_map,
                        void* workspace, size_t workspace_bytes, void* stream) {
    const std::string nm("rr_detect_keypoints");
    if (c != 1 && c != 3) return fail(RR_EINVAL, nm + ": c must be 1 or 3");
    int rc = check_response(nm, x, n, c, h, w, c == 3, kind, k);
    if (rc) return rc;
    rc = check_select(nm, n, h, w, ks, num, min_score, border);
    if (rc) return rc;
    if (n > 0 && (!kpts || !scores || !count)) return fail(RR_EINVAL, nm + ": null output");
    Arena arena(workspace, workspace_bytes);
    const DetectWs ws = layout(arena, n, h, w);
    if (!workspace || !arena.fits()) return fail(RR_ENOSPACE, nm + ": workspace too small");
    if (n == 0) return RR_OK;
    float* map = score_map ? score_map : ws.map;
    rc = launch_response(x, n, c, h, w, u8 != 0, c == 3, kind, k, sigmas, map, as_stream(stream), "rr_detect_keypoints");
    if (rc) return rc;
    return launch_select(map, n, h, w, ks, num, min_score, border, kpts, scores, count, ws, as_stream(stream),
                         "rr_detect_keypoints");
}

}  // extern "C"
