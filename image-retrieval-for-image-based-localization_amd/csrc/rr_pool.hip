// librr.so — descriptor head: global pooling (GeM / MAC / SPoC), L2N, the
// whitening Linear, and the fused globalHead tail.  All HBM-/L2-bound:
// coalesced 8-16 B loads, f32 accumulation, wave shuffles + LDS partials.
//
// Reference: cirtorch/modules/pools.py:10-38 (MAC, SPoC, GeM),
// cirtorch/modules/normalizations.py:9-16 (L2N),
// cirtorch/modules/heads/global_head.py:52-67 (pool -> L2N -> Linear -> L2N).
#include "rr_internal.h"

namespace rr {

// GeM power: exact repeated product for the common integer p (the reference
// evaluates torch.pow with a tensor exponent; for p = 3 both are the cube).
__device__ __forceinline__ float powp(float x, float p, int ip) {
    if (ip == 3) return x * x * x;
    if (ip == 2) return x * x;
    if (ip == 1) return x;
    return __powf(x, p);
}

// NaN-propagating clamp / max (max_nan, rr_internal.h), the semantics of
// torch.clamp(min=eps) and torch.max the reference pools use (pools.py:10-38):
// a NaN activation (an overflowed fp16 chain) must reach the descriptor, where
// extract_vectors sees it, instead of being replaced by eps (fmaxf drops a NaN
// operand).
__device__ __forceinline__ float clamp_min_nan(float v, float eps) { return v < eps ? eps : v; }

// The exponent of a GeM parameter living in device memory (a learnable
// ``pool.p``, pools.py:34) is read by the kernel itself: no host read-back, so
// any update of the parameter (load_state_dict, optimizer step, in-place
// ``p.data.fill_``) is seen by the next launch and a forward stays
// graph-capturable.  pdev == nullptr: the host value p is used.
__device__ __forceinline__ void gem_exponent(const float* pdev, float& p, int& ip) {
    if (pdev) {
        p = *pdev;
        ip = (p == 3.f) ? 3 : (p == 2.f) ? 2 : (p == 1.f) ? 1 : 0;
    }
}

// NHWC: [n][hw][c].  Block = 256 threads = 4 waves; each lane owns 4 channels
// (one 16-B f32 / 8-B bf16 load per pixel), each wave a quarter of the pixels;
// the 4 partial sums are combined through LDS.  grid = (ceil(c/256), n).
template <typename T>
__global__ void __launch_bounds__(256) k_pool_nhwc(const T* __restrict__ x, int c, int hw, int mode, float p,
                                                   int ip, const float* __restrict__ pdev, float eps,
                                                   float* __restrict__ out) {
    gem_exponent(pdev, p, ip);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ch = blockIdx.x * 256 + lane * 4;
    const long long img = blockIdx.y;
    __shared__ float part[4][256];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (mode == RR_POOL_MAC) acc[0] = acc[1] = acc[2] = acc[3] = -INFINITY;
    if (ch < c) {
        const T* base = x + img * hw * c + ch;
        for (int i = wave; i < hw; i += 4) {
            float v[4];
            const T* q = base + (long long)i * c;
            if constexpr (sizeof(T) == 4) {
                float4 t = *reinterpret_cast<const float4*>(q);
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else if constexpr (std::is_same<T, f16_t>::value) {
                typedef __attribute__((ext_vector_type(4))) _Float16 h4;
                const h4 t = *reinterpret_cast<const h4*>(q);
                v[0] = (float)t.x; v[1] = (float)t.y; v[2] = (float)t.z; v[3] = (float)t.w;
            } else {
                ushort4 t = *reinterpret_cast<const ushort4*>(q);
                v[0] = bf2f(t.x); v[1] = bf2f(t.y); v[2] = bf2f(t.z); v[3] = bf2f(t.w);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (mode == RR_POOL_GEM) acc[r] += powp(clamp_min_nan(v[r], eps), p, ip);
                else if (mode == RR_POOL_MAC) acc[r] = max_nan(acc[r], v[r]);
                else acc[r] += v[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][lane * 4 + r] = acc[r];
    __syncthreads();
    if (wave == 0 && ch < c) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = lane * 4 + r;
            float v;
            if (mode == RR_POOL_MAC) {
                v = max_nan(max_nan(part[0][j], part[1][j]), max_nan(part[2][j], part[3][j]));
            } else {
                v = ((part[0][j] + part[1][j]) + (part[2][j] + part[3][j])) / (float)hw;
                if (mode == RR_POOL_GEM) v = __powf(v, 1.0f / p);
            }
            out[img * c + ch + r] = v;
        }
    }
}

// NHWC bf16 with c % 8 == 0 (the extractor's stage maps): one 16-B load = 8
// channels per lane, a wave covers 512 channels of one pixel, the block's 16
// waves split the pixels (4 loads in flight per lane); the 16 partials are
// combined through LDS in a fixed order.  grid = (ceil(c/512), n).
template <typename H>
__global__ void __launch_bounds__(1024) k_pool_nhwc_h16x8(const uint4* __restrict__ x, int c, int hw, int mode,
                                                           float p, int ip, const float* __restrict__ pdev,
                                                           float eps, float* __restrict__ out) {
    gem_exponent(pdev, p, ip);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c8 = c >> 3;
    const int g = blockIdx.x * 64 + lane;  // this lane's 8-channel group
    const long long img = blockIdx.y;
    __shared__ float part[16][512];
    const bool mac = mode == RR_POOL_MAC;
    float acc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = mac ? -INFINITY : 0.f;
    auto add = [&](uint4 q) {
        const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v0 = H16<H>::lo(u[e]), v1 = H16<H>::hi(u[e]);
            if (mode == RR_POOL_GEM) {
                acc[2 * e] += powp(clamp_min_nan(v0, eps), p, ip);
                acc[2 * e + 1] += powp(clamp_min_nan(v1, eps), p, ip);
            } else if (mac) {
                acc[2 * e] = max_nan(acc[2 * e], v0);
                acc[2 * e + 1] = max_nan(acc[2 * e + 1], v1);
            } else {
                acc[2 * e] += v0;
                acc[2 * e + 1] += v1;
            }
        }
    };
    if (g < c8) {
        const uint4* base = x + img * hw * c8 + g;
        int i = wave;
        for (; i + 48 < hw; i += 64) {
            const uint4 q0 = base[(long long)i * c8], q1 = base[(long long)(i + 16) * c8];
            const uint4 q2 = base[(long long)(i + 32) * c8], q3 = base[(long long)(i + 48) * c8];
            add(q0); add(q1); add(q2); add(q3);
        }
        for (; i < hw; i += 16) add(base[(long long)i * c8]);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) part[wave][lane * 8 + r] = acc[r];
    __syncthreads();
    if (threadIdx.x < 512) {
        const int ch = blockIdx.x * 512 + threadIdx.x;
        if (ch < c) {
            float v = part[0][threadIdx.x];
            for (int w = 1; w < 16; ++w) v = mac ? max_nan(v, part[w][threadIdx.x]) : v + part[w][threadIdx.x];
            if (!mac) {
                v = v / (float)hw;
                if (mode == RR_POOL_GEM) v = __powf(v, 1.0f / p);
            }
            out[img * c + ch] = v;
        }
    }
}

// NCHW: one wave per (image, channel) plane of hw contiguous values.
template <typename T>
__global__ void __launch_bounds__(256) k_pool_nchw(const T* __restrict__ x, long long planes, int hw, int mode,
                                                   float p, int ip, const float* __restrict__ pdev, float eps,
                                                   float* __restrict__ out) {
    gem_exponent(pdev, p, ip);
    const long long plane = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (plane >= planes) return;
    const T* base = x + plane * hw;
    float acc = mode == RR_POOL_MAC ? -INFINITY : 0.f;
    for (int i = lane; i < hw; i += 64) {
        float v = DT<T>::to_f(base[i]);
        if (mode == RR_POOL_GEM) acc += powp(clamp_min_nan(v, eps), p, ip);
        else if (mode == RR_POOL_MAC) acc = max_nan(acc, v);
        else acc += v;
    }
    if (mode == RR_POOL_MAC) {
        for (int o = 32; o > 0; o >>= 1) acc = max_nan(acc, __shfl_xor(acc, o, 64));
    } else {
        acc = wave_sum(acc);
    }
    if (lane == 0) {
        float v = acc;
        if (mode != RR_POOL_MAC) {
            v = v / (float)hw;
            if (mode == RR_POOL_GEM) v = __powf(v, 1.0f / p);
        }
        out[plane] = v;
    }
}

// Row L2N: one 256-thread block per row.
__global__ void __launch_bounds__(256) k_l2n_rows(const float* __restrict__ x, int dim, float eps,
                                                  float* __restrict__ y) {
    const long long row = blockIdx.x;
    const float* xr = x + row * dim;
    __shared__ float red[4];
    float ss = 0.f;
    for (int i = threadIdx.x; i < dim; i += 256) ss += xr[i] * xr[i];
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float nrm = sqrtf((red[0] + red[1]) + (red[2] + red[3])) + eps;
    for (int i = threadIdx.x; i < dim; i += 256) y[row * dim + i] = xr[i] / nrm;
}

// Dense layer on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32): a block of 8
// waves owns 16 outputs x 64 rows; wave w takes the K-slices kb = w, w+8, ...
// of 16 inputs.  Lane (r = lane & 15, g = lane >> 4) loads W[o0+r][16kb+4g..+3]
// and x[row+r][16kb+4g..+3] as float4; MFMA e of the four uses component e, so
// each instruction sums k = 16kb + 4g + e over g — every k exactly once.  The
// 8 partial tiles are reduced through LDS in a fixed order.  W is read once per
// 64 rows (the old one-wave-per-output form re-read x per output: ~100x the
// L2 traffic).  in_dim % 4 == 0.  grid = (ceil(out/16), ceil(rows/64)).
typedef __attribute__((ext_vector_type(4))) float lf32x4_t;
__global__ void __launch_bounds__(512) k_linear_mfma(const float* __restrict__ x, int rows, int in_dim,
                                                     const float* __restrict__ w, const float* __restrict__ b,
                                                     int out_dim, float* __restrict__ y) {
    constexpr int RG = 4;  // 16-row groups per block
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int o0 = blockIdx.x * 16, row0 = blockIdx.y * 16 * RG;
    __shared__ float part[8][RG][64][4];
    lf32x4_t acc[RG];
#pragma unroll
    for (int j = 0; j < RG; ++j) acc[j] = (lf32x4_t){0.f, 0.f, 0.f, 0.f};
    const int nkb = (in_dim + 15) / 16;
    const bool orow = o0 + r < out_dim;
    const float* wr = w + (long long)(orow ? o0 + r : 0) * in_dim;
    for (int kb = wave; kb < nkb; kb += 8) {
        const int k = kb * 16 + g * 4;
        const bool kin = k < in_dim;
        const float4 a = (orow && kin) ? *reinterpret_cast<const float4*>(wr + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 bx[RG];
#pragma unroll
        for (int j = 0; j < RG; ++j) {
            const int row = row0 + j * 16 + r;
            bx[j] = (row < rows && kin) ? *reinterpret_cast<const float4*>(x + (long long)row * in_dim + k)
                                        : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < RG; ++j) {
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bx[j].x, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bx[j].y, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bx[j].z, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bx[j].w, acc[j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < RG; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) part[wave][j][lane][e] = acc[j][e];
    __syncthreads();
    // lane L of the tile holds D[o = 4*(L>>4) + e][row = L & 15]
    for (int t = threadIdx.x; t < RG * 64 * 4; t += 512) {
        const int j = t >> 8, L = (t >> 2) & 63, e = t & 3;
        float v = part[0][j][L][e];
#pragma unroll
        for (int q = 1; q < 8; ++q) v += part[q][j][L][e];
        const int o = o0 + 4 * (L >> 4) + e, row = row0 + j * 16 + (L & 15);
        if (o < out_dim && row < rows) y[(long long)row * out_dim + o] = v + (b ? b[o] : 0.f);
    }
}


// Post-hoc learned whitening (cirtorch/utils/whiten.py:4-12, applied by
// scripts/test.py:253-254) in the reference's arithmetic type: numpy promotes
// the float32 descriptors to float64 against the float64 (m, P) of
// whitenlearn, so y = P[:d] (x - m) and the L2 norm run in float64 here too,
// on the f64 MFMA (v_mfma_f64_16x16x4_f64).  Whitening matrices amplify
// directions of small variance, so a float32 GEMM loses ~1e-3 absolute on
// the output; float64 keeps it at the final float32 rounding.
// Block = 8 waves, 16 outputs x 64 rows; wave w takes the K-slices kb = w,
// w + 8, ... of 16 inputs; lane (r = lane & 15, g = lane >> 4) loads
// P[o0 + r][16 kb + 4 g .. + 3] and x[row + r][...] (centred in f64), MFMA e
// of the four uses component e.  f64 C/D layout: col = lane & 15,
// row = (lane >> 4) + 4 e.  Partial tiles reduced through LDS in fixed order.
typedef __attribute__((ext_vector_type(4))) double lf64x4_t;
__global__ void __launch_bounds__(512) k_whiten_f64(const float* __restrict__ x, int rows, int dim,
                                                    const double* __restrict__ m, const double* __restrict__ P,
                                                    int d_out, double* __restrict__ y) {
    constexpr int RG = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int o0 = blockIdx.x * 16, row0 = blockIdx.y * 16 * RG;
    __shared__ double part[8][RG][64][4];
    lf64x4_t acc[RG];
#pragma unroll
    for (int j = 0; j < RG; ++j) acc[j] = (lf64x4_t){0.0, 0.0, 0.0, 0.0};
    const int nkb = dim / 16;
    const bool orow = o0 + r < d_out;
    const double* pr = P + (long long)(orow ? o0 + r : 0) * dim;
    for (int kb = wave; kb < nkb; kb += 8) {
        const int k = kb * 16 + g * 4;
        double a[4];
        if (orow) {
            const double2 a01 = *reinterpret_cast<const double2*>(pr + k);
            const double2 a23 = *reinterpret_cast<const double2*>(pr + k + 2);
            a[0] = a01.x; a[1] = a01.y; a[2] = a23.x; a[3] = a23.y;
        } else {
            a[0] = a[1] = a[2] = a[3] = 0.0;
        }
        const double2 m01 = *reinterpret_cast<const double2*>(m + k);
        const double2 m23 = *reinterpret_cast<const double2*>(m + k + 2);
        double b[RG][4];
#pragma unroll
        for (int j = 0; j < RG; ++j) {
            const int row = row0 + j * 16 + r;
            if (row < rows) {
                const float4 v = *reinterpret_cast<const float4*>(x + (long long)row * dim + k);
                b[j][0] = (double)v.x - m01.x; b[j][1] = (double)v.y - m01.y;
                b[j][2] = (double)v.z - m23.x; b[j][3] = (double)v.w - m23.y;
            } else {
                b[j][0] = b[j][1] = b[j][2] = b[j][3] = 0.0;
            }
        }
#pragma unroll
        for (int j = 0; j < RG; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], b[j][e], acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < RG; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) part[wave][j][lane][e] = acc[j][e];
    __syncthreads();
    for (int t = threadIdx.x; t < RG * 64 * 4; t += 512) {
        const int j = t >> 8, L = (t >> 2) & 63, e = t & 3;
        double v = part[0][j][L][e];
#pragma unroll
        for (int q = 1; q < 8; ++q) v += part[q][j][L][e];
        const int o = o0 + (L >> 4) + 4 * e, row = row0 + j * 16 + (L & 15);
        if (o < d_out && row < rows) y[(long long)row * d_out + o] = v;
    }
}

// y32 = y / (||y||_2 + eps) per row, norm in float64 (whiten.py:10), fixed order.
__global__ void __launch_bounds__(256) k_l2n_rows_f64(const double* __restrict__ y, int dim, double eps,
                                                      float* __restrict__ out) {
    const long long row = blockIdx.x;
    const double* yr = y + row * dim;
    __shared__ double red[4];
    double ss = 0.0;
    for (int i = threadIdx.x; i < dim; i += 256) ss = fma(yr[i], yr[i], ss);
    ss = wave_sum_d(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    const double nrm = sqrt((red[0] + red[1]) + (red[2] + red[3])) + eps;
    for (int i = threadIdx.x; i < dim; i += 256) out[row * dim + i] = (float)(yr[i] / nrm);
}

// Regional pooling (Rpool.roipool, pools.py:127-172; GeMmp, pools.py:43-54): up
// to REGION_MAX regions per launch, every pixel of the chunk's bounding box read
// once.  The region table travels by value in the kernel arguments (256 B).
// Block = 4 waves over 256 channels: a lane owns 4 channels (one 16-B f32 / 8-B
// 16-bit load per pixel) and REGION_MAX x 4 statically indexed accumulators;
// the waves split the pixels of the box (pixel j of the box goes to wave j % 4).
// A pixel is wave-uniform: lane r < 32 tests it against region r, one ballot
// gives the 32-bit membership mask in an SGPR, and the fully unrolled region
// loop branches on its bits (scalar branches: only the regions that contain the
// pixel cost vector work, the power of GeM is taken once per pixel).  The four
// per-wave partials are combined through LDS in wave order, so a result depends
// on nothing but the image and the chunk's table.
constexpr int REGION_MAX = 32;
struct RegionTab {
    rr_region r[REGION_MAX];  // entries past the chunk's count have h == 0 (contain no pixel)
};
enum { RK_SPOC = 0, RK_GEM = 1, RK_GEM_PVEC = 2, RK_MAX = 3 };  // GEM: one exponent; GEM_PVEC: one per channel

// one pixel's 4 channels as loaded (8 B of 16-bit values or 16 B of f32), converted when it is pooled
template <typename T> struct RegionRaw { typedef uint2 type; };
template <> struct RegionRaw<float> { typedef float4 type; };
template <typename T>
__device__ __forceinline__ void region_unpack(const typename RegionRaw<T>::type& q, float* v) {
    if constexpr (sizeof(T) == 4) {
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = H16<T>::lo(q.x); v[1] = H16<T>::hi(q.x); v[2] = H16<T>::lo(q.y); v[3] = H16<T>::hi(q.y);
    }
}

// Waves per SIMD the kernel is compiled for (its VGPR budget: 168 at 3, 256 at 2) and pixels
// per batch, sized so that two batches of raw pixels fit beside the accumulators (GeM's
// general power needs the most temporaries; the per-channel form is compiled for 2 waves).
#ifndef RR_REGION_WAVES
#define RR_REGION_WAVES 3
#endif
constexpr int region_unroll(size_t esz, int kind) {
    const int regs = (RR_REGION_WAVES >= 3 && kind != RK_GEM_PVEC) ? (kind == RK_GEM ? 4 : 8) : 16;  // per batch
    return regs / (esz == 4 ? 4 : 2) > 0 ? regs / (esz == 4 ? 4 : 2) : 1;
}

// x: image 0 of the launch; map row stride W pixels, image stride hw pixels.
// (by0, bx0, bh, bw): bounding box of the chunk's regions.  out row of region r:
// (img * R + r0 + r) * c.
template <typename T, int KIND>
__global__ void __launch_bounds__(256, KIND == RK_GEM_PVEC ? 2 : RR_REGION_WAVES) k_region_pool(const T* __restrict__ x, int c, int W, long long hw,
                                                        const RegionTab tab, int nr, int by0, int bx0, int bh, int bw,
                                                        float p, int ip, const float* __restrict__ pdev, float eps,
                                                        int R, int r0, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ch = blockIdx.x * 256 + lane * 4;
    const bool valid = ch < c;
    const int chl = valid ? ch : 0;  // lanes past c pool channels 0..3 again and store nothing
    const long long img = blockIdx.y;
    __shared__ float part[REGION_MAX][256];

    float p4[4] = {p, p, p, p};
    if constexpr (KIND == RK_GEM_PVEC) {
        const float4 q = *reinterpret_cast<const float4*>(pdev + chl);
        p4[0] = q.x; p4[1] = q.y; p4[2] = q.z; p4[3] = q.w;
    } else if constexpr (KIND == RK_GEM) {
        gem_exponent(pdev, p, ip);
    }

    // lane r holds region r of the table
    int ry0 = 0, rx0 = 0, rh = 0, rw = 0;
#pragma unroll
    for (int r = 0; r < REGION_MAX; ++r) {
        if (lane == r) {
            ry0 = tab.r[r].y0; rx0 = tab.r[r].x0; rh = tab.r[r].h; rw = tab.r[r].w;
        }
    }

    float acc[REGION_MAX][4];
#pragma unroll
    for (int r = 0; r < REGION_MAX; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[r][k] = KIND == RK_MAX ? -INFINITY : 0.f;

    auto member = [&](int yy, int xx) __attribute__((always_inline)) -> unsigned {
        const bool in = (unsigned)(yy - ry0) < (unsigned)rh && (unsigned)(xx - rx0) < (unsigned)rw;
        return (unsigned)__ballot(in);
    };
    auto add = [&](const float* v, unsigned m) __attribute__((always_inline)) {
        float t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (KIND == RK_GEM_PVEC) {
                // the integer fast paths of powp as selects (the exponent differs per lane)
                const float b = clamp_min_nan(v[k], eps), b2 = b * b;
                t[k] = p4[k] == 3.f ? b2 * b : p4[k] == 2.f ? b2 : p4[k] == 1.f ? b : __powf(b, p4[k]);
            } else if constexpr (KIND == RK_GEM) {
                t[k] = powp(clamp_min_nan(v[k], eps), p, ip);
            } else {
                t[k] = v[k];
            }
        }
#pragma unroll
        for (int r = 0; r < REGION_MAX; ++r) {
            if (m & (1u << r)) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[r][k] = KIND == RK_MAX ? max_nan(acc[r][k], t[k]) : acc[r][k] + t[k];
                // keeps the scalar branch: without it the compiler turns the 32 ifs into
                // add + select for every region of every pixel (5x the vector work)
                asm volatile("" : "+v"(acc[r][0]), "+v"(acc[r][1]), "+v"(acc[r][2]), "+v"(acc[r][3]));
            }
        }
    };

    const T* base = x + img * hw * c + chl;
    const int npx = bh * bw;
    // box pixel j -> map pixel (by0 + j / bw, bx0 + j % bw), kept incrementally; a wave takes
    // its pixels wave, wave + 4, ... in batches of UNR.  The loads of batch b + 1 are issued
    // before batch b is pooled, so a wave always has loads in flight.  A slot past the box's
    // last pixel reads the box's first pixel with an empty membership mask: every load is
    // unconditional.
    typedef typename RegionRaw<T>::type raw_t;
    constexpr int UNR = region_unroll(sizeof(T), KIND);
    int j = wave;
    int yy = by0 + j / bw, xx = bx0 + j % bw;
    auto fetch = [&](raw_t* q, unsigned* m) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const bool live = j < npx;
            const int py = live ? yy : by0, px = live ? xx : bx0;
            q[u] = *reinterpret_cast<const raw_t*>(base + ((long long)py * W + px) * c);
            m[u] = live ? member(yy, xx) : 0u;
            j += 4;
            xx += 4;
            while (xx >= bx0 + bw) { xx -= bw; ++yy; }
        }
    };
    const int nbatch = (npx - wave + 4 * UNR - 1) / (4 * UNR);  // npx >= 1: wave 0 has one at least
    raw_t cur[UNR], nxt[UNR];
    unsigned mcur[UNR], mnxt[UNR];
    if (nbatch > 0) fetch(cur, mcur);
    for (int b = 0; b < nbatch; ++b) {
        fetch(nxt, mnxt);
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            float v[4];
            region_unpack<T>(cur[u], v);
            add(v, mcur[u]);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            cur[u] = nxt[u];
            mcur[u] = mnxt[u];
        }
    }

    // ((wave 0 + wave 1) + wave 2) + wave 3
    for (int w = 1; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int r = 0; r < REGION_MAX; ++r)
                if (r < nr)
                    *reinterpret_cast<float4*>(&part[r][lane * 4]) = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < REGION_MAX; ++r)
                if (r < nr) {
                    const float4 q = *reinterpret_cast<const float4*>(&part[r][lane * 4]);
                    const float o[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[r][k] = KIND == RK_MAX ? max_nan(acc[r][k], o[k]) : acc[r][k] + o[k];
                }
        }
        __syncthreads();
    }
    // the block finishes the totals (one rolled loop: mean, root, store)
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < REGION_MAX; ++r)
            if (r < nr)
                *reinterpret_cast<float4*>(&part[r][lane * 4]) = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
    }
    __syncthreads();
    const int cho = blockIdx.x * 256 + (threadIdx.x & 255);
    if (cho < c) {
        float pc = p;
        if constexpr (KIND == RK_GEM_PVEC) pc = pdev[cho];
        const unsigned short* dims = reinterpret_cast<const unsigned short*>(&tab);  // y0, x0, h, w per region
        for (int r = 0; r < nr; ++r) {
            float v = part[r][threadIdx.x];
            if constexpr (KIND != RK_MAX) v = v / (float)((int)dims[4 * r + 2] * (int)dims[4 * r + 3]);
            if constexpr (KIND == RK_GEM || KIND == RK_GEM_PVEC) v = __powf(v, 1.0f / pc);
            out[(img * R + r0 + r) * c + cho] = v;
        }
    }
}

// out[img] = L2N(sum_r rows_r), rows_r = rv[img][r] or its L2N (pools.py:183,195).
// One block per image; the row norms and the final norm are formed exactly as
// k_l2n_rows forms them (same thread partition, same order), the sum over the
// regions runs r = 0 .. R - 1.
constexpr int AGG_RMAX = 1024;
__global__ void __launch_bounds__(256) k_region_aggregate(const float* __restrict__ rv, int R, int dim, int l2n,
                                                          float eps, float* __restrict__ out) {
    const long long img = blockIdx.x;
    const float* base = rv + img * R * dim;
    float* o = out + img * dim;
    __shared__ float nrm[AGG_RMAX];
    __shared__ float red[4];
    if (l2n) {
        for (int r = 0; r < R; ++r) {
            const float* xr = base + (long long)r * dim;
            float ss = 0.f;
            for (int i = threadIdx.x; i < dim; i += 256) ss += xr[i] * xr[i];
            ss = wave_sum(ss);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
            __syncthreads();
            if (threadIdx.x == 0) nrm[r] = sqrtf((red[0] + red[1]) + (red[2] + red[3])) + eps;
            __syncthreads();
        }
    }
    float ss = 0.f;
    for (int i = threadIdx.x; i < dim; i += 256) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) {
            const float v = base[(long long)r * dim + i];
            s += l2n ? v / nrm[r] : v;
        }
        o[i] = s;  // read back below by the thread that wrote it
        ss += s * s;
    }
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float n2 = sqrtf((red[0] + red[1]) + (red[2] + red[3])) + eps;
    for (int i = threadIdx.x; i < dim; i += 256) o[i] = o[i] / n2;
}

template <typename T>
static void launch_region_pool(int kind, dim3 grid, hipStream_t s, const void* x, int c, int W, long long hw,
                               const RegionTab& tab, int nr, const int* box, float p, int ip, const float* pdev,
                               float eps, int R, int r0, float* out) {
#define RR_REGION_LAUNCH(K)                                                                                          \
    hipLaunchKernelGGL((k_region_pool<T, K>), grid, dim3(256), 0, s, (const T*)x, c, W, hw, tab, nr, box[0], box[1], \
                       box[2], box[3], p, ip, pdev, eps, R, r0, out)
    if (kind == RK_MAX) RR_REGION_LAUNCH(RK_MAX);
    else if (kind == RK_GEM_PVEC) RR_REGION_LAUNCH(RK_GEM_PVEC);
    else if (kind == RK_GEM) RR_REGION_LAUNCH(RK_GEM);
    else RR_REGION_LAUNCH(RK_SPOC);
#undef RR_REGION_LAUNCH
}

}  // namespace rr

using namespace rr;

extern "C" {

int rr_global_pool(const void* x, int n, int c, int hw, int layout, int mode, float p, float eps, float* out,
                   int dtype, void* stream) {
    if (mode == RR_POOL_GEM && !(p > 0.f)) return fail(RR_EINVAL, "rr_global_pool: GeM p must be > 0");
    return rr_global_pool_pdev(x, n, c, hw, layout, mode, p, nullptr, eps, out, dtype, stream);
}

int rr_global_pool_pdev(const void* x, int n, int c, int hw, int layout, int mode, float p, const float* p_dev,
                        float eps, float* out, int dtype, void* stream) {
    if (n <= 0 || c <= 0 || hw <= 0) return fail(RR_EINVAL, "rr_global_pool: empty input");
    if (mode < 0 || mode > 2) return fail(RR_EINVAL, "rr_global_pool: mode");
    // the host exponent is validated here; a device exponent (p_dev) is read by the kernel
    if (mode == RR_POOL_GEM && !p_dev && !(p > 0.f)) return fail(RR_EINVAL, "rr_global_pool: GeM p must be > 0");
    const float* pdev = mode == RR_POOL_GEM ? p_dev : nullptr;
    int ip = (p == 3.f) ? 3 : (p == 2.f) ? 2 : (p == 1.f) ? 1 : 0;
    hipStream_t s = as_stream(stream);
    if (layout == RR_NHWC) {
        if (c % 4) return fail(RR_EINVAL, "rr_global_pool: NHWC needs c % 4 == 0");
        dim3 grid((c + 255) / 256, n);
        if (dtype == RR_BF16 && c % 8 == 0 && ((uintptr_t)x & 15) == 0)
            hipLaunchKernelGGL(k_pool_nhwc_h16x8<bf16_t>, dim3((c + 511) / 512, n), dim3(1024), 0, s, (const uint4*)x, c, hw,
                               mode, p, ip, pdev, eps, out);
        else if (dtype == RR_F16 && c % 8 == 0 && ((uintptr_t)x & 15) == 0)
            hipLaunchKernelGGL(k_pool_nhwc_h16x8<f16_t>, dim3((c + 511) / 512, n), dim3(1024), 0, s, (const uint4*)x, c,
                               hw, mode, p, ip, pdev, eps, out);
        else if (dtype == RR_BF16)
            hipLaunchKernelGGL(k_pool_nhwc<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)x, c, hw, mode, p, ip, pdev, eps, out);
        else if (dtype == RR_F16)
            hipLaunchKernelGGL(k_pool_nhwc<f16_t>, grid, dim3(256), 0, s, (const f16_t*)x, c, hw, mode, p, ip, pdev, eps, out);
        else if (dtype == RR_F32)
            hipLaunchKernelGGL(k_pool_nhwc<float>, grid, dim3(256), 0, s, (const float*)x, c, hw, mode, p, ip, pdev, eps, out);
        else
            return fail(RR_EINVAL, "rr_global_pool: dtype");
    } else if (layout == RR_NCHW) {
        long long planes = (long long)n * c;
        dim3 grid((unsigned)((planes + 3) / 4));
        if (dtype == RR_BF16)
            hipLaunchKernelGGL(k_pool_nchw<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)x, planes, hw, mode, p, ip, pdev, eps, out);
        else if (dtype == RR_F16)
            hipLaunchKernelGGL(k_pool_nchw<f16_t>, grid, dim3(256), 0, s, (const f16_t*)x, planes, hw, mode, p, ip, pdev, eps, out);
        else if (dtype == RR_F32)
            hipLaunchKernelGGL(k_pool_nchw<float>, grid, dim3(256), 0, s, (const float*)x, planes, hw, mode, p, ip, pdev, eps, out);
        else
            return fail(RR_EINVAL, "rr_global_pool: dtype");
    } else {
        return fail(RR_EINVAL, "rr_global_pool: layout");
    }
    return check_launch("rr_global_pool");
}

int rr_l2n_rows(const float* x, int rows, int dim, float eps, float* y, void* stream) {
    if (rows <= 0 || dim <= 0) return fail(RR_EINVAL, "rr_l2n_rows: empty");
    hipLaunchKernelGGL(k_l2n_rows, dim3(rows), dim3(256), 0, as_stream(stream), x, dim, eps, y);
    return check_launch("rr_l2n_rows");
}

int rr_linear_rows(const float* x, int rows, int in_dim, const float* w, const float* b, int out_dim, float* y,
                   void* stream) {
    if (rows <= 0 || out_dim <= 0) return fail(RR_EINVAL, "rr_linear_rows: empty");
    if (in_dim % 4 || in_dim <= 0) return fail(RR_EINVAL, "rr_linear_rows: in_dim must be a positive multiple of 4");
    if ((((uintptr_t)x) | ((uintptr_t)w)) & 15) return fail(RR_EINVAL, "rr_linear_rows: x and w must be 16-byte aligned");
    hipLaunchKernelGGL(k_linear_mfma, dim3((out_dim + 15) / 16, (rows + 63) / 64), dim3(512), 0, as_stream(stream), x,
                       rows, in_dim, w, b, out_dim, y);
    return check_launch("rr_linear_rows");
}

size_t rr_head_workspace_bytes(int rows, int dim) { return (size_t)2 * rows * dim * sizeof(float); }

int rr_head_l2n_whiten_l2n(const float* x, int rows, int dim, const float* w, const float* b, int whiten, float eps,
                           float* y, void* workspace, void* stream) {
    if (!whiten) return rr_l2n_rows(x, rows, dim, eps, y, stream);
    if (!workspace) return fail(RR_EINVAL, "rr_head_l2n_whiten_l2n: workspace required");
    float* t0 = (float*)workspace;
    float* t1 = t0 + (size_t)rows * dim;
    int rc = rr_l2n_rows(x, rows, dim, eps, t0, stream);
    if (rc) return rc;
    rc = rr_linear_rows(t0, rows, dim, w, b, dim, t1, stream);
    if (rc) return rc;
    return rr_l2n_rows(t1, rows, dim, eps, y, stream);
}

int rr_region_pool(const void* x, int n, int h, int w, int c, const rr_region* regions, int R, int mode, float p,
                   const float* p_dev, int p_count, float eps, float* out, int dtype, void* stream) {
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || R <= 0 || !x || !out || !regions)
        return fail(RR_EINVAL, "rr_region_pool: empty input");
    if (h > 65535 || w > 65535) return fail(RR_EINVAL, "rr_region_pool: map larger than 65535");
    if (mode < 0 || mode > 2) return fail(RR_EINVAL, "rr_region_pool: mode");
    if (dtype != RR_F32 && dtype != RR_BF16 && dtype != RR_F16) return fail(RR_EINVAL, "rr_region_pool: dtype");
    if (c % 4) return fail(RR_EINVAL, "rr_region_pool: needs c % 4 == 0");
    if (((uintptr_t)x & (dtype == RR_F32 ? 15 : 7)) || ((uintptr_t)out & 15))
        return fail(RR_EINVAL, "rr_region_pool: x must be aligned to 4 channels, out to 16 bytes");
    for (int r = 0; r < R; ++r) {
        const rr_region& g = regions[r];
        if (g.h == 0 || g.w == 0 || (int)g.y0 + g.h > h || (int)g.x0 + g.w > w)
            return fail(RR_EINVAL, "rr_region_pool: region " + std::to_string(r) + " is empty or outside the map");
    }
    int kind = mode == RR_POOL_MAC ? RK_MAX : mode == RR_POOL_GEM ? RK_GEM : RK_SPOC;
    const float* pdev = nullptr;
    if (mode == RR_POOL_GEM) {
        if (p_count == 0) {
            if (!(p > 0.f)) return fail(RR_EINVAL, "rr_region_pool: GeM p must be > 0");
        } else if (p_count == 1 || p_count == c) {
            // a device exponent is read by the kernel
            if (!p_dev) return fail(RR_EINVAL, "rr_region_pool: p_count > 0 needs p_dev");
            if (p_count == c && ((uintptr_t)p_dev & 15))
                return fail(RR_EINVAL, "rr_region_pool: per-channel p_dev must be 16-byte aligned");
            pdev = p_dev;
            if (p_count == c) kind = RK_GEM_PVEC;
        } else {
            return fail(RR_EINVAL, "rr_region_pool: p_count must be 0, 1 or c");
        }
    }
    const int ip = (p == 3.f) ? 3 : (p == 2.f) ? 2 : (p == 1.f) ? 1 : 0;
    hipStream_t s = as_stream(stream);
    const size_t esz = dtype == RR_F32 ? 4 : 2;
    const long long hw = (long long)h * w;
    for (int r0 = 0; r0 < R; r0 += REGION_MAX) {
        const int nr = R - r0 < REGION_MAX ? R - r0 : REGION_MAX;
        RegionTab tab = {};
        int y0 = h, x0 = w, y1 = 0, x1 = 0;
        for (int r = 0; r < nr; ++r) {
            const rr_region& g = tab.r[r] = regions[r0 + r];
            y0 = g.y0 < y0 ? g.y0 : y0;
            x0 = g.x0 < x0 ? g.x0 : x0;
            y1 = g.y0 + g.h > y1 ? g.y0 + g.h : y1;
            x1 = g.x0 + g.w > x1 ? g.x0 + g.w : x1;
        }
        const int box[4] = {y0, x0, y1 - y0, x1 - x0};
        for (int i0 = 0; i0 < n; i0 += 65535) {  // grid.y limit
            const int ni = n - i0 < 65535 ? n - i0 : 65535;
            const dim3 grid((c + 255) / 256, ni);
            const void* xi = (const char*)x + (size_t)i0 * hw * c * esz;
            float* oi = out + (size_t)i0 * R * c;
            if (dtype == RR_F32) launch_region_pool<float>(kind, grid, s, xi, c, w, hw, tab, nr, box, p, ip, pdev, eps, R, r0, oi);
            else if (dtype == RR_BF16) launch_region_pool<bf16_t>(kind, grid, s, xi, c, w, hw, tab, nr, box, p, ip, pdev, eps, R, r0, oi);
            else launch_region_pool<f16_t>(kind, grid, s, xi, c, w, hw, tab, nr, box, p, ip, pdev, eps, R, r0, oi);
        }
    }
    return check_launch("rr_region_pool");
}

int rr_region_aggregate(const float* rv, int n, int R, int dim, int l2n_rows, float eps, float* out, void* stream) {
    if (n <= 0 || R <= 0 || dim <= 0 || !rv || !out) return fail(RR_EINVAL, "rr_region_aggregate: empty input");
    if (R > AGG_RMAX) return fail(RR_EINVAL, "rr_region_aggregate: more than 1024 regions");
    hipLaunchKernelGGL(k_region_aggregate, dim3(n), dim3(256), 0, as_stream(stream), rv, R, dim, l2n_rows ? 1 : 0, eps,
                       out);
    return check_launch("rr_region_aggregate");
}

size_t rr_whiten_workspace_bytes(int rows, int d_out) { return (size_t)rows * d_out * sizeof(double); }

int rr_whitenapply(const float* x, int rows, int dim, const double* m, const double* P, int d_out, float* y,
                   void* workspace, size_t workspace_bytes, void* stream) {
    if (rows <= 0 || dim <= 0 || d_out <= 0) return fail(RR_EINVAL, "rr_whitenapply: empty");
    if (dim % 16) return fail(RR_EINVAL, "rr_whitenapply: dim must be a multiple of 16");
    if (d_out > dim) return fail(RR_EINVAL, "rr_whitenapply: d_out > dim");
    if ((((uintptr_t)x) | ((uintptr_t)m) | ((uintptr_t)P)) & 15)
        return fail(RR_EINVAL, "rr_whitenapply: x, m and P must be 16-byte aligned");
    if (!workspace || workspace_bytes < rr_whiten_workspace_bytes(rows, d_out))
        return fail(RR_ENOSPACE, "rr_whitenapply: workspace too small");
    hipStream_t s = as_stream(stream);
    double* t = (double*)workspace;
    for (int r0 = 0; r0 < rows; r0 += 1 << 20) {  // <= 16384 row blocks per launch
        const int n = rows - r0 < (1 << 20) ? rows - r0 : (1 << 20);
        hipLaunchKernelGGL(k_whiten_f64, dim3((d_out + 15) / 16, (n + 63) / 64), dim3(512), 0, s,
                           x + (long long)r0 * dim, n, dim, m, P, d_out, t + (long long)r0 * d_out);
    }
    hipLaunchKernelGGL(k_l2n_rows_f64, dim3(rows), dim3(256), 0, s, t, d_out, 1e-6, y);
    return check_launch("rr_whitenapply");
}

}  // extern "C"
