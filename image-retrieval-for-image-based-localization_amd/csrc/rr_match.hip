// librr.so — batched local-descriptor matching (nn / mnn / snn / smnn).
// Replaces cirtorch/features/matching.py:5-154 (match_nn, match_mnn, match_snn,
// match_smnn: torch.cdist -> N1 x N2 matrix -> min / topk(2) per row and column)
// and, batched, the mutual check of HPatchesEval.py:31-43.
//
// One launch matches P ragged pairs in both directions and never writes a
// distance matrix.  A block owns 32 rows of one side of one pair (its "query"
// rows; 16 when 32-row blocks would not fill the chip) and streams the pair's
// other side through LDS in stages of 64 rows x 128 columns, the next stage's
// global reads in flight in registers meanwhile.  The dot products run on
// v_mfma_f64_16x16x4_f64 (float32 inputs converted on the LDS read), so
//   d2 = max(0, (|q|^2 + |o|^2) - 2 q.o)
// is exact to float64 rounding and the order needs no certificate.  Every dot
// product is one accumulator chain over k in the same order (K-chunk, 16-column
// step, MFMA e = 0..3 taking columns 16 s + 4 g + e of lane group g), whatever
// tile or operand slot the two rows sit in: identical rows give identical
// bits, d(a_i, b_j) has the same bits in both directions, and a result does
// not depend on P or the launch geometry.  The row norms come from one
// pre-pass (one wave per row, fixed order).
//
// MFMA operand slots: A = other rows (C/D row = (lane >> 4) + 4 e), B = query
// rows (C/D col = lane & 15), so a lane's four results of one MFMA are four
// other rows of ONE query row, in ascending index order: the running top-2 of
// a lane is a strict-< insert, and the 16 lists of a query row (4 lane groups
// x 4 waves) are merged once at the end by (distance, index).
#include "rr_internal.h"
#include "rr_workspace.h"

#include <math.h>

namespace rr {

namespace {

typedef __attribute__((ext_vector_type(4))) double mf64x4_t;

constexpr int M_TN = 64;         // other rows per LDS stage (16 per wave)
constexpr int M_KC = 128;        // columns per LDS stage
constexpr int M_LD = M_KC + 4;   // LDS row stride (floats): the 16 rows of a 16-B read hit 64 distinct banks

struct MatchArgs {
    const float* x[2];           // side 0 = a, side 1 = b
    const long long* off[2];
    const double* nrm[2];
    long long rows[2];
    double* od[2];               // [rows][2] of side s: distances to the other side
    int* oi[2];
    int npairs, d, tiles0;
};

// begin / length of pair p on one side, clamped to the buffer
__device__ __forceinline__ void pair_range(const long long* off, int p, long long rows, long long& b, long long& n) {
    long long lo = off[p], hi = off[p + 1];
    lo = lo < 0 ? 0 : (lo > rows ? rows : lo);
    hi = hi < lo ? lo : (hi > rows ? rows : hi);
    b = lo;
    n = hi - lo;
}

// nrm[row] = sum_k x[row][k]^2 in float64: one wave per row, lane l takes the
// 16-B groups l, l + 64, ..., then the xor butterfly
__global__ void __launch_bounds__(256) k_match_norms(const float* __restrict__ x, long long rows, int d,
                                                     double* __restrict__ nrm) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + row * d;
    double ss = 0.0;
    for (int k = lane * 4; k < d; k += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xr + k);
        ss = fma((double)v.x, (double)v.x, ss);
        ss = fma((double)v.y, (double)v.y, ss);
        ss = fma((double)v.z, (double)v.z, ss);
        ss = fma((double)v.w, (double)v.w, ss);
    }
    ss = wave_sum_d(ss);
    if (lane == 0) nrm[row] = ss;
}

// rows [r0, r0 + R) of a side (n valid) x columns [c0, c0 + kc) -> LDS, zeros outside
template <int R>
__device__ __forceinline__ void stage_rows(float* __restrict__ s, const float* __restrict__ x, long long r0,
                                           long long n, int d, int c0, int kc) {
    for (int t = threadIdx.x; t < R * (M_KC / 4); t += 256) {
        const int row = t >> 5, f = t & 31;
        if (4 * f >= kc) continue;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + row < n && c0 + 4 * f < d) v = *reinterpret_cast<const float4*>(x + (r0 + row) * d + c0 + 4 * f);
        *reinterpret_cast<float4*>(s + row * M_LD + 4 * f) = v;
    }
}

// The other side's M_TN x M_KC stage in two steps, so that the global reads of stage s + 1
// are in flight while stage s is multiplied: thread t holds the 16-B groups t, t + 256, ...
// (row = group >> 5, column group = t & 31) in 8 registers-of-four.
constexpr int M_PRE = M_TN * (M_KC / 4) / 256;
__device__ __forceinline__ void other_fetch(float4 (&pre)[M_PRE], const float* __restrict__ x, long long r0,
                                            long long n, int d, int c0) {
    const int f = threadIdx.x & 31;
#pragma unroll
    for (int u = 0; u < M_PRE; ++u) {
        const int row = (threadIdx.x >> 5) + 8 * u;
        pre[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + row < n && c0 + 4 * f < d) pre[u] = *reinterpret_cast<const float4*>(x + (r0 + row) * d + c0 + 4 * f);
    }
}
__device__ __forceinline__ void other_store(float* __restrict__ s, const float4 (&pre)[M_PRE]) {
    const int f = threadIdx.x & 31;
#pragma unroll
    for (int u = 0; u < M_PRE; ++u)
        *reinterpret_cast<float4*>(s + ((threadIdx.x >> 5) + 8 * u) * M_LD + 4 * f) = pre[u];
}

__device__ __forceinline__ bool lex_less(double d, int i, double bd, int bi) { return d < bd || (d == bd && i < bi); }

// QT: 16-row query tiles of a block (2: the throughput form; 1: twice the blocks, for
// launches that would leave compute units idle).  The two forms give the same bits.
template <int QT>
__global__ void __launch_bounds__(256, QT == 1 ? 3 : 2) k_match_top2(const MatchArgs m) {
    constexpr int TM = 16 * QT;
    __shared__ __attribute__((aligned(16))) float s_q[TM * M_LD];
    __shared__ __attribute__((aligned(16))) float s_o[M_TN * M_LD];   // reused by the final merge
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int side = (int)blockIdx.x >= m.tiles0 ? 1 : 0;
    const int tile = side ? (int)blockIdx.x - m.tiles0 : (int)blockIdx.x;
    const int d = m.d, dk = (d + 15) & ~15, nkc = (dk + M_KC - 1) / M_KC;
    for (int p = blockIdx.y; p < m.npairs; p += gridDim.y) {
        long long qb, nq, ob, no;
        pair_range(m.off[side], p, m.rows[side], qb, nq);
        pair_range(m.off[side ^ 1], p, m.rows[side ^ 1], ob, no);
        const long long row0 = (long long)tile * TM;
        if (row0 >= nq) continue;   // block-uniform
        const float* xq = m.x[side] + qb * d;
        const float* xo = m.x[side ^ 1] + ob * d;
        const double* on = m.nrm[side ^ 1] + ob;
        double qn[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) qn[t] = row0 + 16 * t + r < nq ? m.nrm[side][qb + row0 + 16 * t + r] : 0.0;
        double bd1[QT], bd2[QT];
        int bi1[QT], bi2[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            bd1[t] = bd2[t] = INFINITY;
            bi1[t] = bi2[t] = -1;
        }
        bool q_staged = false;
        float4 pre[M_PRE];
        if (no > 0) other_fetch(pre, xo, 0, no, d, 0);
        for (long long j0 = 0; j0 < no; j0 += M_TN) {
            mf64x4_t acc[QT];
#pragma unroll
            for (int t = 0; t < QT; ++t) acc[t] = (mf64x4_t){0.0, 0.0, 0.0, 0.0};
            // |o|^2 of this lane's four other rows, read while the stage is multiplied
            double nj[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long j = j0 + wave * 16 + g + 4 * e;
                nj[e] = j < no ? on[j] : 0.0;
            }
            for (int c = 0; c < nkc; ++c) {
                const int c0 = c * M_KC, kc = dk - c0 < M_KC ? dk - c0 : M_KC;
                __syncthreads();   // the previous stage's readers are done
                if (nkc > 1 || !q_staged) {
                    stage_rows<TM>(s_q, xq, row0, nq, d, c0, kc);
                    q_staged = true;
                }
                other_store(s_o, pre);
                __syncthreads();
                {   // the next stage's rows: in flight during the MFMAs below
                    const bool last_c = c + 1 == nkc;
                    const long long nj0 = last_c ? j0 + M_TN : j0;
                    if (nj0 < no) other_fetch(pre, xo, nj0, no, d, last_c ? 0 : c0 + M_KC);
                }
                const float* po = s_o + (wave * 16 + r) * M_LD + 4 * g;
                const float* pq = s_q + r * M_LD + 4 * g;
                for (int k = 0; k < kc; k += 16) {
                    const float4 vo = *reinterpret_cast<const float4*>(po + k);
                    const double ao[4] = {(double)vo.x, (double)vo.y, (double)vo.z, (double)vo.w};
                    double bq[QT][4];
#pragma unroll
                    for (int t = 0; t < QT; ++t) {
                        const float4 v = *reinterpret_cast<const float4*>(pq + 16 * t * M_LD + k);
                        bq[t][0] = (double)v.x; bq[t][1] = (double)v.y; bq[t][2] = (double)v.z; bq[t][3] = (double)v.w;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int t = 0; t < QT; ++t)
                            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ao[e], bq[t][e], acc[t], 0, 0, 0);
                }
            }
            // acc[t][e]: query row row0 + 16 t + r, other row j0 + 16 wave + g + 4 e (ascending in e)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long j = j0 + wave * 16 + g + 4 * e;
                if (j >= no) continue;
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    double dd = fma(-2.0, acc[t][e], qn[t] + nj[e]);
                    dd = dd < 0.0 ? 0.0 : dd;   // keeps NaN (a NaN row matches nothing)
                    if (dd < bd1[t]) {
                        bd2[t] = bd1[t]; bi2[t] = bi1[t];
                        bd1[t] = dd; bi1[t] = (int)j;
                    } else if (dd < bd2[t]) {
                        bd2[t] = dd; bi2[t] = (int)j;
                    }
                }
            }
        }
        // merge the 16 lists of every query row by (distance, index); LDS of the other tile reused
        __syncthreads();
        double* md = reinterpret_cast<double*>(s_o);                 // [16 lists][TM][2]
        int* mi = reinterpret_cast<int*>(md + 16 * TM * 2);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const int slot = ((wave * 4 + g) * TM + 16 * t + r) * 2;
            md[slot] = bd1[t]; md[slot + 1] = bd2[t];
            mi[slot] = bi1[t]; mi[slot + 1] = bi2[t];
        }
        __syncthreads();
        if (threadIdx.x < TM && row0 + threadIdx.x < nq) {
            double d1 = INFINITY, d2 = INFINITY;
            int i1 = -1, i2 = -1;
            for (int l = 0; l < 16; ++l) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int slot = (l * TM + threadIdx.x) * 2 + s;
                    const double cd = md[slot];
                    const int ci = mi[slot];
                    if (ci < 0) continue;
                    if (i1 < 0 || lex_less(cd, ci, d1, i1)) {
                        d2 = d1; i2 = i1;
                        d1 = cd; i1 = ci;
                    } else if (i2 < 0 || lex_less(cd, ci, d2, i2)) {
                        d2 = cd; i2 = ci;
                    }
                }
            }
            const long long o = (qb + row0 + threadIdx.x) * 2;
            m.od[side][o] = d1; m.od[side][o + 1] = d2;
            m.oi[side][o] = i1; m.oi[side][o + 1] = i2;
        }
        // the next pair's first stage starts with a barrier
    }
}

// The matching rule on the two directions' top-2 lists: one thread per side-1 row.
__global__ void __launch_bounds__(256) k_match_final(const long long* __restrict__ a_off, long long rows1,
                                                     const long long* __restrict__ b_off, long long rows2, int npairs,
                                                     const double* __restrict__ d12, const int* __restrict__ i12,
                                                     const double* __restrict__ d21, const int* __restrict__ i21,
                                                     int mode, float th, long long* __restrict__ match,
                                                     float* __restrict__ dist) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    for (int p = blockIdx.y; p < npairs; p += gridDim.y) {
        long long ab, n1, bb, n2;
        pair_range(a_off, p, rows1, ab, n1);
        pair_range(b_off, p, rows2, bb, n2);
        if (i >= n1) continue;
        const long long row = ab + i;
        const int j = i12[2 * row];
        // float32-rounded distances (what torch.cdist returns for float32 descriptors)
        const float s1 = (float)sqrt(d12[2 * row]), s2 = (float)sqrt(d12[2 * row + 1]);
        bool keep = j >= 0;
        float v = s1;
        if (keep && (mode == RR_MATCH_MNN || mode == RR_MATCH_SMNN)) keep = i21[2 * (bb + j)] == (int)i;
        if (keep && (mode == RR_MATCH_SNN || mode == RR_MATCH_SMNN)) {
            v = s1 / s2;
            keep = n2 >= 2 && v <= th;   // NaN (0 / 0) fails like the reference's `ratio <= th`
        }
        if (keep && mode == RR_MATCH_SMNN) {
            const float t1 = (float)sqrt(d21[2 * (bb + j)]), t2 = (float)sqrt(d21[2 * (bb + j) + 1]);
            const float w = t1 / t2;
            keep = n1 >= 2 && w <= th;
            v = fmaxf(v, w);
        }
        match[row] = keep ? (long long)j : -1ll;
        dist[row] = keep ? v : INFINITY;
    }
}

struct MatchWs {
    double* nrm[2];
    double* dd[2];
    int* ii[2];
};

// lists: the two directions' top-2 lists of rr_match_pairs; rr_match_top2 writes the caller's
MatchWs layout(Arena& a, long long rows1, long long rows2, int lists) {
    const size_t r[2] = {(size_t)(rows1 > 0 ? rows1 : 0), (size_t)(rows2 > 0 ? rows2 : 0)};
    MatchWs w{};
    for (int s = 0; s < 2; ++s) w.nrm[s] = a.take<double>(r[s]);
    if (!lists) return w;
    for (int s = 0; s < 2; ++s) w.dd[s] = a.take<double>(r[s] * 2);
    for (int s = 0; s < 2; ++s) w.ii[s] = a.take<int>(r[s] * 2);
    return w;
}

// argument checks shared by the two entry points: nothing here touches the GPU
int check_args(const char* who, const float* a, const long long* a_off, long long rows1, const float* b,
               const long long* b_off, long long rows2, int npairs, int d, int max_n1, int max_n2) {
    const std::string w(who);
    if (d < 4 || d > 512 || d % 4) return fail(RR_EINVAL, w + ": d must be a multiple of 4 in [4, 512]");
    if (npairs < 0 || rows1 < 0 || rows2 < 0 || max_n1 < 0 || max_n2 < 0)
        return fail(RR_EINVAL, w + ": negative size");
    if (!a_off || !b_off) return fail(RR_EINVAL, w + ": null offsets");
    if ((rows1 > 0 && !a) || (rows2 > 0 && !b)) return fail(RR_EINVAL, w + ": null descriptors");
    if ((((uintptr_t)a) & 15) || (((uintptr_t)b) & 15)) return fail(RR_EINVAL, w + ": descriptors must be 16-byte aligned");
    if (max_n1 > rows1 || max_n2 > rows2) return fail(RR_EINVAL, w + ": max_n exceeds the row count");
    if (rows1 > 0x7fffffffll || rows2 > 0x7fffffffll) return fail(RR_EINVAL, w + ": too many rows");
    return RR_OK;
}

int launch_top2(const float* a, const long long* a_off, long long rows1, const float* b, const long long* b_off,
                long long rows2, int npairs, int d, int max_n1, int max_n2, double* d12, int* i12, double* d21,
                int* i21, double* na, double* nb, hipStream_t s) {
    if (npairs == 0 || (max_n1 == 0 && max_n2 == 0)) return RR_OK;
    if (rows1 > 0) hipLaunchKernelGGL(k_match_norms, dim3((unsigned)((rows1 + 3) / 4)), dim3(256), 0, s, a, rows1, d, na);
    if (rows2 > 0) hipLaunchKernelGGL(k_match_norms, dim3((unsigned)((rows2 + 3) / 4)), dim3(256), 0, s, b, rows2, d, nb);
    int rc = check_launch("rr_match_top2: norms");
    if (rc) return rc;
    MatchArgs m;
    m.x[0] = a; m.x[1] = b;
    m.off[0] = a_off; m.off[1] = b_off;
    m.nrm[0] = na; m.nrm[1] = nb;
    m.rows[0] = rows1; m.rows[1] = rows2;
    m.od[0] = d12; m.od[1] = d21;
    m.oi[0] = i12; m.oi[1] = i21;
    m.npairs = npairs; m.d = d;
    const unsigned gy = (unsigned)(npairs < 65535 ? npairs : 65535);
    // 32-row blocks unless they would not fill the chip (a single pair, say): then 16-row blocks
    const long long blocks32 = ((long long)(max_n1 + 31) / 32 + (max_n2 + 31) / 32) * npairs;
    if (blocks32 >= 2ll * grid_cus()) {
        m.tiles0 = (max_n1 + 31) / 32;
        hipLaunchKernelGGL(k_match_top2<2>, dim3((unsigned)(m.tiles0 + (max_n2 + 31) / 32), gy), dim3(256), 0, s, m);
    } else {
        m.tiles0 = (max_n1 + 15) / 16;
        hipLaunchKernelGGL(k_match_top2<1>, dim3((unsigned)(m.tiles0 + (max_n2 + 15) / 16), gy), dim3(256), 0, s, m);
    }
    return check_launch("rr_match_top2");
}

}  // namespace

}  // namespace rr

using namespace rr;

extern "C" {

size_t rr_match_workspace_bytes(long long rows1, long long rows2, int lists) { return measured(layout, rows1, rows2, lists); }

int rr_match_top2(const float* a, const long long* a_off, long long rows1, const float* b, const long long* b_off,
                  long long rows2, int npairs, int d, int max_n1, int max_n2, double* d12, int* i12, double* d21,
                  int* i21, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_args("rr_match_top2", a, a_off, rows1, b, b_off, rows2, npairs, d, max_n1, max_n2);
    if (rc) return rc;
    if ((rows1 > 0 && (!d12 || !i12)) || (rows2 > 0 && (!d21 || !i21)))
        return fail(RR_EINVAL, "rr_match_top2: null output");
    Arena arena(workspace, workspace_bytes);
    const MatchWs w = layout(arena, rows1, rows2, 0);
    if (!workspace || !arena.fits())
        return fail(RR_ENOSPACE, "rr_match_top2: workspace too small");
    return launch_top2(a, a_off, rows1, b, b_off, rows2, npairs, d, max_n1, max_n2, d12, i12, d21, i21, w.nrm[0],
                       w.nrm[1], as_stream(stream));
}

int rr_match_pairs(const float* a, const long long* a_off, long long rows1, const float* b, const long long* b_off,
                   long long rows2, int npairs, int d, int max_n1, int max_n2, int mode, float th, long long* match,
                   float* dist, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_args("rr_match_pairs", a, a_off, rows1, b, b_off, rows2, npairs, d, max_n1, max_n2);
    if (rc) return rc;
    if (mode != RR_MATCH_NN && mode != RR_MATCH_MNN && mode != RR_MATCH_SNN && mode != RR_MATCH_SMNN)
        return fail(RR_EINVAL, "rr_match_pairs: unknown mode");
    if (rows1 > 0 && (!match || !dist)) return fail(RR_EINVAL, "rr_match_pairs: null output");
    Arena arena(workspace, workspace_bytes);
    const MatchWs w = layout(arena, rows1, rows2, 1);
    if (!workspace || !arena.fits())
        return fail(RR_ENOSPACE, "rr_match_pairs: workspace too small");
    if (npairs == 0 || max_n1 == 0) return RR_OK;
    hipStream_t s = as_stream(stream);
    rc = launch_top2(a, a_off, rows1, b, b_off, rows2, npairs, d, max_n1, max_n2, w.dd[0], w.ii[0], w.dd[1], w.ii[1],
                     w.nrm[0], w.nrm[1], s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_match_final, dim3((unsigned)((max_n1 + 255) / 256), (unsigned)(npairs < 65535 ? npairs : 65535)),
                       dim3(256), 0, s, a_off, rows1, b_off, rows2, npairs, w.dd[0], w.ii[0], w.dd[1], w.ii[1], mode, th,
                       match, dist);
    return check_launch("rr_match_pairs: finalise");
}

}  // extern "C"
