// librr.so — spatial verification: batched RANSAC homography and (weighted) DLT.
// Replaces, batched and on the device, the per-pair cv2.findHomography(..., cv2.RANSAC) loop of
// cirtorch/utils/evaluation/HPatchesEval.py:45-69 and the solvers of
// cirtorch/geometry/homography.py:11-74 (find_homography_dlt, find_homography_dlt_iterated) with
// normalize_points of cirtorch/geometry/epipolar/fundamental.py:6-33.
//
// Everything is float64 on float32 pixel keypoints, every sum has one fixed order, no atomic
// touches a floating-point value and nothing waits for the host.  Four kernels per rr_verify_pairs:
//
//   k_verify_compact  one block per pair: the kept matches (0 <= match[i] < n2) of the pair, in
//                     ascending side-1 index, become records (x1, y1, x2, y2) of four doubles at
//                     the pair's side-1 offset in the workspace (ballot + prefix over 256 rows
//                     at a time); cnt[p] = M_p.
//   k_verify_ransac   block (c, p) scores hypotheses t = 256 c .. 256 c + 255 of pair p, one per
//                     thread: the four sample indices by the counter hash of rr.h (a pure function
//                     of seed, p, t, j), the 4-point homography in registers from the projective
//                     basis construction (H = B adj(A), A and B from 3x3 adjugates, static
//                     indexing, no pivoting), then a walk over all M_p records.  The records of a
//                     pair with M_p <= V_STAGE = 1024 (32 KiB) are staged in LDS once per block and
//                     every lane reads the same record at the same time (a broadcast read); a
//                     longer pair reads them from the workspace (wave-uniform global reads).  The
//                     block's best (count desc, t asc) goes to best[p][c] as one 64-bit key.
//   k_verify_refit    one block per pair: the winner over the chunks (integer max of the keys),
//                     its H recomputed from t, then `refine` rounds of {inlier set S of H, the
//                     reference's unweighted DLT on S, accept while the count does not drop};
//                     writes inliers, H and the side-1 mask.
//   k_dlt_batch       rr_homography_dlt: the same DLT routine on caller-supplied float64 points
//                     with optional weights.
//
// The DLT routine (dlt_block) is block-wide: three passes over the selected points (sums for the
// means; mean distances; the 24 sums A^T W A is made of), each a per-thread chain over
// i = tid, tid + 256, ... followed by the xor butterfly of a wave and a fixed-order sum of the
// four waves; then cyclic Jacobi on the 9 x 9 matrix in LDS in the round-robin ordering: four
// disjoint (p, q) pairs per step, 36 lanes of wave 0, lane 9 g + k owning index k of the two rows /
// columns that pair g's rotation touches (jacobi_round).  A rotation is skipped where
// |a_pq| <= 2^-52 sqrt(a_pp a_qq) (the relative criterion for positive semi-definite matrices);
// the sweeps end with the first one that rotates nothing (6 to 8 on these matrices, V_SWEEPS at most).
// With p = (x1, y1, 1) the rows of homography.py:32-33 are ax = [0, -p, y2 p], ay = [p, 0, -x2 p], so
//   A^T W A = [[S0, 0, -Sx], [0, S0, -Sy], [-Sx, -Sy, Sr]],  S0 = sum w p p^T,  Sx = sum w x2 p p^T,
//   Sy = sum w y2 p p^T,  Sr = sum w (x2^2 + y2^2) p p^T:  4 x 6 sums per point instead of 45.
//
// A result depends on nothing but the pair's own data, seed, p and t: not on npairs, the grid or
// which pairs share the launch (the block size of every kernel is the constant 256).
//
// k_verify_compact, the pair ranges, the sampler, the block reductions, jacobi_round and the
// workspace layout are shared with the epipolar verifier (rr_epipolar.hip) and live in rr_ransac.h.
#include "rr_ransac.h"

namespace rr {

namespace {

constexpr double V_DET_EPS = RR_VERIFY_DET_EPS;
constexpr double V_W_EPS = 1e-8;

// ---------------------------------------------------------------- 4-point homography
// det [[xa, xb, xc], [ya, yb, yc], [1, 1, 1]] by differences (exact for float32 inputs)
__device__ __forceinline__ double tri(double xa, double ya, double xb, double yb, double xc, double yc) {
    return (xb - xa) * (yc - ya) - (xc - xa) * (yb - ya);
}

// B = [l0 p0, l1 p1, l2 p2] maps the projective basis e0, e1, e2, (1, 1, 1) to p0 .. p3 (up to
// scale): l = adj([p0 p1 p2]) p3.  false when three of the four points are collinear.
__device__ __forceinline__ bool basis(const double (&x)[4], const double (&y)[4], double (&b)[9]) {
    const double l0 = tri(x[3], y[3], x[1], y[1], x[2], y[2]);
    const double l1 = tri(x[0], y[0], x[3], y[3], x[2], y[2]);
    const double l2 = tri(x[0], y[0], x[1], y[1], x[3], y[3]);
    const double d = tri(x[0], y[0], x[1], y[1], x[2], y[2]);
    b[0] = l0 * x[0]; b[1] = l1 * x[1]; b[2] = l2 * x[2];
    b[3] = l0 * y[0]; b[4] = l1 * y[1]; b[5] = l2 * y[2];
    b[6] = l0;        b[7] = l1;        b[8] = l2;
    const double m = fmin(fmin(fabs(l0), fabs(l1)), fmin(fabs(l2), fabs(d)));
    return m > V_DET_EPS;   // false for NaN too
}

// H (h[8] = 1) through four records r[j] = (x1, y1, x2, y2); false: degenerate (scores 0)
__device__ __forceinline__ bool h_from4(const double (&r)[4][4], double (&h)[9]) {
    double xa[4], ya[4], xb[4], yb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { xa[j] = r[j][0]; ya[j] = r[j][1]; xb[j] = r[j][2]; yb[j] = r[j][3]; }
    double a[9], b[9];
    const bool oka = basis(xa, ya, a);
    const bool okb = basis(xb, yb, b);
    // adj(a): transposed cofactors
    double c[9];
    c[0] = a[4] * a[8] - a[5] * a[7]; c[1] = a[2] * a[7] - a[1] * a[8]; c[2] = a[1] * a[5] - a[2] * a[4];
    c[3] = a[5] * a[6] - a[3] * a[8]; c[4] = a[0] * a[8] - a[2] * a[6]; c[5] = a[2] * a[3] - a[0] * a[5];
    c[6] = a[3] * a[7] - a[4] * a[6]; c[7] = a[1] * a[6] - a[0] * a[7]; c[8] = a[0] * a[4] - a[1] * a[3];
    double g[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            g[3 * i + j] = b[3 * i] * c[j] + b[3 * i + 1] * c[3 + j] + b[3 * i + 2] * c[6 + j];
    const double inv = 1.0 / g[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = g[i] * inv;
    h[8] = 1.0;
    return oka && okb && all_finite9(h);
}

// ---------------------------------------------------------------- scoring
// || pi(H [x1, y1, 1]) - (x2, y2) ||^2 <= th^2 with both sides multiplied by w^2 (no division);
// |w| <= 1e-8 is never an inlier.  Explicit fma: the same bits wherever it is inlined.
__device__ __forceinline__ bool is_inlier(const double (&h)[9], double x1, double y1, double x2, double y2, double th2) {
    const double w = fma(h[6], x1, fma(h[7], y1, h[8]));
    const double u = fma(h[0], x1, fma(h[1], y1, h[2]));
    const double v = fma(h[3], x1, fma(h[4], y1, h[5]));
    const double du = fma(-x2, w, u), dv = fma(-y2, w, v);
    const double e = fma(du, du, dv * dv);
    return fabs(w) > V_W_EPS && e <= th2 * (w * w);
}

// every lane walks all m records (the same address in every lane)
__device__ __forceinline__ int count_all(const double (&h)[9], const double* __restrict__ rec, int m, double th2) {
    int c = 0;
#pragma unroll 4
    for (int i = 0; i < m; ++i) {
        const double2 a = *reinterpret_cast<const double2*>(rec + 4 * i);
        const double2 b = *reinterpret_cast<const double2*>(rec + 4 * i + 2);
        c += is_inlier(h, a.x, a.y, b.x, b.y, th2) ? 1 : 0;
    }
    return c;
}

// ---------------------------------------------------------------- DLT (the reference's, block-wide)
struct DltLds {
    double a[81];        // A^T W A, then its Jacobi iterate
    double v[81];        // eigenvectors (columns)
    double tmp[5 * 24];  // block_sum_d
};

// Point sources: n points, get(i, x1, y1, x2, y2, w) -> selected (SrcPoints: rr_ransac.h).
struct SrcInliers {      // the inliers of h among the records of a pair, weight 1
    const double* rec;
    int n;
    double h[9];
    double th2;
    __device__ __forceinline__ bool get(int i, double& x1, double& y1, double& x2, double& y2, double& w) const {
        const double2 a = *reinterpret_cast<const double2*>(rec + 4 * (long long)i);
        const double2 b = *reinterpret_cast<const double2*>(rec + 4 * (long long)i + 2);
        x1 = a.x; y1 = a.y; x2 = b.x; y2 = b.y; w = 1.0;
        return is_inlier(h, x1, y1, x2, y2, th2);
    }
};

// find_homography_dlt (homography.py:11-58) on the selected points of src; every thread of the
// block calls it and returns the same h.  false: fewer than 4 selected points (h untouched).
template <typename Src>
__device__ __forceinline__ bool dlt_block(const Src& src, DltLds& L, double (&h)[9]) {
    const int tid = threadIdx.x;
    double x1, y1, x2, y2, w;
    // normalize_points: mean, then sqrt(2) / (mean distance to it + eps)
    double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < src.n; i += V_TB)
        if (src.get(i, x1, y1, x2, y2, w)) { s5[0] += 1.0; s5[1] += x1; s5[2] += y1; s5[3] += x2; s5[4] += y2; }
    block_sum_d<5>(s5, L.tmp);
    const double cnt = s5[0];
    if (cnt < 4.0) return false;   // block-uniform
    const double mx1 = s5[1] / cnt, my1 = s5[2] / cnt, mx2 = s5[3] / cnt, my2 = s5[4] / cnt;
    double s2[2] = {0.0, 0.0};
    for (int i = tid; i < src.n; i += V_TB)
        if (src.get(i, x1, y1, x2, y2, w)) {
            const double ax = x1 - mx1, ay = y1 - my1, bx = x2 - mx2, by = y2 - my2;
            s2[0] += sqrt(ax * ax + ay * ay);
            s2[1] += sqrt(bx * bx + by * by);
        }
    block_sum_d<2>(s2, L.tmp);
    // the reference takes sqrt(2) from a float32 tensor: torch.sqrt(torch.tensor(2.))
    const double rt2 = (double)1.41421356237309504880f;
    const double sc1 = rt2 / (s2[0] / cnt + V_EPS), sc2 = rt2 / (s2[1] / cnt + V_EPS);
    const double tx1 = -sc1 * mx1, ty1 = -sc1 * my1, tx2 = -sc2 * mx2, ty2 = -sc2 * my2;
    // A^T W A of the rows ax / ay of homography.py:32-33 from S0, Sx, Sy, Sr (upper triangles of 3 x 3)
    double acc[24];
#pragma unroll
    for (int e = 0; e < 24; ++e) acc[e] = 0.0;
    for (int i = tid; i < src.n; i += V_TB)
        if (src.get(i, x1, y1, x2, y2, w)) {
            const double u2 = fma(sc2, x2, tx2), v2 = fma(sc2, y2, ty2);
            const double pt[3] = {fma(sc1, x1, tx1), fma(sc1, y1, ty1), 1.0};
            const double wx = w * u2, wy = w * v2, wr = w * (u2 * u2 + v2 * v2);
            int e = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = r; c < 3; ++c, ++e) {
                    const double pp = pt[r] * pt[c];
                    acc[e] = fma(w, pp, acc[e]);
                    acc[6 + e] = fma(wx, pp, acc[6 + e]);
                    acc[12 + e] = fma(wy, pp, acc[12 + e]);
                    acc[18 + e] = fma(wr, pp, acc[18 + e]);
                }
        }
    block_sum_d<24>(acc, L.tmp);
    __syncthreads();   // the previous call's readers of L.a / L.v are done
    if (tid == 0) {    // every thread holds the totals; one writes the symmetric matrix
        int e = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c, ++e) {
#pragma unroll
                for (int f = 0; f < 2; ++f) {   // (r, c) and its mirror
                    const int i = f ? c : r, j = f ? r : c;
                    L.a[9 * i + j] = acc[e];
                    L.a[9 * (3 + i) + 3 + j] = acc[e];
                    L.a[9 * i + 3 + j] = 0.0;
                    L.a[9 * (3 + i) + j] = 0.0;
                    L.a[9 * i + 6 + j] = -acc[6 + e];
                    L.a[9 * (6 + j) + i] = -acc[6 + e];
                    L.a[9 * (3 + i) + 6 + j] = -acc[12 + e];
                    L.a[9 * (6 + j) + 3 + i] = -acc[12 + e];
                    L.a[9 * (6 + i) + 6 + j] = acc[18 + e];
                }
            }
    }
    // the eigenvector of the smallest eigenvalue (ties: the lower index)
    double e9[9];
    jacobi_smallest9(L.a, L.v, e9);
    // H = T2^-1 (h T1) / (H[2][2] + eps)
    double g[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        g[3 * r] = e9[3 * r] * sc1;
        g[3 * r + 1] = e9[3 * r + 1] * sc1;
        g[3 * r + 2] = e9[3 * r] * tx1 + e9[3 * r + 1] * ty1 + e9[3 * r + 2];
    }
    const double i2 = 1.0 / sc2;
    double o[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = g[c] * i2 + mx2 * g[6 + c];
        o[3 + c] = g[3 + c] * i2 + my2 * g[6 + c];
        o[6 + c] = g[6 + c];
    }
    const double den = o[8] + V_EPS;
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = o[i] / den;
    return true;
}

// ---------------------------------------------------------------- kernels
__device__ __forceinline__ unsigned long long score_key64(int count, int t) {
    return ((unsigned long long)(unsigned)count << 32) | (unsigned long long)(0xffffffffu - (unsigned)t);
}

__global__ void __launch_bounds__(V_TB) k_verify_ransac(const double* __restrict__ rec, const long long* __restrict__ off1,
                                                        long long rows1, const int* __restrict__ cnt, int npairs,
                                                        int iters, int chunks, double th2, unsigned long long seed,
                                                        unsigned long long* __restrict__ best) {
    __shared__ __attribute__((aligned(16))) double s_rec[V_STAGE * 4];
    __shared__ unsigned long long s_red[4];
    const int tid = threadIdx.x;
    const int t = (int)blockIdx.x * V_TB + tid;
    for (int p = blockIdx.y; p < npairs; p += gridDim.y) {
        const int m = cnt[p];
        unsigned long long key = 0ull;
        if (m >= 4) {   // block-uniform
            long long b1, n1;
            pair_range(off1, p, rows1, b1, n1);
            const double* r = rec + 4 * b1;
            const bool staged = m <= V_STAGE;
            __syncthreads();   // the previous pair's readers of s_rec are done
            if (staged) {
                for (int i = tid; i < 2 * m; i += V_TB)
                    *reinterpret_cast<double2*>(s_rec + 2 * i) = *reinterpret_cast<const double2*>(r + 2 * i);
                __syncthreads();
            }
            if (t < iters) {
                int smp[4];
                draw4(seed, p, t, m, smp);
                double q[4][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double* s = staged ? s_rec + 4 * smp[j] : r + 4 * (long long)smp[j];
                    q[j][0] = s[0]; q[j][1] = s[1]; q[j][2] = s[2]; q[j][3] = s[3];
                }
                double h[9];
                if (h_from4(q, h)) {
                    const int c = staged ? count_all(h, s_rec, m, th2) : count_all(h, r, m, th2);
                    key = c > 0 ? score_key64(c, t) : 0ull;
                }
            }
        }
        key = block_max_u64(key, s_red);
        if (tid == 0) best[(long long)p * chunks + blockIdx.x] = key;
    }
}

// block-parallel inlier count of h over the m records of a pair
__device__ __forceinline__ int count_block(const double (&h)[9], const double* __restrict__ rec, int m, double th2, int* s4) {
    int c = 0;
    for (int i = threadIdx.x; i < m; i += V_TB) {
        const double2 a = *reinterpret_cast<const double2*>(rec + 4 * (long long)i);
        const double2 b = *reinterpret_cast<const double2*>(rec + 4 * (long long)i + 2);
        c += is_inlier(h, a.x, a.y, b.x, b.y, th2) ? 1 : 0;
    }
    return block_sum_i(c, s4);
}

// 3 blocks per CU (no scratch): while one wave of a block runs its Jacobi rotations the other blocks keep the CU busy
__global__ void __launch_bounds__(V_TB, 3) k_verify_refit(const float* __restrict__ kp1, const long long* __restrict__ off1,
                                                       long long rows1, const float* __restrict__ kp2,
                                                       const long long* __restrict__ off2, long long rows2,
                                                       const long long* __restrict__ match, int npairs, int max_n1,
                                                       const double* __restrict__ rec, const int* __restrict__ cnt,
                                                       const unsigned long long* __restrict__ best, int chunks,
                                                       double th2, int refine, unsigned long long seed,
                                                       int* __restrict__ inliers, double* __restrict__ Hout,
                                                       unsigned char* __restrict__ mask) {
    __shared__ DltLds L;
    __shared__ unsigned long long s_red[4];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x;
    for (int p = blockIdx.x; p < npairs; p += gridDim.x) {
        long long b1, n1, b2, n2;
        pair_range(off1, p, rows1, b1, n1);
        pair_range(off2, p, rows2, b2, n2);
        if (n1 > max_n1) n1 = max_n1;
        const int m = cnt[p];
        const double* r = rec + 4 * b1;
        unsigned long long key = 0ull;
        for (int c = tid; c < chunks; c += V_TB) {
            const unsigned long long k = best[(long long)p * chunks + c];
            key = k > key ? k : key;
        }
        key = block_max_u64(key, s_red);
        double h[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = 0.0;
        int count = 0;
        bool have = m >= 4 && key != 0ull;   // block-uniform
        if (have) {
            const int t = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
            int smp[4];
            draw4(seed, p, t, m, smp);
            double q[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double* s = r + 4 * (long long)smp[j];
                q[j][0] = s[0]; q[j][1] = s[1]; q[j][2] = s[2]; q[j][3] = s[3];
            }
            have = h_from4(q, h);
            if (have) count = count_block(h, r, m, th2, s_cnt);
            have = have && count > 0;
            for (int it = 0; have && it < refine; ++it) {
                SrcInliers src;
                src.rec = r; src.n = m; src.th2 = th2;
#pragma unroll
                for (int i = 0; i < 9; ++i) src.h[i] = h[i];
                double h2[9];
                if (!dlt_block(src, L, h2) || !all_finite9(h2)) break;
                const int c2 = count_block(h2, r, m, th2, s_cnt);
                if (c2 < count) break;
                count = c2;
#pragma unroll
                for (int i = 0; i < 9; ++i) h[i] = h2[i];
            }
        }
        if (!have) {
            count = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i) h[i] = 0.0;
        }
        if (tid == 0) {
            inliers[p] = count;
#pragma unroll
            for (int i = 0; i < 9; ++i) Hout[9 * (long long)p + i] = h[i];
        }
        // the mask straight from the rows: the same values and the same test as the records
        for (long long i = tid; i < n1; i += V_TB) {
            const long long j = match[b1 + i];
            bool in = false;
            if (have && j >= 0 && j < n2) {
                const float2 a = *reinterpret_cast<const float2*>(kp1 + 2 * (b1 + i));
                const float2 b = *reinterpret_cast<const float2*>(kp2 + 2 * (b2 + j));
                in = is_inlier(h, (double)a.x, (double)a.y, (double)b.x, (double)b.y, th2);
            }
            mask[b1 + i] = in ? 1 : 0;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(V_TB, 3) k_dlt_batch(const double* __restrict__ p1, const double* __restrict__ p2,
                                                    const double* __restrict__ wt, const long long* __restrict__ off,
                                                    long long rows, int npairs, double* __restrict__ Hout) {
    __shared__ DltLds L;
    for (int p = blockIdx.x; p < npairs; p += gridDim.x) {
        long long b, n;
        pair_range(off, p, rows, b, n);
        SrcPoints src;
        src.p1 = p1 + 2 * b; src.p2 = p2 + 2 * b; src.wt = wt ? wt + b : nullptr;
        src.n = (int)n;
        double h[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = 0.0;
        dlt_block(src, L, h);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) Hout[9 * (long long)p + i] = h[i];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- host
}  // namespace

}  // namespace rr

using namespace rr;

extern "C" {

size_t rr_verify_workspace_bytes(long long rows1, int npairs, int iters) { return measured(layout, rows1, npairs, iters); }

int rr_verify_pairs(const float* kp1, const long long* off1, long long rows1, const float* kp2, const long long* off2,
                    long long rows2, const long long* match, int npairs, int max_n1, double th, int iters, int refine,
                    unsigned long long seed, int* inliers, double* H, unsigned char* mask, void* workspace,
                    size_t workspace_bytes, void* stream) {
    const std::string w("rr_verify_pairs");
    if (npairs < 0 || rows1 < 0 || rows2 < 0 || max_n1 < 0) return fail(RR_EINVAL, w + ": negative size");
    if (iters < 1) return fail(RR_EINVAL, w + ": iters must be >= 1");
    if (iters > (1 << 24)) return fail(RR_EINVAL, w + ": iters above 2^24");
    if (refine < 0) return fail(RR_EINVAL, w + ": refine must be >= 0");
    if (!(th > 0.0) || !std::isfinite(th)) return fail(RR_EINVAL, w + ": th must be positive and finite");
    if (!off1 || !off2) return fail(RR_EINVAL, w + ": null offsets");
    if ((rows1 > 0 && (!kp1 || !match)) || (rows2 > 0 && !kp2)) return fail(RR_EINVAL, w + ": null keypoints or match");
    if ((((uintptr_t)kp1) & 7) || (((uintptr_t)kp2) & 7)) return fail(RR_EINVAL, w + ": keypoints must be 8-byte aligned");
    if (max_n1 > rows1) return fail(RR_EINVAL, w + ": max_n1 exceeds the row count");
    if (rows1 > 0x7fffffffll || rows2 > 0x7fffffffll) return fail(RR_EINVAL, w + ": too many rows");
    if (npairs > 0 && (rows1 > 0 && !mask)) return fail(RR_EINVAL, w + ": null output");
    if (npairs > 0 && (!inliers || !H)) return fail(RR_EINVAL, w + ": null output");
    Arena arena(workspace, workspace_bytes);
    const auto [rec, cnt, best] = layout(arena, rows1, npairs, iters);
    if (!workspace || !arena.fits()) return fail(RR_ENOSPACE, w + ": workspace too small");
    if (npairs == 0) return RR_OK;
    hipStream_t s = as_stream(stream);
    const int chunks = chunks_of(iters);
    const unsigned gp = (unsigned)(npairs < 65535 ? npairs : 65535);
    hipLaunchKernelGGL(k_verify_compact, dim3(gp), dim3(V_TB), 0, s, kp1, off1, rows1, kp2, off2, rows2, match, npairs,
                       max_n1, rec, cnt);
    int rc = check_launch("rr_verify_pairs: compact");
    if (rc) return rc;
    hipLaunchKernelGGL(k_verify_ransac, dim3((unsigned)chunks, gp), dim3(V_TB), 0, s, rec, off1, rows1, cnt, npairs, iters,
                       chunks, th * th, seed, best);
    rc = check_launch("rr_verify_pairs: ransac");
    if (rc) return rc;
    hipLaunchKernelGGL(k_verify_refit, dim3(gp), dim3(V_TB), 0, s, kp1, off1, rows1, kp2, off2, rows2, match, npairs,
                       max_n1, rec, cnt, best, chunks, th * th, refine, seed, inliers, H, mask);
    return check_launch("rr_verify_pairs: refit");
}

int rr_homography_dlt(const double* pts1, const double* pts2, const double* weights, const long long* off,
                      long long rows, int npairs, double* H, void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    const std::string w("rr_homography_dlt");
    if (npairs < 0 || rows < 0) return fail(RR_EINVAL, w + ": negative size");
    if (!off) return fail(RR_EINVAL, w + ": null offsets");
    if (rows > 0 && (!pts1 || !pts2)) return fail(RR_EINVAL, w + ": null points");
    if ((((uintptr_t)pts1) & 15) || (((uintptr_t)pts2) & 15)) return fail(RR_EINVAL, w + ": points must be 16-byte aligned");
    if (rows > 0x7fffffffll) return fail(RR_EINVAL, w + ": too many rows");
    if (npairs > 0 && !H) return fail(RR_EINVAL, w + ": null output");
    if (npairs == 0) return RR_OK;
    hipLaunchKernelGGL(k_dlt_batch, dim3((unsigned)(npairs < 65535 ? npairs : 65535)), dim3(V_TB), 0, as_stream(stream),
                       pts1, pts2, weights, off, rows, npairs, H);
    return check_launch("rr_homography_dlt");
}

}  // extern "C"
