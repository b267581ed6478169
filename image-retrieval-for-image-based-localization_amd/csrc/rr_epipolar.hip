// librr.so — epipolar verification: batched RANSAC fundamental matrix, the (weighted) 8-point fit
// and the epipolar distances.  The two-view counterpart of rr_verify.hip: it brings
// cirtorch/geometry/epipolar/fundamental.py:6-86 (normalize_points, normalize_transformation,
// find_fundamental) and metrics.py:4-83 (sampson_epipolar_distance, symmetrical_epipolar_distance)
// to the device and puts a seven-point RANSAC in front of them.  rr.h states every rule.
//
// Everything is float64 on float32 pixel keypoints, every sum has one fixed order, no atomic
// touches a floating-point value and nothing waits for the host.  Kernels of rr_verify_pairs_epipolar:
//
//   k_verify_compact  (rr_ransac.h) the kept matches of a pair become records (x1, y1, x2, y2).
//   k_epi_ransac      block (c, p) scores hypotheses t = 256 c .. 256 c + 255 of pair p, one per
//                     thread: seven sample indices by the counter hash, the seven-point solver in
//                     registers (f_from7: Hartley normalisation of the seven points, the 7 x 9
//                     system reduced to [I | B] by Gauss-Jordan with partial pivoting -- fully
//                     unrolled, static indices, a pivot is a chain of conditional row swaps --, the
//                     null space in the canonical basis, the cubic det(F2 + l (F1 - F2)) = 0, one
//                     or three roots), then ONE walk over the M_p records that scores all roots:
//                     each record is read once per hypothesis.  Records are staged in LDS up to
//                     V_STAGE and read from the workspace past it, as in k_verify_ransac.  The
//                     block's best (count desc, t asc, root asc) goes to best[p][c] as a 64-bit key.
//   k_epi_refit       one block per pair: the winner over the chunks, its F recomputed from
//                     (t, root), `refine` rounds of {inlier set S of F, the unweighted 8-point fit
//                     on S, accept while the count does not drop}; writes inliers, F (unit
//                     Frobenius norm, largest entry positive) and the side-1 mask.
//   k_fund_batch      rr_fundamental_dlt: the same 8-point routine on caller-supplied points.
//   k_epi_distance    rr_epipolar_distance.
//
// One residual routine (epi_terms) serves the RANSAC scorer, the refit, the mask and
// rr_epipolar_distance.  The 8-point routine (fund_block) is block-wide like dlt_block: three
// passes (means; mean distances; the 36 sums X^T W X = sum w (p2 p2^T) (x) (p1 p1^T) is made of),
// the 9 x 9 cyclic Jacobi of rr_ransac.h, then the rank-2 projection F - (F v3) v3^T with v3 from a
// 3 x 3 cyclic Jacobi on F^T F in registers (every thread the same).
//
// A result depends on nothing but the pair's own data, seed, p and t (block size 256 everywhere).
#include "rr_ransac.h"

namespace rr {

namespace {

// the reference takes sqrt(2) from a float32 tensor: torch.sqrt(torch.tensor(2.))
constexpr double E_RT2 = (double)1.41421356237309504880f;

// ---------------------------------------------------------------- the epipolar residual
// r = x2^T F x1, l = F x1 (the line in image 2), m = F^T x2 (the line in image 1):
// num = r^2, d1 = l0^2 + l1^2, d2 = m0^2 + m1^2.  Sampson^2 = num / (d1 + d2), symmetrical^2 =
// num (1 / d1 + 1 / d2) (metrics.py:33-38, :74-78).  Explicit fma: the same bits wherever it is inlined.
__device__ __forceinline__ void epi_terms(const double (&f)[9], double x1, double y1, double x2, double y2, double& num,
                                          double& d1, double& d2) {
    const double l0 = fma(f[0], x1, fma(f[1], y1, f[2]));
    const double l1 = fma(f[3], x1, fma(f[4], y1, f[5]));
    const double l2 = fma(f[6], x1, fma(f[7], y1, f[8]));
    const double m0 = fma(f[0], x2, fma(f[3], y2, f[6]));
    const double m1 = fma(f[1], x2, fma(f[4], y2, f[7]));
    const double r = fma(x2, l0, fma(y2, l1, l2));
    num = r * r;
    d1 = fma(l0, l0, l1 * l1);
    d2 = fma(m0, m0, m1 * m1);
}

// Sampson^2 <= th^2 without the division; den = 0 (or NaN) is never an inlier
__device__ __forceinline__ bool is_inlier_f(const double (&f)[9], double x1, double y1, double x2, double y2, double th2) {
    double num, d1, d2;
    epi_terms(f, x1, y1, x2, y2, num, d1, d2);
    const double den = d1 + d2;
    return den > 0.0 && num <= th2 * den;
}

// ---------------------------------------------------------------- seven-point solver
__device__ __forceinline__ double det3(double a0, double a1, double a2, double b0, double b1, double b2, double c0,
                                       double c1, double c2) {
    return a0 * (b1 * c2 - b2 * c1) - a1 * (b0 * c2 - b2 * c0) + a2 * (b0 * c1 - b1 * c0);
}

// real roots of c3 x^3 + c2 x^2 + c1 x + c0 in ascending order -> their number (0, 1 or 3); rr.h
// states the rule.  No root when c3 is 0 or anything is not finite.
__device__ __forceinline__ int cubic_roots(double c3, double c2, double c1, double c0, double (&x)[3]) {
    x[0] = x[1] = x[2] = 0.0;
    if (!(fabs(c3) > 0.0)) return 0;
    const double a = c2 / c3, b = c1 / c3, c = c0 / c3;
    const double Q = (a * a - 3.0 * b) / 9.0;
    const double R = (2.0 * a * a * a - 9.0 * a * b + 27.0 * c) / 54.0;
    const double Q3 = Q * Q * Q, R2 = R * R, a3 = a / 3.0;
    if (R2 < Q3) {   // three real roots
        const double ratio = fmin(1.0, fmax(-1.0, R / sqrt(Q3)));
        const double th = acos(ratio) / 3.0;   // in [0, pi / 3]
        const double m = -2.0 * sqrt(Q), ct = cos(th), st = sin(th);
        const double h = 0.86602540378443864676;   // sqrt(3) / 2
        // cos(th), cos(th - 2 pi / 3), cos(th + 2 pi / 3) are descending, m < 0: the roots ascend
        x[0] = m * ct - a3;
        x[1] = m * (h * st - 0.5 * ct) - a3;
        x[2] = m * (-h * st - 0.5 * ct) - a3;
        return 3;
    }
    if (!(R2 >= Q3)) return 0;   // NaN
    const double A = -copysign(cbrt(fabs(R) + sqrt(R2 - Q3)), R);
    const double B = A != 0.0 ? Q / A : 0.0;
    x[0] = (A + B) - a3;
    return isfinite(x[0]) ? 1 : 0;
}

// Hartley normalisation of the seven points of one side: u = s x + tx, v = s y + ty
__device__ __forceinline__ void norm7(const double (&x)[7], const double (&y)[7], double& s, double& tx, double& ty) {
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) { sx += x[j]; sy += y[j]; }
    const double mx = sx / 7.0, my = sy / 7.0;
    double sd = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double ax = x[j] - mx, ay = y[j] - my;
        sd += sqrt(ax * ax + ay * ay);
    }
    s = E_RT2 / (sd / 7.0 + V_EPS);
    tx = -s * mx;
    ty = -s * my;
}

// The fundamental matrices through seven records r[j] = (x1, y1, x2, y2): F[k], k < the number
// returned, in ascending root order; the others (and a root with a non-finite entry) are all zero,
// which never has an inlier.  Everything is statically indexed after unrolling: registers only.
__device__ __forceinline__ int f_from7(const double (&r)[7][4], double (&F)[3][9]) {
    double s1, tx1, ty1, s2, tx2, ty2;
    {
        double xa[7], ya[7], xb[7], yb[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) { xa[j] = r[j][0]; ya[j] = r[j][1]; xb[j] = r[j][2]; yb[j] = r[j][3]; }
        norm7(xa, ya, s1, tx1, ty1);
        norm7(xb, yb, s2, tx2, ty2);
    }
    // the 7 x 9 system, rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1] (fundamental.py:69)
    double A[7][9];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double x1 = fma(s1, r[j][0], tx1), y1 = fma(s1, r[j][1], ty1);
        const double x2 = fma(s2, r[j][2], tx2), y2 = fma(s2, r[j][3], ty2);
        A[j][0] = x2 * x1; A[j][1] = x2 * y1; A[j][2] = x2;
        A[j][3] = y2 * x1; A[j][4] = y2 * y1; A[j][5] = y2;
        A[j][6] = x1;      A[j][7] = y1;      A[j][8] = 1.0;
    }
    // Gauss-Jordan on columns 0..6 with partial pivoting -> [I | B]
#pragma unroll
    for (int c = 0; c < 7; ++c) {
#pragma unroll
        for (int i = c + 1; i < 7; ++i) {   // the largest |A[i][c]|, i >= c, ends in row c
            const bool sw = fabs(A[i][c]) > fabs(A[c][c]);
#pragma unroll
            for (int k = c; k < 9; ++k) {
                const double u = A[c][k], v = A[i][k];
                A[c][k] = sw ? v : u;
                A[i][k] = sw ? u : v;
            }
        }
        const double inv = 1.0 / A[c][c];
#pragma unroll
        for (int k = c + 1; k < 9; ++k) A[c][k] *= inv;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            if (i == c) continue;
            const double g = A[i][c];
#pragma unroll
            for (int k = c + 1; k < 9; ++k) A[i][k] = fma(-g, A[c][k], A[i][k]);
        }
    }
    // the null vectors with last two entries (1, 0) and (0, 1); D = F1 - F2
    double f2[9], d[9];
#pragma unroll
    for (int i = 0; i < 7; ++i) { f2[i] = -A[i][8]; d[i] = A[i][8] - A[i][7]; }
    f2[7] = 0.0; f2[8] = 1.0;
    d[7] = 1.0;  d[8] = -1.0;
    // det(F2 + l D) = c0 + c1 l + c2 l^2 + c3 l^3: rows of F2 replaced by rows of D, one, two, three at a time
    const double c0 = det3(f2[0], f2[1], f2[2], f2[3], f2[4], f2[5], f2[6], f2[7], f2[8]);
    const double c1 = det3(d[0], d[1], d[2], f2[3], f2[4], f2[5], f2[6], f2[7], f2[8]) +
                      det3(f2[0], f2[1], f2[2], d[3], d[4], d[5], f2[6], f2[7], f2[8]) +
                      det3(f2[0], f2[1], f2[2], f2[3], f2[4], f2[5], d[6], d[7], d[8]);
    const double c2 = det3(f2[0], f2[1], f2[2], d[3], d[4], d[5], d[6], d[7], d[8]) +
                      det3(d[0], d[1], d[2], f2[3], f2[4], f2[5], d[6], d[7], d[8]) +
                      det3(d[0], d[1], d[2], d[3], d[4], d[5], f2[6], f2[7], f2[8]);
    const double c3 = det3(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8]);
    double lam[3];
    const int nr = cubic_roots(c3, c2, c1, c0, lam);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double g[9], h[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) g[i] = fma(lam[k], d[i], f2[i]);
        // T2^T (G T1)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            h[3 * i] = g[3 * i] * s1;
            h[3 * i + 1] = g[3 * i + 1] * s1;
            h[3 * i + 2] = fma(g[3 * i], tx1, fma(g[3 * i + 1], ty1, g[3 * i + 2]));
        }
        bool ok = k < nr;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            g[j] = h[j] * s2;
            g[3 + j] = h[3 + j] * s2;
            g[6 + j] = fma(h[j], tx2, fma(h[3 + j], ty2, h[6 + j]));
        }
        ok = ok && all_finite9(g);
#pragma unroll
        for (int i = 0; i < 9; ++i) F[k][i] = ok ? g[i] : 0.0;
    }
    return nr;
}

// seven records of hypothesis t of pair p
__device__ __forceinline__ void sample7(const double* __restrict__ rec, unsigned long long seed, int p, int t, int m,
                                        double (&q)[7][4]) {
    int smp[7];
    draw_n<7>(seed, p, t, m, smp);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double2 a = *reinterpret_cast<const double2*>(rec + 4 * (long long)smp[j]);
        const double2 b = *reinterpret_cast<const double2*>(rec + 4 * (long long)smp[j] + 2);
        q[j][0] = a.x; q[j][1] = a.y; q[j][2] = b.x; q[j][3] = b.y;
    }
}

// ---------------------------------------------------------------- scoring
// every lane walks all m records once (the same address in every lane) and scores the three roots
__device__ __forceinline__ void count_roots(const double (&F)[3][9], const double* __restrict__ rec, int m, double th2,
                                            int (&c)[3]) {
    c[0] = c[1] = c[2] = 0;
#pragma unroll 2
    for (int i = 0; i < m; ++i) {
        const double2 a = *reinterpret_cast<const double2*>(rec + 4 * i);
        const double2 b = *reinterpret_cast<const double2*>(rec + 4 * i + 2);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] += is_inlier_f(F[k], a.x, a.y, b.x, b.y, th2) ? 1 : 0;
    }
}

// (count desc, t asc, root asc) as one integer: t < 2^24, root < 4
__device__ __forceinline__ unsigned long long epi_key(int count, int t, int root) {
    return ((unsigned long long)(unsigned)count << 32) | (unsigned long long)(0xffffffffu - (unsigned)(4 * t + root));
}

__global__ void __launch_bounds__(V_TB) k_epi_ransac(const double* __restrict__ rec, const long long* __restrict__ off1,
                                                     long long rows1, const int* __restrict__ cnt, int npairs, int iters,
                                                     int chunks, double th2, unsigned long long seed,
                                                     unsigned long long* __restrict__ best) {
    __shared__ __attribute__((aligned(16))) double s_rec[V_STAGE * 4];
    __shared__ unsigned long long s_red[4];
    const int tid = threadIdx.x;
    const int t = (int)blockIdx.x * V_TB + tid;
    for (int p = blockIdx.y; p < npairs; p += gridDim.y) {
        const int m = cnt[p];
        unsigned long long key = 0ull;
        if (m >= 7) {   // block-uniform
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
                const double* src = staged ? s_rec : r;
                double q[7][4];
                sample7(src, seed, p, t, m, q);
                double F[3][9];
                if (f_from7(q, F) > 0) {
                    int c[3];
                    count_roots(F, src, m, th2, c);
#pragma unroll
                    for (int k = 2; k >= 0; --k) {
                        const unsigned long long kk = c[k] > 0 ? epi_key(c[k], t, k) : 0ull;
                        key = kk > key ? kk : key;
                    }
                }
            }
        }
        key = block_max_u64(key, s_red);
        if (tid == 0) best[(long long)p * chunks + blockIdx.x] = key;
    }
}

// ---------------------------------------------------------------- the 8-point fit, block-wide
struct FundLds {
    double a[81];        // X^T W X, then its Jacobi iterate
    double v[81];        // eigenvectors (columns)
    double tmp[5 * 36];  // block_sum_d
};

struct SrcInliersF {     // the inliers of f among the records of a pair, weight 1
    const double* rec;
    int n;
    double f[9];
    double th2;
    __device__ __forceinline__ bool get(int i, double& x1, double& y1, double& x2, double& y2, double& w) const {
        const double2 a = *reinterpret_cast<const double2*>(rec + 4 * (long long)i);
        const double2 b = *reinterpret_cast<const double2*>(rec + 4 * (long long)i + 2);
        x1 = a.x; y1 = a.y; x2 = b.x; y2 = b.y; w = 1.0;
        return is_inlier_f(f, x1, y1, x2, y2, th2);
    }
};

// f <- f - (f v3) v3^T, v3 the eigenvector of the smallest eigenvalue of f^T f (ties: the lower
// index): the reference's U diag(s1, s2, 0) V^T without a full SVD
__device__ __forceinline__ void rank2(double (&f)[9]) {
    double g[9], v[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            g[3 * i + j] = fma(f[i], f[j], fma(f[3 + i], f[3 + j], f[6 + i] * f[6 + j]));
            v[3 * i + j] = i == j ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sweep = 0; sweep < V_SWEEPS; ++sweep) {
        const bool r0 = rot3<0, 1>(g, v);
        const bool r1 = rot3<0, 2>(g, v);
        const bool r2 = rot3<1, 2>(g, v);
        if (!(r0 || r1 || r2)) break;
    }
    const bool m1 = g[4] < g[0];
    const double b01 = m1 ? g[4] : g[0];
    const bool m2 = g[8] < b01;
    double v3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v3[k] = m2 ? v[3 * k + 2] : (m1 ? v[3 * k + 1] : v[3 * k]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double w = fma(f[3 * i], v3[0], fma(f[3 * i + 1], v3[1], f[3 * i + 2] * v3[2]));
#pragma unroll
        for (int j = 0; j < 3; ++j) f[3 * i + j] = fma(-w, v3[j], f[3 * i + j]);
    }
}

// find_fundamental (fundamental.py:49-86) on the selected points of src; every thread of the block
// calls it and returns the same f.  false: fewer than 8 selected points (f untouched).
template <typename Src>
__device__ __forceinline__ bool fund_block(const Src& src, FundLds& L, double (&f)[9]) {
    const int tid = threadIdx.x;
    double x1, y1, x2, y2, w;
    // normalize_points: mean, then sqrt(2) / (mean distance to it + eps)
    double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < src.n; i += V_TB)
        if (src.get(i, x1, y1, x2, y2, w)) { s5[0] += 1.0; s5[1] += x1; s5[2] += y1; s5[3] += x2; s5[4] += y2; }
    block_sum_d<5>(s5, L.tmp);
    const double cnt = s5[0];
    if (cnt < 8.0) return false;   // block-uniform
    const double mx1 = s5[1] / cnt, my1 = s5[2] / cnt, mx2 = s5[3] / cnt, my2 = s5[4] / cnt;
    double sd[2] = {0.0, 0.0};
    for (int i = tid; i < src.n; i += V_TB)
        if (src.get(i, x1, y1, x2, y2, w)) {
            const double ax = x1 - mx1, ay = y1 - my1, bx = x2 - mx2, by = y2 - my2;
            sd[0] += sqrt(ax * ax + ay * ay);
            sd[1] += sqrt(bx * bx + by * by);
        }
    block_sum_d<2>(sd, L.tmp);
    const double sc1 = E_RT2 / (sd[0] / cnt + V_EPS), sc2 = E_RT2 / (sd[1] / cnt + V_EPS);
    const double tx1 = -sc1 * mx1, ty1 = -sc1 * my1, tx2 = -sc2 * mx2, ty2 = -sc2 * my2;
    // X^T W X = sum w (p2 p2^T) (x) (p1 p1^T): acc[6 e2 + e1], e the upper-triangle index of a 3 x 3
    double acc[36];
#pragma unroll
    for (int e = 0; e < 36; ++e) acc[e] = 0.0;
    for (int i = tid; i < src.n; i += V_TB)
        if (src.get(i, x1, y1, x2, y2, w)) {
            const double p1[3] = {fma(sc1, x1, tx1), fma(sc1, y1, ty1), 1.0};
            const double p2[3] = {fma(sc2, x2, tx2), fma(sc2, y2, ty2), 1.0};
            double q1[6], q2[6];
            int e = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = r; c < 3; ++c, ++e) {
                    q1[e] = p1[r] * p1[c];
                    q2[e] = w * (p2[r] * p2[c]);
                }
#pragma unroll
            for (int e2 = 0; e2 < 6; ++e2)
#pragma unroll
                for (int e1 = 0; e1 < 6; ++e1) acc[6 * e2 + e1] = fma(q2[e2], q1[e1], acc[6 * e2 + e1]);
        }
    block_sum_d<36>(acc, L.tmp);
    __syncthreads();   // the previous call's readers of L.a / L.v are done
    if (tid < 81) {    // every thread holds the totals: entry (3 a + b, 3 c + d) = (p2 p2^T)[a][c] (p1 p1^T)[b][d]
        constexpr int TRI[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
        const int row = tid / 9, col = tid - 9 * row;
        const int e = 6 * TRI[3 * (row / 3) + col / 3] + TRI[3 * (row % 3) + col % 3];
        double val = 0.0;
#pragma unroll
        for (int k = 0; k < 36; ++k) val = e == k ? acc[k] : val;   // static indices: acc stays in registers
        L.a[tid] = val;
    }
    double e9[9];
    jacobi_smallest9(L.a, L.v, e9);
    rank2(e9);
    // F = T2^T (f T1), then normalize_transformation
    double g[9], o[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        g[3 * r] = e9[3 * r] * sc1;
        g[3 * r + 1] = e9[3 * r + 1] * sc1;
        g[3 * r + 2] = e9[3 * r] * tx1 + e9[3 * r + 1] * ty1 + e9[3 * r + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = g[c] * sc2;
        o[3 + c] = g[3 + c] * sc2;
        o[6 + c] = g[c] * tx2 + g[3 + c] * ty2 + g[6 + c];
    }
    const bool div = fabs(o[8]) > V_EPS;
    const double den = o[8] + V_EPS;
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = div ? o[i] / den : o[i];
    return true;
}

// block-parallel inlier count of f over the m records of a pair
__device__ __forceinline__ int count_block_f(const double (&f)[9], const double* __restrict__ rec, int m, double th2,
                                             int* s4) {
    int c = 0;
    for (int i = threadIdx.x; i < m; i += V_TB) {
        const double2 a = *reinterpret_cast<const double2*>(rec + 4 * (long long)i);
        const double2 b = *reinterpret_cast<const double2*>(rec + 4 * (long long)i + 2);
        c += is_inlier_f(f, a.x, a.y, b.x, b.y, th2) ? 1 : 0;
    }
    return block_sum_i(c, s4);
}

__global__ void __launch_bounds__(V_TB) k_epi_refit(const float* __restrict__ kp1, const long long* __restrict__ off1,
                                                    long long rows1, const float* __restrict__ kp2,
                                                    const long long* __restrict__ off2, long long rows2,
                                                    const long long* __restrict__ match, int npairs, int max_n1,
                                                    const double* __restrict__ rec, const int* __restrict__ cnt,
                                                    const unsigned long long* __restrict__ best, int chunks, double th2,
                                                    int refine, unsigned long long seed, int* __restrict__ inliers,
                                                    double* __restrict__ Fout, unsigned char* __restrict__ mask) {
    __shared__ FundLds L;
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
        double f[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) f[i] = 0.0;
        int count = 0;
        bool have = m >= 7 && key != 0ull;   // block-uniform
        if (have) {
            const unsigned tr = 0xffffffffu - (unsigned)(key & 0xffffffffull);
            const int t = (int)(tr >> 2), root = (int)(tr & 3u);
            {
                double q[7][4];
                sample7(r, seed, p, t, m, q);
                double F[3][9];
                f_from7(q, F);
#pragma unroll
                for (int i = 0; i < 9; ++i) f[i] = root == 0 ? F[0][i] : (root == 1 ? F[1][i] : F[2][i]);
            }
            count = count_block_f(f, r, m, th2, s_cnt);
            have = count > 0;
            for (int it = 0; have && it < refine; ++it) {
                SrcInliersF src;
                src.rec = r; src.n = m; src.th2 = th2;
#pragma unroll
                for (int i = 0; i < 9; ++i) src.f[i] = f[i];
                double f2[9];
                if (!fund_block(src, L, f2) || !all_finite9(f2)) break;
                const int c2 = count_block_f(f2, r, m, th2, s_cnt);
                if (c2 < count) break;
                count = c2;
#pragma unroll
                for (int i = 0; i < 9; ++i) f[i] = f2[i];
            }
        }
        if (!have) {
            count = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i) f[i] = 0.0;
        }
        if (tid == 0) {
            inliers[p] = count;
            // unit Frobenius norm, the entry of largest magnitude (the lowest index among equals) positive
            double ss = 0.0, big = 0.0, sign = 1.0;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                ss = fma(f[i], f[i], ss);
                if (fabs(f[i]) > big) { big = fabs(f[i]); sign = f[i] < 0.0 ? -1.0 : 1.0; }
            }
            const double nrm = have ? sign * sqrt(ss) : 1.0;
#pragma unroll
            for (int i = 0; i < 9; ++i) Fout[9 * (long long)p + i] = have ? f[i] / nrm : 0.0;
        }
        // the mask straight from the rows: the same values and the same test as the records
        for (long long i = tid; i < n1; i += V_TB) {
            const long long j = match[b1 + i];
            bool in = false;
            if (have && j >= 0 && j < n2) {
                const float2 a = *reinterpret_cast<const float2*>(kp1 + 2 * (b1 + i));
                const float2 b = *reinterpret_cast<const float2*>(kp2 + 2 * (b2 + j));
                in = is_inlier_f(f, (double)a.x, (double)a.y, (double)b.x, (double)b.y, th2);
            }
            mask[b1 + i] = in ? 1 : 0;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(V_TB) k_fund_batch(const double* __restrict__ p1, const double* __restrict__ p2,
                                                     const double* __restrict__ wt, const long long* __restrict__ off,
                                                     long long rows, int npairs, double* __restrict__ Fout) {
    __shared__ FundLds L;
    for (int p = blockIdx.x; p < npairs; p += gridDim.x) {
        long long b, n;
        pair_range(off, p, rows, b, n);
        SrcPoints src;
        src.p1 = p1 + 2 * b; src.p2 = p2 + 2 * b; src.wt = wt ? wt + b : nullptr;
        src.n = (int)n;
        double f[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) f[i] = 0.0;
        fund_block(src, L, f);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) Fout[9 * (long long)p + i] = f[i];
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(V_TB) k_epi_distance(const double* __restrict__ p1, const double* __restrict__ p2,
                                                       const double* __restrict__ Fm, const long long* __restrict__ off,
                                                       long long rows, int npairs, int kind, int squared, double eps,
                                                       double* __restrict__ out) {
    for (int p = blockIdx.x; p < npairs; p += gridDim.x) {
        long long b, n;
        pair_range(off, p, rows, b, n);
        double f[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) f[i] = Fm[9 * (long long)p + i];
        for (long long i = threadIdx.x; i < n; i += V_TB) {
            const double2 a = *reinterpret_cast<const double2*>(p1 + 2 * (b + i));
            const double2 c = *reinterpret_cast<const double2*>(p2 + 2 * (b + i));
            double num, d1, d2;
            epi_terms(f, a.x, a.y, c.x, c.y, num, d1, d2);
            double v = kind == RR_EPI_SAMPSON ? num / (d1 + d2) : num * (1.0 / d1 + 1.0 / d2);
            if (!squared) v = sqrt(v + eps);
            out[b + i] = v;
        }
    }
}

}  // namespace

}  // namespace rr

using namespace rr;

extern "C" {

size_t rr_verify_epipolar_workspace_bytes(long long rows1, int npairs, int iters) {
    return measured(layout, rows1, npairs, iters);
}

int rr_verify_pairs_epipolar(const float* kp1, const long long* off1, long long rows1, const float* kp2,
                             const long long* off2, long long rows2, const long long* match, int npairs, int max_n1,
                             double th, int iters, int refine, unsigned long long seed, int* inliers, double* F,
                             unsigned char* mask, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string w("rr_verify_pairs_epipolar");
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
    if (npairs > 0 && (!inliers || !F)) return fail(RR_EINVAL, w + ": null output");
    Arena arena(workspace, workspace_bytes);
    const auto [rec, cnt, best] = layout(arena, rows1, npairs, iters);
    if (!workspace || !arena.fits()) return fail(RR_ENOSPACE, w + ": workspace too small");
    if (npairs == 0) return RR_OK;
    hipStream_t s = as_stream(stream);
    const int chunks = chunks_of(iters);
    const unsigned gp = (unsigned)(npairs < 65535 ? npairs : 65535);
    hipLaunchKernelGGL(k_verify_compact, dim3(gp), dim3(V_TB), 0, s, kp1, off1, rows1, kp2, off2, rows2, match, npairs,
                       max_n1, rec, cnt);
    int rc = check_launch("rr_verify_pairs_epipolar: compact");
    if (rc) return rc;
    hipLaunchKernelGGL(k_epi_ransac, dim3((unsigned)chunks, gp), dim3(V_TB), 0, s, rec, off1, rows1, cnt, npairs, iters,
                       chunks, th * th, seed, best);
    rc = check_launch("rr_verify_pairs_epipolar: ransac");
    if (rc) return rc;
    hipLaunchKernelGGL(k_epi_refit, dim3(gp), dim3(V_TB), 0, s, kp1, off1, rows1, kp2, off2, rows2, match, npairs, max_n1,
                       rec, cnt, best, chunks, th * th, refine, seed, inliers, F, mask);
    return check_launch("rr_verify_pairs_epipolar: refit");
}

int rr_fundamental_dlt(const double* pts1, const double* pts2, const double* weights, const long long* off,
                       long long rows, int npairs, double* F, void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    const std::string w("rr_fundamental_dlt");
    if (npairs < 0 || rows < 0) return fail(RR_EINVAL, w + ": negative size");
    if (!off) return fail(RR_EINVAL, w + ": null offsets");
    if (rows > 0 && (!pts1 || !pts2)) return fail(RR_EINVAL, w + ": null points");
    if ((((uintptr_t)pts1) & 15) || (((uintptr_t)pts2) & 15)) return fail(RR_EINVAL, w + ": points must be 16-byte aligned");
    if (rows > 0x7fffffffll) return fail(RR_EINVAL, w + ": too many rows");
    if (npairs > 0 && !F) return fail(RR_EINVAL, w + ": null output");
    if (npairs == 0) return RR_OK;
    hipLaunchKernelGGL(k_fund_batch, dim3((unsigned)(npairs < 65535 ? npairs : 65535)), dim3(V_TB), 0, as_stream(stream),
                       pts1, pts2, weights, off, rows, npairs, F);
    return check_launch("rr_fundamental_dlt");
}

int rr_epipolar_distance(const double* pts1, const double* pts2, const double* F, const long long* off, long long rows,
                         int npairs, int kind, int squared, double eps, double* out, void* stream) {
    const std::string w("rr_epipolar_distance");
    if (npairs < 0 || rows < 0) return fail(RR_EINVAL, w + ": negative size");
    if (kind != RR_EPI_SAMPSON && kind != RR_EPI_SYMMETRICAL) return fail(RR_EINVAL, w + ": unknown kind");
    if (squared != 0 && squared != 1) return fail(RR_EINVAL, w + ": squared must be 0 or 1");
    if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(RR_EINVAL, w + ": eps must be >= 0 and finite");
    if (!off) return fail(RR_EINVAL, w + ": null offsets");
    if (rows > 0 && (!pts1 || !pts2 || !out)) return fail(RR_EINVAL, w + ": null points or output");
    if ((((uintptr_t)pts1) & 15) || (((uintptr_t)pts2) & 15)) return fail(RR_EINVAL, w + ": points must be 16-byte aligned");
    if (rows > 0x7fffffffll) return fail(RR_EINVAL, w + ": too many rows");
    if (npairs > 0 && !F) return fail(RR_EINVAL, w + ": null F");
    if (npairs == 0) return RR_OK;
    hipLaunchKernelGGL(k_epi_distance, dim3((unsigned)(npairs < 65535 ? npairs : 65535)), dim3(V_TB), 0, as_stream(stream),
                       pts1, pts2, F, off, rows, npairs, kind, squared, eps, out);
    return check_launch("rr_epipolar_distance");
}

}  // extern "C"
