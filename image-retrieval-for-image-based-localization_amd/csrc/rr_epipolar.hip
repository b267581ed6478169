// librr.so — epipolar verification: batched RANSAC fundamental matrix, the (weighted) 8-point fit
// and the epipolar distances.  The two-view counterpart of rr_verify.hip: it brings
// cirtorch/geometry/epipolar/fundamental.py:6-86 (normalize_points, normalize_transformation,
// find_fundamental) and metrics.py:4-83 (sampson_epipolar_distance, symmetrical_epipolar_distance)
// to the device and puts a seven-point RANSAC in front of them.  rr.h states every rule.
//
// Everything is float64 on float32 pixel keypoints, every sum has one fixed order, no atomic
// touches a floating-point value and nothing waits for the host.  This file holds the model
// (struct Fundamental) and k_epi_distance; the other kernels are the skeleton of rr_ransac.h
// instantiated for it:
//
//   k_verify_compact  (rr_ransac.h) the kept matches of a pair become records (x1, y1, x2, y2).
//   k_ransac<F>       block (c, p) scores hypotheses t = 256 c .. 256 c + 255 of pair p, one per
//                     thread: seven sample indices by the counter hash, the seven-point solver in
//                     registers (f_from7: Hartley normalisation of the seven points, the 7 x 9
//                     system reduced to [I | B] by Gauss-Jordan with partial pivoting -- fully
//                     unrolled, static indices, a pivot is a chain of conditional row swaps --, the
//                     null space in the canonical basis, the cubic det(F2 + l (F1 - F2)) = 0, one
//                     or three roots), then ONE walk over the M_p records that scores all roots:
//                     each record is read once per hypothesis.  Records are staged in LDS up to
//                     V_STAGE and read from the workspace past it, as for the homography.  The
//                     block's best (count desc, t asc, root asc) goes to best[p][c] as a 64-bit key.
//   k_refit<F>        one block per pair: the winner over the chunks, its F recomputed from
//                     (t, root), `refine` rounds of {inlier set S of F, the unweighted 8-point fit
//                     on S, accept while the count does not drop}; writes inliers, F (unit
//                     Frobenius norm, largest entry positive) and the side-1 mask.
//   k_fit_batch<F>    rr_fundamental_dlt: the same 8-point routine on caller-supplied points.
//   k_epi_distance    rr_epipolar_distance.
//   k_ransac<E>, k_refit<E>   the same two kernels for struct Essential (rr_verify_pairs_essential): the
//                     pair's intrinsics are its context (K, K^-1 of both views, loaded once per pair),
//                     a hypothesis is a five-point sample solved by rr_fivepoint.h (up to ten roots,
//                     scored in one walk as F = K2^-T E K1^-1 with the residual routine below), the
//                     refit is the 8-point fit projected onto the essential matrices.
//   k_essential_5pt   rr_essential_5pt: the five-point solver alone, a thread per sample.
//
// One residual routine (epi_terms) serves the RANSAC scorer, the refit, the mask and
// rr_epipolar_distance.  The 8-point routine (fit_block<Fundamental>) is block-wide like the DLT: three
// passes (means; mean distances; the 36 sums X^T W X = sum w (p2 p2^T) (x) (p1 p1^T) is made of),
// the 9 x 9 cyclic Jacobi of rr_ransac.h, then the rank-2 projection F - (F v3) v3^T with v3 from a
// 3 x 3 cyclic Jacobi on F^T F in registers (every thread the same).
//
// A result depends on nothing but the pair's own data, seed, p and t (block size 256 everywhere).
#include "rr_ransac.h"
#include "rr_fivepoint.h"

namespace rr {

namespace {

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
    s = V_RT2 / (sd / 7.0 + V_EPS);
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

// ---------------------------------------------------------------- the model (rr_ransac.h states what a model provides)
struct Fundamental {
    // a key holds 4 t + root; every root of a sample is scored in ONE walk over a generic pointer
    static constexpr int SAMPLE = 7, FIT_MIN = 8, ROOTS = 3, KEY_SLOTS = 4, ACC = 36, WALK_UNROLL = 2;
    static constexpr bool WALK_SPLIT = false;
    static constexpr bool TRUST_ROOT = true;   // the refit does not count the roots again: the key's root was scored from the same records
    static constexpr int REFIT_OCC = 1;   // no bound: the refit holds 244 VGPRs, the batch fit 193

    struct Ctx {};   // a pair is its records
    static __device__ __forceinline__ Ctx load(const double*, const double*, int) { return {}; }

    static __device__ __forceinline__ int hypotheses(const Ctx&, const double (&q)[7][4], double (&F)[3][9]) { return f_from7(q, F); }
    static __device__ __forceinline__ bool inlier(const double (&f)[9], double x1, double y1, double x2, double y2, double th2) {
        return is_inlier_f(f, x1, y1, x2, y2, th2);
    }

    // find_fundamental (fundamental.py:49-86): X^T W X = sum w (p2 p2^T) (x) (p1 p1^T): acc[6 e2 + e1],
    // e the upper-triangle index of a 3 x 3
    static __device__ __forceinline__ void accumulate(const FitNorm& n, double x1, double y1, double x2, double y2, double w,
                                                      double (&acc)[36]) {
        const double p1[3] = {fma(n.sc1, x1, n.tx1), fma(n.sc1, y1, n.ty1), 1.0};
        const double p2[3] = {fma(n.sc2, x2, n.tx2), fma(n.sc2, y2, n.ty2), 1.0};
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

    // entry (3 a + b, 3 c + d) = (p2 p2^T)[a][c] (p1 p1^T)[b][d], one thread each
    static __device__ __forceinline__ void write_matrix(const double (&acc)[36], double* a) {
        const int tid = threadIdx.x;
        if (tid < 81) {
            constexpr int TRI[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
            const int row = tid / 9, col = tid - 9 * row;
            const int e = 6 * TRI[3 * (row / 3) + col / 3] + TRI[3 * (row % 3) + col % 3];
            double val = 0.0;
#pragma unroll
            for (int k = 0; k < 36; ++k) val = e == k ? acc[k] : val;   // static indices: acc stays in registers
            a[tid] = val;
        }
    }

    // rank 2, F = T2^T (f T1), then normalize_transformation
    static __device__ __forceinline__ void finish(const Ctx&, double (&e9)[9], const FitNorm& n, double (&f)[9]) {
        rank2(e9);
        double g[9], o[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            g[3 * r] = e9[3 * r] * n.sc1;
            g[3 * r + 1] = e9[3 * r + 1] * n.sc1;
            g[3 * r + 2] = e9[3 * r] * n.tx1 + e9[3 * r + 1] * n.ty1 + e9[3 * r + 2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[c] = g[c] * n.sc2;
            o[3 + c] = g[3 + c] * n.sc2;
            o[6 + c] = g[c] * n.tx2 + g[3 + c] * n.ty2 + g[6 + c];
        }
        const bool div = fabs(o[8]) > V_EPS;
        const double den = o[8] + V_EPS;
#pragma unroll
        for (int i = 0; i < 9; ++i) f[i] = div ? o[i] / den : o[i];
    }

    // unit Frobenius norm, the entry of largest magnitude (the lowest index among equals) positive
    static __device__ __forceinline__ void emit(const Ctx&, bool have, const double (&f)[9], double* __restrict__ out) {
        double ss = 0.0, big = 0.0, sign = 1.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            ss = fma(f[i], f[i], ss);
            if (fabs(f[i]) > big) { big = fabs(f[i]); sign = f[i] < 0.0 ? -1.0 : 1.0; }
        }
        const double nrm = have ? sign * sqrt(ss) : 1.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] = have ? f[i] / nrm : 0.0;
    }
};

// ---------------------------------------------------------------- the calibrated model
// o = a^T b, o = a b (3 x 3 row-major)
__device__ __forceinline__ void mat3_atb(const double (&a)[9], const double (&b)[9], double (&o)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = fma(a[i], b[j], fma(a[3 + i], b[3 + j], a[6 + i] * b[6 + j]));
}
__device__ __forceinline__ void mat3_ab(const double (&a)[9], const double (&b)[9], double (&o)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = fma(a[3 * i], b[j], fma(a[3 * i + 1], b[3 + j], a[3 * i + 2] * b[6 + j]));
}

// inverse by the adjugate -> det
__device__ __forceinline__ double inv3(const double (&a)[9], double (&o)[9]) {
    double c[9];
    c[0] = a[4] * a[8] - a[5] * a[7]; c[1] = a[2] * a[7] - a[1] * a[8]; c[2] = a[1] * a[5] - a[2] * a[4];
    c[3] = a[5] * a[6] - a[3] * a[8]; c[4] = a[0] * a[8] - a[2] * a[6]; c[5] = a[2] * a[3] - a[0] * a[5];
    c[6] = a[3] * a[7] - a[4] * a[6]; c[7] = a[1] * a[6] - a[0] * a[7]; c[8] = a[0] * a[4] - a[1] * a[3];
    const double det = a[0] * c[0] + a[1] * c[3] + a[2] * c[6];
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = c[i] / det;
    return det;
}

// e <- the nearest essential matrix: singular values (s, s, 0), s = (s1 + s2) / 2.  The eigenvectors
// v of e^T e by the 3 x 3 cyclic Jacobi of rank2; the one of the smallest eigenvalue (ties: the
// lower index) is dropped, the other two give e <- s (e va) va^T / sa + s (e vb) vb^T / sb.
__device__ __forceinline__ void essential_project(double (&e)[9]) {
    double g[9], v[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            g[3 * i + j] = fma(e[i], e[j], fma(e[3 + i], e[3 + j], e[6 + i] * e[6 + j]));
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
    const bool m2 = g[8] < (m1 ? g[4] : g[0]);
    const bool drop0 = !m2 && !m1;   // the smallest eigenvalue is number 0 / number 2 (otherwise number 1)
    const bool drop2 = m2;
    double va[3], vb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        va[k] = drop0 ? v[3 * k + 1] : v[3 * k];
        vb[k] = drop2 ? v[3 * k + 1] : v[3 * k + 2];
    }
    const double sa = sqrt(drop0 ? g[4] : g[0]), sb = sqrt(drop2 ? g[4] : g[8]);
    const double s = 0.5 * (sa + sb), fa = s / sa, fb = s / sb;
    double o[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double wa = fa * fma(e[3 * i], va[0], fma(e[3 * i + 1], va[1], e[3 * i + 2] * va[2]));
        const double wb = fb * fma(e[3 * i], vb[0], fma(e[3 * i + 1], vb[1], e[3 * i + 2] * vb[2]));
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = fma(wa, va[j], wb * vb[j]);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] = o[i];
}

// The essential matrix as a model of the skeleton: its matrices are fundamental matrices in
// pixels, F = K2^-T E K1^-1, so the records, the score, the refit's acceptance and the mask are
// Fundamental's; only the family of matrices differs.  rr.h states every rule.
struct Essential {
    // a key holds 16 t + root; the ten roots of a sample are scored in ONE walk over a generic pointer
    static constexpr int SAMPLE = 5, FIT_MIN = 8, ROOTS = FP_ROOTS, KEY_SLOTS = 16, ACC = 36, WALK_UNROLL = 1;
    static constexpr bool WALK_SPLIT = false;
    static constexpr bool TRUST_ROOT = true;
    static constexpr int REFIT_OCC = 1;

    struct Ctx {   // the intrinsics of the pair and their inverses
        double k1[9], k2[9], i1[9], i2[9];
        bool ok;   // every entry finite, |det| positive and finite on both sides
    };
    static __device__ __forceinline__ Ctx load(const double* __restrict__ K1, const double* __restrict__ K2, int p) {
        Ctx c;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            c.k1[i] = K1[9 * (long long)p + i];
            c.k2[i] = K2[9 * (long long)p + i];
        }
        const double d1 = inv3(c.k1, c.i1), d2 = inv3(c.k2, c.i2);
        c.ok = all_finite9(c.k1) && all_finite9(c.k2) && isfinite(d1) && isfinite(d2) && fabs(d1) > 0.0 && fabs(d2) > 0.0 &&
               all_finite9(c.i1) && all_finite9(c.i2);
        return c;
    }

    // the five-point solver on K^-1 (x, y, 1)^T, every root as F = K2^-T E K1^-1
    static __device__ __forceinline__ int hypotheses(const Ctx& c, const double (&q)[5][4], double (&F)[FP_ROOTS][9]) {
        double h1[5][3], h2[5][3];
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                h1[j][r] = fma(c.i1[3 * r], q[j][0], fma(c.i1[3 * r + 1], q[j][1], c.i1[3 * r + 2]));
                h2[j][r] = fma(c.i2[3 * r], q[j][2], fma(c.i2[3 * r + 1], q[j][3], c.i2[3 * r + 2]));
            }
        const int n = c.ok ? five_point(h1, h2, F) : 0;
#pragma unroll
        for (int k = 0; k < FP_ROOTS; ++k) {
            double t[9], f[9];
            mat3_ab(F[k], c.i1, t);
            mat3_atb(c.i2, t, f);
            const bool ok = k < n && all_finite9(f);
#pragma unroll
            for (int i = 0; i < 9; ++i) F[k][i] = ok ? f[i] : 0.0;
        }
        return n;
    }
    static __device__ __forceinline__ bool inlier(const double (&f)[9], double x1, double y1, double x2, double y2, double th2) {
        return is_inlier_f(f, x1, y1, x2, y2, th2);
    }
    static __device__ __forceinline__ void accumulate(const FitNorm& n, double x1, double y1, double x2, double y2, double w,
                                                      double (&acc)[36]) {
        Fundamental::accumulate(n, x1, y1, x2, y2, w, acc);
    }
    static __device__ __forceinline__ void write_matrix(const double (&acc)[36], double* a) { Fundamental::write_matrix(acc, a); }

    // E <- K2^T F K1, projected
    static __device__ __forceinline__ void to_essential(const Ctx& c, const double (&f)[9], double (&e)[9]) {
        double t[9];
        mat3_ab(f, c.k1, t);
        mat3_atb(c.k2, t, e);
        essential_project(e);
    }

    // find_fundamental, E' = K2^T F' K1 projected onto the essential matrices, back to pixels
    static __device__ __forceinline__ void finish(const Ctx& c, double (&e9)[9], const FitNorm& n, double (&f)[9]) {
        double f1[9], e[9], t[9];
        Fundamental::finish({}, e9, n, f1);
        to_essential(c, f1, e);
        mat3_ab(e, c.i1, t);
        mat3_atb(c.i2, t, f);
    }

    // E = K2^T F K1 projected, then Fundamental's rule
    static __device__ __forceinline__ void emit(const Ctx& c, bool have, const double (&f)[9], double* __restrict__ out) {
        double e[9];
        to_essential(c, f, e);
        Fundamental::emit({}, have && all_finite9(e), e, out);
    }
};

// rr_essential_5pt: one thread per sample
__global__ void __launch_bounds__(V_TB) k_essential_5pt(const double* __restrict__ x1, const double* __restrict__ x2, int n,
                                                        double* __restrict__ Eout, int* __restrict__ nroots) {
    for (long long s = (long long)blockIdx.x * V_TB + threadIdx.x; s < n; s += (long long)gridDim.x * V_TB) {
        double h1[5][3], h2[5][3];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const double2 a = *reinterpret_cast<const double2*>(x1 + 10 * s + 2 * j);
            const double2 b = *reinterpret_cast<const double2*>(x2 + 10 * s + 2 * j);
            h1[j][0] = a.x; h1[j][1] = a.y; h1[j][2] = 1.0;
            h2[j][0] = b.x; h2[j][1] = b.y; h2[j][2] = 1.0;
        }
        double E[FP_ROOTS][9];
        const int nr = five_point(h1, h2, E);
        int good = 0;
#pragma unroll
        for (int k = 0; k < FP_ROOTS; ++k) {
            const bool ok = k < nr && all_finite9(E[k]);
            good += ok ? 1 : 0;
            Fundamental::emit({}, ok, E[k], Eout + 90 * s + 9 * k);
        }
        nroots[s] = good == nr ? nr : 0;   // a root that is not finite: the sample is refused whole
        if (good != nr) {
#pragma unroll 1
            for (int i = 0; i < 90; ++i) Eout[90 * s + i] = 0.0;
        }
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
    return verify_pairs_impl<Fundamental>("rr_verify_pairs_epipolar", kp1, off1, rows1, kp2, off2, rows2, match, npairs, max_n1,
                                          th, iters, refine, seed, nullptr, nullptr, inliers, F, mask, workspace,
                                          workspace_bytes, stream);
}

size_t rr_verify_essential_workspace_bytes(long long rows1, int npairs, int iters) {
    return measured(layout, rows1, npairs, iters);
}

int rr_verify_pairs_essential(const float* kp1, const long long* off1, long long rows1, const float* kp2,
                              const long long* off2, long long rows2, const long long* match, int npairs, int max_n1,
                              const double* K1, const double* K2, double th, int iters, int refine, unsigned long long seed,
                              int* inliers, double* E, unsigned char* mask, void* workspace, size_t workspace_bytes,
                              void* stream) {
    return verify_pairs_impl<Essential>("rr_verify_pairs_essential", kp1, off1, rows1, kp2, off2, rows2, match, npairs, max_n1,
                                        th, iters, refine, seed, K1, K2, inliers, E, mask, workspace, workspace_bytes, stream);
}

int rr_essential_5pt(const double* x1, const double* x2, int n, double* E, int* nroots, void* stream) {
    const std::string w("rr_essential_5pt");
    if (n < 0) return fail(RR_EINVAL, w + ": negative size");
    if (n > 0 && (!x1 || !x2)) return fail(RR_EINVAL, w + ": null points");
    if (n > 0 && (!E || !nroots)) return fail(RR_EINVAL, w + ": null output");
    if ((((uintptr_t)x1) & 15) || (((uintptr_t)x2) & 15)) return fail(RR_EINVAL, w + ": points must be 16-byte aligned");
    if (n == 0) return RR_OK;
    const int blocks = (n + V_TB - 1) / V_TB;
    hipLaunchKernelGGL(k_essential_5pt, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(V_TB), 0, as_stream(stream), x1,
                       x2, n, E, nroots);
    return check_launch("rr_essential_5pt");
}

int rr_fundamental_dlt(const double* pts1, const double* pts2, const double* weights, const long long* off,
                       long long rows, int npairs, double* F, void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    return fit_batch_impl<Fundamental>("rr_fundamental_dlt", pts1, pts2, weights, off, rows, npairs, F, stream);
}

int rr_epipolar_distance(const double* pts1, const double* pts2, const double* F, const long long* off, long long rows,
                         int npairs, int kind, int squared, double eps, double* out, void* stream) {
    const std::string w("rr_epipolar_distance");
    if (npairs >= 0 && rows >= 0) {   // a negative size is reported first, by check_point_set_args
        if (kind != RR_EPI_SAMPSON && kind != RR_EPI_SYMMETRICAL) return fail(RR_EINVAL, w + ": unknown kind");
        if (squared != 0 && squared != 1) return fail(RR_EINVAL, w + ": squared must be 0 or 1");
        if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(RR_EINVAL, w + ": eps must be >= 0 and finite");
    }
    const int rc = check_point_set_args(w, pts1, pts2, off, rows, npairs, true, out);
    if (rc) return rc;
    if (npairs > 0 && !F) return fail(RR_EINVAL, w + ": null F");
    if (npairs == 0) return RR_OK;
    hipLaunchKernelGGL(k_epi_distance, dim3((unsigned)(npairs < 65535 ? npairs : 65535)), dim3(V_TB), 0, as_stream(stream),
                       pts1, pts2, F, off, rows, npairs, kind, squared, eps, out);
    return check_launch("rr_epipolar_distance");
}

}  // extern "C"
