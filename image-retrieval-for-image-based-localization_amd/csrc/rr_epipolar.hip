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
//
// One residual routine (epi_terms) serves the RANSAC scorer, the refit, the mask and
// rr_epipolar_distance.  The 8-point routine (fit_block<Fundamental>) is block-wide like the DLT: three
// passes (means; mean distances; the 36 sums X^T W X = sum w (p2 p2^T) (x) (p1 p1^T) is made of),
// the 9 x 9 cyclic Jacobi of rr_ransac.h, then the rank-2 projection F - (F v3) v3^T with v3 from a
// 3 x 3 cyclic Jacobi on F^T F in registers (every thread the same).
//
// A result depends on nothing but the pair's own data, seed, p and t (block size 256 everywhere).
#include "rr_ransac.h"

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

    static __device__ __forceinline__ int hypotheses(const double (&q)[7][4], double (&F)[3][9]) { return f_from7(q, F); }
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
    static __device__ __forceinline__ void finish(double (&e9)[9], const FitNorm& n, double (&f)[9]) {
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
    static __device__ __forceinline__ void emit(bool have, const double (&f)[9], double* __restrict__ out) {
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
                                          th, iters, refine, seed, inliers, F, mask, workspace, workspace_bytes, stream);
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
