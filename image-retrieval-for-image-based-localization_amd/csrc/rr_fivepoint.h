// librr.so — the five-point minimal solver of the essential-matrix verifier (rr_epipolar.hip:
// struct Essential, k_essential_5pt).  One thread solves one sample in float64 with statically
// indexed arrays only (everything is unrolled; a runtime index would send the array to scratch):
//   1. an orthonormal basis X, Y, Z, W of the null space of the 5 x 9 system of rows h2 (x) h1 by
//      five Householder reflections (the basis whose entries 5 .. 8 are unit loses every digit on
//      one sample in thirty: its entries reach 1e4);
//   2. E = x X + y Y + z Z + W in det E = 0 and 2 E E^T E - tr(E E^T) E = 0: a 10 x 20 matrix in the
//      monomials of (x, y, z), eliminated in Nister's column order;
//   3. x and y eliminated: a 3 x 3 matrix of polynomials in z whose determinant has degree 10; its
//      real roots by the derivative ladder (the roots of each derivative bracket those of the next);
//   4. x and y back-substituted at every root.
// rr.h states every rule.  The functions are __host__ __device__ so that a host program can run the
// same statements on the CPU.
#pragma once

#include <math.h>

namespace rr {

namespace {

constexpr int FP_ROOTS = 10;    // most real roots of a sample
constexpr int FP_BISECT = 48;   // bisection steps per root
constexpr int FP_NEWTON = 3;    // Newton steps after them, each kept only inside the last bracket

// ---------------------------------------------------------------- polynomials in (x, y, z)
// linear:    [x, y, z, 1]
// quadratic: [x^2, y^2, z^2, xy, xz, yz, x, y, z, 1]
// cubic, the 20 columns of the constraint matrix in Nister's order:
//   [x^3, y^3, x^2 y, x y^2, x^2 z, x^2, y^2 z, y^2, xyz, xy | x z^2, xz, x, y z^2, yz, y, z^3, z^2, z, 1]
// o += s a b, linear x linear
__host__ __device__ __forceinline__ void mul11(const double (&a)[4], const double (&b)[4], double s, double (&o)[10]) {
    constexpr int IDX[4][4] = {{0, 3, 4, 6}, {3, 1, 5, 7}, {4, 5, 2, 8}, {6, 7, 8, 9}};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[IDX[i][j]] = fma(s * a[i], b[j], o[IDX[i][j]]);
}

// o += a b, quadratic x linear
__host__ __device__ __forceinline__ void mul21(const double (&a)[10], const double (&b)[4], double (&o)[20]) {
    constexpr int IDX[10][4] = {{0, 2, 4, 5},     {3, 1, 6, 7},    {10, 13, 16, 17}, {2, 3, 8, 9},     {4, 8, 10, 11},
                                {8, 6, 13, 14},   {5, 9, 11, 12},  {9, 7, 14, 15},   {11, 14, 17, 18}, {12, 15, 18, 19}};
#pragma unroll
    for (int i = 0; i < 10; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[IDX[i][j]] = fma(a[i], b[j], o[IDX[i][j]]);
}

// ---------------------------------------------------------------- polynomials in z, ascending powers
// o += s a b
template <int NA, int NB>
__host__ __device__ __forceinline__ void zmul(const double (&a)[NA], const double (&b)[NB], double s, double (&o)[NA + NB - 1]) {
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) o[i + j] = fma(s * a[i], b[j], o[i + j]);
}

template <int N>
__host__ __device__ __forceinline__ double zeval(const double (&a)[N], double z) {
    double v = a[N - 1];
#pragma unroll
    for (int i = N - 2; i >= 0; --i) v = fma(v, z, a[i]);
    return v;
}

// the polynomial and its derivative at z
template <int N>
__host__ __device__ __forceinline__ void zeval2(const double (&a)[N], double z, double& v, double& dv) {
    v = a[N - 1];
    dv = 0.0;
#pragma unroll
    for (int i = N - 2; i >= 0; --i) {
        dv = fma(dv, z, v);
        v = fma(v, z, a[i]);
    }
}

// ---------------------------------------------------------------- real roots of the degree-10 polynomial
// The real roots in (-B, B) of the polynomial a of degree D, ascending, given the nin ascending real
// roots of its derivative: they cut (-B, B) into nin + 1 intervals, each holds at most one root, and
// it holds one where the sign (v < 0) of a differs at its ends.  -> their number
template <int D>
__host__ __device__ __forceinline__ int level_roots(const double (&a)[D + 1], double B, const double (&cin)[FP_ROOTS], int nin,
                                                    double (&out)[FP_ROOTS]) {
#pragma unroll
    for (int j = 0; j < FP_ROOTS; ++j) out[j] = 0.0;
    int n = 0;
    double lo = -B, flo = zeval<D + 1>(a, lo);
#pragma unroll
    for (int i = 0; i < D; ++i) {   // at most D - 1 roots of the derivative: D intervals
        if (i <= nin) {
            const double hi = i < nin ? cin[i] : B;
            const double fhi = zeval<D + 1>(a, hi);
            const bool neg = flo < 0.0;
            if (neg != (fhi < 0.0)) {
                double u = lo, w = hi;
#pragma unroll 1
                for (int k = 0; k < FP_BISECT; ++k) {
                    const double mid = 0.5 * (u + w);
                    const bool left = (zeval<D + 1>(a, mid) < 0.0) == neg;
                    u = left ? mid : u;
                    w = left ? w : mid;
                }
                double r = 0.5 * (u + w);
#pragma unroll 1
                for (int k = 0; k < FP_NEWTON; ++k) {
                    double v, dv;
                    zeval2<D + 1>(a, r, v, dv);
                    const double rn = r - v / dv;
                    r = (rn >= u && rn <= w) ? rn : r;
                }
#pragma unroll
                for (int j = 0; j < FP_ROOTS; ++j) out[j] = j == n ? r : out[j];
                ++n;
            }
            lo = hi;
            flo = fhi;
        }
    }
    return n;
}

// n (n - 1) .. (n - k + 1)
__host__ __device__ constexpr double falling(int n, int k) {
    double f = 1.0;
    for (int i = 0; i < k; ++i) f *= (double)(n - i);
    return f;
}

// the real roots of derivative number 10 - D of c (degree D) from those of derivative number 11 - D
template <int D>
struct Ladder {
    static __host__ __device__ __forceinline__ int run(const double (&c)[11], double B, double (&out)[FP_ROOTS]) {
        double prev[FP_ROOTS];
        const int np = Ladder<D - 1>::run(c, B, prev);
        double a[D + 1];
#pragma unroll
        for (int i = 0; i <= D; ++i) a[i] = c[i + 10 - D] * falling(i + 10 - D, 10 - D);
        return level_roots<D>(a, B, prev, np, out);
    }
};
template <>
struct Ladder<0> {
    static __host__ __device__ __forceinline__ int run(const double (&)[11], double, double (&out)[FP_ROOTS]) {
#pragma unroll
        for (int j = 0; j < FP_ROOTS; ++j) out[j] = 0.0;
        return 0;
    }
};

// real roots of c0 + c1 z + .. + c10 z^10 in ascending order -> their number; rr.h states the rule
__host__ __device__ __forceinline__ int poly10_roots(const double (&c)[11], double (&z)[FP_ROOTS]) {
    double big = 0.0;
#pragma unroll
    for (int i = 0; i < 10; ++i) big = fmax(big, fabs(c[i] / c[10]));   // fmax drops a NaN: the sum below keeps it
    double chk = 0.0;
#pragma unroll
    for (int i = 0; i < 11; ++i) chk += c[i];
    const double B = 1.0 + big;
    if (!(isfinite(B) && isfinite(chk) && fabs(c[10]) > 0.0)) {
#pragma unroll
        for (int j = 0; j < FP_ROOTS; ++j) z[j] = 0.0;
        return 0;
    }
    return Ladder<10>::run(c, B, z);
}

// ---------------------------------------------------------------- the solver
// The essential matrices through five correspondences h2[j]^T E h1[j] = 0 (homogeneous normalised
// points): E[k] = x X + y Y + z Z + W, k < the number returned, in ascending order of z; the slots
// past it are all zero.
__host__ __device__ __forceinline__ int five_point(const double (&h1)[5][3], const double (&h2)[5][3], double (&E)[FP_ROOTS][9]) {
    // 1. the null space: e[i] = the linear polynomial [x, y, z, 1] of entry i of E
    double e[9][4];
    {
        // A[j] = h2[j] (x) h1[j] is column j of the 9 x 5 matrix that five Householder reflections
        // H_k = I - beta_k v_k v_k^T make upper triangular; v_k is zero above entry k
        double A[5][9], beta[5];
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) A[j][3 * a + b] = h2[j][a] * h1[j][b];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            double ss = 0.0;
#pragma unroll
            for (int i = k; i < 9; ++i) ss = fma(A[k][i], A[k][i], ss);
            const double nrm = sqrt(ss);
            A[k][k] += A[k][k] < 0.0 ? -nrm : nrm;     // v = x + sign(x_0) |x| e_0, kept in place of the column
            beta[k] = 1.0 / fma(nrm, fabs(A[k][k]) - nrm, ss);   // 2 / v^T v = 1 / (|x|^2 + |x| |x_0|)
#pragma unroll
            for (int j = k + 1; j < 5; ++j) {
                double d = 0.0;
#pragma unroll
                for (int i = k; i < 9; ++i) d = fma(A[k][i], A[j][i], d);
                d *= beta[k];
#pragma unroll
                for (int i = k; i < 9; ++i) A[j][i] = fma(-d, A[k][i], A[j][i]);
            }
        }
        // X, Y, Z, W = H_0 H_1 H_2 H_3 H_4 e_j, j = 5 .. 8
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double n[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) n[i] = i == 5 + j ? 1.0 : 0.0;
#pragma unroll
            for (int k = 4; k >= 0; --k) {
                double d = 0.0;
#pragma unroll
                for (int i = k; i < 9; ++i) d = fma(A[k][i], n[i], d);
                d *= beta[k];
#pragma unroll
                for (int i = k; i < 9; ++i) n[i] = fma(-d, A[k][i], n[i]);
            }
#pragma unroll
            for (int i = 0; i < 9; ++i) e[i][j] = n[i];
        }
    }
    // 2. the ten cubic constraints
    double M[10][20];
#pragma unroll
    for (int r = 0; r < 10; ++r)
#pragma unroll
        for (int k = 0; k < 20; ++k) M[r][k] = 0.0;
    {   // det E along the first row
        double m0[10], m1[10], m2[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) m0[k] = m1[k] = m2[k] = 0.0;
        mul11(e[4], e[8], 1.0, m0);  mul11(e[5], e[7], -1.0, m0);
        mul11(e[3], e[8], -1.0, m1); mul11(e[5], e[6], 1.0, m1);    // minus the minor
        mul11(e[3], e[7], 1.0, m2);  mul11(e[4], e[6], -1.0, m2);
        mul21(m0, e[0], M[0]);
        mul21(m1, e[1], M[0]);
        mul21(m2, e[2], M[0]);
    }
    {   // (2 E E^T - tr(E E^T) I) E
        constexpr int TRI[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
        double G[6][10];
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
            for (int k = 0; k < 10; ++k) G[t][k] = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 3; ++k) mul11(e[3 * r + k], e[3 * c + k], 1.0, G[TRI[3 * r + c]]);
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            const double tr = G[0][k] + G[3][k] + G[5][k];
            G[0][k] = 2.0 * G[0][k] - tr;
            G[3][k] = 2.0 * G[3][k] - tr;
            G[5][k] = 2.0 * G[5][k] - tr;
            G[1][k] *= 2.0;
            G[2][k] *= 2.0;
            G[4][k] *= 2.0;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 3; ++k) mul21(G[TRI[3 * r + k]], e[3 * k + c], M[1 + 3 * r + c]);
    }
    // Gauss-Jordan on columns 0 .. 9 with partial pivoting; rows 0 .. 3 are not needed afterwards
    // and are left alone once their pivot is done
#pragma unroll
    for (int c = 0; c < 10; ++c) {
#pragma unroll
        for (int i = c + 1; i < 10; ++i) {
            const bool sw = fabs(M[i][c]) > fabs(M[c][c]);
#pragma unroll
            for (int k = c; k < 20; ++k) {
                const double u = M[c][k], v = M[i][k];
                M[c][k] = sw ? v : u;
                M[i][k] = sw ? u : v;
            }
        }
        const double inv = 1.0 / M[c][c];
#pragma unroll
        for (int k = c + 1; k < 20; ++k) M[c][k] *= inv;
#pragma unroll
        for (int i = 4; i < 10; ++i) {
            if (i == c) continue;
            const double g = M[i][c];
#pragma unroll
            for (int k = c + 1; k < 20; ++k) M[i][k] = fma(-g, M[c][k], M[i][k]);
        }
#pragma unroll
        for (int i = c + 1; i < 4; ++i) {
            const double g = M[i][c];
#pragma unroll
            for (int k = c + 1; k < 20; ++k) M[i][k] = fma(-g, M[c][k], M[i][k]);
        }
    }
    // 3. rows (x^2 z, x^2), (y^2 z, y^2), (xyz, xy): the first minus z times the second is
    //    x bx(z) + y by(z) + bc(z) with bx, by of degree 3 and bc of degree 4
    double bx[3][4], by[3][4], bc[3][5];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double (&p)[20] = M[4 + 2 * r];
        const double (&q)[20] = M[5 + 2 * r];
        bx[r][0] = p[12]; bx[r][1] = p[11] - q[12]; bx[r][2] = p[10] - q[11]; bx[r][3] = -q[10];
        by[r][0] = p[15]; by[r][1] = p[14] - q[15]; by[r][2] = p[13] - q[14]; by[r][3] = -q[13];
        bc[r][0] = p[19]; bc[r][1] = p[18] - q[19]; bc[r][2] = p[17] - q[18]; bc[r][3] = p[16] - q[17]; bc[r][4] = -q[16];
    }
    double c[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) c[i] = 0.0;
    {
        double t7[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) t7[i] = 0.0;
        zmul<4, 5>(by[1], bc[2], 1.0, t7);
        zmul<4, 5>(by[2], bc[1], -1.0, t7);
        zmul<4, 8>(bx[0], t7, 1.0, c);
#pragma unroll
        for (int i = 0; i < 8; ++i) t7[i] = 0.0;
        zmul<4, 5>(bx[1], bc[2], 1.0, t7);
        zmul<4, 5>(bx[2], bc[1], -1.0, t7);
        zmul<4, 8>(by[0], t7, -1.0, c);
        double t6[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) t6[i] = 0.0;
        zmul<4, 4>(bx[1], by[2], 1.0, t6);
        zmul<4, 4>(bx[2], by[1], -1.0, t6);
        zmul<5, 7>(bc[0], t6, 1.0, c);
    }
    double z[FP_ROOTS];
    const int nr = poly10_roots(c, z);
    // 4. (x, y, 1) spans the null space of the 3 x 3 at the root: the cross product of the two rows
    //    whose third component is largest in magnitude (the earlier pair among equals)
#pragma unroll
    for (int k = 0; k < FP_ROOTS; ++k) {
        double rx[3], ry[3], rc[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            rx[r] = zeval<4>(bx[r], z[k]);
            ry[r] = zeval<4>(by[r], z[k]);
            rc[r] = zeval<5>(bc[r], z[k]);
        }
        double n0 = ry[0] * rc[1] - rc[0] * ry[1], n1 = rc[0] * rx[1] - rx[0] * rc[1], n2 = rx[0] * ry[1] - ry[0] * rx[1];
        {
            const double a0 = ry[0] * rc[2] - rc[0] * ry[2], a1 = rc[0] * rx[2] - rx[0] * rc[2], a2 = rx[0] * ry[2] - ry[0] * rx[2];
            const bool t = fabs(a2) > fabs(n2);
            n0 = t ? a0 : n0; n1 = t ? a1 : n1; n2 = t ? a2 : n2;
        }
        {
            const double a0 = ry[1] * rc[2] - rc[1] * ry[2], a1 = rc[1] * rx[2] - rx[1] * rc[2], a2 = rx[1] * ry[2] - ry[1] * rx[2];
            const bool t = fabs(a2) > fabs(n2);
            n0 = t ? a0 : n0; n1 = t ? a1 : n1; n2 = t ? a2 : n2;
        }
        const double x = n0 / n2, y = n1 / n2;
#pragma unroll
        for (int i = 0; i < 9; ++i)
            E[k][i] = k < nr ? fma(x, e[i][0], fma(y, e[i][1], fma(z[k], e[i][2], e[i][3]))) : 0.0;
    }
    return nr;
}

}  // namespace

}  // namespace rr
