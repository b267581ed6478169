// librr.so — the three-point minimal solver of absolute pose (rr_pnp.hip: k_pnp_ransac, k_pnp_refit,
// k_p3p).  One thread solves one sample in float64 with statically indexed arrays only (everything
// is unrolled; a runtime index would send the array to scratch):
//   1. unit bearings j_k of the three image points, side lengths of the 3-D triangle, the cosines
//      between the bearings;
//   2. Grunert's elimination: a quartic in v = s3 / s1 (s_k the depth of point k along j_k); its real
//      roots by the derivative ladder of rr_fivepoint.h at degree 4 (the roots of each derivative
//      bracket those of the next, 48 bisections, 3 guarded Newton steps);
//   3. per root u = s2 / s1 and s1 in closed form, the camera-frame points Y_k = s_k j_k;
//   4. the rigid motion between the triangles X and Y from the orthonormal frame each one spans.
// rr.h states every rule.  Contraction is switched off and every fused multiply-add is written out, so
// the routine yields the same bits in each kernel it is inlined into; the functions are
// __host__ __device__ so that a host program can run the same statements on the CPU
// (tests/asan/p3p_host.cpp).
#pragma once

#include <math.h>

namespace rr {

namespace {

constexpr int P3P_SOLS = 4;     // most solutions of a sample
constexpr int P3P_BISECT = 48;  // bisection steps per root
constexpr int P3P_NEWTON = 3;   // Newton steps after them, each kept only inside the last bracket

// ---------------------------------------------------------------- small vectors
__host__ __device__ __forceinline__ double p3_dot(const double (&a)[3], const double (&b)[3]) {
    return fma(a[0], b[0], fma(a[1], b[1], a[2] * b[2]));
}

__host__ __device__ __forceinline__ void p3_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
#pragma clang fp contract(off)
    c[0] = fma(a[1], b[2], -(a[2] * b[1]));
    c[1] = fma(a[2], b[0], -(a[0] * b[2]));
    c[2] = fma(a[0], b[1], -(a[1] * b[0]));
}

// the frame of a triangle: e1 along p1 - p0, e3 normal to the plane, e2 = e3 x e1 -> |e1 x (p2 - p0)|
__host__ __device__ __forceinline__ double p3_frame(const double (&p0)[3], const double (&p1)[3], const double (&p2)[3],
                                                    double (&e1)[3], double (&e2)[3], double (&e3)[3]) {
#pragma clang fp contract(off)
    double d1[3], d2[3], n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d1[k] = p1[k] - p0[k];
        d2[k] = p2[k] - p0[k];
    }
    const double l1 = sqrt(p3_dot(d1, d1));
#pragma unroll
    for (int k = 0; k < 3; ++k) e1[k] = d1[k] / l1;
    p3_cross(e1, d2, n);
    const double ln = sqrt(p3_dot(n, n));
#pragma unroll
    for (int k = 0; k < 3; ++k) e3[k] = n[k] / ln;
    p3_cross(e3, e1, e2);
    return ln;
}

// ---------------------------------------------------------------- polynomials, ascending powers
template <int N>
__host__ __device__ __forceinline__ double p3_eval(const double (&a)[N], double z) {
    double v = a[N - 1];
#pragma unroll
    for (int i = N - 2; i >= 0; --i) v = fma(v, z, a[i]);
    return v;
}

// the polynomial and its derivative at z
template <int N>
__host__ __device__ __forceinline__ void p3_eval2(const double (&a)[N], double z, double& v, double& dv) {
    v = a[N - 1];
    dv = 0.0;
#pragma unroll
    for (int i = N - 2; i >= 0; --i) {
        dv = fma(dv, z, v);
        v = fma(v, z, a[i]);
    }
}

// The real roots in (-B, B) of the polynomial a of degree D, ascending, given the nin ascending real
// roots of its derivative: they cut (-B, B) into nin + 1 intervals, each holds at most one root, and
// it holds one where the sign (v < 0) of a differs at its ends.  -> their number
template <int D>
__host__ __device__ __forceinline__ int p3_level(const double (&a)[D + 1], double B, const double (&cin)[P3P_SOLS], int nin,
                                                 double (&out)[P3P_SOLS]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < P3P_SOLS; ++j) out[j] = 0.0;
    int n = 0;
    double lo = -B, flo = p3_eval<D + 1>(a, lo);
#pragma unroll
    for (int i = 0; i < D; ++i) {   // at most D - 1 roots of the derivative: D intervals
        if (i <= nin) {
            const double hi = i < nin ? cin[i] : B;
            const double fhi = p3_eval<D + 1>(a, hi);
            const bool neg = flo < 0.0;
            if (neg != (fhi < 0.0)) {
                double u = lo, w = hi;
#pragma unroll 1
                for (int k = 0; k < P3P_BISECT; ++k) {
                    const double mid = 0.5 * (u + w);
                    const bool left = (p3_eval<D + 1>(a, mid) < 0.0) == neg;
                    u = left ? mid : u;
                    w = left ? w : mid;
                }
                double r = 0.5 * (u + w);
#pragma unroll 1
                for (int k = 0; k < P3P_NEWTON; ++k) {
                    double v, dv;
                    p3_eval2<D + 1>(a, r, v, dv);
                    const double rn = r - v / dv;
                    r = (rn >= u && rn <= w) ? rn : r;
                }
#pragma unroll
                for (int j = 0; j < P3P_SOLS; ++j) out[j] = j == n ? r : out[j];
                ++n;
            }
            lo = hi;
            flo = fhi;
        }
    }
    return n;
}

// real roots of c0 + c1 v + .. + c4 v^4 in ascending order -> their number; rr.h states the rule
__host__ __device__ __forceinline__ int p3_quartic_roots(const double (&c)[5], double (&z)[P3P_SOLS]) {
#pragma clang fp contract(off)
    double big = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) big = fmax(big, fabs(c[i] / c[4]));   // fmax drops a NaN: the sum below keeps it
    double chk = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i) chk += c[i];
    const double B = 1.0 + big;
#pragma unroll
    for (int j = 0; j < P3P_SOLS; ++j) z[j] = 0.0;
    if (!(isfinite(B) && isfinite(chk) && fabs(c[4]) > 0.0)) return 0;
    // derivative number 4 - D of c has the coefficients c[i + 4 - D] (i + 4 - D)! / i!
    const double d1[2] = {6.0 * c[3], 24.0 * c[4]};
    const double d2[3] = {2.0 * c[2], 6.0 * c[3], 12.0 * c[4]};
    const double d3[4] = {c[1], 2.0 * c[2], 3.0 * c[3], 4.0 * c[4]};
    double r0[P3P_SOLS] = {0.0, 0.0, 0.0, 0.0}, r1[P3P_SOLS], r2[P3P_SOLS], r3[P3P_SOLS];
    const int n1 = p3_level<1>(d1, B, r0, 0, r1);
    const int n2 = p3_level<2>(d2, B, r1, n1, r2);
    const int n3 = p3_level<3>(d3, B, r2, n2, r3);
    return p3_level<4>(c, B, r3, n3, z);
}

// ---------------------------------------------------------------- the solver
// The camera poses (R, t), Y = R X + t, under which the three 3-D points X[k] lie on the rays of the
// homogeneous image points h[k] (any scale, in front of the camera): R[s] row-major and t[s], s < the
// number returned, in ascending order of the quartic's root; the slots past it are all zero.
__host__ __device__ __forceinline__ int p3p(const double (&h)[3][3], const double (&X)[3][3], double (&R)[P3P_SOLS][9],
                                            double (&t)[P3P_SOLS][3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int s = 0; s < P3P_SOLS; ++s) {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[s][i] = 0.0;
        t[s][0] = t[s][1] = t[s][2] = 0.0;
    }
    double j[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double l = sqrt(p3_dot(h[k], h[k]));
#pragma unroll
        for (int i = 0; i < 3; ++i) j[k][i] = h[k][i] / l;
    }
    double d23[3], d13[3], d12[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d23[i] = X[1][i] - X[2][i];
        d13[i] = X[0][i] - X[2][i];
        d12[i] = X[0][i] - X[1][i];
    }
    const double a2 = p3_dot(d23, d23), b2 = p3_dot(d13, d13), c2 = p3_dot(d12, d12);
    double e1[3], e2[3], e3[3];
    const double area = p3_frame(X[0], X[1], X[2], e1, e2, e3);
    if (!(b2 > 0.0) || !(area > 0.0)) return 0;
    const double ca = p3_dot(j[1], j[2]), cb = p3_dot(j[0], j[2]), cg = p3_dot(j[0], j[1]);
    const double q = (a2 - c2) / b2, p = (a2 + c2) / b2, ab = a2 / b2, cbb = c2 / b2;
    double c[5];
    c[4] = (q - 1.0) * (q - 1.0) - 4.0 * cbb * ca * ca;
    c[3] = 4.0 * (q * (1.0 - q) * cb - (1.0 - p) * ca * cg + 2.0 * cbb * ca * ca * cb);
    c[2] = 2.0 * (q * q - 1.0 + 2.0 * q * q * cb * cb + 2.0 * ((b2 - c2) / b2) * ca * ca - 4.0 * p * ca * cb * cg +
                  2.0 * ((b2 - a2) / b2) * cg * cg);
    c[1] = 4.0 * (-q * (1.0 + q) * cb + 2.0 * ab * cg * cg * cb - (1.0 - p) * ca * cg);
    c[0] = (1.0 + q) * (1.0 + q) - 4.0 * ab * cg * cg;
    double v[P3P_SOLS];
    const int nr = p3_quartic_roots(c, v);   // A4 == 0 or a coefficient that is not finite: none
    const double b = sqrt(b2);
    int n = 0;
    bool good = true;
#pragma unroll
    for (int k = 0; k < P3P_SOLS; ++k) {
        const double vk = v[k];
        const double u = (fma((q - 1.0) * vk, vk, -(2.0 * q * cb * vk)) + 1.0 + q) / (2.0 * (cg - vk * ca));
        const double s1 = b / sqrt(fma(vk, vk, 1.0) - 2.0 * vk * cb);
        const double s2 = u * s1, s3 = vk * s1;
        const bool keep = k < nr && vk > 0.0 && u > 0.0 && s1 > 0.0 && isfinite(s1) && isfinite(s2) && isfinite(s3);
        double Y[3][3], f1[3], f2[3], f3[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            Y[0][i] = s1 * j[0][i];
            Y[1][i] = s2 * j[1][i];
            Y[2][i] = s3 * j[2][i];
        }
        p3_frame(Y[0], Y[1], Y[2], f1, f2, f3);
        double Rk[9], tk[3];
        bool fin = true;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                Rk[3 * r + cc] = fma(f1[r], e1[cc], fma(f2[r], e2[cc], f3[r] * e3[cc]));
                fin = fin && isfinite(Rk[3 * r + cc]);
            }
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            tk[r] = Y[0][r] - fma(Rk[3 * r], X[0][0], fma(Rk[3 * r + 1], X[0][1], Rk[3 * r + 2] * X[0][2]));
            fin = fin && isfinite(tk[r]);
        }
        good = good && (!keep || fin);
#pragma unroll
        for (int s = 0; s < P3P_SOLS; ++s) {
            const bool put = keep && s == n;
#pragma unroll
            for (int i = 0; i < 9; ++i) R[s][i] = put ? Rk[i] : R[s][i];
#pragma unroll
            for (int i = 0; i < 3; ++i) t[s][i] = put ? tk[i] : t[s][i];
        }
        n += keep ? 1 : 0;
    }
    if (!good) {   // a kept root whose pose is not finite: the sample is refused whole
#pragma unroll
        for (int s = 0; s < P3P_SOLS; ++s) {
#pragma unroll
            for (int i = 0; i < 9; ++i) R[s][i] = 0.0;
            t[s][0] = t[s][1] = t[s][2] = 0.0;
        }
        return 0;
    }
    return n;
}

}  // namespace

}  // namespace rr
