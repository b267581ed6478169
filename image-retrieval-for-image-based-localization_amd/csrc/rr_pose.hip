// librr.so — relative pose of verified pairs: the essential matrix of a fundamental matrix, its four
// candidate motions, the triangulation of the matches under each and the choice by the depths.  The
// step after rr_epipolar.hip: it brings cirtorch/geometry/epipolar/essential.py:8-153
// (essential_from_fundamental, decompose_essential_matrix, motion_from_essential,
// motion_from_essential_choose_solution), triangulation.py:7-41 (triangulate_points) and
// projection.py:60-78, :111-119 (projection_from_KRt, depth) to the device.  rr.h states every rule.
//
// The reference is a chain of torch.svd calls: one 3 x 3 per pair and one 4 x 4 per correspondence
// and candidate.  Here both decompositions are Jacobi iterations in registers:
//
//   ess_candidates   E0 -> U, V by the 3 x 3 cyclic Jacobi (rot3 of rr_ransac.h) on E0^T E0, the sign
//                    fix in closed form (u2 = u0 x u1, v2 = v0 x v1), then Ra, Rb, t and E.
//   tri_point        one correspondence under (P1, P2): the 4 x 4 system of triangulation.py:27-31,
//                    one-sided (Hestenes) Jacobi on its columns -- the system is in pixel units and
//                    badly scaled, A^T A would square its condition number --, the right singular
//                    vector of the smallest singular value, de-homogenised.  Every index is static
//                    after unrolling: the 4 x 4 and its rotations stay in VGPRs, no scratch.
//
//   k_recover_pose          one block per pair.  Thread 0 decomposes E0 = K2^T F K1 and leaves the
//                           candidates and their projection matrices in LDS; the threads stride over
//                           the pair's rows, a thread triangulates a used row under the four
//                           candidates and counts the fronts; block_sum_i; a second pass over the rows
//                           writes the winner's points with the same arithmetic, hence the same bits.
//   k_triangulate           rr_triangulate_points: tri_point on caller-supplied points.
//   k_essential_decompose   rr_essential_decompose: ess_candidates, one thread per matrix.
//
// No workspace, no atomics, nothing waits for the host.  Contraction is switched off in the shared
// routines and every fused multiply-add is written out, so a routine yields the same bits in each
// kernel it is inlined into.
#include "rr_ransac.h"

namespace rr {

namespace {

// ---------------------------------------------------------------- essential matrix -> candidates
__device__ __forceinline__ double sel3(int i, double a, double b, double c) { return i == 0 ? a : (i == 1 ? b : c); }

__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
#pragma clang fp contract(off)
    c[0] = fma(a[1], b[2], -(a[2] * b[1]));
    c[1] = fma(a[2], b[0], -(a[0] * b[2]));
    c[2] = fma(a[0], b[1], -(a[1] * b[0]));
}

__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) {
    return fma(a[0], b[0], fma(a[1], b[1], a[2] * b[2]));
}

// steps b and c of rr.h on e = E0 (row-major): Ra, Rb, t = u2 and En = U diag(1, 1, 0) V^T.
// false (outputs all zero): e not finite or all zero, or its second singular value not > 0.
__device__ __forceinline__ bool ess_candidates(const double (&e)[9], double (&Ra)[9], double (&Rb)[9], double (&t)[3],
                                               double (&En)[9]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 9; ++i) Ra[i] = Rb[i] = En[i] = 0.0;
    t[0] = t[1] = t[2] = 0.0;
    if (!all_finite9(e)) return false;
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
    // the largest and the second largest eigenvalue, the lower index first among equals
    const double d0 = g[0], d1 = g[4], d2 = g[8];
    int i0 = d1 > d0 ? 1 : 0;
    if (d2 > (i0 == 1 ? d1 : d0)) i0 = 2;
    const int ra = i0 == 0 ? 1 : 0, rb = i0 == 2 ? 1 : 2;
    const int i1 = sel3(rb, d0, d1, d2) > sel3(ra, d0, d1, d2) ? rb : ra;
    double v0[3], v1[3], v2[3], a0[3], a1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v0[k] = sel3(i0, v[3 * k], v[3 * k + 1], v[3 * k + 2]);
        v1[k] = sel3(i1, v[3 * k], v[3 * k + 1], v[3 * k + 2]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a0[k] = fma(e[3 * k], v0[0], fma(e[3 * k + 1], v0[1], e[3 * k + 2] * v0[2]));
        a1[k] = fma(e[3 * k], v1[0], fma(e[3 * k + 1], v1[1], e[3 * k + 2] * v1[2]));
    }
    const double s0 = sqrt(dot3(a0, a0)), s1 = sqrt(dot3(a1, a1));
    if (!isfinite(s0) || !(s1 > 0.0)) return false;
    double u0[3], u1[3], u2[3], b[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) u0[k] = a0[k] / s0;
    const double h = dot3(u0, a1);
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = fma(-h, u0[k], a1[k]);
    const double sb = sqrt(dot3(b, b));
    if (!(sb > 0.0)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) u1[k] = b[k] / sb;
    cross3(u0, u1, u2);
    cross3(v0, v1, v2);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double p = u1[i] * v0[j], q = u0[i] * v1[j], r = u2[i] * v2[j];
            Ra[3 * i + j] = (p - q) + r;
            Rb[3 * i + j] = (q - p) + r;
            En[3 * i + j] = fma(u0[i], v0[j], u1[i] * v1[j]);
        }
    t[0] = u2[0]; t[1] = u2[1]; t[2] = u2[2];
    return true;
}

// ---------------------------------------------------------------- triangulation of one correspondence
// one Hestenes rotation of columns P and Q of the 4 x 4 a (row-major), the same on v
template <int P, int Q>
__device__ __forceinline__ bool hrot4(double (&a)[16], double (&v)[16]) {
#pragma clang fp contract(off)
    double app = 0.0, aqq = 0.0, apq = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        app = fma(a[4 * k + P], a[4 * k + P], app);
        aqq = fma(a[4 * k + Q], a[4 * k + Q], aqq);
        apq = fma(a[4 * k + P], a[4 * k + Q], apq);
    }
    if (!(fabs(apq) > V_JTOL * sqrt(app * aqq))) return false;
    const double theta = (aqq - app) / (2.0 * apq);
    const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
    const double c = 1.0 / sqrt(fma(tt, tt, 1.0)), s = tt * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double x = a[4 * k + P], y = a[4 * k + Q];
        a[4 * k + P] = fma(c, x, -(s * y));
        a[4 * k + Q] = fma(s, x, c * y);
        const double vx = v[4 * k + P], vy = v[4 * k + Q];
        v[4 * k + P] = fma(c, vx, -(s * vy));
        v[4 * k + Q] = fma(s, vx, c * vy);
    }
    return true;
}

// step d of rr.h: P1, P2 [3][4] row-major (any address space: they are read once), -> X
__device__ __forceinline__ void tri_point(const double* P1, const double* P2, double x1, double y1, double x2, double y2,
                                          double (&X)[3]) {
#pragma clang fp contract(off)
    double a[16], v[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double p12 = P1[8 + i], p22 = P2[8 + i];
        a[i] = fma(x1, p12, -P1[i]);
        a[4 + i] = fma(y1, p12, -P1[4 + i]);
        a[8 + i] = fma(x2, p22, -P2[i]);
        a[12 + i] = fma(y2, p22, -P2[4 + i]);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[4 * k + i] = i == k ? 1.0 : 0.0;
    }
#pragma unroll 1
    for (int sweep = 0; sweep < RR_POSE_SWEEPS; ++sweep) {
        const bool r0 = hrot4<0, 1>(a, v);
        const bool r1 = hrot4<0, 2>(a, v);
        const bool r2 = hrot4<0, 3>(a, v);
        const bool r3 = hrot4<1, 2>(a, v);
        const bool r4 = hrot4<1, 3>(a, v);
        const bool r5 = hrot4<2, 3>(a, v);
        if (!(r0 || r1 || r2 || r3 || r4 || r5)) break;
    }
    double n[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) n[i] = fma(a[i], a[i], fma(a[4 + i], a[4 + i], fma(a[8 + i], a[8 + i], a[12 + i] * a[12 + i])));
    int m = 0;
    double best = n[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (n[i] < best) { best = n[i]; m = i; }
    double h[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = m == 0 ? v[4 * k] : (m == 1 ? v[4 * k + 1] : (m == 2 ? v[4 * k + 2] : v[4 * k + 3]));
    const double s = fabs(h[3]) > V_EPS ? 1.0 / h[3] : 1.0;
    X[0] = s * h[0]; X[1] = s * h[1]; X[2] = s * h[2];
}

// both depths of X positive: X_z and (R X)_z + t_z (projection.py:116-117)
__device__ __forceinline__ bool in_front(const double (&X)[3], double r20, double r21, double r22, double tz) {
#pragma clang fp contract(off)
    const double d2 = fma(r20, X[0], fma(r21, X[1], r22 * X[2])) + tz;
    return X[2] > 0.0 && d2 > 0.0;
}

// ---------------------------------------------------------------- kernels
struct PoseLds {
    double P1[12];
    double P2[4][12];
    double R[2][9];
    double t[3];
    double E[9];
    int ok;
};

__global__ void __launch_bounds__(V_TB) k_recover_pose(const float* __restrict__ kp1, const long long* __restrict__ off1,
                                                       long long rows1, const float* __restrict__ kp2,
                                                       const long long* __restrict__ off2, long long rows2,
                                                       const long long* __restrict__ match,
                                                       const unsigned char* __restrict__ mask, const double* __restrict__ Fm,
                                                       const double* __restrict__ K1m, const double* __restrict__ K2m,
                                                       int npairs, int max_n1, double* __restrict__ Rout,
                                                       double* __restrict__ tout, double* __restrict__ Eout,
                                                       int* __restrict__ front, double* __restrict__ points3d,
                                                       unsigned char* __restrict__ front_mask) {
    __shared__ PoseLds L;
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x;
    for (int p = blockIdx.x; p < npairs; p += gridDim.x) {
        long long b1, n1, b2, n2;
        pair_range(off1, p, rows1, b1, n1);
        pair_range(off2, p, rows2, b2, n2);
        if (n1 > max_n1) n1 = max_n1;
        if (tid == 0) {
            double f[9], k1[9], k2[9], m[9], e[9];
            bool nz = false;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                f[i] = Fm[9 * (long long)p + i];
                k1[i] = K1m[9 * (long long)p + i];
                k2[i] = K2m[9 * (long long)p + i];
                nz = nz || f[i] != 0.0;
            }
            // E0 = K2^T (F K1)
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) m[3 * i + j] = fma(f[3 * i], k1[j], fma(f[3 * i + 1], k1[3 + j], f[3 * i + 2] * k1[6 + j]));
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) e[3 * i + j] = fma(k2[i], m[j], fma(k2[3 + i], m[3 + j], k2[6 + i] * m[6 + j]));
            double Ra[9], Rb[9], t[3], En[9];
            const bool ok = nz && all_finite9(f) && all_finite9(k1) && all_finite9(k2) && ess_candidates(e, Ra, Rb, t, En);
            L.ok = ok ? 1 : 0;
#pragma unroll
            for (int i = 0; i < 9; ++i) { L.R[0][i] = Ra[i]; L.R[1][i] = Rb[i]; L.E[i] = En[i]; }
#pragma unroll
            for (int i = 0; i < 3; ++i) L.t[i] = t[i];
            // P1 = K1 [I | 0], P2 = K2 [R | +-t]
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    L.P1[4 * i + j] = k1[3 * i + j];
                    L.P2[0][4 * i + j] = L.P2[1][4 * i + j] = fma(k2[3 * i], Ra[j], fma(k2[3 * i + 1], Ra[3 + j], k2[3 * i + 2] * Ra[6 + j]));
                    L.P2[2][4 * i + j] = L.P2[3][4 * i + j] = fma(k2[3 * i], Rb[j], fma(k2[3 * i + 1], Rb[3 + j], k2[3 * i + 2] * Rb[6 + j]));
                }
                const double kt = fma(k2[3 * i], t[0], fma(k2[3 * i + 1], t[1], k2[3 * i + 2] * t[2]));
                L.P1[4 * i + 3] = 0.0;
                L.P2[0][4 * i + 3] = L.P2[2][4 * i + 3] = kt;
                L.P2[1][4 * i + 3] = L.P2[3][4 * i + 3] = -kt;
            }
        }
        __syncthreads();
        const bool ok = L.ok != 0;   // block-uniform
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0, used = 0;
        if (ok) {
            for (long long i = tid; i < n1; i += V_TB) {
                const long long j = match[b1 + i];
                if (!(j >= 0 && j < n2) || (mask && !mask[b1 + i])) continue;
                const float2 a = *reinterpret_cast<const float2*>(kp1 + 2 * (b1 + i));
                const float2 b = *reinterpret_cast<const float2*>(kp2 + 2 * (b2 + j));
                used += 1;
#pragma unroll 1
                for (int c = 0; c < 4; ++c) {
                    double X[3];
                    tri_point(L.P1, L.P2[c], (double)a.x, (double)a.y, (double)b.x, (double)b.y, X);
                    const double* R = L.R[c >> 1];
                    const int in = in_front(X, R[6], R[7], R[8], (c & 1) ? -L.t[2] : L.t[2]) ? 1 : 0;
                    c0 += c == 0 ? in : 0;
                    c1 += c == 1 ? in : 0;
                    c2 += c == 2 ? in : 0;
                    c3 += c == 3 ? in : 0;
                }
            }
        }
        used = block_sum_i(used, s_cnt);
        c0 = block_sum_i(c0, s_cnt);
        c1 = block_sum_i(c1, s_cnt);
        c2 = block_sum_i(c2, s_cnt);
        c3 = block_sum_i(c3, s_cnt);
        // the most fronts, the lowest index among equals
        int win = 0, best = c0;
        if (c1 > best) { best = c1; win = 1; }
        if (c2 > best) { best = c2; win = 2; }
        if (c3 > best) { best = c3; win = 3; }
        const bool have = ok && used > 0;
        const double* R = L.R[win >> 1];
        const double sg = (win & 1) ? -1.0 : 1.0;
        if (tid < 9) {
            Rout[9 * (long long)p + tid] = have ? R[tid] : 0.0;
            Eout[9 * (long long)p + tid] = have ? L.E[tid] : 0.0;
        }
        if (tid < 3) tout[3 * (long long)p + tid] = have ? sg * L.t[tid] : 0.0;
        if (tid == 0) front[p] = have ? best : 0;
        for (long long i = tid; i < n1; i += V_TB) {
            double X[3] = {0.0, 0.0, 0.0};
            bool in = false;
            if (have) {
                const long long j = match[b1 + i];
                if (j >= 0 && j < n2 && !(mask && !mask[b1 + i])) {
                    const float2 a = *reinterpret_cast<const float2*>(kp1 + 2 * (b1 + i));
                    const float2 b = *reinterpret_cast<const float2*>(kp2 + 2 * (b2 + j));
                    tri_point(L.P1, L.P2[win], (double)a.x, (double)a.y, (double)b.x, (double)b.y, X);
                    in = in_front(X, R[6], R[7], R[8], sg * L.t[2]);
                }
            }
            double* o = points3d + 3 * (b1 + i);
            o[0] = X[0]; o[1] = X[1]; o[2] = X[2];
            front_mask[b1 + i] = in ? 1 : 0;
        }
        __syncthreads();   // L and s_cnt are free for the next pair
    }
}

__global__ void __launch_bounds__(V_TB) k_triangulate(const double* __restrict__ p1, const double* __restrict__ p2,
                                                      const double* __restrict__ P1m, const double* __restrict__ P2m,
                                                      const long long* __restrict__ off, long long rows, int npairs,
                                                      double* __restrict__ Xout) {
    __shared__ double s_P[24];
    for (int p = blockIdx.x; p < npairs; p += gridDim.x) {
        long long b, n;
        pair_range(off, p, rows, b, n);
        __syncthreads();   // the previous set's readers of s_P are done
        if (threadIdx.x < 24)
            s_P[threadIdx.x] = threadIdx.x < 12 ? P1m[12 * (long long)p + threadIdx.x] : P2m[12 * (long long)p + threadIdx.x - 12];
        __syncthreads();
        for (long long i = threadIdx.x; i < n; i += V_TB) {
            const double2 a = *reinterpret_cast<const double2*>(p1 + 2 * (b + i));
            const double2 c = *reinterpret_cast<const double2*>(p2 + 2 * (b + i));
            double X[3];
            tri_point(s_P, s_P + 12, a.x, a.y, c.x, c.y, X);
            double* o = Xout + 3 * (b + i);
            o[0] = X[0]; o[1] = X[1]; o[2] = X[2];
        }
    }
}

__global__ void __launch_bounds__(V_TB) k_essential_decompose(const double* __restrict__ Em, int n, double* __restrict__ R1,
                                                              double* __restrict__ R2, double* __restrict__ tout) {
    for (long long i = (long long)blockIdx.x * V_TB + threadIdx.x; i < n; i += (long long)gridDim.x * V_TB) {
        double e[9], Ra[9], Rb[9], t[3], En[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] = Em[9 * i + k];
        ess_candidates(e, Ra, Rb, t, En);
#pragma unroll
        for (int k = 0; k < 9; ++k) { R1[9 * i + k] = Ra[k]; R2[9 * i + k] = Rb[k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) tout[3 * i + k] = t[k];
    }
}

}  // namespace

}  // namespace rr

using namespace rr;

extern "C" {

int rr_recover_pose(const float* kp1, const long long* off1, long long rows1, const float* kp2, const long long* off2,
                    long long rows2, const long long* match, const unsigned char* mask, const double* F, const double* K1,
                    const double* K2, int npairs, int max_n1, double* R, double* t, double* E, int* front,
                    double* points3d, unsigned char* front_mask, void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    const std::string w("rr_recover_pose");
    const int rc = check_pair_args(w, kp1, off1, rows1, kp2, off2, rows2, match, npairs, max_n1);
    if (rc) return rc;
    if (npairs > 0 && (!F || !K1 || !K2)) return fail(RR_EINVAL, w + ": null F, K1 or K2");
    if (npairs > 0 && (!R || !t || !E || !front)) return fail(RR_EINVAL, w + ": null output");
    if (npairs > 0 && rows1 > 0 && (!points3d || !front_mask)) return fail(RR_EINVAL, w + ": null output");
    if (npairs == 0) return RR_OK;
    hipLaunchKernelGGL(k_recover_pose, dim3((unsigned)(npairs < 65535 ? npairs : 65535)), dim3(V_TB), 0, as_stream(stream),
                       kp1, off1, rows1, kp2, off2, rows2, match, mask, F, K1, K2, npairs, max_n1, R, t, E, front, points3d,
                       front_mask);
    return check_launch("rr_recover_pose");
}

int rr_triangulate_points(const double* pts1, const double* pts2, const double* P1, const double* P2, const long long* off,
                          long long rows, int npairs, double* X, void* stream) {
    const std::string w("rr_triangulate_points");
    const int rc = check_point_set_args(w, pts1, pts2, off, rows, npairs, true, X);
    if (rc) return rc;
    if (npairs > 0 && (!P1 || !P2)) return fail(RR_EINVAL, w + ": null projection matrices");
    if (npairs == 0) return RR_OK;
    hipLaunchKernelGGL(k_triangulate, dim3((unsigned)(npairs < 65535 ? npairs : 65535)), dim3(V_TB), 0, as_stream(stream),
                       pts1, pts2, P1, P2, off, rows, npairs, X);
    return check_launch("rr_triangulate_points");
}

int rr_essential_decompose(const double* E, int n, double* R1, double* R2, double* t, void* stream) {
    const std::string w("rr_essential_decompose");
    if (n < 0) return fail(RR_EINVAL, w + ": negative size");
    if (n > 0 && (!E || !R1 || !R2 || !t)) return fail(RR_EINVAL, w + ": null matrices or output");
    if (n == 0) return RR_OK;
    const unsigned blocks = (unsigned)((n + V_TB - 1) / V_TB);
    hipLaunchKernelGGL(k_essential_decompose, dim3(blocks < 65535u ? blocks : 65535u), dim3(V_TB), 0, as_stream(stream), E, n,
                       R1, R2, t);
    return check_launch("rr_essential_decompose");
}

}  // extern "C"
