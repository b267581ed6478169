// librr.so — spatial verification: batched RANSAC homography and (weighted) DLT.
// Replaces, batched and on the device, the per-pair cv2.findHomography(..., cv2.RANSAC) loop of
// cirtorch/utils/evaluation/HPatchesEval.py:45-69 and the solvers of
// cirtorch/geometry/homography.py:11-74 (find_homography_dlt, find_homography_dlt_iterated) with
// normalize_points of cirtorch/geometry/epipolar/fundamental.py:6-33.
//
// Everything is float64 on float32 pixel keypoints, every sum has one fixed order, no atomic
// touches a floating-point value and nothing waits for the host.  This file holds the model
// (struct Homography: the 4-point fit, the residual test, the DLT's sums, matrix and
// de-normalisation); the kernels are the skeleton of rr_ransac.h instantiated for it:
//
//   k_verify_compact  one block per pair: the kept matches (0 <= match[i] < n2) of the pair, in
//                     ascending side-1 index, become records (x1, y1, x2, y2) of four doubles at
//                     the pair's side-1 offset in the workspace (ballot + prefix over 256 rows
//                     at a time); cnt[p] = M_p.
//   k_ransac<H>       block (c, p) scores hypotheses t = 256 c .. 256 c + 255 of pair p, one per
//                     thread: the four sample indices by the counter hash of rr.h (a pure function
//                     of seed, p, t, j), the 4-point homography in registers from the projective
//                     basis construction (H = B adj(A), A and B from 3x3 adjugates, static
//                     indexing, no pivoting), then a walk over all M_p records.  The records of a
//                     pair with M_p <= V_STAGE = 1024 (32 KiB) are staged in LDS once per block and
//                     every lane reads the same record at the same time (a broadcast read); a
//                     longer pair reads them from the workspace (wave-uniform global reads).  The
//                     block's best (count desc, t asc) goes to best[p][c] as one 64-bit key.
//   k_refit<H>        one block per pair: the winner over the chunks (integer max of the keys),
//                     its H recomputed from t, then `refine` rounds of {inlier set S of H, the
//                     reference's unweighted DLT on S, accept while the count does not drop};
//                     writes inliers, H and the side-1 mask.
//   k_fit_batch<H>    rr_homography_dlt: the same DLT routine on caller-supplied float64 points
//                     with optional weights.
//
// The DLT routine (fit_block<Homography>) is block-wide: three passes over the selected points (sums for the
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
// Everything but the model is shared with the epipolar verifier (rr_epipolar.hip) and lives in rr_ransac.h.
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

// ---------------------------------------------------------------- the model (rr_ransac.h states what a model provides)
struct Homography {
    static constexpr int SAMPLE = 4, FIT_MIN = 4, ROOTS = 1, KEY_SLOTS = 1, ACC = 24, WALK_UNROLL = 4;
    static constexpr bool WALK_SPLIT = true;
    static constexpr bool TRUST_ROOT = false;  // the refit checks the winner's 4-point fit again
    // 3 blocks per CU (no scratch): while one wave of a block runs its Jacobi rotations the other blocks keep the CU busy
    static constexpr int REFIT_OCC = 3;

    struct Ctx {};   // a pair is its records
    static __device__ __forceinline__ Ctx load(const double*, const double*, int) { return {}; }

    static __device__ __forceinline__ int hypotheses(const Ctx&, const double (&q)[4][4], double (&M)[1][9]) { return h_from4(q, M[0]) ? 1 : 0; }
    static __device__ __forceinline__ bool inlier(const double (&h)[9], double x1, double y1, double x2, double y2, double th2) {
        return is_inlier(h, x1, y1, x2, y2, th2);
    }

    // find_homography_dlt (homography.py:11-58): A^T W A of the rows ax / ay of homography.py:32-33
    // from S0, Sx, Sy, Sr (upper triangles of 3 x 3)
    static __device__ __forceinline__ void accumulate(const FitNorm& n, double x1, double y1, double x2, double y2, double w,
                                                      double (&acc)[24]) {
        const double u2 = fma(n.sc2, x2, n.tx2), v2 = fma(n.sc2, y2, n.ty2);
        const double pt[3] = {fma(n.sc1, x1, n.tx1), fma(n.sc1, y1, n.ty1), 1.0};
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

    static __device__ __forceinline__ void write_matrix(const double (&acc)[24], double* a) {
        if (threadIdx.x == 0) {    // one thread writes the symmetric matrix
            int e = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = r; c < 3; ++c, ++e) {
#pragma unroll
                    for (int f = 0; f < 2; ++f) {   // (r, c) and its mirror
                        const int i = f ? c : r, j = f ? r : c;
                        a[9 * i + j] = acc[e];
                        a[9 * (3 + i) + 3 + j] = acc[e];
                        a[9 * i + 3 + j] = 0.0;
                        a[9 * (3 + i) + j] = 0.0;
                        a[9 * i + 6 + j] = -acc[6 + e];
                        a[9 * (6 + j) + i] = -acc[6 + e];
                        a[9 * (3 + i) + 6 + j] = -acc[12 + e];
                        a[9 * (6 + j) + 3 + i] = -acc[12 + e];
                        a[9 * (6 + i) + 6 + j] = acc[18 + e];
                    }
                }
        }
    }

    // H = T2^-1 (h T1) / (H[2][2] + eps)
    static __device__ __forceinline__ void finish(const Ctx&, const double (&e9)[9], const FitNorm& n, double (&h)[9]) {
        double g[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            g[3 * r] = e9[3 * r] * n.sc1;
            g[3 * r + 1] = e9[3 * r + 1] * n.sc1;
            g[3 * r + 2] = e9[3 * r] * n.tx1 + e9[3 * r + 1] * n.ty1 + e9[3 * r + 2];
        }
        const double i2 = 1.0 / n.sc2;
        double o[9];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[c] = g[c] * i2 + n.mx2 * g[6 + c];
            o[3 + c] = g[3 + c] * i2 + n.my2 * g[6 + c];
            o[6 + c] = g[6 + c];
        }
        const double den = o[8] + V_EPS;
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = o[i] / den;
    }

    static __device__ __forceinline__ void emit(const Ctx&, bool, const double (&h)[9], double* out) {   // h is all zero without a winner
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] = h[i];
    }
};

}  // namespace

}  // namespace rr

using namespace rr;

extern "C" {

size_t rr_verify_workspace_bytes(long long rows1, int npairs, int iters) { return measured(layout, rows1, npairs, iters); }

int rr_verify_pairs(const float* kp1, const long long* off1, long long rows1, const float* kp2, const long long* off2,
                    long long rows2, const long long* match, int npairs, int max_n1, double th, int iters, int refine,
                    unsigned long long seed, int* inliers, double* H, unsigned char* mask, void* workspace,
                    size_t workspace_bytes, void* stream) {
    return verify_pairs_impl<Homography>("rr_verify_pairs", kp1, off1, rows1, kp2, off2, rows2, match, npairs, max_n1, th, iters,
                                         refine, seed, nullptr, nullptr, inliers, H, mask, workspace, workspace_bytes, stream);
}

int rr_homography_dlt(const double* pts1, const double* pts2, const double* weights, const long long* off,
                      long long rows, int npairs, double* H, void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    return fit_batch_impl<Homography>("rr_homography_dlt", pts1, pts2, weights, off, rows, npairs, H, stream);
}

}  // extern "C"
