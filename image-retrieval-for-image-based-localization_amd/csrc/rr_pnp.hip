// librr.so — absolute pose of a query camera against known 3-D points (localization): per pair a RANSAC
// pose from three-point samples (rr_p3p.h), refitted by Gauss-Newton on the reprojection error of
// its inliers.  The step after rr_pose.hip: points3d and front_mask of rr_recover_pose are this entry's
// side 2.  rr.h states every rule.  The primitives (pair ranges, the counter-hash sampler, ransac_key,
// the fixed-order block reductions) are those of rr_ransac.h; the kernels of the 3 x 4 model are here:
//
//   k_pnp_compact   one block per pair: the kept rows (a match inside side 2, valid, finite X) in
//                   ascending order become records (x, y, X, Y, Z, 0) of six doubles (48 B: three
//                   16-byte loads); cnt[p] = M.
//   k_pnp_ransac    block (chunk, pair): the records staged in LDS while M <= V_STAGE (48 KiB), one
//                   hypothesis per thread: draw_n<3>, p3p, P = K [R | t] of each of its (up to four)
//                   solutions, then every lane walks all M records (the same address in every lane)
//                   and scores the four at once; the block's best key -> best[p][chunk].
//   k_pnp_refit     one block per pair: the winner over the chunks, its pose recomputed from
//                   (t, solution), `refine` rounds of RR_PNP_GN_STEPS Gauss-Newton steps (27 sums per
//                   step by block_sum_d, the 6 x 6 Cholesky in every thread), the mask from the rows.
//   k_p3p           rr_p3p: the minimal solver alone, one thread per sample.
//
// Nothing waits for the host, no atomics.  Contraction is switched off in the shared routines and
// every fused multiply-add is written out, so a routine yields the same bits in each kernel.
#include "rr_ransac.h"
#include "rr_p3p.h"

namespace rr {

namespace {

constexpr int PNP_REC = 6;   // doubles per record: x, y, X, Y, Z and one of padding

struct Pnp {   // what ransac_key needs of a model
    static constexpr int KEY_SLOTS = P3P_SOLS;
};

// ---------------------------------------------------------------- the model
struct PnpCam {   // the intrinsics of a pair and their inverse
    double k[9], inv[9];
    bool ok;      // every entry finite, |det| positive and finite, the inverse finite
};

// inverse by the adjugate (the statements of rr_verify_pairs_essential's step a)
__device__ __forceinline__ PnpCam pnp_cam(const double* __restrict__ K, int p) {
    PnpCam c;
#pragma unroll
    for (int i = 0; i < 9; ++i) c.k[i] = K[9 * (long long)p + i];
    const double (&a)[9] = c.k;
    double j[9];
    j[0] = a[4] * a[8] - a[5] * a[7]; j[1] = a[2] * a[7] - a[1] * a[8]; j[2] = a[1] * a[5] - a[2] * a[4];
    j[3] = a[5] * a[6] - a[3] * a[8]; j[4] = a[0] * a[8] - a[2] * a[6]; j[5] = a[2] * a[3] - a[0] * a[5];
    j[6] = a[3] * a[7] - a[4] * a[6]; j[7] = a[1] * a[6] - a[0] * a[7]; j[8] = a[0] * a[4] - a[1] * a[3];
    const double det = a[0] * j[0] + a[1] * j[3] + a[2] * j[6];
#pragma unroll
    for (int i = 0; i < 9; ++i) c.inv[i] = j[i] / det;
    c.ok = all_finite9(c.k) && isfinite(det) && fabs(det) > 0.0 && all_finite9(c.inv);
    return c;
}

// P = K [R | t], row-major 3 x 4
__device__ __forceinline__ void pnp_proj(const double (&k)[9], const double (&R)[9], const double (&t)[3], double (&P)[12]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) P[4 * i + j] = fma(k[3 * i], R[j], fma(k[3 * i + 1], R[3 + j], k[3 * i + 2] * R[6 + j]));
        P[4 * i + 3] = fma(k[3 * i], t[0], fma(k[3 * i + 1], t[1], k[3 * i + 2] * t[2]));
    }
}

// pc = P [X, Y, Z, 1]^T
__device__ __forceinline__ void pnp_apply(const double (&P)[12], double X, double Y, double Z, double (&pc)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) pc[i] = fma(P[4 * i], X, fma(P[4 * i + 1], Y, fma(P[4 * i + 2], Z, P[4 * i + 3])));
}

// step c of rr.h: in front of the camera and within th pixels, without a division
__device__ __forceinline__ bool pnp_inlier(const double (&P)[12], double x, double y, double X, double Y, double Z, double th2) {
#pragma clang fp contract(off)
    double pc[3];
    pnp_apply(P, X, Y, Z, pc);
    const double du = fma(-x, pc[2], pc[0]), dv = fma(-y, pc[2], pc[1]);
    return pc[2] > 0.0 && fma(du, du, dv * dv) <= th2 * (pc[2] * pc[2]);
}

// the (up to four) poses through hypothesis t of pair p; rec: the pair's records
__device__ __forceinline__ int pnp_hypotheses(const PnpCam& cam, const double* __restrict__ rec, unsigned long long seed, int p,
                                              int t, int m, double (&R)[P3P_SOLS][9], double (&tr)[P3P_SOLS][3]) {
    int smp[3];
    draw_n<3>(seed, p, t, m, smp);
    double h[3][3], X[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double* r = rec + PNP_REC * (long long)smp[k];
        const double2 a = *reinterpret_cast<const double2*>(r);
        const double2 b = *reinterpret_cast<const double2*>(r + 2);
        const double2 c = *reinterpret_cast<const double2*>(r + 4);
#pragma unroll
        for (int i = 0; i < 3; ++i) h[k][i] = fma(cam.inv[3 * i], a.x, fma(cam.inv[3 * i + 1], a.y, cam.inv[3 * i + 2]));
        X[k][0] = b.x; X[k][1] = b.y; X[k][2] = c.x;
    }
    return p3p(h, X, R, tr);
}

// a row of a pair -> kept, with its record
__device__ __forceinline__ bool pnp_row(const float* __restrict__ kp1, const double* __restrict__ pts3d,
                                        const unsigned char* __restrict__ valid, const long long* __restrict__ match,
                                        long long b1, long long b2, long long n2, long long i, double& x, double& y, double& X,
                                        double& Y, double& Z) {
    const long long j = match[b1 + i];
    if (!(j >= 0 && j < n2)) return false;
    if (valid && !valid[b2 + j]) return false;
    const double* q = pts3d + 3 * (b2 + j);
    X = q[0]; Y = q[1]; Z = q[2];
    if (!(isfinite(X) && isfinite(Y) && isfinite(Z))) return false;
    const float2 a = *reinterpret_cast<const float2*>(kp1 + 2 * (b1 + i));
    x = (double)a.x; y = (double)a.y;
    return true;
}

// ---------------------------------------------------------------- records
__global__ void __launch_bounds__(V_TB) k_pnp_compact(const float* __restrict__ kp1, const long long* __restrict__ off1,
                                                      long long rows1, const double* __restrict__ pts3d,
                                                      const unsigned char* __restrict__ valid,
                                                      const long long* __restrict__ off2, long long rows2,
                                                      const long long* __restrict__ match, int npairs, int max_n1,
                                                      double* __restrict__ rec, int* __restrict__ cnt) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int p = blockIdx.x; p < npairs; p += gridDim.x) {
        long long b1, n1, b2, n2;
        pair_range(off1, p, rows1, b1, n1);
        pair_range(off2, p, rows2, b2, n2);
        if (n1 > max_n1) n1 = max_n1;
        int total = 0;   // block-uniform
        for (long long i0 = 0; i0 < n1; i0 += V_TB) {
            const long long i = i0 + tid;
            double x = 0.0, y = 0.0, X = 0.0, Y = 0.0, Z = 0.0;
            const bool keep = i < n1 && pnp_row(kp1, pts3d, valid, match, b1, b2, n2, i, x, y, X, Y, Z);
            const unsigned long long bal = __ballot(keep);
            const int before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
            __syncthreads();   // s_w free
            if (lane == 0) s_w[wave] = __popcll(bal);
            __syncthreads();
            int base = total;
            for (int w = 0; w < wave; ++w) base += s_w[w];
            if (keep) {   // base + before < n1: the record lies inside the pair's side-1 rows
                double* r = rec + PNP_REC * (b1 + base + before);
                *reinterpret_cast<double2*>(r) = make_double2(x, y);
                *reinterpret_cast<double2*>(r + 2) = make_double2(X, Y);
                *reinterpret_cast<double2*>(r + 4) = make_double2(Z, 0.0);
            }
            total += (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
        }
        if (tid == 0) cnt[p] = total;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- hypotheses
// every lane walks all m records once (the same address in every lane) and scores the four solutions
__device__ __forceinline__ void pnp_count_all(const double (&P)[P3P_SOLS][12], const double* __restrict__ rec, int m, double th2,
                                              int (&c)[P3P_SOLS]) {
#pragma unroll
    for (int k = 0; k < P3P_SOLS; ++k) c[k] = 0;
#pragma unroll 2
    for (int i = 0; i < m; ++i) {
        const double2 a = *reinterpret_cast<const double2*>(rec + PNP_REC * i);
        const double2 b = *reinterpret_cast<const double2*>(rec + PNP_REC * i + 2);
        const double2 d = *reinterpret_cast<const double2*>(rec + PNP_REC * i + 4);
#pragma unroll
        for (int k = 0; k < P3P_SOLS; ++k) c[k] += pnp_inlier(P[k], a.x, a.y, b.x, b.y, d.x, th2) ? 1 : 0;
    }
}

// block (c, p) scores hypotheses t = 256 c .. 256 c + 255 of pair p, one per thread; the block's best key -> best[p][c]
__global__ void __launch_bounds__(V_TB) k_pnp_ransac(const double* __restrict__ rec, const long long* __restrict__ off1,
                                                     long long rows1, const int* __restrict__ cnt, int npairs, int iters,
                                                     int chunks, double th2, unsigned long long seed,
                                                     const double* __restrict__ K, unsigned long long* __restrict__ best) {
    __shared__ __attribute__((aligned(16))) double s_rec[V_STAGE * PNP_REC];
    __shared__ unsigned long long s_red[4];
    const int tid = threadIdx.x;
    const int t = (int)blockIdx.x * V_TB + tid;
    for (int p = blockIdx.y; p < npairs; p += gridDim.y) {
        const int m = cnt[p];
        unsigned long long key = 0ull;
        if (m >= 3) {   // block-uniform
            long long b1, n1;
            pair_range(off1, p, rows1, b1, n1);
            const double* r = rec + PNP_REC * b1;
            const bool staged = m <= V_STAGE;
            __syncthreads();   // the previous pair's readers of s_rec are done
            if (staged) {
                for (int i = tid; i < 3 * m; i += V_TB)
                    *reinterpret_cast<double2*>(s_rec + 2 * i) = *reinterpret_cast<const double2*>(r + 2 * i);
                __syncthreads();
            }
            if (t < iters) {
                const PnpCam cam = pnp_cam(K, p);
                double R[P3P_SOLS][9], tr[P3P_SOLS][3];
                const int n = cam.ok ? pnp_hypotheses(cam, staged ? s_rec : r, seed, p, t, m, R, tr) : 0;
                if (n > 0) {
                    double P[P3P_SOLS][12];   // the slots past n: all zero, pc2 = 0, never an inlier
#pragma unroll
                    for (int k = 0; k < P3P_SOLS; ++k) pnp_proj(cam.k, R[k], tr[k], P[k]);
                    int c[P3P_SOLS];
                    if (staged) pnp_count_all(P, s_rec, m, th2, c);
                    else pnp_count_all(P, r, m, th2, c);
#pragma unroll
                    for (int k = P3P_SOLS - 1; k >= 0; --k) {
                        const unsigned long long kk = (k < n && c[k] > 0) ? ransac_key<Pnp>(c[k], t, k) : 0ull;
                        key = kk > key ? kk : key;
                    }
                }
            }
        }
        key = block_max_u64(key, s_red);
        if (tid == 0) best[(long long)p * chunks + blockIdx.x] = key;
    }
}

// ---------------------------------------------------------------- refit
// block-parallel inlier count of P over the m records of a pair
__device__ __forceinline__ int pnp_count_block(const double (&P)[12], const double* __restrict__ rec, int m, double th2, int* s4) {
    int c = 0;
    for (int i = threadIdx.x; i < m; i += V_TB) {
        const double* r = rec + PNP_REC * (long long)i;
        const double2 a = *reinterpret_cast<const double2*>(r);
        const double2 b = *reinterpret_cast<const double2*>(r + 2);
        const double2 d = *reinterpret_cast<const double2*>(r + 4);
        c += pnp_inlier(P, a.x, a.y, b.x, b.y, d.x, th2) ? 1 : 0;
    }
    return block_sum_i(c, s4);
}

// H d = -g for the symmetric positive definite 6 x 6 H (upper triangle, row-major: 21 entries) by Cholesky
// without pivoting; false: a pivot that is not > 0 or not finite
__device__ __forceinline__ bool pnp_solve6(const double (&hg)[27], double (&d)[6]) {
#pragma clang fp contract(off)
    double L[6][6];
    {
        int e = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) L[j][i] = hg[e++];   // the lower triangle of H
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = fma(-L[j][k], L[j][k], s);
        ok = ok && s > 0.0 && isfinite(s);
        const double l = sqrt(s);
        L[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = L[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v = fma(-L[i][k], L[j][k], v);
            L[i][j] = v / l;
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {   // L y = -g
        double v = -hg[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = fma(-L[i][k], y[k], v);
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {   // L^T d = y
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v = fma(-L[k][i], d[k], v);
        d[i] = v / L[i][i];
    }
    return ok;
}

// R <- exp([w]x) R, t <- exp([w]x) t + tau (Rodrigues; the series below RR_PNP_SMALL_ANGLE2)
__device__ __forceinline__ void pnp_update(const double (&d)[6], double (&R)[9], double (&t)[3]) {
#pragma clang fp contract(off)
    const double wx = d[0], wy = d[1], wz = d[2];
    const double th2 = fma(wx, wx, fma(wy, wy, wz * wz));
    double A, B;
    if (th2 < RR_PNP_SMALL_ANGLE2) {
        A = 1.0 - th2 / 6.0;
        B = 0.5 - th2 / 24.0;
    } else {
        const double th = sqrt(th2);
        A = sin(th) / th;
        B = (1.0 - cos(th)) / th2;
    }
    // E = I + A [w]x + B [w]x^2, [w]x^2 = w w^T - |w|^2 I
    double E[9];
    E[0] = fma(B, fma(wx, wx, -th2), 1.0); E[1] = fma(B, wx * wy, -(A * wz));       E[2] = fma(B, wx * wz, A * wy);
    E[3] = fma(B, wx * wy, A * wz);        E[4] = fma(B, fma(wy, wy, -th2), 1.0);   E[5] = fma(B, wy * wz, -(A * wx));
    E[6] = fma(B, wx * wz, -(A * wy));     E[7] = fma(B, wy * wz, A * wx);          E[8] = fma(B, fma(wz, wz, -th2), 1.0);
    double Rn[9], tn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = fma(E[3 * i], R[j], fma(E[3 * i + 1], R[3 + j], E[3 * i + 2] * R[6 + j]));
        tn[i] = fma(E[3 * i], t[0], fma(E[3 * i + 1], t[1], E[3 * i + 2] * t[2])) + d[3 + i];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rn[i];
    t[0] = tn[0]; t[1] = tn[1]; t[2] = tn[2];
}

// one record into the 21 + 6 sums of a Gauss-Newton step at (R, t): nothing where its depth is not > 0
__device__ __forceinline__ void pnp_accumulate(const double (&k)[9], const double (&R)[9], const double (&t)[3], double x,
                                               double y, double X, double Y, double Z, double (&acc)[27]) {
#pragma clang fp contract(off)
    double xc[3], pc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) xc[i] = fma(R[3 * i], X, fma(R[3 * i + 1], Y, fma(R[3 * i + 2], Z, t[i])));
#pragma unroll
    for (int i = 0; i < 3; ++i) pc[i] = fma(k[3 * i], xc[0], fma(k[3 * i + 1], xc[1], k[3 * i + 2] * xc[2]));
    if (!(pc[2] > 0.0)) return;
    const double iz = 1.0 / pc[2];
    const double uv[2] = {pc[0] * iz, pc[1] * iz};
    const double res[2] = {uv[0] - x, uv[1] - y};
    double J[2][6];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        double mr[3];   // row r of d(u, v)/dpc . K
#pragma unroll
        for (int c = 0; c < 3; ++c) mr[c] = fma(-uv[r], k[6 + c], k[3 * r + c]) * iz;
        // -M [Xc]x | M
        J[r][0] = fma(mr[2], xc[1], -(mr[1] * xc[2]));
        J[r][1] = fma(mr[0], xc[2], -(mr[2] * xc[0]));
        J[r][2] = fma(mr[1], xc[0], -(mr[0] * xc[1]));
        J[r][3] = mr[0]; J[r][4] = mr[1]; J[r][5] = mr[2];
    }
    int e = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            acc[e] += fma(J[0][i], J[0][j], J[1][i] * J[1][j]);
            ++e;
        }
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += fma(J[0][i], res[0], J[1][i] * res[1]);
}

__device__ __forceinline__ bool pnp_finite(const double (&R)[9], const double (&t)[3]) {
    return all_finite9(R) && isfinite(t[0]) && isfinite(t[1]) && isfinite(t[2]);
}

// one block per pair: the winner over the chunks (integer max of the keys), its pose recomputed from
// (t, solution), then `refine` rounds of {inlier set S, RR_PNP_GN_STEPS Gauss-Newton steps on S, accept
// while the count does not drop}; writes inliers, the pose and the side-1 mask
__global__ void __launch_bounds__(V_TB) k_pnp_refit(const float* __restrict__ kp1, const long long* __restrict__ off1,
                                                    long long rows1, const double* __restrict__ pts3d,
                                                    const unsigned char* __restrict__ valid,
                                                    const long long* __restrict__ off2, long long rows2,
                                                    const long long* __restrict__ match, int npairs, int max_n1,
                                                    const double* __restrict__ rec, const int* __restrict__ cnt,
                                                    const unsigned long long* __restrict__ best, int chunks, double th2,
                                                    int refine, unsigned long long seed, const double* __restrict__ K,
                                                    int* __restrict__ inliers, double* __restrict__ Rout,
                                                    double* __restrict__ tout, unsigned char* __restrict__ mask) {
    __shared__ double s_tmp[5 * 27];
    __shared__ unsigned long long s_red[4];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x;
    for (int p = blockIdx.x; p < npairs; p += gridDim.x) {
        long long b1, n1, b2, n2;
        pair_range(off1, p, rows1, b1, n1);
        pair_range(off2, p, rows2, b2, n2);
        if (n1 > max_n1) n1 = max_n1;
        const int m = cnt[p];
        const double* r = rec + PNP_REC * b1;
        const PnpCam cam = pnp_cam(K, p);
        unsigned long long key = 0ull;
        for (int c = tid; c < chunks; c += V_TB) {
            const unsigned long long k = best[(long long)p * chunks + c];
            key = k > key ? k : key;
        }
        key = block_max_u64(key, s_red);
        double R[9], t[3], P[12];
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = 0.0;
        t[0] = t[1] = t[2] = 0.0;
        int count = 0;
        bool have = m >= 3 && cam.ok && key != 0ull;   // block-uniform
        if (have) {
            const unsigned ts = 0xffffffffu - (unsigned)(key & 0xffffffffull);
            const int th = (int)(ts / P3P_SOLS), sol = (int)(ts % P3P_SOLS);
            {
                double Rs[P3P_SOLS][9], trs[P3P_SOLS][3];
                const int n = pnp_hypotheses(cam, r, seed, p, th, m, Rs, trs);
                have = sol < n;
#pragma unroll
                for (int i = 0; i < 9; ++i) {
                    R[i] = Rs[P3P_SOLS - 1][i];
#pragma unroll
                    for (int k = P3P_SOLS - 2; k >= 0; --k) R[i] = sol == k ? Rs[k][i] : R[i];
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    t[i] = trs[P3P_SOLS - 1][i];
#pragma unroll
                    for (int k = P3P_SOLS - 2; k >= 0; --k) t[i] = sol == k ? trs[k][i] : t[i];
                }
            }
            pnp_proj(cam.k, R, t, P);
            if (have) count = pnp_count_block(P, r, m, th2, s_cnt);
            have = have && count > 0;
            for (int it = 0; have && it < refine && count >= 4; ++it) {
                double R2[9], t2[3];
#pragma unroll
                for (int i = 0; i < 9; ++i) R2[i] = R[i];
                t2[0] = t[0]; t2[1] = t[1]; t2[2] = t[2];
                bool solved = true;
#pragma unroll 1
                for (int step = 0; step < RR_PNP_GN_STEPS && solved; ++step) {
                    double acc[27];
#pragma unroll
                    for (int e = 0; e < 27; ++e) acc[e] = 0.0;
                    for (int i = tid; i < m; i += V_TB) {
                        const double* q = r + PNP_REC * (long long)i;
                        const double2 a = *reinterpret_cast<const double2*>(q);
                        const double2 b = *reinterpret_cast<const double2*>(q + 2);
                        const double2 d = *reinterpret_cast<const double2*>(q + 4);
                        if (pnp_inlier(P, a.x, a.y, b.x, b.y, d.x, th2))   // S: the inliers of the round's pose
                            pnp_accumulate(cam.k, R2, t2, a.x, a.y, b.x, b.y, d.x, acc);
                    }
                    block_sum_d<27>(acc, s_tmp);
                    double d6[6];
                    solved = pnp_solve6(acc, d6);   // block-uniform: every thread holds the totals
                    if (solved) pnp_update(d6, R2, t2);
                }
                if (!solved || !pnp_finite(R2, t2)) break;
                double P2[12];
                pnp_proj(cam.k, R2, t2, P2);
                const int c2 = pnp_count_block(P2, r, m, th2, s_cnt);
                if (c2 < count) break;
                count = c2;
#pragma unroll
                for (int i = 0; i < 9; ++i) R[i] = R2[i];
                t[0] = t2[0]; t[1] = t2[1]; t[2] = t2[2];
#pragma unroll
                for (int i = 0; i < 12; ++i) P[i] = P2[i];
            }
        }
        if (!have) {
            count = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = 0.0;
            t[0] = t[1] = t[2] = 0.0;
        }
        if (tid == 0) {
            inliers[p] = count;
#pragma unroll
            for (int i = 0; i < 9; ++i) Rout[9 * (long long)p + i] = R[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) tout[3 * (long long)p + i] = t[i];
        }
        // the mask straight from the rows: the same values and the same test as the records
        for (long long i = tid; i < n1; i += V_TB) {
            double x, y, X, Y, Z;
            bool in = false;
            if (have && pnp_row(kp1, pts3d, valid, match, b1, b2, n2, i, x, y, X, Y, Z)) in = pnp_inlier(P, x, y, X, Y, Z, th2);
            mask[b1 + i] = in ? 1 : 0;
        }
        __syncthreads();
    }
}

// rr_p3p: one thread per sample
__global__ void __launch_bounds__(V_TB) k_p3p(const double* __restrict__ x, const double* __restrict__ Xw, int n,
                                              double* __restrict__ Rout, double* __restrict__ tout, int* __restrict__ nsol) {
    for (long long s = (long long)blockIdx.x * V_TB + threadIdx.x; s < n; s += (long long)gridDim.x * V_TB) {
        double h[3][3], X[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            h[k][0] = x[6 * s + 2 * k]; h[k][1] = x[6 * s + 2 * k + 1]; h[k][2] = 1.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) X[k][i] = Xw[9 * s + 3 * k + i];
        }
        double R[P3P_SOLS][9], t[P3P_SOLS][3];
        nsol[s] = p3p(h, X, R, t);
#pragma unroll
        for (int k = 0; k < P3P_SOLS; ++k) {
#pragma unroll
            for (int i = 0; i < 9; ++i) Rout[36 * s + 9 * k + i] = R[k][i];
#pragma unroll
            for (int i = 0; i < 3; ++i) tout[12 * s + 3 * k + i] = t[k][i];
        }
    }
}

// ---------------------------------------------------------------- workspace
struct PnpWs {
    double* rec;               // PNP_REC per side-1 row
    int* cnt;                  // per pair
    unsigned long long* best;  // per (pair, chunk)
};

inline PnpWs pnp_layout(Arena& a, long long rows1, int npairs, int iters) {
    const size_t r1 = (size_t)(rows1 > 0 ? rows1 : 0), np = (size_t)(npairs > 0 ? npairs : 0);
    const size_t ch = (size_t)(iters > 0 ? chunks_of(iters) : 1);
    return {a.take<double>(r1 * PNP_REC), a.take<int>(np), a.take<unsigned long long>(np * ch)};
}

}  // namespace

}  // namespace rr

using namespace rr;

extern "C" {

size_t rr_localize_workspace_bytes(long long rows1, int npairs, int iters) { return measured(pnp_layout, rows1, npairs, iters); }

int rr_localize_pairs(const float* kp1, const long long* off1, long long rows1, const double* pts3d, const unsigned char* valid,
                      const long long* off2, long long rows2, const long long* match, int npairs, int max_n1, const double* K,
                      double th, int iters, int refine, unsigned long long seed, int* inliers, double* R, double* t,
                      unsigned char* mask, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string w("rr_localize_pairs");
    if (npairs >= 0 && rows1 >= 0 && rows2 >= 0 && max_n1 >= 0) {   // a negative size is reported first, by check_pair_args
        if (iters < 1) return fail(RR_EINVAL, w + ": iters must be >= 1");
        if (iters > (1 << 24)) return fail(RR_EINVAL, w + ": iters above 2^24");
        if (refine < 0) return fail(RR_EINVAL, w + ": refine must be >= 0");
        if (!(th > 0.0) || !std::isfinite(th)) return fail(RR_EINVAL, w + ": th must be positive and finite");
        if (rows2 > 0 && !pts3d) return fail(RR_EINVAL, w + ": null points3d");
    }
    // side 2 is float64 [rows2][3]: the keypoint checks of side 2 (non-null, 8-byte aligned) hold for it as they are
    int rc = check_pair_args(w, kp1, off1, rows1, reinterpret_cast<const float*>(pts3d), off2, rows2, match, npairs, max_n1);
    if (rc) return rc;
    if (npairs > 0 && (rows1 > 0 && !mask)) return fail(RR_EINVAL, w + ": null output");
    if (npairs > 0 && (!inliers || !R || !t)) return fail(RR_EINVAL, w + ": null output");
    if (npairs > 0 && !K) return fail(RR_EINVAL, w + ": null K");
    if (((uintptr_t)K) & 15) return fail(RR_EINVAL, w + ": K must be 16-byte aligned");
    Arena arena(workspace, workspace_bytes);
    const auto [rec, cnt, best] = pnp_layout(arena, rows1, npairs, iters);
    if (!workspace || !arena.fits()) return fail(RR_ENOSPACE, w + ": workspace too small");
    if (npairs == 0) return RR_OK;
    hipStream_t s = as_stream(stream);
    const int chunks = chunks_of(iters);
    const unsigned gp = (unsigned)(npairs < 65535 ? npairs : 65535);
    hipLaunchKernelGGL(k_pnp_compact, dim3(gp), dim3(V_TB), 0, s, kp1, off1, rows1, pts3d, valid, off2, rows2, match, npairs,
                       max_n1, rec, cnt);
    rc = check_launch((w + ": compact").c_str());
    if (rc) return rc;
    hipLaunchKernelGGL(k_pnp_ransac, dim3((unsigned)chunks, gp), dim3(V_TB), 0, s, rec, off1, rows1, cnt, npairs, iters,
                       chunks, th * th, seed, K, best);
    rc = check_launch((w + ": ransac").c_str());
    if (rc) return rc;
    hipLaunchKernelGGL(k_pnp_refit, dim3(gp), dim3(V_TB), 0, s, kp1, off1, rows1, pts3d, valid, off2, rows2, match, npairs,
                       max_n1, rec, cnt, best, chunks, th * th, refine, seed, K, inliers, R, t, mask);
    return check_launch((w + ": refit").c_str());
}

int rr_p3p(const double* x, const double* X, int n, double* R, double* t, int* nsol, void* stream) {
    const std::string w("rr_p3p");
    if (n < 0) return fail(RR_EINVAL, w + ": negative size");
    if (n > 0 && (!x || !X)) return fail(RR_EINVAL, w + ": null points");
    if (n > 0 && (!R || !t || !nsol)) return fail(RR_EINVAL, w + ": null output");
    if ((((uintptr_t)x) & 7) || (((uintptr_t)X) & 7)) return fail(RR_EINVAL, w + ": points must be 8-byte aligned");
    if (n == 0) return RR_OK;
    const int blocks = (n + V_TB - 1) / V_TB;
    hipLaunchKernelGGL(k_p3p, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(V_TB), 0, as_stream(stream), x, X, n, R, t,
                       nsol);
    return check_launch("rr_p3p");
}

}  // extern "C"
