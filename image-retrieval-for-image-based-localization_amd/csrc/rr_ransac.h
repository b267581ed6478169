// librr.so — what the geometric verifiers (rr_verify.hip: homography, rr_epipolar.hip:
// fundamental and essential matrix) and the pose entry after them (rr_pose.hip) share: the pair ranges, the
// counter-hash sampler of rr.h, the compaction of kept matches into records, the block reductions
// with one fixed order, the round-robin cyclic Jacobi on a symmetric 9 x 9 matrix in LDS, the
// cyclic Jacobi on a symmetric 3 x 3 in registers, the workspace layout, and on top of them the
// RANSAC skeleton: the kernels k_ransac<M>, k_refit<M>, k_fit_batch<M>, the block-wide fit and the
// host entries, written once for a model M that each verifier defines.  The files compile this
// with the same floating-point settings, so a shared routine yields the same bits in each.
#pragma once
#include "rr_internal.h"
#include "rr_workspace.h"

#include <math.h>
#include <type_traits>

namespace rr {

namespace {

constexpr int V_TB = 256;        // threads of every block (fixed: it fixes the summation order)
constexpr int V_STAGE = 1024;    // records of the LDS stage of the RANSAC kernels (x 32 B = 32 KiB)
constexpr int V_SWEEPS = 16;     // cyclic Jacobi: the most sweeps (it stops after 6 - 8)
constexpr double V_JTOL = 0x1p-52; // a rotation is skipped where |a_pq| <= V_JTOL sqrt(a_pp a_qq)
constexpr double V_EPS = 1e-8;   // the reference's eps (normalize_points, find_homography_dlt, find_fundamental)
constexpr double V_RT2 = (double)1.41421356237309504880f;   // the reference's sqrt(2): torch.sqrt(torch.tensor(2.)), float32

// begin / length of pair p on one side, clamped to the buffer (as rr_match.hip)
__device__ __forceinline__ void pair_range(const long long* off, int p, long long rows, long long& b, long long& n) {
    long long lo = off[p], hi = off[p + 1];
    lo = lo < 0 ? 0 : (lo > rows ? rows : lo);
    hi = hi < lo ? lo : (hi > rows ? rows : hi);
    b = lo;
    n = hi - lo;
}

__device__ __forceinline__ bool all_finite9(const double (&h)[9]) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && isfinite(h[i]);
    return ok;
}

// ---------------------------------------------------------------- sampling (rr.h states the rule)
__host__ __device__ __forceinline__ uint32_t vmix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// K distinct record indices of hypothesis t of pair p, m >= K records: draw j depends on the
// draws before it only, so the first four of any K are the four of K = 4
template <int K>
__device__ __forceinline__ void draw_n(unsigned long long seed, int p, int t, int m, int (&smp)[K]) {
    uint32_t s = vmix((uint32_t)seed + 0x9e3779b9u);
    s = vmix(s ^ (uint32_t)(seed >> 32));
    s = vmix(s + (uint32_t)p);
    s = vmix(s + (uint32_t)t);
    int slot[K], moved[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int k = (int)(vmix(s + (uint32_t)j) % (uint32_t)(m - j));
        const int last = m - 1 - j;
        int vk = k, vl = last;   // a[k], a[last] of the virtual array a[i] = i after the earlier moves
#pragma unroll
        for (int i = 0; i < j; ++i) {
            if (slot[i] == k) vk = moved[i];
            if (slot[i] == last) vl = moved[i];
        }
        smp[j] = vk;
        slot[j] = k;
        moved[j] = vl;
    }
}

// the K records (x1, y1, x2, y2) of hypothesis t of pair p
template <int K>
__device__ __forceinline__ void sample(const double* __restrict__ rec, unsigned long long seed, int p, int t, int m,
                                       double (&q)[K][4]) {
    int smp[K];
    draw_n<K>(seed, p, t, m, smp);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double2 a = *reinterpret_cast<const double2*>(rec + 4 * (long long)smp[j]);
        const double2 b = *reinterpret_cast<const double2*>(rec + 4 * (long long)smp[j] + 2);
        q[j][0] = a.x; q[j][1] = a.y; q[j][2] = b.x; q[j][3] = b.y;
    }
}

// ---------------------------------------------------------------- block reductions (256 threads)
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* s4) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    __syncthreads();   // s4 free
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long r = s4[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) r = s4[i] > r ? s4[i] : r;
    return r;
}

__device__ __forceinline__ int block_sum_i(int v, int* s4) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// K sums at once: wave butterfly (a + b == b + a: every lane holds the same bits), then the four
// waves as (w0 + w1) + (w2 + w3) by thread e < K; every thread returns the totals.  tmp: 5 K doubles of LDS.
template <int K>
__device__ __forceinline__ void block_sum_d(double (&v)[K], double* tmp) {
#pragma unroll
    for (int e = 0; e < K; ++e)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[e] += __shfl_xor(v[e], o, 64);
    __syncthreads();   // tmp free
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int e = 0; e < K; ++e) tmp[(threadIdx.x >> 6) * K + e] = v[e];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int e = threadIdx.x;
        tmp[4 * K + e] = (tmp[e] + tmp[K + e]) + (tmp[2 * K + e] + tmp[3 * K + e]);
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < K; ++e) v[e] = tmp[4 * K + e];
}

// ---------------------------------------------------------------- point source of the batched fits
// n points, get(i, x1, y1, x2, y2, w) -> selected
struct SrcPoints {       // rr_homography_dlt: every point, weight from the table or 1
    const double* p1;
    const double* p2;
    const double* wt;
    int n;
    __device__ __forceinline__ bool get(int i, double& x1, double& y1, double& x2, double& y2, double& w) const {
        const double2 a = *reinterpret_cast<const double2*>(p1 + 2 * (long long)i);
        const double2 b = *reinterpret_cast<const double2*>(p2 + 2 * (long long)i);
        x1 = a.x; y1 = a.y; x2 = b.x; y2 = b.y; w = wt ? wt[i] : 1.0;
        return true;
    }
};

// ---------------------------------------------------------------- cyclic Jacobi, 9 x 9 in LDS
// One round of cyclic Jacobi in the round-robin ordering on the symmetric 9 x 9 matrix in LDS:
// round r = 0..8 leaves index (5 r) mod 9 out and rotates the four disjoint pairs
// {idle + d, idle - d} (mod 9), d = 1..4, at once (their rotations commute), so a sweep is 9 steps
// instead of 36.  36 lanes of ONE wave: lane = 9 g + k, group g owns pair g, k the element of the
// two columns, then of the two rows, that its rotation touches.  Every angle is taken from the
// matrix as the round finds it.  The LDS traffic of one wave is executed in issue order; the
// fences keep the compiler from moving an access across a step.  -> this lane's pair was rotated
__device__ __forceinline__ bool jacobi_round(double* A, double* V, int r, int lane) {
    const int g = lane / 9, k = lane - 9 * g;
    const int idle = (5 * r) % 9, a = (idle + g + 1) % 9, b = (idle + 8 - g) % 9;
    const int p = a < b ? a : b, q = a < b ? b : a;
    const double apq = A[9 * p + q], app = A[9 * p + p], aqq = A[9 * q + q];
    const bool rot = fabs(apq) > V_JTOL * sqrt(fabs(app * aqq));   // the same in the nine lanes of a group
    double c = 1.0, s = 0.0;
    if (rot) {
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
        c = 1.0 / sqrt(fma(t, t, 1.0));
        s = t * c;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    {   // A <- A J, V <- V J: columns p and q
        const double x = A[9 * k + p], y = A[9 * k + q];
        const double vx = V[9 * k + p], vy = V[9 * k + q];
        if (rot) {
            A[9 * k + p] = c * x - s * y;
            A[9 * k + q] = s * x + c * y;
            V[9 * k + p] = c * vx - s * vy;
            V[9 * k + q] = s * vx + c * vy;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    {   // A <- J^T A: rows p and q (after every group's columns)
        const double x = A[9 * p + k], y = A[9 * q + k];
        if (rot) {
            A[9 * p + k] = c * x - s * y;
            A[9 * q + k] = s * x + c * y;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    if (rot && k == 0) A[9 * p + q] = A[9 * q + p] = 0.0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    return rot;
}

// The eigenvector of the smallest eigenvalue (ties: the lower index) of the symmetric 9 x 9
// matrix A in LDS; V is scratch of 81 doubles.  Block-wide: every thread calls it after A is
// written (no barrier needed in between) and returns the same e9; sweeps end with the first one
// that rotates nothing.
__device__ __forceinline__ void jacobi_smallest9(double* A, double* V, double (&e9)[9]) {
    const int tid = threadIdx.x;
    if (tid < 81) V[tid] = (tid / 9 == tid % 9) ? 1.0 : 0.0;
    __syncthreads();
    if (tid < 64) {    // wave 0: 36 lanes rotate, all 64 vote
#pragma unroll 1
        for (int sweep = 0; sweep < V_SWEEPS; ++sweep) {
            bool any = false;
#pragma unroll 1
            for (int r = 0; r < 9; ++r) {
                const bool rot = tid < 36 ? jacobi_round(A, V, r, tid) : false;
                any = (__ballot(rot) != 0ull) || any;
            }
            if (!any) break;   // wave-uniform
        }
    }
    __syncthreads();
    int m = 0;
    double best = A[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        const double d = A[10 * i];
        if (d < best) { best = d; m = i; }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) e9[i] = V[9 * i + m];
}

// ---------------------------------------------------------------- cyclic Jacobi, 3 x 3 in registers
// one Jacobi rotation of the symmetric 3 x 3 matrix g in registers (the criterion and the angle of
// jacobi_round), eigenvectors accumulated in the columns of v
template <int P, int Q>
__device__ __forceinline__ bool rot3(double (&g)[9], double (&v)[9]) {
    constexpr int R = 3 - P - Q;
    const double apq = g[3 * P + Q], app = g[4 * P], aqq = g[4 * Q];
    if (!(fabs(apq) > V_JTOL * sqrt(fabs(app * aqq)))) return false;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
    const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = t * c;
    const double arp = g[3 * R + P], arq = g[3 * R + Q];
    g[4 * P] = app - t * apq;
    g[4 * Q] = aqq + t * apq;
    g[3 * P + Q] = g[3 * Q + P] = 0.0;
    g[3 * R + P] = g[3 * P + R] = c * arp - s * arq;
    g[3 * R + Q] = g[3 * Q + R] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x = v[3 * k + P], y = v[3 * k + Q];
        v[3 * k + P] = c * x - s * y;
        v[3 * k + Q] = s * x + c * y;
    }
    return true;
}

// ---------------------------------------------------------------- records
// one block per pair: the kept matches (0 <= match[i] < n2) in ascending side-1 index become
// records (x1, y1, x2, y2) of four doubles at the pair's side-1 offset; cnt[p] = M_p
[[maybe_unused]]   // rr_pose.hip includes this header and reads the rows itself
__global__ void __launch_bounds__(V_TB) k_verify_compact(const float* __restrict__ kp1, const long long* __restrict__ off1,
                                                         long long rows1, const float* __restrict__ kp2,
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
            long long j = -1;
            if (i < n1) j = match[b1 + i];
            const bool keep = j >= 0 && j < n2;
            const unsigned long long bal = __ballot(keep);
            const int before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
            __syncthreads();   // s_w free
            if (lane == 0) s_w[wave] = __popcll(bal);
            __syncthreads();
            int base = total;
            for (int w = 0; w < wave; ++w) base += s_w[w];
            if (keep) {
                const float2 a = *reinterpret_cast<const float2*>(kp1 + 2 * (b1 + i));
                const float2 b = *reinterpret_cast<const float2*>(kp2 + 2 * (b2 + j));
                double* r = rec + 4 * (b1 + base + before);
                *reinterpret_cast<double2*>(r) = make_double2((double)a.x, (double)a.y);
                *reinterpret_cast<double2*>(r + 2) = make_double2((double)b.x, (double)b.y);
            }
            total += (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
        }
        if (tid == 0) cnt[p] = total;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- workspace (both verifiers)
inline int chunks_of(int iters) { return (iters + V_TB - 1) / V_TB; }

struct VerifyWs {
    double* rec;               // 4 per side-1 row
    int* cnt;                  // per pair
    unsigned long long* best;  // per (pair, chunk)
};

inline VerifyWs layout(Arena& a, long long rows1, int npairs, int iters) {
    const size_t r1 = (size_t)(rows1 > 0 ? rows1 : 0), np = (size_t)(npairs > 0 ? npairs : 0);
    const size_t ch = (size_t)(iters > 0 ? chunks_of(iters) : 1);
    return {a.take<double>(r1 * 4), a.take<int>(np), a.take<unsigned long long>(np * ch)};
}

// ================================================================ the RANSAC skeleton
// Everything above the primitives, once, for a model M: a struct of constants and
// __device__ __forceinline__ static functions (Homography: rr_verify.hip, Fundamental and Essential: rr_epipolar.hip).
//   SAMPLE      records of a minimal sample          FIT_MIN     fewest points of the least-squares fit
//   ROOTS       most matrices through one sample     KEY_SLOTS   key values per hypothesis (>= ROOTS)
//   ACC         sums the fit's normal matrix is of   REFIT_OCC   blocks per CU k_refit / k_fit_batch are built for
//   WALK_UNROLL unroll factor of the scoring walk    WALK_SPLIT  the walk is written once per address space
//   TRUST_ROOT  the refit takes matrix `root` of the winner's sample as it comes (false: only where hypotheses() > 0)
//   Ctx, load(K1, K2, p)        what the model knows of pair p besides its records (empty, or the intrinsics);
//                               it reaches hypotheses, finish and emit
//   hypotheses(ctx, q, Mx) -> n the matrices through the sample q; those past n are all zero
//   inlier(m, x1, y1, x2, y2, th2)
//   accumulate(n, x1, y1, x2, y2, w, acc)   one point, normalised by n, into the ACC sums
//   write_matrix(acc, a)        the block's totals -> the symmetric 9 x 9 matrix in LDS
//   finish(ctx, e9, n, out)     its smallest eigenvector -> the de-normalised 3 x 3
//   emit(ctx, have, m, out)     the refit's final write
// A model adds no kernel and no host code: its two entry points are verify_pairs_impl<M> and
// fit_batch_impl<M>.  The arithmetic of a model stays in its own file, statement for statement: the
// files are compiled with the default floating-point contraction, so moving an expression moves bits.

// (count desc, t asc, root asc) as one integer: t < 2^24
template <typename M>
__device__ __forceinline__ unsigned long long ransac_key(int count, int t, int root) {
    return ((unsigned long long)(unsigned)count << 32) | (unsigned long long)(0xffffffffu - (unsigned)(M::KEY_SLOTS * t + root));
}

// every lane walks all m records once (the same address in every lane) and scores every root
template <typename M>
__device__ __forceinline__ void count_all(const double (&Mx)[M::ROOTS][9], const double* __restrict__ rec, int m,
                                          double th2, int (&c)[M::ROOTS]) {
#pragma unroll
    for (int k = 0; k < M::ROOTS; ++k) c[k] = 0;
#pragma unroll M::WALK_UNROLL
    for (int i = 0; i < m; ++i) {
        const double2 a = *reinterpret_cast<const double2*>(rec + 4 * i);
        const double2 b = *reinterpret_cast<const double2*>(rec + 4 * i + 2);
#pragma unroll
        for (int k = 0; k < M::ROOTS; ++k) c[k] += M::inlier(Mx[k], a.x, a.y, b.x, b.y, th2) ? 1 : 0;
    }
}

// block (c, p) scores hypotheses t = 256 c .. 256 c + 255 of pair p, one per thread; the block's best key -> best[p][c]
template <typename M>
__global__ void __launch_bounds__(V_TB) k_ransac(const double* __restrict__ rec, const long long* __restrict__ off1,
                                                 long long rows1, const int* __restrict__ cnt, int npairs, int iters,
                                                 int chunks, double th2, unsigned long long seed,
                                                 const double* __restrict__ K1, const double* __restrict__ K2,
                                                 unsigned long long* __restrict__ best) {
    __shared__ __attribute__((aligned(16))) double s_rec[V_STAGE * 4];
    __shared__ unsigned long long s_red[4];
    const int tid = threadIdx.x;
    const int t = (int)blockIdx.x * V_TB + tid;
    for (int p = blockIdx.y; p < npairs; p += gridDim.y) {
        const int m = cnt[p];
        unsigned long long key = 0ull;
        if (m >= M::SAMPLE) {   // block-uniform
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
                double q[M::SAMPLE][4];
                sample<M::SAMPLE>(src, seed, p, t, m, q);
                double Mx[M::ROOTS][9];
                // once per pair and thread, next to its only use: loaded before the staging it stays live across
                // it and k_ransac<Essential> spills 236 B per lane more
                const typename M::Ctx ctx = M::load(K1, K2, p);
                if (M::hypotheses(ctx, q, Mx) > 0) {
                    int c[M::ROOTS];
                    if constexpr (M::WALK_SPLIT) {   // a walk per address space: LDS reads, global reads
                        if (staged) count_all<M>(Mx, s_rec, m, th2, c);
                        else count_all<M>(Mx, r, m, th2, c);
                    } else {                         // one walk over a generic pointer: a third of the code
                        count_all<M>(Mx, src, m, th2, c);
                    }
#pragma unroll
                    for (int k = M::ROOTS - 1; k >= 0; --k) {
                        const unsigned long long kk = c[k] > 0 ? ransac_key<M>(c[k], t, k) : 0ull;
                        key = kk > key ? kk : key;
                    }
                }
            }
        }
        key = block_max_u64(key, s_red);
        if (tid == 0) best[(long long)p * chunks + blockIdx.x] = key;
    }
}

// block-parallel inlier count of mx over the m records of a pair
template <typename M>
__device__ __forceinline__ int count_block(const double (&mx)[9], const double* __restrict__ rec, int m, double th2, int* s4) {
    int c = 0;
    for (int i = threadIdx.x; i < m; i += V_TB) {
        const double2 a = *reinterpret_cast<const double2*>(rec + 4 * (long long)i);
        const double2 b = *reinterpret_cast<const double2*>(rec + 4 * (long long)i + 2);
        c += M::inlier(mx, a.x, a.y, b.x, b.y, th2) ? 1 : 0;
    }
    return block_sum_i(c, s4);
}

// ---------------------------------------------------------------- the least-squares fit, block-wide
template <typename M>
struct FitLds {
    double a[81];            // the normal matrix, then its Jacobi iterate
    double v[81];            // eigenvectors (columns)
    double tmp[5 * M::ACC];  // block_sum_d
};

template <typename M>
struct SrcInliers {      // the inliers of mx among the records of a pair, weight 1 (SrcPoints: above)
    const double* rec;
    int n;
    double mx[9];
    double th2;
    __device__ __forceinline__ bool get(int i, double& x1, double& y1, double& x2, double& y2, double& w) const {
        const double2 a = *reinterpret_cast<const double2*>(rec + 4 * (long long)i);
        const double2 b = *reinterpret_cast<const double2*>(rec + 4 * (long long)i + 2);
        x1 = a.x; y1 = a.y; x2 = b.x; y2 = b.y; w = 1.0;
        return M::inlier(mx, x1, y1, x2, y2, th2);
    }
};

// normalize_points of both sides: u = sc x + tx, v = sc y + ty; mx2, my2 the means of side 2
struct FitNorm {
    double sc1, tx1, ty1, sc2, tx2, ty2, mx2, my2;
};

// The reference's fit (find_homography_dlt, find_fundamental) on the selected points of src; every
// thread of the block calls it and returns the same out.  false: fewer than M::FIT_MIN selected
// points (out untouched).  Three passes, each a per-thread chain over i = tid, tid + 256, ... and a
// block sum: the means; the mean distances; the M::ACC sums of the normal matrix.
template <typename M, typename Src>
__device__ __forceinline__ bool fit_block(const typename M::Ctx& ctx, const Src& src, FitLds<M>& L, double (&out)[9]) {
    const int tid = threadIdx.x;
    double x1, y1, x2, y2, w;
    // normalize_points: mean, then sqrt(2) / (mean distance to it + eps)
    double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < src.n; i += V_TB)
        if (src.get(i, x1, y1, x2, y2, w)) { s5[0] += 1.0; s5[1] += x1; s5[2] += y1; s5[3] += x2; s5[4] += y2; }
    block_sum_d<5>(s5, L.tmp);
    const double cnt = s5[0];
    if (cnt < (double)M::FIT_MIN) return false;   // block-uniform
    const double mx1 = s5[1] / cnt, my1 = s5[2] / cnt, mx2 = s5[3] / cnt, my2 = s5[4] / cnt;
    double s2[2] = {0.0, 0.0};
    for (int i = tid; i < src.n; i += V_TB)
        if (src.get(i, x1, y1, x2, y2, w)) {
            const double ax = x1 - mx1, ay = y1 - my1, bx = x2 - mx2, by = y2 - my2;
            s2[0] += sqrt(ax * ax + ay * ay);
            s2[1] += sqrt(bx * bx + by * by);
        }
    block_sum_d<2>(s2, L.tmp);
    const double sc1 = V_RT2 / (s2[0] / cnt + V_EPS), sc2 = V_RT2 / (s2[1] / cnt + V_EPS);
    const double tx1 = -sc1 * mx1, ty1 = -sc1 * my1, tx2 = -sc2 * mx2, ty2 = -sc2 * my2;
    const FitNorm nrm = {sc1, tx1, ty1, sc2, tx2, ty2, mx2, my2};
    double acc[M::ACC];
#pragma unroll
    for (int e = 0; e < M::ACC; ++e) acc[e] = 0.0;
    for (int i = tid; i < src.n; i += V_TB)
        if (src.get(i, x1, y1, x2, y2, w)) M::accumulate(nrm, x1, y1, x2, y2, w, acc);
    block_sum_d<M::ACC>(acc, L.tmp);
    __syncthreads();   // the previous call's readers of L.a / L.v are done
    M::write_matrix(acc, L.a);   // every thread holds the totals
    // the eigenvector of the smallest eigenvalue (ties: the lower index)
    double e9[9];
    jacobi_smallest9(L.a, L.v, e9);
    M::finish(ctx, e9, nrm, out);
    return true;
}

// one block per pair: the winner over the chunks (integer max of the keys), its matrix recomputed
// from (t, root), then `refine` rounds of {inlier set S, the fit on S, accept while the count does
// not drop}; writes inliers, the matrix and the side-1 mask
template <typename M>
__global__ void __launch_bounds__(V_TB, M::REFIT_OCC)
k_refit(const float* __restrict__ kp1, const long long* __restrict__ off1, long long rows1, const float* __restrict__ kp2,
        const long long* __restrict__ off2, long long rows2, const long long* __restrict__ match, int npairs, int max_n1,
        const double* __restrict__ rec, const int* __restrict__ cnt, const unsigned long long* __restrict__ best, int chunks,
        double th2, int refine, unsigned long long seed, const double* __restrict__ K1, const double* __restrict__ K2,
        int* __restrict__ inliers, double* __restrict__ Mout, unsigned char* __restrict__ mask) {
    __shared__ FitLds<M> L;
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
        const typename M::Ctx ctx = M::load(K1, K2, p);
        unsigned long long key = 0ull;
        for (int c = tid; c < chunks; c += V_TB) {
            const unsigned long long k = best[(long long)p * chunks + c];
            key = k > key ? k : key;
        }
        key = block_max_u64(key, s_red);
        double mx[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) mx[i] = 0.0;
        int count = 0;
        bool have = m >= M::SAMPLE && key != 0ull;   // block-uniform
        if (have) {
            const unsigned tr = 0xffffffffu - (unsigned)(key & 0xffffffffull);
            const int t = (int)(tr / M::KEY_SLOTS), root = (int)(tr % M::KEY_SLOTS);
            {
                double q[M::SAMPLE][4];
                sample<M::SAMPLE>(r, seed, p, t, m, q);
                double Mx[M::ROOTS][9];
                const int n = M::hypotheses(ctx, q, Mx);
                have = M::TRUST_ROOT || n > 0;
#pragma unroll
                for (int i = 0; i < 9; ++i) {
                    mx[i] = Mx[M::ROOTS - 1][i];
#pragma unroll
                    for (int k = M::ROOTS - 2; k >= 0; --k) mx[i] = root == k ? Mx[k][i] : mx[i];
                }
            }
            if (have) count = count_block<M>(mx, r, m, th2, s_cnt);
            have = have && count > 0;
            for (int it = 0; have && it < refine; ++it) {
                SrcInliers<M> src;
                src.rec = r; src.n = m; src.th2 = th2;
#pragma unroll
                for (int i = 0; i < 9; ++i) src.mx[i] = mx[i];
                double m2[9];
                if (!fit_block<M>(ctx, src, L, m2) || !all_finite9(m2)) break;
                const int c2 = count_block<M>(m2, r, m, th2, s_cnt);
                if (c2 < count) break;
                count = c2;
#pragma unroll
                for (int i = 0; i < 9; ++i) mx[i] = m2[i];
            }
        }
        if (!have) {
            count = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i) mx[i] = 0.0;
        }
        if (tid == 0) {
            inliers[p] = count;
            M::emit(ctx, have, mx, Mout + 9 * (long long)p);
        }
        // the mask straight from the rows: the same values and the same test as the records
        for (long long i = tid; i < n1; i += V_TB) {
            const long long j = match[b1 + i];
            bool in = false;
            if (have && j >= 0 && j < n2) {
                const float2 a = *reinterpret_cast<const float2*>(kp1 + 2 * (b1 + i));
                const float2 b = *reinterpret_cast<const float2*>(kp2 + 2 * (b2 + j));
                in = M::inlier(mx, (double)a.x, (double)a.y, (double)b.x, (double)b.y, th2);
            }
            mask[b1 + i] = in ? 1 : 0;
        }
        __syncthreads();
    }
}

// the same fit on caller-supplied float64 points with optional weights, one block per point set
template <typename M>
__global__ void __launch_bounds__(V_TB, M::REFIT_OCC)
k_fit_batch(const double* __restrict__ p1, const double* __restrict__ p2, const double* __restrict__ wt,
            const long long* __restrict__ off, long long rows, int npairs, double* __restrict__ Mout) {
    __shared__ FitLds<M> L;
    for (int p = blockIdx.x; p < npairs; p += gridDim.x) {
        long long b, n;
        pair_range(off, p, rows, b, n);
        SrcPoints src;
        src.p1 = p1 + 2 * b; src.p2 = p2 + 2 * b; src.wt = wt ? wt + b : nullptr;
        src.n = (int)n;
        double mx[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) mx[i] = 0.0;
        fit_block<M>(typename M::Ctx{}, src, L, mx);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) Mout[9 * (long long)p + i] = mx[i];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- host: launches (argument checks: rr_internal.h)
// rr_verify_pairs / rr_verify_pairs_epipolar / rr_verify_pairs_essential: compaction, k_ransac<M>, k_refit<M>
// (K1, K2: the per-pair data of a model with a Ctx, NULL otherwise)
template <typename M>
int verify_pairs_impl(const char* name, const float* kp1, const long long* off1, long long rows1, const float* kp2,
                      const long long* off2, long long rows2, const long long* match, int npairs, int max_n1, double th,
                      int iters, int refine, unsigned long long seed, const double* K1, const double* K2, int* inliers,
                      double* Mout, unsigned char* mask, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string w(name);
    if (npairs >= 0 && rows1 >= 0 && rows2 >= 0 && max_n1 >= 0) {   // a negative size is reported first, by check_pair_args
        if (iters < 1) return fail(RR_EINVAL, w + ": iters must be >= 1");
        if (iters > (1 << 24)) return fail(RR_EINVAL, w + ": iters above 2^24");
        if (refine < 0) return fail(RR_EINVAL, w + ": refine must be >= 0");
        if (!(th > 0.0) || !std::isfinite(th)) return fail(RR_EINVAL, w + ": th must be positive and finite");
    }
    int rc = check_pair_args(w, kp1, off1, rows1, kp2, off2, rows2, match, npairs, max_n1);
    if (rc) return rc;
    if (npairs > 0 && (rows1 > 0 && !mask)) return fail(RR_EINVAL, w + ": null output");
    if (npairs > 0 && (!inliers || !Mout)) return fail(RR_EINVAL, w + ": null output");
    if constexpr (!std::is_empty<typename M::Ctx>::value) {   // a model with per-pair data: the two intrinsics
        if (npairs > 0 && (!K1 || !K2)) return fail(RR_EINVAL, w + ": null K");
        if ((((uintptr_t)K1) & 15) || (((uintptr_t)K2) & 15)) return fail(RR_EINVAL, w + ": K must be 16-byte aligned");
    }
    Arena arena(workspace, workspace_bytes);
    const auto [rec, cnt, best] = layout(arena, rows1, npairs, iters);
    if (!workspace || !arena.fits()) return fail(RR_ENOSPACE, w + ": workspace too small");
    if (npairs == 0) return RR_OK;
    hipStream_t s = as_stream(stream);
    const int chunks = chunks_of(iters);
    const unsigned gp = (unsigned)(npairs < 65535 ? npairs : 65535);
    hipLaunchKernelGGL(k_verify_compact, dim3(gp), dim3(V_TB), 0, s, kp1, off1, rows1, kp2, off2, rows2, match, npairs,
                       max_n1, rec, cnt);
    rc = check_launch((w + ": compact").c_str());
    if (rc) return rc;
    hipLaunchKernelGGL(k_ransac<M>, dim3((unsigned)chunks, gp), dim3(V_TB), 0, s, rec, off1, rows1, cnt, npairs, iters,
                       chunks, th * th, seed, K1, K2, best);
    rc = check_launch((w + ": ransac").c_str());
    if (rc) return rc;
    hipLaunchKernelGGL(k_refit<M>, dim3(gp), dim3(V_TB), 0, s, kp1, off1, rows1, kp2, off2, rows2, match, npairs, max_n1,
                       rec, cnt, best, chunks, th * th, refine, seed, K1, K2, inliers, Mout, mask);
    return check_launch((w + ": refit").c_str());
}

// rr_homography_dlt / rr_fundamental_dlt: k_fit_batch<M>
template <typename M>
int fit_batch_impl(const char* name, const double* pts1, const double* pts2, const double* weights, const long long* off,
                   long long rows, int npairs, double* Mout, void* stream) {
    const std::string w(name);
    const int rc = check_point_set_args(w, pts1, pts2, off, rows, npairs);
    if (rc) return rc;
    if (npairs > 0 && !Mout) return fail(RR_EINVAL, w + ": null output");
    if (npairs == 0) return RR_OK;
    hipLaunchKernelGGL(k_fit_batch<M>, dim3((unsigned)(npairs < 65535 ? npairs : 65535)), dim3(V_TB), 0, as_stream(stream),
                       pts1, pts2, weights, off, rows, npairs, Mout);
    return check_launch(name);
}

}  // namespace

}  // namespace rr
