// librr.so — what the two geometric verifiers (rr_verify.hip: homography, rr_epipolar.hip:
// fundamental matrix) and the pose entry after them (rr_pose.hip) share: the pair ranges, the
// counter-hash sampler of rr.h, the compaction of kept matches into records, the block reductions
// with one fixed order, the round-robin cyclic Jacobi on a symmetric 9 x 9 matrix in LDS, the
// cyclic Jacobi on a symmetric 3 x 3 in registers and the workspace layout.  The files compile
// this with the same floating-point settings, so a shared routine yields the same bits in each.
#pragma once
#include "rr_internal.h"
#include "rr_workspace.h"

#include <math.h>

namespace rr {

namespace {

constexpr int V_TB = 256;        // threads of every block (fixed: it fixes the summation order)
constexpr int V_STAGE = 1024;    // records of the LDS stage of the RANSAC kernels (x 32 B = 32 KiB)
constexpr int V_SWEEPS = 16;     // cyclic Jacobi: the most sweeps (it stops after 6 - 8)
constexpr double V_JTOL = 0x1p-52; // a rotation is skipped where |a_pq| <= V_JTOL sqrt(a_pp a_qq)
constexpr double V_EPS = 1e-8;   // the reference's eps (normalize_points, find_homography_dlt, find_fundamental)

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
// draws before it only, so the first four of any K are draw4's
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

__device__ __forceinline__ void draw4(unsigned long long seed, int p, int t, int m, int (&smp)[4]) {
    draw_n<4>(seed, p, t, m, smp);
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

}  // namespace

}  // namespace rr
