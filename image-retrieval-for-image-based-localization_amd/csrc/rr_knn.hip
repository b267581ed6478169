// librr.so — brute-force cosine kNN with exact ordering.
//
// Replaces `scores = np.dot(vecs.T, qvecs); ranks = np.argsort(-scores, 0)`
// (scripts/test.py:247-248) restricted to the first k ranks.
//
// Pipeline per query batch (all on one HIP stream, no host sync):
//  1. score GEMM   slab[q][n] = <q, db_n> for a pass of G chunks of L rows,
//                  MFMA (bf16 or exact f32), f32 scores.  The slab is sized to
//                  at most 512 MiB per pass: fewer, fuller GEMM tile loops
//                  (Q = 128 over 1M rows: 64 / 256 / 512 MiB -> 1.71 / 1.53 /
//                  1.49 ms; Q = 1024: 8.27 / 7.62 / 7.44 ms).
//  2. chunk select per (query, chunk): radix-select of the top KC fp32 keys
//                  over L scores staged in LDS; candidates emitted in index
//                  order (deterministic, ties -> lower index).
//  3. final        per query: radix-select top KC of all chunk candidates;
//                  re-score them in float64 from the float32 rows (exact
//                  products, fixed-order reduction; one wave per candidate
//                  over the whole chip); bitonic sort by (score desc,
//                  index asc), emit k.
// KC > k is the screening margin: bf16 scores err by ~1e-4, exact-f32 by
// ~1e-7, far below KC-k candidates' worth of score density at the boundary.
#include "rr_internal.h"
#include "rr_workspace.h"

#include <cstdlib>
#include <type_traits>

namespace rr {


constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int CHUNK_L = 16384;           // rows per select chunk (keys staged in 64 KiB LDS)
// score-slab budget per GEMM pass (Infinity-Cache resident); RR_KNN_SLAB_MB overrides (tuning)
static size_t slab_budget() {
    static size_t b = 0;
    if (!b) {
        const char* e = getenv("RR_KNN_SLAB_MB");
        const long v = e ? atol(e) : 0;
        b = (v >= 16 && v <= 1024) ? (size_t)v << 20 : (512ull << 20);
    }
    return b;
}
typedef __attribute__((ext_vector_type(4))) float f32x4_knn_t;
constexpr int MAX_SORT = 8192;
constexpr int PREFIX_CHUNKS = 4;         // chunks through the slab path before the screening GEMM
constexpr int TOPK_BINS = 2048;          // radix-select histogram (11-bit digits)

__device__ __forceinline__ uint32_t fkey(float f) {
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float funkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Radix select of the K-th largest key of keys[0..len) (SKIP0: key 0 marks
// a slot screened out before the select — neither counted nor emitted).
// Returns the K-th key and sets *rem to how many keys equal to it belong to
// the top K.  Precondition: more than K counted keys.
template <bool SKIP0, typename GK>
__device__ uint32_t radix_kth(GK getk, int len, int K, int* smem_i, int* rem) {
    int* hist = smem_i;                        // TOPK_BINS
    int* sel = smem_i + TOPK_BINS + 32;        // [0]=digit, [1]=remaining
    const int tid = threadIdx.x;
    int remaining = K;
    // digits of 11, 11 and 10 bits: the first covers sign, exponent and two
    // mantissa bits, so the scores' few exponents spread over many bins
    // (fewer same-address LDS atomics than an 8-bit top digit), 3 passes.
    uint32_t prefix = 0, mask = 0;
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
        const int bits = pass == 2 ? 10 : 11;
        const uint32_t dmask = (1u << bits) - 1;
        for (int i = tid; i < TOPK_BINS; i += SEL_THREADS) hist[i] = 0;
        __syncthreads();
        for (int i = tid; i < len; i += SEL_THREADS) {
            uint32_t k = getk(i);
            if ((k & mask) == prefix && (!SKIP0 || k != 0u)) atomicAdd(&hist[(k >> shift) & dmask], 1);
        }
        __syncthreads();
        if (tid < 64) {
            // wave 0: lane owns bins [32*tid, 32*tid + 32); suffix sums
            // across lanes (lane 63 holds the highest digits), then a walk
            // down its own bins to the digit holding the K-th key
            constexpr int PER = TOPK_BINS / 64;
            int lsum = 0;
#pragma unroll
            for (int e = 0; e < PER; ++e) lsum += hist[tid * PER + ((e + tid) & (PER - 1))];  // rotated: conflict-free
            int sfx = lsum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                int y = __shfl_down(sfx, o, 64);
                if (tid + o < 64) sfx += y;
            }
            int acc = sfx - lsum;  // count of keys with digit above this lane's bins
            if (acc < remaining && acc + lsum >= remaining) {
                for (int e = PER - 1; e >= 0; --e) {
                    const int c = hist[tid * PER + e];
                    if (acc + c >= remaining) {
                        sel[0] = tid * PER + e;
                        sel[1] = remaining - acc;
                        break;
                    }
                    acc += c;
                }
            }
        }
        __syncthreads();
        const int digit = sel[0];
        remaining = sel[1];
        prefix |= (uint32_t)digit << shift;
        mask |= dmask << shift;
        __syncthreads();
    }
    *rem = remaining;
    return prefix;
}

// Top-K (largest keys) of keys[0..len).  `getk(i)` gives the key, `geti(i)`
// the payload index; K results are written to out_k/out_i in ascending
// position order; missing slots get (key 0, index -1).
// Ties at the K-th key: by position (IDXTIE false — the position order is the
// index order for the chunk selects, whose keys come in row order) or by
// smallest index (IDXTIE true — candidate pools appended by the screening
// epilogue in arbitrary order; a second radix pass on ~index picks the
// lowest indices among the tied keys).
// SKIP0: key 0 marks a slot screened out before the select (below the
// query's running threshold); such keys are neither counted nor emitted,
// `nvalid` is the number of non-zero keys, and fewer than K of them are
// emitted followed by (0, -1) padding.  Returns the K-th key (0 when every
// valid key was taken).
template <bool SKIP0 = false, bool IDXTIE = false, typename GK, typename GI>
__device__ uint32_t block_topk(GK getk, GI geti, int len, int K, uint32_t* out_k, int* out_i, int* smem_i,
                               int nvalid = -1) {
    if (!SKIP0) nvalid = len;
    int* wsum = smem_i + TOPK_BINS;            // SEL_WAVES + 1
    const int tid = threadIdx.x;
    uint32_t thr = 0;
    int remaining = K;
    if (nvalid > K) thr = radix_kth<SKIP0>(getk, len, K, smem_i, &remaining);
    // index tie-break: among the keys equal to thr, take the `remaining` smallest indices
    bool itie = false;
    int ithr = 0;
    if constexpr (IDXTIE) {
        if (nvalid > K && thr != 0u) {
            int* cnt = smem_i + TOPK_BINS + 56;
            if (tid == 0) cnt[0] = 0;
            __syncthreads();
            int e = 0;
            for (int i = tid; i < len; i += SEL_THREADS) e += getk(i) == thr;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
            if ((tid & 63) == 0 && e) atomicAdd(cnt, e);
            __syncthreads();
            const int E = cnt[0];
            __syncthreads();
            if (E > remaining) {
                int rem2;
                const uint32_t t2 = radix_kth<true>(
                    [&](int i) { return getk(i) == thr ? ~(uint32_t)geti(i) : 0u; }, len, remaining, smem_i, &rem2);
                itie = true;
                ithr = (int)~t2;  // indices are unique: exactly `remaining` tied keys have index <= ithr
            }
        }
    }
    const int take_eq = itie ? 0x7fffffff : remaining;
    // ordered emission: wave w owns the contiguous range [wb, we) and walks it
    // 64 keys at a time (stride-1 reads); ballot + mbcnt give each key's rank
    // among the taken keys before it, one 16-entry scan orders the waves.
    const int lane = tid & 63, w = tid >> 6;
    int* wgt = wsum;                 // SEL_WAVES counts of keys above the threshold
    int* weq = smem_i + TOPK_BINS + 40;  // SEL_WAVES counts of keys equal to it
    const bool sel_all = nvalid <= K;
    const int wseg = (((len + SEL_WAVES - 1) / SEL_WAVES) + 63) & ~63;
    const int wb = min(len, w * wseg), we = min(len, wb + wseg);
    auto is_eq = [&](bool in, uint32_t k, int i) {
        return in && !sel_all && k == thr && (!itie || geti(i) <= ithr);
    };
    int cgt = 0, ceq = 0;
    for (int i0 = wb; i0 < we; i0 += 64) {
        const int i = i0 + lane;
        const bool in = i < we;
        const uint32_t k = in ? getk(i) : 0u;
        cgt += __popcll(__ballot(in && (sel_all ? (!SKIP0 || k != 0u) : k > thr)));
        ceq += __popcll(__ballot(is_eq(in, k, i)));
    }
    if (lane == 0) {
        wgt[w] = cgt;
        weq[w] = ceq;
    }
    __syncthreads();
    int pgt = 0, peq = 0;
    for (int j = 0; j < w; ++j) {
        pgt += wgt[j];
        peq += weq[j];
    }
    for (int i0 = wb; i0 < we; i0 += 64) {
        const int i = i0 + lane;
        const bool in = i < we;
        const uint32_t k = in ? getk(i) : 0u;
        const bool gt = in && (sel_all ? (!SKIP0 || k != 0u) : k > thr);
        const bool eq = is_eq(in, k, i);
        const unsigned long long bg = __ballot(gt), be = __ballot(eq);
        const int rg = pgt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bg >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bg, 0u));
        const int re = peq + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(be >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)be, 0u));
        if (gt) {
            const int slot = rg + min(re, take_eq);
            out_k[slot] = k;
            out_i[slot] = geti(i);
        } else if (eq && re < take_eq) {
            out_k[rg + re] = k;
            out_i[rg + re] = geti(i);
        }
        pgt += __popcll(bg);
        peq += __popcll(be);
    }
    if (sel_all) {
        for (int i = nvalid + tid; i < K; i += SEL_THREADS) {
            out_k[i] = 0u;
            out_i[i] = -1;
        }
    }
    __syncthreads();
    return thr;
}

// ---------------------------------------------------------------- chunk select
// grid (nq, chunks in pass).  slab row q: slab + q*S; chunk c covers
// columns [c*L, c*L + len).  Global row index of column j = row0 + c*L + j.
// tau[q]: the query's running screen threshold = the largest K-th key any
// earlier (or concurrent) chunk of this search has selected.  Keys below it
// cannot reach the final top KC — that chunk already put KC keys >= tau into
// the candidate pool — so they are dropped at load time (key 0): the radix
// passes skip them and a chunk with <= KC survivors skips the passes
// altogether.  The final select's result is unchanged by construction:
// every candidate removed is below KC pool keys, and the kept ones keep their
// index order.  Reads of tau race benignly with other chunks' atomicMax (any
// value ever stored is a valid bound).
__global__ void __launch_bounds__(SEL_THREADS) k_chunk_select(const float* __restrict__ slab, long long S, int L,
                                                              int rows_in_pass, int row0, int chunk0, int nchunks,
                                                              int KC, uint32_t* __restrict__ cand_k,
                                                              int* __restrict__ cand_i, uint32_t* tau) {
    extern __shared__ __attribute__((aligned(16))) uint32_t keys[];  // L
    __shared__ int smi[TOPK_BINS + 64];
    __shared__ int nsurv;
    __shared__ int wcnt[SEL_WAVES];
    const int q = blockIdx.x, c = blockIdx.y;
    const int len = min(L, rows_in_pass - c * L);
    const float* src = slab + (long long)q * S + (long long)c * L;
    const uint32_t tq = __atomic_load_n(tau + q, __ATOMIC_RELAXED);
    if (threadIdx.x == 0) nsurv = 0;
    __syncthreads();
    int mine = 0;
    auto keep = [&](float f) {
        const uint32_t k = fkey(f);
        const bool ok = k >= tq;
        mine += ok;
        return ok ? k : 0u;
    };
    const long long o = ((long long)q * nchunks + chunk0 + c) * KC;
    const int base = row0 + c * L;
    // slab rows start 16-B aligned (S % 4 == 0, L % 4 == 0): float4 loads.
    if (len == CHUNK_L) {
        // Full chunk: wave w owns the contiguous keys [1024 w, 1024 w + 1024),
        // 4 float4 per lane, all loads issued before any use.  When at most KC
        // keys survive the screen (every chunk after the first few of a
        // search) they are emitted straight from registers in index order —
        // wave prefix, then per float4 a lane scan — with no LDS staging and
        // no radix pass; otherwise the keys go to LDS for block_topk.
        constexpr int PER = CHUNK_L / (SEL_THREADS * 4);
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        float4 v[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) v[j] = reinterpret_cast<const float4*>(src)[w * 256 + j * 64 + lane];
        uint4 kq[PER];
        int cnt[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) kq[j] = make_uint4(keep(v[j].x), keep(v[j].y), keep(v[j].z), keep(v[j].w));
        // Pre-screen bound (KC <= 1024, KC % 16 == 0): every wave sorts its 64
        // lane maxima (16 keys each) and takes the (KC/16)-th largest; the
        // smallest of these 16 wave values m has KC distinct keys >= it (KC/16
        // lane maxima per wave), so m <= the chunk's KC-th key and keys below
        // it cannot be selected.  ~2-4 % of a chunk survives (vs all of it):
        // the radix passes run over a compacted few hundred keys.
        uint32_t m = 0u;
        if (KC <= 1024 && (KC & 15) == 0) {
            uint32_t lm = 0u;
#pragma unroll
            for (int j = 0; j < PER; ++j) lm = max(lm, max(max(kq[j].x, kq[j].y), max(kq[j].z, kq[j].w)));
            // bitonic sort of the 64 lane maxima, descending
#pragma unroll
            for (int kb = 2; kb <= 64; kb <<= 1)
#pragma unroll
                for (int jb = kb >> 1; jb > 0; jb >>= 1) {
                    const uint32_t o2 = (uint32_t)__shfl_xor((int)lm, jb, 64);
                    const bool desc = (lane & kb) == 0, lower = (lane & jb) == 0;
                    lm = (desc == lower) ? max(lm, o2) : min(lm, o2);
                }
            const uint32_t wm = (uint32_t)__shfl((int)lm, KC / 16 - 1, 64);
            if (lane == 0) wcnt[w] = (int)wm;
            __syncthreads();
            m = 0xffffffffu;
#pragma unroll
            for (int j = 0; j < SEL_WAVES; ++j) m = min(m, (uint32_t)wcnt[j]);
            __syncthreads();
        }
        mine = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            uint32_t kk[4] = {kq[j].x, kq[j].y, kq[j].z, kq[j].w};
            int c2 = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                kk[e] = kk[e] >= m ? kk[e] : 0u;
                c2 += kk[e] != 0u;
            }
            kq[j] = make_uint4(kk[0], kk[1], kk[2], kk[3]);
            cnt[j] = c2;
            mine += c2;
        }
#pragma unroll
        for (int s2 = 32; s2 > 0; s2 >>= 1) mine += __shfl_xor(mine, s2, 64);
        if (lane == 0) wcnt[w] = mine;
        __syncthreads();
        int nvalid = 0, before = 0;
#pragma unroll
        for (int j = 0; j < SEL_WAVES; ++j) {
            nvalid += wcnt[j];
            before += j < w ? wcnt[j] : 0;
        }
        if (nvalid > KC && nvalid <= CHUNK_L / 2) {
            // compact the survivors into LDS in index order (keys | indices)
            uint32_t* ck = keys;
            int* ci = reinterpret_cast<int*>(keys + CHUNK_L / 2);
            int run = before;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                int x = cnt[j];
#pragma unroll
                for (int s2 = 1; s2 < 64; s2 <<= 1) {
                    const int y = __shfl_up(x, s2, 64);
                    if (lane >= s2) x += y;
                }
                int slot = run + x - cnt[j];
                run += __shfl(x, 63, 64);
                const uint32_t kk[4] = {kq[j].x, kq[j].y, kq[j].z, kq[j].w};
                const int i0 = base + (w * 256 + j * 64 + lane) * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (kk[e] != 0u) {
                        ck[slot] = kk[e];
                        ci[slot] = i0 + e;
                        ++slot;
                    }
            }
            __syncthreads();
            const uint32_t thr = block_topk([&](int i) { return ck[i]; }, [&](int i) { return ci[i]; }, nvalid, KC,
                                            cand_k + o, cand_i + o, smi);
            if (threadIdx.x == 0 && thr > tq) atomicMax(tau + q, thr);
            return;
        }
        if (nvalid <= KC) {
            int run = before;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                int x = cnt[j];
#pragma unroll
                for (int s2 = 1; s2 < 64; s2 <<= 1) {
                    const int y = __shfl_up(x, s2, 64);
                    if (lane >= s2) x += y;
                }
                int slot = run + x - cnt[j];
                run += __shfl(x, 63, 64);
                const uint32_t kk[4] = {kq[j].x, kq[j].y, kq[j].z, kq[j].w};
                const int i0 = base + (w * 256 + j * 64 + lane) * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (kk[e] != 0u) {
                        cand_k[o + slot] = kk[e];
                        cand_i[o + slot] = i0 + e;
                        ++slot;
                    }
            }
            for (int i = nvalid + (int)threadIdx.x; i < KC; i += SEL_THREADS) {
                cand_k[o + i] = 0u;
                cand_i[o + i] = -1;
            }
            return;  // block-uniform branch
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) reinterpret_cast<uint4*>(keys)[w * 256 + j * 64 + lane] = kq[j];
        __syncthreads();
        const uint32_t thr = block_topk<true>([&](int i) { return keys[i]; }, [&](int i) { return base + i; }, len,
                                              KC, cand_k + o, cand_i + o, smi, nvalid);
        if (threadIdx.x == 0 && thr > tq) atomicMax(tau + q, thr);
        return;
    }
    {
        const int len4 = len & ~3;
        for (int i = threadIdx.x * 4; i < len4; i += SEL_THREADS * 4) {
            const float4 v = *reinterpret_cast<const float4*>(src + i);
            *reinterpret_cast<uint4*>(keys + i) = make_uint4(keep(v.x), keep(v.y), keep(v.z), keep(v.w));
        }
        for (int i = len4 + threadIdx.x; i < len; i += SEL_THREADS) keys[i] = keep(src[i]);
    }
#pragma unroll
    for (int s2 = 32; s2 > 0; s2 >>= 1) mine += __shfl_xor(mine, s2, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&nsurv, mine);
    __syncthreads();
    const int nvalid = nsurv;
    const uint32_t thr = block_topk<true>([&](int i) { return keys[i]; }, [&](int i) { return base + i; }, len, KC,
                                          cand_k + o, cand_i + o, smi, nvalid);
    if (threadIdx.x == 0 && nvalid > KC && thr > tq) atomicMax(tau + q, thr);
}

// ------------------------------------------------------------------ bitonic
// Struct-of-arrays sort of (score f64, index) pairs, best first:
// better(a, b) = a.s > b.s || (a.s == b.s && a.i < b.i).  Sentinel: (-inf, MAX).
template <typename I>
__device__ __forceinline__ bool better(double sa, I ia, double sb, I ib) {
    return sa > sb || (sa == sb && ia < ib);
}
template <typename I>
__device__ void bitonic_best_first(double* ks, I* is, int n) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < n; t += blockDim.x) {
                int p = t ^ j;
                if (p > t) {
                    bool up = (t & k) == 0;
                    double sa = ks[t], sb = ks[p];
                    I ia = is[t], ib = is[p];
                    if (up ? better(sb, ib, sa, ia) : better(sa, ia, sb, ib)) {
                        ks[t] = sb; ks[p] = sa;
                        is[t] = ib; is[p] = ia;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------ final
// Three launches per query batch, so the re-score runs on the whole chip:
//  k_final_select  grid (nq):          top KC of the chunk candidates -> sel_i[q][KC]
//  k_rescore       grid (npow2/4, nq): one wave per candidate, float64 score
//  k_final_sort    grid (nq):          bitonic (score desc, index asc), emit k
// Staged form (`stage` true: nchunks <= FSEL_MAXCH, dynamic LDS of
// FSEL_LDS bytes): the occupied slots' keys are gathered once, in slot order,
// into LDS (one pass of independent loads) and the select's 5-8 passes read
// LDS instead of re-walking the nchunks x KC slot array in L2.  Unoccupied
// slots are (key 0, index -1) in the unstaged form; one such entry is appended
// when any exists, so the K-th key (and thereby sel_thr) and the selected set
// are the same.  Indices are read from the slot array for the taken keys only.
// Re-score cut (certified): with delta = the screening error bound of the query
// (delta_scale * ||q||), every candidate's exact score lies within delta of its
// screening key, so the k best keys have exact scores >= t_k - delta (t_k = the
// k-th largest candidate key) and so does the exact k-th score; a candidate with
// key < t_k - 2 delta has an exact score < t_k - delta, strictly below it -- it
// cannot be in the top k, and k_rescore skips its float32 row (-inf).
// prune_thr[q] = t_k - 2 delta, or -inf when fewer than k candidates are valid.
__device__ void rescore_cut(const uint32_t* __restrict__ keys, int KC, int k, const float* __restrict__ qr, int d,
                            double delta_scale, int* smi, float* __restrict__ out) {
    __shared__ double red[SEL_WAVES];
    __shared__ int nvs[SEL_WAVES];
    __shared__ uint32_t tk_s;
    uint32_t* lk = reinterpret_cast<uint32_t*>(smi);  // KC <= SEL_THREADS keys (TOPK_BINS >= SEL_THREADS)
    __syncthreads();  // this block's sel_k stores are visible to all its threads; smi is free
    const int tid = threadIdx.x;
    const bool small = KC <= SEL_THREADS;             // block-uniform
    const uint32_t mine = tid < KC && small ? keys[tid] : 0u;
    if (small && tid < KC) lk[tid] = mine;
    if (tid == 0) tk_s = 0u;
    double ss = 0.0;
    for (int t = tid; t < d; t += SEL_THREADS) ss += (double)qr[t] * qr[t];
    ss = wave_sum_d(ss);
    int nv = mine != 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nv += __shfl_xor(nv, o, 64);
    if ((tid & 63) == 0) {
        red[tid >> 6] = ss;
        nvs[tid >> 6] = nv;
    }
    __syncthreads();
    int tot_nv = 0;
    double tot = 0.0;
    for (int w = 0; w < SEL_WAVES; ++w) { tot_nv += nvs[w]; tot += red[w]; }
    if (!small || tot_nv <= k) {  // block-uniform: no cut
        if (tid == 0) *out = -INFINITY;
        return;
    }
    // t_k = the k-th largest valid key: the key x with #{> x} < k <= #{>= x}
    if (mine != 0u) {
        int gt = 0, ge = 0;
        for (int i = 0; i < KC; ++i) {
            const uint32_t v = lk[i];
            gt += v > mine;
            ge += v >= mine;
        }
        if (gt < k && k <= ge) tk_s = mine;  // every writer writes the same value
    }
    __syncthreads();
    if (tid == 0) {
        const double cut = (double)funkey(tk_s) - 2.0 * delta_scale * sqrt(tot) * 1.0001;
        float f = (float)cut;
        if ((double)f > cut) f = nextafterf(f, -INFINITY);  // round the cut down
        *out = f;
    }
}

constexpr int FSEL_CAP = 12288;   // staged keys (48 KiB): ~4.2k occupied for 1M rows at k = 100
constexpr int FSEL_MAXCH = 1024;  // chunk offsets (4 KiB)
constexpr size_t FSEL_LDS = (size_t)(FSEL_CAP + FSEL_MAXCH + 1) * 4;
__global__ void __launch_bounds__(SEL_THREADS) k_final_select(const uint32_t* __restrict__ cand_k,
                                                              const int* __restrict__ cand_i,
                                                              const int* __restrict__ cnt, int nchunks, int KC,
                                                              uint32_t* __restrict__ sel_k, int* __restrict__ sel_i,
                                                              uint32_t* __restrict__ sel_thr, int stage, int k,
                                                              const float* __restrict__ q32, int d, double delta_scale,
                                                              float* __restrict__ prune_thr) {
    __shared__ int smi[TOPK_BINS + 64];
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    const int q = blockIdx.x;
    const int ncand = nchunks * KC;
    const uint32_t* ck = cand_k + (long long)q * ncand;
    const int* ci = cand_i + (long long)q * ncand;
    const int* cq = cnt + (long long)q * nchunks;
    if (stage) {
        uint32_t* lk = reinterpret_cast<uint32_t*>(dyn);
        int* off = reinterpret_cast<int*>(lk + FSEL_CAP);  // nchunks + 1 exclusive offsets
        const int tid = threadIdx.x, lane = tid & 63;
        if (tid < 64) {
            int run = 0;
            for (int b = 0; b < nchunks; b += 64) {
                const int c = b + lane;
                const int v = c < nchunks ? min(cq[c], KC) : 0;
                int x = v;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int y = __shfl_up(x, o, 64);
                    if (lane >= o) x += y;
                }
                if (c < nchunks) off[c] = run + x - v;
                run += __shfl(x, 63, 64);
            }
            if (lane == 0) off[nchunks] = run;
        }
        __syncthreads();
        const int total = off[nchunks];
        if (total < FSEL_CAP) {  // block-uniform
            for (int c = tid >> 6; c < nchunks; c += SEL_WAVES) {
                const int o = off[c], v = off[c + 1] - o;
                for (int j = lane; j < v; j += 64) lk[o + j] = ck[(long long)c * KC + j];
            }
            const bool pad = total < ncand;
            if (pad && tid == 0) lk[total] = 0u;
            __syncthreads();
            auto gi = [&](int i) -> int {
                if (i >= total) return -1;
                int lo = 0, hi = nchunks;  // off[lo] <= i < off[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (off[mid] <= i) lo = mid;
                    else hi = mid;
                }
                return ci[(long long)lo * KC + (i - off[lo])];
            };
            const uint32_t thr = block_topk<false, true>([&](int i) { return lk[i]; }, gi, total + (pad ? 1 : 0), KC,
                                                         sel_k + (long long)q * KC, sel_i + (long long)q * KC, smi);
            if (threadIdx.x == 0) sel_thr[q] = thr;
            if (prune_thr) rescore_cut(sel_k + (long long)q * KC, KC, k, q32 + (long long)q * d, d, delta_scale, smi,
                                       prune_thr + q);
            return;
        }
    }
    // slot (chunk c, position j) holds a candidate when j < min(cnt, KC); the
    // chunk selects fill whole slots (sentinels (0, -1) past their survivors),
    // the screening epilogue appends in arbitrary order -> ties by index
    auto valid = [&](int i) { const int c = i / KC; return i - c * KC < min(cq[c], KC); };
    const uint32_t thr = block_topk<false, true>([&](int i) { return valid(i) ? ck[i] : 0u; },
                                                 [&](int i) { return valid(i) ? ci[i] : -1; }, ncand, KC,
                                                 sel_k + (long long)q * KC, sel_i + (long long)q * KC, smi);
    // every row outside the KC candidates has a screening key <= thr: a chunk's
    // own KC-th key, the running threshold and the pool's KC-th key are all <= it
    if (threadIdx.x == 0) sel_thr[q] = thr;
    if (prune_thr) rescore_cut(sel_k + (long long)q * KC, KC, k, q32 + (long long)q * d, d, delta_scale, smi,
                               prune_thr + q);
}

// After the prefix chunks: tau[q] = the KC-th largest key of the whole prefix
// pool (g0 x KC candidates).  The chunk selects only raised tau to the best
// per-chunk KC-th key, which would let ~KC rows of every screened chunk
// through (slot overflow); the pool's KC-th key lets ~KC / g0 through.
// Still a valid bound: the pool holds KC keys >= it.
__global__ void __launch_bounds__(SEL_THREADS) k_tau_refine(const uint32_t* __restrict__ cand_k, int nchunks, int g0,
                                                            int KC, uint32_t* __restrict__ tau) {
    __shared__ int smi[TOPK_BINS + 64];
    __shared__ int nv;
    const int q = blockIdx.x;
    const uint32_t* ck = cand_k + (long long)q * nchunks * KC;
    const int len = g0 * KC;
    if (threadIdx.x == 0) nv = 0;
    __syncthreads();
    int c = 0;
    for (int i = threadIdx.x; i < len; i += SEL_THREADS) c += ck[i] != 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&nv, c);
    __syncthreads();
    if (nv <= KC) return;  // block-uniform
    int rem;
    const uint32_t t = radix_kth<true>([&](int i) { return ck[i]; }, len, KC, smi, &rem);
    if (threadIdx.x == 0 && t > tau[q]) tau[q] = t;
}

// tau[q] = 0 and the slot counts: chunks [0, g0) are filled whole by the
// chunk select (count KC), the others start empty (screening epilogue).
__global__ void k_knn_reset(uint32_t* __restrict__ tau, int* __restrict__ cnt, int nq, int nchunks, int g0, int KC,
                            int zero_tau) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (zero_tau && i < nq) tau[i] = 0u;
    if (i < (long long)nq * nchunks) cnt[i] = (int)(i % nchunks) < g0 ? KC : 0;
}

// Overflow fix-up of the screened chunks: a (query, chunk) slot that received
// more than KC survivors (the prefix threshold was too low for that chunk —
// e.g. many near-duplicates of the query there) is rebuilt exactly: the
// chunk's scores for that query are recomputed and radix-selected in row
// order, like the chunk select.  The scores must be the SAME bits the score
// GEMM produced (ties across chunks are broken by index only when equal rows
// get equal keys), so they are recomputed with the GEMM's own MFMA, operand
// layout and K order: 16 rows per MFMA as the A operand, the query as column
// 0 of B (the other columns zero; every output element is an independent dot
// product of its row and column).  One block per query walks its chunks;
// chunks that did not overflow cost one load.
template <typename T>
__device__ __forceinline__ void fixup_scores(const T* __restrict__ dr, bool row_ok, const T* __restrict__ qr, bool col0,
                                             int d, f32x4_knn_t& acc) {
    const int kq = (threadIdx.x & 63) >> 4;
    if constexpr (std::is_same<T, int8_t>::value) {  // int8 rows: exact int32 dot products (any order)
        typedef __attribute__((ext_vector_type(4))) int i32x4_knn_t;
        for (int k0 = 0; k0 < d; k0 += 128) {
#pragma unroll
            for (int hs = 0; hs < 2; ++hs) {
                const int off = k0 + (kq + 4 * hs) * 16;
                const uint4 av = row_ok ? *reinterpret_cast<const uint4*>(dr + off) : make_uint4(0, 0, 0, 0);
                const uint4 bv = col0 ? *reinterpret_cast<const uint4*>(qr + off) : make_uint4(0, 0, 0, 0);
                acc = __builtin_bit_cast(f32x4_knn_t, __builtin_amdgcn_mfma_i32_16x16x64_i8(
                    __builtin_bit_cast(i32x4_knn_t, av), __builtin_bit_cast(i32x4_knn_t, bv),
                    __builtin_bit_cast(i32x4_knn_t, acc), 0, 0, 0));
            }
        }
    } else if constexpr (sizeof(T) == 2) {
        for (int k0 = 0; k0 < d; k0 += 64) {
#pragma unroll
            for (int hs = 0; hs < 2; ++hs) {
                const int off = k0 + (kq + 4 * hs) * 8;
                const uint4 av = row_ok ? *reinterpret_cast<const uint4*>(dr + off) : make_uint4(0, 0, 0, 0);
                const uint4 bv = col0 ? *reinterpret_cast<const uint4*>(qr + off) : make_uint4(0, 0, 0, 0);
                acc = H16<T>::mfma(av, bv, acc);
            }
        }
    } else {
        for (int k0 = 0; k0 < d; k0 += 32) {
#pragma unroll
            for (int hs = 0; hs < 2; ++hs) {
                const int off = k0 + (kq + 4 * hs) * 4;
                const float4 av = row_ok ? *reinterpret_cast<const float4*>(dr + off) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 bv = col0 ? *reinterpret_cast<const float4*>(qr + off) : make_float4(0.f, 0.f, 0.f, 0.f);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0);
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(SEL_THREADS) k_slot_fixup(const T* __restrict__ db, long long n_db, const T* __restrict__ q,
                                                            int d, int L, int nchunks, int g0, int KC,
                                                            int* __restrict__ cnt, uint32_t* __restrict__ cand_k,
                                                            int* __restrict__ cand_i, uint32_t* __restrict__ tau) {
    extern __shared__ __attribute__((aligned(16))) uint32_t keys[];  // L
    __shared__ int smi[TOPK_BINS + 64];
    const int qi = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const T* qr = q + (long long)qi * d;
    for (int c = g0; c < nchunks; ++c) {
        const long long slot = (long long)qi * nchunks + c;
        if (cnt[slot] <= KC) continue;  // block-uniform
        const long long r0 = (long long)c * L;
        const int len = (int)min((long long)L, n_db - r0);
        for (int g = w * 16; g < len; g += SEL_WAVES * 16) {  // 16 rows per wave step
            const bool row_ok = g + r16 < len;
            f32x4_knn_t acc = (f32x4_knn_t){0.f, 0.f, 0.f, 0.f};
            fixup_scores<T>(db + (r0 + g + (row_ok ? r16 : 0)) * d, row_ok, qr, r16 == 0, d, acc);
            if (r16 == 0) {  // D[row 4 kq + e][column 0]
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (g + 4 * kq + e < len)  // as the GEMM epilogue (-0 -> +0; int8: float of the exact int32)
                        keys[g + 4 * kq + e] = score_key(std::is_same<T, int8_t>::value
                                                             ? (float)__float_as_int(acc[e]) : acc[e] * 1.f + 0.f);
            }
        }
        __syncthreads();
        const uint32_t thr = block_topk([&](int i) { return keys[i]; }, [&](int i) { return (int)(r0 + i); }, len, KC,
                                        cand_k + slot * KC, cand_i + slot * KC, smi);
        if (threadIdx.x == 0) {
            cnt[slot] = KC;
            if (len > KC && thr > tau[qi]) atomicMax(tau + qi, thr);
        }
        __syncthreads();
    }
}

// float64 re-score from the float32 rows: exact products, a fixed per-lane
// order and a butterfly reduction -> bit-reproducible on any sharding.
__global__ void __launch_bounds__(256) k_rescore(const int* __restrict__ sel_i, int KC, int npow2,
                                                 const float* __restrict__ db32, const float* __restrict__ q32, int d,
                                                 double* __restrict__ fin_s, int* __restrict__ fin_i,
                                                 const uint32_t* __restrict__ sel_k, const float* __restrict__ prune_thr) {
    const int q = blockIdx.y, lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= npow2) return;
    const int idx = j < KC ? sel_i[(long long)q * KC + j] : -1;
    // a candidate below the certified cut (rescore_cut) cannot be in the top k: no row read
    const bool cut = prune_thr && idx >= 0 && funkey(sel_k[(long long)q * KC + j]) < prune_thr[q];
    double sc = -INFINITY;
    if (idx >= 0 && !cut) {
        const float* dr = db32 + (long long)idx * d;
        const float* qr = q32 + (long long)q * d;
        double acc = 0.0;
        if (d % 256 == 0) {
#pragma unroll 4
            for (int t = lane * 4; t < d; t += 256) {
                const float4 x = *reinterpret_cast<const float4*>(dr + t);
                const float4 y = *reinterpret_cast<const float4*>(qr + t);
                acc = fma((double)x.x, (double)y.x, acc);
                acc = fma((double)x.y, (double)y.y, acc);
                acc = fma((double)x.z, (double)y.z, acc);
                acc = fma((double)x.w, (double)y.w, acc);
            }
        } else {
            for (int t = lane; t < d; t += 64) acc = fma((double)dr[t], (double)qr[t], acc);
        }
        sc = wave_sum_d(acc);
    }
    if (lane == 0) {
        fin_s[(long long)q * npow2 + j] = sc;
        fin_i[(long long)q * npow2 + j] = idx >= 0 ? idx : 0x7fffffff;
    }
}

// Certificate of the screening margin (out_unc != nullptr): every row left
// out of the candidates has screening score <= funkey(thr) and hence exact
// score <= funkey(thr) + delta, delta = delta_scale * ||q|| (the screening
// error bound); if that is below the exact k-th score the top k are exact,
// else the query is flagged (dense clusters tighter than the screening error).
__global__ void __launch_bounds__(SEL_THREADS) k_final_sort(const double* __restrict__ fin_s,
                                                            const int* __restrict__ fin_i, int npow2, int k,
                                                            long long idx_offset, double* __restrict__ out_s,
                                                            long long* __restrict__ out_i,
                                                            const uint32_t* __restrict__ sel_thr,
                                                            const float* __restrict__ q32, int d, double delta_scale,
                                                            int* __restrict__ out_unc,
                                                            const float* __restrict__ i8_qamax, int i8_qstride,
                                                            const float* __restrict__ i8_dbamax) {
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    double* ks = reinterpret_cast<double*>(dyn);
    int* is = reinterpret_cast<int*>(ks + npow2);
    const int q = blockIdx.x;
    for (int j = threadIdx.x; j < npow2; j += SEL_THREADS) {
        ks[j] = fin_s[(long long)q * npow2 + j];
        is[j] = fin_i[(long long)q * npow2 + j];
    }
    __syncthreads();
    bitonic_best_first(ks, is, npow2);
    for (int j = threadIdx.x; j < k; j += SEL_THREADS) {
        const int i = is[j];
        out_s[(long long)q * k + j] = ks[j];
        out_i[(long long)q * k + j] = i == 0x7fffffff ? -1 : (long long)i + idx_offset;
    }
    if (out_unc) {
        __shared__ double red[SEL_WAVES];
        double ss = 0.0;
        for (int t = threadIdx.x; t < d; t += SEL_THREADS) ss += (double)q32[(long long)q * d + t] * q32[(long long)q * d + t];
        ss = wave_sum_d(ss);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
        __syncthreads();
        if (threadIdx.x == 0) {
            double tot = 0.0;
            for (int w = 0; w < SEL_WAVES; ++w) tot += red[w];
            const uint32_t thr = sel_thr[q];
            const bool full = k > npow2 || is[k - 1] == 0x7fffffff;  // fewer than k rows: all rows are in
            double bound;
            if (i8_dbamax) {
                // int8 keys are integer dot products I of q8 = rint(127 q / aq), x8 = rint(127 x / ax):
                // q.x - s I = s (q8.ex + eq.x8 + eq.ex), s = aq ax / 127^2, residuals |e| <= 1/2 per
                // element (amax scaling never clamps), so |q.x - s I| <= s E (||q8|| + ||x8|| + E) with
                // E = sqrt(d) / 2, ||q8|| <= 127 ||q|| / aq + E, ||x8|| <= 127 max||x|| / ax + E; the
                // f32 key adds |I| 2^-24
                const double aq = i8_qamax[(long long)q * i8_qstride], ax = *i8_dbamax;
                const double sc = aq * ax / (127.0 * 127.0);
                const double E = sqrt((double)d) * 0.50002;
                const double key = (double)funkey(thr);
                bound = sc * key + (ax / 127.0 * E * sqrt(tot) + aq / 127.0 * E * delta_scale + 3.0 * sc * E * E +
                                    sc * fabs(key) * 0x1p-23) * 1.001;
            } else {
                bound = (double)funkey(thr) + delta_scale * sqrt(tot);
            }
            const bool ok = thr == 0u || full || bound < ks[k - 1];
            out_unc[q] = ok ? 0 : 1;
        }
    }
}

// ------------------------------------------------------------------ merge
__global__ void __launch_bounds__(SEL_THREADS) k_merge(const double* __restrict__ in_s, const long long* __restrict__ in_i,
                                                       int r, int nq, int k_in, int k, int npow2,
                                                       double* __restrict__ out_s, long long* __restrict__ out_i) {
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    double* ks = reinterpret_cast<double*>(dyn);
    long long* is = reinterpret_cast<long long*>(ks + npow2);
    const long long SENT = 0x7fffffffffffffffll;
    const int q = blockIdx.x;
    const int n = r * k_in;
    for (int j = threadIdx.x; j < npow2; j += SEL_THREADS) {
        double sc = -INFINITY;
        long long id = SENT;
        if (j < n) {
            const int src = j / k_in, jj = j - src * k_in;
            const long long o = ((long long)src * nq + q) * k_in + jj;
            if (in_i[o] >= 0) { sc = in_s[o]; id = in_i[o]; }
        }
        ks[j] = sc;
        is[j] = id;
    }
    __syncthreads();
    bitonic_best_first(ks, is, npow2);
    for (int j = threadIdx.x; j < k; j += SEL_THREADS) {
        out_s[(long long)q * k + j] = ks[j];
        out_i[(long long)q * k + j] = is[j] == SENT ? -1 : is[j];
    }
}

static int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

struct KnnPlan {
    int L, nchunks, G, KC, npow2;
    long long S;
};

struct KnnWs {   // in layout order
    float* slab;
    uint32_t* cand_k;
    int* cand_i;
    uint32_t* sel_k;
    int* sel_i;
    double* fin_s;
    int* fin_i;
    uint32_t *tau, *sel_thr;
    float* prune_thr;
    int* cnt;
};

static int default_cand(int k, int dtype) {
    // screening error: bf16 ~5e-5, fp16 ~1e-5, int8 ~4e-4 (std on unit 2048-d rows; at 1M random rows
    // the true top 100 lie within the first 118 int8-ordered rows, 32 queries measured)
    int extra = dtype == RR_BF16 || dtype == RR_I8 ? 128 : dtype == RR_F16 ? 64 : 32;
    return ((k + extra + 63) / 64) * 64;
}

static KnnPlan plan(long long n_db, int nq, int k, int cand, int dtype) {
    KnnPlan p;
    p.KC = cand > 0 ? cand : default_cand(k, dtype);
    p.L = (int)(n_db < CHUNK_L ? n_db : CHUNK_L);
    p.nchunks = (int)((n_db + p.L - 1) / p.L);
    long long g = (long long)(slab_budget() / ((size_t)nq * p.L * 4));
    if (g < 1) g = 1;
    if (g > p.nchunks) g = p.nchunks;
    if (g * p.L > (4ll << 20)) g = (4ll << 20) / p.L;  // <= 4M rows per GEMM pass (grid.y limit)
    if (g < 1) g = 1;
    p.G = (int)g;
    p.S = ((long long)p.G * p.L + 3) / 4 * 4;
    p.npow2 = pow2_at_least(p.KC);
    return p;
}

static KnnWs layout(Arena& a, const KnnPlan& p, int nq) {
    const size_t q = (size_t)nq, cands = q * p.nchunks * p.KC, sel = q * p.KC, fin = q * p.npow2;
    return {a.take<float>(q * p.S), a.take<uint32_t>(cands), a.take<int>(cands), a.take<uint32_t>(sel), a.take<int>(sel),
            a.take<double>(fin), a.take<int>(fin), a.take<uint32_t>(q), a.take<uint32_t>(q), a.take<float>(q),
            a.take<int>(q * p.nchunks)};
}

}  // namespace rr

using namespace rr;

extern "C" {

size_t rr_knn_workspace_bytes(long long n_db, int nq, int d, int k, int cand, int dtype) {
    (void)d;
    if (n_db <= 0 || nq <= 0) return 0;
    return measured(layout, plan(n_db, nq, k, cand, dtype), nq);
}

static int knn_topk_impl(const void* db, const float* db_f32, long long n_db, const void* q, const float* q_f32,
                         int nq, int d, int k, int cand, long long idx_offset, double* out_scores, long long* out_idx,
                         void* workspace, size_t workspace_bytes, int dtype, float db_norm_max, int* out_uncertain,
                         const float* i8_qamax, int i8_qstride, const float* i8_dbamax, void* stream);

int rr_knn_topk(const void* db, const float* db_f32, long long n_db, const void* q, const float* q_f32, int nq, int d,
                int k, int cand, long long idx_offset, double* out_scores, long long* out_idx, void* workspace,
                size_t workspace_bytes, int dtype, void* stream) {
    return knn_topk_impl(db, db_f32, n_db, q, q_f32, nq, d, k, cand, idx_offset, out_scores, out_idx, workspace,
                         workspace_bytes, dtype, 1.0f, nullptr, nullptr, 0, nullptr, stream);
}

static int knn_topk_impl(const void* db, const float* db_f32, long long n_db, const void* q, const float* q_f32,
                         int nq, int d, int k, int cand, long long idx_offset, double* out_scores, long long* out_idx,
                         void* workspace, size_t workspace_bytes, int dtype, float db_norm_max, int* out_uncertain,
                         const float* i8_qamax, int i8_qstride, const float* i8_dbamax, void* stream) {
    if (n_db <= 0 || nq <= 0 || k <= 0) return fail(RR_EINVAL, "rr_knn_topk: empty problem");
    if (n_db > 0x7fffffffll) return fail(RR_EINVAL, "rr_knn_topk: shard rows must fit int32 (shard the database)");
    if (dtype != RR_BF16 && dtype != RR_F32 && dtype != RR_F16 && dtype != RR_I8)
        return fail(RR_EINVAL, "rr_knn_topk: dtype");
    if (dtype == RR_F16 && d < 64) return fail(RR_EINVAL, "rr_knn_topk: fp16 screening needs d >= 64");
    if (dtype == RR_I8 && (d < 128 || (nq > 128 && d < 256)))
        return fail(RR_EINVAL, "rr_knn_topk: int8 screening needs d >= 128 (d >= 256 above 128 queries)");
    if (d <= 0 || d % 32 || (d & (d - 1))) return fail(RR_EINVAL, "rr_knn_topk: d must be a power of two >= 32");
    KnnPlan p = plan(n_db, nq, k, cand, dtype);
    if (p.KC < k) return fail(RR_EINVAL, "rr_knn_topk: cand must be >= k");
    if (p.npow2 > MAX_SORT) return fail(RR_EINVAL, "rr_knn_topk: k / cand too large (max 8192)");
    Arena arena(workspace, workspace_bytes);
    const auto [slab, cand_k, cand_i, sel_k, sel_i, fin_s, fin_i, tau, sel_thr, prune_thr, cnt] = layout(arena, p, nq);
    if (!workspace || !arena.fits()) return fail(RR_ENOSPACE, "rr_knn_topk: workspace too small");
    hipStream_t s = as_stream(stream);
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)k_chunk_select, hipFuncAttributeMaxDynamicSharedMemorySize, CHUNK_L * 4);
        (void)hipFuncSetAttribute((const void*)k_slot_fixup<bf16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, CHUNK_L * 4);
        (void)hipFuncSetAttribute((const void*)k_slot_fixup<f16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, CHUNK_L * 4);
        (void)hipFuncSetAttribute((const void*)k_slot_fixup<float>, hipFuncAttributeMaxDynamicSharedMemorySize, CHUNK_L * 4);
        (void)hipFuncSetAttribute((const void*)k_slot_fixup<int8_t>, hipFuncAttributeMaxDynamicSharedMemorySize, CHUNK_L * 4);
        (void)hipFuncSetAttribute((const void*)k_final_sort, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        (void)hipFuncSetAttribute((const void*)k_merge, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        attr_done = true;
    }

    const size_t esz = dtype == RR_F32 ? 4 : dtype == RR_I8 ? 1 : 2;
    auto scores = [&](const ConvArgs& a) { return dtype == RR_I8 ? gemm_scores_i8(a, s) : (gemm_scores(a, dtype, s), RR_OK); };
    // Screening (default): the first PREFIX_CHUNKS chunks go through the score
    // slab + chunk select, which sets each query's running threshold tau; the
    // rest of the database is ONE score GEMM whose epilogue appends only the
    // scores >= tau to per-(query, chunk) slots (no slab write / read, no
    // select launch); overflowing slots are rebuilt by k_slot_fixup.
    // RR_KNN_FUSED=0: every chunk through the slab (the round-1 pipeline).
    // RR_KNN_PREFIX: prefix chunks (A/B knob; any count gives the same results -- tau is
    // a valid bound whatever the prefix, and overflowing slots are rebuilt)
    static const int prefix = getenv("RR_KNN_PREFIX") ? atoi(getenv("RR_KNN_PREFIX")) : PREFIX_CHUNKS;
    const int pre = prefix >= 1 ? prefix : PREFIX_CHUNKS;
    const bool fused = g_tune.knn_fused && p.nchunks > pre && (d * esz) % 128 == 0;
    const int g0 = fused ? pre : p.nchunks;
    const long long slab_rows = (long long)g0 * p.L < n_db ? (long long)g0 * p.L : n_db;
    // the running threshold is reset by a kernel (RR_KNN_TAU_MEMSET=1: by
    // hipMemsetAsync, kept to reproduce the graph-replay finding of DESIGN §4)
    static const bool tau_memset = getenv("RR_KNN_TAU_MEMSET") && getenv("RR_KNN_TAU_MEMSET")[0] == '1';
    if (tau_memset) (void)hipMemsetAsync(tau, 0, (size_t)nq * 4, s);
    const long long nreset = (long long)nq * p.nchunks > nq ? (long long)nq * p.nchunks : nq;
    hipLaunchKernelGGL(k_knn_reset, dim3((unsigned)((nreset + 255) / 256)), dim3(256), 0, s, tau, cnt, nq, p.nchunks, g0,
                       p.KC, tau_memset ? 0 : 1);
    auto score_args = [&, slab = slab](long long r0, int rows) {   // (C++17 lambdas capture no structured binding)
        ConvArgs a{};
        a.x = q;
        a.w = (const char*)db + (size_t)r0 * d * esz;
        a.y = slab;
        a.n = 1; a.h = 1; a.w_ = nq; a.cin = d; a.ho = 1; a.wo = nq; a.cout = rows;
        a.kh = 1; a.kw = 1; a.stride = 1; a.pad = 0; a.dil = 1; a.kp = d; a.ldy = (int)p.S;
        a.act = RR_ACT_IDENTITY; a.flags = 0; a.slope = 0.f;
        a.lc = __builtin_ctz((unsigned)d);
        a.P = nq;
        return a;
    };
    for (long long r0 = 0; r0 < slab_rows; r0 += (long long)p.G * p.L) {
        const int rows = (int)((slab_rows - r0) < (long long)p.G * p.L ? (slab_rows - r0) : (long long)p.G * p.L);
        if (int rc = scores(score_args(r0, rows))) return rc;
        const int chunks = (rows + p.L - 1) / p.L;
        hipLaunchKernelGGL(k_chunk_select, dim3(nq, chunks), dim3(SEL_THREADS), (size_t)p.L * 4, s, slab, p.S, p.L,
                           rows, (int)r0, (int)(r0 / p.L), p.nchunks, p.KC, cand_k, cand_i, tau);
    }
    if (fused) {
        hipLaunchKernelGGL(k_tau_refine, dim3(nq), dim3(SEL_THREADS), 0, s, cand_k, p.nchunks, g0, p.KC, tau);
        ConvArgs a = score_args(slab_rows, (int)(n_db - slab_rows));
        a.scr_tau = tau; a.scr_cnt = cnt; a.scr_k = cand_k; a.scr_i = cand_i;
        a.scr_L = p.L; a.scr_nchunks = p.nchunks; a.scr_KC = p.KC; a.scr_row0 = (int)slab_rows;
        if (int rc = scores(a)) return rc;
        const dim3 g(nq), b(SEL_THREADS);
        const size_t lds = (size_t)p.L * 4;
        if (dtype == RR_BF16)
            hipLaunchKernelGGL(k_slot_fixup<bf16_t>, g, b, lds, s, (const bf16_t*)db, n_db, (const bf16_t*)q, d, p.L,
                               p.nchunks, g0, p.KC, cnt, cand_k, cand_i, tau);
        else if (dtype == RR_F16)
            hipLaunchKernelGGL(k_slot_fixup<f16_t>, g, b, lds, s, (const f16_t*)db, n_db, (const f16_t*)q, d, p.L,
                               p.nchunks, g0, p.KC, cnt, cand_k, cand_i, tau);
        else if (dtype == RR_I8)
            hipLaunchKernelGGL(k_slot_fixup<int8_t>, g, b, lds, s, (const int8_t*)db, n_db, (const int8_t*)q, d, p.L,
                               p.nchunks, g0, p.KC, cnt, cand_k, cand_i, tau);
        else
            hipLaunchKernelGGL(k_slot_fixup<float>, g, b, lds, s, (const float*)db, n_db, (const float*)q, d, p.L,
                               p.nchunks, g0, p.KC, cnt, cand_k, cand_i, tau);
    }
    const size_t fin_lds = (size_t)p.npow2 * 12;
    if (fin_lds > 160 * 1024 - 4096) return fail(RR_EINVAL, "rr_knn_topk: candidate set exceeds LDS");
    // screening error bound per unit ||q|| ||x||: input rounding of both
    // operands (bf16 2^-9, fp16 2^-11 relative each; products exact in f32)
    // plus f32 accumulation over d terms (d 2^-24)
    // int8 scores are integer dot products: certified only through rr_knn_topk_checked_i8,
    // which passes the quantisation scales (without them every query with more than k rows is flagged)
    const double in_eps = dtype == RR_BF16 ? 0x1p-8 + 0x1p-17 : dtype == RR_F16 ? 0x1p-10 + 0x1p-21 : 0.0;
    // (int8 with its scales: k_final_sort's own bound, delta_scale = max ||x||; without them: no certificate)
    const bool i8_cert = dtype == RR_I8 && i8_qamax && i8_dbamax;
    const double nm = db_norm_max > 0.f ? (double)db_norm_max : 1.0;
    const double delta_scale = dtype == RR_I8 ? (i8_cert ? nm : (double)INFINITY) : (in_eps + d * 0x1p-24) * 1.001 * nm;
    // the certified re-score cut (16/32-bit screens, whose keys are scores): only with a
    // known database norm bound (the checked entry points), RR_KNN_CUT=0 disables it (A/B)
    static const int cut_env = getenv("RR_KNN_CUT") && getenv("RR_KNN_CUT")[0] == '0' ? 0 : 1;
    float* const prune = cut_env && dtype != RR_I8 && out_uncertain && k < p.KC ? prune_thr : nullptr;
    // RR_KNN_FSEL=0: the unstaged final select (A/B)
    static const int fsel = getenv("RR_KNN_FSEL") ? atoi(getenv("RR_KNN_FSEL")) : 1;
    const int stage = fsel && p.nchunks <= FSEL_MAXCH;
    hipLaunchKernelGGL(k_final_select, dim3(nq), dim3(SEL_THREADS), stage ? FSEL_LDS : 0, s, cand_k, cand_i, cnt,
                       p.nchunks, p.KC, sel_k, sel_i, sel_thr, stage, k, q_f32, d, delta_scale, prune);
    hipLaunchKernelGGL(k_rescore, dim3((p.npow2 + 3) / 4, nq), dim3(256), 0, s, sel_i, p.KC, p.npow2, db_f32, q_f32, d,
                       fin_s, fin_i, sel_k, (const float*)prune);
    hipLaunchKernelGGL(k_final_sort, dim3(nq), dim3(SEL_THREADS), fin_lds, s, fin_s, fin_i, p.npow2, k, idx_offset,
                       out_scores, out_idx, sel_thr, q_f32, d, delta_scale, out_uncertain, i8_cert ? i8_qamax : nullptr,
                       i8_qstride, i8_cert ? i8_dbamax : nullptr);
    return check_launch("rr_knn_topk");
}

int rr_knn_topk_checked(const void* db, const float* db_f32, long long n_db, const void* q, const float* q_f32, int nq,
                        int d, int k, int cand, long long idx_offset, double* out_scores, long long* out_idx,
                        void* workspace, size_t workspace_bytes, int dtype, float db_norm_max, int* out_uncertain,
                        void* stream) {
    return knn_topk_impl(db, db_f32, n_db, q, q_f32, nq, d, k, cand, idx_offset, out_scores, out_idx, workspace,
                         workspace_bytes, dtype, db_norm_max, out_uncertain, nullptr, 0, nullptr, stream);
}

int rr_knn_topk_checked_i8(const void* db, const float* db_f32, long long n_db, const void* q, const float* q_f32,
                           int nq, int d, int k, int cand, long long idx_offset, double* out_scores, long long* out_idx,
                           void* workspace, size_t workspace_bytes, float db_norm_max, const float* q_amax,
                           int q_amax_per_row, const float* db_amax, int* out_uncertain, void* stream) {
    if (!q_amax || !db_amax || !out_uncertain) return fail(RR_EINVAL, "rr_knn_topk_checked_i8: null scale / flags");
    return knn_topk_impl(db, db_f32, n_db, q, q_f32, nq, d, k, cand, idx_offset, out_scores, out_idx, workspace,
                         workspace_bytes, RR_I8, db_norm_max, out_uncertain, q_amax, q_amax_per_row ? 1 : 0, db_amax,
                         stream);
}

int rr_topk_merge(const double* in_scores, const long long* in_idx, int r, int nq, int k_in, int k, double* out_scores,
                  long long* out_idx, void* stream) {
    if (r <= 0 || nq <= 0 || k_in <= 0 || k <= 0) return fail(RR_EINVAL, "rr_topk_merge: empty");
    const int n = r * k_in;
    const int np2 = pow2_at_least(n < k ? k : n);
    if (np2 > MAX_SORT) return fail(RR_EINVAL, "rr_topk_merge: r*k_in too large");
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)k_merge, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
        attr_done = true;
    }
    hipLaunchKernelGGL(k_merge, dim3(nq), dim3(SEL_THREADS), (size_t)np2 * 16, as_stream(stream),
                       in_scores, in_idx, r, nq, k_in, k, np2, out_scores, out_idx);
    return check_launch("rr_topk_merge");
}

}  // extern "C"
