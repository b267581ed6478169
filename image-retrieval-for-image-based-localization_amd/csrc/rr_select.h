// The best `num` of a list of unique 64-bit keys, sorted descending, by one block of D_SEL_TB threads:
// shared by k_select (rr_detect.hip) and k_ss_select (rr_scalespace.hip), with the reset of the
// per-image candidate counters that both run first.
#pragma once

#include "rr_internal.h"

namespace rr {

constexpr int D_SEL_TB = 1024;     // threads of a selecting block
constexpr int D_MAXNUM = 8192;     // keypoints per image (64 KiB of keys in LDS)

__device__ __forceinline__ float key_score(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

static __global__ void __launch_bounds__(256) k_reset_counts(int* __restrict__ cnt, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) cnt[i] = 0;
}

struct SelLds {
    unsigned long long sel[D_MAXNUM];
    unsigned int hist[256];
    unsigned long long prefix;
    int remaining;
    int equal;      // keys that share the threshold's bits so far
    int nsel;
};

// A radix select, 8 bits a pass from the top (it stops at the first pass after which every key
// sharing the settled bits is wanted), finds the num-th largest of the m keys kb; the keys at or
// above it are gathered into L.sel and sorted by a bitonic network, descending.  Returns
// want = min(m, num); every thread of the block must call it.
__device__ __forceinline__ int select_sorted(SelLds& L, const unsigned long long* __restrict__ kb, long long m, int num) {
    const int tid = threadIdx.x;
    const int want = (int)(m < num ? m : num);
    unsigned long long thr = 0ull;
    if (m > num) {   // the num-th largest key, 8 bits at a time from the top
        unsigned long long mask = 0ull;
        if (tid == 0) { L.prefix = 0ull; L.remaining = num; }
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (tid < 256) L.hist[tid] = 0u;
            __syncthreads();
            const unsigned long long pre = L.prefix;
            for (long long i0 = tid; i0 < m; i0 += 4 * D_SEL_TB) {   // four loads in flight per thread
                unsigned long long k[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) k[u] = i0 + u * D_SEL_TB < m ? kb[i0 + u * D_SEL_TB] : 0ull;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (i0 + u * D_SEL_TB < m && (k[u] & mask) == pre) atomicAdd(&L.hist[(unsigned)(k[u] >> shift) & 255u], 1u);
            }
            __syncthreads();
            // the digit: bin d with fewer than `remaining` keys above it and at least that many from it on
            int rem = 0;
            unsigned above = 0u, mine = 0u;
            if (tid < 256) {
                rem = L.remaining;
                for (int j = tid + 1; j < 256; ++j) above += L.hist[j];
                mine = L.hist[tid];
            }
            __syncthreads();   // every thread has read remaining (and prefix)
            if (tid < 256 && (int)above < rem && (int)(above + mine) >= rem) {
                L.remaining = rem - (int)above;
                L.equal = (int)mine;
                L.prefix = pre | ((unsigned long long)tid << shift);
            }
            mask |= 0xffull << shift;
            __syncthreads();
            // every key that shares the bits settled so far is wanted: the bits below need no pass
            if (L.equal == L.remaining) break;
        }
        thr = L.prefix;
    }
    if (tid == 0) L.nsel = 0;
    __syncthreads();
    for (long long i = tid; i < m; i += D_SEL_TB) {
        const unsigned long long k = kb[i];
        if (k >= thr) {
            const int pos = atomicAdd(&L.nsel, 1);
            if (pos < D_MAXNUM) L.sel[pos] = k;   // always: exactly `want` keys reach thr
        }
    }
    int P = 1;
    while (P < want) P <<= 1;
    __syncthreads();
    for (int i = want + tid; i < P; i += D_SEL_TB) L.sel[i] = 0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += D_SEL_TB) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = L.sel[i], c = L.sel[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? a < c : a > c) { L.sel[i] = c; L.sel[l] = a; }
                }
            }
            __syncthreads();
        }
    }
    return want;
}

}  // namespace rr
