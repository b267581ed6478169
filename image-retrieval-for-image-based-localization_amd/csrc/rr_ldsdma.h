// librr.so — the LDS-DMA issue sequence and the small device helpers around it, shared by the
// conv and GEMM kernels (rr_gemm / rr_conv3 / rr_conv3s / rr_c3pair / rr_stream; rr_conv and
// rr_stem take the types).  Include after rr_internal.h.  tools/dma_audit.py audits the compiled
// result of dma16 + make_rsrc in every object; this is their only source.
#pragma once

#include "rr_internal.h"

namespace rr {

// the 4-float MFMA accumulator (H16<T>::mfma's type, rr_internal.h) and the 4-dword descriptor
typedef h16_f32x4_t f32x4_t;
typedef __attribute__((ext_vector_type(4))) int i32x4_t;

constexpr unsigned OOB = 0x80000000u;  // voffset beyond every buffer: the DMA writes zeros

// One 16-B-per-lane LDS-DMA wave-instruction: LDS[lds_addr + lane*16] = buf[voff].
// Issued from inline asm so hipcc neither counts it nor inserts a blanket
// vmcnt(0) before later ds_reads (which it does for compiler-visible LDS-DMA):
// completion is tracked by the explicit vm_wait<N>() below.  M0 is saved/restored.
__device__ __forceinline__ void dma16(i32x4_t rsrc, unsigned voff, unsigned lds_addr) {
    unsigned keep;
    lds_addr = __builtin_amdgcn_readfirstlane(lds_addr);  // wave-uniform by construction; make it provable
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"  // M0 write -> LDS-DMA: 1 wait state (descriptor: fenced in make_rsrc)
        "buffer_load_dwordx4 %1, %2, 0 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(rsrc), "s"(lds_addr)
        : "memory");
}

// Buffer descriptor of [base, base + bytes): reads past the end return zeros.
__device__ __forceinline__ i32x4_t make_rsrc(const void* base, unsigned bytes) {
    const unsigned long long b = (unsigned long long)base;
    i32x4_t r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)b);
    r.y = __builtin_amdgcn_readfirstlane((int)((unsigned)(b >> 32) & 0xFFFFu));
    r.z = __builtin_amdgcn_readfirstlane((int)bytes);
    r.w = 0x00020000;
    // VALU (readfirstlane) SGPR write -> LDS-DMA descriptor read: 5 wait states, tied to the
    // registers so no use of the descriptor is scheduled above it (tools/dma_audit.py checks)
    int x = r.x, y = r.y, z = r.z;
    asm volatile("s_nop 4" : "+s"(x), "+s"(y), "+s"(z));
    r.x = x;
    r.y = y;
    r.z = z;
    return r;
}

// Counted waits for the DMA (and the stores / loads in flight with it), and the raw barriers
// that go with them (never __syncthreads(), whose fence would drain the prefetch).
template <int N>
__device__ __forceinline__ void vm_wait() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void vm_wait_barrier() {
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"i"(N) : "memory");
}
// vmcnt(n) + barrier for a wave-uniform runtime n <= N (a chain of scalar
// compares picks the exact immediate).
template <int N>
__device__ __forceinline__ void vm_wait_barrier_n(int n) {
    if constexpr (N == 0) {
        vm_wait_barrier<0>();
    } else {
        if (n >= N) vm_wait_barrier<N>();
        else vm_wait_barrier_n<N - 1>(n);
    }
}
// data that reached the LDS by ds_write (not DMA): the writes must be done before the barrier
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void raw_barrier() { asm volatile("s_barrier" ::: "memory"); }

// A value loaded once before a loop (weights kept in VGPRs): passing it through an
// empty asm makes the asm its producer, so the compiler's wait for the load sits
// before the loop instead of (counted against the loop's own LDS-DMA / stores,
// which it cannot see) in front of every use inside it.
__device__ __forceinline__ void pin_loaded(uint4& v) {
    asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
}

// elements of T per 16-B chunk
template <typename T> struct Vec;
template <> struct Vec<bf16_t> { static constexpr int N = 8; };
template <> struct Vec<f16_t> { static constexpr int N = 8; };
template <> struct Vec<float> { static constexpr int N = 4; };

// 4 consecutive output values: float <-> TO, one vector access
template <typename TO> struct St4;
template <> struct St4<float> {
    static __device__ __forceinline__ void st(float* p, const float* v) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    }
    static __device__ __forceinline__ void ld(const float* p, float* v) {
        float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
};
template <> struct St4<bf16_t> {
    static __device__ __forceinline__ void st(bf16_t* p, const float* v) {
        ushort4 o;
        o.x = f2bf(v[0]); o.y = f2bf(v[1]); o.z = f2bf(v[2]); o.w = f2bf(v[3]);
        *reinterpret_cast<ushort4*>(p) = o;
    }
    static __device__ __forceinline__ void ld(const bf16_t* p, float* v) {
        ushort4 t = *reinterpret_cast<const ushort4*>(p);
        v[0] = bf2f(t.x); v[1] = bf2f(t.y); v[2] = bf2f(t.z); v[3] = bf2f(t.w);
    }
};
template <> struct St4<f16_t> {
    static __device__ __forceinline__ void st(f16_t* p, const float* v) {
        typedef __attribute__((ext_vector_type(4))) _Float16 h4;
        *reinterpret_cast<h4*>(p) = (h4){(f16_t)v[0], (f16_t)v[1], (f16_t)v[2], (f16_t)v[3]};
    }
    static __device__ __forceinline__ void ld(const f16_t* p, float* v) {
        typedef __attribute__((ext_vector_type(4))) _Float16 h4;
        const h4 t = *reinterpret_cast<const h4*>(p);
        v[0] = (float)t.x; v[1] = (float)t.y; v[2] = (float)t.z; v[3] = (float)t.w;
    }
};

}  // namespace rr
