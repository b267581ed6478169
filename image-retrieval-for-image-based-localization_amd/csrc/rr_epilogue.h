// librr.so — what follows the MFMAs, shared by the conv and GEMM kernels (rr_gemm / rr_stream /
// rr_c3pair / rr_conv3 / rr_conv3s / rr_stem; rr_conv takes the zeroing and the activation): the
// folded-BN, residual, activation and pack steps of the PERM32 fused epilogue on a float v[8], and
// the accumulator zeroing.  Include after rr_ldsdma.h.  Every helper is the text the kernels wrote
// out, term for term, and nearly all are macros: a forced-inline function is optimised on its own
// before it is inlined, and the kernels then no longer compile to the instructions they had
// (tools/isa_diff.py).
#pragma once

#include "rr_ldsdma.h"

namespace rr {

// ---- accumulators
// zero an f32x4_t accumulator array: RR_ZERO(rank, acc), the nested unrolled loops over acc's
// extents.  A macro: handing the array to a function, even a forced-inline one, changes the code
// the kernels compile to (tools/isa_diff.py), and so does one flat loop over all its elements.
#define RR_EXTENT_(a) ((int)(sizeof(a) / sizeof((a)[0])))
#define RR_FOR_(i, a) _Pragma("unroll") for (int i = 0; i < RR_EXTENT_(a); ++i)
#define RR_ZERO_VALUE_ (::rr::f32x4_t){0.f, 0.f, 0.f, 0.f}
#define RR_ZERO_1(a) RR_FOR_(i_, a) (a)[i_] = RR_ZERO_VALUE_
#define RR_ZERO_2(a) RR_FOR_(i_, a) RR_FOR_(j_, (a)[0]) (a)[i_][j_] = RR_ZERO_VALUE_
#define RR_ZERO_3(a) RR_FOR_(i_, a) RR_FOR_(j_, (a)[0]) RR_FOR_(k_, (a)[0][0]) (a)[i_][j_][k_] = RR_ZERO_VALUE_
#define RR_ZERO_4(a) \
    RR_FOR_(i_, a) RR_FOR_(j_, (a)[0]) RR_FOR_(k_, (a)[0][0]) RR_FOR_(l_, (a)[0][0][0])(a)[i_][j_][k_][l_] = RR_ZERO_VALUE_
#define RR_ZERO(rank, a) RR_ZERO_##rank(a)

// ---- 8 consecutive channels: a PERM32 fragment pair (2 i2, 2 i2 + 1) of one pixel, as float v[8].
// Macros like RR_ZERO, and for its reason: as forced-inline functions on v, the pack and the BN
// fold each changed 40-odd of rr_stream's 58 kernels, the activation 4 and the residual add 7.
// folded BN: v = (lo | hi) * sc + sh; lo / hi: two accumulators or float[4] rows; sc / sh: 8 floats
// in registers, or a pointer into LDS or global memory
#define RR_BN_PAIR(lo, hi, sc, sh, v)                              \
    do {                                                           \
        _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) {         \
            (v)[r_] = (lo)[r_] * (sc)[r_] + (sh)[r_];              \
            (v)[4 + r_] = (hi)[r_] * (sc)[4 + r_] + (sh)[4 + r_];  \
        }                                                          \
    } while (0)
// leaky activation of v[0 .. N); the caller keeps its `if (leaky)`
#define RR_LEAKY(N, v, slope)                                                                                  \
    do {                                                                                                       \
        _Pragma("unroll") for (int r_ = 0; r_ < (N); ++r_) (v)[r_] = (v)[r_] > 0.f ? (v)[r_] : (v)[r_] * (slope); \
    } while (0)
// v += rv
#define RR_ADD8(v, rv)                                                       \
    do {                                                                     \
        _Pragma("unroll") for (int r_ = 0; r_ < 8; ++r_) (v)[r_] += (rv)[r_]; \
    } while (0)
// q (uint4) = v packed to 8 values of the 16-bit type H
#define RR_PACK8(H, q, v)                           \
    do {                                            \
        (q).x = H16<H>::pack2((v)[0], (v)[1]);      \
        (q).y = H16<H>::pack2((v)[2], (v)[3]);      \
        (q).z = H16<H>::pack2((v)[4], (v)[5]);      \
        (q).w = H16<H>::pack2((v)[6], (v)[7]);      \
    } while (0)
// rv = the 8 values of H packed in q (a residual prefetched as 16 B) ...
#define RR_UNPACK8(H, q, rv)                                         \
    do {                                                             \
        const unsigned w4_[4] = {(q).x, (q).y, (q).z, (q).w};        \
        _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) {           \
            (rv)[2 * r_] = H16<H>::lo(w4_[r_]);                      \
            (rv)[2 * r_ + 1] = H16<H>::hi(w4_[r_]);                  \
        }                                                            \
    } while (0)
// ... or v += them
#define RR_ADD_PACKED8(H, q, v)                                      \
    do {                                                             \
        const unsigned w4_[4] = {(q).x, (q).y, (q).z, (q).w};        \
        _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) {           \
            (v)[2 * r_] += H16<H>::lo(w4_[r_]);                      \
            (v)[2 * r_ + 1] += H16<H>::hi(w4_[r_]);                  \
        }                                                            \
    } while (0)
// 8 values of TO at p (scale / shift of 8 channels, a residual): two St4 loads.  A function: the
// loads only fill a fresh array, and the kernels that use it compile as before.
template <typename TO>
__device__ __forceinline__ void ld8(const TO* p, float* v) {
    St4<TO>::ld(p, v);
    St4<TO>::ld(p + 4, v + 4);
}

}  // namespace rr
