// librr.so — learned patch descriptors (gfx950): HardNet and SOSNet of cirtorch/features/hardnet.py
// and cirtorch/features/sosnet.py in eval mode.  One launch runs the normalisation and layers 1-6 of a
// patch with every activation in LDS (k_patchnet_trunk, one workgroup per patch), a second one the
// 8 x 8 convolution of layer 7 as a GEMM over the patches of a chunk with its BatchNorm and the
// descriptor normalisation (k_patchnet_head).  fp16 operands, float32 accumulation on
// v_mfma_f32_16x16x32_f16; the semantics and every rounding point are stated in rr.h.
#include "rr_internal.h"
#include "rr_workspace.h"

namespace rr {

namespace {

typedef H16<f16_t> HF;

constexpr int PN_LAYERS = 7;
constexpr int pn_cin(int l) { return l == 0 ? 1 : l < 3 ? 32 : l < 5 ? 64 : 128; }
constexpr int pn_cout(int l) { return l < 2 ? 32 : l < 4 ? 64 : 128; }
constexpr int pn_taps(int l) { return l < 6 ? 9 : 64; }
constexpr int PN_MAP = 8 * 8 * 128;   // fp16 values of one patch's layer-6 map

// The packed blob: the fp16 weights of layers 1..7 one after the other, then float32 scale[576] and
// shift[576] (the channels of layers 1..7 in order).  Layer 1 is [tap][cout]; layers 2..7 are
// [K-step][cout][32] with K-step = tap * (cin / 32) + cin / 32 chunk: one MFMA K-step is 32 input
// channels of one tap, and the 16 B a lane loads for its B fragment are contiguous.
constexpr size_t pn_w_count(int l) { return (size_t)pn_taps(l) * pn_cin(l) * pn_cout(l); }
constexpr size_t pn_w_off(int l) {
    size_t o = 0;
    for (int i = 0; i < l; ++i) o += pn_w_count(i);
    return o;
}
constexpr int pn_c_off(int l) {
    int o = 0;
    for (int i = 0; i < l; ++i) o += pn_cout(i);
    return o;
}
constexpr int PN_CHANNELS = pn_c_off(PN_LAYERS);                        // 576
constexpr size_t PN_W_TOTAL = pn_w_off(PN_LAYERS);                   // 1,334,560
constexpr size_t PN_BN_OFF = (PN_W_TOTAL * 2 + 255) / 256 * 256;                                     // bytes
constexpr size_t PN_PACKED_BYTES = PN_BN_OFF + 2 * PN_CHANNELS * sizeof(float);
static_assert(PN_CHANNELS == 576 && PN_W_TOTAL == 1334560 && pn_w_off(1) % 8 == 0 && pn_w_off(6) % 8 == 0, "16-byte aligned layer blocks");

// --------------------------------------------------------------------------------------------- pack
struct PackArgs {
    const float* w[PN_LAYERS];
    const float* mean[PN_LAYERS];
    const float* var[PN_LAYERS];
};

// dst element i of layer l <- w[cout][cin][ky][kx] (row-major float32), rounded once to fp16
__global__ void __launch_bounds__(256) k_patchnet_pack(PackArgs a, f16_t* __restrict__ wp, float* __restrict__ bn) {
    const int l = blockIdx.y;
    const int cin = pn_cin(l), cout = pn_cout(l), taps = pn_taps(l);
    const size_t count = (size_t)taps * cin * cout;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        int tap, co, ci;
        if (l == 0) {
            tap = (int)(i / cout);
            co = (int)(i % cout);
            ci = 0;
        } else {
            const int ncc = cin / 32;
            const int ks = (int)(i / ((size_t)cout * 32));
            co = (int)(i / 32 % cout);
            tap = ks / ncc;
            ci = (ks % ncc) * 32 + (int)(i % 32);
        }
        wp[pn_w_off(l) + i] = (f16_t)a.w[l][((size_t)co * cin + ci) * taps + tap];
    }
    if (blockIdx.x == 0) {
        for (int c = threadIdx.x; c < cout; c += 256) {
            const double s = 1.0 / sqrt((double)a.var[l][c] + 1e-5);
            bn[pn_c_off(l) + c] = (float)s;
            bn[PN_CHANNELS + pn_c_off(l) + c] = (float)(-(double)a.mean[l][c] * s);
        }
    }
}

// -------------------------------------------------------------------------------------------- trunk
constexpr int T_TB = 512;                       // 8 waves: every MFMA layer is 8 jobs, one per wave
constexpr int T_MAP_BYTES = 34 * 34 * 32 * 2;   // a zero-padded 34 x 34 x 32 fp16 map: 73,984 B
constexpr int T_LDS_BYTES = 2 * T_MAP_BYTES + 64;   // both maps of layer 2, and 8 doubles of the reduction
static_assert(18 * 18 * 64 * 2 <= T_MAP_BYTES && 10 * 10 * 128 * 2 <= T_MAP_BYTES, "later maps reuse the two regions");

__device__ __forceinline__ void lds_zero(unsigned char* p, int bytes) {
    for (int i = threadIdx.x * 16; i < bytes; i += T_TB * 16) *reinterpret_cast<uint4*>(p + i) = make_uint4(0, 0, 0, 0);
}

// One 3 x 3 layer as an implicit GEMM on the maps in LDS: M = WO x WO pixels in tiles of 16 (a tile is
// 16 consecutive pixels of the row-major output), N = COUT in tiles of 16, K = 9 taps x CIN / 32 steps
// in (tap, chunk) order.  A job is MB pixel tiles x one channel tile; (WO * WO / 16 / MB) * (COUT / 16)
// is 8 for every layer, one job per wave.  in: zero-padded [(WO * S + 2)][(WO * S + 2)][CIN] fp16.
// out: zero-padded [(WO + 2)][(WO + 2)][COUT] fp16 in LDS, or the [WO][WO][COUT] map in memory (TO_MEM),
// which is NaN in every entry when `bad` (a non-finite patch).
template <int CIN, int COUT, int WO, int S, int MB, bool TO_MEM>
__device__ __forceinline__ void conv3_layer(const unsigned char* in, unsigned char* out, f16_t* gout,
                                            const f16_t* __restrict__ w, const float* __restrict__ scale,
                                            const float* __restrict__ shift, bool bad = false) {
    constexpr int WP = WO * S + 2, NCC = CIN / 32, NT = COUT / 16, MT = WO * WO / 16;
    static_assert(MT % MB == 0 && (MT / MB) * NT == T_TB / 64, "one job per wave");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int nt = wave % NT, mblk = wave / NT;
    int abase[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int p = (mblk * MB + mb) * 16 + fr;
        abase[mb] = (((p / WO) * S) * WP + (p % WO) * S) * CIN * 2 + fq * 16;
    }
    const f16_t* wl = w + (size_t)(nt * 16 + fr) * 32 + fq * 8;
    h16_f32x4_t acc[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[mb] = (h16_f32x4_t){0.f, 0.f, 0.f, 0.f};
    // the weights of tap t + 1 are requested before the MFMAs of tap t are issued
    uint4 b[NCC], bn[NCC];
#pragma unroll
    for (int cc = 0; cc < NCC; ++cc) b[cc] = *reinterpret_cast<const uint4*>(wl + (size_t)cc * COUT * 32);
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const int nx = tap < 8 ? tap + 1 : 8;
#pragma unroll
        for (int cc = 0; cc < NCC; ++cc) bn[cc] = *reinterpret_cast<const uint4*>(wl + (size_t)(nx * NCC + cc) * COUT * 32);
        const int ky = tap / 3, kx = tap - 3 * ky;
        const int toff = (ky * WP + kx) * CIN * 2;
#pragma unroll
        for (int cc = 0; cc < NCC; ++cc) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const uint4 a = *reinterpret_cast<const uint4*>(in + abase[mb] + toff + cc * 64);
                acc[mb] = HF::mfma(a, b[cc], acc[mb]);
            }
        }
#pragma unroll
        for (int cc = 0; cc < NCC; ++cc) b[cc] = bn[cc];
    }
    // D: column (channel) = lane & 15, row (pixel of the tile) = 4 (lane >> 4) + r
    const int c = nt * 16 + fr;
    const float sc = scale[c], sh = shift[c];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = (mblk * MB + mb) * 16 + fq * 4 + r;
            const f16_t v = (f16_t)fmaxf(fmaf(acc[mb][r], sc, sh), 0.f);
            if (TO_MEM)
                gout[p * COUT + c] = bad ? (f16_t)__builtin_nanf("") : v;
            else
                reinterpret_cast<f16_t*>(out)[((p / WO + 1) * (WO + 2) + p % WO + 1) * COUT + c] = v;
        }
    }
}

__global__ void __launch_bounds__(T_TB) k_patchnet_trunk(const float* __restrict__ patches, long long B, int variant,
                                                         const f16_t* __restrict__ wp, const float* __restrict__ bn,
                                                         f16_t* __restrict__ maps) {
    __shared__ __attribute__((aligned(16))) unsigned char t_lds[T_LDS_BYTES];   // one block per CU
    unsigned char* const ra = t_lds;                  // layer 1, 3, 5 outputs
    unsigned char* const rb = t_lds + T_MAP_BYTES;    // the normalised patch, layer 2, 4 outputs
    double* const red = reinterpret_cast<double*>(t_lds + 2 * T_MAP_BYTES);
    const float* scale = bn;
    const float* shift = bn + PN_CHANNELS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long patch = blockIdx.x; patch < B; patch += gridDim.x) {
        __syncthreads();   // the previous patch's layer 6 has read region a
        // ---- patch statistics, float64 in a fixed order: thread t sums pixels 2t, 2t + 1, a wave by the
        // xor butterfly (offsets 32 .. 1), the 8 wave sums in ascending order
        const float2 xv = *reinterpret_cast<const float2*>(patches + patch * 1024 + 2 * tid);
        double s = wave_sum_d((double)xv.x + (double)xv.y);
        if (lane == 0) red[wave] = s;
        lds_zero(ra, T_MAP_BYTES);
        lds_zero(rb, 34 * 34 * 2 + 8);   // 2,312 B rounded up to 16
        __syncthreads();
        s = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += red[i];
        // A NaN or an infinite pixel makes this sum non-finite (1024 finite floats cannot), and then every
        // normalised pixel is NaN.  fmaxf in the ReLUs below would turn that into zeros and give the patch
        // the descriptor of the BatchNorm shifts, so the patch gets its all-NaN map here (rr.h).  s is the
        // same in every thread: the whole block takes the branch.
        // A NaN or an infinite pixel makes this sum non-finite (1024 finite floats cannot), and then every
        // normalised pixel is NaN.  fmaxf in the ReLUs below turns that into zeros, which would give the
        // patch the descriptor of the BatchNorm shifts; layer 6 stores NaN instead (rr.h).  The same in
        // every thread, and no control flow depends on it.
        const bool bad = !isfinite(s);
        const double mean = s / 1024.0;
        const double d0 = (double)xv.x - mean, d1 = (double)xv.y - mean;
        __syncthreads();   // every thread has read red
        double q = wave_sum_d(d0 * d0 + d1 * d1);
        if (lane == 0) red[wave] = q;
        __syncthreads();
        q = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) q += red[i];
        const double den = variant == RR_PATCHNET_HARDNET ? sqrt(q / 1023.0) + 1e-6 : sqrt(q / 1024.0 + 1e-5);
        {
            const int y = (2 * tid) >> 5, x = (2 * tid) & 31;
            f16_t* pin = reinterpret_cast<f16_t*>(rb) + (y + 1) * 34 + x + 1;
            pin[0] = (f16_t)(d0 / den);   // one rounding, float64 -> fp16
            pin[1] = (f16_t)(d1 / den);
        }
        __syncthreads();
        // ---- layer 1 (K = 9): vector work, two pixels per thread, taps in ascending order
        {
            const f16_t* pin = reinterpret_cast<const f16_t*>(rb);
#pragma unroll 1
            for (int h = 0; h < 2; ++h) {
                const int p = tid + h * T_TB, y = p >> 5, x = p & 31;
                float xin[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) xin[t] = (float)pin[(y + t / 3) * 34 + x + t % 3];
                uint4* dst = reinterpret_cast<uint4*>(ra + ((y + 1) * 34 + x + 1) * 64);
#pragma unroll 1
                for (int k = 0; k < 4; ++k) {   // 8 channels, one 16-byte store
                    uint32_t o[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int c = 8 * k + 2 * j;
                        float a0 = 0.f, a1 = 0.f;
#pragma unroll
                        for (int t = 0; t < 9; ++t) {
                            const uint32_t wv = *reinterpret_cast<const uint32_t*>(wp + t * 32 + c);
                            a0 = fmaf(xin[t], HF::lo(wv), a0);
                            a1 = fmaf(xin[t], HF::hi(wv), a1);
                        }
                        o[j] = HF::pack2(fmaxf(fmaf(a0, scale[c], shift[c]), 0.f),
                                         fmaxf(fmaf(a1, scale[c + 1], shift[c + 1]), 0.f));
                    }
                    dst[k] = make_uint4(o[0], o[1], o[2], o[3]);
                }
            }
        }
        __syncthreads();
        lds_zero(rb, T_MAP_BYTES);
        __syncthreads();
        conv3_layer<32, 32, 32, 1, 16, false>(ra, rb, nullptr, wp + pn_w_off(1), scale + pn_c_off(1), shift + pn_c_off(1));
        __syncthreads();
        lds_zero(ra, 18 * 18 * 64 * 2);
        __syncthreads();
        conv3_layer<32, 64, 16, 2, 8, false>(rb, ra, nullptr, wp + pn_w_off(2), scale + pn_c_off(2), shift + pn_c_off(2));
        __syncthreads();
        lds_zero(rb, 18 * 18 * 64 * 2);
        __syncthreads();
        conv3_layer<64, 64, 16, 1, 8, false>(ra, rb, nullptr, wp + pn_w_off(3), scale + pn_c_off(3), shift + pn_c_off(3));
        __syncthreads();
        lds_zero(ra, 10 * 10 * 128 * 2);
        __syncthreads();
        conv3_layer<64, 128, 8, 2, 4, false>(rb, ra, nullptr, wp + pn_w_off(4), scale + pn_c_off(4), shift + pn_c_off(4));
        __syncthreads();
        conv3_layer<128, 128, 8, 1, 4, true>(ra, nullptr, maps + patch * PN_MAP, wp + pn_w_off(5), scale + pn_c_off(5),
                                              shift + pn_c_off(5), bad);
    }
}

// --------------------------------------------------------------------------------------------- head
// Layer 7 as a GEMM: a workgroup owns 16 patches x all 128 channels, K = 8192 in the order of the map,
// 256 steps of 32.  Its 8 waves split K: wave w accumulates steps 32 w .. 32 w + 31 (8 accumulators),
// waves 1 .. 7 leave their partial sums in LDS and wave 0 adds them in ascending order -- one fixed
// order whatever the batch.  A fragments come straight from the maps, B fragments from the packed
// weights, which the launch streams through the L2 once per 16 patches.  Rows past B read patch
// B - 1 and are not stored.
constexpr int H_WAVES = 8, H_TB = 64 * H_WAVES, H_STEPS = 256 / H_WAVES;

__global__ void __launch_bounds__(H_TB) k_patchnet_head(const f16_t* __restrict__ maps, long long B, int variant,
                                                        const f16_t* __restrict__ w7, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, float* __restrict__ desc) {
    __shared__ float part[H_WAVES - 1][32][64];   // [wave - 1][4 n + r][lane]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
    for (long long t = blockIdx.x; t * 16 < B; t += gridDim.x) {
        const long long row = t * 16 + fr;
        const f16_t* ap = maps + (row < B ? row : B - 1) * PN_MAP + wave * H_STEPS * 32 + fq * 8;
        const f16_t* bp = w7 + (size_t)wave * H_STEPS * 128 * 32 + fr * 32 + fq * 8;
        h16_f32x4_t acc[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) acc[n] = (h16_f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int ks = 0; ks < H_STEPS; ++ks) {
            const uint4 a = *reinterpret_cast<const uint4*>(ap + ks * 32);
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                const uint4 b = *reinterpret_cast<const uint4*>(bp + ((size_t)ks * 128 + n * 16) * 32);
                acc[n] = HF::mfma(a, b, acc[n]);
            }
        }
        __syncthreads();   // wave 0 has read the previous tile's partial sums
        if (wave > 0) {
#pragma unroll
            for (int n = 0; n < 8; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) part[wave - 1][4 * n + r][lane] = acc[n][r];
        }
        __syncthreads();
        if (wave > 0) continue;
#pragma unroll 1
        for (int w = 0; w < H_WAVES - 1; ++w)
#pragma unroll
            for (int n = 0; n < 8; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[n][r] += part[w][4 * n + r][lane];
        // BatchNorm, then the descriptor normalisation in float32: lane (fr, fq) holds channels
        // 16 n + fr of patches 16 t + 4 fq + r.  Sum of squares: n ascending in the lane, then the xor
        // butterfly (offsets 8 .. 1) over the 16 lanes of a patch.
        float ss[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const float sc = scale[n * 16 + fr], sh = shift[n * 16 + fr];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = fmaf(acc[n][r], sc, sh);
                if (variant == RR_PATCHNET_SOSNET) v += 1e-10f;
                acc[n][r] = v;
                ss[r] = fmaf(v, v, ss[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) ss[r] += __shfl_xor(ss[r], o, 64);
            const float nrm = sqrtf(ss[r]);
            const float den = variant == RR_PATCHNET_HARDNET ? fmaxf(nrm, 1e-12f) : nrm;
            const long long orow = t * 16 + fq * 4 + r;
            if (orow < B) {
#pragma unroll
                for (int n = 0; n < 8; ++n) desc[orow * 128 + n * 16 + fr] = acc[n][r] / den;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------- workspace
struct PatchnetWs {
    f16_t* maps;
};
// the one layout: the layer-6 maps of a chunk
PatchnetWs patchnet_layout(Arena& a, long long chunk) {
    PatchnetWs w;
    w.maps = a.take<f16_t>((size_t)chunk * PN_MAP);
    return w;
}
long long chunk_of(long long B) {
    const long long c = g_tune.patchnet_chunk;
    return B < c ? (B > 0 ? B : 1) : c;
}

const char* check_common(long long B, int variant, const void* packed) {
    if (B < 0) return ": negative patch count";
    if (variant != RR_PATCHNET_HARDNET && variant != RR_PATCHNET_SOSNET) return ": unknown variant";
    if (!packed) return ": null packed weights";
    if (((uintptr_t)packed) & 15) return ": packed weights must be 16-byte aligned";
    return nullptr;
}

int launch_trunk(const float* patches, long long B, int variant, const void* packed, f16_t* maps, hipStream_t s) {
    const f16_t* wp = reinterpret_cast<const f16_t*>(packed);
    const float* bn = reinterpret_cast<const float*>(reinterpret_cast<const char*>(packed) + PN_BN_OFF);
    hipLaunchKernelGGL(k_patchnet_trunk, dim3((unsigned)(B < 65535 ? B : 65535)), dim3(T_TB), 0, s, patches, B,
                       variant, wp, bn, maps);
    return check_launch("rr_patchnet_trunk");
}

int launch_head(const f16_t* maps, long long B, int variant, const void* packed, float* desc, hipStream_t s) {
    const f16_t* wp = reinterpret_cast<const f16_t*>(packed);
    const float* bn = reinterpret_cast<const float*>(reinterpret_cast<const char*>(packed) + PN_BN_OFF);
    const long long tiles = (B + 15) / 16;
    hipLaunchKernelGGL(k_patchnet_head, dim3((unsigned)(tiles < 65535 ? tiles : 65535)), dim3(H_TB), 0, s, maps, B, variant,
                       wp + pn_w_off(6), bn + pn_c_off(6), bn + PN_CHANNELS + pn_c_off(6), desc);
    return check_launch("rr_patchnet_head");
}

}  // namespace

}  // namespace rr

using namespace rr;

extern "C" {

size_t rr_patchnet_packed_bytes(void) { return PN_PACKED_BYTES; }

int rr_patchnet_pack(const float* const* weights, const float* const* means, const float* const* vars, void* packed,
                     size_t packed_bytes, void* stream) {
    const std::string w("rr_patchnet_pack");
    if (!weights || !means || !vars || !packed) return fail(RR_EINVAL, w + ": null pointer");
    PackArgs a;
    for (int l = 0; l < PN_LAYERS; ++l) {
        if (!weights[l] || !means[l] || !vars[l]) return fail(RR_EINVAL, w + ": null tensor of layer " + std::to_string(l + 1));
        a.w[l] = weights[l];
        a.mean[l] = means[l];
        a.var[l] = vars[l];
    }
    if (((uintptr_t)packed) & 15) return fail(RR_EINVAL, w + ": packed must be 16-byte aligned");
    if (packed_bytes < PN_PACKED_BYTES) return fail(RR_ENOSPACE, w + ": packed buffer too small");
    hipLaunchKernelGGL(k_patchnet_pack, dim3(64, PN_LAYERS), dim3(256), 0, as_stream(stream), a,
                       reinterpret_cast<f16_t*>(packed), reinterpret_cast<float*>(reinterpret_cast<char*>(packed) + PN_BN_OFF));
    return check_launch("rr_patchnet_pack");
}

size_t rr_patchnet_workspace_bytes(long long B) {
    if (B < 0) return 0;
    return measured(patchnet_layout, chunk_of(B));
}

int rr_patchnet_trunk(const float* patches, long long B, int variant, const void* packed, void* map, void* stream) {
    const std::string w("rr_patchnet_trunk");
    if (const char* e = check_common(B, variant, packed)) return fail(RR_EINVAL, w + e);
    if (B > 0 && (!patches || !map)) return fail(RR_EINVAL, w + ": null patches or map");
    if ((((uintptr_t)patches) & 7) || (((uintptr_t)map) & 15)) return fail(RR_EINVAL, w + ": misaligned patches or map");
    if (B == 0) return RR_OK;
    return launch_trunk(patches, B, variant, packed, reinterpret_cast<f16_t*>(map), as_stream(stream));
}

int rr_patchnet_head(const void* map, long long B, int variant, const void* packed, float* desc, void* stream) {
    const std::string w("rr_patchnet_head");
    if (const char* e = check_common(B, variant, packed)) return fail(RR_EINVAL, w + e);
    if (B > 0 && (!map || !desc)) return fail(RR_EINVAL, w + ": null map or output");
    if (((uintptr_t)map) & 15) return fail(RR_EINVAL, w + ": misaligned map");
    if (B == 0) return RR_OK;
    return launch_head(reinterpret_cast<const f16_t*>(map), B, variant, packed, desc, as_stream(stream));
}

int rr_patchnet_describe(const float* patches, long long B, int variant, const void* packed, float* desc, void* workspace,
                         size_t workspace_bytes, void* stream) {
    const std::string w("rr_patchnet_describe");
    if (const char* e = check_common(B, variant, packed)) return fail(RR_EINVAL, w + e);
    if (B > 0 && (!patches || !desc)) return fail(RR_EINVAL, w + ": null patches or output");
    if (((uintptr_t)patches) & 7) return fail(RR_EINVAL, w + ": misaligned patches");
    if (B == 0) return RR_OK;
    if (!workspace) return fail(RR_EINVAL, w + ": null workspace");
    const long long chunk = chunk_of(B);
    Arena arena(workspace, workspace_bytes);
    const PatchnetWs ws = patchnet_layout(arena, chunk);
    if (!arena.fits()) return fail(RR_ENOSPACE, w + ": workspace too small");
    for (long long b0 = 0; b0 < B; b0 += chunk) {
        const long long nb = B - b0 < chunk ? B - b0 : chunk;
        int rc = launch_trunk(patches + b0 * 1024, nb, variant, packed, ws.maps, as_stream(stream));
        if (rc != RR_OK) return rc;
        rc = launch_head(ws.maps, nb, variant, packed, desc + b0 * 128, as_stream(stream));
        if (rc != RR_OK) return rc;
    }
    return RR_OK;
}

}  // extern "C"
