// Engine tuning state: every rr_set_tuning key is one member of Tuning, its
// default the member initialiser, and TUNE_KEYS maps rr_tune_key to the member
// (and the environment variable that seeds it when the library loads).
// Launch paths read g_tune.<member>; rr_set_tuning / rr_get_tuning
// (rr_runtime.hip) are the only writers.  Values are documented in rr.h.
#pragma once

#include "../../include/rr.h"

namespace rr {

struct Tuning {
    int gemm_config = 0;
    int gemm_stages = 2;
    int gemm_wide = 1;
    int gemm_astat = 0;
    int gemm_xcd_map = 0;
    int stream_1x1 = 1;
    int conv3x3 = 1;
    int grid_cus = 0;
    int gemm8 = 1;  // packed as on the wire: mode in the low two bits, side switches above
    int knn_fused = 1;
    int conv3_pipe = 1;
    int stem = 2;
    int stream_xcd = 1;
    int conv3s = 1;
    int wres = 2;
    int pair_mid = 1;
    int wres_ring = 1;
    int patchnet_chunk = 16384;  // a size key (TUNE_SIZE_KEYS)
    // RR_KNN_FUSED=0 in the environment pins knn_fused to 0 for the process
    bool knn_fused_env_off = false;

    static constexpr int GEMM8_FLAGS = 4 | 8 | 16 | 32 | 64 | 128 | 512;
    int gemm8_mode() const { return gemm8 & 3; }               // 0 off, 1 auto, 2 force where legal
    bool gemm8_tile() const { return gemm8 & 4; }              // one block per tile instead of persistent blocks
    bool gemm8h() const { return !(gemm8 & 8); }               // k_gemm8h / k_gemm8s allowed
    bool gemm8a() const { return !(gemm8 & 16); }              // k_gemm8a allowed
    bool gemm8s() const { return !(gemm8 & 32); }              // k_gemm8s (else k_gemm8h) at <= 128 queries
    bool gemm8_pmajor() const { return !(gemm8 & 64); }        // conv tiles pixel-major (else channel-major)
    bool gemm8a_tile() const { return gemm8 & 128; }           // k_gemm8a one block per tile
    bool gemm8_short_persist() const { return !(gemm8 & 512); }  // short-K 1x1 convs on persistent blocks
};

extern Tuning g_tune;  // rr_runtime.hip

struct TuneKey {
    int Tuning::*member;
    const char* env;  // seeds the member at load, or nullptr
};

// indexed by rr_tune_key
inline constexpr TuneKey TUNE_KEYS[] = {
    {&Tuning::gemm_config, nullptr},
    {&Tuning::gemm_stages, "RR_GEMM_STAGES"},
    {&Tuning::gemm_wide, "RR_GEMM_WIDE"},
    {&Tuning::gemm_astat, nullptr},
    {&Tuning::gemm_xcd_map, nullptr},
    {&Tuning::stream_1x1, nullptr},
    {&Tuning::conv3x3, nullptr},
    {&Tuning::grid_cus, nullptr},
    {&Tuning::gemm8, "RR_GEMM8"},
    {&Tuning::knn_fused, "RR_KNN_FUSED"},
    {&Tuning::conv3_pipe, nullptr},
    {&Tuning::stem, nullptr},
    {&Tuning::stream_xcd, nullptr},
    {&Tuning::conv3s, nullptr},
    {&Tuning::wres, nullptr},
    {&Tuning::pair_mid, nullptr},
    {&Tuning::wres_ring, nullptr},
};
constexpr int TUNE_NKEYS = sizeof(TUNE_KEYS) / sizeof(TUNE_KEYS[0]);
static_assert(TUNE_NKEYS == RR_TUNE_WRES_RING + 1, "one TUNE_KEYS row per rr_tune_key");

// indexed by rr_tune_size_key - RR_TUNE_SIZE_BASE: the keys that set a length (and with it a
// workspace size) instead of choosing a kernel; every value must be >= 1
inline constexpr TuneKey TUNE_SIZE_KEYS[] = {
    {&Tuning::patchnet_chunk, nullptr},
};
constexpr int TUNE_NSIZEKEYS = sizeof(TUNE_SIZE_KEYS) / sizeof(TUNE_SIZE_KEYS[0]);
static_assert(TUNE_NSIZEKEYS == RR_TUNE_PATCHNET_CHUNK - RR_TUNE_SIZE_BASE + 1, "one TUNE_SIZE_KEYS row per rr_tune_size_key");

}  // namespace rr
