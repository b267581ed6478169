// Host half of librr under AddressSanitizer (SURVEY §5 "Race detection /
// sanitizers").  Built by `make -C <csrc> asan` against librr_asan.so (every
// .hip compiled host-only with -fsanitize=address: no device code objects, so
// a launch that gets past the host checks fails with a HIP error instead of
// running).  Drives, on a host without a GPU:
//  * the workspace sizing of every entry point that has one, over a grid of sizes;
//  * the argument checks of the entry points (null / negative / unsupported
//    arguments must return RR_EINVAL / RR_ENOSPACE with a message, never touch memory);
//  * the ragged-batch table packing (> 64 images -> several launches, host arrays
//    of pointers and extents read in full);
//  * rr_set_tuning, rr_last_error, rr_comm_unique_id (RCCL dlopen'ed);
//  * the persistent kernels' tile walks (rr_tilewalk.h), exhaustively over small grids.
// Exit status 0 and the last line "ASAN-DRIVER OK" when nothing was reported.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../image-retrieval-for-image-based-localization_amd/csrc/rr_tilewalk.h"
#include "../../image-retrieval-for-image-based-localization_amd/csrc/rr_workspace.h"
#include "../../include/rr.h"

static int g_fail = 0;
#define EXPECT(cond)                                                               \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, \
                         rr_last_error());                                         \
            ++g_fail;                                                              \
        }                                                                          \
    } while (0)

// a non-null, never-dereferenced stand-in for a device address
static void* fake(size_t off = 0) { return reinterpret_cast<void*>(static_cast<uintptr_t>(0x100000000ull + off)); }

// the blocks of one arena pass: mixed element sizes, a zero-length and a 1-byte block
struct ArenaBlocks {
    char* p[6];
    size_t len[6];
};

static ArenaBlocks arena_blocks(rr::Arena& a) {
    ArenaBlocks b{};
    const size_t cnt[6] = {300, 0, 1, 77, 1000, 5};
    b.p[0] = (char*)a.take<float>(cnt[0]);     b.len[0] = cnt[0] * 4;
    b.p[1] = (char*)a.take<double>(cnt[1]);    b.len[1] = 0;
    b.p[2] = (char*)a.take<char>(cnt[2]);      b.len[2] = 1;
    b.p[3] = (char*)a.take<double>(cnt[3]);    b.len[3] = cnt[3] * 8;
    b.p[4] = (char*)a.take<uint16_t>(cnt[4]);  b.len[4] = cnt[4] * 2;
    b.p[5] = (char*)a.take<unsigned long long>(cnt[5]);  b.len[5] = cnt[5] * 8;
    return b;
}

static void arena_case() {
    rr::Arena m;
    const ArenaBlocks mb = arena_blocks(m);
    for (char* p : mb.p) EXPECT(p == nullptr);                 // measuring hands out nothing
    const size_t need = m.bytes();
    EXPECT(need >= 256 + 1200 + 1 + 616 + 2000 + 40 && need % 256 == 0);
    EXPECT(rr::Arena().bytes() == 256);                        // the base slack alone
    std::vector<char> host(need + 512);                        // ASan guards both ends
    char* base = host.data() + (256 - (uintptr_t)host.data() % 256) % 256 + 8;   // 8 bytes off a 256 boundary
    rr::Arena c(base, need);
    const ArenaBlocks cb = arena_blocks(c);
    EXPECT(c.bytes() == need && c.fits());
    for (int i = 0; i < 6; ++i) {
        EXPECT(cb.p[i] != nullptr && (uintptr_t)cb.p[i] % 256 == 0);
        EXPECT(cb.p[i] >= base && cb.p[i] + cb.len[i] <= base + need);
        for (int j = 0; j < i; ++j) EXPECT(cb.p[j] + cb.len[j] <= cb.p[i]);   // disjoint, in order
        std::memset(cb.p[i], 0x5a, cb.len[i]);                 // inside the host buffer, or ASan reports it
    }
    rr::Arena tight(base, need - 1);
    arena_blocks(tight);
    EXPECT(tight.bytes() == need && !tight.fits());
    for (rr::Arena* a : {&m, &c}) {                            // count * sizeof(T) overflows: saturate, never wrap
        EXPECT(a->take<double>(SIZE_MAX / 4) == nullptr);
        EXPECT(a->bytes() == SIZE_MAX && !a->fits());
        EXPECT(a->take<char>(1) == nullptr && a->bytes() == SIZE_MAX);
    }
    rr::Arena edge(base, SIZE_MAX);                            // the sum overflows, the product does not
    edge.take<char>(1);
    EXPECT(edge.take<char>(SIZE_MAX - 300) == nullptr && edge.bytes() == SIZE_MAX && !edge.fits());
}

// every tile of [0, ntiles) exactly once, and the tiles of each XCD (block & 7) one contiguous run
static bool covers(const std::vector<int>& xcd_of_tile, const std::vector<int>& times) {
    bool seen[8] = {};
    for (size_t t = 0; t < times.size(); ++t) {
        if (times[t] != 1) return false;
        if (t > 0 && xcd_of_tile[t] == xcd_of_tile[t - 1]) continue;
        if (seen[xcd_of_tile[t]]) return false;   // a second run of this XCD
        seen[xcd_of_tile[t]] = true;
    }
    return true;
}

static void tilewalk_case() {
    for (int ntiles = 0; ntiles <= 80; ++ntiles) {
        for (int grid = 8; grid <= 40; ++grid) {        // range walk: any grid of at least 8 blocks
            std::vector<int> xcd(ntiles, -1), times(ntiles, 0);
            bool inside = true;
            for (int b = 0; b < grid; ++b) {
                const rr::TileRange r = rr::xcd_tile_range(b, ntiles, grid);
                const rr::XcdTiles x = rr::xcd_tiles(b, ntiles);
                EXPECT(x.s_x == r.s_x && x.n_x == r.n_x);
                for (int m = 0; r.li + m * r.nb_x < r.n_x; ++m) {
                    const int t = r.s_x + r.li + m * r.nb_x;
                    if (t < 0 || t >= ntiles) { inside = false; continue; }
                    ++times[t];
                    xcd[t] = b & 7;
                }
            }
            EXPECT(inside && covers(xcd, times));
        }
        for (int grid = 8; grid <= 40; grid += 8) {     // round walk: grids that are multiples of 8
            std::vector<int> xcd(ntiles, -1), times(ntiles, 0);
            bool inside = true;
            for (int b = 0; b < grid; ++b) {
                const int n = rr::xcd_round_count(b, ntiles, grid);
                for (int i = 0; i < n; ++i) {
                    const int t = rr::xcd_round_tile(b, grid, i);
                    if (t < 0 || t >= ntiles) { inside = false; continue; }
                    ++times[t];
                    xcd[t] = b & 7;
                }
                EXPECT(rr::xcd_round_tile(b, grid, n) >= ntiles);   // the count stops at the first missing tile
            }
            // contiguous per XCD inside each round of `grid` tiles
            bool ok = inside;
            for (int t0 = 0; t0 < ntiles && ok; t0 += grid) {
                const int n = std::min(grid, ntiles - t0);
                ok = covers(std::vector<int>(xcd.begin() + t0, xcd.begin() + t0 + n),
                            std::vector<int>(times.begin() + t0, times.begin() + t0 + n));
            }
            EXPECT(ok);
        }
        for (int cus : {8, 100, 256}) {
            const int g = rr::persistent_grid8(ntiles, cus);
            EXPECT(g % 8 == 0 && g >= 8 && g <= std::max(8, cus));
        }
        // the range walk's launch grid: one block per CU or one per tile, the rule the GEMM launch
        // sites wrote out, and a grid with which the range walk covers every tile exactly once
        for (int cus : {1, 4, 7, 8, 9, 16, 32, 40}) {
            const int g = (int)rr::range_walk_grid(ntiles, cus);
            EXPECT(g == ntiles || g == cus);
            EXPECT(g == (cus < 8 || ntiles < cus ? ntiles : cus));
            std::vector<int> xcd(ntiles, -1), times(ntiles, 0);
            bool inside = true;
            for (int b = 0; b < g; ++b) {
                const rr::TileRange r = rr::xcd_tile_range(b, ntiles, g);
                for (int m = 0; r.li + m * r.nb_x < r.n_x; ++m) {
                    const int t = r.s_x + r.li + m * r.nb_x;
                    if (t < 0 || t >= ntiles) { inside = false; continue; }
                    ++times[t];
                    xcd[t] = b & 7;
                }
            }
            EXPECT(inside && covers(xcd, times));
        }
    }
}

int main() {
    EXPECT(rr_version() > 0);
    arena_case();
    tilewalk_case();
    EXPECT(rr_last_error() != nullptr);

    // --- workspace sizing
    for (long long n : {1ll, 1000ll, 65536ll, 1000000ll, 10000000ll})
        for (int nq : {1, 70, 128, 1024})
            for (int dt : {RR_F32, RR_BF16, RR_F16, RR_I8}) {
                const size_t b = rr_knn_workspace_bytes(n, nq, 2048, 100, 0, dt);
                EXPECT(b > 0);
                EXPECT(rr_knn_workspace_bytes(n, nq, 2048, 100, 4096, dt) >= b);
            }
    EXPECT(rr_knn_workspace_bytes(0, 10, 2048, 10, 0, RR_F32) == 0);
    for (int rows : {1, 5, 128, 5063}) {
        EXPECT(rr_head_workspace_bytes(rows, 2048) > 0);
        EXPECT(rr_whiten_workspace_bytes(rows, 2048) > 0);
    }
    for (int r : {1, 2, 8}) EXPECT(rr_topk_allgather_workspace_bytes(r, 1024, 100) >= (size_t)r * 1024 * 100 * 16);
    EXPECT(rr_rank_workspace_bytes(5000, 70) > 0);
    EXPECT(rr_local_head_workspace_bytes(8 * 2048, 1024, 128) > 0);

    // --- argument checks (each must fail cleanly)
    double s[4];
    long long ix[4];
    EXPECT(rr_knn_topk(nullptr, nullptr, 0, nullptr, nullptr, 1, 64, 1, 0, 0, s, ix, nullptr, 0, RR_F32, nullptr) ==
           RR_EINVAL);
    EXPECT(rr_knn_topk(fake(), (const float*)fake(), 100, fake(), (const float*)fake(), 1, 48, 1, 0, 0, s, ix,
                       fake(), 1 << 20, RR_F32, nullptr) == RR_EINVAL);          // d not a power of two
    EXPECT(rr_knn_topk(fake(), (const float*)fake(), 100, fake(), (const float*)fake(), 1, 64, 1, 0, 0, s, ix,
                       fake(), 1 << 20, 7, nullptr) == RR_EINVAL);               // dtype
    EXPECT(rr_knn_topk(fake(), (const float*)fake(), 100, fake(), (const float*)fake(), 200, 128, 1, 0, 0, s, ix,
                       fake(), 1 << 30, RR_I8, nullptr) == RR_EINVAL);           // int8 d = 128 above 128 queries
    EXPECT(rr_knn_topk(fake(), (const float*)fake(), 100, fake(), (const float*)fake(), 1, 64, 5, 3, 0, s, ix,
                       fake(), 1 << 20, RR_F32, nullptr) == RR_EINVAL);          // cand < k
    EXPECT(rr_knn_topk(fake(), (const float*)fake(), 100000, fake(), (const float*)fake(), 4, 256, 10, 0, 0, s, ix,
                       fake(), 16, RR_BF16, nullptr) == RR_ENOSPACE);            // workspace too small
    EXPECT(rr_knn_topk_checked_i8(fake(), (const float*)fake(), 100, fake(), (const float*)fake(), 1, 256, 1, 0, 0,
                                  s, ix, fake(), 1 << 20, 1.f, nullptr, 1, nullptr, nullptr, nullptr) == RR_EINVAL);
    EXPECT(rr_topk_merge(nullptr, nullptr, 0, 1, 1, 1, s, ix, nullptr) == RR_EINVAL);
    EXPECT(rr_topk_merge((const double*)fake(), (const long long*)fake(), 8, 1, 4096, 10, s, ix, nullptr) == RR_EINVAL);
    EXPECT(rr_quantize_i8(nullptr, 16, fake(), (float*)fake(), nullptr) == RR_EINVAL);
    EXPECT(rr_quantize_i8((const float*)fake(), 15, fake(), (float*)fake(), nullptr) == RR_EINVAL);
    EXPECT(rr_quantize_i8_rows(nullptr, 4, 16, fake(), (float*)fake(), nullptr) == RR_EINVAL);
    EXPECT(rr_quantize_i8_rows((const float*)fake(), 4, 18, fake(), (float*)fake(), nullptr) == RR_EINVAL);
    EXPECT(rr_quantize_i8_rows((const float*)fake(), 0, 18, fake(), (float*)fake(), nullptr) == RR_OK);

    rr_conv_desc d;
    std::memset(&d, 0, sizeof d);
    d.n = 1; d.h = 8; d.w = 8; d.c_in = 48;  // c_in not a power of two
    d.ho = 8; d.wo = 8; d.c_out = 64; d.kh = d.kw = 1; d.stride = 1; d.dil = 1; d.k_packed = 64; d.ldy = 64;
    EXPECT(rr_conv2d_fused(fake(), fake(), (const float*)fake(), (const float*)fake(), nullptr, fake(), &d, RR_BF16,
                           RR_BF16, nullptr) != RR_OK);
    EXPECT(rr_conv2d_fused(fake(), fake(), nullptr, nullptr, nullptr, fake(), nullptr, RR_BF16, RR_BF16, nullptr) !=
           RR_OK);
    EXPECT(rr_conv1x1_pair(fake(), 100, 32, fake(), nullptr, nullptr, 256, nullptr, nullptr, nullptr, nullptr,
                           nullptr, 1, 0.01f, fake(), nullptr, nullptr, 64, 1, 0.01f, fake(), fake(), RR_BF16,
                           nullptr) == RR_EINVAL);                                // c_in 32: no fused form
    const float* ff = (const float*)fake();
    EXPECT(rr_conv3x3_pair(fake(), 2, 18, 64, nullptr, nullptr, nullptr, 0, 0.f, fake(), ff, ff, 1, 0.01f, fake(), ff, ff, fake(), nullptr, nullptr,
                           nullptr, nullptr, 1, 0.01f, fake(), ff, ff, 64, 1, 0.01f, fake(), fake(), nullptr, RR_BF16,
                           nullptr) == RR_EINVAL);                                // h % 4
    EXPECT(rr_conv3x3_pair(fake(), 2, 16, 64, nullptr, nullptr, nullptr, 0, 0.f, fake(), ff, ff, 1, 0.01f, fake(), ff, ff, nullptr, fake(), fake(),
                           ff, ff, 1, 0.01f, fake(), ff, ff, 128, 1, 0.01f, fake(), fake(), nullptr, RR_F16,
                           nullptr) == RR_EINVAL);                                // projection form with c_out 128
    EXPECT(rr_conv3x3_pair(fake(), 2, 16, 64, nullptr, nullptr, nullptr, 0, 0.f, fake(), ff, ff, 1, 0.01f, fake(), ff, ff, fake(), nullptr, nullptr,
                           nullptr, nullptr, 1, 0.01f, fake(), ff, ff, 64, 1, 0.01f, fake(), fake(), nullptr, RR_F32,
                           nullptr) == RR_EINVAL);                                // 16-bit only

    // --- ragged batches: 150 images (3 launches of <= 64), host tables read in full
    const int n = 150;
    std::vector<const void*> srcs(n);
    std::vector<int> ext(2 * n);
    for (int i = 0; i < n; ++i) {
        srcs[i] = (i % 17 == 5) ? nullptr : fake((size_t)i << 24);
        ext[2 * i] = (i % 17 == 5) ? 0 : 64 + (i * 7) % 64;
        ext[2 * i + 1] = (i % 17 == 5) ? 0 : 96 + (i * 13) % 32;
    }
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    // no device code in this build: each call gets through its table packing, then the launch fails
    const int r1 = rr_image_to_nhwc_ragged(srcs.data(), ext.data(), n, 3, 128, 128, 0, mean, stdv, 1, fake(), 4,
                                           RR_BF16, nullptr);
    EXPECT(r1 != RR_OK);
    const int r2 = rr_stem_conv_pool_ragged(srcs.data(), ext.data(), n, 128, 128, 1, mean, stdv, 1, fake(),
                                            (const float*)fake(), (const float*)fake(), RR_ACT_LEAKY, 0.01f, fake(),
                                            32, 32, RR_F16, nullptr);
    EXPECT(r2 != RR_OK);
    const float pad0 = 0.f;
    const int r3 = rr_pad_images(srcs.data(), ext.data(), n, 3, 128, 128, 4, &pad0, fake(), nullptr);
    EXPECT(r3 != RR_OK);
    ext[3] = 129;  // an extent larger than the batch map
    EXPECT(rr_image_to_nhwc_ragged(srcs.data(), ext.data(), n, 3, 128, 128, 0, mean, stdv, 1, fake(), 4, RR_BF16,
                                   nullptr) == RR_EINVAL);
    EXPECT(rr_pad_images(srcs.data(), ext.data(), n, 3, 128, 128, 3, &pad0, fake(), nullptr) == RR_EINVAL);

    // --- tuning knobs
    EXPECT(rr_set_tuning(7, 64) == RR_OK);
    EXPECT(rr_set_tuning(7, 0) == RR_OK);
    EXPECT(rr_set_tuning(-1, 0) != RR_OK);
    EXPECT(rr_set_tuning(1 << 20, 0) != RR_OK);

    // --- RCCL id (librccl dlopen'ed; any outcome is fine, it must not corrupt memory)
    char id[256];
    const int rc = rr_comm_unique_id(id, 256);
    std::printf("rr_comm_unique_id -> %d (%s)\n", rc, rc ? rr_last_error() : "ok");
    EXPECT(rr_comm_unique_id(id, 16) == RR_EINVAL);

    std::printf("%d check(s) failed\n", g_fail);
    if (g_fail) return 1;
    std::printf("ASAN-DRIVER OK\n");
    return 0;
}
