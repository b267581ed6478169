/*
 * rr.h — C ABI of librr.so, the MI355X (gfx950) extract-and-match engine.
 *
 * The reference (Tarekbouamer/Image-Retrieval-for-Image-Based-Localization,
 * package `cirtorch`) is pure Python: its hot path is a chain of torch
 * nn.Modules plus two numpy calls.  Each entry point below replaces one
 * reference operator; the Python host package `cirtorch` (same module names,
 * same argument meaning) binds them with ctypes — see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, a negative code on error;
 *     rr_last_error() returns the message (thread-local).
 *   - all tensor pointers are DEVICE pointers; nothing here allocates:
 *     scratch is caller-provided and sized by the matching *_workspace_bytes
 *     (a workspace may start at any address: its blocks begin at the next
 *     256-byte boundary, and the size includes that slack).
 *   - `stream` is a hipStream_t (NULL = default stream); every call only
 *     enqueues work (no host synchronisation), so calls are graph-capturable.
 *   - activations are NHWC ("channels_last"); dtype codes below.
 *   - re-entrant; one process per GPU.
 */
#ifndef RR_H_
#define RR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 16-bit types: every conv kernel; RR_F16 also kNN screening; RR_I8: kNN screening only (rr_quantize_i8) */
enum rr_dtype { RR_F32 = 0, RR_BF16 = 1, RR_F16 = 2, RR_I8 = 3 };
enum rr_act { RR_ACT_IDENTITY = 0, RR_ACT_LEAKY = 1 };
enum rr_pool_mode { RR_POOL_GEM = 0, RR_POOL_MAC = 1, RR_POOL_SPOC = 2 };
enum rr_conv_flags { RR_CONV_AFFINE = 1, RR_CONV_RESIDUAL = 2, RR_CONV_PERM32 = 4 };
enum rr_layout { RR_NHWC = 0, RR_NCHW = 1 };

#define RR_OK 0
#define RR_EINVAL -1
#define RR_EHIP -2
#define RR_ENOSPACE -3

/* ------------------------------------------------------------------ runtime */
int rr_version(void);
/* "source_digest=<12 hex> arch=gfx950": the sha1 digest of the csrc .hip / .h sources and this
 * header the library was built from (tools/src_digest.py), for the provenance of a prebuilt
 * librr.so. */
const char* rr_build_info(void);
const char* rr_last_error(void);
/* Device architecture name of the current device (e.g. "gfx950"). */
int rr_device_arch(char* buf, int buflen);

/* ------------------------------------------------------------ extractor ops */

/* NCHW float32 image batch -> NHWC `dtype` with `c_pad` channels (zeros in the
 * pad channels), optionally (x - mean_c) / std_c.
 * Replaces cirtorch/utils/image.py:86-127 `normalize` (called from
 * datasets/augmentation/random_augmentation.py:174) fused with the layout
 * change the conv stack needs.  mean/std are HOST arrays of c floats. */
int rr_image_to_nhwc(const float* src, int n, int c, int h, int w,
                     const float* mean_host, const float* std_host, int do_normalize,
                     void* dst, int c_pad, int dtype, void* stream);

/* Implicit-GEMM convolution on MFMA with a fused epilogue:
 *   y = act( conv(x, w) * scale[c] + shift[c] (+ residual) )
 * Replaces nn.Conv2d (cirtorch/backbones/resnet.py:61, backbones/misc.py:166-180)
 * followed by the inplace_abn ABN eval BN + leaky_relu / identity
 * (utils/misc.py:175-235) and the residual add + activation of
 * ResidualBlock.forward (backbones/misc.py:184-203).
 *   x  : [n][h][w][c_in]            (dtype)
 *   w  : [c_out][k_packed]          (dtype) k = (kh*KW + kw)*c_in + ci, zero padded
 *   y  : [n*ho*wo][ldy]             (out_dtype), channel c at column c
 *   residual : same layout/dtype as y (flag RR_CONV_RESIDUAL)
 *   RR_CONV_PERM32: w rows are in the 32-row MFMA-interleaved order written by
 *   rr_pack_conv_weights(perm32=1) (c_out % 32 == 0); y is still in natural
 *   channel order.  scale/shift are always indexed by the natural channel.
 * Also used as the score GEMM of the kNN (1x1, ldy = slab width). */
typedef struct rr_conv_desc {
    int n, h, w, c_in;     /* input; c_in = channel stride, power of two */
    int ho, wo, c_out;     /* output */
    int kh, kw, stride, pad, dil;
    int k_packed;          /* weight row length, multiple of 32 */
    int ldy;               /* output row stride in elements (>= c_out) */
    int act;               /* rr_act */
    float slope;           /* leaky slope */
    int flags;             /* rr_conv_flags */
} rr_conv_desc;

int rr_conv2d_fused(const void* x, const void* w, const float* scale, const float* shift,
                    const void* residual, void* y, const rr_conv_desc* desc,
                    int dtype, int out_dtype, void* stream);

/* Pack nn.Conv2d weights w[c_out][c_in][kh][kw] (float32, the reference
 * state-dict layout, cirtorch/backbones/resnet.py:61) into the engine layout
 * out[c_out][k_packed] (`dtype`), k = (kh*KW + kw)*c_in_pad + ci, zero padded
 * channels and K tail; perm32 != 0 stores rows in the RR_CONV_PERM32 order. */
int rr_pack_conv_weights(const float* w, int c_out, int c_in, int kh, int kw, int c_in_pad,
                         int k_packed, int perm32, void* out, int dtype, void* stream);

/* Fused bottleneck boundary, bf16 or fp16 (dtype), PERM32-packed weights (1x1 convs):
 *   y = act3(conv1x1(x, w3) * scale3 + shift3 + shortcut)      [p][c_mid]
 *   z = act1(conv1x1(y, w1) * scale1 + shift1)                 [p][c_out]
 * i.e. conv3 + bn3 + residual add + activation of ResidualBlock i and conv1 +
 * bn1 + activation of block i + 1 (cirtorch/backbones/misc.py:166-203), in one
 * pass that never re-reads y.  shortcut = residual ([p][c_mid]) when given;
 * with residual == NULL it is the block's projection proj_bn(proj_conv(xp))
 * (1x1 stride 1, xp [p][c_in], wp [c_mid][c_in], scalep/shiftp; misc.py:179-182)
 * computed in the same pass.  p = pixels (n*h*w, stride 1).  Shapes: c_in 64,
 * c_mid 256, c_out 64 or 128 (the 256-channel stage); anything else returns
 * RR_EINVAL and the caller runs separate rr_conv2d_fused launches instead. */
int rr_conv1x1_pair(const void* x, long long p, int c_in, const void* w3, const float* scale3,
                    const float* shift3, int c_mid, const void* residual, const void* xp, const void* wp,
                    const float* scalep, const float* shiftp, int act3, float slope3, const void* w1,
                    const float* scale1, const float* shift1, int c_out, int act1, float slope1, void* y,
                    void* z, int dtype, void* stream);

/* One bottleneck block of the 256-channel stage fused (bf16 or fp16 dtype, PERM32 weights):
 *   t2 = act2(conv3x3(t1, w33) * scale2 + shift2)                 3x3 / s1 / p1, 64 -> 64
 *   y  = act3(conv1x1(t2, w3) * scale3 + shift3 + shortcut)       64 -> 256
 *   z  = act1(conv1x1(y, w1) * scale1 + shift1)                   256 -> c_out (64 or 128)
 * conv2 .. conv3 + residual of ResidualBlock i and conv1 of block i + 1
 * (cirtorch/backbones/misc.py:163-203) in one pass: t2 never reaches HBM and the 3x3's
 * matrix work runs beside the boundary's memory traffic.  shortcut = residual ([p][256]) or,
 * with residual == NULL, the projection proj_bn(proj_conv(xp)) (c_out 64).  t1 [n][h][w][64],
 * h % 4 == 0, w % 32 == 0; y / z bit-identical to the unfused launches (the 3x3 kernel +
 * rr_conv1x1_pair).  RR_EINVAL for other shapes (the caller runs those launches instead).
 * w0 (PERM32 [64][64]) or NULL: with w0 (projection form only) t1 is the block's input x and
 * conv1 + bn1 + act0 of the block (t1 = act0(conv1x1(x, w0) * scale0 + shift0)) runs in the
 * same launch; pass x as xp too.  Bit-identical to rr_conv2d_fused of conv1 first.
 * tile_queue: 8 ints, zero on entry, used as per-XCD tile counters (blocks that start late
 * take fewer tiles; the kernel leaves them non-zero, so one zeroed array per launch), or
 * NULL for the static tile walk; the results do not depend on it. */
int rr_conv3x3_pair(const void* t1, int n, int h, int w, const void* w0, const float* scale0,
                    const float* shift0, int act0, float slope0, const void* w33, const float* scale2,
                    const float* shift2, int act2, float slope2, const void* w3, const float* scale3,
                    const float* shift3, const void* residual, const void* xp, const void* wp,
                    const float* scalep, const float* shiftp, int act3, float slope3, const void* w1,
                    const float* scale1, const float* shift1, int c_out, int act1, float slope1, void* y,
                    void* z, int* tile_queue, int dtype, void* stream);

/* 3x3/s2/p1 style max pooling, NHWC.  Replaces nn.MaxPool2d(3, stride=2,
 * padding=1) of the stem (cirtorch/backbones/resnet.py:65). */
int rr_maxpool2d(const void* x, int n, int h, int w, int c, int k, int stride, int pad,
                 void* y, int ho, int wo, int dtype, void* stream);

/* Fused ResNet stem, bf16 or fp16 (dtype): normalise + conv1 7x7/s2/p3 (3 -> 64) + BN affine
 * + activation + max-pool 3x3/s2/p1 in one kernel.  Replaces mod1 =
 * Sequential(conv1, bn1, pool1) of cirtorch/backbones/resnet.py:59-66 applied
 * to the output of utils/image.py:125 `normalize`.
 *   x     : [n][3][h][w] float32 (raw pixels when do_normalize, mean/std HOST arrays of 3)
 *   wpk   : rr_stem_pack_weights output, [64][448] (dtype): the kernel-row layout (k < 256) and the
 *           space-to-depth layout (k >= 256) of the two stem kernel families
 *   scale, shift : [64] float32 (folded BN), act RR_ACT_*, slope for leaky
 *   y     : [n][hp][wp][64] (dtype), hp/wp = the pool of the (h+1)/2 x (w+1)/2 stem map */
int rr_stem_pack_weights(const float* w, int c_out, int c_in, int kh, int kw, void* out, int dtype, void* stream);
int rr_stem_conv_pool(const float* x, int n, int h, int w, const float* mean_host, const float* std_host,
                      int do_normalize, const void* wpk, const float* scale, const float* shift, int act,
                      float slope, void* y, int hp, int wp, int dtype, void* stream);
/* Same, on uint8 pixels [n][3][h][w]: each value is x / 255 in float32 (the
 * torchvision ToTensor the reference's loaders apply, datasets/generic/
 * transform.py:128), so the result equals rr_stem_conv_pool on x / 255.
 * A decoded image crosses PCIe as 1 B per channel instead of 4. */
int rr_stem_conv_pool_u8(const unsigned char* x, int n, int h, int w, const float* mean_host,
                         const float* std_host, int do_normalize, const void* wpk, const float* scale,
                         const float* shift, int act, float slope, void* y, int hp, int wp, int dtype,
                         void* stream);

/* ---- ragged image batches (a PackedSequence of different-size images) ----
 * Replace pad_packed_images (cirtorch/utils/sequence.py:4-67) + normalize
 * (utils/image.py:125) on a cirtorch.utils.parallel.PackedSequence
 * (utils/parallel/packed_sequence.py:8-96) feeding the body: image i is
 * [c][h_i][w_i] at its own DEVICE address srcs[i] (NULL with h_i = w_i = 0 for
 * a None entry); `extents` is a HOST array {h_0, w_0, h_1, w_1, ...}; the
 * batch map is h x w (>= every extent).  Map pixels outside image i read as 0
 * (the reference's top-left zero pad) BEFORE normalisation -- in-tree order,
 * random_augmentation.py:102 then :174 -- so a pad becomes -mean/std when
 * do_normalize.  No padded copy of the batch is written; `srcs` are read
 * directly.  u8: srcs are uint8 pixels read as x / 255 (to_tensor), else
 * float32.  Any n (split internally into launches of <= 64 images). */
int rr_image_to_nhwc_ragged(const void* const* srcs, const int* extents, int n, int c, int h, int w, int u8,
                            const float* mean_host, const float* std_host, int do_normalize,
                            void* dst, int c_pad, int dtype, void* stream);
/* The fused stem (rr_stem_conv_pool) on a ragged batch; y is [n][hp][wp][64]
 * of the h x w batch map.  Results equal rr_stem_conv_pool(_u8) on the padded
 * batch bit for bit. */
int rr_stem_conv_pool_ragged(const void* const* srcs, const int* extents, int n, int h, int w, int u8,
                             const float* mean_host, const float* std_host, int do_normalize, const void* wpk,
                             const float* scale, const float* shift, int act, float slope, void* y, int hp, int wp,
                             int dtype, void* stream);
/* pad_packed_images itself (utils/sequence.py:4-67) for device tensors: one
 * launch writes the [n][c][h][w] padded batch (elements of elem_bytes = 1, 2,
 * 4 or 8 bytes; pad_value points to one HOST element) from the ragged list. */
int rr_pad_images(const void* const* srcs, const int* extents, int n, int c, int h, int w, int elem_bytes,
                  const void* pad_value_host, void* dst, void* stream);

/* Bilinear resize, align_corners=False, NCHW float32 (one image).
 * Replaces nn.functional.interpolate(scale_factor=s, mode='bilinear',
 * align_corners=False) of the multi-scale pyramid (cirtorch/models/GF_net.py:32-35). */
int rr_resize_bilinear(const float* src, int c, int h, int w, float* dst, int ho, int wo,
                       double scale_h, double scale_w, void* stream);

/* Global pooling to out[n][c] float32.
 * GeM: (mean_hw max(x,eps)^p)^(1/p)  — cirtorch/modules/pools.py:30-38
 * MAC: max_hw x                      — pools.py:10-16
 * SPoC: mean_hw x                    — pools.py:20-26
 * x layout RR_NHWC ([n][hw][c], any dtype) or RR_NCHW ([n][c][hw]). */
int rr_global_pool(const void* x, int n, int c, int hw, int layout, int mode,
                   float p, float eps, float* out, int dtype, void* stream);
/* Same, GeM exponent read by the kernel from DEVICE memory when p_dev != NULL
 * (the learnable scalar `pool.p` Parameter, pools.py:34): no host read-back,
 * so every update of the parameter is seen and the call stays graph-capturable. */
int rr_global_pool_pdev(const void* x, int n, int c, int hw, int layout, int mode,
                        float p, const float* p_dev, float eps, float* out, int dtype, void* stream);

/* Row L2 normalisation y = x / (||x||_2 + eps) over `dim` contiguous floats.
 * Replaces cirtorch/modules/normalizations.py:9-16 (L2N). In-place allowed. */
int rr_l2n_rows(const float* x, int rows, int dim, float eps, float* y, void* stream);

/* Dense layer y[r][o] = sum_i x[r][i] * W[o][i] + b[o] (b may be NULL), fp32.
 * Replaces the nn.Linear "learned whitening" of globalHead
 * (cirtorch/modules/heads/global_head.py:26,63). */
int rr_linear_rows(const float* x, int rows, int in_dim, const float* w, const float* b,
                   int out_dim, float* y, void* stream);

/* Fused globalHead tail: y = L2N(W . L2N(x) + b) (whiten != 0) or L2N(x).
 * x: pooled [rows][dim] f32.  Replaces global_head.py:52-67 after the pool.
 * workspace: rr_head_workspace_bytes(rows, dim). */
size_t rr_head_workspace_bytes(int rows, int dim);
int rr_head_l2n_whiten_l2n(const float* x, int rows, int dim, const float* w, const float* b,
                           int whiten, float eps, float* y, void* workspace, void* stream);

/* Regional pooling (R-GeM / R-MAC / R-SPoC): out[n][R][c] float32, one pooled
 * vector per region of every image, all regions in one pass over the map.
 * Replaces the per-region loop of Rpool.roipool (cirtorch/modules/pools.py:127-172:
 * one inner-pool call per narrowed view) and, with the single whole-map region
 * and per-channel exponents, GeMmp (pools.py:43-54).
 * x: NHWC [n][h][w][c], c % 4 == 0, any dtype.  regions: R host rectangles inside
 * the map (copied into the kernel arguments: no device allocation, no host->device
 * copy, graph-capturable; any R).  GeM exponent by p_count: 0 = the host float p;
 * 1 = a device scalar p_dev (semantics of rr_global_pool_pdev); c = a device
 * vector p_dev of one exponent per channel. */
typedef struct rr_region {
    uint16_t y0, x0, h, w;
} rr_region;
int rr_region_pool(const void* x, int n, int h, int w, int c, const rr_region* regions, int R,
                   int mode, float p, const float* p_dev, int p_count, float eps, float* out,
                   int dtype, void* stream);

/* Aggregation of region descriptors: out[n][dim] = L2N(sum_r rv[n][r][:]), eps as
 * rr_l2n_rows; l2n_rows != 0 first L2-normalises every region row (Rpool without
 * a whitening layer).  R <= 1024.  Replaces pools.py:183,195 (with a whitening
 * layer, pools.py:183-187 is rr_head_l2n_whiten_l2n on the n * R rows). */
int rr_region_aggregate(const float* rv, int n, int R, int dim, int l2n_rows, float eps,
                        float* out, void* stream);

/* Post-hoc learned whitening, y = L2N(P[:d_out] (x - m)) per row, computed in
 * float64 on the f64 MFMA like the reference (cirtorch/utils/whiten.py:4-12:
 * numpy promotes the float32 vectors to the float64 m, P of whitenlearn;
 * applied at scripts/test.py:253-254).  x [rows][dim] float32 (dim % 16 == 0),
 * m [dim] float64, P [>= d_out][dim] float64 row-major, y [rows][d_out]
 * float32 (the float64 result rounded once).  L2N adds 1e-6 to the norm.
 * workspace: rr_whiten_workspace_bytes(rows, d_out). */
size_t rr_whiten_workspace_bytes(int rows, int d_out);
int rr_whitenapply(const float* x, int rows, int dim, const double* m, const double* P, int d_out,
                   float* y, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------- matching */

/* Brute-force cosine kNN with exact ordering.
 * Replaces `scores = np.dot(vecs.T, qvecs); ranks = np.argsort(-scores, axis=0)`
 * (scripts/test.py:247-248, scripts/train_globalF.py:733-734), returning only
 * the first k ranks.  Candidates are screened with an MFMA score GEMM in
 * `dtype` (db/q: RR_F32, RR_BF16, or RR_F16 — the fp16 database of SURVEY
 * §8d config 5; d >= 64 for the 16-bit types), then re-scored in float64
 * from the float32 copies and ordered by (score desc, index asc).
 *   db      : [n_db][d] (dtype)      db_f32 : [n_db][d] float32 (re-rank)
 *   q       : [nq][d]   (dtype)      q_f32  : [nq][d]   float32
 *   out_scores : [nq][k] float64     out_idx : [nq][k] int64 (+ idx_offset)
 * `cand` = candidates kept per query (>= k); 0 picks the default for dtype. */
size_t rr_knn_workspace_bytes(long long n_db, int nq, int d, int k, int cand, int dtype);
int rr_knn_topk(const void* db, const float* db_f32, long long n_db,
                const void* q, const float* q_f32, int nq, int d, int k, int cand,
                long long idx_offset, double* out_scores, long long* out_idx,
                void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* Same, with a certificate: out_uncertain[q] = 0 when the screening margin
 * provably covers query q (every row outside the candidates has exact score
 * below the returned k-th score: screening key + error bound, the bound from
 * the screening dtype, d, ||q|| and db_norm_max = max ||db row||), 1 when a
 * cluster tighter than the screening error straddles the candidate cut —
 * re-search such queries with RR_F32 screening / more candidates
 * (cirtorch.search.KnnIndex.search(verify=True) does). */
int rr_knn_topk_checked(const void* db, const float* db_f32, long long n_db,
                        const void* q, const float* q_f32, int nq, int d, int k, int cand,
                        long long idx_offset, double* out_scores, long long* out_idx,
                        void* workspace, size_t workspace_bytes, int dtype, float db_norm_max,
                        int* out_uncertain, void* stream);

/* The certificate for int8 screening (rr_quantize_i8 database, rr_quantize_i8_rows
 * or rr_quantize_i8 queries): q_amax = the queries' max |x| (one per row when
 * q_amax_per_row, else one for all), db_amax = the database's; the bound is the
 * quantisation residual bound s E (||q8|| + ||x8|| + E), s = aq ax / 127^2,
 * E = sqrt(d) / 2 — ~0.02 at d = 2048, so on dense random data most queries stay
 * uncertified (re-search them), while well-separated top-k certify. */
int rr_knn_topk_checked_i8(const void* db, const float* db_f32, long long n_db,
                           const void* q, const float* q_f32, int nq, int d, int k, int cand,
                           long long idx_offset, double* out_scores, long long* out_idx,
                           void* workspace, size_t workspace_bytes, float db_norm_max,
                           const float* q_amax, int q_amax_per_row, const float* db_amax,
                           int* out_uncertain, void* stream);

/* Merge R per-shard top-k lists per query into one top-k by (score desc,
 * index asc).  in_*: [R][nq][k_in]; out_*: [nq][k].  Used after the RCCL
 * all-gather of per-shard results.  k_in*R <= 4096. */
int rr_topk_merge(const double* in_scores, const long long* in_idx, int r, int nq, int k_in,
                  int k, double* out_scores, long long* out_idx, void* stream);

/* ------------------------------------------------------ sharded search (RCCL) */
/* For a non-Python host of the sharded search (one process per GPU; the Python
 * host uses torch.distributed, cirtorch/search.py ShardedIndex).  RCCL is
 * dlopen'ed on first use.  Rank 0 creates the id, the host sends it to every
 * rank out of band, each rank calls rr_comm_init with its GPU current.  Then
 * per search: rr_knn_topk on the local rows (idx_offset = the shard's first
 * global row) -> rr_topk_allgather_merge = RCCL all-gather of the [nq][k]
 * (score f64, index i64) lists over xGMI + rr_topk_merge, bit-identical to a
 * 1-GPU search of the whole database.  Replaces the missing per-rank gather
 * of scripts/train_globalF.py:667-730. */
int rr_comm_unique_id(void* id_out, int id_bytes);                 /* id_bytes >= 128 */
int rr_comm_init(void** comm, int nranks, const void* id, int id_bytes, int rank);
int rr_comm_destroy(void* comm);
size_t rr_topk_allgather_workspace_bytes(int nranks, int nq, int k);
int rr_topk_allgather_merge(void* comm, const double* scores, const long long* idx, int nq, int k,
                            double* out_scores, long long* out_idx, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ------------------------------------------------------- local descriptors */
/* Local-descriptor head (config 5): desc = normalize(W . grid_sample(x, kpts) + b).
 * Replaces cirtorch/modules/heads/local_head.py:43-71 (localHead.forward:
 * functional.grid_sample(mode="bilinear", padding_mode="zeros",
 * align_corners=False) -> nn.Linear(dim, e) -> functional.normalize(dim=2)).
 *   x    : [n][h][w][c] NHWC feature map (dtype), c a multiple of 8 (bf16) / 4 (f32)
 *   kpts : [n][npts][2] float32 normalised (x, y) in [-1, 1] (grid_sample grid)
 *   weight [e][c], bias [e] (may be NULL) float32;  out [n][npts][e] float32
 * workspace: rr_local_head_workspace_bytes(n*npts, c, e). */
size_t rr_local_head_workspace_bytes(long long nkp, int c, int e);
int rr_local_head(const void* x, int n, int h, int w, int c, int dtype, const float* kpts, int npts,
                  const float* weight, const float* bias, int e, float* out, void* workspace,
                  size_t workspace_bytes, void* stream);
/* Mutual nearest neighbours from the two directions' top-1 lists (int64):
 * match[i] = nn12[i] if nn21[nn12[i]] == i else -1.  Replaces the
 * np.argmin/argmin mutual check of HPatchesEval.py:31-43 (nn12/nn21 from
 * rr_knn_topk with k = 1: exact order, ties -> lower index like np.argmin). */
int rr_mutual_nn(const long long* nn12, int n1, const long long* nn21, int n2, long long* match, void* stream);

/* Batched local-descriptor matching: cirtorch/features/matching.py:5-154 (match_nn, match_mnn,
 * match_snn, match_smnn) and, batched, the matcher of HPatchesEval.py:31-43, without the N1 x N2
 * distance matrix of torch.cdist.  npairs ragged pairs in one launch: side-1 rows of pair p are
 * a[a_off[p] : a_off[p + 1]], side-2 rows b[b_off[p] : b_off[p + 1]].
 *   a [rows1][d], b [rows2][d]  float32 rows, 16-byte aligned, any norm; d % 4 == 0, 4 <= d <= 512
 *   a_off, b_off                DEVICE int64 [npairs + 1], ascending, within [0, rows]
 *   max_n1, max_n2              host upper bounds of a pair's side lengths (they size the grid;
 *                               rows1 / rows2 always serve, blocks past a pair's length exit)
 * rr_match_top2: for every row of both sides the two nearest rows of the pair's other side,
 *   d12 [rows1][2] float64 squared L2 distances, i12 [rows1][2] int32 pair-local indices in side 2
 *   (d21 / i21 [rows2][2]: side-2 rows in side 1), ordered by (distance asc, index asc); +inf / -1
 *   where the other side has fewer than two rows.  d2 = max(0, |a|^2 + |b|^2 - 2 a.b) in float64
 *   (v_mfma_f64_16x16x4_f64 on the float32 inputs): identical rows tie bit for bit and the lower
 *   index wins, a row holding a NaN has no neighbour and is nobody's, d12 and d21 hold the same
 *   bits for the same two rows, and no result depends on npairs or the launch.  Rows outside
 *   every pair are not written.
 * rr_match_pairs: rr_match_top2 into the workspace, then the rule of `mode` per side-1 row:
 *   match [rows1] int64 pair-local index in side 2 or -1, dist [rows1] float32 (+inf where -1);
 *   s = float32(sqrt(d2)), the value torch.cdist returns, r12 = s(first) / s(second):
 *     RR_MATCH_NN    nearest row, its distance
 *     RR_MATCH_MNN   kept when the nearest of match[i] is i; its distance
 *     RR_MATCH_SNN   kept when r12[i] <= th (Lowe's ratio test); dist = r12[i]
 *     RR_MATCH_SMNN  both directions pass the ratio test and point at each other;
 *                    dist = max(r12[i], r21[match[i]])
 *   SNN / SMNN keep nothing where a side they rank has fewer than two rows.
 * workspace: rr_match_workspace_bytes(rows1, rows2, lists) with lists = 0 for rr_match_top2,
 * 1 for rr_match_pairs.  Bad arguments return an error before anything is enqueued. */
enum rr_match_mode { RR_MATCH_NN = 0, RR_MATCH_MNN = 1, RR_MATCH_SNN = 2, RR_MATCH_SMNN = 3 };
size_t rr_match_workspace_bytes(long long rows1, long long rows2, int lists);
int rr_match_top2(const float* a, const long long* a_off, long long rows1, const float* b, const long long* b_off,
                  long long rows2, int npairs, int d, int max_n1, int max_n2, double* d12, int* i12, double* d21,
                  int* i21, void* workspace, size_t workspace_bytes, void* stream);
int rr_match_pairs(const float* a, const long long* a_off, long long rows1, const float* b, const long long* b_off,
                   long long rows2, int npairs, int d, int max_n1, int max_n2, int mode, float th, long long* match,
                   float* dist, void* workspace, size_t workspace_bytes, void* stream);

/* Spatial verification of matched pairs: a RANSAC homography per pair, its inlier count and
 * mask.  Replaces, batched and without a host round trip, the per-pair
 * cv2.findHomography(kp1[matches], kp2[matches], cv2.RANSAC) of
 * cirtorch/utils/evaluation/HPatchesEval.py:45-69 (compute_H_estimation) and refits with
 * find_homography_dlt of cirtorch/geometry/homography.py:11-58.  (It is not OpenCV's RANSAC bit
 * for bit: the sampling, the stopping rule and the refit are the ones stated here.)
 *   kp1 [rows1][2], kp2 [rows2][2]  float32 pixel keypoints (x, y), 8-byte aligned
 *   off1, off2                      DEVICE int64 [npairs + 1], the tables of rr_match_pairs
 *   match [rows1]                   int64, what rr_match_pairs wrote: the pair-local side-2 index
 *                                   or -1 (an index outside the pair's side 2 counts as -1)
 *   max_n1                          host upper bound of a pair's side-1 length, <= rows1; rows of
 *                                   a pair past max_n1 are ignored
 * All arithmetic is float64, every sum has a fixed order: results are bit-identical run to run
 * and do not depend on npairs or the launch.  Per pair p:
 *  a. records: the kept rows i (match[i] >= 0) in ascending i as (x1, y1, x2, y2); M of them.
 *  b. hypothesis t in [0, iters): four distinct record indices from a counter hash.  With
 *       mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *     on uint32 (wrapping),
 *       s = mix(lo32(seed) + 0x9e3779b9);  s = mix(s ^ hi32(seed));  s = mix(s + p);  s = mix(s + t)
 *     and a = [0, 1, ..., M - 1]:  for j = 0, 1, 2, 3:
 *       k = mix(s + j) mod (M - j);  sample_j = a[k];  a[k] = a[M - 1 - j]
 *     (a partial Fisher-Yates draw over the M - j records that remain).  The homography through
 *     the four records, scaled to H[2][2] = 1.  The hypothesis is degenerate and scores 0 when,
 *     on either side, the determinant [[xa, xb, xc], [ya, yb, yc], [1, 1, 1]] =
 *     (xb - xa)(yc - ya) - (xc - xa)(yb - ya) of any three of its four points has magnitude
 *     <= RR_VERIFY_DET_EPS (px^2: twice a triangle's area; the float64 rounding of that
 *     expression on coordinates below 2^11 is below 1e-9), or an entry of H is not finite.
 *  c. score: the number of records with |w| > 1e-8 and (u - x2 w)^2 + (v - y2 w)^2 <= th^2 w^2,
 *     (u, v, w) = H [x1, y1, 1] -- that is || pi(H x1) - x2 ||^2 <= th^2 without the division.
 *     The winner is the hypothesis of the highest score, the lowest t among equals.
 *  d. refit, `refine` times: S = the inliers of H; H' = find_homography_dlt on S (unweighted:
 *     normalize_points on both sides, A^T A of the rows of homography.py:32-33, the eigenvector
 *     of its smallest eigenvalue by cyclic Jacobi, T2^-1 h T1, divided by H[2][2] + 1e-8);
 *     H' replaces H when it is finite and score(H') >= score(H), otherwise the refit stops.
 *  e. inliers[p] = score(H), H [npairs][3][3] float64 row-major, mask [rows1] uint8 = 1 on the
 *     side-1 rows that are inliers of H (every row of the pair is written).  M < 4 or no
 *     hypothesis with a score above 0: inliers 0, H all zeros, mask 0.
 * workspace: rr_verify_workspace_bytes(rows1, npairs, iters).  Nothing waits for the host
 * (graph-capturable).  Bad arguments (null pointers, iters < 1, refine < 0, th <= 0 or not finite,
 * max_n1 > rows1, a short workspace) return an error before anything is enqueued; npairs == 0
 * returns RR_OK and launches nothing. */
#define RR_VERIFY_DET_EPS 1e-6
size_t rr_verify_workspace_bytes(long long rows1, int npairs, int iters);
int rr_verify_pairs(const float* kp1, const long long* off1, long long rows1, const float* kp2, const long long* off2,
                    long long rows2, const long long* match, int npairs, int max_n1, double th, int iters, int refine,
                    unsigned long long seed, int* inliers, double* H, unsigned char* mask, void* workspace,
                    size_t workspace_bytes, void* stream);
/* Batched weighted DLT: find_homography_dlt of cirtorch/geometry/homography.py:11-58 (and the
 * solver inside find_homography_dlt_iterated, :61-74) with normalize_points of
 * cirtorch/geometry/epipolar/fundamental.py:6-33, for npairs ragged point sets in one launch; the
 * device routine of step d above.
 *   pts1, pts2 [rows][2]  float64 (x, y), 16-byte aligned; set p is rows off[p] .. off[p + 1]
 *   weights [rows]        float64 or NULL (unweighted); they weigh the two rows of a point in
 *                         A^T W A, the normalisation is over all points of the set
 *   off                   DEVICE int64 [npairs + 1]
 *   H [npairs][3][3]      float64; all zeros for a set of fewer than 4 points
 * sqrt(2) of normalize_points is the float32 value the reference's torch.sqrt(torch.tensor(2.))
 * yields.  The eigenvector comes from cyclic Jacobi on the 9 x 9 matrix, rotations skipped where
 * |a_pq| <= 2^-52 sqrt(a_pp a_qq), until a sweep rotates nothing (the reference: the last right
 * singular vector of torch.svd; the sign cancels in the division).
 * workspace: none is needed (NULL, 0); the arguments are reserved. */
int rr_homography_dlt(const double* pts1, const double* pts2, const double* weights, const long long* off,
                      long long rows, int npairs, double* H, void* workspace, size_t workspace_bytes, void* stream);

/* Epipolar verification of matched pairs (rr_epipolar.hip): a RANSAC fundamental matrix per pair,
 * its inlier count and mask -- the model for two views of a 3-D scene from different positions,
 * where correct matches at different depths share no homography.  Brings
 * cirtorch/geometry/epipolar/fundamental.py:6-86 and metrics.py:4-83 to the device.  The
 * arguments, the float64 arithmetic, the fixed summation order and the independence of npairs and
 * the launch are those of rr_verify_pairs; F [npairs][3][3] float64 row-major satisfies
 * [x2, y2, 1] F [x1, y1, 1]^T = 0.  Per pair p:
 *  a. records: step a of rr_verify_pairs.
 *  b. hypothesis t in [0, iters): seven distinct record indices by the hash and the partial
 *     Fisher-Yates draw of rr_verify_pairs with j = 0 .. 6 (its first four are that entry's four).
 *     The seven-point solver, on each side: u = s x + tx, v = s y + ty with (mx, my) the mean of
 *     the seven points, s = sqrt(2) / (mean distance to it + 1e-8), tx = -s mx, ty = -s my (the
 *     transform T of normalize_points; sqrt(2) is the float32 value, as below).  The 7 x 9 system
 *     has the rows [u2 u1, u2 v1, u2, v2 u1, v2 v1, v2, u1, v1, 1] (fundamental.py:69).  F1 and F2
 *     are the vectors of its null space whose last two entries are (1, 0) and (0, 1), as 3 x 3
 *     row-major matrices; a system whose leading 7 x 7 block is singular has no such basis, its
 *     entries are not finite and the hypothesis scores 0.  With D = F1 - F2 and
 *     det3(a, b, c) = a0 (b1 c2 - b2 c1) - a1 (b0 c2 - b2 c0) + a2 (b0 c1 - b1 c0) on rows, the cubic
 *     det(l F1 + (1 - l) F2) = det(F2 + l D) = c0 + c1 l + c2 l^2 + c3 l^3 has
 *       c0 = det3(F2_0, F2_1, F2_2),  c3 = det3(D_0, D_1, D_2),
 *       c1 = det3(D_0, F2_1, F2_2) + det3(F2_0, D_1, F2_2) + det3(F2_0, F2_1, D_2),
 *       c2 = det3(F2_0, D_1, D_2) + det3(D_0, F2_1, D_2) + det3(D_0, D_1, F2_2).
 *     Cubic rule: c3 == 0 (or any value not finite) gives no root -- F2 alone, the root at
 *     infinity, is not tried.  Otherwise a = c2 / c3, b = c1 / c3, c = c0 / c3,
 *     Q = (a^2 - 3 b) / 9, R = (2 a^3 - 9 a b + 27 c) / 54.  R^2 < Q^3: three real roots
 *       l_k = -2 sqrt(Q) cos((theta + 2 pi k) / 3) - a / 3,  theta = acos(clamp(R / sqrt(Q^3), -1, 1)),
 *     in ascending order k = 0, -1, +1.  R^2 >= Q^3 (a double root included): the one root
 *       l = A + B - a / 3,  A = -sign(R) cbrt(|R| + sqrt(R^2 - Q^3)),  B = Q / A (0 when A == 0).
 *     Root number r (0, 1, 2 in ascending l) gives F = T2^T (F2 + l D) T1; a root whose F has an
 *     entry that is not finite scores 0.
 *  c. score of a root: the number of records with den > 0 and num <= th^2 den, where
 *     num = ([x2, y2, 1] F [x1, y1, 1]^T)^2 and den = (F x1)_0^2 + (F x1)_1^2 + (F^T x2)_0^2 +
 *     (F^T x2)_1^2 -- the squared Sampson distance of metrics.py:33-38 at most th^2 (th in pixels),
 *     without the division.  The winner is (score desc, t asc, root asc).
 *  d. refit, `refine` times: S = the inliers of F; when |S| >= 8, F' = the unweighted
 *     rr_fundamental_dlt fit on S; F' replaces F when it is finite and score(F') >= score(F),
 *     otherwise (and when |S| < 8) the refit stops.
 *  e. inliers[p] = score(F); mask [rows1] uint8 = 1 on the side-1 rows that are inliers of F
 *     (every row of the pair is written); then F is scaled to unit Frobenius norm with its entry
 *     of largest magnitude positive (the lowest row-major index among equal magnitudes).  It is
 *     not divided by F[2][2]: a sideways translation has F[2][2] = 0.  M < 7 or no root with a
 *     score above 0: inliers 0, F all zeros, mask 0.
 * On a planar scene, or between views that differ by a pure rotation, F is not determined: the
 * count is inflated and rr_verify_pairs is the model to use.  There is no degeneracy test.
 * workspace: rr_verify_epipolar_workspace_bytes(rows1, npairs, iters).  Nothing waits for the host
 * (graph-capturable).  Bad arguments are refused as by rr_verify_pairs, before anything is
 * enqueued; npairs == 0 returns RR_OK and launches nothing. */
size_t rr_verify_epipolar_workspace_bytes(long long rows1, int npairs, int iters);
int rr_verify_pairs_epipolar(const float* kp1, const long long* off1, long long rows1, const float* kp2,
                             const long long* off2, long long rows2, const long long* match, int npairs, int max_n1,
                             double th, int iters, int refine, unsigned long long seed, int* inliers, double* F,
                             unsigned char* mask, void* workspace, size_t workspace_bytes, void* stream);
/* Batched weighted 8-point fit: find_fundamental of cirtorch/geometry/epipolar/fundamental.py:49-86
 * for npairs ragged point sets in one launch; the device routine of step d above.  Arguments as
 * rr_homography_dlt (pts 16-byte aligned float64, weights or NULL, DEVICE offsets).
 *   F [npairs][3][3]  float64; all zeros for a set of fewer than 8 points
 * normalize_points on all points of the set, each side (weights do not enter it; sqrt(2) is the
 * float32 value the reference's torch.sqrt(torch.tensor(2.)) yields); X^T W X of the rows
 * [u2 u1, u2 v1, u2, v2 u1, v2 v1, v2, u1, v1, 1], summed as sum w (p2 p2^T) (x) (p1 p1^T), p = (u, v, 1);
 * the eigenvector of its smallest eigenvalue by the cyclic Jacobi of rr_homography_dlt, as a
 * 3 x 3 matrix f; the rank-2 projection f - (f v3) v3^T, v3 the eigenvector of the smallest
 * eigenvalue of f^T f (cyclic Jacobi on the 3 x 3, pairs (0, 1), (0, 2), (1, 2), the same skip
 * criterion) -- equal to the reference's U diag(s1, s2, 0) V^T; then F = T2^T f T1 and
 * normalize_transformation: F / (F[2][2] + 1e-8) where |F[2][2]| > 1e-8, F itself otherwise.
 * workspace: none is needed (NULL, 0); the arguments are reserved. */
int rr_fundamental_dlt(const double* pts1, const double* pts2, const double* weights, const long long* off,
                       long long rows, int npairs, double* F, void* workspace, size_t workspace_bytes, void* stream);
/* Epipolar distances of correspondences under a fundamental matrix per set:
 * sampson_epipolar_distance and symmetrical_epipolar_distance of metrics.py:4-83.
 *   pts1, pts2 [rows][2]  float64 (x, y), 16-byte aligned; set p is rows off[p] .. off[p + 1]
 *   F [npairs][3][3]      float64;  off DEVICE int64 [npairs + 1]
 *   out [rows]            float64; rows of no set are not written
 * With num, d1 = (F x1)_0^2 + (F x1)_1^2 and d2 = (F^T x2)_0^2 + (F^T x2)_1^2 of step c above:
 * RR_EPI_SAMPSON num / (d1 + d2), RR_EPI_SYMMETRICAL num (1 / d1 + 1 / d2); squared = 0 returns
 * sqrt(that + eps).  A zero denominator yields what IEEE division yields, as in the reference.
 * Bad arguments (null pointers, an unknown kind, squared not 0 / 1, eps negative or not finite)
 * return an error before anything is enqueued; npairs == 0 returns RR_OK. */
enum rr_epi_kind { RR_EPI_SAMPSON = 0, RR_EPI_SYMMETRICAL = 1 };
int rr_epipolar_distance(const double* pts1, const double* pts2, const double* F, const long long* off, long long rows,
                         int npairs, int kind, int squared, double eps, double* out, void* stream);

/* Calibrated verification of matched pairs (rr_epipolar.hip, rr_fivepoint.h): a RANSAC essential
 * matrix per pair from five-point samples -- the model for two views whose intrinsics are known.
 * It has five degrees of freedom instead of seven and stays determined (up to two discrete
 * solutions) on a planar scene.  The arguments of rr_verify_pairs_epipolar plus
 *   K1, K2 [npairs][3][3]  float64 row-major intrinsics of the two views, DEVICE, 16-byte aligned
 *   E [npairs][3][3]       float64 row-major, x2n^T E x1n = 0 for xn = K^-1 [x, y, 1]^T
 * Records, score, the refit's acceptance and the mask are those of rr_verify_pairs_epipolar, in
 * pixels: a matrix E is scored as F = K2^-T E K1^-1, so inliers and mask mean the same under both
 * models.  Per pair p:
 *  a. records: step a of rr_verify_pairs.  K1^-1 and K2^-1 by the adjugate divided by the
 *     determinant.  A K with an entry that is not finite, a determinant that is zero or not finite,
 *     or an inverse with an entry that is not finite fails the pair (step e).
 *  b. hypothesis t in [0, iters): five distinct record indices by the hash and the partial
 *     Fisher-Yates draw of rr_verify_pairs with j = 0 .. 4.  The five-point solver on the homogeneous
 *     points h1 = K1^-1 [x1, y1, 1]^T, h2 = K2^-1 [x2, y2, 1]^T (not divided by their last entry):
 *     1. the 5 x 9 system A with rows h2 (x) h1 (entry 3 a + b = h2_a h1_b).  Five Householder
 *        reflections H_k = I - 2 v_k v_k^T / v_k^T v_k, k = 0 .. 4, make the 9 x 5 matrix A^T upper
 *        triangular: v_k = x + sign(x_0) |x| e_0 on entries k .. 8, x the current column k from its
 *        diagonal down (sign(0) = +).  X, Y, Z, W = H_0 H_1 H_2 H_3 H_4 e_j, j = 5, 6, 7, 8, as 3 x 3
 *        row-major matrices: an orthonormal basis of the null space, and E = x X + y Y + z Z + W.  (The
 *        basis whose entries 5 .. 8 are unit vectors was measured first: its entries reach 1e4 on
 *        normalised points and one sample in thirty loses every digit in step 2.)
 *     2. det E = 0 (expanded along the first row) and the nine entries of 2 E E^T E - tr(E E^T) E = 0
 *        in row-major order are ten cubics in (x, y, z): a 10 x 20 matrix in the monomials
 *          x^3, y^3, x^2 y, x y^2, x^2 z, x^2, y^2 z, y^2, xyz, xy | x z^2, xz, x, y z^2, yz, y, z^3, z^2, z, 1,
 *        reduced by Gauss-Jordan with partial pivoting on its first ten columns.
 *     3. with <m> the row whose pivot is the monomial m, the three rows <x^2 z> - z <x^2>,
 *        <y^2 z> - z <y^2>, <xyz> - z <xy> are x bx(z) + y by(z) + bc(z) with deg bx = deg by = 3,
 *        deg bc = 4 (Nister).  The determinant of that 3 x 3 matrix, expanded along its first row, is a
 *        polynomial c(z) of degree 10.  Root rule: c10 == 0 or a coefficient that is not finite gives
 *        no root.  All roots lie in |z| < Bz = 1 + max_i |c_i / c10|.  For d = 1 .. 10 the real roots
 *        of derivative number 10 - d of c (degree d) are found from those of derivative number 11 - d:
 *        these and -Bz, Bz cut the line into intervals in ascending order, and an interval holds a
 *        root where the sign (value < 0) of the polynomial differs at its ends; the root is the
 *        midpoint after 48 bisection steps, followed by 3 Newton steps, each kept only where it
 *        stays inside the last bracket.  Every simple real root is found, in ascending order; two
 *        roots between which c does not change sign at the computed critical point (a double root,
 *        or a pair closer than that critical point's error) are not found and count as none.
 *     4. at a root z the 3 x 3 matrix has the null vector (x, y, 1): the cross product n of two of
 *        its rows, the pair (0,1), (0,2), (1,2) with the largest |n_2| (the first among equals),
 *        x = n_0 / n_2, y = n_1 / n_2.  Root number r (ascending z) gives E, and F = K2^-T E K1^-1; a
 *        root whose F has an entry that is not finite scores 0.  At most 10 roots.
 *  c. score of a root: step c of rr_verify_pairs_epipolar on F.  The winner is (score desc, t asc,
 *     root asc).
 *  d. refit, `refine` times: S = the inliers of F; when |S| >= 8, F' = the unweighted
 *     rr_fundamental_dlt fit on S in pixels, E' = K2^T F' K1 (essential_from_fundamental,
 *     essential.py:8-18), E'' = the projection of E' onto the essential matrices: with v_i the
 *     eigenvectors of E'^T E' by the 3 x 3 cyclic Jacobi of rr_fundamental_dlt, the one of the smallest
 *     eigenvalue dropped (the lower index among equals), s_i = sqrt(eigenvalue), s = (s_a + s_b) / 2,
 *     E'' = s (E' v_a) v_a^T / s_a + s (E' v_b) v_b^T / s_b = U diag(s, s, 0) V^T; F'' = K2^-T E'' K1^-1
 *     replaces F when it is finite and score(F'') >= score(F), otherwise (and when |S| < 8) the refit
 *     stops.  On a plane the 8-point fit is rank deficient and the rule keeps the minimal solution.
 *  e. inliers[p] = score(F); mask as rr_verify_pairs_epipolar; E = K2^T F K1 projected as in step d,
 *     scaled to unit Frobenius norm with its entry of largest magnitude positive (the lowest
 *     row-major index among equal magnitudes).  M < 5, a failed K or no root with a score above 0:
 *     inliers 0, E all zeros, mask 0.
 * On a plane two essential matrices explain the points (the true one and its twisted twin); either
 * may win.  workspace: rr_verify_essential_workspace_bytes(rows1, npairs, iters).  Nothing waits for
 * the host (graph-capturable).  Bad arguments are refused as by rr_verify_pairs_epipolar, and so are
 * a null or misaligned K1 / K2, before anything is enqueued; npairs == 0 returns RR_OK and launches
 * nothing. */
size_t rr_verify_essential_workspace_bytes(long long rows1, int npairs, int iters);
int rr_verify_pairs_essential(const float* kp1, const long long* off1, long long rows1, const float* kp2,
                              const long long* off2, long long rows2, const long long* match, int npairs, int max_n1,
                              const double* K1, const double* K2, double th, int iters, int refine, unsigned long long seed,
                              int* inliers, double* E, unsigned char* mask, void* workspace, size_t workspace_bytes,
                              void* stream);
/* The five-point solver of step b above alone, one thread per sample.
 *   x1, x2 [n][5][2]  float64 normalised points (h = [x, y, 1]), 16-byte aligned
 *   E [n][10][3][3]   float64: the solutions in ascending root order, each scaled to unit Frobenius
 *                     norm with its entry of largest magnitude positive; all zeros past nroots[i]
 *   nroots [n]        int32; a sample with a root whose E is not finite has nroots 0 and zeros
 * n < 0, null pointers and misaligned points are refused before anything is enqueued; n == 0
 * returns RR_OK. */
int rr_essential_5pt(const double* x1, const double* x2, int n, double* E, int* nroots, void* stream);

/* Relative pose of verified pairs (rr_pose.hip): the essential matrix of a fundamental matrix, its
 * four candidate motions, the triangulation of the pair's matches under each and the choice of the
 * motion that puts the most points in front of both cameras.  Brings essential_from_fundamental
 * (cirtorch/geometry/epipolar/essential.py:8-18), decompose_essential_matrix (:21-54),
 * motion_from_essential (:75-89), motion_from_essential_choose_solution (:92-153), triangulate_points
 * (triangulation.py:7-41), projection_from_KRt and depth (projection.py:60-78, :111-119) and
 * convert_points_from_homogeneous (conversions.py:67-83) to the device.  kp1, off1, rows1, kp2, off2,
 * rows2, match, npairs and max_n1 are those of rr_verify_pairs_epipolar, and every output of that
 * entry is an input here.
 *   mask [rows1]                 uint8 as rr_verify_pairs_epipolar writes it, or NULL: every matched row
 *   F, K1, K2 [npairs][3][3]     float64 row-major: the fundamental matrix ([x2, y2, 1] F [x1, y1, 1]^T = 0)
 *                                and the intrinsics of the two views
 *   R, E [npairs][3][3]          float64;  t [npairs][3] float64, unit norm;  front [npairs] int32
 *   points3d [rows1][3]          float64, in the frame of the first camera, in units of |t|
 *   front_mask [rows1]           uint8
 * All arithmetic is float64 and a result depends on the pair's own data only.  Per pair p:
 *  a. used records: the kept rows of step a of rr_verify_pairs (0 <= match[i] < n2, i < max_n1) with,
 *     when mask is given, mask[i] != 0; as (x1, y1, x2, y2) in float64.
 *  b. E0 = K2^T F K1 (essential.py:18).  Its singular value decomposition: the eigenvectors of
 *     E0^T E0 by the 3 x 3 cyclic Jacobi of rr_fundamental_dlt, v0 and v1 those of the largest and
 *     the second largest eigenvalue (the lower index first among equals); a_i = E0 v_i,
 *     u0 = a0 / |a0|, u1 = b / |b| with b = a1 - (u0 . a1) u0, u2 = u0 x u1, v2 = v0 x v1.  U = [u0 u1 u2]
 *     and V = [v0 v1 v2] have determinant +1, which is the sign fix of essential.py:33-40 in closed
 *     form.  E = u0 v0^T + u1 v1^T = U diag(1, 1, 0) V^T.
 *  c. candidates 0 .. 3: (Ra, t), (Ra, -t), (Rb, t), (Rb, -t) with W = [[0, -1, 0], [1, 0, 0], [0, 0, 1]],
 *     Ra = U W V^T = u1 v0^T - u0 v1^T + u2 v2^T, Rb = U W^T V^T = u0 v1^T - u1 v0^T + u2 v2^T, t = u2.
 *     The labelling of Ra / Rb and the sign of t follow the signs of v0 and v1, which the Jacobi
 *     iteration fixes and another SVD would fix otherwise: the candidate order is this entry's own,
 *     not the reference's.  The set of four is the same, and so is the winner whenever it is unique.
 *  d. every used record is triangulated under each candidate as triangulate_points does, in pixel
 *     units: P1 = K1 [I | 0], P2 = K2 [R | t]; the 4 x 4 system with rows x1 P1_2 - P1_0,
 *     y1 P1_2 - P1_1, x2 P2_2 - P2_0, y2 P2_2 - P2_1 (P_r: row r; triangulation.py:27-31); its right
 *     singular vector h of the smallest singular value (the lower index among equals) by one-sided
 *     (Hestenes) Jacobi on the columns of the 4 x 4 itself -- not on A^T A, whose condition number is
 *     the square --: column pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), a pair is rotated where
 *     |c_p . c_q| > 2^-52 sqrt(|c_p|^2 |c_q|^2) (the criterion and the angle of rr_homography_dlt with
 *     a_pp = |c_p|^2, a_qq = |c_q|^2, a_pq = c_p . c_q), the same rotation applied to the identity
 *     gives the singular vectors, until a sweep rotates nothing or RR_POSE_SWEEPS sweeps are done.
 *     X = s (h0, h1, h2), s = 1 / h3 where |h3| > 1e-8 and 1 otherwise (conversions.py:77-83).  The
 *     depths are X_z and (R X)_z + t_z; a record is in front under a candidate when both are > 0.
 *  e. the winner is the candidate with the most records in front, the lowest index among equals.
 *     R, t, front[p] (its count), front_mask (1 on its records in front) and points3d (its X on used
 *     rows, zeros on the other rows) come from the winner; every row of the pair (below max_n1) is
 *     written.  An F with an entry that is not finite or with all entries zero (what
 *     rr_verify_pairs_epipolar returns for a failed pair), a K with an entry that is not finite,
 *     |a0| not finite, |a1| or |b| not > 0, and a pair with no used record give zeros in R, t, E,
 *     points3d and front_mask and front = 0.
 * Deliberate deviation: motion_from_essential_choose_solution indexes Rs[:, mask_indices][:, 0, 0]
 * (essential.py:149-151), which for a batch of more than one applies the choice of pair 0 to every
 * pair.  Here every pair chooses its own solution.
 * The fused entry shares its device routines with the two entries below: its result has the bits of
 * rr_essential_decompose on E0, rr_triangulate_points under P1 and each candidate's P2 and a count
 * of the depths (E0 and the P are products inside this entry; with K1 = K2 = I they are exact and
 * the chain can be formed outside).  workspace: none is needed (NULL, 0); the arguments
 * are reserved.  Nothing waits for the host (graph-capturable).  Bad arguments (null pointers, negative
 * sizes, max_n1 > rows1, misaligned keypoints) return an error before anything is enqueued;
 * npairs == 0 returns RR_OK and launches nothing. */
#define RR_POSE_SWEEPS 30
int rr_recover_pose(const float* kp1, const long long* off1, long long rows1, const float* kp2, const long long* off2,
                    long long rows2, const long long* match, const unsigned char* mask, const double* F, const double* K1,
                    const double* K2, int npairs, int max_n1, double* R, double* t, double* E, int* front,
                    double* points3d, unsigned char* front_mask, void* workspace, size_t workspace_bytes, void* stream);
/* Batched triangulation: triangulate_points of triangulation.py:7-41 for npairs ragged point sets
 * in one launch; the device routine of step d above.
 *   pts1, pts2 [rows][2]   float64 (x, y), 16-byte aligned; set p is rows off[p] .. off[p + 1]
 *   P1, P2 [npairs][3][4]  float64 row-major projection matrices of the two views
 *   off                    DEVICE int64 [npairs + 1]
 *   X [rows][3]            float64; rows of no set are not written
 * Bad arguments are refused before anything is enqueued; npairs == 0 returns RR_OK. */
int rr_triangulate_points(const double* pts1, const double* pts2, const double* P1, const double* P2, const long long* off,
                          long long rows, int npairs, double* X, void* stream);
/* Steps b and c above for n essential matrices: decompose_essential_matrix of essential.py:21-54.
 *   E [n][3][3] float64 -> R1 = Ra, R2 = Rb [n][3][3], t [n][3] float64 (unit norm)
 * A matrix that step e above refuses gives zeros.  n < 0 and null pointers are refused before
 * anything is enqueued; n == 0 returns RR_OK. */
int rr_essential_decompose(const double* E, int n, double* R1, double* R2, double* t, void* stream);

/* Localization: the absolute pose of a camera against known 3-D points (rr_pnp.hip, rr_p3p.h) -- a
 * RANSAC pose per pair from three-point samples (P3P), refitted by Gauss-Newton on the reprojection
 * error of its inliers.  The step after rr_recover_pose: side 1 is the query image's keypoints, side 2
 * the 3-D points of a database image (points3d and front_mask of rr_recover_pose are indexed by that
 * image's keypoint rows, and rr_match_pairs(query, that image) returns indices into those rows).  The
 * upstream project has no absolute pose (it calls OpenCV on the host for its geometry): every rule is
 * this entry's own.  kp1, off1, rows1, off2, rows2, match, npairs, max_n1, th, iters, refine and seed
 * are those of rr_verify_pairs_essential.
 *   pts3d [rows2][3]   float64 3-D points in any world frame, 8-byte aligned
 *   valid [rows2]      uint8 or NULL (every point): front_mask of rr_recover_pose
 *   K [npairs][3][3]   float64 row-major intrinsics of the query camera, DEVICE, 16-byte aligned
 *   inliers [npairs] int32;  R [npairs][3][3], t [npairs][3] float64;  mask [rows1] uint8
 * The pose satisfies [x, y, 1]^T ~ K (R X + t).  All arithmetic is float64, every sum has a fixed
 * order, and a result depends on the pair's own data only.  Per pair p:
 *  a. records: row i < min(n1, max_n1) is kept where 0 <= match[i] < n2, valid is NULL or
 *     valid[match[i]] != 0, and the three coordinates of X = pts3d[match[i]] are finite; as
 *     (x, y, X, Y, Z) in float64 in ascending i; M of them.  K^-1 by the adjugate divided by the
 *     determinant; step a of rr_verify_pairs_essential's failure rule for K fails the pair (step e).
 *  b. hypothesis t in [0, iters): three distinct record indices by the hash and the partial
 *     Fisher-Yates draw of rr_verify_pairs with j = 0, 1, 2 (the first three of that entry's four).
 *     P3P by Grunert's elimination on the records 1, 2, 3 of the sample:
 *       j_k = h_k / |h_k|, h_k = K^-1 [x_k, y_k, 1]^T;
 *       a^2 = |X2 - X3|^2, b^2 = |X1 - X3|^2, c^2 = |X1 - X2|^2;  ca = j2 . j3, cb = j1 . j3, cg = j1 . j2;
 *       q = (a^2 - c^2) / b^2, p = (a^2 + c^2) / b^2;
 *     with s_k the distance of point k along j_k, v = s3 / s1 is a root of A4 v^4 + .. + A0:
 *       A4 = (q - 1)^2 - 4 (c^2 / b^2) ca^2
 *       A3 = 4 [q (1 - q) cb - (1 - p) ca cg + 2 (c^2 / b^2) ca^2 cb]
 *       A2 = 2 [q^2 - 1 + 2 q^2 cb^2 + 2 ((b^2 - c^2) / b^2) ca^2 - 4 p ca cb cg + 2 ((b^2 - a^2) / b^2) cg^2]
 *       A1 = 4 [-q (1 + q) cb + 2 (a^2 / b^2) cg^2 cb - (1 - p) ca cg]
 *       A0 = (1 + q)^2 - 4 (a^2 / b^2) cg^2
 *     Real roots by the root rule of step b.3 of rr_verify_pairs_essential at degree 4 (A4 == 0 or a
 *     coefficient that is not finite gives none; the bound 1 + max |A_i / A4|; for d = 1 .. 4 the roots
 *     of derivative number 4 - d from those of derivative number 5 - d; 48 bisections, 3 guarded Newton
 *     steps): every simple real root, in ascending order; double roots are not found.  Per root v:
 *       u = [(q - 1) v^2 - 2 q cb v + 1 + q] / (2 (cg - v ca));
 *       s1 = b / sqrt(1 + v^2 - 2 v cb), s2 = u s1, s3 = v s1;
 *     the root is kept where v > 0, u > 0, s1 > 0 and s1, s2, s3 are finite.  Solution number r is the
 *     r-th kept root in ascending v; at most 4.  Its pose, from Y_k = s_k j_k: with
 *       e1 = (X2 - X1) / |X2 - X1|,  e3 = e1 x (X3 - X1) normalised,  e2 = e3 x e1
 *     and f1, f2, f3 the same construction on Y:  R = [f1 f2 f3] [e1 e2 e3]^T,  t = Y1 - R X1.
 *     A sample gives no solution where b^2 is not > 0, |e1 x (X3 - X1)| is not > 0, or R or t of a kept
 *     root has an entry that is not finite.
 *  c. score of a solution: with P = K [R | t] (3 x 4) and (pc0, pc1, pc2) = P [X, Y, Z, 1]^T, the
 *     number of records with pc2 > 0 and (pc0 - x pc2)^2 + (pc1 - y pc2)^2 <= th^2 pc2^2 -- the
 *     reprojection error at most th pixels without the division; a point behind the camera never
 *     counts.  The winner is (score desc, t asc, solution asc).
 *  d. refit, `refine` times: S = the inliers of (R, t), fixed for the round; while |S| >= 4,
 *     RR_PNP_GN_STEPS Gauss-Newton steps on the sum over S of |r_i|^2, r_i = (pc0 / pc2 - x,
 *     pc1 / pc2 - y) with pc = K Xc, Xc = R X + t of the current iterate; a record of S with pc2 not
 *     > 0 contributes nothing to that step.  Left perturbation Xc' = exp([w]x) Xc + tau: the 2 x 6
 *     Jacobian of r_i in (w, tau) is D K [-[Xc]x | I], D = [[1, 0, -pc0 / pc2], [0, 1, -pc1 / pc2]] / pc2.
 *     The 21 entries of the upper triangle of H = sum J^T J and the 6 of g = sum J^T r are summed
 *     per thread over i = tid, tid + 256, .. and over the block in the fixed order of
 *     rr_homography_dlt's sums; H d = -g by Cholesky without pivoting, and a pivot that is not > 0 or
 *     not finite stops the refit.  R <- exp([w]x) R, t <- exp([w]x) t + tau with exp([w]x) =
 *     I + A [w]x + B [w]x^2, A = sin(a) / a, B = (1 - cos(a)) / a^2, a = |w|, and the series
 *     A = 1 - a^2 / 6, B = 1/2 - a^2 / 24 where a^2 < RR_PNP_SMALL_ANGLE2.  The new pose replaces
 *     the old one when it is finite and its score does not drop; otherwise (and when |S| < 4) the
 *     refit stops.
 *  e. inliers[p] = the score of (R, t); mask [rows1] uint8 = 1 on the side-1 rows that are kept
 *     (step a) and inliers (step c); every row of the pair (below max_n1) is written; R and t are
 *     the final pose.  M < 3, a failed K or no solution with a score above 0: inliers 0, R and t all
 *     zeros, mask 0.
 * Not here: EPnP / DLT on more than three points, local optimisation inside the loop, early
 * termination, lens distortion.  workspace: rr_localize_workspace_bytes(rows1, npairs, iters).  Nothing
 * waits for the host (graph-capturable).  Bad arguments (null pointers, negative sizes, iters < 1 or
 * above 2^24, refine < 0, th <= 0 or not finite, max_n1 > rows1, a null or misaligned K, a short
 * workspace) return an error before anything is enqueued; npairs == 0 returns RR_OK and launches
 * nothing. */
#define RR_PNP_GN_STEPS 3
#define RR_PNP_SMALL_ANGLE2 1e-8
size_t rr_localize_workspace_bytes(long long rows1, int npairs, int iters);
int rr_localize_pairs(const float* kp1, const long long* off1, long long rows1, const double* pts3d,
                      const unsigned char* valid, const long long* off2, long long rows2, const long long* match,
                      int npairs, int max_n1, const double* K, double th, int iters, int refine, unsigned long long seed,
                      int* inliers, double* R, double* t, unsigned char* mask, void* workspace, size_t workspace_bytes,
                      void* stream);
/* The three-point solver of step b above alone, one thread per sample.
 *   x [n][3][2]     float64 normalised image points (h = [x, y, 1], K = I), 8-byte aligned
 *   X [n][3][3]     float64 3-D points
 *   R [n][4][3][3], t [n][4][3]  float64: the solutions in ascending v; all zeros past nsol[i]
 *   nsol [n]        int32
 * n < 0 and null pointers are refused before anything is enqueued; n == 0 returns RR_OK. */
int rr_p3p(const double* x, const double* X, int n, double* R, double* t, int* nsol, void* stream);

/* Keypoint detection (rr_detect.hip): corner / blob responses, 2-D non-maxima suppression and the
 * best N local maxima per image.  Replaces harris_response, gftt_response and hessian_response of
 * cirtorch/features/responses.py:8-103 (spatial_gradient of cirtorch/filters/sobel.py:12-45,
 * gaussian_blur2d of cirtorch/filters/gaussian.py:8-16, filter2D of cirtorch/filters/filter.py:34-77),
 * rgb_to_grayscale of cirtorch/enhance/color/gray.py:7-25, nms2d of cirtorch/features/nms.py:29-67
 * and the torch.topk(x * mask) after it -- and with them the host-side cv2 SIFT detector of
 * cirtorch/datasets/localFeatures/utils.py:56-99.  The image is read once (apart from tile halos)
 * and the score written once: no gradient, product or blurred plane ever exists in memory.
 *
 * The response of a plane.  x [n][c][h][w] float32, or uint8 with u8 = 1 (a pixel is then
 * float32(v) / 255.0f in IEEE float32, so the result has the bits of the float32 path fed
 * x.float() / 255).  gray = 0: each of the n c planes is scored on its own, out [n][c][h][w];
 * gray = 1: c must be 3, a pixel is (0.299 r + 0.587 g) + 0.114 b and out is [n][1][h][w].
 * With p(y, x) the pixel at clamped coordinates (replicate padding):
 *   dx = ((p(y-1,x+1) - p(y-1,x-1)) + 2 (p(y,x+1) - p(y,x-1)) + (p(y+1,x+1) - p(y+1,x-1))) / 8
 *   dy = ((p(y+1,x-1) - p(y-1,x-1)) + 2 (p(y+1,x) - p(y-1,x)) + (p(y+1,x+1) - p(y-1,x+1))) / 8
 * (the 3 x 3 Sobel pair / 8 as a correlation: dx > 0 where the right neighbour is larger),
 *   A = G * dx^2,  B = G * dy^2,  C = G * (dx dy),  det = A B - C C,  tr = A + B
 * with G the 7 x 7 Gaussian of sigma 1 applied separably (along x, then along y, taps in ascending
 * offset; the seven weights are the float32 values of get_gaussian_kernel1d(7, 1.0)) on reflected
 * coordinates (-i reads i, h - 1 + i reads h - 1 - i; the edge sample is not repeated), and
 *   RR_RESP_HARRIS   det - k tr^2
 *   RR_RESP_GFTT     0.5 (tr - sqrt(|tr^2 - 4 det|))
 *   RR_RESP_HESSIAN  dxx dyy - dxy^2, the 5 x 5 second-order Sobel kernels gxx, gxy, gyy as
 *                    correlations over clamped coordinates (rows, then columns, ascending), divided
 *                    by the sums of their magnitudes 64, 36, 64 (1 / 36 as its float32 value, which
 *                    is what the reference's normalised kernel holds).
 * sigmas: NULL or DEVICE float32 [n]; the score of every plane of image i is multiplied by
 * sigma_i^4 = (s s)(s s).  All arithmetic is float64 in one fixed order per pixel and each score is
 * rounded once to float32: a score depends on the pixels of its window only, not on n, the tile,
 * the launch or the run.  Only sobel gradients (grads_mode = 'sobel') exist.
 * Errors, before anything is enqueued: null x or out, c < 1, h or w below 4 (what the reference's
 * reflect padding accepts), gray not 0 / 1 or gray with c != 3, an unknown kind, a non-finite k for
 * Harris, more than 2^31 pixels.  n == 0 returns RR_OK and launches nothing.  Nothing waits for the
 * host (graph-capturable). */
#define RR_RESP_HARRIS 0
#define RR_RESP_GFTT 1
#define RR_RESP_HESSIAN 2
int rr_response(const void* x, int n, int c, int h, int w, int u8, int gray, int kind, double k, const float* sigmas,
                float* out, void* stream);
/* 2-D non-maxima suppression of float32 planes x [planes][h][w] with a square window ks in
 * {3, 5, 7, 9}.  A pixel is kept when its value is greater than 0 and strictly greater than every
 * other position of the window; window coordinates are clamped to the map and a clamped neighbour
 * that lands on the centre still counts, so a pixel on the map's edge is never kept; NaN is never
 * kept.  (The comparison with 0 is the reference's: the centre filter of _get_nms_kernel2d,
 * nms.py:6-15, is all zeros, so its maximum over the other positions includes 0 and it keeps no
 * maximum that is not positive.)  out: mask_only = 1 a uint8 mask [planes][h][w], else x * mask as
 * float32.  Pure comparisons: the result equals the reference's on finite maps bit for bit.
 * Errors: null x or out, a bad ks, h or w < 1, more than 2^31 pixels.  planes == 0 returns RR_OK.
 * Nothing waits for the host. */
int rr_nms2d(const float* x, long long planes, int h, int w, int ks, int mask_only, void* out, void* stream);
/* The best num local maxima of one score plane per image, score [n][h][w] float32.  Candidates are
 * the pixels the NMS rule above keeps for ks whose score is > min_score and which lie at least
 * `border` pixels from every edge (border <= x < w - border, likewise y).  The num best by (score
 * descending, y w + x ascending) go to
 *   kpts [n][num][2] float32 pixel (x, y) -- the layout rr_verify_pairs takes --,
 *   scores [n][num] float32, count [n] int32;
 * the slots past count hold (-1, -1) and score 0.  1 <= num <= 8192.  No two 8-neighbours are both
 * strict maxima, so an image has at most ceil(h / 2) ceil(w / 2) candidates; the workspace
 * (rr_detect_workspace_bytes(n, h, w, num)) is sized by that bound and cannot overflow.  Candidates
 * are compacted with integer atomics in any order; their keys (score bits, index) are unique per
 * image, so the selected set and its order are fully determined.
 * Errors: null pointers, a bad ks, num, h or w, a negative border, a NaN min_score, more than 2^31
 * pixels, a short workspace (RR_ENOSPACE).  n == 0 returns RR_OK.  Nothing waits for the host. */
size_t rr_detect_workspace_bytes(int n, int h, int w, int num);
int rr_select_keypoints(const float* score, int n, int h, int w, int ks, int num, float min_score, int border, float* kpts,
                        float* scores, int* count, void* workspace, size_t workspace_bytes, void* stream);
/* The response of x [n][c][h][w] (c = 1, or c = 3 reduced to gray), written to score_map
 * [n][1][h][w] (or, when score_map is NULL, into the workspace), then the selection above on the
 * same stream: bit-identical to calling the two entries one after the other.  Errors: those of the
 * two entries and c not 1 or 3.  n == 0 returns RR_OK.  Nothing waits for the host. */
int rr_detect_keypoints(const void* x, int n, int c, int h, int w, int u8, int kind, double k, const float* sigmas, int ks,
                        int num, float min_score, int border, float* kpts, float* scores, int* count, float* score_map,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Scale-space keypoint detection (rr_scalespace.hip): image -> Gaussian scale pyramid -> response per
 * level -> strict 3-D extrema with sub-voxel refinement -> local affine frames (LAFs) -> the best num
 * frames per image over all octaves.  Replaces ScaleSpaceDetector.detect of
 * cirtorch/features/scale_space_detector.py:85-161 with ConvQuadInterp3d as its nms module.  Common to
 * the entries: all arithmetic is float64 in one fixed order per output and every stored value is rounded
 * once, no atomic touches a floating-point value, a result depends on its own image only (not on the
 * batch, the launch or the run), argument errors are returned before anything is enqueued and nothing
 * waits for the host (graph-capturable).
 *
 * rr_gaussian_blur: gaussian_blur2d of cirtorch/filters/gaussian.py:8-16 (filter2D of
 * cirtorch/filters/filter.py:34-77) with border_type 'reflect' on float32 planes x [planes][h][w].
 * The 1-D taps are the float32-valued weights of get_gaussian_kernel1d(ksize, sigma)
 * (cirtorch/filters/kernels.py:26-35): e_i = exp(-(i - ksize / 2)^2 / (2 sigma^2)) in float64, their sum
 * in ascending i, t_i = float32(e_i / sum) -- the rule of rr_sift_describe's window.  The blur is
 * separable: along x, then along y, taps in ascending offset, on reflected coordinates (-i reads i,
 * h - 1 + i reads h - 1 - i; the edge sample is not repeated); the x pass is kept in float64 and the
 * output is rounded once.  ksize is odd, at most 63, and ksize / 2 < min(h, w) (what reflect padding
 * accepts); sigma > 0.  Errors: those, null pointers, more than 2^31 pixels.  planes == 0 returns RR_OK. */
int rr_gaussian_blur(const float* x, long long planes, int h, int w, int ksize, double sigma, float* out, void* stream);
/* rr_scale_pyramid: ScalePyramid.forward of cirtorch/geometry/transform/pyramid.py:30-158 with
 * double_image = False.  x [n][c][h][w] float32, or uint8 with u8 = 1 (a pixel is float32(v) / 255.0f);
 * c is 1 or 3, three channels become (0.299 r + 0.587 g) + 0.114 b first.  With L = levels + 3,
 * step = 2^(1 / levels), ksize(s) = int(8 s + 1) made odd:
 *   first level   the image blurred by s0 = max(sqrt(sigma^2 - 0.25), 0.01) with ksize(s0) taps when
 *                 sigma > 0.5 (the level's sigma is then `sigma`), else the image (sigma 0.5);
 *   level l >= 1  level l - 1 blurred by s = cur sqrt(step^2 - 1), cur the sigma of level l - 1, with
 *                 min(ksize(s), min(h_o, w_o)) taps made odd again (the reference's cap is part of the
 *                 rule); its sigma is cur step;
 *   next octave   its first level is level L - 3 at the even pixels (F.interpolate(scale_factor = 0.5,
 *                 mode = 'nearest')), size floor(h_o / 2) x floor(w_o / 2), its sigma is `sigma`;
 *                 octaves stop when the next one's smaller side is <= min_size.
 * The octave count, the sizes, every sigma and kernel size are host arithmetic from (h, w, levels,
 * sigma, min_size); nothing is read back.  out holds, octave after octave, [n][1][L][h_o][w_o] float32;
 * octave o + 1 starts n L h_o w_o floats, rounded up to a multiple of 64, after octave o.  A level is
 * blurred from the float64 value of the previous level (kept in the workspace), not from its float32
 * rounding: each float32 level is rounded once.  rr_scale_pyramid_bytes gives the bytes of out and of the
 * workspace.  1 <= levels <= 8, min_size >= 1, every blur at most 63 taps.
 * Errors: a bad c, levels, sigma or min_size, h or w too small for the reflect padding of a level
 * (RR_EINVAL), more than 2^31 pixels in x or in an octave, more than 16 octaves, null pointers, a short
 * out or workspace (RR_ENOSPACE).  n == 0 returns RR_OK. */
int rr_scale_pyramid_bytes(int n, int c, int h, int w, int levels, double sigma, int min_size, size_t* out_bytes,
                           size_t* workspace_bytes);
int rr_scale_pyramid(const void* x, int n, int c, int h, int w, int u8, int levels, double sigma, int min_size, float* out,
                     size_t out_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* dog_response of cirtorch/features/responses.py:106-115: out [n][L - 1][h][w] = levels[:, l + 1] -
 * levels[:, l] of levels [n][L][h][w] float32.  L >= 2.  n == 0 returns RR_OK. */
#define RR_RESP_DOG 3
int rr_dog_response(const float* levels, int n, int L, int h, int w, float* out, void* stream);
/* rr_scale_space_extrema: nms3d(x, (3, 3, 3)) of cirtorch/features/nms.py:70-108 and conv_quad_interp3d
 * of cirtorch/geometry/subpix/spatial_soft_argmax.py:348-411 on a volume x [n][D][h][w] float32.
 * A voxel is a candidate when its value is > 0 and strictly greater than its 26 neighbours at clamped
 * coordinates, so no voxel on a face of the volume (first and last level included) is kept; NaN is never
 * kept (the rule of rr_nms2d in three dimensions).  With minima = 1 the same rule on -x gives candidates
 * too; p below is then -x.  Refinement of a candidate, with p(d, y, x) the volume -- the taps of
 * spatial_gradient3d(mode = 'diff') of cirtorch/filters/sobel.py:48-78 (replicate border, which no
 * candidate reaches), whose kernel is flipped along the level axis:
 *   b = (gx, gy, gs) = (p(x+1) - p(x-1), p(y+1) - p(y-1), p(d-1) - p(d+1)) / 2
 *   dxx = (p(x-1) + p(x+1)) - 2 p, dyy and dss likewise
 *   dxy = 0.25 (((p(y-1,x-1) - p(y-1,x+1)) - p(y+1,x-1)) + p(y+1,x+1))
 *   dys = 0.25 (((p(d-1,y+1) - p(d-1,y-1)) + p(d+1,y-1)) - p(d+1,y+1))
 *   dxs = 0.25 (((p(d-1,x+1) - p(d-1,x-1)) + p(d+1,x-1)) - p(d+1,x+1))
 *   H = [[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]],  offset (ox, oy, os) = -H^-1 b
 * solved in float64 by elimination with partial pivoting; a singular system (a zero pivot) or a
 * non-finite solution gives a zero offset, and so does any |offset| > 0.7.
 * value = p + 0.5 ((gx ox + gy oy) + gs os).  The reference's rand * eps on H is left out.
 * Two deliberate deviations from the reference: it adds the x offset to y and the y offset to x
 * (create_meshgrid3d orders a voxel (d, x, y) and dx.flip(1) yields (ds, dy, dx)) -- here each offset
 * belongs to its own axis --, and no strict_maxima_bonus is added to values.
 * Outputs: mask [n][D][h][w] uint8 (0 none, 1 maximum, 2 minimum), offsets [n][3][D][h][w] float32 in
 * the order (os, ox, oy) of the reference's coordinates (d, x, y), values [n][D][h][w] float32: the
 * refined value of a candidate, x elsewhere.
 * Errors: null pointers, D, h or w < 1, minima not 0 / 1, more than 2^31 voxels.  n == 0 returns RR_OK. */
int rr_scale_space_extrema(const float* x, int n, int D, int h, int w, int minima, unsigned char* mask, float* offsets,
                           float* values, void* stream);
/* Frames and selection (scale_space_detector.py:137-161).  resp has the pyramid's layout (octave after
 * octave [n][L][h_o][w_o] of (h, w, levels, sigma, min_size)); the volume of an octave is its first
 * D = L - 1 planes (the reference drops the last level of Hessian, Harris and GFTT; DoG has L - 1).
 * For each candidate of the rule above with refined coordinates (s, y, x) = (d + os, y + oy, x + ox):
 *   sig = first_sigma 2^(s / levels), first_sigma the sigma of the octave's first level,
 *   frame [[a, 0, x], [0, a, y]] in octave pixels, a = mr_size sig.
 * The frame is dropped unless its centre and the 11 points (x + a sin t_i, y + a cos t_i), t_i the
 * float32 values of linspace(0, 2 pi, 11) and sin, cos their float32 values -- laf_to_boundary_points(laf,
 * 12) of laf_is_inside_image, cirtorch/features/laf.py:180-203,363-382 -- lie in [0, w_o] x [0, h_o].
 * It is mapped to the image by normalize_laf on the octave and denormalize_laf on the image:
 * a' = (a / min(h_o, w_o)) min(h, w), x' = (x (1 / w_o)) w, y' = (y (1 / h_o)) h.  The score is the
 * refined value.  The best num per image over all octaves by (score descending, octave ascending, voxel
 * index (d h_o + y) w_o + x ascending) go to lafs [n][num][2][3], scores [n][num] float32 and count [n]
 * int32; the slots past count hold a zero frame and score 0.  The reference also cuts every octave to num
 * before the inside test; that is not reproduced (they differ only when an octave has more than num
 * extrema).  No two 26-neighbours are both strict maxima (or both minima), so an octave has at most
 * 2 ceil(D / 2) ceil(h_o / 2) ceil(w_o / 2) candidates per image: the lists in the workspace are sized by
 * that bound and cannot overflow; keys (score bits, octave and voxel) are unique per image and compacted
 * with integer atomics.  1 <= num <= 8192; any workspace of rr_detect_scale_space_workspace_bytes will do.
 * Errors: those of the pyramid's arguments, minima not 0 / 1, mr_size not positive, a bad num, more than
 * 2^32 - 1 voxels per image, null pointers, a short workspace (RR_ENOSPACE).  n == 0 returns RR_OK. */
int rr_scale_space_select(const float* resp, int n, int h, int w, int levels, double sigma, int min_size, int minima,
                          double mr_size, int num, float* lafs, float* scores, int* count, void* workspace,
                          size_t workspace_bytes, void* stream);
/* The whole detector on one stream: rr_scale_pyramid, then per octave rr_response (kind RR_RESP_HARRIS,
 * RR_RESP_GFTT or RR_RESP_HESSIAN on the n L planes with the level sigmas as its `sigmas`) or
 * rr_dog_response (RR_RESP_DOG), then rr_scale_space_select: bit-identical to calling them one after the
 * other.  The pyramid is at the (256-byte aligned) start of the workspace.
 * rr_detect_scale_space_workspace_bytes returns 0 for arguments the detector refuses.
 * Errors: those of the entries, an unknown kind, a non-finite k for Harris, an octave below 4 pixels for
 * the three corner responses.  n == 0 returns RR_OK. */
size_t rr_detect_scale_space_workspace_bytes(int n, int c, int h, int w, int levels, double sigma, int min_size);
int rr_detect_scale_space(const void* x, int n, int c, int h, int w, int u8, int levels, double sigma, int min_size, int kind,
                          double k, int minima, double mr_size, int num, float* lafs, float* scores, int* count,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Keypoint description (rr_describe.hip): local-affine-frame (LAF) patches, the dominant gradient
 * orientation of a patch, the SIFT descriptor of a patch, and the three fused per keypoint.  Common
 * to the four entries: all arithmetic is float64 in one fixed order per output and rounded once to
 * float32, no atomic touches a floating-point value, a result depends on its own patch only (not on
 * the batch, the slot, the launch or the run), argument errors are returned before anything is
 * enqueued, and nothing waits for the host (graph-capturable).  pi below is the float32 value
 * 3.14159274... that the reference's pi tensor (cirtorch/geometry/conversions.py:29) holds, also in
 * its float64 run.  8 <= ps <= 64.  One block of 256 threads works on one patch or keypoint slot and
 * a grid holds fewer than 2^32 threads, so a call takes at most 2^24 - 1 patches (extract: n npts
 * channels) or slots; more is an argument error, split the batch.
 *
 * rr_extract_patches replaces extract_patches_simple and generate_patch_grid_from_normalized_LAF
 * (cirtorch/features/laf.py:260-308: normalize_laf, denormalize_laf, F.affine_grid, F.grid_sample
 * with bilinear, border, align_corners=False) without the normalise / denormalise round trip.
 * x [n][c][h][w] float32, or uint8 with u8 = 1 (a pixel is float32(v) / 255.0f, as in rr_response);
 * gray = 1: c must be 3 and a pixel is (0.299 r + 0.587 g) + 0.114 b, one output channel.
 * lafs [n][npts][2][3] float32 in pixels.  out [n][npts][c or 1][ps][ps] float32.  For patch row i,
 * column j and frame [[a00, a01, a02], [a10, a11, a12]]:
 *   u = (2 j + 1) / ps - 1,  v = (2 i + 1) / ps - 1
 *   sx = ((a00 u + a01 v) + a02) - 0.5 clamped to [0, w - 1],  sy likewise with row 1 and h
 *   x0 = floor(sx), x1 = min(x0 + 1, w - 1), fx = sx - x0 (y likewise)
 *   value = ((p00 (1-fx)(1-fy) + p01 fx (1-fy)) + p10 (1-fx) fy) + p11 fx fy
 * A frame with a non-finite entry gives a zero patch (the reference is undefined there).
 * Errors: null pointers, c < 1, h or w < 1, a bad gray, ps, npts < 0, more than 2^31 image pixels,
 * more than 2^24 - 1 patches.  n npts == 0 returns RR_OK. */
int rr_extract_patches(const void* x, int n, int c, int h, int w, int u8, int gray, const float* lafs, int npts, int ps,
                       float* out, void* stream);
/* rr_patch_orientation replaces PatchDominantGradientOrientation.forward
 * (cirtorch/features/orientation.py:56-105).  patches [B][ps][ps] float32, 1 <= num_ang_bins <= 64,
 * angle [B] float32 in radians.  Per pixel, on clamped patch coordinates, dx and dy are the Sobel
 * pair / 8 of rr_response,
 *   mag = sqrt((dx^2 + dy^2) + 1e-8),  ori = atan2(dy, dx + 1e-8) + 2 pi
 *   o = nb (ori + pi) / (2 pi),  b0 = floor(o),  w1 = o - b0
 * bin b0 mod nb takes (1 - w1) mag and bin (b0 + 1) mod nb takes w1 mag; a bin is the MEAN over the
 * patch.  No Gaussian weight: the reference builds one and never applies it.  The histogram is
 * smoothed circularly with the float32 values of [0.33, 0.34, 0.33]; idx is the argmax (ties to the
 * lower index) and angle = -((2 pi idx) / nb - pi).
 * Errors: null pointers, a bad ps or num_ang_bins, B outside [0, 2^24).  B == 0 returns RR_OK. */
int rr_patch_orientation(const float* patches, long long B, int ps, int num_ang_bins, float* angle, void* stream);
/* rr_sift_describe replaces SIFTDescriptor.forward (cirtorch/features/siftdesc.py:78-129).
 * patches [B][ps][ps] float32, 1 <= num_ang_bins <= 16, 1 <= num_spatial_bins <= 8,
 * out [B][num_ang_bins ns^2] float32.  (ps, ns) must pass get_sift_bin_ksize_stride_pad
 * (siftdesc.py:21-37): ksize = 2 int(ps / (ns + 1)), stride = ps / ns, pad = ksize / 4 and
 * (ps + 2 pad - ksize) / stride + 1 == ns, else RR_EINVAL.  Per pixel, on clamped patch coordinates:
 *   gx = (p(y, x+1) - p(y, x-1)) / 2,  gy = (p(y+1, x) - p(y-1, x)) / 2
 *   mag = sqrt((gx^2 + gy^2) + 1e-10) G(y, x),  ori = atan2(gy, gx + 1e-10) + 2 pi
 *   o = (nb ori) / (2 pi),  b0 = floor(o),  w1 = o - b0
 * bin b0 mod nb takes (1 - w1) mag, bin (b0 + 1) mod nb takes w1 mag.  G is float32-valued, as in
 * the reference: G(y, x) = g(y) g(x) multiplied in float32, g the 1-D Gaussian of sigma =
 * ps / sqrt 2 at x - ps / 2 (+ 0.5 for even ps), normalised to sum 1 (computed in float64, each
 * weight rounded to float32; the reference's float32 exponentials differ from that in the last
 * place).  Each angular plane is pooled by the ksize x ksize kernel with the float32 values
 * (xc(ky) xc(kx)) / (ksize / 2)^2, xc(k) = ksize / 2 - |k + 0.5 - ksize / 2|, at stride and pad with
 * zeros outside the patch; out index a ns^2 + cy ns + cx.  Then v / max(|v|_2, 1e-12), clamp to
 * [0, clipval], v / max(|v|_2, 1e-12) and, with rootsift, sqrt(v / max(|v|_1, 1e-12) + 1e-10).
 * Errors: null pointers, bad sizes or bins, an incompatible (ps, ns), a non-finite clipval, B outside
 * [0, 2^24).  B == 0 returns RR_OK. */
int rr_sift_describe(const float* patches, long long B, int ps, int num_ang_bins, int num_spatial_bins, int rootsift,
                     double clipval, float* out, void* stream);
/* rr_describe_keypoints: image -> descriptors in one kernel, one block per keypoint, the patch in
 * LDS: no patch, gradient, histogram or angular plane exists in memory.  It replaces the
 * descriptor half of generate_kpts(..., 'sift') (cirtorch/datasets/localFeatures/utils.py:56-99),
 * i.e. LAFOrienter.forward (orientation.py:122-150) followed by extract_patches_simple and
 * SIFTDescriptor.forward.
 * x [n][c][h][w] float32 or uint8, c = 1, or c = 3 reduced to gray.  The frame of slot (i, k):
 * lafs [n][npts][2][3] when lafs is not NULL, else [[scale, 0, x], [0, scale, y]] with (x, y) =
 * kpts [n][npts][2], which is what rr_select_keypoints writes.  count: NULL or int32 [n]; slots at
 * or past count[i] and slots whose centre is (-1, -1) get an all-zero descriptor, angle 0 and a zero
 * frame.  orient = 1: the upright frame U is make_upright (laf.py:112-134) in float64, rounded to
 * float32 (the frame itself when it comes from scale); the patch of U gives theta by
 * rr_patch_orientation with orient_bins bins, and the frame becomes U . [[cos theta, sin theta],
 * [-sin theta, cos theta]] -- the float32 U that was sampled, turned in float64 and rounded once to
 * float32 -- before the patch is sampled again.  orient = 0 samples the
 * frame as given.  desc [n][npts][num_ang_bins ns^2]; angles (NULL or [n][npts]) and lafs_out (NULL
 * or [n][npts][2][3]) receive theta and the frame that was described.
 * The result is bit-identical to rr_extract_patches (gray = 1 for c = 3) on lafs_out followed by
 * rr_sift_describe, and theta to rr_patch_orientation on the patches of the upright frames.
 * Patches are always sampled from the image itself (pyramid level 0 of
 * extract_patches_from_pyramid, which LAFOrienter calls: the two agree while 2 scale / ps < sqrt 2).
 * The workspace (rr_describe_workspace_bytes) is a formality of 256 bytes today.
 * Errors: those of the entries above, c not 1 or 3, orient not 0 / 1, a scale that is not positive
 * and finite when lafs is NULL, kpts and lafs both NULL, more than 2^24 - 1 slots, a short workspace
 * (RR_ENOSPACE).
 * n npts == 0 returns RR_OK. */
size_t rr_describe_workspace_bytes(int n, int npts, int ps, int num_ang_bins, int num_spatial_bins);
int rr_describe_keypoints(const void* x, int n, int c, int h, int w, int u8, const float* kpts, const int* count, int npts,
                          double scale, const float* lafs, int orient, int orient_bins, int ps, int num_ang_bins,
                          int num_spatial_bins, int rootsift, double clipval, float* desc, float* angles, float* lafs_out,
                          void* workspace, size_t workspace_bytes, void* stream);

/* The patch pyramid (rr_describe.hip): large frames are sampled from a blurred, halved level of the
 * image instead of stepping over full-resolution pixels.  The rules of the four entries above hold:
 * float64 in one fixed order per output, rounded once to float32, no atomic on a floating-point
 * value, a result depends on its own frame and image only, argument errors before anything is
 * enqueued, nothing is read back (levels, sizes and offsets are host arithmetic on (h, w, ps)),
 * graph-capturable.
 *
 * rr_pyrdown is PyrDown.forward (cirtorch/geometry/transform/pyramid.py:161-196) with
 * border_type 'reflect' and align_corners False: the 5 x 5 binomial kernel [1, 4, 6, 4, 1]^2 / 256 on
 * the plane reflect-padded by 2, then F.interpolate(scale_factor=0.5, bilinear), which is the mean
 * of the blurred pixels (2i, 2i+1) x (2j, 2j+1).  The two are one separable pass:
 *   out[i][j] = sum_a sum_b c6[a] c6[b] xpad[2 i + a][2 j + b],  c6 = [1, 5, 10, 10, 5, 1] / 32,
 *   xpad[k] = x[reflect(k - 2)], reflect(-1) = 1, reflect(size) = size - 2
 * along x first, then along y, each sum in ascending tap order.  x [n][c][h][w] float32,
 * out [n][c][h / 2][w / 2] (floor, odd sizes too).  h, w >= 3.  One block per output tile of 32 x 16 (w x h):
 * the input tile and its halo are read once into LDS, the x pass stays in LDS, the output is written
 * once.  Errors: null pointers, bad sizes, h or w < 3, more than 2^31 pixels, more than 2^24 - 1
 * tiles.  n == 0 returns RR_OK.
 *
 * rr_patch_pyramid builds levels 1 .. last_level of extract_patches_from_pyramid
 * (cirtorch/features/laf.py:311-360): level 0 is the image, level l + 1 = pyrdown(level l), of size
 * (h >> l) x (w >> l); last_level is the largest l with min(h_l, w_l) >= ps (the reference's loop
 * condition, laf.py:335), 0 when there is none.  Level 1 reads the image itself: float32, or uint8
 * (float32(v) / 255.0f), and with gray = 1 (c == 3) the pixel (0.299 r + 0.587 g) + 0.114 b of
 * rr_extract_patches; it stores c planes per image (one with gray).  pyr receives the levels back to
 * back, level l as [n][c or 1][h_l][w_l] float32; rr_patch_pyramid_bytes is its size for c stored
 * planes per image (pass 1 for gray) and writes last_level (may be NULL); it returns 0, last_level
 * 0, for arguments out of range.  Errors: those of rr_extract_patches, a null or short buffer
 * (RR_ENOSPACE).  Nothing to build returns RR_OK.
 *
 * rr_extract_patches_pyramid is rr_extract_patches with every frame sampled from its level:
 *   s = sqrt(|(a00 a11 - a10 a01) + 1e-10|),  level = max(0, floor(log2((2 s) / ps) + 0.5))
 * (laf.py:327-329), float64.  On level l >= 1 the frame is renormalised as normalize_laf /
 * denormalize_laf do (laf.py:219-257): the centre becomes (a02 (w_l / w), a12 (h_l / h)), the 2 x 2
 * part is multiplied by min(h_l, w_l) / min(h, w), all float64 and not rounded to float32, and the
 * level's plane is sampled by the rule of rr_extract_patches.  Level 0 gives the bits of
 * rr_extract_patches.  A frame whose level exceeds last_level is sampled from last_level: a
 * deliberate deviation, the reference leaves a zero patch there (constant descriptors that match
 * each other).  levels_out (NULL or int32 [n][npts]) receives the unclamped level (0 for a
 * non-finite frame); beyond_flag (NULL or one device int) is cleared by the call and set to 1 when a
 * frame was clamped.  pyr is what rr_patch_pyramid wrote for the same (x, gray, ps); it may be NULL
 * when last_level is 0.
 *
 * rr_describe_keypoints_pyramid takes the arguments of rr_describe_keypoints, builds the gray
 * pyramid at the (256-byte aligned) start of the workspace (rr_describe_pyramid_workspace_bytes) and describes; every
 * patch, the upright frame's and the described frame's, comes from the level of the frame it is
 * sampled from.  desc is bit-identical to rr_patch_pyramid -> rr_extract_patches_pyramid on lafs_out
 * -> rr_sift_describe, theta to rr_patch_orientation on the pyramid patches of the upright frames,
 * and where every frame is of level 0 the bits are those of rr_describe_keypoints. */
int rr_pyrdown(const float* x, int n, int c, int h, int w, float* out, void* stream);
size_t rr_patch_pyramid_bytes(int n, int c, int h, int w, int ps, int* last_level);
int rr_patch_pyramid(const void* x, int n, int c, int h, int w, int u8, int gray, int ps, float* pyr, size_t pyr_bytes,
                     void* stream);
int rr_extract_patches_pyramid(const void* x, int n, int c, int h, int w, int u8, int gray, const float* pyr, const float* lafs,
                               int npts, int ps, float* out, int* levels_out, int* beyond_flag, void* stream);
size_t rr_describe_pyramid_workspace_bytes(int n, int c, int h, int w, int npts, int ps, int num_ang_bins, int num_spatial_bins);
int rr_describe_keypoints_pyramid(const void* x, int n, int c, int h, int w, int u8, const float* kpts, const int* count,
                                  int npts, double scale, const float* lafs, int orient, int orient_bins, int ps,
                                  int num_ang_bins, int num_spatial_bins, int rootsift, double clipval, float* desc,
                                  float* angles, float* lafs_out, void* workspace, size_t workspace_bytes, void* stream);

/* Affine shape (rr_describe.hip): the second-moment matrix of a patch's gradients, the frame of an
 * ellipse, and the two fused per keypoint -- the stage of ScaleSpaceDetector between detection and
 * orientation (cirtorch/features/affine_shape.py, whose kornia helpers are laf.py's).  The rules of
 * the describe entries hold: float64 in one fixed order per output, rounded once to float32, no
 * atomic on a floating-point value, a result depends on its own patch or frame and image only,
 * argument errors before anything is enqueued, nothing is read back (graph-capturable), one block of
 * 256 threads per patch or slot (rr_ellipse_to_laf: per 256 ellipses), at most 2^24 - 1 patches,
 * ellipses or slots, 8 <= ps <= 64.
 *
 * rr_patch_affine_shape replaces PatchAffineShapeEstimator.forward (affine_shape.py:36-69).
 * patches [B][ps][ps] float32, out [B][3] float32 = (a, b, c).  Per pixel, on clamped patch
 * coordinates, dx and dy are the Sobel pair / 8 of rr_patch_orientation and
 *   gx = dx G(y, x),  gy = dy G(y, x)
 * with G the float32-valued window of rr_sift_describe (get_gaussian_kernel2d((ps, ps), (sigma,
 * sigma), True), sigma = ps / sqrt 2: the same table).  The weight is on the gradients, so it enters
 * the moments squared, as in the reference.
 *   a = mean(gx^2),  b = mean(gx gy),  c = mean(gy^2)
 * Each sum: thread t of the 256 adds its pixels t, t + 256, ... (row-major) in ascending order; the
 * 256 partial sums are added by an xor butterfly over each wave of 64 (offsets 32, 16, ..., 1) and
 * the four wave sums as ((w0 + w1) + w2) + w3; then / ps^2.  The degenerate rule comes BEFORE the
 * normalisation: if [a < eps] + [b < eps] + [c < eps] >= 2 (a negative b counts) the shape is
 * (1, 0, 1).  Then (a, b, c) / max(a, b, c).  The reference's default eps is 1e-10; G is of order
 * 1 / ps^2, so raw moments of a [0, 1] image at ps 32 are 1e-9 .. 1e-7 and the threshold is live.
 * Errors: null pointers, a bad ps, a non-finite eps, B outside [0, 2^24).  B == 0 returns RR_OK.
 *
 * rr_ellipse_to_laf replaces ellipse_to_laf (cirtorch/features/laf.py:137-167).  ells [B][5] float32
 * = (x, y, a, b, c), lafs [B][2][3] float32:
 *   a11 = sqrt|a|,  a22 = sqrt|c|,  a21 = b / max(a11 + a22, 1e-9)
 *   lafs = [[1 / a11, 0, x], [0 - a21 / (a11 a22), 1 / a22, y]]
 * the closed form of the reference's inverse of [[a11, 0], [a21, a22]].
 * Errors: null pointers, B outside [0, 2^24).  B == 0 returns RR_OK.
 *
 * rr_laf_affine_shape replaces LAFAffineShapeEstimator.forward (affine_shape.py:91-119) by the
 * pyramid build and one kernel, one block per slot, the patch in LDS: no patch, gradient or ellipse
 * exists in memory.  x, count, lafs [n][npts][2][3] and the workspace
 * (rr_laf_affine_shape_workspace_bytes; the gray pyramid at its 256-byte aligned start) are those of
 * rr_describe_keypoints_pyramid.  Per slot: U = make_upright(frame) in float64 rounded to float32;
 * the patch of U from U's level by the rule of rr_extract_patches_pyramid (a frame past the last
 * level from the last level: the reference's zero patch would give a circle there), rounded to
 * float32; (a, b, c) by rr_patch_affine_shape, rounded to float32; E = rr_ellipse_to_laf(x, y, a, b,
 * c), rounded to float32; s0 = sqrt|det + 1e-10| of the INPUT frame's 2 x 2 part and s1 of E's; the
 * output's 2 x 2 part is E (s0 / s1) and its centre the input's, bit for bit.  Slots at or past
 * count[i], slots whose centre is (-1, -1) and frames with a non-finite entry get an all-zero frame.
 * lafs_out [n][npts][2][3] may be lafs.  The result is bit-identical to rr_patch_pyramid ->
 * rr_extract_patches_pyramid on the upright frames -> rr_patch_affine_shape -> rr_ellipse_to_laf ->
 * that rescaling in float64.
 * Errors: those of the entries above, c not 1 or 3, a non-finite eps, more than 2^24 - 1 slots, a
 * short workspace (RR_ENOSPACE).  n npts == 0 returns RR_OK. */
int rr_patch_affine_shape(const float* patches, long long B, int ps, double eps, float* out, void* stream);
int rr_ellipse_to_laf(const float* ells, long long B, float* lafs, void* stream);
size_t rr_laf_affine_shape_workspace_bytes(int n, int c, int h, int w, int npts, int ps);
int rr_laf_affine_shape(const void* x, int n, int c, int h, int w, int u8, const float* lafs, const int* count, int npts, int ps,
                        double eps, float* lafs_out, void* workspace, size_t workspace_bytes, void* stream);

/* Learned patch descriptors (rr_patchnet.hip): HardNet and SOSNet on 32 x 32 patches in eval mode.
 * Replaces HardNet.forward / HardNet._normalize_input of cirtorch/features/hardnet.py:12-76 and
 * SOSNet.forward of cirtorch/features/sosnet.py:9-58 (nn.Conv2d, nn.BatchNorm2d(affine=False),
 * nn.ReLU, nn.InstanceNorm2d, nn.LocalResponseNorm, F.normalize; nn.Dropout is the identity).
 *
 * The shared trunk is seven bias-free convolutions, each followed by BatchNorm in eval mode,
 * y = (x - running_mean) / sqrt(running_var + 1e-5), and, layers 1 .. 6, by ReLU:
 *   layer   1        2         3          4         5          6           7
 *   cin     1        32        32         64        64         128         128
 *   cout    32       32        64         64        128        128         128
 *   kernel  3x3 p1   3x3 p1    3x3 p1 s2  3x3 p1    3x3 p1 s2  3x3 p1      8x8 p0
 *   map     32x32    32x32     16x16      16x16     8x8        8x8         1x1
 * The input of layer 1 is the patch normalised by its own statistics (mean m over its 1024 pixels):
 *   RR_PATCHNET_HARDNET  (x - m) / (sd + 1e-6),  sd = sqrt(sum (x - m)^2 / 1023)  (unbiased)
 *   RR_PATCHNET_SOSNET   (x - m) / sqrt(sum (x - m)^2 / 1024 + 1e-5)              (InstanceNorm2d)
 * and the descriptor is, with f the 128 values after layer 7's BatchNorm:
 *   RR_PATCHNET_HARDNET  f / max(|f|_2, 1e-12)                                    (F.normalize)
 *   RR_PATCHNET_SOSNET   v / |v|_2 with v = f + 1e-10, no eps.  That is LocalResponseNorm(256,
 *                        alpha=256, beta=0.5, k=0) of v: over 128 channels the window of 256 covers
 *                        every channel, and alpha times the averaged sum is the plain sum of squares.
 *
 * Precision: fp16 operands, float32 accumulation (v_mfma_f32_16x16x32_f16).  Where a value is rounded:
 *  - rr_patchnet_pack rounds every weight once, float32 -> fp16 (nearest even), as given: BatchNorm is
 *    not folded into the weights.  Per channel scale = float32(1 / sqrt(float64(var) + 1e-5)) and
 *    shift = float32(-float64(mean) * (1 / sqrt(float64(var) + 1e-5))).
 *  - the patch statistics are float64 sums in one fixed order (two pixels per thread, the xor
 *    butterfly of a wave, the eight waves in ascending order); the normalised pixel is the float64
 *    quotient rounded once to fp16.
 *  - a layer's output pixel is float32 acc over K in the fixed order (tap ascending, then 32-channel
 *    chunk ascending; layer 1: taps ascending, fmaf), then fmaf(acc, scale, shift) in float32, then
 *    max(., 0), rounded once to fp16.  Layers 1 .. 6 do this.
 *  - layer 7 accumulates in float32 over K = 8192 in the order of the map ((y, x) ascending, then
 *    channel) in eight slices of 1024 (one per wave), each from zero; the slices are added in
 *    ascending order.  Its BatchNorm is fmaf(acc, scale, shift) in float32, the + 1e-10 (SOSNet), the sum of
 *    squares (channels 16 n + c over n ascending, then the xor butterfly over c), the square root
 *    and the quotient are float32.  The descriptor is float32.
 * A descriptor depends on its own patch and the weights only: not on B, on the patch's position in
 * the batch, on the chunk length or on the run (no atomics, fixed summation order).
 * Non-finite input: a patch with a NaN or an infinite pixel has non-finite statistics, so every
 * normalised pixel is NaN and the reference modules return NaN in every entry.  So do these entries:
 * the trunk sees it in the float64 sum of the pixels (finite for 1024 finite floats) and stores NaN
 * (0x7E00) in every entry of the map in place of layer 6's outputs, because the max(., 0) of the
 * layers drops a NaN; the head carries the NaN to all 128 entries.  No other patch of the batch is affected (a row of the head's GEMM is one
 * patch).  A NaN descriptor matches nothing in rr_match_pairs.
 *
 * rr_patchnet_packed_bytes / rr_patchnet_pack: the seven weights [cout][cin][kh][kw] float32 and the
 * seven running_mean / running_var [cout] float32 -- weights, means, vars are HOST arrays of 7 DEVICE
 * pointers, layer 1 first -- into one device blob `packed` (16-byte aligned, at least
 * rr_patchnet_packed_bytes() = 2,673,920 B): the fp16 weights of layers 1 .. 7, layer 1 as [tap][cout],
 * layers 2 .. 7 as [tap * cin / 32 + chunk][cout][32] (layer 7's taps are the 64 pixels of the map, so
 * its K order is the order in which the trunk writes the map), then float32 scale[576] and shift[576].
 *
 * rr_patchnet_trunk: patches [B][32][32] float32 (8-byte aligned) -> map [B][8][8][128] fp16, the
 * output of layer 6 (16-byte aligned).  One launch, one workgroup per patch; the normalised patch
 * and the maps of layers 1 .. 5 stay in LDS (two regions of one zero-padded 34 x 34 x 32 fp16 map,
 * 147,968 B; later maps reuse them), layer 1 is vector work and layers 2 .. 6 are implicit GEMMs of
 * M = pixels, N = cout, K = 9 cin whose weights stream from the L2.
 * rr_patchnet_head: map -> desc [B][128] float32: layer 7 as a [B][8192] x [8192][128] GEMM, a workgroup
 * per 16 patches (its 8 waves split K), its BatchNorm and the descriptor normalisation; the 2 MiB of
 * weights are read once per 16 patches, from the L2.
 * rr_patchnet_describe: the two in chunks of RR_TUNE_PATCHNET_CHUNK patches (trunk on a chunk, then
 * head on that chunk), so the workspace -- the maps of one chunk, 16 KiB a patch -- is bounded
 * whatever B is; the result has the bits of the chain of the two entries.  workspace: at least
 * rr_patchnet_workspace_bytes(B), which reads the chunk length in force when it is called.
 * Errors, before anything is enqueued: B < 0, an unknown variant, null pointers, a misaligned
 * pointer (RR_EINVAL), a short packed buffer or workspace (RR_ENOSPACE).  B == 0 returns RR_OK and
 * launches nothing.  Nothing waits for the host (graph-capturable).
 * Not built: an fp32 or bf16 mode of the net, HardNet8, AffNet, OriNet, training (batch statistics,
 * dropout, a backward pass), pretrained files, and patch sampling fused into the trunk. */
#define RR_PATCHNET_HARDNET 0
#define RR_PATCHNET_SOSNET 1
size_t rr_patchnet_packed_bytes(void);
int rr_patchnet_pack(const float* const* weights, const float* const* means, const float* const* vars, void* packed,
                     size_t packed_bytes, void* stream);
size_t rr_patchnet_workspace_bytes(long long B);
int rr_patchnet_trunk(const float* patches, long long B, int variant, const void* packed, void* map, void* stream);
int rr_patchnet_head(const void* map, long long B, int variant, const void* packed, float* desc, void* stream);
int rr_patchnet_describe(const float* patches, long long B, int variant, const void* packed, float* desc, void* workspace,
                         size_t workspace_bytes, void* stream);

/* Full ranking for any database size: out_idx[q][r] = the r-th database row of
 * query q by (float64 score desc, index asc) — np.argsort(-np.dot(vecs.T, qvecs),
 * axis=0) of scripts/test.py:247-248 as [nq][n] (rr_knn_topk ranks k <= 8192).
 * The float64 score is rr_knn_topk's re-score (same summation order), so the
 * first k ranks equal a top-k search.  db_f32 [n][d], q_f32 [nq][d] float32,
 * d a multiple of 256 (zero-pad); workspace >= rr_rank_workspace_bytes
 * (24 B x nq x n + histograms). */
size_t rr_rank_workspace_bytes(long long n, int nq);
int rr_rank_full(const float* db_f32, long long n, const float* q_f32, int nq, int d, long long* out_idx,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------ tuning */
/* Engine tuning knobs (process-wide; for benchmarking / autotuning tools).  One table
 * (csrc/rr_tuning.h) holds every key's state and default.  rr_set_tuning stores a value
 * after the key's normalisation (noted below; values are not range-checked otherwise) and
 * rr_get_tuning reads it back in the same encoding, so set(key, get(key)) changes nothing.
 * Neither makes a HIP call.  Four keys are seeded from the environment when the library
 * loads (first character of the variable); rr_set_tuning then overrides the seed, except
 * that RR_KNN_FUSED=0 pins RR_TUNE_KNN_FUSED to 0 for the process.
 *   RR_TUNE_GEMM_CONFIG  0 = automatic tile choice (default), 1 = 128x128, 2 = 64x256,
 *                        3 = 256x128 (8 waves), 4 = 256x256 (8 waves), 5 = 256x64,
 *                        7 / 8 = 256x128 / 128x256 (8 waves, 3-stage ring)
 *                        6 = A-stationary (weights resident in LDS) where eligible
 *   RR_TUNE_GEMM_STAGES  2 (default) or 3 LDS stages (3: one resident block per CU); any other
 *                        value is stored as 2.  Seed: RR_GEMM_STAGES ("3": 3, else 2)
 *   RR_TUNE_GEMM_WIDE    0/1 allow the 8-wave tiles in the automatic choice (default 1; stored
 *                        as value != 0).  Seed: RR_GEMM_WIDE ("0": 0, else 1)
 *   RR_TUNE_GEMM_ASTAT   0/1 allow the A-stationary tiles in the automatic choice (default 0;
 *                        stored as value != 0)
 *   RR_TUNE_GEMM_XCD_MAP 0/1 XCD-contiguous tile order (default 0; stored as value != 0)
 *   RR_TUNE_STREAM_1X1   0/1 weight-stationary streaming kernel for the
 *                        HBM-bound bf16 1x1 convs (default 1); 2 / 3 also route the
 *                        residual 512->2048 / 256->1024 1x1s to the 8-phase GEMM (A/B only)
 *   RR_TUNE_CONV3X3      0 off, 1 auto (default): direct 3x3 kernel with LDS
 *                        halo patches for the bf16 stride-1 3x3 convs;
 *                        2 / 3 prefer its 8x32 / 4x32 pixel tiles, 4 / 6 use
 *                        1x8 / 1x4 waves for the c_in = 64 A-stationary form,
 *                        7 a 3-stage weight ring, 8 256-channel x 6x32 tiles,
 *                        9 the c_in = c_out = 64 form with the weights in VGPRs
 *                        (k_c3w64; also what 1 picks for that shape)
 *   RR_TUNE_GRID_CUS     cap on the CUs one persistent launch spreads over
 *                        (0 = all, the default; e.g. half the chip for two concurrent
 *                        streams); a negative value is an error
 *   RR_TUNE_GEMM8        0 off, 1 auto, 2 forced: the 8-phase staggered 256x256 GEMM for eligible
 *                        16-bit 1x1 / tap-uniform convs and score GEMMs (default 1: persistent
 *                        blocks for the kNN score GEMM, one block per tile for convs; 2: also
 *                        persistent everywhere; | 4: one block per tile everywhere; | 8: no
 *                        k_gemm8h / k_gemm8s; | 16: no k_gemm8a; | 32: k_gemm8h instead of the streaming
 *                        k_gemm8s for the <= 128-query score GEMM; | 64: conv tiles walked
 *                        channel-major instead of pixel-major; | 128: k_gemm8a one block per
 *                        tile instead of persistent blocks; | 512: the short-K non-residual
 *                        1x1 convs one block per tile instead of persistent blocks).  Stored as
 *                        mode | switches: a negative value as 0, mode 3 as 2, other bits
 *                        dropped.  Seed: RR_GEMM8 ("0": 0, else 1)
 *   RR_TUNE_KNN_FUSED    0/1 kNN screening in the score-GEMM epilogue after a 4-chunk
 *                        prefix (default 1; stored as value != 0); 0 = every chunk through the
 *                        score slab.  Seed: RR_KNN_FUSED ("0": 0 for the whole process, else 1)
 *   RR_TUNE_CONV3_PIPE   1 (default): the direct 3x3 kernel reads the operands of its next
 *                        half-step while the current one's MFMAs issue; 0: compiler schedule
 *   RR_TUNE_STEM         2 (default): fused stem v3 (pixels x channels MFMA, lane-local
 *                        pooling; 3 / 4: patch fill in 2 / 5 parts; 6: the 3-part fill without
 *                        border selects where a pixel pair lies inside the image); 5: v4
 *                        (space-to-depth K: same value per tap as v3, another f32 summation
 *                        order); 1: v2 (pools the raw conv before BN/activation, exact by
 *                        monotonicity); 0: v1 (BN/activation on every stem pixel).  Odd stem
 *                        maps always take v1.
 *   RR_TUNE_STREAM_XCD   1 (default): the streaming 1x1's channel-slice blocks of one pixel
 *                        strip run on one XCD (the strip's input is re-read from that L2)
 *   RR_TUNE_CONV3S       1 (default): the staggered two-wave-group direct 3x3 (persistent,
 *                        chunk-double-buffered halo patches) for the stride-1 3x3s with
 *                        c_out = 128 under RR_TUNE_CONV3X3 = 1; 2: also c_in = c_out = 64; 0 off
 *   RR_TUNE_WRES         1: the residual 256 -> 1024 / 512 -> 2048 1x1s (bottleneck conv3 of
 *                        mod4 / mod5) on the weight-stationary k_wres1x1 (weights in VGPRs,
 *                        activation + residual tiles by LDS-DMA); 2 (default): also the non-residual
 *                        K = 256 / 512 1x1s (projections, strided or not; mod4 block-1 conv1);
 *                        0: the streaming 1x1 / 8-phase GEMM
 *   RR_TUNE_PAIR_MID     1 (default): the 128/512 boundary of rr_conv1x1_pair on 32-pixel tiles
 *                        with a 4-slot residual ring (3 tiles ahead); 0: 64-pixel tiles, one ahead
 *                        (same results bit for bit)
 *   RR_TUNE_WRES_RING    1 (default): the non-residual k_wres1x1 forms (projections, mod4 block-1
 *                        conv1) keep 5 (K = 256) / 3 (K = 512) activation tiles in flight; 0: two
 *                        (same results bit for bit)
 *
 * Size keys (enum rr_tune_size_key, from RR_TUNE_SIZE_BASE): a length, not a kernel choice; a value
 * below 1 is an error.  A workspace-size function reads the value in force when it is called.
 *   RR_TUNE_PATCHNET_CHUNK  patches per trunk + head pair of rr_patchnet_describe (default 16384:
 *                        256 MiB of maps); the result does not depend on it
 *
 * Environment variables without a key (A/B switches, read where they apply):
 *   RR_GEMM_PRIO=1       raised wave priority for the second half of k_igemm's waves
 *   RR_GEMM8S_R=3|6      K-steps in flight per wave in k_gemm8s (default 4)
 *   RR_GEMM_V1=1         the first-generation GEMM engine instead of the LDS-DMA engine
 *   RR_KNN_SLAB_MB=n     kNN score-slab budget per GEMM pass, 16..1024 MiB (default 512)
 *   RR_KNN_PREFIX=n      kNN chunks through the slab before the fused screen (default 4)
 *   RR_KNN_TAU_MEMSET=1  reset the kNN running threshold by hipMemsetAsync, not a kernel
 *   RR_KNN_CUT=0         no certified re-score cut in the kNN candidate select
 *   RR_KNN_FSEL=0        the unstaged final kNN select */
enum rr_tune_key { RR_TUNE_GEMM_CONFIG = 0, RR_TUNE_GEMM_STAGES = 1, RR_TUNE_GEMM_WIDE = 2,
                   RR_TUNE_GEMM_ASTAT = 3, RR_TUNE_GEMM_XCD_MAP = 4, RR_TUNE_STREAM_1X1 = 5,
                   RR_TUNE_CONV3X3 = 6, RR_TUNE_GRID_CUS = 7, RR_TUNE_GEMM8 = 8,
                   RR_TUNE_KNN_FUSED = 9, RR_TUNE_CONV3_PIPE = 10,
                   RR_TUNE_STEM = 11, RR_TUNE_STREAM_XCD = 12, RR_TUNE_CONV3S = 13,
                   RR_TUNE_WRES = 14, RR_TUNE_PAIR_MID = 15, RR_TUNE_WRES_RING = 16 };
enum rr_tune_size_key { RR_TUNE_SIZE_BASE = 32, RR_TUNE_PATCHNET_CHUNK = 32 };
int rr_set_tuning(int key, int value);
int rr_get_tuning(int key, int* value);

/* What the last fused-conv entry on this thread launched (for tests: the kernel a shape
 * dispatches to and its persistent grid are otherwise arithmetic nobody can observe).
 * Host-only and thread-local: one struct copy per launch, nothing on the device.
 * rr_conv2d_fused clears the record on entry, so a conv that runs on the tiled engine or the
 * 8-phase GEMM reads back with an empty kernel; the persistent kernels (k_wres1x1,
 * k_stream1x1, k_stream_pair, k_pair_mid, k_pair_mid_ring, k_c3pair, k_conv3x3, k_c3w64,
 * k_c3s) record their name, template variant, grid and block size, output-channel slices
 * (0 where the kernel has none), whether the XCD tile map is on, and how many launches
 * (image or pixel chunks) the entry made.  RR_EINVAL if nothing was recorded on this thread. */
typedef struct { char kernel[32]; char variant[48]; unsigned grid, block; int nslices, xmap, launches; } rr_launch_info;
int rr_last_launch(rr_launch_info* out);

/* ----------------------------------------------------------- data helpers */
/* Counter-based N(0,1) rows, each L2-normalised: row i of the global matrix
 * depends only on (seed, i0 + i), so shards generate identical rows. */
int rr_fill_unit_rows(float* out, long long rows, int d, unsigned long long seed,
                      long long row0, void* stream);
/* int8 screening copy of float32 rows for rr_knn_topk(dtype RR_I8): y = clamp(rint(x * 127 / amax),
 * -127, 127) with amax = max |x| over all n elements, reduced on the device into amax_dev (one float of
 * caller scratch; no host synchronisation).  The screening scores are then exact int32 dot products of
 * the quantised rows (v_mfma_i32_16x16x64_i8, twice the bf16 MFMA rate, half the bf16 bytes); the final
 * top-k is the exact float64 re-score of the candidates, as for every screening dtype. */
int rr_quantize_i8(const float* x, long long n, void* y, float* amax_dev, void* stream);
/* Per-row int8 copy (queries): amax_rows[r] = max |x_r|, y_r = clamp(rint(x_r * 127 / amax_rows[r]),
 * -127, 127); x [rows][d] float32, d % 4 == 0.  A query's screened candidates then do not depend on
 * the other queries of its batch. */
int rr_quantize_i8_rows(const float* x, int rows, int d, void* y, float* amax_rows, void* stream);
/* float32 -> bf16 (round to nearest even). */
int rr_cast_f32_bf16(const float* x, void* y, long long n, void* stream);
/* float32 -> fp16 (IEEE binary16, round to nearest even). */
int rr_cast_f32_f16(const float* x, void* y, long long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RR_H_ */
