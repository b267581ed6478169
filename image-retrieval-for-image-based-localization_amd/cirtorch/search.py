"""GPU matching: the replacement for the reference's host-side rank
``scores = np.dot(vecs.T, qvecs); ranks = np.argsort(-scores, axis=0)``
(``scripts/test.py:247-248``, ``scripts/train_globalF.py:733-734``).

* ``knn(vecs, qvecs, k)``  -> first k ranks (k x Q, int64) and their scores,
  exactly ordered by (score desc, index asc); scores re-computed in float64.
* ``rank(vecs, qvecs)``     -> full ranks (N x Q) for mAP evaluation, any N.
* ``KnnIndex``              -> a resident database (float32 rows + optional
  bf16 or fp16 screening copy) queried many times.
* ``ShardedIndex``          -> database rows split over the ranks of a
  torch.distributed group (RCCL on ROCm), per-shard top-k, all-gather of the
  (score, index) lists, on-GPU merge — bit-identical to the 1-GPU result.
* ``match_pairs``           -> local-descriptor matching of P pairs in one launch
  (nn / mnn / snn / smnn of ``cirtorch/features/matching.py``), no host sync.
* ``detect_keypoints``      -> the best N corners / blobs of every image of a batch (response,
  non-maxima suppression and top-N selection on the device), no host sync.
* ``describe_keypoints``    -> SIFT / RootSIFT descriptors of those keypoints straight from the image
  (patch, optional dominant orientation and descriptor in one kernel), no host sync.

Layouts: the reference keeps descriptors as D x N columns; the engine reads
row-major [N][D].  ``vecs.t()`` of a D x N column matrix produced by
``globalHead`` is already a contiguous [N][D] view (no copy).
"""

import torch
import torch.distributed as dist

from . import _ops

# screening precision of the score GEMM (the final top-k is always the exact float64
# re-score): int8 = database rows quantised with one scale per tensor, queries with one
# per row, exact int32 dot products on v_mfma_i32_16x16x64_i8 (twice the bf16 rate, half
# the bytes).  Certificates (verify): fp16 / bf16 / fp32 from the rounding error bound,
# int8 from the quantisation residual bound (~0.02 at D = 2048: on dense random data most
# int8 queries stay uncertified and are re-searched, so fp16 is the certified default)
_PREC = {"fp32": torch.float32, "float32": torch.float32, "bf16": torch.bfloat16, "bfloat16": torch.bfloat16,
         "fp16": torch.float16, "float16": torch.float16, "int8": torch.int8}


def _rows(cols):
    """D x N column matrix (torch or numpy) -> contiguous float32 [N][D] on GPU."""
    if not torch.is_tensor(cols):
        cols = torch.from_numpy(cols)
    rows = cols.t()
    if not rows.is_cuda:
        rows = rows.cuda()
    return rows.float().contiguous()


def _padded_dim(d, dtype):
    """The engine's score GEMM takes power-of-two D >= 32 (>= 64 for fp16,
    >= 256 for int8 screening); other D are zero-padded, which changes no dot
    product."""
    p = 64 if dtype == torch.float16 else 256 if dtype == torch.int8 else 32
    while p < d:
        p <<= 1
    return p


def _pad_cols(x, d_pad):
    if x.shape[1] == d_pad:
        return x
    return torch.nn.functional.pad(x, (0, d_pad - x.shape[1])).contiguous()


class KnnIndex:
    def __init__(self, db_rows, precision="fp32", cand=0, idx_offset=0):
        """db_rows: [N, D] float32 on the GPU (kept by reference, not copied,
        when D is a power of two >= 32; zero-padded otherwise)."""
        self.dtype = _PREC[precision]
        self.dim = db_rows.shape[1]
        self.d_pad = _padded_dim(self.dim, self.dtype)
        self.db32 = _pad_cols(db_rows.float().contiguous(), self.d_pad)
        self.db_amax = None   # int8: the database's quantisation scale (max |x|), kept for the certificate
        if self.dtype == torch.int8 and self.db32.shape[0]:
            self.db, self.db_amax = _ops.quantize_i8(self.db32, with_scale=True)
        else:
            self.db = _ops.cast_screen(self.db32, self.dtype) if self.db32.shape[0] else self.db32.to(self.dtype)
        self.cand = cand
        self.idx_offset = idx_offset
        self._ws = {}   # scratch per stream: searches on different streams never share a slab
        # the certificate's max row norm, read once here so that no search (and no
        # profile of one) pays for the norm pass over the database
        self._norm_max = float(self.db32.norm(dim=1).max().item()) if self.ntotal else 0.0

    @property
    def ntotal(self):
        return self.db32.shape[0]

    def _workspace(self, need, device):
        """Scratch of the current stream.  A buffer is only ever used by the
        stream it was allocated on, so concurrent searches of one index on two
        streams do not race; a replaced buffer is freed in that stream's order."""
        stream = torch.cuda.current_stream(device)
        ws = self._ws.get(stream.cuda_stream)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=device)
            self._ws[stream.cuda_stream] = ws
        return ws

    def norm_max(self):
        """largest database row norm (computed when the index is built)"""
        return self._norm_max

    def _screen_queries(self, q32):
        """float32 query rows -> (screening copy, int8 per-row scales or None)"""
        if self.dtype == torch.int8:
            return _ops.quantize_i8(q32, per_row=True, with_scale=True)
        return _ops.cast_screen(q32, self.dtype), None

    def search(self, q_rows, k, verify=True):
        """q_rows [Q, D] -> (scores float64 [Q, k], idx int64 [Q, k]) on the current stream.
        An empty shard (ntotal == 0) returns k (-inf, -1) entries per query, which
        the sharded merge drops.

        verify=True (the default: the reference ranks exactly, scripts/test.py:247-248)
        certifies the screening margin of every query (the rows left out are provably
        below the returned k-th score given the screening dtype's error bound) and
        re-searches uncertain queries — clusters of near-duplicates tighter than the
        screening error — with float32 screening and more candidates; this costs one
        device->host read per search, so it cannot be captured in a graph.

        verify=False is the explicit opt-out: the screened candidate pool re-ranked in
        float64, no certificate (exact unless near-ties straddle the screening cut);
        graph-capturable.

        verify="deferred" returns (scores, idx, pending): the same certificate,
        copied to pinned host memory without a synchronisation; pending.resolve()
        (later, e.g. once the next batch's work is queued) waits for it and
        re-searches the uncertain queries in place, returning how many there were."""
        if q_rows.shape[1] != self.dim:
            raise RuntimeError("KnnIndex.search: queries have D=%d, the database D=%d" % (q_rows.shape[1], self.dim))
        q32 = _pad_cols(q_rows.float().contiguous(), self.d_pad)
        if verify is True and q32.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("KnnIndex.search: verify=True reads the certificate back and cannot run "
                               "inside a graph capture; capture with verify=False (or 'deferred' outside)")
        if self.ntotal == 0 or q32.shape[0] == 0:
            s = torch.full((q32.shape[0], k), float("-inf"), dtype=torch.float64, device=q32.device)
            i = torch.full((q32.shape[0], k), -1, dtype=torch.int64, device=q32.device)
            return (s, i, Pending.done()) if verify == "deferred" else (s, i)
        if verify:
            s, i, unc = self.search_checked(q32, k)
            pend = Pending(unc, lambda bad: self._research(q32, bad, k), s, i)
            if verify == "deferred":
                return s, i, pend
            pend.resolve()
            return s, i
        q, _ = self._screen_queries(q32)
        need = _ops.knn_workspace_bytes(self.ntotal, q.shape[0], q.shape[1], k, self.cand, self.dtype)
        return _ops.knn_topk(self.db, self.db32, q, q32, k, cand=self.cand, idx_offset=self.idx_offset,
                             workspace=self._workspace(need, q.device))

    def search_checked(self, q_rows, k):
        """queries [Q, D] -> (scores, idx, int32 [Q] uncertain flags), no synchronisation"""
        q32 = _pad_cols(q_rows.float().contiguous(), self.d_pad)
        q, qa = self._screen_queries(q32)
        need = _ops.knn_workspace_bytes(self.ntotal, q.shape[0], q.shape[1], k, self.cand, self.dtype)
        return _ops.knn_topk(self.db, self.db32, q, q32, k, cand=self.cand, idx_offset=self.idx_offset,
                             workspace=self._workspace(need, q.device), db_norm_max=self.norm_max(),
                             i8_scales=None if qa is None else (qa, self.db_amax))

    def _research(self, q32, bad, k):
        """exact top-k of the queries q32[bad] (int64 [n] on the device): float32
        screening (error ~d 2^-24), then the largest candidate pool"""
        s, i = None, None
        sel = torch.arange(bad.numel(), device=bad.device)
        for cand in (0, min(8192, max(1024, 8 * k))):
            qb = q32[bad[sel]].contiguous()
            need = _ops.knn_workspace_bytes(self.ntotal, qb.shape[0], qb.shape[1], k, cand, torch.float32)
            s2, i2, u2 = _ops.knn_topk(self.db32, self.db32, qb, qb, k, cand=cand, idx_offset=self.idx_offset,
                                       workspace=self._workspace(need, qb.device), db_norm_max=self.norm_max())
            if s is None:
                s, i = s2, i2
            else:
                s[sel], i[sel] = s2, i2
            keep = torch.nonzero(u2).flatten()
            if keep.numel() == 0:
                return s, i
            sel = sel[keep]
        # more than 8192 rows within the float32 screening error of the k-th score
        # (exact duplicates of it, say): the full exact ranking of those queries
        s[sel], i[sel] = self._exact_by_rank(q32[bad[sel]].contiguous(), k)
        return s, i

    def _exact_by_rank(self, q32, k):
        """top-k of every row's float64 score by (score desc, index asc) -- rr_rank_full
        (the k_rescore summation order, stable radix sort), no screening at all; the
        scores are the same rows re-scored by the top-k pipeline over just those rows
        (gathered in index order, so its tie order is the global one)"""
        n, kk = self.ntotal, min(k, self.ntotal)
        d256 = (self.d_pad + 255) // 256 * 256
        db = _pad_cols(self.db32, d256)
        q = _pad_cols(q32, d256)
        per = max(1, min(65535, RANK_BYTES_MAX // (32 * n)))
        top = torch.cat([_ops.rank_full(db, q[j:j + per].contiguous())[:, :kk] for j in range(0, q.shape[0], per)])
        s = torch.full((q32.shape[0], k), float("-inf"), dtype=torch.float64, device=q32.device)
        i = torch.full((q32.shape[0], k), -1, dtype=torch.int64, device=q32.device)
        for r in range(q32.shape[0]):
            rows = torch.sort(top[r]).values
            sub = KnnIndex(self.db32[rows], "fp32", cand=max(kk, 32))
            sr, ir = sub.search(q32[r:r + 1], kk, verify=False)   # every row is a candidate
            s[r, :kk], i[r, :kk] = sr[0], rows[ir[0]] + self.idx_offset
        return s, i


class Pending:
    """The certificate of a search, read back later: the int32 flags are copied to
    pinned host memory on the search's stream and an event is recorded, so the
    caller is not synchronised until resolve().  resolve() waits for the event and,
    for the flagged queries, calls research(bad) -> (scores, idx) and writes them
    into the returned rows; it returns the number of re-searched queries."""

    def __init__(self, unc, research, s, i):
        self.s, self.i, self.research, self.unc = s, i, research, unc
        self.ev = None
        if unc.is_cuda:
            self.host = torch.empty(unc.shape, dtype=unc.dtype, pin_memory=True)
            self.host.copy_(unc, non_blocking=True)
            self.ev = torch.cuda.Event()
            self.ev.record()
        else:
            self.host = unc.clone()
        self.count = None

    @classmethod
    def done(cls):
        p = cls.__new__(cls)
        p.count = 0
        return p

    def resolve(self):
        if self.count is not None:
            return self.count
        if self.ev is not None:
            self.ev.synchronize()
        bad = torch.nonzero(self.host).flatten()
        self.count = int(bad.numel())
        if self.count:
            bad = bad.to(self.s.device)
            s2, i2 = self.research(bad)
            self.s[bad], self.i[bad] = s2, i2
        return self.count


def knn(vecs, qvecs, k, precision="fp32", cand=0, verify=True):
    """vecs D x N, qvecs D x Q (reference layout) -> (ranks k x Q int64, scores k x Q float64),
    certified exact by default (verify=False: the uncertified screen, see KnnIndex.search)."""
    db = _rows(vecs)
    q = _rows(qvecs)
    s, i = KnnIndex(db, precision, cand).search(q, k, verify=verify)
    return i.t(), s.t()


RANK_BYTES_MAX = 2 << 30  # device scratch + output of one rr_rank_full call
RANK_KNN_MAX = 8192  # up to this size the top-k pipeline (LDS bitonic sort of all rows) ranks in one pass


def rank(vecs, qvecs, precision="fp32", method="auto"):
    """Full ranking, the GPU equivalent of ``np.argsort(-np.dot(vecs.T, qvecs), axis=0)``:
    N x Q int64 by (score desc, index asc) on the float64 re-score.  N <= 8192: the
    top-k pipeline with k = N; larger N (revisited datasets with distractors):
    rr_rank_full (float64 scores + a stable radix sort), identical order."""
    n = vecs.shape[1]
    if method == "knn" or (method == "auto" and n <= RANK_KNN_MAX):
        # cand = n: every row is re-scored in float64, nothing is screened out to certify
        ranks, _ = knn(vecs, qvecs, n, precision=precision, cand=n, verify=False)
        return ranks
    db, q = _rows(vecs), _rows(qvecs)
    d_pad = (db.shape[1] + 255) // 256 * 256
    db, q = _pad_cols(db, d_pad), _pad_cols(q, d_pad)
    # ~32 B of scratch + output per (query, row): queries in independent groups that
    # fit RANK_BYTES_MAX (and the kernels' 65535-query grid), each ranked on its own
    per = max(1, min(65535, RANK_BYTES_MAX // (32 * n)))
    if q.shape[0] <= per:
        return _ops.rank_full(db, q).t()
    out = torch.empty((n, q.shape[0]), dtype=torch.int64, device=db.device)
    for j in range(0, q.shape[0], per):
        out[:, j:j + per] = _ops.rank_full(db, q[j:j + per].contiguous()).t()
    return out


def shard_range(n, rank, world):
    """Contiguous row shard of rank r: [r*ceil(n/R), min(n, (r+1)*ceil(n/R)))."""
    per = (n + world - 1) // world
    r0 = min(n, rank * per)
    return r0, max(0, min(per, n - r0))


def all_gather_stacked(t, group=None):
    """[...] per rank -> [R, ...] on every rank.  GPU tensors on an RCCL group
    ("nccl" backend on ROCm): one all_gather_into_tensor over xGMI.  Other
    backends (gloo) gather host copies and the result returns to t's device."""
    world = dist.get_world_size(group)
    if t.is_cuda and dist.get_backend(group) == "nccl":
        out = torch.empty((world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        dist.all_gather_into_tensor(out, t.contiguous(), group=group)
        return out
    host = t.detach().cpu().contiguous()
    out = torch.empty((world,) + tuple(host.shape), dtype=host.dtype)
    dist.all_gather(list(out.unbind(0)), host, group=group)
    return out.to(t.device)


class ShardedIndex:
    """Database rows [row0, row0 + n_local) of a global matrix live on this
    rank; ``search`` expects the same queries on every rank (all-gather them
    first if each rank extracted its own).

    The only exchange is one all-gather of the per-shard (score f64, index i64)
    lists, packed in one buffer — Q x k x 16 bytes per rank — followed by the on-GPU merge with the
    (score desc, index asc) rule, so the merged result is bit-identical to a
    single-GPU search of the whole database."""

    def __init__(self, local_rows, row0, precision="bf16", cand=0, group=None, local_index=None, merge=None):
        self.local = local_index if local_index is not None else KnnIndex(local_rows, precision, cand, idx_offset=row0)
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.merge = merge or _ops.topk_merge

    def search(self, q_rows, k, verify=True):
        """merged top-k of the queries (the same on every rank).  verify=True (default) /
        "deferred": every shard certifies its own top-k; the flags travel in the
        same all-gather as the lists, so every rank sees the same uncertain set
        and re-searches it (each shard in float32, then one more exchange) together.
        verify=False: the uncertified screen."""
        if not verify:
            s, i = self.local.search(q_rows, k, verify=False)
            return (s, i) if self.world == 1 else self.exchange(s, i, k)
        if self.world == 1:
            return self.local.search(q_rows, k, verify=verify)
        if self.local.ntotal == 0 or q_rows.shape[0] == 0:
            # an empty shard certifies trivially: (-inf, -1) lists, no flags
            s, i = self.local.search(q_rows, k, verify=False)
            unc = torch.zeros(q_rows.shape[0], dtype=torch.int32, device=s.device)
        else:
            # the flags travel in the all-gather: no per-shard Pending (pinned copy + event)
            s, i, unc = self.local.search_checked(q_rows, k)
        s, i, flags = self.exchange(s, i, k, flags=unc)

        def research(bad):
            s2, i2 = self.local.search(q_rows[bad], k, verify=True)
            return self.exchange(s2, i2, k)

        pend = Pending(flags, research, s, i)
        if verify == "deferred":
            return s, i, pend
        pend.resolve()
        return s, i

    def exchange(self, s, i, k, flags=None):
        """per-shard (score f64, index i64) [Q, k] -> merged [Q, k]: ONE all-gather of
        the two lists packed as int64 pairs [Q, k, 2] (16 B per entry), then the merge.
        flags (int32 [Q], optional) ride along as one more pair per query and come back
        OR-ed over the shards."""
        packed = torch.stack([s.contiguous().view(torch.int64), i], dim=-1)
        if flags is not None:
            extra = torch.zeros((s.shape[0], 1, 2), dtype=torch.int64, device=s.device)
            extra[:, 0, 0] = flags
            packed = torch.cat([packed, extra], dim=1)
        g = all_gather_stacked(packed, self.group)                 # [R, Q, k(+1), 2]
        ms, mi = self.merge(g[:, :, :k, 0].contiguous().view(torch.float64), g[:, :, :k, 1].contiguous(), k)
        if flags is None:
            return ms, mi
        return ms, mi, g[:, :, k, 0].amax(0).to(torch.int32)


def merge_topk(scores, idx, k):
    """[R, Q, k_in] per-shard lists -> [Q, k] by (score desc, index asc)."""
    return _ops.topk_merge(scores, idx, k)


def mutual_nn(desc1, desc2, precision="fp32"):
    """Mutual nearest-neighbour matcher of HPatchesEval.py:31-43 for unit-norm
    descriptors [N1, D] and [N2, D] (rows): nearest by L2 distance == highest
    dot product, exact order with ties to the lower index like np.argmin.
    Returns int64 [N1]: the match in desc2, or -1 where not mutual."""
    a = desc1.float().contiguous()
    b = desc2.float().contiguous()
    _, n12 = KnnIndex(b, precision).search(a, 1, verify=True)
    _, n21 = KnnIndex(a, precision).search(b, 1, verify=True)
    return _ops.mutual_nn(n12[:, 0], n21[:, 0])


def detect_keypoints(images, num_features=2048, response="harris", k=0.04, nms=5, min_score=0.0, border=0, sigmas=None,
                     return_response=False):
    """Keypoints of a batch of images in one call (rr_detect_keypoints): the Harris, Shi-Tomasi
    ("gftt") or Hessian response of ``cirtorch/features/responses.py`` on the gray image, the
    ``nms x nms`` non-maxima suppression of ``cirtorch/features/nms.py`` and the `num_features`
    best maxima by (score desc, y * W + x asc) -- the device-side replacement of the host
    detector ``generate_kpts(..., 'sift')`` (``cirtorch/datasets/localFeatures/utils.py:56-99``).

    images  [B, 1|3, H, W], float32 in [0, 1] or uint8 (a pixel is v / 255); three channels are
            reduced by 0.299 r + 0.587 g + 0.114 b
    ->      kpts float32 [B, N, 2] pixel (x, y) (the layout ``verify_pairs`` takes), scores float32
            [B, N], count int32 [B]; the slots past count hold (-1, -1) and score 0.  With
            return_response=True also the score map float32 [B, 1, H, W].

    A candidate is a positive strict maximum of its window with score > min_score, at least
    `border` pixels from every edge.  float64 arithmetic rounded once: the result is
    bit-identical run to run and does not depend on the batch.  No device->host
    synchronisation: graph-capturable for fixed shapes."""
    if response not in _ops.RESPONSES:
        raise ValueError("detect_keypoints: response %r (one of harris, gftt, hessian)" % (response,))
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] not in (1, 3):
        raise ValueError("detect_keypoints: images are [B, 1, H, W] or [B, 3, H, W], got %s"
                         % (tuple(images.shape) if torch.is_tensor(images) else type(images),))
    if images.dtype not in (torch.float32, torch.uint8):
        raise TypeError("detect_keypoints: images are float32 or uint8, got %s" % images.dtype)
    if isinstance(nms, tuple):
        if len(nms) != 2 or nms[0] != nms[1]:
            raise ValueError("detect_keypoints: the nms window must be square, got %r" % (nms,))
        nms = nms[0]
    return _ops.detect_keypoints(images, int(num_features), response, float(k), nms, float(min_score), int(border),
                                 sigmas, return_response)


def detect_keypoints_scale_space(images, num_features=2048, response="hessian", levels=3, sigma=1.6, min_size=15, mr_size=6.0,
                                 minima=None, k=0.04, affine=False, affine_patch_size=32):
    """Scale-covariant keypoints of a batch of images in one call (rr_detect_scale_space): the
    ``ScalePyramid`` of ``cirtorch/geometry/transform/pyramid.py``, the Hessian, Harris, Shi-Tomasi
    ("gftt") or difference-of-Gaussians ("dog") response of every level, the strict 3 x 3 x 3 extrema
    and quadratic refinement of ``ConvQuadInterp3d``, and the frames and top-N selection of
    ``ScaleSpaceDetector.detect`` (``cirtorch/features/scale_space_detector.py``).

    images  [B, 1|3, H, W], float32 in [0, 1] or uint8 (a pixel is v / 255); three channels are
            reduced by 0.299 r + 0.587 g + 0.114 b
    ->      lafs float32 [B, N, 2, 3] in image pixels, [[s, 0, x], [0, s, y]] with
            s = mr_size * sigma of the keypoint -- what ``describe_keypoints(images, None, lafs=lafs)``
            takes, and ``get_laf_center(lafs)`` is the (x, y) layout of ``verify_pairs`` --, scores
            float32 [B, N] (the refined response), count int32 [B]; the slots past count hold a zero
            frame and score 0.

    The best `num_features` are taken over all octaves by (score desc, octave asc, voxel asc).  With
    `minima` (default: only for "dog") strict minima count too, scored by -response.  A frame whose
    circle of radius s leaves its octave is dropped.  With `affine` the detected frames go through
    ``estimate_affine_shape`` (patch size `affine_patch_size`) before they are returned: one more
    call, in place, the scale and centre of every frame kept (Hessian-Affine with response
    "hessian").  float64 arithmetic rounded once: bit-identical
    run to run and independent of the batch.  No device->host synchronisation: graph-capturable
    for fixed shapes."""
    if response not in _ops.SS_RESPONSES:
        raise ValueError("detect_keypoints_scale_space: response %r (one of harris, gftt, hessian, dog)" % (response,))
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] not in (1, 3):
        raise ValueError("detect_keypoints_scale_space: images are [B, 1, H, W] or [B, 3, H, W], got %s"
                         % (tuple(images.shape) if torch.is_tensor(images) else type(images),))
    if images.dtype not in (torch.float32, torch.uint8):
        raise TypeError("detect_keypoints_scale_space: images are float32 or uint8, got %s" % images.dtype)
    if minima is None:
        minima = response == "dog"
    if affine and not _ops.PATCH_SIZES[0] <= int(affine_patch_size) <= _ops.PATCH_SIZES[1]:
        raise ValueError("detect_keypoints_scale_space: affine_patch_size %r outside [8, 64]" % (affine_patch_size,))
    lafs, scores, count = _ops.detect_scale_space(images, int(num_features), response, int(levels), float(sigma), int(min_size),
                                                  float(mr_size), bool(minima), float(k))
    if affine:
        _ops.laf_affine_shape(images, lafs, count, int(affine_patch_size), out=lafs)
    return lafs, scores, count


def estimate_affine_shape(images, lafs, count=None, patch_size=32):
    """Affine shape of the frames of a batch of images in one call (rr_laf_affine_shape): the
    ``LAFAffineShapeEstimator`` of ``cirtorch/features/affine_shape.py`` -- the stage of
    ``ScaleSpaceDetector`` between detection and orientation.

    images  [B, 1|3, H, W], float32 in [0, 1] or uint8 (a pixel is v / 255); three channels are
            reduced by 0.299 r + 0.587 g + 0.114 b
    lafs    float32 [B, N, 2, 3] in pixels; count int32 [B] or None
    ->      lafs float32 [B, N, 2, 3]: per frame the patch of ``make_upright(laf)`` from its pyramid
            level (`patch_size` a side), the second-moment matrix of its Gaussian-weighted Sobel
            gradients, ``ellipse_to_laf`` of it, rescaled to the scale of the input frame; the centre
            is the input's.  A patch without structure (two of the three raw moments below 1e-10,
            judged before the normalisation) keeps a circle.  Slots at or past count, slots whose
            centre is (-1, -1) and frames with a non-finite entry hold zeros.

    The result is upright; ``describe_keypoints(lafs=..., orientation=True, pyramid=True)`` gives it
    an orientation.  float64 arithmetic rounded once: bit-identical run to run and independent of
    the batch.  No patch is written to memory and nothing waits for the host: graph-capturable for
    fixed shapes.  No gradients."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] not in (1, 3):
        raise ValueError("estimate_affine_shape: images are [B, 1, H, W] or [B, 3, H, W], got %s"
                         % (tuple(images.shape) if torch.is_tensor(images) else type(images),))
    return _ops.laf_affine_shape(images, lafs, count, int(patch_size))


# patches the learned-descriptor path of describe_keypoints holds at a time (4 KiB each)
LEARNED_PATCH_BUDGET = 16384


def _describe_learned(images, kpts, count, scale, lafs, orientation, pyramid, descriptor):
    """describe_keypoints with a HardNet / SOSNet module: frames -> patches -> rr_patchnet_describe, a
    slice of the keypoints at a time.  Device work only."""
    from .features.laf import _rotation, make_upright
    from .geometry.conversions import rad2deg
    images = _ops._describe_image(images, "describe_keypoints")
    n = images.shape[0]
    _ops.E.require_gpu(kpts, count, lafs)
    _ops._no_grad("describe_keypoints", images, kpts, lafs)
    if lafs is not None:
        if lafs.dim() != 4 or lafs.shape[0] != n or tuple(lafs.shape[2:]) != (2, 3):
            raise ValueError("describe_keypoints: lafs must be [%d, N, 2, 3], got %s" % (n, tuple(lafs.shape)))
        lafs = lafs.float().contiguous()
    else:
        if kpts is None or kpts.dim() != 3 or kpts.shape[0] != n or kpts.shape[2] != 2:
            raise ValueError("describe_keypoints: kpts must be [%d, N, 2], got %s"
                             % (n, None if kpts is None else tuple(kpts.shape)))
        if not (scale > 0.0 and scale != float("inf")):
            raise ValueError("describe_keypoints: scale must be positive and finite, got %r" % (scale,))
        kpts = kpts.float()
        lafs = torch.zeros(kpts.shape[:2] + (2, 3), dtype=torch.float32, device=kpts.device)
        lafs[..., 0, 0] = scale
        lafs[..., 1, 1] = scale
        lafs[..., 2] = kpts
    npts = lafs.shape[1]
    dev = images.device
    if count is not None and (count.dim() != 1 or count.shape[0] != n or count.dtype != torch.int32):
        raise ValueError("describe_keypoints: count must be int32 [%d], got %s %s" % (n, count.dtype, tuple(count.shape)))
    # dead slots: at or past count, a (-1, -1) centre, a frame that is not finite.  They are sampled as
    # the unit frame at the origin and their rows zeroed.
    dead = (lafs[..., 2] == -1).all(-1) | ~torch.isfinite(lafs).all(-1).all(-1)
    if count is not None:
        dead |= torch.arange(npts, device=dev)[None, :] >= count[:, None]
    safe = torch.zeros((2, 3), dtype=torch.float32, device=dev)
    safe[0, 0] = 1.0
    safe[1, 1] = 1.0
    lafs = torch.where(dead[..., None, None], safe, lafs)
    gray = images.shape[1] == 3
    pyr = _ops.patch_pyramid(images, 32, gray)[1] if pyramid else None
    extract = (lambda f: _ops.extract_patches_pyramid(images, f, 32, gray, pyr=pyr)) if pyramid else \
        (lambda f: _ops.extract_patches(images, f, 32, gray))
    desc = torch.empty((n, npts, 128), dtype=torch.float32, device=dev)
    angles = torch.zeros((n, npts), dtype=torch.float32, device=dev)
    step = max(1, LEARNED_PATCH_BUDGET // max(n, 1))
    for j0 in range(0, npts, step):
        frames = lafs[:, j0:j0 + step].contiguous()
        if orientation:
            frames = make_upright(frames).contiguous()
            ang = _ops.patch_orientation(extract(frames)[:, :, 0], 36)
            angles[:, j0:j0 + step] = ang
            frames = torch.cat([torch.matmul(frames[..., :2, :2], _rotation(rad2deg(ang))), frames[..., :2, 2:]], dim=3).contiguous()
        d = descriptor.describe(extract(frames)[:, :, 0])
        desc[:, j0:j0 + step] = d.view(n, -1, 128)
    desc.masked_fill_(dead[..., None], 0.0)
    angles.masked_fill_(dead, 0.0)
    return desc, angles


def describe_keypoints(images, kpts, count=None, scale=12.0, lafs=None, orientation=False, patch_size=32, num_ang_bins=8,
                       num_spatial_bins=4, rootsift=True, clipval=0.2, pyramid=False, descriptor=None):
    """SIFT descriptors of the keypoints of a batch of images in one call (rr_describe_keypoints):
    the patch of ``extract_patches_simple`` (``cirtorch/features/laf.py``), optionally the dominant
    gradient orientation of ``LAFOrienter`` (``cirtorch/features/orientation.py``, 36 bins) and the
    ``SIFTDescriptor`` of ``cirtorch/features/siftdesc.py`` -- the device-side replacement of the
    descriptor half of ``generate_kpts(..., 'sift')``.  It takes what ``detect_keypoints`` returns.

    images  [B, 1|3, H, W], float32 in [0, 1] or uint8 (a pixel is v / 255); three channels are
            reduced by 0.299 r + 0.587 g + 0.114 b
    kpts    float32 [B, N, 2] pixel (x, y); count int32 [B] or None.  The frame of a keypoint is
            [[scale, 0, x], [0, scale, y]]: the patch covers 2 * scale pixels a side.  lafs
            [B, N, 2, 3] (pixels), when given, are the frames instead (kpts is then ignored; with
            orientation=True they are made upright first).
    ->      desc float32 [B, N, num_ang_bins * num_spatial_bins ** 2] (L2-normalised; RootSIFT by
            default), angles float32 [B, N] in radians (0 without orientation).  Slots at or past
            count and slots whose keypoint is (-1, -1) hold zeros.

    pyramid=False samples every patch from the image itself (pyramid level 0; the reference's
    pyramid agrees while 2 * scale / patch_size < sqrt(2)).  pyramid=True
    (rr_describe_keypoints_pyramid) first builds the ``pyrdown`` levels of the gray image and samples
    each frame from level max(0, floor(log2(2 s / patch_size) + 0.5)) as
    ``extract_patches_from_pyramid`` does -- what the frames of ``detect_keypoints_scale_space`` need;
    a frame past the last level (the last whose smaller side is at least patch_size) is sampled from
    the last level, where the reference leaves a zero patch.  Frames of level 0 give the same bits
    either way.  float64 arithmetic rounded once: bit-identical run to run and independent of the
    batch.  No patch is written to memory and nothing waits for the host: graph-capturable for
    fixed shapes.  No gradients.

    descriptor=None is the SIFT descriptor above.  A ``cirtorch.features.HardNet`` or ``SOSNet``
    instance (on the GPU, in eval mode) describes the same frames instead: desc is then float32
    [B, N, 128] from rr_patchnet_describe (fp16 operands, float32 accumulation), the patches are those
    of ``extract_patches_simple`` (``extract_patches_from_pyramid`` with pyramid=True) at patch_size
    32 -- any other size raises --, orientation=True estimates the angle on the upright frame's patch
    (rr_patch_orientation) and describes the frame turned by it.  The patches of at most 16384
    keypoints are held at a time; dead slots are masked on the device; nothing waits for the host.
    The SIFT arguments are ignored."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] not in (1, 3):
        raise ValueError("describe_keypoints: images are [B, 1, H, W] or [B, 3, H, W], got %s"
                         % (tuple(images.shape) if torch.is_tensor(images) else type(images),))
    if descriptor is not None:
        from .features.patchnet import PatchNet
        if not isinstance(descriptor, PatchNet):
            raise TypeError("describe_keypoints: descriptor is None (SIFT), a HardNet or a SOSNet, got %s" % type(descriptor))
        if int(patch_size) != 32:
            raise ValueError("describe_keypoints: %s takes 32 x 32 patches, got patch_size = %r"
                             % (type(descriptor).__name__, patch_size))
        return _describe_learned(images, kpts, count, float(scale), lafs, bool(orientation), bool(pyramid), descriptor)
    return _ops.describe_keypoints(images, kpts, count, float(scale), lafs, bool(orientation), 36, int(patch_size),
                                   int(num_ang_bins), int(num_spatial_bins), bool(rootsift), float(clipval),
                                   pyramid=bool(pyramid))


def _match_rows(x):
    """[rows, D] -> contiguous float32 rows with D zero-padded to a multiple of 4
    (zero columns change no distance)."""
    x = x.float()
    if x.shape[1] % 4:
        x = torch.nn.functional.pad(x, (0, 4 - x.shape[1] % 4))
    return x.contiguous()


def match_pairs(desc1, desc2, mode="mnn", th=0.8, offsets1=None, offsets2=None, max_n1=None, max_n2=None):
    """Batched local-descriptor matching in one launch (rr_match_pairs): the rules of
    ``cirtorch/features/matching.py`` -- "nn", "mnn", "snn" (Lowe's ratio test
    first / second <= th), "smnn" -- for P pairs at once, L2 distances exact to
    float64 rounding (ties to the lower index), descriptors of any norm,
    4 <= D <= 512, no N1 x N2 matrix.

    dense   desc1 [P, N1, D] x desc2 [P, N2, D] (or [N1, D] x [N2, D])
            -> match int64 [P, N1] ([N1]), dist float32 of the same shape
    ragged  desc1 [rows1, D], desc2 [rows2, D] with device int64 offsets1 / offsets2
            [P + 1]: pair p is desc1[offsets1[p]:offsets1[p + 1]] against
            desc2[offsets2[p]:offsets2[p + 1]] -> match, dist [rows1]
            (max_n1 / max_n2: optional host bounds of a pair's lengths; they
            only trim the launch grid)

    match[i] is the pair-local index in desc2 or -1, dist[i] the L2 distance
    (nn, mnn) or the first / second ratio (snn; smnn: the larger of the two
    directions'), +inf where match is -1.  No device->host synchronisation:
    graph-capturable (``cirtorch.utils.graph``) for fixed shapes."""
    if mode not in _ops.MATCH_MODES:
        raise ValueError("match_pairs: mode %r (one of nn, mnn, snn, smnn)" % (mode,))
    if (offsets1 is None) != (offsets2 is None):
        raise ValueError("match_pairs: give both offsets1 and offsets2 (ragged) or neither (dense)")
    if desc1.shape[-1] != desc2.shape[-1]:
        raise ValueError("match_pairs: D differs (%d and %d)" % (desc1.shape[-1], desc2.shape[-1]))
    if not 1 <= desc1.shape[-1] <= 512:
        raise ValueError("match_pairs: D = %d outside [1, 512]" % desc1.shape[-1])
    _ops.E.require_gpu(desc1, desc2, offsets1, offsets2)
    if offsets1 is not None:
        if desc1.dim() != 2 or desc2.dim() != 2:
            raise ValueError("match_pairs: the ragged form takes [rows, D] descriptors")
        return _ops.match_pairs(_match_rows(desc1), offsets1.contiguous(), _match_rows(desc2), offsets2.contiguous(),
                                mode, th, max_n1, max_n2)
    if desc1.dim() != desc2.dim() or desc1.dim() not in (2, 3) or (desc1.dim() == 3 and desc1.shape[0] != desc2.shape[0]):
        raise ValueError("match_pairs: dense descriptors are [P, N, D] or [N, D] on both sides, got %s and %s"
                         % (tuple(desc1.shape), tuple(desc2.shape)))
    lead = desc1.shape[:-1]
    p = desc1.shape[0] if desc1.dim() == 3 else 1
    n1, n2, d = desc1.shape[-2], desc2.shape[-2], desc1.shape[-1]
    steps = torch.arange(p + 1, dtype=torch.int64, device=desc1.device)
    match, dist = _ops.match_pairs(_match_rows(desc1.reshape(p * n1, d)), steps * n1,
                                   _match_rows(desc2.reshape(p * n2, d)), steps * n2, mode, th, n1, n2, covered=True)
    return match.view(lead), dist.view(lead)


def verify_pairs(kpts1, kpts2, match, th=3.0, iters=1024, refine=2, seed=0, offsets1=None, offsets2=None, max_n1=None,
                 model="homography", K1=None, K2=None):
    """Spatial verification of matched pairs in one call (rr_verify_pairs): per pair a RANSAC
    homography over the kept matches (``match[i] >= 0``), refitted `refine` times by the
    reference's DLT on its inliers -- what ``compute_H_estimation`` (HPatchesEval.py:45-69) gets
    from ``cv2.findHomography(..., cv2.RANSAC)`` one pair at a time on the host.  float64 on
    float32 pixel keypoints (x, y); `iters` hypotheses per pair drawn by a counter hash of
    (seed, pair, t), so a result is bit-identical run to run and does not depend on the batch.

    dense   kpts1 [P, N1, 2], kpts2 [P, N2, 2], match int64 [P, N1] (or [N1, 2], [N2, 2], [N1])
            -> inliers int32 [P], H float64 [P, 3, 3], mask bool [P, N1]
    ragged  kpts1 [rows1, 2], kpts2 [rows2, 2], match [rows1] with device int64 offsets1 /
            offsets2 [P + 1], the tables given to ``match_pairs`` -> inliers [P], H [P, 3, 3],
            mask [rows1] (max_n1: optional host bound of a pair's side-1 length)

    `match` is exactly what ``match_pairs`` returns.  inliers counts the matches within `th`
    pixels of H, mask marks their side-1 rows; a pair with fewer than 4 matches or only degenerate
    samples gives 0, an all-zero H and an empty mask.  No device->host synchronisation:
    graph-capturable for fixed shapes.

    model="fundamental" (rr_verify_pairs_epipolar) verifies against the epipolar geometry of two
    views of a 3-D scene instead: a seven-point RANSAC fundamental matrix, refitted by the
    reference's 8-point ``find_fundamental`` on its inliers, inliers = the matches whose Sampson
    distance is at most `th` pixels.  Same forms and outputs, with F [P, 3, 3] (unit Frobenius
    norm, ``x2^T F x1 = 0``) in place of H; fewer than 7 matches give 0.  On a planar scene or
    under pure rotation F is not determined and the count is inflated: use the homography there, or,
    with known cameras, the essential matrix.

    model="essential" (rr_verify_pairs_essential) is the calibrated verifier: K1 / K2 [3, 3] (one camera
    for every pair) or [P, 3, 3] are the intrinsics of the two views, the hypotheses come from a
    five-point solver on five matches, the refit is the 8-point fit projected onto the essential
    matrices.  inliers and mask mean what they mean for "fundamental" (Sampson distance in pixels of
    F = K2^-T E K1^-1); E [P, 3, 3] has unit Frobenius norm and singular values (s, s, 0).  It stays
    determined on a plane, up to the two motions a plane admits.  Fewer than 5 matches, or a K that
    cannot be inverted, give 0.  ``fundamental_from_essential(E, K1, K2)`` is what ``recover_pose``
    takes."""
    if model not in _ops.VERIFY_MODELS:
        raise ValueError("verify_pairs: model is 'homography', 'fundamental' or 'essential', got %r" % (model,))
    if model == "essential" and (K1 is None or K2 is None):
        raise ValueError("verify_pairs: model 'essential' needs the intrinsics K1 and K2")
    if model != "essential" and (K1 is not None or K2 is not None):
        raise ValueError("verify_pairs: K1 / K2 go with model 'essential', not with %r" % (model,))
    if (offsets1 is None) != (offsets2 is None):
        raise ValueError("verify_pairs: give both offsets1 and offsets2 (ragged) or neither (dense)")
    if kpts1.shape[-1] != 2 or kpts2.shape[-1] != 2:
        raise ValueError("verify_pairs: keypoints are (x, y) rows, got %s and %s" % (tuple(kpts1.shape), tuple(kpts2.shape)))
    if int(iters) < 1 or int(refine) < 0 or not (float(th) > 0.0 and float(th) < float("inf")):
        raise ValueError("verify_pairs: iters >= 1, refine >= 0 and a positive finite th, got %r, %r, %r" % (iters, refine, th))
    if match.dtype != torch.int64:
        raise ValueError("verify_pairs: match must be int64 (the output of match_pairs), got %s" % match.dtype)
    if offsets1 is not None:
        if kpts1.dim() != 2 or kpts2.dim() != 2 or match.dim() != 1 or match.shape[0] != kpts1.shape[0]:
            raise ValueError("verify_pairs: the ragged form takes [rows, 2] keypoints and match [rows1]")
        mats = _verify_mats(K1, K2, offsets1.numel() - 1)
        _ops.E.require_gpu(kpts1, kpts2, match, offsets1, offsets2, K1, K2)
        inl, H, mask = _ops.verify_pairs(kpts1.float().contiguous(), offsets1.contiguous(), kpts2.float().contiguous(),
                                         offsets2.contiguous(), match.contiguous(), th, iters, refine, seed, max_n1,
                                         model=model, **mats)
        return inl, H, mask.view(torch.bool)
    if kpts1.dim() != kpts2.dim() or kpts1.dim() not in (2, 3) or (kpts1.dim() == 3 and kpts1.shape[0] != kpts2.shape[0]) \
            or tuple(match.shape) != tuple(kpts1.shape[:-1]):
        raise ValueError("verify_pairs: dense keypoints are [P, N, 2] or [N, 2] on both sides with match [P, N1] or [N1], "
                         "got %s, %s and %s" % (tuple(kpts1.shape), tuple(kpts2.shape), tuple(match.shape)))
    p = kpts1.shape[0] if kpts1.dim() == 3 else 1
    n1, n2 = kpts1.shape[-2], kpts2.shape[-2]
    if max_n1 is not None and int(max_n1) < n1:
        raise ValueError("verify_pairs: max_n1 = %d below the pairs' length %d" % (int(max_n1), n1))
    mats = _verify_mats(K1, K2, p)
    _ops.E.require_gpu(kpts1, kpts2, match, K1, K2)
    steps = torch.arange(p + 1, dtype=torch.int64, device=kpts1.device)
    inl, H, mask = _ops.verify_pairs(kpts1.float().reshape(p * n1, 2).contiguous(), steps * n1,
                                     kpts2.float().reshape(p * n2, 2).contiguous(), steps * n2,
                                     match.reshape(p * n1).contiguous(), th, iters, refine, seed, n1, covered=True,
                                     model=model, **mats)
    return inl, H, mask.view(torch.bool).view(match.shape)


def _pose_mats(m, p, what, who="recover_pose"):
    """[3, 3] (one for every pair) or [P, 3, 3] -> contiguous float64 [P, 3, 3]"""
    if tuple(m.shape) == (3, 3):
        m = m.unsqueeze(0).expand(p, 3, 3)
    if tuple(m.shape) != (p, 3, 3):
        raise ValueError("%s: %s must be [3, 3] or [P, 3, 3] with P = %d, got %s" % (who, what, p, tuple(m.shape)))
    return m.double().contiguous()


def _verify_mats(K1, K2, p):
    """the intrinsics of verify_pairs(model="essential") as keyword arguments of _ops.verify_pairs"""
    if K1 is None:
        return {}
    return dict(K1=_pose_mats(K1, p, "K1", "verify_pairs"), K2=_pose_mats(K2, p, "K2", "verify_pairs"))


def recover_pose(kpts1, kpts2, match, F, K1, K2, mask=None, offsets1=None, offsets2=None, max_n1=None):
    """The camera motion between the two views of each verified pair, and the 3-D points its matches
    triangulate to, in one call (rr_recover_pose) -- the step after
    ``verify_pairs(model="fundamental")``, every output of which is an input here:

        inl, F, mask = verify_pairs(q_kpts, db_kpts, match, th=1.5, model="fundamental")
        R, t, X, front_mask, front = recover_pose(q_kpts, db_kpts, match, F, Kq, Kdb, mask=mask)

    Per pair: E = K2^T F K1 (``essential_from_fundamental``), its four candidate motions
    (``decompose_essential_matrix``), the matches triangulated under each (``triangulate_points``) and
    the candidate with the most points in front of both cameras
    (``motion_from_essential_choose_solution``), all in float64 on the device without a
    ``torch.svd``.  Each pair chooses its own solution (the reference applies the choice of pair 0 to
    a whole batch).

    dense   kpts1 [P, N1, 2], kpts2 [P, N2, 2], match int64 [P, N1], mask bool [P, N1] or None
            (or [N1, 2], [N2, 2], [N1]), F [P, 3, 3] (or [3, 3] for one pair), K1 / K2 [3, 3] (one
            camera for every pair) or [P, 3, 3]
            -> R float64 [P, 3, 3], t float64 [P, 3, 1] (unit norm: the scale is not observable),
               points3d float64 [P, N1, 3] in the first camera's frame (zeros on unused rows),
               front_mask bool [P, N1], front int32 [P] (the number of points in front)
    ragged  kpts1 [rows1, 2], kpts2 [rows2, 2], match [rows1], mask [rows1] with the device int64
            offsets1 / offsets2 [P + 1] of ``verify_pairs`` -> points3d [rows1, 3], front_mask [rows1]

    mask=None uses every kept match.  A pair whose F is all zero (a failed verification), or with no
    match to use, gives zeros and front 0.  ``x2 = K2 (R X + t)``, ``x1 = K1 X``.  No device->host
    synchronisation: graph-capturable for fixed shapes."""
    if (offsets1 is None) != (offsets2 is None):
        raise ValueError("recover_pose: give both offsets1 and offsets2 (ragged) or neither (dense)")
    if kpts1.shape[-1] != 2 or kpts2.shape[-1] != 2:
        raise ValueError("recover_pose: keypoints are (x, y) rows, got %s and %s" % (tuple(kpts1.shape), tuple(kpts2.shape)))
    if match.dtype != torch.int64:
        raise ValueError("recover_pose: match must be int64 (the output of match_pairs), got %s" % match.dtype)
    if mask is not None and (tuple(mask.shape) != tuple(match.shape) or mask.dtype not in (torch.bool, torch.uint8)):
        raise ValueError("recover_pose: mask must be bool or uint8 of match's shape %s, got %s %s"
                         % (tuple(match.shape), mask.dtype, tuple(mask.shape)))
    if offsets1 is not None:
        if kpts1.dim() != 2 or kpts2.dim() != 2 or match.dim() != 1 or match.shape[0] != kpts1.shape[0]:
            raise ValueError("recover_pose: the ragged form takes [rows, 2] keypoints and match [rows1]")
        p = offsets1.numel() - 1
        if offsets2.numel() != p + 1 or p < 0:
            raise ValueError("recover_pose: offsets1 and offsets2 must both be [P + 1]")
        Fm, Ka, Kb = _pose_mats(F, p, "F"), _pose_mats(K1, p, "K1"), _pose_mats(K2, p, "K2")
        _ops.E.require_gpu(kpts1, kpts2, match, mask, offsets1, offsets2, F, K1, K2)
        R, t, _, front, pts, fmask = _ops.recover_pose(kpts1.float().contiguous(), offsets1.contiguous(),
                                                       kpts2.float().contiguous(), offsets2.contiguous(), match.contiguous(),
                                                       None if mask is None else mask.contiguous(), Fm, Ka, Kb, max_n1)
        return R, t.unsqueeze(-1), pts, fmask.view(torch.bool), front
    if kpts1.dim() != kpts2.dim() or kpts1.dim() not in (2, 3) or (kpts1.dim() == 3 and kpts1.shape[0] != kpts2.shape[0]) \
            or tuple(match.shape) != tuple(kpts1.shape[:-1]):
        raise ValueError("recover_pose: dense keypoints are [P, N, 2] or [N, 2] on both sides with match [P, N1] or [N1], "
                         "got %s, %s and %s" % (tuple(kpts1.shape), tuple(kpts2.shape), tuple(match.shape)))
    p = kpts1.shape[0] if kpts1.dim() == 3 else 1
    n1, n2 = kpts1.shape[-2], kpts2.shape[-2]
    if max_n1 is not None and int(max_n1) < n1:
        raise ValueError("recover_pose: max_n1 = %d below the pairs' length %d" % (int(max_n1), n1))
    Fm, Ka, Kb = _pose_mats(F, p, "F"), _pose_mats(K1, p, "K1"), _pose_mats(K2, p, "K2")
    _ops.E.require_gpu(kpts1, kpts2, match, mask, F, K1, K2)
    steps = torch.arange(p + 1, dtype=torch.int64, device=kpts1.device)
    R, t, _, front, pts, fmask = _ops.recover_pose(kpts1.float().reshape(p * n1, 2).contiguous(), steps * n1,
                                                   kpts2.float().reshape(p * n2, 2).contiguous(), steps * n2,
                                                   match.reshape(p * n1).contiguous(),
                                                   None if mask is None else mask.reshape(p * n1).contiguous(), Fm, Ka, Kb,
                                                   n1, covered=True)
    return R, t.unsqueeze(-1), pts.view(tuple(match.shape) + (3,)), fmask.view(torch.bool).view(match.shape), front


def localize_pairs(kpts, points3d, match, K, th=3.0, iters=1024, refine=2, seed=0, valid=None, offsets1=None, offsets2=None,
                   max_n1=None):
    """The pose of a query camera against the 3-D points of each database image it was matched to, in
    one call (rr_localize_pairs): per pair a RANSAC pose from three-point samples (P3P), refitted
    `refine` times by Gauss-Newton on the reprojection error of its inliers.  The last step of a
    localization pipeline; every input comes from the steps before it:

        inl, F, m = verify_pairs(a_kpts, b_kpts, match_ab, th=1.5, model="fundamental")
        Rab, tab, X, front_mask, front = recover_pose(a_kpts, b_kpts, match_ab, F, Ka, Kb, mask=m)
        match_qa, _ = match_pairs(q_desc, a_desc, mode="smnn")
        inl, R, t, mask = localize_pairs(q_kpts, X, match_qa, Kq, th=3.0, valid=front_mask)   # query pose in view a's frame, in units of |tab|

    ``points3d`` and ``front_mask`` of ``recover_pose`` are indexed by view a's keypoint rows, and
    ``match_pairs(query, view a)`` returns indices into exactly those rows.  float64 on float32 pixel
    keypoints (x, y); `iters` hypotheses per pair drawn by the counter hash of ``verify_pairs``, so a
    result is bit-identical run to run and does not depend on the batch.

    dense   kpts [P, N1, 2], points3d [P, N2, 3], match int64 [P, N1], valid bool [P, N2] or None
            (or [N1, 2], [N2, 3], [N1], [N2] for one pair), K [3, 3] (one camera for every pair) or [P, 3, 3]
            -> inliers int32 [P], R float64 [P, 3, 3], t float64 [P, 3, 1], mask bool [P, N1]
    ragged  kpts [rows1, 2], points3d [rows2, 3], match [rows1], valid [rows2] with the device int64
            offsets1 / offsets2 [P + 1] of ``match_pairs`` -> mask [rows1] (max_n1: optional host bound
            of a pair's side-1 length)

    ``[x, y, 1]^T ~ K (R X + t)``.  points3d is float64 (what ``recover_pose`` writes) or float32,
    converted once.  A row counts where its match is kept, `valid` (when given) marks its 3-D point and
    the point is finite; inliers counts the rows whose point lies in front of the camera and
    reprojects within `th` pixels, mask marks them.  Fewer than 3 such rows, a K that cannot be
    inverted, or no sample with an inlier give 0, an all-zero R and t and an empty mask.
    ``rerank_by_inliers`` takes these counts as it takes ``verify_pairs``'.  No device->host
    synchronisation: graph-capturable for fixed shapes."""
    if (offsets1 is None) != (offsets2 is None):
        raise ValueError("localize_pairs: give both offsets1 and offsets2 (ragged) or neither (dense)")
    if kpts.shape[-1] != 2 or points3d.shape[-1] != 3:
        raise ValueError("localize_pairs: keypoints are (x, y) rows and points3d (X, Y, Z) rows, got %s and %s"
                         % (tuple(kpts.shape), tuple(points3d.shape)))
    if int(iters) < 1 or int(refine) < 0 or not (float(th) > 0.0 and float(th) < float("inf")):
        raise ValueError("localize_pairs: iters >= 1, refine >= 0 and a positive finite th, got %r, %r, %r" % (iters, refine, th))
    if match.dtype != torch.int64:
        raise ValueError("localize_pairs: match must be int64 (the output of match_pairs), got %s" % match.dtype)
    if points3d.dtype not in (torch.float32, torch.float64):
        raise ValueError("localize_pairs: points3d must be float64 or float32, got %s" % points3d.dtype)
    if valid is not None and (tuple(valid.shape) != tuple(points3d.shape[:-1]) or valid.dtype not in (torch.bool, torch.uint8)):
        raise ValueError("localize_pairs: valid must be bool or uint8 of shape %s, got %s %s"
                         % (tuple(points3d.shape[:-1]), valid.dtype, tuple(valid.shape)))
    if offsets1 is not None:
        if kpts.dim() != 2 or points3d.dim() != 2 or match.dim() != 1 or match.shape[0] != kpts.shape[0]:
            raise ValueError("localize_pairs: the ragged form takes [rows1, 2] keypoints, [rows2, 3] points and match [rows1]")
        p = offsets1.numel() - 1
        if offsets2.numel() != p + 1 or p < 0:
            raise ValueError("localize_pairs: offsets1 and offsets2 must both be [P + 1]")
        Km = _pose_mats(K, p, "K", "localize_pairs")
        _ops.E.require_gpu(kpts, points3d, match, valid, offsets1, offsets2, K)
        inl, R, t, mask = _ops.localize_pairs(kpts.float().contiguous(), offsets1.contiguous(), points3d.double().contiguous(),
                                              None if valid is None else valid.contiguous(), offsets2.contiguous(),
                                              match.contiguous(), Km, th, iters, refine, seed, max_n1)
        return inl, R, t.unsqueeze(-1), mask.view(torch.bool)
    if kpts.dim() != points3d.dim() or kpts.dim() not in (2, 3) or (kpts.dim() == 3 and kpts.shape[0] != points3d.shape[0]) \
            or tuple(match.shape) != tuple(kpts.shape[:-1]):
        raise ValueError("localize_pairs: dense inputs are [P, N1, 2] keypoints and [P, N2, 3] points (or [N1, 2] and [N2, 3]) "
                         "with match [P, N1] or [N1], got %s, %s and %s"
                         % (tuple(kpts.shape), tuple(points3d.shape), tuple(match.shape)))
    p = kpts.shape[0] if kpts.dim() == 3 else 1
    n1, n2 = kpts.shape[-2], points3d.shape[-2]
    if max_n1 is not None and int(max_n1) < n1:
        raise ValueError("localize_pairs: max_n1 = %d below the pairs' length %d" % (int(max_n1), n1))
    Km = _pose_mats(K, p, "K", "localize_pairs")
    _ops.E.require_gpu(kpts, points3d, match, valid, K)
    steps = torch.arange(p + 1, dtype=torch.int64, device=kpts.device)
    inl, R, t, mask = _ops.localize_pairs(kpts.float().reshape(p * n1, 2).contiguous(), steps * n1,
                                          points3d.double().reshape(p * n2, 3).contiguous(),
                                          None if valid is None else valid.reshape(p * n2).contiguous(), steps * n2,
                                          match.reshape(p * n1).contiguous(), Km, th, iters, refine, seed, n1, covered=True)
    return inl, R, t.unsqueeze(-1), mask.view(torch.bool).view(match.shape)


def rerank_by_inliers(idx, inliers):
    """Re-order a [k, Q] shortlist (``knn``'s ranks: column q lists query q's database rows, best
    first) by the verified inlier counts [k, Q] of its entries: (inliers desc, original rank
    asc).  Plain torch (a stable sort), works on any device, no host synchronisation."""
    if idx.dim() != 2 or tuple(inliers.shape) != tuple(idx.shape):
        raise ValueError("rerank_by_inliers: idx and inliers must both be [k, Q], got %s and %s"
                         % (tuple(idx.shape), tuple(inliers.shape)))
    order = torch.sort(inliers.to(torch.int64), dim=0, descending=True, stable=True).indices
    return torch.gather(idx, 0, order)
