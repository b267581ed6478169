"""ImageRetrievalNet (reference ``cirtorch/models/GF_net.py:10-126``) plus the
upstream entry points ``scripts/test.py`` imports from this module
(``init_network``, ``extract_vectors``; ``scripts/test.py:12,105,200,236-238``).

forward(img=PackedSequence, scales=[...]) -> (OrderedDict(ret_loss=None),
OrderedDict(ret_pred=Tensor[D, N])), with the reference semantics:
  * multi-scale: per-image bilinear resize (align_corners=False), recursive
    single-scale extraction, plain mean of the per-scale L2-normalised
    descriptors, no re-normalisation (``GF_net.py:20-40,74-92``);
  * a PackedSequence goes to the body as a ragged batch: the stem reads every
    image at its own address and pads to the max H, W top-left on the fly
    (``utils/sequence.py`` semantics, no padded copy), then normalises (pads
    become -mean/std, ``random_augmentation.py:102,174``) when an augment
    object carrying rgb_mean / rgb_std is attached;
  * body -> ret_algo.inference(head, x) -> D x N.
"""

import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from .. import _ops
from ..algos.GF_algo import globalFeatureAlgo
from ..backbones import resnet as _resnet
from ..modules.heads.global_head import globalHead
from ..modules.pools import POOLING_LAYERS
from ..utils.parallel import PackedSequence

from ..modules.utils import OUTPUT_DIM  # noqa: E402  (reference cirtorch/modules/utils.py:61-79)


class Normalize:
    """Minimal stand-in for the reference augment object
    (``RandomAugmentation(rgb_mean, rgb_std)``): eval-time normalisation only,
    fused by the engine into the first kernel."""

    def __init__(self, rgb_mean=(0.485, 0.456, 0.406), rgb_std=(0.229, 0.224, 0.225)):
        self.rgb_mean = list(rgb_mean)
        self.rgb_std = list(rgb_std)


class ImageRetrievalNet(nn.Module):
    def __init__(self, body, ret_algo, ret_head, augment=None):
        super().__init__()
        self.augment = augment
        self.body = body
        self.ret_algo = ret_algo
        self.ret_head = ret_head
        self.meta = {}

    # ----------------------------------------------------------------- helpers
    def _prepare_pyramid_inputs(self, img, scales):
        out = []
        for scale in scales:
            if scale == 1:
                out.append(img)
            else:
                out.append(PackedSequence([_ops.resize_bilinear(im, scale) for im in img]))
        return out

    def _normalizer(self):
        a = self.augment
        if a is None:
            return None
        if hasattr(a, "rgb_mean") and hasattr(a, "rgb_std"):
            return (list(a.rgb_mean), list(a.rgb_std))
        raise NotImplementedError("only normalising augment objects (rgb_mean/rgb_std) are supported at eval time")

    @property
    def pool(self):
        """upstream ``net.pool`` (``scripts/test.py:137``)."""
        return self.ret_head.pool

    def meta_repr(self):
        tmp = "  (meta): dict( \n"
        for k in ("architecture", "local_whitening", "pooling", "regional", "whitening", "outputdim", "mean", "std"):
            if k in self.meta:
                tmp += "     %s: %s\n" % (k, self.meta[k])
        tmp += "  )\n"
        return tmp

    # ----------------------------------------------------------------- forward
    def forward(self, img=None, positive_img=None, negative_img=None, scales=[1], do_augmentaton=False,
                do_loss=False, do_prediction=True, **varargs):
        if do_loss:
            raise NotImplementedError("training (tuple loss) is out of scope for the MI355X engine")
        if isinstance(img, torch.Tensor) and img.dim() == 4 and len(scales) == 1:
            # already a same-size batch: no packing / padding copy
            x = self.body(img, normalize=self._normalizer())
            ret_pred = self.ret_algo.inference(self.ret_head, x, [img.shape[-2:]] * img.shape[0]) \
                if do_prediction else None
            return OrderedDict([("ret_loss", None)]), OrderedDict([("ret_pred", ret_pred)])
        if isinstance(img, torch.Tensor) and img.dim() == 4:
            # same-size batch, multi-scale: one batched resize per pyramid level
            # (every image has the same output size), then one extractor chain
            preds = []
            for scale in scales:
                if scale == 1:
                    xs = img
                else:
                    xf = _ops.pixels_to_unit(img) if img.dtype == torch.uint8 else img
                    xs = _ops.resize_bilinear(xf, scale)
                _, pred = self.forward(img=xs, scales=[1], do_prediction=True, do_loss=False)
                preds.append(pred["ret_pred"].unsqueeze(0))
            pred = torch.cat(preds, dim=0).permute(1, 2, 0)
            pred = nn.functional.avg_pool1d(pred, kernel_size=len(scales)).squeeze(-1)
            return OrderedDict([("ret_loss", None)]), OrderedDict([("ret_pred", pred)])
        if isinstance(img, torch.Tensor):
            if img.dtype == torch.uint8 and len(scales) > 1:  # pixels -> [0, 1] (to_tensor) for the resize
                img = _ops.pixels_to_unit(img)
            img = PackedSequence(list(img)) if img.dim() == 4 else PackedSequence([img])
        if len(scales) > 1:
            if img.dtype == torch.uint8:
                img = PackedSequence([_ops.pixels_to_unit(t) if t is not None else None for t in img])
            preds = []
            for im in self._prepare_pyramid_inputs(img, scales):
                _, pred = self.forward(img=im, scales=[1], do_prediction=True, do_loss=False)
                preds.append(pred["ret_pred"].unsqueeze(0))
            pred = torch.cat(preds, dim=0).permute(1, 2, 0)
            pred = nn.functional.avg_pool1d(pred, kernel_size=len(scales)).squeeze(-1)
            return OrderedDict([("ret_loss", None)]), OrderedDict([("ret_pred", pred)])

        # the ragged batch goes to the body as is: the stem reads each image at its own
        # address and pads to the max extent on the fly (pad_packed_images semantics,
        # utils/sequence.py:4-67, without writing the padded batch)
        images = list(img)
        x = self.body(images, normalize=self._normalizer())
        valid_size = [tuple(t.shape[-2:]) if t is not None else (0, 0) for t in images]
        if do_prediction:
            ret_pred = self.ret_algo.inference(self.ret_head, x, valid_size)
        else:
            ret_pred = None
        return OrderedDict([("ret_loss", None)]), OrderedDict([("ret_pred", ret_pred)])

    # upstream-style single call: list of [3, H, W] tensors -> D x N
    def extract(self, images, scales=(1,)):
        """images: list of [3, H, W] tensors or one [N, 3, H, W] batch -> D x N."""
        if not isinstance(images, torch.Tensor):
            images = PackedSequence(list(images))
        with torch.no_grad():
            _, pred = self.forward(img=images, scales=list(scales))
        return pred["ret_pred"]


def make_net(architecture="resnet50", pooling="gem", whitening=True, mean=None, std=None, precision="bf16",
             p=3.0, regional=False, regional_whitening=True, L=3):
    """Build body + globalHead + algo the way ``scripts/train_globalF.py:make_model`` does
    (``:240-356``): leaky_relu(0.01) ABN, GeM(p, 1e-6), L2N, Linear(dim, dim) whitening.
    regional=True (the ``-reg`` networks of ``scripts/test.py:42-43,98,124``) wraps the pool in
    ``Rpool(pool, Linear(dim, dim), L)`` (``regional_whitening=False``: no regional Linear)."""
    body = _resnet.__dict__[architecture](precision=precision)
    dim = OUTPUT_DIM[architecture]
    pname = {"gem": "GeM", "mac": "MAC", "spoc": "SPoC", "gemmp": "GeMmp"}[pooling.lower()]
    params = {"p": p, "eps": 1e-6} if pname in ("GeM", "GeMmp") else {}
    if regional:
        if pname == "GeMmp":
            params["mp"] = dim
        rwhiten = nn.Linear(dim, dim, bias=True) if regional_whitening else None
        params = {"rpool": POOLING_LAYERS[pname](**params), "whiten": rwhiten, "L": L}
        pname = "ROIpool"
    head = globalHead(pooling={"name": pname, "params": params}, normal={"name": "L2N", "params": {}}, dim=dim)
    algo = globalFeatureAlgo(loss=None, min_level=0, fpn_levels=1)
    if not whitening:
        algo._head = lambda h, x: h(x, do_whitening=False)
    augment = Normalize(mean, std) if mean is not None else None
    net = ImageRetrievalNet(body, algo, head, augment=augment)
    net.meta = {"architecture": architecture, "pooling": pooling, "local_whitening": False, "regional": bool(regional),
                "whitening": whitening, "mean": list(mean) if mean is not None else None,
                "std": list(std) if std is not None else None, "outputdim": dim}
    return net


def init_network(params):
    """Upstream ``init_network(params)`` (``scripts/test.py:105``)."""
    arch = params.get("architecture", "resnet101")
    pooling = params.get("pooling", "gem")
    if params.get("local_whitening", False):
        raise NotImplementedError("local_whitening (the per-pixel whitening of upstream cirtorch) is not part of "
                                  "the reference this engine follows; regional pooling is: regional=True")
    if params.get("pretrained", False):
        # offline build: no ImageNet weights can be fetched; random init instead
        pass
    mean = params.get("mean", [0.485, 0.456, 0.406])
    std = params.get("std", [0.229, 0.224, 0.225])
    # fp16 by default: it meets the north_star descriptor bar (cosine >= 1 - 1e-4
    # vs the fp32 reference) at bf16 speed; extract_vectors re-extracts any
    # descriptor that overflowed fp16's range in bf16.  "bf16" is an explicit
    # opt-in and "fp32" the exact-f32 MFMA parity mode.
    return make_net(arch, pooling, params.get("whitening", False), mean, std,
                    precision=params.get("precision", "fp16"), regional=params.get("regional", False),
                    regional_whitening=params.get("regional_whitening", True), L=params.get("L", 3))


def _load_pil(path, imsize, bbx=None):
    from PIL import Image
    with open(path, "rb") as f:
        img = Image.open(f).convert("RGB")
    if bbx is not None:
        img = img.crop(bbx)
    if imsize is not None:
        img.thumbnail((imsize, imsize), Image.LANCZOS)
    return img


def _to_pixels(img):
    return torch.from_numpy(np.asarray(img, dtype=np.uint8).transpose(2, 0, 1).copy())


def _to_tensor(img):
    a = np.asarray(img, dtype=np.float32) / 255.0
    return torch.from_numpy(a.transpose(2, 0, 1).copy())


def _decode(item, image_size, bbx, transform, tf):
    """one input -> CHW tensor on the host: uint8 pixels (no transform) or the
    transform's float tensor."""
    if not isinstance(item, str):
        return item
    if tf is not None:                       # ISSTestTransform semantics (bbx crop, shortest side)
        from PIL import Image
        with open(item, "rb") as f:
            pil = Image.open(f).convert("RGB")
        return tf.pixels(pil, bbx) if transform is None else transform(tf._resized(pil, bbx))
    pil = _load_pil(item, image_size, bbx)
    # no transform: the decoded uint8 pixels cross PCIe (1 B per channel) and the
    # fused stem reads them as x / 255 (== _to_tensor, bit for bit)
    return transform(pil) if transform is not None else _to_pixels(pil)


class _PinnedBlocks:
    """Page-locked host blocks for decoded files, reused across chains and calls
    (allocating page-locked memory costs far more than decoding into it): a block
    goes back to the free list once the H2D copy that read it has finished (its
    chain's event).  Blocks are flat uint8 buffers viewed as [H, W, 3]; a request
    takes the smallest free block that holds it.  At most `cap` bytes stay free."""

    def __init__(self, cap=2 << 30):
        import threading
        self.lock = threading.Lock()
        self.free = []   # flat pinned uint8 tensors
        self.busy = []   # (event, [flat tensors])
        self.out = {}    # data_ptr of a handed-out view -> its block
        self.cap = cap

    def _reclaim(self):
        keep = []
        for ev, blocks in self.busy:
            if ev.query():
                self.free.extend(blocks)
            else:
                keep.append((ev, blocks))
        self.busy = keep
        total = sum(b.numel() for b in self.free)
        if total > self.cap:   # drop the largest free blocks first
            self.free.sort(key=lambda b: b.numel())
            while self.free and total > self.cap:
                total -= self.free.pop().numel()

    def acquire(self, shape):
        n = int(np.prod(shape))
        with self.lock:
            self._reclaim()
            fit = [k for k, b in enumerate(self.free) if b.numel() >= n]
            b = self.free.pop(min(fit, key=lambda k: self.free[k].numel())) if fit else None
        if b is None:
            b = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        v = b[:n].view(shape)
        with self.lock:
            self.out[v.data_ptr()] = b
        return v

    def release(self, views, event):
        """views: tensors from acquire() (others are ignored); event: recorded after
        the copies that read them"""
        with self.lock:
            blocks = [self.out.pop(v.data_ptr()) for v in views if v.data_ptr() in self.out]
            if blocks:
                self.busy.append((event, blocks))


_BLOCKS = _PinnedBlocks()


def _decode_pinned(item, image_size, bbx):
    """file path -> its uint8 pixels as a pinned [H, W, 3] host tensor from the
    block pool (the decode thread's copies: PIL's buffer and one contiguous copy
    into page-locked memory).  The HWC -> CHW transpose runs on the GPU, once per
    chain."""
    a = np.asarray(_load_pil(item, image_size, bbx), dtype=np.uint8)
    t = _BLOCKS.acquire(a.shape)
    # numpy's copy: one memcpy on this thread (torch's copy_ would fan out over
    # intra-op threads from every decode thread at once: measured 6.7x slower)
    np.copyto(t.numpy(), a)
    return t


_PINNED = [None, None]  # one grown-on-demand pinned staging buffer per double-buffer slot, kept across calls


def _pinned_chain(slot, shape, dtype):
    """pinned host view of `shape` in slot's staging buffer: pinning 150 MB
    per chain costs more than the chain's H2D, so the buffer is reused (the
    caller has waited for the slot's previous copy)."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = _PINNED[slot]
    if buf is None or buf.numel() < n:
        buf = _PINNED[slot] = torch.empty(n, dtype=torch.uint8).pin_memory()
    return buf[:n].view(dtype).view(shape)


def _default_workers():
    """decode threads: the CPUs this process may run on, at most 16 (RR_EV_WORKERS overrides)"""
    import os
    if os.environ.get("RR_EV_WORKERS"):
        return max(1, int(os.environ["RR_EV_WORKERS"]))
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def extract_vectors(net, images, image_size, transform=None, bbxs=None, ms=[1], msp=1, print_freq=10,
                    batch=64, workers=None, test_transform=None, _no_procs=False):
    """Upstream ``extract_vectors`` (``scripts/test.py:200,236-238``): returns a
    CPU float32 tensor D x len(images).  ``images`` are file paths (PIL load,
    bbx crop, longest side resized to image_size — or ``test_transform``, an
    ``ISSTestTransform`` of the in-tree loaders) or [3, H, W] tensors (float
    in [0, 1] or uint8 pixels).  ms/msp follow the upstream rule:
    v = (mean_s f(x_s)^msp)^(1/msp), then L2-normalised.

    Each image is extracted on its own, as with batch size 1 (the engine's
    kernels give the same bits whatever the chain length): images are grouped
    by size (nothing is ever padded inside a group) into chains of up to
    ``batch`` images.  ``workers`` host threads (default: the usable CPUs, at
    most 16) decode up to ``4 * batch`` inputs ahead of the GPU; a chain starts
    as soon as its group is full.  Decoded files travel as pinned uint8 HWC
    pixels, host tensors as one pinned chain, on a copy stream double-buffered
    against the extractor (the fused stem reads x / 255)."""
    from concurrent.futures import ThreadPoolExecutor
    workers = workers or _default_workers()
    dev = next(net.parameters()).device
    n = len(images)
    D = net.meta.get("outputdim", 2048)
    vecs = torch.zeros(D, n, device=dev)
    if n == 0:
        return vecs.cpu()
    normalize_in_net = net.augment is not None and transform is None
    mean = torch.tensor(net.meta["mean"], device=dev)[:, None, None] if net.meta.get("mean") is not None else None
    std = torch.tensor(net.meta["std"], device=dev)[:, None, None] if net.meta.get("std") is not None else None
    ms = list(ms)
    main = torch.cuda.current_stream(dev)
    copy = torch.cuda.Stream(dev)
    copied = [torch.cuda.Event(), torch.cuda.Event()]
    freed = [torch.cuda.Event(), torch.cuda.Event()]
    for e in freed:
        e.record(main)
    state = {"slot": 0}

    outs = []  # (columns, descriptors) per chain; scattered into vecs once at the end

    def run(part, items, hwc=False):
        """one same-size group of images -> their descriptor columns (hwc: pinned
        [H, W, 3] pixels of decoded files, copied one by one into the chain)"""
        slot = state["slot"]
        if hwc:
            copy.wait_event(freed[slot])
            with torch.cuda.stream(copy):
                xh = torch.empty((len(items),) + tuple(items[0].shape), dtype=torch.uint8, device=dev)
                for j, t in enumerate(items):
                    xh[j].copy_(t, non_blocking=True)
            copied[slot].record(copy)
            done = torch.cuda.Event()
            done.record(copy)
            _BLOCKS.release(items, done)
            if procs is not None:
                procs.release(items, done)
            main.wait_event(copied[slot])
            xh.record_stream(main)
            x = xh.permute(0, 3, 1, 2).contiguous()
            host = None
        elif items[0].is_cuda:                # device tensors: stacked in place, no host staging
            x = torch.stack([t.to(dev) for t in items]) if len(items) > 1 else items[0].to(dev)[None]
            host = None
        elif len(part) > 1:
            copied[slot].synchronize()        # the previous H2D out of this slot's host buffer has finished
            host = _pinned_chain(slot, (len(part),) + tuple(items[0].shape), items[0].dtype)
            torch.stack(items, out=host)      # (measured: faster than a per-image copy on 8 host threads)
        else:
            host = items[0][None]
        if host is not None:
            copy.wait_event(freed[slot])      # the extractor is done with this slot's device buffer
            with torch.cuda.stream(copy):
                x = host.to(dev, non_blocking=len(part) > 1)
            copied[slot].record(copy)
            main.wait_event(copied[slot])
            x.record_stream(main)
        if x.dtype == torch.uint8 and (ms != [1] or not normalize_in_net):
            x = _ops.pixels_to_unit(x)
        elif x.dtype != torch.uint8:
            x = x.float()
        if not normalize_in_net and transform is None and mean is not None:
            x = (x - mean) / std
        if ms == [1]:
            v = net.extract(x)
        else:
            acc = None
            for s in ms:
                xs = x if s == 1 else _ops.resize_bilinear(x, s)
                vs = net.extract(xs).pow(msp)
                acc = vs if acc is None else acc + vs
            v = (acc / len(ms)).pow(1.0 / msp)
            v = v / v.norm(dim=0, keepdim=True)
        # no host->device index copy here: a pageable copy would wait for the
        # whole queued extraction and serialise host and device
        outs.append((part, v.float()))
        freed[slot].record(main)
        state["slot"] = slot ^ 1
        state["last"] = freed[slot]

    saved = net.augment
    if not normalize_in_net:
        net.augment = None
    # Decode threads run up to `ahead` inputs in front of the consumer; decoded
    # images are grouped by size and a group runs as soon as it holds `batch`
    # images (partial groups: when the buffered images exceed `ahead`, the
    # largest one runs; the rest at the end), so extraction overlaps decoding.
    ahead = max(2, 4 * batch)
    # shortest chain started early while the GPU idles (RR_EV_MIN_CHAIN: A/B knob; 16 / 32 / 64
    # within the host's noise on 128 JPEGs, profiles/r03_ab/r03q_dropin_sched_ab.txt)
    min_chain = max(1, min(batch, int(os.environ.get("RR_EV_MIN_CHAIN", "32"))))
    pinned_files = transform is None and test_transform is None

    def decode(i):
        item, bbx = images[i], bbxs[i] if bbxs is not None else None
        if pinned_files and isinstance(item, str):
            return "hwc", _decode_pinned(item, image_size, bbx)
        return "chw", _decode(item, image_size, bbx, transform, test_transform)

    # Files of a long list decode in worker processes (no GIL) into a page-locked
    # shared-memory ring (cirtorch/utils/decode_procs.py); RR_DECODE_PROCS=0: threads.
    procs = None
    if (pinned_files and workers > 1 and n >= 2 * batch and os.environ.get("RR_DECODE_PROCS", "1") != "0"
            and not _no_procs and all(isinstance(it, str) for it in images)):
        from ..utils import decode_procs
        # slots: pending decodes + decoded images waiting in size groups (each <= ahead)
        # + the chains whose H2D copy is in flight (<= 2 x batch); ahead = 2 chains in
        # decode keep every worker busy.  None (no room in /dev/shm, no page-locking):
        # the decode threads below.
        procs = decode_procs.get(workers, 6 * batch + 8, decode_procs.slot_bytes_for(image_size))
        if procs is not None:
            ahead = max(2, 2 * batch)

    first1 = workers if os.environ.get("RR_EV_FIRST1", "0") == "1" else 0  # single-file first tasks (A/B knob)

    class _ProcFuture:
        def __init__(self, p):
            self.p = p

        def result(self):
            return "hwc", self.p.result()

    def submit_next(pool, futs, nxt):
        """submit input nxt (files through the process decoder: up to 4 per task, one
        per task for the first `workers` files so the first chain starts early) -> next index"""
        if procs is None:
            futs.append((nxt, pool.submit(decode, nxt)))
            return nxt + 1
        hi = min(n, nxt + (1 if nxt < first1 else 4))
        ps = procs.submit_group([(images[i], image_size, bbxs[i] if bbxs is not None else None)
                                 for i in range(nxt, hi)])
        for i, p in zip(range(nxt, hi), ps):
            futs.append((i, _ProcFuture(p)))
        return hi

    try:
        with ThreadPoolExecutor(max_workers=max(1, workers)) as pool, torch.no_grad():
            from collections import deque
            futs = deque()
            nxt = 0
            groups = {}
            buffered = 0

            def flush(key):
                nonlocal buffered
                g = groups.pop(key)
                buffered -= len(g)
                run([i for i, _ in g], [x for _, x in g], hwc=key[0] == "hwc")

            while nxt < n and len(futs) < ahead:
                nxt = submit_next(pool, futs, nxt)
            while futs:
                i, f = futs.popleft()
                kind, x = f.result()
                if nxt < n and len(futs) < ahead:
                    nxt = submit_next(pool, futs, nxt)
                key = (kind, tuple(x.shape), x.dtype, x.is_cuda)
                groups.setdefault(key, []).append((i, x))
                buffered += 1
                if len(groups[key]) == batch:
                    flush(key)
                elif buffered > ahead:
                    flush(max(groups, key=lambda k: len(groups[k])))
                elif len(groups[key]) >= min_chain and (state.get("last") is None or state["last"].query()):
                    # the GPU has run out of work while decoding is the bound: start
                    # a shorter chain now (same bits: chain length never changes them)
                    flush(key)
            for key in list(groups):
                flush(key)
            if outs:
                cols = torch.tensor([c for part, _ in outs for c in part], dtype=torch.long).to(dev)
                vecs[:, cols] = torch.cat([v for _, v in outs], dim=1)
    except Exception as e:
        if procs is None:
            raise
        # the process decoder's slots held by undelivered images are lost with the
        # error: drop the cached decoder (a later call builds a fresh ring)
        from ..utils import decode_procs
        decode_procs.drop()
        if not isinstance(e, decode_procs.DecoderFailure):
            raise
        import warnings
        warnings.warn("extract_vectors: the process decoder failed (%s); decoding on threads instead" % e)
        net.augment = saved
        return extract_vectors(net, images, image_size, transform=transform, bbxs=bbxs, ms=ms, msp=msp,
                               print_freq=print_freq, batch=batch, workers=workers, test_transform=test_transform,
                               _no_procs=True)
    finally:
        net.augment = saved
    out = vecs.cpu()
    # fp16 activations saturate at 65504: a descriptor that overflowed (checkpoints
    # whose activations leave fp16 range) is re-extracted with bf16 storage (fp32
    # range) instead of being returned as inf / NaN.  One check on the host copy.
    body = getattr(net, "body", None)
    bad = (~torch.isfinite(out)).any(dim=0).nonzero().flatten().tolist()
    if bad and getattr(body, "engine_dtype", None) == torch.float16 and hasattr(body, "set_precision"):
        import warnings
        warnings.warn("extract_vectors: %d descriptor(s) overflowed fp16; re-extracting them in bf16" % len(bad))
        body.set_precision("bf16")
        try:
            redo = extract_vectors(net, [images[i] for i in bad], image_size, transform=transform,
                                   bbxs=[bbxs[i] for i in bad] if bbxs is not None else None, ms=ms, msp=msp,
                                   print_freq=print_freq, batch=batch, workers=workers,
                                   test_transform=test_transform)
        finally:
            body.set_precision("fp16")
        out[:, bad] = redo
    return out
