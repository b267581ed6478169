"""torch-tensor wrappers over the librr.so entry points (device memory and
streams come from PyTorch; all arithmetic is in the HIP kernels).

Shapes follow the engine's layouts: activations NHWC ([N, H, W, C] tensors),
packed conv weights [c_out, k_packed], descriptors row-major [n, D].
"""

import ctypes
import os

import numpy as np
import torch

from . import _engine as E


def _st():
    return E.stream_ptr()


def _workspace(nbytes, device):
    """A workspace of the size the library asked for (never empty: an entry rejects a null pointer)."""
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# ---------------------------------------------------------------- extractor ops
def image_to_nhwc(img, c_pad, dtype, mean=None, std=None):
    """img: [N, C<=4, H, W] float32 (GPU) -> [N, H, W, c_pad] `dtype`, normalised
    with (x - mean) / std when mean/std are given (cirtorch/utils/image.py:86-127)."""
    E.require_gpu(img)
    img = img.contiguous().float()
    n, c, h, w = img.shape
    out = torch.empty((n, h, w, c_pad), dtype=dtype, device=img.device)
    do = mean is not None
    m = (ctypes.c_float * 4)(*(list(mean) + [0.0] * (4 - c))[:4]) if do else (ctypes.c_float * 4)()
    s = (ctypes.c_float * 4)(*(list(std) + [1.0] * (4 - c))[:4]) if do else (ctypes.c_float * 4)(1, 1, 1, 1)
    E.check(E.lib().rr_image_to_nhwc(E.ptr(img), n, c, h, w, m, s, int(do), E.ptr(out), c_pad,
                                     E.dtype_code(dtype), _st()), "rr_image_to_nhwc")
    return out


def pack_conv_weights(weight, cin_pad, dtype, perm32=False, k_mult=64):
    """nn.Conv2d weight [c_out, c_in, kh, kw] (GPU) -> engine layout [c_out, k_packed]."""
    E.require_gpu(weight)
    w = weight.detach().float().contiguous()
    co, ci, kh, kw = w.shape
    kp = (kh * kw * cin_pad + k_mult - 1) // k_mult * k_mult
    out = torch.empty((co, kp), dtype=dtype, device=w.device)
    E.check(E.lib().rr_pack_conv_weights(E.ptr(w), co, ci, kh, kw, cin_pad, kp, int(bool(perm32)), E.ptr(out),
                                         E.dtype_code(dtype), _st()), "rr_pack_conv_weights")
    return out


def conv2d_fused(x, w_packed, kh, kw, stride, pad, c_out, scale=None, shift=None, residual=None,
                 leaky=True, slope=0.01, out_dtype=None, dil=1, perm32=False, out=None):
    """x: [N, H, W, C] -> act(conv(x) * scale + shift (+ residual)) as [N, Ho, Wo, c_out].
    perm32: w_packed rows are in the RR_CONV_PERM32 order (pack_conv_weights(perm32=True)).
    out: an optional contiguous [N, Ho, Wo, c_out] destination (e.g. a batch slice)."""
    E.require_gpu(x, w_packed)
    n, h, w, c = x.shape
    ho = (h + 2 * pad - dil * (kh - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    out_dtype = out_dtype or x.dtype
    if out is not None:
        E.require_gpu(out)
        assert tuple(out.shape) == (n, ho, wo, c_out) and out.dtype == out_dtype and out.is_contiguous()
        y = out
    else:
        y = torch.empty((n, ho, wo, c_out), dtype=out_dtype, device=x.device)
    flags = 0
    if scale is not None:
        flags |= E.RR_CONV_AFFINE
    if residual is not None:
        flags |= E.RR_CONV_RESIDUAL
        assert residual.shape == y.shape and residual.dtype == out_dtype and residual.is_contiguous()
    if perm32:
        flags |= E.RR_CONV_PERM32
    d = E.ConvDesc(n=n, h=h, w=w, c_in=c, ho=ho, wo=wo, c_out=c_out, kh=kh, kw=kw, stride=stride, pad=pad,
                   dil=dil, k_packed=w_packed.shape[1], ldy=c_out,
                   act=E.RR_ACT_LEAKY if leaky else E.RR_ACT_IDENTITY, slope=slope, flags=flags)
    E.check(E.lib().rr_conv2d_fused(E.ptr(x), E.ptr(w_packed), E.ptr(scale), E.ptr(shift), E.ptr(residual),
                                    E.ptr(y), ctypes.byref(d), E.dtype_code(x.dtype), E.dtype_code(out_dtype),
                                    _st()), "rr_conv2d_fused")
    return y


def _pair_out(out, shape_y, shape_z, dtype, device):
    """The (y, z) destinations of a pair op: new tensors, or the caller's out=(y, z) checked as
    conv2d_fused checks its out."""
    if out is None:
        return torch.empty(shape_y, dtype=dtype, device=device), torch.empty(shape_z, dtype=dtype, device=device)
    y, z = out
    E.require_gpu(y, z)
    assert tuple(y.shape) == shape_y and y.dtype == dtype and y.is_contiguous()
    assert tuple(z.shape) == shape_z and z.dtype == dtype and z.is_contiguous()
    return y, z


def conv1x1_pair(x, w3, scale3, shift3, residual, leaky3, slope3, w1, scale1, shift1, c_out, leaky1, slope1,
                 proj=None, out=None):
    """Fused y = act3(conv1x1(x, w3)*scale3 + shift3 + shortcut); z = act1(conv1x1(y, w1)*scale1 + shift1)
    (conv3 of one bottleneck block + conv1 of the next, cirtorch/backbones/misc.py:166-203).
    shortcut = residual, or with residual=None and proj=(xp, wp, scalep, shiftp) the block's 1x1
    projection proj_bn(proj_conv(xp)) computed in the same pass (64 -> 256 boundaries only).
    x: [N, H, W, 64] or [N, H, W, 128] bf16 / fp16, PERM32-packed weights; returns
    (y [N, H, W, 256 | 512], z [N, H, W, c_out]).  out: optional contiguous (y, z) destinations."""
    E.require_gpu(x, w3, residual, w1)
    n, h, w, c = x.shape
    c_mid = w3.shape[0]
    y, z = _pair_out(out, (n, h, w, c_mid), (n, h, w, c_out), x.dtype, x.device)
    assert x.is_contiguous()
    if residual is not None:
        assert residual.shape == y.shape and residual.dtype == x.dtype and residual.is_contiguous()
        xp = wp = sp = hp = None
    else:
        xp, wp, sp, hp = proj
        E.require_gpu(xp, wp, sp, hp)
        assert xp.shape == x.shape and xp.dtype == x.dtype and xp.is_contiguous()
    E.check(E.lib().rr_conv1x1_pair(E.ptr(x), n * h * w, c, E.ptr(w3), E.ptr(scale3), E.ptr(shift3), c_mid,
                                    E.ptr(residual), E.ptr(xp), E.ptr(wp), E.ptr(sp), E.ptr(hp),
                                    E.RR_ACT_LEAKY if leaky3 else E.RR_ACT_IDENTITY, float(slope3),
                                    E.ptr(w1), E.ptr(scale1), E.ptr(shift1), c_out,
                                    E.RR_ACT_LEAKY if leaky1 else E.RR_ACT_IDENTITY, float(slope1), E.ptr(y), E.ptr(z),
                                    E.dtype_code(x.dtype), _st()), "rr_conv1x1_pair")
    return y, z


def conv3x3_pair(t1, w33, scale2, shift2, leaky2, slope2, w3, scale3, shift3, residual, leaky3, slope3,
                 w1, scale1, shift1, c_out, leaky1, slope1, proj=None, dynamic=None, conv1=None,
                 out=None):
    """One whole bottleneck block of the 256-channel stage plus the next block's conv1 in one
    launch (cirtorch/backbones/misc.py:163-203): t2 = act2(conv3x3(t1, w33)*scale2 + shift2),
    y = act3(conv1x1(t2, w3)*scale3 + shift3 + shortcut), z = act1(conv1x1(y, w1)*scale1 + shift1);
    t2 stays on chip.  shortcut = residual, or with residual=None and proj=(xp, wp, scalep, shiftp)
    the block's projection.  t1: [N, H, W, 64] bf16 / fp16 with H % 4 == 0 and W % 32 == 0, PERM32
    weights; returns (y [N, H, W, 256], z [N, H, W, c_out]), bit-identical to the 3x3 launch
    followed by conv1x1_pair.  dynamic (default: RR_C3PAIR_QUEUE != "0"): per-XCD tile counters
    (a zeroed 8-int array per launch) instead of the static tile walk — same results.
    conv1=(w0, scale0, shift0, leaky0, slope0) (projection form, the stage's first block): t1 is
    the block input x (pass it as proj's xp too) and the block's conv1 runs in the launch.
    out: optional contiguous (y, z) destinations."""
    E.require_gpu(t1, w33, w3, residual, w1)
    n, h, w, c = t1.shape
    assert c == 64 and t1.is_contiguous() and tuple(w33.shape) == (64, 576) and tuple(w3.shape) == (256, 64)
    assert tuple(w1.shape) == (c_out, 256)
    y, z = _pair_out(out, (n, h, w, 256), (n, h, w, c_out), t1.dtype, t1.device)
    if residual is not None:
        assert residual.shape == y.shape and residual.dtype == t1.dtype and residual.is_contiguous()
        xp = wp = sp = hp = None
    else:
        xp, wp, sp, hp = proj
        E.require_gpu(xp, wp, sp, hp)
        assert tuple(xp.shape) == (n, h, w, 64) and xp.dtype == t1.dtype and xp.is_contiguous()
    act = lambda leaky: E.RR_ACT_LEAKY if leaky else E.RR_ACT_IDENTITY
    if dynamic is None:
        dynamic = os.environ.get("RR_C3PAIR_QUEUE", "1") != "0"
    queue = torch.zeros(8, dtype=torch.int32, device=t1.device) if dynamic else None
    w0, s0, h0, leaky0, slope0 = conv1 if conv1 is not None else (None, None, None, False, 0.0)
    if conv1 is not None:
        E.require_gpu(w0, s0, h0)
        assert proj is not None and tuple(w0.shape) == (64, 64)
    E.check(E.lib().rr_conv3x3_pair(E.ptr(t1), n, h, w, E.ptr(w0), E.ptr(s0), E.ptr(h0), act(leaky0), float(slope0),
                                    E.ptr(w33), E.ptr(scale2), E.ptr(shift2), act(leaky2),
                                    float(slope2), E.ptr(w3), E.ptr(scale3), E.ptr(shift3), E.ptr(residual),
                                    E.ptr(xp), E.ptr(wp), E.ptr(sp), E.ptr(hp), act(leaky3), float(slope3),
                                    E.ptr(w1), E.ptr(scale1), E.ptr(shift1), c_out, act(leaky1), float(slope1),
                                    E.ptr(y), E.ptr(z), E.ptr(queue), E.dtype_code(t1.dtype), _st()),
            "rr_conv3x3_pair")
    return y, z


def maxpool2d(x, k=3, stride=2, pad=1):
    E.require_gpu(x)
    n, h, w, c = x.shape
    ho = (h + 2 * pad - k) // stride + 1
    wo = (w + 2 * pad - k) // stride + 1
    y = torch.empty((n, ho, wo, c), dtype=x.dtype, device=x.device)
    E.check(E.lib().rr_maxpool2d(E.ptr(x), n, h, w, c, k, stride, pad, E.ptr(y), ho, wo, E.dtype_code(x.dtype),
                                 _st()), "rr_maxpool2d")
    return y


def pack_stem_weights(weight, dtype=torch.bfloat16):
    """conv1 weight [64, 3, 7, 7] (GPU) -> the fused stem's [64, 448] layout (bf16 or fp16):
    kernel-row K (v1-v3 stems) then space-to-depth K (v4)."""
    E.require_gpu(weight)
    w = weight.detach().float().contiguous()
    co, ci, kh, kw = w.shape
    out = torch.empty((co, 448), dtype=dtype, device=w.device)
    E.check(E.lib().rr_stem_pack_weights(E.ptr(w), co, ci, kh, kw, E.ptr(out), E.dtype_code(dtype), _st()),
            "rr_stem_pack_weights")
    return out


_UNIT_LUT = {}


def pixels_to_unit(x):
    """uint8 pixels -> float32 x / 255 with numpy's IEEE division (torchvision
    ``to_tensor``): a 256-entry table computed on the host, gathered on the
    device (torch's scalar division multiplies by the reciprocal, which differs
    in the last bit for some pixel values)."""
    lut = _UNIT_LUT.get(x.device)
    if lut is None:
        lut = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(x.device)
        _UNIT_LUT[x.device] = lut
    return lut[x.long()]


def _stem_norm_arrays(mean, std):
    """the stem entries' (mean[3], std[3], do_normalize) arguments"""
    do = mean is not None
    m = (ctypes.c_float * 3)(*mean) if do else (ctypes.c_float * 3)()
    s = (ctypes.c_float * 3)(*std) if do else (ctypes.c_float * 3)(1, 1, 1)
    return m, s, int(do)


def _stem_pooled_size(h, w):
    """(hp, wp) of the stem's output: conv 7x7/s2/p3, then max-pool 3x3/s2/p1"""
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return (ho - 1) // 2 + 1, (wo - 1) // 2 + 1


def stem_conv_pool(img, wpk, scale, shift, leaky=True, slope=0.01, mean=None, std=None):
    """Fused normalise + conv1 7x7/s2/p3 + BN + act + maxpool 3x3/s2/p1
    (cirtorch/backbones/resnet.py:59-66): [N, 3, H, W] float32 -> [N, Hp, Wp, 64] in wpk's dtype
    (bf16 or fp16).  uint8 images are read as pixels (value / 255, torchvision
    ``to_tensor``) by ``rr_stem_conv_pool_u8``: identical output to the float32
    path on ``img.float() / 255``."""
    E.require_gpu(img, wpk, scale, shift)
    u8 = img.dtype == torch.uint8
    img = img.contiguous() if u8 else img.contiguous().float()
    n, c, h, w = img.shape
    if c != 3:
        raise RuntimeError("stem_conv_pool: expected 3-channel images, got %d" % c)
    hp, wp = _stem_pooled_size(h, w)
    y = torch.empty((n, hp, wp, 64), dtype=wpk.dtype, device=img.device)
    m, s, do = _stem_norm_arrays(mean, std)
    fn = E.lib().rr_stem_conv_pool_u8 if u8 else E.lib().rr_stem_conv_pool
    E.check(fn(E.ptr(img), n, h, w, m, s, do, E.ptr(wpk), E.ptr(scale), E.ptr(shift),
               E.RR_ACT_LEAKY if leaky else E.RR_ACT_IDENTITY, float(slope), E.ptr(y), hp, wp,
               E.dtype_code(wpk.dtype), _st()), "rr_stem_conv_pool")
    return y


def _ragged(images):
    """a ragged batch (list of [C, h_i, w_i] GPU tensors of one dtype, None entries
    allowed) -> the C ABI's host (pointer, extent) arrays + the contiguous tensors
    they point into (kept referenced until the launch is enqueued)."""
    n = len(images)
    ptrs = (ctypes.c_void_p * n)()
    ext = (ctypes.c_int * (2 * n))()
    kept = []
    for i, t in enumerate(images):
        if t is None:
            continue
        E.require_gpu(t)
        t = t.contiguous()
        kept.append(t)
        ptrs[i] = t.data_ptr()
        ext[2 * i], ext[2 * i + 1] = int(t.shape[-2]), int(t.shape[-1])
    return ptrs, ext, kept


def _norm_arrays(mean, std, c):
    do = mean is not None
    m = (ctypes.c_float * 4)(*(list(mean) + [0.0] * (4 - c))[:4]) if do else (ctypes.c_float * 4)()
    s = (ctypes.c_float * 4)(*(list(std) + [1.0] * (4 - c))[:4]) if do else (ctypes.c_float * 4)(1, 1, 1, 1)
    return m, s, int(do)


def image_to_nhwc_ragged(images, h, w, c_pad, dtype, mean=None, std=None):
    """ragged batch of [C, h_i, w_i] float32 or uint8 images (h_i <= h, w_i <= w) ->
    [N, h, w, c_pad] `dtype`: the padded, normalised map (map pixels outside an
    image read 0 before normalisation, utils/sequence.py:51 then utils/image.py:125)
    without a padded copy of the inputs."""
    ref = next(t for t in images if t is not None)
    c = int(ref.shape[0])
    u8 = ref.dtype == torch.uint8
    if not u8 and ref.dtype != torch.float32:
        images = [t.float() if t is not None else None for t in images]
    ptrs, ext, kept = _ragged(images)
    out = torch.empty((len(images), h, w, c_pad), dtype=dtype, device=ref.device)
    m, s, do = _norm_arrays(mean, std, c)
    E.check(E.lib().rr_image_to_nhwc_ragged(ptrs, ext, len(images), c, h, w, int(u8), m, s, do, E.ptr(out), c_pad,
                                            E.dtype_code(dtype), _st()), "rr_image_to_nhwc_ragged")
    return out


def stem_conv_pool_ragged(images, h, w, wpk, scale, shift, leaky=True, slope=0.01, mean=None, std=None):
    """The fused stem (stem_conv_pool) on a ragged batch padded to h x w: equals
    stem_conv_pool on the padded batch bit for bit, with no padded copy."""
    E.require_gpu(wpk, scale, shift)
    ref = next(t for t in images if t is not None)
    if ref.shape[0] != 3:
        raise RuntimeError("stem_conv_pool: expected 3-channel images, got %d" % ref.shape[0])
    u8 = ref.dtype == torch.uint8
    if not u8 and ref.dtype != torch.float32:
        images = [t.float() if t is not None else None for t in images]
    ptrs, ext, kept = _ragged(images)
    hp, wp = _stem_pooled_size(h, w)
    y = torch.empty((len(images), hp, wp, 64), dtype=wpk.dtype, device=ref.device)
    m, s, do = _stem_norm_arrays(mean, std)
    E.check(E.lib().rr_stem_conv_pool_ragged(ptrs, ext, len(images), h, w, int(u8), m, s, do, E.ptr(wpk),
                                             E.ptr(scale), E.ptr(shift), E.RR_ACT_LEAKY if leaky else E.RR_ACT_IDENTITY,
                                             float(slope), E.ptr(y), hp, wp, E.dtype_code(wpk.dtype), _st()),
            "rr_stem_conv_pool_ragged")
    return y


_ELEM_CT = {1: ctypes.c_uint8, 2: ctypes.c_uint16, 4: ctypes.c_uint32, 8: ctypes.c_uint64}


def pad_images(images, h, w, pad_value=0.0):
    """ragged batch of [C, h_i, w_i] (or [h_i, w_i]) GPU tensors -> one padded
    [N, C, h, w] (or [N, h, w]) tensor, images top-left, pad_value elsewhere:
    one rr_pad_images launch (utils/sequence.py:4-67)."""
    ref = next(t for t in images if t is not None)
    chw = ref.dim() == 3
    c = int(ref.shape[0]) if chw else 1
    shape = (len(images), c, h, w) if chw else (len(images), h, w)
    out = torch.empty(shape, dtype=ref.dtype, device=ref.device)
    esz = out.element_size()
    pv = torch.tensor([pad_value], dtype=ref.dtype).view(_ELEM_TORCH[esz]).item()
    pad = _ELEM_CT[esz](pv & ((1 << (8 * esz)) - 1))
    ptrs, ext, kept = _ragged(images)
    E.check(E.lib().rr_pad_images(ptrs, ext, len(images), c, h, w, esz, ctypes.byref(pad), E.ptr(out), _st()),
            "rr_pad_images")
    return out


_ELEM_TORCH = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def resize_bilinear(img, scale_factor):
    """img: [C, H, W] (or a same-size batch [N, C, H, W]) float32 -> bilinear
    (align_corners=False) resize by scale_factor, output size floor(H*s) x
    floor(W*s) like nn.functional.interpolate(scale_factor=s)
    (cirtorch/models/GF_net.py:32-35).  Planes are independent, so a batch is
    one launch over N*C planes."""
    E.require_gpu(img)
    img = img.contiguous().float()
    lead = img.shape[:-2]
    h, w = img.shape[-2:]
    c = int(np.prod(lead)) if len(lead) else 1
    ho, wo = int(h * scale_factor), int(w * scale_factor)
    out = torch.empty(tuple(lead) + (ho, wo), dtype=torch.float32, device=img.device)
    E.check(E.lib().rr_resize_bilinear(E.ptr(img), c, h, w, E.ptr(out), ho, wo, 1.0 / scale_factor,
                                       1.0 / scale_factor, _st()), "rr_resize_bilinear")
    return out


# ---------------------------------------------------------------- head ops
def global_pool(x, mode, p=3.0, eps=1e-6):
    """x: [N, C, H, W] (NCHW-contiguous or channels_last view) -> [N, C] float32.
    p: a float, or a one-element GPU tensor (the learnable ``pool.p``) that the
    kernel reads from device memory (rr_global_pool_pdev: no host read-back)."""
    E.require_gpu(x)
    p_dev = None
    if torch.is_tensor(p):
        if p.numel() != 1:
            raise ValueError("global_pool takes one exponent; per-channel exponents go through region_pool")
        E.require_gpu(p)
        p_dev = p.detach().reshape(1)
        if p_dev.dtype != torch.float32:
            p_dev = p_dev.float()
        p = 1.0
    n, c, h, w = x.shape
    if x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
        layout = E.RR_NHWC
    elif x.is_contiguous():
        layout = E.RR_NCHW
    else:
        x = x.contiguous()
        layout = E.RR_NCHW
    if layout == E.RR_NHWC and c % 4:
        x = x.contiguous()
        layout = E.RR_NCHW
    if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        x = x.float()
    out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    if p_dev is not None:
        E.check(E.lib().rr_global_pool_pdev(E.ptr(x), n, c, h * w, layout, mode, float(p), E.ptr(p_dev), float(eps),
                                            E.ptr(out), E.dtype_code(x.dtype), _st()), "rr_global_pool_pdev")
    else:
        E.check(E.lib().rr_global_pool(E.ptr(x), n, c, h * w, layout, mode, float(p), float(eps), E.ptr(out),
                                       E.dtype_code(x.dtype), _st()), "rr_global_pool")
    return out


def region_pool(x, regions, mode, p=3.0, eps=1e-6):
    """x: [N, C, H, W] (channels_last view: read in place; anything else is
    converted to NHWC once) -> [N, R, C] float32, one pooled vector per
    rectangle of ``regions`` ((y0, x0, h, w) tuples, ``roi_regions``), all of
    them in one pass over the map (rr_region_pool).  p: a float; a one-element
    GPU tensor (a learnable ``GeM.p``), read by the kernel; or a C-element GPU
    tensor of per-channel exponents (GeMmp)."""
    E.require_gpu(x)
    n, c, h, w = x.shape
    p_dev, p_count = None, 0
    if torch.is_tensor(p):
        if p.numel() not in (1, c):
            raise ValueError("GeM exponents: one, or one per channel (%d); got %d" % (c, p.numel()))
        E.require_gpu(p)
        p_dev = p.detach().reshape(-1)
        if p_dev.dtype != torch.float32:
            p_dev = p_dev.float()
        p_count, p = p_dev.numel(), 1.0
    if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        x = x.float()
    xh = x.permute(0, 2, 3, 1)  # NHWC view
    cp = (c + 3) // 4 * 4
    if cp != c:
        # the kernel reads 4 channels per lane: zero channels are pooled and dropped
        xh = torch.nn.functional.pad(xh, (0, cp - c))
        if p_count == c:
            p_dev = torch.nn.functional.pad(p_dev, (0, cp - c), value=1.0)
        p_count = cp if p_count == c else p_count
    xh = xh.contiguous()  # no copy for a channels_last tensor
    p_dev = p_dev.contiguous() if p_dev is not None else None
    R = len(regions)
    tab = (E.Region * max(R, 1))(*[E.Region(*[int(v) for v in r]) for r in regions])
    out = torch.empty((n, R, cp), dtype=torch.float32, device=x.device)
    E.check(E.lib().rr_region_pool(E.ptr(xh), n, h, w, cp, tab, R, mode, float(p), E.ptr(p_dev), p_count,
                                   float(eps), E.ptr(out), E.dtype_code(xh.dtype), _st()), "rr_region_pool")
    return out if cp == c else out[:, :, :c].contiguous()


def region_aggregate(rv, l2n_rows=False, eps=1e-6):
    """rv: [N, R, D] float32 region descriptors -> L2N(sum_r rv) [N, D];
    l2n_rows: L2-normalise every region row first (rr_region_aggregate)."""
    E.require_gpu(rv)
    rv = rv.contiguous().float()
    n, R, dim = rv.shape
    out = torch.empty((n, dim), dtype=torch.float32, device=rv.device)
    E.check(E.lib().rr_region_aggregate(E.ptr(rv), n, R, dim, int(bool(l2n_rows)), float(eps), E.ptr(out), _st()),
            "rr_region_aggregate")
    return out


def l2n_rows(x, eps=1e-6):
    E.require_gpu(x)
    x = x.contiguous().float()
    rows = x.shape[0]
    dim = x.numel() // max(rows, 1)
    y = torch.empty_like(x)
    E.check(E.lib().rr_l2n_rows(E.ptr(x), rows, dim, float(eps), E.ptr(y), _st()), "rr_l2n_rows")
    return y


def linear_rows(x, weight, bias=None):
    E.require_gpu(x, weight, bias)
    x = x.contiguous().float()
    weight = weight.contiguous().float()
    bias = bias.contiguous().float() if bias is not None else None
    rows, in_dim = x.shape
    out_dim = weight.shape[0]
    y = torch.empty((rows, out_dim), dtype=torch.float32, device=x.device)
    E.check(E.lib().rr_linear_rows(E.ptr(x), rows, in_dim, E.ptr(weight), E.ptr(bias), out_dim, E.ptr(y), _st()),
            "rr_linear_rows")
    return y


def head_tail(pooled, weight, bias, whiten=True, eps=1e-6):
    """pooled [N, D] -> L2N(W . L2N(pooled) + b) (global_head.py:59-64), [N, D]."""
    E.require_gpu(pooled, weight, bias)
    pooled = pooled.contiguous().float()
    rows, dim = pooled.shape
    y = torch.empty_like(pooled)
    ws = torch.empty(int(E.lib().rr_head_workspace_bytes(rows, dim)) // 4 + 1, dtype=torch.float32,
                     device=pooled.device) if whiten else None
    w = weight.contiguous().float() if whiten else None
    b = bias.contiguous().float() if (whiten and bias is not None) else None
    E.check(E.lib().rr_head_l2n_whiten_l2n(E.ptr(pooled), rows, dim, E.ptr(w), E.ptr(b), int(bool(whiten)),
                                           float(eps), E.ptr(y), E.ptr(ws), _st()), "rr_head_l2n_whiten_l2n")
    return y


def whitenapply_rows(x, m, P, d_out):
    """x [N, D] float32 rows, m [D] / P [>= d_out, D] float64 (GPU) ->
    L2N(P[:d_out] (x - m)) [N, d_out] float32, computed in float64 on the f64
    MFMA (cirtorch/utils/whiten.py:4-12)."""
    E.require_gpu(x, m, P)
    x = x.contiguous().float()
    m = m.contiguous().double().reshape(-1)
    P = P.contiguous().double()
    rows, dim = x.shape
    if dim % 16:
        # the f64 MFMA kernel takes 16-wide K-steps: zero columns of x, m and P
        # add exact zeros to every dot product (any D, like the numpy reference)
        pad = 16 - dim % 16
        x = torch.nn.functional.pad(x, (0, pad))
        m = torch.nn.functional.pad(m, (0, pad))
        P = torch.nn.functional.pad(P, (0, pad))
        dim += pad
    y = torch.empty((rows, d_out), dtype=torch.float32, device=x.device)
    ws = _workspace(E.lib().rr_whiten_workspace_bytes(rows, d_out), x.device)
    E.check(E.lib().rr_whitenapply(E.ptr(x), rows, dim, E.ptr(m), E.ptr(P), int(d_out), E.ptr(y), E.ptr(ws),
                                   ws.numel(), _st()), "rr_whitenapply")
    return y


# ---------------------------------------------------------------- matching
def knn_workspace_bytes(n_db, nq, d, k, cand=0, dtype=torch.float32):
    return int(E.lib().rr_knn_workspace_bytes(int(n_db), int(nq), int(d), int(k), int(cand), E.dtype_code(dtype)))


def knn_topk(db, db_f32, q, q_f32, k, cand=0, idx_offset=0, workspace=None, db_norm_max=None, i8_scales=None):
    """db/q: [n, D] rows in the screening dtype (float32, bfloat16, float16 or int8);
    db_f32/q_f32: the float32 rows used for the exact re-score.
    Returns (scores float64 [Q, k], idx int64 [Q, k]); with db_norm_max (the
    largest database row norm) also int32 [Q] flags: 1 where the screening
    margin could not be certified (rr_knn_topk_checked).  int8 screening is
    certified with i8_scales = (query max|x| [Q] or [1], database max|x| [1])
    (rr_knn_topk_checked_i8); without them every int8 query is flagged."""
    E.require_gpu(db, db_f32, q, q_f32)
    assert db.dtype == q.dtype and db_f32.dtype == torch.float32 and q_f32.dtype == torch.float32
    for t in (db, db_f32, q, q_f32):
        assert t.is_contiguous()
    if i8_scales is not None and (db_norm_max is None or db.dtype != torch.int8):
        raise ValueError("knn_topk: i8_scales apply to the certified int8 search only "
                         "(int8 rows with db_norm_max); they would be ignored here")
    n_db, d = db.shape
    nq = q.shape[0]
    need = knn_workspace_bytes(n_db, nq, d, k, cand, db.dtype)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, db.device)
    out_s = torch.empty((nq, k), dtype=torch.float64, device=db.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=db.device)
    if db_norm_max is None:
        E.check(E.lib().rr_knn_topk(E.ptr(db), E.ptr(db_f32), n_db, E.ptr(q), E.ptr(q_f32), nq, d, k, int(cand),
                                    int(idx_offset), E.ptr(out_s), E.ptr(out_i), E.ptr(workspace),
                                    workspace.numel(), E.dtype_code(db.dtype), _st()), "rr_knn_topk")
        return out_s, out_i
    unc = torch.empty(nq, dtype=torch.int32, device=db.device)
    if i8_scales is not None:
        qa, da = i8_scales
        assert qa.dtype == torch.float32 and da.dtype == torch.float32 and qa.numel() in (1, nq)
        E.check(E.lib().rr_knn_topk_checked_i8(E.ptr(db), E.ptr(db_f32), n_db, E.ptr(q), E.ptr(q_f32), nq, d, k,
                                               int(cand), int(idx_offset), E.ptr(out_s), E.ptr(out_i),
                                               E.ptr(workspace), workspace.numel(), float(db_norm_max), E.ptr(qa),
                                               int(qa.numel() == nq and nq > 1), E.ptr(da), E.ptr(unc), _st()),
                "rr_knn_topk_checked_i8")
        return out_s, out_i, unc
    E.check(E.lib().rr_knn_topk_checked(E.ptr(db), E.ptr(db_f32), n_db, E.ptr(q), E.ptr(q_f32), nq, d, k, int(cand),
                                        int(idx_offset), E.ptr(out_s), E.ptr(out_i), E.ptr(workspace),
                                        workspace.numel(), E.dtype_code(db.dtype), float(db_norm_max), E.ptr(unc),
                                        _st()), "rr_knn_topk_checked")
    return out_s, out_i, unc


def rank_full(db_f32, q_f32):
    """db_f32 [n, D], q_f32 [Q, D] float32 rows (D % 256 == 0) -> int64 [Q, n]: every
    database row per query by (float64 score desc, index asc) (rr_rank_full)."""
    E.require_gpu(db_f32, q_f32)
    assert db_f32.dtype == torch.float32 and q_f32.dtype == torch.float32
    assert db_f32.is_contiguous() and q_f32.is_contiguous() and db_f32.shape[1] == q_f32.shape[1]
    n, d = db_f32.shape
    nq = q_f32.shape[0]
    ws = _workspace(E.lib().rr_rank_workspace_bytes(n, nq), db_f32.device)
    out = torch.empty((nq, n), dtype=torch.int64, device=db_f32.device)
    E.check(E.lib().rr_rank_full(E.ptr(db_f32), n, E.ptr(q_f32), nq, d, E.ptr(out), E.ptr(ws), ws.numel(), _st()),
            "rr_rank_full")
    return out


def topk_merge(scores, idx, k):
    """scores/idx: [R, Q, k_in] per-shard lists -> merged [Q, k]."""
    E.require_gpu(scores, idx)
    r, nq, k_in = scores.shape
    out_s = torch.empty((nq, k), dtype=torch.float64, device=scores.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=scores.device)
    E.check(E.lib().rr_topk_merge(E.ptr(scores.contiguous()), E.ptr(idx.contiguous()), r, nq, k_in, k,
                                  E.ptr(out_s), E.ptr(out_i), _st()), "rr_topk_merge")
    return out_s, out_i


def fill_unit_rows(rows, d, seed, row0=0, device=None):
    out = torch.empty((rows, d), dtype=torch.float32, device=device or "cuda")
    E.check(E.lib().rr_fill_unit_rows(E.ptr(out), int(rows), int(d), ctypes.c_ulonglong(seed), int(row0), _st()),
            "rr_fill_unit_rows")
    return out


def cast_bf16(x):
    E.require_gpu(x)
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    E.check(E.lib().rr_cast_f32_bf16(E.ptr(x), E.ptr(y), x.numel(), _st()), "rr_cast_f32_bf16")
    return y


def cast_f16(x):
    """float32 -> IEEE fp16 (round to nearest even): the kNN screening copy of an
    fp16 database."""
    E.require_gpu(x)
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    E.check(E.lib().rr_cast_f32_f16(E.ptr(x), E.ptr(y), x.numel(), _st()), "rr_cast_f32_f16")
    return y


def quantize_i8(x, per_row=False, with_scale=False):
    """float32 rows -> int8 screening copy: rint(x * 127 / max|x|) clamped to +-127, the
    scale reduced on the device (no host read-back): one scale for the whole tensor (the
    database), or with per_row one per row (queries: a query's screened candidates then
    do not depend on the other queries of its batch).  with_scale: also return the
    float32 max |x| ([1] or [rows]) -- the certificate's quantisation scale."""
    E.require_gpu(x)
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.int8, device=x.device)
    if per_row:
        rows, d = x.shape
        if d % 4:
            raise RuntimeError("quantize_i8: row length must be a multiple of 4")
        amax = torch.empty(rows, dtype=torch.float32, device=x.device)
        E.check(E.lib().rr_quantize_i8_rows(E.ptr(x), rows, d, E.ptr(y), E.ptr(amax), _st()), "rr_quantize_i8_rows")
    else:
        if x.numel() % 4:
            raise RuntimeError("quantize_i8: element count must be a multiple of 4")
        amax = torch.empty(1, dtype=torch.float32, device=x.device)
        E.check(E.lib().rr_quantize_i8(E.ptr(x), x.numel(), E.ptr(y), E.ptr(amax), _st()), "rr_quantize_i8")
    return (y, amax) if with_scale else y


def cast_screen(x, dtype):
    """float32 rows -> the screening dtype's copy (the rows themselves for float32)."""
    if dtype == torch.float32:
        return x
    if dtype == torch.int8:
        return quantize_i8(x)
    if dtype == torch.bfloat16:
        return cast_bf16(x)
    if dtype == torch.float16:
        return cast_f16(x)
    raise RuntimeError("unsupported screening dtype %s" % dtype)


# ---------------------------------------------------------------- local descriptors
def local_head(x, kpts, weight, bias):
    """x: [N, C, H, W] feature map (channels_last view or NHWC-able, f32/bf16), kpts [N, P, 2]
    normalised (x, y) -> normalize(Linear(grid_sample(x, kpts))) as [N, P, E] float32
    (cirtorch/modules/heads/local_head.py:43-71)."""
    E.require_gpu(x, kpts, weight, bias)
    n, c, h, w = x.shape
    xh = x.permute(0, 2, 3, 1)
    if not xh.is_contiguous():
        xh = xh.contiguous()
    if xh.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        xh = xh.float()
    kp = kpts.contiguous().float()
    npts = kp.shape[1]
    wt = weight.contiguous().float()
    b = bias.contiguous().float() if bias is not None else None
    e = wt.shape[0]
    out = torch.empty((n, npts, e), dtype=torch.float32, device=x.device)
    ws = _workspace(E.lib().rr_local_head_workspace_bytes(n * npts, c, e), x.device)
    E.check(E.lib().rr_local_head(E.ptr(xh), n, h, w, c, E.dtype_code(xh.dtype), E.ptr(kp), npts, E.ptr(wt), E.ptr(b),
                                  e, E.ptr(out), E.ptr(ws), ws.numel(), _st()), "rr_local_head")
    return out


def mutual_nn(nn12, nn21):
    """int64 top-1 lists of both directions -> match [n1] (-1 where not mutual)."""
    E.require_gpu(nn12, nn21)
    a, b = nn12.contiguous().long(), nn21.contiguous().long()
    out = torch.empty_like(a)
    E.check(E.lib().rr_mutual_nn(E.ptr(a), a.numel(), E.ptr(b), b.numel(), E.ptr(out), _st()), "rr_mutual_nn")
    return out


# ---------------------------------------------------------------- batched local matching
MATCH_MODES = {"nn": E.RR_MATCH_NN, "mnn": E.RR_MATCH_MNN, "snn": E.RR_MATCH_SNN, "smnn": E.RR_MATCH_SMNN}


def _match_args(a, a_off, b, b_off, max_n1, max_n2):
    E.require_gpu(a, a_off, b, b_off)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise RuntimeError("match: descriptors must be [rows, D] with one D, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if a.dtype != torch.float32 or b.dtype != torch.float32 or not a.is_contiguous() or not b.is_contiguous():
        raise RuntimeError("match: descriptors must be contiguous float32 rows")
    if a_off.dtype != torch.int64 or b_off.dtype != torch.int64 or a_off.numel() != b_off.numel() or a_off.numel() < 1:
        raise RuntimeError("match: offsets must be int64 [P + 1] for both sides")
    rows1, rows2 = a.shape[0], b.shape[0]
    max_n1 = rows1 if max_n1 is None else min(int(max_n1), rows1)
    max_n2 = rows2 if max_n2 is None else min(int(max_n2), rows2)
    return rows1, rows2, a_off.numel() - 1, a.shape[1], max_n1, max_n2


def match_top2(a, a_off, b, b_off, max_n1=None, max_n2=None):
    """rr_match_top2: a [rows1, D], b [rows2, D] float32 rows, device int64 offsets [P + 1] ->
    (d12 float64 [rows1, 2], i12 int32 [rows1, 2], d21 [rows2, 2], i21 [rows2, 2]); rows outside
    every pair keep (+inf, -1).  No synchronisation."""
    rows1, rows2, npairs, d, max_n1, max_n2 = _match_args(a, a_off, b, b_off, max_n1, max_n2)
    dev = a.device
    d12 = torch.full((rows1, 2), float("inf"), dtype=torch.float64, device=dev)
    d21 = torch.full((rows2, 2), float("inf"), dtype=torch.float64, device=dev)
    i12 = torch.full((rows1, 2), -1, dtype=torch.int32, device=dev)
    i21 = torch.full((rows2, 2), -1, dtype=torch.int32, device=dev)
    ws = _workspace(E.lib().rr_match_workspace_bytes(rows1, rows2, 0), dev)
    E.check(E.lib().rr_match_top2(E.ptr(a), E.ptr(a_off), rows1, E.ptr(b), E.ptr(b_off), rows2, npairs, d, max_n1,
                                  max_n2, E.ptr(d12), E.ptr(i12), E.ptr(d21), E.ptr(i21), E.ptr(ws), ws.numel(),
                                  _st()), "rr_match_top2")
    return d12, i12, d21, i21


def match_pairs(a, a_off, b, b_off, mode, th=0.8, max_n1=None, max_n2=None, covered=False):
    """rr_match_pairs: -> (match int64 [rows1], dist float32 [rows1]) by the rule of `mode`
    ("nn", "mnn", "snn", "smnn").  covered=True: the pairs cover every row of a (the outputs are
    not pre-filled with -1 / inf).  No synchronisation."""
    if mode not in MATCH_MODES:
        raise ValueError("match mode %r (one of nn, mnn, snn, smnn)" % (mode,))
    rows1, rows2, npairs, d, max_n1, max_n2 = _match_args(a, a_off, b, b_off, max_n1, max_n2)
    dev = a.device
    if covered and npairs and max_n1:
        match = torch.empty(rows1, dtype=torch.int64, device=dev)
        dist = torch.empty(rows1, dtype=torch.float32, device=dev)
    else:
        match = torch.full((rows1,), -1, dtype=torch.int64, device=dev)
        dist = torch.full((rows1,), float("inf"), dtype=torch.float32, device=dev)
    ws = _workspace(E.lib().rr_match_workspace_bytes(rows1, rows2, 1), dev)
    E.check(E.lib().rr_match_pairs(E.ptr(a), E.ptr(a_off), rows1, E.ptr(b), E.ptr(b_off), rows2, npairs, d, max_n1,
                                   max_n2, MATCH_MODES[mode], float(th), E.ptr(match), E.ptr(dist), E.ptr(ws),
                                   ws.numel(), _st()), "rr_match_pairs")
    return match, dist


# ---------------------------------------------------------------- spatial verification
VERIFY_MODELS = {"homography": ("rr_verify_workspace_bytes", "rr_verify_pairs"),
                 "fundamental": ("rr_verify_epipolar_workspace_bytes", "rr_verify_pairs_epipolar"),
                 "essential": ("rr_verify_essential_workspace_bytes", "rr_verify_pairs_essential")}


def _pair_args(prefix, kp1, off1, kp2, off2, match, max_n1):
    """the checks of every entry on float32 keypoints, offsets and a match list -> rows1, rows2, P, max_n1"""
    if kp1.dim() != 2 or kp2.dim() != 2 or kp1.shape[1] != 2 or kp2.shape[1] != 2:
        raise RuntimeError("%s: keypoints must be [rows, 2], got %s and %s" % (prefix, tuple(kp1.shape), tuple(kp2.shape)))
    if kp1.dtype != torch.float32 or kp2.dtype != torch.float32 or not kp1.is_contiguous() or not kp2.is_contiguous():
        raise RuntimeError("%s: keypoints must be contiguous float32 rows" % prefix)
    if off1.dtype != torch.int64 or off2.dtype != torch.int64 or off1.numel() != off2.numel() or off1.numel() < 1:
        raise RuntimeError("%s: offsets must be int64 [P + 1] for both sides" % prefix)
    rows1, rows2, npairs = kp1.shape[0], kp2.shape[0], off1.numel() - 1
    if match.dtype != torch.int64 or match.dim() != 1 or match.shape[0] != rows1 or not match.is_contiguous():
        raise RuntimeError("%s: match must be contiguous int64 [rows1]" % prefix)
    return rows1, rows2, npairs, rows1 if max_n1 is None else min(int(max_n1), rows1)


def _point_set_args(prefix, pts1, pts2, off, weights=None, mats=(), names=None, mat_shape=None):
    """the checks of every entry on float64 point sets [rows, 2] x 2 with offsets [P + 1] -> rows, P.
    weights: per-row float64 or None; mats: per-pair float64 [P, *mat_shape] the messages call `names`"""
    if pts1.dim() != 2 or pts1.shape[1] != 2 or pts1.shape != pts2.shape:
        raise RuntimeError("%s: points must be [rows, 2] on both sides, got %s and %s" % (prefix, tuple(pts1.shape), tuple(pts2.shape)))
    if any(t.dtype != torch.float64 or not t.is_contiguous() for t in (pts1, pts2) + tuple(mats)):
        raise RuntimeError("%s: points%s must be contiguous float64%s" % (prefix, " and " + names if mats else "", "" if mats else " rows"))
    rows, npairs = pts1.shape[0], off.numel() - 1
    if weights is not None and (weights.dtype != torch.float64 or weights.shape != (rows,) or not weights.is_contiguous()):
        raise RuntimeError("%s: weights must be contiguous float64 [rows]" % prefix)
    if off.dtype != torch.int64 or off.numel() < 1 or any(tuple(m.shape) != (npairs,) + tuple(mat_shape) for m in mats):
        raise RuntimeError("%s: offsets int64 [P + 1] and %s [P, %d, %d]" % ((prefix, names) + tuple(mat_shape)) if mats
                           else "%s: offsets must be int64 [P + 1]" % prefix)
    return rows, npairs


def verify_pairs(kp1, off1, kp2, off2, match, th=3.0, iters=1024, refine=2, seed=0, max_n1=None, covered=False,
                 model="homography", K1=None, K2=None):
    """rr_verify_pairs (model "homography") / rr_verify_pairs_epipolar ("fundamental") /
    rr_verify_pairs_essential ("essential", with the intrinsics K1, K2 float64 [P, 3, 3]): kp1 [rows1, 2],
    kp2 [rows2, 2] float32 pixel keypoints, device int64 offsets [P + 1], match int64 [rows1]
    (rr_match_pairs' output) -> (inliers int32 [P], H, F or E float64 [P, 3, 3], mask uint8 [rows1]).
    covered=True: the pairs cover every side-1 row (the mask is not pre-filled with 0).  No synchronisation."""
    ws_bytes, entry = VERIFY_MODELS[model]
    calibrated = model == "essential"
    if calibrated != (K1 is not None and K2 is not None) or (K1 is None) != (K2 is None):
        raise RuntimeError("verify: K1 and K2 go with model 'essential' and with no other model")
    E.require_gpu(kp1, off1, kp2, off2, match, K1, K2)
    rows1, rows2, npairs, max_n1 = _pair_args("verify", kp1, off1, kp2, off2, match, max_n1)
    dev = kp1.device
    mats = ()   # the intrinsics go between max_n1 and th in the calibrated entry
    if calibrated:
        for m, what in ((K1, "K1"), (K2, "K2")):
            if m.dtype != torch.float64 or tuple(m.shape) != (npairs, 3, 3) or not m.is_contiguous():
                raise RuntimeError("verify: %s must be contiguous float64 [P, 3, 3], got %s %s" % (what, m.dtype, tuple(m.shape)))
        mats = (E.ptr(K1), E.ptr(K2))
    inliers = torch.empty(npairs, dtype=torch.int32, device=dev)   # written for every pair
    H = torch.empty((npairs, 3, 3), dtype=torch.float64, device=dev)
    mask = (torch.empty if covered and npairs else torch.zeros)(rows1, dtype=torch.uint8, device=dev)
    ws = _workspace(getattr(E.lib(), ws_bytes)(rows1, npairs, int(iters)), dev)
    E.check(getattr(E.lib(), entry)(E.ptr(kp1), E.ptr(off1), rows1, E.ptr(kp2), E.ptr(off2), rows2, E.ptr(match),
                                    npairs, max_n1, *mats, float(th), int(iters), int(refine),
                                    int(seed) & 0xFFFFFFFFFFFFFFFF, E.ptr(inliers), E.ptr(H), E.ptr(mask), E.ptr(ws),
                                    ws.numel(), _st()), entry)
    return inliers, H, mask


def _fit_batch(entry, prefix, pts1, pts2, weights, off):
    """one of the two batched fits: pts1, pts2 float64 [rows, 2], weights float64 [rows] or None,
    device int64 offsets [P + 1] -> float64 [P, 3, 3].  No synchronisation."""
    E.require_gpu(pts1, pts2, weights, off)
    rows, npairs = _point_set_args(prefix, pts1, pts2, off, weights)
    M = torch.empty((npairs, 3, 3), dtype=torch.float64, device=pts1.device)
    E.check(getattr(E.lib(), entry)(E.ptr(pts1), E.ptr(pts2), E.ptr(weights), E.ptr(off), rows, npairs, E.ptr(M),
                                    E.ptr(None), 0, _st()), entry)
    return M


def homography_dlt(pts1, pts2, weights, off):
    """rr_homography_dlt: pts1, pts2 float64 [rows, 2], weights float64 [rows] or None, device int64
    offsets [P + 1] -> H float64 [P, 3, 3] (find_homography_dlt per point set).  No synchronisation."""
    return _fit_batch("rr_homography_dlt", "dlt", pts1, pts2, weights, off)


def fundamental_dlt(pts1, pts2, weights, off):
    """rr_fundamental_dlt: the arguments of homography_dlt -> F float64 [P, 3, 3] (find_fundamental
    per point set; zeros for a set of fewer than 8 points).  No synchronisation."""
    return _fit_batch("rr_fundamental_dlt", "fundamental", pts1, pts2, weights, off)


def essential_5pt(x1, x2):
    """rr_essential_5pt: x1, x2 float64 [n, 5, 2] normalised points -> (E float64 [n, 10, 3, 3] in ascending
    root order, zeros past nroots; nroots int32 [n]).  No synchronisation."""
    E.require_gpu(x1, x2)
    if x1.dim() != 3 or tuple(x1.shape[1:]) != (5, 2) or x1.shape != x2.shape:
        raise RuntimeError("five-point: points must be [n, 5, 2] on both sides, got %s and %s" % (tuple(x1.shape), tuple(x2.shape)))
    if x1.dtype != torch.float64 or x2.dtype != torch.float64 or not x1.is_contiguous() or not x2.is_contiguous():
        raise RuntimeError("five-point: points must be contiguous float64")
    n = x1.shape[0]
    Em = torch.empty((n, 10, 3, 3), dtype=torch.float64, device=x1.device)
    nroots = torch.empty(n, dtype=torch.int32, device=x1.device)
    E.check(E.lib().rr_essential_5pt(E.ptr(x1), E.ptr(x2), n, E.ptr(Em), E.ptr(nroots), _st()), "rr_essential_5pt")
    return Em, nroots


EPI_KINDS = {"sampson": E.RR_EPI_SAMPSON, "symmetrical": E.RR_EPI_SYMMETRICAL}


def epipolar_distance(pts1, pts2, F, off, kind, squared=True, eps=1e-8):
    """rr_epipolar_distance: pts1, pts2 float64 [rows, 2], F float64 [P, 3, 3], device int64 offsets
    [P + 1] covering every row -> float64 [rows].  No synchronisation."""
    E.require_gpu(pts1, pts2, F, off)
    rows, npairs = _point_set_args("epipolar distance", pts1, pts2, off, mats=(F,), names="F", mat_shape=(3, 3))
    out = torch.empty(rows, dtype=torch.float64, device=pts1.device)
    E.check(E.lib().rr_epipolar_distance(E.ptr(pts1), E.ptr(pts2), E.ptr(F), E.ptr(off), rows, npairs, EPI_KINDS[kind],
                                         1 if squared else 0, float(eps), E.ptr(out), _st()), "rr_epipolar_distance")
    return out


# ---------------------------------------------------------------- relative pose
def _mat33(m, npairs, what):
    if m.dtype != torch.float64 or tuple(m.shape) != (npairs, 3, 3) or not m.is_contiguous():
        raise RuntimeError("pose: %s must be contiguous float64 [P, 3, 3], got %s %s" % (what, m.dtype, tuple(m.shape)))


def recover_pose(kp1, off1, kp2, off2, match, mask, F, K1, K2, max_n1=None, covered=False):
    """rr_recover_pose: the keypoints, offsets and match of verify_pairs, mask uint8 / bool [rows1] or
    None, F, K1, K2 float64 [P, 3, 3] -> (R [P, 3, 3], t [P, 3], E [P, 3, 3] float64, front int32 [P],
    points3d float64 [rows1, 3], front_mask uint8 [rows1]).  covered=True: the pairs cover every
    side-1 row (the per-row outputs are not pre-filled with 0).  No synchronisation."""
    E.require_gpu(kp1, off1, kp2, off2, match, mask, F, K1, K2)
    rows1, rows2, npairs, max_n1 = _pair_args("pose", kp1, off1, kp2, off2, match, max_n1)
    if mask is not None:
        if mask.dtype not in (torch.uint8, torch.bool) or tuple(mask.shape) != (rows1,) or not mask.is_contiguous():
            raise RuntimeError("pose: mask must be contiguous uint8 or bool [rows1]")
    for m, what in ((F, "F"), (K1, "K1"), (K2, "K2")):
        _mat33(m, npairs, what)
    dev = kp1.device
    new = torch.empty if covered and npairs else torch.zeros
    R = torch.empty((npairs, 3, 3), dtype=torch.float64, device=dev)   # written for every pair
    t = torch.empty((npairs, 3), dtype=torch.float64, device=dev)
    Em = torch.empty((npairs, 3, 3), dtype=torch.float64, device=dev)
    front = torch.empty(npairs, dtype=torch.int32, device=dev)
    pts = new((rows1, 3), dtype=torch.float64, device=dev)
    fmask = new(rows1, dtype=torch.uint8, device=dev)
    E.check(E.lib().rr_recover_pose(E.ptr(kp1), E.ptr(off1), rows1, E.ptr(kp2), E.ptr(off2), rows2, E.ptr(match),
                                    E.ptr(mask), E.ptr(F), E.ptr(K1), E.ptr(K2), npairs, max_n1, E.ptr(R), E.ptr(t),
                                    E.ptr(Em), E.ptr(front), E.ptr(pts), E.ptr(fmask), E.ptr(None), 0, _st()),
            "rr_recover_pose")
    return R, t, Em, front, pts, fmask


def triangulate_points(pts1, pts2, P1, P2, off):
    """rr_triangulate_points: pts1, pts2 float64 [rows, 2], P1, P2 float64 [P, 3, 4], device int64
    offsets [P + 1] covering every row -> X float64 [rows, 3].  No synchronisation."""
    E.require_gpu(pts1, pts2, P1, P2, off)
    rows, npairs = _point_set_args("triangulate", pts1, pts2, off, mats=(P1, P2), names="projections", mat_shape=(3, 4))
    X = torch.empty((rows, 3), dtype=torch.float64, device=pts1.device)
    E.check(E.lib().rr_triangulate_points(E.ptr(pts1), E.ptr(pts2), E.ptr(P1), E.ptr(P2), E.ptr(off), rows, npairs,
                                          E.ptr(X), _st()), "rr_triangulate_points")
    return X


def essential_decompose(Em):
    """rr_essential_decompose: E float64 [n, 3, 3] -> (R1, R2 [n, 3, 3], t [n, 3]) float64.  No synchronisation."""
    E.require_gpu(Em)
    if Em.dtype != torch.float64 or Em.dim() != 3 or tuple(Em.shape[1:]) != (3, 3) or not Em.is_contiguous():
        raise RuntimeError("essential: E must be contiguous float64 [n, 3, 3], got %s %s" % (Em.dtype, tuple(Em.shape)))
    n = Em.shape[0]
    R1, R2 = torch.empty_like(Em), torch.empty_like(Em)
    t = torch.empty((n, 3), dtype=torch.float64, device=Em.device)
    E.check(E.lib().rr_essential_decompose(E.ptr(Em), n, E.ptr(R1), E.ptr(R2), E.ptr(t), _st()), "rr_essential_decompose")
    return R1, R2, t


# ---------------------------------------------------------------- localization (absolute pose)
def localize_pairs(kp1, off1, pts3d, valid, off2, match, K, th=3.0, iters=1024, refine=2, seed=0, max_n1=None, covered=False):
    """rr_localize_pairs: kp1 [rows1, 2] float32 pixel keypoints, pts3d float64 [rows2, 3], valid uint8 / bool
    [rows2] or None, device int64 offsets [P + 1], match int64 [rows1], K float64 [P, 3, 3] ->
    (inliers int32 [P], R float64 [P, 3, 3], t float64 [P, 3], mask uint8 [rows1]).  covered=True: the
    pairs cover every side-1 row (the mask is not pre-filled with 0).  No synchronisation."""
    E.require_gpu(kp1, off1, pts3d, valid, off2, match, K)
    if kp1.dim() != 2 or kp1.shape[1] != 2 or kp1.dtype != torch.float32 or not kp1.is_contiguous():
        raise RuntimeError("localize: keypoints must be contiguous float32 [rows1, 2], got %s %s" % (kp1.dtype, tuple(kp1.shape)))
    if pts3d.dim() != 2 or pts3d.shape[1] != 3 or pts3d.dtype != torch.float64 or not pts3d.is_contiguous():
        raise RuntimeError("localize: points3d must be contiguous float64 [rows2, 3], got %s %s" % (pts3d.dtype, tuple(pts3d.shape)))
    if off1.dtype != torch.int64 or off2.dtype != torch.int64 or off1.numel() != off2.numel() or off1.numel() < 1:
        raise RuntimeError("localize: offsets must be int64 [P + 1] for both sides")
    rows1, rows2, npairs = kp1.shape[0], pts3d.shape[0], off1.numel() - 1
    if match.dtype != torch.int64 or match.dim() != 1 or match.shape[0] != rows1 or not match.is_contiguous():
        raise RuntimeError("localize: match must be contiguous int64 [rows1]")
    if valid is not None and (valid.dtype not in (torch.uint8, torch.bool) or tuple(valid.shape) != (rows2,)
                              or not valid.is_contiguous()):
        raise RuntimeError("localize: valid must be contiguous uint8 or bool [rows2]")
    if K.dtype != torch.float64 or tuple(K.shape) != (npairs, 3, 3) or not K.is_contiguous():
        raise RuntimeError("localize: K must be contiguous float64 [P, 3, 3], got %s %s" % (K.dtype, tuple(K.shape)))
    max_n1 = rows1 if max_n1 is None else min(int(max_n1), rows1)
    dev = kp1.device
    inliers = torch.empty(npairs, dtype=torch.int32, device=dev)   # written for every pair
    R = torch.empty((npairs, 3, 3), dtype=torch.float64, device=dev)
    t = torch.empty((npairs, 3), dtype=torch.float64, device=dev)
    mask = (torch.empty if covered and npairs else torch.zeros)(rows1, dtype=torch.uint8, device=dev)
    ws = _workspace(E.lib().rr_localize_workspace_bytes(rows1, npairs, int(iters)), dev)
    E.check(E.lib().rr_localize_pairs(E.ptr(kp1), E.ptr(off1), rows1, E.ptr(pts3d), E.ptr(valid), E.ptr(off2), rows2,
                                      E.ptr(match), npairs, max_n1, E.ptr(K), float(th), int(iters), int(refine),
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, E.ptr(inliers), E.ptr(R), E.ptr(t), E.ptr(mask),
                                      E.ptr(ws), ws.numel(), _st()), "rr_localize_pairs")
    return inliers, R, t, mask


def p3p(x, X):
    """rr_p3p: x float64 [n, 3, 2] normalised image points, X float64 [n, 3, 3] -> (R float64 [n, 4, 3, 3],
    t float64 [n, 4, 3] in ascending root order, zeros past nsol; nsol int32 [n]).  No synchronisation."""
    E.require_gpu(x, X)
    if x.dim() != 3 or tuple(x.shape[1:]) != (3, 2) or X.dim() != 3 or tuple(X.shape[1:]) != (3, 3) or x.shape[0] != X.shape[0]:
        raise RuntimeError("p3p: points must be [n, 3, 2] and [n, 3, 3], got %s and %s" % (tuple(x.shape), tuple(X.shape)))
    if x.dtype != torch.float64 or X.dtype != torch.float64 or not x.is_contiguous() or not X.is_contiguous():
        raise RuntimeError("p3p: points must be contiguous float64")
    n = x.shape[0]
    R = torch.empty((n, 4, 3, 3), dtype=torch.float64, device=x.device)
    t = torch.empty((n, 4, 3), dtype=torch.float64, device=x.device)
    nsol = torch.empty(n, dtype=torch.int32, device=x.device)
    E.check(E.lib().rr_p3p(E.ptr(x), E.ptr(X), n, E.ptr(R), E.ptr(t), E.ptr(nsol), _st()), "rr_p3p")
    return R, t, nsol


# ---------------------------------------------------------------- keypoint detection
RESPONSES = {"harris": E.RR_RESP_HARRIS, "gftt": E.RR_RESP_GFTT, "hessian": E.RR_RESP_HESSIAN}
NMS_SIZES = (3, 5, 7, 9)


def _detect_input(x, what):
    E.require_gpu(x)
    if x.dim() != 4:
        raise ValueError("%s: expected [B, C, H, W], got %s" % (what, tuple(x.shape)))
    if x.dtype not in (torch.float32, torch.uint8):
        raise TypeError("%s: images are float32 or uint8, got %s" % (what, x.dtype))
    if x.shape[2] < 4 or x.shape[3] < 4:
        raise ValueError("%s: H and W must be at least 4, got %s" % (what, tuple(x.shape)))
    return x.contiguous()


def _detect_sigmas(sigmas, n):
    if sigmas is None:
        return None
    E.require_gpu(sigmas)
    if sigmas.dim() != 1 or sigmas.shape[0] != n:
        raise ValueError("sigmas must be [B], got %s" % (tuple(sigmas.shape),))
    return sigmas.float().contiguous()


def response(x, kind, k=0.04, sigmas=None, gray=False):
    """rr_response: x [B, C, H, W] float32 or uint8 -> float32 scores [B, C, H, W] (gray=True:
    C == 3 reduced to gray first, [B, 1, H, W]).  kind: "harris" (with k), "gftt", "hessian".
    No synchronisation."""
    if kind not in RESPONSES:
        raise ValueError("response %r (one of harris, gftt, hessian)" % (kind,))
    x = _detect_input(x, "response")
    n, c, h, w = x.shape
    if gray and c != 3:
        raise ValueError("response: gray needs C == 3, got %d" % c)
    sg = _detect_sigmas(sigmas, n)
    out = torch.empty((n, 1 if gray else c, h, w), dtype=torch.float32, device=x.device)
    E.check(E.lib().rr_response(E.ptr(x), n, c, h, w, int(x.dtype == torch.uint8), int(bool(gray)), RESPONSES[kind],
                                float(k), E.ptr(sg), E.ptr(out), _st()), "rr_response")
    return out


def nms2d(x, ks, mask_only=False):
    """rr_nms2d: float32 planes [..., H, W], square window ks in (3, 5, 7, 9) -> bool mask or
    x * mask of the same shape.  No synchronisation."""
    E.require_gpu(x)
    if x.dim() < 2 or x.dtype != torch.float32:
        raise RuntimeError("nms2d: float32 planes [..., H, W], got %s %s" % (x.dtype, tuple(x.shape)))
    if ks not in NMS_SIZES:
        raise ValueError("nms2d: window %r (one of 3, 5, 7, 9)" % (ks,))
    x = x.contiguous()
    h, w = x.shape[-2:]
    planes = x.numel() // (h * w) if h * w else 0
    out = torch.empty(x.shape, dtype=torch.uint8 if mask_only else torch.float32, device=x.device)
    E.check(E.lib().rr_nms2d(E.ptr(x), planes, h, w, int(ks), int(bool(mask_only)), E.ptr(out), _st()), "rr_nms2d")
    return out.view(torch.bool) if mask_only else out


def _select_args(num, ks, min_score, border):
    if ks not in NMS_SIZES:
        raise ValueError("keypoints: nms window %r (one of 3, 5, 7, 9)" % (ks,))
    if not 1 <= int(num) <= 8192:
        raise ValueError("keypoints: num_features = %r outside [1, 8192]" % (num,))
    if int(border) < 0 or float(min_score) != float(min_score):
        raise ValueError("keypoints: border >= 0 and a min_score that is not NaN, got %r, %r" % (border, min_score))


def select_keypoints(score, num, ks=5, min_score=0.0, border=0):
    """rr_select_keypoints: score [B, H, W] float32 -> (kpts float32 [B, num, 2] pixel (x, y), scores
    float32 [B, num], count int32 [B]); the slots past count hold (-1, -1) and 0.  No synchronisation."""
    E.require_gpu(score)
    if score.dim() != 3 or score.dtype != torch.float32:
        raise RuntimeError("select_keypoints: score must be float32 [B, H, W], got %s %s" % (score.dtype, tuple(score.shape)))
    _select_args(num, ks, min_score, border)
    score = score.contiguous()
    n, h, w = score.shape
    dev = score.device
    kpts = torch.empty((n, num, 2), dtype=torch.float32, device=dev)
    scores = torch.empty((n, num), dtype=torch.float32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    ws = _workspace(E.lib().rr_detect_workspace_bytes(n, h, w, int(num)), dev)
    E.check(E.lib().rr_select_keypoints(E.ptr(score), n, h, w, int(ks), int(num), float(min_score), int(border),
                                        E.ptr(kpts), E.ptr(scores), E.ptr(count), E.ptr(ws), ws.numel(), _st()),
            "rr_select_keypoints")
    return kpts, scores, count


def detect_keypoints(x, num, kind="harris", k=0.04, ks=5, min_score=0.0, border=0, sigmas=None, return_response=False):
    """rr_detect_keypoints: x [B, 1|3, H, W] float32 or uint8 -> (kpts, scores, count) as
    select_keypoints, plus the score map [B, 1, H, W] on request.  No synchronisation."""
    if kind not in RESPONSES:
        raise ValueError("response %r (one of harris, gftt, hessian)" % (kind,))
    x = _detect_input(x, "detect_keypoints")
    n, c, h, w = x.shape
    if c not in (1, 3):
        raise ValueError("detect_keypoints: images are [B, 1, H, W] or [B, 3, H, W], got C = %d" % c)
    _select_args(num, ks, min_score, border)
    sg = _detect_sigmas(sigmas, n)
    dev = x.device
    kpts = torch.empty((n, num, 2), dtype=torch.float32, device=dev)
    scores = torch.empty((n, num), dtype=torch.float32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    smap = torch.empty((n, 1, h, w), dtype=torch.float32, device=dev) if return_response else None
    ws = _workspace(E.lib().rr_detect_workspace_bytes(n, h, w, int(num)), dev)
    E.check(E.lib().rr_detect_keypoints(E.ptr(x), n, c, h, w, int(x.dtype == torch.uint8), RESPONSES[kind], float(k),
                                        E.ptr(sg), int(ks), int(num), float(min_score), int(border), E.ptr(kpts),
                                        E.ptr(scores), E.ptr(count), E.ptr(smap), E.ptr(ws), ws.numel(), _st()),
            "rr_detect_keypoints")
    return (kpts, scores, count, smap) if return_response else (kpts, scores, count)


# ---------------------------------------------------------------- scale-space detection
SS_RESPONSES = dict(RESPONSES, dog=E.RR_RESP_DOG)


def pyramid_plan(n, h, w, levels=3, sigma=1.6, min_size=15):
    """The host arithmetic of ScalePyramid (the rule of rr_scale_pyramid in include/rr.h): a list of
    octaves, each a dict with h, w, off (floats from the start of the pyramid buffer), sigmas (one
    per level) and blurs ((ksize, sigma) per level; level 0 of octave 0 holds the first blur or None)."""
    import math
    L = levels + 3
    step = 2 ** (1. / float(levels))
    cur = 0.5
    first = None
    if sigma > cur:
        s0 = max(math.sqrt(sigma ** 2 - cur ** 2), 0.01)
        k0 = int(2.0 * 4.0 * s0 + 1.0)
        first = (k0 + 1 if k0 % 2 == 0 else k0, s0)
        cur = sigma
    octs, off = [], 0
    while True:
        o = dict(h=h, w=w, off=off, sigmas=[cur], blurs=[first if not octs else None])
        for _ in range(1, L):
            s = cur * math.sqrt(step ** 2 - 1.0)
            ks = int(2.0 * 4.0 * s + 1.0)
            if ks % 2 == 0:
                ks += 1
            ks = min(ks, min(h, w))
            if ks % 2 == 0:
                ks += 1
            cur *= step
            o["sigmas"].append(cur)
            o["blurs"].append((ks, s))
        octs.append(o)
        off += (n * L * h * w + 63) // 64 * 64
        h, w = h // 2, w // 2
        cur = sigma
        if min(h, w) <= min_size:
            break
    return octs


def _pyr_input(x, what):
    E.require_gpu(x)
    if x.dim() != 4 or x.shape[1] not in (1, 3):
        raise ValueError("%s: images are [B, 1, H, W] or [B, 3, H, W], got %s" % (what, tuple(x.shape)))
    if x.dtype not in (torch.float32, torch.uint8):
        raise TypeError("%s: images are float32 or uint8, got %s" % (what, x.dtype))
    return x.contiguous()


def _pyr_views(buf, n, L, octs):
    return [buf[o["off"]:o["off"] + n * L * o["h"] * o["w"]].view(n, 1, L, o["h"], o["w"]) for o in octs]


def gaussian_blur(x, ksize, sigma):
    """rr_gaussian_blur: float32 planes [..., H, W], reflect borders -> the same shape.  No synchronisation."""
    E.require_gpu(x)
    if x.dim() < 2 or x.dtype != torch.float32:
        raise RuntimeError("gaussian_blur: float32 planes [..., H, W], got %s %s" % (x.dtype, tuple(x.shape)))
    x = x.contiguous()
    h, w = x.shape[-2:]
    planes = x.numel() // (h * w) if h * w else 0
    out = torch.empty_like(x)
    E.check(E.lib().rr_gaussian_blur(E.ptr(x), planes, h, w, int(ksize), float(sigma), E.ptr(out), _st()), "rr_gaussian_blur")
    return out


def scale_pyramid(x, levels=3, sigma=1.6, min_size=15):
    """rr_scale_pyramid: x [B, 1|3, H, W] float32 or uint8 -> (views [B, 1, L, h_o, w_o] of one float32
    buffer, one per octave; the plan of pyramid_plan).  No synchronisation."""
    x = _pyr_input(x, "scale_pyramid")
    n, c, h, w = x.shape
    ob, wb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    args = (int(levels), float(sigma), int(min_size))
    E.check(E.lib().rr_scale_pyramid_bytes(n, c, h, w, *args, ctypes.byref(ob), ctypes.byref(wb)), "rr_scale_pyramid_bytes")
    out = torch.empty(ob.value // 4, dtype=torch.float32, device=x.device)
    ws = _workspace(wb.value, x.device)
    E.check(E.lib().rr_scale_pyramid(E.ptr(x), n, c, h, w, int(x.dtype == torch.uint8), *args, E.ptr(out), ob.value,
                                     E.ptr(ws), ws.numel(), _st()), "rr_scale_pyramid")
    octs = pyramid_plan(n, h, w, *args)
    return _pyr_views(out, n, int(levels) + 3, octs), octs


def dog_response(levels):
    """rr_dog_response: float32 [B, L, H, W] -> [B, L - 1, H, W].  No synchronisation."""
    E.require_gpu(levels)
    if levels.dim() != 4 or levels.dtype != torch.float32:
        raise RuntimeError("dog_response: float32 levels [B, L, H, W], got %s %s" % (levels.dtype, tuple(levels.shape)))
    levels = levels.contiguous()
    n, L, h, w = levels.shape
    if L < 2:
        raise ValueError("dog_response: at least two levels, got %d" % L)
    out = torch.empty((n, L - 1, h, w), dtype=torch.float32, device=levels.device)
    E.check(E.lib().rr_dog_response(E.ptr(levels), n, L, h, w, E.ptr(out), _st()), "rr_dog_response")
    return out


def scale_space_extrema(x, minima=False):
    """rr_scale_space_extrema: a float32 volume [B, D, H, W] -> (mask uint8 [B, D, H, W]: 1 maximum,
    2 minimum; offsets float32 [B, 3, D, H, W] in the order (level, x, y); values float32 [B, D, H, W]).
    No synchronisation."""
    E.require_gpu(x)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise RuntimeError("scale_space_extrema: a float32 volume [B, D, H, W], got %s %s" % (x.dtype, tuple(x.shape)))
    x = x.contiguous()
    n, D, h, w = x.shape
    mask = torch.empty((n, D, h, w), dtype=torch.uint8, device=x.device)
    offs = torch.empty((n, 3, D, h, w), dtype=torch.float32, device=x.device)
    vals = torch.empty((n, D, h, w), dtype=torch.float32, device=x.device)
    E.check(E.lib().rr_scale_space_extrema(E.ptr(x), n, D, h, w, int(bool(minima)), E.ptr(mask), E.ptr(offs), E.ptr(vals),
                                           _st()), "rr_scale_space_extrema")
    return mask, offs, vals


def _ss_args(num, mr_size):
    if not 1 <= int(num) <= 8192:
        raise ValueError("keypoints: num_features = %r outside [1, 8192]" % (num,))
    if not float(mr_size) > 0:
        raise ValueError("keypoints: mr_size = %r must be positive" % (mr_size,))


def _ss_outputs(n, num, dev):
    return (torch.empty((n, num, 2, 3), dtype=torch.float32, device=dev), torch.empty((n, num), dtype=torch.float32, device=dev),
            torch.empty(n, dtype=torch.int32, device=dev))


def scale_space_select(resp, n, h, w, num, levels=3, sigma=1.6, min_size=15, minima=False, mr_size=6.0):
    """rr_scale_space_select: resp, a float32 buffer in the pyramid's layout for n images of h x w ->
    (lafs float32 [n, num, 2, 3], scores [n, num], count int32 [n]).  No synchronisation."""
    E.require_gpu(resp)
    _ss_args(num, mr_size)
    args = (int(levels), float(sigma), int(min_size))
    need = pyramid_plan(n, h, w, *args)[-1]
    if resp.dtype != torch.float32 or resp.dim() != 1 or resp.numel() < need["off"] + n * (args[0] + 3) * need["h"] * need["w"]:
        raise RuntimeError("scale_space_select: resp must be the flat float32 buffer of the pyramid's layout")
    lafs, scores, count = _ss_outputs(n, int(num), resp.device)
    ws = _workspace(E.lib().rr_detect_scale_space_workspace_bytes(n, 1, h, w, *args), resp.device)
    E.check(E.lib().rr_scale_space_select(E.ptr(resp), n, h, w, *args, int(bool(minima)), float(mr_size), int(num), E.ptr(lafs),
                                          E.ptr(scores), E.ptr(count), E.ptr(ws), ws.numel(), _st()), "rr_scale_space_select")
    return lafs, scores, count


def detect_scale_space(x, num, kind="hessian", levels=3, sigma=1.6, min_size=15, mr_size=6.0, minima=False, k=0.04,
                       return_pyramid=False):
    """rr_detect_scale_space: x [B, 1|3, H, W] float32 or uint8 -> (lafs float32 [B, num, 2, 3] in image
    pixels, scores [B, num], count int32 [B]); with return_pyramid also the views of the pyramid the
    call left at the start of its workspace.  No synchronisation."""
    if kind not in SS_RESPONSES:
        raise ValueError("response %r (one of harris, gftt, hessian, dog)" % (kind,))
    _ss_args(num, mr_size)
    x = _pyr_input(x, "detect_scale_space")
    n, c, h, w = x.shape
    args = (int(levels), float(sigma), int(min_size))
    lafs, scores, count = _ss_outputs(n, int(num), x.device)
    ws = _workspace(E.lib().rr_detect_scale_space_workspace_bytes(n, c, h, w, *args), x.device)
    E.check(E.lib().rr_detect_scale_space(E.ptr(x), n, c, h, w, int(x.dtype == torch.uint8), *args, SS_RESPONSES[kind],
                                          float(k), int(bool(minima)), float(mr_size), int(num), E.ptr(lafs), E.ptr(scores),
                                          E.ptr(count), E.ptr(ws), ws.numel(), _st()), "rr_detect_scale_space")
    if not return_pyramid:
        return lafs, scores, count
    pad = (-ws.data_ptr()) % 256
    octs = pyramid_plan(n, h, w, *args)
    total = octs[-1]["off"] + n * (args[0] + 3) * octs[-1]["h"] * octs[-1]["w"]
    buf = ws[pad:pad + 4 * total].view(torch.float32)
    return lafs, scores, count, _pyr_views(buf, n, args[0] + 3, octs)


# ---------------------------------------------------------------- keypoint description
PATCH_SIZES = (8, 64)


def sift_geometry(patch_size, num_spatial_bins):
    """(ksize, stride, pad) of get_sift_bin_ksize_stride_pad, or None when the pair is incompatible"""
    ksize = 2 * int(patch_size / (num_spatial_bins + 1))
    stride = patch_size // num_spatial_bins
    pad = ksize // 4
    if ksize < 1 or stride < 1 or (patch_size + 2 * pad - (ksize - 1) - 1) // stride + 1 != num_spatial_bins:
        return None
    return ksize, stride, pad


def _no_grad(what, *tensors):
    for t in tensors:
        if t is not None and t.requires_grad:
            raise RuntimeError("%s: gradients are not supported (the kernels have no backward pass); detach the input" % what)


def _describe_image(x, what):
    E.require_gpu(x)
    if x.dim() != 4:
        raise ValueError("%s: expected [B, C, H, W], got %s" % (what, tuple(x.shape)))
    if x.dtype not in (torch.float32, torch.uint8):
        raise TypeError("%s: images are float32 or uint8, got %s" % (what, x.dtype))
    return x.contiguous()


def _patch_size(ps, what):
    if not PATCH_SIZES[0] <= int(ps) <= PATCH_SIZES[1]:
        raise ValueError("%s: patch size %r outside [8, 64]" % (what, ps))
    return int(ps)


def _patches(patches, what):
    E.require_gpu(patches)
    _no_grad(what, patches)
    if patches.dim() < 2 or not patches.is_floating_point() or patches.shape[-1] != patches.shape[-2]:
        raise RuntimeError("%s: floating-point square patches [..., PS, PS], got %s %s" % (what, patches.dtype, tuple(patches.shape)))
    return patches.float().contiguous()   # the kernels read float32 (the reference also takes float64)


def extract_patches(x, lafs, ps=32, gray=False):
    """rr_extract_patches: x [B, C, H, W] float32 or uint8, lafs [B, N, 2, 3] float32 pixels ->
    float32 [B, N, C, ps, ps] ([B, N, 1, ps, ps] with gray=True, C == 3).  No synchronisation."""
    x = _describe_image(x, "extract_patches")
    E.require_gpu(lafs)
    _no_grad("extract_patches", x, lafs)
    n, c, h, w = x.shape
    if lafs.dim() != 4 or lafs.shape[0] != n or tuple(lafs.shape[2:]) != (2, 3):
        raise ValueError("extract_patches: lafs must be [%d, N, 2, 3], got %s" % (n, tuple(lafs.shape)))
    if gray and c != 3:
        raise ValueError("extract_patches: gray needs C == 3, got %d" % c)
    ps = _patch_size(ps, "extract_patches")
    lafs = lafs.float().contiguous()
    npts = lafs.shape[1]
    out = torch.empty((n, npts, 1 if gray else c, ps, ps), dtype=torch.float32, device=x.device)
    E.check(E.lib().rr_extract_patches(E.ptr(x), n, c, h, w, int(x.dtype == torch.uint8), int(bool(gray)), E.ptr(lafs),
                                       npts, ps, E.ptr(out), _st()), "rr_extract_patches")
    return out


def patch_orientation(patches, num_ang_bins=36):
    """rr_patch_orientation: float32 patches [..., ps, ps] -> angles [...] in radians.  No synchronisation."""
    patches = _patches(patches, "patch_orientation")
    ps = _patch_size(patches.shape[-1], "patch_orientation")
    if not 1 <= int(num_ang_bins) <= 64:
        raise ValueError("patch_orientation: num_ang_bins = %r outside [1, 64]" % (num_ang_bins,))
    lead = patches.shape[:-2]
    out = torch.empty(lead, dtype=torch.float32, device=patches.device)
    E.check(E.lib().rr_patch_orientation(E.ptr(patches), out.numel(), ps, int(num_ang_bins), E.ptr(out), _st()),
            "rr_patch_orientation")
    return out


def _sift_args(ps, num_ang_bins, num_spatial_bins, what):
    if not 1 <= int(num_ang_bins) <= 16:
        raise ValueError("%s: num_ang_bins = %r outside [1, 16]" % (what, num_ang_bins))
    if not 1 <= int(num_spatial_bins) <= 8:
        raise ValueError("%s: num_spatial_bins = %r outside [1, 8]" % (what, num_spatial_bins))
    if sift_geometry(ps, int(num_spatial_bins)) is None:
        raise ValueError("%s: patch size %d is incompatible with %d spatial bins" % (what, ps, num_spatial_bins))
    return int(num_ang_bins), int(num_spatial_bins)


def sift_describe(patches, num_ang_bins=8, num_spatial_bins=4, rootsift=True, clipval=0.2):
    """rr_sift_describe: float32 patches [..., ps, ps] -> descriptors [..., num_ang_bins * ns^2].
    No synchronisation."""
    patches = _patches(patches, "sift_describe")
    ps = _patch_size(patches.shape[-1], "sift_describe")
    nb, ns = _sift_args(ps, num_ang_bins, num_spatial_bins, "sift_describe")
    lead = tuple(patches.shape[:-2])
    out = torch.empty(lead + (nb * ns * ns,), dtype=torch.float32, device=patches.device)
    B = patches.numel() // (ps * ps)
    E.check(E.lib().rr_sift_describe(E.ptr(patches), B, ps, nb, ns, int(bool(rootsift)), float(clipval), E.ptr(out), _st()),
            "rr_sift_describe")
    return out


def pyramid_levels(h, w, ps):
    """[(h_l, w_l)] of levels 0 .. last_level of the patch pyramid: level l is (h >> l, w >> l) while
    its smaller side is at least ps (level 0 always exists).  Host arithmetic, as rr_patch_pyramid_bytes."""
    out = [(int(h), int(w))]
    while min(out[-1][0] // 2, out[-1][1] // 2) >= ps:
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


def pyrdown(x):
    """rr_pyrdown: float32 [B, C, H, W], H, W >= 3 -> [B, C, H // 2, W // 2].  No synchronisation."""
    E.require_gpu(x)
    _no_grad("pyrdown", x)
    if x.dim() != 4:
        raise ValueError("Invalid input shape, we expect BxCxHxW. Got: {}".format(tuple(x.shape)))
    if not x.is_floating_point():
        raise TypeError("pyrdown: a floating-point image, got %s" % x.dtype)
    n, c, h, w = x.shape
    if h < 3 or w < 3:
        raise ValueError("pyrdown: H and W must be at least 3 (reflect padding by 2), got %d x %d" % (h, w))
    x = x.float().contiguous()
    out = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    E.check(E.lib().rr_pyrdown(E.ptr(x), n, c, h, w, E.ptr(out), _st()), "rr_pyrdown")
    return out


def patch_pyramid(x, ps=32, gray=False):
    """rr_patch_pyramid: levels 1 .. last of x [B, C, H, W] float32 or uint8 as a list of float32
    [B, C or 1, H_l, W_l] views of one buffer (empty when the image has no level 1), and the buffer."""
    x = _describe_image(x, "patch_pyramid")
    _no_grad("patch_pyramid", x)
    n, c, h, w = x.shape
    if gray and c != 3:
        raise ValueError("patch_pyramid: gray needs C == 3, got %d" % c)
    ps = _patch_size(ps, "patch_pyramid")
    co = 1 if gray else c
    nbytes = int(E.lib().rr_patch_pyramid_bytes(n, co, h, w, ps, None))
    buf = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=x.device)
    E.check(E.lib().rr_patch_pyramid(E.ptr(x), n, c, h, w, int(x.dtype == torch.uint8), int(bool(gray)), ps, E.ptr(buf), nbytes,
                                     _st()), "rr_patch_pyramid")
    views, off = [], 0
    for hl, wl in pyramid_levels(h, w, ps)[1:] if n else []:
        views.append(buf[off:off + n * co * hl * wl].view(n, co, hl, wl))
        off += n * co * hl * wl
    return views, buf


def extract_patches_pyramid(x, lafs, ps=32, gray=False, return_levels=False, pyr=None):
    """rr_patch_pyramid + rr_extract_patches_pyramid: as extract_patches, every frame from its pyramid
    level, a frame past the last level from the last.  With return_levels also the unclamped levels
    int32 [B, N] and the flag int32 [1] (1 when a frame was clamped).  pyr: the buffer patch_pyramid
    returned for the same (x, ps, gray).  No synchronisation."""
    x = _describe_image(x, "extract_patches_pyramid")
    E.require_gpu(lafs)
    _no_grad("extract_patches_pyramid", x, lafs)
    n, c, h, w = x.shape
    if lafs.dim() != 4 or lafs.shape[0] != n or tuple(lafs.shape[2:]) != (2, 3):
        raise ValueError("extract_patches_pyramid: lafs must be [%d, N, 2, 3], got %s" % (n, tuple(lafs.shape)))
    if gray and c != 3:
        raise ValueError("extract_patches_pyramid: gray needs C == 3, got %d" % c)
    ps = _patch_size(ps, "extract_patches_pyramid")
    lafs = lafs.float().contiguous()
    npts = lafs.shape[1]
    if pyr is None:
        pyr = patch_pyramid(x, ps, gray)[1]
    out = torch.empty((n, npts, 1 if gray else c, ps, ps), dtype=torch.float32, device=x.device)
    levels = torch.empty((n, npts), dtype=torch.int32, device=x.device) if return_levels else None
    flag = torch.empty(1, dtype=torch.int32, device=x.device) if return_levels else None
    E.check(E.lib().rr_extract_patches_pyramid(E.ptr(x), n, c, h, w, int(x.dtype == torch.uint8), int(bool(gray)), E.ptr(pyr),
                                               E.ptr(lafs), npts, ps, E.ptr(out), E.ptr(levels), E.ptr(flag), _st()),
            "rr_extract_patches_pyramid")
    return (out, levels, flag) if return_levels else out


def describe_keypoints(x, kpts=None, count=None, scale=12.0, lafs=None, orient=False, orient_bins=36, ps=32, num_ang_bins=8,
                       num_spatial_bins=4, rootsift=True, clipval=0.2, return_lafs=False, pyramid=False):
    """rr_describe_keypoints (rr_describe_keypoints_pyramid with pyramid): x [B, 1|3, H, W] float32 or
    uint8, kpts [B, N, 2] pixel (x, y) (or
    lafs [B, N, 2, 3]), count int32 [B] or None -> (desc float32 [B, N, dim], angles float32 [B, N])
    and, with return_lafs, the described frames [B, N, 2, 3].  No synchronisation."""
    x = _describe_image(x, "describe_keypoints")
    n, c, h, w = x.shape
    if c not in (1, 3):
        raise ValueError("describe_keypoints: images are [B, 1, H, W] or [B, 3, H, W], got C = %d" % c)
    E.require_gpu(kpts, count, lafs)
    _no_grad("describe_keypoints", x, kpts, lafs)
    if lafs is not None:
        if lafs.dim() != 4 or lafs.shape[0] != n or tuple(lafs.shape[2:]) != (2, 3):
            raise ValueError("describe_keypoints: lafs must be [%d, N, 2, 3], got %s" % (n, tuple(lafs.shape)))
        lafs = lafs.float().contiguous()
        npts = lafs.shape[1]
        kpts = None
    else:
        if kpts is None or kpts.dim() != 3 or kpts.shape[0] != n or kpts.shape[2] != 2:
            raise ValueError("describe_keypoints: kpts must be [%d, N, 2], got %s"
                             % (n, None if kpts is None else tuple(kpts.shape)))
        kpts = kpts.float().contiguous()
        npts = kpts.shape[1]
        if not (float(scale) > 0.0 and float(scale) != float("inf")):
            raise ValueError("describe_keypoints: scale must be positive and finite, got %r" % (scale,))
    if count is not None:
        if count.dim() != 1 or count.shape[0] != n or count.dtype != torch.int32:
            raise ValueError("describe_keypoints: count must be int32 [%d], got %s %s" % (n, count.dtype, tuple(count.shape)))
        count = count.contiguous()
    ps = _patch_size(ps, "describe_keypoints")
    nb, ns = _sift_args(ps, num_ang_bins, num_spatial_bins, "describe_keypoints")
    if orient and not 1 <= int(orient_bins) <= 64:
        raise ValueError("describe_keypoints: orientation bins = %r outside [1, 64]" % (orient_bins,))
    dev = x.device
    desc = torch.empty((n, npts, nb * ns * ns), dtype=torch.float32, device=dev)
    angles = torch.empty((n, npts), dtype=torch.float32, device=dev)
    lafs_out = torch.empty((n, npts, 2, 3), dtype=torch.float32, device=dev) if return_lafs else None
    if pyramid:
        ws = _workspace(E.lib().rr_describe_pyramid_workspace_bytes(n, c, h, w, npts, ps, nb, ns), dev)
        E.check(E.lib().rr_describe_keypoints_pyramid(E.ptr(x), n, c, h, w, int(x.dtype == torch.uint8), E.ptr(kpts), E.ptr(count),
                                                      npts, float(scale), E.ptr(lafs), int(bool(orient)), int(orient_bins), ps, nb,
                                                      ns, int(bool(rootsift)), float(clipval), E.ptr(desc), E.ptr(angles),
                                                      E.ptr(lafs_out), E.ptr(ws), ws.numel(), _st()), "rr_describe_keypoints_pyramid")
        return (desc, angles, lafs_out) if return_lafs else (desc, angles)
    ws = _workspace(E.lib().rr_describe_workspace_bytes(n, npts, ps, nb, ns), dev)
    E.check(E.lib().rr_describe_keypoints(E.ptr(x), n, c, h, w, int(x.dtype == torch.uint8), E.ptr(kpts), E.ptr(count), npts,
                                          float(scale), E.ptr(lafs), int(bool(orient)), int(orient_bins), ps, nb, ns,
                                          int(bool(rootsift)), float(clipval), E.ptr(desc), E.ptr(angles), E.ptr(lafs_out),
                                          E.ptr(ws), ws.numel(), _st()), "rr_describe_keypoints")
    return (desc, angles, lafs_out) if return_lafs else (desc, angles)


# ---------------------------------------------------------------- affine shape
def patch_affine_shape(patches, eps=1e-10):
    """rr_patch_affine_shape: float32 patches [..., ps, ps] -> the normalised second-moment matrix
    (a, b, c) float32 [..., 3], (1, 0, 1) where two of the raw moments are below eps.  No synchronisation."""
    patches = _patches(patches, "patch_affine_shape")
    ps = _patch_size(patches.shape[-1], "patch_affine_shape")
    if not np.isfinite(float(eps)):
        raise ValueError("patch_affine_shape: eps = %r must be finite" % (eps,))
    lead = tuple(patches.shape[:-2])
    out = torch.empty(lead + (3,), dtype=torch.float32, device=patches.device)
    E.check(E.lib().rr_patch_affine_shape(E.ptr(patches), patches.numel() // (ps * ps), ps, float(eps), E.ptr(out), _st()),
            "rr_patch_affine_shape")
    return out


def ellipse_to_laf(ells):
    """rr_ellipse_to_laf: ellipses (x, y, a, b, c) [..., 5] -> float32 frames [..., 2, 3].  No synchronisation."""
    E.require_gpu(ells)
    _no_grad("ellipse_to_laf", ells)
    if ells.dim() < 1 or ells.shape[-1] != 5 or not ells.is_floating_point():
        raise RuntimeError("ellipse_to_laf: floating-point ellipses [..., 5], got %s %s" % (ells.dtype, tuple(ells.shape)))
    ells = ells.float().contiguous()
    out = torch.empty(tuple(ells.shape[:-1]) + (2, 3), dtype=torch.float32, device=ells.device)
    E.check(E.lib().rr_ellipse_to_laf(E.ptr(ells), ells.numel() // 5, E.ptr(out), _st()), "rr_ellipse_to_laf")
    return out


def laf_affine_shape(x, lafs, count=None, ps=32, eps=1e-10, out=None):
    """rr_laf_affine_shape: x [B, 1|3, H, W] float32 or uint8, lafs [B, N, 2, 3] float32 pixels, count
    int32 [B] or None -> the frames with the affine shape of their patch and their own scale and
    centre, float32 [B, N, 2, 3]; dead slots hold zeros.  out: a contiguous float32 tensor of that
    shape to write to (it may be lafs itself).  No synchronisation."""
    x = _describe_image(x, "laf_affine_shape")
    n, c, h, w = x.shape
    if c not in (1, 3):
        raise ValueError("laf_affine_shape: images are [B, 1, H, W] or [B, 3, H, W], got C = %d" % c)
    E.require_gpu(lafs, count, out)
    _no_grad("laf_affine_shape", x, lafs)
    if lafs.dim() != 4 or lafs.shape[0] != n or tuple(lafs.shape[2:]) != (2, 3):
        raise ValueError("laf_affine_shape: lafs must be [%d, N, 2, 3], got %s" % (n, tuple(lafs.shape)))
    lafs = lafs.float().contiguous()
    npts = lafs.shape[1]
    if count is not None:
        if count.dim() != 1 or count.shape[0] != n or count.dtype != torch.int32:
            raise ValueError("laf_affine_shape: count must be int32 [%d], got %s %s" % (n, count.dtype, tuple(count.shape)))
        count = count.contiguous()
    ps = _patch_size(ps, "laf_affine_shape")
    if not np.isfinite(float(eps)):
        raise ValueError("laf_affine_shape: eps = %r must be finite" % (eps,))
    if out is None:
        out = torch.empty((n, npts, 2, 3), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, npts, 2, 3) or not out.is_contiguous():
        raise ValueError("laf_affine_shape: out must be contiguous float32 [%d, %d, 2, 3]" % (n, npts))
    ws = _workspace(E.lib().rr_laf_affine_shape_workspace_bytes(n, c, h, w, npts, ps), x.device)
    E.check(E.lib().rr_laf_affine_shape(E.ptr(x), n, c, h, w, int(x.dtype == torch.uint8), E.ptr(lafs), E.ptr(count), npts, ps,
                                        float(eps), E.ptr(out), E.ptr(ws), ws.numel(), _st()), "rr_laf_affine_shape")
    return out


# ---------------------------------------------------------------- learned patch descriptors
PATCHNET_VARIANTS = {"hardnet": E.RR_PATCHNET_HARDNET, "sosnet": E.RR_PATCHNET_SOSNET}
PATCHNET_SHAPES = ((32, 1, 3), (32, 32, 3), (64, 32, 3), (64, 64, 3), (128, 64, 3), (128, 128, 3), (128, 128, 8))


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def patchnet_pack(weights, means, variances):
    """rr_patchnet_pack: the seven conv weights [cout, cin, k, k] and running_mean / running_var
    [cout] of the trunk -> the packed device blob (uint8).  No synchronisation."""
    if not (len(weights) == len(means) == len(variances) == 7):
        raise ValueError("patchnet_pack: seven weights, means and variances")
    E.require_gpu(*weights, *means, *variances)
    keep = []
    for group in (weights, means, variances):
        keep.append([t.detach().float().contiguous() for t in group])
    for (co, ci, k), w, m, v in zip(PATCHNET_SHAPES, *keep):
        if tuple(w.shape) != (co, ci, k, k) or tuple(m.shape) != (co,) or tuple(v.shape) != (co,):
            raise ValueError("patchnet_pack: expected weight %s with statistics [%d], got %s, %s, %s"
                             % ((co, ci, k, k), co, tuple(w.shape), tuple(m.shape), tuple(v.shape)))
    nbytes = int(E.lib().rr_patchnet_packed_bytes())
    packed = torch.empty(nbytes, dtype=torch.uint8, device=keep[0][0].device)
    E.check(E.lib().rr_patchnet_pack(_ptr_array(keep[0]), _ptr_array(keep[1]), _ptr_array(keep[2]), E.ptr(packed), nbytes, _st()),
            "rr_patchnet_pack")
    return packed


def _patchnet_patches(patches, what):
    patches = _patches(patches, what)
    if tuple(patches.shape[-2:]) != (32, 32):
        raise ValueError("%s: patches are 32 x 32, got %s" % (what, tuple(patches.shape)))
    return patches, patches.numel() // 1024


def patchnet_trunk(patches, packed, variant):
    """rr_patchnet_trunk: float32 patches [..., 32, 32] -> the layer-6 maps fp16 [B, 8, 8, 128].  No synchronisation."""
    patches, B = _patchnet_patches(patches, "patchnet_trunk")
    out = torch.empty((B, 8, 8, 128), dtype=torch.float16, device=patches.device)
    E.check(E.lib().rr_patchnet_trunk(E.ptr(patches), B, PATCHNET_VARIANTS[variant], E.ptr(packed), E.ptr(out), _st()),
            "rr_patchnet_trunk")
    return out


def patchnet_head(maps, packed, variant):
    """rr_patchnet_head: maps fp16 [B, 8, 8, 128] -> descriptors float32 [B, 128].  No synchronisation."""
    E.require_gpu(maps)
    if maps.dtype != torch.float16 or maps.dim() != 4 or tuple(maps.shape[1:]) != (8, 8, 128):
        raise ValueError("patchnet_head: maps are fp16 [B, 8, 8, 128], got %s %s" % (maps.dtype, tuple(maps.shape)))
    maps = maps.contiguous()
    out = torch.empty((maps.shape[0], 128), dtype=torch.float32, device=maps.device)
    E.check(E.lib().rr_patchnet_head(E.ptr(maps), maps.shape[0], PATCHNET_VARIANTS[variant], E.ptr(packed), E.ptr(out), _st()),
            "rr_patchnet_head")
    return out


def patchnet_describe(patches, packed, variant, out=None):
    """rr_patchnet_describe: float32 patches [..., 32, 32] -> descriptors float32 [B, 128] (into out, a
    contiguous float32 [B, 128], when given).  No synchronisation."""
    patches, B = _patchnet_patches(patches, "patchnet_describe")
    if out is None:
        out = torch.empty((B, 128), dtype=torch.float32, device=patches.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, 128) or not out.is_contiguous():
        raise ValueError("patchnet_describe: out must be contiguous float32 [%d, 128]" % B)
    ws = _workspace(E.lib().rr_patchnet_workspace_bytes(B), patches.device)
    E.check(E.lib().rr_patchnet_describe(E.ptr(patches), B, PATCHNET_VARIANTS[variant], E.ptr(packed), E.ptr(out), E.ptr(ws),
                                         ws.numel(), _st()), "rr_patchnet_describe")
    return out
