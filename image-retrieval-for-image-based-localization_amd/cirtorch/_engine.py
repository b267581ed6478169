"""ctypes binding of librr.so (the C ABI in include/rr.h).

This is the only place the Python host touches native code.  Tensors cross
the boundary as raw device pointers + sizes; the stream is PyTorch's current
HIP stream, so every call is asynchronous and ordered with torch work.

There is deliberately no CPU fallback: if librr.so cannot be loaded, or a
tensor is not on the GPU, the call raises.
"""

import contextlib
import ctypes
import os
import threading

import torch

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("RR_LIB", os.path.join(PKG_DIR, "librr.so"))

RR_F32, RR_BF16, RR_F16, RR_I8 = 0, 1, 2, 3
RR_ACT_IDENTITY, RR_ACT_LEAKY = 0, 1
RR_POOL_GEM, RR_POOL_MAC, RR_POOL_SPOC = 0, 1, 2
RR_CONV_AFFINE, RR_CONV_RESIDUAL, RR_CONV_PERM32 = 1, 2, 4
RR_NHWC, RR_NCHW = 0, 1
RR_MATCH_NN, RR_MATCH_MNN, RR_MATCH_SNN, RR_MATCH_SMNN = 0, 1, 2, 3
RR_RESP_HARRIS, RR_RESP_GFTT, RR_RESP_HESSIAN, RR_RESP_DOG = 0, 1, 2, 3
RR_EPI_SAMPSON, RR_EPI_SYMMETRICAL = 0, 1
# enum rr_tune_key, in order: RR_TUNE_<name> = index
TUNE_KEYS = ("GEMM_CONFIG", "GEMM_STAGES", "GEMM_WIDE", "GEMM_ASTAT", "GEMM_XCD_MAP", "STREAM_1X1", "CONV3X3",
             "GRID_CUS", "GEMM8", "KNN_FUSED", "CONV3_PIPE", "STEM", "STREAM_XCD", "CONV3S", "WRES", "PAIR_MID",
             "WRES_RING")
globals().update(("RR_TUNE_" + name, key) for key, name in enumerate(TUNE_KEYS))
# enum rr_tune_size_key: the keys that set a length, RR_TUNE_<name> = number
TUNE_SIZE_KEYS = {"PATCHNET_CHUNK": 32}
globals().update(("RR_TUNE_" + name, key) for name, key in TUNE_SIZE_KEYS.items())
RR_PATCHNET_HARDNET, RR_PATCHNET_SOSNET = 0, 1

_DTYPE_CODE = {torch.float32: RR_F32, torch.bfloat16: RR_BF16, torch.float16: RR_F16,
               torch.int8: RR_I8}  # RR_I8: kNN screening only


class ConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("n", "h", "w", "c_in", "ho", "wo", "c_out", "kh", "kw", "stride",
                                            "pad", "dil", "k_packed", "ldy", "act")] + \
               [("slope", ctypes.c_float), ("flags", ctypes.c_int)]


class LaunchInfo(ctypes.Structure):
    """rr_launch_info: what the last fused-conv entry on this thread launched."""
    _fields_ = [("kernel", ctypes.c_char * 32), ("variant", ctypes.c_char * 48), ("grid", ctypes.c_uint),
                ("block", ctypes.c_uint), ("nslices", ctypes.c_int), ("xmap", ctypes.c_int), ("launches", ctypes.c_int)]


class Region(ctypes.Structure):
    """rr_region: one pooling rectangle of a stage map."""
    _fields_ = [(n, ctypes.c_uint16) for n in ("y0", "x0", "h", "w")]


_vp, _i, _ll, _f, _d, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
_SIGS = {
    "rr_version": ([], _i),
    "rr_build_info": ([], ctypes.c_char_p),
    "rr_last_error": ([], ctypes.c_char_p),
    "rr_device_arch": ([ctypes.c_char_p, _i], _i),
    "rr_image_to_nhwc": ([_vp, _i, _i, _i, _i, ctypes.POINTER(_f), ctypes.POINTER(_f), _i, _vp, _i, _i, _vp], _i),
    "rr_conv2d_fused": ([_vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(ConvDesc), _i, _i, _vp], _i),
    "rr_conv1x1_pair": ([_vp, _ll, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _i, _i, _f,
                         _vp, _vp, _i, _vp], _i),
    "rr_conv3x3_pair": ([_vp, _i, _i, _i, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _f,
                         _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _i, _vp], _i),
    "rr_pack_conv_weights": ([_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp], _i),
    "rr_stem_pack_weights": ([_vp, _i, _i, _i, _i, _vp, _i, _vp], _i),
    "rr_stem_conv_pool": ([_vp, _i, _i, _i, ctypes.POINTER(_f), ctypes.POINTER(_f), _i, _vp, _vp, _vp, _i, _f, _vp,
                           _i, _i, _i, _vp], _i),
    "rr_stem_conv_pool_u8": ([_vp, _i, _i, _i, ctypes.POINTER(_f), ctypes.POINTER(_f), _i, _vp, _vp, _vp, _i, _f,
                              _vp, _i, _i, _i, _vp], _i),
    "rr_image_to_nhwc_ragged": ([_vp, _vp, _i, _i, _i, _i, _i, ctypes.POINTER(_f), ctypes.POINTER(_f), _i, _vp, _i,
                                 _i, _vp], _i),
    "rr_stem_conv_pool_ragged": ([_vp, _vp, _i, _i, _i, _i, ctypes.POINTER(_f), ctypes.POINTER(_f), _i, _vp, _vp, _vp,
                                  _i, _f, _vp, _i, _i, _i, _vp], _i),
    "rr_pad_images": ([_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "rr_maxpool2d": ([_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _vp], _i),
    "rr_resize_bilinear": ([_vp, _i, _i, _i, _vp, _i, _i, _d, _d, _vp], _i),
    "rr_global_pool": ([_vp, _i, _i, _i, _i, _i, _f, _f, _vp, _i, _vp], _i),
    "rr_global_pool_pdev": ([_vp, _i, _i, _i, _i, _i, _f, _vp, _f, _vp, _i, _vp], _i),
    "rr_region_pool": ([_vp, _i, _i, _i, _i, ctypes.POINTER(Region), _i, _i, _f, _vp, _i, _f, _vp, _i, _vp], _i),
    "rr_region_aggregate": ([_vp, _i, _i, _i, _i, _f, _vp, _vp], _i),
    "rr_l2n_rows": ([_vp, _i, _i, _f, _vp, _vp], _i),
    "rr_linear_rows": ([_vp, _i, _i, _vp, _vp, _i, _vp, _vp], _i),
    "rr_head_workspace_bytes": ([_i, _i], _sz),
    "rr_whiten_workspace_bytes": ([_i, _i], _sz),
    "rr_whitenapply": ([_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _sz, _vp], _i),
    "rr_head_l2n_whiten_l2n": ([_vp, _i, _i, _vp, _vp, _i, _f, _vp, _vp, _vp], _i),
    "rr_knn_workspace_bytes": ([_ll, _i, _i, _i, _i, _i], _sz),
    "rr_knn_topk": ([_vp, _vp, _ll, _vp, _vp, _i, _i, _i, _i, _ll, _vp, _vp, _vp, _sz, _i, _vp], _i),
    "rr_knn_topk_checked": ([_vp, _vp, _ll, _vp, _vp, _i, _i, _i, _i, _ll, _vp, _vp, _vp, _sz, _i, _f, _vp, _vp], _i),
    "rr_topk_merge": ([_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "rr_comm_unique_id": ([_vp, _i], _i),
    "rr_comm_init": ([ctypes.POINTER(_vp), _i, _vp, _i, _i], _i),
    "rr_comm_destroy": ([_vp], _i),
    "rr_topk_allgather_workspace_bytes": ([_i, _i, _i], _sz),
    "rr_topk_allgather_merge": ([_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp], _i),
    "rr_local_head_workspace_bytes": ([_ll, _i, _i], _sz),
    "rr_local_head": ([_vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _sz, _vp], _i),
    "rr_mutual_nn": ([_vp, _i, _vp, _i, _vp, _vp], _i),
    "rr_match_workspace_bytes": ([_ll, _ll, _i], _sz),
    "rr_match_top2": ([_vp, _vp, _ll, _vp, _vp, _ll, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp], _i),
    "rr_match_pairs": ([_vp, _vp, _ll, _vp, _vp, _ll, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _sz, _vp], _i),
    "rr_verify_workspace_bytes": ([_ll, _i, _i], _sz),
    "rr_verify_pairs": ([_vp, _vp, _ll, _vp, _vp, _ll, _vp, _i, _i, _d, _i, _i, ctypes.c_ulonglong, _vp, _vp, _vp, _vp, _sz,
                         _vp], _i),
    "rr_homography_dlt": ([_vp, _vp, _vp, _vp, _ll, _i, _vp, _vp, _sz, _vp], _i),
    "rr_verify_epipolar_workspace_bytes": ([_ll, _i, _i], _sz),
    "rr_verify_pairs_epipolar": ([_vp, _vp, _ll, _vp, _vp, _ll, _vp, _i, _i, _d, _i, _i, ctypes.c_ulonglong, _vp, _vp, _vp,
                                  _vp, _sz, _vp], _i),
    "rr_fundamental_dlt": ([_vp, _vp, _vp, _vp, _ll, _i, _vp, _vp, _sz, _vp], _i),
    "rr_epipolar_distance": ([_vp, _vp, _vp, _vp, _ll, _i, _i, _i, _d, _vp, _vp], _i),
    "rr_verify_essential_workspace_bytes": ([_ll, _i, _i], _sz),
    "rr_verify_pairs_essential": ([_vp, _vp, _ll, _vp, _vp, _ll, _vp, _i, _i, _vp, _vp, _d, _i, _i, ctypes.c_ulonglong, _vp,
                                   _vp, _vp, _vp, _sz, _vp], _i),
    "rr_essential_5pt": ([_vp, _vp, _i, _vp, _vp, _vp], _i),
    "rr_recover_pose": ([_vp, _vp, _ll, _vp, _vp, _ll, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                         _vp], _i),
    "rr_triangulate_points": ([_vp, _vp, _vp, _vp, _vp, _ll, _i, _vp, _vp], _i),
    "rr_essential_decompose": ([_vp, _i, _vp, _vp, _vp, _vp], _i),
    "rr_localize_workspace_bytes": ([_ll, _i, _i], _sz),
    "rr_localize_pairs": ([_vp, _vp, _ll, _vp, _vp, _vp, _ll, _vp, _i, _i, _vp, _d, _i, _i, ctypes.c_ulonglong, _vp, _vp, _vp,
                           _vp, _vp, _sz, _vp], _i),
    "rr_p3p": ([_vp, _vp, _i, _vp, _vp, _vp, _vp], _i),
    "rr_patchnet_packed_bytes": ([], _sz),
    "rr_patchnet_pack": ([ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _sz, _vp], _i),
    "rr_patchnet_workspace_bytes": ([_ll], _sz),
    "rr_patchnet_trunk": ([_vp, _ll, _i, _vp, _vp, _vp], _i),
    "rr_patchnet_head": ([_vp, _ll, _i, _vp, _vp, _vp], _i),
    "rr_patchnet_describe": ([_vp, _ll, _i, _vp, _vp, _vp, _sz, _vp], _i),
    "rr_detect_workspace_bytes": ([_i, _i, _i, _i], _sz),
    "rr_response": ([_vp, _i, _i, _i, _i, _i, _i, _i, _d, _vp, _vp, _vp], _i),
    "rr_nms2d": ([_vp, _ll, _i, _i, _i, _i, _vp, _vp], _i),
    "rr_select_keypoints": ([_vp, _i, _i, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _sz, _vp], _i),
    "rr_detect_keypoints": ([_vp, _i, _i, _i, _i, _i, _i, _d, _vp, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp, _sz,
                             _vp], _i),
    "rr_gaussian_blur": ([_vp, _ll, _i, _i, _i, _d, _vp, _vp], _i),
    "rr_scale_pyramid_bytes": ([_i, _i, _i, _i, _i, _d, _i, ctypes.POINTER(_sz), ctypes.POINTER(_sz)], _i),
    "rr_scale_pyramid": ([_vp, _i, _i, _i, _i, _i, _i, _d, _i, _vp, _sz, _vp, _sz, _vp], _i),
    "rr_dog_response": ([_vp, _i, _i, _i, _i, _vp, _vp], _i),
    "rr_scale_space_extrema": ([_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp], _i),
    "rr_scale_space_select": ([_vp, _i, _i, _i, _i, _d, _i, _i, _d, _i, _vp, _vp, _vp, _vp, _sz, _vp], _i),
    "rr_detect_scale_space_workspace_bytes": ([_i, _i, _i, _i, _i, _d, _i], _sz),
    "rr_detect_scale_space": ([_vp, _i, _i, _i, _i, _i, _i, _d, _i, _i, _d, _i, _d, _i, _vp, _vp, _vp, _vp, _sz, _vp], _i),
    "rr_describe_workspace_bytes": ([_i, _i, _i, _i, _i], _sz),
    "rr_extract_patches": ([_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp], _i),
    "rr_patch_orientation": ([_vp, _ll, _i, _i, _vp, _vp], _i),
    "rr_sift_describe": ([_vp, _ll, _i, _i, _i, _i, _d, _vp, _vp], _i),
    "rr_describe_keypoints": ([_vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _d, _vp, _i, _i, _i, _i, _i, _i, _d, _vp, _vp, _vp,
                               _vp, _sz, _vp], _i),
    "rr_pyrdown": ([_vp, _i, _i, _i, _i, _vp, _vp], _i),
    "rr_patch_pyramid_bytes": ([_i, _i, _i, _i, _i, ctypes.POINTER(_i)], _sz),
    "rr_patch_pyramid": ([_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp], _i),
    "rr_extract_patches_pyramid": ([_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp], _i),
    "rr_describe_pyramid_workspace_bytes": ([_i, _i, _i, _i, _i, _i, _i, _i], _sz),
    "rr_describe_keypoints_pyramid": ([_vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _d, _vp, _i, _i, _i, _i, _i, _i, _d, _vp, _vp,
                                       _vp, _vp, _sz, _vp], _i),
    "rr_patch_affine_shape": ([_vp, _ll, _i, _d, _vp, _vp], _i),
    "rr_ellipse_to_laf": ([_vp, _ll, _vp, _vp], _i),
    "rr_laf_affine_shape_workspace_bytes": ([_i, _i, _i, _i, _i, _i], _sz),
    "rr_laf_affine_shape": ([_vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _i, _d, _vp, _vp, _sz, _vp], _i),
    "rr_rank_workspace_bytes":([_ll, _i], _sz),
    "rr_rank_full": ([_vp, _ll, _vp, _i, _i, _vp, _vp, _sz, _vp], _i),
    "rr_set_tuning": ([_i, _i], _i),
    "rr_get_tuning": ([_i, ctypes.POINTER(_i)], _i),
    "rr_last_launch": ([ctypes.POINTER(LaunchInfo)], _i),
    "rr_fill_unit_rows": ([_vp, _ll, _i, ctypes.c_ulonglong, _ll, _vp], _i),
    "rr_cast_f32_bf16": ([_vp, _vp, _ll, _vp], _i),
    "rr_cast_f32_f16": ([_vp, _vp, _ll, _vp], _i),
    "rr_quantize_i8": ([_vp, _ll, _vp, _vp, _vp], _i),
    "rr_quantize_i8_rows": ([_vp, _i, _i, _vp, _vp, _vp], _i),
    "rr_knn_topk_checked_i8": ([_vp, _vp, _ll, _vp, _vp, _i, _i, _i, _i, _ll, _vp, _vp, _vp, _sz, _f, _vp, _i, _vp,
                                _vp, _vp], _i),
}

_lib = None
_lock = threading.Lock()


def lib():
    """Load librr.so once; raise (never fall back) if it is missing."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError("librr.so not found at %s — build it with "
                                       "`python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
                handle = ctypes.CDLL(LIB_PATH)
                for name, (args, res) in _SIGS.items():
                    fn = getattr(handle, name)
                    fn.argtypes = args
                    fn.restype = res
                _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().rr_last_error().decode(errors="replace")
        raise RuntimeError("%s failed (rc=%d): %s" % (what, rc, msg))


def _tune_key(name):
    """'WRES', 'RR_TUNE_WRES', 'wres' or '14' -> 14."""
    name = str(name).upper()
    name = name[len("RR_TUNE_"):] if name.startswith("RR_TUNE_") else name
    if name in TUNE_KEYS:
        return TUNE_KEYS.index(name)
    if name in TUNE_SIZE_KEYS:
        return TUNE_SIZE_KEYS[name]
    try:
        return int(name)
    except ValueError:
        raise ValueError("unknown tuning key %r (one of %s, or a number)" % (name, ", ".join(TUNE_KEYS + tuple(TUNE_SIZE_KEYS))))


def get_tuning(key):
    value = ctypes.c_int()
    check(lib().rr_get_tuning(_tune_key(key), ctypes.byref(value)), "rr_get_tuning")
    return value.value


def set_tuning(key, value):
    check(lib().rr_set_tuning(_tune_key(key), int(value)), "rr_set_tuning")


def last_launch():
    """rr_last_launch as a dict: kernel ('' when the conv ran on the tiled engine or the
    8-phase GEMM), variant, grid, block, nslices, xmap, launches.  Raises if no fused conv
    has run on this thread."""
    info = LaunchInfo()
    check(lib().rr_last_launch(ctypes.byref(info)), "rr_last_launch")
    return {"kernel": info.kernel.decode(), "variant": info.variant.decode(), "grid": info.grid, "block": info.block,
            "nslices": info.nslices, "xmap": info.xmap, "launches": info.launches}


@contextlib.contextmanager
def tuning(**values):
    """with tuning(WRES=0, GEMM8=1 | 8): ... -- set the named rr_tune_key knobs for the
    body and put back the values they had, in reverse order, however the body ends."""
    saved = []
    try:
        for name, value in values.items():
            saved.append((name, get_tuning(name)))
            set_tuning(name, value)
        yield
    finally:
        for name, value in reversed(saved):
            set_tuning(name, value)


def apply_tuning_arg(arg):
    """A command line's --tune "k=v,k=v" (keys by name or number), set for the process."""
    for kv in filter(None, (arg or "").split(",")):
        key, value = kv.split("=")
        set_tuning(key.strip(), int(value, 0))


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def require_gpu(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("cirtorch (MI355X engine) operates on GPU tensors only; got a %s tensor. "
                               "Move the model and inputs to the GPU (net.cuda()); there is no CPU path." % t.device)


def dtype_code(dt):
    try:
        return _DTYPE_CODE[dt]
    except KeyError:
        raise RuntimeError("unsupported dtype %s (float32, bfloat16; float16 for kNN screening)" % dt)


def device_arch():
    buf = ctypes.create_string_buffer(64)
    check(lib().rr_device_arch(buf, 64), "rr_device_arch")
    return buf.value.decode()
