"""Pooling, head and resampling kernels against float64 at the shapes where their code paths
change: the tile, wave and block edges of k_pool_nhwc_h16x8 / k_pool_nhwc / k_pool_nchw,
k_l2n_rows, k_linear_mfma, k_whiten_f64 / k_l2n_rows_f64, k_grid_sample_nhwc / k_normalize_rows,
the two max-pool kernels and k_resize_bilinear.  Inputs are generated on the CPU, rounded to the
dtype under test, and the reference is float64 on the CPU from the rounded tensor
(tests/head_ops_cases.py).  Every test prints its largest error before it asserts."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_ops_cases as C
from head_ops_cases import BF16, F16, F32, dt_id

pytestmark = pytest.mark.gpu


def _ops():
    from cirtorch import _ops
    return _ops


def _hw_id(hw):
    return "%dx%d" % hw


# ------------------------------------------------------------------ 1. global pooling
def _pool(xd, kind, p, on_device):
    from cirtorch import _engine as E
    from cirtorch.layers import functional as LF
    if kind == "mac":
        return LF.mac(xd)
    if kind == "spoc":
        return LF.spoc(xd)
    if on_device:  # the exponent as a one-element device tensor, read by the kernel
        pt = torch.tensor([p], dtype=torch.float32, device=xd.device)
        return _ops().global_pool(xd, E.RR_POOL_GEM, pt, 1e-6).unsqueeze(-1).unsqueeze(-1)
    return LF.gem(xd, p=p)


def _check_pool(make, modes):
    """make(sign) -> the CPU map and its device twin; every mode on the positive and the
    mixed-sign map.  GeM / SPoC: rtol 1e-5, atol 1e-6 against float64; MAC: equal."""
    for sign in ("pos", "mixed"):
        x, xd = make(sign)
        n, c = x.shape[:2]
        for name, kind, p, on_device in modes:
            got = _pool(xd, kind, p, on_device)
            assert got.dtype == torch.float32 and tuple(got.shape) == (n, c, 1, 1), (name, sign)
            got = got.reshape(n, c).cpu().double()
            ref = C.pool_ref(x, kind, p)
            err = ((got - ref).abs() / (1e-6 + 1e-5 * ref.abs())).max().item()
            print("pool %s %s: max |err| / (atol + rtol |ref|) = %.3g" % (name, sign, err))
            if kind == "mac":
                assert torch.equal(got, ref), (name, sign)
            else:
                assert torch.allclose(got, ref, rtol=1e-5, atol=1e-6), (name, sign, err)


def _nhwc_maker(cuda, n, c, h, w, dtype, *key):
    def make(sign):
        x = C.pool_map(n, c, h, w, dtype, sign, True, *key)
        xd = x.to(cuda)
        assert xd.is_contiguous(memory_format=torch.channels_last)
        return x, xd
    return make


@pytest.mark.parametrize("hw", C.H16_HW, ids=_hw_id)
@pytest.mark.parametrize("dtype", [BF16, F16], ids=dt_id)
def test_pool_nhwc_16bit_every_hw(cuda, dtype, hw):
    """k_pool_nhwc_h16x8 at c = 520 (a second channel block of 8 channels): hw below, at and
    past the 16 waves, and at 49 / 64 / 65 / 130 / 207 where wave 0, then every wave, takes one
    and then several trips of the unrolled loop.  The 1x1 ids do not reach this kernel: such a
    map is also NCHW-contiguous and global_pool sends it to k_pool_nchw."""
    _check_pool(_nhwc_maker(cuda, 2, 520, hw[0], hw[1], dtype), C.POOL_MODES_SHORT)


@pytest.mark.parametrize("c", C.H16_C)
@pytest.mark.parametrize("hw", C.H16_HW_ALL_MODES, ids=_hw_id)
@pytest.mark.parametrize("dtype", [BF16, F16], ids=dt_id)
def test_pool_nhwc_16bit_modes(cuda, dtype, hw, c):
    """k_pool_nhwc_h16x8, every mode (GeM p = 3, 2, 1, 2.5 from the host, 3 and 2.5 from device
    memory, MAC, SPoC) at c = 8, 520, 1032: one lane, two and three channel blocks"""
    _check_pool(_nhwc_maker(cuda, 2, c, hw[0], hw[1], dtype), C.POOL_MODES)


@pytest.mark.parametrize("hw", C.NHWC_HW, ids=_hw_id)
@pytest.mark.parametrize("dtype,c", C.NHWC_DT_C, ids=lambda v: dt_id(v) if isinstance(v, torch.dtype) else str(v))
def test_pool_nhwc_generic(cuda, dtype, c, hw):
    """k_pool_nhwc: f32 maps, and 16-bit maps with c % 8 == 4; c below, just below and just
    past one 256-channel block, and past two.  The 1x1 ids do not reach this kernel: such a
    map is also NCHW-contiguous and global_pool sends it to k_pool_nchw."""
    _check_pool(_nhwc_maker(cuda, 2, c, hw[0], hw[1], dtype), C.POOL_MODES)


@pytest.mark.parametrize("hw", C.NHWC_HW, ids=_hw_id)
def test_pool_nhwc_bf16_base_offset_8_bytes(cuda, hw):
    """a bf16 channels_last map with c = 16 whose base pointer is 8 bytes past a 16-byte
    boundary takes k_pool_nhwc (8-byte loads, every address a multiple of 8); the 1x1 id is
    NCHW-contiguous too and goes to k_pool_nchw instead"""
    n, c, (h, w) = 2, 16, hw

    def make(sign):
        x = C.pool_map(n, c, h, w, BF16, sign, True, "offset")
        flat = torch.zeros(x.numel() + 4, dtype=BF16, device=cuda)
        flat[4:].copy_(x.permute(0, 2, 3, 1).reshape(-1))
        xd = flat[4:].view(n, h, w, c).permute(0, 3, 1, 2)
        assert xd.data_ptr() % 16 == 8 and xd.is_contiguous(memory_format=torch.channels_last)
        return x, xd
    _check_pool(make, C.POOL_MODES)


@pytest.mark.parametrize("hw", C.NCHW_HW, ids=_hw_id)
@pytest.mark.parametrize("planes", C.NCHW_PLANES)
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=dt_id)
def test_pool_nchw(cuda, dtype, planes, hw):
    """k_pool_nchw: n c = 1, 3, 5, 7 planes (a ragged last block of 4), hw around and past the
    64 lanes of the wave that owns a plane"""
    def make(sign):
        x = C.pool_map(1, planes, hw[0], hw[1], dtype, sign, False)
        return x, x.to(cuda)
    _check_pool(make, C.POOL_MODES)


# ------------------------------------------------------------------ 2. l2n
@pytest.mark.parametrize("dim", C.L2N_DIMS)
@pytest.mark.parametrize("rows", C.L2N_ROWS)
def test_l2n_rows(cuda, rows, dim):
    """k_l2n_rows against x / (||x|| + eps) in float64: dim below, at and past the 256 threads,
    a zero row (zeros) and a row of norm 1e-5 where eps = 1e-6 is a tenth of the denominator"""
    from cirtorch.layers import functional as LF
    x = C.l2n_rows_input(rows, dim)
    ref = C.l2n_ref(x, 1e-6)
    got = _ops().l2n_rows(x.to(cuda), 1e-6).cpu()
    assert got.dtype == torch.float32 and got.shape == x.shape
    err = ((got.double() - ref).abs() / (1e-7 + 2e-6 * ref.abs())).max().item()
    print("l2n rows=%d dim=%d: max |err| / (atol + rtol |ref|) = %.3g" % (rows, dim, err))
    np.testing.assert_allclose(got.double().numpy(), ref.numpy(), rtol=2e-6, atol=1e-7)
    if rows == 3:
        assert (got[1] == 0).all()
        # the reference rule is + eps, not max(||x||, eps): the two differ by a tenth here
        assert abs(got[2].double().norm().item() - 1e-5 / (1e-5 + 1e-6)) < 1e-5
    got4 = LF.l2n(x.reshape(rows, dim, 1, 1).to(cuda)).cpu()
    assert got4.shape == (rows, dim, 1, 1) and torch.equal(got4.reshape(rows, dim), got)


# ------------------------------------------------------------------ 3. linear_rows / head_tail
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("case", C.LINEAR_CASES, ids=lambda v: "%dx%d-%d" % v)
def test_linear_rows(cuda, case, bias):
    """k_linear_mfma within the elementwise float32 dot-product bound of x W^T + b: in_dim not a
    multiple of 16 (the kin guard), fewer K-blocks than the 8 waves, rows / outputs that are no
    multiple of 64 / 16, with and without bias"""
    rows, in_dim, out_dim = case
    x, w, b = C.linear_input(rows, in_dim, out_dim)
    if not bias:
        b = None
    ref, bound = C.linear_ref_and_bound(x, w, b)
    got = _ops().linear_rows(x.to(cuda), w.to(cuda), b.to(cuda) if bias else None).cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (rows, out_dim)
    err = (got.double() - ref).abs()
    print("linear %s bias=%s: max |err| / bound = %.3g" % (case, bias, (err / bound).max().item()))
    assert bool((err <= bound).all()), (err / bound).max().item()


HEAD_TAIL_PARAMS = [(rd, wh, True) for rd in C.HEAD_TAIL_CASES for wh in (True, False)] + [((2, 36), True, False)]


@pytest.mark.parametrize("rd,whiten,bias", HEAD_TAIL_PARAMS,
                         ids=["%dx%d-%s-%s" % (rd[0], rd[1], "whiten" if wh else "l2n", "bias" if b else "nobias")
                              for rd, wh, b in HEAD_TAIL_PARAMS])
def test_head_tail(cuda, rd, whiten, bias):
    """rr_head_l2n_whiten_l2n against the float64 composition L2N(W L2N(x) + b)"""
    rows, dim = rd
    x, w, b = C.head_tail_input(rows, dim)
    ref = C.head_tail_ref(x, w, b if bias else None, whiten)
    got = _ops().head_tail(x.to(cuda), w.to(cuda), b.to(cuda) if bias else None, whiten=whiten).cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (rows, dim)
    err = ((got.double() - ref).abs() / (2e-7 + 1e-5 * ref.abs())).max().item()
    print("head_tail %s whiten=%s bias=%s: max |err| / (atol + rtol |ref|) = %.3g" % (rd, whiten, bias, err))
    np.testing.assert_allclose(got.double().numpy(), ref.numpy(), rtol=1e-5, atol=2e-7)


# ------------------------------------------------------------------ 4. whitenapply_rows
@pytest.mark.parametrize("case", C.WHITEN_CASES, ids=lambda v: "%dx%d-%d" % v)
def test_whitenapply_rows(cuda, case):
    """k_whiten_f64 + k_l2n_rows_f64 against numpy float64: d_out that is no multiple of 16,
    fewer than 64 rows, fewer K-blocks than waves, and dim = 30 zero-padded by the wrapper"""
    rows, dim, d_out = case
    x, m, P = C.whiten_input(rows, dim, d_out)
    ref = C.whiten_ref(x, m, P, d_out)
    got = _ops().whitenapply_rows(torch.from_numpy(x).to(cuda), torch.from_numpy(m).to(cuda),
                                  torch.from_numpy(P).to(cuda), d_out).cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (rows, d_out)
    err = np.abs(got.double().numpy() - ref).max()
    print("whitenapply %s: max |err| = %.3g" % (case, err))
    np.testing.assert_allclose(got.double().numpy(), ref, rtol=0, atol=1e-7)


# ------------------------------------------------------------------ 5. localHead
@pytest.mark.parametrize("dtype,c", C.LOCAL_CASES, ids=lambda v: dt_id(v) if isinstance(v, torch.dtype) else str(v))
def test_local_head(cuda, dtype, c):
    """localHead on 2 x c x 5 x 7 maps against grid_sample -> Linear -> normalize in float64:
    a second pass of the channel loop (c = 520 / 260), n npts = 10 keypoints (no multiple of the
    4 per block), image 1 sampled at its own keypoints, taps inside, partly and wholly outside"""
    from cirtorch.modules.heads.local_head import localHead
    x, w, b = C.local_input(dtype, c)
    kpts = C.local_keypoints()
    assert not torch.equal(kpts[0], kpts[1]) and not torch.equal(x[0], x[1])
    ref = C.local_ref(x, kpts, w, b)
    # the keypoints two pixels outside sample zeros: their descriptor is the normalised bias
    nb = (b.double() / b.double().norm())
    assert torch.allclose(ref[0, 4], nb, rtol=0, atol=1e-12) and torch.allclose(ref[1, 4], nb, rtol=0, atol=1e-12)
    head = localHead(c, C.LOCAL_E)
    head.load_state_dict({"whiten.weight": w, "whiten.bias": b})
    head = head.to(cuda)
    xd = x.to(cuda)
    assert xd.is_contiguous(memory_format=torch.channels_last)
    got = head(xd, kpts.to(cuda)).cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, C.LOCAL_NPTS, C.LOCAL_E)
    err = (got.double() - ref).abs().max().item()
    print("local_head %s c=%d: max |err| = %.3g" % (dt_id(dtype), c, err))
    np.testing.assert_allclose(got.double().numpy(), ref.numpy(), rtol=0, atol=2e-6)


# ------------------------------------------------------------------ 6. maxpool2d
def _maxpool_id(case):
    (h, w), (k, s, p), (dt, c) = case
    return "%dx%d-k%ds%dp%d-%s-c%d" % (h, w, k, s, p, dt_id(dt), c)


@pytest.mark.parametrize("case", C.MAXPOOL_CASES, ids=_maxpool_id)
def test_maxpool2d(cuda, case):
    """both max-pool kernels equal F.max_pool2d: odd and even extents, one pixel, 3x3/2/1,
    2x2/2/0 and 3x3/1/1, c a multiple of 8 (bf16: 8 channels per thread) and not"""
    (h, w), (k, s, p), (dtype, c) = case
    x = C.maxpool_input(h, w, c, dtype)
    ref = C.maxpool_ref(x, k, s, p)
    got = _ops().maxpool2d(x.to(cuda), k, s, p).cpu()
    assert got.dtype == dtype and got.shape == ref.shape
    assert torch.equal(got.float(), ref)


@pytest.mark.parametrize("ksp", [(3, 2, 1), (3, 1, 1)], ids=lambda v: "k%ds%dp%d" % v)
@pytest.mark.parametrize("dtype,c", C.MAXPOOL_NAN_DT_C,
                         ids=lambda v: dt_id(v) if isinstance(v, torch.dtype) else str(v))
def test_maxpool2d_non_finite(cuda, dtype, c, ksp):
    """+inf, -inf and one NaN per image, in different channels: every window that holds the NaN
    is NaN (F.max_pool2d's rule; fmaxf would drop it), every other element equals torch's"""
    k, s, p = ksp
    h, w = 7, 8
    x = C.maxpool_input(h, w, c, dtype)
    # (y, x, channel) per image: NaN, +inf, -inf
    spots = [((2, 3, 0), (4, 6, 1), (0, 0, c - 1)), ((6, 7, c - 1), (1, 1, 0), (3, 4, 1))]
    for img, (nan_at, pinf_at, ninf_at) in enumerate(spots):
        x[(img,) + nan_at] = float("nan")
        x[(img,) + pinf_at] = float("inf")
        x[(img,) + ninf_at] = float("-inf")
    ref = C.maxpool_ref(x, k, s, p)
    # the windows that hold the NaN, found independently of any maximum
    holds = F.max_pool2d(torch.isnan(x).float().permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1) > 0
    assert torch.equal(torch.isnan(ref), holds) and bool(holds[0].any()) and bool(holds[1].any())
    got = _ops().maxpool2d(x.to(cuda), k, s, p).cpu()
    assert got.dtype == dtype and got.shape == ref.shape
    got = got.float()
    assert torch.equal(torch.isnan(got), holds), "windows holding a NaN: %d, NaN outputs: %d" % (
        int(holds.sum()), int(torch.isnan(got).sum()))
    assert torch.equal(got[~holds], ref[~holds])
    assert bool(torch.isinf(got).any())


# ------------------------------------------------------------------ 7. resize_bilinear
@pytest.mark.parametrize("case", C.RESIZE_CASES, ids=lambda v: "%s-s%.4g" % ("x".join(map(str, v[0])), v[1]))
def test_resize_bilinear(cuda, case):
    """k_resize_bilinear has F.interpolate's output shape and, for inputs in [0, 1], its values
    (float64, bilinear, align_corners=False) within 1e-5: tiny planes, a batch, and the scales
    of the multi-scale extraction (2^-1/2, 2^1/2) beside 0.5, 2, 0.7 and 1.  An axis whose
    extent the scale leaves unchanged is kept as it is, whatever the other axis does (2x3, 3x2
    and 2x2 at 2^1/2, 4x7 at 1.2)"""
    shape, s = case
    x = torch.rand(shape, generator=C.gen("resize", shape))
    x4 = x if x.dim() == 4 else x[None]
    ref = F.interpolate(x4.double(), scale_factor=s, mode="bilinear", align_corners=False)
    ref = ref if x.dim() == 4 else ref[0]
    got = _ops().resize_bilinear(x.to(cuda), s).cpu()
    assert got.dtype == torch.float32 and got.shape == ref.shape
    err = (got.double() - ref).abs().max().item()
    print("resize %s x %.4g: max |err| = %.3g" % (shape, s, err))
    assert err < 1e-5
    if s == 1.0:
        assert torch.equal(got, x)
