"""Regional pooling on the GPU (rr_region_pool / rr_region_aggregate, Rpool,
GeMmp, the regional globalHead and net) against the reference outputs of
tests/golden/rpool.npz and the rectangles of tests/golden/regions.npz (both
written by make_golden_regional.py from the reference modules).

Tolerances are the ones the project uses for the same operators
(test_gpu_kernels.py): rtol 2e-6 / atol 1e-7 for pooled vectors, exact for MAC,
rtol 1e-5 / atol 2e-7 after a whitening layer."""

import numpy as np
import pytest
import torch

from conftest import cosines, golden

pytestmark = pytest.mark.gpu

C = 72
SHAPES = [(7, 7), (5, 9), (9, 5), (3, 11), (1, 1), (2, 7)]
POOLS = ["gem3", "gem2.5", "mac", "spoc", "gemmp"]
POOL_TOL = dict(rtol=2e-6, atol=1e-7)
WHITEN_TOL = dict(rtol=1e-5, atol=2e-7)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


# ----------------------------------------------------------------------------- fixtures and references
_cache = {}


def G():
    if "g" not in _cache:
        _cache["g"] = golden("rpool.npz")
    return _cache["g"]


def recorded(h, w, L=3):
    """the rectangles the reference pools on an h x w map (regions.npz)"""
    if "r" not in _cache:
        g = golden("regions.npz")
        _cache["r"] = {tuple(int(v) for v in s): [tuple(int(v) for v in r) for r in g["rects"][a:b]]
                       for s, a, b in zip(g["shapes"], g["offsets"][:-1], g["offsets"][1:])}
    return _cache["r"][(h, w, L)]


def rpool_input(h, w):
    """make_golden_regional.rpool_input: regenerated from the seed, guarded by the stored checksum"""
    key = ("x", h, w)
    if key not in _cache:
        from oracle import data
        r = data.rng(int(G()["seed"]) + 100 * h + w)
        x = (r.standard_normal((3, C, h, w)).astype(np.float32) * np.float32(0.5) + np.float32(0.2)).astype(np.float32)
        assert x.astype(np.float64).sum() == float(G()["%dx%d_xsum" % (h, w)])
        _cache[key] = torch.from_numpy(x)
    return _cache[key]


def make_pool(name, cuda):
    from cirtorch.layers.pooling import GeM, GeMmp, MAC, SPoC
    if name == "gemmp":
        m = GeMmp(p=3, mp=C)
        m.p.copy_(torch.from_numpy(G()["gemmp_p"]).reshape(C, 1, 1))
        return m.to(cuda)
    return {"gem3": lambda: GeM(p=3), "gem2.5": lambda: GeM(p=2.5), "mac": MAC, "spoc": SPoC}[name]().to(cuda)


def make_rpool(name, wh, cuda):
    from cirtorch.layers.pooling import Rpool
    lin = None
    if wh:
        lin = torch.nn.Linear(C, C)
        lin.load_state_dict({"weight": torch.from_numpy(G()["whiten_weight"]),
                             "bias": torch.from_numpy(G()["whiten_bias"])})
    return Rpool(make_pool(name, cuda), whiten=lin, L=3).to(cuda).eval()


def ref_pool64(x, rects, mode, p=3.0, eps=1e-6):
    """float64 pooling of x [N, C, H, W] (CPU) over the rectangles -> [N, R, C]"""
    x = x.double()
    out = []
    for (y0, x0, h, w) in rects:
        v = x[:, :, y0:y0 + h, x0:x0 + w]
        if mode == "mac":
            out.append(v.amax(dim=(2, 3)))
        elif mode == "spoc":
            out.append(v.mean(dim=(2, 3)))
        else:
            pp = torch.as_tensor(p, dtype=torch.float64).reshape(1, -1, 1, 1)
            out.append(v.clamp(min=eps).pow(pp).mean(dim=(2, 3)).pow(1.0 / pp.reshape(1, -1)))
    return torch.stack(out, dim=1)


def l2n64(v, eps=1e-6):
    return v / (v.norm(dim=-1, keepdim=True) + eps)


def ref_rpool64(x, rects, name, wh, aggregate):
    """the whole Rpool chain in float64 on the given (already rounded) inputs"""
    p = {"gem3": 3.0, "gem2.5": 2.5, "gemmp": G()["gemmp_p"].astype(np.float64)}.get(name, 3.0)
    mode = name if name in ("mac", "spoc") else "gem"
    o = l2n64(ref_pool64(x, rects, mode, p))
    if wh:
        o = l2n64(o @ torch.from_numpy(G()["whiten_weight"]).double().t() + torch.from_numpy(G()["whiten_bias"]).double())
    return l2n64(o.sum(1)) if aggregate else o


def report(tag, got, ref, rtol, atol):
    """max error in units of the tolerance (<= 1 passes), printed before any assertion"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    excess = (np.abs(got - ref) / (atol + rtol * np.abs(ref))).max()
    print("%-28s max|d|=%.3g  max|d|/tol=%.3f" % (tag, np.abs(got - ref).max(), excess))
    return excess


def mode_code(mode):
    from cirtorch import _engine as E
    return {"gem": E.RR_POOL_GEM, "mac": E.RR_POOL_MAC, "spoc": E.RR_POOL_SPOC}[mode]


# ----------------------------------------------------------------------------- membership
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("hwl", [(7, 7, 3), (5, 9, 3), (9, 5, 3), (1, 1, 3), (2, 7, 3), (3, 11, 3), (3, 11, 4),
                                 (3, 13, 4)])
def test_membership_is_exact(cuda, hwl, dtype):
    """A one-hot map (channel k is 1 at pixel k mod H*W): MAC is exactly 1 on the
    regions that contain the pixel and 0 elsewhere, SPoC 1 / area or 0 (1 ulp).
    (3, 11) has 45 regions at L = 3 and 81 at L = 4, (3, 13) the L = 4 maximum of 91: two
    and three region chunks."""
    from cirtorch import _ops
    h, w, L = hwl
    rects = recorded(h, w, L)
    assert len(rects) == {(3, 11, 3): 45, (3, 11, 4): 81, (3, 13, 4): 91}.get(hwl, len(rects))
    c = max(C, (h * w + 7) // 8 * 8)
    x = torch.zeros(1, c, h, w)
    k = torch.arange(c)
    x[0, k, (k % (h * w)) // w, (k % (h * w)) % w] = 1.0
    inside = torch.zeros(len(rects), c, dtype=torch.bool)
    area = torch.zeros(len(rects), 1)
    for r, (y0, x0, rh, rw) in enumerate(rects):
        py, px = (k % (h * w)) // w, (k % (h * w)) % w
        inside[r] = (py >= y0) & (py < y0 + rh) & (px >= x0) & (px < x0 + rw)
        area[r] = rh * rw
    xg = x.to(cuda).to(DTYPES[dtype]).contiguous(memory_format=torch.channels_last)
    mac = _ops.region_pool(xg, rects, mode_code("mac")).cpu()[0]
    assert torch.equal(mac, inside.float())
    spoc = _ops.region_pool(xg, rects, mode_code("spoc")).cpu()[0]
    want = torch.where(inside, torch.ones(1) / area, torch.zeros(1))
    ulp = torch.from_numpy(np.spacing(want.numpy()))
    assert bool(((spoc - want).abs() <= ulp).all())
    assert torch.equal(spoc == 0, ~inside)


# ----------------------------------------------------------------------------- values
@pytest.mark.parametrize("hw", SHAPES)
def test_rpool_matches_reference_outputs(cuda, hw):
    """Every rpool.npz case (5 inner pools x with / without whitening x aggregated /
    per region) against the reference float32 output, at the project tolerances.
    Measured on the MI355X: the largest error is 0.26 of the tolerance (7x7 GeM p=2.5
    with whitening, per region: max |d| = 1.5e-7); the reference's own float32-vs-
    float64 difference on these cases is at most 1.6e-7 (``*_e64`` in rpool.npz), so no
    bar was widened.  Every figure is printed before the assertion."""
    g = G()
    x = rpool_input(*hw).to(cuda)
    worst = 0.0
    for name in POOLS:
        for wh in (0, 1):
            m = make_rpool(name, wh, cuda)
            tol = WHITEN_TOL if wh else POOL_TOL
            with torch.no_grad():
                agg, reg = m(x), m(x, aggregate=False)
            R = len(recorded(*hw))
            assert tuple(agg.shape) == (3, C, 1, 1) and tuple(reg.shape) == (3, R, C, 1, 1)
            assert agg.dtype == torch.float32 and reg.dtype == torch.float32
            key = "%dx%d_%s_w%d" % (hw[0], hw[1], name, wh)
            worst = max(worst, report(key + "_agg", agg.reshape(3, C).cpu(), g[key + "_agg"], **tol))
            worst = max(worst, report(key + "_reg", reg[1].reshape(R, C).cpu(), g[key + "_reg"], **tol))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("hw", SHAPES)
def test_region_vectors_f32_and_mac_exact(cuda, hw):
    """The pooled region vectors themselves (before any L2N): MAC is exact, GeM /
    SPoC / GeMmp hold rtol 2e-6 / atol 1e-7 against a float64 evaluation over the
    recorded rectangles."""
    from cirtorch import _ops
    rects = recorded(*hw)
    x = rpool_input(*hw)
    xg = x.to(cuda)
    got = _ops.region_pool(xg, rects, mode_code("mac")).cpu()
    assert torch.equal(got, ref_pool64(x, rects, "mac").float())
    worst = 0.0
    for tag, mode, p in (("spoc", "spoc", 3.0), ("gem3", "gem", 3.0), ("gem2.5", "gem", 2.5),
                         ("gemmp", "gem", torch.from_numpy(G()["gemmp_p"]))):
        pg = p.to(cuda) if torch.is_tensor(p) else p
        got = _ops.region_pool(xg, rects, mode_code(mode), pg).cpu()
        ref = ref_pool64(x, rects, mode, p.double().numpy() if torch.is_tensor(p) else p)
        worst = max(worst, report("%dx%d %s" % (hw[0], hw[1], tag), got, ref, **POOL_TOL))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hw", [(7, 7), (3, 11), (2, 7)])
def test_rpool_16bit_inputs(cuda, hw, dtype):
    """16-bit inputs are pooled with float32 accumulation: compared with a float64
    evaluation of the same rounded inputs over the recorded rectangles."""
    rects = recorded(*hw)
    xr = rpool_input(*hw).to(DTYPES[dtype])
    xg = xr.to(cuda).contiguous(memory_format=torch.channels_last)
    worst = 0.0
    for name in POOLS:
        for wh in (0, 1):
            m = make_rpool(name, wh, cuda)
            tol = WHITEN_TOL if wh else POOL_TOL
            with torch.no_grad():
                agg, reg = m(xg), m(xg, aggregate=False)
            tag = "%s %dx%d %s w%d" % (dtype, hw[0], hw[1], name, wh)
            worst = max(worst, report(tag + " agg", agg.reshape(3, C).cpu(),
                                      ref_rpool64(xr.float(), rects, name, wh, True), **tol))
            worst = max(worst, report(tag + " reg", reg.reshape(3, len(rects), C).cpu(),
                                      ref_rpool64(xr.float(), rects, name, wh, False), **tol))
    assert worst <= 1.0, worst


# ----------------------------------------------------------------------------- shapes and layouts
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("c", [8, 72, 520])
def test_channel_edges(cuda, c, dtype):
    """c below one block's 256-channel span, not a multiple of it, and past one block;
    NHWC (read in place) and NCHW-contiguous (converted once) inputs agree bit for bit."""
    from cirtorch import _ops
    from cirtorch.layers.regions import roi_regions
    rects = roi_regions(5, 9)
    assert rects == recorded(5, 9)
    g = torch.Generator().manual_seed(100 + c)
    x = (torch.randn(3, c, 5, 9, generator=g) * 0.5 + 0.2).to(DTYPES[dtype])
    xg = x.to(cuda)
    worst = 0.0
    for mode, p in (("mac", 3.0), ("spoc", 3.0), ("gem", 3.0), ("gem", 2.5)):
        got = _ops.region_pool(xg.contiguous(memory_format=torch.channels_last), rects, mode_code(mode), p)
        assert torch.equal(got, _ops.region_pool(xg, rects, mode_code(mode), p))
        assert tuple(got.shape) == (3, len(rects), c)
        ref = ref_pool64(x.float(), rects, mode, p)
        if mode == "mac":
            assert torch.equal(got.cpu(), ref.float())
        else:
            worst = max(worst, report("c=%d %s p=%g" % (c, mode, p), got.cpu(), ref, **POOL_TOL))
    assert worst <= 1.0, worst


def test_channels_not_a_multiple_of_four(cuda):
    from cirtorch import _ops
    rects = recorded(5, 9)
    x = torch.randn(2, 10, 5, 9, generator=torch.Generator().manual_seed(3)) * 0.5 + 0.2
    p = torch.linspace(2, 4, 10)
    got = _ops.region_pool(x.to(cuda), rects, mode_code("gem"), p.to(cuda)).cpu()
    assert tuple(got.shape) == (2, len(rects), 10)
    assert report("c=10 gemmp", got, ref_pool64(x, rects, "gem", p.double().numpy()), **POOL_TOL) <= 1.0


def test_batch_of_three_equals_three_single_images(cuda):
    from cirtorch import _ops
    rects = recorded(5, 9)
    x = rpool_input(5, 9).to(cuda)
    for mode in ("gem", "mac", "spoc"):
        both = _ops.region_pool(x, rects, mode_code(mode))
        single = torch.cat([_ops.region_pool(x[i:i + 1], rects, mode_code(mode)) for i in range(3)])
        assert torch.equal(both, single)
        # and independent of the position in the batch
        assert torch.equal(_ops.region_pool(x.flip(0), rects, mode_code(mode)).flip(0), both)
    for name, wh in (("gem3", 1), ("gemmp", 0), ("mac", 1)):
        m = make_rpool(name, wh, cuda)
        with torch.no_grad():
            for agg in (True, False):
                assert torch.equal(m(x, aggregate=agg), torch.cat([m(x[i:i + 1], aggregate=agg) for i in range(3)]))
            assert torch.equal(m(x), m(x))  # run to run


@pytest.mark.parametrize("mode", ["gem", "mac", "spoc"])
def test_nan_reaches_exactly_the_regions_that_contain_it(cuda, mode):
    from cirtorch import _ops
    h, w = 5, 9
    rects = recorded(h, w)
    x = rpool_input(h, w).clone()
    clean = _ops.region_pool(x.to(cuda), rects, mode_code(mode)).cpu()
    img, ch, py, px = 1, 5, 3, 7
    x[img, ch, py, px] = float("nan")
    got = _ops.region_pool(x.to(cuda), rects, mode_code(mode)).cpu()
    want = torch.zeros_like(got, dtype=torch.bool)
    for r, (y0, x0, rh, rw) in enumerate(rects):
        want[img, r, ch] = y0 <= py < y0 + rh and x0 <= px < x0 + rw
    assert 1 < int(want.sum()) < len(rects)
    assert torch.equal(torch.isnan(got), want)
    assert torch.equal(got[~want], clean[~want])


# ----------------------------------------------------------------------------- exponents
def test_device_exponent_is_read_at_every_forward(cuda):
    from cirtorch.layers.pooling import GeM, Rpool
    x = rpool_input(7, 7).to(cuda)
    m = Rpool(GeM(p=3)).to(cuda).eval()
    with torch.no_grad():
        a3 = m(x)
        m.rpool.p.data.fill_(2.5)
        a25 = m(x)
        fresh = Rpool(GeM(p=2.5)).to(cuda).eval()(x)
    assert not torch.equal(a3, a25)
    assert torch.equal(a25, fresh)
    assert report("p.fill_(2.5)", a25.reshape(3, C).cpu(), G()["7x7_gem2.5_w0_agg"], **POOL_TOL) <= 1.0


def test_gemmp_whole_map_equals_gem(cuda):
    from cirtorch.layers import functional as LF
    from cirtorch.layers.pooling import GeMmp
    from cirtorch.modules.heads.global_head import globalHead
    x = rpool_input(5, 9).to(cuda)
    m = GeMmp(p=3, mp=C).to(cuda)
    assert m.p.is_cuda
    with torch.no_grad():
        got, ref = m(x), LF.gem(x, 3)
    assert tuple(got.shape) == (3, C, 1, 1)
    torch.testing.assert_close(got, ref, rtol=2e-6, atol=0)
    # per-channel exponents against float64, through the head's GeMmp constructor path
    head = globalHead(pooling={"name": "GeMmp", "params": {"p": 3, "eps": 1e-6}}, normal={"name": "L2N", "params": {}},
                      dim=C).to(cuda).eval()
    head.pool.p.copy_(torch.from_numpy(G()["gemmp_p"]).reshape(C, 1, 1))
    with torch.no_grad():
        got = head(x, do_whitening=False).t().cpu()
    ref = l2n64(ref_pool64(x.cpu(), [(0, 0, 5, 9)], "gem", G()["gemmp_p"].astype(np.float64))[:, 0])
    assert report("head GeMmp", got, ref, **POOL_TOL) <= 1.0


# ----------------------------------------------------------------------------- head and net
def regional_head(cuda):
    from cirtorch.layers.pooling import GeM
    from cirtorch.modules.heads.global_head import globalHead
    g = G()
    head = globalHead(pooling={"name": "ROIpool", "params": {"rpool": GeM(p=3), "whiten": torch.nn.Linear(C, C),
                                                              "L": 3}},
                      normal={"name": "L2N", "params": {}}, dim=C)
    head.load_state_dict({"whiten.weight": torch.from_numpy(g["head_whiten_weight"]),
                          "whiten.bias": torch.from_numpy(g["head_whiten_bias"]),
                          "pool.rpool.p": torch.tensor([3.0]),
                          "pool.whiten.weight": torch.from_numpy(g["whiten_weight"]),
                          "pool.whiten.bias": torch.from_numpy(g["whiten_bias"])})
    return head.to(cuda).eval()


@pytest.mark.parametrize("hw", [(7, 7), (3, 11)])
def test_regional_global_head_matches_reference(cuda, hw):
    head = regional_head(cuda)
    x = rpool_input(*hw).to(cuda)
    with torch.no_grad():
        got, got_nw = head(x), head(x, do_whitening=False)
    assert tuple(got.shape) == (C, 3)
    key = "head_%dx%d" % hw
    worst = max(report(key, got.cpu(), G()[key], **WHITEN_TOL),
                report(key + "_nowhiten", got_nw.cpu(), G()[key + "_nowhiten"], **WHITEN_TOL))
    assert worst <= 1.0, worst


def regional_state(dim):
    """make_golden_regional.regional_state: the regional Linear of the R18 case"""
    from oracle import weights
    seed = weights.SEED_WEIGHTS
    std = np.float32(0.1 * np.sqrt(2.0 / (dim + dim)))
    return {"pool.whiten.weight": (weights._stream(seed, "pool.whiten.weight").standard_normal((dim, dim), dtype=np.float32)
                                   * std).astype(np.float32),
            "pool.whiten.bias": weights._stream(seed, "pool.whiten.bias").uniform(-0.002, 0.002, dim).astype(np.float32)}


def regional_r18(precision, cuda):
    from cirtorch.models.GF_net import make_net
    from oracle import weights
    net = make_net("resnet18", precision=precision, regional=True)
    missing, unexpected = net.body.load_state_dict(
        {k: torch.from_numpy(v) for k, v in weights.backbone_state("resnet18").items()}, strict=False)
    assert not missing and not unexpected
    hs = weights.head_state(512)
    sd = {"whiten.weight": hs["whiten.weight"], "whiten.bias": golden("r18.npz")["head_bias"],
          "pool.rpool.p": np.array([3.0], dtype=np.float32)}
    sd.update(regional_state(512))
    net.ret_head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net.to(cuda).eval()


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_regional_r18_vs_reference(cuda, precision):
    """The cosine bars of test_gpu_extract.py for R18 (1 - 1e-4 in fp32 and fp16)."""
    from oracle import backbone as obb, data
    g = golden("r18.npz")
    net = regional_r18(precision, cuda)
    assert net.meta["regional"] is True
    imgs = data.structured_images(int(g["n"]), *[int(v) for v in g["res"]], seed=int(g["seed"]))[:2]
    got = net.extract([obb.normalize_images(torch.from_numpy(im)).to(cuda) for im in imgs]).cpu().numpy()
    ref = G()["r18reg_desc"]
    assert got.shape == ref.shape == (512, 2)
    cos = cosines(got, ref)
    print(precision, "regional r18 cos min", cos.min(), "cos between the two images", cosines(ref[:, :1], ref[:, 1:]))
    assert cos.min() >= 1 - 1e-4


def test_extract_vectors_regional_multiscale(cuda):
    from cirtorch.models.GF_net import extract_vectors, make_net
    from cirtorch.models.init import random_init_
    net = random_init_(make_net("resnet18", precision="fp16", regional=True), 4).to(cuda).eval()
    imgs = [torch.rand(3, 96, 128, generator=torch.Generator().manual_seed(i)) for i in range(3)]
    # the msp rule of scripts/test.py:136 gives 1 for a regional net
    msp = net.pool.rpool.p.item() if (net.meta["pooling"] == "gem" and not net.meta["regional"]
                                      and not net.meta["whitening"]) else 1
    assert msp == 1
    v = extract_vectors(net, imgs, None, ms=[1, 1 / 2 ** 0.5], msp=msp, batch=4)
    assert tuple(v.shape) == (512, 3)
    assert bool(torch.isfinite(v).all())
    torch.testing.assert_close(v.norm(dim=0).cpu(), torch.ones(3), rtol=1e-5, atol=0)


def test_regional_head_is_graph_capturable(cuda):
    """one stream, no host->device copy and no sync in the forward: captured once,
    replayed with new inputs, bit-identical to the eager launches"""
    from cirtorch.utils.graph import GraphedForward
    head = regional_head(cuda)
    x1 = rpool_input(7, 7).to(cuda).contiguous(memory_format=torch.channels_last)
    x2 = (x1 * 0.5 + 0.1).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        e1, e2 = head(x1).clone(), head(x2).clone()
        g = GraphedForward(lambda t: head(t), x1)
        assert torch.equal(g(x1), e1)
        assert torch.equal(g(x2), e2)
        assert torch.equal(g(x1), e1)
    assert not torch.equal(e1, e2)
