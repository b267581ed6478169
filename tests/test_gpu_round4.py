"""Round-4 GPU tests: the ragged image batch.

A PackedSequence of different-size images goes to the body as a ragged table
(rr_stem_conv_pool_ragged / rr_image_to_nhwc_ragged): the stem reads each
image at its own address and pads to the max extent on the fly.  Checked
  * against the reference (tests/golden/r50mixed.npz: R50 at 768x1024,
    640x960, 700x1000, both pad orders the reference code has), fp32 at the
    north-star bar 1 - 1e-4 and fp16 at its documented bar;
  * bit for bit against the same engine on the explicitly padded batch
    (ragged and padded runs must be the same computation);
  * rr_pad_images (pad_packed_images on device tensors) against the host path.
Plus the scripts/test.py:84-259 replay through the product vs the oracle's run
of the same sequence (tests/testpy_replay.py, tests/golden/testpy.npz).
"""

import numpy as np
import pytest
import torch

from conftest import cosines, golden

pytestmark = pytest.mark.gpu

FP32_COS = 1 - 1e-4
FP16_COS = 1 - 1e-4  # the north-star bar the fp16 headline claims
BF16_COS = 1 - 2e-3
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _net(arch, head_bias, precision, cuda, normalize):
    from cirtorch.models.GF_net import make_net
    from oracle import weights
    net = make_net(arch, precision=precision, mean=MEAN if normalize else None, std=STD if normalize else None)
    missing, unexpected = net.body.load_state_dict(
        {k: torch.from_numpy(v) for k, v in weights.backbone_state(arch).items()}, strict=False)
    assert not unexpected and not missing
    hs = weights.head_state(weights.OUTPUT_DIM[arch])
    hs["whiten.bias"] = head_bias
    net.ret_head.load_state_dict({k: torch.from_numpy(v) for k, v in hs.items()})
    return net.to(cuda).eval()


def _mixed_images(g):
    from oracle import data
    sizes = [tuple(int(v) for v in hw) for hw in g["mixed_sizes"]]
    return [data.structured_images(1, h, w, seed=int(g["seed"]) + i)[0] for i, (h, w) in enumerate(sizes)]


@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
def test_r50_ragged_batch_vs_reference(cuda, precision):
    """the ragged R50 batch, both pad orders, vs the reference golden"""
    from oracle import backbone as obb
    g = golden("r50mixed.npz")
    imgs = _mixed_images(g)
    bar = {"fp32": FP32_COS, "fp16": FP16_COS, "bf16": BF16_COS}[precision]
    # (a) augment=None on pre-normalised images: the pads are 0 in the normalised domain
    net = _net("resnet50", g["head_bias"], precision, cuda, normalize=False)
    got = net.extract([obb.normalize_images(torch.from_numpy(im)).to(cuda) for im in imgs]).cpu().numpy()
    cos = cosines(got, g["desc_mixed"])
    print(precision, "normalise->pad cos", cos)
    assert cos.min() >= bar
    # (b) the in-tree order: pad with 0 first, then normalise (pads become -mean/std)
    net = _net("resnet50", g["head_bias"], precision, cuda, normalize=True)
    got = net.extract([torch.from_numpy(im).to(cuda) for im in imgs]).cpu().numpy()
    cos = cosines(got, g["desc_mixed_padnorm"])
    print(precision, "pad->normalise cos", cos)
    assert cos.min() >= bar


def _padded(imgs, pad=0):
    h = max(t.shape[-2] for t in imgs)
    w = max(t.shape[-1] for t in imgs)
    out = imgs[0].new_full((len(imgs), imgs[0].shape[0], h, w), pad)
    for i, t in enumerate(imgs):
        out[i, :, :t.shape[-2], :t.shape[-1]] = t
    return out


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("sizes", [[(96, 128), (80, 100), (64, 128)],     # even stem map: fused v3 stem
                                   [(100, 130), (90, 120), (75, 130)]])   # odd stem map (wo = 65)
@pytest.mark.parametrize("u8", [False, True])
def test_ragged_equals_padded_bitwise(cuda, precision, sizes, u8):
    """the ragged stem and the padded-batch stem are the same computation: bit-identical
    descriptors (the pad read as 0 before normalisation, like the padded tensor's zeros)"""
    from cirtorch.models.GF_net import make_net
    from cirtorch.models.init import random_init_
    net = make_net("resnet18", precision=precision, mean=MEAN, std=STD)
    random_init_(net, seed=4)
    net = net.to(cuda).eval()
    g = torch.Generator(device=cuda).manual_seed(9)
    if u8:
        imgs = [torch.randint(0, 256, (3, h, w), generator=g, device=cuda, dtype=torch.uint8) for h, w in sizes]
    else:
        imgs = [torch.rand((3, h, w), generator=g, device=cuda) for h, w in sizes]
    ragged = net.extract(imgs)
    padded = net.extract(_padded(imgs))
    assert torch.equal(ragged, padded)


def test_ragged_none_entry_and_long_batch(cuda):
    """> 64 images (several ragged launches) and a None entry (all pad) equal the padded batch"""
    from cirtorch.models.GF_net import make_net
    from cirtorch.models.init import random_init_
    from cirtorch.utils.parallel import PackedSequence
    net = make_net("resnet18", precision="fp16", mean=MEAN, std=STD)
    random_init_(net, seed=5)
    net = net.to(cuda).eval()
    g = torch.Generator(device=cuda).manual_seed(11)
    sizes = [(64 - 2 * (i % 7), 96 - 4 * (i % 5)) for i in range(70)]
    imgs = [torch.rand((3, h, w), generator=g, device=cuda) for h, w in sizes]
    assert torch.equal(net.extract(imgs), net.extract(_padded(imgs)))
    with torch.no_grad():
        _, pred = net(img=PackedSequence([imgs[0], None, imgs[1]]))
        zero = torch.zeros_like(imgs[0])
        ref = net.extract(_padded([imgs[0], zero, imgs[1]]))
    assert torch.equal(pred["ret_pred"], ref)


@pytest.mark.parametrize("u8", [False, True])
def test_ragged_thin_images(cuda, u8):
    """images 1-5 pixels wide or high inside a wider batch: the float stem reads pixel
    pairs with one 8-B load clamped into the image row (a 1-pixel row loads its pixel
    and the next element), the pad around them reads 0 -- same bits as the padded batch"""
    from cirtorch.models.GF_net import make_net
    from cirtorch.models.init import random_init_
    net = make_net("resnet18", precision="fp16", mean=MEAN, std=STD)
    random_init_(net, seed=6)
    net = net.to(cuda).eval()
    g = torch.Generator(device=cuda).manual_seed(12)
    sizes = [(64, 96), (40, 1), (33, 2), (20, 3), (1, 50), (2, 5), (64, 95)]
    if u8:
        imgs = [torch.randint(0, 256, (3, h, w), generator=g, device=cuda, dtype=torch.uint8) for h, w in sizes]
    else:
        imgs = [torch.rand((3, h, w), generator=g, device=cuda) for h, w in sizes]
    assert torch.equal(net.extract(imgs), net.extract(_padded(imgs)))


def test_ragged_stage_maps_equal_padded(cuda):
    """every stage map of the ragged batch equals the padded batch's (fp32 and fp16)"""
    from cirtorch.models.GF_net import make_net
    from cirtorch.models.init import random_init_
    g = torch.Generator(device=cuda).manual_seed(12)
    imgs = [torch.rand((3, h, w), generator=g, device=cuda) for h, w in [(120, 160), (96, 150), (128, 100)]]
    for prec in ("fp32", "fp16"):
        net = make_net("resnet50", precision=prec, mean=MEAN, std=STD)
        random_init_(net, seed=6)
        net = net.to(cuda).eval()
        with torch.no_grad():
            a = net.body(imgs, normalize=(MEAN, STD))
            b = net.body(_padded(imgs), normalize=(MEAN, STD))
        for k in a:
            assert torch.equal(a[k], b[k]), (prec, k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.uint8, torch.int64])
def test_pad_packed_images_device_equals_host(cuda, dtype):
    from cirtorch.utils.parallel import PackedSequence
    from cirtorch.utils.sequence import pad_packed_images, pack_padded_images
    r = np.random.default_rng(3)
    shapes = [(3, 5, 7), (3, 6, 4), None, (3, 2, 9)]
    host = [None if s is None else torch.from_numpy((r.random(s) * 100).astype(np.float64)).to(dtype) for s in shapes]
    for snap in (None, 4):
        for pad in (0, 7):
            ph, sh = pad_packed_images(PackedSequence(host), pad_value=pad, snap_size_to=snap)
            pd, sd = pad_packed_images(PackedSequence([None if t is None else t.to(cuda) for t in host]),
                                       pad_value=pad, snap_size_to=snap)
            assert pd.is_cuda and torch.equal(pd.cpu(), ph)
            assert [tuple(s) for s in sd] == [tuple(s) for s in sh]
    back = pack_padded_images(pd, sd)
    for t, b in zip(host, back):
        if t is not None:
            assert torch.equal(b.cpu(), t)
    # 2D entries
    h2 = [torch.rand(4, 6), torch.rand(5, 3)]
    ph, _ = pad_packed_images(PackedSequence(h2), pad_value=-1.0)
    pd, _ = pad_packed_images(PackedSequence([t.to(cuda) for t in h2]), pad_value=-1.0)
    assert torch.equal(pd.cpu(), ph) and ph.shape == (2, 5, 6)


# ------------------------------------------------------------------ scripts/test.py replay
class _ToTensorNormalize:
    """transforms.Compose([ToTensor(), Normalize(mean, std)]) of scripts/test.py:149-156
    (torchvision is absent: to_tensor = HWC uint8 -> CHW float32 / 255, then (x - m) / s)"""

    def __init__(self, mean, std):
        self.m = torch.tensor(mean)[:, None, None]
        self.s = torch.tensor(std)[:, None, None]

    def __call__(self, pil):
        x = torch.from_numpy(np.asarray(pil, dtype=np.float32).transpose(2, 0, 1).copy() / 255.0)
        return (x - self.m) / self.s


def _product_api(precision):
    import types
    from cirtorch.datasets.datahelpers import cid2filename
    from cirtorch.datasets.testdataset import configdataset
    from cirtorch.models.GF_net import init_network, extract_vectors
    from cirtorch.utils.evaluate import compute_map_and_print
    from cirtorch.utils.whiten import whitenlearn, whitenapply

    def load_net(state):
        meta = state["meta"]
        params = {"architecture": meta["architecture"], "pooling": meta["pooling"],
                  "local_whitening": meta.get("local_whitening", False), "regional": meta.get("regional", False),
                  "whitening": meta.get("whitening", False), "mean": meta["mean"], "std": meta["std"],
                  "pretrained": False}
        if precision is not None:
            params["precision"] = precision
        net = init_network(params)
        net.load_state_dict(state["state_dict"])
        net.cuda()
        net.eval()
        return net, net.meta, net.pool.p.item()

    def extract(net, images, size, bbxs, ms, msp):
        tf = _ToTensorNormalize(net.meta["mean"], net.meta["std"])
        return extract_vectors(net, images, size, tf, bbxs=bbxs, ms=ms, msp=msp)

    return types.SimpleNamespace(load_net=load_net, extract_vectors=extract, whitenlearn=whitenlearn,
                                 whitenapply=whitenapply, compute_map=compute_map_and_print,
                                 cid2filename=cid2filename, configdataset=configdataset,
                                 to_numpy=lambda v: v.numpy())


@pytest.mark.parametrize("case,precision", [("A", "fp32"), ("B", "fp32"), ("B", None)])
def test_scripts_test_replay(cuda, tmp_path, case, precision):
    """scripts/test.py:84-259 as one sequence through the product -- checkpoint load,
    init_network, Lw learned from extract_vectors of a whitening db, configdataset,
    extract_vectors (ms = [1, 1/sqrt2, sqrt2], msp = pool.p for case A; query bbx
    crops), np.dot / np.argsort, 3-argument compute_map_and_print, whitenapply,
    re-rank -- equals the oracle's run of the same sequence (tests/golden/testpy.npz).
    Case A: meta whitening=False (msp = 3); B: whitening=True (msp = 1), also at the
    init_network default precision (fp16).  B's Lw re-rank is decided by rounding
    (the float32 and float64 oracle runs disagree on it), so only its plain rank and
    mAP are compared."""
    import testpy_replay as T
    g = golden("testpy.npz")
    hashes = T.make_dataset(str(tmp_path))
    names = sorted(hashes)
    assert names == [str(x) for x in g["file_names"]]
    assert [hashes[k] for k in names] == [str(x) for x in g["file_sha1"]], "JPEG encoder output differs"
    ck = str(tmp_path / "ck.pth")
    T.checkpoint(ck, case == "B", g["head_bias"] if case == "B" else None)
    r = T.run(_product_api(precision), str(tmp_path), ck)
    assert r["msp"] == float(g[case + "_msp"])
    bar = FP32_COS if precision == "fp32" else FP16_COS
    assert cosines(r["vecs"], g[case + "_vecs"]).min() >= bar
    assert cosines(r["qvecs"], g[case + "_qvecs"]).min() >= bar
    assert (r["ranks"] == g[case + "_ranks"]).all()
    assert r["map"]["mAP"] == pytest.approx(float(g[case + "_map"]), abs=1e-9)
    if bool(g[case + "_ranks_lw_stable"]):
        assert (r["ranks_lw"] == g[case + "_ranks_lw"]).all()
        assert r["map_lw"]["mAP"] == pytest.approx(float(g[case + "_map_lw"]), abs=1e-9)


# ------------------------------------------------------------------ stem v4 (space-to-depth K)
@pytest.mark.parametrize("shape", [(2, 64, 84), (1, 100, 472), (3, 200, 132), (2, 96, 128)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_stem_v4_space_to_depth(cuda, dt, shape):
    """RR_TUNE_STEM 5: the stem with its K in space-to-depth form (6 MFMA K-steps of
    12-channel 2x2 pixel blocks instead of 7 kernel rows of 8 x 4) against a float64
    restatement on the same 16-bit operands and against v3 (same taps, only the f32
    summation order differs: within 1 output ulp); uint8 pixels == float x / 255; a
    ragged batch == its padded batch (bit for bit)."""
    import torch.nn.functional as F
    from cirtorch import _engine as E
    from cirtorch import _ops as ops
    n, h, w = shape
    g = torch.Generator().manual_seed(h * 7 + w)
    x = torch.rand(n, 3, h, w, generator=g)
    wt = (torch.randn(64, 3, 7, 7, generator=g) * 0.1).to(dt).float()
    scale = torch.rand(64, generator=g) + 0.5
    scale[::5] *= -1.0
    shift = torch.randn(64, generator=g) * 0.1
    wpk = ops.pack_stem_weights(wt.to(cuda), dt)
    xu = (x * 255).to(torch.uint8)
    xf = xu.float() / 255.0
    outs = {}
    for mode in (2, 5):
        with E.tuning(STEM=mode):
            outs[mode] = [ops.stem_conv_pool(inp.to(cuda), wpk, scale.to(cuda), shift.to(cuda), leaky=True, slope=0.01,
                                             mean=MEAN, std=STD).float().cpu() for inp in (xf, xu)]
            if mode == 5:
                imgs = [xu[i, :, : h - 2 * i, : w - 4 * i].contiguous().to(cuda) for i in range(n)]
                rag = ops.stem_conv_pool_ragged(imgs, h, w, wpk, scale.to(cuda), shift.to(cuda), mean=MEAN, std=STD)
                pad = torch.zeros_like(xu)
                for i in range(n):
                    pad[i, :, : h - 2 * i, : w - 4 * i] = xu[i, :, : h - 2 * i, : w - 4 * i]
                ref_rag = ops.stem_conv_pool(pad.to(cuda), wpk, scale.to(cuda), shift.to(cuda), mean=MEAN, std=STD)
                assert torch.equal(rag, ref_rag)
    v3, v4 = outs[2][0], outs[5][0]
    assert torch.equal(outs[5][0], outs[5][1])            # uint8 == float x / 255
    xn = ((xf - torch.tensor(MEAN)[:, None, None]) / torch.tensor(STD)[:, None, None]).to(dt).float()
    ref = F.conv2d(xn.double(), wt.double(), stride=2, padding=3) * scale.double()[None, :, None, None] \
        + shift.double()[None, :, None, None]
    ref = F.max_pool2d(F.leaky_relu(ref, 0.01), 3, 2, 1).permute(0, 2, 3, 1).float()
    err = (v4 - ref).abs().max().item()
    assert err <= 8e-3 * ref.abs().max().item(), err
    ulp = 2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10
    d = (v4 - v3).abs()
    assert (d <= ulp * v3.abs().clamp_min(1.0) + 1e-6).all(), d.max().item()
    assert (d == 0).float().mean().item() > 0.9
