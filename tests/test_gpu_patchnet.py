"""GPU checks of the learned patch descriptors (rr_patchnet.hip): HardNet and SOSNet against the float64
reference modules recorded in tests/golden/patchnet.npz (tolerances measured by the generator), the
layer-6 map of the trunk, the fused entry against the chain of the two, independence of the batch, of
the chunk length and of a patch's position, the exact cases, the module's weight cache, the
describe_keypoints(descriptor=...) path and one graph capture.

Measured on the MI355X (every test prints its figures before it asserts; pytest -s), over the 129 patches
against the float64 reference: largest entry difference 3.35e-4 (HardNet, tolerance 1.25e-3) and 3.28e-4
(SOSNet, tolerance 1.28e-3), smallest cosine 0.99999965 / 0.99999955; the layer-6 map within 8.9e-4 / 1.14e-3
of its largest entry (tolerances 2.94e-3 / 4.79e-3).
"""

import numpy as np
import pytest
import torch

import patchnet_cases as NC
from conftest import golden

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


@pytest.fixture(scope="module")
def fix():
    return golden("patchnet.npz")


@pytest.fixture(scope="module")
def x129(cuda):
    return torch.from_numpy(NC.patches()).to(cuda)


def _module(variant, seed, cuda):
    from cirtorch.features import HardNet, SOSNet
    net = (HardNet if variant == "hardnet" else SOSNet)(False)
    sd = {k: torch.from_numpy(np.asarray(a)) for k, a in NC.state_dict(variant, NC.net_params(seed)).items()}
    net.load_state_dict(sd, strict=True)
    return net.to(cuda).eval()


@pytest.fixture(scope="module")
def nets(cuda):
    return {v: _module(v, NC.SEEDS[v], cuda) for v in NC.VARIANTS}


@pytest.fixture(scope="module")
def full(nets, x129):
    """the 129 descriptors of each variant, computed once (default chunk) and left unchanged"""
    return {v: nets[v](x129[:, None]) for v in NC.VARIANTS}


@pytest.mark.parametrize("variant", NC.VARIANTS)
@pytest.mark.parametrize("B", NC.BATCHES)
def test_descriptors_against_reference(cuda, fix, nets, x129, full, variant, B):
    got = nets[variant](x129[:B, None])
    assert got.shape == (B, 128) and got.dtype == torch.float32
    g = got.cpu().numpy().astype(np.float64)
    want = fix[variant + "_desc"][:B].astype(np.float64)
    diff = np.abs(g - want).max()
    cos = (g * want).sum(1) / (np.linalg.norm(g, axis=1) * np.linalg.norm(want, axis=1))
    print("%s B=%d: max |diff| %.3e (tol %.3e), min cosine %.9f" % (variant, B, diff, fix[variant + "_tol"][0], cos.min()))
    assert np.isfinite(g).all()
    assert diff <= fix[variant + "_tol"][0]
    assert cos.min() >= 1 - 1e-4
    # a descriptor does not depend on the batch it is in
    assert bits(got) == bits(full[variant][:B])


@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_descriptors_against_the_restatement(cuda, full, variant):
    """against patchnet_cases.quantised_net (fp16 at the rounding points of rr.h, float64 elsewhere), within 4 x
    what a float32 accumulation moves it by: the difference of quantised_net and quantised_net_f32 over the
    same 129 patches, measured by make_golden_patchnet_edges.py (1.18e-4 / 1.20e-4) and re-measured by
    test_host_patchnet_edges.py.  Less than half the tolerance against the float64 reference above."""
    tol = float(golden("patchnet_edges.npz")[variant + "_f32_tol"])
    want = NC.quantised_net(NC.patches(), NC.net_params(NC.SEEDS[variant]), variant)[0]
    diff = np.abs(full[variant].cpu().numpy().astype(np.float64) - want).max()
    print("%s: max |GPU - quantised_net| %.3e (tol %.3e)" % (variant, diff, tol))
    assert tol < 5e-4
    assert diff <= tol


@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_trunk_map_against_reference(cuda, fix, nets, x129, variant):
    from cirtorch import _ops
    idx = list(NC.MAP_PATCHES)
    maps = _ops.patchnet_trunk(x129[idx], nets[variant].packed(), variant)
    assert maps.shape == (len(idx), 8, 8, 128) and maps.dtype == torch.float16
    got = maps.cpu().numpy().astype(np.float64)
    want = fix[variant + "_map"]
    rel = np.abs(got - want).max() / np.abs(want).max()
    print("%s map: max |diff| / max |map| %.3e (tol %.3e)" % (variant, rel, fix[variant + "_tol"][1]))
    assert rel <= fix[variant + "_tol"][1]
    assert (got >= 0).all() and (got > 0).mean() > 0.1     # after a ReLU, and not an empty map


@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_fused_equals_chain(cuda, nets, x129, full, variant):
    from cirtorch import _ops
    packed = nets[variant].packed()
    chain = _ops.patchnet_head(_ops.patchnet_trunk(x129, packed, variant), packed, variant)
    assert bits(_ops.patchnet_describe(x129, packed, variant)) == bits(chain) == bits(full[variant])


@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_chunk_batch_position_and_run_independence(cuda, nets, x129, full, variant):
    from cirtorch import _engine as E
    net, want = nets[variant], full[variant]
    with E.tuning(PATCHNET_CHUNK=64):                       # 129 = 64 + 64 + 1
        assert bits(net(x129[:, None])) == bits(want)
    assert E.get_tuning("PATCHNET_CHUNK") == 16384
    assert bits(net(x129[:, None])) == bits(want)           # a second run
    rev = net(x129.flip(0)[:, None])
    assert bits(rev.flip(0)) == bits(want)                  # reversed order
    one = torch.cat([net(x129[i:i + 1, None]) for i in range(NC.NPATCH)])
    assert bits(one) == bits(want)                          # one at a time


def test_exact_cases(cuda):
    """fresh statistics (mean 0, var 1), constant patch: HardNet zeros; SOSNet 1 / sqrt(128) in every entry, to
    float32 rounding of the head (1e-10 and its square are normal float32 numbers; twelve additions and
    a square root and a quotient, each within 2^-24 relative: below 4.2e-8 absolute on 0.0884)"""
    from cirtorch.features import HardNet, SOSNet
    x = torch.full((3, 1, 32, 32), 0.5, device=cuda)
    x[1] = 17.0
    x[2] = 0.0
    hard = HardNet().to(cuda).eval()(x)
    assert bits(hard) == bits(torch.zeros(3, 128))
    sos = SOSNet(False).to(cuda).eval()(x).cpu().numpy().astype(np.float64)
    assert np.abs(sos - 1 / np.sqrt(128)).max() <= 1e-7


def test_input_conversions(cuda, nets, x129, full):
    net, want = nets["hardnet"], full["hardnet"]
    x = x129[:5, None]
    assert bits(net(x.double())) == bits(want[:5])
    wide = torch.zeros((5, 1, 32, 64), device=cuda)
    wide[..., ::2] = x
    assert not wide[..., ::2].is_contiguous() and bits(net(wide[..., ::2])) == bits(want[:5])
    h = x.half()
    assert bits(net(h)) == bits(net(h.float()))


@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_module_cache_follows_the_weights(cuda, fix, nets, x129, full, variant):
    net = _module(variant, NC.SEEDS[variant], cuda)
    x = x129[:8, None]
    first = net(x)
    assert bits(first) == bits(full[variant][:8])
    blob = net.packed()
    assert net.packed() is blob                              # cached
    other = NC.state_dict(variant, NC.net_params(NC.OTHER_SEED))
    net.load_state_dict({k: torch.from_numpy(np.asarray(a)) for k, a in other.items()}, strict=True)
    second = net(x)
    assert bits(second) != bits(first)
    assert bits(second) == bits(_module(variant, NC.OTHER_SEED, cuda)(x))
    want = fix[variant + "_other_desc"].astype(np.float64)
    assert np.abs(second.cpu().numpy() - want).max() <= fix[variant + "_tol"][0]
    # an in-place change of a buffer, and a move
    seq = net.features if variant == "hardnet" else net.layers
    bn = [m for m in seq if isinstance(m, torch.nn.BatchNorm2d)][-1]
    with torch.no_grad():
        bn.running_mean.add_(0.25)
    third = net(x)
    assert bits(third) != bits(second)
    moved = net.cpu().to(cuda)
    assert bits(moved(x)) == bits(third)
    with pytest.raises(NotImplementedError):
        net.train()(x)


def _images(cuda):
    rng = np.random.default_rng(NC.PATCH_SEED + 1)
    img = rng.uniform(0.0, 1.0, (2, 1, 96, 128))
    for _ in range(2):    # a little structure: two passes of a 3 x 3 box filter
        p = np.pad(img, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")
        img = np.mean(np.lib.stride_tricks.sliding_window_view(p, (3, 3), axis=(2, 3)), axis=(4, 5))
    kp = np.stack([rng.uniform(20.0, 108.0, (2, 16)), rng.uniform(20.0, 76.0, (2, 16))], axis=-1)
    kp[0, 3] = -1.0
    return (torch.from_numpy(img.astype(np.float32)).to(cuda), torch.from_numpy(kp.astype(np.float32)).to(cuda),
            torch.tensor([16, 11], dtype=torch.int32, device=cuda))


@pytest.mark.parametrize("pyramid", (False, True))
@pytest.mark.parametrize("orientation", (False, True))
def test_describe_keypoints_with_a_descriptor(cuda, nets, orientation, pyramid):
    from cirtorch import _ops
    from cirtorch.features.laf import _rotation, make_upright
    from cirtorch.geometry.conversions import rad2deg
    from cirtorch.search import describe_keypoints
    net = nets["hardnet"]
    img, kp, count = _images(cuda)
    scale = 40.0 if pyramid else 12.0        # 2 * 40 / 32 = 2.5: pyramid level 1 (48 x 64)
    desc, angles = describe_keypoints(img, kp, count, scale=scale, orientation=orientation, pyramid=pyramid, descriptor=net)
    assert desc.shape == (2, 16, 128) and angles.shape == (2, 16)
    dead = torch.zeros((2, 16), dtype=torch.bool, device=cuda)
    dead[0, 3] = True
    dead[1, 11:] = True
    assert not desc[dead].any() and not angles[dead].any()
    norms = desc[~dead].norm(dim=1)
    assert torch.isfinite(desc).all() and (norms - 1).abs().max() < 1e-5
    # the same by hand: frames -> extract_patches_* -> (angle, turned frame, patches again) -> forward
    lafs = torch.zeros((2, 16, 2, 3), device=cuda)
    lafs[..., 0, 0] = scale
    lafs[..., 1, 1] = scale
    lafs[..., 2] = kp
    lafs[dead] = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], device=cuda)
    extract = (lambda f: _ops.extract_patches_pyramid(img, f, 32)) if pyramid else (lambda f: _ops.extract_patches(img, f, 32))
    if orientation:
        lafs = make_upright(lafs).contiguous()
        ang = _ops.patch_orientation(extract(lafs)[:, :, 0], 36)
        assert bits(ang[~dead]) == bits(angles[~dead]) and bool((ang[~dead] != 0).any())
        lafs = torch.cat([torch.matmul(lafs[..., :2, :2], _rotation(rad2deg(ang))), lafs[..., :2, 2:]], dim=3).contiguous()
    want = net(extract(lafs).view(32, 1, 32, 32)).view(2, 16, 128)
    assert bits(desc[~dead]) == bits(want[~dead])
    # lafs= gives what kpts + scale give
    if not orientation:
        again = describe_keypoints(img, None, count, lafs=lafs, pyramid=pyramid, descriptor=net)[0]
        assert bits(again[~dead]) == bits(desc[~dead]) and not again[1, 11:].any()


def test_descriptor_none_is_the_sift_path(cuda):
    from cirtorch.search import describe_keypoints
    img, kp, count = _images(cuda)
    for kw in (dict(), dict(orientation=True, pyramid=True, scale=40.0)):
        a = describe_keypoints(img, kp, count, **kw)
        b = describe_keypoints(img, kp, count, descriptor=None, **kw)
        assert a[0].shape == (2, 16, 128) and all(bits(p) == bits(q) for p, q in zip(a, b))


def test_graph_capture_replay_equals_eager(cuda, nets, x129):
    """one stream, no parallel branches: trunk and head of the module's forward in a torch.cuda.graph"""
    from cirtorch.utils.graph import GraphedForward
    net = nets["sosnet"]
    xs = [x129[0:65, None].contiguous(), x129[64:129, None].contiguous()]
    g = GraphedForward(net, xs[0])
    for t in (xs[1], xs[0]):
        got = g(t).clone()
        assert bits(got) == bits(net(t))
