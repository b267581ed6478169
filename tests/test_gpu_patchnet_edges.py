"""GPU checks of the learned patch descriptors (rr_patchnet.hip) where tests/test_gpu_patchnet.py cannot see:

A. probe weights (one entry +-1 per output channel, packed scale exactly 1.0f): every accumulation has one
   non-zero term, so the trunk's layer-6 map must equal the numpy restatement BIT FOR BIT
   (test_host_patchnet_edges.py shows that restatement to be plain index arithmetic on the fp16 normalised
   patch).  The normalisation window shows all 1024 normalised pixels with both signs: it pins the float64
   statistics, 1023 against 1024, both eps values and the one float64 -> fp16 rounding to the bit, on ordinary
   patches and on the edge patches of C.  The geometry probes put each of the 9 taps of each of layers 2 .. 6
   under a channel map ci = (5 co + 3) mod cin: the [K-step][cout][32] packing, the chunk order, the cout tiles,
   the stride-2 phase and the zero halo on all four borders.  The head probe calls rr_patchnet_head on hand-made
   integer maps under a one-hot layer 7 for B in 1, 15, 16, 17, 33 with a sentinel row behind the output, and
   once more with two different BatchNorm variances, which makes BatchNorm's 1e-5 matter at order 1.
B. past the 65535-block cap (patchnet_cases.cap_seven: seven kinds, 65535 mod 7 == 1, so a block's second patch is
   of the next kind).  Which kernel's second trip each test executes:
     test_trunk_and_describe_past_the_cap  k_patchnet_trunk: blocks 0 .. 69 of one launch of 65605 patches re-zero
                                           and reuse both LDS regions (rr_patchnet_trunk, and rr_patchnet_describe
                                           under PATCHNET_CHUNK = 65605, which the tuning table accepts)
     test_head_past_the_cap                k_patchnet_head: blocks 0 .. 2 of one launch of 16 x 65535 + 37 maps
                                           (17.2 GB) reuse part[][][] behind the two barriers, waves 1 .. 7 by
                                           `continue`; the last tile has 5 live rows
C. the fixture tests/golden/patchnet_edges.npz: patches on which HardNet's + 1e-6, SOSNet's + 1e-5 and the
   float64 statistics decide the descriptor at order 1, against the float64 reference modules within 4 x the
   restatement's own difference (the discrimination of every group is asserted on the CPU).
D. non-finite patches: a patch with a NaN or an infinite pixel gives an all-NaN map and descriptor, as the
   reference and the restatement do, and no other patch of the batch changes a bit; through describe_keypoints
   the NaN rows match nothing.

Measured on the MI355X (every test prints its figures before it asserts; pytest -s):
  window               24 patches (12 ordinary, 12 of C), 196,608 map entries per variant: 0 differ in bits
                       (6,192 / 8,110 distinct non-zero fp16 values, HardNet / SOSNet)
  geometry             layers 2 .. 6, 9 taps x 4 patches x 8,192 entries each: 0 differ in bits, 9 distinct maps a layer
  head probe           |diff| / |want| at most 1.15, 1.44, 1.44, 1.44, 1.50 x 2^-24 for B = 1, 15, 16, 17, 33 (bound 12),
                       both variants; the sentinel row untouched.  Two variances: 2.32 x 2^-24 of the largest entry
                       (bound 14); dropping BatchNorm's 1e-5 would move the descriptor by 0.020
  trunk, fused, cap    65,605 patches in one launch: 0 maps and 0 descriptors differ in bits from their kind; the seven
                       within 1.3e-4 .. 2.3e-4 of the float64 reference (tolerances 5.8e-4 .. 1.28e-3); 0.18 s / 0.04 s
  head, cap            1,048,597 maps (17.2 GB), not skipped: 0 descriptors differ in bits from their kind, both
                       variants; the launch takes 0.011 s, the whole test 0.57 s (0.49 s of it tiling the maps)
  edge fixture         HardNet: hard_eps 1.8e-4 (tol 8.1e-4), sos_eps 2.6e-4 (9.2e-4), offset 1.9e-4 (9.3e-4), huge
                       2.9e-4 (9.5e-4), ulp 1.2e-4 (4.6e-4); SOSNet: 1.3e-4 (5.8e-4), 2.0e-4 (7.6e-4), 2.0e-4 (8.1e-4),
                       3.0e-4 (1.17e-3), 1.7e-4 (6.8e-4)
  non-finite           before the trunk's check (the parent commit): no NaN at all; the four patches got one and the
                       same finite map (norm 41.8 HardNet, 30.5 SOSNet) and one descriptor of norm 1.0, and the 3
                       keypoints on the NaN pixel got finite rows: both tests failed.  Now every entry of those maps
                       and descriptors is NaN, the 33 finite patches keep their bits, and the 3 rows match nothing
The whole file takes 4 s.
"""

import time

import numpy as np
import pytest
import torch

import patchnet_cases as NC
from conftest import golden
from test_gpu_patchnet import _images, _module, bits

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -24     # half a float32 ulp relative: the bound of one correctly rounded float32 operation


@pytest.fixture(scope="module")
def fix():
    return golden("patchnet_edges.npz")


@pytest.fixture(scope="module")
def nets(cuda):
    return {v: _module(v, NC.SEEDS[v], cuda) for v in NC.VARIANTS}


def pack(params, cuda):
    from cirtorch import _ops
    return _ops.patchnet_pack(*[[torch.from_numpy(a).to(cuda) for a in group] for group in params])


def map_bits(t):
    """fp16 values (a device tensor, or float64 / float16 numpy) -> uint16 numpy"""
    if torch.is_tensor(t):
        assert t.dtype == torch.float16
        return t.detach().cpu().contiguous().numpy().view(np.uint16)
    return np.ascontiguousarray(np.asarray(t).astype(np.float16)).view(np.uint16)


def same_bits(a, b):
    view = {torch.float16: torch.int16, torch.float32: torch.int32}[a.dtype]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def probe_patches():
    """ordinary patches (the four bright corners, constant, zero, noise, smoothed, 0 .. 255) and every patch of C"""
    return np.concatenate([NC.patches()[:12]] + list(NC.edge_patches().values()))


# ---------------------------------------------------------------- A. probes
@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_normalisation_window_bitwise(cuda, variant):
    from cirtorch import _ops
    x = probe_patches()
    params = NC.probe_params(NC.window_spec())
    want = map_bits(NC.quantised_net(x, params, variant)[1])
    got = map_bits(_ops.patchnet_trunk(torch.from_numpy(x).to(cuda), pack(params, cuda), variant))
    bad = got != want
    print("%s window: %d patches, %d map entries, %d differ in bits; %d distinct non-zero fp16 values"
          % (variant, len(x), got.size, bad.sum(), len(np.unique(want[want != 0]))))
    assert got.shape == want.shape == (len(x), 8, 8, 128)
    assert not bad.any(), np.argwhere(bad)[:8]
    assert len(np.unique(want)) > 5000


@pytest.mark.parametrize("layer", range(2, 7))
def test_geometry_probes_bitwise(cuda, layer):
    from cirtorch import _ops
    x = NC.patches()[[0, 3, 6, 8]]         # two bright corners (the halo), noise, values in 0 .. 255
    xd = torch.from_numpy(x).to(cuda)
    differ, seen = 0, set()
    for tap in range(9):
        variant = NC.VARIANTS[tap % 2]
        params = NC.probe_params(NC.geometry_spec(layer, tap))
        want = map_bits(NC.quantised_net(x, params, variant)[1])
        got = map_bits(_ops.patchnet_trunk(xd, pack(params, cuda), variant))
        differ += int((got != want).sum())
        assert np.array_equal(got, want), (layer, tap, np.argwhere(got != want)[:8])
        seen.add(want.tobytes())
        assert (want != 0).mean() > 0.05
    print("layer %d: 9 taps x %d patches x 8192 map entries, %d differ in bits, %d distinct maps" % (layer, len(x), differ, len(seen)))
    assert len(seen) == 9


def run_head(maps, B, variant, packed, rows):
    """rr_patchnet_head on the first B maps into a [rows, 128] buffer filled with a sentinel"""
    from cirtorch import _engine as E, _ops
    out = torch.full((rows, 128), -7.25, dtype=torch.float32, device=maps.device)
    E.check(E.lib().rr_patchnet_head(E.ptr(maps), B, _ops.PATCHNET_VARIANTS[variant], E.ptr(packed), E.ptr(out), _ops._st()),
            "rr_patchnet_head")
    return out


@pytest.mark.parametrize("variant", NC.VARIANTS)
@pytest.mark.parametrize("B", (1, 15, 16, 17, 33))
def test_head_probe(cuda, variant, B):
    """f[co] = map[ky, kx, ci] exactly (integers below 251, one non-zero term, scale 1.0f, shift 0).  What is
    left is the float32 descriptor normalisation: v = f + 1e-10f (SOSNet; one rounding, and 1e-10f is within
    2^-24 of 1e-10), the sum of 128 squares by 8 fmaf in the lane and 4 butterfly additions (12 roundings of a sum
    of non-negative terms: 12 x 2^-24 relative, half of it on the root), one square root, one quotient: first
    order (1 + 1 + 6 + 1 + 1) 2^-24 = 10 x 2^-24 of the entry; asserted at 12 x 2^-24."""
    maps = NC.head_maps(B)
    packed = pack(NC.probe_params(NC.centre_spec()), cuda)
    md = torch.from_numpy(maps).to(cuda)
    out = run_head(md, B, variant, packed, B + 1)
    got = out.cpu().numpy().astype(np.float64)
    want = NC.head_expected(maps, variant)
    err = np.abs(got[:B] - want)
    worst = (err / np.maximum(np.abs(want), 1e-300)).max() if want.any() else 0.0
    print("%s head probe B=%d: largest |diff| / |want| = %.2f x 2^-24 (bound 12)" % (variant, B, worst / ULP32))
    assert (got[B] == -7.25).all()                                  # the row behind the output is untouched
    assert (err <= 12 * ULP32 * np.abs(want)).all()
    if B > 2:
        assert bits(out[2]) == bits(torch.zeros(128)) if variant == "hardnet" else abs(got[2] - 1 / np.sqrt(128)).max() <= 1e-7
    # a row does not depend on the rows clamped in behind it
    assert bits(out[:B]) == bits(run_head(torch.cat([md, md.flip(0)]), 2 * B, variant, packed, 2 * B)[:B])


@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_head_probe_with_two_batchnorm_variances(cuda, variant):
    """layer 7's running_var is 9e-5 on even channels and 1e-5 on odd ones, running_mean 1 on channels 4 k and
    4 k + 1: the scales are 1 / sqrt(9e-5 + 1e-5) = 100 and 1 / sqrt(2e-5) = 224, and 105 and 316 if the 1e-5 were
    dropped, which turns the descriptor at order 1.  Reference: float64 with scale and shift the float32
    values rr.h states.  On top of test_head_probe's 10 x 2^-24 come one rounding of fmaf(acc, scale, shift) on
    the numerator and as much on the norm: asserted at 14 x 2^-24 of the descriptor's largest entry (fmaf rounds
    once, and the float64 products are exact, so a cancellation in acc scale + shift costs nothing more)."""
    B = 17
    maps = NC.head_maps(B)
    w, m, v = NC.probe_params(NC.centre_spec())
    v[6][0::2] = np.float32(9e-5)
    v[6][1::2] = np.float32(1e-5)
    m[6][::4] = m[6][1::4] = 1.0
    s64 = 1.0 / np.sqrt(v[6].astype(np.float64) + 1e-5)
    scale, shift = s64.astype(np.float32).astype(np.float64), (-m[6].astype(np.float64) * s64).astype(np.float32).astype(np.float64)
    s = NC.head_spec()
    acc = maps.astype(np.float64)[:, s["ky"], s["kx"], s["ci"]]
    want = NC.normalise_output(acc * scale + shift, variant)
    dropped = NC.normalise_output((acc - m[6]) / np.sqrt(v[6].astype(np.float64)), variant)
    got = run_head(torch.from_numpy(maps).to(cuda), B, variant, pack((w, m, v), cuda), B)[:B].cpu().numpy().astype(np.float64)
    err, big = np.abs(got - want).max(axis=1), np.abs(want).max(axis=1)
    print("%s head, two variances: largest |diff| = %.2f x 2^-24 of the largest entry (bound 14); without the 1e-5 the "
          "descriptor moves by %.3f" % (variant, (err / big).max() / ULP32, np.abs(dropped - want).max()))
    assert np.abs(dropped - want).max() > 0.01       # 1e5 x the bound below
    assert (err <= 14 * ULP32 * big).all()


# ---------------------------------------------------------------- B. past the cap
def check_seven(fix, variant, desc7, maps7):
    """the seven distinct patches by the existing float64 criteria: patchnet.npz for the six that come from
    patches(), patchnet_edges.npz for the near-constant one"""
    g = golden("patchnet.npz")
    src = [NC.ZERO, 3, NC.CONSTANT, 6, None, 7, 8]
    got = desc7.cpu().numpy().astype(np.float64)
    for k, i in enumerate(src):
        if i is None:
            want, tol = fix["%s_hard_eps_desc" % variant][1].astype(np.float64), float(fix["%s_hard_eps_tol" % variant])
        else:
            want, tol = g[variant + "_desc"][i].astype(np.float64), g[variant + "_tol"][0]
        diff = np.abs(got[k] - want).max()
        print("%s kind %d: max |diff| %.3e (tol %.3e)" % (variant, k, diff, tol))
        assert diff <= tol, (k, diff, tol)
    for k, i in ((3, 6), (5, 7)):          # the maps the fixture holds
        want = g[variant + "_map"][list(NC.MAP_PATCHES).index(i)]
        rel = np.abs(maps7[k].cpu().numpy().astype(np.float64) - want).max() / np.abs(g[variant + "_map"]).max()
        assert rel <= g[variant + "_tol"][1], (k, rel)


@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_trunk_and_describe_past_the_cap(cuda, fix, nets, variant):
    from cirtorch import _engine as E, _ops
    packed = nets[variant].packed()
    x7 = torch.from_numpy(NC.cap_seven()).to(cuda)
    maps7 = _ops.patchnet_trunk(x7, packed, variant)
    desc7 = _ops.patchnet_describe(x7, packed, variant)
    assert same_bits(desc7, _ops.patchnet_head(maps7, packed, variant))
    check_seven(fix, variant, desc7, maps7)
    # the zero and the constant patch normalise to the same zeros: six different maps
    assert len({bits(m) for m in maps7}) == 6 and bits(maps7[0]) == bits(maps7[2])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kind = torch.from_numpy(NC.cap_kinds(NC.CAP_P)).to(cuda)
    X = x7[kind].contiguous()
    maps = _ops.patchnet_trunk(X, packed, variant)                   # one launch of 65535 blocks
    wrong_maps = int((maps.view(torch.int16) != maps7.view(torch.int16)[kind]).reshape(NC.CAP_P, -1).any(1).sum())
    del maps
    chunk = E.get_tuning("PATCHNET_CHUNK")
    with E.tuning(PATCHNET_CHUNK=NC.CAP_P):                          # one trunk launch and one head launch of P
        assert E.get_tuning("PATCHNET_CHUNK") == NC.CAP_P
        desc = _ops.patchnet_describe(X, packed, variant)
    assert E.get_tuning("PATCHNET_CHUNK") == chunk
    wrong_desc = int((desc.view(torch.int32) != desc7.view(torch.int32)[kind]).any(1).sum())
    torch.cuda.synchronize()
    print("%s: %d patches in one launch: %d maps and %d descriptors differ in bits from their kind; %.2f s"
          % (variant, NC.CAP_P, wrong_maps, wrong_desc, time.perf_counter() - t0))
    assert tuple(desc.shape) == (NC.CAP_P, 128)
    assert wrong_maps == 0 and wrong_desc == 0


def test_head_past_the_cap(cuda, nets):
    """B = 16 x 65535 + 37 maps, tiled on the device from seven distinct maps: the layer-6 maps of cap_seven
    (HardNet's trunk) with the all-zero map in place of the constant patch's; the head of both variants runs on
    them"""
    from cirtorch import _ops
    free = torch.cuda.mem_get_info()[0]
    if free < 24 << 30:
        pytest.skip("%.1f GiB free, the batch of maps needs 24 GiB" % (free / 2.0 ** 30))
    x7 = torch.from_numpy(NC.cap_seven()).to(cuda)
    maps7 = _ops.patchnet_trunk(x7, nets["hardnet"].packed(), "hardnet")
    maps7[2] = 0            # the constant patch has the zero patch's map (both normalise to zeros): the zero map instead
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kind = torch.from_numpy(NC.cap_kinds(NC.CAP_HEAD_B)).to(cuda)
    big = maps7[kind]
    assert tuple(big.shape) == (NC.CAP_HEAD_B, 8, 8, 128) and big.is_contiguous()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for variant in NC.VARIANTS:
        packed = nets[variant].packed()
        desc7 = _ops.patchnet_head(maps7, packed, variant)
        assert len({bits(d) for d in desc7}) == 7 and bool(torch.isfinite(desc7).all())
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        desc = _ops.patchnet_head(big, packed, variant)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        wrong = int((desc.view(torch.int32) != desc7.view(torch.int32)[kind]).any(1).sum())
        print("%s head on %d maps (%.1f GB): %.3f s the launch, %d descriptors differ in bits from their kind"
              % (variant, NC.CAP_HEAD_B, big.numel() * 2 / 1e9, t3 - t2, wrong))
        assert tuple(desc.shape) == (NC.CAP_HEAD_B, 128) and wrong == 0
        del desc
    print("head past the cap: %.2f s building the maps, %.2f s in all" % (t1 - t0, time.perf_counter() - t0))
    del big
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- C. the edge fixture
@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_edge_patches_against_reference(cuda, fix, nets, variant):
    edges = NC.edge_patches()
    worst = {}
    for g, x in edges.items():
        got = nets[variant](torch.from_numpy(x).to(cuda)[:, None]).cpu().numpy().astype(np.float64)
        want, tol = fix["%s_%s_desc" % (variant, g)].astype(np.float64), float(fix["%s_%s_tol" % (variant, g)])
        worst[g] = (np.abs(got - want).max(), tol)
        print("%s %-8s max |diff| %.3e (tol %.3e)" % (variant, g, worst[g][0], tol))
    for g, (diff, tol) in worst.items():
        assert diff <= tol, (g, diff, tol)


# ---------------------------------------------------------------- D. non-finite patches
def report_nonfinite(what, t, bad):
    """print what the non-finite patches gave before anything is asserted"""
    rows = t[bad].reshape(int(bad.sum()), -1).float()
    nan = torch.isnan(rows).float().mean(1).cpu().numpy()
    norm = torch.nan_to_num(rows).norm(dim=1).cpu().numpy()
    same = all(bits(r) == bits(rows[0]) for r in rows)
    print("%s of the non-finite patches: share of NaN entries %s, norm of the rest %s, all rows alike %s" % (what, nan, norm, same))


@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_non_finite_patches(cuda, nets, variant):
    from cirtorch import _ops
    x, where = NC.nonfinite_batch()
    bad = torch.zeros(len(x), dtype=torch.bool, device=cuda)
    bad[where] = True
    xd = torch.from_numpy(x).to(cuda)
    packed = nets[variant].packed()
    maps = _ops.patchnet_trunk(xd, packed, variant)
    chain = _ops.patchnet_head(maps, packed, variant)
    fused = _ops.patchnet_describe(xd, packed, variant)
    report_nonfinite(variant + " map", maps, bad)
    report_nonfinite(variant + " descriptor (trunk, head)", chain, bad)
    report_nonfinite(variant + " descriptor (describe)", fused, bad)
    alone_maps = _ops.patchnet_trunk(xd[~bad], packed, variant)
    alone = _ops.patchnet_describe(xd[~bad], packed, variant)
    # every finite patch keeps the bits it has when run alone
    assert same_bits(maps[~bad], alone_maps)
    assert same_bits(chain[~bad], alone) and same_bits(fused[~bad], alone) and bool(torch.isfinite(alone).all())
    assert same_bits(_ops.patchnet_head(maps[~bad].contiguous(), packed, variant), alone)
    # the non-finite ones are all NaN
    assert bool(torch.isnan(maps[bad]).all())
    assert bool(torch.isnan(chain[bad]).all()) and bool(torch.isnan(fused[bad]).all())
    assert bool(torch.isnan(nets[variant](xd[:, None])[bad]).all())


def test_describe_keypoints_with_a_nan_pixel(cuda, nets):
    from cirtorch import _ops
    from cirtorch.search import describe_keypoints, match_pairs
    net = nets["hardnet"]
    img, kp, count = _images(cuda)
    clean, _ = describe_keypoints(img, kp, count, scale=12.0, descriptor=net)
    hurt = img.clone()
    px, py = (int(v) for v in kp[0, 5].round().tolist())             # inside the patch of keypoint 5 of image 0
    hurt[0, 0, py + 3, px - 2] = float("nan")
    desc, _ = describe_keypoints(hurt, kp, count, scale=12.0, descriptor=net)
    dead = torch.zeros((2, 16), dtype=torch.bool, device=cuda)
    dead[0, 3] = True
    dead[1, 11:] = True
    lafs = torch.zeros((2, 16, 2, 3), device=cuda)
    lafs[..., 0, 0] = 12.0
    lafs[..., 1, 1] = 12.0
    lafs[..., 2] = kp
    lafs[dead] = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], device=cuda)
    touch = torch.isnan(_ops.extract_patches(hurt, lafs.contiguous(), 32)).reshape(2, 16, -1).any(-1) & ~dead
    print("keypoints whose patch holds the NaN pixel: %d of %d live; their rows: share of NaN %.3f"
          % (int(touch.sum()), int((~dead).sum()), float(torch.isnan(desc[touch]).float().mean())))
    assert 0 < int(touch.sum()) < int((~dead[0]).sum()) and not bool(touch[1].any())
    assert not desc[dead].any()                                       # dead slots stay zero
    assert same_bits(desc[~dead & ~touch], clean[~dead & ~touch])     # other keypoints keep their bits
    assert bool(torch.isnan(desc[touch]).all())
    # the NaN rows match nothing, on either side
    for mode in ("nn", "mnn", "snn", "smnn"):
        m12, _ = match_pairs(desc[0], clean[0], mode=mode, th=0.95)
        m21, _ = match_pairs(clean[0], desc[0], mode=mode, th=0.95)
        assert bool((m12[touch[0]] == -1).all()), mode
        hit = m21[m21 >= 0]
        assert not bool(touch[0][hit].any()), mode
        if mode == "nn":
            live = ~dead[0] & ~touch[0]
            assert bool((m12[live] == torch.arange(16, device=cuda)[live]).all())     # the others find themselves
