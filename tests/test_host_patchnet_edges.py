"""CPU checks of what tests/test_gpu_patchnet_edges.py relies on (numpy only, no GPU):

 - the probe weights of patchnet_cases give a packed scale of exactly 1.0f and a shift of zero;
 - under them quantised_net's layer-6 map is plain index arithmetic on f16(normalise_input(x)): the closed
   form of the normalisation window, and patchnet_cases.probe_map for every geometry probe;
 - the one-hot layer 7 makes the features the map entries it names;
 - the patchnet_edges.npz fixture is reproduced from the seeds (inputs, tolerances against the stored
   float64 reference, the bound between the two restatements over the 129 patches, printed);
 - every discrimination condition of patchnet_cases.EDGE_PINS: the restatement with the pinned constant
   altered misses the reference by more than 10 x the group's tolerance;
 - the restatement gives all-NaN maps and descriptors for the non-finite patches, as the reference does
   (recorded in the fixture), and leaves the finite patches of the batch alone;
 - the seven patches of the cap tests follow one another as patchnet_cases.cap_seven says.

Constants that no group of the fixture pins at 10 x its tolerance (printed ratios of the generator, 0.2 .. 0.4):
the unbiased 1023 and two-pass float32 statistics on ordinary ranges.  They are pinned bit for bit by the
normalisation window of the GPU test alone."""

import numpy as np
import pytest

import patchnet_cases as NC
from conftest import golden


@pytest.fixture(scope="module")
def fix():
    return golden("patchnet_edges.npz")


def n16_of(x, variant):
    return NC.f16(NC.normalise_input(x.astype(np.float64), variant))


def probe_inputs():
    edges = NC.edge_patches()
    return np.concatenate([NC.patches()[[0, 3, 6, 8]], edges["hard_eps"][1:2], edges["offset"][:1]])


def test_probe_scale_is_exactly_one():
    v = NC.PROBE_VAR
    assert v.dtype == np.float32 and v != 1
    assert np.float32(1 / np.sqrt(np.float64(v) + 1e-5)) == np.float32(1)
    w, m, var = NC.probe_params(NC.window_spec())
    for wl, ml, vl in zip(w, m, var):
        assert (np.float32(1 / np.sqrt(vl.astype(np.float64) + 1e-5)) == 1).all() and not ml.any()
        flat = wl.reshape(wl.shape[0], -1)
        assert ((flat != 0).sum(1) == 1).all() and set(np.unique(flat)) <= {-1.0, 0.0, 1.0}


@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_window_is_index_arithmetic(variant):
    x = probe_inputs()
    n16 = n16_of(x, variant)
    spec = NC.window_spec()
    qmap = NC.quantised_net(x, NC.probe_params(spec), variant)[1]
    seen = np.zeros((2, 32, 32), dtype=int)
    for c in range(128):
        cc = c % 32
        s, ay, ax, by, bx = 1 - 2 * (cc >> 4), cc >> 3 & 1, cc >> 2 & 1, cc >> 1 & 1, cc & 1
        want = np.maximum(s * n16[:, ay + 2 * by::4, ax + 2 * bx::4], 0.0)
        assert want.shape == (len(x), 8, 8) and np.array_equal(qmap[..., c], want), c
        if c < 32:
            seen[cc >> 4, ay + 2 * by::4, ax + 2 * bx::4] += 1
    assert (seen == 1).all()            # every normalised pixel once with each sign
    assert np.array_equal(qmap, NC.probe_map(n16, spec))
    assert (qmap > 0).mean() > 0.3 and len(np.unique(qmap)) > 1000


@pytest.mark.parametrize("layer", range(2, 7))
def test_geometry_probes_are_index_arithmetic(layer):
    x = probe_inputs()[:3]
    n16 = n16_of(x, "hardnet")
    maps = []
    for tap in range(9):
        spec = NC.geometry_spec(layer, tap)
        s = spec[layer - 1]
        assert sorted(set(s["ci"])) == list(range(NC.LAYERS[layer - 1][1])) and (s["ky"] * 3 + s["kx"] == tap).all()
        qmap = NC.quantised_net(x, NC.probe_params(spec), "hardnet")[1]
        assert np.array_equal(qmap, NC.probe_map(n16, spec)), tap
        maps.append(qmap)
    # the nine taps give nine different maps, and the border taps read the zero halo on their side
    for i in range(9):
        for j in range(i):
            assert not np.array_equal(maps[i], maps[j]), (i, j)
    # tap (0, 0) reads the top and left halo (seen by map channels below 32), tap (2, 2) of a stride-1 layer the
    # bottom and right one (seen by channels from 96); the centre tap has values there
    assert not maps[0][:, 0, :, :32].any() and not maps[0][:, :, 0, :32].any()
    assert maps[4][:, 0, :, :32].any() and maps[4][:, :, 0, :32].any()
    if NC.LAYERS[layer - 1][3] == 1:
        assert not maps[8][:, 7, :, 96:].any() and not maps[8][:, :, 7, 96:].any()
        assert maps[4][:, 7, :, 96:].any() and maps[4][:, :, 7, 96:].any()


def test_channels_of_the_centre_routing_differ_at_every_structured_offset():
    """a swap of 32-channel chunks, of 16-channel tiles, of the 8 values of a lane or of neighbours would show: at
    every layer's output no channel equals the one a power of two away"""
    n16 = n16_of(probe_inputs()[2:3], "hardnet")
    spec = NC.centre_spec()
    for upto in range(1, 7):
        part = spec[:upto] + [dict(ci=np.arange(c[0]), ky=np.ones(c[0], int), kx=np.ones(c[0], int), sign=np.ones(c[0], int))
                              for c in NC.LAYERS[upto:6]]
        if any(NC.LAYERS[l][0] != NC.LAYERS[l][1] for l in range(upto, 6)):
            continue        # an identity tail needs cin == cout: layers 5 and 6, and the whole net
        m = NC.probe_map(n16, part)[0].reshape(64, -1)
        for off in (1, 2, 4, 8, 16, 32, 64):
            for c in range(m.shape[1] - off):
                assert not np.array_equal(m[:, c], m[:, c + off]), (upto, c, off)
    m = NC.probe_map(n16, spec)[0].reshape(64, 128)
    assert len({m[:, c].tobytes() for c in range(128)}) >= 48


@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_head_probe_features_are_map_entries(variant):
    maps = NC.head_maps(17)
    assert maps.dtype == np.float16 and not maps[2].any() and maps.max() == 250
    s = NC.head_spec()
    assert len(set(zip(s["ky"], s["kx"], s["ci"]))) == 128 and len(set(8 * s["ky"] + s["kx"])) == 64
    w7 = NC.probe_params(NC.centre_spec())[0][6]
    f = NC.conv_nhwc(maps.astype(np.float64), w7, 1, 0).reshape(17, 128)
    assert np.array_equal(f, maps.astype(np.float64)[:, s["ky"], s["kx"], s["ci"]])
    d = NC.head_expected(maps, variant)
    if variant == "hardnet":
        assert not d[2].any()
    else:
        assert np.abs(d[2] - 1 / np.sqrt(128)).max() < 1e-15
    assert np.abs(np.linalg.norm(d[[0, 1, 3]], axis=1) - 1).max() < 1e-12


def test_fixture_inputs_and_tolerances_from_the_seeds(fix):
    edges = NC.edge_patches()
    assert int(fix["edge_seed"]) == NC.EDGE_SEED and tuple(edges) == NC.EDGE_GROUPS
    for g, x in edges.items():
        assert x.dtype == np.float32 and float(fix[g + "_chk"]) == NC.checksum([x]), g
    # the patches are what the group names say
    sd = edges["hard_eps"].astype(np.float64).std(axis=(1, 2), ddof=1)
    assert np.allclose(sd, (0.5e-6, 1e-6, 2e-6), rtol=1e-3)
    var = edges["sos_eps"].astype(np.float64).var(axis=(1, 2))
    assert np.allclose(var, (0.5e-5, 1e-5, 2e-5), rtol=1e-3)
    off = edges["offset"].astype(np.float64) - 1e6
    assert (off == np.floor(off)).all() and off.min() >= 0 and off.max() <= 255
    with np.errstate(over="ignore"):
        assert np.isfinite(edges["huge"] ** 2).all() and not np.isfinite((edges["huge"] ** 2).sum(dtype=np.float32))
    for u in edges["ulp"]:
        assert sorted(np.unique(u)) == [0.5, np.nextafter(np.float32(0.5), np.float32(1))] and (u != 0.5).sum() == 1


@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_tolerances_and_discrimination(fix, variant):
    params = NC.net_params(NC.SEEDS[variant])
    for g, x in NC.edge_patches().items():
        ref, tol = fix["%s_%s_desc" % (variant, g)].astype(np.float64), float(fix["%s_%s_tol" % (variant, g)])
        q = NC.quantised_net(x, params, variant)[0]
        diff = np.abs(q - ref).max()
        # 1e-7: the reference is stored as float32
        assert abs(4 * diff - tol) <= 4e-7 and 1e-4 < tol < 2e-3, (g, diff, tol)
        for v, how in NC.EDGE_PINS[g]:
            if v != variant:
                continue
            with np.errstate(all="ignore"):
                miss = np.abs(NC.quantised_net_altered(x, params, variant, how) - ref)
            ratio = np.where(np.isfinite(miss), miss, np.inf).max() / tol
            print("%s %s: tol %.3e, %s misses by %.3g x tol" % (variant, g, tol, how, ratio))
            assert ratio > 10, (g, how, ratio)
    assert NC.normalise_input.__name__ == "normalise_input"      # quantised_net_altered put it back


@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_restatements_differ_by_the_stored_bound(fix, variant):
    x, params = NC.patches(), NC.net_params(NC.SEEDS[variant])
    q, qmap = NC.quantised_net(x, params, variant)
    q32, qmap32 = NC.quantised_net_f32(x, params, variant)
    d = np.abs(q - q32).max()
    moved = (qmap != qmap32).mean()
    print("%s: float64 vs float32 accumulation over %d patches: descriptors %.3e (bound 4 x = %.3e), %.2f %% of the "
          "map's fp16 entries differ" % (variant, len(x), d, 4 * d, 100 * moved))
    # the float32 matmul's summation order belongs to the BLAS in use: the stored bound is the generator's run
    assert 0.8 * 4 * d <= float(fix[variant + "_f32_tol"]) <= 1.25 * 4 * d
    assert 2e-5 < d < 3e-4 and 0 < moved < 0.2
    g = golden("patchnet.npz")
    assert 4 * d < 0.5 * g[variant + "_tol"][0]                   # the new bound is less than half the old one


@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_restatement_on_non_finite_patches(fix, variant):
    x, where = NC.nonfinite_batch()
    assert x.shape == (37, 32, 32) and where == [0, 16, 17, 36]
    bad = np.zeros(37, dtype=bool)
    bad[where] = True
    assert np.array_equal(~np.isfinite(x).all(axis=(1, 2)), bad) and np.array_equal(x[~bad], NC.patches()[:33])
    assert fix[variant + "_nonfinite"].all()                      # the reference: all NaN
    params = NC.net_params(NC.SEEDS[variant])
    with np.errstate(all="ignore"):
        q, qmap = NC.quantised_net(x, params, variant)
    assert np.isnan(q[bad]).all() and np.isnan(qmap[bad]).all()
    alone, alone_map = NC.quantised_net(x[~bad], params, variant)
    assert np.array_equal(q[~bad], alone) and np.array_equal(qmap[~bad], alone_map)


def test_order_of_the_seven_cap_patches():
    seven = NC.cap_seven()
    assert seven.shape == (7, 32, 32) and seven.dtype == np.float32 and NC.CAP % 7 == 1
    assert not seven[0].any() and seven[1].max() == 8.0 and len(np.unique(seven[2])) == 1 and seven[6].max() > 200
    assert 0 < seven[4].std() < 2e-6
    assert len({s.tobytes() for s in seven}) == 7
    kind = NC.cap_kinds(NC.CAP_P)
    second = kind[NC.CAP:]                                         # blocks 0 .. 69, second trip
    assert len(second) == 70 and (second == (kind[:70] + 1) % 7).all()
    pairs = set(zip(kind[:70], second))
    assert len(pairs) == 7 and (0, 1) in pairs and (6, 0) in pairs      # zero -> bright, 0 .. 255 -> zero
    assert (NC.CAP_HEAD_B + 15) // 16 == NC.CAP + 3 and NC.CAP_HEAD_B % 16 == 5
