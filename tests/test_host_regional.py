"""Host side of regional pooling (no GPU): the region grid against the
rectangles recorded from the reference ``Rpool.roipool`` (tests/golden/
regions.npz, make_golden_regional.py), the pooling registry, the state-dict
schema of the regional head, ``init_network`` flags, and the argument checks of
``rr_region_pool`` / ``rr_region_aggregate``."""

import ctypes
import os

import pytest
import torch
import torch.nn as nn

from conftest import PKG, golden

LIB = os.path.join(PKG, "librr.so")

# region counts the reference gives (recorded in regions.npz as well)
COUNTS = {(24, 32): 21, (7, 7): 15, (3, 11): 45, (2, 7): 39, (1, 1): 2, (1, 6): 8, (12, 40): 39}


def test_roi_regions_equal_the_recorded_rectangles():
    from cirtorch.layers.regions import roi_regions
    g = golden("regions.npz")
    shapes, offsets, rects = g["shapes"], g["offsets"], g["rects"]
    assert len(shapes) >= 1600 + 36 and (3, 13, 4) in {tuple(int(v) for v in s) for s in shapes}
    seen_l = set()
    for (h, w, L), a, b in zip(shapes, offsets[:-1], offsets[1:]):
        ref = [tuple(int(v) for v in r) for r in rects[a:b]]
        got = roi_regions(int(h), int(w), int(L))
        assert got == ref, (h, w, L)
        assert got[0] == (0, 0, h, w)
        seen_l.add(int(L))
    assert seen_l == {1, 2, 3, 4}


@pytest.mark.parametrize("hw,count", sorted(COUNTS.items()))
def test_roi_regions_counts(hw, count):
    from cirtorch.layers.regions import roi_regions
    regs = roi_regions(*hw)
    assert len(regs) == count
    for (y0, x0, h, w) in regs:
        assert 0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= hw[0] and x0 + w <= hw[1]


def test_roi_regions_maxima():
    from cirtorch.layers.regions import roi_regions
    assert max(len(roi_regions(h, w, 3)) for h in range(1, 41) for w in range(1, 41)) == 51
    assert max(len(roi_regions(h, w, 4)) for h in range(1, 41) for w in range(1, 41)) == 91


def test_registry_constructs_gemmp_and_roipool():
    from cirtorch.layers.pooling import GeM, GeMmp, MAC, Rpool
    from cirtorch.modules.pools import POOLING_LAYERS
    m = POOLING_LAYERS["GeMmp"](p=3, mp=16, eps=1e-6)
    assert isinstance(m, GeMmp) and tuple(m.p.shape) == (16, 1, 1) and float(m.p.min()) == 3.0
    r = POOLING_LAYERS["ROIpool"](rpool=GeM(), whiten=nn.Linear(8, 8), L=2)
    assert isinstance(r, Rpool) and r.L == 2 and isinstance(r.rpool, GeM)
    assert isinstance(POOLING_LAYERS["ROIpool"](rpool=MAC()).rpool, MAC)
    with pytest.raises(NotImplementedError, match=r"Rpool\(MAC\(\)\)"):
        POOLING_LAYERS["RMAC"]()
    with pytest.raises(NotImplementedError):
        POOLING_LAYERS["ROIpool"](rpool=nn.Identity())


def test_gemmp_state_dict_has_no_p_but_moves_with_the_module():
    from cirtorch.layers.pooling import GeMmp
    m = GeMmp(p=3, mp=8)
    assert list(m.state_dict()) == []
    assert dict(m.named_buffers()).keys() == {"p"}
    m.load_state_dict({})  # the reference checkpoint schema: no key
    assert m.double().p.dtype == torch.float64  # buffers follow .to() / .cuda()


def test_regional_head_state_keys():
    from cirtorch.layers.pooling import GeM, GeMmp, SPoC
    from cirtorch.modules.heads.global_head import globalHead
    normal = {"name": "L2N", "params": {}}
    head = globalHead(pooling={"name": "ROIpool", "params": {"rpool": GeM(), "whiten": nn.Linear(24, 24), "L": 3}},
                      normal=normal, dim=24)
    assert set(head.state_dict()) == {"whiten.weight", "whiten.bias", "pool.rpool.p", "pool.whiten.weight",
                                      "pool.whiten.bias"}
    assert [n for n, _ in head.pool.named_children()] == ["rpool", "whiten", "norm"]
    head = globalHead(pooling={"name": "ROIpool", "params": {"rpool": SPoC(), "whiten": None}}, normal=normal, dim=24)
    assert set(head.state_dict()) == {"whiten.weight", "whiten.bias"}
    head = globalHead(pooling={"name": "ROIpool", "params": {"rpool": GeMmp(mp=24)}}, normal=normal, dim=24)
    assert set(head.state_dict()) == {"whiten.weight", "whiten.bias"}
    head = globalHead(pooling={"name": "GeMmp", "params": {"p": 3, "eps": 1e-6}}, normal=normal, dim=24)
    assert head.pool.mp == 24 and set(head.state_dict()) == {"whiten.weight", "whiten.bias"}


def test_init_network_regional_flags():
    from cirtorch.layers.pooling import GeM, MAC, Rpool
    from cirtorch.models.GF_net import init_network, make_net
    net = init_network({"architecture": "resnet18", "pooling": "gem", "regional": True, "whitening": True})
    assert net.meta["regional"] is True and net.meta["local_whitening"] is False
    assert isinstance(net.pool, Rpool) and isinstance(net.pool.rpool, GeM) and net.pool.L == 3
    assert isinstance(net.pool.whiten, nn.Linear) and net.pool.whiten.in_features == 512
    assert {"pool.rpool.p", "pool.whiten.weight", "pool.whiten.bias"} <= set(net.ret_head.state_dict())
    assert "regional: True" in net.meta_repr()
    net = make_net("resnet18", pooling="mac", regional=True, regional_whitening=False, L=2)
    assert isinstance(net.pool.rpool, MAC) and net.pool.whiten is None and net.pool.L == 2
    assert init_network({"architecture": "resnet18"}).meta["regional"] is False
    with pytest.raises(NotImplementedError, match="local_whitening"):
        init_network({"architecture": "resnet18", "local_whitening": True})
    with pytest.raises(NotImplementedError, match="local_whitening"):
        init_network({"architecture": "resnet18", "local_whitening": True, "regional": True})


def test_regional_ops_refuse_cpu_tensors():
    from cirtorch.layers.pooling import GeM, Rpool
    with pytest.raises(RuntimeError, match="GPU"):
        Rpool(GeM())(torch.rand(1, 8, 5, 5))


# ----------------------------------------------------------------------------- C ABI argument checks
@pytest.fixture()
def lib():
    if not os.path.exists(LIB):
        pytest.skip("librr.so not built (run __graft_entry__.build())")
    from cirtorch import _engine
    return _engine.lib()


def _regions(*rects):
    from cirtorch import _engine as E
    return (E.Region * len(rects))(*[E.Region(*r) for r in rects])


# never dereferenced: every call below fails validation before any launch
X = ctypes.c_void_p(0x10000)
OUT = ctypes.c_void_p(0x20000)
PDEV = ctypes.c_void_p(0x30000)


def _pool(lib, x=X, n=1, h=5, w=9, c=8, regions=None, R=None, mode=0, p=3.0, p_dev=None, p_count=0, out=OUT,
          dtype=0):
    regions = regions if regions is not None else _regions((0, 0, 5, 9))
    R = len(regions) if R is None else R
    return lib.rr_region_pool(x, n, h, w, c, regions, R, mode, p, p_dev, p_count, 1e-6, out, dtype, None)


@pytest.mark.parametrize("kwargs,message", [
    (dict(n=0), b"empty"),
    (dict(c=0), b"empty"),
    (dict(R=0), b"empty"),
    (dict(x=None), b"empty"),
    (dict(mode=3), b"mode"),
    (dict(mode=-1), b"mode"),
    (dict(dtype=3), b"dtype"),
    (dict(c=6), b"c % 4"),
    (dict(regions=((0, 0, 6, 9),)), b"region 0"),
    (dict(regions=((0, 0, 5, 9), (1, 1, 4, 9))), b"region 1"),
    (dict(regions=((0, 0, 5, 9), (2, 2, 0, 3))), b"region 1"),
    (dict(p=0.0), b"p must be > 0"),
    (dict(p=-1.0), b"p must be > 0"),
    (dict(p=float("nan")), b"p must be > 0"),
    (dict(p_count=2, p_dev=PDEV), b"p_count"),
    (dict(p_count=-1, p_dev=PDEV), b"p_count"),
    (dict(p_count=1, p_dev=None), b"p_dev"),
    (dict(p_count=8, p_dev=None), b"p_dev"),
])
def test_region_pool_rejects_bad_arguments(lib, kwargs, message):
    if "regions" in kwargs:
        kwargs = dict(kwargs, regions=_regions(*kwargs["regions"]))
    rc = _pool(lib, **kwargs)
    err = lib.rr_last_error()
    assert rc != 0 and b"rr_region_pool" in err and message in err, err


def test_region_pool_p_is_only_checked_for_gem(lib):
    # MAC / SPoC ignore p: a bad region is what gets reported
    rc = _pool(lib, mode=1, p=0.0, regions=_regions((0, 0, 9, 9)))
    assert rc != 0 and b"region 0" in lib.rr_last_error()


@pytest.mark.parametrize("args,message", [
    ((None, 1, 3, 8, 0, 1e-6, OUT, None), b"empty"),
    ((X, 0, 3, 8, 0, 1e-6, OUT, None), b"empty"),
    ((X, 1, 0, 8, 1, 1e-6, OUT, None), b"empty"),
    ((X, 1, 3, 0, 1, 1e-6, OUT, None), b"empty"),
    ((X, 1, 3, 8, 0, 1e-6, None, None), b"empty"),
    ((X, 1, 1025, 8, 0, 1e-6, OUT, None), b"1024"),
])
def test_region_aggregate_rejects_bad_arguments(lib, args, message):
    rc = lib.rr_region_aggregate(*args)
    err = lib.rr_last_error()
    assert rc != 0 and b"rr_region_aggregate" in err and message in err, err
