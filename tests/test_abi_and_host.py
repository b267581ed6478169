"""CPU checks of the C ABI (library loads, every header symbol exported and
bound) and of the host-side mirror of the reference interface (no GPU
compute calls here)."""

import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, REPO, golden

HEADER = os.path.join(REPO, "include", "rr.h")
LIB = os.path.join(PKG, "librr.so")


def header_symbols():
    text = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:[\w\*\s]+?)\b(rr_\w+)\s*\(", text, flags=re.M)))


def test_library_exports_every_header_symbol():
    if not os.path.exists(LIB):
        pytest.skip("librr.so not built (run __graft_entry__.build())")
    syms = header_symbols()
    assert len(syms) >= 15
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(rr_\w+)\b", out))
    missing = [s for s in syms if s not in exported]
    assert not missing, missing


def test_ctypes_binding_covers_header():
    if not os.path.exists(LIB):
        pytest.skip("librr.so not built")
    from cirtorch import _engine
    lib = _engine.lib()
    assert set(header_symbols()) == set(_engine._SIGS), set(header_symbols()) ^ set(_engine._SIGS)
    assert lib.rr_version() >= 1
    assert lib.rr_knn_workspace_bytes(1000, 4, 512, 10, 0, _engine.RR_F32) > 0


def test_conv_desc_layout_matches_header():
    from cirtorch import _engine
    text = open(HEADER).read()
    body = re.search(r"typedef struct rr_conv_desc \{(.*?)\} rr_conv_desc;", text, re.S).group(1)
    fields = []
    for line in body.splitlines():
        line = line.split("/*")[0].strip().rstrip(";")
        if not line:
            continue
        typ, names = line.split(None, 1)
        fields += [(n.strip(), typ) for n in names.split(",")]
    assert [f[0] for f in fields] == [f[0] for f in _engine.ConvDesc._fields_]


def test_error_path_reports_message():
    if not os.path.exists(LIB):
        pytest.skip("librr.so not built")
    from cirtorch import _engine
    lib = _engine.lib()
    rc = lib.rr_l2n_rows(None, 0, 0, 1e-6, None, None)
    assert rc != 0 and b"rr_l2n_rows" in lib.rr_last_error()


def test_product_refuses_cpu_tensors():
    from cirtorch.layers import functional as LF
    with pytest.raises(RuntimeError, match="GPU"):
        LF.gem(torch.rand(1, 8, 3, 3))
    from cirtorch.models.GF_net import make_net
    net = make_net("resnet18", precision="fp32")
    with pytest.raises(RuntimeError, match="GPU"):
        net.extract([torch.rand(3, 32, 32)])


def test_backbone_state_dict_matches_reference_layout():
    """Our module tree accepts the reference key layout exactly (oracle weights use it)."""
    from cirtorch.backbones import resnet
    from oracle import weights
    for arch in ("resnet18", "resnet50", "resnet101"):
        body = resnet.__dict__[arch]()
        sd = {k: torch.from_numpy(v) for k, v in weights.backbone_state(arch).items()}
        missing, unexpected = body.load_state_dict(sd, strict=False)
        assert not missing and not unexpected, (arch, missing[:3], unexpected[:3])


def test_convert_torchvision_keys():
    from cirtorch.backbones import resnet
    body = resnet.resnet50()
    tv = {}
    for k, v in body.state_dict().items():
        k2 = k.replace("mod1.conv1", "conv1").replace("mod1.bn1", "bn1")
        m = re.match(r"mod(\d)\.block(\d+)\.(.*)", k2)
        if m:
            mod, blk, rest = int(m.group(1)), int(m.group(2)), m.group(3)
            rest = rest.replace("convs.", "").replace("proj_conv", "downsample.0").replace("proj_bn", "downsample.1")
            k2 = "layer%d.%d.%s" % (mod - 1, blk - 1, rest)
        tv[k2] = v
    out = body.convert(tv)
    assert set(out) == {k for k in body.state_dict() if not k.endswith("num_batches_tracked")}


def test_packed_sequence_and_padding():
    from cirtorch.utils.parallel import PackedSequence
    from cirtorch.utils.sequence import pad_packed_images, pack_padded_images
    a, b = torch.rand(3, 5, 7), torch.rand(3, 6, 4)
    ps = PackedSequence([a, b])
    padded, sizes = pad_packed_images(ps)
    assert padded.shape == (2, 3, 6, 7)
    assert torch.equal(padded[0, :, :5, :7], a) and torch.equal(padded[1, :, :6, :4], b)
    assert padded[0, :, 5:].abs().sum() == 0 and padded[1, :, :, 4:].abs().sum() == 0
    back = pack_padded_images(padded, sizes)
    assert torch.equal(back[0], a) and torch.equal(back[1], b)
    with pytest.raises(ValueError):
        pad_packed_images(PackedSequence([torch.rand(3, 4, 4), torch.rand(1, 4, 4)]))
    with pytest.raises(TypeError):
        PackedSequence([a, b.double()])


def test_map_evaluation_host_code_matches_reference_golden():
    from cirtorch.utils.evaluation.ParisOxfordEval import compute_map_and_print
    g = golden("map.npz")
    from test_oracle_golden import _gnd
    gnd = _gnd(g)
    logs = []
    score = compute_map_and_print("roxford5k", g["ranks"].astype(np.int64), gnd, lambda *a: logs.append(a))
    assert score["mAP"] == pytest.approx(float(g["score_mAP"]), abs=1e-10)
    assert score["mapE"] == pytest.approx(float(g["mapE"]), abs=1e-12)


def test_upstream_surface_imports():
    """Every name scripts/test.py imports (scripts/test.py:12-18) resolves."""
    from cirtorch.models.GF_net import init_network, extract_vectors  # noqa: F401
    from cirtorch.datasets.datahelpers import cid2filename
    from cirtorch.datasets.testdataset import configdataset  # noqa: F401
    from cirtorch.utils.download import download_train, download_test  # noqa: F401
    from cirtorch.utils.whiten import whitenlearn, whitenapply  # noqa: F401
    from cirtorch.utils.evaluate import compute_map_and_print  # noqa: F401
    from cirtorch.utils.general import get_data_root, htime
    from cirtorch.layers.pooling import GeM, MAC, SPoC  # noqa: F401
    from cirtorch.layers.normalization import L2N  # noqa: F401
    from cirtorch.modules.pools import POOLING_LAYERS
    from cirtorch.modules.normalizations import NORMALIZATION_LAYERS
    assert cid2filename("abcdef123", "/r") == "/r/23/f1/de/abcdef123"
    assert htime(3725) == "1h 2m 5s"
    assert get_data_root().endswith("data")
    assert {"GeM", "MAC", "SPoC"} <= set(POOLING_LAYERS) and "L2N" in NORMALIZATION_LAYERS
    net = init_network({"architecture": "resnet50", "pooling": "gem", "whitening": True,
                        "mean": [0.485, 0.456, 0.406], "std": [0.229, 0.224, 0.225]})
    assert abs(float(net.pool.p.item()) - 3.0) < 1e-7 and "architecture" in net.meta_repr()


def test_whitenlearn_host_matches_reference_golden():
    from cirtorch.utils.whiten import whitenlearn
    from oracle import data
    g = golden("whiten.npz")
    X = data.unit_rows(600, 64, seed=601).T.astype(np.float64)
    m, P = whitenlearn(X, g["qidxs"], g["pidxs"])
    np.testing.assert_allclose(m, g["m"], rtol=1e-12)
    np.testing.assert_allclose(np.abs(P), np.abs(g["P"]), rtol=1e-6, atol=1e-8)


def test_pmc_traffic_profile_matches_bench_defaults():
    """bench.py reports roofline.traffic only when profiles/r02_pmc_traffic.json
    was measured on its default workload; keep the file's config keys in step."""
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    t = json.load(open(os.path.join(root, "profiles", "r02_pmc_traffic.json")))
    c = t["config"]
    assert (c["arch"], c["precision"], c["image"]) == ("resnet50", "bf16", [3, 768, 1024])
    assert c["batch"] == 128 and c.get("source_commit")
    # measured HBM bytes per image near the 808 MB per-layer algorithmic sum (the
    # fused stage boundaries skip re-reads that sum counts: 799 MB at r02j)
    assert 6.0e8 < t["hbm_bytes_per_image"] < 1.2e9


def test_pmc_knn_traffic_profiles_match_bench_defaults():
    """bench.py fills knn.roofline.traffic from profiles/r02_pmc_knn_q<Q>.json
    only for its default database (1M x 2048 bf16, k=100)."""
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for q in (128, 1024):
        t = json.load(open(os.path.join(root, "profiles", "r02_pmc_knn_q%d.json" % q)))
        c = t["config"]
        assert (c["q"], c["db_rows"], c["dim"], c["k"], c["screen"]) == (q, 1000000, 2048, 100, "bf16")
        # at least one pass over the bf16 database (4.096 GB)
        assert 4.0e9 < t["hbm_bytes_per_search"] < 2.0e10


def test_comm_entry_points_validate_arguments():
    """rr_comm_* / rr_topk_allgather_*: argument checks need no GPU (RCCL is
    only dlopen'ed once a communicator is really created)."""
    if not os.path.exists(LIB):
        pytest.skip("librr.so not built")
    import ctypes
    from cirtorch import _engine
    lib = _engine.lib()
    comm = ctypes.c_void_p()
    idbuf = ctypes.create_string_buffer(128)
    assert lib.rr_comm_init(ctypes.byref(comm), 2, idbuf, 128, 2) != 0       # rank >= nranks
    assert b"rank" in lib.rr_last_error()
    assert lib.rr_comm_init(ctypes.byref(comm), 2, idbuf, 64, 0) != 0        # id shorter than ncclUniqueId
    assert lib.rr_comm_unique_id(idbuf, 16) != 0
    assert lib.rr_comm_destroy(None) == 0
    assert lib.rr_topk_allgather_workspace_bytes(8, 1024, 100) >= 2 * 8 * 1024 * 100 * 8
    assert lib.rr_topk_allgather_workspace_bytes(0, 1, 1) == 0
    assert lib.rr_topk_allgather_merge(None, None, None, 1, 1, None, None, None, 0, None) != 0


def test_library_built_from_this_tree():
    """rr_build_info: librr.so records the digest of the kernel sources it was built from
    (tools/src_digest.py, the digest bench.py reports as build.tree_source_digest); the
    library in the tree must be built from the tree's sources (provenance of a prebuilt
    librr.so pushed to a GPU box)."""
    import importlib.util
    from cirtorch import _engine as E
    spec = importlib.util.spec_from_file_location("src_digest", os.path.join(REPO, "tools", "src_digest.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    info = dict(kv.split("=", 1) for kv in E.lib().rr_build_info().decode().split())
    assert info["source_digest"] == m.digest(), info
    # the Makefile's ARCH (gfx950 unless overridden) is recorded, not assumed
    assert info["arch"].startswith("gfx"), info


# ------------------------------------------------------------------ tuning table
TUNE_DEFAULTS = {0: 0, 1: 2, 2: 1, 3: 0, 4: 0, 5: 1, 6: 1, 7: 0, 8: 1, 9: 1, 10: 1, 11: 2, 12: 1, 13: 1, 14: 2,
                 15: 1, 16: 1}
TUNE_BOOL_KEYS = (2, 3, 4, 9)
# (key, value set, value read back): every value a test or tool passes
TUNE_ROUND_TRIPS = (
    [(0, v, v) for v in range(9)] + [(1, 2, 2), (1, 3, 3), (1, 7, 2)] + [(5, v, v) for v in range(4)] +
    [(6, v, v) for v in range(10)] + [(7, v, v) for v in (0, 8, 16)] +
    [(8, v, v) for v in (0, 1, 2, 9, 1 | 16, 1 | 32, 1 | 4 | 64 | 128 | 512)] + [(8, -1, 0)] +
    [(11, v, v) for v in range(7)] + [(13, v, v) for v in range(3)] + [(14, v, v) for v in range(3)] +
    [(k, v, r) for k in TUNE_BOOL_KEYS + (10, 12, 15, 16) for v, r in ((0, 0), (1, 1))] +
    [(k, 5, 1) for k in TUNE_BOOL_KEYS])


def _tuning_in_fresh_process(**env):
    """{key: rr_get_tuning(key)} of a new process whose environment has no RR_* variable but env."""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("RR_")}
    clean.update(env)
    code = ("import ctypes, json, sys; lib = ctypes.CDLL(sys.argv[1]); v = ctypes.c_int(); out = {}\n"
            "for k in range(17):\n"
            "    assert lib.rr_get_tuning(k, ctypes.byref(v)) == 0; out[k] = v.value\n"
            "print(json.dumps(out))")
    out = subprocess.run([sys.executable, "-c", code, LIB], env=clean, capture_output=True, text=True, check=True)
    return {int(k): v for k, v in json.loads(out.stdout).items()}


def test_tuning_key_constants_match_header():
    from cirtorch import _engine as E
    body = re.search(r"enum rr_tune_key \{(.*?)\};", open(HEADER).read(), re.S).group(1)
    keys = {name: int(value) for name, value in re.findall(r"(RR_TUNE_\w+)\s*=\s*(\d+)", body)}
    assert len(keys) == 17 and sorted(keys.values()) == list(range(17))
    assert {"RR_TUNE_" + name: key for key, name in enumerate(E.TUNE_KEYS)} == keys
    assert {name: getattr(E, name) for name in keys} == keys


def test_tuning_defaults_in_fresh_process():
    assert _tuning_in_fresh_process() == TUNE_DEFAULTS


@pytest.mark.parametrize("env,key,value", [("RR_GEMM_STAGES", 1, 3), ("RR_GEMM_WIDE", 2, 0), ("RR_GEMM8", 8, 0),
                                           ("RR_KNN_FUSED", 9, 0)])
def test_tuning_seeded_from_environment(env, key, value):
    assert _tuning_in_fresh_process(**{env: str(value)}) == {**TUNE_DEFAULTS, key: value}


def test_tuning_set_get_round_trip():
    from cirtorch import _engine as E
    lib, got = E.lib(), ctypes.c_int()
    start = {k: E.get_tuning(k) for k in range(17)}
    try:
        for key, value, back in TUNE_ROUND_TRIPS:
            if key == E.RR_TUNE_KNN_FUSED and start[key] == 0:
                continue  # RR_KNN_FUSED=0 in this process's environment pins the key
            assert lib.rr_set_tuning(key, value) == 0, (key, value)
            assert lib.rr_get_tuning(key, ctypes.byref(got)) == 0 and got.value == back, (key, value, got.value)
            assert lib.rr_set_tuning(key, got.value) == 0                      # set(get) changes nothing
            assert lib.rr_get_tuning(key, ctypes.byref(got)) == 0 and got.value == back, (key, value, got.value)
    finally:
        for key, value in start.items():
            lib.rr_set_tuning(key, value)
    assert {k: E.get_tuning(k) for k in range(17)} == start


def test_tuning_errors_name_the_function():
    from cirtorch import _engine as E
    lib, got = E.lib(), ctypes.c_int()
    for key in (-1, 17, 1 << 20):
        assert lib.rr_set_tuning(key, 0) != 0 and b"rr_set_tuning" in lib.rr_last_error()
        assert lib.rr_get_tuning(key, ctypes.byref(got)) != 0 and b"rr_get_tuning" in lib.rr_last_error()
    assert lib.rr_get_tuning(0, None) != 0 and b"rr_get_tuning" in lib.rr_last_error()
    assert lib.rr_set_tuning(E.RR_TUNE_GRID_CUS, -1) != 0 and b"RR_TUNE_GRID_CUS must be >= 0" in lib.rr_last_error()
    with pytest.raises(ValueError, match="unknown tuning key"):
        E.get_tuning("NO_SUCH_KEY")


def test_tuning_context_manager_restores_state():
    from cirtorch import _engine as E
    start = {k: E.get_tuning(k) for k in range(17)}
    with E.tuning(WRES=0, GEMM8=1 | 8, GRID_CUS=16):
        assert (E.get_tuning("WRES"), E.get_tuning("GEMM8"), E.get_tuning("GRID_CUS")) == (0, 9, 16)
        with E.tuning(WRES=1):
            assert E.get_tuning(E.RR_TUNE_WRES) == 1
        assert E.get_tuning("WRES") == 0
    assert {k: E.get_tuning(k) for k in range(17)} == start
    with pytest.raises(KeyError):
        with E.tuning(STEM=5, CONV3X3=0):
            assert (E.get_tuning("STEM"), E.get_tuning("CONV3X3")) == (5, 0)
            raise KeyError("body")
    assert {k: E.get_tuning(k) for k in range(17)} == start
    with pytest.raises(RuntimeError, match="RR_TUNE_GRID_CUS"):  # a refused value: the keys set before it go back
        with E.tuning(STEM=5, GRID_CUS=-1):
            pass
    assert {k: E.get_tuning(k) for k in range(17)} == start


def test_apply_tuning_arg_takes_names_and_numbers():
    from cirtorch import _engine as E
    start = {k: E.get_tuning(k) for k in range(17)}
    try:
        E.apply_tuning_arg("WRES=0,rr_tune_stem=5, 8=0x9,")
        assert (E.get_tuning("WRES"), E.get_tuning("STEM"), E.get_tuning("GEMM8")) == (0, 5, 9)
        E.apply_tuning_arg("")
    finally:
        for key, value in start.items():
            E.set_tuning(key, value)


def test_launch_info_layout_matches_header():
    from cirtorch import _engine as E
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{(.*?)\} rr_launch_info;", text, re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        typ, names = decl.rsplit(None, 1) if "," not in decl else decl.split(None, 1)
        if typ == "char":
            name, size = re.fullmatch(r"(\w+)\[(\d+)\]", names).groups()
            fields.append((name, ctypes.c_char * int(size)))
        else:
            fields += [(n.strip(), {"unsigned": ctypes.c_uint, "int": ctypes.c_int}[typ]) for n in names.split(",")]
    assert fields == list(E.LaunchInfo._fields_)
    assert ctypes.sizeof(E.LaunchInfo) == 32 + 48 + 5 * 4


def test_last_launch_is_thread_local_and_checks_its_argument():
    """Nothing has been recorded on a new thread (RR_EINVAL, the message names the function); a null pointer
    is refused; neither call needs a device."""
    import threading
    from cirtorch import _engine as E
    lib, seen = E.lib(), {}

    def fresh():
        info = E.LaunchInfo()
        seen["rc"] = lib.rr_last_launch(ctypes.byref(info))
        seen["err"] = lib.rr_last_error()
        try:
            E.last_launch()
        except RuntimeError as e:
            seen["raised"] = str(e)

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert seen["rc"] == -1 and b"rr_last_launch" in seen["err"] and "rr_last_launch" in seen["raised"]
    assert lib.rr_last_launch(None) == -1 and b"rr_last_launch: null" in lib.rr_last_error()
