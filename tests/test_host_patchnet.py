"""CPU checks of the learned patch descriptors' host side: the new names of cirtorch.features, the new C
entries (in the header, exported, bound), their argument checks (they return before anything is
enqueued, so they run without a GPU), the size key of the tuning table, the Python surface's refusals,
the state-dict layout against the reference's key lists, the patchnet.npz fixture against the numpy
restatement of tests/patchnet_cases.py and the recorded kernel resources."""

import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import patchnet_cases as NC
from conftest import PKG, REPO, golden

HEADER = os.path.join(REPO, "include", "rr.h")
LIB = os.path.join(PKG, "librr.so")
NEW_INT = ("rr_patchnet_pack", "rr_patchnet_trunk", "rr_patchnet_head", "rr_patchnet_describe")
NEW_SIZE = ("rr_patchnet_packed_bytes", "rr_patchnet_workspace_bytes")
P = ctypes.c_void_p(0x1000)   # "non-null, aligned"; never dereferenced
NULL = ctypes.c_void_p(0)
HARD, SOS = 0, 1


def _lib():
    from cirtorch import _engine
    return _engine.lib()


# ---------------------------------------------------------------- the package and the ABI
def test_package_and_names():
    import cirtorch.features as F
    from cirtorch.features import hardnet, sosnet
    assert F.HardNet is hardnet.HardNet and F.SOSNet is sosnet.SOSNet
    assert issubclass(F.HardNet, torch.nn.Module) and issubclass(F.SOSNet, torch.nn.Module)
    assert "liberty_aug" in hardnet.urls and "lib" in sosnet.urls
    # what was there stays
    for name in ("SIFTDescriptor", "LAFOrienter", "extract_patches_simple", "extract_patches_from_pyramid"):
        assert callable(getattr(F, name))
    import inspect
    import cirtorch.search as S
    assert inspect.signature(S.describe_keypoints).parameters["descriptor"].default is None


def test_new_symbols_in_header_exported_and_bound():
    from cirtorch import _engine
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(rr_\w+)\b", out))
    for name in NEW_INT + NEW_SIZE:
        kind = "int" if name in NEW_INT else "size_t"
        assert re.search(r"^\s*%s\s+%s\s*\(" % (kind, name), text, flags=re.M), name
        assert name in exported and name in _engine._SIGS, name
        assert getattr(_engine.lib(), name) is not None
    assert re.search(r"^#define RR_PATCHNET_HARDNET 0$", text, flags=re.M)
    assert re.search(r"^#define RR_PATCHNET_SOSNET 1$", text, flags=re.M)
    assert (_engine.RR_PATCHNET_HARDNET, _engine.RR_PATCHNET_SOSNET) == (0, 1)
    # the header cites the reference lines it replaces and says what is not built
    for cite in ("hardnet.py:12-76", "sosnet.py:9-58", "HardNet8", "AffNet", "OriNet"):
        assert cite in text, cite


def test_packed_and_workspace_sizes():
    from cirtorch import _engine as E
    lib = _lib()
    nw = sum(co * ci * k * k for co, ci, k, _, _ in NC.LAYERS)
    nc = sum(co for co, *_ in NC.LAYERS)
    assert (nw, nc) == (1334560, 576)
    assert lib.rr_patchnet_packed_bytes() == (2 * nw + 255) // 256 * 256 + 8 * nc
    per = 8 * 8 * 128 * 2
    chunk = E.get_tuning("PATCHNET_CHUNK")
    assert chunk == 16384
    for b in (1, 63, chunk, chunk + 1, 10 * chunk):
        assert lib.rr_patchnet_workspace_bytes(b) == 256 + min(b, chunk) * per, b
    assert lib.rr_patchnet_workspace_bytes(0) == 256 + per and lib.rr_patchnet_workspace_bytes(-1) == 0
    with E.tuning(PATCHNET_CHUNK=64):
        assert E.get_tuning(E.RR_TUNE_PATCHNET_CHUNK) == 64 and E.get_tuning("rr_tune_patchnet_chunk") == 64
        assert lib.rr_patchnet_workspace_bytes(129) == 256 + 64 * per
    assert E.get_tuning("PATCHNET_CHUNK") == chunk


def test_size_key_of_the_tuning_table():
    from cirtorch import _engine as E
    text = open(HEADER).read()
    body = re.search(r"enum rr_tune_size_key \{(.*?)\};", text, re.S).group(1)
    keys = {name: int(value) for name, value in re.findall(r"(RR_TUNE_\w+)\s*=\s*(\d+)", body)}
    assert keys == {"RR_TUNE_SIZE_BASE": 32, "RR_TUNE_PATCHNET_CHUNK": 32}
    assert E.TUNE_SIZE_KEYS == {"PATCHNET_CHUNK": 32} and E.RR_TUNE_PATCHNET_CHUNK == 32
    lib, got = _lib(), ctypes.c_int()
    for bad in (0, -5):
        assert lib.rr_set_tuning(32, bad) != 0 and b"rr_set_tuning" in lib.rr_last_error()
    assert lib.rr_get_tuning(32, None) != 0 and b"rr_get_tuning" in lib.rr_last_error()
    assert lib.rr_get_tuning(33, ctypes.byref(got)) != 0 and lib.rr_set_tuning(33, 1) != 0
    assert lib.rr_get_tuning(32, ctypes.byref(got)) == 0 and got.value == 16384


# ---------------------------------------------------------------- argument refusals
def test_argument_checks():
    """every refusal happens on the host: made-up device addresses, nothing is launched"""
    lib = _lib()
    odd = ctypes.c_void_p(0x1004)
    ok7 = (ctypes.c_void_p * 7)(*[0x1000] * 7)
    hole = (ctypes.c_void_p * 7)(*([0x1000] * 3 + [0] + [0x1000] * 3))
    nbytes = lib.rr_patchnet_packed_bytes()

    def pack(w=ok7, m=ok7, v=ok7, packed=P, n=nbytes):
        return lib.rr_patchnet_pack(w, m, v, packed, n, NULL)

    for kw in [dict(w=None), dict(m=None), dict(v=None), dict(packed=NULL), dict(w=hole), dict(m=hole), dict(v=hole),
               dict(packed=odd), dict(n=nbytes - 1), dict(n=0)]:
        assert pack(**kw) != 0, kw
        assert lib.rr_last_error().decode().startswith("rr_patchnet_pack"), kw
    assert pack(n=nbytes - 1) == -3

    def trunk(x=P, B=4, variant=HARD, packed=P, out=P):
        return lib.rr_patchnet_trunk(x, B, variant, packed, out, NULL)

    for kw in [dict(x=NULL), dict(out=NULL), dict(packed=NULL), dict(B=-1), dict(variant=2), dict(variant=-1), dict(x=odd),
               dict(out=odd), dict(packed=odd)]:
        assert trunk(**kw) != 0, kw
        assert lib.rr_last_error().decode().startswith("rr_patchnet_trunk"), kw
    assert trunk(B=0) == 0 and trunk(B=0, x=NULL, out=NULL, variant=SOS) == 0

    def head(m=P, B=4, variant=SOS, packed=P, out=P):
        return lib.rr_patchnet_head(m, B, variant, packed, out, NULL)

    for kw in [dict(m=NULL), dict(out=NULL), dict(packed=NULL), dict(B=-1), dict(variant=2), dict(m=odd)]:
        assert head(**kw) != 0, kw
        assert lib.rr_last_error().decode().startswith("rr_patchnet_head"), kw
    assert head(B=0) == 0 and head(B=0, m=NULL, out=NULL) == 0

    need = lib.rr_patchnet_workspace_bytes(4)

    def desc(x=P, B=4, variant=HARD, packed=P, out=P, ws=P, n=need):
        return lib.rr_patchnet_describe(x, B, variant, packed, out, ws, n, NULL)

    for kw in [dict(x=NULL), dict(out=NULL), dict(packed=NULL), dict(B=-1), dict(variant=7), dict(ws=NULL), dict(n=need - 1),
               dict(n=0), dict(x=odd)]:
        assert desc(**kw) != 0, kw
        assert lib.rr_last_error().decode().startswith("rr_patchnet_describe"), kw
    assert desc(n=need - 1) == -3
    assert desc(B=0) == 0 and desc(B=0, x=NULL, out=NULL, ws=NULL, n=0) == 0


def test_python_refusals():
    from cirtorch.features import HardNet, SOSNet
    from cirtorch.search import describe_keypoints
    for cls, name in ((HardNet, "checkpoint_liberty_with_aug.pth"), (SOSNet, "sosnet_32x32_liberty.pth")):
        with pytest.raises(RuntimeError, match="load_state_dict") as err:
            cls(pretrained=True)
        assert name in str(err.value)
        net = cls(False).eval()
        with pytest.raises(RuntimeError, match="GPU"):
            net(torch.zeros(2, 1, 32, 32))                         # a CPU tensor
        for shape in ((2, 1, 31, 32), (2, 3, 32, 32), (2, 32, 32), (2, 1, 64, 64)):
            with pytest.raises(ValueError, match="Bx1x32x32"):
                net(torch.zeros(shape))
        with pytest.raises(TypeError):
            net(np.zeros((2, 1, 32, 32)))
        assert cls(False).training
        with pytest.raises(NotImplementedError, match="eval"):
            cls(False).describe(torch.zeros(2, 32, 32))            # train() mode, before anything else
        img, kp = torch.zeros(1, 1, 64, 64), torch.zeros(1, 4, 2)
        with pytest.raises(ValueError, match="32 x 32"):
            describe_keypoints(img, kp, patch_size=16, descriptor=net)
        with pytest.raises(RuntimeError, match="GPU"):
            describe_keypoints(img, kp, descriptor=net)
    with pytest.raises(TypeError, match="descriptor"):
        describe_keypoints(torch.zeros(1, 1, 64, 64), torch.zeros(1, 4, 2), descriptor=torch.nn.Identity())
    with pytest.raises(NotImplementedError):
        SOSNet(False).eval()(torch.zeros(1, 1, 32, 32), eps=1e-8)


# ---------------------------------------------------------------- state dicts and the fixture
@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_state_dict_keys_are_the_reference(variant):
    from cirtorch.features import HardNet, SOSNet
    g = golden("patchnet.npz")
    net = (HardNet if variant == "hardnet" else SOSNet)(False)
    keys = [str(k) for k in g[variant + "_keys"]]
    assert list(net.state_dict().keys()) == keys
    params = NC.net_params(NC.SEEDS[variant])
    sd = {k: torch.from_numpy(np.asarray(a)) for k, a in NC.state_dict(variant, params).items()}
    assert list(sd) == keys
    net.load_state_dict(sd, strict=True)
    if variant == "sosnet":
        assert len(list(net.desc_norm.parameters())) == 0 and isinstance(net.desc_norm[0], torch.nn.LocalResponseNorm)


@pytest.mark.parametrize("variant", NC.VARIANTS)
def test_restatement_equals_fixture(variant):
    g = golden("patchnet.npz")
    x = NC.patches()
    assert int(g["patch_seed"]) == NC.PATCH_SEED and float(g["patch_chk"]) == NC.checksum([x])
    params = NC.net_params(NC.SEEDS[variant])
    assert int(g[variant + "_seed"]) == NC.SEEDS[variant]
    assert float(g[variant + "_chk"]) == NC.checksum(params[0] + params[1] + params[2])
    want, tol = g[variant + "_desc"].astype(np.float64), g[variant + "_tol"]
    assert want.shape == (NC.NPATCH, 128) and g[variant + "_map"].shape == (len(NC.MAP_PATCHES), 8, 8, 128)
    # the tolerances are 4 x what the restatement differs by: a few 1e-4, three orders below an indexing fault
    assert 1e-4 < tol[0] < 4e-3 and 1e-4 < tol[1] < 2e-2
    idx = sorted(set(NC.MAP_PATCHES) | set(range(12)))
    q, qmap = NC.quantised_net(x[idx], params, variant)
    assert np.abs(q - want[idx]).max() <= tol[0] / 4 + 1e-7            # 1e-7: the fixture is stored as float32
    cos = (q * want[idx]).sum(1) / (np.linalg.norm(q, axis=1) * np.linalg.norm(want[idx], axis=1))
    assert cos.min() >= 1 - 1e-4
    pos = [idx.index(i) for i in NC.MAP_PATCHES]
    ref_map = g[variant + "_map"]
    assert np.abs(qmap[pos] - ref_map).max() <= tol[1] / 4 * np.abs(ref_map).max() * (1 + 1e-12)


def test_restatement_exact_cases():
    """fresh statistics (mean 0, var 1) on a constant patch: HardNet gives zeros, SOSNet 1 / sqrt(128)"""
    w = NC.net_params(7)[0]
    fresh = (w, [np.zeros(c[0], np.float32) for c in NC.LAYERS], [np.ones(c[0], np.float32) for c in NC.LAYERS])
    x = np.full((1, 32, 32), 0.5, np.float32)
    assert (NC.quantised_net(x, fresh, "hardnet")[0] == 0).all()
    assert np.abs(NC.quantised_net(x, fresh, "sosnet")[0] - 1 / np.sqrt(128)).max() < 1e-15


def test_recorded_kernel_resources():
    """profiles/patchnet_kernel_resources.json: what the compiler reported for the three kernels; no scratch,
    and the trunk's LDS is the figure DESIGN.md states"""
    rec = json.load(open(os.path.join(REPO, "profiles", "patchnet_kernel_resources.json")))
    assert set(rec["kernels"]) == {"k_patchnet_pack", "k_patchnet_trunk", "k_patchnet_head"}
    for name, r in rec["kernels"].items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs"] + r["AGPRs"] <= 256 and r["Occupancy [waves/SIMD]"] >= 1, name
    lds = rec["kernels"]["k_patchnet_trunk"]["LDS Size [bytes/block]"]
    assert lds == 2 * 34 * 34 * 32 * 2 + 64 == 148032 and lds <= 160 * 1024
    assert rec["kernels"]["k_patchnet_head"]["LDS Size [bytes/block]"] == 7 * 32 * 64 * 4   # the partial sums of 7 waves
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "148,032" in design
