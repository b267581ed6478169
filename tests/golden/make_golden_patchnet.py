"""Generate tests/golden/patchnet.npz (build container only, like make_golden_pose.py).

    python tests/golden/make_golden_patchnet.py

From the reference, unmodified, each module loaded from its file: cirtorch/features/hardnet.py (HardNet) and
cirtorch/features/sosnet.py (SOSNet), in eval mode and float64 on the CPU, with the seeded state dicts
of tests/patchnet_cases.py loaded with strict=True (data, not code).  No reference source is copied and
no weight is stored: the fixture holds seeds, input checksums, the two modules' state-dict key lists,
the expected descriptors (float32), the float64 layer-6 map of patchnet_cases.MAP_PATCHES, and
tolerances; inputs are rebuilt from the seeds.

Tolerances are measured here.  Per variant the descriptor tolerance is 4 x the largest absolute
difference between the quantised restatement (patchnet_cases.quantised_net: fp16 at the rounding points
of include/rr.h, float64 elsewhere) and the float64 reference: a factor of 2 covers the quantisation
error plus the float32 accumulation of the kernels (which moves a few fp16 roundings by one ulp), the
rest is room for the MFMA's summation order.  The map tolerance is made the same way, relative to the
largest entry of the reference map.

Conditions (asserted): the restatement of SOSNet's LocalResponseNorm as v / |v| agrees with the module
to 1e-12; every descriptor of the restatement has cosine >= 1 - 1e-4 with the reference's; the reference
in float32 agrees with itself in float64 to 1e-5.

Arrays, per variant v in (hardnet, sosnet): <v>_seed, <v>_chk (weights), <v>_keys, <v>_desc [129, 128]
float32, <v>_map [3, 8, 8, 128] float64, <v>_tol (descriptor, map), <v>_other_desc (the weights of
OTHER_SEED, patches 0 .. 7); patch_seed, patch_chk.
"""

import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the reference tree
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("RR_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REF)   # the reference's cirtorch package, not this repository's

import importlib.util  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import patchnet_cases as NC  # noqa: E402


def _load(name):
    """one reference module by file, without importing the rest of the reference's features package"""
    path = os.path.join(REF, "cirtorch", "features", name + ".py")
    spec = importlib.util.spec_from_file_location("ref_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert os.path.abspath(mod.__file__).startswith(os.path.abspath(REF)), mod.__file__
    return mod


REF_CLASS = {"hardnet": _load("hardnet").HardNet, "sosnet": _load("sosnet").SOSNet}


def ref_module(variant, params, dtype=torch.float64):
    net = REF_CLASS[variant](pretrained=False)
    sd = {k: torch.from_numpy(np.asarray(a)) for k, a in NC.state_dict(variant, params).items()}
    net.load_state_dict(sd, strict=True)
    return net.to(dtype).eval()


def ref_run(variant, net, x):
    """-> descriptors [B, 128], the layer-6 map [B, 8, 8, 128] (after its ReLU)"""
    with torch.no_grad():
        t = torch.from_numpy(x)[:, None].to(net_dtype(net))
        desc = net(t)
        if variant == "hardnet":
            fmap = net.features[:18](net._normalize_input(t))
        else:
            fmap = net.layers[:19](t)
        return desc.numpy(), fmap.permute(0, 2, 3, 1).contiguous().numpy()


def net_dtype(net):
    return next(p for p in net.parameters()).dtype


def main():
    x = NC.patches()
    out = {"patch_seed": np.int64(NC.PATCH_SEED), "patch_chk": np.float64(NC.checksum([x]))}
    for variant in NC.VARIANTS:
        params = NC.net_params(NC.SEEDS[variant])
        net = ref_module(variant, params)
        ref, ref_map = ref_run(variant, net, x)
        q, q_map = NC.quantised_net(x, params, variant)
        # the output normalisation as rr.h restates it, on the reference's own features
        with torch.no_grad():
            t = torch.from_numpy(x)[:, None].double()
            seq = net.features if variant == "hardnet" else net.layers
            feats = seq(net._normalize_input(t) if variant == "hardnet" else t).reshape(len(x), 128).numpy()
        lrn = np.abs(NC.normalise_output(feats, variant) - ref).max()
        assert lrn <= 1e-12, (variant, lrn)
        ref32 = ref_run(variant, ref_module(variant, params, torch.float32), x)[0]
        d32 = np.abs(ref32.astype(np.float64) - ref).max()
        assert d32 <= 1e-5, (variant, d32)
        diff = np.abs(q - ref).max()
        cos = (q * ref).sum(1) / (np.linalg.norm(q, axis=1) * np.linalg.norm(ref, axis=1))
        assert cos.min() >= 1 - 1e-4, (variant, cos.min())
        mp = list(NC.MAP_PATCHES)
        mdiff = np.abs(q_map[mp] - ref_map[mp]).max() / np.abs(ref_map[mp]).max()
        print("%s: float32 vs float64 %.2e, restated output norm %.2e, quantised vs float64 %.2e (cos >= %.9f), map %.2e rel"
              % (variant, d32, lrn, diff, cos.min(), mdiff))
        keys = list(net.state_dict().keys())
        assert keys == list(NC.state_dict(variant, params).keys())
        other = NC.net_params(NC.OTHER_SEED)
        out.update({
            variant + "_seed": np.int64(NC.SEEDS[variant]),
            variant + "_chk": np.float64(NC.checksum(params[0] + params[1] + params[2])),
            variant + "_keys": np.array(keys),
            variant + "_desc": ref.astype(np.float32),
            variant + "_map": ref_map[mp],
            variant + "_tol": np.array([4.0 * diff, 4.0 * mdiff]),
            variant + "_other_desc": ref_run(variant, ref_module(variant, other), x[:8])[0].astype(np.float32),
        })
    path = os.path.join(HERE, "patchnet.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
