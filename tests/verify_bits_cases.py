"""Shared by tests/golden/make_golden_verify_bits.py and tests/test_gpu_verify_bits.py: the calls
whose output bytes tests/golden/verify_bits.npz pins.  Every RANSAC case of verify_cases.py
(homography) and epipolar_cases.py (fundamental) through cirtorch._ops.verify_pairs, every point set
of DLT_CASES / FUND_CASES through homography_dlt / fundamental_dlt, and per model the ragged case
with a max_n1 below the length of two of its pairs -- each with its module's seed, threshold and
iterations.  Between them: m = 0, SAMPLE - 1, SAMPLE and FIT_MIN records, 257 (a second block-stride
trip), 1025 (past the LDS stage), iters 1 and 257 (a second, partial chunk), refine 0 and 2, an
all-outlier pair, a ragged batch with an empty pair, zero-weight rows and point sets below FIT_MIN.

groups() names the calls; run(group, cuda) -> {array name: uint8 array of the output's bytes}."""

import numpy as np
import torch

import epipolar_cases as EC
import verify_cases as VC
from conftest import golden

MAX_N1 = 45     # ragged4 has side-1 lengths 0, 30, 80, 60: two pairs are cut
MODELS = {"homography": ("v", VC, "verify.npz", "v_seeds", VC.VERIFY_CASES),
          "fundamental": ("e", EC, "epipolar.npz", "e_seeds", EC.EPI_CASES)}


def groups():
    out = []
    for model, (tag, _, _, _, cases) in MODELS.items():
        out += ["%s%d" % (tag, k) for k in range(len(cases))] + ["%s_maxn1" % tag]
    return out + ["dlt%d" % k for k in range(len(VC.DLT_CASES))] + ["fund%d" % k for k in range(len(EC.FUND_CASES))]


def raw(t):
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype=np.uint8)


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def run_pairs(model, k, cuda, max_n1=None):
    from cirtorch import _ops
    _, mod, npz, seeds, cases = MODELS[model]
    case = cases[k]
    kp1, off1, kp2, off2, match, _ = mod.build_case(case, int(golden(npz)[seeds][k]))
    inl, M, mask = _ops.verify_pairs(dev(kp1, cuda), dev(off1, cuda), dev(kp2, cuda), dev(off2, cuda), dev(match, cuda),
                                     mod.TH, case["iters"], case["refine"], mod.RUN_SEED, max_n1, model=model)
    return {"inliers": raw(inl), "matrix": raw(M), "mask": raw(mask)}


def run_fit(model, k, cuda):
    from cirtorch import _ops
    if model == "homography":
        b, n, weighted = VC.DLT_CASES[k]
        p1, p2, w = VC.dlt_points(b, n, weighted, int(golden("verify.npz")["dlt_seeds"][k]))
        fit = _ops.homography_dlt
    else:
        b, n, weighted = EC.FUND_CASES[k]
        p1, p2, w = EC.fund_points(b, n, weighted, int(golden("epipolar.npz")["fund_seeds"][k]))
        fit = _ops.fundamental_dlt
    off = dev(np.arange(b + 1, dtype=np.int64) * n, cuda)
    out = {"matrix": raw(fit(dev(p1.reshape(-1, 2), cuda), dev(p2.reshape(-1, 2), cuda),
                             None if w is None else dev(w.reshape(-1), cuda), off))}
    if n > 5:   # the same rows cut into sets of 3 (below both FIT_MIN), 0, at most 7 and the rest
        off2 = dev(np.array([0, 3, 3, min(b * n, 10), b * n], dtype=np.int64), cuda)
        out["matrix_short"] = raw(fit(dev(p1.reshape(-1, 2), cuda), dev(p2.reshape(-1, 2), cuda),
                                      None if w is None else dev(w.reshape(-1), cuda), off2))
    return out


def run(group, cuda):
    """the outputs of one group, keyed '<group>_<array>'"""
    if group.startswith("dlt"):
        out = run_fit("homography", int(group[3:]), cuda)
    elif group.startswith("fund"):
        out = run_fit("fundamental", int(group[4:]), cuda)
    else:
        model = "homography" if group[0] == "v" else "fundamental"
        if group.endswith("_maxn1"):
            k = [c["name"] for c in MODELS[model][4]].index("ragged4")
            out = run_pairs(model, k, cuda, MAX_N1)
        else:
            out = run_pairs(model, int(group[1:]), cuda)
    return {"%s_%s" % (group, name): a for name, a in out.items()}
