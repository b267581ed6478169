"""Generate tests/golden/patchnet_edges.npz (build container only, like make_golden_patchnet.py).

    python tests/golden/make_golden_patchnet_edges.py

The method of make_golden_patchnet.py: the reference's HardNet and SOSNet modules, unmodified and loaded by
file, in eval mode and float64 on the CPU, with the seeded state dicts of tests/patchnet_cases.py.  The
inputs are patchnet_cases.edge_patches(): patches on which one constant of the input normalisation decides
the descriptor at order 1.  No reference source and no weight is stored; inputs are rebuilt from the seed.

Per variant and group the tolerance is 4 x the largest absolute difference between the quantised
restatement (patchnet_cases.quantised_net) and the float64 reference, the rule of patchnet.npz.

Discrimination (asserted here, and again by tests/test_host_patchnet_edges.py): for every pair of
patchnet_cases.EDGE_PINS[group] the restatement rerun with that constant altered
(patchnet_cases.normalise_input_altered) misses the reference by more than 10 x the group's tolerance.
The table of every (group, variant, alteration) ratio is printed, so what a group does not pin shows too.

Also stored: f32_tol, per variant 4 x the largest difference of the two restatements (float64 and float32
accumulation, quantised_net and quantised_net_f32) over the 129 patches of patchnet_cases.patches(), the
bound of the GPU test on those patches against quantised_net; and nonfinite, whether the reference's
descriptor of each non-finite patch of patchnet_cases.nonfinite_batch() is all NaN.

Arrays: edge_seed, per group g <g>_chk (the input), per variant v and group g <v>_<g>_desc [n, 128] float32
and <v>_<g>_tol, <v>_f32_tol, <v>_nonfinite [4] bool.
"""

import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the reference tree
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden_patchnet as MG  # noqa: E402  (puts tests/ and the reference on the path, loads the two modules)
import patchnet_cases as NC  # noqa: E402


def main():
    edges = NC.edge_patches()
    out = {"edge_seed": np.int64(NC.EDGE_SEED)}
    for g, x in edges.items():
        out[g + "_chk"] = np.float64(NC.checksum([x]))
    x129 = NC.patches()
    bad, where = NC.nonfinite_batch()
    for variant in NC.VARIANTS:
        params = NC.net_params(NC.SEEDS[variant])
        net = MG.ref_module(variant, params)
        for g, x in edges.items():
            ref = MG.ref_run(variant, net, x)[0]
            assert np.isfinite(ref).all(), (variant, g)
            q = NC.quantised_net(x, params, variant)[0]
            tol = 4.0 * np.abs(q - ref).max()
            line = []
            for how in NC.ALTERATIONS:
                miss = np.abs(NC.quantised_net_altered(x, params, variant, how) - ref)
                ratio = np.where(np.isfinite(miss), miss, np.inf).max() / tol
                line.append("%s %.3g" % (how, ratio))
                if (variant, how) in NC.EDGE_PINS[g]:
                    assert ratio > 10.0, (variant, g, how, ratio)
            print("%s %-8s tol %.3e; altered / tol: %s" % (variant, g, tol, ", ".join(line)))
            out["%s_%s_desc" % (variant, g)] = ref.astype(np.float32)
            out["%s_%s_tol" % (variant, g)] = np.float64(tol)
        d = np.abs(NC.quantised_net(x129, params, variant)[0] - NC.quantised_net_f32(x129, params, variant)[0]).max()
        print("%s: float64 vs float32 restatement over %d patches %.3e" % (variant, len(x129), d))
        out[variant + "_f32_tol"] = np.float64(4.0 * d)
        with torch.no_grad():
            ref_bad = MG.ref_run(variant, net, bad[where])[0]
        out[variant + "_nonfinite"] = np.isnan(ref_bad).all(axis=1)
        print("%s: reference descriptor all NaN on the non-finite patches: %s" % (variant, out[variant + "_nonfinite"]))
    path = os.path.join(HERE, "patchnet_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
