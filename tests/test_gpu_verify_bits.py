"""The pair-geometry entries (verify_pairs of both models, homography_dlt, fundamental_dlt) return
the BYTES recorded in tests/golden/verify_bits.npz (make_golden_verify_bits.py: recorded on an
MI355X from the commit before the homography and fundamental-matrix verifiers were folded into the
one RANSAC skeleton of csrc/rr_ransac.h) on the calls of tests/verify_bits_cases.py.

No tolerance: inlier counts, 3 x 3 matrices and masks are compared byte for byte.  The kernels have
one fixed summation order, explicit fma where a routine is shared and a block size that does not
depend on the launch, so a result is a pure function of the inputs; test_gpu_verify.py and
test_gpu_epipolar.py check that it is the right one, this file that it is still the same one."""

import numpy as np
import pytest

import verify_bits_cases as BC
from conftest import golden

def test_fixture_covers_every_group():
    g = golden("verify_bits.npz")
    names = set(g.files) - {"build"}
    assert names and all(any(n.startswith(grp + "_") for n in names) for grp in BC.groups())
    assert all(any(n.startswith(grp + "_") for grp in BC.groups()) for n in names)
    assert bytes(g["build"]).decode().startswith("source_digest=")


@pytest.mark.gpu
@pytest.mark.parametrize("group", BC.groups())
def test_same_bytes_as_recorded(cuda, group):
    g = golden("verify_bits.npz")
    got = BC.run(group, cuda)
    want = [n for n in g.files if n.startswith(group + "_") and n[len(group) + 1:] in ("inliers", "matrix", "mask", "matrix_short")]
    assert sorted(got) == sorted(want)
    for name, a in got.items():
        w = g[name]
        if name.endswith(("matrix", "matrix_short")) and a.tobytes() != w.tobytes():
            print(name, "got", a.view(np.float64), "recorded", w.view(np.float64))
        assert a.dtype == np.uint8 and a.size == w.size and a.tobytes() == w.tobytes(), name
