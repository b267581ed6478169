"""Generate tests/golden/verify_bits.npz: the output BYTES of the pair-geometry entries (verify_pairs
of both models, homography_dlt, fundamental_dlt) on the calls of tests/verify_bits_cases.py, recorded
on an MI355X from a librr.so whose rr_build_info is BUILD below.

    python tests/golden/make_golden_verify_bits.py [OUT.npz]   (needs the GPU and that library; RR_LIB selects it)

The fixture pins the arithmetic of csrc/rr_verify.hip, csrc/rr_epipolar.hip and csrc/rr_ransac.h bit
for bit, so that a change of their structure can be told from a change of what they compute
(tests/test_gpu_verify_bits.py).  It was recorded from the commit before the two verifiers were
folded into one skeleton.

Regeneration.  Only a commit that changes nothing under csrc/ may regenerate this fixture (after
building the library of its parent and setting BUILD to that library's rr_build_info): a commit that
touches the kernels and the fixture together proves nothing.  A deliberate change of the arithmetic
is made in one commit with this test failing on purpose named in it, and the fixture follows in the
next.

Arrays: build (the library's rr_build_info), then '<group>_<array>' uint8 per group of
verify_bits_cases.groups(): inliers (int32 [P]), matrix (float64 [P, 3, 3]), mask (uint8 [rows1]);
matrix and matrix_short for the fits.
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "image-retrieval-for-image-based-localization_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import verify_bits_cases as BC  # noqa: E402

BUILD = "source_digest=4b0cd34c187a arch=gfx950"


def main():
    from cirtorch import _engine
    if not torch.cuda.is_available():
        raise SystemExit("make_golden_verify_bits needs a GPU")
    build = _engine.lib().rr_build_info().decode()
    assert build == BUILD, "recorded from %r only, this library is %r" % (BUILD, build)
    cuda = torch.device("cuda:0")
    out = {"build": np.frombuffer(build.encode(), dtype=np.uint8)}
    for group in BC.groups():
        first, again = BC.run(group, cuda), BC.run(group, cuda)
        for name, a in first.items():
            assert a.tobytes() == again[name].tobytes(), "%s differs between two runs" % name
            out[name] = a
        print("  %s: %s" % (group, ", ".join("%s %d B" % (n, a.size) for n, a in first.items())))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "verify_bits.npz")
    np.savez_compressed(path, **out)
    print("  %s: %d arrays, %.0f KB" % (os.path.basename(path), len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
