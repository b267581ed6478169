"""Generate tests/golden/stem_bits.npz: SHA-256 digests of the output BYTES of the fused stem
(stem_conv_pool, stem_conv_pool_ragged; every RR_TUNE_STEM mode) on the calls of
tests/stem_bits_cases.py, recorded on an MI355X from a librr.so whose rr_build_info is BUILD below.

    python tests/golden/make_golden_stem_bits.py [OUT.npz]   (needs the GPU and that library; RR_LIB selects it)

The fixture pins the arithmetic of csrc/rr_stem.hip bit for bit, so that a change of its structure
can be told from a change of what it computes (tests/test_gpu_stem_bits.py).  It was recorded from
the commit before the v3 and v4 stem kernels were folded into one kernel frame with two patch
layouts; BUILD is that parent commit's library, not the library of the commit that added this file.

Regeneration.  Only a commit that changes nothing under csrc/ may regenerate this fixture (after
building the library of its parent and setting BUILD to that library's rr_build_info): a commit that
touches the kernels and the fixture together proves nothing.  A deliberate change of the arithmetic
is made in one commit with this test failing on purpose named in it, and the fixture follows in the
next.

Arrays: build (the library's rr_build_info), then per group of stem_bits_cases.groups(), uint8 with
one row per case of stem_bits_cases.cases(group): '<group>_out' (SHA-256 of the output tensor's
bytes), '<group>_in' (SHA-256 of the pixels, conv weights, scale and shift), '<group>_shape' (the
output shape, 4 int64) and '<group>_cases' (the case names, one per line).
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "image-retrieval-for-image-based-localization_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import stem_bits_cases as BC  # noqa: E402

BUILD = "source_digest=fa63fa3ff53a arch=gfx950"


def main():
    from cirtorch import _engine
    if not torch.cuda.is_available():
        raise SystemExit("make_golden_stem_bits needs a GPU")
    build = _engine.lib().rr_build_info().decode()
    assert build == BUILD, "recorded from %r only, this library is %r" % (BUILD, build)
    cuda = torch.device("cuda:0")
    out = {"build": np.frombuffer(build.encode(), dtype=np.uint8)}
    for group in BC.groups():
        first, again = BC.run(group, cuda), BC.run(group, cuda)
        for name, a in first.items():
            assert a.tobytes() == again[name].tobytes(), "%s differs between two runs" % name
            out[name] = a
        print("  %s: %d cases" % (group, len(BC.cases(group))))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "stem_bits.npz")
    np.savez_compressed(path, **out)
    print("  %s: %d arrays, %.0f KB" % (os.path.basename(path), len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
