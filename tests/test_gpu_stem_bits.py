"""The fused stem (stem_conv_pool, stem_conv_pool_ragged; every RR_TUNE_STEM mode) returns the BYTES
whose digests tests/golden/stem_bits.npz records (make_golden_stem_bits.py: recorded on an MI355X
from the commit before the v3 and v4 stem kernels were folded into one kernel frame) on the calls of
tests/stem_bits_cases.py.

No tolerance: the SHA-256 of every output tensor is compared.  A stem kernel has one fixed summation
order per mode and a tile walk that does not change what a tile computes, so a result is a pure
function of the inputs and the mode -- whatever the grid; test_stem_conv_pool,
test_stem_pool_before_epilogue_bit_identical and test_stem_v4_space_to_depth check that it is the
right one, this file that it is still the same one, also where a block walks several tiles."""

import numpy as np
import pytest

import stem_bits_cases as BC
from conftest import golden

ARRAYS = ("out", "in", "shape", "cases")


def test_fixture_covers_every_group():
    g = golden("stem_bits.npz")
    assert set(g.files) - {"build"} == {"%s_%s" % (grp, a) for grp in BC.groups() for a in ARRAYS}
    for grp in BC.groups():
        assert g[grp + "_cases"].tobytes() == BC.case_names(grp).tobytes(), grp
        assert all(g["%s_%s" % (grp, a)].shape == (len(BC.cases(grp)), 32) for a in ARRAYS[:3]), grp
    assert bytes(g["build"]).decode().startswith("source_digest=")


@pytest.mark.gpu
@pytest.mark.parametrize("group", BC.groups())
def test_same_bytes_as_recorded(cuda, group):
    g = golden("stem_bits.npz")
    got = BC.run(group, cuda)
    assert sorted(got) == sorted("%s_%s" % (group, a) for a in ARRAYS)
    assert got[group + "_cases"].tobytes() == g[group + "_cases"].tobytes()
    for k, (name, *_) in enumerate(BC.cases(group)):
        assert got[group + "_in"][k].tobytes() == g[group + "_in"][k].tobytes(), \
            "%s: the INPUT bytes differ from the recorded ones (torch's CPU generator, not the kernels)" % name
        shape, want = got[group + "_shape"][k].view(np.int64), g[group + "_shape"][k].view(np.int64)
        assert shape.tolist() == want.tolist(), "%s: output shape %s, recorded %s" % (name, shape, want)
    for k, (name, *_) in enumerate(BC.cases(group)):
        assert got[group + "_out"][k].tobytes() == g[group + "_out"][k].tobytes(), "%s: output bytes differ" % name
