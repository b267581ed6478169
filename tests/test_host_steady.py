"""What tests/test_gpu_steady.py rests on, checked without a GPU (tests/steady_cases.py): that every row of
the case tables reaches the state it is there for -- a ring wrapped more than twice and left on a tail, a
register rotation past 2 D strips with a remainder, three or more tiles through the 3x3 tile pipeline, every
tile count from 1 to 7 through k_c3pair's two-tile unroll -- by the launch arithmetic restated from the
launchers, and that the element-wise bound holds for a float32 evaluation of every case, so the float64
reference alone never comes near it.

Conditions on "some block" or "some wave" are taken over the caps of a row (a row is one conv with its caps);
the per-cap numbers are pinned as well."""

import pytest
import torch

import steady_cases as SC

DTYPES = [torch.bfloat16, torch.float16]


def wraps(counts, depth):
    """some worker runs the ring or rotation more than twice round, and some worker ends on a tail"""
    return max(counts) >= 2 * depth + 1 and any(c % depth for c in counts)


def union(plans):
    return sorted({c for p in plans for c in p.counts})


# ---------------------------------------------------------------- k_wres1x1
WRES_EXPECT = {  # (c_in, c_out, residual, cap) -> (grid, xmap, counts)
    (512, 2048, True, 8): (8, 0, [137]), (512, 2048, True, 24): (24, 0, [45, 46]), (512, 2048, True, 64): (64, 1, [17, 18]),
    (256, 1024, True, 8): (8, 0, [34, 35]), (256, 1024, True, 16): (16, 1, [17, 18]),
    (128, 512, True, 8): (8, 0, [17, 18]), (512, 256, False, 8): (8, 0, [17, 18]),
    (512, 1024, False, 8): (8, 0, [67]), (512, 1024, False, 32): (32, 1, [16, 17]),
    (512, 2048, False, 64): (64, 1, [17, 18]), (256, 512, False, 8): (8, 0, [16, 17]),
    (256, 1024, False, 8): (8, 0, [34, 35]), (256, 1024, False, 16): (16, 1, [17, 18]),
}


def wres_plans(row):
    k, c, res, _, stride, shape, caps = row
    return [SC.wres_plan(SC.pixels(shape, stride), c, 8 * SC.wres_cw(k), cap) for cap in caps]


def test_wres_rows_wrap_the_ring():
    assert {(r[0], r[1], r[2], cap) for r in SC.WRES_ROWS for cap in r[6]} == set(WRES_EXPECT)
    for row in SC.WRES_ROWS:
        k, c, res, _, stride, shape, caps = row
        for cap, plan in zip(caps, wres_plans(row)):
            assert (plan.grid, plan.xmap, plan.counts) == WRES_EXPECT[(k, c, res, cap)], (row, cap, plan)
            assert plan.grid == plan.G * plan.nslices and plan.nslices == c // (8 * SC.wres_cw(k))
        for ring in (1, 0):
            nbuf = SC.wres_nbuf(k, res, ring)
            assert nbuf == (3 if res or not ring else {256: 6, 512: 4}[k])
            assert wraps(union(wres_plans(row)), nbuf), (row, ring)
        assert SC.pixels(shape, stride) >= 4096 and SC.pixels(shape, stride) % 32      # the stores of the last tile are masked
    plans = [p for row in SC.WRES_ROWS for p in wres_plans(row)]
    assert {p.xmap for p in plans} == {0, 1} and any(len(p.counts) > 1 for p in plans)
    assert {SC.wres_nbuf(r[0], r[2], 1) for r in SC.WRES_ROWS} == {3, 4, 6}
    assert {r[3] for r in SC.WRES_ROWS} == {True, False} and {r[4] for r in SC.WRES_ROWS} == {1, 2}


def test_wres_cases_of_the_kernel_tests_never_wrap_the_ring():
    """the reason this file exists: at 256 CUs no non-residual WRES_CASES shape of test_gpu_kernels.py gives a block
    more than 3 tiles, fewer than the 4 or 6 buffers of its ring"""
    from test_gpu_kernels import WRES_CASES
    seen = 0
    for n, cin, h, w, cout, k, s, p, res, _ in WRES_CASES:
        if res:
            continue
        plan = SC.wres_plan(SC.pixels((n, h, w), s), cout, 8 * SC.wres_cw(cin), 256)
        assert max(plan.counts) <= 3 < SC.wres_nbuf(cin, False, 1), (cin, cout, plan)
        seen += 1
    assert seen == 4


# ---------------------------------------------------------------- k_stream1x1
STREAM_EXPECT = {  # (c_in, c_out, residual, pixels, cap) -> (nslices, xmap, counts)
    (64, 64, False, 8710, 1): (1, 0, [17, 18]), (64, 256, True, 4355, 1): (1, 0, [17, 18]),
    (64, 256, False, 4355, 1): (1, 0, [17, 18]), (256, 64, False, 4355, 1): (1, 0, [17, 18]),
    (256, 128, False, 4355, 1): (1, 0, [17, 18]), (128, 512, False, 4355, 1): (2, 0, [34, 35]),
    (128, 512, False, 8710, 8): (2, 1, [8, 9]), (512, 128, False, 4355, 1): (1, 0, [34, 35]),
    (512, 2048, True, 4355, 16): (16, 0, [34, 35]), (512, 2048, True, 4355, 128): (16, 1, [4, 5]),
    (256, 1024, True, 4355, 4): (4, 0, [34, 35]), (256, 1024, True, 4355, 32): (4, 1, [4, 5]),
    (256, 512, False, 4284, 2): (2, 0, [33, 34]), (256, 512, False, 4284, 16): (2, 1, [4, 5]),
    (512, 256, False, 4355, 1): (2, 0, [34, 35]), (512, 1024, False, 4355, 1): (8, 0, [34, 35]),
}


def stream_plans(row):
    k, c, _, _, stride, shape, caps, _ = row
    return [SC.stream_plan(SC.pixels(shape, stride), *SC.stream_variant(k, c), c, cap) for cap in caps]


def test_stream_rows_rotate_past_the_depth():
    assert {(r[0], r[1], r[2], SC.pixels(r[5], r[4]), cap) for r in SC.STREAM_ROWS for cap in r[6]} == set(STREAM_EXPECT)
    for row in SC.STREAM_ROWS:
        k, c, res, _, stride, shape, caps, wres = row
        tc, kk, fn, d, nw = SC.stream_variant(k, c)
        assert kk == k and c % tc == 0
        for cap, plan in zip(caps, stream_plans(row)):
            assert (plan.nslices, plan.xmap, plan.counts) == STREAM_EXPECT[(k, c, res, SC.pixels(shape, stride), cap)], (row, cap, plan)
        assert wraps(union(stream_plans(row)), d), row
        assert SC.pixels(shape, stride) >= 4096 and SC.pixels(shape, stride) % (16 * fn)
        # k_wres1x1 must not take the shape (rr_stream.hip:997-1006): WRES = 0, or 1 for a plain form (only WRES = 2 gives it those)
        assert wres == 0 or (wres == 1 and not res), row
    plans = [p for row in SC.STREAM_ROWS for p in stream_plans(row)]
    assert {p.xmap for p in plans} == {0, 1} and any(len(p.counts) > 1 for p in plans)
    assert {SC.stream_variant(r[0], r[1])[3] for r in SC.STREAM_ROWS} == {2, 3, 4}


# ---------------------------------------------------------------- the 1x1 boundaries
def test_pair_rows_rotate_and_wrap():
    p = SC.pixels(SC.MAP_P)
    assert p == 851 and p % 64 and p % 32 and p % 16
    plans = [SC.pair_plan(p, cap) for cap in SC.PAIR_CAPS]
    assert [pl.counts for pl in plans] == [[6, 7], [3, 4]] and [pl.grid for pl in plans] == [1, 2]
    assert wraps(union(plans), 2)                                           # D = 2
    assert set(SC.PAIR_ROWS) == {(c1, pj) for c1 in (64, 128) for pj in (False, True)}
    ring = [SC.mid_plan(p, cap, 32) for cap in SC.MID_CAPS[1]]
    assert [pl.counts for pl in ring] == [[27], [13, 14], [9]]
    assert all(wraps(pl.counts, 4) for pl in ring)                          # the 4-slot residual ring, at every cap
    assert all(wraps(pl.counts, 2) for pl in ring)                          # ... and the two x buffers
    mid = [SC.mid_plan(p, cap, 64) for cap in SC.MID_CAPS[0]]
    assert [pl.counts for pl in mid] == [[14], [4, 5]] and wraps(union(mid), 2)
    assert any(len(pl.counts) > 1 for pl in ring) and any(len(pl.counts) > 1 for pl in mid)


# ---------------------------------------------------------------- k_c3pair
def test_c3pair_rows_cover_one_to_seven_tiles():
    expect = {(1, 4, 32): (1, [1]), (1, 36, 32): (9, [1, 2]), (1, 52, 32): (13, [1, 2]), (2, 28, 64): (28, [3, 4]),
              (5, 12, 64): (30, [3, 4]), (3, 20, 96): (45, [5, 6]), (3, 36, 64): (54, [6, 7])}
    covered, forms_seen = set(), set()
    for shape, forms in SC.C3PAIR_ROWS:
        n, h, w = shape
        assert h % 4 == 0 and w % 32 == 0 and len(forms) >= 2 and set(forms) <= set(SC.C3PAIR_FORMS)
        forms_seen |= set(forms)
        ntiles = n * (h // 4) * (w // 32)
        static, dynamic = SC.c3pair_plan(n, h, w, 8)
        assert (ntiles, static.counts) == expect[shape] and dynamic.counts == static.counts and static.grid == 8
        covered |= set(static.counts)
        if ntiles >= 16:
            s16, d16 = SC.c3pair_plan(n, h, w, 16)
            assert s16.grid == 16 and sum(d16.counts) >= 2 and max(s16.counts) >= 2
    assert covered == set(range(1, 8))
    assert forms_seen == set(SC.C3PAIR_FORMS)
    assert SC.c3pair_plan(1, 4, 32, 8)[0].counts == [1]                     # seven blocks idle


# ---------------------------------------------------------------- direct 3x3
def c3_row_plans(row):
    (n, cin, h, w, cout), _, runs = row
    out = []
    for mode, cap in runs:
        kernel, v = SC.c3_variant(cin, cout, h, mode, cap, n, w)
        out.append((mode, cap, kernel, v, SC.c3w64_plan(n, h, w, cap) if v is None else SC.c3_plan(n, h, w, cout, *v[:3], cap)))
    return out


def test_c3_rows_run_three_tiles_per_block():
    expect = {((3, 64, 24, 96, 64), 9): [3, 4], ((3, 64, 24, 96, 64), 4): [3, 4], ((3, 64, 24, 96, 64), 6): [3, 4],
              ((3, 64, 24, 96, 64), 2): [3, 4], ((3, 64, 24, 96, 128), 2): [3, 4], ((3, 64, 24, 96, 128), 3): [6, 7],
              ((3, 64, 24, 96, 128), 7): [3, 4], ((2, 128, 24, 64, 128), 2): [3], ((2, 128, 24, 64, 128), 3): [6],
              ((2, 128, 24, 64, 128), 7): [3], ((2, 256, 24, 64, 256), 8): [4], ((2, 256, 24, 64, 256), 2): [6],
              ((2, 256, 24, 64, 256), 3): [12], ((1, 512, 24, 32, 512), 8): [4], ((1, 512, 24, 32, 512), 3): [6]}
    kernels, variants, unequal = set(), set(), False
    for row in SC.C3_ROWS:
        for mode, cap, kernel, v, plan in c3_row_plans(row):
            assert plan.counts == expect[(row[0], mode)], (row, mode, plan)
            assert min(plan.counts) >= 3 and plan.grid == cap
            kernels.add(kernel)
            variants.add(v)
            unequal |= len(plan.counts) > 1
    assert kernels == {"k_conv3x3", "k_c3w64"} and unequal
    assert {(256, 6, 32, 4, 2, 2), (128, 8, 32, 2, 4, 3), (128, 4, 32, 2, 4, 2), (64, 8, 32, 1, 8, 2)} <= variants


# ---------------------------------------------------------------- the bound holds for a float32 evaluation
def inside(got, ref, pre, ktot, dt, what):
    worst, i = SC.excess(got.float(), ref, pre, ktot, dt)
    assert torch.isfinite(got.float()).all() and worst <= 1.0, (what, worst, i)
    return worst


def conv_rows():
    for k, c, res, leaky, stride, shape, _ in SC.WRES_ROWS:
        yield k, c, 1, shape, stride, res, leaky
    for k, c, res, leaky, stride, shape, _, _ in SC.STREAM_ROWS:
        yield k, c, 1, shape, stride, res, leaky
    for (n, cin, h, w, cout), leaky, _ in SC.C3_ROWS:
        yield cin, cout, 3, (n, h, w), 1, False, leaky


@pytest.mark.parametrize("dt", DTYPES)
def test_float32_conv_is_inside_the_bound(dt):
    worst = 0.0
    for cin, cout, k, shape, stride, res, leaky in sorted(set(conv_rows()), key=str):
        o = SC.conv_operands(cin, cout, k, shape, stride, res, dt)
        args = (o["x"], o["w"], o["scale"], o["shift"], leaky)
        kw = dict(stride=stride, pad=k // 2, residual=o["residual"])
        ref, pre, ktot = SC.reference(*args, **kw)
        assert ktot == cin * k * k
        worst = max(worst, inside(SC.float32_conv(*args, dt, **kw), ref, pre, ktot, dt, (cin, cout, k, shape)))
    print("float32 conv, worst |got - ref| / bound:", dt, worst)


def pair_chain(o, c_in, dt, x=None):
    """conv3 + shortcut then conv1 in float32, each stage checked against the float64 reference of its own input"""
    x = o["x"] if x is None else x
    proj = None if o["residual"] is not None else (o["xp"], o["wp"], o["sp"], o["hp"])
    ref, pre, ktot = SC.reference(x, o["w3"], o["s3"], o["h3"], True, residual=o["residual"], proj=proj)
    assert ktot == c_in * (2 if proj else 1)
    y = SC.float32_conv(x, o["w3"], o["s3"], o["h3"], True, dt, residual=o["residual"], proj=proj)
    a = inside(y, ref, pre, ktot, dt, "y")
    refz, prez, kz = SC.reference(y.float(), o["w1"], o["s1"], o["h1"], True)
    return max(a, inside(SC.float32_conv(y.float(), o["w1"], o["s1"], o["h1"], True, dt), refz, prez, kz, dt, "z"))


@pytest.mark.parametrize("dt", DTYPES)
def test_float32_boundaries_are_inside_the_bound(dt):
    worst = 0.0
    for c_out, proj in SC.PAIR_ROWS:
        worst = max(worst, pair_chain(SC.pair_operands(64, 256, c_out, SC.MAP_P, proj, dt), 64, dt))
    worst = max(worst, pair_chain(SC.pair_operands(128, 512, 128, SC.MAP_P, False, dt), 128, dt))
    for shape, forms in SC.C3PAIR_ROWS:
        for form in forms:
            c_out, proj, conv1 = SC.C3PAIR_FORMS[form]
            o = SC.block_operands(shape, c_out, proj, dt)
            t1 = o["t1"]
            if conv1:
                ref, pre, ktot = SC.reference(o["xp"], o["w0"], o["s0"], o["h0"], True)
                t1 = SC.float32_conv(o["xp"], o["w0"], o["s0"], o["h0"], True, dt)
                worst = max(worst, inside(t1, ref, pre, ktot, dt, (shape, form, "t1")))
                t1 = t1.float()
            ref, pre, ktot = SC.reference(t1, o["w33"], o["s2"], o["h2"], True, pad=1)
            t2 = SC.float32_conv(t1, o["w33"], o["s2"], o["h2"], True, dt, pad=1)
            worst = max(worst, inside(t2, ref, pre, ktot, dt, (shape, form, "t2")), pair_chain(o, 64, dt, x=t2.float()))
    print("float32 boundaries, worst |got - ref| / bound:", dt, worst)


def test_the_bound_catches_one_wrong_element():
    """a single element off by one storage ulp more than the rounding allows is outside; its neighbour's value is too"""
    dt = torch.bfloat16
    o = SC.conv_operands(64, 64, 1, SC.MAP_P, 1, False, dt)
    args = (o["x"], o["w"], o["scale"], o["shift"], True)
    ref, pre, ktot = SC.reference(*args)
    good = SC.float32_conv(*args, dt).float()
    big = int(torch.argmax(ref.abs().flatten()))
    bad = good.clone().flatten()
    bad[big] = bad[big] * (1 + 2.0 ** -6)
    assert SC.excess(bad.view_as(good), ref, pre, ktot, dt)[1] == big and SC.excess(bad.view_as(good), ref, pre, ktot, dt)[0] > 1
    moved = torch.roll(good, 1, dims=2)                                      # every pixel holds its neighbour's answer
    assert SC.excess(moved, ref, pre, ktot, dt)[0] > 1
