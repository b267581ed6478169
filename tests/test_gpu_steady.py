"""The persistent conv kernels past their ring depth, against float64 (tests/steady_cases.py has the tables, the
launch arithmetic and the references; tests/test_host_steady.py shows what every row reaches).

One checker for every family.  A capped run (RR_TUNE_GRID_CUS below the device's CU count) writes into a view of a
buffer filled with 0xFF bytes (0xFFFF is a NaN in bf16 and fp16) with 64 pixel-rows of guard on either side, so a
tile that is never written, or a store outside the map, cannot hide behind what the allocator left there.  Then:
rr_last_launch must report the kernel, variant, block size, grid, slices and xmap that the plan functions give;
the guards must be intact and the output finite; every element must be within the bound of steady_cases of the
float64 reference (chained through the kernel's own 16-bit intermediates); the bits must equal those of the same op
uncapped, of the sibling kernels the project claims bit-identity with, and of two more capped runs.

These tests prove the indexing, the slot and register rotation, the tails and the store masks at these tile
counts.  The three identical runs are a determinism check only: a counted wait that is one too loose can pass
any number of clean runs, so nothing here proves the waits right.

If an element were outside the bound the failure message carries the same element's figure from the tiled engine
(STREAM_1X1 = 0, CONV3X3 = 0, GEMM8 = 0), the independent kernel by which the middle term may be widened -- never by the
kernel under test.  No widening was needed.  Worst |got - ref| / bound measured on an MI355X (bf16, fp16; the bound
is 1, and the output rounding alone reaches it at a value just above a power of two):
  k_wres1x1 0.990, 0.966    k_stream1x1 0.990, 0.977    k_stream_pair 0.991, 0.979    k_pair_mid_ring / k_pair_mid 0.981, 0.959
  k_c3pair 0.993, 0.980     k_conv3x3 / k_c3w64 0.910, 0.650
The float32 evaluation of the same cases on the host (test_host_steady.py) reaches 0.993: the kernels' MFMA sums sit
where a float32 sum does."""

import math

import pytest
import torch

import steady_cases as SC

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
GUARD_ROWS = 64
TILED = dict(STREAM_1X1=0, CONV3X3=0, GEMM8=0)


def _mods():
    from cirtorch import _engine as E, _ops as ops
    return E, ops


class Poisoned:
    """a contiguous tensor of the given shape inside a buffer of 0xFF bytes, 64 pixel-rows of guard before and after"""

    def __init__(self, shape, dt, cuda):
        self.g = GUARD_ROWS * shape[-1]
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * self.g,), -1, dtype=torch.int16, device=cuda)
        self.t = self.buf[self.g:self.g + n].view(dt).view(shape)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0 and bool(torch.isnan(self.t.float()).all())

    def intact(self):
        return bool((self.buf[:self.g] == -1).all()) and bool((self.buf[-self.g:] == -1).all())


def run(cuda, op, shapes, dt, **tune):
    """op(*outs) under the tuning, every out poisoned -> (outs, what rr_last_launch reports); guards and finiteness checked"""
    E, _ = _mods()
    outs = [Poisoned(s, dt, cuda) for s in shapes]
    with E.tuning(**tune):
        op(*[o.t for o in outs])
        info = E.last_launch()
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert o.intact(), ("guard rows touched", i, info, tune)
        bad = int((~torch.isfinite(o.t.float())).sum())
        assert bad == 0, ("elements never written or not finite", i, bad, info, tune)
    return [o.t for o in outs], info


def launched(info, kernel, variant, block, plan):
    want = dict(kernel=kernel, variant=variant, grid=plan.grid, block=block, nslices=plan.nslices, xmap=plan.xmap, launches=1)
    assert info == want, (info, want)


def capped(cuda, cap):
    assert torch.cuda.get_device_properties(cuda).multi_processor_count > cap, "the cap must be below the device's CU count"


def within(got, ref3, dt, what, family, tiled=None):
    """the element-wise bound; tiled: a function that returns the tiled engine's output for the failure message"""
    ref, pre, ktot = ref3
    worst, i = SC.excess(got, ref, pre, ktot, dt)
    print("%s %s %s: worst |got - ref| / bound = %.4f" % (family, dt, what, worst))
    if worst > 1.0:
        other = None
        if tiled is not None:
            t = tiled().double().flatten()[i]
            other = float((t - ref.flatten()[i]).abs() / SC.bound(ref, pre, ktot, dt).flatten()[i])
        raise AssertionError("%s: element %d is %.3f x the bound (the tiled engine's at that element: %s)" % (what, i, worst, other))


def three_times(cuda, op, shapes, dt, first, **tune):
    for _ in range(2):
        again, _ = run(cuda, op, shapes, dt, **tune)
        assert all(torch.equal(a, b) for a, b in zip(again, first)), ("not the same bits on a repeated run", tune)


def dev(o, cuda, dt, *names):
    """the named operands on the device: activations and weights in dt, affines in float32"""
    out = []
    for nm in names:
        t = o[nm]
        out.append(None if t is None else t.to(cuda) if t.dim() == 1 else t.to(dt).to(cuda))
    return out


def pack(ops, w, dt, cuda):
    return ops.pack_conv_weights(w.to(cuda), w.shape[1], dt, perm32=True)


def ref_on(cuda, *args, **kw):
    """steady_cases.reference with every tensor moved to the device (float64 matrix products there)"""
    mv = lambda t: t.to(cuda) if torch.is_tensor(t) else tuple(mv(q) for q in t) if isinstance(t, tuple) else t  # noqa: E731
    return SC.reference(*[mv(a) for a in args], **{k: mv(v) for k, v in kw.items()})


# ---------------------------------------------------------------- one conv2d_fused row
def conv_row(cuda, dt, family, cin, cout, k, shape, stride, res, leaky, variants, sibling=None, uncapped_variant=True):
    """variants: [(label, cap, tuning, (kernel, variant, block, plan))]; the first run of all is uncapped with the first
    variant's tuning.  sibling: (tuning, kernel name) of a kernel with the same bits.  Every variant must have the bits
    of every other."""
    E, ops = _mods()
    o = SC.conv_operands(cin, cout, k, shape, stride, res, dt)
    x, residual = dev(o, cuda, dt, "x", "residual")
    scale, shift = dev(o, cuda, dt, "scale", "shift")
    wp = pack(ops, o["w"], dt, cuda)
    oshape = (*SC.out_map(shape, stride), cout) if k == 1 else (*shape, cout)
    pad = k // 2

    def op(y):
        ops.conv2d_fused(x, wp, k, k, stride, pad, cout, scale, shift, residual=residual, leaky=leaky, slope=SC.SLOPE,
                         perm32=True, out=y)

    ref3 = ref_on(cuda, o["x"], o["w"], o["scale"], o["shift"], leaky, stride=stride, pad=pad, residual=o["residual"])
    tiled = lambda: run(cuda, op, [oshape], dt, **TILED)[0][0]  # noqa: E731
    base = None
    for label, cap, tune, (kernel, variant, block, plan) in variants:
        capped(cuda, cap)
        (free,), info = run(cuda, op, [oshape], dt, GRID_CUS=0, **tune)
        assert info["kernel"] == kernel and (info["variant"] == variant or not uncapped_variant), (label, info)
        (got,), info = run(cuda, op, [oshape], dt, GRID_CUS=cap, **tune)
        launched(info, kernel, variant, block, plan)
        within(got, ref3, dt, "%s cap %d" % (label, cap), family, tiled)
        assert torch.equal(got, free), (label, cap, "capped and uncapped bits differ")
        base = got if base is None else base
        assert torch.equal(got, base), (label, cap, "bits differ from the first variant's")
        three_times(cuda, op, [oshape], dt, [got], GRID_CUS=cap, **tune)
    if sibling is not None:
        tune, kernel = sibling
        (sib,), info = run(cuda, op, [oshape], dt, **tune)
        assert info["kernel"] == kernel, info
        within(sib, ref3, dt, "sibling " + (kernel or "tiled engine"), family)
        assert torch.equal(sib, base), ("bits differ from the sibling's", kernel)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("row", SC.WRES_ROWS, ids=lambda r: "%d-%d-%s-s%d" % (r[0], r[1], "res" if r[2] else "plain", r[4]))
def test_wres1x1_past_the_ring(cuda, dt, row):
    """k_wres1x1 with 16 .. 137 tiles per block: the 3-, 4- and 6-buffer rings wrap at least twice and end on a tail;
    ring on and off; bit-identical to what WRES = 0 runs (k_stream1x1, or the tiled engine where it has no such form)"""
    k, c, res, leaky, stride, shape, caps = row
    cw = SC.wres_cw(k)
    variants = []
    for cap in caps:
        plan = SC.wres_plan(SC.pixels(shape, stride), c, 8 * cw, cap)
        for ring in (1, 0):
            form = "res" if res else ("ring" if ring else "noring")
            variants.append(("ring %d" % ring, cap, dict(WRES=2, WRES_RING=ring), ("k_wres1x1", "%d,%d,%s" % (k, cw, form), 512, plan)))
    # WRES = 0: k_stream1x1 where it has the form, else (plain 512 -> 2048, 256 -> 1024) the tiled engine, as in test_wres1x1
    other = "" if not res and (k, c) in ((512, 2048), (256, 1024)) else "k_stream1x1"
    conv_row(cuda, dt, "k_wres1x1", k, c, 1, shape, stride, res, leaky, variants, sibling=(dict(WRES=0, GEMM8=0), other))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("row", SC.STREAM_ROWS, ids=lambda r: "%d-%d-%s-n%d-s%d" % (r[0], r[1], "res" if r[2] else "plain", r[5][0], r[4]))
def test_stream1x1_past_the_depth(cuda, dt, row):
    """k_stream1x1 with 4 .. 35 strips per wave: the D = 2, 3, 4 register rotation past 2 D strips with a clamped refill
    at the tail, one to sixteen channel slices, XCD map on and off"""
    k, c, res, leaky, stride, shape, caps, wres = row
    tc, _, fn, d, nw = SC.stream_variant(k, c)
    variant = "%d,%d,%d,%d,%d%s" % (tc, k, fn, d, nw, ",res" if res else "")
    variants = [("stream", cap, dict(WRES=wres, GEMM8=0),
                 ("k_stream1x1", variant, 64 * nw, SC.stream_plan(SC.pixels(shape, stride), tc, k, fn, d, nw, c, cap))) for cap in caps]
    conv_row(cuda, dt, "k_stream1x1", k, c, 1, shape, stride, res, leaky, variants)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("row", SC.C3_ROWS, ids=lambda r: "x".join(map(str, r[0])))
def test_conv3x3_past_two_tiles(cuda, dt, row):
    """k_conv3x3 and k_c3w64 with 3 .. 12 tiles per block (CONV3S = 0): the software-pipelined tile loop and the
    overlapped epilogue in their steady state, CONV3_PIPE on and off, every mode the bits of every other"""
    (n, cin, h, w, cout), leaky, runs = row
    variants = []
    for mode, cap in runs:
        kernel, v = SC.c3_variant(cin, cout, h, mode, cap, n, w)
        for pipe in (1, 0):
            tune = dict(CONV3S=0, CONV3X3=mode, CONV3_PIPE=pipe)
            if v is None:
                want = ("k_c3w64", "64,8,32", 512, SC.c3w64_plan(n, h, w, cap))
            else:
                want = ("k_conv3x3", "%d,%d,%d,%d,%d,%d,pipe%d" % (*v, pipe), 64 * v[3] * v[4], SC.c3_plan(n, h, w, cout, *v[:3], cap))
            variants.append(("mode %d pipe %d" % (mode, pipe), cap, tune, want))
    # uncapped, modes 2 and 7 choose their tile height by the CU count (rr_conv3.hip:587): the name only there
    conv_row(cuda, dt, "direct 3x3", cin, cout, 3, (n, h, w), 1, False, leaky, variants, uncapped_variant=False)


# ---------------------------------------------------------------- the 1x1 boundaries
def pair_refs(cuda, o, dt, x, y):
    """(ref, pre, Ktot) of y from the x the launch read and of z from the y it returned"""
    proj = None if o["residual"] is not None else (o["xp"], o["wp"], o["sp"], o["hp"])
    ry = ref_on(cuda, x.float(), o["w3"], o["s3"], o["h3"], True, residual=o["residual"], proj=proj)
    rz = ref_on(cuda, y.float(), o["w1"], o["s1"], o["h1"], True)
    return ry, rz


def pair_setup(cuda, dt, o, c_in, proj):
    _, ops = _mods()
    x, residual, xp = dev(o, cuda, dt, "x", "residual", "xp")
    s3, h3, s1, h1, sp, hp = dev(o, cuda, dt, "s3", "h3", "s1", "h1", "sp", "hp")
    w3p, w1p, wpp = pack(ops, o["w3"], dt, cuda), pack(ops, o["w1"], dt, cuda), pack(ops, o["wp"], dt, cuda)
    pj = (xp, wpp, sp, hp) if proj else None
    return x, residual, pj, (w3p, s3, h3), (w1p, s1, h1)


def unfused_pair(cuda, dt, x, residual, c3, c1, c_mid, c_out, shape):
    """the two launches that the boundary fuses, each into its own poisoned buffer (residual form)"""
    _, ops = _mods()
    (y2,), _ = run(cuda, lambda y: ops.conv2d_fused(x, c3[0], 1, 1, 1, 0, c_mid, c3[1], c3[2], residual=residual, leaky=True,
                                                    slope=SC.SLOPE, perm32=True, out=y), [(*shape, c_mid)], dt)
    (z2,), _ = run(cuda, lambda z: ops.conv2d_fused(y2, c1[0], 1, 1, 1, 0, c_out, c1[1], c1[2], leaky=True, slope=SC.SLOPE,
                                                    perm32=True, out=z), [(*shape, c_out)], dt)
    return y2, z2


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("c_out,proj", SC.PAIR_ROWS)
def test_stream_pair_past_the_depth(cuda, dt, c_out, proj):
    """k_stream_pair with 3/4 and 6/7 strips per wave: the D = 2 rotation, the niter / nmine tail, all four forms"""
    _, ops = _mods()
    shape = SC.MAP_P
    o = SC.pair_operands(64, 256, c_out, shape, proj, dt)
    x, residual, pj, c3, c1 = pair_setup(cuda, dt, o, 64, proj)
    shapes = [(*shape, 256), (*shape, c_out)]

    def op(y, z):
        ops.conv1x1_pair(x, *c3, residual, True, SC.SLOPE, *c1, c_out, True, SC.SLOPE, proj=pj, out=(y, z))

    variant = "%d,2,%s" % (c_out, "proj" if proj else "res")
    (fy, fz), info = run(cuda, op, shapes, dt, GRID_CUS=0)
    assert (info["kernel"], info["variant"]) == ("k_stream_pair", variant), info
    ry, rz = pair_refs(cuda, o, dt, x, fy)
    for cap in SC.PAIR_CAPS:
        capped(cuda, cap)
        (y, z), info = run(cuda, op, shapes, dt, GRID_CUS=cap)
        launched(info, "k_stream_pair", variant, 512, SC.pair_plan(SC.pixels(shape), cap))
        within(y, ry, dt, "y cap %d" % cap, "k_stream_pair")
        within(z, rz, dt, "z cap %d" % cap, "k_stream_pair")
        assert torch.equal(y, fy) and torch.equal(z, fz), (cap, "capped and uncapped bits differ")
        three_times(cuda, op, shapes, dt, [y, z], GRID_CUS=cap)
    if not proj:  # the rule of test_conv1x1_pair: y bit for bit, z equal on more than 99 % (another K-step order below 4096 px)
        y2, z2 = unfused_pair(cuda, dt, x, residual, c3, c1, 256, c_out, shape)
        assert torch.equal(fy, y2)
        assert (fz.float() == z2.float()).float().mean().item() > 0.99


@pytest.mark.parametrize("dt", DTYPES)
def test_pair_mid_past_the_ring(cuda, dt):
    """k_pair_mid_ring with 9, 13/14 and 27 tiles per block (4 residual slots, 2 x buffers) and k_pair_mid with 4/5 and
    14 (2 residual buffers): the partial last tile, and both kernels the same bits"""
    _, ops = _mods()
    shape = SC.MAP_P
    o = SC.pair_operands(128, 512, 128, shape, False, dt)
    x, residual, _, c3, c1 = pair_setup(cuda, dt, o, 128, False)
    shapes = [(*shape, 512), (*shape, 128)]

    def op(y, z):
        ops.conv1x1_pair(x, *c3, residual, True, SC.SLOPE, *c1, 128, True, SC.SLOPE, out=(y, z))

    (fy, fz), info = run(cuda, op, shapes, dt, GRID_CUS=0, PAIR_MID=1)
    assert info["kernel"] == "k_pair_mid_ring", info
    ry, rz = pair_refs(cuda, o, dt, x, fy)
    for mid, caps in SC.MID_CAPS.items():
        kernel, tp = ("k_pair_mid_ring", 32) if mid else ("k_pair_mid", 64)
        (uy, uz), info = run(cuda, op, shapes, dt, GRID_CUS=0, PAIR_MID=mid)
        assert info["kernel"] == kernel, info
        assert torch.equal(uy, fy) and torch.equal(uz, fz), ("PAIR_MID 1 and 0 differ", mid)
        for cap in caps:
            capped(cuda, cap)
            (y, z), info = run(cuda, op, shapes, dt, GRID_CUS=cap, PAIR_MID=mid)
            launched(info, kernel, "128,512,128,res", 512, SC.mid_plan(SC.pixels(shape), cap, tp))
            within(y, ry, dt, "%s y cap %d" % (kernel, cap), kernel)
            within(z, rz, dt, "%s z cap %d" % (kernel, cap), kernel)
            assert torch.equal(y, fy) and torch.equal(z, fz), (kernel, cap, "capped and uncapped bits differ")
            three_times(cuda, op, shapes, dt, [y, z], GRID_CUS=cap, PAIR_MID=mid)
    # the rule of test_conv1x1_pair_mod3 below 4096 px: y bit for bit, z equal on more than 99 %
    y2, z2 = unfused_pair(cuda, dt, x, residual, c3, c1, 512, 128, shape)
    assert torch.equal(fy, y2)
    assert (fz.float() == z2.float()).float().mean().item() > 0.99


# ---------------------------------------------------------------- k_c3pair
C3PAIR_PARAMS = [(shape, form) for shape, forms in SC.C3PAIR_ROWS for form in forms]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,form", C3PAIR_PARAMS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_c3pair_one_to_seven_tiles(cuda, dt, shape, form):
    """k_c3pair with 1 .. 7 tiles per block (one block per XCD under a cap of 8; two under 16): the tail of the pair
    role's two-tile unroll on odd and even counts, the 4-slot tile ring, the lookahead slot holding -1, idle blocks;
    the dynamic and the static walk; bit-identical to the 3x3 launch followed by rr_conv1x1_pair"""
    _, ops = _mods()
    c_out, proj, conv1 = SC.C3PAIR_FORMS[form]
    n, h, w = shape
    o = SC.block_operands(shape, c_out, proj, dt)
    _, residual, pj, c3, c1 = pair_setup(cuda, dt, o, 64, proj)
    (t1,), (s2, h2, s0, h0) = dev(o, cuda, dt, "t1"), dev(o, cuda, dt, "s2", "h2", "s0", "h0")
    w33p, w0p = pack(ops, o["w33"], dt, cuda), pack(ops, o["w0"], dt, cuda)
    shapes = [(*shape, 256), (*shape, c_out)]
    src, c1arg = t1, None
    if conv1:  # the launch reads the block input and runs conv1 itself; unfused, conv1 is its own launch
        src, c1arg = pj[0], (w0p, s0, h0, True, SC.SLOPE)
        (t1,), _ = run(cuda, lambda t: ops.conv2d_fused(src, w0p, 1, 1, 1, 0, 64, s0, h0, leaky=True, slope=SC.SLOPE, perm32=True,
                                                        out=t), [(*shape, 64)], dt)
        within(t1, ref_on(cuda, o["xp"], o["w0"], o["s0"], o["h0"], True), dt, "t1", "k_c3pair")
    # the unfused chain; t2 is the fused kernel's by design, checked against float64 here from the t1 it read
    (t2,), _ = run(cuda, lambda t: ops.conv2d_fused(t1, w33p, 3, 3, 1, 1, 64, s2, h2, leaky=True, slope=SC.SLOPE, perm32=True, out=t),
                   [(*shape, 64)], dt)
    within(t2, ref_on(cuda, t1.float(), o["w33"], o["s2"], o["h2"], True, pad=1), dt, "t2", "k_c3pair")
    (y2, z2), _ = run(cuda, lambda y, z: ops.conv1x1_pair(t2, *c3, residual, True, SC.SLOPE, *c1, c_out, True, SC.SLOPE, proj=pj,
                                                          out=(y, z)), shapes, dt)
    ry, rz = pair_refs(cuda, o, dt, t2, y2)
    variant = "%d%s%s" % (c_out, ",proj" if proj else "", ",conv1" if conv1 else "")
    ntiles = n * (h // 4) * (w // 32)
    for cap in (8, 16) if ntiles >= 16 else (8,):
        capped(cuda, cap)
        plan = SC.c3pair_plan(n, h, w, cap)[0]
        for dyn in (True, False):
            def op(y, z):
                ops.conv3x3_pair(src, w33p, s2, h2, True, SC.SLOPE, *c3, residual, True, SC.SLOPE, *c1, c_out, True, SC.SLOPE,
                                 proj=pj, dynamic=dyn, conv1=c1arg, out=(y, z))

            (fy, fz), info = run(cuda, op, shapes, dt, GRID_CUS=0)
            assert (info["kernel"], info["variant"]) == ("k_c3pair", variant), info
            (y, z), info = run(cuda, op, shapes, dt, GRID_CUS=cap)
            launched(info, "k_c3pair", variant, 512, plan)
            what = "%s cap %d %s" % (form, cap, "dynamic" if dyn else "static")
            within(y, ry, dt, "y " + what, "k_c3pair")
            within(z, rz, dt, "z " + what, "k_c3pair")
            assert torch.equal(y, fy) and torch.equal(z, fz), (what, "capped and uncapped bits differ")
            assert torch.equal(y, y2) and torch.equal(z, z2), (what, "bits differ from the unfused launches'")
            three_times(cuda, op, shapes, dt, [y, z], GRID_CUS=cap)


def test_conv3s_records_its_name(cuda):
    """the staggered 3x3 (out of scope here: tests/test_gpu_kernels.py runs it under a cap) leaves its name and grid in the record"""
    E, ops = _mods()
    dt, shape = torch.bfloat16, (3, 24, 96)
    o = SC.conv_operands(128, 128, 3, shape, 1, False, dt)
    (x,), (scale, shift) = dev(o, cuda, dt, "x"), dev(o, cuda, dt, "scale", "shift")
    wp = pack(ops, o["w"], dt, cuda)
    op = lambda y: ops.conv2d_fused(x, wp, 3, 3, 1, 1, 128, scale, shift, leaky=True, slope=SC.SLOPE, perm32=True, out=y)  # noqa: E731
    capped(cuda, 8)
    (got,), info = run(cuda, op, [(*shape, 128)], dt, GRID_CUS=8, CONV3X3=1, CONV3S=1)
    assert info == dict(kernel="k_c3s_w128", variant="", grid=8, block=512, nslices=0, xmap=1, launches=1), info
    within(got, ref_on(cuda, o["x"], o["w"], o["scale"], o["shift"], True, pad=1), dt, "k_c3s_w128 cap 8", "k_c3s")
