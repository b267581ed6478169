"""Shared by tests/golden/make_golden_stem_bits.py and tests/test_gpu_stem_bits.py: the calls whose
output bytes tests/golden/stem_bits.npz pins, as SHA-256 digests.  Every stem kernel of
csrc/rr_stem.hip (RR_TUNE_STEM 0-6) on the smallest shapes that reach each of its branches, with
bf16 and fp16 weights and float32 and uint8 pixels, and with RR_TUNE_GRID_CUS caps that make a block
walk several tiles: the next-tile prefetch, the patch double buffer and the part-wise fill schedule
run in no other unit test (every other stem test has fewer tiles than the device has CUs).

group          shape (n, h, w)  reaches                                               modes  grids
even_one_tile  (2, 64, 84)      one 8 x 56 tile per image, waves 3..7 idle, st1 cut   0-6    no cap
even_tiles     (1, 100, 472)    4 x 3 tiles, partial last tile both ways              0-6    no cap, 5 (blocks walk
                                                                                             3, 3, 2, 2, 2 tiles)
even_batch     (3, 200, 132)    7 tile rows x 3 images, image boundary inside a walk  0-6    4
odd_v1         (2, 61, 83)      odd stem map: v1's 4 x 32 tiles, 8 of them            0, 2   no cap, 3
ragged         map 200 x 132    extents (200, 132), (198, 131) odd width with pair    0, 2-6 4
                                overhang, (37, 1) the one-pixel row of pair_base,
                                (1, 90) the one-row image, and a None entry
plain          (2, 64, 84)      no normalisation, identity activation                 0, 1,  no cap
                                                                                      2, 5

Inputs come from torch.Generator().manual_seed(...) on the CPU; scale[::3] *= -1 and scale[5] = 0
(negated weight rows, a zero scale), mean / std normalisation except in `plain`.

groups() names the groups, cases(group) the calls of one (no GPU needed); run(group, cuda) ->
{'<group>_out': the SHA-256 of each case's output bytes [cases, 32], '<group>_in': the SHA-256 of its
input bytes (pixels, conv weights, scale, shift: tells a change of torch's CPU generator from a
change of the kernels) [cases, 32], '<group>_shape': its output shape as 4 int64 [cases, 32],
'<group>_cases': the case names, one per line}, uint8 arrays with one row per case in the order of
cases(group)."""

import hashlib

import numpy as np
import torch

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
PIXELS = ("f32", "u8")

RAGGED_MAP = (200, 132)
RAGGED_EXTENTS = [(200, 132), (198, 131), (37, 1), None, (1, 90)]

# group -> (shape, modes, grid caps (0 = no cap), seed)
GROUPS = {
    "even_one_tile": ((2, 64, 84), (0, 1, 2, 3, 4, 5, 6), (0,), 101),
    "even_tiles": ((1, 100, 472), (0, 1, 2, 3, 4, 5, 6), (0, 5), 102),
    "even_batch": ((3, 200, 132), (0, 1, 2, 3, 4, 5, 6), (4,), 103),
    "odd_v1": ((2, 61, 83), (0, 2), (0, 3), 104),
    "ragged": ((len(RAGGED_EXTENTS),) + RAGGED_MAP, (0, 2, 3, 4, 5, 6), (4,), 105),
    "plain": ((2, 64, 84), (0, 1, 2, 5), (0,), 106),
}


def groups():
    return list(GROUPS)


def cases(group):
    """[(case name, mode, grid cap, weight dtype name, pixel type)] of one group"""
    _, modes, grids, _ = GROUPS[group]
    return [("%s_m%d_g%d_%s_%s" % (group, m, cap, dt, px), m, cap, dt, px)
            for m in modes for cap in grids for dt in DTYPES for px in PIXELS]


def case_names(group):
    """the names of cases(group), one per line, as bytes: which row of the fixture is which call"""
    return np.frombuffer("\n".join(c[0] for c in cases(group)).encode(), dtype=np.uint8)


def raw(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


def digest(*blobs):
    h = hashlib.sha256()
    for b in blobs:
        h.update(b)
    return np.frombuffer(h.digest(), dtype=np.uint8)


def inputs(group):
    """-> {pixel type: CPU pixels (a tensor, or for `ragged` a list with None entries)}, wt, scale, shift"""
    (n, h, w), _, _, seed = GROUPS[group]
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, h, w, generator=g)
    wt = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    scale = torch.rand(64, generator=g) + 0.5
    scale[::3] *= -1.0
    scale[5] = 0.0
    shift = torch.randn(64, generator=g) * 0.1
    pix = {"f32": x, "u8": (x * 255).to(torch.uint8)}
    if group == "ragged":
        pix = {k: [None if e is None else v[i, :, :e[0], :e[1]].contiguous() for i, e in enumerate(RAGGED_EXTENTS)]
               for k, v in pix.items()}
    return pix, wt, scale, shift


def run(group, cuda):
    from cirtorch import _engine as E
    from cirtorch import _ops
    pix, wt, scale, shift = inputs(group)
    plain = group == "plain"
    kw = dict(leaky=not plain, slope=0.01, mean=None if plain else MEAN, std=None if plain else STD)
    dscale, dshift = scale.to(cuda), shift.to(cuda)
    wpk = {dt: _ops.pack_stem_weights(wt.to(cuda), tdt) for dt, tdt in DTYPES.items()}
    common = raw(wt) + raw(scale) + raw(shift)
    if group == "ragged":
        dpix = {k: [None if t is None else t.to(cuda) for t in v] for k, v in pix.items()}
        din = {k: digest(*[b"-" if t is None else raw(t) for t in v], common) for k, v in pix.items()}
    else:
        dpix = {k: v.to(cuda) for k, v in pix.items()}
        din = {k: digest(raw(v), common) for k, v in pix.items()}
    out, inp, shape = [], [], []
    for _, mode, cap, dt, px in cases(group):
        with E.tuning(STEM=mode, GRID_CUS=cap):
            if group == "ragged":
                y = _ops.stem_conv_pool_ragged(dpix[px], RAGGED_MAP[0], RAGGED_MAP[1], wpk[dt], dscale, dshift, **kw)
            else:
                y = _ops.stem_conv_pool(dpix[px], wpk[dt], dscale, dshift, **kw)
        out.append(digest(raw(y)))
        inp.append(din[px])
        shape.append(np.frombuffer(np.array(y.shape, dtype=np.int64).tobytes(), dtype=np.uint8))
    return {group + "_out": np.stack(out), group + "_in": np.stack(inp), group + "_shape": np.stack(shape),
            group + "_cases": case_names(group)}
