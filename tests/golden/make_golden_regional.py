"""Generate the regional-pooling fixtures tests/golden/regions.npz and
tests/golden/rpool.npz by running the REFERENCE modules themselves (build
container only, like make_golden.py, whose ``inplace_abn`` stand-in, reference
imports and ``sys.dont_write_bytecode`` this script reuses by importing it).

    python tests/golden/make_golden_regional.py [regions] [rpool]

From the reference, unmodified: cirtorch.modules.pools (Rpool, GeM, GeMmp, MAC,
SPoC), cirtorch.modules.heads.global_head.globalHead and the R18 body / net
wrappers of make_golden.py.  No reference source is copied: the fixtures hold
rectangles, seeds, small weights and outputs only.

regions.npz  the rectangles ``Rpool.roipool`` pools, recorded from the views
             it hands to the inner pool (not from a restatement of its
             arithmetic): every (H, W) in 1..40 x 1..40 at L = 3, and
             L in {1, 2, 4} for a dozen shapes ((3, 13) reaches the L = 4
             maximum, 91).  ``shapes`` [K, 3] (H, W, L), ``offsets`` [K + 1],
             ``rects`` [sum R, 4] (y0, x0, h, w), int16.
rpool.npz    reference float32 outputs of Rpool on f32 inputs [3, 72, H, W]
             (regenerated from the stored seed by oracle.data.rng; a float64
             checksum guards the generator) for the inner pools GeM p=3,
             GeM p=2.5, MAC, SPoC, GeMmp (stored per-channel p in [2, 4]), each
             with and without a stored Linear(72, 72) whitening:
             ``<shape>_<pool>_<w0|w1>_agg`` [3, 72] and ``..._reg`` [R, 72], the
             region descriptors of image 1 (the three images' worth would be
             1.2 MB).  ``..._agg_e64`` / ``..._reg_e64``: max |float32 run -
             float64 run| of the same modules, the reference's own rounding
             error, to calibrate tolerances.  ``head_*``: a globalHead(ROIpool)
             at dim 72 with / without do_whitening.  ``r18reg_*``: an R18 with
             regional=True end to end on the first two images of r18.npz.
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (installs the inplace_abn stand-in, imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from oracle import data, weights  # noqa: E402

R_pools = MG.R_pools

SHAPES = [(7, 7), (5, 9), (9, 5), (3, 11), (1, 1), (2, 7)]
C = 72
SEED = 4101


# ----------------------------------------------------------------------------- regions
def recorded_regions(H, W, L):
    """(y0, x0, h, w) of every view Rpool.roipool hands to the inner pool."""
    x = torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W)
    seen = []

    def spy(t):
        y0, x0 = divmod(int(t[0, 0, 0, 0]), W)
        assert t.data_ptr() == x[0, 0, y0, x0].data_ptr()
        seen.append((y0, x0, t.shape[2], t.shape[3]))
        return torch.zeros(1, 1, 1, 1)

    R_pools.Rpool(rpool=None).roipool(x, spy, L=L)
    return seen


def gen_regions():
    cases = [(h, w, 3) for h in range(1, 41) for w in range(1, 41)]
    for L in (1, 2, 4):
        cases += [(h, w, L) for (h, w) in [(1, 1), (2, 7), (3, 11), (11, 3), (7, 7), (5, 9), (9, 5), (24, 32),
                                            (32, 24), (12, 40), (40, 12), (1, 6), (3, 13)]]
    shapes, offsets, rects = [], [0], []
    for (h, w, L) in cases:
        r = recorded_regions(h, w, L)
        shapes.append((h, w, L))
        rects += r
        offsets.append(len(rects))
    counts = np.diff(offsets)
    print("  %d cases, %d rectangles, max R at L=3: %d, at L=4: %d" % (
        len(cases), len(rects), max(c for c, s in zip(counts, shapes) if s[2] == 3),
        max(c for c, s in zip(counts, shapes) if s[2] == 4)))
    np.savez_compressed(os.path.join(HERE, "regions.npz"), shapes=np.array(shapes, dtype=np.int16),
                        offsets=np.array(offsets, dtype=np.int32), rects=np.array(rects, dtype=np.int16))


# ----------------------------------------------------------------------------- rpool
def rpool_input(h, w):
    """The f32 input of shape (h, w): mostly positive, some below the GeM clamp."""
    r = data.rng(SEED + 100 * h + w)
    return (r.standard_normal((3, C, h, w)).astype(np.float32) * np.float32(0.5) + np.float32(0.2)).astype(np.float32)


def inner_pools(pmp):
    def gemmp():
        m = R_pools.GeMmp(p=3, mp=C, eps=1e-6)
        m.p = torch.from_numpy(pmp).reshape(C, 1, 1)
        return m
    return {"gem3": lambda: R_pools.GeM(p=3, eps=1e-6), "gem2.5": lambda: R_pools.GeM(p=2.5, eps=1e-6),
            "mac": lambda: R_pools.MAC(), "spoc": lambda: R_pools.SPoC(), "gemmp": gemmp}


def linear(wt, b, dtype=torch.float32):
    lin = nn.Linear(wt.shape[1], wt.shape[0], bias=True)
    lin.load_state_dict({"weight": torch.from_numpy(wt), "bias": torch.from_numpy(b)})
    return lin.to(dtype)


def gen_rpool():
    r = data.rng(SEED)
    out = {"seed": np.int64(SEED), "shapes": np.array(SHAPES, dtype=np.int16)}
    pmp = r.uniform(2.0, 4.0, C).astype(np.float32)
    ww = (r.standard_normal((C, C)) * 0.3).astype(np.float32)
    wb = r.uniform(-0.05, 0.05, C).astype(np.float32)
    out.update({"gemmp_p": pmp, "whiten_weight": ww, "whiten_bias": wb})
    with torch.no_grad():
        for (h, w) in SHAPES:
            x = rpool_input(h, w)
            tag = "%dx%d" % (h, w)
            out[tag + "_xsum"] = np.float64(x.astype(np.float64).sum())
            xt = torch.from_numpy(x)
            for name, make in inner_pools(pmp).items():
                for wh in (0, 1):
                    m32 = R_pools.Rpool(make(), whiten=linear(ww, wb) if wh else None, L=3)
                    m64 = R_pools.Rpool(make().double(), whiten=linear(ww, wb, torch.float64) if wh else None, L=3)
                    for agg in (True, False):
                        o32 = m32(xt, aggregate=agg).squeeze(-1).squeeze(-1).numpy()
                        o64 = m64(xt.double(), aggregate=agg).squeeze(-1).squeeze(-1).numpy()
                        assert o32.dtype == np.float32 and o64.dtype == np.float64
                        key = "%s_%s_w%d_%s" % (tag, name, wh, "agg" if agg else "reg")
                        out[key] = o32 if agg else o32[1]
                        out[key + "_e64"] = np.float64(np.abs(o32 - o64).max())
        # globalHead(ROIpool) at dim 72
        hw_ = (r.standard_normal((C, C)) * 0.3).astype(np.float32)
        hb = r.uniform(-0.05, 0.05, C).astype(np.float32)
        out.update({"head_whiten_weight": hw_, "head_whiten_bias": hb})
        for (h, w) in [(7, 7), (3, 11)]:
            head = MG.globalHead(pooling={"name": "ROIpool", "params": {"rpool": R_pools.GeM(p=3, eps=1e-6),
                                                                        "whiten": nn.Linear(C, C), "L": 3}},
                                 normal={"name": "L2N", "params": {}}, dim=C)
            head.load_state_dict({"whiten.weight": torch.from_numpy(hw_), "whiten.bias": torch.from_numpy(hb),
                                  "pool.rpool.p": torch.tensor([3.0]), "pool.whiten.weight": torch.from_numpy(ww),
                                  "pool.whiten.bias": torch.from_numpy(wb)})
            head.eval()
            xt = torch.from_numpy(rpool_input(h, w))
            out["head_%dx%d" % (h, w)] = head(xt).numpy()
            out["head_%dx%d_nowhiten" % (h, w)] = head(xt, do_whitening=False).numpy()
        # R18, regional=True, end to end on the first two images of r18.npz
        g = np.load(os.path.join(HERE, "r18.npz"))
        net, _ = MG.reference_net("resnet18", head_bias=g["head_bias"])
        dim = weights.OUTPUT_DIM["resnet18"]
        rs = regional_state(dim)
        head = MG.globalHead(pooling={"name": "ROIpool", "params": {"rpool": R_pools.GeM(p=3, eps=1e-6),
                                                                    "whiten": nn.Linear(dim, dim), "L": 3}},
                             normal={"name": "L2N", "params": {}}, dim=dim)
        hs = weights.head_state(dim)
        head.load_state_dict({"whiten.weight": torch.from_numpy(hs["whiten.weight"]),
                              "whiten.bias": torch.from_numpy(g["head_bias"]), "pool.rpool.p": torch.tensor([3.0]),
                              "pool.whiten.weight": torch.from_numpy(rs["pool.whiten.weight"]),
                              "pool.whiten.bias": torch.from_numpy(rs["pool.whiten.bias"])})
        net.ret_head = head.eval()
        imgs = data.structured_images(int(g["n"]), *[int(v) for v in g["res"]], seed=int(g["seed"]))[:2]
        out["r18reg_desc"] = MG.run_ref(net, list(imgs))
    np.savez_compressed(os.path.join(HERE, "rpool.npz"), **out)
    print("  rpool.npz: %d arrays, %.0f KB" % (len(out), os.path.getsize(os.path.join(HERE, "rpool.npz")) / 1024))
    worst = max((float(v), k) for k, v in out.items() if k.endswith("_e64"))
    print("  largest float32-vs-float64 difference of the reference: %.3g (%s)" % worst)


def regional_state(dim, seed=weights.SEED_WEIGHTS):
    """The regional whitening Linear of the R18 case, from the oracle's weight streams."""
    std = np.float32(0.1 * np.sqrt(2.0 / (dim + dim)))
    return {"pool.whiten.weight": (weights._stream(seed, "pool.whiten.weight").standard_normal((dim, dim), dtype=np.float32)
                                   * std).astype(np.float32),
            "pool.whiten.bias": weights._stream(seed, "pool.whiten.bias").uniform(-0.002, 0.002, dim).astype(np.float32)}


if __name__ == "__main__":
    names = sys.argv[1:] or ["regions", "rpool"]
    for name in names:
        print("golden", name)
        {"regions": gen_regions, "rpool": gen_rpool}[name]()
    print("done")
