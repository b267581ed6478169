"""Shared by tests/test_host_hard_geometry.py and tests/test_gpu_hard_geometry.py: seeded inputs that put
the engine's own solvers (the Gauss-Jordan seven-point solver with its closed-form cubic, the four-point
solver with its determinant gate, the 3 x 3 Jacobi of rr_essential_decompose and the one-sided Jacobi
of rr_triangulate_points) on geometry the fixtures of epipolar_cases.planted_pair never reach: large
rotations, forward motion with the epipole in the image, a tiny baseline, long focal lengths, three
of four points nearly on a line, rotations by 0 and pi, low parallax.  The oracles are the float64
numpy restatements of verify_cases / epipolar_cases / pose_cases.  numpy only.

A pair with exactly the minimal number of matches, iters = 1 and refine = 0 returns the minimal solver's
own answer: one hypothesis, its sample all the records in hash order, no refit.

`python tests/hard_geometry_cases.py` prints the figures recorded below as constants."""

import functools

import numpy as np

import epipolar_cases as EC
import pose_cases as PC
import verify_cases as VC

SEED = 11000
RUN_SEED = EC.RUN_SEED
TH_MIN = 1e-6            # px: the threshold of the minimal-solver runs
NOISE = 0.3              # px, on side 2
TRIES = 64               # bound of every rejection loop
W, H_IMG, FOCAL = EC.W, EC.H_IMG, EC.FOCAL

# ---------------------------------------------------------------- two-view scenes of four kinds
KINDS = ("ordinary", "wide", "forward", "narrow")
PER_KIND = 200


def motion(kind, r):
    """ordinary: planted_pair's; wide: rotations up to 0.6 rad per axis; forward: t near the optical axis
    (the epipole inside the image); narrow: the ordinary baseline times 0.01"""
    amp = 0.6 if kind == "wide" else 0.25
    R = EC.rot(*r.uniform(-amp, amp, 3))
    if kind == "forward":
        t = np.array([r.uniform(-0.1, 0.1), r.uniform(-0.1, 0.1), r.uniform(0.8, 1.5)])
    else:
        t = np.array([r.uniform(0.6, 1.2) * r.choice([-1, 1]), r.uniform(-0.3, 0.3), r.uniform(-0.5, 0.5)])
        if kind == "narrow":
            t = 0.01 * t
    return R, t


def scene(kind, n, r, plane=False):
    """n correspondences of a scene of `kind` -> rec [n, 4] (float32 values held in float64), R, t.
    Depths 3 .. 40 (plane=True: the points of one plane through that range), NOISE px on side 2, both
    projections inside the frame.  Both rejection loops are bounded."""
    for _ in range(TRIES):
        R, t = motion(kind, r)
        nrm = np.array([r.uniform(-0.3, 0.3), r.uniform(-0.3, 0.3), 1.0])
        dist = r.uniform(3.0, 40.0)
        rec = np.empty((0, 4))
        for _ in range(TRIES):
            px = r.uniform([0, 0], [W, H_IMG], (8 * n + 16, 2))
            ray = np.concatenate([(px - EC.K[:2, 2]) / FOCAL, np.ones((len(px), 1))], 1)
            z = dist / (ray @ nrm) if plane else r.uniform(3.0, 40.0, len(px))
            q, zz = EC.project(ray * z[:, None], R, t)
            q = q + NOISE * r.standard_normal(q.shape)
            ok = VC.inside(q) & (zz > 0.5) & (z > 0.5)
            rec = np.concatenate([rec, np.concatenate([px, q], 1)[ok]])
            if len(rec) >= n:
                return rec[:n].astype(np.float32).astype(np.float64), R, t
    raise RuntimeError("no %s scene with %d points inside both frames" % (kind, n))


def minimal_pair(rec):
    """records [m, 4] as a pair in which every row is matched to the row of the same index"""
    return rec[:, :2].astype(np.float32), rec[:, 2:].astype(np.float32), np.arange(len(rec), dtype=np.int64)


def ragged(tuples):
    """kp1 [rows, 2] f32, off [P + 1], kp2, off, match [rows] of equally long minimal pairs"""
    m = len(tuples[0]["rec"])
    rec = np.concatenate([t["rec"] for t in tuples])
    off = np.arange(len(tuples) + 1, dtype=np.int64) * m
    return rec[:, :2].astype(np.float32), off, rec[:, 2:].astype(np.float32), off.copy(), np.tile(np.arange(m, dtype=np.int64), len(tuples))


# ---------------------------------------------------------------- seven-point tuples
def cubic_roots_ld(c3, c2, c1, c0):
    """epipolar_cases.cubic_roots evaluated in extended precision: the roots its float64 arithmetic aims at"""
    ld = np.longdouble
    if not (np.isfinite([c3, c2, c1, c0]).all() and abs(c3) > 0):
        return []
    c3, c2, c1, c0 = ld(c3), ld(c2), ld(c1), ld(c0)
    a, b, c = c2 / c3, c1 / c3, c0 / c3
    Q = (a * a - 3 * b) / 9
    R = (2 * a ** 3 - 9 * a * b + 27 * c) / 54
    if R * R < Q ** 3:
        th = np.arccos(np.clip(R / np.sqrt(Q ** 3), ld(-1), ld(1)))
        return [-2 * np.sqrt(Q) * np.cos((th + 2 * ld(np.pi) * k) / 3) - a / 3 for k in (0, -1, 1)]
    A = -np.sign(R) * np.cbrt(abs(R) + np.sqrt(R * R - Q ** 3))
    B = Q / A if A != 0 else ld(0)
    return [A + B - a / 3]


ORDERS = ([6, 5, 4, 3, 2, 1, 0], [3, 0, 6, 2, 5, 1, 4], [1, 2, 3, 4, 5, 6, 0])


def fund_spread(rec, p, root, nroots):
    """How far float64 routes to the same root differ on one seven-tuple (f_err from the Gauss-Jordan route): the
    other null-space routine, the records in three other orders with either routine, and the cubic's closed form
    in extended precision.  None when a route finds another number of roots.  Two null-space routines alone
    share one evaluation of the cubic and so hide its conditioning: near a double root acos loses half the digits,
    and there the routes differ by 1e-9 and more where the two routines agree to 1e-14."""
    q = rec[EC.draw_n(RUN_SEED, p, [0], 7, 7)[0]]
    base = EC.seven_point(q[None], EC.null_gj)[0][0, root]
    routes = [(q, EC.null_svd)] + [(q[o], nl) for o in ORDERS for nl in (EC.null_gj, EC.null_svd)]
    out = []
    for qq, nl in routes:
        Fs, nr = EC.seven_point(qq[None], nl)
        if nr[0] != nroots:
            return None
        out.append(EC.f_err(base, Fs[0, root]))
    saved = EC.cubic_roots
    EC.cubic_roots = cubic_roots_ld
    try:
        Fs, nr = EC.seven_point(q[None], EC.null_gj)
    finally:
        EC.cubic_roots = saved
    if nr[0] != nroots:
        return None
    return max(out + [EC.f_err(base, Fs[0, root])])


def fund_oracle(rec, p):
    """the restated verifier on one seven-tuple as pair p, by both null-space routines -> (svd, gj, spread, ok):
    ok when both reach 7 inliers at TH_MIN with the same winner and every route of fund_spread finds as many roots"""
    kp1, kp2, match = minimal_pair(rec)
    a = EC.epipolar_pair(kp1, kp2, match, p, TH_MIN, 1, 0, RUN_SEED, EC.null_svd)
    b = EC.epipolar_pair(kp1, kp2, match, p, TH_MIN, 1, 0, RUN_SEED, EC.null_gj)
    ok = a["inliers"] == b["inliers"] == 7 and a["root"] == b["root"] and a["nroots"][0] == b["nroots"][0]
    spread = fund_spread(rec, p, b["root"], b["nroots"][0]) if ok else None
    return a, b, spread, ok and spread is not None


@functools.lru_cache(maxsize=None)
def fund_tuples():
    """PER_KIND seven-tuples of each kind; tuple number p is pair p of the one call.  A tuple the oracle
    does not reach (see fund_oracle) is replaced by the next seed: none is left out.  -> (tuples, replaced)"""
    out, replaced = [], 0
    for k, kind in enumerate(KINDS):
        for i in range(PER_KIND):
            p = k * PER_KIND + i
            for attempt in range(TRIES):
                rec, R, t = scene(kind, 7, np.random.default_rng(SEED + 10007 * attempt + p))
                a, b, spread, ok = fund_oracle(rec, p)
                if ok:
                    break
                replaced += 1
            assert ok, "no seven-tuple of kind %s for pair %d" % (kind, p)
            rec.setflags(write=False)
            out.append(dict(kind=kind, rec=rec, R=R, t=t, svd=a, gj=b, nroots=int(b["nroots"][0]),
                            spread=spread, tol=max(100 * spread, 1e-12)))
    return out, replaced


# ---------------------------------------------------------------- four-point tuples
H_KINDS = ("planted",) + tuple("plane_" + k for k in KINDS) + ("collinear",)
H_PER_KIND = {"planted": 200, "collinear": 200, **{"plane_" + k: 100 for k in KINDS}}
TH_GATE = 1.0            # px: the threshold of gate_tuples()
GATE_TUPLES = 100
BAND = 4.0               # every determinant of the gate is outside (DET_EPS / BAND, DET_EPS * BAND)


def gate_dets(rec):
    """the eight determinants of the gate of rr.h step b: four triples on each side"""
    out = []
    for q in (rec[:, :2], rec[:, 2:]):
        out += [VC.tri(q[3], q[1], q[2]), VC.tri(q[0], q[3], q[2]), VC.tri(q[0], q[1], q[3]), VC.tri(q[0], q[1], q[2])]
    return np.abs(np.array(out))


def gate_clear(rec):
    d = gate_dets(rec)
    return bool(((d <= VC.DET_EPS / BAND) | (d >= VC.DET_EPS * BAND)).all())


def planted_four(r):
    Ht = VC.true_homography(r)
    for _ in range(TRIES):
        a = r.uniform([0, 0], [W, H_IMG], (16, 2))
        b = VC.transfer(Ht, a) + NOISE * r.standard_normal(a.shape)
        ok = VC.inside(b)
        if ok.sum() >= 4:
            return np.concatenate([a, b], 1)[ok][:4].astype(np.float32).astype(np.float64)
    raise RuntimeError("no four points inside both frames")


def collinear_four(r, accept, side):
    """three of the four points of `side` within 1e-3 px of a line; the determinant of the three is drawn
    log-uniformly above DET_EPS * BAND (accept) or below DET_EPS / BAND (an exact 0 among them).  The line
    runs along y ~ 1e-3, where float32 is dense enough (2^-33) to hold such a determinant with 500 px
    between the end points.  The other side holds four points in general position."""
    xa, xb = r.uniform(50, 400), r.uniform(600, 1000)
    s = r.uniform(0.3, 0.7)
    ya, yb = r.uniform(1e-3, 2e-3, 2)
    if accept:
        det = 10.0 ** r.uniform(np.log10(VC.DET_EPS * BAND) + 0.05, -1.0)
    else:
        det = 0.0 if r.uniform() < 0.1 else 10.0 ** r.uniform(-10.0, np.log10(VC.DET_EPS / BAND) - 0.05)
    if det == 0.0:
        yb = ya          # a horizontal line: exactly collinear in float32 too
    yc = ya + s * (yb - ya) + r.choice([-1, 1]) * det / (xb - xa)
    line = np.array([[xa, ya], [xb, yb], [xa + s * (xb - xa), yc], [r.uniform(0, W), r.uniform(100, H_IMG)]])
    line = line[r.permutation(4)]
    while True:
        other = r.uniform([0, 0], [W, H_IMG], (4, 2))
        q = other.astype(np.float32).astype(np.float64)
        if min(abs(VC.tri(q[3], q[1], q[2])), abs(VC.tri(q[0], q[3], q[2])), abs(VC.tri(q[0], q[1], q[3])), abs(VC.tri(q[0], q[1], q[2]))) > 1e4:
            break
    rec = np.concatenate([line, other] if side == 0 else [other, line], 1)
    return rec.astype(np.float32).astype(np.float64)


def homog_oracle(rec, p, th=TH_MIN):
    kp1, kp2, match = minimal_pair(rec)
    return VC.verify_pair(kp1, kp2, match, p, th, 1, 0, RUN_SEED)


@functools.lru_cache(maxsize=None)
def homog_tuples():
    """the four-tuples of every kind of H_KINDS; tuple number p is pair p of the one call.  Every tuple has
    its gate determinants clear of the band; an accepted one the oracle's own 8 x 8 solve does not fit
    within TH_MIN / ENGINE_FACTOR is replaced by the next seed (mapping three nearly collinear points to
    points in general position is so ill-conditioned that np.linalg.solve misses 1e-6 px on about half of
    the draws; what the oracle cannot reach is not asked of the engine).  -> (tuples, replaced)"""
    out, replaced = [], 0
    for kind in H_KINDS:
        for i in range(H_PER_KIND[kind]):
            p = len(out)
            for attempt in range(TRIES):
                r = np.random.default_rng(SEED + 500000 + 10007 * attempt + p)
                accept = True
                if kind == "planted":
                    rec = planted_four(r)
                elif kind == "collinear":
                    accept = i % 2 == 0     # accepted: the three on side 1 (see gate_tuples); rejected: either side
                    rec = collinear_four(r, accept, 0 if accept else (i // 2) % 2)
                else:
                    rec = scene(kind[6:], 4, r, plane=True)[0]
                o = homog_oracle(rec, p)
                d = gate_dets(rec)
                ok = gate_clear(rec) and (d.min() >= VC.DET_EPS * BAND) == accept and o["inliers"] == (4 if accept else 0)
                if ok and accept:   # the oracle's own fit leaves the engine ENGINE_FACTOR times its error below TH_MIN
                    ok = VC.residuals(o["H"], rec)[1].max() <= TH_MIN / ENGINE_FACTOR
                if ok:
                    break
                replaced += 1
            assert ok, "no four-tuple of kind %s for pair %d" % (kind, p)
            rec.setflags(write=False)
            out.append(dict(kind=kind, rec=rec, accept=accept, oracle=o, det=float(d.min())))
    return out, replaced


@functools.lru_cache(maxsize=None)
def gate_tuples():
    """GATE_TUPLES four-tuples whose near-collinear three sit on side 2, their determinant above the gate: H then maps
    points in general position onto a near-line and is close to singular, the oracle's own solve misses 1e-6 px
    on nearly every draw (none of 94 with a determinant below 1e-4 reached it), so these are run at TH_GATE = 1 px,
    where the oracle fits within TH_GATE / ENGINE_FACTOR (it does from a determinant of about 3e-5 upwards; below
    that |w| <= 1e-8 or the transfer error exceeds even this).  They show that the gate on side 2 lets small
    determinants above RR_VERIFY_DET_EPS pass; the rejected tuples of homog_tuples() show that it stops those
    below.  -> (tuples, replaced)"""
    out, replaced = [], 0
    for p in range(GATE_TUPLES):
        for attempt in range(TRIES):
            rec = collinear_four(np.random.default_rng(SEED + 700000 + 10007 * attempt + p), True, 1)
            o, d = homog_oracle(rec, p, TH_GATE), gate_dets(rec)
            ok = gate_clear(rec) and d.min() >= VC.DET_EPS * BAND and o["inliers"] == 4 \
                and VC.residuals(o["H"], rec)[1].max() <= TH_GATE / ENGINE_FACTOR
            if ok:
                break
            replaced += 1
        assert ok, "no gate tuple for pair %d" % p
        rec.setflags(write=False)
        out.append(dict(kind="collinear_side2", rec=rec, accept=True, oracle=o, det=float(d.min())))
    return out, replaced


# ---------------------------------------------------------------- essential matrices
ANGLES = (0.0, 1e-8, 1e-3, 1.0, np.pi - 1e-3, np.pi)
SCALES = (1e-6, 1.0, 1e6)
T_KINDS = ("x", "y", "z", "axis", "random")
AXES_PER_ANGLE = 3
NEAR_FOCALS = (500.0, 5000.0)
NEAR_PER_KIND = 25


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def rodrigues(axis, ang):
    k = skew(axis / np.linalg.norm(axis))
    return np.eye(3) + np.sin(ang) * k + (1 - np.cos(ang)) * (k @ k)


@functools.lru_cache(maxsize=None)
def essential_cases():
    """-> list of dict(group, E, R, t): group "exact" is s [t]x R of a known motion (R, unit t); group "near" is
    K'^T F K' of a fund_tuples() scene under a wrong focal length: two unequal non-zero singular values, no
    true motion to compare with."""
    r = np.random.default_rng(SEED + 3)
    out = []
    for ang in ANGLES:
        for _ in range(AXES_PER_ANGLE):
            axis = r.standard_normal(3)
            axis /= np.linalg.norm(axis)
            R = rodrigues(axis, ang)
            for tk in T_KINDS:
                t = dict(x=np.array([1.0, 0, 0]), y=np.array([0, 1.0, 0]), z=np.array([0, 0, 1.0]), axis=axis)[tk] if tk != "random" \
                    else r.standard_normal(3)
                t = t / np.linalg.norm(t)
                for s in SCALES:
                    out.append(dict(group="exact", E=s * skew(t) @ R, R=R, t=t, what="angle %g t %s scale %g" % (ang, tk, s)))
    tuples = fund_tuples()[0]
    for k in range(len(KINDS)):
        for i in range(NEAR_PER_KIND):
            tp = tuples[k * PER_KIND + i]
            F = EC.true_fundamental(tp["R"], tp["t"])
            for f in NEAR_FOCALS:
                Kf = np.array([[f, 0.0, W / 2], [0.0, f, H_IMG / 2], [0.0, 0.0, 1.0]])
                out.append(dict(group="near", E=Kf.T @ F @ Kf, R=None, t=None, what="%s %d f %g" % (tp["kind"], i, f)))
    return out


def refused_essentials():
    """matrices rr.h says give zeros: all zero, an entry not finite, and rank one (exactly: E^T E is diagonal
    and E v1 is an exact zero; a rank-one matrix in general position has |a1| at rounding level, not 0)"""
    out = [np.zeros((3, 3))]
    for bad in (np.nan, np.inf, -np.inf):
        E = skew(np.array([0.3, -0.5, 0.8])) @ rodrigues(np.array([1.0, 2.0, 3.0]), 0.7)
        E[1, 2] = bad
        out.append(E)
    for i in range(3):
        for j in range(3):
            E = np.zeros((3, 3))
            E[i, j] = (-2.5, 1.0, 3e6)[(i + j) % 3]
            out.append(E)
    out.append(np.outer([1.0, 2.0, 0.0], [0.0, 0.0, 4.0]))
    return np.stack(out)


QUANTITIES = ("orth", "det", "tnorm", "tE", "rot_deg", "dir_deg")


def decompose_errors(R1, R2, t, case):
    """the quantities of the decomposition tests for one case -> dict (rot_deg / dir_deg only with a true motion)"""
    E = case["E"]
    e = dict(orth=max(np.abs(R.T @ R - np.eye(3)).max() for R in (R1, R2)),
             det=max(abs(np.linalg.det(R) - 1) for R in (R1, R2)),
             tnorm=abs(np.linalg.norm(t) - 1), tE=np.linalg.norm(t @ E) / np.linalg.norm(E))
    if case["R"] is not None:
        e["rot_deg"] = min(PC.rot_angle_deg(R1, case["R"]), PC.rot_angle_deg(R2, case["R"]))
        e["dir_deg"] = min(PC.dir_angle_deg(t, case["t"]), PC.dir_angle_deg(-t, case["t"]))
    return e


def worst_errors(results):
    """results: (R1, R2, t) per case of essential_cases() -> {group: {quantity: worst}}"""
    worst = {}
    for case, (R1, R2, t) in zip(essential_cases(), results):
        w = worst.setdefault(case["group"], {})
        for q, v in decompose_errors(R1, R2, t, case).items():
            w[q] = max(w.get(q, 0.0), float(v))
    return worst


def oracle_decompositions():
    out = []
    for case in essential_cases():
        Ra, Rb, t, _ = PC.decompose(case["E"])
        out.append((Ra, Rb, t))
    return out


# The worst error of pose_cases.decompose (np.linalg.svd) per quantity on essential_cases(), as printed by
# `python tests/hard_geometry_cases.py`; test_host_hard_geometry.py asserts that the oracle still stays within
# them.  The engine gets ENGINE_FACTOR times each, floor ENGINE_FLOOR.
ORACLE_WORST = {
    "exact": dict(orth=1.3322676295501878e-15, det=1.4432899320127035e-15, tnorm=2.220446049250313e-16, tE=1.2790144318896504e-16,
                  rot_deg=2.091309789151873e-06, dir_deg=1.2074182697257333e-06),
    "near": dict(orth=1.6653345369377348e-15, det=1.5543122344752192e-15, tnorm=3.3306690738754696e-16, tE=2.097866609760607e-16),
}
ENGINE_FACTOR, ENGINE_FLOOR = 16.0, 1e-12


def engine_bound(group, q):
    return max(ENGINE_FACTOR * ORACLE_WORST[group][q], ENGINE_FLOOR)


# ---------------------------------------------------------------- triangulation
TRI_FOCALS = (500.0, 900.0, 5000.0)
TRI_RATIOS = (5.0, 50.0, 5e3, 5e5)      # depth over baseline
TRI_SIZES = (1, 255, 256, 257)          # points per set: around one pass of the block
TRI_W, TRI_H = 4000.0, 3000.0
W_CLEAR = 100 * PC.W_EPS                # the oracle's |w| of every kept point: the de-homogenisation branch is the same everywhere
X_RATIO = 50.0                          # X itself is compared up to this depth over baseline
X_RTOL = 1e-9                           # of |X|: a singular vector is accurate normwise, a coordinate near 0 has no digits of its own


def tri_design(P1, P2, rec):
    """the 4 x 4 of rr.h step d per record [M, 4, 4]"""
    x1, y1, x2, y2 = rec.T
    return np.stack([x1[:, None] * P1[2] - P1[0], y1[:, None] * P1[2] - P1[1], x2[:, None] * P2[2] - P2[0],
                     y2[:, None] * P2[2] - P2[1]], 1)


@functools.lru_cache(maxsize=None)
def tri_sets():
    """one camera pair per (focal, ratio), len(TRI_SIZES) point sets under each -> list of dict(f, ratio, P1, P2,
    rec [n, 4] float64, X, w): the baseline is 1, the depths ratio x (0.8 .. 1.2), NOISE px on side 2, image
    coordinates up to TRI_W x TRI_H, and the oracle's |w| >= W_CLEAR on every point"""
    r = np.random.default_rng(SEED + 5)
    out = []
    for f in TRI_FOCALS:
        K = np.array([[f, 0.0, TRI_W / 2], [0.0, f, TRI_H / 2], [0.0, 0.0, 1.0]])
        for ratio in TRI_RATIOS:
            R = EC.rot(*r.uniform(-0.1, 0.1, 3))
            t = np.array([r.choice([-1, 1]) * 1.0, r.uniform(-0.3, 0.3), r.uniform(-0.3, 0.3)])
            t /= np.linalg.norm(t)
            P1, P2 = PC.projection(K, np.eye(3), np.zeros(3)), PC.projection(K, R, t)
            for n in TRI_SIZES:
                rec = np.empty((0, 4))
                for _ in range(TRIES):
                    px = r.uniform([0, 0], [TRI_W, TRI_H], (4 * n + 16, 2))
                    z = ratio * r.uniform(0.8, 1.2, len(px))
                    X = np.concatenate([(px - K[:2, 2]) / f, np.ones((len(px), 1))], 1) * z[:, None]
                    q = (X @ R.T + t) @ K.T
                    q2 = q[:, :2] / q[:, 2:] + NOISE * r.standard_normal((len(px), 2))
                    cand = np.concatenate([px, q2], 1)
                    ok = (q[:, 2] > 0.5) & (q2[:, 0] >= 0) & (q2[:, 0] < TRI_W) & (q2[:, 1] >= 0) & (q2[:, 1] < TRI_H)
                    ok &= np.abs(PC.triangulate(P1, P2, cand)[1]) >= W_CLEAR
                    rec = np.concatenate([rec, cand[ok]])
                    if len(rec) >= n:
                        break
                assert len(rec) >= n, (f, ratio, n)
                rec = rec[:n]
                Xo, w = PC.triangulate(P1, P2, rec)
                for a in (rec, Xo, w):
                    a.setflags(write=False)
                out.append(dict(f=f, ratio=ratio, P1=P1, P2=P2, rec=rec, X=Xo, w=w))
    return out


def tri_residuals(s, X):
    """per point of set s under the points X [n, 3]: (|A h|, sigma_min(A), |A|_2) with h = (X, 1) normalised"""
    A = tri_design(s["P1"], s["P2"], s["rec"])
    h = np.concatenate([X, np.ones((len(X), 1))], 1)
    h /= np.linalg.norm(h, axis=1, keepdims=True)
    sv = np.linalg.svd(A, compute_uv=False)
    return np.linalg.norm(np.einsum("nij,nj->ni", A, h), axis=1), sv[:, -1], sv[:, 0]


def tri_residual_ok(res, smin, nrm):
    """rr.h step d reached the smallest singular vector: |A h| <= sigma_min (1 + 1e-6) + 1e-12 |A|; the 1e-6
    allows for X / w having been rounded once"""
    return res <= smin * (1 + 1e-6) + 1e-12 * nrm


if __name__ == "__main__":
    tuples, replaced = fund_tuples()
    print("seven-tuples: %d, replaced %d, three roots %d" % (len(tuples), replaced, sum(t["nroots"] == 3 for t in tuples)))
    print("  largest tol", max(t["tol"] for t in tuples))
    ht, hrep = homog_tuples()
    print("four-tuples: %d, replaced %d, accepted %d" % (len(ht), hrep, sum(t["accept"] for t in ht)))
    gt, grep = gate_tuples()
    print("gate tuples: %d, replaced %d, determinants %.3g .. %.3g" % (len(gt), grep, min(t["det"] for t in gt), max(t["det"] for t in gt)))
    print("ORACLE_WORST =", worst_errors(oracle_decompositions()))
