"""Shared by tests/test_host_gridcap.py and tests/test_gpu_gridcap.py: batches of more pairs than the
65535-block cap of the one-block-per-pair kernels (rr_match.hip, rr_verify.hip, rr_epipolar.hip,
rr_pose.hip), so that blocks 0 .. TAIL - 1 walk their pair loop a second time.

A batch has P = CAP + TAIL pairs, pair p being distinct pair p % K of K = 7 small ones (CAP % 7 == 1: a
block's second pair is another one than its first).  The seven of every entry alternate the paths a
block can take from one pair to the next: an empty pair, a pair below the minimal sample, a pair of
exactly the minimal size, ordinary pairs of different sizes.  The RANSAC verifiers, whose sample depends on
p, also get an eighth pair of STAGE + 1 matches (read from global memory, not staged in LDS) at a few
chosen indices, and are compared with the float64 oracle at each pair's own p.

The oracles are those of match_cases / verify_cases / epipolar_cases / pose_cases; the second solvers
here (SVD of the design matrix, QR, eigh) exist to derive each tolerance by those modules' rule: 100 x the
difference of two float64 solvers on the same input, with the module's floor.  numpy only."""

import functools

import numpy as np

import epipolar_cases as EC
import match_cases as MC
import pose_cases as PC
import verify_cases as VC

CAP = 65535              # the most blocks a pair kernel launches
TAIL = 70                # blocks 0 .. TAIL - 1 run two pairs
K = 7
P = CAP + TAIL
SEED = 12000
ITERS, REFINE = 257, 2   # two chunks of hypotheses: the RANSAC kernels run a (2, CAP) grid
MARGIN = 1e-7            # the margin rule of the verifier fixtures (make_golden_verify / make_golden_epipolar)
# the unstaged pair: at a, b and their block-mates a + CAP, b + CAP (unstaged twice in one block), at c
# alone (unstaged, then a staged or skipped pair) and at d + CAP alone (staged or skipped, then unstaged)
SPECIAL = (5, 40, 5 + CAP, 40 + CAP, 12, 23 + CAP)


def kinds(special=()):
    """the distinct pair of every pair p: p % K, and K (the eighth) at the special indices"""
    kind = np.arange(P, dtype=np.int64) % K
    kind[list(special)] = K
    return kind


def compared():
    """the pairs whose results are compared with the oracle: every p >= CAP and its block-mate p - CAP"""
    return np.concatenate([np.arange(TAIL), np.arange(CAP, P)])


def offsets(lens):
    return np.cumsum([0] + list(lens)).astype(np.int64)


def freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------- matching
D = 8
MATCH_TH = 0.9
# (N1, N2): empty side 1; N2 = 0 (nothing to match); N1 below one 16-row tile; N1 above one; N1 above a 32-row tile;
# N2 above one; one row against one row (no second neighbour)
MATCH_PAIRS = [(0, 5), (6, 0), (4, 9), (17, 12), (40, 23), (23, 40), (1, 1)]
MATCH_MAX = 40


@functools.lru_cache(maxsize=None)
def match_seven():
    """-> list of (a [n1, D], b [n2, D]) float32"""
    return [freeze(*MC.descriptors(n1, n2, D, SEED + 17 * k)) for k, (n1, n2) in enumerate(MATCH_PAIRS)]


# ---------------------------------------------------------------- batched fits
H_SIZES = [4, 9, 50, 0, 3, 13, 27]      # 4: the minimum; 0 and 3: all-zero H
F_SIZES = [8, 9, 50, 0, 7, 13, 27]      # 8: the minimum; 0 and 7: all-zero F


@functools.lru_cache(maxsize=None)
def dlt_seven():
    """-> list of (p1 [n, 2], p2 [n, 2], w [n]) float64, weighted"""
    out = []
    for k, n in enumerate(H_SIZES):
        p1, p2, w = VC.dlt_points(1, n, True, SEED + 100 + k)
        out.append(freeze(p1[0], p2[0], w[0]))
    return out


@functools.lru_cache(maxsize=None)
def fund_seven():
    out = []
    for k, n in enumerate(F_SIZES):
        p1, p2, w = EC.fund_points(1, n, True, SEED + 200 + k)
        out.append(freeze(p1[0], p2[0], w[0]))
    return out


def dlt_svd(p1, p2, w=None):
    """verify_cases.dlt by the SVD of the weighted design matrix instead of eigh of A^T W A"""
    p1, p2 = np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)
    q1, T1 = VC.normalize_points(p1)
    q2, T2 = VC.normalize_points(p2)
    x1, y1, x2, y2 = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    o, z = np.ones_like(x1), np.zeros_like(x1)
    ax = np.stack([z, z, z, -x1, -y1, -o, y2 * x1, y2 * y1, y2], 1)
    ay = np.stack([x1, y1, o, z, z, z, -x2 * x1, -x2 * y1, -x2], 1)
    A = np.stack([ax, ay], 1).reshape(-1, 9)
    ww = np.ones(len(p1)) if w is None else np.asarray(w, dtype=np.float64)
    A = np.concatenate([A * np.sqrt(np.repeat(ww, 2))[:, None], np.zeros((max(0, 9 - len(A)), 9))])
    h = np.linalg.svd(A)[2][-1]
    Hm = np.linalg.inv(T2) @ (h.reshape(3, 3) @ T1)
    return Hm / (Hm[2, 2] + VC.EPS)


def fundamental_svd(p1, p2, w=None):
    """epipolar_cases.fundamental by the SVD of the weighted design matrix and the SVD rank-2 projection"""
    p1, p2 = np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)
    if len(p1) < 8:
        return np.zeros((3, 3))
    q1, T1 = EC.normalize_points(p1)
    q2, T2 = EC.normalize_points(p2)
    ww = np.ones(len(p1)) if w is None else np.asarray(w, dtype=np.float64)
    X = EC.design(q1, q2) * np.sqrt(ww)[:, None]
    X = np.concatenate([X, np.zeros((max(0, 9 - len(X)), 9))])
    f = np.linalg.svd(X)[2][-1].reshape(3, 3)
    U, s, Vt = np.linalg.svd(f)
    f = U @ np.diag([s[0], s[1], 0.0]) @ Vt
    F = T2.T @ f @ T1
    return F / (F[2, 2] + EC.EPS) if abs(F[2, 2]) > EC.EPS else F


def dlt_tol(p1, p2, w):
    """corner transfer px: 100 x (eigh route vs SVD route), floor 1e-9 (the rule of verify.npz)"""
    return max(100 * VC.corner_err(VC.dlt(p1, p2, w), dlt_svd(p1, p2, w)), 1e-9)


def fund_tol(p1, p2, w):
    """f_err: 100 x (eigh route vs SVD route), floor 1e-12 (the rule of epipolar.npz)"""
    return max(100 * EC.f_err(EC.fundamental(p1, p2, w), fundamental_svd(p1, p2, w)), 1e-12)


# ---------------------------------------------------------------- distances
DIST_KINDS = (("sampson", True), ("sampson", False), ("symmetrical", True), ("symmetrical", False))


@functools.lru_cache(maxsize=None)
def dist_seven():
    """the point sets of fund_seven() with an F per set: the set's own weighted fit, or (fewer than 8 points)
    the fit of the 50-point set -> list of (p1, p2, F)"""
    sets = fund_seven()
    big = EC.fundamental(*sets[2])
    return [freeze(p1, p2, EC.fundamental(p1, p2, w) if len(p1) >= 8 else big.copy()) for p1, p2, w in sets]


def dist_tol(p1, p2, F, kind, squared):
    """relative to the set's largest distance: 100 x (float64 vs extended precision), floor 1e-12"""
    if len(p1) == 0:
        return 1e-12
    ld = np.longdouble
    a, b = EC.distance(p1, p2, F, kind, squared), EC.distance(p1.astype(ld), p2.astype(ld), F.astype(ld), kind, squared, ld(1e-8))
    return max(100 * float(np.abs(a - b).max() / np.abs(b).max()), 1e-12)


# ---------------------------------------------------------------- triangulation
TRI_SIZES = [0, 1, 4, 8, 23, 40, 17]


@functools.lru_cache(maxsize=None)
def tri_seven():
    """-> list of dict(rec [n, 4] float64, P1, P2 [3, 4], scale): the planted matches of a pose_cases scene under its
    true motion; scale: the median depth of its points"""
    out = []
    for k, n in enumerate(TRI_SIZES):
        s = PC.scene(n, n, n, 1.0, 0.3, SEED + 300 + k)
        rows, rec = PC.records(s)
        P1, P2 = PC.projection(s["K1"], np.eye(3), np.zeros(3)), PC.projection(s["K2"], s["R"], s["t"])
        out.append(dict(rec=rec, P1=P1, P2=P2, scale=PC.median_depth(s["X"][rows])))
        freeze(rec, P1, P2)
    return out


def triangulate_qr(P1, P2, rec):
    """pose_cases.triangulate by another route: the SVD of the R factor of a QR factorisation of the 4 x 4"""
    if len(rec) == 0:
        return np.zeros((0, 3)), np.zeros(0)
    x1, y1, x2, y2 = rec.T
    A = np.stack([x1[:, None] * P1[2] - P1[0], y1[:, None] * P1[2] - P1[1], x2[:, None] * P2[2] - P2[0],
                  y2[:, None] * P2[2] - P2[1]], 1)
    h = np.stack([np.linalg.svd(np.linalg.qr(a)[1])[2][-1] for a in A])
    w = h[:, 3]
    s = np.where(np.abs(w) > PC.W_EPS, 1.0 / np.where(np.abs(w) > PC.W_EPS, w, 1.0), 1.0)
    return h[:, :3] * s[:, None], w


def tri_tol(t):
    """largest coordinate difference over the median depth: 100 x (SVD route vs QR route), floor 1e-12"""
    if len(t["rec"]) == 0:
        return 1e-12
    a, b = PC.triangulate(t["P1"], t["P2"], t["rec"])[0], triangulate_qr(t["P1"], t["P2"], t["rec"])[0]
    return max(100 * np.abs(a - b).max() / t["scale"], 1e-12)


# ---------------------------------------------------------------- pose
# (name, (n1, n2, m, planted fraction, noise), second camera other than the first)
POSE_PAIRS = [("empty", (0, 0, 0, 0.0, 0.3), False), ("zeroF", (30, 28, 20, 1.0, 0.3), False), ("unused", (23, 20, 12, 1.0, 0.3), False),
              ("k2_8", (9, 12, 8, 1.0, 0.3), True), ("k1_30", (40, 35, 30, 1.0, 0.3), False), ("k2_17", (23, 29, 17, 1.0, 0.3), True),
              ("masked", (16, 11, 9, 1.0, 0.3), False)]


def decompose_eigh(E0):
    """pose_cases.decompose with the right singular vectors from np.linalg.eigh(E0^T E0) instead of np.linalg.svd"""
    if not np.isfinite(E0).all() or not E0.any():
        return None
    V = np.linalg.eigh(E0.T @ E0)[1]
    v0, v1 = V[:, 2], V[:, 1]
    a0, a1 = E0 @ v0, E0 @ v1
    s0, s1 = np.linalg.norm(a0), np.linalg.norm(a1)
    if not np.isfinite(s0) or not s1 > 0:
        return None
    u0 = a0 / s0
    b = a1 - (u0 @ a1) * u0
    if not np.linalg.norm(b) > 0:
        return None
    u1 = b / np.linalg.norm(b)
    u2, v2 = np.cross(u0, u1), np.cross(v0, v1)
    Ra = np.outer(u1, v0) - np.outer(u0, v1) + np.outer(u2, v2)
    Rb = np.outer(u0, v1) - np.outer(u1, v0) + np.outer(u2, v2)
    return Ra, Rb, u2, np.outer(u0, v0) + np.outer(u1, v1)


def pose_pair_second(*args):
    """pose_cases.pose_pair through the two other solvers above (the candidate order may differ; the winner does not)"""
    saved = PC.decompose, PC.triangulate
    PC.decompose, PC.triangulate = decompose_eigh, triangulate_qr
    try:
        return PC.pose_pair(*args)
    finally:
        PC.decompose, PC.triangulate = saved


@functools.lru_cache(maxsize=None)
def pose_seven():
    """-> list of dict(name, scene, F, mask, K1, K2, want (pose_cases.pose_pair), tol (R, t, X), scale)"""
    out = []
    for k, (name, spec, other) in enumerate(POSE_PAIRS):
        s = PC.scene(*spec, SEED + 400 + 17 * k, PC.K2_OTHER if other else None)
        F = np.zeros((3, 3)) if name == "zeroF" else EC.unit(s["F"])
        mask = np.ones(len(s["kp1"]), dtype=bool)
        if name == "unused":
            mask[:] = False
        if name == "masked":
            mask[np.nonzero(s["match"] >= 0)[0][::3]] = False
        args = (s["kp1"], s["kp2"], s["match"], mask, F, s["K1"], s["K2"])
        want, alt = PC.pose_pair(*args), pose_pair_second(*args)
        rows = want["rows"]
        scale = PC.median_depth(s["X"][rows]) if len(rows) else 1.0
        tol = tuple(max(100 * float(np.abs(want[q] - alt[q]).max()) / sc, 1e-12) if want[q].size else 1e-12
                    for q, sc in (("R", 1.0), ("t", 1.0), ("points3d", scale)))
        freeze(F, mask, *[v for v in s.values() if isinstance(v, np.ndarray)])
        out.append(dict(name=name, scene=s, F=F, mask=mask, K1=s["K1"], K2=s["K2"], want=want, alt=alt, tol=tol, scale=scale))
    return out


# ---------------------------------------------------------------- essential decomposition past the cap
DEC_DISTINCT = 11
DEC_N = CAP * 256 + 1000      # one thread per matrix, 256 per block: the blocks stride from matrix CAP * 256 on


@functools.lru_cache(maxsize=None)
def essential_eleven():
    """eleven matrices: six exact essential matrices (rotations by 0.3 .. 3 rad, scales 1e-3 .. 1e3), two with unequal
    singular values, a zero, one with a NaN and an exactly rank-one one (the last three: zeros out)"""
    r = np.random.default_rng(SEED + 500)
    out = []
    for i in range(8):
        axis = r.standard_normal(3)
        k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]]) / np.linalg.norm(axis)
        ang = (0.3, 0.9, 1.5, 2.1, 2.7, 3.0, 0.5, 1.1)[i]
        R = np.eye(3) + np.sin(ang) * k + (1 - np.cos(ang)) * (k @ k)
        t = r.standard_normal(3)
        E = 10.0 ** (i % 3 * 3 - 3) * np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
        if i >= 6:
            E = np.diag([1.0, 1.0, 1.7]) @ E @ np.diag([0.6, 1.0, 1.0])
        out.append(E)
    bad = out[0].copy()
    bad[2, 1] = np.nan
    out += [np.zeros((3, 3)), bad, np.outer([0.0, 2.0, 0.0], [0.0, 0.0, 3.0])]
    assert len(out) == DEC_DISTINCT
    return freeze(np.stack(out))[0]


def decompose_diff(a, b):
    """two decompositions (Ra, Rb, t): the largest entry difference with {Ra, Rb} matched in either order and t up to sign"""
    same = max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())
    swap = max(np.abs(a[0] - b[1]).max(), np.abs(a[1] - b[0]).max())
    return max(min(same, swap), min(np.abs(a[2] - b[2]).max(), np.abs(a[2] + b[2]).max()))


def decompose_tol(E):
    """100 x (np.linalg.svd route vs eigh route), floor 1e-12"""
    return max(100 * decompose_diff(PC.decompose(E), decompose_eigh(E)), 1e-12)


# ---------------------------------------------------------------- the RANSAC verifiers
# (n1, n2, kept matches, planted fraction, noise px): empty; below the minimal sample; exactly minimal; just above;
# two ordinary pairs; no kept match -- and the eighth, STAGE + 1 matches
H_PAIRS = [(0, 0, 0, 0.0, 0.5), (20, 25, 3, 1.0, 0.5), (9, 12, 4, 1.0, 0.5), (16, 11, 8, 0.8, 0.5), (40, 35, 30, 0.6, 0.5),
           (23, 29, 17, 0.7, 0.5), (30, 28, 0, 0.0, 0.5), (1100, 1060, VC.STAGE + 1, 0.5, 0.5)]
F_PAIRS = [(0, 0, 0, 0.0, 0.3), (20, 25, 6, 1.0, 0.3), (12, 14, 7, 1.0, 0.3), (12, 11, 8, 1.0, 0.3), (40, 35, 30, 0.7, 0.3),
           (23, 29, 17, 0.8, 0.3), (30, 28, 0, 0.0, 0.3), (1100, 1060, EC.STAGE + 1, 0.6, 0.3)]
MINIMAL = {"homography": 4, "fundamental": 7}
VERIFY_SEEDS = {"homography": SEED + 600, "fundamental": SEED + 700}


@functools.lru_cache(maxsize=None)
def verify_eight(model):
    """the eight distinct pairs of a verifier -> list of (kp1 f32, kp2 f32, match int64)"""
    mod, specs = (VC, H_PAIRS) if model == "homography" else (EC, F_PAIRS)
    return [freeze(*mod.planted_pair(*spec, VERIFY_SEEDS[model] + 17 * k)[:3]) for k, spec in enumerate(specs)]


def kept(match, n2):
    return int(((match >= 0) & (match < n2)).sum())


def h_pair_tol(info):
    """make_golden_verify.pair_tol with the SVD route in place of the reference's"""
    fit = info["fit"]
    if fit is None:
        return 1e-9
    Hs = dlt_svd(fit[:, :2], fit[:, 2:])
    d = VC.corner_err(VC.dlt(fit[:, :2], fit[:, 2:]), Hs)
    if len(fit) == 4:
        d = max(d, VC.corner_err(VC.four_point(fit[:, :2], fit[:, 2:]), Hs))
    return max(100 * d, 1e-9)


def f_pair_tol(a, b):
    """make_golden_epipolar.pair_tol with the SVD route in place of the reference's (a: null_svd, b: null_gj)"""
    fit = a["fit"]
    if fit is None:
        return 1e-12
    if len(fit) >= 8:
        d = EC.f_err(EC.fundamental(fit[:, :2], fit[:, 2:]), fundamental_svd(fit[:, :2], fit[:, 2:]))
    else:
        d = EC.f_err(a["F"], b["F"])
    return max(100 * d, 1e-12)


@functools.lru_cache(maxsize=None)
def verify_oracle(model):
    """the float64 oracle at the pair's own p for every compared pair -> {p: dict(info, tol, kind[, gj])}"""
    eight, kind = verify_eight(model), kinds(SPECIAL)
    out = {}
    for p in compared():
        kp1, kp2, match = eight[kind[p]]
        if model == "homography":
            o = VC.verify_pair(kp1, kp2, match, int(p), VC.TH, ITERS, REFINE, VC.RUN_SEED)
            out[int(p)] = dict(info=o, tol=h_pair_tol(o), kind=int(kind[p]))
        else:
            a = EC.epipolar_pair(kp1, kp2, match, int(p), EC.TH, ITERS, REFINE, EC.RUN_SEED, EC.null_svd)
            b = EC.epipolar_pair(kp1, kp2, match, int(p), EC.TH, ITERS, REFINE, EC.RUN_SEED, EC.null_gj)
            out[int(p)] = dict(info=a, gj=b, tol=f_pair_tol(a, b), kind=int(kind[p]))
    return out
