"""Shared by tests/golden/make_golden_pnp.py and the localization tests: planted 2-D to 3-D scenes (the
camera, image size and noise of epipolar_cases / pose_cases) and a float64 numpy restatement of
rr_localize_pairs (steps a - e of include/rr.h) and rr_p3p, written from the header, with two
independent routes:
  A  the header's construction: Grunert's quartic in v = s3 / s1 with np.roots, the pose from the frames
     the two triangles span, the refit by the normal equations (np.linalg.cholesky);
  B  the same three points with the roles of point 1 and point 3 exchanged, which gives another quartic
     (in 1 / v), the solutions sorted back by v, the pose by absolute orientation (Kabsch, np.linalg.svd),
     the refit by np.linalg.lstsq on the stacked Jacobian and another form of Rodrigues' formula.
The upstream project has no absolute pose: nothing here is compared with it.  numpy only."""

import numpy as np

import epipolar_cases as EC
import pose_cases as PC

K = EC.K
K_OTHER = PC.K2_OTHER
TH = 3.0
NOISE = 0.3
RUN_SEED = EC.RUN_SEED
STAGE = EC.STAGE
PNP_SEED = 9300
GN_STEPS = 3          # RR_PNP_GN_STEPS
SMALL2 = 1e-8         # RR_PNP_SMALL_ANGLE2
NEAR = 1e-4           # a sample with two roots this close (relative) to each other or to the real axis is dropped
REAL = 1e-9           # |imag| <= REAL max(1, |v|): a real root

# pairs: (n1, n2, kept matches M, planted fraction, noise px, kind); th 3.0 px everywhere
PNP_CASES = [
    dict(name="m0", pairs=[(20, 25, 0, 0.0, NOISE, "general")], iters=256, refine=2),
    dict(name="m2", pairs=[(20, 25, 2, 1.0, NOISE, "general")], iters=256, refine=2),
    dict(name="m3", pairs=[(12, 14, 3, 1.0, NOISE, "general")], iters=256, refine=2),
    dict(name="m4", pairs=[(12, 11, 4, 1.0, NOISE, "general")], iters=256, refine=2),
    dict(name="m40", pairs=[(70, 64, 40, 0.6, NOISE, "general")], iters=300, refine=2),
    dict(name="m257_r0", pairs=[(300, 310, 257, 0.6, NOISE, "general")], iters=300, refine=0),
    dict(name="m257_r2", pairs=[(300, 310, 257, 0.6, NOISE, "general")], iters=256, refine=2),
    dict(name="m1025", pairs=[(1100, 1060, STAGE + 1, 0.6, NOISE, "general")], iters=256, refine=2),
    dict(name="iters1", pairs=[(70, 64, 40, 1.0, NOISE, "general")], iters=1, refine=2),
    dict(name="iters257", pairs=[(70, 64, 40, 0.6, NOISE, "general")], iters=257, refine=2),
    dict(name="outliers", pairs=[(80, 90, 60, 0.0, NOISE, "general")], iters=300, refine=2),
    dict(name="ragged4", pairs=[(0, 0, 0, 0.0, NOISE, "general"), (30, 28, 2, 1.0, NOISE, "general"),
                                (80, 90, 60, 0.0, NOISE, "general"), (60, 70, 50, 1.0, NOISE, "general")], iters=300, refine=2),
    dict(name="valid", pairs=[(90, 80, 60, 0.6, NOISE, "valid")], iters=300, refine=2),
    dict(name="nan", pairs=[(70, 64, 40, 0.6, NOISE, "nan")], iters=300, refine=2),
    dict(name="behind", pairs=[(90, 80, 60, 0.9, NOISE, "behind")], iters=300, refine=2),
    dict(name="coplanar", pairs=[(90, 80, 60, 0.6, NOISE, "coplanar")], iters=300, refine=2),
    dict(name="singularK", pairs=[(70, 64, 40, 0.6, NOISE, "general"), (70, 64, 40, 0.6, NOISE, "singular"),
                                  (70, 64, 40, 0.6, NOISE, "general"), (60, 66, 30, 0.7, NOISE, "othercam")], iters=256, refine=2),
]
# the cases with extra checks in the tests
EXACT_CASE = dict(name="exact", pairs=[(60, 70, 50, 1.0, 0.0, "general")], iters=300, refine=2)
CHAIN_CASE = dict(name="chain", pairs=[(130, 120, 100, 0.6, NOISE, "chain")], iters=300, refine=2)
ALL_CASES = PNP_CASES + [EXACT_CASE, CHAIN_CASE]
CHAIN_VER = dict(th=EC.TH, iters=256, refine=2, seed=RUN_SEED)   # verify_pairs(model="fundamental") of the chain
CHAIN_Q = (140, 60, 0.7)      # the chain's query view: keypoints, rows matched to view a, planted fraction
SOLVER_N = 257        # samples of the minimal-solver test: a second block trip
SOLVER_SEED = 9500
CAM_SEED = 9600

checksum = EC.checksum


# ---------------------------------------------------------------- scenes
def random_motion(r):
    R = EC.rot(*r.uniform(-0.25, 0.25, 3))
    t = np.array([r.uniform(0.6, 1.2) * r.choice([-1, 1]), r.uniform(-0.3, 0.3), r.uniform(-0.5, 0.5)])
    return R, t


def scene(n1, n2, m, frac, noise, kind, seed):
    """-> dict(kp [n1, 2] f32, X [n2, 3] f64 world points, valid bool [n2] or None, match int64 [n1], planted bool
    [n1], R, t (the camera: Xc = R X + t), K).  Every 3-D point lies at depth 4 .. 12 in front of the
    camera and projects into the 1024 x 768 frame.  m rows of side 1 are matched to distinct rows of side
    2; round(frac m) of them are the projection of their point plus Gaussian noise, the others uniform.
      "coplanar"  every point on the oblique plane n . Xc = 8, n = (0.2, -0.1, 1)
      "valid"     `valid` knocks out a third of the matched points (planted ones among them)
      "nan"       one planted point has a NaN coordinate
      "behind"    a third of the planted points are mirrored behind the camera (Xc -> -Xc, which the pinhole
                  formula sends to the same pixel); their 2-D rows are left as random outliers
      "othercam"  the camera is K_OTHER;  "singular"  K has two equal rows"""
    r = np.random.default_rng(seed)
    Km = K_OTHER.copy() if kind == "othercam" else K.copy()
    R, t = random_motion(r)
    px = r.uniform([0, 0], [EC.W - 1, EC.H_IMG - 1], (n2, 2))
    if noise == 0.0:
        px = np.round(px * 16) / 16        # exact in float32
    ray = np.concatenate([px, np.ones((n2, 1))], 1) @ np.linalg.inv(Km).T
    z = r.uniform(4.0, 12.0, n2)
    if kind == "coplanar":
        z = 8.0 / (ray @ np.array([0.2, -0.1, 1.0]))
    Xc = ray * z[:, None]
    kp = r.uniform([0, 0], [EC.W, EC.H_IMG], (n1, 2))
    match = np.full(n1, -1, dtype=np.int64)
    planted = np.zeros(n1, dtype=bool)
    rows = np.sort(r.permutation(n1)[:m])
    cols = r.permutation(n2)[:m]
    match[rows] = cols
    nin = int(round(frac * m))
    inl = r.permutation(m)[:nin]
    valid = None
    if kind == "behind":
        back = inl[:nin // 3]
        inl = inl[nin // 3:]
        Xc[cols[back]] *= -1.0
    planted[rows[inl]] = True
    kp[rows[inl]] = np.clip(px[cols[inl]] + noise * r.standard_normal((len(inl), 2)), 0, [EC.W - 0.01, EC.H_IMG - 0.01])
    X = (Xc - t) @ R                       # R^T (Xc - t)
    if kind == "valid":
        valid = np.ones(n2, dtype=bool)
        valid[cols[r.permutation(m)[:m // 3]]] = False
        planted &= valid[np.maximum(match, 0)]
    if kind == "nan":
        X[cols[inl[0]], int(r.integers(3))] = np.nan
        planted[rows[inl[0]]] = False
    if kind == "singular":
        Km = np.array([[900.0, 0.0, 512.0], [900.0, 0.0, 512.0], [0.0, 0.0, 1.0]])
    return dict(kp=kp.astype(np.float32), X=X, valid=valid, match=match, planted=planted, R=R, t=t, K=Km)


def chain_scene(n1, n2, m, frac, noise, seed):
    """three planted views: PC.scene gives views a and b (X in a's frame); the query view q sees a's points
    through (Rq, tq) and K_OTHER.  -> dict(ab = that scene, kq [nq, 2] f32, match_qa int64 [nq], planted_q,
    Rq, tq, Kq)"""
    ab = PC.scene(n1, n2, m, frac, noise, seed)
    r = np.random.default_rng(seed + 7)
    nq, mq, fq = CHAIN_Q
    while True:
        Rq, tq = random_motion(r)
        q = (ab["X"] @ Rq.T + tq) @ K_OTHER.T
        pq = q[:, :2] / q[:, 2:]
        if (EC.VC.inside(pq) & (q[:, 2] > 0.5)).mean() > 0.8:
            break
    kq = r.uniform([0, 0], [EC.W, EC.H_IMG], (nq, 2))
    match = np.full(nq, -1, dtype=np.int64)
    planted = np.zeros(nq, dtype=bool)
    # the query matches rows of a that a -> b matched and planted, so that their 3-D points exist
    good = np.nonzero(ab["planted"] & EC.VC.inside(pq) & (q[:, 2] > 0.5))[0]
    other = np.setdiff1d(np.arange(n1), good)
    nin = min(int(round(fq * mq)), len(good))
    cols = np.concatenate([r.permutation(good)[:nin], r.permutation(other)[:mq - nin]])
    rows = np.sort(r.permutation(nq)[:mq])
    match[rows] = cols
    planted[rows[:nin]] = True
    kq[rows[:nin]] = np.clip(pq[cols[:nin]] + noise * r.standard_normal((nin, 2)), 0, [EC.W - 0.01, EC.H_IMG - 0.01])
    return dict(ab=ab, kq=kq.astype(np.float32), match=match, planted=planted, Rq=Rq, tq=tq, Kq=K_OTHER.copy())


def chain_points(ch):
    """the oracle's views a -> b: verify (fundamental), recover_pose -> (X [n1, 3] in a's frame in units of
    |tab|, front_mask bool [n1], the verifier's and the pose's dicts)"""
    ab = ch["ab"]
    v = EC.epipolar_pair(ab["kp1"], ab["kp2"], ab["match"], 0, **CHAIN_VER)
    o = PC.pose_pair(ab["kp1"], ab["kp2"], ab["match"], v["mask"], v["F"], ab["K1"], ab["K2"])
    return o["points3d"], o["front_mask"], v, o


def build_case(case, seed):
    """the ragged batch of a case: kp [rows1, 2], off1 [P + 1], X [rows2, 3], valid bool [rows2] or None, off2,
    match [rows1], planted [rows1], K [P, 3, 3], scenes"""
    parts = []
    for k, (n1, n2, m, f, nz, kind) in enumerate(case["pairs"]):
        if kind == "chain":
            ch = chain_scene(n1, n2, m, f, nz, seed + 17 * k)
            X, front, _, _ = chain_points(ch)
            parts.append(dict(kp=ch["kq"], X=X, valid=front, match=ch["match"], planted=ch["planted"], R=ch["Rq"], t=ch["tq"],
                              K=ch["Kq"], chain=ch))
        else:
            parts.append(scene(n1, n2, m, f, nz, kind, seed + 17 * k))
    off1 = np.cumsum([0] + [len(q["kp"]) for q in parts]).astype(np.int64)
    off2 = np.cumsum([0] + [len(q["X"]) for q in parts]).astype(np.int64)
    valid = None
    if any(q["valid"] is not None for q in parts):
        valid = np.concatenate([np.ones(len(q["X"]), dtype=bool) if q["valid"] is None else q["valid"] for q in parts])
    return (np.concatenate([q["kp"] for q in parts]).astype(np.float32).reshape(-1, 2), off1,
            np.concatenate([q["X"] for q in parts]).astype(np.float64).reshape(-1, 3), valid, off2,
            np.concatenate([q["match"] for q in parts]).astype(np.int64), np.concatenate([q["planted"] for q in parts]).astype(bool),
            np.stack([q["K"] for q in parts]), parts)


def case_checksum(kp, X, match):
    return checksum(kp, np.nan_to_num(X), match)


def cam_inputs(seed=CAM_SEED):
    """seeded inputs of the camera functions: points [2, 40, 3] (one of them at Z = 0), a camera per batch entry,
    pixels [2, 40, 2], depths [2, 40, 1]"""
    r = np.random.default_rng(seed)
    pts = r.uniform([-4, -3, 2], [4, 3, 12], (2, 40, 3))
    pts[0, 5, 2] = 0.0
    Ks = np.stack([K, K_OTHER])[:, None]                    # [2, 1, 3, 3]
    uv = r.uniform([0, 0], [1024, 768], (2, 40, 2))
    depth = r.uniform(1.0, 20.0, (2, 40, 1))
    return pts, Ks, uv, depth


# ---------------------------------------------------------------- P3P
def grunert(j, X):
    """unit bearings j [3, 3] and points X [3, 3] (rows: points 1, 2, 3) -> (A0 .. A4, (q, cb, cg, ca, b)) of rr.h"""
    a2, b2, c2 = ((X[1] - X[2]) ** 2).sum(), ((X[0] - X[2]) ** 2).sum(), ((X[0] - X[1]) ** 2).sum()
    ca, cb, cg = j[1] @ j[2], j[0] @ j[2], j[0] @ j[1]
    with np.errstate(all="ignore"):
        q, p = (a2 - c2) / b2, (a2 + c2) / b2
        A4 = (q - 1) ** 2 - 4 * (c2 / b2) * ca ** 2
        A3 = 4 * (q * (1 - q) * cb - (1 - p) * ca * cg + 2 * (c2 / b2) * ca ** 2 * cb)
        A2 = 2 * (q ** 2 - 1 + 2 * q ** 2 * cb ** 2 + 2 * ((b2 - c2) / b2) * ca ** 2 - 4 * p * ca * cb * cg
                  + 2 * ((b2 - a2) / b2) * cg ** 2)
        A1 = 4 * (-q * (1 + q) * cb + 2 * (a2 / b2) * cg ** 2 * cb - (1 - p) * ca * cg)
        A0 = (1 + q) ** 2 - 4 * (a2 / b2) * cg ** 2
    return np.array([A0, A1, A2, A3, A4]), (q, cb, cg, ca, np.sqrt(b2))


def real_roots(c):
    """c [5] ascending -> (ascending real roots, near): near = two roots within NEAR (relative) of each
    other, or a complex root within NEAR of the real axis"""
    with np.errstate(all="ignore"):
        if not (np.isfinite(c).all() and abs(c[4]) > 0 and np.isfinite(c[:4] / c[4]).all()):
            return np.zeros(0), False
    w = np.roots(c[::-1])
    rel = np.abs(w.imag) / np.maximum(1.0, np.abs(w))
    real = np.sort(w[rel <= REAL].real)
    near = bool(((rel > REAL) & (rel < NEAR)).any())
    if len(real) > 1:
        near = near or bool((np.diff(real) / np.maximum(1.0, np.abs(real[1:]))).min() < NEAR)
    return real, near


def depths(j, X):
    """-> (list of (v, s1, s2, s3) over the kept roots in ascending v, near)"""
    c, (q, cb, cg, ca, b) = grunert(j, X)
    if not b > 0:
        return [], False
    v, near = real_roots(c)
    out = []
    for vk in v:
        with np.errstate(all="ignore"):
            u = ((q - 1) * vk * vk - 2 * q * cb * vk + 1 + q) / (2 * (cg - vk * ca))
            s1 = b / np.sqrt(1 + vk * vk - 2 * vk * cb)
        s = (s1, u * s1, vk * s1)
        if vk > 0 and u > 0 and s1 > 0 and np.isfinite(s).all():
            out.append((vk,) + s)
    return out, near


def frame(p):
    e1 = (p[1] - p[0]) / np.linalg.norm(p[1] - p[0])
    n = np.cross(e1, p[2] - p[0])
    ln = np.linalg.norm(n)
    e3 = n / ln
    return np.stack([e1, np.cross(e3, e1), e3], 1), ln     # columns e1 e2 e3


def kabsch(X, Y):
    """the rotation and translation with Y = R X + t on three points, by SVD"""
    mx, my = X.mean(0), Y.mean(0)
    U, _, Vt = np.linalg.svd((Y - my).T @ (X - mx))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, my - R @ mx


def p3p(h, X, route="A"):
    """h [3, 3] homogeneous image points, X [3, 3] -> (R [n, 3, 3], t [n, 3] in ascending v, near)"""
    with np.errstate(all="ignore"):
        j = h / np.linalg.norm(h, axis=1, keepdims=True)
        E, area = frame(X)
    none = (np.zeros((0, 3, 3)), np.zeros((0, 3)), False)
    if not area > 0 or not np.isfinite(j).all():
        return none
    if route == "A":
        sols, near = depths(j, X)
    else:   # points 1 and 3 exchanged: v' = s1 / s3 = 1 / v, and the depths come out as (s3, s2, s1)
        rev, near = depths(j[::-1], X[::-1])
        sols = sorted([(1.0 / vv, s3, s2, s1) for vv, s1, s2, s3 in rev])
    Rs, ts = [], []
    for _, s1, s2, s3 in sols:
        Y = np.array([s1, s2, s3])[:, None] * j
        with np.errstate(all="ignore"):
            if route == "A":
                Fm, _ = frame(Y)
                R = Fm @ E.T
                t = Y[0] - R @ X[0]
            else:
                R, t = kabsch(X, Y)
        if not (np.isfinite(R).all() and np.isfinite(t).all()):
            return none
        Rs.append(R)
        ts.append(t)
    return np.array(Rs).reshape(-1, 3, 3), np.array(ts).reshape(-1, 3), near


# ---------------------------------------------------------------- rr_p3p restated
def pose_err(Ra, ta, Rb, tb):
    """the largest absolute entry difference of R, and of t divided by max(1, |t|)"""
    return float(max(np.abs(Ra - Rb).max(), np.abs(ta - tb).max() / max(1.0, np.linalg.norm(tb))))


def solver_samples(seed=SOLVER_SEED, n=SOLVER_N):
    """-> x [n', 3, 2] float64 normalised points, X [n', 3, 3], the oracle's R [n', 4, 3, 3] and t [n', 4, 3]
    (ascending v, zeros past nsol), nsol [n'], the share of dropped (near-degenerate) samples, the largest
    A - B difference of every sample [n'], the oracle's largest reprojection residual of a sample's own points"""
    r = np.random.default_rng(seed)
    xs, Xs = [], []
    for _ in range(n):
        R = EC.rot(*r.uniform(-0.3, 0.3, 3))
        t = r.uniform(-1.0, 1.0, 3)
        px = r.uniform([0, 0], [EC.W, EC.H_IMG], (3, 2))
        ray = np.concatenate([px, np.ones((3, 1))], 1) @ np.linalg.inv(K).T
        Xc = ray * r.uniform(4.0, 12.0, 3)[:, None]
        obs = px + NOISE * r.standard_normal((3, 2))
        xs.append((np.concatenate([obs, np.ones((3, 1))], 1) @ np.linalg.inv(K).T)[:, :2])
        Xs.append((Xc - t) @ R)
    x, X = np.array(xs), np.array(Xs)
    Rm, tm = np.zeros((n, 4, 3, 3)), np.zeros((n, 4, 3))
    nsol, keep, diffs, resid = np.zeros(n, dtype=np.int32), np.ones(n, dtype=bool), np.zeros(n), 0.0
    for i in range(n):
        h = np.concatenate([x[i], np.ones((3, 1))], 1)
        Ra, ta, near_a = p3p(h, X[i], "A")
        Rb, tb, near_b = p3p(h, X[i], "B")
        if near_a or near_b:
            keep[i] = False
            continue
        assert len(Ra) == len(Rb), (i, len(Ra), len(Rb))
        nsol[i] = len(Ra)
        Rm[i, :len(Ra)], tm[i, :len(Ra)] = Ra, ta
        for k in range(len(Ra)):
            diffs[i] = max(diffs[i], pose_err(Rb[k], tb[k], Ra[k], ta[k]))
            Y = X[i] @ Ra[k].T + ta[k]
            resid = max(resid, float(np.abs(Y[:, :2] / Y[:, 2:] - x[i]).max()))
    return (np.ascontiguousarray(x[keep]), np.ascontiguousarray(X[keep]), Rm[keep], tm[keep], nsol[keep],
            float(1.0 - keep.mean()), diffs[keep], resid)


# ---------------------------------------------------------------- rr_localize_pairs restated
def inv_adj(Km):
    """(inverse by the adjugate, ok): the failure rule of step a"""
    with np.errstate(all="ignore"):
        c = np.array([[Km[1, 1] * Km[2, 2] - Km[1, 2] * Km[2, 1], Km[0, 2] * Km[2, 1] - Km[0, 1] * Km[2, 2], Km[0, 1] * Km[1, 2] - Km[0, 2] * Km[1, 1]],
                      [Km[1, 2] * Km[2, 0] - Km[1, 0] * Km[2, 2], Km[0, 0] * Km[2, 2] - Km[0, 2] * Km[2, 0], Km[0, 2] * Km[1, 0] - Km[0, 0] * Km[1, 2]],
                      [Km[1, 0] * Km[2, 1] - Km[1, 1] * Km[2, 0], Km[0, 1] * Km[2, 0] - Km[0, 0] * Km[2, 1], Km[0, 0] * Km[1, 1] - Km[0, 1] * Km[1, 0]]])
        det = Km[0] @ c[:, 0]
        inv = c / det
    ok = np.isfinite(Km).all() and np.isfinite(det) and abs(det) > 0 and np.isfinite(inv).all()
    return inv, bool(ok)


def reproject(Km, R, t, rec):
    """poses R [..., 3, 3], t [..., 3] on records [M, 5] -> (in front [..., M], reprojection error px [..., M])"""
    with np.errstate(all="ignore"):
        Xc = np.einsum("...ab,mb->...ma", R, rec[:, 2:]) + t[..., None, :]
        pc = Xc @ Km.T
        front = pc[..., 2] > 0
        z = np.where(front, pc[..., 2], 1.0)
        err = np.sqrt((pc[..., 0] / z - rec[:, 0]) ** 2 + (pc[..., 1] / z - rec[:, 1]) ** 2)
    return front, err


def exp_a(w):
    """Rodrigues as rr.h writes it: I + A [w]x + B [w]x^2, the series below SMALL2"""
    th2 = w @ w
    if th2 < SMALL2:
        A, B = 1 - th2 / 6, 0.5 - th2 / 24
    else:
        th = np.sqrt(th2)
        A, B = np.sin(th) / th, (1 - np.cos(th)) / th2
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + A * W + B * (W @ W)


def exp_b(w):
    """the axis-angle form: cos I + sin [k]x + (1 - cos) k k^T"""
    th = np.linalg.norm(w)
    if th < 1e-150:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * np.outer(k, k)


def gn_round(Km, R, t, rec, route):
    """GN_STEPS Gauss-Newton steps on the records rec [n, 5] -> (R, t) or None where the refit stops"""
    for _ in range(GN_STEPS):
        Xc = rec[:, 2:] @ R.T + t
        pc = Xc @ Km.T
        use = pc[:, 2] > 0
        Xc, pc, obs = Xc[use], pc[use], rec[use, :2]
        uv = pc[:, :2] / pc[:, 2:]
        res = uv - obs
        D = np.zeros((len(pc), 2, 3))
        D[:, 0, 0] = D[:, 1, 1] = 1.0 / pc[:, 2]
        D[:, 0, 2], D[:, 1, 2] = -uv[:, 0] / pc[:, 2], -uv[:, 1] / pc[:, 2]
        Mm = D @ Km                                               # [n, 2, 3]
        Sk = np.zeros((len(pc), 3, 3))
        Sk[:, 0, 1], Sk[:, 0, 2], Sk[:, 1, 0] = -Xc[:, 2], Xc[:, 1], Xc[:, 2]
        Sk[:, 1, 2], Sk[:, 2, 0], Sk[:, 2, 1] = -Xc[:, 0], -Xc[:, 1], Xc[:, 0]
        J = np.concatenate([-Mm @ Sk, Mm], 2)                     # [n, 2, 6]
        if route == "A":
            H = np.einsum("nri,nrj->ij", J, J)
            g = np.einsum("nri,nr->i", J, res)
            try:
                np.linalg.cholesky(H)
            except np.linalg.LinAlgError:
                return None
            if not np.isfinite(H).all():
                return None
            d = np.linalg.solve(H, -g)
            Ex = exp_a(d[:3])
        else:
            if len(J) == 0:
                return None
            d, _, rank, _ = np.linalg.lstsq(J.reshape(-1, 6), -res.reshape(-1), rcond=None)
            if rank < 6:
                return None
            Ex = exp_b(d[:3])
        R, t = Ex @ R, Ex @ t + d[3:]
    return R, t


def pnp_pair(kp, X, valid, match, Km, p, th=TH, iters=256, refine=2, seed=0, route="A"):
    """One pair of rr_localize_pairs in float64 -> dict(inliers, R, t, mask bool [n1]) plus the generator's
    diagnostics: t_win, sol (winner, -1 when none), margin (the smallest | reprojection error - th | met in
    any solution of any hypothesis or refit), m, counts [iters, 4], nsol [iters]"""
    n1, n2 = len(kp), len(X)
    keep = (match >= 0) & (match < n2)
    j = np.where(keep, match, 0)
    if n2:
        if valid is not None:
            keep &= valid[j].astype(bool)
        keep &= np.isfinite(X[j]).all(1)
    rows = np.nonzero(keep)[0]
    rec = np.concatenate([kp[rows].astype(np.float64), X[match[rows]]], 1).reshape(-1, 5)
    m = len(rows)
    out = dict(inliers=0, R=np.zeros((3, 3)), t=np.zeros(3), mask=np.zeros(n1, dtype=bool), t_win=-1, sol=-1, margin=np.inf,
               m=m, counts=np.zeros((iters, 4), dtype=np.int64), nsol=np.zeros(iters, dtype=np.int64))
    inv, ok = inv_adj(Km)
    if m < 3 or not ok:
        return out
    smp = EC.draw_n(seed, p, np.arange(iters), m, 3)
    Rs, ts = np.zeros((iters, 4, 3, 3)), np.zeros((iters, 4, 3))
    for it in range(iters):
        q = rec[smp[it]]
        h = np.concatenate([q[:, :2], np.ones((3, 1))], 1) @ inv.T
        Rk, tk, _ = p3p(h, q[:, 2:], route)
        out["nsol"][it] = len(Rk)
        Rs[it, :len(Rk)], ts[it, :len(Rk)] = Rk, tk
    live = np.arange(4)[None, :] < out["nsol"][:, None]               # [T, 4]
    front, err = reproject(Km, Rs, ts, rec)                           # [T, 4, M]
    front &= live[..., None]
    margin = np.abs(err[front] - th).min() if front.any() else np.inf
    counts = (front & (err <= th)).sum(-1)
    out.update(margin=margin, counts=counts)
    if counts.max() == 0:
        return out
    flat = int(np.argmax(counts.reshape(-1)))
    tw, sol = flat // 4, flat % 4
    out.update(t_win=tw, sol=sol)
    R, t, count = Rs[tw, sol], ts[tw, sol], int(counts[tw, sol])
    for _ in range(refine):
        fr, er = reproject(Km, R, t, rec)
        S = fr & (er <= th)
        if S.sum() < 4:
            break
        new = gn_round(Km, R, t, rec[S], route)
        if new is None or not (np.isfinite(new[0]).all() and np.isfinite(new[1]).all()):
            break
        fr2, er2 = reproject(Km, new[0], new[1], rec)
        margin = min(margin, np.abs(er2[fr2] - th).min() if fr2.any() else np.inf)
        c2 = int((fr2 & (er2 <= th)).sum())
        if c2 < count:
            break
        R, t, count = new[0], new[1], c2
    fr, er = reproject(Km, R, t, rec)
    out["mask"][rows[fr & (er <= th)]] = True
    out.update(inliers=count, R=R, t=t, margin=margin)
    return out


def pnp_batch(kp, off1, X, valid, off2, match, Ks, th=TH, iters=256, refine=2, seed=0, route="A"):
    """the ragged batch -> (inliers int32 [P], R [P, 3, 3], t [P, 3], mask bool [rows1], per-pair dicts)"""
    npairs = len(off1) - 1
    inl = np.zeros(npairs, dtype=np.int32)
    Rs, ts = np.zeros((npairs, 3, 3)), np.zeros((npairs, 3))
    mask = np.zeros(len(kp), dtype=bool)
    infos = []
    for p in range(npairs):
        a, b = slice(off1[p], off1[p + 1]), slice(off2[p], off2[p + 1])
        o = pnp_pair(kp[a], X[b], None if valid is None else valid[b], match[a], Ks[p], p, th, iters, refine, seed, route)
        inl[p], Rs[p], ts[p], mask[a] = o["inliers"], o["R"], o["t"], o["mask"]
        infos.append(o)
    return inl, Rs, ts, mask, infos
