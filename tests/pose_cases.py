"""Shared by tests/golden/make_golden_pose.py and the relative-pose tests: seeded two-view scenes built
on epipolar_cases.planted_pair that also return the true motion and 3-D points, and a float64 numpy
restatement of rr_recover_pose (steps a - e of include/rr.h), rr_triangulate_points and
rr_essential_decompose written from the header: np.linalg.svd for the 3 x 3, and for the
triangulation the SVD of the 4 x 4 itself.  numpy only: the golden generator imports this next to the
reference's own package."""

import numpy as np

import epipolar_cases as EC

STAGE = EC.STAGE
K1 = EC.K
# the second camera of the K1 != K2 cases: other focal lengths, another principal point
K2_OTHER = np.array([[760.0, 0.0, 500.0], [0.0, 775.0, 390.0], [0.0, 0.0, 1.0]])
W_EPS = 1e-8
SIZES = (0, 1, 7, 63, 64, 65, 257, STAGE + 1)   # used records: around a wavefront, above a block, above the LDS stage

# kind "true": every match planted (0.3 px noise), F the true one, mask None
# kind "ver":  60 % planted, F and mask from the restated verifier (epipolar_cases.epipolar_pair)
# kind "nomask": as "ver" but mask None, so the outliers are triangulated too
# kind "k2":   as "ver" with the second view seen through K2_OTHER
CASES = [dict(name="true%d" % m, kind="true", m=m) for m in SIZES] + \
        [dict(name="ver%d" % m, kind="ver", m=m) for m in (63, 64, 65, 257, STAGE + 1)] + \
        [dict(name="nomask65", kind="nomask", m=65), dict(name="k2_40", kind="k2", m=40)]
N_MOTIONS = 16
CASES += [dict(name="motion%d" % i, kind="true", m=24) for i in range(N_MOTIONS)]
POSE_SEED = 9100
VER = dict(th=EC.TH, iters=256, refine=2, seed=EC.RUN_SEED)
# the ragged batch: an empty pair, a pair whose F is all zeros, a pair with 3 matches, a noisy pair (verifier's F and
# mask) and the noise-free pair (exact in float32: R = I, t = (4, 1, 0) / sqrt(17))
RAGGED = [("empty", (0, 0, 0, 0.0, 0.3)), ("zeroF", (30, 28, 20, 1.0, 0.3)), ("three", (30, 28, 3, 1.0, 0.3)),
          ("noisy", (80, 90, 60, 0.6, 0.3)), ("exact", (60, 70, 50, 1.0, 0.0))]
RAGGED_SEED = 9700
T_EXACT = np.array([4.0, 1.0, 0.0]) / np.sqrt(17.0)
# end to end: verify_pairs(model="fundamental") -> recover_pose, 60 % inliers, 0.3 px noise
E2E = [(120, 130, 100, 0.6, 0.3), (150, 140, 120, 0.6, 0.3)]
E2E_SEED = 9900

checksum = EC.checksum


# ---------------------------------------------------------------- scenes
def scene(n1, n2, m, frac, noise, seed, K2=None):
    """epipolar_cases.planted_pair plus its truth -> dict(kp1, kp2, match, planted, F, R, t, X [n1, 3], K1, K2).
    The generator's random stream is replayed for the motion and the 3-D points (planted_pair does
    not return them); the replay is checked against the keypoints it returned.  K2: the second view
    is seen through these intrinsics instead of K1 (its keypoints are mapped by K2 K1^-1)."""
    kp1, kp2, match, planted, F = EC.planted_pair(n1, n2, m, frac, noise, seed)
    r = np.random.default_rng(seed)
    exact = noise == 0.0
    R = EC.rot(*r.uniform(-0.25, 0.25, 3))
    t = np.array([r.uniform(0.6, 1.2) * r.choice([-1, 1]), r.uniform(-0.3, 0.3), r.uniform(-0.5, 0.5)])
    if exact:
        R, t = np.eye(3), T_EXACT.copy()
    px_all, X_all = np.empty((0, 2)), np.empty((0, 3))
    while len(px_all) < n1:
        px = r.uniform([0, 0], [EC.W, EC.H_IMG], (4 * n1 + 16, 2))
        z = r.uniform(4.0, 12.0, len(px))
        if exact:
            px = np.round(px * 16) / 16
            z = EC.FOCAL * t[0] / (np.round(EC.FOCAL * t[0] / z * 16) / 16)
        P = np.concatenate([(px - EC.K[:2, 2]) / EC.FOCAL, np.ones((len(px), 1))], 1) * z[:, None]
        q, zz = EC.project(P, R, t)
        if exact:
            q = px + np.round(EC.FOCAL * t[0] / z * 16)[:, None] / 16 * np.array([1.0, 0.25])
        ok = EC.VC.inside(q) & (zz > 0.5)
        px_all, X_all = np.concatenate([px_all, px[ok]]), np.concatenate([X_all, P[ok]])
    assert np.array_equal(px_all[:n1].astype(np.float32), kp1), "the replay left planted_pair's stream"
    if K2 is not None:
        A = K2 @ np.linalg.inv(EC.K)
        kp2 = (kp2.astype(np.float64) @ A[:2, :2].T + A[:2, 2]).astype(np.float32)
        F = np.linalg.inv(A).T @ F
    return dict(kp1=kp1, kp2=kp2, match=match, planted=planted, F=F, R=R, t=t, X=X_all[:n1], K1=EC.K.copy(),
                K2=EC.K.copy() if K2 is None else K2.copy())


def records(s, mask=None):
    """the used rows of a scene and their records [M, 4] in float64 (rr.h step a)"""
    n2 = len(s["kp2"])
    use = (s["match"] >= 0) & (s["match"] < n2)
    if mask is not None:
        use &= mask.astype(bool)
    rows = np.nonzero(use)[0]
    rec = np.concatenate([s["kp1"][rows].astype(np.float64), s["kp2"][s["match"][rows]].astype(np.float64)], 1).reshape(-1, 4)
    return rows, rec


def build_case(case, seed):
    """-> (scene, F [3, 3], mask bool [n1] or None): the inputs of one single-pair case"""
    m = case["m"]
    n1, n2 = m + 10 + m // 8, m + 6 + m // 10
    if case["kind"] == "true":
        s = scene(n1, n2, m, 1.0, 0.3, seed)
        return s, EC.unit(s["F"]), None
    s = scene(n1, n2, m, 0.6, 0.3, seed, K2_OTHER if case["kind"] == "k2" else None)
    o = EC.epipolar_pair(s["kp1"], s["kp2"], s["match"], 0, **VER)
    return s, o["F"], (None if case["kind"] == "nomask" else o["mask"])


def build_ragged(seed):
    """-> (scenes, F [5, 3, 3], mask bool [rows1]): the five pairs of RAGGED"""
    scenes = [scene(*spec, seed + 17 * k) for k, (_, spec) in enumerate(RAGGED)]
    Fs, masks = [], []
    for (name, _), s in zip(RAGGED, scenes):
        F, mask = EC.unit(s["F"]), np.ones(len(s["kp1"]), dtype=bool)
        if name == "zeroF":
            F = np.zeros((3, 3))
        elif name == "noisy":
            o = EC.epipolar_pair(s["kp1"], s["kp2"], s["match"], 3, **VER)
            F, mask = o["F"], o["mask"]
        Fs.append(F)
        masks.append(mask)
    return scenes, np.stack(Fs), np.concatenate(masks)


def ragged_arrays(scenes):
    """kp1 [rows1, 2], off1, kp2 [rows2, 2], off2, match [rows1] of a list of scenes"""
    off1 = np.cumsum([0] + [len(s["kp1"]) for s in scenes]).astype(np.int64)
    off2 = np.cumsum([0] + [len(s["kp2"]) for s in scenes]).astype(np.int64)
    cat = lambda key, dt: np.concatenate([s[key] for s in scenes]).astype(dt)  # noqa: E731
    return cat("kp1", np.float32).reshape(-1, 2), off1, cat("kp2", np.float32).reshape(-1, 2), off2, cat("match", np.int64)


# ---------------------------------------------------------------- rr_essential_decompose restated
def decompose(E0):
    """steps b and c of rr.h -> (Ra, Rb, t, E) or None where the entry gives zeros"""
    if not np.isfinite(E0).all() or not E0.any():
        return None
    Vt = np.linalg.svd(E0)[2]
    v0, v1 = Vt[0], Vt[1]
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


# ---------------------------------------------------------------- rr_triangulate_points restated
def triangulate(P1, P2, rec):
    """records [M, 4] under P1, P2 [3, 4] -> (X [M, 3], w [M]): the rows of triangulation.py:27-31, the
    right singular vector of the smallest singular value of the 4 x 4 itself, de-homogenised"""
    if len(rec) == 0:
        return np.zeros((0, 3)), np.zeros(0)
    x1, y1, x2, y2 = rec.T
    A = np.stack([x1[:, None] * P1[2] - P1[0], y1[:, None] * P1[2] - P1[1], x2[:, None] * P2[2] - P2[0],
                  y2[:, None] * P2[2] - P2[1]], 1)
    h = np.linalg.svd(A)[2][:, -1, :]
    w = h[:, 3]
    s = np.where(np.abs(w) > W_EPS, 1.0 / np.where(np.abs(w) > W_EPS, w, 1.0), 1.0)
    return h[:, :3] * s[:, None], w


def projection(K, R, t):
    return K @ np.concatenate([R, t.reshape(3, 1)], 1)


# ---------------------------------------------------------------- rr_recover_pose restated
def pose_pair(kp1, kp2, match, mask, F, Ka, Kb):
    """One pair of rr_recover_pose in float64 -> dict(R, t, E, front, points3d [n1, 3], front_mask bool
    [n1]) plus the generator's diagnostics: counts [4], slot (the winner), rows (the used rows), depth
    (the smallest |depth| of a used record under any candidate), wgap (the smallest relative distance
    of a |w| from 1e-8), X4 [4, M, 3]."""
    n1 = len(kp1)
    s = dict(kp1=kp1, kp2=kp2, match=match)
    rows, rec = records(s, mask)
    out = dict(R=np.zeros((3, 3)), t=np.zeros(3), E=np.zeros((3, 3)), front=0, points3d=np.zeros((n1, 3)),
               front_mask=np.zeros(n1, dtype=bool), counts=np.zeros(4, dtype=np.int64), slot=-1, rows=rows, depth=np.inf,
               wgap=np.inf, X4=None)
    ok = np.isfinite(F).all() and F.any() and np.isfinite(Ka).all() and np.isfinite(Kb).all()
    dec = decompose(Kb.T @ F @ Ka) if ok else None
    if dec is None or len(rows) == 0:
        return out
    Ra, Rb, t, E = dec
    cands = [(Ra, t), (Ra, -t), (Rb, t), (Rb, -t)]
    P1 = projection(Ka, np.eye(3), np.zeros(3))
    X4, fronts = [], []
    for R, tt in cands:
        X, w = triangulate(P1, projection(Kb, R, tt), rec)
        d1, d2 = X[:, 2], (X @ R.T)[:, 2] + tt[2]
        out["depth"] = min(out["depth"], np.abs(d1).min(), np.abs(d2).min())
        out["wgap"] = min(out["wgap"], (np.abs(np.abs(w) - W_EPS) / W_EPS).min())
        X4.append(X)
        fronts.append((d1 > 0) & (d2 > 0))
    counts = np.array([f.sum() for f in fronts])
    slot = int(np.argmax(counts))        # the first of the highest count
    out["points3d"][rows] = X4[slot]
    out["front_mask"][rows] = fronts[slot]
    out.update(R=cands[slot][0], t=cands[slot][1], E=E, front=int(counts[slot]), counts=counts, slot=slot, X4=np.stack(X4))
    return out


def pose_batch(kp1, off1, kp2, off2, match, mask, F, Ka, Kb):
    """the ragged batch -> (R [P, 3, 3], t [P, 3], E [P, 3, 3], front int32 [P], points3d [rows1, 3], front_mask
    bool [rows1], per-pair dicts); Ka / Kb [3, 3] or [P, 3, 3]"""
    npairs = len(off1) - 1
    Ka, Kb = np.broadcast_to(Ka, (npairs, 3, 3)), np.broadcast_to(Kb, (npairs, 3, 3))
    R, t, E = np.zeros((npairs, 3, 3)), np.zeros((npairs, 3)), np.zeros((npairs, 3, 3))
    front = np.zeros(npairs, dtype=np.int32)
    pts, fm, infos = np.zeros((len(kp1), 3)), np.zeros(len(kp1), dtype=bool), []
    for p in range(npairs):
        a, b = slice(off1[p], off1[p + 1]), slice(off2[p], off2[p + 1])
        o = pose_pair(kp1[a], kp2[b], match[a], None if mask is None else mask[a], F[p], Ka[p], Kb[p])
        R[p], t[p], E[p], front[p], pts[a], fm[a] = o["R"], o["t"], o["E"], o["front"], o["points3d"], o["front_mask"]
        infos.append(o)
    return R, t, E, front, pts, fm, infos


# ---------------------------------------------------------------- errors
def median_depth(X):
    z = X[:, 2][np.abs(X[:, 2]) > 0]
    return float(np.median(np.abs(z))) if len(z) else 1.0


def rot_angle_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1.0, 1.0))))


def dir_angle_deg(a, b):
    return float(np.degrees(np.arccos(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1.0, 1.0))))
