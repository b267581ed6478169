"""Shared by tests/golden/make_golden_verify.py and the spatial-verification tests: seeded
planted-homography cases, the point sets of the DLT cases, a numpy restatement of the sampling
hash of include/rr.h and a float64 restatement of rr_verify_pairs (steps a - e of rr.h) and of
the reference's find_homography_dlt (np.linalg.solve for the 4-point fit, np.linalg.eigh for the
DLT).  numpy only: the golden generator imports this next to the reference's own package."""

import numpy as np

W, H_IMG = 1024.0, 768.0
CORNERS = np.array([[0.0, 0.0], [W, 0.0], [W, H_IMG], [0.0, H_IMG]])
DET_EPS = 1e-6      # RR_VERIFY_DET_EPS
W_EPS = 1e-8
EPS = 1e-8
STAGE = 1024        # records of the LDS stage of the RANSAC kernel (V_STAGE)

# ---------------------------------------------------------------- DLT cases (find_homography_dlt)
# (B, N, weighted): N in {4, 5, 8, 50, 500}, B in {1, 3}; weighted cases zero some rows' weights
DLT_CASES = [(1, 4, False), (1, 4, True), (3, 5, False), (1, 5, True), (3, 8, True), (1, 8, False),
             (3, 50, False), (1, 50, True), (1, 500, False), (3, 500, True)]
DLT_SEED = 7100

# ---------------------------------------------------------------- RANSAC cases (rr_verify_pairs)
# pairs: (n1, n2, kept matches M, planted inlier fraction, noise px); th 3 px everywhere
VERIFY_CASES = [
    dict(name="m0", pairs=[(20, 25, 0, 0.0, 0.5)], iters=256, refine=2),
    dict(name="m3", pairs=[(20, 25, 3, 1.0, 0.5)], iters=256, refine=2),
    dict(name="m4", pairs=[(9, 12, 4, 1.0, 0.5)], iters=256, refine=2),
    dict(name="m5", pairs=[(16, 11, 5, 0.8, 0.5)], iters=256, refine=2),
    dict(name="m40", pairs=[(70, 64, 40, 0.5, 0.5)], iters=300, refine=2),
    dict(name="m257_r0", pairs=[(300, 310, 257, 0.4, 0.5)], iters=300, refine=0),
    dict(name="m257_r2", pairs=[(300, 310, 257, 0.4, 0.5)], iters=256, refine=2),
    dict(name="m1025", pairs=[(1100, 1060, STAGE + 1, 0.5, 0.5)], iters=256, refine=2),
    dict(name="iters1", pairs=[(70, 64, 40, 1.0, 0.5)], iters=1, refine=2),
    dict(name="ragged4", pairs=[(0, 0, 0, 0.0, 0.5), (30, 28, 2, 1.0, 0.5), (80, 90, 60, 0.0, 0.5), (60, 70, 50, 1.0, 0.0)],
         iters=300, refine=2),
]
VERIFY_SEED = 7300
TH = 3.0
RUN_SEED = 12345    # the `seed` argument of verify_pairs in the cases


def true_homography(r):
    """a mild random homography of the image: rotation, scale, shift and a little perspective"""
    ang = r.uniform(-0.2, 0.2)
    s = r.uniform(0.85, 1.15)
    c = np.array([W / 2, H_IMG / 2])
    R = s * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    t = c - R @ c + r.uniform(-40, 40, 2)
    Ht = np.eye(3)
    Ht[:2, :2] = R
    Ht[:2, 2] = t
    Ht[2, :2] = r.uniform(-5e-5, 5e-5, 2)
    return Ht


def transfer(Hm, pts):
    """pi(H [x, y, 1]) of float64 points [n, 2]"""
    pts = np.asarray(pts, dtype=np.float64)
    q = pts @ Hm[:2, :2].T + Hm[:2, 2]
    w = pts @ Hm[2, :2] + Hm[2, 2]
    return q / w[:, None]


def corner_err(Ha, Hb):
    """largest distance in px between the images of the four image corners under two homographies"""
    return float(np.sqrt(((transfer(Ha, CORNERS) - transfer(Hb, CORNERS)) ** 2).sum(1)).max())


def inside(p):
    return (p[:, 0] >= 0) & (p[:, 0] < W - 1) & (p[:, 1] >= 0) & (p[:, 1] < H_IMG - 1)


def planted_pair(n1, n2, m, frac, noise, seed):
    """-> kp1 [n1, 2] f32, kp2 [n2, 2] f32, match int64 [n1], planted bool [n1], H_true.
    m rows of side 1 are matched to distinct rows of side 2; round(frac m) of them are images
    under H_true plus Gaussian noise, the others uniform."""
    r = np.random.default_rng(seed)
    Ht = true_homography(r)
    kp1 = np.empty((0, 2))
    while len(kp1) < n1:   # side-1 points whose image stays inside the frame
        c = r.uniform([0, 0], [W, H_IMG], (2 * n1 + 8, 2))
        kp1 = np.concatenate([kp1, c[inside(transfer(Ht, c))]])
    kp1 = kp1[:n1].astype(np.float32)
    kp2 = r.uniform([0, 0], [W, H_IMG], (n2, 2))
    match = np.full(n1, -1, dtype=np.int64)
    planted = np.zeros(n1, dtype=bool)
    rows = np.sort(r.permutation(n1)[:m])
    cols = r.permutation(n2)[:m]
    match[rows] = cols
    nin = int(round(frac * m))
    inl = r.permutation(m)[:nin]
    planted[rows[inl]] = True
    img = transfer(Ht, kp1[rows[inl]].astype(np.float64)) + noise * r.standard_normal((nin, 2))
    kp2[cols[inl]] = np.clip(img, 0, [W - 0.01, H_IMG - 0.01])
    return kp1, kp2.astype(np.float32), match, planted, Ht


def build_case(case, seed):
    """the ragged batch of a case: kp1 [rows1, 2], off1 [P + 1], kp2, off2, match [rows1], planted [rows1]"""
    parts = [planted_pair(n1, n2, m, f, nz, seed + 17 * k) for k, (n1, n2, m, f, nz) in enumerate(case["pairs"])]
    off1 = np.cumsum([0] + [len(q[0]) for q in parts]).astype(np.int64)
    off2 = np.cumsum([0] + [len(q[1]) for q in parts]).astype(np.int64)
    cat = lambda i, dt: np.concatenate([q[i] for q in parts]).astype(dt)  # noqa: E731
    return cat(0, np.float32).reshape(-1, 2), off1, cat(1, np.float32).reshape(-1, 2), off2, cat(2, np.int64), cat(3, bool)


def checksum(*arrays):
    return np.array([np.asarray(a, dtype=np.float64).sum() for a in arrays], dtype=np.float64)


def dlt_points(b, n, weighted, seed):
    """float64 point sets [b, n, 2] x 2 and weights [b, n] (None when unweighted): images under a
    planted homography plus 0.5 px noise; weighted sets carry a few gross outliers of small
    weight and (n > 5) some rows of weight exactly 0."""
    r = np.random.default_rng(seed)
    p1 = np.empty((b, n, 2))
    p2 = np.empty((b, n, 2))
    w = np.ones((b, n)) if weighted else None
    for i in range(b):
        kp1, kp2, match, _, _ = planted_pair(n, n, n, 1.0, 0.5, int(r.integers(1 << 30)))
        p1[i] = kp1.astype(np.float64)
        p2[i] = kp2.astype(np.float64)[match]
        if weighted:
            w[i] = r.uniform(0.2, 1.0, n)
            if n > 5:
                bad = r.permutation(n)[:max(1, n // 10)]
                p2[i, bad] = r.uniform([0, 0], [W, H_IMG], (len(bad), 2))
                w[i, bad] = 1e-3
                w[i, r.permutation(n)[:max(1, n // 8)]] = 0.0
    return p1, p2, w


# ---------------------------------------------------------------- the sampling hash of rr.h
def mix(x):
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def draw4(seed, p, t, m):
    """sample indices [len(t), 4] of hypotheses t (array) of pair p over m >= 4 records: the rule
    of rr.h, on an explicit array a = [0 .. m)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s = mix((seed & 0xFFFFFFFF) + 0x9E3779B9)
    s = mix(s ^ np.uint64(seed >> 32))
    s = mix(s + np.uint64(p))
    t = np.asarray(t, dtype=np.uint64)
    s = mix(s + t)
    out = np.empty((len(t), 4), dtype=np.int64)
    for n, st in enumerate(s):
        a = np.arange(m)
        for j in range(4):
            k = int(mix(st + np.uint64(j))) % (m - j)
            out[n, j] = a[k]
            a[k] = a[m - 1 - j]
    return out


# ---------------------------------------------------------------- the reference's DLT on eigh
def normalize_points(pts):
    mean = pts.mean(0)
    scale = np.float64(np.sqrt(np.float32(2.0))) / (np.sqrt(((pts - mean) ** 2).sum(1)).mean() + EPS)
    T = np.array([[scale, 0, -scale * mean[0]], [0, scale, -scale * mean[1]], [0, 0, 1.0]])
    return pts @ T[:2, :2].T + T[:2, 2], T


def dlt(p1, p2, w=None):
    """find_homography_dlt of the reference for one point set [n, 2] x 2 (float64), eigh in place of svd"""
    p1 = np.asarray(p1, dtype=np.float64)
    p2 = np.asarray(p2, dtype=np.float64)
    q1, T1 = normalize_points(p1)
    q2, T2 = normalize_points(p2)
    x1, y1, x2, y2 = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    o, z = np.ones_like(x1), np.zeros_like(x1)
    ax = np.stack([z, z, z, -x1, -y1, -o, y2 * x1, y2 * y1, y2], 1)
    ay = np.stack([x1, y1, o, z, z, z, -x2 * x1, -x2 * y1, -x2], 1)
    A = np.stack([ax, ay], 1).reshape(-1, 9)
    ww = np.ones(len(p1)) if w is None else np.asarray(w, dtype=np.float64)
    M = A.T @ (np.repeat(ww, 2)[:, None] * A)
    _, V = np.linalg.eigh(M)
    Hm = np.linalg.inv(T2) @ (V[:, 0].reshape(3, 3) @ T1)
    return Hm / (Hm[2, 2] + EPS)


def dlt_iterated(p1, p2, w, th=3.0, n_iter=5):
    Hm = dlt(p1, p2, w)
    for _ in range(n_iter - 1):
        q = p1 @ Hm[:2, :2].T + Hm[:2, 2]
        zz = p1 @ Hm[2, :2] + Hm[2, 2]
        q = q * np.where(np.abs(zz) > EPS, 1.0 / zz, 1.0)[:, None]
        Hm = dlt(p1, p2, np.exp(-((q - p2) ** 2).sum(1) / (2.0 * th ** 2)))
    return Hm


# ---------------------------------------------------------------- rr_verify_pairs restated
def tri(a, b, c):
    return (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (c[..., 0] - a[..., 0]) * (b[..., 1] - a[..., 1])


def degenerate(q):
    """q [T, 4, 2]: any three of the four points within DET_EPS of collinear"""
    d = np.stack([np.abs(tri(q[:, 3], q[:, 1], q[:, 2])), np.abs(tri(q[:, 0], q[:, 3], q[:, 2])),
                  np.abs(tri(q[:, 0], q[:, 1], q[:, 3])), np.abs(tri(q[:, 0], q[:, 1], q[:, 2]))], 1)
    return ~(d.min(1) > DET_EPS)


def four_point(a, b):
    """H with H[2, 2] = 1 through a [4, 2] -> b [4, 2] by the 8 x 8 system; None when singular / not finite"""
    A = np.zeros((8, 8))
    for k in range(4):
        x, y, u, v = a[k, 0], a[k, 1], b[k, 0], b[k, 1]
        A[2 * k] = [x, y, 1, 0, 0, 0, -u * x, -u * y]
        A[2 * k + 1] = [0, 0, 0, x, y, 1, -v * x, -v * y]
    try:
        h = np.linalg.solve(A, b.reshape(8))
    except np.linalg.LinAlgError:
        return None
    Hm = np.append(h, 1.0).reshape(3, 3)
    return Hm if np.isfinite(Hm).all() else None


def residuals(Hm, rec):
    """(inlier-eligible [m], residual px [m]) of records (x1, y1, x2, y2) under H"""
    w = rec[:, 0] * Hm[2, 0] + rec[:, 1] * Hm[2, 1] + Hm[2, 2]
    ok = np.abs(w) > W_EPS
    ws = np.where(ok, w, 1.0)
    u = (rec[:, 0] * Hm[0, 0] + rec[:, 1] * Hm[0, 1] + Hm[0, 2]) / ws
    v = (rec[:, 0] * Hm[1, 0] + rec[:, 1] * Hm[1, 1] + Hm[1, 2]) / ws
    return ok, np.sqrt((u - rec[:, 2]) ** 2 + (v - rec[:, 3]) ** 2)


def verify_pair(kp1, kp2, match, p, th=TH, iters=1024, refine=2, seed=0):
    """One pair of rr_verify_pairs in float64 -> dict(inliers, H [3, 3], mask bool [n1]) plus the
    generator's diagnostics: t (winner, -1 when none), runner (the best count of another t),
    margin (the smallest | residual - th | met in any hypothesis or refit), m, fit (the records
    the returned H was fitted to: the 4 samples, or the last accepted inlier set)."""
    n1, n2 = len(kp1), len(kp2)
    rows = np.nonzero((match >= 0) & (match < n2))[0]
    rec = np.concatenate([kp1[rows].astype(np.float64), kp2[match[rows]].astype(np.float64)], 1).reshape(-1, 4)
    m = len(rows)
    out = dict(inliers=0, H=np.zeros((3, 3)), mask=np.zeros(n1, dtype=bool), t=-1, runner=0, margin=np.inf, m=m, fit=None)
    if m < 4:
        return out
    smp = draw4(seed, p, np.arange(iters), m)
    q = rec[smp]                                   # [T, 4, 4]
    deg = degenerate(q[:, :, :2]) | degenerate(q[:, :, 2:])
    counts = np.zeros(iters, dtype=np.int64)
    Hs = [None] * iters
    margin = np.inf
    for t in np.nonzero(~deg)[0]:
        Hm = four_point(q[t, :, :2], q[t, :, 2:])
        if Hm is None:
            continue
        ok, res = residuals(Hm, rec)
        margin = min(margin, np.abs(res[ok] - th).min() if ok.any() else np.inf)
        counts[t] = (ok & (res <= th)).sum()
        Hs[t] = Hm
    out["margin"] = margin
    if counts.max() == 0:
        return out
    t = int(np.argmax(counts))                     # the first of the highest count
    out["t"] = t
    out["runner"] = int(np.delete(counts, t).max()) if iters > 1 else 0
    Hm, count, fit = Hs[t], int(counts[t]), rec[smp[t]]
    for _ in range(refine):
        ok, res = residuals(Hm, rec)
        S = ok & (res <= th)
        if S.sum() < 4:
            break
        H2 = dlt(rec[S, :2], rec[S, 2:])
        if not np.isfinite(H2).all():
            break
        ok2, res2 = residuals(H2, rec)
        margin = min(margin, np.abs(res2[ok2] - th).min() if ok2.any() else np.inf)
        c2 = int((ok2 & (res2 <= th)).sum())
        if c2 < count:
            break
        Hm, count, fit = H2, c2, rec[S]
    ok, res = residuals(Hm, rec)
    out["mask"][rows[ok & (res <= th)]] = True
    out.update(inliers=count, H=Hm, margin=margin, fit=fit)
    return out


def verify_batch(kp1, off1, kp2, off2, match, th=TH, iters=1024, refine=2, seed=0):
    """the ragged batch -> (inliers int32 [P], H [P, 3, 3], mask bool [rows1], per-pair dicts)"""
    npairs = len(off1) - 1
    inl = np.zeros(npairs, dtype=np.int32)
    Hs = np.zeros((npairs, 3, 3))
    mask = np.zeros(len(kp1), dtype=bool)
    infos = []
    for p in range(npairs):
        a, b = slice(off1[p], off1[p + 1]), slice(off2[p], off2[p + 1])
        o = verify_pair(kp1[a], kp2[b], match[a], p, th, iters, refine, seed)
        inl[p], Hs[p], mask[a] = o["inliers"], o["H"], o["mask"]
        infos.append(o)
    return inl, Hs, mask, infos
