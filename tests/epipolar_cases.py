"""Shared by tests/golden/make_golden_epipolar.py and the epipolar-verification tests: seeded
planted two-view scenes, the point sets of the 8-point cases, and a float64 numpy restatement of
rr_verify_pairs_epipolar (steps a - e of include/rr.h), rr_fundamental_dlt and rr_epipolar_distance,
written from the header: np.linalg.svd for the null space of the seven-point system (converted to
the canonical basis), np.linalg.eigh for the 8-point fit and the rank-2 projection.  A second,
independent null-space solver (Gauss-Jordan with partial pivoting) is there for the generator's
conditions.  numpy only: the golden generator imports this next to the reference's own package."""

import numpy as np

import verify_cases as VC

W, H_IMG, FOCAL = 1024.0, 768.0, 900.0
K = np.array([[FOCAL, 0.0, W / 2], [0.0, FOCAL, H_IMG / 2], [0.0, 0.0, 1.0]])
EPS = 1e-8
STAGE = VC.STAGE     # records of the LDS stage of the RANSAC kernels
RT2 = np.float64(np.sqrt(np.float32(2.0)))

# ---------------------------------------------------------------- 8-point cases (find_fundamental)
# (B, N, weighted): N in {8, 9, 50, 500}; weighted sets carry rows of weight 0; B = 3 among them
FUND_CASES = [(1, 8, False), (1, 8, True), (3, 9, False), (1, 9, True), (3, 50, True), (1, 50, False),
              (1, 500, False), (3, 500, True)]
FUND_SEED = 8100

# ---------------------------------------------------------------- RANSAC cases (rr_verify_pairs_epipolar)
# pairs: (n1, n2, kept matches M, planted fraction, noise px); th 1.5 px everywhere, iters <= 512
EPI_CASES = [
    dict(name="m0", pairs=[(20, 25, 0, 0.0, 0.3)], iters=256, refine=2),
    dict(name="m6", pairs=[(20, 25, 6, 1.0, 0.3)], iters=256, refine=2),
    dict(name="m7", pairs=[(12, 14, 7, 1.0, 0.3)], iters=256, refine=2),
    dict(name="m8", pairs=[(12, 11, 8, 1.0, 0.3)], iters=256, refine=2),
    dict(name="m40", pairs=[(70, 64, 40, 0.6, 0.3)], iters=300, refine=2),
    dict(name="m257_r0", pairs=[(300, 310, 257, 0.6, 0.3)], iters=300, refine=0),
    dict(name="m257_r2", pairs=[(300, 310, 257, 0.6, 0.3)], iters=256, refine=2),
    dict(name="m1025", pairs=[(1100, 1060, STAGE + 1, 0.6, 0.3)], iters=256, refine=2),
    dict(name="iters1", pairs=[(70, 64, 40, 1.0, 0.3)], iters=1, refine=2),
    dict(name="iters257", pairs=[(70, 64, 40, 0.6, 0.3)], iters=257, refine=2),
    dict(name="outliers", pairs=[(80, 90, 60, 0.0, 0.3)], iters=300, refine=2),
    dict(name="ragged4", pairs=[(0, 0, 0, 0.0, 0.3), (30, 28, 3, 1.0, 0.3), (80, 90, 60, 0.0, 0.3), (60, 70, 50, 1.0, 0.0)],
         iters=300, refine=2),
]
EPI_SEED = 8300
TH = 1.5
RUN_SEED = 12345     # the `seed` argument of verify_pairs in the cases


# ---------------------------------------------------------------- scenes
def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def project(P, R, t):
    q = (P @ R.T + t) @ K.T
    return q[:, :2] / q[:, 2:], q[:, 2]


def true_fundamental(R, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    return Ki.T @ tx @ R @ Ki


def planted_pair(n1, n2, m, frac, noise, seed):
    """-> kp1 [n1, 2] f32, kp2 [n2, 2] f32, match int64 [n1], planted bool [n1], F_true.
    3-D points at depth 4 .. 12 in front of the first camera (1024 x 768, f = 900); the second view
    is rotated by up to 0.25 rad per axis and translated; both projections lie inside the frame.
    m rows of side 1 are matched to distinct rows of side 2; round(frac m) of them are true
    correspondences plus Gaussian noise on side 2, the others uniform."""
    r = np.random.default_rng(seed)
    exact = noise == 0.0
    R = rot(*r.uniform(-0.25, 0.25, 3))
    t = np.array([r.uniform(0.6, 1.2) * r.choice([-1, 1]), r.uniform(-0.3, 0.3), r.uniform(-0.5, 0.5)])
    if exact:
        # A noise-free pair has to be noise-free in float32, or the rounding of the keypoints
        # (6e-5 px at x = 1000) is its noise.  Only a view without rotation allows that: side 1 on a
        # 1/16 px grid, t = (4, 1, 0) / sqrt(17), and depths at which the disparity f |t| / z is a
        # multiple of 1/16 px too, so x2 = x1 + d, y2 = y1 + d / 4 are float32 numbers.  Its true
        # F is [t]_x up to scale with F[2][2] = 0.
        R, t = np.eye(3), np.array([4.0, 1.0, 0.0]) / np.sqrt(17.0)
    kp1, img2 = np.empty((0, 2)), np.empty((0, 2))
    while len(kp1) < n1:
        px = r.uniform([0, 0], [W, H_IMG], (4 * n1 + 16, 2))
        z = r.uniform(4.0, 12.0, len(px))
        if exact:
            px = np.round(px * 16) / 16
            z = FOCAL * t[0] / (np.round(FOCAL * t[0] / z * 16) / 16)
        P = np.concatenate([(px - K[:2, 2]) / FOCAL, np.ones((len(px), 1))], 1) * z[:, None]
        q, zz = project(P, R, t)
        if exact:
            q = px + np.round(FOCAL * t[0] / z * 16)[:, None] / 16 * np.array([1.0, 0.25])
        ok = VC.inside(q) & (zz > 0.5)
        kp1, img2 = np.concatenate([kp1, px[ok]]), np.concatenate([img2, q[ok]])
    kp1, img2 = kp1[:n1], img2[:n1]
    kp2 = r.uniform([0, 0], [W, H_IMG], (n2, 2))
    match = np.full(n1, -1, dtype=np.int64)
    planted = np.zeros(n1, dtype=bool)
    rows = np.sort(r.permutation(n1)[:m])
    cols = r.permutation(n2)[:m]
    match[rows] = cols
    nin = int(round(frac * m))
    inl = r.permutation(m)[:nin]
    planted[rows[inl]] = True
    kp2[cols[inl]] = np.clip(img2[rows[inl]] + noise * r.standard_normal((nin, 2)), 0, [W - 0.01, H_IMG - 0.01])
    return kp1.astype(np.float32), kp2.astype(np.float32), match, planted, true_fundamental(R, t)


def build_case(case, seed):
    """the ragged batch of a case: kp1 [rows1, 2], off1 [P + 1], kp2, off2, match [rows1], planted [rows1]"""
    parts = [planted_pair(n1, n2, m, f, nz, seed + 17 * k) for k, (n1, n2, m, f, nz) in enumerate(case["pairs"])]
    off1 = np.cumsum([0] + [len(q[0]) for q in parts]).astype(np.int64)
    off2 = np.cumsum([0] + [len(q[1]) for q in parts]).astype(np.int64)
    cat = lambda i, dt: np.concatenate([q[i] for q in parts]).astype(dt)  # noqa: E731
    return cat(0, np.float32).reshape(-1, 2), off1, cat(1, np.float32).reshape(-1, 2), off2, cat(2, np.int64), cat(3, bool)


checksum = VC.checksum


def fund_points(b, n, weighted, seed):
    """float64 point sets [b, n, 2] x 2 and weights [b, n] (all ones when unweighted): a planted two-view
    scene plus 0.3 px noise; weighted sets carry a few gross outliers of small weight and rows of weight 0"""
    r = np.random.default_rng(seed)
    p1, p2, w = np.empty((b, n, 2)), np.empty((b, n, 2)), np.ones((b, n))
    for i in range(b):
        kp1, kp2, match, _, _ = planted_pair(n, n, n, 1.0, 0.3, int(r.integers(1 << 30)))
        p1[i], p2[i] = kp1.astype(np.float64), kp2.astype(np.float64)[match]
        if weighted:
            w[i] = r.uniform(0.2, 1.0, n)
            if n >= 50:   # a set of 8 or 9 keeps every point: the fit needs 8
                bad = r.permutation(n)[:max(1, n // 10)]
                p2[i, bad] = r.uniform([0, 0], [W, H_IMG], (len(bad), 2))
                w[i, bad] = 1e-3
                w[i, r.permutation(n)[:max(1, n // 8)]] = 0.0
            elif n == 9:
                w[i, r.integers(n)] = 0.0
    return p1, p2, w


# ---------------------------------------------------------------- the sampler of rr.h, K indices
def draw_n(seed, p, t, m, k):
    """sample indices [len(t), k] of hypotheses t of pair p over m >= k records: the rule of rr.h with
    j = 0 .. k - 1, on an explicit array a = [0 .. m)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s = VC.mix((seed & 0xFFFFFFFF) + 0x9E3779B9)
    s = VC.mix(s ^ np.uint64(seed >> 32))
    s = VC.mix(s + np.uint64(p))
    s = VC.mix(s + np.asarray(t, dtype=np.uint64))
    out = np.empty((len(s), k), dtype=np.int64)
    for n, st in enumerate(s):
        a = np.arange(m)
        for j in range(k):
            i = int(VC.mix(st + np.uint64(j))) % (m - j)
            out[n, j] = a[i]
            a[i] = a[m - 1 - j]
    return out


# ---------------------------------------------------------------- residuals (metrics.py, rr.h step c)
def epi_terms(F, rec):
    """F [..., 3, 3], records [M, 4] -> num, d1, d2 [..., M]"""
    x1 = np.concatenate([rec[:, :2], np.ones((len(rec), 1))], 1)
    x2 = np.concatenate([rec[:, 2:], np.ones((len(rec), 1))], 1)
    l = np.einsum("...ij,mj->...mi", F, x1)      # F x1
    mt = np.einsum("...ji,mj->...mi", F, x2)     # F^T x2
    num = (l * x2).sum(-1) ** 2
    return num, l[..., 0] ** 2 + l[..., 1] ** 2, mt[..., 0] ** 2 + mt[..., 1] ** 2


def sampson(F, rec):
    """(eligible [..., M], Sampson distance px [..., M])"""
    num, d1, d2 = epi_terms(F, rec)
    den = d1 + d2
    ok = den > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        return ok, np.sqrt(np.where(ok, num / np.where(ok, den, 1.0), np.inf))


def distance(p1, p2, F, kind, squared=True, eps=1e-8):
    """rr_epipolar_distance for one set: p1, p2 [N, 2], F [3, 3]"""
    num, d1, d2 = epi_terms(F, np.concatenate([p1, p2], 1))
    out = num / (d1 + d2) if kind == "sampson" else num * (1.0 / d1 + 1.0 / d2)
    return out if squared else np.sqrt(out + eps)


# ---------------------------------------------------------------- normalisation, 8-point fit
def normalize_points(pts):
    mean = pts.mean(0)
    s = RT2 / (np.sqrt(((pts - mean) ** 2).sum(1)).mean() + EPS)
    T = np.array([[s, 0, -s * mean[0]], [0, s, -s * mean[1]], [0, 0, 1.0]])
    return pts @ T[:2, :2].T + T[:2, 2], T


def design(q1, q2):
    """rows [u2 u1, u2 v1, u2, v2 u1, v2 v1, v2, u1, v1, 1] of points [..., 2]"""
    u1, v1, u2, v2 = q1[..., 0], q1[..., 1], q2[..., 0], q2[..., 1]
    return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], -1)


def fundamental(p1, p2, w=None):
    """rr_fundamental_dlt for one point set [n, 2] x 2 (float64); zeros below 8 points"""
    p1, p2 = np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)
    if len(p1) < 8:
        return np.zeros((3, 3))
    q1, T1 = normalize_points(p1)
    q2, T2 = normalize_points(p2)
    X = design(q1, q2)
    ww = np.ones(len(p1)) if w is None else np.asarray(w, dtype=np.float64)
    _, V = np.linalg.eigh(X.T @ (ww[:, None] * X))
    f = V[:, 0].reshape(3, 3)
    _, V3 = np.linalg.eigh(f.T @ f)
    v3 = V3[:, 0]
    f = f - np.outer(f @ v3, v3)
    F = T2.T @ f @ T1
    return F / (F[2, 2] + EPS) if abs(F[2, 2]) > EPS else F


def unit(F):
    """unit Frobenius norm, the entry of largest magnitude positive (rr.h step e)"""
    n = np.sqrt((F ** 2).sum())
    if not n > 0:
        return np.zeros((3, 3))
    i = int(np.argmax(np.abs(F).reshape(-1)))
    return F / (n if F.reshape(-1)[i] > 0 else -n)


def f_err(Fa, Fb):
    """largest absolute entry difference after scaling both to unit Frobenius norm and aligning the sign"""
    a, b = Fa / np.sqrt((Fa ** 2).sum()), Fb / np.sqrt((Fb ** 2).sum())
    return float(min(np.abs(a - b).max(), np.abs(a + b).max()))


# ---------------------------------------------------------------- seven-point solver (rr.h step b)
def null_svd(A):
    """A [T, 7, 9] -> (F1, F2) [T, 9]: the null vectors with last two entries (1, 0) and (0, 1)"""
    N = np.linalg.svd(A)[2][:, 7:, :]                       # [T, 2, 9], any basis
    with np.errstate(all="ignore"):
        C = np.linalg.inv(N[:, :, 7:])                      # (C N)[:, 7:] = I
        B = np.einsum("tij,tjk->tik", C, N)
    return B[:, 0], B[:, 1]


def null_gj(A):
    """the same by Gauss-Jordan with partial pivoting on columns 0 .. 6"""
    A = A.copy()
    T = np.arange(len(A))
    with np.errstate(all="ignore"):
        for c in range(7):
            piv = c + np.argmax(np.abs(A[:, c:, c]), axis=1)
            tmp = A[T, piv].copy()
            A[T, piv] = A[:, c]
            A[:, c] = tmp
            A[:, c] = A[:, c] / A[:, c, c][:, None]
            for i in range(7):
                if i != c:
                    A[:, i] = A[:, i] - A[:, i, c][:, None] * A[:, c]
    F1 = np.concatenate([-A[:, :, 7], np.ones((len(A), 1)), np.zeros((len(A), 1))], 1)
    F2 = np.concatenate([-A[:, :, 8], np.zeros((len(A), 1)), np.ones((len(A), 1))], 1)
    return F1, F2


def det3(a, b, c):
    return a[..., 0] * (b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]) - a[..., 1] * (b[..., 0] * c[..., 2] - b[..., 2] * c[..., 0]) \
        + a[..., 2] * (b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0])


def cubic_roots(c3, c2, c1, c0):
    """the cubic rule of rr.h for one cubic -> ascending real roots (0, 1 or 3 of them)"""
    if not (np.isfinite([c3, c2, c1, c0]).all() and abs(c3) > 0):
        return []
    a, b, c = c2 / c3, c1 / c3, c0 / c3
    Q = (a * a - 3 * b) / 9
    R = (2 * a ** 3 - 9 * a * b + 27 * c) / 54
    if not np.isfinite([Q, R, Q ** 3, R * R]).all():
        return []
    if R * R < Q ** 3:
        th = np.arccos(np.clip(R / np.sqrt(Q ** 3), -1.0, 1.0))
        return [-2 * np.sqrt(Q) * np.cos((th + 2 * np.pi * k) / 3) - a / 3 for k in (0, -1, 1)]
    A = -np.sign(R) * np.cbrt(abs(R) + np.sqrt(R * R - Q ** 3))
    B = Q / A if A != 0 else 0.0
    x = A + B - a / 3
    return [x] if np.isfinite(x) else []


def seven_point(q, null=null_svd):
    """q [T, 7, 4] records -> F [T, 3, 3, 3] (root, then the matrix; zeros where there is no such
    root or it is not finite), nroots [T]"""
    T = len(q)
    T1 = np.empty((T, 3, 3))
    T2 = np.empty((T, 3, 3))
    A = np.empty((T, 7, 9))
    for t in range(T):
        a, T1[t] = normalize_points(q[t, :, :2])
        b, T2[t] = normalize_points(q[t, :, 2:])
        A[t] = design(a, b)
    F1, F2 = null(A)
    F1, F2 = F1.reshape(T, 3, 3), F2.reshape(T, 3, 3)
    D = F1 - F2
    with np.errstate(all="ignore"):
        c0 = det3(F2[:, 0], F2[:, 1], F2[:, 2])
        c1 = det3(D[:, 0], F2[:, 1], F2[:, 2]) + det3(F2[:, 0], D[:, 1], F2[:, 2]) + det3(F2[:, 0], F2[:, 1], D[:, 2])
        c2 = det3(F2[:, 0], D[:, 1], D[:, 2]) + det3(D[:, 0], F2[:, 1], D[:, 2]) + det3(D[:, 0], D[:, 1], F2[:, 2])
        c3 = det3(D[:, 0], D[:, 1], D[:, 2])
    out = np.zeros((T, 3, 3, 3))
    nroots = np.zeros(T, dtype=np.int64)
    for t in range(T):
        with np.errstate(all="ignore"):
            lam = cubic_roots(c3[t], c2[t], c1[t], c0[t])
        nroots[t] = len(lam)
        for k, l in enumerate(lam):
            F = T2[t].T @ (F2[t] + l * D[t]) @ T1[t]
            if np.isfinite(F).all():
                out[t, k] = F
    return out, nroots


# ---------------------------------------------------------------- rr_verify_pairs_epipolar restated
def epipolar_pair(kp1, kp2, match, p, th=TH, iters=512, refine=2, seed=0, null=null_svd):
    """One pair of rr_verify_pairs_epipolar in float64 -> dict(inliers, F [3, 3], mask bool [n1]) plus
    the generator's diagnostics: t, root (winner, -1 when none), runner (the best count of another
    hypothesis t), margin (the smallest | Sampson - th | met in any root of any hypothesis or
    refit), m, counts [iters, 3], nroots [iters], fit (the records the returned F was fitted to)."""
    n1, n2 = len(kp1), len(kp2)
    rows = np.nonzero((match >= 0) & (match < n2))[0]
    rec = np.concatenate([kp1[rows].astype(np.float64), kp2[match[rows]].astype(np.float64)], 1).reshape(-1, 4)
    m = len(rows)
    out = dict(inliers=0, F=np.zeros((3, 3)), mask=np.zeros(n1, dtype=bool), t=-1, root=-1, runner=0, margin=np.inf, m=m,
               counts=np.zeros((iters, 3), dtype=np.int64), nroots=np.zeros(iters, dtype=np.int64), fit=None)
    if m < 7:
        return out
    smp = draw_n(seed, p, np.arange(iters), m, 7)
    Fs, nroots = seven_point(rec[smp], null)
    ok, res = sampson(Fs, rec)                      # [T, 3, M]
    live = ok & np.isfinite(res)
    margin = np.abs(res[live] - th).min() if live.any() else np.inf
    counts = (ok & (res <= th)).sum(-1)             # [T, 3]; an all-zero F has den = 0: count 0
    out.update(margin=margin, counts=counts, nroots=nroots)
    if counts.max() == 0:
        return out
    flat = int(np.argmax(counts.reshape(-1)))       # the first of the highest count: (t asc, root asc)
    t, root = flat // 3, flat % 3
    out.update(t=t, root=root, runner=int(np.delete(counts.max(1), t).max()) if iters > 1 else 0)
    F, count, fit = Fs[t, root], int(counts[t, root]), rec[smp[t]]
    for _ in range(refine):
        ok, res = sampson(F, rec)
        S = ok & (res <= th)
        if S.sum() < 8:
            break
        F2 = fundamental(rec[S, :2], rec[S, 2:])
        if not np.isfinite(F2).all():
            break
        ok2, res2 = sampson(F2, rec)
        margin = min(margin, np.abs(res2[ok2] - th).min() if ok2.any() else np.inf)
        c2 = int((ok2 & (res2 <= th)).sum())
        if c2 < count:
            break
        F, count, fit = F2, c2, rec[S]
    ok, res = sampson(F, rec)
    out["mask"][rows[ok & (res <= th)]] = True
    out.update(inliers=count, F=unit(F), margin=margin, fit=fit)
    return out


def epipolar_batch(kp1, off1, kp2, off2, match, th=TH, iters=512, refine=2, seed=0, null=null_svd):
    """the ragged batch -> (inliers int32 [P], F [P, 3, 3], mask bool [rows1], per-pair dicts)"""
    npairs = len(off1) - 1
    inl = np.zeros(npairs, dtype=np.int32)
    Fs = np.zeros((npairs, 3, 3))
    mask = np.zeros(len(kp1), dtype=bool)
    infos = []
    for p in range(npairs):
        a, b = slice(off1[p], off1[p + 1]), slice(off2[p], off2[p + 1])
        o = epipolar_pair(kp1[a], kp2[b], match[a], p, th, iters, refine, seed, null)
        inl[p], Fs[p], mask[a] = o["inliers"], o["F"], o["mask"]
        infos.append(o)
    return inl, Fs, mask, infos
