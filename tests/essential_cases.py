"""Shared by tests/golden/make_golden_essential.py and the essential-matrix tests: planted two-view
scenes (general, planar, two different cameras) and a float64 numpy restatement of
rr_verify_pairs_essential (steps a - e of include/rr.h) and rr_essential_5pt, written from the
header, with two independent five-point solvers:
  A  null space by np.linalg.svd, the 10 x 20 constraint matrix reduced by np.linalg.solve in
     Stewenius' monomial order, the 10 x 10 action matrix of x and np.linalg.eig; its refit takes
     the singular vector of the design matrix where B takes the eigenvector of the normal matrix;
  B  the header's construction: the orthonormal null-space basis by Householder reflections, Nister's
     elimination to the degree-10 polynomial in z and np.roots.
The upstream project has no five-point solver: nothing here is compared with it.  numpy only."""

import numpy as np

import epipolar_cases as EC
import pose_cases as PC

K = EC.K
K2B = np.array([[700.0, 0.0, 480.0], [0.0, 720.0, 400.0], [0.0, 0.0, 1.0]])   # the second camera of the two-camera scenes
TH = EC.TH
RUN_SEED = EC.RUN_SEED
STAGE = EC.STAGE
ESS_SEED = 8700
NEAR = 1e-4           # a sample with two roots this close (relative) to each other or to the real axis is dropped
REAL = 1e-9           # |imag| <= REAL max(1, |z|): a real root

# pairs: (n1, n2, kept matches M, planted fraction, noise px, kind); th 1.5 px everywhere
ESS_CASES = [
    dict(name="m0", pairs=[(20, 25, 0, 0.0, 0.3, "general")], iters=256, refine=2),
    dict(name="m4", pairs=[(20, 25, 4, 1.0, 0.3, "general")], iters=256, refine=2),
    dict(name="m5", pairs=[(12, 14, 5, 1.0, 0.3, "general")], iters=256, refine=2),
    dict(name="m8", pairs=[(12, 11, 8, 1.0, 0.3, "general")], iters=256, refine=2),
    dict(name="m40", pairs=[(70, 64, 40, 0.6, 0.3, "general")], iters=300, refine=2),
    dict(name="m257_r0", pairs=[(300, 310, 257, 0.6, 0.3, "general")], iters=300, refine=0),
    dict(name="m257_r2", pairs=[(300, 310, 257, 0.6, 0.3, "general")], iters=256, refine=2),
    dict(name="m1025", pairs=[(1100, 1060, STAGE + 1, 0.6, 0.3, "general")], iters=256, refine=2),
    dict(name="iters1", pairs=[(70, 64, 40, 1.0, 0.3, "general")], iters=1, refine=2),
    dict(name="iters257", pairs=[(70, 64, 40, 0.6, 0.3, "general")], iters=257, refine=2),
    dict(name="outliers", pairs=[(80, 90, 60, 0.0, 0.3, "general")], iters=300, refine=2),
    dict(name="ragged4", pairs=[(0, 0, 0, 0.0, 0.3, "general"), (30, 28, 3, 1.0, 0.3, "general"),
                                (80, 90, 60, 0.0, 0.3, "general"), (60, 70, 50, 1.0, 0.0, "general")], iters=300, refine=2),
    dict(name="planar", pairs=[(90, 80, 60, 0.6, 0.3, "planar")], iters=300, refine=2),
    dict(name="twocam", pairs=[(90, 80, 60, 0.6, 0.3, "twocam")], iters=300, refine=2),
    dict(name="singularK", pairs=[(70, 64, 40, 0.6, 0.3, "general"), (70, 64, 40, 0.6, 0.3, "singular"),
                                  (70, 64, 40, 0.6, 0.3, "general"), (60, 66, 30, 0.7, 0.3, "twocam")], iters=256, refine=2),
]
# the cases with extra checks in the tests
EXACT_CASE = dict(name="exact", pairs=[(60, 70, 50, 1.0, 0.0, "general")], iters=300, refine=2)
CHAIN_CASE = dict(name="chain", pairs=[(130, 120, 100, 0.6, 0.3, "twocam")], iters=300, refine=2)
ALL_CASES = ESS_CASES + [EXACT_CASE, CHAIN_CASE]
SOLVER_N = 257        # samples of the minimal-solver test: a second block trip
SOLVER_SEED = 8900

checksum = EC.checksum


# ---------------------------------------------------------------- scenes
def planar_pair(n1, n2, m, frac, noise, seed):
    """EC.planted_pair with every 3-D point on the oblique plane n . X = 8, n = (0.2, -0.1, 1)
    -> kp1, kp2, match, planted, F_true, R, t, X [n1, 3]"""
    r = np.random.default_rng(seed)
    R = EC.rot(*r.uniform(-0.25, 0.25, 3))
    t = np.array([r.uniform(0.6, 1.2) * r.choice([-1, 1]), r.uniform(-0.3, 0.3), r.uniform(-0.5, 0.5)])
    nrm = np.array([0.2, -0.1, 1.0])
    kp1, img2, X = np.empty((0, 2)), np.empty((0, 2)), np.empty((0, 3))
    while len(kp1) < n1:
        px = r.uniform([0, 0], [EC.W, EC.H_IMG], (4 * n1 + 16, 2))
        ray = np.concatenate([(px - K[:2, 2]) / EC.FOCAL, np.ones((len(px), 1))], 1)
        P = ray * (8.0 / (ray @ nrm))[:, None]
        q, zz = EC.project(P, R, t)
        ok = EC.VC.inside(q) & (zz > 0.5)
        kp1, img2, X = np.concatenate([kp1, px[ok]]), np.concatenate([img2, q[ok]]), np.concatenate([X, P[ok]])
    kp1, img2, X = kp1[:n1], img2[:n1], X[:n1]
    kp2 = r.uniform([0, 0], [EC.W, EC.H_IMG], (n2, 2))
    match = np.full(n1, -1, dtype=np.int64)
    planted = np.zeros(n1, dtype=bool)
    rows = np.sort(r.permutation(n1)[:m])
    cols = r.permutation(n2)[:m]
    match[rows] = cols
    nin = int(round(frac * m))
    inl = r.permutation(m)[:nin]
    planted[rows[inl]] = True
    kp2[cols[inl]] = np.clip(img2[rows[inl]] + noise * r.standard_normal((nin, 2)), 0, [EC.W - 0.01, EC.H_IMG - 0.01])
    return kp1.astype(np.float32), kp2.astype(np.float32), match, planted, EC.true_fundamental(R, t), R, t, X


def scene(n1, n2, m, frac, noise, kind, seed):
    """-> dict(kp1, kp2, match, planted, F, R, t, X, K1, K2).  kind: "general" (EC.planted_pair),
    "planar", "twocam" (the second view through K2B), "singular" (general, but K1 has two equal rows)"""
    if kind == "planar":
        kp1, kp2, match, planted, F, R, t, X = planar_pair(n1, n2, m, frac, noise, seed)
        return dict(kp1=kp1, kp2=kp2, match=match, planted=planted, F=F, R=R, t=t, X=X, K1=K.copy(), K2=K.copy())
    s = PC.scene(n1, n2, m, frac, noise, seed, K2=K2B if kind == "twocam" else None)
    if kind == "singular":
        s["K1"] = np.array([[900.0, 0.0, 512.0], [900.0, 0.0, 512.0], [0.0, 0.0, 1.0]])
    return s


def build_case(case, seed):
    """the ragged batch of a case: kp1 [rows1, 2], off1 [P + 1], kp2, off2, match [rows1], planted [rows1],
    K1, K2 [P, 3, 3], scenes"""
    parts = [scene(n1, n2, m, f, nz, kind, seed + 17 * k) for k, (n1, n2, m, f, nz, kind) in enumerate(case["pairs"])]
    off1 = np.cumsum([0] + [len(q["kp1"]) for q in parts]).astype(np.int64)
    off2 = np.cumsum([0] + [len(q["kp2"]) for q in parts]).astype(np.int64)
    cat = lambda key, dt: np.concatenate([q[key] for q in parts]).astype(dt)  # noqa: E731
    return (cat("kp1", np.float32).reshape(-1, 2), off1, cat("kp2", np.float32).reshape(-1, 2), off2, cat("match", np.int64),
            cat("planted", bool), np.stack([q["K1"] for q in parts]), np.stack([q["K2"] for q in parts]), parts)


# ---------------------------------------------------------------- polynomials in (x, y, z)
def _pmul(a, b):
    """polynomials as {exponent triple: coefficients [T]}"""
    o = {}
    for ea, ca in a.items():
        for eb, cb in b.items():
            e = (ea[0] + eb[0], ea[1] + eb[1], ea[2] + eb[2])
            o[e] = o[e] + ca * cb if e in o else ca * cb
    return o


def _padd(a, b, s=1.0):
    o = dict(a)
    for e, c in b.items():
        o[e] = o[e] + s * c if e in o else s * c
    return o


STEWENIUS = [(3, 0, 0), (2, 1, 0), (1, 2, 0), (0, 3, 0), (2, 0, 1), (1, 1, 1), (0, 2, 1), (1, 0, 2), (0, 1, 2), (0, 0, 3),
             (2, 0, 0), (1, 1, 0), (0, 2, 0), (1, 0, 1), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
NISTER = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
          (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]


def constraints(N, order):
    """N [T, 4, 3, 3] (X, Y, Z, W) -> the 10 x 20 matrices [T, 10, 20] of det E = 0 and
    2 E E^T E - tr(E E^T) E = 0 (row-major) for E = x X + y Y + z Z + W, columns in `order`"""
    T = len(N)
    E = [[{(1, 0, 0): N[:, 0, r, c], (0, 1, 0): N[:, 1, r, c], (0, 0, 1): N[:, 2, r, c], (0, 0, 0): N[:, 3, r, c]}
          for c in range(3)] for r in range(3)]
    minor = lambda a, b, c, d: _padd(_pmul(a, d), _pmul(b, c), -1.0)  # noqa: E731
    det = _padd(_padd(_pmul(E[0][0], minor(E[1][1], E[1][2], E[2][1], E[2][2])),
                      _pmul(E[0][1], minor(E[1][0], E[1][2], E[2][0], E[2][2])), -1.0),
                _pmul(E[0][2], minor(E[1][0], E[1][1], E[2][0], E[2][1])))
    G = [[None] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(3):
            g = {}
            for k in range(3):
                g = _padd(g, _pmul(E[r][k], E[c][k]))
            G[r][c] = g
    tr = _padd(_padd(G[0][0], G[1][1]), G[2][2])
    rows = [det]
    for r in range(3):
        for c in range(3):
            q = {}
            for k in range(3):
                q = _padd(q, _pmul(G[r][k], E[k][c]), 2.0)
            rows.append(_padd(q, _pmul(tr, E[r][c]), -1.0))
    M = np.zeros((T, 10, 20))
    for i, row in enumerate(rows):
        for e, c in row.items():
            M[:, i, order.index(e)] = c
    return M


def design5(h1, h2):
    """h1, h2 [T, 5, 3] -> the 5 x 9 systems, entry 3 a + b = h2_a h1_b"""
    return np.einsum("tja,tjb->tjab", h2, h1).reshape(len(h1), 5, 9)


# ---------------------------------------------------------------- solver A
def five_point_a(h1, h2):
    """-> list over samples of E [n, 3, 3], scaled to W . E = 1 and in ascending z = Z . E of the header's
    orthonormal basis (the order of rr.h; the solutions themselves come from the SVD basis)"""
    T = len(h1)
    N = np.linalg.svd(design5(h1, h2))[2][:, 5:, :].reshape(T, 4, 3, 3)
    Nh = null_house(design5(h1, h2))
    M = constraints(N, STEWENIUS)
    out = []
    for t in range(T):
        try:
            Bm = np.linalg.solve(M[t, :, :10], M[t, :, 10:])
        except np.linalg.LinAlgError:
            out.append(np.zeros((0, 3, 3)))
            continue
        Ax = np.zeros((10, 10))
        for row, src in enumerate([0, 1, 2, 4, 5, 7]):
            Ax[row] = -Bm[src]
        Ax[6, 0] = Ax[7, 1] = Ax[8, 3] = Ax[9, 6] = 1
        if not np.isfinite(Ax).all():
            out.append(np.zeros((0, 3, 3)))
            continue
        w, v = np.linalg.eig(Ax)
        sol = []
        for k in range(10):
            if abs(w[k].imag) <= REAL * max(1.0, abs(w[k])):
                vv = v[:, k].real if abs(v[9, k].real) >= abs(v[9, k].imag) else v[:, k].imag
                x, y, z = vv[6] / vv[9], vv[7] / vv[9], vv[8] / vv[9]
                Em = x * N[t, 0] + y * N[t, 1] + z * N[t, 2] + N[t, 3]
                sol.append(Em / (Nh[t, 3] * Em).sum())
        sol.sort(key=lambda m: (Nh[t, 2] * m).sum())
        out.append(np.array(sol).reshape(-1, 3, 3))
    return out


# ---------------------------------------------------------------- solver B (the header's construction)
def null_house(A):
    """A [T, 5, 9] -> N [T, 4, 3, 3]: the orthonormal null vectors X, Y, Z, W = H_0 .. H_4 e_j, j = 5 .. 8,
    of the Householder reflections H_k = I - beta_k v_k v_k^T that make A^T upper triangular (rr.h step b.1)"""
    Bm = np.transpose(A, (0, 2, 1)).copy()      # [T, 9, 5]
    T = len(Bm)
    vs, betas = [], []
    with np.errstate(all="ignore"):
        for k in range(5):
            x = Bm[:, k:, k]
            nrm = np.sqrt((x ** 2).sum(1))
            v = x.copy()
            v[:, 0] += np.where(x[:, 0] < 0, -nrm, nrm)
            beta = 2.0 / (v ** 2).sum(1)
            Bm[:, k:, :] -= beta[:, None, None] * v[:, :, None] * np.einsum("ti,tij->tj", v, Bm[:, k:, :])[:, None, :]
            vs.append(v)
            betas.append(beta)
        N = np.zeros((T, 4, 9))
        for j in range(4):
            n = np.zeros((T, 9))
            n[:, 5 + j] = 1.0
            for k in range(4, -1, -1):
                n[:, k:] -= (betas[k] * (vs[k] * n[:, k:]).sum(1))[:, None] * vs[k]
            N[:, j] = n
    return N.reshape(T, 4, 3, 3)


def poly10(h1, h2):
    """-> N [T, 4, 3, 3], bx, by [T, 3, 4], bc [T, 3, 5] (ascending powers of z), c [T, 11]"""
    T = len(h1)
    N = null_house(design5(h1, h2))
    M = constraints(N, NISTER)
    bx, by, bc, c = np.full((T, 3, 4), np.nan), np.full((T, 3, 4), np.nan), np.full((T, 3, 5), np.nan), np.full((T, 11), np.nan)
    for t in range(T):
        try:
            with np.errstate(all="ignore"):
                Rm = np.linalg.solve(M[t, :, :10], M[t, :, 10:])    # columns 10 .. 19 of the reduced rows
        except np.linalg.LinAlgError:
            continue
        for r in range(3):
            p, q = Rm[4 + 2 * r], Rm[5 + 2 * r]
            bx[t, r] = [p[2], p[1] - q[2], p[0] - q[1], -q[0]]
            by[t, r] = [p[5], p[4] - q[5], p[3] - q[4], -q[3]]
            bc[t, r] = [p[9], p[8] - q[9], p[7] - q[8], p[6] - q[7], -q[6]]
        P = np.polynomial.polynomial
        m = lambda a, b: P.polymul(a, b)  # noqa: E731
        d = P.polyadd(P.polysub(m(bx[t, 0], P.polysub(m(by[t, 1], bc[t, 2]), m(by[t, 2], bc[t, 1]))),
                                m(by[t, 0], P.polysub(m(bx[t, 1], bc[t, 2]), m(bx[t, 2], bc[t, 1])))),
                      m(bc[t, 0], P.polysub(m(bx[t, 1], by[t, 2]), m(bx[t, 2], by[t, 1]))))
        c[t, :len(d)] = d
        c[t, len(d):] = 0.0
    return N, bx, by, bc, c


def real_roots(c):
    """c [11] ascending -> (ascending real roots, near): near = two roots within NEAR (relative) of each
    other, or a complex root within NEAR of the real axis"""
    if not (np.isfinite(c).all() and abs(c[10]) > 0 and np.isfinite(c[:10] / c[10]).all()):
        return np.zeros(0), False
    w = np.roots(c[::-1])
    rel = np.abs(w.imag) / np.maximum(1.0, np.abs(w))
    real = np.sort(w[rel <= REAL].real)
    near = bool(((rel > REAL) & (rel < NEAR)).any())
    if len(real) > 1:
        near = near or bool((np.diff(real) / np.maximum(1.0, np.abs(real[1:]))).min() < NEAR)
    return real, near


def five_point_b(h1, h2):
    """-> (list over samples of E [n, 3, 3] = x X + y Y + z Z + W in ascending root order, near [T])"""
    N, bx, by, bc, c = poly10(h1, h2)
    out, near = [], np.zeros(len(h1), dtype=bool)
    for t in range(len(h1)):
        z, near[t] = real_roots(c[t])
        sol = []
        for zz in z:
            pw = zz ** np.arange(5)
            rows = np.stack([bx[t] @ pw[:4], by[t] @ pw[:4], bc[t] @ pw], 1)    # [3 rows, (x, y, 1)]
            cr = [np.cross(rows[0], rows[1]), np.cross(rows[0], rows[2]), np.cross(rows[1], rows[2])]
            n = cr[0]
            for k in (1, 2):
                if abs(cr[k][2]) > abs(n[2]):
                    n = cr[k]
            with np.errstate(all="ignore"):
                x, y = n[0] / n[2], n[1] / n[2]
            sol.append(x * N[t, 0] + y * N[t, 1] + zz * N[t, 2] + N[t, 3])
        out.append(np.array(sol).reshape(-1, 3, 3))
    return out, near


def solve(h1, h2, solver):
    return five_point_a(h1, h2) if solver == "A" else five_point_b(h1, h2)[0]


# ---------------------------------------------------------------- rr_essential_5pt restated
def unit_all(Es):
    return np.array([EC.unit(e) for e in Es]).reshape(-1, 3, 3)


def solver_samples(seed=SOLVER_SEED, n=SOLVER_N):
    """-> x1, x2 [n', 5, 2] float64 normalised points from general, planar and two-camera scenes (one
    third each), the oracle's E [n', 10, 3, 3] (unit norm, largest entry positive, ascending root
    order, zeros past nroots), nroots [n'], the share of dropped (near-degenerate) samples, the
    largest A - B difference of every sample [n'], the oracle's largest |h2^T E h1|"""
    r = np.random.default_rng(seed)
    h1s, h2s = [], []
    for i in range(n):
        kind = ("general", "planar", "twocam")[i % 3]
        s = scene(40, 40, 40, 1.0, 0.3, kind, int(r.integers(1 << 30)))
        rows = r.permutation(40)[:5]
        a = np.concatenate([s["kp1"][rows].astype(np.float64), np.ones((5, 1))], 1) @ np.linalg.inv(s["K1"]).T
        b = np.concatenate([s["kp2"][s["match"][rows]].astype(np.float64), np.ones((5, 1))], 1) @ np.linalg.inv(s["K2"]).T
        h1s.append(a / a[:, 2:])
        h2s.append(b / b[:, 2:])
    h1, h2 = np.array(h1s), np.array(h2s)
    Eb, near = five_point_b(h1, h2)
    Ea = five_point_a(h1, h2)
    keep = ~near
    E = np.zeros((n, 10, 3, 3))
    nroots = np.zeros(n, dtype=np.int32)
    diffs, resid = np.zeros(n), 0.0
    for t in range(n):
        if not keep[t]:
            continue
        assert len(Ea[t]) == len(Eb[t]), (t, len(Ea[t]), len(Eb[t]))
        nroots[t] = len(Eb[t])
        E[t, :nroots[t]] = unit_all(Eb[t])
        for k in range(nroots[t]):
            diffs[t] = max(diffs[t], EC.f_err(Ea[t][k], Eb[t][k]))
            resid = max(resid, float(np.abs(np.einsum("ja,ab,jb->j", h2[t], E[t, k], h1[t])).max()))
    return (np.ascontiguousarray(h1[keep, :, :2]), np.ascontiguousarray(h2[keep, :, :2]), E[keep], nroots[keep],
            float(near.mean()), diffs[keep], resid)


# ---------------------------------------------------------------- rr_verify_pairs_essential restated
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


def project_essential(Em):
    """U diag(s, s, 0) V^T, s = (s1 + s2) / 2"""
    U, S, Vt = np.linalg.svd(Em)
    s = 0.5 * (S[0] + S[1])
    return U @ np.diag([s, s, 0.0]) @ Vt


def fundamental_svd(p1, p2):
    """EC.fundamental by another route: the last right singular vector of the design matrix itself
    (not the eigenvector of X^T X) and np.linalg.svd for the rank-2 projection -- solver A's refit"""
    q1, T1 = EC.normalize_points(p1)
    q2, T2 = EC.normalize_points(p2)
    f = np.linalg.svd(EC.design(q1, q2))[2][-1].reshape(3, 3)
    U, S, Vt = np.linalg.svd(f)
    F = T2.T @ (U @ np.diag([S[0], S[1], 0.0]) @ Vt) @ T1
    return F / (F[2, 2] + EC.EPS) if abs(F[2, 2]) > EC.EPS else F


def essential_pair(kp1, kp2, match, Ka, Kb, p, th=TH, iters=256, refine=2, seed=0, solver="B"):
    """One pair of rr_verify_pairs_essential in float64 -> dict(inliers, E [3, 3], mask bool [n1]) plus the
    generator's diagnostics: t, root (winner, -1 when none), margin (the smallest | Sampson - th | met in
    any root of any hypothesis or refit), m, counts [iters, 10], nroots [iters], F (the winner in pixels)"""
    n1, n2 = len(kp1), len(kp2)
    rows = np.nonzero((match >= 0) & (match < n2))[0]
    rec = np.concatenate([kp1[rows].astype(np.float64), kp2[match[rows]].astype(np.float64)], 1).reshape(-1, 4)
    m = len(rows)
    out = dict(inliers=0, E=np.zeros((3, 3)), mask=np.zeros(n1, dtype=bool), t=-1, root=-1, margin=np.inf, m=m,
               counts=np.zeros((iters, 10), dtype=np.int64), nroots=np.zeros(iters, dtype=np.int64), F=np.zeros((3, 3)))
    i1, ok1 = inv_adj(Ka)
    i2, ok2 = inv_adj(Kb)
    if m < 5 or not (ok1 and ok2):
        return out
    smp = EC.draw_n(seed, p, np.arange(iters), m, 5)
    q = rec[smp]                                                   # [T, 5, 4]
    one = np.ones(q.shape[:2] + (1,))
    h1 = np.concatenate([q[..., :2], one], -1) @ i1.T
    h2 = np.concatenate([q[..., 2:], one], -1) @ i2.T
    Es = solve(h1, h2, solver)
    Fs = np.zeros((iters, 10, 3, 3))
    nroots = np.array([len(e) for e in Es])
    for t in range(iters):
        for k in range(len(Es[t])):
            with np.errstate(all="ignore"):
                F = i2.T @ Es[t][k] @ i1
            if np.isfinite(F).all():
                Fs[t, k] = F
    okk, res = EC.sampson(Fs, rec)                                  # [T, 10, M]
    live = okk & np.isfinite(res)
    margin = np.abs(res[live] - th).min() if live.any() else np.inf
    counts = (okk & (res <= th)).sum(-1)
    out.update(margin=margin, counts=counts, nroots=nroots)
    if counts.max() == 0:
        return out
    flat = int(np.argmax(counts.reshape(-1)))
    t, root = flat // 10, flat % 10
    out.update(t=t, root=root)
    F, count = Fs[t, root], int(counts[t, root])
    for _ in range(refine):
        okk, res = EC.sampson(F, rec)
        S = okk & (res <= th)
        if S.sum() < 8:
            break
        F1 = fundamental_svd(rec[S, :2], rec[S, 2:]) if solver == "A" else EC.fundamental(rec[S, :2], rec[S, 2:])
        with np.errstate(all="ignore"):
            E1 = Kb.T @ F1 @ Ka
            if not np.isfinite(E1).all():
                break
            F2 = i2.T @ project_essential(E1) @ i1
        if not np.isfinite(F2).all():
            break
        ok2_, res2 = EC.sampson(F2, rec)
        margin = min(margin, np.abs(res2[ok2_] - th).min() if ok2_.any() else np.inf)
        c2 = int((ok2_ & (res2 <= th)).sum())
        if c2 < count:
            break
        F, count = F2, c2
    okk, res = EC.sampson(F, rec)
    out["mask"][rows[okk & (res <= th)]] = True
    out.update(inliers=count, E=EC.unit(project_essential(Kb.T @ F @ Ka)), margin=margin, F=F)
    return out


def essential_batch(kp1, off1, kp2, off2, match, K1, K2, th=TH, iters=256, refine=2, seed=0, solver="B"):
    """the ragged batch -> (inliers int32 [P], E [P, 3, 3], mask bool [rows1], per-pair dicts)"""
    npairs = len(off1) - 1
    inl = np.zeros(npairs, dtype=np.int32)
    Es = np.zeros((npairs, 3, 3))
    mask = np.zeros(len(kp1), dtype=bool)
    infos = []
    for p in range(npairs):
        a, b = slice(off1[p], off1[p + 1]), slice(off2[p], off2[p + 1])
        o = essential_pair(kp1[a], kp2[b], match[a], K1[p], K2[p], p, th, iters, refine, seed, solver)
        inl[p], Es[p], mask[a] = o["inliers"], o["E"], o["mask"]
        infos.append(o)
    return inl, Es, mask, infos
