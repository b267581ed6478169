"""Timing of batched relative pose (rr_recover_pose, cirtorch.search.recover_pose) beside a torch
composition of the same steps on the device (torch.linalg.svd for the 3 x 3 of every pair and for the
4 x 4 of every used correspondence under each of the four candidate motions), in the same process and
on the same pairs: the re-ranking shape k = 100 x Q = 128 -> P = 12 800 pairs of N1 = N2 = 2048
keypoints, 600 rows matched of which about 300 are the verified inliers (planted correspondences of
the pair's two-view scene, 0.3 px noise; `mask` marks them, F is the scene's).  --distinct scenes are
generated and repeated to P pairs.  HIP events around every call, warm-up, median and min-max.
    python tools/pose_probe.py [--reps 10] [--pairs 12800] [--n 2048] [--torch-pairs 64] [--out profiles/pose_probe.json]
The torch composition materialises 4 x M 4 x 4 systems and their SVD factors per pair, so it runs on
the first --torch-pairs pairs only; both paths are reported per pair as well.
Prints (and writes to --out) one JSON line:
  engine_us (+ _min_max)          one recover_pose call over all P pairs
  engine_us_per_pair
  torch_us (+ _min_max)           the composition over --torch-pairs pairs
  torch_us_per_pair, ratio        ratio = torch_us_per_pair / engine_us_per_pair
  front_equal, max_R_diff, max_t_diff   the two paths agree on those pairs
Developer tool; A/B two builds with RR_LIB.
"""

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "image-retrieval-for-image-based-localization_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_pairs(p, n, matched, distinct, seed):
    """kp1, kp2 float32 [p, n, 2], match int64 [p, n], mask bool [p, n], F float64 [p, 3, 3]"""
    import epipolar_cases as EC
    parts = [EC.planted_pair(n, n, matched, 0.5, 0.3, seed + i) for i in range(distinct)]
    idx = np.arange(p) % distinct
    kp1, kp2, match, mask = (np.stack([q[i] for q in parts])[idx] for i in range(4))
    return kp1, kp2, match, mask, np.stack([EC.unit(q[4]) for q in parts])[idx]


def torch_pose(kp1, kp2, match, mask, F, K1, K2, m_max):
    """the steps of rr.h in torch on the device: -> R [P, 3, 3], t [P, 3], front [P]"""
    p, n1 = match.shape
    use = (match >= 0) & mask
    order = torch.argsort(use.to(torch.int8), dim=1, descending=True, stable=True)[:, :m_max]     # the used rows first
    valid = torch.gather(use, 1, order)
    j = torch.gather(match, 1, order).clamp(min=0)
    x1 = torch.gather(kp1, 1, order[..., None].expand(-1, -1, 2)).double()
    x2 = torch.gather(kp2, 1, j[..., None].expand(-1, -1, 2)).double()
    E0 = K2.transpose(1, 2) @ F @ K1
    U, _, Vh = torch.linalg.svd(E0)
    U = torch.cat([U[..., :2], torch.linalg.cross(U[..., 0], U[..., 1])[..., None]], -1)          # det +1
    V = Vh.transpose(1, 2)
    V = torch.cat([V[..., :2], torch.linalg.cross(V[..., 0], V[..., 1])[..., None]], -1)
    W = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64, device=F.device)
    Ra, Rb, t = U @ W @ V.transpose(1, 2), U @ W.T @ V.transpose(1, 2), U[..., 2]
    Rs = torch.stack([Ra, Ra, Rb, Rb], 1)                                                         # [P, 4, 3, 3]
    ts = torch.stack([t, -t, t, -t], 1)                                                           # [P, 4, 3]
    P1 = torch.cat([K1, torch.zeros(p, 3, 1, dtype=torch.float64, device=F.device)], 2)[:, None]  # [P, 1, 3, 4]
    P2 = K2[:, None] @ torch.cat([Rs, ts[..., None]], 3)                                          # [P, 4, 3, 4]
    a, b = x1[:, None], x2[:, None]                                                               # [P, 1, M, 2]
    rows = [a[..., 0:1] * P1[:, :, None, 2] - P1[:, :, None, 0], a[..., 1:2] * P1[:, :, None, 2] - P1[:, :, None, 1],
            b[..., 0:1] * P2[:, :, None, 2] - P2[:, :, None, 0], b[..., 1:2] * P2[:, :, None, 2] - P2[:, :, None, 1]]
    A = torch.stack([r.expand(p, 4, m_max, 4) for r in rows], -2)                                 # [P, 4, M, 4, 4]
    h = torch.linalg.svd(A)[2][..., -1, :]                                                        # [P, 4, M, 4]
    w = h[..., 3:]
    X = h[..., :3] * torch.where(w.abs() > 1e-8, 1.0 / w, torch.ones_like(w))
    d2 = (X @ Rs.transpose(2, 3))[..., 2] + ts[..., None, 2]
    front = ((X[..., 2] > 0) & (d2 > 0) & valid[:, None]).sum(-1)                                 # [P, 4]
    win = front.argmax(1)
    pick = win[:, None, None, None]
    return torch.gather(Rs, 1, pick.expand(-1, 1, 3, 3))[:, 0], torch.gather(ts, 1, pick[..., 0].expand(-1, 1, 3))[:, 0], \
        front.gather(1, win[:, None])[:, 0]


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return 1000 * t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=12800)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--matched", type=int, default=600)
    ap.add_argument("--distinct", type=int, default=128)
    ap.add_argument("--torch-pairs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pose_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_probe needs a GPU")
    import epipolar_cases as EC
    from cirtorch import _engine as E
    from cirtorch.search import recover_pose
    from tools.src_digest import digest
    kp1, kp2, match, mask, F = make_pairs(args.pairs, args.n, args.matched, min(args.distinct, args.pairs), 2700)
    d1, d2, dm, dk, dF = (torch.from_numpy(a).cuda() for a in (kp1, kp2, match, mask, F))
    K = torch.from_numpy(EC.K).cuda()
    q = min(args.torch_pairs, args.pairs)
    Kq = K[None].expand(q, 3, 3).contiguous()
    m_max = int(mask[:q].sum(1).max())
    run = {"engine": lambda: recover_pose(d1, d2, dm, dF, K, K, mask=dk),
           "torch": lambda: torch_pose(d1[:q], d2[:q], dm[:q], dk[:q], dF[:q], Kq, Kq, m_max)}
    times = {m: [] for m in run}
    for r in range(args.warmup + args.reps):
        for m in run:
            t = once(run[m])
            if r >= args.warmup:
                times[m].append(t)
    R, t, _, _, front = run["engine"]()
    Rt, tt, ft = run["torch"]()
    med = {m: statistics.median(times[m]) for m in run}
    out = {"pairs": args.pairs, "n": args.n, "matched": args.matched, "distinct": min(args.distinct, args.pairs),
           "mean_used": round(float(mask.sum(1).mean()), 1), "torch_pairs": q, "reps": args.reps,
           "build": E.lib().rr_build_info().decode(), "tree_digest": digest(), "device": E.device_arch()}
    for m in run:
        out[m + "_us"] = round(med[m], 1)
        out[m + "_us_min_max"] = [round(min(times[m]), 1), round(max(times[m]), 1)]
    out["engine_us_per_pair"] = round(med["engine"] / args.pairs, 3)
    out["torch_us_per_pair"] = round(med["torch"] / q, 3)
    out["ratio"] = round(out["torch_us_per_pair"] / out["engine_us_per_pair"], 1)
    out["mean_front"] = round(float(front.float().mean().item()), 1)
    out["front_equal"] = bool(torch.equal(front[:q].long(), ft.long()))
    out["max_R_diff"] = float((R[:q] - Rt).abs().max().item())
    out["max_t_diff"] = float((t[:q, :, 0] - tt).abs().max().item())
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
