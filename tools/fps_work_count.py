"""What the pruned farthest-point-sampling kernel (gaussianformer_amd/csrc/fps.hip) does per pick, counted on the CPU by
replaying its bucket structure: a 32^3 Morton counting sort (stable here; the kernel's order within a cell differs, the
counts barely), buckets of 64, bucket j on wave j mod 16, the box bound against the bucket's largest d.  Prints, per
phase of the run, the mean number of buckets updated per pick and the mean over picks of the largest number any one wave
updates (the waves run in parallel, so that is the critical path).  DESIGN.md §3.8.

    python tools/fps_work_count.py [M]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianformer_amd.synthetic import make_lifter_points  # noqa: E402


def morton_order(p):
    lo, hi = p.min(0), p.max(0)
    scale = np.where(hi > lo, np.float32(32.0) / (hi - lo), 0).astype(np.float32)
    cell = np.clip(((p - lo) * scale), 0, 31).astype(np.int64)
    key = np.zeros(len(p), np.int64)
    for b in range(5):
        for c in range(3):
            key |= ((cell[:, c] >> b) & 1) << (3 * b + c)
    return np.argsort(key, kind="stable")


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
    p = make_lifter_points(seed=0)
    order = morton_order(p)
    q = p[order]
    n = len(q)
    nbk = (n + 63) // 64
    pad = nbk * 64 - n
    qb = np.concatenate([q, np.repeat(q[-1:], pad, 0)]).reshape(nbk, 64, 3)
    lo, hi = qb.min(1), qb.max(1)
    d = np.full(nbk * 64, 1e10, np.float32)
    d[n:] = 0
    wave = np.arange(nbk) % 16
    cur = int(np.flatnonzero(order == 0)[0])
    tot, crit = [], []
    for _ in range(m - 1):
        c = q[cur]
        g = np.maximum(np.maximum(lo - c, c - hi), 0)
        lb = g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]
        act = lb < d.reshape(nbk, 64).max(1)
        tot.append(int(act.sum()))
        crit.append(int(np.bincount(wave[act], minlength=16).max()))
        rows = np.flatnonzero(act)
        pts = qb[rows].reshape(-1, 3) - c
        dist = pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1] + pts[:, 2] * pts[:, 2]
        sl = (rows[:, None] * 64 + np.arange(64)).reshape(-1)
        d[sl] = np.minimum(d[sl], np.where(sl < n, dist, 0))
        cur = int(np.argmax(d))
    tot, crit = np.array(tot), np.array(crit)
    for a, b in ((0, 100), (100, 1000), (1000, m - 1)):
        if a < len(tot):
            print(f"picks {a + 1}-{min(b, len(tot))}: buckets updated per pick {tot[a:b].mean():.1f}, "
                  f"busiest wave {crit[a:b].mean():.2f}")
    print(f"all {len(tot)} picks: buckets updated per pick {tot.mean():.1f}, busiest wave {crit.mean():.2f} "
          f"(of {nbk} buckets, {int(np.ceil(nbk / 16))} per wave)")


if __name__ == "__main__":
    main()
