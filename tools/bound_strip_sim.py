"""CPU replay of the one-coordinate strip bound (DESIGN.md §4 "Strip pre-stage"): per hypothesis the count of
points with |ex| <= C Wcap(tile) (x strip) or |ey| <= C Wcap(tile) (y strip), in ransac_tiles_kernel's
source-local tile order, next to the capped diamond hi1 and the exact count.  Setup as in
tools/bound_cap_sim.py (same hypotheses, thr^2 = 25 + 0.5, no E slack, uniform sampling).  Per problem and
strip coordinate: the mean, standard deviation and the 99th / 99.9th percentile and the maximum of the strip count over the
hypotheses whose exact count is below 50 (no planted model), the share of those above 100 and above the
planted level - 1, and where the good hypotheses (exact count >= 100) rank among all strip counts, largest
first: the pilot takes the top few, so the rank of the best good hypothesis must be below that number.
    python tools/bound_strip_sim.py c4 > profiles/bound_strip_sim_c4.txt
"""
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from computervision_objectdetection_featurematching_amd.synthetic import CONFIGS, make_config_dataset  # noqa: E402
from tools.bound_cap_sim import check_subset, solve_h, tile_order  # noqa: E402


def strip_counts(H, src, dst, order):
    x, y, u, v = src[order, 0], src[order, 1], dst[order, 0], dst[order, 1]
    n = len(x)
    tile = np.arange(n) // 32
    mn = lambda a: np.minimum.reduceat(a, np.arange(0, n, 32))
    mx = lambda a: np.maximum.reduceat(a, np.arange(0, n, 32))
    cx, cy = 0.5 * (mn(x) + mx(x)), 0.5 * (mn(y) + mx(y))
    rx, ry = mx(x) - cx, mx(y) - cy
    r = np.sqrt(2) * np.sqrt(25.5)
    out = [np.zeros(len(H), int) for _ in range(4)]
    for a in range(0, len(H), 1000):
        h = H[a:a + 1000]
        X = h[:, 0:1] * x + h[:, 1:2] * y + h[:, 2:3]
        Y = h[:, 3:4] * x + h[:, 4:5] * y + h[:, 5:6]
        W = h[:, 6:7] * x + h[:, 7:8] * y + 1
        ex, ey = np.abs(X - u * W), np.abs(Y - v * W)
        R = r * (np.abs(h[:, 6:7] * cx + h[:, 7:8] * cy + 1) + np.abs(h[:, 6:7]) * rx + np.abs(h[:, 7:8]) * ry)[:, tile]
        out[0][a:a + 1000] = (ex ** 2 + ey ** 2 <= 25.0 * W * W).sum(1)
        out[1][a:a + 1000] = (ex + ey <= R).sum(1)
        out[2][a:a + 1000] = (ex <= R).sum(1)
        out[3][a:a + 1000] = (ey <= R).sum(1)
    return out


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "c4"
    scenes = [int(a) for a in sys.argv[2:]] or [0, 1, 3, 5]
    cfg = CONFIGS[name]
    nh = 46000 if cfg["max_iters"] > 4096 else cfg["max_iters"] - 512
    rng = np.random.default_rng(1)
    print(f"# {name}: {nh} hypotheses per problem, source-local tiles; bad = exact count < 50, good = exact >= 100")
    for s in scenes:
        ds = make_config_dataset(name, scene_ids=[s])
        pos = ds.plant_pos[0][0]
        src = ds.model_kp[0][:len(pos)].astype(np.float64)
        dst = ds.scene_kp[0][pos].astype(np.float64)
        if len(src) < 128:
            continue
        n = len(src)
        H = []
        while sum(len(h) for h in H) < nh:
            idx = np.array([rng.choice(n, 4, replace=False) for _ in range(8000)])
            k = check_subset(src[idx], dst[idx])
            H.append(solve_h(src[idx][k], dst[idx][k]))
        H = np.concatenate(H)[:nh]
        exact, cap, sx, sy = strip_counts(H, src, dst, tile_order(src))
        good = exact >= 100
        bad = exact < 50
        lvl = exact.max() - 1
        print(f"{name} scene {s} n {n} good hypotheses {good.sum()} best exact {exact.max()} mean hi1 {cap[bad].mean():.2f}")
        for nm, c in (("x", sx), ("y", sy)):
            order = np.argsort(-c, kind="stable")
            rank = np.nonzero(good[order])[0]
            q = np.percentile(c[bad], [50, 99, 99.9])
            print(f"  strip {nm}: bad mean {c[bad].mean():7.2f} sd {c[bad].std():.1f} median {q[0]:.0f} p99 {q[1]:.0f} p99.9 {q[2]:.0f} max {c[bad].max()} "
                  f"share > 100 {(c[bad] > 100).mean():.5f} share > {lvl} {(c[bad] > lvl).mean():.5f} "
                  f"(count {(c[bad] > lvl).sum()}); good: strip counts {[int(v) for v in sorted(c[good])[:4]]} ranks {[int(v) for v in rank[:4]]}")


if __name__ == "__main__":
    main()
