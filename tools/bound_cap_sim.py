"""CPU replay of the capped bound's selectivity (DESIGN.md §4 "Capped bound, then the full one"): which
share of a chunk's hypotheses keeps more points than the bar when |W| is replaced, per 32-point tile, by
its cap over the tile's source box.  The tiles are ordered as ransac_tiles_kernel orders them (x-strips of
about equal count from a 1,024-bin histogram, 64 snaked y bins per strip, ties by point index); "match
order" is the order before this change.  Per problem: the planted matches as the good set, random
4-samples that pass OpenCV's orientation test, H from the 8x8 solve, thr^2 = 25 + 0.5, C = sqrt 2 r, no E
slack, uniform sampling (not cv::RNG's stream).  The bar is chunk 1's best exact count (4,096
hypotheses at maxIters 50,000, 512 below).
    python tools/bound_cap_sim.py c4 > profiles/bound_cap_sim_c4.txt      (c3, c2 likewise)
"""
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from computervision_objectdetection_featurematching_amd.synthetic import CONFIGS, make_config_dataset  # noqa: E402

XB, YB, SMAX = 1024, 64, 32


def tile_order(src):
    """Row order of ransac_tiles_kernel (fp32 binning as on the device)."""
    x, y = src[:, 0].astype(np.float32), src[:, 1].astype(np.float32)
    n = len(x)
    nt = (n + 31) // 32
    ns = 1
    while ns < SMAX and (2 * ns + 1) ** 2 <= 4 * nt:
        ns += 1
    x0, x1, y0, y1 = x.min(), x.max(), y.min(), y.max()
    invx = np.float32(XB) / (x1 - x0) if x1 > x0 else np.float32(0)
    invy = np.float32(YB) / (y1 - y0) if y1 > y0 else np.float32(0)
    xb = np.clip(((x - x0) * invx).astype(np.int64), 0, XB - 1)
    yb = np.clip(((y - y0) * invy).astype(np.int64), 0, YB - 1)
    c = np.bincount(xb, minlength=XB)
    base = np.cumsum(c) - c
    strip = np.minimum(ns - 1, (2 * base + c) * ns // (2 * n))[xb]
    key = strip * YB + np.where(strip & 1, YB - 1 - yb, yb)
    return np.lexsort((np.arange(n), key))


def check_subset(s, d):
    neg = np.zeros(len(s), int)
    for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        def det(p):
            return (p[:, b, 0] - p[:, a, 0]) * (p[:, c, 1] - p[:, a, 1]) - (p[:, b, 1] - p[:, a, 1]) * (p[:, c, 0] - p[:, a, 0])
        neg += det(s) * det(d) < 0
    return (neg == 0) | (neg == 4)


def solve_h(s, d):
    N = len(s)
    A = np.zeros((N, 8, 8))
    b = np.zeros((N, 8))
    for i in range(4):
        x, y, u, v = s[:, i, 0], s[:, i, 1], d[:, i, 0], d[:, i, 1]
        A[:, 2 * i, 0], A[:, 2 * i, 1], A[:, 2 * i, 2], A[:, 2 * i, 6], A[:, 2 * i, 7], b[:, 2 * i] = x, y, 1, -u * x, -u * y, u
        A[:, 2 * i + 1, 3], A[:, 2 * i + 1, 4], A[:, 2 * i + 1, 5] = x, y, 1
        A[:, 2 * i + 1, 6], A[:, 2 * i + 1, 7], b[:, 2 * i + 1] = -v * x, -v * y, v
    ok = np.abs(np.linalg.det(A)) > 1e-6
    h = np.zeros((N, 8))
    h[ok] = np.linalg.solve(A[ok], b[ok][..., None])[..., 0]
    return h[ok]


def counts(H, src, dst, order):
    """(exact, diamond, capped diamond) counts per hypothesis, the tiles cut from `order`."""
    x, y, u, v = src[order, 0], src[order, 1], dst[order, 0], dst[order, 1]
    n = len(x)
    tile = np.arange(n) // 32
    nt = tile[-1] + 1
    mn = lambda a: np.minimum.reduceat(a, np.arange(0, n, 32))
    mx = lambda a: np.maximum.reduceat(a, np.arange(0, n, 32))
    cx, cy = 0.5 * (mn(x) + mx(x)), 0.5 * (mn(y) + mx(y))
    rx, ry = mx(x) - cx, mx(y) - cy
    r = np.sqrt(25.5)
    ex_c, dia, cap = (np.zeros(len(H), int) for _ in range(3))
    for a in range(0, len(H), 1000):
        h = H[a:a + 1000]
        X = h[:, 0:1] * x + h[:, 1:2] * y + h[:, 2:3]
        Y = h[:, 3:4] * x + h[:, 4:5] * y + h[:, 5:6]
        W = h[:, 6:7] * x + h[:, 7:8] * y + 1
        s = np.abs(X - u * W) + np.abs(Y - v * W)
        Wc = np.abs(h[:, 6:7] * cx + h[:, 7:8] * cy + 1) + np.abs(h[:, 6:7]) * rx + np.abs(h[:, 7:8]) * ry
        assert Wc.shape[1] == nt
        ex_c[a:a + 1000] = ((X - u * W) ** 2 + (Y - v * W) ** 2 <= 25.0 * W * W).sum(1)
        dia[a:a + 1000] = (s <= np.sqrt(2) * r * np.abs(W)).sum(1)
        cap[a:a + 1000] = (s <= np.sqrt(2) * r * Wc[:, tile]).sum(1)
    return ex_c, dia, cap


def problem(src, dst, first, nh, rng):
    n = len(src)
    H = []
    while sum(len(h) for h in H) < first + nh:
        idx = np.array([rng.choice(n, 4, replace=False) for _ in range(8000)])
        k = check_subset(src[idx], dst[idx])
        H.append(solve_h(src[idx][k], dst[idx][k]))
    H = np.concatenate(H)[:first + nh]
    out = {}
    for name, order in (("match order", np.arange(n)), ("source-local", tile_order(src))):
        ex_c, dia, cap = counts(H, src, dst, order)
        bar = max(3, ex_c[:first].max())
        out[name] = (bar, cap[first:].mean(), (cap[first:] > bar).mean(), (dia[first:] > bar).mean(), dia.mean(),
                     [(b, (cap[first:] > b).mean()) for b in (3, 6, 10, 18, 24)])
    return out


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "c4"  # a config with planted matches: c2, c3, c4
    scenes = [int(a) for a in sys.argv[2:]] or [0, 1, 3, 5]
    cfg = CONFIGS[name]
    first = 4096 if cfg["max_iters"] > 4096 else 512
    nh = 20000 if cfg["max_iters"] > 4096 else cfg["max_iters"] - first
    rng = np.random.default_rng(1)
    print(f"# {name}: first chunk {first}, {nh} hypotheses after it; columns: n, bar, mean hi1, share hi1 > bar, "
          f"share diamond > bar, share hi1 > b for b = 3, 6, 10, 18, 24")
    for s in scenes:
        m = 0
        ds = make_config_dataset(name, scene_ids=[s])
        pos = ds.plant_pos[m][0]
        src = ds.model_kp[m][:len(pos)].astype(np.float64)
        dst = ds.scene_kp[0][pos].astype(np.float64)
        if len(src) < 128:
            continue
        for order, (bar, mean, share, dshare, dmean, at) in problem(src, dst, first, nh, rng).items():
            print(f"{name} model {m} scene {s} {order:13s} n {len(src):5d} bar {bar:3d} mean hi1 {mean:6.2f} "
                  f"hi1>bar {share:.4f} diamond>bar {dshare:.5f} | " + " ".join(f"{v:.4f}" for _, v in at))


if __name__ == "__main__":
    main()
