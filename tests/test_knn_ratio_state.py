"""CPU restatement of the distance kernel's ratio mode (csrc/knn.hip, knn2_i8_kernel<true>).

The state machine, in numpy: a query's train rows are cut into splits, a split's rows into two lane
halves ((row % 32) >> 2) & 1; each half keeps the two smallest D = d^2 - c(q) as values and the index of
the smallest.  After the early rows a stage begins with a refresh (the halves exchange their pairs; the
pair's two smallest Q1 <= Q2 classify it: failing when d1^2 >= kappa d2^2 in float32) and sets the
threshold on R = (D - p) / 2 to floor((Q1 - 1) / 2) (failing) or floor((Q2 - 1) / 2); a row at or under the
threshold is inserted, and an insertion may only lower the threshold, to the candidate one from the
half's fresh pair and the partner's stale copy.  Rows are also inserted at random, as the kernel inserts
a row in every lane of a wave when one lane hits.  Splits are merged by key as ratio_compact_kernel
does.  Against brute force: the decision sqrtf(d1^2) < ratio * sqrtf(d2^2) of every query, and the index
of the nearest row where it passes.
"""
from fractions import Fraction

import numpy as np
import pytest

INT_MAX = np.int64(2**31 - 1)
EARLY = 256
STAGE = 256


def kappa_f32(ratio: float) -> np.float32:
    """The launcher's kappa (csrc/api.cpp knn_ratio_kappa); 0 = exact kernel."""
    r = np.float32(ratio)
    if not (r > 0 and r < 1):
        return np.float32(0)
    k = float(r) * float(r) * (1.0 + 2.0**-18) * (1.0 + 2.0**-20)
    kf = np.nextafter(np.float32(k), np.float32(2))
    return kf if kf < 1 else np.float32(0)


def dist2(q, t):
    """Exact integer |q - t|^2 of every pair (float64 products of small integers are exact)."""
    qf, tf = q.astype(np.float64), t.astype(np.float64)
    d = (qf * qf).sum(1)[:, None] + (tf * tf).sum(1)[None, :] - 2.0 * (qf @ tf.T)
    return np.rint(d).astype(np.int64)


def brute(q, t):
    d = dist2(q, t)
    order = np.argsort(d, axis=1, kind="stable")
    return d, order


def decide(d1, d2, ratio):
    return np.sqrt(np.float32(d1)) < np.float32(ratio) * np.sqrt(np.float32(d2))


def med_push(m1, i1, m2, v, idx, on):
    """sel_push_r of the lanes in `on`."""
    c1 = on & (v < m1)
    nm2 = np.maximum(np.minimum(m1, m2), np.minimum(np.maximum(m1, m2), v))
    m2[:] = np.where(on, nm2, m2)
    i1[:] = np.where(c1, idx, i1)
    m1[:] = np.where(on, np.minimum(m1, v), m1)


def sweep_split(q, t, row0, kappa, rng, extra_push=0.02):
    """One work item: the split's rows t (global index row0 ..) for every query; returns the merged
    (D1, i1, D2) of the two halves."""
    nq = len(q)
    q128 = q.astype(np.int64) - 128
    cq = (q128**2).sum(1) + 2 * q128.sum(1)
    n2 = ((t.astype(np.int64) - 128) ** 2).sum(1)
    par = n2 & 1
    D = dist2(q, t) - cq[:, None]
    R = (D - par[None, :]) >> 1
    assert (2 * R + par[None, :] == D).all()
    m1 = np.full((2, nq), INT_MAX); m2 = np.full((2, nq), INT_MAX); i1 = np.full((2, nq), INT_MAX)
    o1 = np.full((2, nq), INT_MAX); o2 = np.full((2, nq), INT_MAX)
    T = np.full((2, nq), INT_MAX >> 1)
    n = len(t)
    for b0 in range(0, n, 32):  # one 32-row block: the threshold is fixed inside it
        if b0 >= EARLY and (b0 - EARLY) % STAGE == 0:  # refresh
            for h in range(2):
                o1[h], o2[h] = m1[1 - h].copy(), m2[1 - h].copy()
            for h in range(2):
                q1 = np.minimum(m1[h], o1[h])
                q2 = np.minimum(np.maximum(m1[h], o1[h]), np.minimum(m2[h], o2[h]))
                fail = (q2 != INT_MAX) & ((q1 + cq).astype(np.float32) >= kappa * (q2 + cq).astype(np.float32))
                T[h] = (np.where(fail, q1, q2) - 1) >> 1
        Tb = T.copy()
        for j in range(b0, min(b0 + 32, n)):
            h = ((j % 32) >> 2) & 1
            on = np.ones(nq, bool) if b0 < EARLY else (R[:, j] <= Tb[h]) | (rng.random(nq) < extra_push)
            med_push(m1[h], i1[h], m2[h], D[:, j], row0 + j, on)
        if b0 >= EARLY:
            for h in range(2):
                q2 = np.minimum(np.maximum(m1[h], o1[h]), np.minimum(m2[h], o2[h]))
                T[h] = np.minimum(T[h], (q2 - 1) >> 1)
    l = m1[1] < m1[0]
    M1 = np.where(l, m1[1], m1[0]); I1 = np.where(l, i1[1], i1[0])
    M2 = np.minimum(np.maximum(m1[0], m1[1]), np.minimum(m2[0], m2[1]))
    return M1 + cq, I1, np.where(M2 == INT_MAX, -1, M2 + cq)


def ratio_mode(q, t, ratio, nsplit, rng):
    """Good flags and nearest indices of every query by the ratio-mode kernel and the split merge."""
    kappa = kappa_f32(ratio)
    assert kappa > 0
    nq = len(q)
    K1 = np.full(nq, np.inf, np.float32); K2 = np.full(nq, np.inf, np.float32)
    I1 = np.full(nq, INT_MAX); have2 = np.zeros(nq, bool)
    cuts = [len(t) * s // nsplit for s in range(nsplit + 1)]
    for s in range(nsplit):
        if cuts[s] == cuts[s + 1]:
            continue
        d1, i1, d2 = sweep_split(q, t[cuts[s]:cuts[s + 1]], cuts[s], kappa, rng)
        k1 = np.sqrt(d1.astype(np.float32))
        k2 = np.where(d2 < 0, np.float32(np.inf), np.sqrt(np.maximum(d2, 0).astype(np.float32)))
        # top2_merge by key of (k1, i1) and (k2, any index)
        for k, i in ((k1, i1), (k2, None)):
            l1 = k < K1
            l2 = k < K2
            K2 = np.where(l1, K1, np.where(l2, k, K2))
            if i is not None:
                I1 = np.where(l1, i, I1)
            K1 = np.where(l1, k, K1)
    have2 = np.isfinite(K2)
    good = have2 & (K1 < np.float32(ratio) * K2)
    return good, I1


def check(q, t, ratio, nsplit, seed=0):
    rng = np.random.default_rng(seed)
    d, order = brute(q, t)
    rows = np.arange(len(q))
    d1 = d[rows, order[:, 0]]
    want = np.zeros(len(q), bool)
    if t.shape[0] >= 2:
        want = decide(d1, d[rows, order[:, 1]], ratio)
    good, i1 = ratio_mode(q, t, ratio, nsplit, rng)
    np.testing.assert_array_equal(good, want)
    np.testing.assert_array_equal(i1[want], order[want, 0])
    return want


def offset(d2):
    v = np.zeros(128, np.int64)
    k = 0
    while d2 > 0:
        s = min(100, int(np.sqrt(d2)))
        v[k] = s if k % 2 == 0 else -s
        d2 -= s * s
        k += 1
    return v


@pytest.mark.parametrize("ratio", [0.5, 0.9, 0.999])
@pytest.mark.parametrize("nsplit", [1, 3])
def test_random_integer_sets(ratio, nsplit):
    rng = np.random.default_rng(int(ratio * 1000) + nsplit)
    t = rng.integers(0, 256, size=(1100, 128))
    q = rng.integers(0, 256, size=(96, 128))
    # nearby rows at every scale of d^2, so that both outcomes and both states occur
    for j in range(64):
        for p in rng.choice(1100, size=3, replace=False):
            t[p] = np.clip(q[j] + rng.integers(-1 - j % 7, 2 + j % 7, size=128), 0, 255)
    want = check(q, t, ratio, nsplit)
    assert 0 < want.sum() < len(q) or ratio == 0.999


@pytest.mark.parametrize("ratio", [0.5, 0.9, 0.999])
def test_duplicated_rows_and_equal_query(ratio):
    rng = np.random.default_rng(7)
    pool = rng.integers(0, 256, size=(20, 128))
    t = pool[rng.integers(0, 20, size=900)]  # every nearest pair is a tie
    q = np.concatenate([pool[:10], rng.integers(0, 256, size=(30, 128))])
    want = check(q, t, ratio, 2)
    assert not want[:10].any()
    t2 = rng.integers(0, 256, size=(900, 128))
    t2[700] = q[12]  # a query equal to one train row: d1 = 0 passes against any d2 > 0
    want = check(q, t2, ratio, 1)
    assert want[12]


@pytest.mark.parametrize("ratio", [0.5, 0.9, 0.999])
def test_boundary_pairs_in_every_arrival_order(ratio):
    """d1^2 : d2^2 at ratio^2 exactly (81 : 100 for 0.9) and one off either side, the two rows early or
    late, in one 32-row block (same lane half, opposite halves) or stages apart."""
    rng = np.random.default_rng(11)
    r2 = Fraction(float(np.float32(ratio))) ** 2
    pairs = []
    for d2 in (100, 10000):
        c = int(r2 * d2)
        pairs += [(c + e, d2 + f) for e in (-1, 0, 1, 2) for f in (-1, 0, 1) if c + e > 0]
    kinds = ["early_late", "late_early", "same_up", "same_down", "opp_up", "opp_down", "far_up", "far_down"]
    nt = 1600
    q = rng.integers(100, 156, size=(len(pairs) * len(kinds), 128))
    t = rng.integers(0, 60, size=(nt, 128))  # far background: every pair starts failing
    free = np.ones(nt, bool)
    half = ((np.arange(nt) % 32) >> 2) & 1

    def take(mask):
        i = int(np.flatnonzero(mask & free)[0])  # IndexError = the set is too small for the cases
        free[i] = False
        return i

    rows = np.arange(nt)
    k = 0
    for a, b in pairs:
        for kind in kinds:
            if kind in ("early_late", "late_early"):
                pa, pb = take(rows < 256), take(rows >= 256)
            elif kind.startswith("far"):
                pa, pb = take((rows >= 256) & (rows < 512)), take(rows >= 1024)
            else:  # one 32-row block of the late rows, same lane half or opposite halves
                pa = take((rows >= 512) & (rows < 1024) & (rows % 4 == 0))
                same = kind.startswith("same")
                pb = take((rows // 32 == pa // 32) & ((half == half[pa]) == same))
            if kind.endswith(("late_early", "down")):
                pa, pb = pb, pa
            t[pa] = q[k] + np.roll(offset(a), k)
            t[pb] = q[k] + np.roll(offset(b), k)
            k += 1
    assert t.min() >= 0 and t.max() <= 255
    want = check(q, t, ratio, 1, seed=1)
    check(q, t, ratio, 4, seed=2)
    assert 0 < want.sum() < len(q)


@pytest.mark.parametrize("ratio", [0.5, 0.9, 0.999])
def test_margin(ratio):
    """kappa = ratio^2 (1 + 2^-18): at d1^2 = ceil(kappa d2^2) the float32 test is false, over a dense
    sample of d2^2 in [1, 2^23]; and the kernel's float32 classification (float)d1 >= kappa_f * (float)d2
    implies d1 >= kappa d2 exactly."""
    r = Fraction(float(np.float32(ratio)))
    kappa = r * r * (1 + Fraction(1, 2**18))
    rng = np.random.default_rng(3)
    d2 = np.unique(np.concatenate([np.arange(1, 100001), rng.integers(1, 2**23 + 1, size=100000),
                                   2 ** np.arange(1, 24), 2 ** np.arange(1, 24) - 1])).astype(np.int64)
    num, den = kappa.numerator, kappa.denominator
    d1 = np.array([-((-int(x) * num) // den) for x in d2], np.int64)  # ceil(kappa d2), exact
    assert not decide(d1, d2, ratio).any()
    kf = kappa_f32(ratio)
    assert 0 < kf < 1
    for delta in (-2, -1, 0, 1, 2):
        e1 = np.maximum(d1 + delta, 0)
        fail = e1.astype(np.float32) >= kf * d2.astype(np.float32)
        exact = e1 >= d1  # d1 = ceil(kappa d2): e1 >= kappa d2 exactly when e1 >= d1
        assert not (fail & ~exact).any()
        assert not (fail & decide(e1, d2, ratio)).any()


def test_kappa_selects_exact_kernel():
    for ratio in (1.0, 1.2, 0.0, -0.5, float("nan"), 0.9999999):
        assert kappa_f32(ratio) == 0
    for ratio in (0.5, 0.9, 0.999):
        assert 0 < kappa_f32(ratio) < 1
