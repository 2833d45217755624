"""GPU parity of the distance kernel's verdict mode (csrc/knn.hip, knn2_i8_kernel<2>).

For whole sweeps of one split (MIM_KNN_DYN=1) a lane pair that surely fails the ratio test records a new
minimum without an insertion event and takes an event only for a row that could make it pass; the record
of a failing query then carries no valid nearest index, and the few queries the kernel cannot decide are
rescanned exactly.  The records and good-match lists must equal the ratio mode's (MIM_KNN_FLIP=0), the
exact kernel's (MIM_KNN_RATIO=0) and the oracle's knnMatch + ratio filter, for ratios on both sides of 1;
with the static schedule (MIM_KNN_DYN=0) the earlier kernels run and nothing changes.

Train row i sits in tile i // 64, 32-row block (i % 64) // 32, lane half ((i % 32) >> 2) & 1; the first
256 rows of a work item are early tiles, a stage is 256 rows, the last tile (rows 1472 ..) is padded.
Every planted query has two rows M, M' in the early tiles, close enough to each other that the pair
surely fails at 0.9, far from everything else; a row b with M > b >= 0.81 M then arrives late and is
recorded without an event, and what follows walks the pair through the state changes listed in `data`.
"""
import os

import numpy as np
import pytest

from computervision_objectdetection_featurematching_amd.synthetic import sift_like

pytestmark = pytest.mark.gpu

NQ, NT = 600, 1500
RATIOS = [0.5, 0.9, 0.999, 1.0, 1.2]


def _offset(d2: int) -> np.ndarray:
    """An integer vector of 128 entries, |.|^2 = d2, entries within +-100 (greedy sum of squares)."""
    v = np.zeros(128, np.float32)
    k = 0
    while d2 > 0:
        s = min(100, int(np.sqrt(d2)))
        v[k] = s if k % 2 == 0 else -s
        d2 -= s * s
        k += 1
    assert k <= 128
    return v


def _half(i: int) -> int:
    return ((i % 32) >> 2) & 1


class _Rows:
    """Hands out unused train positions by kind."""

    def __init__(self, rng):
        self.rng = rng
        self.used = set()

    def take(self, lo, hi, pred=lambda i: True):
        for _ in range(10000):
            i = int(self.rng.integers(lo, hi))
            if i not in self.used and pred(i):
                self.used.add(i)
                return i
        raise AssertionError("no free row")

    def block(self, n, halves, lo=512, hi=NT - 64):
        """n free rows of one 32-row block of the late rows, in ascending order, row k in lane half
        halves[k] relative to the first (0 same, 1 opposite)."""
        for _ in range(10000):
            a = self.take(lo, hi, lambda i: i % 32 < 8)
            out = [a]
            for k in range(1, n):
                cand = [i for i in range(out[-1] + 1, a - a % 32 + 32)
                        if i not in self.used and i not in out and (_half(i) != _half(a)) == bool(halves[k])]
                if not cand:
                    break
                out.append(cand[int(self.rng.integers(min(len(cand), 4)))])
            if len(out) == n:
                self.used.update(out)
                return out
            self.used.discard(a)
        raise AssertionError("no free block")


# position kinds: e early rows, s1 .. s5 the late stages (s5 ends before the padded tile), last the padded tile,
# ("blk", halves) the rows of one 32-row block in arrival order
_SPAN = {"e": (0, 256), "s1": (256, 512), "s2": (512, 768), "s3": (768, 1024), "s4": (1024, 1280),
         "s5": (1280, 1472), "last": (1472, NT)}


def _cases():
    cases = []  # (d^2 of the rows after M, M', their positions, M)
    M = 12000
    # a close row arriving late after a farther minimum that was recorded without an event
    cases += [(M, [10000, 5000], ["s1", "s3"]), (M, [10000, 5000], ["s2", "s2"])]
    # the same with both rows in one 32-row block, same half and opposite halves
    cases += [(M, [10000, 5000], [("blk", (0, h))]) for h in (0, 1)]
    # two rows under the old minimum in one block, only the closer one under the flip limit, either order
    for h in (0, 1):
        cases += [(M, [11000, 5000], [("blk", (0, h))]), (M, [5000, 11000], [("blk", (0, h))]),
                  (M, [10000, 11000, 5000], ["s1", ("blk", (0, h))])]
    # a flip in one half and the old minimum in the other (rows picked by lane half)
    cases += [(M, [10000, 5000], ["s2/0", "s4/1"]), (M, [10000, 5000], ["s2/1", "s4/0"])]
    # a flip in the last, padded tile; a recorded row there
    cases += [(M, [10000, 5000], ["s2", "last"]), (M, [5000], ["last"]), (M, [10000], ["last"])]
    # the old minimum in the early tiles alone
    cases += [(M, [5000], ["s3"]), (M, [], [])]
    # candidate -> failing -> candidate again over three stages, with and without the recorded row first
    cases += [(M, [5000, 5500, 4000], ["s1", "s3", "s5"]), (M, [10000, 5000, 5500, 4000], ["s1", "s2", "s3", "s4"])]
    # d1 = d2: recorded twice, flipped twice
    cases += [(M, [10000, 10000], ["s1", "s3"]), (M, [5000, 5000], ["s1", "s3"]), (M, [5000, 5000], [("blk", (0, 1))]),
              (M, [10000, 5000, 5000], ["s1", "s2", ("blk", (0,))])]
    # a query equal to a train row
    cases += [(M, [0], ["s3"]), (M, [0, 0], ["s2", "s4"]), (M, [10000, 0], ["s1", "last"]), (7, [0], ["s2"])]
    # parity boundaries: 81 : 100 exactly and one off either side, the farther row first and recorded
    # without an event; each twice (the queries' c(q), and with it the rows' norm parity, differs)
    for a, b, m in [(81, 100, 115), (80, 100, 115), (82, 100, 115), (81, 99, 115), (81, 101, 115),
                    (8100, 10000, 11500), (8099, 10000, 11500), (8101, 10000, 11500), (8100, 9999, 11500),
                    (8100, 10001, 11500)]:
        for _ in range(2):
            cases += [(m, [b, a], ["s1", "s3"]), (m, [b, a], [("blk", (0, 0))]), (m, [b, a], [("blk", (0, 1))]),
                      (m, [b, a], ["s2", "last"])]
    return cases


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(20241020)
    t = sift_like(rng, NT)
    q = sift_like(rng, NQ)
    rows = _Rows(rng)
    cases = _cases()
    assert len(cases) < NQ // 2
    recorded = []  # (query, row) of the rows meant to be recorded without an event
    for j, (m, d2s, kinds) in enumerate(cases):
        base = rng.integers(100, 156, size=128).astype(np.float32)  # far from the SIFT-like rows and each other
        q[j] = base
        pos = []
        for k in kinds:
            if isinstance(k, tuple):
                pos += rows.block(len(k[1]), k[1])
            elif "/" in k:
                lo, hi = _SPAN[k[:2]]
                pos.append(rows.take(lo, hi, lambda i, h=int(k[3]): _half(i) == h))
            else:
                pos.append(rows.take(*_SPAN[k]))
        assert len(pos) == len(d2s)
        for d2, p in zip([m, m + m // 100 + 1] + d2s, [rows.take(0, 256), rows.take(0, 256)] + pos):
            t[p] = base + np.roll(_offset(d2), int(rng.integers(128)))
        if d2s and 0.81 * m < d2s[0] < m:
            recorded.append((j, pos[0]))
    # ordinary matches among the remaining queries: a noisy copy somewhere in the train set
    for j in range(len(cases), len(cases) + 150):
        p = rows.take(0, NT)
        t[p] = np.clip(q[j] + rng.integers(-3, 4, size=128), 0, 255)
    assert t.min() >= 0 and t.max() <= 255
    kq = rng.uniform(0, 640, size=(NQ, 2)).astype(np.float32)
    kt = rng.uniform(0, 640, size=(NT, 2)).astype(np.float32)
    # train sets of the batch: the whole set, and its first 1, 2 and 65 rows
    return q, kq, [(t[:n].copy(), kt[:n].copy()) for n in (NT, 1, 2, 65)], recorded


@pytest.fixture(scope="module")
def expected(oracle, data):
    """Per train set the oracle's knnMatch rows (computed once; the ratio filter runs per ratio)."""
    q, _, trains, _ = data
    return [oracle.knn2(q, t) for t, _ in trains]


@pytest.fixture(scope="module")
def own_matcher(data):
    from computervision_objectdetection_featurematching_amd import Matcher, build
    build.build()
    q, kq, trains, _ = data
    m = Matcher(0)
    qs = m.add_set(q, kq)
    ts = [m.add_set(t, k) for t, k in trains]
    yield m, [(qs, x) for x in ts]
    m.close()


def _run(m, problems, ratio, env):
    from computervision_objectdetection_featurematching_amd import default_params
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        res = m.match_batch(problems, default_params(ratio=ratio, max_iters=20))
        det = [m.problem_detail(i, int(r["n_good"])) for i, r in enumerate(res)]
        mode = int(m.kernel_ms("knn_mode"))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return res, det, mode


def _same(new, ref, what):
    assert new[0].tobytes() == ref[0].tobytes(), f"records differ ({what})"
    for i, (a, b) in enumerate(zip(new[1], ref[1])):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y, err_msg=f"problem {i} {what}")


@pytest.mark.parametrize("ratio", RATIOS)
def test_verdict_mode_equals_ratio_mode_exact_and_oracle(own_matcher, oracle, expected, ratio):
    m, problems = own_matcher
    new = _run(m, problems, ratio, {"MIM_KNN_DYN": "1"})
    assert new[2] == (2 if ratio < 1 else 0)  # the new kernel where the ratio mode would run, for every problem
    off = _run(m, problems, ratio, {"MIM_KNN_DYN": "1", "MIM_KNN_FLIP": "0"})
    assert off[2] == (1 if ratio < 1 else 0)
    exact = _run(m, problems, ratio, {"MIM_KNN_DYN": "1", "MIM_KNN_RATIO": "0"})
    assert exact[2] == 0
    _same(new, off, f"MIM_KNN_FLIP=0, ratio {ratio}")
    _same(new, exact, f"MIM_KNN_RATIO=0, ratio {ratio}")
    for i, a in enumerate(new[1]):
        oi, od = expected[i]
        gq, gt = oracle.ratio_filter(oi, od, ratio)
        np.testing.assert_array_equal(a[0], gq, err_msg=f"good_q problem {i} ratio {ratio}")
        np.testing.assert_array_equal(a[1], gt, err_msg=f"good_t problem {i} ratio {ratio}")
    # the static schedule cuts problems into train ranges: the earlier kernels run, nothing changes
    stat = _run(m, problems, ratio, {"MIM_KNN_DYN": "0"})
    assert stat[2] == (1 if ratio < 1 else 0)
    _same(stat, exact, f"MIM_KNN_DYN=0, ratio {ratio}")
    # the tail pieces are more than one split: not the new kernel either
    tail = _run(m, problems, ratio, {"MIM_KNN_DYN": "1", "MIM_KNN_TAIL": "1"})
    assert tail[2] in ((1, 2) if ratio < 1 else (0,))
    _same(tail, exact, f"MIM_KNN_TAIL=1, ratio {ratio}")


def test_two_problems_sharing_the_query_set_both_take_the_new_path(own_matcher, oracle, expected):
    m, problems = own_matcher
    two = [problems[0], problems[3]]
    new = _run(m, two, 0.9, {"MIM_KNN_DYN": "1"})
    assert new[2] == 2  # one launch serves the batch: every i8 problem of it ran in verdict mode
    ref = _run(m, two, 0.9, {"MIM_KNN_DYN": "1", "MIM_KNN_RATIO": "0"})
    _same(new, ref, "two problems")
    for a, i in zip(new[1], (0, 3)):
        gq, gt = oracle.ratio_filter(*expected[i], 0.9)
        np.testing.assert_array_equal(a[0], gq)
        np.testing.assert_array_equal(a[1], gt)
        assert len(gq) > 0


def test_planted_cases_decide_as_built(data, expected):
    """The fixture's boundary pairs really straddle the float test (at 0.9 the exact 81 : 100 pair fails,
    one below passes), the rows meant to be recorded without an event are the second neighbours of
    queries that pass, with both norm parities, and the lists are not trivially empty."""
    q, _, trains, recorded = data
    oi, od = expected[0]
    good = od[:, 0] < np.float32(0.9) * od[:, 1]
    assert 100 < good.sum() < NQ - 50
    assert not (np.float32(9.0) < np.float32(0.9) * np.float32(10.0))
    assert np.sqrt(np.float32(80)) < np.float32(0.9) * np.float32(10.0)
    assert not (np.sqrt(np.float32(8100)) < np.float32(0.9) * np.sqrt(np.float32(10000)))
    assert np.sqrt(np.float32(8099)) < np.float32(0.9) * np.sqrt(np.float32(10000))
    assert np.sqrt(np.float32(8100)) < np.float32(0.9) * np.sqrt(np.float32(10001))
    t = trains[0][0]
    second = [(j, p) for j, p in recorded if oi[j, 1] == p]
    assert len(second) > 40
    par = {int(((t[p].astype(np.int64) - 128) ** 2).sum() & 1) for _, p in second}
    assert par == {0, 1}
    assert 0 < sum(bool(good[j]) for j, _ in second) < len(second)
