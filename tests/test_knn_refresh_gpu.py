"""GPU parity of the distance kernel with its refresh schedule and idle padded waves (csrc/knn.hip).

The late loop refreshes its limits on every stage for the first MIM_KNN_REFRESH_DENSE late stages of a sweep
and on every MIM_KNN_REFRESH_EVERY-th after that (default 8 and 4: the sparse part starts at row
256 + 8 x 256 = 2,304 of a work item); a wave whose 64 queries all lie past the query set takes no part in
the tiles, the refreshes or the epilogue, but stages its share and meets every barrier.

Shapes, the smallest at which these paths can go wrong:
  Nq 65    one real query beyond the first wave (waves 2-7 idle)
     300   waves 5-7 of the only block all padding
     513   one real query in a block of seven idle waves
     1100  a padded tail after two full blocks
  Nt 257   one late row
     2369, 5000   past the dense part and through at least two sparse periods; neither a multiple of 64
Families: random SIFT-like rows with noisy copies, train rows by falling distance to the queries (every row
a new minimum), passing matches planted in the first stage after a skipped refresh and in each length's
last stage, and heavy duplicates (ties in d^2).

Per case: knn_sets_dev (the exact mode) against oracle.knn2, indices and distance bits; then a batch of
two problems (this Nq and the next one of the list against the same train rows) through whole sweeps
(MIM_KNN_DYN=1, the verdict mode) and through the static schedule (several splits, the ratio mode; there a
block runs pieces of both problems one after another, idle waves and all) against oracle.match_problem.
"""
import os

import numpy as np
import pytest

from computervision_objectdetection_featurematching_amd.synthetic import sift_like

pytestmark = pytest.mark.gpu

NQS = [65, 300, 513, 1100]
NTS = [257, 2369, 5000]
FAMILIES = ["random", "falling", "planted", "duplicates"]
NQ, NT = max(NQS), max(NTS)
RATIO, MAX_ITERS = 0.9, 50
DENSE, EVERY = 8, 4
# the largest Nt leaves the dense part and skips through two sparse periods
assert NT >= 256 * (1 + DENSE + 2 * EVERY)
# queries that get a planted row: every fourth, and the lone real query of a block or wave
PLANTED_Q = sorted(set(range(0, NQ, 4)) | {64, 512, 1024, NQ - 1})


def _family(name):
    rng = np.random.default_rng(FAMILIES.index(name) + 77)
    if name == "random":
        q, t = sift_like(rng, NQ), sift_like(rng, NT)
        for j in PLANTED_Q:  # a noisy copy anywhere in the set, at several noise levels
            t[rng.integers(0, NT)] = np.clip(q[j] + rng.integers(-1 - j % 9, 2 + j % 9, size=128), 0, 255)
    elif name == "falling":
        c = rng.integers(60, 196, size=128)
        q = np.clip(c + rng.integers(-3, 4, size=(NQ, 128)), 0, 255).astype(np.float32)
        amp = np.linspace(120, 6, NT)
        t = np.clip(c + (rng.standard_normal((NT, 128)) * amp[:, None]).astype(np.int64), 0, 255)
        d0 = ((t - c) ** 2).sum(1)
        t = t[np.argsort(-d0, kind="stable")]
        for r in (256, 2368, NT - 1):  # each length's last row lies much closer than everything before it
            t[r] = c + ((t[r] - c) * 0.4).astype(np.int64)
        t = t.astype(np.float32)
    elif name == "planted":
        q, t = sift_like(rng, NQ), sift_like(rng, NT)
        skipped = 256 + 256 * (DENSE + 1)  # the first stage off the default schedule
        spots = [256, skipped, skipped + 37, skipped + 255, 2304, 2368, 4864, NT - 1, NT - 40]
        free = np.ones(NT, bool)

        def take(base):
            row = next(r for r in [*range(base, NT), *range(base - 1, -1, -1)] if free[r])
            free[row] = False
            return row

        for k, j in enumerate(PLANTED_Q):
            t[take(spots[k % len(spots)])] = np.clip(q[j] + rng.integers(-1 - k % 5, 2 + k % 5, size=128), 0, 255)
            if k % 2:  # a weaker match before it: the pair is a candidate when the close row arrives
                t[take([17, 700, skipped - 30][(k // 2) % 3])] = np.clip(q[j] + rng.integers(-12, 13, size=128), 0, 255)
    else:
        pool = sift_like(rng, 40)
        t = pool[rng.integers(0, 40, size=NT)]
        q = sift_like(rng, NQ)
        q[::3] = pool[rng.integers(0, 40, size=len(q[::3]))]  # d1 = d2 = 0
        q[1::3] = np.clip(q[1::3] * 0.5 + pool[rng.integers(0, 40, size=len(q[1::3]))] * 0.5, 0, 255).round()
    kq = rng.uniform(0, 640, size=(NQ, 2)).astype(np.float32)
    kt = rng.uniform(0, 640, size=(NT, 2)).astype(np.float32)
    assert q.min() >= 0 and q.max() <= 255 and t.min() >= 0 and t.max() <= 255
    return np.ascontiguousarray(q, np.float32), kq, np.ascontiguousarray(t, np.float32), kt


_DATA, _KNN, _MATCH = {}, {}, {}


def _data(fam):
    if fam not in _DATA:
        _DATA[fam] = _family(fam)
    return _DATA[fam]


def _oracle_knn(oracle, fam, nt):
    """knnMatch rows of all NQ queries against the first nt train rows (a shorter query set is a prefix)."""
    if (fam, nt) not in _KNN:
        q, _, t, _ = _data(fam)
        _KNN[fam, nt] = oracle.knn2(q, t[:nt], 8)
    return _KNN[fam, nt]


def _oracle_match(oracle, fam, nq, nt):
    if (fam, nq, nt) not in _MATCH:
        q, kq, t, kt = _data(fam)
        _MATCH[fam, nq, nt] = oracle.match_problem(q[:nq], kq[:nq], t[:nt], kt[:nt],
                                                   oracle.default_params(ratio=RATIO, max_iters=MAX_ITERS), 8)
    return _MATCH[fam, nq, nt]


def _batch(m, problems, env):
    from computervision_objectdetection_featurematching_amd import default_params
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        res = m.match_batch(problems, default_params(ratio=RATIO, max_iters=MAX_ITERS))
        det = [m.problem_detail(i, int(r["n_good"])) for i, r in enumerate(res)]
        mode = int(m.kernel_ms("knn_mode"))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return res, det, mode


def _compare(res, det, outs, what):
    for i, o in enumerate(outs):
        r = res[i]
        gq, gt, gm = det[i]
        assert int(r["n_good"]) == o["n_good"], (what, i)
        np.testing.assert_array_equal(gq, o["good_q"], err_msg=f"{what} good_q {i}")
        np.testing.assert_array_equal(gt, o["good_t"], err_msg=f"{what} good_t {i}")
        assert (int(r["status"]), int(r["n_inl"])) == (o["status"], o["n_inl"]), (what, i, r, o)
        if o["n_good"] > 4:
            assert int(r["iters"]) == o["iters"], (what, i)
            np.testing.assert_array_equal(gm, o["mask"], err_msg=f"{what} mask {i}")
        if o["status"] != 2 and o["n_good"] >= 4:
            np.testing.assert_array_equal(r["H"].reshape(3, 3), o["H"], err_msg=f"{what} H {i}")


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_exact_verdict_and_ratio_modes_equal_the_oracle(matcher, oracle, fam, nq, nt):
    import torch
    q, kq, t, kt = _data(fam)
    nq2 = NQS[(NQS.index(nq) + 1) % len(NQS)]
    m = matcher
    m.clear_sets()
    try:
        a = m.add_set(q[:nq], kq[:nq])
        a2 = m.add_set(q[:nq2], kq[:nq2])
        b = m.add_set(t[:nt], kt[:nt])
        # the exact mode: knnMatch rows, indices and distance bits
        dev = torch.device("cuda", 0)
        idx = torch.empty((nq, 2), dtype=torch.int32, device=dev)
        dist = torch.empty((nq, 2), dtype=torch.float32, device=dev)
        m.knn_sets_dev(a, b, idx, dist)
        m.synchronize()
        oi, od = _oracle_knn(oracle, fam, nt)
        np.testing.assert_array_equal(idx.cpu().numpy(), oi[:nq])
        np.testing.assert_array_equal(dist.cpu().numpy().view(np.int32), od[:nq].view(np.int32))
        # the batch path: two problems, whole sweeps (verdict mode) and the static schedule's pieces (ratio mode)
        outs = [_oracle_match(oracle, fam, nq, nt), _oracle_match(oracle, fam, nq2, nt)]
        res, det, mode = _batch(m, [(a, b), (a2, b)], {"MIM_KNN_DYN": "1"})
        assert mode == 2
        _compare(res, det, outs, "verdict mode")
        res, det, mode = _batch(m, [(a, b), (a2, b)], {"MIM_KNN_DYN": "0"})
        assert mode == 1
        _compare(res, det, outs, "ratio mode")
    finally:
        m.clear_sets()


def test_families_are_what_they_claim(oracle):
    """Both outcomes occur where they should, the falling family's nearest rows are its last ones, the
    planted rows are the nearest neighbours of their queries, and the duplicates tie."""
    for fam in FAMILIES:
        oi, od = _oracle_knn(oracle, fam, NT)
        good = od[:, 0] < np.float32(RATIO) * od[:, 1]
        if fam == "random":
            assert 100 < good.sum() < NQ - 100
        elif fam == "falling":
            assert (oi[:, 0] > NT - 256).mean() > 0.8 and good.mean() > 0.5
        elif fam == "planted":
            assert good[PLANTED_Q].mean() > 0.8
            rows = oi[PLANTED_Q, 0]
            skipped = 256 + 256 * (DENSE + 1)
            assert ((rows >= skipped) & (rows < skipped + 256)).sum() > 50 and (rows >= 4864).sum() > 50
            assert 256 in rows and 2368 in rows
        else:
            assert (od[::3, 0] == 0).all() and (od[::3, 1] == 0).all() and not good[::3].any()
