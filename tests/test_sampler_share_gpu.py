"""Sampler classes (ransac_class_kernel): the attempt tables are built once per class of windowed
problems with equal good-match count and nearby stream positions, in the leader's slices, and every
sampler reader goes through the class.  Sharing must change nothing: records and masks are compared
bit for bit with MIM_SAMPLER_SHARE=0 (every problem its own class), MIM_SHARE_SPREAD=0 (a class per
distinct stream position) and the attempt-by-attempt walker (MIM_SAMPLER_WALK=1).

Shapes: 8 (16) problems of 700 x 900 descriptors, 300 planted, maxIters 6,000: two chunks
([0, 4096) and [4096, 6000)), good-match counts ~300 >= kSmallMaxN, a second or so per arm."""
import os
import re

import numpy as np
import pytest

from computervision_objectdetection_featurematching_amd.synthetic import make_dataset

pytestmark = pytest.mark.gpu

SHAPE = (1, 8, 700, 900, 300)
SEED = 2024
MAX_ITERS = 6000
FIRST_CHUNK = 4096
_LINE = re.compile(r"\[mim\] sampler chunk \[(\d+),(\d+)\): windowed (\d+) classes (\d+)")

_data = {}
_runs = {}


def _dataset(frac):
    if frac not in _data:
        _data[frac] = make_dataset(*SHAPE, inlier_frac=frac, seed=SEED)
    return _data[frac]


def _run(fracs, ratio, env):
    """One batch (the scenes of the datasets `fracs` against their common model) in a fresh context
    with `env` set: (records, masks).  Cached per arm; the cached values are never modified."""
    key = (fracs, ratio, tuple(sorted(env.items())))
    if key in _runs:
        return _runs[key]
    from computervision_objectdetection_featurematching_amd import Matcher, default_params
    sets = [_dataset(f) for f in fracs]
    os.environ.update(env)
    try:
        m = Matcher(0)
        try:
            q = m.add_set(sets[0].model_desc[0], sets[0].model_kp[0])
            t = [m.add_set(d, k) for ds in sets for d, k in zip(ds.scene_desc, ds.scene_kp)]
            res = m.match_batch([(q, x) for x in t], default_params(max_iters=MAX_ITERS, ratio=ratio))
            masks = [m.problem_detail(i, int(r["n_good"]))[2].copy() for i, r in enumerate(res)]
        finally:
            m.close()
    finally:
        for k in env:
            os.environ.pop(k)
    _runs[key] = (res.copy(), masks)
    return _runs[key]


def _assert_same(a, b, what):
    (ra, ma), (rb, mb) = a, b
    assert ra.tobytes() == rb.tobytes(), what
    assert len(ma) == len(mb)
    for i, (x, y) in enumerate(zip(ma, mb)):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: mask of problem {i}")


def _chunks(err):
    """The MIM_DEBUG_NCLASS lines: [(c0, c1, windowed, classes)]."""
    return [tuple(int(x) for x in g) for g in _LINE.findall(err)]


def test_shared_and_single_classes_two_chunks(capfd):
    """Counts that partly coincide: chunk 1 (every stream position 0) has fewer classes than windowed
    problems, chunk 2's positions differ; all four arms give the same records and masks."""
    capfd.readouterr()
    dbg = _run((0.1,), 0.9, {"MIM_DEBUG_NCLASS": "1"})
    err = capfd.readouterr().err
    ng = [int(x) for x in dbg[0]["n_good"]]
    distinct = len(set(ng))
    assert distinct < len(ng), ng       # at least two problems share a count
    assert distinct >= 2, ng            # and at least two differ
    assert min(ng) >= 128, ng           # all windowed (not the small-problem kernel)
    assert all(int(x) == MAX_ITERS for x in dbg[0]["iters"]), dbg[0]["iters"]  # both chunks run in full
    ch = _chunks(err)
    assert len(ch) == 2 and ch[0][:2] == (0, FIRST_CHUNK) and ch[1][:2] == (FIRST_CHUNK, MAX_ITERS), err
    assert ch[0][2] == len(ng) and ch[0][3] == distinct and ch[0][3] < ch[0][2], ch
    assert ch[1][2] == len(ng) and distinct <= ch[1][3] <= len(ng), ch
    base = _run((0.1,), 0.9, {})
    _assert_same(dbg, base, "MIM_DEBUG_NCLASS changes nothing")
    for env in ({"MIM_SAMPLER_SHARE": "0"}, {"MIM_SHARE_SPREAD": "0"}, {"MIM_SAMPLER_WALK": "1"}):
        _assert_same(base, _run((0.1,), 0.9, env), f"default against {env}")


def test_share_off_and_spread_zero_classes(capfd):
    """The knobs do what they say: MIM_SAMPLER_SHARE=0 gives one class per windowed problem in every
    chunk, MIM_SHARE_SPREAD=0 shares only among equal stream positions (all of chunk 1's)."""
    capfd.readouterr()
    off = _run((0.1,), 0.9, {"MIM_SAMPLER_SHARE": "0", "MIM_DEBUG_NCLASS": "1"})
    ch_off = _chunks(capfd.readouterr().err)
    zero = _run((0.1,), 0.9, {"MIM_SHARE_SPREAD": "0", "MIM_DEBUG_NCLASS": "1"})
    ch_zero = _chunks(capfd.readouterr().err)
    distinct = len(set(int(x) for x in off[0]["n_good"]))
    assert [c[2] == c[3] for c in ch_off] == [True, True], ch_off
    assert len(ch_zero) == 2 and ch_zero[0][3] == distinct, ch_zero
    _assert_same(off, zero, "share off against spread 0")
    _assert_same(off, _run((0.1,), 0.9, {}), "share off against the default")


def test_one_class(capfd):
    """ratio 0.75 leaves the planted matches only: every problem has the same count, one class."""
    capfd.readouterr()
    dbg = _run((0.1,), 0.75, {"MIM_DEBUG_NCLASS": "1"})
    ch = _chunks(capfd.readouterr().err)
    ng = [int(x) for x in dbg[0]["n_good"]]
    assert len(set(ng)) == 1 and ng[0] >= 128, ng
    assert ch and ch[0][2] == len(ng) and ch[0][3] == 1, ch
    _assert_same(dbg, _run((0.1,), 0.75, {"MIM_SAMPLER_SHARE": "0"}), "one class against share off")
    _assert_same(dbg, _run((0.1,), 0.75, {"MIM_SAMPLER_WALK": "1"}), "one class against the walker")


def test_members_finish_at_different_times(capfd):
    """Scenes with 50 % inliers stop inside chunk 1, the same scenes with 8 % run on (same descriptors,
    so the same counts): chunk 2's classes have done and live members."""
    capfd.readouterr()
    dbg = _run((0.5, 0.08), 0.9, {"MIM_DEBUG_NCLASS": "1"})
    ch = _chunks(capfd.readouterr().err)
    res = dbg[0]
    ng = [int(x) for x in res["n_good"]]
    it = [int(x) for x in res["iters"]]
    early = {n for n, i in zip(ng, it) if i <= FIRST_CHUNK}
    late = {n for n, i in zip(ng, it) if i > FIRST_CHUNK}
    assert early and late and early & late, (ng, it)  # a count with a stopped and a live problem
    assert len(ch) == 2 and ch[0][2] == len(ng) and ch[0][3] < ch[0][2], ch
    assert ch[1][2] == sum(i > FIRST_CHUNK for i in it) < ch[0][2], (ch, it)
    _assert_same(dbg, _run((0.5, 0.08), 0.9, {"MIM_SAMPLER_SHARE": "0"}), "mixed batch against share off")


def test_overflow_path_with_sharing():
    """MIM_ATTEMPT_REP_CAP=1: the leader resolves nearly every redraw in place (list overflow)."""
    _assert_same(_run((0.1,), 0.9, {"MIM_ATTEMPT_REP_CAP": "1"}), _run((0.1,), 0.9, {"MIM_SAMPLER_WALK": "1"}),
                 "rep cap 1 against the walker")
