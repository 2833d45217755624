"""CPU checks of tests/flagged_inputs.py: from the yardstick alone, the cases of tests/test_knn_flagged_gpu.py
are not vacuous.  A set that should be flagged and is not would be answered from (int)v saturated to a byte
(flagged_inputs.as_i8_path): every flagging value but one changes a distance bit against that, at every
position used."""
import numpy as np
import pytest

import flagged_inputs as FI
import float_ref


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_batch_problems_accept(oracle):
    """At ratio 0.9 every full-size problem of the batch passes the ratio filter often enough for RANSAC to run, and
    is accepted; the small train sets cover the few-good gate."""
    S = FI.sets()
    prm = oracle.default_params(ratio=0.9, max_iters=FI.MAX_ITERS)
    out = [oracle.match_problem(*S[a], *S[b], prm) for a, b in FI.PROBLEMS]
    for i in FI.FULL_SIZE:
        assert out[i]["n_good"] > 50, (i, out[i]["n_good"])  # well over the 4 that RANSAC needs
    assert sum(o["status"] == FI.MIM_ACCEPTED for o in out) >= 3
    assert all(out[i]["status"] == FI.MIM_ACCEPTED for i in FI.FULL_SIZE)
    assert out[6]["n_good"] == 0  # one train row: no second neighbour
    # the jittered sets' squares need more than 24 bits: the distances differ from the integer rows'
    assert not np.array_equal(_bits(oracle.knn2(S["QI"][0], S["TI"][0])[1]), _bits(oracle.knn2(S["QR"][0], S["TR"][0])[1]))


def test_single_values_of_the_batch_move_distance_bits(oracle):
    """T1's row is a nearest row of some query, and Q1's query has its own distances: read as the integers the i8
    path would take them for (0 and 255), both would give other knnMatch rows."""
    S = FI.sets()
    base = oracle.knn2(S["QI"][0], S["TI"][0])
    t1 = oracle.knn2(S["QI"][0], S["T1"][0])
    q1 = oracle.knn2(S["Q1"][0], S["TI"][0])
    assert (t1[0] == FI.T1_POS[0]).any() and not np.array_equal(_bits(t1[1]), _bits(base[1]))
    assert not np.array_equal(_bits(q1[1][FI.Q1_POS[0]]), _bits(base[1][FI.Q1_POS[0]]))
    for (name, pos, v), other in zip((("T1", FI.T1_POS, FI.T1_VALUE), ("Q1", FI.Q1_POS, FI.Q1_VALUE)), ("QI", "TI")):
        wrong = S[name][0].copy()
        wrong[pos] = FI.as_i8_path(v)
        got = oracle.knn2(S[other][0], wrong) if name == "T1" else oracle.knn2(wrong, S[other][0])
        assert not np.array_equal(_bits(got[1]), _bits((t1 if name == "T1" else q1)[1])), name


def test_single_values_sit_where_stated():
    S = FI.sets()
    for name, base, pos, v in (("T1", "TI", FI.T1_POS, FI.T1_VALUE), ("Q1", "QI", FI.Q1_POS, FI.Q1_VALUE)):
        diff = np.argwhere(S[name][0] != S[base][0])
        assert diff.tolist() == [list(pos)] and S[name][0][pos] == v
    assert FI.T1_POS[0] // 64 == 23 and FI.T1_POS[0] % 64 == 27  # the last row of the 28-row tile
    for n in ("QR", "TR"):
        r = S[n][0]
        assert r.min() >= 0 and r.max() <= 255 and (r != np.rint(r)).any(axis=1).all()


@pytest.mark.parametrize("name", [n for n in FI.FLAGGING if n != "nan"])
def test_flagging_value_changes_a_distance_bit(oracle, name):
    v = FI.FLAGGING[name]
    assert not (v >= 0 and v <= 255 and v == np.rint(v))
    w = FI.as_i8_path(v)
    assert 0 <= w <= 255 and w == np.rint(w)
    for side, r, c in FI.boundary_cases():
        a = oracle.knn2(*FI.altered(side, r, c, v))
        b = oracle.knn2(*FI.altered(side, r, c, w))
        same = np.array_equal(_bits(a[1]), _bits(b[1]))
        if name in FI.UNOBSERVABLE:
            # (1e-40 - x)^2 == x^2 in float for every integer x: either kernel gives the same bits, stated, not hidden
            assert same and np.array_equal(a[0], b[0]), (name, side, r, c)
        else:
            assert not same, (name, side, r, c)


def test_nan_row_is_never_inserted(oracle):
    for side, r, c in FI.boundary_cases():
        idx, dist = oracle.knn2(*FI.altered(side, r, c, FI.FLAGGING["nan"]))
        if side == "q":
            assert (idx[r] == -1).all() and (dist[r] == FI.FLT_MAX).all()
            assert (np.delete(idx, r, axis=0) >= 0).all()
        else:
            assert not (idx == r).any() and (idx >= 0).all()


@pytest.mark.parametrize("name", list(FI.NOT_FLAGGING))
def test_not_flagging_values_are_integers_in_range(name):
    v = FI.NOT_FLAGGING[name]
    assert v >= 0 and v <= 255 and v == np.rint(v) and int(v) == FI.as_i8_path(v)


@pytest.mark.parametrize("name", list(FI.VALUES))
def test_float_ref_agrees_with_oracle(oracle, name):
    for side, r, c in FI.boundary_cases():
        q, t = FI.altered(side, r, c, FI.VALUES[name])
        a, b = oracle.knn2(q, t), float_ref.knn2(q, t)
        np.testing.assert_array_equal(a[0], b[0], err_msg=f"{name} {side} {r} {c}")
        np.testing.assert_array_equal(_bits(a[1]), _bits(b[1]), err_msg=f"{name} {side} {r} {c}")


def test_boundary_positions_cover_the_prep_lanes():
    """Of prep_tile's index arithmetic: row = 64 tile + 32 k + (lane & 31), col = 32 wave + 16 (lane >> 5) + j."""
    for pos, n in ((FI.T_POSITIONS, FI.B_NT), (FI.Q_POSITIONS, FI.B_NQ)):
        rows, cols = [r for r, _ in pos], [c for _, c in pos]
        assert {r // 64 for r in rows} == set(range((n + 63) // 64))  # every tile
        assert {(r % 64) // 32 for r in rows} == {0, 1}  # both k passes
        assert {(c % 32) // 16 for c in cols} == {0, 1}  # both lane halves
        assert len({c // 32 for c in cols}) >= 3 and max(rows) == n - 1  # three waves, the last row
    q, t = FI.boundary_base()
    assert (q == np.rint(q)).all() and (t == np.rint(t)).all() and min(q.min(), t.min()) >= 0 and max(q.max(), t.max()) <= 255


def test_mixed_sets_have_mutual_neighbours():
    import cross_ref as X
    M = FI.mixed_sets()
    for a, b in FI.MIXED_PAIRS:
        idx, _ = X.mutual(X.distances("f32", M[a], M[b]))
        assert (idx >= 0).sum() >= 100
    assert (M["QR"] != np.rint(M["QR"])).any(axis=1).all() and (M["TI"] == np.rint(M["TI"])).all()
