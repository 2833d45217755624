"""The host-callable parts of the collection entry on the CPU: tests/cpp/knn_coll_driver.cpp runs
knn_coll_offsets / knn_coll_groups (csrc/knn_schedule.h) and coll_merge_query (csrc/knn_coll_merge.h, the
function the merge kernel runs per query row), under a plain and an ASan + UBSan build (a stand-alone program,
run as its own process).

* merge: the k smallest (distance, image, row) keys over the images' live lists, ascending: ties between images
  and between the lists of one image, lists shorter than k, a seed left by an earlier group, the flags words
  selecting the i8 or the float lists, and the key's last bits (image 8190, row 2^18 - 1);
* offsets: a pair's float lists follow the previous pair's lists, its i8 lists its own float lists; the output
  rows follow the query sets; every i8 work item lies inside its pair's share; the bound covers every pair;
* groups: consecutive, in order, within the budget unless a single image exceeds it.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX_BITS, INT_MAX = 0x7F7FFFFF, 2**31 - 1


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("knn_coll")
    src = os.path.join(ROOT, "tests", "cpp", "knn_coll_driver.cpp")
    plain, san = str(d / "driver"), str(d / "driver_san")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", src, "-o", plain])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", src, "-o", san])
    return plain, san


def run(drivers, text):
    """Both builds' output, which must agree (a sanitizer finding aborts the second)."""
    outs = [subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout for exe in drivers]
    assert outs[0] == outs[1] and outs[0].endswith("end\n")
    return [line.split() for line in outs[0].splitlines()]


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _fmt(ents, k):
    ents = sorted(ents) + [(FLT_MAX_BITS, INT_MAX)] * (k - len(ents))
    return " ".join(f"{b:x} {i}" for b, i in ents)


def _merge(drivers, k, parts, seed=None):
    """parts: [(img, qflag, tflag, [i8 lists], [float lists])], a list = [(bits, row)] of at most k entries;
    seed: [(row, img, bits)] ascending, at most k.  Returns the driver's (row, img, bits) triples and the expected
    ones from a plain sort of the live lists' (bits, img, row)."""
    text = [f"merge {k} {int(seed is not None)} {len(parts)}"]
    live = []
    if seed is not None:
        full = list(seed) + [(-1, -1, FLT_MAX_BITS)] * (k - len(seed))
        text.append(" ".join(f"{r} {im} {b:x}" for r, im, b in full))
        live += [(b, im, r) for r, im, b in seed]
    for img, qf, tf, a, b in parts:
        text.append(f"{img} {qf} {tf} {len(a)} {len(b)}")
        text += [_fmt(l, k) for l in a] + [_fmt(l, k) for l in b]
        for l in (a if a and not (qf | tf) else b):
            live += [(bits, img, row) for bits, row in l]
    exp = [(r, im, b) for b, im, r in sorted(live)[:k]]
    exp += [(-1, -1, FLT_MAX_BITS)] * (k - len(exp))
    w = next(w for w in run(drivers, "\n".join(text) + "\n") if w[0] == "row")
    got = [(int(w[1 + 3 * s]), int(w[2 + 3 * s]), int(w[3 + 3 * s], 16)) for s in range(k)]
    return got, exp


def _rand_list(rng, k, levels, rows):
    m = int(rng.integers(0, k + 1))
    d = rng.integers(0, levels, size=m).astype(np.float32) * np.float32(0.37)
    return sorted(zip(map(_bits, d), map(int, rng.choice(rows, size=m, replace=False))))


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9, 16])
def test_merge_order_with_ties_and_short_lists(drivers, k):
    rng = np.random.default_rng(100 + k)
    for trial in range(12):
        parts = []
        for img in sorted(rng.choice(40, size=int(rng.integers(1, 6)), replace=False)):
            qf, tf = (int(v) for v in rng.integers(0, 2, size=2) * rng.integers(0, 2, size=2))
            sift = bool(rng.integers(0, 2))
            na = 2 * int(rng.integers(1, 4)) if sift else 0
            # rows of the lists of one image are distinct: list l holds rows = l (mod its list count)
            a = [_rand_list(rng, k, 3, np.arange(l, 600, max(na, 1))) for l in range(na)]
            nb = int(rng.integers(1, 4))
            b = [_rand_list(rng, k, 3, np.arange(l, 600, nb)) for l in range(nb)]
            parts.append((int(img), qf if sift else 0, tf if sift else 0, a, b))
        got, exp = _merge(drivers, k, parts)
        assert got == exp, (trial, parts)


@pytest.mark.parametrize("k", [1, 3, 8, 16])
def test_seed_from_an_earlier_group(drivers, k):
    rng = np.random.default_rng(200 + k)
    for trial in range(8):
        m = int(rng.integers(0, k + 1))
        d = np.sort(rng.integers(0, 3, size=m)).astype(np.float32) * np.float32(0.37)
        seed = sorted((_bits(v), int(im), int(r)) for v, im, r in zip(d, rng.integers(0, 3, size=m), rng.permutation(500)[:m]))
        seed = [(r, im, b) for b, im, r in seed]
        parts = [(3 + j, 0, 0, [], [_rand_list(rng, k, 3, np.arange(500))]) for j in range(2)]
        got, exp = _merge(drivers, k, parts, seed)
        assert got == exp, (trial, seed, parts)
    got, exp = _merge(drivers, k, [(5, 0, 0, [], [[]])], seed=[])  # nothing before, nothing now
    assert got == exp == [(-1, -1, FLT_MAX_BITS)] * k


def test_flags_select_the_lists(drivers):
    a = [[(_bits(1.0), 4)], [(_bits(1.0), 9)]]
    b = [[(_bits(2.0), 7)]]
    for qf, tf, want in ((0, 0, [(4, 6, _bits(1.0)), (9, 6, _bits(1.0))]), (1, 0, [(7, 6, _bits(2.0))]),
                         (0, 1, [(7, 6, _bits(2.0))]), (1, 1, [(7, 6, _bits(2.0))])):
        got, exp = _merge(drivers, 2, [(6, qf, tf, a, b)])
        assert got == exp and got[:len(want)] == want


def test_the_keys_last_bits(drivers):
    """Image 8190 and row 2^18 - 1 come back whole, and order behind image 8189 / row 2^18 - 2 at one distance."""
    top = 2**18 - 1
    one = FLT_MAX_BITS - 1  # the largest float below FLT_MAX
    parts = [(8189, 0, 0, [], [[(one, top)]]), (8190, 0, 0, [[(one, top - 1)], [(one, top)]], [[(0, 0)]])]
    got, exp = _merge(drivers, 4, parts)
    assert got == exp == [(top, 8189, one), (top - 1, 8190, one), (top, 8190, one), (-1, -1, FLT_MAX_BITS)]


KINDS = {"bin": 0, "f32": 1, "sift": 2}
NQ, NT = [2500, 0, 300, 513], [300, 0, 1, 5000, 64, 129]


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_offsets(drivers, kind, k):
    kt = 4 if k <= 4 else 8 if k <= 8 else 16
    text = f"offsets {k} 256 512 {KINDS[kind]} {len(NQ)} {len(NT)}\n{' '.join(map(str, NQ))}\n{' '.join(map(str, NT))}\n"
    lines = run(drivers, text)
    pairs = [tuple(map(int, w[2:])) for w in lines if w[0] == "pair"]
    assert len(pairs) == len(NQ) * len(NT)
    part = 0
    for i, (nsplit, q_pad, part_off, nsplit8, q_pad8, part8_off, bound) in enumerate(pairs):
        nq = NQ[i // len(NT)]
        assert part_off == part and nsplit >= 1 and q_pad >= nq
        part += nsplit * q_pad * k
        if kind == "sift":
            assert part8_off == part and nsplit8 >= 1 and q_pad8 >= nq and q_pad8 % 512 == 0
            part += 2 * nsplit8 * q_pad8 * kt
        else:
            assert part8_off == -1
        assert part - part_off <= bound
    outs = [int(w[2]) for w in lines if w[0] == "out"]
    assert outs == [k * sum(NQ[:i]) for i in range(len(NQ))]
    assert [int(v) for v in next(w for w in lines if w[0] == "total")[1:]] == [part, k * sum(NQ)]
    works = [tuple(map(int, w[1:])) for w in lines if w[0] == "i8"]
    assert bool(works) == (kind == "sift")
    for p, q0, t0, t1, split in works:
        assert 0 <= split < pairs[p][3] and q0 % 512 == 0 and q0 < pairs[p][4] and t0 <= t1 <= (NT[p % len(NT)] + 63) // 64
    if kind == "sift":  # one query block against 5,000 rows is cut along the train tiles
        assert pairs[2 * len(NT) + 3][3] > 1


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_groups(drivers, kind):
    k, nq, nt = 5, [700, 40], [300, 0, 64, 5000, 1, 129, 300, 300]
    head = f"{KINDS[kind]} {{}} {len(nq)} {len(nt)}\n{' '.join(map(str, nq))}\n{' '.join(map(str, nt))}\n"
    lines = run(drivers, f"offsets {k} 256 512 " + head.format(""))
    bound = [int(w[8]) for w in lines if w[0] == "pair"]
    per_image = [8 * sum(bound[qi * len(nt) + j] for qi in range(len(nq))) for j in range(len(nt))]

    def groups(budget):
        return [int(w[1]) for w in run(drivers, f"groups {k} " + head.format(budget)) if w[0] == "group"]

    assert groups(1) == list(range(len(nt) + 1))  # one image per group
    assert groups(10**12) == [0, len(nt)]
    mid = per_image[0] + per_image[1] + per_image[2]
    g = groups(mid)
    assert g[0] == 0 and g[-1] == len(nt) and g == sorted(set(g)) and g[1] == 3
    for a, b in zip(g[:-1], g[1:]):
        assert sum(per_image[a:b]) <= mid or b - a == 1
