"""The host-callable parts of the top-k entries on the CPU: tests/cpp/knn_topk_driver.cpp runs
knn_topk_offsets (csrc/knn_schedule.h) and topk_merge_query (csrc/knn_topk_merge.h, the function the merge
kernel runs per query), under a plain and an ASan + UBSan build (a stand-alone program, run as its own
process).

* offsets: a problem's partials follow the previous problem's nsplit * q_pad * k entries, its output rows the
  previous problems' k * nq entries; the pieces cover every (query, train row) once, and every piece's list
  block lies inside its problem's share;
* merge: the k smallest (distance, index) pairs over the splits' sorted lists, ascending, with sentinel
  tails, distances shared between splits and lists shorter than k; absent entries are -1 / FLT_MAX.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX_BITS, INT_MAX = 0x7F7FFFFF, 2**31 - 1
HAM_BLOCK_Q, HAM_TILE, FLT_BLOCK_Q, FLT_ROW_PAD = 256, 128, 256, 64

# (nq, nt, bin, fdim): binary, generic float and 128-D sets (given as fdim 128), empty sides included
PROBS = [(64, 70000, 1, 0), (64, 70000, 0, 64), (333, 700, 0, 128), (257, 129, 1, 0), (1, 1, 0, 7), (5, 3, 1, 0),
         (0, 300, 0, 64), (300, 0, 1, 0), (300, 0, 0, 200), (2000, 2000, 0, 128), (10000, 10000, 1, 0)]


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("knn_topk")
    src = os.path.join(ROOT, "tests", "cpp", "knn_topk_driver.cpp")
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


@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("n_cu", [256, 8])
def test_offsets_and_pieces(drivers, k, n_cu):
    text = f"offsets {k} {n_cu} {len(PROBS)}\n" + "\n".join(" ".join(map(str, p)) for p in PROBS) + "\n"
    lines = run(drivers, text)
    slots = [tuple(map(int, w[2:])) for w in lines if w[0] == "slot"]
    assert len(slots) == len(PROBS)
    part = out = 0
    for (nq, nt, binary, fdim), (nsplit, q_pad, part_off, out_off) in zip(PROBS, slots):
        assert (part_off, out_off) == (part, out)
        assert nsplit >= 1 and q_pad % 256 == 0 and q_pad >= max(nq, 1)
        part += nsplit * q_pad * k
        out += nq * k
    assert [int(v) for v in next(w for w in lines if w[0] == "total")[1:]] == [part, out]
    if n_cu == 256:  # one query block over 70,000 rows is cut along the train rows while CUs would idle
        assert slots[0][0] >= 2 and slots[1][0] >= 2
    cover = {}
    for w in lines:
        if w[0] not in ("ham", "flt"):
            continue
        p, q0, r0, r1, sp = map(int, w[1:])
        nq, nt, binary, fdim = PROBS[p]
        nsplit, q_pad = slots[p][:2]
        assert (w[0] == "ham") == bool(binary)
        assert 0 <= sp < nsplit and q0 % 256 == 0 and q0 < q_pad and q0 < nq
        assert r0 % (HAM_TILE if binary else FLT_ROW_PAD) == 0 and r0 <= r1 <= nt
        cover.setdefault((p, q0), []).append((sp, r0, r1))
    for p, (nq, nt, binary, fdim) in enumerate(PROBS):
        for q0 in range(0, nq, 256):
            pieces = sorted(cover[(p, q0)])
            assert [sp for sp, _, _ in pieces] == list(range(slots[p][0]))  # every split's lists are written
            end = 0
            for _, r0, r1 in pieces:
                assert r0 == end or r1 == r0
                end = max(end, r1)
            assert end == nt
    assert all(p < len(PROBS) and PROBS[p][0] > 0 for p, _ in cover)


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _merge_case(rng, k, nsplit, nq, q_pad, tied):
    """Random sorted lists; returns the driver's input and the expected rows."""
    text = [f"merge {k} {nsplit} {q_pad} {nq}"]
    per_q = [[] for _ in range(nq)]
    for sp in range(nsplit):
        for q in range(nq):
            m = int(rng.integers(0, k + 1))  # entries of this list, the rest sentinels
            d = rng.integers(0, 4 if tied else 1000, size=m).astype(np.float32) * np.float32(0.37)
            idx = sp * 1000 + rng.permutation(1000)[:m]  # rows of distinct splits are distinct
            ents = sorted(zip(map(_bits, d), map(int, idx)))
            per_q[q] += ents
            ents += [(FLT_MAX_BITS, INT_MAX)] * (k - m)
            text.append(" ".join(f"{b:x} {i}" for b, i in ents))
    exp = []
    for q in range(nq):
        best = sorted(per_q[q])[:k]
        best += [(FLT_MAX_BITS, -1)] * (k - len(best))
        exp.append([v for b, i in best for v in (i, b)])
    return "\n".join(text) + "\n", exp


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9, 16])
def test_merge_order(drivers, k):
    rng = np.random.default_rng(k)
    text, exp = "", []
    for nsplit, nq, q_pad, tied in ((1, 5, 256, True), (2, 7, 256, True), (9, 3, 512, False), (33, 4, 256, True)):
        t, e = _merge_case(rng, k, nsplit, nq, q_pad, tied)
        text += t
        exp += e
    rows = [w for w in run(drivers, text) if w[0] == "row"]
    got = [[int(w[j], 16) if (j - 2) % 2 else int(w[j]) for j in range(2, len(w))] for w in rows]
    assert got == exp
