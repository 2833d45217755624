"""The distance schedule (csrc/knn_schedule.h) on the CPU: tests/cpp/knn_schedule_driver.cpp prints its tables.

Two independent checks per case, each under a plain and an ASan + UBSan build of the driver:
* the printed tables hash to the digest in tests/golden/knn_schedule.json, recorded
  (tests/golden/make_knn_schedule_golden.py) from the verbatim move of the schedule out of api.cpp's
  build_tables, before it was restructured: the tables stay the parent's byte for byte;
* invariants computed here from the printed tables alone (offsets, coverage of every query block's train
  tiles, block load, list order, Hamming row ranges), which would also catch an error the parent shared.
"""
import hashlib
import json
import os
import subprocess
from collections import defaultdict

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "knn_schedule.json")
BLOCK_Q, TILE_ROWS, HAM_BLOCK_Q, HAM_TILE_ROWS, MIN_CHUNK, SUB_DEFAULT = 512, 64, 256, 128, 8, -1


def _p(nq, nt, binary=False):
    return (nq, nt, (nt + TILE_ROWS - 1) // TILE_ROWS, int(binary))


def _case(probs, G=512, n_cu=256, max_iters=2000, sub=None, dyn=-1, tail=0):
    return dict(G=G, n_cu=n_cu, max_iters=max_iters, sub=sub, dyn=dyn, tail=tail, probs=list(probs))


def _cases():
    c = {}
    big = _p(10000, 10000)
    c["c3"] = _case([big] * 96, max_iters=50000)
    c["c4"] = _case([big] * 256, max_iters=50000)
    for tail in (0, 1):
        c[f"c4_shard32_tail{tail}"] = _case([big] * 32, max_iters=50000, tail=tail)
        c[f"split_tail40_tail{tail}"] = _case([_p(8000, 2500)] * 40, max_iters=500, tail=tail)
    # the tail search steps over binary problems at the end of the batch
    c["split_tail40_tail1_bin"] = _case([_p(8000, 2500)] * 40 + [_p(500, 3000, True), _p(300, 700, True)],
                                        max_iters=500, tail=1)
    c["c5"] = _case([_p(50000, 50000)])
    for sub in (-1, 0, 16, 64):
        c[f"schedules_sub{sub}_dyn0"] = _case([_p(12000, 30000)], sub=sub, dyn=0)
    c["schedules_dyn1"] = _case([_p(12000, 30000)], dyn=1)
    rng = np.random.default_rng(20240611)
    c["c1_ragged145"] = _case([_p(int(q), int(t)) for q, t in
                               zip(rng.integers(100, 501, 145), rng.integers(1000, 4001, 145))])
    for G in (8, 16, 304, 512):
        for name, pr in (("1x1", _p(1, 1)), ("0x5", _p(0, 5)), ("5x0", _p(5, 0))):
            c[f"degenerate_{name}_G{G}"] = _case([pr], G=G, n_cu=max(1, G // 2))
    c["mixed_kinds"] = _case([_p(3000, 4000), _p(700, 12000), _p(64, 70000, True), _p(5000, 900), _p(1200, 2500, True),
                              _p(10000, 10000), _p(300, 300, True), _p(513, 65), _p(257, 129, True), _p(2048, 6400)])
    c["binary_only"] = _case([_p(64, 70000, True), _p(2000, 2000, True), _p(256, 512, True), _p(1, 1, True),
                              _p(0, 300, True), _p(300, 0, True)])
    return c


CASES = _cases()


def case_text(name):
    c = CASES[name]
    head = [name, c["G"], c["n_cu"], c["max_iters"], "default" if c["sub"] is None else c["sub"], c["dyn"], c["tail"],
            len(c["probs"])]
    return "\n".join([" ".join(map(str, head))] + [" ".join(map(str, p)) for p in c["probs"]]) + "\n"


def build_driver(exe, sanitize=False):
    """tests/cpp/knn_schedule_driver.cpp over csrc/knn_schedule.h alone; sanitize: ASan + UBSan, any finding
    aborts the driver, so every test below fails on it."""
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call(["g++", "-std=c++17", *(san if sanitize else ["-O2"]), "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "knn_schedule_driver.cpp"), "-o", exe])
    return exe


def run_driver(exe, name):
    return subprocess.run([exe], input=case_text(name), capture_output=True, text=True, check=True).stdout


def parse(text):
    t = dict(slots=[], works=[], ham=[])
    for line in text.splitlines():
        w = line.split()
        if w[0] == "block_q":
            assert [int(w[1]), int(w[3]), int(w[5])] == [BLOCK_Q, HAM_BLOCK_Q, HAM_TILE_ROWS]
        elif w[0] == "n_blocks":
            t.update(n_blocks=int(w[1]), dyn=int(w[3]), part=int(w[5]), good=int(w[7]))
        elif w[0] == "slot":
            t["slots"].append(dict(zip(("nsplit", "q_pad", "part_off", "good_off", "it_off"), map(int, w[2:]))))
        elif w[0] == "work":
            t["works"].append(tuple(int(v) for v in w[1:]))  # problem, q0, tile0, tile1, split
        elif w[0] == "seg":
            t["seg"] = [int(v) for v in w[1:]]
        elif w[0] == "ham":
            t["ham"].append(tuple(int(v) for v in w[1:]))  # problem, q0, r0, r1, split
    return t


def summary(text):
    t = parse(text)
    return dict(digest=hashlib.sha256(text.encode()).hexdigest(), n_blocks=t["n_blocks"], n_works=len(t["works"]),
                part=t["part"], dyn=t["dyn"])


@pytest.fixture(scope="module", params=["plain", "asan+ubsan"])
def driver(tmp_path_factory, request):
    exe = str(tmp_path_factory.mktemp("knn_schedule") / "knn_schedule_driver")
    return build_driver(exe, sanitize=request.param != "plain")


_runs = {}


@pytest.fixture
def tables(driver, request):
    """(text, parsed tables) of the case, run once per driver build"""
    name = request.param
    if (driver, name) not in _runs:
        text = run_driver(driver, name)
        _runs[driver, name] = (text, parse(text))
    return name, _runs[driver, name]


with open(GOLDEN) as _f:
    _golden = json.load(_f)


def test_golden_lists_the_cases():
    assert sorted(_golden) == sorted(CASES)


@pytest.mark.parametrize("tables", sorted(CASES), indirect=True)
def test_tables_match_moved_code(tables):
    name, (text, _) = tables
    assert summary(text) == _golden[name]


def _ceil(a, b):
    return -(-a // b)


def _check_offsets(c, t):
    part = good = it = 0
    assert len(t["slots"]) == len(c["probs"])
    for (nq, _, _, binary), s in zip(c["probs"], t["slots"]):
        bq = HAM_BLOCK_Q if binary else BLOCK_Q
        assert s["q_pad"] % bq == 0 and s["q_pad"] >= nq and s["nsplit"] >= 1
        assert s["part_off"] == part
        part += s["nsplit"] * s["q_pad"]
        assert s["good_off"] % 32 == 0 and s["good_off"] >= good  # disjoint: starts at or past the previous slot's end
        good = s["good_off"] + max(nq, 1)
        assert s["it_off"] == it
        it += max(c["max_iters"], 1)
    assert t["part"] == part
    assert t["good"] >= good and t["good"] % 32 == 0


def _check_seg(t):
    seg = t["seg"]
    assert seg[0] == 0 and seg[-1] == len(t["works"]) and all(a <= b for a, b in zip(seg, seg[1:]))
    assert len(seg) == (9 if t["dyn"] else t["n_blocks"] + 1)


def _check_coverage(c, t):
    """every float problem's query block: the splits 0 .. nsplit-1 once each, the non-empty ones covering
    [0, n_tiles) in split order, the empty ones (n_tiles, n_tiles)"""
    items = defaultdict(list)
    for p, q0, t0, t1, sp in t["works"]:
        assert not c["probs"][p][3] and q0 % BLOCK_Q == 0
        items[p, q0 // BLOCK_Q].append((sp, t0, t1))
    want = set()
    for p, (nq, _, nt, binary) in enumerate(c["probs"]):
        if binary:
            continue
        for b in range(_ceil(nq, BLOCK_Q)):
            want.add((p, b))
            its = sorted(items[p, b])
            assert [sp for sp, _, _ in its] == list(range(t["slots"][p]["nsplit"]))
            at = 0
            for _, t0, t1 in its:
                if t0 == t1:
                    assert t0 == nt
                else:
                    assert t0 == at and t1 > t0
                    at = t1
            assert at == nt
    assert set(k for k, v in items.items() if v) == want


def _check_static(c, t):
    units = sum(_ceil(nq, BLOCK_Q) * nt for nq, _, nt, binary in c["probs"] if not binary)
    st = SUB_DEFAULT if c["sub"] is None else c["sub"]
    chunk = max(MIN_CHUNK, _ceil(units, c["G"]))
    R = _ceil(chunk, st) if st > 0 and chunk > st else 1
    sub = max(MIN_CHUNK, _ceil(chunk, R))
    seg = t["seg"]
    for b in range(t["n_blocks"]):
        assert sum(t1 - t0 for _, _, t0, t1, _ in t["works"][seg[b]:seg[b + 1]]) <= R * sub
    assert t["n_blocks"] <= max(c["G"], 8)


def _check_dynamic(c, t):
    G, probs, n = c["G"], c["probs"], len(c["probs"])
    assert t["n_blocks"] % 8 == 0 and 8 <= t["n_blocks"] <= G
    sweeps = [0 if binary else _ceil(nq, BLOCK_Q) for nq, _, _, binary in probs]
    # the tail: the trailing problems whose sweeps cover the remainder of the last round, in k ~ G / their
    # sweeps (2 .. 8) tile ranges each
    tail_from, k = n, 1
    rem = sum(sweeps) % G
    if c["tail"] and sum(sweeps) > G and rem > 0:
        ts = 0
        while tail_from > 0 and ts < rem:
            tail_from -= 1
            ts += sweeps[tail_from]
        k = max(2, min(8, (G + ts // 2) // ts))
    by_prob = defaultdict(list)
    for p, q0, t0, t1, sp in t["works"]:
        by_prob[p].append((q0 // BLOCK_Q, sp, t0, t1))
    for p, (nq, _, nt, binary) in enumerate(probs):
        if binary:
            continue
        kp = 1 if p < tail_from else min(k, max(nt, 1))
        assert t["slots"][p]["nsplit"] == kp
        assert sorted(by_prob[p]) == [(b, j, j * nt // kp, (j + 1) * nt // kp) for b in range(sweeps[p]) for j in range(kp)]
    seg = t["seg"]
    for x in range(8):
        is_piece = [p >= tail_from for p, *_ in t["works"][seg[x]:seg[x + 1]]]
        assert is_piece == sorted(is_piece)  # whole sweeps, then pieces


def _check_hamming(c, t):
    items = defaultdict(list)
    for p, q0, r0, r1, sp in t["ham"]:
        assert c["probs"][p][3] and q0 % HAM_BLOCK_Q == 0 and r0 % HAM_TILE_ROWS == 0 and r0 <= r1
        items[p, q0 // HAM_BLOCK_Q].append((sp, r0, r1))
    want = set()
    for p, (nq, nt, _, binary) in enumerate(c["probs"]):
        if not binary:
            continue
        for b in range(_ceil(nq, HAM_BLOCK_Q)):
            want.add((p, b))
            its = sorted(items[p, b])
            assert [sp for sp, _, _ in its] == list(range(t["slots"][p]["nsplit"]))
            assert its[0][1] == 0 and its[-1][2] == nt
            assert all(a[2] == b_[1] for a, b_ in zip(its, its[1:]))
    assert set(items) == want


@pytest.mark.parametrize("tables", sorted(CASES), indirect=True)
def test_invariants(tables):
    name, (_, t) = tables
    c = CASES[name]
    n_sweeps = sum(_ceil(nq, BLOCK_Q) for nq, _, _, binary in c["probs"] if not binary)
    assert t["dyn"] == (c["dyn"] if c["dyn"] >= 0 else int(n_sweeps >= c["G"]))
    _check_offsets(c, t)
    _check_seg(t)
    _check_coverage(c, t)
    (_check_dynamic if t["dyn"] else _check_static)(c, t)
    _check_hamming(c, t)
