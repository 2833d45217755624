"""The generic-float work list of the distance schedule (csrc/knn_schedule.h knn_float_plan) on the CPU:
tests/cpp/knn_float_plan_driver.cpp prints the schedule's tables, under a plain and an ASan + UBSan build
(a stand-alone program, run as its own process).

* every (query, train row) of every generic-float problem is covered exactly once; a query block's split
  ranges are disjoint, ordered and start at multiples of the row unit; q_pad / nsplit agree with part_off;
* adding generic-float problems to a batch leaves the i8 works / seg and the Hamming list of the other
  problems unchanged (problem indices aside).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_BLOCK_Q, FLT_ROW_PAD, FLT_MAX_DIM = 256, 64, 512

# (nq, nt, bin, fdim)
I8 = [(3000, 4000, 0, 0), (700, 12000, 0, 0), (5000, 900, 0, 0), (513, 65, 0, 0)]
BIN = [(64, 70000, 1, 0), (1200, 2500, 1, 0), (257, 129, 1, 0)]
FLT = [(64, 70000, 0, 64), (300, 5000, 0, 128), (10000, 10000, 0, 256), (1, 1, 0, 1), (257, 63, 0, 512), (256, 64, 0, 17),
       (0, 300, 0, 64), (300, 0, 0, 64), (2000, 2000, 0, 128)]


def _interleave(*lists):
    out = []
    for i in range(max(len(x) for x in lists)):
        out += [x[i] for x in lists if i < len(x)]
    return out


CASES = {
    "mixed": dict(G=512, n_cu=256, probs=_interleave(FLT, I8, BIN)),
    "mixed_small_gpu": dict(G=16, n_cu=8, probs=_interleave(I8, FLT, BIN)),
    "float_only": dict(G=512, n_cu=256, probs=FLT),
    "float_one_big": dict(G=512, n_cu=256, probs=[(64, 262143, 0, 200)]),
    "float_batch": dict(G=512, n_cu=256, probs=[(300, 2500, 0, 64)] * 600),
    "dyn_i8_with_float": dict(G=512, n_cu=256, probs=[(10000, 10000, 0, 0)] * 40 + FLT),
}


def case_text(name, probs=None):
    c = CASES[name]
    probs = c["probs"] if probs is None else probs
    return "\n".join([f"{name} {c['G']} {c['n_cu']} 2000 {len(probs)}"] + [" ".join(map(str, p)) for p in probs]) + "\n"


def parse(text):
    t = dict(slots=[], works=[], ham=[], flt=[])
    for line in text.splitlines():
        w = line.split()
        if w[0] == "flt_block_q":
            assert [int(w[1]), int(w[3]), int(w[5])] == [FLT_BLOCK_Q, FLT_ROW_PAD, FLT_MAX_DIM]
        elif w[0] == "n_blocks":
            t.update(n_blocks=int(w[1]), dyn=int(w[3]), part=int(w[5]), good=int(w[7]))
        elif w[0] == "slot":
            t["slots"].append(dict(zip(("nsplit", "q_pad", "part_off", "good_off", "it_off"), map(int, w[2:]))))
        elif w[0] == "work":
            t["works"].append(tuple(map(int, w[1:])))
        elif w[0] == "seg":
            t["seg"] = list(map(int, w[1:]))
        elif w[0] in ("ham", "flt"):
            t[w[0]].append(tuple(map(int, w[1:])))
    return t


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("knn_float_plan")
    src = os.path.join(ROOT, "tests", "cpp", "knn_float_plan_driver.cpp")
    plain, san = str(d / "driver"), str(d / "driver_san")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", src, "-o", plain])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", src, "-o", san])
    return plain, san


def run(drivers, text):
    """Both builds' output, which must agree (a sanitizer finding aborts the second)."""
    outs = [subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout for exe in drivers]
    assert outs[0] == outs[1] and outs[0].endswith("end\n")
    return parse(outs[0])


@pytest.mark.parametrize("name", sorted(CASES))
def test_float_pieces_cover_every_pair_once(drivers, name):
    probs = CASES[name]["probs"]
    t = run(drivers, case_text(name))
    assert len(t["slots"]) == len(probs)
    by_prob = {}
    for p, q0, r0, r1, sp in t["flt"]:
        by_prob.setdefault(p, {}).setdefault(q0, []).append((sp, r0, r1))
    part = 0
    for i, (nq, nt, binary, fdim) in enumerate(probs):
        s = t["slots"][i]
        assert s["part_off"] == part
        part += s["nsplit"] * s["q_pad"]
        if not fdim:
            assert i not in by_prob
            continue
        assert all(w[0] != i for w in t["works"]) and all(h[0] != i for h in t["ham"])
        nqb = (nq + FLT_BLOCK_Q - 1) // FLT_BLOCK_Q
        assert s["q_pad"] == max(nqb, 1) * FLT_BLOCK_Q and s["nsplit"] >= 1
        blocks = by_prob.get(i, {})
        assert sorted(blocks) == [b * FLT_BLOCK_Q for b in range(nqb)]  # every query in exactly one block
        for q0, pieces in blocks.items():
            assert q0 + FLT_BLOCK_Q <= s["q_pad"]
            assert [sp for sp, _, _ in pieces] == list(range(s["nsplit"]))  # one piece per split, in order
            end = 0
            for sp, r0, r1 in pieces:
                assert r0 % FLT_ROW_PAD == 0 and r0 <= r1 <= nt
                assert r0 == end or (r0 >= nt and r1 == r0)  # disjoint, ordered, no gap
                end = max(end, r1)
            assert end == nt  # every train row once
    assert t["part"] == part
    # a long train set under few query blocks is cut, a full batch is not
    if name == "float_one_big":
        assert t["slots"][0]["nsplit"] > 100
    if name == "float_batch":
        assert all(s["nsplit"] == 1 for s in t["slots"])


@pytest.mark.parametrize("name", ["mixed", "mixed_small_gpu", "dyn_i8_with_float"])
def test_other_kinds_unchanged_by_float_problems(drivers, name):
    probs = CASES[name]["probs"]
    keep = [i for i, p in enumerate(probs) if not p[3]]
    full = run(drivers, case_text(name))
    rest = run(drivers, case_text(name, [probs[i] for i in keep]))
    assert rest["flt"] == [] and full["flt"] != []
    assert [(keep[w[0]],) + w[1:] for w in rest["works"]] == full["works"] and full["works"]
    assert rest["seg"] == full["seg"] and (rest["n_blocks"], rest["dyn"]) == (full["n_blocks"], full["dyn"])
    assert [(keep[h[0]],) + h[1:] for h in rest["ham"]] == full["ham"]
    for j, i in enumerate(keep):
        a, b = rest["slots"][j], full["slots"][i]
        assert (a["nsplit"], a["q_pad"]) == (b["nsplit"], b["q_pad"])
