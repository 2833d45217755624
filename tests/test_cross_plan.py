"""The distance schedule of a cross-check batch (csrc/knn_schedule.h knn_cross_problems) on the CPU:
tests/cpp/cross_plan_driver.cpp prints the schedule's tables, under a plain and an ASan + UBSan build (a
stand-alone program, run as its own process).

* every shadow is its problem with the sides swapped, and its partials region [nsplit][q_pad] holds the
  problem's train rows and is disjoint from every other region;
* shadows take no good-match or iteration capacity: the totals are those of the batch without the filter;
* binary problems get no shadow pieces under the fused kernel and get them without it;
* without a filter the tables are those of the schedule's own driver for the same input (whose digests
  tests/test_knn_schedule.py pins to the code before).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_Q, HAM_BLOCK_Q, FLT_BLOCK_Q, HAM_TILE_ROWS, FLT_ROW_PAD = 512, 256, 256, 128, 64

# (nq, nt, bin, fdim)
I8 = [(3000, 4000, 0, 0), (700, 12000, 0, 0), (5000, 900, 0, 0), (513, 65, 0, 0), (1, 1, 0, 0)]
BIN = [(64, 70000, 1, 0), (1200, 2500, 1, 0), (257, 129, 1, 0), (5000, 300, 1, 0), (1, 1, 1, 0)]
FLT = [(300, 5000, 0, 64), (5000, 300, 0, 20), (1, 1, 0, 1), (257, 63, 0, 512), (0, 300, 0, 64), (300, 0, 0, 64)]


def _interleave(*lists):
    out = []
    for i in range(max(len(x) for x in lists)):
        out += [x[i] for x in lists if i < len(x)]
    return out


CASES = {
    "mixed": dict(G=512, n_cu=256, probs=_interleave(FLT, I8, BIN)),
    "mixed_small_gpu": dict(G=16, n_cu=8, probs=_interleave(I8, FLT, BIN)),
    "binary_only": dict(G=512, n_cu=256, probs=BIN),
    "dyn_i8": dict(G=512, n_cu=256, probs=[(10000, 10000, 0, 0)] * 30 + BIN[:2]),
}


def case_text(name, filter, fused):
    c = CASES[name]
    head = f"{name} {c['G']} {c['n_cu']} 2000 {filter} {int(fused)} {len(c['probs'])}"
    return "\n".join([head] + [" ".join(map(str, p)) for p in c["probs"]]) + "\n"


def parse(text):
    t = dict(slots=[], works=[], ham=[], flt=[])
    for line in text.splitlines():
        w = line.split()
        if w[0] == "n_blocks":
            t.update(n_blocks=int(w[1]), dyn=int(w[3]), part=int(w[5]), good=int(w[7]))
        elif w[0] == "slot":
            keys = ("nsplit", "q_pad", "part_off", "good_off", "it_off", "shadow", "nq", "nt")
            t["slots"].append(dict(zip(keys, map(int, w[2:]))))
        elif w[0] == "shadow_of":
            t["shadow_of"] = list(map(int, w[1:]))
        elif w[0] == "seg":
            t["seg"] = list(map(int, w[1:]))
        elif w[0] in ("work", "ham", "flt"):
            t[w[0] + "s" if w[0] == "work" else w[0]].append(tuple(map(int, w[1:])))
    return t


def _build(src, exe, sanitize):
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call(["g++", "-std=c++17", *(san if sanitize else ["-O2"]), "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", src), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("cross_plan")
    return (_build("cross_plan_driver.cpp", str(d / "driver"), False),
            _build("cross_plan_driver.cpp", str(d / "driver_san"), True))


def run(drivers, text):
    """Both builds' output, which must agree (a sanitizer finding aborts the second)."""
    outs = [subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout for exe in drivers]
    assert outs[0] == outs[1] and outs[0].endswith("end\n")
    return parse(outs[0])


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_shadow_regions(drivers, name, fused):
    probs = CASES[name]["probs"]
    n = len(probs)
    t = run(drivers, case_text(name, 1, fused))
    plain = run(drivers, case_text(name, 0, fused))
    assert len(t["shadow_of"]) == n and len(plain["slots"]) == n
    n_shadow = sum(1 for (_, _, binary, _) in probs if not (binary and fused))
    assert len(t["slots"]) == n + n_shadow
    # regions: [part_off, part_off + nsplit * q_pad), in list order, one after another, none overlapping
    end = 0
    for s in t["slots"]:
        assert s["part_off"] == end and s["nsplit"] >= 1
        end += s["nsplit"] * s["q_pad"]
    assert t["part"] == end
    seen = set()
    for i, (nq, nt, binary, fdim) in enumerate(probs):
        j = t["shadow_of"][i]
        if binary and fused:
            assert j == -1
            continue
        assert n <= j < n + n_shadow and j not in seen
        seen.add(j)
        s = t["slots"][j]
        assert s["shadow"] == 1 and (s["nq"], s["nt"]) == (nt, nq)
        unit = HAM_BLOCK_Q if binary else FLT_BLOCK_Q if fdim else BLOCK_Q
        # [nsplit][pad(nt)]: one Top2 per train row of the problem and split
        assert s["q_pad"] == max(-(-nt // unit), 1) * unit and s["q_pad"] >= nt
    # no good-match or iteration capacity: the totals and the problems' own shares are the unfiltered batch's
    assert t["good"] == plain["good"]
    for i in range(n):
        a, b = t["slots"][i], plain["slots"][i]
        assert a["shadow"] == 0 and (a["good_off"], a["it_off"], a["q_pad"]) == (b["good_off"], b["it_off"], b["q_pad"])
    for s in t["slots"][n:]:
        assert (s["good_off"], s["it_off"]) == (plain["good"], 2000 * n)


@pytest.mark.parametrize("name", sorted(CASES))
def test_binary_shadow_pieces_only_without_the_fused_kernel(drivers, name):
    probs = CASES[name]["probs"]
    n = len(probs)
    fused, swept = run(drivers, case_text(name, 1, True)), run(drivers, case_text(name, 1, False))
    assert all(h[0] < n for h in fused["ham"])  # the problems' own pieces alone
    assert [h for h in swept["ham"] if h[0] >= n]
    for i, (nq, nt, binary, _) in enumerate(probs):
        if not binary:
            continue
        j = swept["shadow_of"][i]
        pieces = [h for h in swept["ham"] if h[0] == j]
        s = swept["slots"][j]
        # every (train row as query, query row as train row) pair once: per query block the splits in order
        blocks = {}
        for _, q0, r0, r1, sp in pieces:
            assert q0 % HAM_BLOCK_Q == 0 and r0 % HAM_TILE_ROWS == 0
            blocks.setdefault(q0, []).append((sp, r0, r1))
        assert sorted(blocks) == [b * HAM_BLOCK_Q for b in range(-(-nt // HAM_BLOCK_Q))]
        for its in blocks.values():
            assert [sp for sp, _, _ in its] == list(range(s["nsplit"]))
            assert its[0][1] == 0 and its[-1][2] == nq and all(a[2] == b[1] for a, b in zip(its, its[1:]))
    # the float and i8 kinds sweep their shadows either way
    for t in (fused, swept):
        for i, (nq, nt, binary, fdim) in enumerate(probs):
            if binary or nt == 0:
                continue
            j = t["shadow_of"][i]
            assert any(w[0] == j for w in (t["flt"] if fdim else t["works"])), (i, j)


@pytest.mark.parametrize("name", sorted(CASES))
def test_without_a_filter_the_tables_are_unchanged(drivers, name, tmp_path):
    """filter 0 goes through knn_schedule alone: the same lines as the generic-float plan's driver prints."""
    c = CASES[name]
    ref_exe = _build("knn_float_plan_driver.cpp", str(tmp_path / "ref"), False)
    text = "\n".join([f"{name} {c['G']} {c['n_cu']} 2000 {len(c['probs'])}"] + [" ".join(map(str, p)) for p in c["probs"]])
    ref = subprocess.run([ref_exe], input=text + "\n", capture_output=True, text=True, check=True).stdout
    mine = subprocess.run([drivers[0]], input=case_text(name, 0, True), capture_output=True, text=True, check=True).stdout
    keep = ("n_blocks", "work", "seg", "ham", "flt")
    pick = lambda out: [l for l in out.splitlines() if l.split()[0] in keep]
    assert pick(mine) == pick(ref) and any(l.startswith("work") or l.startswith("ham") for l in pick(ref))
    slots = lambda out: [l.split()[1:7] for l in out.splitlines() if l.startswith("slot")]
    assert slots(mine) == slots(ref)
