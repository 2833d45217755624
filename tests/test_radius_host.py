"""The host-callable parts of radius matching (csrc/radius_host.h) on the CPU:
tests/cpp/radius_driver.cpp under a plain and an ASan + UBSan build (a stand-alone program, run as its own
process), whose outputs must agree.

* integer threshold: for a few hundred radii radius_int_threshold's T2 splits the whole range [0, 8,323,200] as
  the literal test sqrtf((float)n) <= r does: checked by the driver against its table of every sqrtf in the range
  and here against numpy's float32 sqrt of the same range.  The radii: exact sqrtf values of integers and their
  nextafter neighbours on both sides, the classes above 4e6 where two integers share a sqrtf (8,000,000 and
  8,000,001), tiny, huge and infinite values, a NaN and negatives.
* float threshold (the form the float kernel uses): the largest float T with sqrtf(T) <= r, likewise.
* Hamming threshold: floor(r) capped at 512, against a scan of the 513 distances.
* argument check: above FLT_EPSILON only.
* merge placement: on random and tied (shared distance bits) runs, of lengths 0, 1 and non-powers of two, the
  places are a permutation and the union equals the sorted input; whole passes over lists with a short last run.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_D2 = 128 * 255 * 255


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("radius")
    src = os.path.join(ROOT, "tests", "cpp", "radius_driver.cpp")
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
    return struct.unpack("<I", struct.pack("<f", float(np.float32(x))))[0]


def _radii():
    f32 = np.float32
    ints = [0, 1, 2, 3, 4, 15, 16, 17, 99, 100, 101, 65535, 65536, 1 << 20, 3999999, 4000000, 4000001, 4194303, 4194304,
            4194305, 7999999, 8000000, 8000001, 8000002, MAX_D2 - 2, MAX_D2 - 1, MAX_D2]
    rng = np.random.default_rng(5)
    ints += [int(v) for v in rng.integers(0, MAX_D2 + 1, 40)] + [int(v) for v in rng.integers(4_000_000, MAX_D2 + 1, 40)]
    out = []
    for n in ints:
        s = np.sqrt(f32(n))
        out += [s, np.nextafter(s, f32(np.inf)), np.nextafter(s, f32(-np.inf))]
    out += [f32(v) for v in rng.uniform(0, 2900, 60)]
    out += [f32(1.2e-7), f32(1e-30), f32(1e-45), f32(0.0), f32(0.5), f32(0.99999994), f32(2884.9), f32(2885.0), f32(2885.1),
            f32(1e10), f32(3.4e38), f32(np.inf), f32(-1.0), f32(-np.inf), f32(np.nan)]
    return out


def test_integer_threshold_over_the_whole_range(drivers):
    radii = _radii()
    assert len(radii) > 300
    lines = [w for w in run(drivers, f"int {len(radii)}\n" + " ".join(f"{_bits(r):x}" for r in radii) + "\n") if w[0] == "int"]
    assert len(lines) == len(radii)
    table = np.sqrt(np.arange(MAX_D2 + 1, dtype=np.float32))  # exact conversions, correctly rounded roots
    assert (np.diff(table) >= 0).all()
    shared = 0
    for r, w in zip(radii, lines):
        t2, ref, lit = int(w[2]), int(w[3]), int(w[4])
        assert int(w[1], 16) == _bits(r)
        expect = -1 if np.isnan(r) else int(np.searchsorted(table, r, side="right")) - 1
        assert t2 == ref == expect and lit == 1, (r, w)
        if 0 <= t2 < MAX_D2:
            assert table[t2] <= r and not table[t2 + 1] <= r
        shared += int(t2 > 4_000_000 and t2 < MAX_D2 and table[t2] == table[t2 - 1])
    assert shared >= 10  # radii whose last passing integer shares its sqrtf with the one before
    by_bits = {int(w[1], 16): int(w[2]) for w in lines}
    s = np.sqrt(np.float32(8000000))
    assert s == np.sqrt(np.float32(8000001)) and by_bits[_bits(s)] >= 8000001
    assert by_bits[_bits(np.nextafter(s, np.float32(0)))] < 8000000
    assert by_bits[_bits(np.float32(np.inf))] == MAX_D2 and by_bits[_bits(np.float32(1e-30))] == 0
    assert by_bits[_bits(np.float32(-1.0))] == -1 and by_bits[_bits(np.float32(np.nan))] == -1


def test_float_threshold(drivers):
    """radius_flt_threshold: the largest float T with sqrtf(T) <= r, checked with the literal compare on T and on the
    float after it, by the driver and by numpy's float32 sqrt."""
    f32 = np.float32
    rng = np.random.default_rng(6)
    radii = _radii() + [f32(v) for v in np.exp(rng.uniform(np.log(1e-30), np.log(3e38), 200))]
    radii += [f32(1.8446743e19), f32(1.8446744e19), f32(1.8446746e19), f32(3.4028235e38), f32(1e-20), f32(3.7e-23), f32(1e-23)]
    lines = [w for w in run(drivers, f"flt {len(radii)}\n" + " ".join(f"{_bits(r):x}" for r in radii) + "\n") if w[0] == "flt"]
    assert len(lines) == len(radii)
    with np.errstate(invalid="ignore", over="ignore"):
        for r, w in zip(radii, lines):
            assert int(w[1], 16) == _bits(r) and w[3] == "1", (r, w)
            T = np.array([int(w[2], 16)], np.uint32).view(np.float32)[0]
            if not r >= 0:
                assert T < 0
            elif np.isinf(r):
                assert np.isinf(T) and T > 0
            else:
                assert T >= 0 and np.sqrt(T) <= r and not np.sqrt(np.nextafter(T, f32(np.inf))) <= r, (r, T)


def test_hamming_threshold_and_argument_check(drivers):
    f32 = np.float32
    radii = [f32(v) for v in (0.0, 0.5, 1.0, 1.5, 31.999, 32.0, 255.5, 511.0, 511.99, 512.0, 513.0, 1e9, np.inf, -0.5, np.nan,
                              1.2e-7, 1e-40)]
    text = f"ham {len(radii)}\n" + " ".join(f"{_bits(r):x}" for r in radii) + "\n"
    text += f"arg {len(radii)}\n" + " ".join(f"{_bits(r):x}" for r in radii) + "\n"
    lines = run(drivers, text)
    ham = [w for w in lines if w[0] == "ham"]
    arg = [w for w in lines if w[0] == "arg"]
    eps = np.finfo(np.float32).eps
    for r, h, a in zip(radii, ham, arg):
        assert int(h[2]) == int(h[3]), (r, h)
        assert int(h[2]) == (-1 if not r >= 0 else min(int(np.floor(min(r, f32(600)))), 512))
        assert int(a[2]) == int(bool(r > eps)), (r, a)
    assert int(arg[radii.index(f32(1.2e-7))][2]) == 1 and int(arg[0][2]) == 0


def _keys(rng, n, tied):
    """n distinct keys, ascending: distance bits << 32 | row, a handful of distances when tied."""
    d = rng.integers(0, 3 if tied else 1 << 30, size=n).astype(np.uint64)
    rows = rng.permutation(1 << 18)[:n].astype(np.uint64)
    return sorted({int(a) << 32 | int(b) for a, b in zip(d, rows)})


@pytest.mark.parametrize("tied", [False, True])
def test_merge_place(drivers, tied):
    rng = np.random.default_rng(11 + tied)
    text, cases = "", []
    for na, nb in [(0, 0), (0, 1), (1, 0), (1, 1), (0, 7), (5, 0), (3, 5), (13, 1), (100, 37), (257, 1000), (2048, 2049)]:
        allk = _keys(rng, na + nb, tied)
        pick = np.zeros(len(allk), bool)
        pick[rng.permutation(len(allk))[:min(na, len(allk))]] = True
        a = [k for k, p in zip(allk, pick) if p]
        b = [k for k, p in zip(allk, pick) if not p]
        text += f"merge {len(a)} {len(b)}\n" + " ".join(f"{k:x}" for k in a + b) + "\n"
        cases.append(allk)
    lines = run(drivers, text)
    merged = [w for w in lines if w[0] == "merged"]
    flags = [w for w in lines if w[0] == "sorted"]
    assert len(merged) == len(flags) == len(cases)
    for allk, m, f in zip(cases, merged, flags):
        assert [int(v, 16) for v in m[1:]] == allk and f[1] == "1"


@pytest.mark.parametrize("tied", [False, True])
def test_merge_passes_sort_a_list(drivers, tied):
    """Runs of `width` merged in passes until one run is left, as the sort kernel does: lengths with a short
    last run, an unpaired run and a single element."""
    rng = np.random.default_rng(21 + tied)
    for n, width in [(1, 4), (9, 4), (13, 4), (4 * 5 + 1, 5), (64, 8), (1000, 7)]:
        keys = _keys(rng, n, tied)
        n = len(keys)
        cur = [keys[i] for i in rng.permutation(n)]
        cur = [k for a in range(0, n, width) for k in sorted(cur[a:a + width])]
        w = width
        while w < n:
            lines = run(drivers, f"pass {n} {w}\n" + " ".join(f"{k:x}" for k in cur) + "\n")
            out = next(x for x in lines if x[0] == "passed")
            assert next(x for x in lines if x[0] == "perm")[1] == "1"
            cur = [int(v, 16) for v in out[1:]]
            w *= 2
            assert all(cur[a:a + w] == sorted(cur[a:a + w]) for a in range(0, n, w))
        assert cur == keys
