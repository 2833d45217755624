#!/usr/bin/env python
"""Hamming kNN kernel (csrc/hamming.hip): "knn" milliseconds and pairs per second beside the VALU issue floor.

Cases (uniform random rows; the work does not depend on the data):
  a  one 10,000 x 10,000 problem, 32-byte rows (ORB)          mim_knn2_sets_dev
  b  256 such problems in one batch (16 x 16 sets)            mim_batch_run
  c  445 problems of 300 x 2500 rows, 32 bytes                mim_batch_run
  d  case a with 64-byte rows (BRISK / FREAK)                 mim_knn2_sets_dev
Each figure is the median of --reps timed batches after --warmup untimed ones, from the library's own
events around the distance kernels (mim_last_kernel_ms "knn").

The floor: the kernel's inner loop, per train row and lane, is for each of its 4 queries W v_xor_b32 +
W v_bcnt_u32_b32 (W dwords per padded row) + v_lshl_or_b32 + v_max_u32 + 2 v_min_u32, and one v_mov_b32 a
row (counted in the gfx950 listing of knn2_hamming_kernel): VALU_PER_PAIR below.  A wave64 VALU
instruction issues over 2 cycles on a SIMD, so the floor is
pairs x VALU_PER_PAIR x 2 / 64 cycles spread over CUs x 4 SIMDs at the device's clock.  The same count
priced at 4 cycles (what one wave's stream sustains, and what the counters show this kernel's
integer instructions to cost with 4 waves a SIMD: DESIGN.md §13) is reported beside it.

Writes profiles/hamming_knn.json (or --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PER_PAIR = {16: 12.25, 32: 20.25, 64: 36.25}  # by padded row bytes


def floor_ms(pairs, pad, n_cu, clock_hz):
    cycles = pairs * VALU_PER_PAIR[pad] * 2 / 64
    return cycles / (n_cu * 4) / clock_hz * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--clock-mhz", type=float, default=0.0,
                    help="engine clock for the floor (default: the device's reported clock, else the MI355X's "
                         "2400 MHz peak)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hamming_knn.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import torch

    from computervision_objectdetection_featurematching_amd import Matcher, build, default_params
    from computervision_objectdetection_featurematching_amd.synthetic import orb_like
    build.build()
    prop = torch.cuda.get_device_properties(0)
    n_cu = prop.multi_processor_count
    khz = getattr(prop, "clock_rate", 0)  # absent from some torch builds
    clock_hz = args.clock_mhz * 1e6 if args.clock_mhz > 0 else (khz * 1e3 if khz else 2400e6)
    m = Matcher(0)
    m.set_timing(True)
    rng = np.random.default_rng(0xB17)
    prm = default_params(max_iters=100)  # random rows: almost no good matches, RANSAC is not what is timed

    def sets(n_sets, rows, width):
        return [m.add_binary_set(orb_like(rng, rows, width), np.zeros((rows, 2), np.float32)) for _ in range(n_sets)]

    def timed(run):
        ms = []
        for i in range(args.warmup + args.reps):
            run()
            m.batch_results(0) if run.knn_only else m.batch_results(run.n)
            if i >= args.warmup:
                ms.append(m.kernel_ms("knn"))
        return ms

    def case_single(width):
        m.clear_sets()
        (q,), (t,) = sets(1, 10000, width), sets(1, 10000, width)
        idx = torch.zeros((10000, 2), dtype=torch.int32, device="cuda")
        dist = torch.zeros((10000, 2), dtype=torch.float32, device="cuda")

        def run():
            m.knn_sets_dev(q, t, idx, dist)
        run.knn_only = True
        return timed(run), 10000 * 10000, width

    def case_batch(nqs, nts, nq, nt, pairs_of):
        m.clear_sets()
        q, t = sets(nqs, nq, 32), sets(nts, nt, 32)
        probs = np.array(pairs_of(q, t), np.int32)

        def run():
            m.match_batch_async(probs, prm)
        run.knn_only, run.n = False, len(probs)
        return timed(run), len(probs) * nq * nt, 32

    cases = {
        "a": ("1 x (10000 x 10000), 32 B", lambda: case_single(32)),
        "b": ("256 x (10000 x 10000), 32 B", lambda: case_batch(16, 16, 10000, 10000,
                                                                 lambda q, t: [(a, b) for a in q for b in t])),
        "c": ("445 x (300 x 2500), 32 B", lambda: case_batch(445, 445, 300, 2500, lambda q, t: list(zip(q, t)))),
        "d": ("1 x (10000 x 10000), 64 B", lambda: case_single(64)),
    }
    out = dict(device=prop.name, compute_units=n_cu, clock_mhz=clock_hz / 1e6, reps=args.reps, warmup=args.warmup,
               valu_per_pair=VALU_PER_PAIR, cases={})
    for key in args.cases:
        name, fn = cases[key]
        ms, pairs, pad = fn()
        med = statistics.median(ms)
        fl = floor_ms(pairs, pad, n_cu, clock_hz)
        out["cases"][key] = dict(name=name, knn_ms_median=med, knn_ms_min=min(ms), knn_ms_max=max(ms), pairs=pairs,
                                 pairs_per_s=pairs / (med * 1e-3), valu_floor_ms=fl, fraction_of_floor=fl / med,
                                 valu_floor_4cyc_ms=2 * fl, fraction_of_4cyc_floor=2 * fl / med)
        print(f"{key}  {name:32s} knn {med:9.4f} ms (min {min(ms):.4f}, max {max(ms):.4f})  "
              f"{pairs / (med * 1e-3):.3e} pairs/s  floor {fl:.4f} ms ({100 * fl / med:.0f} % of the floor rate; {200 * fl / med:.0f} % at 4 cycles)")
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(written=args.out)))


if __name__ == "__main__":
    main()
