#!/usr/bin/env python
"""Generic-float kNN kernel (csrc/knn_float.hip): "knn" milliseconds and pairs per second beside the VALU
issue floor, and the comparison with the 128-D fp32 kernel that mim_set_create routes non-integer rows to
(knn2_f32_kernel, csrc/knn.hip).

Cases (non-integer rows; the work does not depend on the data):
  a  one 10,000 x 10,000 problem, dim 128                     mim_knn2_sets_dev
  b  96 such problems in one batch (8 x 12 sets)              mim_batch_run
  c  445 problems of 300 x 2500 rows, dim 64                  mim_batch_run
  d  one 10,000 x 10,000 problem, dim 256                     mim_knn2_sets_dev
Each figure is the median of --reps timed batches after --warmup untimed ones, from the library's own
events around the distance kernels (mim_last_kernel_ms "knn").  For a and b the same rows are also
registered with mim_set_create and the two paths run in alternation in this process; the ratio of the
medians and both spreads are written.

The floor prices the loop's own VALU instructions per pair and lane, counted in the gfx950 listing of
knn2_float_kernel (VALU_PER_PAIR below: per round of 16 floats 8 v_pk_add_f32 with a negated operand,
8 v_pk_mul_f32 and 8 v_pk_add_f32, the first round's sums elided; 7 packed and 1 scalar add of the
reduction; the compare against m2sq and the loop's moves; the streamed path's per-round address moves
shared by its 4 rows), at 2 cycles per wave64 instruction and, beside it, at 4:
pairs x VALU_PER_PAIR x cycles / 64 spread over CUs x 4 SIMDs at the device's clock.

Writes profiles/float_knn.json (or --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PER_PAIR = {64: 100, 128: 196, 256: 555}  # by dim


def floor_ms(pairs, dim, n_cu, clock_hz):
    cycles = pairs * VALU_PER_PAIR[dim] * 2 / 64
    return cycles / (n_cu * 4) / clock_hz * 1e3


def rows(rng, n, dim):
    """Non-integer rows: square roots of L1-normalised gamma draws (RootSIFT-like)."""
    v = rng.gamma(0.5, 1.0, size=(n, dim))
    v /= v.sum(axis=1, keepdims=True)
    return np.sqrt(v).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--clock-mhz", type=float, default=0.0,
                    help="engine clock for the floor (default: the device's reported clock, else the MI355X's "
                         "2400 MHz peak)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "float_knn.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import torch

    from computervision_objectdetection_featurematching_amd import Matcher, build, default_params
    build.build()
    prop = torch.cuda.get_device_properties(0)
    n_cu = prop.multi_processor_count
    khz = getattr(prop, "clock_rate", 0)  # absent from some torch builds
    clock_hz = args.clock_mhz * 1e6 if args.clock_mhz > 0 else (khz * 1e3 if khz else 2400e6)
    m = Matcher(0)
    m.set_timing(True)
    rng = np.random.default_rng(0xF10A7)
    prm = default_params(max_iters=100)  # random rows: almost no good matches, RANSAC is not what is timed

    def sets(n_sets, n, dim, both):
        """Set ids as generic-float sets and, with `both`, the same rows as mim_set_create sets."""
        new, old = [], []
        for _ in range(n_sets):
            d, kp = rows(rng, n, dim), np.zeros((n, 2), np.float32)
            new.append(m.add_float_set(d, kp))
            if both:
                old.append(m.add_set(d, kp))
        return new, old

    def timed(runs):
        """runs: the paths to time in alternation; the "knn" milliseconds of each."""
        ms = [[] for _ in runs]
        for i in range(args.warmup + args.reps):
            for k, run in enumerate(runs):
                run()
                m.batch_results(0) if run.knn_only else m.batch_results(run.n)
                if i >= args.warmup:
                    ms[k].append(m.kernel_ms("knn"))
        return ms

    def case_single(dim, both):
        m.clear_sets()
        (q, t), (qo, to) = zip(*[sets(1, 10000, dim, both) for _ in range(2)])
        idx = torch.zeros((10000, 2), dtype=torch.int32, device="cuda")
        dist = torch.zeros((10000, 2), dtype=torch.float32, device="cuda")

        def knn(a, b):
            def run():
                m.knn_sets_dev(a, b, idx, dist)
            run.knn_only = True
            return run
        runs = [knn(q[0], t[0])] + ([knn(qo[0], to[0])] if both else [])
        return timed(runs), 10000 * 10000, dim

    def case_batch(nqs, nts, nq, nt, dim, pairs_of, both):
        m.clear_sets()
        (q, qo), (t, to) = sets(nqs, nq, dim, both), sets(nts, nt, dim, both)

        def batch(a, b):
            probs = np.array(pairs_of(a, b), np.int32)

            def run():
                m.match_batch_async(probs, prm)
            run.knn_only, run.n = False, len(probs)
            return run
        runs = [batch(q, t)] + ([batch(qo, to)] if both else [])
        return timed(runs), runs[0].n * nq * nt, dim

    cases = {
        "a": ("1 x (10000 x 10000), dim 128", lambda: case_single(128, True)),
        "b": ("96 x (10000 x 10000), dim 128", lambda: case_batch(8, 12, 10000, 10000, 128,
                                                                   lambda q, t: [(a, b) for a in q for b in t], True)),
        "c": ("445 x (300 x 2500), dim 64", lambda: case_batch(445, 445, 300, 2500, 64, lambda q, t: list(zip(q, t)),
                                                                False)),
        "d": ("1 x (10000 x 10000), dim 256", lambda: case_single(256, False)),
    }
    out = dict(device=prop.name, compute_units=n_cu, clock_mhz=clock_hz / 1e6, reps=args.reps, warmup=args.warmup,
               valu_per_pair=VALU_PER_PAIR, cases={})
    for key in args.cases:
        name, fn = cases[key]
        ms, pairs, dim = fn()
        new = ms[0]
        med = statistics.median(new)
        fl = floor_ms(pairs, dim, n_cu, clock_hz)
        rec = dict(name=name, knn_ms_median=med, knn_ms_min=min(new), knn_ms_max=max(new), pairs=pairs,
                   pairs_per_s=pairs / (med * 1e-3), valu_floor_ms=fl, fraction_of_floor=fl / med,
                   valu_floor_4cyc_ms=2 * fl, fraction_of_4cyc_floor=2 * fl / med)
        line = (f"{key}  {name:32s} knn {med:9.4f} ms (min {min(new):.4f}, max {max(new):.4f})  "
                f"{pairs / (med * 1e-3):.3e} pairs/s  floor {fl:.4f} ms ({100 * fl / med:.0f} % of the floor rate; "
                f"{200 * fl / med:.0f} % at 4 cycles)")
        if len(ms) > 1:
            old = ms[1]
            omed = statistics.median(old)
            rec.update(set_create_knn_ms_median=omed, set_create_knn_ms_min=min(old), set_create_knn_ms_max=max(old),
                       speedup_over_set_create=omed / med, faster_beyond_spread=max(new) < min(old))
            line += f"\n   same rows through mim_set_create: {omed:9.4f} ms (min {min(old):.4f}, max {max(old):.4f})  x{omed / med:.2f}"
        out["cases"][key] = rec
        print(line, flush=True)
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(written=args.out)))


if __name__ == "__main__":
    main()
