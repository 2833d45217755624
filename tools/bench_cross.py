#!/usr/bin/env python
"""Cross-check matching on binary rows: what the reverse direction costs the distance stage.

Cases (uniform random 32-byte rows; the work does not depend on the data):
  a  one 10,000 x 10,000 problem
  b  445 problems of 300 x 2500 rows
  c  64 problems of 10,000 x 10,000 rows in one batch (8 x 8 sets)
Forms, alternating in one process, each batch fetched before the next starts:
  ratio  filter "ratio": the launches of mim_batch_run, the yardstick
  sweep  filter "cross" with MIM_CROSS_FUSED=0: a second sweep with the two sets swapped
  fused  filter "cross": knn2_hamming_cross_kernel, every pair's popcount taken once
Per case and form: the median, minimum and maximum over --reps timed batches after --warmup untimed ones of
the library's own event times "knn" (the distance kernels) and "ratio" (the ratio or cross compaction), and
the ratios sweep / ratio and fused / ratio of the "knn" medians.

Writes profiles/cross_knn.json (or --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = {"ratio": ("ratio", None), "sweep": ("cross", "0"), "fused": ("cross", "1")}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_knn.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import torch

    from computervision_objectdetection_featurematching_amd import Matcher, build, default_params
    from computervision_objectdetection_featurematching_amd.synthetic import orb_like
    build.build()
    prop = torch.cuda.get_device_properties(0)
    m = Matcher(0)
    m.set_timing(True)
    rng = np.random.default_rng(0xC2055)
    prm = default_params(max_iters=100)  # RANSAC is not what is timed

    def sets(n_sets, rows):
        return [m.add_binary_set(orb_like(rng, rows, 32), np.zeros((rows, 2), np.float32)) for _ in range(n_sets)]

    def case(nqs, nts, nq, nt, pairs_of):
        m.clear_sets()
        q, t = sets(nqs, nq), sets(nts, nt)
        probs = np.array(pairs_of(q, t), np.int32)
        ms = {f: dict(knn=[], ratio=[]) for f in FORMS}
        for i in range(args.warmup + args.reps):
            for form, (filt, fused) in FORMS.items():
                if fused is None:
                    os.environ.pop("MIM_CROSS_FUSED", None)
                else:
                    os.environ["MIM_CROSS_FUSED"] = fused
                m.match_batch_async(probs, prm, filter=filt)
                m.batch_results(len(probs))
                assert int(m.kernel_ms("knn_cross")) == {"ratio": 0, "sweep": 1, "fused": 2}[form]
                if i >= args.warmup:
                    for k in ("knn", "ratio"):
                        ms[form][k].append(m.kernel_ms(k))
        os.environ.pop("MIM_CROSS_FUSED", None)
        return ms, len(probs) * nq * nt

    cases = {
        "a": ("1 x (10000 x 10000), 32 B", lambda: case(1, 1, 10000, 10000, lambda q, t: [(q[0], t[0])])),
        "b": ("445 x (300 x 2500), 32 B", lambda: case(445, 445, 300, 2500, lambda q, t: list(zip(q, t)))),
        "c": ("64 x (10000 x 10000), 32 B", lambda: case(8, 8, 10000, 10000, lambda q, t: [(a, b) for a in q for b in t])),
    }
    out = dict(device=prop.name, compute_units=prop.multi_processor_count, reps=args.reps, warmup=args.warmup, cases={})
    for key in args.cases:
        name, fn = cases[key]
        ms, pairs = fn()
        rec = dict(name=name, pairs=pairs)
        for form in FORMS:
            for k in ("knn", "ratio"):
                v = ms[form][k]
                rec[f"{form}_{k}_ms"] = dict(median=statistics.median(v), min=min(v), max=max(v))
        base = rec["ratio_knn_ms"]["median"]
        rec["sweep_over_ratio"] = rec["sweep_knn_ms"]["median"] / base
        rec["fused_over_ratio"] = rec["fused_knn_ms"]["median"] / base
        rec["fused_slowest_below_sweep_fastest"] = rec["fused_knn_ms"]["max"] < rec["sweep_knn_ms"]["min"]
        out["cases"][key] = rec
        print(f"{key}  {name:28s} knn ms: " + "  ".join(
            f"{f} {rec[f + '_knn_ms']['median']:.4f} [{rec[f + '_knn_ms']['min']:.4f}, {rec[f + '_knn_ms']['max']:.4f}]"
            for f in FORMS) + f"  sweep/ratio {rec['sweep_over_ratio']:.3f}  fused/ratio {rec['fused_over_ratio']:.3f}"
              f"  compaction ms: " + "  ".join(f"{f} {rec[f + '_ratio_ms']['median']:.4f}" for f in FORMS), flush=True)
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(written=args.out)))


if __name__ == "__main__":
    main()
