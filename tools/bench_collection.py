#!/usr/bin/env python
"""knnMatch over a train collection (mim_knn_collection_dev, csrc/knn_coll.hip): milliseconds of
the distance kernels ("knn") and of the merge ("ratio") at k = 1, 2, 4, 8, 16, beside the same (query, image)
problems through the entries that existed before it.

Shapes: views = 5 scene sets of 2,500 rows against a collection of 89 views of 300 rows (445 pairs), and
single = one 10,000-row query against one 10,000-row image; each for
  sift  integer 128-D rows of mim_set_create      collection: the i8 MFMA top-k kernel
  bin   binary rows of 32 bytes                   collection: the Hamming top-k kernel
  f32   non-integer float rows of dim 128         collection: the float top-k kernel
Yardsticks in the same process, on the same sets:
  batch_k*     mim_knn_batch_dev over the pairs (for sift rows: the float top-k kernel), whose per-pair lists a
               caller would still have to merge on the host;
  existing_k2  sift only: mim_batch_run (views; RANSAC capped and not timed) / mim_knn2_sets_dev (single), the
               k = 2 i8 MFMA kernel.
Every form of a shape runs in alternation: --warmup untimed rounds, then --reps timed ones; each figure is the
median, minimum and maximum of the library's own events (mim_last_kernel_ms).

Writes profiles/knn_collection.json (or --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_knn_topk import rows  # noqa: E402  (the same row generators)

KS = [1, 2, 4, 8, 16]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kinds", default="sift,bin,f32")
    ap.add_argument("--shapes", default="views,single")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_collection.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import torch

    from computervision_objectdetection_featurematching_amd import Matcher, build, default_params
    build.build()
    prop = torch.cuda.get_device_properties(0)
    m = Matcher(0)
    m.set_timing(True)
    rng = np.random.default_rng(0xC011)
    prm = default_params(max_iters=100)  # random rows: almost no good matches, RANSAC is not what is timed
    add = {"bin": m.add_binary_set, "f32": m.add_float_set, "sift": m.add_set}
    shapes = {"views": (5, 2500, 89, 300), "single": (1, 10000, 1, 10000)}
    out = dict(device=prop.name, compute_units=prop.multi_processor_count, reps=args.reps, warmup=args.warmup, cases={})
    for shape in args.shapes.split(","):
        n_q, nq, n_img, nt = shapes[shape]
        for kind in args.kinds.split(","):
            m.clear_sets()
            q = [add[kind](rows(rng, kind, nq), np.zeros((nq, 2), np.float32)) for _ in range(n_q)]
            t = [add[kind](rows(rng, kind, nt), np.zeros((nt, 2), np.float32)) for _ in range(n_img)]
            probs = np.array([(a, b) for a in q for b in t], np.int32)
            n = len(probs)
            idx = torch.zeros(n * nq * 16, dtype=torch.int32, device="cuda")
            img = torch.zeros(n_q * nq * 16, dtype=torch.int32, device="cuda")
            dist = torch.zeros(n * nq * 16, dtype=torch.float32, device="cuda")
            groups = {}

            def coll(k):
                def run():
                    m.knn_collection_dev(q, t, k, idx, img, dist)
                    m.batch_results(0)
                    groups[k] = int(m.kernel_ms("knn_coll_groups"))
                return run

            def batch(k):
                def run():
                    m.knn_batch_dev(probs, k, idx, dist)
                    m.batch_results(0)
                return run

            def existing():
                if n == 1:
                    m.knn_sets_dev(q[0], t[0], idx, dist)
                    m.batch_results(0)
                else:
                    m.match_batch_async(probs, prm)
                    m.batch_results(n)
            forms = [(f"coll_k{k}", coll(k)) for k in KS] + [(f"batch_k{k}", batch(k)) for k in KS]
            if kind == "sift":
                forms.append(("existing_k2", existing))
            knn = {name: [] for name, _ in forms}
            merge = {name: [] for name, _ in forms}
            for i in range(args.warmup + args.reps):
                for name, run in forms:
                    run()
                    if i >= args.warmup:
                        knn[name].append(m.kernel_ms("knn"))
                        merge[name].append(m.kernel_ms("ratio"))
            rec = dict(query_sets=n_q, nq=nq, images=n_img, nt=nt, pairs=n_q * nq * n_img * nt,
                       i8_splits=int(m.kernel_ms("knn_coll_i8_splits")), forms={})
            print(f"{shape} {kind}: {n_q} x {nq} rows against {n_img} x {nt} rows", flush=True)
            for name, _ in forms:
                f = dict(knn_ms_median=statistics.median(knn[name]), knn_ms_min=min(knn[name]), knn_ms_max=max(knn[name]))
                if name != "existing_k2":
                    f.update(merge_ms_median=statistics.median(merge[name]), merge_ms_min=min(merge[name]),
                             merge_ms_max=max(merge[name]))
                rec["forms"][name] = f
            for k in KS:
                c, b = rec["forms"][f"coll_k{k}"], rec["forms"][f"batch_k{k}"]
                c["groups"] = groups[k]
                # the same pairs on the entry that existed before: ratio of medians, and the range the two spreads allow
                c["batch_over_coll_knn"] = b["knn_ms_median"] / c["knn_ms_median"]
                c["batch_over_coll_knn_min"] = b["knn_ms_min"] / c["knn_ms_max"]
                c["batch_over_coll_knn_max"] = b["knn_ms_max"] / c["knn_ms_min"]
                line = (f"   k{k:<2d} collection knn {c['knn_ms_median']:9.4f} ms (min {c['knn_ms_min']:.4f}, max "
                        f"{c['knn_ms_max']:.4f}) merge {c['merge_ms_median']:.4f} ms, {groups[k]} group(s); batch knn "
                        f"{b['knn_ms_median']:9.4f} ms (min {b['knn_ms_min']:.4f}, max {b['knn_ms_max']:.4f}) merge "
                        f"{b['merge_ms_median']:.4f} ms: x{c['batch_over_coll_knn']:.2f} "
                        f"({c['batch_over_coll_knn_min']:.2f}-{c['batch_over_coll_knn_max']:.2f})")
                print(line, flush=True)
            if kind == "sift":
                e = rec["forms"]["existing_k2"]
                c = rec["forms"]["coll_k2"]
                c["coll_over_existing_k2"] = c["knn_ms_median"] / e["knn_ms_median"]
                print(f"   existing k = 2 i8 kernel {e['knn_ms_median']:.4f} ms (min {e['knn_ms_min']:.4f}, max "
                      f"{e['knn_ms_max']:.4f}): the collection at k = 2 takes x{c['coll_over_existing_k2']:.2f} of it", flush=True)
            out["cases"][f"{shape}_{kind}"] = rec
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(written=args.out)))


if __name__ == "__main__":
    main()
