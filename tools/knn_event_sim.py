"""Count the distance kernel's late-tile insertion events on the CPU (numpy): exact mode, ratio mode and
verdict mode (flip-only events).

usage: python tools/knn_event_sim.py [--config c4] [--scene 0] [--queries 2048] [--offset 0] [--stride 0] [--ratio 0.9]
                                      [--schedule DENSE,EVERY ...] [--problems N]

--schedule: the late loop's refresh schedule (csrc/knn.hip, MIM_KNN_REFRESH_DENSE / _EVERY): a refresh on
every stage for the first DENSE late stages, then on every EVERY-th late stage counted from the first; several
may be given, each is replayed (default: every stage, i.e. 0,1).  A stage off the schedule keeps the partner
copies and the limits the last refresh and the events since left.  --problems N (ragged configs such as c1):
the first N problems of the batch, each problem's whole 64-query waves, summed.

The sample is whole 64-query waves: --queries of them in all, from query --offset on, every --stride-th
wave (0: spread evenly over the whole query set, the default, which weights planted and unplanted queries
as the batch does; 1: contiguous).  On C3/C4 the planted matches are the first 2,000 queries of a model, so
a contiguous sample from 0 describes the planted fifth of the batch only.

Replays one problem of a config with the kernel's layout (csrc/knn.hip): rows of a 32-row block go to
the lane halves ((row % 32) >> 2) & 1, the first 256 rows are early, a stage is 256 rows, the limit of a
lane is fixed inside a 32-row half tile.  An event is a row at or under its lane's limit.  Exact mode:
limit = 2nd smallest of the pair's four values.  Ratio mode: a pair that fails d1^2 >= kappa d2^2 at the
stage's refresh has limit = its minimum.  Verdict mode: such a pair has limit kappa x its minimum (only a
row that could make it pass), records a new minimum without an event, and a lane that takes an event goes
on with the candidate limit.  Prints events per query, the share of (64-query wave, half tile) visits with
at least one event, and the number of sampled queries whose brute-force verdict changes when either d^2
moves by one (the queries verdict mode may have to rescan).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from computervision_objectdetection_featurematching_amd.synthetic import make_config_dataset  # noqa: E402

BIG = np.int64(2**40)


def replay(d, kappa, flip=False, schedule=(0, 1)):
    """d: (nq, nt) exact squared distances (nq a multiple of 64).  kappa = 0: exact mode.  Returns
    (events, wave x half-tile visits, visits with an event)."""
    dense, every = schedule
    nq, nt = d.shape
    m = np.full((2, 2, nq), BIG)  # [half][rank][query]
    o = np.full((2, 2, nq), BIG)
    lim = np.full((2, nq), BIG)
    events = np.zeros(nq, np.int64)
    visits = hits = 0

    def push(h, v, on):
        a, b = m[h, 0], m[h, 1]
        nb = np.maximum(np.minimum(a, b), np.minimum(np.maximum(a, b), v))
        m[h, 1] = np.where(on, nb, b)
        m[h, 0] = np.where(on, np.minimum(a, v), a)

    def second(h):
        return np.minimum(np.maximum(m[h, 0], o[h, 0]), np.minimum(m[h, 1], o[h, 1]))

    for b0 in range(0, nt, 32):
        late = b0 >= 256
        ls = (b0 - 256) // 256  # late stage, counted from the sweep's first
        if late and (b0 - 256) % 256 == 0 and (every == 1 or ls < dense or ls % every == 0):
            for h in range(2):
                o[h] = m[1 - h].copy()
            for h in range(2):
                q1, q2 = np.minimum(m[h, 0], o[h, 0]), second(h)
                fail = (kappa > 0) & (q1.astype(np.float32) >= np.float32(kappa) * q2.astype(np.float32))
                lim[h] = np.where(fail, q1, q2 + (kappa == 0))  # exact mode keeps ties (index order)
                if flip:  # rows that pass against the minimum: (float)d < kappa (float)q1
                    fl = np.ceil(np.float32(kappa) * q1.astype(np.float32)).astype(np.int64)
                    lim[h] = np.where(fail, np.minimum(fl, q1), q2)
        cur = lim.copy()
        hit = np.zeros(nq, bool)
        if flip and late:  # a lane with a row under its limit takes the candidate limit first
            for h in range(2):
                jh = [j for j in range(b0, min(b0 + 32, nt)) if ((j % 32) >> 2) & 1 == h]
                if jh:
                    cur[h] = np.where(d[:, jh].min(1) < cur[h], second(h), cur[h])
        for j in range(b0, min(b0 + 32, nt)):
            h = ((j % 32) >> 2) & 1
            on = d[:, j] < cur[h] if late else np.ones(nq, bool)
            if late:
                events += on
                hit |= on
            push(h, d[:, j], on)
            if flip and late:  # the minimum without an event (the sim keeps no parities: a plain push)
                push(h, d[:, j], ~on)
        if late:
            # the kernel recomputes a limit only on the event path, for the 32-query column tile that took
            # the event (in verdict mode the tracked minimum lowers a pair's values without it)
            ev = np.repeat(hit.reshape(-1, 32).any(1), 32)
            for h in range(2):
                base = cur[h] if flip else lim[h]
                lim[h] = np.where(ev, np.minimum(base, second(h) + (kappa == 0)), base)
            w = hit[: nq // 64 * 64].reshape(-1, 64).any(1)
            visits += w.size
            hits += int(w.sum())
    return int(events.sum()), visits, hits


def dist2(q, t):
    q, t = q.astype(np.float64), t.astype(np.float64)
    return np.rint((q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2.0 * (q @ t.T)).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4")
    ap.add_argument("--scene", type=int, default=0)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--offset", type=int, default=0)
    ap.add_argument("--stride", type=int, default=0, help="in 64-query waves; 0 = spread over the whole set")
    ap.add_argument("--ratio", type=float, default=0.9)
    ap.add_argument("--schedule", nargs="*", default=["0,1"], help="DENSE,EVERY refresh schedules to replay")
    ap.add_argument("--problems", type=int, default=0, help="ragged configs: the first N problems, summed")
    a = ap.parse_args()
    r = float(np.float32(a.ratio))
    kappa = r * r * (1 + 2.0**-18) * (1 + 2.0**-20)
    schedules = [tuple(int(x) for x in sc.split(",")) for sc in a.schedule]
    if a.problems > 0:
        ds = make_config_dataset(a.config)
        ds_list = []
        for m, sc in ds.problems[: a.problems]:
            q = ds.model_desc[m]
            if len(q) >= 64:
                ds_list.append(dist2(q[: len(q) // 64 * 64], ds.scene_desc[sc]))
        what = f"{a.config} first {a.problems} problems ({len(ds_list)} with a whole wave, {sum(len(d) for d in ds_list)} queries)"
    else:
        ds = make_config_dataset(a.config, scene_ids=[a.scene])
        allq = ds.model_desc[0]
        waves = np.arange(a.offset // 64, len(allq) // 64)
        n_w = max(1, a.queries // 64)
        if a.stride > 0:
            waves = waves[:: a.stride][:n_w]
        else:
            waves = waves[np.unique(np.linspace(0, len(waves) - 1, min(n_w, len(waves))).astype(int))]
        ds_list = [dist2(allq[(waves[:, None] * 64 + np.arange(64)[None, :]).ravel()], ds.scene_desc[0])]
        what = f"{a.config} scene {a.scene} {ds_list[0].shape[0]} x {ds_list[0].shape[1]}"
        print(f"{a.config} scene {a.scene}: {len(waves)} waves of 64 queries, waves {waves[0]} .. {waves[-1]} of {len(allq) // 64}")
    for sched in schedules:
        for name, k, flip in (("exact", 0.0, False), ("ratio", kappa, False), ("verdict", kappa, True)):
            ev = vis = hit = nq = 0
            for d in ds_list:
                e, v, h = replay(d, k, flip, sched)
                ev, vis, hit, nq = ev + e, vis + v, hit + h, nq + len(d)
            print(f"{what} refresh {sched[0]},{sched[1]} {name:7s}: {ev / nq:.2f} events per query, "
                  f"{100 * hit / max(vis, 1):.1f} % of wave x half-tile visits take the event path")
    d = np.concatenate([np.sort(x, axis=1)[:, :2] for x in ds_list])
    s2 = d

    def good(d1, d2):
        return np.sqrt(np.float32(d1)) < np.float32(a.ratio) * np.sqrt(np.float32(d2))

    g = good(s2[:, 0], s2[:, 1])
    dep = (good(np.maximum(s2[:, 0] - 1, 0), s2[:, 1]) != g) | (good(s2[:, 0], s2[:, 1] - 1) != g) | \
          (good(s2[:, 0] + 1, s2[:, 1]) != g) | (good(s2[:, 0], s2[:, 1] + 1) != g)
    print(f"{int(g.sum())} of {len(g)} sampled queries pass; {int(dep.sum())} verdicts change when either d^2 moves by one")


if __name__ == "__main__":
    main()
