#!/usr/bin/env python3
"""Projects the sharded photon shoot (pvol_preprocess_ranks) to N GPUs from ONE GPU.

    python tools/time_shoot_ranks.py --emulate-ranks 2,4,8 [--scene volumescene_h] [--photons 1000000] [--tasks 16384]
                                     [--block 4096] [--render-step-ms 1764,944,488,260] [--link-gbs 50] [--out FILE]

1. The N = 1 shoot runs through the host all-gather branch; the callback records every round's count table (with one rank it
   sees all of them).
2. For each N, rank 0 of N replays: the callback answers each count exchange from the recording, re-dealt rank-major exactly as N
   ranks would send it (task t in slot t / N of rank t % N), so rank 0 shoots exactly its share of every round; it answers the
   counter exchange with rank 0's own row and zeros, and the row exchanges with zero padding (the map rank 0 ends with is not
   the real one: only its timing is used).

Reported per N: rank 0's shoot time (pvol_get_preprocess_seconds minus the time inside the callbacks), the search-structure
build time of the N = 1 run (the build stays replicated and sees the same map on every rank), and an ESTIMATED row exchange: the
map's 144 B per photon all-gathered at an assumed link bandwidth (--link-gbs, NOT measured: no multi-GPU node has run this).
--render-step-ms takes the render step per N (e.g. DESIGN §6's projected steps) to give an end-to-end column.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401  (load torch's HIP runtime first, as tests/conftest.py does)
except Exception:
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emulate-ranks", default="2,4,8")
    ap.add_argument("--scene", default="volumescene_h")
    ap.add_argument("--photons", type=int, default=1000000)
    ap.add_argument("--tasks", type=int, default=16384)
    ap.add_argument("--block", type=int, default=4096)
    ap.add_argument("--render-step-ms", default="", help="render step per N, comma-separated in the order 1,N... (optional)")
    ap.add_argument("--link-gbs", type=float, default=50.0, help="ASSUMED per-GPU all-gather bandwidth for the row-exchange estimate")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ranks = [int(x) for x in args.emulate_ranks.split(",") if x]
    steps = [float(x) * 1e-3 for x in args.render_step_ms.split(",") if x]
    pkg = importlib.import_module("cs348b-pbrt_amd")
    pvol = importlib.import_module("cs348b-pbrt_amd.pvol")
    abi, blob = pkg.abi, pkg.blob
    s = blob.load(os.path.join(ROOT, "tests", "golden", "scene_%s.bin" % args.scene))
    p = abi.params_from_blob(s, n_volume_photons=args.photons)
    pv = pvol.PhotonVolume(p)
    pv.set_scene(abi.SceneHolder(s))
    T = args.tasks
    count_bytes = 4 * (1 + 8 * T)

    # 1. N = 1, recording the count tables (the count exchanges come first, all of this size; the counter exchange follows)
    tables = []
    done_counting = [False]

    def record(data):
        if not done_counting[0] and len(data) == count_bytes:
            tables.append(np.frombuffer(data, np.uint32).copy())
        else:
            done_counting[0] = True
        return [data]
    t0 = time.perf_counter()
    pv.preprocess_ranks(T, 0, 1, allgather=record, block_paths=args.block)
    wall1 = time.perf_counter() - t0
    shoot1, build1 = pv.preprocess_times()
    ex1 = pv.exchange_seconds()
    n_photons = pv.photon_count()
    stats1 = pv.shoot_stats()
    rows = []
    row_bytes = 144.0 * n_photons
    rows.append({"n_ranks": 1, "rank0_shoot_s": shoot1 - ex1, "callback_s": ex1, "grid_build_s": build1, "rounds": len(tables),
                 "row_exchange_est_s": 0.0, "wall_s": wall1})

    # 2. rank 0 of N, replaying the recording
    for N in ranks:
        Lpad = (T + N - 1) // N
        calls = [0]

        def replay(data):
            i = calls[0]
            calls[0] += 1
            if i < len(tables):
                rec = tables[i]
                out = np.zeros((N, 1 + 8 * Lpad), np.uint32)
                for r in range(N):
                    ids = np.arange(r, T, N)
                    out[r, 1:1 + 8 * len(ids)] = rec[1:].reshape(T, 8)[ids].reshape(-1)
                return [out[r].tobytes() for r in range(N)]
            # the counter exchange (rank 0's own row, the others zero), the status words (all zero) and the rows (padding)
            return [data] + [bytes(len(data))] * (N - 1)
        pv.preprocess_ranks(T, 0, N, allgather=replay, block_paths=args.block)
        shoot, _ = pv.preprocess_times()
        ex = pv.exchange_seconds()
        est = row_bytes * (N - 1) / N / (args.link_gbs * 1e9)
        rows.append({"n_ranks": N, "rank0_shoot_s": shoot - ex, "callback_s": ex, "grid_build_s": build1, "rounds": len(tables),
                     "exchanges": calls[0],
                     "row_exchange_est_s": est})
    for i, r in enumerate(rows):
        if i < len(steps):
            r["render_step_s"] = steps[i]
            r["end_to_end_s"] = r["rank0_shoot_s"] + r["row_exchange_est_s"] + r["grid_build_s"] + steps[i]
    if len(steps) >= 1:
        t1 = rows[0]["end_to_end_s"]
        for r in rows:
            if "end_to_end_s" in r:
                r["efficiency"] = t1 / (r["n_ranks"] * r["end_to_end_s"])
    res = {"what": "sharded photon shoot projected from ONE GPU (rank 0 of N replayed from the N = 1 count tables); "
                   "row_exchange_est_s is an estimate at an assumed, unmeasured link bandwidth, not a scaling measurement",
           "scene": args.scene, "requested": args.photons, "n_tasks": T, "block_paths": args.block, "stored": n_photons,
           "row_bytes_all_gathered": row_bytes, "assumed_link_GBps": args.link_gbs, "stats_n1": stats1, "rows": rows}
    pv.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
