"""A/B: basic-slack deactivation on the shards of one process on / off (simplex_set_deactivate_shards),
alternating on the same box.  Whole twoPhaseMethod solves on peer-memory virtual shards -- config 4 at
W = 4, config 5 at W = 8 -- with the per-phase pivot-loop times (simplex_last_phase_seconds).  Virtual
shards share one GPU: these are not multi-GPU timings.
usage: python tools/deact_shards_ab.py [repeats (default 2)] [config:W ...]"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (CONFIGS)


def main():
    import torch

    torch.cuda.set_device(0)
    import simplexoncuda_amd as sx

    args = sys.argv[1:]
    repeats = int(args.pop(0)) if args and args[0].isdigit() else 2
    cases = [(a.split(":")[0], int(a.split(":")[1])) for a in args] or [("config4", 4), ("config5", 8)]
    lib = sx.load()
    for cfg, W in cases:
        n, m, seed = bench.CONFIGS[cfg]
        prob = sx.generateRandomProblemDevice(n, m, seed, 1, 100)
        for rep in range(repeats):
            for on in (1, 0):
                h0 = lib.simplex_hang_recoveries()
                try:
                    sx.set_virtual_ranks(W)
                    sx.set_p2p(1)
                    sx.set_deactivate_shards(on)
                    t0 = time.perf_counter()
                    res = sx.twoPhaseMethodEx(prob)
                    dt = time.perf_counter() - t0
                finally:
                    sx.set_deactivate_shards(1)
                    sx.set_p2p(-1)
                    sx.set_virtual_ranks(1)
                ph = (ctypes.c_double * 2)()
                lib.simplex_last_phase_seconds(ph)
                print(json.dumps({"config": cfg, "W": W, "deactivate_shards": on, "repeat": rep,
                                  "status": sx.STATUS_NAMES.get(res.status), "pivots": list(res.pivots),
                                  "objective": res.optimal_value, "seconds": dt, "pivot_loop_s": [ph[0], ph[1]],
                                  "pivots_per_s": [res.pivots[k] / ph[k] if ph[k] > 0 else None for k in (0, 1)],
                                  "hang_recoveries": lib.simplex_hang_recoveries() - h0}), flush=True)
        prob.close()


if __name__ == "__main__":
    main()
