#!/usr/bin/env python3
"""Writes configs/bench_tilings.json: the kernel tilings bench.py runs its plans with (bench.TILINGS), picked by the autotuner on this GPU.

    python scripts/bench_tilings.py [OUT.json]

One autotuner search per plan of the benchmark: every BASELINE config at its samples per launch, the default config at the per-rank
sample counts of the strong split (K = 16 over 2 / 4 / 8 / 16 ranks) and the drop-in loop at K = 1 and K = 16.  Run it again when a
kernel's tilings change; a plan the table lacks runs on the built-in heuristic tilings."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import bench
    os.environ.pop("MFVI_TUNE_CACHE", None)          # a fresh search for every plan
    out = sys.argv[1] if len(sys.argv) > 1 else bench.TILINGS
    specs = [("engine", name, cfg["k"] if "spl" not in cfg else cfg["spl"]) for name, cfg in bench.CONFIGS.items()]
    specs += [("engine", "cfg2", k) for k in (1, 2, 4, 8)] + [("dropin", "cfg2", 1), ("dropin", "cfg2", 16)]
    table = {}
    for mode, name, k in specs:
        cfg = dict(bench.CONFIGS[name])
        if mode == "dropin":
            eng = bench.DropInLoop(cfg, k, torch, autotune=True)
            n = k
        else:
            cfg["k"] = k
            eng = bench.make_engine(cfg, k, 0, 1, torch, autotune=True)
            n = eng.chunk
        sig = bench.plan_signature(eng.plan.prog, n)
        what = "%s %s, %d samples per launch" % (mode, name, n)
        if sig in table:
            table[sig]["what"] += "; " + what
        else:
            table[sig] = {"what": what, "tunes": bench.plan_tilings(eng.plan)}
        print(what, file=sys.stderr)
        del eng
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
