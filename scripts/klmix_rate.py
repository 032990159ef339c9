"""What a scale-mixture prior costs an iteration, with the protocol of scripts/kl_rate.py.

The cfg2 shape of bench.py (256x256 denoising, input depth 16, the 26-layer skip net, K = 16) with the tilings of configs/bench_tilings.json.
Every timed loop is warmed up, then timed in windows that end in a synchronise; a figure is the minimum over its windows, every window is
kept, and the run-to-run spread of a figure is (max - min) / min over its windows.

  default path  ElboEngine.step with kl_type='reverse' on this build and on a library built from the PARENT commit's sources (--parent-lib),
                each in a fresh child process (the library path is read at import), the two builds alternated, --rounds times each.  No
                kernel or launch of that path changed: the two must agree inside the spread.
  mixture       the same iteration with kl_type='forward' and a two-component prior_mixture against kl_type='forward' alone (this build,
                this process, alternated); a 16-fit FitBatch at 256x256, K = 1, all rows forward, with no row (the typed update), half of
                the rows and all rows on a mixture (the update with the prior table).
Writes profiles/kl_mixture_rate.json.  The figures are recorded, not gated.

  --family      instead of the two sections above: every path of the KL kernel family on this build against the
                parent's, each in fresh child processes alternated as the default path is: the reverse, the forward and the mixture engine,
                and the 16-fit batch with every row reverse and every row on a mixture.  Per path this / parent - 1 must lie inside the
                band, the larger of the two builds' spreads (`inside_spread`; the exit status is 1 if a path is outside).
                Writes profiles/kl_family_rate.json.

usage: python scripts/klmix_rate.py [--parent-lib PATH/libmfvi_hip.so] [--family] [--iters 100] [--rounds 3] [--out profiles/...json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MIX = {"pi": [0.5, 0.5], "sigma": [1.0, 0.0025]}      # spike and slab


def window(torch, fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def spread(v):
    return (max(v) - min(v)) / min(v)


def engine(torch, kl_type, **kw):
    import numpy as np
    import bench
    from mfvi_dip_mia_amd.engine import ElboEngine
    from mfvi_dip_mia_amd.runner import phantom
    cfg = bench.CONFIGS["cfg2"]; hp, S = cfg["hp"], cfg["size"]
    eng = ElboEngine(S, S, task="den", K=cfg["k"], input_depth=cfg["input_depth"], temp=hp["temp"], sigma=hp["sigma"], lr=hp["lr"], seed=hp["seed"],
                     autotune=False, kl_type=kl_type, **kw)
    eng.tilings = bench.pin_tilings(eng.plan, eng.chunk)
    rng = np.random.default_rng(hp["seed"] + 1)
    img = phantom(S, S, hp["seed"])
    eng.set_target(torch.from_numpy(np.clip(img + rng.normal(scale=hp["p_sigma"], size=img.shape), 0, 1).astype(np.float32)))
    return eng


PATHS = ("reverse", "forward", "mixture", "batch16_reverse", "batch16_mixture")


def batch(torch, F, kl_type, prior_mixture, target):
    import numpy as np
    import bench
    from mfvi_dip_mia_amd import FitBatch
    cfg = bench.CONFIGS["cfg2"]; hp, S = cfg["hp"], cfg["size"]
    fb = FitBatch(S, S, F, task="den", K=1, input_depth=cfg["input_depth"], temp=[hp["temp"] * 2 ** (f % 4) for f in range(F)], sigma=hp["sigma"],
                  lr=hp["lr"], seed=hp["seed"], autotune=False, kl_type=kl_type, prior_mixture=prior_mixture)
    fb.plan.set_fits(0)                                                  # tilings are set with the mode off
    bench.pin_tilings(fb.plan, 16)
    fb.plan.set_fits(1, fb.stride, fb.stride)
    fb.set_targets(torch.from_numpy(np.stack([target] * F)))
    return fb


def child(iters, path):
    """One fresh process: one path's iteration on whatever library MFVI_LIB_PATH names -> one JSON line."""
    from mfvi_dip_mia_amd import _lib as L
    import torch
    mix = MIX if path.endswith("mixture") else None
    eng = engine(torch, "forward" if mix or path == "forward" else "reverse", prior_mixture=mix)
    step = eng.step
    if path.startswith("batch16"):
        step = batch(torch, 16, "forward" if mix else "reverse", mix, eng.target.cpu().numpy()).step
    window(torch, step, 30)
    print(json.dumps(dict(windows_ms=[window(torch, step, iters) for _ in range(3)], lib=L.LIB_PATH, tilings=eng.tilings)))


def against_parent(a, path):
    """`path` on this build and, with --parent-lib, on the parent's: fresh processes, alternated (before this process opens the GPU)."""
    off = {"this": [], "parent": []}
    builds = [("this", None)] + ([("parent", os.path.abspath(a.parent_lib))] if a.parent_lib else [])
    for _ in range(a.rounds):
        for name, lib in builds:
            env = dict(os.environ)
            env.pop("MFVI_LIB_PATH", None)
            if lib:
                env["MFVI_LIB_PATH"] = lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--iters", str(a.iters)], env=env, capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:
                raise SystemExit("child (%s, %s) failed with %d:\n%s" % (path, name, r.returncode, r.stderr[-2000:]))
            off[name] += json.loads(r.stdout.strip().splitlines()[-1])["windows_ms"]
    res = dict(windows_ms=off, ms={k: min(v) for k, v in off.items() if v}, spread={k: spread(v) for k, v in off.items() if v})
    if off["parent"]:
        d = min(off["this"]) / min(off["parent"]) - 1.0
        band = max(spread(off["this"]), spread(off["parent"]))
        res.update(this_over_parent_minus_1=d, band=band, inside_spread=bool(abs(d) <= band))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--family", action="store_true")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", choices=PATHS, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.iters, a.child)
    out = a.out or os.path.join(ROOT, "profiles", "kl_family_rate.json" if a.family else "kl_mixture_rate.json")
    res = dict(config="cfg2", size=256, K=16, iterations_per_window=a.iters, prior_mixture=MIX)
    if a.family:
        res["paths"] = {}
        for p in PATHS:
            res["paths"][p] = against_parent(a, p)
            print(p, json.dumps({k: v for k, v in res["paths"][p].items() if k != "windows_ms"}), flush=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        return int(not all(r.get("inside_spread", True) for r in res["paths"].values()))
    res["default_path"] = against_parent(a, "reverse")
    # ---- the mixture prior, this process
    import torch
    from mfvi_dip_mia_amd.rowbatch import check_prior_mixture, mixture_struct
    e_fwd, e_mix = engine(torch, "forward"), engine(torch, "forward", prior_mixture=MIX)
    variants = [("step_forward", e_fwd.step), ("step_mixture", e_mix.step)]
    F = 16
    # ONE batch serves the three variants (its prior table is swapped): some of several batches of one process step 1.5-1.7x slower than
    # the others whatever they compute (scripts/batchbook_rate.py)
    fb = batch(torch, F, "forward", MIX, e_fwd.target.cpu().numpy())
    pm = check_prior_mixture(MIX)
    half = b"".join(bytes(mixture_struct(pm if f % 2 else None)) for f in range(F))
    tables = dict(none=None, half=torch.frombuffer(bytearray(half), dtype=torch.uint8).cuda(), all=fb._mix_dev)

    def batch_step(which):
        def fn():
            fb._mix_dev = tables[which]
            fb.step()
        return fn
    variants += [("fitbatch16_" + k, batch_step(k)) for k in tables]
    for _, fn in variants:
        window(torch, fn, 20)
    ms = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            ms[name].append(window(torch, fn, a.iters))
    t = {k: min(v) for k, v in ms.items()}
    res["mixture"] = dict(windows_ms=ms, ms=t, spread={k: spread(v) for k, v in ms.items()}, step_delta_ms=t["step_mixture"] - t["step_forward"],
                          fitbatch16_all_delta_ms=t["fitbatch16_all"] - t["fitbatch16_none"],
                          fitbatch16_half_delta_ms=t["fitbatch16_half"] - t["fitbatch16_none"], kl_forward=e_fwd.losses()[1], kl_mixture=e_mix.losses()[1],
                          tilings=e_mix.tilings)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    sys.exit(main())
