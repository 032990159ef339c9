"""What the total-variation term costs an iteration, and that it costs nothing when it is off.

The cfg2 shape of bench.py (256x256 denoising, input depth 16, the 26-layer skip net, K = 16) with the tilings of configs/bench_tilings.json.
Every timed loop is warmed up, then timed in windows that end in a synchronise; a figure is the minimum over its windows, every window is
kept, and the run-to-run spread of a figure is (max - min) / min over its windows.

  off path   ElboEngine.step with the term off, on this build and on a library built from the PARENT commit's sources (--parent-lib), each
             in a fresh child process (the library path is read at import), the two builds alternated, --rounds times each.  No kernel or
             launch was added to that path: the two must agree inside the spread.
  on path    the same iteration with tv_weight > 0 (this build, this process, alternated with the term off);
             the two launches alone: device events around 100 mfvi_tv_term calls at the iteration's shape (n_fits 1, S 16, C 2);
             a 16-fit FitBatch at 256x256, K = 1, with the term on and off.
Writes profiles/tv_rate.json.  The on-path figures are recorded, not gated.

usage: python scripts/tv_rate.py [--parent-lib PATH/libmfvi_hip.so] [--iters 100] [--rounds 3] [--out profiles/tv_rate.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TV_WEIGHT = 0.05


def window(torch, fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def spread(v):
    return (max(v) - min(v)) / min(v)


def engine(torch, tv_weight):
    import numpy as np
    import bench
    from mfvi_dip_mia_amd.engine import ElboEngine
    from mfvi_dip_mia_amd.runner import phantom
    cfg = bench.CONFIGS["cfg2"]; hp, S = cfg["hp"], cfg["size"]
    kw = dict(tv_weight=tv_weight) if tv_weight else {}                  # (the parent's engine has no such keyword)
    eng = ElboEngine(S, S, task="den", K=cfg["k"], input_depth=cfg["input_depth"], temp=hp["temp"], sigma=hp["sigma"], lr=hp["lr"], seed=hp["seed"],
                     autotune=False, **kw)
    eng.tilings = bench.pin_tilings(eng.plan, eng.chunk)
    rng = np.random.default_rng(hp["seed"] + 1)
    img = phantom(S, S, hp["seed"])
    eng.set_target(torch.from_numpy(np.clip(img + rng.normal(scale=hp["p_sigma"], size=img.shape), 0, 1).astype(np.float32)))
    return eng


def child(iters):
    """One fresh process: the off-path iteration on whatever library MFVI_LIB_PATH names -> one JSON line."""
    from mfvi_dip_mia_amd import _lib as L
    if os.environ.get("MFVI_LIB_PATH"):                                  # the parent commit's library lacks the two new symbols
        for name in ("mfvi_tv_term", "mfvi_tv_term_scratch_bytes"):
            L.SIGNATURES.pop(name, None)
    import torch
    eng = engine(torch, 0.0)
    window(torch, eng.step, 30)
    print(json.dumps(dict(windows_ms=[window(torch, eng.step, iters) for _ in range(3)], lib=L.LIB_PATH, tilings=eng.tilings)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tv_rate.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.iters)
    res = dict(config="cfg2", size=256, K=16, iterations_per_window=a.iters, tv_weight=TV_WEIGHT, tv_beta=0.5)
    # ---- off path: this build against the parent's, fresh processes, alternated (before this process opens the GPU)
    off = {"this": [], "parent": []}
    builds = [("this", None)] + ([("parent", os.path.abspath(a.parent_lib))] if a.parent_lib else [])
    for _ in range(a.rounds):
        for name, lib in builds:
            env = dict(os.environ)
            env.pop("MFVI_LIB_PATH", None)
            if lib:
                env["MFVI_LIB_PATH"] = lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters)], env=env, capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:
                raise SystemExit("child (%s) failed with %d:\n%s" % (name, r.returncode, r.stderr[-2000:]))
            off[name] += json.loads(r.stdout.strip().splitlines()[-1])["windows_ms"]
    res["off_path"] = dict(windows_ms=off, ms={k: min(v) for k, v in off.items() if v}, spread={k: spread(v) for k, v in off.items() if v})
    if off["parent"]:
        d = min(off["this"]) / min(off["parent"]) - 1.0
        band = max(spread(off["this"]), spread(off["parent"]))
        res["off_path"].update(this_over_parent_minus_1=d, inside_spread=bool(abs(d) <= band))
    # ---- on path, this process
    import numpy as np
    import torch
    import bench
    from mfvi_dip_mia_amd import FitBatch, _lib as L
    from mfvi_dip_mia_amd.runner import phantom
    e_off, e_on = engine(torch, 0.0), engine(torch, TV_WEIGHT)
    variants = [("step_off", e_off.step), ("step_on", e_on.step)]
    cfg = bench.CONFIGS["cfg2"]; hp, S, F = cfg["hp"], cfg["size"], 16
    tgt = e_off.target.cpu().numpy()

    def batch(tv_weight):
        fb = FitBatch(S, S, F, task="den", K=1, input_depth=cfg["input_depth"], temp=[hp["temp"] * 2 ** (f % 4) for f in range(F)], sigma=hp["sigma"],
                      lr=hp["lr"], seed=hp["seed"], autotune=False, tv_weight=tv_weight)
        fb.plan.set_fits(0)                                              # tilings are set with the mode off
        bench.pin_tilings(fb.plan, 16)
        fb.plan.set_fits(1, fb.stride, fb.stride)
        fb.set_targets(torch.from_numpy(np.stack([tgt] * F)))
        return fb
    # ONE batch serves both variants (its term is detached or not): a second FitBatch of a process gets another side stream, and some of
    # several batches of one process step 1.5-1.7x slower than the others whatever they compute (scripts/batchbook_rate.py)
    fb = batch(TV_WEIGHT)
    term = fb._tv

    def batch_off():
        fb._tv = None
        fb.step()

    def batch_on():
        fb._tv = term
        fb.step()
    variants += [("fitbatch16_off", batch_off), ("fitbatch16_on", batch_on)]
    for _, fn in variants:
        window(torch, fn, 20)
    ms = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            ms[name].append(window(torch, fn, a.iters))
    t = {k: min(v) for k, v in ms.items()}
    res["on_path"] = dict(windows_ms=ms, ms=t, spread={k: spread(v) for k, v in ms.items()}, step_delta_ms=t["step_on"] - t["step_off"],
                          fitbatch16_delta_ms=t["fitbatch16_on"] - t["fitbatch16_off"], tv_mean=e_on.tv(), tilings=e_on.tilings)
    # ---- the two launches alone: device events around 100 calls
    lib, p_ = L.lib(), L.ptr
    out = e_on.out; dout = torch.zeros_like(out)
    w = torch.full((1,), TV_WEIGHT, device="cuda"); acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    scratch = torch.empty(lib.mfvi_tv_term_scratch_bytes(1, out.shape[0], S, S), dtype=torch.uint8, device="cuda")
    calls = {}
    for name, tv in (("gradient_and_value", acc), ("gradient_only", None)):
        def call():
            L.check(lib.mfvi_tv_term(p_(out), 1, out.shape[0], out.shape[1], S, S, 0, 0.5, p_(w), 0, 1.0 / 16, 1, p_(dout), p_(tv), p_(scratch), L.stream_ptr()))
        us = []
        for _ in range(a.rounds + 1):                                    # the first round is the warm-up
            a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a_.record()
            for _ in range(100):
                call()
            b_.record(); torch.cuda.synchronize()
            us.append(a_.elapsed_time(b_) * 10.0)                        # ms per 100 calls -> us per call
        calls[name] = dict(us_per_call=min(us[1:]), rounds_us=us[1:])
    res["launches_alone"] = dict(shape=[int(v) for v in out.shape], **calls)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
