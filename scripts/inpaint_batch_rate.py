"""What F inpainting fits cost per iteration, one InpaintBatch against one ElboEngine(task="inp") per fit.

One process, one GPU, K = 1, the inpainting runner's defaults (input depth 32, lr 2e-3), autotuned plans, at two sizes: 256 x 256 (every
map of the pyramid a multiple of 4 wide: all matrix-core) and H x W = 256 x 320 (the reference's 320 x 256 images: the two deepest levels,
10 and 5 wide, run on the generic fp32 kernels).  Every variant is warmed, then timed in windows that end in a device synchronise, old and
new alternating, two windows per variant, each at least 0.2 s.  Reported per variant: the minimum of its two windows and the spread between
them (|a - b| / min) -- the yardstick a difference between old and new is read against.

Per size and F in 1, 4, 8, 16: ms per InpaintBatch.step() ("new") against F sequential ElboEngine(task="inp", K=1).step() calls ("old"),
timed two ways: ONE engine stepped F times ("one_engine": the reference's use, a fit's whole run before the next starts, so its buffers
stay warm in the caches) and F engines, one per fit, stepped in turn ("round_robin").  `old_ms` is the smaller of the two.  The tilings of one
launch size are searched once per size and shared through a cache file in a temporary directory.

Fixes no ratio in advance.  The one condition it records, per size: the F = 16 batch takes less time than 16 sequential engine iterations --
the cheaper way of running them -- by more than the largest of the spreads (`f16_faster_beyond_spread`).  Writes
profiles/inpaint_batch_rate.json.

usage: python scripts/inpaint_batch_rate.py [--only 256x256|256x320] [--fits 1,4,8,16] [--window 0.25] [--out profiles/inpaint_batch_rate.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 1
SIZES = {"256x256": (256, 256), "256x320": (256, 320)}                          # H x W
FITS = (1, 4, 8, 16)
HYPER = dict(temp=4e-6, sigma=0.01, lr=2e-3, seed=42, input_depth=32)           # run_inp_mfvi's defaults


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=tuple(SIZES), default=None)
    ap.add_argument("--fits", default=",".join(str(f) for f in FITS))
    ap.add_argument("--window", type=float, default=0.25, help="seconds a timed window aims at (at least 0.2 is enforced)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inpaint_batch_rate.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import mfvi_dip_mia_amd as M
    from mfvi_dip_mia_amd.engine import ElboEngine
    from mfvi_dip_mia_amd.runner import phantom, scratch_mask
    if not torch.cuda.is_available():
        sys.exit("inpaint_batch_rate.py measures on the GPU; there is none")
    M._lib.lib()
    want = max(a.window, 0.2)
    fits = tuple(int(f) for f in a.fits.split(","))

    def window(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def timed(fn, iters):
        """One window of at least 0.2 s: (seconds per call, iterations used)."""
        while True:
            dt = window(fn, iters)
            if dt >= 0.2:
                return dt / iters, iters
            iters = int(iters * max(2.0, 0.3 / max(dt, 1e-6))) + 1

    def alternate(calls, warm):
        """calls: {variant: fn} -> per variant dict(per_call_s, windows_s, spread, calls_per_window); the variants in turn, twice."""
        iters = {}
        for key, fn in calls.items():
            window(fn, warm)
            per = window(fn, warm) / warm
            iters[key] = max(warm, int(want * 1.15 / per) + 1)
        secs = {key: [] for key in calls}
        for _ in range(2):
            for key, fn in calls.items():
                per, iters[key] = timed(fn, iters[key])
                secs[key].append(per)
        return {key: dict(per_call_s=min(w), windows_s=w, spread=abs(w[0] - w[1]) / min(w), calls_per_window=iters[key]) for key, w in secs.items()}

    res = dict(device=torch.cuda.get_device_name(0), K=K, window_s=want, only=a.only, hyper=HYPER, sizes={})
    tune_dir = tempfile.mkdtemp(prefix="inpaint_tune_")
    for name, (H, W) in SIZES.items():
        if a.only not in (None, name):
            continue

        def cache(n, name=name):      # the tilings of a launch of n samples at this size, searched once
            os.environ["MFVI_TUNE_CACHE"] = os.path.join(tune_dir, "%s_n%d.json" % (name, n))

        Fmax = max(fits)
        gt = np.stack([np.stack([phantom(H, W, HYPER["seed"] + 3 * f + c) for c in range(3)]) for f in range(Fmax)]).astype(np.float32)
        mask = scratch_mask(H, W, HYPER["seed"])
        cache(1)
        engines = [ElboEngine(H, W, task="inp", K=K, input_depth=HYPER["input_depth"], temp=HYPER["temp"], sigma=HYPER["sigma"], lr=HYPER["lr"],
                              seed=HYPER["seed"] + f, autotune=True) for f in range(Fmax)]
        for f, e in enumerate(engines):
            e.set_target(torch.from_numpy(gt[f]), torch.from_numpy(mask))
        rows = []
        for F in fits:
            cache(F * K)
            ib = M.InpaintBatch(H, W, F, K=K, input_depth=HYPER["input_depth"], temp=HYPER["temp"], sigma=HYPER["sigma"], lr=HYPER["lr"], seed=HYPER["seed"],
                                autotune=True)
            ib.set_targets(torch.from_numpy(gt[:F]), torch.from_numpy(mask))
            used = engines[:F]

            def round_robin(used=used):
                for e in used:
                    e.step()

            def one_engine(e=engines[0], F=F):
                for _ in range(F):
                    e.step()
            r = alternate(dict(one_engine=one_engine, round_robin=round_robin, new=ib.step), 5)
            assert not ib.dead.any() and all(np.isfinite(e.losses()[2]) for e in used)
            old_s = min(r["one_engine"]["per_call_s"], r["round_robin"]["per_call_s"])
            lib = M._lib.lib()
            generic = [i for i, o in enumerate(ib.prog.ops) if o["type"] == M._lib.OP_CONV and lib.mfvi_plan_last_kernel(ib.plan.handle, i, 0) == 0]      # forward
            row = dict(F=F, old_one_engine_ms=r["one_engine"]["per_call_s"] * 1e3, old_round_robin_ms=r["round_robin"]["per_call_s"] * 1e3,
                       old_ms=old_s * 1e3, new_ms=r["new"]["per_call_s"] * 1e3, old_over_new=old_s / r["new"]["per_call_s"],
                       spread=max(v["spread"] for v in r.values()), new_ms_per_fit=r["new"]["per_call_s"] * 1e3 / F, old_ms_per_fit=old_s * 1e3 / F,
                       ops_on_generic_kernels=generic, detail=r)
            row["faster_beyond_spread"] = bool(row["old_ms"] - row["new_ms"] > row["spread"] * row["old_ms"])
            rows.append(row)
            print(name, json.dumps({k: v for k, v in row.items() if k != "detail"}))
            del ib
            torch.cuda.empty_cache()
        entry = dict(H=H, W=W, iteration=rows)
        f16 = [r for r in rows if r["F"] == 16]
        if f16:
            entry["f16_faster_beyond_spread"] = f16[0]["faster_beyond_spread"]
        res["sizes"][name] = entry
        del engines
        torch.cuda.empty_cache()
    os.environ.pop("MFVI_TUNE_CACHE", None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
