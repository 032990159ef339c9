"""What an iteration of 16 DIP / MC-dropout / SGLD fits costs, one SiblingBatch against one SiblingEngine per fit.

One process, one GPU, everything at 256 x 256, K = 1, denoising -- the shape of the reference's candidate sweeps.  Every variant is warmed,
then timed in windows that end in a device synchronise, the variants alternating, two windows per variant, each at least 0.2 s.  Reported
per variant: the minimum of its two windows and the spread between them (|a - b| / min) -- the yardstick a difference is read against.

Per method: ms per SiblingBatch.step() of F = 16 fits ("batch") against 16 sequential SiblingEngine(K=1).step() calls, timed two ways: ONE
engine stepped 16 times ("one_engine": the reference's use, a candidate's whole fit before the next starts) and 16 engines stepped in turn
("round_robin").  `sequential_ms` is the smaller of the two.  Every plan is autotuned on this device (the tilings of one launch size are
searched once and shared through a cache file in a temporary directory).  Each method is measured in a fresh process of its own.

The sequential figure belongs to the code before the batch existed: `--part sequential --root <checkout of the parent commit, built>`
measures it there (that checkout has no SiblingBatch) and writes a JSON that `--part batch --sequential-from <that JSON>` folds into the
result; `--part both` (the default) measures both in this build.  Fixes no ratio in advance.  Writes profiles/sibling_batch_rate.json.

usage: python scripts/siblingbatch_rate.py [--part both|batch|sequential] [--root DIR] [--sequential-from JSON] [--methods dip,mcd,sgld] [--out JSON]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

S, K, F = 256, 1, 16
HYPER = dict(dip=dict(lr=1e-3), mcd=dict(lr=1e-3, dropout_p=0.3, weight_decay=3e-4), sgld=dict(lr=1e-3, gamma=0.996, weight_decay=5e-8))      # the runners' defaults


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("both", "batch", "sequential"), default="both")
    ap.add_argument("--root", default=ROOT, help="the checkout to import the package from (a built checkout of the parent commit for --part sequential)")
    ap.add_argument("--sequential-from", default=None, help="JSON written by a --part sequential run: its figures become the sequential side")
    ap.add_argument("--methods", default="dip,mcd,sgld")
    ap.add_argument("--window", type=float, default=0.25, help="seconds a timed window aims at (at least 0.2 is enforced)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sibling_batch_rate.json"))
    a = ap.parse_args()
    methods = a.methods.split(",")
    if len(methods) > 1:
        # one fresh process per method: in one process the engines of the second and third method ran 3.5 - 4.3 x slower than those of the
        # first, whichever method came first (measured; not explained), so each method is measured the way the first one is
        import subprocess
        res = None
        for m in methods:
            with tempfile.TemporaryDirectory() as d:
                out = os.path.join(d, "%s.json" % m)
                cmd = [sys.executable, os.path.abspath(__file__), "--part", a.part, "--root", a.root, "--methods", m, "--window", str(a.window), "--out", out]
                subprocess.run(cmd + (["--sequential-from", a.sequential_from] if a.sequential_from else []), check=True)
                one = json.load(open(out))
            if res is None:
                res = one
            else:
                res["methods"] += one["methods"]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)
        return
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    import mfvi_dip_mia_amd as M
    from mfvi_dip_mia_amd.engine import SiblingEngine
    from mfvi_dip_mia_amd.runner import phantom
    if not torch.cuda.is_available():
        sys.exit("siblingbatch_rate.py measures on the GPU; there is none")
    M._lib.lib()
    want = max(a.window, 0.2)

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

    res = dict(device=torch.cuda.get_device_name(0), S=S, K=K, F=F, task="den", window_s=want, part=a.part, root=os.path.basename(os.path.abspath(a.root)))
    seq_from = json.load(open(a.sequential_from)) if a.sequential_from else None
    tune_dir = tempfile.mkdtemp(prefix="siblingbatch_tune_")

    def cache(method, n):      # the tilings of a method's launches of n samples: searched by the first plan that needs them, read by the others
        os.environ["MFVI_TUNE_CACHE"] = os.path.join(tune_dir, "%s_n%d.json" % (method, n))

    rng = np.random.default_rng(1)
    gt = np.stack([phantom(S, S, 42 + f) for f in range(F)])
    noisy = np.clip(gt + rng.normal(scale=0.1, size=gt.shape), 0, 1).astype(np.float32)
    rows = []
    for method in methods:
        h = HYPER[method]
        calls = {}
        engines = batch = None
        if a.part in ("both", "sequential"):
            cache(method, K)      # (engines[0], the one `one_engine` steps, searches its tilings itself for every method)
            engines = [SiblingEngine(S, S, method=method, task="den", K=K, input_depth=16, seed=42 + f, autotune=True, **h) for f in range(F)]
            for f, e in enumerate(engines):
                e.set_target(torch.from_numpy(noisy[f]))

            def round_robin(engines=engines):
                for e in engines:
                    e.step()

            def one_engine(e=engines[0]):
                for _ in range(F):
                    e.step()
            calls.update(one_engine=one_engine, round_robin=round_robin)
        if a.part in ("both", "batch"):
            cache(method, F * K)
            batch = M.SiblingBatch(S, S, F, method, task="den", K=K, input_depth=16, seed=42, autotune=True, **h)
            batch.set_targets(torch.from_numpy(noisy))
            calls["batch"] = batch.step
        r = alternate(calls, 5)
        row = dict(method=method, detail=r, spread=max(v["spread"] for v in r.values()))
        if batch is not None:
            assert not batch.dead.any() and np.isfinite(batch.losses()).all()
            row["batch_ms"] = r["batch"]["per_call_s"] * 1e3
        if engines is not None:
            assert all(np.isfinite(e.losses()[0]) for e in engines)
            row.update(one_engine_ms=r["one_engine"]["per_call_s"] * 1e3, round_robin_ms=r["round_robin"]["per_call_s"] * 1e3)
            row["sequential_ms"] = min(row["one_engine_ms"], row["round_robin_ms"]); row["sequential_build"] = res["root"]
        elif seq_from is not None:
            prev = next(x for x in seq_from["methods"] if x["method"] == method)
            row.update(one_engine_ms=prev["one_engine_ms"], round_robin_ms=prev["round_robin_ms"], sequential_ms=prev["sequential_ms"],
                       sequential_build=seq_from.get("root"), spread=max(row["spread"], prev["spread"]), sequential_detail=prev["detail"])
        if "batch_ms" in row and "sequential_ms" in row:
            row["sequential_over_batch"] = row["sequential_ms"] / row["batch_ms"]
            row["faster_beyond_spread"] = bool(row["sequential_ms"] - row["batch_ms"] > row["spread"] * row["sequential_ms"])
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if "detail" not in k}), flush=True)
        del engines, batch, calls
        torch.cuda.empty_cache()
    res["methods"] = rows
    os.environ.pop("MFVI_TUNE_CACHE", None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
