"""What a CT volume costs per iteration, one CtVolume against one ElboEngine per slice.

One process, one GPU, everything at 256 x 256 with 45 angles and K = 1, the CT runner's shape.  Every variant is warmed, then timed in windows
that end in a device synchronise, old and new alternating, two windows per variant, each at least 0.2 s.  Reported per variant: the minimum
of its two windows and the spread between them (|a - b| / min) -- the yardstick a difference between old and new is read against.

  (a) the data term alone: mfvi_radon_mse_fits for F = 1, 4, 16 fits ("new") against F calls of mfvi_radon_mse, one per fit ("old", the
      path of ElboEngine(task="ct")), on the same seeded outputs and sinograms; dout and the per-fit mse of the two must agree (4e-5 / 1e-5).
  (b) the whole iteration: ms per CtVolume.step() for D = F = 1, 4, 8, 16 slices and for D = 32 in groups of F = 16 ("new") against D
      sequential ElboEngine(task="ct", K=1).step() calls ("old"), timed two ways: ONE engine stepped D times ("one_engine": the reference's
      use, a slice's whole fit before the next slice starts, so its buffers stay warm in the caches) and D engines, one per slice, stepped
      in turn ("round_robin": what advancing a stack in lockstep costs without the volume).  `old_ms` is the smaller of the two.  Every plan
      is autotuned on this device (the tilings of one launch size are searched once and shared through a cache file in a temporary
      directory).

Fixes no ratio in advance.  The one condition it records: the F = 16 volume takes less time than 16 sequential engine iterations -- the
cheaper way of running them -- by more than the largest of the spreads (`f16_faster_beyond_spread`).  Writes profiles/ctvolume_rate.json.

usage: python scripts/ctvolume_rate.py [--only a|b] [--window 0.25] [--out profiles/ctvolume_rate.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, T, K = 256, 45, 1
DATA_TERM_F = (1, 4, 16)
VOLUMES = ((1, 1), (4, 4), (8, 8), (16, 16), (32, 16))                          # (D slices, F per launch set)
HYPER = dict(temp=4e-6, sigma=0.01, lr=3e-4, seed=42, input_depth=16)           # run_ct_mfvi's defaults


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("a", "b"), default=None)
    ap.add_argument("--window", type=float, default=0.25, help="seconds a timed window aims at (at least 0.2 is enforced)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctvolume_rate.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import mfvi_dip_mia_amd as M
    from mfvi_dip_mia_amd import _lib as L
    from mfvi_dip_mia_amd.engine import ElboEngine
    from mfvi_dip_mia_amd.runner import phantom
    if not torch.cuda.is_available():
        sys.exit("ctvolume_rate.py measures on the GPU; there is none")
    lib = L.lib()
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

    res = dict(device=torch.cuda.get_device_name(0), S=S, T=T, K=K, window_s=want, only=a.only)
    theta = torch.arange(0, 180, 4, dtype=torch.float32).cuda()
    st = L.stream_ptr()

    if a.only in (None, "a"):
        rows = []
        for F in DATA_TERM_F:
            g = torch.Generator(device="cpu").manual_seed(2000 + F)
            out = torch.rand((F, 1, S, S), generator=g).cuda()
            sinos = (60.0 * torch.rand((F, T, S), generator=g)).cuda()
            dn, do = torch.empty_like(out), torch.empty_like(out)
            mn, mo = torch.zeros(F, dtype=torch.float64, device="cuda"), torch.zeros(F, dtype=torch.float64, device="cuda")
            sn = torch.empty(lib.mfvi_radon_mse_fits_scratch_bytes(F, K, S, T), dtype=torch.uint8, device="cuda")
            so = torch.empty((F, T * S), device="cuda")
            p_out, p_sin, p_th, p_sn, p_dn, p_mn = L.ptr(out), L.ptr(sinos), L.ptr(theta), L.ptr(sn), L.ptr(dn), L.ptr(mn)
            per_fit = [(L.ptr(out[f]), L.ptr(sinos[f]), L.ptr(so[f]), L.ptr(do[f]), L.ptr(mo[f:])) for f in range(F)]

            def new():
                L.check(lib.mfvi_radon_mse_fits(p_out, p_sin, T * S, p_th, F, K, S, T, 1.0, p_sn, p_dn, p_mn, st))

            def old():
                for o, s, sc, d, m in per_fit:
                    L.check(lib.mfvi_radon_mse(o, s, p_th, 1, S, S, T, 1.0, sc, d, m, st))
            new(); old()
            torch.cuda.synchronize()
            row = dict(F=F, relerr_dout=float((dn - do).abs().max() / do.abs().max()), relerr_mse=float(((mn - mo).abs() / mo.abs()).max()))
            assert row["relerr_dout"] < 4e-5 and row["relerr_mse"] < 1e-5, row      # faster and different is not faster
            r = alternate(dict(old=old, new=new), 20)
            row.update(old_us=r["old"]["per_call_s"] * 1e6, new_us=r["new"]["per_call_s"] * 1e6, old_over_new=r["old"]["per_call_s"] / r["new"]["per_call_s"],
                       spread=max(r["old"]["spread"], r["new"]["spread"]), detail=r)
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "detail"}))
        res["data_term"] = rows

    if a.only in (None, "b"):
        tune_dir = tempfile.mkdtemp(prefix="ctvolume_tune_")

        def cache(n):      # the tilings of a launch of n samples, searched once
            os.environ["MFVI_TUNE_CACHE"] = os.path.join(tune_dir, "n%d.json" % n)

        Dmax = max(d for d, _ in VOLUMES)
        gt = np.stack([phantom(S, S, HYPER["seed"] + d) for d in range(Dmax)])
        cache(1)
        engines = [ElboEngine(S, S, task="ct", K=K, input_depth=HYPER["input_depth"], temp=HYPER["temp"], sigma=HYPER["sigma"], lr=HYPER["lr"],
                              seed=HYPER["seed"] + d, autotune=True) for d in range(Dmax)]
        rows = []
        for D, F in VOLUMES:
            cache(F * K)
            vol = M.CtVolume(S, D, slices_per_launch=F, K=K, input_depth=HYPER["input_depth"], temp=HYPER["temp"], sigma=HYPER["sigma"], lr=HYPER["lr"],
                             seed=HYPER["seed"], autotune=True)
            vol.set_volume(torch.from_numpy(gt[:D]))
            for d in range(D):
                engines[d].set_target(vol.sinos[d].clone())
            used = engines[:D]

            def round_robin():
                for e in used:
                    e.step()

            def one_engine(e=engines[0], D=D):
                for _ in range(D):
                    e.step()
            r = alternate(dict(one_engine=one_engine, round_robin=round_robin, new=vol.step), 5)
            assert not vol.dead.any() and all(np.isfinite(e.losses()[2]) for e in used)
            old_s = min(r["one_engine"]["per_call_s"], r["round_robin"]["per_call_s"])
            row = dict(D=D, F=F, groups=len(vol.groups), old_one_engine_ms=r["one_engine"]["per_call_s"] * 1e3,
                       old_round_robin_ms=r["round_robin"]["per_call_s"] * 1e3, old_ms=old_s * 1e3, new_ms=r["new"]["per_call_s"] * 1e3,
                       old_over_new=old_s / r["new"]["per_call_s"], spread=max(v["spread"] for v in r.values()),
                       new_ms_per_slice=r["new"]["per_call_s"] * 1e3 / D, old_ms_per_slice=old_s * 1e3 / D, detail=r)
            row["faster_beyond_spread"] = bool(row["old_ms"] - row["new_ms"] > row["spread"] * row["old_ms"])
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "detail"}))
            del vol
            torch.cuda.empty_cache()
        res["iteration"] = rows
        res["f16_faster_beyond_spread"] = next(r["faster_beyond_spread"] for r in rows if (r["D"], r["F"]) == (16, 16))
        os.environ.pop("MFVI_TUNE_CACHE", None)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
