"""What the anti-aliased super-resolution data term costs per iteration.

One process, one GPU, the cfg3 shape of bench.py (512x512 4x super-resolution, input depth 32, the tilings of configs/bench_tilings.json on
every plan) at K = 8 (one GPU's share, what bench.py times) and K = 32 (the whole job).  Per K two engines that differ in the data term
alone — downsampler="nearest" (mfvi_gaussian_nll with factor 4, the path bench.py measures) and downsampler="lanczos2"
(mfvi_gaussian_nll_filtered) — and a device-to-device copy of `out`.  Everything is warmed up, then timed in windows that end in a
synchronise, the variants alternated, twice; the minimum over a variant's windows is reported, as ms per iteration / per call:
  iteration_ms {nearest, lanczos2}, data_term_ms {nearest, lanczos2} (the loss launches alone, on the engine's own buffers), copy_out_ms.
Acceptance: iteration_ms[lanczos2] - iteration_ms[nearest] <= 2 copy_out_ms (the data term must read out and write dout once each; the
second factor covers the halo re-reads and the low-resolution scratch pass).
Writes profiles/sr_downsampler_cfg3.json.

usage: python scripts/sr_downsampler_rate.py [--iters 100] [--k 8,32] [--out profiles/sr_downsampler_cfg3.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--k", default="8,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sr_downsampler_cfg3.json"))
    a = ap.parse_args()
    import torch
    import bench
    from mfvi_dip_mia_amd.downsampler import downsample
    from mfvi_dip_mia_amd.engine import ElboEngine
    from mfvi_dip_mia_amd.runner import phantom
    if not torch.cuda.is_available():
        sys.exit("sr_downsampler_rate.py measures on the GPU; there is none")
    cfg = dict(bench.CONFIGS["cfg3"]); hp, S = cfg["hp"], cfg["size"]
    img = torch.from_numpy(phantom(S, S, hp["seed"])).cuda()

    def engine(K, kind):
        eng = ElboEngine(S, S, task="sr", K=K, input_depth=cfg["input_depth"], temp=hp["temp"], sigma=hp["sigma"], lr=hp["lr"], seed=hp["seed"],
                         autotune=False, sr_factor=4, downsampler=kind)
        eng.tilings = bench.pin_tilings(eng.plan, eng.chunk)
        eng.set_target(img[::4, ::4].contiguous() if kind == "nearest" else downsample(img, kind, 4))
        return eng

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    res = dict(config="cfg3", size=S, factor=4, iterations_per_window=a.iters, per_k={})
    for K in (int(k) for k in a.k.split(",")):
        engs = {kind: engine(K, kind) for kind in ("nearest", "lanczos2")}
        dst = torch.empty_like(engs["nearest"].out)
        variants = [("iteration_" + kind, e.step, a.iters) for kind, e in engs.items()]
        variants += [("data_term_" + kind, (lambda e=e: e._loss_and_dout(e.chunk)), 4 * a.iters) for kind, e in engs.items()]
        variants += [("copy_out", lambda: dst.copy_(engs["nearest"].out), 4 * a.iters)]
        for _, fn, _ in variants:      # warm every shape: tables uploaded, side streams created, clocks up
            window(fn, 10)
        ms = {name: [] for name, _, _ in variants}
        for _ in range(2):
            for name, fn, n in variants:
                ms[name].append(window(fn, n))
        t = {name: min(v) for name, v in ms.items()}
        added = t["iteration_lanczos2"] - t["iteration_nearest"]
        res["per_k"][str(K)] = dict(
            out_bytes=engs["nearest"].out.numel() * 4, tilings=engs["nearest"].tilings,
            iteration_ms=dict(nearest=t["iteration_nearest"], lanczos2=t["iteration_lanczos2"]),
            data_term_ms=dict(nearest=t["data_term_nearest"], lanczos2=t["data_term_lanczos2"]), copy_out_ms=t["copy_out"], windows_ms=ms,
            nll={kind: e.losses()[0] for kind, e in engs.items()},
            acceptance=dict(bound="iteration_ms[lanczos2] - iteration_ms[nearest] <= 2 * copy_out_ms", added_ms=added, rhs_ms=2 * t["copy_out"],
                            met=bool(added <= 2 * t["copy_out"])))
        del engs, dst
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
