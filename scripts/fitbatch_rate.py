"""Fit-iterations per second of batched independent fits against sequential single fits.

One process, the cfg2 shape of bench.py (256x256 denoising, input depth 16, the 26-layer skip net) with the tilings of
configs/bench_tilings.json on every plan.  Every variant is warmed up, then timed in windows of at least 200 iterations that end in a
synchronise; the variants are alternated, twice.  Measured, as ms per iteration (the minimum over the windows of a variant):
  ElboEngine K = 1 (one fit as it runs today), ElboEngine K = 16, 16 sequential mfvi_elbo_update calls and one,
  FitBatch F = 4, 8, 16 with K = 1.
Writes profiles/fitbatch_rate_cfg2.json: the times, fit-iterations per second, the gain F t(K=1) / t_batch(F), and the acceptance bound
  t_batch(16) <= 1.15 (t(K=16) + 16 t_upd - t_upd),
both sides measured in this run.

usage: python scripts/fitbatch_rate.py [--iters 200] [--out profiles/fitbatch_rate_cfg2.json] [--only F]   (--only: a kernel trace of one batch size)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fitbatch_rate_cfg2.json"))
    ap.add_argument("--only", type=int, default=0, help="run --iters iterations of FitBatch(F, K = 1) and nothing else (for rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from mfvi_dip_mia_amd import FitBatch, _lib as L
    from mfvi_dip_mia_amd.runner import phantom
    cfg = dict(bench.CONFIGS["cfg2"]); hp, S = cfg["hp"], cfg["size"]
    rng = np.random.default_rng(hp["seed"] + 1)
    tgt = np.clip(phantom(S, S, hp["seed"]) + rng.normal(scale=hp["p_sigma"], size=(S, S)), 0, 1).astype(np.float32)

    def batch(F):
        fb = FitBatch(S, S, F, task="den", K=1, input_depth=cfg["input_depth"], temp=[hp["temp"] * 2 ** (f % 4) for f in range(F)], sigma=hp["sigma"],
                      lr=hp["lr"], seed=hp["seed"], autotune=False)
        fb.plan.set_fits(0)                                   # tilings are set with the mode off (in-kernel-eps ones fall back when it goes on)
        fb.tilings = bench.pin_tilings(fb.plan, 16)           # the table's entry for launches of 16 samples, whatever F is
        fb.plan.set_fits(1, fb.stride, fb.stride)
        fb.set_targets(torch.from_numpy(np.stack([tgt] * F)))
        return fb

    if a.only:
        fb = batch(a.only)
        for _ in range(a.iters):
            fb.step()
        torch.cuda.synchronize()
        print(json.dumps(dict(config="cfg2", only=a.only, iterations=a.iters, tilings=fb.tilings)))
        return
    engines = {K: bench.make_engine(cfg, K, 0, 1, torch) for K in (1, 16)}
    batches = {F: batch(F) for F in (4, 8, 16)}
    e1 = engines[1]
    lib, p_ = L.lib(), L.ptr

    def upd(n):
        def run():
            sp = L.stream_ptr()
            for _ in range(n):      # on the K = 1 engine's own state with zero gradients and lr 0: the traffic of an update, no drift
                L.check(lib.mfvi_elbo_update(p_(e1.params), p_(upd.g), p_(upd.m), p_(upd.v), e1.n_vi, e1.n_bn, 0.0, e1.prior_sigma, 0.0, 0.0, 0.9, 0.999,
                                             1e-8, 1, p_(upd.kl), p_(e1.upd_scratch), sp))
        return run
    upd.g = torch.zeros(e1.n_params, device="cuda"); upd.m = torch.zeros_like(upd.g); upd.v = torch.zeros_like(upd.g)
    upd.kl = torch.zeros(1, dtype=torch.float64, device="cuda")
    variants = [("engine_k1", engines[1].step), ("engine_k16", engines[16].step), ("update_x1", upd(1)), ("update_x16", upd(16))]
    variants += [("batch_f%d" % F, batches[F].step) for F in (4, 8, 16)]

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for _, fn in variants:      # warm every shape: tables uploaded, side streams created, allocator pools filled, clocks up
        window(fn, 20)
    ms = {name: [] for name, _ in variants}
    for _ in range(2):
        for name, fn in variants:
            ms[name].append(window(fn, max(200, a.iters)))
    t = {name: min(v) for name, v in ms.items()}
    res = dict(config="cfg2", size=S, iterations_per_window=max(200, a.iters), tilings={"engine": engines[1].tilings, "batch": batches[16].tilings},
               ms_per_iteration=t, windows_ms=ms)
    res["fit_iterations_per_s"] = dict(engine_k1=1e3 / t["engine_k1"], **{"batch_f%d" % F: F * 1e3 / t["batch_f%d" % F] for F in (4, 8, 16)})
    res["gain"] = {"f%d" % F: F * t["engine_k1"] / t["batch_f%d" % F] for F in (4, 8, 16)}
    rhs = 1.15 * (t["engine_k16"] + t["update_x16"] - t["update_x1"])
    res["acceptance"] = dict(bound="t_batch(16) <= 1.15 * (t(K=16) + t_upd x 16 - t_upd x 1)", lhs_ms=t["batch_f16"], rhs_ms=rhs, met=bool(t["batch_f16"] <= rhs))
    res["dead"] = {"f%d" % F: [int(x) for x in batches[F].dead] for F in (4, 8, 16)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
