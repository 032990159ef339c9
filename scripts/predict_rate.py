"""Posterior predictive sampling rate against the forward-only MC rate of the same engine.

At cfg2 of bench.py (256x256 denoising, the 26-layer skip net, bench tilings, launches of 16) one process times, warmed and alternating,
  A: 64 x ElboEngine.forward_only()  = 1024 MC forward passes on the training plan (the "MC forward passes/s" leg of the metric)
  B: ElboEngine.predict(1024)        = 64 launches of 16 on the prediction plan + 64 accumulate launches + finalize
with HIP events on the stream.  The prediction plan gets the training plan's tilings, so both run the same convolution kernels and the
difference is the reduction.  Prints one JSON line.

usage: python scripts/predict_rate.py [--n 1024] [--reps 5] [--predict-only]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--predict-only", action="store_true", help="run predict(n) twice and nothing else (for a kernel trace)")
    a = ap.parse_args()
    import torch
    import bench
    cfg = dict(bench.CONFIGS["cfg2"])
    eng = bench.make_engine(cfg, cfg["k"], 0, 1, torch)
    plan, _ = eng._pred_plan(eng.chunk)
    tilings = bench.pin_tilings(plan, eng.chunk)            # the bench tilings of the training plan on the prediction plan too
    calls = a.n // eng.K_local
    if a.predict_only:
        for _ in range(2):
            eng.predict(a.n)
        torch.cuda.synchronize()
        print(json.dumps(dict(config="cfg2", predict_only=True, n_samples=a.n, runs=2, chunk=eng.chunk)))
        return

    def run_fwd():
        for i in range(calls):
            eng.forward_only(step=1000 + i)

    def run_pred():
        eng.predict(a.n)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    run_fwd(); run_pred(); torch.cuda.synchronize()          # warm: tables uploaded, allocator pools filled
    fwd_ms, pred_ms = [], []
    for _ in range(a.reps):
        fwd_ms.append(timed(run_fwd))
        pred_ms.append(timed(run_pred))
    # the reduction alone: the same 64 accumulate launches + finalize on the outputs of one launch
    from mfvi_dip_mia_amd.predictive import Accumulator
    out = eng.forward_only(step=7)

    def run_red():
        acc = Accumulator(out.shape[1], eng.H, eng.W, "logprec")
        for _ in range(calls):
            acc.add(out, eng.chunk)
        acc.finalize(a.n)
    run_red()
    red_ms = sorted(timed(run_red) for _ in range(a.reps))[a.reps // 2]
    f, p = sorted(fwd_ms)[a.reps // 2], sorted(pred_ms)[a.reps // 2]
    rec = dict(config="cfg2", n_samples=a.n, chunk=eng.chunk, reps=a.reps, tilings=[eng.tilings, tilings], forward_only_ms=f, predict_ms=p,
               forward_only_passes_per_s=a.n / f * 1e3, predict_passes_per_s=a.n / p * 1e3, ratio=f / p,
               reduction_only_ms=red_ms, reduction_share_of_predict=red_ms / p, fwd_ms_all=fwd_ms, predict_ms_all=pred_ms,
               device=torch.cuda.get_device_name(0))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
