"""What the per-iteration records of every fit cost a batch.

One process, the cfg2 shape of bench.py (256x256 denoising, input depth 16, the 26-layer skip net) with the tilings of
configs/bench_tilings.json, 16 fits with K = 1.  Every variant is warmed up, then timed in windows of at least 200 iterations that end in
a synchronise; the variants are alternated, twice; a variant's time is the minimum over its windows.  Measured, as ms per iteration:
  (a) step_untracked       FitBatch.step as it runs without a book
  (b) step_tracked         FitBatch.step with a BatchBook: mfvi_bookkeep_fits + 4 mfvi_pair_metrics calls beside the backward pass
  (c) step_plus_16_books   the untracked step followed by 16 sequential runner._Book.iteration calls on the fits' slices of the output
                           (9 launches per fit and iteration: the only way to the same records without BatchBook)
and, as ms per call,
  pair_metrics_16          one mfvi_pair_metrics call with want_ssim for 16 pairs of 256x256 maps (2 launches)
  ssim_sum_x16             16 mfvi_ssim_sum calls on the same pairs
Writes profiles/batchbook_rate.json with the times, every window, and the acceptance condition (b) <= (c).

usage: python scripts/batchbook_rate.py [--iters 200] [--out profiles/batchbook_rate.json]"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batchbook_rate.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from mfvi_dip_mia_amd import FitBatch, _lib as L
    from mfvi_dip_mia_amd.runner import _Book, phantom
    cfg = dict(bench.CONFIGS["cfg2"]); hp, S = cfg["hp"], cfg["size"]
    F, n_win = 16, max(200, a.iters)
    gt = phantom(S, S, hp["seed"])
    rng = np.random.default_rng(hp["seed"] + 1)
    tgt = np.clip(gt + rng.normal(scale=hp["p_sigma"], size=(S, S)), 0, 1).astype(np.float32)

    def batch():
        fb = FitBatch(S, S, F, task="den", K=1, input_depth=cfg["input_depth"], temp=[hp["temp"] * 2 ** (f % 4) for f in range(F)], sigma=hp["sigma"],
                      lr=hp["lr"], seed=hp["seed"], autotune=False)
        fb.plan.set_fits(0)                                   # tilings are set with the mode off
        fb.tilings = bench.pin_tilings(fb.plan, 16)
        fb.plan.set_fits(1, fb.stride, fb.stride)
        fb.set_targets(torch.from_numpy(np.stack([tgt] * F)))
        return fb

    # ONE batch serves the three variants (its book is attached or not): a second FitBatch of a process gets another side stream, and in the
    # measured process some of several batches (the 2nd and the 5th created) stepped 1.5-1.7x slower than the others, tracked or not
    fb = batch()
    book = fb.track(gt, n_win, noisy=tgt)
    books = [_Book(types.SimpleNamespace(H=S, W=S, out=fb.out[f:f + 1]), n_win, gt, tgt, task="den") for f in range(F)]
    engs = [types.SimpleNamespace(out=fb.out[f:f + 1]) for f in range(F)]
    count = [0]

    def step_untracked():
        fb._book = None
        fb.step()

    def step_tracked():
        fb._book = book
        if book.i == book.num_iter:      # a window holds n_win iterations: start the curves over
            book.i = 0
        fb.step()

    def step_plus_books():
        fb._book = None
        fb.step()
        i = count[0] % n_win
        for f in range(F):
            books[f].iteration(engs[f], i, 1)
        count[0] += 1

    x = torch.from_numpy(np.stack([gt] * F)).cuda(); y = torch.from_numpy(np.stack([tgt] * F)).cuda()
    lib, p_ = L.lib(), L.ptr
    scratch = torch.empty(lib.mfvi_pair_metrics_scratch_bytes(F, S, S), dtype=torch.uint8, device="cuda")
    sums = torch.zeros((F, 2), dtype=torch.float64, device="cuda"); single = torch.zeros(F, dtype=torch.float64, device="cuda")

    def pair_metrics_16():
        L.check(lib.mfvi_pair_metrics(p_(x), S * S, p_(y), S * S, F, S, S, 1, p_(scratch), p_(sums), 2, L.stream_ptr()))

    def ssim_sum_x16():
        sp = L.stream_ptr()
        for f in range(F):
            L.check(lib.mfvi_ssim_sum(p_(x[f]), p_(y[f]), S, S, p_(single[f:]), sp))

    variants = [("step_untracked", step_untracked), ("step_tracked", step_tracked), ("step_plus_16_books", step_plus_books),
                ("pair_metrics_16", pair_metrics_16), ("ssim_sum_x16", ssim_sum_x16)]

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
            ms[name].append(window(fn, n_win))
    t = {name: min(v) for name, v in ms.items()}
    ssim_diff = float(np.abs(sums[:, 1].cpu().numpy() - single.cpu().numpy()).max() / (S * S))
    res = dict(config="cfg2", size=S, fits=F, K=1, iterations_per_window=n_win, tilings=fb.tilings, ms=t, windows_ms=ms,
               bookkeeping_ms=dict(tracked=t["step_tracked"] - t["step_untracked"], sixteen_books=t["step_plus_16_books"] - t["step_untracked"]),
               ssim_mean_max_abs_diff_pair_vs_single=ssim_diff,
               acceptance=dict(bound="step_tracked <= step_plus_16_books", lhs_ms=t["step_tracked"], rhs_ms=t["step_plus_16_books"],
                               met=bool(t["step_tracked"] <= t["step_plus_16_books"])),
               dead=[int(v) for v in fb.dead])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
