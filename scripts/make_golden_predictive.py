"""Writes tests/golden/predictive_gal.npz: fp32 sample stacks and the outputs of the reference's uncert_regression_gal
(BayTorch/inference/utils.py:11-24) on them, for reduction 'mean', 'sum' and anything else (the maps).

usage:  PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_predictive.py <reference checkout> [out.npz]

Two cases: C = 2 (one image channel + a variance channel, N = 25 draws at 24 x 28) and C = 4 (three colour channels + a variance
channel, N = 7 at 17 x 19: odd widths, so the kernels' scalar tail is exercised).  Keys per case <tag> in {c2, c4}:
  <tag>_x [N, C, H, W]  the draws (the last channel already a variance: positive)
  <tag>_mean / <tag>_sum  [ale, epi, uncert] as float64 (the Python floats of reduction 'mean' / 'sum')
  <tag>_ale, <tag>_epi, <tag>_uncert  [1, 1, H, W] fp32 maps (reduction 'none')."""
import os
import sys

import numpy as np

CASES = {"c2": (25, 2, 24, 28, 11), "c4": (7, 4, 17, 19, 12)}


def draws(N, C, H, W, seed):
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.0, 1.0, size=(1, C - 1, H, W))
    img = base + rng.normal(scale=0.05, size=(N, C - 1, H, W))                # per-draw spread around one image
    var = np.exp(-rng.normal(4.0, 1.0, size=(1, 1, H, W)) + rng.normal(scale=0.3, size=(N, 1, H, W)))
    return np.concatenate([img, var], axis=1).astype(np.float32)


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                               "predictive_gal.npz")
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    import torch
    from BayTorch.inference.utils import uncert_regression_gal
    res = {}
    for tag, (N, C, H, W, seed) in CASES.items():
        x = draws(N, C, H, W, seed)
        imgs = [torch.from_numpy(x[k:k + 1].copy()) for k in range(N)]
        res[tag + "_x"] = x
        for red in ("mean", "sum"):
            res["%s_%s" % (tag, red)] = np.array(uncert_regression_gal(imgs, red), np.float64)
        ale, epi, unc = uncert_regression_gal(imgs, "none")
        res[tag + "_ale"], res[tag + "_epi"], res[tag + "_uncert"] = (t.numpy().astype(np.float32) for t in (ale, epi, unc))
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
