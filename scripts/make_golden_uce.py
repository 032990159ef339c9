"""Writes tests/golden/uce.npz: error / uncertainty maps and the outputs of the reference's uceloss (utils/uce.py:9-40) on them, for
outlier 0 and 1e-4, beside a float64 numpy restatement (tests/uce_restatement.py) and the reference's own deviation from it.

usage:  PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_uce.py <reference checkout> [out.npz]

Inputs (seeded numpy): unc = exp(N(-5, 0.6)), err = unc * chi^2_1 * factor -- an uncertainty map spread over a decade and a squared error
whose expectation is factor times it.  Cases <tag>:
  a  [1, 96, 112]  factor 1.0, range None            (n % 4 == 0: the kernels' 16-byte loads)
  b  [3, 37, 41]   factor 1.6, range None            (odd, multi-channel as the inpainting notebook passes: the scalar tail)
  c  [1, 50, 51]   factor 0.6, range (0, 0.05)       (elements above the range fall in no bin)
Keys per case:
  <tag>_err, <tag>_unc               the inputs (float32, the case's shape)
  <tag>_range                        (lo, hi) float64, NaN NaN for range None;  <tag>_bounds  the host torch.linspace boundaries (float32)
  <tag>_uce_o<j>, _err_o<j>, _unc_o<j>, _prop_o<j>     uceloss's four outputs, j = 0: outlier 0, j = 1: outlier 1e-4
  <tag>_count (int64), _mean_err, _mean_unc, _unc_mean, _uce64_o0, _uce64_o1      the float64 restatement
  <tag>_ref_dev                      the largest relative deviation of the reference's fp32 outputs from the restatement (per-bin means
                                     relative to the largest mean, uce relative to sum_k prop_k max(unc_k, err_k))
and n_bins, outliers."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_BINS = 15
OUTLIERS = (0.0, 1e-4)
CASES = {"a": ((1, 96, 112), 1.0, None, 22), "b": ((3, 37, 41), 1.6, None, 24), "c": ((1, 50, 51), 0.6, (0.0, 0.05), 23)}


def maps(shape, factor, seed):
    rng = np.random.default_rng(seed)
    unc = np.exp(rng.normal(-5.0, 0.6, size=shape)).astype(np.float32)
    err = (unc * rng.chisquare(1, size=shape) * factor).astype(np.float32)
    return err, unc


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "uce.npz")
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from utils.uce import uceloss
    import uce_restatement as R
    res = {"n_bins": np.int64(N_BINS), "outliers": np.array(OUTLIERS)}
    any_empty = any_dropped = False
    for tag, (shape, factor, rng_, seed) in CASES.items():
        err, unc = maps(shape, factor, seed)
        te, tu = torch.from_numpy(err.copy()), torch.from_numpy(unc.copy())
        lo, hi = (tu.min().item(), tu.max().item()) if rng_ is None else rng_
        bounds = torch.linspace(lo, hi, N_BINS + 1).numpy()                  # what uceloss computes on CPU tensors
        r = R.restate(err, unc, bounds)
        res[tag + "_err"], res[tag + "_unc"], res[tag + "_bounds"] = err, unc, bounds
        res[tag + "_range"] = np.array([np.nan, np.nan] if rng_ is None else rng_, np.float64)
        res[tag + "_count"], res[tag + "_mean_err"], res[tag + "_mean_unc"] = r["count"], r["mean_err"], r["mean_unc"]
        res[tag + "_unc_mean"] = np.float64(r["unc_mean"])
        dev = 0.0
        for j, o in enumerate(OUTLIERS):
            uce, e_b, u_b, prop = (t.numpy() for t in uceloss(te, tu, n_bins=N_BINS, outlier=o, range=rng_))
            for name, v in (("uce", uce), ("err", e_b), ("unc", u_b), ("prop", prop)):
                res["%s_%s_o%d" % (tag, name, j)] = v.astype(np.float32)
            k = R.kept(r, o)
            res["%s_uce64_o%d" % (tag, j)] = np.float64(R.uce(r, o))
            # the restatement and the reference agree on what is where
            assert np.array_equal(np.rint(prop.astype(np.float64) * r["n"]).astype(np.int64), r["count"]), tag
            assert e_b.shape == u_b.shape == (int(k.sum()),), tag
            dev = max(dev, np.abs(e_b - r["mean_err"][k]).max() / R.mean_scale(r), np.abs(u_b - r["mean_unc"][k]).max() / R.mean_scale(r),
                      abs(float(uce[0]) - R.uce(r, o)) / R.uce_scale(r))
            if o == 0.0:
                any_empty |= bool((r["count"] == 0).any())
            else:
                any_dropped |= bool(((r["count"] > 0) & ~k).any())
        res[tag + "_ref_dev"] = np.float64(dev)
        # the quirks the cases are there to exercise
        flat = unc.reshape(-1)
        if rng_ is None:
            assert r["count"].sum() == flat.size - int((flat == flat.min()).sum()), tag        # the minimum pixel is in no bin
        else:
            assert r["count"].sum() < flat.size, tag                                           # elements outside the range
        on_edge = np.isin(flat, bounds) & (flat != flat.min()) & (flat != flat.max())
        assert not on_edge.any(), tag
        print("%s: n %d, populated bins %d, kept at 1e-4 %d, ref_dev %.3e" % (tag, flat.size, (r["count"] > 0).sum(), R.kept(r, 1e-4).sum(), dev))
    assert any_empty, "no case has an empty bin"
    assert any_dropped, "no case drops a populated bin at outlier 1e-4"
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) <= 200 * 1024


if __name__ == "__main__":
    main()
