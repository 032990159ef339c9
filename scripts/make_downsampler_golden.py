"""Writes tests/golden/downsampler.npz: the reference's Downsampler (models/downsampler.py:6-136, loaded by file path at generation time)
on seeded inputs — its 2-D kernel, forward output and autograd input gradient — for the cases of tests/test_downsampler_host.py.

usage:  PYTHONDONTWRITEBYTECODE=1 python scripts/make_downsampler_golden.py <reference checkout> [out.npz]

Keys per case <tag> = <kind>_f<factor>_<H>x<W>, everything for Downsampler(2, factor, kind, phase=0.5, preserve_size=True) on CPU float32:
  <tag>_kernel   the module's .kernel (float64 [T][T])
  <tag>_x_u8     the input [3][2][H][W] as uint8 (seeded); the input itself is x_u8.astype(float32) / float32(255), in [0, 1]
  <tag>_y        the module's output (float32 [3][2][H/f][W/f])
  <tag>_gy       the upstream gradient (float32, seeded N(0, 1), the shape of y)
  <tag>_gx       autograd's gradient of sum(y * gy) with respect to the input (float32 [3][2][H][W])
  <tag>_ref_dev  (2,) float64: the largest deviation of y and of gx from the float64 restatement (the reference's own fp32 error)"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "downsampler.npz")
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import test_downsampler_host as R
    spec = importlib.util.spec_from_file_location("reference_downsampler", os.path.join(ref, "models", "downsampler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = {}
    for ci, case in enumerate(R.CASES):
        kind, f, H, W = case
        tag = R.tag(case)
        rng = np.random.default_rng(1000 + ci)
        x_u8 = rng.integers(0, 256, size=(R.N, R.C, H, W), dtype=np.uint8)
        x = x_u8.astype(np.float32) / np.float32(255.0)
        gy = rng.standard_normal((R.N, R.C, H // f, W // f)).astype(np.float32)
        m = mod.Downsampler(n_planes=R.C, factor=f, kernel_type=kind, phase=0.5, preserve_size=True)
        xt = torch.from_numpy(x.copy()).requires_grad_(True)
        y = m(xt)
        assert tuple(y.shape) == gy.shape, tag
        (y * torch.from_numpy(gy)).sum().backward()
        y_np, gx = y.detach().numpy().astype(np.float32), xt.grad.numpy().astype(np.float32)
        dev = (np.abs(R.forward64(x, kind, f) - y_np).max(), np.abs(R.adjoint64(gy, kind, f, H, W) - gx).max())
        assert max(dev) <= 1e-6, (tag, dev)
        res[tag + "_kernel"], res[tag + "_x_u8"], res[tag + "_y"], res[tag + "_gy"], res[tag + "_gx"] = m.kernel.astype(np.float64), x_u8, y_np, gy, gx
        res[tag + "_ref_dev"] = np.array(dev, np.float64)
        print("%s: kernel %s, forward dev %.2e, gradient dev %.2e" % (tag, m.kernel.shape, dev[0], dev[1]))
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) <= 1024 * 1024


if __name__ == "__main__":
    main()
