"""Writes tests/golden/radon_dropin.npz: the reference's FastRadonTransform (radon/radon.py:4-55, loaded by file path at generation time)
on seeded inputs — its forward output and autograd image gradient — for the cases of tests/radon_restatement.py.

usage:  PYTHONDONTWRITEBYTECODE=1 python scripts/make_radon_golden.py <reference checkout> [out.npz]

Keys per case <name>, everything for FastRadonTransform((1, C, S, S), theta) on CPU float32:
  <name>_theta_deg  the angles in degrees (float32 [T]; the default arange(180.) where the case passes theta=None)
  <name>_x          the input [1][C][S][S] (float32, seeded uniform [0, 1))
  <name>_y          the module's output (float32 [1][C][T][S])
  <name>_gy         the upstream gradient (float32, seeded N(0, 1), the shape of y)
  <name>_gx         autograd's gradient of sum(y * gy) with respect to the input (float32 [1][C][S][S])
  <name>_ref_dev    (2,) float64: relerr of y and of gx against the float64 restatement (the reference's own fp32 error)
and for the case radon_restatement.CTOR_CASE the constructor's buffers: ctor_theta (radians), ctor_ts, ctor_tc, ctor_z, ctor_trans."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "radon_dropin.npz")
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import radon_restatement as R
    spec = importlib.util.spec_from_file_location("reference_radon", os.path.join(ref, "radon", "radon.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = {}
    for ci, case in enumerate(R.CASES):
        name, S, C, th = case
        rng = np.random.default_rng(2000 + ci)
        x = rng.random((1, C, S, S), dtype=np.float32)
        theta = R.theta_of(case)
        m = mod.FastRadonTransform((1, C, S, S), None if th is None else torch.from_numpy(theta.copy()))
        gy = rng.standard_normal((1, C, theta.size, S)).astype(np.float32)
        xt = torch.from_numpy(x.copy()).requires_grad_(True)
        y = m(xt)
        assert tuple(y.shape) == gy.shape, name
        (y * torch.from_numpy(gy)).sum().backward()
        y_np, gx = y.detach().numpy().astype(np.float32), xt.grad.numpy().astype(np.float32)
        dev = (R.relerr(y_np, R.forward64(x, theta)), R.relerr(gx, R.adjoint64(gy, theta, S)))
        assert max(dev) < 5e-5, (name, dev)
        res[name + "_theta_deg"], res[name + "_x"], res[name + "_y"], res[name + "_gy"], res[name + "_gx"] = theta, x, y_np, gy, gx
        res[name + "_ref_dev"] = np.array(dev, np.float64)
        if name == R.CTOR_CASE:
            for k in ("theta", "ts", "tc", "z", "trans"):
                res["ctor_" + k] = getattr(m, k).numpy().copy()
        print("%s: T = %d, forward dev %.2e, gradient dev %.2e" % (name, theta.size, dev[0], dev[1]))
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) <= 1024 * 1024


if __name__ == "__main__":
    main()
