"""Writes tests/golden/tv.npz: inputs and the outputs of the reference's tv_loss (utils/sr_utils.py:84-94) and of its autograd on them.

usage:  PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_tv.py <reference checkout> [out.npz]

Inputs: seeded uniform [0, 1) on a 2^-16 grid (exact in float32), checked to have no zero cell (no two neighbours tie in both
directions), one per shape and shared by the shape's betas.  Cases (`cases`: their names, "<N>x<C>x<H>x<W>_b<beta>"):
  1x1x2x2                one cell
  1x1x1x8, 1x1x8x1       no cell: value and gradient 0
  2x3x5x7                odd, multi-plane, narrower than one 16-byte load pair                     beta 0.5, 1.0, 0.75
  3x1x17x65, 1x2x33x130  cells straddling a 16 x 64 tile edge, row tails that are no multiple of 4
  1x2x32x40              rows of whole 16-byte quads                                                beta 0.5, 1.0, 0.75
Keys:
  x_<shape>              the input (float32)
  <case>_val32           tv_loss on the float32 input (float32);   <case>_val64   on the input converted to float64
  <case>_grad64          autograd's gradient of the float64 evaluation (float64, the input's shape)
and the flat-patch case: flat_x (1x1x5x7 with the constant patch [1:3, 1:3]), flat_val32, flat_val64, flat_nan (bool: where the
reference's float64 autograd gradient at beta 0.5 is NaN -- asserted here to be exactly the pixels that touch a zero cell, 3 of them)."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {(1, 1, 2, 2): (0.5,), (1, 1, 1, 8): (0.5,), (1, 1, 8, 1): (0.5,), (2, 3, 5, 7): (0.5, 1.0, 0.75), (3, 1, 17, 65): (0.5,),
          (1, 2, 33, 130): (0.5,), (1, 2, 32, 40): (0.5, 1.0, 0.75)}


def shape_tag(shape):
    return "x".join(str(s) for s in shape)


def case_name(shape, beta):
    return "%s_b%g" % (shape_tag(shape), beta)


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "tv.npz")
    sys.dont_write_bytecode = True
    # in-process empty stubs for packages utils/common_utils.py imports but tv_loss never uses (as oracle/make_golden.py does)
    for m in ["torchvision", "torchvision.transforms", "skimage", "skimage.metrics"]:
        sys.modules.setdefault(m, types.ModuleType(m))
    sys.modules["skimage.metrics"].peak_signal_noise_ratio = None
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from utils.sr_utils import tv_loss
    import tv_restatement as R

    def reference(x, beta):
        v32 = tv_loss(torch.from_numpy(x.copy()), beta).numpy()
        t = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
        v64 = tv_loss(t, beta)
        v64.backward()
        return np.float32(v32), np.float64(v64.item()), t.grad.numpy().copy()
    res, names = {}, []
    for si, (shape, betas) in enumerate(SHAPES.items()):
        rng = np.random.default_rng(700 + si)
        x = (rng.integers(0, 1 << 16, size=shape) / float(1 << 16)).astype(np.float32)
        assert not R.zero_cells_touch(x).any(), shape                    # no ties: the reference's gradient is finite everywhere
        res["x_" + shape_tag(shape)] = x
        for beta in betas:
            name = case_name(shape, beta)
            v32, v64, g64 = reference(x, beta)
            assert np.isfinite(g64).all(), name
            if shape[2] == 1 or shape[3] == 1:
                assert v64 == 0.0 and not g64.any(), name
            res[name + "_val32"], res[name + "_val64"], res[name + "_grad64"] = v32, v64, g64
            names.append(name)
            dv = abs(R.tv_value(x, beta) - v64) / max(abs(v64), 1e-300)
            dg = np.abs(R.tv_grad(x, beta) - g64).max()
            print("%-22s value %.6f  restatement: value rel %.1e, gradient abs %.1e" % (name, v64, dv, dg))
    res["cases"] = np.array(names)
    # the flat patch: one zero cell
    rng = np.random.default_rng(799)
    x = (rng.integers(0, 1 << 16, size=(1, 1, 5, 7)) / float(1 << 16)).astype(np.float32)
    x[0, 0, 1:3, 1:3] = 0.5
    v32, v64, g64 = reference(x, 0.5)
    nan = np.isnan(g64)
    assert np.array_equal(nan, R.zero_cells_touch(x)) and nan.sum() == 3, nan.sum()
    res["flat_x"], res["flat_val32"], res["flat_val64"], res["flat_nan"] = x, v32, v64, nan
    print("flat patch: value %.6f, %d NaN pixels in the reference's gradient" % (v64, nan.sum()))
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) <= 200 * 1024


if __name__ == "__main__":
    main()
