"""One calibration() at a given size, repeated, for a kernel trace (DESIGN.md section 12 "Cost"):

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/calibration_prof.py [--size 256] [--reps 20]

Inputs as in scripts/make_golden_uce.py (unc = exp(N(-5, 0.6)), err = unc * chi^2_1); range=None, so every call runs the min / max kernels,
the binning kernel, the final kernel and, for the two outliers, the UCE kernel."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bins", type=int, default=15)
    a = ap.parse_args()
    import torch
    from mfvi_dip_mia_amd.calibration import calibration
    rng = np.random.default_rng(0)
    unc = np.exp(rng.normal(-5.0, 0.6, size=(a.size, a.size))).astype(np.float32)
    err = (unc * rng.chisquare(1, size=unc.shape)).astype(np.float32)
    e, u = torch.from_numpy(err).cuda(), torch.from_numpy(unc).cuda()
    for _ in range(a.reps):
        c = calibration(e, u, n_bins=a.bins)
        u0, u1 = c.uce(0.0), c.uce(1e-4)
    torch.cuda.synchronize()
    print("n %d, bins %d: uce %.6e, uce_1e-4 %.6e, populated bins %d" % (unc.size, a.bins, float(u0), float(u1), int((c["count"] > 0).sum())))


if __name__ == "__main__":
    main()
