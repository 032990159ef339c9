"""utils/uce.py uceloss restated in float64 numpy, shared by the calibration tests and scripts/make_golden_uce.py.

The bin of an element is decided exactly as the reference decides it: float32 uncertainty against float32 boundaries, gt on the lower and
le on the upper one.  Everything after that (sums, means, the UCE) is float64; `prop32` is count / n rounded once to float32, which is what
the reference compares with `outlier`."""
import numpy as np

FP32_ULP = float(np.finfo(np.float32).eps)          # 2^-23


def restate(err, unc, bounds):
    """-> dict(count i64 [nb], n, sum_err, sum_unc, mean_err, mean_unc f64 [nb] (NaN in an empty bin), prop f64, prop32 f32, unc_mean f64)."""
    e = np.asarray(err, np.float32).reshape(-1)
    u = np.asarray(unc, np.float32).reshape(-1)
    b = np.asarray(bounds, np.float32).reshape(-1)
    nb, n = b.size - 1, u.size
    count = np.zeros(nb, np.int64); se = np.zeros(nb); su = np.zeros(nb)
    for k in range(nb):
        with np.errstate(invalid="ignore"):
            m = (u > b[k]) & (u <= b[k + 1])
        count[k] = m.sum()
        se[k] = e[m].astype(np.float64).sum()
        su[k] = u[m].astype(np.float64).sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        me, mu = se / count, su / count
    prop = count / float(n)
    return dict(count=count, n=n, sum_err=se, sum_unc=su, mean_err=me, mean_unc=mu, prop=prop, prop32=prop.astype(np.float32),
                unc_mean=u.astype(np.float64).sum() / n)


def kept(r, outlier):
    return r["prop32"].astype(np.float64) > float(outlier)


def uce(r, outlier):
    k = kept(r, outlier)
    return float((np.abs(r["mean_unc"][k] - r["mean_err"][k]) * r["prop"][k]).sum())


def uce_scale(r):
    """What a UCE error is measured against: sum_k prop_k * max(unc_k, err_k) over the populated bins (the UCE itself cancels when a fit is
    well calibrated)."""
    k = r["count"] > 0
    return float((r["prop"][k] * np.maximum(r["mean_unc"][k], r["mean_err"][k])).sum())


def mean_scale(r):
    k = r["count"] > 0
    return float(max(r["mean_unc"][k].max(), r["mean_err"][k].max()))


def tolerance(ref_dev):
    """fp32 outputs against the reference golden: max(4 x the reference's own deviation from float64, 4 fp32 ulp)."""
    return max(4.0 * float(ref_dev), 4.0 * FP32_ULP)
