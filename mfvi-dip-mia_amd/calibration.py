"""Uncertainty calibration on the GPU (utils/uce.py uceloss, the "UCE" cells of eval_{denoising,sr,ct,inp}.ipynb).

calibration(err, unc) bins an uncertainty map into n_bins equal-width bins and returns, per bin, the element count, the proportion and the
mean error / mean uncertainty (mfvi_uce_bins), all as device tensors; .uce(outlier) is uceloss's scalar.  The bin boundaries are
torch.linspace(lo, hi, n_bins + 1) in float32 computed ON THE HOST, exactly as the reference computes them on CPU tensors, and uploaded: one
ulp on a boundary moves pixels between bins.  An element equal to the lowest boundary (with range=None: the minimum pixel) is in no bin
but counts in n -- uceloss's own behaviour, kept."""
from . import _lib as L

MAX_BINS = L.UCE_MAX_BINS


def _flat(x, what):
    import torch
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s: a torch tensor, got %s" % (what, type(x).__name__))
    if not x.is_cuda:
        raise NotImplementedError("this implementation runs on the GPU only; there is no CPU path")
    return x.detach().to(torch.float32).contiguous().view(-1)


def host_bounds(lo, hi, n_bins):
    """The reference's boundaries: torch.linspace(lo, hi, n_bins + 1), float32, on the host."""
    import torch
    return torch.linspace(float(lo), float(hi), int(n_bins) + 1, dtype=torch.float32)


class Calibration(dict):
    """The result of calibration(): a dict of device tensors
        bounds [n_bins+1] f32, count [n_bins] i64, prop / err_in_bin / unc_in_bin [n_bins] f32 (NaN in an empty bin), unc_mean [] f32,
        n [] i64, sum_err / sum_unc [n_bins] f64 (the sums the means round)
    with uce(outlier) -> [1] f32 device tensor and kept(outlier) -> the boolean mask of the bins uceloss keeps."""

    def uce(self, outlier=0.0):
        import torch
        out = torch.empty(1, dtype=torch.float32, device=self["prop"].device)
        L.check(L.lib().mfvi_uce_value(L.ptr(self["prop"]), L.ptr(self["err_in_bin"]), L.ptr(self["unc_in_bin"]), int(self["prop"].numel()),
                                       float(outlier), L.ptr(out), L.stream_ptr()))
        return out

    def kept(self, outlier=0.0):
        return self["prop"].double() > float(outlier)          # the fp32 prop against the Python float, as `prop_in_bin.item() > outlier`


def minmax(unc):
    """(min, max) of a CUDA tensor as Python floats, NaN ignored (mfvi_uce_minmax; one sync)."""
    import torch
    u = _flat(unc, "unc")
    if u.numel() < 1:
        raise ValueError("empty tensor")
    scratch = torch.empty(L.lib().mfvi_uce_scratch_bytes(u.numel(), 1) // 8, dtype=torch.float64, device=u.device)
    mm = torch.empty(2, dtype=torch.float32, device=u.device)
    L.check(L.lib().mfvi_uce_minmax(L.ptr(u), u.numel(), L.ptr(mm), L.ptr(scratch), L.stream_ptr()))
    lo, hi = mm.cpu().tolist()
    return lo, hi


def calibration(err, unc, n_bins=15, range=None, bounds=None):
    """Per-bin calibration statistics of the error map `err` against the uncertainty map `unc` (CUDA tensors of equal numel, any shape).
    range: (lo, hi) of the bins; None: the min / max of unc (one device sync).  bounds: n_bins + 1 boundaries to use as given instead."""
    import torch
    e, u = _flat(err, "err"), _flat(unc, "unc")
    n = u.numel()
    if e.numel() != n:
        raise ValueError("err has %d elements, unc %d" % (e.numel(), n))
    if n < 1:
        raise ValueError("empty tensors")
    n_bins = int(n_bins)
    if not 1 <= n_bins <= MAX_BINS:
        raise ValueError("n_bins=%d outside 1..%d" % (n_bins, MAX_BINS))
    if e.device != u.device:
        raise ValueError("err on %s, unc on %s" % (e.device, u.device))
    with torch.cuda.device(u.device):
        lib, sp = L.lib(), L.stream_ptr()
        nbytes = lib.mfvi_uce_scratch_bytes(n, n_bins)
        if nbytes < 0:
            raise L.MfviError(lib.mfvi_last_error().decode())
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=u.device)
        if bounds is None:
            if range is None:
                mm = torch.empty(2, dtype=torch.float32, device=u.device)
                L.check(lib.mfvi_uce_minmax(L.ptr(u), n, L.ptr(mm), L.ptr(scratch), sp))
                range = mm.cpu().tolist()
            b = host_bounds(range[0], range[1], n_bins)
        else:
            b = torch.as_tensor(bounds, dtype=torch.float32).cpu().contiguous().view(-1)
            if b.numel() != n_bins + 1:
                raise ValueError("%d boundaries for %d bins" % (b.numel(), n_bins))
        if bool((b[1:] < b[:-1]).any()):
            raise ValueError("bin boundaries must not decrease")
        b = b.to(u.device)
        count = torch.empty(n_bins + 1, dtype=torch.int64, device=u.device)
        sums = torch.empty(2 * n_bins + 1, dtype=torch.float64, device=u.device)
        f = torch.empty(3 * n_bins + 1, dtype=torch.float32, device=u.device)
        prop, eb, ub, um = f[:n_bins], f[n_bins:2 * n_bins], f[2 * n_bins:3 * n_bins], f[3 * n_bins:]
        L.check(lib.mfvi_uce_bins(L.ptr(e), L.ptr(u), n, L.ptr(b), n_bins, L.ptr(scratch), L.ptr(count), L.ptr(sums), L.ptr(prop), L.ptr(eb),
                                  L.ptr(ub), L.ptr(um), sp))
    return Calibration(bounds=b, count=count[:n_bins], prop=prop, err_in_bin=eb, unc_in_bin=ub, unc_mean=um[0], n=count[n_bins],
                       sum_err=sums[:n_bins], sum_unc=sums[n_bins:2 * n_bins])


def uceloss(errors, uncert, n_bins=15, outlier=0.0, range=None):
    """Drop-in for utils/uce.py:9-40 on the HIP kernels: -> (uce [1], err_in_bin, avg_uncert_in_bin (the kept bins only: those with
    prop_in_bin > outlier), prop_in_bin [n_bins]), float32 on the inputs' device."""
    import torch
    if isinstance(errors, torch.Tensor) and isinstance(uncert, torch.Tensor) and not (errors.is_cuda and uncert.is_cuda):
        raise NotImplementedError("this implementation runs on the GPU only; there is no CPU path")
    if errors.numel() != uncert.numel():
        raise ValueError("errors has %d elements, uncert %d" % (errors.numel(), uncert.numel()))
    c = calibration(errors, uncert, n_bins=n_bins, range=range)
    with torch.cuda.device(c["prop"].device):
        keep = c.kept(outlier)
        return c.uce(outlier), c["err_in_bin"][keep], c["unc_in_bin"][keep], c["prop"].clone()


def ring_inputs(recons, gt, epi, ale=None, mask=None):
    """The notebooks' uceloss inputs from a run's arrays, on the GPU (mfvi_uce_ring_inputs): recons [S, C, H, W] snapshots, gt [C, H, W],
    epi [C, H, W], ale [1 | C, H, W] or None, mask [1 | C, H, W] or None (inpainting) -> (errvar, uncert), both [C, H, W] float32:
    errvar = mean_s (recon_s - gt)^2 (* mask), uncert = epi + ale."""
    import torch

    def dev(x):
        return None if x is None else torch.as_tensor(x).to(device="cuda", dtype=torch.float32).contiguous()
    rec, g, ep, al, mk = dev(recons), dev(gt), dev(epi), dev(ale), dev(mask)
    S, n = rec.shape[0], g.numel()
    if rec.numel() != S * n or ep.numel() != n:
        raise ValueError("recons %s, gt %s, epi %s do not match" % (tuple(rec.shape), tuple(g.shape), tuple(ep.shape)))
    err, unc = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    L.check(L.lib().mfvi_uce_ring_inputs(L.ptr(rec), S, n, L.ptr(g), L.ptr(mk), 0 if mk is None else mk.numel(), L.ptr(ep), L.ptr(al),
                                         0 if al is None else al.numel(), L.ptr(err), L.ptr(unc), L.stream_ptr()))
    return err.view(ep.shape), unc.view(ep.shape)


def npz_block(c, prefix):
    """The calibration.npz arrays of one source: <prefix>bounds, count, prop_in_bin, err_in_bin, uncert_in_bin (all n_bins, NaN in an empty
    bin), uce (outlier 0), uce_1e-4, U = sqrt(mean uncertainty) (the notebooks' title figure)."""
    u0, u1 = c.uce(0.0), c.uce(1e-4)
    return {prefix + "bounds": c["bounds"].cpu().numpy(), prefix + "count": c["count"].cpu().numpy(), prefix + "prop_in_bin": c["prop"].cpu().numpy(),
            prefix + "err_in_bin": c["err_in_bin"].cpu().numpy(), prefix + "uncert_in_bin": c["unc_in_bin"].cpu().numpy(),
            prefix + "uce": u0.cpu().numpy(), prefix + "uce_1e-4": u1.cpu().numpy(), prefix + "U": c["unc_mean"].sqrt().cpu().numpy()}
