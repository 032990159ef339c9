"""Posterior predictive statistics on the GPU (BayTorch/inference/utils.py:11-24 uncert_regression_gal).

N draws y_k of the fitted net are folded chunk by chunk into a per-pixel fp64 accumulator (mfvi_predictive_accumulate) and turned into
fp32 maps once (mfvi_predictive_finalize):  mean [Cimg,H,W], epi / ale / total [H,W], and with a ground truth err2 / mse_mc [H,W].
The per-pixel summation order is the sample order, so the maps do not depend on how the draws were chunked."""
from . import _lib as L

MODES = {"raw": L.PRED_RAW, "logprec": L.PRED_LOGPREC, "inp": L.PRED_INP, "mean_only": L.PRED_MEAN_ONLY}
DEFAULT_STEP = 2 ** 31          # RNG step of the posterior draws: a counter value no fit reaches, so no training iteration's eps is reused


def mode_code(mode):
    if mode not in MODES:
        raise ValueError("mode %r: one of %s" % (mode, ", ".join(MODES)))
    return MODES[mode]


def image_channels(C, mode):
    """(Cimg, has_ale) of a C-channel output under `mode`."""
    return {"raw": (C - 1, True), "logprec": (1, True), "inp": (3, True), "mean_only": (1, False)}[mode]


def default_mode(C):
    """The task's transform by channel count: 1 -> CT (mean_only), 2 -> den / SR (logprec), 4 -> inpainting (inp)."""
    if C not in (1, 2, 4):
        raise ValueError("no default predictive mode for %d output channels: pass mode='raw' | 'logprec' | 'inp' | 'mean_only'" % C)
    return {1: "mean_only", 2: "logprec", 4: "inp"}[C]


class Accumulator:
    """The fp64 accumulator of one prediction: add(out, n) per chunk (first chunk overwrites), finalize(N, ref) -> dict of maps."""

    def __init__(self, C, H, W, mode):
        import torch
        self.torch = torch
        self.C, self.H, self.W, self.mode = int(C), int(H), int(W), mode
        code = mode_code(mode)
        n = L.lib().mfvi_predictive_acc_doubles(self.C, self.H, self.W, code)
        if n < 0:
            raise ValueError("predictive mode %r does not take %d output channels" % (mode, C))
        self.code = code
        self.cimg, self.has_ale = image_channels(self.C, mode)
        self.buf = torch.empty(n, dtype=torch.float64, device="cuda")
        self.state = self.buf[:(2 * self.cimg + int(self.has_ale)) * self.H * self.W]      # the part an all-reduce over ranks sums
        self.n = 0

    def add(self, out, n, clip=False):
        """Fold out[:n] (a contiguous fp32 [>= n, C, H, W] CUDA tensor) into the sums."""
        t = self.torch
        if not (out.is_cuda and out.dtype == t.float32 and out.is_contiguous()):
            raise TypeError("predictive accumulate needs a contiguous float32 CUDA tensor")
        if tuple(out.shape[1:]) != (self.C, self.H, self.W) or out.shape[0] < n:
            raise ValueError("chunk of shape %s, expected [>= %d, %d, %d, %d]" % (tuple(out.shape), n, self.C, self.H, self.W))
        L.check(L.lib().mfvi_predictive_accumulate(L.ptr(out), int(n), self.C, self.H, self.W, self.code, int(bool(clip)), int(self.n == 0),
                                                   L.ptr(self.buf), L.stream_ptr()))
        self.n += int(n)

    def finalize(self, n_total=None, ref=None):
        """-> dict(mean [Cimg,H,W], epi, ale (None in mean_only), total, err2, mse_mc (None without ref) [H,W], sums float64[3])."""
        t = self.torch
        N = self.n if n_total is None else int(n_total)
        if N < 2:
            raise ValueError("posterior predictive statistics need at least 2 samples, got %d" % N)
        H, W = self.H, self.W
        if ref is not None:
            ref = t.as_tensor(ref).to(device="cuda", dtype=t.float32).contiguous()
            if ref.numel() != self.cimg * H * W:
                raise ValueError("target of %d elements, expected %d x %d x %d" % (ref.numel(), self.cimg, H, W))
        maps = t.empty((self.cimg + 5) * H * W, dtype=t.float32, device="cuda")
        mean = maps[:self.cimg * H * W].view(self.cimg, H, W)
        epi, ale, total, err2, mse_mc = (maps[(self.cimg + i) * H * W:(self.cimg + i + 1) * H * W].view(H, W) for i in range(5))
        sums = t.empty(3, dtype=t.float64, device="cuda")
        L.check(L.lib().mfvi_predictive_finalize(L.ptr(self.buf), N, self.C, H, W, self.code, L.ptr(ref), L.ptr(mean), L.ptr(epi),
                                                 L.ptr(ale) if self.has_ale else None, L.ptr(total), L.ptr(err2) if ref is not None else None,
                                                 L.ptr(mse_mc) if ref is not None else None, L.ptr(sums), L.stream_ptr()))
        return dict(mean=mean, epi=epi, ale=ale if self.has_ale else None, total=total, err2=err2 if ref is not None else None,
                    mse_mc=mse_mc if ref is not None else None, sums=sums)
