"""Many independent MFVI inpainting fits advanced by ONE iteration of launches.

The reference's inpainting search runs 50 000 iterations per (temp, sigma) candidate, one process per fit, each a chain of small K = 1
launches on the 6-scale no-skip net (bayesian_optimization.py:2923-3075, bo_configs/bo_mfvi_inp.json), and ships six images with hair
masks.  An InpaintBatch of F fits with K samples each is one plan of F * K samples of that net (4 outputs) in fits mode, as FitBatch is
for denoising and super-resolution; one iteration is the one-group iteration of rowbatch.py with two launches of its own,

    nll[f] = 1/K sum_k masked NLL(out[f, k], image[f], mask[f])                        (mfvi_gaussian_nll_inpainting_fits)
    ema[f]                                         on a second stream beside the backward pass (mfvi_ema_inpainting_fits)

whatever F is.  The reference's images are 320 x 256: the two deepest maps (10 and 5 wide) are no multiple of 4 wide and run on the generic
fp32 kernels, which fits mode serves with the fit's own mu / rho.  RNG identity as FitBatch: fit 0 is ElboEngine(task="inp", seed, K)."""
from . import _lib as L
from .rowbatch import EXP_WEIGHT, ElboRowBatch, check_kl_type, check_prior_mixtures, per_fit


def inp_net():
    from .engine import INP_NET
    return dict(INP_NET)


def pyramid(H, W, n_scales):
    """The map sizes below the input: every scale halves with a stride-2 convolution, (h, w) -> (ceil(h / 2), ceil(w / 2))."""
    maps = []
    for _ in range(n_scales):
        H, W = (H + 1) // 2, (W + 1) // 2
        maps.append((H, W))
    return maps


def check_args(H, W, n_fits, K, temp, sigma, lr, init, net_kwargs=None):
    """Everything that can be refused without the library; -> (temps, sigmas, lrs)."""
    if int(n_fits) < 1 or int(K) < 1 or int(n_fits) * int(K) > 65535:
        raise ValueError("n_fits=%r, K=%r: at least 1 each, n_fits * K < 65536" % (n_fits, K))
    if H < 1 or W < 1 or H % 4 or W % 4:
        raise ValueError("H=%r, W=%r: multiples of 4 (the input-scale layers run on the matrix-core kernels)" % (H, W))
    kw = inp_net(); kw.update(net_kwargs or {})
    pad = max(kw.get("fd", 3), kw.get("fu", 3)) // 2
    ns = kw.get("ns", ())
    maps = pyramid(H, W, len(kw["nd"]))
    for i, (h, w) in enumerate(maps):
        if min(h, w) <= pad:
            raise ValueError("H=%r, W=%r: the map of scale %d is %d x %d; every map of the pyramid must be at least %d on a side (reflection pad %d "
                             "of the %d x %d filters)" % (H, W, i + 1, h, w, pad + 1, pad, 2 * pad + 1, 2 * pad + 1))
        if i < len(maps) - 1 and not (ns and ns[i + 1]) and (h % 2 or w % 2):
            raise ValueError("H=%r, W=%r: the map of scale %d is %d x %d; without a skip branch only the deepest map may be odd" % (H, W, i + 1, h, w))
    if init not in ("per_fit", "shared"):
        raise ValueError("init %r: 'per_fit' or 'shared'" % (init,))
    temps, sigmas, lrs = per_fit(temp, n_fits, "temp"), per_fit(sigma, n_fits, "sigma"), per_fit(lr, n_fits, "lr")
    if any(not t >= 0.0 for t in temps) or any(not s >= 0.0 for s in sigmas) or any(not r > 0.0 for r in lrs):
        raise ValueError("temp and sigma must be >= 0 and lr > 0 for every fit")
    return temps, sigmas, lrs


class InpaintBatch(ElboRowBatch):
    """The one-group ElboRowBatch of the 4-output inpainting net: rowbatch.py runs the iteration; here are the images and masks, the masked
    data term, the inpainting EMA, the 3-channel reconstruction and PSNR, and the engine of one fit."""
    task = "inp"
    images = None; masks = None; _mask_stride = 0

    def __init__(self, H, W, n_fits, K=1, input_depth=32, temp=1.0, sigma=0.1, lr=2e-3, seed=1, net_kwargs=None, init="per_fit", autotune=True,
                 kl_type="reverse", prior_mixture=None):
        self.temps, self.sigmas, self.lrs = check_args(H, W, n_fits, K, temp, sigma, lr, init, net_kwargs)
        self.kl_types = check_kl_type(kl_type, int(n_fits))      # a name, or one per fit
        self.prior_mixtures = check_prior_mixtures(prior_mixture, self.kl_types)      # None, one scale-mixture prior, or one per fit (None: a Gaussian row)
        self.F = int(n_fits)
        self.net_kwargs = dict(net_kwargs or {})
        kw = inp_net(); kw.update(self.net_kwargs)
        self._allocate(n_fits, n_fits, K, H, W, 4, input_depth, kw, seed, init, autotune)

    def _check_plan(self):
        if tuple(self.plan.out_shape) != (4, self.H, self.W):
            raise ValueError("the net maps %dx%d to %s" % (self.H, self.W, tuple(self.plan.out_shape)))

    def _alloc_own(self):
        super()._alloc_own()
        self.err_scratch = self.torch.zeros(self.F * L.MASKED_SQ_ERR_BLOCKS, dtype=self.torch.float64, device="cuda")

    def set_targets(self, images, masks):
        """The colour images [F, 3, H, W] and the masks (1 = known pixel): [F, 1|3, H, W], or one mask [1|3, H, W] / [H, W] shared by every
        fit.  Masks are rounded as ElboEngine.set_target rounds them (bayesian_optimization.py:3024)."""
        torch = self.torch
        t = torch.as_tensor(images)
        if tuple(t.shape) != (self.F, 3, self.H, self.W):
            raise ValueError("images of shape %s, expected %s" % (tuple(t.shape), (self.F, 3, self.H, self.W)))
        m = torch.as_tensor(masks)
        if m.dim() == 2:
            m = m[None]
        shared = m.dim() == 3
        if m.dim() not in (3, 4) or tuple(m.shape[-2:]) != (self.H, self.W) or m.shape[-3] not in (1, 3) or (not shared and m.shape[0] != self.F):
            raise ValueError("masks of shape %s, expected [%d, 1|3, %d, %d] or one shared [1|3, %d, %d]" % (tuple(m.shape), self.F, self.H, self.W, self.H, self.W))
        self.images = t.contiguous().float().cuda()
        self.masks = m.contiguous().float().cuda().round()
        self.mask_channels = int(m.shape[-3])
        self._mask_stride = 0 if shared else self.mask_channels * self.H * self.W

    def mask_of(self, f):
        return self.masks if self._mask_stride == 0 else self.masks[f]

    def _require_targets(self):
        if self.images is None:
            raise ValueError("set_targets first")

    def _data_term(self, d0, nd, out, dout):      # one group: d0 = 0, nd = F
        L.check(L.lib().mfvi_gaussian_nll_inpainting_fits(L.ptr(out), L.ptr(self.images), 3 * self.H * self.W, L.ptr(self.masks), self._mask_stride,
                                                          self.mask_channels, nd, self.K, self.H, self.W, 1.0 / self.K, L.ptr(dout),
                                                          L.ptr(self.nll_acc), L.stream_ptr()))

    def _ema_launch(self, d0, nd):
        L.check(L.lib().mfvi_ema_inpainting_fits(L.ptr(self.out), nd, self.K, self.H, self.W, L.ptr(self.ema), EXP_WEIGHT, int(self._ema_n == 0),
                                                 L.stream_ptr()))

    def track(self, gt, num_iter, noisy=None):
        """FitBatch.track for inpainting is not built: the 3-channel masked bookkeeping of the inpainting runner is not batched."""
        raise NotImplementedError("InpaintBatch.track: the 3-channel masked bookkeeping (book._BookInp) is not batched; run the single-fit "
                                  "runner on to_engine(f) for per-iteration records")

    def recon(self):
        """clip(ema[:, :3], 0, 1) [F, 3, H, W]: the smoothed reconstruction of every fit."""
        self._wait_ema()
        return self.ema[:, :3].clamp(0.0, 1.0).contiguous()

    def ale(self):
        """clip(ema[:, 3], 0, 1) [F, H, W]: the smoothed aleatoric variance exp(-s) of every fit."""
        self._wait_ema()
        return self.ema[:, 3].clamp(0.0, 1.0).contiguous()

    def psnr(self, gt):
        """[F]: PSNR of clip(ema[:, :3]) * mask against gt * mask, gt [3, H, W] shared or [F, 3, H, W] -- the psnr_gt_sm the inpainting runner
        returns to its search (bayesian_optimization.py:3049-3055), by mfvi_masked_sq_err_fits: one fixed-order reduction for all fits."""
        import numpy as np
        torch, lib, sp = self.torch, L.lib(), L.stream_ptr()
        if self.masks is None:
            raise ValueError("set_targets first")
        g = torch.as_tensor(gt).float().cuda()
        if g.dim() == 3:
            g = g[None].expand(self.F, -1, -1, -1)
        if tuple(g.shape) != (self.F, 3, self.H, self.W):
            raise ValueError("ground truth of shape %s, expected %s" % (tuple(g.shape), (self.F, 3, self.H, self.W)))
        g = g.contiguous()
        self._wait_ema()
        HW = self.H * self.W
        acc = torch.zeros(self.F, dtype=torch.float64, device="cuda")
        L.check(lib.mfvi_masked_sq_err_fits(L.ptr(self.ema), 4 * HW, L.ptr(g), 3 * HW, L.ptr(self.masks), self._mask_stride, self.mask_channels, self.F,
                                            self.H, self.W, L.ptr(acc), L.ptr(self.err_scratch), sp))
        mse = acc.cpu().numpy() / float(3 * HW)
        with np.errstate(divide="ignore"):
            return 10.0 * np.log10(1.0 / mse)

    def _make_engine(self, f, autotune):
        from .engine import ElboEngine
        return ElboEngine(self.H, self.W, task="inp", K=self.K, input_depth=self.input_depth, temp=self.temps[f], sigma=self.sigmas[f],
                          lr=self.lrs[f], seed=self.seed, net_kwargs=self.net_kwargs, autotune=autotune, **self._kl_kw(f))

    def _hand_target(self, eng, f):
        if self.images is not None:
            eng.set_target(self.images[f].clone(), self.mask_of(f).clone())
