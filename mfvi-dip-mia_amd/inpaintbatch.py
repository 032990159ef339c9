"""Many independent MFVI inpainting fits advanced by ONE iteration of launches.

The reference's inpainting search runs 50 000 iterations per (temp, sigma) candidate, one process per fit, each a chain of small K = 1
launches on the 6-scale no-skip net (bayesian_optimization.py:2923-3075, bo_configs/bo_mfvi_inp.json), and ships six images with hair
masks.  An InpaintBatch of F fits with K samples each is one plan of F * K samples of that net (4 outputs) in fits mode, as FitBatch is
for denoising and super-resolution; one iteration is

    z[f]   = z0[f] + 0.1 * N(0,1)                 RNG domain INPUT, sample f          (mfvi_perturb_input_fits)
    out    = net(z)                                eps of global sample f * K + k      (mfvi_forward, fits mode)
    nll[f] = 1/K sum_k masked NLL(out[f, k], image[f], mask[f])                        (mfvi_gaussian_nll_inpainting_fits)
    grads                                                                              (mfvi_backward, fits mode)
    KL[f], Adam with temp[f], prior_sigma[f], lr[f]                                    (mfvi_elbo_update_fits)
    ema[f]                                         on a second stream beside the backward pass (mfvi_ema_inpainting_fits)

whatever F is.  The reference's images are 320 x 256: the two deepest maps (10 and 5 wide) are no multiple of 4 wide and run on the generic
fp32 kernels, which fits mode serves with the fit's own mu / rho.  RNG identity as FitBatch: fit 0 is ElboEngine(task="inp", seed, K)."""
from . import _lib as L
from .fitbatch import EXP_WEIGHT, per_fit, prior_sigmas
from .program import skip_program


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


class InpaintBatch:
    def __init__(self, H, W, n_fits, K=1, input_depth=32, temp=1.0, sigma=0.1, lr=2e-3, seed=1, net_kwargs=None, init="per_fit", autotune=True):
        self.temps, self.sigmas, self.lrs = check_args(H, W, n_fits, K, temp, sigma, lr, init, net_kwargs)
        import numpy as np
        import torch
        self.torch = torch
        self.task, self.F, self.K, self.H, self.W = "inp", int(n_fits), int(K), H, W
        self.seed, self.input_depth, self.init = int(seed), int(input_depth), init
        self.net_kwargs = dict(net_kwargs or {})
        self.prior_sigma = prior_sigmas(self.temps, self.sigmas)
        kw = inp_net(); kw.update(self.net_kwargs)
        self.prog, self.zin, self.zout, self.names = skip_program(H, W, input_depth, 4, **kw)
        F, K, P = self.F, self.K, self.prog
        self.n = F * K
        self.plan = P.compile(self.zin, self.zout, self.n)
        if tuple(self.plan.out_shape) != (4, H, W):
            raise ValueError("the net maps %dx%d to %s" % (H, W, tuple(self.plan.out_shape)))
        self.n_vi, self.n_bn = P.n_vi, P.n_bn
        self.n_params = 2 * P.n_vi + P.n_bn
        self.stride = (self.n_params + 3) // 4 * 4                   # as FitBatch: every fit's MU block 16-byte aligned
        dev = "cuda"
        self._pbuf = torch.zeros((F, self.stride), dtype=torch.float32, device=dev)
        self._mbuf = torch.zeros_like(self._pbuf); self._vbuf = torch.zeros_like(self._pbuf)
        self.params, self.m, self.v = self._pbuf[:, :self.n_params], self._mbuf[:, :self.n_params], self._vbuf[:, :self.n_params]
        # gradients and the float64 NLL accumulators in ONE allocation: one fill launch clears both per iteration (the generic kernels
        # accumulate into the rows by atomics, so the rows must start from zero)
        self._gbuf = torch.zeros(4 * F * self.stride + 8 * F, dtype=torch.uint8, device=dev)
        self._grows = self._gbuf[:4 * F * self.stride].view(torch.float32).view(F, self.stride)
        self.grads = self._grows[:, :self.n_params]
        self.nll_acc = self._gbuf[4 * F * self.stride:].view(torch.float64)
        self.kl = torch.zeros(F, dtype=torch.float64, device=dev)
        self.dead_dev = torch.zeros(F, dtype=torch.int32, device=dev)
        self.hyper = torch.tensor(np.array([[0.0, ps, t, r] for ps, t, r in zip(self.prior_sigma, self.temps, self.lrs)], np.float32), device=dev)   # mfvi_fit_hyper[F]
        self.z0 = torch.empty((F, input_depth, H, W), dtype=torch.float32, device=dev)
        self.z = torch.empty_like(self.z0)
        self.out = torch.empty((self.n, 4, H, W), dtype=torch.float32, device=dev)
        self.dout = torch.empty_like(self.out)
        self.ema = torch.zeros((F, 4, H, W), dtype=torch.float32, device=dev)
        self.upd_scratch = torch.zeros(L.lib().mfvi_elbo_update_fits_scratch_bytes(F), dtype=torch.uint8, device=dev)
        self.err_scratch = torch.zeros(F * L.MASKED_SQ_ERR_BLOCKS, dtype=torch.float64, device=dev)
        self.images = None; self.masks = None; self._mask_stride = 0
        self.t = 0
        self._ema_n = 0                  # EMA updates so far (the first one copies)
        self._side = None; self._ema_done = None
        self.init_params()
        if autotune:                     # before the mode is switched on (tilings do not depend on it), with fit 0's parameters and input
            f0 = self.fit(0)
            self.plan.autotune(f0["mu"], f0["rho"], f0["bn"], self.z0[0], self.n)
        self.plan.set_fits(K, self.stride, self.stride)

    # -------------------------------------------------------------------------------------------
    def fit(self, f):
        """Views of fit f: dict(mu, rho, bn, params, m, v, grads, z0, ema)."""
        n = self.n_vi
        p = self._pbuf[f]
        return dict(mu=p[:n], rho=p[n:2 * n], bn=p[2 * n:self.n_params], params=p[:self.n_params], m=self._mbuf[f, :self.n_params],
                    v=self._vbuf[f, :self.n_params], grads=self._grows[f, :self.n_params], z0=self.z0[f], ema=self.ema[f])

    def init_params(self):
        """Per fit f as ElboEngine.init_params with sample f of the INIT / z0 streams (init='shared': every fit starts from fit 0's)."""
        lib, sp = L.lib(), L.stream_ptr()
        n = self.n_vi
        self._pbuf.zero_()
        for f in range(self.F if self.init == "per_fit" else 1):
            p = self._pbuf[f]
            L.check(lib.mfvi_normal_fill(self.seed, L.DOMAIN_INIT, 0, f, 0, n, 0.0, 0.1, L.ptr(p), sp))
            L.check(lib.mfvi_normal_fill(self.seed, L.DOMAIN_INIT, 1, f, 0, n, -3.0, 0.1, L.ptr(p[n:]), sp))
            L.check(lib.mfvi_uniform_fill(self.seed, 0, f, 0, self.z0[f].numel(), 0.1, L.ptr(self.z0[f]), sp))
        for b in self.prog.bns:
            self._pbuf[:, 2 * n + b["off"]:2 * n + b["off"] + b["C"]] = 1.0
        if self.init == "shared":
            self._pbuf[1:] = self._pbuf[:1]; self.z0[1:] = self.z0[:1]
        self._mbuf.zero_(); self._vbuf.zero_(); self.dead_dev.zero_(); self.t = 0; self._ema_n = 0

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

    # -------------------------------------------------------------------------------------------
    def _wait_ema(self):
        if self._ema_done is not None:
            self.torch.cuda.current_stream().wait_event(self._ema_done)

    def _ema(self):
        """The smoothed outputs of every fit from self.out, on a second stream behind the forward and beside the backward pass."""
        t = self.torch
        if self._side is None:
            self._side = t.cuda.Stream(); self._ema_done = t.cuda.Event()
        ready = t.cuda.Event(); ready.record(t.cuda.current_stream())
        with t.cuda.stream(self._side):
            self._side.wait_event(ready)
            L.check(L.lib().mfvi_ema_inpainting_fits(L.ptr(self.out), self.F, self.K, self.H, self.W, L.ptr(self.ema), EXP_WEIGHT, int(self._ema_n == 0),
                                                     L.stream_ptr()))
            self._ema_done.record(self._side)
        self._ema_n += 1

    def track(self, gt, num_iter, noisy=None):
        """FitBatch.track for inpainting is not built: the 3-channel masked bookkeeping of the inpainting runner is not batched."""
        raise NotImplementedError("InpaintBatch.track: the 3-channel masked bookkeeping (runner._BookInp) is not batched; run the single-fit "
                                  "runner on to_engine(f) for per-iteration records")

    def grad_only(self, step=None, perturb=True, ema=False):
        """Everything of one iteration except the update: grads [F, n_params] and nll_acc [F] hold the result (no KL term)."""
        if self.images is None:
            raise ValueError("set_targets first")
        lib, sp = L.lib(), L.stream_ptr()
        step = self.t if step is None else int(step)
        F, K = self.F, self.K
        self._gbuf.zero_()
        zsrc = self.z0
        if perturb:
            L.check(lib.mfvi_perturb_input_fits(L.ptr(self.z0), self.seed, step, self.z0[0].numel(), F, 0, 0.1, L.ptr(self.z), sp))
            zsrc = self.z
        self._wait_ema()                 # the previous iteration's EMA has read self.out
        p0 = self._pbuf[0]
        mu, rho, bn = p0[:self.n_vi], p0[self.n_vi:], p0[2 * self.n_vi:]
        g0 = self._grows[0]
        self.plan.forward(mu, rho, bn, zsrc, self.seed, step, 0, self.n, True, self.out)
        L.check(lib.mfvi_gaussian_nll_inpainting_fits(L.ptr(self.out), L.ptr(self.images), 3 * self.H * self.W, L.ptr(self.masks), self._mask_stride,
                                                      self.mask_channels, F, K, self.H, self.W, 1.0 / K, L.ptr(self.dout), L.ptr(self.nll_acc), sp))
        if ema:
            self._ema()
        self.plan.backward(mu, rho, bn, zsrc, self.seed, step, 0, self.n, self.dout, g0[:self.n_vi], g0[self.n_vi:], g0[2 * self.n_vi:], True)

    def step(self):
        """One ELBO iteration of every fit.  A fit whose data term is not finite keeps its parameters and moments and is marked dead."""
        lib, sp = L.lib(), L.stream_ptr()
        self.grad_only(self.t, ema=True)
        self.t += 1
        L.check(lib.mfvi_elbo_update_fits(L.ptr(self._pbuf), L.ptr(self._grows), L.ptr(self._mbuf), L.ptr(self._vbuf), self.n_vi, self.n_bn, self.stride,
                                          self.stride, self.F, L.ptr(self.hyper), 0.9, 0.999, 1e-8, self.t, L.ptr(self.nll_acc), L.ptr(self.dead_dev),
                                          L.ptr(self.kl), L.ptr(self.upd_scratch), sp))

    # -------------------------------------------------------------------------------------------
    def losses(self):
        """(nll[F], kl[F], loss[F]) of the last step (kl: of the parameters that step started from) -- forces a device sync.
        After grad_only alone kl is stale: the KL term is part of the update launch."""
        import numpy as np
        nll = self.nll_acc.cpu().numpy() / self.K
        kl = self.kl.cpu().numpy()
        return nll, kl, nll + np.asarray(self.temps) * kl

    @property
    def dead(self):
        """[F] int32: 1 for a fit that met a non-finite data term (sticky; its parameters stopped there)."""
        return self.dead_dev.cpu().numpy()

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

    def predict(self, n_samples, target=None, clip=False, step=None, chunk=None, fits_per_call=None, calibration=None):
        """Posterior predictive maps of every fit at once (batchpredict.predict_fits): per fit what
        to_engine(f).predict(n_samples, ...) returns, stacked, from one set of launches per chunk of draws instead of one chain per fit."""
        from .batchpredict import predict_fits
        return predict_fits(self, n_samples, target=target, clip=clip, step=step, chunk=chunk, fits_per_call=fits_per_call, calibration=calibration)

    def to_engine(self, f, autotune=False):
        """An ElboEngine(task="inp") holding copies of fit f's parameters, Adam moments, step count, input, image and mask: predict() and
        the single-fit runner then work on any fit of a batch.  (Continued alone it draws eps of the global samples 0 .. K - 1, not f * K ..)"""
        from .engine import ElboEngine
        if not 0 <= f < self.F:
            raise ValueError("fit %r outside 0..%d" % (f, self.F - 1))
        eng = ElboEngine(self.H, self.W, task="inp", K=self.K, input_depth=self.input_depth, temp=self.temps[f], sigma=self.sigmas[f],
                         lr=self.lrs[f], seed=self.seed, net_kwargs=self.net_kwargs, autotune=autotune)
        v = self.fit(f)
        eng.params.copy_(v["params"]); eng.m.copy_(v["m"]); eng.v.copy_(v["v"]); eng.z0.copy_(v["z0"])
        eng.t = self.t; eng.t_applied.fill_(self.t)
        if self.images is not None:
            eng.set_target(self.images[f].clone(), self.mask_of(f).clone())
        return eng
