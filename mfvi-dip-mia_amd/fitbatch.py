"""Many independent MFVI fits advanced by ONE iteration of launches.

The reference runs its (temp, sigma) candidates and the slices of a volume as one process per fit, each a chain of small K = 1
launches that leave most of an MI355X idle (bayesian_optimization.py:3760-3775, :1360-1372).  A FitBatch of F fits with K samples
each is one plan of F * K samples in fits mode (mfvi_plan_set_fits): sample i belongs to fit i // K, reads that fit's mu / rho / BN
block and input, and its gradient is reduced into that fit's row.  One iteration is

    z[f]   = z0[f] + 0.1 * N(0,1)                 RNG domain INPUT, sample f          (mfvi_perturb_input_fits)
    out    = net(z)                                eps of global sample f * K + k      (mfvi_forward, fits mode)
    nll[f] = 1/K sum_k NLL(out[f, k], target[f])                                       (mfvi_gaussian_nll_fits)
    grads                                                                              (mfvi_backward, fits mode)
    KL[f], Adam with temp[f], prior_sigma[f], lr[f]                                    (mfvi_elbo_update_fits)
    ema[f]                                         on a second stream beside the backward pass (mfvi_ema_fits)

whatever F is.  RNG identity: fit f owns the global samples f * K .. f * K + K - 1 of eps and sample f of the INIT, z0 and input
perturbation domains, so fit 0 of a batch is the standalone ElboEngine(seed, K)."""
import math

from . import _lib as L
from .program import skip_program

TASKS = ("den", "sr")
EXP_WEIGHT = 0.99       # EMA weight of the smoothed output (bayesian_optimization.py:1292)


def per_fit(value, n_fits, name):
    """A scalar or a sequence of length n_fits -> list of n_fits floats."""
    try:
        vals = [float(v) for v in value]
    except TypeError:
        return [float(value)] * n_fits
    if len(vals) != n_fits:
        raise ValueError("%s: %d values for %d fits (a scalar, or one value per fit)" % (name, len(vals), n_fits))
    return vals


def prior_sigmas(temps, sigmas):
    """Per fit, exactly as ElboEngine computes it (bayesian_optimization.py:1335-1336 + modules/module.py:38, rounded to fp32)."""
    import numpy as np
    return [float(np.float32(math.sqrt(t) * s + 1e-6)) for t, s in zip(temps, sigmas)]


def check_args(H, W, n_fits, task, K, temp, sigma, lr, init):
    """Everything that can be refused without the library; -> (temps, sigmas, lrs)."""
    if task in ("ct", "inp"):
        raise NotImplementedError("FitBatch serves denoising and super-resolution; the data terms of task %r are not batched" % (task,))
    if task not in TASKS:
        raise ValueError("task %r: 'den' or 'sr'" % (task,))
    if int(n_fits) < 1 or int(K) < 1 or int(n_fits) * int(K) > 65535:
        raise ValueError("n_fits=%r, K=%r: at least 1 each, n_fits * K < 65536" % (n_fits, K))
    if H < 1 or W < 1 or H % 4 or W % 4:
        raise ValueError("H=%r, W=%r: multiples of 4 (the input-scale layers run on the matrix-core kernels)" % (H, W))
    if init not in ("per_fit", "shared"):
        raise ValueError("init %r: 'per_fit' or 'shared'" % (init,))
    temps, sigmas, lrs = per_fit(temp, n_fits, "temp"), per_fit(sigma, n_fits, "sigma"), per_fit(lr, n_fits, "lr")
    if any(not t >= 0.0 for t in temps) or any(not s >= 0.0 for s in sigmas) or any(not r > 0.0 for r in lrs):
        raise ValueError("temp and sigma must be >= 0 and lr > 0 for every fit")
    return temps, sigmas, lrs


class FitBatch:
    _book = None            # a BatchBook once track()ed

    def __init__(self, H, W, n_fits, task="den", K=1, input_depth=16, temp=1.0, sigma=0.1, lr=1e-3, seed=1, sr_factor=4, net_kwargs=None,
                 init="per_fit", autotune=True):
        self.temps, self.sigmas, self.lrs = check_args(H, W, n_fits, task, K, temp, sigma, lr, init)
        if task == "sr" and (sr_factor < 1 or H % sr_factor or W % sr_factor):
            raise ValueError("sr_factor %r does not divide %dx%d" % (sr_factor, H, W))
        import numpy as np
        import torch
        self.torch = torch
        self.task, self.F, self.K, self.H, self.W = task, int(n_fits), int(K), H, W
        self.seed, self.sr_factor, self.input_depth, self.init = int(seed), int(sr_factor), int(input_depth), init
        self.net_kwargs = dict(net_kwargs or {})
        self.prior_sigma = prior_sigmas(self.temps, self.sigmas)
        self.prog, self.zin, self.zout, self.names = skip_program(H, W, input_depth, 2, **self.net_kwargs)
        F, K, P = self.F, self.K, self.prog
        self.n = F * K
        self.plan = P.compile(self.zin, self.zout, self.n)
        self.n_vi, self.n_bn = P.n_vi, P.n_bn
        self.n_params = 2 * P.n_vi + P.n_bn
        self.stride = (self.n_params + 3) // 4 * 4                   # row stride of params / m / v / grads: every fit's MU block 16-byte aligned
        dev = "cuda"
        self._pbuf = torch.zeros((F, self.stride), dtype=torch.float32, device=dev)
        self._mbuf = torch.zeros_like(self._pbuf); self._vbuf = torch.zeros_like(self._pbuf)
        self.params, self.m, self.v = self._pbuf[:, :self.n_params], self._mbuf[:, :self.n_params], self._vbuf[:, :self.n_params]
        # gradients and the float64 NLL accumulators in ONE allocation: one fill launch clears both per iteration
        self._gbuf = torch.zeros(4 * F * self.stride + 8 * F, dtype=torch.uint8, device=dev)
        self._grows = self._gbuf[:4 * F * self.stride].view(torch.float32).view(F, self.stride)
        self.grads = self._grows[:, :self.n_params]
        self.nll_acc = self._gbuf[4 * F * self.stride:].view(torch.float64)
        self.kl = torch.zeros(F, dtype=torch.float64, device=dev)
        self.dead_dev = torch.zeros(F, dtype=torch.int32, device=dev)
        self.hyper = torch.tensor(np.array([[0.0, ps, t, r] for ps, t, r in zip(self.prior_sigma, self.temps, self.lrs)], np.float32), device=dev)   # mfvi_fit_hyper[F]
        self.z0 = torch.empty((F, input_depth, H, W), dtype=torch.float32, device=dev)
        self.z = torch.empty_like(self.z0)
        self.out = torch.empty((self.n, 2, H, W), dtype=torch.float32, device=dev)
        self.dout = torch.empty_like(self.out)
        self.ema = torch.zeros((F, 2, H, W), dtype=torch.float32, device=dev)
        self.upd_scratch = torch.zeros(L.lib().mfvi_elbo_update_fits_scratch_bytes(F), dtype=torch.uint8, device=dev)
        self.targets = None
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

    def set_targets(self, targets):
        """den: the noisy images [F, H, W]; sr: the low-resolution images [F, H / f, W / f]."""
        t = self.torch.as_tensor(targets)
        f = self.sr_factor if self.task == "sr" else 1
        if tuple(t.shape) != (self.F, self.H // f, self.W // f):
            raise ValueError("targets of shape %s, expected %s" % (tuple(t.shape), (self.F, self.H // f, self.W // f)))
        self.targets = t.contiguous().float().cuda()

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
            if self._book is None:
                L.check(L.lib().mfvi_ema_fits(L.ptr(self.out), self.F, self.K, 2, self.H, self.W, L.ptr(self.ema), EXP_WEIGHT, int(self._ema_n == 0),
                                              L.stream_ptr()))
            else:                        # the same EMA from mfvi_bookkeep_fits, and the iteration's records (batchbook.BatchBook)
                self._book.iteration(self.out, self.K, self._ema_n == 0)
            self._ema_done.record(self._side)
        self._ema_n += 1

    def track(self, gt, num_iter, noisy=None):
        """Record what the single-fit runner records per iteration, for every fit -> the BatchBook; step() then
        runs its iteration where the EMA runs."""
        from .batchbook import BatchBook
        return BatchBook(self, num_iter, gt, noisy)

    def metrics(self, gt):
        """dict(psnr=[F], ssim=[F]) of recon() against the ground truth ([H, W] shared, or [F, H, W]), one mfvi_pair_metrics call."""
        from .batchbook import recon_metrics
        return recon_metrics(self, gt)

    def grad_only(self, step=None, perturb=True, ema=False):
        """Everything of one iteration except the update: grads [F, n_params] and nll_acc [F] hold the result (no KL term)."""
        if self.targets is None:
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
        L.check(lib.mfvi_gaussian_nll_fits(L.ptr(self.out), L.ptr(self.targets), self.targets[0].numel(), F, K, self.H, self.W,
                                           self.sr_factor if self.task == "sr" else 1, 1.0 / K, L.ptr(self.dout), L.ptr(self.nll_acc), sp))
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
        """clip(ema[:, 0], 0, 1) [F, H, W]: the smoothed reconstruction of every fit."""
        self._wait_ema()
        return self.ema[:, 0].clamp(0.0, 1.0).contiguous()

    def psnr(self, gt):
        """[F]: PSNR of clip(ema[:, 0], 0, 1) against the ground truth ([H, W] shared, or [F, H, W]) -- the psnr_gt_sm the reference returns to
        its search (bayesian_optimization.py:1400-1403, :1436)."""
        import numpy as np
        torch, lib, sp = self.torch, L.lib(), L.stream_ptr()
        g = torch.as_tensor(gt).float().cuda()
        if g.dim() == 2:
            g = g[None].expand(self.F, -1, -1)
        if tuple(g.shape) != (self.F, self.H, self.W):
            raise ValueError("ground truth of shape %s, expected %s" % (tuple(g.shape), (self.F, self.H, self.W)))
        g = g.contiguous()
        rec = self.recon()
        acc = torch.zeros(self.F, dtype=torch.float64, device="cuda")
        for f in range(self.F):
            L.check(lib.mfvi_sq_err_sum(L.ptr(g[f]), L.ptr(rec[f]), self.H * self.W, L.ptr(acc[f:]), sp))
        mse = acc.cpu().numpy() / float(self.H * self.W)
        with np.errstate(divide="ignore"):
            return 10.0 * np.log10(1.0 / mse)

    def predict(self, n_samples, target=None, clip=False, step=None, chunk=None, fits_per_call=None, calibration=None):
        """Posterior predictive maps of every fit at once (batchpredict.predict_fits): per fit what
        to_engine(f).predict(n_samples, ...) returns, stacked, from one set of launches per chunk of draws instead of one chain per fit."""
        from .batchpredict import predict_fits
        return predict_fits(self, n_samples, target=target, clip=clip, step=step, chunk=chunk, fits_per_call=fits_per_call, calibration=calibration)

    def to_engine(self, f, autotune=False):
        """An ElboEngine holding copies of fit f's parameters, Adam moments, step count, input and target: predict(), calibration and the
        single-fit runner then work on any fit of a batch.  (Continued alone it draws eps of the global samples 0 .. K - 1, not f * K ..)"""
        from .engine import ElboEngine
        if not 0 <= f < self.F:
            raise ValueError("fit %r outside 0..%d" % (f, self.F - 1))
        eng = ElboEngine(self.H, self.W, task=self.task, K=self.K, input_depth=self.input_depth, temp=self.temps[f], sigma=self.sigmas[f],
                         lr=self.lrs[f], seed=self.seed, sr_factor=self.sr_factor, net_kwargs=self.net_kwargs, autotune=autotune)
        v = self.fit(f)
        eng.params.copy_(v["params"]); eng.m.copy_(v["m"]); eng.v.copy_(v["v"]); eng.z0.copy_(v["z0"])
        eng.t = self.t; eng.t_applied.fill_(self.t)
        if self.targets is not None:
            eng.set_target(self.targets[f].clone())
        return eng
