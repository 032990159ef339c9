"""The iteration core under FitBatch, CtVolume, InpaintBatch and SiblingBatch.

A batch holds one parameter / moment / gradient row per fit (n_rows of them; a CtVolume's rows are its slices) and ONE plan of
rows_per_launch * K samples in fits mode (mfvi_plan_set_fits): sample i of a launch belongs to row i // K of the launch's group, reads that
row's mu / rho / BN block and input, and its gradient is reduced into that row.  The rows advance in groups of rows_per_launch through the
plan and its workspace, the last group with what is left; a batch whose rows all fit one launch has the single group (0, n_rows, 0, 0,
n_rows K).  One iteration is, per group g,

    z[r]   = z0[r] + 0.1 * N(0,1)                 RNG domain INPUT, sample r          (mfvi_perturb_input_fits, fit0 = g F)
    out    = net(z)                                eps of global sample r * K + k      (mfvi_forward, fits mode, k0 = g F K)
    the class's data term                                                              (_data_term)
    ema[r]                                         on a second stream beside the backward pass (_ema_launch, or the BatchBook's)
    grads                                                                              (mfvi_backward, fits mode)

and one update launch over all rows closes it (_update).  RNG identity: row r owns the global samples r * K .. r * K + K - 1 and sample r
of every per-row stream whatever rows_per_launch is, so row 0 of a batch is the standalone engine with the batch's seed."""
import math

from . import _lib as L
from .program import skip_program

TASKS = ("den", "sr")
EXP_WEIGHT = 0.99       # EMA weight of the smoothed output (bayesian_optimization.py:1292)
MAX_LAUNCH = 65535      # samples of one launch, and rows of one update launch (a grid dimension)


def per_fit(value, n_fits, name):
    """A scalar or a sequence of length n_fits -> list of n_fits floats."""
    try:
        vals = [float(v) for v in value]
    except TypeError:
        return [float(value)] * n_fits
    if len(vals) != n_fits:
        raise ValueError("%s: %d values for %d fits (a scalar, or one value per fit)" % (name, len(vals), n_fits))
    return vals


KL_TYPES = ("reverse", "forward")      # MFVI_KL_REVERSE, MFVI_KL_FORWARD: a name's index is its value in the C ABI


def check_kl_type(kl_type, n=None, name="kl_type"):
    """The direction of the KL term, refused without the library: 'reverse' = KL(prior || posterior), what the
    reference's runners use, or 'forward' = KL(posterior || prior), the textbook ELBO's.  n None: one name -> the name; else one name, or
    one per row -> the list of n names."""
    names = [kl_type] * (n or 1) if isinstance(kl_type, str) or not hasattr(kl_type, "__iter__") else list(kl_type)
    if len(names) != (n or 1):
        raise ValueError("%s: %d values for %s (a name, or one name per fit)" % (name, len(names), "%d fits" % n if n else "one fit"))
    for k in names:
        if k not in KL_TYPES:
            raise ValueError("%s=%r: 'reverse' or 'forward'" % (name, k))
    names = [str(k) for k in names]
    return names[0] if n is None else names


MIXTURE_MAX = 4      # MFVI_MIXTURE_MAX


def check_prior_mixture(prior_mixture, name="prior_mixture"):
    """A scale-mixture prior sum_j pi_j N(m_j, sigma_j^2), refused without the library: {'pi': seq, 'sigma': seq,
    'mu': seq or absent -> 0} with 1 to 4 components.  The sigma are prior scales as the reference's layers take them: 1e-6 is added and
    the value rounded to float32 (BayTorch/modules/module.py:34); the pi are used as given, not normalised.  None -> None; else
    dict(pi, mu, sigma: the given values as floats; scale: the final float32 scales), what mixture_struct packs for the C ABI."""
    import numpy as np
    if prior_mixture is None:
        return None
    if not isinstance(prior_mixture, dict) or "pi" not in prior_mixture or "sigma" not in prior_mixture or set(prior_mixture) - {"pi", "sigma", "mu"}:
        raise ValueError("%s=%r: a dict with 'pi' and 'sigma' (and 'mu'), one sequence each" % (name, prior_mixture))

    def seq(key, default=None):
        v = prior_mixture.get(key, default)
        try:
            return [float(x) for x in np.asarray(v, dtype=np.float64).reshape(-1)] if np.ndim(v) == 1 else None
        except (TypeError, ValueError):
            return None
    pi, sigma = seq("pi"), seq("sigma")
    if pi is None or sigma is None or not 1 <= len(pi) <= MIXTURE_MAX:
        raise ValueError("%s: 'pi' and 'sigma' are sequences of 1 to %d numbers, got %r" % (name, MIXTURE_MAX, prior_mixture))
    mu = seq("mu", [0.0] * len(pi))
    if mu is None or len(sigma) != len(pi) or len(mu) != len(pi):
        raise ValueError("%s: %d pi, %d sigma and %s mu (one of each per component)" % (name, len(pi), len(sigma), "no" if mu is None else len(mu)))
    scale = [float(np.float32(s + 1e-6)) for s in sigma]
    with np.errstate(all="ignore"):
        for j, (p, s, m) in enumerate(zip(pi, scale, mu)):
            p32, m32, iv = np.float32(p), np.float32(m), np.float32(1.0) / (np.float32(s) * np.float32(s))
            if not (np.isfinite(p32) and p32 > 0):
                raise ValueError("%s: pi[%d]=%r is not a finite positive float32" % (name, j, p))
            if not (np.isfinite(s) and s > 0):
                raise ValueError("%s: sigma[%d]=%r + 1e-6 is not a finite positive float32" % (name, j, sigma[j]))
            if not (np.isfinite(iv) and iv >= np.finfo(np.float32).tiny):
                raise ValueError("%s: 1 / (sigma[%d] + 1e-6)^2 is not a normal float32 (sigma=%r)" % (name, j, sigma[j]))
            if not np.isfinite(m32):
                raise ValueError("%s: mu[%d]=%r is not a finite float32" % (name, j, m))
    return dict(pi=pi, mu=mu, sigma=sigma, scale=scale)


def check_prior_mixtures(prior_mixture, kl_types, name="prior_mixture"):
    """Per row of a batch: None (no row has a mixture), one prior for every row, or a sequence with one prior or None (a Gaussian row) per
    row -> the list of checked priors.  A row with a mixture runs the forward direction: 'reverse' is refused as ElboEngine refuses it."""
    n = len(kl_types)
    rows = [prior_mixture] * n if prior_mixture is None or isinstance(prior_mixture, dict) else list(prior_mixture)
    if len(rows) != n:
        raise ValueError("%s: %d values for %d fits (None, one prior, or one prior or None per fit)" % (name, len(rows), n))
    rows = [check_prior_mixture(r, "%s[%d]" % (name, f)) for f, r in enumerate(rows)]
    for f, r in enumerate(rows):
        if r is not None and kl_types[f] == "reverse":
            raise NotImplementedError("%s[%d] with kl_type='reverse' is not built: the reference's estimate of that direction samples through "
                                      "MixtureNormal.rsample (BayTorch/distributions/distributions.py:17-22), no draw from the mixture; pass kl_type='forward'" % (name, f))
    return rows


def mixture_struct(pm):
    """mfvi_mixture_prior of a checked prior (None: the n == 0 entry of a per-row table, a Gaussian row)."""
    s = L.MixturePrior()
    if pm is not None:
        s.n = len(pm["pi"])
        for j in range(s.n):
            s.pi[j], s.mu[j], s.sigma[j] = pm["pi"][j], pm["mu"][j], pm["scale"][j]
    return s


def prior_sigmas(temps, sigmas):
    """Per fit, exactly as ElboEngine computes it (bayesian_optimization.py:1335-1336 + modules/module.py:38, rounded to fp32)."""
    import numpy as np
    return [float(np.float32(math.sqrt(t) * s + 1e-6)) for t, s in zip(temps, sigmas)]


def groups(n_slices, slices_per_launch, K):
    """The launch groups of a batch, a pure function: [(first row, rows, k0, fit0, samples)] -- group g starts at row g F, draws eps
    from global sample k0 = g F K on, perturbs with the INPUT samples fit0 = g F .., and the last group holds what is left."""
    D, F, K = int(n_slices), int(slices_per_launch), int(K)
    if D < 1 or F < 1 or K < 1:
        raise ValueError("n_slices=%r, slices_per_launch=%r, K=%r: at least 1 each" % (n_slices, slices_per_launch, K))
    return [(d0, min(F, D - d0), d0 * K, d0, min(F, D - d0) * K) for d0 in range(0, D, F)]


class RowBatch:
    """What a subclass supplies: its check_args before _allocate (nothing here is refused without the library), and the hooks
    _check_plan, _alloc_own, _fill_row, _after_init, _require_targets, _data_term, _ema_launch, _pre_step, _update, _make_engine and
    _hand_target."""
    _book = None                # a BatchBook once track()ed
    sample_weights = True       # plan.forward / backward draw w = mu + softplus(rho) eps (False: w = mu, the point-weight siblings)
    shared_gt = True            # psnr(gt) takes one [H, W] ground truth for all rows
    row_name = "fit"            # what to_engine calls a row when it refuses one
    tv_weights = None           # per-row weights of the total-variation term (tv.check_tv); None or all 0: the term does not exist
    tv_beta = 0.5
    _tv = None

    def _allocate(self, n_rows, rows_per_launch, K, H, W, C_out, input_depth, net_kwargs, seed, init, autotune):
        """Everything a batch of n_rows rows holds on the device, rows_per_launch of them per set of launches; then init_params(), the
        tilings, and fits mode on."""
        import torch
        self.torch = torch
        self.n_rows, self.K, self.H, self.W, self.C = int(n_rows), int(K), H, W, int(C_out)
        self.seed, self.input_depth, self.init = int(seed), int(input_depth), init
        R, F, K = self.n_rows, int(rows_per_launch), self.K
        self.prog, self.zin, self.zout, self.names = skip_program(H, W, input_depth, self.C, **net_kwargs)
        P = self.prog
        self.n = F * K
        self.plan = P.compile(self.zin, self.zout, self.n)
        self._check_plan()
        self.n_vi, self.n_bn = P.n_vi, P.n_bn
        self.n_params = 2 * P.n_vi + P.n_bn
        self.stride = (self.n_params + 3) // 4 * 4                   # row stride of params / m / v / grads: every row's MU block 16-byte aligned
        dev = "cuda"
        self._pbuf = torch.zeros((R, self.stride), dtype=torch.float32, device=dev)
        self._mbuf = torch.zeros_like(self._pbuf); self._vbuf = torch.zeros_like(self._pbuf)
        self.params, self.m, self.v = self._pbuf[:, :self.n_params], self._mbuf[:, :self.n_params], self._vbuf[:, :self.n_params]
        # gradients and the float64 data-term accumulators of ALL rows in one allocation: one fill launch clears both per iteration (the
        # generic kernels accumulate into the rows by atomics, so the rows must start from zero)
        tv_on = self.tv_weights is not None and any(w > 0.0 for w in self.tv_weights)      # its accumulators [n_rows] behind the data term's
        self._gbuf = torch.zeros(4 * R * self.stride + 8 * R * (2 if tv_on else 1), dtype=torch.uint8, device=dev)
        self._grows = self._gbuf[:4 * R * self.stride].view(torch.float32).view(R, self.stride)
        self.grads = self._grows[:, :self.n_params]
        self.nll_acc = self._gbuf[4 * R * self.stride:4 * R * self.stride + 8 * R].view(torch.float64)
        if tv_on:
            from .tv import TvTerm
            self._tv = TvTerm(self.tv_weights, self.tv_beta, F, K, H, W, acc=self._gbuf[4 * R * self.stride + 8 * R:].view(torch.float64))
        self.dead_dev = torch.zeros(R, dtype=torch.int32, device=dev)
        self.z0 = torch.empty((R, input_depth, H, W), dtype=torch.float32, device=dev)
        # what one group needs, shared by the groups like the plan's workspace
        self.z = torch.empty((F, input_depth, H, W), dtype=torch.float32, device=dev)
        self.out = torch.empty((self.n, self.C, H, W), dtype=torch.float32, device=dev)
        self.dout = torch.empty_like(self.out)
        self.ema = torch.zeros((R, self.C, H, W), dtype=torch.float32, device=dev)
        self.t = 0
        self._ema_n = 0                  # EMA updates so far (the first one copies)
        self._side = None; self._ema_done = None
        self.groups = groups(R, F, K)
        self._alloc_own()
        self.init_params()
        if autotune:                     # before the mode is switched on (tilings do not depend on it), with row 0's parameters and input
            f0 = self.fit(0)
            self.plan.autotune(f0["mu"], f0["rho"], f0["bn"], self.z0[0], self.n)
        self.plan.set_fits(K, self.stride, self.stride)

    def _check_plan(self):
        """Refuse a compiled plan (self.plan) before anything is allocated for it."""

    def _alloc_own(self):
        """The class's own device state; everything init_params() and its hooks read exists when this returns."""

    # -------------------------------------------------------------------------------------------
    def fit(self, f):
        """Views of row f: dict(mu, rho, bn, params, m, v, grads, z0, ema)."""
        n = self.n_vi
        p = self._pbuf[f]
        return dict(mu=p[:n], rho=p[n:2 * n], bn=p[2 * n:self.n_params], params=p[:self.n_params], m=self._mbuf[f, :self.n_params],
                    v=self._vbuf[f, :self.n_params], grads=self._grows[f, :self.n_params], z0=self.z0[f], ema=self.ema[f])

    def init_params(self):
        """Per row f as the standalone engine's init_params with sample f of its streams (init='shared': every row starts from row 0's)."""
        n = self.n_vi
        self._pbuf.zero_()
        for f in range(self.n_rows if self.init == "per_fit" else 1):
            self._fill_row(f)
        for b in self.prog.bns:
            self._pbuf[:, 2 * n + b["off"]:2 * n + b["off"] + b["C"]] = 1.0
        if self.init == "shared":
            self._pbuf[1:] = self._pbuf[:1]; self.z0[1:] = self.z0[:1]
        self._mbuf.zero_(); self._vbuf.zero_(); self.dead_dev.zero_(); self.t = 0; self._ema_n = 0
        self._after_init()

    def _fill_row(self, f):
        """mu, rho and z0 of row f as ElboEngine.init_params fills them, with sample f of the INIT / z0 streams."""
        lib, sp = L.lib(), L.stream_ptr()
        n, p = self.n_vi, self._pbuf[f]
        L.check(lib.mfvi_normal_fill(self.seed, L.DOMAIN_INIT, 0, f, 0, n, 0.0, 0.1, L.ptr(p), sp))
        L.check(lib.mfvi_normal_fill(self.seed, L.DOMAIN_INIT, 1, f, 0, n, -3.0, 0.1, L.ptr(p[n:]), sp))
        L.check(lib.mfvi_uniform_fill(self.seed, 0, f, 0, self.z0[f].numel(), 0.1, L.ptr(self.z0[f]), sp))

    def _after_init(self):
        """What init_params() resets besides the rows."""

    # -------------------------------------------------------------------------------------------
    def _wait_ema(self):
        if self._ema_done is not None:
            self.torch.cuda.current_stream().wait_event(self._ema_done)

    def _ema(self, d0, nd):
        """The smoothed outputs of the group's rows from self.out, on a second stream behind the forward and beside the backward pass."""
        t = self.torch
        if self._side is None:
            self._side = t.cuda.Stream(); self._ema_done = t.cuda.Event()
        ready = t.cuda.Event(); ready.record(t.cuda.current_stream())
        with t.cuda.stream(self._side):
            self._side.wait_event(ready)
            if self._book is None:
                self._ema_launch(d0, nd)
            else:                        # the same EMA from mfvi_bookkeep_fits; behind the last group, the iteration's records of every row
                self._book.group(self.out, d0, nd, self.K, self._ema_n == 0)
                if d0 + nd == self.n_rows:
                    self._book.finish()
            self._ema_done.record(self._side)

    def _ema_launch(self, d0, nd):
        L.check(L.lib().mfvi_ema_fits(L.ptr(self.out), nd, self.K, self.C, self.H, self.W, L.ptr(self.ema[d0:]), EXP_WEIGHT, int(self._ema_n == 0),
                                      L.stream_ptr()))

    def track(self, gt, num_iter, noisy=None):
        """Record what the single-fit runner records per iteration, for every row -> the BatchBook; step() then
        runs its iteration where the EMA runs.  gt: [n_rows, H, W], or one [H, W] for all; noisy: denoising only (both 'corrupted'
        columns of the CT runner are against the ground truth)."""
        from .batchbook import BatchBook
        return BatchBook(self, num_iter, gt, noisy)

    def metrics(self, gt):
        """dict(psnr=[n_rows], ssim=[n_rows]) of recon() against the ground truth ([H, W] shared, or [n_rows, H, W]), one mfvi_pair_metrics
        call."""
        from .batchbook import recon_metrics
        return recon_metrics(self, gt)

    def grad_only(self, step=None, perturb=True, ema=False):
        """Everything of one iteration except the update, group by group: grads [n_rows, n_params] and the accumulator [n_rows] hold the
        result (no KL term)."""
        self._require_targets()
        lib, sp = L.lib(), L.stream_ptr()
        step = self.t if step is None else int(step)
        nv, sw = self.n_vi, self.sample_weights
        self._gbuf.zero_()
        for d0, nd, k0, fit0, n in self.groups:
            if perturb:
                zsrc = self.z[:nd]
                L.check(lib.mfvi_perturb_input_fits(L.ptr(self.z0[d0:]), self.seed, step, self.z0[0].numel(), nd, fit0, 0.1, L.ptr(zsrc), sp))
            else:
                zsrc = self.z0[d0:d0 + nd]
            self._wait_ema()             # the EMA of the previous group (or iteration) has read self.out
            p, g = self._pbuf[d0], self._grows[d0]
            mu, rho, bn = p[:nv], p[nv:], p[2 * nv:]
            out, dout = self.out[:n], self.dout[:n]
            self.plan.forward(mu, rho, bn, zsrc, self.seed, step, k0, n, sw, out)
            self._data_term(d0, nd, out, dout)
            if self._tv is not None:     # dout[:, 0] += tv_weight[row] / K * dTV/dout[:, 0]; the rows' TV sums
                self._tv.add(out, dout, d0, nd, self.K, 1.0 / self.K)
            if ema:
                self._ema(d0, nd)
            self.plan.backward(mu, rho, bn, zsrc, self.seed, step, k0, n, dout, g[:nv], g[nv:], g[2 * nv:], sw)
        if ema:
            self._ema_n += 1

    def _pre_step(self):
        """What step() launches ahead of the iteration."""

    def step(self):
        """One iteration of every row.  A row whose data term is not finite keeps its parameters and moments and is marked dead (sticky);
        the reference's CT loop instead skips that one update (`if not torch.isnan(loss)`, bayesian_optimization.py:581-582)."""
        self._pre_step()
        self.grad_only(self.t, ema=True)
        self.t += 1
        self._update()

    # -------------------------------------------------------------------------------------------
    @property
    def dead(self):
        """[n_rows] int32: 1 for a row that met a non-finite data term (sticky; its parameters stopped there)."""
        return self.dead_dev.cpu().numpy()

    def tv(self):
        """[n_rows]: mean over a row's K samples of TV_beta(out_k[0]) at the last grad_only / step (zeros when no row has a weight: the
        term did not run) -- forces a device sync.  A row's share of its objective is tv_weight[row] * tv()[row]; losses() leaves it out."""
        import numpy as np
        if self._tv is None:
            return np.zeros(self.n_rows)
        return self._tv.acc.cpu().numpy() / self.K

    def _tv_kw(self, f):
        """The keywords that hand row f's term to its standalone engine."""
        return dict(tv_weight=self.tv_weights[f], tv_beta=self.tv_beta) if self.tv_weights is not None else {}

    def _kl_kw(self, f):
        """The keywords that hand row f's direction of the KL term, and its scale-mixture prior if it has one, to its standalone engine (none
        where the class has no KL term)."""
        kl, pm = getattr(self, "kl_types", None), getattr(self, "prior_mixtures", None)
        kw = dict(kl_type=kl[f]) if kl is not None else {}
        if pm is not None and pm[f] is not None:
            kw["prior_mixture"] = {k: pm[f][k] for k in ("pi", "sigma", "mu")}
        return kw

    def recon(self):
        """clip(ema[:, 0], 0, 1) [n_rows, H, W]: the smoothed reconstruction of every row."""
        self._wait_ema()
        return self.ema[:, 0].clamp(0.0, 1.0).contiguous()

    def psnr(self, gt):
        """[n_rows]: PSNR of clip(ema[:, 0], 0, 1) against the ground truth ([n_rows, H, W]; one [H, W] for all where the class takes it)
        -- per row the psnr_gt_sm the reference returns to its search (bayesian_optimization.py:1400-1403, :1436; :1220-1223, :1237)."""
        import numpy as np
        torch, lib, sp = self.torch, L.lib(), L.stream_ptr()
        R, H, W = self.n_rows, self.H, self.W
        g = torch.as_tensor(gt).float().cuda()
        if self.shared_gt and g.dim() == 2:
            g = g[None].expand(R, -1, -1)
        if tuple(g.shape) != (R, H, W):
            raise ValueError("ground truth of shape %s, expected %s" % (tuple(g.shape), (R, H, W)))
        g = g.contiguous()
        rec = self.recon()
        acc = torch.zeros(R, dtype=torch.float64, device="cuda")
        for f in range(R):
            L.check(lib.mfvi_sq_err_sum(L.ptr(g[f]), L.ptr(rec[f]), H * W, L.ptr(acc[f:]), sp))
        mse = acc.cpu().numpy() / float(H * W)
        with np.errstate(divide="ignore"):
            return 10.0 * np.log10(1.0 / mse)

    def _snr_select(self):
        """The batch's SnrSelect over all rows (prune.py), allocated on first use; the point-weight siblings are refused before the library is touched."""
        from . import prune as P
        P.check_batch(self)
        return P.owner_select(self, self.n_rows, self.stride, self.n_params)

    def snr(self):
        """float32 [n_rows, n_vi] on the device: |mu| / softplus(rho) of every row's posterior, one launch."""
        return self._snr_select().compute_keys(self._pbuf)

    def prune_mask(self, amount):
        """Per row what ElboEngine.prune_mask returns (a list of n_rows dicts), the selection of all rows in one set of launches.  amount: a
        share in [0, 1], or one per row."""
        from . import prune as P
        P.check_batch(self)
        a = P.check_amount(amount, self.n_rows)
        sel = self._snr_select()
        return sel.info(sel.select(self._pbuf, a), a)

    def predict(self, n_samples, target=None, clip=False, step=None, chunk=None, fits_per_call=None, calibration=None, prune=None):
        """Posterior predictive maps of every row at once (batchpredict.predict_fits): per row what
        to_engine(f).predict(n_samples, ...) returns, stacked, from one set of launches per chunk of draws instead of one chain per row.
        prune: a share in [0, 1] or one per row: keys, selection and the pruned clone of ALL rows in one set of launches, the prediction
        reads the clone, r["prune"] is the list of per-row prune_mask dicts without their masks; _pbuf is untouched.  None, 0 or all 0:
        no pruning code runs."""
        from .batchpredict import predict_fits
        pbuf = info = None
        if prune is not None:
            from . import prune as P
            a = P.check_amount(prune, self.n_rows)
            if any(a):
                sel = self._snr_select()
                ks = sel.select(self._pbuf, a)
                pbuf, info = sel.apply(self._pbuf).view(self.n_rows, self.stride), sel.info(ks, a, with_mask=False)
        r = predict_fits(self, n_samples, target=target, clip=clip, step=step, chunk=chunk, fits_per_call=fits_per_call, calibration=calibration, pbuf=pbuf)
        if info is not None:
            r["prune"] = info
        return r

    def to_engine(self, f, autotune=False):
        """The standalone engine of the class holding copies of row f's parameters, Adam moments, step count, input and target: predict(),
        calibration and the single-fit runner then work on any row of a batch.  (Continued alone it draws the global samples 0 .. K - 1 and
        sample 0 of the per-row streams, not row f's.)"""
        if not 0 <= f < self.n_rows:
            raise ValueError("%s %r outside 0..%d" % (self.row_name, f, self.n_rows - 1))
        eng = self._make_engine(f, autotune)
        v = self.fit(f)
        eng.params.copy_(v["params"]); eng.m.copy_(v["m"]); eng.v.copy_(v["v"]); eng.z0.copy_(v["z0"])
        eng.t = self.t; eng.t_applied.fill_(self.t)
        self._hand_target(eng, f)
        return eng


class ElboRowBatch(RowBatch):
    """The mean-field VI layer: per-row temp / prior sigma / lr / direction of the KL term, the KL term and Adam in one launch over all rows.
    The subclass sets temps, sigmas, lrs (its check_args) and kl_types (check_kl_type) before _allocate."""
    kl_types = None             # per row 'reverse' or 'forward' 
    prior_mixtures = None       # per row a checked scale-mixture prior or None
    _mix_dev = None             # mfvi_mixture_prior[n_rows] on the device once a row has a mixture; none has: nothing, and the library runs the typed update
    _kl_dev = None              # the directions on the device (int32 [n_rows]) once a row is forward; all reverse: nothing, and the library runs the untyped update

    def _alloc_own(self):
        import numpy as np
        torch, R = self.torch, self.n_rows
        self.prior_sigma = prior_sigmas(self.temps, self.sigmas)
        self.kl = torch.zeros(R, dtype=torch.float64, device="cuda")
        self.hyper = torch.tensor(np.array([[0.0, ps, t, r] for ps, t, r in zip(self.prior_sigma, self.temps, self.lrs)], np.float32), device="cuda")   # mfvi_fit_hyper[n_rows]
        self.upd_scratch = torch.zeros(L.lib().mfvi_elbo_update_fits_scratch_bytes(R), dtype=torch.uint8, device="cuda")
        if self.kl_types is None:
            self.kl_types = ["reverse"] * R
        if any(k != "reverse" for k in self.kl_types):
            self._kl_dev = torch.tensor([KL_TYPES.index(k) for k in self.kl_types], dtype=torch.int32, device="cuda")
        if self.prior_mixtures is None:
            self.prior_mixtures = [None] * R
        if any(pm is not None for pm in self.prior_mixtures):      # a Gaussian row is the n == 0 entry
            table = b"".join(bytes(mixture_struct(pm)) for pm in self.prior_mixtures)
            self._mix_dev = torch.frombuffer(bytearray(table), dtype=torch.uint8).cuda()

    def _update(self):
        # one entry for every batch: a NULL prior table is the typed update, a NULL direction table the all-reverse one (the library delegates).
        # A row on a mixture draws with sample r at counter word t - 1, the iteration just run (what its standalone engine draws with sample 0)
        L.check(L.lib().mfvi_elbo_update_fits_mixture(L.ptr(self._pbuf), L.ptr(self._grows), L.ptr(self._mbuf), L.ptr(self._vbuf), self.n_vi, self.n_bn,
                                                      self.stride, self.stride, self.n_rows, L.ptr(self.hyper), L.ptr(self._kl_dev), L.ptr(self._mix_dev),
                                                      self.seed, 0, self.t - 1, None, 0.9, 0.999, 1e-8, self.t, L.ptr(self.nll_acc), L.ptr(self.dead_dev),
                                                      L.ptr(self.kl), L.ptr(self.upd_scratch), L.stream_ptr()))

    def losses(self):
        """(nll[n_rows], kl[n_rows], loss[n_rows]) of the last step (kl: of the parameters that step started from, in the row's direction) -- forces a device sync.
        After grad_only alone kl is stale: the KL term is part of the update launch."""
        import numpy as np
        nll = self.nll_acc.cpu().numpy() / self.K
        kl = self.kl.cpu().numpy()
        return nll, kl, nll + np.asarray(self.temps) * kl
