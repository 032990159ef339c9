"""The slices of a sparse-view CT volume fitted in one set of launches.

The reference fits a CT stack as one run_ct_mfvi process per slice (bayesian_optimization.py:442-648), each iteration a chain of small
K = 1 launches.  A CtVolume of D slices holds one parameter / moment / gradient row per slice, laid out as FitBatch lays out its rows, and
ONE plan of F * K samples in fits mode (F = slices_per_launch).  The slices advance in groups of F through that plan and its workspace --
a stack of 100 slices does not fit one launch set's activations --, the last group with what is left.  One iteration is the group loop of rowbatch.py
(per group: perturb with fit0 = g F, forward with k0 = g F K, data term, EMA with C = 1 on a second stream beside the backward pass, backward)
with

    nll[d] = 1/K sum_k mean((R out[d, k] - sino[d])^2)                                 (mfvi_radon_mse_fits)

as its data term, and one update launch over all D rows closes it (KL[d], Adam with temp[d], prior_sigma[d], lr[d]).  RNG identity: slice d
owns the global eps samples d * K .. d * K + K - 1 and sample d of the INIT, z0 and perturbation streams whatever slices_per_launch is, so
slice 0 is ElboEngine(S, S, task="ct", seed, K)."""
from . import _lib as L
from .rowbatch import MAX_LAUNCH, ElboRowBatch, check_kl_type, check_prior_mixtures, groups, per_fit      # (groups and MAX_LAUNCH re-exported: their home is rowbatch.py)


def check_args(S, n_slices, slices_per_launch, K, temp, sigma, lr, theta_deg, init):
    """Everything that can be refused without the library; -> (S, F, temps, sigmas, lrs, theta list)."""
    try:
        H, W = S
    except TypeError:
        H = W = S
    if H != W:
        raise ValueError("size %r: the Radon operator takes square slices" % (S,))
    H = int(H)
    if H < 1 or H % 4:
        raise ValueError("S=%r: a multiple of 4 (the input-scale layers run on the matrix-core kernels)" % (S,))
    if int(n_slices) < 1 or int(n_slices) > MAX_LAUNCH:
        raise ValueError("n_slices=%r: 1 .. %d" % (n_slices, MAX_LAUNCH))
    if int(K) < 1:
        raise ValueError("K=%r: at least 1" % (K,))
    if slices_per_launch is not None and int(slices_per_launch) < 1:
        raise ValueError("slices_per_launch=%r: None (all slices) or at least 1" % (slices_per_launch,))
    D = int(n_slices)
    F = min(int(slices_per_launch) if slices_per_launch else D, D)
    if F * int(K) > MAX_LAUNCH:
        raise ValueError("slices_per_launch * K = %d * %d: below 65536 samples per launch" % (F, K))
    if init not in ("per_fit", "shared"):
        raise ValueError("init %r: 'per_fit' or 'shared'" % (init,))
    temps, sigmas, lrs = per_fit(temp, D, "temp"), per_fit(sigma, D, "sigma"), per_fit(lr, D, "lr")
    if any(not t >= 0.0 for t in temps) or any(not s >= 0.0 for s in sigmas) or any(not r > 0.0 for r in lrs):
        raise ValueError("temp and sigma must be >= 0 and lr > 0 for every slice")
    theta = [float(t) for t in (range(0, 180, 4) if theta_deg is None else theta_deg)]      # bayesian_optimization.py:545
    if not theta or len(theta) > 32768:
        raise ValueError("theta_deg: 1 .. 32768 angles, got %d" % len(theta))
    return H, F, temps, sigmas, lrs, theta


class CtVolume(ElboRowBatch):
    """The ElboRowBatch whose rows are slices and whose groups are more than one: rowbatch.py runs the iteration; here are the angles, the
    sinograms, the Radon data term and the engine of one slice."""
    task = "ct"
    shared_gt = False           # psnr(gt) takes the stack
    row_name = "slice"
    sinos = None

    def __init__(self, S, n_slices, slices_per_launch=None, K=1, input_depth=16, temp=1.0, sigma=0.1, lr=1e-3, theta_deg=None, seed=1,
                 net_kwargs=None, init="per_fit", autotune=True, tv_weight=0.0, tv_beta=0.5, kl_type="reverse", prior_mixture=None):
        self.S, self.F, self.temps, self.sigmas, self.lrs, self.theta_list = check_args(S, n_slices, slices_per_launch, K, temp, sigma, lr,
                                                                                        theta_deg, init)
        self.D, self.T = int(n_slices), len(self.theta_list)
        self.kl_types = check_kl_type(kl_type, self.D)      # a name, or one per slice
        self.prior_mixtures = check_prior_mixtures(prior_mixture, self.kl_types)      # None, one scale-mixture prior, or one per slice (None: a Gaussian slice)
        from .tv import check_tv
        self.tv_weights, self.tv_beta = check_tv(tv_weight, tv_beta, "ct", n=self.D)      # a scalar, or one weight per slice
        self.net_kwargs = dict(net_kwargs or {})
        self._allocate(self.D, self.F, K, self.S, self.S, 1, input_depth, self.net_kwargs, seed, init, autotune)      # the CT net: n_channels = 1

    def _alloc_own(self):
        super()._alloc_own()
        torch = self.torch
        self.theta = torch.tensor(self.theta_list, dtype=torch.float32, device="cuda")
        self.ct_scratch = torch.empty(L.lib().mfvi_radon_mse_fits_scratch_bytes(self.F, self.K, self.S, self.T), dtype=torch.uint8, device="cuda")

    def set_sinograms(self, sinos):
        """The measured sinograms [D, T, S], one per slice."""
        s = self.torch.as_tensor(sinos)
        if tuple(s.shape) != (self.D, self.T, self.S):
            raise ValueError("sinograms of shape %s, expected %s" % (tuple(s.shape), (self.D, self.T, self.S)))
        self.sinos = s.contiguous().float().cuda()

    def set_volume(self, volume):
        """The sinograms of a ground-truth stack [D, S, S] by mfvi_radon_project, as the reference makes img_radon
        (bayesian_optimization.py:547)."""
        torch = self.torch
        v = torch.as_tensor(volume)
        if tuple(v.shape) != (self.D, self.S, self.S):
            raise ValueError("volume of shape %s, expected %s" % (tuple(v.shape), (self.D, self.S, self.S)))
        v = v.contiguous().float().cuda()
        sinos = torch.empty((self.D, self.T, self.S), dtype=torch.float32, device="cuda")
        L.check(L.lib().mfvi_radon_project(L.ptr(v), L.ptr(self.theta), self.D, self.S, self.T, L.ptr(sinos), L.stream_ptr()))
        self.sinos = sinos

    def _require_targets(self):
        if self.sinos is None:
            raise ValueError("set_sinograms or set_volume first")

    def _data_term(self, d0, nd, out, dout):
        L.check(L.lib().mfvi_radon_mse_fits(L.ptr(out), L.ptr(self.sinos[d0:]), self.T * self.S, L.ptr(self.theta), nd, self.K, self.S, self.T,
                                            1.0 / self.K, L.ptr(self.ct_scratch), L.ptr(dout), L.ptr(self.nll_acc[d0:]), L.stream_ptr()))

    def _make_engine(self, d, autotune):
        from .engine import ElboEngine
        return ElboEngine(self.S, self.S, task="ct", K=self.K, input_depth=self.input_depth, temp=self.temps[d], sigma=self.sigmas[d],
                          lr=self.lrs[d], seed=self.seed, theta_deg=self.theta_list, net_kwargs=self.net_kwargs, autotune=autotune, **self._tv_kw(d), **self._kl_kw(d))

    def _hand_target(self, eng, d):
        if self.sinos is not None:
            eng.set_target(self.sinos[d].clone())
