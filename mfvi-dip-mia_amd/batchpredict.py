"""Posterior predictive maps of every fit of a batch in one set of launches.

FitBatch, CtVolume, InpaintBatch and SiblingBatch (MC dropout) share the layout this needs: the parameter rows _pbuf [F, stride], the layer
program, the unperturbed inputs z0 [F, Cin, H, W].  Per group of G fits a forward-only plan of G * S samples in fits mode draws S samples
of every fit per call, with the sample stride 0 (mfvi_plan_set_fits_sample_stride): fit f's draw s of chunk c is the global sample
c * S + s of the batch's seed at the prediction's RNG step -- the sample to_engine(f).predict(N) draws, whatever S and G are.  The draws
fold into one fp64 accumulator row per fit (mfvi_predictive_accumulate_fits) and become the maps in two launches
(mfvi_predictive_finalize_fits).  The calibration statistics, when asked for, loop over the fits (calibration.calibration: a few small
launches and one host sync per fit); they are not batched."""
from . import _lib as L
from .predictive import DEFAULT_STEP, image_channels, mode_code

MAX_WORKSPACE_SAMPLES = 64      # default S = max(1, min(N, 64 // G)): the prediction plan's workspace holds at most 64 samples


def n_fits_of(owner):
    """Fits of a batch: its rows (the D slices of a CtVolume, whose F is the slices per launch)."""
    return int(owner.n_rows)


def task_of(owner):
    return owner.task


def plan_chunks(n_fits, n_samples, fits_per_call, chunk):
    """The calls of one prediction, in order: (g0, G, c, n_use) = fits g0 .. g0 + G - 1 draw the samples c * chunk .. c * chunk + n_use - 1.
    The last group holds n_fits % fits_per_call fits, the last chunk of a group n_samples % chunk samples, when those are not 0."""
    calls = []
    for g0 in range(0, n_fits, fits_per_call):
        G = min(fits_per_call, n_fits - g0)
        for c, k in enumerate(range(0, n_samples, chunk)):
            calls.append((g0, G, c, min(chunk, n_samples - k)))
    return calls


def check_args(owner, n_samples, target=None, step=None, chunk=None, fits_per_call=None, calibration=None):
    """Everything predict_fits refuses, without the library -> (N, S, G, step, calibration dict | None, target shape kind).
    The kind is None, "shared" (one ground truth for all fits) or "per_fit"."""
    method = getattr(owner, "method", None)
    if method == "dip":
        raise ValueError("the plain deep image prior (method 'dip') is deterministic: there is no posterior to sample")
    if method == "sgld":
        raise NotImplementedError("SGLD's posterior samples are its iterates (the runner's ring buffer), not draws of one network")
    F, N = n_fits_of(owner), int(n_samples)
    cal = None
    if calibration is not None and calibration is not False:
        cal = {} if calibration is True else dict(calibration)
        if set(cal) - {"n_bins", "range"}:
            raise ValueError("calibration=%r: True or a dict with n_bins and range" % (calibration,))
        if target is None:
            raise ValueError("calibration compares the uncertainty with the error against a ground truth: pass target")
    if N < 2:
        raise ValueError("posterior predictive statistics need at least 2 samples, got n_samples=%d" % N)
    G = int(fits_per_call) if fits_per_call is not None else min(F, int(owner.F))
    if not 1 <= G <= F:
        raise ValueError("fits_per_call=%r outside 1..%d" % (fits_per_call, F))
    S = int(chunk) if chunk is not None else max(1, min(N, MAX_WORKSPACE_SAMPLES // G))
    if S < 1:
        raise ValueError("chunk=%d" % S)
    if G * S > 65535:
        raise ValueError("fits_per_call * chunk = %d: below 65536" % (G * S))
    step = DEFAULT_STEP if step is None else int(step)
    if not 0 <= step < 2 ** 32:
        raise ValueError("step %d outside the 32-bit counter word" % step)
    kind = None
    if target is not None:
        H, W = owner.H, owner.W
        cimg = 3 if task_of(owner) == "inp" else 1
        shape = tuple(target.shape)
        shared = [(cimg, H, W)] + ([(H, W)] if cimg == 1 else [])
        per_fit = [(F, cimg, H, W)] + ([(F, H, W)] if cimg == 1 else [])
        if shape in shared:
            kind = "shared"
        elif shape in per_fit:      # (F == Cimg == 1 and [1, H, W]: the same array either way)
            kind = "per_fit"
        else:
            raise ValueError("target of shape %s, expected %s shared by the fits or %s" % (shape, " / ".join(map(str, shared)), " / ".join(map(str, per_fit))))
    return N, S, G, step, cal, kind


def _group_plan(owner, G, S):
    """The forward-only plan of G fits x S samples (cached on the batch): its own workspace, sampled-weight slab and output buffer, so a
    prediction never touches the training plan's state or the batch's out."""
    cache = owner.__dict__.setdefault("_predict_plans", {})
    if (G, S) not in cache:
        torch = owner.torch
        plan = owner.prog.compile(owner.zin, owner.zout, G * S)
        if getattr(owner.plan, "tuned", False):      # as the training plan: before the mode is switched on, with fit 0's parameters and input
            nv = owner.n_vi
            p = owner._pbuf[0]
            plan.autotune(p[:nv], p[nv:2 * nv], p[2 * nv:owner.n_params], owner.z0[0], G * S)
        plan.set_fits(S, owner.stride, 0)
        plan.set_fits_sample_stride(0)
        if getattr(owner, "method", None) is not None:
            plan.set_fits_points(True)
        out = torch.empty((G * S,) + plan.out_shape, dtype=torch.float32, device="cuda")
        cache[(G, S)] = (plan, out)
    return cache[(G, S)]


def predict_fits(owner, n_samples, target=None, clip=False, step=None, chunk=None, fits_per_call=None, calibration=None, pbuf=None):
    """N posterior draws of EVERY fit of the batch, reduced on the device ->
        dict(mean [F,Cimg,H,W], epi, ale | None, total, err2 | None, mse_mc | None [F,H,W], psnr_mean [F] | None, dead [F], n, step)
    fit f's maps being those of owner.to_engine(f).predict(n_samples, ...) up to the order of the convolutions' sums: the same global
    samples 0 .. N-1 of the batch's seed at RNG step `step` (default predictive.DEFAULT_STEP), the unperturbed z0, the task's transform
    (den / sr logprec, inp inp, ct mean_only).  target: the clean image, [H,W] / [Cimg,H,W] shared by the fits or one per fit; gives err2,
    mse_mc and psnr_mean = 10 log10(1 / mean err2).  chunk: samples per fit and call (default max(1, min(N, 64 // G)));
    fits_per_call: G (default every fit; CtVolume: its slices per launch).  A dead fit is predicted from its frozen parameters and
    flagged in `dead`.  calibration: True or dict(n_bins, range) adds r["calibration"], one Calibration per fit.
    pbuf: parameter rows [F, stride] to predict from in place of the batch's own (RowBatch.predict(prune=): the pruned clone).
    Leaves the training plan, out, the parameters, the moments and the counters untouched."""
    import numpy as np
    N, S, G, step, cal, kind = check_args(owner, n_samples, target, step, chunk, fits_per_call, calibration)
    torch, lib, sp = owner.torch, L.lib(), L.stream_ptr()
    F, task = n_fits_of(owner), task_of(owner)
    mode = {"ct": "mean_only", "inp": "inp"}.get(task, "logprec")
    plan, out = _group_plan(owner, G, S)
    C, H, W = plan.out_shape
    code = mode_code(mode)
    cimg, has_ale = image_channels(C, mode)
    HW = H * W
    acc_stride = int(lib.mfvi_predictive_acc_doubles_fits(C, H, W, code))
    if acc_stride < 0:
        raise ValueError("predictive mode %r does not take %d output channels" % (mode, C))
    ref, ref_stride = None, 0
    if kind is not None:
        ref = torch.as_tensor(target).to(device="cuda", dtype=torch.float32).contiguous()
        ref_stride = cimg * HW if kind == "per_fit" else 0
    acc = torch.empty((F, acc_stride), dtype=torch.float64, device="cuda")
    sample_weights = getattr(owner, "method", None) is None      # the MC-dropout sibling runs w = mu under its masks
    ps = getattr(owner, "dropout_ps", None) if getattr(owner, "plan_p", 0.0) > 0.0 else None
    nv = owner.n_vi
    group = None
    for g0, Gn, c, n_use in plan_chunks(F, N, G, S):
        if ps is not None and group != (g0, Gn):      # a host array copied by the call: once per group
            plan.set_fit_dropout(ps[g0:g0 + Gn])
        group = (g0, Gn)
        p = (owner._pbuf if pbuf is None else pbuf)[g0]
        plan.forward(p[:nv], p[nv:], p[2 * nv:], owner.z0[g0:g0 + Gn], owner.seed, step, c * S, Gn * S, sample_weights, out[:Gn * S])
        L.check(lib.mfvi_predictive_accumulate_fits(L.ptr(out), Gn, S, n_use, C, H, W, code, int(bool(clip)), int(c == 0), L.ptr(acc[g0]), acc_stride, sp))
    maps = torch.empty((cimg + 5) * F * HW, dtype=torch.float32, device="cuda")
    mean = maps[:F * cimg * HW].view(F, cimg, H, W)
    epi, ale, total, err2, mse_mc = (maps[(cimg + i) * F * HW:(cimg + i + 1) * F * HW].view(F, H, W) for i in range(5))
    sums = torch.empty((F, 4), dtype=torch.float64, device="cuda")
    L.check(lib.mfvi_predictive_finalize_fits(L.ptr(acc), acc_stride, F, N, C, H, W, code, L.ptr(ref), ref_stride, L.ptr(mean), L.ptr(epi),
                                              L.ptr(ale) if has_ale else None, L.ptr(total), L.ptr(err2) if ref is not None else None,
                                              L.ptr(mse_mc) if ref is not None else None, L.ptr(sums), sp))
    r = dict(mean=mean, epi=epi, ale=ale if has_ale else None, total=total, err2=err2 if ref is not None else None,
             mse_mc=mse_mc if ref is not None else None, psnr_mean=None, dead=owner.dead, n=N, step=step)
    if ref is not None:
        with np.errstate(divide="ignore"):
            r["psnr_mean"] = 10.0 * np.log10(1.0 / (sums[:, 3].cpu().numpy() / float(HW)))
    if cal is not None:
        from .calibration import calibration as _calibration
        r["calibration"] = [_calibration(mse_mc[f], total[f], n_bins=cal.get("n_bins", 15), range=cal.get("range")) for f in range(F)]
    return r
