"""Task runners: the reference's run_{den,sr,ct,inp}_mfvi loops (bayesian_optimization.py:1240-1444, 2048-2263, 442-648, 2892-3114)
and their non-Bayesian siblings run_{den,sr,ct,inp}_{dip,mcd,sgld} (:261-439, 651-1237, 1447-2045, 2266-2692, 3117-3544)
on the fused engine, producing the same artefacts (`save.npz` with the dict-of-'mfvi' object arrays that
eval_denoising.ipynb / eval_sr.ipynb / eval_ct.ipynb read, `locals.txt`).

MI355X-first differences (none changes a stored number's meaning):
  * the whole per-iteration bookkeeping (EMA, clip, ring buffers, 2 MSE + 3 PSNR + 3 SSIM) runs in HIP kernels that
    write into device arrays; the host reads them once at the end instead of ~10 `.item()` syncs per iteration;
  * K Monte-Carlo samples per iteration (K = 1 reproduces the reference); `out` in the bookkeeping is the sample mean;
  * images come from the caller (array / .npy / image file); the reference's data/ folder is git-ignored upstream, so a
    seeded synthetic phantom is available (`img='phantom'`).
CLI:  python -m mfvi_dip_mia_amd.runner --task denoising --bayes mfvi --config configs/mfvi_den.json [--img phantom --imsize 256 --k 16]
"""
import argparse
import json
import os
import time

import numpy as np

from . import _lib as L
from . import artifacts as A
from .book import EXP_WEIGHT, MC_ITER, _Book, _BookInp      # noqa: F401  (the bookkeeping's home is book.py; the names stay readable here)
from .engine import ElboEngine, SiblingEngine

PREDICT_METHODS = ("mfvi", "mcd")      # methods whose fit is a posterior predict_samples can draw from (engine.ElboEngine.predict)
CALIBRATION_METHODS = ("mfvi", "mcd", "sgld")      # methods whose run carries uncertainty maps to calibrate (dip has none)


def phantom(H, W, seed):
    """Seeded synthetic ground truth in [0,1]: soft ellipses, two hard bars, a faint texture."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    img = np.zeros((H, W))
    for _ in range(6):
        cx, cy = rng.uniform(-0.6, 0.6, 2); ax, ay = rng.uniform(0.1, 0.5, 2); th = rng.uniform(0, np.pi); amp = rng.uniform(0.2, 0.6)
        xr = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th); yr = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        img += amp / (1.0 + np.exp(np.minimum(((xr / ax) ** 2 + (yr / ay) ** 2 - 1.0) * 8.0, 60.0)))
    img[int(0.2 * H):int(0.25 * H), int(0.1 * W):int(0.9 * W)] += 0.3
    img[int(0.1 * H):int(0.9 * H), int(0.7 * W):int(0.74 * W)] += 0.25
    img += 0.03 * np.sin(9 * xx) * np.cos(7 * yy)
    img -= img.min(); img /= img.max()
    return img.astype(np.float32)


def _load_image(img, imsize, seed):
    if isinstance(img, np.ndarray):
        a = img.astype(np.float32)
    elif img == "phantom":
        a = phantom(imsize[0], imsize[1], seed)
    elif isinstance(img, str) and img.endswith(".npy"):
        a = np.load(img).astype(np.float32)
    elif isinstance(img, str):
        from PIL import Image
        a = np.asarray(Image.open(img).convert("L"), np.float32) / 255.0       # utils/common_utils.py:179-191
    else:
        raise FileNotFoundError("img=%r: the reference's data/ images are not distributed (git-ignored upstream); pass an array, "
                                "a path, or img='phantom'" % (img,))
    a = np.squeeze(a)
    if a.ndim != 2:
        raise ValueError("expected one grayscale image, got shape %s" % (a.shape,))
    h, w = a.shape
    return np.ascontiguousarray(a[:h - h % 32, :w - w % 32])                     # crop to a multiple of 32 (get_image: d=32)


def _make_engine(method, H, W, task, K, input_depth, temp, sigma, lr, seed, net_kwargs, sib, param_dtype="f32", **kw):
    if param_dtype != "f32":
        kw["param_dtype"] = param_dtype             # bf16 mu / rho (BASELINE configs[4]); the MFVI engines only
    if method == "mfvi":
        return ElboEngine(H, W, task=task, K=K, input_depth=input_depth, temp=temp, sigma=sigma, lr=lr, seed=seed, net_kwargs=net_kwargs, **kw)
    return SiblingEngine(H, W, method=method, task=task, K=K, input_depth=input_depth, lr=lr, seed=seed, net_kwargs=net_kwargs, **sib, **kw)


def _check_downsampler(task, method, downsampler, factor=4):
    """The SR forward operator of a run: 'nearest' everywhere; 'lanczos2' / 'lanczos3' for run_sr_mfvi."""
    if downsampler == "nearest":
        return
    from .downsampler import SUPPORT, check_geometry
    if downsampler not in SUPPORT:
        raise ValueError("downsampler=%r: 'nearest', 'lanczos2' or 'lanczos3'" % (downsampler,))
    if task != "sr" or method != "mfvi":
        raise ValueError("downsampler=%r is built for the MFVI super-resolution runner (run_sr_mfvi), not task %r / method %r"
                         % (downsampler, task, method))
    check_geometry(downsampler, factor)


def _tv_fields(tv_weight, tv_beta, task):
    """The total-variation term of a single-fit run, refused before anything is written or loaded -> the keywords
    of the engine and the extra locals.txt fields: both empty with the term off."""
    from .tv import check_tv
    w, b = check_tv(tv_weight, tv_beta, task)
    return dict(tv_weight=w, tv_beta=b) if w > 0.0 else {}


def _kl_fields(kl_type, method="mfvi", prior_mixture=None):
    """The direction of the KL term of a single-fit run and its scale-mixture prior (section 26), refused before
    anything is written or loaded -> the keywords of the engine and the extra locals.txt fields: empty with the default 'reverse' and no
    mixture."""
    from .rowbatch import check_kl_type, check_prior_mixture
    k = check_kl_type(kl_type)
    if k != "reverse" and method != "mfvi":
        raise ValueError("kl_type=%r: the direction of the KL term belongs to mean-field VI (mfvi); %r has no KL term" % (k, method))
    out = dict(kl_type=k) if k != "reverse" else {}
    pm = check_prior_mixture(prior_mixture)
    if pm is not None:
        if method != "mfvi":
            raise ValueError("prior_mixture: the prior belongs to mean-field VI (mfvi); %r has no KL term" % (method,))
        out["prior_mixture"] = {key: pm[key] for key in ("pi", "sigma", "mu")}      # (with kl_type 'reverse' the engine refuses it)
    return out


def parse_prior_mixture(text):
    """--prior-mixture PI:SIGMA[:MU],PI:SIGMA[:MU],... -> {'pi': [...], 'sigma': [...], 'mu': [...]} (ValueError on anything else)."""
    pi, sigma, mu = [], [], []
    for part in text.split(","):
        f = part.split(":")
        if len(f) not in (2, 3):
            raise ValueError("component %r: PI:SIGMA or PI:SIGMA:MU" % part)
        pi.append(float(f[0])); sigma.append(float(f[1])); mu.append(float(f[2]) if len(f) == 3 else 0.0)
    return dict(pi=pi, sigma=sigma, mu=mu)


def _mix_keys(batch):
    """What batch.npz / volume.npz record of the rows' scale-mixture priors, and only when some row has one: per row the number of components
    (0: a Gaussian row) and pi, sigma (as given), mu padded with zeros to four."""
    pms = getattr(batch, "prior_mixtures", None) or ()
    if not any(p is not None for p in pms):
        return {}
    pad = lambda p, k: (list(p[k]) + [0.0] * 4)[:4] if p is not None else [0.0] * 4
    return dict(prior_mixture_n=np.asarray([0 if p is None else len(p["pi"]) for p in pms], np.int64),
                **{"prior_mixture_" + k: np.asarray([pad(p, k) for p in pms], np.float64) for k in ("pi", "sigma", "mu")})


def _check_predict(method, predict_samples):
    if predict_samples and method not in PREDICT_METHODS:
        raise ValueError("predict_samples=%d: posterior predictive sampling needs a posterior to draw from (mfvi, mcd), not %r"
                         % (predict_samples, method))
    if predict_samples and predict_samples < 2:
        raise ValueError("predict_samples=%d: at least 2 draws" % predict_samples)


def _check_batch_predict(batch_predict_samples, batch_calibration_bins=0):
    if batch_predict_samples and batch_predict_samples < 2:
        raise ValueError("batch_predict_samples=%d: 0 (off) or at least 2 draws" % batch_predict_samples)
    if batch_calibration_bins and not batch_predict_samples:
        raise ValueError("batch_calibration_bins: the calibration of a batch is that of its posterior predictive maps (batch_predict_samples >= 2)")
    if batch_calibration_bins and not 1 <= int(batch_calibration_bins) <= L.UCE_MAX_BINS:
        raise ValueError("batch_calibration_bins=%r outside 1..%d" % (batch_calibration_bins, L.UCE_MAX_BINS))


def _batch_predict(batch, n, gt, run_dir, calibration_bins=0):
    """After the last iteration of a batch: batch.predict(n, target=gt) -> predictive_batch.npz beside batch.npz /
    volume.npz (the maps stacked over the fits, psnr_mean, n, step, dead) and, with calibration_bins > 0, calibration_batch.npz (the pred_
    block of calibration.npz for every fit, stacked along axis 0).  Returns the arrays of the first file."""
    import torch
    from . import calibration as Cb
    r = batch.predict(n, target=torch.from_numpy(np.ascontiguousarray(gt, np.float32)),
                      calibration=dict(n_bins=calibration_bins) if calibration_bins else None)
    arrs = {k: r[k].cpu().numpy() for k in ("mean", "epi", "ale", "total", "err2", "mse_mc") if r[k] is not None}
    arrs.update(psnr_mean=r["psnr_mean"], n=np.int64(r["n"]), step=np.int64(r["step"]), dead=r["dead"])
    if run_dir is not None:
        np.savez(os.path.join(run_dir, "predictive_batch.npz"), **arrs)
        if calibration_bins:
            blocks = [Cb.npz_block(c, "pred_") for c in r["calibration"]]
            np.savez(os.path.join(run_dir, "calibration_batch.npz"), **{k: np.stack([b[k] for b in blocks]) for k in blocks[0]})
    return arrs


def _check_calibration(method, calibration, n_bins=15):
    if calibration and method not in CALIBRATION_METHODS:
        raise ValueError("calibration: the uncertainty calibration error needs uncertainty maps (mfvi, mcd, sgld), not %r" % (method,))
    if calibration and not 1 <= int(n_bins) <= L.UCE_MAX_BINS:
        raise ValueError("calibration_bins=%r outside 1..%d" % (n_bins, L.UCE_MAX_BINS))


def _calibrate(run_dir, gt, recons, uncerts_epi, uncerts_ale, pred_cal, n_bins, mask=None):
    """calibration.npz.  Source ring_: the "UCE" cell of the task's evaluation notebook on the run's own arrays, on
    the GPU: errvar = mean over the last min(25, n_snap) `recons` snapshots of (recon - gt)^2 (times the mask for inpainting) against
    uncerts[-1] + uncerts_ale[-1].  Source pred_ (with predict_samples): mse_mc against total of the posterior predictive maps."""
    from . import calibration as Cb
    S = min(MC_ITER, recons.shape[0])
    err, unc = Cb.ring_inputs(recons[-S:], gt, uncerts_epi[-1], uncerts_ale[-1], mask)
    arrs = Cb.npz_block(Cb.calibration(err, unc, n_bins=n_bins), "ring_")
    if pred_cal is not None:
        arrs.update(Cb.npz_block(pred_cal, "pred_"))
    arrs["n_bins"] = np.int64(n_bins)
    if run_dir is not None:
        np.savez(os.path.join(run_dir, "calibration.npz"), **arrs)
    return arrs


def _predict(eng, n, gt, run_dir, drop_ale=False, calibration_bins=0):
    """After the last iteration: eng.predict(n, target=gt) -> predictive.npz in the run directory (when saving); returns the arrays
    (and the maps' Calibration under "_calibration" when calibration_bins > 0; popped by the caller)."""
    import torch
    r = eng.predict(n, target=torch.from_numpy(np.ascontiguousarray(gt, np.float32)),
                    calibration=dict(n_bins=calibration_bins) if calibration_bins else None)
    arrs = {k: r[k].cpu().numpy() for k in ("mean", "epi", "ale", "total", "err2", "mse_mc") if r[k] is not None and not (drop_ale and k == "ale")}
    arrs.update(n_samples=np.int64(r["n"]), step=np.int64(r["step"]))
    if run_dir is not None:
        np.savez(os.path.join(run_dir, "predictive.npz"), **arrs)
    if calibration_bins:
        arrs["_calibration"] = r["calibration"]
    return arrs


def parse_prune_amounts(text):
    """'0,0.5,0.9' -> [0.0, 0.5, 0.9] (ValueError for anything that is not a list of numbers)."""
    return [float(x) for x in str(text).split(",") if x.strip() != ""]


def _check_prune(method, predict_samples, prune_amounts):
    """The shares of --prune-amounts / run_params.prune_amounts, checked without the library -> list of floats, or None (off)."""
    if prune_amounts is None or len(prune_amounts) == 0:
        return None
    if method != "mfvi":
        raise ValueError("prune_amounts: SNR pruning ranks the posterior of mean-field VI (mfvi), not %r" % (method,))
    if not predict_samples:
        raise ValueError("prune_amounts: the pruned posterior is evaluated by its predictive maps (predict_samples >= 2)")
    from .prune import check_amount
    return [check_amount(a, name="prune_amounts") for a in prune_amounts]


def _pruning(eng, n, gt, run_dir, amounts):
    """After the last iteration: per share of `amounts` eng.predict(n, target=gt, prune=share) -> pruning.npz in the
    run directory (when saving): what was pruned, per-layer sparsity, the PSNR and mean uncertainties of the pruned posterior's predictive
    maps, and the histogram of log10(snr) of the unpruned posterior per group (weights, biases).  Returns the arrays."""
    import torch
    from . import prune as P
    target = torch.from_numpy(np.ascontiguousarray(gt, np.float32))
    infos, stats = [], []
    for a in amounts:
        r = eng.predict(n, target=target, prune=a)
        infos.append(r["prune"] if "prune" in r else {k: v for k, v in eng.prune_mask(a).items() if k != "mask"})
        with np.errstate(divide="ignore"):
            psnr = 10.0 * np.log10(1.0 / float(r["err2"].double().mean()))
        stats.append([psnr, float(r["epi"].double().mean()), float(r["ale"].double().mean()) if r["ale"] is not None else np.nan,
                      float(r["total"].double().mean())])
    sel = eng._snr_select()
    sel.compute_keys(eng.params)
    counts, edges = P.snr_histogram(sel)
    stats = np.asarray(stats, np.float64)
    arrs = dict(amount=np.asarray(amounts, np.float64), n_pruned=np.stack([i["k"] for i in infos]), n=infos[0]["n"],
                snr_threshold=np.stack([i["threshold"] for i in infos]), layer_sparsity=np.stack([i["layer_sparsity"] for i in infos]),
                layer_names=np.array(P.layer_names(eng.prog)), psnr_mean=stats[:, 0], epi_mean=stats[:, 1], ale_mean=stats[:, 2], total_mean=stats[:, 3],
                snr_hist_counts=counts[0], snr_hist_edges_log10=edges)
    if run_dir is not None:
        np.savez(os.path.join(run_dir, "pruning.npz"), **arrs)
    return arrs


def _fit(task, method, fields, prepare, num_iter, show_every, plot, save, save_path, verbose=False, predict_samples=0, calibration=False,
         calibration_bins=15, downsampler="nearest", factor=4, prune_amounts=None):
    """The loop of every single-fit runner: the refusals; the run directory and the head of locals.txt (`fields`), written
    before anything is loaded; `prepare(n_it)` -> (ground truth, engine with its target set, book, the two head arrays of save.npz, mask or
    None, channel count of recons / uncerts); the iterations with a snapshot every show_every; predictive.npz and calibration.npz; save.npz,
    the tail of locals.txt and the plots -> the dict of results.  The inpainting runner writes its snapshot PNGs once, at the end."""
    import torch
    _check_downsampler(task, method, downsampler, factor)
    _check_predict(method, predict_samples)
    _check_calibration(method, calibration, calibration_bins)
    prune_amounts = _check_prune(method, predict_samples, prune_amounts)
    run_dir = os.path.join(save_path, str(time.time()))
    if save:
        os.makedirs(run_dir, exist_ok=False)
        A.write_locals(run_dir, **fields)
    num_iter += 1                                                    # bayesian_optimization.py:1291, :2935
    gt, eng, book, head, mask, C = prepare(num_iter)
    H, W = gt.shape[-2:]

    def pngs(i, curves, recon, var, ale):      # loss_<method>.png, out_avg.png, out_var.png, out_ale.png (:1418-1422); the maps (C | 1, H, W)
        A.snapshot_pngs(run_dir, method, i, *curves, recon, None if method == "dip" else var, None if (method == "dip" or task == "ct") else ale)
    n_snap = num_iter // show_every + 1
    recons = np.zeros((n_snap, C, H, W)); uncerts_epi = np.zeros((n_snap, C, H, W)); uncerts_ale = np.zeros((n_snap, 1, H, W))
    t0 = time.perf_counter()
    for i in range(num_iter):
        # one fused ELBO iteration (a non-finite loss skips the update on the device: engine.step); the bookkeeping of :1374-1406 reads only the
        # iteration's forward output and runs on a second stream beside the backward pass
        eng.step(after_forward=book.hook(eng, i, eng.chunk))
        if i % show_every == 0:
            var, ale, recon = book.snapshot()
            uncerts_epi[i // show_every] = var; uncerts_ale[i // show_every, 0] = ale; recons[i // show_every] = recon
            if verbose:
                nll, kl, loss = eng.losses()
                tv = "  tv %.5f (weight %g)" % (eng.tv(), eng.tv_weight) if eng.tv_weight > 0.0 else ""
                print("iter %6d  loss %.5f  nll %.5f  kl %.4e%s  (%.1f it/s)" % (i, loss, nll, kl, tv, (i + 1) / (time.perf_counter() - t0)))
            if plot and save and task != "inp":
                pngs(i, book.results()[:3], recon.reshape(C, H, W), var.reshape(C, H, W), ale[None])
    pred = _predict(eng, predict_samples, gt, run_dir if save else None, drop_ale=task == "ct",
                    calibration_bins=calibration_bins if calibration else 0) if predict_samples else None
    cal = _calibrate(run_dir if save else None, gt, recons, uncerts_epi, uncerts_ale, pred.pop("_calibration") if pred else None,
                     calibration_bins, mask=mask) if calibration else None
    pruning = _pruning(eng, predict_samples, gt, run_dir if save else None, prune_amounts) if prune_amounts else None
    torch.cuda.synchronize()
    mse_corrupted, mse_gt, psnrs, ssims = book.results()
    if save:
        A.save_npz(run_dir, task, method, head, mse_corrupted, mse_gt, recons, uncerts_epi, uncerts_ale, psnrs, ssims)
        with open(os.path.join(run_dir, "locals.txt"), "a") as f:
            print("max psnr_gt_sm = %.4f, max ssim_gt_sm = %.4f" % (np.nanmax(psnrs[:, 2]), np.nanmax(ssims[:, 2])), file=f)
            if plot:                                                  # mse_noisy / mse_gt / psnrs / ssims .png + the maxima lines (:201-258, :1431-1433)
                A.plot_results({method: mse_corrupted}, {method: mse_gt}, {method: psnrs}, {method: ssims}, run_dir, f)
        if plot and task == "sr":
            A.sr_input_png(run_dir, head[0], head[1], factor)
        if plot and task == "inp":
            pngs(num_iter - 1, (mse_corrupted, mse_gt, psnrs), recons[-1], uncerts_epi[-1], uncerts_ale[-1])
    res = {"psnr": float(psnrs[-1, 2]), "run_dir": run_dir if save else None, "psnrs": psnrs, "ssims": ssims, A.MSE_KEY[task]: mse_corrupted,
           "mse_gt": mse_gt, "recons": recons, "uncerts": uncerts_epi, "uncerts_ale": uncerts_ale, "seconds": time.perf_counter() - t0, "engine": eng}
    if pred is not None:
        res["predictive"] = pred
    if cal is not None:
        res["calibration"] = cal
    if pruning is not None:
        res["pruning"] = pruning
    return res


def _run(task, img, imsize, p_sigma, num_iter, lr, temp, sigma, input_depth, seed, show_every, plot, save, save_path, K, factor=4,
         theta_step=4.0, verbose=False, net_kwargs=None, method="mfvi", weight_decay=0.0, dropout_p=0.3, gamma=0.996, param_dtype="f32", predict_samples=0,
         calibration=False, calibration_bins=15, downsampler="nearest", tv_weight=0.0, tv_beta=0.5, kl_type="reverse", prior_mixture=None, prune_amounts=None,
         **unused):
    """What _fit needs of a den / sr / ct run: its locals.txt fields and, once the run directory stands, the image, the task's target and engine,
    the _Book and the two head arrays as the reference writes them per task: den img_gt / img_noisy (:1438), sr img_hr / img_lr (:2258), ct
    img_gt / img_radon (:643) with the reference's shapes (get_image() arrays are (1, H, W), img_lr is squeezed, the CT tensors keep
    (1, 1, ., .))."""
    sib = dict(weight_decay=weight_decay, dropout_p=dropout_p, gamma=gamma)
    tv = _tv_fields(tv_weight, tv_beta, task)      # tv_weight * mean_k TV_beta(out_k[0]) joins the objective (all four methods); off: nothing changes
    tv.update(_kl_fields(kl_type, method, prior_mixture))      # kl_type='forward' (mfvi): KL(posterior || prior) in the objective, against prior_mixture if given; 'reverse': nothing changes
    hyper = dict(temp=temp, sigma=sigma) if method == "mfvi" else {"dip": {}, "mcd": dict(dropout_p=dropout_p, weight_decay=weight_decay),
                                                                  "sgld": dict(gamma=gamma, weight_decay=weight_decay)}.get(method, {})
    fields = dict(task=task, method=method, img=img if not isinstance(img, np.ndarray) else "<array>", imsize=imsize, p_sigma=p_sigma,
                  num_iter=num_iter, lr=lr, input_depth=input_depth, seed=seed, show_every=show_every, K=K, save_path=save_path,
                  **(dict(downsampler=downsampler) if task == "sr" else {}), **hyper, **tv,
                  **(dict(prune_amounts=list(prune_amounts)) if prune_amounts else {}))
    if prune_amounts and param_dtype == "bf16":
        raise NotImplementedError("prune_amounts with param_dtype='bf16' is not built: the pruning kernels read float32 parameter rows")

    def prepare(n_it):
        import torch
        img_np = _load_image(img, imsize, seed)
        H, W = img_np.shape
        noisy = None
        if task == "den":
            rng = np.random.default_rng(seed + 1)
            noisy = np.clip(img_np + rng.normal(scale=p_sigma, size=img_np.shape), 0, 1).astype(np.float32)      # denoising_utils.py:11
            target, head = noisy, (img_np[None], noisy[None])
            eng = _make_engine(method, H, W, "den", K, input_depth, temp, sigma, lr, seed, net_kwargs, sib, param_dtype=param_dtype, **tv)
        elif task == "sr":
            if downsampler != "nearest":      # img_small = downsampler(img_hr) with the run's operator (models/downsampler.py)
                from .downsampler import downsample
                eng = _make_engine(method, H, W, "sr", K, input_depth, temp, sigma, lr, seed, net_kwargs, sib, sr_factor=factor, param_dtype=param_dtype,
                                   downsampler=downsampler, **tv)
                target = downsample(torch.from_numpy(img_np).cuda(), downsampler, factor).cpu().numpy()
            else:
                target = np.ascontiguousarray(img_np[::factor, ::factor])    # nearest /factor decimation (:2095-2099)
                eng = _make_engine(method, H, W, "sr", K, input_depth, temp, sigma, lr, seed, net_kwargs, sib, sr_factor=factor, param_dtype=param_dtype,
                                   **tv)
            head = (img_np[None], target)
        else:
            theta = np.arange(0, 180.0, theta_step, dtype=np.float32)     # :545
            eng = _make_engine(method, H, W, "ct", K, input_depth, temp, sigma, lr, seed, net_kwargs, sib, theta_deg=theta.tolist(), **tv)
            target = torch.empty((len(theta), W), device="cuda")
            gt_d = torch.from_numpy(img_np).cuda()
            L.check(L.lib().mfvi_radon_forward(L.ptr(gt_d), L.ptr(eng.theta), 1, H, W, len(theta), L.ptr(target), L.stream_ptr()))
            head = (img_np[None, None], target.cpu().numpy()[None, None])
        eng.set_target(torch.from_numpy(target) if isinstance(target, np.ndarray) else target)
        return img_np, eng, _Book(eng, n_it, img_np, noisy, task=task, factor=factor, downsampler=downsampler), head, None, 1
    return _fit(task, method, fields, prepare, num_iter, show_every, plot, save, save_path, verbose, predict_samples, calibration, calibration_bins,
                downsampler, factor, prune_amounts=prune_amounts)


def run_den_mfvi(img="phantom", imsize=(256, 256), p_sigma=0.1, num_iter=5000, lr=3e-4, temp=4e-6, sigma=0.01, input_depth=16, seed=42,
                 show_every=100, plot=False, save=True, save_path="../logs", K=1, **kw):
    """bayesian_optimization.py:1240-1444.  Returns the dict of results; ['psnr'] is the reference's return value."""
    return _run("den", img, imsize, p_sigma, num_iter, lr, temp, sigma, input_depth, seed, show_every, plot, save, save_path, K, **kw)


def run_sr_mfvi(img="phantom", imsize=(512, 512), factor=4, num_iter=5000, lr=3e-4, temp=4e-6, sigma=0.01, input_depth=32, seed=42,
                show_every=100, plot=False, save=True, save_path="../logs", K=1, **kw):
    """bayesian_optimization.py:2048-2263 (p_sigma is swallowed by **kwargs there too)."""
    kw.pop("p_sigma", None)
    return _run("sr", img, imsize, 0.0, num_iter, lr, temp, sigma, input_depth, seed, show_every, plot, save, save_path, K, factor=factor, **kw)


def run_ct_mfvi(img="phantom", imsize=(256, 256), num_iter=5000, lr=3e-4, temp=4e-6, sigma=0.01, input_depth=16, seed=42,
                show_every=100, plot=False, save=True, save_path="../logs", K=1, **kw):
    """bayesian_optimization.py:442-648."""
    kw.pop("p_sigma", None)
    return _run("ct", img, imsize, 0.0, num_iter, lr, temp, sigma, input_depth, seed, show_every, plot, save, save_path, K, **kw)


def _sibling(task, method, defaults):
    """run_<task>_<method> with the reference's keyword names and defaults; everything else as the MFVI runner of the task."""
    def run(img="phantom", imsize=defaults.get("imsize", (256, 256)), num_iter=5000, lr=defaults.get("lr", 3e-4), input_depth=defaults.get("input_depth", 16),
            seed=42, show_every=100, plot=False, save=True, save_path="../logs", K=1, p_sigma=0.1, **kw):
        hyper = {k: kw.pop(k, v) for k, v in defaults.items() if k in ("weight_decay", "dropout_p", "gamma")}
        kw.pop("temp", None); kw.pop("sigma", None)
        if task == "inp":
            hyper.setdefault("weight_decay", 0.0)                     # run_inp_dip: weight_decay = 0 (bayesian_optimization.py:2756)
            return run_inp_mfvi(img=img, imsize=imsize, num_iter=num_iter, lr=lr, input_depth=input_depth, seed=seed, show_every=show_every,
                                plot=plot, save=save, save_path=save_path, K=K, method=method, **hyper, **kw)
        return _run(task, img, imsize, p_sigma if task == "den" else 0.0, num_iter, lr, 0.0, 0.0, input_depth, seed, show_every, plot, save, save_path, K,
                    method=method, **hyper, **kw)
    run.__name__ = "run_%s_%s" % (task, method)
    run.defaults = dict(defaults)      # (run_sibling_batch fills a job's missing hyper-parameters from them)
    run.__doc__ = "bayesian_optimization.py run_%s_%s; returns the dict of results (['psnr'] is the reference's return value)." % (task, method)
    return run


# keyword defaults of the reference's signatures (bayesian_optimization.py:261-280, 651-670, 862-881, 1064-1083, 1447-1466, 1658-1677,
# 1863-1883, 2266-2286, 2484-2504, 3117-3135, 3328-3346)
run_den_dip = _sibling("den", "dip", dict())
run_den_mcd = _sibling("den", "mcd", dict(dropout_p=0.3, weight_decay=3e-4))
run_den_sgld = _sibling("den", "sgld", dict(gamma=0.996, weight_decay=5e-8))
run_sr_dip = _sibling("sr", "dip", dict(imsize=(512, 512), input_depth=32))
run_sr_mcd = _sibling("sr", "mcd", dict(imsize=(512, 512), input_depth=32, dropout_p=0.2, weight_decay=1e-4))
run_sr_sgld = _sibling("sr", "sgld", dict(imsize=(512, 512), input_depth=32, gamma=0.996, weight_decay=1e-4))
run_ct_dip = _sibling("ct", "dip", dict())
run_ct_mcd = _sibling("ct", "mcd", dict(dropout_p=0.3, weight_decay=3e-4))
run_ct_sgld = _sibling("ct", "sgld", dict(gamma=0.996, weight_decay=5e-8))


def scratch_mask(H, W, seed):
    """Synthetic scratches for a job without a mask: a seeded random-walk mask [1, H, W], ~12 % missing (1 = known pixel)."""
    rng = np.random.default_rng(seed)
    mask = np.ones((1, H, W), np.float32)
    for _ in range(24):
        y, x = rng.integers(0, H), rng.integers(0, W)
        for _ in range(H):
            mask[0, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 0
            y = int(np.clip(y + rng.integers(-1, 2), 0, H - 1)); x = int(np.clip(x + rng.integers(-1, 2), 0, W - 1))
    return mask


def run_inp_mfvi(img="phantom", mask=None, imsize=(256, 256), num_iter=5000, lr=2e-3, temp=4e-6, sigma=0.01, input_depth=32, seed=42,
                 show_every=100, plot=False, save=True, save_path="../logs", K=1, net_kwargs=None, verbose=False, method="mfvi",
                 weight_decay=1e-4, dropout_p=0.2, gamma=0.996, predict_samples=0, calibration=False, calibration_bins=15, kl_type="reverse", prior_mixture=None, prune_amounts=None,
                 **unused):
    """bayesian_optimization.py:2892-3114: inpainting with the 6-scale no-skip net (5x5 down filters, nearest up-sampling), sigmoid on
    the colour channels, masked Gaussian NLL.  img: (3, H, W) array in [0, 1] or 'phantom' (three synthetic planes); mask: (1|3, H, W),
    1 = known pixel (the reference ships its masks in data/inpainting/).  save.npz carries the reference's keys for this task
    (img_inpainting, img_mask, mse_corrupted, mse_gt, recons, uncerts, uncerts_ale, psnrs, ssims)."""
    _tv_fields(unused.get("tv_weight", 0.0), unused.get("tv_beta", 0.5), "inp")      # refused with a weight > 0: the term is not built for inpainting
    kl = _kl_fields(kl_type, method, prior_mixture)
    fields = dict(task="inp", imsize=imsize, num_iter=num_iter, lr=lr, temp=temp, sigma=sigma, input_depth=input_depth, seed=seed,
                  show_every=show_every, K=K, save_path=save_path, **kl)

    def prepare(n_it):
        import torch
        if isinstance(img, np.ndarray):
            img_np = np.ascontiguousarray(img, np.float32)
        else:
            img_np = np.stack([_load_image(img, imsize, seed + c) for c in range(3)]).astype(np.float32)
        _, H, W = img_np.shape
        mask_np = np.ascontiguousarray(scratch_mask(H, W, seed) if mask is None else mask, np.float32)
        if mask_np.ndim == 2:
            mask_np = mask_np[None]
        eng = _make_engine(method, H, W, "inp", K, input_depth, temp, sigma, lr, seed, net_kwargs, dict(weight_decay=weight_decay, dropout_p=dropout_p, gamma=gamma),
                           **kl)
        eng.set_target(torch.from_numpy(img_np), torch.from_numpy(mask_np))
        return img_np, eng, _BookInp(eng, n_it, img_np, mask_np), (img_np, mask_np), mask_np, 3
    return _fit("inp", method, fields, prepare, num_iter, show_every, plot, save, save_path, verbose, predict_samples, calibration, calibration_bins,
                unused.get("downsampler", "nearest"), prune_amounts=prune_amounts)


run_inp_dip = _sibling("inp", "dip", dict(input_depth=32, lr=2e-3))
run_inp_mcd = _sibling("inp", "mcd", dict(input_depth=32, lr=2e-3, dropout_p=0.2, weight_decay=1e-4))
run_inp_sgld = _sibling("inp", "sgld", dict(input_depth=32, lr=2e-3, gamma=0.996, weight_decay=1e-4))

# which two bo_params a method's candidates are (bayesian_optimization.py:3715-3718)
BO_KEYS = {"mfvi": ("temp", "sigma"), "mcd": ("dropout_p", "weight_decay"), "sgld": ("gamma", "weight_decay"), "dip": ()}


def load_config(path, bayes="mfvi", with_devices=False):
    """The reference's JSON schema {bo_params:{<name>:{candidates}, ...}, run_params:{...}} (bayesian_optimization.py:3901-3909 reads it
    through pandas; plain json is equivalent).  Returns ([candidate dicts], run_params[, devices]); `devices` is run_params['devices']
    of the reference's configs (eval_result.py:21-22), e.g. ["cuda:0", ..., "cuda:7"]."""
    cfg = json.load(open(path))
    rp = dict(cfg["run_params"])
    devices = rp.pop("devices", None)
    rp.pop("bo_results_path", None)
    keys = BO_KEYS[bayes]
    if not keys:
        cands = [dict()]
    else:
        a, b = keys
        cands = [{a: x, b: y} for x in cfg["bo_params"][a]["candidates"] for y in cfg["bo_params"][b]["candidates"]]
    return (cands, rp, devices) if with_devices else (cands, rp)


def _save_bookkeeping(book, run_dir, heads):
    """--batch-bookkeeping: bookkeeping_batch.npz (the per-iteration curves [n_it, F, ...] and the snapshots [n_snap, F, H, W] of a BatchBook)
    beside batch.npz / volume.npz, and fit_%03d/save.npz per fit as the single-fit runner of the task writes it (heads[f]: its two
    task-specific arrays, artifacts.save_npz)."""
    mse_noisy, mse_gt, psnrs, ssims = book.results()
    stack = lambda k: np.stack([s[k] for s in book.snaps]) if book.snaps else np.zeros((0, book.F, book.H, book.W), np.float32)
    arrs = dict(iterations=np.asarray([s[0] for s in book.snaps], np.int64), mse_noisy=mse_noisy, mse_gt=mse_gt, psnrs=psnrs, ssims=ssims, recons=stack(3),
                uncerts=stack(1))
    if book.C > 1:
        arrs["uncerts_ale"] = stack(2)
    np.savez(os.path.join(run_dir, "bookkeeping_batch.npz"), **arrs)
    for f in range(book.F):
        fit_dir = os.path.join(run_dir, "fit_%03d" % f)
        os.makedirs(fit_dir, exist_ok=False)
        book.save_npz(f, fit_dir, heads[f])


def _drive_batch(batch, gt, kind, keys, num_iter, show_every, save, save_path, verbose, track=None, heads=None, batch_predict_samples=0,
                 batch_calibration_bins=0):
    """What every batched run does with its batch once the targets are set.  kind: "batch" or "volume", the name of the
    run directory's suffix and of the npz.  track: the keywords of batch.track (None: no bookkeeping), heads: per row the two head arrays of
    its save.npz.  The loop: step(), the book's snapshot every show_every, and every show_every and at the last iteration losses() (kept as
    the class returns it) and psnr(gt).  Then dead / final, <kind>.npz = the common keys + keys(losses) (the caller's own, evaluated after the
    last iteration), _save_bookkeeping, _batch_predict -> the common keys of the result."""
    n_it = num_iter + 1                                               # bayesian_optimization.py:1291, :2935
    book = batch.track(gt, n_it, **track) if track is not None else None      # 
    at, psnrs, losses, tvs = [], [], [], []
    tv_on = getattr(batch, "_tv", None) is not None                  # the total-variation term: recorded like nll, and only then
    kl_on = any(k != "reverse" for k in getattr(batch, "kl_types", None) or ())      # some row is forward: the npz names every row's direction, and only then
    t0 = time.perf_counter()
    for i in range(n_it):
        batch.step()
        if book is not None and i % show_every == 0:
            book.snapshot()
        if i % show_every == 0 or i == n_it - 1:
            losses.append(batch.losses()); at.append(i); psnrs.append(batch.psnr(gt))
            if tv_on:
                tvs.append(batch.tv())
            if verbose:
                print("iter %6d  psnr_gt_sm %s%s  (%.1f it/s x %d %s)" % (i, np.array2string(psnrs[-1], precision=2),
                                                                         "  tv %s" % np.array2string(tvs[-1], precision=3) if tv_on else "",
                                                                         (i + 1) / (time.perf_counter() - t0), batch.n_rows,
                                                                         {"batch": "fits", "volume": "slices"}[kind]))
    dead = batch.dead
    final = np.where(dead != 0, np.nan, psnrs[-1])
    run_dir = None
    if save:
        run_dir = os.path.join(save_path, "%s_%s" % (time.time(), kind))
        os.makedirs(run_dir, exist_ok=False)
        np.savez(os.path.join(run_dir, kind + ".npz"), K=np.int64(batch.K), seed=np.int64(batch.seed), num_iter=np.int64(num_iter), iterations=np.asarray(at),
                 psnr_gt_sm=np.stack(psnrs), recon=batch.recon().cpu().numpy(), dead=dead, **keys(losses),
                 **(dict(tv_weight=np.asarray(batch.tv_weights), tv_beta=np.float64(batch.tv_beta), tv=np.stack(tvs)) if tv_on else {}),
                 **(dict(kl_type=np.asarray(batch.kl_types)) if kl_on else {}),      # fixed-width strings, one per row
                 **_mix_keys(batch))                                                # the rows' scale-mixture priors, when a row has one (section 26)
        if book is not None:
            _save_bookkeeping(book, run_dir, heads)
    pred = _batch_predict(batch, batch_predict_samples, gt, run_dir, batch_calibration_bins) if batch_predict_samples else None
    return dict(psnr=[float(x) for x in final], run_dir=run_dir, seconds=time.perf_counter() - t0, dead=dead, predictive=pred)


def _nll_kl(losses):
    """The recorded losses() of an ELBO batch, (nll, kl, loss) per record -> the nll and kl keys of its npz."""
    return dict(nll=np.stack([l[0] for l in losses]), kl=np.stack([l[1] for l in losses]))


def _den_sr_batch(task, jobs, imsize, seed, p_sigma, factor):
    """The den / sr jobs of one batch -> (gt [F, H, W], targets, the keywords of track(), per fit the head arrays of its save.npz)."""
    imgs = [_load_image(j["img"], imsize, seed) for j in jobs]
    H, W = imgs[0].shape
    if any(im.shape != (H, W) for im in imgs):
        raise ValueError("the images of one batch must share their size")
    gt = np.stack(imgs)
    if task == "den":      # every job's noise as the single-fit runner draws it (same image and seed: the same noisy image)
        targets = np.stack([np.clip(im + np.random.default_rng(seed + 1).normal(scale=p_sigma, size=im.shape), 0, 1).astype(np.float32) for im in imgs])
        return gt, targets, dict(noisy=targets), [(g[None], t[None]) for g, t in zip(gt, targets)]
    targets = np.ascontiguousarray(gt[:, ::factor, ::factor])
    return gt, targets, dict(noisy=None), [(g[None], t) for g, t in zip(gt, targets)]


def run_fit_batch(task, jobs, imsize=(256, 256), p_sigma=0.1, num_iter=5000, lr=3e-4, input_depth=16, seed=42, show_every=100, save=True,
                  save_path="../logs", K=1, factor=4, net_kwargs=None, verbose=False, autotune=True, batch_predict_samples=0,
                  batch_calibration_bins=0, batch_bookkeeping=False, tv_weight=0.0, tv_beta=0.5, kl_type="reverse", prior_mixture=None, **unused):
    """The (image, temp, sigma) jobs of one batch as ONE FitBatch (--fits-per-launch): the loop of run_den_mfvi /
    run_sr_mfvi for every job at once, every fit with the noise of its own RNG samples.  jobs: dicts with img, temp, sigma (and optionally
    lr, tv_weight and kl_type; tv_weight / tv_beta: the run-wide total-variation term, DESIGN.md section 23 -- with a weight > 0 batch.npz also
    holds tv_weight, tv_beta and tv, per record as nll; kl_type: the run-wide direction of the KL term, DESIGN.md section 25 -- with a forward
    fit batch.npz also names every fit's direction, kl_type).  Writes batch.npz (hyper-parameters; per fit psnr_gt_sm, nll and kl every
    show_every iterations, the final reconstruction, dead);
    save.npz and the PNG artefacts stay with the single-fit runners.  batch_predict_samples >= 2: predictive_batch.npz (and with
    batch_calibration_bins calibration_batch.npz) beside it (_batch_predict).  batch_bookkeeping: the per-iteration records of every fit
    (BatchBook) -> bookkeeping_batch.npz and fit_%03d/save.npz beside it (_save_bookkeeping).  Returns dict(psnr=[per fit, NaN for a dead
    fit], ...)."""
    import torch
    from .fitbatch import FitBatch
    _check_batch_predict(batch_predict_samples, batch_calibration_bins)
    if task not in ("den", "sr"):
        raise NotImplementedError("--fits-per-launch serves denoising and super-resolution, not %r" % (task,))
    if unused.get("downsampler", "nearest") != "nearest":
        raise NotImplementedError("batched fits project with [::f, ::f] only (downsampler='nearest'), not %r" % (unused["downsampler"],))
    gt, targets, track, heads = _den_sr_batch(task, jobs, imsize, seed, p_sigma, factor)
    temps, sigmas, lrs = [j["temp"] for j in jobs], [j["sigma"] for j in jobs], [j.get("lr", lr) for j in jobs]
    fb = FitBatch(gt.shape[1], gt.shape[2], len(jobs), task=task, K=K, input_depth=input_depth, temp=temps, sigma=sigmas, lr=lrs, seed=seed, sr_factor=factor,
                  net_kwargs=net_kwargs, init="shared", autotune=autotune,      # the reference's candidates all start from one seed
                  tv_weight=[j.get("tv_weight", tv_weight) for j in jobs], tv_beta=tv_beta, kl_type=[j.get("kl_type", kl_type) for j in jobs],
                  prior_mixture=[j.get("prior_mixture", prior_mixture) for j in jobs])      # a job's scale-mixture prior (absent: the run's; None: Gaussian)
    fb.set_targets(torch.from_numpy(targets))
    keys = lambda losses: dict(task=task, temp=np.asarray(temps), sigma=np.asarray(sigmas), lr=np.asarray(lrs), prior_sigma=np.asarray(fb.prior_sigma),
                               **_nll_kl(losses))
    return dict(_drive_batch(fb, gt, "batch", keys, num_iter, show_every, save, save_path, verbose, track if batch_bookkeeping else None, heads,
                             batch_predict_samples, batch_calibration_bins), batch=fb)


def fit_batch_job(task, jobs, **kw):
    """One batch of fits in a worker process of the fan-out -> the PSNR of every fit."""
    return run_fit_batch(task, jobs, **kw)["psnr"]


def run_inpaint_batch(jobs, imsize=(256, 256), num_iter=5000, lr=2e-3, input_depth=32, seed=42, show_every=100, save=True, save_path="../logs",
                      K=1, net_kwargs=None, verbose=False, autotune=True, mask=None, batch_predict_samples=0, batch_calibration_bins=0, kl_type="reverse", prior_mixture=None,
                      **unused):
    """The (image, mask, temp, sigma) jobs of one batch as ONE InpaintBatch (--inpaint-fits): the loop of run_inp_mfvi for
    every job at once.  jobs: dicts with img ((3, H, W) array, or what run_inp_mfvi loads), temp, sigma and optionally mask ((1|3, H, W);
    absent: `mask`, the run_params' mask that run_inp_mfvi takes too, else that function's seeded scratch mask), lr and kl_type (absent: the run's).
    Writes batch.npz with the keys of run_fit_batch plus mask, recon [F, 3, H, W] and
    ale [F, H, W]; save.npz and the PNG artefacts stay with the single-fit runner (an InpaintBatch has no bookkeeping).  Returns
    dict(psnr=[per fit, NaN for a dead fit], ...)."""
    import torch
    from .inpaintbatch import InpaintBatch
    _check_batch_predict(batch_predict_samples, batch_calibration_bins)
    for w in [unused.get("tv_weight", 0.0)] + [j.get("tv_weight", 0.0) for j in jobs]:      # (an InpaintBatch has no total-variation term)
        _tv_fields(w, unused.get("tv_beta", 0.5), "inp")
    imgs = [np.ascontiguousarray(j["img"], np.float32) if isinstance(j["img"], np.ndarray) else
            np.stack([_load_image(j["img"], imsize, seed + c) for c in range(3)]).astype(np.float32) for j in jobs]
    _, H, W = imgs[0].shape
    if any(im.shape != (3, H, W) for im in imgs):
        raise ValueError("the images of one batch must share their size, (3, H, W) each")
    masks = []
    for j in jobs:
        m = j.get("mask") if j.get("mask") is not None else mask
        m = np.ascontiguousarray(m, np.float32) if m is not None else scratch_mask(H, W, seed)
        masks.append(m[None] if m.ndim == 2 else m)
    if any(m.shape != masks[0].shape or m.shape[1:] != (H, W) for m in masks):
        raise ValueError("the masks of one batch must share their shape, (1|3, H, W) each")
    gt = np.stack(imgs)
    temps, sigmas, lrs = [j["temp"] for j in jobs], [j["sigma"] for j in jobs], [j.get("lr", lr) for j in jobs]
    ib = InpaintBatch(H, W, len(jobs), K=K, input_depth=input_depth, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=net_kwargs, init="shared",
                      autotune=autotune, kl_type=[j.get("kl_type", kl_type) for j in jobs],                               # the reference's candidates all start from one seed
                      prior_mixture=[j.get("prior_mixture", prior_mixture) for j in jobs])
    ib.set_targets(torch.from_numpy(gt), torch.from_numpy(np.stack(masks)))
    keys = lambda losses: dict(task="inp", temp=np.asarray(temps), sigma=np.asarray(sigmas), lr=np.asarray(lrs), prior_sigma=np.asarray(ib.prior_sigma),
                               **_nll_kl(losses), mask=ib.masks.cpu().numpy(), ale=ib.ale().cpu().numpy())
    return dict(_drive_batch(ib, gt, "batch", keys, num_iter, show_every, save, save_path, verbose, batch_predict_samples=batch_predict_samples,
                             batch_calibration_bins=batch_calibration_bins), batch=ib)


def inpaint_batch_job(task, jobs, **kw):
    """One batch of inpainting fits in a worker process of the fan-out -> the PSNR of every fit."""
    return run_inpaint_batch(jobs, **kw)["psnr"]


def run_sibling_batch(task, method, jobs, imsize=None, p_sigma=0.1, num_iter=5000, lr=None, input_depth=None, seed=42, show_every=100, save=True,
                      save_path="../logs", K=1, factor=4, net_kwargs=None, verbose=False, autotune=True, param_noise_sigma=2.0,
                      batch_predict_samples=0, batch_calibration_bins=0, batch_bookkeeping=False, tv_weight=0.0, tv_beta=0.5, **unused):
    """The (image, candidate) jobs of one batch as ONE SiblingBatch (--sibling-fits): the loop of run_<task>_<method> for
    every job at once.  jobs: dicts with img and, per method, dropout_p / weight_decay (mcd) or gamma / weight_decay (sgld), optionally lr;
    what a job leaves out takes the default of run_<task>_<method>.  Writes batch.npz (hyper-parameters; per fit psnr_gt_sm and the data
    term every show_every iterations, the final reconstruction, dead); save.npz, SGLD's iterate ring and the PNG artefacts stay with the
    single-fit runners; batch_bookkeeping: bookkeeping_batch.npz and fit_%03d/save.npz as run_fit_batch writes them.  Returns
    dict(psnr=[per fit, NaN for a dead fit], ...)."""
    import torch
    from .siblingbatch import SiblingBatch
    if task not in ("den", "sr") or method not in ("dip", "mcd", "sgld"):
        raise NotImplementedError("--sibling-fits serves dip, mcd and sgld on denoising and super-resolution, not %r / %r" % (method, task))
    _check_batch_predict(batch_predict_samples, batch_calibration_bins)
    if batch_predict_samples and method != "mcd":
        raise ValueError("batch_predict_samples=%d: of the batched siblings only MC dropout (mcd) has a posterior to draw from, not %r" % (batch_predict_samples, method))
    dflt = globals()["run_%s_%s" % (task, method)].defaults
    imsize = imsize or dflt.get("imsize", (256, 256))
    lr = dflt.get("lr", 3e-4) if lr is None else lr
    input_depth = dflt.get("input_depth", 16) if input_depth is None else input_depth
    gt, targets, track, heads = _den_sr_batch(task, jobs, imsize, seed, p_sigma, factor)
    hyper = {k: [j.get(k, dflt.get(k, d)) for j in jobs] for k, d in (("weight_decay", 0.0), ("dropout_p", 0.3), ("gamma", 0.996))}
    lrs = [j.get("lr", lr) for j in jobs]
    sb = SiblingBatch(gt.shape[1], gt.shape[2], len(jobs), method, task=task, K=K, input_depth=input_depth, lr=lrs, seed=seed, sr_factor=factor,
                      net_kwargs=net_kwargs, param_noise_sigma=param_noise_sigma, init="shared", autotune=autotune, **hyper,      # (one seed, as above)
                      tv_weight=[j.get("tv_weight", tv_weight) for j in jobs], tv_beta=tv_beta)      # (the total-variation term as run_fit_batch takes it)
    sb.set_targets(torch.from_numpy(targets))
    keys = lambda losses: dict(method=method, task=task, lr=np.asarray(lrs), weight_decay=np.asarray(sb.weight_decays), dropout_p=np.asarray(sb.dropout_ps),
                               gamma=np.asarray(sb.gammas), loss=np.stack(losses))
    return dict(_drive_batch(sb, gt, "batch", keys, num_iter, show_every, save, save_path, verbose, track if batch_bookkeeping else None, heads,
                             batch_predict_samples, batch_calibration_bins), batch=sb)


def sibling_batch_job(task, jobs, method="dip", **kw):
    """One batch of sibling fits in a worker process of the fan-out -> the PSNR of every fit."""
    return run_sibling_batch(task, method, jobs, **kw)["psnr"]


# the batching flags of the CLI: the function that runs one batch of jobs in this process (called with task=, jobs= and the run parameters; the
# method of --sibling-fits rides in the run parameters) and the worker a device's fresh process resolves by name (fanout.run_jobs)
BATCH_KINDS = {"fits_per_launch": (run_fit_batch, "mfvi_dip_mia_amd.runner:fit_batch_job"),
               "inpaint_fits": (run_inpaint_batch, "mfvi_dip_mia_amd.runner:inpaint_batch_job"),
               "sibling_fits": (run_sibling_batch, "mfvi_dip_mia_amd.runner:sibling_batch_job")}


def _run_batches(task, jobs, n, rp, K, devices, verbose=False, kind="fits_per_launch"):
    """jobs -> batches of up to n (fanout.group_jobs) -> one batch of BATCH_KINDS[kind] each (a FitBatch, an InpaintBatch or a SiblingBatch), here
    or dealt round-robin to one worker per device.  Returns (results [(job index, job, psnr)], dropped [(job index, job, why)], batches)."""
    batch_fn, worker = BATCH_KINDS[kind]
    from .fanout import group_jobs, run_jobs
    shapes = {}      # (the size of an image file is known once it is read; every distinct image once)
    for j in jobs:
        if isinstance(j["img"], str) and j["img"] not in shapes:
            shapes[j["img"]] = _load_image(j["img"], rp.get("imsize", (256, 256)), rp.get("seed", 42)).shape
    key = (task, rp.get("input_depth"), rp.get("num_iter"), K)
    batches = group_jobs([key + (shapes[j["img"]] if isinstance(j["img"], str) else np.squeeze(j["img"]).shape,) for j in jobs], n)
    bjobs = [dict(jobs=[jobs[i] for i in b]) for b in batches]
    rp = {k: v for k, v in rp.items() if k not in ("plot",)}
    per_batch = {}
    if devices:
        res, drop = run_jobs(bjobs, devices, worker, dict(rp, task=task, K=K))
        per_batch = {bi: (y, None) for bi, _, y in res}
        per_batch.update({bi: (None, why) for bi, _, why in drop})
    else:
        for bi, bj in enumerate(bjobs):
            try:
                per_batch[bi] = (batch_fn(task=task, jobs=bj["jobs"], K=K, verbose=verbose, **rp)["psnr"], None)
            except (RuntimeError, ValueError) as e:
                per_batch[bi] = (None, "%s: %s" % (type(e).__name__, e))
    results, dropped = [], []
    for bi, b in enumerate(batches):
        ys, why = per_batch[bi]
        for pos, i in enumerate(b):
            if ys is None:
                dropped.append((i, jobs[i], why))
            elif np.isnan(ys[pos]):
                dropped.append((i, jobs[i], "dead fit (non-finite data term)"))
            else:
                results.append((i, jobs[i], ys[pos]))
    results.sort(key=lambda r: r[0]); dropped.sort(key=lambda r: r[0])
    return results, dropped, batches


def parse_ct_volume(spec):
    """--ct-volume: 'phantom:D' -> ("phantom", D), a .npy path -> ("npy", path); anything else is a ValueError (no file is touched)."""
    if isinstance(spec, str) and spec.startswith("phantom:"):
        try:
            D = int(spec[len("phantom:"):])
        except ValueError:
            D = 0
        if D < 1:
            raise ValueError("--ct-volume %s: phantom:D with D >= 1 slices" % spec)
        return "phantom", D
    if isinstance(spec, str) and spec.endswith(".npy"):
        return "npy", spec
    raise ValueError("--ct-volume %s: a .npy file holding [D, S, S], or phantom:D" % (spec,))


def _load_volume(volume, imsize, seed):
    """[D, S, S] float32 from an array, a .npy path or 'phantom:D' (the package's phantom at seeds seed .. seed + D - 1)."""
    if isinstance(volume, np.ndarray):
        v = volume.astype(np.float32)
    else:
        kind, what = parse_ct_volume(volume)
        v = np.stack([phantom(imsize[0], imsize[1], seed + d) for d in range(what)]) if kind == "phantom" else np.load(what).astype(np.float32)
    if v.ndim != 3 or v.shape[1] != v.shape[2]:
        raise ValueError("expected a stack of square slices [D, S, S], got shape %s" % (v.shape,))
    return np.ascontiguousarray(v)


def run_ct_volume(volume, temp, sigma, slices_per_launch=None, imsize=(256, 256), num_iter=5000, lr=3e-4, input_depth=16, seed=42, show_every=100,
                  save=True, save_path="../logs", K=1, theta_step=4.0, net_kwargs=None, verbose=False, autotune=True, batch_predict_samples=0,
                  batch_calibration_bins=0, batch_bookkeeping=False, tv_weight=0.0, tv_beta=0.5, kl_type="reverse", prior_mixture=None, **unused):
    """The loop of run_ct_mfvi (bayesian_optimization.py:442-648) for every slice of a stack at once, as ONE CtVolume (--ct-volume; DESIGN.md
    section 16).  volume: [D, S, S] array, .npy path or 'phantom:D'; temp / sigma / lr / tv_weight: scalars or one value per slice
    (tv_weight > 0: volume.npz also holds tv_weight, tv_beta and tv); kl_type: a name or one per slice (a forward slice:
    volume.npz also holds kl_type).  Writes volume.npz
    (angles, sinograms, hyper-parameters; per slice psnr_gt_sm, nll and kl every show_every iterations, the reconstruction, dead); the ring
    buffers, SSIM curves, save.npz and PNG artefacts stay with the single-fit runner unless batch_bookkeeping (bookkeeping_batch.npz and
    fit_%03d/save.npz per slice, _save_bookkeeping; no PNGs).  Returns dict(psnr=[per slice, NaN for a dead one], ...)."""
    import torch
    from .ctvolume import CtVolume
    _check_batch_predict(batch_predict_samples, batch_calibration_bins)
    gt = _load_volume(volume, imsize, seed)
    theta = np.arange(0, 180.0, theta_step, dtype=np.float32)         # :545
    vol = CtVolume(gt.shape[1], gt.shape[0], slices_per_launch=slices_per_launch, K=K, input_depth=input_depth, temp=temp, sigma=sigma, lr=lr,
                   theta_deg=theta.tolist(), seed=seed, net_kwargs=net_kwargs, autotune=autotune, tv_weight=tv_weight, tv_beta=tv_beta, kl_type=kl_type,
                   prior_mixture=prior_mixture)      # one scale-mixture prior, or one (or None) per slice
    vol.set_volume(torch.from_numpy(gt))                              # img_radon = forward_radon(img_torch) (:547)
    sinos = vol.sinos.cpu().numpy()
    keys = lambda losses: dict(theta=theta, sinograms=sinos, temp=np.asarray(vol.temps), sigma=np.asarray(vol.sigmas), lr=np.asarray(vol.lrs),
                               prior_sigma=np.asarray(vol.prior_sigma), slices_per_launch=np.int64(vol.F), **_nll_kl(losses))
    heads = [(g[None, None], s[None, None]) for g, s in zip(gt, sinos)]      # as run_ct_mfvi writes them: img_gt (1, 1, S, S), img_radon (1, 1, T, S)
    r = _drive_batch(vol, gt, "volume", keys, num_iter, show_every, save, save_path, verbose, {} if batch_bookkeeping else None, heads,
                     batch_predict_samples, batch_calibration_bins)
    live = np.asarray(r["psnr"])[r["dead"] == 0]
    return dict(r, mean_psnr=float(live.mean()) if live.size else float("nan"), volume=vol)


def fit_job(fn_name, **kw):
    """One independent fit in a worker process of the fan-out: run_<task>_<method>(**kw) -> PSNR (the reference's return value)."""
    return globals()[fn_name](**kw)["psnr"]


def _check_cli(ap, a):
    """What main() refuses from the parsed arguments alone, before the config is read and before anything loads the library.  The order is
    behaviour (the first refusal that applies is the one reported; tests/golden/cli_refusals.json): --sr-downsampler, --batch-bookkeeping,
    --batch-predict-samples / --batch-calibration, then --sibling-fits, --inpaint-fits, --ct-volume and --fits-per-launch each ahead of the
    batching flags after it, then --calibration and --predict-samples of a single fit, then --tv-weight / --tv-beta, then --kl-type, then --prior-mixture."""
    on = {"--fits-per-launch": a.fits_per_launch, "--inpaint-fits": a.inpaint_fits, "--sibling-fits": a.sibling_fits, "--ct-volume": a.ct_volume is not None,
          "--predict-samples": a.predict_samples, "--calibration": a.calibration, "--bo-rounds": a.bo_rounds}

    def count(flag):
        if on[flag] < 0:
            ap.error("%s %d: 0 (off) or the number of fits per launch" % (flag, on[flag]))

    def alone(flag, others, why):
        for other in others:
            if on[other]:
                ap.error("%s does not combine with %s (%s)" % (flag, other, why))

    def f32(flag):
        if a.param_dtype != "f32":
            ap.error("%s takes float32 parameters (--param-dtype f32)" % flag)
    if a.sr_downsampler not in (None, "nearest"):
        if a.task != "super-resolution" or a.bayes != "mfvi":
            ap.error("--sr-downsampler %s belongs to --task super-resolution --bayes mfvi" % a.sr_downsampler)
        if a.fits_per_launch:
            ap.error("--sr-downsampler %s does not combine with --fits-per-launch (batched fits project with [::f, ::f])" % a.sr_downsampler)
    if a.batch_bookkeeping and not (a.fits_per_launch > 0 or a.sibling_fits > 0 or a.ct_volume is not None):
        ap.error("--batch-bookkeeping records every fit of a batch: it needs --fits-per-launch, --sibling-fits or --ct-volume (a single fit always "
                 "keeps these records; --inpaint-fits has no batched bookkeeping)")
    if a.batch_predict_samples or a.batch_calibration:
        if a.batch_predict_samples < 0 or a.batch_predict_samples == 1:
            ap.error("--batch-predict-samples %d: 0 (off) or at least 2" % a.batch_predict_samples)
        if not (a.fits_per_launch > 0 or a.ct_volume is not None or a.inpaint_fits > 0 or a.sibling_fits > 0):
            ap.error("--batch-predict-samples / --batch-calibration predict every fit of a batch: they need --fits-per-launch, --ct-volume, --inpaint-fits or "
                     "--sibling-fits (a single fit takes --predict-samples / --calibration)")
        if a.sibling_fits > 0 and a.bayes != "mcd":
            ap.error("--batch-predict-samples / --batch-calibration with --sibling-fits need a posterior to draw from (--bayes mcd), not %s" % a.bayes)
        if a.batch_calibration and not a.batch_predict_samples:
            ap.error("--batch-calibration calibrates the posterior predictive maps of --batch-predict-samples N (N >= 2)")
        if a.batch_calibration and not 1 <= a.calibration_bins <= L.UCE_MAX_BINS:
            ap.error("--calibration-bins %d outside 1..%d" % (a.calibration_bins, L.UCE_MAX_BINS))
    count("--sibling-fits")
    if a.sibling_fits:
        if a.bayes == "mfvi":
            ap.error("--sibling-fits batches the DIP, MC-dropout and SGLD fits (--bayes dip, mcd or sgld); mean-field VI fits batch with --fits-per-launch")
        if a.task not in ("denoising", "super-resolution"):
            ap.error("--sibling-fits serves denoising and super-resolution, not %s" % a.task)
        alone("--sibling-fits", ("--fits-per-launch", "--inpaint-fits", "--ct-volume", "--predict-samples", "--calibration"),
              "SiblingBatch.to_engine(f) serves one fit of a batch")
        f32("--sibling-fits")
    count("--inpaint-fits")
    if a.inpaint_fits:
        alone("--inpaint-fits", ("--fits-per-launch", "--ct-volume", "--predict-samples", "--calibration"), "InpaintBatch.to_engine(f) serves one fit of a batch")
        if a.task != "inpainting" or a.bayes != "mfvi":
            ap.error("--inpaint-fits batches mean-field VI inpainting fits (--task inpainting --bayes mfvi), not --task %s --bayes %s" % (a.task, a.bayes))
        f32("--inpaint-fits")
    if a.slices_per_launch is not None and (a.ct_volume is None or a.slices_per_launch < 1):
        ap.error("--slices-per-launch %d: at least 1, and only with --ct-volume" % a.slices_per_launch)
    if a.ct_volume is not None:
        try:
            parse_ct_volume(a.ct_volume)
        except ValueError as e:
            ap.error(str(e))
        if a.task != "ct" or a.bayes != "mfvi":
            ap.error("--ct-volume fits a CT stack by mean-field VI (--task ct --bayes mfvi), not --task %s --bayes %s" % (a.task, a.bayes))
        f32("--ct-volume")
        alone("--ct-volume", ("--fits-per-launch", "--predict-samples", "--calibration", "--bo-rounds"), "CtVolume.to_engine(d) serves one slice of a volume")
    count("--fits-per-launch")
    if a.fits_per_launch:
        if a.bayes != "mfvi":
            ap.error("--fits-per-launch batches mean-field VI fits (--bayes mfvi), not %s" % a.bayes)
        if a.task not in ("denoising", "super-resolution"):
            ap.error("--fits-per-launch serves denoising and super-resolution, not %s" % a.task)
        f32("--fits-per-launch")
        alone("--fits-per-launch", ("--predict-samples",), "FitBatch.to_engine(f).predict serves one fit of a batch")
        if a.calibration:
            ap.error("--fits-per-launch does not combine with --calibration")
    if a.calibration and a.bayes not in CALIBRATION_METHODS:
        ap.error("--calibration needs uncertainty maps (--bayes mfvi, mcd or sgld), not %s" % a.bayes)
    if a.calibration and not 1 <= a.calibration_bins <= L.UCE_MAX_BINS:
        ap.error("--calibration-bins %d outside 1..%d" % (a.calibration_bins, L.UCE_MAX_BINS))
    if a.predict_samples and a.bayes not in PREDICT_METHODS:
        ap.error("--predict-samples needs a posterior to draw from (--bayes mfvi or mcd), not %s" % a.bayes)
    if a.predict_samples < 0 or a.predict_samples == 1:
        ap.error("--predict-samples %d: 0 (off) or at least 2" % a.predict_samples)
    # the total-variation term, behind every older check (their order is pinned)
    if a.tv_weight is not None and not 0.0 <= a.tv_weight < float("inf"):
        ap.error("--tv-weight %r: finite and >= 0" % a.tv_weight)
    if a.tv_beta is not None and not 0.0 < a.tv_beta < float("inf"):
        ap.error("--tv-beta %r: finite and > 0" % a.tv_beta)
    if a.tv_weight and a.task == "inpainting":
        ap.error("--tv-weight %g does not combine with --task inpainting (the total-variation term serves denoising, super-resolution and ct)" % a.tv_weight)
    if a.kl_type == "forward" and a.bayes != "mfvi":
        ap.error("--kl-type forward chooses the direction of mean-field VI's KL term (--bayes mfvi); %s has no KL term" % a.bayes)
    if a.prior_mixture is not None:
        if a.bayes != "mfvi":
            ap.error("--prior-mixture is the prior of mean-field VI's KL term (--bayes mfvi); %s has no KL term" % a.bayes)
        from .rowbatch import check_prior_mixture
        try:
            check_prior_mixture(parse_prior_mixture(a.prior_mixture), "--prior-mixture")
        except ValueError as e:
            ap.error("--prior-mixture %s: %s" % (a.prior_mixture, e))
    # SNR pruning of the fitted posterior, behind every older check
    if a.prune_amounts is not None:
        if a.bayes != "mfvi":
            ap.error("--prune-amounts ranks the posterior of mean-field VI (--bayes mfvi); %s has no rho" % a.bayes)
        if not a.predict_samples:
            ap.error("--prune-amounts evaluates the pruned posterior by its predictive maps: it needs --predict-samples N (N >= 2)")
        if a.fits_per_launch or a.inpaint_fits or a.sibling_fits or a.ct_volume is not None:
            ap.error("--prune-amounts serves a single fit; for a batch call batch.predict(N, prune=...) (the batch drivers write no pruning file)")
        if a.param_dtype == "bf16":
            ap.error("--prune-amounts does not combine with --param-dtype bf16 (the pruning kernels read float32 parameter rows)")
        try:
            _check_prune(a.bayes, a.predict_samples, parse_prune_amounts(a.prune_amounts))
        except ValueError as e:
            ap.error("--prune-amounts %s: %s" % (a.prune_amounts, e))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="denoising", choices=["denoising", "super-resolution", "ct", "inpainting"])
    ap.add_argument("--bayes", default="mfvi", choices=["mfvi", "dip", "mcd", "sgld"])
    ap.add_argument("--config", required=True)
    ap.add_argument("--img", default=None, help="one image, or a comma-separated list: every (image, candidate) pair is one independent fit")
    ap.add_argument("--imsize", type=int, default=None)
    ap.add_argument("--k", type=int, default=1); ap.add_argument("--num-iter", type=int, default=None); ap.add_argument("--save-path", default=None)
    ap.add_argument("--devices", default=None, help="comma-separated devices (cuda:0,cuda:1,...): the independent fits are dealt round-robin to one "
                                                    "fresh worker process per device (default: the config's run_params.devices; absent: this process)")
    ap.add_argument("--param-dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--bo-rounds", type=int, default=0, help="> 0: the reference's Gaussian-process outer loop over the method's two hyper-parameters "
                                                             "(bo_params.<name>.logbounds of the config) for this many rounds, each round's candidates "
                                                             "run as independent fits (bo.py; parity unpinned: gpytorch is not available here)")
    ap.add_argument("--predict-samples", type=int, default=0, help="> 0: after the last iteration draw N posterior samples of the fit (mfvi, mcd) "
                                                                 "and write predictive.npz (mean, epi, ale, total, err2, mse_mc) beside save.npz")
    ap.add_argument("--calibration", action="store_true", help="write calibration.npz beside save.npz: per-bin calibration statistics and the "
                                                                "UCE of the run's uncertainty maps (mfvi, mcd, sgld), and of the posterior "
                                                                "predictive maps with --predict-samples")
    ap.add_argument("--calibration-bins", type=int, default=15)
    ap.add_argument("--batch-predict-samples", type=int, default=0, help="0 (off) or >= 2, with --fits-per-launch, --ct-volume, --inpaint-fits or --sibling-fits "
                                                                       "(--bayes mcd): after the last iteration of a batch draw N posterior samples of "
                                                                       "EVERY fit in one set of launches and write predictive_batch.npz beside batch.npz / "
                                                                       "volume.npz")
    ap.add_argument("--batch-calibration", action="store_true", help="with --batch-predict-samples: calibration_batch.npz, the calibration statistics of "
                                                                      "every fit's posterior predictive maps (--calibration-bins bins)")
    ap.add_argument("--batch-bookkeeping", action="store_true", help="with --fits-per-launch, --sibling-fits or --ct-volume: record what the single-fit "
                                                                     "runner records per iteration for EVERY fit of a batch (BatchBook) and write "
                                                                     "bookkeeping_batch.npz and fit_NNN/save.npz beside batch.npz / volume.npz")
    ap.add_argument("--fits-per-launch", type=int, default=0, help="> 0: the independent (image, candidate) fits run in batches of up to N as ONE "
                                                                   "set of launches per iteration (FitBatch; mfvi denoising / super-resolution); "
                                                                   "writes batch.npz per batch instead of save.npz per fit")
    ap.add_argument("--inpaint-fits", type=int, default=0, help="> 0 (--task inpainting --bayes mfvi): the independent (image, candidate) fits run in "
                                                                "batches of up to N as ONE set of launches per iteration (InpaintBatch); writes "
                                                                "batch.npz per batch instead of save.npz per fit")
    ap.add_argument("--sibling-fits", type=int, default=0, help="> 0 (--bayes dip, mcd or sgld; denoising / super-resolution): the independent (image, "
                                                                "candidate) fits run in batches of up to N as ONE set of launches per iteration "
                                                                "(SiblingBatch); writes batch.npz per batch instead of save.npz per fit")
    ap.add_argument("--ct-volume", default=None, help="--task ct --bayes mfvi: a .npy file holding a stack [D, S, S], or phantom:D; the slices are "
                                                         "fitted as ONE CtVolume per candidate (one set of launches per group of slices) and "
                                                         "volume.npz is written instead of save.npz per slice")
    ap.add_argument("--slices-per-launch", type=int, default=None, help="with --ct-volume: slices per set of launches (default: all of them)")
    ap.add_argument("--sr-downsampler", default=None, choices=["nearest", "lanczos2", "lanczos3"],
                    help="super-resolution (mfvi): the forward operator of the data term, the low-resolution target and the low-resolution "
                         "metrics; nearest = [::f, ::f] (default, or the config's run_params.downsampler), lanczos2 / lanczos3 = the "
                         "anti-aliasing Downsampler of the reference's models/downsampler.py")
    ap.add_argument("--tv-weight", type=float, default=None, help="> 0: add G * TV_beta of the reconstruction (the image channel of every MC sample) "
                                                                  "to the objective of every fit (all four methods; denoising, super-resolution, "
                                                                  "ct; default: the config's run_params.tv_weight, else off)")
    ap.add_argument("--tv-beta", type=float, default=None, help="the exponent of --tv-weight's term, (dh^2 + dw^2)^B per cell (default 0.5: isotropic TV)")
    ap.add_argument("--kl-type", default=None, choices=["reverse", "forward"],
                    help="--bayes mfvi: the direction of the KL term; reverse = KL(prior || posterior), what the reference's runners use "
                         "(default, or the config's run_params.kl_type), forward = KL(posterior || prior), the textbook ELBO's")
    ap.add_argument("--prior-mixture", default=None, metavar="PI:SIGMA[:MU],...",
                    help="--bayes mfvi with --kl-type forward: a scale mixture of 1 to 4 Gaussians as the prior of every weight, one PI:SIGMA[:MU] "
                         "per component (1e-6 is added to SIGMA; MU defaults to 0); the KL term becomes the one-draw Monte-Carlo estimate of "
                         "KL(posterior || mixture) (default: the config's run_params.prior_mixture, else the Gaussian prior)")
    ap.add_argument("--prune-amounts", default=None, metavar="A,B,...",
                    help="--bayes mfvi with --predict-samples N: after the fit, prune the given shares of the posterior's weights by signal-to-noise "
                         "ratio |mu| / sigma (a pruned COPY; the fit is untouched), evaluate the predictive maps under each and write pruning.npz "
                         "(default: the config's run_params.prune_amounts, else off)")
    a = ap.parse_args(argv)
    _check_cli(ap, a)
    cands, rp, cfg_devices = load_config(a.config, a.bayes, with_devices=True)
    short = {"denoising": "den", "super-resolution": "sr", "ct": "ct", "inpainting": "inp"}[a.task]
    fn_name = "run_%s_%s" % (short, a.bayes)
    fn = globals().get(fn_name)                # f(): bayesian_optimization.py:3709-3724
    if fn is None:
        raise NotImplementedError("run_%s_%s is not built" % (short, a.bayes))
    if a.imsize:
        rp["imsize"] = (a.imsize, a.imsize)
    if a.num_iter is not None:
        rp["num_iter"] = a.num_iter
    if a.save_path:
        rp["save_path"] = a.save_path
    rp["plot"] = False
    if a.param_dtype != "f32":
        rp["param_dtype"] = a.param_dtype
    if a.sr_downsampler is not None:
        rp["downsampler"] = a.sr_downsampler
    if rp.get("downsampler", "nearest") != "nearest" and a.fits_per_launch:
        ap.error("run_params.downsampler=%s does not combine with --fits-per-launch (batched fits project with [::f, ::f])" % rp["downsampler"])
    if a.predict_samples:
        rp["predict_samples"] = a.predict_samples
    if a.calibration:
        rp["calibration"] = True
        rp["calibration_bins"] = a.calibration_bins
    if a.batch_predict_samples:
        rp["batch_predict_samples"] = a.batch_predict_samples
        rp["batch_calibration_bins"] = a.calibration_bins if a.batch_calibration else 0
    if a.batch_bookkeeping:
        rp["batch_bookkeeping"] = True
    if a.tv_weight is not None:
        rp["tv_weight"] = a.tv_weight
    if a.tv_beta is not None:
        rp["tv_beta"] = a.tv_beta
    if a.kl_type is not None:
        rp["kl_type"] = a.kl_type
    if a.prior_mixture is not None:
        rp["prior_mixture"] = parse_prior_mixture(a.prior_mixture)
    if a.prune_amounts is not None:
        rp["prune_amounts"] = parse_prune_amounts(a.prune_amounts)
    if a.ct_volume is not None:      # one volume fit per candidate of the config
        from .fanout import print_table
        vrp = {k: v for k, v in rp.items() if k not in ("img", "plot", "p_sigma")}
        results = []
        for i, cand in enumerate(cands):
            r = run_ct_volume(a.ct_volume, slices_per_launch=a.slices_per_launch, K=a.k, verbose=True, **cand, **vrp)
            print("%s -> mean PSNR %.3f dB over %d live of %d slices in %.1f s (%s)" % (" ".join("%s %.3e" % kv for kv in cand.items()), r["mean_psnr"],
                                                                                      int((r["dead"] == 0).sum()), len(r["dead"]), r["seconds"], r["run_dir"]))
            results.append((i, cand, r["mean_psnr"]))
        print_table(results, list(BO_KEYS[a.bayes]))
        return results
    imgs = a.img.split(",") if a.img else [rp.pop("img", "phantom")]
    rp.pop("img", None)
    jobs = [dict(cand, img=im) for im in imgs for cand in cands]
    devices = a.devices.split(",") if a.devices else cfg_devices
    kind = next((k for k in BATCH_KINDS if getattr(a, k)), None)      # (the batching flags exclude one another: _check_cli)
    per = getattr(a, kind) if kind else 0
    if a.sibling_fits:      # the method rides in the run parameters to the batch function (here, or in a worker of the fan-out)
        rp["method"] = a.bayes
    if a.bo_rounds > 0:
        # bo() of the reference (bayesian_optimization.py:3727-3880): rounds of [fits of the candidates over the devices -> GP -> new candidates]
        from . import bo as _bo
        keys = BO_KEYS[a.bayes]
        if not keys or len(imgs) != 1:
            raise ValueError("--bo-rounds needs a method with two hyper-parameters (mfvi, mcd, sgld) and one image")
        bo_params = {k: json.load(open(a.config))["bo_params"][k] for k in keys}

        def evaluate(cand_list):
            jb = [dict(zip(keys, c), img=imgs[0]) for c in cand_list]
            if kind:      # a round's candidates form batches
                res, _, _ = _run_batches(short, jb, per, rp, a.k, devices, kind=kind)
                return [(tuple(job[k] for k in keys), y) for _, job, y in res]
            if devices:
                from .fanout import run_jobs
                res, _ = run_jobs(jb, devices, "mfvi_dip_mia_amd.runner:fit_job", dict(rp, fn_name=fn_name, K=a.k))
                return [(tuple(job[k] for k in keys), y) for _, job, y in res]
            return [(c, fn(K=a.k, verbose=False, **j, **rp)["psnr"]) for c, j in zip(cand_list, jb)]
        return _bo.bo(bo_params, evaluate, n_rounds=a.bo_rounds)
    if kind or devices:
        from .fanout import run_jobs, print_table
        if kind:
            results, dropped, batches = _run_batches(short, jobs, per, rp, a.k, devices, verbose=True, kind=kind)
            print("%d fits in %d batches of up to %d" % (len(jobs), len(batches), per))
        else:
            # independent fits over the node's GPUs (bayesian_optimization.py:3760-3781, eval_result.py:27-53): no per-step communication,
            # one final gather of (candidate, psnr), NaNs dropped
            results, dropped = run_jobs(jobs, devices, "mfvi_dip_mia_amd.runner:fit_job", dict(rp, fn_name=fn_name, K=a.k))
        print_table(results, list(BO_KEYS[a.bayes]))
        for i, job, why in dropped:
            print("dropped fit %d %s: %s" % (i, {k: v for k, v in job.items() if k != "img"}, why))
        return results
    out = []
    for job in jobs:
        r = fn(K=a.k, verbose=True, **job, **rp)
        cand = {k: v for k, v in job.items() if k != "img"}
        print("%s -> PSNR %.3f dB in %.1f s (%s)" % (" ".join("%s %.3e" % kv for kv in cand.items()) or "dip", r["psnr"], r["seconds"], r["run_dir"]))
        out.append(r)
    return out


if __name__ == "__main__":
    main()
