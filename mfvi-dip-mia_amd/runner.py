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
from .engine import ElboEngine, SiblingEngine

MC_ITER = 25            # ring-buffer length (bayesian_optimization.py:1314)
PREDICT_METHODS = ("mfvi", "mcd")      # methods whose fit is a posterior predict_samples can draw from (engine.ElboEngine.predict)
CALIBRATION_METHODS = ("mfvi", "mcd", "sgld")      # methods whose run carries uncertainty maps to calibrate (dip has none)
EXP_WEIGHT = 0.99       # EMA weight (:1292)


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


class _AsyncBook:
    """The per-iteration bookkeeping only READS the iteration's forward output, so it runs on a second stream beside the backward pass:
    `eng.step(after_forward=book.hook(eng, i, n))` enqueues it behind the forward, `book.wait()` (called by the next hook and by snapshot /
    results) orders the caller's stream behind it before `eng.out` is written again."""
    _side = None; _done = None

    def hook(self, eng, i, n=None):
        """-> the callable for eng.step(after_forward=...).  The engine passes the sample count of its LAST launch (eng.out holds only
        those; with K_local not a multiple of the launch size the last launch is partial), which overrides `n`."""
        def run(n_last=None):
            n_ = n if n_last is None else n_last
            t = self.t
            if self._side is None:
                self._side = t.cuda.Stream(); self._done = t.cuda.Event()
            main = t.cuda.current_stream()
            ready = t.cuda.Event(); ready.record(main)
            with t.cuda.stream(self._side):
                self._side.wait_event(ready)
                self.iteration(eng, i, n_)
                self._done.record(self._side)
        self.wait()          # the previous iteration's bookkeeping has read eng.out before this iteration's forward overwrites it
        return run

    def wait(self):
        if self._done is not None:
            self.t.cuda.current_stream().wait_event(self._done)


class _Book(_AsyncBook):
    """Device-side bookkeeping state of one den / sr / ct fit (bayesian_optimization.py:1374-1416, :2190-2236, :584-626).
    Column 0 of mse_noisy / psnrs / ssims is the 'corrupted' reference of the task: the noisy image (den), the low-resolution image
    against the [::f, ::f] projection of the output (sr: downsampler(out_avg) / out_lr, :2203-2218), the ground truth (ct)."""

    def __init__(self, eng, num_iter, gt, noisy_or_none, task="den", factor=4, downsampler="nearest"):
        import torch
        self.t = torch
        H, W, C = eng.H, eng.W, eng.out.shape[1]
        dev = "cuda"
        self.C, self.H, self.W, self.task, self.f = C, H, W, task, int(factor)
        self.ema = torch.zeros((C, H, W), device=dev)
        self.out_clip = torch.zeros((H, W), device=dev); self.ale_clip = torch.zeros((H, W), device=dev); self.avg_clip = torch.zeros((H, W), device=dev)
        self.ring_epi = torch.zeros((MC_ITER, H, W), device=dev); self.ring_ale = torch.zeros((MC_ITER, H, W), device=dev)
        self.metrics = torch.zeros((num_iter, 8), dtype=torch.float64, device=dev)     # mse_noisy, mse_gt, 3 psnr-mse, 3 ssim sums
        self.gt = torch.from_numpy(np.ascontiguousarray(gt, np.float32)).to(dev)
        self.noisy = None if noisy_or_none is None else torch.from_numpy(np.ascontiguousarray(noisy_or_none, np.float32)).to(dev)
        self.var = torch.zeros((H, W), device=dev); self.ale_mean = torch.zeros((H, W), device=dev)
        if task == "sr":      # img_small_torch = downsampler(img_torch) and the projections of out_avg / out (:2101, :2203, :2207)
            h, w = H // self.f, W // self.f
            self.taps = None
            if downsampler != "nearest":      # the run's `downsampler` is the Lanczos operator: project with it throughout
                from .downsampler import c_taps
                self.taps = c_taps(downsampler, self.f)
                self.gt_lr = torch.empty((h, w), device=dev)
                self._project(self.gt, self.gt_lr)
            else:
                self.gt_lr = self.gt[::self.f, ::self.f].contiguous()
            self.avg_lr = torch.zeros((h, w), device=dev); self.out_lr_clip = torch.zeros((h, w), device=dev)

    def _project(self, src, dst):
        """dst = downsampler(src) for one [H][W] map: [::f, ::f] (mfvi_decimate) or the run's Lanczos operator (mfvi_downsample)."""
        lib, sp, p = L.lib(), L.stream_ptr(), L.ptr
        if self.taps is None:
            L.check(lib.mfvi_decimate(p(src), self.H, self.W, self.f, p(dst), sp))
        else:
            L.check(lib.mfvi_downsample(p(src), 1, 1, self.H, self.W, self.f, self.taps[0], self.taps[1], p(dst), sp))

    def iteration(self, eng, i, n, lr_view=None):
        lib, sp, p = L.lib(), L.stream_ptr(), L.ptr
        slot = i % MC_ITER
        L.check(lib.mfvi_bookkeep(p(eng.out), n, self.C, self.H, self.W, p(self.ema), EXP_WEIGHT, int(i == 0), p(self.out_clip), p(self.ale_clip),
                                  p(self.avg_clip), p(self.ring_epi[slot]), p(self.ring_ale[slot]) if self.C > 1 else None, sp))
        m = self.metrics[i]
        hw = self.H * self.W
        avg0 = self.ema[0]
        if self.task == "sr":
            h, w = self.gt_lr.shape
            self._project(avg0, self.avg_lr)
            self._project(self.out_clip, self.out_lr_clip)      # nearest: clip and [::f, ::f] commute; Lanczos: downsampler(out) of the clipped output
            L.check(lib.mfvi_sq_err_sum(p(self.avg_lr), p(self.gt_lr), h * w, p(m[0:]), sp))         # mse(downsampler(out_avg)[:, :1], img_small)  :2203
            L.check(lib.mfvi_sq_err_sum(p(self.gt_lr), p(self.out_lr_clip), h * w, p(m[2:]), sp))    # psnr_lr                                       :2214
            L.check(lib.mfvi_ssim_sum(p(self.gt_lr), p(self.out_lr_clip), h, w, p(m[5:]), sp))       # ssim_lr                                       :2217
        else:
            ref_noisy = self.noisy if self.noisy is not None else self.gt                            # ct: both columns against the ground truth (:594-606)
            L.check(lib.mfvi_sq_err_sum(p(avg0), p(ref_noisy), hw, p(m[0:]), sp))                    # mse(out_avg[:, :1], noisy)  :1389
            L.check(lib.mfvi_sq_err_sum(p(ref_noisy), p(self.out_clip), hw, p(m[2:]), sp))           # psnr_corrupted              :1398
            L.check(lib.mfvi_ssim_sum(p(ref_noisy), p(self.out_clip), self.H, self.W, p(m[5:]), sp))
        L.check(lib.mfvi_sq_err_sum(p(avg0), p(self.gt), hw, p(m[1:]), sp))              # mse(out_avg[:, :1], gt)     :1390
        L.check(lib.mfvi_sq_err_sum(p(self.gt), p(self.out_clip), hw, p(m[3:]), sp))     # psnr_gt
        L.check(lib.mfvi_sq_err_sum(p(self.gt), p(self.avg_clip), hw, p(m[4:]), sp))     # psnr_gt_sm
        L.check(lib.mfvi_ssim_sum(p(self.gt), p(self.out_clip), self.H, self.W, p(m[6:]), sp))
        L.check(lib.mfvi_ssim_sum(p(self.gt), p(self.avg_clip), self.H, self.W, p(m[7:]), sp))

    def snapshot(self):
        self.wait()
        lib, sp, p = L.lib(), L.stream_ptr(), L.ptr
        L.check(lib.mfvi_ring_stats(p(self.ring_epi), MC_ITER, self.H, self.W, p(self.var), None, sp))
        if self.C > 1:
            L.check(lib.mfvi_ring_stats(p(self.ring_ale), MC_ITER, self.H, self.W, None, p(self.ale_mean), sp))
        return self.var.cpu().numpy(), self.ale_mean.cpu().numpy(), self.avg_clip.cpu().numpy()

    def results(self):
        self.wait()
        m = self.metrics.cpu().numpy(); hw = float(self.H * self.W)
        n = np.full(8, hw)
        if self.task == "sr":
            n[[0, 2, 5]] = float(self.gt_lr.numel())
        m = m / n
        with np.errstate(divide="ignore"):
            psnrs = 10.0 * np.log10(1.0 / m[:, 2:5])
        return m[:, 0], m[:, 1], psnrs, m[:, 5:8]


class _BookInp(_AsyncBook):
    """Device-side bookkeeping of the inpainting runner (bayesian_optimization.py:3039-3090): sigmoid colour channels, masked PSNR / SSIM."""

    def __init__(self, eng, num_iter, img, mask):
        import torch
        self.t = torch
        dev = "cuda"
        H, W = eng.H, eng.W
        self.H, self.W = H, W
        self.img = torch.from_numpy(np.ascontiguousarray(img, np.float32)).to(dev)
        self.mask = torch.from_numpy(np.ascontiguousarray(mask, np.float32)).to(dev).round()
        self.mc = self.mask.shape[0]
        self.ema = torch.zeros((4, H, W), device=dev)
        self.out_clip = torch.zeros((3, H, W), device=dev); self.avg_clip = torch.zeros_like(self.out_clip); self.ale_clip = torch.zeros((H, W), device=dev)
        self.img_m = torch.zeros_like(self.out_clip); self.out_m = torch.zeros_like(self.out_clip); self.avg_m = torch.zeros_like(self.out_clip)
        self.ring_epi = torch.zeros((MC_ITER, 3, H, W), device=dev); self.ring_ale = torch.zeros((MC_ITER, H, W), device=dev)
        self.metrics = torch.zeros((num_iter, 10, 3), dtype=torch.float64, device=dev)      # per channel: mse, 3 psnr-mse, 3 ssim sums (+ spare)
        self.var = torch.zeros((3, H, W), device=dev); self.ale_mean = torch.zeros((H, W), device=dev)

    def iteration(self, eng, i, n):
        lib, p, sp = L.lib(), L.ptr, L.stream_ptr()
        H, W = self.H, self.W; HW = H * W; slot = i % MC_ITER
        L.check(lib.mfvi_bookkeep_inpainting(p(eng.out), n, H, W, p(self.img), p(self.mask), self.mc, p(self.ema), EXP_WEIGHT, int(i == 0),
                                             p(self.out_clip), p(self.ale_clip), p(self.avg_clip), p(self.img_m), p(self.out_m), p(self.avg_m),
                                             p(self.ring_epi[slot]), p(self.ring_ale[slot]), sp))
        m = self.metrics[i]
        for c in range(3):                                            # channel-wise sums; means over the 3 channels taken on the host
            L.check(lib.mfvi_sq_err_sum(p(self.ema[c]), p(self.img[c]), HW, p(m[0, c:]), sp))            # mse(out_avg[:, :3], img)        :3051-3052
            L.check(lib.mfvi_sq_err_sum(p(self.img[c]), p(self.out_clip[c]), HW, p(m[1, c:]), sp))       # psnr_corrupted                  :3062
            L.check(lib.mfvi_sq_err_sum(p(self.img_m[c]), p(self.out_m[c]), HW, p(m[2, c:]), sp))        # psnr_gt (masked)                :3063
            L.check(lib.mfvi_sq_err_sum(p(self.img_m[c]), p(self.avg_m[c]), HW, p(m[3, c:]), sp))        # psnr_gt_sm
            L.check(lib.mfvi_ssim_sum(p(self.img[c]), p(self.out_clip[c]), H, W, p(m[4, c:]), sp))
            L.check(lib.mfvi_ssim_sum(p(self.img_m[c]), p(self.out_m[c]), H, W, p(m[5, c:]), sp))
            L.check(lib.mfvi_ssim_sum(p(self.img_m[c]), p(self.avg_m[c]), H, W, p(m[6, c:]), sp))

    def snapshot(self):
        self.wait()
        lib, p, sp = L.lib(), L.ptr, L.stream_ptr()
        for c in range(3):
            L.check(lib.mfvi_ring_stats(p(self.ring_epi[:, c].contiguous()), MC_ITER, self.H, self.W, p(self.var[c]), None, sp))
        L.check(lib.mfvi_ring_stats(p(self.ring_ale), MC_ITER, self.H, self.W, None, p(self.ale_mean), sp))
        return self.var.cpu().numpy(), self.ale_mean.cpu().numpy(), self.avg_clip.cpu().numpy()

    def results(self):
        self.wait()
        mt = self.metrics.cpu().numpy().mean(axis=2) / (self.H * self.W)      # mean over the colour channels == mean over all 3*H*W elements
        with np.errstate(divide="ignore"):
            psnrs = 10.0 * np.log10(1.0 / mt[:, 1:4])
        return mt[:, 0], mt[:, 0], psnrs, mt[:, 4:7]                          # the reference computes both MSEs against img_torch (:3051-3052)


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


def _run(task, img, imsize, p_sigma, num_iter, lr, temp, sigma, input_depth, seed, show_every, plot, save, save_path, K, factor=4,
         theta_step=4.0, verbose=False, net_kwargs=None, method="mfvi", weight_decay=0.0, dropout_p=0.3, gamma=0.996, param_dtype="f32", predict_samples=0,
         calibration=False, calibration_bins=15, downsampler="nearest", **unused):
    import torch
    _check_downsampler(task, method, downsampler, factor)
    _check_predict(method, predict_samples)
    _check_calibration(method, calibration, calibration_bins)
    sib = dict(weight_decay=weight_decay, dropout_p=dropout_p, gamma=gamma)
    timestamp = str(time.time())
    run_dir = os.path.join(save_path, timestamp)
    if save:
        os.makedirs(run_dir, exist_ok=False)
        with open(os.path.join(run_dir, "locals.txt"), "w") as f:
            hyper = dict(temp=temp, sigma=sigma) if method == "mfvi" else {"dip": {}, "mcd": dict(dropout_p=dropout_p, weight_decay=weight_decay),
                                                                          "sgld": dict(gamma=gamma, weight_decay=weight_decay)}[method]
            for key, val in dict(task=task, method=method, img=img if not isinstance(img, np.ndarray) else "<array>", imsize=imsize, p_sigma=p_sigma,
                                 num_iter=num_iter, lr=lr, input_depth=input_depth, seed=seed, show_every=show_every,
                                 K=K, save_path=save_path, **(dict(downsampler=downsampler) if task == "sr" else {}), **hyper).items():
                print(key, "=", val, file=f)
    img_np = _load_image(img, imsize, seed)
    H, W = img_np.shape
    num_iter += 1                                                    # bayesian_optimization.py:1291
    extra = {}
    noisy = None
    if task == "den":
        rng = np.random.default_rng(seed + 1)
        noisy = np.clip(img_np + rng.normal(scale=p_sigma, size=img_np.shape), 0, 1).astype(np.float32)      # denoising_utils.py:11
        target = noisy
        eng = _make_engine(method, H, W, "den", K, input_depth, temp, sigma, lr, seed, net_kwargs, sib, param_dtype=param_dtype)
    elif task == "sr":
        noisy = None
        if downsampler != "nearest":      # img_small = downsampler(img_hr) with the run's operator (models/downsampler.py)
            from .downsampler import downsample
            eng = _make_engine(method, H, W, "sr", K, input_depth, temp, sigma, lr, seed, net_kwargs, sib, sr_factor=factor, param_dtype=param_dtype,
                               downsampler=downsampler)
            target = downsample(torch.from_numpy(img_np).cuda(), downsampler, factor).cpu().numpy()
        else:
            target = np.ascontiguousarray(img_np[::factor, ::factor])    # nearest /factor decimation (:2095-2099)
            eng = _make_engine(method, H, W, "sr", K, input_depth, temp, sigma, lr, seed, net_kwargs, sib, sr_factor=factor, param_dtype=param_dtype)
        extra["img_lr"] = target
    else:
        theta = np.arange(0, 180.0, theta_step, dtype=np.float32)     # :545
        eng = _make_engine(method, H, W, "ct", K, input_depth, temp, sigma, lr, seed, net_kwargs, sib, theta_deg=theta.tolist())
        sino = torch.empty((len(theta), W), device="cuda")
        gt_d = torch.from_numpy(img_np).cuda()
        L.check(L.lib().mfvi_radon_forward(L.ptr(gt_d), L.ptr(eng.theta), 1, H, W, len(theta), L.ptr(sino), L.stream_ptr()))
        target = sino
        extra["img_radon"] = sino.cpu().numpy()[None, None]
    eng.set_target(torch.from_numpy(target) if isinstance(target, np.ndarray) else target)
    book = _Book(eng, num_iter, img_np, noisy, task=task, factor=factor, downsampler=downsampler)
    n_snap = num_iter // show_every + 1
    recons = np.zeros((n_snap, 1, H, W)); uncerts_epi = np.zeros((n_snap, 1, H, W)); uncerts_ale = np.zeros((n_snap, 1, H, W))
    t0 = time.perf_counter()
    for i in range(num_iter):
        # one fused ELBO iteration (a non-finite loss skips the update on the device: engine.step); the bookkeeping of :1374-1406 reads only the
        # iteration's forward output and runs on a second stream beside the backward pass
        eng.step(after_forward=book.hook(eng, i, eng.chunk))
        if i % show_every == 0:
            var, ale, recon = book.snapshot()
            uncerts_epi[i // show_every, 0] = var; uncerts_ale[i // show_every, 0] = ale; recons[i // show_every, 0] = recon
            if verbose:
                nll, kl, loss = eng.losses()
                print("iter %6d  loss %.5f  nll %.5f  kl %.4e  (%.1f it/s)" % (i, loss, nll, kl, (i + 1) / (time.perf_counter() - t0)))
            if plot and save:                                        # loss_<method>.png, out_avg.png, out_var.png, out_ale.png (:1418-1422)
                mn, mg, ps_, _ = book.results()
                A.snapshot_pngs(run_dir, method, i, mn, mg, ps_, recon[None], None if method == "dip" else var[None],
                                None if (method == "dip" or task == "ct") else ale[None])
    pred = _predict(eng, predict_samples, img_np, run_dir if save else None, drop_ale=task == "ct",
                    calibration_bins=calibration_bins if calibration else 0) if predict_samples else None
    cal = _calibrate(run_dir if save else None, img_np, recons, uncerts_epi, uncerts_ale, pred.pop("_calibration") if pred else None,
                     calibration_bins) if calibration else None
    torch.cuda.synchronize()
    mse_noisy, mse_gt, psnrs, ssims = book.results()
    if save:
        # first two keys as the reference writes them per task: den img_gt / img_noisy (:1438), sr img_hr / img_lr (:2258), ct img_gt / img_radon (:643)
        # with the reference's shapes: get_image() arrays are (1, H, W), img_lr is squeezed, the CT tensors keep (1, 1, ., .)
        head = dict(den=(img_np[None], None if noisy is None else noisy[None]), sr=(img_np[None], extra.get("img_lr")),
                    ct=(img_np[None, None], extra.get("img_radon")))[task]
        A.save_npz(run_dir, task, method, head, mse_noisy, mse_gt, recons, uncerts_epi, uncerts_ale, psnrs, ssims)
        with open(os.path.join(run_dir, "locals.txt"), "a") as f:
            print("max psnr_gt_sm = %.4f, max ssim_gt_sm = %.4f" % (np.nanmax(psnrs[:, 2]), np.nanmax(ssims[:, 2])), file=f)
            if plot:                                                  # mse_noisy / mse_gt / psnrs / ssims .png + the maxima lines (:201-258, :1431-1433)
                A.plot_results({method: mse_noisy}, {method: mse_gt}, {method: psnrs}, {method: ssims}, run_dir, f)
        if plot and task == "sr":
            A.sr_input_png(run_dir, img_np[None], extra["img_lr"], factor)
    res = dict(psnr=float(psnrs[-1, 2]), run_dir=run_dir if save else None, psnrs=psnrs, ssims=ssims, mse_noisy=mse_noisy, mse_gt=mse_gt,
               recons=recons, uncerts=uncerts_epi, uncerts_ale=uncerts_ale, seconds=time.perf_counter() - t0, engine=eng)
    if pred is not None:
        res["predictive"] = pred
    if cal is not None:
        res["calibration"] = cal
    return res


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
                 weight_decay=1e-4, dropout_p=0.2, gamma=0.996, predict_samples=0, calibration=False, calibration_bins=15, **unused):
    """bayesian_optimization.py:2892-3114: inpainting with the 6-scale no-skip net (5x5 down filters, nearest up-sampling), sigmoid on
    the colour channels, masked Gaussian NLL.  img: (3, H, W) array in [0, 1] or 'phantom' (three synthetic planes); mask: (1|3, H, W),
    1 = known pixel (the reference ships its masks in data/inpainting/).  save.npz carries the reference's keys for this task
    (img_inpainting, img_mask, mse_corrupted, mse_gt, recons, uncerts, uncerts_ale, psnrs, ssims)."""
    import torch
    _check_downsampler("inp", method, unused.get("downsampler", "nearest"))
    _check_predict(method, predict_samples)
    _check_calibration(method, calibration, calibration_bins)
    timestamp = str(time.time())
    run_dir = os.path.join(save_path, timestamp)
    if save:
        os.makedirs(run_dir, exist_ok=False)
        with open(os.path.join(run_dir, "locals.txt"), "w") as f:
            for key, val in dict(task="inp", imsize=imsize, num_iter=num_iter, lr=lr, temp=temp, sigma=sigma, input_depth=input_depth,
                                 seed=seed, show_every=show_every, K=K, save_path=save_path).items():
                print(key, "=", val, file=f)
    if isinstance(img, np.ndarray):
        img_np = np.ascontiguousarray(img, np.float32)
    else:
        img_np = np.stack([_load_image(img, imsize, seed + c) for c in range(3)]).astype(np.float32)
    _, H, W = img_np.shape
    if mask is None:
        mask = scratch_mask(H, W, seed)
    mask_np = np.ascontiguousarray(mask, np.float32)
    if mask_np.ndim == 2:
        mask_np = mask_np[None]
    num_iter += 1                                                     # bayesian_optimization.py:2935
    eng = _make_engine(method, H, W, "inp", K, input_depth, temp, sigma, lr, seed, net_kwargs, dict(weight_decay=weight_decay, dropout_p=dropout_p, gamma=gamma))
    eng.set_target(torch.from_numpy(img_np), torch.from_numpy(mask_np))
    book = _BookInp(eng, num_iter, img_np, mask_np)
    n_snap = num_iter // show_every + 1
    recons = np.zeros((n_snap, 3, H, W)); uncerts_epi = np.zeros((n_snap, 3, H, W)); uncerts_ale = np.zeros((n_snap, 1, H, W))
    t0 = time.perf_counter()
    for i in range(num_iter):
        eng.step(after_forward=book.hook(eng, i, eng.chunk))
        if i % show_every == 0:
            var, ale, recon = book.snapshot()
            uncerts_epi[i // show_every] = var; uncerts_ale[i // show_every, 0] = ale; recons[i // show_every] = recon
            if verbose:
                nll, kl, loss = eng.losses()
                print("iter %6d  loss %.5f  nll %.5f  kl %.4e  (%.1f it/s)" % (i, loss, nll, kl, (i + 1) / (time.perf_counter() - t0)))
    pred = _predict(eng, predict_samples, img_np, run_dir if save else None,
                    calibration_bins=calibration_bins if calibration else 0) if predict_samples else None
    cal = _calibrate(run_dir if save else None, img_np, recons, uncerts_epi, uncerts_ale, pred.pop("_calibration") if pred else None,
                     calibration_bins, mask=mask_np) if calibration else None
    torch.cuda.synchronize()
    mse_corrupted, mse_gt, psnrs, ssims = book.results()
    if save:
        A.save_npz(run_dir, "inp", method, (img_np, mask_np), mse_corrupted, mse_gt, recons, uncerts_epi, uncerts_ale, psnrs, ssims)
        with open(os.path.join(run_dir, "locals.txt"), "a") as f:
            print("max psnr_gt_sm = %.4f, max ssim_gt_sm = %.4f" % (np.nanmax(psnrs[:, 2]), np.nanmax(ssims[:, 2])), file=f)
            if plot:
                A.plot_results({method: mse_corrupted}, {method: mse_gt}, {method: psnrs}, {method: ssims}, run_dir, f)
        if plot:
            A.snapshot_pngs(run_dir, method, num_iter - 1, mse_corrupted, mse_gt, psnrs, recons[-1], None if method == "dip" else uncerts_epi[-1],
                            None if method == "dip" else uncerts_ale[-1])
    res = dict(psnr=float(psnrs[-1, 2]), run_dir=run_dir if save else None, psnrs=psnrs, ssims=ssims, mse_corrupted=mse_corrupted, mse_gt=mse_gt,
               recons=recons, uncerts=uncerts_epi, uncerts_ale=uncerts_ale, seconds=time.perf_counter() - t0, engine=eng)
    if pred is not None:
        res["predictive"] = pred
    if cal is not None:
        res["calibration"] = cal
    return res


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


def run_fit_batch(task, jobs, imsize=(256, 256), p_sigma=0.1, num_iter=5000, lr=3e-4, input_depth=16, seed=42, show_every=100, save=True,
                  save_path="../logs", K=1, factor=4, net_kwargs=None, verbose=False, autotune=True, batch_predict_samples=0,
                  batch_calibration_bins=0, batch_bookkeeping=False, **unused):
    """The (image, temp, sigma) jobs of one batch as ONE FitBatch (--fits-per-launch): the loop of run_den_mfvi /
    run_sr_mfvi for every job at once, every fit with the noise of its own RNG samples.  jobs: dicts with img, temp, sigma (and optionally
    lr).  Writes batch.npz (hyper-parameters; per fit psnr_gt_sm, nll and kl every show_every iterations, the final reconstruction, dead);
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
    F = len(jobs)
    imgs = [_load_image(j["img"], imsize, seed) for j in jobs]
    H, W = imgs[0].shape
    if any(im.shape != (H, W) for im in imgs):
        raise ValueError("the images of one batch must share their size")
    gt = np.stack(imgs)
    if task == "den":      # every job's noise as the single-fit runner draws it (same image and seed: the same noisy image)
        targets = np.stack([np.clip(im + np.random.default_rng(seed + 1).normal(scale=p_sigma, size=im.shape), 0, 1).astype(np.float32) for im in imgs])
    else:
        targets = np.ascontiguousarray(gt[:, ::factor, ::factor])
    temps, sigmas, lrs = [j["temp"] for j in jobs], [j["sigma"] for j in jobs], [j.get("lr", lr) for j in jobs]
    fb = FitBatch(H, W, F, task=task, K=K, input_depth=input_depth, temp=temps, sigma=sigmas, lr=lrs, seed=seed, sr_factor=factor,
                  net_kwargs=net_kwargs, init="shared", autotune=autotune)      # the reference's candidates all start from one seed
    fb.set_targets(torch.from_numpy(targets))
    n_it = num_iter + 1                                               # bayesian_optimization.py:1291
    book = fb.track(gt, n_it, noisy=targets if task == "den" else None) if batch_bookkeeping else None      # 
    at, psnrs, nlls, kls = [], [], [], []
    t0 = time.perf_counter()
    for i in range(n_it):
        fb.step()
        if book is not None and i % show_every == 0:
            book.snapshot()
        if i % show_every == 0 or i == n_it - 1:
            nll, kl, _ = fb.losses()
            at.append(i); psnrs.append(fb.psnr(gt)); nlls.append(nll); kls.append(kl)
            if verbose:
                print("iter %6d  psnr_gt_sm %s  (%.1f it/s x %d fits)" % (i, np.array2string(psnrs[-1], precision=2), (i + 1) / (time.perf_counter() - t0), F))
    dead = fb.dead
    final = np.where(dead != 0, np.nan, psnrs[-1])
    run_dir = None
    if save:
        run_dir = os.path.join(save_path, "%s_batch" % time.time())
        os.makedirs(run_dir, exist_ok=False)
        np.savez(os.path.join(run_dir, "batch.npz"), task=task, temp=np.asarray(temps), sigma=np.asarray(sigmas), lr=np.asarray(lrs),
                 prior_sigma=np.asarray(fb.prior_sigma), K=np.int64(K), seed=np.int64(seed), num_iter=np.int64(num_iter), iterations=np.asarray(at),
                 psnr_gt_sm=np.stack(psnrs), nll=np.stack(nlls), kl=np.stack(kls), recon=fb.recon().cpu().numpy(), dead=dead)
        if book is not None:
            _save_bookkeeping(book, run_dir, [(gt[f][None], targets[f][None] if task == "den" else targets[f]) for f in range(F)])
    pred = _batch_predict(fb, batch_predict_samples, gt, run_dir, batch_calibration_bins) if batch_predict_samples else None
    return dict(psnr=[float(x) for x in final], run_dir=run_dir, seconds=time.perf_counter() - t0, batch=fb, dead=dead, predictive=pred)


def fit_batch_job(task, jobs, **kw):
    """One batch of fits in a worker process of the fan-out -> the PSNR of every fit."""
    return run_fit_batch(task, jobs, **kw)["psnr"]


def run_inpaint_batch(jobs, imsize=(256, 256), num_iter=5000, lr=2e-3, input_depth=32, seed=42, show_every=100, save=True, save_path="../logs",
                      K=1, net_kwargs=None, verbose=False, autotune=True, mask=None, batch_predict_samples=0, batch_calibration_bins=0, **unused):
    """The (image, mask, temp, sigma) jobs of one batch as ONE InpaintBatch (--inpaint-fits): the loop of run_inp_mfvi for
    every job at once.  jobs: dicts with img ((3, H, W) array, or what run_inp_mfvi loads), temp, sigma and optionally mask ((1|3, H, W);
    absent: `mask`, the run_params' mask that run_inp_mfvi takes too, else that function's seeded scratch mask) and lr.
    Writes batch.npz with the keys of run_fit_batch plus mask, recon [F, 3, H, W] and
    ale [F, H, W]; save.npz and the PNG artefacts stay with the single-fit runner.  Returns dict(psnr=[per fit, NaN for a dead fit], ...)."""
    import torch
    from .inpaintbatch import InpaintBatch
    _check_batch_predict(batch_predict_samples, batch_calibration_bins)
    F = len(jobs)
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
    gt, mask = np.stack(imgs), np.stack(masks)
    temps, sigmas, lrs = [j["temp"] for j in jobs], [j["sigma"] for j in jobs], [j.get("lr", lr) for j in jobs]
    ib = InpaintBatch(H, W, F, K=K, input_depth=input_depth, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=net_kwargs, init="shared",
                      autotune=autotune)                               # the reference's candidates all start from one seed
    ib.set_targets(torch.from_numpy(gt), torch.from_numpy(mask))
    n_it = num_iter + 1                                               # bayesian_optimization.py:2935
    at, psnrs, nlls, kls = [], [], [], []
    t0 = time.perf_counter()
    for i in range(n_it):
        ib.step()
        if i % show_every == 0 or i == n_it - 1:
            nll, kl, _ = ib.losses()
            at.append(i); psnrs.append(ib.psnr(gt)); nlls.append(nll); kls.append(kl)
            if verbose:
                print("iter %6d  psnr_gt_sm %s  (%.1f it/s x %d fits)" % (i, np.array2string(psnrs[-1], precision=2), (i + 1) / (time.perf_counter() - t0), F))
    dead = ib.dead
    final = np.where(dead != 0, np.nan, psnrs[-1])
    run_dir = None
    if save:
        run_dir = os.path.join(save_path, "%s_batch" % time.time())
        os.makedirs(run_dir, exist_ok=False)
        np.savez(os.path.join(run_dir, "batch.npz"), task="inp", temp=np.asarray(temps), sigma=np.asarray(sigmas), lr=np.asarray(lrs),
                 prior_sigma=np.asarray(ib.prior_sigma), K=np.int64(K), seed=np.int64(seed), num_iter=np.int64(num_iter), iterations=np.asarray(at),
                 psnr_gt_sm=np.stack(psnrs), nll=np.stack(nlls), kl=np.stack(kls), recon=ib.recon().cpu().numpy(), dead=dead,
                 mask=ib.masks.cpu().numpy(), ale=ib.ale().cpu().numpy())
    pred = _batch_predict(ib, batch_predict_samples, gt, run_dir, batch_calibration_bins) if batch_predict_samples else None      # (as batch.npz)
    return dict(psnr=[float(x) for x in final], run_dir=run_dir, seconds=time.perf_counter() - t0, batch=ib, dead=dead, predictive=pred)


def inpaint_batch_job(task, jobs, **kw):
    """One batch of inpainting fits in a worker process of the fan-out -> the PSNR of every fit."""
    return run_inpaint_batch(jobs, **kw)["psnr"]


def run_sibling_batch(task, method, jobs, imsize=None, p_sigma=0.1, num_iter=5000, lr=None, input_depth=None, seed=42, show_every=100, save=True,
                      save_path="../logs", K=1, factor=4, net_kwargs=None, verbose=False, autotune=True, param_noise_sigma=2.0,
                      batch_predict_samples=0, batch_calibration_bins=0, batch_bookkeeping=False, **unused):
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
    F = len(jobs)
    imgs = [_load_image(j["img"], imsize, seed) for j in jobs]
    H, W = imgs[0].shape
    if any(im.shape != (H, W) for im in imgs):
        raise ValueError("the images of one batch must share their size")
    gt = np.stack(imgs)
    if task == "den":      # every job's noise as the single-fit runner draws it (same image and seed: the same noisy image)
        targets = np.stack([np.clip(im + np.random.default_rng(seed + 1).normal(scale=p_sigma, size=im.shape), 0, 1).astype(np.float32) for im in imgs])
    else:
        targets = np.ascontiguousarray(gt[:, ::factor, ::factor])
    hyper = {k: [j.get(k, dflt.get(k, d)) for j in jobs] for k, d in (("weight_decay", 0.0), ("dropout_p", 0.3), ("gamma", 0.996))}
    lrs = [j.get("lr", lr) for j in jobs]
    sb = SiblingBatch(H, W, F, method, task=task, K=K, input_depth=input_depth, lr=lrs, seed=seed, sr_factor=factor, net_kwargs=net_kwargs,
                      param_noise_sigma=param_noise_sigma, init="shared", autotune=autotune, **hyper)      # the reference's candidates all start from one seed
    sb.set_targets(torch.from_numpy(targets))
    n_it = num_iter + 1                                               # bayesian_optimization.py:1291
    book = sb.track(gt, n_it, noisy=targets if task == "den" else None) if batch_bookkeeping else None      # 
    at, psnrs, losses = [], [], []
    t0 = time.perf_counter()
    for i in range(n_it):
        sb.step()
        if book is not None and i % show_every == 0:
            book.snapshot()
        if i % show_every == 0 or i == n_it - 1:
            at.append(i); psnrs.append(sb.psnr(gt)); losses.append(sb.losses())
            if verbose:
                print("iter %6d  psnr_gt_sm %s  (%.1f it/s x %d fits)" % (i, np.array2string(psnrs[-1], precision=2), (i + 1) / (time.perf_counter() - t0), F))
    dead = sb.dead
    final = np.where(dead != 0, np.nan, psnrs[-1])
    run_dir = None
    if save:
        run_dir = os.path.join(save_path, "%s_batch" % time.time())
        os.makedirs(run_dir, exist_ok=False)
        np.savez(os.path.join(run_dir, "batch.npz"), method=method, task=task, lr=np.asarray(lrs), weight_decay=np.asarray(sb.weight_decays),
                 dropout_p=np.asarray(sb.dropout_ps), gamma=np.asarray(sb.gammas), K=np.int64(K), seed=np.int64(seed), num_iter=np.int64(num_iter),
                 iterations=np.asarray(at), psnr_gt_sm=np.stack(psnrs), loss=np.stack(losses), recon=sb.recon().cpu().numpy(), dead=dead)
        if book is not None:
            _save_bookkeeping(book, run_dir, [(gt[f][None], targets[f][None] if task == "den" else targets[f]) for f in range(F)])
    pred = _batch_predict(sb, batch_predict_samples, gt, run_dir, batch_calibration_bins) if batch_predict_samples else None
    return dict(psnr=[float(x) for x in final], run_dir=run_dir, seconds=time.perf_counter() - t0, batch=sb, dead=dead, predictive=pred)


def sibling_batch_job(task, jobs, method="dip", **kw):
    """One batch of sibling fits in a worker process of the fan-out -> the PSNR of every fit."""
    return run_sibling_batch(task, method, jobs, **kw)["psnr"]


def _sibling_batches(task, jobs, method="dip", **kw):
    return run_sibling_batch(task, method, jobs, **kw)


def _fit_batches(task, jobs, **kw):
    return run_fit_batch(task, jobs, **kw)


def _inpaint_batches(task, jobs, **kw):
    return run_inpaint_batch(jobs, **kw)


def _run_batches(task, jobs, n, rp, K, devices, verbose=False, batch_fn=_fit_batches, worker="mfvi_dip_mia_amd.runner:fit_batch_job"):
    """jobs -> batches of up to n (fanout.group_jobs) -> one batch_fn(task, jobs, ...) each (a FitBatch, or an InpaintBatch), here or dealt
    round-robin to one worker per device.  Returns (results [(job index, job, psnr)], dropped [(job index, job, why)], batches)."""
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
                per_batch[bi] = (batch_fn(task, bj["jobs"], K=K, verbose=verbose, **rp)["psnr"], None)
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
                  batch_calibration_bins=0, batch_bookkeeping=False, **unused):
    """The loop of run_ct_mfvi (bayesian_optimization.py:442-648) for every slice of a stack at once, as ONE CtVolume (--ct-volume; DESIGN.md
    section 16).  volume: [D, S, S] array, .npy path or 'phantom:D'; temp / sigma / lr: scalars or one value per slice.  Writes volume.npz
    (angles, sinograms, hyper-parameters; per slice psnr_gt_sm, nll and kl every show_every iterations, the reconstruction, dead); the ring
    buffers, SSIM curves, save.npz and PNG artefacts stay with the single-fit runner unless batch_bookkeeping (bookkeeping_batch.npz and
    fit_%03d/save.npz per slice, _save_bookkeeping; no PNGs).  Returns dict(psnr=[per slice, NaN for a dead one], ...)."""
    import torch
    from .ctvolume import CtVolume
    _check_batch_predict(batch_predict_samples, batch_calibration_bins)
    gt = _load_volume(volume, imsize, seed)
    D, S = gt.shape[0], gt.shape[1]
    theta = np.arange(0, 180.0, theta_step, dtype=np.float32)         # :545
    vol = CtVolume(S, D, slices_per_launch=slices_per_launch, K=K, input_depth=input_depth, temp=temp, sigma=sigma, lr=lr, theta_deg=theta.tolist(),
                   seed=seed, net_kwargs=net_kwargs, autotune=autotune)
    vol.set_volume(torch.from_numpy(gt))                              # img_radon = forward_radon(img_torch) (:547)
    n_it = num_iter + 1                                               # as the single-fit runners count
    book = vol.track(gt, n_it) if batch_bookkeeping else None          # 
    at, psnrs, nlls, kls = [], [], [], []
    t0 = time.perf_counter()
    for i in range(n_it):
        vol.step()
        if book is not None and i % show_every == 0:
            book.snapshot()
        if i % show_every == 0 or i == n_it - 1:
            nll, kl, _ = vol.losses()
            at.append(i); psnrs.append(vol.psnr(gt)); nlls.append(nll); kls.append(kl)
            if verbose:
                print("iter %6d  psnr_gt_sm %s  (%.1f it/s x %d slices)" % (i, np.array2string(psnrs[-1], precision=2), (i + 1) / (time.perf_counter() - t0), D))
    dead = vol.dead
    final = np.where(dead != 0, np.nan, psnrs[-1])
    run_dir = None
    if save:
        run_dir = os.path.join(save_path, "%s_volume" % time.time())
        os.makedirs(run_dir, exist_ok=False)
        np.savez(os.path.join(run_dir, "volume.npz"), theta=theta, sinograms=vol.sinos.cpu().numpy(), temp=np.asarray(vol.temps), sigma=np.asarray(vol.sigmas),
                 lr=np.asarray(vol.lrs), prior_sigma=np.asarray(vol.prior_sigma), K=np.int64(K), seed=np.int64(seed), num_iter=np.int64(num_iter),
                 slices_per_launch=np.int64(vol.F), iterations=np.asarray(at), psnr_gt_sm=np.stack(psnrs), nll=np.stack(nlls), kl=np.stack(kls),
                 recon=vol.recon().cpu().numpy(), dead=dead)
        if book is not None:      # heads as run_ct_mfvi writes them: img_gt (1, 1, S, S), img_radon (1, 1, T, S)
            sinos = vol.sinos.cpu().numpy()
            _save_bookkeeping(book, run_dir, [(gt[d][None, None], sinos[d][None, None]) for d in range(D)])
    pred = _batch_predict(vol, batch_predict_samples, gt, run_dir, batch_calibration_bins) if batch_predict_samples else None
    live = final[dead == 0]
    return dict(psnr=[float(x) for x in final], mean_psnr=float(live.mean()) if live.size else float("nan"), run_dir=run_dir,
                seconds=time.perf_counter() - t0, volume=vol, dead=dead, predictive=pred)


def fit_job(fn_name, **kw):
    """One independent fit in a worker process of the fan-out: run_<task>_<method>(**kw) -> PSNR (the reference's return value)."""
    return globals()[fn_name](**kw)["psnr"]


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
    a = ap.parse_args(argv)
    if a.sr_downsampler not in (None, "nearest"):      # refused before anything loads the library
        if a.task != "super-resolution" or a.bayes != "mfvi":
            ap.error("--sr-downsampler %s belongs to --task super-resolution --bayes mfvi" % a.sr_downsampler)
        if a.fits_per_launch:
            ap.error("--sr-downsampler %s does not combine with --fits-per-launch (batched fits project with [::f, ::f])" % a.sr_downsampler)
    if a.batch_bookkeeping and not (a.fits_per_launch > 0 or a.sibling_fits > 0 or a.ct_volume is not None):      # refused before anything loads the library
        ap.error("--batch-bookkeeping records every fit of a batch: it needs --fits-per-launch, --sibling-fits or --ct-volume (a single fit always "
                 "keeps these records; --inpaint-fits has no batched bookkeeping)")
    if a.batch_predict_samples or a.batch_calibration:      # refused before anything loads the library
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
    if a.sibling_fits < 0:
        ap.error("--sibling-fits %d: 0 (off) or the number of fits per launch" % a.sibling_fits)
    if a.sibling_fits:      # refused before anything loads the library, and ahead of the other batching flags' own refusals
        if a.bayes == "mfvi":
            ap.error("--sibling-fits batches the DIP, MC-dropout and SGLD fits (--bayes dip, mcd or sgld); mean-field VI fits batch with --fits-per-launch")
        if a.task not in ("denoising", "super-resolution"):
            ap.error("--sibling-fits serves denoising and super-resolution, not %s" % a.task)
        for flag, on in (("--fits-per-launch", a.fits_per_launch), ("--inpaint-fits", a.inpaint_fits), ("--ct-volume", a.ct_volume is not None),
                         ("--predict-samples", a.predict_samples), ("--calibration", a.calibration)):
            if on:
                ap.error("--sibling-fits does not combine with %s (SiblingBatch.to_engine(f) serves one fit of a batch)" % flag)
        if a.param_dtype != "f32":
            ap.error("--sibling-fits takes float32 parameters (--param-dtype f32)")
    if a.inpaint_fits < 0:
        ap.error("--inpaint-fits %d: 0 (off) or the number of fits per launch" % a.inpaint_fits)
    if a.inpaint_fits:      # refused before anything loads the library, and ahead of the other batching flags' own refusals
        for flag, on in (("--fits-per-launch", a.fits_per_launch), ("--ct-volume", a.ct_volume is not None), ("--predict-samples", a.predict_samples),
                         ("--calibration", a.calibration)):
            if on:
                ap.error("--inpaint-fits does not combine with %s (InpaintBatch.to_engine(f) serves one fit of a batch)" % flag)
        if a.task != "inpainting" or a.bayes != "mfvi":
            ap.error("--inpaint-fits batches mean-field VI inpainting fits (--task inpainting --bayes mfvi), not --task %s --bayes %s" % (a.task, a.bayes))
        if a.param_dtype != "f32":
            ap.error("--inpaint-fits takes float32 parameters (--param-dtype f32)")
    if a.slices_per_launch is not None and (a.ct_volume is None or a.slices_per_launch < 1):
        ap.error("--slices-per-launch %d: at least 1, and only with --ct-volume" % a.slices_per_launch)
    if a.ct_volume is not None:      # refused before anything loads the library
        try:
            parse_ct_volume(a.ct_volume)
        except ValueError as e:
            ap.error(str(e))
        if a.task != "ct" or a.bayes != "mfvi":
            ap.error("--ct-volume fits a CT stack by mean-field VI (--task ct --bayes mfvi), not --task %s --bayes %s" % (a.task, a.bayes))
        if a.param_dtype != "f32":
            ap.error("--ct-volume takes float32 parameters (--param-dtype f32)")
        for flag, on in (("--fits-per-launch", a.fits_per_launch), ("--predict-samples", a.predict_samples), ("--calibration", a.calibration),
                         ("--bo-rounds", a.bo_rounds)):
            if on:
                ap.error("--ct-volume does not combine with %s (CtVolume.to_engine(d) serves one slice of a volume)" % flag)
    if a.fits_per_launch < 0:
        ap.error("--fits-per-launch %d: 0 (off) or the number of fits per launch" % a.fits_per_launch)
    if a.fits_per_launch:      # refused before anything loads the library
        if a.bayes != "mfvi":
            ap.error("--fits-per-launch batches mean-field VI fits (--bayes mfvi), not %s" % a.bayes)
        if a.task not in ("denoising", "super-resolution"):
            ap.error("--fits-per-launch serves denoising and super-resolution, not %s" % a.task)
        if a.param_dtype != "f32":
            ap.error("--fits-per-launch takes float32 parameters (--param-dtype f32)")
        if a.predict_samples:
            ap.error("--fits-per-launch does not combine with --predict-samples (FitBatch.to_engine(f).predict serves one fit of a batch)")
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
    batch_kw = dict(batch_fn=_inpaint_batches, worker="mfvi_dip_mia_amd.runner:inpaint_batch_job") if a.inpaint_fits else {}
    if a.sibling_fits:      # the method rides in the run parameters to the batch function (here, or in a worker of the fan-out)
        batch_kw = dict(batch_fn=_sibling_batches, worker="mfvi_dip_mia_amd.runner:sibling_batch_job")
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
            if a.fits_per_launch or a.inpaint_fits or a.sibling_fits:      # a round's candidates form batches
                res, _, _ = _run_batches(short, jb, a.fits_per_launch or a.inpaint_fits or a.sibling_fits, rp, a.k, devices, **batch_kw)
                return [(tuple(job[k] for k in keys), y) for _, job, y in res]
            if devices:
                from .fanout import run_jobs
                res, _ = run_jobs(jb, devices, "mfvi_dip_mia_amd.runner:fit_job", dict(rp, fn_name=fn_name, K=a.k))
                return [(tuple(job[k] for k in keys), y) for _, job, y in res]
            return [(c, fn(K=a.k, verbose=False, **j, **rp)["psnr"]) for c, j in zip(cand_list, jb)]
        return _bo.bo(bo_params, evaluate, n_rounds=a.bo_rounds)
    if a.fits_per_launch or a.inpaint_fits or a.sibling_fits:
        from .fanout import print_table
        per = a.fits_per_launch or a.inpaint_fits or a.sibling_fits
        results, dropped, batches = _run_batches(short, jobs, per, rp, a.k, devices, verbose=True, **batch_kw)
        print("%d fits in %d batches of up to %d" % (len(jobs), len(batches), per))
        print_table(results, list(BO_KEYS[a.bayes]))
        for i, job, why in dropped:
            print("dropped fit %d %s: %s" % (i, {k: v for k, v in job.items() if k != "img"}, why))
        return results
    if devices:
        # independent fits over the node's GPUs (bayesian_optimization.py:3760-3781, eval_result.py:27-53): no per-step communication,
        # one final gather of (candidate, psnr), NaNs dropped
        from .fanout import run_jobs, print_table
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
