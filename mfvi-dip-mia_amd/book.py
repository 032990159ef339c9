"""Device-side bookkeeping of one single-fit run: what the reference's loops record per iteration (EMA, clip, ring buffers, 2 MSE + 3 PSNR +
3 SSIM; bayesian_optimization.py:1374-1416, :2190-2236, :584-626, :3039-3090) in HIP kernels that write into device arrays, beside the backward
pass on a second stream.  `_Book` serves den / sr / ct, `_BookInp` inpainting; the runner (runner._fit) drives either through hook / snapshot /
results.  batchbook.BatchBook records the same for every fit of a batch."""
import numpy as np

from . import _lib as L
from .rowbatch import EXP_WEIGHT

MC_ITER = 25            # ring-buffer length (bayesian_optimization.py:1314)


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
