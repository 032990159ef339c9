"""What the reference's runners record every iteration, for every fit of a batch at once.

The single-fit runners keep mse_noisy, mse_gt, three PSNRs and three SSIMs per iteration and, every show_every iterations, the variance and
the mean of two 25-slot ring buffers and the clipped EMA reconstruction (bayesian_optimization.py:1374-1416, :2190-2236, :584-626;
book._Book).  A BatchBook attached to a FitBatch, a SiblingBatch or a CtVolume records the same per fit from a number of launches per
iteration that does not depend on the number of fits:

    mfvi_bookkeep_fits       EMA (in the batch's own ema: it replaces mfvi_ema_fits), clipped copies, ring slots      1 launch (per group: CtVolume)
    mfvi_decimate            sr only: the stacked [F * C * H][W] EMA and the stacked [F * H][W] clipped output         2 launches
    mfvi_pair_metrics        the eight columns of _Book in 4 calls (ct: 2) of 2 launches each

on the batch's side stream, where its EMA runs, with no host sync.  The batch's parameters, moments, EMA, outputs and losses are bit-equal
to an untracked batch's: the EMA comes from the same per-pixel code and nothing else of the iteration is touched."""
import numpy as np

from . import _lib as L
from . import artifacts as A
from .book import MC_ITER
from .rowbatch import EXP_WEIGHT


def owner_geometry(batch):
    """(kind, n_fits, C, H, W, factor) of a batch that can be tracked, from the attributes every RowBatch has: 'den' / 'sr' (FitBatch,
    SiblingBatch; two output channels), 'ct' (CtVolume; one)."""
    if batch.task == "inp":
        raise NotImplementedError("InpaintBatch is not tracked: its 3-channel masked bookkeeping is not batched")
    if batch.task not in ("den", "sr", "ct"):
        raise NotImplementedError("bookkeeping of task %r is not batched" % (batch.task,))
    return batch.task, int(batch.n_rows), int(batch.C), int(batch.H), int(batch.W), int(batch.sr_factor) if batch.task == "sr" else 1


def check_maps(kind, n_fits, H, W, gt, noisy):
    """Shapes, before anything touches the device: gt [H, W] (shared) or [n_fits, H, W]; noisy (den only, required there) likewise.
    -> (gt, noisy) as float32 arrays [n_fits, H, W] (noisy: None unless den)."""
    def one(a, name):
        a = np.asarray(a, np.float32)
        if a.shape == (H, W):
            a = np.broadcast_to(a, (n_fits, H, W))
        if a.shape != (n_fits, H, W):
            raise ValueError("%s of shape %s, expected %s or %s" % (name, a.shape, (H, W), (n_fits, H, W)))
        return np.ascontiguousarray(a)
    g = one(gt, "ground truth")
    if kind == "den":
        if noisy is None:
            raise ValueError("denoising bookkeeping needs the noisy images (noisy=...)")
        return g, one(noisy, "noisy")
    if noisy is not None:
        raise ValueError("noisy=... belongs to denoising; task %r takes its corrupted reference from the ground truth" % (kind,))
    return g, None


def gt_maps(batch, gt, n_fits, H, W):
    """Ground truth for batch.metrics(gt): ([H, W] or [n_fits, H, W] on the device, its pair stride)."""
    g = batch.torch.as_tensor(gt).float().cuda().contiguous()
    if tuple(g.shape) == (H, W):
        return g, 0
    if tuple(g.shape) != (n_fits, H, W):
        raise ValueError("ground truth of shape %s, expected %s" % (tuple(g.shape), (n_fits, H, W)))
    return g, H * W


def recon_metrics(batch, gt):
    """dict(psnr=[F], ssim=[F]) of batch.recon() against the ground truth ([H, W] shared, or [F, H, W]): one mfvi_pair_metrics call."""
    torch, lib, sp = batch.torch, L.lib(), L.stream_ptr()
    _, F, _, H, W, _ = owner_geometry(batch)
    g, gs = gt_maps(batch, gt, F, H, W)
    rec = batch.recon()
    scratch = torch.empty(max(lib.mfvi_pair_metrics_scratch_bytes(F, H, W), 8), dtype=torch.uint8, device="cuda")
    sums = torch.zeros((F, 2), dtype=torch.float64, device="cuda")
    L.check(lib.mfvi_pair_metrics(L.ptr(g), gs, L.ptr(rec), H * W, F, H, W, 1, L.ptr(scratch), L.ptr(sums), 2, sp))
    s = sums.cpu().numpy() / float(H * W)
    with np.errstate(divide="ignore"):
        return dict(psnr=10.0 * np.log10(1.0 / s[:, 0]), ssim=s[:, 1])


class BatchBook:
    def __init__(self, batch, num_iter, gt, noisy=None, mc_iter=MC_ITER):
        self.kind, F, C, H, W, f = owner_geometry(batch)
        if int(num_iter) < 1 or int(mc_iter) < 1:
            raise ValueError("num_iter=%r, mc_iter=%r: at least 1 each" % (num_iter, mc_iter))
        g, nz = check_maps(self.kind, F, H, W, gt, noisy)
        import torch
        self.t, self.batch = torch, batch
        self.F, self.C, self.H, self.W, self.f, self.R, self.num_iter = F, C, H, W, f, int(mc_iter), int(num_iter)
        self.method = getattr(batch, "method", "mfvi")
        dev = "cuda"
        self.gt2 = torch.from_numpy(np.stack([g, g])).to(dev)                     # [2][F][H][W]: the x of the (gt, out_clip) and (gt, avg_clip) pairs
        self.gt = self.gt2[0]
        self.noisy = None if nz is None else torch.from_numpy(nz).to(dev)
        self.clips = torch.zeros((2, F, H, W), device=dev)                       # out_clip, avg_clip: the y of those pairs
        self.out_clip, self.avg_clip = self.clips[0], self.clips[1]
        self.ale_clip = torch.zeros((F, H, W), device=dev) if C > 1 else None
        self.ring_epi = torch.zeros((self.R, F, H, W), device=dev)
        self.ring_ale = torch.zeros((self.R, F, H, W), device=dev) if C > 1 else None
        self.var = torch.zeros((F, H, W), device=dev)
        self.ale_mean = torch.zeros((F, H, W), device=dev) if C > 1 else None
        # raw[i][row][fit] = (squared-error sum, SSIM sum) of the pairs  0 (ema, corrupted)  1 (ema, gt)  2 (corrupted, out_clip)
        # 3 (gt, out_clip)  4 (gt, avg_clip); ct: the corrupted reference IS the ground truth, rows 0 and 2 stay unused
        self.raw = torch.zeros((self.num_iter, 5, F, 2), dtype=torch.float64, device=dev)
        self.scratch = torch.empty(L.lib().mfvi_pair_metrics_scratch_bytes(2 * F, H, W), dtype=torch.uint8, device=dev)
        if self.kind == "sr":      # img_small = img[::f, ::f] and the projections of out_avg / out (:2101, :2203, :2207)
            h, w = H // f, W // f
            self.gt_lr = self.gt[:, ::f, ::f].contiguous()
            self.avg_lr = torch.zeros((F, C, h, w), device=dev); self.out_lr_clip = torch.zeros((F, h, w), device=dev)
        self.i = 0                       # iterations recorded
        self.snaps = []                  # (iteration, var, ale_mean, recon) of every snapshot() so far, for save_npz
        batch._book = self

    # ---- called by the batch on its side stream, behind the forward pass ------------------------------------------------------------
    def group(self, out, f0, nf, S, first):
        """mfvi_bookkeep_fits on the fits f0 .. f0 + nf - 1, whose samples are out[: nf * S]."""
        if self.i >= self.num_iter:
            raise ValueError("the book holds %d iterations and all are recorded" % self.num_iter)
        p, slot = L.ptr, self.i % self.R
        two = self.C > 1
        L.check(L.lib().mfvi_bookkeep_fits(p(out), nf, S, self.C, self.H, self.W, p(self.batch.ema[f0:]), EXP_WEIGHT, int(first), p(self.out_clip[f0:]),
                                           p(self.avg_clip[f0:]), p(self.ale_clip[f0:]) if two else None, p(self.ring_epi[slot, f0:]),
                                           p(self.ring_ale[slot, f0:]) if two else None, L.stream_ptr()))

    def finish(self):
        """The metrics of iteration self.i for every fit, once all groups of the iteration are book-kept."""
        lib, sp, p = L.lib(), L.stream_ptr(), L.ptr
        F, C, H, W = self.F, self.C, self.H, self.W
        hw, raw, ema = H * W, self.raw[self.i], self.batch.ema

        def pairs(x, xs, y, ys, n, h, w, ssim, row):
            L.check(lib.mfvi_pair_metrics(p(x), xs, p(y), ys, n, h, w, ssim, p(self.scratch), p(raw[row]), 2, sp))
        if self.kind == "sr":
            h, w = H // self.f, W // self.f
            L.check(lib.mfvi_decimate(p(ema), F * C * H, W, self.f, p(self.avg_lr), sp))                 # every fit's [C][H][W] in one stacked image
            L.check(lib.mfvi_decimate(p(self.out_clip), F * H, W, self.f, p(self.out_lr_clip), sp))      # clip and [::f, ::f] commute
            pairs(self.avg_lr, C * h * w, self.gt_lr, h * w, F, h, w, 0, 0)          # mse(downsampler(out_avg)[:, :1], img_small)  :2203
            pairs(self.gt_lr, h * w, self.out_lr_clip, h * w, F, h, w, 1, 2)         # psnr_lr, ssim_lr                              :2214-2217
        elif self.kind == "den":
            pairs(ema, C * hw, self.noisy, hw, F, H, W, 0, 0)                        # mse(out_avg[:, :1], noisy)                    :1389
            pairs(self.noisy, hw, self.out_clip, hw, F, H, W, 1, 2)                  # psnr_corrupted, ssim_corrupted                :1398
        pairs(ema, C * hw, self.gt, hw, F, H, W, 0, 1)                               # mse(out_avg[:, :1], gt)                       :1390
        pairs(self.gt2, hw, self.clips, hw, 2 * F, H, W, 1, 3)                       # psnr / ssim of gt vs out_clip, then vs avg_clip
        self.i += 1

    # ---- results -------------------------------------------------------------------------------------------------------------------
    @property
    def metrics(self):
        """[num_iter, F, 8] float64 on the device, the columns of book._Book: mse_noisy, mse_gt, 3 squared-error sums for the PSNRs, 3 SSIM
        sums (sums over the pixels; results() divides).  Gathered from the raw pair sums on the device, no host sync."""
        self.batch._wait_ema()
        r = self.raw
        c = 1 if self.kind == "ct" else 0, 3 if self.kind == "ct" else 2      # ct: both corrupted columns are against the ground truth (:594-606)
        return self.t.stack([r[:, c[0], :, 0], r[:, 1, :, 0], r[:, c[1], :, 0], r[:, 3, :, 0], r[:, 4, :, 0], r[:, c[1], :, 1], r[:, 3, :, 1], r[:, 4, :, 1]], dim=-1)

    def results(self):
        """(mse_noisy [n_it, F], mse_gt [n_it, F], psnrs [n_it, F, 3], ssims [n_it, F, 3]) of the iterations recorded so far, by the host
        arithmetic of book._Book.results."""
        m = self.metrics[:self.i].cpu().numpy()
        n = np.full(8, float(self.H * self.W))
        if self.kind == "sr":
            n[[0, 2, 5]] = float(self.gt_lr[0].numel())
        m = m / n
        with np.errstate(divide="ignore"):
            psnrs = 10.0 * np.log10(1.0 / m[..., 2:5])
        return m[..., 0], m[..., 1], psnrs, m[..., 5:8]

    def snapshot(self):
        """(var [F, H, W], ale_mean [F, H, W] or None for one output channel, recon [F, H, W]): the ring variance (epistemic), the ring mean
        (aleatoric) and the clipped EMA of every fit; mfvi_ring_stats is element-wise, so the [R][F][H][W] rings are one call with H := F * H."""
        self.batch._wait_ema()
        lib, sp, p = L.lib(), L.stream_ptr(), L.ptr
        L.check(lib.mfvi_ring_stats(p(self.ring_epi), self.R, self.F * self.H, self.W, p(self.var), None, sp))
        if self.C > 1:
            L.check(lib.mfvi_ring_stats(p(self.ring_ale), self.R, self.F * self.H, self.W, None, p(self.ale_mean), sp))
        snap = (self.var.cpu().numpy(), self.ale_mean.cpu().numpy() if self.C > 1 else None, self.avg_clip.cpu().numpy())
        self.snaps.append((self.i - 1,) + snap)
        return snap

    def save_npz(self, f, run_dir, head):
        """save.npz of fit f in run_dir (artifacts.save_npz: what a single-fit run of the task writes, with the snapshots taken so far)."""
        if not 0 <= f < self.F:
            raise ValueError("fit %r outside 0..%d" % (f, self.F - 1))
        mn, mg, ps, ss = self.results()
        H, W = self.H, self.W
        pick = lambda k: np.stack([s[k][f] if s[k] is not None else np.zeros((H, W), np.float32) for s in self.snaps]).astype(np.float64)[:, None] \
            if self.snaps else np.zeros((0, 1, H, W))
        A.save_npz(run_dir, self.kind, self.method, head, mn[:, f], mg[:, f], pick(3), pick(1), pick(2), ps[:, f], ss[:, f])
