"""Batched bookkeeping: mfvi_pair_metrics against the oracle's SSIM, float64 numpy and the single-pair entry points,
its reproducibility and isolation properties; mfvi_bookkeep_fits against mfvi_bookkeep / mfvi_ema_fits per fit; BatchBook on FitBatch (den,
sr), CtVolume and SiblingBatch against the oracle's Bookkeeper fed the batch's own outputs, with the tolerances of test_gpu_bookkeeping.py;
a dead fit; batch.metrics; the runner's --batch-bookkeeping.  Nets and sizes: the SMALL net of the batch tests at 32 x 32, input depth 8."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SMALL = dict(nd=(8, 16), nu=(8, 16), ns=(4, 4))
# (13, 9): smaller than the 11-tap window and than the 16 x 64 tile; (37, 50): a tile remainder in both directions; (41, 150): 3 x 3 tiles
# with a remainder in both directions
SHAPES = [(13, 9), (48, 40), (37, 50), (41, 150)]
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def M():
    import mfvi_dip_mia_amd as M_
    assert torch.cuda.is_available()
    M_._lib.lib()
    return M_


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---- 1. mfvi_pair_metrics -------------------------------------------------------------------------------------------------------------------
def smooth(H, W, p=0):
    row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return (0.5 + 0.4 * np.sin((col + 3 * p) / 7.0) * np.cos((row + 2 * p) / 5.0)).astype(np.float32)


def pair_images(H, W, shared):
    """x [1 or 4][H][W] and the four y of the issue, y_p built from x_p."""
    rng = np.random.default_rng(H * 1000 + W)
    xs = np.stack([smooth(H, W, 0 if shared else p) for p in range(4)])
    ys = np.stack([np.clip(xs[0] + rng.normal(scale=0.1, size=(H, W)), 0, 1), np.clip(xs[1] + rng.normal(scale=0.003, size=(H, W)), 0, 1),
                   np.full((H, W), 0.5), np.clip(3 * xs[3] - 1, 0, 1)]).astype(np.float32)
    return (xs[:1] if shared else xs), ys


def pair_call(M, x, xs, y, ys, n, H, W, want_ssim, sums=None, stride=2):
    L = M._lib
    lib = L.lib()
    scratch = torch.empty(max(lib.mfvi_pair_metrics_scratch_bytes(n, H, W), 8), dtype=torch.uint8, device="cuda")
    sums = torch.full((n, stride), SENTINEL, dtype=torch.float64, device="cuda") if sums is None else sums
    L.check(lib.mfvi_pair_metrics(L.ptr(x), xs, L.ptr(y), ys, n, H, W, want_ssim, L.ptr(scratch), L.ptr(sums), stride, L.stream_ptr()))
    return host(sums)


@pytest.fixture(scope="module")
def pair_reference():
    """Per (shape, shared): the images and the references, computed once: the oracle's SSIM mean and the float64 sum of the float32 terms."""
    ref = {}
    for H, W in SHAPES:
        for shared in (True, False):
            xs, ys = pair_images(H, W, shared)
            xp = [xs[0 if shared else p] for p in range(4)]
            ssim = np.array([O.ssim(xp[p], ys[p]) for p in range(4)])
            d = [(xp[p] - ys[p]).astype(np.float32) for p in range(4)]
            sq = np.array([np.sum((d[p] * d[p]).astype(np.float32).astype(np.float64)) for p in range(4)])
            ref[(H, W, shared)] = (xs, ys, ssim, sq)
    return ref


@pytest.mark.parametrize("shared", [True, False], ids=["x_stride0", "distinct_x"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_pair_metrics_against_oracle_numpy_and_single_pair_entries(M, pair_reference, shape, shared):
    H, W = shape
    L = M._lib
    lib, sp = L.lib(), L.stream_ptr()
    xs, ys, ssim_ref, sq_ref = pair_reference[(H, W, shared)]
    x, y = dev(xs), dev(ys)
    xst = 0 if shared else H * W
    s = pair_call(M, x, xst, y, H * W, 4, H, W, 1)
    print("ssim mean - oracle:", s[:, 1] / (H * W) - ssim_ref, " sq rel:", s[:, 0] / sq_ref - 1)
    assert np.abs(s[:, 1] / (H * W) - ssim_ref).max() < 2e-5
    assert np.abs(s[:, 0] - sq_ref).max() <= 1e-9 * sq_ref.max() and np.all(np.abs(s[:, 0] - sq_ref) <= 1e-9 * sq_ref)
    one = torch.zeros(2, dtype=torch.float64, device="cuda")
    for p in range(4):      # the single-pair entry points of the library, same bounds
        xp = x[0 if shared else p]
        L.check(lib.mfvi_sq_err_sum(L.ptr(xp), L.ptr(y[p]), H * W, L.ptr(one), sp))
        L.check(lib.mfvi_ssim_sum(L.ptr(xp), L.ptr(y[p]), H, W, L.ptr(one[1:]), sp))
        o = host(one)
        assert abs(s[p, 0] - o[0]) <= 1e-9 * o[0] and abs(s[p, 1] - o[1]) / (H * W) < 2e-5, p
    # two calls bit-equal; pair p alone bit-equal to pair p of the batch (its sums depend neither on n_pairs nor on the other pairs)
    assert np.array_equal(s, pair_call(M, x, xst, y, H * W, 4, H, W, 1))
    for p in range(4):
        alone = pair_call(M, x[0 if shared else p], xst, y[p], H * W, 1, H, W, 1)
        assert np.array_equal(alone[0], s[p]), p
    # want_ssim = 0: slot 1 untouched, slot 0 the same sum
    s0 = pair_call(M, x, xst, y, H * W, 4, H, W, 0)
    assert np.all(s0[:, 1] == SENTINEL) and np.array_equal(s0[:, 0], s[:, 0])
    # a wider sums_stride lands where it should and writes nothing else
    s3 = pair_call(M, x, xst, y, H * W, 4, H, W, 1, stride=3)
    assert np.array_equal(s3[:, :2], s) and np.all(s3[:, 2] == SENTINEL)
    # a NaN in one y reaches that pair's sums only
    bad = ys.copy(); bad[2, H // 2, W // 3] = np.nan
    sb = pair_call(M, x, xst, dev(bad), H * W, 4, H, W, 1)
    assert np.isnan(sb[2]).all()
    for p in (0, 1, 3):
        assert np.array_equal(sb[p], s[p]), p


def test_pair_metrics_refuses_bad_arguments(M):
    L = M._lib
    lib, sp = L.lib(), L.stream_ptr()
    H, W = 16, 20
    x = torch.zeros((2, H, W), device="cuda"); sums = torch.full((2, 2), SENTINEL, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(lib.mfvi_pair_metrics_scratch_bytes(2, H, W), dtype=torch.uint8, device="cuda")
    assert lib.mfvi_pair_metrics_scratch_bytes(2, H, W) == 2 * 1 * 2 * 8
    assert lib.mfvi_pair_metrics_scratch_bytes(3, 41, 150) == 3 * 9 * 2 * 8
    for n, h, w in ((0, H, W), (65536, H, W), (2, 0, W), (2, H, 0)):
        assert lib.mfvi_pair_metrics_scratch_bytes(n, h, w) == 0
    p = L.ptr
    ok = dict(x=x, xs=H * W, y=x, ys=H * W, n=2, H=H, W=W, scratch=scratch, sums=sums, ss=2)
    for change in (dict(x=None), dict(y=None), dict(scratch=None), dict(sums=None), dict(n=0), dict(n=65536), dict(H=0), dict(W=0), dict(xs=H * W - 1),
                   dict(ys=1), dict(ss=1)):
        a = dict(ok, **change)
        rc = lib.mfvi_pair_metrics(p(a["x"]), a["xs"], p(a["y"]), a["ys"], a["n"], a["H"], a["W"], 1, p(a["scratch"]), p(a["sums"]), a["ss"], sp)
        assert rc < 0 and b"pair_metrics" in lib.mfvi_last_error(), change
    torch.cuda.synchronize()
    assert np.all(host(sums) == SENTINEL)               # nothing was launched
    rc = lib.mfvi_bookkeep_fits(None, 2, 1, 1, H, W, p(x), 0.99, 1, p(x), p(x), None, None, None, sp)
    assert rc < 0 and b"bookkeep_fits" in lib.mfvi_last_error()
    for n, S, Cc in ((0, 1, 1), (65536, 1, 1), (2, 0, 1), (2, 1, 3)):
        assert lib.mfvi_bookkeep_fits(p(x), n, S, Cc, H, W, p(x), 0.99, 1, p(x), p(x), p(x), None, None, sp) < 0
    assert lib.mfvi_bookkeep_fits(p(x), 1, 1, 2, H, W, p(x), 0.99, 1, p(x), p(x), None, None, None, sp) < 0      # C = 2 needs ale_clip


# ---- 2. mfvi_bookkeep_fits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,Cc", [(1, 1), (3, 2)])
def test_bookkeep_fits_is_bookkeep_per_fit(M, S, Cc):
    L = M._lib
    lib, sp, p = L.lib(), L.stream_ptr(), L.ptr
    F, H, W = 3, 16, 20
    z = lambda *s: torch.full(s, SENTINEL, device="cuda")
    ema_b, ema_s, ema_e = z(F, Cc, H, W), z(F, Cc, H, W), z(F, Cc, H, W)
    for it, first in enumerate((1, 0)):
        raw = np.stack([O.bookkeeping_raw("den", 50 + f, it, O.phantom(H, W, 50 + f), Cc, k=k) for f in range(F) for k in range(S)])
        out = dev(raw)
        B = dict(oc=z(F, H, W), av=z(F, H, W), al=z(F, H, W), re=z(F, H, W), ra=z(F, H, W))
        L.check(lib.mfvi_bookkeep_fits(p(out), F, S, Cc, H, W, p(ema_b), 0.99, first, p(B["oc"]), p(B["av"]), p(B["al"]) if Cc > 1 else None, p(B["re"]),
                                       p(B["ra"]) if Cc > 1 else None, sp))
        R = dict(oc=z(F, H, W), av=z(F, H, W), al=z(F, H, W), re=z(F, H, W), ra=z(F, H, W))
        for f in range(F):
            L.check(lib.mfvi_bookkeep(p(out[f * S:]), S, Cc, H, W, p(ema_s[f]), 0.99, first, p(R["oc"][f]), p(R["al"][f]) if Cc > 1 else None, p(R["av"][f]),
                                      p(R["re"][f]), p(R["ra"][f]) if Cc > 1 else None, sp))
        L.check(lib.mfvi_ema_fits(p(out), F, S, Cc, H, W, p(ema_e), 0.99, first, sp))
        for k in B:
            assert torch.equal(B[k], R[k]), (it, k)
            assert bool((B[k] == SENTINEL).all()) == (Cc == 1 and k in ("al", "ra")), (it, k)      # C = 1: the aleatoric buffers are not written
        assert torch.equal(ema_b, ema_s) and torch.equal(ema_b, ema_e), it
    # ring_epi may be NULL
    L.check(lib.mfvi_bookkeep_fits(p(out), F, S, Cc, H, W, p(ema_b), 0.99, 0, p(B["oc"]), p(B["av"]), p(B["al"]) if Cc > 1 else None, None, None, sp))
    torch.cuda.synchronize()


# ---- 3. BatchBook against the oracle's Bookkeeper ------------------------------------------------------------------------------------------
def _hyper(F):
    return [1e-6 * 2 ** f for f in range(F)], [0.05 * 2 ** f for f in range(F)], [1e-3 * (f + 1) for f in range(F)]


def check_book(book, rows, keepers, n_fits):
    """rows [n_it][F][8] of the oracle's Bookkeepers against book.results(), snapshot against snapshot: the bounds of test_gpu_bookkeeping.py
    (rings shorter than 25 iterations included: variance and mean over ALL slots, zeros too)."""
    rows = np.asarray(rows)
    a, b, psnrs, ssims = book.results()
    assert a.shape == b.shape == rows.shape[:2] and psnrs.shape == ssims.shape == rows.shape[:2] + (3,)
    for f in range(n_fits):
        print("fit", f, "mse", relerr(a[:, f], rows[:, f, 0]), relerr(b[:, f], rows[:, f, 1]), "psnr", np.abs(psnrs[:, f] - rows[:, f, 2:5]).max(),
              "ssim", np.abs(ssims[:, f] - rows[:, f, 5:8]).max())
        assert relerr(a[:, f], rows[:, f, 0]) < 2e-5 and relerr(b[:, f], rows[:, f, 1]) < 2e-5, f
        assert np.abs(psnrs[:, f] - rows[:, f, 2:5]).max() < 2e-4 and np.abs(ssims[:, f] - rows[:, f, 5:8]).max() < 2e-5, f
    var, ale, recon = book.snapshot()
    for f in range(n_fits):
        ovar, oale, orecon = keepers[f].snapshot()
        assert relerr(var[f], ovar) < 2e-5 and relerr(recon[f], orecon) < 2e-6, f
        if ale is not None:
            assert relerr(ale[f], oale) < 2e-6, f
    return a, b, psnrs, ssims


def run_tracked(batch, book, keepers, n_it, S, n_fits):
    rows = []
    for _ in range(n_it):
        batch.step()
        out = host(batch.out)                          # this iteration's forward outputs (the next forward overwrites them)
        rows.append([keepers[f].step(out[f * S:(f + 1) * S]) for f in range(n_fits)])
    return rows


def test_fitbatch_den_tracked_against_oracle_and_untracked_twin(M):
    H = W = 32; F, K, seed, n_it = 3, 2, 31, 5
    temps, sigmas, lrs = _hyper(F)
    gt = np.stack([O.phantom(H, W, seed + f) for f in range(F)])
    noisy = np.stack([O.noisy(gt[f], 0.1, seed + f) for f in range(F)]).astype(np.float32)
    make = lambda: M.FitBatch(H, W, F, task="den", K=K, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=SMALL, autotune=False)
    fb = make(); fb.set_targets(torch.from_numpy(noisy))
    book = fb.track(gt, n_it, noisy=noisy)
    assert isinstance(book, M.BatchBook) and fb._book is book
    keepers = [O.Bookkeeper("den", H, W, gt[f], noisy=noisy[f]) for f in range(F)]
    rows = run_tracked(fb, book, keepers, n_it, K, F)
    assert tuple(book.metrics.shape) == (n_it, F, 8) and book.metrics.dtype == torch.float64 and book.metrics.is_cuda
    check_book(book, rows, keepers, F)
    twin = make(); twin.set_targets(torch.from_numpy(noisy))
    for _ in range(n_it):
        twin.step()
    assert twin._book is None
    for name in ("params", "m", "v"):
        assert torch.equal(getattr(fb, name), getattr(twin, name)), name
    fb._wait_ema(); twin._wait_ema()
    assert torch.equal(fb.ema, twin.ema)
    with pytest.raises(ValueError, match="all are recorded"):
        fb.step()                                      # the book holds n_it iterations


def test_fitbatch_sr_low_resolution_columns(M):
    H = W = 32; F, K, seed, n_it, f4 = 2, 1, 33, 4, 4
    temps, sigmas, lrs = _hyper(F)
    gt = np.stack([O.phantom(H, W, seed + f) for f in range(F)])
    fb = M.FitBatch(H, W, F, task="sr", K=K, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, sr_factor=f4, net_kwargs=SMALL, autotune=False)
    fb.set_targets(torch.from_numpy(np.ascontiguousarray(gt[:, ::f4, ::f4])))
    book = fb.track(gt, n_it)
    keepers = [O.Bookkeeper("sr", H, W, gt[f], factor=f4) for f in range(F)]
    rows = run_tracked(fb, book, keepers, n_it, K, F)
    a, b, psnrs, ssims = check_book(book, rows, keepers, F)
    # columns 0, 2 and 5 are sums over the 8 x 8 grid, divided by 64; the rest over 32 x 32
    raw = host(book.metrics)
    assert np.allclose(a, raw[..., 0] / 64.0, rtol=1e-15) and np.allclose(b, raw[..., 1] / 1024.0, rtol=1e-15)
    assert np.allclose(ssims[..., 0], raw[..., 5] / 64.0, rtol=1e-15) and np.allclose(ssims[..., 2], raw[..., 7] / 1024.0, rtol=1e-15)
    assert not np.allclose(psnrs[..., 0], psnrs[..., 1])


def test_ctvolume_groups_tracked_against_oracle(M):
    S, D, K, seed, n_it = 32, 3, 1, 35, 4
    theta = np.arange(0, 180.0, 4.0, dtype=np.float32)
    gt = np.stack([O.phantom(S, S, seed + d) for d in range(D)])
    make = lambda: M.CtVolume(S, D, slices_per_launch=2, K=K, input_depth=8, temp=[1e-4, 2e-4, 4e-4], sigma=[0.05, 0.1, 0.2], lr=1e-3,
                              theta_deg=theta.tolist(), seed=seed, net_kwargs=SMALL, autotune=False)
    vol = make()
    assert [g[1] for g in vol.groups] == [2, 1]        # one group of 2 slices and one of 1
    vol.set_volume(torch.from_numpy(gt))
    book = vol.track(gt, n_it)
    assert book.C == 1 and book.ale_clip is None and book.ring_ale is None
    keepers = [O.Bookkeeper("ct", S, S, gt[d]) for d in range(D)]
    seen, inner = [], vol._ema

    def ema_and_read(d0, nd):      # the groups share vol.out: read each group's outputs where its bookkeeping is enqueued
        inner(d0, nd)
        seen.append((d0, nd, host(vol.out)[:nd * K].copy()))
    vol._ema = ema_and_read
    rows = []
    for _ in range(n_it):
        del seen[:]
        vol.step()
        per = {d0 + j: o[j * K:(j + 1) * K] for d0, nd, o in seen for j in range(nd)}
        rows.append([keepers[d].step(per[d]) for d in range(D)])
    a, b, psnrs, ssims = check_book(book, rows, keepers, D)
    assert np.array_equal(a, b) and np.array_equal(psnrs[..., 0], psnrs[..., 1]) and np.array_equal(ssims[..., 0], ssims[..., 1])      # both 'corrupted' columns: the ground truth
    assert book.snapshot()[1] is None                  # one output channel: no aleatoric map
    twin = make(); twin.set_volume(torch.from_numpy(gt))
    for _ in range(n_it):
        twin.step()
    for name in ("params", "m", "v"):
        assert torch.equal(getattr(vol, name), getattr(twin, name)), name
    vol._wait_ema(); twin._wait_ema()
    assert torch.equal(vol.ema, twin.ema)


def test_siblingbatch_dip_tracked_against_oracle(M):
    H = W = 32; F, K, seed, n_it = 2, 1, 37, 4
    gt = np.stack([O.phantom(H, W, seed + f) for f in range(F)])
    noisy = np.stack([O.noisy(gt[f], 0.1, seed + f) for f in range(F)]).astype(np.float32)
    sb = M.SiblingBatch(H, W, F, "dip", task="den", K=K, input_depth=8, lr=[1e-3, 5e-4], seed=seed, net_kwargs=SMALL, autotune=False)
    sb.set_targets(torch.from_numpy(noisy))
    book = sb.track(gt, n_it, noisy=noisy)
    assert book.method == "dip"
    keepers = [O.Bookkeeper("den", H, W, gt[f], noisy=noisy[f]) for f in range(F)]
    rows = run_tracked(sb, book, keepers, n_it, K, F)
    check_book(book, rows, keepers, F)


def test_dead_fit_stays_in_its_rows(M):
    """A NaN in fit 1's target (tests/test_gpu_fitbatch.py): its rows may be NaN, every other fit's metrics are bit-equal to the clean run's."""
    H = W = 32; F, K, seed, n_it = 3, 2, 12, 3
    temps, sigmas, lrs = _hyper(F)
    gt = np.stack([O.phantom(H, W, seed + f) for f in range(F)])
    tg = np.stack([O.noisy(gt[f], 0.1, seed + f) for f in range(F)]).astype(np.float32)
    bad = tg.copy(); bad[1, 5, 7] = np.nan
    got = []
    for t in (tg, bad):
        fb = M.FitBatch(H, W, F, task="den", K=K, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=SMALL, autotune=False)
        fb.set_targets(torch.from_numpy(t))
        book = fb.track(gt, n_it, noisy=t)
        for _ in range(n_it):
            fb.step()
        got.append((host(book.metrics), fb.dead))
    (clean, dead0), (m, dead1) = got
    assert list(dead0) == [0, 0, 0] and list(dead1) == [0, 1, 0]
    assert np.isfinite(clean).all() and np.isfinite(m[:, [0, 2]]).all()
    for f in (0, 2):
        assert np.array_equal(m[:, f], clean[:, f]), f
    assert np.isnan(m[:, 1, [0, 2, 5]]).all()          # the columns against its NaN target


def test_batch_metrics_is_psnr_and_oracle_ssim(M):
    H = W = 32; F, K, seed = 3, 1, 41
    temps, sigmas, lrs = _hyper(F)
    gt = np.stack([O.phantom(H, W, seed + f) for f in range(F)])
    fb = M.FitBatch(H, W, F, task="den", K=K, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=SMALL, autotune=False)
    fb.set_targets(torch.from_numpy(np.stack([O.noisy(g, 0.1, seed) for g in gt]).astype(np.float32)))
    for _ in range(3):
        fb.step()
    rec = host(fb.recon())
    for g in (gt, gt[1]):                              # per fit, and one shared map (x_stride 0)
        r = fb.metrics(g)
        assert set(r) == {"psnr", "ssim"} and r["psnr"].shape == r["ssim"].shape == (F,)
        assert np.abs(r["psnr"] - fb.psnr(g)).max() < 2e-4
        want = [O.ssim(g[f] if g.ndim == 3 else g, rec[f]) for f in range(F)]
        assert np.abs(r["ssim"] - np.array(want)).max() < 2e-5
    with pytest.raises(ValueError):
        fb.metrics(gt[:2])
    S, D = 32, 2
    vol = M.CtVolume(S, D, K=1, input_depth=8, temp=1e-4, sigma=0.05, lr=1e-3, seed=seed, net_kwargs=SMALL, autotune=False)
    vol.set_volume(torch.from_numpy(gt[:D])); vol.step()
    r = vol.metrics(gt[:D])
    assert np.abs(r["psnr"] - vol.psnr(gt[:D])).max() < 2e-4
    assert np.abs(r["ssim"] - np.array([O.ssim(gt[d], host(vol.recon())[d]) for d in range(D)])).max() < 2e-5
    sb = M.SiblingBatch(H, W, 2, "dip", task="den", K=1, input_depth=8, lr=1e-3, seed=seed, net_kwargs=SMALL, autotune=False)
    sb.set_targets(torch.from_numpy(gt[:2].copy())); sb.step()
    r = sb.metrics(gt[:2])
    assert np.abs(r["psnr"] - sb.psnr(gt[:2])).max() < 2e-4
    assert np.abs(r["ssim"] - np.array([O.ssim(gt[f], host(sb.recon())[f]) for f in range(2)])).max() < 2e-5


# ---- 4. runner ------------------------------------------------------------------------------------------------------------------------------
def test_runner_batch_bookkeeping(M, tmp_path):
    cfg = dict(bo_params=dict(temp=dict(candidates=[1e-6, 2e-6]), sigma=dict(candidates=[0.05])),
               run_params=dict(img="phantom", num_iter=7, lr=1e-3, seed=1, p_sigma=0.1, input_depth=8, show_every=3, plot=False, save=True,
                               net_kwargs=SMALL, save_path=str(tmp_path / "logs")))
    path = str(tmp_path / "cfg.json")
    json.dump(cfg, open(path, "w"))
    res = M.runner.main(["--task", "denoising", "--config", path, "--imsize", "32", "--fits-per-launch", "2", "--batch-bookkeeping"])
    assert [i for i, _, _ in res] == [0, 1]
    (d,) = os.listdir(str(tmp_path / "logs"))
    run_dir = os.path.join(str(tmp_path / "logs"), d)
    assert sorted(os.listdir(run_dir)) == ["batch.npz", "bookkeeping_batch.npz", "fit_000", "fit_001"]
    z = np.load(os.path.join(run_dir, "batch.npz"))
    assert set(z.files) == {"task", "temp", "sigma", "lr", "prior_sigma", "K", "seed", "num_iter", "iterations", "psnr_gt_sm", "nll", "kl", "recon", "dead"}
    b = np.load(os.path.join(run_dir, "bookkeeping_batch.npz"))
    assert set(b.files) == {"iterations", "mse_noisy", "mse_gt", "psnrs", "ssims", "recons", "uncerts", "uncerts_ale"}
    n_it = 8                                            # num_iter + 1 iterations, snapshots at 0, 3, 6
    assert b["mse_noisy"].shape == b["mse_gt"].shape == (n_it, 2) and b["psnrs"].shape == b["ssims"].shape == (n_it, 2, 3)
    assert list(b["iterations"]) == [0, 3, 6]
    assert b["recons"].shape == b["uncerts"].shape == b["uncerts_ale"].shape == (3, 2, 32, 32)
    assert all(np.isfinite(b[k]).all() for k in b.files)
    for f, (_, _, y) in enumerate(res):
        assert abs(b["psnrs"][-1, f, 2] - y) < 2e-4     # the run's returned psnr_gt_sm
        assert os.listdir(os.path.join(run_dir, "fit_%03d" % f)) == ["save.npz"]
        s = np.load(os.path.join(run_dir, "fit_%03d" % f, "save.npz"), allow_pickle=True)
        assert set(s.files) == {"img_gt", "img_noisy", "mse_noisy", "mse_gt", "recons", "uncerts", "uncerts_ale", "psnrs", "ssims"}      # a den save.npz
        for key, shape in [("mse_noisy", (n_it,)), ("mse_gt", (n_it,)), ("psnrs", (n_it, 3)), ("ssims", (n_it, 3)), ("recons", (3, 1, 32, 32)),
                           ("uncerts", (3, 1, 32, 32)), ("uncerts_ale", (3, 1, 32, 32))]:
            assert s[key].flat[0]["mfvi"].shape == shape, key      # as the notebooks read it (.flat[0]['mfvi'])
        assert s["img_gt"].shape == s["img_noisy"].shape == (1, 32, 32)
        assert np.array_equal(s["psnrs"].flat[0]["mfvi"], b["psnrs"][:, f]) and np.array_equal(s["recons"].flat[0]["mfvi"][:, 0], b["recons"][:, f])


def test_runner_batch_bookkeeping_ct_volume_and_siblings(M, tmp_path):
    """The flag's other two owners, through the batch runners: the same files, a CT save.npz per slice (no aleatoric maps) and a DIP one."""
    r = M.runner.run_ct_volume("phantom:3", temp=1e-4, sigma=0.05, slices_per_launch=2, imsize=(32, 32), num_iter=4, lr=1e-3, input_depth=8, seed=2,
                               show_every=2, save_path=str(tmp_path / "ct"), net_kwargs=SMALL, autotune=False, batch_bookkeeping=True)
    assert sorted(os.listdir(r["run_dir"])) == ["bookkeeping_batch.npz", "fit_000", "fit_001", "fit_002", "volume.npz"]
    b = np.load(os.path.join(r["run_dir"], "bookkeeping_batch.npz"))
    assert set(b.files) == {"iterations", "mse_noisy", "mse_gt", "psnrs", "ssims", "recons", "uncerts"}      # one output channel
    assert b["psnrs"].shape == (5, 3, 3) and b["recons"].shape == b["uncerts"].shape == (3, 3, 32, 32) and list(b["iterations"]) == [0, 2, 4]
    assert np.abs(b["psnrs"][-1, :, 2] - np.array(r["psnr"])).max() < 2e-4
    s = np.load(os.path.join(r["run_dir"], "fit_002", "save.npz"), allow_pickle=True)
    assert set(s.files) == {"img_gt", "img_radon", "mse_noisy", "mse_gt", "recons", "uncerts", "uncerts_ale", "psnrs", "ssims"}
    assert s["img_gt"].shape == (1, 1, 32, 32) and s["img_radon"].shape == (1, 1, 45, 32) and s["psnrs"].flat[0]["mfvi"].shape == (5, 3)
    jobs = [dict(img="phantom"), dict(img="phantom", lr=5e-4)]
    r = M.runner.run_sibling_batch("sr", "dip", jobs, imsize=(32, 32), num_iter=3, lr=1e-3, input_depth=8, seed=2, show_every=2, save_path=str(tmp_path / "sib"),
                                   net_kwargs=SMALL, autotune=False, batch_bookkeeping=True)
    assert sorted(os.listdir(r["run_dir"])) == ["batch.npz", "bookkeeping_batch.npz", "fit_000", "fit_001"]
    b = np.load(os.path.join(r["run_dir"], "bookkeeping_batch.npz"))
    assert b["psnrs"].shape == (4, 2, 3) and list(b["iterations"]) == [0, 2] and np.abs(b["psnrs"][-1, :, 2] - np.array(r["psnr"])).max() < 2e-4
    s = np.load(os.path.join(r["run_dir"], "fit_001", "save.npz"), allow_pickle=True)
    assert set(s.files) == {"img_hr", "img_lr", "mse_noisy", "mse_gt", "recons", "uncerts", "uncerts_ale", "psnrs", "ssims"}
    assert s["img_lr"].shape == (8, 8) and s["uncerts"].flat[0] == {} and s["recons"].flat[0]["dip"].shape == (2, 1, 32, 32)      # DIP: no uncertainty maps
