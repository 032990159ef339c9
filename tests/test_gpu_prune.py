"""SNR pruning on the GPU: the keys against their float64 statement, the radix select against numpy's lexsort on the
device keys (exact masks, thresholds and tie counts), the pruned copy, engines and batches under prune=, the histogram against
numpy.searchsorted, the drop-in against the reference's own masks, the runner's pruning.npz."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SMALL = dict(nd=(8, 16), nu=(8, 16), ns=(4, 4))
INP_KW = dict(nd=(8, 16, 16), nu=(8, 16, 16), ns=(0, 0, 0))
MAPS = ("mean", "epi", "ale", "total", "err2", "mse_mc")
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def M():
    import mfvi_dip_mia_amd as M_
    assert torch.cuda.is_available()
    M_._lib.lib()
    return M_


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def bits_of(keys):
    return np.ascontiguousarray(keys, np.float32).view(np.uint32) & np.uint32(0x7fffffff)


# ---- segment tables ----------------------------------------------------------------------------------------------------------------------------
def layout(n_w, n_b):
    """Interleaved multi-layer table [(offset, count, group)] over n_w + n_b elements: weights split into up to 3 layers, the middle layer
    without a bias, the others sharing the biases."""
    w = [n_w - 2 * (n_w // 3), n_w // 3, n_w // 3] if n_w >= 3 else [n_w]
    b = ([n_b - n_b // 2, 0, n_b // 2] if n_b >= 2 else [n_b, 0, 0])[:len(w)]
    segs, off = [], 0
    for cw, cb in zip(w, b):
        segs.append((off, cw, 0)); off += cw
        if cb:
            segs.append((off, cb, 1)); off += cb
    assert off == n_w + n_b
    return segs


def group_index(segs, g):
    idx = [np.arange(o, o + c, dtype=np.int64) for o, c, gg in segs if gg == g]
    return np.concatenate(idx) if idx else np.zeros(0, np.int64)


def expected_select(keys_row, segs, ks):
    """(mask, threshold bits [2], ties [2]) of one row from np.lexsort((index, key bits)) per group."""
    bits = bits_of(keys_row)
    mask = np.ones(keys_row.size, np.uint8)
    thr, ties = np.zeros(2, np.uint32), np.zeros(2, np.int64)
    for g in (0, 1):
        idx = group_index(segs, g)
        k = min(max(int(ks[g]), 0), idx.size)
        if k == 0:
            continue
        order = np.lexsort((idx, bits[idx]))
        pruned = idx[order[:k]]
        mask[pruned] = 0
        thr[g] = bits[pruned[-1]]
        ties[g] = int((bits[pruned] == thr[g]).sum())
    return mask, thr, ties


def seg_tensor(M, segs):
    from mfvi_dip_mia_amd.prune import pack_segments
    return torch.frombuffer(bytearray(pack_segments(segs) or b"\0" * 24), dtype=torch.uint8).cuda()


def run_select(M, keys, segs, ks, pad=64):
    """mfvi_snr_select on keys [rows, n] with k [rows, 2] -> (mask, thr bits, ties), the words around every output checked for overruns."""
    L, lib = M._lib, M._lib.lib()
    rows, n = keys.shape
    d_keys, d_segs = dev(keys), seg_tensor(M, segs)
    d_k = dev(np.asarray(ks, np.int64).reshape(rows, 2))
    mask = torch.full((rows * n + pad,), 77, dtype=torch.uint8, device="cuda")
    thr = torch.full((rows * 2 + 2,), -7, dtype=torch.int32, device="cuda")
    ties = torch.full((rows * 2 + 2,), -7, dtype=torch.int64, device="cuda")
    nb = lib.mfvi_snr_select_scratch_bytes(rows)
    assert nb > 0 and nb % 8 == 0
    scratch = torch.full((nb // 8 + 8,), -1, dtype=torch.int64, device="cuda")
    L.check(lib.mfvi_snr_select(L.ptr(d_keys), rows, n, L.ptr(d_segs), len(segs), L.ptr(d_k), L.ptr(mask), L.ptr(thr), L.ptr(ties), L.ptr(scratch),
                                L.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((mask[rows * n:] == 77).all()) and bool((thr[rows * 2:] == -7).all()) and bool((ties[rows * 2:] == -7).all())
    assert bool((scratch[nb // 8:] == -1).all()), "mfvi_snr_select wrote past its scratch"
    assert np.array_equal(host(d_keys).view(np.uint32), keys.view(np.uint32))                # the keys are only read
    return host(mask[:rows * n]).reshape(rows, n), host(thr[:rows * 2]).view(np.uint32).reshape(rows, 2), host(ties[:rows * 2]).reshape(rows, 2)


def check_select(M, keys, segs, ks, what):
    got = run_select(M, keys, segs, ks)
    for r in range(keys.shape[0]):
        mask, thr, ties = expected_select(keys[r], segs, ks[r])
        assert np.array_equal(got[0][r], mask), (what, r, ks[r], int((got[0][r] != mask).sum()))
        assert np.array_equal(got[1][r], thr) and np.array_equal(got[2][r], ties), (what, r, ks[r], got[1][r], thr, got[2][r], ties)
    again = run_select(M, keys, segs, ks)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), what
    return got


# ---- 1. keys -----------------------------------------------------------------------------------------------------------------------------------
def test_keys_against_float64_statement(M):
    L, lib = M._lib, M._lib.lib()
    n, rows = 1027 + 37, 3
    stride = 2 * n + 13                                                        # a padded stride, rows not 16-byte aligned
    rng = np.random.default_rng(3)
    buf = np.full((rows, stride), np.nan, np.float32)                          # the padding must not be read into a key
    mu = rng.normal(0.0, 0.1, size=(rows, n)).astype(np.float32)
    rho = rng.normal(-3.0, 1.0, size=(rows, n)).astype(np.float32)
    sp_rho = np.array([-200.0, -30.0, 0.0, 19.9, 20.1, 50.0], np.float32)
    sp_mu = np.array([0.0, -0.0, np.nan, 0.25], np.float32)
    j = 5
    for r_ in sp_rho:                                                          # every special rho with every special mu, in row 1
        for m_ in sp_mu:
            mu[1, j], rho[1, j] = m_, r_
            j += 7
    buf[:, :n], buf[:, n:2 * n] = mu, rho
    keys = torch.full((rows * n + 32,), SENTINEL, dtype=torch.float32, device="cuda")
    L.check(lib.mfvi_snr_keys(L.ptr(dev(buf)), rows, stride, n, L.ptr(keys), L.stream_ptr()))
    assert bool((keys[rows * n:] == SENTINEL).all())
    got = host(keys[:rows * n]).reshape(rows, n)
    r64 = rho.astype(np.float64)
    with np.errstate(all="ignore"):
        sig = np.where(r64 > 20.0, r64, np.log1p(np.exp(r64)))
        want = np.abs(mu.astype(np.float64)) / sig
        sig32 = sig.astype(np.float32)                                         # softplus(-200) underflows to +0 in float32: x / 0 as IEEE gives it
        want = np.where(sig32 == 0, np.abs(mu).astype(np.float32) / sig32, want)
    finite = np.isfinite(want) & (want < 3e38)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), ~finite & ~np.isnan(want))
    assert int(np.isnan(got).sum()) >= len(sp_rho) + 2 and int(np.isinf(got).sum()) >= 1      # NaN mu at every rho, 0 / 0 and 0.25 / 0 at rho = -200
    nz = finite & (want > 0)
    err = float((np.abs(got[nz] - want[nz]) / want[nz]).max())
    print("snr keys: largest relative error against the float64 statement %.3e over %d keys" % (err, nz.sum()))
    # expf <= 1 ulp, log1pf <= 2 ulp, the division <= 0.5 ulp: under 4 ulp = 4.2e-7
    assert err < 1e-6
    assert (got[finite & (want == 0)].view(np.uint32) == 0).all()              # |-0.0| / sigma is +0


# ---- 2. selection ------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = {"1027+37": (1027, 37), "3+300": (3, 300), "grid-cap": (2048 * 256 + 259, 0)}


def ks_for(n_w, n_b, prune):
    """Three rows of k per layout: every amount of the list (0, a share with k = 0, k = 1, 0.5, k = n - 1, 1.0), a different one per row and group."""
    out = []
    for n in (n_w, n_b):
        out.append([0, prune.k_of(0.5 / max(n, 1), n), min(1, n), prune.k_of(0.5, n), max(n - 1, 0), prune.k_of(1.0, n)])
    kw, kb = out
    assert kw[1] == 0 and kb[1] == 0
    return [[[kw[0], kb[3]], [kw[2], kb[5]], [kw[3], kb[4]]], [[kw[1], kb[2]], [kw[4], kb[0]], [kw[5], kb[1]]]]


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_select_exact(M, name):
    from mfvi_dip_mia_amd import prune
    n_w, n_b = LAYOUTS[name]
    segs, n = layout(n_w, n_b), n_w + n_b
    assert any(a[2] == 0 and b[2] == 0 for a, b in zip(segs, segs[1:]))        # a layer without a bias: two weight segments in a row
    rng = np.random.default_rng(n)
    keys = (np.abs(rng.normal(0.0, 0.1, size=(3, n))) / np.log1p(np.exp(rng.normal(-3.0, 1.0, size=(3, n))))).astype(np.float32)
    for i, ks in enumerate(ks_for(n_w, n_b, prune)):
        got = check_select(M, keys, segs, ks, "%s set %d" % (name, i))
        for r in range(3):
            assert int((got[0][r] == 0).sum()) == min(ks[r][0], n_w) + min(ks[r][1], n_b)
    if n_b == 0:
        check_select(M, keys, segs, [[n_w // 3, 5], [0, 1], [n_w, n_b + 9]], name + " k beyond an empty group")


def test_select_ties_inf_nan(M):
    n_w, n_b = 1027, 37
    segs, n = layout(n_w, n_b), n_w + n_b
    rng = np.random.default_rng(11)
    sig = np.float32(np.log1p(np.exp(-3.0)))
    q = np.abs(rng.choice(np.array([0.0, 0.05, -0.05, 0.1, -0.1], np.float32), size=(3, n))) / sig      # three tie classes per group
    q[1] = np.float32(0.05) / sig                                              # row 1: all keys equal
    q[2, rng.choice(n, 40, replace=False)] = np.inf                            # row 2: inf and NaN keys, of both signs of NaN
    nan_at = rng.choice(n, 40, replace=False)
    q[2, nan_at[:20]] = np.nan
    q[2, nan_at[20:]] = np.array([0xffc00000], np.uint32).view(np.float32)[0]
    assert q.dtype == np.float32 and int((q[2].view(np.uint32) == 0xffc00000).sum()) == 20
    wi, bi = group_index(segs, 0), group_index(segs, 1)
    n0 = int((q[0, wi] == 0).sum())
    assert 10 < n0 < n_w - 10
    finite2 = int(np.isfinite(q[2, wi]).sum())
    cases = [[[n0 // 2, 5], [n_w // 2, n_b // 2], [finite2 + 3, n_b - 1]],       # inside the lowest class; all equal; into the inf class
             [[n0 + 7, n_b], [1, 1], [n_w - 3, 2]],                            # inside the second class; k = 1 of equals; into the NaN class
             [[n_w, 0], [n_w - 1, n_b - 1], [n_w, n_b]]]
    for i, ks in enumerate(cases):
        got = check_select(M, q, segs, ks, "ties set %d" % i)
        if i == 0:      # the prefix in index order of the tie class is what is pruned
            zero_w = wi[q[0, wi] == 0]
            assert (got[0][0][zero_w[:n0 // 2]] == 0).all() and (got[0][0][zero_w[n0 // 2:]] == 1).all()
            assert (got[0][1][wi[:n_w // 2]] == 0).all() and (got[0][1][wi[n_w // 2:]] == 1).all() and got[2][1][0] == n_w // 2
    bits2 = bits_of(q[2])
    got = run_select(M, q, segs, cases[1])
    kept = wi[got[0][2][wi] == 1]
    assert kept.size == 3 and (bits2[kept] > 0x7f800000).all() and np.array_equal(kept, wi[bits2[wi] > 0x7f800000][-3:])      # NaN keys are pruned last


def test_select_untouched_outside_segments(M):
    """Elements that belong to no segment (or to a segment of another group number) are kept whatever k says."""
    n = 700
    segs = [(10, 200, 0), (300, 50, 1), (400, 100, 7), (600, 90, 0)]
    keys = np.abs(np.random.default_rng(2).normal(size=(2, n))).astype(np.float32)
    got = check_select(M, keys, segs, [[290, 50], [100, 7]], "gaps")
    outside = np.ones(n, bool)
    outside[10:210] = outside[300:350] = outside[600:690] = False
    assert (got[0][:, outside] == 1).all() and (got[0][0][~outside] == 0).all()


# ---- 3. apply ----------------------------------------------------------------------------------------------------------------------------------
def test_apply_copies_rows_and_prunes(M):
    L, lib = M._lib, M._lib.lib()
    rows, n, n_bn = 3, 1027 + 37, 53
    row_floats = 2 * n + n_bn
    stride = row_floats + 7
    rng = np.random.default_rng(8)
    src = rng.normal(size=(rows, stride)).astype(np.float32)
    mask = (rng.uniform(size=(rows, n)) > 0.4).astype(np.uint8)
    d_src = dev(src)
    dst = torch.full((rows, stride), SENTINEL, dtype=torch.float32, device="cuda")
    L.check(lib.mfvi_prune_apply(L.ptr(d_src), L.ptr(dst), L.ptr(dev(mask)), rows, stride, n, row_floats, L.stream_ptr()))
    want = src.copy()
    want[:, row_floats:] = SENTINEL                                            # the words between the rows are not written
    want[:, :n][mask == 0] = 0.0
    want[:, n:2 * n][mask == 0] = L.PRUNED_RHO
    assert L.PRUNED_RHO == -200.0 and host(dst).tobytes() == want.tobytes()   # bit-equal: +0 where pruned, the BN tail copied
    assert host(d_src).tobytes() == src.tobytes()
    # at the pruned rho every softplus of the library is exactly +0: the KL-free forward of a fully pruned engine has zero spread (test below)


# ---- 4. engine ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def den_engine(M):
    from oracle import oracle as O
    H = W = 32
    eng = M.engine.ElboEngine(H, W, K=2, input_depth=8, net_kwargs=SMALL, autotune=False, seed=5)
    gt = O.phantom(H, W, 5).astype(np.float32)
    eng.set_target(torch.from_numpy(O.noisy(gt, 0.1, 5).astype(np.float32)))
    for _ in range(3):
        eng.step()
    torch.cuda.synchronize()
    return eng, torch.from_numpy(gt)


def numpy_pruned(M, eng, amount):
    """(mu, rho, mask, k) pruned on the host from the device keys, per group by lexsort."""
    from mfvi_dip_mia_amd import prune
    keys = host(eng.snr()).copy()
    segs = prune.segment_table(eng.prog)
    ks = [prune.k_of(amount, n) for n in prune.group_sizes(segs)]
    mask, _, _ = expected_select(keys, segs, ks)
    mu, rho = host(eng.mu).copy(), host(eng.rho).copy()
    mu[mask == 0] = 0.0
    rho[mask == 0] = M._lib.PRUNED_RHO
    return mu, rho, mask, ks


def test_engine_predict_pruned(M, den_engine):
    eng, gt = den_engine
    state = lambda: [host(x).copy() for x in (eng.params, eng.m, eng.v, eng.out)]
    before, t = state(), eng.t
    base = eng.predict(4, target=gt)
    zero = eng.predict(4, target=gt, prune=0)
    assert "prune" not in base and "prune" not in zero and all(torch.equal(base[k], zero[k]) for k in MAPS)
    r = eng.predict(4, target=gt, prune=0.5)
    mu, rho, mask, ks = numpy_pruned(M, eng, 0.5)
    other = M.engine.ElboEngine(32, 32, K=2, input_depth=8, net_kwargs=SMALL, autotune=False, seed=5)
    other.params.copy_(eng.params); other.z0.copy_(eng.z0)
    other.mu.copy_(dev(mu)); other.rho.copy_(dev(rho))
    want = other.predict(4, target=gt)
    for k in MAPS:
        assert torch.equal(r[k], want[k]), k
    assert not torch.equal(r["mean"], base["mean"])
    p = r["prune"]
    assert "mask" not in p and list(p["k"]) == ks and list(p["n"]) == [int(mask.size - sum(l["cout"] for l in eng.prog.layers)), sum(l["cout"] for l in eng.prog.layers)]
    assert int(p["layer_pruned"].sum()) == sum(ks) and p["layer_sparsity"].shape == (len(eng.prog.layers),)
    info = eng.prune_mask(0.5)
    assert np.array_equal(host(info["mask"]), mask) and np.array_equal(info["layer_pruned"], p["layer_pruned"])
    assert abs(float((p["layer_sparsity"] * [l["cout"] * l["cin"] * l["k"] ** 2 + l["cout"] for l in eng.prog.layers]).sum()) - sum(ks)) < 1e-6
    assert np.isfinite(p["threshold"]).all() and p["threshold"].tobytes() == info["threshold"].tobytes()
    full =eng.predict(4, target=gt, prune=1.0)
    assert bool((full["epi"] == 0).all()), "a fully pruned posterior has no spread: pruned weights are exactly zero with zero variance"
    after = state()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)) and eng.t == t


def test_engine_threshold_is_largest_pruned_key(M, den_engine):
    from mfvi_dip_mia_amd import prune
    eng, _ = den_engine
    info = eng.prune_mask(0.3)
    keys, mask = host(eng.snr()), host(info["mask"])
    segs = prune.segment_table(eng.prog)
    for g in (0, 1):
        idx = group_index(segs, g)
        pruned = idx[mask[idx] == 0]
        assert pruned.size == info["k"][g] == prune.k_of(0.3, idx.size)
        assert float(info["threshold"][g]) == float(keys[pruned].max()) <= float(keys[idx[mask[idx] == 1]].min())


# ---- 5. batches --------------------------------------------------------------------------------------------------------------------------------
def pruned_draws_max(eng, amount, N, chunk):
    """max |y| over the raw outputs eng.predict(N, chunk=chunk, prune=amount) reduces."""
    from mfvi_dip_mia_amd.predictive import DEFAULT_STEP
    plan, out = eng._pred_plan(chunk)
    mu, rho, bn = (eng.mu, eng.rho, eng.bn) if not amount else eng._pruned_params(amount)[0]
    m = 0.0
    for c0 in range(0, N, chunk):
        n = min(chunk, N - c0)
        plan.forward(mu, rho, bn, eng.z0, eng.seed, DEFAULT_STEP, c0, n, eng.sample_weights, out)
        m = max(m, float(out[:n].abs().max()))
    return m


def check_rows_against_engines(batch, r, amounts, N, chunk, targets, what):
    """Row f of r against batch.to_engine(f).predict(N, prune=amounts[f]) under the bounds of tests/test_gpu_batchpredict.py (map_bounds: the
    same arithmetic in another order moves a raw output by at most 1e-5 max|y|)."""
    import test_gpu_batchpredict as BP
    for f, a in enumerate(amounts):
        eng = batch.to_engine(f, autotune=False)
        s = eng.predict(N, target=targets[f], chunk=chunk, prune=a)
        if a:
            assert list(s["prune"]["k"]) == list(r["prune"][f]["k"]) and np.array_equal(s["prune"]["layer_pruned"], r["prune"][f]["layer_pruned"])
            assert s["prune"]["threshold"].tobytes() == r["prune"][f]["threshold"].tobytes()
            assert torch.equal(eng.prune_mask(a)["mask"], batch.prune_mask(amounts)[f]["mask"])
        s = {k: (host(v) if torch.is_tensor(v) else v) for k, v in s.items()}
        bounds = BP.map_bounds(s, 1e-5 * pruned_draws_max(eng, a, N, chunk))
        for k in MAPS:
            if s[k] is None:
                assert r[k] is None
                continue
            d = np.abs(host(r[k][f]).reshape(s[k].shape).astype(np.float64) - s[k])
            b = np.broadcast_to(bounds[k], d.shape)
            worst = float(np.where(d == 0, 0.0, d / np.where(b > 0, b, 1e-300)).max())      # (a heavily pruned row can be all zeros: bound 0, difference 0)
            print("%s row %d prune %.2f %-6s max |diff| %.2e, largest diff / bound %.3f" % (what, f, a, k, d.max(), worst))
            assert (d <= b).all(), (what, f, k, worst)


def test_fitbatch_predict_pruned_rows(M):
    from oracle import oracle as O
    import test_gpu_batchpredict as BP
    H = W = 32; F, seed, N = 3, 6, 4
    temps, sigmas, lrs = BP._hyper(F)
    fb = M.FitBatch(H, W, F, task="den", K=1, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=SMALL, autotune=False)
    BP.write_bn(fb, seed)
    gt = np.stack([O.phantom(H, W, seed + f) for f in range(F)]).astype(np.float32)
    fb.set_targets(torch.from_numpy(np.stack([O.noisy(g, 0.1, seed + f) for f, g in enumerate(gt)]).astype(np.float32)))
    fb.step(); fb.step()
    fb.recon()
    pbuf = host(fb._pbuf).copy()
    amounts = [0.0, 0.5, 0.9]
    base = fb.predict(N, target=torch.from_numpy(gt), chunk=2)
    r = fb.predict(N, target=torch.from_numpy(gt), chunk=2, prune=amounts)
    assert host(fb._pbuf).tobytes() == pbuf.tobytes()
    assert all(torch.equal(r[k][0], base[k][0]) for k in MAPS) and not torch.equal(r["mean"][1], base["mean"][1])      # amount 0: the row's own bits
    assert [list(p["k"]) for p in r["prune"]] == [[0, 0]] + [[int(a * n) for n in r["prune"][0]["n"]] for a in amounts[1:]]
    check_rows_against_engines(fb, r, amounts, N, 2, torch.from_numpy(gt), "den")
    same = fb.predict(N, target=torch.from_numpy(gt), chunk=2, prune=0)
    assert "prune" not in same and all(torch.equal(same[k], base[k]) for k in MAPS)
    snr = host(fb.snr())
    assert snr.shape == (F, fb.n_vi) and np.array_equal(snr[2], host(fb.to_engine(2, autotune=False).snr()))


def test_inpaintbatch_predict_pruned_rows(M):
    from oracle import oracle as O
    import test_gpu_batchpredict as BP
    H = W = 32; F, seed, N = 2, 10, 4
    temps, sigmas, lrs = BP._hyper(F)
    ib = M.InpaintBatch(H, W, F, K=1, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=INP_KW, autotune=False)
    BP.write_bn(ib, seed)
    img = np.stack([np.stack([O.phantom(H, W, seed + 3 * f + c) for c in range(3)]) for f in range(F)]).astype(np.float32)
    mask = (np.random.default_rng(seed).uniform(size=(F, 1, H, W)) > 0.3).astype(np.float32)
    ib.set_targets(torch.from_numpy(img), torch.from_numpy(mask))
    ib.step(); ib.step()
    ib.recon()
    pbuf = host(ib._pbuf).copy()
    amounts = [0.5, 0.9]
    r = ib.predict(N, target=torch.from_numpy(img), chunk=2, prune=amounts)
    assert host(ib._pbuf).tobytes() == pbuf.tobytes()
    check_rows_against_engines(ib, r, amounts, N, 2, torch.from_numpy(img), "inp")


def test_sibling_batch_and_engine_refuse(M):
    kw = dict(task="den", K=1, input_depth=8, lr=1e-3, weight_decay=0.0, seed=1, net_kwargs=SMALL, autotune=False)
    sb = M.SiblingBatch(32, 32, 2, "mcd", dropout_p=0.3, **kw)
    for call in (lambda: sb.predict(4, prune=0.5), lambda: sb.snr(), lambda: sb.prune_mask(0.5)):
        with pytest.raises(TypeError, match="no rho"):
            call()
    se = M.engine.SiblingEngine(32, 32, method="mcd", input_depth=8, net_kwargs=SMALL, autotune=False)
    with pytest.raises(TypeError, match="no rho"):
        se.predict(4, prune=0.5)


# ---- 6. histogram ------------------------------------------------------------------------------------------------------------------------------
def test_histogram_exact(M, den_engine):
    from mfvi_dip_mia_amd import prune
    eng, _ = den_engine
    L, lib = M._lib, M._lib.lib()
    segs = layout(1027, 37)
    n, rows, n_bins = 1027 + 37, 3, 17
    rng = np.random.default_rng(4)
    keys = (10.0 ** rng.uniform(-5.0, 5.0, size=(rows, n))).astype(np.float32)
    edges, bounds = prune.hist_bounds(n_bins, (-3.0, 2.5))
    keys[0, :n_bins + 1] = bounds                                              # keys ON the boundaries
    keys[1, 3], keys[1, 4], keys[1, 5], keys[1, 1030] = np.nan, np.inf, 0.0, np.nan
    counts = torch.full((rows * 2 * (n_bins + 2) + 4,), -3, dtype=torch.int64, device="cuda")
    L.check(lib.mfvi_snr_histogram(L.ptr(dev(keys)), rows, n, L.ptr(seg_tensor(M, segs)), len(segs), L.ptr(dev(bounds)), n_bins, L.ptr(counts), L.stream_ptr()))
    assert bool((counts[-4:] == -3).all())
    got = host(counts[:-4]).reshape(rows, 2, n_bins + 2)
    for r in range(rows):
        for g in (0, 1):
            idx = group_index(segs, g)
            slot = np.searchsorted(bounds, keys[r, idx], side="right")          # NaN sorts above everything: the overflow slot
            assert np.array_equal(got[r, g], np.bincount(slot, minlength=n_bins + 2)), (r, g)
            assert got[r, g].sum() == idx.size
    # the engine's own histogram over its device keys
    sel = eng._snr_select()
    sel.compute_keys(eng.params)
    c, e = prune.snr_histogram(sel)
    k = host(sel.keys)[0]
    _, b = prune.hist_bounds()
    for g in (0, 1):
        idx = group_index(sel.segs, g)
        assert np.array_equal(c[0, g], np.bincount(np.searchsorted(b, k[idx], side="right"), minlength=b.size + 1))
    assert c.shape == (1, 2, prune.HIST_BINS + 2) and e.shape == (prune.HIST_BINS + 1,)


# ---- 7. the drop-in against the reference ------------------------------------------------------------------------------------------------------
def golden_net(M, g, flat=False):
    """The two-scale net of tests/test_gpu_dropin.py as our MeanFieldVI, holding the mu / rho of tests/golden/prune_ffg.npz."""
    net = M.get_net(8, 'skip', 'reflection', skip_n33d=[8, 16], skip_n33u=[8, 16], skip_n11=4, num_scales=2, n_channels=2, upsample_mode='bilinear')
    net = M.MeanFieldVI(net, reparam='', device=torch.device('cuda'), seed=3, autotune=False, flat_parameters=flat)
    assert len(net._vi) == len(g["layers"])
    with torch.no_grad():
        for i, m in enumerate(net._vi):
            mu, rho, nw = g["mu%d" % i], g["rho%d" % i], m.W_mu.numel()
            assert mu.size == nw + m.out_channels
            m.W_mu.copy_(dev(mu[:nw]).view_as(m.W_mu)); m.W_rho.copy_(dev(rho[:nw]).view_as(m.W_rho))
            m.bias_mu.copy_(dev(mu[nw:])); m.bias_rho.copy_(dev(rho[nw:]))
    return net


@pytest.mark.parametrize("flat", [False, True])
def test_dropin_masks_equal_the_reference(M, golden_dir, flat):
    import os
    g = np.load(os.path.join(golden_dir, "prune_ffg.npz"), allow_pickle=False)
    net = golden_net(M, g, flat)
    before = host(net._flat).copy()
    keys = set(net.state_dict())
    for j, a in enumerate(g["amounts"]):
        info = M.prune_weights_ffg(net, 'percentage', amount=float(a))
        assert list(info["k"]) == list(g["a%d_k" % j])
        for i, m in enumerate(net._vi):
            assert m.W_mu_mask.shape == m.W_mu.shape and m.W_mu_mask.dtype == torch.float32 and m.W_rho_mask is m.W_mu_mask
            assert np.array_equal(host(m.W_mu_mask).ravel(), g["a%d_W%d" % (j, i)]), (a, i)
            assert np.array_equal(host(m.bias_mu_mask), g["a%d_b%d" % (j, i)]) and np.array_equal(host(m.bias_rho_mask), g["a%d_b%d" % (j, i)]), (a, i)
            w0 = host(m.W_mu_mask) == 0
            assert (host(m.W_mu)[w0] == 0).all() and (host(m.W_rho)[w0] == M._lib.PRUNED_RHO).all()
            assert np.array_equal(host(m.W_mu)[~w0], before[m._w_off:m._w_off + w0.size].reshape(w0.shape)[~w0])
        assert set(net.state_dict()) == keys                                   # the masks are no buffers
        if flat:
            assert next(net.parameters()).data_ptr() == net._flat.data_ptr()
        with pytest.raises(RuntimeError, match="pruned"):
            net.kl()
        with pytest.raises(RuntimeError, match="already pruned"):
            M.prune_weights_ffg(net, 'percentage', amount=0.5)
        y = net(torch.zeros(1, 8, 32, 32, device="cuda"))                      # a pruned net still runs
        assert bool(torch.isfinite(y).all())
        M.prune_remove(net)
        assert host(net._flat).tobytes() == before.tobytes() and not hasattr(net._vi[0], "W_mu_mask")
        assert bool(torch.isfinite(net.kl()).all())


def test_dropin_refusals_and_bias_free_layer(M):
    mk = lambda: M.get_net(8, 'skip', 'reflection', skip_n33d=[8, 16], skip_n33u=[8, 16], skip_n11=4, num_scales=2, n_channels=2, upsample_mode='bilinear')
    plain = mk()
    convs = [m for m in plain.modules() if isinstance(m, torch.nn.Conv2d)]
    convs[1].bias = None                                                       # a layer without a bias: the reference crashes here
    net = M.MeanFieldVI(plain, reparam='', device=torch.device('cuda'), seed=3, autotune=False)
    assert sum(not m._has_bias for m in net._vi) == 1
    info = M.prune_weights_ffg(net, amount=0.5)
    n_b = sum(m.out_channels for m in net._vi if m._has_bias)
    assert list(info["n"]) == [net.n_vi - n_b, n_b] and list(info["k"]) == [int(0.5 * (net.n_vi - n_b)), int(0.5 * n_b)]
    free = [m for m in net._vi if not m._has_bias][0]
    assert hasattr(free, "W_mu_mask") and not hasattr(free, "bias_mu_mask")
    assert sum(int((host(m.W_mu_mask) == 0).sum()) for m in net._vi) == info["k"][0]
    M.prune_remove(net)
    with pytest.raises(RuntimeError, match="not pruned"):
        M.prune_remove(net)
    with pytest.raises(NotImplementedError, match="pdb"):
        M.prune_weights_ffg(net, mode='threshold', thresh=0.1)
    with pytest.raises(ValueError):
        M.prune_weights_ffg(net, mode='percentage', amount=1.5)
    with pytest.raises(ValueError):
        M.prune_weights_ffg(net, mode='other')
    with pytest.raises(TypeError, match="no rho"):
        M.prune_weights_ffg(M.FusedNet(mk(), autotune=False), amount=0.5)
    with pytest.raises(TypeError):
        M.prune_weights_ffg(mk(), amount=0.5)


# ---- 8. runner ---------------------------------------------------------------------------------------------------------------------------------
def test_runner_writes_pruning_npz(M, tmp_path):
    import json
    import os
    from mfvi_dip_mia_amd import prune
    cfg = dict(bo_params=dict(temp=dict(candidates=[1e-6]), sigma=dict(candidates=[0.05])),
               run_params=dict(img="phantom", num_iter=3, lr=1e-3, seed=1, p_sigma=0.1, input_depth=8, show_every=5, plot=False, save=True,
                               net_kwargs=SMALL, autotune=False, save_path=str(tmp_path / "logs")))
    path = str(tmp_path / "cfg.json")
    json.dump(cfg, open(path, "w"))
    M.runner.main(["--task", "denoising", "--config", path, "--imsize", "32", "--predict-samples", "4", "--prune-amounts", "0,0.5"])
    (d,) = os.listdir(str(tmp_path / "logs"))
    run = os.path.join(str(tmp_path / "logs"), d)
    assert {"pruning.npz", "predictive.npz", "save.npz"} <= set(os.listdir(run))
    z = np.load(os.path.join(run, "pruning.npz"), allow_pickle=False)
    assert set(z.files) == {"amount", "n_pruned", "n", "snr_threshold", "layer_sparsity", "layer_names", "psnr_mean", "epi_mean", "ale_mean", "total_mean",
                            "snr_hist_counts", "snr_hist_edges_log10"}
    n_layers = len(z["layer_names"])
    assert list(z["amount"]) == [0.0, 0.5] and z["n_pruned"].shape == (2, 2) and z["n"].shape == (2,) and z["snr_threshold"].shape == (2, 2)
    assert z["layer_sparsity"].shape == (2, n_layers) and z["snr_hist_counts"].shape == (2, prune.HIST_BINS + 2)
    assert z["snr_hist_edges_log10"].shape == (prune.HIST_BINS + 1,)
    assert list(z["n_pruned"][0]) == [0, 0] and list(z["n_pruned"][1]) == [int(0.5 * n) for n in z["n"]]
    assert np.isnan(z["snr_threshold"][0]).all() and np.isfinite(z["snr_threshold"][1]).all() and (z["layer_sparsity"][0] == 0).all()
    assert list(z["snr_hist_counts"].sum(axis=1)) == list(z["n"])
    p = np.load(os.path.join(run, "predictive.npz"))
    assert z["psnr_mean"][0] == 10.0 * np.log10(1.0 / p["err2"].astype(np.float64).mean())      # amount 0: the unpruned prediction
    assert z["epi_mean"][0] == p["epi"].astype(np.float64).mean() and z["psnr_mean"][1] != z["psnr_mean"][0]
    # without the option: no file
    cfg["run_params"]["save_path"] = str(tmp_path / "logs2")
    json.dump(cfg, open(path, "w"))
    M.runner.main(["--task", "denoising", "--config", path, "--imsize", "32", "--predict-samples", "4"])
    (d2,) = os.listdir(str(tmp_path / "logs2"))
    assert "pruning.npz" not in os.listdir(os.path.join(str(tmp_path / "logs2"), d2))
