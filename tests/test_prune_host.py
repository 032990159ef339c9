"""SNR pruning without a GPU: the host arithmetic of prune.py, the refusals of engines and batches ahead of the library,
the header, and the argument refusals of the new C entries (each returns before any launch)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(nd=(8, 16), nu=(8, 16), ns=(4, 4))


@pytest.fixture(scope="module")
def M():
    import mfvi_dip_mia_amd as M_
    M_.build()
    return M_


@pytest.fixture()
def no_library(M, monkeypatch):
    def refuse():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(M._lib, "lib", refuse)
    return M


def test_k_of_is_the_reference_truncation(M):
    from mfvi_dip_mia_amd.prune import k_of
    for amount, n in ((0.29, 100), (0.1, 1027), (0.5, 37), (0.9, 1035446), (1.0, 7), (0.0, 7), (1e-9, 1000), (0.57, 100), (np.float32(0.1), 1000)):
        assert k_of(amount, n) == int(float(amount) * n), (amount, n)
    assert k_of(0.29, 100) == 28 and k_of(0.57, 100) == 56                     # 0.29 * 100 = 28.999999999999996: truncation, not rounding
    assert k_of(np.float32(0.1), 1000) == 100 and k_of(1.0, 7) == 7 and k_of(0.0, 7) == 0


def test_check_amount(M):
    from mfvi_dip_mia_amd.prune import check_amount
    assert check_amount(0.25) == 0.25 and check_amount(0) == 0.0 and check_amount(1) == 1.0
    assert check_amount(0.5, 3) == [0.5, 0.5, 0.5] and check_amount([0, 0.5, 1.0], 3) == [0.0, 0.5, 1.0]
    assert check_amount(np.array([0.1, 0.2]), 2) == [0.1, 0.2]
    for bad in (-0.1, 1.0001, float("nan"), float("inf"), "half", None, [0.5]):
        with pytest.raises(ValueError):
            check_amount(bad)
    for bad in ([0.1, 0.2], [0.1, 0.2, 0.3, 0.4], [0.1, 1.5, 0.2], [0.1, float("nan"), 0.2], -1, ["a", "b", "c"]):
        with pytest.raises(ValueError):
            check_amount(bad, 3)


def test_segment_table_of_the_small_net(M):
    from mfvi_dip_mia_amd import prune
    P, _, _, _ = M.skip_program(32, 32, 8, 2, **SMALL)
    segs = prune.segment_table(P)
    assert segs == sorted(segs) and prune.check_segments(segs, P.n_vi) is segs
    assert len(segs) == 2 * len(P.layers)                                      # every layer of skip() has a bias
    covered = np.zeros(P.n_vi, np.int32)
    for lay in P.layers:
        nw = lay["cout"] * lay["cin"] * lay["k"] ** 2
        assert (lay["w_off"], nw, 0) in segs and (lay["b_off"], lay["cout"], 1) in segs
    for off, cnt, g in segs:
        covered[off:off + cnt] += 1
    assert (covered == 1).all()                                                # the segments tile [0, n_vi)
    n = prune.group_sizes(segs)
    assert n == [P.n_vi - sum(l["cout"] for l in P.layers), sum(l["cout"] for l in P.layers)]
    raw = prune.pack_segments(segs)
    assert len(raw) == 24 * len(segs) and ctypes.sizeof(M._lib.PruneSegment) == 24
    first = M._lib.PruneSegment.from_buffer_copy(raw[:24])
    assert (first.offset, first.count, first.group) == segs[0]
    # a layer without a bias: one segment
    Q = M.Program()
    a, b, c = Q.tensor(3, 8, 8), Q.tensor(4, 8, 8), Q.tensor(2, 8, 8)
    Q.conv(a, b, 3, bias=False); Q.conv(b, c, 1)
    assert prune.segment_table(Q) == [(0, 108, 0), (108, 8, 0), (116, 2, 1)] and prune.layer_names(Q) == ["layer0", "layer1"]
    for bad in ([(0, 5, 0), (3, 5, 1)], [(0, 5, 2)], [(0, 200, 0)], [(5, 2, 0), (0, 2, 0)], [(0, -1, 0)]):
        with pytest.raises(ValueError):
            prune.check_segments(bad, 100)
    with pytest.raises(ValueError):
        prune.check_segments([(i, 1, 0) for i in range(M._lib.PRUNE_MAX_SEGMENTS + 1)], 10 ** 6)


def test_hist_bounds(M):
    from mfvi_dip_mia_amd import prune
    edges, b = prune.hist_bounds(8, (-2.0, 2.0))
    assert edges.shape == (9,) and b.dtype == np.float32 and (np.diff(b) > 0).all() and b[0] == np.float32(0.01) and b[-1] == np.float32(100.0)
    for bad in ((0, (-1, 1)), (M._lib.SNR_MAX_BINS + 1, (-1, 1)), (4, (1, 1)), (4, (2, 1)), (4, (float("nan"), 1))):
        with pytest.raises(ValueError):
            prune.hist_bounds(*bad)


def _bare(cls, **attrs):
    o = object.__new__(cls)
    o.__dict__.update(attrs)
    return o


def test_engines_refuse_before_the_library(no_library):
    M = no_library
    base = dict(rank=0, world=1, param_dtype="f32", chunk=2)
    bf16 = _bare(M.engine.ElboEngine, **dict(base, param_dtype="bf16"))
    for call in (lambda: bf16.predict(4, prune=0.5), bf16.snr, lambda: bf16.prune_mask(0.5)):
        with pytest.raises(NotImplementedError, match="bf16"):
            call()
    sharded = _bare(M.engine.ElboEngine, **dict(base, world=2))
    with pytest.raises(NotImplementedError, match="world_size"):
        sharded.predict(4, prune=0.5)
    sib = _bare(M.engine.SiblingEngine, **dict(base, method="mcd"))
    for call in (lambda: sib.predict(4, prune=0.5), sib.snr, lambda: sib.prune_mask(0.5)):
        with pytest.raises(TypeError, match="no rho"):
            call()
    eng = _bare(M.engine.ElboEngine, **base)
    for bad in (-0.5, 1.5, float("nan"), [0.1, 0.2], "x"):
        with pytest.raises(ValueError):
            eng.predict(4, prune=bad)
        with pytest.raises(ValueError):
            eng.prune_mask(bad)


def test_batches_refuse_before_the_library(no_library):
    M = no_library
    sb = _bare(M.SiblingBatch, method="mcd", n_rows=2, sample_weights=False)
    for call in (lambda: sb.predict(4, prune=0.5), sb.snr, lambda: sb.prune_mask([0.5, 0.1])):
        with pytest.raises(TypeError, match="no rho"):
            call()
    for cls in (M.FitBatch, M.CtVolume, M.InpaintBatch):
        b = _bare(cls, n_rows=3)
        for bad in ([0.1, 0.2], 1.5, [0.1, -0.2, 0.3], "x"):
            with pytest.raises(ValueError):
                b.predict(4, prune=bad)
            with pytest.raises(ValueError):
                b.prune_mask(bad)


def test_header_has_the_entries_and_the_abi_version(M):
    txt = open(os.path.join(ROOT, "include", "mfvi_hip.h")).read()
    assert "#define MFVI_ABI_VERSION 6\n" in txt
    for name in ("mfvi_snr_keys", "mfvi_snr_select_scratch_bytes", "mfvi_snr_select", "mfvi_prune_apply", "mfvi_snr_histogram"):
        assert re.search(r"\b%s\s*\(" % name, txt) and name in M._lib.SIGNATURES
    assert "#define MFVI_PRUNE_MAX_SEGMENTS %d\n" % M._lib.PRUNE_MAX_SEGMENTS in txt and "#define MFVI_SNR_MAX_BINS %d\n" % M._lib.SNR_MAX_BINS in txt
    common = open(os.path.join(ROOT, "mfvi-dip-mia_amd", "csrc", "common.h")).read()
    m = re.search(r"#define MFVI_PRUNED_RHO \((-?[0-9.]+)f\)", common)
    assert m and float(m.group(1)) == M._lib.PRUNED_RHO
    r = np.float32(M._lib.PRUNED_RHO)
    assert np.isfinite(r) and np.exp(r, dtype=np.float32) == 0.0               # expf underflows to +0: every softplus of it is exactly +0


def test_c_entries_refuse_bad_arguments(M):
    """No GPU needed: every refusal returns before a launch."""
    lib = M._lib.lib()
    p = ctypes.c_void_p(0x1000)        # never dereferenced on the host
    odd = ctypes.c_void_p(0x1004)
    big = 2 ** 31
    err = lambda: lib.mfvi_last_error()
    assert lib.mfvi_snr_keys(p, 1, 2 * big, big, p, None) == -2 and b"snr_keys" in err()
    for args in ((None, 1, 20, 10, p), (p, 1, 20, 10, None), (p, 0, 20, 10, p), (p, 65536, 20, 10, p), (p, 1, 19, 10, p)):
        assert lib.mfvi_snr_keys(*args, None) == -1, args
    assert lib.mfvi_snr_keys(p, 1, 20, 0, p, None) == -2
    assert lib.mfvi_snr_select_scratch_bytes(0) == -1 and lib.mfvi_snr_select_scratch_bytes(65536) == -1 and b"snr_select_scratch_bytes" in err()
    assert lib.mfvi_snr_select_scratch_bytes(1) > 0 and lib.mfvi_snr_select_scratch_bytes(3) % 8 == 0
    ok = dict(keys=p, rows=1, n_vi=10, segs=p, n_seg=2, k=p, mask=p, thr=p, ties=p, scratch=p)
    order = ("keys", "rows", "n_vi", "segs", "n_seg", "k", "mask", "thr", "ties", "scratch")
    sel = lambda **kw: lib.mfvi_snr_select(*[dict(ok, **kw)[k] for k in order], None)
    assert sel(n_vi=big) == -2 and sel(n_vi=0) == -2 and sel(n_seg=-1) == -2 and sel(n_seg=M._lib.PRUNE_MAX_SEGMENTS + 1) == -2
    for kw in (dict(keys=None), dict(segs=None), dict(k=None), dict(mask=None), dict(thr=None), dict(ties=None), dict(scratch=None), dict(rows=0),
               dict(rows=65536), dict(scratch=odd)):
        assert sel(**kw) == -1 and b"snr_select" in err(), kw
    assert lib.mfvi_prune_apply(p, odd, p, 1, 30, big, 2 * big, None) == -2
    for args in ((None, odd, p, 1, 30, 10, 25), (p, None, p, 1, 30, 10, 25), (p, odd, None, 1, 30, 10, 25), (p, p, p, 1, 30, 10, 25), (p, odd, p, 0, 30, 10, 25),
                 (p, odd, p, 1, 30, 10, 19), (p, odd, p, 1, 24, 10, 25)):
        assert lib.mfvi_prune_apply(*args, None) == -1 and b"prune_apply" in err(), args
    hist = lambda keys=p, rows=1, n_vi=10, segs=p, n_seg=2, bounds=p, n_bins=4, counts=p: lib.mfvi_snr_histogram(keys, rows, n_vi, segs, n_seg, bounds, n_bins,
                                                                                                                 counts, None)
    assert hist(n_bins=0) == -2 and hist(n_bins=M._lib.SNR_MAX_BINS + 1) == -2 and hist(n_vi=big) == -2 and hist(n_seg=513) == -2
    for kw in (dict(keys=None), dict(segs=None), dict(bounds=None), dict(counts=None), dict(rows=0)):
        assert hist(**kw) == -1 and b"snr_histogram" in err(), kw


def test_cli_refusals(M, monkeypatch, tmp_path, capsys):
    """_check_cli refuses --prune-amounts from the arguments alone: before load_config and before the library."""
    class Accepted(Exception):
        pass

    def accepted(*a, **kw):
        raise Accepted

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(M.runner, "load_config", accepted)
    monkeypatch.setattr(M._lib, "lib", boom)
    base = ["--config", "unused.json", "--save-path", str(tmp_path)]
    for tail, text in ((["--prune-amounts", "0.5"], "needs --predict-samples"),
                       (["--bayes", "mcd", "--predict-samples", "4", "--prune-amounts", "0.5"], "no rho"),
                       (["--predict-samples", "4", "--prune-amounts", "0.5,1.5"], "outside [0, 1]"),
                       (["--predict-samples", "4", "--prune-amounts", "0.5,x"], "--prune-amounts 0.5,x"),
                       (["--predict-samples", "4", "--prune-amounts", "-0.1"], "outside [0, 1]"),
                       (["--predict-samples", "4", "--param-dtype", "bf16", "--prune-amounts", "0.5"], "bf16"),
                       (["--fits-per-launch", "2", "--batch-predict-samples", "4", "--prune-amounts", "0.5"], "--prune-amounts")):
        with pytest.raises(SystemExit) as e:
            M.runner.main(base + tail)
        err = capsys.readouterr().err
        assert e.value.code == 2 and text in err, (tail, err)
    with pytest.raises(Accepted):
        M.runner.main(base + ["--predict-samples", "4", "--prune-amounts", "0,0.5,0.9"])
    with pytest.raises(Accepted):
        M.runner.main(base + ["--predict-samples", "4"])
    assert os.listdir(str(tmp_path)) == []
    # the same refusals for run_params.prune_amounts / prune_amounts= of the run_*_mfvi functions, before anything is created
    for kw, exc in ((dict(prune_amounts=[0.5]), ValueError), (dict(prune_amounts=[0.5], predict_samples=4, method="mcd"), ValueError),
                    (dict(prune_amounts=[1.5], predict_samples=4), ValueError), (dict(prune_amounts=[0.5], predict_samples=4, param_dtype="bf16"), NotImplementedError)):
        with pytest.raises(exc):
            M.runner.run_den_mfvi(imsize=(32, 32), num_iter=1, save=True, save_path=str(tmp_path), **kw)
    assert os.listdir(str(tmp_path)) == []
    assert M.runner.parse_prune_amounts("0, 0.5,0.9") == [0.0, 0.5, 0.9]
