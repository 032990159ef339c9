"""What tests/test_gpu_posterior_range.py relies on, checked on the CPU: the layouts of tests/posterior_cases.py put
every ladder value in every probed layer at every position of a quad, the elements a ratio check leaves out are the constructed share and
no more, the unit-impulse plans return every weight exactly once through the oracle's own convolution, the float64 statement is torch's
softplus, and the whole-net cases sit away from the LeakyReLU kink."""
import numpy as np
import pytest

from oracle import oracle as O
import oddmap_cases as C
import oracle_program
import posterior_cases as PC


def _layers_of(name):
    (cin, cout, k, stride, H, W), _ = PC.DRAW_CASES[name]
    return PC.single_layer(cin, cout, k), cin * cout * k * k, cout


def test_ladder_holds_the_named_points():
    L = PC.LADDER.astype(np.float64)
    assert L.size == 217 and np.unique(PC.LADDER).size == 216          # (20.0 closes the linspace and is named again)
    assert np.array_equal(PC.LADDER[:201], np.linspace(-30, 20, 201).astype(np.float32))
    c = np.log(0.06)
    edge = PC.LADDER[201:205]
    assert edge[0] < edge[1] <= c < edge[2] < edge[3] and all(np.nextafter(edge[i], np.float32(np.inf)) == edge[i + 1] for i in range(3))
    # the switch of softplus_fast (e < 0.06) falls between two of them: both branches are taken next to it
    assert np.exp(edge[0].astype(np.float64)) < 0.06 < np.exp(edge[3].astype(np.float64))
    for v in (19.9, 20.0, 25.0, 50.0, -45.0, -60.0, -87.0, -88.0, -104.0, 89.0, 120.0):
        assert np.float32(v) in PC.LADDER
    assert np.nextafter(np.float32(20.0), np.float32(np.inf)) in PC.LADDER
    # every band of the draw's bound is populated
    assert set(np.unique(PC.band_of(L))) == {-1, 0, 1, 2, 3}


@pytest.mark.parametrize("name", list(PC.DRAW_CASES))
def test_every_ladder_value_at_every_quad_position_in_every_probed_layer(name):
    layers, nw, cout = _layers_of(name)
    n = nw + cout
    seen = np.zeros((PC.N_LADDER, 4), bool); seen_broad = np.zeros(PC.N_LADDER, bool)
    for shift in PC.ladder_shifts(nw):
        _, rho = PC.layout("ladder", n, 7, shift=shift)
        t = np.arange(nw) + shift
        assert np.array_equal(rho[:nw], PC.LADDER[t % PC.N_LADDER])        # nothing but ladder values, in order
        seen[t % PC.N_LADDER, np.arange(nw) & 3] = True
        mu_b, rho_b = PC.layout("broad", n, 7, shift=shift)
        on = (t // PC.N_LADDER) % 3 == 0
        assert np.array_equal(rho_b[:nw][on], PC.LADDER[t[on] % PC.N_LADDER])
        seen_broad[t[on] % PC.N_LADDER] = True
        assert rho_b.min() >= -104 and rho_b.max() <= 120 and np.abs(mu_b).max() > 0
    assert seen.all(), "ladder values missing at a quad position: %d of 868" % (~seen).sum()
    assert seen_broad.all()
    # the bias block: every value, through shifts of its own
    got = set()
    for shift in range(0, PC.N_LADDER, cout):
        got |= set(PC.LADDER[(np.arange(cout) + shift) % PC.N_LADDER].tolist())
    assert got == set(PC.LADDER.tolist())


@pytest.mark.parametrize("name", list(PC.DRAW_CASES))
@pytest.mark.parametrize("lay", ["fitted", "broad", "pruned"])
def test_share_left_out_of_a_ratio_check_is_the_constructed_one(name, lay):
    layers, nw, cout = _layers_of(name)
    n = nw + cout
    dead = PC.dead_channels(layers) if lay == "pruned" else ()
    mu, rho = PC.layout(lay, n, 11, layers=layers, dead=dead)
    out = float((rho < PC.RATIO_FLOOR).mean())
    per = nw // cout + 1
    built = {"fitted": 0.0, "broad": 3.0 / PC.BROAD_PERIOD, "pruned": 0.25 + len(dead) * per / n}[lay]
    assert out <= built + 4.0 / n, (out, built)          # (+ one partial quad / ladder run)
    assert out < 0.30
    if lay == "pruned":
        m = rho == np.float32(PC.PRUNED_RHO)
        assert np.all(mu[m] == 0) and np.all(mu[~m] != 0) and m.mean() >= 0.24
        q = m[:nw // 4 * 4].reshape(-1, 4)
        assert np.all(q.sum(1) >= 1) and (q.sum(1) == 1).mean() > 0.9          # pruned and live weights share every quad
        assert len(set(np.argmax(q, 1)[q.sum(1) == 1].tolist())) == 4           # at every position
        w = m[:nw].reshape(cout, -1)
        assert np.all(w.any(1))                                                 # and every output channel
        for _, co in dead:
            assert w[co].all() and m[nw + co]
        assert (cout < 32) == (len(dead) == 0)
    else:
        assert rho.min() >= (-20 if lay == "fitted" else -104)
    if lay == "fitted":
        assert -14.3 < rho.mean() < -13.3 and rho.max() <= -6 and 0.08 < mu.std() < 0.12


def test_two_layouts_that_differ_in_rho_only():
    """fitted / broad share mu: the pair a bit-identical dmu is asserted on."""
    a = PC.layout("fitted", 1000, 3); b = PC.layout("broad", 1000, 3)
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", list(PC.DRAW_CASES))
def test_impulse_plans_observe_every_weight_exactly_once(name):
    """Through the oracle's convolution, reflection padding and stride included: the gathered outputs ARE the weights, bit for bit."""
    (cin, cout, k, stride, H, W), _ = PC.DRAW_CASES[name]
    passes = PC.impulse_plan(cin, k, stride, H, W)
    w = O.normal_fill(5, 2, 0, 0, 0, cout * cin * k * k).reshape(cout, cin, k, k)
    outs = [O.conv_fwd(p[0], w, np.zeros(cout, np.float32), stride) for p in passes]
    got, seen = PC.gather_weights(passes, outs, cin, cout, k)
    assert np.all(seen == 1)
    assert np.array_equal(got, w)
    for x, ci, *_ in passes:
        assert x.sum() == np.unique(ci).size and set(np.unique(x)) <= {0.0, 1.0}          # one impulse per channel used
        # an impulse is the only non-zero element the taps of its outputs see: every other product is with an exact 0
        assert np.count_nonzero(x.sum(0)) == np.unique(ci).size


def test_float64_statement_is_torchs_softplus():
    torch = pytest.importorskip("torch")
    r = torch.from_numpy(PC.LADDER.astype(np.float64))
    assert np.allclose(PC.softplus64(PC.LADDER), torch.nn.functional.softplus(r).numpy(), rtol=1e-15, atol=0)
    assert np.allclose(PC.sigmoid64(PC.LADDER), torch.sigmoid(r).numpy(), rtol=1e-15, atol=0)
    mu, rho = PC.layout("broad", 4096, 5); e = O.normal_fill(5, 2, 4, 0, 0, 4096)
    # the oracle's fp32 reparam stays inside the bound the device draw is held to
    assert np.all(np.abs(O.reparam(mu, rho, e).astype(np.float64) - PC.w64(mu, rho, e)) <= PC.draw_bound(mu, rho, e))
    # a wrong series coefficient (1/3 -> 0.3) would not
    x = rho.astype(np.float64); ex = np.exp(np.minimum(x, 20.0))
    bad = np.where(ex < 0.06, ex * (1 - ex * (0.5 - ex * 0.3)), PC.softplus64(rho))
    assert np.any(np.abs(mu + bad * e - PC.w64(mu, rho, e)) > PC.draw_bound(mu, rho, e))
    # above 20 softplus IS rho: with mu = 0 the draw is the correctly rounded product rho * eps, which the GPU test asks for bit for bit
    hi = PC.LADDER[PC.LADDER > 20].astype(np.float64)
    assert hi.size == 5 and np.array_equal(PC.softplus64(hi), hi)
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(np.float32(89.0)))          # log(1 + expf(rho)) without the branch is inf at the ladder's last two points


def test_q_metric_sees_what_the_max_normalised_one_hides():
    """sigmoid(rho) replaced by a constant: invisible to max |a - b| / max |b| where one large-rho element sets the scale, 100 % in q."""
    mu, rho = PC.layout("broad", 4096, 9)
    layers = [dict(cin=455, cout=1, k=3, w_off=0, b_off=4095)]
    q_ref = O.normal_fill(9, 2, 5, 0, 0, 4096).astype(np.float64)
    good = q_ref * PC.sigmoid64(rho)
    small = rho < -8
    bad = np.where(small, q_ref * 0.5 * PC.sigmoid64(rho), good)             # every weight below -8 wrong by a factor 2
    assert np.abs(bad - good).max() / np.abs(good).max() < 2e-4              # passes test_small_nets_fwd_bwd's tolerance
    assert PC.layer_q_err(good.astype(np.float32), q_ref, rho, layers)[0] < 1e-6
    assert PC.layer_q_err(bad.astype(np.float32), q_ref, rho, layers)[0] > 0.1


@pytest.mark.parametrize("key", list(PC.NET_SEEDS))
def test_net_cases_stay_clear_of_the_leaky_relu_kink(key):
    """At the seed of a whole-net case (the first from 77 on that does so) every BatchNorm output under a LeakyReLU is at least 2e-6 of its
    tensor's scale from zero in the oracle's forward, in every sample (the rule of tests/test_skip_restatement_host.py)."""
    import mfvi_dip_mia_amd as M
    net, lay = key
    kw = PC.NETS[net]
    P, zin, out_id, _ = M.skip_program(**kw)

    def kink(seed, step=PC.NET_STEP, k0=PC.NET_K0, n=PC.NET_N):
        mu, rho, bnp = PC.net_params(P, lay, seed)
        z = PC.net_input(kw, seed)
        k = np.inf
        for i in range(n):
            k = min(k, C.conditioning(P, oracle_program.run(P, zin, out_id, mu, rho, bnp, z, seed, step, k0 + i))[0])
            if k < PC.KINK:
                break
        return k
    seed = PC.NET_SEEDS[key]
    assert kink(seed) >= PC.KINK
    if net == "three_scale_32":          # the draws of tests/golden/posterior_range.npz: step 3, samples 0 and 1
        assert kink(seed, 3, 0, 2) >= PC.KINK
    assert net == "three_scale_32" or kink(77) < PC.KINK          # (the scan from 77 to the chosen seed is not repeated here: a thousand forwards)
    # the layout reaches every layer: pruned weights and fitted rho in each
    mu, rho, _ = PC.net_params(P, lay, seed)
    for l in P.layers:
        r = rho[l["w_off"]:l["b_off"] + l["cout"]]
        assert r.max() <= -6 and (lay != "pruned" or 0.2 < (r == np.float32(PC.PRUNED_RHO)).mean() < 0.3)
