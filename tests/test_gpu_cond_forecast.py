"""The forecast conditioned on an observed prefix: gpode_dec10_predict_w (the importance-weighted twin of gpode_dec10_predict),
vae_ops.dec10_predict_w, evaluate.predict_conditional / cond_stats / compute_forecast and ``--eval_condition_frames``.

Kernel level (tests/cond_ref.py holds inputs, reference and runner): random c of L = 5 draws of F = 15 frames (N = 3, Th = 5, T_obs = 4),
the state arrays NaN-filled with guards behind them, against exact softmax weights and direct weighted sums in float64 with the bound
relerr(hip, fp64) <= 2e-5 + 3 relerr(fp32 restatement, fp64) on mean, M2/W, wse/W and W exp(ref) -- every figure printed before it is
asserted, no floor raised.  The weight sets each aim at one failure: sorted ascending every draw rescales, descending none does, random
mixes them; a draw 200 below the top underflows to weight 0 and must leave the bits of the state alone; -inf is weight 0 (also as the
FIRST draw, while the reference is still -inf); equal weights must give the unweighted twin's moments; a dominant draw must give a
variance of 0 and not a cancellation residue; log-weights near 3000 are handed over relative to draw 0, as evaluate does.  The effective
sample size of the reference is asserted on the inputs, so that a degenerate weight set cannot hide a wrong fold.

Model level: the tiny models of tests/test_gpu_z0_draws.py, N = 4, T = 5, L = 6, n_cond = 2, T_custom = 7."""
import json
import math

import pytest
import torch

import cond_ref as R
from cond_ref import F, L, N, TH, T_OBS, relerr

pytestmark = pytest.mark.gpu


def _weights(kind):
    """(L,N) float64 log-weights of the named set"""
    g = torch.Generator().manual_seed(5)
    base = 1.2 * torch.randn(L, N, generator=g, dtype=torch.float64)
    if kind == 'random':
        return base
    if kind == 'ascending':
        return base.sort(dim=0).values
    if kind == 'descending':
        return base.sort(dim=0, descending=True).values
    if kind == 'equal':
        return torch.full((L, N), 0.75, dtype=torch.float64)
    if kind == 'dominant':
        base[3] += 100.0
        return base
    if kind == 'minus_inf':
        base[1, 0] = -math.inf
        base[0, 1] = -math.inf                                        # the first draw folded: the reference is still -inf
        base[0, 2] = base[1, 2] = -math.inf
        return base
    raise KeyError(kind)


# ---- 1. against the float64 reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['random', 'ascending', 'descending', 'minus_inf'])
def test_weighted_moments_match_the_reference(kind):
    lw = _weights(kind)
    ess = R.ess64(lw)
    print(kind, 'ess of the reference:', [round(v, 3) for v in ess.tolist()])
    if kind == 'random':
        assert ((ess >= 2) & (ess <= L - 1)).any()                   # a condition on the inputs: the weights do spread over the draws
    got = R.run(lw)
    assert got['tags'] == ['dec10_predict_w'] and got['tags'][0].endswith('_w')
    for k in ('wstate', 'mean', 'm2', 'wse'):
        assert torch.isfinite(got[k]).all(), k
    R.check(got, lw, kind)
    # forecast frames t >= T_obs: the moments are filled, the error is 0
    wse = got['wse'].view(N, TH)
    assert (wse[:, T_OBS:] == 0).all() and (wse[:, :T_OBS] > 0).all()
    # the reference of every frame of a sequence is the largest log-weight handed over (in float32), W counts against it
    top = lw.float().max(0).values
    assert torch.equal(got['wstate'][:, 0].view(N, TH), top[:, None].expand(N, TH))


def test_a_draw_that_underflows_leaves_the_state_bit_for_bit():
    lw = _weights('random')
    lw[2] = lw.max(0).values - 200.0                                   # exp(-200) is 0 in float32
    with_it = R.run(lw)
    keep = [0, 1, 3, 4]
    without = R.run(lw[keep], draws=keep)
    for k in ('wstate', 'mean', 'm2', 'wse'):
        assert torch.equal(with_it[k], without[k]), k
        assert torch.isfinite(with_it[k]).all(), k
    R.check(with_it, lw, 'one draw 200 below the top')
    # ... and as the LAST draw, behind everything: still nothing
    order = [0, 1, 3, 4, 2]
    last = R.run(lw[order], draws=order)
    for k in ('wstate', 'mean', 'm2', 'wse'):
        assert torch.equal(last[k], without[k]), k


def test_equal_weights_give_the_unweighted_twin():
    from vae_gp_ode_amd import vae_ops as V
    lw = _weights('equal')
    got = R.run(lw)
    r64 = R.check(got, lw, 'equal weights')
    i = R.inputs()
    st = V.PredictState(F, 'cuda', True)
    V.dec10_predict(i['c'].cuda().view(-1, 16, 28, 28), i['table'].cuda(), i['w'].cuda(), i['b'].cuda(), i['X'].cuda(), TH, st)
    r32 = R.reference(lw, torch.float32)
    assert torch.equal(got['wstate'][:, 1], torch.full((F,), float(L)))
    for name, a, b, want, k in (('mean', got['mean'], st.mean, r64['mean'], 'mean'),
                                ('M2', got['m2'], st.m2, r64['var'] * L, 'var'),
                                ('var = m2 / L', got['var'], st.m2 / L, r64['var'], 'var')):
        bound = R.FLOOR + 3 * relerr(r32[k], r64[k])
        e_tw, e_w, e_p = relerr(a, b), relerr(a, want), relerr(b, want)
        print('equal weights %-12s: %.2e from the twin (weighted %.2e, twin %.2e from float64; bound %.2e)' % (name, e_tw, e_w, e_p, bound))
        assert e_tw <= bound and e_w <= bound, (name, e_tw, e_w, bound)


def test_a_dominant_draw_gives_no_variance():
    lw = _weights('dominant')
    ess = R.ess64(lw)
    print('dominant: ess of the reference', ess.tolist())
    assert (ess - 1).abs().max() < 1e-6 and (ess == 1).any()          # the inputs are degenerate, as meant
    got = R.run(lw)
    r64, r32 = R.reference(lw, torch.float64), R.reference(lw, torch.float32)
    bound = R.FLOOR + 3 * relerr(r32['mean'], r64['mean'])
    e = relerr(got['mean'], r64['mean'])
    scale = r64['mean'].abs().max().item()
    vmax = got['var'].abs().max().item()
    print('dominant: mean %.2e from float64 (bound %.2e); max M2/W %.3e against %.3e = bound x the mean\'s scale %.3f'
          % (e, bound, vmax, bound * scale, scale))
    assert e <= bound
    assert vmax <= bound * scale
    assert relerr(got['mean'].view(N, TH, 784), R.images(torch.float64)[3]) <= bound      # the forecast IS the dominant draw
    assert relerr(got['wmse'][:, :T_OBS], r64['wmse'][:, :T_OBS]) <= R.FLOOR + 3 * relerr(r32['wmse'], r64['wmse'])


def test_log_weights_of_realistic_magnitude_relative_to_draw_0():
    g = torch.Generator().manual_seed(8)
    lw = 3000.0 + 1.5 * torch.randn(L, N, generator=g, dtype=torch.float64) + 40.0 * torch.randn(1, N, generator=g, dtype=torch.float64)
    rel = lw - lw[0]                                                   # what evaluate.predict_conditional hands over
    print('log-weights near 3000: ess', [round(v, 3) for v in R.ess64(lw).tolist()])
    got = R.run(rel.float())
    R.check(got, rel, 'near 3000, relative')
    # the weights themselves are those of the absolute log-weights: the shift cancels in the softmax
    a, b = R.reference(lw, torch.float64), R.reference(rel, torch.float64)
    assert relerr(a['mean'], b['mean']) < 1e-12 and relerr(a['var'], b['var']) < 1e-9


# ---- 2. splits, ragged sequences -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['random', 'ascending', 'minus_inf'])
def test_any_split_of_the_draws_gives_the_bits_of_one_launch(kind):
    lw = _weights(kind)
    one = R.run(lw)
    for splits in ([2, 3], [1, 1, 1, 1, 1]):
        parts = R.run(lw, splits=splits)
        assert len(parts['tags']) == len(splits)
        for k in ('wstate', 'mean', 'm2', 'wse'):
            assert torch.equal(one[k], parts[k]), (splits, k)


def test_ragged_sequences():
    lw = _weights('random')
    n_obs = [4, 2, 0]
    X = R.inputs()['X'].clone()
    for n, k in enumerate(n_obs):
        X[n, k:] = float('nan')                                        # what the padded targets hold must reach nothing
    got = R.run(lw, n_obs=n_obs, X=X)
    assert got['tags'] == ['dec10_predict_len_w']
    full = R.run(lw)
    wse = got['wse'].view(N, TH)
    for n, k in enumerate(n_obs):
        assert (wse[n, k:] == 0).all() and torch.equal(wse[n, :k], full['wse'].view(N, TH)[n, :k])
    for k in ('wstate', 'mean', 'm2', 'wse'):
        assert torch.isfinite(got[k]).all(), k
    assert torch.equal(got['mean'], full['mean']) and torch.equal(got['m2'], full['m2']) and torch.equal(got['wstate'], full['wstate'])
    R.check(got, lw, 'ragged', n_obs=n_obs)
    for splits in ([2, 3], [1, 1, 1, 1, 1]):
        parts = R.run(lw, splits=splits, n_obs=n_obs, X=X)
        assert all(torch.equal(got[k], parts[k]) for k in ('wstate', 'mean', 'm2', 'wse'))


def test_python_refusals_and_the_nan_flag():
    from vae_gp_ode_amd import _lib, vae_ops as V
    i = R.inputs()
    c, tb, w, b, X = (i[k].cuda() for k in ('c', 'table', 'w', 'b', 'X'))
    c = c.view(-1, 16, 28, 28)
    lw = torch.zeros(L, N, device='cuda')
    st = V.CondState(F, N, 'cuda')
    with pytest.raises(_lib.GpodeError, match='logw must be'):
        V.dec10_predict_w(c, tb, w, b, X, TH, st, lw.double())
    with pytest.raises(_lib.GpodeError, match='logw must be'):
        V.dec10_predict_w(c, tb, w, b, X, TH, st, lw[:, :2].contiguous())
    with pytest.raises(_lib.GpodeError, match='need done \\+ Lc'):
        V.dec10_predict_w(c, tb, w, b, X, TH, st, lw[:4].contiguous())
    with pytest.raises(_lib.GpodeError, match='CondState'):
        V.dec10_predict_w(c, tb, w, b, X, TH, V.PredictState(F, 'cuda'), lw)
    with pytest.raises(_lib.GpodeError, match='F = N \\* Th'):
        V.dec10_predict_w(c, tb, w, b, X, TH + 1, st, lw)
    assert st.done == 0 and (st.wstate == 0).all()
    # the library's own refusals, through the binding, with nothing written
    sentinel = torch.full((F, 2), 7.0, device='cuda')
    with pytest.raises(_lib.GpodeError, match='gpode_dec10_predict_w: logw has L_total rows, need done \\+ Lc <= L_total'):
        _lib.call('gpode_dec10_predict_w', V._ptr(c), V._ptr(tb), V._ptr(w), V._ptr(b), V._ptr(X), L, F, TH, T_OBS, 1, V._ptr(lw), L, N,
                  V._ptr(sentinel), V._ptr(st.mean), V._ptr(st.m2), V._ptr(st.wse), V._ptr(None), V._stream())
    with pytest.raises(_lib.GpodeError, match='gpode_dec10_predict_w: need N >= 1 and F = N \\* Th'):
        _lib.call('gpode_dec10_predict_w', V._ptr(c), V._ptr(tb), V._ptr(w), V._ptr(b), V._ptr(X), L, F, TH, T_OBS, 0, V._ptr(lw), L, 2,
                  V._ptr(sentinel), V._ptr(st.mean), V._ptr(st.m2), V._ptr(st.wse), V._ptr(None), V._stream())
    assert (sentinel == 7.0).all()
    # a NaN (or +inf) log-weight: flagged on the device, refused where the state is read; -inf is a weight like any other
    for bad in (float('nan'), float('inf')):
        st = V.CondState(F, N, 'cuda')
        lwb = lw.clone()
        lwb[2, 1] = bad
        V.dec10_predict_w(c, tb, w, b, X, TH, st, lwb)
        with pytest.raises(_lib.GpodeError, match='NaN or \\+inf'):
            st.check()
    st = V.CondState(F, N, 'cuda')
    lwb = lw.clone()
    lwb[2, 1] = -float('inf')
    assert V.dec10_predict_w(c, tb, w, b, X, TH, st, lwb).check() is st


# ---- 3. the model -----------------------------------------------------------------------------------------------------------------------
LM, NM, TM, KC, THM = 6, 4, 5, 2, 7


def _armed(kw):
    """the tiny random model of test_gpu_z0_draws, its sequences, and arm(): queue the same draws again"""
    from test_gpu_z0_draws import _eval_model
    m, gp, gen = _eval_model(kw)
    q = m.vae.latent_dim
    X = torch.rand(NM, TM, 1, 28, 28, generator=gen).cuda()
    noises = [gp._take_noise() for _ in range(LM)]
    eps = [torch.randn(LM, NM, q, generator=gen).cuda() for _ in range(2)]

    def arm():
        gp._next_noise.clear(); gp.set_noise(*noises)
        m.vae.encoder.next_eps = eps[0]
        if m.order == 2:
            m.vae.encoder_v.next_eps = eps[1]
    return m, X, arm


@pytest.fixture(scope='module')
def rbf1():
    from vae_gp_ode_amd import evaluate as E
    m, X, arm = _armed(dict())
    m.train()
    flags = [mod.training for mod in m.modules()]
    arm()
    p = E.predict_conditional(m, X, LM, KC, T_custom=THM)
    assert [mod.training for mod in m.modules()] == flags
    arm()
    pm = E.predict_marginal(m, X, LM)
    return m, X, arm, p, pm


def test_predict_conditional_is_consistent_with_predict_marginal(rbf1):
    from vae_gp_ode_amd import evaluate as E
    m, X, arm, p, pm = rbf1
    assert isinstance(p, E.ConditionalPrediction) and p.passes == [LM]
    assert tuple(p.mean.shape) == tuple(p.var.shape) == (NM, THM, 1, 28, 28) and p.logw.dtype == torch.float64 and p.logw.device.type == 'cpu'
    assert tuple(p.logw.shape) == (LM, NM) and all(tuple(v.shape) == (NM,) for v in (p.ess, p.evidence, p.fc_ll))
    assert all(tuple(v.shape) == (TM,) for v in (p.fc_nlpd_t, p.fc_mse_t, p.fc_mse_uncond_t))
    # conditioned on every observed frame the weights are those of the marginal likelihood: predict_marginal under the same draws
    arm()
    full = E.predict_conditional(m, X, LM, TM)
    e_ll = relerr(full.logw, pm.lw + pm.ll)
    print('n_cond = T: logw against lw + ll of predict_marginal: %.2e' % e_ll)
    assert e_ll <= 1e-12
    iw_ll, _, ess = E.iw_stats(pm.ll, pm.lw)
    assert relerr(full.evidence, iw_ll) <= 1e-12 and relerr(full.ess, ess) <= 1e-12
    assert math.isnan(full.fc_nlpd) and torch.isnan(full.fc_nlpd_t).all() and (full.fc_ll == 0).all()    # nothing is left to forecast
    # n_cond = 2 < T: the identity log p(x_{>=k} | x_{<k}) = log p(x) - log p(x_{<k}), estimate by estimate
    e_id = (p.fc_ll - (iw_ll - p.evidence)).abs().max().item()
    print('fc_ll against iw_ll - evidence: %.2e' % e_id)
    assert e_id <= 1e-9
    assert abs(p.fc_nlpd + p.fc_ll.mean().item()) <= 1e-12 * abs(p.fc_nlpd)
    assert ((p.ess >= 1) & (p.ess <= LM)).all()
    print('ess', [round(v, 3) for v in p.ess.tolist()], 'fc_mse %.5f uncond %s' % (p.fc_mse, [round(v, 5) for v in p.fc_mse_uncond_t.tolist()]))
    assert torch.isnan(p.fc_mse_t[:KC]).all() and torch.isfinite(p.fc_mse_t[KC:]).all() and torch.isfinite(p.fc_mse_uncond_t[KC:]).all()
    assert abs(p.fc_mse - p.fc_mse_t[KC:].mean().item()) <= 1e-12


def test_logw_is_lw_plus_the_prefix_of_ell_and_the_stats_are_cond_stats(rbf1):
    from vae_gp_ode_amd import evaluate as E, vae_ops as V
    m, X, arm, p, pm = rbf1
    # ell (L,N,T) under the same seed, from the route predict_marginal takes (dec10_predict with loglik on the same trajectories)
    arm()
    with torch.no_grad():
        m.eval()
        z0, lw, _, _ = m.encode_initial_state(X, draws=LM)
        ztL = m.sample_trajectories(z0, TM, LM)
        dec = m.vae.decoder
        c, t8 = dec.decode_frozen_raw(ztL, dec._frozen_tables())
        st = V.PredictState(NM * TM, X.device, False, loglik=LM)
        V.dec10_predict(c, t8, dec.decnn[10].weight, dec.decnn[10].bias, X, TM, st)
        m.train()
    ell = st.ell.cpu().double().view(LM, NM, TM)
    assert torch.equal(ell.sum(2), pm.ll)                              # it IS predict_marginal's pass
    want = pm.lw + ell[:, :, :KC].sum(-1)
    e = relerr(p.logw, want)
    print('logw against lw + ell[:, :, :2].sum(-1) of the marginal pass: %.2e' % e)
    assert e <= 1e-12
    cs = E.cond_stats(ell, pm.lw, KC, TM)
    assert relerr(cs.logw, p.logw) <= 1e-12
    for name in ('evidence', 'ess', 'fc_ll', 'fc_nlpd_t'):
        a, b = getattr(p, name), getattr(cs, name)
        ok = torch.isfinite(b)
        assert torch.equal(torch.isfinite(a), ok) and relerr(a[ok], b[ok]) <= 1e-12, name
    assert abs(p.fc_nlpd - cs.fc_nlpd) <= 1e-12 * abs(cs.fc_nlpd)


def test_mean_and_var_are_the_weighted_moments_of_the_decoded_draws(rbf1):
    m, X, arm, p, pm = rbf1
    arm()
    with torch.no_grad():
        m.eval()
        z0, _, _, _ = m.encode_initial_state(X, draws=LM)
        ztL = m.sample_trajectories(z0, THM, LM)
        img = m.vae.decoder(ztL).view(LM, NM, THM, 784)
        m.train()
    wn = torch.softmax(p.logw, dim=0)
    res = {}
    for dt in (torch.float64, torch.float32):
        z, w_ = img.cpu().to(dt), wn.to(dt)
        mean = (w_[:, :, None, None] * z).sum(0)
        res[dt] = (mean, (w_[:, :, None, None] * (z - mean[None]) ** 2).sum(0))
    for name, got, j in (('mean', p.mean, 0), ('var', p.var, 1)):
        e, e32 = relerr(got.view(NM, THM, 784), res[torch.float64][j]), relerr(res[torch.float32][j], res[torch.float64][j])
        # the decoder in front of the last stage is float32 on both sides; its own distance from float64 is not in this comparison
        print('model %-4s: %.2e from the float64 weighted moments of the eval-mode decodings (float32 restatement %.2e, bound %.2e)'
              % (name, e, e32, R.FLOOR + 3 * e32))
        assert e <= R.FLOOR + 3 * e32, (name, e)
    assert torch.isfinite(p.mean).all() and torch.isfinite(p.var).all() and (p.var >= 0).all()


def test_the_split_into_passes_does_not_enter(rbf1):
    from vae_gp_ode_amd import evaluate as E
    m, X, arm, p, pm = rbf1
    for per, passes in ((1, [1] * 6), (2, [2] * 3), (6, [6])):
        arm()
        q = E.predict_conditional(m, X, LM, KC, T_custom=THM, images_per_pass=per * NM * THM)
        assert q.passes == passes
        assert torch.equal(q.mean, p.mean) and torch.equal(q.var, p.var) and torch.equal(q.logw, p.logw)
        assert q.fc_mse == p.fc_mse and torch.equal(q.fc_mse_t[KC:], p.fc_mse_t[KC:]) and torch.equal(q.fc_mse_uncond_t[KC:], p.fc_mse_uncond_t[KC:])
        assert torch.equal(q.ess, p.ess) and torch.equal(q.evidence, p.evidence) and torch.equal(q.fc_ll, p.fc_ll)


def test_arguments_and_grids(rbf1):
    from vae_gp_ode_amd import evaluate as E
    m, X, arm, p, pm = rbf1
    # a prefix per sequence: every sequence is what it is in a batch where all share its prefix
    kc = torch.tensor([2, 3, 5, 1])
    arm()
    q = E.predict_conditional(m, X, LM, kc, T_custom=THM)
    for k in sorted(set(kc.tolist())):
        arm()
        r = E.predict_conditional(m, X, LM, k, T_custom=THM)
        sel = kc == k
        assert torch.equal(q.logw[:, sel], r.logw[:, sel]) and torch.equal(q.mean[sel.cuda()], r.mean[sel.cuda()])
        assert torch.equal(q.ess[sel], r.ess[sel]) and torch.equal(q.fc_ll[sel], r.fc_ll[sel])
    assert q.fc_ll[2] == 0                                             # conditioned on all of its frames
    # ts as (N,Th): the uniform grid written out gives the bits of the default
    ts = (m.dt * torch.arange(THM, dtype=torch.float32))[None].expand(NM, THM).contiguous().cuda()
    arm()
    r = E.predict_conditional(m, X, LM, KC, T_custom=THM, ts=ts)
    assert relerr(r.logw, p.logw) <= 1e-5 and relerr(r.mean, p.mean) <= 1e-4
    arm()
    r2 = E.predict_conditional(m, X, LM, KC, T_custom=THM, ts=(ts * torch.linspace(1.0, 1.3, NM).cuda()[:, None]).contiguous())
    assert not torch.equal(r2.mean, r.mean) and torch.isfinite(r2.mean).all()
    with pytest.raises(ValueError, match='ts'):
        E.predict_conditional(m, X, LM, KC, T_custom=THM, ts=ts[:, :3])
    # ragged: a sequence shorter than the prefix is conditioned on what it has
    nb = torch.tensor([5, 1, 3, 4], dtype=torch.int32).cuda()
    Xr = X.clone()
    for n, k in enumerate(nb.tolist()):
        Xr[n, k:] = float('nan')
    arm()
    rg = E.predict_conditional(m, Xr, LM, 3, T_custom=THM, n_obs=nb)
    assert torch.isfinite(rg.mean).all() and torch.isfinite(rg.logw).all() and math.isfinite(rg.fc_mse)
    arm()
    r1 = E.predict_conditional(m, X, LM, 1, T_custom=THM)
    assert torch.equal(rg.logw[:, 1], r1.logw[:, 1]) and rg.fc_ll[1] == 0 and rg.fc_ll[2] == 0


def test_order_2_needs_the_frames_its_velocity_encoder_reads():
    from vae_gp_ode_amd import evaluate as E
    m, X, arm = _armed(dict(ode=2, D_in=6, D_out=3, latent_dim=3))
    assert m.order == 2 and m.v_steps == 5
    with pytest.raises(ValueError, match='encoder reads the first 5'):
        E.predict_conditional(m, X, LM, 4)
    arm()
    p = E.predict_conditional(m, X, LM, 5, T_custom=THM)
    assert torch.isfinite(p.mean).all() and (p.fc_ll == 0).all() and math.isnan(p.fc_nlpd)


def test_compute_forecast_over_a_loader(rbf1):
    from vae_gp_ode_amd import evaluate as E
    m, X, arm, p, pm = rbf1

    class Loader:
        def __iter__(self):
            arm()
            yield X
    mse, nlpd, ess = E.compute_forecast(m, Loader(), LM, KC)
    arm()
    q = E.predict_conditional(m, X, LM, KC)
    assert abs(mse - q.fc_mse) <= 1e-12 * q.fc_mse and abs(nlpd - q.fc_nlpd) <= 1e-12 * abs(q.fc_nlpd) and abs(ess - q.ess.mean().item()) < 1e-12
    assert torch.equal(q.logw, p.logw)                                 # the roll-out length does not enter the weights


# ---- 4. the command line, in process --------------------------------------------------------------------------------------------------
def test_cli_forecasts_only_when_asked(tmp_path, capsys):
    import numpy as np
    from vae_gp_ode_amd import evaluate as E
    from vae_gp_ode_amd.model.create_model import build_model
    from vae_gp_ode_amd.model.misc.torch_utils import seed_everything
    argv = ['--task', 'synthetic', '--Ndata', '8', '--Ntest', '6', '--batch', '4', '--T', '6', '--solver', 'rk4', '--num_inducing', '16',
            '--num_features', '32', '--model_path', str(tmp_path), '--eval_sample_size', '4', '--Troll', '2', '--save', str(tmp_path / 'ev'),
            '--device_noise', 'True']
    args = E.make_parser().parse_args(argv)
    args.device = torch.device('cuda')
    seed_everything(3)
    torch.save(build_model(args).to(args.device).state_dict(), tmp_path / 'odegpvae_mnist.pth')
    new = ('cond_frames', 'fc_mse', 'fc_mse_uncond', 'fc_nlpd', 'fc_mse_t', 'fc_nlpd_t', 'cond_ess_mean', 'cond_ess_min')

    def text(path):
        d = json.load(open(path))
        d['ms'] = 0
        return json.dumps(d)
    plain = E.main(argv)
    files = sorted(f.name for f in (tmp_path / 'ev').iterdir())
    off_text = text(tmp_path / 'ev' / 'eval.json')
    assert not any(k in plain for k in new) and 'forecast_mean.npy' not in files
    E.main(argv + ['--eval_condition_frames', '0'])
    assert text(tmp_path / 'ev' / 'eval.json') == off_text and sorted(f.name for f in (tmp_path / 'ev').iterdir()) == files
    capsys.readouterr()
    ret = E.main(argv + ['--eval_condition_frames', '2'])
    out = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')][-1])
    assert out == json.loads(json.dumps(ret)) and json.load(open(tmp_path / 'ev' / 'eval.json')) == out
    assert list(out)[:len(plain)] == list(plain) and tuple(list(out)[len(plain):]) == new
    assert {k: v for k, v in out.items() if k not in new + ('ms',)} == {k: v for k, v in plain.items() if k != 'ms'}
    assert out['cond_frames'] == 2 and len(out['fc_mse_t']) == len(out['fc_nlpd_t']) == 6
    assert all(v is None for v in out['fc_mse_t'][:2] + out['fc_nlpd_t'][:2])          # a frame nobody forecasts: null, not NaN
    assert all(math.isfinite(v) for v in out['fc_mse_t'][2:] + out['fc_nlpd_t'][2:])
    assert all(math.isfinite(out[k]) for k in ('fc_mse', 'fc_mse_uncond', 'fc_nlpd', 'cond_ess_mean', 'cond_ess_min'))
    assert 1 <= out['cond_ess_min'] <= out['cond_ess_mean'] <= 4 and out['fc_mse'] > 0
    fm, fv = np.load(tmp_path / 'ev' / 'forecast_mean.npy'), np.load(tmp_path / 'ev' / 'forecast_var.npy')
    assert fm.shape == fv.shape == (3, 12, 1, 28, 28) and np.isfinite(fm).all() and (fv >= 0).all()
