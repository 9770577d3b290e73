"""GPU: compute_loss(iw_draws=K) -- training on the importance-weighted bound -- on the tiny models of test_gpu_ragged_compact.py, N = 3,
T = 4, K in {1,3}, L in {1,2}: order 1 with RBF and order 2 with RBF under rk4, order 1 with DF under dopri5.  The noise is fixed: the
encoders' draws through next_eps (K,N,q), the field's through its device source, re-seeded before every run.

(i)   against the torch-side composition of the same model: encoder, flow and decoder go through the package's ops; the K draws
      (iw_ref.draws_forward, float64; the float32 VALUE handed to the flow is moved onto the bits of the forward-only
      gpode_reparam_draws_fwd, at most one unit in the last place away, because dopri5 accepts and rejects steps on those bits: one
      run without this, on a model instance that the then unseeded GP initialisation did not reproduce, had decoder gradients 3e-3
      apart at a loss 2e-8 apart for df1-dopri5 K = 3, L = 1 -- supposed, not confirmed, to be another step sequence; the step
      counts of the two sides are now asserted equal, and the GP initialisation is seeded) and the loss stage (iw_ref.objective on x a - softplus(a) from the
      model's float32 logits) are plain torch.  Compared: the loss, the four reported values, model.last_ess and the gradient of every
      parameter.  Bounds: those of test_gpu_ragged_model.py / test_gpu_ragged_compact.py -- terms within loss_routes.TOL_KL (1e-5) of
      the sum of the absolute values of what they add up, gradients within 2e-5 of their largest entry, the dead biases as that file
      holds them -- WIDENED where float32 itself is further off: the composition's loss stage is evaluated a second time in float32 on the
      same logits, and a figure may be 4 times as far from float64 as that evaluation is (the floor of a figure is its largest distance
      over the four (K, L) cases of a model, as test_gpu_iw_loss.py takes it and for the reason given there).  The widening is needed
      because a softmax weight moves by 1e-4 when its a of magnitude 2e3 moves by one unit in the last place, and every gradient
      behind the loss stage carries the weights.  The encoders' noise is drawn at a twentieth of its scale: at a fresh model the K
      likelihoods of a sequence are otherwise tens of nats apart and every weight is one-hot (ess = 1.000, as evaluation reports).
      Measured on an MI355X, worst over the 12 cases (figure | its float32 distance in the same case):
        loss 1.1e-7 | 5.0e-8, iw_nll 1.1e-7 | 1.1e-7, kl_mc 1.1e-8 | 9.4e-9, kl_u 1.0e-7 | 1.5e-8 -- all inside TOL_KL, no widening;
        ess (of K) 9.7e-6 | 8.2e-6 (rbf1, K = 3, L = 1: ratio 1.2; the bound there is 4 x 8.2e-6 = 3.3e-5 in place of 1e-5);
        gradients: K = 1 at most 1.6e-6, the 2e-5 bound holds; K = 3 at most 4.05e-5 | 3.45e-5 (vae.encoder.fc.weight, rbf1, L = 1:
        ratio 1.2, bound 4 x 3.45e-5 = 1.4e-4 in place of 2e-5), rbf2 2.2e-5 | 5.5e-5 (kern.unconstrained_variance, L = 2),
        df1-dopri5 6.5e-6 | 3.5e-6 (no widening).  With ts: 1.1e-6; with n_obs: 4.1e-6.
(ii)  iw_draws=None runs no launch whose name or tag contains `iw` or `reparam_draws`, and equals a second identical call bit for bit.
(iii) evaluate.iw_stats on the step's own (ll, lw) for L = 1 equals -out[1] within TOL_KL of the largest |a|, and its mean ess equals
      model.last_ess within the ess floor of (i).
(iv)  with ts (N,T) and with n_obs the five figures equal the composition's, bounds as in (i) from the case's own float32 evaluation.
(v)   a captured step (graph.GraphedStep, device noise for the function draw AND the K-fold encoder noise) equals the eager step with
      the same seed bit for bit over the warm-up and two replays.
(vi)  each refusal of compute_loss raises."""
import copy
import functools
import unittest.mock

import pytest
import torch
import torch.nn.functional as Fn

import iw_ref as W
import loss_routes as R
from test_gpu_ragged_model import compare_grads, grads
from test_gpu_time_grids import bits, tiny_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def leave_the_global_generators_as_found():
    """as test_gpu_ragged_model.py: the tests here seed and draw from the process-wide generators; later files must not see that"""
    import random
    import numpy as np
    saved = (torch.get_rng_state(), torch.cuda.get_rng_state_all(), np.random.get_state(), random.getstate())
    yield
    torch.set_rng_state(saved[0])
    torch.cuda.set_rng_state_all(saved[1])
    np.random.set_state(saved[2])
    random.setstate(saved[3])


N, T = 3, 4
KINDS = {'rbf1-rk4': dict(), 'rbf2-rk4': dict(ode=2, D_in=6, D_out=3, latent_dim=3, frames=3), 'df1-dopri5': dict(kernel='DF', solver='dopri5')}
KL = [(1, 1), (3, 1), (1, 2), (3, 2)]
TERMS = ('loss', 'iw_nll', 'kl_mc', 'kl_u', 'ess')


def build(kind):
    import numpy as np
    np.random.seed(13)                               # build_model initialises the GP parameters from numpy's global generator
    m, src = tiny_model(**KINDS[kind])
    if 'dopri5' in kind:
        m.flow.rtol, m.flow.atol, m.flow.max_steps = 1e-4, 1e-4, 64
    return m, src


def batch(m, K, seed=5, N=N):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(N, T, 1, 28, 28, generator=g).cuda()
    q = m.vae.encoder.fc.out_features // 2
    # at a fresh model the K likelihoods of a sequence are tens of nats apart and every weight is one-hot (ess = 1.000): the noise is
    # drawn at a twentieth of its scale, which brings the draws within a few nats of each other and the weights into play
    eps = [(0.05 * torch.randn(K, N, q, generator=g)).cuda() for _ in range(m.order)]
    return X, eps


def set_eps(m, eps):
    m.vae.encoder.next_eps = eps[0]
    if m.order == 2:
        m.vae.encoder_v.next_eps = eps[1]


def run_hip(m, src, X, L, K, eps, **kw):
    """compute_loss(iw_draws=K) + backward -> (the five figures, gradients)"""
    from vae_gp_ode_amd.model.create_model import compute_loss
    m.zero_grad(set_to_none=True)
    src.manual_seed(17)
    set_eps(m, eps)
    out = compute_loss(m, X, L, iw_draws=K, **kw)
    out[0].backward()
    torch.cuda.synchronize()
    return [t.detach().clone() for t in out] + [m.last_ess.detach().clone()], grads(m)


def torch_side(m, src, X, L, K, eps, dt, ts=None, n_obs=None, N=N):
    """the composition: the model's own encoder, flow and decoder; the draws and the loss stage in plain torch (the stage in ``dt``)
    -> (five figures, their scales, gradients)"""
    from vae_gp_ode_amd import vae_ops as V
    stash = {}

    def snapped(z64, mu, lv, e):
        """z64 rounded to float32, its VALUE moved onto the bits of the forward-only draws (gpode_reparam_draws_fwd, the evaluation's
        entry, which contracts mu + sigma eps to one fma: at most one unit in the last place away) -- an adaptive solver accepts and
        rejects steps on those bits, and two step sequences would be two discretisations.  The gradient stays plain torch's."""
        z = z64.float()
        zk, _ = V.reparam_draws(mu.detach(), lv.detach(), e)
        assert float((zk - z).abs().max()) <= 2.0 ** -22 * float(z.abs().max()), 'the draws are more than a rounding apart'
        return z + (zk - z).detach()

    def draws(mu_s, lv_s, e_s, mu_v=None, lv_v=None, e_v=None):
        z64, lw = W.draws_forward(mu_s.double(), lv_s.double(), e_s.double())
        absw = (0.5 * e_s.double() ** 2 + 0.5 * z64.detach() ** 2 + 0.5 * lv_s.detach().double().abs()).sum(-1)
        z = snapped(z64, mu_s, lv_s, e_s)
        if mu_v is not None:
            zv64, lwv = W.draws_forward(mu_v.double(), lv_v.double(), e_v.double())
            absw = absw + (0.5 * e_v.double() ** 2 + 0.5 * zv64.detach() ** 2 + 0.5 * lv_v.detach().double().abs()).sum(-1)
            z, lw = torch.cat((z, snapped(zv64, mu_v, lv_v, e_v)), -1), lw + lwv
        stash['absw'] = absw
        return z.contiguous(), lw
    m.zero_grad(set_to_none=True)
    src.manual_seed(17)
    set_eps(m, eps)
    with unittest.mock.patch.object(V, 'reparam_draws_train', draws):
        logits, _, _, lw = m(X, L, logits=True, z0_draws=K, **({} if ts is None else {'ts': ts}))
    a, x = logits.to(dt).view(L, K, N, T, -1), X.to(dt).view(1, 1, N, T, -1)
    lp = x * a - Fn.softplus(a)
    if n_obs is not None:
        obs = torch.arange(T, device=X.device)[None, :] < n_obs[:, None].long()
        lp = torch.where(obs[None, None, :, :, None], lp, torch.zeros((), dtype=dt, device=X.device))
    ll = lp.sum(dim=(3, 4))
    field = m.flow.odefunc.diffeq
    nobs = float(m.num_observations)
    out = W.objective(ll, lw.to(dt), field.Um.optvar.to(dt), field.us_packed().to(dt), field.M, nobs)
    out[0].backward()
    torch.cuda.synchronize()
    ku_abs = float(W.svgp_kl_abs(field.Um.optvar.detach().double(), field.us_packed().detach().double(), field.M))
    s_iw = float((lp.detach().double().abs().sum(dim=(3, 4)) + stash['absw'][None]).max(1).values.mean())
    scale = [s_iw * nobs + ku_abs, s_iw, float(stash['absw'].mean()), ku_abs, float(K)]
    return [t.detach().double() for t in out], scale, grads(m), (ll.detach(), lw.detach())


def one_case(m, src, init, K, L, N=N, **kw):
    """-> the kernel's and the float32 composition's distances from the float64 composition: {figure: (error, floor)}, {parameter: ...}"""
    X, eps = batch(m, K, N=N)
    res, steps = {}, {}
    for tag, fn in (('hip', lambda: run_hip(m, src, X, L, K, eps, **kw)), ('f64', lambda: torch_side(m, src, X, L, K, eps, torch.float64, N=N, **kw)),
                    ('f32', lambda: torch_side(m, src, X, L, K, eps, torch.float32, N=N, **kw))):
        m.load_state_dict(init)
        res[tag] = fn()
        steps[tag] = m.flow.last_counts.clone() if m.flow.solver == 'dopri5' else None
    if steps['hip'] is not None:                     # the adaptive solver took the same steps on both sides: one discretisation
        assert torch.equal(steps['hip'], steps['f64']) and torch.equal(steps['hip'], steps['f32']), (steps['hip'], steps['f64'])
    ref, scale, gref = res['f64'][:3]
    terms = {n: (abs(float(res['hip'][0][i]) - float(ref[i])) / scale[i], abs(float(res['f32'][0][i]) - float(ref[i])) / scale[i])
             for i, n in enumerate(TERMS)}
    eh, ef = compare_grads(res['hip'][1], gref, 'iw'), compare_grads(res['f32'][2], gref, 'iw float32')
    return terms, {k: (eh[k], ef[k]) for k in eh}


@functools.lru_cache(maxsize=None)
def kind_results(kind):
    m, src = build(kind)
    init = copy.deepcopy(m.state_dict())
    out = {}
    for K, L in KL:
        out[K, L] = one_case(m, src, init, K, L)
        terms, gr = out[K, L]
        print('%s K %d L %d: terms %s; gradients worst %s' % (kind, K, L, {k: '%.1e|%.1e' % v for k, v in terms.items()},
                                                             sorted(((v[0], v[1], k) for k, v in gr.items()), reverse=True)[:3]))
    return out


def bounds(results):
    """{figure: bound}, {parameter: bound}: the other files' bounds, widened to 4 x the largest float32 distance over the cases"""
    t = {n: max(R.TOL_KL, 4 * max(r[0][n][1] for r in results.values())) for n in TERMS}
    g = {k: max(2e-5, 4 * max(r[1][k][1] for r in results.values())) for k in next(iter(results.values()))[1]}
    return t, g


@pytest.mark.parametrize('K,L', KL)
@pytest.mark.parametrize('kind', list(KINDS))
def test_iw_loss_matches_the_torch_side_composition(kind, K, L):
    results = kind_results(kind)
    tb, gb = bounds(results)
    terms, gr = results[K, L]
    bad = {n: (v, tb[n]) for n, v in terms.items() if not v[0] <= tb[n]}
    assert not bad, bad
    bad = {k: (v, gb[k]) for k, v in gr.items() if not v[0] <= gb[k]}
    assert not bad, bad
    if K == 1:                                       # one draw: every weight is exactly 1 and nothing needs widening
        assert all(v[0] <= 2e-5 for v in gr.values()), gr
        assert terms['ess'][0] == 0.0


def test_without_iw_draws_nothing_changes(monkeypatch):
    from vae_gp_ode_amd import _lib
    from vae_gp_ode_amd.model.create_model import compute_loss
    m, src = build('rbf1-rk4')
    X, _ = batch(m, 1)
    calls, real = [], _lib.call

    def call(name, *args):
        rc = real(name, *args)
        calls.append((name, _lib.load().gpode_last_launch().decode()))
        return rc
    monkeypatch.setattr(_lib, 'call', call)

    def record(**kw):
        del calls[:]
        m.zero_grad(set_to_none=True)
        src.manual_seed(17)
        out = compute_loss(m, X, 2, **kw)
        out[0].backward()
        torch.cuda.synchronize()
        return [t.detach().clone() for t in out], grads(m), list(calls)
    # (a size query launches nothing and leaves the tag of the launch before it: an entry counts by its name, or by a tag of its own)
    new = lambda cs: [c for i, c in enumerate(cs) if any(w in c[0] for w in ('iw', 'reparam_draws')) or
                      (any(w in c[1] for w in ('iw', 'reparam_draws')) and not (i and cs[i - 1][1] == c[1]))]
    (oa, ga, ca), (ob, gb, cb), (oc, gc, cc) = record(), record(iw_draws=None), record(iw_draws=3)
    assert not new(ca) and not new(cb) and ca == cb
    assert all(bits(a, b) for a, b in zip(oa, ob)) and all(bits(ga[k], gb[k]) for k in ga)
    assert [c[0] for c in new(cc)] == ['gpode_reparam_draws_fwd', 'gpode_elbo_iw_fwd', 'gpode_elbo_iw_bwd_ll', 'gpode_reparam_draws_bwd'], new(cc)
    assert [c[1] for c in new(cc)] == ['reparam_draws_fwd', 'elbo_iw_fwd', 'elbo_iw_loglik_bwd', 'reparam_draws_bwd']
    assert not [c for c in cc if c[0].startswith('gpode_sigmoid_loglik_bwd')], 'the fused backward leaves the logits nothing to launch'


def test_iw_stats_on_the_steps_own_rows(monkeypatch):
    from vae_gp_ode_amd import evaluate as E
    from vae_gp_ode_amd import vae_ops as V
    m, src = build('rbf1-rk4')
    K = 3
    X, eps = batch(m, K)
    seen, real = {}, V.elbo_iw

    def spy(lpart, lw, *a, **k):
        seen['ll'], seen['lw'] = lpart.detach().double().sum(1).view(K, N).cpu(), lw.detach().double().cpu()
        return real(lpart, lw, *a, **k)
    monkeypatch.setattr(V, 'elbo_iw', spy)
    out, _ = run_hip(m, src, X, 1, K, eps)
    iw_ll, iw_nll, ess = E.iw_stats(seen['ll'], seen['lw'])
    scale = float((seen['ll'] + seen['lw']).abs().max())
    print('iw_nll %.6f against the kernel %.6f; ess %.5f against %.5f' % (iw_nll, float(out[1]), float(ess.mean()), float(out[4])))
    assert abs(iw_nll - float(out[1])) <= R.TOL_KL * scale
    tb, _ = bounds(kind_results('rbf1-rk4'))
    assert abs(float(ess.mean()) - float(out[4])) <= tb['ess'] * K


@pytest.mark.parametrize('what', ['ts', 'n_obs'])
def test_time_grids_and_frame_counts(what):
    m, src = build('rbf1-rk4')
    init = copy.deepcopy(m.state_dict())
    kw = dict(ts=(m.dt * torch.tensor([[0, 1, 2, 3], [0, 2, 3, 5], [0, 1, 4, 6]], dtype=torch.float32)).cuda())
    if what == 'n_obs':
        kw['n_obs'] = torch.tensor([4, 2, 3], dtype=torch.int32, device='cuda')
    terms, gr = one_case(m, src, init, 3, 2, **kw)
    m.load_state_dict(init)
    X, eps = batch(m, 3)
    plain = run_hip(m, src, X, 2, 3, eps)[0]
    m.load_state_dict(init)
    this = run_hip(m, src, X, 2, 3, eps, **kw)[0]
    print('%s: terms %s; gradients worst %s' % (what, {k: '%.1e|%.1e' % v for k, v in terms.items()},
                                                 sorted(((v[0], v[1], k) for k, v in gr.items()), reverse=True)[:3]))
    assert not bits(plain[0], this[0]), 'the grid / the counts changed nothing'
    tb, gb = bounds(kind_results('rbf1-rk4'))
    bad = {n: v for n, v in terms.items() if not v[0] <= max(tb[n], 4 * v[1])}
    assert not bad, bad
    bad = {k: v for k, v in gr.items() if not v[0] <= max(gb[k], 4 * v[1])}
    assert not bad, bad


def test_graph_replay_equals_the_eager_steps():
    from vae_gp_ode_amd.graph import GraphedStep
    from vae_gp_ode_amd.model.create_model import compute_loss
    from vae_gp_ode_amd.optim import HipAdam
    m, src = build('rbf2-rk4')
    init = copy.deepcopy(m.state_dict())
    batches = [batch(m, 1, seed=5)[0], batch(m, 1, seed=6)[0]]
    order = (0, 0, 1)

    def run(use_graph):
        m.load_state_dict(init)
        src.manual_seed(17)
        opt = HipAdam(m.parameters(), lr=1e-4)
        buf = torch.empty_like(batches[0])

        def step():
            opt.zero_grad()
            out = compute_loss(m, buf, 2, iw_draws=3)
            out[0].backward()
            opt.step()
            return out + (m.last_ess,)
        outs, gs = [], None
        for b in order:
            buf.copy_(batches[b])
            if not use_graph:
                outs.append([t.detach().clone() for t in step()])
            elif gs is None:
                gs = GraphedStep(step, warmup=1)
                outs.append([t.clone() for t in gs.warm_out])
            else:
                outs.append([t.clone() for t in gs()])
        torch.cuda.synchronize()
        return outs, [p.detach().clone() for p in m.parameters()]
    try:
        oe, pe = run(False)
        og, pg = run(True)
    finally:                                         # the process-wide switch HipAdam sets for itself
        from vae_gp_ode_amd import vae_ops
        vae_ops.set_deferred_reductions(False)
    print('eager %s\ngraph %s' % ([[float(t) for t in o] for o in oe], [[float(t) for t in o] for o in og]))
    assert all(bool(torch.isfinite(t).all()) for o in oe for t in o)
    assert all(bits(a, b) for x, y in zip(oe, og) for a, b in zip(x, y))
    assert all(bits(a, b) for a, b in zip(pe, pg))
    assert not bits(oe[0][0], oe[1][0]) and not bits(oe[1][0], oe[2][0])


@pytest.mark.parametrize('case', ['compact', 'unfused', 'decoder', 'ranks', 'K = 0', 'K = 65', 'rows'])
def test_compute_loss_refusals(case, monkeypatch):
    from vae_gp_ode_amd.model import create_model as C
    m, src = build('rbf1-rk4')
    X, _ = batch(m, 1)
    kw, want = dict(iw_draws=3), None
    if case == 'compact':
        kw.update(compact=True, n_obs=torch.full((N,), T, dtype=torch.int32, device='cuda'))
        want = 'not built for compact=True'
    elif case == 'unfused':
        monkeypatch.setattr(C, '_FUSED_LOSS', False)
        want = 'GPODE_UNFUSED_LOSS=1'
    elif case == 'decoder':
        monkeypatch.setattr(m.vae.decoder, 'distribution', 'gaussian')
        want = 'Bernoulli decoder'
    elif case == 'ranks':
        monkeypatch.setattr(torch.distributed, 'is_initialized', lambda: True)
        monkeypatch.setattr(torch.distributed, 'get_world_size', lambda *a: 2)
        want = 'several ranks'
    elif case == 'K = 0':
        kw['iw_draws'], want = 0, '1..64'
    elif case == 'K = 65':
        kw['iw_draws'], want = 65, '1..64'
    else:
        X, kw['iw_draws'], want = torch.zeros(1100, 2, 1, 28, 28, device='cuda'), 64, '65535'
    with pytest.raises(ValueError, match=want):
        C.compute_loss(m, X, 1, **kw)
