"""GPU: an initial state PER Monte-Carlo draw -- gpode_rollout_fwd_nz / _adaptive_fwd_nz / _dense_fwd_nz, gpode_reparam_draws_fwd, their
routing through ops.rollout / ops.flow, and evaluate.predict_marginal (the importance-weighted marginal held-out likelihood).

What is held, and to what:
  * one `_nz` launch over L draws with z0 (L,N,D) against L single-draw launches on (pack[l], z0[l]): BITS (torch.equal) -- the property
    test_gpu_draws.py holds for a shared z0; every forward route of the fixed-grid dispatch (shapes of integrator_routes.py, route read
    back from gpode_last_launch()), and dopri5 landing / dense with its reverse sweep on the team and on the wave mapping and on the same
    route shapes;
  * z0_per_draw = 0, and z0_per_draw = 1 on L copies of one z0, against the `_n` entry point: BITS;
  * the gradient of a (L,N,D) leaf against ops.rollout_bwd on the same record: BITS; GP parameter gradients with L copies against the
    shared flow: BITS;
  * reparam_draws: z against gpode_reparam_fwd draw by draw: BITS.  lw against float64 on the same float32 inputs:
        |d| <= (Q + 8) 2^-24 sum_i (eps^2 + (|mu| + sigma |eps|)^2 + |logvar|),    Q = terms summed into the row (q, or 2q for both halves)
    -- Q serial float32 additions, each at most 2^-24 of the magnitudes summed so far, plus the rounding of every term (two products, an
    fma, the exponential's few ulp on sigma, which enters z^2 twice): 8 roundings' worth;
  * predict_marginal: ll against the float64 logit form on the logits of the route the suite already tests, to the suite's standing 2e-4
    of the largest value; the statistics against iw_stats exactly; ll against predict(loglik=True) on the same draws: BITS."""
import json
import math

import pytest
import torch

import integrator_routes as IR
from test_eval_loglik_host import loglik64_from_logits
from test_gpu_draws import _build, _noise, _params
from test_gpu_eval import model_args
from test_gpu_forward import relerr

pytestmark = pytest.mark.gpu

L, T = 3, 4
TS4 = (0.0, 0.05, 0.2, 0.3)                          # non-uniform, as integrator_routes.TS


# ---- launches through the C ABI -------------------------------------------------------------------------------------------------------
def _tag():
    from vae_gp_ode_amd import _lib
    return _lib.load().gpode_last_launch().decode()


def _one_draw(cb, l):
    """draw l of a stacked cache as a single-draw cache: its slab of the pack, nothing rebuilt"""
    from vae_gp_ode_amd import ops
    c = ops.GPCache()
    c.kernel, c.Di, c.Do, c.M, c.S, c.nd, c.stacked = cb.kernel, cb.Di, cb.Do, cb.M, cb.S, 1, False
    c.pack = cb.pack[l].contiguous()
    return c


def _raw_fixed(cb, z0, ts, order, method, flag, save=True):
    """gpode_rollout_fwd_n (flag None) or gpode_rollout_fwd_nz with z0_per_draw = flag, on NaN-filled outputs: rc, zt, xstage"""
    from vae_gp_ode_amd import _lib
    from vae_gp_ode_amd.ops import KERNEL_ID, METHOD_ID, NSTAGE, _ptr, _stream
    N, D = z0.shape[-2:]
    nT = ts.shape[0]
    zt = torch.full((cb.nd, N, nT, D), float('nan'), device='cuda')
    xs = torch.full((cb.nd, N, nT - 1, NSTAGE[method], D), float('nan'), device='cuda') if save else None
    head = (KERNEL_ID[cb.kernel], order, METHOD_ID[method], cb.Di, cb.Do, cb.M, cb.S, cb.nd, _ptr(cb.pack), _ptr(z0), _ptr(ts), N, nT,
            _ptr(zt), _ptr(xs))
    lib = _lib.load()
    rc = lib.gpode_rollout_fwd_n(*head, _stream()) if flag is None else lib.gpode_rollout_fwd_nz(*head, flag, _stream())
    return rc, zt, xs


def _raw_adaptive(cb, z0, ts, order, K, dense, flag, nd=None, z0_null=False):
    """the adaptive twins the same way: rc, (zt, counts, xstage, hstep, iend[, theta])"""
    from vae_gp_ode_amd import _lib
    from vae_gp_ode_amd.ops import KERNEL_ID, _ptr, _stream
    N, D = z0.shape[-2:]
    nT = ts.shape[0]
    nan = lambda *s: torch.full(s, float('nan'), device='cuda')
    zt, xs, hs = nan(cb.nd, N, nT, D), nan(cb.nd, N, K, 7 if dense else 6, D), nan(cb.nd, N, K)
    ie = torch.full((cb.nd, N, nT - 1), -7, dtype=torch.int32, device='cuda')
    counts = torch.full((cb.nd, N, 4), -7, dtype=torch.int32, device='cuda')
    th = nan(cb.nd, N, nT - 1)
    head = (KERNEL_ID[cb.kernel], order, 3, cb.Di, cb.Do, cb.M, cb.S, cb.nd if nd is None else nd, _ptr(cb.pack),
            _ptr(None if z0_null else z0), _ptr(ts), N, nT, 1e-4, 1e-4, K, _ptr(zt), _ptr(xs), _ptr(hs), _ptr(ie))
    lib = _lib.load()
    if dense:
        head = head + (_ptr(th), _ptr(counts))
        rc = lib.gpode_rollout_dense_fwd_n(*head, _stream()) if flag is None else lib.gpode_rollout_dense_fwd_nz(*head, flag, _stream())
        return rc, (zt, counts, xs, hs, ie, th)
    head = head + (_ptr(counts),)
    rc = lib.gpode_rollout_adaptive_fwd_n(*head, _stream()) if flag is None else lib.gpode_rollout_adaptive_fwd_nz(*head, flag, _stream())
    return rc, (zt, counts, xs, hs, ie)


def _per_draw_states(z0, seed):
    """(L,N,D): the case's initial states, moved by a different amount in every draw"""
    g = torch.Generator().manual_seed(seed)
    return (z0[None] + 0.3 * torch.randn(L, *z0.shape, generator=g)).cuda()


# ---- 1. fixed grid: every forward route -----------------------------------------------------------------------------------------------
def _route_cases():
    """the first 'full' case of integrator_routes.TABLE for every forward route, at L = 3 draws and T = 4"""
    seen = {}
    for c, route in IR.TABLE.items():
        if c.kind == 'full' and route not in seen:
            seen[route] = c._replace(nd=L, T=3)      # T = 3: the table's own input generator; the grid of this file has T = 4
    assert set(seen) == set(IR._F)
    return [(r, seen[r]) for r in IR._F]


@pytest.mark.parametrize('route,c', _route_cases(), ids=[r for r, _ in _route_cases()])
def test_fixed_grid_per_draw_launch_equals_single_draw_launches(route, c):
    from vae_gp_ode_amd import ops
    assert IR.forward_route(c) == route
    p, nz, z0, _, _ = IR.inputs(c)
    dev_in = ({k: v.cuda() for k, v in p.items()}, {k: v.cuda() for k, v in nz.items()})
    cb = IR.build(c, dev_in)
    ts = torch.tensor(TS4).cuda()
    z0L = _per_draw_states(z0, 7)
    ztb, xsb = ops.rollout(cb, z0L, ts, c.order, c.method, save_stages=True)
    assert _tag() == 'rollout_' + route, (_tag(), route)
    assert tuple(ztb.shape) == (L, c.N, T, c.Di) and not torch.isnan(ztb).any() and not torch.isnan(xsb).any()
    for l in range(L):
        zt1, xs1 = ops.rollout(_one_draw(cb, l), z0L[l], ts, c.order, c.method, save_stages=True)
        assert _tag() == 'rollout_' + route
        assert torch.equal(ztb[l], zt1) and torch.equal(xsb[l], xs1), (route, 'draw', l)
    assert not torch.equal(ztb[0], ztb[1])                              # the draws did start from different states
    # the shared form: flag 0 is the `_n` entry point; flag 1 on L copies of one z0 is it too
    z0s = z0.cuda()
    rc, zn, xn = _raw_fixed(cb, z0s, ts, c.order, c.method, None)
    assert rc == 0
    for flag, z in ((0, z0s), (1, z0s[None].expand(L, -1, -1).contiguous())):
        rc, zz, xz = _raw_fixed(cb, z, ts, c.order, c.method, flag)
        assert rc == 0 and _tag() == 'rollout_' + route
        assert torch.equal(zz, zn) and torch.equal(xz, xn), (route, 'z0_per_draw', flag)
    # without the record, as evaluation calls it
    assert torch.equal(ops.rollout(cb, z0L, ts, c.order, c.method), ztb)


# ---- 2. dopri5, landing and dense -----------------------------------------------------------------------------------------------------
ADAPT = [('rbf1', 'RBF', 6, 6, 24, 32), ('rbf2', 'RBF', 6, 3, 24, 32), ('df', 'DF', 4, 4, 16, 32)]
ANCHOR_ROWS, ANCHOR_TOL, ANCHOR_BOUND = 683, 1e-5, 3e-4 + 2e-4


def _dopri5_cases():
    """The small caches of ADAPT at 1, 5, 300 and 2049 rows, then the nine route shapes of _route_cases() (their fixed-grid method is
    not used), each in landing and in dense mode: (id, (route, kernel, Di, Do, M, S, N, dense, table case))"""
    out = []
    for name, kernel, Di, Do, M, S in ADAPT:
        for N in (1, 5, 300, 2049):
            for dense in (False, True):
                out.append(('%s-%d-%s' % (name, N, 'dense' if dense else 'landing'), (None, kernel, Di, Do, M, S, N, dense, None)))
    for route, c in _route_cases():
        for dense in (False, True):
            out.append(('%s-%s' % (route, 'dense' if dense else 'landing'), (route, c.kernel, c.Di, c.Do, c.M, c.S, c.N, dense, c)))
    return out


def _dopri5_setup(route, kernel, Di, Do, M, S, N, c):
    """the cache of L draws, the initial states (N,Di) on the CPU, the tag of the forward launch and the tag of the reverse sweep"""
    from vae_gp_ode_amd import ops
    k = kernel.lower()
    if c is None:                                                       # M <= 24, S = 32, Do <= 6: register-resident on either side
        p = {kk: v.cuda() for kk, v in _params(kernel, Di, Do, M, 3).items()}
        nz = {kk: v.cuda() for kk, v in _noise(kernel, Di, Do, M, S, L, 4).items()}
        cb = _build(ops, kernel, p, nz)
        cb.check_factorisation()
        z0 = torch.randn(N, Di, generator=torch.Generator().manual_seed(50 + N))
        return cb, z0, 'rollout_adaptive_%s%s' % (k, '_team' if N <= 2048 else ''), 'rollout_adaptive_bwd_' + k
    assert IR.forward_route(c) == route
    p, nz, z0, _, _ = IR.inputs(c)
    cb = IR.build(c, ({kk: v.cuda() for kk, v in p.items()}, {kk: v.cuda() for kk, v in nz.items()}))
    mapping = route[len(k):] if 'team' in route else ''                 # _team, _team_stream; every wave route reports the family alone
    return cb, z0, 'rollout_adaptive_' + k + mapping, 'rollout_adaptive_bwd_%s%s' % (k, '' if IR.backward_resident(c) else '_stream')


def _solve_all(ops, cb, z0, ts, order, tol, dense, save):
    """ops.rollout_adaptive with a budget no trajectory exhausts: (its outputs, the budget)"""
    K = 4 * (T - 1)
    while True:
        out = ops.rollout_adaptive(cb, z0, ts, order, tol, tol, K, save_stages=save, dense=dense)
        if int(out[1][..., 2].max()) == 0 or K >= 512:
            return out, K
        K *= 2


@pytest.mark.parametrize('case', [v for _, v in _dopri5_cases()], ids=[i for i, _ in _dopri5_cases()])
def test_dopri5_per_draw_launch_equals_single_draw_launches(case):
    """N = 1, 5, 300: one workgroup per trajectory (the team mapping, up to 2048 rows); N = 2049: one wavefront per trajectory.
    The route shapes run dopri5 and its reverse sweep on every evaluator of the forward dispatch and on both reverse ones.  On the
    wave routes the first 683 rows, solved on their own by the team kernels, anchor the values: the bound and tolerance of
    test_gpu_dopri5.test_wave_and_team_mappings_agree (3e-4 + 2e-4 at rtol = atol = 1e-5).  Measured on an MI355X with the dispatch
    as it was before the launchers shared one selector, landing / dense: rbf_reg42 3.9e-6 / 9.1e-6, rbf_reg11 2.9e-6 / 1.5e-5, rbf_stream
    2.2e-6 / 1.7e-5, df_lds 1.8e-5 / 1.2e-5, df_stream 6.0e-6 / 2.7e-5 -- no case needs a bound of its own."""
    from vae_gp_ode_amd import ops
    route, kernel, Di, Do, M, S, N, dense, c = case
    name = route or kernel
    order = Di // Do
    cb, z0, want, want_bwd = _dopri5_setup(route, kernel, Di, Do, M, S, N, c)
    z0L = _per_draw_states(z0, 8)
    ts = torch.tensor(TS4).cuda() * 4                                   # long enough intervals for more than one step each
    out, K = _solve_all(ops, cb, z0L, ts, order, 1e-4, dense, True)
    assert _tag() == want, (_tag(), want)
    assert int(out[1][..., 2].max()) == 0 and len(out) == (6 if dense else 5)
    assert not torch.isnan(out[0]).any() and int(out[1][..., 0].min()) >= 1
    # the reverse sweep on the record, all draws in one launch
    gzt = torch.randn(L, N, T, Di, generator=torch.Generator().manual_seed(60 + N)).cuda()
    bwd = ops.rollout_adaptive_bwd(cb, out[2], out[3], out[4], gzt, order, theta=out[5] if dense else None)
    assert _tag() == want_bwd, (_tag(), want_bwd)
    assert not torch.isnan(bwd[0]).any() and not torch.isnan(bwd[1]).any()
    for l in range(L):
        c1 = _one_draw(cb, l)
        one = ops.rollout_adaptive(c1, z0L[l], ts, order, 1e-4, 1e-4, K, save_stages=True, dense=dense)
        assert _tag() == want
        for i, (a, b) in enumerate(zip(out, one)):
            assert torch.equal(a[l], b), (name, N, 'draw', l, 'output', i)
        bwd1 = ops.rollout_adaptive_bwd(c1, one[2], one[3], one[4], gzt[l], order, theta=one[5] if dense else None)
        assert _tag() == want_bwd
        assert torch.equal(bwd[0][l], bwd1[0]) and torch.equal(bwd[1][l], bwd1[1]), (name, N, 'draw', l, 'reverse sweep')
    assert not torch.equal(out[0][0], out[0][1])
    # shared form, through the C ABI on NaN-filled buffers
    z0s = z0.cuda()
    rc, ref = _raw_adaptive(cb, z0s, ts, order, K, dense, None)
    assert rc == 0
    for flag, z in ((0, z0s), (1, z0s[None].expand(L, -1, -1).contiguous())):
        rc, got = _raw_adaptive(cb, z, ts, order, K, dense, flag)
        assert rc == 0 and _tag() == want
        for i, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), (name, N, 'z0_per_draw', flag, 'output', i)
    # without the record
    zt, counts = ops.rollout_adaptive(cb, z0L, ts, order, 1e-4, 1e-4, K, dense=dense)
    assert torch.equal(zt, out[0]) and torch.equal(counts, out[1])
    # the values of a wave route against the team kernels, which the fixed-grid route tests hold to fp64
    if c is not None and N > IR.TEAM_MAX_ROWS:
        (zw, cw), _ = _solve_all(ops, cb, z0L, ts, order, ANCHOR_TOL, dense, False)
        (zq, cq), _ = _solve_all(ops, cb, z0L[:, :ANCHOR_ROWS].contiguous(), ts, order, ANCHOR_TOL, dense, False)
        assert _tag() in ('rollout_adaptive_%s_team' % kernel.lower(), 'rollout_adaptive_%s_team_stream' % kernel.lower())
        assert int(cw[..., 2].max()) == 0 and int(cq[..., 2].max()) == 0
        e = relerr(zq, zw[:, :ANCHOR_ROWS])
        print('%s %s: first %d rows on the team kernels vs the wave route %.2e  bound %.2e' %
              (route, 'dense' if dense else 'landing', ANCHOR_ROWS, e, ANCHOR_BOUND))
        assert e < ANCHOR_BOUND, (route, e)


# ---- 3. gradients ---------------------------------------------------------------------------------------------------------------------
def _tiny_model(kernel, order, q, solver='rk4'):
    from vae_gp_ode_amd.model.core.initialization import initialize_and_fix_kernel_parameters
    from vae_gp_ode_amd.model.create_model import build_model
    torch.manual_seed(21)
    m = build_model(model_args(kernel=kernel, ode=order, D_in=q * order, D_out=q, latent_dim=q, num_inducing=16, num_features=32, solver=solver)).cuda()
    initialize_and_fix_kernel_parameters(m, 2.0, 1.0, fix=False)
    return m


@pytest.mark.parametrize('kernel,order,q,method,adaptive', [('RBF', 1, 6, 'rk4', None), ('RBF', 2, 3, 'midpoint', None),
                                                            ('DF', 1, 4, 'dopri5', (1e-4, 1e-4, 64, None, False)),
                                                            ('RBF', 1, 6, 'dopri5', (1e-4, 1e-4, 64, None, True))])
def test_gradient_of_per_draw_initial_states(kernel, order, q, method, adaptive):
    from vae_gp_ode_amd import ops
    m = _tiny_model(kernel, order, q)
    gp = m.flow.odefunc.diffeq
    D, N = q * order, 5
    nzs = [{k: v[0].cuda() for k, v in _noise(kernel, D, q, 16, 32, 1, 30 + l).items()} for l in range(L)]
    g = torch.Generator().manual_seed(31)
    z0 = torch.randn(N, D, generator=g)
    W = torch.randn(L, N, T, D, generator=g).cuda()
    ts = torch.tensor(TS4).cuda() * (4 if method == 'dopri5' else 1)
    params = [p for p in gp.parameters() if p.requires_grad]
    assert len(params) == 5

    def run(z):
        for p in params:
            p.grad = None
        gp._next_noise.clear(); gp.set_noise(*nzs)
        z = z.clone().requires_grad_(True)
        zt = ops.flow(gp, z, ts, order, method, draws=L, adaptive=adaptive)
        (zt * W).sum().backward()
        return z.grad, [p.grad.clone() for p in params], zt.detach(), gp.cache

    # a (L,N,D) leaf: its gradient is the reverse sweep's gz0, slab by slab
    gz, _, zt, cache = run(_per_draw_states(z0, 9))
    assert tuple(gz.shape) == (L, N, D) and cache.stacked and cache.nd == L
    zt2, rec = ops.rollout(cache, _per_draw_states(z0, 9), ts, order, method, save_stages=True,
                           **({} if adaptive is None else dict(rtol=adaptive[0], atol=adaptive[1], max_steps=adaptive[2], dense=adaptive[4])))
    assert torch.equal(zt2, zt)
    if method == 'dopri5':
        assert int(rec[3][..., 2].max()) == 0
    gz0, _ = ops.rollout_bwd(cache, rec, W, ts, order, method)
    for l in range(L):
        assert torch.equal(gz[l], gz0[l]), ('draw', l)
    assert gz.abs().max().item() > 0
    # L copies of one z0 against the shared flow: the same trajectories, the same five parameter gradients, and the copies' gradients
    # add up to the shared one (the same sum over the leading axis)
    gs, ps, zs, _ = run(z0.cuda())
    gc, pc, zc, _ = run(z0.cuda()[None].expand(L, -1, -1).contiguous())
    assert tuple(gs.shape) == (N, D) and tuple(gc.shape) == (L, N, D)
    assert torch.equal(zs, zc) and torch.equal(gc.sum(0), gs)
    for a, b, p in zip(ps, pc, params):
        assert torch.equal(a, b), tuple(p.shape)
        assert a.abs().max().item() > 0


# ---- 4. reparam_draws -----------------------------------------------------------------------------------------------------------------
def _lw_check(lw, mu, logvar, eps, Q, what):
    """lw (L,N) against float64 on the same float32 inputs; mu / logvar / eps: lists of the halves summed into it"""
    ref, mag = 0.0, 0.0
    for m_, lv, e in zip(mu, logvar, eps):
        m_, lv, e = m_.double().cpu(), lv.double().cpu(), e.double().cpu()
        sg = torch.exp(0.5 * lv)
        z = m_ + sg * e
        ref = ref + (0.5 * e * e - 0.5 * z * z + 0.5 * lv).sum(-1)
        mag = mag + (e * e + (m_.abs() + sg * e.abs()) ** 2 + lv.abs()).sum(-1)
    d = (lw.double().cpu() - ref).abs()
    bound = (Q + 8) * 2.0 ** -24 * mag
    print('%s: lw worst |d| %.3e, worst ratio to the bound %.3f (bound at that entry %.3e)' %
          (what, d.max().item(), (d / bound).max().item(), bound.flatten()[(d / bound).argmax()].item()))
    assert torch.isfinite(lw).all() and (d <= bound).all(), what


@pytest.mark.parametrize('Ld,N,q', [(1, 1, 1), (3, 5, 6), (4, 7, 16), (5, 300, 6)])
def test_reparam_draws(Ld, N, q):
    from vae_gp_ode_amd import vae_ops as V
    g = torch.Generator().manual_seed(Ld * 1000 + N * 10 + q)
    h = [torch.cat((1.5 * torch.randn(N, q, generator=g), -1.0 + 1.5 * torch.randn(N, q, generator=g)), 1).cuda() for _ in range(2)]
    mu, logvar = [x[:, :q] for x in h], [x[:, q:] for x in h]
    eps = [torch.randn(Ld, N, q, generator=g).cuda() for _ in range(2)]
    runs = []
    for _ in range(2):
        out = torch.full((Ld, N, 2 * q), float('nan'), device='cuda')      # ldz = 2q: the two halves of an order-2 state
        zs, lw = V.reparam_draws(mu[0], logvar[0], eps[0], out=out, col=0)
        assert tuple(lw.shape) == (Ld, N) and zs.data_ptr() == out.data_ptr()
        assert torch.isnan(out[..., q:]).all() and not torch.isnan(out[..., :q]).any()       # the other half is not touched
        lw0 = lw.clone()
        zv, lw2 = V.reparam_draws(mu[1], logvar[1], eps[1], out=out, col=q, lw=lw)
        assert lw2.data_ptr() == lw.data_ptr() and zv.data_ptr() == out.data_ptr() + 4 * q
        runs.append((out, lw0, lw.clone()))
    out, lw0, lw1 = runs[0]
    for l in range(Ld):
        for half in range(2):
            assert torch.equal(out[l, :, half * q:(half + 1) * q], V.reparam(mu[half], logvar[half], eps[half][l])), ('draw', l, 'half', half)
    _lw_check(lw0, mu[:1], logvar[:1], eps[:1], q, 'L=%d N=%d q=%d accumulate 0' % (Ld, N, q))
    _lw_check(lw1, mu, logvar, eps, 2 * q, 'L=%d N=%d q=%d accumulate 1' % (Ld, N, q))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    # a fresh output of its own: the same bits
    z, lw = V.reparam_draws(mu[0], logvar[0], eps[0])
    assert torch.equal(z, out[..., :q]) and torch.equal(lw, lw0)


# ---- 5. zero-padded width: the draws are built one by one -------------------------------------------------------------------------------
@pytest.mark.parametrize('solver', ['rk4', 'dopri5'])
def test_padded_width_falls_back_to_a_loop_over_the_draws(solver):
    from vae_gp_ode_amd import ops
    m = _tiny_model('RBF', 1, 5, solver)
    m.flow.rtol = m.flow.atol = 1e-4
    m.flow.max_steps = 64
    gp = m.flow.odefunc.diffeq
    assert gp.width_pad is not None and not gp.batched_draws_supported()
    N = 4
    nzs = [{k: v[0].cuda() for k, v in _noise('RBF', 5, 5, 16, 32, 1, 40 + l).items()} for l in range(L)]
    z0L = _per_draw_states(torch.randn(N, 5, generator=torch.Generator().manual_seed(41)), 10)
    ts = m.dt * torch.arange(T, dtype=torch.float).cuda()
    with torch.no_grad():
        gp.set_noise(*nzs)
        want = torch.stack([m.flow(z0L[l], ts) for l in range(L)])
        gp.set_noise(*nzs)
        a = m.sample_trajectories(z0L, T, L)
        gp.set_noise(*nzs)
        b = m.flow(z0L, ts, draws=L)
        gp.set_noise(*nzs)
        c = m.flow(z0L, ts)
    assert tuple(want.shape) == (L, N, T, 5) and not torch.isnan(want).any()
    assert torch.equal(a, want) and torch.equal(b, want) and torch.equal(c, want)
    assert not gp._next_noise
    # and the gradient reaches every slab
    gp.set_noise(*nzs)
    z = z0L.clone().requires_grad_(True)
    m.flow(z, ts, draws=L).sum().backward()
    assert tuple(z.grad.shape) == (L, N, 5) and all(z.grad[l].abs().max().item() > 0 for l in range(L))
    with pytest.raises(ops._lib.GpodeError, match='asked for 2'):
        ops.flow(gp, z0L, ts, 1, 'rk4', draws=2)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_entry_point_and_write_nothing():
    from vae_gp_ode_amd import _lib, ops
    from vae_gp_ode_amd.ops import _ptr, _stream
    lib = _lib.load()
    err = lambda: lib.gpode_last_error().decode()
    p = {k: v.cuda() for k, v in _params('RBF', 6, 6, 16, 3).items()}
    nz = {k: v.cuda() for k, v in _noise('RBF', 6, 6, 16, 32, L, 4).items()}
    cb = _build(ops, 'RBF', p, nz)
    N = 4
    z0L = torch.randn(L, N, 6).cuda()
    ts = torch.tensor(TS4).cuda()

    def untouched(ts_):
        torch.cuda.synchronize()
        return all((torch.isnan(t).all() if t.is_floating_point() else (t == -7).all()).item() for t in ts_)

    # fixed grid: a bad flag, no draws, no z0
    for flag in (2, -1):
        rc, zt, xs = _raw_fixed(cb, z0L, ts, 1, 'rk4', flag)
        assert rc != 0 and err().startswith('gpode_rollout_fwd_nz:') and 'z0_per_draw' in err() and untouched((zt, xs))
    full, cb.nd = cb.nd, 0
    rc, zt, xs = _raw_fixed(cb, z0L, ts, 1, 'rk4', 1)
    cb.nd = full
    assert rc != 0 and err().startswith('gpode_rollout_fwd_nz:') and 'draws=0' in err()
    from vae_gp_ode_amd.ops import KERNEL_ID
    zt, xs = torch.full((L, N, T, 6), float('nan'), device='cuda'), torch.full((L, N, T - 1, 4, 6), float('nan'), device='cuda')
    rc = lib.gpode_rollout_fwd_nz(KERNEL_ID['RBF'], 1, 1, 6, 6, cb.M, cb.S, L, _ptr(cb.pack), _ptr(None), _ptr(ts), N, T, _ptr(zt), _ptr(xs), 1,
                                  _stream())
    assert rc != 0 and err() == 'gpode_rollout_fwd_nz: null pointer' and untouched((zt, xs))
    # adaptive, landing and dense
    for dense, name in ((False, 'gpode_rollout_adaptive_fwd_nz'), (True, 'gpode_rollout_dense_fwd_nz')):
        for kw in (dict(flag=2), dict(flag=-1), dict(flag=1, nd=0), dict(flag=1, z0_null=True)):
            rc, outs = _raw_adaptive(cb, z0L, ts, 1, 8, dense, **kw)
            assert rc != 0 and err().startswith(name + ':'), (name, kw, err())
            assert untouched(outs), (name, kw)
    # through ops: a leading size that is not the cache's draws; a single-draw cache
    with pytest.raises(_lib.GpodeError, match='z0 must be'):
        ops.rollout(cb, z0L[:2], ts, 1, 'rk4')
    with pytest.raises(_lib.GpodeError, match='z0 must be'):
        ops.rollout(cb, z0L[:2], ts, 1, 'dopri5')
    with pytest.raises(_lib.GpodeError, match='z0 must be'):
        ops.rollout(_one_draw(cb, 0), z0L[:1], ts, 1, 'rk4')
    # reparam_draws
    mu, lv, eps = torch.randn(N, 6).cuda(), torch.randn(N, 6).cuda(), torch.randn(L, N, 6).cuda()
    z, lw = torch.full((L, N, 6), float('nan'), device='cuda'), torch.full((L, N), float('nan'), device='cuda')
    call = lambda mu_=mu, q=6, ld=6, ldz=6, acc=0: lib.gpode_reparam_draws_fwd(_ptr(mu_), _ptr(lv), ld, _ptr(eps), _ptr(z), ldz, _ptr(lw), acc, L, N,
                                                                             q, _stream())
    for kw in (dict(acc=2), dict(ldz=5), dict(ld=5), dict(q=17, ld=17, ldz=17), dict(q=0), dict(mu_=None)):
        assert call(**kw) != 0 and err().startswith('gpode_reparam_draws_fwd:'), kw
    assert untouched((z, lw))
    # and the calls the refusals were variations of go through
    assert call() == 0 and _raw_fixed(cb, z0L, ts, 1, 'rk4', 1)[0] == 0 and _raw_adaptive(cb, z0L, ts, 1, 64, True, 1)[0] == 0
    torch.cuda.synchronize()
    assert torch.isfinite(z).all() and torch.isfinite(lw).all()


# ---- 7. predict_marginal end to end ---------------------------------------------------------------------------------------------------
def _eval_model(kw):
    """the random models of test_gpu_eval_loglik.test_nll_matches_compute_loss_on_the_same_draws"""
    from vae_gp_ode_amd.model.core.initialization import initialize_and_fix_kernel_parameters
    from vae_gp_ode_amd.model.create_model import build_model
    torch.manual_seed(11)
    m = build_model(model_args(num_inducing=16, num_features=32, dt=0.5, **kw)).cuda()
    initialize_and_fix_kernel_parameters(m, 2.0, 1.0)
    gp = m.flow.odefunc.diffeq
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():
        gp.Um.optvar.add_(2.0 * torch.randn(gp.Um.optvar.shape, generator=gen).cuda())
        for i in (2, 5, 8):
            bn = m.vae.decoder.decnn[i]
            bn.running_mean.copy_(0.3 * torch.randn(bn.weight.shape[0], generator=gen))
            bn.running_var.copy_(0.5 + torch.rand(bn.weight.shape[0], generator=gen))
    return m, gp, gen


@pytest.mark.parametrize('kw', [dict(), dict(ode=2, D_in=6, D_out=3, latent_dim=3), dict(kernel='DF')], ids=['rbf1', 'rbf2', 'df'])
def test_predict_marginal_end_to_end(kw):
    from vae_gp_ode_amd import evaluate as E
    Lm, N, Tm = 4, 3, 4
    m, gp, gen = _eval_model(kw)
    q = m.vae.latent_dim
    X = torch.rand(N, Tm, 1, 28, 28, generator=gen).cuda()
    noises = [gp._take_noise() for _ in range(Lm)]
    eps = [torch.randn(Lm, N, q, generator=gen).cuda() for _ in range(2)]

    def arm(e):
        gp._next_noise.clear(); gp.set_noise(*noises)
        m.vae.encoder.next_eps = e[0]
        if m.order == 2:
            m.vae.encoder_v.next_eps = e[1]
    m.train()
    flags = [mod.training for mod in m.modules()]
    arm(eps)
    p = E.predict_marginal(m, X, Lm, images_per_pass=2 * N * Tm)
    assert [mod.training for mod in m.modules()] == flags and m.vae.encoder.next_eps is None and not gp._next_noise
    assert isinstance(p, E.MarginalPrediction) and p.passes == [2, 2]
    assert tuple(p.ll.shape) == (Lm, N) and tuple(p.lw.shape) == (Lm, N) and p.ll.dtype == p.lw.dtype == torch.float64
    assert p.ll.device.type == 'cpu' and tuple(p.nll_t.shape) == (Tm,) and tuple(p.ess.shape) == (N,) and tuple(p.iw_ll.shape) == (N,)
    # the same trajectories through the route the suite already tests, in float64 from its logits
    arm(eps)
    m.eval()
    with torch.no_grad():
        z0, lw, code_s, code_v = m.encode_initial_state(X, draws=Lm)
        ztL = m.sample_trajectories(z0, Tm, Lm)
        lat = ztL if m.order == 1 else ztL[..., :q]
        a = m.vae.decoder.decode_frozen(lat, logits=True).view(Lm, N, Tm, 784)
    m.train()
    assert tuple(z0.shape) == (Lm, N, m.order * q) and not torch.equal(ztL[0, :, 0], ztL[1, :, 0])
    assert torch.equal(ztL[:, :, 0], z0)                               # draw l starts from its own sample
    ll64 = loglik64_from_logits(a.double().cpu(), X.view(N, Tm, 784).double().cpu()[None]).sum(2)
    e = relerr(p.ll, ll64)
    print('%s: ll %.2e of max|ll| = %.1f from the float64 logit form; nll %.4f nlpd %.4f iw_nll %.4f ess %s' %
          (kw, e, ll64.abs().max().item(), p.nll, p.nlpd, p.iw_nll, [round(v, 3) for v in p.ess.tolist()]))
    assert e < 2e-4
    assert torch.equal(p.lw, lw.double().cpu())
    halves = [(code_s, eps[0])] + ([(code_v, eps[1])] if m.order == 2 else [])
    _lw_check(p.lw, [c[0] for c, _ in halves], [c[1] for c, _ in halves], [e_ for _, e_ in halves], q * m.order, str(kw))
    # the statistics are iw_stats / loglik_stats on those arrays
    iw_ll, iw_nll, ess = E.iw_stats(p.ll, p.lw)
    assert torch.equal(p.iw_ll, iw_ll) and p.iw_nll == iw_nll and torch.equal(p.ess, ess)
    assert p.nll == -p.ll.mean().item() and p.nlpd == -E.log_mean_exp(p.ll).mean().item() and p.nlpd <= p.nll
    assert (p.ess >= 1).all() and (p.ess <= Lm).all() and math.isfinite(p.iw_nll) and math.isfinite(p.mse) and math.isfinite(p.std)
    assert abs(float(p.nll_t.sum()) - p.nll) < 1e-9 * abs(p.nll)
    # one eps for all draws and the same function draws: the trajectories, and so ll and the error statistics, are predict's, bit for bit
    same = [e_[:1].expand(Lm, -1, -1).contiguous() for e_ in eps]
    arm(same)
    pm = E.predict_marginal(m, X, Lm)
    arm([e_[0] for e_ in eps])
    pp = E.predict(m, X, Lm, variance=False, loglik=True)
    assert torch.equal(pm.ll, pp.ll) and pm.nll == pp.nll and pm.nlpd == pp.nlpd and torch.equal(pm.nll_t, pp.nll_t)
    assert pm.state == pp.state and pm.mse == pp.mse and pm.std == pp.std
    assert (pm.lw == pm.lw[:1]).all()

    # a loader of two unequal batches: means over all sequences
    class Loader:
        def __iter__(self):
            for i, sl in enumerate((slice(0, 1), slice(1, N))):
                arm([e_[:, sl].contiguous() for e_ in eps])
                yield X[sl] if i == 0 else (X[sl],)
    iw, nlpd, ess_mean = E.compute_iw_nll(m, Loader(), Lm)
    parts = []
    for sl in (slice(0, 1), slice(1, N)):
        arm([e_[:, sl].contiguous() for e_ in eps])
        parts.append(E.predict_marginal(m, X[sl], Lm))
    assert iw == (parts[0].iw_nll * 1 + parts[1].iw_nll * (N - 1)) / N and nlpd == (parts[0].nlpd * 1 + parts[1].nlpd * (N - 1)) / N
    assert ess_mean == (parts[0].ess.sum().item() + parts[1].ess.sum().item()) / N


# ---- 8. the command line, in process --------------------------------------------------------------------------------------------------
def test_cli_reports_the_marginal_likelihood_only_when_asked(tmp_path, capsys):
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
    new = ('iw_nll', 'nlpd_marginal', 'ess_mean', 'ess_min')
    capsys.readouterr()
    plain = E.main(argv)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')][-1]
    assert not any(k in plain for k in new) and json.loads(line) == json.loads(json.dumps(plain))
    ret = E.main(argv + ['--eval_z0_draws', 'True'])
    out = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')][-1])
    assert out == json.loads(json.dumps(ret)) and json.load(open(tmp_path / 'ev' / 'eval.json')) == out
    assert all(k in out and math.isfinite(out[k]) for k in new)
    assert 1 <= out['ess_min'] <= out['ess_mean'] <= 4 and out['nlpd_marginal'] > 0
    # everything else is what it is without the flag (the same seed gives the same draws; the marginal pass comes last)
    assert list(out)[:len(plain)] == list(plain)
    assert {k: v for k, v in out.items() if k not in new + ('ms',)} == {k: v for k, v in plain.items() if k != 'ms'}
