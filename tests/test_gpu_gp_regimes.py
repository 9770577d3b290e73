"""The GP path across hyper-parameter regimes (tests/gp_regimes.py): lengthscales from 0.5 to 30, variances from 0.01 to 28, different in
every dimension, states among the inducing points and far from all of them.  Every other GPU test draws its hyper-parameters next to
the initialisation (ell = 2, var = 1), where a kernel that reads var[a] for var[b] or ell[i,d] for ell[d,i] computes the right numbers
(tests/test_gp_regimes_host.py shows both, and that every input used here is well posed).

The regimes go through the harnesses the route tests use, so NaN-filled outputs, guard floats, exact workspace sizes, the bit-identical
second run and the gpode_last_launch() tags are those of gp_routes.run_case / check_case and integrator_routes.run_case:

  cache build and backward   gp_regimes.cache_cases(): nu, u, f_prior(Z), Lu, zt and the gradients of raw_ell, raw_var, Z, Um, Us, z0
  integrator, reverse sweep  gp_regimes.integrator_cases(): f in three modes, zt, xstage, gz0, astage, gx and the leaf gradients, on
                             every forward evaluator, both reverse families, every param_grad kernel and the fused sweep
  public operators           kernel_matrix, f_update, kern_cache + rhs mode 1, conditional (diag, full_cov), conditional_df (diag, point,
                             full), rhs_jvp modes 0 / 1 / 2; RBF (6,6) and DF (6), all eight regimes
  the layer through autograd SVGP_Layer + Flow, rk4, RBF order 1 and 2 and DF, var_spread and ell_spread: kernels.py, svpy.py and the
                             packing in ops.py handle ell and var, too

Bounds: the project's, unchanged -- gp_routes.BASE, integrator_routes.FLOOR, tangent_ref.bound, 1e-4 for the conditionals
(test_gpu_gp_routes.py, posterior_ref.within), test_gpu_backward.py's 2e-4 / 1e-3 for the layer -- each plus
3 relerr(fp32 oracle, fp64 oracle) of that very case and regime.  No floor has been raised.  Every figure is printed before it is
asserted; the module prints the largest per regime and family when it ends.

The integrator cases also assert the condition itself on the cache the GPU built, all rows: the fp32 oracle within 2e-5 of fp64 for
f, zt and the stage inputs, within 1e-4 for the adjoints and leaf gradients (gp_regimes.integrator_cap, the caps of the host gate), as
gp_routes.check_case does for the cache cases.

Measured on an MI355X, largest relerr to fp64 over the cases of a regime, hip / fp32 oracle on the same inputs:

  regime      build (nu, u, f_prior(Z), Lu, zt)  its backward     f (3 modes)      zt, xstage, adjoints  param_grad, fused  operators       conditional     rhs_jvp
  var_spread  4.8e-6 / 5.5e-6                     3.7e-5 / 6.7e-6  1.0e-6 / 1.9e-6  6.6e-7 / 1.4e-6       1.8e-6 / 1.2e-6    3.3e-7 / 3.9e-7 2.9e-7 / 4.5e-7 5.5e-7 / 4.1e-7
  ell_spread  1.6e-5 / 1.0e-5                     1.1e-5 / 1.2e-5  1.0e-6 / 1.6e-6  1.8e-6 / 1.6e-6       2.0e-6 / 1.4e-6    3.8e-7 / 4.7e-7 3.4e-7 / 4.1e-7 5.7e-7 / 6.5e-7
  short       1.6e-6 / 4.1e-6                     3.0e-6 / 1.9e-6  5.6e-7 / 1.7e-6  4.4e-6 / 1.6e-6       1.7e-6 / 2.1e-6    5.1e-7 / 3.2e-7 4.4e-7 / 2.9e-7 5.2e-7 / 5.9e-7
  long        1.4e-5 / 1.3e-5                     4.8e-5 / 1.3e-5  1.9e-6 / 3.4e-6  9.3e-7 / 1.3e-6       1.4e-6 / 7.4e-7    4.0e-7 / 5.9e-7 4.5e-7 / 6.8e-7 6.3e-7 / 4.8e-7
  ell_linear  6.9e-6 / 4.0e-6                     1.1e-4 / 2.2e-5  1.4e-6 / 2.8e-6  8.8e-7 / 1.4e-6       6.3e-7 / 6.1e-7    3.0e-7 / 4.3e-7 3.7e-7 / 5.8e-7 4.2e-7 / 7.2e-7
  var_linear  5.0e-6 / 8.3e-6                     3.3e-5 / 5.4e-6  1.2e-6 / 2.4e-6  5.4e-6 / 4.3e-6       2.5e-6 / 2.1e-6    3.5e-7 / 3.0e-7 3.5e-7 / 3.6e-7 4.8e-7 / 4.4e-7
  var_small   5.8e-6 / 6.5e-6                     2.2e-5 / 4.6e-6  1.3e-6 / 2.8e-6  7.5e-7 / 9.0e-7       1.6e-6 / 8.7e-7    3.3e-7 / 3.6e-7 4.1e-7 / 6.0e-7 4.8e-7 / 4.5e-7
  far         9.8e-6 / 1.1e-5                     4.5e-6 / 3.3e-6  1.5e-6 / 2.8e-6  1.8e-6 / 1.3e-6       2.5e-6 / 2.2e-6    1.0e-6 / 6.6e-7 3.6e-7 / 3.6e-7 1.3e-6 / 9.7e-7

The layer through autograd: 1.0e-6 / 1.4e-6 (var_spread), 2.4e-6 / 1.9e-6 (ell_spread).  No bound was missed and no floor moved.
The largest fraction of a bound used is 0.18 (the stage adjoints of the DF team case in `short`, 4.4e-6 of 2e-5 + 3 x 1.6e-6), and the
fp32 oracle's largest fraction of a cap on the cache the GPU built is 0.17 (f of the RBF team case in `long`, 3.4e-6 of 2e-5).  f
itself, where the cosine in revolutions takes the fract of an argument in the tens (short, far, ell_linear), is at 5.6e-7 .. 1.5e-6,
below the fp32 oracle's own 1.7e-6 .. 2.8e-6.  The kernels agreed with the oracle in every index of ell and var, and the four copies
of softplus / sigmoid (softplus_lower, softplus_lower_m, softplus_l, sigmoid_raw) agree with each other and with torch on the raw > 20
branch: the sweep found no bug, and no kernel was changed.
The fp32 yardstick of the operator tests is the oracle with its squared distances in difference form (gp_regimes.twin): the expanded
form cancels at |x| = 25 in `far` and put K(x, x) and the conditional variance 3e-5 from fp64, where the kernels are at 1e-6.
The module takes 75 s; its slowest case, DF M = 129, S = 384 at 2049 rows, 4 .. 6 s, nearly all of it the fp64 oracle on the CPU.
"""
import collections

import pytest
import torch

import gp_regimes as G
import gp_routes as R
import integrator_routes as IR
import posterior_ref as PR
import tangent_ref as TR

pytestmark = pytest.mark.gpu
SEEN = collections.defaultdict(set)                  # regime -> tags that ran
DONE = set()                                         # what ran, for the closing test
FIGS = {}                                            # (regime, family) -> (largest hip relerr to fp64, largest fp32-oracle relerr)
COND_FLOOR = 1e-4

CACHE_CASES, INT_CASES = G.cache_cases(), G.integrator_cases()
OP_CASES = [(k, r) for k in ('RBF', 'DF') for r in G.REGIMES]
LAYER_CASES = [s + (r,) for s in G.LAYER_SHAPES for r in G.FIRST]


def _note(regime, family, errs):
    """errs: iterable of (hip, fp32 oracle)"""
    errs = list(errs)
    a, b = FIGS.get((regime, family), (0.0, 0.0))
    FIGS[(regime, family)] = (max([a] + [e for e, _ in errs]), max([b] + [e for _, e in errs]))


@pytest.fixture(scope='module', autouse=True)
def _figures_and_cached_results():
    yield
    fams = sorted({f for _, f in FIGS})
    print('\nlargest relerr to fp64 per regime, hip / fp32 oracle')
    for r in G.REGIMES:
        print('  %-10s %s' % (r, ', '.join('%s %.1e/%.1e' % ((f,) + FIGS[(r, f)]) for f in fams if (r, f) in FIGS)))
    R.reference.cache_clear()
    IR.inputs.cache_clear()


# ---- 1. cache build and its backward ---------------------------------------------------------------------------------------------------
def _cache(mode, c):
    got = R.run_case(c, mode)
    r64, e32, _ = R.reference(c)
    for fam, keys in (('build', R.FWD_KEYS + ('Lu',)), ('build bwd', R.GRAD_KEYS)):
        _note(c.regime, fam, [(G.relerr(got[k], r64[k].reshape(got[k].shape)), e32[k]) for k in keys])
    R.check_case(c, mode, got, SEEN[c.regime])
    DONE.add(('cache', mode, c))


@pytest.mark.parametrize('mode,c', CACHE_CASES, ids=['%s-%s' % (m, R.case_id(c)) for m, c in CACHE_CASES])
def test_cache_build_and_backward(mode, c):
    _cache(mode, c)


# ---- 2. integrator and reverse sweep ---------------------------------------------------------------------------------------------------
def _integrator(c):
    """integrator_routes.check_case; then its figures are kept, and the fp32 oracle is held to the caps of the host gate on the cache
    the GPU built, all rows: the condition under which floor + 3 relerr(fp32 oracle, fp64) is a small multiple of the floor"""
    errs = IR.check_case(c, IR.run_case(c), SEEN[c.regime])
    for fam, keys in (('f', IR.OUT_F), ('rollout', IR.OUT_ROLL), ('param_grad', IR.OUT_LEAF)):
        _note(c.regime, fam, [v for (_, k), v in errs.items() if k in keys])
    ill = {what + k: '%.1e' % e32 for (what, k), (_, e32) in errs.items() if not e32 <= G.integrator_cap(k)}
    assert not ill, ('the inputs are not well conditioned', IR.case_id(c), ill)
    DONE.add(('integrator', c))


@pytest.mark.parametrize('c', INT_CASES, ids=IR.case_id)
def test_integrator_and_reverse_sweep(c):
    _integrator(c)


# ---- 3. the public operators -----------------------------------------------------------------------------------------------------------
def _tag():
    from vae_gp_ode_amd import _lib
    return _lib.load().gpode_last_launch().decode()


def _held(regime, family, what, figs, floor):
    """figs {name: (hip, fp32 oracle)}: printed, noted, then asserted against floor + 3 x the fp32 oracle's own distance"""
    print('%s hip / fp32-oracle relerr to fp64: %s' % (what, ', '.join('%s %.1e/%.1e' % ((n,) + e) for n, e in figs.items())))
    _note(regime, family, figs.values())
    miss = {n: (e, floor + 3 * e32) for n, (e, e32) in figs.items() if not e <= floor + 3 * e32}
    assert not miss, (what, miss)


def _operators(kernel, regime):
    from oracle import gpode_oracle as O
    from vae_gp_ode_amd import ops
    c = G.operator_case(kernel, regime)
    S = c.S
    p, nz, x, _, _ = IR.inputs(c)
    what = IR.case_id(c)
    pd, nd_, xd = {k: v.cuda() for k, v in p.items()}, {k: v.cuda() for k, v in nz.items()}, x.cuda()
    seen, flo = SEEN[regime], IR.FLOOR['f0']
    K_ = O.rbf_K if kernel == 'RBF' else O.df_K
    fu_ = O.rbf_f_update if kernel == 'RBF' else O.df_f_update
    pr_ = O.rbf_rff_forward if kernel == 'RBF' else O.df_rff_forward
    ev = {}
    nu32 = O.build_cache(O.to_dtype(p, torch.float64), O.to_dtype(nz, torch.float64), kernel)['nu'].float()       # ONE nu for both and the GPU
    for dt in (torch.float64, torch.float32):
        q, n_, y = O.to_dtype(p, dt), O.to_dtype(nz, dt), x.to(dt)
        ell, var = O.softplus(q['raw_ell']), O.softplus(q['raw_var'])
        with G.twin(dt):
            cl = O.build_cache(q, n_, kernel)
            ev[dt] = dict(Kxz=K_(y, q['Z'], ell, var), Kxx=K_(y, None, ell, var), f_update=fu_(y, q['Z'], nu32.to(dt), ell, var),
                          omega=cl['omega'], f_prior=pr_(y, cl['omega'], cl['phase'], cl['w'], var, S))
    e64, e32 = ev[torch.float64], ev[torch.float32]
    # kern.K
    got = dict(Kxz=ops.kernel_matrix(kernel, pd['raw_ell'], pd['raw_var'], xd, pd['Z']))
    seen.add(_tag())
    got['Kxx'] = ops.kernel_matrix(kernel, pd['raw_ell'], pd['raw_var'], xd)
    # kern.f_update on the fp64 oracle's nu
    got['f_update'] = ops.f_update(kernel, pd['raw_ell'], pd['raw_var'], xd, pd['Z'], nu32.cuda())
    # kern.build_cache + rff_forward
    kc = ops.kern_cache(kernel, pd['raw_ell'], pd['raw_var'], nd_['rff_w'], nd_['rff_eps'], nd_['rff_u'])
    seen.add(_tag())
    got['omega'], got['f_prior'] = kc.omega, ops.rhs(kc, xd, mode=1)
    seen.add(_tag())
    _held(regime, 'operators', what, {k: (G.relerr(got[k], e64[k]), G.relerr(e32[k], e64[k])) for k in got}, flo)
    # the posterior moments
    if kernel == 'RBF':
        figs = {}
        for full in (False, True):
            mean, var = ops.conditional(pd['raw_ell'], pd['raw_var'], pd['Z'], pd['Um'], pd['Us'], xd, full_cov=full)
            seen.add(_tag())
            m64, v64 = O.build_conditional(O.to_dtype(p, torch.float64), x.double(), full_cov=full)
            with G.twin(torch.float32):
                m32, v32 = O.build_conditional(p, x, full_cov=full)
            figs.update({'mean%d' % full: (G.relerr(mean, m64), G.relerr(m32, m64)), 'var%d' % full: (G.relerr(var, v64), G.relerr(v32, v64))})
        _held(regime, 'conditional', what + ' conditional', figs, COND_FLOOR)
    else:
        r64 = PR.posterior(O.to_dtype(p, torch.float64), x.double())
        with G.twin(torch.float32):
            r32 = PR.posterior(p, x)
        figs = {}
        for cov, key in (('diag', 'diag'), ('point', 'point'), ('full', 'full')):
            mean, var = ops.conditional_df(pd['raw_ell'], pd['raw_var'], pd['Z'], pd['Um'], pd['Us'], xd, cov=cov)
            seen.add(_tag())
            figs.update({'mean/' + cov: (G.relerr(mean, r64['mean']), G.relerr(r32['mean'], r64['mean'])),
                         cov: (G.relerr(var, r64[key]), G.relerr(r32[key], r64[key]))})
        _held(regime, 'conditional', what + ' conditional_df', figs, COND_FLOOR)
    # J_f in the three modes, on the cache the GPU built (tangent_ref)
    k = IR.build(c, (pd, nd_))
    cache = IR.cache_dicts(c, k, (pd, nd_))
    figs = {}
    for mode in (0, 1, 2):
        f, jv = ops.rhs_jvp(k, xd, mode=mode)
        seen.add(_tag())
        assert _tag() == 'rhs_jvp_%s_stream' % kernel.lower()
        J64, J32 = TR.jacobian(cache[0], x, torch.float64, mode), TR.jacobian(cache[0], x, torch.float32, mode)
        f64 = getattr(O, TR.PARTS[mode])(x.double(), TR.in_dtype(cache[0], torch.float64))
        f32 = getattr(O, TR.PARTS[mode])(x, TR.in_dtype(cache[0], torch.float32))
        figs['J%d' % mode] = (G.relerr(jv.transpose(-1, -2), J64), G.relerr(J32, J64))
        figs['f%d' % mode] = (G.relerr(f, f64), G.relerr(f32, f64))
    _held(regime, 'rhs_jvp', what + ' rhs_jvp', figs, TR.FLOOR)
    DONE.add(('operators', kernel, regime))


@pytest.mark.parametrize('kernel,regime', OP_CASES, ids=['%s-%s' % kr for kr in OP_CASES])
def test_public_operators(kernel, regime):
    _operators(kernel, regime)


# ---- 4. the layer, through autograd ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel,Di,Do,order,M,S,regime', LAYER_CASES, ids=['%s-%d-%d-o%d-M%d-S%d-%s' % s for s in LAYER_CASES])
def test_layer_through_autograd(kernel, Di, Do, order, M, S, regime):
    """test_gpu_backward.test_streamed_backward_matches_fp64_oracle's route (SVGP_Layer, Flow, loss.backward()) and bounds"""
    from vae_gp_ode_amd.model.core.flow import Flow
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    p, nz, z0, ts, gw = G.layer_inputs(kernel, Di, Do, order, M, S, regime)
    gp = SVGP_Layer(Di, Do, M, S, kernel=kernel).cuda()
    with torch.no_grad():
        gp.kern.unconstrained_lengthscales.copy_(p['raw_ell'])
        gp.kern.unconstrained_variance.copy_(p['raw_var'])
        gp.inducing_loc.optvar.copy_(p['Z'])
        gp.Um.optvar.copy_(p['Um'])
        gp.Us_sqrt.optvar.copy_(p['Us'])
    flow = Flow(gp, order=order, solver='rk4').cuda()
    gp.set_noise({k: v.cuda() for k, v in nz.items()})
    zg = z0.cuda().requires_grad_(True)
    zt = flow(zg, ts.cuda())
    (zt * gw.cuda()).sum().backward()
    got = {'raw_ell': gp.kern.unconstrained_lengthscales.grad, 'raw_var': gp.kern.unconstrained_variance.grad,
           'Z': gp.inducing_loc.optvar.grad, 'Um': gp.Um.optvar.grad, 'Us': gp.Us_sqrt.optvar.grad, 'z0': zg.grad, 'zt': zt.detach()}
    (r64, _), (r32, _) = (G.oracle(kernel, p, [nz], z0, ts, gw[None], order, 'rk4', dt) for dt in (torch.float64, torch.float32))
    r64['zt'], r32['zt'] = r64['zt'][0], r32['zt'][0]
    figs = {k: (G.relerr(got[k], r64[k]), G.relerr(r32[k], r64[k])) for k in got}
    print('%s-o%d-%s hip / fp32-oracle relerr to fp64: %s' % (kernel, order, regime, ', '.join('%s %.1e/%.1e' % ((n,) + e) for n, e in figs.items())))
    _note(regime, 'layer', figs.values())
    miss = {k: (e, (2e-4 if k == 'zt' else 1e-3) + 3 * e32) for k, (e, e32) in figs.items() if not e < (2e-4 if k == 'zt' else 1e-3) + 3 * e32}
    assert not miss, miss


# ---- 5. what every regime reached ------------------------------------------------------------------------------------------------------
NAMED = {                                            # what the union of tags must cover at least, per regime
    'every': {'cache build: lds', 'cache build: chain32+deep', 'kernel_matrix', 'conditional: chain32', 'conditional_df: chain32',
              'rhs_jvp_rbf_stream', 'rhs_jvp_df_stream', 'rhs_rbf_team', 'rollout_rbf_team', 'rhs_df_team', 'rollout_df_team',
              'rollout_bwd_rbf', 'rollout_bwd_df', 'rhs_vjp_rbf', 'rhs_vjp_df', 'param_grad_rbf', 'param_grad_df_split'} |
    {'%s, %s' % (R.BWD_FAMILY[f], k) for f in ('solves', 'inverse32') for k in ('rbf', 'df')},     # k_Kbwd_rbf and k_Kbwd_df behind either
    'roll': set(IR.REQUIRED_TAGS),                   # every forward evaluator, both reverse families, every param_grad_*, the fused sweep
}


def _table(regime):
    want = {'kernel_matrix', 'kern.build_cache', 'rhs_rbf_team', 'rhs_df_team', 'conditional: chain32', 'conditional_df: chain32',
            'rhs_jvp_rbf_stream', 'rhs_jvp_df_stream'}
    for mode, c in CACHE_CASES:
        if c.regime == regime:
            want.update(R.expected(c, mode).values())
    for c in INT_CASES:
        if c.regime == regime:
            want.update(IR.expected(c).values())
    return want


def test_every_regime_reached_every_reader():
    """The union of gpode_last_launch() per regime equals what the case lists name, and that covers every forward evaluator, both
    reverse families, every param_grad kernel, the LDS and the chain build, both k_Kbwd families, kernel_matrix, conditional: chain32
    and rhs_jvp_* (run after the tests above; on its own it runs the cases it needs)."""
    for regime in G.REGIMES:
        want = _table(regime)
        assert want >= NAMED['every'] and (regime not in G.ROLL or want >= NAMED['roll']), (regime, (NAMED['every'] | NAMED['roll']) - want)
    for mode, c in CACHE_CASES:
        if ('cache', mode, c) not in DONE:
            _cache(mode, c)
    for c in INT_CASES:
        if ('integrator', c) not in DONE:
            _integrator(c)
    for kernel, regime in OP_CASES:
        if ('operators', kernel, regime) not in DONE:
            _operators(kernel, regime)
    for regime in G.REGIMES:
        assert SEEN[regime] == _table(regime), (regime, sorted(SEEN[regime] ^ _table(regime)))
