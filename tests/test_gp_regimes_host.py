"""What tests/test_gpu_gp_regimes.py rests on, checked without a GPU (tests/gp_regimes.py has the regime table and the case lists).

Well-posedness: for every (case, regime) the GPU tests use, the fp64 and the fp32 oracle both factorise and the fp32 oracle is within
2e-5 of fp64 for nu, f_prior(Z), f and the trajectories, within 1e-4 for every parameter gradient and d/dz0.  This is a condition on
the INPUTS: it keeps floor + 3 relerr(fp32 oracle, fp64) within a small multiple of the floor, so that the GPU tests' bound means in
every regime what it means at the initialisation.  The table is fixed; a pair that fails is repaired by its inputs (Z scale, width, M),
never skipped.  (Integrator cases: their first 256 trajectories; the GPU test compares on the cache the GPU built.)

Sensitivity: each mistake in how ell or var is indexed (gp_regimes.mutant), made in the fp64 oracle, moves at least one compared
output by 10 x the GPU tests' bound (gp_routes.BASE + 3 relerr(fp32 oracle, fp64)) in at least one regime -- and the variance mutants
move nothing but d/d raw_var at synthetic_gp's own parameters, which is the gap the regimes close."""
import pytest
import torch

import gp_regimes as G
import gp_routes as R
import integrator_routes as IR

SENS_CASES = {'RBF': R.C('RBF', 6, 6, 40, 1), 'DF': R.C('DF', 6, 6, 16, 1)}


def _gate(kind, item, name):
    errs, piv = G.well_posed(*G.gate_inputs(kind, item))
    print('%s: pivots %.3g .. %.3g; relerr(fp32 oracle, fp64): %s' % (name, piv[0], piv[1], ', '.join('%s %.1e' % kv for kv in errs.items())))
    bad = {k: e for k, e in errs.items() if not e <= (G.FWD_CAP if k in G.FWD_KEYS else G.GRAD_CAP)}
    assert not bad, (name, bad)


def test_the_regime_table():
    assert G.REGIMES == ('var_spread', 'ell_spread', 'short', 'long', 'ell_linear', 'var_linear', 'var_small', 'far')
    from oracle import gpode_oracle as O
    from test_gpu_backward import synthetic_gp
    p0, _, z0, _, _ = synthetic_gp('RBF', 6, 3, 10, 8, 4, 3, seed=1)
    for r in G.REGIMES:
        p, z = G.apply(r, p0, z0, 'RBF')
        t = G.TABLE[r]
        assert set(p) == set(p0) and all(torch.equal(p[k], p0[k]) for k in ('Um', 'Us'))
        assert torch.equal(p['Z'], p0['Z'] * (t.z_scale / 2.0)) and torch.equal(z, z0 * t.x_scale)
        assert (t.ell is None) == torch.equal(p['raw_ell'], p0['raw_ell']) and not torch.equal(p['raw_var'], p0['raw_var'])
        p2, _ = G.apply(r, p0, z0, 'RBF')
        assert all(torch.equal(p[k], p2[k]) for k in p)                                      # seeded
        var = O.softplus(p['raw_var'])
        assert len(set(var.tolist())) == var.numel()                                         # no two dimensions share a variance
    assert (G.apply('ell_linear', p0, z0, 'RBF')[0]['raw_ell'] > 20).all() and (G.apply('var_linear', p0, z0, 'RBF')[0]['raw_var'] > 20).all()
    e = O.softplus(G.apply('ell_spread', p0, z0, 'RBF')[0]['raw_ell'])
    assert e.min() >= 1 and e.max() <= 4.001 and e.max() / e.min() > 2
    assert G.apply('base', p0, z0, 'DF') == (p0, z0)
    ts = torch.tensor(IR.TS[3])
    assert all(G.times(r, ts) is ts for r in ('base',) + G.REGIMES if r != 'short') and torch.equal(G.times('short', ts), 0.25 * ts)
    assert torch.equal(IR.inputs(IR.CASES[0]._replace(N=5, regime='short'))[3], 0.25 * ts) and torch.equal(IR.inputs(IR.CASES[0]._replace(N=5))[3], ts)
    # the trailing field: absent, a case is what it was
    assert R.C('RBF', 6, 6, 40, 1) == R.C('RBF', 6, 6, 40, 1, 'base') and R.case_id(R.C('RBF', 6, 6, 40, 1)) == 'RBF-6-6-M40-L1'
    assert R.case_id(R.C('RBF', 6, 6, 40, 1, 'far')) == 'RBF-6-6-M40-L1-far'
    c = IR.CASES[0]
    assert c.regime == 'base' and IR.case_id(c._replace(regime='short')) == IR.case_id(c) + '-short'


def test_the_case_lists():
    cc, ic = G.cache_cases(), G.integrator_cases()
    assert len(set(cc)) == len(cc) == 4 * 8 + 4 * 2 and len(set(ic)) == len(ic) == 12 * 4 + 2 * 4
    for r in G.ROLL:
        routes = {IR.forward_route(c) for c in ic if c.regime == r}
        assert routes == set(IR._F), (r, routes)
        tags = set()
        for c in ic:
            if c.regime == r:
                tags.update(IR.expected(c).values())
        assert tags == set(IR.REQUIRED_TAGS), (r, tags ^ set(IR.REQUIRED_TAGS))
    for r in G.REGIMES:
        assert {IR.forward_route(c) for c in ic if c.regime == r} >= {'rbf_team', 'df_team'}
        fwd = {R.expected(c, m)['fwd'] for m, c in cc if c.regime == r}
        assert fwd >= {'cache build: lds', 'cache build: chain32+deep'}, (r, fwd)
    # DF at width 3 does not factorise in fp32 in four of the regimes: every DF case here is 6 wide or more
    assert all(c.Do >= 6 for _, c in cc if c.kernel == 'DF') and all(c.Do >= 6 for c in ic if c.kernel == 'DF')


@pytest.mark.parametrize('mode,c', G.cache_cases(), ids=['%s-%s' % (m, R.case_id(c)) for m, c in G.cache_cases()])
def test_cache_cases_are_well_posed(mode, c):
    _gate('cache', c, R.case_id(c))


@pytest.mark.parametrize('c', G.integrator_cases(), ids=IR.case_id)
def test_integrator_cases_are_well_posed(c):
    _gate('integrator', c, IR.case_id(c))


@pytest.mark.parametrize('c', G.integrator_cases(), ids=IR.case_id)
def test_integrator_cases_are_well_posed_in_what_the_gpu_test_compares(c):
    """integrator_routes.reference on the oracle's own cache, first GATE_ROWS = 256 trajectories: f, zt and the stage inputs within 2e-5, the
    adjoints and the leaf gradients within 1e-4 (the GPU test holds the same caps on the cache the GPU built, all rows)"""
    p, nz, z0, ts, gw = IR.inputs(c)
    n, cache = G.GATE_ROWS, IR.host_cache(c)
    r64, r32 = (IR.reference(c, cache, dt, z0[:n], ts, gw[:, :n]) for dt in (torch.float64, torch.float32))
    errs = {k: IR.relerr(r32[k], r64[k]) for k in r64}
    print('%s relerr(fp32 oracle, fp64): %s' % (IR.case_id(c), ', '.join('%s %.1e' % kv for kv in errs.items())))
    bad = {k: e for k, e in errs.items() if not e <= G.integrator_cap(k)}
    assert not bad, (IR.case_id(c), bad)


@pytest.mark.parametrize('regime', G.REGIMES)
@pytest.mark.parametrize('kernel', ['RBF', 'DF'])
def test_operator_cases_are_well_posed(kernel, regime):
    c = G.operator_case(kernel, regime)
    _gate('integrator', c, IR.case_id(c))


@pytest.mark.parametrize('regime', G.REGIMES)
@pytest.mark.parametrize('shape', G.LAYER_SHAPES, ids=['%s-%d-%d-o%d-M%d-S%d' % s for s in G.LAYER_SHAPES])
def test_layer_shapes_are_well_posed(shape, regime):
    """the layer test runs var_spread and ell_spread on the GPU; its shapes are held in all eight here"""
    _gate('layer', shape + (regime,), '%s-%d-%d-o%d-M%d-S%d-%s' % (shape + (regime,)))


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------------
_REF = {}


def _ref(kernel, regime):
    c = SENS_CASES[kernel]._replace(regime=regime)
    if c not in _REF:
        r64, e32, _ = R.reference(c)
        _REF[c] = (r64, {k: R.BASE[k] + 3 * e32[k] for k in R.FWD_KEYS + R.GRAD_KEYS})
    return (c,) + _REF[c]


def _moved(name, regime):
    """{key: (how far the mutant moves it, the GPU tests' bound for it)}"""
    c, r64, bound = _ref(G.mutant_kernel(name), regime)
    with G.mutant(name):
        m64 = R._oracle(c, torch.float64)
    return {k: (G.relerr(m64[k], r64[k]), bound[k]) for k in bound}


@pytest.mark.parametrize('name', G.mutant_names())
def test_every_mutant_is_far_past_the_bound_in_some_regime(name):
    best = (0.0, None, None)
    for regime in G.REGIMES:
        moved = _moved(name, regime)
        print('%-60s %-10s %s' % (name, regime, ', '.join('%s %.0e/%.0e' % ((k,) + v) for k, v in moved.items())))
        for k, (d, b) in moved.items():
            if k == 'raw_var' and name in G.VAR_MUTANTS:         # moves at the base parameters already: the regimes add nothing there
                continue
            best = max(best, (d / b, regime, k), key=lambda t: t[0])
    print('%s: largest (movement / bound) %.1f, %s in %s' % ((name, best[0], best[2], best[1])))
    assert best[0] >= 10, (name, best)


@pytest.mark.parametrize('name', G.VAR_MUTANTS)
def test_variance_mutants_are_invisible_at_the_base_parameters(name):
    """var = 1 in every dimension: reading another dimension's variance changes d/d raw_var (the gradient lands in another slot) and
    nothing else.  This is the gap: no test before the regimes could tell these kernels from the right ones."""
    moved = _moved(name, 'base')
    print(name, {k: '%.1e' % v[0] for k, v in moved.items()})
    assert all(d <= 1e-12 for k, (d, _) in moved.items() if k != 'raw_var'), moved
    assert moved['raw_var'][0] > 1e-3, moved


def test_mutants_leave_the_oracle_as_it_was():
    from oracle import gpode_oracle as O
    before = {k: getattr(O, k) for k in ('df_K', 'rbf_K', 'rbf_rff_forward', 'rff_omega', 'df_compute_nu')}
    for name in G.mutant_names():
        with G.mutant(name):
            assert any(getattr(O, k) is not v for k, v in before.items())
        assert all(getattr(O, k) is v for k, v in before.items())
