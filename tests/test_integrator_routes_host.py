"""What tests/integrator_routes.py rests on, checked without a GPU.

Routes: expected() names, for every case, the evaluator the case table was written for; every required tag has a case; every threshold
of the dispatch has a case on each side; the byte and register counts the table quotes come out of the restated layout.
Reference pinned: reference() fed an oracle-built cache reproduces the reference's own trajectories and dL/dz0 (tests/golden) to the
standard tests/test_oracle_golden.py holds the oracle to.
Sensitivity: for every case, four deliberately wrong references -- the last Fourier feature dropped, the last inducing point dropped,
classical RK4 in place of the 3/8 rule, a uniform time grid of the same span -- differ from the true one by at least 10 x the bound
the GPU test applies, in every output the fault can reach (SEEN_IN).  That is what shows that a ragged lane or the per-step dt is
visible through the tolerance.  It is evaluated on the first ROWS trajectories of the case: the rows are independent draws of one
distribution, and neither fault depends on how many there are."""
import pytest
import torch

import integrator_routes as IR
from conftest import load_golden, sub
from oracle import gpode_oracle as O

ROWS = 48


# ---- routes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', IR.CASES, ids=IR.case_id)
def test_expected_names_the_route_of_the_table(c):
    want = IR.expected(c)
    assert want['rhs'] == 'rhs_' + IR.TABLE[c]
    if c.kind != 'prior':
        assert want['rollout'] == 'rollout_' + IR.TABLE[c]


def test_every_required_tag_has_a_case():
    tags = set()
    for c in IR.CASES:
        tags.update(IR.expected(c).values())
    for c in IR.ACC_CASES:
        tags.add(IR.param_grad_route(c, c.N))
    assert tags == set(IR.REQUIRED_TAGS), (tags ^ set(IR.REQUIRED_TAGS))


def test_quoted_byte_and_register_counts():
    for c, b in IR.BYTES.items():
        assert IR.pack_bytes(c) == b, (IR.case_id(c), IR.pack_bytes(c), b)
    for (c, SJ, MJ), n in IR.REG_FLOATS.items():
        assert IR.rbf_reg_floats(c, SJ, MJ) == n, (IR.case_id(c), IR.rbf_reg_floats(c, SJ, MJ), n)
    assert IR.LDS_LIMIT == 153600
    assert IR.rows(IR.D_(6, 100, 256, 2049, 'rk4', T=2)) == 8196 >= 1024      # param_grad_df_split


def _find(**kw):
    hit = [c for c in IR.CASES if all(getattr(c, k) == v for k, v in kw.items())]
    assert hit, kw
    return hit[0]


THRESHOLDS = [    # (what, the case below, the case above, the tag that must differ)
    ('S = 256 | 257', dict(kernel='RBF', M=128, S=256, N=2048), dict(kernel='RBF', M=128, S=257, N=5), 'rollout_bwd'),
    ('M = 128 | 129', dict(kernel='RBF', M=128, S=256, N=2048), dict(kernel='RBF', M=129, S=256, N=5), 'rollout_bwd'),
    ('N = 2048 | 2049, RBF', dict(kernel='RBF', M=128, S=256, N=2048), dict(kernel='RBF', M=128, S=256, N=2049), 'rollout'),
    ('N = 2048 | 2049, DF', dict(kernel='DF', Do=6, M=100, S=256, N=2048), dict(kernel='DF', Do=6, M=100, S=256, N=2049, nd=1), 'rollout'),
    ('MJ = 2 | 1 at SJ = 4', dict(kernel='RBF', Do=6, M=65, S=193, N=2049), dict(kernel='RBF', Do=6, M=64, S=256, N=2049), 'rollout'),
    ('SJ = 4 | 2 at the wave kernels', dict(kernel='RBF', Do=6, M=100, S=256, N=8197), dict(kernel='RBF', Do=6, M=64, S=128, N=8197), 'rollout'),
    ('SJ = 1 | 2 at MJ = 1', dict(kernel='RBF', Do=6, M=64, S=64, N=2049), dict(kernel='RBF', Do=6, M=64, S=65, N=2049), 'rollout'),
    ('260 floats, reg42', dict(kernel='RBF', Do=6, M=128, S=256, N=2049), dict(kernel='RBF', Do=8, M=100, S=256, N=2049), 'rollout'),
    ('260 floats, reg11', dict(kernel='RBF', Di=16, Do=8, N=2049), dict(kernel='RBF', Di=16, Do=16, N=2049), 'rollout'),
    ('the LDS byte limit', dict(kernel='DF', Do=6, M=128, S=384, N=2049), dict(kernel='DF', Do=6, M=129, S=384, N=2049), 'rollout'),
    ('the LDS byte limit by the width', dict(kernel='DF', Do=15, N=2049), dict(kernel='DF', Do=16, N=2049), 'rollout'),
    ('R = 1023 | 1024', dict(kernel='DF', N=1023), dict(kernel='DF', N=1024), 'param_grad'),
    ('forward Do <= 16, backward Do <= 8', dict(kernel='RBF', Do=8, M=40, N=2049), dict(kernel='RBF', Do=16, M=40, N=5), 'rollout_bwd'),
]


@pytest.mark.parametrize('what,lo,hi,key', THRESHOLDS, ids=[t[0] for t in THRESHOLDS])
def test_every_threshold_has_a_case_on_each_side(what, lo, hi, key):
    a, b = IR.expected(_find(**lo)), IR.expected(_find(**hi))
    assert a[key] != b[key], (what, a, b)


def test_width_sixteen_keeps_the_forward_register_team():
    c = _find(kernel='RBF', Do=16, N=5)
    assert IR.expected(c)['rollout'] == 'rollout_rbf_team' and IR.expected(c)['rollout_bwd'] == 'rollout_bwd_rbf_stream'
    c = _find(kernel='DF', Do=16)
    assert IR.pack_bytes(c._replace(M=1, S=1)) > IR.LDS_LIMIT                      # no LDS route at any size


# ---- the reference, pinned -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel,order', [('gp_rbf1_tiny', 'RBF', 1), ('gp_rbf2_tiny', 'RBF', 2), ('gp_df1_tiny', 'DF', 1)])
@pytest.mark.parametrize('method', ['euler', 'rk4'])
def test_reference_reproduces_the_golden_trajectories_and_dz0(name, kernel, order, method):
    g = load_golden(name)
    p = O.gp_params_from_state_dict(sub(g, 'sd.'))
    cd = O.build_cache(p, sub(g, 'noise.'), kernel)
    Do, Di = p['raw_ell'].shape
    N, T = g['z0'].shape[0], g['ts'].shape[0]
    c = IR.Case(kernel, Di, Do, order, p['Z'].shape[0], cd['S'], N, T, method, 1, 'full')
    r = IR.reference(c, [cd], torch.float32, z0=g['z0'], ts=g['ts'], gw=g['gw'])
    assert torch.equal(r['zt'][0], O.flow_forward(g['z0'], g['ts'], cd, order, method))      # the oracle's own composition, to the bit
    for what, a, b, rtol, atol in (('zt', r['zt'][0], g['zt_' + method], 2e-5, 0), ('d z0', r['gz0'][0], g['grad_%s.z0' % method], 1e-4, 1e-6)):
        err, scale = (a - b).abs().max().item(), b.abs().max().item()                          # test_oracle_golden._close
        assert err <= atol + rtol * scale, (what, err, scale)
    assert torch.equal(r['xstage'][0][:, 0, 0], g['z0'])


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------------
def classical_rk4(f, y0, ts, method):
    """odeint_fixed with the classical Runge-Kutta step (nodes 0, 1/2, 1/2, 1; weights 1/6, 1/3, 1/3, 1/6) where rk4 means the 3/8 rule"""
    assert method == 'rk4'
    ys, y = [y0], y0
    for j in range(len(ts) - 1):
        dt = ts[j + 1] - ts[j]
        k1 = f(y)
        k2 = f(y + 0.5 * dt * k1)
        k3 = f(y + 0.5 * dt * k2)
        k4 = f(y + dt * k3)
        y = y + dt * (k1 + 2 * (k2 + k3) + k4) / 6
        ys.append(y)
    return torch.stack(ys, 0)


def without_last_feature(c, cd):
    w = cd['w'].clone()
    w[c.S - 1] = 0
    if c.kernel == 'DF':
        w[2 * c.S - 1] = 0
    return dict(cd, w=w)


def without_last_inducing_point(c, cd):
    nu = cd['nu'].clone()
    if c.kernel == 'RBF':
        nu[:, c.M - 1] = 0
    else:
        nu[(c.M - 1) * c.Do:] = 0
    return dict(cd, nu=nu)


# the outputs each fault reaches at first order.  (Classical RK4 and the 3/8 rule are both of fourth order: their trajectories differ by
# O(dt^5), below any fp32 bound at these steps, so that fault is looked for where it is of first order -- the stage inputs the forward
# records and the stage adjoints the sweep returns.)
SEEN_IN = {'feature': ('f0', 'f1', 'zt', 'xstage', 'gz0', 'astage', 'omega', 'var'), 'inducing': ('f0', 'f2', 'zt', 'xstage', 'gz0', 'astage', 'Z'),
           'rk4': ('xstage', 'astage'), 'ts': ('zt', 'xstage', 'gz0', 'astage')}
SENS_CASES = [c for c in IR.CASES if c.kind != 'fused']


@pytest.mark.parametrize('c', SENS_CASES, ids=IR.case_id)
def test_a_wrong_reference_is_seen_through_the_bound(c):
    full, c = c, c._replace(N=min(c.N, ROWS))
    cache = IR.host_cache(c)
    r64, r32 = IR.reference(c, cache, torch.float64), IR.reference(c, cache, torch.float32)
    bound = {k: IR.bound(k, IR.relerr(r32[k], r64[k])) for k in r64}
    wrong = {'feature': lambda: IR.reference(c, [without_last_feature(c, cd) for cd in cache], torch.float64)}
    if c.kind != 'prior':
        wrong['inducing'] = lambda: IR.reference(c, [without_last_inducing_point(c, cd) for cd in cache], torch.float64)
        if c.method == 'rk4':
            wrong['rk4'] = lambda: IR.reference(c, cache, torch.float64, integrate=classical_rk4)
        if c.T > 2:                                      # one step has no second dt to confuse it with
            wrong['ts'] = lambda: IR.reference(c, cache, torch.float64, ts=torch.linspace(IR.TS[c.T][0], IR.TS[c.T][-1], c.T, dtype=torch.float64))
    bad = {}
    for what, run in wrong.items():
        r = run()
        for k in SEEN_IN[what]:
            if k in ('xstage', 'astage') and IR.rows(c) == c.N:      # one Euler step: the only stage input is z0, its adjoint dt gw
                continue
            if k in r64:
                d = IR.relerr(r[k], r64[k])
                print('%s %s %s: differs by %.1e, bound %.1e' % (IR.case_id(full), what, k, d, bound[k]))
                if not d >= 10 * bound[k]:
                    bad[(what, k)] = (d, bound[k])
    assert not bad, (IR.case_id(full), bad)
