"""Every route of the GP cache build, its backward, kern.compute_nu and build_conditional (csrc/gp_cache.hip, csrc/gp_cache_bwd.hip),
driven through the C ABI (gpode_cache_sizes_n, gpode_cache_build_fwd_n, gpode_cache_bwd_sizes_n, gpode_cache_bwd_prepare_n,
gpode_cache_build_bwd_n) at the smallest shapes that sit on each edge of the dispatch (gp_routes.CASES), N = 4 trajectories, T = 3,
euler, S = 32.  Six modes:

  default       no switch
  never         ops.set_backward_solves('never'), the runtime form of GPODE_BWD_EXPLICIT_INVERSE=1: the explicit inverse behind k_draw_lds
  always        ops.set_backward_solves('always'), what main.py --backward_solves adaptive selects: k_trsm_slab up to np = 1216
  draw_chain    GPODE_DRAW_CHAIN=1            \\  read once per process: all cases of the mode in ONE fresh child process
  small_factor  GPODE_SMALL_FACTOR_KERNELS=1   >  (gp_routes.child), which saves its outputs to a file
  env_solves    GPODE_BWD_SOLVES=1            /

Per case (gp_routes.run_case / check_case): (a) gpode_last_launch() after build, prepare and backward equals the route the table
gp_routes.expected names -- a restatement of the thresholds that never asks the library; (b) nu, u, f_prior(Z) and the trajectories
within 2e-4 + 3 relerr(fp32 oracle, fp64) of the fp64 oracle, Lu within 1e-4 + 3 ..., the five parameter gradients and d/dz0 of a loss
summed over the draws within 1e-3 + 3 ...; (c) the inputs are well conditioned: the fp32 oracle itself is within 1e-4 of fp64 on
every compared quantity; (d) a second run is bit-identical; (e) prepared = the workspace of cache_bwd_prepare gives the bits of the
unprepared call, add_to of a random (gUm, gUs) gives that tensor plus the plain result to 1e-6 of its largest entry;
(f) check_factorisation() passes; (g) pivot_range() equals min / max of the diagonal of the fp64 factor to the Lu bound.  pack, both
workspaces and every output are NaN-filled; the workspaces are exactly as long as the size queries say, with 4096 NaN guard floats
behind them that must come back untouched.

kern.compute_nu on the oracle's K_uu past the fixture sizes (all three routes; an indefinite 1024-row matrix on the panelled route sets
the status bit) and SVGP_Layer.build_conditional with 892 / 893 / 1100 query points (the last 32-tile size, the first panelled one,
np = 1280) follow.  The last test requires the union of the tags seen to equal gp_routes.REQUIRED_TAGS.

Two batched builds that differ in the number of draws alone can take different forward routes (RBF-16-8-M190 with one draw is
LDS-resident, with two it is 768 B over the limit and takes the chain): both are held to the oracle here, not to each other.

Measured on an MI355X, largest relerr against fp64 per route over all cases and modes (the fp32 oracle on the same inputs: at most 3e-5):
cache build -- lds 9.3e-6, chain32+deep 1.4e-5, chain32+back<1> 1.3e-5, <2> 1.0e-6, <0> 1.4e-6, panel 8.7e-6 (nu in every case; Lu at most
2.0e-6); cache backward -- solves 2.3e-5 (rbf) / 2.8e-6 (df), inverse32 2.5e-5 / 2.2e-6, inverse_mfma 2.1e-5 / 6.4e-7 (d/d variance or
d/dZ); kern.compute_nu -- chain32+deep 4.9e-6, chain32+back<0> 3.4e-6, panel 7.3e-6; build_conditional -- 2.1e-7 (mean), 8.8e-8
(variance, covariance) on both routes, where the fp32 oracle is at 7.7e-6 and 6.1e-5.  add_to: at most 2.7e-7 of the plain result's
largest entry.  No route came near its bound and no NaN of the fills reached an output; the whole module takes 18 s,
the 2176-row case included."""
import pytest
import torch

import gp_routes as R
from oracle import gpode_oracle as O
from test_gpu_forward import relerr

pytestmark = pytest.mark.gpu
SEEN = set()                                        # tags that ran, over all modes
_COND = {}
MAXIMA = {}                                         # tag -> largest relerr against fp64 of the quantities behind that route


@pytest.fixture(scope='module', autouse=True)
def _drop_cached_results():
    yield
    print('largest relerr against fp64 per route:', {k: '%.1e' % v for k, v in sorted(MAXIMA.items())})
    R.child.cache_clear()
    R.reference.cache_clear()
    R.nu_inputs.cache_clear()
    _COND.clear()


def _param(mode):
    cases = R.CASES[mode]
    assert len(set(cases)) == len(cases)
    return pytest.mark.parametrize('c', cases, ids=[R.case_id(c) for c in cases])


@pytest.mark.parametrize('mode,c', [(m, c) for m in ('default', 'never', 'always') for c in R.CASES[m]],
                         ids=['%s-%s' % (m, R.case_id(c)) for m in ('default', 'never', 'always') for c in R.CASES[m]])
def test_in_process_modes(mode, c):
    R.check_case(c, mode, R.run_case(c, mode), SEEN, MAXIMA)


@_param('draw_chain')
def test_draw_chain_switch(c):
    """GPODE_DRAW_CHAIN=1: the systems that fit the LDS-resident draw on the launch chain, with the same results"""
    R.check_case(c, 'draw_chain', R.child('draw_chain')[tuple(c)], SEEN, MAXIMA)


@_param('small_factor')
def test_small_factor_kernels_switch(c):
    """GPODE_SMALL_FACTOR_KERNELS=1: factors past 1024 rows on the 32-tile kernels -- k_solve_back<1>, <2>, <0>, k_linv_dc, k_gemm_phiX,
    k_gemm_S at sizes where the panelled / matrix-core route is the default"""
    R.check_case(c, 'small_factor', R.child('small_factor')[tuple(c)], SEEN, MAXIMA)


def test_backward_solves_from_the_environment():
    """GPODE_BWD_SOLVES=1 is set_backward_solves('always') at start-up: configs[1]'s system at L = 5, bit for bit the runtime form"""
    c = R.CASES['env_solves'][0]
    got = R.child('env_solves')[tuple(c)]
    R.check_case(c, 'env_solves', got, SEEN, MAXIMA)
    here = R.run_case(c, 'always')
    differs = [k for k in got if not (torch.equal(got[k], here[k]) if torch.is_tensor(got[k]) else got[k] == here[k])]
    assert not differs, differs


@pytest.mark.parametrize('mode', ['default', 'small_factor'])
@pytest.mark.parametrize('c', R.NU_CASES, ids=[R.case_id(c) for c in R.NU_CASES])
def test_compute_nu_routes(c, mode):
    got = R.run_nu(c) if mode == 'default' else R.child('small_factor')[('nu',) + tuple(c)]
    R.check_nu(c, mode, got, SEEN, MAXIMA)


def test_compute_nu_reports_an_indefinite_matrix_on_the_panelled_route():
    """test_compute_nu_reports_a_matrix_that_is_not_positive_definite on a 1024-row system (two batched 1000-row matrices, np = 1024):
    one negative pivot in the sixth panel of the second matrix sets the status bit, the identity does not."""
    import ctypes
    from vae_gp_ode_amd import _lib, ops
    M, D = 1000, 2
    assert R.expected_nu(R.Case('RBF', D, D, M, 1), 'default') == 'kern.compute_nu: panel'
    for bad in (False, True):
        Ku = torch.eye(M).expand(D, M, M).contiguous()
        if bad:
            Ku[1, 700, 700] = -1.0
        nu, ws = ops.compute_nu('RBF', D, D, Ku.cuda(), torch.zeros(M, D).cuda(), torch.ones(M, D).cuda())
        assert _lib.load().gpode_last_launch().decode() == 'kern.compute_nu: panel'
        info = ctypes.c_int(0)
        _lib.call('gpode_cache_info', ops._ptr(ws), ctypes.byref(info), ops._stream())
        assert bool(info.value & 1) == bad, (bad, info.value)


def _conditional_layer():
    """SVGP_Layer(6, 3, 100, 32) perturbed as in test_build_conditional_many_queries_and_errors, and 1100 query points"""
    if not _COND:
        from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
        torch.manual_seed(5)
        gp = SVGP_Layer(6, 3, 100, 32, kernel='RBF').cuda()
        with torch.no_grad():
            gp.Um.optvar.add_(0.2 * torch.randn_like(gp.Um.optvar))
            gp.Us_sqrt.optvar.add_(0.05 * torch.randn_like(gp.Us_sqrt.optvar))
        p = dict(raw_ell=gp.kern.unconstrained_lengthscales, raw_var=gp.kern.unconstrained_variance, Z=gp.inducing_loc.optvar,
                 Um=gp.Um.optvar, Us=gp.Us_sqrt.optvar)
        _COND.update(gp=gp, p32={k: v.detach().cpu() for k, v in p.items()}, x=torch.randn(max(R.COND_N), 6))
    return _COND['gp'], _COND['p32'], _COND['x']


@pytest.mark.parametrize('Nq', R.COND_N)
def test_build_conditional_past_the_32_tile_sizes(Nq):
    """build_conditional does not chunk its queries: all Nq rows K(x, Z) are appended to K_uu, each with a 1e30 diagonal, and from
    M + Nq = 993 the factorisation takes the panelled kernels with hundreds of appended rows that span several panels.  Mean and
    marginal variance at all three sizes, the full covariance at 892 and 893, against the fp64 oracle (1e-4 + 3 relerr(fp32 oracle,
    fp64), the bound of test_build_conditional_many_queries_and_errors)."""
    from vae_gp_ode_amd import _lib
    gp, p32, x = _conditional_layer()
    x = x[:Nq]
    want = R.expected_conditional(100, Nq)
    assert want == ('conditional: chain32' if Nq == 892 else 'conditional: panel')
    for full_cov in ((False, True) if Nq < 1000 else (False,)):
        mean, var = gp.build_conditional(x.cuda(), full_cov=full_cov)
        tag = _lib.load().gpode_last_launch().decode()
        SEEN.add(tag)
        m64, v64 = O.build_conditional(O.to_dtype(p32, torch.float64), x.double(), full_cov=full_cov)
        m32, v32 = O.build_conditional(p32, x, full_cov=full_cov)
        em, ev, em32, ev32 = relerr(mean, m64), relerr(var, v64), relerr(m32, m64), relerr(v32, v64)
        print('N = %d full_cov %d [%s]: mean %.1e/%.1e, var %.1e/%.1e (hip / fp32 oracle to fp64)' % (Nq, full_cov, tag, em, em32, ev, ev32))
        MAXIMA[tag] = max(MAXIMA.get(tag, 0.0), em, ev)
        assert tag == want, (tag, want)
        assert em < 1e-4 + 3 * em32 and ev < 1e-4 + 3 * ev32, (em, em32, ev, ev32)
        d = var if not full_cov else torch.diagonal(var, dim1=0, dim2=1)
        assert (d > 0).all()


def test_every_route_was_reached():
    """The union of gpode_last_launch() over all modes equals the list of routes (run after the tests above; on its own it runs the
    cases it needs)."""
    table = set()
    for mode, cases in R.CASES.items():
        for c in cases:
            table.update(R.expected(c, mode).values())
    table.update(R.expected_nu(c, m) for c in R.NU_CASES for m in ('default', 'small_factor'))
    table.update(R.expected_conditional(100, n) for n in R.COND_N)
    assert table == set(R.REQUIRED_TAGS), sorted(table ^ set(R.REQUIRED_TAGS))
    if not set(R.REQUIRED_TAGS) <= SEEN:
        from vae_gp_ode_amd import _lib
        for mode, cases in R.CASES.items():
            for c in cases:
                if set(R.expected(c, mode).values()) <= SEEN:
                    continue
                got = R.child(mode)[tuple(c)] if mode in R.CHILD_ENV else R.run_case(c, mode)
                assert not isinstance(got, str), got
                SEEN.update((got['tag_fwd'], got['tag_prepare'], got['tag_bwd']))
        for c in R.NU_CASES:
            for mode in ('default', 'small_factor'):
                if R.expected_nu(c, mode) not in SEEN:
                    got = R.run_nu(c) if mode == 'default' else R.child(mode)[('nu',) + tuple(c)]
                    assert not isinstance(got, str), got
                    SEEN.add(got[1])
        gp, _, x = _conditional_layer()
        for n in R.COND_N:
            if R.expected_conditional(100, n) not in SEEN:
                gp.build_conditional(x[:n].cuda())
                SEEN.add(_lib.load().gpode_last_launch().decode())
    assert SEEN == set(R.REQUIRED_TAGS), sorted(SEEN ^ set(R.REQUIRED_TAGS))
