"""GPU: posterior moments of the GP vector field -- gpode_conditional_df (csrc/gp_cache.hip), ops.conditional_df,
SVGP_Layer.posterior / mean_noise and evaluate's --eval_field -- against tests/posterior_ref.py, the definition in plain torch on
the oracle's df_K, in float64.

Bound (the form test_gpu_forward.py uses for build_conditional): relerr(got, ref64) < 1e-4 + 3 relerr(ref32, ref64), norm-wise, for
the mean, the marginals, the point blocks and the full covariance separately; ref32 is the same definition in float32.  Bitwise
claims (the workspace, RBF q_diag=False against build_conditional) have no tolerance."""
import ctypes
import glob
import json
import os
import subprocess
import sys

import pytest
import torch

import posterior_ref as R
from conftest import ROOT
from oracle import gpode_oracle as O

pytestmark = pytest.mark.gpu

KEYS = ('raw_ell', 'raw_var', 'Z', 'Um', 'Us')
MODES = ('diag', 'point', 'full')
# (M, D, N, spread of Z, expected route).  M D + N D system rows go to whole 32-tiles, from 32 tiles on to whole 128-panels, and a
# factor of np >= 1024 rows with np % 128 == 0 takes the panel route (big_factor, csrc/gp_launch.hpp): at M = 100, D = 6 that is
# N <= 65 (990 rows, np = 992) chain32, N >= 66 (996 rows, np = 1024) panel; N = 71 (1026 rows) is the first np = 1152.
CASES = [(8, 3, 6, 1.5, 'chain32'), (8, 2, 9, 8.0, 'chain32'), (12, 16, 5, 1.5, 'chain32'), (100, 6, 65, 1.5, 'chain32'),
         (100, 6, 66, 1.5, 'panel'), (100, 6, 71, 1.5, 'panel')]
_REF = {}


@pytest.fixture(autouse=True)
def _global_generators_left_as_found():
    """Layers draw their initial values from the global numpy generator, _rbf_layer seeds torch's, and evaluate.main() seeds all of
    them (seed_everything): later tests of the suite that initialise modules from the global generators see the state they always saw."""
    import random
    import numpy as np
    state = (torch.get_rng_state(), torch.cuda.get_rng_state_all(), np.random.get_state(), random.getstate(), os.environ.get('PYTHONHASHSEED'))
    yield
    torch.set_rng_state(state[0])
    torch.cuda.set_rng_state_all(state[1])
    np.random.set_state(state[2])
    random.setstate(state[3])
    if state[4] is None:
        os.environ.pop('PYTHONHASHSEED', None)
    else:
        os.environ['PYTHONHASHSEED'] = state[4]


def case(M, D, N, spread=1.5, **kw):
    """(p, x, ref64, ref32) of a case, computed once and shared"""
    key = (M, D, N, spread, tuple(sorted(kw.items())))
    if key not in _REF:
        p, x = R.inputs(M, D, N, seed=M * 100 + D, z_spread=spread, **kw)
        _REF[key] = (p, x) + R.references(p, x)
    return _REF[key]


def on_gpu(p, x, cov, **kw):
    from vae_gp_ode_amd import ops
    return ops.conditional_df(*[p[k].cuda() for k in KEYS], x.cuda(), cov=cov, **kw)


def last_launch():
    from vae_gp_ode_amd import _lib
    return _lib.load().gpode_last_launch().decode()


def df_layer(p, S=16, q_diag=False):
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    M, D = p['Um'].shape
    gp = SVGP_Layer(D, D, M, S, q_diag=q_diag, kernel='DF').cuda()
    with torch.no_grad():
        gp.kern.unconstrained_lengthscales.copy_(p['raw_ell'])
        gp.kern.unconstrained_variance.copy_(p['raw_var'])
        gp.inducing_loc.optvar.copy_(p['Z'])
        gp.Um.optvar.copy_(p['Um'])
        gp.Us_sqrt.optvar.copy_(p['Us'])
    return gp


# ---- 1. shapes and routes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,D,N,spread,route', CASES)
def test_every_mode_matches_the_definition(M, D, N, spread, route):
    p, x, r64, r32 = case(M, D, N, spread)
    assert (r64['diag'] > 0).all()
    for cov in MODES:
        mean, var = on_gpu(p, x, cov)
        assert last_launch() == 'conditional_df: ' + route
        assert mean.shape == (N, D) and var.shape == r64[cov].shape
        R.within(mean, r64, r32, 'mean')
        R.within(var, r64, r32, cov)
    assert (on_gpu(p, x, 'diag')[1] > 0).all()


# ---- 2. K(Z,x), not K(x,Z)^T -------------------------------------------------------------------------------------------------------
def test_the_fill_is_not_the_transposed_one():
    p, x, r64, r32 = case(8, 3, 6)
    t64, t32 = R.references(p, x, transposed_fill=True)
    mean, full = on_gpu(p, x, 'full')
    for got, what in ((mean, 'mean'), (full, 'full')):
        R.within(got, r64, r32, what)
        e, tw = R.relerr(got, t64[what]), R.relerr(t32[what], t64[what])
        print('%s against the K(x,Z)^T variant: %.3e (its bound %.3e)' % (what, e, 1e-4 + 3 * tw))
        assert e > 1e-4 + 3 * tw


# ---- 3. the zero-noise draw is the mean; the identity scale is the prior ----------------------------------------------------------------
def test_zero_noise_draw_and_prior_on_the_device():
    p, x, r64, r32 = case(8, 3, 6)
    gp = df_layer(p)
    gp.build_cache(noise=gp.mean_noise())
    gp.cache.check_factorisation()
    R.within(gp(x.cuda()), r64, r32, 'mean')
    R.within(gp.posterior(x.cuda())[0], r64, r32, 'mean')
    pi, xi, i64, i32 = case(8, 3, 6, us_identity=True)
    ell, var, _ = R.factor(O.to_dtype(pi, torch.float64))
    prior = torch.diagonal(O.df_K(xi.double(), None, ell, var)).reshape(6, 3)
    assert (i64['diag'] - prior).abs().max() < 1e-10
    got = df_layer(pi).posterior(xi.cuda())[1]
    R.within(got, dict(diag=prior), i32, 'diag')


# ---- 4. q_diag=True ------------------------------------------------------------------------------------------------------------------
def test_q_diag_layer_uses_the_diagonal_covariance():
    p, x, _, _ = case(8, 3, 6)
    raw = torch.randn(8, 3, generator=torch.Generator().manual_seed(3))
    pq = dict(p, Us=raw)
    r64, r32 = R.references(pq, x)
    gp = df_layer(pq, q_diag=True)
    for cov in MODES:
        mean, var = gp.posterior(x.cuda(), cov=cov)
        R.within(mean, r64, r32, 'mean')
        R.within(var, r64, r32, cov)


# ---- 5. chunks -----------------------------------------------------------------------------------------------------------------------
def test_chunked_queries():
    from vae_gp_ode_amd import _lib, ops
    M, D, N = 8, 3, 20
    p, x, r64, r32 = case(M, D, N)
    assert ops.conditional_df_chunks(D, M, N, 'diag', 48) == [(0, 8), (8, 16), (16, 20)]
    for cov in ('diag', 'point'):
        one = on_gpu(p, x, cov)
        cut = on_gpu(p, x, cov, max_rows=48)
        for got, ref, what in zip(cut, one, ('mean', cov)):
            R.within(got, r64, r32, what)
            e, tw = R.relerr(got, ref), R.relerr(r32[what], r64[what])
            print('%s chunked against one chunk: %.3e' % (what, e))
            assert e < 1e-4 + 3 * tw
    args = [p[k].cuda() for k in KEYS] + [x.cuda()]
    ops.kernel_matrix('DF', args[0], args[1], args[5], None)   # something else launched last: a launch by the refused call would show
    assert last_launch() == 'kernel_matrix'
    with pytest.raises(_lib.GpodeError, match='max_rows=48'):
        ops.conditional_df(*args, cov='full', max_rows=48)
    assert last_launch() == 'kernel_matrix'


# ---- 6. the workspace ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,D,N', [(8, 3, 6), (100, 6, 66)])
def test_nothing_is_read_from_the_workspace_that_the_call_did_not_write(M, D, N):
    from vae_gp_ode_amd import _lib, ops
    p, x, _, _ = case(M, D, N)
    dev = [p[k].cuda().contiguous() for k in KEYS] + [x.cuda().contiguous()]
    wf = ctypes.c_size_t(0)
    _lib.call('gpode_conditional_df_ws', D, M, N, ctypes.byref(wf))
    for mode, shape in enumerate(((N, D), (N, D, D), (N * D, N * D))):
        outs = []
        for fill in (float('nan'), 0.0):
            ws = torch.full((wf.value,), fill, dtype=torch.float32, device='cuda')
            mean, var = torch.full((N, D), 7.0, device='cuda'), torch.full(shape, 7.0, device='cuda')
            _lib.call('gpode_conditional_df', D, M, N, *[ops._ptr(t) for t in dev[:5]], ops._ptr(dev[5]), mode, ops._ptr(mean), ops._ptr(var),
                      ops._ptr(ws), ops._stream())
            torch.cuda.synchronize()
            assert ws[:1].view(torch.int32).item() & 1 == 0
            outs.append((mean, var))
        assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    from vae_gp_ode_amd import _lib, ops
    g = torch.Generator().manual_seed(0)
    M, D = 4, 17
    big = [torch.randn(D, D, generator=g), torch.randn(D, generator=g), torch.randn(M, D, generator=g), torch.randn(M, D, generator=g),
           torch.randn(D, M * (M + 1) // 2, generator=g), torch.randn(3, D, generator=g)]
    big = [t.cuda() for t in big]
    with pytest.raises(_lib.GpodeError, match='D = 2 .. 16'):
        ops.conditional_df(*big)
    mean, var, ws = (torch.full((n,), 7.0, device='cuda') for n in (3 * D, 3 * D, 4096))
    rc = _lib.load().gpode_conditional_df(D, M, 3, *[ops._ptr(t) for t in big], 0, ops._ptr(mean), ops._ptr(var), ops._ptr(ws), ops._stream())
    torch.cuda.synchronize()
    assert rc != 0 and b'D = 2 .. 16' in _lib.load().gpode_last_error()
    assert (mean == 7).all() and (var == 7).all() and (ws == 7).all()
    p, x, _, _ = case(8, 3, 6)
    args = [p[k].cuda() for k in KEYS]
    with pytest.raises(_lib.GpodeError, match='D_in == D_out'):
        ops.conditional_df(args[0][:, :2].contiguous(), *args[1:], x.cuda())
    with pytest.raises(_lib.GpodeError, match=r'x must be \(N,3\)'):
        ops.conditional_df(*args, x[:, :2].cuda())
    with pytest.raises(_lib.GpodeError, match='cov_mode=3'):
        _lib.call('gpode_conditional_df', 3, 8, 6, *[ops._ptr(t) for t in args], ops._ptr(x.cuda()), 3, ops._ptr(mean), ops._ptr(var),
                  ops._ptr(ws), ops._stream())
    torch.cuda.synchronize()
    assert (mean == 7).all() and (var == 7).all() and (ws == 7).all()


# ---- 8. the RBF layer ----------------------------------------------------------------------------------------------------------------
def _rbf_layer(Di, Do, q_diag, seed):
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    torch.manual_seed(seed)
    gp = SVGP_Layer(Di, Do, 20, 16, q_diag=q_diag, kernel='RBF').cuda()
    with torch.no_grad():
        gp.kern.unconstrained_lengthscales.fill_(O.invsoftplus(torch.tensor(1.5)).item())
        gp.kern.unconstrained_variance.fill_(O.invsoftplus(torch.tensor(0.7)).item())
        gp.Um.optvar.add_(0.2 * torch.randn_like(gp.Um.optvar))
        gp.Us_sqrt.optvar.add_(0.3 * torch.randn_like(gp.Us_sqrt.optvar))
    return gp, torch.randn(11, Di)


def test_rbf_posterior_is_build_conditional_for_a_triangular_scale():
    gp, x = _rbf_layer(6, 3, False, 5)
    mean, var = gp.posterior(x.cuda())
    m0, v0 = gp.build_conditional(x.cuda())
    assert torch.equal(mean, m0) and torch.equal(var, v0)
    mean_f, cov = gp.posterior(x.cuda(), cov='full')
    m1, c1 = gp.build_conditional(x.cuda(), full_cov=True)
    assert torch.equal(mean_f, m1) and torch.equal(cov, c1) and cov.shape == (11, 11, 3)
    mean_p, blocks = gp.posterior(x.cuda(), cov='point')
    assert torch.equal(mean_p, m0) and torch.equal(blocks, torch.diag_embed(v0)) and blocks.shape == (11, 3, 3)


@pytest.mark.parametrize('Di,Do', [(6, 3), (5, 5)])
def test_rbf_posterior_with_a_diagonal_scale(Di, Do):
    """q_diag=True: S_d = diag(s_d^2) -- the oracle's build_conditional fed the diagonal scale as a packed triangle.  (5, 5) is not a
    compiled width: evaluated zero-padded."""
    gp, x = _rbf_layer(Di, Do, True, 6)
    dense = torch.diag_embed(O.softplus(gp.Us_sqrt.optvar.detach().cpu()).T)
    p32 = dict(raw_ell=gp.kern.unconstrained_lengthscales.detach().cpu(), raw_var=gp.kern.unconstrained_variance.detach().cpu(),
               Z=gp.inducing_loc.optvar.detach().cpu(), Um=gp.Um.optvar.detach().cpu(), Us=O.tril_pack(dense))
    p64 = O.to_dtype(p32, torch.float64)
    for cov, full in (('diag', False), ('full', True)):
        mean, var = gp.posterior(x.cuda(), cov=cov)
        m64, v64 = O.build_conditional(p64, x.double(), full_cov=full)
        m32, v32 = O.build_conditional(p32, x, full_cov=full)
        assert mean.shape == m64.shape and var.shape == v64.shape
        em, ev = R.relerr(mean, m64), R.relerr(var, v64)
        print('%s: mean %.3e (twin %.3e), var %.3e (twin %.3e)' % (cov, em, R.relerr(m32, m64), ev, R.relerr(v32, v64)))
        assert em < 1e-4 + 3 * R.relerr(m32, m64) and ev < 1e-4 + 3 * R.relerr(v32, v64)
    blocks = gp.posterior(x.cuda(), cov='point')[1]
    assert torch.equal(blocks, torch.diag_embed(gp.posterior(x.cuda())[1]))


# ---- 9. the command line -------------------------------------------------------------------------------------------------------------
def test_cli_eval_field(tmp_path):
    import numpy as np
    from vae_gp_ode_amd import evaluate as E
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('WORLD_SIZE', None)
    common = ['--task', 'synthetic', '--Ndata', '8', '--Ntest', '6', '--batch', '4', '--T', '6', '--solver', 'rk4', '--num_inducing', '16',
              '--num_features', '32', '--lr', '1e-4', '--log_freq', '1', '--kernel', 'DF']
    r = subprocess.run([sys.executable, '-m', 'vae_gp_ode_amd.main'] + common + ['--Nepoch', '1', '--save', 'results/t'], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ck = glob.glob(str(tmp_path / 'results' / 't_*' / 'odegpvae_mnist.pth'))
    assert len(ck) == 1
    argv = common + ['--model_path', os.path.dirname(ck[0]), '--eval_sample_size', '3', '--Troll', '2', '--device_noise', 'True']
    r = subprocess.run([sys.executable, '-m', 'vae_gp_ode_amd.evaluate'] + argv + ['--save', 'results/on', '--eval_field', 'True'], cwd=tmp_path,
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    on = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    d = tmp_path / 'results' / 'on'
    assert json.load(open(d / 'eval.json')) == on
    z, mean, var = (np.load(d / ('field_%s.npy' % k)) for k in ('z', 'mean', 'var'))
    assert z.shape == mean.shape == var.shape == (6, 6) and on['field_points'] == 6
    assert np.isfinite(z).all() and np.isfinite(mean).all() and np.isfinite(var).all() and (var > 0).all()
    assert on['field_var_mean'] == float(var.mean()) and on['field_var_max'] == float(var.max())
    # switched off (the default): the same process-independent figures, none of the keys, none of the files
    off = E.main(argv + ['--save', str(tmp_path / 'results' / 'off')])
    assert not [k for k in off if k.startswith('field_')]
    assert sorted(k for k in on if not k.startswith('field_')) == sorted(off)
    assert not glob.glob(str(tmp_path / 'results' / 'off' / 'field_*'))
    assert sorted(os.listdir(tmp_path / 'results' / 'off')) == ['eval.json', 'rollout_mean.npy', 'rollout_var.npy']
    assert all(on[k] == off[k] for k in ('mse', 'std', 'nll', 'nlpd', 'count', 'sequences'))
