"""CPU: the definition of the DF posterior (tests/posterior_ref.py) held to identities through functions of the oracle that are
already trusted, the chunk planner of ops.conditional_df, and the argument checks that need no device."""
import ctypes

import pytest
import torch

import posterior_ref as R
from oracle import gpode_oracle as O

SHAPES = [(8, 3, 6), (8, 2, 9), (12, 16, 5), (100, 6, 12)]


@pytest.fixture(autouse=True)
def _global_generators_left_as_found():
    """a layer draws its initial values from the global numpy generator: later tests see the state they always saw"""
    import numpy as np
    state = (torch.get_rng_state(), np.random.get_state())
    yield
    torch.set_rng_state(state[0])
    np.random.set_state(state[1])


def _case(M, D, N, **kw):
    p, x = R.inputs(M, D, N, seed=M * 100 + D, z_spread=8.0 if (M, D) == (8, 2) else 1.5, **kw)
    return O.to_dtype(p, torch.float64), x.double()


@pytest.mark.parametrize('M,D,N', SHAPES)
def test_mean_is_the_update_under_zero_noise(M, D, N):
    """mean = df_f_update with nu = L^-T vec(Um): what build_cache leaves when eps_u and rff_w are zero"""
    p, x = _case(M, D, N)
    ell, var, L = R.factor(p)
    nu = torch.linalg.solve_triangular(L.T, p['Um'].reshape(-1, 1), upper=True)
    _, nu_oracle = O.df_compute_nu(O.df_K(p['Z'], None, ell, var), torch.zeros(M, D, dtype=torch.float64), p['Um'])
    assert torch.equal(nu, nu_oracle)
    want = O.df_f_update(x, p['Z'], nu, ell, var)
    got = R.posterior(p, x)['mean']
    assert (got - want).abs().max().item() < 1e-12 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize('M,D,N', SHAPES)
def test_identity_scale_gives_the_prior(M, D, N):
    """Us = I: q(u) is the prior, so the covariance is df_K(x, x) -- as it stands, not symmetrised"""
    p, x = _case(M, D, N, us_identity=True)
    ell, var, _ = R.factor(p)
    K = O.df_K(x, None, ell, var)
    ref = R.posterior(p, x)
    assert (ref['full'] - K).abs().max().item() < 1e-10
    assert (ref['diag'] - torch.diagonal(K).reshape(N, D)).abs().max().item() < 1e-10


@pytest.mark.parametrize('M,D,N', SHAPES)
def test_point_and_diag_are_entries_of_full(M, D, N):
    p, x = _case(M, D, N)
    ref = R.posterior(p, x)
    full = ref['full']
    assert ref['mean'].shape == (N, D) and ref['diag'].shape == (N, D) and ref['point'].shape == (N, D, D) and full.shape == (N * D, N * D)
    for n in range(N):
        assert torch.equal(ref['point'][n], full[n * D:(n + 1) * D, n * D:(n + 1) * D])
        assert torch.equal(ref['diag'][n], torch.diagonal(ref['point'][n]))
    assert (ref['diag'] > 0).all()


def test_transposed_fill_is_a_different_matrix():
    """K(Z,x) against K(x,Z)^T: 2 % apart in the lengthscales moves entries by about 1e-2 -- the two variants are told apart"""
    p, x = _case(8, 3, 6)
    ell, var, _ = R.factor(p)
    d = (O.df_K(p['Z'], x, ell, var) - O.df_K(x, p['Z'], ell, var).T).abs().max().item()
    assert d > 1e-4
    a, b = R.posterior(p, x), R.posterior(p, x, transposed_fill=True)
    assert R.relerr(a['mean'], b['mean']) > 1e-3


def test_q_diag_scale_is_the_diagonal_covariance():
    """a q_diag layer's raw (M,D) scale: S_d = diag(softplus(raw)^2), the distribution sample_inducing draws from"""
    p, x = _case(8, 3, 6)
    raw = torch.randn(8, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    dense = torch.diag_embed(O.softplus(raw).T)
    a = R.posterior(dict(p, Us=raw), x)
    b = R.posterior(dict(p, Us=O.tril_pack(dense)), x)
    assert torch.equal(a['full'], b['full'])


# ---- the chunk planner -------------------------------------------------------------------------------------------------------------
def test_chunk_planner():
    from vae_gp_ode_amd import _lib, ops
    plan = ops.conditional_df_chunks
    # the default holds N = 256 at M = 100, D = 6 (2136 rows) in one chunk
    assert plan(6, 100, 256) == [(0, 256)] and plan(6, 100, 256, 'full') == [(0, 256)]
    assert 100 * 6 + 256 * 6 <= ops.CONDITIONAL_DF_MAX_ROWS
    # (8, 3, 20) with 48 rows: 24 inducing rows, 8 queries per chunk -> 8, 8, 4
    assert plan(3, 8, 20, 'diag', 48) == [(0, 8), (8, 16), (16, 20)] == plan(3, 8, 20, 'point', 48)
    assert plan(3, 8, 20, 'diag', 50) == [(0, 8), (8, 16), (16, 20)]          # 26 spare rows are still 8 queries of 3
    assert plan(3, 8, 16, 'diag', 48) == [(0, 8), (8, 16)]                     # no empty tail
    assert plan(3, 8, 1, 'diag', 27) == [(0, 1)]
    for D, M, N, mr in ((3, 8, 20, 48), (6, 100, 1000, 1024), (2, 5, 7, 12)):
        ch = plan(D, M, N, 'diag', mr)
        assert ch[0][0] == 0 and ch[-1][1] == N and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all(M * D + (e - s) * D <= mr and e > s for s, e in ch)
        assert len({e - s for s, e in ch[:-1]}) <= 1 and ch[-1][1] - ch[-1][0] <= ch[0][1] - ch[0][0]
    with pytest.raises(_lib.GpodeError, match='max_rows=48'):
        plan(3, 8, 20, 'full', 48)
    assert plan(3, 8, 8, 'full', 48) == [(0, 8)]
    with pytest.raises(_lib.GpodeError, match='no room'):
        plan(3, 8, 4, 'diag', 26)
    with pytest.raises(_lib.GpodeError, match="'diag', 'point' or 'full'"):
        plan(3, 8, 4, 'marginal')
    with pytest.raises(_lib.GpodeError):
        plan(3, 8, 0)


# ---- argument checks that need no device ---------------------------------------------------------------------------------------------
def test_wrapper_argument_checks_without_a_device():
    from vae_gp_ode_amd import _lib, ops
    p, x = R.inputs(8, 3, 6, seed=1)
    args = [p['raw_ell'], p['raw_var'], p['Z'], p['Um'], p['Us']]
    with pytest.raises(_lib.GpodeError, match='D_in == D_out'):
        ops.conditional_df(p['raw_ell'][:, :2], *args[1:], x)
    with pytest.raises(_lib.GpodeError, match=r'x must be \(N,3\)'):
        ops.conditional_df(*args, x[:, :2])
    with pytest.raises(_lib.GpodeError, match="'diag', 'point' or 'full'"):
        ops.conditional_df(*args, x, cov='marginal')
    with pytest.raises(_lib.GpodeError, match='CUDA/HIP tensor'):
        ops.conditional_df(*args, x)                                           # no CPU fallback


def test_layer_argument_checks_without_a_device():
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    gp = SVGP_Layer(3, 3, 8, 16, kernel='DF')
    with pytest.raises(ValueError, match="'diag', 'point' or 'full'"):
        gp.posterior(torch.zeros(2, 3), cov='marginal')
    nz = gp.mean_noise()
    assert {k: tuple(v.shape) for k, v in nz.items()} == dict(eps_u=(8, 3), rff_w=(32, 3), rff_eps=(3, 16, 3), rff_u=(1, 16, 3))
    assert not nz['eps_u'].any() and not nz['rff_w'].any() and nz['rff_eps'].abs().min() > 0
    rbf = SVGP_Layer(6, 3, 8, 16, kernel='RBF').mean_noise()
    assert {k: tuple(v.shape) for k, v in rbf.items()} == dict(eps_u=(8, 3), rff_w=(16, 3), rff_eps=(6, 16, 3), rff_u=(1, 16, 3))
    with pytest.raises(NotImplementedError):
        gp.build_conditional(torch.zeros(2, 3))                                # stays refused for DF


def test_eval_field_switch_is_off_unless_given():
    from vae_gp_ode_amd import evaluate, main
    p = evaluate.make_parser()
    off = p.parse_args([])
    assert evaluate.eval_field(off) is False
    assert {k: v for k, v in vars(off).items() if k != 'eval_z0_draws'} == vars(main.make_parser().parse_args([]))
    assert evaluate.eval_field(p.parse_args(['--eval_field', 'True'])) is True
    assert evaluate.eval_field(p.parse_args(['--eval_field', 'False'])) is False
    with pytest.raises(SystemExit):
        main.make_parser().parse_args(['--eval_field', 'True'])


def test_c_abi_refusals_ahead_of_any_launch():
    """D outside 2 .. 16, M <= 0, N <= 0 and M D > 8192: a message, a non-zero return, and no buffer touched (host memory here:
    a launch would have faulted on it)"""
    from vae_gp_ode_amd import _lib
    lib = _lib.load()
    wf = ctypes.c_size_t(7)
    for D, M, N, words in ((17, 8, 4, b'D = 2 .. 16'), (1, 8, 4, b'D = 2 .. 16'), (3, 0, 4, b'M=0'), (3, 8, 0, b'N=0'), (3, 8, -1, b'N=-1'),
                           (6, 1366, 4, b'at most 8192')):
        assert lib.gpode_conditional_df_ws(D, M, N, ctypes.byref(wf)) != 0
        assert words in lib.gpode_last_error(), (D, M, N, lib.gpode_last_error())
        assert wf.value == 7
    buf = (ctypes.c_float * 64)(*([3.0] * 64))
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gpode_conditional_df(17, 8, 4, ptr, ptr, ptr, ptr, ptr, ptr, 0, ptr, ptr, ptr, None) != 0
    assert b'D = 2 .. 16' in lib.gpode_last_error() and all(v == 3.0 for v in buf)
    assert lib.gpode_conditional_df(3, 8, 4, ptr, ptr, ptr, None, ptr, ptr, 0, ptr, ptr, ptr, None) != 0
    assert b'null pointer' in lib.gpode_last_error()
    assert lib.gpode_conditional_df_ws(3, 8, 6, ctypes.byref(wf)) == 0
    np_ = 64                                                                   # 24 + 18 = 42 rows -> two tiles
    assert 2 * np_ * np_ < wf.value <= 3 * np_ * np_
    assert lib.gpode_conditional_df_ws(6, 100, 256, ctypes.byref(wf)) == 0 and wf.value <= 3 * 2176 * 2176
