"""CPU-only: the host side of training on the importance-weighted bound (iw_ref.py states the objective).
  closed forms    gmu / glogvar of the K draws and grow / glw of the loss stage, restated in float64 as the kernels evaluate them, agree with
                  autograd on iw_ref to 1e-12 of the largest entry (float64 round-off over sums of at most 64 terms)
  Jensen          iw[l,n] >= mean_k a[l,k,n] for random inputs, in float64, a of magnitude 2e3
  iw_stats        evaluate.iw_stats(ll, lw) equals iw_ref for L = 1 (both subtract the maximum; float64 on both sides: 1e-12)
  degenerate      equal a over k: weights exactly 1/K, ess exactly K; one draw ahead by 1000 nats: one-hot weights, ess exactly 1
  the CLI         --iw_draws is 0 by default, parses in main and evaluate, and each refusal (K outside 1..64, --ragged_compact True,
                  several ranks) is raised by main() ahead of any device work
  compute_loss    compact=True, a bad K and too many rows raise before the model is touched; GPODE_UNFUSED_LOSS=1 likewise
  the C ABI       the four new entry points stand in _lib.SIGNATURES and in include/gpode.h with the same number of arguments"""
import os
import re

import pytest
import torch

import iw_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('gpode_reparam_draws_bwd', 'gpode_elbo_iw_fwd', 'gpode_elbo_iw_bwd', 'gpode_elbo_iw_bwd_ll')
F64 = torch.float64


def _inputs(L, K, N, seed):
    g = torch.Generator().manual_seed(seed)
    ll = -2000.0 + 3.0 * torch.randn(L, K, N, generator=g, dtype=F64)
    lw = -3.0 + 2.0 * torch.randn(K, N, generator=g, dtype=F64)
    return ll, lw


@pytest.mark.parametrize('K,N,q,null', [(1, 1, 1, ''), (3, 5, 6, ''), (3, 5, 6, 'gz'), (3, 5, 6, 'glw'), (64, 2, 16, '')])
def test_draws_closed_form_against_autograd(K, N, q, null):
    g = torch.Generator().manual_seed(K * 100 + N * 10 + q)
    mu, logvar = torch.randn(N, q, generator=g, dtype=F64), 0.7 * torch.randn(N, q, generator=g, dtype=F64) - 1
    eps = torch.randn(K, N, q, generator=g, dtype=F64)
    gz = None if null == 'gz' else torch.randn(K, N, q, generator=g, dtype=F64)
    glw = None if null == 'glw' else torch.randn(K, N, generator=g, dtype=F64)
    for got, ref in zip(W.draws_grads_closed_form(mu, logvar, eps, gz, glw), W.draws_grads(mu, logvar, eps, gz, glw)):
        assert float((got - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1.0)


@pytest.mark.parametrize('L,K,N', [(1, 1, 1), (2, 3, 5), (1, 64, 2), (2, 8, 3)])
def test_stage_closed_form_against_autograd(L, K, N):
    ll, lw = _inputs(L, K, N, 7 * L + K + N)
    M, Do, nobs, seeds = 5, 3, 360.0, (1.3, -0.7, 0.45, 2.1)
    g = torch.Generator().manual_seed(3)
    Um = torch.randn(M, Do, generator=g, dtype=F64)
    Us = 0.01 * torch.randn(Do, M * (M + 1) // 2, generator=g, dtype=F64)
    Us[:, W.diag_index(M)] = 0.5 + torch.rand(Do, M, generator=g, dtype=F64)
    _, grow, glw, dUm, dUs = W.objective_grads(ll.reshape(-1, 1), lw, Um, Us, L, K, N, M, nobs, seeds)
    grow_c, glw_c = W.stage_grads_closed_form(ll, lw, nobs, seeds)
    assert float((grow_c.reshape(-1) - grow).abs().max()) <= 1e-12 * float(grow.abs().max())
    assert float((glw_c - glw).abs().max()) <= 1e-12 * float(glw.abs().max())
    # k_elbo_all_bwd's expressions for the inducing posterior
    gk = seeds[0] + seeds[3]
    dUs_c = gk * Us.clone()
    dUs_c[:, W.diag_index(M)] = gk * (Us[:, W.diag_index(M)] - 1 / Us[:, W.diag_index(M)])
    assert float((gk * Um - dUm).abs().max()) <= 1e-12 * float(dUm.abs().max())
    assert float((dUs_c - dUs).abs().max()) <= 1e-12 * float(dUs.abs().max())


def test_jensen_holds_for_random_inputs():
    for seed in range(20):
        L, K, N = 1 + seed % 3, 1 + (seed * 7) % 64, 1 + seed % 5
        ll, lw = _inputs(L, K, N, seed)
        a, iw, p, ess = W.weights(ll, lw)
        assert bool((iw >= a.mean(1) - 1e-9).all()), seed
        assert bool(((ess >= 1 - 1e-12) & (ess <= K + 1e-9)).all()) and bool(((p.sum(1) - 1).abs() < 1e-12).all())
        if K == 1:
            assert bool((iw == a[:, 0]).all())


def test_iw_stats_equals_the_reference_for_one_function_draw():
    from vae_gp_ode_amd import evaluate as E
    K, N = 16, 7
    ll, lw = _inputs(1, K, N, 11)
    iw_ll, iw_nll, ess = E.iw_stats(ll[0], lw)
    _, iw, _, ess_ref = W.weights(ll, lw)
    assert float((iw_ll - iw[0]).abs().max()) <= 1e-12 * 2000 and abs(iw_nll + float(iw.mean())) <= 1e-12 * 2000
    assert float((ess - ess_ref[0]).abs().max()) <= 1e-12 * K


@pytest.mark.parametrize('K', [1, 2, 8, 64])
def test_degenerate_weights_are_exact(K):
    L, N = 2, 3
    g = torch.Generator().manual_seed(K)
    base = -2000.0 + 3.0 * torch.randn(L, 1, N, generator=g, dtype=F64)
    lw = torch.zeros(K, N, dtype=F64)
    # equal a over k
    a, iw, p, ess = W.weights(base.expand(L, K, N).contiguous(), lw)
    assert bool((p == 1.0 / K).all()) and bool((ess == float(K)).all())
    assert float((iw - base[:, 0]).abs().max()) <= 1e-12 * 2000
    # one draw ahead by 1000 nats
    ll = base.expand(L, K, N).clone()
    ahead = K // 2
    ll[:, ahead] += 1000.0
    a, iw, p, ess = W.weights(ll, lw)
    onehot = torch.zeros(L, K, N, dtype=F64)
    onehot[:, ahead] = 1.0
    assert bool((p == onehot).all()) and bool((ess == 1.0).all())


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_flag_is_off_by_default_and_parses():
    from vae_gp_ode_amd import evaluate as E
    from vae_gp_ode_amd import main as M
    assert M.make_parser().parse_args([]).iw_draws == 0
    assert M.make_parser().parse_args(['--iw_draws', '4']).iw_draws == 4
    assert E.make_parser().parse_args(['--iw_draws', '4']).iw_draws == 4      # training command lines are reused; evaluate ignores it


@pytest.mark.parametrize('case', ['K = 65', 'K = -1', 'ragged_compact', 'ranks'])
def test_flag_refusals_come_before_any_device_work(case, monkeypatch, tmp_path):
    from vae_gp_ode_amd import main as M
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    touched = []
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: touched.append('is_available') or False)
    monkeypatch.setattr(M, 'init_distributed', lambda: touched.append('init_distributed'))
    argv = ['--task', 'synthetic', '--T', '6']
    if case == 'K = 65':
        argv += ['--iw_draws', '65']
        want = '1..64'
    elif case == 'K = -1':
        argv += ['--iw_draws', '-1']
        want = '1..64'
    elif case == 'ragged_compact':
        argv += ['--iw_draws', '4', '--ragged_frames', '3', '--ragged_compact', 'True']
        want = 'not with --ragged_compact'
    else:
        argv += ['--iw_draws', '4']
        monkeypatch.setenv('WORLD_SIZE', '2')
        want = 'not on several ranks'
    with pytest.raises(SystemExit) as e:
        M.main(argv)
    assert '--iw_draws' in str(e.value) and want in str(e.value), str(e.value)
    assert not touched and not os.listdir(tmp_path), (touched, os.listdir(tmp_path))


@pytest.mark.parametrize('kw,want', [(dict(iw_draws=4, compact=True), 'not built for compact=True'), (dict(iw_draws=0), '1..64'),
                                     (dict(iw_draws=65), '1..64'), (dict(iw_draws=2.5), '1..64'), (dict(iw_draws=64), '65535')])
def test_compute_loss_refusals_need_no_model(kw, want):
    from vae_gp_ode_amd.model.create_model import compute_loss
    X = torch.zeros(600, 3, 1, 28, 28) if kw.get('iw_draws') == 64 else torch.zeros(2, 3, 1, 28, 28)
    with pytest.raises(ValueError, match=want):
        compute_loss(None, X, 2, **kw)


def test_compute_loss_refuses_the_unfused_loss(monkeypatch):
    from vae_gp_ode_amd.model import create_model as C
    monkeypatch.setattr(C, '_FUSED_LOSS', False)
    with pytest.raises(ValueError, match='GPODE_UNFUSED_LOSS=1'):
        C.compute_loss(None, torch.zeros(2, 3, 1, 28, 28), 1, iw_draws=2)


def test_new_entry_points_are_declared_and_bound_alike():
    from vae_gp_ode_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'gpode.h')).read(), flags=re.S)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, txt)
        assert m, 'not declared in include/gpode.h: ' + name
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
