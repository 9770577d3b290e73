"""CPU: the host half of the marginal held-out likelihood -- evaluate.iw_stats, the result type, the command-line parser -- and the host-side
refusals of the per-draw initial-state entry points (they return before any launch, so they run without a GPU).

Notation: a[l,n] = ll[l,n] + lw[l,n];  iw_ll[n] = log mean_l exp a;  ess[n] = (sum_l w)^2 / sum_l w^2, w = exp(a - max_l a)."""
import ctypes
import math

import pytest
import torch


def _draws(L, N, seed, scale=5.0, centre=-50.0):
    g = torch.Generator().manual_seed(seed)
    return centre + scale * torch.randn(L, N, generator=g, dtype=torch.float64), 2.0 * torch.randn(L, N, generator=g, dtype=torch.float64)


def test_iw_stats_matches_brute_force():
    """values small enough for a plain exp: log(mean(exp(a))) and the weights exp(a) themselves, no maximum subtracted"""
    from vae_gp_ode_amd.evaluate import iw_stats
    for L, N, seed in ((1, 1, 0), (4, 3, 1), (128, 40, 2)):
        ll, lw = _draws(L, N, seed)
        iw_ll, iw_nll, ess = iw_stats(ll, lw)
        w = torch.exp(ll + lw)
        ref_ll, ref_ess = torch.log(w.mean(0)), w.sum(0) ** 2 / (w * w).sum(0)
        assert iw_ll.dtype == torch.float64 and tuple(iw_ll.shape) == (N,) and tuple(ess.shape) == (N,) and isinstance(iw_nll, float)
        assert ((iw_ll - ref_ll).abs() <= 1e-12 * ref_ll.abs()).all()
        assert ((ess - ref_ess).abs() <= 1e-12 * ref_ess).all()
        assert abs(iw_nll + ref_ll.mean().item()) <= 1e-12 * abs(ref_ll.mean().item())
        assert (ess >= 1 - 1e-12).all() and (ess <= L + 1e-12).all()
        # float32 input (what the device hands over) is widened, not rounded again; the same input gives the same bits
        again = iw_stats(ll, lw)
        assert torch.equal(again[0], iw_ll) and again[1] == iw_nll and torch.equal(again[2], ess)


def test_zero_log_weights_give_log_mean_exp():
    """lw = 0: iw_ll is log_mean_exp(ll), the same bits (the same operations in the same order).  The weights are then exp(ll), so the
    effective sample size is L where the draws agree on ll -- exactly L: L ones summed -- and below L where they do not."""
    from vae_gp_ode_amd.evaluate import iw_stats, log_mean_exp
    ll, _ = _draws(7, 11, 3, centre=-3000.0)
    iw_ll, iw_nll, ess = iw_stats(ll, torch.zeros_like(ll))
    assert torch.equal(iw_ll, log_mean_exp(ll)) and iw_nll == -log_mean_exp(ll).mean().item()
    assert (ess < 7).all()
    same = ll[:1].expand(7, 11).contiguous()
    iw_ll, _, ess = iw_stats(same, torch.zeros_like(same))
    assert torch.equal(iw_ll, log_mean_exp(same)) and (ess == 7).all()
    assert ((iw_ll - same[0]).abs() <= 1e-12 * same[0].abs()).all()


def test_shift_of_the_log_weights():
    """adding c to lw[:, n] multiplies every weight of sequence n by e^c: iw_ll[n] moves by c, ess[n] does not move"""
    from vae_gp_ode_amd.evaluate import iw_stats
    ll, lw = _draws(9, 6, 4, centre=-800.0)
    base_ll, _, base_ess = iw_stats(ll, lw)
    c = torch.tensor([0.0, 1.0, -3.5, 40.0, -700.0, 1e-3], dtype=torch.float64)
    got_ll, _, got_ess = iw_stats(ll, lw + c)
    assert ((got_ll - (base_ll + c)).abs() <= 1e-12 * (base_ll + c).abs()).all()
    assert ((got_ess - base_ess).abs() <= 1e-10 * base_ess).all()      # a + c rounds at |a| = 1e3: 1e-13 relative on every weight


def test_large_magnitudes_stay_finite_and_jensen_holds():
    from vae_gp_ode_amd.evaluate import iw_stats
    g = torch.Generator().manual_seed(5)
    L, N = 16, 8
    ll = -3000.0 + 30.0 * torch.randn(L, N, generator=g, dtype=torch.float64)
    lw = 50.0 * (2 * torch.randint(0, 2, (L, N), generator=g).double() - 1) + torch.randn(L, N, generator=g, dtype=torch.float64)
    iw_ll, iw_nll, ess = iw_stats(ll, lw)
    assert torch.isfinite(iw_ll).all() and math.isfinite(iw_nll) and torch.isfinite(ess).all()
    assert (iw_ll >= (ll + lw).mean(0)).all()                          # log of a mean >= mean of the logs
    assert (iw_ll <= (ll + lw).max(0).values).all() and (iw_ll >= (ll + lw).max(0).values - math.log(L)).all()
    assert (ess >= 1).all() and (ess <= L).all()
    # float32 inputs, as they come back from the device
    f_ll, _, f_ess = iw_stats(ll.float(), lw.float())
    assert torch.isfinite(f_ll).all() and f_ll.dtype == torch.float64 and ((f_ll - iw_ll).abs() <= 1e-3).all()


def test_one_dominant_weight():
    from vae_gp_ode_amd.evaluate import iw_stats
    ll, lw = _draws(12, 5, 6)
    lw[3] += 200.0
    iw_ll, _, ess = iw_stats(ll, lw)
    assert ((ess - 1).abs() <= 1e-12).all()
    assert ((iw_ll - (ll[3] + lw[3] - math.log(12))).abs() <= 1e-12 * iw_ll.abs()).all()


def test_result_type_and_unchanged_prediction():
    from vae_gp_ode_amd import evaluate as E
    assert E.MarginalPrediction._fields == ('ll', 'lw', 'nll', 'nlpd', 'iw_ll', 'iw_nll', 'ess', 'nll_t', 'mse', 'std', 'state', 'passes')
    assert E.Prediction._fields == ('mean', 'var', 'mse', 'std', 'count', 'mse_t', 'state', 'passes', 'll', 'nll', 'nlpd', 'nll_t')


def test_evaluation_parser_accepts_a_training_command_line():
    """evaluate.make_parser: main.py's parser (the reference's 39 flags, untouched) plus --eval_z0_draws, off by default"""
    from vae_gp_ode_amd import evaluate, main
    assert len(main.FLAGS) == 39 and 'eval_z0_draws' not in {f[0] for f in main.FLAGS + main.EXT_FLAGS}
    argv = ['--data_root', 'data/', '--task', 'mnist', '--mask', 'True', '--value', '3', '--data_seqlen', '100', '--batch', '20', '--T', '16',
            '--Ndata', '360', '--Ntest', '40', '--rotrand', 'True', '--latent_dim', '6', '--n_filt', '8', '--frames', '5', '--pretrained', 'False',
            '--vae_path', 'x', '--kernel', 'RBF', '--num_features', '256', '--num_inducing', '100', '--dimwise', 'True', '--variance', '0.7',
            '--lengthscale', '2.0', '--q_diag', 'False', '--ode', '1', '--D_in', '6', '--D_out', '6', '--solver', 'rk4', '--ts_dense_scale', '2',
            '--use_adjoint', 'False', '--dt', '0.1', '--Nepoch', '5000', '--lr', '0.001', '--eval_sample_size', '128', '--save', 'results/mnist',
            '--seed', '121', '--log_freq', '5', '--device', 'cuda:0', '--continue_training', 'False', '--model_path', 'results/mnist_x', '--Troll', '2']
    assert {a[2:] for a in argv[::2]} == {f[0] for f in main.FLAGS}
    a = evaluate.make_parser().parse_args(argv)
    assert a.eval_z0_draws is False and a.eval_sample_size == 128 and a.model_path == 'results/mnist_x'
    ref = vars(main.make_parser().parse_args(argv))
    assert {k: v for k, v in vars(a).items() if k != 'eval_z0_draws'} == ref
    b = evaluate.make_parser().parse_args(argv + ['--eval_z0_draws', 'True', '--device_noise', 'True'])
    assert b.eval_z0_draws is True and b.device_noise is True
    with pytest.raises(SystemExit):
        main.make_parser().parse_args(['--eval_z0_draws', 'True'])


NZ = ('gpode_rollout_fwd_nz', 'gpode_rollout_adaptive_fwd_nz', 'gpode_rollout_dense_fwd_nz')


def test_per_draw_entry_points_are_the_twins_plus_one_flag():
    from vae_gp_ode_amd import _lib
    for name in NZ:
        res, args = _lib.SIGNATURES[name]
        tres, targs = _lib.SIGNATURES[name[:-1]]
        assert res is tres and args == targs[:-1] + [ctypes.c_int, ctypes.c_void_p] and targs[-1] is ctypes.c_void_p


def test_bad_flag_is_refused_on_the_host():
    """z0_per_draw outside {0, 1} is refused before anything else is looked at: no device is touched, so this runs anywhere"""
    from vae_gp_ode_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    for flag in (2, -1):
        assert lib.gpode_rollout_fwd_nz(0, 1, 1, 6, 6, 8, 16, 3, null, null, null, 4, 3, null, null, flag, null) != 0
        assert lib.gpode_last_error().decode().startswith('gpode_rollout_fwd_nz:')
        assert lib.gpode_rollout_adaptive_fwd_nz(0, 1, 3, 6, 6, 8, 16, 3, null, null, null, 4, 3, 1e-4, 1e-4, 8, null, null, null, null, null,
                                                 flag, null) != 0
        assert lib.gpode_last_error().decode().startswith('gpode_rollout_adaptive_fwd_nz:')
        assert lib.gpode_rollout_dense_fwd_nz(0, 1, 3, 6, 6, 8, 16, 3, null, null, null, 4, 3, 1e-4, 1e-4, 8, null, null, null, null, null, null,
                                              flag, null) != 0
        assert lib.gpode_last_error().decode().startswith('gpode_rollout_dense_fwd_nz:')
    # a good flag gets as far as the pointer check
    assert lib.gpode_rollout_fwd_nz(0, 1, 1, 6, 6, 8, 16, 3, null, null, null, 4, 3, null, null, 1, null) != 0
    assert lib.gpode_last_error().decode() == 'gpode_rollout_fwd_nz: null pointer'
    assert lib.gpode_reparam_draws_fwd(null, null, 6, null, null, 6, null, 2, 3, 4, 6, null) != 0
    assert lib.gpode_last_error().decode().startswith('gpode_reparam_draws_fwd:')
