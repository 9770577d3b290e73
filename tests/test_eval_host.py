"""CPU-only: the host side of the posterior-predictive evaluation (vae_gp_ode_amd/evaluate.py) -- the merge of {n, mean, M2}
triples, the pass splitter, the command-line parser, and the internal consistency of the eval_* fixtures."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

EVAL_CASES = ['eval_rbf1', 'eval_rbf2', 'eval_df1', 'eval_rbf1_roll']


def triple(x):
    x = np.asarray(x, dtype=np.float64)
    return float(x.size), float(x.mean()), float(((x - x.mean()) ** 2).sum())


@pytest.mark.parametrize('sizes', [(784, 784, 784), (1, 5, 2, 1000), (3,), (7, 1)])
@pytest.mark.parametrize('kind', ['plain', 'large_mean_tiny_variance', 'mixed_scales'])
def test_merge_states_matches_numpy_float64(sizes, kind):
    from vae_gp_ode_amd.evaluate import mean_std, merge_states
    rng = np.random.RandomState(len(sizes) * 31 + len(kind))
    chunks = []
    for i, n in enumerate(sizes):
        if kind == 'plain':
            chunks.append(rng.rand(n))
        elif kind == 'large_mean_tiny_variance':        # sum-of-squares formulas lose every digit here
            chunks.append(1e6 + 1e-3 * rng.randn(n))
        else:
            chunks.append(10.0 ** (i - 1) * rng.randn(n) + i)
    allx = np.concatenate(chunks)
    n, mean, m2 = merge_states([triple(c) for c in chunks])
    assert n == allx.size
    assert abs(mean - allx.mean()) <= 1e-12 * max(1.0, abs(allx.mean()))
    ref_m2 = ((allx - allx.mean()) ** 2).sum()
    # float64 cannot do better than this: every chunk mean carries a rounding error of eps |mean|, which enters the merge relative to
    # the spread of the data, so M2 is good to a few eps |mean| / sigma (8 of them allowed), and to 1e-12 where that is smaller
    rel = 8 * np.finfo(np.float64).eps * abs(allx.mean()) / allx.std() + 1e-12
    assert abs(m2 - ref_m2) <= rel * ref_m2
    got_mean, got_std = mean_std((n, mean, m2))
    if allx.size > 1:
        ref_std = torch.std(torch.from_numpy(allx)).item()
        assert abs(got_std - ref_std) <= rel * ref_std
    assert got_mean == mean


def test_merge_states_edge_cases():
    from vae_gp_ode_amd.evaluate import mean_std, merge_states
    assert merge_states([]) == (0.0, 0.0, 0.0)
    assert merge_states([(0, 0.0, 0.0), (4, 2.5, 1.0), (0, 0.0, 0.0)]) == (4.0, 2.5, 1.0)     # empty triples (forecast frames) are skipped
    one = merge_states([triple([0.25])])
    assert one == (1.0, 0.25, 0.0)
    mean, std = mean_std(one)
    assert mean == 0.25 and np.isnan(std) and torch.isnan(torch.std(torch.tensor([0.25])))     # n - 1 = 0: nan, as torch
    # the order of the triples is part of the definition: the same order gives the same bits
    ts = [triple(np.random.RandomState(s).rand(50)) for s in range(5)]
    assert merge_states(ts) == merge_states(list(ts))
    # float32 triples as the kernel leaves them merge without leaving float64
    n, mean, m2 = merge_states([(np.float32(784), np.float32(0.1), np.float32(2.0))] * 3)
    assert n == 2352.0 and abs(mean - float(np.float32(0.1))) < 1e-15 and abs(m2 - 6.0) < 1e-12


def test_plan_passes():
    from vae_gp_ode_amd.evaluate import plan_passes
    assert plan_passes(128, 640, 8192) == [(i, min(128, i + 12)) for i in range(0, 128, 12)]
    assert plan_passes(5, 96, 8192) == [(0, 5)]
    assert plan_passes(5, 96, 96) == [(i, i + 1) for i in range(5)]
    assert plan_passes(1, 8192, 8192) == [(0, 1)]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        assert plan_passes(3, 1280, 1000) == [(0, 1), (1, 2), (2, 3)]          # a pass cannot hold less than one draw
    assert len(w) == 1 and 'one draw per pass' in str(w[0].message)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        plan_passes(3, 1280, 1280)                                            # an exact fit is not a fall-back
    for bad in ((0, 10, 10), (1, 0, 10), (1, 10, 0)):
        with pytest.raises(ValueError):
            plan_passes(*bad)
    # every draw is decoded exactly once, whatever the budget
    for L, per, budget in ((128, 640, 8192), (7, 33, 100), (9, 10, 10)):
        got = plan_passes(L, per, budget)
        assert [a for a, _ in got] == [0] + [b for _, b in got[:-1]] and got[-1][1] == L
        assert all((b - a) * per <= budget for a, b in got)


def test_cli_parser_accepts_the_reference_flag_set():
    """The evaluation CLI parses with main.py's parser: a training command line is reusable as it stands."""
    from vae_gp_ode_amd.main import FLAGS, make_parser
    assert len(FLAGS) == 39
    argv = ['--data_root', 'data/', '--task', 'mnist', '--mask', 'True', '--value', '3', '--data_seqlen', '100', '--batch', '20', '--T', '16',
            '--Ndata', '360', '--Ntest', '40', '--rotrand', 'True', '--latent_dim', '6', '--n_filt', '8', '--frames', '5', '--pretrained', 'False',
            '--vae_path', 'x', '--kernel', 'RBF', '--num_features', '256', '--num_inducing', '100', '--dimwise', 'True', '--variance', '0.7',
            '--lengthscale', '2.0', '--q_diag', 'False', '--ode', '1', '--D_in', '6', '--D_out', '6', '--solver', 'rk4', '--ts_dense_scale', '2',
            '--use_adjoint', 'False', '--dt', '0.1', '--Nepoch', '5000', '--lr', '0.001', '--eval_sample_size', '128', '--save', 'results/mnist',
            '--seed', '121', '--log_freq', '5', '--device', 'cuda:0', '--continue_training', 'False', '--model_path', 'results/mnist_x', '--Troll', '2']
    assert len(argv) == 2 * 39 and {a[2:] for a in argv[::2]} == {f[0] for f in FLAGS}
    a = make_parser().parse_args(argv)
    assert a.eval_sample_size == 128 and a.Troll == 2 and a.model_path == 'results/mnist_x'


def test_cli_refuses_more_than_one_rank(monkeypatch):
    from vae_gp_ode_amd import evaluate
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit) as e:
        evaluate.main(['--task', 'synthetic'])
    assert 'single-process' in str(e.value) and 'not built' in str(e.value)


@pytest.mark.parametrize('name', EVAL_CASES)
def test_eval_fixtures_are_consistent(name):
    """What the fixture says about itself: its own mse / std / mse_t are the reductions of its own Xrec against its own targets,
    its predictive moments are those of Xrec over the draws, eval() moved the running statistics off (0, 1), and it carries the
    signal the generator promises (peak predictive variance >= 1e-3, span >= 0.1)."""
    g = load_golden(name)
    X, Xrec = g['X'], g['Xrec']
    L, N, Th = Xrec.shape[:3]
    T = X.shape[1]
    assert (L, N, T) == (3, 2, 6) and Th == (12 if name.endswith('_roll') else 6) and tuple(g['ztL'].shape[:3]) == (L, N, Th)
    for tag, tgt, rec in (('', X, Xrec), ('01', g['X01'], Xrec), ('64', X.double(), g['Xrec64']), ('01_64', g['X01'].double(), g['Xrec64'])):
        se = (rec[:, :, :T] - tgt[None]) ** 2
        # the same reductions in the same precision on another CPU may sum in another order: a few units of the format's rounding
        rt = 1e-6 if rec.dtype == torch.float32 else 1e-13
        close = lambda a, b: ((a.double() - b.double()).abs().max() <= rt * b.double().abs().max()).item()
        assert close(torch.mean(se), g['mse' + tag]) and close(torch.std(se), g['std' + tag])
        assert close(se.mean(dim=(0, 1, 3, 4, 5)), g['mse_t' + tag])
        assert abs(g['mse_t' + tag].double().mean().item() - g['mse' + tag].item()) < 1e-5 * g['mse' + tag].item()
    assert (Xrec.mean(0) - g['pmean']).abs().max().item() <= 1e-6 and (Xrec.var(0) - g['pvar']).abs().max().item() <= 1e-6 * g['pvar'].max().item()
    assert g['Xrec64'].dtype == torch.float64 and g['pvar64'].dtype == torch.float64
    assert g['pvar'].max().item() >= 1e-3 and (Xrec.max() - Xrec.min()).item() >= 0.1
    assert 0.0 <= g['X01'].min().item() and g['X01'].max().item() <= 1.0
    for i in (2, 5, 8):
        rm, rv = g['sd.vae.decoder.decnn.%d.running_mean' % i], g['sd.vae.decoder.decnn.%d.running_var' % i]
        assert rm.abs().max().item() > 1e-3 and (rv - 1).abs().max().item() > 1e-3
        assert g['sd.vae.decoder.decnn.%d.num_batches_tracked' % i].item() == 3
    # the reference's own float32 result against its float64 recomputation: far inside the 2e-4 the tests start from
    assert ((Xrec.double() - g['Xrec64']).abs().max() / g['Xrec64'].abs().max()).item() < 1e-5
    assert ((g['pvar'].double() - g['pvar64']).abs().max() / g['pvar64'].max()).item() < 1e-4
    for l in range(L):
        assert {'noise%d.%s' % (l, k) for k in ('rff_w', 'rff_eps', 'rff_u', 'eps_u')} <= set(g)
