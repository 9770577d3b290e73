"""GPU: the layers above the tangent-linear rollout -- Flow.sensitivity, evaluate.flow_diagnostics and --eval_flow -- on the tiny RBF and
DF models of tests/test_gpu_eval.py.  The kernels themselves are held to the oracle in tests/test_gpu_tangent.py; here the layers are
held to the operation underneath (bits) and to their own host reductions."""
import json
import os

import pytest
import torch

from test_gpu_eval import L_FIX, make_model, queue_fixture_noise

pytestmark = pytest.mark.gpu

MODELS = [('eval_rbf1', dict()), ('eval_df1', dict(kernel='DF')), ('eval_rbf2', dict(ode=2, D_in=6, D_out=3, latent_dim=3))]
KEYS = ('flow_logdet_mean', 'flow_logdet_absmax', 'flow_ftle_mean', 'flow_ftle_max', 'flow_div_absmean', 'flow_div_absmean_meanfield')
FILES = ['flow_%s%s.npy' % (n, s) for s in ('', '_mean') for n in ('phi', 'logdet', 'div')]


@pytest.fixture(scope='module', autouse=True)
def leave_the_global_generators_as_found():
    import random
    import numpy as np
    saved = (torch.get_rng_state(), torch.cuda.get_rng_state_all(), np.random.get_state(), random.getstate())
    yield
    torch.set_rng_state(saved[0])
    torch.cuda.set_rng_state_all(saved[1])
    np.random.set_state(saved[2])
    random.setstate(saved[3])


@pytest.mark.parametrize('name,kw', MODELS, ids=[m[0] for m in MODELS])
def test_sensitivity_is_rollout_jvp(name, kw):
    from vae_gp_ode_amd import _lib, ops
    m, g = make_model(name, kw)
    flow, gp = m.flow, m.flow.odefunc.diffeq
    D, order = gp.D_in, m.order
    gen = torch.Generator().manual_seed(3)
    z0, ts = torch.randn(4, D, generator=gen).cuda(), torch.tensor([0.0, 0.1, 0.25, 0.3]).cuda()
    for sub in (1, 2):
        flow.substeps = sub
        queue_fixture_noise(m, g)
        zt, Phi = flow.sensitivity(z0, ts)                                       # one fresh draw: the first queued noise
        assert _lib.load().gpode_last_launch().decode() == 'rollout_jvp_%s_stream' % gp.kernel_n.lower()
        zr, vr = ops.rollout_jvp(gp.cache, z0, ts, order, flow.solver, substeps=sub)
        assert zt.shape == (4, 4, D) and Phi.shape == (4, 4, D, D)
        assert torch.equal(zt, zr) and torch.equal(Phi, vr.transpose(-1, -2))
        assert torch.equal(Phi[:, 0], torch.eye(D, device='cuda').expand(4, D, D))
        # explicit directions, and the draws of a batched build
        v0 = torch.randn(4, 2, D, generator=gen).cuda()
        _, vt = flow.sensitivity(z0, ts, v0=v0, cache=gp.cache)
        assert torch.equal(vt, ops.rollout_jvp(gp.cache, z0, ts, order, flow.solver, v0=v0, substeps=sub)[1])
        ztL, PhiL = flow.sensitivity(z0, ts, draws=2)                            # the next two queued noises, one build
        assert ztL.shape == (2, 4, 4, D) and PhiL.shape == (2, 4, 4, D, D) and gp.cache.stacked
    flow.solver = 'dopri5'
    with pytest.raises(ValueError, match='controller'):
        flow.sensitivity(z0, ts)


@pytest.mark.parametrize('name,kw', MODELS, ids=[m[0] for m in MODELS])
def test_flow_diagnostics_shapes_and_reductions(name, kw):
    from vae_gp_ode_amd import evaluate as E
    m, g = make_model(name, kw)
    gp = m.flow.odefunc.diffeq
    D = gp.D_in
    X = g['X'].cuda()
    N, T = X.shape[:2]
    queue_fixture_noise(m, g)
    d = E.flow_diagnostics(m, X, L=L_FIX)
    ts = m.dt * torch.arange(T, dtype=torch.float32)
    _, var0 = E.initial_state_moments(m, X)
    for L, d in ((L_FIX, d), (1, E.flow_diagnostics(m, X, mean_field=True)), (1, E.flow_diagnostics(m, X, L=1, ts=ts.cuda().expand(N, T).contiguous()))):
        assert d['zt'].shape == (L, N, T, D) and d['Phi'].shape == (L, N, T, D, D)
        assert d['logdet'].shape == (L, N, T) and d['ftle'].shape == (L, N) and d['div'].shape == (L, N, T) and d['z_var_lin'].shape == (L, N, T, D)
        assert all(d[k].dtype == torch.float64 and d[k].device.type == 'cpu' for k in ('logdet', 'ftle', 'div', 'z_var_lin'))
        assert torch.equal(d['logdet'], E.flow_logdet(d['Phi'])) and torch.equal(d['ftle'], E.flow_ftle(d['Phi'], ts))
        assert torch.equal(d['z_var_lin'], E.flow_var_lin(d['Phi'], var0))
        assert all(torch.isfinite(d[k]).all() for k in d)
        assert d['logdet'][:, :, 0].abs().max() == 0 and torch.equal(d['z_var_lin'][:, :, 0], var0.double().cpu().expand(L, N, D))
        assert torch.equal(d['zt'][:, :, 0], E.initial_state_means(m, X).expand(L, N, D))


def _checkpoint(tmp_path, common):
    """a checkpoint of an untrained model set up the way the command line sets it up"""
    from vae_gp_ode_amd import evaluate as E
    from vae_gp_ode_amd.model.core.initialization import initialize_and_fix_kernel_parameters
    from vae_gp_ode_amd.model.create_model import build_model
    from vae_gp_ode_amd.model.misc.torch_utils import seed_everything
    args = E.make_parser().parse_args(common)
    seed_everything(args.seed)
    args.device = torch.device('cuda')
    model = build_model(args).to(args.device)
    model = initialize_and_fix_kernel_parameters(model, lengthscale_value=args.lengthscale, variance_value=args.variance, fix=False)
    os.makedirs(tmp_path / 'ck', exist_ok=True)
    torch.save(model.state_dict(), tmp_path / 'ck' / 'odegpvae_mnist.pth')
    return str(tmp_path / 'ck')


def test_cli_eval_flow(tmp_path, monkeypatch):
    import numpy as np
    from vae_gp_ode_amd import evaluate as E
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    common = ['--task', 'synthetic', '--Ndata', '8', '--Ntest', '6', '--batch', '4', '--T', '6', '--solver', 'rk4', '--num_inducing', '16',
              '--num_features', '32', '--kernel', 'DF']
    argv = common + ['--model_path', _checkpoint(tmp_path, common), '--eval_sample_size', '3', '--Troll', '2', '--device_noise', 'True']
    on = E.main(argv + ['--save', str(tmp_path / 'on'), '--eval_flow', 'True'])
    assert json.load(open(tmp_path / 'on' / 'eval.json')) == on
    assert all(k in on and np.isfinite(on[k]) for k in KEYS)
    assert sorted(os.listdir(tmp_path / 'on')) == sorted(['eval.json', 'rollout_mean.npy', 'rollout_var.npy'] + FILES)
    phi, ld, dv = (np.load(tmp_path / 'on' / ('flow_%s.npy' % k)) for k in ('phi', 'logdet', 'div'))
    assert phi.shape == (3, 6, 6, 6, 6) and ld.shape == dv.shape == (3, 6, 6)
    phim, ldm, dvm = (np.load(tmp_path / 'on' / ('flow_%s_mean.npy' % k)) for k in ('phi', 'logdet', 'div'))
    assert phim.shape == (1, 6, 6, 6, 6) and ldm.shape == dvm.shape == (1, 6, 6)
    assert on['flow_logdet_mean'] == float(ld[..., -1].mean()) and on['flow_logdet_absmax'] == float(np.abs(ld).max())
    assert on['flow_div_absmean'] == float(np.abs(dv).mean()) and on['flow_div_absmean_meanfield'] == float(np.abs(dvm).mean())
    assert on['flow_ftle_max'] >= on['flow_ftle_mean']
    # switched off (the default): the figures, the keys and the files of a command line that never heard of the switch
    off = E.main(argv + ['--save', str(tmp_path / 'off')])
    assert not [k for k in off if k.startswith('flow_')]
    assert sorted(k for k in on if not k.startswith('flow_')) == sorted(off)
    assert sorted(os.listdir(tmp_path / 'off')) == ['eval.json', 'rollout_mean.npy', 'rollout_var.npy']
    assert all(on[k] == off[k] for k in ('mse', 'std', 'nll', 'nlpd', 'count', 'sequences', 'mse_t', 'nll_t', 'rollout_mse'))
    assert np.array_equal(np.load(tmp_path / 'on' / 'rollout_mean.npy'), np.load(tmp_path / 'off' / 'rollout_mean.npy'))
    with pytest.raises(SystemExit, match='dopri5'):
        E.main([a if a != 'rk4' else 'dopri5' for a in argv] + ['--save', str(tmp_path / 'no'), '--eval_flow', 'True'])
    assert not os.path.exists(tmp_path / 'no')
