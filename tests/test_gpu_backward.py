"""GPU parity (backward): reverse sweep (dL/dz0) and parameter gradients in pack layout, against the
reference's autograd results (golden) and the oracle's fp64 autograd on the same inputs.

Tolerance: |hip - ref| <= 5e-4 + 3 |ref - fp64 twin| relative to max|ref| (gradients pass through the same
ill-conditioned nu as the forward; see tests/test_gpu_forward.py)."""
import pytest
import torch

from conftest import load_golden, sub
from oracle import gpode_oracle as O
from pack_layout import PackView, leaf_grads
from test_gpu_forward import GP_CASES, build, relerr

pytestmark = pytest.mark.gpu


def oracle_leaf_grads(g, kernel, order, method, dtype=torch.float64):
    """fp64 autograd of L = sum(zt * gw) w.r.t. z0 and the cache-level quantities treated as leaves."""
    p = O.to_dtype(O.gp_params_from_state_dict(sub(g, 'sd.')), dtype)
    c = O.build_cache(p, O.to_dtype(sub(g, 'noise.'), dtype), kernel)
    leaf = {k: c[k].detach().clone().requires_grad_(True) for k in ('omega', 'var', 'nu', 'Z', 'ell')}
    cl = dict(c, **leaf)
    if kernel == 'DF':
        leaf['B'] = O.df_B_omega(c['omega']).detach().clone().requires_grad_(True)
        cl['B'] = leaf['B']
    z0 = g['z0'].to(dtype).clone().requires_grad_(True)
    zt = O.flow_forward(z0, g['ts'].to(dtype), cl, order, method)
    (zt * g['gw'].to(dtype)).sum().backward()
    out = {k: v.grad for k, v in leaf.items()}
    out['z0'] = z0.grad
    out['cache'] = c
    return out


@pytest.mark.parametrize('name,kernel,order', GP_CASES)
@pytest.mark.parametrize('method', ['euler', 'rk4'])
def test_dz0_matches_reference(name, kernel, order, method):
    from vae_gp_ode_amd import ops
    g = load_golden(name)
    c = build(g, kernel, want_Lu=False)
    zt, xs = ops.rollout(c, g['z0'].cuda(), g['ts'].cuda(), order, method, save_stages=True)
    gz0, ast = ops.rollout_bwd(c, xs, g['gw'].cuda(), g['ts'].cuda(), order, method)
    ref = g['grad_%s.z0' % method]
    twin = oracle_leaf_grads(g, kernel, order, method)['z0']
    tol = 5e-4 + 3 * relerr(ref, twin)
    assert relerr(gz0, ref) < tol, (relerr(gz0, ref), tol)


@pytest.mark.parametrize('name,kernel,order', GP_CASES)
def test_param_grads_in_pack_layout(name, kernel, order):
    """Kernel B against the oracle's fp64 autograd with the cache quantities as leaves."""
    from vae_gp_ode_amd import ops
    g = load_golden(name)
    method = 'rk4'
    c = build(g, kernel, want_Lu=False)
    zt, xs = ops.rollout(c, g['z0'].cuda(), g['ts'].cuda(), order, method, save_stages=True)
    gz0, ast = ops.rollout_bwd(c, xs, g['gw'].cuda(), g['ts'].cuda(), order, method)
    gp = ops.param_grad(c, xs.reshape(-1, c.Di), ast.reshape(-1, c.Do), nchunk=37).cpu().double()
    gp2 = ops.param_grad(c, xs.reshape(-1, c.Di), ast.reshape(-1, c.Do), nchunk=5).cpu().double()
    pv = PackView(kernel, c.Di, c.Do, c.M, c.S)
    for view in (pv.rff, pv.ind, pv.uni):  # chunking only changes the summation order (padding lanes are not compared)
        assert relerr(view(gp2), view(gp)) < 2e-5
    tw = oracle_leaf_grads(g, kernel, order, method)
    c64 = tw['cache']
    got = leaf_grads(pv, gp, c64)
    tol = 2e-3
    assert relerr(got['omega'], tw['omega']) < tol
    if kernel == 'DF':
        ref_B = tw['B'][:c.S] + tw['B'][c.S:]                                # cos and sin halves share B
        assert relerr(got['B'], ref_B) < tol
    assert relerr(got['var'], tw['var']) < tol
    assert relerr(got['Z'], tw['Z']) < tol
    assert relerr(got['nu'], tw['nu']) < tol
    assert relerr(got['ell'], tw['ell']) < tol


def make_layer(g, kernel, order, method):
    """The mirror API on the GPU, loaded with the fixture's state_dict and primed with its noise."""
    from vae_gp_ode_amd.model.core.flow import Flow
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    sd = sub(g, 'sd.flow.odefunc.diffeq.')
    Do, Di = (sd['kern.unconstrained_lengthscales'].shape if sd['kern.unconstrained_lengthscales'].dim() == 2 else (0, 0))
    M = sd['inducing_loc.optvar'].shape[0]
    S = g['noise.rff_eps'].shape[1]
    q_diag = tuple(sd['Us_sqrt.optvar'].shape) == (M, Do) and (M, Do) != (Do, M * (M + 1) // 2)
    if sd['kern.unconstrained_lengthscales'].dim() == 1:      # dimwise=False fixture: lengthscales (D_in,), Um tells D_out
        Di, Do = sd['kern.unconstrained_lengthscales'].shape[0], sd['Um.optvar'].shape[1]
    gp = SVGP_Layer(Di, Do, M, S, q_diag=q_diag, dimwise=sd['kern.unconstrained_lengthscales'].dim() == 2, kernel=kernel).cuda()
    gp.load_state_dict(sd)
    flow = Flow(gp, order=order, solver=method).cuda()
    gp.set_noise({k: v.cuda() for k, v in sub(g, 'noise.').items()})
    return flow, gp


@pytest.mark.parametrize('name,kernel,order', GP_CASES)
@pytest.mark.parametrize('method', ['euler', 'rk4'])
def test_flow_autograd_matches_reference(name, kernel, order, method):
    """loss.backward() through the mirror's Flow.forward: every GP parameter gradient against the
    reference's autograd (golden) with the fp64-calibrated tolerance."""
    g = load_golden(name)
    flow, gp = make_layer(g, kernel, order, method)
    z0 = g['z0'].cuda().requires_grad_(True)
    zt = flow(z0, g['ts'].cuda())
    (zt * g['gw'].cuda()).sum().backward()
    # fp64 twin of the full gradient
    p64 = {k: v.double().clone().requires_grad_(True) for k, v in O.gp_params_from_state_dict(sub(g, 'sd.')).items()}
    c64 = O.build_cache(p64, O.to_dtype(sub(g, 'noise.'), torch.float64), kernel)
    z64 = g['z0'].double().clone().requires_grad_(True)
    (O.flow_forward(z64, g['ts'].double(), c64, order, method) * g['gw'].double()).sum().backward()
    gr = sub(g, 'grad_%s.' % method)
    got = {'raw_ell': gp.kern.unconstrained_lengthscales.grad, 'raw_var': gp.kern.unconstrained_variance.grad,
           'Z': gp.inducing_loc.optvar.grad, 'Um': gp.Um.optvar.grad, 'Us': gp.Us_sqrt.optvar.grad}
    worst = {}
    for short, key in O.GP_KEYS.items():
        ref = gr[key[len('flow.'):]]
        tol = 1e-3 + 3 * relerr(ref, p64[short].grad)
        err = relerr(got[short], ref)
        worst[short] = (err, tol)
        assert err < tol, (short, err, tol)
    assert relerr(z0.grad, gr['z0']) < 5e-4 + 3 * relerr(gr['z0'], z64.grad)
    print(name, method, {k: '%.1e/%.1e' % v for k, v in worst.items()})


@pytest.mark.parametrize('name,kernel,order', GP_CASES[:3])
def test_midpoint_solver_forward_and_backward(name, kernel, order):
    """'midpoint' (flow.py:76-85 hands the solver name to torchdiffeq; fixed-grid y1 = y + dt f(y + dt/2 f(y))).
    No reference fixture holds it (the integrator is restated), so the check is against the oracle:
    |hip - oracle32| <= base + 3 |oracle32 - oracle64| for the trajectory and every gradient."""
    g = load_golden(name)
    method = 'midpoint'
    flow, gp = make_layer(g, kernel, order, method)
    z0 = g['z0'].cuda().requires_grad_(True)
    zt = flow(z0, g['ts'].cuda())
    (zt * g['gw'].cuda()).sum().backward()
    assert int(flow.num_evals()) == 2 * (g['ts'].shape[0] - 1)
    res = {}
    for dt in (torch.float32, torch.float64):
        p = {k: v.to(dt).clone().requires_grad_(True) for k, v in O.gp_params_from_state_dict(sub(g, 'sd.')).items()}
        c = O.build_cache(p, O.to_dtype(sub(g, 'noise.'), dt), kernel)
        z = g['z0'].to(dt).clone().requires_grad_(True)
        out = O.flow_forward(z, g['ts'].to(dt), c, order, method)
        (out * g['gw'].to(dt)).sum().backward()
        res[dt] = dict({k: v.grad for k, v in p.items()}, z0=z.grad, zt=out.detach())
    r32, r64 = res[torch.float32], res[torch.float64]
    assert relerr(zt, r32['zt']) < 1e-4 + 3 * relerr(r32['zt'], r64['zt'])
    got = {'raw_ell': gp.kern.unconstrained_lengthscales.grad, 'raw_var': gp.kern.unconstrained_variance.grad,
           'Z': gp.inducing_loc.optvar.grad, 'Um': gp.Um.optvar.grad, 'Us': gp.Us_sqrt.optvar.grad, 'z0': z0.grad}
    for k, v in got.items():
        tol = 1e-3 + 3 * relerr(r32[k], r64[k])
        assert relerr(v, r32[k]) < tol, (k, relerr(v, r32[k]), tol)


@pytest.mark.parametrize('name,kernel', [('gp_rbf1_tiny_qdiag', 'RBF'), ('gp_df1_tiny_qdiag', 'DF')])
@pytest.mark.parametrize('method', ['euler', 'rk4'])
def test_q_diag_variant_matches_reference(name, kernel, method):
    """SVGP_Layer(q_diag=True) (svpy.py:79-82,95-96,153-167): diagonal inducing scale under a softplus.  Trajectory, KL
    and every parameter gradient (incl. the raw diagonal scale) against fixtures captured from the reference."""
    g = load_golden(name)
    flow, gp = make_layer(g, kernel, 1, method)
    assert gp.q_diag and tuple(gp.Us_sqrt.optvar.shape) == (gp.M, gp.D_out)
    z0 = g['z0'].cuda().requires_grad_(True)
    zt = flow(z0, g['ts'].cuda())
    kl = gp.kl()
    (zt * g['gw'].cuda()).sum().backward()
    p64 = {k: v.double().clone().requires_grad_(True) for k, v in O.gp_params_from_state_dict(sub(g, 'sd.')).items()}
    c64 = O.build_cache(p64, O.to_dtype(sub(g, 'noise.'), torch.float64), kernel)
    z64 = g['z0'].double().clone().requires_grad_(True)
    zt64 = O.flow_forward(z64, g['ts'].double(), c64, 1, method)
    (zt64 * g['gw'].double()).sum().backward()
    assert relerr(zt, g['zt_' + method]) < 2e-4 + 3 * relerr(g['zt_' + method], zt64)
    assert abs(kl.item() - g['kl_u'].item()) < 1e-5 * abs(g['kl_u'].item())
    gr = sub(g, 'grad_%s.' % method)
    got = {'raw_ell': gp.kern.unconstrained_lengthscales.grad, 'raw_var': gp.kern.unconstrained_variance.grad,
           'Z': gp.inducing_loc.optvar.grad, 'Um': gp.Um.optvar.grad, 'Us': gp.Us_sqrt.optvar.grad}
    for short, key in O.GP_KEYS.items():
        ref = gr[key[len('flow.'):]]
        tol = 1e-3 + 3 * relerr(ref, p64[short].grad)
        assert relerr(got[short], ref) < tol, (short, relerr(got[short], ref), tol)
    assert relerr(z0.grad, gr['z0']) < 5e-4 + 3 * relerr(gr['z0'], z64.grad)


@pytest.mark.parametrize('name,order', [('gp_rbf1_tiny_shared', 1), ('gp_rbf2_tiny_shared', 2)])
@pytest.mark.parametrize('method', ['euler', 'rk4'])
def test_shared_hyperparameter_rbf_matches_reference(name, order, method):
    """RBF(dimwise=False) (kernels.py:45-46,81-96,108-110,118-132,164-181): one lengthscale vector / variance / frequency
    set for all outputs.  Cached attributes in the reference's layouts, K, the trajectory and every gradient (the shared
    lengthscales receive the sum over outputs) against fixtures captured from the reference's non-dimwise code path."""
    g = load_golden(name)
    flow, gp = make_layer(g, 'RBF', order, method)
    k = gp.kern
    assert not k.dimwise and tuple(k.unconstrained_lengthscales.shape) == (gp.D_in,) and tuple(k.unconstrained_variance.shape) == (1,)
    z0 = g['z0'].cuda().requires_grad_(True)
    zt = flow(z0, g['ts'].cuda())
    (zt * g['gw'].cuda()).sum().backward()
    p64 = {kk: v.double().clone().requires_grad_(True) for kk, v in O.gp_params_from_state_dict(sub(g, 'sd.')).items()}
    c64 = O.build_cache(p64, O.to_dtype(sub(g, 'noise.'), torch.float64), 'RBF')
    z64 = g['z0'].double().clone().requires_grad_(True)
    zt64 = O.flow_forward(z64, g['ts'].double(), c64, order, method)
    (zt64 * g['gw'].double()).sum().backward()
    assert tuple(k.rff_omega.shape) == tuple(g['omega'].shape) and relerr(k.rff_omega, g['omega']) < 1e-6
    assert tuple(k.rff_phase.shape) == tuple(g['phase'].shape) and relerr(k.rff_phase, g['phase']) < 1e-6
    assert tuple(k.nu.shape) == tuple(g['nu'].shape)
    assert relerr(k.nu, g['nu']) < 2e-4 + 3 * relerr(g['nu'], c64['nu'].squeeze(2).T)
    Z = gp.inducing_loc.optvar.detach()
    assert relerr(k.K(Z), g['Ku']) < 1e-5 and relerr(k.K(Z, g['x'].cuda()), g['Kzx']) < 1e-5
    assert relerr(zt, g['zt_' + method]) < 2e-4 + 3 * relerr(g['zt_' + method], zt64)
    gr = sub(g, 'grad_%s.' % method)
    got = {'raw_ell': k.unconstrained_lengthscales.grad, 'raw_var': k.unconstrained_variance.grad,
           'Z': gp.inducing_loc.optvar.grad, 'Um': gp.Um.optvar.grad, 'Us': gp.Us_sqrt.optvar.grad}
    for short, key in O.GP_KEYS.items():
        ref = gr[key[len('flow.'):]]
        tol = 1e-3 + 3 * relerr(ref, p64[short].grad)
        assert relerr(got[short], ref) < tol, (short, relerr(got[short], ref), tol)
    assert relerr(z0.grad, gr['z0']) < 5e-4 + 3 * relerr(gr['z0'], z64.grad)


def synthetic_gp(kernel, Di, Do, M, S, N, T, seed):
    """Seeded parameters + noise in the oracle's naming (no fixture exists past the reference's CPU-runnable shapes)."""
    g = torch.Generator().manual_seed(seed)
    p = dict(raw_ell=O.invsoftplus(2.0 * (1 + 0.05 * torch.rand(Do, Di, generator=g))), raw_var=O.invsoftplus(torch.ones(Do)),
             Z=torch.randn(M, Di, generator=g) * 2.0, Um=torch.randn(M, Do, generator=g) * 0.1,
             Us=torch.zeros(Do, M * (M + 1) // 2))
    p['Us'][:, torch.tensor([n * (n + 1) // 2 + n for n in range(M)])] = 1e-2
    p['Us'] += 1e-3 * torch.randn(p['Us'].shape, generator=g) * (p['Us'] == 0)
    if kernel == 'DF':
        nz = dict(rff_w=torch.randn(2 * S, Do, generator=g), rff_eps=torch.randn(Di, S, Do, generator=g),
                  rff_u=torch.rand(1, S, Do, generator=g), eps_u=torch.randn(M, Do, generator=g))
    else:
        nz = dict(rff_w=torch.randn(S, Do, generator=g), rff_eps=torch.randn(Di, S, Do, generator=g),
                  rff_u=torch.rand(1, S, Do, generator=g), eps_u=torch.randn(M, Do, generator=g))
    return p, nz, torch.randn(N, Di, generator=g), 0.1 * torch.arange(T, dtype=torch.float), torch.randn(N, T, Di, generator=g)


STREAM_CASES = [                                   # shapes past the register-resident team mapping (S <= 256, M <= 128, D <= 8)
    ('DF', 6, 6, 1, 160, 64, 'rk4'),              # M > 128
    ('DF', 6, 6, 1, 48, 320, 'rk4'),              # S > 256
    ('DF', 16, 16, 1, 72, 96, 'rk4'),             # BASELINE configs[4]'s latent width
    ('DF', 16, 16, 1, 24, 64, 'midpoint'),
    ('DF', 16, 16, 1, 66, 64, 'euler'),           # n = 1056: the last 128-row tile of the big-factor kernels is partial
    ('RBF', 6, 6, 1, 200, 320, 'rk4'),
    ('RBF', 6, 3, 2, 136, 64, 'euler'),
    ('RBF', 16, 16, 1, 40, 64, 'rk4'),
    ('RBF', 16, 8, 2, 40, 64, 'rk4'),
    ('RBF', 8, 8, 1, 1056, 64, 'euler'),          # eight batched 1056-row factors on the big-factor (panelled / matrix-core) kernels
    ('DF', 16, 16, 1, 512, 256, 'rk4'),           # BASELINE configs[4] at full width: K_uu is 8192 x 8192 (oracle: ~30 s of CPU)
    # every divergence-free width 2 .. 16 is compiled (main.py:45,77,79 take any integer): the remaining odd / in-between ones
    ('DF', 7, 7, 1, 40, 64, 'rk4'),               # register-resident team, odd width
    ('DF', 7, 7, 1, 160, 64, 'euler'),            # the same width streamed (M > 128)
    ('DF', 9, 9, 1, 24, 64, 'rk4'),               # first width past the register-resident kernels
    ('DF', 11, 11, 1, 24, 32, 'rk4'),
    ('DF', 12, 12, 1, 40, 64, 'midpoint'),
    ('DF', 13, 13, 1, 24, 64, 'euler'),
    ('DF', 14, 14, 1, 24, 32, 'rk4'),
    ('DF', 15, 15, 1, 40, 96, 'rk4'),
]


@pytest.mark.parametrize('kernel,Di,Do,order,M,S,method', STREAM_CASES)
def test_streamed_backward_matches_fp64_oracle(kernel, Di, Do, order, M, S, method):
    """loss.backward() through Flow.forward where the backward takes the STREAMED team kernels (pack read from L2 instead of
    held in registers): every gradient against the oracle's fp64 autograd on the same parameters and noise, tolerance
    calibrated by the oracle's own fp32 run."""
    from vae_gp_ode_amd.model.core.flow import Flow
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    N, T = (5, 4) if M < 512 else (4, 3)
    p, nz, z0, ts, gw = synthetic_gp(kernel, Di, Do, M, S, N, T, seed=1000 + M + S + Di)
    gp = SVGP_Layer(Di, Do, M, S, kernel=kernel).cuda()
    with torch.no_grad():
        gp.kern.unconstrained_lengthscales.copy_(p['raw_ell'])
        gp.kern.unconstrained_variance.copy_(p['raw_var'])
        gp.inducing_loc.optvar.copy_(p['Z'])
        gp.Um.optvar.copy_(p['Um'])
        gp.Us_sqrt.optvar.copy_(p['Us'])
    flow = Flow(gp, order=order, solver=method).cuda()
    gp.set_noise({k: v.cuda() for k, v in nz.items()})
    zg = z0.cuda().requires_grad_(True)
    zt = flow(zg, ts.cuda())
    (zt * gw.cuda()).sum().backward()
    got = {'raw_ell': gp.kern.unconstrained_lengthscales.grad, 'raw_var': gp.kern.unconstrained_variance.grad,
           'Z': gp.inducing_loc.optvar.grad, 'Um': gp.Um.optvar.grad, 'Us': gp.Us_sqrt.optvar.grad, 'z0': zg.grad}

    def oracle(dtype):
        q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items()}
        c = O.build_cache(q, O.to_dtype(nz, dtype), kernel)
        z = z0.to(dtype).clone().requires_grad_(True)
        out = O.flow_forward(z, ts.to(dtype), c, order, method)
        (out * gw.to(dtype)).sum().backward()
        return out.detach(), dict({k: v.grad for k, v in q.items()}, z0=z.grad)
    z64, g64 = oracle(torch.float64)
    z32, g32 = oracle(torch.float32)
    assert relerr(zt, z64) < 2e-4 + 3 * relerr(z32, z64)
    for k in got:
        tol = 1e-3 + 3 * relerr(g32[k], g64[k])
        assert relerr(got[k], g64[k]) < tol, (k, relerr(got[k], g64[k]), tol)


@pytest.mark.parametrize('M,Dd', [(1056, 3), (600, 2)])
def test_hyperparameter_gradients_on_a_rank_deficient_kuu(M, Dd):
    """Many inducing points in a low-dimensional latent: K_uu + jitter I is numerically rank deficient (what training drives the
    model towards).  The cache backward takes the solve-based route (block substitution with the factor, csrc/gp_cache_bwd.hip
    k_trsm_slab) -- the autograd of kernels.py:163-171 -- instead of products with an explicit L^-1, which at M = 1056, D = 3
    left d/d lengthscale 12 % from fp64 where torch's own fp32 solves are at 1 % (round 1, tools/ab_bigfactor.py).
    Every GP gradient must now be within 4x of the fp32 oracle's distance to the fp64 oracle (floor 2e-4); the variance
    gradient -- a small difference of two large sums at this conditioning -- within 8x (measured: d/d ell 1.3e-2 vs torch 1.1e-2,
    d/d var 3.4e-3 vs 1.4e-3 at M = 1056)."""
    kernel, Di, Do, order, S, method, N, T_ = 'RBF', Dd, Dd, 1, 64, 'euler', 5, 4
    p, nz, z0, ts, gw = synthetic_gp(kernel, Di, Do, M, S, N, T_, seed=1000 + M + S + Di)
    from vae_gp_ode_amd import ops
    from vae_gp_ode_amd.model.core.flow import Flow
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    gp = SVGP_Layer(Di, Do, M, S, kernel=kernel).cuda()
    with torch.no_grad():
        gp.kern.unconstrained_lengthscales.copy_(p['raw_ell']); gp.kern.unconstrained_variance.copy_(p['raw_var'])
        gp.inducing_loc.optvar.copy_(p['Z']); gp.Um.optvar.copy_(p['Um']); gp.Us_sqrt.optvar.copy_(p['Us'])
    flow = Flow(gp, order=order, solver=method).cuda()
    gp.set_noise({k: v.cuda() for k, v in nz.items()})
    zg = z0.cuda().requires_grad_(True)
    ops.set_backward_solves('always')                # what main.py --backward_solves adaptive selects at this conditioning
    try:
        zt = flow(zg, ts.cuda())
        lo, hi = gp.cache.pivot_range()
        assert hi / lo >= 200.0, (lo, hi)            # the adaptive rule does fire here
        (zt * gw.cuda()).sum().backward()
    finally:
        ops.set_backward_solves('auto')
    got = {'raw_ell': gp.kern.unconstrained_lengthscales.grad, 'raw_var': gp.kern.unconstrained_variance.grad,
           'Z': gp.inducing_loc.optvar.grad, 'Um': gp.Um.optvar.grad, 'Us': gp.Us_sqrt.optvar.grad, 'z0': zg.grad}

    def oracle(dtype):
        q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items()}
        c = O.build_cache(q, O.to_dtype(nz, dtype), kernel)
        z = z0.to(dtype).clone().requires_grad_(True)
        out = O.flow_forward(z, ts.to(dtype), c, order, method)
        (out * gw.to(dtype)).sum().backward()
        return dict({k: v.grad for k, v in q.items()}, z0=z.grad)
    g64, g32 = oracle(torch.float64), oracle(torch.float32)
    rep = {k: (relerr(got[k], g64[k]), relerr(g32[k], g64[k])) for k in got}
    print('M=%d D=%d  hip / fp32-oracle distance to fp64:' % (M, Dd), {k: '%.1e/%.1e' % v for k, v in rep.items()})
    for k, (e_hip, e_ref) in rep.items():
        # (4x: the fp32 oracle's own distance moves by a third with the host's thread count -- 3x sat within 2 % of failing)
        assert e_hip < max((8 if k == 'raw_var' else 4) * e_ref, 2e-4), (k, e_hip, e_ref)


@pytest.mark.parametrize('Di,Do,order,method', [(5, 5, 1, 'rk4'), (10, 10, 1, 'euler'), (10, 5, 2, 'rk4'), (7, 7, 1, 'midpoint')])
def test_rbf_widths_outside_the_compiled_list(Di, Do, order, method):
    """--latent_dim / --D_in / --D_out are free integers in the reference (main.py:45,77,79).  An RBF layer whose widths are not
    compiled (5, 7, 10 ...) is evaluated at the next compiled width on zero-padded operands (ops.WidthPad), which is the same
    arithmetic term for term: trajectories, f(x), the cached attributes' shapes and every gradient against the fp64 oracle at
    the TRUE widths, with the tolerances of the compiled widths."""
    from vae_gp_ode_amd import _lib
    from vae_gp_ode_amd.model.core.flow import Flow
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    assert not _lib.load().gpode_supported(0, Di, Do)
    M, S, N, T_ = 40, 96, 6, 5
    p, nz, z0, ts, gw = synthetic_gp('RBF', Di, Do, M, S, N, T_, seed=31 * Di + Do)
    gp = SVGP_Layer(Di, Do, M, S, kernel='RBF').cuda()
    with torch.no_grad():
        gp.kern.unconstrained_lengthscales.copy_(p['raw_ell']); gp.kern.unconstrained_variance.copy_(p['raw_var'])
        gp.inducing_loc.optvar.copy_(p['Z']); gp.Um.optvar.copy_(p['Um']); gp.Us_sqrt.optvar.copy_(p['Us'])
    flow = Flow(gp, order=order, solver=method).cuda()
    gp.set_noise({k: v.cuda() for k, v in nz.items()})
    zg = z0.cuda().requires_grad_(True)
    zt = flow(zg, ts.cuda())
    assert tuple(zt.shape) == (N, T_, Di)
    (zt * gw.cuda()).sum().backward()
    k = gp.kern
    assert tuple(k.rff_omega.shape) == (Di, S, Do) and tuple(k.nu.shape) == (Do, M, 1) and tuple(k.rff_phase.shape) == (1, S, Do)
    p64 = {kk: v.double().clone().requires_grad_(True) for kk, v in p.items()}
    c64 = O.build_cache(p64, O.to_dtype(nz, torch.float64), 'RBF')
    z64 = z0.double().clone().requires_grad_(True)
    zt64 = O.flow_forward(z64, ts.double(), c64, order, method)
    (zt64 * gw.double()).sum().backward()
    p32 = {kk: v.clone().requires_grad_(True) for kk, v in p.items()}
    z32 = z0.clone().requires_grad_(True)
    zt32 = O.flow_forward(z32, ts, O.build_cache(p32, nz, 'RBF'), order, method)
    (zt32 * gw).sum().backward()
    assert relerr(zt, zt64) < 2e-4 + 3 * relerr(zt32, zt64)
    x = z0.cuda()
    assert relerr(gp(x), O.gp_forward(z0.double(), c64)) < 2e-4 + 3 * relerr(O.gp_forward(z0, O.build_cache(p, nz, 'RBF')), O.gp_forward(z0.double(), c64))
    assert relerr(k.nu, c64['nu']) < 2e-4 + 3 * relerr(O.build_cache(p, nz, 'RBF')['nu'], c64['nu'])
    got = {'raw_ell': k.unconstrained_lengthscales.grad, 'raw_var': k.unconstrained_variance.grad, 'Z': gp.inducing_loc.optvar.grad,
           'Um': gp.Um.optvar.grad, 'Us': gp.Us_sqrt.optvar.grad}
    for kk in got:
        assert tuple(got[kk].shape) == tuple(p[kk].shape)
        tol = 1e-3 + 3 * relerr(p32[kk].grad, p64[kk].grad)
        assert relerr(got[kk], p64[kk].grad) < tol, (kk, relerr(got[kk], p64[kk].grad), tol)
    assert relerr(zg.grad, z64.grad) < 5e-4 + 3 * relerr(z32.grad, z64.grad)


def test_df_width_outside_the_compiled_list_is_refused_loudly():
    """Every divergence-free width 2 .. 16 is compiled (fixtures at 5 and 10, the others in STREAM_CASES); past 16 the layer says so
    instead of evaluating something else (the DF kernel cannot be zero-padded: it carries the width itself)."""
    from vae_gp_ode_amd import _lib
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    assert all(_lib.load().gpode_supported(1, d, d) for d in range(2, 17))
    gp = SVGP_Layer(17, 17, 8, 16, kernel='DF').cuda()
    with pytest.raises(_lib.GpodeError, match='divergence-free kernel is compiled for D = 2 .. 16'):
        gp.build_cache()


def test_side_stream_parameter_gradient_does_not_depend_on_the_main_stream():
    """ops.param_grad under launch_on(side) while the main stream is held up behind the fork: everything that writes its
    result must run on the side stream.  (A torch-native fill of the result buffer launches on torch's CURRENT stream; queued
    behind a busy main stream it used to land after the side-stream reduction had written the buffer and wipe it -- seen as a
    run-to-run wobble of the GP parameter gradients in overlap / HIP-graph mode.)"""
    from vae_gp_ode_amd import ops
    name, kernel, order = GP_CASES[0]
    g = load_golden(name)
    c = build(g, kernel, want_Lu=False)
    zt, xs = ops.rollout(c, g['z0'].cuda(), g['ts'].cuda(), order, 'rk4', save_stages=True)
    gz0, ast = ops.rollout_bwd(c, xs, g['gw'].cuda(), g['ts'].cuda(), order, 'rk4')
    x, a = xs.reshape(-1, c.Di), ast.reshape(-1, c.Do)
    ref = ops.param_grad(c, x, a).clone()
    torch.cuda.synchronize()
    side = ops.fork_side_stream()
    torch.cuda._sleep(int(2e8))                      # ~0.1 s of main-stream work queued behind the fork point
    keep = []
    with ops.launch_on(side):
        got = ops.param_grad(c, x, a, keep=keep)
    ops.join_side_stream()
    torch.cuda.synchronize()
    pv = PackView(kernel, c.Di, c.Do, c.M, c.S)
    for view in (pv.rff, pv.ind, pv.uni):
        assert torch.equal(view(got.cpu().double()), view(ref.cpu().double()))
