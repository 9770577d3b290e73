"""GPU: the dense-output mode of the adaptive Dormand-Prince solver -- rollout (gpode_rollout_dense_fwd_n), reverse sweep
(gpode_rollout_dense_bwd_n) and the surface above them -- against tests/dopri5_dense_ref.py on the oracle's right-hand side.

Inputs: the fixtures' own z0 on two grids, G1 = 0.1 arange(16) (the reference's training grid: the controller's steps span several
outputs) and G2 = dopri5_ref.case_ts (stretched, non-uniform: steps without an output), at rtol = atol = 1e-3 and 1e-5, with
max_steps = 32 on G2 (tests/test_dopri5_dense_host.py proves on the CPU that these inputs exercise the feature).

What is compared with what: as in tests/test_gpu_dopri5.py the kernel's result is never compared with another SOLVE, but with a
REPLAY of its own record (hstep, istep, theta), and the choice of the steps is checked on its own.
Bounds: trajectories 2e-4 + 3 relerr(fp32 replay, fp64 replay); dL/dz0 and dL/df 5e-4 + 3 relerr(fp32, fp64); parameter gradients
1e-3 + 3 relerr(fp32, fp64)."""
import copy
import types

import pytest
import torch

import dopri5_dense_ref as DR
import dopri5_ref as R
from conftest import load_golden, sub
from oracle import gpode_oracle as O
from test_gpu_forward import build, relerr

pytestmark = pytest.mark.gpu

_RUNS, _TRUTH = {}, {}
EPS = torch.finfo(torch.float32).eps


def budget(which):
    return None if which == 'G1' else 32


def run(name, kernel, order, tol, which):
    """The kernel's dense solve of one case (with the record), computed once and shared -- nobody writes to it."""
    from vae_gp_ode_amd import ops
    key = (name, tol, which)
    if key not in _RUNS:
        g = load_golden(name)
        c = build(g, kernel, want_Lu=False)
        ts = DR.grid(name, which)
        zt, cnt, xs, hs, ie, th = ops.rollout_adaptive(c, g['z0'].cuda(), ts.cuda(), order, tol, tol, max_steps=budget(which), save_stages=True,
                                                       dense=True)
        _RUNS[key] = types.SimpleNamespace(g=g, c=c, ts=ts, zt=zt.cpu(), cnt=cnt.cpu().long(), xs=xs.cpu(), hs=hs.cpu(), ie=ie.cpu().long(),
                                           th=th.cpu(), K=hs.shape[-1], used=max(int(cnt[:, 0].max()), 1))
    return _RUNS[key]


def truth(name, kernel, order, which):
    """fp64 rk4 with 64 sub-steps per interval, computed once per case and grid."""
    if (name, which) not in _TRUTH:
        g, f64 = R.oracle_rhs(name, kernel, order)
        ts = DR.grid(name, which)
        fine = torch.cat([ts[i].double() + (ts[i + 1] - ts[i]).double() * torch.arange(64, dtype=torch.float64) / 64 for i in range(len(ts) - 1)]
                         + [ts[-1:].double()])
        _TRUTH[name, which] = O.odeint_fixed(f64, g['z0'].double(), fine, 'rk4')[::64].permute(1, 0, 2)
    return _TRUTH[name, which]


def recorded(zt):
    """(xstage, hstep, istep, theta) the forward behind ``zt`` saved for its backward (the autograd node of ops._Flow)"""
    fn = zt.grad_fn
    while '_Flow' not in type(fn).__name__:
        fn = fn.next_functions[0][0]
    saved = fn.saved_tensors
    return saved[1], saved[5], saved[6], saved[7]


def held(ie, K):
    """(N,K): outputs per accepted step"""
    return torch.stack([(ie == i + 1).sum(1) for i in range(K)], 1)


GRID_CASES = [(n, k, o, w) for (n, k, o) in R.CASES for w in DR.GRIDS]


# ---- 1. forward against a replay of the record -------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel,order,which', GRID_CASES)
@pytest.mark.parametrize('tol', R.TOLS)
def test_trajectories_equal_a_replay_of_the_record(name, kernel, order, which, tol):
    r = run(name, kernel, order, tol, which)
    g, f64 = R.oracle_rhs(name, kernel, order)
    _, f32 = R.oracle_rhs(name, kernel, order, torch.float32)
    N, T = r.zt.shape[:2]
    u = r.used
    assert (r.cnt[:, 2] == 0).all(), r.cnt
    aux = {}
    z64 = DR.replay_dense(f64, g['z0'].double(), r.hs[:, :u].double(), r.ie, r.th.double(), aux)
    z32 = DR.replay_dense(f32, g['z0'], r.hs[:, :u], r.ie, r.th)
    e, bound = relerr(r.zt, z64), 2e-4 + 3 * relerr(z32, z64)
    print('%s %s tol %g: |hip - replay64| %.2e  bound %.2e  steps %s rejected %s  outputs per step up to %d'
          % (name, which, tol, e, bound, r.cnt[:, 0].tolist(), r.cnt[:, 1].tolist(), held(r.ie, u).max()))
    assert e < bound
    assert torch.equal(r.zt[:, 0], g['z0'])
    # the last output is the end state of the last step: row 6 of that step's record
    last = r.xs[torch.arange(N), r.cnt[:, 0] - 1, 6]
    assert torch.equal(r.zt[:, -1], last)
    # the record
    span = (r.ts[-1] - r.ts[0]).double().item()
    for n in range(N):
        k = int(r.cnt[n, 0])
        assert abs(r.hs[n].double().sum().item() - span) <= 4 * EPS * k * span, (n, r.hs[n].double().sum().item(), span)
        assert (r.hs[n, :k] > 0).all() and (r.hs[n, k:] == 0).all() and (r.xs[n, k:] == 0).all()
    assert (torch.diff(r.ie, dim=1) >= 0).all() and (r.ie[:, 0] >= 1).all() and (r.ie[:, -1] == r.cnt[:, 0]).all() and (r.ie <= r.K).all()
    assert (r.th > 0).all() and (r.th <= 1).all() and (r.th[:, -1] == 1).all()
    assert torch.equal(r.xs[:, 0, 0], g['z0'])
    # the recorded stage inputs, the end state (row 6) included, are those of the replay
    xs64 = torch.stack([torch.stack(x, 1) for x in aux['xs']], 1)           # (N,u,7,D)
    live = (torch.arange(u)[None] < r.cnt[:, :1])[:, :, None, None]
    assert tuple(r.xs.shape[1:3]) == (r.K, 7)
    assert relerr(r.xs[:, :u] * live, xs64 * live) < bound
    assert relerr((r.xs[:, :u] * live)[:, :, 6], (xs64 * live)[:, :, 6]) < bound


# ---- 2. the controller ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel,order,which', GRID_CASES)
@pytest.mark.parametrize('tol', R.TOLS)
def test_every_accepted_step_passes_the_error_test_in_fp64(name, kernel, order, which, tol):
    r = run(name, kernel, order, tol, which)
    _, f64 = R.oracle_rhs(name, kernel, order)
    live = torch.arange(r.K)[None] < r.cnt[:, :1]
    y = r.xs[:, :, 0][live].double()                                         # (rows, D): where each accepted step started
    h = r.hs[live].double().unsqueeze(1)
    ynew, err, _, _ = R.step(f64, y, h)
    ratio = ((err / (tol + tol * torch.maximum(y.abs(), ynew.abs()))) ** 2).mean(1).sqrt()
    print('%s %s tol %g: largest fp64 error ratio of an accepted step %.4f; accepted %s rejected %s'
          % (name, which, tol, ratio.max(), r.cnt[:, 0].tolist(), r.cnt[:, 1].tolist()))
    assert ratio.max() <= 1.01          # fp32 rounding of the error estimate (see tests/test_gpu_dopri5.py)
    assert (r.cnt[:, 3] == 1 + 6 * (r.cnt[:, 0] + r.cnt[:, 1])).all()
    if which == 'G1' and tol == 1e-3:
        assert (r.cnt[:, 0] < r.ts.shape[0] - 1).all(), r.cnt[:, 0]


def test_the_cases_together_show_rejections_and_both_kinds_of_step():
    rej = shared = empty = 0
    for name, kernel, order, which in GRID_CASES:
        for tol in R.TOLS:
            r = run(name, kernel, order, tol, which)
            h = held(r.ie, r.K)
            live = torch.arange(r.K)[None] < r.cnt[:, :1]
            rej += int(r.cnt[:, 1].sum())
            shared += int((h >= 2).sum())
            empty += int((h[live] == 0).sum())
    print('rejections %d, steps with several outputs %d, accepted steps without an output %d' % (rej, shared, empty))
    assert rej >= 1 and shared >= 1 and empty >= 1


# ---- 3. accuracy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel,order,which', GRID_CASES)
def test_global_error_follows_the_tolerance(name, kernel, order, which):
    """Against fp64 rk4 with 64 sub-steps per interval: the kernel's error is at most twice the error of the fp64 reference solve
    (dopri5_dense_ref.solve_dense) at the same tolerances (+ 1e-5), a tighter tolerance gives a smaller error and costs no fewer
    evaluations.  Measured on MI355X on G1, (kernel, reference solve) at 1e-3 | 1e-5:
    rbf1_tiny (1.47e-3, 1.47e-3) | (8.89e-6, 6.70e-6);  rbf2_tiny (2.21e-3, 2.00e-3) | (3.47e-5, 3.15e-5);
    df1_tiny (2.38e-2, 2.37e-2) | (6.89e-5, 6.31e-5);  df1_tiny_q5 (2.04e-3, 2.04e-3) | (1.48e-5, 1.67e-5);
    evaluations summed over the trajectories 64 | 106, 76 | 124, 154 | 316, 131 | 215 (landing mode on G1: 364 .. 485)."""
    g, f64 = R.oracle_rhs(name, kernel, order)
    ts = DR.grid(name, which)
    tr = truth(name, kernel, order, which)
    errs, evals = [], []
    for tol in R.TOLS:
        r = run(name, kernel, order, tol, which)
        ref = DR.solve_dense(f64, g['z0'].double(), ts, tol, tol, max_steps=budget(which))[0]
        e_hip, e_ref = relerr(r.zt, tr), relerr(ref, tr)
        print('%s %s tol %g: |hip - truth| %.2e  |fp64 solve - truth| %.2e  evaluations %d' % (name, which, tol, e_hip, e_ref, r.cnt[:, 3].sum()))
        assert e_hip <= 2 * e_ref + 1e-5
        errs.append(e_hip); evals.append(int(r.cnt[:, 3].sum()))
    assert errs[1] < errs[0] and evals[1] >= evals[0]


# ---- 4. reverse sweep ----------------------------------------------------------------------------------------------------------------
def replay_grads(name, kernel, order, r, gw, dtype):
    """autograd through the replay of the record: dL/dz0, dL/df at every recorded evaluation (N,used,7,Do), L = sum(zt gw)"""
    _, f = R.oracle_rhs(name, kernel, order, dtype)
    z0 = r.g['z0'].to(dtype).clone().requires_grad_(True)
    aux = {}
    zt = DR.replay_dense(f, z0, r.hs[:, :r.used].to(dtype), r.ie, r.th.to(dtype), aux)
    ks = [k for step in aux['ks'] for k in step]
    grads = torch.autograd.grad((zt * gw.to(dtype)).sum(), [z0] + ks, allow_unused=True)
    Do = r.c.Do
    gk = torch.stack([torch.zeros_like(z0) if x is None else x for x in grads[1:]], 1).view(z0.shape[0], r.used, 7, -1)[..., -Do:]
    return grads[0], gk


@pytest.mark.parametrize('name,kernel,order,which', GRID_CASES)
def test_reverse_sweep_matches_autograd_through_the_replay(name, kernel, order, which):
    from vae_gp_ode_amd import ops
    r = run(name, kernel, order, 1e-3, which)
    gw = torch.randn(r.zt.shape, generator=torch.Generator().manual_seed(11))
    args = (r.c, r.xs.cuda(), r.hs.cuda(), r.ie.int().cuda(), gw.cuda(), order)
    gz0, ast = ops.rollout_adaptive_bwd(*args, theta=r.th.cuda())
    assert tuple(ast.shape) == (r.zt.shape[0], r.K, 7, r.c.Do)
    (z64, a64), (z32, a32) = replay_grads(name, kernel, order, r, gw, torch.float64), replay_grads(name, kernel, order, r, gw, torch.float32)
    for what, got, ref, twin in (('dL/dz0', gz0, z64, z32), ('dL/df', ast[:, :r.used], a64, a32)):
        e, bound = relerr(got, ref), 5e-4 + 3 * relerr(twin, ref)
        print('%s %s %s: %.2e  bound %.2e' % (name, which, what, e, bound))
        assert e < bound
    ast = ast.cpu()
    live = (torch.arange(r.K)[None] < r.cnt[:, :1])
    assert (ast[~live] == 0).all()
    # row 6 (the seventh slope) only where the step holds an output with theta < 1
    interior = torch.stack([((r.ie == i + 1) & (r.th < 1)).any(1) for i in range(r.K)], 1)
    assert (ast[:, :, 6][~interior] == 0).all() and (ast[:, :, 6][interior].abs().amax(-1) > 0).all()
    assert interior.any() and (which == 'G1' or (~interior & live).any())
    gz0b, astb = ops.rollout_adaptive_bwd(*args, theta=r.th.cuda())
    assert torch.equal(gz0, gz0b) and torch.equal(ast, astb.cpu())


# ---- 5. loss.backward() through Flow ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel,order,which', GRID_CASES)
def test_flow_parameter_gradients(name, kernel, order, which):
    """loss.backward() through Flow(solver='dopri5', dense_output=True): the five GP parameter gradients and dL/dz0 against fp64
    autograd through the cache build and the replay of the record this very solve wrote; then the same with the side-stream overlap
    on."""
    from test_gpu_backward import make_layer
    from vae_gp_ode_amd import ops
    g = load_golden(name)
    ts = DR.grid(name, which)
    gw = torch.randn(g['z0'].shape[0], ts.shape[0], g['z0'].shape[1], generator=torch.Generator().manual_seed(12))
    flow, gp = make_layer(g, kernel, order, 'dopri5')
    flow.rtol = flow.atol = 1e-3
    flow.dense_output, flow.max_steps = True, budget(which)
    names = {'raw_ell': gp.kern.unconstrained_lengthscales, 'raw_var': gp.kern.unconstrained_variance, 'Z': gp.inducing_loc.optvar,
             'Um': gp.Um.optvar, 'Us': gp.Us_sqrt.optvar}
    ref = None
    for overlap in (False, True):
        ops.set_overlap(overlap)
        try:
            gp.set_noise({k: v.cuda() for k, v in sub(g, 'noise.').items()})
            for p in names.values():
                p.grad = None
            z0 = g['z0'].cuda().requires_grad_(True)
            zt = flow(z0, ts.cuda())
            xs, hs, ie, th = recorded(zt)
            assert xs.shape[-2] == 7 and th is not None
            hs, ie, th = hs.cpu(), ie.cpu().long(), th.cpu()
            (zt * gw.cuda()).sum().backward()
            ops.join_side_stream()
            torch.cuda.synchronize()
        finally:
            ops.set_overlap(False)
        got = dict({k: p.grad.clone() for k, p in names.items()}, z0=z0.grad)
        cnt = flow.last_counts.cpu()
        assert (cnt[:, 2] == 0).all()
        u = int(cnt[:, 0].max())
        if ref is None:
            ref = {}
            for dtype in (torch.float64, torch.float32):
                p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in O.gp_params_from_state_dict(sub(g, 'sd.')).items()}
                c = O.build_cache(p, O.to_dtype(sub(g, 'noise.'), dtype), kernel)
                z = g['z0'].to(dtype).clone().requires_grad_(True)
                out = DR.replay_dense(lambda y: O.ode_rhs(y, c, order), z, hs[:, :u].to(dtype), ie, th.to(dtype))
                (out * gw.to(dtype)).sum().backward()
                ref[dtype] = dict({k: v.grad for k, v in p.items()}, z0=z.grad)
        for k in got:
            e, bound = relerr(got[k], ref[torch.float64][k]), (5e-4 if k == 'z0' else 1e-3) + 3 * relerr(ref[torch.float32][k], ref[torch.float64][k])
            print('%s %s overlap=%s %s: %.2e  bound %.2e' % (name, which, overlap, k, e, bound))
            assert e < bound, (k, overlap)


# ---- 6. mappings, draws, repeatability -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel,order', R.CASES)
def test_wave_and_team_mappings_agree(name, kernel, order):
    """2600 trajectories take the one-wavefront-per-trajectory kernel, chunks of 650 the team kernel; three time points, so one
    output is interpolated.  Bound 3e-4 + 2e-4, as tests/test_gpu_dopri5.py::test_wave_and_team_mappings_agree derives it."""
    from vae_gp_ode_amd import ops
    r = run(name, kernel, order, 1e-5, 'G2')
    N, tol = 2600, 1e-5
    x = torch.randn(N, r.c.Di, generator=torch.Generator().manual_seed(5)).cuda()
    ts = r.ts[:3].cuda()
    zw, cw = ops.rollout_adaptive(r.c, x, ts, order, tol, tol, max_steps=40, dense=True)
    parts = [ops.rollout_adaptive(r.c, x[i:i + 650], ts, order, tol, tol, max_steps=40, dense=True) for i in range(0, N, 650)]
    zt_, ct = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    assert (cw[:, 2] == 0).all() and (ct[:, 2] == 0).all()
    same = (cw[:, :2] == ct[:, :2]).all(1).float().mean().item()
    print('%s: team vs wave %.2e; same step counts on %.1f %% of the trajectories' % (name, relerr(zt_, zw), 100 * same))
    assert relerr(zt_, zw) < 3e-4 + 2e-4
    zw2, cw2 = ops.rollout_adaptive(r.c, x, ts, order, tol, tol, max_steps=40, dense=True)
    assert torch.equal(zw, zw2) and torch.equal(cw, cw2)


@pytest.mark.parametrize('kernel,Di,Do', [('RBF', 6, 6), ('DF', 4, 4), ('RBF', 6, 3)])
def test_draws_in_one_pass_equal_single_draw_calls(kernel, Di, Do):
    from test_gpu_draws import _build, _noise, _params
    from vae_gp_ode_amd import ops
    M, S, N, L, order = 16, 32, 5, 3, Di // Do
    p = {k: v.cuda() for k, v in _params(kernel, Di, Do, M, 3).items()}
    nz = {k: v.cuda() for k, v in _noise(kernel, Di, Do, M, S, L, 4).items()}
    gen = torch.Generator().manual_seed(5)
    T = 7
    z0, ts = torch.randn(N, Di, generator=gen).cuda(), (0.25 * torch.arange(T, dtype=torch.float)).cuda()
    gw = torch.randn(L, N, T, Di, generator=gen).cuda()
    cb = _build(ops, kernel, p, nz)
    solve = lambda c, **kw: ops.rollout_adaptive(c, z0, ts, order, 1e-3, 1e-3, dense=True, **kw)
    bwd = lambda c, out, g: ops.rollout_adaptive_bwd(c, out[2], out[3], out[4], g, order, theta=out[5])
    outb = solve(cb, save_stages=True)
    bwdb = bwd(cb, outb, gw)
    again = solve(cb, save_stages=True)
    assert all(torch.equal(a, b) for a, b in zip(outb, again))
    assert (outb[1][..., 2] == 0).all() and (outb[1][..., 0] >= 1).all()
    for l in range(L):
        c1 = _build(ops, kernel, p, {k: v[l].contiguous() for k, v in nz.items()})
        out1 = solve(c1, save_stages=True)
        for a, b, what in zip(outb, out1, ('zt', 'counts', 'xstage', 'hstep', 'istep', 'theta')):
            assert torch.equal(a[l], b), (l, what)
        bwd1 = bwd(c1, out1, gw[l].contiguous())
        assert torch.equal(bwdb[0][l], bwd1[0]) and torch.equal(bwdb[1][l], bwd1[1]), l
        # without the record: the same trajectories, nothing else written
        z_only, c_only = solve(c1)
        assert torch.equal(z_only, out1[0]) and torch.equal(c_only, out1[1])


# ---- 7. budget and degenerate shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel,order', R.CASES[:3])
def test_a_trajectory_that_exhausts_its_budget_fails_alone(name, kernel, order):
    """max_steps one below what the hungriest trajectory needs: a designed status, nothing is provoked."""
    from vae_gp_ode_amd import ops
    r = run(name, kernel, order, 1e-3, 'G2')
    z0, ts = r.g['z0'].cuda(), r.ts.cuda()
    need = r.cnt[:, 0]
    K = int(need.max()) - 1
    solve = lambda z, t, **kw: ops.rollout_adaptive(r.c, z, t, order, 1e-3, 1e-3, dense=True, **kw)
    zt, cnt, xs, hs, ie, th = [t.cpu() for t in solve(z0, ts, max_steps=K, save_stages=True)]
    torch.cuda.synchronize()                                                 # no HIP error follows
    assert (need > K).any()
    for n in range(z0.shape[0]):
        if need[n] > K:
            t_fail = int((r.ie[n] > K).nonzero()[0])                          # the first output that needs more than K steps
            assert cnt[n, 2] == 1 and cnt[n, 0] == K
            assert torch.equal(zt[n, :t_fail + 1], r.zt[n, :t_fail + 1]) and torch.isnan(zt[n, t_fail + 1:]).all()
            assert (ie[n, t_fail:] == K).all() and (th[n, t_fail:] == 1).all() and torch.equal(hs[n], r.hs[n, :K])
            assert torch.equal(ie[n, :t_fail].long(), r.ie[n, :t_fail]) and torch.equal(th[n, :t_fail], r.th[n, :t_fail])
        else:
            assert cnt[n, 2] == 0 and torch.equal(zt[n], r.zt[n]) and torch.equal(cnt[n], r.cnt[n].int())
            assert torch.equal(xs[n], r.xs[n, :K]) and torch.equal(ie[n].long(), r.ie[n]) and torch.equal(th[n], r.th[n])
    # the reverse sweep of such a record faults nothing either, and the healthy trajectories keep their gradient
    gw = torch.ones_like(r.zt).cuda()
    gz0, _ = ops.rollout_adaptive_bwd(r.c, xs.cuda(), hs.cuda(), ie.cuda(), gw, order, theta=th.cuda())
    gz0_full, _ = ops.rollout_adaptive_bwd(r.c, r.xs.cuda(), r.hs.cuda(), r.ie.int().cuda(), gw, order, theta=r.th.cuda())
    torch.cuda.synchronize()
    assert (need <= K).any() and torch.equal(gz0[need <= K], gz0_full[need <= K])
    # one time point: the initial state, no step; one trajectory; no trajectory
    z1, c1, x1, h1, i1, t1 = solve(z0, ts[:1], save_stages=True)
    assert torch.equal(z1[:, 0], z0) and (c1[:, :3] == 0).all() and x1.shape[1] == 0 and i1.shape[1] == 0 and t1.shape[1] == 0
    g1, a1 = ops.rollout_adaptive_bwd(r.c, x1, h1, i1, torch.ones_like(z1), order, theta=t1)
    assert torch.equal(g1, torch.ones_like(z0))
    zs, cs = solve(z0[:1], ts, max_steps=32)
    assert torch.equal(zs.cpu(), r.zt[:1]) and torch.equal(cs.cpu().long(), r.cnt[:1])
    assert tuple(solve(z0[:0], ts)[0].shape) == (0, ts.shape[0], z0.shape[1])
    with pytest.raises(Exception, match='strictly increasing'):
        solve(z0, ts.flip(0).contiguous())


# ---- 8. surface ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel,order', R.CASES)
def test_flow_counts_fewer_evaluations_on_the_training_grid(name, kernel, order):
    """Flow(dense_output=True) against Flow(dense_output=False) on G1 at 1e-3: fewer evaluations by the flow's own counts, and two
    results that differ by no more than the sum of their global errors against fp64 rk4 with 64 sub-steps per interval."""
    from test_gpu_backward import make_layer
    g = load_golden(name)
    ts = DR.G1
    tr = truth(name, kernel, order, 'G1')
    out = {}
    for dense in (False, True):
        flow, gp = make_layer(g, kernel, order, 'dopri5')
        flow.rtol = flow.atol = 1e-3
        flow.dense_output = dense
        with torch.no_grad():
            zt = flow(g['z0'].cuda(), ts.cuda())
        cnt = flow.last_counts.cpu().long()
        assert (cnt[:, 2] == 0).all() and tuple(cnt.shape) == (g['z0'].shape[0], 4)
        assert flow.num_evals() == cnt[:, 3].max().item()
        out[dense] = (zt.cpu(), cnt)
    (zl, cl), (zd, cd) = out[False], out[True]
    el, ed = relerr(zl, tr), relerr(zd, tr)
    print('%s: evaluations landing %d dense %d; global error landing %.2e dense %.2e; apart %.2e'
          % (name, cl[:, 3].sum(), cd[:, 3].sum(), el, ed, relerr(zd, zl)))
    assert (cd[:, 3] < cl[:, 3]).all() and (cd[:, 0] < ts.shape[0] - 1).all()
    assert ((zd - zl).abs().max() / tr.abs().max()).item() <= el + ed


def test_the_generic_rollout_entry_points_pass_the_dense_mode_through():
    """ops.rollout(..., 'dopri5', dense=True) / ops.rollout_bwd are rollout_adaptive / rollout_adaptive_bwd: the same bits."""
    from vae_gp_ode_amd import ops
    name, kernel, order = R.CASES[0]
    r = run(name, kernel, order, 1e-3, 'G1')
    z0, ts = r.g['z0'].cuda(), r.ts.cuda()
    zt, rec = ops.rollout(r.c, z0, ts, order, 'dopri5', save_stages=True, rtol=1e-3, atol=1e-3, dense=True)
    assert len(rec) == 5 and torch.equal(zt.cpu(), r.zt) and torch.equal(rec[3].cpu().long(), r.cnt)
    for got, want in zip((rec[0], rec[1], rec[2], rec[4]), (r.xs, r.hs, r.ie.int(), r.th)):
        assert torch.equal(got.cpu(), want)
    assert torch.equal(ops.rollout(r.c, z0, ts, order, 'dopri5', rtol=1e-3, atol=1e-3, dense=True).cpu(), r.zt)
    gw = torch.randn(r.zt.shape, generator=torch.Generator().manual_seed(13)).cuda()
    a = ops.rollout_bwd(r.c, rec, gw, ts, order, 'dopri5')
    b = ops.rollout_adaptive_bwd(r.c, rec[0], rec[1], rec[2], gw, order, theta=rec[4])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].shape[-2] == 7
    # the landing record of the same call has four entries and six rows per step
    _, rec_l = ops.rollout(r.c, z0, ts, order, 'dopri5', save_stages=True, rtol=1e-3, atol=1e-3)
    assert len(rec_l) == 4 and rec_l[0].shape[-2] == 6 and ops.rollout_bwd(r.c, rec_l, gw, ts, order, 'dopri5')[1].shape[-2] == 6


def test_a_padded_width_meets_the_tolerance_of_its_real_components():
    """RBF width 5 runs at the compiled width 6 on zero-padded operands; the tolerances are scaled so that the accepted steps are
    those of the 5 real components (see tests/test_gpu_dopri5.py)."""
    from vae_gp_ode_amd.model.core.flow import Flow
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    torch.manual_seed(4)
    gp = SVGP_Layer(5, 5, 16, 32, kernel='RBF').cuda()
    flow = Flow(gp, order=1, atol=1e-3, rtol=1e-3, max_steps=32, dense_output=True).cuda()
    z0, ts = torch.randn(4, 5).cuda().requires_grad_(True), R.case_ts('gp_rbf1_tiny', 5).cuda()
    zt = flow(z0, ts)
    xs, hs, ie, th = recorded(zt)
    xs, hs, cnt = xs.cpu(), hs.cpu(), flow.last_counts.cpu().long()
    assert tuple(zt.shape) == (4, 5, 5) and tuple(xs.shape[-2:]) == (7, 6) and (cnt[:, 2] == 0).all() and (xs[..., 5] == 0).all()
    assert (th > 0).all() and (th <= 1).all() and (ie[:, -1].cpu().long() == cnt[:, 0]).all()
    rhs = lambda y: gp(y.float().cuda()).double().cpu()
    live = torch.arange(hs.shape[1])[None] < cnt[:, :1]
    y = xs[:, :, 0][live][:, :5].double()
    ynew, err, _, _ = R.step(rhs, y, hs[live].double().unsqueeze(1))
    ratio = ((err / (1e-3 + 1e-3 * torch.maximum(y.abs(), ynew.abs()))) ** 2).mean(1).sqrt()
    assert ratio.max() <= 1.01, ratio.max()
    zt.sum().backward()
    assert torch.isfinite(z0.grad).all() and torch.isfinite(gp.Um.optvar.grad).all()


def test_predict_and_no_grad_rollout_equal_the_recording_forward():
    """evaluate.predict integrates under no_grad (no record is written): the same trajectories, bit for bit, as the forward of a
    training step, which records its steps; and a roll-out of twice the observed length runs through predict in dense mode."""
    from test_gpu_eval import CASES, L_FIX, make_model, queue_fixture_noise
    from vae_gp_ode_amd.evaluate import predict
    name, kw = CASES[0]
    m, g = make_model(name, dict(kw, solver='dopri5'))
    m.flow.dense_output = True
    m.flow.rtol = m.flow.atol = 1e-4
    X = g['X'].cuda()
    N, T = X.shape[:2]
    queue_fixture_noise(m, g)
    a = predict(m, X, L_FIX)
    queue_fixture_noise(m, g)
    b = predict(m, X, L_FIX)
    assert a.state == b.state and torch.isfinite(a.mean).all() and a.mse > 0 and a.mse == a.mse
    queue_fixture_noise(m, g)
    c = predict(m, X, L_FIX, T_custom=2 * T)
    cnt = m.flow.last_counts.cpu()
    assert tuple(c.mean.shape) == (N, 2 * T, 1, 28, 28) and torch.isfinite(c.mean).all() and (cnt[..., 2] == 0).all()
    assert tuple(cnt.shape) == (L_FIX, N, 4)
    gp = m.flow.odefunc.diffeq
    z0 = torch.randn(4, 6, generator=torch.Generator().manual_seed(1)).cuda()
    ts = DR.G1.cuda()
    nz = {k: v.cuda() for k, v in sub(g, 'noise0.').items()}
    gp.set_noise(nz)
    with torch.no_grad():
        z_eval = m.flow(z0, ts)
    gp.set_noise(nz)
    z_train = m.flow(z0.clone().requires_grad_(True), ts)
    assert z_train.grad_fn is not None and torch.equal(z_eval, z_train.detach())
    assert recorded(z_train)[3] is not None


def test_the_environment_variable_switches_models_built_through_build_model(monkeypatch):
    from test_gpu_eval import model_args
    from vae_gp_ode_amd.model.create_model import build_model
    monkeypatch.setenv('GPODE_DOPRI5_DENSE', '1')
    m = build_model(model_args(solver='dopri5')).cuda()
    assert m.flow.dense_output is True
    m.flow.rtol = m.flow.atol = 1e-3
    z0 = torch.randn(3, 6, generator=torch.Generator().manual_seed(2)).cuda().requires_grad_(True)
    zt = m.flow(z0, DR.G1.cuda())
    assert recorded(zt)[0].shape[-2] == 7 and (m.flow.last_counts[:, 2] == 0).all()
    monkeypatch.setenv('GPODE_DOPRI5_DENSE', '0')
    assert build_model(model_args(solver='dopri5')).flow.dense_output is False


# ---- 9. graph replay ---------------------------------------------------------------------------------------------------------------------
def test_graph_replay_of_a_dense_dopri5_training_step_equals_the_eager_step():
    """tests/test_gpu_dopri5.py::test_graph_replay_of_a_dopri5_training_step_equals_the_eager_step with Flow.dense_output = True:
    1 eager + 2 replayed steps == 3 eager steps, bit for bit."""
    from vae_gp_ode_amd.graph import GraphedStep
    from vae_gp_ode_amd.model.core.initialization import initialize_and_fix_kernel_parameters
    from vae_gp_ode_amd.model.core.noise import DeviceNoise
    from vae_gp_ode_amd.model.create_model import build_model, compute_loss
    from vae_gp_ode_amd.model.misc.torch_utils import seed_everything
    from vae_gp_ode_amd.optim import HipAdam
    seed_everything(4)
    args = types.SimpleNamespace(D_in=6, D_out=6, num_inducing=16, num_features=32, dimwise=True, q_diag=False, device='cuda',
                                 kernel='RBF', ode=1, solver='dopri5', use_adjoint=False, frames=5, n_filt=8, latent_dim=6, Ndata=64, dt=0.1)
    m = build_model(args).cuda()
    m.flow.rtol = m.flow.atol = 1e-4
    m.flow.dense_output = True
    initialize_and_fix_kernel_parameters(m, 2.0, 1.0)
    init = copy.deepcopy(m.state_dict())
    X = torch.rand(4, 6, 1, 28, 28, device='cuda')
    fixed = DeviceNoise(9).draw('RBF', 6, 6, 16, 32, 'cuda')

    class FixedNoise:
        def draw(self, *a):
            return fixed
    m.flow.odefunc.diffeq.noise_source = FixedNoise()
    eps = torch.randn(4, 6, device='cuda')

    def run_steps(use_graph):
        m.load_state_dict(init)
        opt = HipAdam(m.parameters(), lr=1e-3)

        def step():
            m.vae.encoder.next_eps = eps
            opt.zero_grad()
            loss, *_ = compute_loss(m, X, 1)
            loss.backward()
            opt.step()
            return loss
        if use_graph:
            gs = GraphedStep(step, warmup=1)
            gs(); gs()
        else:
            for _ in range(3):
                step()
        torch.cuda.synchronize()
        assert (m.flow.last_counts[..., 2] == 0).all() and m.flow.num_evals() >= 1 + 6
        return [p.detach().clone() for p in m.parameters()]
    for a, b in zip(run_steps(False), run_steps(True)):
        assert torch.equal(a, b)
