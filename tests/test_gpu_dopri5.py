"""GPU: the adaptive Dormand-Prince solver -- rollout (gpode_rollout_adaptive_fwd_n), reverse sweep (gpode_rollout_adaptive_bwd_n)
and the surface above them -- against tests/dopri5_ref.py on the oracle's right-hand side.

Inputs: the fixtures' own z0 with the stretched, non-uniform ts of dopri5_ref.case_ts, at rtol = atol = 1e-3 and 1e-5
(tests/test_dopri5_host.py proves on the CPU that they make the controller cut, reject and take several steps per interval).

What is compared with what.  The kernel chooses its steps in fp32, so a borderline accept / reject can fall differently than in any
reference run; the result is therefore never compared step by step with another SOLVE.  It is compared with a REPLAY of the kernel's
own recorded steps (that is also what the gradient is defined through), and the choice of the steps is checked on its own: every
accepted step must pass the error test when it is recomputed in fp64.
Bounds: trajectories 2e-4 + 3 relerr(fp32 replay, fp64 replay) (tests/test_gpu_forward.py: tol_downstream); dL/dz0 and dL/df
5e-4 + 3 relerr(fp32, fp64), parameter gradients 1e-3 + 3 relerr(fp32, fp64) (tests/test_gpu_backward.py, rk4)."""
import copy
import types

import pytest
import torch

import dopri5_ref as R
from conftest import load_golden, sub
from oracle import gpode_oracle as O
from test_gpu_forward import build, relerr

pytestmark = pytest.mark.gpu

_RUNS = {}


def run(name, kernel, order, tol):
    """The kernel's solve of one case (with the record), computed once and shared -- nobody writes to it."""
    from vae_gp_ode_amd import ops
    key = (name, tol)
    if key not in _RUNS:
        g = load_golden(name)
        c = build(g, kernel, want_Lu=False)
        ts = R.case_ts(name, g['ts'].shape[0])
        zt, cnt, xs, hs, ie = ops.rollout_adaptive(c, g['z0'].cuda(), ts.cuda(), order, tol, tol, save_stages=True)
        _RUNS[key] = types.SimpleNamespace(g=g, c=c, ts=ts, zt=zt.cpu(), cnt=cnt.cpu().long(), xs=xs.cpu(), hs=hs.cpu(), ie=ie.cpu().long(),
                                           K=hs.shape[-1])
    return _RUNS[key]


def recorded(zt):
    """(xstage, hstep, iend) the forward behind ``zt`` saved for its backward (the autograd node of ops._Flow)"""
    fn = zt.grad_fn
    while '_Flow' not in type(fn).__name__:
        fn = fn.next_functions[0][0]
    saved = fn.saved_tensors
    return saved[1], saved[5], saved[6]


def per_interval(ie):
    return torch.diff(torch.cat([torch.zeros(ie.shape[0], 1, dtype=torch.long), ie], 1), dim=1)


# ---- 1. forward against a replay of the recorded steps -----------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel,order', R.CASES)
@pytest.mark.parametrize('tol', R.TOLS)
def test_trajectories_equal_a_replay_of_the_recorded_steps(name, kernel, order, tol):
    r = run(name, kernel, order, tol)
    g, f64 = R.oracle_rhs(name, kernel, order)
    _, f32 = R.oracle_rhs(name, kernel, order, torch.float32)
    N, T = r.zt.shape[:2]
    assert (r.cnt[:, 2] == 0).all(), r.cnt
    z64 = R.replay(f64, g['z0'].double(), r.ts, r.hs.double(), r.ie)
    z32 = R.replay(f32, g['z0'], r.ts, r.hs, r.ie)
    e, bound = relerr(r.zt, z64), 2e-4 + 3 * relerr(z32, z64)
    print('%s tol %g: |hip - replay64| %.2e  bound %.2e  steps %s rejected %s' % (name, tol, e, bound, r.cnt[:, 0].tolist(), r.cnt[:, 1].tolist()))
    assert e < bound
    assert torch.equal(r.zt[:, 0], g['z0'])
    # the record: steps add up to the intervals, the step numbers at the outputs increase, nothing but zeros past the count
    dts = torch.diff(r.ts)
    assert (torch.diff(r.ie, dim=1) >= 1).all() and (r.ie[:, 0] >= 1).all() and (r.ie[:, -1] == r.cnt[:, 0]).all() and (r.ie <= r.K).all()
    for n in range(N):
        lo = 0
        for t in range(T - 1):
            hi = int(r.ie[n, t])
            got, want = r.hs[n, lo:hi].double().sum().item(), float(dts[t])
            assert abs(got - want) <= 4 * torch.finfo(torch.float32).eps * want, (n, t, got, want)
            lo = hi
        assert (r.hs[n, :lo] > 0).all() and (r.hs[n, lo:] == 0).all() and (r.xs[n, lo:] == 0).all()
    assert torch.equal(r.xs[:, 0, 0], g['z0'])
    # the recorded stage inputs are those of the replay
    aux = {}
    R.replay(f64, g['z0'].double(), r.ts, r.hs.double(), r.ie, aux)
    xs64 = torch.stack([torch.stack(x, 1) for x in aux['xs']], 1)           # (N,K,6,D)
    live = (torch.arange(r.K)[None] < r.cnt[:, :1])[:, :, None, None]
    assert relerr(r.xs * live, xs64 * live) < bound


# ---- 2. the controller ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel,order', R.CASES)
def test_every_accepted_step_passes_the_error_test_in_fp64(name, kernel, order):
    tol = 1e-3
    r = run(name, kernel, order, tol)
    _, f64 = R.oracle_rhs(name, kernel, order)
    live = torch.arange(r.K)[None] < r.cnt[:, :1]
    y = r.xs[:, :, 0][live].double()                                         # (rows, D): where each accepted step started
    h = r.hs[live].double().unsqueeze(1)
    ynew, err, _, _ = R.step(f64, y, h)
    ratio = ((err / (tol + tol * torch.maximum(y.abs(), ynew.abs()))) ** 2).mean(1).sqrt()
    print('%s: largest fp64 error ratio of an accepted step %.4f; accepted %s rejected %s' % (name, ratio.max(), r.cnt[:, 0].tolist(), r.cnt[:, 1].tolist()))
    assert ratio.max() <= 1.01          # fp32 rounding of an error estimate of size 1e-3 is about 1e-3 relative
    assert r.cnt[:, 1].sum() >= 1 and per_interval(r.ie).max() >= 2
    assert (r.cnt[:, 3] == 1 + 6 * (r.cnt[:, 0] + r.cnt[:, 1])).all()


# ---- 3. accuracy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel,order', R.CASES)
def test_global_error_follows_the_tolerance(name, kernel, order):
    """Against fp64 rk4 with 64 sub-steps per interval: the kernel's error is at most twice the error of the fp64 reference solve
    at the same tolerances (+ 1e-5; borderline decisions fall differently in fp32), a tighter tolerance gives a smaller error and
    costs no fewer evaluations.  Measured on MI355X, (kernel, reference solve) at 1e-3 | 1e-5:
    rbf1_tiny (1.49e-3, 1.49e-3) | (2.06e-5, 2.02e-5);  rbf2_tiny (2.52e-3, 2.52e-3) | (5.00e-6, 5.99e-6);
    df1_tiny (4.47e-3, 4.57e-3) | (5.03e-5, 6.32e-5);  df1_tiny_q5 (1.79e-3, 1.92e-3) | (5.03e-6, 4.88e-6);
    evaluations summed over the trajectories 172 | 268, 178 | 304, 154 | 316, 149 | 227."""
    g, f64 = R.oracle_rhs(name, kernel, order)
    ts = R.case_ts(name, g['ts'].shape[0])
    dense = torch.cat([ts[i].double() + (ts[i + 1] - ts[i]).double() * torch.arange(64, dtype=torch.float64) / 64 for i in range(len(ts) - 1)]
                      + [ts[-1:].double()])
    truth = O.odeint_fixed(f64, g['z0'].double(), dense, 'rk4')[::64].permute(1, 0, 2)
    errs, evals = [], []
    for tol in R.TOLS:
        r = run(name, kernel, order, tol)
        ref = R.solve(f64, g['z0'].double(), ts, tol, tol)[0]
        e_hip, e_ref = relerr(r.zt, truth), relerr(ref, truth)
        print('%s tol %g: |hip - truth| %.2e  |fp64 solve - truth| %.2e  evaluations %d' % (name, tol, e_hip, e_ref, r.cnt[:, 3].sum()))
        assert e_hip <= 2 * e_ref + 1e-5
        errs.append(e_hip); evals.append(int(r.cnt[:, 3].sum()))
    assert errs[1] < errs[0] and evals[1] >= evals[0]


# ---- 4. reverse sweep ----------------------------------------------------------------------------------------------------------------
def replay_grads(name, kernel, order, r, gw, dtype):
    """autograd through the replay of the recorded steps: dL/dz0, dL/df at every recorded evaluation (N,K,6,Do), L = sum(zt gw)"""
    _, f = R.oracle_rhs(name, kernel, order, dtype)
    z0 = r.g['z0'].to(dtype).clone().requires_grad_(True)
    aux = {}
    zt = R.replay(f, z0, r.ts, r.hs.to(dtype), r.ie, aux)
    ks = [k for step in aux['ks'] for k in step]
    grads = torch.autograd.grad((zt * gw.to(dtype)).sum(), [z0] + ks, allow_unused=True)
    Do = r.c.Do
    gk = torch.stack([torch.zeros_like(z0) if x is None else x for x in grads[1:]], 1).view(z0.shape[0], r.K, 6, -1)[..., -Do:]
    return grads[0], gk


@pytest.mark.parametrize('name,kernel,order', R.CASES)
def test_reverse_sweep_matches_autograd_through_the_replay(name, kernel, order):
    from vae_gp_ode_amd import ops
    r = run(name, kernel, order, 1e-3)
    gw = torch.randn(r.zt.shape, generator=torch.Generator().manual_seed(11))
    gz0, ast = ops.rollout_adaptive_bwd(r.c, r.xs.cuda(), r.hs.cuda(), r.ie.int().cuda(), gw.cuda(), order)
    (z64, a64), (z32, a32) = replay_grads(name, kernel, order, r, gw, torch.float64), replay_grads(name, kernel, order, r, gw, torch.float32)
    for what, got, ref, twin in (('dL/dz0', gz0, z64, z32), ('dL/df', ast, a64, a32)):
        e, bound = relerr(got, ref), 5e-4 + 3 * relerr(twin, ref)
        print('%s %s: %.2e  bound %.2e' % (name, what, e, bound))
        assert e < bound
    live = (torch.arange(r.K)[None] < r.cnt[:, :1])[:, :, None, None]
    assert (ast.cpu()[~live.expand_as(ast)] == 0).all()
    gz0b, astb = ops.rollout_adaptive_bwd(r.c, r.xs.cuda(), r.hs.cuda(), r.ie.int().cuda(), gw.cuda(), order)
    assert torch.equal(gz0, gz0b) and torch.equal(ast, astb)


@pytest.mark.parametrize('name,kernel,order', R.CASES)
def test_flow_parameter_gradients(name, kernel, order):
    """loss.backward() through Flow(solver='dopri5'): the five GP parameter gradients and dL/dz0 against fp64 autograd through the
    cache build and the replay of the steps this very solve recorded; then the same with the side-stream overlap on."""
    from test_gpu_backward import make_layer
    from vae_gp_ode_amd import ops
    g = load_golden(name)
    ts = R.case_ts(name, g['ts'].shape[0])
    gw = torch.randn(g['z0'].shape[0], ts.shape[0], g['z0'].shape[1], generator=torch.Generator().manual_seed(12))
    flow, gp = make_layer(g, kernel, order, 'dopri5')
    flow.rtol = flow.atol = 1e-3
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
            _, hs, ie = recorded(zt)
            hs, ie = hs.cpu(), ie.cpu().long()
            (zt * gw.cuda()).sum().backward()
            ops.join_side_stream()
            torch.cuda.synchronize()
        finally:
            ops.set_overlap(False)
        got = dict({k: p.grad.clone() for k, p in names.items()}, z0=z0.grad)
        assert (flow.last_counts[:, 2] == 0).all()
        if ref is None:
            ref = {}
            for dtype in (torch.float64, torch.float32):
                p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in O.gp_params_from_state_dict(sub(g, 'sd.')).items()}
                c = O.build_cache(p, O.to_dtype(sub(g, 'noise.'), dtype), kernel)
                z = g['z0'].to(dtype).clone().requires_grad_(True)
                out = R.replay(lambda y: O.ode_rhs(y, c, order), z, ts, hs.to(dtype), ie)
                (out * gw.to(dtype)).sum().backward()
                ref[dtype] = dict({k: v.grad for k, v in p.items()}, z0=z.grad)
        for k in got:
            e, bound = relerr(got[k], ref[torch.float64][k]), (5e-4 if k == 'z0' else 1e-3) + 3 * relerr(ref[torch.float32][k], ref[torch.float64][k])
            print('%s overlap=%s %s: %.2e  bound %.2e' % (name, overlap, k, e, bound))
            assert e < bound, (k, overlap)


# ---- 5. mappings, draws, repeatability -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel,order', R.CASES)
def test_wave_and_team_mappings_agree(name, kernel, order):
    """2600 trajectories take the one-wavefront-per-trajectory kernel, chunks of 650 the team kernel.  The two sum f in different
    orders (3e-4 on a trajectory, tests/test_gpu_forward.py), so a borderline step can be accepted by one and rejected by the other:
    the results then differ like two solves that both meet the tolerance -- by their global errors, which 10 steps of local error
    1e-5 bound by 1e-4 each.  Bound: 3e-4 + 2e-4."""
    from vae_gp_ode_amd import ops
    r = run(name, kernel, order, 1e-5)
    N, tol = 2600, 1e-5
    x = torch.randn(N, r.c.Di, generator=torch.Generator().manual_seed(5)).cuda()
    ts = r.ts[:3].cuda()
    zw, cw = ops.rollout_adaptive(r.c, x, ts, order, tol, tol, max_steps=40)
    parts = [ops.rollout_adaptive(r.c, x[i:i + 650], ts, order, tol, tol, max_steps=40) for i in range(0, N, 650)]
    zt_, ct = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    assert (cw[:, 2] == 0).all() and (ct[:, 2] == 0).all()
    same = (cw[:, :2] == ct[:, :2]).all(1).float().mean().item()
    print('%s: team vs wave %.2e; same step counts on %.1f %% of the trajectories' % (name, relerr(zt_, zw), 100 * same))
    assert relerr(zt_, zw) < 3e-4 + 2e-4
    zw2, cw2 = ops.rollout_adaptive(r.c, x, ts, order, tol, tol, max_steps=40)
    assert torch.equal(zw, zw2) and torch.equal(cw, cw2)


@pytest.mark.parametrize('kernel,Di,Do', [('RBF', 6, 6), ('DF', 4, 4), ('RBF', 6, 3)])
def test_draws_in_one_pass_equal_single_draw_calls(kernel, Di, Do):
    from test_gpu_draws import _build, _noise, _params
    from vae_gp_ode_amd import ops
    M, S, N, L, order = 16, 32, 5, 3, Di // Do
    p = {k: v.cuda() for k, v in _params(kernel, Di, Do, M, 3).items()}
    nz = {k: v.cuda() for k, v in _noise(kernel, Di, Do, M, S, L, 4).items()}
    gen = torch.Generator().manual_seed(5)
    z0, ts = torch.randn(N, Di, generator=gen).cuda(), R.case_ts('gp_rbf1_tiny', 4).cuda()
    gw = torch.randn(L, N, 4, Di, generator=gen).cuda()
    cb = _build(ops, kernel, p, nz)
    outb = ops.rollout_adaptive(cb, z0, ts, order, 1e-3, 1e-3, save_stages=True)
    bwdb = ops.rollout_adaptive_bwd(cb, outb[2], outb[3], outb[4], gw, order)
    again = ops.rollout_adaptive(cb, z0, ts, order, 1e-3, 1e-3, save_stages=True)
    assert all(torch.equal(a, b) for a, b in zip(outb, again))
    assert (outb[1][..., 2] == 0).all() and (outb[1][..., 0] >= 3).all()
    for l in range(L):
        c1 = _build(ops, kernel, p, {k: v[l].contiguous() for k, v in nz.items()})
        out1 = ops.rollout_adaptive(c1, z0, ts, order, 1e-3, 1e-3, save_stages=True)
        for a, b, what in zip(outb, out1, ('zt', 'counts', 'xstage', 'hstep', 'iend')):
            assert torch.equal(a[l], b), (l, what)
        bwd1 = ops.rollout_adaptive_bwd(c1, out1[2], out1[3], out1[4], gw[l].contiguous(), order)
        assert torch.equal(bwdb[0][l], bwd1[0]) and torch.equal(bwdb[1][l], bwd1[1]), l
        # without the record: the same trajectories, nothing else written
        z_only, c_only = ops.rollout_adaptive(c1, z0, ts, order, 1e-3, 1e-3)
        assert torch.equal(z_only, out1[0]) and torch.equal(c_only, out1[1])


# ---- 6. budget and degenerate shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kernel,order', R.CASES[:3])
def test_a_trajectory_that_exhausts_its_budget_fails_alone(name, kernel, order):
    from vae_gp_ode_amd import ops
    r = run(name, kernel, order, 1e-3)
    z0, ts = r.g['z0'].cuda(), r.ts.cuda()
    need = r.cnt[:, 0]
    K = int(need.max()) - 1
    zt, cnt, xs, hs, ie = [t.cpu() for t in ops.rollout_adaptive(r.c, z0, ts, order, 1e-3, 1e-3, max_steps=K, save_stages=True)]
    torch.cuda.synchronize()                                                 # no HIP error follows
    assert (need > K).any()
    for n in range(z0.shape[0]):
        if need[n] > K:
            t_fail = int((r.ie[n] > K).nonzero()[0])                          # the first output that needs more than K steps
            assert cnt[n, 2] == 1 and cnt[n, 0] == K
            assert torch.equal(zt[n, :t_fail + 1], r.zt[n, :t_fail + 1]) and torch.isnan(zt[n, t_fail + 1:]).all()
            assert (ie[n, t_fail:] == K).all() and torch.equal(hs[n], r.hs[n, :K])
        else:
            assert cnt[n, 2] == 0 and torch.equal(zt[n], r.zt[n]) and torch.equal(cnt[n], r.cnt[n].int())
            assert torch.equal(xs[n], r.xs[n, :K]) and torch.equal(ie[n].long(), r.ie[n])
    # the reverse sweep of such a record faults nothing either, and the healthy trajectories keep their gradient
    gw = torch.ones_like(r.zt).cuda()
    gz0, _ = ops.rollout_adaptive_bwd(r.c, xs.cuda(), hs.cuda(), ie.cuda(), gw, order)
    gz0_full, _ = ops.rollout_adaptive_bwd(r.c, r.xs.cuda(), r.hs.cuda(), r.ie.int().cuda(), gw, order)
    torch.cuda.synchronize()
    assert torch.equal(gz0[need <= K], gz0_full[need <= K])
    # one time point: the initial state, no step; one trajectory; no trajectory
    z1, c1, x1, h1, i1 = ops.rollout_adaptive(r.c, z0, ts[:1], order, 1e-3, 1e-3, save_stages=True)
    assert torch.equal(z1[:, 0], z0) and (c1[:, :3] == 0).all() and x1.shape[1] == 0 and i1.shape[1] == 0
    g1, a1 = ops.rollout_adaptive_bwd(r.c, x1, h1, i1, torch.ones_like(z1), order)
    assert torch.equal(g1, torch.ones_like(z0))
    zs, cs = ops.rollout_adaptive(r.c, z0[:1], ts, order, 1e-3, 1e-3)
    assert torch.equal(zs.cpu(), r.zt[:1]) and torch.equal(cs.cpu().long(), r.cnt[:1])
    assert tuple(ops.rollout_adaptive(r.c, z0[:0], ts, order, 1e-3, 1e-3)[0].shape) == (0, ts.shape[0], z0.shape[1])
    with pytest.raises(Exception, match='strictly increasing'):
        ops.rollout_adaptive(r.c, z0, ts.flip(0).contiguous(), order, 1e-3, 1e-3)


# ---- 7. surface ------------------------------------------------------------------------------------------------------------------------
def test_flow_with_its_defaults_runs():
    """Flow(gp): second order, solver 'dopri5', tolerances 1e-6 -- the reference's defaults (flow.py:49)."""
    from vae_gp_ode_amd.model.core.flow import Flow
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    torch.manual_seed(3)
    gp = SVGP_Layer(6, 3, 16, 32, kernel='RBF').cuda()
    flow = Flow(gp).cuda()
    assert flow.solver == 'dopri5' and flow.odefunc.order == 2
    z0, ts = torch.randn(5, 6).cuda(), (0.1 * torch.arange(6, dtype=torch.float)).cuda()
    zt = flow(z0, ts)
    cnt = flow.last_counts
    assert tuple(zt.shape) == (5, 6, 6) and tuple(cnt.shape) == (5, 4)
    ok = cnt[:, 2] == 0
    assert ok.any() and torch.isfinite(zt[ok]).all() and torch.isnan(zt[~ok][:, -1]).all()
    assert flow.num_evals() == cnt[:, 3].max().item() == flow.odefunc.state_dict()['_num_evals'].item()
    assert (cnt[:, 3] == 1 + 6 * (cnt[:, 0] + cnt[:, 1])).all()
    # three draws in one pass; a fixed-grid solve afterwards owns the count again
    ztL = flow(z0, ts, draws=3)
    assert tuple(ztL.shape) == (3, 5, 6, 6) and tuple(flow.last_counts.shape) == (3, 5, 4)
    assert flow.num_evals() == flow.last_counts[..., 3].max().item()
    flow.solver = 'rk4'
    flow(z0, ts)
    assert flow.num_evals() == 4 * 5 and flow.last_counts is None


def test_a_padded_width_meets_the_tolerance_of_its_real_components():
    """RBF width 5 runs at the compiled width 6 on zero-padded operands; the controller's norm then averages over 6 components, one
    of them exactly 0, and the tolerances are scaled so that the accepted steps are those of the 5 real ones."""
    from vae_gp_ode_amd.model.core.flow import Flow
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    torch.manual_seed(4)
    gp = SVGP_Layer(5, 5, 16, 32, kernel='RBF').cuda()
    flow = Flow(gp, order=1, atol=1e-3, rtol=1e-3).cuda()
    z0, ts = torch.randn(4, 5).cuda().requires_grad_(True), R.case_ts('gp_rbf1_tiny', 5).cuda()
    zt = flow(z0, ts)
    xs, hs, _ = recorded(zt)
    xs, hs, cnt = xs.cpu(), hs.cpu(), flow.last_counts.cpu().long()
    assert tuple(zt.shape) == (4, 5, 5) and xs.shape[-1] == 6 and (cnt[:, 2] == 0).all() and (xs[..., 5] == 0).all()
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
    training step, which records its steps."""
    from test_gpu_eval import CASES, L_FIX, make_model, queue_fixture_noise
    from vae_gp_ode_amd.evaluate import predict
    name, kw = CASES[0]
    m, g = make_model(name, dict(kw, solver='dopri5'))
    assert m.flow.solver == 'dopri5'
    m.flow.rtol = m.flow.atol = 1e-4
    X = g['X'].cuda()
    queue_fixture_noise(m, g)
    a = predict(m, X, L_FIX)
    queue_fixture_noise(m, g)
    b = predict(m, X, L_FIX)
    assert a.state == b.state and torch.isfinite(a.mean).all() and a.mse > 0 and a.mse == a.mse
    gp = m.flow.odefunc.diffeq
    z0 = torch.randn(4, 6, generator=torch.Generator().manual_seed(1)).cuda()
    ts = R.case_ts('gp_rbf1_tiny', 5).cuda()
    nz = {k: v.cuda() for k, v in sub(g, 'noise0.').items()}
    gp.set_noise(nz)
    with torch.no_grad():
        z_eval = m.flow(z0, ts)
    gp.set_noise(nz)
    z_train = m.flow(z0.clone().requires_grad_(True), ts)
    assert z_train.grad_fn is not None and torch.equal(z_eval, z_train.detach())


def test_graph_replay_of_a_dopri5_training_step_equals_the_eager_step():
    """tests/test_gpu_optim.py::test_graph_replay_equals_eager_steps with --solver dopri5: 1 eager + 2 replayed steps == 3 eager
    steps, bit for bit (the data-dependent trip counts live inside the kernel; nothing synchronises with the host)."""
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
        assert (m.flow.last_counts[..., 2] == 0).all() and m.flow.num_evals() >= 1 + 6 * 5
        return [p.detach().clone() for p in m.parameters()]
    for a, b in zip(run_steps(False), run_steps(True)):
        assert torch.equal(a, b)

