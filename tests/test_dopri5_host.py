"""CPU: the Dormand-Prince reference helper (tests/dopri5_ref.py), the host surface of the 'dopri5' solver, and a proof that the
inputs of the GPU tests exercise the step-size controller."""
import math
import os
import re
from fractions import Fraction

import pytest
import torch

import dopri5_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tableau_identities():
    F = lambda v: Fraction(v).limit_denominator(10 ** 7)
    assert sum(F(b) for b in R.B5) == 1 and sum(F(b) for b in R.B4) == 1
    for c, row in zip(R.C, R.A):
        assert F(c) == sum(F(a) for a in row)
    assert sum(F(e) for e in R.E) == 0
    assert [F(a) for a in R.A[6]] == [F(b) for b in R.B5[:6]] and R.B5[6] == 0         # first-same-as-last; b7 = 0
    # order conditions up to 3 for both weight sets (sum b c = 1/2, sum b c^2 = 1/3)
    for b in (R.B5, R.B4):
        assert sum(F(x) * F(c) for x, c in zip(b, R.C)) == Fraction(1, 2)
        assert sum(F(x) * F(c) ** 2 for x, c in zip(b, R.C)) == Fraction(1, 3)


def oscillator(y):
    return torch.stack([y[:, 1], -y[:, 0]], 1)


def exact(t):
    return torch.stack([torch.cos(t), -torch.sin(t)], -1)


def test_replay_converges_with_fifth_order():
    y0 = torch.tensor([[1.0, 0.0]], dtype=torch.float64)
    ts = torch.tensor([0.0, 2.0], dtype=torch.float64)
    errs = []
    for n in (8, 16, 32):
        zt = R.replay(oscillator, y0, ts, torch.full((1, n), 2.0 / n, dtype=torch.float64), torch.tensor([[n]]))
        errs.append((zt[0, 1] - exact(ts[1])).abs().max().item())
    for a, b in zip(errs, errs[1:]):
        assert 0.75 * 32 < a / b < 1.25 * 32, errs


def test_replay_is_differentiable_and_zero_steps_change_nothing():
    y0 = torch.tensor([[1.0, 0.0], [0.5, 0.5]], dtype=torch.float64, requires_grad=True)
    ts = torch.tensor([0.0, 0.4, 1.0], dtype=torch.float64)
    hs = torch.tensor([[0.4, 0.3, 0.3, 0.0], [0.2, 0.2, 0.6, 0.0]], dtype=torch.float64)
    ie = torch.tensor([[1, 3], [2, 3]])
    zt = R.replay(oscillator, y0, ts, hs, ie)
    assert (zt[0, 1] - exact(ts[1])).abs().max() < 1e-4 and (zt[0, 2] - exact(ts[2])).abs().max() < 1e-4
    assert torch.equal(zt[:, 0], y0)
    zt.sum().backward()
    assert torch.isfinite(y0.grad).all() and y0.grad.abs().min() > 0


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_solve_lands_on_every_output_time(dtype):
    y0 = torch.tensor([[1.0, 0.0], [0.0, 2.0], [3.0, -1.0]], dtype=dtype)
    ts = torch.tensor([0.0, 0.05, 1.3, 1.31, 6.0, 7.5])
    tol = 1e-6 if dtype == torch.float64 else 1e-4
    zt, hs, ie, cnt = R.solve(oscillator, y0, ts, tol, tol, max_steps=200)
    assert (cnt[:, 2] == 0).all() and (cnt[:, 3] == 1 + 6 * (cnt[:, 0] + cnt[:, 1])).all()
    assert (ie[:, -1] == cnt[:, 0]).all() and (torch.diff(ie, dim=1) >= 1).all()
    dts = torch.diff(ts.to(dtype))
    ulp = torch.finfo(dtype).eps
    for n in range(y0.shape[0]):
        lo = 0
        for t in range(ts.shape[0] - 1):
            hi = ie[n, t].item()
            assert abs(hs[n, lo:hi].double().sum().item() - dts[t].double().item()) <= max(4, hi - lo) * ulp * dts[t].item()
            lo = hi
        assert (hs[n, lo:] == 0).all()
    # the states at the output times are the solution there: rotation of y0 by the angle ts[t]
    t64 = ts.double()
    rot = torch.stack([torch.stack([torch.cos(t64), torch.sin(t64)], -1), torch.stack([-torch.sin(t64), torch.cos(t64)], -1)], -2)   # (T,2,2)
    want = torch.einsum('tij,nj->nti', rot, y0.double())
    assert (zt.double() - want).abs().max() < 200 * tol


def test_solve_budget_and_underflow_failures():
    y0 = torch.tensor([[1.0, 0.0], [0.0, 2.0]], dtype=torch.float64)
    ts = torch.tensor([0.0, 1.0, 4.0])
    full = R.solve(oscillator, y0, ts, 1e-6, 1e-6, max_steps=100)
    need = full[3][:, 0]
    K = int(need.max()) - 1
    zt, hs, ie, cnt = R.solve(oscillator, y0, ts, 1e-6, 1e-6, max_steps=K)
    for n in range(2):
        if need[n] > K:
            assert cnt[n, 2] == 1 and torch.isnan(zt[n, -1]).all() and cnt[n, 0] == K
        else:
            assert cnt[n, 2] == 0 and torch.equal(zt[n], full[0][n])
    # a right-hand side that blows up in finite time: the step shrinks until it underflows
    zt, hs, ie, cnt = R.solve(lambda y: y * y, torch.tensor([[1.0]], dtype=torch.float64), torch.tensor([0.0, 0.5, 2.0]), 1e-6, 1e-6,
                              max_steps=2000)
    assert cnt[0, 2] == 2 and torch.isfinite(zt[0, 1]).all() and torch.isnan(zt[0, 2]).all()


def test_dopri5_is_a_method_of_the_host_surface():
    from vae_gp_ode_amd import ops
    assert 'dopri5' in ops.METHOD_ID and ops.METHOD_ID['dopri5'] == 3
    assert ops.METHOD_ID['euler'] == 0 and ops.METHOD_ID['rk4'] == 1 and ops.METHOD_ID['midpoint'] == 2


def test_refused_solver_names_say_why():
    from vae_gp_ode_amd import _lib, ops
    from vae_gp_ode_amd.main import SOLVERS
    from vae_gp_ode_amd.model.core.flow import Flow
    refused = ('bdf', 'adams', 'explicit_adams', 'fixed_adams')
    assert sorted(ops.REFUSED_SOLVERS) == sorted(refused)
    assert set(SOLVERS) <= set(ops.METHOD_ID) | set(refused)             # every name of the --solver list is either built or refused
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in refused:
        with pytest.raises(_lib.GpodeError) as e:
            ops.check_solver(name)
        assert name in str(e.value) and ops.REFUSED_SOLVERS[name] in str(e.value)
        with pytest.raises(ValueError):
            Flow(None, solver=name)(None, None)
        assert re.search(r'`%s`' % name, doc), name
    ops.check_solver('dopri5')


def test_header_declares_the_adaptive_entry_points():
    from vae_gp_ode_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gpode.h')).read()
    for sym in ('gpode_rollout_adaptive_fwd_n', 'gpode_rollout_adaptive_bwd_n'):
        assert re.search(r'\bint\s+%s\s*\(' % sym, hdr) and sym in _lib.SIGNATURES
    assert re.search(r'#define\s+GPODE_METHOD_MIDPOINT\s+2\b', hdr) and re.search(r'#define\s+GPODE_METHOD_DOPRI5\s+3\b', hdr)


def test_num_evals_sources_do_not_fight():
    """A pending host-side count of an earlier solve must not overwrite a count that load_state_dict brought in."""
    from vae_gp_ode_amd.model.core.flow import ODEfunc
    a, b = ODEfunc(None, 1), ODEfunc(None, 1)
    a._set_evals(24)
    sd = a.state_dict()
    assert sd['_num_evals'].item() == 24
    b._set_evals(7)
    b.load_state_dict(sd)
    assert b.num_evals() == 24
    b._set_counts(torch.tensor([[3, 1, 0, 25], [4, 0, 0, 31]], dtype=torch.int32))
    assert b.num_evals() == 31 and b.state_dict()['_num_evals'].item() == 31
    b._set_counts(torch.tensor([[3, 1, 0, 25]], dtype=torch.int32))
    b.load_state_dict(sd)
    assert b.num_evals() == 24


@pytest.mark.parametrize('name,kernel,order', R.CASES)
@pytest.mark.parametrize('tol', R.TOLS)
def test_gpu_case_inputs_exercise_the_controller(name, kernel, order, tol):
    """The fixture's z0 with its stretched, non-uniform ts on the fp64 oracle right-hand side: some interval takes two or more
    accepted steps, some step is rejected, and nobody exhausts the default budget of 4 (T - 1)."""
    g, f = R.oracle_rhs(name, kernel, order)
    ts = R.case_ts(name, g['ts'].shape[0])
    assert (torch.diff(ts) > 0).all() and torch.diff(ts).max() > 3 * torch.diff(ts).min()
    zt, hs, ie, cnt = R.solve(f, g['z0'].double(), ts, tol, tol)
    per = torch.diff(torch.cat([torch.zeros(ie.shape[0], 1, dtype=torch.long), ie], 1), dim=1)
    assert (cnt[:, 2] == 0).all() and torch.isfinite(zt).all()
    assert per.max() >= 2 and per.min() >= 1 and cnt[:, 1].sum() >= 1
    assert cnt[:, 0].max() <= 4 * (ts.shape[0] - 1) - 2, 'no margin to the default budget left for the fp32 kernel'
    assert math.isclose(ts[-1].item(), R.TS_SHAPE[ts.shape[0] - 1] * R.TS_SCALE[name], rel_tol=1e-6)
