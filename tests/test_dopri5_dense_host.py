"""CPU: the dense-output reference helper (tests/dopri5_dense_ref.py) -- the interpolant's order conditions in exact arithmetic, its
convergence, replay against solve, the reverse recursion against autograd -- a proof that the inputs of the GPU tests exercise the
feature, and the host surface of Flow(dense_output=...)."""
import math
from fractions import Fraction

import pytest
import torch

import dopri5_dense_ref as DR
import dopri5_ref as R

THETAS = [Fraction(1, 4), Fraction(1, 3), Fraction(1, 2), Fraction(3, 4), Fraction(1)]


def _tableau():
    F = lambda v: Fraction(v).limit_denominator(10 ** 7)
    A = [[F(a) for a in row] + [Fraction(0)] * (7 - len(row)) for row in R.A]
    c = [sum(row) for row in A]
    return A, c


@pytest.mark.parametrize('th', THETAS)
def test_order_conditions_up_to_four_hold_exactly(th):
    """The eight order conditions of a continuous method of order 4 at theta (Hairer, Noersett, Wanner II.6):
    sum w = th, sum w c = th^2/2, sum w c^2 = th^3/3, sum w a c = th^3/6, sum w c^3 = th^4/4, sum w c a c = th^4/8,
    sum w a c^2 = th^4/12, sum w a a c = th^4/24."""
    A, c = _tableau()
    wt = DR.w(th, DR.B_FRAC, DR.D_FRAC)
    Ac = [sum(A[i][j] * c[j] for j in range(7)) for i in range(7)]
    Ac2 = [sum(A[i][j] * c[j] ** 2 for j in range(7)) for i in range(7)]
    AAc = [sum(A[i][j] * Ac[j] for j in range(7)) for i in range(7)]
    dot = lambda u: sum(a * b for a, b in zip(wt, u))
    assert dot([1] * 7) == th
    assert dot(c) == th ** 2 / 2
    assert dot([x ** 2 for x in c]) == th ** 3 / 3
    assert dot(Ac) == th ** 3 / 6
    assert dot([x ** 3 for x in c]) == th ** 4 / 4
    assert dot([x * y for x, y in zip(c, Ac)]) == th ** 4 / 8
    assert dot(Ac2) == th ** 4 / 12
    assert dot(AAc) == th ** 4 / 24


def test_end_point_and_end_slopes_of_the_weights():
    """w(1) = b, w'(0) = e_1, w'(1) = e_7: the quartic is the Hermite interpolant through (y_n, k_1) and (y_{n+1}, k_7); and
    w(1/2) is the midpoint rule torchdiffeq fits its quartic through."""
    assert DR.w(Fraction(1), DR.B_FRAC, DR.D_FRAC) == DR.B_FRAC
    assert DR.w(Fraction(0), DR.B_FRAC, DR.D_FRAC) == [0] * 7
    assert DR.dw(Fraction(0)) == [1, 0, 0, 0, 0, 0, 0]
    assert DR.dw(Fraction(1)) == [0, 0, 0, 0, 0, 0, 1]
    F = lambda v: Fraction(v).limit_denominator(10 ** 7)
    assert [F(b) for b in R.B5] == DR.B_FRAC
    assert all(abs(a - float(b)) < 1e-16 for a, b in zip(DR.D, DR.D_FRAC))
    # dw is the derivative of w: central differences of the exact quartic are exact up to O(e^2) terms of known size
    e = Fraction(1, 10 ** 6)
    for th in (Fraction(1, 3), Fraction(3, 4)):
        num = [(a - b) / (2 * e) for a, b in zip(DR.w(th + e, DR.B_FRAC, DR.D_FRAC), DR.w(th - e, DR.B_FRAC, DR.D_FRAC))]
        assert all(abs(x - y) < Fraction(1, 10 ** 9) for x, y in zip(num, DR.dw(th)))
    # fp64 weights agree with the exact ones
    for th in (0.25, 0.5, 1.0):
        assert all(abs(a - float(b)) < 1e-15 for a, b in zip(DR.w(th), DR.w(Fraction(th), DR.B_FRAC, DR.D_FRAC)))


def test_interpolation_error_of_one_step_falls_with_h5():
    """One step on the oracle's right-hand side, output at theta = 1/2, against fp64 rk4 with 256 sub-steps: local order 5.  The
    step sizes lie in the asymptotic range of this right-hand side (lengthscale 2: above h = 0.4 the next term of the error
    expansion still shows) and above the rounding floor (error 1e-11 at h = 0.05)."""
    from oracle import gpode_oracle as O
    g, f = R.oracle_rhs('gp_rbf1_tiny', 'RBF', 1)
    y0 = g['z0'].double()
    errs = []
    for h in (0.4, 0.2, 0.1, 0.05):
        ynew, _, _, ks = R.step(f, y0, h)
        z = DR.interpolate(y0, h, ks, 0.5)
        fine = torch.linspace(0, h / 2, 257, dtype=torch.float64)
        truth = O.odeint_fixed(f, y0, fine, 'rk4')[-1]
        errs.append((z - truth).abs().max().item())
    slopes = [math.log2(a / b) for a, b in zip(errs, errs[1:])]
    print('errors %s slopes %s' % (errs, slopes))
    assert len(slopes) == 3 and all(4.5 < s < 5.5 for s in slopes), (errs, slopes)


def oscillator(y):
    return torch.stack([y[:, 1], -y[:, 0]], 1)


def test_solve_dense_steps_freely_and_meets_the_tolerance():
    y0 = torch.tensor([[1.0, 0.0], [0.0, 2.0], [3.0, -1.0]], dtype=torch.float64)
    ts = DR.G1.double()
    zt, hs, ie, th, cnt = DR.solve_dense(oscillator, y0, ts, 1e-6, 1e-6)
    assert (cnt[:, 2] == 0).all() and (cnt[:, 3] == 1 + 6 * (cnt[:, 0] + cnt[:, 1])).all()
    assert (cnt[:, 0] < 15).all() and (ie[:, -1] == cnt[:, 0]).all() and (torch.diff(ie, dim=1) >= 0).all() and (ie >= 1).all()
    assert (th > 0).all() and (th <= 1).all() and (th[:, -1] == 1).all()
    assert ((hs.sum(1) - 1.5).abs() < 1e-14).all()
    rot = torch.stack([torch.stack([torch.cos(ts), torch.sin(ts)], -1), torch.stack([-torch.sin(ts), torch.cos(ts)], -1)], -2)
    want = torch.einsum('tij,nj->nti', rot, y0)
    assert (zt - want).abs().max() < 200 * 1e-6
    # budget, and a decreasing grid
    K = int(cnt[:, 0].max()) - 1
    z2, _, i2, t2, c2 = DR.solve_dense(oscillator, y0, ts, 1e-6, 1e-6, max_steps=K)
    for n in range(3):
        if cnt[n, 0] > K:
            first = int((ie[n] > K).nonzero()[0])
            assert c2[n, 2] == 1 and c2[n, 0] == K and torch.isnan(z2[n, first + 1:]).all() and torch.equal(z2[n, :first + 1], zt[n, :first + 1])
            assert (i2[n, first:] == K).all() and (t2[n, first:] == 1).all()
        else:
            assert c2[n, 2] == 0 and torch.equal(z2[n], zt[n])
    assert (DR.solve_dense(oscillator, y0, ts.flip(0), 1e-6, 1e-6)[4][:, 2] == 3).all()


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_replay_reproduces_what_solve_recorded(dtype):
    g, f = R.oracle_rhs('gp_df1_tiny', 'DF', 1, dtype)
    y0 = g['z0'].to(dtype)
    for ts in (DR.G1, R.case_ts('gp_df1_tiny', 5)):
        zt, hs, ie, th, cnt = DR.solve_dense(f, y0, ts, 1e-4, 1e-4, max_steps=32)
        assert (cnt[:, 2] == 0).all()
        # trajectory by trajectory the replay evaluates f on the very inputs of the solve (which carried the FSAL slope over
        # instead of evaluating it again): the same bits
        for n in range(y0.shape[0]):
            aux = {}
            z2 = DR.replay_dense(f, y0[n:n + 1], hs[n:n + 1], ie[n:n + 1], th[n:n + 1], aux)
            assert z2.dtype == dtype and torch.equal(z2, zt[n:n + 1]), n
            assert len(aux['xs']) == hs.shape[1] and len(aux['xs'][0]) == 7 and len(aux['ks'][0]) == 7


def test_reverse_recursion_equals_autograd_through_the_replay():
    """The recursion the kernel implements, restated in torch (dopri5_dense_ref.reverse_sweep), on a record with several outputs per
    step, steps without an output, and interior as well as end-point outputs."""
    torch.manual_seed(0)
    Wm = torch.randn(3, 3, dtype=torch.float64) * 0.7
    f = lambda y: torch.tanh(y @ Wm.T) - 0.3 * y
    N, K = 2, 4
    hs = torch.tensor([[0.3, 0.2, 0.4, 0.0], [0.5, 0.1, 0.2, 0.1]], dtype=torch.float64)
    ie = torch.tensor([[1, 1, 3, 3, 3], [1, 2, 2, 2, 4]])                    # step 2 of trajectory 0 and step 3 of trajectory 1 hold none
    th = torch.tensor([[0.3, 0.9, 0.5, 0.2, 1.0], [1.0, 0.25, 0.5, 1.0, 1.0]], dtype=torch.float64)
    y0 = torch.randn(N, 3, dtype=torch.float64, requires_grad=True)
    gw = torch.randn(N, 6, 3, dtype=torch.float64)
    aux = {}
    zt = DR.replay_dense(f, y0, hs, ie, th, aux)
    ks = [k for st in aux['ks'] for k in st]
    grads = torch.autograd.grad((zt * gw).sum(), [y0] + ks, allow_unused=True)
    gk = torch.stack([torch.zeros(N, 3, dtype=torch.float64) if x is None else x for x in grads[1:]], 1).view(N, K, 7, 3)
    xs = torch.stack([torch.stack(x, 1) for x in aux['xs']], 1).detach()      # (N,K,7,D)

    def vjp(x, a):
        x = x.clone().requires_grad_(True)
        return torch.autograd.grad(f(x[None])[0], x, a)[0]
    gz0, ak = DR.reverse_sweep(vjp, xs, hs, ie, th, gw)
    assert (gz0 - grads[0]).abs().max() < 1e-14 * grads[0].abs().max()
    live = (torch.arange(K)[None] < ie[:, -1:])[:, :, None, None]
    assert ((ak - gk * live).abs().max() < 1e-14 * gk.abs().max())
    assert (ak[0, 1, 6] == 0).all() and (ak[1, 0, 6] == 0).all() and ak[0, 0, 6].abs().max() > 0     # row 7 only with an interior output


_SOLVES = {}


def solved(name, kernel, order, which, tol):
    """fp64 solve_dense of one GPU test case: counts (N,4) and the outputs held per step (N,K); computed once."""
    key = (name, which, tol)
    if key not in _SOLVES:
        g, f = R.oracle_rhs(name, kernel, order)
        ts = DR.grid(name, which)
        zt, hs, ie, th, cnt = DR.solve_dense(f, g['z0'].double(), ts, tol, tol, max_steps=32)
        assert (cnt[:, 2] == 0).all() and torch.isfinite(zt).all()
        _SOLVES[key] = (cnt, torch.stack([(ie == i + 1).sum(1) for i in range(hs.shape[1])], 1), ts.shape[0])
    return _SOLVES[key]


@pytest.mark.parametrize('name,kernel,order', R.CASES)
def test_gpu_case_inputs_exercise_the_dense_mode(name, kernel, order):
    """In fp64 on the oracle's right-hand side, for every fixture: on G1 at 1e-3 every trajectory needs fewer accepted steps than
    outputs (at most 7) and some step on G1 holds at least 4 outputs; on G2 some accepted step holds no output (both tolerances); some
    grid x tolerance has a rejection, G2 at 1e-5 always; nobody needs more than 15 accepted steps on G2 (budget of the GPU tests: 32,
    default 16)."""
    rejected, most_g1 = {}, 0
    for which in DR.GRIDS:
        for tol in R.TOLS:
            cnt, held, T = solved(name, kernel, order, which, tol)
            livem = torch.arange(held.shape[1])[None] < cnt[:, :1]
            rejected[which, tol] = int(cnt[:, 1].sum())
            if which == 'G1':
                if tol == 1e-3:
                    assert (cnt[:, 0] < T - 1).all() and cnt[:, 0].max() <= 7, cnt[:, 0]
                most_g1 = max(most_g1, int(held.max()))
            else:
                assert (held[livem] == 0).any()
                assert cnt[:, 0].max() <= 15
    assert most_g1 >= 4, 'on G1 some step holds at least 4 outputs'
    assert sum(rejected.values()) >= 1 and rejected['G2', 1e-5] >= 1, rejected


def test_on_g2_some_steps_hold_two_outputs():
    """G2 at 1e-3: a step that holds two outputs exists for gp_rbf1_tiny, gp_rbf2_tiny and gp_df1_tiny_q5.  It does not for gp_df1_tiny
    (steps of 0.1 .. 0.3 against intervals of 0.09, 0.36, 0.15, 0.75: at most one output per step); that fixture's steps with several
    outputs are those of G1."""
    two = {name: int(solved(name, kernel, order, 'G2', 1e-3)[1].max()) >= 2 for name, kernel, order in R.CASES}
    assert [n for n, v in two.items() if v] == ['gp_rbf1_tiny', 'gp_rbf2_tiny', 'gp_df1_tiny_q5'], two


def test_flow_takes_dense_output_from_the_argument_or_the_environment(monkeypatch):
    from vae_gp_ode_amd.model.core.flow import Flow
    monkeypatch.delenv('GPODE_DOPRI5_DENSE', raising=False)
    assert Flow(None).dense_output is False and Flow(None, dense_output=True).dense_output is True
    monkeypatch.setenv('GPODE_DOPRI5_DENSE', '0')
    assert Flow(None).dense_output is False
    monkeypatch.setenv('GPODE_DOPRI5_DENSE', '1')
    assert Flow(None).dense_output is True and Flow(None, dense_output=False).dense_output is False
    fl = Flow(None, solver='rk4', dense_output=True)                         # ignored by a fixed-grid solver, as the tolerances are
    assert fl.solver == 'rk4' and fl.dense_output is True


def test_header_and_binding_table_declare_the_dense_entry_points():
    import os
    import re
    from vae_gp_ode_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'gpode.h')).read()
    for sym in ('gpode_rollout_dense_fwd_n', 'gpode_rollout_dense_bwd_n'):
        assert re.search(r'\bint\s+%s\s*\(' % sym, hdr) and sym in _lib.SIGNATURES
    assert ops.NSTAGE['dopri5'] == 6 and ops.NSTAGE_DENSE == 7
