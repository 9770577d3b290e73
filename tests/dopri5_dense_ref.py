"""Reference for the DENSE-OUTPUT mode of the adaptive Dormand-Prince solver (torch, differentiable), written independently of the
kernel source; the tableau, ``step`` and the fixtures come from tests/dopri5_ref.py.

Interpolant: the 4th-order continuous extension of the pair (Shampine; Hairer, Noersett, Wanner, Solving ODEs I, II.6, CONTD5).
With theta = (t - t_n) / h in (0, 1] and k_1 .. k_7 the slopes of the accepted step (k_7 = f(y_{n+1}), the FSAL slope):
  z(theta) = y_n + h sum_j w_j(theta) k_j
  w_j(theta) = theta [b_j + (1 - theta) ((d_j1 - b_j) + theta ((2 b_j - d_j1 - d_j7) + (1 - theta) D_j))]       (b_7 = 0)

Controller: the one of dopri5_ref.solve, with two changes -- ``rem`` is the distance to the LAST output time (one cut, at the end),
and the first step is capped by ts[-1] - ts[0].  After a step t_n -> t_n + h is accepted every output not yet written with
ts[j] - ts[0] <= t_n + h belongs to it (all that are left when it is the cut step); the last output is the end state of the last
step, theta = 1.  Time is the running sum of the accepted steps, an offset from ts[0], in the dtype of y0.
Record: hstep (N,K), istep (N,T-1) = 1-based number of the accepted step that holds output t+1, theta (N,T-1); outputs a failed
trajectory did not reach: istep = its count of accepted steps, theta = 1.
"""
from fractions import Fraction

import torch

import dopri5_ref as R

D_FRAC = [Fraction(-12715105075, 11282082432), Fraction(0), Fraction(87487479700, 32700410799), Fraction(-10690763975, 1880347072),
          Fraction(701980252875, 199316789632), Fraction(-1453857185, 822651844), Fraction(69997945, 29380423)]
B_FRAC = [Fraction(35, 384), Fraction(0), Fraction(500, 1113), Fraction(125, 192), Fraction(-2187, 6784), Fraction(11, 84), Fraction(0)]
D = [float(d) for d in D_FRAC]


def w(theta, b=R.B5, d=D):
    """The seven weights at theta (a number, a Fraction with b=B_FRAC, d=D_FRAC, or a tensor)."""
    out = []
    for j in range(7):
        d1, d7 = (1 if j == 0 else 0), (1 if j == 6 else 0)
        out.append(theta * (b[j] + (1 - theta) * ((d1 - b[j]) + theta * ((2 * b[j] - d1 - d7) + (1 - theta) * d[j]))))
    return out


def dw(theta, b=B_FRAC, d=D_FRAC):
    """d w_j / d theta, from the expanded quartic w_j = c1 th + c2 th^2 + c3 th^3 + c4 th^4."""
    out = []
    for j in range(7):
        d1, d7 = (1 if j == 0 else 0), (1 if j == 6 else 0)
        p, q, r = d1 - b[j], 2 * b[j] - d1 - d7, d[j]
        # w = th [b + (1-th)(p + th (q + (1-th) r))] = th b + th(1-th) p + th^2 (1-th) q + th^2 (1-th)^2 r
        out.append(b[j] + (1 - 2 * theta) * p + (2 * theta - 3 * theta ** 2) * q + (2 * theta - 6 * theta ** 2 + 4 * theta ** 3) * r)
    return out


def interpolate(y, h, ks, theta):
    """z(theta) of one step: y (N,D), h and theta (N,1) or scalars, ks the seven slopes."""
    return y + h * sum(wj * k for wj, k in zip(w(theta), ks))


def replay_dense(f, y0, hstep, istep, theta, aux=None):
    """Integrate with the GIVEN steps hstep (N,K) (0 past a trajectory's count) and evaluate the outputs with the GIVEN istep, theta
    (N,T-1): -> zt (N,T,D), zt[:, 0] = y0.  theta = 1 reads the end state of the step; istep = 0 the initial state.  ``aux`` (a dict)
    receives 'xs' (K lists of the seven stage inputs, the seventh = the end state) and 'ks' (K lists of the seven slopes)."""
    dt_ = y0.dtype
    N, K = hstep.shape
    T1 = istep.shape[1]
    y = y0
    outs = [y0] * T1
    all_x, all_k = [], []
    for i in range(K):
        h = hstep[:, i:i + 1].to(dt_)
        ynew, _, xs, ks = R.step(f, y, h)
        for t in range(T1):
            m = (istep[:, t] == i + 1).unsqueeze(1)
            if m.any():
                th = theta[:, t:t + 1].to(dt_)
                z = torch.where(th >= 1, ynew, interpolate(y, h, ks, th))
                outs[t] = torch.where(m, z, outs[t])
        all_x.append(xs + [ynew])
        all_k.append(ks)
        y = ynew
    if aux is not None:
        aux['xs'], aux['ks'] = all_x, all_k
    return torch.stack([y0] + outs, 1)


def _rms(v, sc):
    return ((v / sc) ** 2).mean().sqrt()


def solve_dense(f, y0, ts, rtol, atol, max_steps=None):
    """The controller above, one trajectory after the other.  -> zt (N,T,D), hstep (N,K), istep (N,T-1) int64, theta (N,T-1),
    counts (N,4) int64 = accepted, rejected, status (1 budget, 2 step underflow, 3 ts not increasing), evaluations."""
    dt_, N, T = y0.dtype, y0.shape[0], ts.shape[0]
    ts = ts.to(dt_)
    K = 4 * (T - 1) if max_steps is None else max_steps
    eps = torch.finfo(dt_).eps
    zt = torch.full((N, T, y0.shape[1]), float('nan'), dtype=dt_)
    zt[:, 0] = y0
    hstep, theta = torch.zeros(N, K, dtype=dt_), torch.zeros(N, max(T - 1, 0), dtype=dt_)
    istep = torch.zeros(N, max(T - 1, 0), dtype=torch.long)
    counts = torch.zeros(N, 4, dtype=torch.long)
    counts[:, 3] = 1
    if T == 1:
        return zt, hstep, istep, theta, counts
    to = ts - ts[0]
    tend, tabs = to[-1], torch.maximum(ts[0].abs(), ts[-1].abs())
    increasing = bool((torch.diff(ts) > 0).all())
    for n in range(N):
        y = y0[n:n + 1]
        k1 = f(y)
        nacc = nrej = status = 0
        nfe, jout = 1, 1
        if not increasing:
            status = 3
        sc = atol + rtol * y.abs()
        d0, d1 = _rms(y, sc), _rms(k1, sc)
        h0 = torch.tensor(1e-6, dtype=dt_) if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
        h1 = torch.clamp(h0 * 1e-3, min=1e-6) if d1 <= 1e-15 else (0.01 / d1) ** 0.2
        h = torch.minimum(torch.minimum(100 * h0, h1), tend)
        tn = torch.zeros((), dtype=dt_)
        after_rej = False
        while not status:
            if nacc >= K:
                status = 1
                break
            rem = tend - tn
            cut = bool(1.01 * h >= rem)
            hs = rem if cut else h
            if not bool(hs > 16 * eps * torch.maximum(tabs, hs.abs())):
                status = 2
                break
            ynew, err, _, ks = R.step(f, y, hs, k1)
            nfe += 6
            ratio = _rms(err, atol + rtol * torch.maximum(y.abs(), ynew.abs()))
            fac = torch.clamp(0.9 * ratio ** -0.2, 0.2, 10.0)
            if torch.isnan(fac):
                fac = torch.tensor(0.2, dtype=dt_)
            if bool(ratio <= 1):
                if after_rej:
                    fac = torch.clamp(fac, max=1.0)
                after_rej = False
                tnew = tn + hs
                while jout < T and (cut or bool(to[jout] <= tnew)):
                    last = jout == T - 1
                    th = torch.ones((), dtype=dt_) if last else torch.clamp((to[jout] - tn) / hs, eps, 1.0)
                    zt[n, jout] = (ynew if last else interpolate(y, hs, ks, th))[0]
                    istep[n, jout - 1], theta[n, jout - 1] = nacc + 1, th
                    jout += 1
                hstep[n, nacc] = hs
                nacc += 1
                y, k1, tn, h = ynew, ks[6], tnew, hs * fac
                if cut:
                    break
            else:
                nrej += 1
                after_rej = True
                h = hs * fac
        if status:
            istep[n, jout - 1:], theta[n, jout - 1:] = nacc, 1.0
        counts[n] = torch.tensor([nacc, nrej, status, nfe])
    return zt, hstep, istep, theta, counts


def reverse_sweep(vjp, xs, hstep, istep, theta, gzt):
    """The reverse recursion of the kernel, restated: vjp(x, a) = J_F(x)^T a.  xs (N,K,7,D), gzt (N,T,D) -> gz0 (N,D) and the
    adjoints of the seven slopes (N,K,7,D).  Walks the steps backwards; at step i, with lam the adjoint of its end state:
      G0 = sum_o g_o, S_j = h sum_o w_j(theta_o) g_o over the outputs o of the step;  if some theta_o < 1: lam += J(x_7)^T S_7
      ak_j = h b_j lam + S_j (j = 1..6);  for j = 6..1: g = J(x_j)^T ak_j, lam += g, ak_l += h a_jl g (l < j);  lam += G0"""
    N, K = hstep.shape
    T = gzt.shape[1]
    gz0 = torch.zeros_like(gzt[:, 0])
    ak_all = torch.zeros(N, K, 7, gzt.shape[2], dtype=gzt.dtype)
    for n in range(N):
        lam = torch.zeros_like(gzt[n, 0])
        nacc = int(istep[n, -1]) if T > 1 else 0
        for i in range(nacc, 0, -1):
            h = hstep[n, i - 1]
            outs = [t for t in range(T - 1) if istep[n, t] == i]
            G0 = sum((gzt[n, t + 1] for t in outs), torch.zeros_like(lam))
            S = [torch.zeros_like(lam) for _ in range(7)]
            for t in outs:
                for j, wj in enumerate(w(theta[n, t])):
                    S[j] = S[j] + h * wj * gzt[n, t + 1]
            if any(theta[n, t] < 1 for t in outs):
                ak_all[n, i - 1, 6] = S[6]
                lam = lam + vjp(xs[n, i - 1, 6], S[6])
            ak = [h * R.B5[j] * lam + S[j] for j in range(6)]
            for j in range(5, -1, -1):
                ak_all[n, i - 1, j] = ak[j]
                g = vjp(xs[n, i - 1, j], ak[j])
                lam = lam + g
                for l in range(j):
                    ak[l] = ak[l] + h * R.A[j][l] * g
            lam = lam + G0
        for t in range(T - 1):
            if istep[n, t] == 0:
                lam = lam + gzt[n, t + 1]
        gz0[n] = lam + gzt[n, 0]
    return gz0, ak_all


# ---- grids of the dense tests
G1 = (0.1 * torch.arange(16, dtype=torch.float64)).float()          # the reference's training grid: dt = 0.1, T = 16


def grid(name, which):
    """'G1': the training grid; 'G2': the stretched, non-uniform grid of the landing tests."""
    return G1 if which == 'G1' else R.case_ts(name, 5)


GRIDS = ('G1', 'G2')
