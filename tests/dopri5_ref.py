"""Reference for the adaptive Dormand-Prince 5(4) solver (torch, fp64 or fp32 by the dtype of y0, differentiable), written
independently of the kernel source: the tableau (Hairer, Noersett, Wanner, Solving ODEs I, table II.5.2), ``replay`` (integrate with
GIVEN step sizes -- what the gradient is defined through) and ``solve`` (the controller the kernel specifies).

Controller, per trajectory (state y of D components, f autonomous):
  err   = h sum_j E_j k_j;  ratio = sqrt(mean_i (err_i / (atol + rtol max(|y_i|, |ynew_i|)))^2);  accept iff ratio <= 1
  h_new = h clamp(0.9 ratio^(-1/5), 0.2, 10), not above h on the first accepted step after a rejection
  first step: min(100 h0, (0.01 / d1)^(1/5), ts[1] - ts[0]), h0 = 0.01 d0 / d1, d0 = ||y0||, d1 = ||f(y0)|| in the scaled RMS norm
              (Hairer's estimate II.4 without the second-derivative probe: no evaluation beyond f(y0), which is k1 of step one)
  landing: with ``rem`` left to the next output time, a proposal with 1.01 h >= rem becomes rem; after such a cut step the larger of
           the uncut proposal and the controller's is carried on.  No dense output: every zt[:, t] is a step end point.
  failure: max_steps accepted steps taken and more needed -> status 1; step <= 16 eps max(|t|, |h|) -> status 2; the trajectory
           is NaN from the output it did not reach.
"""
import torch

# c_i = sum_j A[i][j]; row 6 is b (the 5th-order weights; first-same-as-last)
A = [[],
     [1 / 5],
     [3 / 40, 9 / 40],
     [44 / 45, -56 / 15, 32 / 9],
     [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
     [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
     [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]]
C = [0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1, 1]
B5 = [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0]
B4 = [5179 / 57600, 0, 7571 / 16695, 393 / 640, -92097 / 339200, 187 / 2100, 1 / 40]
E = [b5 - b4 for b5, b4 in zip(B5, B4)]


def step(f, y, h, k1=None):
    """One step of size h ((N,1) or scalar) from y (N,D): -> ynew, err, the stage inputs [x1..x6], the slopes [k1..k7]."""
    ks = [f(y) if k1 is None else k1]
    xs = [y]
    for s in range(1, 7):
        x = y + h * sum(a * k for a, k in zip(A[s], ks) if a != 0)
        if s < 6:
            xs.append(x)
        ks.append(f(x))
    ynew = x
    err = h * sum(e * k for e, k in zip(E, ks) if e != 0)
    return ynew, err, xs, ks


def replay(f, y0, ts, hstep, iend, aux=None):
    """Integrate with the given steps: hstep (N,K) (0 past a trajectory's count: a step that changes nothing), iend (N,T-1) the
    number of steps taken when output t+1 is reached.  -> zt (N,T,D).  ``aux`` (a dict) receives 'xs' (K lists of six stage
    inputs) and 'ks' (K lists of the six slopes that enter the step) for callers that differentiate w.r.t. them."""
    N, K = hstep.shape
    y = y0
    states = [y0]
    all_x, all_k = [], []
    for i in range(K):
        y, _, xs, ks = step(f, y, hstep[:, i:i + 1].to(y0.dtype))
        states.append(y)
        all_x.append(xs)
        all_k.append(ks[:6])
    if aux is not None:
        aux['xs'], aux['ks'] = all_x, all_k
    S = torch.stack(states, 1)                                                   # (N,K+1,D)
    idx = torch.cat([torch.zeros(N, 1, dtype=torch.long), iend.long()], 1)       # (N,T)
    return torch.gather(S, 1, idx.unsqueeze(-1).expand(-1, -1, y0.shape[1]))


def _rms(v, sc):
    return ((v / sc) ** 2).mean(1).sqrt()


def solve(f, y0, ts, rtol, atol, max_steps=None):
    """The controller above, every trajectory on its own (vectorised: one round = one attempted step of every unfinished
    trajectory).  -> zt (N,T,D), hstep (N,K), iend (N,T-1) int64, counts (N,4) int64 = accepted, rejected, status, evaluations."""
    dt_, N, T = y0.dtype, y0.shape[0], ts.shape[0]
    ts = ts.to(dt_)
    K = 4 * (T - 1) if max_steps is None else max_steps
    eps = torch.finfo(dt_).eps
    zt = torch.full((N, T, y0.shape[1]), float('nan'), dtype=dt_)
    zt[:, 0] = y0
    hstep, iend = torch.zeros(N, K, dtype=dt_), torch.zeros(N, max(T - 1, 0), dtype=torch.long)
    nacc, nrej, status = (torch.zeros(N, dtype=torch.long) for _ in range(3))
    nfe = torch.ones(N, dtype=torch.long)
    if T == 1:
        return zt, hstep, iend, torch.stack([nacc, nrej, status, nfe], 1)
    y, k1 = y0.clone(), f(y0)
    sc = atol + rtol * y.abs()
    d0, d1 = _rms(y, sc), _rms(k1, sc)
    h0 = torch.where((d0 < 1e-5) | (d1 < 1e-5), torch.full_like(d0, 1e-6), 0.01 * d0 / d1)
    h1 = torch.where(d1 <= 1e-15, torch.clamp(h0 * 1e-3, min=1e-6), (0.01 / d1) ** 0.2)
    h = torch.minimum(torch.minimum(100 * h0, h1), (ts[1] - ts[0]).expand(N))
    tix = torch.zeros(N, dtype=torch.long)
    rem = (ts[1] - ts[0]).expand(N).clone()
    after_rej = torch.zeros(N, dtype=torch.bool)
    done = torch.zeros(N, dtype=torch.bool)
    ar = torch.arange(N)
    while not done.all():
        tabs = torch.maximum(ts[tix].abs(), ts[tix + 1].abs())
        cut = 1.01 * h >= rem
        hs = torch.where(cut, rem, h)
        fail1 = ~done & (nacc >= K)
        fail2 = ~done & ~fail1 & ~(hs > 16 * eps * torch.maximum(tabs, hs.abs()))
        status[fail1], status[fail2] = 1, 2
        done = done | fail1 | fail2
        if done.all():
            break
        act = ~done
        hs = torch.where(act, hs, torch.zeros_like(hs))
        ynew, err, _, ks = step(f, y, hs.unsqueeze(1), k1)
        nfe[act] += 6
        ratio = _rms(err, atol + rtol * torch.maximum(y.abs(), ynew.abs()))
        fac = torch.clamp(0.9 * ratio ** -0.2, 0.2, 10.0)
        fac = torch.where(torch.isnan(fac), torch.full_like(fac, 0.2), fac)
        acc = act & (ratio <= 1)
        rej = act & ~acc
        fac = torch.where(acc & after_rej, torch.clamp(fac, max=1.0), fac)
        y = torch.where(acc.unsqueeze(1), ynew, y)
        k1 = torch.where(acc.unsqueeze(1), ks[6], k1)
        hstep[ar[acc], nacc[acc]] = hs[acc]
        nacc = nacc + acc.long()
        nrej = nrej + rej.long()
        h = torch.where(acc, torch.where(cut, torch.maximum(h, hs * fac), hs * fac), torch.where(rej, hs * fac, h))
        after_rej = (after_rej & ~acc) | rej
        land = acc & cut
        zt[ar[land], tix[land] + 1] = y[land]
        iend[ar[land], tix[land]] = nacc[land]
        rem = torch.where(acc & ~cut, rem - hs, rem)
        tix = tix + land.long()
        done = done | (tix >= T - 1)
        tix = tix.clamp(max=T - 2)
        nxt = land & ~done
        rem = torch.where(nxt, ts[tix + 1] - ts[tix], rem)
    for n in range(N):                       # outputs a failed trajectory did not reach count as reached at its last step
        if status[n] != 0:
            iend[n, tix[n]:] = nacc[n]
    return zt, hstep, iend, torch.stack([nacc, nrej, status, nfe], 1)


# ---- the inputs of the GPU tests (tests/test_gpu_dopri5.py); tests/test_dopri5_host.py proves on the CPU that they exercise the
# controller: fixture, kernel, order.  ts: the fixture's grid stretched and made non-uniform
CASES = [('gp_rbf1_tiny', 'RBF', 1), ('gp_rbf2_tiny', 'RBF', 2), ('gp_df1_tiny', 'DF', 1), ('gp_df1_tiny_q5', 'DF', 1)]
TOLS = (1e-3, 1e-5)
TS_SHAPE = (0.0, 0.3, 1.5, 2.0, 4.5)          # intervals of 0.3, 1.2, 0.5, 2.5 time units ...
TS_SCALE = {'gp_rbf1_tiny': 1.0, 'gp_rbf2_tiny': 0.8, 'gp_df1_tiny': 0.3, 'gp_df1_tiny_q5': 0.7}   # ... times this


def case_ts(name, T):
    return (torch.tensor(TS_SHAPE[:T], dtype=torch.float64) * TS_SCALE[name]).float()


_F64 = {}


def oracle_rhs(name, kernel, order, dtype=torch.float64):
    """f of the fixture's function draw from the CPU oracle, in ``dtype``; cached."""
    from conftest import load_golden, sub
    from oracle import gpode_oracle as O
    key = (name, dtype)
    if key not in _F64:
        g = load_golden(name)
        p = O.to_dtype(O.gp_params_from_state_dict(sub(g, 'sd.')), dtype)
        c = O.build_cache(p, O.to_dtype(sub(g, 'noise.'), dtype), kernel)
        _F64[key] = (g, lambda y: O.ode_rhs(y, c, order))
    return _F64[key]
