"""Posterior-predictive evaluation of a trained model: what the reference's evaluation notebooks compute from a checkpoint
(experiments/plots_dynamics.ipynb cell 13, ``compute_mse_std``: model in ``eval()``, encode, L function draws, integrate, decode,
``torch.mean`` / ``torch.std`` of the squared error over every draw, sequence, frame and pixel) and the long roll-out of
create_plots.py:19-23 (``odegpvae(test_batch, T_custom=Troll*T)``), plus the predictive mean and variance over the draws.

The decoder runs frozen (``Decoder.decode_frozen_raw``: running statistics as tables, BatchNorm + ReLU folded into the transposed
convolutions) and its last stage is ``gpode_dec10_predict``: the sigmoid, the squared error and every reduction over draws and
pixels happen in the registers of the convolution's epilogue, so neither the (L,N,T,1,28,28) stack of reconstructions nor any
element-wise temporary exists.  The kernel leaves one {count, mean, M2} triple per frame; they are combined here, on the host, in
double precision and in a fixed order (``merge_states``) after one copy of 3 F floats.

Held-out log-likelihood (``predict(..., loglik=True)``, ``compute_nll``): the model is trained on a Bernoulli likelihood
(vae.py:136-153, create_model.py:52-53), so the same kernel epilogue -- as ``gpode_dec10_predict_ll`` -- also leaves the
log-likelihood of every (draw, frame) image, computed from the logit as ``x a - softplus(a)`` (finite for every finite logit; the
reference's ``log(z) x + log(1 - z) (1 - x)`` on a float32 sigmoid is -inf / nan from a logit of about 17).  The L F floats come back
in one copy; the sums over time and the log-mean-exp over the draws are taken here in double precision (``loglik_stats``).

Marginal likelihood (``predict_marginal``, ``compute_iw_nll``, ``--eval_z0_draws True``): ``predict`` shares one sample of the initial
state among its L function draws.  ``predict_marginal`` draws L JOINT samples (z0_l ~ q(z0 | x), f_l ~ q(f)) -- one launch for the L
reparameterised initial states and their log-weights lw = log p(z0) - log q(z0 | x) (``gpode_reparam_draws_fwd``), one rollout launch
in which every draw starts from its own z0 (the ``_nz`` entry points) -- and reports the importance-weighted estimate
log p(x) ~ log (1/L) sum_l p(x | z0_l, f_l) p(z0_l) / q(z0_l | x) (``iw_stats``) with its effective sample size.

Command line (``python -m vae_gp_ode_amd.evaluate``, the flags of ``vae_gp_ode_amd.main`` so a training command line can be
reused): loads ``--model_path``, evaluates the test split with L = ``--eval_sample_size`` draws (squared error and the held-out
log-likelihood: ``mse``, ``std``, ``mse_t``, ``nll``, ``nlpd``, ``nll_t``), rolls ``--Troll`` * T frames out for
the first three test sequences, prints one JSON line and writes ``eval.json``, ``rollout_mean.npy``, ``rollout_var.npy`` under
``--save``.  The draws come from the host generators as in the reference (two of them unseeded there, SURVEY F6, so two runs differ
by Monte-Carlo noise); ``--device_noise True`` draws on the device, reproducibly from ``--seed``.  ``--ragged_frames KMIN``: every test
sequence keeps between KMIN and K (``--subsample_frames``, else T) of its frames and is padded to K; the error and the likelihood
take its observed frames only (``predict(..., n_obs=)``), ``mse_t`` / ``nll_t`` are means over the sequences that have the frame and
``count`` is L 784 times the number of observed frames.  ``--subsample_frames K``: every test
sequence keeps K of its frames (drawn per sequence, reproducibly from ``--seed``) and is evaluated on its own time grid
(``predict(..., ts=)``); the long roll-out stays on the uniform grid.  ``--eval_z0_draws True`` adds a second pass over the test split
with a z0 sample per draw and reports ``iw_nll``, ``nlpd_marginal``, ``ess_mean``, ``ess_min``; every other figure is unchanged.
``--eval_field True`` then evaluates the posterior of the vector field itself (``field_posterior``: mean and marginal variances of
q(f(z)), either kernel) at the encoder means of the initial states of the test split, writes ``field_z.npy``, ``field_mean.npy``,
``field_var.npy`` and adds ``field_points``, ``field_var_mean``, ``field_var_max``; without it nothing changes.
``--eval_flow True`` (fixed-grid solvers) then linearises the learnt flow about the same initial states (``flow_diagnostics``: the
state-transition matrices Phi_t = d z_t / d z0 in forward mode, their log-determinants, the finite-time Lyapunov exponent, the
divergence of the field along the trajectories), for ``--eval_sample_size`` function draws and for the posterior-mean field: writes
``flow_phi.npy``, ``flow_logdet.npy``, ``flow_div.npy`` and the same three with the suffix ``_mean``, and adds ``flow_logdet_mean``
(of log |det Phi| at the last time), ``flow_logdet_absmax`` (over all times), ``flow_ftle_mean``, ``flow_ftle_max``, ``flow_div_absmean``, ``flow_div_absmean_meanfield``; without it nothing
changes.  ``--eval_condition_frames K`` then forecasts every test sequence CONDITIONED on its first K frames
(``predict_conditional``: the joint draws of ``--eval_z0_draws`` weighted by how well each explains those frames, the weighted moments
folded inside the decoder's last kernel, ``gpode_dec10_predict_w``): adds ``cond_frames``, ``fc_mse``, ``fc_mse_uncond`` (the same draws
equally weighted), ``fc_nlpd``, ``fc_mse_t``, ``fc_nlpd_t``, ``cond_ess_mean``, ``cond_ess_min`` and writes ``forecast_mean.npy``,
``forecast_var.npy`` (the three rolled-out sequences, ``--Troll`` * T frames); 0, the default: nothing changes.
Single process: data-parallel evaluation is not built.  No plots.
"""
import argparse
import json
import math
import os
import sys
import time
import warnings
from collections import namedtuple

import numpy as np
import torch

Prediction = namedtuple('Prediction', 'mean var mse std count mse_t state passes ll nll nlpd nll_t', defaults=(None,) * 4)
Prediction.__doc__ = """mean, var (N,Th,1,28,28): predictive mean and unbiased variance of the decoded images over the L draws (None
without ``variance``; var is nan for L = 1, as torch.var);  mse, std: mean and unbiased standard deviation of the squared error over
all ``count`` = L N T_obs 784 elements;  mse_t (T_obs,): error per time step;  state: the (n, mean, M2) triple behind mse / std, for
merging over batches;  passes: draws per decoder pass.  With ``loglik`` (None otherwise):  ll (L,N) float64 on the CPU: log-likelihood of
every sequence under every draw;  nll: -mean of ll, the averaged negative log-likelihood (the likelihood term of the ELBO);  nlpd: the
negative log predictive density -mean_n log mean_l exp ll[l,n];  nll_t (T_obs,): -mean over draws and sequences per time step."""


MarginalPrediction = namedtuple('MarginalPrediction', 'll lw nll nlpd iw_ll iw_nll ess nll_t mse std state passes')
MarginalPrediction.__doc__ = """ll (L,N) float64 on the CPU: log p(x_n | z0_l, f_l) of every sequence under every JOINT draw of the initial state
and the function;  lw (L,N) float64: log p(z0_l) - log q(z0_l | x_n);  nll: -mean of ll;  nlpd: -mean_n log mean_l exp ll[l,n], the
predictive density with the initial state marginalised under q(z0 | x) (not under the prior);  iw_ll (N,), iw_nll: the
importance-weighted estimate of log p(x_n) and minus its mean over the sequences;  ess (N,): effective sample size of the L weights,
in [1, L];  nll_t (T,);  mse, std, state, passes: as in Prediction, over the same joint draws."""


def iw_stats(ll, lw):
    """(iw_ll, iw_nll, ess) of the importance-weighted marginal likelihood from ll, lw (L,N):
    iw_ll[n] = log mean_l exp(ll[l,n] + lw[l,n]);  iw_nll = -mean_n iw_ll;  ess[n] = (sum_l w)^2 / sum_l w^2 with
    w = exp(ll + lw - max_l(ll + lw)) -- the maximum cancels in the ratio.  Double precision on the CPU, the maximum subtracted as in
    log_mean_exp, a fixed order of operations: the same input gives the same bits."""
    a = torch.as_tensor(ll, dtype=torch.float64).cpu() + torch.as_tensor(lw, dtype=torch.float64).cpu()
    top = a.max(dim=0).values
    w = torch.exp(a - top)
    s1, s2 = w.sum(dim=0), (w * w).sum(dim=0)
    iw_ll = top + torch.log(s1) - math.log(a.shape[0])
    return iw_ll, -iw_ll.mean().item(), s1 * s1 / s2


CondStats = namedtuple('CondStats', 'logw wn ess evidence fc_ll fc_nlpd fc_nlpd_t prefix forecast')
CondStats.__doc__ = """cond_stats' result: logw (L,N), wn (L,N) the normalised weights, ess (N,), evidence (N,), fc_ll (N,), fc_nlpd,
fc_nlpd_t (T,), prefix (N,) the frames every sequence is conditioned on, forecast (N,T) bool: the observed frames behind the prefix."""


def _prefix(n_cond, N, T, n_obs=None):
    """frames t < min(n_cond[n], T, n_obs[n]) of sequence n are conditioned on: (N,) int64 on the CPU"""
    k = torch.as_tensor(n_cond).detach().cpu().to(torch.int64)
    k = k.expand(N) if k.dim() == 0 else k.reshape(N)
    k = k.clamp(min=0, max=T)
    if n_obs is not None:
        k = torch.minimum(k, torch.as_tensor(n_obs).detach().cpu().to(torch.int64).reshape(N).clamp(min=0))
    return k


def _split_frames(n_cond, N, T, n_obs=None):
    """(prefix (N,), conditioned-on frames (N,T) bool, forecast frames that have a target (N,T) bool), on the CPU"""
    k, o = _prefix(n_cond, N, T, n_obs), _prefix(T, N, T, n_obs)
    tt = torch.arange(T)[None, :]
    return k, tt < k[:, None], (tt >= k[:, None]) & (tt < o[:, None])


def cond_stats(ell, lw, n_cond, T, n_obs=None):
    """The weights of a forecast conditioned on an observed prefix, and what is read off them, from the frame log-likelihoods ell
    (L,N,Th) of L joint draws (z0_l ~ q(z0 | x), f_l ~ q(f)) and their log-weights lw (L,N) = log p(z0_l) - log q(z0_l | x_n).  With
    k[n] = min(n_cond[n], T, n_obs[n]) (``n_cond`` an int or (N,); T the observed length; ``n_obs`` (N,) the frame counts of ragged
    sequences or None) and o[n] = min(T, n_obs[n]):
      logw[l,n]    = lw[l,n] + sum_{t < k[n]} ell[l,n,t]
      wn[l,n]      = softmax_l logw[., n]                                (self-normalised weights)
      ess[n]       = (sum_l w)^2 / sum_l w^2                             (in [1, L])
      evidence[n]  = log (1/L) sum_l exp logw[l,n]                       (the estimate of log p(x_{<k}))
      fc_ll[n]     = log sum_l wn[l,n] exp sum_{k[n] <= t < o[n]} ell[l,n,t]   (= the estimate of log p(x) minus evidence)
      fc_nlpd      = -mean of fc_ll over the sequences that have a frame behind their prefix (nan when none has)
      fc_nlpd_t[t] = -mean_n log sum_l wn[l,n] exp ell[l,n,t] over the sequences with k[n] <= t < o[n]; nan where there is none.
    A column of logw that is -inf throughout (no draw has any weight) gives evidence = -inf and ess, wn, fc_ll = nan.  Double precision
    on the CPU, every maximum subtracted before its exp, a fixed order of operations: the same input gives the same bits.  -> CondStats."""
    ell = torch.as_tensor(ell, dtype=torch.float64).cpu()
    lw = torch.as_tensor(lw, dtype=torch.float64).cpu()
    L, N = lw.shape
    T = int(T)
    ell = ell[:, :, :T]
    k, pre, fut = _split_frames(n_cond, N, T, n_obs)
    zero = torch.zeros((), dtype=torch.float64)
    logw = lw + torch.where(pre[None], ell, zero).sum(dim=2)
    top = logw.max(dim=0).values
    top0 = torch.where(torch.isfinite(top), top, zero)
    w = torch.exp(logw - top0)
    s1, s2 = w.sum(dim=0), (w * w).sum(dim=0)
    evidence = top0 + torch.log(s1) - math.log(L)
    wn = w / s1
    a = logw + torch.where(fut[None], ell, zero).sum(dim=2)
    atop = a.max(dim=0).values
    atop0 = torch.where(torch.isfinite(atop), atop, zero)
    fc_ll = atop0 + torch.log(torch.exp(a - atop0).sum(dim=0)) - (top0 + torch.log(s1))
    has = fut.any(dim=1)
    fc_nlpd = -(torch.where(has, fc_ll, zero).sum() / has.sum().to(torch.float64)).item()
    b = logw[:, :, None] + ell                                                         # (L,N,T)
    btop = b.max(dim=0).values
    btop0 = torch.where(torch.isfinite(btop), btop, zero)
    lt = btop0 + torch.log(torch.exp(b - btop0).sum(dim=0)) - (top0 + torch.log(s1))[:, None]
    return CondStats(logw, wn, s1 * s1 / s2, evidence, fc_ll, fc_nlpd, -frame_means(lt, fut), k, fut)


def log_mean_exp(ll):
    """log(mean_l exp(ll[l, ...])) over the first axis, in double precision: the maximum over the draws is subtracted first (a plain
    exp underflows to 0 at ll of about -745, and a sequence's ll is in the thousands).  A fixed order of operations: the same input
    gives the same bits."""
    ll = torch.as_tensor(ll, dtype=torch.float64)
    top = ll.max(dim=0).values
    return top + torch.log(torch.exp(ll - top).sum(dim=0)) - math.log(ll.shape[0])


def _observed(n_obs, N, T):
    """(N,T) bool on the CPU: frame t of sequence n is observed iff t < n_obs[n] (counts <= 0: none, >= T: all)"""
    k = torch.as_tensor(n_obs).detach().cpu().to(torch.int64).reshape(N)
    return torch.arange(T)[None, :] < k[:, None]


def frame_means(v, obs):
    """Per-frame mean of v (N,T) float64 over the sequences that have the frame (obs (N,T) bool): (T,), nan where none has it.
    The entries of v behind a False are not read."""
    v = torch.where(obs, v, torch.zeros((), dtype=v.dtype))
    return v.sum(0) / obs.sum(0).to(v.dtype)           # 0 / 0 = nan: no sequence has the frame


def loglik_stats(ell, T_obs, n_obs=None):
    """(ll, nll, nlpd, nll_t) from the frame log-likelihoods ell (L,N,Th) (frames t >= T_obs hold 0 and are left out):
    ll[l,n] = sum_{t < T_obs} ell[l,n,t];  nll = -mean_{l,n} ll;  nlpd = -mean_n (logsumexp_l ll[l,n] - log L);
    nll_t[t] = -mean_{l,n} ell[l,n,t].  Double precision, a fixed order of operations.
    ``n_obs`` (N,): ragged sequences -- ll[l,n] sums the frames t < min(T_obs, n_obs[n]) (the others hold 0 and are left out by a
    select), nll and nlpd stay means over the sequences, and nll_t[t] is the mean over the draws and the sequences that HAVE frame t
    (nan where none has it).  None: the same bits as ever."""
    ell = torch.as_tensor(ell, dtype=torch.float64)[:, :, :T_obs]
    if n_obs is None:
        ll = ell.sum(dim=2)
        return ll, -ll.mean().item(), -log_mean_exp(ll).mean().item(), -ell.mean(dim=(0, 1))
    obs = _observed(n_obs, ell.shape[1], ell.shape[2])
    ell = torch.where(obs[None], ell, torch.zeros((), dtype=torch.float64))
    ll = ell.sum(dim=2)
    return ll, -ll.mean().item(), -log_mean_exp(ll).mean().item(), -frame_means(ell.mean(dim=0), obs)


def merge_states(states):
    """Combine (n, mean, M2) triples of disjoint samples into one (Chan, Golub & LeVeque), sequentially in the order given, in double
    precision.  Empty triples (n = 0) are skipped; no triple at all gives (0, 0, 0)."""
    n, mean, m2 = 0.0, 0.0, 0.0
    for nb, mb, qb in states:
        nb, mb, qb = float(nb), float(mb), float(qb)
        if nb == 0.0:
            continue
        if n == 0.0:
            n, mean, m2 = nb, mb, qb
            continue
        tot = n + nb
        delta = mb - mean
        mean = mean + delta * (nb / tot)
        m2 = m2 + qb + delta * delta * (n * nb / tot)
        n = tot
    return n, mean, m2


def mean_std(state):
    """(mean, sqrt(M2 / (n - 1))): torch.mean and torch.std (unbiased, its default) of the sample behind the triple; a single element
    has no standard deviation (nan, as torch gives)."""
    n, mean, m2 = state
    if n < 1:
        return float('nan'), float('nan')
    return mean, (math.sqrt(max(m2, 0.0) / (n - 1)) if n > 1 else float('nan'))


def plan_passes(L, images_per_draw, images_per_pass):
    """Split L draws of ``images_per_draw`` decoded images each into passes of whole draws of at most ``images_per_pass`` images:
    a list of (first draw, end draw).  A budget smaller than one draw cannot be met -- a draw is the unit the kernel folds -- so it
    falls back to one draw per pass and warns."""
    if L < 1 or images_per_draw < 1 or images_per_pass < 1:
        raise ValueError('plan_passes: L, images_per_draw and images_per_pass must be positive')
    per = images_per_pass // images_per_draw
    if per < 1:
        warnings.warn('images_per_pass=%d is smaller than one draw (%d images): decoding one draw per pass' % (images_per_pass, images_per_draw))
        per = 1
    return [(l0, min(L, l0 + per)) for l0 in range(0, L, per)]


class _EvalMode:
    """model.eval() for the duration of a call; every submodule's own ``training`` flag is put back afterwards."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.flags = [(m, m.training) for m in self.model.modules()]
        self.model.eval()

    def __exit__(self, *exc):
        for m, flag in self.flags:
            m.training = flag
        return False


def _grid(ts, N, Th, T, who):
    """``ts`` of predict / predict_marginal: None, or (N,Th) observation times per sequence (a grid over the T observed frames alone is
    enough when the roll-out stops there)"""
    if ts is None:
        return None
    if ts.dim() != 2 or ts.shape[0] != N or ts.shape[1] not in (Th, T):
        raise ValueError('%s: ts must be (N,T\') = (%d,%d), one row of observation times per sequence; got %s' % (who, N, Th, tuple(ts.shape)))
    if ts.shape[1] != Th:
        raise ValueError('%s: ts covers %d frames, the roll-out %d: give the times of the forecast frames as well' % (who, ts.shape[1], Th))
    return ts


def _grid_kw(ts, n_obs=None):
    """ts= / n_obs= for predict / predict_marginal when the loader item carries them; nothing otherwise -- the call as it always was"""
    kw = {} if ts is None else {'ts': ts}
    if n_obs is not None:
        kw['n_obs'] = n_obs
    return kw


def _frames_ts(batch):
    """(X, ts, n_obs) of a loader item: a loader that yields (X, ts (N,T)) pairs carries the observation times of its sequences, one
    that yields (X, ts, n_obs (N,)) triples their frame counts as well (ragged sequences, padded to T); every other item (the tensor
    itself, a TensorDataset 1-tuple) has neither"""
    if isinstance(batch, (list, tuple)):
        return batch[0], (batch[1] if len(batch) > 1 else None), (batch[2] if len(batch) > 2 else None)
    return batch, None, None


def _counts(n_obs, X, who):
    """``n_obs`` of predict / predict_marginal on X's device: None, or (N,) int32 (shape and dtype are checked by vae_ops)"""
    if n_obs is None:
        return None
    if not torch.is_tensor(n_obs):
        raise ValueError('%s: n_obs must be an int32 tensor (N,), one frame count per sequence' % who)
    return n_obs.to(X.device)


def predict(model, X, L=1, T_custom=None, images_per_pass=8192, variance=True, loglik=False, ts=None, n_obs=None):
    """Posterior-predictive statistics of ``model`` (ODEGPVAE) for the sequences X (N,T,1,28,28): encode once, one z0 sample per
    sequence, L function draws shared by the batch, integrate ``T_custom or T`` steps, decode (positions only for order 2) --
    the order of operations of the notebook routine -- and reduce inside the decoder's last kernel.  Frames beyond T have no
    target: they enter the predictive mean / variance and not the error.  The draws go through the decoder in passes of at most
    ``images_per_pass`` images (8192: the largest image count the decoder's parity tests cover, not a tuned value).
    ``variance=False``: the error statistics only; the roll-out then stops at T, since the first T frames of a longer one are
    the same trajectory.  ``loglik=True`` also fills ``ll``, ``nll``, ``nlpd`` and ``nll_t`` of the result (Bernoulli log-likelihood of
    the observed frames, from the logits); every other field is the same bits as without it.  One z0 sample per sequence is shared by
    the L draws, so ``nlpd`` is the predictive density under the GP function draws GIVEN that sample of the initial state, not the
    marginal over the encoder's distribution.  ``ts`` (N,T'), T' = ``T_custom or T``: the observation (and forecast) times of every
    sequence instead of the uniform grid dt * arange(T'); with ``variance=False`` the first T columns are read.  ``mse_t`` and ``nll_t``
    stay indexed by FRAME: entry t averages frame t of every sequence, whatever time each of them was observed at.
    ``n_obs`` (N,) int32: ragged sequences, X padded to T frames -- frame t of sequence n has a target iff t < n_obs[n]; the padded
    frames are integrated and decoded like forecast frames (they enter mean / var) and add nothing to the error or the likelihood,
    whatever the padded targets hold.  ``count`` is then L 784 sum_n min(n_obs[n], T), and ``mse_t`` / ``nll_t`` average over the
    sequences that have the frame (nan where none has it).  None: every field the same bits as ever.  Runs without
    autograd and in eval mode; leaves every module buffer and ``training`` flag as it found them."""
    from . import vae_ops as V
    if X.dim() != 5 or tuple(X.shape[2:]) != (1, 28, 28):
        raise ValueError('predict: X must be (N,T,1,28,28)')
    n_obs = _counts(n_obs, X, 'predict')
    N, T = X.shape[0], X.shape[1]
    Th = int(T_custom) if T_custom else T
    if Th < T:
        raise ValueError('predict: T_custom (%d) must be at least the observed length (%d)' % (Th, T))
    if ts is not None and not variance and ts.dim() == 2 and ts.shape[1] == Th:
        ts = ts[:, :T]
    if not variance:
        Th = T              # forecast frames have no target: without the moments over the draws nothing would come of them
    ts = _grid(ts, N, Th, T, 'predict')
    L = int(L)
    F = N * Th
    passes = plan_passes(L, F, int(images_per_pass))
    dec = model.vae.decoder
    with torch.no_grad(), _EvalMode(model):
        X = X.contiguous().float()
        z0, _, _ = model.encode_initial_state(X)
        ztL = model.sample_trajectories(z0, Th, L) if ts is None else model.sample_trajectories(z0, Th, L, ts=ts.to(X.device))
        lat = ztL if model.order == 1 else ztL[..., :ztL.shape[-1] // 2]
        tables = dec._frozen_tables()
        state = V.PredictState(F, X.device, variance, loglik=L if loglik else 0)
        for l0, l1 in passes:
            c, t8 = dec.decode_frozen_raw(lat[l0:l1], tables)
            if n_obs is None:
                V.dec10_predict(c, t8, dec.decnn[10].weight, dec.decnn[10].bias, X, Th, state)
            else:
                V.dec10_predict(c, t8, dec.decnn[10].weight, dec.decnn[10].bias, X, Th, state, n_obs=n_obs)
            del c
        se = state.se.double().cpu().view(N, Th, 3)[:, :T]            # one copy of 3 F floats; frames t >= T hold zeros
        mean = var = None
        if variance:
            mean = state.mean.view(N, Th, 1, 28, 28)
            var = (state.m2 / (L - 1) if L > 1 else torch.full_like(state.m2, float('nan'))).view(N, Th, 1, 28, 28)
    total = merge_states(se.reshape(-1, 3).tolist())
    mse, std = mean_std(total)
    if n_obs is None:
        mse_t = se[:, :, 1].mean(0)                                    # every frame holds the same count L * 784
    else:
        mse_t = frame_means(se[:, :, 1], _observed(n_obs, N, T))       # a frame with a target holds L * 784 errors, one without none
    extra = ()
    if loglik:
        extra = loglik_stats(state.ell.cpu().double().view(L, N, Th), T, *(() if n_obs is None else (n_obs,)))   # one copy of L F floats
    return Prediction(mean, var, mse, std, int(total[0]), mse_t, total, [b - a for a, b in passes], *extra)


def predict_marginal(model, X, L, images_per_pass=8192, ts=None, n_obs=None):
    """``predict(variance=False, loglik=True)`` with the initial state sampled PER DRAW: ``encode_initial_state(X, draws=L)`` gives
    z0 (L,N,order*q) and the log-weights lw (L,N), draw l integrates from z0[l] under function draw l (one rollout launch over L N
    trajectories), and the decoder passes and the fused last kernel are predict's.  -> MarginalPrediction.  ``ts`` (N,T): the
    observation times of every sequence, shared by its L draws; ``nll_t`` stays indexed by frame, as in predict.  ``n_obs`` (N,) int32:
    the frame counts of ragged sequences, as in predict.  Runs without autograd
    and in eval mode; leaves every module buffer and ``training`` flag as it found them."""
    from . import vae_ops as V
    if X.dim() != 5 or tuple(X.shape[2:]) != (1, 28, 28):
        raise ValueError('predict_marginal: X must be (N,T,1,28,28)')
    n_obs = _counts(n_obs, X, 'predict_marginal')
    N, T = X.shape[0], X.shape[1]
    L = int(L)
    F = N * T
    ts = _grid(ts, N, T, T, 'predict_marginal')
    passes = plan_passes(L, F, int(images_per_pass))
    dec = model.vae.decoder
    with torch.no_grad(), _EvalMode(model):
        X = X.contiguous().float()
        z0, lw, _, _ = model.encode_initial_state(X, draws=L)          # (L,N,order*q), (L,N)
        ztL = model.sample_trajectories(z0, T, L) if ts is None else model.sample_trajectories(z0, T, L, ts=ts.to(X.device))
        lat = ztL if model.order == 1 else ztL[..., :ztL.shape[-1] // 2]
        tables = dec._frozen_tables()
        state = V.PredictState(F, X.device, False, loglik=L)
        for l0, l1 in passes:
            c, t8 = dec.decode_frozen_raw(lat[l0:l1], tables)
            if n_obs is None:
                V.dec10_predict(c, t8, dec.decnn[10].weight, dec.decnn[10].bias, X, T, state)
            else:
                V.dec10_predict(c, t8, dec.decnn[10].weight, dec.decnn[10].bias, X, T, state, n_obs=n_obs)
            del c
        se = state.se.double().cpu().view(N, T, 3)
        ell = state.ell.cpu().double().view(L, N, T)
        lw = lw.cpu().double()
    total = merge_states(se.reshape(-1, 3).tolist())
    mse, std = mean_std(total)
    ll, nll, nlpd, nll_t = loglik_stats(ell, T, *(() if n_obs is None else (n_obs,)))
    iw_ll, iw_nll, ess = iw_stats(ll, lw)
    return MarginalPrediction(ll, lw, nll, nlpd, iw_ll, iw_nll, ess, nll_t, mse, std, total, [b - a for a, b in passes])


def compute_iw_nll(model, loader, L, images_per_pass=8192):
    """(iw_nll, nlpd, mean ess) over a whole loader with L joint draws per batch (predict_marginal): means over all sequences, the
    batches weighted by their sequence counts.  A loader that yields (X, ts) pairs is evaluated on its time grids, one that yields
    (X, ts, n_obs) triples on its ragged sequences."""
    dev = next(model.parameters()).device
    nseq, iw, nlpd, ess = 0, 0.0, 0.0, 0.0
    for batch in loader:
        X, ts, n_obs = _frames_ts(batch)
        X = X.to(dev)
        p = predict_marginal(model, X, L, images_per_pass=images_per_pass, **_grid_kw(ts, n_obs))
        nseq += X.shape[0]
        iw += p.iw_nll * X.shape[0]
        nlpd += p.nlpd * X.shape[0]
        ess += p.ess.sum().item()
    if nseq == 0:
        return float('nan'), float('nan'), float('nan')
    return iw / nseq, nlpd / nseq, ess / nseq


ConditionalPrediction = namedtuple('ConditionalPrediction',
                                   'mean var logw ess evidence fc_ll fc_nlpd fc_nlpd_t fc_mse fc_mse_t fc_mse_uncond_t passes')
ConditionalPrediction.__doc__ = """mean, var (N,Th,1,28,28): the self-normalised importance-weighted predictive mean and variance of the
decoded images given the observed prefix; var = M2 / W is the variance of the weighted mixture of the draws -- NO Bessel correction (a
weighted sample has no agreed one, and with the weight on one draw it is 0, not nan);  logw (L,N) float64 on the CPU: the log-weights
lw + sum_{t < prefix} ell;  ess (N,): their effective sample size, in [1, L] -- read it first: at ess ~ 1 every other field rests on one
draw;  evidence (N,): log (1/L) sum_l exp logw, the estimate of log p(x_{<prefix});  fc_ll (N,): log sum_l wn_l exp(sum of ell over the
observed frames behind the prefix), the predictive log-density of those frames given the prefix;  fc_nlpd: -mean_n fc_ll;  fc_nlpd_t
(T,): the same per frame, nan where no sequence has frame t behind its prefix;  fc_mse: the weighted mean squared error over the
forecast frames that have a target;  fc_mse_t (T,): per frame;  fc_mse_uncond_t (T,): the same frames with the draws equally weighted
-- the baseline the weighting is meant to beat;  passes: draws per decoder pass."""


def _cond_frames(model, n_cond, T, who):
    """``n_cond`` of predict_conditional against what the encoder reads and the observed length; before any device work"""
    need = 1 if model.order == 1 else int(model.v_steps)
    k = torch.as_tensor(n_cond).detach().cpu()
    if k.is_floating_point() or k.dtype == torch.bool or k.dim() > 1:
        raise ValueError('%s: n_cond must be an int or an (N,) integer tensor' % who)
    lo, hi = int(k.min()), int(k.max())
    if lo < need:
        raise ValueError('%s: n_cond = %d, but the encoder reads the first %d frame(s) (order %d): the proposal q(z0 | x) would have '
                         'seen frames the target has not' % (who, lo, need, model.order))
    if hi > T:
        raise ValueError('%s: n_cond = %d exceeds the observed length T = %d' % (who, hi, T))
    return k.to(torch.int64)


def predict_conditional(model, X, L, n_cond, T_custom=None, images_per_pass=8192, ts=None, n_obs=None):
    """The forecast of the sequences X (N,T,1,28,28) CONDITIONED on their first frames: sequence n on the frames
    t < min(n_cond[n], T, n_obs[n]) (``n_cond`` an int or an (N,) integer tensor).  L joint draws (z0_l ~ q(z0 | x), f_l ~ q(f)) are
    rolled out over ``T_custom or T`` frames exactly as predict_marginal draws them, and draw l gets the self-normalised weight
    wn[l,n] = softmax_l (lw[l,n] + sum_{t < prefix} ell[l,n,t]) -- how well it explains what was in fact observed.  Per decoder pass, on
    the same raw decoder output: dec10_predict leaves ell and the unweighted error, the log-weights of the pass are formed on the device
    (float64, no host sync) and handed over relative to the log-weight of draw 0 of each sequence (so that float32 resolves them, and so
    that the split into passes does not enter), and dec10_predict_w folds the weighted moments.  -> ConditionalPrediction.
    ValueError: n_cond below what the encoder reads (1 frame; ``model.v_steps`` for order 2) or above T.  ``ts`` (N,Th), ``n_obs`` (N,)
    int32 as in predict.  Runs without autograd and in eval mode; leaves every module buffer and ``training`` flag as it found them."""
    from . import vae_ops as V
    if X.dim() != 5 or tuple(X.shape[2:]) != (1, 28, 28):
        raise ValueError('predict_conditional: X must be (N,T,1,28,28)')
    N, T = X.shape[0], X.shape[1]
    kc = _cond_frames(model, n_cond, T, 'predict_conditional')
    if kc.dim() == 1 and kc.shape[0] != N:
        raise ValueError('predict_conditional: n_cond must be an int or (N,) = (%d,); got %s' % (N, tuple(kc.shape)))
    Th = int(T_custom) if T_custom else T
    if Th < T:
        raise ValueError('predict_conditional: T_custom (%d) must be at least the observed length (%d)' % (Th, T))
    n_obs = _counts(n_obs, X, 'predict_conditional')
    ts = _grid(ts, N, Th, T, 'predict_conditional')
    L = int(L)
    F = N * Th
    passes = plan_passes(L, F, int(images_per_pass))
    dec = model.vae.decoder
    k_host = _prefix(kc, N, T, n_obs)
    with torch.no_grad(), _EvalMode(model):
        X = X.contiguous().float()
        z0, lw, _, _ = model.encode_initial_state(X, draws=L)          # (L,N,order*q), (L,N)
        ztL = model.sample_trajectories(z0, Th, L) if ts is None else model.sample_trajectories(z0, Th, L, ts=ts.to(X.device))
        lat = ztL if model.order == 1 else ztL[..., :ztL.shape[-1] // 2]
        tables = dec._frozen_tables()
        state = V.PredictState(F, X.device, False, loglik=L)
        cond = V.CondState(F, N, X.device)
        kmax = int(k_host.max())
        pre = torch.arange(kmax)[None, :] < k_host[:, None]            # (N,kmax): frame t of sequence n is conditioned on
        pre = pre.to(X.device)
        zero = torch.zeros((), dtype=torch.float64, device=X.device)
        lw64 = lw.double()
        rel = torch.empty(L, N, dtype=torch.float32, device=X.device)
        ref = None
        for l0, l1 in passes:
            c, t8 = dec.decode_frozen_raw(lat[l0:l1], tables)
            if n_obs is None:
                V.dec10_predict(c, t8, dec.decnn[10].weight, dec.decnn[10].bias, X, Th, state)
            else:
                V.dec10_predict(c, t8, dec.decnn[10].weight, dec.decnn[10].bias, X, Th, state, n_obs=n_obs)
            e = state.ell[l0:l1].view(l1 - l0, N, Th).double()
            lg = lw64[l0:l1]
            for t in range(kmax):                                      # element-wise, frame by frame: the same bits for any pass size
                lg = lg + torch.where(pre[:, t], e[:, :, t], zero)
            if ref is None:                                            # draw 0 of every sequence: the same whatever the passes are
                ref = torch.where(torch.isfinite(lg[0]), lg[0], torch.zeros_like(lg[0]))
            rel[l0:l1] = (lg - ref).float()
            V.dec10_predict_w(c, t8, dec.decnn[10].weight, dec.decnn[10].bias, X, Th, cond, rel, n_obs=n_obs)
            del c
        cond.check()
        se = state.se.double().cpu().view(N, Th, 3)[:, :T]
        ell = state.ell.cpu().double().view(L, N, Th)
        W = cond.wstate[:, 1]
        mean = cond.mean.view(N, Th, 1, 28, 28)
        var = (cond.m2 / W[:, None]).view(N, Th, 1, 28, 28)
        wmse = (cond.wse.double() / W.double()).cpu().view(N, Th)[:, :T]
        lw = lw.cpu().double()
    st = cond_stats(ell, lw, kc, T, n_obs)
    nf = st.forecast.sum().to(torch.float64)
    fc_mse = (torch.where(st.forecast, wmse, torch.zeros((), dtype=torch.float64)).sum() / nf).item()
    return ConditionalPrediction(mean, var, st.logw, st.ess, st.evidence, st.fc_ll, st.fc_nlpd, st.fc_nlpd_t, fc_mse,
                                 frame_means(wmse, st.forecast), frame_means(se[:, :, 1], st.forecast), [b - a for a, b in passes])


def compute_forecast(model, loader, L, n_cond, images_per_pass=8192):
    """(fc_mse, fc_nlpd, mean ess) of the forecast conditioned on the first ``n_cond`` frames over a whole loader with L joint draws per
    batch (predict_conditional): fc_mse is the mean over all forecast frames that have a target, fc_nlpd the mean over the sequences
    that have such a frame, ess the mean over all sequences.  A loader that yields (X, ts) pairs is evaluated on its time grids, one
    that yields (X, ts, n_obs) triples on its ragged sequences."""
    dev = next(model.parameters()).device
    nseq = nfc = nfr = 0
    mse = nlpd = ess = 0.0
    for batch in loader:
        X, ts, n_obs = _frames_ts(batch)
        X = X.to(dev)
        p = predict_conditional(model, X, L, n_cond, images_per_pass=images_per_pass, **_grid_kw(ts, n_obs))
        fut = _split_frames(n_cond, X.shape[0], X.shape[1], n_obs)[2]
        frames, seqs = int(fut.sum()), int(fut.any(dim=1).sum())
        nseq += X.shape[0]
        ess += p.ess.sum().item()
        if frames:
            mse += p.fc_mse * frames
            nlpd += p.fc_nlpd * seqs
            nfr += frames
            nfc += seqs
    if nseq == 0:
        return float('nan'), float('nan'), float('nan')
    return (mse / nfr if nfr else float('nan')), (nlpd / nfc if nfc else float('nan')), ess / nseq


def compute_mse_std(model, loader, L=1, images_per_pass=8192):
    """(mse, std) of the squared reconstruction error over a whole loader with L draws per batch -- ``compute_mse_std`` of the
    evaluation notebook: the batches' (n, mean, M2) triples are merged, so the result is the mean / std over all elements.
    A loader that yields (X, ts) pairs is evaluated on its time grids, one that yields (X, ts, n_obs) triples on its ragged sequences."""
    dev = next(model.parameters()).device
    states = []
    for batch in loader:
        X, ts, n_obs = _frames_ts(batch)
        states.append(predict(model, X.to(dev), L, images_per_pass=images_per_pass, variance=False, **_grid_kw(ts, n_obs)).state)
    return mean_std(merge_states(states))


def compute_nll(model, loader, L=1, images_per_pass=8192):
    """(nll, nlpd) of the held-out log-likelihood over a whole loader with L draws per batch: the batches' figures are means over
    their sequences, so they are weighted by the sequence counts -- the mean over all sequences, not over batches.
    A loader that yields (X, ts) pairs is evaluated on its time grids, one that yields (X, ts, n_obs) triples on its ragged sequences."""
    dev = next(model.parameters()).device
    nseq, nll, nlpd = 0, 0.0, 0.0
    for batch in loader:
        X, ts, n_obs = _frames_ts(batch)
        X = X.to(dev)
        p = predict(model, X, L, images_per_pass=images_per_pass, variance=False, loglik=True, **_grid_kw(ts, n_obs))
        nseq += X.shape[0]
        nll += p.nll * X.shape[0]
        nlpd += p.nlpd * X.shape[0]
    if nseq == 0:
        return float('nan'), float('nan')
    return nll / nseq, nlpd / nseq


def initial_state_means(model, X):
    """The encoder means of the initial states of the sequences X (N,T,1,28,28), (N, order*q): for order 2 the position and the
    velocity means concatenated, the layout of the state the flow integrates.  No sample is drawn.  Eval mode, no autograd."""
    with torch.no_grad(), _EvalMode(model):
        X = X.contiguous().float()
        mu_s, _ = model.vae.encoder(X[:, 0])
        if model.order == 1:
            return mu_s
        mu_v, _ = model.vae.encoder_v(X[:, 0:model.v_steps].squeeze(2))
        return torch.cat([mu_s, mu_v], dim=1)


def field_posterior(model, z, cov='diag'):
    """(mean, var) of the learnt vector field q(f(z)) at the latent states z (N, order*q): ``SVGP_Layer.posterior`` of the model's
    GP layer, for either kernel -- where the field is confident and what its mean is, away from the decoded frames.  ``cov`` as
    there ('diag': marginal variances (N,D_out))."""
    return model.flow.odefunc.diffeq.posterior(z, cov=cov)


def initial_state_moments(model, X):
    """(mean, variance) of the encoder's q(z0 | X) for the sequences X (N,T,1,28,28), each (N, order*q) in the layout of the state the
    flow integrates.  No sample is drawn.  Eval mode, no autograd."""
    with torch.no_grad(), _EvalMode(model):
        X = X.contiguous().float()
        mu_s, lv_s = model.vae.encoder(X[:, 0])
        if model.order == 1:
            return mu_s, lv_s.exp()
        mu_v, lv_v = model.vae.encoder_v(X[:, 0:model.v_steps].squeeze(2))
        return torch.cat([mu_s, mu_v], dim=1), torch.cat([lv_s, lv_v], dim=1).exp()


def flow_logdet(Phi):
    """log |det Phi_t| of state-transition matrices Phi (..., T, D, D): (..., T) float64 on the CPU.  The volume change of the flow
    about the trajectory; 0 for a volume-preserving one."""
    return torch.linalg.slogdet(Phi.detach().double().cpu())[1]


def flow_ftle(Phi, ts):
    """The finite-time Lyapunov exponent log sigma_max(Phi_{T-1}) / (t_{T-1} - t_0) of Phi (..., N, T, D, D) over the grid ts (T,) or
    (N,T): (..., N) float64 on the CPU."""
    ts = ts.detach().double().cpu()
    smax = torch.linalg.matrix_norm(Phi[..., -1, :, :].detach().double().cpu(), ord=2)
    return smax.log() / (ts[..., -1] - ts[..., 0])


def flow_var_lin(Phi, var0):
    """diag(Phi_t diag(var0) Phi_t^T): the first-order propagation of a diagonal initial covariance var0 (N,D) along Phi
    (..., N, T, D, D) -> (..., N, T, D) float64 on the CPU."""
    P = Phi.detach().double().cpu()
    return (P * P * var0.detach().double().cpu()[:, None, None, :]).sum(-1)


def flow_diagnostics(model, X, L=1, ts=None, mean_field=False):
    """The learnt flow linearised about the trajectories that start at the encoder means of the initial states of X (N,T,1,28,28), as
    ``field_posterior`` starts there: L function draws from the model's noise stream, or -- ``mean_field`` -- the single draw
    ``mean_noise()`` under which the field is its posterior mean (the leading axis is then 1).  ``ts``: (T,) or (N,T) output times,
    None = the uniform grid dt * arange(T).  Fixed-grid solvers only (``Flow.sensitivity``).  Returns a dict of
      zt (L,N,T,D), Phi (L,N,T,D,D)       the trajectories and d z_t / d z0 (float32, on the device)
      logdet (L,N,T)                      flow_logdet(Phi)
      ftle (L,N)                          flow_ftle(Phi, ts)
      div (L,N,T)                         the divergence of the field at zt (the phase-space divergence for order 2)
      z_var_lin (L,N,T,D)                 flow_var_lin(Phi, the encoder's variance)
    the reductions in float64 on the host."""
    flow = model.flow
    gp = flow.odefunc.diffeq
    z0, var0 = initial_state_moments(model, X)
    if ts is None:
        ts = model.dt * torch.arange(X.shape[1], dtype=torch.float32, device=z0.device)
    ts = ts.to(device=z0.device, dtype=torch.float32).contiguous()
    N, D = z0.shape

    def one(cache):
        zt, Phi = flow.sensitivity(z0, ts, cache=cache)
        x = zt.reshape((cache.nd, -1, D) if cache.stacked else (-1, D)).contiguous()
        div = gp.divergence(x).reshape(zt.shape[:-1])
        return (zt, Phi, div) if cache.stacked else (zt.unsqueeze(0), Phi.unsqueeze(0), div.unsqueeze(0))
    with torch.no_grad(), _EvalMode(model):
        if mean_field:
            parts = [one(gp.build_cache(noise=gp.mean_noise()))]
        elif int(L) > 1 and gp.batched_draws_supported():
            parts = [one(gp.build_cache(draws=int(L)))]
        else:
            parts = [one(gp.build_cache()) for _ in range(int(L))]
    zt, Phi, div = (torch.cat([p[i] for p in parts]) for i in range(3))
    return dict(zt=zt, Phi=Phi, logdet=flow_logdet(Phi), ftle=flow_ftle(Phi, ts), div=div.double().cpu(), z_var_lin=flow_var_lin(Phi, var0))


def build_from_checkpoint(args):
    """(model, test loader, checkpoint file) for a parsed command line, the way ``vae_gp_ode_amd.main`` sets a run up: seed, data,
    model, kernel initialisation, then the checkpoint ``--model_path`` (the .pth file, or the results directory that holds
    odegpvae_mnist.pth).  As in ``main``, ``--device`` is a place holder: ``args.device`` becomes the current HIP device."""
    from .main import load_data
    from .model.core.initialization import initialize_and_fix_kernel_parameters
    from .model.create_model import build_model
    from .model.misc.torch_utils import seed_everything
    seed_everything(args.seed)
    args.device = torch.device('cuda')
    fname = args.model_path
    if os.path.isdir(fname) or not fname.endswith('.pth'):
        fname = os.path.join(fname, 'odegpvae_mnist.pth')
    if not os.path.exists(fname):
        raise SystemExit('--model_path: no checkpoint at %s' % fname)
    _, testset = load_data(args)
    model = build_model(args).to(args.device)
    model = initialize_and_fix_kernel_parameters(model, lengthscale_value=args.lengthscale, variance_value=args.variance, fix=False)
    model.load_state_dict(torch.load(fname, map_location=args.device))
    if args.device_noise or args.hip_graph:          # as main.py: draws from the device generator, reproducible from --seed
        from .model.core.noise import install_device_noise
        install_device_noise(model, args.seed + 1)
    return model, testset, fname


def make_parser():
    """The training command line (``vae_gp_ode_amd.main.make_parser``, whose flag list is the reference's) plus what only the
    evaluation reads."""
    from .main import make_parser as train_parser
    p = train_parser()
    p.add_argument('--eval_z0_draws', type=eval, default=False,
                   help='also report the importance-weighted marginal likelihood: a second pass over the test split in which every one of '
                        'the --eval_sample_size draws samples its own initial state (iw_nll, nlpd_marginal, ess_mean, ess_min)')
    # absent from the namespace unless given (read with eval_field(args)): a command line without it parses to what it always did
    p.add_argument('--eval_field', type=eval, default=argparse.SUPPRESS,
                   help='also evaluate the posterior of the vector field at the encoder means of the initial states of the test split: '
                        'field_z.npy, field_mean.npy, field_var.npy (marginal variances) and field_points, field_var_mean, field_var_max '
                        '(default: False)')
    p.add_argument('--eval_flow', type=eval, default=argparse.SUPPRESS,
                   help='also linearise the learnt flow about the encoder means of the initial states of the test split (euler, midpoint, '
                        'rk4): flow_phi.npy, flow_logdet.npy, flow_div.npy for the sampled draws and for the posterior-mean field (_mean), and '
                        'flow_logdet_mean, flow_logdet_absmax, flow_ftle_mean, flow_ftle_max, flow_div_absmean, flow_div_absmean_meanfield '
                        '(default: False)')
    return p


def eval_flow(args):
    """--eval_flow of a parsed command line; False when the switch was not given"""
    return bool(getattr(args, 'eval_flow', False))


def eval_field(args):
    """--eval_field of a parsed command line; False when the switch was not given"""
    return bool(getattr(args, 'eval_field', False))


def _nullable(v):
    """a (T,) tensor as a list for eval.json, None (null) where it is nan: a frame that no sequence forecasts"""
    return [None if math.isnan(x) else x for x in v.tolist()]


def check_condition_frames(args):
    """--eval_condition_frames K: 0 (off), or at least what the encoder reads (1 frame; --frames for --ode 2) and at most the frames a
    test sequence has (--subsample_frames if set, else --T); refused with a message otherwise, ahead of any device work"""
    K = args.eval_condition_frames
    if not K:
        return
    need, T = (1 if args.ode == 1 else args.frames), (args.subsample_frames or args.T)
    if K < need:
        raise SystemExit('--eval_condition_frames %d: the encoder reads the first %d frame(s) (--ode %d), so the forecast must be '
                         'conditioned on at least as many' % (K, need, args.ode))
    if K > T:
        raise SystemExit('--eval_condition_frames %d: a test sequence has %d frames' % (K, T))


def _subsampled(args, loader):
    """The loader's items as (all frames, X, ts, n_obs): with --subsample_frames K every sequence keeps K frames, drawn per batch from
    a generator of its own seeded from --seed (so a second pass sees the same subsets), ts = dt * (kept indices); with
    --ragged_frames KMIN every sequence keeps between KMIN and K (or T) frames and is padded (data.utils.ragged_frames), n_obs its
    count; without either X is all frames and ts, n_obs are None."""
    from .main import _frames, subsample_generator, subsample_lead
    if not args.subsample_frames and not args.ragged_frames:
        for batch in loader:
            X = _frames(batch).to(args.device)
            yield X, X, None, None
        return
    from .data.utils import ragged_frames, subsample_frames
    gen = subsample_generator(args)
    for batch in loader:
        full = _frames(batch).to(args.device)
        if args.ragged_frames:
            X, kept, n_obs = ragged_frames(full, args.ragged_frames, args.subsample_frames or full.shape[1], subsample_lead(args), gen)
            yield full, X, args.dt * kept.to(torch.float32), n_obs
            continue
        X, kept = subsample_frames(full, args.subsample_frames, subsample_lead(args), gen)
        yield full, X, args.dt * kept.to(torch.float32), None


def main(argv=None):
    from .main import check_dense_scale, check_ragged, check_subsample
    args = make_parser().parse_args(argv)
    if eval_flow(args) and args.solver == 'dopri5':  # before any device work: the tangent-linear rollout has fixed grids only
        from .ops import DOPRI5_TANGENT
        raise SystemExit('--eval_flow True with --solver dopri5: ' + DOPRI5_TANGENT)
    check_subsample(args)
    check_ragged(args)
    check_dense_scale(args)
    check_condition_frames(args)
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise SystemExit('vae_gp_ode_amd.evaluate is a single-process tool: data-parallel evaluation is not built '
                         '(start it without torchrun, or with one rank)')
    if not torch.cuda.is_available():
        raise SystemExit('this build runs on an MI355X (no CPU fallback)')
    model, testset, fname = build_from_checkpoint(args)
    L = args.eval_sample_size

    torch.cuda.synchronize()
    t0 = time.time()
    states, per_step, nseq, first = [], None, 0, None
    nll = nlpd = 0.0
    nll_step = None
    have = None                                      # --ragged_frames: sequences that have frame t, the weights of the per-frame means
    for full, Xb, tsb, nb in _subsampled(args, testset):
        first = full if first is None else first     # the roll-out below: all frames, the uniform grid
        p = predict(model, Xb, L, variance=False, loglik=True, **_grid_kw(tsb, nb))
        states.append(p.state)
        nll += p.nll * Xb.shape[0]
        nlpd += p.nlpd * Xb.shape[0]
        wt = Xb.shape[0]
        if nb is not None:                           # a frame no sequence of the batch has is nan with weight 0: it adds nothing
            wt = _observed(nb, Xb.shape[0], Xb.shape[1]).sum(0).to(torch.float64)
            have = wt if have is None else have + wt
            p = p._replace(nll_t=torch.nan_to_num(p.nll_t), mse_t=torch.nan_to_num(p.mse_t))
        nll_step = p.nll_t * wt if nll_step is None else nll_step + p.nll_t * wt
        per_step = p.mse_t * wt if per_step is None else per_step + p.mse_t * wt
        nseq += Xb.shape[0]
    total = merge_states(states)
    mse, std = mean_std(total)
    T = first.shape[1]
    roll = predict(model, first[:3].contiguous(), L, T_custom=args.Troll * T)
    if args.subsample_frames:
        T = args.subsample_frames                    # the frames per sequence behind every figure but the roll-out's
    per_frame = nseq if have is None else have       # means over the sequences that have the frame (nan where none has it)
    marginal = None
    if args.eval_z0_draws:                           # behind everything else: the figures above see the draws they see without it
        iw = nlpd_m = ess_sum = 0.0
        ess_min = float('inf')
        for _, Xb, tsb, nb in _subsampled(args, testset):
            pm = predict_marginal(model, Xb, L, **_grid_kw(tsb, nb))
            iw += pm.iw_nll * pm.ll.shape[1]
            nlpd_m += pm.nlpd * pm.ll.shape[1]
            ess_sum += pm.ess.sum().item()
            ess_min = min(ess_min, pm.ess.min().item())
        marginal = dict(iw_nll=iw / nseq, nlpd_marginal=nlpd_m / nseq, ess_mean=ess_sum / nseq, ess_min=ess_min)
    field = None
    if eval_field(args):                             # behind everything else, and draws nothing: the figures above are unchanged
        fz = torch.cat([initial_state_means(model, Xb) for _, Xb, _, _ in _subsampled(args, testset)])
        fm, fv = field_posterior(model, fz)
        field = (fz.cpu().numpy(), fm.cpu().numpy(), fv.cpu().numpy())
    flowd = None
    if eval_flow(args):                              # behind everything else: every figure above sees the draws it sees without it
        Xf = torch.cat([full for full, _, _, _ in _subsampled(args, testset)])     # all frames: the uniform grid dt * arange(T)
        flowd = (flow_diagnostics(model, Xf, L), flow_diagnostics(model, Xf, mean_field=True))
    forecast = None
    if args.eval_condition_frames:                   # behind everything else: every figure above sees the draws it sees without it
        K = args.eval_condition_frames
        fr = sq = 0
        fmse = fnl = ess_sum = 0.0
        ess_min = float('inf')
        wt_t = mse_t = unc_t = nl_t = None
        for _, Xb, tsb, nb in _subsampled(args, testset):
            pc = predict_conditional(model, Xb, L, K, **_grid_kw(tsb, nb))
            fut = _split_frames(K, Xb.shape[0], Xb.shape[1], nb)[2]
            wt = fut.sum(0).to(torch.float64)
            seqs = int(fut.any(dim=1).sum())
            if seqs:
                fmse += pc.fc_mse * float(wt.sum())
                fnl += pc.fc_nlpd * seqs
            fr += float(wt.sum())
            sq += seqs
            ess_sum += pc.ess.sum().item()
            ess_min = min(ess_min, pc.ess.min().item())
            parts = [torch.nan_to_num(v) * wt for v in (pc.fc_mse_t, pc.fc_mse_uncond_t, pc.fc_nlpd_t)]
            mse_t, unc_t, nl_t = parts if wt_t is None else (mse_t + parts[0], unc_t + parts[1], nl_t + parts[2])
            wt_t = wt if wt_t is None else wt_t + wt
        froll = predict_conditional(model, first[:3].contiguous(), L, K, T_custom=args.Troll * first.shape[1])
        forecast = (dict(cond_frames=K, fc_mse=fmse / fr if fr else float('nan'), fc_mse_uncond=float(unc_t.sum() / wt_t.sum()),
                         fc_nlpd=fnl / sq if sq else float('nan'), fc_mse_t=_nullable(mse_t / wt_t), fc_nlpd_t=_nullable(nl_t / wt_t),
                         cond_ess_mean=ess_sum / nseq, cond_ess_min=ess_min), froll.mean.cpu().numpy(), froll.var.cpu().numpy())
    torch.cuda.synchronize()
    ms = (time.time() - t0) * 1e3

    os.makedirs(args.save, exist_ok=True)
    out = dict(mse=mse, std=std, mse_t=(per_step / per_frame).tolist(), nll=nll / nseq, nlpd=nlpd / nseq, nll_t=(nll_step / per_frame).tolist(), L=L, sequences=nseq, T=T, count=int(total[0]),
               rollout_sequences=int(roll.mean.shape[0]), rollout_T=int(roll.mean.shape[1]), rollout_mse=roll.mse, ms=ms,
               checkpoint=os.path.abspath(fname), ranks=1)
    if args.subsample_frames:
        out['subsample_frames'] = args.subsample_frames
    if args.ragged_frames:
        out['ragged_frames'] = args.ragged_frames
    if marginal is not None:
        out.update(marginal)
    if field is not None:
        out.update(field_points=int(field[0].shape[0]), field_var_mean=float(field[2].mean()), field_var_max=float(field[2].max()))
        for name, arr in zip(('field_z.npy', 'field_mean.npy', 'field_var.npy'), field):
            np.save(os.path.join(args.save, name), arr)
    if flowd is not None:
        fs, fm = flowd
        out.update(flow_logdet_mean=float(fs['logdet'][..., -1].mean()), flow_logdet_absmax=float(fs['logdet'].abs().max()),
                   flow_ftle_mean=float(fs['ftle'].mean()), flow_ftle_max=float(fs['ftle'].max()),
                   flow_div_absmean=float(fs['div'].abs().mean()), flow_div_absmean_meanfield=float(fm['div'].abs().mean()))
        for d, suffix in ((fs, ''), (fm, '_mean')):
            np.save(os.path.join(args.save, 'flow_phi%s.npy' % suffix), d['Phi'].cpu().numpy())
            np.save(os.path.join(args.save, 'flow_logdet%s.npy' % suffix), d['logdet'].numpy())
            np.save(os.path.join(args.save, 'flow_div%s.npy' % suffix), d['div'].numpy())
    if forecast is not None:
        out.update(forecast[0])
        np.save(os.path.join(args.save, 'forecast_mean.npy'), forecast[1])
        np.save(os.path.join(args.save, 'forecast_var.npy'), forecast[2])
    np.save(os.path.join(args.save, 'rollout_mean.npy'), roll.mean.cpu().numpy())
    np.save(os.path.join(args.save, 'rollout_var.npy'), roll.var.cpu().numpy())
    with open(os.path.join(args.save, 'eval.json'), 'w') as f:
        json.dump(out, f)
    print(json.dumps(out))
    sys.stdout.flush()
    return out


if __name__ == '__main__':
    main()
