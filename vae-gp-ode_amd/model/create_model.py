"""Model factory + ELBO (operator API of experiments/model/create_model.py)."""
import os

import torch
from torch.distributions import kl_divergence as kl

from .core.flow import Flow, substeps_of_dense_scale
from .core.odegpvae import ODEGPVAE
from .core.svpy import SVGP_Layer
from .core.vae import VAE


_FUSED_LOSS = os.environ.get('GPODE_UNFUSED_LOSS', '0') != '1'


def build_model(args):
    """GP vector field -> Flow -> VAE -> ODEGPVAE from the argument namespace of main.py (create_model.py:16-33 reads the
    same fields).  The construction order fixes the order of the numpy draws that initialise the GP parameters.
    ``ts_dense_scale`` (optional, 2 when absent): scale - 1 solver steps per output interval for the fixed-grid solvers; a value the
    kernels are not built for exits here, ahead of any device work."""
    a = args
    substeps = substeps_of_dense_scale(getattr(a, 'ts_dense_scale', 2))
    field = SVGP_Layer(a.D_in, a.D_out, a.num_inducing, a.num_features, q_diag=a.q_diag, dimwise=a.dimwise, device=a.device,
                       kernel=a.kernel)
    return ODEGPVAE(flow=Flow(field, order=a.ode, solver=a.solver, use_adjoint=a.use_adjoint, substeps=substeps),
                    vae=VAE(frames=a.frames, n_filt=a.n_filt, latent_dim=a.latent_dim, device=a.device, order=a.ode),
                    num_observations=a.Ndata, steps=a.frames, order=a.ode, dt=a.dt)


def elbo(model, X, Xrec, s0_mu, s0_logv, v0_mu, v0_logv, L):
    """-> (mean log-likelihood per sequence, mean KL(q(z0)||p), KL(q(u)||p)) (create_model.py:37-58)."""
    q = model.vae.encoder.q_dist(s0_mu, s0_logv, v0_mu, v0_logv)
    kl_reg = kl(q, model.vae.prior).sum(-1)
    lhood = model.vae.decoder.log_prob_rowsum(X, Xrec, L).mean(0)  # == log_prob(...).sum([2,3,4,5]).mean(0)
    return lhood.mean(), kl_reg.mean(), model.flow.kl()


def _compact_index(model, data, n_obs, counts):
    """compute_loss(compact=True): its refusals, then the index of the observed frames (vae_ops.frame_index)"""
    from .. import vae_ops as V
    if n_obs is None:
        raise ValueError('compute_loss: compact=True needs n_obs, the frame count of every sequence of the padded minibatch')
    field = model.flow.odefunc.diffeq
    if not _FUSED_LOSS:
        raise ValueError('compute_loss: compact=True has one loss route, from the logits; it is not available under GPODE_UNFUSED_LOSS=1')
    if not hasattr(field, 'us_packed') or model.vae.decoder.distribution != 'bernoulli':
        raise ValueError('compute_loss: compact=True needs the Bernoulli decoder and the fused loss stage (a %s decoder is not covered)'
                         % model.vae.decoder.distribution)
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise ValueError('compute_loss: compact=True on several ranks is not built: the cross-rank BatchNorm (parallel.count_all) takes a '
                         "rank's image count to be proportional to its share of the sequences, which taking the padding out breaks")
    return V.frame_index(n_obs, data.shape[1], counts=counts)


IW_MAX_DRAWS, IW_MAX_ROWS = 64, 65535


def _iw_loss(model, data, L, K, grid, n_obs, compact):
    """compute_loss(iw_draws=K): its refusals, then the importance-weighted bound (vae_ops.elbo_iw)"""
    from .. import vae_ops as V
    if compact:
        raise ValueError('compute_loss: iw_draws is not built for compact=True (the compact ragged route); use n_obs alone')
    if not _FUSED_LOSS:
        raise ValueError('compute_loss: iw_draws has one loss route, from the logits; it is not available under GPODE_UNFUSED_LOSS=1')
    if isinstance(K, bool) or int(K) != K or not 1 <= K <= IW_MAX_DRAWS:
        raise ValueError('compute_loss: iw_draws must be an integer in 1..%d (one lane of a wavefront per draw), got %r' % (IW_MAX_DRAWS, K))
    K, N = int(K), data.shape[0]
    if L * K * N > IW_MAX_ROWS:
        raise ValueError('compute_loss: L * iw_draws * N = %d x %d x %d = %d likelihood rows, more than the %d the loss stage takes'
                         % (L, K, N, L * K * N, IW_MAX_ROWS))
    field = model.flow.odefunc.diffeq
    if not hasattr(field, 'us_packed') or model.vae.decoder.distribution != 'bernoulli':
        raise ValueError('compute_loss: iw_draws needs the Bernoulli decoder and the fused loss stage (a %s decoder is not covered)'
                         % model.vae.decoder.distribution)
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise ValueError('compute_loss: iw_draws on several ranks is out of scope: the sharding is per sequence and would probably work, '
                         'but it is untested')
    logits, _, _, lw = model(data, L, logits=True, z0_draws=K, **grid)
    lpart, _ = V.sigmoid_loglik_parts(data, logits, L * K * N, n_obs)
    loss, iw_nll, kl_mc, kl_u, ess = V.elbo_iw(lpart, lw, field.Um.optvar, field.us_packed(), L, K, N, field.M, model.num_observations)
    model.last_ess = ess.detach()                    # the mean effective sample size of the step: a device scalar, not read back
    return loss, iw_nll, kl_mc, kl_u


def compute_loss(model, data, L, ts=None, n_obs=None, compact=False, counts=None, iw_draws=None):
    """-> (loss, nll, kl_reg, kl_u) (create_model.py:61-73).  Same terms as elbo() above; the per-row pieces go through
    three fused launches (KL rows, likelihood row sums, loss algebra) instead of ~25 elementwise ones.
    ``ts`` (N,T): the observation time of every frame of every sequence (ODEGPVAE.forward); None = the uniform grid, the call as
    it always was.
    ``n_obs`` (N,) int32 on the device: a ragged minibatch, padded to T frames -- frame t of sequence n is observed iff t < n_obs[n].
    The likelihood of a sequence sums its observed frames only (nothing is renormalised by the count: the ELBO is a sum over
    observations), a padded frame gets exactly zero gradient at its logits, and what the padded targets hold is never read into a
    result.  The padded frames are still integrated and decoded (the forecast at the padding times, whose columns of ``ts`` must
    keep every row increasing) and enter the decoder's training-mode BatchNorm statistics.  The counts are not read back.
    ``compact=True`` (needs ``n_obs``): the padded frames are taken out in front of the decoder (vae_ops.frame_index, gather_frames).
    The states are integrated over the whole padded grid as before, the decoder runs on the L P observed frames only, so its
    BatchNorm batch and running statistics are over observed frames, and the loss stage reads compact logits
    (gpode_sigmoid_loglik_fwd_pk, gpode_elbo_all_fwd; backward: gpode_elbo_all_bwd and gpode_sigmoid_loglik_bwd_pk).  What the padded
    columns of ``ts`` and the padded target frames hold then reaches no result.  The index needs the counts on the host: ``counts`` (a
    host sequence) if the caller has them, else ``n_obs`` is read back once per call (one synchronisation).  One loss route, from the
    logits: refused under GPODE_UNFUSED_LOSS=1, for a non-Bernoulli decoder, and with several ranks.
    ``iw_draws`` = K in 1..64: train on the importance-weighted bound -- K initial states z0_{k,n} ~ q(z0 | x_n) per sequence, shared by
    the L function draws; with lw[k,n] = log p(z0) - log q(z0 | x), ll[l,k,n] the log-likelihood of sequence n under (z0_{k,n}, f_l)
    and iw[l,n] = logsumexp_k (ll + lw) - log K:  loss = -(nobs mean_{l,n} iw - kl_u) -> (loss, iw_nll = -mean iw, kl_mc = -mean lw,
    kl_u).  The weighting is over z0 only, the mean over the function draws stays outside the log; the analytic
    KL(q(z0) || p) does not appear, lw stands for it.  K = 1 is legal: a = ll + lw.  The mean effective sample size of the step is
    left in ``model.last_ess`` (a device scalar, not read back).  Works with ``ts`` and ``n_obs``; L K N <= 65535.  Refused:
    compact=True, GPODE_UNFUSED_LOSS=1, a non-Bernoulli decoder, several ranks (sharding is per sequence and would probably work, but
    it is untested).  None: the call as it always was."""
    from .. import vae_ops as V
    grid = {} if ts is None else {'ts': ts}
    if iw_draws is not None:
        return _iw_loss(model, data, L, iw_draws, grid, n_obs, compact)
    index = None
    if compact:                                      # the index stands for the counts from here on
        index, n_obs = _compact_index(model, data, n_obs, counts), None
        grid['obs_index'] = index
    field = model.flow.odefunc.diffeq
    if compact or (_FUSED_LOSS and hasattr(field, 'us_packed') and model.vae.decoder.distribution == 'bernoulli'):
        # the decoder stops at its logits; sigmoid + likelihood row sums are one pass over them, and the three KL / mean / loss
        # launches one more (gpode_sigmoid_loglik_fwd, gpode_elbo_all_fwd)
        logits, (s0_mu, s0_logv), (v0_mu, v0_logv) = model(data, L, logits=True, **grid)
        lpart, _ = V.sigmoid_loglik_parts(data, logits, L * data.shape[0], n_obs, index=index)
        return V.elbo_all(lpart, s0_mu, s0_logv, v0_mu, v0_logv, field.Um.optvar, field.us_packed(), field.M, model.num_observations)
    Xrec, (s0_mu, s0_logv), (v0_mu, v0_logv) = model(data, L, **grid)
    kl_rows = model.vae.encoder.kl_rows(s0_mu, s0_logv, v0_mu, v0_logv)               # (N,)
    lhood_rows = model.vae.decoder.log_prob_rowsum(data, Xrec, L, n_obs=n_obs)        # (L, N)
    out = V.elbo_terms(lhood_rows, kl_rows, model.flow.kl(), model.num_observations)
    return out[0], out[1], out[2], out[3]


_ONE = {}


def backward(loss):
    """``loss.backward()`` (main.py:210) with the root gradient handed over: autograd otherwise fills a fresh ones-tensor in every
    step -- one more few-microsecond launch on the chain of a step that is bound by the number of such launches."""
    key = (loss.device, loss.dtype)
    if key not in _ONE:
        _ONE[key] = torch.ones((), dtype=loss.dtype, device=loss.device)
    loss.backward(gradient=_ONE[key])


def compute_test_error(X, Xrec):
    assert list(X.shape) == list(Xrec.shape), f'incorrect shapes X: {list(X.shape)}, X_Rec: {list(Xrec.shape)}'
    return torch.mean((Xrec - X) ** 2)
