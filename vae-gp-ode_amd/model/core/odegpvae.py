"""Composite model: encode -> L x integrate -> decode (operator API of experiments/model/core/odegpvae.py)."""
import torch
import torch.nn as nn


class ODEGPVAE(nn.Module):
    def __init__(self, flow, vae, num_observations, steps, order=2, dt=0.1):
        super().__init__()
        self.flow = flow
        self.vae = vae
        self.num_observations = num_observations
        self.dt = dt
        self.v_steps = steps
        self.order = order

    def build_decoding(self, ztL, dims, logits=False):
        """ztL (L,N,T,order*q) -> Xrec (L,N,T,nc,d,d); only positions are decoded for order 2 (odegpvae.py:18-35)."""
        L, N, T, nc, d, _ = dims
        lat = ztL if self.order == 1 else ztL[..., :ztL.shape[-1] // 2]
        return (self.vae.decoder(lat, logits=True) if logits else self.vae.decoder(lat)).view([L, N, T, nc, d, d])

    def decode_observed(self, ztL, index, logits=False):
        """ztL (L,N,T,order*q) -> the decodings of the OBSERVED frames only, (L P, nc, d, d) ordered (l, n, t): the latent states (the
        positions for order 2) of the frames ``index`` lists (vae_ops.frame_index) are gathered in one launch and the decoder runs on
        L P images -- a padded frame is not decoded and enters no BatchNorm statistic."""
        from ... import vae_ops
        lat = vae_ops.gather_frames(ztL, index, ztL.shape[-1] // self.order)
        return self.vae.decoder(lat, logits=True) if logits else self.vae.decoder(lat)

    def sample_trajectories(self, z0, T, L=1, ts=None):
        """L independent function draws, each shared by the whole minibatch (odegpvae.py:37-45).  z0 (L,N,D): draw l starts from
        its own sample z0[l] of the initial states (encode_initial_state(X, draws=L)).
        ``ts`` (N,T): the observation times of every sequence (shared by the draws); None = the uniform grid dt * arange(T)."""
        if z0.dim() == 3 and z0.shape[0] != L:
            raise ValueError('sample_trajectories: z0 holds initial states for %d draws, L = %d' % (z0.shape[0], L))
        if ts is not None:
            N = z0.shape[-2]
            if ts.dim() != 2 or tuple(ts.shape) != (N, T):
                raise ValueError('sample_trajectories: ts must be (N,T) = (%d,%d), one row of observation times per sequence; got %s'
                                 % (N, T, tuple(ts.shape)))
            ts = ts.to(device=z0.device, dtype=torch.float32).contiguous()
        else:
            key = (T, str(z0.device))
            if getattr(self, '_ts_key', None) != key:        # the grid dt * arange(T) is a constant of the run: build it once
                self._ts, self._ts_key = self.dt * torch.arange(T, dtype=torch.float, device=z0.device), key
            ts = self._ts
        if L == 1:
            return self.flow(z0[0] if z0.dim() == 3 else z0, ts).unsqueeze(0)
        field = self.flow.odefunc.diffeq
        if getattr(field, 'batched_draws_supported', lambda: False)():
            # the L draws in ONE pass: K_uu factored once, one rollout launch over L * N trajectories, one reverse sweep
            return self.flow(z0, ts, draws=L)
        return torch.stack([self.flow(z0[l] if z0.dim() == 3 else z0, ts) for l in range(L)], 0)

    def _pair_encoders(self):
        from ... import vae_ops
        enc, vel = self.vae.encoder, self.vae.encoder_v
        return (vae_ops.pack_bn_gathers() and enc.training and vel.training and
                all(m.training for m in (enc.cnn[1], enc.cnn[4], vel.cnn[1], vel.cnn[4])))

    def encode_initial_state(self, X, draws=None):
        """q(z0 | X): position code from the first frame, velocity code (order 2) from the first ``v_steps`` frames stacked as
        channels; returns the reparameterised sample and the (mean, log-variance) pairs the ELBO needs (odegpvae.py:55-63).
        ``draws`` = L: L samples per sequence instead of one, z0 (L,N,order*q), and their importance log-weights
        lw (L,N) = log p(z0) - log q(z0 | X) under the standard-normal prior -> (z0, lw, code_s, code_v).  With gradients enabled and
        an encoder that requires them, z0 and lw are differentiable (training on the importance-weighted bound, compute_loss(iw_draws=));
        under torch.no_grad() (evaluation) the draws are written in place, forward only."""
        pos = self.vae.encoder
        if draws is not None:
            from ... import vae_ops
            L = int(draws)
            mu_s, logv_s = pos(X[:, 0])
            N, q = mu_s.shape
            if torch.is_grad_enabled() and mu_s.requires_grad:
                eps_s = pos.draws_eps(mu_s, L)
                if self.order == 1:
                    z0, lw = vae_ops.reparam_draws_train(mu_s, logv_s, eps_s.to(mu_s))
                    return z0, lw, (mu_s, logv_s), (None, None)
                vel = self.vae.encoder_v
                mu_v, logv_v = vel(X[:, 0:self.v_steps].squeeze(2))
                eps_v = vel.draws_eps(mu_v, L)
                z0, lw = vae_ops.reparam_draws_train(mu_s, logv_s, eps_s.to(mu_s), mu_v, logv_v, eps_v.to(mu_v))
                return z0, lw, (mu_s, logv_s), (mu_v, logv_v)
            z0 = torch.empty((L, N, self.order * q), dtype=torch.float32, device=mu_s.device)
            _, lw = pos.sample_draws(mu_s, logv_s, L, out=z0, col=0)
            if self.order == 1:
                return z0, lw, (mu_s, logv_s), (None, None)
            vel = self.vae.encoder_v
            mu_v, logv_v = vel(X[:, 0:self.v_steps].squeeze(2))   # the frames as channels; a batch of one sequence keeps its axis
            vel.sample_draws(mu_v, logv_v, L, out=z0, col=q, lw=lw)
            return z0, lw, (mu_s, logv_s), (mu_v, logv_v)
        if self.order == 2 and self._pair_encoders():
            # data parallelism with global-minibatch BatchNorm: the two encoders run in lockstep and share their statistics exchanges
            vel = self.vae.encoder_v
            (mu_s, logv_s), (mu_v, logv_v) = pos.forward_pair(pos, X[:, 0], vel, torch.squeeze(X[:, 0:self.v_steps]))
            z0 = pos.sample(mu=mu_s, logvar=logv_s)
            return torch.concat([z0, vel.sample(mu=mu_v, logvar=logv_v)], dim=1), (mu_s, logv_s), (mu_v, logv_v)
        mu_s, logv_s = pos(X[:, 0])
        z0 = pos.sample(mu=mu_s, logvar=logv_s)
        if self.order == 1:
            return z0, (mu_s, logv_s), (None, None)
        vel = self.vae.encoder_v
        mu_v, logv_v = vel(torch.squeeze(X[:, 0:self.v_steps]))
        return torch.concat([z0, vel.sample(mu=mu_v, logvar=logv_v)], dim=1), (mu_s, logv_s), (mu_v, logv_v)

    def forward(self, X, L=1, T_custom=None, logits=False, ts=None, obs_index=None, z0_draws=None):
        """X (N,T,nc,d,d) -> (Xrec (L,N,T',nc,d,d), (mu_s, logv_s), (mu_v, logv_v)); T' = T_custom or T (odegpvae.py:48-70).
        ``ts`` (N,T'): the time at which frame t of sequence n was observed -- the latent state is integrated to those times and
        decoded there; None = the uniform grid dt * arange(T').  The encoders read the leading frames as they stand: for a
        second-order model the first ``v_steps`` frames are taken to be consecutive.
        ``obs_index`` (vae_ops.frame_index of a ragged minibatch): the states are integrated over the whole padded grid as ever, but
        only the observed frames are decoded (decode_observed) -- in place of Xrec stands the compact (L P, nc, d, d) tensor; None:
        the calls as they always were.
        ``z0_draws`` = K (training on the importance-weighted bound): K initial states per sequence, z0 (K,N,D) integrated as K N
        trajectories that the L function draws share (a ``ts`` (N,T') is tiled to (K N, T')); L K N T' frames are decoded, ordered
        (l,k,n,t) -> (Xrec (L, K N, T', nc, d, d), (mu_s, logv_s), (mu_v, logv_v), lw (K,N)).  None: the call as it was."""
        N, T, nc, d, _ = X.shape
        horizon = T_custom if T_custom else T
        if z0_draws is not None and obs_index is not None:
            raise ValueError('forward: z0_draws and obs_index exclude each other (the compact ragged route has no importance-weighted form)')
        if obs_index is not None and (obs_index.N, obs_index.T) != (N, horizon):
            raise ValueError('forward: obs_index lists the frames of (N,T\') = (%d,%d), the minibatch is (%d,%d)'
                             % (obs_index.N, obs_index.T, N, horizon))
        if ts is not None and (ts.dim() != 2 or tuple(ts.shape) != (N, horizon)):
            raise ValueError('forward: ts must be (N,T\') = (%d,%d), one row of observation times per sequence; got %s'
                             % (N, horizon, tuple(ts.shape)))
        field = self.flow.odefunc.diffeq
        src = getattr(self.vae.encoder, 'eps_source', None)
        if src is not None and src is getattr(field, 'noise_source', None) and hasattr(field, 'predraw'):
            # device noise: the function draw(s) AND the encoders' reparameterisation draws in one launch, ahead of the encoder
            # (the same order of draws whether or not the cache build then runs on the side stream)
            src.reserve((1 if z0_draws is None else int(z0_draws)) * N * (self.vae.encoder.fc.out_features // 2) * self.order)
            field.predraw(L if L > 1 and field.batched_draws_supported() else None)
        if hasattr(field, 'prebuild_cache') and (L == 1 or field.batched_draws_supported()):
            field.prebuild_cache(None if L == 1 else L)   # overlap mode only: the cache of the draw(s) builds next to the encoder
        if z0_draws is not None:
            K = int(z0_draws)
            z0, lw, code_s, code_v = self.encode_initial_state(X, draws=K)
            ztL = self.sample_trajectories(z0.view(K * N, z0.shape[-1]), horizon, L, ts=None if ts is None else ts.repeat(K, 1))
            return self.build_decoding(ztL, (L, K * N, horizon, nc, d, d), logits), code_s, code_v, lw
        z0, code_s, code_v = self.encode_initial_state(X)
        ztL = self.sample_trajectories(z0, horizon, L, ts=ts)
        if obs_index is not None:
            return self.decode_observed(ztL, obs_index, logits).view([L * obs_index.P, nc, d, d]), code_s, code_v
        return self.build_decoding(ztL, (L, N, horizon, nc, d, d), logits), code_s, code_v
