"""ODE right-hand side wrapper and flow -- operator API of experiments/model/core/flow.py.

The reference hands ``ODEfunc`` to torchdiffeq, which calls it 1 (euler) or 4 (rk4) times per step
from Python.  Here ``Flow.forward`` is ONE persistent HIP kernel for all MC draws: each wavefront (or
team of four) integrates one trajectory over the whole grid.  Solvers: the fixed-grid 'euler', 'rk4'
(= torchdiffeq's 3/8 rule) and 'midpoint' (csrc/gp_forward.hip), and the adaptive 'dopri5'
(csrc/gp_adaptive.hip: Dormand-Prince 5(4), one step-size controller per trajectory, steps landing
on ``ts`` -- it agrees with torchdiffeq's to the tolerances, not step by step; with
``dense_output`` the steps are free of ``ts`` and the outputs are interpolated, as torchdiffeq
does).  The fixed-grid solvers take ``substeps`` equal steps inside every interval of ``ts``
(1 by default; the reference's --ts_dense_scale, torchdiffeq's options=dict(step_size=...)), so
that where the observations are does not set the step size; nothing between the output times is
stored or returned.  The rest of the
reference's --solver list (bdf, adams, explicit_adams, fixed_adams) is refused: ops.REFUSED_SOLVERS.
"""
import os

import torch
import torch.nn as nn

from ... import ops

EVALS_PER_STEP = {'euler': 1, 'rk4': 4, 'midpoint': 2}


class ODEfunc(nn.Module):
    def __init__(self, diffeq, order):
        super().__init__()
        self.diffeq = diffeq
        self.order = order
        self.register_buffer('_num_evals', torch.tensor(0.))
        self._host_evals = None                      # count of the last fused solve, not yet written to the buffer
        self._counts = None                          # adaptive solve: its per-trajectory counts, still on the device

    def before_odeint(self, rebuild_cache):
        self._host_evals = self._counts = None
        self._num_evals.fill_(0)
        if rebuild_cache:
            self.diffeq.build_cache()

    def _set_evals(self, n):
        """The fused rollout knows its evaluation count on the host: the ``_num_evals`` buffer (a state_dict entry of the
        reference, flow.py:14) is brought up to date when somebody looks -- not by a fill and an add on the device in every step."""
        self._host_evals, self._counts = float(n), None

    def _set_counts(self, counts):
        """An adaptive solve: the count is data, ([L,] N, 4) int32 on the device.  Kept as it is -- no synchronisation, nothing a
        graph capture could not record -- and reduced to the largest evaluation count when somebody looks."""
        self._host_evals, self._counts = None, counts

    def _resolve_counts(self):
        if self._counts is not None:
            c, self._counts = self._counts, None
            self._host_evals = float(c[..., 3].max().item()) if c.numel() else 0.0

    def _flush_evals(self):
        self._resolve_counts()
        if self._host_evals is not None:
            self._num_evals.fill_(self._host_evals)
            self._host_evals = None

    def num_evals(self):
        self._resolve_counts()
        return self._host_evals if self._host_evals is not None else self._num_evals.item()

    def _load_from_state_dict(self, *args, **kwargs):
        # the loaded buffer is the count now: a pending one of an earlier solve must not overwrite it at the next look
        self._host_evals = self._counts = None
        super()._load_from_state_dict(*args, **kwargs)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        self._flush_evals()
        super()._save_to_state_dict(destination, prefix, keep_vars)

    def first_order(self, sv):
        return self.diffeq(sv)

    def second_order(self, sv):
        q = sv.shape[1] // 2
        return torch.cat([sv[:, q:], self.diffeq(sv)], 1)

    def forward(self, t, sv):
        """One RHS evaluation (flow.py:40-45); autonomous, ``t`` ignored."""
        self._flush_evals()
        self._num_evals += 1
        return self.first_order(sv) if self.order == 1 else self.second_order(sv)


def dense_output_default():
    """GPODE_DOPRI5_DENSE: unset, empty or 0 -> False; anything else -> True."""
    return os.environ.get('GPODE_DOPRI5_DENSE', '0').strip() not in ('', '0')


def substeps_of_dense_scale(ts_dense_scale):
    """--ts_dense_scale -> solver steps per output interval, with the reference's meaning: compute_ts_dense (torch_utils.py) places
    linspace(t1, t2, scale)[:-1] in every interval -- scale - 1 steps -- and leaves the grid alone for scale <= 2."""
    sub = max(int(ts_dense_scale) - 1, 1)
    if sub > ops.MAX_SUBSTEPS:
        raise SystemExit('--ts_dense_scale %d asks for %d solver steps per output interval; at most %d (--ts_dense_scale %d) are built'
                         % (ts_dense_scale, sub, ops.MAX_SUBSTEPS, ops.MAX_SUBSTEPS + 1))
    return sub


class Flow(nn.Module):
    def __init__(self, diffeq, order=2, solver='dopri5', atol=1e-6, rtol=1e-6, use_adjoint=False, max_steps=None, dense_output=None,
                 substeps=1):
        """``substeps`` (an int in 1 ... ops.MAX_SUBSTEPS): read by 'euler', 'midpoint' and 'rk4' only, and ignored by 'dopri5', as
        ``atol`` / ``rtol`` / ``max_steps`` / ``dense_output`` are ignored by the others.  Every interval [ts[t], ts[t+1]] of every
        trajectory is integrated in ``substeps`` equal steps; the outputs stay at ``ts``.  Time grids per sequence, z0 per draw and
        several draws work with it unchanged; 1 is the launch it always was."""
        super().__init__()
        self.odefunc = ODEfunc(diffeq, order)
        self.solver = solver
        # read by 'dopri5' only (as in torchdiffeq).  The reference's defaults of 1e-6 are at the fp32 floor: the controller then
        # works against rounding as much as against truncation error -- Flow(..., atol=, rtol=) is the knob
        self.atol, self.rtol = atol, rtol
        self.max_steps = max_steps         # dopri5: accepted steps a trajectory may take; None = 4 (T - 1)
        self.use_adjoint = use_adjoint     # same forward; gradients are discretise-then-optimise either way
        # dopri5: steps cut at ts[-1] only, interior outputs interpolated.  None = the environment decides (GPODE_DOPRI5_DENSE,
        # unset or 0: off), so that everything built through build_model can be switched without a flag; ignored by fixed grids
        self.dense_output = dense_output_default() if dense_output is None else bool(dense_output)
        self.substeps = substeps
        self._last_counts = None

    def forward(self, z0, ts, draws=None):
        """z0 (N,D), ts (T,) -> zt (N,T,D) for a fresh function draw (flow.py:68-86).  ``draws`` = L: L fresh draws integrated in
        one pass -> (L,N,T,D), the stack ODEGPVAE.sample_trajectories builds from L calls (odegpvae.py:41-44); ``_num_evals`` ends
        at the count of ONE solve, as it does after the reference's last call.  z0 (L,N,D): draw l starts from z0[l].
        ts (N,T): sequence n of every draw is integrated over its own output times ts[n] -- the same launch with a row stride
        on the grid; a first axis other than N is refused (ops.GpodeError).
        'dopri5': a trajectory that exhausts ``max_steps`` or whose step underflows is NaN from the output it missed (status in
        ``last_counts``); the others are unaffected."""
        try:
            ops.check_solver(self.solver)
        except ops._lib.GpodeError as e:
            raise ValueError(str(e)) from None
        gp = self.odefunc.diffeq
        self._last_counts = None
        if self.solver == 'dopri5':
            return ops.flow(gp, z0, ts, self.odefunc.order, self.solver, draws,
                            (self.rtol, self.atol, self.max_steps, self._take_counts, bool(self.dense_output)))
        zt = ops.flow(gp, z0, ts, self.odefunc.order, self.solver, draws, substeps=self.substeps)
        self.odefunc._set_evals(EVALS_PER_STEP[self.solver] * (ts.shape[-1] - 1) * self.substeps)
        return zt

    def sensitivity(self, z0, ts, v0=None, draws=None, cache=None):
        """(zt, Phi): the trajectories of ``forward`` and their first-order sensitivity to the initial state, in forward mode
        (ops.rollout_jvp: the exact derivative of the discrete solver, ``substeps`` included; no autograd).  v0 None: Phi
        ([L,] N,T,D,D) is the state-transition matrix d z_t / d z0, Phi[..., 0, :, :] = I.  v0 ([L,] N,K,D): Phi = vt ([L,] N,T,K,D),
        row k the image Phi_t v0[k].  A fresh function draw is fixed as ``forward`` fixes it (``draws`` = L: L of them), unless
        ``cache`` hands one over (``diffeq.cache`` after a build).  'dopri5' is refused: its steps depend on the state."""
        if self.solver == 'dopri5':
            raise ValueError(ops.DOPRI5_TANGENT)
        try:
            ops.check_solver(self.solver)
        except ops._lib.GpodeError as e:
            raise ValueError(str(e)) from None
        gp = self.odefunc.diffeq
        pad = getattr(gp, 'width_pad', None)
        with torch.no_grad():
            if cache is None and draws is not None and pad is not None:     # a zero-padded width builds its draws one by one
                per = [self.sensitivity(z0[l] if z0.dim() == 3 else z0, ts, None if v0 is None else (v0[l] if z0.dim() == 3 else v0))
                       for l in range(draws)]
                return torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per])
            if cache is None:
                cache = gp.build_cache() if draws is None else gp.build_cache(draws=draws)
            zt, vt = ops.rollout_jvp(cache, z0, ts, self.odefunc.order, self.solver, v0=v0, substeps=self.substeps, pad=pad)
        return zt, (vt.transpose(-1, -2).contiguous() if v0 is None else vt)

    def _take_counts(self, counts):
        self._last_counts = counts
        self.odefunc._set_counts(counts)

    @property
    def last_counts(self):
        """'dopri5': ([L,] N, 4) int32 of the last solve, on the device -- accepted steps, rejected steps, status (0 ok, 1 step
        budget exhausted, 2 step size underflow, 3 ts not increasing), evaluations of f.  None after a fixed-grid solve."""
        return self._last_counts

    def num_evals(self):
        """Evaluations of f in the last solve; 'dopri5': the largest count over the trajectories (read from the device here)."""
        return self.odefunc.num_evals()

    def kl(self):
        return self.odefunc.diffeq.kl()
