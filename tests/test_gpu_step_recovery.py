"""GPU: the training step AFTER one that did not run to its end.

Four pieces of state outlive a step -- vae_ops._deferred (deferred final reductions), ops._overlap (side-stream gradients waiting for
the optimiser), HipAdam._tables / _static_tabs (gradient-pointer tables) and graph._capture -- and a prebuilt GP cache on the layer.
Each is right only if the step before ran to its end.  Here a backward pass, a capture warm-up or a capture is aborted by a plain
Python exception (no GPU work fails, and no capture is aborted while the side stream is forked into it), and the steps that follow
must train exactly as if nothing had happened.

The reference of every comparison is the CONTROL: load_state_dict(init), a fresh HipAdam of the same kind, n eager steps on X under
the same switches.  Comparisons are torch.equal on every parameter and buffer: test_graph_replay_equals_eager_steps already holds
eager, replayed, overlap and deferred runs to bit equality, so there is no tolerance.  The aborted step runs on OTHER inputs (X2):
with the caching allocator, leftover memory of an identical step can hold exactly the right gradients.

The model is that test's first-order DF model at the smallest sizes that take the same paths (16 inducing points, 32 features, 4
sequences of 4 frames).  No test calls the public reset (vae_ops.reset_step_state) in mid-scenario: the recovery has to happen on its
own; the reset runs in every ``finally``, so that a failure here does not leak into the tests behind it."""
import copy
import types

import pytest
import torch

from step_recovery import owner_of, stale_table_entries

pytestmark = pytest.mark.gpu

SETTINGS = [(False, False, True), (False, True, True), ('gather', True, True), (True, True, False)]   # (bucketed, overlap, deferred)


class _Abort(RuntimeError):
    pass


def _raiser(g):
    raise _Abort('raised by the test inside the backward pass')


class _Scene:
    def __init__(self):
        from vae_gp_ode_amd.model.core.initialization import initialize_and_fix_kernel_parameters
        from vae_gp_ode_amd.model.core.noise import DeviceNoise
        from vae_gp_ode_amd.model.create_model import build_model
        from vae_gp_ode_amd.model.misc.torch_utils import seed_everything
        seed_everything(4)
        args = types.SimpleNamespace(D_in=6, D_out=6, num_inducing=16, num_features=32, dimwise=True, q_diag=False, device='cuda',
                                     kernel='DF', ode=1, solver='rk4', use_adjoint=False, frames=5, n_filt=8, latent_dim=6, Ndata=64, dt=0.1)
        self.m = build_model(args).cuda()
        initialize_and_fix_kernel_parameters(self.m, 2.0, 1.0)
        self.init = copy.deepcopy(self.m.state_dict())
        self.X = torch.rand(4, 4, 1, 28, 28, device='cuda')
        self.X2 = torch.rand(4, 4, 1, 28, 28, device='cuda')
        fixed = DeviceNoise(9).draw('DF', 6, 6, 16, 32, 'cuda')

        class FixedNoise:
            def draw(self, *a):
                return fixed
        self.field = self.m.flow.odefunc.diffeq
        self.field.noise_source = FixedNoise()
        self.eps = torch.randn(4, 6, device='cuda')
        self.enc = self.m.vae.encoder
        self._controls = {}

    def restore(self):
        self.m.load_state_dict(self.init)

    def optimiser(self, setting):
        """a fresh HipAdam of the setting's kind, and the process-wide switches of the setting"""
        from vae_gp_ode_amd import ops, vae_ops
        from vae_gp_ode_amd.optim import HipAdam
        bucketed, overlap, deferred = setting
        ops.set_overlap(overlap)
        opt = HipAdam(self.m.parameters(), lr=1e-3, bucketed=bucketed)
        vae_ops.set_deferred_reductions(deferred)
        return opt

    def loss(self, X):
        from vae_gp_ode_amd.model.create_model import compute_loss
        self.enc.next_eps = self.eps
        return compute_loss(self.m, X, 1)[0]

    def step_fn(self, opt, X=None):
        def step():
            opt.zero_grad()
            loss = self.loss(self.X if X is None else X)
            loss.backward()
            opt.step()
            return loss
        return step

    def state(self):
        torch.cuda.synchronize()
        return [p.detach().clone() for p in self.m.parameters()], [b.detach().clone() for b in self.m.buffers()]

    def control(self, setting, steps=2, prepare=None):
        """parameters and buffers after ``steps`` eager steps on X from ``init`` (computed once per setting, never modified)"""
        key = (setting, steps, prepare)
        if key not in self._controls:
            self.restore()
            if prepare is not None:
                prepare(self)
            opt = self.optimiser(setting)
            step = self.step_fn(opt)
            for _ in range(steps):
                step()
            state = self.state()
            assert opt.step_dev.tolist() == [steps, 0]
            self._controls[key] = state
        return self._controls[key]

    def assert_equals(self, want, what):
        names = [k for k, _ in self.m.named_parameters()], [k for k, _ in self.m.named_buffers()]
        for kind, ns, ws, gs in zip(('parameter', 'buffer'), names, want, self.state()):
            for n, w, g in zip(ns, ws, gs):
                assert torch.equal(w, g), '%s: %s %s differs from the control (max |difference| %.3e)' % (
                    what, kind, n, (w.double() - g.double()).abs().max().item())


@pytest.fixture(scope='module')
def scene():
    return _Scene()


@pytest.fixture(autouse=True)
def _clean_step_state():
    """every test starts from and leaves behind an empty carried-over state, whatever it or the one before it did"""
    from vae_gp_ode_amd import ops, vae_ops
    vae_ops.reset_step_state()
    try:
        yield
    finally:
        torch.cuda.synchronize()
        vae_ops.reset_step_state()
        ops.set_overlap(False)
        vae_ops.set_deferred_reductions(False)


class _Spy:
    """wraps _lib.call: the names (and arguments) of every entry point called while it is installed"""

    def __enter__(self):
        from vae_gp_ode_amd import _lib
        self._lib, self._real, self.calls = _lib, _lib.call, []

        def call(name, *args):
            self.calls.append((name, args))
            return self._real(name, *args)
        _lib.call = call
        return self

    def __exit__(self, *exc):
        self._lib.call = self._real

    def count(self, name):
        return sum(n == name for n, _ in self.calls)


def _aborted_backward(scene, opt, seen):
    """zero_grad, the loss of X2, and a backward pass that a hook on the encoder's fc.weight ends with an exception: behind the
    decoder's and the flow's backward, in front of the encoder's convolutions.  ``seen``: what the pass had left by then."""
    from vae_gp_ode_amd import ops, vae_ops

    def hook(g):
        seen['keep'], seen['pending'] = len(vae_ops._deferred['keep']), len(ops._overlap['pending'])
        _raiser(g)
    opt.zero_grad()
    loss = scene.loss(scene.X2)
    handle = scene.enc.fc.weight.register_hook(hook)
    try:
        with pytest.raises(_Abort):
            loss.backward()
    finally:
        handle.remove()


def _assert_nothing_carried_over():
    from vae_gp_ode_amd import ops, vae_ops
    assert vae_ops._deferred['keep'] == [], 'deferred scratch buffers outlive the step: %d' % len(vae_ops._deferred['keep'])
    assert vae_ops._deferred['queued'] is False, 'a flush is still marked as queued after the step'
    assert ops._overlap['pending'] == [], 'side-stream gradients outlive the step: %d' % len(ops._overlap['pending'])
    assert ops._overlap['kl'] is None, 'parked KL gradients outlive the step'


@pytest.mark.parametrize('setting', SETTINGS, ids=lambda s: 'bucketed=%s-overlap=%s-deferred=%s' % s)
def test_steps_after_an_aborted_backward_equal_the_control(scene, setting):
    """A1.  On the tree before the fix every setting failed: where ``deferred``, no gpode_flush_reductions at all for the two completed
    passes (autograd drops the aborted pass's callback and no later pass queues one); (True, True, False) on the parameters, the
    kernel's lengthscales first, by 3e-3 (the aborted pass's GP gradients are added to the first step's).  The count of flushes is
    the deterministic detector of the first: the parameter comparison alone could pass by luck on leftover memory."""
    want = scene.control(setting)
    bucketed, overlap, deferred = setting
    scene.restore()
    opt = scene.optimiser(setting)
    seen = {}
    with _Spy() as spy:
        _aborted_backward(scene, opt, seen)
        # the scenario is only worth anything if the aborted pass did leave state behind
        assert not deferred or seen['keep'] > 0, 'the aborted pass had recorded no deferred reduction: the test is vacuous'
        assert not overlap or seen['pending'] > 0, 'the aborted pass had left no side-stream gradients: the test is vacuous'
        assert opt.step_dev.tolist() == [0, 0]
        scene.restore()                              # the aborted forward advanced the BatchNorm buffers
        step = scene.step_fn(opt)
        step()
        step()
        torch.cuda.synchronize()
    flushes = spy.count('gpode_flush_reductions')
    assert flushes == (2 if deferred else 0), \
        '%d gpode_flush_reductions for 2 completed backward passes: gradients of the steps after the aborted one are never reduced' % flushes
    assert opt.step_dev.tolist() == [2, 0]
    scene.assert_equals(want, 'two steps after an aborted backward, %s' % (setting,))
    _assert_nothing_carried_over()


def test_a_capture_warmup_that_aborts_then_a_second_capture(scene):
    """A2.  The benchmark's sequence 'capture failed, carry on in this process': the first warm-up step of a GraphedStep aborts in its
    backward, the constructor propagates; a second GraphedStep (fresh optimiser, restored model) is then built and replayed."""
    from vae_gp_ode_amd.graph import GraphedStep
    setting = (False, True, True)
    want = scene.control(setting)
    scene.restore()
    opt = scene.optimiser(setting)
    calls, seen = {'n': 0}, {}

    def aborting_step():
        calls['n'] += 1
        if calls['n'] == 1:
            _aborted_backward_raises(scene, opt, seen)
        return scene.step_fn(opt)()
    with pytest.raises(_Abort):
        GraphedStep(aborting_step, warmup=2)
    assert calls['n'] == 1 and seen['keep'] > 0 and seen['pending'] > 0, ('the first warm-up call did not abort as planned', calls, seen)
    scene.restore()
    opt = scene.optimiser(setting)
    with _Spy() as spy:
        gs = GraphedStep(scene.step_fn(opt), warmup=1)
        flushes = spy.count('gpode_flush_reductions')
    assert flushes == 2, '%d gpode_flush_reductions for the warm-up step and the captured one' % flushes
    gs()
    torch.cuda.synchronize()
    assert opt.step_dev.tolist() == [2, 0]
    scene.assert_equals(want, 'a warm-up step and a replay after an aborted warm-up')
    _assert_nothing_carried_over()


def _aborted_backward_raises(scene, opt, seen):
    """_aborted_backward for a caller that wants the exception: the pass is aborted and the exception raised again"""
    _aborted_backward(scene, opt, seen)
    raise _Abort('the warm-up step aborted in its backward pass')


def _reset_adam(opt):
    """the optimiser's own state as HipAdam.__init__ leaves it (moments and update count); its tables are left as they are"""
    for t in opt.exp_avg + opt.exp_avg_sq:
        t.zero_()
    opt.step_dev.zero_()
    opt.step_count = 0


def test_a_failed_capture_leaves_the_optimiser_usable(scene):
    """A3.  The step function raises as its last statement during the capture (behind opt.step(): every stream is joined), so the
    uploads registered with graph.after_capture never run.  (b) is host state only and comes first: before the fix it fails there and
    nothing ever reads the table of zeros.  (c) captures again on the SAME optimiser; the control is two updates from fresh moments,
    so the moments and the update count the warm-up step left are zeroed with the model restore (the tables are not touched)."""
    from vae_gp_ode_amd import graph
    from vae_gp_ode_amd.graph import GraphedStep
    setting = (False, False, True)
    want = scene.control(setting)
    scene.restore()
    opt = scene.optimiser(setting)
    inner, calls = scene.step_fn(opt), {'n': 0}

    def step():
        calls['n'] += 1
        out = inner()
        if calls['n'] == 2:
            raise _Abort('the step function raised during the capture')
        return out
    with pytest.raises(_Abort):                      # (a)
        GraphedStep(step, warmup=1)
    assert calls['n'] == 2
    torch.cuda.synchronize()
    stale = stale_table_entries(opt)                 # (b)
    assert stale == [], '%d of %d entries of HipAdam._tables map gradient addresses to a table with other content' % (len(stale), len(opt._tables))
    assert len(opt._static_tabs) == 8, 'the failed capture consumed a static table for good: %d of 8 left' % len(opt._static_tabs)
    assert graph.capturing_step() is False
    scene.restore()                                  # (c)
    _reset_adam(opt)
    gs = GraphedStep(scene.step_fn(opt), warmup=1)
    gs()
    torch.cuda.synchronize()
    assert opt.step_dev.tolist() == [2, 0]
    assert stale_table_entries(opt) == []
    scene.assert_equals(want, 'a warm-up step and a replay on an optimiser whose previous capture failed')
    _assert_nothing_carried_over()


def test_a_graphs_gradient_table_survives_the_256_set_clear(scene):
    """A4.  The table a captured update reads is referenced by the optimiser alone; 257 further distinct sets of gradient addresses
    (interleaved eager steps, as far as the table bookkeeping sees them) must not release it."""
    from vae_gp_ode_amd.graph import GraphedStep
    setting = (False, False, True)
    want = scene.control(setting)
    scene.restore()
    opt = scene.optimiser(setting)
    with _Spy() as spy:
        gs = GraphedStep(scene.step_fn(opt), warmup=1, grad_params=opt.params)
    updates = [args for name, args in spy.calls if name == 'gpode_adam_multi']
    assert len(updates) == 2                         # the warm-up step's and the captured one
    addr = updates[-1][1].value                      # the gradient table the captured update was given
    keep = []
    for _ in range(257):
        for p in opt.params:
            keep.append(torch.zeros_like(p))         # all alive: no address repeats
            p.grad = keep[-1]
        opt._refresh_grad_table()
    torch.cuda.synchronize()
    table = owner_of(opt, addr)
    assert table is not None, 'the optimiser no longer owns the gradient table its captured graph reads (released by the 256-set clear)'
    assert table.tolist() == [g.data_ptr() for g in gs.grads], 'the captured graph\'s table no longer holds the addresses of its gradients'
    gs()
    torch.cuda.synchronize()
    assert opt.step_dev.tolist() == [2, 0]
    scene.assert_equals(want, 'a warm-up step and a replay behind 257 other gradient-address sets')


def _nudge_Um(scene):
    with torch.no_grad():
        scene.field.Um.optvar.add_(0.25)


def test_a_leftover_prebuilt_cache_does_not_reach_a_later_step(scene):
    """A5, through the model.  ODEGPVAE.forward prebuilds before every flow it reaches under overlap, so a leftover is overwritten
    there whatever take_prebuilt_cache does: this pins that property.  The callers that reach a flow WITHOUT prebuilding are the
    subject of the next test."""
    setting = (False, True, True)
    want = scene.control(setting, steps=1, prepare=_nudge_Um)
    scene.restore()
    opt = scene.optimiser(setting)
    scene.field.prebuild_cache(None)                 # ... and no flow takes it
    assert getattr(scene.field, '_prebuilt', None) is not None
    _nudge_Um(scene)
    scene.step_fn(opt)()
    scene.assert_equals(want, 'a step behind a prebuilt cache nobody took')
    assert getattr(scene.field, '_prebuilt', None) is None
    _assert_nothing_carried_over()


def test_a_leftover_prebuilt_cache_does_not_reach_a_flow_that_did_not_prebuild(scene):
    """A5, past the model's forward: evaluate.py calls sample_trajectories itself, which never prebuilds.  A cache left by a forward
    pass that raised (older parameters) must not be what that flow integrates."""
    from vae_gp_ode_amd import ops
    z0 = torch.randn(4, 6, device='cuda')
    ops.set_overlap(True)
    with torch.no_grad():
        scene.restore()
        _nudge_Um(scene)
        want = scene.m.sample_trajectories(z0, 4).clone()
        scene.restore()
        scene.field.prebuild_cache(None)             # built from the parameters before the change
        _nudge_Um(scene)
        got = scene.m.sample_trajectories(z0, 4)
        torch.cuda.synchronize()
    assert torch.equal(want, got), 'the flow integrated a cache prebuilt from older parameters (max |difference| %.3e)' % (
        (want - got).abs().max().item())
    ops.join_side_stream()


def test_two_passes_without_zero_grad_both_land_in_the_gradient(scene):
    """Gradient accumulation under overlap: zero_grad drops pending side-stream gradients, two completed passes WITHOUT one between
    them must still both arrive -- Um.grad after two backward passes and one join is the sum of the two passes run apart."""
    from vae_gp_ode_amd import ops, vae_ops
    Um = scene.field.Um.optvar
    scene.restore()
    ops.set_overlap(True)
    vae_ops.set_deferred_reductions(False)
    for p in scene.m.parameters():
        p.grad = None
    apart = []
    for X in (scene.X, scene.X2):
        scene.loss(X).backward()
        assert len(ops._overlap['pending']) == 1, 'the flow\'s backward did not take the side-stream branch: the test is vacuous'
        ops.join_side_stream()
        apart.append(Um.grad.clone())
        for p in scene.m.parameters():
            p.grad = None
    for X in (scene.X, scene.X2):
        scene.loss(X).backward()
    assert len(ops._overlap['pending']) == 2
    ops.join_side_stream()
    torch.cuda.synchronize()
    assert not torch.equal(apart[0], apart[1])
    assert torch.equal(Um.grad, apart[0] + apart[1]), (Um.grad - (apart[0] + apart[1])).abs().max().item()
    _assert_nothing_carried_over()
