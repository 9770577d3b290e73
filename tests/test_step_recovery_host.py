"""Host side of the state a training step carries over to the next one (vae_ops._deferred, HipAdam's gradient-pointer tables,
graph._capture): what the step AFTER one that did not run to its end launches and keeps.  No kernel runs: the recorder and the
stand-ins of test_vae_ops_calls_host take the library's place, and HipAdam is driven on host tensors that answer is_cuda."""
import pytest
import torch

from step_recovery import owner_of, stale_table_entries
from test_vae_ops_calls_host import Recorder, _OnDevice, _bn, _leaf, patched


class _Abort(RuntimeError):
    pass


def _encoder_pass(rec, V, abort):
    """the graph of the ``deferred_encoder`` scenario (conv -> BatchNorm -> linear: three reducing backward calls), built anew and run
    backward; ``abort``: a hook on x raises once its gradient -- the last product of the pass -- exists"""
    x, w, b = _leaf(rec, 'x', 2, 3, 8, 8), _leaf(rec, 'w', 4, 3, 3, 3), _leaf(rec, 'b', 4)
    fw, fb = _leaf(rec, 'fw', 5, 64), _leaf(rec, 'fb', 5)
    y = V.linear(V.batch_norm_train(V.conv2d(x, w, b, 2, 1), _bn(rec, 4), True).flatten(1), fw, fb)
    if abort:
        def hook(g):
            raise _Abort('raised by the test inside the backward pass')
        x.register_hook(hook)
    y.sum().backward()


def test_the_pass_after_an_aborted_backward_flushes_its_own_reductions():
    """B1.  Autograd drops the end-of-backward callbacks of a pass that raises.  The next pass must notice on its own (another graph
    task) that it is a new one: its first reducing call drops the leftovers and queues a flush (gpode_defer_reductions(2)), the later
    ones record (1), and exactly one gpode_flush_reductions ends it.  With a flag instead of the task every call of the second pass
    records (1), nothing is flushed, and ``keep`` holds the scratch buffers of both passes."""
    rec = Recorder()
    with patched(rec, stats_min=2) as V:
        try:
            V.set_deferred_reductions(True)
            with pytest.raises(_Abort):
                _encoder_pass(rec, V, abort=True)
            first = list(rec.lines)
            # the aborted pass recorded its three reductions and never flushed them: the state the next pass has to recover from
            assert sum(l.startswith('gpode_defer_reductions(') and not l.endswith('(0)') for l in first) == 3, first
            assert not any(l.startswith('gpode_flush_reductions') for l in first), first
            assert len(V._deferred['keep']) > 0 and V._deferred['queued'] is True, 'the aborted pass left nothing behind: the test is vacuous'
            _encoder_pass(rec, V, abort=False)
            second = rec.lines[len(first):]
            modes = [l for l in second if l.startswith('gpode_defer_reductions(') and not l.endswith('(0)')]
            assert modes == ['gpode_defer_reductions(2)', 'gpode_defer_reductions(1)', 'gpode_defer_reductions(1)'], \
                'the pass after an aborted one did not start anew (stale _deferred["queued"]): %s' % modes
            flushes = [i for i, l in enumerate(second) if l.startswith('gpode_flush_reductions')]
            assert flushes == [len(second) - 1], 'one flush, as the last call of the pass; got them at %s of %d lines' % (flushes, len(second))
            assert V._deferred['keep'] == [] and V._deferred['queued'] is False, \
                'stale deferred state after a completed pass: keep %d, queued %s' % (len(V._deferred['keep']), V._deferred['queued'])
        finally:
            V.reset_step_state()


def test_reset_step_state_empties_what_an_aborted_pass_left():
    """vae_ops.reset_step_state(): recording mode dropped and closed ((2) then (0)), nothing kept, nothing queued"""
    rec = Recorder()
    with patched(rec, stats_min=2) as V:
        V.set_deferred_reductions(True)
        with pytest.raises(_Abort):
            _encoder_pass(rec, V, abort=True)
        assert V._deferred['keep'] and V._deferred['queued']
        n = len(rec.lines)
        V.reset_step_state()
        assert rec.lines[n:] == ['gpode_defer_reductions(2)', 'gpode_defer_reductions(0)']
        assert V._deferred['keep'] == [] and V._deferred['queued'] is False
        from vae_gp_ode_amd import graph, ops
        assert ops._overlap['pending'] == [] and ops._overlap['kl'] is None and not graph.capturing_step()


# ---- B2: HipAdam's table bookkeeping on host tensors --------------------------------------------------------------------------------------
@pytest.fixture
def host_adam(monkeypatch):
    """A HipAdam over two host parameters that answer is_cuda, and a switch for 'the current stream is capturing'.  Pinned memory
    needs a device: the staging buffers are plain host tensors here (no copy from them is ever made)."""
    from vae_gp_ode_amd import graph, vae_ops
    from vae_gp_ode_amd.optim import HipAdam
    state = {'capturing': False}
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self, *a, **k: self)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: state['capturing'])
    params = [torch.zeros(n).as_subclass(_OnDevice).requires_grad_() for n in (3, 5)]
    opt = HipAdam(params, bucketed=False)
    vae_ops.set_deferred_reductions(False)
    keep = []

    def fresh_grads():
        for p in params:
            keep.append(torch.zeros(p.numel()))      # all kept alive: no address repeats
            p.grad = keep[-1]
        return [p.grad.data_ptr() for p in params]

    def capture(fail):
        """what GraphedStep does around the captured call of the step function"""
        state['capturing'], graph._capture['active'], graph._capture['after'] = True, True, []
        try:
            opt._refresh_grad_table()
            if fail:
                raise _Abort('the step function raised during the capture')
        except BaseException:
            graph.abandon_capture()
            raise
        finally:
            state['capturing'] = False
        graph._capture['active'] = False
        after, graph._capture['after'] = graph._capture['after'], []
        for fn, _ in after:
            fn()
    yield opt, fresh_grads, capture
    graph.abandon_capture()


def test_a_failed_capture_leaves_no_table_entry_and_returns_the_static_table(host_adam):
    """A3(b) on the host: the capture raises, so the upload registered with graph.after_capture never runs -- the entry that mapped the
    capture's gradient addresses to a table of zeros must go, and the static table must be back among the eight."""
    from vae_gp_ode_amd import graph
    opt, fresh_grads, capture = host_adam
    fresh_grads()
    opt._refresh_grad_table()                        # an eager step
    want = fresh_grads()
    with pytest.raises(_Abort):
        capture(fail=True)
    assert stale_table_entries(opt) == [], 'a table entry without its content outlives the failed capture'
    assert tuple(want) not in opt._tables
    assert len(opt._static_tabs) == 8, 'the failed capture kept a static table: %d of 8 left' % len(opt._static_tabs)
    assert not graph.capturing_step() and graph._capture['after'] == []
    capture(fail=False)                              # the same addresses again: a fresh entry, uploaded
    assert opt._tables[tuple(want)][0].tolist() == want and opt._g.tolist() == want
    assert len(opt._static_tabs) == 7


def test_a_captured_graphs_table_survives_the_256_set_clear(host_adam):
    """A4 on the host: the table a capture took is what the graph reads at every replay; 257 further gradient-address sets (the point
    at which the eager entries are dropped) must leave it owned by the optimiser, with its content."""
    opt, fresh_grads, capture = host_adam
    want = fresh_grads()
    capture(fail=False)
    tab = opt._g
    assert tab.tolist() == want
    addr = tab.data_ptr()
    del tab
    opt._g = None
    for _ in range(257):
        fresh_grads()
        opt._refresh_grad_table()
    assert len(opt._tables) < 256, 'the clear never ran: the test is vacuous'
    owned = owner_of(opt, addr)
    assert owned is not None, 'the table of the captured graph was released by the 256-set clear'
    assert owned.tolist() == want
