"""autograd bindings of the conv-VAE HIP kernels (csrc/vae_conv.hip).  Every forward AND backward is a
call into libgpode_hip.so; torch only allocates the tensors and records the graph."""
import ctypes
import os

import torch

from . import _lib, ops
from .ops import _chk, _ptr, _stream


# ---- what rides on tensors and modules --------------------------------------------------------------------------------------------
# Six attributes carry a by-product from the function that has it to the one that would otherwise launch for it.  None is a
# contract with callers; each has one writer and one reader.
#   _gpode_chansum  on an input gradient: its per-channel sums.  Set by every BatchNorm backward (_BatchNormTrain, _BatchNormTrainPair,
#                   _BnReluConvT); taken by the convolution backward that receives the gradient (_fused_chansum) as its bias
#                   gradient.  The taker DELETES it: the sums go on to autograd, which clones a gradient that has a second owner -- a
#                   read, and none may happen before the deferred reductions have run (set_deferred_reductions).
#   _gpode_bnstats  on a convolution output: (module, mean, invstd, table) of the BatchNorm behind it.  Set by _convT_fwd_stats;
#                   read (not deleted: the fallback of bn_relu_conv_transpose2d looks too) by the _BnReluConvT that consumes the
#                   output for that very module.  Lives as long as the activation.
#   _gpode_ll       on the partial sums of sigmoid_loglik_parts: (X, z, route).  Set by _SigmoidLogLikParts.forward; read by
#                   elbo_all(), which decides there whether its backward also produces the logit gradients.  Lives with the sums.
#   _gpode_ga       on the row gradient the ELBO backward returns: the logit gradients it produced in the same launch.  Set in
#                   _elbo_all_bwd; read by _SigmoidLogLikParts.backward, which then launches nothing.  Dies with the row gradient at
#                   the end of that backward; nobody else may keep the row gradient.
#   _gpode_klpart   on the encoder's packed (mu | logvar) rows: the KL partial sums of _ReparamKL.  Set by reparam(); read by
#                   elbo_all().  Replaced by the next reparam() on the same rows; lives with them.
#   _gpode_slot     on an nn.BatchNorm2d: its slot (0..63) in the library's statistics hand-over.  Set once by _stats_slot; never
#                   deleted.
# A new by-product follows _fused_chansum: hand the tensor over with no second owner before the deferred reductions have run.


def _new(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _bchw(x):
    """(images, channels, elements per channel image) of x (B,C,...)"""
    return x.shape[0], x.shape[1], x[0, 0].numel()


def _convT_out(Hi, Wi, K, stride, pad, out_pad):
    """output size of a transposed convolution"""
    return (Hi - 1) * stride - 2 * pad + K + out_pad, (Wi - 1) * stride - 2 * pad + K + out_pad


def _scratch(n, like):
    return torch.empty(max(int(n), 4), dtype=torch.float32, device=like.device)


def _wgrad_scratch(B, Ci, Co, K, like):
    return _scratch(_lib.load().gpode_conv_wgrad_scratch(B, Ci, Co, K), like)


def _bn_scratch(B, C, like):
    return _scratch(_lib.load().gpode_bn_scratch(B, C), like)


# ---- deferred final reductions (include/gpode.h: gpode_defer_reductions / gpode_flush_reductions) --------------------------------
# set_deferred_reductions(True): the weight / bias gradients and BatchNorm channel sums produced by the backward functions below
# become valid at the END of the backward pass -- ONE launch reduces all their workgroup partials (from autograd's end-of-backward
# callback) instead of one few-microsecond launch per function (14 per step of a first-order model: graph nodes on the critical
# chain).  Sound only when nothing reads those tensors earlier, and autograd does read in two cases: it CLONES an incoming
# gradient that has a second owner, and it ADDS to ``p.grad`` when that exists.  Hence: on only with an optimiser that drops the
# gradients in zero_grad and takes over the tensors autograd hands it (optim.HipAdam(bucketed=False | 'gather'):
# ``allows_deferred_reductions``): creating a HipAdam sets the switch for its kind (the optimiser in charge of the step decides);
# the default, and the setting for any other consumer of ``.grad``, is off.  configs[0]: 14 reduction launches -> 1.
# The bookkeeping of a pass is keyed on autograd's graph task: a pass that raises never runs its end-of-backward callback (autograd drops
# the callbacks it had queued), so ``queued`` alone would stay set for good and no later pass would flush.  A reducing call under another
# task than the stored one therefore starts a new pass, whatever the last one left behind.
_deferred = {'on': False, 'keep': [], 'queued': False, 'task': -1}
_DEFER_ALLOWED = os.environ.get('GPODE_EAGER_REDUCTIONS', '0') != '1'


def set_deferred_reductions(on):
    _deferred['on'] = bool(on) and _DEFER_ALLOWED


def _flush_deferred(task):
    if task != _deferred['task']:                    # the callback of a pass that is no longer the current one: nothing of it is recorded
        return
    _deferred['queued'], _deferred['task'] = False, -1
    try:
        _lib.call('gpode_flush_reductions', _stream())
    finally:
        _deferred['keep'].clear()


def _bwd_call(name, *args, keep=()):
    """A backward-pass entry point whose last step is a reduction of workgroup partials (``keep``: its scratch buffers)."""
    task = torch._C._current_graph_task_id() if _deferred['on'] else -1
    if task < 0:
        return _lib.call(name, *args)
    lib = _lib.load()
    if not _deferred['queued'] or task != _deferred['task']:
        lib.gpode_defer_reductions(2)                # drop leftovers of an aborted pass, then record
        _deferred['keep'].clear()                    # ... and its scratch buffers: the jobs that read them are gone
        torch.autograd.Variable._execution_engine.queue_callback(lambda t=task: _flush_deferred(t))
        _deferred['queued'], _deferred['task'] = True, task
    else:
        lib.gpode_defer_reductions(1)
    try:
        _lib.call(name, *args)
    finally:
        lib.gpode_defer_reductions(0)
    _deferred['keep'].extend(keep)


def reset_step_state():
    """Put everything a training step carries over to the next one back to its start: the deferred reductions (recorded jobs, their
    scratch buffers, the library's recording mode), the side-stream gradients a pass left for the optimiser (ops.drop_pending_grads) and
    the registrations of a GraphedStep capture.  A step that ran to its end leaves all of these empty, and a step that did not is
    recovered from by the next one on its own (the graph task above, HipAdam.zero_grad, GraphedStep); this is the explicit form, for a
    caller that gives up on a step and wants nothing of it kept alive."""
    from . import graph
    lib = _lib.load()
    lib.gpode_defer_reductions(2)
    lib.gpode_defer_reductions(0)
    _deferred['keep'].clear()
    _deferred['queued'], _deferred['task'] = False, -1
    ops.drop_pending_grads()
    graph.abandon_capture()


_bn_sync = None        # parallel.BatchNormSync while data-parallel training normalises with global-minibatch statistics


def set_bn_sync(group):
    """group: parallel.BatchNormSync (or None = per-process statistics, the single-GPU path)."""
    global _bn_sync
    _bn_sync = group


# The cross-rank BatchNorm in its halves: what a rank computes before the all-gather and what it does with the gathered rows.
# _bn_global_stats / _bn_global_bwd put one gather between them; _BatchNormTrainPair puts ONE between the halves of two layers.
def _bn_moments(x):
    """the local moments of x, (2C + 1,): what the ranks exchange in the forward pass"""
    B, C, HW = _bchw(x)
    mom = _new((2 * C + 1,), x)
    _lib.call('gpode_bn_moments', _ptr(x), _ptr(mom), B, C, HW, _ptr(_bn_scratch(B, C, x)), _stream())
    return mom


def _bn_finalize(gathered, x, gamma, beta, running_mean, running_var, nbt, momentum, eps):
    """rank-ordered combination of the gathered moments.  Returns (mean, invstd, table[C][4])."""
    C = x.shape[1]
    mean, invstd, table = _new((C,), x), _new((C,), x), _new((C, 4), x)
    _lib.call('gpode_bn_finalize', _ptr(gathered), _bn_sync.world, _ptr(_chk(gamma, 'gamma')), _ptr(_chk(beta, 'beta')), _ptr(mean),
              _ptr(invstd), _ptr(running_mean), _ptr(running_var), _ptr(nbt), ctypes.c_float(momentum), ctypes.c_float(eps), _ptr(table), C,
              _stream())
    return mean, invstd, table


def _bn_apply(x, table, relu):
    B, C, HW = _bchw(x)
    y = _new(x.shape, x)
    _lib.call('gpode_bn_apply', _ptr(x), _ptr(table), _ptr(y), B, C, HW, int(relu), _stream())
    return y


def _bn_global_stats(x, gamma, beta, running_mean, running_var, nbt, momentum, eps):
    """Forward half of the cross-rank BatchNorm: local moments -> all-gather -> rank-ordered combination."""
    return _bn_finalize(_bn_sync.gather(_bn_moments(x)), x, gamma, beta, running_mean, running_var, nbt, momentum, eps)


def _bn_bwd_sums(x, gy, gamma, beta, mean, invstd, relu):
    """the local sums of the backward pass, (2C,): what the ranks exchange.  Returns (sums, gy as the kernels read it, scratch)."""
    B, C, HW = _bchw(x)
    scratch, sums, gy = _bn_scratch(B, C, x), _new((2 * C,), x), gy.contiguous()
    _lib.call('gpode_bn_bwd_sums', _ptr(x), _ptr(gy), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), _ptr(sums), B, C, HW, int(relu),
              _ptr(scratch), _stream())
    return sums, gy, scratch


def _bn_bwd_apply(sync, gathered, scratch, x, gy, gamma, beta, mean, invstd, relu):
    """gx with the global centring terms from the gathered sums.  Returns (gx, ggamma, gbeta, chansum)."""
    B, C, HW = _bchw(x)
    gx, gg, gb, cs = _new(x.shape, x), _new((C,), x), _new((C,), x), _new((C,), x)
    _bwd_call('gpode_bn_bwd_apply', _ptr(x), _ptr(gy), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), _ptr(gathered),
              _ptr(sync.weights(x.device)), sync.world, ctypes.c_float(sync.count_all(B * HW)), _ptr(gx), _ptr(gg), _ptr(gb), _ptr(cs),
              B, C, HW, int(relu), _ptr(scratch), _stream(), keep=(scratch,))
    return gx, gg, gb, cs


def _bn_global_bwd(sync, x, gy, gamma, beta, mean, invstd, relu):
    """Backward half: local sums -> all-gather -> gx with the global centring terms."""
    sums, gy, scratch = _bn_bwd_sums(x, gy, gamma, beta, mean, invstd, relu)
    return _bn_bwd_apply(sync, sync.gather(sums), scratch, x, gy, gamma, beta, mean, invstd, relu)


def _bn_bwd(sync, x, gy, gamma, beta, mean, invstd, relu):
    """BatchNorm (+ ReLU) backward on the statistics of this process (``sync`` None) or of all ranks: (gx, ggamma, gbeta, chansum)."""
    if sync is not None:
        return _bn_global_bwd(sync, x, gy, gamma, beta, mean, invstd, relu)
    B, C, HW = _bchw(x)
    gx, gg, gb, cs = _new(x.shape, x), _new((C,), x), _new((C,), x), _new((C,), x)
    bs = _bn_scratch(B, C, x)
    _bwd_call('gpode_bn_bwd', _ptr(x), _ptr(gy.contiguous()), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), _ptr(gx), _ptr(gg),
              _ptr(gb), _ptr(cs), B, C, HW, relu, _ptr(bs), _stream(), keep=(bs,))
    return gx, gg, gb, cs


# -- two independent BatchNorm layers of the same depth (the position and the velocity encoder of a second-order model, vae.py:14-19)
# with ONE all-gather per direction instead of two: on N ranks every collective of a step is a latency-bound exchange of a few
# hundred bytes, so their number is what counts (parallel.BatchNormSync.gather_many; switch: set_pack_bn_gathers) ---------------
_pack_bn = {'on': os.environ.get('GPODE_PACK_BN_GATHERS', '0') == '1'}


def set_pack_bn_gathers(on):
    _pack_bn['on'] = bool(on)


def pack_bn_gathers():
    return _pack_bn['on'] and _bn_sync is not None


class _BatchNormTrainPair(torch.autograd.Function):
    """(BatchNorm2d_train + ReLU)(x1), (BatchNorm2d_train + ReLU)(x2) under cross-rank statistics, the two layers' moments (forward)
    and backward sums (backward) exchanged in one packed all-gather each.  Same kernels, same rank order of every combination as two
    _BatchNormTrain calls: results are bit-identical to the unpacked form."""

    @staticmethod
    def forward(ctx, x1, g1, b1, rm1, rv1, nbt1, x2, g2, b2, rm2, rv2, nbt2, momentum, eps, relu):
        xs = (_chk(x1, 'x1'), _chk(x2, 'x2'))
        gathered = _bn_sync.gather_many([_bn_moments(x) for x in xs])
        ys, saved = [], []
        for x, gam, bet, rm, rv, nbt, got in zip(xs, (g1, g2), (b1, b2), (rm1, rm2), (rv1, rv2), (nbt1, nbt2), gathered):
            mean, invstd, table = _bn_finalize(got, x, gam, bet, rm, rv, nbt, momentum, eps)
            ys.append(_bn_apply(x, table, relu))
            saved += [x, gam, bet, mean, invstd]
        ctx.save_for_backward(*saved)
        ctx.sync, ctx.relu = _bn_sync, int(relu)
        return ys[0], ys[1]

    @staticmethod
    def backward(ctx, gy1, gy2):
        sv, sync = ctx.saved_tensors, ctx.sync
        # per layer (x, gy, gamma, beta, mean, invstd, relu), as the halves take them; both sums, one gather, both applies
        layers = [(x, gy, *rest, ctx.relu) for (x, *rest), gy in zip((sv[:5], sv[5:]), (gy1, gy2))]
        sums = [_bn_bwd_sums(*layer) for layer in layers]
        gathered = sync.gather_many([s for s, _, _ in sums])
        out = []
        for (x, _, *rest), (_, gy, scratch), got in zip(layers, sums, gathered):
            gx, gg, gb, cs = _bn_bwd_apply(sync, got, scratch, x, gy, *rest)
            gx._gpode_chansum = cs
            out += [gx, gg, gb, None, None, None]
        return (*out, None, None, None)


def batch_norm_train_pair(x1, bn1, x2, bn2, relu):
    """Two training-mode BatchNorm2d modules on their own inputs with packed cross-rank exchanges (see _BatchNormTrainPair)."""
    return _BatchNormTrainPair.apply(x1, bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var, bn1.num_batches_tracked,
                                     x2, bn2.weight, bn2.bias, bn2.running_mean, bn2.running_var, bn2.num_batches_tracked,
                                     bn1.momentum, bn1.eps, relu)


_dec10_fused = os.environ.get('GPODE_DEC10_BN_UNFUSED', '0') != '1'


def _dec10_bn_bwd(sync, c, gy, w, gamma, beta, mean, invstd, gw=None, gbias=None):
    """decnn.10's input gradient + the BatchNorm/ReLU backward in front of it in two passes over c (include/gpode.h,
    gpode_dec10_bn_bwd_*): (gc, ggamma, gbeta, channel sums of gc).  ``gw`` (a tensor to fill): the layer's weight gradient rides
    in the first pass (gpode_dec10_bn_bwd_sums_wgrad)."""
    B = c.shape[0]
    scratch = _scratch(_lib.load().gpode_dec10_bn_scratch_floats(), c)
    gc, gg, gb, cs = _new(c.shape, c), _new((16,), c), _new((16,), c), _new((16,), c)
    head = (_ptr(c), _ptr(gy), _ptr(w), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd))
    sums = _new((32,), c) if sync is not None else None
    if gw is not None:
        ws = _scratch(_lib.load().gpode_dec10_bn_wgrad_scratch_floats(), c)
        _bwd_call('gpode_dec10_bn_bwd_sums_wgrad', *head, _ptr(sums), _ptr(gw), _ptr(gbias), B, _ptr(scratch), _ptr(ws), _stream(),
                  keep=(ws, scratch))
    else:
        _lib.call('gpode_dec10_bn_bwd_sums', *head, _ptr(sums), B, _ptr(scratch), _stream())
    if sync is None:
        _bwd_call('gpode_dec10_bn_bwd_apply', *head, _ptr(None), _ptr(None), 0, ctypes.c_float(0.0), _ptr(gc), _ptr(gg), _ptr(gb), _ptr(cs),
                  B, _ptr(scratch), _stream(), keep=(scratch,))
    else:
        gathered = sync.gather(sums)
        _bwd_call('gpode_dec10_bn_bwd_apply', *head, _ptr(gathered), _ptr(sync.weights(c.device)), sync.world,
                  ctypes.c_float(sync.count_all(B * 784)), _ptr(gc), _ptr(gg), _ptr(gb), _ptr(cs), B, _ptr(scratch), _stream(), keep=(scratch,))
    return gc, gg, gb, cs


fused_bias_grads = 0   # how many bias gradients arrived ready-made from a BatchNorm backward (see _BatchNormTrain.backward)


def _fused_chansum(gy, C):
    global fused_bias_grads
    cs = getattr(gy, '_gpode_chansum', None)
    if cs is None or tuple(cs.shape) != (C,):
        return None
    # hand the tensor over with no second owner: autograd takes a gradient as it is only when nothing else refers to it, and clones
    # it otherwise -- a read, which must not happen before the deferred reductions have run (set_deferred_reductions)
    del gy._gpode_chansum
    fused_bias_grads += 1
    return cs


def _batch_strided(x):
    """x (B,C,H,W) with dense images at a constant distance (e.g. X[:, 0] of a minibatch X (N,T,1,28,28), odegpvae.py:55-63) and a
    channel count the generic convolution kernels take: floats between images, else 0."""
    if x.dim() != 4 or x.is_contiguous() or x.dtype != torch.float32 or not x.is_cuda or x.shape[1] % 4 == 0 or x.shape[0] < 2:
        return 0
    B, C, H, W = x.shape
    if x.stride()[1:] != (H * W, W, 1) or x.stride(0) < C * H * W:
        return 0
    return x.stride(0)


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pad):
        xbs = _batch_strided(x)                      # read in place: no contiguous copy of the slice (a launch on the step's first chain)
        if not xbs:
            x = _chk(x, 'x')
        w = _chk(w, 'weight')
        B, Ci, H, W = x.shape
        Co, _, K, _ = w.shape
        Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
        y = _new((B, Co, Ho, Wo), x)
        if xbs:
            _lib.call('gpode_conv2d_fwd_bs', _ptr(x), xbs, _ptr(w), _ptr(b), _ptr(y), B, Ci, H, W, Co, K, stride, pad, Ho, Wo, _stream())
        else:
            _lib.call('gpode_conv2d_fwd', _ptr(x), _ptr(w), _ptr(b), _ptr(y), B, Ci, H, W, Co, K, stride, pad, Ho, Wo, _stream())
        ctx.save_for_backward(x, w)
        ctx.geom = (B, Ci, H, W, Co, K, stride, pad, Ho, Wo, b is not None)
        ctx.xbs = xbs
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        B, Ci, H, W, Co, K, S, P, Ho, Wo, has_b = ctx.geom
        gy = gy.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _new(x.shape, x)
            _lib.call('gpode_conv2d_bwd_data', _ptr(gy), _ptr(w), _ptr(None), _ptr(gx), B, Ci, H, W, Co, K, S, P, Ho, Wo, _stream())
        if ctx.needs_input_grad[1]:
            gw = _new(w.shape, x)
            pre = _fused_chansum(gy, Co) if has_b else None     # bias gradient already produced by the BatchNorm backward
            gb = _new((Co,), x) if (has_b and pre is None) else None
            ws = _wgrad_scratch(B, Ci, Co, K, x)
            if ctx.xbs:
                _bwd_call('gpode_conv2d_bwd_weight_bs', _ptr(x), ctx.xbs, _ptr(gy), _ptr(gw), _ptr(gb), _ptr(ws),
                          B, Ci, H, W, Co, K, S, P, Ho, Wo, _stream(), keep=(ws, gy))
            else:
                _bwd_call('gpode_conv2d_bwd_weight', _ptr(x), _ptr(gy), _ptr(gw), _ptr(gb), _ptr(ws),
                          B, Ci, H, W, Co, K, S, P, Ho, Wo, _stream(), keep=(ws, gy))
            if pre is not None:
                gb = pre
        return gx, gw, gb, None, None


# ---- BatchNorm statistics produced by the convolution in front of it (include/gpode.h: gpode_convT_fwd_stats) ----------------------
# The decoder's transposed convolutions decnn.1/4/7 are each followed by a BatchNorm2d in training mode (vae.py:107-120).  When the
# caller names that module (``stats_for``), the convolution sums the statistics of its output while storing it and its last workgroup
# finalises them: the output tensor then carries (mean, invstd, table) as ``_gpode_bnstats`` and the consuming _BnReluConvT takes them
# instead of launching the statistics pass + table kernel (two graph nodes and one read of the tensor per layer).
_STATS_GEOMS = {(32, 64, 3, 1, 0, 4), (64, 32, 5, 2, 1, 6), (32, 16, 5, 2, 1, 13)}      # (Cin, Cout, K, stride, pad, Hi) of decnn.1/4/7
_fused_stats = os.environ.get('GPODE_BN_STATS_PASS', '0') != '1'
_FUSED_STATS_MIN_IMAGES = int(os.environ.get('GPODE_BN_STATS_FUSED_MIN', '512'))
_slots = {'next': 0}


def _stats_slot(bn):
    s = getattr(bn, '_gpode_slot', None)
    if s is None:
        s = bn._gpode_slot = _slots['next'] % 64
        _slots['next'] += 1
    return s


def _can_fuse_stats(bn, x, Cin, Cout, K, stride, pad, Hi):
    # from 512 images on: below that the statistics pass is a few microseconds and the per-workgroup hand-over at the end of the
    # convolution costs as much.  configs[0] (512 images): 0.722 vs 0.724 ms per step fused vs separate -- even, with five graph nodes
    # less; configs[1] (4096): 2.62 vs 2.66.  (With four loads in flight in the last workgroup's combine, round 3's first version, the
    # break-even was at 1024 images: bn_sink.hpp.)
    return (_fused_stats and bn is not None and bn.training and _bn_sync is None and (Cin, Cout, K, stride, pad, Hi) in _STATS_GEOMS
            and x.shape[0] >= _FUSED_STATS_MIN_IMAGES and x.data_ptr() % 16 == 0 and os.environ.get('GPODE_CONV_VALU', '0') != '1')


def _convT_fwd_stats(x, table_in, w, b, y, geom, bn):
    """y = convT(x [after BatchNorm + ReLU by table_in], w) + b and the statistics of y for the BatchNorm module ``bn`` behind it."""
    B, Cout, Ht, Wt, Cin, K, stride, pad, Hi, Wi = geom
    mean, invstd, table = _new((Cout,), x), _new((Cout,), x), _new((Cout, 4), x)
    scratch = _scratch(_lib.load().gpode_convT_fwd_stats_scratch(Cout), x)
    _lib.call('gpode_convT_fwd_stats', _ptr(x), _ptr(table_in), _ptr(w), _ptr(b), _ptr(y), B, Cout, Ht, Wt, Cin, K, stride, pad, Hi, Wi,
              _ptr(_chk(bn.weight, 'gamma')), _ptr(_chk(bn.bias, 'beta')), _ptr(mean), _ptr(invstd), _ptr(bn.running_mean),
              _ptr(bn.running_var), _ptr(bn.num_batches_tracked), ctypes.c_float(bn.momentum), ctypes.c_float(bn.eps), _ptr(table),
              _ptr(scratch), _stats_slot(bn), _stream())
    y._gpode_bnstats = (bn, mean, invstd, table)


class _ConvT2d(torch.autograd.Function):
    """nn.ConvTranspose2d as the adjoint of the convolution that shares its weight buffer."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad, out_pad, stats_for=None):
        x, w = _chk(x, 'x'), _chk(w, 'weight')
        B, Cin, Hi, Wi = x.shape
        _, Cout, K, _ = w.shape
        Ht, Wt = _convT_out(Hi, Wi, K, stride, pad, out_pad)
        y = _new((B, Cout, Ht, Wt), x)
        # conv geometry: "input" (B,Ci=Cout,H=Ht,W=Wt), "output" (B,Co=Cin,Ho=Hi,Wo=Wi)
        if _can_fuse_stats(stats_for, x, Cin, Cout, K, stride, pad, Hi):
            _convT_fwd_stats(x, None, w, b, y, (B, Cout, Ht, Wt, Cin, K, stride, pad, Hi, Wi), stats_for)
        else:
            _lib.call('gpode_conv2d_bwd_data', _ptr(x), _ptr(w), _ptr(b), _ptr(y), B, Cout, Ht, Wt, Cin, K, stride, pad, Hi, Wi, _stream())
        ctx.save_for_backward(x, w)
        ctx.geom = (B, Cout, Ht, Wt, Cin, K, stride, pad, Hi, Wi, b is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        B, Cout, Ht, Wt, Cin, K, S, P, Hi, Wi, has_b = ctx.geom
        gy = gy.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _new(x.shape, x)
            _lib.call('gpode_conv2d_fwd', _ptr(gy), _ptr(w), _ptr(None), _ptr(gx), B, Cout, Ht, Wt, Cin, K, S, P, Hi, Wi, _stream())
        if ctx.needs_input_grad[1]:
            gw = _new(w.shape, x)
            ws = _wgrad_scratch(B, Cout, Cin, K, x)
            _bwd_call('gpode_conv2d_bwd_weight', _ptr(gy), _ptr(x), _ptr(gw), _ptr(None), _ptr(ws),
                      B, Cout, Ht, Wt, Cin, K, S, P, Hi, Wi, _stream(), keep=(ws,))
            if has_b:
                gb = _fused_chansum(gy, Cout)
                if gb is None:
                    gb, bs = _new((Cout,), x), _bn_scratch(B, Cout, x)
                    _bwd_call('gpode_chan_sum', _ptr(gy), _ptr(gb), B, Cout, Ht * Wt, _ptr(bs), _stream(), keep=(bs,))
        return gx, gw, gb, None, None, None, None


class _BnReluConvT(torch.autograd.Function):
    """ConvTranspose2d(ReLU(BatchNorm2d_train(c))) (vae.py:113-120, one decoder stage) with the normalised activation never
    written to memory: forward = batch statistics of c (one read) + the transposed convolution applying normalise / affine /
    ReLU while it stages its input; backward = weight gradient (same staging), input gradient of the convolution, then the
    BatchNorm backward on c.  Training mode only; the eval-mode path keeps the separate ops."""

    @staticmethod
    def forward(ctx, c, gamma, beta, running_mean, running_var, nbt, momentum, eps, w, b, stride, pad, out_pad, bn=None, stats_for=None):
        pre = getattr(c, '_gpode_bnstats', None)     # the convolution that produced c summed its statistics for module ``bn`` already
        c, w = _chk(c, 'c'), _chk(w, 'weight')
        B, Cin, Hi, Wi = c.shape
        _, Cout, K, _ = w.shape
        Ht, Wt = _convT_out(Hi, Wi, K, stride, pad, out_pad)
        ctx.sync = _bn_sync
        if pre is not None and pre[0] is bn and bn is not None and _bn_sync is None:
            _, mean, invstd, table = pre
        elif _bn_sync is not None:
            mean, invstd, table = _bn_global_stats(c, gamma, beta, running_mean, running_var, nbt, momentum, eps)
        else:
            mean, invstd, table = _new((Cin,), c), _new((Cin,), c), _new((Cin, 4), c)
            _lib.call('gpode_bn_stats', _ptr(c), _ptr(_chk(gamma, 'gamma')), _ptr(_chk(beta, 'beta')), _ptr(mean), _ptr(invstd),
                      _ptr(running_mean), _ptr(running_var), _ptr(nbt), ctypes.c_float(momentum), ctypes.c_float(eps), _ptr(table),
                      B, Cin, Hi * Wi, _ptr(_bn_scratch(B, Cin, c)), _stream())
        y = _new((B, Cout, Ht, Wt), c)
        if _can_fuse_stats(stats_for, c, Cin, Cout, K, stride, pad, Hi):
            _convT_fwd_stats(c, table, w, b, y, (B, Cout, Ht, Wt, Cin, K, stride, pad, Hi, Wi), stats_for)
        else:
            _lib.call('gpode_conv2d_bwd_data_bn', _ptr(c), _ptr(table), _ptr(w), _ptr(b), _ptr(y), B, Cout, Ht, Wt, Cin, K, stride, pad, Hi, Wi,
                      _stream())
        ctx.save_for_backward(c, gamma, beta, mean, invstd, table, w)
        ctx.geom = (B, Cout, Ht, Wt, Cin, K, stride, pad, Hi, Wi, b is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        c, gamma, beta, mean, invstd, table, w = ctx.saved_tensors
        B, Cout, Ht, Wt, Cin, K, S, P, Hi, Wi, has_b = ctx.geom
        gy = gy.contiguous()
        gw = gb = None
        last_stage = _dec10_fused and (Cout, Cin, K, S, P, Hi, Wi, Ht, Wt) == (1, 16, 5, 1, 2, 28, 28, 28, 28)
        # the last stage's weight gradient rides in its BatchNorm sums pass below, and a bias gradient nobody has summed yet with it
        gw_rides = last_stage and ctx.needs_input_grad[8] and c.data_ptr() % 16 == 0
        if ctx.needs_input_grad[8]:
            gw = _new(w.shape, c)
            if not gw_rides:
                ws = _wgrad_scratch(B, Cout, Cin, K, c)
                _bwd_call('gpode_conv2d_bwd_weight_bn', _ptr(gy), _ptr(c), _ptr(table), _ptr(gw), _ptr(None),
                          _ptr(ws), B, Cout, Ht, Wt, Cin, K, S, P, Hi, Wi, _stream(), keep=(ws,))
            gb = _fused_chansum(gy, Cout) if has_b else None
        to_sum = has_b and gw is not None and gb is None
        if to_sum:
            gb = _new((Cout,), c)
            if not gw_rides:
                bs = _bn_scratch(B, Cout, c)
                _bwd_call('gpode_chan_sum', _ptr(gy), _ptr(gb), B, Cout, Ht * Wt, _ptr(bs), _stream(), keep=(bs,))
        gb_rides = gb if (to_sum and gw_rides) else None
        if last_stage:
            # the decoder's last stage: the gradient w.r.t. the normalised activation is recomputed inside both BatchNorm passes
            gc, gg, gbeta, cs = _dec10_bn_bwd(ctx.sync, c, gy, w, gamma, beta, mean, invstd, gw=gw if gw_rides else None, gbias=gb_rides)
        else:
            # gradient w.r.t. the (never materialised) normalised activation, then through the BatchNorm to c
            ga = _new(c.shape, c)
            _lib.call('gpode_conv2d_fwd', _ptr(gy), _ptr(w), _ptr(None), _ptr(ga), B, Cout, Ht, Wt, Cin, K, S, P, Hi, Wi, _stream())
            gc, gg, gbeta, cs = _bn_bwd(ctx.sync, c, ga, gamma, beta, mean, invstd, 1)
        gc._gpode_chansum = cs
        return gc, gg, gbeta, None, None, None, None, None, gw, gb, None, None, None, None, None


class _BatchNormTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, relu, nbt=None):
        x = _chk(x, 'x')
        B, C, HW = _bchw(x)
        if nbt is not None and not (nbt.is_cuda and nbt.dtype == torch.int64):
            raise _lib.GpodeError('num_batches_tracked must be an int64 CUDA/HIP scalar')
        ctx.sync = _bn_sync
        if _bn_sync is not None:
            mean, invstd, table = _bn_global_stats(x, gamma, beta, running_mean, running_var, nbt, momentum, eps)
            y = _bn_apply(x, table, relu)
        else:
            y, mean, invstd = _new(x.shape, x), _new((C,), x), _new((C,), x)
            _lib.call('gpode_bn_fwd', _ptr(x), _ptr(_chk(gamma, 'gamma')), _ptr(_chk(beta, 'beta')), _ptr(y), _ptr(mean), _ptr(invstd),
                      _ptr(running_mean), _ptr(running_var), _ptr(nbt), ctypes.c_float(momentum), ctypes.c_float(eps), B, C, HW, int(relu),
                      _ptr(_bn_scratch(B, C, x)), _stream())
        ctx.save_for_backward(x, gamma, beta, mean, invstd)
        ctx.relu = int(relu)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, beta, mean, invstd = ctx.saved_tensors
        gx, gg, gb, cs = _bn_bwd(ctx.sync, x, gy, gamma, beta, mean, invstd, ctx.relu)
        # the channel sums of gx ride along with it: the convolution that produced x needs exactly these as its bias gradient
        gx._gpode_chansum = cs
        return gx, gg, gb, None, None, None, None, None, None


class _BatchNormEval(torch.autograd.Function):
    """nn.BatchNorm2d under module.eval(): running statistics, gradient w.r.t. the input only."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, relu):
        x = _chk(x, 'x')
        B, C, HW = _bchw(x)
        y = _new(x.shape, x)
        _lib.call('gpode_bn_eval', _ptr(x), _ptr(None), _ptr(_chk(gamma, 'gamma')), _ptr(_chk(beta, 'beta')), _ptr(running_mean),
                  _ptr(running_var), ctypes.c_float(eps), _ptr(y), B, C, HW, int(relu), _stream())
        ctx.save_for_backward(x, gamma, beta, running_mean, running_var)
        ctx.eps, ctx.relu = eps, int(relu)
        return y

    @staticmethod
    def backward(ctx, gy):
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise _lib.GpodeError('eval-mode BatchNorm is built for frozen layers (main.py:160-161 sets requires_grad=False)')
        x, gamma, beta, rm, rv = ctx.saved_tensors
        B, C, HW = _bchw(x)
        gx = _new(x.shape, x)
        _lib.call('gpode_bn_eval', _ptr(x), _ptr(gy.contiguous()), _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), ctypes.c_float(ctx.eps),
                  _ptr(gx), B, C, HW, ctx.relu, _stream())
        return gx, None, None, None, None, None, None


class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mode):
        x = _chk(x, 'x')
        y = _new(x.shape, x)
        _lib.call('gpode_act_fwd', _ptr(x), _ptr(y), x.numel(), mode, _stream())
        ctx.save_for_backward(y)
        ctx.mode = mode
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gx = _new(y.shape, y)
        _lib.call('gpode_act_bwd', _ptr(y), _ptr(gy.contiguous()), _ptr(gx), y.numel(), ctx.mode, _stream())
        return gx, None


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        x, w = _chk(x, 'x'), _chk(w, 'weight')
        B, In = x.shape
        Out = w.shape[0]
        y = _new((B, Out), x)
        _lib.call('gpode_linear_fwd', _ptr(x), _ptr(w), _ptr(b), _ptr(y), B, In, Out, _stream())
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        B, In = x.shape
        Out = w.shape[0]
        gx = _new(x.shape, x) if ctx.needs_input_grad[0] else None
        gw = _new(w.shape, x) if ctx.needs_input_grad[1] else None
        gb = _new((Out,), x) if (ctx.has_b and gw is not None) else None
        ws = _scratch(_lib.load().gpode_linear_bwd_scratch(B, In, Out), x) if (gw is not None and B >= 1024 and In <= 8) else None
        _bwd_call('gpode_linear_bwd', _ptr(x), _ptr(w), _ptr(gy.contiguous()), _ptr(gx), _ptr(gw), _ptr(gb), B, In, Out, _ptr(ws), _stream(),
                  keep=(ws,) if ws is not None else ())
        return gx, gw, gb


class _LinearReluIn(torch.autograd.Function):
    """linear(relu(x), w, b) with the ReLU folded into the layer's loads in both directions (gpode_linear_relu_fwd / _bwd): the
    encoder's Conv2d -> ReLU -> Flatten -> Linear (vae.py:58-61, 72-74) without the activation tensor and its two launches."""

    @staticmethod
    def forward(ctx, x, w, b):
        x, w = _chk(x, 'x'), _chk(w, 'weight')
        B, In = x.shape
        Out = w.shape[0]
        y = _new((B, Out), x)
        _lib.call('gpode_linear_relu_fwd', _ptr(x), _ptr(w), _ptr(b), _ptr(y), B, In, Out, _stream())
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        B, In = x.shape
        Out = w.shape[0]
        gx = _new(x.shape, x) if ctx.needs_input_grad[0] else None
        gw = _new(w.shape, x) if ctx.needs_input_grad[1] else None
        gb = _new((Out,), x) if (ctx.has_b and gw is not None) else None
        _lib.call('gpode_linear_relu_bwd', _ptr(x), _ptr(w), _ptr(gy.contiguous()), _ptr(gx), _ptr(gw), _ptr(gb), B, In, Out, _stream())
        return gx, gw, gb


class _LogLik(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, z):
        X, z = _chk(X, 'X'), _chk(z, 'z')
        ll = _new(z.shape, z)
        _lib.call('gpode_loglik_fwd', _ptr(X), _ptr(z), _ptr(ll), z.numel(), X.numel(), _stream())
        ctx.save_for_backward(X, z)
        return ll

    @staticmethod
    def backward(ctx, g):
        X, z = ctx.saved_tensors
        gz = _new(z.shape, z)
        _lib.call('gpode_loglik_bwd', _ptr(X), _ptr(z), _ptr(g.contiguous()), _ptr(gz), z.numel(), X.numel(), _stream())
        return None, gz


def _chk_n_obs(n_obs, X, who):
    """The frame counts of a ragged minibatch X (N,T,...): (N,) int32 on X's device.  Shape, dtype and device only -- the values are
    never read back (a captured step stays capturable); the kernels clamp them to [0, T].  -> (n_obs, T, elements per frame)."""
    if not (torch.is_tensor(n_obs) and n_obs.dtype == torch.int32 and n_obs.device == X.device):
        raise _lib.GpodeError('%s: n_obs must be an int32 tensor on the device of X' % who)
    if X.dim() < 2 or tuple(n_obs.shape) != (X.shape[0],):
        raise _lib.GpodeError('%s: n_obs must be (N,) = (%d,), one frame count per sequence of X (N,T,...); got %s'
                              % (who, X.shape[0] if X.dim() else 0, tuple(n_obs.shape)))
    T = int(X.shape[1])
    return n_obs.contiguous(), T, X.numel() // (X.shape[0] * T)


# ---- which frames of X (N,T,...) the loss stage scores: a route object per call -----------------------------------------------------
# The library has one templated kernel per operation and an entry point per route (include/gpode.h: gpode_sigmoid_loglik_fwd, _fwd_len,
# _fwd_pk, ...); a route says which, and with which arguments, so that every wrapper below is written once.  A route has
#   suffix        of the entry points ('', '_len', '_pk');
#   fused         whether the ELBO backward has a form that also produces the logit gradients on this route (elbo_all);
#   bind(X, elements, rows, who)   its argument checks, run by the Function once X has passed _chk; -> the row length the partial sums
#                 are split for (gpode_sigmoid_loglik_splits);
#   fwd_dims / bwd_dims(X, rows, inner)   the header's arguments behind the four tensor pointers, up to and including nX;
#   tail          the header's arguments in front of the stream (also of the fused ELBO backward);
#   tensors       what a Function saves for its backward besides (X, z).
# Every frame: _EVERY.  Padded logits masked by the frame counts: _Masked(n_obs).  Compact logits: a FrameIndex (below).
class _EveryFrame:
    suffix, fused, tail, tensors = '', True, (), ()

    def bind(self, X, elements, rows, who):
        return elements // rows

    def fwd_dims(self, X, rows, inner):
        return rows, inner, X.numel()

    bwd_dims = fwd_dims


_EVERY = _EveryFrame()


class _Masked(_EveryFrame):
    """the frames t < n_obs[n] of every sequence; the launches cover the padded frames too"""
    suffix = '_len'

    def __init__(self, n_obs):
        self.n_obs = n_obs

    def bind(self, X, elements, rows, who):
        n_obs, T, frame = _chk_n_obs(self.n_obs, X, who)
        self.tensors, self.tail = (n_obs,), (_ptr(n_obs), T, frame)
        return elements // rows


class _LogLikRowSum(torch.autograd.Function):
    """row sums of the Bernoulli log-likelihood of X under z, over the frames of ``route`` (gpode_loglik_rowsum_fwd[_len] / _bwd[_len])"""

    @staticmethod
    def forward(ctx, X, z, rows, route):
        X, z = _chk(X, 'X'), _chk(z, 'z')
        inner = route.bind(X, z.numel(), rows, 'bernoulli_loglik_rowsum')
        out = _new((rows,), z)
        _lib.call('gpode_loglik_rowsum_fwd' + route.suffix, _ptr(X), _ptr(z), _ptr(out), *route.fwd_dims(X, rows, inner), *route.tail, _stream())
        ctx.save_for_backward(X, z, *route.tensors)
        ctx.rows, ctx.inner, ctx.route = rows, inner, route
        return out

    @staticmethod
    def backward(ctx, g):
        X, z = ctx.saved_tensors[:2]
        route, gz = ctx.route, _new(z.shape, z)
        _lib.call('gpode_loglik_rowsum_bwd' + route.suffix, _ptr(X), _ptr(z), _ptr(g.contiguous()), _ptr(gz),
                  *route.bwd_dims(X, ctx.rows, ctx.inner), *route.tail, _stream())
        return None, gz, None, None


def _packed_halves(mu, logvar):
    """If (mu, logvar) are the two column halves of one contiguous (N, 2q) tensor (Encoder.forward returns fc(h).chunk(2)),
    return that tensor: the kernels then read both halves in place and produce ONE gradient for it."""
    base = getattr(mu, '_base', None)
    if base is None or getattr(logvar, '_base', None) is not base or base.dim() != 2 or not base.is_contiguous():
        return None
    N, q = mu.shape
    if tuple(base.shape) != (N, 2 * q) or mu.stride() != (2 * q, 1) or logvar.stride() != (2 * q, 1):
        return None
    if mu.data_ptr() != base.data_ptr() or logvar.data_ptr() != base.data_ptr() + 4 * q:
        return None
    return base


class _Reparam(torch.autograd.Function):
    """z = mu + exp(logvar / 2) * eps (vae.py:75-78) in one launch; h = [mu | logvar] packed (N, 2q)."""

    @staticmethod
    def forward(ctx, h, eps):
        h = _chk(h, 'h')
        N, q = h.shape[0], h.shape[1] // 2
        eps = _chk(eps, 'eps', (N, q))
        z = _new((N, q), h)
        _lib.call('gpode_reparam_fwd', _ptr(h), ctypes.c_void_p(h.data_ptr() + 4 * q), 2 * q, _ptr(eps), _ptr(z), N, q, _stream())
        ctx.save_for_backward(h, eps)
        return z

    @staticmethod
    def backward(ctx, gz):
        h, eps = ctx.saved_tensors
        N, q = h.shape[0], h.shape[1] // 2
        g = _new(h.shape, h)
        _lib.call('gpode_reparam_bwd', _ptr(gz.contiguous()), ctypes.c_void_p(h.data_ptr() + 4 * q), 2 * q, _ptr(eps), _ptr(g),
                  ctypes.c_void_p(g.data_ptr() + 4 * q), 2 * q, N, q, _stream())
        return g, None


class _ReparamKL(torch.autograd.Function):
    """_Reparam that also returns the partial sums of KL(q(z0) || N(0, I)) over its workgroups (gpode_reparam_kl_fwd): the ELBO adds
    them up instead of reading (mu | logvar) again, and the backward writes the gradient of h = [mu | logvar] through z AND through
    the KL sum in one launch -- otherwise two gradient tensors that autograd adds in a launch of its own."""

    @staticmethod
    def forward(ctx, h, eps):
        h = _chk(h, 'h')
        N, q = h.shape[0], h.shape[1] // 2
        eps = _chk(eps, 'eps', (N, q))
        z, klpart = _new((N, q), h), _new(((N * q + 255) // 256,), h)
        _lib.call('gpode_reparam_kl_fwd', _ptr(h), ctypes.c_void_p(h.data_ptr() + 4 * q), 2 * q, _ptr(eps), _ptr(z), _ptr(klpart), N, q, _stream())
        ctx.save_for_backward(h, eps)
        ctx.set_materialize_grads(False)
        return z, klpart

    @staticmethod
    def backward(ctx, gz, gkl):
        h, eps = ctx.saved_tensors
        N, q = h.shape[0], h.shape[1] // 2
        g = _new(h.shape, h)
        _lib.call('gpode_reparam_kl_bwd', _ptr(gz.contiguous() if gz is not None else None), _ptr(gkl.contiguous() if gkl is not None else None),
                  _ptr(h), ctypes.c_void_p(h.data_ptr() + 4 * q), 2 * q, _ptr(eps), _ptr(g), ctypes.c_void_p(g.data_ptr() + 4 * q), 2 * q, N, q,
                  _stream())
        return g, None


class _NormalKL(torch.autograd.Function):
    """sum_d KL(N(mu, exp(logvar/2)) || N(0, 1)) per row (what kl_divergence(q_dist, prior).sum(-1) evaluates,
    create_model.py:47-49); h = [mu | logvar] packed (N, 2q)."""

    @staticmethod
    def forward(ctx, h):
        h = _chk(h, 'h')
        N, q = h.shape[0], h.shape[1] // 2
        out = _new((N,), h)
        _lib.call('gpode_normal_kl_fwd', _ptr(h), ctypes.c_void_p(h.data_ptr() + 4 * q), 2 * q, _ptr(out), N, q, _stream())
        ctx.save_for_backward(h)
        return out

    @staticmethod
    def backward(ctx, g):
        (h,) = ctx.saved_tensors
        N, q = h.shape[0], h.shape[1] // 2
        gh = _new(h.shape, h)
        _lib.call('gpode_normal_kl_bwd', _ptr(g.contiguous()), _ptr(h), ctypes.c_void_p(h.data_ptr() + 4 * q), 2 * q, _ptr(gh),
                  ctypes.c_void_p(gh.data_ptr() + 4 * q), 2 * q, N, q, _stream())
        return gh


class _Elbo(torch.autograd.Function):
    """(loss, -mean lhood, mean KL(z0), KL(u)) of create_model.py:61-73 from the per-row terms, one launch."""

    @staticmethod
    def forward(ctx, lhood, klrow, kl_u, nobs):
        ctx.dims = (lhood.numel(), klrow.numel(), float(nobs), lhood.shape, klrow.shape, kl_u.shape)
        lhood, klrow, kl_u = _chk(lhood, 'lhood'), _chk(klrow, 'klrow'), _chk(kl_u, 'kl_u')
        out = _new((4,), lhood)
        _lib.call('gpode_elbo_fwd', _ptr(lhood), lhood.numel(), _ptr(klrow), klrow.numel(), _ptr(kl_u), ctypes.c_float(nobs), _ptr(out), _stream())
        return out

    @staticmethod
    def backward(ctx, gout):
        nl, nk, nobs, sl, sk, su = ctx.dims
        gl, gk, gu = _new(sl, gout), _new(sk, gout), _new(su, gout)
        _lib.call('gpode_elbo_bwd', _ptr(gout.contiguous()), nl, nk, ctypes.c_float(nobs), _ptr(gl), _ptr(gk), _ptr(gu), _stream())
        return gl, gk, gu, None


class _SigmoidLogLikParts(torch.autograd.Function):
    """Decoder logits -> partial row sums of the Bernoulli log-likelihood of X under sigmoid(logits) (gpode_sigmoid_loglik_fwd):
    the decoder's nn.Sigmoid (vae.py:84) and the summed log_prob (vae.py:136-153, create_model.py:49) in one pass over the logits.
    ``route``: every frame; the observed frames of a ragged minibatch, z for every element but sums and logit gradients for the frames
    t < n_obs[n] only (_fwd_len / _bwd_len); or COMPACT logits (L P, ...) in the order of a FrameIndex, rows (draw, sequence) as ever
    and the padded target frames of X never addressed (_fwd_pk / _bwd_pk)."""

    @staticmethod
    def forward(ctx, X, a, rows, route):
        X, a = _chk(X, 'X'), _chk(a, 'logits')
        inner = route.bind(X, a.numel(), rows, 'sigmoid_loglik_parts')
        ns = _lib.load().gpode_sigmoid_loglik_splits(rows, inner)
        z, part = torch.empty_like(a), _new((rows, ns), a)
        _lib.call('gpode_sigmoid_loglik_fwd' + route.suffix, _ptr(X), _ptr(a), _ptr(z), _ptr(part), *route.fwd_dims(X, rows, inner), ns,
                  *route.tail, _stream())
        ctx.save_for_backward(X, z, *route.tensors)
        ctx.rows, ctx.inner, ctx.route = rows, inner, route
        ctx.mark_non_differentiable(z)
        ctx.set_materialize_grads(False)             # no zero-filled stand-in for the gradient of z (a fill of rows x inner floats per step)
        part._gpode_ll = (X, z, route)               # for elbo_all(): its backward can then produce the logit gradients in the same launch
        return part, z

    @staticmethod
    def backward(ctx, gpart, _gz):
        X, z = ctx.saved_tensors[:2]
        ga = getattr(gpart, '_gpode_ga', None)       # already computed by the ELBO's backward (gpode_elbo_all_bwd_ll*)
        if ga is not None and ga.shape == z.shape:
            return None, ga, None, None
        # the ELBO hands every slice of a row the row's gradient: column 0 is the row gradient
        grow = gpart[:, 0].contiguous() if gpart.shape[1] > 1 else gpart.contiguous()
        ga = torch.empty_like(z)
        _lib.call('gpode_sigmoid_loglik_bwd' + ctx.route.suffix, _ptr(X), _ptr(z), _ptr(grow), _ptr(ga),
                  *ctx.route.bwd_dims(X, ctx.rows, ctx.inner), *ctx.route.tail, _stream())
        return None, ga, None, None


class _ElboAll(torch.autograd.Function):
    """(loss, -mean lhood, mean KL(z0), KL(u)) of create_model.py:61-73 from the likelihood partial sums, the encoder's packed
    (mu | logvar) rows and the inducing posterior, one launch forward and one backward (gpode_elbo_all_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, lpart, hs, hv, Um, Us, rows, M, nobs, ll=None):
        ctx.ll = ll
        lpart, hs, Um, Us = _chk(lpart, 'lpart'), _chk(hs, 'hs'), _chk(Um, 'Um'), _chk(Us, 'Us_sqrt.optvar')
        hv = _chk(hv, 'hv') if hv is not None else None
        N, q = hs.shape[0], hs.shape[1] // 2
        out = _new((4 + 256,), lpart)                # four results + the library's scratch
        _lib.call('gpode_elbo_all_fwd', _ptr(lpart), rows, lpart.numel(), _ptr(hs), _ptr(hv), N, q, M, Um.shape[1], _ptr(Um), _ptr(Us),
                  ctypes.c_float(nobs), _ptr(out), _stream())
        ctx.save_for_backward(hs, hv, Um, Us)
        ctx.dims = (rows, N, q, M, float(nobs), tuple(lpart.shape))
        ctx.set_materialize_grads(False)
        return out[0], out[1], out[2], out[3]

    @staticmethod
    def backward(ctx, g0, g1, g2, g3):
        hs, hv, Um, Us = ctx.saved_tensors
        rows, N, q, M, nobs, lshape = ctx.dims
        ghs, ghv = torch.empty_like(hs), (torch.empty_like(hv) if hv is not None else None)
        ll = ctx.ll if ctx.needs_input_grad[0] else None
        glr, dUm, dUs = _elbo_all_bwd(
            ctx, (g0, g1, g2, g3), 'gpode_elbo_all_bwd' if ll is None else 'gpode_elbo_all_bwd_ll', ll, Um, Us, rows, lshape,
            lambda glrow, dUm, dUs: (rows, _ptr(hs), _ptr(hv), N, q, M, Um.shape[1], _ptr(Um), _ptr(Us), ctypes.c_float(nobs), _ptr(glrow),
                                     _ptr(ghs), _ptr(ghv), _ptr(dUm), _ptr(dUs)))
        return glr, ghs, ghv, dUm, dUs, None, None, None, None


def _elbo_all_bwd(ctx, seeds, name, ll, Um, Us, rows, lshape, args, kl_inputs=(3, 4)):
    """What the backward of both ELBO forms does: gradient seeds -> ONE launch -> in overlap mode the gradients of (Um, Us) go to the
    flow's deferred backward -> the row gradient as a broadcast view.  ``name``: the entry point, without the route's suffix;
    ``args(glrow, dUm, dUs)``: its arguments between the seeds and the logit block.  ``ll`` = (X, z, route) of sigmoid_loglik_parts: the
    logits' gradient comes out of the same launch (every likelihood row receives the same gradient) and rides on the row gradient,
    where _SigmoidLogLikParts.backward finds it and launches nothing.  ``kl_inputs``: where (Um, Us) stand among the Function's inputs.
    -> (row gradient, dUm, dUs)"""
    gs = [None if g is None else g.contiguous().float() for g in seeds]
    glrow, dUm, dUs = _new((rows,), Um), torch.empty_like(Um), torch.empty_like(Us)
    ga, logit_block = None, ()
    if ll is not None:
        X, z, route = ll
        ga = torch.empty_like(z)
        name, logit_block = name + route.suffix, (_ptr(X), _ptr(z), _ptr(ga), z.numel(), X.numel(), *route.tail)
    _lib.call(name, *[_ptr(g) for g in gs], *args(glrow, dUm, dUs), *logit_block, _stream())
    if (ctx.needs_input_grad[kl_inputs[0]] and ctx.needs_input_grad[kl_inputs[1]] and Um.is_leaf and Us.is_leaf and
            ops.defer_kl_grads((Um, Us), (dUm, dUs))):
        dUm = dUs = None                             # overlap mode: the flow's deferred backward adds its share to them in place
    # every slice of a likelihood row carries the row's gradient (a broadcast view: nothing is copied)
    glr = glrow.view(rows, 1).expand(lshape)
    if ga is not None:
        glr._gpode_ga = ga
    return glr, dUm, dUs


# ---- ragged minibatches, compact route: the padded frames are taken out in front of the decoder (include/gpode.h) ------------------------
class FrameIndex:
    """The observed frames of a ragged minibatch (N sequences padded to T frames), see frame_index().  Also the loss stage's route
    over COMPACT logits (see _EveryFrame): the `_pk` entry points take ``off, T, frame`` (forward) or ``src, P, T, frame`` (backward)
    in front of nX, and there is no fused ELBO backward for them -- elbo_all() runs gpode_elbo_all_bwd, and the logits' gradient is one
    launch of its own."""
    __slots__ = ('off', 'src', 'P', 'N', 'T', 'counts')
    suffix, fused, tail, tensors = '_pk', False, (), ()

    def __init__(self, off, src, P, N, T, counts):
        self.off, self.src, self.P, self.N, self.T, self.counts = off, src, P, N, T, counts

    def _frame(self, X):
        return X.numel() // (self.N * self.T)

    def bind(self, X, elements, rows, who):
        N, T, P = self.N, self.T, self.P
        if X.dim() < 2 or tuple(X.shape[:2]) != (N, T) or rows % N != 0:
            raise _lib.GpodeError('%s: X must be (N,T,...) = (%d,%d,...) and rows a multiple of N; got %s, rows %d'
                                  % (who, N, T, tuple(X.shape), rows))
        frame, L = self._frame(X), rows // N
        if elements != L * P * frame:
            raise _lib.GpodeError('%s: %d compact logits expected (L P frame = %d x %d x %d), got %d'
                                  % (who, L * P * frame, L, P, frame, elements))
        return T * frame

    def fwd_dims(self, X, rows, inner):
        return rows, _ptr(self.off), self.T, self._frame(X), X.numel()

    def bwd_dims(self, X, rows, inner):
        return rows, _ptr(self.src), self.P, self.T, self._frame(X), X.numel()


def frame_index(n_obs, T, counts=None):
    """-> FrameIndex of a ragged minibatch: c[n] = clamp(n_obs[n], 0, T); ``off`` (N+1,) int32 on the device, the exclusive prefix sum
    of c with off[N] = P; ``src`` (P,) int32 on the device, src[j] = n T + t for compact image j = off[n] + t; ``P``, ``N``, ``T`` and the
    host ``counts`` c.  The compact batch of L draws is (L P, ...), ordered (l, n, t).
    The index needs the counts on the HOST: the decoder's launch sizes depend on P.  ``counts`` (a host sequence of N integers): nothing
    is read back.  Otherwise ``n_obs`` (N,) int32 on the device is read back once -- 4 N bytes and ONE SYNCHRONISATION per step, which a
    caller that has the counts on the host anyway avoids by passing them.  The index itself goes to the device in one copy.
    Refused under stream capture (the read-back and the copy cannot be captured, and a captured step would have P baked in) and when
    no frame of the minibatch is observed."""
    T = int(T)
    on_device = torch.is_tensor(n_obs) and n_obs.is_cuda
    if (on_device or (n_obs is None and torch.cuda.is_available())) and torch.cuda.is_current_stream_capturing():
        raise _lib.GpodeError('frame_index: the frame index cannot be built under stream capture (its size P sets the launch sizes of the '
                              'decoder); build it ahead of the capture, or run the step eagerly')
    if counts is None:
        if not (torch.is_tensor(n_obs) and n_obs.dim() == 1):
            raise _lib.GpodeError('frame_index: n_obs must be an (N,) integer tensor, or pass counts=')
        counts = n_obs.detach().cpu().tolist()       # the read-back: 4 N bytes, one synchronisation
    c = torch.as_tensor([int(k) for k in counts], dtype=torch.int64).reshape(-1).clamp_(0, T)
    N = c.numel()
    if torch.is_tensor(n_obs) and tuple(n_obs.shape) != (N,):
        raise _lib.GpodeError('frame_index: %d counts for n_obs of shape %s' % (N, tuple(n_obs.shape)))
    off = torch.zeros(N + 1, dtype=torch.int64)
    torch.cumsum(c, 0, out=off[1:])
    P = int(off[N])
    if P == 0:
        raise _lib.GpodeError('frame_index: no observed frame in the minibatch (every count is <= 0)')
    seq = torch.repeat_interleave(torch.arange(N), c)
    src = seq * T + (torch.arange(P) - off[:-1][seq])
    device = n_obs.device if torch.is_tensor(n_obs) else torch.device('cuda' if torch.cuda.is_available() else 'cpu')
    both = torch.cat((off, src)).to(torch.int32).to(device)
    return FrameIndex(both[:N + 1], both[N + 1:], P, N, T, c.tolist())


class _GatherFrames(torch.autograd.Function):
    """ztL (L,N,T,ld) -> the first q columns of the observed rows, (L P, q) ordered (l, n, t) (gpode_gather_frames_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, zt, index, q):
        zt = _chk(zt, 'ztL')
        if zt.dim() != 4 or tuple(zt.shape[1:3]) != (index.N, index.T):
            raise _lib.GpodeError('gather_frames: ztL must be (L,N,T,ld) = (L,%d,%d,ld), got %s' % (index.N, index.T, tuple(zt.shape)))
        L, N, T, ld = zt.shape
        out = _new((L * index.P, q), zt)
        _lib.call('gpode_gather_frames_fwd', _ptr(zt), ld, q, _ptr(index.src), L, N, T, index.P, _ptr(out), _stream())
        ctx.index, ctx.dims = index, (L, N, T, ld, q)
        return out

    @staticmethod
    def backward(ctx, gout):
        index, (L, N, T, ld, q) = ctx.index, ctx.dims
        gzt = _new((L, N, T, ld), gout)
        _lib.call('gpode_gather_frames_bwd', _ptr(gout.contiguous()), ld, q, _ptr(index.src), _ptr(index.off), L, N, T, index.P, _ptr(gzt),
                  _stream())
        return gzt, None, None


def gather_frames(ztL, index, q):
    """The latent states of the observed frames only: ztL (L,N,T,order*q) -> (L P, q), the first ``q`` columns (the positions of a
    second-order model) of the rows ``index`` (frame_index) lists, ordered (l, n, t).  The backward writes every element of the
    gradient of ztL: zero on padded rows and on the columns >= q."""
    return _GatherFrames.apply(ztL, index, int(q))


def sigmoid_loglik_parts(X, logits, rows, n_obs=None, *, index=None):
    """-> (partial row sums (rows, nsplit) of the Bernoulli log-likelihood, z = sigmoid(logits)).  ``n_obs`` (N,) int32: the frame
    count of every sequence of a ragged (padded) minibatch X (N,T,...) -- the sums take the frames t < n_obs[n] only and the padded
    logits get a zero gradient; None: every frame, the launches as they always were.
    ``index`` (frame_index; not together with ``n_obs``): ``logits`` are COMPACT, (L P, ...) for the observed frames only, ordered
    (l, n, t) -- z and the logit gradients are compact as well, rows stay (draw, sequence)."""
    if index is not None and n_obs is not None:
        raise _lib.GpodeError('sigmoid_loglik_parts: n_obs (padded logits, masked) and index (compact logits) exclude each other')
    return _SigmoidLogLikParts.apply(X, logits, rows, index if index is not None else _Masked(n_obs) if n_obs is not None else _EVERY)


class _ElboAllKL(torch.autograd.Function):
    """_ElboAll on the KL partial sums of _ReparamKL instead of the packed (mu | logvar) rows (gpode_elbo_all_fwd_kl /
    gpode_elbo_all_bwd_ll_kl); its backward also produces the logits' gradient (ll = (X, z, route) of sigmoid_loglik_parts)."""

    @staticmethod
    def forward(ctx, lpart, kls, klv, Um, Us, rows, N, M, nobs, ll):
        lpart, kls, Um, Us = _chk(lpart, 'lpart'), _chk(kls, 'kl partial sums'), _chk(Um, 'Um'), _chk(Us, 'Us_sqrt.optvar')
        klv = _chk(klv, 'kl partial sums (v)') if klv is not None else None
        out = _new((4 + 256,), lpart)
        _lib.call('gpode_elbo_all_fwd_kl', _ptr(lpart), rows, lpart.numel(), _ptr(kls), kls.numel(), _ptr(klv), klv.numel() if klv is not None else 0,
                  N, M, Um.shape[1], _ptr(Um), _ptr(Us), ctypes.c_float(nobs), _ptr(out), _stream())
        ctx.save_for_backward(Um, Us)
        ctx.dims = (rows, N, M, float(nobs), tuple(lpart.shape), kls.numel(), klv.numel() if klv is not None else 0)
        ctx.ll = ll
        ctx.set_materialize_grads(False)
        return out[0], out[1], out[2], out[3]

    @staticmethod
    def backward(ctx, g0, g1, g2, g3):
        Um, Us = ctx.saved_tensors
        rows, N, M, nobs, lshape, nks, nkv = ctx.dims
        gkls, gklv = _new((nks,), Um), (_new((nkv,), Um) if nkv else None)
        glr, dUm, dUs = _elbo_all_bwd(
            ctx, (g0, g1, g2, g3), 'gpode_elbo_all_bwd_ll_kl', ctx.ll, Um, Us, rows, lshape,
            lambda glrow, dUm, dUs: (rows, N, M, Um.shape[1], _ptr(Um), _ptr(Us), ctypes.c_float(nobs), _ptr(glrow), _ptr(gkls), nks,
                                     _ptr(gklv), nkv, _ptr(dUm), _ptr(dUs)))
        return glr, gkls, gklv, dUm, dUs, None, None, None, None, None


def elbo_all(lpart, mu_s, logvar_s, mu_v, logvar_v, Um, Us_packed, M, nobs):
    """-> (loss, nll, kl_reg, kl_u), see _ElboAll."""
    # (X, z, route) when the backward can produce the logits' gradient in its own launch: the parts come from sigmoid_loglik_parts
    # on a route that has the fused form, and X covers the logits a whole number of times (the draws)
    ll = getattr(lpart, '_gpode_ll', None)
    if ll is not None and not (ll[2].fused and ll[1].numel() % ll[0].numel() == 0):
        ll = None
    hs0 = _packed_halves(mu_s, logvar_s)
    kls = getattr(hs0, '_gpode_klpart', None) if hs0 is not None else None
    klv = None
    if mu_v is not None:
        hv0 = _packed_halves(mu_v, logvar_v)
        klv = getattr(hv0, '_gpode_klpart', None) if hv0 is not None else None
    if ll is not None and kls is not None and (mu_v is None or klv is not None):
        return _ElboAllKL.apply(lpart, kls, klv, Um, Us_packed, lpart.shape[0], mu_s.shape[0], M, float(nobs), ll)
    hv = _pack(mu_v, logvar_v) if mu_v is not None else None
    return _ElboAll.apply(lpart, _pack(mu_s, logvar_s), hv, Um, Us_packed, lpart.shape[0], M, float(nobs), ll)


def _pack(mu, logvar):
    h = _packed_halves(mu, logvar)
    return h if h is not None else torch.cat((mu, logvar), dim=1)


def reparam(mu, logvar, eps):
    h = _packed_halves(mu, logvar)
    if h is not None and h.requires_grad:
        # (mu | logvar) are the halves of the encoder's fc output: the KL term's partial sums ride along for elbo_all()
        z, klpart = _ReparamKL.apply(h, eps)
        h._gpode_klpart = klpart
        return z
    return _Reparam.apply(_pack(mu, logvar), eps)


def reparam_draws(mu, logvar, eps, out=None, col=0, lw=None):
    """L reparameterised draws of one N(mu, exp(logvar)) (N,q) and their importance log-weights, one launch (gpode_reparam_draws_fwd):
    eps (L,N,q) -> z[l] = mu + exp(logvar / 2) eps[l] -- the bits reparam() gives draw by draw -- and
    lw[l,n] = sum_i log N(z; 0, 1) - log N(z; mu, sigma^2) (L,N).  ``out`` (L,N,W) with ``col``: z is written into columns
    col .. col+q-1 of it (one half of an order-2 state) and that view is returned; ``lw``: the sum is ADDED to it (the other half's).
    Forward only, in place: the evaluation's form.  reparam_draws_train() is the differentiable one."""
    h = _chk(_pack(mu, logvar).detach(), 'h')
    N, q = h.shape[0], h.shape[1] // 2
    if eps.dim() != 3:
        raise _lib.GpodeError('reparam_draws: eps must be (L,N,q), got %s' % (tuple(eps.shape),))
    L = eps.shape[0]
    eps = _chk(eps, 'eps', (L, N, q))
    if out is None:
        out, col = _new((L, N, q), h), 0
    W = out.shape[-1]
    if tuple(out.shape) != (L, N, W) or not out.is_contiguous() or out.dtype != torch.float32 or not out.is_cuda or col < 0 or col + q > W:
        raise _lib.GpodeError('reparam_draws: out must be a contiguous float32 (L,N,W) with col + q <= W, got %s, col %d' % (tuple(out.shape), col))
    acc = 1 if lw is not None else 0
    if lw is None:
        lw = _new((L, N), h)
    elif tuple(lw.shape) != (L, N) or not lw.is_contiguous() or lw.dtype != torch.float32 or not lw.is_cuda:
        raise _lib.GpodeError('reparam_draws: lw must be a contiguous float32 (L,N), got %s' % (tuple(lw.shape),))
    _lib.call('gpode_reparam_draws_fwd', _ptr(h), ctypes.c_void_p(h.data_ptr() + 4 * q), 2 * q, _ptr(eps),
              ctypes.c_void_p(out.data_ptr() + 4 * col), W, _ptr(lw), acc, L, N, q, _stream())
    return out[..., col:col + q], lw


class _ReparamDraws(torch.autograd.Function):
    """K reparameterised draws of the encoders' distributions and their importance log-weights, with a backward (training on the
    importance-weighted bound): hs = [mu | logvar] (N, 2q) of the position encoder, hv the velocity encoder's of a second-order model
    or None -> z (K,N,order*q), the two halves side by side, and lw (K,N), the sum of the two.  One gpode_reparam_draws_fwd per encoder,
    the second adding to lw; the backward is one gpode_reparam_draws_bwd per encoder, reading its half of the state gradient in place."""

    @staticmethod
    def forward(ctx, hs, hv, eps_s, eps_v):
        hs = _chk(hs, 'hs')
        N, q = hs.shape[0], hs.shape[1] // 2
        if eps_s.dim() != 3:
            raise _lib.GpodeError('reparam_draws_train: eps must be (K,N,q), got %s' % (tuple(eps_s.shape),))
        K = eps_s.shape[0]
        eps_s = _chk(eps_s, 'eps', (K, N, q))
        W = q if hv is None else 2 * q
        z, lw = _new((K, N, W), hs), _new((K, N), hs)
        _lib.call('gpode_reparam_draws_fwd', _ptr(hs), ctypes.c_void_p(hs.data_ptr() + 4 * q), 2 * q, _ptr(eps_s), _ptr(z), W, _ptr(lw), 0,
                  K, N, q, _stream())
        if hv is not None:
            hv, eps_v = _chk(hv, 'hv', (N, 2 * q)), _chk(eps_v, 'eps (v)', (K, N, q))
            _lib.call('gpode_reparam_draws_fwd', _ptr(hv), ctypes.c_void_p(hv.data_ptr() + 4 * q), 2 * q, _ptr(eps_v),
                      ctypes.c_void_p(z.data_ptr() + 4 * q), W, _ptr(lw), 1, K, N, q, _stream())
        ctx.save_for_backward(hs, hv, eps_s, eps_v)
        ctx.set_materialize_grads(False)
        return z, lw

    @staticmethod
    def backward(ctx, gz, glw):
        hs, hv, eps_s, eps_v = ctx.saved_tensors
        N, q = hs.shape[0], hs.shape[1] // 2
        K, W = eps_s.shape[0], (q if hv is None else 2 * q)
        gz = gz.contiguous() if gz is not None else None
        glw = glw.contiguous() if glw is not None else None
        out = []
        for col, h, eps in ((0, hs, eps_s), (q, hv, eps_v)):
            if h is None:
                out.append(None)
                continue
            g = _new(h.shape, h)
            _lib.call('gpode_reparam_draws_bwd', ctypes.c_void_p(gz.data_ptr() + 4 * col) if gz is not None else None, W, _ptr(glw), _ptr(h),
                      ctypes.c_void_p(h.data_ptr() + 4 * q), 2 * q, _ptr(eps), _ptr(g), ctypes.c_void_p(g.data_ptr() + 4 * q), 2 * q, K, N, q,
                      _stream())
            out.append(g)
        return out[0], out[1], None, None


def reparam_draws_train(mu_s, logvar_s, eps_s, mu_v=None, logvar_v=None, eps_v=None):
    """The differentiable form of reparam_draws(): K draws per sequence of q(z0 | x) -> fresh z (K,N,order*q) and
    lw (K,N) = log p(z) - log q(z | x), the gradients of both flowing back to (mu, logvar) of either encoder (_ReparamDraws)."""
    hv = _pack(mu_v, logvar_v) if mu_v is not None else None
    return _ReparamDraws.apply(_pack(mu_s, logvar_s), hv, eps_s, eps_v)


class _ElboIW(torch.autograd.Function):
    """(loss, -mean iw, -mean lw, KL(u), mean ess) of the importance-weighted bound from the likelihood partial sums of L K N rows
    ordered (l,k,n) and the log-weights lw (K,N): gpode_elbo_iw_fwd, and ONE backward launch -- gpode_elbo_iw_bwd_ll, which also
    produces the logits' gradient (ll = (X, z, route) of sigmoid_loglik_parts), or gpode_elbo_iw_bwd where the route has no fused
    form, _SigmoidLogLikParts.backward then launching from column 0 of the row gradient.  The ess output carries no gradient."""

    @staticmethod
    def forward(ctx, lpart, lw, Um, Us, L, K, N, M, nobs, ll):
        lpart, lw, Um, Us = _chk(lpart, 'lpart'), _chk(lw, 'lw', (K, N)), _chk(Um, 'Um'), _chk(Us, 'Us_sqrt.optvar')
        rows = L * K * N
        if lpart.dim() != 2 or lpart.shape[0] != rows:
            raise _lib.GpodeError('elbo_iw: lpart must be (L K N, nsplit) = (%d, nsplit), got %s' % (rows, tuple(lpart.shape)))
        out = _new((5 + 256,), lpart)                # five results + the library's scratch
        _lib.call('gpode_elbo_iw_fwd', _ptr(lpart), rows, lpart.shape[1], _ptr(lw), L, K, N, M, Um.shape[1], _ptr(Um), _ptr(Us),
                  ctypes.c_float(nobs), _ptr(out), _stream())
        ctx.save_for_backward(lpart, lw, Um, Us)
        ctx.dims = (rows, L, K, N, M, float(nobs), tuple(lpart.shape))
        ctx.ll = ll
        ctx.set_materialize_grads(False)
        return out[0], out[1], out[2], out[3], out[4]

    @staticmethod
    def backward(ctx, g0, g1, g2, g3, _g4):
        lpart, lw, Um, Us = ctx.saved_tensors
        rows, L, K, N, M, nobs, lshape = ctx.dims
        glw = torch.empty_like(lw)
        ll = ctx.ll if ctx.needs_input_grad[0] else None
        glr, dUm, dUs = _elbo_all_bwd(
            ctx, (g0, g1, g2, g3, None), 'gpode_elbo_iw_bwd' if ll is None else 'gpode_elbo_iw_bwd_ll', ll, Um, Us, rows, lshape,
            lambda grow, dUm, dUs: (_ptr(lpart), rows, lshape[1], _ptr(lw), L, K, N, M, Um.shape[1], _ptr(Um), _ptr(Us), ctypes.c_float(nobs),
                                    _ptr(grow), _ptr(glw), _ptr(dUm), _ptr(dUs)), kl_inputs=(2, 3))
        return glr, glw, dUm, dUs, None, None, None, None, None, None


def elbo_iw(lpart, lw, Um, Us_packed, L, K, N, M, nobs, fused=True):
    """-> (loss, iw_nll, kl_mc, kl_u, ess): the importance-weighted bound over K initial-state draws per sequence, shared by the L
    function draws (_ElboIW).  ``lpart``: sigmoid_loglik_parts over the L K N rows ordered (l,k,n); ``lw`` (K,N): reparam_draws_train.
    ``fused=False`` (A/B), and every route without the fused form (ragged minibatches): the logits' gradient is a launch of its own."""
    ll = getattr(lpart, '_gpode_ll', None) if fused else None
    if ll is not None and not (ll[2].fused and ll[2].suffix == '' and ll[1].numel() % ll[0].numel() == 0):
        ll = None
    return _ElboIW.apply(lpart, lw, Um, Us_packed, int(L), int(K), int(N), int(M), float(nobs), ll)


def normal_kl_rows(mu, logvar):
    return _NormalKL.apply(_pack(mu, logvar))


def elbo_terms(lhood_rows, kl_rows, kl_u, nobs):
    """-> tensor [loss, nll, kl_reg, kl_u] (views are taken by the caller)."""
    return _Elbo.apply(lhood_rows, kl_rows, kl_u, float(nobs))


def conv2d(x, w, b, stride, pad):
    return _Conv2d.apply(x, w, b, stride, pad)


def conv_transpose2d(x, w, b, stride, pad, out_pad=0, stats_for=None):
    """``stats_for``: the nn.BatchNorm2d (training mode) that follows -- its batch statistics are then summed by this convolution."""
    return _ConvT2d.apply(x, w, b, stride, pad, out_pad, stats_for)


def batch_norm_train(x, bn, relu):
    """nn.BatchNorm2d in training mode on the module's own parameters/buffers (updates running stats)."""
    # running statistics and the num_batches_tracked counter are updated by the kernel itself (one launch less per layer)
    return _BatchNormTrain.apply(x, bn.weight, bn.bias, bn.running_mean if bn.training else None,
                                 bn.running_var if bn.training else None, bn.momentum, bn.eps, relu,
                                 bn.num_batches_tracked if bn.training else None)


def _matrix_core_path(*tensors):
    """False under GPODE_CONV_VALU=1 (the library reads it once per process) or when an operand is not a 16-byte aligned dense tensor as
    it stands: the convolutions then run their VALU / generic kernels, which take no BatchNorm table."""
    return os.environ.get('GPODE_CONV_VALU', '0') != '1' and all(not t.is_contiguous() or t.data_ptr() % 16 == 0 for t in tensors)


def bn_relu_conv_transpose2d(c, bn, w, b, stride, pad, out_pad=0, stats_for=None):
    """conv_transpose2d(relu(bn(c)), w, b) for a BatchNorm2d module in training mode, fused (see _BnReluConvT).  ``stats_for``: the
    BatchNorm2d that follows THIS convolution (see conv_transpose2d)."""
    if not _matrix_core_path(c, w):
        # the fused form exists on the matrix-core kernels only: the separate ops, same result
        pre = getattr(c, '_gpode_bnstats', None)
        if c.data_ptr() % 16:                        # (the BatchNorm kernels read float4 where the image size allows)
            c = c.clone(memory_format=torch.contiguous_format)
        if pre is not None and pre[0] is bn:         # the producer of c has updated bn's running statistics already
            a = _BatchNormTrain.apply(c, bn.weight, bn.bias, None, None, bn.momentum, bn.eps, True, None)
        else:
            a = batch_norm_train(c, bn, True)
        return conv_transpose2d(a, w, b, stride, pad, out_pad, stats_for)
    return _BnReluConvT.apply(c, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps,
                              w, b, stride, pad, out_pad, bn, stats_for)


def batch_norm_eval(x, bn, relu):
    """nn.BatchNorm2d in evaluation mode on the module's running statistics."""
    return _BatchNormEval.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, relu)


def relu(x):
    return _Act.apply(x, 0)


def sigmoid(x):
    return _Act.apply(x, 1)


def linear(x, w, b):
    return _Linear.apply(x, w, b)


def linear_relu_in(x, w, b):
    """linear(relu(x), w, b); the ReLU is folded into the layer for wide fan-in (>= 128 inputs), applied separately otherwise."""
    if x.dim() == 2 and x.shape[1] >= 128 and x.shape[0] * w.shape[0] <= (1 << 22):
        return _LinearReluIn.apply(x, w, b)
    return _Linear.apply(relu(x), w, b)


def bernoulli_loglik(X, z):
    """log(z) X + log(1-z)(1-X), X broadcast over the leading copies of z (vae.py:136-153)."""
    return _LogLik.apply(X, z)


def bernoulli_loglik_rowsum(X, z, rows, n_obs=None):
    """``n_obs`` (N,) int32: sum the frames t < n_obs[n] of a ragged minibatch only (sigmoid_loglik_parts); None: every frame."""
    return _LogLikRowSum.apply(X, z, rows, _Masked(n_obs) if n_obs is not None else _EVERY)


# ---- frozen decoder / posterior-predictive evaluation (forward only; evaluate.py) ------------------------------------------------
def bn_eval_table(bn):
    """{running_mean, rsqrt(running_var + eps), gamma, beta} per channel of an nn.BatchNorm2d in evaluation mode, (C, 4): the table
    gpode_conv2d_bwd_data_bn / gpode_dec10_predict apply to the raw output of the layer in front.  Writes no module buffer."""
    if bn.training:
        raise _lib.GpodeError('bn_eval_table: the BatchNorm module is in training mode (its batch statistics are not a table of constants)')
    g = _chk(bn.weight.detach(), 'gamma')
    table = _new((g.shape[0], 4), g)
    _lib.call('gpode_bn_eval_table', _ptr(g), _ptr(_chk(bn.bias.detach(), 'beta')), _ptr(_chk(bn.running_mean, 'running_mean')),
              _ptr(_chk(bn.running_var, 'running_var')), ctypes.c_float(bn.eps), _ptr(table), g.shape[0], _stream())
    return table


def table_conv_transpose2d(c, table, w, b, stride, pad, out_pad=0):
    """conv_transpose2d(relu(bn(c)), w, b) with the BatchNorm given as a (C, 4) table; no graph is recorded."""
    c, w, table = _chk(c.detach(), 'c'), _chk(w.detach(), 'weight'), _chk(table, 'table')
    B, Cin, Hi, Wi = c.shape
    _, Cout, K, _ = w.shape
    if tuple(table.shape) != (Cin, 4):
        raise _lib.GpodeError('table_conv_transpose2d: table must be (%d, 4)' % Cin)
    Ht, Wt = _convT_out(Hi, Wi, K, stride, pad, out_pad)
    y = _new((B, Cout, Ht, Wt), c)
    _lib.call('gpode_conv2d_bwd_data_bn', _ptr(c), _ptr(table), _ptr(w), _ptr(None if b is None else _chk(b.detach(), 'bias')), _ptr(y),
              B, Cout, Ht, Wt, Cin, K, stride, pad, Hi, Wi, _stream())
    return y


class PredictState:
    """State of gpode_dec10_predict for F = N * Th frames: Welford mean / M2 of the decoded images over the draws (``variance``),
    {count, mean, M2} of the squared error per frame, and the number of draws folded in so far.  ``loglik`` = L > 0 adds ``ell`` (L, F),
    the log-likelihood of every (draw, frame) image against its target (gpode_dec10_predict_ll), for L draws in all."""

    def __init__(self, F, device, variance=True, loglik=0):
        self.F, self.done = int(F), 0
        self.ell = torch.zeros(int(loglik), F, dtype=torch.float32, device=device) if loglik > 0 else None
        self.mean = torch.zeros(F, 784, dtype=torch.float32, device=device) if variance else None
        self.m2 = torch.zeros(F, 784, dtype=torch.float32, device=device) if variance else None
        self.se = torch.zeros(F, 3, dtype=torch.float32, device=device)


def dec10_predict(c, table, w, b, X, Th, state, n_obs=None):
    """Fold the draws held in ``c`` -- raw decnn.7 output (Lc * F, 16, 28, 28) laid out (draw, frame) -- into ``state``:
    sigmoid(decnn.10(relu(bn(c)))) is formed in registers and only its statistics against the targets X (N, T_obs, 1, 28, 28) leave
    the kernel (frames t >= T_obs of a sequence have no target and add nothing to the error).  A state with ``ell`` takes
    gpode_dec10_predict_ll, which also writes the rows of ``ell`` of these draws; a state without it takes gpode_dec10_predict.
    ``n_obs`` (N,) int32: the frame count of every sequence of a ragged X -- frame t of sequence n has a target iff
    t < min(T_obs, n_obs[n]) (the *_len entry points); None: the launches as they always were."""
    c, w, table, X = _chk(c.detach(), 'c'), _chk(w.detach(), 'weight'), _chk(table, 'table'), _chk(X, 'X')
    name, extra = 'gpode_dec10_predict', ()
    if n_obs is not None:
        n_obs = _chk_n_obs(n_obs, X, 'dec10_predict')[0]
    F = state.F
    N, T_obs = X.shape[0], X.shape[1]
    if tuple(c.shape[1:]) != (16, 28, 28) or tuple(w.shape) != (16, 1, 5, 5) or tuple(table.shape) != (16, 4):
        raise _lib.GpodeError('dec10_predict: c (B,16,28,28), weight (16,1,5,5), table (16,4)')
    if tuple(X.shape[2:]) != (1, 28, 28) or F != N * Th or c.shape[0] % F != 0 or c.shape[0] == 0:
        raise _lib.GpodeError('dec10_predict: X (N,T_obs,1,28,28), F = N * Th frames, c a whole number of draws of F frames')
    Lc = c.shape[0] // F
    ell = getattr(state, 'ell', None)
    if ell is not None:
        if ell.dim() != 2 or ell.shape[1] != F or ell.dtype != torch.float32 or not ell.is_contiguous():
            raise _lib.GpodeError('gpode_dec10_predict_ll: ell must be a contiguous float32 (L_total, F) tensor')
        name, extra = name + '_ll', (_ptr(ell), ell.shape[0])
    if n_obs is not None:
        name, extra = name + '_len', extra + (_ptr(n_obs),)
    _lib.call(name, _ptr(c), _ptr(table), _ptr(w), _ptr(None if b is None else _chk(b.detach(), 'bias')), _ptr(X),
              Lc, F, int(Th), T_obs, state.done, _ptr(state.mean), _ptr(state.m2), _ptr(state.se), *extra, _stream())
    state.done += Lc
    return state


class CondState:
    """State of gpode_dec10_predict_w for F = N * Th frames of N sequences: ``wstate`` (F,2) = {ref, W} -- the largest log-weight folded
    so far and W = sum_l exp(logw_l - ref) --, the weighted ``mean`` / ``m2`` (F,784) of the decoded images over the draws, ``wse`` (F,)
    the weighted sum of the per-image squared error, and ``done``, the number of draws folded in.  ``bad`` is a device flag that
    dec10_predict_w raises (without a host sync) when a log-weight is NaN or +inf; ``check()`` reads it -- one sync, where the results
    are read anyway -- and refuses such a state."""

    def __init__(self, F, N, device):
        self.F, self.N, self.done = int(F), int(N), 0
        if self.N < 1 or self.F < 1 or self.F % self.N != 0:
            raise _lib.GpodeError('CondState: F = N * Th frames of N >= 1 sequences; got F = %d, N = %d' % (self.F, self.N))
        self.wstate = torch.zeros(self.F, 2, dtype=torch.float32, device=device)
        self.mean = torch.zeros(self.F, 784, dtype=torch.float32, device=device)
        self.m2 = torch.zeros(self.F, 784, dtype=torch.float32, device=device)
        self.wse = torch.zeros(self.F, dtype=torch.float32, device=device)
        self.bad = torch.zeros((), dtype=torch.bool, device=device)

    def check(self):
        if bool(self.bad.item()):
            raise _lib.GpodeError('dec10_predict_w: a log-weight was NaN or +inf (-inf means weight 0; anything else must be finite)')
        return self


def dec10_predict_w(c, table, w, b, X, Th, state, logw, n_obs=None):
    """The importance-weighted twin of dec10_predict (gpode_dec10_predict_w): fold the draws held in ``c`` -- (Lc * F, 16, 28, 28), laid
    out (draw, frame) -- into the CondState ``state`` under the log-weights ``logw`` (L_total, N) float32, whose rows
    state.done .. state.done + Lc - 1 belong to these draws.  -inf is weight 0; a NaN or +inf is refused: the flag ``state.bad`` is
    raised on the device and ``state.check()`` throws, so that a pass costs no host sync (the kernel itself treats such a draw as
    weight 0).  ``n_obs`` (N,) int32 as in dec10_predict; None: every frame t < T_obs has a target."""
    c, w, table, X = _chk(c.detach(), 'c'), _chk(w.detach(), 'weight'), _chk(table, 'table'), _chk(X, 'X')
    if not isinstance(state, CondState):
        raise _lib.GpodeError('dec10_predict_w: state must be a vae_ops.CondState')
    if n_obs is not None:
        n_obs = _chk_n_obs(n_obs, X, 'dec10_predict_w')[0]
    F, N, T_obs = state.F, X.shape[0], X.shape[1]
    if tuple(c.shape[1:]) != (16, 28, 28) or tuple(w.shape) != (16, 1, 5, 5) or tuple(table.shape) != (16, 4):
        raise _lib.GpodeError('dec10_predict_w: c (B,16,28,28), weight (16,1,5,5), table (16,4)')
    if tuple(X.shape[2:]) != (1, 28, 28) or N != state.N or F != N * Th or c.shape[0] % F != 0 or c.shape[0] == 0:
        raise _lib.GpodeError('dec10_predict_w: X (N,T_obs,1,28,28), F = N * Th frames, c a whole number of draws of F frames')
    Lc = c.shape[0] // F
    if not (torch.is_tensor(logw) and logw.is_cuda and logw.dtype == torch.float32 and logw.dim() == 2 and logw.shape[1] == N
            and logw.is_contiguous()):
        raise _lib.GpodeError('gpode_dec10_predict_w: logw must be a contiguous float32 (L_total, N) tensor on the device')
    if state.done + Lc > logw.shape[0]:
        raise _lib.GpodeError('gpode_dec10_predict_w: logw has %d rows, need done + Lc = %d' % (logw.shape[0], state.done + Lc))
    state.bad |= ~(logw[state.done:state.done + Lc] < float('inf')).all()      # NaN or +inf; stays on the device
    _lib.call('gpode_dec10_predict_w', _ptr(c), _ptr(table), _ptr(w), _ptr(None if b is None else _chk(b.detach(), 'bias')), _ptr(X),
              Lc, F, int(Th), T_obs, state.done, _ptr(logw), logw.shape[0], N, _ptr(state.wstate), _ptr(state.mean), _ptr(state.m2),
              _ptr(state.wse), _ptr(n_obs), _stream())
    state.done += Lc
    return state
