"""Host side of vae_ops and create_model.compute_loss: WHICH entry points every public wrapper calls, in which order and with which
arguments -- pinned as transcripts, so that the autograd layer can be rearranged without a GPU telling whether a launch changed.

Host tensors stand in for device tensors (the pattern of test_time_grids_host): ``vae_ops._chk`` lets them through, ``vae_ops._stream``
is a null pointer and ``_lib.call`` is a recorder that returns 0, so no kernel runs.  The real library is still loaded for the host-only
size queries (gpode_sigmoid_loglik_splits, gpode_bn_scratch, gpode_dec10_bn_*_scratch_floats, gpode_conv_wgrad_scratch,
gpode_linear_bwd_scratch).  Per call the recorder keeps the name and every argument: integers and floats as values, pointers
symbolically -- ``0`` for null, the name of the caller's tensor they point into (plus the byte offset), else ``new#k`` by order of first
appearance -- so a swapped pair of pointers or a dropped offset changes the transcript.  ``vae_ops._ptr`` is wrapped to learn the extent
of every tensor handed to the library (a pointer into the middle of a fresh tensor reads ``new#k+offset``) and to keep it alive for the
scenario (no address is used twice).  The calls of a fake two-rank BatchNorm group and gpode_defer_reductions are recorded in line.

Only public functions (and set_bn_sync) are driven; besides the stand-ins above the test touches the switches ``_FUSED_STATS_MIN_IMAGES``
and ``create_model._FUSED_LOSS``, reads ``_deferred`` and sets the attribute ``_gpode_slot``.  EXPECTED below was written by ``python tests/test_vae_ops_calls_host.py`` from the tree in front of the change that
made the loss-stage routes data (one _SigmoidLogLikParts / _LogLikRowSum, shared ELBO backward tail, BatchNorm halves); the same
literals hold behind it."""
import contextlib
import ctypes
import os
import pprint
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, L, Q, M, DO = 3, 4, 2, 2, 5, 2
NOBS = 360.0


class _OnDevice(torch.Tensor):
    """a host tensor that answers is_cuda (BatchNorm's num_batches_tracked is checked by the wrapper itself, not by _chk)"""
    is_cuda = property(lambda self: True)


class Recorder:
    def __init__(self):
        self.lines, self.named, self.new, self.extent, self.keep = [], [], [], {}, []

    def name(self, **tensors):
        for k, t in tensors.items():
            st = t.untyped_storage()
            self.named.append((st.data_ptr(), max(st.nbytes(), 1), k))
            self.keep.append(t)
        return tensors[k]

    def ptr(self, t):                                # stands in for vae_ops._ptr
        if t is None:
            return ctypes.c_void_p(0)
        st = t.untyped_storage()
        self.extent[st.data_ptr()] = max(st.nbytes(), 1)
        self.keep.append(t)
        return ctypes.c_void_p(t.data_ptr())

    def label(self, p):
        if not p:
            return '0'
        for lo, n, k in self.named:
            if lo <= p < lo + n:
                return k if p == lo else '%s+%d' % (k, p - lo)
        for i, (lo, n) in enumerate(self.new):
            if lo <= p < lo + n:
                return 'new#%d' % i if p == lo else 'new#%d+%d' % (i, p - lo)
        for lo, n in self.extent.items():
            if lo <= p < lo + n:
                break
        else:
            lo, n = p, 1
        self.new.append((lo, n))
        return self.label(p)

    def fmt(self, a):
        if isinstance(a, ctypes.c_void_p):
            return self.label(a.value)
        if isinstance(a, ctypes.c_float):
            return '%.6g' % a.value
        if isinstance(a, float):
            return '%.6g' % a
        if isinstance(a, (bool, int)):
            return str(int(a))
        if torch.is_tensor(a):
            return self.label(a.data_ptr())
        raise AssertionError('argument of an unexpected type: %r' % (a,))

    def call(self, name, *args):                     # stands in for _lib.call
        self.lines.append('%s(%s)' % (name, ', '.join(self.fmt(a) for a in args)))
        return 0

    def note(self, text):
        self.lines.append(text)

    def raises(self, what, fn, kind=None):
        from vae_gp_ode_amd import _lib
        try:
            fn()
        except (kind or _lib.GpodeError) as e:
            self.lines.append('%s -> %s: %s' % (what, type(e).__name__, e))
        else:
            self.lines.append('%s -> no error' % what)


class Sync:
    """a two-rank parallel.BatchNormSync as far as vae_ops looks at one"""
    world = 2

    def __init__(self, rec):
        self.rec, self.w = rec, rec.name(sync_weights=torch.ones(2))

    def gather(self, t):
        self.rec.note('sync.gather(%s)' % self.rec.fmt(t))
        return t.repeat(2)

    def gather_many(self, ts):
        self.rec.note('sync.gather_many(%s)' % ', '.join(self.rec.fmt(t) for t in ts))
        return [t.repeat(2) for t in ts]

    def weights(self, device):
        return self.w

    def count_all(self, n):
        return 2.0 * n


@contextlib.contextmanager
def patched(rec, stats_min=None):
    from vae_gp_ode_amd import _lib
    from vae_gp_ode_amd import vae_ops as V
    lib = _lib.load()
    saved = (_lib.call, V._chk, V._stream, V._ptr, lib.gpode_defer_reductions, V._FUSED_STATS_MIN_IMAGES)
    _lib.call, V._ptr = rec.call, rec.ptr
    V._chk = lambda t, name, shape=None: t.contiguous()
    V._stream = lambda: ctypes.c_void_p(0)
    lib.gpode_defer_reductions = lambda mode: rec.note('gpode_defer_reductions(%d)' % mode)
    if stats_min is not None:
        V._FUSED_STATS_MIN_IMAGES = stats_min
    V.set_bn_sync(None)                              # (an earlier test of the process may have left a group behind)
    try:
        yield V
    finally:
        V.set_bn_sync(None)
        V.set_deferred_reductions(False)
        _lib.call, V._chk, V._stream, V._ptr, lib.gpode_defer_reductions, V._FUSED_STATS_MIN_IMAGES = saved


# ---- the pieces the scenarios are made of -------------------------------------------------------------------------------------------------
def _bn(rec, C, tag='', slot=None, train=True, frozen=False):
    bn = torch.nn.BatchNorm2d(C)
    bn.train(train)
    bn.num_batches_tracked = torch.zeros((), dtype=torch.int64).as_subclass(_OnDevice)
    if slot is not None:
        bn._gpode_slot = slot
    if frozen:
        bn.weight.requires_grad_(False), bn.bias.requires_grad_(False)
    rec.name(**{'gamma' + tag: bn.weight, 'beta' + tag: bn.bias, 'running_mean' + tag: bn.running_mean, 'running_var' + tag: bn.running_var,
                'nbt' + tag: bn.num_batches_tracked})
    return bn


def _leaf(rec, name, *shape, grad=True):
    return rec.name(**{name: torch.zeros(*shape, requires_grad=grad)})


def _n_obs(rec):
    return rec.name(n_obs=torch.tensor([4, 2, 1], dtype=torch.int32))


def _encoder_rows(rec, V, halves, order, reparam=True):
    """[(mu, logvar, z)] per half of the state: the halves of one fc output (the KL partial sums then ride with reparam), or
    separately allocated tensors (the packed route)"""
    out = []
    for k in ('s', 'v')[:order]:
        h = _leaf(rec, 'fc_' + k, N, 2 * Q) * 1.0
        if halves:
            rec.name(**{'h_' + k: h})
            mu, lv = h.chunk(2, dim=1)
        else:
            mu, lv = h[:, :Q].clone(), h[:, Q:].clone()
            rec.name(**{'mu_' + k: mu, 'logvar_' + k: lv})
        z = V.reparam(mu, lv, rec.name(**{'eps_' + k: torch.zeros(N, Q)})) if reparam else None
        out.append((mu, lv, z))
    return out


def elbo_chain(rec, V, route, halves, order):
    X = rec.name(X=torch.zeros(N, T, 1, 28, 28))
    rows = _encoder_rows(rec, V, halves, order)
    if route == 'index':
        index = V.frame_index(_n_obs(rec), T)
        rec.name(index=index.off)
        rec.note('frame_index: P %d, N %d, T %d, counts %s, off %s, src %s'
                 % (index.P, index.N, index.T, index.counts, index.off.tolist(), index.src.tolist()))
        logits = _leaf(rec, 'logits', L * index.P, 1, 28, 28)
        lpart, z = V.sigmoid_loglik_parts(X, logits, L * N, index=index)
    else:
        logits = _leaf(rec, 'logits', L * N * T, 1, 28, 28)
        lpart, z = V.sigmoid_loglik_parts(X, logits, L * N, _n_obs(rec)) if route == 'n_obs' else V.sigmoid_loglik_parts(X, logits, L * N)
    rec.note('parts %s, z %s, z needs a gradient: %s' % (tuple(lpart.shape), tuple(z.shape), z.requires_grad))
    Um, Us = _leaf(rec, 'Um', M, DO), _leaf(rec, 'Us', DO * M * (M + 1) // 2)
    (mu_s, lv_s, z_s), (mu_v, lv_v, z_v) = rows[0], (rows[1] if order == 2 else (None, None, None))
    out = V.elbo_all(lpart, mu_s, lv_s, mu_v, lv_v, Um, Us, M, NOBS)
    rec.note('backward')
    (out[0] + z_s.sum() + (z_v.sum() if order == 2 else 0.0)).backward()
    rec.note('gradients: %s' % ', '.join(k for k, t in (('logits', logits), ('Um', Um), ('Us', Us)) if t.grad is not None))


def parts_alone(rec, V, masked):
    """a consumer other than elbo_all(): the backward of the parts launches for the logit gradients itself"""
    X, logits = rec.name(X=torch.zeros(N, T, 1, 28, 28)), _leaf(rec, 'logits', L * N * T, 1, 28, 28)
    lpart, _ = V.sigmoid_loglik_parts(X, logits, L * N, _n_obs(rec)) if masked else V.sigmoid_loglik_parts(X, logits, L * N)
    rec.note('backward')
    (lpart * rec.name(weights=torch.ones(L * N, 1))).sum().backward()


def rowsum(rec, V, masked):
    X, z = rec.name(X=torch.zeros(N, T, 1, 28, 28)), _leaf(rec, 'z', L * N * T, 1, 28, 28)
    out = V.bernoulli_loglik_rowsum(X, z, L * N, _n_obs(rec)) if masked else V.bernoulli_loglik_rowsum(X, z, L * N)
    rec.note('rows %s; backward' % (tuple(out.shape),))
    out.sum().backward()


def kl_and_terms(rec, V, halves):
    (mu, lv, _), = _encoder_rows(rec, V, halves, 1, reparam=False)
    lhood, kl_u = _leaf(rec, 'lhood', L, N), _leaf(rec, 'kl_u', ())
    out = V.elbo_terms(lhood, V.normal_kl_rows(mu, lv), kl_u, NOBS)
    rec.note('terms %s; backward' % (tuple(out.shape),))
    out[0].backward()


def gather(rec, V):
    index = V.frame_index(_n_obs(rec), T)
    rec.name(index=index.off)
    zt = _leaf(rec, 'ztL', L, N, T, 2 * Q)
    out = V.gather_frames(zt, index, Q)
    rec.note('gathered %s; backward' % (tuple(out.shape),))
    out.sum().backward()
    rec.raises('gather_frames of a ztL with one frame too many', lambda: V.gather_frames(torch.zeros(L, N, T + 1, 2 * Q), index, Q))


def _stub_model(rec, V, order=1):
    """what compute_loss asks of a model: the decoder's logits or images, the encoder rows, the inducing posterior"""
    calls = []
    enc = _encoder_rows(rec, V, True, order)
    field = types.SimpleNamespace(Um=types.SimpleNamespace(optvar=_leaf(rec, 'Um', M, DO)), M=M,
                                  us_packed=lambda Us=_leaf(rec, 'Us', DO * M * (M + 1) // 2): Us)
    decoder = types.SimpleNamespace(distribution='bernoulli')
    decoder.log_prob_rowsum = lambda x, z, L, n_obs=None: (V.bernoulli_loglik_rowsum(x, z, L * N) if n_obs is None
                                                           else V.bernoulli_loglik_rowsum(x, z, L * N, n_obs)).view(L, N)
    encoder = types.SimpleNamespace(kl_rows=lambda ms, ls, mv, lv: V.normal_kl_rows(ms, ls))

    def model(data, L, logits=False, obs_index=None, **grid):
        frames = L * (obs_index.P if obs_index is not None else N * T)
        calls.append('model(logits=%s, obs_index=%s, %s)' % (logits, type(obs_index).__name__, sorted(grid)))
        rec.note(calls[-1])
        return _leaf(rec, 'logits' if logits else 'Xrec', frames, 1, 28, 28), enc[0][:2], (None, None)
    model.flow = types.SimpleNamespace(odefunc=types.SimpleNamespace(diffeq=field), kl=lambda: _leaf(rec, 'kl_u', ()))
    model.vae = types.SimpleNamespace(decoder=decoder, encoder=encoder)
    model.num_observations = NOBS
    return model


def loss(rec, V, route, ragged, fused=True):
    from vae_gp_ode_amd.model import create_model as C
    X, n_obs = rec.name(X=torch.zeros(N, T, 1, 28, 28)), (_n_obs(rec) if ragged else None)
    reached, real = [], {}

    def spy(name):
        def f(*a, **kw):
            what = {'sigmoid_loglik_parts': lambda: (a[3] if len(a) > 3 else kw.get('n_obs'), kw.get('index')),
                    'bernoulli_loglik_rowsum': lambda: (a[3] if len(a) > 3 else kw.get('n_obs'), None),
                    'frame_index': lambda: (a[0], None)}.get(name, lambda: (None, None))()
            reached.append((name, 'n_obs' if what[0] is n_obs and n_obs is not None else what[0], type(what[1]).__name__))
            return real[name](*a, **kw)
        return f
    names = ('sigmoid_loglik_parts', 'bernoulli_loglik_rowsum', 'frame_index', 'elbo_all', 'elbo_terms', 'normal_kl_rows')
    was = C._FUSED_LOSS
    for k in names:
        real[k] = getattr(V, k)
        setattr(V, k, spy(k))
    C._FUSED_LOSS = fused
    try:
        model = _stub_model(rec, V)
        kw = dict(n_obs=n_obs) if ragged else {}
        if route == 'compact':
            kw.update(compact=True, counts=[4, 2, 1])
        out = C.compute_loss(model, X, L, **kw)
        rec.note('%d terms; backward' % len(out))
        out[0].backward()
        if route == 'compact':
            rec.raises('compact without n_obs', lambda: C.compute_loss(model, X, L, compact=True), ValueError)
            C._FUSED_LOSS = False
            rec.raises('compact on the unfused route', lambda: C.compute_loss(model, X, L, n_obs=n_obs, compact=True), ValueError)
    finally:
        C._FUSED_LOSS = was
        for k in names:
            setattr(V, k, real[k])
    rec.note('reached: %s' % reached)


def _sync(rec, V, on):
    V.set_bn_sync(Sync(rec) if on else None)


def bn_train(rec, V, sync, training=True):
    _sync(rec, V, sync)
    bn = _bn(rec, 8, train=training)
    y = V.batch_norm_train(_leaf(rec, 'x', 2, 8, 5, 5), bn, True)
    rec.note('backward')
    y.sum().backward()


def bn_eval(rec, V):
    bn = _bn(rec, 8, train=False, frozen=True)
    y = V.batch_norm_eval(_leaf(rec, 'x', 2, 8, 5, 5), bn, True)
    rec.note('backward')
    y.sum().backward()
    bn.weight.requires_grad_(True)
    rec.raises('backward with a trainable gamma', lambda: V.batch_norm_eval(_leaf(rec, 'x2', 2, 8, 5, 5), bn, False).sum().backward())
    rec.raises('bn_eval_table in training mode', lambda: V.bn_eval_table(bn.train()))
    plain = torch.nn.BatchNorm2d(8)
    rec.raises('batch_norm_train with a host counter', lambda: V.batch_norm_train(torch.zeros(2, 8, 5, 5), plain, True))


def bn_pair(rec, V):
    _sync(rec, V, True)
    y1, y2 = V.batch_norm_train_pair(_leaf(rec, 'x1', 2, 8, 5, 5), _bn(rec, 8, '1'), _leaf(rec, 'x2', 2, 4, 3, 3), _bn(rec, 4, '2'), True)
    rec.note('backward')
    (y1.sum() + y2.sum()).backward()


def conv(rec, V, then_bn):
    x, w, b = _leaf(rec, 'x', 2, 3, 8, 8), _leaf(rec, 'w', 4, 3, 3, 3), _leaf(rec, 'b', 4)
    y = V.conv2d(x, w, b, 2, 1)
    if then_bn:                                      # the bias gradient then arrives with the BatchNorm backward's channel sums
        y = V.batch_norm_train(y, _bn(rec, 4), True)
    rec.note('y %s; backward' % (tuple(y.shape),))
    before = V.fused_bias_grads
    y.sum().backward()
    rec.note('bias gradients taken from a BatchNorm backward: %d' % (V.fused_bias_grads - before))


def convT(rec, V, stats):
    """decnn.1 -> BatchNorm -> decnn.4 (vae.py:107-120); ``stats``: decnn.1 sums the BatchNorm's statistics"""
    h, w1, b1 = _leaf(rec, 'h', 2, 32, 4, 4), _leaf(rec, 'w1', 32, 64, 3, 3), _leaf(rec, 'b1', 64)
    w4, b4 = _leaf(rec, 'w4', 64, 32, 5, 5), _leaf(rec, 'b4', 32)
    bn = _bn(rec, 64, slot=7)
    c = V.conv_transpose2d(h, w1, b1, 1, 0, stats_for=bn if stats else None)
    rec.note('c %s carries statistics: %s' % (tuple(c.shape), hasattr(c, '_gpode_bnstats')))
    y = V.bn_relu_conv_transpose2d(c, bn, w4, b4, 2, 1)
    rec.note('y %s; backward' % (tuple(y.shape),))
    y.sum().backward()


def stage4(rec, V, sync):
    _sync(rec, V, sync)
    c, w, b = _leaf(rec, 'c', 2, 64, 6, 6), _leaf(rec, 'w', 64, 32, 5, 5), _leaf(rec, 'b', 32)
    y = V.bn_relu_conv_transpose2d(c, _bn(rec, 64), w, b, 2, 1)
    rec.note('y %s; backward' % (tuple(y.shape),))
    y.sum().backward()


def last_stage(rec, V, sync, wgrad=True, bias=True, misaligned=False, deferred=False):
    _sync(rec, V, sync)
    if misaligned:
        c = rec.name(c=torch.zeros(2 * 16 * 784 + 1))[1:].view(2, 16, 28, 28).requires_grad_(True)
    else:
        c = _leaf(rec, 'c', 2, 16, 28, 28)
    w, b = _leaf(rec, 'w', 16, 1, 5, 5, grad=wgrad), (_leaf(rec, 'b', 1, grad=wgrad) if bias else None)
    y = V.bn_relu_conv_transpose2d(c, _bn(rec, 16), w, b, 1, 2)
    rec.note('y %s; backward' % (tuple(y.shape),))
    if deferred:
        V.set_deferred_reductions(True)
    y.sum().backward()
    if deferred:
        rec.note('kept until the flush: %d, queued: %s' % (len(V._deferred['keep']), V._deferred['queued']))


def deferred_encoder(rec, V):
    """set_deferred_reductions(True): the first reducing backward call of a pass drops leftovers and queues the flush (2), the
    later ones record (1), each is closed (0), and one gpode_flush_reductions ends the pass"""
    x, w, b = _leaf(rec, 'x', 2, 3, 8, 8), _leaf(rec, 'w', 4, 3, 3, 3), _leaf(rec, 'b', 4)
    fw, fb = _leaf(rec, 'fw', 5, 64), _leaf(rec, 'fb', 5)
    y = V.linear(V.batch_norm_train(V.conv2d(x, w, b, 2, 1), _bn(rec, 4), True).flatten(1), fw, fb)
    V.set_deferred_reductions(True)
    rec.note('backward')
    y.sum().backward()
    rec.note('kept until the flush: %d, queued: %s' % (len(V._deferred['keep']), V._deferred['queued']))
    V.set_deferred_reductions(False)
    rec.note('backward, switch off')
    V.conv2d(x, w, b, 2, 1).sum().backward()


def dense(rec, V):
    y = V.linear(_leaf(rec, 'x', 3, 4), _leaf(rec, 'w', 5, 4), _leaf(rec, 'b', 5))
    rec.note('backward')
    y.sum().backward()
    rec.note('linear_relu_in, wide')
    y = V.linear_relu_in(_leaf(rec, 'xw', 3, 128), _leaf(rec, 'ww', 5, 128), _leaf(rec, 'bw', 5))
    y.sum().backward()
    rec.note('linear_relu_in, narrow')
    y = V.linear_relu_in(_leaf(rec, 'xn', 3, 8), _leaf(rec, 'wn', 5, 8), None)
    y.sum().backward()


def predict(rec, V):
    Th = T + 1
    F = N * Th
    c, table = rec.name(c=torch.zeros(F, 16, 28, 28)), rec.name(table=torch.zeros(16, 4))
    w, b, X, n_obs = rec.name(w=torch.zeros(16, 1, 5, 5)), rec.name(b=torch.zeros(1)), rec.name(X=torch.zeros(N, T, 1, 28, 28)), _n_obs(rec)
    for loglik in (0, 2):
        for masked in (False, True):
            st = V.PredictState(F, 'cpu', loglik=loglik)
            tag = '%d%d' % (loglik, masked)
            rec.name(**{'mean' + tag: st.mean, 'm2' + tag: st.m2, 'se' + tag: st.se})
            if loglik:
                rec.name(**{'ell' + tag: st.ell})
            for bias in (b, None):
                assert V.dec10_predict(c, table, w, bias, X, Th, st, n_obs if masked else None) is st
            rec.note('draws folded in: %d' % st.done)
    st = V.PredictState(F, 'cpu', variance=False)
    V.dec10_predict(torch.zeros(2 * F, 16, 28, 28), table, w, b, X, Th, st)
    rec.note('two draws, no variance: done %d' % st.done)
    rec.raises('c of 8 channels', lambda: V.dec10_predict(torch.zeros(F, 8, 28, 28), table, w, b, X, Th, st))
    rec.raises('a table of 8 channels', lambda: V.dec10_predict(c, torch.zeros(8, 4), w, b, X, Th, st))
    rec.raises('c not a whole number of draws', lambda: V.dec10_predict(torch.zeros(F + 1, 16, 28, 28), table, w, b, X, Th, st))
    rec.raises('F that is not N Th', lambda: V.dec10_predict(c, table, w, b, X, Th + 1, st))
    rec.raises('targets of another size', lambda: V.dec10_predict(c, table, w, b, torch.zeros(N, T, 1, 14, 14), Th, st))
    st = V.PredictState(F, 'cpu', loglik=2)
    st.ell = torch.zeros(2, F + 1)
    rec.raises('ell of the wrong width', lambda: V.dec10_predict(c, table, w, b, X, Th, st))
    rec.raises('n_obs int64', lambda: V.dec10_predict(c, table, w, b, X, Th, st, n_obs.long()))
    rec.note('table_conv_transpose2d')
    c4, w4 = rec.name(c4=torch.zeros(2, 64, 6, 6)), rec.name(w4=torch.zeros(64, 32, 5, 5))
    t4 = rec.name(t4=torch.zeros(64, 4))
    for bias in (rec.name(b4=torch.zeros(32)), None):
        y = V.table_conv_transpose2d(c4, t4, w4, bias, 2, 1, 1)
        rec.note('y %s' % (tuple(y.shape),))
    rec.raises('a table of 16 channels', lambda: V.table_conv_transpose2d(c4, table, w4, None, 2, 1))


def refusals(rec, V):
    X, a, n_obs = torch.zeros(N, T, 1, 28, 28), torch.zeros(L * N * T, 1, 28, 28), torch.tensor([4, 2, 1], dtype=torch.int32)
    index = V.frame_index(n_obs, T)
    for who, fn in (('sigmoid_loglik_parts', V.sigmoid_loglik_parts), ('bernoulli_loglik_rowsum', V.bernoulli_loglik_rowsum)):
        rec.raises('%s, n_obs int64' % who, lambda: fn(X, a, L * N, n_obs.long()))
        rec.raises('%s, n_obs a list' % who, lambda: fn(X, a, L * N, [4, 2, 1]))
        rec.raises('%s, n_obs (N + 1,)' % who, lambda: fn(X, a, L * N, torch.zeros(N + 1, dtype=torch.int32)))
        rec.raises('%s, n_obs (N, 1)' % who, lambda: fn(X, a, L * N, n_obs.view(N, 1)))
        rec.raises('%s, n_obs on another device' % who, lambda: fn(X, a, L * N, torch.zeros(N, dtype=torch.int32, device='meta')))
        rec.raises('%s, X without a frame axis' % who, lambda: fn(torch.zeros(N), torch.zeros(N), N, n_obs))
    compact = torch.zeros(L * index.P, 1, 28, 28)
    rec.raises('n_obs together with index', lambda: V.sigmoid_loglik_parts(X, compact, L * N, n_obs, index=index))
    rec.raises('padded logits with index', lambda: V.sigmoid_loglik_parts(X, a, L * N, index=index))
    rec.raises('index of another minibatch', lambda: V.sigmoid_loglik_parts(torch.zeros(N, T + 1, 1, 28, 28), compact, L * N, index=index))
    rec.raises('rows no multiple of N', lambda: V.sigmoid_loglik_parts(X, compact, L * N + 1, index=index))
    rec.raises('frame_index, nothing observed', lambda: V.frame_index(torch.zeros(N, dtype=torch.int32), T))
    rec.raises('frame_index, n_obs (N, 1)', lambda: V.frame_index(n_obs.view(N, 1), T))
    rec.raises('frame_index, counts of another length', lambda: V.frame_index(n_obs, T, counts=[4, 2]))
    clamped = V.frame_index(None, T, counts=[9, -3, 2])
    rec.note('frame_index from host counts [9, -3, 2]: P %d, counts %s, off %s, src %s'
             % (clamped.P, clamped.counts, clamped.off.tolist(), clamped.src.tolist()))


SCENARIOS = {'bn_eval': bn_eval, 'bn_pair': bn_pair, 'gather_frames': gather, 'dense': dense, 'predict': predict, 'refusals': refusals,
             'deferred_encoder': deferred_encoder}
for _route in ('plain', 'n_obs', 'index'):
    for _halves in (True, False):
        for _order in (1, 2):
            SCENARIOS['elbo_%s_%s_order%d' % (_route, 'halves' if _halves else 'packed', _order)] = (
                lambda rec, V, a=_route, b=_halves, c=_order: elbo_chain(rec, V, a, b, c))
for _flag in (False, True):
    SCENARIOS['rowsum' + '_n_obs' * _flag] = lambda rec, V, a=_flag: rowsum(rec, V, a)
    SCENARIOS['parts_alone' + '_n_obs' * _flag] = lambda rec, V, a=_flag: parts_alone(rec, V, a)
    SCENARIOS['kl_and_terms_' + ('halves' if _flag else 'packed')] = lambda rec, V, a=_flag: kl_and_terms(rec, V, a)
    SCENARIOS['loss_fused' + '_n_obs' * _flag] = lambda rec, V, a=_flag: loss(rec, V, 'fused', a)
    SCENARIOS['loss_unfused' + '_n_obs' * _flag] = lambda rec, V, a=_flag: loss(rec, V, 'unfused', a, fused=False)
    SCENARIOS['bn_train' + '_sync' * _flag] = lambda rec, V, a=_flag: bn_train(rec, V, a)
    SCENARIOS['bn_train_frozen_statistics' + '_sync' * _flag] = lambda rec, V, a=_flag: bn_train(rec, V, a, training=False)
    SCENARIOS['conv2d' + '_then_bn' * _flag] = lambda rec, V, a=_flag: conv(rec, V, a)
    SCENARIOS['convT' + '_stats' * _flag] = lambda rec, V, a=_flag: convT(rec, V, a)
    SCENARIOS['stage4' + '_sync' * _flag] = lambda rec, V, a=_flag: stage4(rec, V, a)
    SCENARIOS['last_stage_misaligned' + '_sync' * _flag] = lambda rec, V, a=_flag: last_stage(rec, V, a, misaligned=True)
    SCENARIOS['last_stage_deferred' + '_sync' * _flag] = lambda rec, V, a=_flag: last_stage(rec, V, a, deferred=True)
    for _wgrad in (True, False):
        for _bias in (True, False):
            SCENARIOS['last_stage%s%s%s' % ('_sync' * _flag, '_frozen' * (not _wgrad), '_nobias' * (not _bias))] = (
                lambda rec, V, a=_flag, b=_wgrad, c=_bias: last_stage(rec, V, a, wgrad=b, bias=c))
SCENARIOS['loss_compact'] = lambda rec, V: loss(rec, V, 'compact', True)


def transcript(name):
    rec = Recorder()
    with patched(rec, stats_min=2) as V:
        SCENARIOS[name](rec, V)
    return rec.lines


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_transcript(name):
    got = transcript(name)
    want = EXPECTED[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, '%s, line %d' % (name, i)
    assert len(got) == len(want), (name, got[len(want):], want[len(got):])


def test_every_route_of_the_issue_is_in_the_transcripts():
    """the transcripts reach every entry point of the VAE and loss stage these wrappers can call (a route nobody drives is not pinned)"""
    seen = {line.split('(')[0] for lines in EXPECTED.values() for line in lines if line.startswith('gpode_')}
    for name in ('gpode_sigmoid_loglik_fwd', 'gpode_sigmoid_loglik_fwd_len', 'gpode_sigmoid_loglik_fwd_pk', 'gpode_sigmoid_loglik_bwd',
                 'gpode_sigmoid_loglik_bwd_len', 'gpode_sigmoid_loglik_bwd_pk', 'gpode_loglik_rowsum_fwd', 'gpode_loglik_rowsum_fwd_len',
                 'gpode_loglik_rowsum_bwd', 'gpode_loglik_rowsum_bwd_len', 'gpode_elbo_all_fwd', 'gpode_elbo_all_fwd_kl', 'gpode_elbo_all_bwd',
                 'gpode_elbo_all_bwd_ll', 'gpode_elbo_all_bwd_ll_len', 'gpode_elbo_all_bwd_ll_kl', 'gpode_elbo_all_bwd_ll_kl_len',
                 'gpode_elbo_fwd', 'gpode_elbo_bwd', 'gpode_normal_kl_fwd', 'gpode_normal_kl_bwd', 'gpode_reparam_fwd', 'gpode_reparam_bwd',
                 'gpode_reparam_kl_fwd', 'gpode_reparam_kl_bwd', 'gpode_gather_frames_fwd', 'gpode_gather_frames_bwd', 'gpode_bn_fwd',
                 'gpode_bn_bwd', 'gpode_bn_eval', 'gpode_bn_moments', 'gpode_bn_finalize', 'gpode_bn_apply', 'gpode_bn_bwd_sums',
                 'gpode_bn_bwd_apply', 'gpode_bn_stats', 'gpode_conv2d_fwd', 'gpode_conv2d_bwd_data', 'gpode_conv2d_bwd_weight',
                 'gpode_conv2d_bwd_data_bn', 'gpode_conv2d_bwd_weight_bn', 'gpode_convT_fwd_stats', 'gpode_chan_sum',
                 'gpode_dec10_bn_bwd_sums', 'gpode_dec10_bn_bwd_sums_wgrad', 'gpode_dec10_bn_bwd_apply', 'gpode_flush_reductions',
                 'gpode_defer_reductions', 'gpode_linear_fwd', 'gpode_linear_bwd', 'gpode_linear_relu_fwd', 'gpode_linear_relu_bwd',
                 'gpode_act_fwd', 'gpode_act_bwd', 'gpode_dec10_predict', 'gpode_dec10_predict_len', 'gpode_dec10_predict_ll',
                 'gpode_dec10_predict_ll_len'):
        assert name in seen, name


EXPECTED = {
    'bn_eval': [
        'gpode_bn_eval(x, 0, gamma, beta, running_mean, running_var, 1e-05, new#0, 2, 8, 25, 1, 0)',
        'backward',
        'gpode_bn_eval(x, new#1, gamma, beta, running_mean, running_var, 1e-05, new#2, 2, 8, 25, 1, 0)',
        'gpode_bn_eval(x2, 0, gamma, beta, running_mean, running_var, 1e-05, new#3, 2, 8, 25, 0, 0)',
        'backward with a trainable gamma -> GpodeError: eval-mode BatchNorm is built for frozen layers (main.py:160-161 sets requires_grad=False)',
        'bn_eval_table in training mode -> GpodeError: bn_eval_table: the BatchNorm module is in training mode (its batch statistics are not a table of constants)',
        'batch_norm_train with a host counter -> GpodeError: num_batches_tracked must be an int64 CUDA/HIP scalar',
    ],
    'bn_pair': [
        'gpode_bn_moments(x1, new#0, 2, 8, 25, new#1, 0)',
        'gpode_bn_moments(x2, new#2, 2, 4, 9, new#3, 0)',
        'sync.gather_many(new#0, new#2)',
        'gpode_bn_finalize(new#4, 2, gamma1, beta1, new#5, new#6, running_mean1, running_var1, nbt1, 0.1, 1e-05, new#7, 8, 0)',
        'gpode_bn_apply(x1, new#7, new#8, 2, 8, 25, 1, 0)',
        'gpode_bn_finalize(new#9, 2, gamma2, beta2, new#10, new#11, running_mean2, running_var2, nbt2, 0.1, 1e-05, new#12, 4, 0)',
        'gpode_bn_apply(x2, new#12, new#13, 2, 4, 9, 1, 0)',
        'backward',
        'gpode_bn_bwd_sums(x1, new#14, gamma1, beta1, new#5, new#6, new#15, 2, 8, 25, 1, new#16, 0)',
        'gpode_bn_bwd_sums(x2, new#17, gamma2, beta2, new#10, new#11, new#18, 2, 4, 9, 1, new#19, 0)',
        'sync.gather_many(new#15, new#18)',
        'gpode_bn_bwd_apply(x1, new#14, gamma1, beta1, new#5, new#6, new#20, sync_weights, 2, 100, new#21, new#22, new#23, new#24, 2, 8, 25, 1, new#16, 0)',
        'gpode_bn_bwd_apply(x2, new#17, gamma2, beta2, new#10, new#11, new#25, sync_weights, 2, 36, new#26, new#27, new#28, new#29, 2, 4, 9, 1, new#19, 0)',
    ],
    'bn_train': [
        'gpode_bn_fwd(x, gamma, beta, new#0, new#1, new#2, running_mean, running_var, nbt, 0.1, 1e-05, 2, 8, 25, 1, new#3, 0)',
        'backward',
        'gpode_bn_bwd(x, new#4, gamma, beta, new#1, new#2, new#5, new#6, new#7, new#8, 2, 8, 25, 1, new#9, 0)',
    ],
    'bn_train_frozen_statistics': [
        'gpode_bn_fwd(x, gamma, beta, new#0, new#1, new#2, 0, 0, 0, 0.1, 1e-05, 2, 8, 25, 1, new#3, 0)',
        'backward',
        'gpode_bn_bwd(x, new#4, gamma, beta, new#1, new#2, new#5, new#6, new#7, new#8, 2, 8, 25, 1, new#9, 0)',
    ],
    'bn_train_frozen_statistics_sync': [
        'gpode_bn_moments(x, new#0, 2, 8, 25, new#1, 0)',
        'sync.gather(new#0)',
        'gpode_bn_finalize(new#2, 2, gamma, beta, new#3, new#4, 0, 0, 0, 0.1, 1e-05, new#5, 8, 0)',
        'gpode_bn_apply(x, new#5, new#6, 2, 8, 25, 1, 0)',
        'backward',
        'gpode_bn_bwd_sums(x, new#7, gamma, beta, new#3, new#4, new#8, 2, 8, 25, 1, new#9, 0)',
        'sync.gather(new#8)',
        'gpode_bn_bwd_apply(x, new#7, gamma, beta, new#3, new#4, new#10, sync_weights, 2, 100, new#11, new#12, new#13, new#14, 2, 8, 25, 1, new#9, 0)',
    ],
    'bn_train_sync': [
        'gpode_bn_moments(x, new#0, 2, 8, 25, new#1, 0)',
        'sync.gather(new#0)',
        'gpode_bn_finalize(new#2, 2, gamma, beta, new#3, new#4, running_mean, running_var, nbt, 0.1, 1e-05, new#5, 8, 0)',
        'gpode_bn_apply(x, new#5, new#6, 2, 8, 25, 1, 0)',
        'backward',
        'gpode_bn_bwd_sums(x, new#7, gamma, beta, new#3, new#4, new#8, 2, 8, 25, 1, new#9, 0)',
        'sync.gather(new#8)',
        'gpode_bn_bwd_apply(x, new#7, gamma, beta, new#3, new#4, new#10, sync_weights, 2, 100, new#11, new#12, new#13, new#14, 2, 8, 25, 1, new#9, 0)',
    ],
    'conv2d': [
        'gpode_conv2d_fwd(x, w, b, new#0, 2, 3, 8, 8, 4, 3, 2, 1, 4, 4, 0)',
        'y (2, 4, 4, 4); backward',
        'gpode_conv2d_bwd_data(new#1, w, 0, new#2, 2, 3, 8, 8, 4, 3, 2, 1, 4, 4, 0)',
        'gpode_conv2d_bwd_weight(x, new#1, new#3, new#4, new#5, 2, 3, 8, 8, 4, 3, 2, 1, 4, 4, 0)',
        'bias gradients taken from a BatchNorm backward: 0',
    ],
    'conv2d_then_bn': [
        'gpode_conv2d_fwd(x, w, b, new#0, 2, 3, 8, 8, 4, 3, 2, 1, 4, 4, 0)',
        'gpode_bn_fwd(new#0, gamma, beta, new#1, new#2, new#3, running_mean, running_var, nbt, 0.1, 1e-05, 2, 4, 16, 1, new#4, 0)',
        'y (2, 4, 4, 4); backward',
        'gpode_bn_bwd(new#0, new#5, gamma, beta, new#2, new#3, new#6, new#7, new#8, new#9, 2, 4, 16, 1, new#10, 0)',
        'gpode_conv2d_bwd_data(new#6, w, 0, new#11, 2, 3, 8, 8, 4, 3, 2, 1, 4, 4, 0)',
        'gpode_conv2d_bwd_weight(x, new#6, new#12, 0, new#13, 2, 3, 8, 8, 4, 3, 2, 1, 4, 4, 0)',
        'bias gradients taken from a BatchNorm backward: 1',
    ],
    'convT': [
        'gpode_conv2d_bwd_data(h, w1, b1, new#0, 2, 64, 6, 6, 32, 3, 1, 0, 4, 4, 0)',
        'c (2, 64, 6, 6) carries statistics: False',
        'gpode_bn_stats(new#0, gamma, beta, new#1, new#2, running_mean, running_var, nbt, 0.1, 1e-05, new#3, 2, 64, 36, new#4, 0)',
        'gpode_conv2d_bwd_data_bn(new#0, new#3, w4, b4, new#5, 2, 32, 13, 13, 64, 5, 2, 1, 6, 6, 0)',
        'y (2, 32, 13, 13); backward',
        'gpode_conv2d_bwd_weight_bn(new#6, new#0, new#3, new#7, 0, new#8, 2, 32, 13, 13, 64, 5, 2, 1, 6, 6, 0)',
        'gpode_chan_sum(new#6, new#9, 2, 32, 169, new#10, 0)',
        'gpode_conv2d_fwd(new#6, w4, 0, new#11, 2, 32, 13, 13, 64, 5, 2, 1, 6, 6, 0)',
        'gpode_bn_bwd(new#0, new#11, gamma, beta, new#1, new#2, new#12, new#13, new#14, new#15, 2, 64, 36, 1, new#16, 0)',
        'gpode_conv2d_fwd(new#12, w1, 0, new#17, 2, 64, 6, 6, 32, 3, 1, 0, 4, 4, 0)',
        'gpode_conv2d_bwd_weight(new#12, h, new#18, 0, new#19, 2, 64, 6, 6, 32, 3, 1, 0, 4, 4, 0)',
    ],
    'convT_stats': [
        'gpode_convT_fwd_stats(h, 0, w1, b1, new#0, 2, 64, 6, 6, 32, 3, 1, 0, 4, 4, gamma, beta, new#1, new#2, running_mean, running_var, nbt, 0.1, 1e-05, new#3, new#4, 7, 0)',
        'c (2, 64, 6, 6) carries statistics: True',
        'gpode_conv2d_bwd_data_bn(new#0, new#3, w4, b4, new#5, 2, 32, 13, 13, 64, 5, 2, 1, 6, 6, 0)',
        'y (2, 32, 13, 13); backward',
        'gpode_conv2d_bwd_weight_bn(new#6, new#0, new#3, new#7, 0, new#8, 2, 32, 13, 13, 64, 5, 2, 1, 6, 6, 0)',
        'gpode_chan_sum(new#6, new#9, 2, 32, 169, new#10, 0)',
        'gpode_conv2d_fwd(new#6, w4, 0, new#11, 2, 32, 13, 13, 64, 5, 2, 1, 6, 6, 0)',
        'gpode_bn_bwd(new#0, new#11, gamma, beta, new#1, new#2, new#12, new#13, new#14, new#15, 2, 64, 36, 1, new#16, 0)',
        'gpode_conv2d_fwd(new#12, w1, 0, new#17, 2, 64, 6, 6, 32, 3, 1, 0, 4, 4, 0)',
        'gpode_conv2d_bwd_weight(new#12, h, new#18, 0, new#19, 2, 64, 6, 6, 32, 3, 1, 0, 4, 4, 0)',
    ],
    'deferred_encoder': [
        'gpode_conv2d_fwd(x, w, b, new#0, 2, 3, 8, 8, 4, 3, 2, 1, 4, 4, 0)',
        'gpode_bn_fwd(new#0, gamma, beta, new#1, new#2, new#3, running_mean, running_var, nbt, 0.1, 1e-05, 2, 4, 16, 1, new#4, 0)',
        'gpode_linear_fwd(new#1, fw, fb, new#5, 2, 64, 5, 0)',
        'backward',
        'gpode_defer_reductions(2)',
        'gpode_linear_bwd(new#1, fw, new#6, new#7, new#8, new#9, 2, 64, 5, 0, 0)',
        'gpode_defer_reductions(0)',
        'gpode_defer_reductions(1)',
        'gpode_bn_bwd(new#0, new#7, gamma, beta, new#2, new#3, new#10, new#11, new#12, new#13, 2, 4, 16, 1, new#14, 0)',
        'gpode_defer_reductions(0)',
        'gpode_conv2d_bwd_data(new#10, w, 0, new#15, 2, 3, 8, 8, 4, 3, 2, 1, 4, 4, 0)',
        'gpode_defer_reductions(1)',
        'gpode_conv2d_bwd_weight(x, new#10, new#16, 0, new#17, 2, 3, 8, 8, 4, 3, 2, 1, 4, 4, 0)',
        'gpode_defer_reductions(0)',
        'gpode_flush_reductions(0)',
        'kept until the flush: 0, queued: False',
        'backward, switch off',
        'gpode_conv2d_fwd(x, w, b, new#18, 2, 3, 8, 8, 4, 3, 2, 1, 4, 4, 0)',
        'gpode_conv2d_bwd_data(new#19, w, 0, new#20, 2, 3, 8, 8, 4, 3, 2, 1, 4, 4, 0)',
        'gpode_conv2d_bwd_weight(x, new#19, new#21, new#22, new#23, 2, 3, 8, 8, 4, 3, 2, 1, 4, 4, 0)',
    ],
    'dense': [
        'gpode_linear_fwd(x, w, b, new#0, 3, 4, 5, 0)',
        'backward',
        'gpode_linear_bwd(x, w, new#1, new#2, new#3, new#4, 3, 4, 5, 0, 0)',
        'linear_relu_in, wide',
        'gpode_linear_relu_fwd(xw, ww, bw, new#5, 3, 128, 5, 0)',
        'gpode_linear_relu_bwd(xw, ww, new#6, new#7, new#8, new#9, 3, 128, 5, 0)',
        'linear_relu_in, narrow',
        'gpode_act_fwd(xn, new#10, 24, 0, 0)',
        'gpode_linear_fwd(new#10, wn, 0, new#11, 3, 8, 5, 0)',
        'gpode_linear_bwd(new#10, wn, new#12, new#13, new#14, 0, 3, 8, 5, 0, 0)',
        'gpode_act_bwd(new#10, new#13, new#15, 24, 0, 0)',
    ],
    'elbo_index_halves_order1': [
        'gpode_reparam_kl_fwd(h_s, h_s+8, 4, eps_s, new#0, new#1, 3, 2, 0)',
        'frame_index: P 7, N 3, T 4, counts [4, 2, 1], off [0, 4, 6, 7], src [0, 1, 2, 3, 4, 5, 8]',
        'gpode_sigmoid_loglik_fwd_pk(X, logits, new#2, new#3, 6, index, 4, 784, 9408, 4, 0)',
        'parts (6, 4), z (14, 1, 28, 28), z needs a gradient: False',
        'gpode_elbo_all_fwd(new#3, 6, 24, h_s, 0, 3, 2, 5, 2, Um, Us, 360, new#4, 0)',
        'backward',
        'gpode_elbo_all_bwd(new#5, 0, 0, 0, 6, h_s, 0, 3, 2, 5, 2, Um, Us, 360, new#6, new#7, 0, new#8, new#9, 0)',
        'gpode_sigmoid_loglik_bwd_pk(X, new#2, new#6, new#10, 6, index+16, 7, 4, 784, 9408, 0)',
        'gpode_reparam_kl_bwd(new#11, 0, h_s, h_s+8, 4, eps_s, new#12, new#12+8, 4, 3, 2, 0)',
        'gradients: logits, Um, Us',
    ],
    'elbo_index_halves_order2': [
        'gpode_reparam_kl_fwd(h_s, h_s+8, 4, eps_s, new#0, new#1, 3, 2, 0)',
        'gpode_reparam_kl_fwd(h_v, h_v+8, 4, eps_v, new#2, new#3, 3, 2, 0)',
        'frame_index: P 7, N 3, T 4, counts [4, 2, 1], off [0, 4, 6, 7], src [0, 1, 2, 3, 4, 5, 8]',
        'gpode_sigmoid_loglik_fwd_pk(X, logits, new#4, new#5, 6, index, 4, 784, 9408, 4, 0)',
        'parts (6, 4), z (14, 1, 28, 28), z needs a gradient: False',
        'gpode_elbo_all_fwd(new#5, 6, 24, h_s, h_v, 3, 2, 5, 2, Um, Us, 360, new#6, 0)',
        'backward',
        'gpode_elbo_all_bwd(new#7, 0, 0, 0, 6, h_s, h_v, 3, 2, 5, 2, Um, Us, 360, new#8, new#9, new#10, new#11, new#12, 0)',
        'gpode_sigmoid_loglik_bwd_pk(X, new#4, new#8, new#13, 6, index+16, 7, 4, 784, 9408, 0)',
        'gpode_reparam_kl_bwd(new#14, 0, h_v, h_v+8, 4, eps_v, new#15, new#15+8, 4, 3, 2, 0)',
        'gpode_reparam_kl_bwd(new#16, 0, h_s, h_s+8, 4, eps_s, new#17, new#17+8, 4, 3, 2, 0)',
        'gradients: logits, Um, Us',
    ],
    'elbo_index_packed_order1': [
        'gpode_reparam_fwd(new#0, new#0+8, 4, eps_s, new#1, 3, 2, 0)',
        'frame_index: P 7, N 3, T 4, counts [4, 2, 1], off [0, 4, 6, 7], src [0, 1, 2, 3, 4, 5, 8]',
        'gpode_sigmoid_loglik_fwd_pk(X, logits, new#2, new#3, 6, index, 4, 784, 9408, 4, 0)',
        'parts (6, 4), z (14, 1, 28, 28), z needs a gradient: False',
        'gpode_elbo_all_fwd(new#3, 6, 24, new#4, 0, 3, 2, 5, 2, Um, Us, 360, new#5, 0)',
        'backward',
        'gpode_elbo_all_bwd(new#6, 0, 0, 0, 6, new#4, 0, 3, 2, 5, 2, Um, Us, 360, new#7, new#8, 0, new#9, new#10, 0)',
        'gpode_sigmoid_loglik_bwd_pk(X, new#2, new#7, new#11, 6, index+16, 7, 4, 784, 9408, 0)',
        'gpode_reparam_bwd(new#12, new#0+8, 4, eps_s, new#13, new#13+8, 4, 3, 2, 0)',
        'gradients: logits, Um, Us',
    ],
    'elbo_index_packed_order2': [
        'gpode_reparam_fwd(new#0, new#0+8, 4, eps_s, new#1, 3, 2, 0)',
        'gpode_reparam_fwd(new#2, new#2+8, 4, eps_v, new#3, 3, 2, 0)',
        'frame_index: P 7, N 3, T 4, counts [4, 2, 1], off [0, 4, 6, 7], src [0, 1, 2, 3, 4, 5, 8]',
        'gpode_sigmoid_loglik_fwd_pk(X, logits, new#4, new#5, 6, index, 4, 784, 9408, 4, 0)',
        'parts (6, 4), z (14, 1, 28, 28), z needs a gradient: False',
        'gpode_elbo_all_fwd(new#5, 6, 24, new#6, new#7, 3, 2, 5, 2, Um, Us, 360, new#8, 0)',
        'backward',
        'gpode_elbo_all_bwd(new#9, 0, 0, 0, 6, new#6, new#7, 3, 2, 5, 2, Um, Us, 360, new#10, new#11, new#12, new#13, new#14, 0)',
        'gpode_sigmoid_loglik_bwd_pk(X, new#4, new#10, new#15, 6, index+16, 7, 4, 784, 9408, 0)',
        'gpode_reparam_bwd(new#16, new#2+8, 4, eps_v, new#17, new#17+8, 4, 3, 2, 0)',
        'gpode_reparam_bwd(new#18, new#0+8, 4, eps_s, new#19, new#19+8, 4, 3, 2, 0)',
        'gradients: logits, Um, Us',
    ],
    'elbo_n_obs_halves_order1': [
        'gpode_reparam_kl_fwd(h_s, h_s+8, 4, eps_s, new#0, new#1, 3, 2, 0)',
        'gpode_sigmoid_loglik_fwd_len(X, logits, new#2, new#3, 6, 3136, 9408, 4, n_obs, 4, 784, 0)',
        'parts (6, 4), z (24, 1, 28, 28), z needs a gradient: False',
        'gpode_elbo_all_fwd_kl(new#3, 6, 24, new#1, 1, 0, 0, 3, 5, 2, Um, Us, 360, new#4, 0)',
        'backward',
        'gpode_elbo_all_bwd_ll_kl_len(new#5, 0, 0, 0, 6, 3, 5, 2, Um, Us, 360, new#6, new#7, 1, 0, 0, new#8, new#9, X, new#2, new#10, 18816, 9408, n_obs, 4, 784, 0)',
        'gpode_reparam_kl_bwd(new#11, new#7, h_s, h_s+8, 4, eps_s, new#12, new#12+8, 4, 3, 2, 0)',
        'gradients: logits, Um, Us',
    ],
    'elbo_n_obs_halves_order2': [
        'gpode_reparam_kl_fwd(h_s, h_s+8, 4, eps_s, new#0, new#1, 3, 2, 0)',
        'gpode_reparam_kl_fwd(h_v, h_v+8, 4, eps_v, new#2, new#3, 3, 2, 0)',
        'gpode_sigmoid_loglik_fwd_len(X, logits, new#4, new#5, 6, 3136, 9408, 4, n_obs, 4, 784, 0)',
        'parts (6, 4), z (24, 1, 28, 28), z needs a gradient: False',
        'gpode_elbo_all_fwd_kl(new#5, 6, 24, new#1, 1, new#3, 1, 3, 5, 2, Um, Us, 360, new#6, 0)',
        'backward',
        'gpode_elbo_all_bwd_ll_kl_len(new#7, 0, 0, 0, 6, 3, 5, 2, Um, Us, 360, new#8, new#9, 1, new#10, 1, new#11, new#12, X, new#4, new#13, 18816, 9408, n_obs, 4, 784, 0)',
        'gpode_reparam_kl_bwd(new#14, new#10, h_v, h_v+8, 4, eps_v, new#15, new#15+8, 4, 3, 2, 0)',
        'gpode_reparam_kl_bwd(new#16, new#9, h_s, h_s+8, 4, eps_s, new#17, new#17+8, 4, 3, 2, 0)',
        'gradients: logits, Um, Us',
    ],
    'elbo_n_obs_packed_order1': [
        'gpode_reparam_fwd(new#0, new#0+8, 4, eps_s, new#1, 3, 2, 0)',
        'gpode_sigmoid_loglik_fwd_len(X, logits, new#2, new#3, 6, 3136, 9408, 4, n_obs, 4, 784, 0)',
        'parts (6, 4), z (24, 1, 28, 28), z needs a gradient: False',
        'gpode_elbo_all_fwd(new#3, 6, 24, new#4, 0, 3, 2, 5, 2, Um, Us, 360, new#5, 0)',
        'backward',
        'gpode_elbo_all_bwd_ll_len(new#6, 0, 0, 0, 6, new#4, 0, 3, 2, 5, 2, Um, Us, 360, new#7, new#8, 0, new#9, new#10, X, new#2, new#11, 18816, 9408, n_obs, 4, 784, 0)',
        'gpode_reparam_bwd(new#12, new#0+8, 4, eps_s, new#13, new#13+8, 4, 3, 2, 0)',
        'gradients: logits, Um, Us',
    ],
    'elbo_n_obs_packed_order2': [
        'gpode_reparam_fwd(new#0, new#0+8, 4, eps_s, new#1, 3, 2, 0)',
        'gpode_reparam_fwd(new#2, new#2+8, 4, eps_v, new#3, 3, 2, 0)',
        'gpode_sigmoid_loglik_fwd_len(X, logits, new#4, new#5, 6, 3136, 9408, 4, n_obs, 4, 784, 0)',
        'parts (6, 4), z (24, 1, 28, 28), z needs a gradient: False',
        'gpode_elbo_all_fwd(new#5, 6, 24, new#6, new#7, 3, 2, 5, 2, Um, Us, 360, new#8, 0)',
        'backward',
        'gpode_elbo_all_bwd_ll_len(new#9, 0, 0, 0, 6, new#6, new#7, 3, 2, 5, 2, Um, Us, 360, new#10, new#11, new#12, new#13, new#14, X, new#4, new#15, 18816, 9408, n_obs, 4, 784, 0)',
        'gpode_reparam_bwd(new#16, new#2+8, 4, eps_v, new#17, new#17+8, 4, 3, 2, 0)',
        'gpode_reparam_bwd(new#18, new#0+8, 4, eps_s, new#19, new#19+8, 4, 3, 2, 0)',
        'gradients: logits, Um, Us',
    ],
    'elbo_plain_halves_order1': [
        'gpode_reparam_kl_fwd(h_s, h_s+8, 4, eps_s, new#0, new#1, 3, 2, 0)',
        'gpode_sigmoid_loglik_fwd(X, logits, new#2, new#3, 6, 3136, 9408, 4, 0)',
        'parts (6, 4), z (24, 1, 28, 28), z needs a gradient: False',
        'gpode_elbo_all_fwd_kl(new#3, 6, 24, new#1, 1, 0, 0, 3, 5, 2, Um, Us, 360, new#4, 0)',
        'backward',
        'gpode_elbo_all_bwd_ll_kl(new#5, 0, 0, 0, 6, 3, 5, 2, Um, Us, 360, new#6, new#7, 1, 0, 0, new#8, new#9, X, new#2, new#10, 18816, 9408, 0)',
        'gpode_reparam_kl_bwd(new#11, new#7, h_s, h_s+8, 4, eps_s, new#12, new#12+8, 4, 3, 2, 0)',
        'gradients: logits, Um, Us',
    ],
    'elbo_plain_halves_order2': [
        'gpode_reparam_kl_fwd(h_s, h_s+8, 4, eps_s, new#0, new#1, 3, 2, 0)',
        'gpode_reparam_kl_fwd(h_v, h_v+8, 4, eps_v, new#2, new#3, 3, 2, 0)',
        'gpode_sigmoid_loglik_fwd(X, logits, new#4, new#5, 6, 3136, 9408, 4, 0)',
        'parts (6, 4), z (24, 1, 28, 28), z needs a gradient: False',
        'gpode_elbo_all_fwd_kl(new#5, 6, 24, new#1, 1, new#3, 1, 3, 5, 2, Um, Us, 360, new#6, 0)',
        'backward',
        'gpode_elbo_all_bwd_ll_kl(new#7, 0, 0, 0, 6, 3, 5, 2, Um, Us, 360, new#8, new#9, 1, new#10, 1, new#11, new#12, X, new#4, new#13, 18816, 9408, 0)',
        'gpode_reparam_kl_bwd(new#14, new#10, h_v, h_v+8, 4, eps_v, new#15, new#15+8, 4, 3, 2, 0)',
        'gpode_reparam_kl_bwd(new#16, new#9, h_s, h_s+8, 4, eps_s, new#17, new#17+8, 4, 3, 2, 0)',
        'gradients: logits, Um, Us',
    ],
    'elbo_plain_packed_order1': [
        'gpode_reparam_fwd(new#0, new#0+8, 4, eps_s, new#1, 3, 2, 0)',
        'gpode_sigmoid_loglik_fwd(X, logits, new#2, new#3, 6, 3136, 9408, 4, 0)',
        'parts (6, 4), z (24, 1, 28, 28), z needs a gradient: False',
        'gpode_elbo_all_fwd(new#3, 6, 24, new#4, 0, 3, 2, 5, 2, Um, Us, 360, new#5, 0)',
        'backward',
        'gpode_elbo_all_bwd_ll(new#6, 0, 0, 0, 6, new#4, 0, 3, 2, 5, 2, Um, Us, 360, new#7, new#8, 0, new#9, new#10, X, new#2, new#11, 18816, 9408, 0)',
        'gpode_reparam_bwd(new#12, new#0+8, 4, eps_s, new#13, new#13+8, 4, 3, 2, 0)',
        'gradients: logits, Um, Us',
    ],
    'elbo_plain_packed_order2': [
        'gpode_reparam_fwd(new#0, new#0+8, 4, eps_s, new#1, 3, 2, 0)',
        'gpode_reparam_fwd(new#2, new#2+8, 4, eps_v, new#3, 3, 2, 0)',
        'gpode_sigmoid_loglik_fwd(X, logits, new#4, new#5, 6, 3136, 9408, 4, 0)',
        'parts (6, 4), z (24, 1, 28, 28), z needs a gradient: False',
        'gpode_elbo_all_fwd(new#5, 6, 24, new#6, new#7, 3, 2, 5, 2, Um, Us, 360, new#8, 0)',
        'backward',
        'gpode_elbo_all_bwd_ll(new#9, 0, 0, 0, 6, new#6, new#7, 3, 2, 5, 2, Um, Us, 360, new#10, new#11, new#12, new#13, new#14, X, new#4, new#15, 18816, 9408, 0)',
        'gpode_reparam_bwd(new#16, new#2+8, 4, eps_v, new#17, new#17+8, 4, 3, 2, 0)',
        'gpode_reparam_bwd(new#18, new#0+8, 4, eps_s, new#19, new#19+8, 4, 3, 2, 0)',
        'gradients: logits, Um, Us',
    ],
    'gather_frames': [
        'gpode_gather_frames_fwd(ztL, 4, 2, index+16, 2, 3, 4, 7, new#0, 0)',
        'gathered (14, 2); backward',
        'gpode_gather_frames_bwd(new#1, 4, 2, index+16, index, 2, 3, 4, 7, new#2, 0)',
        'gather_frames of a ztL with one frame too many -> GpodeError: gather_frames: ztL must be (L,N,T,ld) = (L,3,4,ld), got (2, 3, 5, 4)',
    ],
    'kl_and_terms_halves': [
        'gpode_normal_kl_fwd(h_s, h_s+8, 4, new#0, 3, 2, 0)',
        'gpode_elbo_fwd(lhood, 6, new#0, 3, kl_u, 360, new#1, 0)',
        'terms (4,); backward',
        'gpode_elbo_bwd(new#2, 6, 3, 360, new#3, new#4, new#5, 0)',
        'gpode_normal_kl_bwd(new#4, h_s, h_s+8, 4, new#6, new#6+8, 4, 3, 2, 0)',
    ],
    'kl_and_terms_packed': [
        'gpode_normal_kl_fwd(new#0, new#0+8, 4, new#1, 3, 2, 0)',
        'gpode_elbo_fwd(lhood, 6, new#1, 3, kl_u, 360, new#2, 0)',
        'terms (4,); backward',
        'gpode_elbo_bwd(new#3, 6, 3, 360, new#4, new#5, new#6, 0)',
        'gpode_normal_kl_bwd(new#5, new#0, new#0+8, 4, new#7, new#7+8, 4, 3, 2, 0)',
    ],
    'last_stage': [
        'gpode_bn_stats(c, gamma, beta, new#0, new#1, running_mean, running_var, nbt, 0.1, 1e-05, new#2, 2, 16, 784, new#3, 0)',
        'gpode_conv2d_bwd_data_bn(c, new#2, w, b, new#4, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'y (2, 1, 28, 28); backward',
        'gpode_dec10_bn_bwd_sums_wgrad(c, new#5, w, gamma, beta, new#0, new#1, 0, new#6, new#7, 2, new#8, new#9, 0)',
        'gpode_dec10_bn_bwd_apply(c, new#5, w, gamma, beta, new#0, new#1, 0, 0, 0, 0, new#10, new#11, new#12, new#13, 2, new#8, 0)',
    ],
    'last_stage_deferred': [
        'gpode_bn_stats(c, gamma, beta, new#0, new#1, running_mean, running_var, nbt, 0.1, 1e-05, new#2, 2, 16, 784, new#3, 0)',
        'gpode_conv2d_bwd_data_bn(c, new#2, w, b, new#4, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'y (2, 1, 28, 28); backward',
        'gpode_defer_reductions(2)',
        'gpode_dec10_bn_bwd_sums_wgrad(c, new#5, w, gamma, beta, new#0, new#1, 0, new#6, new#7, 2, new#8, new#9, 0)',
        'gpode_defer_reductions(0)',
        'gpode_defer_reductions(1)',
        'gpode_dec10_bn_bwd_apply(c, new#5, w, gamma, beta, new#0, new#1, 0, 0, 0, 0, new#10, new#11, new#12, new#13, 2, new#8, 0)',
        'gpode_defer_reductions(0)',
        'gpode_flush_reductions(0)',
        'kept until the flush: 0, queued: False',
    ],
    'last_stage_deferred_sync': [
        'gpode_bn_moments(c, new#0, 2, 16, 784, new#1, 0)',
        'sync.gather(new#0)',
        'gpode_bn_finalize(new#2, 2, gamma, beta, new#3, new#4, running_mean, running_var, nbt, 0.1, 1e-05, new#5, 16, 0)',
        'gpode_conv2d_bwd_data_bn(c, new#5, w, b, new#6, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'y (2, 1, 28, 28); backward',
        'gpode_defer_reductions(2)',
        'gpode_dec10_bn_bwd_sums_wgrad(c, new#7, w, gamma, beta, new#3, new#4, new#8, new#9, new#10, 2, new#11, new#12, 0)',
        'gpode_defer_reductions(0)',
        'sync.gather(new#8)',
        'gpode_defer_reductions(1)',
        'gpode_dec10_bn_bwd_apply(c, new#7, w, gamma, beta, new#3, new#4, new#13, sync_weights, 2, 3136, new#14, new#15, new#16, new#17, 2, new#11, 0)',
        'gpode_defer_reductions(0)',
        'gpode_flush_reductions(0)',
        'kept until the flush: 0, queued: False',
    ],
    'last_stage_frozen': [
        'gpode_bn_stats(c, gamma, beta, new#0, new#1, running_mean, running_var, nbt, 0.1, 1e-05, new#2, 2, 16, 784, new#3, 0)',
        'gpode_conv2d_bwd_data_bn(c, new#2, w, b, new#4, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'y (2, 1, 28, 28); backward',
        'gpode_dec10_bn_bwd_sums(c, new#5, w, gamma, beta, new#0, new#1, 0, 2, new#6, 0)',
        'gpode_dec10_bn_bwd_apply(c, new#5, w, gamma, beta, new#0, new#1, 0, 0, 0, 0, new#7, new#8, new#9, new#10, 2, new#6, 0)',
    ],
    'last_stage_frozen_nobias': [
        'gpode_bn_stats(c, gamma, beta, new#0, new#1, running_mean, running_var, nbt, 0.1, 1e-05, new#2, 2, 16, 784, new#3, 0)',
        'gpode_conv2d_bwd_data_bn(c, new#2, w, 0, new#4, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'y (2, 1, 28, 28); backward',
        'gpode_dec10_bn_bwd_sums(c, new#5, w, gamma, beta, new#0, new#1, 0, 2, new#6, 0)',
        'gpode_dec10_bn_bwd_apply(c, new#5, w, gamma, beta, new#0, new#1, 0, 0, 0, 0, new#7, new#8, new#9, new#10, 2, new#6, 0)',
    ],
    'last_stage_misaligned': [
        'gpode_bn_fwd(new#0, gamma, beta, new#1, new#2, new#3, running_mean, running_var, nbt, 0.1, 1e-05, 2, 16, 784, 1, new#4, 0)',
        'gpode_conv2d_bwd_data(new#1, w, b, new#5, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'y (2, 1, 28, 28); backward',
        'gpode_conv2d_fwd(new#6, w, 0, new#7, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'gpode_conv2d_bwd_weight(new#6, new#1, new#8, 0, new#9, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'gpode_chan_sum(new#6, new#10, 2, 1, 784, new#11, 0)',
        'gpode_bn_bwd(new#0, new#7, gamma, beta, new#2, new#3, new#12, new#13, new#14, new#15, 2, 16, 784, 1, new#16, 0)',
    ],
    'last_stage_misaligned_sync': [
        'gpode_bn_moments(new#0, new#1, 2, 16, 784, new#2, 0)',
        'sync.gather(new#1)',
        'gpode_bn_finalize(new#3, 2, gamma, beta, new#4, new#5, running_mean, running_var, nbt, 0.1, 1e-05, new#6, 16, 0)',
        'gpode_bn_apply(new#0, new#6, new#7, 2, 16, 784, 1, 0)',
        'gpode_conv2d_bwd_data(new#7, w, b, new#8, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'y (2, 1, 28, 28); backward',
        'gpode_conv2d_fwd(new#9, w, 0, new#10, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'gpode_conv2d_bwd_weight(new#9, new#7, new#11, 0, new#12, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'gpode_chan_sum(new#9, new#13, 2, 1, 784, new#14, 0)',
        'gpode_bn_bwd_sums(new#0, new#10, gamma, beta, new#4, new#5, new#15, 2, 16, 784, 1, new#16, 0)',
        'sync.gather(new#15)',
        'gpode_bn_bwd_apply(new#0, new#10, gamma, beta, new#4, new#5, new#17, sync_weights, 2, 3136, new#18, new#19, new#20, new#21, 2, 16, 784, 1, new#16, 0)',
    ],
    'last_stage_nobias': [
        'gpode_bn_stats(c, gamma, beta, new#0, new#1, running_mean, running_var, nbt, 0.1, 1e-05, new#2, 2, 16, 784, new#3, 0)',
        'gpode_conv2d_bwd_data_bn(c, new#2, w, 0, new#4, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'y (2, 1, 28, 28); backward',
        'gpode_dec10_bn_bwd_sums_wgrad(c, new#5, w, gamma, beta, new#0, new#1, 0, new#6, 0, 2, new#7, new#8, 0)',
        'gpode_dec10_bn_bwd_apply(c, new#5, w, gamma, beta, new#0, new#1, 0, 0, 0, 0, new#9, new#10, new#11, new#12, 2, new#7, 0)',
    ],
    'last_stage_sync': [
        'gpode_bn_moments(c, new#0, 2, 16, 784, new#1, 0)',
        'sync.gather(new#0)',
        'gpode_bn_finalize(new#2, 2, gamma, beta, new#3, new#4, running_mean, running_var, nbt, 0.1, 1e-05, new#5, 16, 0)',
        'gpode_conv2d_bwd_data_bn(c, new#5, w, b, new#6, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'y (2, 1, 28, 28); backward',
        'gpode_dec10_bn_bwd_sums_wgrad(c, new#7, w, gamma, beta, new#3, new#4, new#8, new#9, new#10, 2, new#11, new#12, 0)',
        'sync.gather(new#8)',
        'gpode_dec10_bn_bwd_apply(c, new#7, w, gamma, beta, new#3, new#4, new#13, sync_weights, 2, 3136, new#14, new#15, new#16, new#17, 2, new#11, 0)',
    ],
    'last_stage_sync_frozen': [
        'gpode_bn_moments(c, new#0, 2, 16, 784, new#1, 0)',
        'sync.gather(new#0)',
        'gpode_bn_finalize(new#2, 2, gamma, beta, new#3, new#4, running_mean, running_var, nbt, 0.1, 1e-05, new#5, 16, 0)',
        'gpode_conv2d_bwd_data_bn(c, new#5, w, b, new#6, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'y (2, 1, 28, 28); backward',
        'gpode_dec10_bn_bwd_sums(c, new#7, w, gamma, beta, new#3, new#4, new#8, 2, new#9, 0)',
        'sync.gather(new#8)',
        'gpode_dec10_bn_bwd_apply(c, new#7, w, gamma, beta, new#3, new#4, new#10, sync_weights, 2, 3136, new#11, new#12, new#13, new#14, 2, new#9, 0)',
    ],
    'last_stage_sync_frozen_nobias': [
        'gpode_bn_moments(c, new#0, 2, 16, 784, new#1, 0)',
        'sync.gather(new#0)',
        'gpode_bn_finalize(new#2, 2, gamma, beta, new#3, new#4, running_mean, running_var, nbt, 0.1, 1e-05, new#5, 16, 0)',
        'gpode_conv2d_bwd_data_bn(c, new#5, w, 0, new#6, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'y (2, 1, 28, 28); backward',
        'gpode_dec10_bn_bwd_sums(c, new#7, w, gamma, beta, new#3, new#4, new#8, 2, new#9, 0)',
        'sync.gather(new#8)',
        'gpode_dec10_bn_bwd_apply(c, new#7, w, gamma, beta, new#3, new#4, new#10, sync_weights, 2, 3136, new#11, new#12, new#13, new#14, 2, new#9, 0)',
    ],
    'last_stage_sync_nobias': [
        'gpode_bn_moments(c, new#0, 2, 16, 784, new#1, 0)',
        'sync.gather(new#0)',
        'gpode_bn_finalize(new#2, 2, gamma, beta, new#3, new#4, running_mean, running_var, nbt, 0.1, 1e-05, new#5, 16, 0)',
        'gpode_conv2d_bwd_data_bn(c, new#5, w, 0, new#6, 2, 1, 28, 28, 16, 5, 1, 2, 28, 28, 0)',
        'y (2, 1, 28, 28); backward',
        'gpode_dec10_bn_bwd_sums_wgrad(c, new#7, w, gamma, beta, new#3, new#4, new#8, new#9, 0, 2, new#10, new#11, 0)',
        'sync.gather(new#8)',
        'gpode_dec10_bn_bwd_apply(c, new#7, w, gamma, beta, new#3, new#4, new#12, sync_weights, 2, 3136, new#13, new#14, new#15, new#16, 2, new#10, 0)',
    ],
    'loss_compact': [
        'gpode_reparam_kl_fwd(h_s, h_s+8, 4, eps_s, new#0, new#1, 3, 2, 0)',
        'model(logits=True, obs_index=FrameIndex, [])',
        'gpode_sigmoid_loglik_fwd_pk(X, logits, new#2, new#3, 6, new#4, 4, 784, 9408, 4, 0)',
        'gpode_elbo_all_fwd(new#3, 6, 24, h_s, 0, 3, 2, 5, 2, Um, Us, 360, new#5, 0)',
        '4 terms; backward',
        'gpode_elbo_all_bwd(new#6, 0, 0, 0, 6, h_s, 0, 3, 2, 5, 2, Um, Us, 360, new#7, new#8, 0, new#9, new#10, 0)',
        'gpode_sigmoid_loglik_bwd_pk(X, new#2, new#7, new#11, 6, new#4+16, 7, 4, 784, 9408, 0)',
        'compact without n_obs -> ValueError: compute_loss: compact=True needs n_obs, the frame count of every sequence of the padded minibatch',
        'compact on the unfused route -> ValueError: compute_loss: compact=True has one loss route, from the logits; it is not available under GPODE_UNFUSED_LOSS=1',
        "reached: [('frame_index', 'n_obs', 'NoneType'), ('sigmoid_loglik_parts', None, 'FrameIndex'), ('elbo_all', None, 'NoneType')]",
    ],
    'loss_fused': [
        'gpode_reparam_kl_fwd(h_s, h_s+8, 4, eps_s, new#0, new#1, 3, 2, 0)',
        'model(logits=True, obs_index=NoneType, [])',
        'gpode_sigmoid_loglik_fwd(X, logits, new#2, new#3, 6, 3136, 9408, 4, 0)',
        'gpode_elbo_all_fwd_kl(new#3, 6, 24, new#1, 1, 0, 0, 3, 5, 2, Um, Us, 360, new#4, 0)',
        '4 terms; backward',
        'gpode_elbo_all_bwd_ll_kl(new#5, 0, 0, 0, 6, 3, 5, 2, Um, Us, 360, new#6, new#7, 1, 0, 0, new#8, new#9, X, new#2, new#10, 18816, 9408, 0)',
        'gpode_reparam_kl_bwd(0, new#7, h_s, h_s+8, 4, eps_s, new#11, new#11+8, 4, 3, 2, 0)',
        "reached: [('sigmoid_loglik_parts', None, 'NoneType'), ('elbo_all', None, 'NoneType')]",
    ],
    'loss_fused_n_obs': [
        'gpode_reparam_kl_fwd(h_s, h_s+8, 4, eps_s, new#0, new#1, 3, 2, 0)',
        'model(logits=True, obs_index=NoneType, [])',
        'gpode_sigmoid_loglik_fwd_len(X, logits, new#2, new#3, 6, 3136, 9408, 4, n_obs, 4, 784, 0)',
        'gpode_elbo_all_fwd_kl(new#3, 6, 24, new#1, 1, 0, 0, 3, 5, 2, Um, Us, 360, new#4, 0)',
        '4 terms; backward',
        'gpode_elbo_all_bwd_ll_kl_len(new#5, 0, 0, 0, 6, 3, 5, 2, Um, Us, 360, new#6, new#7, 1, 0, 0, new#8, new#9, X, new#2, new#10, 18816, 9408, n_obs, 4, 784, 0)',
        'gpode_reparam_kl_bwd(0, new#7, h_s, h_s+8, 4, eps_s, new#11, new#11+8, 4, 3, 2, 0)',
        "reached: [('sigmoid_loglik_parts', 'n_obs', 'NoneType'), ('elbo_all', None, 'NoneType')]",
    ],
    'loss_unfused': [
        'gpode_reparam_kl_fwd(h_s, h_s+8, 4, eps_s, new#0, new#1, 3, 2, 0)',
        'model(logits=False, obs_index=NoneType, [])',
        'gpode_normal_kl_fwd(h_s, h_s+8, 4, new#2, 3, 2, 0)',
        'gpode_loglik_rowsum_fwd(X, Xrec, new#3, 6, 3136, 9408, 0)',
        'gpode_elbo_fwd(new#3, 6, new#2, 3, kl_u, 360, new#4, 0)',
        '4 terms; backward',
        'gpode_elbo_bwd(new#5, 6, 3, 360, new#6, new#7, new#8, 0)',
        'gpode_loglik_rowsum_bwd(X, Xrec, new#6, new#9, 6, 3136, 9408, 0)',
        'gpode_normal_kl_bwd(new#7, h_s, h_s+8, 4, new#10, new#10+8, 4, 3, 2, 0)',
        "reached: [('normal_kl_rows', None, 'NoneType'), ('bernoulli_loglik_rowsum', None, 'NoneType'), ('elbo_terms', None, 'NoneType')]",
    ],
    'loss_unfused_n_obs': [
        'gpode_reparam_kl_fwd(h_s, h_s+8, 4, eps_s, new#0, new#1, 3, 2, 0)',
        'model(logits=False, obs_index=NoneType, [])',
        'gpode_normal_kl_fwd(h_s, h_s+8, 4, new#2, 3, 2, 0)',
        'gpode_loglik_rowsum_fwd_len(X, Xrec, new#3, 6, 3136, 9408, n_obs, 4, 784, 0)',
        'gpode_elbo_fwd(new#3, 6, new#2, 3, kl_u, 360, new#4, 0)',
        '4 terms; backward',
        'gpode_elbo_bwd(new#5, 6, 3, 360, new#6, new#7, new#8, 0)',
        'gpode_loglik_rowsum_bwd_len(X, Xrec, new#6, new#9, 6, 3136, 9408, n_obs, 4, 784, 0)',
        'gpode_normal_kl_bwd(new#7, h_s, h_s+8, 4, new#10, new#10+8, 4, 3, 2, 0)',
        "reached: [('normal_kl_rows', None, 'NoneType'), ('bernoulli_loglik_rowsum', 'n_obs', 'NoneType'), ('elbo_terms', None, 'NoneType')]",
    ],
    'parts_alone': [
        'gpode_sigmoid_loglik_fwd(X, logits, new#0, new#1, 6, 3136, 9408, 4, 0)',
        'backward',
        'gpode_sigmoid_loglik_bwd(X, new#0, new#2, new#3, 6, 3136, 9408, 0)',
    ],
    'parts_alone_n_obs': [
        'gpode_sigmoid_loglik_fwd_len(X, logits, new#0, new#1, 6, 3136, 9408, 4, n_obs, 4, 784, 0)',
        'backward',
        'gpode_sigmoid_loglik_bwd_len(X, new#0, new#2, new#3, 6, 3136, 9408, n_obs, 4, 784, 0)',
    ],
    'predict': [
        'gpode_dec10_predict(c, table, w, b, X, 1, 15, 5, 4, 0, mean00, m200, se00, 0)',
        'gpode_dec10_predict(c, table, w, 0, X, 1, 15, 5, 4, 1, mean00, m200, se00, 0)',
        'draws folded in: 2',
        'gpode_dec10_predict_len(c, table, w, b, X, 1, 15, 5, 4, 0, mean01, m201, se01, n_obs, 0)',
        'gpode_dec10_predict_len(c, table, w, 0, X, 1, 15, 5, 4, 1, mean01, m201, se01, n_obs, 0)',
        'draws folded in: 2',
        'gpode_dec10_predict_ll(c, table, w, b, X, 1, 15, 5, 4, 0, mean20, m220, se20, ell20, 2, 0)',
        'gpode_dec10_predict_ll(c, table, w, 0, X, 1, 15, 5, 4, 1, mean20, m220, se20, ell20, 2, 0)',
        'draws folded in: 2',
        'gpode_dec10_predict_ll_len(c, table, w, b, X, 1, 15, 5, 4, 0, mean21, m221, se21, ell21, 2, n_obs, 0)',
        'gpode_dec10_predict_ll_len(c, table, w, 0, X, 1, 15, 5, 4, 1, mean21, m221, se21, ell21, 2, n_obs, 0)',
        'draws folded in: 2',
        'gpode_dec10_predict(new#0, table, w, b, X, 2, 15, 5, 4, 0, 0, 0, new#1, 0)',
        'two draws, no variance: done 2',
        'c of 8 channels -> GpodeError: dec10_predict: c (B,16,28,28), weight (16,1,5,5), table (16,4)',
        'a table of 8 channels -> GpodeError: dec10_predict: c (B,16,28,28), weight (16,1,5,5), table (16,4)',
        'c not a whole number of draws -> GpodeError: dec10_predict: X (N,T_obs,1,28,28), F = N * Th frames, c a whole number of draws of F frames',
        'F that is not N Th -> GpodeError: dec10_predict: X (N,T_obs,1,28,28), F = N * Th frames, c a whole number of draws of F frames',
        'targets of another size -> GpodeError: dec10_predict: X (N,T_obs,1,28,28), F = N * Th frames, c a whole number of draws of F frames',
        'ell of the wrong width -> GpodeError: gpode_dec10_predict_ll: ell must be a contiguous float32 (L_total, F) tensor',
        'n_obs int64 -> GpodeError: dec10_predict: n_obs must be an int32 tensor on the device of X',
        'table_conv_transpose2d',
        'gpode_conv2d_bwd_data_bn(c4, t4, w4, b4, new#2, 2, 32, 14, 14, 64, 5, 2, 1, 6, 6, 0)',
        'y (2, 32, 14, 14)',
        'gpode_conv2d_bwd_data_bn(c4, t4, w4, 0, new#3, 2, 32, 14, 14, 64, 5, 2, 1, 6, 6, 0)',
        'y (2, 32, 14, 14)',
        'a table of 16 channels -> GpodeError: table_conv_transpose2d: table must be (64, 4)',
    ],
    'refusals': [
        'sigmoid_loglik_parts, n_obs int64 -> GpodeError: sigmoid_loglik_parts: n_obs must be an int32 tensor on the device of X',
        'sigmoid_loglik_parts, n_obs a list -> GpodeError: sigmoid_loglik_parts: n_obs must be an int32 tensor on the device of X',
        'sigmoid_loglik_parts, n_obs (N + 1,) -> GpodeError: sigmoid_loglik_parts: n_obs must be (N,) = (3,), one frame count per sequence of X (N,T,...); got (4,)',
        'sigmoid_loglik_parts, n_obs (N, 1) -> GpodeError: sigmoid_loglik_parts: n_obs must be (N,) = (3,), one frame count per sequence of X (N,T,...); got (3, 1)',
        'sigmoid_loglik_parts, n_obs on another device -> GpodeError: sigmoid_loglik_parts: n_obs must be an int32 tensor on the device of X',
        'sigmoid_loglik_parts, X without a frame axis -> GpodeError: sigmoid_loglik_parts: n_obs must be (N,) = (3,), one frame count per sequence of X (N,T,...); got (3,)',
        'bernoulli_loglik_rowsum, n_obs int64 -> GpodeError: bernoulli_loglik_rowsum: n_obs must be an int32 tensor on the device of X',
        'bernoulli_loglik_rowsum, n_obs a list -> GpodeError: bernoulli_loglik_rowsum: n_obs must be an int32 tensor on the device of X',
        'bernoulli_loglik_rowsum, n_obs (N + 1,) -> GpodeError: bernoulli_loglik_rowsum: n_obs must be (N,) = (3,), one frame count per sequence of X (N,T,...); got (4,)',
        'bernoulli_loglik_rowsum, n_obs (N, 1) -> GpodeError: bernoulli_loglik_rowsum: n_obs must be (N,) = (3,), one frame count per sequence of X (N,T,...); got (3, 1)',
        'bernoulli_loglik_rowsum, n_obs on another device -> GpodeError: bernoulli_loglik_rowsum: n_obs must be an int32 tensor on the device of X',
        'bernoulli_loglik_rowsum, X without a frame axis -> GpodeError: bernoulli_loglik_rowsum: n_obs must be (N,) = (3,), one frame count per sequence of X (N,T,...); got (3,)',
        'n_obs together with index -> GpodeError: sigmoid_loglik_parts: n_obs (padded logits, masked) and index (compact logits) exclude each other',
        'padded logits with index -> GpodeError: sigmoid_loglik_parts: 10976 compact logits expected (L P frame = 2 x 7 x 784), got 18816',
        'index of another minibatch -> GpodeError: sigmoid_loglik_parts: X must be (N,T,...) = (3,4,...) and rows a multiple of N; got (3, 5, 1, 28, 28), rows 6',
        'rows no multiple of N -> GpodeError: sigmoid_loglik_parts: X must be (N,T,...) = (3,4,...) and rows a multiple of N; got (3, 4, 1, 28, 28), rows 7',
        'frame_index, nothing observed -> GpodeError: frame_index: no observed frame in the minibatch (every count is <= 0)',
        'frame_index, n_obs (N, 1) -> GpodeError: frame_index: n_obs must be an (N,) integer tensor, or pass counts=',
        'frame_index, counts of another length -> GpodeError: frame_index: 2 counts for n_obs of shape (3,)',
        'frame_index from host counts [9, -3, 2]: P 6, counts [4, 0, 2], off [0, 4, 4, 6], src [0, 1, 2, 3, 8, 9]',
    ],
    'rowsum': [
        'gpode_loglik_rowsum_fwd(X, z, new#0, 6, 3136, 9408, 0)',
        'rows (6,); backward',
        'gpode_loglik_rowsum_bwd(X, z, new#1, new#2, 6, 3136, 9408, 0)',
    ],
    'rowsum_n_obs': [
        'gpode_loglik_rowsum_fwd_len(X, z, new#0, 6, 3136, 9408, n_obs, 4, 784, 0)',
        'rows (6,); backward',
        'gpode_loglik_rowsum_bwd_len(X, z, new#1, new#2, 6, 3136, 9408, n_obs, 4, 784, 0)',
    ],
    'stage4': [
        'gpode_bn_stats(c, gamma, beta, new#0, new#1, running_mean, running_var, nbt, 0.1, 1e-05, new#2, 2, 64, 36, new#3, 0)',
        'gpode_conv2d_bwd_data_bn(c, new#2, w, b, new#4, 2, 32, 13, 13, 64, 5, 2, 1, 6, 6, 0)',
        'y (2, 32, 13, 13); backward',
        'gpode_conv2d_bwd_weight_bn(new#5, c, new#2, new#6, 0, new#7, 2, 32, 13, 13, 64, 5, 2, 1, 6, 6, 0)',
        'gpode_chan_sum(new#5, new#8, 2, 32, 169, new#9, 0)',
        'gpode_conv2d_fwd(new#5, w, 0, new#10, 2, 32, 13, 13, 64, 5, 2, 1, 6, 6, 0)',
        'gpode_bn_bwd(c, new#10, gamma, beta, new#0, new#1, new#11, new#12, new#13, new#14, 2, 64, 36, 1, new#15, 0)',
    ],
    'stage4_sync': [
        'gpode_bn_moments(c, new#0, 2, 64, 36, new#1, 0)',
        'sync.gather(new#0)',
        'gpode_bn_finalize(new#2, 2, gamma, beta, new#3, new#4, running_mean, running_var, nbt, 0.1, 1e-05, new#5, 64, 0)',
        'gpode_conv2d_bwd_data_bn(c, new#5, w, b, new#6, 2, 32, 13, 13, 64, 5, 2, 1, 6, 6, 0)',
        'y (2, 32, 13, 13); backward',
        'gpode_conv2d_bwd_weight_bn(new#7, c, new#5, new#8, 0, new#9, 2, 32, 13, 13, 64, 5, 2, 1, 6, 6, 0)',
        'gpode_chan_sum(new#7, new#10, 2, 32, 169, new#11, 0)',
        'gpode_conv2d_fwd(new#7, w, 0, new#12, 2, 32, 13, 13, 64, 5, 2, 1, 6, 6, 0)',
        'gpode_bn_bwd_sums(c, new#12, gamma, beta, new#3, new#4, new#13, 2, 64, 36, 1, new#14, 0)',
        'sync.gather(new#13)',
        'gpode_bn_bwd_apply(c, new#12, gamma, beta, new#3, new#4, new#15, sync_weights, 2, 144, new#16, new#17, new#18, new#19, 2, 64, 36, 1, new#14, 0)',
    ],
}


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    pprint.pprint({k: transcript(k) for k in sorted(SCENARIOS)}, width=250, sort_dicts=True)
