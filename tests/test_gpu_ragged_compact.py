"""GPU: the compact ragged route -- the padded frames of a ragged minibatch are taken out in front of the decoder (vae_ops.frame_index,
gather_frames), the decoder runs on the L P observed frames and the loss stage reads compact logits (gpode_sigmoid_loglik_fwd_pk /
_bwd_pk).  c[n] = clamp(n_obs[n], 0, T), off its exclusive prefix sum, P = sum c, compact image j = off[n] + t <-> src[j] = n T + t.

1  gather / scatter through the C ABI: L = 2, N = 5, T = 4, q = 6, ld in {6, 12}, counts (0, 1, 4, 3, 9).  Forward torch.equal to
   zt[:, n, t, :q]; backward into a NaN-filled gzt: no NaN left, observed rows equal gout, everything else exactly 0; guard words behind
   every buffer intact (loss_routes.Bufs); each refusal (NULL index, q > ld, a non-positive size, P > N T) writes nothing.
2  the _pk loss kernels against fp64 torch: x a - softplus(a) summed over each row's observed frames, the gradient by autograd in fp64.
   Row sums within loss_routes.TOL (2e-5) of sum |terms|, z within TOL_Z (1e-6), ga within 2e-5 of its largest entry -- the bounds
   test_gpu_ragged_loss.py holds the *_len entries to.  Shapes (L, T, frame), counts as above clamped to T = 5: (2, 5, 784) -- 4
   slices of 980 elements, so a slice boundary falls inside an image and the one-frame row (784) is shorter than a slice; (2, 5, 8) --
   one slice; (2, 5, 784) with the logits and z / ga one float off a 16-byte boundary -- the scalar paths.  The row with c = 0 is exactly
   0.0 in every slice; with full lengths z, part and ga have the bits of gpode_sigmoid_loglik_fwd / _bwd; NaN in every padded target
   frame changes no bit.
3  the model (tiny, N = 4, T = 5, L = 2, orders 1 and 2, batch from data.utils.ragged_frames) against the torch-side composition: the
   model's own rollout, index_select on the flattened states (with the position slice for order 2), the model's own decoder on the
   compact states, the loss in fp64 over compact rows as test_gpu_ragged_model.torch_side assembles it over a mask; device generators
   re-seeded before each run.  Terms within TOL_KL (1e-5) of their scales, parameter gradients within 2e-5 of their largest entry, the
   dead biases as that file holds them.  Both sides launch the same decoder on the same bits, so these bounds rest on the loss kernels
   and the gather alone.  After the step the three decoder BatchNorm layers' running_mean, running_var and num_batches_tracked equal the
   reference run's; the compact nll differs from the masked route's (the statistics differ).
4  the padding is gone (rk4, order 1): other padded columns of ts (rows still increasing) and other padded target frames leave the
   compact loss terms and every gradient torch.equal; with n_obs alone the loss changes -- the defect this route closes.
5  full lengths: the compact logits are the plain call's logits bit for bit, the loss terms within TOL_KL of it.
6  recorded launches: compact=False records no _pk / gather_frames entry and is the masked list of before (the plain list with the
   three loss-stage entries in their _len form); compact=True records them and its decoder convolutions carry L P images.
7  main(--ragged_frames 3 --ragged_compact True): two eager steps, finite ELBOs and checkpoint, and the log line."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as Fn

import loss_routes as R
from test_gpu_ragged_model import NO_GRAD, ORDERS, compare_grads, grads, ragged_batch
from test_gpu_time_grids import bits, tiny_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def leave_the_global_generators_as_found():
    """as test_gpu_ragged_model.py: the tests here seed and draw from the process-wide generators; later files must not see that"""
    import random
    import numpy as np
    saved = (torch.get_rng_state(), torch.cuda.get_rng_state_all(), np.random.get_state(), random.getstate())
    yield
    torch.set_rng_state(saved[0])
    torch.cuda.set_rng_state_all(saved[1])
    np.random.set_state(saved[2])
    random.setstate(saved[3])


COUNTS = (0, 1, 4, 3, 9)


def host_index(counts, T):
    """(c, off, src) as lists"""
    c = [min(max(k, 0), T) for k in counts]
    off = [0]
    for k in c:
        off.append(off[-1] + k)
    return c, off, [n * T + t for n, k in enumerate(c) for t in range(k)]


def device_index(counts, T):
    from vae_gp_ode_amd import vae_ops as V
    ix = V.frame_index(torch.tensor(counts, dtype=torch.int32, device='cuda'), T, counts=counts)
    c, off, src = host_index(counts, T)
    assert ix.off.tolist() == off and ix.src.tolist() == src and ix.P == off[-1] and ix.off.is_cuda and ix.off.dtype == torch.int32
    return ix


# ---- 1. gather / scatter ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ld', [6, 12])
def test_gather_and_scatter(ld):
    L, N, T, q = 2, 5, 4, 6
    ix = device_index(COUNTS, T)
    c, off, src = host_index(COUNTS, T)
    P = ix.P
    g = R._gen('compact gather', ld)
    zt_h, gout_h = torch.randn(L, N, T, ld, generator=g), torch.randn(L * P, q, generator=g)
    bf, tags = R.Bufs(), {}
    zt, gout = bf.new('zt', zt_h.numel(), zt_h), bf.new('gout', gout_h.numel(), gout_h)
    out, gzt = bf.new('out', L * P * q), bf.new('gzt', L * N * T * ld)
    R._call(tags, 'fwd', 'gpode_gather_frames_fwd', zt, ld, q, ix.src, L, N, T, P, out)
    R._call(tags, 'bwd', 'gpode_gather_frames_bwd', gout, ld, q, ix.src, ix.off, L, N, T, P, gzt)
    assert not bf.problems(), bf.problems()
    assert tags == dict(fwd='gather_frames_fwd', bwd='gather_frames_bwd'), tags
    want = torch.stack([zt_h[l, s // T, s % T, :q] for l in range(L) for s in src])
    assert torch.equal(out.cpu().view(L * P, q), want)
    ref = torch.zeros(L, N, T, ld)
    for l in range(L):
        for j, s in enumerate(src):
            ref[l, s // T, s % T, :q] = gout_h[l * P + j]
    got = gzt.cpu().view(L, N, T, ld)
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got, ref)
    obs = torch.tensor([[t < k for t in range(T)] for k in c])
    assert bool((got[:, ~obs] == 0).all()) and bool((got[..., q:] == 0).all())


@pytest.mark.parametrize('case', ['null src', 'null off', 'q > ld', 'L = 0', 'P = 0', 'T < 0', 'P > N T'])
def test_gather_refusals_write_nothing(case):
    L, N, T, q, ld = 2, 5, 4, 6, 6
    ix = device_index(COUNTS, T)
    P = ix.P
    bf = R.Bufs()
    zt, gout = bf.new('zt', L * N * T * ld, torch.zeros(L * N * T * ld)), bf.new('gout', L * P * q, torch.zeros(L * P * q))
    out, gzt = bf.new('out', L * P * q), bf.new('gzt', L * N * T * ld)
    src, off = ix.src, ix.off
    if case == 'null src':
        src = None
    elif case == 'null off':
        off = None
    elif case == 'q > ld':
        q = ld + 1
    elif case == 'L = 0':
        L = 0
    elif case == 'P = 0':
        P = 0
    elif case == 'T < 0':
        T = -4
    else:
        P = N * T + 1
    if case != 'null off':                            # the forward takes no off
        with pytest.raises(R.Refused, match='gpode_gather_frames_fwd'):
            R._call({}, 'x', 'gpode_gather_frames_fwd', zt, ld, q, src, L, N, T, P, out)
    with pytest.raises(R.Refused, match='gpode_gather_frames_bwd'):
        R._call({}, 'x', 'gpode_gather_frames_bwd', gout, ld, q, src, off, L, N, T, P, gzt)
    assert bf.untouched(), 'a refused call wrote an output'
    assert not [p for p in bf.problems() if 'guard' in p]


# ---- 2. the _pk loss kernels ------------------------------------------------------------------------------------------------------------
PK = {'f784': (2, 5, 784, ''), 'f8': (2, 5, 8, ''), 'f784mis': (2, 5, 784, 'az')}


@functools.lru_cache(maxsize=None)
def pk_inputs(key):
    L, T, frame, _ = PK[key]
    N = len(COUNTS)
    g = R._gen('compact loss', L, T, frame)
    return dict(X=R._x_form((N, T, frame), 'norm', g), a=R._logits((L, N, T, frame), g), grow=torch.randn(L * N, generator=g))


def pk_once(key, counts, nan_padding=False):
    """the _pk forward and backward on the compact form of pk_inputs(key) -> (outputs on the CPU, nsplit, chunk, host index)"""
    L, T, frame, mis = PK[key]
    N = len(counts)
    d = pk_inputs(key)
    c, off, src = host_index(counts, T)
    ix = device_index(counts, T)
    P, rows = ix.P, L * N
    X = d['X'].clone()
    if nan_padding:
        for n, k in enumerate(c):
            X[n, k:] = float('nan')
        assert bool(torch.isnan(X).any())
    a_c = torch.stack([d['a'][l, s // T, s % T] for l in range(L) for s in src])          # (L P, frame)
    sh = lambda ch: 1 if ch in mis else 0
    bf, tags = R.Bufs(), {}
    Xd, ad = bf.new('X', X.numel(), X), bf.new('a', a_c.numel(), a_c, shift=sh('a'))
    z, ga = bf.new('z', a_c.numel(), shift=sh('z')), bf.new('ga', a_c.numel(), shift=sh('z'))
    ns = R.sigmoid_loglik_splits(rows, T * frame)
    part, grow = bf.new('part', rows * ns), bf.new('grow', rows, d['grow'])
    R._call(tags, 'fwd', 'gpode_sigmoid_loglik_fwd_pk', Xd, ad, z, part, rows, ix.off, T, frame, X.numel(), ns)
    R._call(tags, 'bwd', 'gpode_sigmoid_loglik_bwd_pk', Xd, z, grow, ga, rows, ix.src, P, T, frame, X.numel())
    assert not bf.problems(), bf.problems()
    assert tags == dict(fwd='sigmoid_loglik_fwd_pk', bwd='sigmoid_loglik_bwd_pk'), tags
    chunk = (-(-(T * frame) // ns) + 3) // 4 * 4
    return dict(z=z.cpu(), part=part.cpu().view(rows, ns), ga=ga.cpu()), ns, chunk, (c, off, src, a_c)


@pytest.mark.parametrize('key', list(PK))
def test_pk_loss_kernels_against_fp64(key):
    L, T, frame, _ = PK[key]
    N = len(COUNTS)
    got, ns, chunk, (c, off, src, a_c) = pk_once(key, COUNTS)
    d = pk_inputs(key)
    P = off[-1]
    a64 = a_c.double().view(L, P, frame).requires_grad_(True)
    x64 = torch.stack([d['X'][s // T, s % T] for s in src]).double()[None]             # (1, P, frame)
    terms = x64 * a64 - Fn.softplus(a64)
    seq = torch.tensor([s // T for s in src])
    rowsum = torch.zeros(L, N, dtype=torch.float64).index_add(1, seq, terms.sum(-1))
    scale = torch.zeros(L, N, dtype=torch.float64).index_add(1, seq, terms.detach().abs().sum(-1))
    (rowsum * d['grow'].double().view(L, N)).sum().backward()
    part = got['part'].double()
    e_rows = ((part.sum(1).view(L, N) - rowsum.detach()).abs() / scale.clamp_min(1e-300))[:, [k > 0 for k in c]].max().item()
    e_z = (got['z'].double() - torch.sigmoid(a_c.double()).reshape(-1)).abs().max().item()
    e_ga = ((got['ga'].double() - a64.grad.reshape(-1)).abs().max() / a64.grad.abs().max()).item()
    print('%s: nsplit %d, chunk %d; row sums %.2e (%.1e), z %.2e (%.1e), ga %.2e (2e-5)' % (key, ns, chunk, e_rows, R.TOL, e_z, R.TOL_Z, e_ga))
    # a row without a frame: exactly 0.0 in every slice; and every slice beyond a row's length
    empty = [n for n, k in enumerate(c) if k == 0]
    assert empty and all(bool((part.view(L, N, ns)[:, n] == 0).all()) for n in empty)
    for n, k in enumerate(c):
        for s in range(ns):
            if s * chunk >= k * frame:
                assert bool((part.view(L, N, ns)[:, n, s] == 0).all()), (n, s)
    if ns > 1:
        inside_image = any(0 < b < k * frame and b % frame != 0 for k in c for b in range(chunk, T * frame, chunk))
        short_row = any(0 < k * frame < chunk for k in c)
        assert inside_image and short_row, (chunk, frame, c)
    assert e_rows <= R.TOL and e_z <= R.TOL_Z and e_ga <= 2e-5, (e_rows, e_z, e_ga)


def test_pk_shapes_run_one_slice_and_several():
    from vae_gp_ode_amd import _lib
    ns = {key: _lib.load().gpode_sigmoid_loglik_splits(PK[key][0] * len(COUNTS), PK[key][1] * PK[key][2]) for key in PK}
    assert 1 in ns.values() and any(v > 1 for v in ns.values()), ns
    assert all(v == R.sigmoid_loglik_splits(PK[key][0] * len(COUNTS), PK[key][1] * PK[key][2]) for key, v in ns.items())


@pytest.mark.parametrize('key', list(PK))
def test_pk_full_lengths_give_the_bits_of_the_twin(key):
    L, T, frame, mis = PK[key]
    N = len(COUNTS)
    got, ns, _, (c, off, src, a_c) = pk_once(key, (T,) * N)
    assert src == list(range(N * T))
    d = pk_inputs(key)
    rows, inner, nX = L * N, T * frame, N * T * frame
    sh = lambda ch: 1 if ch in mis else 0
    bf, tags = R.Bufs(), {}
    Xd, ad = bf.new('X', nX, d['X']), bf.new('a', rows * inner, d['a'], shift=sh('a'))
    z, ga = bf.new('z', rows * inner, shift=sh('z')), bf.new('ga', rows * inner, shift=sh('z'))
    part, grow = bf.new('part', rows * ns), bf.new('grow', rows, d['grow'])
    R._call(tags, 'fwd', 'gpode_sigmoid_loglik_fwd', Xd, ad, z, part, rows, inner, nX, ns)
    R._call(tags, 'bwd', 'gpode_sigmoid_loglik_bwd', Xd, z, grow, ga, rows, inner, nX)
    assert not bf.problems()
    assert torch.equal(R._bits(got['z']), R._bits(z.cpu())), 'z differs from the twin'
    assert torch.equal(R._bits(got['part']), R._bits(part.cpu().view(rows, ns))), 'part differs from the twin'
    assert torch.equal(R._bits(got['ga']), R._bits(ga.cpu())), 'ga differs from the twin'


@pytest.mark.parametrize('key', list(PK))
def test_pk_padded_targets_are_never_read(key):
    clean = pk_once(key, COUNTS)[0]
    dirty = pk_once(key, COUNTS, nan_padding=True)[0]
    for k in clean:
        assert bool(torch.isfinite(dirty[k]).all()), k
        assert torch.equal(R._bits(clean[k]), R._bits(dirty[k])), k


@pytest.mark.parametrize('case', ['null off', 'null src', 'frame % 4', 'nX', 'rows'])
def test_pk_refusals_write_nothing(case):
    L, T, frame = 2, 5, 8
    N = len(COUNTS)
    ix = device_index(COUNTS, T)
    rows, nX, n = L * N, N * T * frame, L * ix.P * frame
    off, src = ix.off, ix.src
    if case == 'null off':
        off = None
    elif case == 'null src':
        src = None
    elif case == 'frame % 4':
        frame = 6
    elif case == 'nX':
        nX = T * frame // 2
    else:
        rows = L * N - 1
    bf = R.Bufs()
    X, a = bf.new('X', N * T * 8, torch.zeros(N * T * 8)), bf.new('a', n, torch.zeros(n))
    zin, grow = bf.new('zin', n, torch.zeros(n) + 0.5), bf.new('grow', L * N, torch.zeros(L * N))
    z, part, ga = bf.new('z', n), bf.new('part', L * N), bf.new('ga', n)
    if case != 'null src':
        with pytest.raises(R.Refused, match='gpode_sigmoid_loglik_fwd_pk'):
            R._call({}, 'x', 'gpode_sigmoid_loglik_fwd_pk', X, a, z, part, rows, off, T, frame, nX, 1)
    if case != 'null off':
        with pytest.raises(R.Refused, match='gpode_sigmoid_loglik_bwd_pk'):
            R._call({}, 'x', 'gpode_sigmoid_loglik_bwd_pk', X, zin, grow, ga, rows, src, ix.P, T, frame, nX)
    assert bf.untouched(), 'a refused call wrote an output'
    assert not [p for p in bf.problems() if 'guard' in p]


# ---- 3 - 6. the model -------------------------------------------------------------------------------------------------------------------
N, T, L = 4, 5, 2
_orders = pytest.mark.parametrize('order', list(ORDERS))


def run(m, src, X, L_, **kw):
    """compute_loss + backward with the device generators re-seeded -> (four terms, gradients)"""
    from vae_gp_ode_amd.model.create_model import compute_loss
    m.zero_grad(set_to_none=True)
    src.manual_seed(17)
    out = compute_loss(m, X, L_, **kw)
    out[0].backward()
    torch.cuda.synchronize()
    return [t.detach().clone() for t in out], grads(m)


def bn_buffers(m):
    d = m.vae.decoder.decnn
    return [t.detach().clone() for i in (2, 5, 8) for t in (d[i].running_mean, d[i].running_var, d[i].num_batches_tracked)]


def torch_side_compact(m, src, X, ts, n_obs, monkeypatch, N=N):
    """the compact ELBO composed in torch: the model's rollout, index_select on the flattened states, the model's decoder on the compact
    states, the loss in float64 over compact rows -> (four terms, their scales, gradients)"""
    from vae_gp_ode_amd import vae_ops as V
    ix = V.frame_index(n_obs, T)
    P = ix.P

    def decode(ztL, index, logits=False):
        Ld, Nd, Td, W = ztL.shape
        take = (torch.arange(Ld, device=ztL.device)[:, None] * (Nd * Td) + index.src.long()[None, :]).reshape(-1)
        lat = ztL.reshape(Ld * Nd * Td, W).index_select(0, take)[:, :W // m.order]
        return m.vae.decoder(lat, logits=True)
    m.zero_grad(set_to_none=True)
    src.manual_seed(17)
    with monkeypatch.context() as mp:
        mp.setattr(m, 'decode_observed', decode)
        logits, (s_mu, s_logv), (v_mu, v_logv) = m(X, L, logits=True, ts=ts, obs_index=ix)
    a = logits.double().view(L, P, -1)
    x = X.double().view(N * T, -1).index_select(0, ix.src.long())[None]
    lp = x * a - Fn.softplus(a)
    seq = torch.div(ix.src.long(), T, rounding_mode='floor')
    zero = torch.zeros(L, N, dtype=torch.float64, device=X.device)
    lh = zero.index_add(1, seq, lp.sum(-1)).mean(0).mean()
    kl = R.normal_kl(s_mu.double(), s_logv.double()).sum(-1)
    if v_mu is not None:
        kl = kl + R.normal_kl(v_mu.double(), v_logv.double()).sum(-1)
    kl = kl.mean()
    ku = m.flow.kl().double()
    nobs = float(m.num_observations)
    out = [-(lh * nobs - kl * nobs - ku), -lh, kl, ku]
    out[0].backward()
    torch.cuda.synchronize()
    field = m.flow.odefunc.diffeq
    ku_abs = R.svgp_kl_terms_abs(field.Um.optvar.detach().double().cpu(), field.us_packed().detach().double().cpu(), field.M)
    lh_abs = zero.index_add(1, seq, lp.detach().abs().sum(-1)).mean().item()
    scale = [lh_abs * nobs + kl.item() * nobs + float(ku_abs), lh_abs, kl.item(), float(ku_abs)]
    return [t.detach() for t in out], scale, grads(m)


@_orders
def test_compact_loss_matches_the_torch_side_composition(order, monkeypatch):
    m, src = tiny_model(**ORDERS[order])
    init = copy.deepcopy(m.state_dict())
    X, ts, n_obs = ragged_batch(m)
    out, g = run(m, src, X, L, ts=ts, n_obs=n_obs, compact=True)
    bn = bn_buffers(m)
    m.load_state_dict(init)
    ref, scale, gr = torch_side_compact(m, src, X, ts, n_obs, monkeypatch)
    bn_ref = bn_buffers(m)
    m.load_state_dict(init)
    masked, _ = run(m, src, X, L, ts=ts, n_obs=n_obs)
    e_terms = [abs(float(a) - float(b)) / s for a, b, s in zip(out, ref, scale)]
    errs = compare_grads(g, gr, 'compact')
    print('%s compact n_obs %s: terms %s; gradients worst %s' % (order, n_obs.tolist(), ['%.2e' % e for e in e_terms],
                                                                 sorted(((v, k) for k, v in errs.items()), reverse=True)[:3]))
    assert all(e <= R.TOL_KL for e in e_terms), e_terms
    bad = {k: v for k, v in errs.items() if not v <= 2e-5}
    assert not bad, bad
    assert int(bn[2]) == 1 and all(torch.equal(a, b) for a, b in zip(bn, bn_ref)), 'the BatchNorm buffers differ from the reference run'
    assert float(out[1]) != float(masked[1]), 'compact and masked nll agree: the statistics must differ'


def test_the_padding_is_gone():
    m, src = tiny_model()
    init = copy.deepcopy(m.state_dict())
    X, ts, n_obs = ragged_batch(m)
    ts2, X2 = ts.clone(), X.clone()
    for n, k in enumerate(n_obs.tolist()):
        assert 0 < k <= T
        ts2[n, k:] = ts[n, k - 1] + 0.037 * torch.arange(1, T - k + 1, device=ts.device)
        X2[n, k:] = 0.25 + 0.5 * torch.rand(X[n, k:].shape, generator=torch.Generator().manual_seed(3)).cuda()
    assert bool((ts2[:, 1:] > ts2[:, :-1]).all()) and not torch.equal(ts, ts2) and not torch.equal(X, X2)
    res = {}
    for name, kw in (('compact', dict(compact=True)), ('masked', dict())):
        for tag, (Xi, ti) in (('a', (X, ts)), ('b', (X2, ts2))):
            m.load_state_dict(init)
            res[name, tag] = run(m, src, Xi, L, ts=ti, n_obs=n_obs, **kw)
    (oa, ga), (ob, gb) = res['compact', 'a'], res['compact', 'b']
    assert all(torch.equal(a, b) for a, b in zip(oa, ob)), ([float(t) for t in oa], [float(t) for t in ob])
    assert ga.keys() == gb.keys()
    differs = [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert not differs, differs
    assert not torch.equal(res['masked', 'a'][0][0], res['masked', 'b'][0][0]), 'the masked loss does not see the padding: nothing to close'


@_orders
def test_full_lengths_are_the_plain_call(order):
    from vae_gp_ode_amd import vae_ops as V
    m, src = tiny_model(**ORDERS[order])
    init = copy.deepcopy(m.state_dict())
    X, ts, _ = ragged_batch(m)
    full = torch.full((N,), T, dtype=torch.int32, device='cuda')
    src.manual_seed(17)
    with torch.no_grad():
        plain = m(X, L, logits=True, ts=ts)[0]
    m.load_state_dict(init)
    src.manual_seed(17)
    with torch.no_grad():
        comp = m(X, L, logits=True, ts=ts, obs_index=V.frame_index(full, T))[0]
    assert tuple(comp.shape) == (L * N * T, 1, 28, 28) and bits(comp.reshape(plain.shape), plain)
    m.load_state_dict(init)
    p, _ = run(m, src, X, L, ts=ts)
    m.load_state_dict(init)
    c, _ = run(m, src, X, L, ts=ts, n_obs=full, compact=True, counts=[T] * N)
    e = [abs(float(a) - float(b)) / max(abs(float(b)), 1e-30) for a, b in zip(c, p)]
    print('%s full lengths, compact against plain: %s' % (order, ['%.2e' % v for v in e]))
    assert all(v <= R.TOL_KL for v in e), e


CONVS = ('gpode_convT_fwd_stats', 'gpode_conv2d_fwd', 'gpode_conv2d_bwd_data', 'gpode_conv2d_bwd_data_bn', 'gpode_conv2d_bwd_weight',
         'gpode_conv2d_bwd_weight_bn')


def test_recorded_launches(monkeypatch):
    from vae_gp_ode_amd import _lib
    from vae_gp_ode_amd.model.create_model import compute_loss
    m, src = tiny_model()
    X, ts, n_obs = ragged_batch(m)
    P = int(n_obs.clamp(0, T).sum())
    assert L * P not in (N, L * N * T)
    calls, images, real = [], [], _lib.call

    def call(name, *args):
        rc = real(name, *args)
        calls.append((name, _lib.load().gpode_last_launch().decode()))
        if name in CONVS:
            images.append(next(a for a in args if isinstance(a, int)))
        return rc
    monkeypatch.setattr(_lib, 'call', call)

    def record(**kw):
        del calls[:], images[:]
        src.manual_seed(17)
        compute_loss(m, X, L, ts=ts, **kw)[0].backward()
        torch.cuda.synchronize()
        return list(calls), list(images)
    new = lambda cs: [c for c in cs if '_pk' in c[0] or '_pk' in c[1] or 'gather_frames' in c[0] or 'gather_frames' in c[1]]
    (plain, _), (masked, im_m), (off, im_o), (comp, im_c) = record(), record(n_obs=n_obs), record(n_obs=n_obs, compact=False), \
        record(n_obs=n_obs, compact=True)
    stage = ('gpode_sigmoid_loglik_fwd', 'gpode_elbo_all_bwd_ll_kl', 'gpode_elbo_all_bwd_ll')
    swapped = [(n + '_len', t + '_len') if n in stage else (n, t) for n, t in plain]
    assert not new(plain) and not new(off) and off == masked == swapped, (off, swapped)
    assert im_o == im_m and L * N * T in im_o and set(im_o) <= {N, L * N * T}, im_o
    assert [c[0] for c in new(comp)] == ['gpode_gather_frames_fwd', 'gpode_sigmoid_loglik_fwd_pk', 'gpode_sigmoid_loglik_bwd_pk',
                                         'gpode_gather_frames_bwd'], comp
    assert [c[1] for c in new(comp)] == ['gather_frames_fwd', 'sigmoid_loglik_fwd_pk', 'sigmoid_loglik_bwd_pk', 'gather_frames_bwd']
    assert L * P in im_c and [L * N * T if b == L * P else b for b in im_c] == im_o, (im_c, im_o)
    assert not [c for c in comp if c[0].endswith('_len')], comp


# ---- 7. the command line ----------------------------------------------------------------------------------------------------------------
def test_main_trains_compact(tmp_path, monkeypatch):
    import glob
    import math
    from vae_gp_ode_amd import main as M
    from vae_gp_ode_amd import ops, vae_ops
    monkeypatch.chdir(tmp_path)
    argv = ['--task', 'synthetic', '--Ndata', '8', '--Ntest', '4', '--batch', '4', '--T', '6', '--solver', 'rk4', '--num_inducing', '16',
            '--num_features', '32', '--lr', '1e-4', '--log_freq', '1', '--Nepoch', '1', '--ragged_frames', '3', '--ragged_compact', 'True',
            '--save', 'results/c']
    try:
        M.main(argv)
        ck = glob.glob(str(tmp_path / 'results' / 'c_*' / 'odegpvae_mnist.pth'))
        assert len(ck) == 1
        sd = torch.load(ck[0])
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
        log = open(glob.glob(str(tmp_path / 'results' / 'c_*' / 'logs'))[0]).read()
        elbo = [float(ln.split('elbo')[1].split('(')[0]) for ln in log.splitlines() if ln.startswith('Iter:')]
        assert len(elbo) == 2 and all(math.isfinite(v) for v in elbo), elbo
        assert 'keeps 3 to 6 of its frames' in log and 'Padded frames are not decoded' in log
    finally:                                         # process-wide switches the training loop sets for itself
        ops.set_overlap(False)
        vae_ops.set_deferred_reductions(False)
