"""GPU: posterior-predictive evaluation -- the frozen decoder (Decoder.decode_frozen), the predictive last stage
(gpode_dec10_predict), evaluate.predict / compute_mse_std and the command line -- against fixtures produced by the reference's own
modules in eval() (tests/golden/make_golden_eval.py) and against the route that existed before (model.eval(); model(X, L); torch
reductions).

Bounds.  Decoded images and the predictive mean: relerr < 2e-4 against the reference's float32 result, the bound
tests/test_gpu_model.py puts on reconstructions.  mse, std, mse_t and the predictive variance: against the reference's float64
recomputation with 2e-4 + 3 relerr(reference float32, reference float64) -- relerr is the max-norm ratio of test_gpu_forward.py,
which for the variance is the largest difference over the peak variance of the case.  End to end (encoder and integrator in the
path) the float64 twin is the oracle's float64 flow on the recorded z0 followed by a float64 evaluation of the eval-mode decoder, and
the allowance is that of test_gpu_forward.py: 2e-4 + 3 relerr(reference float32, twin).  Bitwise claims have no tolerance."""
import copy
import json
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.nn.functional as Fn

from conftest import ROOT, load_golden, sub
from test_gpu_forward import relerr

pytestmark = pytest.mark.gpu

CASES = [('eval_rbf1', dict()), ('eval_rbf2', dict(ode=2, D_in=6, D_out=3, latent_dim=3)), ('eval_df1', dict(kernel='DF')),
         ('eval_rbf1_roll', dict())]
L_FIX = 3


def model_args(**kw):
    a = dict(D_in=6, D_out=6, num_inducing=8, num_features=16, dimwise=True, q_diag=False, device='cuda', kernel='RBF',
             ode=1, solver='rk4', use_adjoint=False, frames=5, n_filt=8, latent_dim=6, Ndata=360, dt=0.1)
    a.update(kw)
    return types.SimpleNamespace(**a)


def make_model(name, kw):
    from vae_gp_ode_amd.model.create_model import build_model
    g = load_golden(name)
    m = build_model(model_args(dt=float(g['dt']), **kw)).cuda()
    m.load_state_dict(sub(g, 'sd.'))
    return m, g


def queue_fixture_noise(m, g):
    m.flow.odefunc.diffeq._next_noise.clear()
    m.flow.odefunc.diffeq.set_noise(*[{k: v.cuda() for k, v in sub(g, 'noise%d.' % l).items()} for l in range(L_FIX)])
    m.vae.encoder.next_eps = g['eps_s'].cuda()
    if 'eps_v' in g:
        m.vae.encoder_v.next_eps = g['eps_v'].cuda()


def positions(g, ztL):
    return ztL if 'eps_v' not in g else ztL[..., :ztL.shape[-1] // 2]


def decoder64(lat, sd):
    """The eval-mode decoder written out with torch.nn.functional in float64 (sd: the decoder's state_dict entries)."""
    p = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    bn = lambda h, i: torch.relu(Fn.batch_norm(h, p['decnn.%d.running_mean' % i], p['decnn.%d.running_var' % i], p['decnn.%d.weight' % i],
                                               p['decnn.%d.bias' % i], False, 0.0, 1e-5))
    h = Fn.linear(lat.double().reshape(-1, lat.shape[-1]), p['fc.weight'], p['fc.bias'])
    h = h.view(h.shape[0], -1, 4, 4)
    h = bn(Fn.conv_transpose2d(h, p['decnn.1.weight'], p['decnn.1.bias']), 2)
    h = bn(Fn.conv_transpose2d(h, p['decnn.4.weight'], p['decnn.4.bias'], stride=2, padding=1), 5)
    h = bn(Fn.conv_transpose2d(h, p['decnn.7.weight'], p['decnn.7.bias'], stride=2, padding=1, output_padding=1), 8)
    return torch.sigmoid(Fn.conv_transpose2d(h, p['decnn.10.weight'], p['decnn.10.bias'], padding=2))


def stats64(Xrec, X):
    """the notebook's reductions in float64: mse, std, mse_t, mean and unbiased variance over the draws"""
    Xrec, X = Xrec.double().cpu(), X.double().cpu()
    T = X.shape[1]
    se = (Xrec[:, :, :T] - X[None]) ** 2
    return dict(mse=torch.mean(se), std=torch.std(se), mse_t=se.mean(dim=(0, 1, 3, 4, 5)), pmean=Xrec.mean(0),
                pvar=Xrec.var(0) if Xrec.shape[0] > 1 else None)


def fold(dec, lat, X, Th, splits=None, variance=True):
    """dec10_predict over the draws of lat (L,N,Th,q), the draws split over launches as ``splits`` says; -> PredictState"""
    from vae_gp_ode_amd import vae_ops as V
    L, N = lat.shape[0], lat.shape[1]
    st = V.PredictState(N * Th, lat.device, variance)
    c, t8 = dec.decode_frozen_raw(lat)
    c = c.view(L, N * Th, 16, 28, 28)
    l0 = 0
    for n in (splits or [L]):
        V.dec10_predict(c[l0:l0 + n].reshape(-1, 16, 28, 28), t8, dec.decnn[10].weight, dec.decnn[10].bias, X, Th, st)
        l0 += n
    assert l0 == L and st.done == L
    return st


def state_stats(st, N, Th, T, L):
    from vae_gp_ode_amd.evaluate import mean_std, merge_states
    se = st.se.double().cpu().view(N, Th, 3)
    tot = merge_states(se[:, :T].reshape(-1, 3).tolist())
    mse, std = mean_std(tot)
    return dict(mse=torch.tensor(mse), std=torch.tensor(std), mse_t=se[:, :T, 1].mean(0), n=tot[0], se=se,
                pmean=None if st.mean is None else st.mean.view(N, Th, 1, 28, 28),
                pvar=None if st.mean is None or L < 2 else (st.m2 / (L - 1)).view(N, Th, 1, 28, 28))


def check_against(got, ref64, ref32, what, extra=0.0):
    """scalars, mse_t, variance: |got - ref64| <= 2e-4 + 3 relerr(ref32, ref64) in the max norm; every figure is printed first"""
    worst = []
    for k in ('mse', 'std', 'mse_t', 'pvar'):
        if got.get(k) is None or ref64.get(k) is None:
            continue
        e, e32 = relerr(got[k], ref64[k].reshape(got[k].shape)), relerr(ref32[k].reshape(ref64[k].shape), ref64[k])
        print('%s %-5s: %.2e from float64 (reference float32: %.2e, bound %.2e)' % (what, k, e, e32, 2e-4 + 3 * e32 + extra))
        worst.append((k, e, 2e-4 + 3 * e32 + extra))
    for k, e, b in worst:
        assert e < b, (what, k, e, b)


def ref_stats(g, tag):
    return ({k: g[k + tag] for k in ('mse', 'std', 'mse_t')} | {'pvar': g['pvar'], 'pmean': g['pmean']},
            {k: g[k + tag + ('_64' if tag else '64')] for k in ('mse', 'std', 'mse_t')} | {'pvar': g['pvar64'], 'pmean': g['pmean64']})


def random_decoder(seed):
    """a decoder in eval mode whose BatchNorm layers are far from (0, 1) / (1, 0)"""
    from vae_gp_ode_amd.model.core.vae import Decoder
    torch.manual_seed(seed)
    dec = Decoder(latent_dim=6, n_filt=8).cuda().eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i in (2, 5, 8):
            bn = dec.decnn[i]
            C = bn.weight.shape[0]
            bn.running_mean.copy_(0.5 * torch.randn(C, generator=g))
            bn.running_var.copy_(0.5 + 2.0 * torch.rand(C, generator=g))
            bn.weight.copy_(0.5 + torch.rand(C, generator=g))
            bn.bias.copy_(0.3 * torch.randn(C, generator=g))
    return dec


# ---- 1. the decoder alone, fed the reference's own latents -------------------------------------------------------------------------
@pytest.mark.parametrize('name,kw', CASES)
def test_decode_frozen_and_predict_kernel_match_the_reference(name, kw):
    m, g = make_model(name, kw)
    m.eval()
    dec = m.vae.decoder
    lat = positions(g, g['ztL']).cuda()
    L, N, Th = lat.shape[:3]
    T = g['X'].shape[1]
    # the float64 twin used by the end-to-end test is the reference's own float64 decoder
    assert relerr(decoder64(positions(g, g['ztL']), sub(g, 'sd.vae.decoder.')).view(g['Xrec64'].shape), g['Xrec64']) < 1e-12
    Xrec = dec.decode_frozen(lat).view(L, N, Th, 1, 28, 28)
    e = relerr(Xrec, g['Xrec'])
    print(name, 'decode_frozen vs reference float32: %.2e (reference float32 vs float64: %.2e)' % (e, relerr(g['Xrec'], g['Xrec64'])))
    assert e < 2e-4
    assert relerr(dec.decode_frozen(lat, logits=True).sigmoid().view(Xrec.shape), g['Xrec']) < 2e-4
    for tag, tgt in (('', g['X']), ('01', g['X01'])):
        st = fold(dec, lat, tgt.cuda(), Th)
        got = state_stats(st, N, Th, T, L)
        ref32, ref64 = ref_stats(g, tag)
        assert got['n'] == L * N * T * 784
        e = relerr(got['pmean'], g['pmean'])
        print(name, 'targets%s predictive mean vs reference float32: %.2e' % (tag, e))
        assert e < 2e-4
        check_against(got, ref64, ref32, name + ' targets' + tag)
        if Th > T:
            assert (got['se'][:, T:] == 0).all()                      # forecast frames: no target, nothing folded


@pytest.mark.parametrize('B', [512, 4096])
def test_decode_frozen_matches_the_unfused_eval_decoder(B):
    dec = random_decoder(7)
    z = torch.randn(B, 6, generator=torch.Generator().manual_seed(B)).cuda()
    with torch.no_grad():
        ref = dec(z)
        ref_logits = dec(z, logits=True)
    got, got_logits = dec.decode_frozen(z), dec.decode_frozen(z, logits=True)
    assert got.shape == ref.shape == (B, 1, 28, 28) and not got.requires_grad
    e, el = relerr(got, ref), relerr(got_logits, ref_logits)
    print('B=%d: decode_frozen vs Decoder.forward in eval mode: images %.2e, logits %.2e (bitwise: %s); output span %.3f'
          % (B, e, el, torch.equal(got, ref), (ref.max() - ref.min()).item()))
    assert e < 2e-4 and el < 2e-4
    # the same convolution kernels on the same operands: the table route changes where BatchNorm + ReLU is applied, not a bit of the result
    assert torch.equal(got, ref) and torch.equal(got_logits, ref_logits)
    assert (ref.max() - ref.min()).item() > 0.1
    # the table is the arithmetic of gpode_bn_eval: the operand a convolution forms from it is the value bn_eval stores
    from vae_gp_ode_amd import vae_ops as V
    for i in (2, 5, 8):
        bn = dec.decnn[i]
        t = V.bn_eval_table(bn)
        x = torch.randn(4, bn.weight.shape[0], 6, 6, generator=torch.Generator().manual_seed(i)).cuda()
        with torch.no_grad():
            stored = V.batch_norm_eval(x, bn, True)
        formed = torch.relu(torch.addcmul(t[:, 3].view(1, -1, 1, 1), (x - t[:, 0].view(1, -1, 1, 1)) * t[:, 1].view(1, -1, 1, 1), t[:, 2].view(1, -1, 1, 1)))
        assert torch.equal(t[:, 0], bn.running_mean) and torch.equal(t[:, 2], bn.weight.detach()) and torch.equal(t[:, 3], bn.bias.detach())
        assert relerr(formed, stored) < 1e-6                          # (torch's addcmul may or may not fuse; the kernels share bn_math.hpp)
        # bit for bit: the table applied by the library's own bn_affine (gpode_bn_apply) is what gpode_bn_eval writes
        from vae_gp_ode_amd import _lib
        from vae_gp_ode_amd.ops import _ptr, _stream
        applied = torch.empty_like(x)
        _lib.call('gpode_bn_apply', _ptr(x), _ptr(t), _ptr(applied), x.shape[0], x.shape[1], 36, 1, _stream())
        assert torch.equal(applied, stored)
    with pytest.raises(RuntimeError):
        dec.train().decode_frozen(z)


@pytest.mark.parametrize('Lc,N,Th,T', [(4, 8, 16, 16), (8, 32, 16, 16), (12, 40, 16, 16), (6, 24, 32, 16)])
def test_predict_kernel_matches_the_unfused_eval_decoder_at_size(Lc, N, Th, T):
    """gpode_dec10_predict on 512, 4096, 7680 and 4608 images in ONE launch (F = 128 frames; 512 and 640: two and three rounds of the
    grid with the operand prefetch across the frame boundary; 768 with forecast frames; up to 12 draws per frame) against the
    statistics, in float64, of the images the unfused Decoder.forward produces in eval mode."""
    dec = random_decoder(9)
    gen = torch.Generator().manual_seed(Lc * 1000 + N)
    lat = (1.5 * torch.randn(Lc, N, Th, 6, generator=gen)).cuda()
    X = torch.rand(N, T, 1, 28, 28, generator=gen).cuda()
    with torch.no_grad():
        ref = stats64(dec(lat).view(Lc, N, Th, 1, 28, 28), X)
    got = state_stats(fold(dec, lat, X, Th), N, Th, T, Lc)
    assert got['n'] == Lc * N * T * 784 and (got['se'][:, T:] == 0).all() and (got['se'][:, :T, 0] == Lc * 784).all()
    assert ref['pvar'].max().item() > 1e-4
    for k in ('mse', 'std', 'mse_t', 'pvar', 'pmean'):
        e = relerr(got[k], ref[k].reshape(got[k].shape))
        print('%d images (F=%d, Lc=%d) %-5s: %.2e from the unfused eval decoder in float64' % (Lc * N * Th, N * Th, Lc, k, e))
        assert e < 2e-4, (k, e)
    # and the same draws in two launches: the same bits at this size too
    two = fold(dec, lat, X, Th, [Lc // 2, Lc - Lc // 2])
    one = fold(dec, lat, X, Th)
    assert torch.equal(one.mean, two.mean) and torch.equal(one.m2, two.m2) and torch.equal(one.se, two.se)


# ---- 2. end to end against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kw', CASES)
def test_predict_end_to_end_matches_the_reference(name, kw):
    from oracle import gpode_oracle as O
    from vae_gp_ode_amd.evaluate import predict
    m, g = make_model(name, kw)
    X = g['X']
    N, T = X.shape[:2]
    Th = g['ztL'].shape[2]
    a = dict(kernel='RBF', ode=1); a.update(kw)
    # float64 twin: the oracle's flow on the recorded z0 under the recorded draws, then the float64 eval-mode decoder
    p64 = O.to_dtype(O.gp_params_from_state_dict(sub(g, 'sd.')), torch.float64)
    ts = float(g['dt']) * torch.arange(Th, dtype=torch.float64)
    zt64 = torch.stack([O.flow_forward(g['z0'].double(), ts, O.build_cache(p64, O.to_dtype(sub(g, 'noise%d.' % l), torch.float64), a['kernel']),
                                       a['ode'], 'rk4') for l in range(L_FIX)])
    assert zt64.shape == g['ztL'].shape
    X64 = decoder64(positions(g, zt64), sub(g, 'sd.vae.decoder.')).view(g['Xrec'].shape)
    print(name, 'latents: reference float32 vs float64 twin %.2e; images %.2e' % (relerr(g['ztL'], zt64), relerr(g['Xrec'], X64)))
    queue_fixture_noise(m, g)
    p = predict(m, X.cuda(), L_FIX, T_custom=Th if Th > T else None)
    twin, ref32 = stats64(X64, X), stats64(g['Xrec'], X)
    assert tuple(p.mean.shape) == (N, Th, 1, 28, 28) and p.count == L_FIX * N * T * 784 and tuple(p.mse_t.shape) == (T,)
    check_against(dict(mse=torch.tensor(p.mse), std=torch.tensor(p.std), mse_t=p.mse_t, pvar=p.var), twin, ref32, name + ' end to end')
    e, e32 = relerr(p.mean, twin['pmean']), relerr(ref32['pmean'], twin['pmean'])
    print(name, 'end to end predictive mean: %.2e from the twin (reference float32: %.2e)' % (e, e32))
    assert e < 2e-4 + 3 * e32
    # the second target tensor with the encoder still reading X: statistics only, through the same draws
    queue_fixture_noise(m, g)
    m.eval()
    with torch.no_grad():
        z0, _, _ = m.encode_initial_state(X.cuda())
        ztL = m.sample_trajectories(z0, Th, L_FIX)
    st = fold(m.vae.decoder, positions(g, ztL), g['X01'].cuda(), Th)
    check_against(state_stats(st, N, Th, T, L_FIX), stats64(X64, g['X01']), stats64(g['Xrec'], g['X01']), name + ' end to end, targets01')


# ---- 3. against the route that existed before, several passes --------------------------------------------------------------------------
@pytest.mark.parametrize('kw,L,N,T,Tc,ipp', [(dict(), 6, 8, 8, None, 128), (dict(kernel='DF'), 5, 4, 6, 12, 100),
                                              (dict(ode=2, D_in=6, D_out=3, latent_dim=3), 4, 6, 7, None, 42)])
def test_predict_matches_the_unfused_route_on_the_same_draws(kw, L, N, T, Tc, ipp):
    from vae_gp_ode_amd.evaluate import predict
    from vae_gp_ode_amd.model.core.initialization import initialize_and_fix_kernel_parameters
    from vae_gp_ode_amd.model.create_model import build_model
    torch.manual_seed(11)
    m = build_model(model_args(num_inducing=16, num_features=32, dt=0.5, **kw)).cuda()
    initialize_and_fix_kernel_parameters(m, 2.0, 1.0)
    gp = m.flow.odefunc.diffeq
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():
        gp.Um.optvar.add_(2.0 * torch.randn(gp.Um.optvar.shape, generator=gen).cuda())
        for i in (2, 5, 8):
            bn = m.vae.decoder.decnn[i]
            bn.running_mean.copy_(0.3 * torch.randn(bn.weight.shape[0], generator=gen))
            bn.running_var.copy_(0.5 + torch.rand(bn.weight.shape[0], generator=gen))
    X = torch.rand(N, T, 1, 28, 28, generator=gen).cuda()
    noises = [gp._take_noise() for _ in range(L)]
    eps = [torch.randn(N, m.vae.latent_dim, generator=gen).cuda() for _ in range(2)]

    def arm():
        gp._next_noise.clear(); gp.set_noise(*noises)
        m.vae.encoder.next_eps = eps[0]
        if m.order == 2:
            m.vae.encoder_v.next_eps = eps[1]
    m.eval()
    arm()
    with torch.no_grad():
        Xrec, _, _ = m(X, L, T_custom=Tc)
    m.train()
    ref = stats64(Xrec, X)
    arm()
    p = predict(m, X, L, T_custom=Tc, images_per_pass=ipp)
    Th = Tc or T
    assert len(p.passes) >= 3 and sum(p.passes) == L and max(p.passes) * N * Th <= max(ipp, N * Th)
    got = dict(mse=torch.tensor(p.mse), std=torch.tensor(p.std), mse_t=p.mse_t, pvar=p.var)
    for k in ('mse', 'std', 'mse_t', 'pvar'):
        e = relerr(got[k], ref[k].reshape(got[k].shape))
        print('%s L=%d N=%d T=%d Th=%d passes %s  %-5s: %.2e from the unfused route in float64' % (kw, L, N, T, Th, p.passes, k, e))
        assert e < 2e-4, (k, e)
    assert relerr(p.mean, ref['pmean']) < 2e-4
    assert ref['pvar'].max().item() > 1e-6 and p.count == L * N * T * 784
    # whole loader: the merged triples are the statistics of all elements
    from vae_gp_ode_amd.evaluate import compute_mse_std
    halves = [slice(0, N // 2), slice(N // 2, N)]

    def arm_part(sl):
        arm()
        m.vae.encoder.next_eps = eps[0][sl]
        if m.order == 2:
            m.vae.encoder_v.next_eps = eps[1][sl]
    seen = []
    m.eval()
    for sl in halves:
        arm_part(sl)
        with torch.no_grad():
            seen.append(((m(X[sl], L)[0].double() - X[sl].double()[None]) ** 2).reshape(-1).cpu())
    m.train()
    allse = torch.cat(seen)

    class Loader:
        def __iter__(self):
            for i, sl in enumerate(halves):
                arm_part(sl)
                yield X[sl] if i == 0 else (X[sl],)              # a tensor, and a TensorDataset-style 1-tuple
    mse, std = compute_mse_std(m, Loader(), L, images_per_pass=ipp)
    print('loader of two batches: mse %.3e from float64, std %.3e' % (abs(mse - allse.mean().item()) / allse.mean().item(),
                                                                      abs(std - allse.std().item()) / allse.std().item()))
    assert abs(mse - allse.mean().item()) < 2e-4 * allse.mean().item() and abs(std - allse.std().item()) < 2e-4 * allse.std().item()


# ---- 4. determinism: splits over launches, repeated runs ----------------------------------------------------------------------------
def test_draws_split_over_launches_give_identical_bits():
    dec = random_decoder(3)
    gen = torch.Generator().manual_seed(4)
    Lc, N, Th, T = 6, 5, 7, 4
    lat = (1.5 * torch.randn(Lc, N, Th, 6, generator=gen)).cuda()
    X = torch.rand(N, T, 1, 28, 28, generator=gen).cuda()
    runs = [fold(dec, lat, X, Th, s) for s in ([Lc], [Lc], [3, 3], [1, 5], [1] * Lc)]
    a = runs[0]
    assert a.m2.max().item() > 1e-4 and a.se[:, 0].max().item() == Lc * 784
    for b in runs[1:]:
        assert torch.equal(a.mean, b.mean) and torch.equal(a.m2, b.m2) and torch.equal(a.se, b.se)
    nv = fold(dec, lat, X, Th, [2, 4], variance=False)             # statistics only: the same error state
    assert nv.mean is None and torch.equal(nv.se, a.se)


# ---- 5. roll-out beyond the observed window ---------------------------------------------------------------------------------------
def test_t_custom_forecast_frames_add_nothing_to_the_error():
    from vae_gp_ode_amd.evaluate import predict
    name, kw = CASES[2]
    m, g = make_model(name, kw)
    X = g['X'].cuda()
    N, T = X.shape[:2]
    queue_fixture_noise(m, g)
    a = predict(m, X, L_FIX)
    queue_fixture_noise(m, g)
    b = predict(m, X, L_FIX, T_custom=2 * T + 1)
    assert tuple(a.mean.shape) == (N, T, 1, 28, 28) and tuple(b.mean.shape) == tuple(b.var.shape) == (N, 2 * T + 1, 1, 28, 28)
    assert tuple(b.mse_t.shape) == (T,) and a.count == b.count == L_FIX * N * T * 784
    # the first T frames of the longer roll-out are the shorter one (same draws), so the error statistics are the same bits
    assert a.mse == b.mse and a.std == b.std and torch.equal(a.mse_t, b.mse_t) and a.state == b.state
    assert torch.equal(a.mean, b.mean[:, :T]) and torch.equal(a.var, b.var[:, :T])
    assert torch.isfinite(b.mean).all() and (b.var[:, T:] >= 0).all() and b.var[:, T:].max().item() > 0
    # statistics only: nothing would come of the forecast frames, so they are not computed -- and the numbers are the same
    queue_fixture_noise(m, g)
    c = predict(m, X, L_FIX, T_custom=2 * T + 1, variance=False)
    assert c.mean is None and c.var is None and c.state == a.state and torch.equal(c.mse_t, a.mse_t) and c.count == a.count
    with pytest.raises(ValueError):
        predict(m, X, L_FIX, T_custom=T - 1)


# ---- 6. predict leaves the model as it found it ----------------------------------------------------------------------------------
def test_predict_leaves_buffers_flags_and_training_untouched():
    from vae_gp_ode_amd.evaluate import predict
    from vae_gp_ode_amd.model.create_model import compute_loss
    name, kw = CASES[0]
    m, g = make_model(name, kw)
    twin = copy.deepcopy(m)
    X = g['X'].cuda()
    m.train()
    m.vae.encoder.cnn[4].eval()                                       # a mixed state: every flag is restored on its own
    flags = {k: mod.training for k, mod in m.named_modules()}
    before = {k: v.clone() for k, v in m.state_dict().items()}
    predict(m, X, 2, T_custom=9)
    predict(m, X, 1, variance=False)
    assert {k: mod.training for k, mod in m.named_modules()} == flags
    for k, v in m.state_dict().items():
        if 'running' in k or 'num_batches' in k or 'decnn' in k or 'cnn' in k:
            assert torch.equal(v, before[k]), k
    m.vae.encoder.cnn[4].train()
    twin.train()
    outs = []
    for mod in (m, twin):
        queue_fixture_noise(mod, g)
        out = compute_loss(mod, X, L_FIX)
        out[0].backward()
        outs.append(out)
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    for (k, p), (_, q) in zip(m.named_parameters(), twin.named_parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k
    for (k, v), (_, w) in zip(m.state_dict().items(), twin.state_dict().items()):
        if 'running' in k or 'num_batches' in k:
            assert torch.equal(v, w), k
            assert 'num_batches' not in k or v.item() == 4        # three passes in the generator, one training step here


# ---- 7. few frames, ragged grids ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,Th,T,Lc', [(3, 5, 5, 4), (1, 1, 1, 1), (20, 15, 9, 2), (43, 7, 7, 3)])
def test_frame_counts_below_and_across_the_grid(N, Th, T, Lc):
    """F = 15 and 1 (fewer frames than CUs), 300 and 301 (one workgroup per CU, ragged last round)"""
    dec = random_decoder(5)
    gen = torch.Generator().manual_seed(N * 100 + Th)
    lat = (1.5 * torch.randn(Lc, N, Th, 6, generator=gen)).cuda()
    X = torch.rand(N, T, 1, 28, 28, generator=gen).cuda()
    st = fold(dec, lat, X, Th)
    got = state_stats(st, N, Th, T, Lc)
    ref = stats64(dec.decode_frozen(lat).view(Lc, N, Th, 1, 28, 28), X)
    assert got['n'] == Lc * N * T * 784 and (got['se'][:, T:] == 0).all()
    for k in ('mse', 'std', 'mse_t', 'pvar', 'pmean'):
        if got[k] is not None and ref[k] is not None:
            e = relerr(got[k], ref[k].reshape(got[k].shape))
            print('F=%d Lc=%d %-5s: %.2e' % (N * Th, Lc, k, e))
            assert e < 2e-4, (k, e)
    # per frame too: count, mean and M2 of every frame against float64
    img = dec.decode_frozen(lat).view(Lc, N, Th, 784).double().cpu()
    se = (img[:, :, :T] - X.view(N, T, 784).double().cpu()[None]) ** 2
    fm = se.mean(dim=(0, 3))
    fq = ((se - fm[None, :, :, None]) ** 2).sum(dim=(0, 3))
    assert (got['se'][:, :T, 0] == Lc * 784).all()
    assert relerr(got['se'][:, :T, 1], fm) < 2e-4 and relerr(got['se'][:, :T, 2], fq) < 2e-4


def test_binding_argument_checks():
    from vae_gp_ode_amd import _lib, vae_ops as V
    dec = random_decoder(1)
    lat = torch.randn(2, 2, 3, 6).cuda()
    X = torch.rand(2, 3, 1, 28, 28).cuda()
    c, t8 = dec.decode_frozen_raw(lat)
    w, b = dec.decnn[10].weight, dec.decnn[10].bias
    with pytest.raises(_lib.GpodeError):
        V.dec10_predict(c, t8, w, b, X, 3, V.PredictState(5, c.device))          # F is not N * Th
    with pytest.raises(_lib.GpodeError):
        V.dec10_predict(c[:5], t8, w, b, X, 3, V.PredictState(6, c.device))      # not a whole number of draws
    with pytest.raises(_lib.GpodeError):
        V.dec10_predict(c, t8, w, b, torch.rand(2, 4, 1, 28, 28).cuda(), 3, V.PredictState(6, c.device))   # T_obs > Th
    with pytest.raises(_lib.GpodeError):
        V.bn_eval_table(dec.decnn[2].train())


# ---- 8. the command line ----------------------------------------------------------------------------------------------------------
def test_cli_end_to_end_in_a_child_process(tmp_path):
    import glob
    from vae_gp_ode_amd import evaluate as E
    from vae_gp_ode_amd.main import _frames, make_parser
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('WORLD_SIZE', None)
    common = ['--task', 'synthetic', '--Ndata', '8', '--Ntest', '6', '--batch', '4', '--T', '6', '--solver', 'rk4', '--num_inducing', '16',
              '--num_features', '32', '--lr', '1e-4', '--log_freq', '1']
    r = subprocess.run([sys.executable, '-m', 'vae_gp_ode_amd.main'] + common + ['--Nepoch', '1', '--save', 'results/t'], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ck = glob.glob(str(tmp_path / 'results' / 't_*' / 'odegpvae_mnist.pth'))
    assert len(ck) == 1
    # device noise: the reference's host draws use unseeded generators, so only this source repeats between processes
    argv = common + ['--model_path', os.path.dirname(ck[0]), '--eval_sample_size', '5', '--Troll', '2', '--save', 'results/ev',
                     '--device_noise', 'True']
    r = subprocess.run([sys.executable, '-m', 'vae_gp_ode_amd.evaluate'] + argv, cwd=tmp_path, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1]
    out = json.loads(line)
    assert out['L'] == 5 and out['sequences'] == 6 and out['T'] == 6 and out['count'] == 5 * 6 * 6 * 784 and len(out['mse_t']) == 6
    assert out['rollout_sequences'] == 3 and out['rollout_T'] == 12 and out['ranks'] == 1 and out['ms'] > 0
    assert 0 < out['mse'] and 0 < out['std']
    import numpy as np
    assert json.load(open(tmp_path / 'results' / 'ev' / 'eval.json')) == out
    mean, var = np.load(tmp_path / 'results' / 'ev' / 'rollout_mean.npy'), np.load(tmp_path / 'results' / 'ev' / 'rollout_var.npy')
    assert mean.shape == var.shape == (3, 12, 1, 28, 28) and np.isfinite(mean).all() and (var >= 0).all()
    # the same set-up in this process, predict batch by batch: the same seed gives the same draws and every kernel on the way sums in
    # a fixed order, so the statistics are the same numbers
    args = make_parser().parse_args(argv)
    model, testset, _ = E.build_from_checkpoint(args)
    states = [E.predict(model, _frames(b).to(args.device), 5, variance=False).state for b in testset]
    mse, std = E.mean_std(E.merge_states(states))
    print('cli mse %.9g std %.9g; predict mse %.9g std %.9g' % (out['mse'], out['std'], mse, std))
    assert out['mse'] == mse and out['std'] == std
    # more than one rank: refused, and says why
    r = subprocess.run([sys.executable, '-m', 'vae_gp_ode_amd.evaluate'] + argv, cwd=tmp_path, env=dict(env, WORLD_SIZE='2'),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and 'data-parallel evaluation is not built' in r.stderr
