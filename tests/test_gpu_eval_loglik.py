"""GPU: the held-out Bernoulli log-likelihood from the fused predict kernel (gpode_dec10_predict_ll, k_fwd_predict<true>),
evaluate.predict(..., loglik=True) / compute_nll and the command line.

Notation: a = logit of decnn.10, x = target as it is, lp = x a - softplus(a) per pixel, ell[l,f] = sum_p lp (0 for a frame without a
target), ll[l,n] = sum_t ell, nll = -mean ll, nlpd = -mean_n (logsumexp_l ll - log L), nll_t[t] = -mean_{l,n} ell[l, n Th + t].

The bound B against the fixtures.  The suite holds the decoder's logits to relerr < 2e-4 of the largest logit, i.e. every logit to
da = 2e-4 max|a64|; d lp / d a = x - z, so a logit error of da moves ll by at most da sum_{t,p} |x - z64|.  The float64 evaluation is
itself only as good as the reference's float32 result is far from it, which enters three-fold as everywhere in test_gpu_eval.py:
    B[l,n] = da sum_{t,p} |x - z64| + 3 |ll32 - ll64|,      z64 = Xrec64, a64 = log z64 - log1p(-z64),
ll32 the reference's own float32 formula (vae.py:147) on Xrec, ll64 the logit form in float64; per frame the same with the sums over
p only.  B is a cap, not the expected error: every test prints the measured distance beside it.  End to end (encoder and integrator
in the path) the float64 twin of test_gpu_eval.py replaces Xrec64, and its allowance 3 relerr(reference float32, twin) on the images
is propagated the same way, through d lp / d z = (x - z) / (z (1 - z)): + 3 relerr max|z64| sum |x - z64| / (z64 (1 - z64)).
Route against route on the same operands: the suite's standing 2e-4 of the largest value.  Bitwise claims have no tolerance."""
import json
import math
import os

import pytest
import torch

from conftest import sub
from test_eval_loglik_host import fixture_loglik64, loglik64_from_logits
from test_gpu_eval import CASES, L_FIX, decoder64, make_model, model_args, positions, queue_fixture_noise, random_decoder
from test_gpu_forward import relerr

pytestmark = pytest.mark.gpu


def fold(dec, lat, X, Th, splits=None, variance=True, loglik=True):
    """dec10_predict over the draws of lat (L,N,Th,q), split over launches as ``splits`` says, with (or without) the log-likelihood"""
    from vae_gp_ode_amd import vae_ops as V
    L, N = lat.shape[0], lat.shape[1]
    st = V.PredictState(N * Th, lat.device, variance, loglik=L if loglik else 0)
    c, t8 = dec.decode_frozen_raw(lat)
    c = c.view(L, N * Th, 16, 28, 28)
    l0 = 0
    for n in (splits or [L]):
        V.dec10_predict(c[l0:l0 + n].reshape(-1, 16, 28, 28), t8, dec.decnn[10].weight, dec.decnn[10].bias, X, Th, st)
        l0 += n
    assert l0 == L and st.done == L
    return st


def route_ell64(dec, lat, X):
    """float64 logit form on the logits of decode_frozen(lat, logits=True), the route the suite already tests: (L,N,T)"""
    L, N, Th = lat.shape[:3]
    T = X.shape[1]
    a = dec.decode_frozen(lat, logits=True).view(L, N, Th, 784)[:, :, :T]
    return loglik64_from_logits(a.double().cpu(), X.view(N, T, 784).double().cpu()[None]), a


# ---- 1. the kernel on the reference's latents ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kw', CASES)
def test_kernel_loglik_matches_float64_on_the_reference_latents(name, kw):
    from vae_gp_ode_amd.evaluate import loglik_stats
    m, g = make_model(name, kw)
    m.eval()
    lat = positions(g, g['ztL']).cuda()
    L, N, Th = lat.shape[:3]
    T = g['X'].shape[1]
    for tag in ('X', 'X01'):
        r = fixture_loglik64(g, g[tag])
        st = fold(m.vae.decoder, lat, g[tag].cuda(), Th)
        ell = st.ell.double().cpu().view(L, N, Th)
        assert torch.isfinite(ell).all()
        if Th > T:
            assert (ell[:, :, T:] == 0).all()                         # forecast frames: no target, exactly 0
        ll, nll, nlpd, nll_t = loglik_stats(ell, T)
        _, nll64, nlpd64, _ = loglik_stats(r['ell64'], T)
        d_f, d_s = (ell[:, :, :T] - r['ell64']).abs(), (ll - r['ll64']).abs()
        cap = r['B'].max(0).values.mean().item()                      # mean_n max_l B
        print('%s targets %s: ell %.3e (min bound %.3e, worst ratio %.3f); ll %.3e (worst ratio %.3f of B, max B %.3f); nll %.6f (%.2e off), '
              'nlpd %.6f (%.2e off), cap %.3f; nll - nlpd %.3f (float64 %.3f)' %
              (name, tag, d_f.max().item(), r['Bf'].min().item(), (d_f / r['Bf']).max().item(), d_s.max().item(), (d_s / r['B']).max().item(),
               r['B'].max().item(), nll, abs(nll - nll64), nlpd, abs(nlpd - nlpd64), cap, nll - nlpd, nll64 - nlpd64))
        assert (d_f <= r['Bf']).all() and (d_s <= r['B']).all()
        assert abs(nll - nll64) <= cap and abs(nlpd - nlpd64) <= cap
        if tag == 'X':
            assert nll64 - nlpd64 > 4 * r['B'].max().item()           # the two numbers are further apart than the bound can bridge
            assert nlpd < nll


# ---- 2. the variant changes nothing else ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Lc,N,Th,T', [(6, 5, 7, 4), (4, 8, 16, 16)])
def test_state_is_bit_identical_with_and_without_loglik(Lc, N, Th, T):
    dec = random_decoder(3)
    gen = torch.Generator().manual_seed(Lc * 10 + N)
    lat = (1.5 * torch.randn(Lc, N, Th, 6, generator=gen)).cuda()
    X = torch.rand(N, T, 1, 28, 28, generator=gen).cuda()
    for splits in (None, [1, Lc - 1]):
        a, b = fold(dec, lat, X, Th, splits, loglik=False), fold(dec, lat, X, Th, splits, loglik=True)
        assert a.ell is None and tuple(b.ell.shape) == (Lc, N * Th)
        assert torch.equal(a.se, b.se) and torch.equal(a.mean, b.mean) and torch.equal(a.m2, b.m2)
        assert a.m2.max().item() > 1e-4 and a.se[:, 0].max().item() == Lc * 784 and b.ell.abs().max().item() > 1
    a, b = fold(dec, lat, X, Th, variance=False, loglik=False), fold(dec, lat, X, Th, variance=False, loglik=True)
    assert a.mean is None and b.mean is None and torch.equal(a.se, b.se)


# ---- 3. determinism -------------------------------------------------------------------------------------------------------------------
def test_loglik_bits_do_not_depend_on_the_split_the_run_or_the_moments():
    dec = random_decoder(3)
    gen = torch.Generator().manual_seed(4)
    Lc, N, Th, T = 6, 5, 7, 4
    lat = (1.5 * torch.randn(Lc, N, Th, 6, generator=gen)).cuda()
    X = torch.rand(N, T, 1, 28, 28, generator=gen).cuda()
    runs = [fold(dec, lat, X, Th, s) for s in ([Lc], [Lc], [3, 3], [1, 5], [1] * Lc)]
    a = runs[0]
    assert torch.isfinite(a.ell).all() and (a.ell.view(Lc, N, Th)[:, :, :T] < -100).all() and (a.ell.view(Lc, N, Th)[:, :, T:] == 0).all()
    for b in runs[1:]:
        assert torch.equal(a.ell, b.ell) and torch.equal(a.se, b.se) and torch.equal(a.mean, b.mean) and torch.equal(a.m2, b.m2)
    nv = fold(dec, lat, X, Th, [2, 4], variance=False)
    assert nv.mean is None and torch.equal(nv.ell, a.ell) and torch.equal(nv.se, a.se)


# ---- 4. few frames, ragged grids, 512 images ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,Th,T,Lc', [(1, 1, 1, 1), (3, 5, 5, 4), (43, 7, 7, 3), (8, 16, 16, 4)])
def test_loglik_across_frame_counts(N, Th, T, Lc):
    """F = 1, 15 (fewer frames than CUs), 301 (ragged second round of the grid) and 128 frames x 4 draws = 512 images"""
    dec = random_decoder(5)
    gen = torch.Generator().manual_seed(N * 100 + Th)
    lat = (1.5 * torch.randn(Lc, N, Th, 6, generator=gen)).cuda()
    X = torch.rand(N, T, 1, 28, 28, generator=gen).cuda()
    ref, _ = route_ell64(dec, lat, X)
    ell = fold(dec, lat, X, Th).ell.double().cpu().view(Lc, N, Th)
    e = relerr(ell, ref)
    print('F=%d Lc=%d: ell %.2e of max|ell| = %.1f from the float64 logit form on the tested route\'s logits' % (N * Th, Lc, e, ref.abs().max().item()))
    assert e < 2e-4


# ---- 5. saturation -------------------------------------------------------------------------------------------------------------------
def test_confident_pixels_stay_finite():
    dec = random_decoder(6)
    gen = torch.Generator().manual_seed(8)
    Lc, N, Th = 3, 4, 5
    lat = (1.5 * torch.randn(Lc, N, Th, 6, generator=gen)).cuda()
    X = (torch.rand(N, Th, 1, 28, 28, generator=gen) < 0.5).float().cuda()
    with torch.no_grad():
        a0 = dec.decode_frozen(lat, logits=True)
        dec.decnn[10].weight.mul_(80.0 / a0.abs().max().item())
    ref, a = route_ell64(dec, lat, X)
    assert a.abs().max().item() > 40
    z = dec.decode_frozen(lat).view(Lc, N, Th, 784)
    x = X.view(N, Th, 784)[None]
    ll32 = (torch.log(z) * x + torch.log(1 - z) * (1 - x)).sum(-1)                   # the reference's formula (vae.py:147) in float32
    assert not torch.isfinite(ll32).all(), 'the case does not bite: the float32 z form is finite'
    ell = fold(dec, lat, X, Th).ell.double().cpu().view(Lc, N, Th)
    assert torch.isfinite(ell).all()
    e = relerr(ell, ref)
    print('max|a| = %.1f, %d of %d frames non-finite in the float32 z form; device ell %.2e of max|ell| = %.1f from float64' %
          (a.abs().max().item(), (~torch.isfinite(ll32)).sum().item(), ll32.numel(), e, ref.abs().max().item()))
    assert e < 2e-4


# ---- 6. end to end against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kw', CASES)
def test_predict_loglik_end_to_end_matches_the_reference(name, kw):
    from oracle import gpode_oracle as O
    from vae_gp_ode_amd.evaluate import loglik_stats, predict
    m, g = make_model(name, kw)
    X = g['X']
    N, T = X.shape[:2]
    Th = g['ztL'].shape[2]
    a = dict(kernel='RBF', ode=1); a.update(kw)
    # the float64 twin, built exactly as test_predict_end_to_end_matches_the_reference builds it
    p64 = O.to_dtype(O.gp_params_from_state_dict(sub(g, 'sd.')), torch.float64)
    ts = float(g['dt']) * torch.arange(Th, dtype=torch.float64)
    zt64 = torch.stack([O.flow_forward(g['z0'].double(), ts, O.build_cache(p64, O.to_dtype(sub(g, 'noise%d.' % l), torch.float64), a['kernel']),
                                       a['ode'], 'rk4') for l in range(L_FIX)])
    X64 = decoder64(positions(g, zt64), sub(g, 'sd.vae.decoder.')).view(g['Xrec'].shape)
    r = fixture_loglik64(g, X, z64=X64)
    rel = relerr(g['Xrec'], X64)
    z, x = X64[:, :, :T].double(), X.double()[None]
    slope = ((x - z).abs() / (z * (1 - z))).sum(dim=(3, 4, 5))         # |d ell / d z| summed over the frame's pixels: (L,N,T)
    Bf = r['Bf'] + 3 * rel * z.max() * slope
    B = r['B'] + 3 * rel * z.max() * slope.sum(2)
    queue_fixture_noise(m, g)
    p = predict(m, X.cuda(), L_FIX, T_custom=Th if Th > T else None, loglik=True)
    ll64, nll64, nlpd64, nll_t64 = loglik_stats(r['ell64'], T)
    assert tuple(p.ll.shape) == (L_FIX, N) and p.ll.dtype == torch.float64 and p.ll.device.type == 'cpu' and tuple(p.nll_t.shape) == (T,)
    assert isinstance(p.nll, float) and isinstance(p.nlpd, float)
    cap, cap_t = B.max(0).values.mean().item(), Bf.mean(dim=(0, 1))
    d = (p.ll - ll64).abs()
    print('%s end to end (images: reference float32 vs twin %.2e): ll %.3e (worst ratio %.3f of B, max B %.3f); nll %.6f (%.2e off), nlpd %.6f '
          '(%.2e off), cap %.3f; nll_t worst ratio %.3f' % (name, rel, d.max().item(), (d / B).max().item(), B.max().item(), p.nll,
                                                            abs(p.nll - nll64), p.nlpd, abs(p.nlpd - nlpd64), cap,
                                                            ((p.nll_t - nll_t64).abs() / cap_t).max().item()))
    assert (d <= B).all() and abs(p.nll - nll64) <= cap and abs(p.nlpd - nlpd64) <= cap and ((p.nll_t - nll_t64).abs() <= cap_t).all()
    assert p.nlpd <= p.nll
    # the other fields: the same bits as a plain predict on the same noise
    queue_fixture_noise(m, g)
    q = predict(m, X.cuda(), L_FIX, T_custom=Th if Th > T else None)
    assert q.ll is None and q.nll is None and q.nlpd is None and q.nll_t is None
    assert p.mse == q.mse and p.std == q.std and p.count == q.count and p.state == q.state and torch.equal(p.mse_t, q.mse_t)
    assert torch.equal(p.mean, q.mean) and torch.equal(p.var, q.var) and p.passes == q.passes


# ---- 7. against the route that existed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw,L,N,T,Tc,ipp', [(dict(), 6, 8, 8, None, 128), (dict(kernel='DF'), 5, 4, 6, 12, 100),
                                              (dict(ode=2, D_in=6, D_out=3, latent_dim=3), 4, 6, 7, None, 42)])
def test_nll_matches_compute_loss_on_the_same_draws(kw, L, N, T, Tc, ipp):
    from vae_gp_ode_amd.evaluate import compute_nll, log_mean_exp, predict
    from vae_gp_ode_amd.model.core.initialization import initialize_and_fix_kernel_parameters
    from vae_gp_ode_amd.model.create_model import build_model, compute_loss
    # the random models of test_predict_matches_the_unfused_route_on_the_same_draws
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

    def arm(sl=slice(None)):
        gp._next_noise.clear(); gp.set_noise(*noises)
        m.vae.encoder.next_eps = eps[0][sl]
        if m.order == 2:
            m.vae.encoder_v.next_eps = eps[1][sl]
    m.eval()
    arm()
    with torch.no_grad():
        ref = compute_loss(m, X, L)[1].item()
    m.train()
    arm()
    p = predict(m, X, L, T_custom=Tc, images_per_pass=ipp, loglik=True)
    assert len(p.passes) >= 3 and sum(p.passes) == L
    e = abs(p.nll - ref) / abs(ref)
    print('%s L=%d N=%d T=%d passes %s: nll %.6f, compute_loss in eval mode %.6f: %.2e relative; nlpd %.6f' % (kw, L, N, T, p.passes, p.nll, ref, e, p.nlpd))
    assert e < 2e-4 and p.nlpd <= p.nll
    # a loader of two batches of unequal size: the float64 statistics of all sequences, from the unfused route's logits
    parts = [slice(0, N // 2 - 1), slice(N // 2 - 1, N)]
    seen = []
    m.eval()
    for sl in parts:
        arm(sl)
        with torch.no_grad():
            logits = m(X[sl], L, logits=True)[0]
        seen.append(loglik64_from_logits(logits.reshape(L, X[sl].shape[0], T, 784).double().cpu(), X[sl].view(-1, T, 784).double().cpu()[None]).sum(2))
    m.train()
    ll = torch.cat(seen, dim=1)
    assert tuple(ll.shape) == (L, N)
    nll64, nlpd64 = -ll.mean().item(), -log_mean_exp(ll).mean().item()

    class Loader:
        def __iter__(self):
            for i, sl in enumerate(parts):
                arm(sl)
                yield X[sl] if i == 0 else (X[sl],)
    nll, nlpd = compute_nll(m, Loader(), L, images_per_pass=ipp)
    print('loader of %d + %d sequences: nll %.2e, nlpd %.2e relative to float64 (nll - nlpd = %.3f)' %
          (parts[0].stop, N - parts[0].stop, abs(nll - nll64) / abs(nll64), abs(nlpd - nlpd64) / abs(nlpd64), nll64 - nlpd64))
    assert abs(nll - nll64) < 2e-4 * abs(nll64) and abs(nlpd - nlpd64) < 2e-4 * abs(nlpd64)


# ---- 8. the command line, in process ------------------------------------------------------------------------------------------------------
def test_cli_reports_the_loglik(tmp_path, capsys):
    from vae_gp_ode_amd import evaluate as E
    from vae_gp_ode_amd.main import _frames, make_parser
    from vae_gp_ode_amd.model.create_model import build_model
    from vae_gp_ode_amd.model.misc.torch_utils import seed_everything
    argv = ['--task', 'synthetic', '--Ndata', '8', '--Ntest', '6', '--batch', '4', '--T', '6', '--solver', 'rk4', '--num_inducing', '16',
            '--num_features', '32', '--model_path', str(tmp_path), '--eval_sample_size', '4', '--Troll', '2', '--save', str(tmp_path / 'ev'),
            '--device_noise', 'True']
    args = make_parser().parse_args(argv)
    args.device = torch.device('cuda')
    seed_everything(3)
    torch.save(build_model(args).to(args.device).state_dict(), tmp_path / 'odegpvae_mnist.pth')
    capsys.readouterr()
    ret = E.main(argv)
    out = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')][-1])
    assert out == json.loads(json.dumps(ret)) and json.load(open(tmp_path / 'ev' / 'eval.json')) == out
    assert out['L'] == 4 and out['sequences'] == 6 and out['T'] == 6 and len(out['nll_t']) == 6 and len(out['mse_t']) == 6
    assert math.isfinite(out['nll']) and math.isfinite(out['nlpd']) and out['nlpd'] <= out['nll'] and out['nll'] > 0
    assert abs(sum(out['nll_t']) - out['nll']) < 1e-9 * out['nll']
    # the same set-up again, batch by batch: the same seed gives the same draws, every sum has a fixed order
    args = make_parser().parse_args(argv)
    model, testset, _ = E.build_from_checkpoint(args)
    nseq, nll, nlpd, nll_t, states, states_plain = 0, 0.0, 0.0, None, [], []
    for b in testset:
        Xb = _frames(b).to(args.device)
        p = E.predict(model, Xb, 4, variance=False, loglik=True)
        nseq += Xb.shape[0]
        nll += p.nll * Xb.shape[0]
        nlpd += p.nlpd * Xb.shape[0]
        nll_t = p.nll_t * Xb.shape[0] if nll_t is None else nll_t + p.nll_t * Xb.shape[0]
        states.append(p.state)
    print('cli nll %.9g nlpd %.9g; predict nll %.9g nlpd %.9g' % (out['nll'], out['nlpd'], nll / nseq, nlpd / nseq))
    assert out['nll'] == nll / nseq and out['nlpd'] == nlpd / nseq and out['nll_t'] == (nll_t / nseq).tolist()
    # mse / std are those of a plain predict, bit for bit
    model, testset, _ = E.build_from_checkpoint(make_parser().parse_args(argv))
    states_plain = [E.predict(model, _frames(b).to('cuda'), 4, variance=False).state for b in testset]
    assert states_plain == states
    mse, std = E.mean_std(E.merge_states(states_plain))
    assert out['mse'] == mse and out['std'] == std


# ---- 9. binding checks --------------------------------------------------------------------------------------------------------------------
def test_binding_refusals_name_the_entry_point_and_write_nothing():
    from vae_gp_ode_amd import _lib, vae_ops as V
    from vae_gp_ode_amd.ops import _ptr, _stream
    dec = random_decoder(1)
    lat = torch.randn(2, 2, 3, 6).cuda()
    X = torch.rand(2, 3, 1, 28, 28).cuda()
    c, t8 = dec.decode_frozen_raw(lat)
    w, b = dec.decnn[10].weight.detach(), dec.decnn[10].bias.detach()

    def nan_state(F, L):
        st = V.PredictState(F, c.device, True, loglik=L)
        for t in (st.ell, st.se, st.mean, st.m2):
            t.fill_(float('nan'))
        return st

    def untouched(st):
        torch.cuda.synchronize()
        return all(torch.isnan(t).all().item() for t in (st.ell, st.se, st.mean, st.m2)) and st.done == 0

    def raw(st, Lc, F, Th, ell, L_total):
        _lib.call('gpode_dec10_predict_ll', _ptr(c), _ptr(t8), _ptr(w), _ptr(b), _ptr(X), Lc, F, Th, 3, 0, _ptr(st.mean), _ptr(st.m2), _ptr(st.se),
                  _ptr(ell), L_total, _stream())
    st = nan_state(6, 2)
    with pytest.raises(_lib.GpodeError, match='gpode_dec10_predict_ll'):
        raw(st, 2, 6, 3, None, 2)                                      # ell missing
    with pytest.raises(_lib.GpodeError, match='gpode_dec10_predict_ll'):
        raw(st, 2, 6, 3, st.ell, 1)                                    # L_total too small for done + Lc
    with pytest.raises(_lib.GpodeError, match='gpode_dec10_predict_ll'):
        raw(st, 2, 5, 3, st.ell, 2)                                    # F is not a multiple of Th
    assert untouched(st)
    # through vae_ops: a state with room for one draw handed two; a state whose F is not N * Th
    one = nan_state(6, 1)
    with pytest.raises(_lib.GpodeError, match='gpode_dec10_predict_ll'):
        V.dec10_predict(c, t8, w, b, X, 3, one)
    assert untouched(one)
    bad = nan_state(5, 2)
    with pytest.raises(_lib.GpodeError, match='dec10_predict'):
        V.dec10_predict(c, t8, w, b, X, 3, bad)
    assert untouched(bad)
    # and the call the refusals were variations of goes through
    V.dec10_predict(c, t8, w, b, X, 3, st)
    assert st.done == 2 and torch.isfinite(st.ell).all() and torch.isfinite(st.se).all()
