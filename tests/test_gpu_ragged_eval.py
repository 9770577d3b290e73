"""GPU: evaluation on ragged sequences -- gpode_dec10_predict_len / gpode_dec10_predict_ll_len (k_fwd_predict<LL, true>) and
evaluate.predict(..., n_obs=).  A ragged batch is a padded one: X (N,T_obs,1,28,28), n_obs (N,) int32, frame t of sequence n has a target
iff t < min(T_obs, n_obs[n]).

The kernels at 2 draws x (N = 3, Th = 4, T_obs = 3) with lengths [3, 1, 2], against the twins run on the same inputs: frames with a
target have the twin's bits in se_state and ell, frames without one leave count 0 and ell 0 (as the forecast frame t = 3 does),
pred_mean / pred_m2 are the twin's everywhere, a split of the draws over two launches equals one launch, NaN in the padded targets
changes nothing, full lengths give the twin's bits, and n_obs == NULL is refused with nothing written.

predict(..., n_obs=) on a tiny random model: mse, mse_t, nll and nll_t against a float64 recomputation from the unfused route
(``model.eval(); model(X, L)`` on the same draws) over the observed frames, to the bounds test_gpu_eval.py (2e-4 of the largest value:
mse, mse_t) and test_gpu_eval_loglik.py (2e-4 relative: nll; route against route 2e-4 of the largest value: nll_t) use for them."""
import pytest
import torch

from test_eval_loglik_host import loglik64_from_logits
from test_gpu_eval import model_args, random_decoder
from test_gpu_forward import relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def leave_the_global_generators_as_found():
    """The tests of this file seed and draw from the process-wide generators (torch on the host and on the device, numpy through
    build_model, random through main()); test files that run after this one build layers from the global generator without seeding it
    (the decoder chain of test_gpu_vae_layers.py), so what they see must not depend on whether this file ran: the states are put back
    when it is done, as test_gpu_time_grids.py does."""
    import random
    import numpy as np
    saved = (torch.get_rng_state(), torch.cuda.get_rng_state_all(), np.random.get_state(), random.getstate())
    yield
    torch.set_rng_state(saved[0])
    torch.cuda.set_rng_state_all(saved[1])
    np.random.set_state(saved[2])
    random.setstate(saved[3])

L, N, TH, T, LENS = 2, 3, 4, 3, [3, 1, 2]


def fold(dec, lat, X, Th, n_obs=None, splits=None, variance=True, loglik=True):
    from vae_gp_ode_amd import vae_ops as V
    Ld, Nd = lat.shape[0], lat.shape[1]
    st = V.PredictState(Nd * Th, lat.device, variance, loglik=Ld if loglik else 0)
    c, t8 = dec.decode_frozen_raw(lat)
    c = c.view(Ld, Nd * Th, 16, 28, 28)
    l0 = 0
    for n in (splits or [Ld]):
        kw = {} if n_obs is None else {'n_obs': n_obs}
        V.dec10_predict(c[l0:l0 + n].reshape(-1, 16, 28, 28), t8, dec.decnn[10].weight, dec.decnn[10].bias, X, Th, st, **kw)
        l0 += n
    assert l0 == Ld and st.done == Ld
    return st


@pytest.fixture(scope='module')
def setup():
    dec = random_decoder(3)
    gen = torch.Generator().manual_seed(21)
    lat = (1.5 * torch.randn(L, N, TH, 6, generator=gen)).cuda()
    X = torch.rand(N, T, 1, 28, 28, generator=gen).cuda()
    n_obs = torch.tensor(LENS, dtype=torch.int32, device='cuda')
    has = (torch.arange(TH)[None, :] < torch.tensor(LENS)[:, None]) & (torch.arange(TH)[None, :] < T)     # (N,Th)
    return dec, lat, X, n_obs, has.reshape(-1).cuda()


def _tag():
    from vae_gp_ode_amd import _lib
    return _lib.load().gpode_last_launch().decode()


@pytest.mark.parametrize('loglik', [True, False], ids=['ll', 'plain'])
def test_kernel_against_the_twin(setup, loglik):
    dec, lat, X, n_obs, has = setup
    twin = fold(dec, lat, X, TH, loglik=loglik)
    assert _tag() == ('dec10_predict_ll' if loglik else 'dec10_predict')
    got = fold(dec, lat, X, TH, n_obs, loglik=loglik)
    assert _tag() == ('dec10_predict_ll_len' if loglik else 'dec10_predict_len')
    assert has.sum().item() == sum(LENS)
    assert torch.equal(got.se[has], twin.se[has]) and bool((got.se[has][:, 0] == L * 784).all())
    assert bool((got.se[~has] == 0).all()), 'a frame without a target has a count'
    assert torch.equal(got.mean, twin.mean) and torch.equal(got.m2, twin.m2)
    if loglik:
        assert torch.equal(got.ell[:, has], twin.ell[:, has]) and bool((got.ell[:, has] < -100).all())
        assert bool((got.ell[:, ~has] == 0).all()), 'a frame without a target has a likelihood'
    # a two-launch split of the draws equals one launch; a second run gives the same bits
    for other in (fold(dec, lat, X, TH, n_obs, splits=[1, 1], loglik=loglik), fold(dec, lat, X, TH, n_obs, loglik=loglik)):
        assert torch.equal(other.se, got.se) and torch.equal(other.mean, got.mean) and torch.equal(other.m2, got.m2)
        assert not loglik or torch.equal(other.ell, got.ell)
    # full lengths (and beyond): the twin's bits everywhere
    for full in ([T] * N, [T + 2, T, TH + 5]):
        f = fold(dec, lat, X, TH, torch.tensor(full, dtype=torch.int32, device='cuda'), loglik=loglik)
        assert torch.equal(f.se, twin.se) and torch.equal(f.mean, twin.mean) and torch.equal(f.m2, twin.m2)
        assert not loglik or torch.equal(f.ell, twin.ell)
    # no frame at all
    none = fold(dec, lat, X, TH, torch.tensor([0, -2, 0], dtype=torch.int32, device='cuda'), loglik=loglik)
    assert bool((none.se == 0).all()) and torch.equal(none.mean, twin.mean) and (not loglik or bool((none.ell == 0).all()))


@pytest.mark.parametrize('bad', [float('nan'), float('inf')], ids=['nan', 'inf'])
def test_padded_targets_are_never_read_into_a_result(setup, bad):
    dec, lat, X, n_obs, has = setup
    got = fold(dec, lat, X, TH, n_obs)
    Xb = X.clone()
    for n, k in enumerate(LENS):
        Xb[n, k:] = bad
    gb = fold(dec, lat, Xb, TH, n_obs)
    assert torch.equal(gb.se, got.se) and torch.equal(gb.ell, got.ell) and torch.equal(gb.mean, got.mean) and torch.equal(gb.m2, got.m2)
    assert bool(torch.isfinite(gb.se).all()) and bool(torch.isfinite(gb.ell).all())


def test_refusals_write_nothing(setup):
    from vae_gp_ode_amd import _lib, vae_ops as V
    from vae_gp_ode_amd.ops import _ptr, _stream
    dec, lat, X, n_obs, _ = setup
    c, t8 = dec.decode_frozen_raw(lat)
    w, b = dec.decnn[10].weight.detach(), dec.decnn[10].bias.detach()
    st = V.PredictState(N * TH, c.device, True, loglik=L)
    for t in (st.ell, st.se, st.mean, st.m2):
        t.fill_(float('nan'))
    with pytest.raises(_lib.GpodeError, match='gpode_dec10_predict_ll_len'):
        _lib.call('gpode_dec10_predict_ll_len', _ptr(c), _ptr(t8), _ptr(w), _ptr(b), _ptr(X), L, N * TH, TH, T, 0, _ptr(st.mean), _ptr(st.m2),
                  _ptr(st.se), _ptr(st.ell), L, _ptr(None), _stream())
    with pytest.raises(_lib.GpodeError, match='gpode_dec10_predict_len'):
        _lib.call('gpode_dec10_predict_len', _ptr(c), _ptr(t8), _ptr(w), _ptr(b), _ptr(X), L, N * TH, TH, T, 0, _ptr(st.mean), _ptr(st.m2),
                  _ptr(st.se), _ptr(None), _stream())
    for wrong in (n_obs.long(), n_obs[:2], n_obs.cpu()):                # dtype, shape, device: refused by the binding
        with pytest.raises(_lib.GpodeError, match='n_obs'):
            V.dec10_predict(c, t8, w, b, X, TH, st, n_obs=wrong)
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all().item() for t in (st.ell, st.se, st.mean, st.m2)) and st.done == 0


def test_predict_with_counts_matches_the_unfused_route_in_float64():
    kw = dict()
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
    n_obs = torch.tensor(LENS, dtype=torch.int32, device='cuda')
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
        Xrec = m(X, L, T_custom=TH)[0]
    arm()
    with torch.no_grad():
        logits = m(X, L, T_custom=TH, logits=True)[0]
    m.train()
    obs = torch.arange(T)[None, :] < torch.tensor(LENS)[:, None]                         # (N,T)
    se = ((Xrec.double().cpu()[:, :, :T] - X.double().cpu()[None]) ** 2).reshape(L, N, T, 784)
    ell = loglik64_from_logits(logits.reshape(L, N, TH, 784)[:, :, :T].double().cpu(), X.view(N, T, 784).double().cpu()[None])   # (L,N,T)
    mse64 = se[:, obs].mean()
    mse_t64 = torch.stack([se[:, obs[:, t], t].mean() for t in range(T)])
    nll64 = -ell.masked_fill(~obs[None], 0.0).sum(2).mean()
    nll_t64 = torch.stack([-ell[:, obs[:, t], t].mean() for t in range(T)])
    arm()
    p = predict(m, X, L, T_custom=TH, loglik=True, n_obs=n_obs)
    e = dict(mse=relerr(torch.tensor(p.mse), mse64), mse_t=relerr(p.mse_t, mse_t64), nll=abs(p.nll - nll64.item()) / abs(nll64.item()),
             nll_t=relerr(p.nll_t, nll_t64))
    print('%s: predict with n_obs = %s against the unfused route in float64: %s' % (kw, LENS, {k: '%.2e' % v for k, v in e.items()}))
    assert p.count == L * 784 * sum(LENS)
    assert all(v < 2e-4 for v in e.values()), e
    # the predictive moments do not depend on the counts
    arm()
    q = predict(m, X, L, T_custom=TH, loglik=True)
    assert torch.equal(p.mean, q.mean) and torch.equal(p.var, q.var)
    # a frame index no sequence has: nan, not a number from the padding
    arm()
    r = predict(m, X, L, T_custom=TH, loglik=True, n_obs=torch.tensor([2, 1, 2], dtype=torch.int32, device='cuda'))
    assert torch.isnan(r.mse_t[2]) and torch.isnan(r.nll_t[2]) and bool(torch.isfinite(r.mse_t[:2]).all()) and r.count == L * 784 * 5
