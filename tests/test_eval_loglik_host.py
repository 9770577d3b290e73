"""CPU-only: the host side of the held-out log-likelihood (evaluate.log_mean_exp / loglik_stats / compute_nll, the Prediction fields,
the header and the binding table), and the float64 facts about the committed fixtures that the GPU tests' bound B rests on."""
import math
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden

FIXTURES = ['eval_rbf1', 'eval_rbf2', 'eval_df1', 'eval_rbf1_roll']


# ---- log-mean-exp ------------------------------------------------------------------------------------------------------------------
def test_log_mean_exp_matches_logsumexp_where_a_plain_exp_underflows():
    from vae_gp_ode_amd.evaluate import log_mean_exp
    g = torch.Generator().manual_seed(1)
    L = 7
    cols = [torch.randn(L, generator=g, dtype=torch.float64),                       # ordinary
            -3000.0 + 5.0 * torch.randn(L, generator=g, dtype=torch.float64),       # exp underflows to 0 in float64
            -1e5 + 40.0 * torch.randn(L, generator=g, dtype=torch.float64),
            torch.full((L,), -3000.0, dtype=torch.float64),                         # draws differ by 0
            -3000.0 + 1e-9 * torch.arange(L, dtype=torch.float64),                  # ... by 1e-9
            -3000.0 - 50.0 * torch.arange(L, dtype=torch.float64),                  # ... by 50: one draw carries the mean
            -1e5 + torch.tensor([0.0, 0.0, 1e-9, 50.0, -50.0, 1.0, 0.0], dtype=torch.float64)]
    ll = torch.stack(cols, dim=1)
    assert (torch.exp(ll[:, 1:]) == 0).all()                                        # the case bites: the naive form is log(0)
    ref = torch.logsumexp(ll, dim=0) - math.log(L)
    got = log_mean_exp(ll)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(cols),) and torch.isfinite(got).all()
    err = ((got - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
    print('log_mean_exp against torch.logsumexp: %.2e relative' % err)
    assert err < 1e-15
    assert got[3].item() == -3000.0                                                 # equal draws: their common value
    assert abs(got[5].item() - (-3000.0 - math.log(L))) < 1e-12                     # one dominant draw: its value less log L
    # float32 input is promoted, a single draw is returned as it is, and the same input gives the same bits
    assert torch.equal(log_mean_exp(ll[:1]), ll[0])
    assert log_mean_exp(ll.float()).dtype == torch.float64
    assert torch.equal(log_mean_exp(ll), got)


def test_nlpd_equals_nll_for_one_draw_and_never_exceeds_it():
    from vae_gp_ode_amd.evaluate import loglik_stats
    g = torch.Generator().manual_seed(2)
    ell = -400.0 + 30.0 * torch.randn(1, 5, 9, generator=g, dtype=torch.float64)
    ll, nll, nlpd, nll_t = loglik_stats(ell, 6)
    assert tuple(ll.shape) == (1, 5) and tuple(nll_t.shape) == (6,) and nlpd == nll
    assert torch.equal(ll, ell[:, :, :6].sum(2))                                    # frames beyond T_obs are left out
    assert abs(nll - (-ll.mean().item())) == 0 and abs(nll_t.sum().item() - nll) < 1e-9 * abs(nll)
    for L in (2, 3, 8):
        ell = -400.0 + 30.0 * torch.randn(L, 5, 6, generator=g, dtype=torch.float64)
        ll, nll, nlpd, nll_t = loglik_stats(ell, 6)
        ref = -(torch.logsumexp(ll, 0) - math.log(L)).mean().item()
        assert nlpd <= nll and abs(nlpd - ref) < 1e-12 * abs(ref)                   # Jensen; and the definition
        assert isinstance(nll, float) and isinstance(nlpd, float) and ll.dtype == torch.float64
        assert torch.allclose(nll_t, -ell.mean(dim=(0, 1)), rtol=1e-14, atol=0)
    # equal draws: nothing to gain from the spread
    ell = (-400.0 + 30.0 * torch.randn(1, 5, 6, generator=g, dtype=torch.float64)).expand(4, 5, 6)
    _, nll, nlpd, _ = loglik_stats(ell, 6)
    assert abs(nll - nlpd) < 1e-12 * abs(nll)


# ---- Prediction --------------------------------------------------------------------------------------------------------------------
def test_prediction_still_takes_eight_fields():
    from vae_gp_ode_amd.evaluate import Prediction
    p = Prediction(1, 2, 3.0, 4.0, 5, 6, (7, 8, 9), [10])
    assert (p.mean, p.var, p.mse, p.std, p.count, p.mse_t, p.state, p.passes) == (1, 2, 3.0, 4.0, 5, 6, (7, 8, 9), [10])
    assert p.ll is None and p.nll is None and p.nlpd is None and p.nll_t is None
    assert Prediction._fields == ('mean', 'var', 'mse', 'std', 'count', 'mse_t', 'state', 'passes', 'll', 'nll', 'nlpd', 'nll_t')
    q = Prediction(1, 2, 3.0, 4.0, 5, 6, (7, 8, 9), [10], 'll', 1.5, 1.25, 'nll_t')
    assert q[:8] == p[:8] and (q.ll, q.nll, q.nlpd, q.nll_t) == ('ll', 1.5, 1.25, 'nll_t')


# ---- header and binding table ------------------------------------------------------------------------------------------------------
def test_header_and_binding_table_have_the_entry_point():
    from vae_gp_ode_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'gpode.h')).read()
    m = re.search(r'int gpode_dec10_predict_ll\((.*?)\);', txt, flags=re.S)
    assert m, 'include/gpode.h does not declare gpode_dec10_predict_ll'
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    assert [p.split()[-1].lstrip('*') for p in params] == ['c', 'table', 'w', 'bias', 'X', 'Lc', 'F', 'Th', 'T_obs', 'done', 'pred_mean',
                                                            'pred_m2', 'se_state', 'ell', 'L_total', 'stream']
    res, args = _lib.SIGNATURES['gpode_dec10_predict_ll']
    assert len(args) == len(params)
    old = _lib.SIGNATURES['gpode_dec10_predict'][1]
    assert args[:len(old) - 1] == old[:-1] and args[-1] == old[-1]                # the old list, then ell and L_total before the stream
    # gpode_dec10_predict itself is declared as it was
    assert re.search(r'int gpode_dec10_predict\(const float\* c, const float\* table, const float\* w, const float\* bias, const float\* X, '
                     r'int Lc, int F, int Th,\s+int T_obs, int done, float\* pred_mean, float\* pred_m2, float\* se_state, void\* stream\);', txt)
    # the formula and where it comes from are in the comment in front of the declaration
    head = txt[:m.start()].rsplit('/*', 1)[1]
    assert 'softplus' in head and 'vae.py:136-153' in head and 'create_model.py:52-53' in head


# ---- loader weighting --------------------------------------------------------------------------------------------------------------
def test_compute_nll_weights_batches_by_their_sequence_counts(monkeypatch):
    from vae_gp_ode_amd import evaluate as E
    figures = {3: (10.0, 8.0), 1: (50.0, 20.0), 4: (1.0, 0.5)}
    seen = []

    def fake_predict(model, X, L=1, T_custom=None, images_per_pass=8192, variance=True, loglik=False):
        assert loglik and not variance and L == 5
        seen.append(X.shape[0])
        nll, nlpd = figures[X.shape[0]]
        return E.Prediction(None, None, 0.0, 0.0, 0, None, (0, 0, 0), [L], None, nll, nlpd, None)
    monkeypatch.setattr(E, 'predict', fake_predict)
    model = torch.nn.Linear(1, 1)
    loader = [torch.zeros(3, 2, 1, 28, 28), (torch.zeros(1, 2, 1, 28, 28),), torch.zeros(4, 2, 1, 28, 28)]
    nll, nlpd = E.compute_nll(model, loader, 5)
    assert seen == [3, 1, 4]
    assert nll == pytest.approx((3 * 10.0 + 50.0 + 4 * 1.0) / 8, rel=1e-15) and nlpd == pytest.approx((3 * 8.0 + 20.0 + 4 * 0.5) / 8, rel=1e-15)
    assert nll != pytest.approx((10.0 + 50.0 + 1.0) / 3)                            # not the mean over batches


def test_cli_adds_no_flag():
    from vae_gp_ode_amd import main
    assert len(main.FLAGS) == 39


# ---- what the bound of the GPU tests rests on, in float64 on the committed fixtures ---------------------------------------------------
def loglik64_from_logits(a, x):
    """sum over the last axis of x a - softplus(a), softplus(a) = max(a, 0) + log1p(exp(-|a|)), in float64"""
    a, x = a.double(), x.double()
    return (x * a - (a.clamp_min(0) + torch.log1p(torch.exp(-a.abs())))).sum(-1)


def fixture_loglik64(g, X, z64=None):
    """Float64 references and the bound B of a fixture for targets X (N,T,1,28,28); z64: the float64 images (default: Xrec64).
    ell32 / ll32: the reference's float32 formula (vae.py:147) on Xrec, per frame (L,N,T) / per sequence (L,N); ell64 / ll64: the logit
    form in float64 on a64 = log z64 - log1p(-z64); zform: the reference's formula in float64;
    Bf[l,n,t] = 2e-4 max|a64| sum_p |x - z64| + 3 |ell32 - ell64| and B[l,n] the same with the sums over t and p."""
    L, N, T = g['Xrec'].shape[0], X.shape[0], X.shape[1]
    z32 = g['Xrec'][:, :, :T].reshape(L, N, T, 784)
    z = (g['Xrec64'] if z64 is None else z64)[:, :, :T].double().reshape(L, N, T, 784)
    x32, x = X.reshape(N, T, 784)[None], X.double().reshape(N, T, 784)[None]
    ell32 = (torch.log(z32) * x32 + torch.log(1 - z32) * (1 - x32)).double().sum(-1)
    a64 = torch.log(z) - torch.log1p(-z)
    ell64 = loglik64_from_logits(a64, x)
    zform = (torch.log(z) * x + torch.log1p(-z) * (1 - x)).sum(-1)
    da = 2e-4 * a64.abs().max()
    reach = (x - z).abs().sum(-1)
    ll32, ll64 = ell32.sum(2), ell64.sum(2)
    return dict(ell32=ell32, ell64=ell64, ll32=ll32, ll64=ll64, zform=zform.sum(2), amax=a64.abs().max().item(),
                Bf=da * reach + 3 * (ell32 - ell64).abs(), B=da * reach.sum(2) + 3 * (ll32 - ll64).abs())


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_facts_behind_the_bound(name):
    from vae_gp_ode_amd.evaluate import loglik_stats
    g = load_golden(name)
    for tag, X in (('X', g['X']), ('X01', g['X01'])):
        r = fixture_loglik64(g, X)
        ll32, ll64, ell64, B, zform = r['ll32'], r['ll64'], r['ell64'], r['B'], r['zform']
        assert torch.isfinite(ll64).all() and torch.isfinite(ll32).all()
        e_form = ((ll64 - zform).abs() / ll64.abs()).max().item()
        e32 = (ll32 - ll64).abs().max().item()
        # float32 rounding of the reference's formula: log, product, log, product, sum -- at most 4 half-ulps of the two terms per pixel
        z32, x32 = g['Xrec'][:, :, :X.shape[1]], X[None]
        cap32 = 4 * 2.0 ** -24 * ((torch.log(z32) * x32).abs() + (torch.log(1 - z32) * (1 - x32)).abs()).double().sum(dim=(2, 3, 4, 5)).max().item()
        _, nll, nlpd, _ = loglik_stats(ell64, X.shape[1])
        print('%s targets %s: |ll| %.0f, logit form vs z form %.1e, |ll32 - ll64| %.2e, nll - nlpd %.3f, max B %.3f' %
              (name, tag, ll64.abs().max().item(), e_form, e32, nll - nlpd, B.max().item()))
        assert e_form < 1e-15                                           # the two forms differ by the rounding of a float64 sum
        assert e32 <= cap32                                             # measured about 3e-5 absolute at |ll| of about 3000: B's second term is small
        if tag == 'X':
            assert nll - nlpd > 4 * B.max().item()                      # nll and nlpd are further apart than the bound can bridge
