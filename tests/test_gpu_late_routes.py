"""The loss-stage and evaluation entry points added after the route suites were written, past the first trip of every loop of theirs
(late_routes.py): gpode_elbo_iw_fwd / _bwd / _bwd_ll, gpode_reparam_draws_bwd, the six *_len loss entries, gpode_sigmoid_loglik_fwd_pk
/ _bwd_pk, gpode_gather_frames_fwd / _bwd, gpode_dec10_predict_len / _ll_len / _w, and the grid check of ops.rollout(..., 'dopri5').

Per case: gpode_last_launch() after every call equals the tag late_routes.expected names; every output and scratch is NaN-filled and
sized exactly with guard words behind it, the guards come back untouched and no NaN of the fill is left; a second run gives the same
bits.  Nothing is compared with the kernel under test: bit identity is to the twin the older route suites hold to fp64, everything else
is held to fp64 with the bound of the small-shape file of its entry point (late_routes.py names each).  The last test requires every
tag and every (kernel, loop) pair of late_routes.REQUIRED_TAGS / REQUIRED_LOOPS to have been seen.

Measured on an MI355X (256 compute units, so the predict cases run N = 37 and 38: F = 259 and 266), worst error (bound):
  gpode_elbo_iw_fwd / _bwd   worst error over the 12 cases / floor of the grid, bound 4: loss 1.38e-7 / 1.32e-7 = 1.04 (the 65535-row
                             case, whose own fp32 distance is 3.5e-8: 16 wavefronts add 4096 groups each in order), -mean iw 1.33e-7 /
                             1.10e-7 = 1.21, -mean lw 1.30e-7 / 1.37e-7 = 0.95, kl_u 8.38e-8 / 6.18e-8 = 1.36, ess 2.01e-6 / 2.01e-6 =
                             1.00, grow 4.12e-5 / 4.13e-5 = 1.00, glw 2.63e-5 / 2.63e-5 = 1.00, dUm 8.86e-8 / 8.86e-8 = 1.00, dUs
                             1.53e-7 / 1.98e-7 = 0.77
  gpode_reparam_draws_bwd    gmu 2.08e-7 / 9.82e-8 = 2.12, glogvar 2.41e-7 / 2.00e-7 = 1.21 (K = 64 terms per lane)
  the *_len entries          fused row sums 3.65e-7, separate row sums 3.65e-7 (2e-5); every bit identity holds
  the *_pk entries           row sums 3.36e-7 (2e-5), z 9.09e-8 (1e-6), ga 2.07e-7 (2e-5); the gather is exact
  predict, *_len / _ll_len   mean 1.75e-7, M2 3.56e-7, the error's mean 7.57e-8 and M2 1.67e-7, ell 1.61e-7 (2e-4)
  predict, weighted          mean 3.36e-7 (2.28e-5), M2 / W 4.26e-7 (2.32e-5), wse / W 1.98e-7 (2.06e-5), W exp(ref) 4.09e-8 (2.01e-5);
                             equal weights give the twin's mean and M2 bit for bit
  the model at N = 20        masked: terms 1.14e-7 (1e-5), gradients 6.37e-7 (2e-5); compact: terms 1.14e-7, gradients 1.24e-6;
                             iw_draws = 3, L = 2: terms at most 2.19e-6 (ess; 1e-5), gradients at most 0.45 of their bounds
No guard was written, no NaN of the fills reached an output, every second run gave the same bits; the module takes 5 s.

A library with these in-bounds mutations, built once from a scratch copy, turned red 23 of the 35 tests, each for the loop it is listed
for, and left green the cases that do not reach the mutated code (the scalar and single-trip *_len cases, both fwd_pk cases, the
65535-row fused case at K = 1, the masked and compact model cases, the refusals): a later group of k_elbo_iw_fwd taking the first trip's
(l, n); blocks > 0 of k_reparam_draws_bwd one lane off; the mask of a later float4 of a slice of k_sigmoid_loglik_fwd<true> taken at the
first one; the mask of k_sigmoid_loglik_bwd<true> taken at e mod 2^21; the second trip of k_sigmoid_loglik_bwd_pk on draw 0's row
gradient; the second trip of k_gather_frames_fwd on column 0; k = (row / K) % K in the logit blocks of k_elbo_iw_bwd<true>; a later
round of k_fwd_predict<*, true> / k_fwd_predict_w reading sequence 0's count / log-weight.

gpode_elbo_iw_bwd_ll at N = 5 cannot run with nb_small = 1 (5 wavefronts are 320 lanes): both inner values run at N = 5 with nb_small
= 2 (set by N 64) and 6 (set by P Do), and at N = 4 with nb_small = 1.
"""
import pytest
import torch

import late_routes as L
import loss_routes as R

pytestmark = pytest.mark.gpu
SEEN = set()
LOOPS = set()
FIGURES = {}


@pytest.fixture(scope='module', autouse=True)
def _report_and_drop_cached_inputs():
    yield
    print('measured:', {k: v for k, v in sorted(FIGURES.items())})
    L.clear_caches()
    R.clear_caches()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _param(cases):
    assert len(set(cases)) == len(cases)
    return pytest.mark.parametrize('c', cases, ids=[L.case_id(c) for c in cases])


def _ran(c, tags, problems, n=L.MAX_CUS):
    """the tags and the buffer checks of a case; what it covers counts only once they hold"""
    assert tags == L.expected(c), (L.case_id(c), tags, L.expected(c))
    assert not problems, (L.case_id(c), problems)
    SEEN.update(tags.values())
    LOOPS.update(L.loops(c, n))


def _figure(key, value, bound):
    if key not in FIGURES or value / bound > FIGURES[key][0] / FIGURES[key][1]:
        FIGURES[key] = (float('%.3g' % value), bound)


# ---- 1. the importance-weighted stage ------------------------------------------------------------------------------------------------------
def test_iw_stage_against_the_reference():
    """gpode_elbo_iw_fwd / _bwd over the grid of late_routes.IW_CASES: every output at most 4 x the grid's fp32 floor from fp64"""
    results = []
    for c in L.IW_CASES:
        errs, tags, problems = L.run_iw(c)
        print(L.case_id(c), {k: '%.2e / %.2e' % v for k, v in errs.items()})
        results.append((c, errs, tags, problems))
    for c, _, tags, problems in results:
        _ran(c, tags, problems)
    for k, (worst, floor) in L.judge([(c, e) for c, e, _, _ in results], 'gpode_elbo_iw_fwd / _bwd').items():
        FIGURES['iw ' + k] = ('%.3g' % worst, '%.3g' % floor)


def test_iw_stage_refuses_65536_rows():
    said, untouched, guards = L.iw_refusal(L.IW_REFUSED)
    assert not said and untouched and not guards, (said, untouched, guards)


@_param(L.IWLL_CASES)
def test_iw_fused_backward_has_the_bits_of_the_pair(c):
    out, tags, problems = L.run_iwll(c)
    _ran(c, tags, problems)


# ---- 2. the adjoint of the draws -------------------------------------------------------------------------------------------------------------
def test_draws_backward_against_the_reference():
    results = []
    for c in L.DR_CASES:
        errs, tags, problems = L.run_dr(c)
        results.append((c, errs))
        _ran(c, tags, problems)
    for k, (worst, floor) in L.judge(results, 'gpode_reparam_draws_bwd').items():
        FIGURES['draws ' + k] = ('%.3g' % worst, '%.3g' % floor)


# ---- 3. the *_len loss kernels -----------------------------------------------------------------------------------------------------------------
@_param(L.LEN_CASES)
def test_len_entries_next_to_their_twins(c):
    twin, ttags, tproblems = L.run_len(c)
    assert ttags == L.LEN_TAGS and not tproblems, (ttags, tproblems)
    # full lengths: every output of every _len entry has the twin's bits
    full, tags, problems = L.run_len(c, 'full')
    _ran(c, tags, problems)
    differs = [k for k in twin if not torch.equal(R._bits(full[k]), R._bits(twin[k]))]
    assert not differs, ('full lengths differ from the twin in', differs)
    # the counts of late_routes.len_counts
    got, tags, problems = L.run_len(c, 'mixed')
    _ran(c, tags, problems)
    assert torch.equal(R._bits(got['z']), R._bits(twin['z'])), 'z differs from the twin'
    e, e2, empty = L.len_row_errors(c, 'mixed', got)
    print('%s: fused row sums %.2e, separate row sums %.2e (bound %.1e)' % (L.case_id(c), e, e2, R.TOL))
    _figure('len fused row sums', e, R.TOL), _figure('len separate row sums', e2, R.TOL)
    assert bool(empty.any()) and bool((got['part'][empty] == 0).all()) and bool((got['rs'][empty] == 0).all()), 'a row without a frame is not exactly 0'
    obs = L.len_observed(c, 'mixed').reshape(-1)
    for k in L.LEN_GA + ('gz',):
        assert torch.equal(R._bits(got[k])[obs], R._bits(twin[k])[obs]), '%s differs from the twin on observed elements' % k
        assert bool((got[k][~obs] == 0).all()), '%s is not zero on padded elements' % k
    for k in L.LEN_OTHERS:
        assert torch.equal(R._bits(got[k]), R._bits(twin[k])), '%s differs from the twin' % k
    assert e <= R.TOL and e2 <= R.TOL, (e, e2)
    # NaN and +-Inf in the padded targets and the padded logits change no bit
    for kind in ('nan', 'inf'):
        dirty, dtags, dproblems = L.run_len(c, 'mixed', kind)
        assert dtags == tags and not dproblems, (kind, dproblems)
        keys = ('part', 'rs', 'gz') + L.LEN_GA + L.LEN_OTHERS
        differs = [k for k in keys if not torch.equal(R._bits(dirty[k]), R._bits(got[k]))]
        assert not differs, (kind, differs)
        assert torch.equal(R._bits(dirty['z'])[obs], R._bits(got['z'])[obs])
        assert all(bool(torch.isfinite(dirty[k]).all()) for k in keys), kind


def test_len_forward_refuses_65536_rows():
    said, untouched, guards = L.len_refusal(L.LEN_REFUSED)
    assert 'gpode_sigmoid_loglik_fwd_len' in said and 'rows <= 65535' in said and untouched and not guards, (said, untouched, guards)


# ---- 4. the compact route ----------------------------------------------------------------------------------------------------------------------
@_param(L.PK_CASES)
def test_pk_loss_kernels(c):
    counts = L.len_lengths(c, 'mixed')
    got, tags, problems = L.run_pk(c, 'mixed')
    _ran(c, tags, problems)
    cl, off, src = L.host_index(counts, c.T)
    ref = L.pk_reference(c, counts)
    part = got['part'].double().view(c.L, c.N, c.ns)
    seen = cl > 0
    e_rows = float(((part.sum(2) - ref['rowsum']).abs() / ref['scale'].clamp_min(1e-300))[:, seen].max())
    e_z = float((got['z'].double() - ref['z'].reshape(-1)).abs().max())
    e_ga = float((got['ga'].double() - ref['ga'].reshape(-1)).abs().max() / ref['ga'].abs().max())
    print('%s: row sums %.2e (%.1e), z %.2e (%.1e), ga %.2e (2e-5)' % (L.case_id(c), e_rows, R.TOL, e_z, R.TOL_Z, e_ga))
    _figure('pk row sums', e_rows, R.TOL), _figure('pk z', e_z, R.TOL_Z), _figure('pk ga', e_ga, 2e-5)
    # a slice beyond its row's length leaves exactly 0
    chunk = L.loglik_chunk(c.T * c.frame, c.ns, not c.mis)
    beyond = (torch.arange(c.ns)[None, :] * chunk >= (cl * c.frame)[:, None])                  # (N, ns)
    assert bool(beyond.any()) and bool((~beyond).any()) and bool((part[:, beyond] == 0).all()), 'a slice beyond its row is not exactly 0'
    assert e_rows <= R.TOL and e_z <= R.TOL_Z and e_ga <= 2e-5, (e_rows, e_z, e_ga)
    # full lengths: z, part and ga have the bits of gpode_sigmoid_loglik_fwd / _bwd
    full, ftags, fproblems = L.run_pk(c, 'full')
    twin, ttags, tproblems = L.pk_twin(c)
    assert ftags == tags and not fproblems and not tproblems and ttags == dict(fwd='sigmoid_loglik_fwd', bwd='sigmoid_loglik_bwd')
    differs = [k for k in twin if not torch.equal(R._bits(full[k]), R._bits(twin[k]))]
    assert not differs, ('full lengths differ from the twin in', differs)
    # NaN in every padded target frame changes no bit
    dirty, _, dproblems = L.run_pk(c, 'mixed', nan_padding=True)
    assert not dproblems and all(torch.equal(R._bits(dirty[k]), R._bits(got[k])) for k in got)


@_param(L.PKB_CASES)
def test_pk_backward_past_the_grid_cap(c):
    counts = L.pkb_counts(c)
    got, tags, problems = L._twice(lambda: L._once_pkb(c, counts, False))
    _ran(c, tags, problems)
    ref = L.pkb_reference(c, counts)
    e = float((got['ga'].double() - ref.reshape(-1)).abs().max() / ref.abs().max())
    print('%s: ga %.2e (2e-5)' % (L.case_id(c), e))
    _figure('pk ga', e, 2e-5)
    assert e <= 2e-5, e
    full = [c.T] * c.N
    a, atags, aproblems = L._once_pkb(c, full, False)
    b, btags, bproblems = L._once_pkb(c, full, True)
    assert atags == tags and btags == dict(bwd='sigmoid_loglik_bwd') and not aproblems and not bproblems
    assert torch.equal(R._bits(a['ga']), R._bits(b['ga'])), 'full lengths: ga differs from gpode_sigmoid_loglik_bwd'


@_param(L.GA_CASES)
def test_gather_past_the_grid_cap(c):
    got, tags, problems = L.run_ga(c)
    _ran(c, tags, problems)
    out, gzt = L.ga_reference(c)
    assert torch.equal(got['out'], out), 'gpode_gather_frames_fwd'
    assert torch.equal(got['gzt'], gzt), 'gpode_gather_frames_bwd'
    assert bool((got['gzt'][..., c.q:] == 0).all())


# ---- 5. the predict epilogue -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def predict_setup():
    n = cus()
    Ns = L.predict_Ns(n, L.PR_TH)
    grid = L.predict_grid(Ns[0] * L.PR_TH, n)
    assert all(N * L.PR_TH > grid for N in Ns) and any((N * L.PR_TH) % grid for N in Ns), (n, Ns)       # F > n, a ragged last round
    return n, Ns, {N: L._predict_dev(Ns[1], N) for N in Ns}


def _same(a, b, keys):
    return [k for k in keys if not torch.equal(R._bits(a[k]), R._bits(b[k]))]


@pytest.mark.parametrize('which', [0, 1], ids=['first F > n', 'second F > n'])
@pytest.mark.parametrize('ll', [False, True], ids=['len', 'll_len'])
def test_predict_len(predict_setup, ll, which):
    n, Ns, devs = predict_setup
    N, Nmax = Ns[which], Ns[1]
    c, dev = L.PR('ll_len' if ll else 'len', N), devs[Ns[which]]
    keys = ('mean', 'm2', 'se') + (('ell',) if ll else ())
    twin, ttags, tproblems = L.predict_run(dev, N, L.PR_SPLITS, ll)
    assert set(ttags) == {'dec10_predict_ll' if ll else 'dec10_predict'} and not tproblems, (ttags, tproblems)
    # the twin itself against fp64 at this F, and full lengths: the twin's bits
    for k, e in L.predict_errors(twin, L.predict_reference(Nmax, N, L.F64), N).items():
        print('%s twin %-7s %.2e' % (L.case_id(c), k, e))
        assert e <= L.PREDICT_TOL, (k, e)
    full, ftags, fproblems = L.predict_run(dev, N, L.PR_SPLITS, ll, n_obs=[L.PR_TH] * N)
    assert not fproblems and not _same(full, twin, keys), (fproblems, _same(full, twin, keys))
    # counts 0 ... Th
    n_obs = L.predict_n_obs(N)
    got, tags, problems = L.predict_run(dev, N, L.PR_SPLITS, ll, n_obs=n_obs)
    assert len(tags) == 2
    _ran(c, dict(run=tags[0]), problems + ([] if tags[0] == tags[1] else ['the second launch took %s' % tags[1]]), n)
    has = L.predict_has(N, n_obs).reshape(-1)
    assert torch.equal(got['se'][has], twin['se'][has]) and bool((got['se'][has][:, 0] == L.PR_L * 784).all())
    assert bool((got['se'][~has] == 0).all()), 'a frame without a target has a count'
    assert torch.equal(got['mean'], twin['mean']) and torch.equal(got['m2'], twin['m2'])
    if ll:
        assert torch.equal(got['ell'][:, has], twin['ell'][:, has]) and bool((got['ell'][:, ~has] == 0).all())
    for k, e in L.predict_errors(got, L.predict_reference(Nmax, N, L.F64, n_obs), N).items():
        print('%s %-7s %.2e (bound %.0e)' % (L.case_id(c), k, e, L.PREDICT_TOL))
        _figure('predict ' + k, e, L.PREDICT_TOL)
        assert e <= L.PREDICT_TOL, (k, e)
    # any split of the draws gives the bits of one launch; a second run gives the same bits
    for splits in ((L.PR_L,), (1, 3), L.PR_SPLITS):
        other, _, oproblems = L.predict_run(dev, N, splits, ll, n_obs=n_obs)
        assert not oproblems and not _same(other, got, keys), (splits, _same(other, got, keys))
    # NaN in the padded targets changes no bit
    Xb = dev['X'].clone()
    for i, k in enumerate(n_obs):
        Xb[i, k:] = float('nan')
    dirty, _, dproblems = L.predict_run(dev, N, L.PR_SPLITS, ll, n_obs=n_obs, X=Xb)
    assert not dproblems and not _same(dirty, got, keys)


@pytest.mark.parametrize('which', [0, 1], ids=['first F > n', 'second F > n'])
@pytest.mark.parametrize('ragged', [False, True], ids=['w', 'w_len'])
def test_predict_weighted(predict_setup, ragged, which):
    n, Ns, devs = predict_setup
    N, Nmax = Ns[which], Ns[1]
    c, dev = L.PR('w_len' if ragged else 'w', N), devs[Ns[which]]
    keys = ('wstate', 'mean', 'm2', 'wse')
    n_obs = L.predict_n_obs(N) if ragged else None
    X = None
    if ragged:                                        # what the padded targets hold must reach nothing
        X = dev['X'].clone()
        for i, k in enumerate(n_obs):
            X[i, k:] = float('nan')
    logw = dev['logw']
    got, tags, problems = L.predict_run_w(dev, N, L.PR_SPLITS, logw, n_obs, X)
    assert len(tags) == 2
    _ran(c, dict(run=tags[0]), problems + ([] if tags[0] == tags[1] else ['the second launch took %s' % tags[1]]), n)
    r64, r32 = (L.predict_reference(Nmax, N, dt, n_obs, logw.double()) for dt in (L.F64, L.F32))
    res = L.weighted_errors(got, r64, r32, N)
    for k, (e, bound) in res.items():
        print('%s %-10s %.2e (bound %.2e)' % (L.case_id(c), k, e, bound))
        _figure('weighted ' + k, e, bound)
    for k, (e, bound) in res.items():
        assert e <= bound, (k, e, bound)
    has = L.predict_has(N, n_obs)
    assert bool((got['wse'].view(N, L.PR_TH)[~has] == 0).all()) and bool((got['wse'].view(N, L.PR_TH)[has] > 0).all())
    # any split of the draws gives the bits of one launch
    for splits in ((L.PR_L,), (1, 3), L.PR_SPLITS):
        other, _, oproblems = L.predict_run_w(dev, N, splits, logw, n_obs, X)
        assert not oproblems and not _same(other, got, keys), (splits, _same(other, got, keys))
    if ragged:                                        # the moments do not depend on the counts
        plain, _, _ = L.predict_run_w(dev, N, L.PR_SPLITS, logw)
        assert not _same(plain, got, ('wstate', 'mean', 'm2'))
        wse, pw = got['wse'].view(N, L.PR_TH), plain['wse'].view(N, L.PR_TH)
        assert torch.equal(wse[has], pw[has])
        return
    # equal weights: mean and M2 of gpode_dec10_predict, bit for bit
    eq, _, eproblems = L.predict_run_w(dev, N, L.PR_SPLITS, torch.full((L.PR_L, N), 0.75))
    twin, _, tproblems = L.predict_run(dev, N, L.PR_SPLITS)
    assert not eproblems and not tproblems
    assert torch.equal(eq['wstate'][:, 1], torch.full((N * L.PR_TH,), float(L.PR_L)))
    print('%s equal weights against the twin: mean %.2e, M2 %.2e' % (L.case_id(c), L.relerr(eq['mean'], twin['mean']), L.relerr(eq['m2'], twin['m2'])))
    assert torch.equal(R._bits(eq['mean']), R._bits(twin['mean'])) and torch.equal(R._bits(eq['m2']), R._bits(twin['m2']))


# ---- 6. one model-level case per feature at N = 20 -----------------------------------------------------------------------------------------
MODEL_N = 20


@pytest.fixture
def generators_as_found():
    """as test_gpu_ragged_model.py: the model tests seed and draw from the process-wide generators; later files must not see that"""
    import random
    import numpy as np
    saved = (torch.get_rng_state(), torch.cuda.get_rng_state_all(), np.random.get_state(), random.getstate())
    yield
    torch.set_rng_state(saved[0])
    torch.cuda.set_rng_state_all(saved[1])
    np.random.set_state(saved[2])
    random.setstate(saved[3])


def test_model_masked_loss_at_20_sequences(generators_as_found):
    """compute_loss(n_obs=) against the torch-side masked loss of test_gpu_ragged_model.py, its bounds"""
    import test_gpu_ragged_model as RM
    m, src = RM.tiny_model()
    X, ts, n_obs = RM.ragged_batch(m, N=MODEL_N)
    assert X.shape[0] == MODEL_N and len(set(n_obs.tolist())) > 1
    out, g = RM.loss_and_grads(m, src, X, RM.L, ts=ts, n_obs=n_obs)
    ref, scale, gr = RM.torch_side(m, src, X, ts, n_obs)
    e_terms = [abs(float(a) - float(b)) / s for a, b, s in zip(out, ref, scale)]
    errs = RM.compare_grads(g, gr, 'masked, N = 20')
    print('masked N %d n_obs %s: terms %s; gradients worst %s' % (MODEL_N, n_obs.tolist(), ['%.2e' % e for e in e_terms],
                                                                sorted(((v, k) for k, v in errs.items()), reverse=True)[:3]))
    _figure('model masked terms', max(e_terms), R.TOL_KL), _figure('model masked gradients', max(errs.values()), 2e-5)
    assert all(e <= R.TOL_KL for e in e_terms), e_terms
    bad = {k: v for k, v in errs.items() if not v <= 2e-5}
    assert not bad, bad


def test_model_compact_loss_at_20_sequences(generators_as_found, monkeypatch):
    """compute_loss(compact=True) against the torch-side composition of test_gpu_ragged_compact.py, its bounds"""
    import copy
    import test_gpu_ragged_compact as RC
    m, src = RC.tiny_model()
    init = copy.deepcopy(m.state_dict())
    X, ts, n_obs = RC.ragged_batch(m, N=MODEL_N)
    out, g = RC.run(m, src, X, RC.L, ts=ts, n_obs=n_obs, compact=True)
    m.load_state_dict(init)
    ref, scale, gr = RC.torch_side_compact(m, src, X, ts, n_obs, monkeypatch, N=MODEL_N)
    e_terms = [abs(float(a) - float(b)) / s for a, b, s in zip(out, ref, scale)]
    errs = RC.compare_grads(g, gr, 'compact, N = 20')
    print('compact N %d: terms %s; gradients worst %s' % (MODEL_N, ['%.2e' % e for e in e_terms], sorted(((v, k) for k, v in errs.items()), reverse=True)[:3]))
    _figure('model compact terms', max(e_terms), R.TOL_KL), _figure('model compact gradients', max(errs.values()), 2e-5)
    assert all(e <= R.TOL_KL for e in e_terms), e_terms
    bad = {k: v for k, v in errs.items() if not v <= 2e-5}
    assert not bad, bad


def test_model_iw_loss_at_20_sequences(generators_as_found):
    """compute_loss(iw_draws=3) at L = 2: 40 groups and 120 rows, against the composition of test_gpu_iw_model.py under its bounds"""
    import copy
    import test_gpu_iw_model as IM
    m, src = IM.build('rbf1-rk4')
    init = copy.deepcopy(m.state_dict())
    K, Ld = 3, 2
    assert L.iw_group_trips(Ld, MODEL_N) == 3 and Ld * K * MODEL_N == 120
    terms, gr = IM.one_case(m, src, init, K, Ld, N=MODEL_N)
    tb, gb = IM.bounds({(K, Ld): (terms, gr)})
    print('iw N %d K %d L %d: terms %s; gradients worst %s' % (MODEL_N, K, Ld, {k: '%.1e|%.1e' % v for k, v in terms.items()},
                                                             sorted(((v[0], v[1], k) for k, v in gr.items()), reverse=True)[:3]))
    for k, v in terms.items():
        _figure('model iw ' + k, v[0], tb[k])
    _figure('model iw gradients', max(v[0] / gb[k] for k, v in gr.items()), 1.0)
    bad = {n: (v, tb[n]) for n, v in terms.items() if not v[0] <= tb[n]}
    assert not bad, bad
    bad = {k: (v, gb[k]) for k, v in gr.items() if not v[0] <= gb[k]}
    assert not bad, bad


# ---- 7. the grid check of the adaptive rollout -------------------------------------------------------------------------------------------------
def test_a_bad_grid_at_the_address_of_a_checked_one_is_refused():
    """ops._check_increasing remembers the grid it checked last.  A freed grid's block goes back to the caching allocator and the next
    grid of the same shape lands on it at version 0: the check must not take the new tensor for the old one"""
    from oracle import gpode_oracle as O
    from vae_gp_ode_amd import _lib, ops
    g = R._gen('late grid check')
    q, M, S, N = 6, 16, 32, 8
    p = [O.invsoftplus(torch.full((q, q), 2.0)), O.invsoftplus(torch.ones(q)), torch.randn(M, q, generator=g), 0.1 * torch.randn(M, q, generator=g),
         O.tril_pack(torch.stack([torch.eye(M)] * q) * 1e-3)]
    nz = [torch.randn(M, q, generator=g), torch.randn(S, q, generator=g), torch.randn(q, S, q, generator=g), torch.rand(1, S, q, generator=g)]
    cache = ops.cache_build('RBF', *[t.cuda() for t in p + nz])
    z0 = torch.randn(N, q, generator=g).cuda()
    good = (0.1 * torch.arange(6, dtype=torch.float32)).cuda()
    ops.rollout(cache, z0, good, 1, 'dopri5')
    torch.cuda.synchronize()
    addr, version, shape = good.data_ptr(), good._version, tuple(good.shape)
    del good
    bad = torch.tensor([0.0, 0.1, 0.2, 0.2, 0.4, 0.5], device='cuda')
    assert (bad.data_ptr(), bad._version, tuple(bad.shape)) == (addr, version, shape), 'the premise: the bad grid reuses the checked grid\'s block'
    with pytest.raises(_lib.GpodeError, match='strictly increasing'):
        ops.rollout(cache, z0, bad, 1, 'dopri5')


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_every_tag_and_every_loop_was_seen():
    """runs last: it reads what the tests above left in this process, so it needs the whole module in one process (no -k, --lf or
    xdist), like the other route modules"""
    missing = [t for t in L.REQUIRED_TAGS if t not in SEEN] + [p for p in L.REQUIRED_LOOPS if p not in LOOPS]
    assert not missing, missing
