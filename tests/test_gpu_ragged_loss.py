"""The loss stage on ragged minibatches, through the C ABI: gpode_sigmoid_loglik_fwd_len / _bwd_len, gpode_elbo_all_bwd_ll_len /
_ll_kl_len and the separate-kernel form gpode_loglik_rowsum_fwd_len / _bwd_len, each against its twin.  A ragged minibatch is a padded
one: X (N,T,frame), n_obs (N,) int32, frame t of sequence n observed iff t < n_obs[n]; rows are (draw, sequence).

Shapes (L, N, T, frame): a (2,3,5,784) -- the float4 path, 4 slices of 980 elements, not frame-aligned; b (2,3,5,7) -- the scalar
path, inner % 4 != 0; c (1,3,4,6) -- inner % 4 == 0 but frame % 4 != 0, where a float4 would straddle two frames; dX / da / dz / d -- a
with one operand, or all three, one float off a 16-byte boundary.  Length vectors: all T, all 1, [T,1,2], [0,T+3,2] (and, for the
full-length rule alone, [T+3,T,T+1]).

Checks, per shape and length vector.  Outputs and scratches are NaN-filled and sized exactly with guard floats behind each
(loss_routes.Bufs); every call's gpode_last_launch() is the twin's tag + "_len"; a second run gives the same bits.
  z bits         z of the _len forward equals the twin's z everywhere
  row sums       within loss_routes.TOL (2e-5) of the fp64 sum of the observed terms, relative to the fp64 sum of their absolute values
                 -- the bound and the scaling of test_gpu_loss_routes for gpode_sigmoid_loglik_fwd, including its rule for rows of up to
                 8 terms (loss_routes.sll_short_rows: such rows are held to the fp64 terms of the z the kernel returned, because one
                 fp32 sigmoid near a logit of 8 is ill-conditioned in 1 - z); a row with n_obs <= 0 gives exactly 0
  ga bits        ga of gpode_sigmoid_loglik_bwd_len, gpode_elbo_all_bwd_ll_len and _ll_kl_len equals the twin's ga on observed elements
                 and is +0.0 or -0.0 on padded ones; glrow, ghs / gkls, dUm, dUs of the two fused launches equal their twins'
  full lengths   lengths all >= T: every output of every _len entry equals its twin's
  garbage        the padded target frames and padded logits set to NaN, and to +-Inf: part and every ga are bit-identical to the clean run
  routes         gpode_loglik_rowsum_fwd_len sums the same observed terms (2e-5 of sum |terms|, against fp64 and against the fused
                 form); gpode_loglik_rowsum_bwd_len -> gpode_act_bwd equals ga of gpode_sigmoid_loglik_bwd_len bit for bit, as the
                 unmasked pair does in test_gpu_loss_routes
  refusals       n_obs NULL, inner != T frame, nX % inner != 0: non-zero return, the NaN fills untouched"""
import ctypes
import functools

import pytest
import torch

import loss_routes as R

pytestmark = pytest.mark.gpu


SHAPES = {'a': (2, 3, 5, 784, ''), 'b': (2, 3, 5, 7, ''), 'c': (1, 3, 4, 6, ''),
          'dX': (2, 3, 5, 784, 'X'), 'da': (2, 3, 5, 784, 'a'), 'dz': (2, 3, 5, 784, 'z'), 'd': (2, 3, 5, 784, 'Xaz')}
LENS = ('full', 'one', 'mixed', 'edge')
M, DO, Q, NKS = 7, 3, 6, 2
TAGS = dict(fwd='sigmoid_loglik_fwd', bwd='sigmoid_loglik_bwd', ll='elbo_loglik_bwd', kl='elbo_loglik_bwd_kl', rs='loglik_rowsum',
            rsb='loglik_rowsum_bwd')
GA = ('ga_bwd', 'ga_ll', 'ga_kl')
OTHERS = ('glrow_ll', 'ghs', 'dUm_ll', 'dUs_ll', 'glrow_kl', 'gkls', 'dUm_kl', 'dUs_kl')


def lengths(key, name):
    T = SHAPES[key][2]
    return dict(full=[T] * 3, one=[1] * 3, mixed=[T, 1, 2], edge=[0, T + 3, 2], over=[T + 3, T, T + 1])[name]


def observed(key, name):
    """(N,T) bool: t < n_obs[n]"""
    T = SHAPES[key][2]
    return torch.arange(T)[None, :] < torch.tensor(lengths(key, name))[:, None]


@functools.lru_cache(maxsize=None)
def inputs(key):
    L, N, T, frame, _ = SHAPES[key]
    g = R._gen('ragged loss', L, N, T, frame)
    rows = L * N
    return dict(X=R._x_form((N, T, frame), 'norm', g), a=R._logits((L, N, T, frame), g), grow=torch.randn(rows, generator=g),
                hs=torch.cat((torch.randn(N, Q, generator=g), torch.randn(N, Q, generator=g) * 0.7 - 1.0), 1),
                Um=0.5 * torch.randn(M, DO, generator=g), Us=R.us_packed(M, DO, 'tril', 1.0, g))


def _garbage(t, kind):
    if kind == 'nan':
        return torch.full_like(t, float('nan'))
    s = torch.ones(t.numel()).reshape(t.shape)
    s.view(-1)[1::2] = -1.0
    return s * float('inf')


def _once(key, lname, kind):
    """every entry of the loss stage once: the twins (lname None) or the _len forms.  -> (outputs on the CPU, tags, problems)"""
    L, N, T, frame, mis = SHAPES[key]
    rows, inner, nX = L * N, T * frame, N * T * frame
    n = rows * inner
    d = inputs(key)
    X, a = d['X'].clone(), d['a'].clone()
    sfx, extra = '', ()
    if lname is not None:
        obs = observed(key, lname)
        if kind != 'clean':
            X[~obs] = _garbage(X[~obs], kind)
            a[:, ~obs] = _garbage(a[:, ~obs], kind)
        n_obs = torch.tensor(lengths(key, lname), dtype=torch.int32, device='cuda')
        sfx, extra = '_len', (n_obs, T, frame)
    bf, tags, out = R.Bufs(), {}, {}
    sh = lambda c: 1 if c in mis else 0
    Xd, ad = bf.new('X', nX, X, shift=sh('X')), bf.new('a', n, a, shift=sh('a'))
    z = bf.new('z', n, shift=sh('z'))
    ns = R.sigmoid_loglik_splits(rows, inner)
    part = bf.new('part', rows * ns)
    R._call(tags, 'fwd', 'gpode_sigmoid_loglik_fwd' + sfx, Xd, ad, z, part, rows, inner, nX, ns, *extra)
    grow = bf.new('grow', rows, d['grow'])
    ga = bf.new('ga_bwd', n, shift=sh('z'))
    R._call(tags, 'bwd', 'gpode_sigmoid_loglik_bwd' + sfx, Xd, z, grow, ga, rows, inner, nX, *extra)
    out.update(z=z, part=part.view(rows, ns), ga_bwd=ga)
    # the two fused backward launches: every likelihood row gets the same gradient
    P = M * (M + 1) // 2
    Um, Us, hs = bf.new('Um', M * DO, d['Um']), bf.new('Us', DO * P, d['Us']), bf.new('hs', N * 2 * Q, d['hs'])
    gs = [bf.new('g%d' % i, 1, torch.tensor([v])) for i, v in enumerate(R.SEED_VALUES)]
    nobs = ctypes.c_float(R.NOBS)
    o = {k: bf.new(k, m) for k, m in (('glrow_ll', rows), ('ghs', N * 2 * Q), ('dUm_ll', M * DO), ('dUs_ll', DO * P), ('ga_ll', n),
                                      ('glrow_kl', rows), ('gkls', NKS), ('dUm_kl', M * DO), ('dUs_kl', DO * P), ('ga_kl', n))}
    R._call(tags, 'll', 'gpode_elbo_all_bwd_ll' + sfx, *gs, rows, hs, None, N, Q, M, DO, Um, Us, nobs, o['glrow_ll'], o['ghs'], None, o['dUm_ll'],
            o['dUs_ll'], Xd, z, o['ga_ll'], n, nX, *extra)
    R._call(tags, 'kl', 'gpode_elbo_all_bwd_ll_kl' + sfx, *gs, rows, N, M, DO, Um, Us, nobs, o['glrow_kl'], o['gkls'], NKS, None, 0, o['dUm_kl'],
            o['dUs_kl'], Xd, z, o['ga_kl'], n, nX, *extra)
    out.update(o)
    # the separate-kernel form on the same z
    rs, gz, ga_sep = bf.new('rs', rows), bf.new('gz', n), bf.new('ga_sep', n)
    R._call(tags, 'rs', 'gpode_loglik_rowsum_fwd' + sfx, Xd, z, rs, rows, inner, nX, *extra)
    R._call(tags, 'rsb', 'gpode_loglik_rowsum_bwd' + sfx, Xd, z, grow, gz, rows, inner, nX, *extra)
    R._call(tags, 'act', 'gpode_act_bwd', z, gz, ga_sep, n, 1)
    out.update(rs=rs, gz=gz, ga_sep=ga_sep)
    problems = bf.problems()
    if kind != 'clean':                               # NaN logits give NaN z on padded elements, as the twin would: not a fill left over
        problems = [p for p in problems if not p.startswith(('z:', 'ga_sep:'))]
    return {k: v.cpu() for k, v in out.items()}, tags, problems


@functools.lru_cache(maxsize=None)
def run(key, lname=None, kind='clean'):
    """_once twice: (outputs, tags, problems incl. what differs in the second run)"""
    (out, tags, problems), (out2, tags2, problems2) = _once(key, lname, kind), _once(key, lname, kind)
    differs = ['the second run differs in %s' % k for k in out if not torch.equal(R._bits(out[k]), R._bits(out2[k]))]
    return out, tags, problems + problems2 + differs + ([] if tags == tags2 else ['the second run took %s' % tags2])


@pytest.fixture(scope='module', autouse=True)
def _drop_caches():
    yield
    run.cache_clear()
    inputs.cache_clear()


def _elements(key, lname):
    """(rows, inner) bool on the CPU: the element is observed"""
    L, N, T, frame, _ = SHAPES[key]
    return observed(key, lname)[None, :, :, None].expand(L, N, T, frame).reshape(L * N, T * frame)


CASES = [(k, l) for k in SHAPES for l in LENS]
_cases = pytest.mark.parametrize('key,lname', CASES, ids=['%s-%s' % c for c in CASES])


@_cases
def test_forward(key, lname):
    L, N, T, frame, _ = SHAPES[key]
    got, tags, problems = run(key, lname)
    twin, ttags, tproblems = run(key)
    assert not problems and not tproblems, (problems, tproblems)
    assert ttags['fwd'] == TAGS['fwd'] and tags['fwd'] == TAGS['fwd'] + '_len', (tags, ttags)
    assert torch.equal(R._bits(got['z']), R._bits(twin['z'])), 'z differs from the twin'
    d = inputs(key)
    obs = _elements(key, lname)
    t = R.bernoulli_terms(d['X'].double().reshape(1, -1).repeat(L, 1).reshape(L * N, -1), torch.sigmoid(d['a'].double()).reshape(L * N, -1))
    short = obs.sum(1) <= R.SLL_SHORT                 # rows of up to 8 observed terms: the fp64 terms of the returned z (sll_short_rows)
    tz = R.bernoulli_terms(d['X'].double().reshape(1, -1).repeat(L, 1).reshape(L * N, -1), got['z'].double().reshape(L * N, -1))
    t = torch.where(short[:, None], tz, t)
    t = torch.where(obs, t, torch.zeros((), dtype=torch.float64))
    ref, scale = t.sum(1), t.abs().sum(1)
    rowsum = got['part'].double().sum(1)
    empty = obs.sum(1) == 0
    err = ((rowsum - ref).abs() / scale.clamp_min(1e-300))[~empty]
    e = err.max().item() if err.numel() else 0.0
    ers = ((got['rs'].double() - ref).abs() / scale.clamp_min(1e-300))[~empty]
    e2 = ers.max().item() if ers.numel() else 0.0
    print('%s %s: fused row sums %.2e, separate row sums %.2e (bound %.1e)' % (key, lname, e, e2, R.TOL))
    assert bool((got['part'][empty] == 0).all()) and bool((got['rs'][empty] == 0).all()), 'a row without a frame is not exactly 0'
    assert tags['rs'] == TAGS['rs'] + '_len'
    assert e <= R.TOL and e2 <= R.TOL, (e, e2)


@_cases
def test_backward(key, lname):
    got, tags, problems = run(key, lname)
    twin, ttags, _ = run(key)
    assert not problems, problems
    for k in ('bwd', 'll', 'kl', 'rsb'):
        assert ttags[k] == TAGS[k] and tags[k] == TAGS[k] + '_len', (k, tags, ttags)
    obs = _elements(key, lname).reshape(-1)
    for k in GA + ('gz',):
        assert torch.equal(R._bits(got[k])[obs], R._bits(twin[k])[obs]), '%s differs from the twin on observed elements' % k
        assert bool((got[k][~obs] == 0).all()), '%s is not zero on padded elements' % k
    for k in OTHERS:
        assert torch.equal(R._bits(got[k]), R._bits(twin[k])), '%s differs from the twin' % k
    # the separate kernels in a chain give the bits of the fused backward; on padded elements 0 z (1 - z) is a zero as well
    assert torch.equal(R._bits(got['ga_sep'])[obs], R._bits(got['ga_bwd'])[obs]) and bool((got['ga_sep'][~obs] == 0).all())


@pytest.mark.parametrize('lname', ['full', 'over'])
@pytest.mark.parametrize('key', list(SHAPES))
def test_full_lengths_give_the_bits_of_the_twin(key, lname):
    got, _, problems = run(key, lname)
    twin, _, _ = run(key)
    assert not problems, problems
    differs = [k for k in twin if not torch.equal(R._bits(got[k]), R._bits(twin[k]))]
    assert not differs, differs


@pytest.mark.parametrize('kind', ['nan', 'inf'])
@_cases
def test_padded_garbage_changes_nothing(key, lname, kind):
    got, tags, problems = run(key, lname, kind)
    clean, ctags, _ = run(key, lname)
    assert not problems and tags == ctags, (problems, tags)
    obs = _elements(key, lname).reshape(-1)
    differs = [k for k in ('part', 'rs', 'gz') + GA + OTHERS if not torch.equal(R._bits(got[k]), R._bits(clean[k]))]
    assert not differs, differs
    assert torch.equal(R._bits(got['z'])[obs], R._bits(clean['z'])[obs])
    for k in ('part', 'rs', 'gz') + GA + OTHERS:
        assert bool(torch.isfinite(got[k]).all()), k


def _refusal_calls(case):
    """[(entry, args builder)] at L = 2, N = 3, T = 5, frame = 4; case: which argument is wrong"""
    L, N, T, frame = 2, 3, 5, 4
    rows, inner, nX = L * N, T * frame, N * T * frame
    n = rows * inner
    bf = R.Bufs()
    n_obs = torch.tensor([5, 1, 2], dtype=torch.int32, device='cuda')
    if case == 'null':
        n_obs = None
    elif case == 'inner':                             # inner != T frame
        T = 4
    elif case == 'nX':                                # nX is no whole number of sequences
        nX = inner // 2
    zeros = lambda m: torch.zeros(m)
    X, a, z, grow = bf.new('X', max(nX, 1), zeros(max(nX, 1))), bf.new('a', n, zeros(n)), bf.new('zin', n, zeros(n) + 0.5), bf.new('grow', rows, zeros(rows))
    P = M * (M + 1) // 2
    Um, Us, hs = bf.new('Um', M * DO, zeros(M * DO)), bf.new('Us', DO * P, zeros(DO * P) + 1), bf.new('hs', N * 2 * Q, zeros(N * 2 * Q))
    o = lambda name, m: bf.new(name, m)
    nobs = ctypes.c_float(R.NOBS)
    calls = [('gpode_sigmoid_loglik_fwd_len', (X, a, o('z', n), o('part', rows * 4), rows, inner, nX, 4, n_obs, T, frame)),
             ('gpode_sigmoid_loglik_bwd_len', (X, z, grow, o('ga', n), rows, inner, nX, n_obs, T, frame)),
             ('gpode_loglik_rowsum_fwd_len', (X, z, o('rs', rows), rows, inner, nX, n_obs, T, frame)),
             ('gpode_loglik_rowsum_bwd_len', (X, z, grow, o('gz', n), rows, inner, nX, n_obs, T, frame))]
    if case != 'inner':                               # the fused launches take no inner: n_logits and nX against T frame
        calls += [('gpode_elbo_all_bwd_ll_len', (None, None, None, None, rows, hs, None, N, Q, M, DO, Um, Us, nobs, o('glrow', rows), o('ghs', N * 2 * Q),
                                                 None, o('dUm', M * DO), o('dUs', DO * P), X, z, o('ga2', n), n, nX, n_obs, T, frame)),
                  ('gpode_elbo_all_bwd_ll_kl_len', (None, None, None, None, rows, N, M, DO, Um, Us, nobs, o('glrow2', rows), o('gkls', NKS), NKS, None, 0,
                                                    o('dUm2', M * DO), o('dUs2', DO * P), X, z, o('ga3', n), n, nX, n_obs, T, frame))]
    return bf, calls


@pytest.mark.parametrize('case', ['null', 'inner', 'nX'])
def test_refusals(case):
    bf, calls = _refusal_calls(case)
    for name, args in calls:
        with pytest.raises(R.Refused, match=name):
            R._call({}, 'x', name, *args)
    assert bf.untouched(), 'a refused call wrote an output'
    bad = [p for p in bf.problems() if 'guard' in p]
    assert not bad, bad
