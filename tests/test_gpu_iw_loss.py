"""GPU: the kernels of training on the importance-weighted bound through the C ABI -- gpode_reparam_draws_bwd, gpode_elbo_iw_fwd,
gpode_elbo_iw_bwd, gpode_elbo_iw_bwd_ll -- against iw_ref.py.  Buffers are loss_routes.Bufs: outputs NaN-filled, guard words behind each.

BOUNDS.  Every comparison against float64 evaluates the same iw_ref formula twice on the same float32 inputs, in float64 (the reference)
and in float32; the distance between the two is the floor, and a kernel may be at most 4 times the floor from float64 (the margin
test_gpu_baseline_sizes.py gives its oracle comparison: the order of the split sums differs).  No bound is taken from a kernel's output.
One scalar's float32 distance is a coin flip around a unit in the last place of a number of magnitude 2e3 -- it is exactly 0 for a good
share of the cases -- so the floor of an output is the largest distance over the cases of its grid, every case relative to its own scale
(the sum of the absolute values of what the output adds up, or the largest reference entry of a gradient tensor); a case fails when its
own error exceeds 4 times that.  Where the distance is 0 by construction (the degenerate inputs) equality is required.
Measured on an MI355X (worst error over the grid / floor of the grid; the bound is 4):
  gpode_reparam_draws_bwd   gmu 4.89e-7 / 4.89e-7 = 1.00, glogvar 2.36e-7 / 2.41e-7 = 0.98 (48 cases; the gmu distance is 0 in 8 of them)
  gpode_elbo_iw_fwd         loss 1.19e-7 / 1.55e-7 = 0.77, -mean iw 8.94e-8 / 9.00e-8 = 0.99, -mean lw 1.08e-7 / 1.28e-7 = 0.84 (distance
                            0 in 30 of 128 cases), kl_u 8.24e-8 / 9.71e-8 = 0.85, ess 1.82e-5 / 1.82e-5 = 1.00 (distance 0 in 32 cases)
  gpode_elbo_iw_bwd         grow 9.63e-5 / 9.64e-5 = 1.00, glw 9.48e-5 / 9.48e-5 = 1.00 (a weight moves by 1e-4 when its a of 2e3 moves
                            by one unit in the last place), dUm 1.00e-7 / 1.00e-7 = 1.00, dUs 3.82e-7 / 3.82e-7 = 1.00
  the _len composition      (frame 8, T 4 | frame 784, T 3; one case each, so `out` is the largest of the five outputs' figures)
                            out 0.60 | 2.05 (loss alone: 1.07e-7 against a distance of 1.27e-8, one unit in the last place against a
                            lucky float32 evaluation -- the coin flip named above), grow 0.36 | 0.21, glw 0.89 | 0.24, ga 0.70 | 0.65
  Jensen: the smallest gap is -1.06e-4 (K = 1, where it is round-off), the largest 7.27 nats.

1  gpode_reparam_draws_bwd: K in {1,3}, N in {1,5}, q in {1,6}, gz dense (ldgz = q) and as the second half of a (K,N,2q) state gradient
   (ldgz = 2q), each of gz / glw NULL in turn.
2  gpode_elbo_iw_fwd / _bwd on iw_ref evaluated on the same float32 (lpart, lw): L in {1,2}, K in {1,2,8,64}, N in {1,3}, nsplit in
   {1,3}, M in {2,5}, Do in {1,3}; a of magnitude 2e3 with a spread of 3 nats over the draws, as real rows have.  Jensen on the device
   output: -out[1] >= mean a - 1e-3 (K = 1: equality), 1e-3 being 8 units in the last place of 2e3 for the roundings of a sum of <= 6
   groups and a mean.  A second run gives the same bits, and the seed of the ess output changes nothing.
3  the two degenerate inputs of test_iw_host.py: equal a over k -> grow == (1/K) c and ess == K exactly; one draw 1000 nats ahead ->
   grow one-hot times c, every other weight exactly 0, ess == 1 exactly (c = -nobs / (L N), g_loss = 1 alone).
4  both refusal lists: nothing is written (the NaN fill is intact).
5  gpode_elbo_iw_bwd_ll against gpode_elbo_iw_bwd + gpode_sigmoid_loglik_bwd: torch.equal on ga, grow, glw, dUm, dUs; frame in {4, 784}
   x T in {1,3} -- no row a multiple of the logit blocks' span of 2048 elements, 2352 taking two blocks -- and (1024, 2): one that is.
6  the _len composition: gpode_sigmoid_loglik_fwd_len -> gpode_elbo_iw_fwd / _bwd -> gpode_sigmoid_loglik_bwd_len with n_obs = (0, T,
   a partial count) and NaN in every padded target: the rows of the empty sequence are exactly 0, padded logits get exactly 0, the stage
   matches iw_ref on the masked sums and ga matches grow[row] times the Bernoulli derivative of the float32 z."""
import functools
import itertools

import pytest
import torch

import iw_ref as W
import loss_routes as R

pytestmark = pytest.mark.gpu

NOBS = R.NOBS
SEEDS = R.SEED_VALUES + (0.5,)                       # g0 .. g3, and a seed for the ess output that must change nothing
F64, F32 = torch.float64, torch.float32


def _scalars(bf, values):
    return [None if v is None else bf.new('g%d' % i, 1, torch.tensor([v])) for i, v in enumerate(values)]


def _us(M, Do, g):
    Us = 0.01 * torch.randn(Do, M * (M + 1) // 2, generator=g)
    Us[:, W.diag_index(M)] = 0.5 + torch.rand(Do, M, generator=g)
    return Us


def _err(got, ref, scale=None):
    s = float(ref.abs().max()) if scale is None else float(scale)
    return float((got.double().reshape(-1) - ref.reshape(-1)).abs().max()) / max(s, 1e-300)


def _judge(results, what):
    """results: [(case, {output: (kernel error, float32 distance)})] -> prints every figure, then asserts error <= 4 x the grid's floor"""
    names = list(results[0][1])
    floor = {k: max(r[k][1] for _, r in results) for k in names}
    worst = {k: max(r[k][0] for _, r in results) for k in names}
    zero = {k: sum(1 for _, r in results if r[k][1] == 0) for k in names}
    print('%s, %d cases: %s' % (what, len(results), {k: 'worst %.2e floor %.2e ratio %.2f (floor 0 in %d cases)'
                                                     % (worst[k], floor[k], worst[k] / floor[k] if floor[k] else 0.0, zero[k]) for k in names}))
    bad = [(c, k, r[k][0], floor[k]) for c, r in results for k in names if not r[k][0] <= 4 * floor[k]]
    assert not bad, bad[:8]


# ---- 1. the adjoint of the K draws ------------------------------------------------------------------------------------------------------
DRAWS = list(itertools.product((1, 3), (1, 5), (1, 6), ('dense', 'half'), ('', 'gz', 'glw')))


def _draws_case(K, N, q, layout, null):
    g = R._gen('iw draws', K, N, q, layout, null)
    h = torch.cat((torch.randn(N, q, generator=g), 0.7 * torch.randn(N, q, generator=g) - 1), 1)
    eps = torch.randn(K, N, q, generator=g)
    W_ = q if layout == 'dense' else 2 * q
    gfull = torch.randn(K, N, W_, generator=g)
    col = W_ - q
    gz = None if null == 'gz' else gfull[..., col:]
    glw = None if null == 'glw' else torch.randn(K, N, generator=g)
    bf, tags = R.Bufs(), {}
    hd, ed = bf.new('h', h.numel(), h), bf.new('eps', eps.numel(), eps)
    gzd = None if gz is None else bf.new('gz', gfull.numel(), gfull)
    glwd = None if glw is None else bf.new('glw', glw.numel(), glw)
    gh = bf.new('gh', N * 2 * q)
    R._call(tags, 'bwd', 'gpode_reparam_draws_bwd', None if gzd is None else gzd[col:], W_, glwd, hd, hd[q:], 2 * q, ed, gh, gh[q:], 2 * q, K, N, q)
    assert not bf.problems(), bf.problems()
    assert tags == dict(bwd='reparam_draws_bwd'), tags
    got = gh.cpu().view(N, 2 * q)
    out = {}
    for dt in (F64, F32):
        args = [t.to(dt) if t is not None else None for t in (h[:, :q], h[:, q:], eps, gz, glw)]
        out[dt] = W.draws_grads(*args)
    return {name: (_err(got[:, i * q:(i + 1) * q], out[F64][i]), _err(out[F32][i], out[F64][i]))
            for i, name in enumerate(('gmu', 'glogvar'))}


def test_draws_backward_against_the_reference():
    _judge([(c, _draws_case(*c)) for c in DRAWS], 'gpode_reparam_draws_bwd')


# ---- 2. the loss stage ------------------------------------------------------------------------------------------------------------------
STAGE = list(itertools.product((1, 2), (1, 2, 8, 64), (1, 3), (1, 3), (2, 5), (1, 3)))


def _stage_inputs(L, K, N, ns, M, Do, ll=None):
    g = R._gen('iw stage', L, K, N, ns, M, Do)
    if ll is None:
        ll = -2000.0 + 3.0 * torch.randn(L, K, N, generator=g)
    lpart = (ll.reshape(-1, 1) / ns + 0.5 * torch.randn(L * K * N, ns, generator=g)).float().contiguous()
    if ns == 1:
        lpart = ll.reshape(-1, 1).float().contiguous()
    return dict(lpart=lpart, lw=-3.0 + 2.0 * torch.randn(K, N, generator=g), Um=torch.randn(M, Do, generator=g), Us=_us(M, Do, g))


def _stage_run(d, L, K, N, ns, M, Do, seeds=SEEDS):
    """gpode_elbo_iw_fwd and _bwd once -> outputs on the CPU"""
    rows, P = L * K * N, M * (M + 1) // 2
    bf, tags = R.Bufs(), {}
    lp, lw = bf.new('lpart', rows * ns, d['lpart']), bf.new('lw', K * N, d['lw'])
    Um, Us = bf.new('Um', M * Do, d['Um']), bf.new('Us', Do * P, d['Us'])
    out = bf.new('out', 5 + R.ELBO_PARTS, output=False)
    grow, glw, dUm, dUs = bf.new('grow', rows), bf.new('glw', K * N), bf.new('dUm', M * Do), bf.new('dUs', Do * P)
    gs = _scalars(bf, seeds)
    R._call(tags, 'fwd', 'gpode_elbo_iw_fwd', lp, rows, ns, lw, L, K, N, M, Do, Um, Us, NOBS, out)
    R._call(tags, 'bwd', 'gpode_elbo_iw_bwd', *gs, lp, rows, ns, lw, L, K, N, M, Do, Um, Us, NOBS, grow, glw, dUm, dUs)
    assert not bf.problems(), bf.problems()
    assert tags == dict(fwd='elbo_iw_fwd', bwd='elbo_iw_bwd'), tags
    res = dict(out=out[:5].cpu(), grow=grow.cpu(), glw=glw.cpu().view(K, N), dUm=dUm.cpu().view(M, Do), dUs=dUs.cpu().view(Do, P))
    assert bool(torch.isfinite(res['out']).all()), res['out']
    return res


def _stage_refs(d, L, K, N, M, seeds=SEEDS):
    """iw_ref on the same float32 inputs, in float64 and in float32 -> {dtype: (out, grow, glw, dUm, dUs)}, the scales of out"""
    sd = tuple(0.0 if s is None else s for s in seeds)
    refs = {dt: W.objective_grads(*(d[k].to(dt) for k in ('lpart', 'lw', 'Um', 'Us')), L, K, N, M, NOBS, sd) for dt in (F64, F32)}
    a = W.rows_of(d['lpart'].double(), L, K, N) + d['lw'].double()[None]
    s_iw = float(a.abs().max(1).values.mean())
    ku_abs = float(W.svgp_kl_abs(d['Um'].double(), d['Us'].double(), M))
    return refs, [s_iw * NOBS + ku_abs, s_iw, float(d['lw'].double().abs().mean()), ku_abs, float(K)]


OUT_NAMES = ('loss', 'iw_nll', 'kl_mc', 'kl_u', 'ess')


def _stage_errors(got, refs, scales):
    r64, r32 = refs[F64], refs[F32]
    e = {n: (_err(got['out'][i], r64[0][i], scales[i]), _err(r32[0][i], r64[0][i], scales[i])) for i, n in enumerate(OUT_NAMES)}
    for i, n in enumerate(('grow', 'glw', 'dUm', 'dUs'), 1):
        e[n] = (_err(got[n], r64[i]), _err(r32[i], r64[i]))
    return e


@functools.lru_cache(maxsize=None)
def _stage_all():
    res = []
    for c in STAGE:
        L, K, N, ns, M, Do = c
        d = _stage_inputs(*c)
        got = _stage_run(d, *c)
        refs, scales = _stage_refs(d, L, K, N, M)
        res.append((c, _stage_errors(got, refs, scales), got, d))
    return res


def test_stage_against_the_reference():
    _judge([(c, e) for c, e, _, _ in _stage_all()], 'gpode_elbo_iw_fwd / _bwd')


def test_jensen_on_the_device_output():
    gaps = []
    for (L, K, N, ns, M, Do), _, got, d in _stage_all():
        a = W.rows_of(d['lpart'].double(), L, K, N) + d['lw'].double()[None]
        gap = -float(got['out'][1]) - float(a.mean())
        gaps.append(gap)
        assert gap >= -1e-3, ((L, K, N, ns), gap)
        if K == 1:
            assert abs(gap) <= 1e-3, ((L, K, N, ns), gap)
    print('Jensen gaps: min %.3e max %.3e' % (min(gaps), max(gaps)))
    assert max(gaps) > 0.1                            # the inequality is not an equality on these inputs


def test_stage_is_reproducible_and_the_ess_seed_is_inert():
    c = (2, 8, 3, 3, 5, 3)
    d = _stage_inputs(*c)
    a, b = _stage_run(d, *c), _stage_run(d, *c)
    no_ess = _stage_run(d, *c, seeds=SEEDS[:4] + (None,))
    other = _stage_run(d, *c, seeds=SEEDS[:4] + (-7.0,))
    for k in a:
        assert torch.equal(R._bits(a[k]), R._bits(b[k])), k
        assert torch.equal(R._bits(a[k]), R._bits(no_ess[k])) and torch.equal(R._bits(a[k]), R._bits(other[k])), k


def test_null_seeds_mean_zero():
    c = (2, 3, 3, 1, 2, 1)
    L, K, N, ns, M, Do = c
    d = _stage_inputs(*c)
    floor = {k: max(e[k][1] for _, e, _, _ in _stage_all()) for k in ('grow', 'glw', 'dUm', 'dUs')}      # the grid's floors
    for seeds in ((1.0, None, None, None, None), (None, None, 0.45, None, None), (None, -0.7, None, 2.1, None)):
        got = _stage_run(d, *c, seeds=seeds)
        refs, scales = _stage_refs(d, L, K, N, M, seeds=seeds)
        e = _stage_errors(got, refs, scales)
        for k in ('grow', 'glw', 'dUm', 'dUs'):
            if float(refs[F64][('grow', 'glw', 'dUm', 'dUs').index(k) + 1].abs().max()) == 0:
                assert bool((got[k] == 0).all()), (seeds, k)
            else:
                assert e[k][0] <= 4 * floor[k], (seeds, k, e[k], floor[k])


# ---- 3. the degenerate inputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 2, 8, 64])
def test_degenerate_inputs_are_exact(K):
    L, N, ns, M, Do = 2, 3, 1, 2, 1
    g = R._gen('iw degenerate', K)
    base = (-2000.0 + 3.0 * torch.randn(L, 1, N, generator=g)).float()
    c32 = torch.tensor(-NOBS, dtype=F32) / torch.tensor(float(L * N), dtype=F32)
    seeds = (1.0, None, None, None, None)
    # equal a over k: every weight is exactly 1/K
    d = _stage_inputs(L, K, N, ns, M, Do, ll=base.expand(L, K, N).contiguous())
    d['lw'] = torch.zeros(K, N)
    got = _stage_run(d, L, K, N, ns, M, Do, seeds=seeds)
    assert torch.equal(got['grow'], (torch.tensor(1.0 / K, dtype=F32) * c32).expand(L * K * N).contiguous()), got['grow']
    assert float(got['out'][4]) == float(K)
    # one draw ahead by 1000 nats: one-hot
    ll = base.expand(L, K, N).clone()
    ahead = K // 2
    ll[:, ahead] += 1000.0
    d = _stage_inputs(L, K, N, ns, M, Do, ll=ll)
    d['lw'] = torch.zeros(K, N)
    got = _stage_run(d, L, K, N, ns, M, Do, seeds=seeds)
    onehot = torch.zeros(L, K, N)
    onehot[:, ahead] = 1.0
    assert torch.equal(got['grow'].view(L, K, N), onehot * c32), got['grow']
    assert torch.equal(got['glw'], (onehot * c32).sum(0))
    assert float(got['out'][4]) == 1.0


# ---- 4. the refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['null lpart', 'null lw', 'null Um', 'null out', 'K = 0', 'K = 65', 'rows', 'rows > 65535', 'nsplit = 0'])
def test_stage_refusals_write_nothing(case):
    L, K, N, ns, M, Do = 2, 3, 2, 1, 2, 1
    rows, P = L * K * N, 3
    bf = R.Bufs()
    z = lambda name, n: bf.new(name, n, torch.zeros(n))
    lp, lw, Um, Us = z('lpart', rows), z('lw', K * N), z('Um', M * Do), bf.new('Us', Do * P, torch.ones(Do * P))
    X, zz = z('X', N * 4), bf.new('z', rows * 4, torch.full((rows * 4,), 0.5))
    out, grow, glw, dUm, dUs, ga = (bf.new(k, n) for k, n in (('out', 5 + R.ELBO_PARTS), ('grow', rows), ('glw', K * N), ('dUm', M * Do),
                                                             ('dUs', Do * P), ('ga', rows * 4)))
    o = out
    if case == 'null lpart':
        lp = None
    elif case == 'null lw':
        lw = None
    elif case == 'null Um':
        Um = None
    elif case == 'null out':
        o, grow = None, None
    elif case == 'K = 0':
        K = 0
    elif case == 'K = 65':
        K = 65
    elif case == 'rows':
        rows -= 1
    elif case == 'rows > 65535':
        L, K, N, rows = 1, 64, 1024, 65536
    else:
        ns = 0
    gs = [None] * 5
    with pytest.raises(R.Refused, match='gpode_elbo_iw_fwd'):
        R._call({}, 'x', 'gpode_elbo_iw_fwd', lp, rows, ns, lw, L, K, N, M, Do, Um, Us, NOBS, o)
    with pytest.raises(R.Refused, match='gpode_elbo_iw_bwd'):
        R._call({}, 'x', 'gpode_elbo_iw_bwd', *gs, lp, rows, ns, lw, L, K, N, M, Do, Um, Us, NOBS, grow, glw, dUm, dUs)
    with pytest.raises(R.Refused, match='gpode_elbo_iw_bwd_ll'):
        R._call({}, 'x', 'gpode_elbo_iw_bwd_ll', *gs, lp, rows, ns, lw, L, K, N, M, Do, Um, Us, NOBS, grow, glw, dUm, dUs, X, zz, ga,
                max(rows, 1) * 4, N * 4)
    assert bf.untouched(), 'a refused call wrote an output'
    assert not [p for p in bf.problems() if 'guard' in p]


@pytest.mark.parametrize('case', ['logits no whole rows', 'X does not tile', 'null z'])
def test_fused_backward_refusals_write_nothing(case):
    L, K, N, ns, M, Do = 2, 3, 2, 1, 2, 1
    rows, P, inner = L * K * N, 3, 4
    bf = R.Bufs()
    z = lambda name, n: bf.new(name, n, torch.zeros(n))
    lp, lw, Um, Us = z('lpart', rows), z('lw', K * N), z('Um', M * Do), bf.new('Us', Do * P, torch.ones(Do * P))
    X, zz = z('X', N * inner), bf.new('z', rows * inner, torch.full((rows * inner,), 0.5))
    grow, glw, dUm, dUs, ga = (bf.new(k, n) for k, n in (('grow', rows), ('glw', K * N), ('dUm', M * Do), ('dUs', Do * P), ('ga', rows * inner)))
    n, nX = rows * inner, N * inner
    if case == 'logits no whole rows':
        n -= 1
    elif case == 'X does not tile':
        nX = 5
    else:
        zz = None
    with pytest.raises(R.Refused, match='gpode_elbo_iw_bwd_ll'):
        R._call({}, 'x', 'gpode_elbo_iw_bwd_ll', *([None] * 5), lp, rows, ns, lw, L, K, N, M, Do, Um, Us, NOBS, grow, glw, dUm, dUs, X, zz, ga, n, nX)
    assert bf.untouched(), 'a refused call wrote an output'


@pytest.mark.parametrize('case', ['null mu', 'null eps', 'null gmu', 'K = 0', 'K = 65', 'ld < q', 'ldgz < q', 'N = 0'])
def test_draws_backward_refusals_write_nothing(case):
    K, N, q = 3, 5, 6
    bf = R.Bufs()
    z = lambda name, n: bf.new(name, n, torch.zeros(n))
    h, eps, gz, glw = z('h', N * 2 * q), z('eps', K * N * q), z('gz', K * N * q), z('glw', K * N)
    gh = bf.new('gh', N * 2 * q)
    mu, e, gmu, ld, ldgz = h, eps, gh, 2 * q, q
    if case == 'null mu':
        mu = None
    elif case == 'null eps':
        e = None
    elif case == 'null gmu':
        gmu = None
    elif case == 'K = 0':
        K = 0
    elif case == 'K = 65':
        K = 65
    elif case == 'ld < q':
        ld = q - 1
    elif case == 'ldgz < q':
        ldgz = q - 1
    else:
        N = 0
    with pytest.raises(R.Refused, match='gpode_reparam_draws_bwd'):
        R._call({}, 'x', 'gpode_reparam_draws_bwd', gz, ldgz, glw, mu, h[q:], ld, e, gmu, gh[q:], 2 * q, K, N, q)
    assert bf.untouched(), 'a refused call wrote an output'


# ---- 5. the fused backward against the pair ---------------------------------------------------------------------------------------------
FUSED = [(4, 1), (4, 3), (784, 1), (784, 3), (1024, 2)]
SPAN = 2048                                          # kIwSpan: the elements of a row one logit block takes


@pytest.mark.parametrize('frame,T', FUSED)
def test_fused_backward_has_the_bits_of_the_pair(frame, T):
    L, K, N, M, Do = 2, 3, 2, 5, 3
    rows, inner, P = L * K * N, T * frame, M * (M + 1) // 2
    g = R._gen('iw fused', frame, T)
    X_h, a_h = R._x_form((N, T, frame), 'norm', g), R._logits((rows, inner), g)
    d = _stage_inputs(L, K, N, 1, M, Do)
    ns = R.sigmoid_loglik_splits(rows, inner)
    nX = X_h.numel()
    bf, tags = R.Bufs(), {}
    X, a = bf.new('X', nX, X_h), bf.new('a', rows * inner, a_h)
    z, part = bf.new('z', rows * inner), bf.new('part', rows * ns)
    lw, Um, Us = bf.new('lw', K * N, d['lw']), bf.new('Um', M * Do, d['Um']), bf.new('Us', Do * P, d['Us'])
    gs = _scalars(bf, SEEDS)
    R._call(tags, 'sll', 'gpode_sigmoid_loglik_fwd', X, a, z, part, rows, inner, nX, ns)
    o = {}
    for tag in ('pair', 'fused'):
        o[tag] = {k: bf.new(tag + k, n) for k, n in (('grow', rows), ('glw', K * N), ('dUm', M * Do), ('dUs', Do * P), ('ga', rows * inner))}
    p, f = o['pair'], o['fused']
    R._call(tags, 'bwd', 'gpode_elbo_iw_bwd', *gs, part, rows, ns, lw, L, K, N, M, Do, Um, Us, NOBS, p['grow'], p['glw'], p['dUm'], p['dUs'])
    R._call(tags, 'sll_bwd', 'gpode_sigmoid_loglik_bwd', X, z, p['grow'], p['ga'], rows, inner, nX)
    R._call(tags, 'll', 'gpode_elbo_iw_bwd_ll', *gs, part, rows, ns, lw, L, K, N, M, Do, Um, Us, NOBS, f['grow'], f['glw'], f['dUm'], f['dUs'],
            X, z, f['ga'], rows * inner, nX)
    assert not bf.problems(), bf.problems()
    assert tags == dict(sll='sigmoid_loglik_fwd', bwd='elbo_iw_bwd', sll_bwd='sigmoid_loglik_bwd', ll='elbo_iw_loglik_bwd'), tags
    assert (inner % SPAN == 0) == ((frame, T) == (1024, 2))
    for k in p:
        assert torch.equal(R._bits(p[k].cpu()), R._bits(f[k].cpu())), k
    assert float(p['ga'].abs().max()) > 0


def test_fused_shapes_cover_one_block_and_several_per_row():
    blocks = {(f, T): -(-(f * T) // SPAN) for f, T in FUSED}
    assert 1 in blocks.values() and 2 in blocks.values(), blocks
    assert any((f * T) % SPAN == 0 for f, T in FUSED) and any((f * T) % SPAN != 0 and f * T > SPAN for f, T in FUSED)


# ---- 6. the _len composition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('frame,T', [(8, 4), (784, 3)])
def test_len_composition(frame, T):
    L, K, N, M, Do = 2, 3, 3, 5, 3
    counts = (0, T, T - 1 if T > 2 else 1)
    rows, inner, P = L * K * N, T * frame, M * (M + 1) // 2
    g = R._gen('iw len', frame, T)
    X_h, a_h = R._x_form((N, T, frame), 'norm', g), R._logits((rows, inner), g)
    for n, k in enumerate(counts):
        X_h[n, k:] = float('nan')
    assert bool(torch.isnan(X_h).any())
    d = _stage_inputs(L, K, N, 1, M, Do)
    ns = R.sigmoid_loglik_splits(rows, inner)
    nX = X_h.numel()
    bf, tags = R.Bufs(), {}
    X, a = bf.new('X', nX, X_h), bf.new('a', rows * inner, a_h)
    n_obs = torch.tensor(counts, dtype=torch.int32, device='cuda')
    z, part = bf.new('z', rows * inner), bf.new('part', rows * ns)
    lw, Um, Us = bf.new('lw', K * N, d['lw']), bf.new('Um', M * Do, d['Um']), bf.new('Us', Do * P, d['Us'])
    out = bf.new('out', 5 + R.ELBO_PARTS, output=False)
    grow, glw, dUm, dUs, ga = (bf.new(k, n_) for k, n_ in (('grow', rows), ('glw', K * N), ('dUm', M * Do), ('dUs', Do * P), ('ga', rows * inner)))
    gs = _scalars(bf, SEEDS)
    R._call(tags, 'sll', 'gpode_sigmoid_loglik_fwd_len', X, a, z, part, rows, inner, nX, ns, n_obs, T, frame)
    R._call(tags, 'fwd', 'gpode_elbo_iw_fwd', part, rows, ns, lw, L, K, N, M, Do, Um, Us, NOBS, out)
    R._call(tags, 'bwd', 'gpode_elbo_iw_bwd', *gs, part, rows, ns, lw, L, K, N, M, Do, Um, Us, NOBS, grow, glw, dUm, dUs)
    R._call(tags, 'sll_bwd', 'gpode_sigmoid_loglik_bwd_len', X, z, grow, ga, rows, inner, nX, n_obs, T, frame)
    assert not bf.problems(), bf.problems()
    assert tags == dict(sll='sigmoid_loglik_fwd_len', fwd='elbo_iw_fwd', bwd='elbo_iw_bwd', sll_bwd='sigmoid_loglik_bwd_len'), tags
    part_h, z_h, ga_h = part.cpu().view(L, K, N, ns), z.cpu().double().view(L, K, N, T, frame), ga.cpu().view(L, K, N, T, frame)
    assert bool((part_h[:, :, 0] == 0).all()), 'the sequence without a frame must sum to exactly 0'
    obs = torch.tensor([[t < k for t in range(T)] for k in counts])
    assert bool((ga_h[:, :, ~obs] == 0).all()) and bool(torch.isfinite(ga_h).all())
    # the stage on the masked sums
    dd = dict(d, lpart=part.cpu().view(rows, ns))
    refs, scales = _stage_refs(dd, L, K, N, M)
    got = dict(out=out[:5].cpu(), grow=grow.cpu(), glw=glw.cpu().view(K, N), dUm=dUm.cpu().view(M, Do), dUs=dUs.cpu().view(Do, P))
    e = _stage_errors(got, refs, scales)
    # ga on the observed frames: grow[row] (x/z - (1-x)/(1-z)) z (1-z) from the float32 z, in float64 and in float32
    x = torch.nan_to_num(X_h, nan=0.0)[None, None]

    def ga_ref(dt):
        zz, xx, gr = z_h.to(dt), x.to(dt), refs[dt][1].view(L, K, N, 1, 1)
        return torch.where(obs[None, None, :, :, None], gr * (xx / zz - (1 - xx) / (1 - zz)) * zz * (1 - zz), torch.zeros((), dtype=dt))
    e['ga'] = (_err(ga_h, ga_ref(F64)), _err(ga_ref(F32), ga_ref(F64)))
    e['out'] = (max(e[k][0] for k in OUT_NAMES), max(e[k][1] for k in OUT_NAMES))
    print('_len composition frame %d T %d counts %s: %s' % (frame, T, counts, {k: '%.2e / %.2e' % v for k, v in e.items()}))
    for k in ('out', 'grow', 'glw', 'ga'):
        assert e[k][0] <= 4 * e[k][1], (k, e[k])
