"""Every route of the BatchNorm family and the channel reductions (csrc/vae_norm.hip), driven through the C ABI (gpode_bn_fwd,
gpode_bn_stats, gpode_bn_bwd, gpode_bn_moments / _finalize / _apply / _bwd_sums / _bwd_apply, gpode_bn_eval, gpode_bn_eval_table,
gpode_chan_sum, gpode_defer_reductions / gpode_flush_reductions) at the smallest shapes that sit on each edge (bn_routes.py).

Per case (bn_routes.launch / check): (a) gpode_last_launch() after every call equals the tag bn_routes.expected names -- a restatement
of kBnSmallFwd = 20000 and kBnSmallBwd = 2048 elements per channel that never asks the library; (b) outputs and gradients within 2e-5
of the fp64 reference relative to its largest entry (test_gpu_vae_layers.TOL), save_mean / save_invstd / running statistics / the table
and evaluation mode within 1e-5, in the max norm -- the inputs keep every pre-activation 1e-4 away from zero, so no ReLU mask is a
coin-flip; gx_chansum (whose exact value over a whole batch is zero) against the fp64 sum of the kernel's own gx within
2^-24 (ceil(bps HW / 256) + 12) sum |gx|; (c) every output and the scratch, exactly gpode_bn_scratch(B, C) floats, are NaN-filled with
4096 guard floats behind each: the guards come back untouched and no NaN is left in an output; (d) num_batches_tracked goes from 7 to 8;
(e) a second run is bit-identical.

The cases: both sides of the two thresholds at two image sizes, relu 0 / 1, channel means of 0 and 100 standard deviations (a
chan_shift that returned 0 is off by 3e-4 in invstd there); the edges of pick(B) -- B in {1, 2, 63, 64, 65, 127, 128, 129, 130, 193} --
on the scalar (13 x 13) and the float4 (6 x 6) path for forward, backward, evaluation mode and gpode_chan_sum; image sizes 1, 3, 9, 49,
289, 784, 1296 with C in {1, 5, 64}; every case under a threshold again in ONE fresh child process under GPODE_BN_ONE_LAUNCH=0, where
it takes the two-launch kernels; the statistics-only form against gpode_bn_fwd bit for bit on both routes; the five cross-rank
pieces on one device with 1, 2, 4 (unequal, one of one image) and 64 simulated ranks whose means differ by the order of the spread,
against the whole-batch layer; W = 0 and W = 65 refused; one non-zero image of 130 attributed to the right slab; gpode_chan_sum
against its worst-case bound; the deferred reduction queue, past its 24 slots; gpode_bn_eval_table at C in {1, 63, 64, 65}; B HW = 1
refused in torch's words.  The last test requires the union of the tags seen to contain bn_routes.REQUIRED_TAGS.

Every case with running statistics runs a second time with momentum 1: running_var is then the unbiased batch variance itself (with
momentum 0.1 the factor count / (count - 1) is 5e-6 of running_var at 2e4 elements per channel, under its bound), running_mean is
save_mean bit for bit.  The inputs are drawn so that rounding the exact statistics to fp32 moves no compared quantity by more than a
quarter of its bound (bn_routes._rounding_sensitivity; the largest is 4.6e-6).

Measured on an MI355X, largest error over all cases, child process included (bound): outputs and gradients -- bn_fwd 2.0e-6 on both
forms, bn_stats + bn_apply 1.7e-6 on both, bn_bwd 4.5e-6, one launch 4.3e-6, cross-rank pieces 5.4e-6 (2e-5); statistics -- bn_fwd
4.7e-6, one launch 3.3e-6, bn_stats 2.4e-6, one launch 2.1e-6, cross-rank 2.6e-6, the unbiased variance 2.6e-6 (1e-5); bn_eval 1.3e-7,
bn_eval_table + bn_apply 1.1e-7 (1e-5); gpode_chan_sum 0.12 and gx_chansum 0.16 of the worst-case summation bound; one rank against
the local route 6.3e-7 (1e-6; 3.6e-6 in ggamma before k_bn_finalize took rank 0's mean as its shift: an ulp of a mean of 100 standard
deviations); attribution -- gpode_chan_sum 8.5e-8, save_mean 9.5e-6 on the two-launch and 7.3e-6 on the one-launch form at b* = 0,
where the shift is the mean of that image (~1) and the channel mean 0.008 is formed as shift + d, and 1.2e-7 at the other b* (1e-5).
No NaN of the fills reached an output and no guard was written; the module takes 6 s.

Each of these, built into the library once, turned red exactly what it should: chan_shift returning 0 -- all 140 training-mode cases
with offset 100 on both forms and the six cross-rank ones with up to four ranks (with 64 ranks of one or two images the variance
between the ranks dominates and the shift does not matter); count / (count - 1) replaced by 1 in k_bn_apply -- the 47 two-launch
gpode_bn_fwd cases with running statistics and the 27 comparisons with gpode_bn_stats, nothing else; k_bn_bwd_apply given one split
too few -- 99 of the 100 two-launch backward cases (in the one left, 40 x 1 x 1 x 1, the dropped slab is an image that the ReLU
masks) and all 16 cross-rank ones; the
n_r (mean_r - mean)^2 term dropped in k_bn_finalize -- the 12 cross-rank cases with more than one rank; the weights read as 1 in
k_bn_bwd_apply -- the 8 with unequal shards, (33, 33) passes."""
import pytest
import torch

import bn_routes as R

pytestmark = pytest.mark.gpu
SEEN = set()
MAXIMA = {}


@pytest.fixture(scope='module', autouse=True)
def _drop_cached_results():
    yield
    print('largest error per route:', {k: '%.1e' % v for k, v in sorted(MAXIMA.items())})
    R.child.cache_clear()
    R._reference.cache_clear()
    R._inputs.cache_clear()


def _param(cases):
    assert len(set(cases)) == len(cases)
    return pytest.mark.parametrize('c', cases, ids=[R.case_id(c) for c in cases])


def _lib():
    from vae_gp_ode_amd import _lib
    return _lib.load()


def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def _untouched(*tensors):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) for t in tensors)


# ---- items 1-3: thresholds, split edges, image sizes, in this process ----------------------------------------------------------------
@_param(R.threshold_cases())
def test_route_thresholds(c):
    R.check(c, R.launch(c), R.one_launch_on(), SEEN, MAXIMA)


@_param(R.split_cases())
def test_split_edges(c):
    R.check(c, R.launch(c), R.one_launch_on(), SEEN, MAXIMA)


@_param(R.image_cases())
def test_image_sizes(c):
    R.check(c, R.launch(c), R.one_launch_on(), SEEN, MAXIMA)


# ---- item 4: the same under GPODE_BN_ONE_LAUNCH=0 ------------------------------------------------------------------------------------
@_param(R.child_cases())
def test_one_launch_switched_off(c):
    """shapes under a threshold on the two-launch kernels: the plain tags, the same tolerances"""
    got = R.child()[tuple(c)]
    R.check(c, got, False, SEEN, MAXIMA)
    assert not any('one launch' in t for t in got['tags'].values())


# ---- item 5: the statistics-only form --------------------------------------------------------------------------------------------------
STATS_PAIRS = [c for c in R.local_cases() if c.op == 'stats']


def _same_statistics(c, stats, fwd):
    s, f = stats['out'], fwd['out']
    for k in ('save_mean', 'save_invstd', 'running_mean', 'running_var', 'nbt', R.MOM1 + 'running_var', R.MOM1 + 'running_mean'):
        assert torch.equal(s[k], f[k]), (R.case_id(c), k)
    d = R.inputs(c)
    assert torch.equal(s['table'].reshape(c.C, 4), torch.stack([f['save_mean'], f['save_invstd'], d['gamma'], d['beta']], 1)), R.case_id(c)
    assert torch.equal(s['y'], f['y']), (R.case_id(c), 'gpode_bn_apply(table) against gpode_bn_fwd')


@_param(STATS_PAIRS)
def test_statistics_only_form_gives_the_bits_of_the_forward(c):
    """gpode_bn_stats against gpode_bn_fwd on the same input and the same route: statistics, counter and table bit for bit, and
    gpode_bn_apply with the table gives gpode_bn_fwd's y (both go through bn_affine)"""
    on = R.one_launch_on()
    f = c._replace(op='fwd')
    stats, fwd = R.launch(c), R.launch(f)
    assert ('one launch' in stats['tags']['stats']) == ('one launch' in fwd['tags']['fwd'])
    _same_statistics(c, stats, fwd)
    if R.expected(c, on) != R.expected(c, False):   # under the threshold: the two-launch pair from the child process as well
        stats, fwd = R.child()[tuple(c)], R.child()[tuple(f)]
        assert stats['tags']['stats'] == 'bn_stats' and fwd['tags']['fwd'] == 'bn_fwd'
        _same_statistics(c, stats, fwd)


# ---- item 6: the cross-rank pieces -------------------------------------------------------------------------------------------------------
@_param(R.xrank_cases())
def test_cross_rank_pieces(c):
    got = R.launch(c)
    R.check(c, got, R.one_launch_on(), SEEN, MAXIMA)
    if len(c.shards) == 1:                          # one rank: the local route to 1e-6
        loc = R.launch(c._replace(op='bwd', shards=()))
        for k in ('y', 'save_mean', 'save_invstd', 'running_mean', 'running_var', 'gx', 'ggamma', 'gbeta'):
            e = R.relerr(got['out'][k], loc['out'][k])
            print('  one rank against the local route: %s %.1e' % (k, e))
            assert e <= 1e-6, (k, e)
        assert int(loc['out']['nbt']) == int(got['out']['nbt']) == R.NBT0 + 1


@pytest.mark.parametrize('W', [0, 65])
def test_rank_count_outside_1_to_64_is_refused(W):
    lib, C, B, HW = _lib(), 3, 4, 9
    rows = max(W, 1)
    gathered, sums = torch.ones(rows, 2 * C + 1, device='cuda'), torch.ones(rows, 2 * C, device='cuda')
    gam, bet, wts = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda'), torch.ones(rows, device='cuda')
    x, gy = torch.randn(B, C, HW, device='cuda'), torch.randn(B, C, HW, device='cuda')
    sm, si, rm, rv, table = _nan(C), _nan(C), _nan(C), _nan(C), _nan(C, 4)
    nbt = torch.tensor([R.NBT0], device='cuda')
    p, st = R._ptr, R._stream()
    rc = lib.gpode_bn_finalize(p(gathered), W, p(gam), p(bet), p(sm), p(si), p(rm), p(rv), p(nbt), R.MOM, R.EPS, p(table), C, st)
    msg = lib.gpode_last_error().decode()
    assert rc != 0 and '64' in msg and 'gpode_bn_finalize' in msg, (rc, msg)
    assert _untouched(sm, si, rm, rv, table) and int(nbt) == R.NBT0
    gx, gg, gb, cs = _nan(B, C, HW), _nan(C), _nan(C), _nan(C)
    scratch = _nan(int(lib.gpode_bn_scratch(B, C)))
    mean, invstd = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    rc = lib.gpode_bn_bwd_apply(p(x), p(gy), p(gam), p(bet), p(mean), p(invstd), p(sums), p(wts), W, float(B * HW), p(gx), p(gg), p(gb), p(cs),
                                B, C, HW, 1, p(scratch), st)
    msg = lib.gpode_last_error().decode()
    assert rc != 0 and '64' in msg and 'gpode_bn_bwd_apply' in msg, (rc, msg)
    assert _untouched(gx, gg, gb, cs, scratch)


# ---- item 7: attribution --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [13, 6])
@pytest.mark.parametrize('bstar', [0, 2, 3, 129])
def test_one_image_is_attributed_once(bstar, H):
    """B = 130 gives slabs of 3 images: a tensor that is zero except in image b* must give that image's sums from gpode_chan_sum and
    that image's sum / N as save_mean -- a dropped, doubled or mis-slabbed image is the whole error"""
    lib, B, C, HW = _lib(), 130, 3, H * H
    assert R.pick(B)[1] == 3
    g = torch.Generator().manual_seed(40 + bstar)
    img = torch.randn(C, HW, generator=g) + 1.0
    x = torch.zeros(B, C, HW)
    x[bstar] = img
    want = img.double().sum(1)
    xd, p, st = x.cuda(), R._ptr, R._stream()
    out = _nan(C)
    assert lib.gpode_chan_sum(p(xd), p(out), B, C, HW, p(_nan(int(lib.gpode_bn_scratch(B, C)))), st) == 0
    assert lib.gpode_last_launch().decode() == 'chan_sum'
    e = ((out.cpu().double() - want).abs() / want.abs()).max().item()
    print('chan_sum: %.1e' % e)
    assert e < 1e-5
    y, sm, si = _nan(B, C, HW), _nan(C), _nan(C)
    gam, bet = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda')
    assert lib.gpode_bn_fwd(p(xd), p(gam), p(bet), p(y), p(sm), p(si), None, None, None, R.MOM, R.EPS, B, C, HW, 0,
                            p(_nan(int(lib.gpode_bn_scratch(B, C)))), st) == 0
    tag = lib.gpode_last_launch().decode()
    SEEN.add(tag)
    assert tag == R.expected(R.case('fwd', B, C, H, H), R.one_launch_on())['fwd']
    e = ((sm.cpu().double() - want / (B * HW)).abs() / (want / (B * HW)).abs()).max().item()
    print('save_mean [%s]: %.1e' % (tag, e))
    assert e < 1e-5


# ---- item 8: gpode_chan_sum accuracy is part of test_split_edges (op chan_sum: the bound of bn_routes.sum_terms) --------------------------
@_param([R.case('chan_sum', B, C, H, W, 0, off) for B, C, H, W, off in ((40, 64, 1, 1, 0), (7, 5, 3, 3, 100), (70, 1, 17, 17, 0), (16, 5, 36, 36, 100),
                                                                        (130, 4, 28, 28, 0))])
def test_chan_sum_accuracy(c):
    """against the fp64 sum within 2^-24 (ceil(bps HW / 256) + 12) sum |v| per channel, the bound computed from the case"""
    R.check(c, R.launch(c), R.one_launch_on(), SEEN, MAXIMA)


# ---- item 9: deferred reductions ---------------------------------------------------------------------------------------------------------------
def test_deferred_reductions_and_the_queue_limit():
    lib, p, st = _lib(), R._ptr, R._stream()
    c = R.case('bwd', 129, 4, 4, 4, 1, 100, chansum=True)                      # two-launch backward
    eager = R.launch(c)
    assert eager['tags']['bwd'] == 'bn_bwd'
    s = R.case('chan_sum', 130, 3, 13, 13)
    eager_sum = R.launch(s)
    d = {k: v.cuda() for k, v in R.inputs(c).items()}
    v = R.inputs(s)['x'].cuda()
    B, C, HW = c.B, c.C, c.H * c.W_img
    sm, si = eager['out']['save_mean'].cuda(), eager['out']['save_invstd'].cuda()
    gx, gg, gb, cs, out = _nan(B, C, HW), _nan(C), _nan(C), _nan(C), _nan(s.C)
    scr1, scr2 = _nan(int(lib.gpode_bn_scratch(B, C))), _nan(int(lib.gpode_bn_scratch(s.B, s.C)))
    outs = [_nan(s.C) for _ in range(30)]
    scrs = [_nan(int(lib.gpode_bn_scratch(s.B, s.C))) for _ in range(30)]
    lib.gpode_defer_reductions(2)
    try:
        assert lib.gpode_bn_bwd(p(d['x']), p(d['gy']), p(d['gamma']), p(d['beta']), p(sm), p(si), p(gx), p(gg), p(gb), p(cs), B, C, HW, 1, p(scr1), st) == 0
        assert lib.gpode_last_launch().decode() == 'bn_bwd'
        assert lib.gpode_chan_sum(p(v), p(out), s.B, s.C, s.H * s.W_img, p(scr2), st) == 0
        assert lib.gpode_last_launch().decode() == 'chan_sum'
        assert _untouched(cs, out), 'a deferred reduction ran before the flush'
        assert torch.equal(gx.cpu().reshape(-1), eager['out']['gx'])            # everything but the final reduction is there
        assert lib.gpode_flush_reductions(st) == 0
        torch.cuda.synchronize()
        assert torch.equal(cs.cpu(), eager['out']['gx_chansum']) and torch.equal(out.cpu(), eager_sum['out']['sums'])
        assert torch.equal(gg.cpu(), eager['out']['ggamma']) and torch.equal(gb.cpu(), eager['out']['gbeta'])
        # 30 jobs in one deferral: the queue holds 24, the rest launch at once
        for o, sc in zip(outs, scrs):
            assert lib.gpode_chan_sum(p(v), p(o), s.B, s.C, s.H * s.W_img, p(sc), st) == 0
        torch.cuda.synchronize()
        pending = [bool(torch.isnan(o).all()) for o in outs]
        assert pending == [True] * 24 + [False] * 6, pending
        assert lib.gpode_flush_reductions(st) == 0
        torch.cuda.synchronize()
        for o in outs:
            assert torch.equal(o.cpu(), eager_sum['out']['sums'])
    finally:
        lib.gpode_defer_reductions(2)               # drop whatever a failed assert left behind ...
        lib.gpode_defer_reductions(0)               # ... and leave recording mode
    # nothing is left behind: a call is eager again, and a flush has nothing to run
    o = _nan(s.C)
    assert lib.gpode_chan_sum(p(v), p(o), s.B, s.C, s.H * s.W_img, p(scr2), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(o.cpu(), eager_sum['out']['sums'])
    assert lib.gpode_flush_reductions(st) == 0


# ---- item 10: the evaluation-mode table ---------------------------------------------------------------------------------------------------------
@_param(R.eval_table_cases())
def test_eval_table(c):
    R.check(c, R.launch(c), R.one_launch_on(), SEEN, MAXIMA)


def test_eval_table_refuses_an_unaligned_table():
    lib, C, p = _lib(), 5, R._ptr
    v = [torch.ones(C, device='cuda') for _ in range(4)]
    buf = _nan(4 * C + 4)
    table = buf[1:4 * C + 1]
    assert table.data_ptr() % 16 == 4
    rc = lib.gpode_bn_eval_table(p(v[0]), p(v[1]), p(v[2]), p(v[3]), R.EPS, p(table), C, R._stream())
    assert rc != 0 and '16-byte aligned' in lib.gpode_last_error().decode()
    assert _untouched(buf)


# ---- the bug that was visible by reading ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('op', ['fwd', 'stats'])
def test_one_value_per_channel_is_refused(op):
    """B HW = 1: count / (count - 1) is 1 / 0 and running_var became NaN in silence; torch raises.  Refused in torch's words, nothing
    written.  (gpode_bn_moments accepts such a shard: test_cross_rank_pieces has one.)"""
    lib, C, p, st = _lib(), 3, R._ptr, R._stream()
    x, gam, bet = torch.randn(1, C, 1, device='cuda'), torch.ones(C, device='cuda'), torch.zeros(C, device='cuda')
    y, sm, si, table, scratch = _nan(1, C, 1), _nan(C), _nan(C), _nan(C, 4), _nan(int(lib.gpode_bn_scratch(1, C)))
    rm, rv = torch.full((C,), 0.25, device='cuda'), torch.full((C,), 0.75, device='cuda')
    nbt = torch.tensor([R.NBT0], device='cuda')
    if op == 'fwd':
        rc = lib.gpode_bn_fwd(p(x), p(gam), p(bet), p(y), p(sm), p(si), p(rm), p(rv), p(nbt), R.MOM, R.EPS, 1, C, 1, 1, p(scratch), st)
    else:
        rc = lib.gpode_bn_stats(p(x), p(gam), p(bet), p(sm), p(si), p(rm), p(rv), p(nbt), R.MOM, R.EPS, p(table), 1, C, 1, p(scratch), st)
    msg = lib.gpode_last_error().decode()
    assert rc != 0 and 'Expected more than 1 value per channel when training' in msg and 'gpode_bn_' + op in msg, (rc, msg)
    assert _untouched(y, sm, si, table, scratch)
    assert bool((rm == 0.25).all()) and bool((rv == 0.75).all()) and int(nbt) == R.NBT0
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        torch.nn.functional.batch_norm(torch.randn(1, C, 1, 1), None, None, training=True)


# ---- item 11: coverage -----------------------------------------------------------------------------------------------------------------------------
def test_every_route_was_reached():
    """The union of gpode_last_launch() over the tests above contains every tag expected() can return (skips on its own)."""
    table = set()
    for c in R.all_cases():
        for on in (True, False):
            table.update(R.expected(c, on).values())
    assert table == set(R.REQUIRED_TAGS), sorted(table ^ set(R.REQUIRED_TAGS))
    if not SEEN:
        pytest.skip('runs after the other tests of this module')
    assert set(R.REQUIRED_TAGS) <= SEEN, sorted(set(R.REQUIRED_TAGS) - SEEN)
