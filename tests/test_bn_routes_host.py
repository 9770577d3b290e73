"""CPU tests of the BatchNorm route helper (bn_routes.py) itself: for every case of the GPU lists the inputs keep the pre-activations
away from zero, the cross-rank reference (autograd on the whole batch) equals an independent fp64 emulation of the five pieces, and
expected() agrees with a restatement of pick() and of the two thresholds at their edges."""
import pytest
import torch

import bn_routes as R


@pytest.fixture(scope='module', autouse=True)
def _drop_cached_results():
    yield
    R._reference.cache_clear()
    R._inputs.cache_clear()


def test_case_lists_hold_no_duplicates_and_reach_every_tag():
    cases = R.all_cases()
    assert len(set(cases)) == len(cases)
    tags = set()
    for c in cases:
        tags.update(R.expected(c, True).values())
    assert tags == set(R.REQUIRED_TAGS), sorted(tags ^ set(R.REQUIRED_TAGS))
    child = R.child_cases()
    assert child and all('(one launch)' in ' '.join(R.expected(c, True).values()) for c in child)
    assert all('(one launch)' not in ' '.join(R.expected(c, False).values()) for c in cases)
    assert max(c.B * c.C * c.H * c.W_img for c in cases) <= 700_000


def test_inputs_keep_every_preactivation_away_from_zero():
    """reference() asserts min |pre-activation| >= 1e-4 itself; here additionally for both values of relu, and that both sides of the
    crossing are populated wherever a channel has more than a handful of elements"""
    lo = {}
    for c in R.all_cases():
        if R._family(c.op) == 'sum':
            continue
        for relu in (0, 1):
            ref = R.reference(c._replace(relu=relu))
            assert ref['pre_min'] >= R.MIN_PRE, (R.case_id(c), ref['pre_min'])
            lo[c.offset] = min(lo.get(c.offset, 1.0), ref['pre_min'])
        if c.B * c.H * c.W_img >= 1000:
            y = R.reference(c._replace(relu=1))['y']
            frac = (y > 0).double().mean((0, 2))
            assert (frac > 0.02).all() and (frac < 0.98).all(), (R.case_id(c), frac)
    print('smallest |pre-activation| per offset:', lo)


def test_inputs_are_well_conditioned_for_fp32_statistics():
    """rounding the exact statistics to fp32 changes no compared quantity by more than a quarter of the tolerance (asserted by
    inputs() itself, which redraws until it holds); the C = 1 case that needed a second draw is among them"""
    worst = max(float(R.inputs(c)['sensitivity']) for c in R.all_cases() if R._family(c.op) == 'train')
    print('largest sensitivity to fp32 statistics: %.1e' % worst)
    assert worst < R.TOL / 4
    first = R._draw(1000003 * 2 + 1009 + 31 * 36 + 36 + 700, 'train', 2, 1, 36, 36, 100, ())
    assert R._rounding_sensitivity(first, (), 2) > R.TOL                      # gbeta 78, ggamma 5.1, a mean of 104 standard deviations


def test_inputs_have_the_stated_offset_and_signs():
    c = R.case('fwd', 555, 3, 6, 6, 1, 100)
    d = R.inputs(c)
    x = d['x'].double().transpose(0, 1).reshape(3, -1)
    ratio = x.mean(1) / x.std(1)
    assert ((ratio - 100).abs() < 2).all(), ratio
    assert d['x'].dtype == torch.float32 and d['beta'].dtype == torch.float32
    signs = torch.cat([R.inputs(R.case('fwd', 40, 64, 1, 1, 1, o))['gamma'] for o in (0, 100)])
    assert 0.15 < (signs < 0).double().mean() < 0.45 and (signs.abs() >= 0.5).all() and (signs.abs() <= 1.5).all()
    # shard means that differ by the order of the spread: n_r (mean_r - mean)^2 is a large part of the variance
    c = R.case('xrank', 204, 5, 3, 3, 1, 100, True, True, (3, 70, 1, 130))
    x = R.inputs(c)['x'].double()
    between = sum(n * 9 * (x[sl].mean((0, 2)) - x.mean((0, 2))) ** 2 for sl, n in R._shard_slices(c)) / (204 * 9)
    assert (between / x.var((0, 2), unbiased=False) > 0.3).all()


@pytest.mark.parametrize('c', R.xrank_cases(), ids=[R.case_id(c) for c in R.xrank_cases()])
def test_xrank_reference_equals_the_emulated_pieces(c):
    ref, emu = R.reference(c), R.emulate_xrank(c)
    for k, v in emu.items():
        if k == 'gx':
            e = max(R.relerr(v[sl], ref[k][sl]) for sl, _ in R._shard_slices(c))
        else:
            e = R.relerr(v, ref[k])
        assert e < 1e-12, (k, e)


def test_single_rank_reference_is_autograd():
    """with one shard the per-shard sums are the layer's own affine gradients and gx is autograd's"""
    for c in (R.case('bwd', 129, 4, 4, 4, 1, 100, chansum=True), R.case('bwd', 7, 64, 3, 3, 0, 0)):
        ref = R.reference(c)
        assert R.relerr(ref['ggamma'][0], ref['autograd']['ggamma']) < 1e-12
        assert R.relerr(ref['gbeta'][0], ref['autograd']['gbeta']) < 1e-12
        assert float(ref['gx_sums'].abs().max()) < 1e-9 * float(ref['gx_abs_sums'].max())       # gx sums to zero over a channel


def _pick(B):
    """csrc/vae_norm.hip pick(), restated with the integer arithmetic of the source"""
    ns = B if B < 64 else 64
    bps = (B + ns - 1) // ns
    return ns, bps, (B + bps - 1) // bps


def test_pick_and_thresholds():
    for B in range(1, 400):
        ns, bps, used = R.pick(B)
        assert (ns, bps, used) == _pick(B)
        assert used <= ns <= 64 and (used - 1) * bps < B <= used * bps              # every slab non-empty, the last one ragged or full
    assert R.pick(130) == (64, 3, 44) and R.pick(64) == (64, 1, 64) and R.pick(65) == (64, 2, 33) and R.pick(129) == (64, 3, 43)
    f = lambda op, B, C, H: R.case(op, B, C, H, H)
    for op in ('fwd', 'stats'):
        assert R.expected(f(op, 1250, 4, 4), True)[op] == 'bn_%s (one launch)' % op         # 20000 elements per channel
        assert R.expected(f(op, 1251, 4, 4), True)[op] == 'bn_%s' % op
        assert R.expected(f(op, 555, 3, 6), True)[op] == 'bn_%s (one launch)' % op          # 19980
        assert R.expected(f(op, 556, 3, 6), True)[op] == 'bn_%s' % op                       # 20016
        assert R.expected(f(op, 1250, 4, 4), False)[op] == 'bn_%s' % op
    assert R.expected(f('bwd', 128, 4, 4), True) == dict(fwd='bn_fwd (one launch)', bwd='bn_bwd (one launch)')   # 2048
    assert R.expected(f('bwd', 129, 4, 4), True) == dict(fwd='bn_fwd (one launch)', bwd='bn_bwd')
    assert R.expected(f('bwd', 128, 4, 4), False) == dict(fwd='bn_fwd', bwd='bn_bwd')
    assert R.sum_terms(f('chan_sum', 130, 3, 13), False) == -(-3 * 169 // 256) + 12
    assert R.sum_terms(f('bwd', 12, 3, 13), True) == -(-12 * 169 // 256) + 12


def test_switch_reading(monkeypatch):
    monkeypatch.delenv('GPODE_BN_ONE_LAUNCH', raising=False)
    assert R.one_launch_on()
    monkeypatch.setenv('GPODE_BN_ONE_LAUNCH', '0')
    assert not R.one_launch_on()
    monkeypatch.setenv('GPODE_BN_ONE_LAUNCH', '1')
    assert R.one_launch_on()
