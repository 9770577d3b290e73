"""CPU tests of the fused last-decoder-stage helper (dec10_bn_routes.py) itself: expected() against (ipb, nwg) tabulated by hand for 256
and 64 CUs, the closed-form fp64 reference against torch.autograd on the whole stage, the input condition (no pre-activation within
bn_routes.MIN_PRE of zero) for every draw the GPU file needs at 256 CUs, and the case tables against the list of edges they exist for."""
import pytest
import torch

import bn_routes as R
import dec10_bn_routes as T


@pytest.fixture(scope='module', autouse=True)
def _drop_cached_results():
    yield
    for f in (T._reference, T.autograd_reference, T.pre_min, T._inputs, R._inputs):
        f.cache_clear()


def test_dispatch_restated_against_a_table_made_by_hand():
    """ipb = B >= 4 n ? 4 : 2; nwg = min(ceil(B / ipb), min(2 n, 512)); n clamped to 256"""
    n256 = {1: (2, 1), 2: (2, 1), 3: (2, 2), 257: (2, 129), 1022: (2, 511), 1023: (2, 512), 1024: (4, 256), 1025: (4, 257), 1026: (4, 257),
            1027: (4, 257), 1028: (4, 257), 1029: (4, 258), 2047: (4, 512), 2048: (4, 512), 2053: (4, 512), 8192: (4, 512)}
    n64 = {1: (2, 1), 65: (2, 33), 255: (2, 128), 256: (4, 64), 257: (4, 65), 259: (4, 65), 512: (4, 128), 513: (4, 128), 517: (4, 128)}
    for B, want in n256.items():
        assert T.expected(B, 256) == want, (B, T.expected(B, 256), want)
        assert T.expected(B, 304) == want, B           # a device with more CUs: num_cus() clamps
    for B, want in n64.items():
        assert T.expected(B, 64) == want, (B, T.expected(B, 64), want)
    assert T.cap(256) == 512 and T.cap(64) == 128 and T.cap(1000) == 512
    assert T.edge_sizes(256) == (1, 2, 3, 257, 1023, 1024, 1025, 1026, 1027, 2053)
    assert T.edge_sizes(64) == (1, 2, 3, 65, 255, 256, 257, 258, 259, 517)
    # 4 * ceil(49 ipb / 8) * rounds + 32 + ceil(nwg / 16) + 16
    assert T.chansum_terms(2053, 256) == 4 * 25 * 2 + 32 + 32 + 16
    assert T.chansum_terms(1027, 256) == 4 * 25 * 1 + 32 + 17 + 16
    assert T.chansum_terms(3, 256) == 4 * 13 * 1 + 32 + 1 + 16


def test_case_tables_contain_the_edges_they_exist_for():
    for n in (256, 64):
        c = T.cap(n)
        sizes = T.edge_sizes(n)
        groups = lambda B: -(-B // T.expected(B, n)[0])
        last = lambda B: B - (groups(B) - 1) * T.expected(B, n)[0]                         # images in the last group
        assert any(T.expected(B, n)[0] == 2 and last(B) == 1 and groups(B) > 1 for B in sizes)          # IPB = 2, ragged
        assert 4 * n - 1 in sizes and T.expected(4 * n - 1, n) == (2, c) and last(4 * n - 1) == 1      # ... at the last IPB = 2 size
        assert T.expected(4 * n, n)[0] == 4 and last(4 * n) == 4
        assert {last(B) for B in sizes if T.expected(B, n)[0] == 4 and groups(B) <= c} == {1, 2, 3, 4}  # IPB = 4, nimg 1, 2, 3 (and full)
        big = max(sizes)                                 # the wrap: workgroup 0 a full second group, workgroup 1 a one-image second group
        assert T.expected(big, n) == (4, c) and groups(big) == c + 2 and last(big) == 1
        # with IPB = 2 the loop wraps only past 2 cap images, and IPB = 2 ends at 4 n - 1 <= 2 cap - 1 on a device of at most 256 CUs
        assert all(groups(B) <= c for B in range(1, 4 * n))
        assert any({T.expected(nr, n)[0] for nr in s} == {2, 4} for s in T.shard_sets(n))              # a mixed-IPB shard set
        assert any(len(s) == 16 and len(set(s)) > 1 for s in T.shard_sets(n))
        for B, b in T.attribution_cases(n):
            assert 0 <= b < B
        assert {b for B, b in T.attribution_cases(n) if B == big} == {0, 4 * c - 1, 4 * c, big - 1}
        for cases in (T.edge_cases(n), T.shard_cases(n), T.optional_cases(n)):
            assert len(set(cases)) == len(cases) and len(set(map(T.case_id, cases))) == len(cases)
        assert all(not k.sums or not k.gbias or not k.chansum for k in T.optional_cases(n))
        assert {(k.wgrad, k.B) for k in T.edge_cases(n)} == {(w, B) for w in (False, True) for B in sizes}
    assert T.shard_sets(256)[2] == (1026, 1, 3, 7)


@pytest.mark.parametrize('shards', [(), (3, 1, 2)], ids=['one-rank-B5', 'shards-3.1.2'])
def test_closed_form_reference_is_autograd_on_the_whole_stage(shards):
    """conv_transpose2d(relu(batch_norm(c)), w, bias, padding 2) under the share-weighted loss, torch.autograd in fp64, against the
    closed form evaluated with the same (exact) statistics: gc per shard, and ggamma, gbeta, gw, gbias as the share-weighted sums of the
    shards' own"""
    B = sum(shards) or 5
    d = T._inputs(B, shards)
    auto, fold = T.autograd_reference(B, shards, by_fold=False), T.autograd_reference(B, shards)
    for k in ('y', 'gc', 'ggamma', 'gbeta', 'gw', 'gbias'):    # the col2im form the GPU file uses at a thousand images: the same function
        assert R.relerr(fold[k], auto[k]) < 1e-12, k
    ref =T.closed_form(B, shards, d['mean64'], d['invstd64'])
    sh = shards or (B,)
    share = torch.tensor(sh, dtype=torch.float64) / B
    errs = {'gc[%d]' % r: R.relerr(ref['gc'][sl], auto['gc'][sl]) for r, (sl, _) in enumerate(R._slices(sh))}
    for k in ('ggamma', 'gbeta', 'gw', 'gbias'):
        errs[k] = R.relerr(share @ ref[k], auto[k])
    print(errs)
    assert max(errs.values()) < 1e-10, errs
    assert float(d['bias'].abs()) > 0.05
    # the sums a rank exchanges are its {sum g, sum g xhat}, interleaved per channel
    assert torch.equal(ref['sums'][:, 0::2], ref['gbeta']) and torch.equal(ref['sums'][:, 1::2], ref['ggamma'])
    # gc sums to zero over a channel of the whole batch under that loss
    whole = sum(s * ref['gc'][sl].sum((0, 2)) for s, (sl, _) in zip(share, R._slices(sh)))
    assert float(whole.abs().max()) < 1e-9 * float(ref['gc_abs_sums'].max())


def test_one_image_reference_is_the_reference_of_a_batch_with_one_nonzero_image():
    """reference(only=b) takes a shortcut (it evaluates image b alone with the batch's statistics): the same as zeroing gy elsewhere"""
    B, b = 5, 3
    d = T._inputs(B, ())
    one = T.closed_form(B, (), d['mean'].double(), d['invstd'].double(), only=b)
    gy = torch.zeros_like(d['gy'])
    gy[b] = d['gy'][b]
    full = T.closed_form(B, (), d['mean'].double(), d['invstd'].double(), gy=gy)
    for k in ('sums', 'gw', 'gbias', 'ggamma', 'gbeta'):
        assert R.relerr(one[k], full[k]) < 1e-12, k


def test_inputs_keep_every_preactivation_away_from_zero():
    """for every draw of the GPU file's tables at 256 CUs, with the fp32 statistics the kernels are given (reference() asserts it too)"""
    lo = {}
    for B, shards in T.input_keys(256):
        lo[(B, shards)] = T.pre_min(B, shards)
        assert lo[(B, shards)] >= R.MIN_PRE, (B, shards, lo[(B, shards)])
        d = T._inputs(B, shards)
        assert d['c'].dtype == d['gy'].dtype == d['mean'].dtype == torch.float32 and d['gy'].shape == (B, 1, 28, 28)
        if B >= 100:                                     # both sides of the ReLU are populated in every channel
            frac = (T._pre(d, d['mean'].double(), d['invstd'].double()) > 0).double().mean((0, 2))
            assert (frac > 0.02).all() and (frac < 0.98).all(), (B, shards, frac)
    print('smallest |pre-activation|:', {k: '%.1e' % v for k, v in lo.items()})
