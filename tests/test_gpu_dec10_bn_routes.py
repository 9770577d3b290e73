"""Every route of the decoder's fused last-stage backward, dec10::k_bwd_data_bn<IPB, MODE, WGRAD> (csrc/conv_dec10_mfma.hpp), driven
through the C ABI (gpode_dec10_bn_bwd_sums, gpode_dec10_bn_bwd_sums_wgrad, gpode_dec10_bn_bwd_apply, the two scratch sizes,
gpode_defer_reductions / gpode_flush_reductions) and once through vae_ops, against fp64 (dec10_bn_routes.py).

The batch sizes come from the device's CU count n (clamped to 256 as the library clamps it) with cap = min(2 n, 512) workgroups; the
parametrisation ids show n = 256.

 1 edges            B in {1, 2, 3, n + 1, 4 n - 1, 4 n, 4 n + 1, 4 n + 2, 4 n + 3, 4 cap + 5}, each with the plain and the _wgrad form of
                    the sums pass followed by the local apply.  IPB = 2 up to 4 n - 1 (3 and 4 n - 1 end in a one-image group), IPB = 4
                    from 4 n on; 4 n + 1 / 2 / 3 end in a group of 1 / 2 / 3 images (the partial prefetch, the f < nimg NP / 4 fill,
                    ntiles = nimg NTILE); at 4 cap + 5 workgroup 0 takes a full second group and workgroup 1 a one-image second group,
                    both with the register prefetch in flight.  With IPB = 2 the persistent loop cannot wrap on a device of at most 256
                    CUs (IPB = 2 ends at 4 n - 1 images = at most cap groups), so there is no such case and none is faked.
 2 attribution      gy zero except in image b* of {0, 4 cap - 1, 4 cap, B - 1} at 4 cap + 5 and of {0, 4 n - 1, 4 n, B - 1} at 4 n + 3,
                    c dense: gw, gbias and sums must be those of that image alone, relative to the one-image result -- a dropped,
                    doubled or stale-plane image is the whole error.
 3 simulated ranks  shards (3, 1, 2), (n + 1, 1, 2 n + 1), (4 n + 2, 1, 3, 7) -- IPB = 4 and IPB = 2 ranks mixed -- and 16 unequal ranks of
                    1 .. 4 images: gc per shard against the whole-batch reference under the data-parallel loss weighting, ggamma / gbeta
                    the shard's own sums; one rank with `gathered` is bit-identical to sums_gathered == NULL.
 4 optional         sums == NULL, gbias == NULL, gc_chansum == NULL: the other outputs bit-identical to the full call, and the scratch
                    region of the absent output (part_b, part_gx) still holds the NaN fill.
 5 deferred         the _wgrad sums pass and the apply between gpode_defer_reductions(1) and (0): gw, gbias, gc_chansum NaN until
                    gpode_flush_reductions, then the bits of the immediate form.
 6 refusals         c / gy / gc one float off 16-byte alignment, wscratch NULL, gathered sums without weights or with nranks 0, B = 0,
                    every required pointer NULL: non-zero, a message naming the cause, nothing written, no launch.
 7 vae_ops          bn_relu_conv_transpose2d on the last-stage geometry at 4 n + 3 against torch.autograd in fp64, every gradient, with
                    an aligned c (the fused route, the weight gradient riding: asserted) and a c one float off (the separate ops).

Per case (dec10_bn_routes.launch / check): gpode_last_launch() after every call (dec10_bn_bwd_sums, dec10_bn_bwd_sums_wgrad,
dec10_bn_bwd_apply: which instantiation ran); gc, ggamma, gbeta, sums within bn_routes.TOL = 2e-5 and gw, gbias within 5
conv_dispatch.TOL = 1e-4 of fp64, in the max norm relative to the reference's largest entry, per shard; every output and both scratches
NaN-filled, the scratches exactly the advertised sizes, guard floats behind every buffer (behind c and gc three images' worth, so a
ragged group taken for a full one stays inside the buffers and is reported); the number of floats written per scratch region equals
what (ipb, nwg) of dec10_bn_routes.expected() implies -- part nwg * 32, part_gx nwg * 32, part_w nwg * 400, part_b nwg -- and they
form a prefix; a second run gives the same bits.

gc_chansum cancels to about zero over the batch, so the fp64 channel sum is no yardstick: it is compared with the fp64 sum of the
kernel's own gc within 2^-24 terms sum |gc| (bn_routes.check.cmp_chansum).  terms follows this kernel's summation order: a lane adds
the four pixels of each of its ceil(49 ipb / 8) tiles per group over the ceil(groups / nwg) groups of its workgroup into one register,
one thread adds the 32 rows of s_red in order, and k_reduce_multi adds the nwg partials as 16 interleaved chains of ceil(nwg / 16) and
then those 16: terms = 4 ceil(49 ipb / 8) ceil(groups / nwg) + 32 + ceil(nwg / 16) + 16 (280 at 4 cap + 5 on 256 CUs).

GPODE_CONV_VALU=1 is no mode of this stage (the fused entry points ignore it, and gpode_conv2d_bwd_weight_bn, the unfused twin of the
riding weight gradient, is refused on the decoder layers under it), so there is no VALU form here.

The inputs have no ReLU coin-flips (bn_routes._inputs: every pre-activation at least 1e-4 from zero; 5.0e-4 at the least over the
draws used at 256 CUs), and save_mean / save_invstd are the fp64 statistics rounded to fp32, the same values the reference uses.

Measured on an MI355X (256 CUs), largest error over all cases (bound): gc 2.8e-7, ggamma / gbeta 4.7e-7 and 2.1e-6 with simulated ranks,
sums 3.8e-7 and 2.1e-6 (2e-5); gw 4.4e-7 and 7.6e-7, gbias 3.4e-6 and 1.7e-5 on shards of one to four images, where sum gy cancels (1e-4);
one image alone: sums 3.2e-7, gw 2.8e-7, gbias 4.7e-7; gc_chansum 0.031 of its summation bound; through vae_ops gc 2.1e-7, ggamma
2.6e-7, gbeta 2.8e-7, gw 4.2e-7, gbias 1.6e-6, the same on both routes.  No NaN of the fills reached an output, no guard was written,
every scratch extent was the expected prefix; the module takes 30 s, its slowest case (4 cap + 5 with its draw and reference) 5 s.

Each of these, built into the library once, turned red what it should: `nimg = IPB` in the group loop of k_bwd_data_bn (a ragged group
taken for a full one) -- every edge case with a ragged group, 1, 3, n + 1, 4 n - 1, 4 n + 1 / 2 / 3 and 4 cap + 5 in both forms (2 and 4 n
pass), the attribution cases at 4 n + 3 whose image lies in the ragged group (b* = 4 n and B - 1; at 4 cap + 5 the planes the one-image
group inherits hold the zeros of gy, so that size is caught by item 1), every case of items 3 to 5 and the aligned run of item 7: 33
of 86; the rank weights read as 1 in the gathered branch -- the four cases of simulated ranks with unequal shares and nothing else."""
import functools

import pytest
import torch

import bn_routes as R
import conv_dispatch as D
import dec10_bn_routes as T

pytestmark = pytest.mark.gpu
N0 = 256                                            # the CU count the ids are written for
MAXIMA = {}


def _n():
    return min(torch.cuda.get_device_properties(0).multi_processor_count, T.MAX_CUS)


@functools.lru_cache(maxsize=None)
def _full(B):
    """the full call (the _wgrad form with every optional output, local statistics) at B images"""
    return T.launch(T.case(B))


@pytest.fixture(scope='module', autouse=True)
def _drop_cached_results():
    yield
    print('largest error per group:', {k: '%.1e' % v for k, v in sorted(MAXIMA.items())})
    for f in (_full, T._reference, T.autograd_reference, T.pre_min, T._inputs, R._inputs):
        f.cache_clear()


def _param(make, ident=T.case_id):
    cases = make(N0)
    assert len(set(map(ident, cases))) == len(cases)
    return pytest.mark.parametrize('i', range(len(cases)), ids=[ident(c) for c in cases])


def _lib():
    from vae_gp_ode_amd import _lib
    return _lib.load()


# ---- item 1: edges against fp64 ------------------------------------------------------------------------------------------------------
@_param(T.edge_cases)
def test_edges(i):
    n = _n()
    c = T.edge_cases(n)[i]
    T.check(c, T.launch(c), n, MAXIMA)


def test_scratch_sizes_are_the_documented_layouts():
    """part[512][16][2] | part_gx[512][16][2], and part_w[512][400] | part_b[512]"""
    assert T.scratch_floats() == (2 * T.MAX_WG * T.C * 2, T.MAX_WG * T.C * T.KK + T.MAX_WG)


# ---- item 2: image attribution -------------------------------------------------------------------------------------------------------
@_param(T.attribution_cases, lambda a: 'B%d-image%d' % a)
def test_one_image_is_attributed_once(i):
    n = _n()
    B, b = T.attribution_cases(n)[i]
    c = T.case(B)
    T.check(c, T.launch(c, only=b, apply=False), n, MAXIMA, only=b, apply=False)


# ---- item 3: simulated ranks ---------------------------------------------------------------------------------------------------------
@_param(T.shard_cases)
def test_simulated_ranks(i):
    n = _n()
    c = T.shard_cases(n)[i]
    T.check(c, T.launch(c), n, MAXIMA)


@pytest.mark.parametrize('i', range(len(T.one_rank_sizes(N0))), ids=['B%d' % B for B in T.one_rank_sizes(N0)])
def test_one_gathered_rank_gives_the_bits_of_the_local_form(i):
    """weights = {1}, count_all = 784 B, gathered = the rank's own sums[32]: fmaf(1, s, 0) = s and the same count"""
    n = _n()
    B = T.one_rank_sizes(n)[i]
    c = T.case(B, shards=(B,))
    got = T.launch(c)
    T.check(c, got, n, MAXIMA)
    assert not T.same_bits(got, _full(B), list(got['out'])) and set(got['out']) == set(_full(B)['out'])


# ---- item 4: optional arguments ------------------------------------------------------------------------------------------------------
@_param(T.optional_cases)
def test_optional_outputs(i):
    """check() holds the scratch extents: part_b (gbias NULL) and part_gx (gc_chansum NULL) keep their NaN fill"""
    n = _n()
    c = T.optional_cases(n)[i]
    got, full = T.launch(c), _full(c.B)
    T.check(c, got, n, MAXIMA)
    missing = set(full['out']) - set(got['out'])
    assert missing == {'sums' if not c.sums else 'gbias' if not c.gbias else 'gc_chansum'}, missing
    assert not T.same_bits(got, full, list(got['out']))


# ---- item 5: deferred reductions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(T.optional_sizes(N0))), ids=['B%d' % B for B in T.optional_sizes(N0)])
def test_deferred_reductions_give_the_bits_of_the_immediate_form(i):
    """launch(deferred=True) reports a reduction that ran before the flush (gw, gbias, gc_chansum must still hold the NaN fill then)"""
    n = _n()
    c = T.case(T.optional_sizes(n)[i])
    got = T.launch(c, deferred=True)
    T.check(c, got, n, MAXIMA)
    assert not T.same_bits(got, _full(c.B), list(got['out']))
    o = torch.full((T.C,), float('nan'), device='cuda')                            # nothing is left behind: a call is eager again
    v = torch.ones(2, T.C, 4, device='cuda')
    lib = _lib()
    assert lib.gpode_chan_sum(R._ptr(v), R._ptr(o), 2, T.C, 4, R._ptr(torch.empty(int(lib.gpode_bn_scratch(2, T.C)), device='cuda')), R._stream()) == 0
    torch.cuda.synchronize()
    assert bool((o == 8).all()) and lib.gpode_flush_reductions(R._stream()) == 0


# ---- item 6: refusals ----------------------------------------------------------------------------------------------------------------
HEAD = ('c', 'gy', 'w', 'gamma', 'beta', 'mean', 'invstd')
SUMS, WGRAD, APPLY = 'gpode_dec10_bn_bwd_sums', 'gpode_dec10_bn_bwd_sums_wgrad', 'gpode_dec10_bn_bwd_apply'
ORDER = {SUMS: HEAD + ('sums', 'B', 'scratch'), WGRAD: HEAD + ('sums', 'gw', 'gbias', 'B', 'scratch', 'wscratch'),
         APPLY: HEAD + ('gathered', 'weights', 'nranks', 'count_all', 'gc', 'ggamma', 'gbeta', 'gc_chansum', 'B', 'scratch')}
REQUIRED = {SUMS: HEAD + ('scratch',), WGRAD: HEAD + ('scratch', 'gw', 'wscratch'), APPLY: HEAD + ('gc', 'ggamma', 'gbeta', 'scratch')}
REFUSALS = ([(e, 'shift', k, '16-byte aligned') for e in (SUMS, WGRAD) for k in ('c', 'gy')]
            + [(APPLY, 'shift', k, '16-byte aligned') for k in ('c', 'gy', 'gc')]
            + [(APPLY, 'gathered', 'weights', 'weights'), (APPLY, 'gathered', 'nranks', 'weights')]
            + [(e, 'zero', 'B', 'B >= 1') for e in (SUMS, WGRAD, APPLY)]
            + [(e, 'null', k, 'null pointer') for e in (SUMS, WGRAD, APPLY) for k in REQUIRED[e]])


@pytest.mark.parametrize('entry,kind,what,names', REFUSALS, ids=['%s-%s-%s' % (e[len('gpode_dec10_bn_bwd_'):], k, w) for e, k, w, _ in REFUSALS])
def test_refusals(entry, kind, what, names):
    """non-zero, the message names the entry point and the cause, every output and scratch still NaN, every guard intact, and
    gpode_last_launch() still names the launch made before"""
    lib, B = _lib(), 3
    d = T.device_inputs(T.case(B))
    b = T.Buffers()
    SCR, WSCR = T.scratch_floats()
    a = dict(d, B=B, nranks=0, count_all=0.0, gathered=None, weights=None, scratch=b.new('scratch', SCR), wscratch=b.new('wscratch', WSCR),
             sums=b.new('sums', 2 * T.C), gw=b.new('gw', T.C * T.KK), gbias=b.new('gbias', 1), gc=b.new('gc', B * T.C * T.HW + 1),
             ggamma=b.new('ggamma', T.C), gbeta=b.new('gbeta', T.C), gc_chansum=b.new('gc_chansum', T.C))
    if kind == 'shift':
        a[what] = a['gc'][1:] if what == 'gc' else D._dev(d[what], shift=True)
        assert a[what].data_ptr() % 16 == 4
    elif kind == 'null':
        a[what] = None
    elif kind == 'zero':
        a[what] = 0
    else:
        a.update(gathered=torch.ones(1, 2 * T.C, device='cuda'), nranks=1, count_all=float(B * T.HW), weights=torch.ones(1, device='cuda'))
        a[what] = None if what == 'weights' else 0
    o, v = torch.empty(T.C, device='cuda'), torch.ones(2, T.C, 4, device='cuda')
    assert lib.gpode_chan_sum(R._ptr(v), R._ptr(o), 2, T.C, 4, R._ptr(torch.empty(int(lib.gpode_bn_scratch(2, T.C)), device='cuda')), R._stream()) == 0
    before = lib.gpode_last_launch().decode()
    assert before == 'chan_sum'
    args = [a[k] if k in ('B', 'nranks', 'count_all') else R._ptr(a[k]) for k in ORDER[entry]]
    rc = getattr(lib, entry)(*args, R._stream())
    msg = lib.gpode_last_error().decode()
    print('%s %s %s: rc %d, "%s"' % (entry, kind, what, rc, msg))
    assert rc != 0, 'served'
    assert entry in msg and names in msg, msg
    assert lib.gpode_last_launch().decode() == before
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in b.outs.values()), [k for k, t in b.outs.items() if not bool(torch.isnan(t).all())]
    assert not [p for p in b.problems() if 'guard' in p]


# ---- item 7: through vae_ops -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [False, True], ids=['aligned', 'one-float-off'])
def test_last_stage_through_vae_ops(shift, monkeypatch):
    """bn_relu_conv_transpose2d(c, BatchNorm2d(16), decnn.10's weight and bias) forward and backward at 4 n + 3 images against
    torch.autograd in fp64 (statistics of its own).  Aligned c: _BnReluConvT, whose backward calls _dec10_bn_bwd once with the weight
    gradient riding.  c one float off 16-byte alignment (a contiguous view into a buffer one float larger): the wrapper takes the
    separate ops on a copy -- _BnReluConvT, whose fused kernels need the alignment from the forward on, never sees it, so its backward
    cannot reach gpode_dec10_bn_bwd_sums with such a c -- and the gradients are the same."""
    from vae_gp_ode_amd import vae_ops as V
    n = _n()
    B = 4 * n + 3
    d, ref = T._inputs(B, ()), T.autograd_reference(B)
    bn = torch.nn.BatchNorm2d(T.C).cuda()
    with torch.no_grad():
        bn.weight.copy_(d['gamma']); bn.bias.copy_(d['beta'])
    a = [D._dev(d['c'].reshape(B, T.C, T.H, T.H), shift).requires_grad_(True), d['w'].cuda().requires_grad_(True), d['bias'].cuda().requires_grad_(True)]
    assert a[0].is_contiguous() and a[0].data_ptr() % 16 == (4 if shift else 0)
    calls, fused = [], V._dec10_bn_bwd
    monkeypatch.setattr(V, '_dec10_bn_bwd', lambda *p, **k: (calls.append(k.get('gw') is not None), fused(*p, **k))[1])
    y = V.bn_relu_conv_transpose2d(a[0], bn, a[1], a[2], 1, 2)
    y.backward(d['gy'].cuda())
    torch.cuda.synchronize()
    errs = dict(y=(R.relerr(y, ref['y']), D.TOL), gc=(R.relerr(a[0].grad, ref['gc']), T.TOL), ggamma=(R.relerr(bn.weight.grad, ref['ggamma']), T.TOL),
                gbeta=(R.relerr(bn.bias.grad, ref['gbeta']), T.TOL), gw=(R.relerr(a[1].grad, ref['gw']), T.TOL_W),
                gbias=(R.relerr(a[2].grad, ref['gbias']), T.TOL_W))
    print('vae_ops %s: fused calls %s, %s' % ('one float off' if shift else 'aligned', calls, {k: '%.1e' % e for k, (e, _) in errs.items()}))
    for k, (e, _) in errs.items():
        MAXIMA['vae_ops ' + k] = max(MAXIMA.get('vae_ops ' + k, 0.0), e)
    assert calls == ([] if shift else [True]), calls
    assert all(e < tol for e, tol in errs.values()), errs
