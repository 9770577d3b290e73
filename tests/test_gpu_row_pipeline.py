"""The kernels that request their operands ahead of the row loops (csrc/gp_backward.hip: the DF parameter-sum kernels load row r + 1
before the arithmetic of row r; csrc/vae_dense.hip: k_linear_bwd_w_cols loads a tile's gy and x before its first FMA), at the places
where a look-ahead can go wrong; the same checks on the RBF parameter sums and the reverse sweep, whose loops are the plain ones.

(a) Chunk additivity.  A chunk's rows go to that chunk's slab and to no other, and reduce_slab adds the used slabs to zeros, so
    param_grad of 2 R rows in two chunks equals, bit for bit, the fp32 sum of two calls on R rows in one chunk each -- unless a row is
    carried across the chunk boundary (a look-ahead that reads, and uses, the first row of the next chunk).  Split DF route at 2 x 1024
    rows and two draws; unsplit DF and RBF routes at 2 x 60 rows.  Compared on the live entries of the pack layout: nobody writes
    its pad.
(b) Edge chunkings of the split route against the fp64 oracle with integrator_routes' bound for param_grad: one row per chunk (nothing
    to look ahead to) and a ragged last chunk (1030 rows in 4 chunks of 258: the last has 256).
(c) The reverse sweep of five trajectories equals, bit for bit, the same five swept one per call, and is within integrator_routes' bound
    of the oracle: T = 2 (one step) and T = 3, rk4 and Euler, DF D = 6 and RBF q = 6.
(d) The fc layer's weight sums on the row-slab route against fp64 with the bound of the dense-layer route test (loss_routes.TOL of the
    largest entry): B = 1024, In = 6, Out = 64, and B = 1027, In = 8, Out = 128 (slabs of 33 rows, the last of 4)."""
import functools

import pytest
import torch

import integrator_routes as IR
import loss_routes as LR

pytestmark = pytest.mark.gpu


def _tag():
    from vae_gp_ode_amd import _lib
    return _lib.load().gpode_last_launch().decode()


def _dev_inputs(c):
    p, nz, z0, ts, gw = IR.inputs(c)
    return ({k: v.cuda() for k, v in p.items()}, {k: v.cuda() for k, v in nz.items()}, z0.cuda(), ts.cuda(), gw.cuda())


@functools.lru_cache(maxsize=2)
def _cache(c):
    dev_in = _dev_inputs(c)
    k = IR.build(c, dev_in)
    return k, IR.cache_dicts(c, k, dev_in)


def _rows(c, R, seed):
    g = torch.Generator().manual_seed(seed)
    lead = (c.nd,) if c.nd > 1 else ()
    return torch.randn(*lead, R, c.Di, generator=g), torch.randn(*lead, R, c.Do, generator=g)


def _live(c, gpack):
    """the entries of a pack-layout gradient ([L,] pack_floats) that belong to a record field or to the uniform tail: the pad lanes
    of the last lane groups and the pad behind the tail are never written by anyone"""
    from pack_layout import PackView
    pv = PackView(c.kernel, c.Di, c.Do, c.M, c.S)
    return torch.cat([torch.cat([v(g).reshape(-1) for v in (pv.rff, pv.ind, pv.uni)]) for g in gpack.reshape(-1, gpack.shape[-1])])


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
ADDITIVE = [(IR.D_(6, 100, 256, 1, 'euler', T=2, nd=2), 1024, 'param_grad_df_split'),
            (IR.D_(6, 16, 32, 1, 'euler', T=2), 60, 'param_grad_df'),
            (IR.R_(6, 6, 1, 16, 32, 1, 'euler', T=2), 60, 'param_grad_rbf')]


@pytest.mark.parametrize('c,R,tag', ADDITIVE, ids=[t[2] for t in ADDITIVE])
def test_two_chunks_equal_the_sum_of_two_calls(c, R, tag):
    from vae_gp_ode_amd import ops
    k, _ = _cache(c)
    x, a = (t.cuda() for t in _rows(c, 2 * R, 31))
    both = ops.param_grad(k, x, a, nchunk=2)
    assert _tag() == tag, _tag()
    lo = ops.param_grad(k, x[..., :R, :].contiguous(), a[..., :R, :].contiguous(), nchunk=1)
    assert _tag() == tag, _tag()
    hi = ops.param_grad(k, x[..., R:, :].contiguous(), a[..., R:, :].contiguous(), nchunk=1)
    torch.cuda.synchronize()
    both, lo, want = _live(c, both), _live(c, lo), _live(c, lo + hi)
    assert not torch.isnan(both).any() and not torch.isnan(want).any()
    print('%s: %d of %d entries differ from the sum of the two halves' % (tag, (both != want).sum().item(), both.numel()))
    assert torch.equal(both, want)
    assert not torch.equal(both, lo)                 # the second chunk was there


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
SPLIT = IR.D_(6, 100, 256, 1, 'euler', T=2)


@pytest.mark.parametrize('R,nchunk', [(1024, 1024), (1030, 4)], ids=['one-row-chunks', 'ragged-last-chunk'])
def test_split_route_edge_chunkings_against_the_oracle(R, nchunk):
    from vae_gp_ode_amd import ops
    c = SPLIT
    k, cache = _cache(c)
    x, a = _rows(c, R, 57)
    gpack = ops.param_grad(k, x.cuda(), a.cuda(), nchunk=nchunk)
    assert _tag() == 'param_grad_df_split', _tag()
    torch.cuda.synchronize()
    (_, r64), (_, r32) = (IR.reference_rows(c, cache, dt, x[None], a[None]) for dt in (torch.float64, torch.float32))
    got = IR.unpack(c, gpack.cpu()[None], cache)
    IR.compare(c, got, r64, r32, [kk for kk in IR.OUT_LEAF if kk in r64], 'param_grad, %d rows in %d chunks: ' % (R, nchunk))


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
SWEEP = [IR.D_(6, 100, 256, 5, m, T=T) for m in ('rk4', 'euler') for T in (2, 3)] + \
        [IR.R_(6, 6, 1, 100, 256, 5, m, T=T) for m in ('rk4', 'euler') for T in (2, 3)]


@pytest.mark.parametrize('c', SWEEP, ids=IR.case_id)
def test_reverse_sweep_batch_equals_one_trajectory_per_call(c):
    from vae_gp_ode_amd import ops
    dev_in = _dev_inputs(c)
    z0, ts, gw = dev_in[2:]
    k = IR.build(c, dev_in)
    zt, xs = ops.rollout(k, z0, ts, c.order, c.method, save_stages=True)
    gz0, ast = ops.rollout_bwd(k, xs, gw[0], ts, c.order, c.method)
    tag = _tag()
    assert tag == IR.expected(c)['rollout_bwd'], tag   # the register-resident team
    for n in range(c.N):
        g1, a1 = ops.rollout_bwd(k, xs[n:n + 1].contiguous(), gw[0, n:n + 1].contiguous(), ts, c.order, c.method)
        assert _tag() == tag, (_tag(), tag)
        assert torch.equal(g1[0], gz0[n]) and torch.equal(a1[0], ast[n]), (IR.case_id(c), n)
    torch.cuda.synchronize()
    cache = IR.cache_dicts(c, k, dev_in)
    r64, r32 = IR.reference(c, cache, torch.float64), IR.reference(c, cache, torch.float32)
    IR.compare(c, dict(gz0=gz0.cpu()[None], astage=ast.cpu()[None]), r64, r32, ('gz0', 'astage'), 'sweep: ')


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,In,Out', [(1024, 6, 64), (1027, 8, 128)])
def test_fc_weight_sums_on_the_row_slab_route(B, In, Out):
    from vae_gp_ode_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(B + In + Out)
    x, gy, w = torch.randn(B, In, generator=g), torch.randn(B, Out, generator=g), torch.randn(Out, In, generator=g)
    xd, gyd, wd = x.cuda(), gy.cuda(), w.cuda()
    gx, gw, gb = (torch.full(s, float('nan'), device='cuda') for s in ((B, In), (Out, In), (Out,)))
    scratch = torch.full((lib.gpode_linear_bwd_scratch(B, In, Out),), float('nan'), device='cuda')
    tags = {}
    LR._call(tags, 'bwd', 'gpode_linear_bwd', xd, wd, gyd, gx, gw, gb, B, In, Out, scratch)
    torch.cuda.synchronize()
    assert tags['bwd'] == 'linear_bwd_fanout (row slabs)', tags
    want_w, want_b = gy.double().t() @ x.double(), gy.double().sum(0)
    for name, got, want in (('gw', gw, want_w), ('gb', gb, want_b)):
        err = ((got.double().cpu() - want).abs().max() / want.abs().max()).item()
        print('B %d In %d Out %d %s: %.2e (bound %.1e)' % (B, In, Out, name, err, LR.TOL))
        assert err <= LR.TOL, (name, err)
