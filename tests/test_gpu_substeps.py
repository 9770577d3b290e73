"""GPU: sub-steps of the fixed-grid solvers -- gpode_rollout_fwd_ns / gpode_rollout_bwd_ns / gpode_rollout_bwd_pgrad_ns, their routing
through ops.rollout / ops.flow / Flow(substeps=), and --ts_dense_scale on top of them.

s steps inside every output interval are one step per interval of the refined grid substeps_ref.refine(ts, s), every s-th frame kept.

What is held to what:
  1 BITS, on every forward route of integrator_routes.TABLE and both reverse routes, s in {2, 4}, T = 4, on three grids whose refined
    entries are small multiples of 2^-7 (uniform, non-uniform, one row per trajectory), so that h = (ts[t+1] - ts[t]) / s is exact and
    equals the refined grid's own differences: `_ns`(ts, s) against `_nt`(refine(ts, s)) -- zt against every s-th refined frame, xstage
    against the refined record reshaped, and with dL/dzt scattered into every s-th refined frame gz0 and astage; gpack on the fused
    cases.  It is the same kernel on the same rows in the same order: torch.equal, nothing weaker.  Also the three solvers, order 2,
    two draws, z0 per draw.  Every output sits in a NaN-filled buffer with a NaN guard behind it; a second run gives the same bits.
    s = 1 is the twin: every output and the tag gpode_last_launch() returns.  A count outside 1 ... 64 and dopri5: refused by name,
    nothing written.
    The rollout kernels have a one-step and a sub-step instantiation.  The checks of 1 and 2 run with gpode_test_substep_kernels(1),
    the door for tests that serves the refined-grid launch from the sub-step instantiation too: then it is literally one kernel on the
    same rows in the same order, and the bound is torch.equal.  Each case also runs with the door shut, the sub-step instantiation
    against the one-step one: two separately compiled kernels, which differed by one unit in the last place in 3 of 240 states on one
    model -- held to twice the project's fp64 floors (RAW_BOUND, FLOW_BOUND below), differences printed.
  2 BITS at the level of ops.flow / Flow: Flow(substeps=s)(z0, ts) against Flow()(z0, refine(ts, s))[:, ::s] with the generator put back
    in between; dL/dz0 and the five GP parameter gradients likewise.
  3 the fp64 oracle on the refined grid, the project's bound integrator_routes.compare (FLOOR + 3 x the fp32 oracle's own error), on
    the non-uniform TS[3] = (0, 0.05, 0.2) with s = 3, which is NOT exact in float32: zt, xstage, gz0, astage and the leaf gradients.
  4 what it is for: on 0.25 arange(6) Euler at s = 8 is at least four times, midpoint at s = 4 at least eight times nearer to the fp64
    oracle's rk4 with 64 sub-steps than at s = 1 (first order predicts 8, second 16; the fp64 oracle alone gives 6.8 ... 8.3 and
    16.4 ... 17.5 on these models, with the smaller errors, 2.7e-3 and 4.1e-5 at the least, far above the float32 floor).
  5 the layers above: main.py --ts_dense_scale 3 eagerly and replayed, a captured step with Flow(substeps=2) against eager steps to BITS,
    evaluate --ts_dense_scale 3, compute_loss(compact=True) on a substeps = 2 model."""
import copy
import glob
import math

import pytest
import torch

import integrator_routes as IR
from substeps_ref import T_EXACT, exact_grids, refine, scatter_frames
from test_gpu_time_grids import route_cases, tiny_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def leave_the_global_generators_as_found():
    """as test_gpu_time_grids.py: the model tests here seed and draw from the process-wide generators; later files must not see that"""
    import random
    import numpy as np
    saved = (torch.get_rng_state(), torch.cuda.get_rng_state_all(), np.random.get_state(), random.getstate())
    yield
    torch.set_rng_state(saved[0])
    torch.cuda.set_rng_state_all(saved[1])
    np.random.set_state(saved[2])
    random.setstate(saved[3])


def _lib_():
    from vae_gp_ode_amd import _lib
    return _lib.load()


def _tag():
    return _lib_().gpode_last_launch().decode()


def _err():
    return _lib_().gpode_last_error().decode()


class Bufs:
    """outputs of one launch: NaN-filled, integrator_routes.GUARD NaN floats behind each"""

    def __init__(self):
        self.t, self.g = {}, {}

    def new(self, name, *shape):
        self.t[name], self.g[name] = IR._guarded(*shape)
        return self.t[name]

    def guards_changed(self):
        torch.cuda.synchronize()
        return [k for k, g in self.g.items() if not torch.isnan(g).all()]

    def untouched(self):
        torch.cuda.synchronize()
        return all(torch.isnan(t).all().item() for t in self.t.values()) and not self.guards_changed()


def _head(cb, nd, order, method):
    from vae_gp_ode_amd.ops import KERNEL_ID, METHOD_ID
    return (KERNEL_ID[cb.kernel], order, METHOD_ID[method] if isinstance(method, str) else method, cb.Di, cb.Do, cb.M, cb.S, nd)


def _rows(s):
    """the sub-step axis of a record buffer; a count the library must refuse still gets a buffer, which has to stay as it is"""
    return 1 if s is None else min(max(s, 1), 64)


def fwd(cb, nd, z0, ts, order, method, s=None):
    """gpode_rollout_fwd_ns with s sub-steps, or (s None) gpode_rollout_fwd_nt on ts as it is -> rc, Bufs(zt, xstage), tag"""
    from vae_gp_ode_amd.ops import NSTAGE, _ptr, _stream
    N, D = z0.shape[-2:]
    T = ts.shape[-1]
    b = Bufs()
    zt = b.new('zt', nd, N, T, D)
    xs = b.new('xstage', nd, N, T - 1, _rows(s), NSTAGE.get(method, 1), D)
    a = _head(cb, nd, order, method) + (_ptr(cb.pack), _ptr(z0), _ptr(ts), N, T, _ptr(zt), _ptr(xs), int(z0.dim() == 3), int(ts.dim() == 2))
    lib = _lib_()
    rc = lib.gpode_rollout_fwd_nt(*a, _stream()) if s is None else lib.gpode_rollout_fwd_ns(*a, s, _stream())
    return rc, b, _tag()


def bwd(cb, nd, xs, gzt, ts, order, method, s=None, fused=0):
    """gpode_rollout_bwd_ns / _nt (fused = the chunk count: gpode_rollout_bwd_pgrad_ns / _nt) -> rc, Bufs(gz0, astage[, gpack]), tag"""
    from vae_gp_ode_amd.ops import NSTAGE, _ptr, _stream
    N, T, D = gzt.shape[-3:]
    b = Bufs()
    gz0, ast = b.new('gz0', nd, N, D), b.new('astage', nd, N, T - 1, _rows(s), NSTAGE.get(method, 1), cb.Do)
    a = _head(cb, nd, order, method) + (_ptr(cb.pack), _ptr(xs), _ptr(gzt), _ptr(ts), N, T, _ptr(gz0), _ptr(ast))
    lib = _lib_()
    if fused:
        pf = cb.pack.shape[-1]
        a += (_ptr(b.new('slab', nd * fused * pf)), fused, _ptr(b.new('gpack', nd, pf)))
        f = lib.gpode_rollout_bwd_pgrad_nt if s is None else lib.gpode_rollout_bwd_pgrad_ns
    else:
        f = lib.gpode_rollout_bwd_nt if s is None else lib.gpode_rollout_bwd_ns
    rc = f(*a, int(ts.dim() == 2), _stream()) if s is None else f(*a, int(ts.dim() == 2), s, _stream())
    return rc, b, _tag()


def dev_inputs(c):
    p, nz, z0, _, _ = IR.inputs(c)
    return ({k: v.cuda() for k, v in p.items()}, {k: v.cuda() for k, v in nz.items()}), z0


def same(a, b):
    """torch.equal on the values, and no NaN left on either side"""
    return a.shape == b.shape and not torch.isnan(a).any() and torch.equal(a, b)


# Across the two instantiations of a rollout kernel (door shut) the comparison is between two separately compiled kernels, which need not
# round alike: measured, 3 of 240 states differed by one unit in the last place (3.0e-8 of 1.95) on one model.  Each side is held to the
# fp64 oracle by the project's bounds -- integrator_routes.FLOOR (2e-5) for the launches' outputs, test_gpu_time_grids.oracle_bound's
# floors (2e-4 trajectories, 1e-3 gradients) through ops.flow -- so the two are within twice that of each other; that is the bound here.
# With the door open it is one kernel against itself and the bound is torch.equal.
def agree(a, b, exact, bound, what=''):
    if exact:
        return same(a, b)
    if a.shape != b.shape or torch.isnan(a).any() or torch.isnan(b).any():
        return False
    e = IR.relerr(a, b)
    if e:
        print('%s: %d of %d elements differ across the two instantiations, relative to the largest entry %.2e (bound %.1e)'
              % (what, int((a != b).sum()), a.numel(), e, bound))
    return e <= bound


RAW_BOUND = 2 * 2e-5
FLOW_BOUND = {'zt': 2 * 2e-4, 'grad': 2 * 1e-3}


# ---- 1. bit for bit against the refined grid --------------------------------------------------------------------------------------------
def bit_cases():
    """(id, case, z0 per draw): one case per forward route (N = 5 on the team routes, 2049 on the wave routes; between them both
    reverse routes), the three solvers on one RBF case, order 2, two draws with shared and with per-draw z0, and the fused cases"""
    out = []
    for route, c in route_cases():
        c = c._replace(N=5 if 'team' in route else 2049)
        assert IR.forward_route(c) == route, (route, c)
        out.append((route, c, False))
    assert {IR.backward_resident(c) for _, c, _ in out} == {True, False}
    out += [('rbf-' + m, IR.R_(6, 6, 1, 100, 256, 5, m), False) for m in ('euler', 'midpoint', 'rk4')]
    out += [('order2', IR.R_(6, 3, 2, 17, 33, 5, 'rk4'), False), ('order2-wave', IR.R_(6, 3, 2, 17, 33, 2049, 'midpoint'), False),
            ('draws2', IR.R_(6, 6, 1, 100, 256, 5, 'rk4', nd=2), False), ('draws2-z0', IR.D_(6, 100, 256, 5, 'midpoint', nd=2), True),
            ('draws2-z0-wave', IR.R_(6, 6, 1, 100, 256, 2049, 'euler', nd=2), True)]
    out += [('fused-' + c.method, c, False) for c in IR.TABLE if c.kind == 'fused']
    out += [('fused-team-rk4', IR.R_(6, 6, 1, 100, 256, 5, 'rk4', kind='fused'), False)]
    return out


@pytest.fixture
def one_step_through_the_substep_kernels():
    """gpode_test_substep_kernels(1) for the test, shut again whatever happens: one-step launches take the sub-step instantiation of the
    rollout kernels, so that what the test compares is one instantiation with itself"""
    lib = _lib_()
    assert lib.gpode_test_substep_kernels(1) == 0
    try:
        yield
    finally:
        assert lib.gpode_test_substep_kernels(0) == 0


@pytest.mark.parametrize('name,c,zpd', bit_cases(), ids=[n for n, _, _ in bit_cases()])
def test_substeps_launch_against_the_one_step_kernels_on_the_refined_grid(name, c, zpd):
    """door shut: the sub-step instantiation against the one-step instantiation, two compiled kernels -- to RAW_BOUND"""
    _bit_case(name, c, zpd, exact=False)


@pytest.mark.parametrize('name,c,zpd', bit_cases(), ids=[n for n, _, _ in bit_cases()])
def test_substeps_launch_equals_the_launch_on_the_refined_grid(name, c, zpd, one_step_through_the_substep_kernels):
    """the refined-grid launch served by the sub-step instantiation: the same kernel on the same rows in the same order -- torch.equal"""
    _bit_case(name, c, zpd, exact=True)


def _bit_case(name, c, zpd, exact):
    from vae_gp_ode_amd import ops
    dev_in, z0 = dev_inputs(c)
    cb = IR.build(c, dev_in)
    nd, N, T = c.nd, c.N, T_EXACT
    g = torch.Generator().manual_seed(11)
    z = (z0[None] + 0.3 * torch.randn(nd, *z0.shape, generator=g)).cuda() if zpd else z0.cuda()
    gzt = torch.randn(nd, N, T, c.Di, generator=g).cuda()
    fused = ops.pgrad_chunks(cb, N, c.order, c.method, force=True) if c.kind == 'fused' else 0
    assert (fused > 0) == (c.kind == 'fused')
    want_fwd = 'rollout_' + IR.forward_route(c)
    want_bwd = 'reduce_slab' if fused else 'rollout_bwd_%s%s' % (c.kernel.lower(), '' if IR.backward_resident(c) else '_stream')
    plain = None
    for gname, ts in exact_grids(N).items():
        ts = ts.cuda()
        for s in (1, 2, 4):
            what = (name, gname, s)
            fine = refine(ts, s).contiguous()
            rc, A, tag = fwd(cb, nd, z, ts, c.order, c.method, s)
            assert rc == 0 and tag == want_fwd, (what, _err(), tag)
            rc, B, tag = fwd(cb, nd, z, fine, c.order, c.method)
            assert rc == 0 and tag == want_fwd, (what, _err(), tag)
            assert agree(A.t['zt'], B.t['zt'][:, :, ::s], exact, RAW_BOUND, 'zt'), what
            assert agree(A.t['xstage'], B.t['xstage'].view_as(A.t['xstage']), exact, RAW_BOUND, 'xstage'), what
            gfine = scatter_frames(gzt, s).contiguous()
            rc, Ab, tag = bwd(cb, nd, A.t['xstage'], gzt, ts, c.order, c.method, s, fused)
            assert rc == 0 and tag == want_bwd, (what, _err(), tag)
            rc, Bb, tag = bwd(cb, nd, B.t['xstage'], gfine, fine, c.order, c.method, None, fused)
            assert rc == 0 and tag == want_bwd, (what, _err(), tag)
            assert agree(Ab.t['gz0'], Bb.t['gz0'], exact, RAW_BOUND, 'gz0'), what
            assert agree(Ab.t['astage'], Bb.t['astage'].view_as(Ab.t['astage']), exact, RAW_BOUND, 'astage'), what
            if fused:
                if exact:
                    assert torch.equal(Ab.t['gpack'].view(torch.int32), Bb.t['gpack'].view(torch.int32)), what     # pad lanes may hold NaN
                else:
                    assert agree(torch.nan_to_num(Ab.t['gpack']), torch.nan_to_num(Bb.t['gpack']), False, RAW_BOUND, 'gpack'), what
                assert not torch.isnan(IR.unpack(c, Ab.t['gpack'].cpu(), IR.cache_dicts(c, cb, dev_in))['omega']).any()
            # the second run: the same bits; and nothing behind any buffer
            rc, A2, _ = fwd(cb, nd, z, ts, c.order, c.method, s)
            rc2, Ab2, _ = bwd(cb, nd, A.t['xstage'], gzt, ts, c.order, c.method, s, fused)
            assert rc == 0 and rc2 == 0
            for x, y in ((A, A2), (Ab, Ab2)):
                for k in x.t:
                    if k != 'slab':
                        assert torch.equal(x.t[k].view(torch.int32), y.t[k].view(torch.int32)), (what, k, 'second run')
            for b in (A, B, Ab, Bb, A2, Ab2):
                assert not b.guards_changed(), (what, b.guards_changed())
            if s == 1:
                plain = (A, Ab)
            else:                                    # the sub-steps do change the result
                assert not torch.equal(A.t['zt'], plain[0].t['zt']) and not torch.equal(Ab.t['gz0'], plain[1].t['gz0']), what


def test_one_substep_is_the_twin():
    """substeps = 1: every output and the tag of the `_nt` twin (and of `_n`), on a team and on a wave route, shared and per-row grids"""
    from vae_gp_ode_amd.ops import _ptr, _stream
    for c in (IR.R_(6, 6, 1, 100, 256, 5, 'rk4', nd=2, kind='fused'), IR.D_(6, 100, 256, 2049, 'euler')):
        dev_in, z0 = dev_inputs(c)
        cb = IR.build(c, dev_in)
        z = z0.cuda()
        gzt = torch.randn(c.nd, c.N, T_EXACT, c.Di, generator=torch.Generator().manual_seed(12)).cuda()
        for gname, ts in exact_grids(c.N).items():
            ts = ts.cuda()
            rc, A, ta = fwd(cb, c.nd, z, ts, c.order, c.method, 1)
            rc2, B, tb = fwd(cb, c.nd, z, ts, c.order, c.method)
            assert rc == 0 and rc2 == 0 and ta == tb == 'rollout_' + IR.forward_route(c)
            assert same(A.t['zt'], B.t['zt']) and same(A.t['xstage'], B.t['xstage'])
            for fused in ((0, 5) if c.kind == 'fused' else (0,)):
                rc, Ab, ta = bwd(cb, c.nd, A.t['xstage'], gzt, ts, c.order, c.method, 1, fused)
                rc2, Bb, tb = bwd(cb, c.nd, A.t['xstage'], gzt, ts, c.order, c.method, None, fused)
                assert rc == 0 and rc2 == 0 and ta == tb, (_err(), ta, tb)
                assert same(Ab.t['gz0'], Bb.t['gz0']) and same(Ab.t['astage'], Bb.t['astage'])
                if fused:
                    assert torch.equal(Ab.t['gpack'].view(torch.int32), Bb.t['gpack'].view(torch.int32))
            if ts.dim() == 1:                        # and the `_n` entry point, which forwards to the same launch
                zt, xs = IR._guarded(c.nd, c.N, T_EXACT, c.Di)[0], IR._guarded(*A.t['xstage'].shape)[0]
                _lib_().gpode_rollout_fwd_n(*_head(cb, c.nd, c.order, c.method), _ptr(cb.pack), _ptr(z), _ptr(ts), c.N, T_EXACT, _ptr(zt), _ptr(xs),
                                            _stream())
                assert same(zt, A.t['zt']) and same(xs, A.t['xstage'])


def test_refusals_write_nothing():
    from vae_gp_ode_amd import ops
    c = IR.R_(6, 6, 1, 16, 32, 5, 'rk4', kind='fused')
    dev_in, z0 = dev_inputs(c)
    cb = IR.build(c, dev_in)
    z, ts = z0.cuda(), exact_grids(c.N)['gaps'].cuda()
    xs = torch.randn(1, c.N, T_EXACT - 1, 2, 4, 6).cuda()
    gzt = torch.randn(1, c.N, T_EXACT, 6).cuda()
    nch = ops.pgrad_chunks(cb, c.N, 1, 'rk4', force=True)
    for bad in (0, 65, -1, 1 << 20):
        rc, b, _ = fwd(cb, 1, z, ts, 1, 'rk4', bad)
        assert rc != 0 and _err().startswith('gpode_rollout_fwd_ns:') and 'substeps=%d' % bad in _err() and b.untouched(), _err()
        rc, b, _ = bwd(cb, 1, xs, gzt, ts, 1, 'rk4', bad)
        assert rc != 0 and _err().startswith('gpode_rollout_bwd_ns:') and 'substeps=%d' % bad in _err() and b.untouched(), _err()
        rc, b, _ = bwd(cb, 1, xs, gzt, ts, 1, 'rk4', bad, nch)
        assert rc != 0 and _err().startswith('gpode_rollout_bwd_pgrad_ns:') and 'substeps=%d' % bad in _err() and b.untouched(), _err()
    # dopri5 is refused as in the twins, whatever the count
    for s in (1, 2):
        rc, b, _ = fwd(cb, 1, z, ts, 1, 3, s)
        assert rc != 0 and 'method 3' in _err() and b.untouched(), _err()
        rc, b, _ = bwd(cb, 1, xs, gzt, ts, 1, 3, s)
        assert rc != 0 and 'method 3' in _err() and b.untouched(), _err()
        rc, b, _ = bwd(cb, 1, xs, gzt, ts, 1, 3, s, nch)
        assert rc != 0 and b.untouched(), _err()
    with pytest.raises(ops._lib.GpodeError, match='dopri5'):
        ops.rollout(cb, z, ts, 1, 'dopri5', substeps=2)
    # and the calls the refusals were variations of go through, at either end of the range
    for s in (2, 64):
        rc, b, _ = fwd(cb, 1, z, ts, 1, 'rk4', s)
        assert rc == 0 and not torch.isnan(b.t['zt']).any() and not torch.isnan(b.t['xstage']).any() and not b.guards_changed()
        rc, bb, _ = bwd(cb, 1, b.t['xstage'], gzt, ts, 1, 'rk4', s, nch)
        assert rc == 0 and not torch.isnan(bb.t['gz0']).any() and not torch.isnan(bb.t['astage']).any() and not bb.guards_changed()


# ---- 2. ops.flow / Flow ------------------------------------------------------------------------------------------------------------------
FLOW_CASES = [(dict(solver='euler'), None, 'uniform'), (dict(solver='rk4'), 3, 'gaps'), (dict(solver='midpoint'), None, 'rows'),
              (dict(ode=2, D_in=6, D_out=3, latent_dim=3, frames=3, solver='rk4'), 2, 'rows'), (dict(kernel='DF', solver='rk4'), None, 'gaps')]
FLOW_IDS = ['euler', 'rk4-draws', 'midpoint-rows', 'order2-draws-rows', 'df']


@pytest.mark.parametrize('s', [2, 4])
@pytest.mark.parametrize('kw,L,grid', FLOW_CASES, ids=FLOW_IDS)
def test_flow_with_substeps_against_the_one_step_kernels_on_the_refined_grid(kw, L, grid, s):
    """door shut: two compiled kernels -- to FLOW_BOUND"""
    _flow_case(kw, L, grid, s, exact=False)


@pytest.mark.parametrize('s', [2, 4])
@pytest.mark.parametrize('kw,L,grid', FLOW_CASES, ids=FLOW_IDS)
def test_flow_with_substeps_is_the_flow_on_the_refined_grid(kw, L, grid, s, one_step_through_the_substep_kernels):
    """Flow() on the refined grid served by the sub-step instantiation: one kernel against itself -- torch.equal"""
    _flow_case(kw, L, grid, s, exact=True)


def _flow_case(kw, L, grid, s, exact):
    from vae_gp_ode_amd.model.core.flow import EVALS_PER_STEP
    m, src = tiny_model(**kw)
    flow, gp = m.flow, m.flow.odefunc.diffeq
    N, D, T = 5, kw.get('D_in', 6), T_EXACT
    g = torch.Generator().manual_seed(21)
    z0 = torch.randn(N, D, generator=g).cuda()
    W = torch.randn(*((L,) if L else ()), N, T, D, generator=g).cuda()
    ts = exact_grids(N)[grid].cuda()
    params = [p for p in gp.parameters() if p.requires_grad]
    assert len(params) == 5 and flow.substeps == 1

    def run(sub, ts_, stride):
        for p in params:
            p.grad = None
        flow.substeps = sub
        src.manual_seed(17)                          # the generator state put back: the same function draw(s)
        z = z0.clone().requires_grad_(True)
        zt = flow(z, ts_, draws=L)[..., ::stride, :]
        (zt * W).sum().backward()
        return zt.detach(), z.grad, [p.grad.clone() for p in params], flow.num_evals()
    za, ga, pa, na = run(s, ts, 1)
    zb, gb, pb, nb = run(1, refine(ts, s), s)
    zc, gc, pc, nc = run(1, ts, 1)
    assert na == nb == EVALS_PER_STEP[flow.solver] * (T - 1) * s and nc == EVALS_PER_STEP[flow.solver] * (T - 1)
    for name, a, b in [('zt', za, zb), ('dL/dz0', ga, gb)] + [('dL/d %s' % (tuple(p.shape),), a, b) for a, b, p in zip(pa, pb, params)]:
        print('%s: %d of %d elements differ from the refined-grid flow, largest difference %.3e of %.3e'
              % (name, int((a != b).sum()), a.numel(), (a - b).abs().max().item(), b.abs().max().item()))
    assert tuple(za.shape) == tuple(W.shape) and agree(za, zb, exact, FLOW_BOUND['zt'], 'zt')
    assert agree(ga, gb, exact, FLOW_BOUND['grad'], 'dL/dz0') and ga.abs().max().item() > 0
    for a, b, p in zip(pa, pb, params):
        assert agree(a, b, exact, FLOW_BOUND['grad'], 'dL/d %s' % (tuple(p.shape),)) and a.abs().max().item() > 0, tuple(p.shape)
    assert not torch.equal(za, zc) and not torch.equal(ga, gc)


def test_zero_padded_width_passes_the_count_through(one_step_through_the_substep_kernels):
    """a latent width outside the compiled list runs on zero-padded operands (ops.WidthPad): the count goes through as it is"""
    from test_gpu_z0_draws import _tiny_model
    m = _tiny_model('RBF', 1, 5, 'midpoint')
    from vae_gp_ode_amd.model.core.noise import install_device_noise
    src = install_device_noise(m, 17)
    gp = m.flow.odefunc.diffeq
    assert gp.width_pad is not None
    N = 7
    z0 = torch.randn(N, 5, generator=torch.Generator().manual_seed(41)).cuda()
    ts = exact_grids(N)['rows'].cuda()

    def run(sub, ts_, stride):
        m.flow.substeps = sub
        src.manual_seed(17)
        z = z0.clone().requires_grad_(True)
        zt = m.flow(z, ts_)[:, ::stride]
        zt.square().sum().backward()
        return zt.detach(), z.grad
    a, b = run(2, ts, 1), run(1, refine(ts, 2), 2)
    assert tuple(a[0].shape) == (N, T_EXACT, 5) and same(a[0], b[0]) and same(a[1], b[1]) and a[1].abs().max().item() > 0


# ---- 3. against the fp64 oracle on the refined grid -------------------------------------------------------------------------------------
S_ORACLE = 3
ORACLE_CASES = [('rbf-rk4', IR.R_(6, 6, 1, 100, 256, 5, 'rk4'), False), ('rbf-fused-euler', IR.R_(6, 6, 1, 100, 256, 2049, 'euler', kind='fused'), False),
                ('df-midpoint', IR.D_(6, 100, 256, 5, 'midpoint'), False), ('rbf-order2-rk4', IR.R_(6, 3, 2, 17, 33, 5, 'rk4'), False),
                ('rbf-rk4-rows', IR.R_(6, 6, 1, 100, 256, 5, 'rk4'), True)]


def oracle_on_the_refined_grid(c, cache, dtype, z0, rows, gw, s):
    """integrator_routes.reference, unmodified, on refine(grid, s) with dL/dzt scattered into every s-th frame -- once per group of
    trajectories that share a grid; the per-row outputs put back in place (zt: every s-th frame), the leaf gradients summed"""
    N = z0.shape[0]
    groups = {}
    for n in range(N):
        groups.setdefault(tuple(rows[n].tolist()), []).append(n)
    out = {}
    for row, idx in groups.items():
        idx = torch.tensor(idx)
        fine = refine(torch.tensor(row, dtype=torch.float64), s)
        r = IR.reference(c, cache, dtype, z0=z0[idx], ts=fine, gw=scatter_frames(gw[:, idx], s))
        r['zt'] = r['zt'][:, :, ::s]
        for k, v in r.items():
            if k in IR.OUT_ROLL:
                out.setdefault(k, torch.zeros((v.shape[0], N) + tuple(v.shape[2:]), dtype=v.dtype))[:, idx] = v
            elif k in IR.OUT_LEAF:
                out[k] = out[k] + v if k in out else v
    return out


@pytest.mark.parametrize('name,c,per_row', ORACLE_CASES, ids=[n for n, _, _ in ORACLE_CASES])
def test_against_the_fp64_oracle_on_the_refined_grid(name, c, per_row):
    from vae_gp_ode_amd import ops
    from vae_gp_ode_amd.ops import _ptr, _stream
    s, T = S_ORACLE, 3
    assert c.T == T
    dev_in, z0 = dev_inputs(c)
    p, nz, _, ts, gw = IR.inputs(c)
    assert tuple(ts.tolist()) == tuple(torch.tensor(IR.TS[3]).tolist())
    rows = ts[None].expand(c.N, -1)
    if per_row:                                      # every other trajectory on the grid stretched by 1.7: not exact either
        rows = torch.stack([ts * (1.7 if n % 2 else 1.0) for n in range(c.N)]).contiguous()
    cb = IR.build(c, dev_in)
    cache = IR.cache_dicts(c, cb, dev_in)
    grid = (rows if per_row else ts).cuda()
    rc, A, tag = fwd(cb, c.nd, z0.cuda(), grid, c.order, c.method, s)
    assert rc == 0 and tag == 'rollout_' + IR.forward_route(c), (_err(), tag)
    fused = ops.pgrad_chunks(cb, c.N, c.order, c.method, force=True) if c.kind == 'fused' else 0
    rc, Ab, tag = bwd(cb, c.nd, A.t['xstage'], gw.cuda(), grid, c.order, c.method, s, fused)
    assert rc == 0, _err()
    if fused:
        gpack = Ab.t['gpack']
    else:                                            # the parameter sums over all rows of the record, unchanged
        R = c.N * (T - 1) * s * IR.NSTAGE[c.method]
        nchunk = max(1, min(min(256, max(64, R // 32)), R))
        pf = cb.pack.shape[-1]
        B = Bufs()
        gpack = B.new('gpack', c.nd, pf)
        rc = _lib_().gpode_param_grad_n(*_head(cb, c.nd, c.order, c.method)[:1], c.Di, c.Do, c.M, c.S, c.nd, _ptr(cb.pack), _ptr(A.t['xstage']),
                                        _ptr(Ab.t['astage']), R, _ptr(B.new('slab', c.nd * nchunk * pf)), nchunk, _ptr(gpack), 0, _stream())
        assert rc == 0 and not B.guards_changed(), _err()
    assert not A.guards_changed() and not Ab.guards_changed()
    got = dict(zt=A.t['zt'].cpu(), xstage=A.t['xstage'].cpu(), gz0=Ab.t['gz0'].cpu(), astage=Ab.t['astage'].cpu())
    got.update(IR.unpack(c, gpack.cpu(), cache))
    r64, r32 = (oracle_on_the_refined_grid(c, cache, dt, z0, rows, gw, s) for dt in (torch.float64, torch.float32))
    assert tuple(r64['xstage'].shape) == (c.nd, c.N, T - 1, s * IR.NSTAGE[c.method], c.Di)
    print(name)
    IR.compare(c, got, r64, r32, ['zt', 'xstage', 'gz0', 'astage'] + [k for k in IR.OUT_LEAF if k in r64], 's = %d: ' % s)
    # (xstage holds the states at the starts of the sub-steps: a launch that took other steps could not meet its bound)


# ---- 4. what it is for ------------------------------------------------------------------------------------------------------------------
ORDER_MODELS = [('rbf', IR.R_(6, 6, 1, 100, 256, 5, 'euler')), ('df', IR.D_(6, 100, 256, 5, 'euler')), ('rbf-order2', IR.R_(6, 3, 2, 17, 33, 5, 'euler'))]


@pytest.mark.parametrize('name,c', ORDER_MODELS, ids=[n for n, _ in ORDER_MODELS])
def test_substeps_buy_the_order_of_the_solver(name, c):
    from oracle import gpode_oracle as O
    dev_in, z0 = dev_inputs(c)
    cb = IR.build(c, dev_in)
    cache = {k: (v.double() if torch.is_tensor(v) else v) for k, v in IR.cache_dicts(c, cb, dev_in)[0].items()}
    ts = 0.25 * torch.arange(6, dtype=torch.float32)
    with torch.no_grad():
        ref = O.flow_forward(z0.double(), refine(ts.double(), 64), cache, c.order, 'rk4')[:, ::64]
    assert tuple(ref.shape) == (c.N, 6, c.Di)
    err = {}
    for method, s_hi, gain in (('euler', 8, 4.0), ('midpoint', 4, 8.0)):
        for s in (1, s_hi):
            rc, A, _ = fwd(cb, 1, z0.cuda(), ts.cuda(), c.order, method, s)
            assert rc == 0 and not A.guards_changed(), _err()
            err[method, s] = IR.relerr(A.t['zt'][0], ref)
        print('%s %s: error to rk4 x 64 in fp64 at s = 1: %.2e, at s = %d: %.2e, ratio %.1f (asked: %.0f)'
              % (name, method, err[method, 1], s_hi, err[method, s_hi], err[method, 1] / err[method, s_hi], gain))
    assert err['euler', 8] <= err['euler', 1] / 4.0, err
    assert err['midpoint', 4] <= err['midpoint', 1] / 8.0, err
    assert err['euler', 8] > 1e-3 and err['midpoint', 4] > 2e-5, err       # far above the float32 floor: truncation error is what is measured


# ---- 5. the layers above ----------------------------------------------------------------------------------------------------------------
def test_main_trains_with_ts_dense_scale(tmp_path, monkeypatch):
    """test_gpu_time_grids.test_main_trains_on_subsampled_sequences's configuration plus --ts_dense_scale 3: two steps, eagerly and replayed"""
    from vae_gp_ode_amd import main as M
    from vae_gp_ode_amd import ops, vae_ops
    monkeypatch.chdir(tmp_path)
    common = ['--task', 'synthetic', '--Ndata', '8', '--Ntest', '4', '--batch', '4', '--T', '6', '--solver', 'rk4', '--num_inducing', '16',
              '--num_features', '32', '--lr', '1e-4', '--log_freq', '1', '--Nepoch', '1', '--subsample_frames', '4', '--ts_dense_scale', '3']
    try:
        for tag, extra in (('s', []), ('g', ['--hip_graph', 'True'])):
            M.main(common + ['--save', 'results/' + tag] + extra)
            ck = glob.glob(str(tmp_path / 'results' / (tag + '_*') / 'odegpvae_mnist.pth'))
            assert len(ck) == 1
            sd = torch.load(ck[0])
            assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
            log = open(glob.glob(str(tmp_path / 'results' / (tag + '_*') / 'logs'))[0]).read()
            elbo = [float(ln.split('elbo')[1].split('(')[0]) for ln in log.splitlines() if ln.startswith('Iter:')]
            assert len(elbo) == 2 and all(math.isfinite(v) for v in elbo), elbo
            assert '--ts_dense_scale 3: 2 rk4 steps inside every output interval' in log and 'keeps 4 of its frames' in log
    finally:                                         # process-wide switches the training loop sets for itself
        ops.set_overlap(False)
        vae_ops.set_deferred_reductions(False)
    with pytest.raises(SystemExit, match='--ts_dense_scale 66'):
        M.main(common[:-1] + ['66', '--save', 'results/x'])


def test_graph_replay_with_substeps_equals_eager_steps():
    """test_gpu_time_grids.test_graph_replay_reads_the_grids_from_a_static_buffer with Flow(substeps=2): the count is a constant of the
    captured step; one eager warm-up step and two replays equal three eager steps, losses and parameters, bit for bit"""
    from vae_gp_ode_amd.data.utils import subsample_frames
    from vae_gp_ode_amd.graph import GraphedStep
    from vae_gp_ode_amd.model.create_model import compute_loss
    from vae_gp_ode_amd.optim import HipAdam
    m, src = tiny_model(solver='euler', ts_dense_scale=3)   # Euler: the sub-steps move the loss by far more than its float32 spacing
    assert m.flow.substeps == 2
    init = copy.deepcopy(m.state_dict())
    N = 4
    X = torch.rand(N, 6, 1, 28, 28, generator=torch.Generator().manual_seed(15)).cuda()
    gen = torch.Generator(device='cuda').manual_seed(3)
    batches = []
    for _ in range(2):
        Xs, idx = subsample_frames(X, 4, 1, gen)
        batches.append((Xs.contiguous(), (m.dt * idx.float()).contiguous()))
    assert not torch.equal(batches[0][1], batches[1][1])
    order = (0, 0, 1)

    def run(use_graph, substeps=2):
        m.load_state_dict(init)
        m.flow.substeps = substeps
        src.manual_seed(17)
        opt = HipAdam(m.parameters(), lr=1e-3)
        buf, tbuf = torch.empty_like(batches[0][0]), torch.empty_like(batches[0][1])

        def step():
            opt.zero_grad()
            loss, *_ = compute_loss(m, buf, 1, ts=tbuf)
            loss.backward()
            opt.step()
            return loss
        losses = []
        gs = None
        for b in order:
            buf.copy_(batches[b][0]); tbuf.copy_(batches[b][1])
            if not use_graph:
                losses.append(step().detach().clone())
            elif gs is None:
                gs = GraphedStep(step, warmup=1)
                losses.append(gs.warm_out.clone())
            else:
                losses.append(gs().clone())
        torch.cuda.synchronize()
        return losses, [p.detach().clone() for p in m.parameters()]
    le, pe = run(False)
    lg, pg = run(True)
    l1, _ = run(False, substeps=1)
    assert m.flow.num_evals() == 1 * 3 * 1
    assert all(torch.isfinite(x).all() for x in le)
    assert all(torch.equal(a, b) for a, b in zip(le, lg)), ([x.item() for x in le], [x.item() for x in lg])
    assert all(torch.equal(a, b) for a, b in zip(pe, pg))
    assert not torch.equal(le[1], le[2]) and not torch.equal(le[0], l1[0])            # the batches differ, and so do the sub-steps


def test_evaluate_with_ts_dense_scale(tmp_path, capsys):
    from vae_gp_ode_amd import evaluate as E
    from vae_gp_ode_amd.model.create_model import build_model
    from vae_gp_ode_amd.model.misc.torch_utils import seed_everything
    argv = ['--task', 'synthetic', '--Ndata', '8', '--Ntest', '6', '--batch', '4', '--T', '6', '--solver', 'midpoint', '--num_inducing', '16',
            '--num_features', '32', '--model_path', str(tmp_path), '--eval_sample_size', '4', '--Troll', '2', '--save', str(tmp_path / 'ev'),
            '--device_noise', 'True']
    args = E.make_parser().parse_args(argv)
    args.device = torch.device('cuda')
    seed_everything(3)
    torch.save(build_model(args).to(args.device).state_dict(), tmp_path / 'odegpvae_mnist.pth')
    plain = E.main(argv)
    two = E.main(argv + ['--ts_dense_scale', '2'])
    dense = E.main(argv + ['--ts_dense_scale', '3'])
    again = E.main(argv + ['--ts_dense_scale', '3'])
    capsys.readouterr()
    strip = lambda d: {k: v for k, v in d.items() if k != 'ms'}
    assert strip(two) == strip(plain)                                   # the default: one step per interval, the run as it was
    assert strip(dense) == strip(again)
    assert all(math.isfinite(dense[k]) for k in ('mse', 'nll', 'nlpd'))
    assert all(dense[k] != plain[k] for k in ('mse', 'nll', 'nlpd')), (dense, plain)
    with pytest.raises(SystemExit, match='--ts_dense_scale 66'):
        E.main(argv + ['--ts_dense_scale', '66'])


def test_compact_ragged_loss_on_a_substeps_model():
    """test_gpu_ragged_compact.test_the_padding_is_gone on a substeps = 2 model: the loss runs, the gradient that reaches the flow is
    exactly zero at every padded frame, and so neither the padded columns of ts nor the padded target frames reach a result"""
    from test_gpu_ragged_compact import L, T, run
    from test_gpu_ragged_model import ragged_batch
    m, src = tiny_model(solver='euler', ts_dense_scale=3)       # Euler: the sub-steps move the loss by far more than its float32 spacing
    assert m.flow.substeps == 2
    init = copy.deepcopy(m.state_dict())
    X, ts, n_obs = ragged_batch(m)
    seen = []
    inner = m.flow.forward

    def watched(z0, ts_, draws=None):
        zt = inner(z0, ts_, draws=draws)
        if zt.requires_grad:
            zt.register_hook(lambda g: seen.append(g.detach().clone()))
        return zt
    m.flow.forward = watched
    try:
        out, g = run(m, src, X, L, ts=ts, n_obs=n_obs, compact=True)
    finally:
        del m.flow.forward
    assert all(torch.isfinite(t).all() for t in out) and m.flow.num_evals() == 1 * (T - 1) * 2
    assert len(seen) == 1 and tuple(seen[0].shape)[:3] == (L, X.shape[0], T)
    for n, k in enumerate(n_obs.tolist()):
        assert k < T or (n_obs < T).any()
        assert not seen[0][:, n, k:].any(), (n, k)                      # exactly zero at the padded frames
        assert seen[0][:, n, :k].abs().max().item() > 0
    gU = g['flow.odefunc.diffeq.Um.optvar']
    assert torch.isfinite(gU).all() and gU.abs().max().item() > 0
    # other padding, the same result
    ts2, X2 = ts.clone(), X.clone()
    for n, k in enumerate(n_obs.tolist()):
        ts2[n, k:] = ts[n, k - 1] + 0.037 * torch.arange(1, T - k + 1, device=ts.device)
        X2[n, k:] = 0.25 + 0.5 * torch.rand(X[n, k:].shape, generator=torch.Generator().manual_seed(3)).cuda()
    assert bool((ts2[:, 1:] > ts2[:, :-1]).all()) and not torch.equal(ts, ts2) and not torch.equal(X, X2)
    m.load_state_dict(init)
    out2, g2 = run(m, src, X2, L, ts=ts2, n_obs=n_obs, compact=True)
    assert all(torch.equal(a, b) for a, b in zip(out, out2)) and not [k for k in g if not torch.equal(g[k], g2[k])]
    # and it is the sub-steps' loss, not the plain model's
    m.load_state_dict(init)
    m.flow.substeps = 1
    out1, _ = run(m, src, X, L, ts=ts, n_obs=n_obs, compact=True)
    assert not torch.equal(out[0], out1[0])
