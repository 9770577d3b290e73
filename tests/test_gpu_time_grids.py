"""GPU: a time grid PER TRAJECTORY -- gpode_rollout_fwd_nt / _adaptive_fwd_nt / _dense_fwd_nt / gpode_rollout_bwd_nt / _bwd_pgrad_nt,
their routing through ops.rollout / ops.flow, and ODEGPVAE / compute_loss / evaluate / main.py on top of them.

The reference of most tests is the GPU's own shared-grid launch.  Three distinct non-uniform grids G0..G2 (T = 4) are dealt out to the
trajectories, G[n % 3] to trajectory n.  A trajectory's arithmetic depends on its own z0, its grid and the pack alone, so row n of the one
(N,T) launch must equal, BIT FOR BIT, row n of the shared-grid launch over the same N trajectories (the same N: the same route, read back
from gpode_last_launch()) with grid G[n % 3].  Floats are compared as their bit patterns, so a NaN equals itself.

What is held to what:
  * fixed grid, every forward route (the first 'full' case of integrator_routes.TABLE per route; N on both sides of 2048), 1 and 3
    draws, shared and per-draw z0: zt and xstage to BITS; ts_per_traj = 0 against the `_nz` twin and ts_per_traj = 1 on N copies of one
    grid against the shared launch: BITS; ts_per_traj = 2: refused, the NaN fill intact;
  * reverse sweep on resident and streamed evaluators, euler / rk4 / midpoint: gz0 and astage to BITS; the fused form: gz0 / astage to
    BITS against the unfused `_nt` sweep, gpack against gpode_param_grad_n on the same (xstage, astage) to integrator_routes.bound with
    the oracle term left out (the two are float32 sums of the same terms in another order: the floor alone, the tighter bound);
  * against the fp64 oracle, one team and one wave case per kernel family, row group by row group on the cache the GPU built: zt, gz0,
    astage to integrator_routes.bound(key, e32) = FLOOR + 3 relerr(fp32 oracle, fp64);
  * dopri5, landing and dense, N = 5 (team) and N = 2049 (wave), rtol = atol = 1e-4, K = 4 (T - 1): every output and the record to BITS,
    the reverse sweep through ops likewise; a launch with one row that is not increasing: that trajectory status 3 and NaN from its
    first missed output, every other one as without it, to BITS;
  * ops.flow: ts (N,T) of equal rows against ts (T,): zt, dL/dz0, the five parameter gradients to BITS; distinct rows against the fp64
    oracle run per grid group, losses summed, to the bound of test_gpu_backward.test_streamed_backward_matches_fp64_oracle for the same
    quantities (that file states it inline and exports no helper for it: `oracle_bound` below restates the expression, not a new figure);
  * the model: compute_loss / predict / predict_marginal with the uniform grid spelt out per sequence against ts=None: BITS; a
    subsampled grid: finite, different; a captured step reads its grids from a static buffer: replay == eager, BITS;
  * main.py --subsample_frames, eager and --hip_graph; evaluate --subsample_frames."""
import copy
import glob
import json
import math

import pytest
import torch

import integrator_routes as IR
from test_gpu_backward import synthetic_gp
from test_gpu_eval import model_args
from test_gpu_forward import relerr
from test_gpu_z0_draws import _dopri5_setup, _tiny_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def leave_the_global_generators_as_found():
    """The tests of this file seed and draw from the process-wide generators (torch on the host and on the device, numpy through
    build_model, random); test files that run after this one build layers from the global generator without seeding it (the decoder chain
    of test_gpu_vae_layers.py), so what they see must not depend on whether this file ran: the states are put back when it is done."""
    import random
    import numpy as np
    saved = (torch.get_rng_state(), torch.cuda.get_rng_state_all(), np.random.get_state(), random.getstate())
    yield
    torch.set_rng_state(saved[0])
    torch.cuda.set_rng_state_all(saved[1])
    np.random.set_state(saved[2])
    random.setstate(saved[3])


T = 4
G = ((0.0, 0.05, 0.2, 0.3), (0.0, 0.12, 0.16, 0.4), (0.1, 0.2, 0.25, 0.55))      # distinct, non-uniform; the last does not start at 0


def grids(N, scale=1.0):
    """(G (3,T), rows (N,T) with row n = G[n % 3]) on the device"""
    g = (torch.tensor(G) * scale).cuda()
    return g, g[torch.arange(N) % 3].contiguous()


def bits(a, b):
    """the same shape and the same bit patterns (NaN == NaN)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def deal(outs):
    """outs[g] = the outputs (tensors with the trajectories on axis 1) of the shared launch with grid g: row n taken from outs[n % 3]"""
    res = []
    for i in range(len(outs[0])):
        t = torch.empty_like(outs[0][i])
        for g in range(3):
            t[:, g::3] = outs[g][i][:, g::3]
        res.append(t)
    return res


def _lib_():
    from vae_gp_ode_amd import _lib
    return _lib.load()


def _tag():
    return _lib_().gpode_last_launch().decode()


def _err():
    return _lib_().gpode_last_error().decode()


def nan(*s):
    return torch.full(s, float('nan'), device='cuda')


def per_draw(z0, nd, seed):
    g = torch.Generator().manual_seed(seed)
    return (z0[None] + 0.3 * torch.randn(nd, *z0.shape, generator=g)).cuda()


# ---- launches through the C ABI, on NaN-filled outputs ----------------------------------------------------------------------------------
def raw_fwd(cb, nd, z0, ts, order, method, entry, zflag=0, tflag=0):
    """gpode_rollout_fwd_n / _nz / _nt: rc, (zt, xstage)"""
    from vae_gp_ode_amd.ops import KERNEL_ID, METHOD_ID, NSTAGE, _ptr, _stream
    N, D = z0.shape[-2:]
    zt, xs = nan(nd, N, T, D), nan(nd, N, T - 1, NSTAGE[method], D)
    head = (KERNEL_ID[cb.kernel], order, METHOD_ID[method], cb.Di, cb.Do, cb.M, cb.S, nd, _ptr(cb.pack), _ptr(z0), _ptr(ts), N, T, _ptr(zt),
            _ptr(xs))
    lib = _lib_()
    tail = {'n': (), 'nz': (zflag,), 'nt': (zflag, tflag)}[entry]
    rc = getattr(lib, 'gpode_rollout_fwd_' + entry)(*head, *tail, _stream())
    return rc, (zt, xs)


def raw_bwd(cb, nd, xs, gzt, ts, order, method, entry, tflag=0):
    """gpode_rollout_bwd_n / _nt: rc, (gz0, astage)"""
    from vae_gp_ode_amd.ops import KERNEL_ID, METHOD_ID, NSTAGE, _ptr, _stream
    N, D = gzt.shape[-3], gzt.shape[-1]
    gz0, ast = nan(nd, N, D), nan(nd, N, T - 1, NSTAGE[method], cb.Do)
    head = (KERNEL_ID[cb.kernel], order, METHOD_ID[method], cb.Di, cb.Do, cb.M, cb.S, nd, _ptr(cb.pack), _ptr(xs), _ptr(gzt), _ptr(ts), N, T,
            _ptr(gz0), _ptr(ast))
    lib = _lib_()
    rc = lib.gpode_rollout_bwd_n(*head, _stream()) if entry == 'n' else lib.gpode_rollout_bwd_nt(*head, tflag, _stream())
    return rc, (gz0, ast)


def raw_adaptive(cb, nd, z0, ts, order, K, dense, entry, zflag=0, tflag=0):
    """the adaptive rollouts the same way: rc, (zt, counts, xstage, hstep, iend[, theta])"""
    from vae_gp_ode_amd.ops import KERNEL_ID, _ptr, _stream
    N, D = z0.shape[-2:]
    zt, xs, hs, th = nan(nd, N, T, D), nan(nd, N, K, 7 if dense else 6, D), nan(nd, N, K), nan(nd, N, T - 1)
    ie = torch.full((nd, N, T - 1), -7, dtype=torch.int32, device='cuda')
    counts = torch.full((nd, N, 4), -7, dtype=torch.int32, device='cuda')
    head = (KERNEL_ID[cb.kernel], order, 3, cb.Di, cb.Do, cb.M, cb.S, nd, _ptr(cb.pack), _ptr(z0), _ptr(ts), N, T, 1e-4, 1e-4, K, _ptr(zt),
            _ptr(xs), _ptr(hs), _ptr(ie)) + ((_ptr(th), _ptr(counts)) if dense else (_ptr(counts),))
    tail = {'n': (), 'nz': (zflag,), 'nt': (zflag, tflag)}[entry]
    rc = getattr(_lib_(), 'gpode_rollout_%s_fwd_%s' % ('dense' if dense else 'adaptive', entry))(*head, *tail, _stream())
    return rc, (zt, counts, xs, hs, ie) + ((th,) if dense else ())


def untouched(ts_):
    torch.cuda.synchronize()
    return all((torch.isnan(t).all() if t.is_floating_point() else (t == -7).all()).item() for t in ts_)


# ---- 1. fixed grid: every forward route -------------------------------------------------------------------------------------------------
def route_cases():
    """the first 'full' case of integrator_routes.TABLE for every forward route (T = 3 selects the table's input generator; the grids
    of this file have T = 4)"""
    seen = {}
    for c, route in IR.TABLE.items():
        if c.kind == 'full' and route not in seen:
            seen[route] = c._replace(T=3)
    assert set(seen) == set(IR._F)
    return [(r, seen[r]) for r in IR._F]


def dev_inputs(c):
    p, nz, z0, _, _ = IR.inputs(c)
    return ({k: v.cuda() for k, v in p.items()}, {k: v.cuda() for k, v in nz.items()}), z0


@pytest.mark.parametrize('nd', [1, 3])
@pytest.mark.parametrize('route,c', route_cases(), ids=[r for r, _ in route_cases()])
def test_fixed_grid_per_trajectory_launch_equals_grouped_shared_launches(route, c, nd):
    c = c._replace(nd=nd)
    assert IR.forward_route(c) == route
    assert (c.N > IR.TEAM_MAX_ROWS) == ('team' not in route)           # the wave routes wrap their persistent loops past 2048 rows
    dev_in, z0 = dev_inputs(c)
    cb = IR.build(c, dev_in)
    gs, rows = grids(c.N)
    for zflag, z in ((0, z0.cuda()), (1, per_draw(z0, nd, 7))):
        rc, got = raw_fwd(cb, nd, z, rows, c.order, c.method, 'nt', zflag, 1)
        assert rc == 0 and _tag() == 'rollout_' + route, (_err(), _tag())
        assert not torch.isnan(got[0]).any() and not torch.isnan(got[1]).any()
        shared = []
        for g in range(3):
            rc, out = raw_fwd(cb, nd, z, gs[g], c.order, c.method, 'nz', zflag)
            assert rc == 0 and _tag() == 'rollout_' + route
            shared.append(out)
        for name, a, b in zip(('zt', 'xstage'), got, deal(shared)):
            assert bits(a, b), (route, nd, 'z0_per_draw', zflag, name)
        assert not bits(shared[0][0], shared[1][0])                     # the grids do differ in what they give
        # the flag: 0 is the twin's launch; 1 on N copies of one grid is the shared launch
        rc, out = raw_fwd(cb, nd, z, gs[1], c.order, c.method, 'nt', zflag, 0)
        assert rc == 0 and _tag() == 'rollout_' + route and all(bits(a, b) for a, b in zip(out, shared[1]))
        rc, out = raw_fwd(cb, nd, z, gs[1][None].expand(c.N, -1).contiguous(), c.order, c.method, 'nt', zflag, 1)
        assert rc == 0 and all(bits(a, b) for a, b in zip(out, shared[1])), (route, 'N copies of one grid')
    if nd == 1:                                                         # the `_n` entry point forwards with 0 as well
        rc, out = raw_fwd(cb, 1, z0.cuda(), gs[2], c.order, c.method, 'n')
        rc2, out2 = raw_fwd(cb, 1, z0.cuda(), gs[2], c.order, c.method, 'nt', 0, 0)
        assert rc == 0 and rc2 == 0 and all(bits(a, b) for a, b in zip(out, out2))


# ---- 2. refusals ------------------------------------------------------------------------------------------------------------------------
def test_any_other_flag_is_refused_with_nothing_written():
    from vae_gp_ode_amd import ops
    from vae_gp_ode_amd.ops import KERNEL_ID, _ptr, _stream
    c = IR.Case('RBF', 6, 6, 1, 16, 32, 5, 3, 'rk4', 1, 'fused')
    dev_in, z0 = dev_inputs(c)
    cb = IR.build(c, dev_in)
    gs, rows = grids(c.N)
    z = z0.cuda()
    for flag in (2, -1):
        rc, out = raw_fwd(cb, 1, z, rows, 1, 'rk4', 'nt', 0, flag)
        assert rc != 0 and _err().startswith('gpode_rollout_fwd_nt:') and 'ts_per_traj' in _err() and untouched(out), _err()
        for dense, name in ((False, 'gpode_rollout_adaptive_fwd_nt'), (True, 'gpode_rollout_dense_fwd_nt')):
            rc, out = raw_adaptive(cb, 1, z, rows, 1, 12, dense, 'nt', 0, flag)
            assert rc != 0 and _err().startswith(name + ':') and 'ts_per_traj' in _err() and untouched(out), _err()
        xs, gzt = torch.randn(1, c.N, T - 1, 4, 6).cuda(), torch.randn(1, c.N, T, 6).cuda()
        rc, out = raw_bwd(cb, 1, xs, gzt, rows, 1, 'rk4', 'nt', flag)
        assert rc != 0 and 'ts_per_traj' in _err() and untouched(out), _err()
        nch = ops.pgrad_chunks(cb, c.N, 1, 'rk4', force=True)
        pf = cb.pack.shape[-1]
        gz0, ast, slab, gpack = nan(1, c.N, 6), nan(1, c.N, T - 1, 4, 6), nan(nch * pf), nan(1, pf)
        rc = _lib_().gpode_rollout_bwd_pgrad_nt(KERNEL_ID['RBF'], 1, 1, 6, 6, cb.M, cb.S, 1, _ptr(cb.pack), _ptr(xs), _ptr(gzt), _ptr(rows), c.N, T,
                                                _ptr(gz0), _ptr(ast), _ptr(slab), nch, _ptr(gpack), flag, _stream())
        assert rc != 0 and 'ts_per_traj' in _err() and untouched((gz0, ast, slab, gpack)), _err()
    # and the calls the refusals were variations of go through
    assert raw_fwd(cb, 1, z, rows, 1, 'rk4', 'nt', 0, 1)[0] == 0 and raw_adaptive(cb, 1, z, rows * 4, 1, 12, True, 'nt', 0, 1)[0] == 0
    # through ops: rows that are not the trajectories'
    with pytest.raises(ops._lib.GpodeError, match='ts must be'):
        ops.rollout(cb, z, rows[:4].contiguous(), 1, 'rk4')
    with pytest.raises(ops._lib.GpodeError, match='ts must be'):
        ops.rollout(cb, z, rows[:4].contiguous(), 1, 'dopri5')


# ---- 3. reverse sweep -------------------------------------------------------------------------------------------------------------------
def sweep_cases():
    """per solver the first 'full' case of the table on either side of integrator_routes.backward_resident"""
    seen = {}
    for c in IR.TABLE:
        key = (c.method, IR.backward_resident(c))
        if c.kind == 'full' and key not in seen:
            seen[key] = c._replace(T=3, nd=2)
    assert len(seen) == 6, sorted(seen)
    return [seen[k] for k in sorted(seen)]


@pytest.mark.parametrize('c', sweep_cases(), ids=['%s-%s' % (c.method, 'resident' if IR.backward_resident(c) else 'streamed') for c in sweep_cases()])
def test_reverse_sweep_per_trajectory_launch_equals_grouped_shared_launches(c):
    dev_in, z0 = dev_inputs(c)
    cb = IR.build(c, dev_in)
    gs, rows = grids(c.N)
    want = 'rollout_bwd_%s%s' % (c.kernel.lower(), '' if IR.backward_resident(c) else '_stream')
    rc, (zt, xs) = raw_fwd(cb, c.nd, z0.cuda(), rows, c.order, c.method, 'nt', 0, 1)
    assert rc == 0
    gzt = torch.randn(c.nd, c.N, T, c.Di, generator=torch.Generator().manual_seed(5)).cuda()
    rc, got = raw_bwd(cb, c.nd, xs, gzt, rows, c.order, c.method, 'nt', 1)
    assert rc == 0 and _tag() == want, (_err(), _tag(), want)
    assert not torch.isnan(got[0]).any() and not torch.isnan(got[1]).any()
    shared = []
    for g in range(3):
        rc, out = raw_bwd(cb, c.nd, xs, gzt, gs[g], c.order, c.method, 'n')      # rows are independent: the record of the one launch serves
        assert rc == 0 and _tag() == want
        shared.append(out)
    for name, a, b in zip(('gz0', 'astage'), got, deal(shared)):
        assert bits(a, b), (IR.case_id(c), name)
    assert not bits(shared[0][0], shared[1][0])
    rc, out = raw_bwd(cb, c.nd, xs, gzt, gs[1], c.order, c.method, 'nt', 0)
    assert rc == 0 and all(bits(a, b) for a, b in zip(out, shared[1]))
    rc, out = raw_bwd(cb, c.nd, xs, gzt, gs[1][None].expand(c.N, -1).contiguous(), c.order, c.method, 'nt', 1)
    assert rc == 0 and all(bits(a, b) for a, b in zip(out, shared[1]))


@pytest.mark.parametrize('c', [c for c in IR.TABLE if c.kind == 'fused'], ids=[c.method for c in IR.TABLE if c.kind == 'fused'])
def test_fused_reverse_sweep_with_a_grid_per_trajectory(c):
    from vae_gp_ode_amd import _lib, ops
    from vae_gp_ode_amd.ops import KERNEL_ID, METHOD_ID, _ptr, _stream
    c = c._replace(T=3)
    dev_in, z0 = dev_inputs(c)
    cb = IR.build(c, dev_in)
    gs, rows = grids(c.N)
    rc, (zt, xs) = raw_fwd(cb, 1, z0.cuda(), rows, c.order, c.method, 'nt', 0, 1)
    assert rc == 0
    gzt = torch.randn(1, c.N, T, c.Di, generator=torch.Generator().manual_seed(6)).cuda()
    rc, (gz0, ast) = raw_bwd(cb, 1, xs, gzt, rows, c.order, c.method, 'nt', 1)
    assert rc == 0
    nch = ops.pgrad_chunks(cb, c.N, c.order, c.method, force=True)
    assert nch == min(c.N, 2048)
    fz, fa, fg = ops.rollout_bwd_pgrad(cb, xs[0], gzt[0], rows, c.order, c.method, nch)
    assert _tag() == 'reduce_slab'
    assert bits(fz, gz0[0]) and bits(fa, ast[0])
    # the flag through the entry point itself: 0 on a shared grid is the twin
    a = ops.rollout_bwd_pgrad(cb, xs[0], gzt[0], gs[0], c.order, c.method, nch)
    pf = cb.pack.shape[-1]
    o = [nan(c.N, c.Di), nan(c.N, T - 1, IR.NSTAGE[c.method], c.Do), nan(nch * pf), nan(pf)]
    _lib.call('gpode_rollout_bwd_pgrad_nt', KERNEL_ID[c.kernel], c.order, METHOD_ID[c.method], c.Di, c.Do, c.M, c.S, 1, _ptr(cb.pack), _ptr(xs),
              _ptr(gzt), _ptr(gs[0]), c.N, T, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), nch, _ptr(o[3]), 0, _stream())
    assert bits(o[0], a[0]) and bits(o[1], a[1]) and bits(o[3], a[2])
    # the parameter sums: the separate launch over the same rows
    R = c.N * (T - 1) * IR.NSTAGE[c.method]
    sep = ops.param_grad(cb, xs[0].reshape(R, c.Di), ast[0].reshape(R, c.Do))
    cache = IR.cache_dicts(c, cb, dev_in)
    lf, ls = IR.unpack(c, fg.view(1, -1).cpu(), cache), IR.unpack(c, sep.view(1, -1).cpu(), cache)
    for k in lf:
        e = relerr(lf[k], ls[k])
        print('fused %s: d/d %s %.2e from the separate parameter sums, bound %.2e' % (c.method, k, e, IR.bound(k, 0.0)))
        assert e <= IR.bound(k, 0.0), (k, e)


# ---- 4. against the fp64 oracle ----------------------------------------------------------------------------------------------------------
ORACLE_CASES = [IR.R_(16, 16, 1, 40, 64, 5, 'rk4'), IR.R_(6, 6, 1, 64, 64, 2049, 'rk4'), IR.D_(6, 128, 384, 5, 'rk4'),
                IR.D_(4, 16, 64, 2049, 'euler')]


@pytest.mark.parametrize('c', ORACLE_CASES, ids=[IR.TABLE[c] for c in ORACLE_CASES])
def test_against_the_fp64_oracle_group_by_group(c):
    assert ('team' in IR.TABLE[c]) == (c.N <= IR.TEAM_MAX_ROWS)
    dev_in, z0 = dev_inputs(c)
    cb = IR.build(c, dev_in)
    cache = IR.cache_dicts(c, cb, dev_in)
    gs, rows = grids(c.N)
    gw = torch.randn(1, c.N, T, c.Di, generator=torch.Generator().manual_seed(8))
    rc, (zt, xs) = raw_fwd(cb, 1, z0.cuda(), rows, c.order, c.method, 'nt', 0, 1)
    assert rc == 0 and _tag() == 'rollout_' + IR.TABLE[c]
    rc, (gz0, ast) = raw_bwd(cb, 1, xs, gw.cuda(), rows, c.order, c.method, 'nt', 1)
    assert rc == 0
    got = dict(zt=zt.cpu(), xstage=xs.cpu(), gz0=gz0.cpu(), astage=ast.cpu())
    c4 = c._replace(T=T)
    for g in range(3):
        idx = torch.arange(g, c.N, 3)
        ts = torch.tensor(G[g])
        r64, r32 = (IR.reference(c4, cache, dt, z0=z0[idx], ts=ts, gw=gw[:, idx]) for dt in (torch.float64, torch.float32))
        for key in ('zt', 'xstage', 'gz0', 'astage'):
            e, e32 = relerr(got[key][:, idx], r64[key]), relerr(r32[key], r64[key])
            print('%s grid %d: %s %.2e from fp64 (fp32 oracle %.2e, bound %.2e)' % (IR.TABLE[c], g, key, e, e32, IR.bound(key, e32)))
            assert e <= IR.bound(key, e32), (IR.TABLE[c], g, key, e)


# ---- 5. dopri5, landing and dense -------------------------------------------------------------------------------------------------------
SCALE = 4.0                                          # intervals long enough for more than one step each
NAMES = ('zt', 'counts', 'xstage', 'hstep', 'iend', 'theta')


@pytest.mark.parametrize('dense', [False, True], ids=['landing', 'dense'])
@pytest.mark.parametrize('N', [5, 2049])
@pytest.mark.parametrize('kernel,Di,Do,M,S', [('RBF', 6, 6, 24, 32), ('DF', 4, 4, 16, 32)], ids=['rbf', 'df'])
def test_dopri5_per_trajectory_launch_equals_grouped_shared_launches(kernel, Di, Do, M, S, N, dense):
    from vae_gp_ode_amd import ops
    cb, z0, want, want_bwd = _dopri5_setup(None, kernel, Di, Do, M, S, N, None)       # a cache of 3 draws
    nd, K = cb.nd, 4 * (T - 1)
    gs, rows = grids(N, SCALE)
    z = z0.cuda()
    rc, got = raw_adaptive(cb, nd, z, rows, 1, K, dense, 'nt', 0, 1)
    assert rc == 0 and _tag() == want, (_err(), _tag(), want)
    status = got[1][..., 2]
    print('%s N=%d %s: accepted %d..%d, status counts %s' % (kernel, N, 'dense' if dense else 'landing', int(got[1][..., 0].min()),
                                                             int(got[1][..., 0].max()), torch.bincount(status.flatten()).tolist()))
    assert int(status.max()) == 0 and not torch.isnan(got[0]).any() and int(got[1][..., 0].max()) > T - 1
    shared = []
    for g in range(3):
        rc, out = raw_adaptive(cb, nd, z, gs[g], 1, K, dense, 'nz', 0)
        assert rc == 0 and _tag() == want
        shared.append(out)
    for name, a, b in zip(NAMES, got, deal(shared)):
        assert bits(a, b), (kernel, N, dense, name)
    assert not bits(shared[0][0], shared[1][0])
    rc, out = raw_adaptive(cb, nd, z, gs[1], 1, K, dense, 'nt', 0, 0)
    assert rc == 0 and all(bits(a, b) for a, b in zip(out, shared[1]))
    rc, out = raw_adaptive(cb, nd, z, gs[1][None].expand(N, -1).contiguous(), 1, K, dense, 'nt', 0, 1)
    assert rc == 0 and all(bits(a, b) for a, b in zip(out, shared[1]))
    # through ops, with the reverse sweep on the record
    gzt = torch.randn(nd, N, T, Di, generator=torch.Generator().manual_seed(60 + N)).cuda()

    def solve(ts):
        rec = ops.rollout_adaptive(cb, z, ts, 1, 1e-4, 1e-4, K, save_stages=True, dense=dense)
        assert _tag() == want
        bwd = ops.rollout_adaptive_bwd(cb, rec[2], rec[3], rec[4], gzt, 1, theta=rec[5] if dense else None)
        assert _tag() == want_bwd
        return rec, bwd
    rec, bwd = solve(rows)
    assert all(bits(a, b) for a, b in zip(rec, got))
    assert not torch.isnan(bwd[0]).any() and not torch.isnan(bwd[1]).any()
    for name, a, b in zip(('gz0', 'astage'), bwd, deal([solve(gs[g])[1] for g in range(3)])):
        assert bits(a, b), (kernel, N, dense, name)
    assert bits(ops.rollout_adaptive(cb, z, rows, 1, 1e-4, 1e-4, K, dense=dense)[0], got[0])     # without the record
    # one row that is not increasing: its second interval is empty
    bad_n = 1 if N == 5 else 1030
    bad = rows.clone()
    bad[bad_n, 2] = bad[bad_n, 1]
    with pytest.raises(ops._lib.GpodeError, match='strictly increasing'):
        ops.rollout_adaptive(cb, z, bad, 1, 1e-4, 1e-4, K, dense=dense)
    rc, out = raw_adaptive(cb, nd, z, bad, 1, K, dense, 'nt', 0, 1)
    assert rc == 0
    others = (torch.arange(N) != bad_n).cuda()
    for name, a, b in zip(NAMES, out, got):
        assert bits(a[:, others], b[:, others]), (kernel, N, dense, name, 'a trajectory next to the bad row changed')
    first = 1 if dense else 2                        # dense: nothing is integrated; landing: the first interval is, the second is refused
    assert (out[1][:, bad_n, 2] == 3).all()
    assert torch.isnan(out[0][:, bad_n, first:]).all() and bits(out[0][:, bad_n, :first], got[0][:, bad_n, :first])
    assert bits(out[0][:, bad_n, 0], z[bad_n][None].expand(nd, -1).contiguous())


# ---- 6. ops.flow ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('draws', [None, 3])
@pytest.mark.parametrize('method,adaptive', [('rk4', None), ('dopri5', (1e-4, 1e-4, 64, None, False)), ('dopri5', (1e-4, 1e-4, 64, None, True))],
                         ids=['rk4', 'dopri5', 'dopri5-dense'])
def test_flow_with_equal_rows_is_the_shared_grid_flow(method, adaptive, draws):
    from test_gpu_draws import _noise
    from vae_gp_ode_amd import ops
    m = _tiny_model('RBF', 1, 6)
    gp = m.flow.odefunc.diffeq
    N, D = 5, 6
    nzs = [{k: v[0].cuda() for k, v in _noise('RBF', D, D, 16, 32, 1, 30 + l).items()} for l in range(draws or 1)]
    g = torch.Generator().manual_seed(31)
    z0 = torch.randn(N, D, generator=g).cuda()
    W = torch.randn(*((draws,) if draws else ()), N, T, D, generator=g).cuda()
    ts = torch.tensor(G[1]).cuda() * (SCALE if method == 'dopri5' else 1.0)
    params = [p for p in gp.parameters() if p.requires_grad]
    assert len(params) == 5

    def run(ts_):
        for p in params:
            p.grad = None
        gp._next_noise.clear(); gp.set_noise(*nzs)
        z = z0.clone().requires_grad_(True)
        zt = ops.flow(gp, z, ts_, 1, method, draws=draws, adaptive=adaptive)
        (zt * W).sum().backward()
        return zt.detach(), z.grad, [p.grad.clone() for p in params]
    za, ga, pa = run(ts)
    zb, gb, pb = run(ts[None].expand(N, -1))                             # not contiguous: ops makes it so
    assert bits(za, zb) and bits(ga, gb) and ga.abs().max().item() > 0
    for a, b, p in zip(pa, pb, params):
        assert bits(a, b) and a.abs().max().item() > 0, tuple(p.shape)
    # the module: Flow.forward takes either, and counts its evaluations from the last axis
    m.flow.solver, m.flow.rtol, m.flow.atol, m.flow.max_steps = method, 1e-4, 1e-4, 64
    gp._next_noise.clear(); gp.set_noise(*nzs[:1])
    z1 = m.flow(z0, ts)
    gp._next_noise.clear(); gp.set_noise(*nzs[:1])
    z2 = m.flow(z0, ts[None].expand(N, -1))
    assert bits(z1, z2) and (method == 'dopri5' or m.flow.num_evals() == 4 * (T - 1))


@pytest.mark.parametrize('solver', ['rk4', 'dopri5'])
def test_zero_padded_width_passes_the_grid_through(solver):
    """a latent width outside the compiled list runs on zero-padded operands (ops.WidthPad): the grid goes through as it is"""
    from test_gpu_draws import _noise
    m = _tiny_model('RBF', 1, 5, solver)
    m.flow.rtol, m.flow.atol, m.flow.max_steps = 1e-4, 1e-4, 64
    gp = m.flow.odefunc.diffeq
    assert gp.width_pad is not None
    N = 7
    nz = {k: v[0].cuda() for k, v in _noise('RBF', 5, 5, 16, 32, 1, 40).items()}
    z0 = torch.randn(N, 5, generator=torch.Generator().manual_seed(41)).cuda()
    gs, rows = grids(N, SCALE if solver == 'dopri5' else 1.0)

    def run(ts):
        gp._next_noise.clear(); gp.set_noise(nz)
        z = z0.clone().requires_grad_(True)
        zt = m.flow(z, ts)
        zt.square().sum().backward()
        return zt.detach(), z.grad
    got = run(rows)
    assert tuple(got[0].shape) == (N, T, 5) and not torch.isnan(got[0]).any() and got[1].abs().max().item() > 0
    shared = [run(gs[g]) for g in range(3)]
    for i, name in enumerate(('zt', 'dL/dz0')):
        want = torch.empty_like(shared[0][i])
        for g in range(3):
            want[g::3] = shared[g][i][g::3]
        assert bits(got[i], want), (solver, name)
    assert not bits(shared[0][0], shared[1][0])


def oracle_bound(key, e32):
    """the bound of test_gpu_backward.test_streamed_backward_matches_fp64_oracle, which states it inline: 2e-4 + 3 relerr(fp32 oracle, fp64)
    for the trajectories, 1e-3 + 3 relerr(fp32 oracle, fp64) for every gradient"""
    return (2e-4 if key == 'zt' else 1e-3) + 3 * e32


@pytest.mark.parametrize('kernel,Di,Do,order,M,S,method', [('RBF', 6, 6, 1, 24, 32, 'rk4'), ('DF', 4, 4, 1, 16, 32, 'rk4'),
                                                           ('RBF', 6, 3, 2, 24, 32, 'midpoint'), ('RBF', 6, 6, 1, 160, 64, 'euler')])
def test_flow_gradients_with_distinct_rows_match_the_fp64_oracle(kernel, Di, Do, order, M, S, method):
    from oracle import gpode_oracle as O
    from vae_gp_ode_amd.model.core.flow import Flow
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    N = 7
    p, nz, z0, _, gw = synthetic_gp(kernel, Di, Do, M, S, N, T, seed=2000 + M + S + Di)
    gp = SVGP_Layer(Di, Do, M, S, kernel=kernel).cuda()
    with torch.no_grad():
        gp.kern.unconstrained_lengthscales.copy_(p['raw_ell'])
        gp.kern.unconstrained_variance.copy_(p['raw_var'])
        gp.inducing_loc.optvar.copy_(p['Z'])
        gp.Um.optvar.copy_(p['Um'])
        gp.Us_sqrt.optvar.copy_(p['Us'])
    flow = Flow(gp, order=order, solver=method).cuda()
    gp.set_noise({k: v.cuda() for k, v in nz.items()})
    _, rows = grids(N)
    zg = z0.cuda().requires_grad_(True)
    zt = flow(zg, rows)
    (zt * gw.cuda()).sum().backward()
    got = {'raw_ell': gp.kern.unconstrained_lengthscales.grad, 'raw_var': gp.kern.unconstrained_variance.grad,
           'Z': gp.inducing_loc.optvar.grad, 'Um': gp.Um.optvar.grad, 'Us': gp.Us_sqrt.optvar.grad, 'z0': zg.grad}

    def oracle(dtype):
        q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items()}
        c = O.build_cache(q, O.to_dtype(nz, dtype), kernel)
        z = z0.to(dtype).clone().requires_grad_(True)
        out, loss = torch.zeros(N, T, Di, dtype=dtype), 0.0
        for g in range(3):                           # one oracle run per grid group, the losses summed
            idx = torch.arange(g, N, 3)
            o = O.flow_forward(z[idx], torch.tensor(G[g], dtype=dtype), c, order, method)
            loss = loss + (o * gw[idx].to(dtype)).sum()
            out[idx] = o.detach()
        loss.backward()
        return out, dict({k: v.grad for k, v in q.items()}, z0=z.grad)
    z64, g64 = oracle(torch.float64)
    z32, g32 = oracle(torch.float32)
    assert relerr(zt, z64) < oracle_bound('zt', relerr(z32, z64))
    for k in got:
        e, tol = relerr(got[k], g64[k]), oracle_bound(k, relerr(g32[k], g64[k]))
        print('%s %s d/d %s: %.2e (bound %.2e)' % (kernel, method, k, e, tol))
        assert e < tol, (k, e, tol)
    # a grid dealt to the wrong trajectories would be seen: the first two rows exchanged is another result
    swapped = rows.clone()
    swapped[0], swapped[1] = rows[1], rows[0]
    gp.set_noise({k: v.cuda() for k, v in nz.items()})
    with torch.no_grad():
        assert relerr(flow(z0.cuda(), swapped)[:2], z64[:2]) > 10 * oracle_bound('zt', relerr(z32, z64))


# ---- 7. the model -----------------------------------------------------------------------------------------------------------------------
def tiny_model(**kw):
    from vae_gp_ode_amd.model.core.initialization import initialize_and_fix_kernel_parameters
    from vae_gp_ode_amd.model.core.noise import install_device_noise
    from vae_gp_ode_amd.model.create_model import build_model
    torch.manual_seed(13)
    m = build_model(model_args(**kw)).cuda()
    initialize_and_fix_kernel_parameters(m, 2.0, 1.0, fix=False)
    return m, install_device_noise(m, 17)


@pytest.mark.parametrize('kw', [dict(), dict(ode=2, D_in=6, D_out=3, latent_dim=3, frames=3), dict(kernel='DF', solver='dopri5')],
                         ids=['rbf1', 'rbf2', 'df-dopri5'])
def test_model_with_the_uniform_grid_spelt_out_is_the_model_without_a_grid(kw):
    from vae_gp_ode_amd import evaluate as E
    from vae_gp_ode_amd.data.utils import subsample_frames
    from vae_gp_ode_amd.model.create_model import compute_loss
    m, src = tiny_model(**kw)
    m.flow.rtol, m.flow.atol, m.flow.max_steps = 1e-4, 1e-4, 64
    N, Tm = 4, 5
    X = torch.rand(N, Tm, 1, 28, 28, generator=torch.Generator().manual_seed(14)).cuda()
    uniform = (m.dt * torch.arange(Tm, dtype=torch.float, device='cuda')).expand(N, Tm)
    for L in (1, 3):
        src.manual_seed(17)
        a = compute_loss(m, X, L)
        src.manual_seed(17)
        b = compute_loss(m, X, L, ts=uniform)
        assert all(bits(x.detach(), y.detach()) for x, y in zip(a, b)), L
        assert all(torch.isfinite(x).all() for x in a)
    for kwargs in (dict(L=3), dict(L=3, T_custom=2 * Tm), dict(L=2, variance=False, loglik=True)):
        Th = kwargs.get('T_custom', Tm)
        grid = (m.dt * torch.arange(Th, dtype=torch.float, device='cuda')).expand(N, Th)
        src.manual_seed(17)
        pa = E.predict(m, X, **kwargs)
        src.manual_seed(17)
        pb = E.predict(m, X, ts=grid, **kwargs)
        assert pa.state == pb.state and pa.mse == pb.mse and torch.equal(pa.mse_t, pb.mse_t)
        if pa.mean is not None:
            assert bits(pa.mean, pb.mean) and bits(pa.var, pb.var)
        if pa.ll is not None:
            assert torch.equal(pa.ll, pb.ll) and pa.nlpd == pb.nlpd and torch.equal(pa.nll_t, pb.nll_t)
    src.manual_seed(17)
    ma = E.predict_marginal(m, X, 3)
    src.manual_seed(17)
    mb = E.predict_marginal(m, X, 3, ts=uniform)
    assert torch.equal(ma.ll, mb.ll) and torch.equal(ma.lw, mb.lw) and ma.iw_nll == mb.iw_nll and ma.state == mb.state
    # a subsampled grid: another loss, finite, and the gradient reaches the GP parameters
    lead = 1 if m.order == 1 else m.v_steps
    gen = torch.Generator(device='cuda').manual_seed(2)
    for _ in range(32):                              # order 2 draws one frame of two per sequence: 1 in 16 subsets is the first four frames
        Xs, idx = subsample_frames(X, 4, lead, gen)
        if not torch.equal(idx, torch.arange(4, device='cuda').expand(N, 4)):
            break
    ts = m.dt * idx.float()
    assert not torch.equal(idx, torch.arange(4, device='cuda').expand(N, 4))
    src.manual_seed(17)
    s = compute_loss(m, Xs, 1, ts=ts)
    src.manual_seed(17)
    u = compute_loss(m, Xs, 1)
    assert all(torch.isfinite(x).all() for x in s) and not bits(s[0].detach(), u[0].detach())
    s[0].backward()
    gU = m.flow.odefunc.diffeq.Um.optvar.grad
    assert torch.isfinite(gU).all() and gU.abs().max().item() > 0
    # the loaders of evaluate: an item (X, ts) is evaluated on its grid
    src.manual_seed(17)
    want = E.predict(m, Xs, 2, variance=False, loglik=True, ts=ts)
    src.manual_seed(17)
    nll, nlpd = E.compute_nll(m, [(Xs, ts)], 2)
    assert nll == want.nll and nlpd == want.nlpd
    src.manual_seed(17)
    assert E.compute_mse_std(m, [(Xs, ts)], 2) == (want.mse, want.std)
    with pytest.raises(ValueError, match='ts must be'):
        E.predict(m, Xs, 2, ts=ts[:3])
    with pytest.raises(ValueError, match='ts must be'):
        compute_loss(m, Xs, 1, ts=ts[:, :3])


@pytest.mark.parametrize('solver', ['rk4'])
def test_graph_replay_reads_the_grids_from_a_static_buffer(solver):
    """test_gpu_optim.test_graph_replay_equals_eager_steps with a grid per sequence: the captured step reads X and ts from static
    buffers; one eager warm-up step and two replays -- the second after both buffers were refreshed -- equal three eager steps on the same
    noise counter, bit for bit."""
    from vae_gp_ode_amd.data.utils import subsample_frames
    from vae_gp_ode_amd.graph import GraphedStep
    from vae_gp_ode_amd.model.create_model import compute_loss
    from vae_gp_ode_amd.optim import HipAdam
    m, src = tiny_model(solver=solver)
    m.flow.rtol, m.flow.atol, m.flow.max_steps = 1e-4, 1e-4, 64
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

    def run(use_graph):
        m.load_state_dict(init)
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
        for i, b in enumerate(order):
            buf.copy_(batches[b][0]); tbuf.copy_(batches[b][1])
            if not use_graph:
                losses.append(step().detach().clone())
            elif gs is None:
                gs = GraphedStep(step, warmup=1)
                losses.append(gs.warm_out.clone())
            else:
                losses.append(gs().clone())
            if solver == 'dopri5':
                cnt = m.flow.last_counts
                print('%s step %d: loss %.6g, accepted %d..%d, status %s' % ('graph' if use_graph else 'eager', i, losses[-1].item(), int(cnt[..., 0].min()),
                                                                             int(cnt[..., 0].max()), cnt[..., 2].tolist()))
        torch.cuda.synchronize()
        return losses, [p.detach().clone() for p in m.parameters()]
    le, pe = run(False)
    lg, pg = run(True)
    assert all(torch.isfinite(x).all() for x in le)
    assert all(bits(a, b) for a, b in zip(le, lg)), ([x.item() for x in le], [x.item() for x in lg])
    assert all(bits(a, b) for a, b in zip(pe, pg))
    assert not bits(le[1], le[2])


# ---- 8. the command lines ---------------------------------------------------------------------------------------------------------------
def test_main_trains_on_subsampled_sequences(tmp_path, monkeypatch):
    """test_gpu_optim.test_main_training_loop_runs's configuration with --subsample_frames 4 --T 6: two steps, eagerly and replayed"""
    from vae_gp_ode_amd import main as M
    from vae_gp_ode_amd import ops, vae_ops
    monkeypatch.chdir(tmp_path)
    common = ['--task', 'synthetic', '--Ndata', '8', '--Ntest', '4', '--batch', '4', '--T', '6', '--solver', 'rk4', '--num_inducing', '16',
              '--num_features', '32', '--lr', '1e-4', '--log_freq', '1', '--Nepoch', '1', '--subsample_frames', '4']
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
            assert 'keeps 4 of its frames' in log
    finally:                                         # process-wide switches the training loop sets for itself
        ops.set_overlap(False)
        vae_ops.set_deferred_reductions(False)
    for bad in ('7', '1'):
        with pytest.raises(SystemExit, match='--subsample_frames ' + bad):
            M.main(common[:-1] + [bad, '--save', 'results/x'])


def test_evaluate_on_subsampled_sequences(tmp_path, capsys):
    from vae_gp_ode_amd import evaluate as E
    from vae_gp_ode_amd.model.create_model import build_model
    from vae_gp_ode_amd.model.misc.torch_utils import seed_everything
    argv = ['--task', 'synthetic', '--Ndata', '8', '--Ntest', '6', '--batch', '4', '--T', '6', '--solver', 'rk4', '--num_inducing', '16',
            '--num_features', '32', '--model_path', str(tmp_path), '--eval_sample_size', '4', '--Troll', '2', '--save', str(tmp_path / 'ev'),
            '--device_noise', 'True', '--eval_z0_draws', 'True']
    args = E.make_parser().parse_args(argv)
    args.device = torch.device('cuda')
    seed_everything(3)
    torch.save(build_model(args).to(args.device).state_dict(), tmp_path / 'odegpvae_mnist.pth')
    plain = E.main(argv)
    sub = E.main(argv + ['--subsample_frames', '4'])
    again = E.main(argv + ['--subsample_frames', '4'])
    out = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')][-1])
    assert out == json.loads(json.dumps(again)) and sub['subsample_frames'] == 4 and 'subsample_frames' not in plain
    assert sub['T'] == 4 and len(sub['mse_t']) == 4 and len(sub['nll_t']) == 4 and plain['T'] == 6
    assert sub['rollout_T'] == plain['rollout_T'] == 12                 # the long roll-out stays on all frames and the uniform grid
    assert all(math.isfinite(sub[k]) for k in ('mse', 'std', 'nll', 'nlpd', 'iw_nll', 'ess_mean')) and sub['mse'] != plain['mse']
    assert {k: v for k, v in sub.items() if k != 'ms'} == {k: v for k, v in again.items() if k != 'ms'}      # reproducible from --seed
    with pytest.raises(SystemExit, match='--subsample_frames'):
        E.main(argv + ['--subsample_frames', '9'])
