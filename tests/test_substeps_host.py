"""Host side of the sub-steps of the fixed-grid solvers: the helper the GPU tests lean on (substeps_ref.refine), the `_ns` entry points in
the header and in _lib.SIGNATURES, the meaning of --ts_dense_scale, Flow's evaluation count, and the checks ops makes before it calls
the library."""
import os
import re
import types

import pytest
import torch

from substeps_ref import T_EXACT, exact_grids, refine, scatter_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = {'gpode_rollout_fwd_ns': 'gpode_rollout_fwd_nt', 'gpode_rollout_bwd_ns': 'gpode_rollout_bwd_nt',
      'gpode_rollout_bwd_pgrad_ns': 'gpode_rollout_bwd_pgrad_nt'}


# ---- refine ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s', [1, 2, 3, 4, 7, 64])
def test_refine_is_linspace_in_every_interval(s):
    g = torch.Generator().manual_seed(s)
    for ts in (torch.tensor([0.0, 0.05, 0.2]), torch.cumsum(torch.rand(6, generator=g, dtype=torch.float64) + 0.01, 0),
               torch.cumsum(torch.rand(5, 4, generator=g, dtype=torch.float64) + 0.01, 1)):
        fine = refine(ts, s)
        T = ts.shape[-1]
        assert fine.dtype == ts.dtype and tuple(fine.shape) == tuple(ts.shape[:-1]) + ((T - 1) * s + 1,)
        assert torch.equal(fine[..., ::s], ts)                              # the output times are kept as they are
        rows, frows = ts.reshape(-1, T), fine.reshape(-1, fine.shape[-1])
        for row, frow in zip(rows, frows):
            for j in range(T - 1):
                want = torch.linspace(row[j].item(), row[j + 1].item(), s + 1, dtype=torch.float64)[:-1]
                assert torch.allclose(frow[j * s:(j + 1) * s].double(), want, rtol=1e-6 if ts.dtype == torch.float32 else 1e-13, atol=0)
        assert (frows[:, 1:] > frows[:, :-1]).all()
    assert torch.equal(refine(ts, 1), ts)
    with pytest.raises(ValueError):
        refine(ts, 0)


@pytest.mark.parametrize('s', [2, 4])
def test_the_exact_grids_refine_without_rounding(s):
    """what the bit-for-bit GPU tests rely on: every gap of the refined grid is the float32 quotient gap / s, exactly, and it is the gap
    the refined grid's own entries give back"""
    for name, ts in exact_grids(5).items():
        fine = refine(ts, s)
        assert torch.equal(fine.double(), refine(ts.double(), s)), name      # no rounding on the way
        h = ((ts[..., 1:] - ts[..., :-1]) / float(s))[..., None].expand(ts.shape[:-1] + (T_EXACT - 1, s)).reshape(ts.shape[:-1] + (-1,))
        assert torch.equal(fine[..., 1:] - fine[..., :-1], h), name
        assert torch.equal(fine * 128, (fine * 128).round()), name           # small multiples of 2^-7
    u = refine(0.25 * torch.arange(6, dtype=torch.float32), s)
    assert torch.equal(u[1:] - u[:-1], torch.full((5 * s,), 0.25 / s))


def test_scatter_frames():
    g = torch.arange(2 * 3 * 2, dtype=torch.float32).view(2, 3, 2) + 1
    out = scatter_frames(g, 3)
    assert tuple(out.shape) == (2, 7, 2) and torch.equal(out[:, ::3], g) and out.sum() == g.sum()
    assert torch.equal(scatter_frames(g, 1), g)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def _decl(hdr, sym):
    m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % sym, hdr)
    assert m, sym
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def test_header_declares_the_substep_entry_points():
    """each `_ns` symbol is declared, is in SIGNATURES, and takes its `_nt` twin's arguments plus `int substeps` in front of the stream;
    the block above them states the record layout and the range"""
    import ctypes
    from vae_gp_ode_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gpode.h')).read()
    for sym, twin in NS.items():
        assert sym in _lib.SIGNATURES, sym
        a, b = _decl(hdr, sym), _decl(hdr, twin)
        assert a == b[:-1] + ['int substeps', 'void* stream'], (sym, a, b)
        (res, args), (res2, args2) = _lib.SIGNATURES[sym], _lib.SIGNATURES[twin]
        assert res is res2 and args == args2[:-1] + [ctypes.c_int, ctypes.c_void_p], sym
    block = ' '.join(hdr[hdr.index('SUB-STEPS'):hdr.index('int gpode_rollout_fwd_ns')].split())
    for words in ('xstage ([L,] N, T-1, substeps, NS, D)', 'astage ([L,] N, T-1, substeps, NS, Do)', '([L,] N, (T-1)*substeps, NS, .)',
                  'substeps = 1', '1 ... 64', 'refused', 'gpode_param_grad_n', 'one fp32 division'):
        assert words in block, words
    from vae_gp_ode_amd import ops
    assert ops.MAX_SUBSTEPS == 64


# ---- --ts_dense_scale ------------------------------------------------------------------------------------------------------------------
def test_ts_dense_scale_has_the_reference_meaning():
    """compute_ts_dense places linspace(t1, t2, scale)[:-1] in every interval -- scale - 1 steps -- and leaves the grid alone up to 2"""
    from vae_gp_ode_amd import main as M
    from vae_gp_ode_amd.model.core.flow import substeps_of_dense_scale
    assert [substeps_of_dense_scale(v) for v in (0, 1, 2, 3, 4, 65)] == [1, 1, 1, 2, 3, 64]
    for scale in (3, 5):                             # the reference's grid in one interval is refine's
        dense = torch.linspace(0.1, 0.4, scale, dtype=torch.float64)[:-1]
        assert torch.allclose(refine(torch.tensor([0.1, 0.4], dtype=torch.float64), substeps_of_dense_scale(scale))[:-1], dense, rtol=1e-14)
    with pytest.raises(SystemExit, match='--ts_dense_scale 66'):
        substeps_of_dense_scale(66)
    p = M.make_parser()
    assert p.parse_args([]).ts_dense_scale == 2 and M.check_dense_scale(p.parse_args([])) == 1
    assert M.check_dense_scale(p.parse_args(['--ts_dense_scale', '3'])) == 2
    with pytest.raises(SystemExit, match='--ts_dense_scale 66'):
        M.check_dense_scale(p.parse_args(['--ts_dense_scale', '66']))


def test_build_model_reads_the_flag_and_an_old_namespace_builds_as_before():
    from vae_gp_ode_amd.model.create_model import build_model
    a = dict(D_in=6, D_out=6, num_inducing=8, num_features=16, dimwise=True, q_diag=False, device='cpu', kernel='RBF', ode=1, solver='euler',
             use_adjoint=False, frames=5, n_filt=8, latent_dim=6, Ndata=360, dt=0.1)
    assert build_model(types.SimpleNamespace(**a)).flow.substeps == 1                        # no such field: one step per interval
    for scale, want in ((1, 1), (2, 1), (3, 2), (9, 8)):
        assert build_model(types.SimpleNamespace(ts_dense_scale=scale, **a)).flow.substeps == want
    with pytest.raises(SystemExit, match='--ts_dense_scale'):
        build_model(types.SimpleNamespace(ts_dense_scale=66, **a))


def test_main_and_evaluate_refuse_the_flag_ahead_of_any_device_work(monkeypatch):
    from vae_gp_ode_amd import evaluate as E
    from vae_gp_ode_amd import main as M

    def reached(*a, **k):
        raise AssertionError('device work reached')
    monkeypatch.setattr(torch.cuda, 'is_available', reached)
    monkeypatch.setattr(M, 'init_distributed', reached)
    monkeypatch.setattr(M, 'load_data', reached)
    with pytest.raises(SystemExit, match='--ts_dense_scale 70'):
        M.main(['--ts_dense_scale', '70'])
    with pytest.raises(SystemExit, match='--ts_dense_scale 70'):
        E.main(['--ts_dense_scale', '70', '--model_path', 'nowhere'])


# ---- Flow ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('solver,per_step', [('euler', 1), ('midpoint', 2), ('rk4', 4)])
def test_flow_counts_its_evaluations(solver, per_step, monkeypatch):
    from vae_gp_ode_amd import ops
    from vae_gp_ode_amd.model.core.flow import EVALS_PER_STEP, Flow
    seen = []

    def fake_flow(gp, z0, ts, order, method, draws=None, adaptive=None, substeps=1):
        seen.append((method, substeps))
        return torch.zeros(z0.shape[0], ts.shape[-1], z0.shape[1])
    monkeypatch.setattr(ops, 'flow', fake_flow)
    assert EVALS_PER_STEP[solver] == per_step
    z0 = torch.zeros(3, 6)
    for T in (2, 5):
        for ts in (torch.arange(T).float(), torch.arange(T).float().expand(3, T)):
            assert Flow(torch.nn.Identity(), order=1, solver=solver)(z0, ts) is not None
            for s in (1, 2, 7):
                f = Flow(torch.nn.Identity(), order=1, solver=solver, substeps=s)
                f(z0, ts)
                assert f.num_evals() == per_step * (T - 1) * s, (solver, T, s)
                assert seen[-1] == (solver, s)
    assert Flow(torch.nn.Identity(), order=1, solver=solver).substeps == 1


def test_dopri5_ignores_the_count(monkeypatch):
    """as atol / rtol are ignored by the fixed grids: Flow(solver='dopri5', substeps=4) never hands the count on"""
    from vae_gp_ode_amd import ops
    from vae_gp_ode_amd.model.core.flow import Flow
    seen = []

    def fake_flow(gp, z0, ts, order, method, draws=None, adaptive=None, substeps=1):
        seen.append(substeps)
        return torch.zeros(z0.shape[0], ts.shape[-1], z0.shape[1])
    monkeypatch.setattr(ops, 'flow', fake_flow)
    Flow(torch.nn.Identity(), order=1, solver='dopri5', substeps=4)(torch.zeros(3, 6), torch.arange(4).float())
    assert seen == [1]


# ---- ops: the checks come before any library call --------------------------------------------------------------------------------------
def test_a_count_outside_the_range_is_refused_before_any_library_call(monkeypatch):
    from vae_gp_ode_amd import _lib, ops

    def reached(name, *a):
        raise AssertionError('library call %s reached' % name)
    monkeypatch.setattr(_lib, 'call', reached)
    monkeypatch.setattr(ops, '_chk', lambda t, name, shape=None: t.contiguous())     # host tensors stand in for device ones
    monkeypatch.setattr(ops, '_stream', lambda: None)
    N, T, D = 5, 4, 6
    c = ops.GPCache()
    c.kernel, c.Di, c.Do, c.M, c.S, c.nd, c.stacked, c.pack = 'RBF', D, D, 8, 16, 1, False, torch.zeros(64)
    z0, ts, gzt = torch.zeros(N, D), torch.arange(T).float(), torch.zeros(N, T, D)
    xs = torch.zeros(N, T - 1, 2, 4, D)
    gp = types.SimpleNamespace()                     # ops.flow refuses before it looks at the layer
    for bad in (0, 65, -1, 2.0, '2', None, True):
        for method in ('euler', 'midpoint', 'rk4'):
            for call in (lambda: ops.rollout(c, z0, ts, 1, method, substeps=bad),
                         lambda: ops.rollout(c, z0, ts, 1, method, save_stages=True, substeps=bad),
                         lambda: ops.rollout_bwd(c, xs, gzt, ts, 1, method, substeps=bad),
                         lambda: ops.rollout_bwd_pgrad(c, xs, gzt, ts, 1, method, 5, substeps=bad),
                         lambda: ops.flow(gp, z0, ts, 1, method, substeps=bad)):
                with pytest.raises(_lib.GpodeError, match='substeps must be an int in 1 ... 64'):
                    call()
    # dopri5 chooses its own steps: any count but 1 is refused, by every function that takes one
    for call in (lambda: ops.rollout(c, z0, ts, 1, 'dopri5', substeps=2), lambda: ops.rollout_bwd(c, (xs,), gzt, ts, 1, 'dopri5', substeps=2),
                 lambda: ops.rollout_bwd_pgrad(c, xs, gzt, ts, 1, 'dopri5', 5, substeps=2), lambda: ops.flow(gp, z0, ts, 1, 'dopri5', substeps=2)):
        with pytest.raises(_lib.GpodeError, match='dopri5'):
            call()
    # a record that is not the sub-step record is refused as well
    with pytest.raises(_lib.GpodeError, match='xstage'):
        ops.rollout_bwd(c, torch.zeros(N, T - 1, 4, D), gzt, ts, 1, 'rk4', substeps=2)


def test_the_calls_reach_the_entry_points_they_should(monkeypatch):
    """substeps = 1 goes where it went (`_n`, `_nz`, `_nt`), launch for launch; any other count goes to `_ns` with the flags of `_nt` and
    the count in front of the stream, and the record carries the sub-step axis"""
    from vae_gp_ode_amd import _lib, ops
    calls = []
    monkeypatch.setattr(_lib, 'call', lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, '_chk', lambda t, name, shape=None: t.contiguous())
    monkeypatch.setattr(ops, '_stream', lambda: None)
    monkeypatch.setattr(ops, '_ptr', lambda t: None if t is None else tuple(t.shape))
    N, T, D, L = 5, 4, 6, 2
    c = ops.GPCache()
    c.kernel, c.Di, c.Do, c.M, c.S, c.nd, c.stacked, c.pack = 'RBF', D, D, 8, 16, L, True, torch.zeros(L, 64)
    z0, zL = torch.zeros(N, D), torch.zeros(L, N, D)
    ts, rows = torch.arange(T).float(), torch.arange(T).float().expand(N, T)
    for z, t, plain in ((z0, ts, 'gpode_rollout_fwd_n'), (zL, ts, 'gpode_rollout_fwd_nz'), (z0, rows, 'gpode_rollout_fwd_nt'),
                        (zL, rows, 'gpode_rollout_fwd_nt')):
        del calls[:]
        zt, xs = ops.rollout(c, z, t, 1, 'rk4', save_stages=True)
        assert [n for n, _ in calls] == [plain] and tuple(xs.shape) == (L, N, T - 1, 4, D)
        zt, xs = ops.rollout(c, z, t, 1, 'rk4', save_stages=True, substeps=3)
        name, a = calls[-1]
        assert name == 'gpode_rollout_fwd_ns' and a[-4:] == (int(z.dim() == 3), int(t.dim() == 2), 3, None)
        assert tuple(zt.shape) == (L, N, T, D) and tuple(xs.shape) == (L, N, T - 1, 3, 4, D) and a[-5] == tuple(xs.shape)
    gzt = torch.zeros(L, N, T, D)
    for t, plain in ((ts, '_n'), (rows, '_nt')):
        del calls[:]
        ops.rollout_bwd(c, torch.zeros(L, N, T - 1, 2, D), gzt, t, 1, 'midpoint')
        ops.rollout_bwd_pgrad(c, torch.zeros(L, N, T - 1, 1, D), gzt, t, 1, 'euler', 5)
        assert [n for n, _ in calls] == ['gpode_rollout_bwd' + plain, 'gpode_rollout_bwd_pgrad' + plain]
        gz0, ast = ops.rollout_bwd(c, torch.zeros(L, N, T - 1, 3, 2, D), gzt, t, 1, 'midpoint', substeps=3)
        assert calls[-1][0] == 'gpode_rollout_bwd_ns' and calls[-1][1][-3:] == (int(t.dim() == 2), 3, None)
        assert tuple(ast.shape) == (L, N, T - 1, 3, 2, D) and tuple(gz0.shape) == (L, N, D)
        gz0, ast, gpack = ops.rollout_bwd_pgrad(c, torch.zeros(L, N, T - 1, 3, 1, D), gzt, t, 1, 'euler', 5, substeps=3)
        assert calls[-1][0] == 'gpode_rollout_bwd_pgrad_ns' and calls[-1][1][-3:] == (int(t.dim() == 2), 3, None)
        assert tuple(ast.shape) == (L, N, T - 1, 3, 1, D) and tuple(gpack.shape) == (L, 64)


def test_the_dopri5_record_has_names_and_stays_a_tuple(monkeypatch):
    """rollout(..., 'dopri5', save_stages=True): the record's fields by name are its positions (xstage, hstep, iend / istep, counts, and in
    dense-output mode theta; a landing record stays four long, its theta None) and are the tensors handed to the entry point;
    rollout_bwd takes a plain tuple in that order as before"""
    from vae_gp_ode_amd import _lib, ops
    calls = []
    monkeypatch.setattr(_lib, 'call', lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, '_chk', lambda t, name, shape=None: t.contiguous())
    monkeypatch.setattr(ops, '_stream', lambda: None)
    monkeypatch.setattr(ops, '_ptr', lambda t: t)                            # the tensors themselves stand in for their addresses
    monkeypatch.setattr(ops, '_check_increasing', lambda ts: None)           # asks the device whether a capture is under way
    N, T, D, L, K = 5, 4, 6, 2, 12
    c = ops.GPCache()
    c.kernel, c.Di, c.Do, c.M, c.S, c.nd, c.stacked, c.pack = 'RBF', D, D, 8, 16, L, True, torch.zeros(L, 64)
    z0, ts, gzt = torch.zeros(N, D), torch.arange(T).float(), torch.zeros(L, N, T, D)
    for dense, fwd, bwd in ((False, 'gpode_rollout_adaptive_fwd_n', 'gpode_rollout_adaptive_bwd_n'),
                            (True, 'gpode_rollout_dense_fwd_n', 'gpode_rollout_dense_bwd_n')):
        del calls[:]
        zt, rec = ops.rollout(c, z0, ts, 1, 'dopri5', save_stages=True, dense=dense)
        names = ('xstage', 'hstep', 'index', 'counts') + (('theta',) if dense else ())
        assert isinstance(rec, tuple) and len(rec) == len(names) and rec._fields == names
        assert all(getattr(rec, n) is rec[i] for i, n in enumerate(names))
        assert tuple(rec.xstage.shape) == (L, N, K, 7 if dense else 6, D) and tuple(rec.hstep.shape) == (L, N, K)
        assert tuple(rec.index.shape) == (L, N, T - 1) and rec.index.dtype == torch.int32 and tuple(rec.counts.shape) == (L, N, 4)
        assert (tuple(rec.theta.shape) == (L, N, T - 1)) if dense else rec.theta is None
        (name, a), = calls
        tail = (rec.xstage, rec.hstep, rec.index) + ((rec.theta,) if dense else ()) + (rec.counts, None)
        assert name == fwd and a[16] is zt and len(a) == 17 + len(tail) and all(x is y for x, y in zip(a[17:], tail))
        # the reverse sweep: the record itself, a plain tuple in its order and one without the counts behind the index go to the same call
        for r in [rec, tuple(rec)] + ([] if dense else [tuple(rec)[:3]]):
            del calls[:]
            gz0, ast = ops.rollout_bwd(c, r, gzt, ts, 1, 'dopri5')
            (name, a), = calls
            want = (rec.xstage, rec.hstep, rec.index) + ((rec.theta,) if dense else ()) + (gzt, N, T, K, gz0, ast, None)
            assert name == bwd and len(a) == 9 + len(want) and all(x is y for x, y in zip(a[9:], want))
            assert tuple(ast.shape) == (L, N, K, 7 if dense else 6, D)


def test_library_refuses_a_count_outside_the_range_by_name():
    """the entry points themselves (no GPU needed: refused before anything is launched), with gpode_last_error() naming the entry point"""
    from vae_gp_ode_amd import _lib
    lib = _lib.load()
    for bad in (0, 65, -3):
        assert lib.gpode_rollout_fwd_ns(0, 1, 1, 6, 6, 8, 16, 1, None, None, None, 5, 4, None, None, 0, 0, bad, None) != 0
        e = lib.gpode_last_error().decode()
        assert e.startswith('gpode_rollout_fwd_ns:') and 'substeps=%d' % bad in e and '64' in e, e
        assert lib.gpode_rollout_bwd_ns(0, 1, 1, 6, 6, 8, 16, 1, None, None, None, None, 5, 4, None, None, 0, bad, None) != 0
        e = lib.gpode_last_error().decode()
        assert e.startswith('gpode_rollout_bwd_ns:') and 'substeps=%d' % bad in e, e
        assert lib.gpode_rollout_bwd_pgrad_ns(0, 1, 1, 6, 6, 8, 16, 1, None, None, None, None, 5, 4, None, None, None, 5, None, 0, bad, None) != 0
        e = lib.gpode_last_error().decode()
        assert e.startswith('gpode_rollout_bwd_pgrad_ns:') and 'substeps=%d' % bad in e, e


def test_the_test_door_takes_0_and_1_only():
    """gpode_test_substep_kernels: the door that sends one-step launches through the sub-step instantiation of the rollout kernels"""
    from vae_gp_ode_amd import _lib
    lib = _lib.load()
    hdr = ' '.join(open(os.path.join(ROOT, 'include', 'gpode.h')).read().split())
    assert 'int gpode_test_substep_kernels(int on);' in hdr and 'For tests.' in hdr
    try:
        for bad in (2, -1):
            assert lib.gpode_test_substep_kernels(bad) != 0
            assert lib.gpode_last_error().decode().startswith('gpode_test_substep_kernels:')
        assert lib.gpode_test_substep_kernels(1) == 0
    finally:
        assert lib.gpode_test_substep_kernels(0) == 0
