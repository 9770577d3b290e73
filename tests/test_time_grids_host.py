"""Host side of the per-sequence time grids: the `_nt` entry points in the header and in _lib.SIGNATURES, data.utils.subsample_frames,
the sharding of a grid with its minibatch, the command-line flag, and the shape checks ops makes before it calls the library."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = {'gpode_rollout_fwd_nt': 'gpode_rollout_fwd_nz', 'gpode_rollout_adaptive_fwd_nt': 'gpode_rollout_adaptive_fwd_nz',
      'gpode_rollout_dense_fwd_nt': 'gpode_rollout_dense_fwd_nz', 'gpode_rollout_bwd_nt': 'gpode_rollout_bwd_n',
      'gpode_rollout_bwd_pgrad_nt': 'gpode_rollout_bwd_pgrad_n'}


def _decl(hdr, sym):
    m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % sym, hdr)
    assert m, sym
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def test_header_declares_the_time_grid_entry_points():
    """each `_nt` symbol is declared, is in SIGNATURES, and takes its twin's arguments plus `int ts_per_traj` in front of the stream"""
    import ctypes
    from vae_gp_ode_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gpode.h')).read()
    for sym, twin in NT.items():
        assert re.search(r'\bint\s+%s\s*\(' % sym, hdr) and sym in _lib.SIGNATURES, sym
        a, b = _decl(hdr, sym), _decl(hdr, twin)
        assert a == b[:-1] + ['int ts_per_traj', 'void* stream'], (sym, a, b)
        (res, args), (res2, args2) = _lib.SIGNATURES[sym], _lib.SIGNATURES[twin]
        assert res is res2 and args == args2[:-1] + [ctypes.c_int, ctypes.c_void_p], sym
    block = hdr[hdr.index('PER TRAJECTORY'):hdr.index('int gpode_rollout_fwd_nt')]
    assert 'ts_per_traj = 0' in block and 'ts_per_traj = 1' in block and 'Status 3' in block and 'refused' in block


# ---- subsample_frames ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,T,keep,lead', [(7, 16, 6, 1), (5, 8, 8, 1), (3, 9, 6, 5), (1, 4, 2, 1), (64, 6, 4, 1)])
def test_subsample_frames_draws_sorted_distinct_indices_that_hold_the_leading_frames(N, T, keep, lead):
    from vae_gp_ode_amd.data.utils import subsample_frames
    X = torch.arange(N * T, dtype=torch.float32).view(N, T, 1, 1, 1).expand(N, T, 1, 2, 2).contiguous()
    state = torch.get_rng_state()
    Xs, idx = subsample_frames(X, keep, lead, torch.Generator().manual_seed(3))
    assert torch.equal(torch.get_rng_state(), state)                   # the global generator is not touched
    assert tuple(Xs.shape) == (N, keep, 1, 2, 2) and tuple(idx.shape) == (N, keep) and idx.dtype == torch.int64
    assert (idx[:, 1:] > idx[:, :-1]).all()                            # sorted and distinct
    assert int(idx.min()) == 0 and int(idx.max()) <= T - 1
    assert torch.equal(idx[:, :lead], torch.arange(lead).expand(N, lead))
    for n in range(N):
        assert torch.equal(Xs[n], X[n, idx[n]])
    # the same seed, the same subsets; another seed, others (where there is anything to draw)
    _, again = subsample_frames(X, keep, lead, torch.Generator().manual_seed(3))
    assert torch.equal(again, idx)
    if keep < T and N >= 5:
        _, other = subsample_frames(X, keep, lead, torch.Generator().manual_seed(4))
        assert not torch.equal(other, idx)
        assert len({tuple(r) for r in idx.tolist()}) > 1               # per sequence, not one subset for the minibatch
    if keep == T:
        assert torch.equal(Xs, X)


def test_subsample_frames_covers_every_later_frame_and_refuses_bad_counts():
    from vae_gp_ode_amd.data.utils import subsample_frames
    X = torch.zeros(400, 7, 1, 1, 1)
    _, idx = subsample_frames(X, 3, 1, torch.Generator().manual_seed(0))
    counts = torch.bincount(idx.flatten(), minlength=7)
    assert counts[0] == 400 and (counts[1:] > 0).all() and int(counts[1:].sum()) == 800
    for keep, lead in ((8, 1), (1, 1), (5, 5), (3, 0)):
        with pytest.raises(ValueError, match='subsample_frames'):
            subsample_frames(X, keep, lead, torch.Generator().manual_seed(0))


def test_shard_batch_selects_the_same_rows_of_the_minibatch_and_of_its_grid():
    from vae_gp_ode_amd.data.utils import subsample_frames
    from vae_gp_ode_amd.parallel import shard_batch, shard_bounds
    N, T, world = 7, 6, 3
    X = torch.arange(N, dtype=torch.float32).view(N, 1, 1, 1, 1).expand(N, T, 1, 2, 2).contiguous()
    Xs, idx = subsample_frames(X, 4, 1, torch.Generator().manual_seed(1))
    ts = 0.1 * idx.float()
    seen = []
    for r in range(world):
        lo, hi = shard_bounds(N, r, world)
        xr, tr = shard_batch(Xs, r, world), shard_batch(ts, r, world)
        assert xr.shape[0] == tr.shape[0] == hi - lo
        assert torch.equal(xr[:, 0, 0, 0, 0], torch.arange(lo, hi, dtype=torch.float32)) and torch.equal(tr, ts[lo:hi])
        seen += list(range(lo, hi))
    assert seen == list(range(N))


# ---- command line ----------------------------------------------------------------------------------------------------------------------
def test_flag_is_off_by_default_and_evaluate_carries_it():
    from vae_gp_ode_amd import evaluate as E
    from vae_gp_ode_amd import main as M
    assert M.make_parser().parse_args([]).subsample_frames == 0
    assert E.make_parser().parse_args([]).subsample_frames == 0
    assert E.make_parser().parse_args(['--subsample_frames', '5']).subsample_frames == 5
    assert 'subsample_frames' in {f[0] for f in M.EXT_FLAGS} and len(M.FLAGS) == 39
    ok = M.make_parser().parse_args(['--T', '6', '--subsample_frames', '4'])
    M.check_subsample(ok)
    M.check_subsample(M.make_parser().parse_args(['--T', '6']))
    M.check_subsample(M.make_parser().parse_args(['--T', '8', '--ode', '2', '--frames', '5', '--subsample_frames', '6']))
    for argv in (['--T', '6', '--subsample_frames', '7'], ['--T', '6', '--subsample_frames', '1'],
                 ['--T', '8', '--ode', '2', '--frames', '5', '--subsample_frames', '5']):
        with pytest.raises(SystemExit, match='--subsample_frames'):
            M.check_subsample(M.make_parser().parse_args(argv))
    assert M.subsample_lead(ok) == 1


# ---- ops: the shape checks come before any library call ---------------------------------------------------------------------------------
def test_a_grid_with_the_wrong_number_of_rows_is_refused_before_any_library_call(monkeypatch):
    from vae_gp_ode_amd import _lib, ops

    def reached(name, *a):
        raise AssertionError('library call %s reached' % name)
    monkeypatch.setattr(_lib, 'call', reached)
    monkeypatch.setattr(ops, '_chk', lambda t, name, shape=None: t.contiguous())     # host tensors stand in for device ones
    monkeypatch.setattr(ops, '_stream', lambda: None)
    N, T, D = 5, 4, 6
    c = ops.GPCache()
    c.kernel, c.Di, c.Do, c.M, c.S, c.nd, c.stacked, c.pack = 'RBF', D, D, 8, 16, 1, False, torch.zeros(64)
    z0, good = torch.zeros(N, D), torch.arange(T).float().expand(N, T)
    assert ops._ts_per_traj(good[0], N) == 0 and ops._ts_per_traj(good, N) == 1
    bad = [torch.zeros(N + 1, T), torch.zeros(1, T), torch.zeros(N, T, 1), torch.zeros(())]
    for ts in bad:
        for method in ('rk4', 'euler', 'dopri5'):
            with pytest.raises(_lib.GpodeError) as e:
                ops.rollout(c, z0, ts, 1, method)
            assert str(tuple(ts.shape)) in str(e.value) and str((N, D)) in str(e.value), str(e.value)     # names both shapes
        with pytest.raises(_lib.GpodeError, match='ts must be'):
            ops.rollout_adaptive(c, z0, ts, 1, dense=True)
    gzt, xs = torch.zeros(N, T, D), torch.zeros(N, T - 1, 4, D)
    for ts in bad[:3] + [torch.zeros(N, T + 1)]:
        with pytest.raises(_lib.GpodeError) as e:
            ops.rollout_bwd(c, xs, gzt, ts, 1, 'rk4')
        assert str(tuple(ts.shape)) in str(e.value) and str((N, T, D)) in str(e.value)
        with pytest.raises(_lib.GpodeError, match='ts must be'):
            ops.rollout_bwd_pgrad(c, xs, gzt, ts, 1, 'rk4', 5)
    # a well-formed grid of either kind gets as far as the library
    for ts in (good[0].contiguous(), good):
        with pytest.raises(AssertionError, match='gpode_rollout_fwd_n' + ('t' if ts.dim() == 2 else ' ')):
            ops.rollout(c, z0, ts, 1, 'rk4')


def test_model_refuses_a_grid_that_does_not_match_the_horizon():
    from vae_gp_ode_amd.model.core.odegpvae import ODEGPVAE
    m = ODEGPVAE(flow=torch.nn.Identity(), vae=torch.nn.Identity(), num_observations=1, steps=5, order=1, dt=0.1)
    X = torch.zeros(3, 5, 1, 28, 28)
    for ts in (torch.zeros(3, 4), torch.zeros(4, 5), torch.zeros(5)):
        with pytest.raises(ValueError, match='ts must be'):
            m(X, ts=ts)
    with pytest.raises(ValueError, match='ts must be'):
        m(X, T_custom=8, ts=torch.zeros(3, 5))
    with pytest.raises(ValueError, match='ts must be'):
        m.sample_trajectories(torch.zeros(3, 6), 5, ts=torch.zeros(3, 6))
