"""CPU-only: the host side of the compact ragged route (padded frames taken out in front of the decoder).
  frame_index     with counts= against numpy for counts (0, 1, T, T+5, -2, 3): off, src, P, and the clamped counts; P == 0 raises
  the CLI         --ragged_compact is off by default, and each of its three refusals (no --ragged_frames, --hip_graph True, several
                  ranks) is raised by main() itself ahead of any device work -- this file runs without a device
  compute_loss    compact=True without n_obs raises before it touches the model
  the C ABI       the four new entry points stand in _lib.SIGNATURES and in include/gpode.h with the same number of arguments"""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('gpode_gather_frames_fwd', 'gpode_gather_frames_bwd', 'gpode_sigmoid_loglik_fwd_pk', 'gpode_sigmoid_loglik_bwd_pk')


def test_frame_index_against_numpy():
    from vae_gp_ode_amd import vae_ops as V
    T = 4
    counts = (0, 1, T, T + 5, -2, 3)
    n_obs = torch.tensor(counts, dtype=torch.int32)
    ix = V.frame_index(n_obs, T, counts=counts)
    c = np.clip(np.array(counts), 0, T)
    off = np.concatenate(([0], np.cumsum(c)))
    src = np.array([n * T + t for n in range(len(c)) for t in range(c[n])])
    assert (ix.P, ix.N, ix.T) == (int(off[-1]), len(counts), T) and ix.P == 12
    assert ix.off.dtype == torch.int32 and ix.src.dtype == torch.int32
    assert ix.off.tolist() == off.tolist() and ix.src.tolist() == src.tolist()
    assert list(ix.counts) == c.tolist()
    # the counts read from the tensor give the same index
    iy = V.frame_index(n_obs, T)
    assert iy.off.tolist() == off.tolist() and iy.src.tolist() == src.tolist() and iy.P == ix.P


def test_frame_index_refuses_an_empty_minibatch():
    from vae_gp_ode_amd import _lib, vae_ops as V
    with pytest.raises(_lib.GpodeError, match='no observed frame in the minibatch'):
        V.frame_index(torch.tensor([0, -3], dtype=torch.int32), 5, counts=(0, -3))
    with pytest.raises(_lib.GpodeError, match='no observed frame in the minibatch'):
        V.frame_index(torch.zeros(3, dtype=torch.int32), 5)


def test_flag_is_off_by_default():
    from vae_gp_ode_amd import main as M
    assert M.make_parser().parse_args([]).ragged_compact is False
    assert M.make_parser().parse_args(['--ragged_compact', 'True']).ragged_compact is True


@pytest.mark.parametrize('case', ['no ragged_frames', 'hip_graph', 'ranks'])
def test_flag_refusals_come_before_any_device_work(case, monkeypatch, tmp_path):
    from vae_gp_ode_amd import main as M
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    touched = []
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: touched.append('is_available') or False)
    monkeypatch.setattr(M, 'init_distributed', lambda: touched.append('init_distributed'))
    argv = ['--task', 'synthetic', '--T', '6', '--ragged_compact', 'True']
    if case == 'no ragged_frames':
        want = 'needs --ragged_frames'
    elif case == 'hip_graph':
        argv += ['--ragged_frames', '3', '--hip_graph', 'True']
        want = 'not with --hip_graph'
    else:
        argv += ['--ragged_frames', '3']
        monkeypatch.setenv('WORLD_SIZE', '2')
        want = 'not on several ranks'
    with pytest.raises(SystemExit) as e:
        M.main(argv)
    assert '--ragged_compact' in str(e.value) and want in str(e.value), str(e.value)
    assert not touched and not os.listdir(tmp_path), (touched, os.listdir(tmp_path))


def test_compact_loss_needs_the_counts():
    from vae_gp_ode_amd.model.create_model import compute_loss
    with pytest.raises(ValueError, match='compact=True needs n_obs'):
        compute_loss(None, torch.zeros(2, 3, 1, 28, 28), 1, compact=True)


def test_new_entry_points_are_declared_and_bound_alike():
    from vae_gp_ode_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'gpode.h')).read(), flags=re.S)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, txt)
        assert m, 'not declared in include/gpode.h: ' + name
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
