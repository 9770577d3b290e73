"""CPU: the host side of ragged sequences -- data.utils.ragged_frames, the per-frame means and loglik_stats of evaluate with frame
counts, and the --ragged_frames flag."""
import math

import pytest
import torch


def brute_subsets(idx, n_obs, lead, T):
    for n in range(idx.shape[0]):
        k = int(n_obs[n])
        kept = idx[n, :k].tolist()
        assert kept == sorted(set(kept)) and kept[:lead] == list(range(lead)) and max(kept) <= T - 1, (n, kept)
        assert idx[n, k:].tolist() == [kept[-1] + 1 + j for j in range(idx.shape[1] - k)], (n, idx[n].tolist())


@pytest.mark.parametrize('kmin,kmax,lead,T', [(3, 8, 2, 16), (2, 16, 1, 16), (6, 6, 5, 7), (4, 5, 3, 8)])
def test_ragged_frames(kmin, kmax, lead, T):
    from vae_gp_ode_amd.data.utils import ragged_frames
    N = 200
    X = torch.rand(N, T, 1, 3, 3, generator=torch.Generator().manual_seed(1)) + 1.0      # no zero in the data
    gen = torch.Generator().manual_seed(2)
    cpu_state = torch.get_rng_state()
    Xp, idx, n_obs = ragged_frames(X, kmin, kmax, lead, gen)
    assert torch.equal(cpu_state, torch.get_rng_state()), 'the global generator was touched'
    assert tuple(Xp.shape) == (N, kmax, 1, 3, 3) and tuple(idx.shape) == (N, kmax) and tuple(n_obs.shape) == (N,)
    assert idx.dtype == torch.int64 and n_obs.dtype == torch.int32 and Xp.dtype == X.dtype
    assert int(n_obs.min()) == kmin and int(n_obs.max()) == kmax                         # both ends are reached over 200 sequences
    assert bool((idx[:, 1:] > idx[:, :-1]).all()), 'a row is not strictly increasing'
    brute_subsets(idx, n_obs, lead, T)
    for n in range(N):
        k = int(n_obs[n])
        assert torch.equal(Xp[n, :k], X[n, idx[n, :k]]) and bool((Xp[n, k:] == 0).all())
    if kmax < T:                                                                        # every later frame is drawn by some sequence
        assert set(idx[torch.arange(kmax)[None, :] < n_obs[:, None]].tolist()) == set(range(T))
    # the same generator state gives the same draw; the draw advances the generator
    again = ragged_frames(X, kmin, kmax, lead, torch.Generator().manual_seed(2))
    assert all(torch.equal(a, b) for a, b in zip((Xp, idx, n_obs), again))
    if kmin < kmax:
        assert not torch.equal(ragged_frames(X, kmin, kmax, lead, gen)[2], n_obs)


@pytest.mark.parametrize('kmin,kmax,lead,T', [(1, 4, 1, 6), (5, 4, 1, 6), (3, 7, 1, 6), (2, 4, 0, 6)])
def test_ragged_frames_refusals(kmin, kmax, lead, T):
    from vae_gp_ode_amd.data.utils import ragged_frames
    with pytest.raises(ValueError, match='ragged_frames'):
        ragged_frames(torch.zeros(2, T, 1), kmin, kmax, lead, torch.Generator().manual_seed(0))


def test_loglik_stats_and_frame_means_with_counts_match_a_brute_force_loop():
    from vae_gp_ode_amd import evaluate as E
    g = torch.Generator().manual_seed(3)
    L, N, Th, T = 3, 4, 6, 5
    counts = [5, 2, 0, 7]                                                               # frame 3 and 4: one sequence; none has frame 5
    ell = -1000.0 * torch.rand(L, N, Th, generator=g, dtype=torch.float64)
    ell[:, :, T:] = 0.0
    dirty = ell.clone()
    for n, k in enumerate(counts):
        dirty[:, n, k:] = float('nan')                                                  # what lies behind the mask is never read
    for n_obs in (counts, torch.tensor(counts, dtype=torch.int32)):
        ll, nll, nlpd, nll_t = E.loglik_stats(dirty, T, n_obs)
        want_ll = torch.zeros(L, N, dtype=torch.float64)
        for l in range(L):
            for n in range(N):
                for t in range(min(counts[n], T)):
                    want_ll[l, n] += ell[l, n, t]
        assert torch.allclose(ll, want_ll, rtol=1e-14, atol=0) and ll.dtype == torch.float64
        assert bool((ll[:, 2] == 0).all())
        assert math.isclose(nll, -want_ll.mean().item(), rel_tol=1e-14)
        assert math.isclose(nlpd, -E.log_mean_exp(want_ll).mean().item(), rel_tol=1e-14)
        for t in range(T):
            have = [n for n in range(N) if t < counts[n]]
            want = -sum(ell[l, n, t].item() for l in range(L) for n in have) / (L * len(have))
            assert math.isclose(nll_t[t].item(), want, rel_tol=1e-13), (t, nll_t[t].item(), want)
    # a frame index no sequence has: nan
    short = [2, 1, 0, 2]
    _, _, _, nll_t = E.loglik_stats(ell, T, short)
    assert tuple(nll_t.shape) == (T,) and bool(torch.isfinite(nll_t[:2]).all()) and bool(torch.isnan(nll_t[2:]).all())
    # the per-frame error means of predict
    se_mean = torch.rand(N, T, generator=g, dtype=torch.float64)
    obs = E._observed(counts, N, T)
    assert obs.tolist() == [[t < k for t in range(T)] for k in counts]
    mse_t = E.frame_means(torch.where(obs, se_mean, torch.full((), float('nan'), dtype=torch.float64)), obs)
    for t in range(T):
        have = [n for n in range(N) if t < counts[n]]
        assert math.isclose(mse_t[t].item(), sum(se_mean[n, t].item() for n in have) / len(have), rel_tol=1e-14)
    assert bool(torch.isnan(E.frame_means(se_mean, E._observed(short, N, T))[2:]).all())
    # without counts: the function as it was
    a, b = E.loglik_stats(ell, T), E.loglik_stats(ell, T, [T] * N)
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and torch.allclose(a[3], b[3], rtol=1e-15, atol=0)
    assert torch.equal(a[3], -ell[:, :, :T].mean(dim=(0, 1)))


def test_loader_items_and_keywords():
    from vae_gp_ode_amd import evaluate as E
    X, ts, n = torch.zeros(2, 3), torch.zeros(2, 3), torch.tensor([3, 1], dtype=torch.int32)
    assert E._frames_ts(X) == (X, None, None) and E._frames_ts((X,)) == (X, None, None)
    assert E._frames_ts((X, ts))[1] is ts and E._frames_ts((X, ts))[2] is None and E._frames_ts([X, ts, n])[2] is n
    assert E._grid_kw(None) == {} and E._grid_kw(ts) == {'ts': ts} and E._grid_kw(ts, n) == {'ts': ts, 'n_obs': n}


def test_cli_flag_is_off_by_default_and_refuses_bad_values():
    from vae_gp_ode_amd import evaluate as E
    from vae_gp_ode_amd import main as M
    for parser in (M.make_parser(), E.make_parser()):
        args = parser.parse_args([])
        assert args.ragged_frames == 0
        M.check_ragged(args)                                                            # off: nothing to refuse
    ok = M.make_parser().parse_args(['--ragged_frames', '2', '--T', '16'])
    M.check_ragged(ok)
    M.check_ragged(M.make_parser().parse_args(['--ragged_frames', '4', '--subsample_frames', '4']))
    M.check_ragged(M.make_parser().parse_args(['--ragged_frames', '6', '--ode', '2', '--frames', '5']))
    for argv, words in ((['--ragged_frames', '1'], '--ragged_frames 1: .*1 leading frame.*--T 16'),
                        (['--ragged_frames', '17'], '--ragged_frames 17: .*--T 16'),
                        (['--ragged_frames', '5', '--subsample_frames', '4'], '--ragged_frames 5: .*--subsample_frames 4'),
                        (['--ragged_frames', '5', '--ode', '2', '--frames', '5'], '--ragged_frames 5: .*5 leading frame')):
        with pytest.raises(SystemExit, match=words):
            M.check_ragged(M.make_parser().parse_args(argv))
        with pytest.raises(SystemExit, match='--ragged_frames'):                        # both command lines refuse ahead of any device work
            M.main(argv)
        with pytest.raises(SystemExit, match='--ragged_frames'):
            E.main(argv)
