"""The host side of the conditional forecast, without a GPU: evaluate.cond_stats against a brute-force float64 loop, the argument checks
of predict_conditional, the command-line switch, and the refusal transcript of gpode_dec10_predict_w (return code and
gpode_last_error() text as literals, every case refused in front of the first HIP runtime call -- the pattern of
tests/test_cabi_refusals_host.py, whose pointers are host addresses too, so those cases are skipped on a machine with a GPU, where
tests/test_gpu_cond_forecast.py holds the same paths by launch tag and result)."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

from vae_gp_ode_amd import _lib


# ---- cond_stats ---------------------------------------------------------------------------------------------------------------------
def _brute(ell, lw, n_cond, T, n_obs=None):
    """the definitions, element by element, in Python floats (max-subtracted sums, math.fsum)"""
    L, N = len(lw), len(lw[0])
    nc = [n_cond] * N if isinstance(n_cond, int) else list(n_cond)
    out = dict(logw=[[0.0] * N for _ in range(L)], ess=[], evidence=[], fc_ll=[], k=[])
    lt = [[float('nan')] * N for _ in range(T)]
    for n in range(N):
        o = T if n_obs is None else max(0, min(T, n_obs[n]))
        k = max(0, min(nc[n], T, o))
        out['k'].append(k)
        lg = [lw[l][n] + math.fsum(ell[l][n][t] for t in range(k)) for l in range(L)]
        for l in range(L):
            out['logw'][l][n] = lg[l]
        top = max(lg)
        if top == -math.inf:
            out['ess'].append(float('nan')); out['evidence'].append(-math.inf); out['fc_ll'].append(float('nan'))
            continue
        w = [math.exp(v - top) for v in lg]
        s1 = math.fsum(w)
        out['ess'].append(s1 * s1 / math.fsum(v * v for v in w))
        out['evidence'].append(top + math.log(s1) - math.log(L))
        wn = [v / s1 for v in w]
        fs = [math.fsum(ell[l][n][t] for t in range(k, o)) for l in range(L)]
        ft = max(fs)
        out['fc_ll'].append(ft + math.log(math.fsum(wn[l] * math.exp(fs[l] - ft) for l in range(L))))
        for t in range(k, o):
            et = max(ell[l][n][t] for l in range(L))
            lt[t][n] = et + math.log(math.fsum(wn[l] * math.exp(ell[l][n][t] - et) for l in range(L)))
    out['fc_nlpd_t'] = []
    for t in range(T):
        v = [x for x in lt[t] if not math.isnan(x)]
        out['fc_nlpd_t'].append(-math.fsum(v) / len(v) if v else float('nan'))
    have = [n for n in range(N) if (T if n_obs is None else max(0, min(T, n_obs[n]))) > out['k'][n]]
    out['fc_nlpd'] = -math.fsum(out['fc_ll'][n] for n in have) / len(have) if have else float('nan')
    return out


def _close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=torch.float64).reshape(-1), torch.as_tensor(b, dtype=torch.float64).reshape(-1)
    same = (torch.isnan(a) == torch.isnan(b)).all() and (torch.isinf(a) == torch.isinf(b)).all()
    ok = torch.isfinite(b)
    return bool(same) and bool(((a[ok] - b[ok]).abs() <= tol * b[ok].abs().clamp_min(1.0)).all()) and bool((a[~ok & ~torch.isnan(b)] == b[~ok & ~torch.isnan(b)]).all())


@pytest.mark.parametrize('n_cond,n_obs', [(2, None), (1, None), (6, None), ([1, 3, 6, 2], None), (3, [6, 2, 0, 4]), ([2, 2, 5, 6], [1, 6, 5, 3])])
def test_cond_stats_against_a_brute_force_loop(n_cond, n_obs):
    from vae_gp_ode_amd import evaluate as E
    L, N, T, Th = 7, 4, 6, 8
    g = torch.Generator().manual_seed(3)
    ell = -3000.0 + 40.0 * torch.randn(L, N, Th, generator=g, dtype=torch.float64)       # the magnitude of a frame's log-likelihood
    lw = -8.0 + 3.0 * torch.randn(L, N, generator=g, dtype=torch.float64)
    nc = n_cond if isinstance(n_cond, int) else torch.tensor(n_cond)
    nb = None if n_obs is None else torch.tensor(n_obs, dtype=torch.int32)
    s = E.cond_stats(ell, lw, nc, T, nb)
    ref = _brute(ell.tolist(), lw.tolist(), n_cond, T, n_obs)
    assert s.prefix.tolist() == ref['k'] and s.logw.dtype == torch.float64
    for name in ('logw', 'ess', 'evidence', 'fc_ll', 'fc_nlpd_t'):
        assert _close(getattr(s, name), ref[name]), (name, getattr(s, name), ref[name])
    assert _close(s.fc_nlpd, ref['fc_nlpd'])
    assert _close(s.wn.sum(0), torch.ones(N)) and ((s.ess >= 1 - 1e-12) & (s.ess <= L + 1e-12)).all()
    # the same input gives the same bits; float32 input is widened first
    s2 = E.cond_stats(ell.clone(), lw.clone(), nc, T, nb)
    assert all(torch.equal(torch.nan_to_num(getattr(s, k), nan=-7.0), torch.nan_to_num(getattr(s2, k), nan=-7.0)) for k in ('logw', 'ess', 'evidence', 'fc_ll', 'fc_nlpd_t'))
    assert E.cond_stats(ell.float(), lw.float(), nc, T, nb).evidence.dtype == torch.float64


def test_cond_stats_identities_and_degenerate_columns():
    from vae_gp_ode_amd import evaluate as E
    L, N, T = 5, 3, 4
    g = torch.Generator().manual_seed(4)
    ell = -500.0 + 10.0 * torch.randn(L, N, T, generator=g, dtype=torch.float64)
    lw = torch.randn(L, N, generator=g, dtype=torch.float64)
    iw_ll, _, ess = E.iw_stats(ell.sum(2), lw)
    full = E.cond_stats(ell, lw, T, T)
    assert torch.equal(full.evidence, iw_ll) and torch.equal(full.ess, ess)              # conditioned on everything: the marginal likelihood
    assert (full.fc_ll == 0).all() and math.isnan(full.fc_nlpd) and torch.isnan(full.fc_nlpd_t).all()
    for k in (1, 2, 3):
        s = E.cond_stats(ell, lw, k, T)
        assert (s.fc_ll - (iw_ll - s.evidence)).abs().max() <= 1e-9                      # log p(x_{>=k} | x_{<k}) = log p(x) - log p(x_{<k})
        assert torch.isnan(s.fc_nlpd_t[:k]).all() and torch.isfinite(s.fc_nlpd_t[k:]).all()
    # a column without any weight: evidence -inf, ess nan (stated in the docstring); the other columns are untouched
    lw2 = lw.clone()
    lw2[:, 1] = -math.inf
    s, ok = E.cond_stats(ell, lw2, 2, T), E.cond_stats(ell, lw, 2, T)
    assert s.evidence[1] == -math.inf and math.isnan(s.ess[1]) and math.isnan(s.fc_ll[1]) and torch.isnan(s.wn[:, 1]).all()
    assert torch.equal(s.evidence[[0, 2]], ok.evidence[[0, 2]]) and torch.equal(s.ess[[0, 2]], ok.ess[[0, 2]])
    assert 'evidence = -inf' in E.cond_stats.__doc__ and 'nan' in E.cond_stats.__doc__
    # one draw without weight is a weight of 0, nothing else
    lw3 = lw.clone()
    lw3[2, 0] = -math.inf
    keep = [0, 1, 3, 4]
    a, b = E.cond_stats(ell, lw3, 2, T), E.cond_stats(ell[keep], lw3[keep], 2, T)
    assert _close(a.ess[0], b.ess[0]) and _close(a.evidence[0] + math.log(L), b.evidence[0] + math.log(L - 1)) and _close(a.fc_ll[0], b.fc_ll[0])
    # equal weights: ess = L, and a dominant one: ess = 1
    assert _close(E.cond_stats(torch.zeros(L, N, T), torch.zeros(L, N), 2, T).ess, torch.full((N,), float(L)))
    lw4 = torch.zeros(L, N, dtype=torch.float64)
    lw4[1] = 200.0
    assert _close(E.cond_stats(torch.zeros(L, N, T), lw4, 2, T).ess, torch.ones(N))


# ---- predict_conditional's argument checks: all in front of any device work ---------------------------------------------------------------
def test_predict_conditional_argument_checks(monkeypatch):
    from vae_gp_ode_amd import evaluate as E
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: pytest.fail('asked for the device'))

    class Model:
        order, v_steps = 1, 5

        def __getattr__(self, name):
            pytest.fail('the model was touched (%s)' % name)
    m1, m2 = Model(), Model()
    m2.order = 2
    X = torch.zeros(3, 6, 1, 28, 28)
    with pytest.raises(ValueError, match='X must be'):
        E.predict_conditional(m1, X[:, :, 0], 4, 2)
    with pytest.raises(ValueError, match='encoder reads the first 1 frame'):
        E.predict_conditional(m1, X, 4, 0)
    with pytest.raises(ValueError, match='encoder reads the first 5 frame'):
        E.predict_conditional(m2, X, 4, 4)
    with pytest.raises(ValueError, match='exceeds the observed length T = 6'):
        E.predict_conditional(m1, X, 4, 7)
    with pytest.raises(ValueError, match='encoder reads the first 1 frame'):
        E.predict_conditional(m1, X, 4, torch.tensor([2, 0, 3]))
    with pytest.raises(ValueError, match='exceeds the observed length'):
        E.predict_conditional(m1, X, 4, torch.tensor([2, 7, 3]))
    with pytest.raises(ValueError, match=r'\(N,\) = \(3,\)'):
        E.predict_conditional(m1, X, 4, torch.tensor([2, 3]))
    with pytest.raises(ValueError, match='integer'):
        E.predict_conditional(m1, X, 4, 2.5)
    with pytest.raises(ValueError, match='T_custom'):
        E.predict_conditional(m1, X, 4, 2, T_custom=5)
    with pytest.raises(ValueError, match='n_obs must be an int32 tensor'):
        E.predict_conditional(m1, X, 4, 2, n_obs=[6, 6, 6])
    with pytest.raises(ValueError, match='ts must be'):
        E.predict_conditional(m1, X, 4, 2, ts=torch.zeros(2, 6))
    assert 'no Bessel correction' in E.ConditionalPrediction.__doc__.replace('NO', 'no')


# ---- the switch -------------------------------------------------------------------------------------------------------------------------
def test_eval_condition_frames_is_off_by_default_and_parsed_by_both():
    from vae_gp_ode_amd import evaluate as E, main as M
    assert E.make_parser().parse_args([]).eval_condition_frames == 0
    assert E.make_parser().parse_args(['--eval_condition_frames', '4']).eval_condition_frames == 4
    assert M.make_parser().parse_args([]).eval_condition_frames == 0
    assert M.make_parser().parse_args(['--eval_condition_frames', '4']).eval_condition_frames == 4    # one command line serves both; training ignores it
    E.check_condition_frames(E.make_parser().parse_args([]))
    E.check_condition_frames(E.make_parser().parse_args(['--T', '16', '--eval_condition_frames', '16']))
    E.check_condition_frames(E.make_parser().parse_args(['--T', '16', '--ode', '2', '--frames', '5', '--eval_condition_frames', '5']))


@pytest.mark.parametrize('argv,words', [(['--T', '16', '--eval_condition_frames', '17'], 'has 16 frames'),
                                        (['--T', '16', '--eval_condition_frames', '-1'], 'encoder reads the first 1'),
                                        (['--T', '16', '--ode', '2', '--frames', '5', '--eval_condition_frames', '4'], 'encoder reads the first 5'),
                                        (['--T', '16', '--subsample_frames', '8', '--eval_condition_frames', '9'], 'has 8 frames')])
def test_a_bad_prefix_exits_before_any_device_work(monkeypatch, argv, words):
    from vae_gp_ode_amd import evaluate
    monkeypatch.setattr(evaluate, 'build_from_checkpoint', lambda *a: pytest.fail('reached the checkpoint'))
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: pytest.fail('asked for the device'))
    with pytest.raises(SystemExit) as e:
        evaluate.main(argv)
    assert '--eval_condition_frames' in str(e.value) and words in str(e.value)


def test_several_ranks_are_refused(monkeypatch):
    from vae_gp_ode_amd import evaluate
    monkeypatch.setattr(evaluate, 'build_from_checkpoint', lambda *a: pytest.fail('reached the checkpoint'))
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: pytest.fail('asked for the device'))
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit) as e:
        evaluate.main(['--T', '16', '--eval_condition_frames', '4'])
    assert 'single-process' in str(e.value)


# ---- the refusal transcript -----------------------------------------------------------------------------------------------------------
_BUF = ctypes.create_string_buffer(4096)
P = (ctypes.addressof(_BUF) + 63) & ~63              # a 16-byte aligned address
Q = P + 4                                            # one that is not
NAME = 'gpode_dec10_predict_w'
SIZES = 'need Lc, F >= 1, 1 <= T_obs <= Th, F a multiple of Th, done >= 0'
NSEQ = 'need N >= 1 and F = N * Th'
ROWS = 'logw has L_total rows, need done + Lc <= L_total'


def _args(c=P, table=P, w=P, bias=0, X=P, Lc=2, F=6, Th=3, T_obs=2, done=2, logw=P, L_total=4, N=2, wstate=P, mean=P, m2=P, wse=P, n_obs=0):
    return (c, table, w, bias, X, Lc, F, Th, T_obs, done, logw, L_total, N, wstate, mean, m2, wse, n_obs, 0)


# in the order of the checks: each case repairs what the one before it was refused for and meets the next
CASES = [(dict(c=0), 'null pointer'), (dict(table=0), 'null pointer'), (dict(w=0), 'null pointer'), (dict(X=0), 'null pointer'),
         (dict(mean=0), 'null pointer'), (dict(m2=0), 'null pointer'), (dict(wse=0), 'null pointer'),
         (dict(logw=0, Lc=0), 'logw is NULL'), (dict(wstate=0, Lc=0), 'wstate is NULL'),
         (dict(Lc=0, N=0), SIZES), (dict(F=0, N=0), SIZES), (dict(Th=0, N=0), SIZES), (dict(T_obs=0, N=0), SIZES), (dict(T_obs=4, N=0), SIZES),
         (dict(F=7, N=0), SIZES), (dict(done=-1, N=0), SIZES),
         (dict(N=0, table=Q), NSEQ), (dict(N=-2, table=Q), NSEQ), (dict(N=4, table=Q), NSEQ), (dict(N=3, table=Q), NSEQ),
         (dict(table=Q, L_total=3), 'the table must be 16-byte aligned'),
         (dict(L_total=3), ROWS), (dict(L_total=0), ROWS), (dict(L_total=4, done=3), ROWS), (dict(L_total=1, Lc=2, done=0), ROWS)]


@pytest.mark.skipif(torch.cuda.is_available(), reason='the pointers are host addresses: with a GPU present a refusal that got lost would '
                    'launch a kernel on host memory (tests/test_gpu_cond_forecast.py covers these paths there)')
@pytest.mark.parametrize('kw,text', CASES, ids=['%d-%s' % (i, '-'.join(c[0])) for i, c in enumerate(CASES)])
def test_refusal_text_and_code(kw, text):
    lib = _lib.load()
    assert getattr(lib, NAME)(*_args(**kw)) == 1
    assert lib.gpode_last_error().decode() == '%s: %s' % (NAME, text)
    assert 'launch failed' not in text and 'hip' not in text.lower()


_VALU_SCRIPT = r'''
import importlib.util, sys
spec = importlib.util.spec_from_file_location('gpode_lib', sys.argv[1])
m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
lib = m.load()
args = [64] * 5 + [0] * 5 + [64, 0, 0] + [64] * 4 + [0, 0]      # bad sizes too: the switch is checked in front of them
print(lib.gpode_dec10_predict_w(*args), lib.gpode_last_error().decode())
'''


def test_the_vector_only_switch_is_refused_first_in_the_ll_twins_words():
    """GPODE_CONV_VALU is read once per process, hence the child; it loads _lib.py by path, without the package and torch."""
    env = dict(os.environ, GPODE_CONV_VALU='1')
    out = subprocess.run([sys.executable, '-c', _VALU_SCRIPT, _lib.__file__], env=env, capture_output=True, text=True, check=True).stdout
    assert out.splitlines() == ['1 %s: matrix-core kernel only (GPODE_CONV_VALU is set)' % NAME]


def test_the_binding_the_header_and_the_library_agree():
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gpode.h')).read()
    proto = re.search(r'int gpode_dec10_predict_w\(([^;]*)\);', hdr).group(1)
    assert len(proto.split(',')) == len(_lib.SIGNATURES[NAME][1]) == 19
    assert hasattr(_lib.load(), NAME)
