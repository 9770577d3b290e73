"""The tangent-linear rollout without a GPU: the host reductions of evaluate.flow_diagnostics on flows with a closed form, the
--eval_flow switch, and the refusal transcript of gpode_rhs_jvp / gpode_rollout_jvp (tests/test_cabi_refusals_host.py's pattern: host
pointers, every refusal in front of the first HIP call, the cases walking the checks in their order -- each repairs what the one
before it was refused for)."""
import ctypes
import math

import pytest
import torch

from vae_gp_ode_amd import _lib


# ---- host reductions ----------------------------------------------------------------------------------------------------------------
def _rotation_flow(ts, w=0.7):
    """Phi_t of dz/dt = w J z in the plane: rotations by w t, (1, N=1, T, 2, 2)"""
    c, s = torch.cos(w * ts), torch.sin(w * ts)
    return torch.stack([torch.stack([c, -s], -1), torch.stack([s, c], -1)], -2)[None, None]


def test_reductions_on_a_rotation_give_zero():
    from vae_gp_ode_amd import evaluate as E
    ts = torch.tensor([0.0, 0.05, 0.2, 1.3], dtype=torch.float64)
    Phi = _rotation_flow(ts)
    ld, ft = E.flow_logdet(Phi), E.flow_ftle(Phi, ts)
    assert ld.shape == (1, 1, 4) and ft.shape == (1, 1) and ld.dtype == ft.dtype == torch.float64
    assert ld.abs().max() < 1e-14 and ft.abs().max() < 1e-14
    # a rotation carries an isotropic covariance to itself
    v = E.flow_var_lin(Phi, torch.full((1, 2), 0.3))
    assert v.shape == (1, 1, 4, 2) and (v - 0.3).abs().max() < 1e-7


def test_reductions_on_a_diagonal_linear_flow():
    from vae_gp_ode_amd import evaluate as E
    a = torch.tensor([0.4, -1.1, 0.25], dtype=torch.float64)
    ts = torch.tensor([0.0, 0.1, 0.35, 0.9], dtype=torch.float64)
    Phi = torch.diag_embed(torch.exp(a[None, :] * ts[:, None]))[None, None].repeat(2, 3, 1, 1, 1)          # (L=2, N=3, T, 3, 3)
    ld, ft = E.flow_logdet(Phi), E.flow_ftle(Phi, ts)
    assert ld.shape == (2, 3, 4) and ft.shape == (2, 3)
    assert (ld - a.sum() * ts).abs().max() < 1e-14
    assert (ft - a.max()).abs().max() < 1e-14
    # a grid per trajectory: the exponent divides by each row's own span
    rows = torch.stack([ts, 2 * ts, 3 * ts])
    assert (E.flow_ftle(Phi, rows) - a.max() / torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)).abs().max() < 1e-14
    var0 = torch.tensor([[1.0, 2.0, 3.0]] * 3)
    v = E.flow_var_lin(Phi, var0)
    assert v.shape == (2, 3, 4, 3)
    assert (v - torch.exp(2 * a[None, :] * ts[:, None]) * var0[0].double()).abs().max() < 1e-12
    # float32 input on any layout is reduced in float64
    assert E.flow_logdet(Phi.float()).dtype == torch.float64


# ---- the switch ---------------------------------------------------------------------------------------------------------------------
def test_eval_flow_switch_is_off_unless_given():
    from vae_gp_ode_amd import evaluate, main
    p = evaluate.make_parser()
    off = p.parse_args([])
    assert evaluate.eval_flow(off) is False and 'eval_flow' not in vars(off)
    assert {k: v for k, v in vars(off).items() if k != 'eval_z0_draws'} == vars(main.make_parser().parse_args([]))
    assert evaluate.eval_flow(p.parse_args(['--eval_flow', 'True'])) is True
    assert evaluate.eval_flow(p.parse_args(['--eval_flow', 'False'])) is False
    with pytest.raises(SystemExit):
        main.make_parser().parse_args(['--eval_flow', 'True'])


def test_eval_flow_refuses_dopri5_before_any_device_work(monkeypatch):
    """the exit comes in front of the device check and the checkpoint: neither is reached"""
    from vae_gp_ode_amd import evaluate
    monkeypatch.setattr(evaluate, 'build_from_checkpoint', lambda *a: pytest.fail('reached the checkpoint'))
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: pytest.fail('asked for the device'))
    with pytest.raises(SystemExit) as e:
        evaluate.main(['--solver', 'dopri5', '--eval_flow', 'True'])
    assert 'dopri5' in str(e.value) and 'controller' in str(e.value) and '--eval_flow' in str(e.value)


def test_layer_and_flow_argument_checks_without_a_device():
    from vae_gp_ode_amd.model.core.flow import Flow
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    gp = SVGP_Layer(3, 3, 8, 16, kernel='DF')
    with pytest.raises(RuntimeError, match='build_cache'):
        gp.jacobian(torch.zeros(2, 3))
    gp.cache = object()
    with pytest.raises(ValueError, match="'full', 'prior' or 'update'"):
        gp.divergence(torch.zeros(2, 3), part='posterior')
    with pytest.raises(ValueError, match='controller'):
        Flow(gp, order=1, solver='dopri5').sensitivity(torch.zeros(2, 3), torch.arange(3.0))
    with pytest.raises(ValueError, match='not built'):
        Flow(gp, order=1, solver='bdf').sensitivity(torch.zeros(2, 3), torch.arange(3.0))


# ---- the refusal transcript -----------------------------------------------------------------------------------------------------------
_BUF = ctypes.create_string_buffer(4096)
P = (ctypes.addressof(_BUF) + 63) & ~63
DOPRI5 = ('gpode_rollout_jvp: method 3 (dopri5): its steps depend on the state through the controller, and the tangent of the '
          'accepted-step sequence is not built (0 euler, 1 rk4, 2 midpoint)')


def _rollout(kernel=0, order=1, method=1, Di=6, Do=6, M=8, S=16, nd=1, pack=P, z0=P, zpd=0, v0=P, K=3, ts=P, tpt=0, sub=1, N=2, T=3,
             zt=P, vt=P):
    return (kernel, order, method, Di, Do, M, S, nd, pack, z0, zpd, v0, K, ts, tpt, sub, N, T, zt, vt, 0)


def _rhs(kernel=0, Di=6, Do=6, M=8, S=16, nd=1, pack=P, x=P, xpd=0, v=P, R=2, K=3, f=P, jv=P, mode=0):
    return (kernel, Di, Do, M, S, nd, pack, x, xpd, v, R, K, f, jv, mode, 0)


ROLLOUT = [
    (_rollout(method=3, sub=0, N=0, K=0, pack=0), DOPRI5),
    (_rollout(method=4, sub=0, N=0, K=0, pack=0), 'gpode_rollout_jvp: method 4 (0 euler, 1 rk4, 2 midpoint)'),
    (_rollout(zpd=2, sub=0, N=0, K=0, pack=0), 'gpode_rollout_jvp: z0_per_draw=2 (0 shared, 1 one (N,D) slab per draw)'),
    (_rollout(tpt=-1, sub=0, N=0, K=0, pack=0), 'gpode_rollout_jvp: ts_per_traj=-1 (0 one (T,) grid shared, 1 one row of (N,T) per trajectory)'),
    (_rollout(sub=0, N=0, K=0, pack=0), 'gpode_rollout_jvp: substeps=0 (1 ... 64 steps per output interval)'),
    (_rollout(sub=65, N=0, K=0, pack=0), 'gpode_rollout_jvp: substeps=65 (1 ... 64 steps per output interval)'),
    (_rollout(N=0, K=0, pack=0), 'gpode_rollout_jvp: N=0 T=3 draws=1'),
    (_rollout(T=0, K=0, pack=0), 'gpode_rollout_jvp: N=2 T=0 draws=1'),
    (_rollout(nd=0, K=0, pack=0), 'gpode_rollout_jvp: N=2 T=3 draws=0'),
    (_rollout(K=0, pack=0), 'gpode_rollout_jvp: K=0 (1 ... 64 tangent directions per row)'),
    (_rollout(K=65, pack=0), 'gpode_rollout_jvp: K=65 (1 ... 64 tangent directions per row)'),
    (_rollout(pack=0), 'gpode_rollout_jvp: null pointer'),
    (_rollout(z0=0), 'gpode_rollout_jvp: null pointer'),
    (_rollout(ts=0), 'gpode_rollout_jvp: null pointer'),
    (_rollout(vt=0), 'gpode_rollout_jvp: null pointer'),
    (_rollout(v0=0, K=5, Di=7, Do=5), 'gpode_rollout_jvp: NULL directions are the identity and need K == Di (K=5 Di=7)'),
    (_rollout(Di=7, Do=5, order=3), 'gpode_rollout_jvp: no specialisation for kernel=0 Di=7 Do=5'),
    (_rollout(kernel=1, Di=6, Do=3, order=3), 'gpode_rollout_jvp: no specialisation for kernel=1 Di=6 Do=3'),
    (_rollout(N=1 << 30, order=3), 'gpode_rollout_jvp: 1073741824 rows x 3 directions do not fit one launch'),
    (_rollout(order=3), 'gpode_rollout_jvp: order=3 needs Di == order*Do (Di=6 Do=6)'),
    (_rollout(order=2), 'gpode_rollout_jvp: order=2 needs Di == order*Do (Di=6 Do=6)'),
    (_rollout(order=1, Di=6, Do=3), 'gpode_rollout_jvp: order=1 needs Di == order*Do (Di=6 Do=3)'),
]
RHS = [
    (_rhs(mode=3, xpd=2, R=0, K=0, pack=0), 'gpode_rhs_jvp: mode=3 (0 full, 1 prior, 2 update)'),
    (_rhs(mode=-1, xpd=2, R=0, K=0, pack=0), 'gpode_rhs_jvp: mode=-1 (0 full, 1 prior, 2 update)'),
    (_rhs(xpd=2, R=0, K=0, pack=0), 'gpode_rhs_jvp: x_per_draw=2 (0 shared, 1 one (R,Di) slab per draw)'),
    (_rhs(R=0, K=0, pack=0), 'gpode_rhs_jvp: R=0 draws=1'),
    (_rhs(nd=70000, K=0, pack=0), 'gpode_rhs_jvp: R=2 draws=70000'),
    (_rhs(K=0, pack=0), 'gpode_rhs_jvp: K=0 (1 ... 64 tangent directions per row)'),
    (_rhs(K=65, pack=0), 'gpode_rhs_jvp: K=65 (1 ... 64 tangent directions per row)'),
    (_rhs(pack=0), 'gpode_rhs_jvp: null pointer'),
    (_rhs(x=0), 'gpode_rhs_jvp: null pointer'),
    (_rhs(jv=0), 'gpode_rhs_jvp: null pointer'),
    (_rhs(v=0, K=5), 'gpode_rhs_jvp: NULL directions are the identity and need K == Di (K=5 Di=6)'),
    (_rhs(Di=7, Do=5), 'gpode_rhs_jvp: no specialisation for kernel=0 Di=7 Do=5'),
    (_rhs(kernel=2), 'gpode_rhs_jvp: no specialisation for kernel=2 Di=6 Do=6'),
    (_rhs(R=1 << 30), 'gpode_rhs_jvp: 1073741824 rows x 3 directions do not fit one launch'),
]
CASES = [('gpode_rollout_jvp', a, t) for a, t in ROLLOUT] + [('gpode_rhs_jvp', a, t) for a, t in RHS]


@pytest.mark.skipif(torch.cuda.is_available(), reason='the pointers are host addresses: with a GPU present a refusal that got lost would '
                    'launch a kernel on host memory (tests/test_gpu_tangent.py holds the refusals there, on device buffers)')
@pytest.mark.parametrize('name,args,text', CASES, ids=['%s-%d' % (c[0][6:], i) for i, c in enumerate(CASES)])
def test_refusal_text_and_code(name, args, text):
    lib = _lib.load()
    before = bytes(_BUF.raw)
    assert getattr(lib, name)(*args) == 1
    assert lib.gpode_last_error().decode() == text
    assert bytes(_BUF.raw) == before                                             # nothing written


def test_no_refusal_text_is_the_runtimes_and_no_case_repeats():
    for _, _, text in CASES:
        assert 'launch failed' not in text and 'hip' not in text.lower(), text
    assert len(set((c[0], c[1]) for c in CASES)) == len(CASES)
    assert len(DOPRI5) < 512 and math.isfinite(len(DOPRI5))


def test_the_two_exports_are_declared_bound_and_exported():
    """tests/test_cabi_exports.py holds header, table and library to each other; this names the two new entries"""
    import test_cabi_exports as X
    protos = X.header_prototypes()
    for name in ('gpode_rhs_jvp', 'gpode_rollout_jvp'):
        assert name in protos and name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert protos['gpode_rhs_jvp'] == ('int', ['int'] * 6 + ['float*', 'float*', 'int', 'float*', 'int', 'int', 'float*', 'float*', 'int', 'void*'])
    assert protos['gpode_rollout_jvp'] == ('int', ['int'] * 8 + ['float*', 'float*', 'int', 'float*', 'int', 'float*', 'int', 'int', 'int', 'int',
                                                                   'float*', 'float*', 'void*'])
    assert X.signature_mismatches(_lib.SIGNATURES, protos) == []
