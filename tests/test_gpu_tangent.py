"""GPU: the tangent-linear rollout and J_f v -- gpode_rollout_jvp / gpode_rhs_jvp (csrc/gp_tangent.hip), ops.rollout_jvp / rhs_jvp /
rhs_jacobian, SVGP_Layer.jacobian / divergence, Flow.sensitivity -- against the fp64 oracle differentiated by torch on the cache the
GPU built (tests/tangent_ref.py), against reverse mode (rollout_bwd, rhs_vjp), and against itself to the bit.

Bound (tangent_ref.bound): relerr(X_hip, X_64) <= 2e-5 + 3 relerr(X_32, X_64) for every output; no floor is raised.  Every figure
is printed before it is asserted.  Every launch that is compared writes into NaN-filled buffers with integrator_routes.GUARD NaN
floats behind each: a NaN left in an output, or a guard that changed, fails the case.

Cases R_(Di,Do,order,M,S,N,method,T) / D_(D,M,S,N,method,T) of integrator_routes, each the smallest shape at which something specific
can go wrong (see CASES); all on the non-uniform TS of that module, identity directions unless said otherwise."""
import functools

import pytest
import torch

import integrator_routes as IR
import tangent_ref as TR
from integrator_routes import D_, R_, relerr

pytestmark = pytest.mark.gpu

CASES = [
    R_(6, 6, 1, 100, 256, 5, 'rk4'),
    R_(6, 3, 2, 17, 33, 5, 'rk4'),                   # order 2
    R_(16, 8, 2, 40, 64, 5, 'euler'),
    R_(16, 16, 1, 40, 64, 5, 'rk4'),                 # the widest, for registers
    R_(3, 3, 1, 100, 200, 5, 'midpoint'),            # an odd width
    R_(6, 6, 1, 65, 193, 5, 'rk4'),                  # one live lane in the last group of each
    D_(6, 100, 256, 5, 'rk4'),
    D_(4, 16, 64, 5, 'euler'),
    D_(7, 65, 100, 5, 'midpoint'),                   # odd and ragged
    D_(16, 24, 64, 5, 'rk4', T=2),                   # the widest: df_ind_jvp's two column halves (D > 8)
    D_(9, 24, 64, 5, 'midpoint'),                    # the smallest width on that path, and odd: the upper half has one column less
]
BIG = R_(6, 6, 1, 64, 128, 1366, 'euler', T=2)       # K = 6: 8196 wavefront rows, four take a second trip of the grid-stride loop


def _lib_():
    from vae_gp_ode_amd import _lib
    return _lib.load()


def _tag():
    return _lib_().gpode_last_launch().decode()


@functools.lru_cache(maxsize=None)
def built(c):
    """(GPU cache, its oracle dicts, z0, ts) of a case, built once"""
    p, nz, z0, ts, _ = IR.inputs(c)
    dev_in = ({k: v.cuda() for k, v in p.items()}, {k: v.cuda() for k, v in nz.items()})
    k = IR.build(c, dev_in)
    return k, IR.cache_dicts(c, k, dev_in), z0, ts


def launch(k, c, z0, ts, v0=None, K=None, sub=1, method=None, order=None, want_zt=True):
    """gpode_rollout_jvp on guarded NaN buffers -> rc, zt, vt, what went wrong with the buffers, tag"""
    from vae_gp_ode_amd.ops import KERNEL_ID, METHOD_ID, _ptr, _stream
    method = c.method if method is None else method
    N, T = z0.shape[-2], ts.shape[-1]
    K = (v0.shape[-2] if v0 is not None else c.Di) if K is None else K
    rows = min(max(K, 1), 64)
    zt, gz = IR._guarded(k.nd, N, T, c.Di)
    vt, gv = IR._guarded(k.nd, N, T, rows, c.Di)
    rc = _lib_().gpode_rollout_jvp(KERNEL_ID[c.kernel], c.order if order is None else order, METHOD_ID.get(method, method), c.Di, c.Do, k.M, k.S,
                                   k.nd, _ptr(k.pack), _ptr(z0), int(z0.dim() == 3), _ptr(v0), K, _ptr(ts), int(ts.dim() == 2), sub, N, T,
                                   _ptr(zt) if want_zt else None, _ptr(vt), _stream())
    torch.cuda.synchronize()
    bad = [n for n, g in (('zt guard', gz), ('vt guard', gv)) if not torch.isnan(g).all()]
    if rc == 0:
        bad += [n for n, t in (('zt', zt), ('vt', vt)) if torch.isnan(t).any() and (want_zt or n != 'zt')]
    return rc, zt, vt, bad, _tag()


def check_rollout(c, k, cache, z0, ts, v0=None, sub=1, what=''):
    from vae_gp_ode_amd import ops
    zd, td, vd = z0.cuda(), ts.cuda(), (None if v0 is None else v0.cuda())
    rc, zt, vt, bad, tag = launch(k, c, zd, td, vd, sub=sub)
    assert rc == 0, _lib_().gpode_last_error()
    assert tag == 'rollout_jvp_%s_stream' % c.kernel.lower(), tag
    assert not bad, (IR.case_id(c), what, bad)
    (z64, v64), (z32, v32) = (TR.rollout(cache, c.order, c.method, dt, z0, ts, v0, sub) for dt in (torch.float64, torch.float32))
    own = ops.rollout(k, zd, td, c.order, c.method, substeps=sub).view_as(zt)
    figs = dict(vt=(relerr(vt, v64), relerr(v32, v64)), zt=(relerr(zt, z64), relerr(z32, z64)), zt_vs_rollout=(relerr(zt, own), relerr(z32, z64)))
    print('%s %s hip / fp32-oracle relerr to fp64: %s' % (IR.case_id(c), what, ', '.join('%s %.1e/%.1e' % ((n,) + e) for n, e in figs.items())))
    miss = {n: (e, TR.bound(e32)) for n, (e, e32) in figs.items() if not e <= TR.bound(e32)}
    assert not miss, (IR.case_id(c), what, miss)
    return zt, vt


# ---- 1. Phi and J against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', CASES, ids=IR.case_id)
def test_rollout_jvp_against_the_oracle(c):
    k, cache, z0, ts = built(c)
    _, vt = check_rollout(c, k, cache, z0, ts)
    assert torch.equal(vt[:, :, 0].cpu(), TR.identity((1, c.N), c.Di))           # vt[., ., 0] = v0


@pytest.mark.parametrize('c', CASES, ids=IR.case_id)
def test_jacobian_against_the_oracle_and_against_reverse_mode(c):
    """modes 0, 1, 2 against the Jacobians of O.gp_forward / gp_prior / gp_update; f against ops.rhs to the bound; mode 0 also against the
    matrix stacked from ops.rhs_vjp with unit adjoints"""
    from oracle import gpode_oracle as O
    from vae_gp_ode_amd import ops
    k, cache, z0, _ = built(c)
    x = z0.cuda()
    figs = {}
    for mode in (0, 1, 2):
        f, jv = ops.rhs_jvp(k, x, mode=mode)
        assert _tag() == 'rhs_jvp_%s_stream' % c.kernel.lower()
        J = ops.rhs_jacobian(k, x, mode=mode)
        assert J.shape == (c.N, c.Do, c.Di) and torch.equal(J, jv.transpose(-1, -2))
        J64, J32 = TR.jacobian(cache[0], z0, torch.float64, mode), TR.jacobian(cache[0], z0, torch.float32, mode)
        f64 = getattr(O, TR.PARTS[mode])(z0.double(), TR.in_dtype(cache[0], torch.float64))
        figs['J%d' % mode] = (relerr(J, J64), relerr(J32, J64))
        figs['f%d' % mode] = (relerr(f, f64), relerr(ops.rhs(k, x, mode=mode), f64))         # f: the existing kernel's own error as the yardstick
        if mode == 0:
            rev = torch.stack([ops.rhs_vjp(k, x, torch.eye(c.Do, device='cuda')[d].expand(c.N, c.Do).contiguous()) for d in range(c.Do)], 1)
            figs['J0_vs_vjp'] = (relerr(J, rev), relerr(J32, J64))
    print('%s hip / yardstick relerr: %s' % (IR.case_id(c), ', '.join('%s %.1e/%.1e' % ((n,) + e) for n, e in figs.items())))
    miss = {n: (e, TR.bound(e32)) for n, (e, e32) in figs.items() if not e <= TR.bound(e32)}
    assert not miss, (IR.case_id(c), miss)


def test_two_draws_and_an_initial_state_per_draw():
    c = R_(6, 6, 1, 100, 256, 5, 'rk4', nd=2)
    k, cache, z0, ts = built(c)
    assert k.nd == 2 and k.stacked
    check_rollout(c, k, cache, z0, ts, what='nd=2')
    g = torch.Generator().manual_seed(5)
    z0d, v0d = torch.stack([z0, z0 + 0.3 * torch.randn(z0.shape, generator=g)]), torch.randn(2, c.N, 3, c.Di, generator=g)
    check_rollout(c, k, cache, z0d, ts, v0d, what='z0 and v0 per draw, K=3')


def test_two_draws_on_the_divergence_free_kernel():
    c = D_(6, 100, 256, 5, 'euler', nd=2)
    k, cache, z0, ts = built(c)
    check_rollout(c, k, cache, z0, ts, what='nd=2')


@pytest.mark.parametrize('c', [R_(6, 6, 1, 100, 256, 5, 'rk4'), D_(7, 65, 100, 5, 'midpoint')], ids=IR.case_id)
def test_substeps_against_the_oracle_on_the_refined_grid(c):
    k, cache, z0, ts = built(c)
    check_rollout(c, k, cache, z0, ts, sub=3, what='substeps=3')


@pytest.mark.parametrize('c', [R_(6, 3, 2, 17, 33, 5, 'rk4'), D_(6, 100, 256, 5, 'rk4')], ids=IR.case_id)
def test_a_time_grid_per_trajectory(c):
    k, cache, z0, ts = built(c)
    rows = (ts[None, :] * (1 + 0.25 * torch.arange(c.N)[:, None].float())).contiguous()     # rows differ
    check_rollout(c, k, cache, z0, rows, what='(N,T) grid')


def test_rows_past_one_trip_of_the_grid():
    c = BIG
    assert c.N * c.Di == 8196 and c.N * c.Di > 2048 * 4
    k, cache, z0, ts = built(c)
    check_rollout(c, k, cache, z0, ts, what='8196 rows')


def _layer(kernel, Di, Do, M, S, seed, shared=True):
    from oracle import gpode_oracle as O
    from vae_gp_ode_amd.model.core.svpy import SVGP_Layer
    import numpy as np
    state = np.random.get_state()
    np.random.seed(seed)
    gp = SVGP_Layer(Di, Do, M, S, kernel=kernel).cuda()
    np.random.set_state(state)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        ell = gp.kern.unconstrained_lengthscales
        ell.copy_(O.invsoftplus(torch.full(ell.shape, 2.0) if shared else 2.0 * (1 + 0.05 * torch.rand(ell.shape, generator=g))))
        gp.kern.unconstrained_variance.fill_(O.invsoftplus(torch.tensor(1.0)).item())
        gp.inducing_loc.optvar.copy_(2.0 * torch.randn(M, Di, generator=g))
    nz = dict(rff_w=torch.randn(S if kernel == 'RBF' else 2 * S, Do, generator=g), rff_eps=torch.randn(Di, S, Do, generator=g),
              rff_u=torch.rand(1, S, Do, generator=g), eps_u=torch.randn(M, Do, generator=g))
    return gp, nz


def layer_cache_dict(gp):
    """what tangent_ref takes, from the cache the layer built last (a zero-padded width: the real rows and columns of it)"""
    k, Di, Do = gp.cache, gp.D_in, gp.D_out
    assert not k.stacked
    if gp.kernel_n == 'RBF':
        return dict(kernel='RBF', S=k.S, omega=k.omega[:Di, :, :Do].cpu(), phase=k.phase[..., :Do].cpu(), w=k.noise['rff_w'][:, :Do].cpu(),
                    var=k.var[:Do].cpu(), Z=gp.inducing_loc.optvar.detach().cpu(), nu=k.nu[:Do].cpu(), ell=k.ell[:Do, :Di].cpu())
    return dict(kernel='DF', S=k.S, omega=k.omega.cpu(), phase=k.phase.cpu(), w=k.noise['rff_w'].cpu(), var=k.var.cpu(),
                Z=gp.inducing_loc.optvar.detach().cpu(), nu=k.nu.cpu(), ell=k.ell.cpu())


def test_a_width_that_is_not_compiled_goes_through_the_pad():
    """RBF width 5, evaluated zero-padded at 6: Flow.sensitivity, SVGP_Layer.jacobian and divergence against the oracle at width 5"""
    from vae_gp_ode_amd.model.core.flow import Flow
    gp, nz = _layer('RBF', 5, 5, 20, 48, 3, shared=False)
    assert gp.width_pad is not None and gp.width_pad.Dip == 6
    flow = Flow(gp, order=1, solver='rk4')
    g = torch.Generator().manual_seed(4)
    z0, ts = torch.randn(5, 5, generator=g), torch.tensor(IR.TS[3])
    gp.set_noise(nz)
    zt, Phi = flow.sensitivity(z0.cuda(), ts.cuda())
    assert _tag() == 'rollout_jvp_rbf_stream' and zt.shape == (5, 3, 5) and Phi.shape == (5, 3, 5, 5)
    cache = [layer_cache_dict(gp)]
    (z64, v64), (z32, v32) = (TR.rollout(cache, 1, 'rk4', dt, z0, ts) for dt in (torch.float64, torch.float32))
    v0 = torch.randn(5, 2, 5, generator=g)
    _, vt = flow.sensitivity(z0.cuda(), ts.cuda(), v0=v0.cuda(), cache=gp.cache)
    (_, w64), (_, w32) = (TR.rollout(cache, 1, 'rk4', dt, z0, ts, v0) for dt in (torch.float64, torch.float32))
    J, div = gp.jacobian(z0.cuda()), gp.divergence(z0.cuda())
    J64, J32 = TR.jacobian(cache[0], z0, torch.float64), TR.jacobian(cache[0], z0, torch.float32)
    figs = dict(Phi=(relerr(Phi.transpose(-1, -2), v64[0]), relerr(v32, v64)), zt=(relerr(zt, z64[0]), relerr(z32, z64)),
                vt=(relerr(vt, w64[0]), relerr(w32, w64)), J=(relerr(J, J64), relerr(J32, J64)))
    print('width 5 through the pad: ' + ', '.join('%s %.1e/%.1e' % ((n,) + e) for n, e in figs.items()))
    assert J.shape == (5, 5, 5) and torch.equal(div, J.diagonal(dim1=-2, dim2=-1).sum(-1))
    assert not {n: e for n, (e, e32) in figs.items() if not e <= TR.bound(e32)}


# ---- 2. forward mode against reverse mode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [R_(6, 6, 1, 100, 256, 5, 'rk4'), D_(6, 100, 256, 5, 'rk4'), R_(6, 3, 2, 17, 33, 5, 'rk4')], ids=IR.case_id)
def test_tangent_is_the_transpose_of_the_reverse_sweep(c):
    """sum_t <gw_t, vt_t> = <gz0, v0> per trajectory and column, gz0 from ops.rollout's record and ops.rollout_bwd; relative to
    sum_t |gw_t| |vt_t|, within 2e-5 + 3 x the same defect of the fp32 oracle (forward against reverse mode of torch)"""
    from vae_gp_ode_amd import ops
    k, cache, z0, ts = built(c)
    gw = IR.inputs(c)[4]
    v0 = torch.randn(c.N, 3, c.Di, generator=torch.Generator().manual_seed(9))
    _, vt = ops.rollout_jvp(k, z0.cuda(), ts.cuda(), c.order, c.method, v0=v0.cuda())
    _, xs = ops.rollout(k, z0.cuda(), ts.cuda(), c.order, c.method, save_stages=True)
    gz0, _ = ops.rollout_bwd(k, xs, gw[0].cuda(), ts.cuda(), c.order, c.method)
    d, d32 = TR.defect(gz0, v0, gw[0], vt), TR.transpose_defect(cache, c.order, c.method, torch.float32, z0, ts, v0, gw)
    print('%s <gz0, v0> against sum_t <gw_t, vt_t>: %.1e (fp32 oracle %.1e)' % (IR.case_id(c), d, d32))
    assert d <= TR.bound(d32)


# ---- 3. exact properties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [R_(6, 6, 1, 100, 256, 5, 'rk4'), D_(7, 65, 100, 5, 'midpoint'), R_(6, 3, 2, 17, 33, 5, 'rk4')], ids=IR.case_id)
def test_exact_properties(c):
    k, _, z0, ts = built(c)
    zd, td, D = z0.cuda(), ts.cuda(), c.Di
    rc, zt, vt, bad, _ = launch(k, c, zd, td)
    assert rc == 0 and not bad                                                   # outputs past the ends of the buffers untouched
    # NULL directions are an explicit identity
    eye = TR.identity((c.N,), D).cuda()
    rc, zt_e, vt_e, bad, _ = launch(k, c, zd, td, eye)
    assert rc == 0 and not bad and torch.equal(vt, vt_e) and torch.equal(zt, zt_e)
    # one launch with K columns is K launches of one column each, and the primal does not depend on K
    for col in range(D):
        rc, zt_1, vt_1, bad, _ = launch(k, c, zd, td, eye[:, col:col + 1].contiguous())
        assert rc == 0 and not bad and torch.equal(vt_1[:, :, :, 0], vt[:, :, :, col]) and torch.equal(zt_1, zt)
    # zt may be left out
    rc, zt_n, vt_n, bad, _ = launch(k, c, zd, td, want_zt=False)
    assert rc == 0 and not bad and torch.isnan(zt_n).all() and torch.equal(vt_n, vt)
    # an (N,T) grid with identical rows is the shared grid
    rc, zt_r, vt_r, bad, _ = launch(k, c, zd, td.expand(c.N, -1).contiguous())
    assert rc == 0 and not bad and torch.equal(vt_r, vt) and torch.equal(zt_r, zt)
    # a second run gives the same bits
    rc, zt_2, vt_2, bad, _ = launch(k, c, zd, td)
    assert torch.equal(vt_2, vt) and torch.equal(zt_2, zt)


# ---- 4. what it is for -----------------------------------------------------------------------------------------------------------------
def test_df_update_term_is_divergence_free_and_the_sampled_field_is_not():
    """DF with shared hyper-parameters: K(x,Z) nu is divergence-free as written (the oracle: 1e-15), so |divergence(x, 'update')| must
    vanish within the bound on J -- (2e-5 + 3 relerr32) D max|J| -- while divergence(x, 'full') must MATCH the oracle's non-zero value:
    the random-feature prior term of the reference's formulas is not divergence-free."""
    D = 6
    gp, nz = _layer('DF', D, D, 100, 256, 11)
    gp.build_cache(noise=nz)
    x = torch.randn(5, D, generator=torch.Generator().manual_seed(12))
    cd = layer_cache_dict(gp)
    Ju, Ju64, Ju32 = gp.jacobian(x.cuda(), 'update'), TR.jacobian(cd, x, torch.float64, 2), TR.jacobian(cd, x, torch.float32, 2)
    du, du64 = gp.divergence(x.cuda(), 'update'), Ju64.diagonal(dim1=-2, dim2=-1).sum(-1)
    tol = TR.bound(relerr(Ju32, Ju64), D * Ju64.abs().max().item())
    print('update: max|div| %.2e (oracle %.2e), max|J| %.3f, tolerance %.2e' % (du.abs().max(), du64.abs().max(), Ju64.abs().max(), tol))
    assert du64.abs().max() < 1e-12 and du.abs().max().item() <= tol
    Jf64, Jf32 = TR.jacobian(cd, x, torch.float64, 0), TR.jacobian(cd, x, torch.float32, 0)
    df, df64, df32 = gp.divergence(x.cuda()), Jf64.diagonal(dim1=-2, dim2=-1).sum(-1), Jf32.diagonal(dim1=-2, dim2=-1).sum(-1)
    print('full: divergence %s, oracle %s; max|J| %.3f' % (df.cpu().tolist(), df64.tolist(), Jf64.abs().max()))
    assert df64.abs().max() > 0.1 * Jf64.abs().max()                             # the finding: far from zero
    assert relerr(df, df64) <= TR.bound(relerr(df32, df64))
    assert relerr(gp.divergence(x.cuda(), 'prior'), df64 - du64) <= TR.bound(relerr(df32, df64))


def test_mean_field_of_the_df_kernel_preserves_volume():
    """Under mean_noise() (no prior term) with shared hyper-parameters, rk4 over 16 steps of 0.1: |logdet Phi_T| within the same
    tolerance scaled by T D of the fp64 oracle's value for that grid (computed here: the discrete map is volume-preserving only to
    the solver's order)."""
    from vae_gp_ode_amd import evaluate as E
    from vae_gp_ode_amd.model.core.flow import Flow
    D, T = 6, 17
    gp, _ = _layer('DF', D, D, 100, 256, 11)
    flow = Flow(gp, order=1, solver='rk4')
    z0, ts = torch.randn(5, D, generator=torch.Generator().manual_seed(13)), 0.1 * torch.arange(T, dtype=torch.float32)
    cache = gp.build_cache(noise=gp.mean_noise())
    zt, Phi = flow.sensitivity(z0.cuda(), ts.cuda(), cache=cache)
    cd = [layer_cache_dict(gp)]
    (_, v64), (_, v32) = (TR.rollout(cd, 1, 'rk4', dt, z0, ts) for dt in (torch.float64, torch.float32))
    ld, ld64 = E.flow_logdet(Phi)[:, -1], E.flow_logdet(v64[0].transpose(-1, -2))[:, -1]
    tol = TR.bound(relerr(v32, v64), T * D)
    print('logdet Phi_T: %s; fp64 oracle %s; tolerance %.2e; Phi %.1e from fp64 (fp32 oracle %.1e)'
          % (ld.tolist(), ld64.tolist(), tol, relerr(Phi.transpose(-1, -2), v64[0]), relerr(v32, v64)))
    assert ld64.abs().max() < 1e-6                                               # the oracle: volume-preserving to rk4's order on this grid
    assert (ld - ld64).abs().max().item() <= tol and ld.abs().max().item() <= tol + ld64.abs().max().item()
    assert relerr(Phi.transpose(-1, -2), v64[0]) <= TR.bound(relerr(v32, v64))


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    c = R_(6, 6, 1, 100, 256, 5, 'rk4')
    k, _, z0, ts = built(c)
    zd, td = z0.cuda(), ts.cuda()
    for kw, words in ((dict(method='dopri5'), 'its steps depend on the state through the controller, and the tangent of the accepted-step '
                                               'sequence is not built'),
                      (dict(K=0), 'K=0 (1 ... 64 tangent directions per row)'),
                      (dict(K=5), 'NULL directions are the identity and need K == Di (K=5 Di=6)'),
                      (dict(sub=65), 'substeps=65'), (dict(order=2), 'order=2 needs Di == order*Do')):
        rc, zt, vt, bad, _ = launch(k, c, zd, td, **kw)
        err = _lib_().gpode_last_error().decode()
        assert rc == 1 and err.startswith('gpode_rollout_jvp: ') and words in err, (kw, err)
        assert not bad and torch.isnan(zt).all() and torch.isnan(vt).all(), kw
    from vae_gp_ode_amd import _lib, ops
    with pytest.raises(_lib.GpodeError, match='controller'):
        ops.rollout_jvp(k, zd, td, 1, 'dopri5')
    with pytest.raises(_lib.GpodeError, match='K=65'):
        ops.rollout_jvp(k, zd, td, 1, 'rk4', v0=torch.zeros(5, 65, 6, device='cuda'))
    with pytest.raises(_lib.GpodeError, match='mode'):
        ops.rhs_jvp(k, zd, mode=3)
