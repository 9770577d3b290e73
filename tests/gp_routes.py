"""Every route of the GP cache build (csrc/gp_cache.hip cache_build_fwd), of its backward (csrc/gp_cache_bwd.hip cache_bwd_prepare,
cache_build_bwd), of kern.compute_nu and of build_conditional, shared by test_gpu_gp_routes.py and by the child processes it starts.

A case is (kernel, Di, Do, M, nd): the kernel family, the widths, the inducing points and the Monte-Carlo draws that share the factor.
A mode is how the process is switched:

  default       no switch
  never         ops.set_backward_solves('never')   (what GPODE_BWD_EXPLICIT_INVERSE=1 selects at start-up)
  always        ops.set_backward_solves('always')  (what main.py --backward_solves adaptive selects once the pivots span 200 x)
  draw_chain    GPODE_DRAW_CHAIN=1                 the three switches that are read once per process: every case of such a mode
  small_factor  GPODE_SMALL_FACTOR_KERNELS=1       runs in ONE fresh child process (`python gp_routes.py <mode> <file>`), which
  env_solves    GPODE_BWD_SOLVES=1                 saves its outputs to a file

expected() restates the thresholds of the dispatch on its own (it never asks the library); run_case() drives the C ABI on buffers it
owns -- NaN-filled, the two workspaces exactly as long as the size queries say with GUARD NaN floats behind them -- and returns the
outputs, the tags gpode_last_launch() gave after build, prepare and backward, and what the buffer checks found; reference() is the
oracle in fp64 and, for the bounds, in fp32 on the same parameters and noise."""
import collections
import contextlib
import ctypes
import functools
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
S, N, T, METHOD = 32, 4, 3, 'euler'
Case = collections.namedtuple('Case', 'kernel Di Do M nd regime', defaults=('base',))     # regime: gp_regimes.TABLE, 'base' = synthetic_gp as it is
C = Case

FWD_TAGS = ('cache build: lds', 'cache build: chain32+deep', 'cache build: chain32+back<1>', 'cache build: chain32+back<2>',
            'cache build: chain32+back<0>', 'cache build: panel')
PREP_TAGS = ('cache bwd prepare: solves', 'cache bwd prepare: inverse32', 'cache bwd prepare: inverse_mfma')
BWD_FAMILY = {'solves': 'cache bwd: solves (k_trsm_slab)', 'inverse32': 'cache bwd: inverse32 (k_linv_dc, k_gemm_phiX)',
              'inverse_mfma': 'cache bwd: inverse_mfma (k_linv_dc_mfma, k_gemm_mfma)'}
BWD_TAGS = tuple('%s, %s' % (t, k) for t in BWD_FAMILY.values() for k in ('rbf', 'df'))
NU_TAGS = ('kern.compute_nu: chain32+deep', 'kern.compute_nu: chain32+back<0>', 'kern.compute_nu: panel')
COND_TAGS = ('conditional: chain32', 'conditional: panel')
REQUIRED_TAGS = FWD_TAGS + PREP_TAGS + BWD_TAGS + NU_TAGS + COND_TAGS

CHILD_ENV = {'draw_chain': 'GPODE_DRAW_CHAIN', 'small_factor': 'GPODE_SMALL_FACTOR_KERNELS', 'env_solves': 'GPODE_BWD_SOLVES'}
SOLVES_MODE = {'default': 'auto', 'never': 'never', 'always': 'always', 'draw_chain': 'auto', 'small_factor': 'auto', 'env_solves': 'always'}


# ---- the dispatch, restated --------------------------------------------------------------------------------------------------------
def geometry(n, extra):
    """(nblk, np) of a factor of n rows with `extra` appended rows: 32-row tiles, whole 128-row panels from 32 tiles on"""
    nblk = -(-(n + extra) // 32)
    if nblk >= 32:
        nblk = (nblk + 3) // 4 * 4
    return nblk, 32 * nblk


def system(c):
    """(n, batch, nblk, np) of case c: RBF factors Do systems of M rows, DF one of M Do"""
    n, batch = (c.M, c.Do) if c.kernel == 'RBF' else (c.M * c.Do, 1)
    return (n, batch) + geometry(n, c.nd)


def draw_lds_bytes(np_, M, Di, nd):
    """the matrix with two pad columns, nd solution vectors, one tile row, Z transposed (row stride M | 1), Di^2 + Di constants"""
    return 4 * (np_ * (np_ + 2) + nd * np_ + 32 + Di * (M | 1) + Di * Di + Di)


def forward_route(n, nblk, np_, mode, lds_fits=False, deep=True):
    if np_ <= 192 and lds_fits and mode != 'draw_chain':
        return 'lds'
    if np_ >= 1024 and np_ % 128 == 0 and mode != 'small_factor':
        return 'panel'
    if deep and np_ <= 1024 and 4 * (np_ + nblk * 32 * 32) <= 150 * 1024:
        return 'chain32+deep'
    cpt = -(-n // 1024)
    return 'chain32+back<%d>' % (cpt if cpt <= 2 else 0)


def backward_route(np_, mode):
    solves = {'auto': np_ <= 192, 'always': np_ <= 1216, 'never': False}[SOLVES_MODE[mode]]
    if solves:
        return 'solves'
    return 'inverse_mfma' if np_ >= 1024 and np_ % 128 == 0 and mode != 'small_factor' else 'inverse32'


def expected(c, mode):
    """the tags after build, prepare and backward of case c in `mode`"""
    n, batch, nblk, np_ = system(c)
    fwd = forward_route(n, nblk, np_, mode, draw_lds_bytes(np_, c.M, c.Di, c.nd) <= 160 * 1024)
    bwd = backward_route(np_, mode)
    return dict(fwd='cache build: ' + fwd, prepare='cache bwd prepare: ' + bwd, bwd='%s, %s' % (BWD_FAMILY[bwd], c.kernel.lower()))


def expected_nu(c, mode):
    n, batch, nblk, np_ = system(c._replace(nd=1))
    r = forward_route(n, nblk, np_, mode)
    return 'kern.compute_nu: ' + ('chain32+back<0>' if r.startswith('chain32+back') else r)     # its copy of the selection has one solve kernel


def expected_conditional(M, Nq, mode='default'):
    nblk, np_ = geometry(M, Nq)
    return 'conditional: ' + ('panel' if forward_route(M, nblk, np_, mode).startswith('panel') else 'chain32')


# ---- the case table ----------------------------------------------------------------------------------------------------------------
LDS_CASES = [C('RBF', 6, 6, 191, 1), C('RBF', 6, 6, 187, 5), C('RBF', 16, 8, 190, 1), C('DF', 6, 6, 31, 5)]
CASES = {
    'default': [C('RBF', 6, 6, 191, 1),       # n + nd = 192: the largest LDS-resident system
                C('RBF', 6, 6, 192, 1),       # 193 rows, np = 224: the chain, 7 tile columns (odd: ends on k_chol_rl)
                C('RBF', 6, 6, 187, 5),       # five rhs rows ending on row 191 ...
                C('RBF', 6, 6, 188, 5),       # ... against opening block 7
                C('RBF', 16, 8, 190, 1),      # np = 192 both; 163 200 B of LDS (fits) ...
                C('RBF', 16, 8, 190, 2),      # ... against 163 968 B (> 163 840): lds against chain on the byte limit alone
                C('DF', 6, 6, 31, 5),         # 191 rows, the same edge for DF
                C('DF', 6, 6, 32, 1),         # 193
                C('DF', 8, 8, 123, 5),        # 989 rows, np = 992: the largest 32-tile chain, 31 columns
                C('DF', 8, 8, 124, 1),        # 993, np = 1024: the smallest panelled factor, n = 992 leaves the last panel partial
                C('RBF', 8, 8, 1000, 1),      # eight batched 1024-row panelled factors
                C('RBF', 8, 8, 1150, 4)],     # rhs rows 1150 .. 1153 straddle the 1152 panel edge, np = 1280
    'never': [C('RBF', 6, 6, 100, 1), C('RBF', 6, 6, 100, 5), C('DF', 6, 6, 31, 5)],     # inverse32 behind k_draw_lds
    'always': [C('DF', 6, 6, 100, 1), C('DF', 6, 6, 100, 5),                             # configs[1]'s system: what adaptive training runs
               C('RBF', 6, 6, 200, 5), C('RBF', 8, 8, 1000, 1),
               C('RBF', 8, 8, 1150, 1),       # np = 1152: the last solves size
               C('RBF', 8, 8, 1150, 4)],      # np = 1280: falls through to inverse_mfma
    'draw_chain': LDS_CASES + [C('RBF', 6, 3, 100, 3)],
    'small_factor': [C('DF', 8, 8, 124, 1),   # np = 1024: the deep back-substitution still fits
                     C('RBF', 8, 8, 1024, 1),  # np = 1152, back<1>
                     C('DF', 16, 16, 72, 2),   # n = 1152, back<2>
                     C('DF', 16, 16, 129, 1)],  # n = 2064, np = 2176, back<0>
    'env_solves': [C('DF', 6, 6, 100, 5)],
}
NU_CASES = [C('RBF', 6, 6, 192, 1), C('DF', 8, 8, 124, 1), C('RBF', 8, 8, 1150, 1)]
COND_N = (892, 893, 1100)                     # M + N = 992: the last 32-tile size; the first panelled; np = 1280


def case_id(c):
    import gp_regimes
    return '%s-%d-%d-M%d-L%d' % c[:5] + gp_regimes.suffix(c.regime)


# ---- inputs, reference -------------------------------------------------------------------------------------------------------------
def inputs(c):
    """parameters of test_gpu_backward.synthetic_gp (widths >= 6: K_uu well conditioned), the noise of nd draws with a leading draw
    axis, initial states, output times and dL/dzt of a loss that is summed over the draws"""
    from test_gpu_backward import synthetic_gp
    import gp_regimes
    p, _, z0, ts, _ = synthetic_gp(c.kernel, c.Di, c.Do, c.M, S, N, T, seed=7000 + c.M + c.Di + 31 * c.Do)
    p, z0, ts = gp_regimes.apply(c.regime, p, z0, c.kernel) + (gp_regimes.times(c.regime, ts),)
    g = torch.Generator().manual_seed(9000 + c.M + 17 * c.nd + c.Di)
    nz = dict(eps_u=torch.randn(c.nd, c.M, c.Do, generator=g), rff_w=torch.randn(c.nd, S if c.kernel == 'RBF' else 2 * S, c.Do, generator=g),
              rff_eps=torch.randn(c.nd, c.Di, S, c.Do, generator=g), rff_u=torch.rand(c.nd, 1, S, c.Do, generator=g))
    return p, nz, z0, ts, torch.randn(c.nd, N, T, c.Di, generator=g)


FWD_KEYS, GRAD_KEYS = ('nu', 'u', 'u_prior', 'zt'), ('raw_ell', 'raw_var', 'Z', 'Um', 'Us', 'z0')
BASE = dict({k: 2e-4 for k in FWD_KEYS}, Lu=1e-4, **{k: 1e-3 for k in GRAD_KEYS})     # the project's bounds: base + 3 relerr(fp32 oracle, fp64)


def _oracle(c, dtype):
    from oracle import gpode_oracle as O
    p, nz, z0, ts, gw = inputs(c)
    q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    z = z0.to(dtype).clone().requires_grad_(True)
    out, loss = collections.defaultdict(list), 0.0
    for l in range(c.nd):                             # every draw with its own oracle build, the loss summed over the draws
        cl = O.build_cache(q, {k: v[l].to(dtype) for k, v in nz.items()}, c.kernel)
        zt = O.flow_forward(z, ts.to(dtype), cl, c.Di // c.Do, METHOD)
        loss = loss + (zt * gw[l].to(dtype)).sum()
        for k in ('nu', 'u', 'u_prior'):
            out[k].append(cl[k].detach())
        out['zt'].append(zt.detach())
    loss.backward()
    r = {k: torch.stack(v) for k, v in out.items()}
    r['Lu'] = cl['Lu'].detach()
    r.update({k: v.grad for k, v in q.items()}, z0=z.grad)
    return r


@functools.lru_cache(maxsize=None)
def reference(c):
    """(the fp64 oracle's results, relerr(fp32 oracle, fp64) per compared quantity, (min, max) of the fp64 factor's diagonal)"""
    from test_gpu_forward import relerr
    r64, r32 = _oracle(c, torch.float64), _oracle(c, torch.float32)
    d = torch.diagonal(r64['Lu'], dim1=-2, dim2=-1)
    return r64, {k: relerr(r32[k], r64[k]) for k in r64}, (float(d.min()), float(d.max()))


@functools.lru_cache(maxsize=None)
def nu_inputs(c):
    """the oracle's fp64 K_uu, f_prior(Z), inducing sample and nu of the case's first draw"""
    from oracle import gpode_oracle as O
    p, nz, _, _, _ = inputs(c)
    cl = O.build_cache(O.to_dtype(p, torch.float64), {k: v[0].double() for k, v in nz.items()}, c.kernel)
    n32 = O.rbf_compute_nu if c.kernel == 'RBF' else O.df_compute_nu
    return cl['Ku'], cl['u_prior'], cl['u'], cl['nu'], n32(cl['Ku'].float(), cl['u_prior'].float(), cl['u'].float())[1]


# ---- launches ----------------------------------------------------------------------------------------------------------------------
def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def _guarded(n):
    """a NaN-filled buffer of exactly n floats with GUARD NaN floats behind it: (the n floats, the guard)"""
    buf = _nan(n + GUARD)
    return buf[:n], buf[n:]


@contextlib.contextmanager
def backward_solves(mode):
    from vae_gp_ode_amd import ops
    if SOLVES_MODE[mode] == 'auto' or mode == 'env_solves':         # env_solves: the process was started in that state
        yield
        return
    ops.set_backward_solves(SOLVES_MODE[mode])
    try:
        yield
    finally:
        ops.set_backward_solves('auto')


def _once(c, dev_in):
    """One build, rollout, reverse sweep and the three forms of the backward (plain, prepared, add_to) of case c."""
    from vae_gp_ode_amd import _lib, ops
    from vae_gp_ode_amd.ops import KERNEL_ID, _ptr, _stream
    lib = _lib.load()
    p, nz, z0, ts, gw = dev_in
    kid, Di, Do, M, nd = KERNEL_ID[c.kernel], c.Di, c.Do, c.M, c.nd
    n, batch, nblk, np_ = system(c)
    dims = (kid, Di, Do, M, S, nd)
    pf, wf, bw = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.call('gpode_cache_sizes_n', *dims, ctypes.byref(pf), ctypes.byref(wf))
    _lib.call('gpode_cache_bwd_sizes_n', *dims, ctypes.byref(bw))
    pf, wf, bw = pf.value, wf.value, bw.value
    lead = (nd,) if nd > 1 else ()

    k = ops.GPCache()
    k.kernel, k.Di, k.Do, k.M, k.S, k.nd, k.stacked, k.prepared = c.kernel, Di, Do, M, S, nd, nd > 1, None
    k.pack = _nan(*lead, pf)
    k.ws, ws_guard = _guarded(wf)
    k.ell, k.var, k.omega, k.phase = _nan(Do, Di), _nan(Do), _nan(*lead, Di, S, Do), _nan(*lead, 1, S, Do)
    k.u, k.u_prior = _nan(*lead, M, Do), _nan(*lead, M, Do)
    k.nu = _nan(*lead, Do, M, 1) if c.kernel == 'RBF' else _nan(*lead, M * Do, 1)
    k.Lu = _nan(batch, n, n) if c.kernel == 'RBF' else _nan(n, n)
    k.noise = {kk: (v if nd > 1 else v[0]) for kk, v in nz.items()}
    _lib.call('gpode_cache_build_fwd_n', *dims, _ptr(p['raw_ell']), _ptr(p['raw_var']), _ptr(p['Z']), _ptr(p['Um']), _ptr(p['Us']),
              _ptr(nz['eps_u']), _ptr(nz['rff_w']), _ptr(nz['rff_eps']), _ptr(nz['rff_u']), _ptr(k.pack), _ptr(k.ws), _ptr(k.ell), _ptr(k.var),
              _ptr(k.omega), _ptr(k.phase), _ptr(k.u), _ptr(k.Lu), _ptr(k.nu), _ptr(k.u_prior), _stream())
    out = dict(tag_fwd=lib.gpode_last_launch().decode())
    torch.cuda.synchronize()
    assert torch.isnan(ws_guard).all(), 'the build wrote past the workspace gpode_cache_sizes_n() sizes'
    try:
        k.check_factorisation()
        out['factorisation'] = 'ok'
    except _lib.GpodeError as e:
        out['factorisation'] = str(e)
    out['pivots'] = k.pivot_range()
    order = Di // Do
    zt, xs = ops.rollout(k, z0, ts, order, METHOD, save_stages=True)
    gz0, ast = ops.rollout_bwd(k, xs, gw if nd > 1 else gw[0], ts, order, METHOD)
    gpack = ops.param_grad(k, xs.reshape(lead + (-1, Di)), ast.reshape(lead + (-1, Do)))
    out.update(nu=k.nu, u=k.u, u_prior=k.u_prior, Lu=k.Lu, zt=zt, z0=gz0.sum(0) if nd > 1 else gz0)

    def backward(flags, bws=None, add_to=None):
        guard = None
        if bws is None:
            bws, guard = _guarded(bw)
        g = dict(raw_ell=_nan(Do, Di), raw_var=_nan(Do), Z=_nan(M, Di), Um=_nan(M, Do), Us=_nan(Do, M * (M + 1) // 2))
        if add_to is not None:
            g['Um'], g['Us'] = add_to[0].clone(), add_to[1].clone()
        gin = gpack.clone()                             # the f_prior(Z) terms are added to it in place
        _lib.call('gpode_cache_build_bwd_n', *dims, _ptr(p['raw_ell']), _ptr(p['raw_var']), _ptr(p['Z']), _ptr(nz['eps_u']), _ptr(k.pack),
                  _ptr(k.ws), _ptr(gin), _ptr(bws), _ptr(g['raw_ell']), _ptr(g['raw_var']), _ptr(g['Z']), _ptr(g['Um']), _ptr(g['Us']),
                  flags, _stream())
        tag = lib.gpode_last_launch().decode()
        torch.cuda.synchronize()
        assert guard is None or torch.isnan(guard).all(), 'the backward wrote past the workspace gpode_cache_bwd_sizes_n() sizes'
        return g, tag

    g, out['tag_bwd'] = backward(0)
    out.update(g)
    # prepared: L^-1 (or the diagonal-block inverses) from cache_bwd_prepare, then the backward on that workspace -- the same bits
    bws, guard = _guarded(bw)
    _lib.call('gpode_cache_bwd_prepare_n', *dims, _ptr(k.ws), _ptr(bws), _stream())
    out['tag_prepare'] = lib.gpode_last_launch().decode()
    gp, tag = backward(1, bws=bws)
    assert torch.isnan(guard).all(), 'prepare + backward wrote past the workspace gpode_cache_bwd_sizes_n() sizes'
    assert tag == out['tag_bwd'], (tag, out['tag_bwd'])
    out['prepared_differs'] = [kk for kk in g if not torch.equal(g[kk], gp[kk])]
    # add_to: the gradient is added to tensors that hold one already (scaled like the plain result: the sum then rounds at its size)
    gen = torch.Generator().manual_seed(5)
    have = [(torch.randn(g[kk].shape, generator=gen).cuda() * g[kk].abs().max()) for kk in ('Um', 'Us')]
    ga, tag = backward(2, add_to=have)
    assert tag == out['tag_bwd'], (tag, out['tag_bwd'])
    out['add_to'] = {kk: float(((ga[kk].double() - (h.double() + g[kk].double())).abs().max() / g[kk].double().abs().max()).item())
                     for kk, h in zip(('Um', 'Us'), have)}
    out['add_to_rest_differs'] = [kk for kk in ('raw_ell', 'raw_var', 'Z') if not torch.equal(g[kk], ga[kk])]
    assert torch.isnan(ws_guard).all(), 'the backward wrote past the forward workspace'
    return {kk: (v.cpu() if torch.is_tensor(v) else v) for kk, v in out.items()}


def run_case(c, mode='default'):
    """Case c TWICE in the process's switch state and the backward mode of `mode`; the second run must be bit-identical."""
    p, nz, z0, ts, gw = inputs(c)
    dev_in = ({k: v.cuda() for k, v in p.items()}, {k: v.cuda() for k, v in nz.items()}, z0.cuda(), ts.cuda(), gw.cuda())
    with backward_solves(mode):
        a, b = _once(c, dev_in), _once(c, dev_in)
    a['second_run_differs'] = [k for k in a if not (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k])]
    return a


def run_nu(c):
    """ops.compute_nu on the oracle's fp64 K_uu (cast to fp32), f_prior(Z) and inducing sample: (nu, tag, status word)"""
    from vae_gp_ode_amd import _lib, ops
    Ku, u_prior, u, _, _ = nu_inputs(c)
    nu, ws = ops.compute_nu(c.kernel, c.Di, c.Do, Ku.float().cuda(), u_prior.float().cuda(), u.float().cuda())
    tag = _lib.load().gpode_last_launch().decode()
    info = ctypes.c_int(0)
    _lib.call('gpode_cache_info', ops._ptr(ws), ctypes.byref(info), ops._stream())
    return nu.cpu(), tag, info.value


# ---- comparison --------------------------------------------------------------------------------------------------------------------
def check_case(c, mode, got, seen=None, maxima=None):
    """got (run_case, or a child's record of it) against the dispatch table and the fp64 oracle; prints every figure before it asserts"""
    from test_gpu_forward import relerr
    assert not isinstance(got, str), (case_id(c), mode, got)
    want = expected(c, mode)
    tags = dict(fwd=got['tag_fwd'], prepare=got['tag_prepare'], bwd=got['tag_bwd'])
    print('%s [%s] %s' % (case_id(c), mode, tags))
    if seen is not None:
        seen.update(tags.values())
    assert tags == want, (case_id(c), mode, tags, want)                                                   # (a)
    r64, e32, (lo64, hi64) = reference(c)
    errs = {k: relerr(got[k], r64[k].reshape(got[k].shape)) for k in BASE}
    print('  hip / fp32-oracle relerr to fp64: ' + ', '.join('%s %.1e/%.1e' % (k, errs[k], e32[k]) for k in BASE))
    if maxima is not None:
        for t, keys in ((tags['fwd'], FWD_KEYS + ('Lu',)), (tags['bwd'], GRAD_KEYS)):
            maxima[t] = max(maxima.get(t, 0.0), max(errs[k] for k in keys))
    lo, hi = got['pivots']
    scale = float(r64['Lu'].abs().max())
    print('  pivots (%.6g, %.6g), fp64 (%.6g, %.6g); add_to %s' % (lo, hi, lo64, hi64, got['add_to']))
    assert all(e32[k] < 1e-4 for k in BASE), ('the inputs are not well conditioned', case_id(c), e32)       # (c)
    bad = {k: (errs[k], BASE[k] + 3 * e32[k]) for k in BASE if not errs[k] < BASE[k] + 3 * e32[k]}
    assert not bad, (case_id(c), mode, bad)                                                                # (b)
    assert not got['second_run_differs'], (case_id(c), mode, got['second_run_differs'])                     # (d)
    assert not got['prepared_differs'], (case_id(c), mode, 'prepared', got['prepared_differs'])             # (e)
    assert not got['add_to_rest_differs'] and all(v <= 1e-6 for v in got['add_to'].values()), (case_id(c), mode, got['add_to'])
    assert got['factorisation'] == 'ok', got['factorisation']                                               # (f)
    # (g) the pivots are entries of Lu: the Lu bound, which is relative to the largest entry of Lu, holds for them as absolute errors
    tol = (BASE['Lu'] + 3 * e32['Lu']) * scale
    assert abs(lo - lo64) < tol and abs(hi - hi64) < tol, (case_id(c), (lo, hi), (lo64, hi64), tol)


def check_nu(c, mode, got, seen=None, maxima=None):
    from test_gpu_forward import relerr
    assert not isinstance(got, str), (case_id(c), mode, got)
    nu, tag, info = got
    _, _, _, nu64, nu32 = nu_inputs(c)
    e, e32 = relerr(nu, nu64.reshape(nu.shape)), relerr(nu32, nu64)
    print('%s [%s] %s: nu hip / fp32-oracle relerr to fp64 %.1e/%.1e' % (case_id(c), mode, tag, e, e32))
    if seen is not None:
        seen.add(tag)
    if maxima is not None:
        maxima[tag] = max(maxima.get(tag, 0.0), e)
    assert tag == expected_nu(c, mode), (tag, expected_nu(c, mode))
    assert not info & 1, 'a positive definite matrix was reported as not positive definite'
    assert e32 < 1e-4, ('the inputs are not well conditioned', case_id(c), e32)
    assert e < 2e-4 + 3 * e32, (case_id(c), mode, e, e32)


# ---- the child processes -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def child(mode):
    """Every case of a switch mode in ONE fresh child process with the switch in its environment: {case: record | error text}"""
    tmp = tempfile.mkdtemp()
    fn = os.path.join(tmp, mode + '.pt')
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, fn], env=dict(os.environ, **{CHILD_ENV[mode]: '1'}),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return torch.load(fn)
    finally:
        if os.path.exists(fn):
            os.remove(fn)
        os.rmdir(tmp)


def _child_main(mode, fn):
    sys.path.insert(0, ROOT)
    assert os.environ.get(CHILD_ENV[mode]) == '1'
    out = {}
    for c in CASES[mode]:
        try:
            out[tuple(c)] = run_case(c, mode)
        except Exception as e:                        # reported by the parent, per case (the package's own errors included)
            out[tuple(c)] = '%s: %s' % (type(e).__name__, e)
    if mode == 'small_factor':
        for c in NU_CASES:
            try:
                out[('nu',) + tuple(c)] = run_nu(c)
            except Exception as e:
                out[('nu',) + tuple(c)] = '%s: %s' % (type(e).__name__, e)
    torch.save(out, fn)


if __name__ == '__main__':
    _child_main(sys.argv[1], sys.argv[2])
