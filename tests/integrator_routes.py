"""Every route of the fixed-grid integrator and of its reverse sweep -- rhs_fwd and rollout_fwd (csrc/gp_forward.hip), rollout_bwd, rhs_vjp,
param_grad and rollout_bwd_pgrad (csrc/gp_backward.hip), with the evaluators they select from gp_rollout.hpp and gp_team.hpp -- shared
by test_gpu_integrator_routes.py and test_integrator_routes_host.py.  The library holds the ladder once (forward_route / reverse_route
in gp_rollout.hpp), and the adaptive launchers of csrc/gp_adaptive.hip take it from there: forward_route() and backward_resident()
below cover dopri5, landing and dense, too -- test_gpu_z0_draws.py runs it on the first 'full' case of every forward route.

A case is (kernel, Di, Do, order, M, S, N, T, method, nd, kind): the kernel family, the widths, the inducing points and Fourier
features, the trajectories, the output times, the solver and the Monte-Carlo draws.  kind: 'full' (everything), 'fused' (also the
reverse sweep with the parameter sums in one pass), 'prior' (an ops.kern_cache pack without inducing records: rhs in mode 1 only).

expected() restates the thresholds of the dispatch on its own (it never asks the library); run_case() builds the cache with
ops.cache_build and drives the C ABI on buffers it owns -- NaN-filled, GUARD NaN floats behind each -- twice, and returns the outputs,
the tags gpode_last_launch() gave, and what the buffer checks found; reference() is the oracle (gp_prior / gp_update / gp_forward,
odeint_fixed, autograd of sum(zt * gw)) on the cache THE GPU BUILT, read back, in fp64 and, for the bounds, in fp32: the conditioning
of K_uu is out of the comparison, what is left is the integrator's own arithmetic.

Bounds.  Every output X: relerr(X_hip, X_64) <= FLOOR[X] + 3 relerr(X_32, X_64).  Every floor starts at 2e-5, the project's bound for
f_prior, whose error source is the same (the hardware cosine in revolutions against libm).  No floor has been raised: measured on an
MI355X, the worst output of any case is 2.1e-6 from fp64 where the fp32 oracle is 9.7e-7 (d/d var, wave `stream` at 8197 rows); f in mode 0
reaches 1.5e-6 (fp32 oracle 2.3e-6), trajectories 1.8e-7, stage adjoints 7.9e-7, every other parameter gradient under 8e-7.

The inputs are test_gpu_backward.synthetic_gp's with two changes of scale, made so that the bounds mean something (inputs()): at
width 3 the inducing points are spread three times wider (as they come, |nu| reaches 1e2 and the fp32 oracle itself is 1e-4 from fp64,
d/d var 3e-4 on the GPU); at widths of 12 and more they are drawn in by half (as they come, no row is near enough to one for a dropped
inducing point to show through the bound)."""
import collections
import ctypes
import functools

import torch

GUARD = 4096
CHUNK = 256                                          # rows per oracle pass: the DF oracle holds (rows, 2 S, D, D) per evaluation
Case = collections.namedtuple('Case', 'kernel Di Do order M S N T method nd kind regime', defaults=('base',))     # regime: gp_regimes.TABLE
NSTAGE = {'euler': 1, 'rk4': 4, 'midpoint': 2}
TS = {3: (0.0, 0.05, 0.2), 2: (0.0, 0.2)}            # non-uniform: a sweep that read another step's dt would be seen

OUT_F = ('f0', 'f1', 'f2')
OUT_ROLL = ('zt', 'xstage', 'gz0', 'astage', 'gx')
OUT_LEAF = ('omega', 'B', 'var', 'Z', 'nu', 'ell')
FLOOR = {k: 2e-5 for k in OUT_F + OUT_ROLL + OUT_LEAF}


# ---- the dispatch, restated --------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


TEAM_MAX_ROWS = 2048
LDS_LIMIT = 150 * 1024
REG_BUDGET = 260                                     # floats of pack a wavefront may keep per lane


def layout(c):
    """(RQ, RQ2, rff_f4, ind_f4) of RbfLayout<Di, Do> / DfLayout<D> at (M, S): float4 per lane of a Fourier / an inducing record, and
    the float4 the records of the pack take"""
    if c.kernel == 'RBF':
        RQ, RQ2 = cdiv(c.Di + 2, 4), cdiv(c.Di + c.Do, 4)
    else:
        RQ, RQ2 = cdiv(2 * c.Do + 3, 4), cdiv(2 * c.Do, 4)
    return RQ, RQ2, cdiv(c.S, 64) * c.Do * RQ * 64, cdiv(c.M, 64) * RQ2 * 64


def rbf_reg_floats(c, SJ, MJ):
    RQ, RQ2, _, _ = layout(c)
    return 4 * (SJ * c.Do * RQ + MJ * RQ2)


def pack_bytes(c):
    _, _, r, i = layout(c)
    return 16 * (r + i)


def team_fits(c):
    """the register-resident quarter pack of a 4-wavefront team: S <= 256, M <= 128"""
    return cdiv(c.S, 64) <= 4 and 2 * cdiv(c.M, 64) <= 4


def forward_route(c):
    """the evaluator of rhs_fwd / rollout_fwd at N rows"""
    k = c.kernel.lower()
    width_ok = c.Do <= 16 if c.kernel == 'RBF' else c.Do <= 8
    if c.N <= TEAM_MAX_ROWS:
        return k + ('_team' if width_ok and team_fits(c) else '_team_stream')
    if c.kernel == 'RBF':
        SJ, MJ = cdiv(c.S, 64), cdiv(c.M, 64)
        if (SJ, MJ) == (4, 2) and rbf_reg_floats(c, 4, 2) <= REG_BUDGET:
            return 'rbf_reg42'
        if (SJ, MJ) == (1, 1) and rbf_reg_floats(c, 1, 1) <= REG_BUDGET:
            return 'rbf_reg11'
        return 'rbf_stream'
    return 'df_lds' if pack_bytes(c) <= LDS_LIMIT else 'df_stream'


def backward_resident(c):
    return c.Do <= 8 and team_fits(c)


def param_grad_route(c, R):
    k = c.kernel.lower()
    if not backward_resident(c):
        return 'param_grad_%s_stream' % k
    if c.kernel == 'DF' and c.Do == 6 and R >= 1024:
        return 'param_grad_df_split'
    return 'param_grad_' + k


def rows(c):
    return c.N * (c.T - 1) * NSTAGE[c.method]


def expected(c):
    """the tags after rhs, rollout, rollout_bwd, rhs_vjp and param_grad of case c"""
    f, k = forward_route(c), c.kernel.lower()
    if c.kind == 'prior':
        return dict(rhs='rhs_' + f)
    s = '' if backward_resident(c) else '_stream'
    want = dict(rhs='rhs_' + f, rollout='rollout_' + f, rollout_bwd='rollout_bwd_%s%s' % (k, s), rhs_vjp='rhs_vjp_%s%s' % (k, s),
                param_grad=param_grad_route(c, rows(c)))
    if c.kind == 'fused':
        want['fused'] = 'reduce_slab'
    return want


# ---- the case table ----------------------------------------------------------------------------------------------------------------
def R_(Di, Do, order, M, S, N, method, T=3, nd=1, kind='full'):
    return Case('RBF', Di, Do, order, M, S, N, T, method, nd, kind)


def D_(D, M, S, N, method, T=3, nd=1):
    return Case('DF', D, D, 1, M, S, N, T, method, nd, 'full')


# (The divergence-free rk4 cases of 2048 / 2049 rows have T = 2: the fp64 oracle holds (rows, 2 S, D, D) per evaluation and its autograd
# over two rk4 steps takes ~10 s of CPU per case; one step keeps every route and the 2049th row.  Their solver loop is the template the
# Euler, midpoint and RBF cases run at T = 3 on the non-uniform grid.)
# case -> the evaluator the table of the issue names for it (the forward route; test_integrator_routes_host.py checks expected() against it)
TABLE = collections.OrderedDict([
    (R_(6, 6, 1, 128, 256, 2048, 'rk4'), 'rbf_team'),              # the largest register team
    (R_(6, 6, 1, 128, 256, 2049, 'euler'), 'rbf_reg42'),
    (R_(6, 6, 1, 129, 256, 5, 'rk4'), 'rbf_team_stream'),          # the M edge
    (R_(6, 6, 1, 128, 257, 5, 'midpoint'), 'rbf_team_stream'),     # the S edge
    (R_(6, 6, 1, 65, 193, 2049, 'rk4'), 'rbf_reg42'),              # its low corner: one live lane in the last group of each
    (R_(3, 3, 1, 100, 200, 2049, 'midpoint'), 'rbf_reg42'),        # odd width
    (R_(6, 6, 1, 64, 64, 2049, 'rk4'), 'rbf_reg11'),
    (R_(6, 3, 2, 17, 33, 2049, 'rk4'), 'rbf_reg11'),               # second order
    (R_(16, 8, 2, 40, 64, 2049, 'euler'), 'rbf_reg11'),            # 184 floats fit
    (R_(6, 6, 1, 64, 65, 2049, 'rk4'), 'rbf_stream'),
    (R_(6, 6, 1, 64, 256, 2049, 'euler'), 'rbf_stream'),           # SJ = 4 but MJ = 1: the neighbour of reg42
    (R_(8, 8, 1, 100, 256, 2049, 'rk4'), 'rbf_stream'),            # 416 floats do not fit
    (R_(16, 16, 1, 40, 64, 5, 'rk4'), 'rbf_team'),                 # forward register team (Do <= 16), backward streamed (Do > 8)
    (R_(16, 16, 1, 40, 64, 2049, 'rk4'), 'rbf_stream'),
    (R_(6, 6, 1, 100, 256, 8197, 'euler', T=2), 'rbf_reg42'),      # 2048 workgroups of 4 wavefronts: five take a second row
    (R_(6, 6, 1, 64, 128, 8197, 'euler', T=2), 'rbf_stream'),
    (R_(6, 6, 1, 100, 256, 2049, 'rk4', nd=2), 'rbf_reg42'),       # several draws on the wave kernels
    (R_(6, 6, 1, 0, 32, 5, 'euler', kind='prior'), 'rbf_team'),    # an ops.kern_cache pack (M = 0), rhs in mode 1
    (R_(6, 6, 1, 0, 32, 2049, 'euler', kind='prior'), 'rbf_stream'),
    (D_(6, 100, 256, 2048, 'rk4', T=2), 'df_team'),
    (D_(6, 100, 256, 2049, 'rk4', T=2), 'df_lds'),                      # 104 448 B, through set_max_lds
    (D_(4, 16, 64, 2049, 'euler'), 'df_lds'),                      # under 64 KiB
    (D_(6, 128, 384, 5, 'rk4'), 'df_team_stream'),
    (D_(6, 128, 384, 2049, 'rk4', T=2), 'df_lds'),                      # exactly 153 600 B = the limit
    (D_(6, 129, 384, 2049, 'euler'), 'df_stream'),                 # 156 672 B
    (D_(15, 24, 64, 2049, 'rk4', T=2), 'df_lds'),                       # 146 432 B
    (D_(16, 24, 64, 2049, 'rk4', T=2), 'df_stream'),                    # 155 648 B: width 16 has no LDS route at all
    (D_(7, 65, 100, 2049, 'midpoint'), 'df_lds'),                  # odd width, ragged
    (D_(6, 100, 256, 2049, 'euler', nd=2), 'df_lds'),              # several draws
    (D_(6, 100, 256, 1023, 'euler', T=2), 'df_team'),              # 1023 rows: param_grad_df
    (D_(6, 100, 256, 1024, 'euler', T=2), 'df_team'),              # 1024 rows: param_grad_df_split
    (R_(6, 6, 1, 100, 256, 2049, 'euler', kind='fused'), 'rbf_reg42'),   # 2048 chunks, one of them holds two rows
    (R_(6, 6, 1, 100, 256, 2049, 'rk4', kind='fused'), 'rbf_reg42'),
])
CASES = list(TABLE)
BYTES = {D_(6, 100, 256, 2049, 'rk4', T=2): 104448, D_(6, 128, 384, 2049, 'rk4', T=2): 153600, D_(6, 129, 384, 2049, 'euler'): 156672,
         D_(15, 24, 64, 2049, 'rk4', T=2): 146432, D_(16, 24, 64, 2049, 'rk4', T=2): 155648}
REG_FLOATS = {(R_(6, 6, 1, 128, 256, 2049, 'euler'), 4, 2): 216, (R_(16, 8, 2, 40, 64, 2049, 'euler'), 1, 1): 184,
              (R_(8, 8, 1, 100, 256, 2049, 'rk4'), 4, 2): 416}
# param_grad alone: R = 10 rows in nchunk = 7 chunks of 2 rows, so used = 5 < nchunk, with two draws; accumulate = 0, then = 1
ACC_CASES = [R_(6, 6, 1, 100, 256, 10, 'euler', T=2, nd=2), D_(6, 100, 256, 10, 'euler', T=2, nd=2)]
ACC_NCHUNK = 7

_F = ('rbf_team', 'rbf_team_stream', 'rbf_reg42', 'rbf_reg11', 'rbf_stream', 'df_team', 'df_team_stream', 'df_lds', 'df_stream')
REQUIRED_TAGS = tuple('%s_%s' % (e, f) for e in ('rhs', 'rollout') for f in _F) + \
    tuple('%s_%s%s' % (e, k, s) for e in ('rollout_bwd', 'rhs_vjp') for k in ('rbf', 'df') for s in ('', '_stream')) + \
    ('param_grad_rbf', 'param_grad_rbf_stream', 'param_grad_df', 'param_grad_df_split', 'param_grad_df_stream', 'reduce_slab')


def case_id(c):
    import gp_regimes
    return '%s-%d-%d-o%d-M%d-S%d-N%d-T%d-%s-L%d-%s' % c[:11] + gp_regimes.suffix(c.regime)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def inputs(c):
    """parameters and noise of test_gpu_backward.synthetic_gp (nd draws of noise, stacked on a leading axis when nd > 1), initial
    states, the non-uniform output times and dL/dzt (nd, N, T, Di) of a loss that is summed over the draws"""
    import gp_regimes
    from test_gpu_backward import synthetic_gp
    seed = 4000 + c.M + 3 * c.S + 7 * c.Di + 11 * c.Do
    p, nz, z0, _, _ = synthetic_gp(c.kernel, c.Di, c.Do, max(c.M, 1), c.S, c.N, c.T, seed=seed)
    p, z0 = gp_regimes.apply(c.regime, p, z0, c.kernel)
    if c.nd > 1:
        more = [synthetic_gp(c.kernel, c.Di, c.Do, max(c.M, 1), c.S, 1, c.T, seed=seed + 100 * l)[1] for l in range(1, c.nd)]
        nz = {k: torch.stack([nz[k]] + [m[k] for m in more]) for k in nz}
    if c.Di >= 12:                                   # 2 randn in 12+ dimensions is further than exp(-r^2 / 2 ell^2) reaches from a row (ell = 2):
        p = dict(p, Z=0.5 * p['Z'])                  # the inducing points would not be seen through the bound (test_integrator_routes_host.py)
    if c.Di == 3:                                    # 100 points of 2 randn in three dimensions at ell = 2: |nu| reaches 1e2 and f is a difference
        p = dict(p, Z=3.0 * p['Z'])                  # of large terms (fp32 oracle 1e-4 from fp64); three times as far apart |nu| stays under 5
    g = torch.Generator().manual_seed(seed + 1)
    gw = torch.randn(c.nd, c.N, c.T, c.Di, generator=g)
    return p, nz, z0, gp_regimes.times(c.regime, torch.tensor(TS[c.T])), gw


def draw(nz, c, l):
    return {k: (v[l] if c.nd > 1 else v) for k, v in nz.items()}


def host_cache(c, dtype=torch.float64):
    """the oracle's own build of the case's cache, one dict per draw (for the tests that run without a GPU)"""
    from oracle import gpode_oracle as O
    p, nz, _, _, _ = inputs(c)
    if c.kind == 'prior':
        ell, var = O.softplus(p['raw_ell'].to(dtype)), O.softplus(p['raw_var'].to(dtype))
        return [dict(kernel=c.kernel, S=c.S, omega=O.rff_omega(nz['rff_eps'].to(dtype), ell), phase=O.rff_phase(nz['rff_u'].to(dtype)),
                     w=nz['rff_w'].to(dtype), var=var, ell=ell)]
    return [O.build_cache(O.to_dtype(p, dtype), O.to_dtype(draw(nz, c, l), dtype), c.kernel) for l in range(c.nd)]


# ---- reference ---------------------------------------------------------------------------------------------------------------------
LEAVES = ('omega', 'var', 'nu', 'Z', 'ell')


def _leaf_cache(cd, dtype, kernel):
    """the cache dict in dtype with the differentiated quantities as autograd leaves (test_gpu_backward.oracle_leaf_grads without the build)"""
    from oracle import gpode_oracle as O
    cl = {k: (v.detach().to(dtype) if torch.is_tensor(v) else v) for k, v in cd.items()}
    leaf = {k: cl[k].clone().requires_grad_(True) for k in LEAVES}
    if kernel == 'DF':
        leaf['B'] = O.df_B_omega(cl['omega']).clone().requires_grad_(True)
    cl.update(leaf)
    return cl, leaf


def _leaf_out(leaf, c):
    out = {k: v.grad if v.grad is not None else torch.zeros_like(v) for k, v in leaf.items()}
    if 'B' in out:
        out['B'] = out['B'][:c.S] + out['B'][c.S:]                  # the cos and sin halves share B
    return out


def reference(c, cache, dtype, z0=None, ts=None, gw=None, integrate=None):
    """The oracle on `cache` (one dict(kernel, omega, phase, w, var, S, Z, nu, ell) per draw) in dtype: f in the three modes at the rows
    of z0, the trajectories, the input of every evaluation of f, and by autograd of sum(zt * gw) dL/dz0, dL/df at every evaluation and
    the gradients w.r.t. the cache quantities as leaves.  Every tensor has a leading draw axis.  Rows go through in chunks of CHUNK
    (they are independent; the leaf gradients add up).  integrate: odeint_fixed unless a test swaps the solver."""
    from oracle import gpode_oracle as O
    integrate = integrate or O.odeint_fixed
    if z0 is None or ts is None or gw is None:
        i_z0, i_ts, i_gw = inputs(c)[2:]
        z0, ts, gw = (i_z0 if z0 is None else z0), (i_ts if ts is None else ts), (i_gw if gw is None else gw)
    z0, ts, gw = z0.to(dtype), ts.to(dtype), gw.to(dtype)
    if gw.dim() == 3:
        gw = gw.unsqueeze(0)
    N, q = z0.shape[0], c.Do
    res = collections.defaultdict(list)
    for l, cd in enumerate(cache):
        if c.kind == 'prior':
            res['f1'].append(O.gp_prior(z0, {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in cd.items()}))
            continue
        cl, leaf = _leaf_cache(cd, dtype, c.kernel)
        per = collections.defaultdict(list)
        for i in range(0, N, CHUNK):
            with torch.no_grad():
                x = z0[i:i + CHUNK]
                per['f0'].append(O.gp_forward(x, cl)); per['f1'].append(O.gp_prior(x, cl)); per['f2'].append(O.gp_update(x, cl))
            z = z0[i:i + CHUNK].clone().requires_grad_(True)
            xs, fs = [], []

            def f(y):                                # flow.py:27-45 as O.ode_rhs states it, keeping what the reverse sweep records
                fv = O.gp_forward(y, cl)
                fv.retain_grad()
                xs.append(y); fs.append(fv)
                return fv if c.order == 1 else torch.cat([y[:, q:], fv], 1)
            zt = integrate(f, z, ts, c.method).permute([1, 0, 2])
            (zt * gw[l, i:i + CHUNK]).sum().backward()
            n, NS = z.shape[0], len(xs) // max(c.T - 1, 1)
            per['zt'].append(zt.detach()); per['gz0'].append(z.grad)
            per['xstage'].append(torch.stack([v.detach() for v in xs], 1).reshape(n, c.T - 1, NS, c.Di))
            per['astage'].append(torch.stack([v.grad for v in fs], 1).reshape(n, c.T - 1, NS, c.Do))
        for k, v in per.items():
            res[k].append(torch.cat(v))
        for k, v in _leaf_out(leaf, c).items():
            res[k].append(v)
    return {k: torch.stack(v) for k, v in res.items()}


def reference_rows(c, cache, dtype, x, a):
    """J_f(x)^T a per row (rhs_vjp) and the leaf gradients of sum_r <a_r, f(x_r)> (param_grad) for rows x (nd, R, Di), a (nd, R, Do)"""
    from oracle import gpode_oracle as O
    gx, leaves = [], collections.defaultdict(list)
    for l, cd in enumerate(cache):
        cl, leaf = _leaf_cache(cd, dtype, c.kernel)
        g = []
        for i in range(0, x.shape[1], 4 * CHUNK):
            xi = x[l, i:i + 4 * CHUNK].to(dtype).clone().requires_grad_(True)
            (O.gp_forward(xi, cl) * a[l, i:i + 4 * CHUNK].to(dtype)).sum().backward()
            g.append(xi.grad)
        gx.append(torch.cat(g))
        for k, v in _leaf_out(leaf, c).items():
            leaves[k].append(v)
    return torch.stack(gx), {k: torch.stack(v) for k, v in leaves.items()}


# ---- launches ----------------------------------------------------------------------------------------------------------------------
def _guarded(*shape):
    """a NaN-filled buffer of the shape with GUARD NaN floats behind it: (the tensor, the guard)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), float('nan'), device='cuda')
    return buf[:n].view(*shape), buf[n:]


def build(c, dev_in):
    """the case's cache on the GPU: ops.cache_build, or ops.kern_cache for a 'prior' case"""
    from vae_gp_ode_amd import ops
    p, nz = dev_in[:2]
    if c.kind == 'prior':
        return ops.kern_cache(c.kernel, p['raw_ell'], p['raw_var'], nz['rff_w'], nz['rff_eps'], nz['rff_u'])
    k = ops.cache_build(c.kernel, p['raw_ell'], p['raw_var'], p['Z'], p['Um'], p['Us'], nz['eps_u'], nz['rff_w'], nz['rff_eps'], nz['rff_u'])
    k.check_factorisation()
    return k


def cache_dicts(c, k, dev_in):
    """what reference() takes, from the tensors the GPU's build left (read back) and the inputs it does not transform"""
    from oracle import gpode_oracle as O
    p, nz = dev_in[:2]
    out = []
    for l in range(c.nd):
        pick = (lambda t: t[l].cpu()) if c.nd > 1 else (lambda t: t.cpu())
        if c.kind == 'prior':
            out.append(dict(kernel=c.kernel, S=c.S, omega=pick(k.omega), phase=pick(k.phase), w=pick(nz['rff_w']),
                            var=O.softplus(p['raw_var'].cpu().double()), ell=O.softplus(p['raw_ell'].cpu().double())))
        else:
            out.append(dict(kernel=c.kernel, S=c.S, omega=pick(k.omega), phase=pick(k.phase), w=pick(nz['rff_w']), var=k.var.cpu(),
                            Z=p['Z'].cpu(), nu=pick(k.nu), ell=k.ell.cpu()))
    return out


def _once(c, k, dev_in):
    from vae_gp_ode_amd import _lib, ops
    from vae_gp_ode_amd.ops import KERNEL_ID, METHOD_ID, _ptr, _stream
    lib = _lib.load()
    tag = lambda: lib.gpode_last_launch().decode()
    p, nz, z0, ts, gw = dev_in
    kid, Di, Do, M, S, N, T, nd = KERNEL_ID[c.kernel], c.Di, c.Do, c.M, c.S, c.N, c.T, c.nd
    NS, mid = NSTAGE[c.method], METHOD_ID[c.method]
    pack = k.pack.view(nd, -1)
    pf = pack.shape[1]
    out, guards = {}, {}

    def new(name, *shape):
        out[name], guards[name] = _guarded(*shape)
        return out[name]
    # f(x) at the rows of z0 in the three modes, draw by draw (the entry point takes one pack)
    modes = (1,) if c.kind == 'prior' else (0, 1, 2)
    for m in modes:
        f = new('f%d' % m, nd, N, Do)
        for l in range(nd):
            _lib.call('gpode_rhs_fwd', kid, Di, Do, M, S, _ptr(pack[l]), _ptr(z0), N, _ptr(f[l]), m, _stream())
            if m == modes[0] and l == 0:
                out['tag_rhs'] = tag()
            assert tag() == out['tag_rhs']
    if c.kind == 'prior':
        return out, guards
    zt, xs = new('zt', nd, N, T, Di), new('xstage', nd, N, T - 1, NS, Di)
    _lib.call('gpode_rollout_fwd_n', kid, c.order, mid, Di, Do, M, S, nd, _ptr(pack), _ptr(z0), _ptr(ts), N, T, _ptr(zt), _ptr(xs), _stream())
    out['tag_rollout'] = tag()
    gz0, ast = new('gz0', nd, N, Di), new('astage', nd, N, T - 1, NS, Do)
    _lib.call('gpode_rollout_bwd_n', kid, c.order, mid, Di, Do, M, S, nd, _ptr(pack), _ptr(xs), _ptr(gw), _ptr(ts), N, T, _ptr(gz0), _ptr(ast),
              _stream())
    out['tag_rollout_bwd'] = tag()
    # J^T a on the first-stage rows: N (T-1) of them, so the team kernels are on their grid-stride from N = 2049
    xv, av = xs[:, :, :, 0].reshape(nd, -1, Di).contiguous(), ast[:, :, :, 0].reshape(nd, -1, Do).contiguous()
    gx = new('gx', nd, xv.shape[1], Di)
    for l in range(nd):
        _lib.call('gpode_rhs_vjp', kid, Di, Do, M, S, _ptr(pack[l]), _ptr(xv[l]), _ptr(av[l]), xv.shape[1], _ptr(gx[l]), _stream())
        if l == 0:
            out['tag_rhs_vjp'] = tag()
        assert tag() == out['tag_rhs_vjp']
    out['vjp_x'], out['vjp_a'] = xv, av
    # the parameter sums over every (stage input, adjoint) row, chunked as ops.param_grad chunks them
    R = rows(c)
    nchunk = max(1, min(min(256, max(64, R // 32)), R))
    slab, gpack = new('slab', nd * nchunk * pf), new('gpack', nd, pf)
    _lib.call('gpode_param_grad_n', kid, Di, Do, M, S, nd, _ptr(pack), _ptr(xs), _ptr(ast), R, _ptr(slab), nchunk, _ptr(gpack), 0, _stream())
    out['tag_param_grad'] = tag()
    if c.kind == 'fused':
        nch = ops.pgrad_chunks(k, N, c.order, c.method, force=True)
        assert nch == min(N, 2048), nch
        out['fused_gz0'], out['fused_astage'], out['fused_gpack'] = ops.rollout_bwd_pgrad(k, xs, gw if nd > 1 else gw[0], ts, c.order, c.method, nch)
        out['tag_fused'] = tag()
    return out, guards


def run_case(c):
    """Case c TWICE on one cache: the outputs (on the CPU), the tags, which guards changed, which outputs kept a NaN, which outputs
    of the second run differ in a bit; and the cache as reference() takes it."""
    p, nz, z0, ts, gw = inputs(c)
    dev_in = ({k: v.cuda() for k, v in p.items()}, {k: v.cuda() for k, v in nz.items()}, z0.cuda(), ts.cuda(), gw.cuda())
    k = build(c, dev_in)
    runs = []
    for _ in range(2):
        out, guards = _once(c, k, dev_in)
        torch.cuda.synchronize()
        rec = {kk: (v.cpu() if torch.is_tensor(v) else v) for kk, v in out.items() if kk != 'slab'}      # scratch: only its guard counts
        rec['guards_changed'] = [kk for kk, g in guards.items() if not torch.isnan(g).all()]
        runs.append(rec)
    a, b = runs
    a['second_run_differs'] = [kk for kk in a if not _same(a[kk], b[kk])]
    a['cache'] = cache_dicts(c, k, dev_in)
    return a


def _same(x, y):
    if torch.is_tensor(x):                           # pad lanes of a pack-layout gradient may hold NaN: the same bits all the same
        return torch.equal(x.view(torch.int32), y.view(torch.int32))
    return x == y


def run_accumulate(c):
    """gpode_param_grad_n on R = c.N rows in ACC_NCHUNK chunks (fewer are used than the slab has) for nd draws: accumulate = 0, then
    accumulate = 1 into a gpack that holds a known tensor."""
    from vae_gp_ode_amd import _lib
    from vae_gp_ode_amd.ops import KERNEL_ID, _ptr, _stream
    p, nz, z0, ts, gw = inputs(c)
    dev_in = ({k: v.cuda() for k, v in p.items()}, {k: v.cuda() for k, v in nz.items()}, z0.cuda(), ts.cuda(), gw.cuda())
    k = build(c, dev_in)
    pack = k.pack.view(c.nd, -1)
    pf, R = pack.shape[1], c.N
    g = torch.Generator().manual_seed(77)
    x, a = torch.randn(c.nd, R, c.Di, generator=g), torch.randn(c.nd, R, c.Do, generator=g)
    have = torch.randn(c.nd, pf, generator=g)
    out = dict(x=x, a=a, have=have, cache=cache_dicts(c, k, dev_in), guards_changed=[])
    xd, ad = x.cuda(), a.cuda()
    for acc in (0, 1):
        slab, sg = _guarded(c.nd * ACC_NCHUNK * pf)
        gpack, gg = _guarded(c.nd, pf)
        if acc:
            gpack.copy_(have)
        _lib.call('gpode_param_grad_n', KERNEL_ID[c.kernel], c.Di, c.Do, c.M, c.S, c.nd, _ptr(pack), _ptr(xd), _ptr(ad), R, _ptr(slab),
                  ACC_NCHUNK, _ptr(gpack), acc, _stream())
        out['tag'] = _lib.load().gpode_last_launch().decode()
        torch.cuda.synchronize()
        out['gpack%d' % acc] = gpack.cpu()
        out['guards_changed'] += [n for n, t in (('slab', sg), ('gpack', gg)) if not torch.isnan(t).all()]
    return out


# ---- comparison --------------------------------------------------------------------------------------------------------------------
def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def unpack(c, gpack, cache):
    """a pack-layout gradient (nd, pack_floats) as the leaf gradients reference() returns, stacked over the draws (fp64)"""
    from pack_layout import PackView, leaf_grads
    pv = PackView(c.kernel, c.Di, c.Do, c.M, c.S)
    per = [leaf_grads(pv, gpack[l].double(), {k: (v.double() if torch.is_tensor(v) else v) for k, v in cache[l].items()})
           for l in range(len(cache))]
    return {k: torch.stack([d[k] for d in per]) for k in per[0]}


def bound(key, e32):
    return FLOOR[key] + 3 * e32


def compare(c, got, r64, r32, keys, what=''):
    """{key: (relerr(hip, fp64), relerr(fp32 oracle, fp64))} printed, then asserted against the bound; a NaN left in an output fails"""
    errs = {k: (relerr(got[k], r64[k].reshape(got[k].shape)), relerr(r32[k], r64[k])) for k in keys}
    print('  %ship / fp32-oracle relerr to fp64: %s' % (what, ', '.join('%s %.1e/%.1e' % ((k,) + errs[k]) for k in keys)))
    nan = [k for k in keys if torch.isnan(got[k]).any()]
    assert not nan, (case_id(c), 'left NaN', nan)
    bad = {k: (e, bound(k, e32)) for k, (e, e32) in errs.items() if not e <= bound(k, e32)}
    assert not bad, (case_id(c), what, bad)
    return errs


def check_case(c, got, seen=None):
    """got (run_case) against the dispatch table and the fp64 oracle on the cache the GPU built; prints every figure before it asserts.
    Returns {(what, key): (relerr(hip, fp64), relerr(fp32 oracle, fp64))} of every comparison it made."""
    want = expected(c)
    tags = {kk[4:]: v for kk, v in got.items() if kk.startswith('tag_')}
    print('%s %s' % (case_id(c), tags))
    if seen is not None:
        seen.update(tags.values())
    assert tags == want, (case_id(c), tags, want)
    assert not got['guards_changed'], (case_id(c), 'wrote past its buffer', got['guards_changed'])
    r64, r32 = reference(c, got['cache'], torch.float64), reference(c, got['cache'], torch.float32)
    errs = {}

    def held(what, *args):
        errs.update({(what, k): v for k, v in compare(c, *args, what).items()})
    if c.kind == 'prior':
        held('', got, r64, r32, ('f1',))
        assert not got['second_run_differs'], (case_id(c), got['second_run_differs'])
        return errs
    held('', got, r64, r32, OUT_F + OUT_ROLL[:4])
    v64, v32 = (reference_rows(c, got['cache'], dt, got['vjp_x'], got['vjp_a'])[0] for dt in (torch.float64, torch.float32))
    held('', got, dict(gx=v64), dict(gx=v32), ('gx',))
    leaf = [k for k in OUT_LEAF if k in r64]
    held('param_grad: ', unpack(c, got['gpack'], got['cache']), r64, r32, leaf)
    if c.kind == 'fused':
        fused = dict(unpack(c, got['fused_gpack'].view(c.nd, -1), got['cache']), gz0=got['fused_gz0'].view(c.nd, c.N, c.Di),
                     astage=got['fused_astage'].view_as(got['astage']))
        held('fused: ', fused, r64, r32, ['gz0', 'astage'] + leaf)
    assert not got['second_run_differs'], (case_id(c), got['second_run_differs'])
    return errs


def check_accumulate(c, got, seen=None):
    want = param_grad_route(c, c.N)
    print('%s %s' % (case_id(c), got['tag']))
    if seen is not None:
        seen.add(got['tag'])
    assert got['tag'] == want, (got['tag'], want)
    assert not got['guards_changed'], got['guards_changed']
    (_, r64), (_, r32) = (reference_rows(c, got['cache'], dt, got['x'], got['a']) for dt in (torch.float64, torch.float32))
    g0 = unpack(c, got['gpack0'], got['cache'])
    compare(c, g0, r64, r32, [k for k in OUT_LEAF if k in r64], 'accumulate = 0: ')
    # accumulate = 1 adds the 16 partial sums to the entry in place of zero: 17 fp32 additions either way, in another order, so the two
    # differ by at most 2 x 16 x 2^-24 = 1.9e-6 of the largest magnitude on the way (the entry that was there plus the sum)
    from pack_layout import PackView
    pv = PackView(c.kernel, c.Di, c.Do, c.M, c.S)
    for l in range(c.nd):
        for view in (pv.rff, pv.ind, pv.uni):
            h, a, b = view(got['have'][l].double()), view(got['gpack0'][l].double()), view(got['gpack1'][l].double())
            assert not torch.isnan(b).any()
            err = (b - (h + a)).abs().max().item()
            assert err <= 2e-6 * (h.abs().max() + a.abs().max()).item(), (case_id(c), l, err)
