"""Hyper-parameter regimes of the GP path, shared by test_gp_regimes_host.py and test_gpu_gp_regimes.py.

test_gpu_backward.synthetic_gp -- the source of gp_routes.inputs and integrator_routes.inputs -- draws every lengthscale from
2 (1 + 0.05 u) and sets every variance to 1: a kernel that read var[a] for var[b], or ell[i,d] for ell[d,i], computes the same numbers
there (test_gp_regimes_host.py shows it).  A regime overrides raw_ell, raw_var, the scale of Z and the scale of the states (z0 / x) of synthetic_gp's output,
in `short` also the scale of the output times, and nothing else.  u ~ U(0,1)^(Do x Di), v ~ U(0,1)^Do, seeded by the regime and the widths.

  regime       ell                    var            Z   states  what it is for
  var_spread   as synthetic_gp        0.3 10^v       2   1       every index of var
  ell_spread   4^u (1..4, asymmetric) 0.3 10^v       2   1       every index of ell; DF's lower-triangle read; the sym(G) convention
  short        0.5 (1 + 0.3 u)        0.3 10^v       0.7 0.7     large phases, sharp exponentials
  long         8 (1 + 0.3 u)          0.3 10^v       8   4       flat K_uu, small pivots
  ell_linear   25 (1 + 0.2 u)         0.3 10^v       25  12      raw > 20: the linear branch of softplus / sigmoid, ell
  var_linear   as synthetic_gp        22 + 6 v       2   1       the same branch, var
  var_small    as synthetic_gp        0.01 (1 + v)   2   1       pivots of 0.06, |nu| of 30
  far          2 (1 + 0.3 u)          0.3 10^v       2   10      update ~ 1e-5 of the prior; the cosine's argument in the tens of revolutions

In `short` the output times move with ell, too: every ts is multiplied by 0.25 (times()).  At ell = 0.5 the prior alone has |f| = 13, and
a step of 0.2 would cross five lengthscales: the solver map is then so nonlinear that the reverse sweep amplifies rounding and the fp32
oracle's own adjoints are 5e-5 .. 4e-4 from fp64, with a perturbation of 1e-6 in the cache moving that figure by a factor of 5.  With
steps of 0.0125 .. 0.05 a step covers what it covers at ell = 2, and they are at 2e-6.  The Z scale moves with ell (`long` with Z left
at 2 is not well posed: the fp32 oracle's nu is 3.8e-4 from fp64), and for DF it is widened further
where the matrix that the lower triangle of K_uu defines would not be positive definite (df_z_spread).
test_gp_regimes_host.py holds every (case, regime) the GPU tests use to relerr(fp32 oracle, fp64 oracle) <= 2e-5 forward, 1e-4 gradients.

A case carries its regime as a trailing field of gp_routes.Case / integrator_routes.Case ('base' = synthetic_gp as it is, the default,
not printed in the case id)."""
import collections
import contextlib

import torch

Regime = collections.namedtuple('Regime', 'ell var z_scale x_scale t_scale', defaults=(1.0,))
SYNTHETIC_Z_SCALE = 2.0                               # synthetic_gp: Z = 2 randn
TABLE = collections.OrderedDict([
    ('var_spread', Regime(None, lambda v: 0.3 * 10.0 ** v, 2.0, 1.0)),
    ('ell_spread', Regime(lambda u: 4.0 ** u, lambda v: 0.3 * 10.0 ** v, 2.0, 1.0)),
    ('short', Regime(lambda u: 0.5 * (1 + 0.3 * u), lambda v: 0.3 * 10.0 ** v, 0.7, 0.7, 0.25)),
    ('long', Regime(lambda u: 8.0 * (1 + 0.3 * u), lambda v: 0.3 * 10.0 ** v, 8.0, 4.0)),
    ('ell_linear', Regime(lambda u: 25.0 * (1 + 0.2 * u), lambda v: 0.3 * 10.0 ** v, 25.0, 12.0)),
    ('var_linear', Regime(None, lambda v: 22.0 + 6.0 * v, 2.0, 1.0)),
    ('var_small', Regime(None, lambda v: 0.01 * (1 + v), 2.0, 1.0)),
    ('far', Regime(lambda u: 2.0 * (1 + 0.3 * u), lambda v: 0.3 * 10.0 ** v, 2.0, 10.0)),
])
REGIMES = tuple(TABLE)
FIRST = ('var_spread', 'ell_spread')                  # the two that every case runs
ROLL = ('var_spread', 'ell_spread', 'short', 'far')   # the four that every integrator route runs
LINEAR = ('ell_linear', 'var_linear')                 # raw > 20 by construction (test_gp_regimes_host.py checks it)


def uniforms(regime, Do, Di):
    """(u (Do,Di), v (Do)) of the regime at these widths"""
    g = torch.Generator().manual_seed(77000 + 1000 * REGIMES.index(regime) + 31 * Do + Di)
    return torch.rand(Do, Di, generator=g), torch.rand(Do, generator=g)


def df_z_spread(regime, M):
    """The factor by which DF's inducing points are spread beyond the table's Z scale.  DF's K_uu is not symmetric once ell or var differ
    between dimensions, and the matrix its lower triangle defines is positive definite only while the blocks between different inducing
    points are small against the diagonal ones.  Measured in fp64 (smallest / largest eigenvalue of that matrix, D = 6): at the table's
    scale ell_spread is indefinite at M = 16 and 31 (-3e-3, -1e-2) and at M = 100 .. 129 even twice as wide (-1e-2), and var_spread, long,
    ell_linear and far are indefinite at M = 100 or 128 (-1e-2 .. -5e-3).  With these factors every case is at 1e-2 or more."""
    if regime == 'ell_spread':
        return 1.5 if M < 100 else 3.0
    return 1.0 if M < 100 else 1.5


def apply(regime, p, x, kernel):
    """(p, x) of synthetic_gp in the regime: raw_ell, raw_var, Z and the states replaced as the table says, everything else as it was"""
    from oracle import gpode_oracle as O
    if regime == 'base':
        return p, x
    r = TABLE[regime]
    Do, Di = p['raw_ell'].shape
    u, v = uniforms(regime, Do, Di)
    z_scale = r.z_scale * (df_z_spread(regime, p['Z'].shape[0]) if kernel == 'DF' else 1.0)
    q = dict(p, raw_var=O.invsoftplus(r.var(v)), Z=p['Z'] * (z_scale / SYNTHETIC_Z_SCALE))
    if r.ell is not None:
        q['raw_ell'] = O.invsoftplus(r.ell(u))
    return q, x * r.x_scale


def times(regime, ts):
    """the output times of a case in the regime"""
    return ts if regime == 'base' or TABLE[regime].t_scale == 1.0 else ts * TABLE[regime].t_scale


def suffix(regime):
    return '' if regime == 'base' else '-' + regime


# ---- the whole path in the oracle: what the well-posedness gate and the layer test compare ----------------------------------------------
FWD_KEYS = ('nu', 'u_prior', 'f', 'zt')
GRAD_KEYS = ('raw_ell', 'raw_var', 'Z', 'Um', 'Us', 'z0')
FWD_CAP, GRAD_CAP = 2e-5, 1e-4


def oracle(kernel, p, draws, z0, ts, gw, order, method, dtype):
    """The oracle's build, f(z0), trajectories and the gradients of sum_l sum(zt_l * gw_l) in dtype.  draws: one noise dict per draw;
    gw (L,N,T,Di).  Raises what torch.linalg.cholesky raises when K_uu + jitter I does not factorise."""
    from oracle import gpode_oracle as O
    q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    z = z0.to(dtype).clone().requires_grad_(True)
    out, loss = collections.defaultdict(list), 0.0
    for l, nz in enumerate(draws):
        cl = O.build_cache(q, {k: v.to(dtype) for k, v in nz.items()}, kernel)
        zt = O.flow_forward(z, ts.to(dtype), cl, order, method)
        loss = loss + (zt * gw[l].to(dtype)).sum()
        for k in ('nu', 'u_prior'):
            out[k].append(cl[k].detach())
        out['f'].append(O.gp_forward(z, cl).detach())
        out['zt'].append(zt.detach())
    loss.backward()
    r = {k: torch.stack(v) for k, v in out.items()}
    d = torch.diagonal(cl['Lu'].detach(), dim1=-2, dim2=-1)
    r.update({k: v.grad for k, v in q.items()}, z0=z.grad)
    return r, (float(d.min()), float(d.max()))


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def well_posed(kernel, p, draws, z0, ts, gw, order, method):
    """({key: relerr(fp32 oracle, fp64 oracle)}, the fp64 factor's (smallest, largest) pivot); both oracles must factorise"""
    r64, piv = oracle(kernel, p, draws, z0, ts, gw, order, method, torch.float64)
    r32, _ = oracle(kernel, p, draws, z0, ts, gw, order, method, torch.float32)
    bad = [k for k in r32 if not torch.isfinite(r32[k]).all()]
    assert not bad, ('the fp32 oracle is not finite', bad)
    return {k: relerr(r32[k], r64[k]) for k in FWD_KEYS + GRAD_KEYS}, piv


# ---- the fp32 twin of the kernel matrices ---------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def twin(dtype):
    """In float32, the oracle with its squared distances in difference form, sum_i ((x_i - y_i) / ell_i)^2, as the kernels compute
    them.  The oracle's own expanded form |x|^2 - 2 x.y + |y|^2 (kernels.py:64-79, :217-230) cancels in fp32: K(x, x) of states at
    |x| = 25 (`far`) is 3e-5 from fp64 that way, which would put a yardstick of the oracle's weakness, not of fp32, into the bound.
    float64 (the reference) is left as it is."""
    from oracle import gpode_oracle as O
    if dtype != torch.float32:
        yield
        return

    def rbf_sqdist(X, X2, ell):
        X2 = X if X2 is None else X2
        return (((X[None, :, None, :] - X2[None, None, :, :]) / ell[:, None, None, :]) ** 2).sum(-1)

    def df_sqdist(X, X2):
        X2 = X if X2 is None else X2
        return ((X[:, None, :] - X2[None, :, :]) ** 2).sum(-1)
    keep = O.rbf_sqdist, O.df_sqdist
    O.rbf_sqdist, O.df_sqdist = rbf_sqdist, df_sqdist
    try:
        yield
    finally:
        O.rbf_sqdist, O.df_sqdist = keep


# ---- mutants of the oracle: the mistakes the regimes are there to show -------------------------------------------------------------------
class _CholLowerGrad(torch.autograd.Function):
    """torch.linalg.cholesky whose backward puts the whole gradient on the lower triangle (G_low = 2 tril(G) - diag(G), G torch's
    symmetrised one): the same directional derivative along symmetric perturbations, another one along the asymmetric ones of DF"""
    @staticmethod
    def forward(ctx, A):
        ctx.save_for_backward(A)
        return torch.linalg.cholesky(A)

    @staticmethod
    def backward(ctx, gL):
        A, = ctx.saved_tensors
        with torch.enable_grad():
            a = A.detach().requires_grad_(True)
            G, = torch.autograd.grad(torch.linalg.cholesky(a), a, gL)
        return 2 * G.tril() - torch.diag_embed(torch.diagonal(G, dim1=-2, dim2=-1))


def _mutants():
    from oracle import gpode_oracle as O

    def df_K_var_row(X, X2, ell, var):               # var[a] where df_K reads var[b]
        return O_df_K(X, X2, ell, torch.ones_like(var)) * var.repeat(X.shape[0])[:, None]

    def df_nu_upper(Ku, u_prior, u):
        return O_df_nu(Ku.T, u_prior, u)

    def df_nu_lower_grad(Ku, u_prior, u):
        n = Ku.shape[0]
        Lu = _CholLowerGrad.apply(Ku + torch.eye(n, dtype=Ku.dtype) * O.JITTER)
        nu = torch.linalg.solve_triangular(Lu, u_prior.reshape(n)[:, None], upper=False)
        return Lu, torch.linalg.solve_triangular(Lu.T, u.reshape(n)[:, None] - nu, upper=True)

    O_df_K, O_rbf_K, O_rff, O_omega, O_df_nu = O.df_K, O.rbf_K, O.rbf_rff_forward, O.rff_omega, O.df_compute_nu
    return {
        'df_K: var[a] for var[b]': ('DF', dict(df_K=df_K_var_row)),
        'rbf_K: var rolled by one': ('RBF', dict(rbf_K=lambda X, X2, ell, var: O_rbf_K(X, X2, ell, var.roll(1)))),
        'rbf_rff_forward: var rolled by one': ('RBF', dict(rbf_rff_forward=lambda x, om, ph, w, var, S: O_rff(x, om, ph, w, var.roll(1), S))),
        'rbf_K: ell transposed': ('RBF', dict(rbf_K=lambda X, X2, ell, var: O_rbf_K(X, X2, ell.T, var))),
        'df_K: ell transposed': ('DF', dict(df_K=lambda X, X2, ell, var: O_df_K(X, X2, ell.T, var))),
        'rff_omega: ell transposed (RBF)': ('RBF', dict(rff_omega=lambda eps, ell: O_omega(eps, ell.T))),
        'rff_omega: ell transposed (DF)': ('DF', dict(rff_omega=lambda eps, ell: O_omega(eps, ell.T))),
        'df_compute_nu: the factor reads Ku.T': ('DF', dict(df_compute_nu=df_nu_upper)),
        'df_compute_nu: cholesky_backward on the lower triangle only': ('DF', dict(df_compute_nu=df_nu_lower_grad)),
    }


VAR_MUTANTS = ('df_K: var[a] for var[b]', 'rbf_K: var rolled by one', 'rbf_rff_forward: var rolled by one')


def mutant_names():
    return list(_mutants())


def mutant_kernel(name):
    return _mutants()[name][0]


@contextlib.contextmanager
def mutant(name):
    """the oracle with one function replaced"""
    from oracle import gpode_oracle as O
    patch = _mutants()[name][1]
    keep = {k: getattr(O, k) for k in patch}
    for k, v in patch.items():
        setattr(O, k, v)
    try:
        yield
    finally:
        for k, v in keep.items():
            setattr(O, k, v)


# ---- the cases of the GPU tests (test_gp_regimes_host.py holds every one of them to the caps) --------------------------------------------
def cache_cases():
    """[(mode, gp_routes case)]: the smallest cases that reach each separately written reader of ell / var in the cache build and
    its backward -- not the factor sizes: the linear algebra is parameter-blind and test_gpu_gp_routes.py covers it"""
    from gp_routes import C
    every = [C('RBF', 6, 6, 40, 1), C('DF', 6, 6, 16, 1),          # the LDS-resident build, the `solves` backward
             C('RBF', 6, 6, 192, 1), C('DF', 6, 6, 32, 1)]         # k_Kzz_*, the chain
    first = [('default', C('RBF', 6, 3, 100, 3)),                  # Di != Do, several draws
             ('default', C('RBF', 16, 8, 40, 1)), ('default', C('DF', 9, 9, 24, 1)),       # the wide half-record evaluators
             ('never', C('DF', 6, 6, 31, 5))]                      # inverse32 behind the LDS build, k_Kbwd_df with several draws
    return [('default', c._replace(regime=r)) for c in every for r in REGIMES] + \
        [(m, c._replace(regime=r)) for m, c in first for r in FIRST]


def integrator_cases():
    """integrator_routes cases: the first 'full' case of every forward route, one 'fused' case, the param_grad_df_split case and its 1023-row neighbour
    (param_grad_df: every resident DF route case has 1024 rows or more) in the four regimes of ROLL; the other four regimes on the RBF and the DF team case"""
    import integrator_routes as IR
    per_route = {}
    for c, route in IR.TABLE.items():
        if c.kind == 'full' and c.nd == 1:
            per_route.setdefault(route, c)
    assert set(per_route) == set(IR._F)
    fused = next(c for c in IR.TABLE if c.kind == 'fused')
    split, plain = IR.D_(6, 100, 256, 1024, 'euler', T=2), IR.D_(6, 100, 256, 1023, 'euler', T=2)     # the threshold of param_grad_df_split
    assert split in IR.TABLE and plain in IR.TABLE
    assert (IR.param_grad_route(split, IR.rows(split)), IR.param_grad_route(plain, IR.rows(plain))) == ('param_grad_df_split', 'param_grad_df')
    cases = [per_route[r] for r in IR._F] + [fused, split, plain]
    rest = [r for r in REGIMES if r not in ROLL]
    return [c._replace(regime=r) for c in cases for r in ROLL] + \
        [per_route[t]._replace(regime=r) for t in ('rbf_team', 'df_team') for r in rest]


OPERATOR_SHAPES = [('RBF', 6, 6, 40, 64), ('DF', 6, 6, 16, 64)]     # (kernel, Di, Do, M, S) of the public-operator tests
LAYER_SHAPES = [('RBF', 6, 6, 1, 40, 64), ('RBF', 6, 3, 2, 40, 64), ('DF', 6, 6, 1, 16, 64)]     # (kernel, Di, Do, order, M, S), rk4
LAYER_N, LAYER_T = 5, 4
OPERATOR_ROWS = 33


def operator_case(kernel, regime):
    """the integrator_routes case whose inputs the public-operator tests use: its parameters, noise and OPERATOR_ROWS states"""
    import integrator_routes as IR
    Di, Do, M, S = next(s[1:] for s in OPERATOR_SHAPES if s[0] == kernel)
    return IR.Case(kernel, Di, Do, 1, M, S, OPERATOR_ROWS, 3, 'rk4', 1, 'full', regime)
GATE_ROWS = 256                                       # trajectories of an integrator case the host gate integrates (the GPU test holds the caps on all)


def layer_inputs(kernel, Di, Do, order, M, S, regime):
    from test_gpu_backward import synthetic_gp
    p, nz, z0, ts, gw = synthetic_gp(kernel, Di, Do, M, S, LAYER_N, LAYER_T, seed=8000 + M + S + Di + 7 * Do)
    p, z0 = apply(regime, p, z0, kernel)
    return p, nz, z0, times(regime, ts), gw


INT_FWD = ('f0', 'f1', 'f2', 'zt', 'xstage')          # integrator_routes' outputs under FWD_CAP; its adjoints and leaf gradients under GRAD_CAP


def integrator_cap(key):
    return FWD_CAP if key in INT_FWD else GRAD_CAP


def gate_inputs(kind, item):
    """(kernel, p, draws, z0, ts, gw, order, method) of a cache case, an integrator case (its first GATE_ROWS trajectories), an
    operator shape or a layer shape in a regime: what well_posed() takes"""
    if kind == 'cache':
        import gp_routes as R
        p, nz, z0, ts, gw = R.inputs(item)
        return item.kernel, p, [{k: v[l] for k, v in nz.items()} for l in range(item.nd)], z0, ts, gw, item.Di // item.Do, R.METHOD
    if kind == 'integrator':
        import integrator_routes as IR
        p, nz, z0, ts, gw = IR.inputs(item)
        n = GATE_ROWS
        return item.kernel, p, [IR.draw(nz, item, l) for l in range(item.nd)], z0[:n], ts, gw[:, :n], item.order, item.method
    kernel, Di, Do, order, M, S, regime = item
    p, nz, z0, ts, gw = layer_inputs(kernel, Di, Do, order, M, S, regime)
    return kernel, p, [nz], z0, ts, gw[None], order, 'rk4'
