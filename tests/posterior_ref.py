"""The yardstick of the DF posterior (gpode_conditional_df, SVGP_Layer.posterior): its definition in plain torch on top of the
oracle's df_K, in the dtype of its inputs (float64: the reference; float32: the twin that sizes the bound).  Shared by
test_posterior_host.py (CPU) and test_gpu_posterior_df.py.

Definition (from the sampling path -- sample_inducing, df_compute_nu, df_f_update -- not from the RBF einsums), n = M D, rows and
columns of K(Z) ordered (m, a) as df_K orders them:
    L = chol(K(Z) + jitter I)                      (the lower triangle is read, as the cache build does)
    A = L^-1 K(Z, x)            (M D, N D)         column j = (n, b);  a_j = column j viewed as (M, D)
    t_{j,d} = Us_d^T a_j[:, d]  (M,)               Us_d the lower-triangular scale of output d
    mean[n, b]  = sum_{m,d} a_j[m, d] Um[m, d]
    cov[j, j']  = K(x, x)[j, j'] + sum_d t_{j,d} . t_{j',d} - a_j . a_j'
With dimwise hyper-parameters the DF matrix is not symmetric (ell by (a, b), var by b): K(Z, x) enters, as in df_f_update, and
K(x, x) is taken as df_K(x, x) returns it.  ``transposed_fill=True`` states the WRONG variant K(x, Z)^T, for the test that shows the
two apart.

Bound (the form test_gpu_forward.py uses for build_conditional): relerr(got, ref64) < 1e-4 + 3 relerr(ref32, ref64), norm-wise
(largest difference over the largest reference entry), over the mean, the marginals, the point blocks and the full covariance
separately."""
import torch

from oracle import gpode_oracle as O


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def factor(p):
    """(ell, var, L) of the parameter dict p (raw_ell (D,D), raw_var (D), Z (M,D), ...)"""
    ell, var = O.softplus(p['raw_ell']), O.softplus(p['raw_var'])
    n = p['Z'].numel()
    L = torch.linalg.cholesky(O.df_K(p['Z'], None, ell, var) + torch.eye(n, dtype=p['Z'].dtype) * O.JITTER)
    return ell, var, L


def scales(p):
    """dense lower-triangular Us (D,M,M): the packed triangle, or diag(softplus(raw)) for a q_diag layer's raw (M,D) scale"""
    M = p['Um'].shape[0]
    if O.is_q_diag(p['Us'], p['Um']):
        return torch.diag_embed(O.softplus(p['Us']).T)
    return O.tril_unpack(p['Us'], M)


def posterior(p, x, transposed_fill=False):
    """dict(mean (N,D), diag (N,D), point (N,D,D), full (N D, N D)) of q(f(x))"""
    M, D = p['Um'].shape
    N = x.shape[0]
    ell, var, L = factor(p)
    Kzx = O.df_K(x, p['Z'], ell, var).T if transposed_fill else O.df_K(p['Z'], x, ell, var)
    A = torch.linalg.solve_triangular(L, Kzx, upper=False)                      # (M D, N D)
    a = A.T.reshape(N * D, M, D)                                                # a[j, m, d]
    t = torch.einsum('dmk,jmd->jkd', scales(p), a)                              # t[j, k, d] = sum_m Us_d[m, k] a[j, m, d]
    mean = torch.einsum('jmd,md->j', a, p['Um']).reshape(N, D)
    full = O.df_K(x, None, ell, var) + t.reshape(N * D, -1) @ t.reshape(N * D, -1).T - A.T @ A
    blocks = full.reshape(N, D, N, D)
    idx = torch.arange(N)
    return dict(mean=mean, diag=torch.diagonal(full).reshape(N, D).clone(), point=blocks[idx, :, idx, :].clone(), full=full)


def inputs(M, D, N, seed, z_spread=1.5, us_identity=False):
    """The recipe of the GPU cases, float32 on the CPU: (p, x).  Half the queries sit within 0.05 of inducing points."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    Z = z_spread * r(M, D)
    Us = torch.stack([torch.eye(M)] * D) if us_identity else torch.tril(0.2 * r(D, M, M)) + 0.5 * torch.eye(M)
    p = dict(raw_ell=O.invsoftplus(2.0 + 0.02 * torch.rand(D, D, generator=g)), raw_var=O.invsoftplus(0.7 + 0.2 * torch.rand(D, generator=g)),
             Z=Z, Um=0.3 * r(M, D), Us=O.tril_pack(Us))
    near = N // 2
    pick = torch.randint(0, M, (near,), generator=g)
    x = torch.cat([Z[pick] + 0.05 * (2 * torch.rand(near, D, generator=g) - 1) / D ** 0.5, 2 * r(N - near, D)])
    return p, x


def references(p, x, **kw):
    """(ref64, ref32): the definition in float64 and its float32 twin"""
    return posterior(O.to_dtype(p, torch.float64), x.double(), **kw), posterior(p, x, **kw)


def within(got, ref64, ref32, what):
    """assert the bound for one quantity; returns (distance, allowance)"""
    e, tw = relerr(got, ref64[what]), relerr(ref32[what], ref64[what])
    print('%s: relerr vs fp64 %.3e, fp32 twin %.3e' % (what, e, tw))
    assert e < 1e-4 + 3 * tw, (what, e, tw)
    return e, tw
