"""Reference values for the tangent-linear rollout (csrc/gp_tangent.hip), shared by test_gpu_tangent.py and
test_gpu_flow_diagnostics.py: the oracle (oracle/gpode_oracle.py) differentiated in forward mode by torch -- autograd.functional.jvp
through O.odeint_fixed for Phi_t v0, autograd.functional.jacobian of O.gp_forward / gp_prior / gp_update for J_f -- on the cache
the GPU built (integrator_routes.cache_dicts), in float64 and, for the bounds, in float32.

The bound is the project's: relerr(X_hip, X_64) <= FLOOR + 3 relerr(X_32, X_64), FLOOR = 2e-5 for every output (no floor has been
raised)."""
import torch

from substeps_ref import refine

FLOOR = 2e-5
PARTS = ('gp_forward', 'gp_prior', 'gp_update')          # mode 0, 1, 2


def bound(e32, scale=1.0):
    return (FLOOR + 3 * e32) * scale


def in_dtype(cd, dtype):
    return {k: (v.detach().to(dtype) if torch.is_tensor(v) else v) for k, v in cd.items()}


def identity(lead, D, dtype=torch.float32):
    """the identity directions ([L,] N, D, D): row k is e_k"""
    return torch.eye(D, dtype=dtype).expand(tuple(lead) + (D, D)).contiguous()


def jacobian(cd, x, dtype, mode=0):
    """J_f (R,Do,Di) at the rows x (R,Di) of one draw's cache: rows are independent, so the Jacobian of the sum over rows is the stack"""
    from oracle import gpode_oracle as O
    cl, fn = in_dtype(cd, dtype), getattr(O, PARTS[mode])
    J = torch.autograd.functional.jacobian(lambda y: fn(y, cl).sum(0), x.to(dtype))        # (Do,R,Di)
    return J.permute(1, 0, 2).contiguous()


def rollout(cache, order, method, dtype, z0, ts, v0=None, substeps=1):
    """(zt (L,N,T,D), vt (L,N,T,K,D)) of the oracle's fixed-grid solver and its tangent, one cache dict per draw.  z0 (N,D) or (L,N,D);
    v0 ([L,] N,K,D) with the leading layout of z0, None: the identity; ts (T,) or (N,T); substeps: the refined grid, every s-th frame
    kept."""
    from oracle import gpode_oracle as O
    L = len(cache)
    z0, ts = z0.to(dtype), refine(ts.to(dtype), substeps)
    grid = ts if ts.dim() == 1 else ts.T[:, :, None].contiguous()                            # (T,N,1): a step size per row
    D = z0.shape[-1]
    v0 = identity(z0.shape[:-1], D, dtype) if v0 is None else v0.to(dtype)
    zs, vs = [], []
    for l, cd in enumerate(cache):
        cl = in_dtype(cd, dtype)
        z, v = (z0[l], v0[l]) if z0.dim() == 3 else (z0, v0)

        def f(y):
            fv = O.gp_forward(y, cl)
            return fv if order == 1 else torch.cat([y[:, D // 2:], fv], 1)

        def flow(y):
            return O.odeint_fixed(f, y, grid, method).permute(1, 0, 2)[:, ::substeps]
        cols = [torch.autograd.functional.jvp(flow, z, v[:, k].contiguous()) for k in range(v.shape[1])]
        zs.append(cols[0][0].detach())
        vs.append(torch.stack([c[1].detach() for c in cols], 2))
    return torch.stack(zs), torch.stack(vs)


def transpose_defect(cache, order, method, dtype, z0, ts, v0, gw):
    """The oracle's own defect of <gz0, v0> = sum_t <gw_t, vt_t> in ``dtype``, relative to sum_t |gw_t| |vt_t|: gz0 by reverse mode
    (autograd of sum(zt * gw)), vt by forward mode.  Max over draws, trajectories and columns."""
    from oracle import gpode_oracle as O
    _, vt = rollout(cache, order, method, dtype, z0, ts, v0)
    gw, D = gw.to(dtype), z0.shape[-1]
    worst = 0.0
    for l, cd in enumerate(cache):
        cl = in_dtype(cd, dtype)
        z = z0.to(dtype).clone().requires_grad_(True)

        def f(y):
            fv = O.gp_forward(y, cl)
            return fv if order == 1 else torch.cat([y[:, D // 2:], fv], 1)
        zt = O.odeint_fixed(f, z, ts.to(dtype), method).permute(1, 0, 2)
        (zt * gw[l]).sum().backward()
        worst = max(worst, defect(z.grad, v0.to(dtype), gw[l], vt[l]))
    return worst


def defect(gz0, v0, gw, vt):
    """max over (n, k) of |<gz0_n, v0_nk> - sum_t <gw_nt, vt_ntk>| / sum_t |gw_nt| |vt_ntk|, in float64"""
    gz0, v0, gw, vt = (t.detach().double().cpu() for t in (gz0, v0, gw, vt))
    lhs = torch.einsum('nd,nkd->nk', gz0, v0)
    rhs = torch.einsum('ntd,ntkd->nk', gw, vt)
    scale = torch.einsum('nt,ntk->nk', gw.norm(dim=-1), vt.norm(dim=-1))
    return ((lhs - rhs).abs() / scale).max().item()
