"""Sub-steps of the fixed-grid solvers (Flow(substeps=s), the `_ns` entry points) -- what test_substeps_host.py and test_gpu_substeps.py share.

s solver steps inside every output interval are, by definition, one step per interval of the REFINED grid refine(ts, s) with every s-th
frame kept: the tests hold the `_ns` launch to the `_nt` launch on the refined grid (bit for bit where the refined grid's differences are
exact in float32) and to the fp64 oracle on the refined grid."""
import torch


def refine(ts, s):
    """ts (T,) or (N,T) -> (.., (T-1) s + 1): ts[j] + (ts[j+1] - ts[j]) k / s for k = 0 .. s-1 in every interval j, then ts[-1]; in the
    dtype of ts.  refine(ts, 1) is ts, and refine(ts, s)[..., ::s] is ts for every s."""
    if s < 1 or ts.dim() not in (1, 2) or ts.shape[-1] < 1:
        raise ValueError('refine: ts %s, s %r' % (tuple(ts.shape), s))
    lo, gap = ts[..., :-1, None], (ts[..., 1:] - ts[..., :-1])[..., None]
    k = torch.arange(s, dtype=ts.dtype, device=ts.device)
    inner = (lo + gap * k / s).reshape(ts.shape[:-1] + (-1,))
    return torch.cat([inner, ts[..., -1:]], -1)


def scatter_frames(g, s):
    """g (.., T, D) -> (.., (T-1) s + 1, D) with g in every s-th frame and zeros between: dL/dzt of the refined grid when the loss reads
    the output frames only"""
    T = g.shape[-2]
    out = g.new_zeros(g.shape[:-2] + ((T - 1) * s + 1, g.shape[-1]))
    out[..., ::s, :] = g
    return out


# grids whose entries, and the entries of refine(., 2) and refine(., 4), are small multiples of 2^-7: every difference and every quotient
# by 2 or 4 is exact in float32, so the `_ns` launch and the `_nt` launch on the refined grid take the same steps to the bit
T_EXACT = 4


def exact_grids(N):
    """{name: grid}: uniform, non-uniform (gaps 0.25, 0.5, 0.125), and (N,T) with step 0.125 (1 + n mod 3) in row n"""
    uniform = 0.25 * torch.arange(T_EXACT, dtype=torch.float32)
    gaps = torch.tensor([0.0, 0.25, 0.5, 0.125])
    per_row = 0.125 * (1 + torch.arange(N) % 3)[:, None].float() * torch.arange(T_EXACT, dtype=torch.float32)[None]
    return {'uniform': uniform, 'gaps': torch.cumsum(gaps, 0), 'rows': per_row.contiguous()}
