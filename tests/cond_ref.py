"""Reference and runner shared by the tests of gpode_dec10_predict_w (tests/test_gpu_cond_forecast.py).

The inputs are one fixed set: raw decnn.7 output c (L, F, 16, 28, 28), a BatchNorm table, decnn.10's weight and bias and the targets X, with
N = 3 sequences of Th = 5 frames of which T_obs = 4 have a target, L = 5 draws, F = 15 frames.  images() is the decoder's last stage
written out with torch.nn.functional -- relu of the table's affine map, conv_transpose2d, sigmoid -- in the dtype asked for, the way
tests/test_gpu_eval.py writes its float64 decoder; it is computed once per dtype and shared.  reference() forms the self-normalised
importance-weighted moments DIRECTLY: exact softmax weights, plain weighted sums (no running update, no rescaling), in float64 as the
reference and in float32 as the restatement whose own error enters the bound
    relerr(hip, fp64) <= 2e-5 + 3 relerr(fp32 restatement, fp64)        (the project's rule; relerr is the max-norm ratio).
run() drives the kernel through vae_ops.dec10_predict_w on state arrays that are NaN-filled with GUARD NaN floats behind each."""
import functools

import torch
import torch.nn.functional as Fn

GUARD = 4096
L, N, TH, T_OBS = 5, 3, 5, 4
F = N * TH
FLOOR = 2e-5


def relerr(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@functools.lru_cache(maxsize=None)
def inputs():
    g = torch.Generator().manual_seed(77)
    c = 1.5 * torch.randn(L, F, 16, 28, 28, generator=g)
    table = torch.stack([0.3 * torch.randn(16, generator=g), 0.5 + torch.rand(16, generator=g), 0.5 + torch.rand(16, generator=g),
                         0.3 * torch.randn(16, generator=g)], dim=1).contiguous()          # mean, invstd, gamma, beta
    w = 0.15 * torch.randn(16, 1, 5, 5, generator=g)
    b = 0.1 * torch.randn(1, generator=g)
    X = torch.rand(N, T_OBS, 1, 28, 28, generator=g)
    return dict(c=c, table=table, w=w, b=b, X=X)


@functools.lru_cache(maxsize=None)
def images(dtype):
    """sigmoid(decnn.10(relu(bn(c)))) of every (draw, frame): (L, N, Th, 784) in ``dtype`` on the CPU"""
    i = inputs()
    t = i['table'].to(dtype)
    h = torch.relu((i['c'].to(dtype).view(L * F, 16, 28, 28) - t[:, 0].view(1, 16, 1, 1)) * t[:, 1].view(1, 16, 1, 1) * t[:, 2].view(1, 16, 1, 1)
                   + t[:, 3].view(1, 16, 1, 1))
    return torch.sigmoid(Fn.conv_transpose2d(h, i['w'].to(dtype), i['b'].to(dtype), padding=2)).view(L, N, TH, 784)


def ess64(logw):
    w = torch.softmax(logw.double(), dim=0)
    return 1.0 / (w * w).sum(0)


def reference(logw, dtype, n_obs=None, draws=None):
    """mean, var (N,Th,784), wmse (N,Th) (0 where the frame has no target) and total (N,) = sum_l exp(logw) of the draws ``draws``
    (default: all), from exact softmax weights and direct weighted sums in ``dtype``"""
    idx = list(range(L)) if draws is None else list(draws)
    z = images(dtype)[idx]
    lw = logw.to(dtype)
    wn = torch.softmax(lw, dim=0)                                     # (l,N); -inf rows get exactly 0
    mean = (wn[:, :, None, None] * z).sum(0)
    var = (wn[:, :, None, None] * (z - mean[None]) ** 2).sum(0)
    X = inputs()['X'].to(dtype).view(N, T_OBS, 784)
    e = ((z[:, :, :T_OBS] - X[None]) ** 2).mean(-1)                    # (l,N,T_obs)
    wmse = torch.zeros(N, TH, dtype=dtype)
    wmse[:, :T_OBS] = (wn[:, :, None] * e).sum(0)
    if n_obs is not None:
        wmse = torch.where(torch.arange(TH)[None, :] < torch.as_tensor(n_obs)[:, None], wmse, torch.zeros((), dtype=dtype))
    return dict(mean=mean, var=var, wmse=wmse, total=torch.exp(lw).sum(0))


def guarded(*shape):
    """a NaN-filled buffer of the shape with GUARD NaN floats behind it: (the tensor, the guard)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), float('nan'), device='cuda')
    return buf[:n].view(*shape), buf[n:]


def run(logw, splits=None, n_obs=None, draws=None, X=None):
    """Fold the draws ``draws`` (default: all L) under the log-weights logw (len(draws), N) float32 in launches of ``splits`` draws.
    -> dict(wstate, mean, m2, wse: the raw state on the CPU; var, wmse, total: what the bound is put on; tags)"""
    from vae_gp_ode_amd import _lib, vae_ops as V
    i = inputs()
    idx = list(range(L)) if draws is None else list(draws)
    c = i['c'][idx].cuda()
    Ld = len(idx)
    st = V.CondState(F, N, 'cuda')
    guards = {}
    for name, shape in (('wstate', (F, 2)), ('mean', (F, 784)), ('m2', (F, 784)), ('wse', (F,))):
        buf, guards[name] = guarded(*shape)
        setattr(st, name, buf)
    Xd = (i['X'] if X is None else X).cuda()
    lw = logw.float().contiguous().cuda()
    nb = None if n_obs is None else torch.as_tensor(n_obs, dtype=torch.int32).cuda()
    l0, tags = 0, []
    for n in (splits or [Ld]):
        V.dec10_predict_w(c[l0:l0 + n].reshape(-1, 16, 28, 28), i['table'].cuda(), i['w'].cuda(), i['b'].cuda(), Xd, TH, st, lw, n_obs=nb)
        tags.append(_lib.load().gpode_last_launch().decode())
        l0 += n
    assert l0 == Ld and st.done == Ld
    st.check()
    torch.cuda.synchronize()
    for name, g in guards.items():
        assert torch.isnan(g).all(), 'the guard behind %s changed' % name
    out = {k: getattr(st, k).cpu().clone() for k in ('wstate', 'mean', 'm2', 'wse')}
    ref, W = out['wstate'][:, 0].double(), out['wstate'][:, 1].double()
    out['var'] = (out['m2'].double() / W[:, None]).view(N, TH, 784)
    out['wmse'] = (out['wse'].double() / W).view(N, TH)
    out['total'] = (W * torch.exp(ref)).view(N, TH)
    out['tags'] = tags
    return out


def check(got, logw64, what, n_obs=None, draws=None):
    """the bound on mean, M2/W, wse/W and W exp(ref), each figure printed before it is asserted"""
    r64, r32 = reference(logw64, torch.float64, n_obs, draws), reference(logw64, torch.float32, n_obs, draws)
    pairs = [('mean', got['mean'].view(N, TH, 784), 'mean'), ('M2/W', got['var'], 'var'), ('wse/W', got['wmse'], 'wmse'),
             ('W exp(ref)', got['total'], 'total')]
    res = []
    for name, g, k in pairs:
        want = r64[k] if k != 'total' else r64[k][:, None].expand(N, TH)
        e, e32 = relerr(g, want), relerr(r32[k], r64[k])
        print('%s %-10s: %.2e from float64 (float32 restatement %.2e, bound %.2e)' % (what, name, e, e32, FLOOR + 3 * e32))
        res.append((name, e, FLOOR + 3 * e32))
    for name, e, bound in res:
        assert e <= bound, (what, name, e, bound)
    return r64
