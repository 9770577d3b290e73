"""Every route of the BatchNorm family and the channel reductions (csrc/vae_norm.hip), shared by test_gpu_bn_routes.py, by the child
process it starts and by test_bn_routes_host.py.

A case is (op, B, C, H, W_img, relu, offset, chansum, running, shards):

  op        fwd         gpode_bn_fwd
            stats       gpode_bn_stats, then gpode_bn_apply with the table it wrote
            bwd         gpode_bn_fwd for the saved statistics, then gpode_bn_bwd
            xrank       the five cross-rank pieces on one device, one simulated rank per entry of `shards` (images per rank)
            eval        gpode_bn_eval forward and backward
            eval_table  gpode_bn_eval_table, gpode_bn_apply with it, gpode_bn_eval
            chan_sum    gpode_chan_sum
  offset    the channel mean in units of the channel's standard deviation, 0 or 100
  chansum   gx_chansum is given (bwd, xrank);  running: running statistics and the counter are given (fwd, stats, xrank)

expected() restates the dispatch of bn_fwd / bn_stats / bn_bwd on its own (it never asks the library).  launch() drives the C ABI on
buffers it owns: every output and the scratch NaN-filled, the scratch exactly gpode_bn_scratch(B, C) floats, GUARD floats of
GUARD_VALUE behind every buffer; it runs the case twice and returns the outputs, the tag gpode_last_launch() gave after every call
and what the buffer checks found.  reference() is torch on the CPU in fp64 on the same fp32 inputs.

Inputs without ReLU coin-flips (inputs()): an fp32 kernel and an fp64 reference disagree on the mask of a pre-activation within
round-off of zero, and one such element is an O(1) error in gx.  So u ~ randn per element, a crossing point u0[c] per channel, every
u within `gap` of u0[c] moved out to u0[c] +- gap, x = scale[c] (u + offset) with scale in [0.3, 2.3], gamma in +-[0.5, 1.5] (30 %
negative), and beta[c] computed in fp64 from the fp32 x so that the pre-activation is zero exactly at scale[c] (u0[c] + offset).  gap
is 1e-3 spreads of the channel, at least 1e-3: for one rank the spread is ~1 and the gap is 1e-3; for `xrank`, where shard r gets an
offset of its own of r standard deviations (so that n_r (mean_r - mean)^2 is a large part of the variance), the spread is up to 18.5
(64 shards) and a fixed 1e-3 in u would leave |gamma| 1e-3 / 18.5 = 2.7e-5 of pre-activation, under the 1e-4 that reference()
asserts.  With the gap in place every comparison is in the max norm."""
import collections
import ctypes
import functools
import os
import subprocess
import sys
import tempfile

import torch
import torch.nn.functional as F

from conv_dispatch import GUARD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD_VALUE = -12345.0
MOM, EPS = 0.1, 1e-5
NBT0 = 7
SMALL_FWD, SMALL_BWD = 20000, 2048          # kBnSmallFwd, kBnSmallBwd: elements per channel
MAX_RANKS = 64
TOL, TOL_STATS = 2e-5, 1e-5                 # test_gpu_vae_layers.TOL; save / running statistics and eval mode in the existing tests
MIN_PRE = 1e-4

Case = collections.namedtuple('Case', 'op B C H W_img relu offset chansum running shards')


def case(op, B, C, H, W_img, relu=1, offset=0, chansum=False, running=False, shards=()):
    return Case(op, B, C, H, W_img, relu, offset, chansum, running, tuple(shards))


def case_id(c):
    s = '%s-%dx%dx%dx%d-relu%d-off%d' % c[:7]
    return s + ('-cs' if c.chansum else '') + ('-run' if c.running else '') + ('-W%d' % len(c.shards) if c.shards else '')


def one_launch_on():
    """the switch as this process reads it (bn_small: GPODE_BN_ONE_LAUNCH starting with '0' turns the one-launch kernels off)"""
    return os.environ.get('GPODE_BN_ONE_LAUNCH', '')[:1] != '0'


# ---- the dispatch, restated --------------------------------------------------------------------------------------------------------
def pick(B):
    """(ns, bps, used): at most 64 slabs of bps = ceil(B / ns) images, `used` of them non-empty, the last one ragged"""
    ns = min(B, 64)
    bps = -(-B // ns)
    return ns, bps, -(-B // bps)


def _local(name, per_channel, limit, on):
    return name + (' (one launch)' if on and per_channel <= limit else '')


def expected(c, on=True):
    """{step: tag} of the calls launch() makes for case c, with the one-launch switch on or off"""
    per = c.B * c.H * c.W_img
    fwd = _local('bn_fwd', per, SMALL_FWD, on)
    if c.op == 'fwd':
        return dict(fwd=fwd)
    if c.op == 'stats':
        return dict(stats=_local('bn_stats', per, SMALL_FWD, on), apply='bn_apply')
    if c.op == 'bwd':
        return dict(fwd=fwd, bwd=_local('bn_bwd', per, SMALL_BWD, on))
    if c.op == 'xrank':
        return dict(moments='bn_moments', finalize='bn_finalize', apply='bn_apply', bwd_sums='bn_bwd_sums', bwd_apply='bn_bwd_apply')
    if c.op == 'eval':
        return dict(eval_fwd='bn_eval', eval_bwd='bn_eval')
    if c.op == 'eval_table':
        return dict(eval_table='bn_eval_table', apply='bn_apply', eval_fwd='bn_eval')
    assert c.op == 'chan_sum', c.op
    return dict(chan_sum='chan_sum')


REQUIRED_TAGS = ('bn_fwd', 'bn_fwd (one launch)', 'bn_stats', 'bn_stats (one launch)', 'bn_bwd', 'bn_bwd (one launch)', 'bn_moments',
                 'bn_finalize', 'bn_apply', 'bn_bwd_sums', 'bn_bwd_apply', 'bn_eval', 'bn_eval_table', 'chan_sum')


def sum_terms(c, one_launch, B=None):
    """ceil(bps HW / 256) + 12: the additions an element of a channel sum passes through (its thread's share of the slab, then the
    wavefront, the workgroup and the slabs), the factor of 2^-24 sum |v| in the worst case of a fixed-order fp32 summation"""
    B = c.B if B is None else B
    bps = B if one_launch else pick(B)[1]
    return -(-bps * c.H * c.W_img // 256) + 12


# ---- the case tables ---------------------------------------------------------------------------------------------------------------
def threshold_cases():
    """item 1: the two sides of kBnSmallFwd at two image sizes (fwd, stats) and of kBnSmallBwd (bwd), relu 0/1, offset 0/100"""
    out = []
    for relu in (0, 1):
        for off in (0, 100):
            for B, C, H in ((1250, 4, 4), (1251, 4, 4), (555, 3, 6), (556, 3, 6)):
                out.append(case('fwd', B, C, H, H, relu, off, running=True))
                out.append(case('stats', B, C, H, H, relu, off, running=True))
            for B in (128, 129):
                out.append(case('bwd', B, 4, 4, 4, relu, off, chansum=True))
    return out


SPLIT_B = (1, 2, 63, 64, 65, 127, 128, 129, 130, 193)


def split_cases():
    """item 2: the edges of pick(B) on C = 3 at HW = 13 x 13 (scalar path) and 6 x 6 (float4 path)"""
    out = []
    for H in (13, 6):
        for B in SPLIT_B:
            out += [case('fwd', B, 3, H, H, 1, 100, running=True), case('fwd', B, 3, H, H, 0, 0, running=False),
                    case('bwd', B, 3, H, H, 1, 100, chansum=True), case('bwd', B, 3, H, H, 0, 0, chansum=False),
                    case('eval', B, 3, H, H, 1, 0), case('eval', B, 3, H, H, 0, 100),
                    case('chan_sum', B, 3, H, H, 0, 0)]
    return out


def image_cases():
    """item 3: HW = 1, 3 and 9 (chan_shift averages fewer than 64 elements), 49, 289 (scalar, HW > 256), 784, 1296 (float4, HW / 4 >
    256), C in {1, 5, 64}; the last two are 289 and 1296 past the forward threshold, on the two-launch kernels"""
    shapes = ((40, 1, 1, 1), (40, 5, 1, 1), (40, 64, 1, 1), (5, 5, 1, 3), (7, 64, 3, 3), (3, 1, 7, 7), (2, 5, 17, 17), (3, 5, 28, 28),
              (2, 1, 36, 36), (70, 1, 17, 17), (16, 5, 36, 36))
    out = []
    for i, (B, C, H, W) in enumerate(shapes):
        relu, off = i % 2, 100 * ((i // 2) % 2)
        out += [case('fwd', B, C, H, W, relu, off, running=True), case('stats', B, C, H, W, relu, off, running=True),
                case('bwd', B, C, H, W, relu, off, chansum=True), case('bwd', B, C, H, W, 1 - relu, 100 - off, chansum=False)]
    return out


XRANK_SHARDS = ((200,), (33, 33), (3, 70, 1, 130), tuple(1 + i % 2 for i in range(64)))


def xrank_cases():
    """item 6: one rank, two equal ranks, four unequal ranks with a one-image shard, the 64 ranks the kernels support"""
    return [case('xrank', sum(s), 5, H, H, relu, 100 * relu, chansum=True, running=True, shards=s)
            for s in XRANK_SHARDS for H in (3, 6) for relu in (0, 1)]


def eval_table_cases():
    return [case('eval_table', 5, C, 3, 3, 1, 0) for C in (1, 63, 64, 65)]


def local_cases():
    return threshold_cases() + split_cases() + image_cases()


def child_cases():
    """item 4: the cases of items 1-3 that lie under a threshold: with GPODE_BN_ONE_LAUNCH=0 they take the two-launch kernels"""
    return [c for c in local_cases() if expected(c, True) != expected(c, False)]


def all_cases():
    return local_cases() + xrank_cases() + eval_table_cases()


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _family(op):
    return {'fwd': 'train', 'stats': 'train', 'bwd': 'train', 'xrank': 'train', 'eval': 'eval', 'eval_table': 'eval', 'chan_sum': 'sum'}[op]


def _slices(shards):
    """(rows of shard r, its size) in rank order"""
    a = 0
    for n in shards:
        yield slice(a, a + n), n
        a += n


def _ranks(c):
    """the shards of case c; one rank holding everything is the local layer: the same inputs, the same reference"""
    return c.shards if len(c.shards) > 1 else ()


def _rows(shards, B):
    """the shard of every image"""
    shards = shards or (B,)
    assert sum(shards) == B
    return torch.repeat_interleave(torch.arange(len(shards)), torch.tensor(shards))


def _layer(d, mean, invstd, relu, shards, B):
    """y, per-shard gx / ggamma / gbeta of the layer in fp64 from GIVEN statistics (the formulas of the header, include/gpode.h)"""
    x, gy, gam, bet = d['x'].double(), d['gy'].double(), d['gamma'].double(), d['beta'].double()
    sh = shards or (B,)
    onehot = F.one_hot(_rows(sh, B), len(sh)).double()
    xh = (x - mean[None, :, None]) * invstd[None, :, None]
    pre = xh * gam[None, :, None] + bet[None, :, None]
    g = gy * (pre > 0) if relu else gy
    sa, sb = torch.einsum('bw,bch->wc', onehot, g), torch.einsum('bw,bch->wc', onehot, g * xh)
    n = torch.tensor(sh, dtype=torch.float64)
    w = n[None, :] / n[:, None]                                                       # w[r][q] = B_q / B_r
    ca, cb = (w @ sa) / (B * x.shape[2]), (w @ sb) / (B * x.shape[2])                   # (W, C): rank r's centring terms
    gx = (gam * invstd)[None, :, None] * (g - (onehot @ ca)[:, :, None] - xh * (onehot @ cb)[:, :, None])
    return dict(y=pre.clamp_min(0) if relu else pre, gx=gx, ggamma=sb, gbeta=sa)


def _rounding_sensitivity(d, shards, B):
    """What rounding the exact batch statistics to fp32 -- the format of save_mean / save_invstd, so a change no fp32 layer can avoid
    -- does to y, gx (per shard), ggamma and gbeta, each relative to its largest entry, over relu 0 and 1.  A channel mean of 100
    standard deviations moves xhat by up to 3e-6 that way and ggamma by that times gbeta: where C = 1 and ggamma happens to be a
    small sum, this alone can be several 1e-5 of it."""
    xc = d['x'].double().transpose(0, 1).reshape(d['x'].shape[1], -1)
    mean, invstd = xc.mean(1), 1.0 / torch.sqrt(xc.var(1, unbiased=False) + EPS)
    worst = 0.0
    for relu in (0, 1):
        a, b = _layer(d, mean, invstd, relu, shards, B), _layer(d, mean.float().double(), invstd.float().double(), relu, shards, B)
        worst = max([worst] + [relerr(b[k], a[k]) for k in ('y', 'ggamma', 'gbeta')]
                    + [relerr(b['gx'][sl], a['gx'][sl]) for sl, _ in _slices(shards or (B,))])
    return worst


@functools.lru_cache(maxsize=None)
def _inputs(family, B, C, H, W_img, offset, shards):
    """The first of at most 20 draws whose compared quantities are well conditioned: _rounding_sensitivity() under TOL / 4 (a property
    of the inputs and the number format alone -- the library is not asked)."""
    seed = 1000003 * B + 1009 * C + 31 * H + W_img + 7 * offset + 13 * len(shards) + 3 * ('train', 'eval', 'sum').index(family)
    for attempt in range(20):
        d = _draw(seed + 7919 * attempt, family, B, C, H, W_img, offset, shards)
        if family != 'train':
            return d
        d['sensitivity'] = torch.tensor(_rounding_sensitivity(d, shards, B))
        if d['sensitivity'] < TOL / 4:
            return d
    raise AssertionError('no well-conditioned draw', (family, B, C, H, W_img, offset, shards))


def _draw(seed, family, B, C, H, W_img, offset, shards):
    HW = H * W_img
    g = torch.Generator().manual_seed(seed)
    f64 = dict(generator=g, dtype=torch.float64)
    v = torch.randn(B, C, HW, **f64) + _rows(shards, B).double()[:, None, None]       # shard r: r standard deviations of its own
    per = v.transpose(0, 1).reshape(C, -1)
    gap = 1e-3 * per.std(1, unbiased=False).clamp_min(1.0)
    u0 = per.mean(1) + 0.5 * torch.randn(C, **f64)
    d = v - u0[None, :, None]
    side = torch.where(d < 0, -1.0, 1.0).double()
    v = torch.where(d.abs() < gap[None, :, None], u0[None, :, None] + side * gap[None, :, None], v)
    scale = 0.3 + 2.0 * torch.rand(C, **f64)
    x = (scale[None, :, None] * (v + offset)).float()
    gamma = (torch.where(torch.rand(C, **f64) < 0.3, -1.0, 1.0) * (0.5 + torch.rand(C, **f64))).float()
    xc = x.double().transpose(0, 1).reshape(C, -1)
    if family == 'eval':                            # the frozen layer normalises with the running statistics: the crossing is set by them
        rm = (scale * (per.mean(1) + offset + 0.2 * torch.randn(C, **f64))).float()
        rv = (scale ** 2 * per.var(1, unbiased=False).clamp_min(1.0) * (0.5 + torch.rand(C, **f64))).float()
        m, var = rm.double(), rv.double()
    else:                                           # running statistics that are neither 0 / 1 nor what the batch has
        rm, rv = (0.3 * torch.randn(C, **f64)).float(), (0.4 + torch.rand(C, **f64)).float()
        m, var = xc.mean(1), xc.var(1, unbiased=False)
    beta = (-gamma.double() * (scale * (u0 + offset) - m) / torch.sqrt(var + EPS)).float()
    gy = torch.randn(B, C, HW, **f64).float()
    return dict(x=x, gamma=gamma, beta=beta, gy=gy, rm=rm, rv=rv)


def inputs(c):
    """fp32 inputs of case c on the CPU (shared by every op of its family, relu 0 and 1 alike): x, gy (B, C, HW), gamma, beta, rm, rv"""
    return _inputs(_family(c.op), c.B, c.C, c.H, c.W_img, c.offset, _ranks(c))


# ---- reference ---------------------------------------------------------------------------------------------------------------------
def reference(c):
    """fp64 results of case c: torch's F.batch_norm (+ F.relu) with autograd on the fp32 inputs.  pre_min = min |pre-activation|."""
    return _reference(_family(c.op), c.B, c.C, c.H, c.W_img, c.relu, c.offset, _ranks(c))


@functools.lru_cache(maxsize=None)
def _reference(family, B, C, H, W_img, relu, offset, shards):
    d = _inputs(family, B, C, H, W_img, offset, shards)
    x = d['x'].double().requires_grad_(True)
    if family == 'sum':
        return dict(sums=d['x'].double().sum((0, 2)), abs_sums=d['x'].double().abs().sum((0, 2)))
    gam, bet = d['gamma'].double().requires_grad_(True), d['beta'].double().requires_grad_(True)
    rm, rv = d['rm'].double().clone(), d['rv'].double().clone()
    pre = F.batch_norm(x, rm, rv, gam, bet, family == 'train', MOM, EPS)               # (B, C, HW): normalised over dims 0 and 2
    y = F.relu(pre) if relu else pre
    out = dict(pre_min=float(pre.detach().abs().min()))
    assert out['pre_min'] >= MIN_PRE, ('a pre-activation within round-off of zero', out['pre_min'])
    if family == 'eval':
        y.backward(d['gy'].double())
        out.update(y=y.detach(), gx=x.grad, invstd=1.0 / torch.sqrt(rv + EPS))
        return out
    # cross-rank: the whole-batch layer with the data-parallel loss, which weights every rank's loss by its share of the batch
    sh = shards or (B,)
    rows, total = _rows(sh, B), float(B)
    share = torch.tensor(sh, dtype=torch.float64)[rows] / total
    gy = d['gy'].double()
    y.backward(gy * share[:, None, None])
    xd = x.detach()
    mean = xd.mean((0, 2))
    invstd = 1.0 / torch.sqrt(xd.var((0, 2), unbiased=False) + EPS)
    xhat = (xd - mean[None, :, None]) * invstd[None, :, None]
    g = gy * (pre.detach() > 0) if relu else gy
    onehot = F.one_hot(rows, len(sh)).double()                                        # (B, W)
    out.update(y=y.detach(), save_mean=mean, save_invstd=invstd, running_mean=rm, running_var=rv, unbiased_var=xd.var((0, 2), unbiased=True),
               gx=x.grad / share[:, None, None],                                      # (sum B / B_r) gx_global[shard r]
               ggamma=torch.einsum('bw,bch->wc', onehot, g * xhat), gbeta=torch.einsum('bw,bch->wc', onehot, g))
    out['gx_sums'] = torch.einsum('bw,bch->wc', onehot, out['gx'])
    out['gx_abs_sums'] = torch.einsum('bw,bch->wc', onehot, out['gx'].abs())
    if len(sh) == 1:
        out['autograd'] = dict(ggamma=gam.grad, gbeta=bet.grad)                       # the layer's own affine gradients
    return out


def emulate_xrank(c):
    """The five pieces in fp64 as the kernels compute them, independent of autograd: per-shard {mean, M2, n}, the rank-ordered
    combination of Chan et al., the table, the per-shard masked sums, gx from sum_q w_q sums_q / count_all."""
    d = inputs(c)
    x, gy, gam, bet = d['x'].double(), d['gy'].double(), d['gamma'].double(), d['beta'].double()
    HW, bounds = c.H * c.W_img, [0]
    for n in c.shards:
        bounds.append(bounds[-1] + n)
    xs = [x[a:b] for a, b in zip(bounds, bounds[1:])]
    mom = [(s.mean((0, 2)), ((s - s.mean((0, 2))[None, :, None]) ** 2).sum((0, 2)), float(s.shape[0] * HW)) for s in xs]
    count = sum(n for _, _, n in mom)
    mean = sum(n * m for m, _, n in mom) / count
    var = sum(q + n * (m - mean) ** 2 for m, q, n in mom) / count
    invstd = 1.0 / torch.sqrt(var + EPS)
    rmean = (1 - MOM) * d['rm'].double() + MOM * mean
    rvar = (1 - MOM) * d['rv'].double() + MOM * var * (count / (count - 1))
    ys, sums, gs, xhs = [], [], [], []
    for s, a, b in zip(xs, bounds, bounds[1:]):
        xh = (s - mean[None, :, None]) * invstd[None, :, None]
        pre = xh * gam[None, :, None] + bet[None, :, None]
        g = gy[a:b] * (pre > 0) if c.relu else gy[a:b]
        ys.append(pre.clamp_min(0) if c.relu else pre)
        sums.append((g.sum((0, 2)), (g * xh).sum((0, 2))))
        gs.append(g)
        xhs.append(xh)
    gx = []
    for r, (g, xh) in enumerate(zip(gs, xhs)):
        w = [c.shards[q] / c.shards[r] for q in range(len(c.shards))]
        ca = sum(wq * sa for wq, (sa, _) in zip(w, sums)) / count
        cb = sum(wq * sb for wq, (_, sb) in zip(w, sums)) / count
        gx.append((gam * invstd)[None, :, None] * (g - ca[None, :, None] - xh * cb[None, :, None]))
    return dict(y=torch.cat(ys), save_mean=mean, save_invstd=invstd, running_mean=rmean, running_var=rvar, gx=torch.cat(gx),
                ggamma=torch.stack([sb for _, sb in sums]), gbeta=torch.stack([sa for sa, _ in sums]))


# ---- launches ----------------------------------------------------------------------------------------------------------------------
class Refused(Exception):
    pass


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


class Buffers:
    """NaN-filled device buffers with GUARD floats of GUARD_VALUE behind each; problems() says which guard was written and which
    output still holds a NaN"""
    def __init__(self):
        self.guards, self.outs = {}, {}

    def new(self, name, n, init=None, dtype=torch.float32, output=True):
        buf = torch.full((n + GUARD,), GUARD_VALUE, device='cuda', dtype=dtype)
        if init is None:
            buf[:n] = float('nan')
        else:
            buf[:n] = init.reshape(-1).to('cuda', dtype)
        assert name not in self.guards, name
        self.guards[name] = buf[n:]
        if output:
            self.outs[name] = buf[:n]
        return buf[:n]

    def problems(self):
        torch.cuda.synchronize()
        bad = []
        for dt in (torch.float32, torch.int64):
            names = [k for k, g in self.guards.items() if g.dtype == dt]
            if names:
                hit = (torch.stack([self.guards[k] for k in names]) != GUARD_VALUE).any(1).cpu()
                bad += ['%s: the guard behind it was written' % k for k, h in zip(names, hit) if h]
        bad += ['%s: a NaN of the fill is left' % k for k, v in self.outs.items() if v.is_floating_point() and torch.isnan(v).any()]
        return bad

    def cpu(self):
        return {k: v.cpu().clone() for k, v in self.outs.items()}


def _call(tags, step, name, *args):
    """one entry point; its tag goes to tags[step] (every call of a step must give the same one)"""
    from vae_gp_ode_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise Refused(lib.gpode_last_error().decode())
    tag = lib.gpode_last_launch().decode()
    assert tags.setdefault(step, tag) == tag, (step, tags[step], tag)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _scratch(b, name, B, C):
    from vae_gp_ode_amd import _lib
    return b.new(name, int(_lib.load().gpode_bn_scratch(B, C)), output=False)


def _stat_outputs(b, d, c, pre=''):
    C = c.C
    sm, si = b.new(pre + 'save_mean', C), b.new(pre + 'save_invstd', C)
    if not c.running:
        return sm, si, None, None, None
    return (sm, si, b.new(pre + 'running_mean', C, d['rm']), b.new(pre + 'running_var', C, d['rv']),
            b.new(pre + 'nbt', 1, torch.tensor([NBT0]), torch.int64))


# With momentum 0.1 and 2e4 elements per channel the factor count / (count - 1) of the running variance is 0.1 / 2e4 = 5e-6 of it, under
# the 1e-5 it is held to.  So every case with running statistics runs once more with momentum 1 (outputs 'mom1_...'): running_var is
# then the unbiased batch variance itself, 1 / count = 3e-5 away from the biased one at the largest case, and running_mean is save_mean.
MOM1 = 'mom1_'


def _run_fwd(b, tags, d, c, pre='', mom=MOM):
    B, C, HW = c.B, c.C, c.H * c.W_img
    y = b.new(pre + 'y', B * C * HW)
    sm, si, rm, rv, nbt = _stat_outputs(b, d, c, pre)
    _call(tags, 'fwd', 'gpode_bn_fwd', _ptr(d['x']), _ptr(d['gamma']), _ptr(d['beta']), _ptr(y), _ptr(sm), _ptr(si), _ptr(rm), _ptr(rv),
          _ptr(nbt), mom, EPS, B, C, HW, c.relu, _ptr(_scratch(b, pre + 'scratch_fwd', B, C)), _stream())
    if c.running and not pre:
        _run_fwd(b, tags, d, c, MOM1, 1.0)
    return sm, si


def _run_stats(b, tags, d, c, pre='', mom=MOM):
    B, C, HW = c.B, c.C, c.H * c.W_img
    sm, si, rm, rv, nbt = _stat_outputs(b, d, c, pre)
    table = b.new(pre + 'table', 4 * C)
    _call(tags, 'stats', 'gpode_bn_stats', _ptr(d['x']), _ptr(d['gamma']), _ptr(d['beta']), _ptr(sm), _ptr(si), _ptr(rm), _ptr(rv), _ptr(nbt),
          mom, EPS, _ptr(table), B, C, HW, _ptr(_scratch(b, pre + 'scratch_stats', B, C)), _stream())
    y = b.new(pre + 'y', B * C * HW)
    _call(tags, 'apply', 'gpode_bn_apply', _ptr(d['x']), _ptr(table), _ptr(y), B, C, HW, c.relu, _stream())
    if c.running and not pre:
        _run_stats(b, tags, d, c, MOM1, 1.0)


def _run_bwd(b, tags, d, c):
    B, C, HW = c.B, c.C, c.H * c.W_img
    sm, si = _run_fwd(b, tags, d, c)
    gx, gg, gb = b.new('gx', B * C * HW), b.new('ggamma', C), b.new('gbeta', C)
    cs = b.new('gx_chansum', C) if c.chansum else None
    _call(tags, 'bwd', 'gpode_bn_bwd', _ptr(d['x']), _ptr(d['gy']), _ptr(d['gamma']), _ptr(d['beta']), _ptr(sm), _ptr(si), _ptr(gx), _ptr(gg),
          _ptr(gb), _ptr(cs), B, C, HW, c.relu, _ptr(_scratch(b, 'scratch_bwd', B, C)), _stream())


def _run_eval(b, tags, d, c):
    B, C, HW = c.B, c.C, c.H * c.W_img
    y, gx = b.new('y', B * C * HW), b.new('gx', B * C * HW)
    for step, gy, out in (('eval_fwd', None, y), ('eval_bwd', d['gy'], gx)):
        _call(tags, step, 'gpode_bn_eval', _ptr(d['x']), _ptr(gy), _ptr(d['gamma']), _ptr(d['beta']), _ptr(d['rm']), _ptr(d['rv']), EPS,
              _ptr(out), B, C, HW, c.relu, _stream())


def _run_eval_table(b, tags, d, c):
    B, C, HW = c.B, c.C, c.H * c.W_img
    table, y, y_eval = b.new('table', 4 * C), b.new('y', B * C * HW), b.new('y_eval', B * C * HW)
    _call(tags, 'eval_table', 'gpode_bn_eval_table', _ptr(d['gamma']), _ptr(d['beta']), _ptr(d['rm']), _ptr(d['rv']), EPS, _ptr(table), C, _stream())
    _call(tags, 'apply', 'gpode_bn_apply', _ptr(d['x']), _ptr(table), _ptr(y), B, C, HW, c.relu, _stream())
    _call(tags, 'eval_fwd', 'gpode_bn_eval', _ptr(d['x']), None, _ptr(d['gamma']), _ptr(d['beta']), _ptr(d['rm']), _ptr(d['rv']), EPS,
          _ptr(y_eval), B, C, HW, c.relu, _stream())


def _run_chan_sum(b, tags, d, c):
    out = b.new('sums', c.C)
    _call(tags, 'chan_sum', 'gpode_chan_sum', _ptr(d['x']), _ptr(out), c.B, c.C, c.H * c.W_img, _ptr(_scratch(b, 'scratch', c.B, c.C)), _stream())


def _run_xrank(b, tags, d, c):
    """Every rank's pieces in rank order on one device, the all-gathers as torch.stack.  Outputs: per-shard tensors concatenated in rank
    order (y, gx: (B, C, HW); ggamma, gbeta, gx_chansum: (W, C)), the statistics of rank 0, `finalize_differs` (names)."""
    C, HW, W = c.C, c.H * c.W_img, len(c.shards)
    bounds = [0]
    for n in c.shards:
        bounds.append(bounds[-1] + n)
    xs = [d['x'][a:e].contiguous() for a, e in zip(bounds, bounds[1:])]
    gys = [d['gy'][a:e].contiguous() for a, e in zip(bounds, bounds[1:])]
    scr = [_scratch(b, 'scratch%d' % r, n, C) for r, n in enumerate(c.shards)]
    moms = [b.new('moments%d' % r, 2 * C + 1) for r in range(W)]
    for r, n in enumerate(c.shards):
        _call(tags, 'moments', 'gpode_bn_moments', _ptr(xs[r]), _ptr(moms[r]), n, C, HW, _ptr(scr[r]), _stream())
    gathered = torch.stack(moms)
    stats = []
    for rep in ('', 'again_', MOM1):                 # every rank runs this on the same gathered moments: the same bits
        sm, si, table = b.new(rep + 'save_mean', C), b.new(rep + 'save_invstd', C), b.new(rep + 'table', 4 * C)
        rm, rv = b.new(rep + 'running_mean', C, d['rm']), b.new(rep + 'running_var', C, d['rv'])
        nbt = b.new(rep + 'nbt', 1, torch.tensor([NBT0]), torch.int64)
        _call(tags, 'finalize', 'gpode_bn_finalize', _ptr(gathered), W, _ptr(d['gamma']), _ptr(d['beta']), _ptr(sm), _ptr(si), _ptr(rm), _ptr(rv),
              _ptr(nbt), 1.0 if rep == MOM1 else MOM, EPS, _ptr(table), C, _stream())
        stats.append((sm, si, table, rm, rv, nbt))
    sm, si, table = stats[0][:3]
    ys = [b.new('y%d' % r, n * C * HW) for r, n in enumerate(c.shards)]
    for r, n in enumerate(c.shards):
        _call(tags, 'apply', 'gpode_bn_apply', _ptr(xs[r]), _ptr(table), _ptr(ys[r]), n, C, HW, c.relu, _stream())
    for r, n in enumerate(c.shards):                 # the backward's scratch: NaN again, so that nothing of the forward's is read
        scr[r].fill_(float('nan'))
    sums = [b.new('sums%d' % r, 2 * C) for r in range(W)]
    for r, n in enumerate(c.shards):
        _call(tags, 'bwd_sums', 'gpode_bn_bwd_sums', _ptr(xs[r]), _ptr(gys[r]), _ptr(d['gamma']), _ptr(d['beta']), _ptr(sm), _ptr(si),
              _ptr(sums[r]), n, C, HW, c.relu, _ptr(scr[r]), _stream())
    sums_gathered = torch.stack(sums)
    count_all = float(c.B * HW)
    parts = dict(gx=[], ggamma=[], gbeta=[], gx_chansum=[])
    for r, n in enumerate(c.shards):
        wts = torch.tensor([q / n for q in c.shards], dtype=torch.float32, device='cuda')
        gx, gg, gb = b.new('gx%d' % r, n * C * HW), b.new('ggamma%d' % r, C), b.new('gbeta%d' % r, C)
        cs = b.new('gx_chansum%d' % r, C) if c.chansum else None
        _call(tags, 'bwd_apply', 'gpode_bn_bwd_apply', _ptr(xs[r]), _ptr(gys[r]), _ptr(d['gamma']), _ptr(d['beta']), _ptr(sm), _ptr(si),
              _ptr(sums_gathered), _ptr(wts), W, count_all, _ptr(gx), _ptr(gg), _ptr(gb), _ptr(cs), n, C, HW, c.relu, _ptr(scr[r]), _stream())
        for k, v in zip(('gx', 'ggamma', 'gbeta', 'gx_chansum'), (gx, gg, gb, cs)):
            if v is not None:
                parts[k].append(v)
    torch.cuda.synchronize()
    names = ('save_mean', 'save_invstd', 'table', 'running_mean', 'running_var', 'nbt')
    out = dict(y=torch.cat(ys), gx=torch.cat(parts['gx']), ggamma=torch.stack(parts['ggamma']), gbeta=torch.stack(parts['gbeta']),
               finalize_differs=[k for k, u, v in zip(names, *stats[:2]) if not torch.equal(u, v)])
    out.update((MOM1 + k, v) for k, v in zip(names, stats[2]))
    if c.chansum:
        out['gx_chansum'] = torch.stack(parts['gx_chansum'])
    out.update(zip(names, stats[0]))
    return out


_RUN = dict(fwd=_run_fwd, stats=_run_stats, bwd=_run_bwd, eval=_run_eval, eval_table=_run_eval_table, chan_sum=_run_chan_sum, xrank=_run_xrank)


def _once(c, d):
    b, tags = Buffers(), {}
    merged = _RUN[c.op](b, tags, d, c)
    problems = b.problems()
    out = b.cpu() if c.op != 'xrank' else {k: (v.cpu().clone() if torch.is_tensor(v) else v) for k, v in merged.items()}
    return out, tags, problems


def launch(c):
    """Case c TWICE; the record of the first run with what the buffer checks of both found and what differs in the second"""
    d = {k: v.cuda() for k, v in inputs(c).items()}
    (out, tags, problems), (out2, tags2, problems2) = _once(c, d), _once(c, d)
    differs = [k for k in out if not (torch.equal(out[k], out2[k]) if torch.is_tensor(out[k]) else out[k] == out2[k])]
    return dict(out=out, tags=tags, problems=problems + problems2 + ['the second run differs in %s' % k for k in differs]
                + ([] if tags == tags2 else ['the second run took %s' % tags2]))


# ---- comparison --------------------------------------------------------------------------------------------------------------------
def relerr(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _shard_slices(c):
    return _slices(c.shards or (c.B,))


def check(c, got, on=True, seen=None, maxima=None):
    """got (launch(), or a child's record of it) against the dispatch table and the fp64 reference; prints every figure before it
    asserts.  The two-launch and one-launch forms of an op are separate groups in `maxima`."""
    assert not isinstance(got, str), (case_id(c), got)
    want, out = expected(c, on), got['out']
    print('%s %s' % (case_id(c), got['tags']))
    if seen is not None:
        seen.update(got['tags'].values())
    assert got['tags'] == want, (case_id(c), got['tags'], want)
    assert not got['problems'], (case_id(c), got['problems'])
    ref = reference(c)
    errs, bad = {}, []

    def cmp(name, a, r, tol, group):
        e = errs[name] = relerr(a, r)
        if maxima is not None:
            key = '%s: %s' % (group, 'statistics' if tol == TOL_STATS and c.op not in ('eval', 'eval_table') else 'outputs')
            maxima[key] = max(maxima.get(key, 0.0), e)
        if not e < tol:
            bad.append((name, e, tol))

    def cmp_chansum(cs, gx, group):
        # gx sums to ZERO over a channel of the whole batch, so the fp64 channel sums are no yardstick: the kernel's sum against the
        # fp64 sum of the kernel's own gx (itself held to the reference), within the worst case of a fixed-order summation
        one = group.endswith('(one launch)')
        worst = 0.0
        for r, (sl, n) in enumerate(_shard_slices(c)):
            bound = 2.0 ** -24 * sum_terms(c, one, n) * ref['gx_abs_sums'][r]
            err = (cs.double().reshape(-1, c.C)[r] - gx.double().reshape(c.B, c.C, -1)[sl].sum((0, 2))).abs()
            worst = max(worst, float((err / bound).max()))
        errs['gx_chansum / bound'] = worst
        if not worst <= 1.0:
            bad.append(('gx_chansum', worst, 1.0))

    if c.op in ('fwd', 'stats', 'bwd', 'xrank'):
        group = got['tags'].get('fwd') or got['tags'].get('stats') or 'xrank'
        cmp('y', out['y'], ref['y'], TOL, group)
        for k in ('save_mean', 'save_invstd') + (('running_mean', 'running_var') if c.running else ()):
            cmp(k, out[k], ref[k], TOL_STATS, group)
        if c.running:
            assert int(out['nbt']) == NBT0 + 1, (case_id(c), 'num_batches_tracked', int(out['nbt']))
            cmp('unbiased var', out[MOM1 + 'running_var'], ref['unbiased_var'], TOL_STATS, group)
            differs = [k for k in ('save_mean', 'save_invstd', 'nbt') + (('y',) if c.op != 'xrank' else ()) if not torch.equal(out[MOM1 + k], out[k])]
            assert not differs and torch.equal(out[MOM1 + 'running_mean'], out['save_mean']), (case_id(c), 'with momentum 1', differs)
        if c.op in ('stats', 'xrank'):
            cmp('table', out['table'].reshape(c.C, 4).double(),
                torch.stack([ref['save_mean'], ref['save_invstd'], inputs(c)['gamma'].double(), inputs(c)['beta'].double()], 1), TOL_STATS, group)
    if c.op in ('bwd', 'xrank'):
        group = got['tags'].get('bwd') or 'xrank'
        for r, (sl, n) in enumerate(_shard_slices(c)):                               # gx per shard: a one-image shard's is (sum B) times larger
            cmp('gx[%d]' % r if c.shards else 'gx', out['gx'].reshape(c.B, c.C, -1)[sl], ref['gx'][sl], TOL, group)
        cmp('ggamma', out['ggamma'], ref['ggamma'], TOL, group)
        cmp('gbeta', out['gbeta'], ref['gbeta'], TOL, group)
        if c.chansum:
            cmp_chansum(out['gx_chansum'], out['gx'], group)
        if c.op == 'xrank':
            assert not out['finalize_differs'], (case_id(c), 'gpode_bn_finalize twice', out['finalize_differs'])
    if c.op == 'eval':
        cmp('y', out['y'], ref['y'], TOL_STATS, 'bn_eval')
        cmp('gx', out['gx'], ref['gx'], TOL_STATS, 'bn_eval')
    if c.op == 'eval_table':
        d = inputs(c)
        t = out['table'].reshape(c.C, 4)
        assert torch.equal(t[:, 0], d['rm']) and torch.equal(t[:, 2], d['gamma']) and torch.equal(t[:, 3], d['beta']), case_id(c)
        cmp('invstd', t[:, 1], ref['invstd'], 1e-6, 'bn_eval_table')
        cmp('y', out['y'], ref['y'], TOL_STATS, 'bn_eval_table')
        assert torch.equal(out['y'], out['y_eval']), (case_id(c), 'gpode_bn_apply with the table against gpode_bn_eval')
    if c.op == 'chan_sum':
        bound = 2.0 ** -24 * sum_terms(c, False) * ref['abs_sums']
        errs['sums / bound'] = float(((out['sums'].double() - ref['sums']).abs() / bound).max())
        if maxima is not None:
            maxima['chan_sum: error / bound'] = max(maxima.get('chan_sum: error / bound', 0.0), errs['sums / bound'])
        if not errs['sums / bound'] <= 1.0:
            bad.append(('sums', errs['sums / bound'], 1.0))
    print('  ' + ', '.join('%s %.1e' % kv for kv in errs.items()))
    assert not bad, (case_id(c), bad)


# ---- the child process -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def child():
    """Every case of child_cases() in ONE fresh child process with GPODE_BN_ONE_LAUNCH=0 (the switch is read once per process), under a
    time limit of its own: {case: record | error text}"""
    tmp = tempfile.mkdtemp()
    fn = os.path.join(tmp, 'two_launch.pt')
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), fn], env=dict(os.environ, GPODE_BN_ONE_LAUNCH='0'),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        return torch.load(fn)
    finally:
        if os.path.exists(fn):
            os.remove(fn)
        os.rmdir(tmp)


def _child_main(fn):
    sys.path.insert(0, ROOT)
    assert not one_launch_on()
    out = {}
    for c in child_cases():
        try:
            out[tuple(c)] = launch(c)
        except Exception as e:                        # reported by the parent, per case (the library's refusals included)
            out[tuple(c)] = '%s: %s' % (type(e).__name__, e)
    torch.save(out, fn)


if __name__ == '__main__':
    _child_main(sys.argv[1])
