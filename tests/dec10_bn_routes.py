"""Every route of the decoder's fused last-stage backward -- dec10::k_bwd_data_bn<IPB, MODE, WGRAD> (csrc/conv_dec10_mfma.hpp) behind
gpode_dec10_bn_bwd_sums[_wgrad] and gpode_dec10_bn_bwd_apply (csrc/vae_conv_tiled.hip) -- shared by test_gpu_dec10_bn_routes.py and
test_dec10_bn_routes_host.py.

A case is (B, wgrad, gbias, sums, chansum, shards):

  wgrad    the sums pass is gpode_dec10_bn_bwd_sums_wgrad (decnn.10's weight gradient rides in it), else gpode_dec10_bn_bwd_sums
  gbias    the _wgrad form is given gbias (NULL otherwise: part_b stays unwritten)
  sums     the sums pass is given sums[32] (NULL otherwise; with shards it is always given: it is what the ranks exchange)
  chansum  the apply pass is given gc_chansum (NULL otherwise: part_gx stays unwritten)
  shards   images per simulated rank, () = the local form (sums_gathered == NULL); one entry = `gathered` with one rank of weight 1

expected(B, n) restates (ipb, nwg) from the CU count alone (it never asks the library): ipb = 4 from 4 n images on, else 2; a grid of
min(groups, min(2 n, 512)) persistent workgroups, n clamped to 256 as num_cus() clamps it.

Inputs: c, gamma and beta are bn_routes._inputs('train', B, 16, 28, 28, 0, shards) -- no ReLU coin-flips, every pre-activation at least
bn_routes.MIN_PRE from zero -- with gy (B, 1, 28, 28) ~ randn, w (16, 1, 5, 5) ~ 0.05 randn and a non-zero bias from a fixed seed.
save_mean / save_invstd are the whole-batch fp64 statistics ROUNDED TO fp32, and reference() uses those same fp32 values (as
bn_routes._layer does with given statistics), so the rounding of the statistics is not part of the error.

reference(case) is fp64 on the CPU: ga = conv2d(gy, w, padding 2), then the header's formulas through bn_routes._layer with ga in place
of gy (masked g, per-shard {sum g, sum g xhat}, gc of rank r from sum_q (B_q / B_r) sums_q / count_all, ggamma / gbeta the shard's own
sums), gw[ci][tap] = sum relu(bn(c))[ci][p] gy[window(p, tap)] and gbias = sum gy per shard, and the per-shard channel sums of |gc|.
reference(case, only=b): gy zero except in image b.  autograd_reference() is torch.autograd on conv_transpose2d(relu(batch_norm(c)), w,
bias, padding 2) in fp64 under the share-weighted data-parallel loss (the host test holds the closed form to it at 1e-10).

launch(case) drives the C ABI on buffers it owns: every output and both scratch buffers NaN-filled, the scratches exactly
gpode_dec10_bn_scratch_floats() / gpode_dec10_bn_wgrad_scratch_floats() floats, GUARD floats of GUARD_VALUE behind every buffer (SLACK =
three images' worth behind c and gc: a kernel that takes a ragged group for a full one then stays inside the buffers); it runs
the case twice (the second run must give the same bits), reads gpode_last_launch() after every call and reports how many floats of each
scratch region were written.  With shards every shard is a sums launch of its own (its own B, its own scratch), the sums[32] rows are
stacked in rank order into gathered[W][32], and every shard runs its own apply with weights[q] = B_q / B_r and count_all = 784 sum B:
what parallel.BatchNormSync computes, on one device.

GPODE_CONV_VALU=1 is not a mode of this stage: the fused entry points ignore the switch, and the unfused twin of the weight-gradient
pass (gpode_conv2d_bwd_weight_bn) is refused on the decoder layers under it, so the stage has no VALU form to test."""
import collections
import functools

import torch
import torch.nn.functional as F

import bn_routes as R
import conv_dispatch as D
from conv_dispatch import GUARD

C, H, HW, KK = 16, 28, 784, 25
MAX_WG = 512                                        # kDec10BnMaxWg
MAX_CUS = 256                                       # num_cus() clamps the CU count: the split-sum scratch is sized for it
TOL = R.TOL                                         # gc, ggamma, gbeta, sums: what the existing fused test holds gc to
TOL_W = 5 * D.TOL                                   # gw, gbias: test_gpu_conv_wgrad.py
TAG_SUMS, TAG_WGRAD, TAG_APPLY = 'dec10_bn_bwd_sums', 'dec10_bn_bwd_sums_wgrad', 'dec10_bn_bwd_apply'
SEED = 20251

Case = collections.namedtuple('Case', 'B wgrad gbias sums chansum shards')


def case(B, wgrad=True, gbias=True, sums=True, chansum=True, shards=()):
    shards = tuple(shards)
    assert not shards or sum(shards) == B
    return Case(B, wgrad, gbias and wgrad, sums or bool(shards), chansum, shards)


def case_id(c):
    flags = ('wgrad' if c.wgrad else 'plain') + ('' if c.gbias or not c.wgrad else '-nogbias') + ('' if c.sums else '-nosums') + \
        ('' if c.chansum else '-nochansum')
    return 'B%d-%s%s' % (c.B, flags, '-W%d(%s)' % (len(c.shards), '.'.join(map(str, c.shards[:4])) + ('..' if len(c.shards) > 4 else ''))
                         if c.shards else '')


# ---- the dispatch, restated --------------------------------------------------------------------------------------------------------
def cap(n):
    return min(2 * min(n, MAX_CUS), MAX_WG)


def expected(B, n):
    """(ipb, nwg) of dec10_bn_nwg on a device of n CUs"""
    n = min(n, MAX_CUS)
    ipb = 4 if B >= 4 * n else 2
    return ipb, min(-(-B // ipb), cap(n))


def chansum_terms(B, n):
    """The additions an element of gc passes through on its way into gc_chansum, the factor of 2^-24 sum |gc| in the worst case of a
    fixed-order fp32 summation.  A lane of k_bwd_data_bn adds into a0 the four pixels of every tile it takes: tiles t = wave, wave + 8,
    ... of the ipb * 49 of a group, ceil(49 ipb / 8) of them, for each of the ceil(groups / nwg) groups of its workgroup.  Then one
    thread adds the 32 rows of s_red in order (32), and k_reduce_multi adds the nwg partials as 16 interleaved chains of ceil(nwg / 16)
    and those 16 in order (16)."""
    ipb, nwg = expected(B, n)
    groups = -(-B // ipb)
    return 4 * -(-49 * ipb // 8) * -(-groups // nwg) + 32 + -(-nwg // 16) + 16


# ---- the case tables (batch sizes from the CU count n) -----------------------------------------------------------------------------
def edge_sizes(n):
    """1, 2, 3: one group, with IPB = 2 one of them ragged; n + 1; 4 n - 1: the last IPB = 2 size, ragged; 4 n: the first IPB = 4 size;
    4 n + 1 / 2 / 3: IPB = 4 with a ragged last group of 1 / 2 / 3 images; 4 cap + 5: workgroup 0 takes a full second group and
    workgroup 1 a one-image second group, both with the register prefetch in flight"""
    return (1, 2, 3, n + 1, 4 * n - 1, 4 * n, 4 * n + 1, 4 * n + 2, 4 * n + 3, 4 * cap(n) + 5)


def edge_cases(n):
    return [case(B, wgrad=wg) for B in edge_sizes(n) for wg in (False, True)]


def attribution_cases(n):
    """(B, b*): the first image, the last of the last full round / group, the first of the ragged part, the last image"""
    big, small = 4 * cap(n) + 5, 4 * n + 3
    return [(big, b) for b in (0, 4 * cap(n) - 1, 4 * cap(n), big - 1)] + [(small, b) for b in (0, 4 * n - 1, 4 * n, small - 1)]


def shard_sets(n):
    """three unequal ranks; ranks on both sides of n; an IPB = 4 rank with a ragged group next to IPB = 2 ranks; 16 small unequal ranks"""
    return ((3, 1, 2), (n + 1, 1, 2 * n + 1), (4 * n + 2, 1, 3, 7), tuple(1 + (5 * i) % 4 for i in range(16)))


def shard_cases(n):
    return [case(sum(s), shards=s) for s in shard_sets(n)]


def one_rank_sizes(n):
    return (3, 4 * n + 3)


def optional_sizes(n):
    return (n + 1, 4 * n + 3)


def optional_cases(n):
    return [case(B, **{k: False}) for B in optional_sizes(n) for k in ('sums', 'gbias', 'chansum')]


def input_keys(n):
    """(B, shards) of every draw the GPU file's tables need on a device of n CUs"""
    keys = {(B, ()) for B in edge_sizes(n) + one_rank_sizes(n) + optional_sizes(n)} | {(B, ()) for B, _ in attribution_cases(n)}
    return sorted(keys | {(sum(s), s) for s in shard_sets(n)})


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _ranks(shards):
    return tuple(shards) if len(shards) > 1 else ()


@functools.lru_cache(maxsize=None)
def _inputs(B, shards):
    d = R._inputs('train', B, C, H, H, 0, shards)
    g = torch.Generator().manual_seed(SEED + B)
    f64 = dict(generator=g, dtype=torch.float64)
    gy = torch.randn(B, 1, H, H, **f64).float()
    w = (0.05 * torch.randn(C, 1, 5, 5, **f64)).float()
    bias = (0.3 + 0.1 * torch.randn(1, **f64)).float()
    xc = d['x'].double().transpose(0, 1).reshape(C, -1)
    mean64, invstd64 = xc.mean(1), 1.0 / torch.sqrt(xc.var(1, unbiased=False) + R.EPS)
    return dict(c=d['x'], gamma=d['gamma'], beta=d['beta'], gy=gy, w=w, bias=bias, mean=mean64.float(), invstd=invstd64.float(),
                mean64=mean64, invstd64=invstd64)


def inputs(c):
    """fp32 inputs of case c on the CPU: c (B, 16, 784), gamma, beta, gy (B, 1, 28, 28), w, bias, mean, invstd (fp32-rounded)"""
    return _inputs(c.B, _ranks(c.shards))


# ---- reference ---------------------------------------------------------------------------------------------------------------------
def _windows(gy):
    """(B, 25, 784): column p of row tap = gy[window(p, tap)] = gy[iy + ky - 2][ix + kx - 2], zero outside the image"""
    gp = F.pad(gy[:, 0], (2, 2, 2, 2))
    return torch.stack([gp[:, ky:ky + H, kx:kx + H] for ky in range(5) for kx in range(5)], 1).reshape(gy.shape[0], KK, HW)


def reference(c, only=None):
    return _reference(c.B, _ranks(c.shards), only)


def _pre(d, mean, invstd):
    return ((d['c'].double() - mean[None, :, None]) * invstd[None, :, None]) * d['gamma'].double()[None, :, None] + d['beta'].double()[None, :, None]


@functools.lru_cache(maxsize=None)
def pre_min(B, shards):
    """min |gamma xhat + beta| with the fp32 statistics the kernels are given: a condition on the inputs, not on the library"""
    d = _inputs(B, shards)
    return float(_pre(d, d['mean'].double(), d['invstd'].double()).abs().min())


def closed_form(B, shards, mean, invstd, only=None, gy=None):
    """the stage's backward in fp64 from GIVEN statistics (fp64 tensors), by the header's formulas (gy: in place of the drawn one)"""
    d = _inputs(B, shards)
    sh = shards or (B,)
    rows = R._rows(sh, B)
    x, gy, w, pre = d['c'].double(), (d['gy'] if gy is None else gy).double(), d['w'].double(), _pre(d, mean, invstd)
    if only is not None:                            # gy is zero elsewhere: every sum is that of image `only`, the statistics stay the batch's
        x, gy, pre, rows = x[only:only + 1], gy[only:only + 1], pre[only:only + 1], rows[only:only + 1] * 0
        sh, shards = (1,), ()
    n = x.shape[0]
    ga = F.conv2d(gy, w, padding=2).reshape(n, C, HW)
    lay = R._layer(dict(x=x, gy=ga, gamma=d['gamma'], beta=d['beta']), mean, invstd, 1, shards, n)
    onehot = F.one_hot(rows, len(sh)).double()
    gw_img = torch.einsum('bcp,btp->bct', pre.clamp_min(0), _windows(gy))               # (n, 16, 25)
    out = dict(ggamma=lay['ggamma'], gbeta=lay['gbeta'], sums=torch.stack([lay['gbeta'], lay['ggamma']], 2).reshape(-1, 2 * C),
               gw=torch.einsum('bw,bct->wct', onehot, gw_img).reshape(-1, C * KK), gbias=onehot.t() @ gy.sum((1, 2, 3))[:, None])
    if only is None:
        out.update(gc=lay['gx'], gc_abs_sums=torch.einsum('bw,bch->wc', onehot, lay['gx'].abs()))
    return out


@functools.lru_cache(maxsize=None)
def _reference(B, shards, only):
    d = _inputs(B, shards)
    assert pre_min(B, shards) >= R.MIN_PRE, ('a pre-activation within round-off of zero', pre_min(B, shards))
    return closed_form(B, shards, d['mean'].double(), d['invstd'].double(), only)


def conv_transpose_by_fold(a, w, bias):
    """F.conv_transpose2d(a, w, bias, padding=2) for a (B, 16, 784) and decnn.10's w as the matrix product with w[ci][tap] followed by
    col2im: the same function and differentiable alike, but seconds instead of half a minute in fp64 at a thousand images (the host
    test holds it to F.conv_transpose2d)"""
    return F.fold(torch.matmul(w.reshape(C, KK).t(), a), (H, H), 5, padding=2) + bias.view(1, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def autograd_reference(B, shards=(), by_fold=True):
    """torch.autograd in fp64 on the whole stage with statistics of its own (exact, not rounded): gc (per shard over its share of the
    loss, as bn_routes._reference), ggamma, gbeta, gw, gbias of the loss sum_r share_r <gy_r, y_r>, and y"""
    d = _inputs(B, shards)
    sh = shards or (B,)
    share = torch.tensor(sh, dtype=torch.float64)[R._rows(sh, B)] / B
    leaves = [d[k].double().requires_grad_(True) for k in ('c', 'gamma', 'beta', 'w', 'bias')]
    x, gam, bet, w, bias = leaves
    pre = F.batch_norm(x, None, None, gam, bet, True, R.MOM, R.EPS)
    pre_min = float(pre.detach().abs().min())
    assert pre_min >= R.MIN_PRE, ('a pre-activation within round-off of zero', pre_min)
    y = conv_transpose_by_fold(F.relu(pre), w, bias) if by_fold else F.conv_transpose2d(F.relu(pre).reshape(B, C, H, H), w, bias, padding=2)
    y.backward(d['gy'].double() * share[:, None, None, None])
    return dict(y=y.detach(), gc=x.grad / share[:, None, None], ggamma=gam.grad, gbeta=bet.grad, gw=w.grad.reshape(-1), gbias=bias.grad,
                pre_min=pre_min)


# ---- launches ----------------------------------------------------------------------------------------------------------------------
def _lib():
    from vae_gp_ode_amd import _lib
    return _lib.load()


def scratch_floats():
    lib = _lib()
    return int(lib.gpode_dec10_bn_scratch_floats()), int(lib.gpode_dec10_bn_wgrad_scratch_floats())


def _prefix(region):
    """how many leading floats of a NaN-filled region were written; -1 if what was written is not a prefix"""
    w = ~torch.isnan(region)
    k = int(w.sum())
    return k if bool(w[:k].all()) else -1


SLACK = 3 * C * HW                                  # IPB - 1 images of c / gc: what a kernel that took a ragged group for a full one touches


class Buffers(R.Buffers):
    """bn_routes.Buffers with a guard of the caller's length: behind gc it is SLACK floats, so that a kernel which writes the images a
    ragged group lacks writes into the guard -- reported, and inside the buffer"""
    def new(self, name, n, output=True, guard=GUARD):
        buf = torch.full((n + guard,), R.GUARD_VALUE, device='cuda')
        buf[:n] = float('nan')
        assert name not in self.guards, name
        self.guards[name] = buf[n:]
        if output:
            self.outs[name] = buf[:n]
        return buf[:n]

    def problems(self):
        torch.cuda.synchronize()
        bad = ['%s: the guard behind it was written' % k for k, g in self.guards.items() if bool((g != R.GUARD_VALUE).any())]
        return bad + ['%s: a NaN of the fill is left' % k for k, v in self.outs.items() if bool(torch.isnan(v).any())]


def device_inputs(c, only=None):
    """the fp32 inputs on the device; c with SLACK floats of GUARD_VALUE behind it (read by mistake, they are the whole error)"""
    d = {k: v.cuda() for k, v in inputs(c).items() if v.dtype == torch.float32 and k != 'c'}
    buf = torch.full((c.B * C * HW + SLACK,), R.GUARD_VALUE, device='cuda')
    buf[:c.B * C * HW] = inputs(c)['c'].reshape(-1).cuda()
    d['c'] = buf[:c.B * C * HW].view(c.B, C, HW)
    if only is not None:
        gy = torch.zeros_like(d['gy'])
        gy[only] = d['gy'][only]
        d['gy'] = gy
    return d


def _once(c, d, apply=True, deferred=False):
    """one run of case c on the device tensors d: (outputs on the device, tags, extents per shard, problems)"""
    lib, p, st = _lib(), R._ptr, R._stream()
    b, tags, notes = Buffers(), {}, []
    sh = c.shards or (c.B,)
    SCR, WSCR = scratch_floats()
    head = lambda sl: (p(d['c'][sl]), p(d['gy'][sl]), p(d['w']), p(d['gamma']), p(d['beta']), p(d['mean']), p(d['invstd']))
    scr, wscr, parts = [], [], collections.defaultdict(list)
    late = []                                       # outputs of final reductions: valid only after the flush when deferred
    if deferred:
        lib.gpode_defer_reductions(2)
    try:
        for r, (sl, nr) in enumerate(R._slices(sh)):
            scr.append(b.new('scratch%d' % r, SCR, output=False))
            sums = b.new('sums%d' % r, 2 * C) if c.sums else None
            if c.wgrad:
                wscr.append(b.new('wscratch%d' % r, WSCR, output=False))
                gw, gb = b.new('gw%d' % r, C * KK), (b.new('gbias%d' % r, 1) if c.gbias else None)
                R._call(tags, 'sums', 'gpode_dec10_bn_bwd_sums_wgrad', *head(sl), p(sums), p(gw), p(gb), nr, p(scr[r]), p(wscr[r]), st)
                parts['gw'].append(gw)
                late.append(gw)
                if gb is not None:
                    parts['gbias'].append(gb)
                    late.append(gb)
            else:
                R._call(tags, 'sums', 'gpode_dec10_bn_bwd_sums', *head(sl), p(sums), nr, p(scr[r]), st)
            if sums is not None:
                parts['sums'].append(sums)
        if apply:
            gathered = torch.stack(parts['sums']) if c.shards else None
            count_all = float(HW * c.B)
            for r, (sl, nr) in enumerate(R._slices(sh)):
                wts = torch.tensor([q / nr for q in sh], dtype=torch.float32, device='cuda') if c.shards else None
                gc, gg, gbt = b.new('gc%d' % r, nr * C * HW, guard=SLACK), b.new('ggamma%d' % r, C), b.new('gbeta%d' % r, C)
                cs = b.new('gc_chansum%d' % r, C) if c.chansum else None
                R._call(tags, 'apply', 'gpode_dec10_bn_bwd_apply', *head(sl), p(gathered), p(wts), len(sh) if c.shards else 0,
                        count_all if c.shards else 0.0, p(gc), p(gg), p(gbt), p(cs), nr, p(scr[r]), st)
                for k, v in zip(('gc', 'ggamma', 'gbeta', 'gc_chansum'), (gc, gg, gbt, cs)):
                    if v is not None:
                        parts[k].append(v)
                if cs is not None:
                    late.append(cs)
        if deferred:
            lib.gpode_defer_reductions(0)
            torch.cuda.synchronize()
            if not all(bool(torch.isnan(t).all()) for t in late):
                notes.append('a deferred reduction ran before the flush')
            if lib.gpode_flush_reductions(st) != 0:
                raise R.Refused(lib.gpode_last_error().decode())
    finally:
        if deferred:
            lib.gpode_defer_reductions(2)           # drop whatever an error left behind ...
            lib.gpode_defer_reductions(0)           # ... and leave recording mode
    problems = b.problems() + notes
    half, wpart = MAX_WG * C * 2, MAX_WG * C * KK
    extents = [dict(part=_prefix(s[:half]), part_gx=_prefix(s[half:])) for s in scr]
    for e, s in zip(extents, wscr):
        e.update(part_w=_prefix(s[:wpart]), part_b=_prefix(s[wpart:]))
    out = {k: (torch.cat(v) if k == 'gc' else torch.stack(v)) for k, v in parts.items()}
    return out, tags, extents, problems


def launch(c, only=None, apply=True, deferred=False):
    """Case c TWICE (only: gy zero except in that image; apply=False: the sums pass alone; deferred: between gpode_defer_reductions(1)
    and (0), then gpode_flush_reductions): the outputs of the first run on the CPU -- gc (B, 16 * 784 flat), ggamma / gbeta / gc_chansum
    (W, 16), sums (W, 32), gw (W, 400), gbias (W, 1) -- the tags, the extents written in the scratches and what the checks found"""
    d = device_inputs(c, only)
    (out, tags, ext, problems), (out2, tags2, ext2, problems2) = _once(c, d, apply, deferred), _once(c, d, apply, deferred)
    differs = [k for k in out if not torch.equal(out[k], out2[k])]
    return dict(out={k: v.cpu() for k, v in out.items()}, tags=tags, extents=ext,
                problems=problems + problems2 + ['the second run differs in %s' % k for k in differs]
                + ([] if tags == tags2 and ext == ext2 else ['the second run took %s %s' % (tags2, ext2)]))


# ---- comparison --------------------------------------------------------------------------------------------------------------------
def expected_tags(c, apply=True):
    t = dict(sums=TAG_WGRAD if c.wgrad else TAG_SUMS)
    if apply:
        t['apply'] = TAG_APPLY
    return t


def expected_extents(c, n, apply=True):
    """floats written per scratch region and shard: part[nwg][16][2] by the sums pass, part_gx[nwg][16][2] by the apply pass when it is
    given gc_chansum, part_w[nwg][400] and part_b[nwg] by the _wgrad form (part_b only with gbias) -- and nothing else"""
    out = []
    for nr in c.shards or (c.B,):
        nwg = expected(nr, n)[1]
        e = dict(part=nwg * 2 * C, part_gx=nwg * 2 * C if apply and c.chansum else 0)
        if c.wgrad:
            e.update(part_w=nwg * C * KK, part_b=nwg if c.gbias else 0)
        out.append(e)
    return out


def check(c, got, n, maxima=None, only=None, apply=True):
    """got (launch()) against the tags, the scratch extents the dispatch implies on n CUs and the fp64 reference; prints every figure
    before it asserts"""
    print('%s%s %s' % (case_id(c), '' if only is None else ' only image %d' % only, got['tags']))
    assert got['tags'] == expected_tags(c, apply), (case_id(c), got['tags'])
    assert not got['problems'], (case_id(c), got['problems'])
    assert got['extents'] == expected_extents(c, n, apply), (case_id(c), got['extents'], expected_extents(c, n, apply))
    ref, out = reference(c, only), got['out']
    sh = (c.shards or (c.B,)) if only is None else (1,)
    errs, bad = {}, []

    def cmp(name, a, r, tol, group):
        e = errs[name] = R.relerr(a, r)
        if maxima is not None:
            maxima[group] = max(maxima.get(group, 0.0), e)
        if not e < tol:
            bad.append((name, e, tol))

    form = ('wgrad' if c.wgrad else 'plain') + (' gathered' if c.shards else '') + (' one image' if only is not None else '')
    for r, (sl, nr) in enumerate(R._slices(sh)):
        s = '[%d]' % r if c.shards else ''
        if only is None and apply:
            cmp('gc' + s, out['gc'].reshape(c.B, -1)[sl], ref['gc'][sl], TOL, 'gc (%s)' % form)
            cmp('ggamma' + s, out['ggamma'][r], ref['ggamma'][r], TOL, 'ggamma, gbeta (%s)' % form)
            cmp('gbeta' + s, out['gbeta'][r], ref['gbeta'][r], TOL, 'ggamma, gbeta (%s)' % form)
        if c.sums:
            cmp('sums' + s, out['sums'][r], ref['sums'][r], TOL, 'sums (%s)' % form)
        if c.wgrad:
            cmp('gw' + s, out['gw'][r], ref['gw'][r], TOL_W, 'gw (%s)' % form)
        if c.gbias:
            cmp('gbias' + s, out['gbias'][r], ref['gbias'][r], TOL_W, 'gbias (%s)' % form)
        if only is None and apply and c.chansum:
            # gc sums to ZERO over a channel of the whole batch, so the fp64 channel sums are no yardstick: the kernel's sum against the
            # fp64 sum of the kernel's own gc (itself held to the reference), within the worst case of its fixed-order summation
            own = out['gc'].reshape(c.B, C, HW)[sl].double().sum((0, 2))
            bound = 2.0 ** -24 * chansum_terms(nr, n) * ref['gc_abs_sums'][r]
            e = errs['gc_chansum%s / bound' % s] = float(((out['gc_chansum'][r].double() - own).abs() / bound).max())
            if maxima is not None:
                maxima['gc_chansum / bound'] = max(maxima.get('gc_chansum / bound', 0.0), e)
            if not e <= 1.0:
                bad.append(('gc_chansum' + s, e, 1.0))
    print('  ' + ', '.join('%s %.1e' % kv for kv in errs.items()))
    assert not bad, (case_id(c), bad)


def same_bits(a, b, keys):
    """the keys of two launch() records whose outputs differ"""
    return [k for k in keys if not torch.equal(a['out'][k], b['out'][k])]
