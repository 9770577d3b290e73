"""Every route of the tail of the training step -- the dense layers, the elementwise kernels, the fused loss stage, the ELBO glue
(csrc/vae_dense.hip, csrc/vae_loss.hip), k_svgp_kl (csrc/gp_misc.hip), Adam and the gradient gather (csrc/vae_optim.hip) -- shared by test_gpu_loss_routes.py and
test_loss_routes_host.py.

A case is a named tuple of one of the families below; case_id(c) names it.

  Lin    op (fwd, relu_fwd, bwd, relu_bwd), B, In, Out, bias given, which of gx / gw / gb is NULL, scratch given
  Ew     op (act_fwd0/1, act_bwd0/1, loglik_fwd/_bwd, rowsum_fwd/_bwd, sll_bwd), n, copies of X, inner (row length)
  Sll    gpode_sigmoid_loglik_fwd: rows, inner, nX, nsplit (0: the proposed one), form of X, which operand is off 16 bytes
  Glue   op (reparam, reparam_kl, normal_kl), N, q, packed halves (ld = 2q), which seed gradient of reparam_kl_bwd is NULL
  Elbo   gpode_elbo_fwd / _bwd: nl, nk
  EA     entry (svgp: gpode_svgp_kl_fwd/_bwd, all: gpode_elbo_all_fwd/_bwd, all_ll: .._fwd/_bwd_ll, all_kl: .._fwd_kl/_bwd_ll_kl), M, Do,
         form of Us (tril, qdiag), diagonal scale s, nl_values, ns (slices per row), N, q, hv given, nks, nkv, seed gradients given
  Adam   tensor sizes, device-side step counter

expected(c) restates the dispatch from the thresholds in the sources and never asks the library.  launch(c) drives the C ABI on
buffers it owns -- every output and every scratch NaN-filled and sized exactly, GUARD floats of GUARD_VALUE behind each -- TWICE, reads
gpode_last_launch() after every call and returns the outputs of the first run, the tags, what the buffer checks found, which claims of
bit-equality failed and what differs in the second run.  reference(c) is the plain torch expression of the operation in fp64 on the same
fp32 inputs, gradients by autograd; per output it gives (reference, bound, scale, step): the error is max |got - ref| / scale, scale =
the largest |ref| unless a sum can cancel, where it is the fp64 sum of the absolute values of the terms.

Inputs (seeded per case, cached): logits uniform in [-8, 8], so that 1 - sigmoid(a) >= 3e-4 in fp32; X uniform in [0, 1] ('unit') or
(x - 0.1307) / 0.3081 ('norm', mixed signs); (mu, logvar) = (randn, 0.7 randn - 1) as test_elbo_glue_ops draws them; Us with a diagonal
in [0.5, 1.5] s and off-diagonals 0.01 s randn ('tril') or exactly 0 ('qdiag'); pre-activations of the ReLU layers at least 1e-3 from 0 (stricter than, so implying, the 1e-4 of MIN_PRE that the reference and the host suite assert).
The kernels that take z = sigmoid(a) as an INPUT get the fp32 z and the reference starts from the same fp32 z (1 - z is exact in both),
so no single term is ill-conditioned; gpode_sigmoid_loglik_fwd, which forms z itself, is held to its row sums relative to sum |terms|."""
import collections
import ctypes
import functools
import math
import zlib

import torch
import torch.nn.functional as F

from conv_dispatch import GUARD

GUARD_VALUE = -12345.0
TOL, TOL_Z, TOL_KL, TOL_ADAM = 2e-5, 1e-6, 1e-5, 1e-6     # test_gpu_vae_layers.TOL; test_elbo_glue_ops; test_hip_adam_matches_torch_adam
A_MAX, MIN_1MZ, MIN_PRE = 8.0, 3e-4, 1e-4
NOBS = 360.0
ELBO_PARTS = 256                                            # kElboParts: the scratch tail of `out`
SEED_VALUES = (1.3, -0.7, 0.45, 2.1)                        # g0 .. g3 where given
LR, BETA1, BETA2, EPS = 1e-2, 0.9, 0.999, 1e-8

Lin = collections.namedtuple('Lin', 'op B In Out bias null scratch')
Ew = collections.namedtuple('Ew', 'op n reps inner')
Sll = collections.namedtuple('Sll', 'rows inner nX nsplit xform mis')
Glue = collections.namedtuple('Glue', 'op N q packed null')
Elbo = collections.namedtuple('Elbo', 'nl nk')
EA = collections.namedtuple('EA', 'entry M Do form s nl_values ns N q hv nks nkv seeds')
Adam = collections.namedtuple('Adam', 'sizes dev')


class Refused(Exception):
    pass


def case_id(c):
    return type(c).__name__ + '-' + '-'.join(('x'.join(map(str, v)) if isinstance(v, tuple) and len(v) < 5 else
                                              ('%dt%d' % (len(v), sum(v)) if isinstance(v, tuple) else str(v))) or 'none' for v in c)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _uniq(cases):
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


# ---- the dispatch, restated ----------------------------------------------------------------------------------------------------------
def linear_fwd_tag(B, In, Out):
    if In <= 16 and Out % 64 == 0 and B >= 256:
        return 'linear_fwd_fanout'
    if In >= 128 and B * Out <= 2 ** 22:
        return 'linear_fwd_fanin'
    return 'linear_fwd'


def linear_bwd_tag(B, In, Out, scratch, gw=True):
    if In <= 16 and Out % 64 == 0 and Out <= 512 and B >= 256:
        return 'linear_bwd_fanout' + (' (row slabs)' if scratch and gw and In <= 8 and B >= 1024 else '')
    return 'linear_bwd'


def linear_bwd_scratch(B, In, Out):
    """LINW_SLABS = 32 slabs of (Out, In) weight and (Out) bias partials"""
    return 32 * Out * (In + 1)


def linear_refused(op, B, In, Out):
    """the words gpode_last_error() must hold for a refused linear_relu_* call, or None"""
    if op == 'relu_fwd' and (In < 128 or B * Out > 2 ** 22):
        return 'gpode_linear_relu_fwd: built for wide fan-in layers'
    if op == 'relu_bwd' and In < 128:
        return 'gpode_linear_relu_bwd: built for wide fan-in layers'
    return None


def sigmoid_loglik_splits(rows, inner):
    if rows == 0 or inner == 0:
        return 1
    return max(1, min(-(-1024 // rows), -(-inner // 1024), 64))


def sll_chunk(c):
    ns = c.nsplit or sigmoid_loglik_splits(c.rows, c.inner)
    return (-(-c.inner // ns) + 3) // 4 * 4


def sll_vector_path(c):
    """float4 loads iff rows, wraps of X and slices start on 16-byte boundaries and X, a, z are aligned"""
    return c.inner % 4 == 0 and c.nX % 4 == 0 and sll_chunk(c) % 4 == 0 and not c.mis


def sll_refused(c):
    if c.nsplit < 0 or c.rows > 65535:
        return 'nsplit >= 1, rows <= 65535'
    if (c.rows * c.inner) % c.nX:
        return 'X must tile the rows'
    return None


def us_in_parts(M, Do):
    return M * (M + 1) // 2 * Do > 2 ** 16


def ew_grid(n):
    return min(max(-(-n // 256), 1), 8192)


def adam_grid(total, dev):
    return min(ew_grid(total), 2048) if dev else ew_grid(total)


EW_TAGS = dict(act_fwd0='act_fwd', act_fwd1='act_fwd', act_bwd0='act_bwd', act_bwd1='act_bwd', loglik_fwd='loglik_fwd',
               loglik_bwd='loglik_bwd', rowsum_fwd='loglik_rowsum', rowsum_bwd='loglik_rowsum_bwd')


def expected(c):
    """{step: tag} of the calls launch() makes for case c"""
    if isinstance(c, Lin):
        if c.op == 'fwd':
            return dict(fwd=linear_fwd_tag(c.B, c.In, c.Out))
        if c.op == 'bwd':
            return dict(bwd=linear_bwd_tag(c.B, c.In, c.Out, c.scratch, c.null != 'gw'))
        return {c.op[5:]: 'linear_' + c.op}
    if isinstance(c, Ew):
        if c.op == 'sll_bwd':
            return dict(sll_bwd='sigmoid_loglik_bwd', rowsum_bwd='loglik_rowsum_bwd', act_bwd='act_bwd')
        return {c.op: EW_TAGS[c.op]}
    if isinstance(c, Sll):
        return dict(fwd='sigmoid_loglik_fwd', act='act_fwd')
    if isinstance(c, Glue):
        if c.op == 'reparam':
            return dict(fwd='reparam_fwd', bwd='reparam_bwd')
        if c.op == 'reparam_kl':
            return dict(fwd='reparam_kl_fwd', bwd='reparam_kl_bwd', plain='reparam_fwd')
        return dict(fwd='normal_kl_fwd', bwd='normal_kl_bwd')
    if isinstance(c, Elbo):
        return dict(fwd='elbo_fwd', bwd='elbo_bwd')
    if isinstance(c, EA):
        parts = ' (Us in parts)' if us_in_parts(c.M, c.Do) else ''
        if c.entry == 'svgp':
            return dict(fwd='svgp_kl', bwd='svgp_kl_bwd')
        if c.entry == 'all':
            return dict(fwd='elbo_all_fwd' + parts, bwd='elbo_all_bwd')
        if c.entry == 'all_ll':
            return dict(fwd='elbo_all_fwd' + parts, bwd='elbo_loglik_bwd', sll_bwd='sigmoid_loglik_bwd')
        return dict(fwd='elbo_all_fwd_kl' + parts, bwd='elbo_loglik_bwd_kl', sll_bwd='sigmoid_loglik_bwd')
    assert isinstance(c, Adam), c
    return dict(adam='adam_multi', gather='gather_multi')


REQUIRED_TAGS = ('act_fwd', 'act_bwd', 'linear_fwd', 'linear_fwd_fanout', 'linear_fwd_fanin', 'linear_bwd', 'linear_bwd_fanout',
                 'linear_bwd_fanout (row slabs)', 'linear_relu_fwd', 'linear_relu_bwd', 'loglik_fwd', 'loglik_bwd', 'loglik_rowsum',
                 'loglik_rowsum_bwd', 'sigmoid_loglik_fwd', 'sigmoid_loglik_bwd', 'elbo_all_fwd', 'elbo_all_fwd (Us in parts)',
                 'elbo_all_fwd_kl', 'elbo_all_fwd_kl (Us in parts)', 'elbo_all_bwd', 'elbo_loglik_bwd', 'elbo_loglik_bwd_kl',
                 'reparam_fwd', 'reparam_bwd', 'reparam_kl_fwd', 'reparam_kl_bwd', 'normal_kl_fwd', 'normal_kl_bwd', 'elbo_fwd', 'elbo_bwd',
                 'svgp_kl', 'svgp_kl_bwd', 'adam_multi', 'gather_multi')


# ---- the case tables -----------------------------------------------------------------------------------------------------------------
LIN_B = (1, 255, 256, 257, 263, 264)
LIN_IN = (1, 6, 8, 16, 17, 127, 128, 129, 191, 512, 513)
LIN_OUT = (1, 7, 63, 64, 65, 192, 256, 320, 512, 576, 1024)


def linear_fwd_cases():
    out = []

    def add(B, In, Out, bias=None):
        out.append(Lin('fwd', B, In, Out, (B + In + Out) % 2 == 0 if bias is None else bias, '', False))
    for B in LIN_B:                                   # the 8-row blocks of the fan-out kernel, ragged and full, on both sides of In = 16
        for In in (1, 16, 17):
            for Out in (64, 65, 320):
                add(B, In, Out)
    for In in LIN_IN:                                 # lanes stride the reduction by 64 on the fan-in route; B Out = 21 is no multiple of 4
        for B, Out in ((3, 7), (257, 64), (256, 576), (5, 1)):
            add(B, In, Out)
    for Out in LIN_OUT:
        for B, In in ((257, 16), (2, 128), (256, 1)):
            add(B, In, Out)
    for bias in (False, True):                        # each route with and without a bias
        for B, In, Out in ((256, 16, 64), (3, 128, 7), (255, 16, 64)):
            add(B, In, Out, bias)
    add(4096, 128, 1024, True)                        # B Out = 2^22: the last fan-in shape ...
    add(4097, 128, 1024, True)                        # ... and the first generic one
    return _uniq(out)


def linear_relu_fwd_cases():
    return [Lin('relu_fwd', B, In, Out, bias, '', False) for In in (128, 129, 512) for B, Out, bias in ((3, 7, True), (64, 12, False))]


def linear_refusals():
    return [Lin('relu_fwd', 3, 127, 7, True, '', False), Lin('relu_fwd', 4097, 128, 1024, True, '', False),
            Lin('relu_bwd', 3, 127, 7, True, '', False)]


def linear_bwd_cases():
    out = []
    for Out in range(64, 513, 64):                    # the eight instantiations of k_linear_bwd_x_fanout, on both weight-gradient routes
        out.append(Lin('bwd', 256, 16, Out, True, '', True))
        out.append(Lin('bwd', 1027, 8, Out, True, '', True))
    out.append(Lin('bwd', 256, 16, 576, True, '', True))
    out.append(Lin('bwd', 1027, 8, 576, True, '', True))
    for In in (1, 8, 9, 16, 17):
        for B in (255, 256, 1023, 1024, 1025, 1027, 2051):
            out.append(Lin('bwd', B, In, 192 if B % 2 else 64, True, '', True))
    for In in (8, 9):                                 # scratch NULL and given on both sides of the slab route's thresholds
        for B in (1023, 1024):
            for scratch in (False, True):
                out.append(Lin('bwd', B, In, 128, True, '', scratch))
    for null in ('gx', 'gw', 'gb'):
        for B, In, Out, scratch in ((1024, 8, 128, True), (1024, 8, 128, False), (300, 16, 64, True), (255, 17, 65, False)):
            out.append(Lin('bwd', B, In, Out, True, null, scratch))
    return _uniq(out)


def linear_relu_bwd_cases():
    return ([Lin('relu_bwd', B, In, Out, True, '', False) for In in (128, 129, 512) for B, Out in ((3, 7), (64, 12))] +
            [Lin('relu_bwd', 5, 128, 9, True, null, False) for null in ('gx', 'gw', 'gb')])


EW_N = (1, 255, 256, 257, 2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1, 2 ** 21 + 2 ** 20 + 3)
EW_INNER = (1, 255, 256, 257, 784, 3136)
EW_OPS = ('act_fwd0', 'act_fwd1', 'act_bwd0', 'act_bwd1', 'loglik_fwd', 'loglik_bwd', 'rowsum_bwd', 'sll_bwd')


def _smallest_factor(n):
    return next((p for p in range(2, 4000) if n % p == 0), 1) if n > 3 else 1


def ew_reps(n):
    """copies of X: three where n divides by 3, else two where it is even, else one"""
    return 3 if n % 3 == 0 else (2 if n % 2 == 0 else 1)


def elementwise_cases():
    out = []
    for n in EW_N:
        for op in EW_OPS:
            out.append(Ew(op, n, ew_reps(n), n // _smallest_factor(n)))
    for inner in EW_INNER:                            # row sums: 3 rows, X broadcast over them (reps 3) or not (reps 1)
        for op in ('rowsum_fwd', 'rowsum_bwd', 'sll_bwd'):
            out.append(Ew(op, 3 * inner, 3 if inner % 2 else 1, inner))
    out.append(Ew('rowsum_fwd', 2 * 3136, 2, 3136))
    return _uniq(out)


SLL_ROWS = (1, 3, 16, 1024, 1025)
SLL_INNER = (4, 8, 1023, 1024, 1028, 3136, 12544)


def sll_cases():
    out = []
    for rows in SLL_ROWS:
        for inner in SLL_INNER + (65536,):            # 65536 / 1024 = 64: the cap of the proposal (rows <= 16)
            if rows * inner > 2 ** 22:
                continue
            for xform in ('unit', 'norm'):
                out.append(Sll(rows, inner, inner if rows % 2 else rows * inner, 0, xform, ''))
    for mis in ('a', 'z', 'X'):                       # an operand one float off a 16-byte boundary: the scalar path
        for rows, inner in ((3, 8), (16, 3136), (3, 12544)):
            out.append(Sll(rows, inner, inner, 0, 'norm', mis))
    out.append(Sll(3, 4, 6, 0, 'norm', ''))           # nX % 4 != 0 with inner % 4 == 0
    out.append(Sll(6, 1028, 3 * 1028 // 2, 0, 'unit', ''))
    for mis in ('', 'a'):                             # more slices than the row has chunks: the trailing parts are 0, not unwritten
        out.append(Sll(3, 8, 8, 5, 'norm', mis))
        out.append(Sll(16, 3136, 3136, 7, 'unit', mis))
        out.append(Sll(1, 1028, 1028, 64, 'norm', mis))
    return _uniq(out)


def sll_refusals():
    return [Sll(65536, 4, 4, 1, 'unit', ''), Sll(3, 8, 5, 1, 'unit', ''), Sll(3, 8, 8, -1, 'unit', '')]     # nsplit -1 stands for 0


def glue_cases():
    out = []
    for q, Ns in ((1, (1, 255, 256, 257, 513)), (6, (1, 42, 43, 86)), (16, (1, 16, 17, 33))):
        for N in Ns:
            for packed in (False, True):
                out.append(Glue('reparam', N, q, packed, ''))
                out.append(Glue('normal_kl', N, q, packed, ''))
                for null in ('', 'gz', 'gkl'):
                    out.append(Glue('reparam_kl', N, q, packed, null))
    return _uniq(out)


def elbo_cases():
    ns = (1, 255, 256, 257, 1000)
    return _uniq([Elbo(n, n) for n in ns] + [Elbo(1, 1000), Elbo(1000, 1), Elbo(255, 257), Elbo(257, 255), Elbo(256, 1)])


EA_SHAPES = ((1, 1), (7, 3), (100, 6), (147, 6), (148, 6), (2047, 1))
EA_NL = (1, 1023, 1024, 7168, 7169, 8193, 20000)
EA_SEEDS = ('0', '0123', '2', '13')


def ea(entry, M=7, Do=3, form='tril', s=1.0, nl_values=12, ns=1, N=3, q=6, hv=False, nks=0, nkv=0, seeds='0123'):
    if entry == 'svgp':
        return EA(entry, M, Do, form, s, 0, 0, 0, 0, False, 0, 0, '')
    if entry == 'all_kl':
        return EA(entry, M, Do, form, s, nl_values, ns, N, 0, False, nks or 1, nkv, seeds)
    return EA(entry, M, Do, form, s, nl_values, ns, N, q, hv, 0, 0, seeds)


def elbo_all_cases():
    out = []
    for M, Do in EA_SHAPES:
        for s in (1e-3, 1.0):
            out.append(ea('svgp', M, Do, s=s))
    out.append(ea('svgp', 100, 6, 'qdiag'))
    k = 0
    for entry in ('all', 'all_ll', 'all_kl'):
        for M, Do in EA_SHAPES:                       # both sides of 2^16 packed entries, and 8k + 1 next to 2^24
            k += 1
            out.append(ea(entry, M, Do, s=(1e-3, 1.0)[k % 2], hv=bool(k % 2), nks=(1, 2, 8)[k % 3], nkv=(0, 2)[k % 2], seeds=EA_SEEDS[k % 4]))
        out.append(ea(entry, 100, 6, 'qdiag', nks=2, nkv=1))
        for nl in EA_NL:                              # the 8-way unrolled loop of strided() and its tail
            for ns in (1, 4):
                if nl % ns == 0:
                    k += 1
                    out.append(ea(entry, nl_values=nl, ns=ns, hv=bool(k % 2), nks=(1, 2, 8)[k % 3], nkv=(0, 3)[k % 2], seeds=EA_SEEDS[k % 4]))
        for seeds in EA_SEEDS:
            for hv in (False, True):
                out.append(ea(entry, 7, 3, nl_values=40, ns=4, hv=hv, nks=8, nkv=2 if hv else 0, seeds=seeds))
        out.append(ea(entry, N=400, q=16, hv=True, nks=8200, nkv=7169))      # N q (or the KL partials) the largest of the extents
        out.append(ea(entry, N=1, q=1))
    return _uniq(out)


def adam_sizes(total):
    """tensor sizes adding up to `total`: boundaries on a 256-element block boundary and beside one, an empty tensor in the middle"""
    if total <= 2:
        return (total,)
    if total == 256:
        return (255, 0, 1)
    head = [s for s in (1, 255, 256, 0, 257, 255, 1, 513)]
    sizes = []
    for s in head:
        if sum(sizes) + s < total:
            sizes.append(s)
    if 0 not in sizes:
        sizes.insert(1, 0)
    return tuple(sizes) + (total - sum(sizes),)


ADAM_TOTALS = (1, 256, 257, 2048 * 256, 2048 * 256 + 1, 8192 * 256 + 1)


def adam_cases():
    out = [Adam(adam_sizes(t), dev) for t in ADAM_TOTALS for dev in (False, True)]
    out += [Adam((2048 * 256 + 1,), True), Adam((300,), False)]          # one tensor
    return _uniq(out)


def all_cases():
    return (linear_fwd_cases() + linear_relu_fwd_cases() + linear_bwd_cases() + linear_relu_bwd_cases() + elementwise_cases() + sll_cases() +
            glue_cases() + elbo_cases() + elbo_all_cases() + adam_cases())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _x_form(shape, xform, g):
    x = torch.rand(shape, generator=g)
    return (x - 0.1307) / 0.3081 if xform == 'norm' else x


def _logits(shape, g):
    return (torch.rand(shape, generator=g) * 2 - 1) * A_MAX


@functools.lru_cache(maxsize=4)
def _lin_inputs(B, In, Out, relu, bwd):
    g = _gen('lin', B, In, Out, relu)
    x = torch.randn(B, In, generator=g)
    if relu:                                          # no pre-activation within 1e-3 of zero: the mask is no coin-flip
        x = torch.where(x.abs() < 1e-3, torch.where(x < 0, -1e-3, 1e-3).to(x), x)
    d = dict(x=x, w=torch.randn(Out, In, generator=g) / math.sqrt(In), b=torch.randn(Out, generator=g))
    if bwd:
        d['gy'] = torch.randn(B, Out, generator=g)
    return d


@functools.lru_cache(maxsize=4)
def _ew_inputs(n, reps, inner):
    g = _gen('ew', n, reps, inner)
    a = _logits(n, g)
    return dict(a=a, z=torch.sigmoid(a), y0=F.relu(a), X=_x_form(n // reps, 'norm' if reps == 2 else 'unit', g), g=torch.randn(n, generator=g),
                grow=torch.randn(n // inner, generator=g))


@functools.lru_cache(maxsize=4)
def _sll_inputs(rows, inner, nX, xform):
    g = _gen('sll', rows, inner, nX, xform)
    return dict(a=_logits(rows * inner, g), X=_x_form(nX, xform, g))


@functools.lru_cache(maxsize=4)
def _glue_inputs(N, q):
    g = _gen('glue', N, q)
    nb = -(-N * q // 256)
    return dict(mu=torch.randn(N, q, generator=g), logvar=torch.randn(N, q, generator=g) * 0.7 - 1.0, eps=torch.randn(N, q, generator=g),
                gz=torch.randn(N, q, generator=g), gkl=torch.randn(nb, generator=g) + 2.0 * torch.arange(nb), grow=torch.randn(N, generator=g))


@functools.lru_cache(maxsize=4)
def _elbo_inputs(nl, nk):
    g = _gen('elbo', nl, nk)
    return dict(lhood=-torch.rand(nl, generator=g) * 500 - 100, klrow=torch.rand(nk, generator=g) * 20, klu=torch.tensor([12.5]),
                gout=torch.tensor(SEED_VALUES))


def us_packed(M, Do, form, s, g):
    """(Do, M(M+1)/2): diagonal in [0.5, 1.5] s, off-diagonals 0.01 s randn ('tril') or exactly 0 ('qdiag')"""
    P = M * (M + 1) // 2
    us = torch.zeros(Do, P) if form == 'qdiag' else 0.01 * s * torch.randn(Do, P, generator=g)
    us[:, diag_index(M)] = (0.5 + torch.rand(Do, M, generator=g)) * s
    return us


def diag_index(M):
    m = torch.arange(M)
    return m * (m + 1) // 2 + m


EA_INNER = 8                                          # logits per likelihood row of the all_ll / all_kl cases


@functools.lru_cache(maxsize=4)
def _ea_inputs(c):
    g = _gen('ea', *c)
    d = dict(Um=0.5 * torch.randn(c.M, c.Do, generator=g), Us=us_packed(c.M, c.Do, c.form, c.s, g))
    if c.entry == 'svgp':
        d['g'] = torch.tensor([SEED_VALUES[3]])
        return d
    rows = c.nl_values // c.ns
    d['lpart'] = (-torch.rand(rows, c.ns, generator=g) * 500 - 100) / c.ns
    if c.entry == 'all_kl':
        d['kls'] = torch.rand(c.nks, generator=g) * 50
        if c.nkv:
            d['klv'] = torch.rand(c.nkv, generator=g) * 50
    else:
        d['hs'] = torch.cat((torch.randn(c.N, c.q, generator=g), torch.randn(c.N, c.q, generator=g) * 0.7 - 1.0), 1)
        if c.hv:
            d['hv'] = torch.cat((torch.randn(c.N, c.q, generator=g), torch.randn(c.N, c.q, generator=g) * 0.7 - 1.0), 1)
    if c.entry != 'all':
        reps = 2 if rows % 2 == 0 else 1
        d['X'] = _x_form(rows * EA_INNER // reps, 'norm' if c.M % 2 else 'unit', g)
        d['z'] = torch.sigmoid(_logits(rows * EA_INNER, g))
    for i in range(4):
        if str(i) in c.seeds:
            d['g%d' % i] = torch.tensor([SEED_VALUES[i]])
    return d


ADAM_STEPS = 3


@functools.lru_cache(maxsize=4)
def _adam_inputs(sizes):
    g = _gen('adam', sizes)
    total = sum(sizes)
    # 0.4 <= |p| < 0.9 with lr = 1e-2 balances the two bounds: half an ulp of the stored parameter (3e-8 under 1) is 7 % of the bound on the
    # update at t = 3 (4.1e-7), and the rounding of 1 - powf(beta2, t) (at most 7.5e-6 of an update of lr) is under 19 % of 1e-6 max |p|
    # even where the table holds ONE parameter
    sign = torch.where(torch.rand(total, generator=g) < 0.5, -1.0, 1.0)
    return dict(p=sign * (0.4 + 0.5 * torch.rand(total, generator=g)), grads=[torch.randn(total, generator=g) * 10.0 ** (t - 1) for t in range(ADAM_STEPS)])


def inputs(c):
    """fp32 inputs of case c on the CPU"""
    if isinstance(c, Lin):
        return _lin_inputs(c.B, c.In, c.Out, c.op.startswith('relu'), c.op.endswith('bwd'))
    if isinstance(c, Ew):
        return _ew_inputs(c.n, c.reps, c.inner)
    if isinstance(c, Sll):
        return _sll_inputs(c.rows, c.inner, c.nX, c.xform)
    if isinstance(c, Glue):
        return _glue_inputs(c.N, c.q)
    if isinstance(c, Elbo):
        return _elbo_inputs(c.nl, c.nk)
    if isinstance(c, EA):
        return _ea_inputs(c)
    return _adam_inputs(c.sizes)


# ---- fp64 references -------------------------------------------------------------------------------------------------------------------
def bernoulli_terms(X, z):
    """vae.py:136-153 (no epsilon)"""
    return torch.log(z) * X + torch.log(1 - z) * (1 - X)


def normal_kl(mu, logvar):
    from torch.distributions import Normal, kl_divergence
    return kl_divergence(Normal(mu, torch.exp(0.5 * logvar)), Normal(torch.zeros_like(mu), torch.ones_like(mu)))


def svgp_kl_terms_abs(Um, Us, M):
    """sum of the absolute values of the terms of oracle.svgp_kl: the scale a cancelling kl_u is compared on"""
    d = Us[:, diag_index(M)]
    return 0.5 * ((Us * Us).sum() + (Um * Um).sum() + torch.log(d * d).abs().sum() + M * Um.shape[1])


def elbo_algebra(lhood_mean, kl_mean, kl_u, nobs=NOBS):
    """create_model.py:61-73"""
    return torch.stack([-(lhood_mean * nobs - kl_mean * nobs - kl_u), -lhood_mean, kl_mean, kl_u])


def adam_reference(p, grads, dtype=torch.float64):
    """the textbook update on the fp32-rounded hyper-parameters; -> per step (p, m, v, update)"""
    lr, b1, b2, eps = (float(torch.tensor(v, dtype=torch.float32)) for v in (LR, BETA1, BETA2, EPS))
    p, m, v = p.to(dtype), torch.zeros_like(p, dtype=dtype), torch.zeros_like(p, dtype=dtype)
    out = []
    for t, g in enumerate(grads, 1):
        g = g.to(dtype)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        bc1, bc2 = ((1 - torch.tensor(b, dtype=dtype) ** t) for b in (b1, b2))      # in fp32 this is the kernel's 1 - powf(beta, t)
        upd = -lr * (m / bc1) / ((v / bc2).sqrt() + eps)
        p = p + upd
        out.append((p.clone(), m.clone(), v.clone(), upd.clone()))
    return out


def adam_update_bound(t):
    """the rounding of 1 - powf(beta, t) in fp32 and of the eight operations of the update, relative to lr"""
    lr, b1, b2 = (float(torch.tensor(v, dtype=torch.float32)) for v in (LR, BETA1, BETA2))
    return lr * 2.0 ** -23 * (1 / (1 - b1 ** t) + 1 / (1 - b2 ** t) + 8)


def _ref_lin(c, dt):
    d = inputs(c)
    x, w, b = (d[k].to(dt) for k in ('x', 'w', 'b'))
    relu = c.op.startswith('relu')
    x.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
    y = F.linear(F.relu(x) if relu else x, w, b if (c.bias or c.op.endswith('bwd')) else None)
    step = c.op[5:] if relu else c.op
    if c.op.endswith('fwd'):
        return dict(y=(y.detach(), TOL, None, step))
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), d['gy'].to(dt))
    if relu:
        assert x.detach().abs().min() >= MIN_PRE
    return {k: (v, TOL, None, step) for k, v in (('gx', gx), ('gw', gw), ('gb', gb)) if k != c.null}


def _ref_ew(c, dt):
    d = inputs(c)
    a, z, X, g, grow = (d[k].to(dt) for k in ('a', 'z', 'X', 'g', 'grow'))
    Xr = X.repeat(c.reps)
    rows = c.n // c.inner
    if c.op == 'act_fwd0':
        return dict(y=(F.relu(a), TOL, None, c.op))
    if c.op == 'act_fwd1':
        return dict(y=(torch.sigmoid(a), TOL, None, c.op))
    if c.op == 'act_bwd0':
        return dict(gx=(g * (a > 0), TOL, None, c.op))
    if c.op == 'act_bwd1':
        return dict(gx=(g * z * (1 - z), TOL, None, c.op))
    zl = z.clone().requires_grad_(True)
    t = bernoulli_terms(Xr, zl)
    if c.op == 'loglik_fwd':
        return dict(ll=(t.detach(), TOL, None, c.op))
    if c.op == 'loglik_bwd':
        return dict(gz=(torch.autograd.grad(t, zl, g)[0], TOL, None, c.op))
    rs = t.view(rows, c.inner).sum(1)
    if c.op == 'rowsum_fwd':
        return dict(out=(rs.detach(), TOL, t.detach().abs().view(rows, c.inner).sum(1), c.op))
    gz = torch.autograd.grad(rs, zl, grow)[0]
    if c.op == 'rowsum_bwd':
        return dict(gz=(gz, TOL, None, c.op))
    return dict(ga=(gz * z * (1 - z), TOL, None, 'sll_bwd'))


def _ref_sll(c, dt):
    d = inputs(c)
    a, X = d['a'].to(dt), d['X'].to(dt)
    z = torch.sigmoid(a)
    t = bernoulli_terms(X.repeat(c.rows * c.inner // c.nX), z).view(c.rows, c.inner)
    return dict(z=(z, TOL, None, 'fwd'), rowsum=(t.sum(1), TOL, t.abs().sum(1), 'fwd'))


SLL_SHORT = 8                                         # rows of up to 8 logits


def sll_short_rows(c, z):
    """Rows of 4 or 8 terms are single terms, and a single term from a logit near 8 is ill-conditioned in fp32: z = sigmoid(a) is within
    half an ulp (3e-8) of 1 - 3.4e-4, which is 9e-5 of 1 - z and of log(1 - z) -- 1.8e-5 of the row's sum |terms| in the fp32 evaluation of
    the reference itself (1.3e-5 at 8 terms, 7e-7 from 1023 terms on, where the errors average out).  So such rows are held to the fp64
    terms of the z the kernel returned (z itself is held to the fp64 sigmoid, and bit for bit to gpode_act_fwd): the logarithms, the
    products and the summation are checked to the same 2e-5 of sum |terms|, the conditioning of 1 - sigmoid(a) is not."""
    X = inputs(c)['X'].double()
    t = bernoulli_terms(X.repeat(c.rows * c.inner // c.nX), z.double().reshape(-1)).view(c.rows, c.inner)
    return t.sum(1), t.abs().sum(1)


def _ref_glue(c, dt):
    d = inputs(c)
    mu, lv, eps, gz, gkl, grow = (d[k].to(dt) for k in ('mu', 'logvar', 'eps', 'gz', 'gkl', 'grow'))
    mu.requires_grad_(True), lv.requires_grad_(True)
    z = mu + torch.exp(0.5 * lv) * eps
    kl = normal_kl(mu, lv)
    if c.op == 'reparam':
        gm, gl = torch.autograd.grad(z, (mu, lv), gz)
        return dict(z=(z.detach(), TOL_Z, None, 'fwd'), gmu=(gm, TOL, None, 'bwd'), glogvar=(gl, TOL, None, 'bwd'))
    if c.op == 'normal_kl':
        klr = kl.sum(1)
        gm, gl = torch.autograd.grad(klr, (mu, lv), grow)
        return dict(klrow=(klr.detach(), TOL_KL, None, 'fwd'), gmu=(gm, TOL, None, 'bwd'), glogvar=(gl, TOL, None, 'bwd'))
    J = 0
    if c.null != 'gz':
        J = J + (z * gz).sum()
    if c.null != 'gkl':                               # every term of workgroup b carries gkl[b]
        J = J + (kl.reshape(-1) * gkl[torch.arange(c.N * c.q) // 256]).sum()
    gm, gl = torch.autograd.grad(J, (mu, lv), allow_unused=True)
    gm, gl = (torch.zeros_like(mu) if v is None else v for v in (gm, gl))
    return dict(z=(z.detach(), TOL_Z, None, 'fwd'), klsum=(kl.sum().detach().reshape(1), TOL_KL, None, 'fwd'), gmu=(gm, TOL, None, 'bwd'),
                glogvar=(gl, TOL, None, 'bwd'))


def _ref_elbo(c, dt):
    d = inputs(c)
    lh, kr, ku = (d[k].to(dt).requires_grad_(True) for k in ('lhood', 'klrow', 'klu'))
    out = elbo_algebra(lh.mean(), kr.mean(), ku[0])
    gl, gk, gu = torch.autograd.grad(out, (lh, kr, ku), d['gout'].to(dt))
    scale = torch.stack([lh.detach().abs().mean() * NOBS + kr.detach().mean() * NOBS + ku.detach()[0], lh.detach().abs().mean(), kr.detach().mean(),
                         ku.detach()[0]])
    return dict(out=(out.detach(), TOL_KL, scale, 'fwd'), glhood=(gl, TOL, None, 'bwd'), gklrow=(gk, TOL, None, 'bwd'), gklu=(gu, TOL, None, 'bwd'))


def _ref_ea(c, dt):
    from oracle import gpode_oracle as O
    d = inputs(c)
    Um, Us = d['Um'].to(dt).requires_grad_(True), d['Us'].to(dt).requires_grad_(True)
    ku = O.svgp_kl(Um, Us)
    ku_abs = svgp_kl_terms_abs(Um.detach(), Us.detach(), c.M)
    di = diag_index(c.M)
    off = torch.ones(Us.shape[1], dtype=torch.bool)
    off[di] = False

    def us_grads(dUs, step):
        r = dict(dUs_diag=(dUs[:, di], TOL, None, step))
        if c.M > 1:
            r['dUs_off'] = (dUs[:, off], TOL, None, step)
        return r
    if c.entry == 'svgp':
        dUm, dUs = torch.autograd.grad(ku, (Um, Us), d['g'].to(dt)[0])
        return dict(kl=(ku.detach().reshape(1), TOL_KL, ku_abs, 'fwd'), dUm=(dUm, TOL, None, 'bwd'), **us_grads(dUs, 'bwd'))
    rows = c.nl_values // c.ns
    lrow = d['lpart'].to(dt).sum(1).requires_grad_(True)
    leaves = dict(lrow=lrow, Um=Um, Us=Us)
    if c.entry == 'all_kl':
        leaves['kls'] = d['kls'].to(dt).requires_grad_(True)
        kl_total = leaves['kls'].sum()
        if c.nkv:
            leaves['klv'] = d['klv'].to(dt).requires_grad_(True)
            kl_total = kl_total + leaves['klv'].sum()
    else:
        for k in ('hs', 'hv')[:1 + c.hv]:
            leaves[k] = d[k].to(dt).requires_grad_(True)
        kl_total = sum(normal_kl(leaves[k][:, :c.q], leaves[k][:, c.q:]).sum() for k in ('hs', 'hv')[:1 + c.hv])
    out = elbo_algebra(lrow.mean(), kl_total / c.N, ku)
    seeds = torch.tensor([SEED_VALUES[i] if str(i) in c.seeds else 0.0 for i in range(4)], dtype=dt)
    names = list(leaves)
    grads = dict(zip(names, torch.autograd.grad((out * seeds).sum(), [leaves[k] for k in names], allow_unused=True)))
    grads = {k: (torch.zeros_like(leaves[k]) if v is None else v) for k, v in grads.items()}
    lh_abs, kl_abs = lrow.detach().abs().mean(), kl_total.detach() / c.N
    scale = torch.stack([lh_abs * NOBS + kl_abs * NOBS + ku_abs, lh_abs, kl_abs, ku_abs])
    r = dict(out=(out.detach(), TOL_KL, scale, 'fwd'), glrow=(grads['lrow'], TOL, None, 'bwd'), dUm=(grads['Um'], TOL, None, 'bwd'),
             **us_grads(grads['Us'], 'bwd'))
    for k, name in (('hs', 'ghs'), ('hv', 'ghv'), ('kls', 'gkls'), ('klv', 'gklv')):
        if k in grads:
            r[name] = (grads[k], TOL, None, 'bwd')
    if c.entry != 'all':                              # the logits' gradient: autograd through sigmoid and the row sums, every row weighted alike
        X, z = d['X'].to(dt), d['z'].to(dt)
        a = torch.logit(z).requires_grad_(True)
        t = bernoulli_terms(X.repeat(z.numel() // X.numel()), torch.sigmoid(a)).view(rows, EA_INNER).sum(1)
        r['ga'] = (torch.autograd.grad(t, a, grads['lrow'])[0], TOL, None, 'bwd')
    return r


def _ref_adam(c, dt):
    d = inputs(c)
    r = {}
    for t, (p, m, v, upd) in enumerate(adam_reference(d['p'], d['grads'], dt), 1):
        r['p%d' % t], r['m%d' % t], r['v%d' % t] = (p, TOL_ADAM, None, 'adam'), (m, TOL_ADAM, None, 'adam'), (v, TOL_ADAM, None, 'adam')
        r['upd%d' % t] = (upd, adam_update_bound(t), 1.0, 'adam')
    return r


_REFS = {Lin: _ref_lin, Ew: _ref_ew, Sll: _ref_sll, Glue: _ref_glue, Elbo: _ref_elbo, EA: _ref_ea, Adam: _ref_adam}


def reference(c, dt=torch.float64):
    """{output: (reference, bound, scale or None, step that produced it)} in fp64; dt = torch.float32: the same expressions evaluated in
    fp32, which the host suite holds to a quarter of the bounds (the inputs leave the kernels that much room)"""
    return _REFS[type(c)](c, dt)


def clear_caches():
    for f in (_lin_inputs, _ew_inputs, _sll_inputs, _glue_inputs, _elbo_inputs, _ea_inputs, _adam_inputs):
        f.cache_clear()


# ---- launches ----------------------------------------------------------------------------------------------------------------------------
class Bufs:
    """device buffers with GUARD floats of GUARD_VALUE behind each; outputs and scratches NaN-filled.  problems() says which guard was
    written and which output still holds a NaN"""

    def __init__(self):
        self.guards, self.outs = {}, {}

    def new(self, name, n, init=None, dtype=torch.float32, output=True, shift=0):
        """n elements; init None: NaN-filled; output False: a scratch or an input (no NaN check); shift: floats off a 16-byte boundary"""
        buf = torch.full((shift + n + GUARD,), GUARD_VALUE, device='cuda', dtype=dtype)
        view = buf[shift:shift + n]
        if init is None:
            view.fill_(float('nan'))
        else:
            view.copy_(init.reshape(-1))
        assert name not in self.guards, name
        assert buf.data_ptr() % 16 == 0
        self.guards[name] = buf[shift + n:]
        if output and init is None:
            self.outs[name] = view
        return view

    def problems(self):
        torch.cuda.synchronize()
        bad = ['%s: the guard behind it was written' % k for k, v in self.guards.items() if bool((v != GUARD_VALUE).any())]
        return bad + ['%s: a NaN of the fill is left' % k for k, v in self.outs.items() if bool(torch.isnan(v).any())]

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(v).all()) for v in self.outs.values())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _call(tags, step, name, *args):
    """one entry point on the current stream; its tag goes to tags[step]"""
    from vae_gp_ode_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, name)(*[_ptr(a) if (a is None or torch.is_tensor(a)) else a for a in args], _stream())
    if rc != 0:
        raise Refused('%s (%d): %s' % (name, rc, lib.gpode_last_error().decode()))
    tag = lib.gpode_last_launch().decode()
    assert tags.setdefault(step, tag) == tag, (step, tags[step], tag)


def _once_lin(c, d):
    bf, tags, out = Bufs(), {}, {}
    relu = c.op.startswith('relu')
    step = c.op[5:] if relu else c.op
    x, w = bf.new('x', c.B * c.In, d['x']), bf.new('w', c.Out * c.In, d['w'])
    b = bf.new('b', c.Out, d['b']) if c.bias else None
    try:
        if c.op.endswith('fwd'):
            y = bf.new('y', c.B * c.Out)
            _call(tags, step, 'gpode_linear_relu_fwd' if relu else 'gpode_linear_fwd', x, w, b, y, c.B, c.In, c.Out)
            out['y'] = y
        else:
            gy = bf.new('gy', c.B * c.Out, d['gy'])
            g = {k: (None if c.null == k else bf.new(k, n)) for k, n in (('gx', c.B * c.In), ('gw', c.Out * c.In), ('gb', c.Out))}
            if relu:
                _call(tags, step, 'gpode_linear_relu_bwd', x, w, gy, g['gx'], g['gw'], g['gb'], c.B, c.In, c.Out)
            else:
                from vae_gp_ode_amd import _lib
                ns = _lib.load().gpode_linear_bwd_scratch(c.B, c.In, c.Out)
                assert ns == linear_bwd_scratch(c.B, c.In, c.Out)
                scratch = bf.new('scratch', ns, output=False, init=None) if c.scratch else None
                _call(tags, step, 'gpode_linear_bwd', x, w, gy, g['gx'], g['gw'], g['gb'], c.B, c.In, c.Out, scratch)
            out.update({k: v for k, v in g.items() if v is not None})
    except Refused as e:
        return dict(refused=str(e), untouched=bf.untouched()), tags, [], []
    return {k: v.cpu() for k, v in out.items()}, tags, bf.problems(), []


def _once_ew(c, d):
    bf, tags, out, bits = Bufs(), {}, {}, []
    n, nX, rows = c.n, c.n // c.reps, c.n // c.inner
    X = bf.new('X', nX, d['X'])
    if c.op.startswith('act_fwd'):
        out['y'] = bf.new('y', n)
        _call(tags, c.op, 'gpode_act_fwd', bf.new('a', n, d['a']), out['y'], n, int(c.op[-1]))
    elif c.op.startswith('act_bwd'):
        out['gx'] = bf.new('gx', n)
        _call(tags, c.op, 'gpode_act_bwd', bf.new('y', n, d['z'] if c.op[-1] == '1' else d['y0']), bf.new('g', n, d['g']), out['gx'], n, int(c.op[-1]))
    else:
        z = bf.new('z', n, d['z'])
        if c.op == 'loglik_fwd':
            out['ll'] = bf.new('ll', n)
            _call(tags, c.op, 'gpode_loglik_fwd', X, z, out['ll'], n, nX)
        elif c.op == 'loglik_bwd':
            out['gz'] = bf.new('gz', n)
            _call(tags, c.op, 'gpode_loglik_bwd', X, z, bf.new('g', n, d['g']), out['gz'], n, nX)
        elif c.op == 'rowsum_fwd':
            out['out'] = bf.new('out', rows)
            _call(tags, c.op, 'gpode_loglik_rowsum_fwd', X, z, out['out'], rows, c.inner, nX)
        else:
            grow = bf.new('grow', rows, d['grow'])
            gz = bf.new('gz', n)
            _call(tags, 'rowsum_bwd', 'gpode_loglik_rowsum_bwd', X, z, grow, gz, rows, c.inner, nX)
            out['gz'] = gz
            if c.op == 'sll_bwd':                     # the fused kernel against the chain it replaces, bit for bit
                out = dict(ga=bf.new('ga', n))
                chain = bf.new('chain', n)
                _call(tags, 'sll_bwd', 'gpode_sigmoid_loglik_bwd', X, z, grow, out['ga'], rows, c.inner, nX)
                _call(tags, 'act_bwd', 'gpode_act_bwd', z, gz, chain, n, 1)
                if not torch.equal(out['ga'], chain):
                    bits.append('ga of gpode_sigmoid_loglik_bwd differs from gpode_loglik_rowsum_bwd -> gpode_act_bwd')
    return {k: v.cpu() for k, v in out.items()}, tags, bf.problems(), bits


def _once_sll(c, d):
    bf, tags, bits = Bufs(), {}, []
    n = c.rows * c.inner
    ns = c.nsplit or sigmoid_loglik_splits(c.rows, c.inner)
    if not c.nsplit:
        from vae_gp_ode_amd import _lib
        assert _lib.load().gpode_sigmoid_loglik_splits(c.rows, c.inner) == ns
    refusal = sll_refused(c) is not None
    X = bf.new('X', c.nX, d['X'] if not refusal else torch.zeros(c.nX), shift=1 if c.mis == 'X' else 0)
    a = bf.new('a', 8 if refusal else n, torch.zeros(8) if refusal else d['a'], shift=1 if c.mis == 'a' else 0)
    z = bf.new('z', 8 if refusal else n, shift=1 if c.mis == 'z' else 0)
    part = bf.new('part', 8 if refusal else c.rows * ns)
    assert not c.mis or {'X': X, 'a': a, 'z': z}[c.mis].data_ptr() % 16 == 4
    try:
        _call(tags, 'fwd', 'gpode_sigmoid_loglik_fwd', X, a, z, part, c.rows, c.inner, c.nX, max(ns, 0))
    except Refused as e:
        return dict(refused=str(e), untouched=bf.untouched()), tags, [], []
    zz = bf.new('z_act', n)
    _call(tags, 'act', 'gpode_act_fwd', a, zz, n, 1)
    if not torch.equal(z, zz):
        bits.append('z of gpode_sigmoid_loglik_fwd differs from gpode_act_fwd(mode 1)')
    part = part.view(c.rows, ns)
    empty = torch.arange(ns) * (sll_chunk(c) + (1 if c.mis else 0)) >= c.inner
    if empty.any() and not bool((part[:, empty.cuda()] == 0).all()):
        bits.append('the parts of empty slices are not 0')
    return dict(z=z.cpu(), part=part.cpu(), rowsum=part.double().sum(1).cpu()), tags, bf.problems(), bits


def _halves(bf, name, mu, lv, packed):
    """(mu, logvar, ld) on the device: two tensors, or the halves of one (N, 2q) tensor; mu None: NaN-filled outputs"""
    N, q = mu.shape if torch.is_tensor(mu) else mu
    if not packed:
        if torch.is_tensor(mu):
            return bf.new(name + '_mu', N * q, mu), bf.new(name + '_lv', N * q, lv), q
        return bf.new(name + '_mu', N * q), bf.new(name + '_lv', N * q), q
    h = bf.new(name, 2 * N * q, torch.cat((mu, lv), 1) if torch.is_tensor(mu) else None).view(N, 2 * q)
    return h[:, :q], h[:, q:], 2 * q


def _unhalve(t, N, q, ld):
    return t.reshape(N, q).contiguous().cpu()


def _once_glue(c, d):
    bf, tags, out, bits = Bufs(), {}, {}, []
    N, q = c.N, c.q
    mu, lv, ld = _halves(bf, 'h', d['mu'], d['logvar'], c.packed)
    gmu, glv, ldg = _halves(bf, 'gh', (N, q), None, c.packed)
    eps = bf.new('eps', N * q, d['eps'])
    if c.op == 'normal_kl':
        out['klrow'] = bf.new('klrow', N)
        _call(tags, 'fwd', 'gpode_normal_kl_fwd', mu, lv, ld, out['klrow'], N, q)
        _call(tags, 'bwd', 'gpode_normal_kl_bwd', bf.new('grow', N, d['grow']), mu, lv, ld, gmu, glv, ldg, N, q)
    else:
        z = bf.new('z', N * q)
        out['z'] = z
        gz = bf.new('gz', N * q, d['gz'])
        if c.op == 'reparam':
            _call(tags, 'fwd', 'gpode_reparam_fwd', mu, lv, ld, eps, z, N, q)
            _call(tags, 'bwd', 'gpode_reparam_bwd', gz, lv, ld, eps, gmu, glv, ldg, N, q)
        else:
            nb = -(-N * q // 256)
            klpart = bf.new('klpart', nb)
            _call(tags, 'fwd', 'gpode_reparam_kl_fwd', mu, lv, ld, eps, z, klpart, N, q)
            _call(tags, 'bwd', 'gpode_reparam_kl_bwd', None if c.null == 'gz' else gz, None if c.null == 'gkl' else bf.new('gkl', nb, d['gkl']),
                  mu, lv, ld, eps, gmu, glv, ldg, N, q)
            zp = bf.new('z_plain', N * q)
            _call(tags, 'plain', 'gpode_reparam_fwd', mu, lv, ld, eps, zp, N, q)
            if not torch.equal(z, zp):
                bits.append('z of gpode_reparam_kl_fwd differs from gpode_reparam_fwd')
            out['klsum'] = klpart.double().sum().reshape(1)
    res = {k: v.cpu() for k, v in out.items()}
    res['gmu'], res['glogvar'] = _unhalve(gmu, N, q, ldg), _unhalve(glv, N, q, ldg)
    return res, tags, bf.problems(), bits


def _once_elbo(c, d):
    bf, tags = Bufs(), {}
    out, gl, gk, gu = bf.new('out', 4), bf.new('glhood', c.nl), bf.new('gklrow', c.nk), bf.new('gklu', 1)
    _call(tags, 'fwd', 'gpode_elbo_fwd', bf.new('lhood', c.nl, d['lhood']), c.nl, bf.new('klrow', c.nk, d['klrow']), c.nk, bf.new('klu', 1, d['klu']),
          ctypes.c_float(NOBS), out)
    _call(tags, 'bwd', 'gpode_elbo_bwd', bf.new('gout', 4, d['gout']), c.nl, c.nk, ctypes.c_float(NOBS), gl, gk, gu)
    return dict(out=out.cpu(), glhood=gl.cpu(), gklrow=gk.cpu(), gklu=gu.cpu()), tags, bf.problems(), []


def _once_ea(c, d):
    bf, tags, bits = Bufs(), {}, []
    M, Do = c.M, c.Do
    P = M * (M + 1) // 2
    Um, Us = bf.new('Um', M * Do, d['Um']), bf.new('Us', Do * P, d['Us'])
    dUm, dUs = bf.new('dUm', M * Do), bf.new('dUs', Do * P)
    res = {}
    if c.entry == 'svgp':
        kl = bf.new('kl', 1)
        _call(tags, 'fwd', 'gpode_svgp_kl_fwd', M, Do, Um, Us, kl)
        _call(tags, 'bwd', 'gpode_svgp_kl_bwd', M, Do, Um, Us, bf.new('g', 1, d['g']), dUm, dUs)
        res['kl'] = kl.cpu()
    else:
        rows = c.nl_values // c.ns
        lpart = bf.new('lpart', c.nl_values, d['lpart'])
        # the 4 results are outputs; the kElboParts floats behind them are scratch, written only when Us is summed in parts
        out = bf.new('out', 4 + ELBO_PARTS, output=False)
        gs = [bf.new('g%d' % i, 1, d['g%d' % i]) if ('g%d' % i) in d else None for i in range(4)]
        glrow = bf.new('glrow', rows)
        nobs = ctypes.c_float(NOBS)
        if c.entry != 'all':
            n, nX = rows * EA_INNER, d['X'].numel()
            X, z, ga = bf.new('X', nX, d['X']), bf.new('z', n, d['z']), bf.new('ga', n)
        if c.entry == 'all_kl':
            kls, klv = bf.new('kls', c.nks, d['kls']), (bf.new('klv', c.nkv, d['klv']) if c.nkv else None)
            gkls, gklv = bf.new('gkls', c.nks), (bf.new('gklv', c.nkv) if c.nkv else None)
            _call(tags, 'fwd', 'gpode_elbo_all_fwd_kl', lpart, rows, c.nl_values, kls, c.nks, klv, c.nkv, c.N, M, Do, Um, Us, nobs, out)
            _call(tags, 'bwd', 'gpode_elbo_all_bwd_ll_kl', *gs, rows, c.N, M, Do, Um, Us, nobs, glrow, gkls, c.nks, gklv, c.nkv, dUm, dUs, X, z, ga,
                  n, nX)
            res['gkls'] = gkls.cpu()
            if c.nkv:
                res['gklv'] = gklv.cpu()
        else:
            hs = bf.new('hs', c.N * 2 * c.q, d['hs'])
            hv = bf.new('hv', c.N * 2 * c.q, d['hv']) if c.hv else None
            ghs = bf.new('ghs', c.N * 2 * c.q)
            ghv = bf.new('ghv', c.N * 2 * c.q) if c.hv else None
            _call(tags, 'fwd', 'gpode_elbo_all_fwd', lpart, rows, c.nl_values, hs, hv, c.N, c.q, M, Do, Um, Us, nobs, out)
            if c.entry == 'all':
                _call(tags, 'bwd', 'gpode_elbo_all_bwd', *gs, rows, hs, hv, c.N, c.q, M, Do, Um, Us, nobs, glrow, ghs, ghv, dUm, dUs)
            else:
                _call(tags, 'bwd', 'gpode_elbo_all_bwd_ll', *gs, rows, hs, hv, c.N, c.q, M, Do, Um, Us, nobs, glrow, ghs, ghv, dUm, dUs, X, z, ga,
                      n, nX)
            res['ghs'] = ghs.view(c.N, 2 * c.q).cpu()
            if c.hv:
                res['ghv'] = ghv.view(c.N, 2 * c.q).cpu()
        torch.cuda.synchronize()
        if bool(torch.isnan(out[:4]).any()):
            bits.append('out: a NaN of the fill is left')
        tail = torch.isnan(out[4:])
        if bool(tail.any()) if us_in_parts(M, Do) else not bool(tail.all()):
            bits.append('out: the scratch tail is %s' % ('not fully written' if us_in_parts(M, Do) else 'written without need'))
        res['out'], res['glrow'] = out[:4].cpu(), glrow.cpu()
        if c.entry != 'all':                          # the fused logit gradient against gpode_sigmoid_loglik_bwd on the uniform row gradient
            ga2 = bf.new('ga_sll', n)
            _call(tags, 'sll_bwd', 'gpode_sigmoid_loglik_bwd', X, z, glrow, ga2, rows, EA_INNER, nX)
            if not torch.equal(ga, ga2):
                bits.append('ga of the fused backward differs from gpode_sigmoid_loglik_bwd')
            res['ga'] = ga.cpu()
    di = diag_index(M)
    off = torch.ones(P, dtype=torch.bool)
    off[di] = False
    dUs = dUs.view(Do, P).cpu()
    res['dUm'], res['dUs_diag'] = dUm.view(M, Do).cpu(), dUs[:, di]
    if M > 1:
        res['dUs_off'] = dUs[:, off]
    return res, tags, bf.problems(), bits


def _table(ptrs):
    return torch.tensor(ptrs, dtype=torch.int64, device='cuda')


def _once_adam(c, d):
    bf, tags, bits, res = Bufs(), {}, [], {}
    total, nt = sum(c.sizes), len(c.sizes)
    offs = [sum(c.sizes[:i]) for i in range(nt)]
    bufs = {k: [] for k in 'pgmv'}
    for i, (o, s) in enumerate(zip(offs, c.sizes)):   # every tensor in a buffer of its own with a guard behind it; an empty one is a guard alone
        bufs['p'].append(bf.new('p%d' % i, s, d['p'][o:o + s]))
        bufs['g'].append(bf.new('g%d' % i, s, torch.zeros(s)))
        bufs['m'].append(bf.new('m%d' % i, s, torch.zeros(s)))
        bufs['v'].append(bf.new('v%d' % i, s, torch.zeros(s)))
    tabs = {k: _table([t.data_ptr() for t in v]) for k, v in bufs.items()}
    offs_d = _table(offs)
    step_dev = torch.zeros(2, dtype=torch.int32, device='cuda') if c.dev else None
    flat = bf.new('flat', total)
    f = ctypes.c_float
    prev = d['p'].double()
    for t, g in enumerate(d['grads'], 1):
        for i, (o, s) in enumerate(zip(offs, c.sizes)):
            bufs['g'][i].copy_(g[o:o + s])
        # with the device-side counter the host's step is ignored: hand it a wrong one
        _call(tags, 'adam', 'gpode_adam_multi', tabs['p'], tabs['g'], tabs['m'], tabs['v'], offs_d, nt, total, f(LR), f(BETA1), f(BETA2), f(EPS),
              1000 if c.dev else t, step_dev)
        if c.dev and step_dev.cpu().tolist() != [t, 0]:
            bits.append('step_dev reads %s after %d launches' % (step_dev.cpu().tolist(), t))
        for k, name in (('p', 'p'), ('m', 'm'), ('v', 'v')):
            res['%s%d' % (name, t)] = torch.cat([x.cpu() for x in bufs[k]])
        res['upd%d' % t] = res['p%d' % t].double() - prev
        prev = res['p%d' % t].double()
    _call(tags, 'gather', 'gpode_gather_multi', tabs['g'], offs_d, nt, total, flat)
    if not torch.equal(flat.cpu(), d['grads'][-1]):
        bits.append('gpode_gather_multi: flat differs from the concatenation')
    return res, tags, bf.problems(), bits


_ONCE = {Lin: _once_lin, Ew: _once_ew, Sll: _once_sll, Glue: _once_glue, Elbo: _once_elbo, EA: _once_ea, Adam: _once_adam}


def _bits(t):
    """floats as integers: a NaN equals itself"""
    return t.contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def launch(c):
    """Case c TWICE; the record of the first run with what the checks of both found and what differs in the second"""
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inputs(c).items()} if not isinstance(c, Adam) else inputs(c)
    (out, tags, problems, bits), (out2, tags2, problems2, bits2) = _ONCE[type(c)](c, d), _ONCE[type(c)](c, d)
    differs = [k for k in out if torch.is_tensor(out[k]) and not torch.equal(_bits(out[k]), _bits(out2[k]))]
    return dict(out=out, tags=tags, bits=bits + bits2, problems=problems + problems2 + ['the second run differs in %s' % k for k in differs] +
                ([] if tags == tags2 else ['the second run took %s' % tags2]))


# ---- comparison --------------------------------------------------------------------------------------------------------------------------
def errors(c, out):
    """{output: (error, bound, step)} of the outputs `out` of case c against reference(c)"""
    r = {}
    for key, (ref, tol, scale, step) in reference(c).items():
        if isinstance(c, Sll) and key == 'rowsum' and c.inner <= SLL_SHORT:
            ref, scale = sll_short_rows(c, out['z'])
        g, ref = out[key].double().reshape(-1), ref.reshape(-1)
        assert g.shape == ref.shape, (case_id(c), key, g.shape, ref.shape)
        s = ref.abs().max().clamp_min(1e-30) if scale is None else (scale.reshape(-1) if torch.is_tensor(scale) else scale)
        e = ((g - ref).abs() / s).max().item()
        r[key] = (float('inf') if e != e else e, tol, step)
    return r


def check(c, got, SEEN, MAXIMA):
    """every figure is printed before anything is asserted: a case that is red for its tag still shows its errors"""
    cid = case_id(c)
    errs = errors(c, got['out'])
    for key, (e, tol, step) in errs.items():
        print('%s %s: %.2e (bound %.1e)' % (cid, key, e, tol))
    assert got['tags'] == expected(c), (cid, got['tags'], expected(c))
    SEEN.update(got['tags'].values())
    assert not got['problems'], (cid, got['problems'])
    assert not got['bits'], (cid, got['bits'])
    bad = []
    for key, (e, tol, step) in errs.items():
        tag = got['tags'][step]
        if tag not in MAXIMA or e / tol > MAXIMA[tag][0] / MAXIMA[tag][1]:
            MAXIMA[tag] = (e, tol, cid + ':' + key)
        if not e <= tol:
            bad.append('%s: %.3e > %.1e' % (key, e, tol))
    assert not bad, (cid, bad)
