"""Every launch arm of the convolution dispatch (csrc/vae_conv_tiled.hip, csrc/vae_conv.hip) through the C ABI, shared by
test_gpu_conv_dispatch.py and test_gpu_conv_wgrad.py.

A case is (layer, op, B, in_bn, sink, shift): one of the seven conv geometries the dispatch knows, one of the three entry-point
families (op 'fwd' = gpode_conv2d_fwd, 'bwd_data' = gpode_conv2d_bwd_data[_bn] / gpode_convT_fwd_stats, 'bwd_weight' =
gpode_conv2d_bwd_weight[_bn]; for a ConvTranspose2d layer these are its d/d input, forward and d/d weight), a batch size, with / without
the BatchNorm + ReLU table of the input, with / without a statistics sink, and the operand that is shifted by one float (unaligned
mode).  run_case() launches it into NaN-filled buffers with guard floats behind them and returns the outputs, the tag of the arm that
ran (gpode_last_launch) and the buffer checks; reference() is torch in fp64 on the same inputs.  The module is also the program of the
GPODE_CONV_VALU=1 child process (the switch is read once per process): `python conv_dispatch.py valu <n> <file>` runs every case of
that mode and saves the outputs.

EXPECTED (function expected()) is the dispatch table as it stands: which arm serves (layer, op, batch size, in_bn, sink) on the
matrix-core path and off it, and which requests are refused."""
import collections
import ctypes
import functools
import os
import subprocess
import sys
import tempfile

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5                      # outputs and input gradients: conv_engine_v2.TOL; weight gradients 5 TOL (test_gpu_vae_layers.py)
GUARD = 4096
MOM, EPS = 0.1, 1e-5
Case = collections.namedtuple('Case', 'layer op B in_bn sink shift', defaults=(False, False, None))
# conv geometry (Ci, H, Co, K, S, P, Ho) -- for a ConvTranspose2d layer that of the convolution it is the adjoint of
LAYERS = {'dec1': (64, 6, 32, 3, 1, 0, 4), 'dec4': (32, 13, 64, 5, 2, 1, 6), 'dec7': (16, 28, 32, 5, 2, 1, 13),
          'dec10': (1, 28, 16, 5, 1, 2, 28), 'cnn0': (1, 28, 8, 5, 2, 2, 14), 'cnn0v': (5, 28, 8, 5, 2, 2, 14),
          'cnn3': (8, 14, 16, 5, 2, 2, 7), 'cnn6': (16, 7, 32, 5, 2, 2, 4)}
DEC = ('dec1', 'dec4', 'dec7', 'dec10')
# arms whose kernels accumulate one output in a single fp32 chain (VALU and generic kernels): see bound()
CHAIN_TAGS = ('conv_fwd', 'conv_bwd_data', 'conv_bwd_weight', 'convT_fwd_tiled', 'convT_bwd_data_tiled', 'convT_wgrad_tiled', 'dec10_fwd',
              'dec10_wgrad', 'enc_conv3_bwd_data_tiled')
REQUIRED_TAGS = CHAIN_TAGS + ('convT_fwd_mfma', 'convT_fwd_mfma_stats', 'convT_wgrad_mfma', 'enc_conv3_fwd_mfma', 'enc_conv6_fwd_mfma',
                              'enc_conv6_bwd_data_mfma', 'dec1_fwd_mfma', 'dec1_bwd_data_mfma', 'dec1_wgrad_mfma', 'dec4_fwd_tapcols',
                              'dec10_fwd_mfma', 'dec10_bwd_data_mfma', 'dec10_wgrad_mfma', 'convT_wgrad_v2', 'conv_v2_dec7_fwd',
                              'conv_v2_dec7_fwd_bn', 'conv_v2_dec7_fwd_stats', 'conv_v2_dec7_fwd_bn_stats', 'conv_v2_dec7_bwd_data',
                              'conv_v2_dec4_bwd_data')
REFUSE_PATH, REFUSE_GEOM = 'matrix-core path', 'specialisation'     # what a refusal's message names


def expected(c, n, mfma):
    """The tag of the arm that serves case c on a device of n CUs -- mfma: the matrix-core path is open (no GPODE_CONV_VALU, every
    operand 16-byte aligned) -- or ('refused', what the message names)."""
    L, B = c.layer, c.B
    if c.op == 'fwd':
        if L in DEC:
            return {'dec7': 'conv_v2_dec7_bwd_data', 'dec4': 'conv_v2_dec4_bwd_data', 'dec1': 'dec1_bwd_data_mfma',
                    'dec10': 'dec10_bwd_data_mfma'}[L] if mfma else 'convT_bwd_data_tiled'
        return {'cnn3': 'enc_conv3_fwd_mfma', 'cnn6': 'enc_conv6_fwd_mfma'}.get(L, 'conv_fwd') if mfma else 'conv_fwd'
    if c.op == 'bwd_data':
        if c.sink and (L not in ('dec1', 'dec4', 'dec7') or (L == 'dec1' and c.in_bn)):
            return ('refused', REFUSE_GEOM)
        if L in ('dec7', 'dec4', 'dec1', 'dec10'):
            if not mfma:
                if c.sink or c.in_bn:
                    return ('refused', REFUSE_PATH)
                if L == 'dec10':
                    return 'conv_bwd_data' if c.shift == 'y' else 'dec10_fwd'      # the VALU kernel stores float4
                return 'convT_fwd_tiled'
            if L == 'dec7':
                return 'conv_v2_dec7_fwd' + ('_bn' if c.in_bn else '') + ('_stats' if c.sink else '')
            if L == 'dec4':
                return 'dec4_fwd_tapcols' if B <= 4 * n else ('convT_fwd_mfma_stats' if c.sink else 'convT_fwd_mfma')
            if L == 'dec1':
                return 'convT_fwd_mfma' if c.in_bn else 'dec1_fwd_mfma'
            return 'dec10_fwd_mfma'
        if L == 'cnn6' and mfma:
            return 'enc_conv6_bwd_data_mfma'
        if c.in_bn:
            return ('refused', REFUSE_GEOM)
        return 'enc_conv3_bwd_data_tiled' if L == 'cnn3' and B >= 96 else 'conv_bwd_data'
    if mfma and L != 'cnn0' and L != 'cnn0v' and L != 'cnn3':
        return {'dec7': 'convT_wgrad_v2', 'dec4': 'convT_wgrad_v2', 'dec1': 'convT_wgrad_mfma' if c.in_bn else 'dec1_wgrad_mfma',
                'dec10': 'dec10_wgrad_mfma', 'cnn6': 'convT_wgrad_mfma'}[L]
    if c.in_bn:
        return ('refused', REFUSE_PATH if L in DEC else REFUSE_GEOM)
    return 'conv_bwd_weight' if L not in DEC else ('dec10_wgrad' if L == 'dec10' else 'convT_wgrad_tiled')


def path_open(c):
    """whether case c leaves the matrix-core path open when GPODE_CONV_VALU is unset: every operand aligned -- the weight gradient itself
    may be unaligned, it is written by the final reduction, element by element"""
    return c.shift is None or (c.op == 'bwd_weight' and c.shift == 'y')


def default_cases(n):
    """No switch, aligned operands.  Batch sizes from the CU count n: 1; n + 1 (one workgroup gets a second image); IPB n + 1 for the
    persistent kernels that take IPB images per group (the loop over groups wraps); 2 n + 1 (a workgroup of convT_wgrad_v2 with three
    images reuses plane buffer 0; dec1's kernels run two workgroups per CU); 3 n + 37 ragged; and the thresholds, one below and one at."""
    G = (1, n + 1, 3 * n + 37)
    out = []
    for L in LAYERS:
        wrap = {'cnn3': (4 * n + 1,), 'cnn6': (8 * n + 1,), 'dec7': (2 * n + 1,), 'dec4': (2 * n + 1,), 'dec1': (2 * n + 1,),
                'dec10': (8 * n + 1,)}.get(L, ())
        out += [Case(L, 'fwd', B) for B in G + wrap]
    out += [Case(L, 'bwd_data', B) for L in ('cnn0', 'cnn0v') for B in G]
    out += [Case('cnn3', 'bwd_data', B) for B in G + (95, 96)]
    out += [Case('cnn6', 'bwd_data', B) for B in G + (2 * n + 1, 4 * n - 1, 4 * n, 8 * n + 1)]
    out += [Case('cnn6', 'bwd_data', B, True) for B in (n + 1, 8 * n + 1)]
    for in_bn in (False, True):
        for sink in (False, True):
            out += [Case('dec7', 'bwd_data', B, in_bn, sink) for B in G]
            out += [Case('dec4', 'bwd_data', B, in_bn, sink) for B in G + (4 * n, 4 * n + 1)]
        out += [Case('dec10', 'bwd_data', B, in_bn) for B in G]
        out += [Case('dec7', 'bwd_weight', B, in_bn) for B in G + (2 * n + 1,)]
        out += [Case('dec4', 'bwd_weight', B, in_bn) for B in G + (2 * n + 1,)]
        out += [Case('dec10', 'bwd_weight', B, in_bn) for B in G]
    out += [Case('dec1', 'bwd_data', B, False, sink) for sink in (False, True) for B in G + (2 * n + 1,)]
    out += [Case('dec1', 'bwd_data', B, True) for B in G + (8 * n + 1,)]
    out += [Case('dec1', 'bwd_weight', B) for B in G]
    out += [Case('dec1', 'bwd_weight', B, True) for B in G + (8 * n + 1,)]
    out += [Case('cnn6', 'bwd_weight', B) for B in G + (8 * n + 1,)]
    out += [Case(L, 'bwd_weight', B) for L in ('cnn0', 'cnn0v', 'cnn3') for B in G]
    return out


def valu_cases(n):
    """GPODE_CONV_VALU=1: every layer and operation on the VALU / generic kernels.  Their grids are one workgroup per image group or per
    slice of the batch (no persistent loop), so the edges are the partial last group and the batch split: 1, n + 1, 3 n + 37, and
    cnn.3's threshold."""
    G = (1, n + 1, 3 * n + 37)
    out = [Case(L, op, B) for L in LAYERS for op in ('fwd', 'bwd_data', 'bwd_weight') for B in G]
    return out + [Case('cnn3', 'bwd_data', 95), Case('cnn3', 'bwd_data', 96)]


def valu_refusals(n):
    B = n + 1
    return ([Case(L, 'bwd_data', B, True) for L in DEC] + [Case(L, 'bwd_weight', B, True) for L in DEC] +
            [Case(L, 'bwd_data', B, False, True) for L in ('dec1', 'dec4', 'dec7')] + [Case('dec7', 'bwd_data', B, True, True)])


OPERANDS = {'fwd': ('x', 'y', 'w'), 'bwd_data': ('x', 'y', 'w'), 'bwd_weight': ('x', 'x2', 'y')}


def unaligned_cases(n):
    """One operand at a time shifted by one float (data pointer = 4 mod 16): the input, the second input of d/d weight, the output, the
    weights -- batch size n + 1.  (The table: unaligned_refusals.)"""
    return [Case(L, op, n + 1, False, False, s) for L in LAYERS for op in OPERANDS for s in OPERANDS[op]]


def unaligned_refusals(n):
    """in_bn (or a sink) with an operand that closes the matrix-core path, the table itself included"""
    B = n + 1
    out = [Case(L, op, B, True, False, s) for L in DEC for op in ('bwd_data', 'bwd_weight') for s in ('x', 'bn')]
    out += [Case(L, 'bwd_data', B, False, True, 'x') for L in ('dec1', 'dec4', 'dec7')]
    return out + [Case('cnn6', 'bwd_data', B, True, False, 'bn'), Case('cnn6', 'bwd_weight', B, True, False, 'bn')]


def default_refusals(n):
    B = n + 1
    return [Case('dec10', 'bwd_data', B, False, True), Case('dec1', 'bwd_data', B, True, True), Case('cnn3', 'bwd_data', B, True),
            Case('cnn3', 'bwd_weight', B, True), Case('cnn0', 'bwd_weight', B, True)]


def case_id(c):
    return '%s-%s-B%d%s%s%s' % (c.layer, c.op, c.B, '-bn' if c.in_bn else '', '-sink' if c.sink else '', '-shift_' + c.shift if c.shift else '')


# ---- inputs, reference -----------------------------------------------------------------------------------------------------------
def inputs(c, step=0):
    """x: the first operand (B, Ci, H, H) of 'fwd' / 'bwd_weight'; gy: the (B, Co, Ho, Ho) operand of 'bwd_data' / 'bwd_weight', the one
    the table applies to (scales of test_fused_batchnorm_relu_conv_transpose; the table holds its batch statistics, fp64, rounded)"""
    Ci, H, Co, K, S, P, Ho = LAYERS[c.layer]
    g = torch.Generator().manual_seed(100003 * step + 1009 * list(LAYERS).index(c.layer) + c.B)
    d = dict(w=torch.randn(Co, Ci, K, K, generator=g) * (0.05 if Ci > 1 else 0.2))
    d['x'] = torch.randn(c.B, Ci, H, H, generator=g)
    d['gy'] = torch.randn(c.B, Co, Ho, Ho, generator=g) * 1.3 + 0.2
    gam, bet = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.3
    g64 = d['gy'].double()
    mean, var = g64.mean((0, 2, 3)), g64.var((0, 2, 3), unbiased=False)
    d['table'] = torch.stack([mean, torch.rsqrt(var + EPS), gam.double(), bet.double()], 1).float().contiguous()
    d['bias_out'] = torch.randn(Co, generator=g) * 0.1      # Conv2d forward
    d['bias_in'] = torch.randn(Ci, generator=g) * 0.1       # ConvTranspose2d forward
    d['gam_out'], d['bet_out'] = torch.rand(Ci, generator=g) + 0.5, torch.randn(Ci, generator=g) * 0.3
    return d


def has_bias(c):
    """'fwd' of an encoder layer (Conv2d forward) and 'bwd_data' of a decoder layer (ConvTranspose2d forward) carry the layer's bias; the
    other direction is an input gradient.  'bwd_weight' of an encoder layer also produces the bias gradient."""
    return (c.layer in DEC) == (c.op == 'bwd_data') if c.op != 'bwd_weight' else c.layer not in DEC


def _bn_relu(v, table):
    t = table.to(v.dtype)
    return F.relu((v - t[:, 0].view(1, -1, 1, 1)) * (t[:, 1] * t[:, 2]).view(1, -1, 1, 1) + t[:, 3].view(1, -1, 1, 1))


def reference(c, dtype=torch.float64, only=None):
    """torch on the CPU in `dtype` on every image (only: a slice of the batch for the first operand -- image attribution): a list of
    steps (two with a sink), each a dict of the outputs and, with a sink, the statistics a BatchNorm2d in training mode would hold"""
    Ci, H, Co, K, S, P, Ho = LAYERS[c.layer]
    steps, rm, rv = [], torch.zeros(Ci, dtype=dtype), torch.ones(Ci, dtype=dtype)
    for step in range(2 if c.sink else 1):
        d = {k: v.to(dtype) for k, v in inputs(c, step).items()}
        gy = _bn_relu(d['gy'], d['table']) if c.in_bn else d['gy']
        if c.op == 'fwd':
            steps.append(dict(y=F.conv2d(d['x'], d['w'], d['bias_out'] if has_bias(c) else None, stride=S, padding=P)))
        elif c.op == 'bwd_data':
            op = H - ((Ho - 1) * S - 2 * P + K)
            y = F.conv_transpose2d(gy, d['w'], d['bias_in'] if has_bias(c) else None, stride=S, padding=P, output_padding=op)
            r = dict(y=y)
            if c.sink:
                cnt = c.B * H * H
                mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
                rm, rv = (1 - MOM) * rm + MOM * mean, (1 - MOM) * rv + MOM * var * cnt / (cnt - 1)
                invstd = torch.rsqrt(var + EPS)
                g0 = inputs(c, 0)
                r.update(mean=mean, invstd=invstd, rm=rm, rv=rv, nbt=step + 1,
                         table=torch.stack([mean, invstd, g0['gam_out'].to(dtype), g0['bet_out'].to(dtype)], 1))
            steps.append(r)
        else:
            x = d['x']
            if only is not None:
                x, gy = x[only:only + 1], gy[only:only + 1]
            r = dict(y=torch.nn.grad.conv2d_weight(x, d['w'].shape, gy, stride=S, padding=P))
            if has_bias(c):
                r['gbias'] = d['gy'].sum((0, 2, 3))
            steps.append(r)
    return steps


# ---- launches --------------------------------------------------------------------------------------------------------------------
def _dev(t, shift=False):
    """t on the device; shift: as a view that starts one float behind a 16-byte boundary"""
    if not shift:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, device='cuda')[1:]
    assert buf.data_ptr() % 16 == 4
    buf.copy_(t.reshape(-1))
    return buf.view(t.shape)


def _nan_buffer(n, shift=False):
    buf = torch.full((n + GUARD + 1,), float('nan'), device='cuda')
    buf = buf[1:] if shift else buf[:-1]
    assert buf.data_ptr() % 16 == (4 if shift else 0)
    return buf


class Refused(Exception):
    pass


def launch(c, d, bn=None, gbias=False, zero_x_except=None, deferred=False):
    """One launch of case c on the device tensors d into NaN-filled buffers with GUARD NaN floats behind them.  bn: the module state a
    sink updates.  Returns the outputs (on the device), the tag of the arm that ran and what the buffer checks found; raises Refused
    with the library's message when the call returns non-zero (after checking that nothing was written)."""
    from vae_gp_ode_amd import _lib
    from vae_gp_ode_amd.ops import _ptr, _stream
    lib = _lib.load()
    Ci, H, Co, K, S, P, Ho = LAYERS[c.layer]
    geo = (c.B, Ci, H, H, Co, K, S, P, Ho, Ho)
    table = d['table'] if c.in_bn else None
    out, extra = {}, []
    if c.op == 'fwd':
        n = c.B * Co * Ho * Ho
        buf = _nan_buffer(n, c.shift == 'y')
        call = ('gpode_conv2d_fwd', _ptr(d['x']), _ptr(d['w']), _ptr(d['bias_out'] if has_bias(c) else None), _ptr(buf), *geo, _stream())
        shape = (c.B, Co, Ho, Ho)
    elif c.op == 'bwd_data':
        n = c.B * Ci * H * H
        buf = _nan_buffer(n, c.shift == 'y')
        bias = d['bias_in'] if has_bias(c) else None
        shape = (c.B, Ci, H, H)
        if bn is not None:
            mean, invstd, tab = (torch.full(s, float('nan'), device='cuda') for s in ((Ci,), (Ci,), (Ci, 4)))
            scratch = torch.empty(int(lib.gpode_convT_fwd_stats_scratch(Ci)), device='cuda')
            extra = [mean, invstd, tab]
            call = ('gpode_convT_fwd_stats', _ptr(d['gy']), _ptr(table), _ptr(d['w']), _ptr(bias), _ptr(buf), *geo, _ptr(bn['gam']),
                    _ptr(bn['bet']), _ptr(mean), _ptr(invstd), _ptr(bn['rm']), _ptr(bn['rv']), _ptr(bn['nbt']), ctypes.c_float(MOM),
                    ctypes.c_float(EPS), _ptr(tab), _ptr(scratch), 5, _stream())
        elif table is not None:
            call = ('gpode_conv2d_bwd_data_bn', _ptr(d['gy']), _ptr(table), _ptr(d['w']), _ptr(bias), _ptr(buf), *geo, _stream())
        else:
            call = ('gpode_conv2d_bwd_data', _ptr(d['gy']), _ptr(d['w']), _ptr(bias), _ptr(buf), *geo, _stream())
    else:
        n = Co * Ci * K * K
        buf = _nan_buffer(n, c.shift == 'y')
        ns = int(lib.gpode_conv_wgrad_scratch(c.B, Ci, Co, K))
        scratch = _nan_buffer(ns)
        gb = _nan_buffer(Co) if gbias else None
        extra = [scratch] + ([gb] if gbias else [])
        shape = (Co, Ci, K, K)
        if table is not None:
            call = ('gpode_conv2d_bwd_weight_bn', _ptr(d['x']), _ptr(d['gy']), _ptr(table), _ptr(buf), _ptr(gb), _ptr(scratch), *geo, _stream())
        else:
            call = ('gpode_conv2d_bwd_weight', _ptr(d['x']), _ptr(d['gy']), _ptr(buf), _ptr(gb), _ptr(scratch), *geo, _stream())
    if deferred:
        lib.gpode_defer_reductions(1)
    rc = getattr(lib, call[0])(*call[1:])
    if deferred:
        lib.gpode_defer_reductions(0)
        if rc == 0:
            torch.cuda.synchronize()
            assert torch.isnan(buf[:n]).all(), 'a deferred reduction ran before the flush'
            _lib.call('gpode_flush_reductions', _stream())
    torch.cuda.synchronize()
    if rc != 0:
        msg = lib.gpode_last_error().decode()
        assert torch.isnan(buf).all() and all(torch.isnan(e).all() for e in extra), 'a refused call wrote something: ' + msg
        raise Refused(msg)
    out['tag'] = lib.gpode_last_launch().decode()
    assert not torch.isnan(buf[:n]).any(), 'output elements left unwritten (or a NaN partial was read)'
    assert torch.isnan(buf[n:]).all(), 'wrote past the end of the output'
    out['y'] = buf[:n].view(shape)
    if c.op == 'bwd_weight':
        assert torch.isnan(scratch[ns:]).all(), 'wrote past the end of the scratch gpode_conv_wgrad_scratch() sizes'
        if gbias:
            assert not torch.isnan(gb[:Co]).any() and torch.isnan(gb[Co:]).all(), 'bias gradient: unwritten elements, or written past the end'
            out['gbias'] = gb[:Co]
    if bn is not None:
        assert not any(torch.isnan(e).any() for e in extra), 'statistics left unwritten'
        out.update(mean=mean, invstd=invstd, table=tab, rm=bn['rm'].clone(), rv=bn['rv'].clone(), nbt=int(bn['nbt']))
    return out


def device_inputs(c, step=0):
    d = inputs(c, step)
    first = 'gy' if c.op == 'bwd_data' else 'x'          # the operand the issue calls "the input"
    sh = {first: c.shift == 'x', 'gy' if first == 'x' else None: c.shift == 'x2', 'w': c.shift == 'w', 'table': c.shift == 'bn'}
    return {k: _dev(v, sh.get(k, False)) for k, v in d.items()}


def run_case(c):
    """All launches of one case: the steps (two with a sink, else one), each run TWICE and required bit-identical; for 'bwd_weight' the
    tag is read from a call without the bias gradient (gpode_chan_sum overwrites it otherwise) and the bias gradient comes from a second
    call.  Returns the steps with CPU tensors."""
    steps, bn = [], None
    for step in range(2 if c.sink else 1):
        d = device_inputs(c, step)
        if c.sink and bn is None:
            Ci = LAYERS[c.layer][0]
            bn = dict(gam=d['gam_out'], bet=d['bet_out'], rm=torch.zeros(Ci, device='cuda'), rv=torch.ones(Ci, device='cuda'),
                      nbt=torch.zeros((), dtype=torch.long, device='cuda'))
        again = {k: v.clone() for k, v in bn.items()} if bn is not None else None
        a, b = launch(c, d, bn), launch(c, d, again)
        for k in a:
            same = torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]
            assert same, 'second run differs in ' + k
        if c.op == 'bwd_weight' and has_bias(c) and c.shift == 'x2' and LAYERS[c.layer][6] ** 2 % 4 == 0:
            try:                                     # gpode_chan_sum reads float4 where the image size allows: refused up front
                launch(c, d, gbias=True)
                raise AssertionError('a bias gradient of an unaligned gy was served')
            except Refused as e:
                assert '16-byte aligned' in str(e), str(e)
        elif c.op == 'bwd_weight' and has_bias(c):
            g = launch(c, d, gbias=True)
            assert torch.equal(g['y'], a['y']), 'the weight gradient depends on whether the bias gradient is asked for'
            a['gbias'] = g['gbias']
        steps.append({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in a.items()})
    for s in steps[:-1]:
        del s['y']
    return steps


def refusal(c):
    """The library's message for a case it must refuse; None if it served it."""
    d = device_inputs(c)
    bn = None
    if c.sink:
        Ci = LAYERS[c.layer][0]
        bn = dict(gam=d['gam_out'], bet=d['bet_out'], rm=torch.zeros(Ci, device='cuda'), rv=torch.ones(Ci, device='cuda'),
                  nbt=torch.zeros((), dtype=torch.long, device='cuda'))
    try:
        launch(c, d, bn)
    except Refused as e:
        if bn is not None:
            assert int(bn['nbt']) == 0 and torch.equal(bn['rm'], torch.zeros_like(bn['rm'])), 'a refused call updated the running statistics'
        return str(e)
    return None


# ---- comparison ------------------------------------------------------------------------------------------------------------------
STAT_KEYS = ('mean', 'invstd', 'rm', 'rv', 'table')


def bound(c, key, tag, err, ref):
    """TOL for outputs and input gradients, 5 TOL for weight (and bias) gradients: the project's own bounds.  An arm of CHAIN_TAGS (one
    fp32 accumulation chain per output, where the matrix-core kernels sum partial tiles) that exceeds it is held to 4 x the distance of
    torch's own fp32 CPU result from the fp64 reference on the same inputs instead (the rule of
    test_decoder_chain_with_statistics_summed_by_the_producing_convolution); that distance is computed only when needed."""
    from test_gpu_forward import relerr
    tol = 5 * TOL if c.op == 'bwd_weight' else TOL
    if err < tol or tag not in CHAIN_TAGS:
        return tol
    e32 = relerr(reference(c, torch.float32)[-1][key], ref)
    print('  %s: %.2e exceeds %.1e; torch fp32 on the CPU is %.2e from fp64, bound 4 x that' % (tag, err, tol, e32))
    return max(tol, 4 * e32)


def check_case(c, got, n, valu=False, seen=None):
    """got (run_case) against the fp64 reference and the dispatch table; prints every figure before it asserts"""
    from test_gpu_forward import relerr
    assert not isinstance(got, str), (case_id(c), got)
    want = expected(c, n, not valu and path_open(c))
    tags = [s['tag'] for s in got]
    if seen is not None:
        seen.update(tags)
    assert all(t == want for t in tags), (case_id(c), tags, want)
    ref = reference(c)
    for key in ('y', 'gbias'):
        if key in got[-1]:
            e = relerr(got[-1][key], ref[len(got) - 1][key])
            b = bound(c, key, tags[-1], e, ref[len(got) - 1][key])
            print('%s [%s] %s relerr vs fp64 %.2e (bound %.1e)' % (case_id(c), tags[-1], key, e, b))
            assert e < b, (case_id(c), key, e, b)
    if c.sink:
        for step, (g, r) in enumerate(zip(got, ref)):
            for k in STAT_KEYS:
                e = relerr(g[k], r[k])
                print('  step %d %-6s relerr vs fp64 %.2e' % (step, k, e))
                assert e < 1e-5, (case_id(c), step, k, e)
            assert g['nbt'] == r['nbt']


# ---- the GPODE_CONV_VALU=1 child -------------------------------------------------------------------------------------------------
def decoder_chain(B):
    """The four-stage decoder chain of test_decoder_chain_with_statistics_summed_by_the_producing_convolution, one training step through
    the package's ops: (output, input gradient, parameter gradients, buffers), CPU tensors."""
    import copy
    from vae_gp_ode_amd import vae_ops as V
    d = copy.deepcopy(chain_reference_module()).float().cuda()
    x = chain_input(B).cuda().requires_grad_(True)
    c = V.conv_transpose2d(x, d[0].weight, d[0].bias, 1, 0, stats_for=d[1])
    c = V.bn_relu_conv_transpose2d(c, d[1], d[3].weight, d[3].bias, 2, 1, stats_for=d[4])
    c = V.bn_relu_conv_transpose2d(c, d[4], d[6].weight, d[6].bias, 2, 1, 1, stats_for=d[7])
    y = V.bn_relu_conv_transpose2d(c, d[7], d[9].weight, d[9].bias, 1, 2)
    y.backward(torch.randn(y.shape, generator=torch.Generator().manual_seed(CHAIN_SEEDS[1])).cuda())
    torch.cuda.synchronize()
    return (y.detach().cpu(), x.grad.cpu(), [p.grad.cpu() for p in d.parameters()], [b.cpu() for b in d.buffers()])


# The input seed is chosen on the fp64 reference alone: the first from 20 on with no BatchNorm output (ReLU pre-activation) of the 37
# images within 4e-6 of zero.  fp32 evaluations of that value differ by about 1e-6 between summation orders; where it lies closer to
# zero than that, fp32 and fp64 disagree on the ReLU mask of the element and its whole upstream gradient (0.11 in a bias gradient of
# norm 46 with seed 20, whose closest pre-activation is -1.1e-6: 2.4e-3 in the L2 norm) is the error -- the comparison is then not
# one of the kernels.  The test asserts the margin.
CHAIN_SEEDS = (40, 140)                             # input, grad_output
CHAIN_MARGIN = 4e-6


def chain_input(B):
    return torch.randn(B, 32, 4, 4, generator=torch.Generator().manual_seed(CHAIN_SEEDS[0])) * 0.8


def chain_reference_module():
    g = torch.Generator().manual_seed(5)
    ref = torch.nn.Sequential(torch.nn.ConvTranspose2d(32, 64, 3, 1, 0), torch.nn.BatchNorm2d(64), torch.nn.ReLU(),
                              torch.nn.ConvTranspose2d(64, 32, 5, 2, 1), torch.nn.BatchNorm2d(32), torch.nn.ReLU(),
                              torch.nn.ConvTranspose2d(32, 16, 5, 2, 1, output_padding=1), torch.nn.BatchNorm2d(16), torch.nn.ReLU(),
                              torch.nn.ConvTranspose2d(16, 1, 5, 1, 2))
    with torch.no_grad():
        for m in ref:
            m.double()
            if isinstance(m, torch.nn.ConvTranspose2d):       # a deterministic initialisation (the module's own draws on the global generator)
                m.weight.copy_(torch.randn(m.weight.shape, generator=g, dtype=torch.float64) * (m.weight.shape[0] * m.weight.shape[2] ** 2) ** -0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)      # channel means of the order of the spread
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5); m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
    return ref


@functools.lru_cache(maxsize=None)
def valu_child(n, chain_B=0):
    """Every VALU-mode case (and refusal) in ONE fresh child process under GPODE_CONV_VALU=1: {case: steps | error text}"""
    tmp = tempfile.mkdtemp()
    fn = os.path.join(tmp, 'valu.pt')
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), 'valu', str(n), str(chain_B), fn],
                           env=dict(os.environ, GPODE_CONV_VALU='1'), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return torch.load(fn)
    finally:
        if os.path.exists(fn):
            os.remove(fn)
        os.rmdir(tmp)


def _child_main(n, chain_B, fn):
    sys.path.insert(0, ROOT)
    assert torch.cuda.get_device_properties(0).multi_processor_count == n
    out = {}
    for c in valu_cases(n):
        try:
            out[tuple(c)] = run_case(c)
        except (AssertionError, Refused) as e:       # reported by the parent, per case
            out[tuple(c)] = '%s: %s' % (type(e).__name__, e)
    for c in valu_refusals(n):
        out[('refusal',) + tuple(c)] = refusal(c)
    if chain_B:
        try:
            out['chain'] = decoder_chain(chain_B)
        except Exception as e:                        # the package's own errors (GpodeError) included
            out['chain'] = '%s: %s' % (type(e).__name__, e)
    torch.save(out, fn)


if __name__ == '__main__':
    assert sys.argv[1] == 'valu'
    _child_main(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
