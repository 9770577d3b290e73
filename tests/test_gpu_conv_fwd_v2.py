"""The forward of the second convolution engine (csrc/conv_fwd_v2.hpp) on decnn.7 (ConvTranspose2d 32 -> 16, 13 -> 28, k5 s2 p1,
output_padding 1): producer / consumer wavefronts, weights in registers, tiles of q-positions that span image boundaries.

All four uses, with bias: with / without the fused BatchNorm + ReLU of the input (`in_bn` table) and with / without the statistics of
the output (BnSink), through the C ABI entry points the package calls (gpode_conv2d_bwd_data, gpode_conv2d_bwd_data_bn,
gpode_convT_fwd_stats).  Batch sizes come from the device's CU count n, so they hit the kernel's edges: 1; n + 1 (one workgroup with
two images: a tile spans the image boundary); NBUF n + 1 (the ring of plane buffers wraps in one workgroup); 5 n + 37 (uneven image
counts, a partial last window).

Per case: the output against torch in fp64 on every image (relerr < 2e-5: fp32 accumulation over <= 288 terms, the TOL of
conv_engine_v2.py / test_gpu_vae_layers.py) and against the first engine (GPODE_CONV_V1=1 is read once per process, so it runs in a
child process; same tolerance -- the class split changes nothing per element); with a sink, over two consecutive steps (the second
shifts the sums by the first one's running mean): save_mean, save_invstd, running mean / variance and the table against fp64 at 1e-5,
and BIT-IDENTICAL to the first engine's (the kernel sums them in the first engine's order on purpose: these sums reach every gradient
of a training step, and a training run must not depend on the engine); a second run bit-identical in output and statistics; and every
launch writes into a NaN-filled buffer with guard elements behind it: every element written, nothing past the end.  Which engine ran is
read back from the library (gpode_last_launch), so a dispatch that fell back to the first engine fails the comparison."""
import functools
import os
import shutil
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

from conv_engine_v2 import TOL
from test_gpu_forward import relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBUF = 3                                            # plane buffers of the kernel's ring (FwV2::NBUF)
SIZES = {'one_image': lambda n: 1, 'tile_spans_two_images': lambda n: n + 1, 'ring_wraps': lambda n: NBUF * n + 1,
         'ragged': lambda n: 5 * n + 37}
COMBOS = [(False, False), (True, False), (False, True), (True, True)]      # (in_bn, sink)
MOM, EPS = 0.1, 1e-5

_RUN = r'''
import ctypes, sys, torch
sys.path.insert(0, %r)
from vae_gp_ode_amd import _lib
from vae_gp_ode_amd.ops import _ptr, _stream
GEO = (16, 28, 28, 32, 5, 2, 1, 13, 13)            # the conv geometry of the adjoint: (Ci, H, W, Co, K, S, P, Ho, Wo)
GUARD = 4096

def inputs(B, step):
    """input scales of test_fused_batchnorm_relu_conv_transpose; the in_bn table holds the batch statistics of c (fp64, rounded)"""
    g = torch.Generator().manual_seed(1000 * step + B)
    c = torch.randn(B, 32, 13, 13, generator=g) * 1.3 + 0.2
    gam, bet = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.3
    w, b = torch.randn(32, 16, 5, 5, generator=g) * 0.05, torch.randn(16, generator=g) * 0.1
    gam_out, bet_out = torch.rand(16, generator=g) + 0.5, torch.randn(16, generator=g) * 0.3
    c64 = c.double()
    mean, var = c64.mean((0, 2, 3)), c64.var((0, 2, 3), unbiased=False)
    table = torch.stack([mean, torch.rsqrt(var + 1e-5), gam.double(), bet.double()], 1).float().contiguous()
    return dict(c=c, gam=gam, bet=bet, w=w, b=b, gam_out=gam_out, bet_out=bet_out, table=table)

def launch(c, w, b, table, bn):
    """one launch into a NaN-filled buffer with guard elements behind it; bn = None or the module state the sink updates"""
    B = c.shape[0]
    n = B * 16 * 784
    buf = torch.full((n + GUARD,), float('nan'), device='cuda')
    out = {}
    if bn is None:
        if table is None:
            _lib.call('gpode_conv2d_bwd_data', _ptr(c), _ptr(w), _ptr(b), _ptr(buf), B, *GEO, _stream())
        else:
            _lib.call('gpode_conv2d_bwd_data_bn', _ptr(c), _ptr(table), _ptr(w), _ptr(b), _ptr(buf), B, *GEO, _stream())
    else:
        mean, invstd, tab = (torch.full(s, float('nan'), device='cuda') for s in ((16,), (16,), (16, 4)))
        scratch = torch.empty(int(_lib.load().gpode_convT_fwd_stats_scratch(16)), device='cuda')
        _lib.call('gpode_convT_fwd_stats', _ptr(c), _ptr(table), _ptr(w), _ptr(b), _ptr(buf), B, *GEO, _ptr(bn['gam']), _ptr(bn['bet']),
                  _ptr(mean), _ptr(invstd), _ptr(bn['rm']), _ptr(bn['rv']), _ptr(bn['nbt']), ctypes.c_float(0.1), ctypes.c_float(1e-5),
                  _ptr(tab), _ptr(scratch), 5, _stream())
        torch.cuda.synchronize()
        out = dict(mean=mean.cpu(), invstd=invstd.cpu(), table=tab.cpu(), rm=bn['rm'].cpu().clone(), rv=bn['rv'].cpu().clone(),
                   nbt=int(bn['nbt']))
    torch.cuda.synchronize()
    assert not torch.isnan(buf[:n]).any(), 'output elements left unwritten'
    assert torch.isnan(buf[n:]).all(), 'wrote past the end of the output'
    out['y'] = buf[:n].view(B, 16, 28, 28).cpu()
    out['launcher'] = _lib.load().gpode_last_launch().decode()     # which engine the entry point dispatched to
    return out

def run_case(B, in_bn, sink):
    """the steps of one case (two with a sink, else one): per step the statistics, and the output of the last step"""
    bn, steps = None, []
    for step in range(2 if sink else 1):
        d = {k: v.cuda() for k, v in inputs(B, step).items()}
        if sink and bn is None:
            bn = dict(gam=d['gam_out'], bet=d['bet_out'], rm=torch.zeros(16, device='cuda'), rv=torch.ones(16, device='cuda'),
                      nbt=torch.zeros((), dtype=torch.long, device='cuda'))
        steps.append(launch(d['c'], d['w'], d['b'], d['table'] if in_bn else None, bn))
    for s in steps[:-1]:
        del s['y']
    return steps
''' % ROOT
exec(_RUN)


def _batch(size):
    return SIZES[size](torch.cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=None)
def second_engine(B, in_bn, sink):
    return run_case(B, in_bn, sink)


@functools.lru_cache(maxsize=None)
def first_engine(B):
    """all four cases of a batch size on the first engine, in one child process"""
    tmp = tempfile.mkdtemp()
    fn = os.path.join(tmp, 'v1.pt')
    code = _RUN + r'''
B = int(sys.argv[1])
torch.save({(i, s): run_case(B, i, s) for i in (False, True) for s in (False, True)}, sys.argv[2])
'''
    r = subprocess.run([sys.executable, '-c', code, str(B), fn], env=dict(os.environ, GPODE_CONV_V1='1'), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = torch.load(fn)
    shutil.rmtree(tmp)
    return out


@functools.lru_cache(maxsize=None)
def reference(B, in_bn):
    """torch in fp64 on every image, both steps: output, and the statistics a BatchNorm2d in training mode behind it would hold"""
    steps, rm, rv = [], torch.zeros(16, dtype=torch.float64), torch.ones(16, dtype=torch.float64)
    for step in range(2):
        d = {k: v.double() for k, v in inputs(B, step).items()}
        x = F.relu(F.batch_norm(d['c'], None, None, d['gam'], d['bet'], True, MOM, EPS)) if in_bn else d['c']
        y = F.conv_transpose2d(x, d['w'], d['b'], stride=2, padding=1, output_padding=1)
        n = B * 784
        mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
        rm, rv = (1 - MOM) * rm + MOM * mean, (1 - MOM) * rv + MOM * var * n / (n - 1)
        invstd = torch.rsqrt(var + EPS)
        g0 = inputs(B, 0)
        steps.append(dict(y=y, mean=mean, invstd=invstd, rm=rm, rv=rv, nbt=step + 1,
                          table=torch.stack([mean, invstd, g0['gam_out'].double(), g0['bet_out'].double()], 1)))
    return steps


STAT_KEYS = ('mean', 'invstd', 'rm', 'rv', 'table')


@pytest.fixture(scope='module', autouse=True)
def _drop_cached_outputs():
    yield
    for f in (second_engine, first_engine, reference):
        f.cache_clear()


@pytest.mark.parametrize('in_bn,sink', COMBOS)
@pytest.mark.parametrize('size', list(SIZES))
def test_dec7_fwd_v2_against_fp64(size, in_bn, sink):
    B = _batch(size)
    got, ref = second_engine(B, in_bn, sink), reference(B, in_bn)
    e = relerr(got[-1]['y'], ref[len(got) - 1]['y'])
    print('B %d in_bn %d sink %d: output relerr vs fp64 %.2e' % (B, in_bn, sink, e))
    assert e < TOL
    if sink:
        for step, (g, r) in enumerate(zip(got, ref)):
            for k in STAT_KEYS:
                e = relerr(g[k], r[k])
                print('  step %d %-6s relerr vs fp64 %.2e' % (step, k, e))
                assert e < 1e-5, (step, k, e)
            assert g['nbt'] == r['nbt']


@pytest.mark.parametrize('in_bn,sink', COMBOS)
@pytest.mark.parametrize('size', list(SIZES))
def test_dec7_fwd_v2_against_first_engine(size, in_bn, sink):
    B = _batch(size)
    got, v1 = second_engine(B, in_bn, sink), first_engine(B)[(in_bn, sink)]
    # the comparison means something only if the two sides ran different kernels
    assert all(s['launcher'].startswith('conv_v2_dec7_fwd') for s in got), [s['launcher'] for s in got]
    assert all(s['launcher'].startswith('convT_fwd_mfma') for s in v1), [s['launcher'] for s in v1]
    e = relerr(got[-1]['y'], v1[-1]['y'])
    print('B %d in_bn %d sink %d: output relerr vs first engine %.2e' % (B, in_bn, sink, e))
    assert e < TOL
    if sink:
        for step, (g, r) in enumerate(zip(got, v1)):
            for k in STAT_KEYS:
                e = relerr(g[k], r[k])
                print('  step %d %-6s relerr vs first engine %.2e' % (step, k, e))
                assert torch.equal(g[k], r[k]), (step, k, e)
            assert g['nbt'] == r['nbt']


@pytest.mark.parametrize('in_bn,sink', COMBOS)
@pytest.mark.parametrize('size', list(SIZES))
def test_dec7_fwd_v2_two_runs_bit_identical(size, in_bn, sink):
    B = _batch(size)
    a, b = second_engine(B, in_bn, sink), run_case(B, in_bn, sink)
    assert torch.equal(a[-1]['y'], b[-1]['y'])
    for s, t in zip(a, b):
        for k in STAT_KEYS:
            assert (k in s) == sink and (not sink or torch.equal(s[k], t[k])), k
