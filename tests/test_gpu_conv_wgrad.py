"""The weight-gradient engines through gpode_conv2d_bwd_weight[_bn]: convT_wgrad_v2 (csrc/conv_wgrad_v2.hpp: decnn.7 and decnn.4, with
and without the BatchNorm + ReLU table of the layer's input), dec1_wgrad_mfma, dec10_wgrad_mfma and the first engine's convT_wgrad_mfma
(cnn.6, and decnn.1 with a table).

Batch sizes from the CU count n: 1; n + 1 and 2 n + 1 (one workgroup with two, with three images: convT_wgrad_v2's two plane buffers
alternate and buffer 0 is used again); 3 n + 37 ragged; 8 n + 1 where the kernel takes 8 images per group (the loop over groups wraps).
Per case the checks of test_gpu_conv_dispatch.py (conv_dispatch.run_case / check_case): gw against torch.nn.grad.conv2d_weight in fp64
at 1e-4, NaN-filled gw and scratch with guards behind both (the scratch exactly gpode_conv_wgrad_scratch() floats), a second run
bit-identical, and gpode_last_launch() names the engine.  And two more:

  image attribution   grad_output is zero except in ONE image b* of 2 n + 1 (b* = 0, n - 1, n, the last): gw must be the fp64 weight
                      gradient of that image alone, at 1e-4 relative to that one-image result -- a dropped, doubled or mis-buffered
                      image is then the whole error (in a Gaussian batch it is a 1 / sqrt(B) part of the signal).  With a table the
                      layer's input stays dense: ReLU(BN(.)) of the other images must not leak in.
  deferred reduction  the same launch between gpode_defer_reductions(1) .. (0) followed by gpode_flush_reductions gives a bit-identical
                      gw (and nothing is reduced before the flush).

The parametrisation ids show the batch sizes of a device with 256 CUs; the sizes used come from the device."""
import pytest
import torch

import conv_dispatch as D
from test_gpu_forward import relerr

pytestmark = pytest.mark.gpu
N0 = 256
ENGINES = [('dec7', False), ('dec7', True), ('dec4', False), ('dec4', True), ('dec1', False), ('dec1', True), ('dec10', False),
           ('dec10', True), ('cnn6', False)]
TAGS = {'dec7': 'convT_wgrad_v2', 'dec4': 'convT_wgrad_v2', 'dec10': 'dec10_wgrad_mfma', 'cnn6': 'convT_wgrad_mfma'}


def _n():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _tag(layer, in_bn):
    return TAGS.get(layer, 'convT_wgrad_mfma' if in_bn else 'dec1_wgrad_mfma')


def edge_cases(n):
    out = []
    for layer, in_bn in ENGINES:
        sizes = (1, n + 1, 2 * n + 1, 3 * n + 37) + ((8 * n + 1,) if _tag(layer, in_bn) == 'convT_wgrad_mfma' else ())
        out += [D.Case(layer, 'bwd_weight', B, in_bn) for B in sizes]
    return out


def attribution_cases(n):
    B = 2 * n + 1
    return [(D.Case(layer, 'bwd_weight', B, in_bn), b) for layer, in_bn in ENGINES for b in (0, n - 1, n, B - 1)]


def _param(cases, ids):
    return pytest.mark.parametrize('i', range(len(cases)), ids=ids)


@_param(edge_cases(N0), [D.case_id(c) for c in edge_cases(N0)])
def test_wgrad_engine_edges(i):
    n = _n()
    c = edge_cases(n)[i]
    got = D.run_case(c)
    assert got[0]['tag'] == _tag(c.layer, c.in_bn), got[0]['tag']      # the engine is the kernel that ran
    D.check_case(c, got, n)


@_param(attribution_cases(N0), ['%s-image%d' % (D.case_id(c), b) for c, b in attribution_cases(N0)])
def test_wgrad_image_attribution(i):
    n = _n()
    c, b = attribution_cases(n)[i]
    d = D.device_inputs(c)
    keep = d['x'][b].clone()
    d['x'].zero_()
    d['x'][b] = keep
    got = D.launch(c, d)
    assert got['tag'] == _tag(c.layer, c.in_bn), got['tag']
    ref = D.reference(c, only=b)[0]['y']
    e = relerr(got['y'], ref)
    print('%s image %d: relerr vs the fp64 gradient of that image alone %.2e' % (D.case_id(c), b, e))
    assert e < 5 * D.TOL, e


@pytest.mark.parametrize('layer,in_bn', ENGINES)
def test_wgrad_deferred_reduction_is_bit_identical(layer, in_bn):
    n = _n()
    c = D.Case(layer, 'bwd_weight', 2 * n + 1, in_bn)
    d = D.device_inputs(c)
    now, later = D.launch(c, d), D.launch(c, d, deferred=True)
    assert now['tag'] == _tag(layer, in_bn) and torch.equal(now['y'], later['y'])
