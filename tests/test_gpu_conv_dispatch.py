"""Every launch arm of the convolution dispatch (csrc/vae_conv_tiled.hip, csrc/vae_conv.hip), driven through the C ABI
(gpode_conv2d_fwd, gpode_conv2d_bwd_data[_bn], gpode_convT_fwd_stats, gpode_conv2d_bwd_weight[_bn]) on all seven layer geometries
(decnn.1 / 4 / 7 / 10, cnn.0 with 1 and 5 input channels, cnn.3, cnn.6), forward, d/d input and d/d weight, with / without the
BatchNorm + ReLU table of the input and with / without a statistics sink where the arm takes them.  Three modes:

  default    no switch, aligned operands; batch sizes from the CU count n that hit each kernel's edges (conv_dispatch.default_cases)
  VALU       GPODE_CONV_VALU=1 (read once per process): every case in ONE fresh child process, which saves its outputs to a file;
             plus the four-stage decoder chain through the package's ops at 37 images -- the switch must run the training decoder
  unaligned  one operand at a time shifted by one float (data pointer = 4 mod 16) at n + 1 images: the documented fallback gives right
             numbers; plus one fused decoder stage through vae_ops on an unaligned activation

Per case (conv_dispatch.run_case / check_case): the result against torch in fp64 on every image (outputs and input gradients 2e-5,
weight and bias gradients 1e-4: the project's bounds); with a sink the statistics over two consecutive steps at 1e-5; every output in a
NaN-filled buffer with 4096 NaN guard floats behind it, the weight-gradient scratch NaN-filled and exactly gpode_conv_wgrad_scratch()
floats long with a guard of its own; a second run bit-identical; and gpode_last_launch() equal to the arm the dispatch table
(conv_dispatch.expected) names.  Requests the dispatch refuses return non-zero with a message that names the reason and write nothing.
The last test requires the union of the arms seen to cover the whole dispatch.

The parametrisation ids show the batch sizes of a device with 256 CUs; the sizes used come from the device.

Measured on an MI355X (256 CUs), largest relerr against fp64 per arm over all cases: 1.4e-6 (conv_v2_dec4_bwd_data; convT_bwd_data_tiled
1.3e-6, dec10_fwd 1.1e-6, every other arm below 1e-6; weight gradients at most 5.8e-7, convT_wgrad_v2).  No VALU or generic arm came
near its bound, so the 4 x torch-fp32 rule of conv_dispatch.bound() was never invoked (it prints both numbers when it is)."""
import pytest
import torch

import conv_dispatch as D
from test_gpu_forward import relerr

pytestmark = pytest.mark.gpu
N0 = 256                                            # the CU count the ids are written for
CHAIN_B = 37
SEEN = set()                                        # arms that ran, over all modes


def _n():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _param(make):
    cases = make(N0)
    assert len(set(map(D.case_id, cases))) == len(cases)
    return pytest.mark.parametrize('i', range(len(cases)), ids=[D.case_id(c) for c in cases])


def _valu():
    return D.valu_child(_n(), CHAIN_B)


@pytest.fixture(scope='module', autouse=True)
def _drop_child_outputs():
    yield
    D.valu_child.cache_clear()


@_param(D.default_cases)
def test_default_mode(i):
    n = _n()
    c = D.default_cases(n)[i]
    D.check_case(c, D.run_case(c), n, seen=SEEN)


@_param(D.valu_cases)
def test_valu_mode(i):
    n = _n()
    c = D.valu_cases(n)[i]
    D.check_case(c, _valu()[tuple(c)], n, valu=True, seen=SEEN)


@_param(D.unaligned_cases)
def test_unaligned_operand(i):
    n = _n()
    c = D.unaligned_cases(n)[i]
    D.check_case(c, D.run_case(c), n, seen=SEEN)


def _check_refusal(c, msg, n, valu):
    want = D.expected(c, n, not valu and D.path_open(c))
    assert want[0] == 'refused', (D.case_id(c), want)
    print('%s: %s' % (D.case_id(c), msg))
    assert msg is not None, D.case_id(c) + ': served (the table or the sink was ignored)'
    assert want[1] in msg, (D.case_id(c), msg)


@_param(D.default_refusals)
def test_default_mode_refusals(i):
    n = _n()
    c = D.default_refusals(n)[i]
    _check_refusal(c, D.refusal(c), n, False)


@_param(D.unaligned_refusals)
def test_unaligned_refusals(i):
    """a BatchNorm table or a sink with an operand that closes the matrix-core path: an error, not the convolution of the raw input"""
    n = _n()
    c = D.unaligned_refusals(n)[i]
    _check_refusal(c, D.refusal(c), n, False)


@_param(D.valu_refusals)
def test_valu_mode_refusals(i):
    n = _n()
    c = D.valu_refusals(n)[i]
    _check_refusal(c, _valu()[('refusal',) + tuple(c)], n, True)


def test_valu_mode_runs_the_training_decoder():
    """decnn.1 -> BatchNorm -> ReLU -> decnn.4 -> ... -> decnn.10 through vae_ops under GPODE_CONV_VALU=1, one forward and backward at 37
    images: bn_relu_conv_transpose2d takes the separate ops (the VALU kernels have no fused BatchNorm input).  Output, every gradient and
    the running statistics against torch in fp64 with the bounds of
    test_decoder_chain_with_statistics_summed_by_the_producing_convolution."""
    import copy
    got = _valu()['chain']
    assert not isinstance(got, str), got
    y, gx, gps, bufs = got
    l2 = lambda a, b: float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())
    r = D.chain_reference_module()
    r32 = copy.deepcopy(r).float()
    x0 = D.chain_input(CHAIN_B)
    gy0 = torch.randn(y.shape, generator=torch.Generator().manual_seed(D.CHAIN_SEEDS[1]))
    x64, x32 = x0.double().requires_grad_(True), x0.clone().requires_grad_(True)
    h = x64.detach()
    for m in r:                                       # the comparison is well-posed: no ReLU mask hangs on fp32 round-off (conv_dispatch.py)
        assert not isinstance(m, torch.nn.ReLU) or float(h.abs().min()) > D.CHAIN_MARGIN
        with torch.no_grad():
            h = m(h)
    for m in r:
        if isinstance(m, torch.nn.BatchNorm2d):       # (the margin pass above has updated the running statistics)
            m.reset_running_stats()
    y64 = r(x64)
    y64.backward(gy0.double())
    r32(x32).backward(gy0)
    tol = lambda g64, g32: 2e-3 + 4 * l2(g32, g64)
    print('y relerr %.2e, gx l2 %.2e (torch fp32: %.2e)' % (relerr(y, y64), l2(gx, x64.grad), l2(x32.grad, x64.grad)))
    assert relerr(y, y64) < D.TOL and l2(gx, x64.grad) < tol(x64.grad, x32.grad)
    for (name, p64), (_, p32), gp in zip(r.named_parameters(), r32.named_parameters(), gps):
        if name in ('0.bias', '3.bias', '6.bias'):    # a bias in front of a BatchNorm has no gradient: round-off on both sides
            assert float(gp.abs().max()) < 10 * float(p32.grad.abs().max()) + 1e-3 and float(p64.grad.abs().max()) < 1e-9, name
            continue
        print('%s l2 %.2e (torch fp32: %.2e)' % (name, l2(gp, p64.grad), l2(p32.grad, p64.grad)))
        assert l2(gp, p64.grad) < tol(p64.grad, p32.grad), name
    for (name, b64), bf in zip(r.named_buffers(), bufs):
        assert relerr(bf.double(), b64.double()) < 1e-5, name


@pytest.mark.parametrize('geom', [((32, 13, 13), (32, 16, 5, 5), (2, 1, 1)), ((16, 28, 28), (16, 1, 5, 5), (1, 2, 0))], ids=['decnn7', 'decnn10'])
def test_fused_stage_with_an_unaligned_activation(geom):
    """vae_ops.bn_relu_conv_transpose2d on an activation c that starts one float behind a 16-byte boundary (no switch set): the separate
    ops instead of the fused form, no error, and the table is never dropped -- for decnn.10 this is the case in which
    _BnReluConvT.backward used to reach the VALU weight-gradient arm.  The inputs and bounds of
    test_fused_batchnorm_relu_conv_transpose at 37 images: output, running statistics and every gradient against torch in fp64."""
    import torch.nn.functional as F
    from vae_gp_ode_amd import vae_ops as V
    B, ((C, H, _), wshape, (s, p, op)) = 37, geom
    g = torch.Generator().manual_seed(11)
    c = torch.randn(B, C, H, H, generator=g) * 1.3 + 0.2
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    w, b = torch.randn(wshape, generator=g) * 0.05, torch.randn(wshape[1], generator=g) * 0.1
    bn = torch.nn.BatchNorm2d(C).cuda()
    ref = torch.nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.weight.copy_(gam); bn.bias.copy_(bet); ref.weight.copy_(gam); ref.bias.copy_(bet)
    a64 = [t.double().requires_grad_(True) for t in (c, w, b)]
    y64 = F.conv_transpose2d(F.relu(ref(a64[0])), a64[1], a64[2], stride=s, padding=p, output_padding=op)
    gy = torch.randn(y64.shape, generator=g)
    y64.backward(gy.double())
    a = [D._dev(c, shift=True).requires_grad_(True)] + [t.cuda().requires_grad_(True) for t in (w, b)]
    assert a[0].data_ptr() % 16 == 4 and a[0].is_contiguous()
    y = V.bn_relu_conv_transpose2d(a[0], bn, a[1], a[2], s, p, op)
    y.backward(gy.cuda())
    assert relerr(y, y64) < D.TOL
    for x, x64 in zip(a, a64):
        assert relerr(x.grad, x64.grad) < 5 * D.TOL
    assert relerr(bn.weight.grad, ref.weight.grad) < 5 * D.TOL and relerr(bn.bias.grad, ref.bias.grad) < 5 * D.TOL
    assert relerr(bn.running_mean, ref.running_mean) < 1e-5 and relerr(bn.running_var, ref.running_var) < 1e-5
    assert int(bn.num_batches_tracked) == 1


def test_every_arm_was_reached():
    """The union of gpode_last_launch() over the three modes covers every arm of the dispatch (run after the tests above; on its own it
    runs the cases it needs)."""
    n = _n()
    table = {D.expected(c, n, True) for c in D.default_cases(n)} | {D.expected(c, n, False) for c in D.valu_cases(n)}
    assert set(D.REQUIRED_TAGS) <= table, sorted(set(D.REQUIRED_TAGS) - table)
    if not set(D.REQUIRED_TAGS) <= SEEN:
        for tag in sorted(set(D.REQUIRED_TAGS) - SEEN):
            if tag in D.CHAIN_TAGS and tag != 'enc_conv3_bwd_data_tiled':
                c = next(c for c in D.valu_cases(n) if D.expected(c, n, False) == tag)
                SEEN.update(s['tag'] for s in _valu()[tuple(c)])
            else:
                c = next(c for c in D.default_cases(n) if D.expected(c, n, True) == tag)
                SEEN.update(s['tag'] for s in D.run_case(c))
    assert set(D.REQUIRED_TAGS) <= SEEN, sorted(set(D.REQUIRED_TAGS) - SEEN)
