"""The second convolution engine (csrc/conv_bwd_v2.hpp) on decnn.4's input gradient (gpode_conv2d_fwd at the conv geometry 32 -> 64
channels, 13 -> 6, k5 s2 p1): one consumer wavefront per SIMD with 200 weight registers, windows of 64 pixels that span up to three
images, five plane buffers.  Checked at batch sizes that leave one image per workgroup (1, 37), two images and a partial last window
(512) and several images per workgroup (4096, 8192) against torch in fp64, against the first engine (GPODE_CONV_V1=1, read once per
process, so it runs in a child process: the summation order is the same, so the result is bit-identical) and for run-to-run
determinism."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

from test_gpu_forward import relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5
SIZES = [1, 37, 512, 4096, 8192]

_RUN = r'''
import sys, torch
sys.path.insert(0, %r)
from vae_gp_ode_amd import _lib
from vae_gp_ode_amd.ops import _ptr, _stream
def run(gy, w):
    B = gy.shape[0]
    gx = torch.empty(B, 64, 6, 6, device='cuda')
    _lib.call('gpode_conv2d_fwd', _ptr(gy), _ptr(w), _ptr(None), _ptr(gx), B, 32, 13, 13, 64, 5, 2, 1, 6, 6, _stream())
    torch.cuda.synchronize()
    return gx
''' % ROOT
exec(_RUN)


def inputs(B, seed=0):
    g = torch.Generator().manual_seed(seed + B)
    return torch.randn(B, 32, 13, 13, generator=g), torch.randn(64, 32, 5, 5, generator=g) * 0.05


def ref64(gy, w, idx):
    return F.conv2d(gy[idx].double(), w.double(), stride=2, padding=1)


@pytest.mark.parametrize('B', SIZES)
def test_dec4_bwd_data_v2_against_fp64_and_first_engine(B):
    gy, w = inputs(B)
    gx = run(gy.cuda(), w.cuda()).cpu()
    idx = torch.arange(B) if B <= 512 else torch.cat([torch.arange(256), torch.arange(B - 256, B)])
    assert relerr(gx[idx], ref64(gy, w, idx)) < TOL
    fn = os.path.join(tempfile.mkdtemp(), 'v1.pt')
    code = _RUN + r'''
gy, w = torch.load(sys.argv[1])
torch.save(run(gy.cuda(), w.cuda()).cpu(), sys.argv[2])
'''
    src = os.path.join(os.path.dirname(fn), 'in.pt')
    torch.save((gy, w), src)
    r = subprocess.run([sys.executable, '-c', code, src, fn], env=dict(os.environ, GPODE_CONV_V1='1'), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    v1 = torch.load(fn)
    assert torch.equal(gx, v1)


@pytest.mark.parametrize('B', [37, 4096])
def test_dec4_bwd_data_v2_deterministic(B):
    gy, w = inputs(B, seed=7)
    gy, w = gy.cuda(), w.cuda()
    a, b = run(gy, w), run(gy, w)
    assert torch.equal(a, b)


def test_dec4_bwd_data_v2_writes_only_its_output():
    """Every element of gx is written (NaN-filled buffer), and nothing past it (guard elements behind the last image)."""
    B = 300
    gy, w = inputs(B, seed=3)
    gyd, wd = gy.cuda(), w.cuda()
    buf = torch.full((B * 64 * 36 + 4096,), float('nan'), device='cuda')
    _lib.call('gpode_conv2d_fwd', _ptr(gyd), _ptr(wd), _ptr(None), _ptr(buf), B, 32, 13, 13, 64, 5, 2, 1, 6, 6, _stream())
    torch.cuda.synchronize()
    gx = buf[:B * 64 * 36].view(B, 64, 6, 6).cpu()
    assert not torch.isnan(gx).any()
    assert torch.isnan(buf[B * 64 * 36:]).all()
    assert relerr(gx, ref64(gy, w, torch.arange(B))) < TOL
