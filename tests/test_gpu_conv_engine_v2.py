"""The second convolution engine (csrc/conv_bwd_v2.hpp): decnn.7's input gradient (gpode_conv2d_fwd at the conv geometry
16 -> 32 channels, 28 -> 13, k5 s2 p1) on producer / consumer wavefronts with the weights in registers and pixel tiles that span
image boundaries.  Checked at batch sizes that leave one image per workgroup (1, 37), a partial last window (512) and several
images per workgroup (4096, 8192) against torch in fp64, against the first engine (GPODE_CONV_V1=1, read once per process, so it
runs in a child process) and for run-to-run determinism."""
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
    gx = torch.empty(B, 32, 13, 13, device='cuda')
    _lib.call('gpode_conv2d_fwd', _ptr(gy), _ptr(w), _ptr(None), _ptr(gx), B, 16, 28, 28, 32, 5, 2, 1, 13, 13, _stream())
    torch.cuda.synchronize()
    return gx
''' % ROOT
exec(_RUN)


def inputs(B, seed=0):
    g = torch.Generator().manual_seed(seed + B)
    return torch.randn(B, 16, 28, 28, generator=g), torch.randn(32, 16, 5, 5, generator=g) * 0.05


def ref64(gy, w, idx):
    return F.conv2d(gy[idx].double(), w.double(), stride=2, padding=1)


@pytest.mark.parametrize('B', SIZES)
def test_dec7_bwd_data_v2_against_fp64_and_first_engine(B):
    gy, w = inputs(B)
    gx = run(gy.cuda(), w.cuda()).cpu()
    # fp64 on every image up to 512; beyond, on the first and last 256 (the first and last images of every workgroup are among them
    # only for the smaller grids -- the comparison with the first engine below covers every image)
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
    assert relerr(gx, v1) < TOL


@pytest.mark.parametrize('B', [37, 4096])
def test_dec7_bwd_data_v2_deterministic(B):
    gy, w = inputs(B, seed=7)
    gy, w = gy.cuda(), w.cuda()
    a, b = run(gy, w), run(gy, w)
    assert torch.equal(a, b)


def test_dec7_bwd_data_v2_writes_only_its_output():
    """Every element of gx is written (NaN-filled buffer), and nothing past it (guard elements behind the last image)."""
    B = 300
    gy, w = inputs(B, seed=3)
    gyd, wd = gy.cuda(), w.cuda()
    buf = torch.full((B * 32 * 169 + 4096,), float('nan'), device='cuda')
    _lib.call('gpode_conv2d_fwd', _ptr(gyd), _ptr(wd), _ptr(None), _ptr(buf), B, 16, 28, 28, 32, 5, 2, 1, 13, 13, _stream())
    torch.cuda.synchronize()
    gx = buf[:B * 32 * 169].view(B, 32, 13, 13).cpu()
    assert not torch.isnan(gx).any()
    assert torch.isnan(buf[B * 32 * 169:]).all()
    assert relerr(gx, ref64(gy, w, torch.arange(B))) < TOL
