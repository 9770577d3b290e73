"""Checks of the second convolution engine (csrc/conv_bwd_v2.hpp), shared by test_gpu_conv_engine_v2.py (decnn.7) and
test_gpu_conv_engine_v2_dec4.py (decnn.4): the layer's input gradient (gpode_conv2d_fwd at its conv geometry, k5 s2 p1) against
torch in fp64, against the first engine (GPODE_CONV_V1=1, read once per process, so it runs in a child process) and for
run-to-run determinism."""
import os
import subprocess
import sys
import tempfile

import torch
import torch.nn.functional as F

from test_gpu_forward import relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5
SIZES = [1, 37, 512, 4096, 8192]
# layer: (channels in, height in, channels out, height out) of the conv geometry, first-engine comparison bit-identical
LAYERS = {'dec7': (16, 28, 32, 13, False), 'dec4': (32, 13, 64, 6, True)}

_RUN = r'''
import sys, torch
sys.path.insert(0, %r)
from vae_gp_ode_amd import _lib
from vae_gp_ode_amd.ops import _ptr, _stream
def launch(gy, w, gx):
    (B, Ci, H, _), Co = gy.shape, w.shape[0]
    Ho = (H + 2 - 5) // 2 + 1
    _lib.call('gpode_conv2d_fwd', _ptr(gy), _ptr(w), _ptr(None), _ptr(gx), B, Ci, H, H, Co, 5, 2, 1, Ho, Ho, _stream())
    torch.cuda.synchronize()
    return Ho
def run(gy, w):
    Ho = (gy.shape[2] + 2 - 5) // 2 + 1
    gx = torch.empty(gy.shape[0], w.shape[0], Ho, Ho, device='cuda')
    launch(gy, w, gx)
    return gx
''' % ROOT
exec(_RUN)


def inputs(layer, B, seed=0):
    Ci, H, Co, _, _ = LAYERS[layer]
    g = torch.Generator().manual_seed(seed + B)
    return torch.randn(B, Ci, H, H, generator=g), torch.randn(Co, Ci, 5, 5, generator=g) * 0.05


def ref64(gy, w, idx):
    return F.conv2d(gy[idx].double(), w.double(), stride=2, padding=1)


def check_against_fp64_and_first_engine(layer, B):
    gy, w = inputs(layer, B)
    gx = run(gy.cuda(), w.cuda()).cpu()
    assert gx.shape[1:] == (LAYERS[layer][2],) + (LAYERS[layer][3],) * 2
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
    if LAYERS[layer][4]:
        assert torch.equal(gx, v1)
    else:
        assert relerr(gx, v1) < TOL


def check_deterministic(layer, B):
    gy, w = inputs(layer, B, seed=7)
    gy, w = gy.cuda(), w.cuda()
    a, b = run(gy, w), run(gy, w)
    assert torch.equal(a, b)


def check_writes_only_its_output(layer):
    """Every element of gx is written (NaN-filled buffer), and nothing past it (guard elements behind the last image)."""
    B = 300
    _, _, Co, Ho, _ = LAYERS[layer]
    gy, w = inputs(layer, B, seed=3)
    n = B * Co * Ho * Ho
    buf = torch.full((n + 4096,), float('nan'), device='cuda')
    assert launch(gy.cuda(), w.cuda(), buf) == Ho
    gx = buf[:n].view(B, Co, Ho, Ho).cpu()
    assert not torch.isnan(gx).any()
    assert torch.isnan(buf[n:]).all()
    assert relerr(gx, ref64(gy, w, torch.arange(B))) < TOL
