"""The launch chain of the blocked Cholesky (csrc/gp_cache.hip cholesky_blocked, non-panelled branch) under its two dispatches,
shared by test_gpu_chol_cols.py and by the child processes it starts.

  cols4   no switch: k_chol_rl4 while four block columns remain, then k_chol_rl2, then k_chol_rl
  cols2   GPODE_CHOL_COLS=2: k_chol_rl2, then k_chol_rl (the chain before k_chol_rl4)

The switch is read once per process, so every case of a mode runs in ONE fresh child process (`python chol_cols.py <mode> <file>`)
that saves its arrays to a file; both children also carry GPODE_DRAW_CHAIN=1, or a two-draw build of 192 padded rows or fewer would
stay in k_draw_lds.

A `nu` case goes through gpode_compute_nu on a matrix the test makes itself (so the factored matrix is known to the bit: Ku with
fp32(1e-5) added to its diagonal in fp32); the factor is read out of the workspace, whose layout (csrc/gp_ws.hpp) ws_layout()
restates.  A `build` case goes through gpode_cache_build_fwd_n with two Monte-Carlo draws, which append two right-hand-side rows."""
import collections
import ctypes
import functools
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 32
S = 32
MODES = {'cols4': {}, 'cols2': {'GPODE_CHOL_COLS': '2'}}

# kernel, Di, Do, M, bad: bad = the row whose diagonal entry is made negative (None: positive definite)
Nu = collections.namedtuple('Nu', 'kernel Di Do M bad')
NU_CASES = {
    'nblk4': Nu('RBF', 2, 2, 127, None),        # 128 rows: one k_chol_rl4, every workgroup stops early; two systems (grid.y)
    'nblk5': Nu('RBF', 2, 2, 130, None),        # rl4 + rl: one trailing tile, i == j
    'nblk6': Nu('RBF', 2, 2, 191, None),        # rl4 + rl2: trailing tiles with i != j
    'nblk7': Nu('RBF', 6, 6, 192, None),        # np = 224: rl4 + rl2 + rl, six systems
    'nblk8': Nu('RBF', 2, 2, 255, None),        # two rl4
    'nblk9': Nu('RBF', 2, 2, 260, None),        # two rl4 + rl
    'nblk19': Nu('DF', 6, 6, 100, None),        # the flagship's system: 601 rows, rl4 x 4 + rl2 + rl
    'bad_col3': Nu('RBF', 2, 2, 191, 2 * NB + 5),    # first non-positive pivot in the THIRD column of the first rl4 launch
    'bad_col4': Nu('RBF', 2, 2, 260, 7 * NB + 30),   # ... in the FOURTH column of the second rl4 launch
    'bad_col4_df': Nu('DF', 6, 6, 100, 3 * NB + 0),  # ... in the fourth column of the first, 19 block columns
}
GOOD = [k for k, c in NU_CASES.items() if c.bad is None]
BAD = [k for k, c in NU_CASES.items() if c.bad is not None]
BUILD_CASE = ('RBF', 6, 6, 192, 2)               # kernel, Di, Do, M, draws: 194 rows, np = 224


def geometry(c):
    n, batch = (c.M, c.Do) if c.kernel == 'RBF' else (c.M * c.Do, 1)
    nblk = -(-(n + 1) // NB)
    assert nblk < 32                                   # the panelled branch is not what these tests are about
    return n, batch, nblk, NB * nblk


def ws_layout(c):
    """offsets (floats) of Lmat and Dfac in the workspace of gpode_compute_nu: csrc/gp_ws.hpp ws_layout with one draw"""
    n, batch, nblk, np_ = geometry(c)
    o = 0
    at = {}
    for name, nfl in (('info', 4), ('ell', c.Do * c.Di), ('var', c.Do), ('u', c.M * c.Do), ('u_prior', c.M * c.Do), ('nu', batch * n),
                      ('A', batch * np_ * np_), ('Lmat', batch * np_ * np_), ('Dfac', batch * nblk * NB * NB)):
        at[name] = o
        o += (nfl + 3) // 4 * 4
    at['total'] = o
    return at


def nu_inputs(name):
    """(Ku, u_prior, u) of a case, fp32 on the CPU.  Ku = W W^T / n + I / 2 per system (eigenvalues in about [0.5, 4.5]), symmetric to
    the bit; a `bad` case gets -1 at one diagonal entry, which leaves the pivots before it as they were."""
    c = NU_CASES[name]
    n, batch, _, _ = geometry(c)
    g = torch.Generator().manual_seed(4200 + n + 7 * batch)
    W = torch.randn(batch, n, n, generator=g, dtype=torch.float64)
    K = W @ W.transpose(1, 2) / n + 0.5 * torch.eye(n, dtype=torch.float64)
    K = (0.5 * (K + K.transpose(1, 2))).float()
    K = torch.tril(K) + torch.tril(K, -1).transpose(1, 2)
    if c.bad is not None:
        K[:, c.bad, c.bad] = -1.0
    Ku = K if c.kernel == 'RBF' else K[0]
    return Ku.contiguous(), torch.randn(c.M, c.Do, generator=g), torch.randn(c.M, c.Do, generator=g)


def factored_matrix(name):
    """what gpode_compute_nu factors: Ku + fp32(1e-5) I, the sum rounded to fp32 (k_fill_from_K) -> (batch, n, n) fp32"""
    c = NU_CASES[name]
    n, batch, _, _ = geometry(c)
    A = nu_inputs(name)[0].reshape(batch, n, n).clone()
    A.diagonal(dim1=1, dim2=2).add_(torch.tensor(1e-5, dtype=torch.float32))
    return A


def residual(L, A):
    """|| L L^T - A ||_F / || A ||_F in fp64"""
    L, A = L.double(), A.double()
    return float((L @ L.transpose(-1, -2) - A).norm() / A.norm())


# ---- launches (child processes only) -----------------------------------------------------------------------------------------------
def _status(ws):
    """(flag word, bits of the smallest and of the largest diagonal entry, what check_factorisation raises or 'ok')"""
    from vae_gp_ode_amd import _lib, ops
    info = ctypes.c_int(0)
    _lib.call('gpode_cache_info', ops._ptr(ws), ctypes.byref(info), ops._stream())
    mm = (ctypes.c_float * 2)()
    _lib.call('gpode_cache_pivots', ops._ptr(ws), mm, ops._stream())
    k = ops.GPCache()
    k.ws = ws
    try:
        k.check_factorisation()
        err = 'ok'
    except _lib.GpodeError as e:
        err = '%s: %s' % (type(e).__name__, e)
    bits = torch.tensor([mm[0], mm[1]], dtype=torch.float32).view(torch.int32)
    return torch.cat([torch.tensor([info.value], dtype=torch.int32), bits]), err


def run_nu(name):
    from vae_gp_ode_amd import _lib, ops
    c = NU_CASES[name]
    n, batch, nblk, np_ = geometry(c)
    Ku, u_prior, u = (t.cuda() for t in nu_inputs(name))
    nu, ws = ops.compute_nu(c.kernel, c.Di, c.Do, Ku, u_prior, u)
    tag = _lib.load().gpode_last_launch().decode()
    torch.cuda.synchronize()
    at = ws_layout(c)
    assert ws.numel() == at['total'], (ws.numel(), at['total'])
    w = ws.cpu()
    Lm = w[at['Lmat']:at['Lmat'] + batch * np_ * np_].reshape(batch, np_, np_)
    Df = w[at['Dfac']:at['Dfac'] + batch * nblk * NB * NB].reshape(batch, nblk, NB, NB)
    L = torch.zeros(batch, np_, np_)
    for b in range(nblk):                              # tiles below the diagonal from Lmat, the diagonal tiles from Dfac
        L[:, b * NB:(b + 1) * NB, :b * NB] = Lm[:, b * NB:(b + 1) * NB, :b * NB]
        L[:, b * NB:(b + 1) * NB, b * NB:(b + 1) * NB] = Df[:, b]
    info, err = _status(ws)
    return dict(Lu=L[:, :n + 1, :n + 1].clone(), nu=nu.cpu(), info=info, error=err, tag=tag)


def build_inputs():
    from test_gpu_backward import synthetic_gp
    kernel, Di, Do, M, nd = BUILD_CASE
    p, _, _, _, _ = synthetic_gp(kernel, Di, Do, M, S, 4, 3, seed=7100)
    g = torch.Generator().manual_seed(9100)
    nz = dict(eps_u=torch.randn(nd, M, Do, generator=g), rff_w=torch.randn(nd, S, Do, generator=g),
              rff_eps=torch.randn(nd, Di, S, Do, generator=g), rff_u=torch.rand(nd, 1, S, Do, generator=g))
    return p, nz


def run_build():
    from vae_gp_ode_amd import _lib, ops
    kernel, Di, Do, M, nd = BUILD_CASE
    p, nz = build_inputs()
    k = ops.cache_build(kernel, *[p[q].cuda() for q in ('raw_ell', 'raw_var', 'Z', 'Um', 'Us')],
                        *[nz[q].cuda() for q in ('eps_u', 'rff_w', 'rff_eps', 'rff_u')], want_Lu=True)
    tag = _lib.load().gpode_last_launch().decode()
    torch.cuda.synchronize()
    info, err = _status(k.ws)
    return dict(Lu=k.Lu.cpu(), nu=k.nu.cpu(), info=info, error=err, tag=tag)


def build_matrix():
    """K_uu + 1e-5 I of BUILD_CASE from the fp64 oracle, rounded to fp32 -> (Do, M, M).  The library evaluates the kernel in fp32 on
    its own, so its matrix differs from this one by that rounding: the residual of its factor against THIS matrix is the larger for it."""
    from oracle import gpode_oracle as O
    kernel, Di, Do, M, nd = BUILD_CASE
    p, nz = build_inputs()
    cl = O.build_cache(O.to_dtype(p, torch.float64), {q: v[0].double() for q, v in nz.items()}, kernel)
    return (cl['Ku'] + 1e-5 * torch.eye(M, dtype=torch.float64)).float()


# ---- the child processes -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def child(mode):
    """every case in ONE fresh child process with the mode's switch in its environment: {case: [first run, second run] | error text}"""
    tmp = tempfile.mkdtemp()
    fn = os.path.join(tmp, mode + '.pt')
    env = {k: v for k, v in os.environ.items() if k != 'GPODE_CHOL_COLS'}
    env.update(MODES[mode], GPODE_DRAW_CHAIN='1')
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, fn], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return torch.load(fn)
    finally:
        if os.path.exists(fn):
            os.remove(fn)
        os.rmdir(tmp)


def _child_main(mode, fn):
    sys.path.insert(0, ROOT)
    assert os.environ.get('GPODE_CHOL_COLS') == MODES[mode].get('GPODE_CHOL_COLS') and os.environ.get('GPODE_DRAW_CHAIN') == '1'
    out = {}
    for name, run in [(n, functools.partial(run_nu, n)) for n in NU_CASES] + [('build', run_build)]:
        try:
            out[name] = [run(), run()]
        except Exception as e:                        # reported by the parent, per case
            out[name] = '%s: %s' % (type(e).__name__, e)
    torch.save(out, fn)


if __name__ == '__main__':
    _child_main(sys.argv[1], sys.argv[2])
