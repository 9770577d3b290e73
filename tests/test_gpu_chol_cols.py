"""k_chol_rl4 (four block columns of the blocked Cholesky per launch, csrc/gp_cache.hip) against the two-column chain it replaces.

Every remainder of the dispatch -- 4, 5, 6, 7, 8, 9 and 19 block columns: rl4; rl4 + rl; rl4 + rl2; rl4 + rl2 + rl; 2 rl4; 2 rl4 + rl;
4 rl4 + rl2 + rl -- which between them hold every way the rows {k .. k+3, i, j} of a workgroup coincide, with one, two and six
systems on grid.y, through gpode_compute_nu on matrices the test makes itself; one cache build with two Monte-Carlo draws (two
right-hand-side rows).  chol_cols.py runs all of them twice in ONE child process per dispatch (the switch is read once per process).

Per case:
  (a) Lu (with its right-hand-side row), nu and the status words (flag, smallest and largest diagonal entry) of the default dispatch
      equal those under GPODE_CHOL_COLS=2 bit for bit;
  (b) the relative residual of L L^T against the factored matrix, in fp64 on the host, is at most 4 x that of torch.linalg.cholesky in
      fp32 on the CPU for the same matrix (the margin of test_gpu_backward.py).  The reference's own residual must stay below
      n eps(fp32), the first-order bound of the backward error of a Cholesky factorisation: the inputs are well conditioned;
  (c) a matrix whose first non-positive pivot lies in the third or the fourth column of an rl4 launch raises the same GpodeError
      under both dispatches;
  (d) the second run of the default dispatch is bit-identical to the first.

Measured on an MI355X: residuals 1.09e-7 .. 1.18e-7 against 7.4e-8 .. 1.0e-7 of torch on the compute_nu cases, 1.78e-7 against 6.6e-8 on the
two-draw build (whose matrix the library evaluates on its own in fp32); the module takes 6 s, both child processes included."""
import pytest
import torch

import chol_cols as C

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -23


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def runs(mode, name):
    got = C.child(mode)[name]
    assert not isinstance(got, str), (mode, name, got)
    return got


def check_bits(name):
    (a, a2), (b, _) = runs('cols4', name), runs('cols2', name)
    print('%s: %s | %s; status %s | %s' % (name, a['tag'], b['tag'], a['info'].tolist(), b['info'].tolist()))
    assert a['tag'] == b['tag']
    assert a['error'] == b['error'] == 'ok', (a['error'], b['error'])
    assert not (a['info'][0] & 1)
    differs = [k for k in ('Lu', 'nu', 'info') if not same(a[k], b[k])]
    assert not differs, (name, 'default against GPODE_CHOL_COLS=2', differs)                               # (a)
    again = [k for k in ('Lu', 'nu', 'info') if not same(a[k], a2[k])]
    assert not again, (name, 'second run', again)                                                          # (d)
    return a


def check_residual(name, L, A):
    ref = torch.linalg.cholesky(A)
    r_hip, r_ref = C.residual(L, A), C.residual(ref, A)
    n = A.shape[-1]
    print('%s: residual hip %.3e, torch fp32 %.3e (n eps %.1e)' % (name, r_hip, r_ref, n * EPS32))
    assert r_ref < n * EPS32, ('the inputs are not well conditioned', name, r_ref)
    assert r_hip <= 4 * r_ref, (name, r_hip, r_ref)                                                        # (b)


@pytest.mark.parametrize('name', C.GOOD)
def test_four_columns_equal_two(name):
    a = check_bits(name)
    n = C.geometry(C.NU_CASES[name])[0]
    assert a['tag'] == 'kern.compute_nu: chain32+deep'
    check_residual(name, a['Lu'][:, :n, :n], C.factored_matrix(name))


def test_two_draws():
    a = check_bits('build')
    assert a['tag'] == 'cache build: chain32+deep'
    assert a['nu'].shape[0] == C.BUILD_CASE[4]
    check_residual('build', a['Lu'], C.build_matrix())


@pytest.mark.parametrize('name', C.BAD)
def test_not_positive_definite(name):
    (a, a2), (b, _) = runs('cols4', name), runs('cols2', name)
    print('%s: %r | %r; flag %d | %d' % (name, a['error'], b['error'], a['info'][0], b['info'][0]))
    assert a['error'].startswith('GpodeError') and 'not positive-definite' in a['error']
    assert a['error'] == b['error'] == a2['error']                                                         # (c)
    assert a['info'][0] == b['info'][0] == a2['info'][0] and a['info'][0] & 1
