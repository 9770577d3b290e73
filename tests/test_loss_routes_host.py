"""CPU-only checks of loss_routes.py, the helper of test_gpu_loss_routes.py: the case tables reach every tag without duplicates, the
restated dispatch sits on the right side of every threshold and equals the library's two host-only entry points, every fp64 reference
agrees with a second, independent formulation, the inputs meet the conditions the bounds rest on, and the reference expressions
evaluated in fp32 stay within a quarter of their bounds -- so a kernel that misses a bound is wrong, not unlucky."""
import numpy as np
import pytest
import torch

import loss_routes as R


def test_case_tables_have_no_duplicates_and_reach_every_tag():
    cases = R.all_cases()
    assert len(set(cases)) == len(cases) and len(set(map(R.case_id, cases))) == len(cases)
    tags = set()
    for c in cases:
        tags.update(R.expected(c).values())
    assert tags == set(R.REQUIRED_TAGS)
    for table in (R.linear_fwd_cases, R.linear_relu_fwd_cases, R.linear_bwd_cases, R.linear_relu_bwd_cases, R.elementwise_cases, R.sll_cases,
                  R.glue_cases, R.elbo_cases, R.elbo_all_cases, R.adam_cases, R.linear_refusals, R.sll_refusals):
        t = table()
        assert t and len(set(t)) == len(t), table.__name__
    for c in R.linear_refusals():
        assert R.linear_refused(c.op, c.B, c.In, c.Out)
    for c in R.linear_relu_fwd_cases() + R.linear_relu_bwd_cases():
        assert R.linear_refused(c.op, c.B, c.In, c.Out) is None
    assert all(R.sll_refused(c) for c in R.sll_refusals()) and not any(R.sll_refused(c) for c in R.sll_cases())


def test_no_tensor_of_a_case_exceeds_the_size_limit():
    limit = 2 ** 22 + 1024
    for c in R.all_cases():
        if isinstance(c, R.Lin):
            assert max(c.B * c.In, c.B * c.Out, c.Out * c.In, R.linear_bwd_scratch(c.B, c.In, c.Out) if c.scratch else 0) <= limit, c
        elif isinstance(c, R.Ew):
            assert c.n <= limit and c.n % c.reps == 0 and c.n % c.inner == 0, c
        elif isinstance(c, R.Sll):
            assert c.rows * c.inner <= limit and (c.rows * c.inner) % c.nX == 0, c
        elif isinstance(c, R.EA):
            assert c.M * (c.M + 1) // 2 * c.Do <= limit and (c.entry == 'svgp' or c.nl_values % c.ns == 0), c
        elif isinstance(c, R.Adam):
            assert sum(c.sizes) <= limit


def test_restated_dispatch_at_every_threshold():
    f, b = R.linear_fwd_tag, R.linear_bwd_tag
    assert f(256, 16, 64) == 'linear_fwd_fanout' and f(255, 16, 64) == 'linear_fwd' and f(256, 17, 64) == 'linear_fwd'
    assert f(256, 16, 65) == 'linear_fwd' and f(256, 16, 576) == 'linear_fwd_fanout' and f(256, 16, 1024) == 'linear_fwd_fanout'
    assert f(3, 128, 7) == 'linear_fwd_fanin' and f(3, 127, 7) == 'linear_fwd'
    assert f(4096, 128, 1024) == 'linear_fwd_fanin' and f(4097, 128, 1024) == 'linear_fwd'
    assert b(256, 16, 512, True) == 'linear_bwd_fanout' and b(255, 16, 512, True) == 'linear_bwd' and b(256, 17, 512, True) == 'linear_bwd'
    assert b(256, 16, 576, True) == 'linear_bwd' and b(256, 16, 65, True) == 'linear_bwd'
    assert b(1024, 8, 64, True) == 'linear_bwd_fanout (row slabs)' and b(1023, 8, 64, True) == 'linear_bwd_fanout'
    assert b(1024, 9, 64, True) == 'linear_bwd_fanout' and b(1024, 8, 64, False) == 'linear_bwd_fanout'
    assert b(1024, 8, 64, True, gw=False) == 'linear_bwd_fanout' and b(1024, 8, 576, True) == 'linear_bwd'
    assert R.linear_refused('relu_fwd', 3, 127, 7) and not R.linear_refused('relu_fwd', 3, 128, 7)
    assert R.linear_refused('relu_fwd', 4097, 128, 1024) and not R.linear_refused('relu_fwd', 4096, 128, 1024)
    assert R.linear_refused('relu_bwd', 3, 127, 7) and not R.linear_refused('relu_bwd', 4097, 128, 1024)
    assert not R.us_in_parts(147, 6) and R.us_in_parts(148, 6) and 147 * 148 // 2 * 6 == 65268 and 148 * 149 // 2 * 6 == 66156
    assert not R.us_in_parts(361, 1) and R.us_in_parts(362, 1)
    assert [R.ew_grid(n) for n in (0, 1, 256, 257, 2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1)] == [1, 1, 1, 2, 8192, 8192, 8192]
    assert [R.adam_grid(n, True) for n in (1, 2048 * 256, 2048 * 256 + 1, 2 ** 22)] == [1, 2048, 2048, 2048]
    assert [R.adam_grid(n, False) for n in (2048 * 256 + 1, 8192 * 256, 8192 * 256 + 1)] == [2049, 8192, 8192]
    S = R.Sll
    assert R.sll_vector_path(S(3, 8, 8, 0, 'unit', '')) and not R.sll_vector_path(S(3, 8, 8, 0, 'unit', 'a'))
    assert not R.sll_vector_path(S(3, 1023, 1023, 0, 'unit', '')) and not R.sll_vector_path(S(3, 4, 6, 0, 'unit', ''))
    assert R.sll_chunk(S(3, 8, 8, 5, 'unit', '')) == 4 and R.sll_chunk(S(1, 1028, 1028, 64, 'unit', '')) == 20
    # the tables hold both paths, the three proposals (1, several, 64) and a caller's larger count
    cases = R.sll_cases()
    assert {R.sll_vector_path(c) for c in cases} == {True, False}
    ns = {R.sigmoid_loglik_splits(c.rows, c.inner) for c in cases if not c.nsplit}
    assert 1 in ns and 64 in ns and ns & set(range(2, 64))


def test_restated_host_entry_points_equal_the_library():
    from vae_gp_ode_amd import _lib
    lib = _lib.load()
    for inner in (0, 1, 4, 1023, 1024, 1025, 3136, 12544, 65535, 65536, 65537, 10 ** 7):
        for rows in range(0, 3001):
            assert lib.gpode_sigmoid_loglik_splits(rows, inner) == R.sigmoid_loglik_splits(rows, inner), (rows, inner)
    assert lib.gpode_sigmoid_loglik_splits(0, 0) == 1 and lib.gpode_sigmoid_loglik_splits(0, 3136) == 1
    assert lib.gpode_sigmoid_loglik_splits(65535, 10 ** 7) == 1 and lib.gpode_sigmoid_loglik_splits(1, 10 ** 7) == 64
    for B, In, Out in ((1, 1, 1), (1024, 8, 512), (4097, 128, 1024), (255, 17, 65)):
        assert lib.gpode_linear_bwd_scratch(B, In, Out) == R.linear_bwd_scratch(B, In, Out)


def _close(a, b, tol=1e-12):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item() < tol


def test_logit_gradient_reference_is_the_closed_form():
    """d/da of the Bernoulli term under z = sigmoid(a) is X - z"""
    for c in (R.Ew('sll_bwd', 3 * 784, 1, 784), R.Ew('sll_bwd', 255, 3, 85)):
        d, ref = R.inputs(c), R.reference(c)['ga'][0]
        X, z, grow = d['X'].double().repeat(c.reps), d['z'].double(), d['grow'].double()
        # the reference differentiates with respect to z and multiplies by z (1 - z); the closed form needs no division by z
        assert _close(ref, grow.repeat_interleave(c.inner) * (X - z), 1e-10)
    c = R.ea('all_ll', nl_values=40, ns=4, hv=True)
    d, r = R.inputs(c), R.reference(c)
    gl = r['glrow'][0][0]
    assert _close(r['ga'][0], gl * (d['X'].double().repeat(d['z'].numel() // d['X'].numel()) - d['z'].double()), 1e-10)
    assert _close(r['glrow'][0], torch.full((10,), (-R.SEED_VALUES[0] * R.NOBS - R.SEED_VALUES[1]) / 10, dtype=torch.float64))


def test_kl_reference_is_the_written_out_form():
    d = R.inputs(R.Glue('normal_kl', 43, 6, False, ''))
    mu, lv = d['mu'].double(), d['logvar'].double()
    assert _close(R.normal_kl(mu, lv), 0.5 * (lv.exp() + mu * mu - 1 - lv))
    r = R.reference(R.Glue('normal_kl', 43, 6, False, ''))
    assert _close(r['gmu'][0], d['grow'].double()[:, None] * mu) and _close(r['glogvar'][0], d['grow'].double()[:, None] * 0.5 * (lv.exp() - 1))


@pytest.mark.parametrize('M,Do,form', [(1, 1, 'tril'), (7, 3, 'tril'), (100, 6, 'tril'), (100, 6, 'qdiag')])
def test_kl_u_reference_is_the_dense_form(M, Do, form):
    """oracle.svgp_kl on the packed triangles against KL(N(Um, L L^T) || N(0, I)) from dense factors, with its autograd"""
    c = R.ea('svgp', M, Do, form)
    d, r = R.inputs(c), R.reference(c)
    Um, Us = d['Um'].double().requires_grad_(True), d['Us'].double().requires_grad_(True)
    rr, cc = np.tril_indices(M)
    L = torch.zeros(Do, M, M, dtype=torch.float64)
    L[:, torch.as_tensor(rr), torch.as_tensor(cc)] = Us
    cov = L @ L.transpose(1, 2)
    kl = 0.5 * (torch.diagonal(cov, dim1=1, dim2=2).sum() + (Um * Um).sum() - M * Do - torch.logdet(cov).sum())
    dUm, dUs = torch.autograd.grad(kl, (Um, Us), d['g'].double()[0])
    assert _close(r['kl'][0], kl.detach().reshape(1), 1e-9) and _close(r['dUm'][0], dUm, 1e-9)
    di = R.diag_index(M)
    assert _close(r['dUs_diag'][0], dUs[:, di], 1e-7)
    if M > 1:
        off = torch.ones(Us.shape[1], dtype=torch.bool)
        off[di] = False
        if form == 'qdiag':
            assert bool((r['dUs_off'][0] == 0).all())
        else:
            assert _close(r['dUs_off'][0], dUs[:, off], 1e-7)
    assert (R.svgp_kl_terms_abs(Um.detach(), Us.detach(), M) >= kl.detach().abs()).item()


def test_loss_algebra_reference():
    out = R.elbo_algebra(torch.tensor(-300.0), torch.tensor(4.0), torch.tensor(12.5), 360.0)
    assert out.tolist() == [300.0 * 360 + 4 * 360 + 12.5, 300.0, 4.0, 12.5]


def test_inputs_meet_the_conditions_of_the_bounds():
    for c in R.all_cases():
        d = R.inputs(c)
        if isinstance(c, (R.Ew, R.Sll)):
            a = d['a']
            assert a.abs().max() <= R.A_MAX
            z = d['z'] if 'z' in d else torch.sigmoid(a)
            assert (1 - z).min() >= R.MIN_1MZ and z.min() >= R.MIN_1MZ, R.case_id(c)
        if isinstance(c, R.EA) and 'z' in d:
            assert (1 - d['z']).min() >= R.MIN_1MZ and d['z'].min() >= R.MIN_1MZ
        if isinstance(c, R.Lin) and c.op.startswith('relu'):
            assert d['x'].abs().min() >= R.MIN_PRE
        if isinstance(c, R.Adam):
            assert d['p'].abs().max() < 1.0 and len(d['grads']) == R.ADAM_STEPS


def _big(c):
    return (isinstance(c, R.Ew) and c.n > 2 ** 20) or (isinstance(c, R.Sll) and c.rows * c.inner > 2 ** 20) or \
        (isinstance(c, R.Lin) and c.B > 4000) or (isinstance(c, R.Adam) and sum(c.sizes) > 2 ** 20)


def test_fp32_evaluation_of_every_reference_is_within_a_quarter_of_its_bound():
    """what the inputs leave to the kernels: the plain torch expression in fp32 against the same in fp64 (the largest case of each
    family once, the rest in full)"""
    worst = {}
    seen_big = set()
    for c in R.all_cases():
        if _big(c):
            key = (type(c), getattr(c, 'op', None))
            if key in seen_big:
                continue
            seen_big.add(key)
        lo = {k: v[0] for k, v in R.reference(c, torch.float32).items()}
        for key, (e, tol, _) in R.errors(c, lo).items():
            k = (type(c).__name__, key)
            if k not in worst or e / tol > worst[k][0] / worst[k][1]:
                worst[k] = (e, tol, R.case_id(c))
    print({k: '%.1e of %.0e' % v[:2] for k, v in sorted(worst.items())})
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1] / 4}
    assert not bad, bad


def test_adam_update_bound_against_an_fp32_emulation():
    """p_new - p_old of the fp32 emulation (1 - pow(beta, t) formed in fp32, as the kernel forms it) against the fp64 update: inside the
    bound at t = 1, 2, 3, while a step count off by one or a missing square root is off by orders of magnitude more"""
    d = R.inputs(R.Adam((300,), False))
    hi, lo = R.adam_reference(d['p'], d['grads']), R.adam_reference(d['p'], d['grads'], torch.float32)
    prev = d['p'].double()
    for t in (1, 2, 3):
        upd = lo[t - 1][0].double() - prev
        prev = lo[t - 1][0].double()
        err = (upd - hi[t - 1][3]).abs().max().item()
        assert err <= R.adam_update_bound(t) / 2, (t, err, R.adam_update_bound(t))
        off_by_one = hi[t - 1][3] * (1 - R.BETA1 ** t) / (1 - R.BETA1 ** (t + 1))
        assert (off_by_one - hi[t - 1][3]).abs().max().item() > 1e3 * R.adam_update_bound(t)
    assert R.adam_update_bound(1) == pytest.approx(1e-2 * 2.0 ** -23 * (10 + 1000 + 8), rel=1e-4)
