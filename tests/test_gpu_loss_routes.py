"""Every route of the tail of the training step -- csrc/vae_dense.hip, csrc/vae_loss.hip and csrc/vae_optim.hip, plus k_svgp_kl
(csrc/gp_misc.hip) -- driven through the C ABI at the smallest shapes that sit on each edge (loss_routes.py): gpode_linear_fwd / _bwd,
gpode_linear_relu_fwd / _bwd, gpode_act_*, gpode_loglik_*, gpode_loglik_rowsum_*, gpode_sigmoid_loglik_fwd / _bwd, gpode_reparam_*,
gpode_reparam_kl_*, gpode_normal_kl_*, gpode_elbo_fwd / _bwd, gpode_svgp_kl_fwd / _bwd, the five gpode_elbo_all_* entry points,
gpode_adam_multi and gpode_gather_multi; and vae_ops.elbo_all on its three routes.

Per case (loss_routes.launch / check): (a) gpode_last_launch() after every call equals the tag loss_routes.expected names -- a
restatement of the thresholds (In <= 16, Out % 64, Out <= 512, B >= 256, In >= 128, B Out <= 2^22, In <= 8 and B >= 1024 with a scratch,
2^16 packed entries of Us) that never asks the library; (b) outputs and gradients within 2e-5 of plain fp64 torch (autograd) relative to
the largest entry, the reparameterised z within 1e-6, KL rows and the four ELBO outputs within 1e-5 (the bounds of test_gpu_vae_layers
and test_elbo_glue_ops), sums that can cancel -- likelihood row sums, kl_u, the loss -- relative to the fp64 sum of |terms|, Adam's
parameters and moments within 1e-6 after every step and its update within lr 2^-23 (1 / (1 - beta1^t) + 1 / (1 - beta2^t) + 8); (c)
every output and scratch NaN-filled and sized exactly, 4096 guard floats behind each: the guards come back untouched, no NaN is left in
an output, the 256 scratch floats of `out` are written when Us is summed in parts and only then; (d) a second run is bit-identical;
(e) the bit-equalities the sources claim: z of gpode_sigmoid_loglik_fwd = gpode_act_fwd(mode 1), ga of gpode_sigmoid_loglik_bwd =
gpode_loglik_rowsum_bwd -> gpode_act_bwd, ga of gpode_elbo_all_bwd_ll / _bwd_ll_kl = gpode_sigmoid_loglik_bwd on the uniform row
gradient, z of gpode_reparam_kl_fwd = gpode_reparam_fwd, the scalar path of gpode_sigmoid_loglik_fwd = its float4 path in z.  All of
them hold.  Rows of 4 and 8 logits are held to the fp64 terms of the z the kernel returned (loss_routes.sll_short_rows says why).

Measured on an MI355X, largest error per tag over all cases (bound): linear_fwd 6.9e-7, linear_fwd_fanout 2.3e-7, linear_fwd_fanin
1.9e-7, linear_relu_fwd 1.2e-7, linear_bwd 8.5e-7, linear_bwd_fanout 1.8e-7, its row slabs 2.0e-7, linear_relu_bwd 1.6e-7, act_fwd
9.8e-8, act_bwd 9.3e-8, loglik_fwd 1.9e-7, loglik_bwd 1.0e-7, loglik_rowsum 1.3e-7, loglik_rowsum_bwd 1.3e-7, sigmoid_loglik_fwd 6.8e-7,
sigmoid_loglik_bwd 2.3e-7, reparam_bwd 9.2e-8, reparam_kl_bwd 1.5e-7, normal_kl_bwd 7.4e-8, elbo_bwd 3.2e-8, elbo_all_bwd 1.5e-7,
elbo_loglik_bwd 2.5e-7, elbo_loglik_bwd_kl 2.6e-7, svgp_kl_bwd 1.8e-7 (2e-5); reparam_fwd and reparam_kl_fwd 7.1e-8 (1e-6);
normal_kl_fwd 1.3e-7, elbo_fwd 9.7e-8, elbo_all_fwd 1.8e-7, in parts 1.5e-7, elbo_all_fwd_kl 1.6e-7, in parts 1.1e-7, svgp_kl 1.1e-7
(1e-5); adam_multi: parameters and moments 1.4e-7 (1e-6), the update at t = 3 6.3e-8 (4.1e-7).  No guard was written, no NaN of the
fills reached an output, every second run gave the same bits; the module takes 5 s.

Nothing observable tells the scalar path of gpode_sigmoid_loglik_fwd from its float4 path (one tag, the same z): the misaligned cases
show that a misaligned operand gives right results and the parts of empty slices are 0, not that it stays off the vector loads.

Each of these, built into the library once from a scratch copy, turned red exactly what it should (658 tests): (a) B >= 257 in
linear_fwd -- the 13 forward cases with B = 256, In <= 16, Out % 64 == 0, on their tag alone (linear_fwd for linear_fwd_fanout); (b)
acc[8] += gv dropped in k_linear_bwd_w_cols -- the 17 cases on the row-slab route that ask for gb (all eight Out at B = 1027, In = 8,
the In in {1, 8} x B >= 1024 rows of the table, gx NULL), in gb alone; gw NULL (the other route) and gb NULL stay green; (c) kr = t[2] /
nl_rows in k_elbo_all_fwd -- all 81 cases of the three elbo_all forms, in `out`, and the six wrapper routes; gpode_svgp_kl_* green;
(d) the diagonal term dropped in k_elbo_loglik_bwd only -- 42 of the 54 _bwd_ll / _bwd_ll_kl cases, in dUs_diag alone, and the four
fused wrapper routes; green: the 12 with g2 as the only seed (g0 + g3 = 0, so dUs is 0 either way), every gpode_elbo_all_bwd and
gpode_svgp_kl_bwd case and the two wrapper routes on separate row sums; (e) the 2^16 threshold moved to 2^17 -- the three (148, 6)
cases, on their tag alone (elbo_all_fwd / elbo_all_fwd_kl without the suffix): their values still pass, `out` at most 1.5e-7
(1e-5) and every gradient at most 1.4e-7 (2e-5); (f) step = step_dev[0] in k_adam_multi -- the 7 cases with the device-side counter: step_dev reads {0, 0} after each of
the three launches, and with bias correction 0 the update and the parameters are off without bound (inf) at t = 1, 2, 3 while both
moments stay within 9.9e-8 (1e-6); the
host-step cases green; (g) the float4 branch of k_sigmoid_loglik_fwd summing .x .y .z -- all 65 float4 cases in their row sums, none of
the 24 scalar ones, the 12 scalar-against-float4 comparisons, the four fused wrapper routes and the fallback of
_SigmoidLogLikParts.backward."""
import pytest
import torch

import loss_routes as R

pytestmark = pytest.mark.gpu
SEEN = set()
MAXIMA = {}


@pytest.fixture(scope='module', autouse=True)
def _report_and_drop_cached_inputs():
    yield
    print('largest error per tag (bound):', {k: '%.1e (%.0e) %s' % v for k, v in sorted(MAXIMA.items())})
    R.clear_caches()


def _param(cases):
    assert len(set(cases)) == len(cases)
    return pytest.mark.parametrize('c', cases, ids=[R.case_id(c) for c in cases])


def _run(c):
    R.check(c, R.launch(c), SEEN, MAXIMA)


def _refused(c, words):
    got = R.launch(c)
    assert not got['tags'] and words in got['out'].get('refused', ''), (R.case_id(c), got['out'], got['tags'])
    assert got['out']['untouched'] and not got['problems'], (R.case_id(c), 'a refused call wrote an output', got['problems'])


# ---- 1, 2: the dense layers ----------------------------------------------------------------------------------------------------------------
@_param(R.linear_fwd_cases() + R.linear_relu_fwd_cases())
def test_linear_forward(c):
    _run(c)


@_param(R.linear_bwd_cases() + R.linear_relu_bwd_cases())
def test_linear_backward(c):
    _run(c)


@_param(R.linear_refusals())
def test_linear_relu_refuses_narrow_and_oversized_layers(c):
    """non-zero return, gpode_last_error names the entry point, the outputs are still NaN"""
    _refused(c, R.linear_refused(c.op, c.B, c.In, c.Out))


# ---- 3: the elementwise kernels, through the grid-stride loop beyond 8192 workgroups ------------------------------------------------------------
@_param(R.elementwise_cases())
def test_elementwise(c):
    _run(c)


# ---- 4: gpode_sigmoid_loglik_fwd -------------------------------------------------------------------------------------------------------------
@_param(R.sll_cases())
def test_sigmoid_loglik_forward(c):
    _run(c)


@_param([c for c in R.sll_cases() if c.mis])
def test_sigmoid_loglik_scalar_path_equals_the_float4_path(c):
    """a misaligned operand takes the scalar loop: the same z bit for bit, the row sums within 2e-5 of sum |terms| of the aligned call"""
    aligned = c._replace(mis='')
    assert R.sll_vector_path(aligned) and not R.sll_vector_path(c)
    a, b = R.launch(c), R.launch(aligned)
    assert not a['problems'] and not b['problems'] and not a['bits'] and not b['bits']
    assert torch.equal(a['out']['z'].view(torch.int32), b['out']['z'].view(torch.int32)), R.case_id(c)
    scale = R.reference(aligned)['rowsum'][2]
    err = ((a['out']['rowsum'] - b['out']['rowsum']).abs() / scale).max().item()
    print('%s: scalar against float4 row sums %.2e' % (R.case_id(c), err))
    assert err <= R.TOL, (R.case_id(c), err)


@_param(R.sll_refusals())
def test_sigmoid_loglik_forward_refusals(c):
    _refused(c, R.sll_refused(c))


# ---- 5: the separate glue kernels ----------------------------------------------------------------------------------------------------------------
@_param(R.glue_cases())
def test_glue(c):
    _run(c)


@_param(R.elbo_cases())
def test_elbo_terms(c):
    _run(c)


# ---- 6: gpode_svgp_kl_* and the five gpode_elbo_all_* ----------------------------------------------------------------------------------------------
@_param(R.elbo_all_cases())
def test_elbo_all(c):
    _run(c)


# ---- 7: the host wrappers ----------------------------------------------------------------------------------------------------------------------------
def _recorded(monkeypatch):
    """every _lib.call of the wrappers with the tag it left"""
    from vae_gp_ode_amd import _lib
    calls, real = [], _lib.call

    def call(name, *args):
        rc = real(name, *args)
        calls.append((name, _lib.load().gpode_last_launch().decode()))
        return rc
    monkeypatch.setattr(_lib, 'call', call)
    return calls


WRAPPER_TAGS = {'kl': ['reparam_kl_fwd', 'sigmoid_loglik_fwd', 'elbo_all_fwd_kl', 'elbo_loglik_bwd_kl', 'reparam_kl_bwd'],
                'll': ['reparam_fwd', 'sigmoid_loglik_fwd', 'elbo_all_fwd', 'elbo_loglik_bwd', 'reparam_bwd'],
                'plain': ['reparam_fwd', 'act_fwd', 'loglik_rowsum', 'elbo_all_fwd', 'elbo_all_bwd', 'reparam_bwd', 'loglik_rowsum_bwd', 'act_bwd']}


@pytest.mark.parametrize('velocity', [False, True], ids=['order1', 'order2'])
@pytest.mark.parametrize('route', ['kl', 'll', 'plain'])
def test_elbo_all_wrapper_routes(route, velocity, monkeypatch):
    """vae_ops.elbo_all on its three routes -- _ElboAllKL after reparam on packed halves, _ElboAll with the (X, z) of sigmoid_loglik_parts,
    _ElboAll on row sums from the separate kernels -- with and without the velocity half: the four terms and the gradients of the
    encoder rows, the logits, Um and Us against fp64, and the kernels each route launched"""
    from oracle import gpode_oracle as O
    from vae_gp_ode_amd import vae_ops as V
    g = R._gen('wrapper', velocity)
    N, q, L, inner, M, Do = 5, 6, 2, 96, 7, 3
    rows = L * N
    hs, hv = (torch.cat((torch.randn(N, q, generator=g), torch.randn(N, q, generator=g) * 0.7 - 1.0), 1) for _ in range(2))
    eps, wz = torch.randn(N, q, generator=g), torch.randn(N, q, generator=g)
    X, a = R._x_form((N, inner), 'norm', g), R._logits((rows, inner), g)
    Um, Us = 0.5 * torch.randn(M, Do, generator=g), R.us_packed(M, Do, 'tril', 1.0, g)
    w4 = torch.tensor([1.0, -0.2, 0.3, 0.1])
    names = ['hs', 'a', 'Um', 'Us'] + (['hv'] if velocity else [])

    def leaves(dev, dt):
        return {k: v.to(dev, dt).requires_grad_(True) for k, v in dict(hs=hs, hv=hv, a=a, Um=Um, Us=Us).items() if k in names}

    r = leaves('cpu', torch.float64)
    z0 = r['hs'][:, :q] + torch.exp(0.5 * r['hs'][:, q:]) * eps.double()
    lrow = R.bernoulli_terms(X.double().repeat(L, 1), torch.sigmoid(r['a'])).sum(1)
    kl = sum(R.normal_kl(r[k][:, :q], r[k][:, q:]).sum() for k in ('hs', 'hv') if k in r) / N
    ku = O.svgp_kl(r['Um'], r['Us'])
    out64 = R.elbo_algebra(lrow.mean(), kl, ku)
    ((z0 * wz.double()).sum() + (out64 * w4.double()).sum()).backward()

    calls = _recorded(monkeypatch)
    d = leaves('cuda', torch.float32)
    Xd = X.cuda()
    if route == 'kl':
        halves = [d[k].chunk(2, dim=1) if k in d else (None, None) for k in ('hs', 'hv')]
    else:                                             # separate tensors: no packed rows for reparam() to attach the KL partial sums to
        halves = [(d[k][:, :q].clone(), d[k][:, q:].clone()) if k in d else (None, None) for k in ('hs', 'hv')]
    (mu_s, lv_s), (mu_v, lv_v) = halves
    z = V.reparam(mu_s, lv_s, eps.cuda())
    if velocity and route == 'kl':
        V.reparam(mu_v, lv_v, eps.cuda())
    if route == 'plain':
        lpart = V.bernoulli_loglik_rowsum(Xd, V.sigmoid(d['a']), rows).view(rows, 1)
    else:
        lpart, _ = V.sigmoid_loglik_parts(Xd, d['a'], rows)
    out = torch.stack(V.elbo_all(lpart, mu_s, lv_s, mu_v, lv_v, d['Um'], d['Us'], M, R.NOBS))
    ((z * wz.cuda()).sum() + (out * w4.cuda()).sum()).backward()
    torch.cuda.synchronize()
    tags = [t for _, t in calls]
    if velocity and route == 'kl':
        assert tags.count('reparam_kl_fwd') == 2 and tags.count('reparam_kl_bwd') == 2
    assert sorted(set(tags)) == sorted(set(WRAPPER_TAGS[route])), (route, calls)
    SEEN.update(tags)
    scale = torch.stack([lrow.detach().abs().mean() * R.NOBS + kl.detach() * R.NOBS + R.svgp_kl_terms_abs(r['Um'].detach(), r['Us'].detach(), M),
                         lrow.detach().abs().mean(), kl.detach(), R.svgp_kl_terms_abs(r['Um'].detach(), r['Us'].detach(), M)])
    e = ((out.detach().double().cpu() - out64.detach()).abs() / scale).max().item()
    ez = ((z.detach().double().cpu() - z0.detach()).abs().max() / z0.detach().abs().max()).item()
    print('%s order %d: terms %.2e, z %.2e' % (route, 1 + velocity, e, ez))
    assert e <= R.TOL_KL and ez <= R.TOL_Z
    for k in names:
        eg = ((d[k].grad.double().cpu() - r[k].grad).abs().max() / r[k].grad.abs().max()).item()
        print('  gradient of %s %.2e' % (k, eg))
        assert eg <= R.TOL, (route, k, eg)


def test_sigmoid_loglik_parts_backward_without_the_fused_gradient(monkeypatch):
    """a consumer other than elbo_all(): _SigmoidLogLikParts.backward launches gpode_sigmoid_loglik_bwd on the row gradients it is handed"""
    from vae_gp_ode_amd import vae_ops as V
    g = R._gen('parts fallback')
    N, L, inner = 4, 3, 3136
    rows = L * N
    X, a, w = R._x_form((N, inner), 'norm', g), R._logits((rows, inner), g), torch.randn(rows, generator=g)
    calls = _recorded(monkeypatch)
    ad = a.cuda().requires_grad_(True)
    lpart, z = V.sigmoid_loglik_parts(X.cuda(), ad, rows)
    assert lpart.shape == (rows, R.sigmoid_loglik_splits(rows, inner)) and lpart.shape[1] > 1
    (lpart * w.cuda()[:, None]).sum().backward()
    assert [t for _, t in calls] == ['sigmoid_loglik_fwd', 'sigmoid_loglik_bwd'], calls
    SEEN.update(t for _, t in calls)
    a64 = a.double().requires_grad_(True)
    t = R.bernoulli_terms(X.double().repeat(L, 1), torch.sigmoid(a64))
    (t.sum(1) * w.double()).sum().backward()
    e = ((ad.grad.double().cpu() - a64.grad).abs().max() / a64.grad.abs().max()).item()
    es = ((lpart.detach().double().sum(1).cpu() - t.detach().sum(1)).abs() / t.detach().abs().sum(1)).max().item()
    print('fallback: logit gradient %.2e, row sums %.2e' % (e, es))
    assert e <= R.TOL and es <= R.TOL


# ---- 8: Adam and the gradient gather -------------------------------------------------------------------------------------------------------------------
@_param(R.adam_cases())
def test_adam_and_gather(c):
    _run(c)


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_tag_was_seen():
    """runs last: the union of the tags gpode_last_launch() reported above holds every tag these entry points can set.  It reads what
    the tests above left in this process, so it needs the whole module in one process (no -k, --lf or xdist), like the other route
    modules"""
    missing = [t for t in R.REQUIRED_TAGS if t not in SEEN]
    assert not missing, missing
