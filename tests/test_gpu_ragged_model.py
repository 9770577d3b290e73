"""GPU: compute_loss on ragged minibatches (n_obs), the tiny model at N = 4, T = 5, L = 2, first and second order, on the fused loss
stage and on the separate launches (GPODE_UNFUSED_LOSS=1).  The batches come from data.utils.ragged_frames; the device generators are
re-seeded identically before every call that is compared with another.

(i)   against a loss assembled in torch from model(X, L, logits=True, ts=ts): the Bernoulli terms x a - softplus(a) in float64 from the
      model's float32 logits, masked with torch.where on the logits' terms, the KL terms from torch.distributions.  The four terms within
      loss_routes.TOL_KL (1e-5) of the sum of the absolute values of what each of them adds up; every parameter gradient within 2e-5 of
      its largest entry.  The five biases in front of a BatchNorm have a true gradient of 0 and hold round-off on either side: they are
      held as test_gpu_model.test_fused_loss_stage_equals_the_separate_launches holds them, below 1e-3 of their layer's weight gradient.
      The same comparison WITHOUT a mask (fused against separate launches, the code of the parent commit) is printed beside it; where
      it exceeds 2e-5 for a parameter, that parameter's bound is twice that figure (PARENT below).  Measured on an MI355X: without
      a mask the worst parameter is 3.2e-7 (order 1; order 2: the two routes agree bit for bit), so PARENT is empty and every bound is
      2e-5; with the mask against the torch-side loss: terms at most 5.1e-7 (1e-5), gradients at most 9.4e-7 (2e-5).
(ii)  n_obs all T: loss and gradients bit-identical to the call without n_obs, and the launches of that call are the ones it always
      made (the call recorder of test_gpu_loss_routes).
(iii) NaN in the padded target frames: bit-identical loss and gradients (the encoders read the leading frames only).
(iv)  --solver dopri5 on a ragged_frames batch: status 0 on every row -- the padding keeps every time row strictly increasing.
(v)   one graphed step with three static buffers (X, ts, n_obs), replayed with a second batch and its counts, equals the eager steps
      bit for bit, the bound of test_gpu_time_grids.test_graph_replay_reads_the_grids_from_a_static_buffer."""
import copy

import pytest
import torch
import torch.nn.functional as Fn

import loss_routes as R
from test_gpu_time_grids import bits, tiny_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def leave_the_global_generators_as_found():
    """The tests of this file seed and draw from the process-wide generators (torch on the host and on the device, numpy through
    build_model, random through main()); test files that run after this one build layers from the global generator without seeding it
    (the decoder chain of test_gpu_vae_layers.py), so what they see must not depend on whether this file ran: the states are put back
    when it is done, as test_gpu_time_grids.py does."""
    import random
    import numpy as np
    saved = (torch.get_rng_state(), torch.cuda.get_rng_state_all(), np.random.get_state(), random.getstate())
    yield
    torch.set_rng_state(saved[0])
    torch.cuda.set_rng_state_all(saved[1])
    np.random.set_state(saved[2])
    random.setstate(saved[3])

N, T, L = 4, 5, 2
ORDERS = {'order1': dict(), 'order2': dict(ode=2, D_in=6, D_out=3, latent_dim=3, frames=3)}
NO_GRAD = ('cnn.0.bias', 'cnn.3.bias', 'decnn.1.bias', 'decnn.4.bias', 'decnn.7.bias')
# parameter -> the parent's fused-against-separate error at this shape without a mask, where it exceeds 2e-5 (the bound is twice it)
PARENT = {}
_orders = pytest.mark.parametrize('order', list(ORDERS))
_routes = pytest.mark.parametrize('fused', [True, False], ids=['fused', 'unfused'])


def ragged_batch(m, seed=5, full_T=8, N=N):
    """(Xpad (N,T,...), ts (N,T), n_obs (N,) int32) with at least one padded frame"""
    from vae_gp_ode_amd.data.utils import ragged_frames
    lead = 1 if m.order == 1 else m.v_steps
    X = torch.rand(N, full_T, 1, 28, 28, generator=torch.Generator().manual_seed(seed)).cuda()
    gen = torch.Generator(device='cuda').manual_seed(seed)
    for _ in range(16):
        Xp, idx, n_obs = ragged_frames(X, lead + 1, T, lead, gen)
        if int(n_obs.min()) < T:
            break
    assert lead < int(n_obs.min()) < T
    return Xp.contiguous(), (m.dt * idx.float()).contiguous(), n_obs


def grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def loss_and_grads(m, src, X, L_, **kw):
    from vae_gp_ode_amd.model.create_model import compute_loss
    m.zero_grad(set_to_none=True)
    src.manual_seed(17)
    out = compute_loss(m, X, L_, **kw)
    out[0].backward()
    torch.cuda.synchronize()
    return [t.detach().clone() for t in out], grads(m)


def torch_side(m, src, X, ts, n_obs):
    """the masked ELBO in torch (float64) from the model's logits and codes; -> (four terms, their scales, gradients)"""
    m.zero_grad(set_to_none=True)
    src.manual_seed(17)
    logits, (s_mu, s_logv), (v_mu, v_logv) = m(X, L, logits=True, ts=ts)
    a, x = logits.double(), X.double()[None]
    lp = x * a - Fn.softplus(a)
    obs = torch.arange(T, device=X.device)[None, :] < n_obs[:, None].long()
    lp = torch.where(obs[None, :, :, None, None, None], lp, torch.zeros((), dtype=torch.float64, device=X.device))
    lh = lp.sum(dim=(2, 3, 4, 5)).mean(0).mean()
    kl = R.normal_kl(s_mu.double(), s_logv.double()).sum(-1)
    if v_mu is not None:
        kl = kl + R.normal_kl(v_mu.double(), v_logv.double()).sum(-1)
    kl = kl.mean()
    ku = m.flow.kl().double()
    nobs = float(m.num_observations)
    out = [-(lh * nobs - kl * nobs - ku), -lh, kl, ku]
    out[0].backward()
    torch.cuda.synchronize()
    field = m.flow.odefunc.diffeq
    ku_abs = R.svgp_kl_terms_abs(field.Um.optvar.detach().double().cpu(), field.us_packed().detach().double().cpu(), field.M)
    lh_abs = lp.detach().abs().sum(dim=(2, 3, 4, 5)).mean().item()
    scale = [lh_abs * nobs + kl.item() * nobs + float(ku_abs), lh_abs, kl.item(), float(ku_abs)]
    return [t.detach() for t in out], scale, grads(m)


def compare_grads(got, ref, what):
    """{parameter: error relative to the largest entry of ref}; the dead biases are checked here, against their layer's weight gradient"""
    assert got.keys() == ref.keys()
    errs = {}
    for k, gb in ref.items():
        if k.endswith(NO_GRAD):
            scale = float(ref[k[:-4] + 'weight'].abs().max())
            assert float(got[k].abs().max()) < 1e-3 * scale and float(gb.abs().max()) < 1e-3 * scale, (what, k, scale)
            continue
        errs[k] = float((got[k].double() - gb.double()).abs().max() / gb.double().abs().max().clamp_min(1e-30))
    return errs


@_routes
@_orders
def test_masked_loss_matches_the_torch_side_loss(order, fused, monkeypatch):
    from vae_gp_ode_amd.model import create_model as C
    m, src = tiny_model(**ORDERS[order])
    X, ts, n_obs = ragged_batch(m)
    # the parent's own comparison at this shape, no mask: fused against the separate launches
    res = {}
    for f in (True, False):
        monkeypatch.setattr(C, '_FUSED_LOSS', f)
        res[f] = loss_and_grads(m, src, X, L, ts=ts)
    parent = compare_grads(res[True][1], res[False][1], 'no mask')
    print('%s no mask, fused against separate launches: worst %s' % (order, sorted(((v, k) for k, v in parent.items()), reverse=True)[:3]))
    monkeypatch.setattr(C, '_FUSED_LOSS', fused)
    out, g = loss_and_grads(m, src, X, L, ts=ts, n_obs=n_obs)
    ref, scale, gr = torch_side(m, src, X, ts, n_obs)
    e_terms = [abs(float(a) - float(b)) / s for a, b, s in zip(out, ref, scale)]
    errs = compare_grads(g, gr, 'masked')
    print('%s %s n_obs %s: terms %s; gradients worst %s' % (order, 'fused' if fused else 'unfused', n_obs.tolist(), ['%.2e' % e for e in e_terms],
                                                          sorted(((v, k) for k, v in errs.items()), reverse=True)[:3]))
    assert float(out[1]) != float(res[fused][0][1]), 'the mask changed nothing'
    assert all(e <= R.TOL_KL for e in e_terms), e_terms
    bad = {k: v for k, v in errs.items() if not v <= max(2e-5, 2 * PARENT.get(k, 0.0))}
    assert not bad, bad


@_routes
@_orders
def test_full_lengths_and_padded_garbage(order, fused, monkeypatch):
    from vae_gp_ode_amd.model import create_model as C
    monkeypatch.setattr(C, '_FUSED_LOSS', fused)
    m, src = tiny_model(**ORDERS[order])
    X, ts, n_obs = ragged_batch(m)
    # (ii) full lengths: the bits of the call without counts
    plain = loss_and_grads(m, src, X, L, ts=ts)
    full = loss_and_grads(m, src, X, L, ts=ts, n_obs=torch.full((N,), T, dtype=torch.int32, device='cuda'))
    assert all(bits(a, b) for a, b in zip(plain[0], full[0]))
    assert plain[1].keys() == full[1].keys() and all(bits(plain[1][k], full[1][k]) for k in plain[1])
    # (iii) NaN in the padded target frames
    clean = loss_and_grads(m, src, X, L, ts=ts, n_obs=n_obs)
    Xb = X.clone()
    for n, k in enumerate(n_obs.tolist()):
        Xb[n, k:] = float('nan')
    assert bool(torch.isnan(Xb).any())
    dirty = loss_and_grads(m, src, Xb, L, ts=ts, n_obs=n_obs)
    assert all(bool(torch.isfinite(t).all()) for t in dirty[0]) and all(bool(torch.isfinite(v).all()) for v in dirty[1].values())
    assert all(bits(a, b) for a, b in zip(clean[0], dirty[0]))
    assert all(bits(clean[1][k], dirty[1][k]) for k in clean[1])
    assert not bits(clean[0][0], plain[0][0])


def test_no_counts_make_the_launches_of_before(monkeypatch):
    """n_obs=None: the recorded launches of compute_loss hold no *_len entry and are those of the call with ts alone; with counts the
    loss stage's three launches are the *_len forms and nothing else changes"""
    from vae_gp_ode_amd import _lib
    from vae_gp_ode_amd.model.create_model import compute_loss
    m, src = tiny_model()
    X, ts, n_obs = ragged_batch(m)
    calls, real = [], _lib.call

    def call(name, *args):
        rc = real(name, *args)
        calls.append((name, _lib.load().gpode_last_launch().decode()))
        return rc
    monkeypatch.setattr(_lib, 'call', call)

    def record(**kw):
        del calls[:]
        src.manual_seed(17)
        compute_loss(m, X, L, ts=ts, **kw)[0].backward()
        torch.cuda.synchronize()
        return list(calls)
    plain, masked = record(), record(n_obs=n_obs)
    assert not [c for c in plain if c[0].endswith('_len') or c[1].endswith('_len')], plain
    stage = ('gpode_sigmoid_loglik_fwd', 'gpode_elbo_all_bwd_ll_kl', 'gpode_elbo_all_bwd_ll')
    assert [n for n, _ in plain if n in stage] in ([stage[0], stage[1]], [stage[0], stage[2]]), plain
    swapped = [(n + '_len', t + '_len') if n in stage else (n, t) for n, t in plain]
    assert masked == swapped, (masked, swapped)


@_orders
def test_dopri5_finishes_every_row_of_a_ragged_batch(order):
    kw = dict(ORDERS[order], solver='dopri5')
    m, src = tiny_model(**kw)
    m.flow.rtol, m.flow.atol, m.flow.max_steps = 1e-4, 1e-4, 64
    X, ts, n_obs = ragged_batch(m)
    assert bool((ts[:, 1:] > ts[:, :-1]).all())
    out, g = loss_and_grads(m, src, X, L, ts=ts, n_obs=n_obs)
    status = m.flow.last_counts[..., 2]
    print('%s dopri5: loss %.6g, status %s' % (order, float(out[0]), status.tolist()))
    assert bool((status == 0).all()) and all(bool(torch.isfinite(t).all()) for t in out)
    assert all(bool(torch.isfinite(v).all()) for v in g.values())


def test_graph_replay_reads_the_counts_from_a_static_buffer():
    from vae_gp_ode_amd.graph import GraphedStep
    from vae_gp_ode_amd.model.create_model import compute_loss
    from vae_gp_ode_amd.optim import HipAdam
    m, src = tiny_model()
    init = copy.deepcopy(m.state_dict())
    batches = [ragged_batch(m, seed=5), ragged_batch(m, seed=6)]
    assert not torch.equal(batches[0][2], batches[1][2])
    order = (0, 0, 1)

    def run(use_graph):
        m.load_state_dict(init)
        src.manual_seed(17)
        opt = HipAdam(m.parameters(), lr=1e-4)      # 1e-3 takes a diagonal entry of the tiny model's Us through 0 in one step (kl_u = inf), mask or no mask
        buf, tbuf, nbuf = (torch.empty_like(t) for t in batches[0])

        def step():
            opt.zero_grad()
            loss, *_ = compute_loss(m, buf, 1, ts=tbuf, n_obs=nbuf)
            loss.backward()
            opt.step()
            return loss
        losses, gs = [], None
        for b in order:
            buf.copy_(batches[b][0]); tbuf.copy_(batches[b][1]); nbuf.copy_(batches[b][2])
            if not use_graph:
                losses.append(step().detach().clone())
            elif gs is None:
                gs = GraphedStep(step, warmup=1)
                losses.append(gs.warm_out.clone())
            else:
                losses.append(gs().clone())
        torch.cuda.synchronize()
        return losses, [p.detach().clone() for p in m.parameters()]
    try:
        le, pe = run(False)
        lg, pg = run(True)
    finally:                                         # the process-wide switch HipAdam sets for itself
        from vae_gp_ode_amd import vae_ops
        vae_ops.set_deferred_reductions(False)
    print('eager losses %s, graphed %s; counts %s' % ([x.item() for x in le], [x.item() for x in lg], [b[2].tolist() for b in batches]))
    assert all(bool(torch.isfinite(x).all()) for x in le)
    assert all(bits(a, b) for a, b in zip(le, lg)), ([x.item() for x in le], [x.item() for x in lg])
    assert all(bits(a, b) for a, b in zip(pe, pg))
    assert not bits(le[1], le[2])


# ---- the command lines ------------------------------------------------------------------------------------------------------------------
def test_main_trains_on_ragged_sequences(tmp_path, monkeypatch):
    """test_gpu_time_grids.test_main_trains_on_subsampled_sequences' configuration with --ragged_frames 3 (of --subsample_frames 5 and of
    --T 6): two steps, eagerly and replayed with the counts in a static buffer"""
    import glob
    import math
    from vae_gp_ode_amd import main as M
    from vae_gp_ode_amd import ops, vae_ops
    monkeypatch.chdir(tmp_path)
    common = ['--task', 'synthetic', '--Ndata', '8', '--Ntest', '4', '--batch', '4', '--T', '6', '--solver', 'rk4', '--num_inducing', '16',
              '--num_features', '32', '--lr', '1e-4', '--log_freq', '1', '--Nepoch', '1', '--ragged_frames', '3']
    try:
        for tag, extra in (('s', ['--subsample_frames', '5']), ('g', ['--hip_graph', 'True'])):
            M.main(common + ['--save', 'results/' + tag] + extra)
            ck = glob.glob(str(tmp_path / 'results' / (tag + '_*') / 'odegpvae_mnist.pth'))
            assert len(ck) == 1
            sd = torch.load(ck[0])
            assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
            log = open(glob.glob(str(tmp_path / 'results' / (tag + '_*') / 'logs'))[0]).read()
            elbo = [float(ln.split('elbo')[1].split('(')[0]) for ln in log.splitlines() if ln.startswith('Iter:')]
            assert len(elbo) == 2 and all(math.isfinite(v) for v in elbo), elbo
            assert 'keeps 3 to %d of its frames' % (5 if tag == 's' else 6) in log
    finally:                                         # process-wide switches the training loop sets for itself
        ops.set_overlap(False)
        vae_ops.set_deferred_reductions(False)


def test_evaluate_on_ragged_sequences(tmp_path, capsys):
    import json
    import math
    from vae_gp_ode_amd import evaluate as E
    from vae_gp_ode_amd.model.create_model import build_model
    from vae_gp_ode_amd.model.misc.torch_utils import seed_everything
    argv = ['--task', 'synthetic', '--Ndata', '8', '--Ntest', '6', '--batch', '4', '--T', '6', '--solver', 'rk4', '--num_inducing', '16',
            '--num_features', '32', '--model_path', str(tmp_path), '--eval_sample_size', '4', '--Troll', '2', '--save', str(tmp_path / 'ev'),
            '--device_noise', 'True', '--eval_z0_draws', 'True']
    args = E.make_parser().parse_args(argv)
    args.device = torch.device('cuda')
    seed_everything(3)
    torch.save(build_model(args).to(args.device).state_dict(), tmp_path / 'odegpvae_mnist.pth')
    plain = E.main(argv)
    rag = E.main(argv + ['--ragged_frames', '2'])
    again = E.main(argv + ['--ragged_frames', '2'])
    out = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')][-1])
    text = lambda d: json.dumps({k: v for k, v in d.items() if k != 'ms'}, sort_keys=True)      # as text: a frame no sequence has is NaN
    assert text(out) == text(again) and rag['ragged_frames'] == 2 and 'ragged_frames' not in plain
    assert text(rag) == text(again)                                      # reproducible from --seed
    assert len(rag['mse_t']) == 6 and len(rag['nll_t']) == 6 and rag['rollout_T'] == plain['rollout_T'] == 12
    assert rag['count'] % (4 * 784) == 0 and 6 * 2 <= rag['count'] // (4 * 784) < 6 * 6 and plain['count'] == 4 * 784 * 6 * 6
    assert all(math.isfinite(rag[k]) for k in ('mse', 'std', 'nll', 'nlpd', 'iw_nll', 'ess_mean')) and rag['nll'] != plain['nll']
    assert all(math.isfinite(v) for v in rag['mse_t'][:2] + rag['nll_t'][:2])
