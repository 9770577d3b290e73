#!/usr/bin/env python3
"""Posterior-predictive evaluation, the route that existed before against evaluate.predict, on one GPU.

    python tools/eval_bench.py [--L 128] [--N 40] [--T 16] [--Troll 1] [--windows 5] [--min_window_s 1.0] [--loglik | --z0_draws [--parent_lib SO]]

  baseline  model.eval(); model(X, Lc[, T_custom]) per pass of at most --images_per_pass images, then torch's var_mean of the squared
            error per pass, merged at the end (the only route before evaluate.py; in passes so that both fit the same memory)
  new       evaluate.predict(model, X, L[, T_custom]) with the predictive mean / variance (`predict_full`: the route to compare), and
            statistics only (`predict_stats`: it stops the roll-out at T, so with --Troll > 1 it does less work than the baseline)

configs[0] model (RBF, q = 6, M = 100, S = 256, rk4), synthetic frames, device noise for both routes.  Every shape is warmed up,
then the routes alternate in windows of whole evaluations, each window at least --min_window_s long, timed with device events around
the window.  One JSON line: per-window ms per evaluation, medians, spread (max - min over the median) and the ratio.  Without a GPU it
fails.

--loglik measures the held-out log-likelihood instead (statistics only, no predictive moments), the same alternating windows:
  predict_plain         evaluate.predict(variance=False)                       -- k_fwd_predict<false>
  predict_loglik        evaluate.predict(variance=False, loglik=True)          -- k_fwd_predict<true>, one more copy of L F floats
  unfused_loglik        model.eval(); model(X, Lc) per pass, torch's var_mean of the squared error and the reference's
                        log(z) x + log(1 - z) (1 - x) summed per sequence, then the log-mean-exp over the draws
  predict_plain_parent  predict_plain through the library of the parent commit given with --parent_lib (loaded next to this
                        build's, the same process and the same windows), to show that the plain route did not move
It reports, with no target set, `loglik_cost` = predict_loglik / predict_plain - 1 beside the window spreads, and -- the condition --
`plain_vs_parent` = predict_plain / predict_plain_parent - 1, which must not exceed the larger of the two spreads.

--z0_draws measures the marginal likelihood route (an initial state per draw), the same alternating windows:
  predict_loglik        evaluate.predict(variance=False, loglik=True)          -- one z0 sample shared by the L draws
  predict_marginal      evaluate.predict_marginal                               -- L z0 samples and their log-weights in one launch, the rollout
                        reading its own z0 per draw; the same trajectory count and decoder work
  predict_plain, predict_plain_parent   as under --loglik (the second with --parent_lib): the route that existed must not have moved
It reports, with no target set, `marginal_cost` = predict_marginal / predict_loglik - 1 beside the window spreads, and `plain_vs_parent` with
its condition as under --loglik.

`--dry` only parses, plans the passes and prints the byte counts (a rehearsal, no timing).
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def byte_counts(L, N, T, Th, passes):
    """HBM bytes the decoder's stages must move per evaluation (float32), from shapes: activations 6x6x64, 13x13x32, 28x28x16."""
    imgs = L * N * Th
    a1, a4, a7, y = 64 * 36 * 4, 32 * 169 * 4, 16 * 784 * 4, 784 * 4
    F = N * Th
    state = len(passes) * F * (2 * 2 * y + 2 * 12) + len(passes) * N * T * y          # predictive state read + written, targets read, per pass
    return dict(images=imgs,
                unfused_eval_decoder=imgs * (4 * (a1 + a4 + a7) + 2 * y),              # conv write, BN read, BN write, conv read; logits + sigmoid
                frozen_decoder=imgs * 2 * (a1 + a4 + a7),                              # conv write, conv read
                dec10_predict=imgs * a7 + state)


def loglik_routes(a, model, X, passes, Tc):
    """the routes of --loglik: [(name, callable returning (mse, std[, nll, nlpd]))]"""
    import ctypes
    import torch
    from vae_gp_ode_amd import _lib
    from vae_gp_ode_amd.evaluate import log_mean_exp, mean_std, merge_states, predict

    def plain():
        p = predict(model, X, a.L, T_custom=Tc, images_per_pass=a.images_per_pass, variance=False)
        return p.mse, p.std

    def loglik():
        p = predict(model, X, a.L, T_custom=Tc, images_per_pass=a.images_per_pass, variance=False, loglik=True)
        return p.mse, p.std, p.nll, p.nlpd

    def unfused():
        model.eval()
        parts, lls = [], []
        with torch.no_grad():
            for s, e in passes:
                Xrec, _, _ = model(X, e - s, T_custom=Tc)
                z = Xrec[:, :, :a.T]
                se = (z - X) ** 2
                parts.append((se.numel(),) + torch.var_mean(se, unbiased=False))
                lls.append((torch.log(z) * X + torch.log(1 - z) * (1 - X)).sum(dim=(2, 3, 4, 5)))
        model.train()
        ll = torch.cat(lls).double().cpu()
        return mean_std(merge_states([(n, m.item(), v.item() * n) for n, v, m in parts])) + (-ll.mean().item(), -log_mean_exp(ll).mean().item())

    def marginal():
        from vae_gp_ode_amd.evaluate import predict_marginal
        p = predict_marginal(model, X, a.L, images_per_pass=a.images_per_pass)
        return p.mse, p.std, p.nll, p.nlpd, p.iw_nll, float(p.ess.mean())

    routes = [('predict_plain', plain), ('predict_loglik', loglik), ('unfused_loglik', unfused)]
    if a.z0_draws:
        routes = [('predict_plain', plain), ('predict_loglik', loglik), ('predict_marginal', marginal)]
    if a.parent_lib:
        this, parent = _lib.load(), ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name, (res, args) in _lib.SIGNATURES.items():
            if hasattr(parent, name):                  # the parent's header is a subset of this build's
                getattr(parent, name).restype, getattr(parent, name).argtypes = res, args

        def plain_parent():
            _lib._lib = parent
            try:
                return plain()
            finally:
                _lib._lib = this
        routes.append(('predict_plain_parent', plain_parent))
    return routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--L', type=int, default=128)
    ap.add_argument('--N', type=int, default=40)
    ap.add_argument('--T', type=int, default=16)
    ap.add_argument('--Troll', type=int, default=1)
    ap.add_argument('--images_per_pass', type=int, default=8192)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--min_window_s', type=float, default=1.0)
    ap.add_argument('--seed', type=int, default=121)
    ap.add_argument('--dry', action='store_true')
    ap.add_argument('--loglik', action='store_true')
    ap.add_argument('--z0_draws', action='store_true')
    ap.add_argument('--parent_lib', default=None)
    a = ap.parse_args()
    from vae_gp_ode_amd.evaluate import plan_passes
    Th = a.Troll * a.T
    Tc = Th if Th > a.T else None
    passes = plan_passes(a.L, a.N * Th, a.images_per_pass)
    cfg = dict(L=a.L, N=a.N, T=a.T, Th=Th, images_per_pass=a.images_per_pass, passes=[e - s for s, e in passes],
               bytes=byte_counts(a.L, a.N, a.T, Th, passes))
    if a.dry:
        print(json.dumps(dict(cfg, dry=True)))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/eval_bench.py measures on an MI355X: no GPU found, nothing measured')
    from vae_gp_ode_amd.evaluate import mean_std, merge_states, predict
    from vae_gp_ode_amd.model.core.initialization import initialize_and_fix_kernel_parameters
    from vae_gp_ode_amd.model.core.noise import install_device_noise
    from vae_gp_ode_amd.model.create_model import build_model
    from vae_gp_ode_amd.model.misc.torch_utils import seed_everything
    dev = torch.device('cuda')
    seed_everything(a.seed)
    args = types.SimpleNamespace(D_in=6, D_out=6, num_inducing=100, num_features=256, dimwise=True, q_diag=False, device=dev, kernel='RBF',
                                 ode=1, solver='rk4', use_adjoint=False, frames=5, n_filt=8, latent_dim=6, Ndata=360, dt=0.1)
    model = build_model(args).to(dev)
    initialize_and_fix_kernel_parameters(model, 2.0, 0.7, fix=False)
    install_device_noise(model, a.seed + 1)
    X = ((torch.rand(a.N, a.T, 1, 28, 28, generator=torch.Generator().manual_seed(a.seed)) - 0.1307) / 0.3081).to(dev)
    with torch.no_grad():                              # running statistics off (0, 1), as after training
        model.train()
        for _ in range(3):
            model(X, 1)

    def baseline():
        model.eval()
        parts = []
        with torch.no_grad():
            for s, e in passes:
                Xrec, _, _ = model(X, e - s, T_custom=Tc)
                se = (Xrec[:, :, :a.T] - X) ** 2
                parts.append((se.numel(),) + torch.var_mean(se, unbiased=False))
        model.train()
        return mean_std(merge_states([(n, m.item(), v.item() * n) for n, v, m in parts]))

    def new_stats():
        p = predict(model, X, a.L, T_custom=Tc, images_per_pass=a.images_per_pass, variance=False)
        return p.mse, p.std

    def new_full():
        p = predict(model, X, a.L, T_custom=Tc, images_per_pass=a.images_per_pass)
        return p.mse, p.std

    routes = [('baseline', baseline), ('predict_stats', new_stats), ('predict_full', new_full)]
    if a.z0_draws and Tc is not None:
        raise SystemExit('--z0_draws: predict_marginal has no forecast frames, use --Troll 1')
    if a.loglik or a.z0_draws:
        routes = loglik_routes(a, model, X, passes, Tc)
    last, reps = {}, {}
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for name, fn in routes:                            # warm every shape, then size the windows
        fn()
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        last[name] = fn()
        e1.record()
        torch.cuda.synchronize()
        reps[name] = max(1, int(a.min_window_s * 1e3 / e0.elapsed_time(e1)) + 1)
    times = {name: [] for name, _ in routes}
    for _ in range(a.windows):
        for name, fn in routes:                        # alternating
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(reps[name]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps[name])
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    if a.loglik or a.z0_draws:
        spread = {k: round((max(v) - min(v)) / med[k], 4) for k, v in times.items()}
        out = dict(cfg, device=torch.cuda.get_device_name(0), windows=a.windows, evaluations_per_window=reps,
                   ms_per_evaluation={k: [round(t, 3) for t in v] for k, v in times.items()}, median_ms={k: round(v, 3) for k, v in med.items()},
                   spread=spread, loglik_cost=round(med['predict_loglik'] / med['predict_plain'] - 1, 4),
                   figures={k: [float(x) for x in v] for k, v in last.items()})
        if a.z0_draws:
            out['marginal_cost'] = round(med['predict_marginal'] / med['predict_loglik'] - 1, 4)
        else:
            out['loglik_vs_unfused'] = round(med['unfused_loglik'] / med['predict_loglik'], 3)
        if 'predict_plain_parent' in med:
            out['plain_vs_parent'] = round(med['predict_plain'] / med['predict_plain_parent'] - 1, 4)
            out['plain_vs_parent_allowed'] = max(spread['predict_plain'], spread['predict_plain_parent'])
            out['plain_not_slower_than_parent'] = out['plain_vs_parent'] <= out['plain_vs_parent_allowed']
        print(json.dumps(out))
        return
    out = dict(cfg, device=torch.cuda.get_device_name(0), windows=a.windows, evaluations_per_window=reps,
               ms_per_evaluation={k: [round(t, 3) for t in v] for k, v in times.items()}, median_ms={k: round(v, 3) for k, v in med.items()},
               spread={k: round((max(v) - min(v)) / med[k], 4) for k, v in times.items()},
               speedup_stats=round(med['baseline'] / med['predict_stats'], 3), speedup_full=round(med['baseline'] / med['predict_full'], 3),
               mse_std={k: [float(x) for x in v] for k, v in last.items()})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
