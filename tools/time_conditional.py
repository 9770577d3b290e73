#!/usr/bin/env python3
"""What the forecast conditioned on an observed prefix costs, at the evaluation size (L = 128, N = 40, T = 16), on one GPU.

    python tools/time_conditional.py [--parent_lib SO] [--out FILE] [--L 128] [--N 40] [--T 16] [--n_cond 4] [--windows 5] [--min_window_s 1.0]

  predict_marginal      evaluate.predict_marginal: L joint draws, the decoder, k_fwd_predict<true> -- the same work minus the second
                        last-stage pass
  predict_conditional   evaluate.predict_conditional(n_cond): the same, plus per decoder pass the log-weights (a few element-wise float64
                        launches on (Lc, N) values) and gpode_dec10_predict_w, a second k_fwd_predict-class kernel over the same c
  predict_plain         evaluate.predict(variance=False), the route that existed
  predict_plain_parent  predict_plain through the parent commit's library (--parent_lib SO, loaded next to this build's, the same
                        process and the same windows): the untouched route against the parent build, never against itself
The model and the inputs of tools/eval_bench.py (configs[0]: RBF, q = 6, M = 100, S = 256, rk4; synthetic frames, device noise).  Every
route is warmed, then the routes alternate in windows of whole evaluations, each at least --min_window_s long, timed with device events;
median ms per evaluation and spread = (max - min) / median.  `conditional_cost` = predict_conditional / predict_marginal - 1 is reported
with the spreads, whichever way it falls -- this is analysis, there is no speed target -- beside `ess` of the weights (read it first: on
this untrained model it says how many draws the conditional forecast rests on).  `plain_vs_parent` is held to the larger of the two
spreads.  No GPU: nothing is measured and the tool says so."""
import argparse
import ctypes
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--L', type=int, default=128)
    ap.add_argument('--N', type=int, default=40)
    ap.add_argument('--T', type=int, default=16)
    ap.add_argument('--n_cond', type=int, default=4)
    ap.add_argument('--images_per_pass', type=int, default=8192)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--min_window_s', type=float, default=1.0)
    ap.add_argument('--seed', type=int, default=121)
    ap.add_argument('--parent_lib', default=None, help="the parent commit's libgpode_hip.so, timed in the same windows")
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_conditional.py measures on an MI355X: no GPU found, nothing measured')
    from vae_gp_ode_amd import _lib
    from vae_gp_ode_amd.evaluate import plan_passes, predict, predict_conditional, predict_marginal
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

    def marginal():
        p = predict_marginal(model, X, a.L, images_per_pass=a.images_per_pass)
        return p.iw_nll, float(p.ess.mean())

    def conditional():
        p = predict_conditional(model, X, a.L, a.n_cond, images_per_pass=a.images_per_pass)
        return p.fc_mse, p.fc_nlpd, float(p.ess.mean()), float(p.ess.min()), float(p.fc_mse_uncond_t[a.n_cond:].mean())

    def plain():
        p = predict(model, X, a.L, images_per_pass=a.images_per_pass, variance=False)
        return p.mse, p.std

    routes = [('predict_marginal', marginal), ('predict_conditional', conditional), ('predict_plain', plain)]
    if a.parent_lib:
        this, parent = _lib.load(), ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name, (res, argt) in _lib.SIGNATURES.items():
            if hasattr(parent, name):                  # the parent's header is a subset of this build's
                getattr(parent, name).restype, getattr(parent, name).argtypes = res, argt

        def plain_parent():
            _lib._lib = parent
            try:
                return plain()
            finally:
                _lib._lib = this
        routes.append(('predict_plain_parent', plain_parent))
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
    spread = {k: round((max(v) - min(v)) / med[k], 4) for k, v in times.items()}
    passes = plan_passes(a.L, a.N * a.T, a.images_per_pass)
    c = last['predict_conditional']
    out = dict(L=a.L, N=a.N, T=a.T, n_cond=a.n_cond, images_per_pass=a.images_per_pass, passes=[e - s for s, e in passes],
               device=torch.cuda.get_device_name(0), windows=a.windows, evaluations_per_window=reps,
               ms_per_evaluation={k: [round(t, 3) for t in v] for k, v in times.items()}, median_ms={k: round(v, 3) for k, v in med.items()},
               spread=spread, conditional_cost=round(med['predict_conditional'] / med['predict_marginal'] - 1, 4),
               conditional_cost_spread=max(spread['predict_conditional'], spread['predict_marginal']),
               conditional_extra_ms=round(med['predict_conditional'] - med['predict_marginal'], 3),
               c_bytes_read_again=a.L * a.N * a.T * 16 * 784 * 4,
               figures=dict(fc_mse=c[0], fc_nlpd=c[1], ess_mean=c[2], ess_min=c[3], fc_mse_uncond=c[4], iw_nll=last['predict_marginal'][0],
                            ess_marginal_mean=last['predict_marginal'][1]))
    if 'predict_plain_parent' in med:
        out['plain_vs_parent'] = round(med['predict_plain'] / med['predict_plain_parent'] - 1, 4)
        out['plain_vs_parent_allowed'] = max(spread['predict_plain'], spread['predict_plain_parent'])
        out['plain_not_slower_than_parent'] = out['plain_vs_parent'] <= out['plain_vs_parent_allowed']
    txt = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')
    print(txt)


if __name__ == '__main__':
    main()
