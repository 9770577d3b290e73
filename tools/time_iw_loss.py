"""Time the loss stage of training on the importance-weighted bound, and a whole training step with --iw_draws 4.

    python tools/time_iw_loss.py [--windows 7] [--min_window_s 0.3] [--parent_lib SO] [--out FILE.json]
    python tools/time_iw_loss.py --step [--windows 5] [--steps 20] [--out FILE.json]

Default: the loss stage at rows = L K N likelihood rows, L = 1, N = 256, K in {1, 4}, inner = 16 x 784 logits.  Legs, timed in alternating
windows on the same buffers (device events around `reps` repetitions, reps sized so that a window lasts --min_window_s; every leg warmed
first); median and spread = (max - min) / median per leg:
  iw_fused      gpode_sigmoid_loglik_fwd + gpode_elbo_iw_fwd + gpode_elbo_iw_bwd_ll
  iw_unfused    gpode_sigmoid_loglik_fwd + gpode_elbo_iw_fwd + gpode_elbo_iw_bwd + gpode_sigmoid_loglik_bwd
  standard      gpode_sigmoid_loglik_fwd + gpode_elbo_all_bwd_ll_kl on the same number of rows (the standard ELBO's pair)
  standard_parent   `standard` through the library of the parent commit given with --parent_lib (loaded next to this build's)
ga of the fused and the unfused leg is compared bit for bit before anything is timed.

--step: a whole training step (zero_grad, compute_loss, backward, Adam) of bench.py's configs[1] model (DF, q = 6, M = 100, T = 16),
eager and replayed as a captured graph, alternating windows of --steps steps:
  std_b256      the standard ELBO at batch 256
  iw4_b256      iw_draws = 4 at batch 256: 1024 trajectories, 4 x the decoder and loss work, the encoder work of batch 256
  std_b1024     the standard ELBO at batch 1024: the same decoder and loss work as iw4_b256, 4 x its encoder work
No GPU: nothing is measured and the tool says so."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _stats(times):
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    return med, {k: round((max(v) - min(v)) / med[k], 4) for k, v in times.items()}


def _windows(legs, windows, reps, torch):
    ev = lambda: torch.cuda.Event(enable_timing=True)
    times = {name: [] for name, _ in legs}
    for _ in range(windows):
        for name, fn in legs:                          # alternating
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(reps[name]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps[name] * 1e3)
    return times


def loss_stage(a, torch):
    from vae_gp_ode_amd import _lib
    lib = _lib.load()
    libs = {'this': lib}
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name, (res, args) in _lib.SIGNATURES.items():
            if hasattr(parent, name):
                getattr(parent, name).restype, getattr(parent, name).argtypes = res, args
        libs['parent'] = parent
    L, N, T, frame, M, Do, nks = 1, a.N, a.T, a.frame, 100, 6, 6
    dev = 'cuda'
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nobs = ctypes.c_float(360.0)
    result = dict(N=N, T=T, frame=frame, device=torch.cuda.get_device_name(0), windows=a.windows, K={})
    for K in (1, 4):
        rows, inner, nX = L * K * N, T * frame, N * T * frame
        n = rows * inner
        g = torch.Generator().manual_seed(a.seed + K)
        X = ((torch.rand(nX, generator=g) - 0.1307) / 0.3081).to(dev)
        logits = ((torch.rand(n, generator=g) * 2 - 1) * 8.0).to(dev)
        lw = (-3.0 + 2.0 * torch.randn(K, N, generator=g)).to(dev)
        Um = (0.5 * torch.randn(M, Do, generator=g)).to(dev)
        Us = (0.01 * torch.randn(Do, M * (M + 1) // 2, generator=g) + 0.5).to(dev)
        gs = [torch.tensor([v], device=dev) for v in (1.0, 0.0, 0.0, 0.0)]
        ns = lib.gpode_sigmoid_loglik_splits(rows, inner)
        new = lambda *s: torch.empty(*s, device=dev)
        z, part, ga, ga2 = new(n), new(rows, ns), new(n), new(n)
        out, grow, glw, gkls, dUm, dUs = new(5 + 256), new(rows), new(K, N), new(nks), new(M, Do), new(Do, M * (M + 1) // 2)

        def check(rc, lb):
            if rc:
                raise SystemExit('launch refused: ' + lb.gpode_last_error().decode())

        def fwd(lb):
            check(lb.gpode_sigmoid_loglik_fwd(p(X), p(logits), p(z), p(part), rows, inner, nX, ns, st()), lb)

        def iw(fused, dst):
            fwd(lib)
            check(lib.gpode_elbo_iw_fwd(p(part), rows, ns, p(lw), L, K, N, M, Do, p(Um), p(Us), nobs, p(out), st()), lib)
            head = [p(t) for t in gs] + [None, p(part), rows, ns, p(lw), L, K, N, M, Do, p(Um), p(Us), nobs, p(grow), p(glw), p(dUm), p(dUs)]
            if fused:
                check(lib.gpode_elbo_iw_bwd_ll(*head, p(X), p(z), p(dst), n, nX, st()), lib)
            else:
                check(lib.gpode_elbo_iw_bwd(*head, st()), lib)
                check(lib.gpode_sigmoid_loglik_bwd(p(X), p(z), p(grow), p(dst), rows, inner, nX, st()), lib)

        def standard(which):
            lb = libs[which]
            fwd(lb)
            check(lb.gpode_elbo_all_bwd_ll_kl(*[p(t) for t in gs], rows, N, M, Do, p(Um), p(Us), nobs, p(grow), p(gkls), nks, None, 0, p(dUm),
                                              p(dUs), p(X), p(z), p(ga), n, nX, st()), lb)
        legs = [('iw_fused', lambda: iw(True, ga)), ('iw_unfused', lambda: iw(False, ga2)), ('standard', lambda: standard('this'))]
        if a.parent_lib:
            legs.append(('standard_parent', lambda: standard('parent')))
        iw(True, ga)
        iw(False, ga2)
        torch.cuda.synchronize()
        same = torch.equal(ga.view(torch.int32), ga2.view(torch.int32))
        ev = lambda: torch.cuda.Event(enable_timing=True)
        reps = {}
        for name, fn in legs:
            fn()
            torch.cuda.synchronize()
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            torch.cuda.synchronize()
            reps[name] = max(10, int(a.min_window_s * 1e3 / (e0.elapsed_time(e1) / 10)) + 1)
        times = _windows(legs, a.windows, reps, torch)
        med, spread = _stats(times)
        nbytes = 4 * (4 * n + 2 * n)                   # logits, z (written, read), ga; X read once per pass over the logits
        r = dict(rows=rows, nsplit=ns, reps_per_window=reps, us={k: [round(t, 2) for t in v] for k, v in times.items()},
                 median_us={k: round(v, 2) for k, v in med.items()}, spread=spread,
                 GBps={k: round(nbytes / (v * 1e-6) / 1e9, 1) for k, v in med.items()}, fused_ga_bit_equal_unfused=same,
                 iw_fused_vs_standard=round(med['iw_fused'] / med['standard'] - 1, 4),
                 iw_fused_vs_unfused=round(med['iw_fused'] / med['iw_unfused'] - 1, 4))
        if a.parent_lib:
            r['standard_vs_parent'] = round(med['standard'] / med['standard_parent'] - 1, 4)
            r['standard_vs_parent_allowed'] = max(spread['standard'], spread['standard_parent'])
        result['K'][str(K)] = r
    return result


def whole_step(a, torch):
    import bench
    from vae_gp_ode_amd import ops
    from vae_gp_ode_amd.graph import GraphedStep, device_generators
    from vae_gp_ode_amd.model.create_model import backward, compute_loss
    from vae_gp_ode_amd.optim import HipAdam
    dev = torch.device('cuda', 0)
    legs, graphs = [], []
    for name, batch, K in (('std_b256', 256, None), ('iw4_b256', 256, 4), ('std_b1024', 1024, None)):
        w = dict(bench.WORKLOADS['cfg2'], batch=batch)
        model, X = bench.make_model_inputs(w, a.seed, dev, 0)
        Xd = X.to(dev)
        opt = HipAdam(model.parameters(), lr=1e-6, bucketed=False)

        def step(model=model, Xd=Xd, opt=opt, K=K):
            opt.zero_grad()
            loss, *_ = compute_loss(model, Xd, 1) if K is None else compute_loss(model, Xd, 1, iw_draws=K)
            backward(loss)
            ops.join_side_stream()
            opt.step()
            return loss
        for _ in range(3):
            step()
        legs.append((name + '_eager', step))
        g = GraphedStep(step, generators=device_generators(model), warmup=2)
        graphs.append(g)
        legs.append((name + '_graph', g))
    torch.cuda.synchronize()
    reps = {name: a.steps for name, _ in legs}
    times = _windows(legs, a.windows, reps, torch)
    med, spread = _stats(times)
    ms = lambda d: {k: round(v / 1e3, 4) for k, v in d.items()}
    return dict(workload=bench.WORKLOADS['cfg2']['desc'], device=torch.cuda.get_device_name(0), windows=a.windows, steps_per_window=a.steps,
                ms={k: [round(t / 1e3, 4) for t in v] for k, v in times.items()}, median_ms=ms(med), spread=spread,
                iw4_b256_vs_std_b1024={m: round(med['iw4_b256_' + m] / med['std_b1024_' + m] - 1, 4) for m in ('eager', 'graph')},
                iw4_b256_vs_std_b256={m: round(med['iw4_b256_' + m] / med['std_b256_' + m] - 1, 4) for m in ('eager', 'graph')})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=256)
    ap.add_argument('--T', type=int, default=16)
    ap.add_argument('--frame', type=int, default=784)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--min_window_s', type=float, default=0.3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--step', action='store_true', help='time whole training steps instead of the loss stage')
    ap.add_argument('--seed', type=int, default=121)
    ap.add_argument('--parent_lib', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_iw_loss.py measures on an MI355X: no GPU found, nothing measured')
    out = whole_step(a, torch) if a.step else loss_stage(a, torch)
    txt = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')
    print(txt)


if __name__ == '__main__':
    main()
