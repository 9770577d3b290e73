"""Time the training step on a ragged minibatch with the padded frames masked out of the likelihood (compute_loss(n_obs=)) against the
compact route that takes them out in front of the decoder (compute_loss(n_obs=, compact=True)), at the benchmark shape configs[1]
(ode1 DF q=6 M=100 S=256, batch 256, T 16), L = 1, frame counts uniform in 8..16 from a fixed seed.

    timeout -k 10 600 python tools/time_ragged_compact.py [--workload cfg2] [--windows 7] [--min_window_s 0.5] [--out FILE.json]

Legs, timed in alternating windows (a host clock around `reps` whole steps -- zero_grad, loss, backward, Adam -- that end in a device
synchronise; reps sized so that a window lasts --min_window_s; every leg warmed first); median and spread = (max - min) / median:
  masked_eager     n_obs alone, every launch eager: all N T frames are decoded
  compact_eager    compact=True, the counts read back from the device in every step (4 N bytes and a synchronisation)
  compact_counts   compact=True with counts= given on the host: nothing is read back
  masked_graph     the masked step replayed as one captured HIP graph (side-stream overlap on, as main.py --hip_graph runs it): for
                   context -- compact mode cannot be captured, its launch sizes follow the counts
The graph is captured first, on a model of its own, ahead of any eager step; the three eager legs share a second model built from the
same seed.  Run it under a time limit of its own, as above.  No GPU: nothing is measured and the tool says so."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg2')
    ap.add_argument('--kmin', type=int, default=8)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--min_window_s', type=float, default=0.5)
    ap.add_argument('--seed', type=int, default=121)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_ragged_compact.py measures on an MI355X: no GPU found, nothing measured')
    from bench import WORKLOADS, make_model_inputs
    from vae_gp_ode_amd import ops
    from vae_gp_ode_amd.graph import GraphedStep, device_generators
    from vae_gp_ode_amd.model.create_model import backward, compute_loss
    from vae_gp_ode_amd.optim import HipAdam
    w = WORKLOADS[a.workload]
    dev = torch.device('cuda')
    N, T, L = w['batch'], w['T'], 1
    counts = torch.randint(a.kmin, T + 1, (N,), generator=torch.Generator().manual_seed(a.seed + 5))
    host_counts = counts.tolist()
    n_obs = counts.to(dev, torch.int32)

    def inputs():
        model, X = make_model_inputs(w, a.seed, dev, 0)
        X = X.clone()
        for n, k in enumerate(host_counts):          # a padded target frame holds zeros, as data.utils.ragged_frames leaves it
            X[n, k:] = 0.0
        ts = (model.dt * torch.arange(T, dtype=torch.float32)).expand(N, T).contiguous()
        return model, X.to(dev), ts.to(dev), HipAdam(model.parameters(), lr=1e-6, bucketed=False)

    def make_step(model, X, ts, opt, **kw):
        def step():
            opt.zero_grad()
            loss, *_ = compute_loss(model, X, L, ts=ts, n_obs=n_obs, **kw)
            backward(loss)
            ops.join_side_stream()
            opt.step()
            return loss
        return step
    # the captured step first, ahead of any eager step of this process
    ops.set_overlap(True)
    mg, Xg, tg, og = inputs()
    graph = GraphedStep(make_step(mg, Xg, tg, og), generators=device_generators(mg), warmup=2)
    ops.set_overlap(False)
    me, Xe, te, oe = inputs()
    legs = [('masked_eager', make_step(me, Xe, te, oe)), ('compact_eager', make_step(me, Xe, te, oe, compact=True)),
            ('compact_counts', make_step(me, Xe, te, oe, compact=True, counts=host_counts)), ('masked_graph', graph)]
    reps, last = {}, {}
    for name, fn in legs:                             # warm every leg, then size its window
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            last[name] = fn()
        torch.cuda.synchronize()
        reps[name] = max(10, int(a.min_window_s / ((time.perf_counter() - t0) / 10)) + 1)
    times = {name: [] for name, _ in legs}
    for _ in range(a.windows):
        for name, fn in legs:                         # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                last[name] = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps[name] * 1e3)
    bad = [k for k, v in last.items() if not bool(torch.isfinite(v).all())]
    if bad:
        raise SystemExit('non-finite loss in %s' % bad)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    spread = {k: round((max(v) - min(v)) / med[k], 4) for k, v in times.items()}
    P = sum(host_counts)
    out = dict(workload=w['desc'], N=N, T=T, L=L, kmin=a.kmin, observed_frames=P, observed_share=round(P / (N * T), 4),
               device=torch.cuda.get_device_name(0), windows=a.windows, steps_per_window=reps,
               ms_per_step={k: [round(t, 4) for t in v] for k, v in times.items()}, median_ms={k: round(v, 4) for k, v in med.items()},
               spread=spread, loss={k: float(v.detach()) for k, v in last.items()},
               compact_eager_vs_masked_eager=round(med['compact_eager'] / med['masked_eager'] - 1, 4),
               compact_counts_vs_masked_eager=round(med['compact_counts'] / med['masked_eager'] - 1, 4),
               compact_counts_vs_masked_graph=round(med['compact_counts'] / med['masked_graph'] - 1, 4),
               readback_cost_ms=round(med['compact_eager'] - med['compact_counts'], 4))
    txt = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')
    print(txt)


if __name__ == '__main__':
    main()
