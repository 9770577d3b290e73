"""Time the fused loss pair of a training step -- gpode_sigmoid_loglik_fwd + gpode_elbo_all_bwd_ll_kl -- against its ragged form
(the *_len entry points) at the benchmark shape: rows = 256 likelihood rows of inner = 16 x 784 logits.

    python tools/time_ragged_loss.py [--rows 256] [--T 16] [--frame 784] [--windows 7] [--min_window_s 0.5] [--parent_lib SO] [--out FILE.json]

Legs, timed in alternating windows on the same buffers (device events around `reps` pairs, reps sized so that a window lasts
--min_window_s; every leg warmed first); median and spread (max - min over the median) per leg:
  twin          the two unmasked launches
  len_full      the *_len launches with n_obs = T for every sequence (the same bits as twin: checked here on part and ga)
  len_ragged    the *_len launches with n_obs uniform in T/2 .. T (seeded)
  twin_parent   `twin` through the library of the parent commit given with --parent_lib (loaded next to this build's)
The bytes a pair must move (logits read, z written and read, ga written, X read twice) over the median time is printed as GB/s: both
kernels are streaming passes.  No GPU: nothing is measured and the tool says so."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=256)
    ap.add_argument('--N', type=int, default=256, help='sequences (rows / N draws)')
    ap.add_argument('--T', type=int, default=16)
    ap.add_argument('--frame', type=int, default=784)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--min_window_s', type=float, default=0.5)
    ap.add_argument('--seed', type=int, default=121)
    ap.add_argument('--parent_lib', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_ragged_loss.py measures on an MI355X: no GPU found, nothing measured')
    from vae_gp_ode_amd import _lib
    lib = _lib.load()
    libs = {'this': lib}
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name, (res, args) in _lib.SIGNATURES.items():
            if hasattr(parent, name):
                getattr(parent, name).restype, getattr(parent, name).argtypes = res, args
        libs['parent'] = parent
    rows, N, T, frame = a.rows, a.N, a.T, a.frame
    assert rows % N == 0
    inner, nX, n = T * frame, N * T * frame, rows * T * frame
    M, Do, nks = 100, 6, 6
    g = torch.Generator().manual_seed(a.seed)
    dev = 'cuda'
    X = ((torch.rand(nX, generator=g) - 0.1307) / 0.3081).to(dev)
    logits = ((torch.rand(n, generator=g) * 2 - 1) * 8.0).to(dev)
    Um = (0.5 * torch.randn(M, Do, generator=g)).to(dev)
    Us = (0.01 * torch.randn(Do, M * (M + 1) // 2, generator=g) + 0.5).to(dev)
    gs = [torch.tensor([v], device=dev) for v in (1.0, 0.0, 0.0, 0.0)]
    ns = lib.gpode_sigmoid_loglik_splits(rows, inner)
    new = lambda *s: torch.empty(*s, device=dev)
    z, part, ga = new(n), new(rows, ns), new(n)
    glrow, gkls, dUm, dUs = new(rows), new(nks), new(M, Do), new(Do, M * (M + 1) // 2)
    counts = {'full': torch.full((N,), T, dtype=torch.int32, device=dev),
              'ragged': torch.randint(T // 2, T + 1, (N,), generator=g).to(dev, torch.int32)}
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nobs = ctypes.c_float(360.0)

    def pair(which, n_obs=None):
        L = libs[which]
        sfx, extra = ('', ()) if n_obs is None else ('_len', (p(n_obs), T, frame))
        rc = getattr(L, 'gpode_sigmoid_loglik_fwd' + sfx)(p(X), p(logits), p(z), p(part), rows, inner, nX, ns, *extra, st())
        rc |= getattr(L, 'gpode_elbo_all_bwd_ll_kl' + sfx)(*[p(t) for t in gs], rows, N, M, Do, p(Um), p(Us), nobs, p(glrow), p(gkls), nks, None, 0,
                                                         p(dUm), p(dUs), p(X), p(z), p(ga), n, nX, *extra, st())
        if rc:
            raise SystemExit('launch refused: ' + L.gpode_last_error().decode())
    legs = [('twin', lambda: pair('this')), ('len_full', lambda: pair('this', counts['full'])),
            ('len_ragged', lambda: pair('this', counts['ragged']))]
    if a.parent_lib:
        legs.append(('twin_parent', lambda: pair('parent')))
    # the bit rule at this shape, before anything is timed
    pair('this')
    ref = (part.clone(), ga.clone(), z.clone())
    pair('this', counts['full'])
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(ref, (part, ga, z)))
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
    times = {name: [] for name, _ in legs}
    for _ in range(a.windows):
        for name, fn in legs:                          # alternating
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(reps[name]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps[name] * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    spread = {k: round((max(v) - min(v)) / med[k], 4) for k, v in times.items()}
    nbytes = 4 * (4 * n + 2 * n)                       # logits, z (written, read), ga; X read once per pass over the logits
    out = dict(rows=rows, N=N, T=T, frame=frame, inner=inner, nsplit=ns, device=torch.cuda.get_device_name(0), windows=a.windows,
               pairs_per_window=reps, us_per_pair={k: [round(t, 2) for t in v] for k, v in times.items()},
               median_us={k: round(v, 2) for k, v in med.items()}, spread=spread, bytes_per_pair=nbytes,
               GBps={k: round(nbytes / (v * 1e-6) / 1e9, 1) for k, v in med.items()}, full_lengths_bit_equal=same,
               observed_share_ragged=round(counts['ragged'].float().mean().item() / T, 4),
               len_full_vs_twin=round(med['len_full'] / med['twin'] - 1, 4), len_ragged_vs_twin=round(med['len_ragged'] / med['twin'] - 1, 4))
    if a.parent_lib:
        out['twin_vs_parent'] = round(med['twin'] / med['twin_parent'] - 1, 4)
        out['twin_vs_parent_allowed'] = max(spread['twin'], spread['twin_parent'])
    txt = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')
    print(txt)


if __name__ == '__main__':
    main()
