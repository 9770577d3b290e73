#!/usr/bin/env python3
"""Generate tests/golden/eval_*.npz: posterior-predictive evaluation by the REFERENCE's own modules in eval().

Run where the reference tree is present (it never travels), like make_golden.py whose stand-ins and helpers are reused:

    python tests/golden/make_golden_eval.py [NAME ...]

What is restated here, in this script's own words, is the evaluation routine of the reference's notebooks: model in eval(),
encode the first frame(s), draw L functions, integrate, decode, squared error against the targets, ``torch.mean`` and
``torch.std`` (unbiased) over every draw, sequence, frame and pixel; plus the mean and unbiased variance of the reconstructions
over the draws and the error per time step.  All model arithmetic is the reference's (ODEGPVAE.forward with its encoder,
sample_trajectories and build_decoding).

A freshly initialised model is a poor yardstick (its decoder output spans a few hundredths and the draws differ by 1e-6), so
each case first gets a signal: ``dt = 1``, inducing means perturbed by 3 randn, the raw inducing scale times 100, then three
training-mode passes that move every BatchNorm's running statistics away from (0, 1).  The script asserts per case that the peak
predictive variance is >= 1e-3 and that the reconstructions span >= 0.1, and prints both.

z-normalised random targets put the error near 1.4 whatever the decoder does; every case therefore also records the statistics
against a second target tensor X01 drawn in [0, 1].  Inflated dynamics amplify float32 differences in the integrator, which is not
what these fixtures are about: ``z0`` and ``ztL`` are recorded so that a test can feed the decoder the reference's own latents.

The ``*64`` entries are the same routine with the reference decoder and the reductions in float64 on the recorded float32
``ztL`` (the GP part stays float32): the distance float32 -> float64 of the reference itself calibrates the tests' bounds.
"""
import copy
import sys

import torch

import make_golden as G
from make_golden import npy


def _stats(Xrec, X, T, tag, out):
    """the notebook's reductions of the squared error, and the error per time step"""
    se = (Xrec[:, :, :T] - X.to(Xrec.dtype)[None]) ** 2
    out['mse' + tag], out['std' + tag] = npy(torch.mean(se)), npy(torch.std(se))
    out['mse_t' + tag] = npy(se.mean(dim=(0, 1, 3, 4, 5)))
    return se


def eval_case(name, kernel, order, q, seed, T_custom=None, L=3, N=2, T=6, M=8, S=16):
    model = G.build(kernel, order, M, S, q, 'rk4', seed, uniform_hyper=False)
    gp = model.flow.odefunc.diffeq
    g = torch.Generator().manual_seed(seed + 21)
    with torch.no_grad():
        model.dt = 1.0
        gp.Um.optvar.add_(3.0 * torch.randn(gp.Um.optvar.shape, generator=g))
        gp.Us_sqrt.optvar.mul_(100.0)
    G.patch(G.Recorder(seed + 23))
    model.train()
    with torch.no_grad():
        for _ in range(3):           # running statistics away from (0, 1); these draws are not recorded
            model((torch.rand(N, T, 1, 28, 28, generator=g) - 0.1307) / 0.3081, 1)
    model.eval()
    sd = {k: npy(v).copy() for k, v in model.state_dict().items()}
    rec = G.Recorder(seed + 11)
    G.patch(rec)
    X = (torch.rand(N, T, 1, 28, 28, generator=g) - 0.1307) / 0.3081
    X01 = torch.rand(N, T, 1, 28, 28, generator=g)
    captured = {}
    orig = model.sample_trajectories

    def spy(z0, T_, L_=1):
        r = orig(z0, T_, L_)
        captured['z0'], captured['ztL'] = z0, r
        return r
    model.sample_trajectories = spy
    with torch.no_grad():
        Xrec, _, _ = model(X, L, T_custom) if T_custom else model(X, L)
    after = model.state_dict()
    for k, v in sd.items():          # eval(): no buffer moved (the solver's evaluation counter aside)
        assert 'num_evals' in k or (npy(after[k]) == v).all(), k
    n_enc = order
    assert all(k == 'randn_like' for k, _ in rec.log[:n_enc]) and len(rec.log) == n_enc + 4 * L
    out = {'sd.' + k: v for k, v in sd.items()}
    out['eps_s'] = npy(rec.log[0][1])
    if order == 2:
        out['eps_v'] = npy(rec.log[1][1])
    for l in range(L):
        nz = G.split_gp_noise(rec.log[n_enc + 4 * l:n_enc + 4 * l + 4], kernel)
        out.update({'noise%d.%s' % (l, k): npy(v) for k, v in nz.items()})
    ztL = captured['ztL']
    out.update(X=npy(X), X01=npy(X01), z0=npy(captured['z0']), ztL=npy(ztL), Xrec=npy(Xrec), dt=npy(torch.tensor(model.dt)))
    _stats(Xrec, X, T, '', out)
    _stats(Xrec, X01, T, '01', out)
    out['pmean'], out['pvar'] = npy(Xrec.mean(0)), npy(Xrec.var(0))
    # float64: decoder and reductions, on the float32 latents
    dec64 = copy.deepcopy(model.vae.decoder).double()
    lat = ztL if order == 1 else ztL[..., :ztL.shape[-1] // 2]
    with torch.no_grad():
        Xrec64 = dec64(lat.double()).view(Xrec.shape)
    out['Xrec64'] = npy(Xrec64)
    _stats(Xrec64, X.double(), T, '64', out)
    _stats(Xrec64, X01.double(), T, '01_64', out)
    out['pmean64'], out['pvar64'] = npy(Xrec64.mean(0)), npy(Xrec64.var(0))
    peak, span = float(Xrec.var(0).max()), float(Xrec.max() - Xrec.min())
    print('%s: peak predictive variance %.3e, span of Xrec %.3f, |ztL| max %.1f, mse %.6f std %.6f, mse01 %.6f std01 %.6f, '
          'Xrec f32-f64 %.2e, pvar f32-f64 %.2e of the peak'
          % (name, peak, span, float(ztL.abs().max()), float(out['mse']), float(out['std']), float(out['mse01']), float(out['std01']),
             float((Xrec.double() - Xrec64).abs().max() / Xrec64.abs().max()),
             float((Xrec.var(0).double() - Xrec64.var(0)).abs().max() / Xrec64.var(0).max())))
    assert peak >= 1e-3 and span >= 0.1, (name, peak, span)
    G.save_fixture(name, out)


if __name__ == '__main__':
    torch.set_num_threads(1)
    only = set(sys.argv[1:])
    for args, kw in [(('eval_rbf1', 'RBF', 1, 6, 501), {}),
                     (('eval_rbf2', 'RBF', 2, 3, 502), {}),
                     (('eval_df1', 'DF', 1, 6, 503), {}),
                     (('eval_rbf1_roll', 'RBF', 1, 6, 504), dict(T_custom=12))]:
        if not only or args[0] in only:
            eval_case(*args, **kw)
