"""Index helpers for the lane-major pack layout (csrc/gp_eval.hpp), used by the tests to read gradients
that the HIP kernels return in pack layout."""
import math

import torch


def cdiv(a, b):
    return (a + b - 1) // b


class PackView:
    def __init__(self, kernel, Di, Do, M, S):
        self.kernel, self.Di, self.Do, self.M, self.S = kernel, Di, Do, M, S
        self.SJ, self.MJ = cdiv(S, 64), cdiv(M, 64)
        if kernel == 'RBF':
            self.RQ, self.RQ2 = cdiv(Di + 2, 4), cdiv(Di + Do, 4)
            self.nuni = Do * Di
        else:
            self.RQ, self.RQ2 = cdiv(2 * Do + 3, 4), cdiv(2 * Do, 4)
            self.nuni = 2 * Do * Do + Do
        self.rff_f4 = self.SJ * Do * self.RQ * 64
        self.ind_f4 = self.MJ * self.RQ2 * 64

    def rff(self, g):
        """-> (S, Do_or_D, 4*RQ): record fields for feature s and record index d (RBF) / i (DF)."""
        t = g[:4 * self.rff_f4].view(self.SJ, self.Do, self.RQ, 64, 4)       # j, d, q, lane, comp
        t = t.permute(0, 3, 1, 2, 4).reshape(self.SJ * 64, self.Do, self.RQ * 4)  # s, d, field
        return t[:self.S]

    def ind(self, g):
        """-> (M, 4*RQ2): record fields for inducing point m."""
        t = g[4 * self.rff_f4:4 * (self.rff_f4 + self.ind_f4)].view(self.MJ, self.RQ2, 64, 4)
        t = t.permute(0, 2, 1, 3).reshape(self.MJ * 64, self.RQ2 * 4)
        return t[:self.M]

    def uni(self, g):
        o = 4 * (self.rff_f4 + self.ind_f4)
        return g[o:o + self.nuni]


def leaf_grads(pv, gpack, c):
    """A pack-layout gradient (ops.param_grad) as the gradients w.r.t. the cache quantities the oracle differentiates as leaves:
    omega (Di,S,Do), var (Do), Z (M,Di), nu (RBF (Do,M,1); DF (M D,1)), ell (Do,Di), and for DF B (S,D,D), the sum of the cos and
    sin halves of df_B_omega's gradient (they share B).  c: the cache the pack was built from (var, ell, nu, w, omega), in the
    precision the result is wanted in.  The record fields are listed in csrc/gp_eval.hpp."""
    from oracle import gpode_oracle as O
    rff, ind, uni = pv.rff(gpack), pv.ind(gpack), pv.uni(gpack)
    Di, Do, S = pv.Di, pv.Do, pv.S
    var, ell, nu = c['var'], c['ell'], c['nu']
    if pv.kernel == 'RBF':
        aw = torch.sqrt(var / S) * c['w']                                    # (S,Do)
        return dict(omega=rff[:, :, :Di].permute(2, 0, 1) / (2 * math.pi),   # (Di,S,Do)
                    var=(rff[:, :, Di + 1] * aw / (2 * var)).sum(0) + (ind[:, Di:Di + Do] * nu.squeeze(2).T).sum(0),
                    Z=ind[:, :Di], nu=(ind[:, Di:Di + Do] * var).T.unsqueeze(2),
                    ell=uni.view(Do, Di) * math.log2(math.e) / ell ** 3)
    D = Do
    # rff record (s,i): fields [om_k (D), ph, wc, ws, bs_j (D)]
    sc = torch.sqrt(var / S)                                                 # per column j
    wab, il2, gvar = uni[:D * D].view(D, D), uni[D * D:2 * D * D].view(D, D), uni[2 * D * D:]
    bs = O.df_B_omega(c['omega'])[:S] * sc
    return dict(omega=rff[:, :, :D].permute(2, 0, 1) / (2 * math.pi),        # [k, s, i]
                B=rff[:, :, D + 3:2 * D + 3] * sc,                           # (S, i, j)
                Z=ind[:, :D], nu=ind[:, D:2 * D].reshape(-1, 1),
                # wab = -log2e/(2 l^2), il2 = 1/l^2
                ell=wab * math.log2(math.e) / ell ** 3 + il2 * (-2.0) / ell ** 3,
                var=gvar + (rff[:, :, D + 3:2 * D + 3] * bs / (2 * var)).sum((0, 1)))
