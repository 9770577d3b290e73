"""The importance-weighted bound in plain torch, shared by test_iw_host.py, test_gpu_iw_loss.py and test_gpu_iw_model.py.

Draw L functions f_l ~ q(f) and, per sequence n, K initial states z0_{k,n} ~ q(z0 | x_n) that the L functions share:
  lw[k,n]   = log p(z0_{k,n}) - log q(z0_{k,n} | x_n) = sum_i (eps^2 / 2 - z^2 / 2 + logvar / 2)     (the 2 pi terms cancel)
  ll[l,k,n] = the Bernoulli log-likelihood of sequence n under (z0_{k,n}, f_l), summed over its observed frames
  a[l,k,n]  = ll[l,k,n] + lw[k,n]
  iw[l,n]   = logsumexp_k a[l,k,n] - log K
  loss      = -(nobs mean_{l,n} iw[l,n] - kl_u),   kl_u = KL(q(u) || p(u))
  out       = [loss, -mean iw, -mean_{k,n} lw, kl_u, mean_{l,n} ess],   ess = (sum_k w)^2 / sum_k w^2, w = exp(a - max_k a)

Everything works in the dtype of its inputs: the tests evaluate it in float64 (the reference) and once more in float32 on the same values
(the distance between the two is the floor the kernels are held to).  Gradients come from autograd; the closed forms the kernels
implement are restated beside them."""
import math

import torch


# ---- the K draws ---------------------------------------------------------------------------------------------------------------------
def draws_forward(mu, logvar, eps):
    """mu, logvar (N,q), eps (K,N,q) -> z (K,N,q), lw (K,N)"""
    z = mu + torch.exp(0.5 * logvar) * eps
    return z, (0.5 * eps * eps - 0.5 * z * z + 0.5 * logvar).sum(-1)


def draws_grads(mu, logvar, eps, gz, glw):
    """(gmu, glogvar) of sum(gz z) + sum(glw lw) by autograd; gz / glw None = zero"""
    mu, logvar = mu.detach().clone().requires_grad_(True), logvar.detach().clone().requires_grad_(True)
    z, lw = draws_forward(mu, logvar, eps)
    total = mu.sum() * 0 + logvar.sum() * 0
    if gz is not None:
        total = total + (gz * z).sum()
    if glw is not None:
        total = total + (glw * lw).sum()
    total.backward()
    return mu.grad, logvar.grad


def draws_grads_closed_form(mu, logvar, eps, gz, glw):
    """what gpode_reparam_draws_bwd evaluates: gmu = sum_k (gz - glw z), glogvar = sum_k (gz sigma eps / 2 + glw (1/2 - z sigma eps / 2))"""
    sg = torch.exp(0.5 * logvar)
    z = mu + sg * eps
    gz = torch.zeros_like(eps) if gz is None else gz
    glw = torch.zeros_like(eps[..., 0]) if glw is None else glw
    g = glw[..., None]
    return (gz - g * z).sum(0), (gz * sg * eps / 2 + g * (0.5 - z * sg * eps / 2)).sum(0)


# ---- the bound -----------------------------------------------------------------------------------------------------------------------
def diag_index(M):
    return torch.tensor([m * (m + 1) // 2 + m for m in range(M)])


def svgp_kl(Um, Us, M):
    """KL(q(u) || N(0, I)) from Um (M,Do) and the packed lower triangles Us (Do, M(M+1)/2)"""
    d = Us[:, diag_index(M).to(Us.device)]
    return 0.5 * ((Us * Us).sum() + (Um * Um).sum() - torch.log(d * d).sum() - M * Um.shape[1])


def svgp_kl_abs(Um, Us, M):
    d = Us[:, diag_index(M).to(Us.device)]
    return 0.5 * ((Us * Us).sum() + (Um * Um).sum() + torch.log(d * d).abs().sum() + M * Um.shape[1])


def weights(ll, lw):
    """ll (L,K,N), lw (K,N) -> a, iw (L,N), softmax weights p (L,K,N), ess (L,N); the maximum over k subtracted before any exp"""
    a = ll + lw[None]
    top = a.max(dim=1, keepdim=True).values
    w = torch.exp(a - top)
    s1, s2 = w.sum(1), (w * w).sum(1)
    iw = top[:, 0] + torch.log(s1) - math.log(a.shape[1])
    return a, iw, w / s1[:, None], s1 * s1 / s2


def objective(ll, lw, Um, Us, M, nobs):
    """-> out (5,) = [loss, -mean iw, -mean lw, kl_u, mean ess]"""
    _, iw, _, ess = weights(ll, lw)
    ku = svgp_kl(Um, Us, M)
    miw = iw.mean()
    return torch.stack([-(miw * nobs - ku), -miw, -lw.mean(), ku, ess.mean()])


def rows_of(lpart, L, K, N):
    """the kernels' operand lpart (L K N, nsplit), rows ordered (l,k,n) -> ll (L,K,N)"""
    return lpart.sum(-1).view(L, K, N)


def objective_grads(lpart, lw, Um, Us, L, K, N, M, nobs, seeds):
    """autograd of sum_i seeds[i] out[i], i < 4 (the ess output carries no gradient) -> out, grow (L K N,), glw (K,N), dUm, dUs"""
    lp, w, um, us = (t.detach().clone().requires_grad_(True) for t in (lpart, lw, Um, Us))
    out = objective(rows_of(lp, L, K, N), w, um, us, M, nobs)
    sum(s * o for s, o in zip(seeds[:4], out[:4])).backward()
    return out.detach(), lp.grad[:, 0].clone(), w.grad, um.grad, us.grad


def stage_grads_closed_form(ll, lw, nobs, seeds):
    """what gpode_elbo_iw_bwd evaluates: grow = softmax_k(a) (-g0 nobs - g1) / (L N), glw = sum_l grow - g2 / (K N)"""
    L, K, N = ll.shape
    _, _, p, _ = weights(ll, lw)
    grow = p * (-seeds[0] * nobs - seeds[1]) / (L * N)
    return grow, grow.sum(0) - seeds[2] / (K * N)
