"""The refusal transcript of the conv, loss-stage and evaluation exports: return code and gpode_last_error() text, as literals.

Every case calls the library directly (_lib.load()) with arguments that the entry point refuses BEFORE its first HIP runtime call, so
nothing is launched and the cases run without a GPU.  The cases of one export walk its refusals in the order of the checks: each case
repairs what the one before it was refused for and meets the next.  The literals were written from the build in front of the change that
moved these exports to argument structs and hold unchanged after it: the texts, the codes and the order are part of the ABI.

Covered: gpode_conv2d_* and gpode_convT_fwd_stats, gpode_sigmoid_loglik_*, gpode_loglik_rowsum_*_len, gpode_elbo_all_*, gpode_elbo_iw_*,
gpode_gather_frames_*, gpode_dec10_predict*.  A limit that repeats a text (nsplit < 1 and rows > 65535, K < 1 and K > 64) is met once.

Not covered, because the text comes after (or from) a HIP runtime call and so depends on the machine:
  gpode_convT_fwd_stats: "no ticket storage" (hipGetSymbolAddress), "slot 0 .. 63", "no specialisation for this geometry", and the
      "... needs the matrix-core path" refusals of the statistics-producing arms, all behind the ticket lookup;
  every "<tag>: launch failed: ..." and "hipFuncSetAttribute(...)" text.

Non-null pointers are addresses inside one host buffer.  On a machine with a GPU a refusal that got lost would therefore launch a kernel
on host memory, so the module is skipped there; tests/test_gpu_loss_routes.py, test_gpu_conv_dispatch.py, test_gpu_ragged_*.py,
test_gpu_iw_loss.py and test_gpu_eval*.py hold the same paths on the GPU by launch tag and result."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from vae_gp_ode_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason='the pointers are host addresses: with a GPU present a refusal that got '
                                'lost would launch a kernel on host memory (the GPU route tests cover these paths)')

_BUF = ctypes.create_string_buffer(4096)
P = (ctypes.addressof(_BUF) + 63) & ~63              # a 16-byte aligned address
Q = P + 4                                            # one that is not
G_ODD = (2, 3, 8, 8, 4, 7, 1, 0, 2, 2)               # B, Ci, H, W, Co, K, S, P, Ho, Wo: no specialisation, kernel size 7 is not built
G_CI4 = (2, 4, 8, 8, 4, 7, 1, 0, 2, 2)               # the same with input channels a multiple of 4
G_DEC7 = (2, 16, 28, 28, 32, 5, 2, 1, 13, 13)        # decnn.7 as the convolution it is the adjoint of
FUSED_FWD = 'convT forward with a fused BatchNorm input needs the matrix-core path (16-byte aligned operands, GPODE_CONV_VALU unset)'
FUSED_WGRAD = 'convT weight gradient with a fused BatchNorm input needs the matrix-core path (16-byte aligned operands, GPODE_CONV_VALU unset)'
LEN_NOBS, LEN_INNER = 'n_obs is NULL', 'inner must be T * frame'
LEN_WHOLE = 'X must hold a whole number of sequences (nX a multiple of inner)'
PK_INDEX, PK_FRAME = 'the frame index is NULL', 'T >= 1 and frame a positive multiple of 4'
PK_WHOLE = 'X must hold a whole number of sequences (nX a multiple of T * frame)'
PK_ROWS = 'rows must be a multiple of the number of sequences'
IW = ('1 <= K <= 64 (one lane of a wavefront per draw)', 'L, N, M, Do >= 1', 'nsplit >= 1',
      'rows <= 65535 (the grid of gpode_sigmoid_loglik_fwd)', 'rows = L * K * N')
IW_ARGS = ((4, 1, P, 1, 0, 4, 3, 2), (4, 1, P, 0, 2, 2, 3, 2), (4, 0, P, 1, 2, 2, 3, 2), (65536, 1, P, 1, 2, 2, 3, 2),
           (5, 1, P, 1, 2, 2, 3, 2))                 # rows, nsplit, lw, L, K, N, M, Do: one per text of IW
PRED_SIZES = 'need Lc, F >= 1, 1 <= T_obs <= Th, F a multiple of Th, done >= 0'
G4 = (P, P, P, P)                                    # the four upstream gradients
G5 = (P, P, P, P, P)


def _cases():
    c = []

    def add(name, args, text):
        c.append((name, args, '%s: %s' % (name, text) if not text.startswith(('gpode_', 'convT ')) else text))

    # ---- convolutions
    add('gpode_conv2d_fwd', (0, P, 0, P) + G_ODD + (0,), 'null pointer')
    add('gpode_conv2d_fwd', (P, P, 0, P) + G_ODD + (0,), 'kernel 7 stride 1 not built')
    add('gpode_conv2d_fwd_bs', (P, 200, P, 0, 0) + G_ODD + (0,), 'null pointer')
    add('gpode_conv2d_fwd_bs', (P, 10, P, 0, P) + G_ODD + (0,), 'images overlap')
    add('gpode_conv2d_fwd_bs', (P, 260, P, 0, P) + G_CI4 + (0,),
        'batch-strided input is for the generic kernels (input channels not a multiple of 4)')
    add('gpode_conv2d_fwd_bs', (P, 200, P, 0, P) + G_ODD + (0,), 'gpode_conv2d_fwd: kernel 7 stride 1 not built')
    add('gpode_conv2d_bwd_data', (P, 0, 0, P) + G_ODD + (0,), 'null pointer')
    add('gpode_conv2d_bwd_data', (P, P, 0, P) + G_ODD + (0,), 'kernel 7 stride 1 not built')
    add('gpode_conv2d_bwd_data_bn', (P, 0, P, 0, P) + G_ODD + (0,), 'null pointer')
    add('gpode_conv2d_bwd_data_bn', (P, P, P, 0, P) + G_ODD + (0,), 'no matrix-core specialisation for this geometry')
    add('gpode_conv2d_bwd_data_bn', (Q, P, P, 0, P) + G_DEC7 + (0,), FUSED_FWD)
    add('gpode_conv2d_bwd_weight', (P, P, P, 0, 0) + G_ODD + (0,), 'null pointer')
    add('gpode_conv2d_bwd_weight', (P, Q, P, P, P) + G_ODD + (0,), 'the bias gradient needs a 16-byte aligned gy')
    add('gpode_conv2d_bwd_weight', (P, P, P, P, P) + G_ODD + (0,), 'kernel 7 stride 1 not built')
    add('gpode_conv2d_bwd_weight_bs', (P, 200, 0, P, 0, P) + G_ODD + (0,), 'null pointer')
    add('gpode_conv2d_bwd_weight_bs', (P, 10, P, P, 0, P) + G_ODD + (0,), 'images overlap')
    add('gpode_conv2d_bwd_weight_bs', (P, 260, P, P, 0, P) + G_CI4 + (0,), 'batch-strided input is for the generic kernels')
    add('gpode_conv2d_bwd_weight_bs', (P, 200, P, P, 0, P) + G_ODD + (0,), 'gpode_conv2d_bwd_weight: kernel 7 stride 1 not built')
    add('gpode_conv2d_bwd_weight_bn', (P, P, 0, P, 0, P) + G_ODD + (0,), 'null pointer')
    add('gpode_conv2d_bwd_weight_bn', (P, P, P, P, 0, P) + G_ODD + (0,), 'no matrix-core specialisation for this geometry')
    add('gpode_conv2d_bwd_weight_bn', (Q, P, P, P, 0, P) + G_DEC7 + (0,), FUSED_WGRAD)
    stats_tail = (P, P, P, P)                        # gamma, beta, save_mean, save_invstd
    add('gpode_convT_fwd_stats', (0, 0, P, 0, P) + G_DEC7 + stats_tail + (0, 0, 0, 0.1, 1e-5, P, P, 0, 0), 'null pointer')
    add('gpode_convT_fwd_stats', (P, 0, P, 0, P) + G_DEC7 + stats_tail + (P, 0, 0, 0.1, 1e-5, P, P, 0, 0),
        'running_mean and running_var go together')

    # ---- the likelihood over padded rows: X, a|z, z|grow, part|ga, rows, inner, nX[, nsplit][, n_obs, T, frame]
    add('gpode_sigmoid_loglik_fwd', (P, P, P, 0, 2, 8, 16, 1, 0), 'null pointer')
    add('gpode_sigmoid_loglik_fwd', (P, P, P, P, 0, 8, 16, 1, 0), 'empty input')
    add('gpode_sigmoid_loglik_fwd', (P, P, P, P, 2, 8, 16, 0, 0), 'nsplit >= 1, rows <= 65535')
    add('gpode_sigmoid_loglik_fwd', (P, P, P, P, 3, 8, 16, 1, 0), 'X must tile the rows')
    add('gpode_sigmoid_loglik_bwd', (P, P, P, 0, 2, 8, 16, 0), 'null pointer')
    add('gpode_sigmoid_loglik_bwd', (P, P, P, P, 2, 0, 16, 0), 'empty input')
    add('gpode_sigmoid_loglik_fwd_len', (0, P, P, P, 2, 8, 16, 1, P, 2, 4, 0), 'null pointer')
    add('gpode_sigmoid_loglik_fwd_len', (P, P, P, P, 2, 8, 0, 1, P, 2, 4, 0), 'empty input')
    add('gpode_sigmoid_loglik_fwd_len', (P, P, P, P, 65536, 8, 16, 1, P, 2, 4, 0), 'nsplit >= 1, rows <= 65535')
    add('gpode_sigmoid_loglik_fwd_len', (P, P, P, P, 2, 8, 16, 1, 0, 2, 4, 0), LEN_NOBS)
    add('gpode_sigmoid_loglik_fwd_len', (P, P, P, P, 2, 8, 16, 1, P, 2, 3, 0), LEN_INNER)
    add('gpode_sigmoid_loglik_fwd_len', (P, P, P, P, 2, 8, 12, 1, P, 2, 4, 0), LEN_WHOLE)
    add('gpode_sigmoid_loglik_fwd_len', (P, P, P, P, 3, 8, 16, 1, P, 2, 4, 0), 'X must tile the rows')
    add('gpode_sigmoid_loglik_bwd_len', (P, P, 0, P, 2, 8, 16, P, 2, 4, 0), 'null pointer')
    add('gpode_sigmoid_loglik_bwd_len', (P, P, P, P, 0, 8, 16, P, 2, 4, 0), 'empty input')
    add('gpode_sigmoid_loglik_bwd_len', (P, P, P, P, 2, 8, 16, 0, 2, 4, 0), LEN_NOBS)
    add('gpode_sigmoid_loglik_bwd_len', (P, P, P, P, 2, 8, 16, P, 0, 4, 0), LEN_INNER)
    add('gpode_sigmoid_loglik_bwd_len', (P, P, P, P, 2, 8, 4, P, 2, 4, 0), LEN_WHOLE)
    add('gpode_sigmoid_loglik_bwd_len', (P, P, P, P, 3, 8, 16, P, 2, 4, 0), 'X must tile the rows')
    add('gpode_loglik_rowsum_fwd_len', (P, 0, P, 2, 8, 16, P, 2, 4, 0), 'null pointer')
    add('gpode_loglik_rowsum_fwd_len', (P, P, P, 2, 0, 16, P, 2, 4, 0), 'empty input')
    add('gpode_loglik_rowsum_fwd_len', (P, P, P, 2, 8, 16, 0, 2, 4, 0), LEN_NOBS)
    add('gpode_loglik_rowsum_fwd_len', (P, P, P, 2, 8, 16, P, 2, 0, 0), LEN_INNER)
    add('gpode_loglik_rowsum_fwd_len', (P, P, P, 2, 8, 12, P, 2, 4, 0), LEN_WHOLE)
    add('gpode_loglik_rowsum_fwd_len', (P, P, P, 3, 8, 16, P, 2, 4, 0), 'X must tile the rows')
    add('gpode_loglik_rowsum_bwd_len', (P, P, P, 0, 2, 8, 16, P, 2, 4, 0), 'null pointer')
    add('gpode_loglik_rowsum_bwd_len', (P, P, P, P, 2, 8, 0, P, 2, 4, 0), 'empty input')
    add('gpode_loglik_rowsum_bwd_len', (P, P, P, P, 2, 8, 16, 0, 2, 4, 0), LEN_NOBS)
    add('gpode_loglik_rowsum_bwd_len', (P, P, P, P, 2, 8, 16, P, 4, 4, 0), LEN_INNER)
    add('gpode_loglik_rowsum_bwd_len', (P, P, P, P, 2, 8, 12, P, 2, 4, 0), LEN_WHOLE)
    add('gpode_loglik_rowsum_bwd_len', (P, P, P, P, 3, 8, 16, P, 2, 4, 0), 'X must tile the rows')

    # ---- the likelihood over compact rows.  fwd: X, a, z, part, rows, off, T, frame, nX, nsplit; bwd: X, z, grow, ga, rows, src, P, T, frame, nX
    add('gpode_sigmoid_loglik_fwd_pk', (P, 0, P, P, 2, P, 2, 4, 16, 1, 0), 'null pointer')
    add('gpode_sigmoid_loglik_fwd_pk', (P, P, P, P, 0, P, 2, 4, 16, 1, 0), 'empty input')
    add('gpode_sigmoid_loglik_fwd_pk', (P, P, P, P, 2, P, 2, 4, 16, 0, 0), 'nsplit >= 1, rows <= 65535')
    add('gpode_sigmoid_loglik_fwd_pk', (P, P, P, P, 2, 0, 2, 4, 16, 1, 0), PK_INDEX)
    add('gpode_sigmoid_loglik_fwd_pk', (P, P, P, P, 2, P, 2, 6, 16, 1, 0), PK_FRAME)
    add('gpode_sigmoid_loglik_fwd_pk', (P, P, P, P, 2, P, 2, 4, 12, 1, 0), PK_WHOLE)
    add('gpode_sigmoid_loglik_fwd_pk', (P, P, P, P, 3, P, 2, 4, 16, 1, 0), PK_ROWS)
    add('gpode_sigmoid_loglik_bwd_pk', (P, P, P, 0, 2, P, 3, 2, 4, 16, 0), 'null pointer')
    add('gpode_sigmoid_loglik_bwd_pk', (P, P, P, P, 2, P, 3, 2, 4, 0, 0), 'empty input')
    add('gpode_sigmoid_loglik_bwd_pk', (P, P, P, P, 2, 0, 3, 2, 4, 16, 0), PK_INDEX)
    add('gpode_sigmoid_loglik_bwd_pk', (P, P, P, P, 2, P, 3, 0, 4, 16, 0), PK_FRAME)
    add('gpode_sigmoid_loglik_bwd_pk', (P, P, P, P, 2, P, 3, 2, 4, 12, 0), PK_WHOLE)
    add('gpode_sigmoid_loglik_bwd_pk', (P, P, P, P, 3, P, 3, 2, 4, 16, 0), PK_ROWS)
    add('gpode_sigmoid_loglik_bwd_pk', (P, P, P, P, 2, P, 5, 2, 4, 16, 0), '1 <= P <= N * T')
    add('gpode_gather_frames_fwd', (P, 8, 6, P, 1, 2, 2, 3, 0, 0), 'null pointer')
    add('gpode_gather_frames_fwd', (P, 8, 6, 0, 1, 2, 2, 3, P, 0), 'the frame index is NULL')
    add('gpode_gather_frames_fwd', (P, 8, 9, P, 1, 2, 2, 3, P, 0), '1 <= q <= ld')
    add('gpode_gather_frames_fwd', (P, 8, 6, P, 1, 2, 2, 5, P, 0), 'L, N, T >= 1 and 1 <= P <= N * T')
    add('gpode_gather_frames_bwd', (0, 8, 6, P, P, 1, 2, 2, 3, P, 0), 'null pointer')
    add('gpode_gather_frames_bwd', (P, 8, 6, P, 0, 1, 2, 2, 3, P, 0), 'the frame index is NULL')
    add('gpode_gather_frames_bwd', (P, 8, 0, P, P, 1, 2, 2, 3, P, 0), '1 <= q <= ld')
    add('gpode_gather_frames_bwd', (P, 8, 6, P, P, 0, 2, 2, 3, P, 0), 'L, N, T >= 1 and 1 <= P <= N * T')

    # ---- the ELBO in one launch.  heads: lpart | g0..g3, nl_rows[, nl_values], hs, hv, N, q, M, Do, Um, Us, nobs, ...
    add('gpode_elbo_all_fwd', (P, 4, 4, 0, 0, 2, 3, 4, 3, P, P, 1.0, P, 0), 'null pointer')
    add('gpode_elbo_all_fwd', (P, 4, 3, P, 0, 2, 3, 4, 3, P, P, 1.0, P, 0), 'bad sizes')
    add('gpode_elbo_all_fwd_kl', (P, 4, 4, 0, 2, 0, 0, 2, 4, 3, P, P, 1.0, P, 0), 'null pointer')
    add('gpode_elbo_all_fwd_kl', (P, 4, 4, P, 2, 0, 1, 2, 4, 3, P, P, 1.0, P, 0), 'null pointer')
    add('gpode_elbo_all_fwd_kl', (P, 4, 4, P, 0, 0, 0, 2, 4, 3, P, P, 1.0, P, 0), 'bad sizes')
    add('gpode_elbo_all_fwd_kl', (P, 4, 4, P, 2, 0, -1, 2, 4, 3, P, P, 1.0, P, 0), 'bad sizes')
    heads = (4, P, P, 2, 3, 4, 3, P, P, 1.0)         # nl_rows, hs, hv, N, q, M, Do, Um, Us, nobs
    add('gpode_elbo_all_bwd', G4 + heads + (P, P, 0, P, P, 0), 'null pointer')
    add('gpode_elbo_all_bwd', G4 + (4, P, P, 2, 0, 4, 3, P, P, 1.0) + (P, P, P, P, P, 0), 'bad sizes')
    add('gpode_elbo_all_bwd_ll', G4 + heads + (P, P, P, P, P, P, P, 0, 24, 12, 0), 'null pointer')
    add('gpode_elbo_all_bwd_ll', G4 + heads + (P, P, P, P, P, P, P, P, 25, 12, 0), 'bad sizes')
    add('gpode_elbo_all_bwd_ll_len', G4 + heads + (P, 0, P, P, P, P, P, P, 32, 16, P, 2, 4, 0), 'null pointer')
    add('gpode_elbo_all_bwd_ll_len', G4 + heads + (P, P, P, P, P, P, P, P, 32, 0, P, 2, 4, 0), 'bad sizes')
    add('gpode_elbo_all_bwd_ll_len', G4 + heads + (P, P, P, P, P, P, P, P, 32, 16, 0, 2, 4, 0), LEN_NOBS)
    add('gpode_elbo_all_bwd_ll_len', G4 + heads + (P, P, P, P, P, P, P, P, 32, 16, P, 0, 4, 0), LEN_INNER)
    add('gpode_elbo_all_bwd_ll_len', G4 + heads + (P, P, P, P, P, P, P, P, 24, 12, P, 2, 4, 0), LEN_WHOLE)
    vals = (4, 2, 4, 3, P, P, 1.0)                   # nl_rows, N, M, Do, Um, Us, nobs; then glrow, gkls, nks, gklv, nkv, dUm, dUs, X, z, ga, n, nX
    add('gpode_elbo_all_bwd_ll_kl', G4 + vals + (P, 0, 2, 0, 0, P, P, P, P, P, 24, 12, 0), 'null pointer')
    add('gpode_elbo_all_bwd_ll_kl', G4 + vals + (P, P, 2, 0, 1, P, P, P, P, P, 24, 12, 0), 'null pointer')
    add('gpode_elbo_all_bwd_ll_kl', G4 + vals + (P, P, 0, 0, 0, P, P, P, P, P, 24, 12, 0), 'bad sizes')
    add('gpode_elbo_all_bwd_ll_kl_len', G4 + vals + (P, P, 2, 0, 0, P, 0, P, P, P, 32, 16, P, 2, 4, 0), 'null pointer')
    add('gpode_elbo_all_bwd_ll_kl_len', G4 + vals + (P, P, 2, 0, 0, P, P, P, P, P, 0, 16, P, 2, 4, 0), 'bad sizes')
    add('gpode_elbo_all_bwd_ll_kl_len', G4 + vals + (P, P, 2, 0, 0, P, P, P, P, P, 32, 16, 0, 2, 4, 0), LEN_NOBS)
    add('gpode_elbo_all_bwd_ll_kl_len', G4 + vals + (P, P, 2, 0, 0, P, P, P, P, P, 32, 16, P, 2, 0, 0), LEN_INNER)
    add('gpode_elbo_all_bwd_ll_kl_len', G4 + vals + (P, P, 2, 0, 0, P, P, P, P, P, 24, 12, P, 2, 4, 0), LEN_WHOLE)

    # ---- the importance-weighted bound: [g0..g4,] lpart, rows, nsplit, lw, L, K, N, M, Do, Um, Us, nobs, ...
    add('gpode_elbo_iw_fwd', (P, 4, 1, 0, 1, 2, 2, 3, 2, P, P, 1.0, P, 0), 'null pointer')
    add('gpode_elbo_iw_bwd', G5 + (P, 4, 1, P, 1, 2, 2, 3, 2, P, P, 1.0, P, 0, P, P, 0), 'null pointer')
    add('gpode_elbo_iw_bwd_ll', G5 + (P, 4, 1, P, 1, 2, 2, 3, 2, P, P, 1.0, P, P, P, P, P, P, 0, 8, 8, 0), 'null pointer')
    for a, text in zip(IW_ARGS, IW):
        add('gpode_elbo_iw_fwd', (P,) + a + (P, P, 1.0, P, 0), text)
        add('gpode_elbo_iw_bwd', G5 + (P,) + a + (P, P, 1.0, P, P, P, P, 0), text)
        add('gpode_elbo_iw_bwd_ll', G5 + (P,) + a + (P, P, 1.0, P, P, P, P, P, P, P, 8, 8, 0), text)
    add('gpode_elbo_iw_bwd_ll', G5 + (P, 4, 1, P, 1, 2, 2, 3, 2, P, P, 1.0, P, P, P, P, P, P, P, 7, 7, 0),
        'the logits must be whole rows and X must tile them')
    add('gpode_elbo_iw_bwd_ll', G5 + (P, 65535, 1, P, 1, 1, 65535, 3, 2, P, P, 1.0, P, P, P, P, P, P, P, 65535 << 26, 65535 << 26, 0),
        'too many logits for one launch')

    # ---- the evaluation epilogue: c, table, w, bias, X, Lc, F, Th, T_obs, done, pred_mean, pred_m2, se_state[, ell, L_total][, n_obs]
    for name, tail, extra in (('gpode_dec10_predict', (), ()), ('gpode_dec10_predict_ll', (P, 4), (('ell is NULL', (0, 4)), ('ell has L_total rows, need done + Lc <= L_total', (P, 3)))),
                              ('gpode_dec10_predict_len', (P,), ((LEN_NOBS, (0,)),)),
                              ('gpode_dec10_predict_ll_len', (P, 4, P), (('ell is NULL', (0, 4, P)), ('ell has L_total rows, need done + Lc <= L_total', (P, 3, P)),
                                                                         (LEN_NOBS, (P, 4, 0))))):
        add(name, (P, P, P, 0, P, 2, 6, 3, 2, 2, P, P, 0) + tail + (0,), 'null pointer')
        add(name, (P, P, P, 0, P, 2, 6, 3, 4, 2, P, P, P) + tail + (0,), PRED_SIZES)
        add(name, (P, P, P, 0, P, 2, 6, 3, 2, 2, P, 0, P) + tail + (0,), 'pred_mean and pred_m2 go together')
        add(name, (P, Q, P, 0, P, 2, 6, 3, 2, 2, P, P, P) + tail + (0,), 'the table must be 16-byte aligned')
        for text, t in extra:
            add(name, (P, P, P, 0, P, 2, 6, 3, 2, 2, P, P, P) + t + (0,), text)
    return c


CASES = _cases()
FAMILIES = ('gpode_conv2d_', 'gpode_convT_fwd_stats', 'gpode_sigmoid_loglik_', 'gpode_loglik_rowsum_', 'gpode_elbo_all_', 'gpode_elbo_iw_',
            'gpode_gather_frames_', 'gpode_dec10_predict')


@pytest.mark.parametrize('name,args,text', CASES, ids=['%s-%d' % (c[0][6:], i) for i, c in enumerate(CASES)])
def test_refusal_text_and_code(name, args, text):
    lib = _lib.load()
    assert getattr(lib, name)(*args) == 1
    assert lib.gpode_last_error().decode() == text


def test_every_family_is_met_and_no_text_is_the_runtimes():
    for fam in FAMILIES:
        assert any(c[0].startswith(fam) for c in CASES), fam
    for _, _, text in CASES:
        assert 'launch failed' not in text and 'hip' not in text.lower(), text
    assert len(set((c[0], c[1]) for c in CASES)) == len(CASES)


_VALU_SCRIPT = r'''
import importlib.util, sys
spec = importlib.util.spec_from_file_location('gpode_lib', sys.argv[1])
m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
lib = m.load()
for name, n in (('gpode_dec10_predict', 14), ('gpode_dec10_predict_ll', 16), ('gpode_dec10_predict_len', 15), ('gpode_dec10_predict_ll_len', 17)):
    args = [64] * 5 + [0] * 5 + [64] * (n - 11) + [0]        # bad sizes too: the switch is checked in front of them
    print(getattr(lib, name)(*args), lib.gpode_last_error().decode())
'''


def test_predict_refuses_the_vector_only_switch_first():
    """GPODE_CONV_VALU is read once per process, hence the child; it loads _lib.py by path, without the package and torch."""
    env = dict(os.environ, GPODE_CONV_VALU='1')
    out = subprocess.run([sys.executable, '-c', _VALU_SCRIPT, _lib.__file__], env=env, capture_output=True, text=True, check=True).stdout
    assert out.splitlines() == ['1 %s: matrix-core kernel only (GPODE_CONV_VALU is set)' % n for n in
                                ('gpode_dec10_predict', 'gpode_dec10_predict_ll', 'gpode_dec10_predict_len', 'gpode_dec10_predict_ll_len')]
