"""ctypes binding of libgpode_hip.so (C ABI: include/gpode.h).

The product path has NO fallback: if the shared library is missing or a call fails, this module
raises.  Build it with ``python -c 'import __graft_entry__ as g; g.build()'`` or
``make -C vae-gp-ode_amd/csrc``.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libgpode_hip.so')

_vp = ctypes.c_void_p  # every pointer but the host out-parameters below; device pointers travel as integers
_i = ctypes.c_int
_f = ctypes.c_float
_sz = ctypes.c_size_t
_sz_p = ctypes.POINTER(_sz)

# name -> (restype, argtypes); mirrors include/gpode.h one to one
SIGNATURES = {
    'gpode_version': (ctypes.c_char_p, []),
    'gpode_last_error': (ctypes.c_char_p, []),
    'gpode_last_launch': (ctypes.c_char_p, []),
    'gpode_supported': (_i, [_i, _i, _i]),
    'gpode_cache_sizes': (_i, [_i, _i, _i, _i, _i, _sz_p, _sz_p]),
    'gpode_cache_build_fwd': (_i, [_i] * 5 + [_vp] * 20),
    'gpode_cache_bwd_sizes': (_i, [_i, _i, _i, _i, _i, _sz_p]),
    'gpode_cache_build_bwd': (_i, [_i] * 5 + [_vp] * 13 + [_i, _vp]),
    'gpode_cache_bwd_prepare': (_i, [_i] * 5 + [_vp] * 2 + [_vp]),
    'gpode_cache_info': (_i, [_vp, ctypes.POINTER(_i), _vp]),
    'gpode_cache_pivots': (_i, [_vp, ctypes.POINTER(_f), _vp]),
    'gpode_set_backward_solves': (_i, [_i]),
    'gpode_kernel_matrix': (_i, [_i, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp]),
    'gpode_conditional_ws': (_i, [_i, _i, _i, _i, _sz_p]),
    'gpode_conditional': (_i, [_i, _i, _i, _i] + [_vp] * 5 + [_i, _vp, _i] + [_vp] * 3 + [_vp]),
    # posterior moments of the divergence-free layer: defined by this entry (include/gpode.h), no reference line computes it
    'gpode_conditional_df_ws': (_i, [_i, _i, _i, _sz_p]),
    'gpode_conditional_df': (_i, [_i, _i, _i] + [_vp] * 6 + [_i] + [_vp] * 3 + [_vp]),
    'gpode_svgp_kl_fwd': (_i, [_i, _i, _vp, _vp, _vp, _vp]),
    'gpode_svgp_kl_bwd': (_i, [_i, _i] + [_vp] * 5 + [_vp]),
    'gpode_rhs_fwd': (_i, [_i] * 5 + [_vp, _vp, _i, _vp, _i, _vp]),
    'gpode_rollout_fwd': (_i, [_i] * 7 + [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    'gpode_rollout_bwd': (_i, [_i] * 7 + [_vp] * 4 + [_i, _i, _vp, _vp, _vp]),
    'gpode_rhs_vjp': (_i, [_i] * 5 + [_vp, _vp, _vp, _i, _vp, _vp]),
    # forward mode: J_f(x) v and the state-transition matrix of the fixed-grid rollout applied to K directions
    'gpode_rhs_jvp': (_i, [_i] * 6 + [_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _i, _vp]),
    'gpode_rollout_jvp': (_i, [_i] * 8 + [_vp, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    'gpode_param_grad': (_i, [_i] * 5 + [_vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp]),
    # Monte-Carlo draws batched into one call (a leading draw axis on every per-draw operand; `ndraws` follows S)
    'gpode_cache_sizes_n': (_i, [_i] * 6 + [_sz_p, _sz_p]),
    'gpode_cache_build_fwd_n': (_i, [_i] * 6 + [_vp] * 20),
    'gpode_rollout_fwd_n': (_i, [_i] * 8 + [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    'gpode_rollout_bwd_n': (_i, [_i] * 8 + [_vp] * 4 + [_i, _i, _vp, _vp, _vp]),
    'gpode_rollout_adaptive_fwd_n': (_i, [_i] * 8 + [_vp] * 3 + [_i, _i, _f, _f, _i] + [_vp] * 5 + [_vp]),
    'gpode_rollout_adaptive_bwd_n': (_i, [_i] * 8 + [_vp] * 5 + [_i, _i, _i, _vp, _vp, _vp]),
    'gpode_rollout_dense_fwd_n': (_i, [_i] * 8 + [_vp] * 3 + [_i, _i, _f, _f, _i] + [_vp] * 6 + [_vp]),
    'gpode_rollout_dense_bwd_n': (_i, [_i] * 8 + [_vp] * 6 + [_i, _i, _i, _vp, _vp, _vp]),
    # ... with an initial state per draw: the `_n` arguments plus `z0_per_draw` in front of the stream
    'gpode_rollout_fwd_nz': (_i, [_i] * 8 + [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp]),
    'gpode_rollout_adaptive_fwd_nz': (_i, [_i] * 8 + [_vp] * 3 + [_i, _i, _f, _f, _i] + [_vp] * 5 + [_i, _vp]),
    'gpode_rollout_dense_fwd_nz': (_i, [_i] * 8 + [_vp] * 3 + [_i, _i, _f, _f, _i] + [_vp] * 6 + [_i, _vp]),
    # ... with a time grid per trajectory: the twin's arguments plus `ts_per_traj` in front of the stream
    'gpode_rollout_fwd_nt': (_i, [_i] * 8 + [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp]),
    'gpode_rollout_adaptive_fwd_nt': (_i, [_i] * 8 + [_vp] * 3 + [_i, _i, _f, _f, _i] + [_vp] * 5 + [_i, _i, _vp]),
    'gpode_rollout_dense_fwd_nt': (_i, [_i] * 8 + [_vp] * 3 + [_i, _i, _f, _f, _i] + [_vp] * 6 + [_i, _i, _vp]),
    'gpode_rollout_bwd_nt': (_i, [_i] * 8 + [_vp] * 4 + [_i, _i, _vp, _vp, _i, _vp]),
    'gpode_rollout_bwd_pgrad_nt': (_i, [_i] * 8 + [_vp] * 4 + [_i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp]),
    'gpode_test_substep_kernels': (_i, [_i]),
    'gpode_rollout_fwd_ns': (_i, [_i] * 8 + [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _vp]),
    'gpode_rollout_bwd_ns': (_i, [_i] * 8 + [_vp] * 4 + [_i, _i, _vp, _vp, _i, _i, _vp]),
    'gpode_rollout_bwd_pgrad_ns': (_i, [_i] * 8 + [_vp] * 4 + [_i, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _vp]),
    'gpode_rollout_bwd_pgrad_chunks': (_i, [_i] * 8),
    'gpode_rollout_bwd_pgrad_n': (_i, [_i] * 8 + [_vp] * 4 + [_i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    'gpode_param_grad_n': (_i, [_i] * 6 + [_vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp]),
    'gpode_cache_bwd_sizes_n': (_i, [_i] * 6 + [_sz_p]),
    'gpode_cache_build_bwd_n': (_i, [_i] * 6 + [_vp] * 13 + [_i, _vp]),
    'gpode_cache_bwd_prepare_n': (_i, [_i] * 6 + [_vp] * 2 + [_vp]),
    # the kernel's own methods (kern.build_cache / sample_freq, kern.compute_nu, kern.f_update)
    'gpode_kern_scratch': (_sz, [_i] * 5),
    'gpode_kern_cache': (_i, [_i] * 4 + [_vp] * 8 + [_vp]),
    'gpode_compute_nu_ws': (_i, [_i] * 4 + [_sz_p]),
    'gpode_compute_nu': (_i, [_i] * 4 + [_vp] * 5 + [_vp]),
    'gpode_f_update': (_i, [_i] * 4 + [_vp] * 5 + [_i, _vp, _vp, _vp]),
    # the conv-VAE, the loss stage and the optimiser (vae_ops, optim)
    'gpode_conv2d_fwd': (_i, [_vp] * 4 + [_i] * 10 + [_vp]),
    'gpode_conv2d_bwd_data': (_i, [_vp] * 4 + [_i] * 10 + [_vp]),
    'gpode_conv2d_fwd_bs': (_i, [_vp, _sz] + [_vp] * 3 + [_i] * 10 + [_vp]),
    'gpode_conv2d_bwd_weight_bs': (_i, [_vp, _sz] + [_vp] * 4 + [_i] * 10 + [_vp]),
    'gpode_convT_fwd_stats_scratch': (_sz, [_i]),
    'gpode_convT_fwd_stats': (_i, [_vp] * 5 + [_i] * 10 + [_vp] * 6 + [_vp, _f, _f, _vp, _vp, _i, _vp]),
    'gpode_conv_wgrad_scratch': (_sz, [_i, _i, _i, _i]),
    'gpode_conv2d_bwd_weight': (_i, [_vp] * 5 + [_i] * 10 + [_vp]),
    'gpode_bn_scratch': (_sz, [_i, _i]),
    'gpode_bn_fwd': (_i, [_vp] * 8 + [_vp, _f, _f, _i, _i, _i, _i, _vp, _vp]),
    'gpode_bn_bwd': (_i, [_vp] * 10 + [_i, _i, _i, _i, _vp, _vp]),
    'gpode_conv2d_bwd_data_bn': (_i, [_vp] * 5 + [_i] * 10 + [_vp]),
    'gpode_conv2d_bwd_weight_bn': (_i, [_vp] * 6 + [_i] * 10 + [_vp]),
    'gpode_bn_stats': (_i, [_vp] * 7 + [_vp, _f, _f, _vp, _i, _i, _i, _vp, _vp]),
    'gpode_bn_moments': (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    'gpode_bn_finalize': (_i, [_vp, _i] + [_vp] * 6 + [_vp, _f, _f, _vp, _i, _vp]),
    'gpode_bn_apply': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'gpode_bn_bwd_sums': (_i, [_vp] * 7 + [_i, _i, _i, _i, _vp, _vp]),
    'gpode_bn_bwd_apply': (_i, [_vp] * 8 + [_i, _f] + [_vp] * 4 + [_i, _i, _i, _i, _vp, _vp]),
    'gpode_defer_reductions': (None, [_i]),
    'gpode_flush_reductions': (_i, [_vp]),
    'gpode_dec10_bn_scratch_floats': (_i, []),
    'gpode_dec10_bn_wgrad_scratch_floats': (_i, []),
    'gpode_dec10_bn_bwd_sums_wgrad': (_i, [_vp] * 10 + [_i, _vp, _vp, _vp]),
    'gpode_dec10_bn_bwd_sums': (_i, [_vp] * 8 + [_i, _vp, _vp]),
    'gpode_dec10_bn_bwd_apply': (_i, [_vp] * 9 + [_i, _f] + [_vp] * 4 + [_i, _vp, _vp]),
    'gpode_bn_eval': (_i, [_vp] * 6 + [_f, _vp, _i, _i, _i, _i, _vp]),
    'gpode_bn_eval_table': (_i, [_vp] * 4 + [_f, _vp, _i, _vp]),
    'gpode_dec10_predict': (_i, [_vp] * 5 + [_i] * 5 + [_vp] * 3 + [_vp]),
    'gpode_dec10_predict_ll': (_i, [_vp] * 5 + [_i] * 5 + [_vp] * 4 + [_i, _vp]),
    'gpode_chan_sum': (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    'gpode_act_fwd': (_i, [_vp, _vp, _sz, _i, _vp]),
    'gpode_act_bwd': (_i, [_vp, _vp, _vp, _sz, _i, _vp]),
    'gpode_linear_fwd': (_i, [_vp] * 4 + [_i, _i, _i, _vp]),
    'gpode_linear_bwd_scratch': (_sz, [_i, _i, _i]),
    'gpode_linear_bwd': (_i, [_vp] * 6 + [_i, _i, _i, _vp, _vp]),
    'gpode_linear_relu_fwd': (_i, [_vp] * 4 + [_i, _i, _i, _vp]),
    'gpode_linear_relu_bwd': (_i, [_vp] * 6 + [_i, _i, _i, _vp]),
    'gpode_loglik_fwd': (_i, [_vp] * 3 + [_sz, _sz, _vp]),
    'gpode_loglik_bwd': (_i, [_vp] * 4 + [_sz, _sz, _vp]),
    'gpode_loglik_rowsum_fwd': (_i, [_vp] * 3 + [_sz, _sz, _sz, _vp]),
    'gpode_noise_fill': (_i, [_vp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_ulonglong, _vp, _vp]),
    'gpode_reparam_kl_fwd': (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp]),
    'gpode_reparam_kl_bwd': (_i, [_vp] * 4 + [_i] + [_vp] * 3 + [_i, _i, _i, _vp]),
    'gpode_elbo_all_fwd_kl': (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _f, _vp, _vp]),
    'gpode_elbo_all_bwd_ll_kl': (_i, [_vp] * 4 + [_i, _i, _i, _i, _vp, _vp, _f, _vp, _vp, _i, _vp, _i] + [_vp] * 5 + [_sz, _sz, _vp]),
    'gpode_reparam_fwd': (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp]),
    'gpode_reparam_draws_fwd': (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp]),
    'gpode_reparam_bwd': (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp]),
    'gpode_normal_kl_fwd': (_i, [_vp, _vp, _i, _vp, _i, _i, _vp]),
    'gpode_normal_kl_bwd': (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp]),
    'gpode_sigmoid_loglik_splits': (_i, [_sz, _sz]),
    'gpode_sigmoid_loglik_fwd': (_i, [_vp] * 4 + [_sz, _sz, _sz, _i, _vp]),
    'gpode_sigmoid_loglik_bwd': (_i, [_vp] * 4 + [_sz, _sz, _sz, _vp]),
    'gpode_elbo_all_fwd': (_i, [_vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _f, _vp, _vp]),
    'gpode_elbo_all_bwd': (_i, [_vp] * 4 + [_i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _f] + [_vp] * 5 + [_vp]),
    'gpode_elbo_all_bwd_ll': (_i, [_vp] * 4 + [_i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _f] + [_vp] * 8 + [_sz, _sz, _vp]),
    'gpode_elbo_fwd': (_i, [_vp, _i, _vp, _i, _vp, _f, _vp, _vp]),
    'gpode_elbo_bwd': (_i, [_vp, _i, _i, _f, _vp, _vp, _vp, _vp]),
    'gpode_gather_multi': (_i, [_vp, _vp, _i, ctypes.c_longlong, _vp, _vp]),
    'gpode_adam_multi': (_i, [_vp, _vp, _vp, _vp, _vp, _i, ctypes.c_longlong, _f, _f, _f, _f, _i, _vp, _vp]),
    'gpode_loglik_rowsum_bwd': (_i, [_vp] * 4 + [_sz, _sz, _sz, _vp]),
    # ragged minibatches: the twins' arguments + n_obs (int32 device pointer) [+ T, frame]
    'gpode_sigmoid_loglik_fwd_len': (_i, [_vp] * 4 + [_sz, _sz, _sz, _i, _vp, _i, _sz, _vp]),
    'gpode_sigmoid_loglik_bwd_len': (_i, [_vp] * 4 + [_sz, _sz, _sz, _vp, _i, _sz, _vp]),
    'gpode_loglik_rowsum_fwd_len': (_i, [_vp] * 3 + [_sz, _sz, _sz, _vp, _i, _sz, _vp]),
    'gpode_loglik_rowsum_bwd_len': (_i, [_vp] * 4 + [_sz, _sz, _sz, _vp, _i, _sz, _vp]),
    'gpode_elbo_all_bwd_ll_len': (_i, [_vp] * 4 + [_i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _f] + [_vp] * 8 + [_sz, _sz, _vp, _i, _sz, _vp]),
    'gpode_elbo_all_bwd_ll_kl_len': (_i, [_vp] * 4 + [_i, _i, _i, _i, _vp, _vp, _f, _vp, _vp, _i, _vp, _i] + [_vp] * 5 + [_sz, _sz, _vp, _i, _sz, _vp]),
    # ragged minibatches, compact route: the frame gather in front of the decoder and the loss stage over compact logits
    'gpode_gather_frames_fwd': (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    'gpode_gather_frames_bwd': (_i, [_vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    'gpode_sigmoid_loglik_fwd_pk': (_i, [_vp] * 4 + [_sz, _vp, _i, _sz, _sz, _i, _vp]),
    'gpode_sigmoid_loglik_bwd_pk': (_i, [_vp] * 4 + [_sz, _vp, _i, _i, _sz, _sz, _vp]),
    # training on the importance-weighted bound: the adjoint of the K draws and the loss stage over (l,k,n) rows
    'gpode_reparam_draws_bwd': (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'gpode_elbo_iw_fwd': (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _f, _vp, _vp]),
    'gpode_elbo_iw_bwd': (_i, [_vp] * 5 + [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _f] + [_vp] * 4 + [_vp]),
    'gpode_elbo_iw_bwd_ll': (_i, [_vp] * 5 + [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _f] + [_vp] * 7 + [_sz, _sz, _vp]),
    'gpode_dec10_predict_len': (_i, [_vp] * 5 + [_i] * 5 + [_vp] * 3 + [_vp, _vp]),
    'gpode_dec10_predict_ll_len': (_i, [_vp] * 5 + [_i] * 5 + [_vp] * 4 + [_i, _vp, _vp]),
    # the importance-weighted twin: logw, L_total, N, wstate, pred_mean, pred_m2, wse, n_obs (may be null)
    'gpode_dec10_predict_w': (_i, [_vp] * 5 + [_i] * 5 + [_vp, _i, _i] + [_vp] * 5 + [_vp]),
}

_lib = None


class GpodeError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes library; raise if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GpodeError('libgpode_hip.so not found at %s -- build the HIP extension first '
                         '(__graft_entry__.build()); there is no CPU fallback' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def call(name, *args):
    """Invoke an int-returning entry point; raise GpodeError with the library's message on failure."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise GpodeError('%s failed (%d): %s' % (name, rc, lib.gpode_last_error().decode()))
    return rc
