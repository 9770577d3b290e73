"""The entry points added after the route suites were written -- the importance-weighted stage (gpode_elbo_iw_fwd / _bwd / _bwd_ll,
gpode_reparam_draws_bwd), the ragged *_len loss kernels, the compact *_pk kernels with the frame gather, and the predict epilogue
(gpode_dec10_predict_len / _ll_len / _w) -- at the smallest shapes that send every loop of theirs past its first trip.  Shared by
test_gpu_late_routes.py and test_late_routes_host.py; the conventions are those of loss_routes.py: every output and scratch NaN-filled
and sized exactly with guard words behind it (loss_routes.Bufs), gpode_last_launch() read after every call, every case run twice and
required bit-identical.

A case is a named tuple of one of the families below; case_id(c) names it, loops(c) lists the (kernel, loop) pairs it sends past one
trip -- computed from the launcher arithmetic restated here, never asked of the library.

  IW    gpode_elbo_iw_fwd / _bwd: L, K, N, nsplit, M, Do                      reference: iw_ref in fp64, floor: iw_ref in fp32
  IWLL  gpode_elbo_iw_bwd_ll against gpode_elbo_iw_bwd + gpode_sigmoid_loglik_bwd (torch.equal): L, K, N, frame, T, M, Do
  DR    gpode_reparam_draws_bwd: K, N, q, layout (ldgz = q or 2q)             reference: iw_ref.draws_grads
  LEN   the six *_len entries next to their twins: L, N, T, frame, nsplit (0: the proposal), the operand one float off 16 bytes
  PK    gpode_sigmoid_loglik_fwd_pk / _bwd_pk at the LEN shape: L, N, T, frame, nsplit, misaligned operands
  PKB   gpode_sigmoid_loglik_bwd_pk past the grid cap: L, N, T, frame, misaligned operands
  GA    gpode_gather_frames_fwd / _bwd past the grid cap: L, N, T, q, ld
  PR    the predict epilogue at F = N Th > n frames: kind (len, ll_len, w, w_len), N

The references: nothing is compared with the kernel under test.  Bit identity is to the twin test_gpu_loss_routes.py and
test_gpu_eval.py hold to fp64; row sums are within loss_routes.TOL of the fp64 sum of the observed terms relative to the sum of their
absolute values (loss_routes.sll_short_rows for rows of <= 8 terms); IW outputs at most 4 x the fp32 restatement's distance from fp64,
the floor taken over the grid (test_gpu_iw_loss.py); weighted moments within cond_ref.FLOOR + 3 x the fp32 restatement's error;
predict statistics within 2e-4 (test_gpu_eval.py)."""
import collections
import ctypes
import functools

import torch
import torch.nn.functional as Fn

import iw_ref as W
import loss_routes as R
from cond_ref import FLOOR, guarded, relerr

F64, F32 = torch.float64, torch.float32
NOBS = R.NOBS
SEEDS = R.SEED_VALUES + (0.5,)                       # g0 .. g3, and a seed for the ess output that must change nothing
IW_SPAN = 2048                                       # kIwSpan
PREDICT_TOL = 2e-4                                   # test_gpu_eval.py
MAX_CUS = 256                                        # num_cus() clamps the CU count

IW = collections.namedtuple('IW', 'L K N ns M Do')
IWLL = collections.namedtuple('IWLL', 'L K N frame T M Do')
DR = collections.namedtuple('DR', 'K N q layout')
LEN = collections.namedtuple('LEN', 'L N T frame ns mis')
PK = collections.namedtuple('PK', 'L N T frame ns mis')
PKB = collections.namedtuple('PKB', 'L N T frame mis')
GA = collections.namedtuple('GA', 'L N T q ld')
PR = collections.namedtuple('PR', 'kind N')


def case_id(c):
    return type(c).__name__ + '-' + '-'.join(str(v) or 'none' for v in c)


# ---- the launcher arithmetic, restated (csrc/vae_loss.hip, csrc/vae_conv_tiled.hip) ---------------------------------------------------------
ew_grid, sigmoid_loglik_splits, us_in_parts = R.ew_grid, R.sigmoid_loglik_splits, R.us_in_parts


def ceil_div(a, b):
    return -(-a // b)


def ew_trips(n):
    """trips of the grid-stride loop of an elementwise kernel over n work items: the second starts at 8192 * 256 = 2^21"""
    return ceil_div(n, ew_grid(n) * 256)


def loglik_chunk(inner, nsplit, aligned):
    """the slice of a row one workgroup of the forward sums: a multiple of 4; an odd one sends the kernel down its scalar path"""
    chunk = (ceil_div(inner, nsplit) + 3) // 4 * 4
    return chunk if aligned else chunk | 1


def slice_trips(chunk):
    """p += 1024 on the float4 path (256 lanes x 4), p += 256 on the scalar one"""
    return ceil_div(chunk, 1024 if chunk % 4 == 0 else 256)


def elbo_small_blocks(nl_rows, M, Do, N=0, q=0, nks=0, nkv=0):
    """blocks of 256 threads over the largest small operand PRESENT: Us, the rows' gradients, Um, and the heads (N, q) or the KL values"""
    return ceil_div(max(M * (M + 1) // 2 * Do, nl_rows, M * Do, N * q, nks, nkv), 256)


def iw_small_blocks(M, Do, N):
    """one wavefront per sequence (N 64 lanes) or the packed Us.  The launcher also takes M Do into the maximum; P Do = M (M + 1) / 2 Do
    >= M Do for every M >= 1, so that term can never set the count"""
    assert M * Do <= M * (M + 1) // 2 * Do
    return ceil_div(max(M * (M + 1) // 2 * Do, N * 64), 256)


def cpr(inner):
    """logit blocks per row of k_elbo_iw_bwd<true>"""
    return ceil_div(inner, IW_SPAN)


def iw_group_trips(L, N):
    """groups the busiest of the 16 wavefronts of k_elbo_iw_fwd takes (g += 16)"""
    return ceil_div(L * N, 16)


def iw_lw_trips(K, N):
    """trips of the lw sum of k_elbo_iw_fwd (e += 1024)"""
    return ceil_div(K * N, 1024)


def draws_blocks(N, q):
    return ceil_div(N * q, 256)


def predict_grid(F, n):
    return min(F, min(n, MAX_CUS))


def predict_trips(F, n):
    """frames the busiest workgroup of k_fwd_predict / k_fwd_predict_w takes (f += gridDim.x)"""
    return ceil_div(F, predict_grid(F, n))


def predict_Ns(n, Th):
    """the two smallest N with F = N Th > min(n, 256) workgroups"""
    N = min(n, MAX_CUS) // Th + 1
    return N, N + 1


# ---- the case tables -----------------------------------------------------------------------------------------------------------------------
IW_CASES = [IW(1, 3, 17, 1, 5, 3),                   # L N = 17: one wavefront takes two groups
            IW(3, 3, 11, 3, 5, 3),                   # 33 groups: three trips, l > 0 in later trips, no multiple of 16
            IW(2, 2, 40, 1, 2, 1),                   # 80 groups: every wavefront takes five
            IW(1, 64, 17, 1, 5, 3),                  # K N = 1088: the second trip of the lw sum
            IW(1, 2, 3, 1, 147, 6),                  # 65268 packed entries: the last shape summed in the kernel ...
            IW(1, 2, 3, 1, 148, 6),                  # ... 66156: the first summed in parts
            IW(2, 3, 5, 1, 2, 1),                    # nb_small = 2, set by N 64
            IW(2, 3, 17, 3, 2, 1),                   # nb_small = 5, set by N 64
            IW(2, 3, 3, 1, 30, 3),                   # nb_small = 6, set by P Do
            IW(2, 3, 5, 1, 30, 3),                   # the same at N = 5
            IW(2, 3, 4, 1, 2, 1),                    # nb_small = 1 (the fused cases below run on these three as well)
            IW(1, 1, 65535, 1, 2, 1)]                # the row limit
IW_REFUSED = IW(1, 1, 65536, 1, 2, 1)
# N = 5 makes nb_small >= 2 (320 lanes): nb_small = 1 needs N <= 4, so the pair of inner values runs at N = 4 as well
IWLL_CASES = [IWLL(2, 3, 5, 784, 3, 2, 1), IWLL(2, 3, 5, 4, 1, 2, 1),         # nb_small = 2 (N 64); inner 2352 (cpr 2) and 4
              IWLL(2, 3, 5, 784, 3, 30, 3), IWLL(2, 3, 5, 4, 1, 30, 3),       # nb_small = 6 (P Do)
              IWLL(2, 3, 4, 784, 3, 2, 1), IWLL(2, 3, 4, 4, 1, 2, 1),         # nb_small = 1
              IWLL(1, 1, 65535, 4, 1, 2, 1)]                                  # the row limit
DR_CASES = [DR(3, 43, 6, 'dense'), DR(3, 43, 6, 'half'),                      # 258 lanes: block 1 holds two
            DR(64, 300, 16, 'dense'), DR(64, 300, 16, 'half')]                # 19 blocks, K = 64
LEN_CASES = [LEN(2, 37, 16, 784, 4, ''),             # float4 path, chunk 3136: four trips of p += 1024
             LEN(2, 37, 16, 784, 4, 'a'), LEN(2, 37, 16, 784, 4, 'X'),        # scalar path, chunk 3137: 13 trips of p += 256
             LEN(2, 37, 16, 784, 0, ''),             # the proposed 13 slices of 968: slice boundaries inside frames
             LEN(1, 168, 16, 784, 0, ''),            # n = 2 107 392 > 2^21: the elementwise backward kernels' second trip
             LEN(3, 21845, 2, 4, 0, '')]             # rows = 65535 at inner = 8, one slice
LEN_REFUSED = LEN(4, 16384, 2, 4, 1, '')             # rows = 65536
PK_CASES = [PK(2, 37, 16, 784, 4, ''), PK(2, 37, 16, 784, 4, 'az')]
PKB_CASES = [PKB(4, 208, 16, 784, ''),               # 10 956 images: n / 4 > 2^21 on the V4 path, no multiple of 256
             PKB(2, 104, 16, 784, 'z')]              # 2 740 images: n > 2^21 on the scalar path
GA_CASES = [GA(2, 14000, 16, 6, 12)]
PR_KINDS = ('len', 'll_len', 'w', 'w_len')
PR_TH, PR_TOBS, PR_L, PR_SPLITS = 7, 5, 4, (2, 2)    # Lc = 2 in two launches: done = 0, then done = 2


def predict_cases(n):
    return [PR(kind, N) for N in predict_Ns(n, PR_TH) for kind in PR_KINDS]


def len_counts(N, T):
    """counts spanning 0, 1, T, T + 3 and the quarter points of the row (the slice boundaries at four slices) with values between them"""
    base = [0, 1, T, T + 3] + sorted({k for k in (T // 4, T // 2, 3 * T // 4, 2, 3, 5, 7, T - 1) if 0 < k < T})
    return [base[i % len(base)] for i in range(N)]


def pkb_counts(c):
    """counts of the *_pk backward cases: mostly full sequences (ga_counts), one of them trimmed if need be so that the number of compact
    float4s is no multiple of 256"""
    counts = [min(max(k, 0), c.T) for k in ga_counts(c)]
    while (c.L * sum(counts) * c.frame // 4) % 256 == 0:
        counts[1] -= 1
    return counts


def ga_counts(c):
    """some sequences without a frame, some with one, most of them full or nearly so"""
    base = (0, c.T, c.T, c.T + 3, c.T - 1, c.T, c.T, 1, c.T, c.T, c.T - 2, c.T)
    return [base[i % 12] for i in range(c.N)]


def host_index(counts, T):
    """(c, off, src) as int64 tensors: c = clamp(counts, 0, T), off its exclusive prefix sum (N + 1), src[j] = n T + t"""
    c = torch.as_tensor(counts, dtype=torch.int64).clamp(0, T)
    off = torch.zeros(c.numel() + 1, dtype=torch.int64)
    torch.cumsum(c, 0, out=off[1:])
    seq = torch.repeat_interleave(torch.arange(c.numel()), c)
    return c, off, seq * T + (torch.arange(int(off[-1])) - off[:-1][seq])


def len_ns(c):
    return c.ns or sigmoid_loglik_splits(c.L * c.N, c.T * c.frame)


def loops(c, n=MAX_CUS):
    """the (kernel, loop) pairs case c sends past one trip (or, for a block count, past one block); n: the device's CU count"""
    out = set()
    if isinstance(c, IW):
        if iw_group_trips(c.L, c.N) >= 2:
            out.add(('k_elbo_iw_fwd', 'groups'))
        if iw_lw_trips(c.K, c.N) >= 2:
            out.add(('k_elbo_iw_fwd', 'lw sum'))
        P, nb = c.M * (c.M + 1) // 2 * c.Do, iw_small_blocks(c.M, c.Do, c.N)
        if nb >= 2:
            out.add(('k_elbo_iw_bwd<false>', 'small blocks set by N 64' if c.N * 64 > P else 'small blocks set by P Do'))
    elif isinstance(c, IWLL):
        if iw_small_blocks(c.M, c.Do, c.N) >= 2:
            out.add(('k_elbo_iw_bwd<true>', 'logit blocks behind nb_small > 1'))
        else:
            out.add(('k_elbo_iw_bwd<true>', 'logit blocks behind nb_small = 1'))
        if cpr(c.frame * c.T) >= 2:
            out.add(('k_elbo_iw_bwd<true>', 'cpr > 1'))
        if min(c.L, c.K, c.N) > 1 and c.N & (c.N - 1):
            out.add(('k_elbo_iw_bwd<true>', 'row split with l, k, n > 1'))
    elif isinstance(c, DR):
        if draws_blocks(c.N, c.q) >= 2:
            out.add(('k_reparam_draws_bwd', 'blocks'))
    elif isinstance(c, (LEN, PK)):
        chunk = loglik_chunk(c.T * c.frame, len_ns(c), not c.mis)
        kern = 'k_sigmoid_loglik_fwd<true>' if isinstance(c, LEN) else 'k_sigmoid_loglik_fwd_pk'
        if slice_trips(chunk) >= 2:
            out.add((kern, 'float4 slice' if chunk % 4 == 0 else 'scalar slice'))
        if isinstance(c, LEN) and ew_trips(c.L * c.N * c.T * c.frame) >= 2:
            out.update((k, 'grid-stride') for k in ('k_sigmoid_loglik_bwd<true>', 'k_elbo_loglik_bwd<true> (heads)', 'k_elbo_loglik_bwd<true> (KL values)',
                                                    'k_loglik_rowsum_bwd<true>'))
    elif isinstance(c, PKB):
        n_el = c.L * sum(pkb_counts(c)) * c.frame
        if not c.mis and ew_trips(n_el // 4) >= 2:
            out.add(('k_sigmoid_loglik_bwd_pk<true>', 'grid-stride'))
        if c.mis and ew_trips(n_el) >= 2:
            out.add(('k_sigmoid_loglik_bwd_pk<false>', 'grid-stride'))
    elif isinstance(c, GA):
        P = int(host_index(ga_counts(c), c.T)[1][-1])
        if ew_trips(c.L * P * c.q) >= 2:
            out.add(('k_gather_frames_fwd', 'grid-stride'))
        if ew_trips(c.L * c.N * c.T * c.ld) >= 2:
            out.add(('k_gather_frames_bwd', 'grid-stride'))
    elif isinstance(c, PR):
        if predict_trips(c.N * PR_TH, n) >= 2:
            out.add(({'len': 'k_fwd_predict<false, true>', 'll_len': 'k_fwd_predict<true, true>'}.get(c.kind, 'k_fwd_predict_w'), 'frames'))
    return out


def expected(c):
    """{step: tag} of the calls the case's launches make"""
    if isinstance(c, IW):
        return dict(fwd='elbo_iw_fwd' + (' (Us in parts)' if us_in_parts(c.M, c.Do) else ''), bwd='elbo_iw_bwd')
    if isinstance(c, IWLL):
        return dict(sll='sigmoid_loglik_fwd', bwd='elbo_iw_bwd', sll_bwd='sigmoid_loglik_bwd', ll='elbo_iw_loglik_bwd')
    if isinstance(c, DR):
        return dict(bwd='reparam_draws_bwd')
    if isinstance(c, LEN):
        return {k: v + '_len' for k, v in LEN_TAGS.items()}
    if isinstance(c, PK):
        return dict(fwd='sigmoid_loglik_fwd_pk', bwd='sigmoid_loglik_bwd_pk')
    if isinstance(c, PKB):
        return dict(bwd='sigmoid_loglik_bwd_pk')
    if isinstance(c, GA):
        return dict(fwd='gather_frames_fwd', bwd='gather_frames_bwd')
    return dict(run={'len': 'dec10_predict_len', 'll_len': 'dec10_predict_ll_len', 'w': 'dec10_predict_w', 'w_len': 'dec10_predict_len_w'}[c.kind])


LEN_TAGS = dict(fwd='sigmoid_loglik_fwd', bwd='sigmoid_loglik_bwd', ll='elbo_loglik_bwd', kl='elbo_loglik_bwd_kl', rs='loglik_rowsum',
                rsb='loglik_rowsum_bwd')
REQUIRED_TAGS = ('elbo_iw_fwd', 'elbo_iw_fwd (Us in parts)', 'elbo_iw_bwd', 'elbo_iw_loglik_bwd', 'reparam_draws_bwd', 'sigmoid_loglik_fwd_len',
                 'sigmoid_loglik_bwd_len', 'elbo_loglik_bwd_len', 'elbo_loglik_bwd_kl_len', 'loglik_rowsum_len', 'loglik_rowsum_bwd_len',
                 'sigmoid_loglik_fwd_pk', 'sigmoid_loglik_bwd_pk', 'gather_frames_fwd', 'gather_frames_bwd', 'dec10_predict_len',
                 'dec10_predict_ll_len', 'dec10_predict_w', 'dec10_predict_len_w')
REQUIRED_LOOPS = (('k_elbo_iw_fwd', 'groups'), ('k_elbo_iw_fwd', 'lw sum'), ('k_elbo_iw_bwd<false>', 'small blocks set by N 64'),
                  ('k_elbo_iw_bwd<false>', 'small blocks set by P Do'), ('k_elbo_iw_bwd<true>', 'logit blocks behind nb_small > 1'),
                  ('k_elbo_iw_bwd<true>', 'logit blocks behind nb_small = 1'), ('k_elbo_iw_bwd<true>', 'cpr > 1'),
                  ('k_elbo_iw_bwd<true>', 'row split with l, k, n > 1'), ('k_reparam_draws_bwd', 'blocks'),
                  ('k_sigmoid_loglik_fwd<true>', 'float4 slice'), ('k_sigmoid_loglik_fwd<true>', 'scalar slice'),
                  ('k_sigmoid_loglik_fwd_pk', 'float4 slice'), ('k_sigmoid_loglik_fwd_pk', 'scalar slice'),
                  ('k_sigmoid_loglik_bwd<true>', 'grid-stride'), ('k_elbo_loglik_bwd<true> (heads)', 'grid-stride'),
                  ('k_elbo_loglik_bwd<true> (KL values)', 'grid-stride'), ('k_loglik_rowsum_bwd<true>', 'grid-stride'),
                  ('k_sigmoid_loglik_bwd_pk<true>', 'grid-stride'), ('k_sigmoid_loglik_bwd_pk<false>', 'grid-stride'),
                  ('k_gather_frames_fwd', 'grid-stride'), ('k_gather_frames_bwd', 'grid-stride'), ('k_fwd_predict<false, true>', 'frames'),
                  ('k_fwd_predict<true, true>', 'frames'), ('k_fwd_predict_w', 'frames'))


def all_cases(n=MAX_CUS):
    return IW_CASES + IWLL_CASES + DR_CASES + LEN_CASES + PK_CASES + PKB_CASES + GA_CASES + predict_cases(n)


def _f(v):
    return ctypes.c_float(v)


def _twice(once):
    """once() -> (outputs on the CPU, tags, problems); run TWICE: the first run's outputs, with what differs in the second among the problems"""
    (out, tags, problems), (out2, tags2, problems2) = once(), once()
    differs = ['the second run differs in %s' % k for k in out if torch.is_tensor(out[k]) and not torch.equal(R._bits(out[k]), R._bits(out2[k]))]
    return out, tags, problems + problems2 + differs + ([] if tags == tags2 else ['the second run took %s' % tags2])


def _err(got, ref, scale=None):
    s = float(ref.abs().max()) if scale is None else float(scale)
    return float((got.double().reshape(-1) - ref.double().reshape(-1)).abs().max()) / max(s, 1e-300)


def judge(results, what):
    """results: [(case, {output: (error, fp32 distance)})] -> every figure printed, then error <= 4 x the grid's floor (test_gpu_iw_loss._judge)"""
    names = list(results[0][1])
    floor = {k: max(r[k][1] for _, r in results) for k in names}
    worst = {k: max(r[k][0] for _, r in results) for k in names}
    print('%s, %d cases: %s' % (what, len(results), {k: 'worst %.2e floor %.2e ratio %.2f' % (worst[k], floor[k], worst[k] / floor[k] if floor[k] else 0.0)
                                                     for k in names}))
    for c, r in results:
        print('  %s: %s' % (case_id(c), {k: '%.2e / %.2e' % v for k, v in r.items()}))
    bad = [(case_id(c), k, r[k][0], floor[k]) for c, r in results for k in names if not r[k][0] <= 4 * floor[k]]
    assert not bad, bad[:8]
    return {k: (worst[k], floor[k]) for k in names}


# ---- 1. the importance-weighted stage ------------------------------------------------------------------------------------------------------
def _us(M, Do, g):
    Us = 0.01 * torch.randn(Do, M * (M + 1) // 2, generator=g)
    Us[:, W.diag_index(M)] = 0.5 + torch.rand(Do, M, generator=g)
    return Us


@functools.lru_cache(maxsize=4)
def iw_inputs(c):
    """the inputs of test_gpu_iw_loss.py: a of magnitude 2e3 with a spread of 3 nats over the draws, as real rows have"""
    g = R._gen('late iw', *c)
    ll = -2000.0 + 3.0 * torch.randn(c.L, c.K, c.N, generator=g)
    lpart = ll.reshape(-1, 1).float().contiguous()
    if c.ns > 1:
        lpart = (ll.reshape(-1, 1) / c.ns + 0.5 * torch.randn(c.L * c.K * c.N, c.ns, generator=g)).float().contiguous()
    return dict(lpart=lpart, lw=-3.0 + 2.0 * torch.randn(c.K, c.N, generator=g), Um=torch.randn(c.M, c.Do, generator=g), Us=_us(c.M, c.Do, g))


OUT_NAMES = ('loss', 'iw_nll', 'kl_mc', 'kl_u', 'ess')


def iw_refs(c, d):
    """iw_ref on the same fp32 inputs in fp64 and fp32 -> {dtype: (out, grow, glw, dUm, dUs)}, the scales of out (test_gpu_iw_loss._stage_refs)"""
    refs = {dt: W.objective_grads(*(d[k].to(dt) for k in ('lpart', 'lw', 'Um', 'Us')), c.L, c.K, c.N, c.M, NOBS, SEEDS) for dt in (F64, F32)}
    a = W.rows_of(d['lpart'].double(), c.L, c.K, c.N) + d['lw'].double()[None]
    s_iw = float(a.abs().max(1).values.mean())
    ku_abs = float(W.svgp_kl_abs(d['Um'].double(), d['Us'].double(), c.M))
    return refs, [s_iw * NOBS + ku_abs, s_iw, float(d['lw'].double().abs().mean()), ku_abs, float(c.K)]


def iw_errors(got, refs, scales):
    """{output: (error of `got`, fp32 distance)} against fp64; got None: the fp32 distances alone (the host suite)"""
    r64, r32 = refs[F64], refs[F32]
    g = (lambda k, i: r32[0][i]) if got is None else (lambda k, i: got['out'][i])
    e = {n: (_err(g(n, i), r64[0][i], scales[i]), _err(r32[0][i], r64[0][i], scales[i])) for i, n in enumerate(OUT_NAMES)}
    for i, n in enumerate(('grow', 'glw', 'dUm', 'dUs'), 1):
        e[n] = (_err(r32[i] if got is None else got[n], r64[i]), _err(r32[i], r64[i]))
    return e


def _scalars(bf, values):
    return [None if v is None else bf.new('g%d' % i, 1, torch.tensor([v])) for i, v in enumerate(values)]


def _once_iw(c, d):
    rows, P = c.L * c.K * c.N, c.M * (c.M + 1) // 2
    bf, tags = R.Bufs(), {}
    lp, lw = bf.new('lpart', rows * c.ns, d['lpart']), bf.new('lw', c.K * c.N, d['lw'])
    Um, Us = bf.new('Um', c.M * c.Do, d['Um']), bf.new('Us', c.Do * P, d['Us'])
    out = bf.new('out', 5 + R.ELBO_PARTS, output=False)          # 5 results; the 256 floats behind them are scratch
    grow, glw, dUm, dUs = bf.new('grow', rows), bf.new('glw', c.K * c.N), bf.new('dUm', c.M * c.Do), bf.new('dUs', c.Do * P)
    gs = _scalars(bf, SEEDS)
    R._call(tags, 'fwd', 'gpode_elbo_iw_fwd', lp, rows, c.ns, lw, c.L, c.K, c.N, c.M, c.Do, Um, Us, _f(NOBS), out)
    R._call(tags, 'bwd', 'gpode_elbo_iw_bwd', *gs, lp, rows, c.ns, lw, c.L, c.K, c.N, c.M, c.Do, Um, Us, _f(NOBS), grow, glw, dUm, dUs)
    problems = bf.problems()
    if bool(torch.isnan(out[:5]).any()):
        problems.append('out: a NaN of the fill is left')
    tail = torch.isnan(out[5:])
    if bool(tail.any()) if us_in_parts(c.M, c.Do) else not bool(tail.all()):
        problems.append('out: the scratch tail is %s' % ('not fully written' if us_in_parts(c.M, c.Do) else 'written without need'))
    return dict(out=out[:5].cpu(), grow=grow.cpu(), glw=glw.cpu().view(c.K, c.N), dUm=dUm.cpu().view(c.M, c.Do), dUs=dUs.cpu().view(c.Do, P)), tags, problems


def run_iw(c):
    """-> ({output: (error, fp32 distance)}, tags, problems)"""
    d = iw_inputs(c)
    dd = {k: v.cuda() for k, v in d.items()}
    got, tags, problems = _twice(lambda: _once_iw(c, dd))
    refs, scales = iw_refs(c, d)
    return iw_errors(got, refs, scales), tags, problems


def iw_refusal(c):
    """the three entry points at rows = 65536: every one refuses, nothing is written"""
    rows, P, inner = c.L * c.K * c.N, c.M * (c.M + 1) // 2, 4
    bf = R.Bufs()
    z = lambda name, n: bf.new(name, n, torch.zeros(n))
    lp, lw, Um, Us = z('lpart', rows), z('lw', c.K * c.N), z('Um', c.M * c.Do), bf.new('Us', c.Do * P, torch.ones(c.Do * P))
    X, zz = z('X', c.N * inner), bf.new('z', rows * inner, torch.full((rows * inner,), 0.5))
    out, grow, glw, dUm, dUs, ga = (bf.new(k, n) for k, n in (('out', 5 + R.ELBO_PARTS), ('grow', rows), ('glw', c.K * c.N), ('dUm', c.M * c.Do),
                                                             ('dUs', c.Do * P), ('ga', rows * inner)))
    gs, said = [None] * 5, []
    head = (lp, rows, c.ns, lw, c.L, c.K, c.N, c.M, c.Do, Um, Us, _f(NOBS))
    for name, args in (('gpode_elbo_iw_fwd', head + (out,)), ('gpode_elbo_iw_bwd', tuple(gs) + head + (grow, glw, dUm, dUs)),
                       ('gpode_elbo_iw_bwd_ll', tuple(gs) + head + (grow, glw, dUm, dUs, X, zz, ga, rows * inner, c.N * inner))):
        try:
            R._call({}, 'x', name, *args)
            said.append('%s ran' % name)
        except R.Refused as e:
            if name not in str(e) or 'rows <= 65535' not in str(e):
                said.append(str(e))
    return said, bf.untouched(), [p for p in bf.problems() if 'guard' in p]


def _once_iwll(c, d, X_h, a_h):
    rows, inner, P = c.L * c.K * c.N, c.T * c.frame, c.M * (c.M + 1) // 2
    ns, nX = sigmoid_loglik_splits(rows, inner), X_h.numel()
    bf, tags = R.Bufs(), {}
    X, a = bf.new('X', nX, X_h), bf.new('a', rows * inner, a_h)
    z, part = bf.new('z', rows * inner), bf.new('part', rows * ns)
    lw, Um, Us = bf.new('lw', c.K * c.N, d['lw']), bf.new('Um', c.M * c.Do, d['Um']), bf.new('Us', c.Do * P, d['Us'])
    gs = _scalars(bf, SEEDS)
    R._call(tags, 'sll', 'gpode_sigmoid_loglik_fwd', X, a, z, part, rows, inner, nX, ns)
    o = {}
    for tag in ('pair', 'fused'):
        o.update({tag + '_' + k: bf.new(tag + k, n) for k, n in (('grow', rows), ('glw', c.K * c.N), ('dUm', c.M * c.Do), ('dUs', c.Do * P),
                                                                 ('ga', rows * inner))})
    p = lambda k: o['pair_' + k]
    f = lambda k: o['fused_' + k]
    head = (part, rows, ns, lw, c.L, c.K, c.N, c.M, c.Do, Um, Us, _f(NOBS))
    R._call(tags, 'bwd', 'gpode_elbo_iw_bwd', *gs, *head, p('grow'), p('glw'), p('dUm'), p('dUs'))
    R._call(tags, 'sll_bwd', 'gpode_sigmoid_loglik_bwd', X, z, p('grow'), p('ga'), rows, inner, nX)
    R._call(tags, 'll', 'gpode_elbo_iw_bwd_ll', *gs, *head, f('grow'), f('glw'), f('dUm'), f('dUs'), X, z, f('ga'), rows * inner, nX)
    return {k: v.cpu() for k, v in o.items()}, tags, bf.problems()


def run_iwll(c):
    """-> (outputs of the pair and of the fused launch, tags, problems incl. every output of the fused launch that differs from the pair's)"""
    g = R._gen('late iw fused', *c)
    X_h, a_h = R._x_form((c.N, c.T, c.frame), 'norm', g), R._logits((c.L * c.K * c.N, c.T * c.frame), g)
    d = {k: v.cuda() for k, v in iw_inputs(IW(c.L, c.K, c.N, 1, c.M, c.Do)).items()}
    out, tags, problems = _twice(lambda: _once_iwll(c, d, X_h.cuda(), a_h.cuda()))
    for k in ('grow', 'glw', 'dUm', 'dUs', 'ga'):
        if not torch.equal(R._bits(out['pair_' + k]), R._bits(out['fused_' + k])):
            problems.append('%s of gpode_elbo_iw_bwd_ll differs from gpode_elbo_iw_bwd + gpode_sigmoid_loglik_bwd' % k)
    if not float(out['pair_ga'].abs().max()) > 0:
        problems.append('ga is zero')
    return out, tags, problems


# ---- 2. the adjoint of the draws -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def dr_inputs(c):
    g = R._gen('late draws', *c)
    Wd = c.q if c.layout == 'dense' else 2 * c.q
    return dict(h=torch.cat((torch.randn(c.N, c.q, generator=g), 0.7 * torch.randn(c.N, c.q, generator=g) - 1), 1),
                eps=torch.randn(c.K, c.N, c.q, generator=g), gfull=torch.randn(c.K, c.N, Wd, generator=g), glw=torch.randn(c.K, c.N, generator=g))


def dr_refs(c, d):
    col = d['gfull'].shape[-1] - c.q
    return {dt: W.draws_grads(*(t.to(dt) for t in (d['h'][:, :c.q], d['h'][:, c.q:], d['eps'], d['gfull'][..., col:], d['glw']))) for dt in (F64, F32)}


def _once_dr(c, d):
    bf, tags = R.Bufs(), {}
    q, Wd = c.q, d['gfull'].shape[-1]
    col = Wd - q
    hd, ed = bf.new('h', d['h'].numel(), d['h']), bf.new('eps', d['eps'].numel(), d['eps'])
    gzd, glwd = bf.new('gz', d['gfull'].numel(), d['gfull']), bf.new('glw', d['glw'].numel(), d['glw'])
    gh = bf.new('gh', c.N * 2 * q)
    R._call(tags, 'bwd', 'gpode_reparam_draws_bwd', gzd[col:], Wd, glwd, hd, hd[q:], 2 * q, ed, gh, gh[q:], 2 * q, c.K, c.N, q)
    return dict(gh=gh.cpu().view(c.N, 2 * q)), tags, bf.problems()


def run_dr(c):
    d = dr_inputs(c)
    dd = {k: v.cuda() for k, v in d.items()}
    got, tags, problems = _twice(lambda: _once_dr(c, dd))
    refs = dr_refs(c, d)
    return {name: (_err(got['gh'][:, i * c.q:(i + 1) * c.q], refs[F64][i]), _err(refs[F32][i], refs[F64][i]))
            for i, name in enumerate(('gmu', 'glogvar'))}, tags, problems


# ---- 3. the ragged *_len loss kernels (the layout of test_gpu_ragged_loss.py) ----------------------------------------------------------------
LM, LDO, LQ, LNKS = 7, 3, 6, 2
LEN_GA = ('ga_bwd', 'ga_ll', 'ga_kl')
LEN_OTHERS = ('glrow_ll', 'ghs', 'dUm_ll', 'dUs_ll', 'glrow_kl', 'gkls', 'dUm_kl', 'dUs_kl')


def len_lengths(c, lname):
    return [c.T] * c.N if lname == 'full' else len_counts(c.N, c.T)


def len_observed(c, lname):
    """(rows, inner) bool: the element is observed"""
    obs = torch.arange(c.T)[None, :] < torch.tensor(len_lengths(c, lname))[:, None]
    return obs[None, :, :, None].expand(c.L, c.N, c.T, c.frame).reshape(c.L * c.N, c.T * c.frame)


@functools.lru_cache(maxsize=2)
def len_inputs(L, N, T, frame):
    g = R._gen('late len', L, N, T, frame)
    return dict(X=R._x_form((N, T, frame), 'norm', g), a=R._logits((L, N, T, frame), g), grow=torch.randn(L * N, generator=g),
                hs=torch.cat((torch.randn(N, LQ, generator=g), torch.randn(N, LQ, generator=g) * 0.7 - 1.0), 1),
                Um=0.5 * torch.randn(LM, LDO, generator=g), Us=R.us_packed(LM, LDO, 'tril', 1.0, g))


def _garbage(t, kind):
    if kind == 'nan':
        return torch.full_like(t, float('nan'))
    s = torch.ones(t.numel()).reshape(t.shape)
    s.view(-1)[1::2] = -1.0
    return s * float('inf')


def _once_len(c, lname, kind):
    """every entry of the loss stage once: the twins (lname None) or the _len forms -> (outputs on the CPU, tags, problems)"""
    rows, inner, nX = c.L * c.N, c.T * c.frame, c.N * c.T * c.frame
    n = rows * inner
    d = len_inputs(c.L, c.N, c.T, c.frame)
    X, a = d['X'], d['a']
    sfx, extra = '', ()
    if lname is not None:
        if kind != 'clean':
            obs = len_observed(c, lname)[:c.N].view(c.N, c.T, c.frame)[:, :, 0]
            X, a = X.clone(), a.clone()
            X[~obs] = _garbage(X[~obs], kind)
            a[:, ~obs] = _garbage(a[:, ~obs], kind)
        sfx, extra = '_len', (torch.tensor(len_lengths(c, lname), dtype=torch.int32, device='cuda'), c.T, c.frame)
    bf, tags, out = R.Bufs(), {}, {}
    sh = lambda ch: 1 if ch in c.mis else 0
    Xd, ad = bf.new('X', nX, X, shift=sh('X')), bf.new('a', n, a, shift=sh('a'))
    z = bf.new('z', n, shift=sh('z'))
    ns = len_ns(c)
    part = bf.new('part', rows * ns)
    R._call(tags, 'fwd', 'gpode_sigmoid_loglik_fwd' + sfx, Xd, ad, z, part, rows, inner, nX, ns, *extra)
    grow = bf.new('grow', rows, d['grow'])
    ga = bf.new('ga_bwd', n, shift=sh('z'))
    R._call(tags, 'bwd', 'gpode_sigmoid_loglik_bwd' + sfx, Xd, z, grow, ga, rows, inner, nX, *extra)
    out.update(z=z, part=part.view(rows, ns), ga_bwd=ga)
    P = LM * (LM + 1) // 2
    Um, Us, hs = bf.new('Um', LM * LDO, d['Um']), bf.new('Us', LDO * P, d['Us']), bf.new('hs', c.N * 2 * LQ, d['hs'])
    gs = [bf.new('g%d' % i, 1, torch.tensor([v])) for i, v in enumerate(R.SEED_VALUES)]
    o = {k: bf.new(k, m) for k, m in (('glrow_ll', rows), ('ghs', c.N * 2 * LQ), ('dUm_ll', LM * LDO), ('dUs_ll', LDO * P), ('ga_ll', n),
                                      ('glrow_kl', rows), ('gkls', LNKS), ('dUm_kl', LM * LDO), ('dUs_kl', LDO * P), ('ga_kl', n))}
    R._call(tags, 'll', 'gpode_elbo_all_bwd_ll' + sfx, *gs, rows, hs, None, c.N, LQ, LM, LDO, Um, Us, _f(NOBS), o['glrow_ll'], o['ghs'], None,
            o['dUm_ll'], o['dUs_ll'], Xd, z, o['ga_ll'], n, nX, *extra)
    R._call(tags, 'kl', 'gpode_elbo_all_bwd_ll_kl' + sfx, *gs, rows, c.N, LM, LDO, Um, Us, _f(NOBS), o['glrow_kl'], o['gkls'], LNKS, None, 0,
            o['dUm_kl'], o['dUs_kl'], Xd, z, o['ga_kl'], n, nX, *extra)
    out.update(o)
    rs, gz = bf.new('rs', rows), bf.new('gz', n)
    R._call(tags, 'rs', 'gpode_loglik_rowsum_fwd' + sfx, Xd, z, rs, rows, inner, nX, *extra)
    R._call(tags, 'rsb', 'gpode_loglik_rowsum_bwd' + sfx, Xd, z, grow, gz, rows, inner, nX, *extra)
    out.update(rs=rs, gz=gz)
    problems = bf.problems()
    if kind != 'clean':                               # NaN logits give NaN z on padded elements, as the twin would: not a fill left over
        problems = [p for p in problems if not p.startswith('z:')]
    return {k: v.cpu() for k, v in out.items()}, tags, problems


def run_len(c, lname=None, kind='clean'):
    return _twice(lambda: _once_len(c, lname, kind))


def len_row_errors(c, lname, got):
    """(error of the fused row sums, of the separate row sums, the rows without a frame) against the fp64 sum of the observed terms"""
    d = len_inputs(c.L, c.N, c.T, c.frame)
    rows = c.L * c.N
    obs = len_observed(c, lname)
    Xr = d['X'].double().reshape(1, -1).repeat(c.L, 1).reshape(rows, -1)
    t = R.bernoulli_terms(Xr, torch.sigmoid(d['a'].double()).reshape(rows, -1))
    short = obs.sum(1) <= R.SLL_SHORT                 # rows of up to 8 observed terms: the fp64 terms of the returned z (sll_short_rows)
    if bool(short.any()):
        t = torch.where(short[:, None], R.bernoulli_terms(Xr, got['z'].double().reshape(rows, -1)), t)
    t = torch.where(obs, t, torch.zeros((), dtype=F64))
    ref, scale = t.sum(1), t.abs().sum(1).clamp_min(1e-300)
    empty = obs.sum(1) == 0
    e = lambda v: float(((v.double() - ref).abs() / scale)[~empty].max())
    return e(got['part'].double().sum(1)), e(got['rs']), empty


def len_refusal(c):
    """rows = 65536: gpode_sigmoid_loglik_fwd_len refuses with nothing written"""
    rows, inner, nX = c.L * c.N, c.T * c.frame, c.N * c.T * c.frame
    bf = R.Bufs()
    X, a = bf.new('X', nX, torch.zeros(nX)), bf.new('a', rows * inner, torch.zeros(rows * inner))
    z, part = bf.new('z', rows * inner), bf.new('part', rows)
    n_obs = torch.full((c.N,), c.T, dtype=torch.int32, device='cuda')
    try:
        R._call({}, 'x', 'gpode_sigmoid_loglik_fwd_len', X, a, z, part, rows, inner, nX, 1, n_obs, c.T, c.frame)
        said = 'ran'
    except R.Refused as e:
        said = str(e)
    return said, bf.untouched(), [p for p in bf.problems() if 'guard' in p]


# ---- 4. the compact route ----------------------------------------------------------------------------------------------------------------------
def _index_dev(counts, T):
    c, off, src = host_index(counts, T)
    return c, off, src, off.to(torch.int32).cuda(), src.to(torch.int32).cuda()


def _once_pk(c, counts, nan_padding):
    """the _pk forward and backward on the compact form of len_inputs -> (outputs on the CPU, tags, problems)"""
    d = len_inputs(c.L, c.N, c.T, c.frame)
    cl, off, src, off_d, src_d = _index_dev(counts, c.T)
    P, rows = int(off[-1]), c.L * c.N
    X = d['X']
    if nan_padding:
        X = X.clone()
        X[torch.arange(c.T)[None, :] >= cl[:, None]] = float('nan')
    a_c = d['a'].reshape(c.L, c.N * c.T, c.frame)[:, src].reshape(c.L * P, c.frame)
    sh = lambda ch: 1 if ch in c.mis else 0
    bf, tags = R.Bufs(), {}
    Xd, ad = bf.new('X', X.numel(), X), bf.new('a', a_c.numel(), a_c, shift=sh('a'))
    z, ga = bf.new('z', a_c.numel(), shift=sh('z')), bf.new('ga', a_c.numel(), shift=sh('z'))
    part, grow = bf.new('part', rows * c.ns), bf.new('grow', rows, d['grow'])
    R._call(tags, 'fwd', 'gpode_sigmoid_loglik_fwd_pk', Xd, ad, z, part, rows, off_d, c.T, c.frame, X.numel(), c.ns)
    R._call(tags, 'bwd', 'gpode_sigmoid_loglik_bwd_pk', Xd, z, grow, ga, rows, src_d, P, c.T, c.frame, X.numel())
    return dict(z=z.cpu(), part=part.cpu().view(rows, c.ns), ga=ga.cpu()), tags, bf.problems()


def run_pk(c, lname, nan_padding=False):
    return _twice(lambda: _once_pk(c, len_lengths(c, lname), nan_padding))


def pk_twin(c):
    """gpode_sigmoid_loglik_fwd / _bwd on the padded logits with the same misalignment and split count"""
    d = len_inputs(c.L, c.N, c.T, c.frame)
    rows, inner, nX = c.L * c.N, c.T * c.frame, c.N * c.T * c.frame
    sh = lambda ch: 1 if ch in c.mis else 0
    bf, tags = R.Bufs(), {}
    Xd, ad = bf.new('X', nX, d['X']), bf.new('a', rows * inner, d['a'], shift=sh('a'))
    z, ga = bf.new('z', rows * inner, shift=sh('z')), bf.new('ga', rows * inner, shift=sh('z'))
    part, grow = bf.new('part', rows * c.ns), bf.new('grow', rows, d['grow'])
    R._call(tags, 'fwd', 'gpode_sigmoid_loglik_fwd', Xd, ad, z, part, rows, inner, nX, c.ns)
    R._call(tags, 'bwd', 'gpode_sigmoid_loglik_bwd', Xd, z, grow, ga, rows, inner, nX)
    return dict(z=z.cpu(), part=part.cpu().view(rows, c.ns), ga=ga.cpu()), tags, bf.problems()


def pk_reference(c, counts, z32=None):
    """fp64: x a - softplus(a) summed over each row's observed frames, sum |terms|, sigmoid(a), and ga = grow (x - z) -- written from the
    fp32 z where the kernel takes z as an INPUT (z32 given: grow (x / z - (1 - x) / (1 - z)) z (1 - z))"""
    d = len_inputs(c.L, c.N, c.T, c.frame)
    cl, off, src = host_index(counts, c.T)
    P = int(off[-1])
    x = d['X'].double().view(c.N * c.T, c.frame)[src][None]                               # (1, P, frame)
    seq = torch.div(src, c.T, rounding_mode='floor')
    g = d['grow'].double().view(c.L, c.N)[:, seq][:, :, None]                             # (L, P, 1)
    if z32 is not None:
        z = z32.double().view(c.L, P, c.frame)
        return dict(ga=g * (x / z - (1 - x) / (1 - z)) * z * (1 - z))
    a = d['a'].double().reshape(c.L, c.N * c.T, c.frame)[:, src]
    terms = x * a - Fn.softplus(a)
    zero = torch.zeros(c.L, c.N, dtype=F64)
    return dict(rowsum=zero.index_add(1, seq, terms.sum(-1)), scale=zero.index_add(1, seq, terms.abs().sum(-1)), z=torch.sigmoid(a),
                ga=g * (x - torch.sigmoid(a)))


@functools.lru_cache(maxsize=1)
def pkb_inputs(c):
    g = R._gen('late pkb', *c)
    a = R._logits((c.L, c.N, c.T, c.frame), g)
    return dict(X=R._x_form((c.N, c.T, c.frame), 'norm', g), z=torch.sigmoid(a), grow=torch.randn(c.L * c.N, generator=g))


def _once_pkb(c, counts, twin):
    """gpode_sigmoid_loglik_bwd_pk on the compact z of pkb_inputs (twin: gpode_sigmoid_loglik_bwd on the padded z)"""
    d = pkb_inputs(c)
    cl, off, src, off_d, src_d = _index_dev(counts, c.T)
    P, rows, nX = int(off[-1]), c.L * c.N, c.N * c.T * c.frame
    sh = 1 if c.mis else 0
    bf, tags = R.Bufs(), {}
    Xd, grow = bf.new('X', nX, d['X']), bf.new('grow', rows, d['grow'])
    if twin:
        n = rows * c.T * c.frame
        zd, ga = bf.new('z', n, d['z'], shift=sh), bf.new('ga', n, shift=sh)
        R._call(tags, 'bwd', 'gpode_sigmoid_loglik_bwd', Xd, zd, grow, ga, rows, c.T * c.frame, nX)
    else:
        z_c = d['z'].reshape(c.L, c.N * c.T, c.frame)[:, src]
        zd, ga = bf.new('z', z_c.numel(), z_c, shift=sh), bf.new('ga', z_c.numel(), shift=sh)
        R._call(tags, 'bwd', 'gpode_sigmoid_loglik_bwd_pk', Xd, zd, grow, ga, rows, src_d, P, c.T, c.frame, nX)
    return dict(ga=ga.cpu()), tags, bf.problems()


def pkb_reference(c, counts, dt=F64):
    d = pkb_inputs(c)
    cl, off, src = host_index(counts, c.T)
    x = d['X'].to(dt).view(c.N * c.T, c.frame)[src][None]
    z = d['z'].reshape(c.L, c.N * c.T, c.frame)[:, src].to(dt)
    g = d['grow'].to(dt).view(c.L, c.N)[:, torch.div(src, c.T, rounding_mode='floor')][:, :, None]
    return g * (x / z - (1 - x) / (1 - z)) * z * (1 - z)


@functools.lru_cache(maxsize=1)
def ga_inputs(c):
    g = R._gen('late gather', *c)
    P = int(host_index(ga_counts(c), c.T)[1][-1])
    return dict(zt=torch.randn(c.L, c.N, c.T, c.ld, generator=g), gout=torch.randn(c.L * P, c.q, generator=g))


def ga_reference(c):
    """exact: out = the first q columns of the observed rows, ordered (l, n, t); gzt = gout on them and 0 everywhere else"""
    d = ga_inputs(c)
    cl, off, src = host_index(ga_counts(c), c.T)
    P = int(off[-1])
    out = d['zt'].view(c.L, c.N * c.T, c.ld)[:, src, :c.q].reshape(c.L * P, c.q)
    gzt = torch.zeros(c.L, c.N * c.T, c.ld)
    gzt[:, src, :c.q] = d['gout'].view(c.L, P, c.q)
    return out, gzt.view(c.L, c.N, c.T, c.ld)


def _once_ga(c, d):
    cl, off, src, off_d, src_d = _index_dev(ga_counts(c), c.T)
    P = int(off[-1])
    bf, tags = R.Bufs(), {}
    zt, gout = bf.new('zt', d['zt'].numel(), d['zt']), bf.new('gout', d['gout'].numel(), d['gout'])
    out, gzt = bf.new('out', c.L * P * c.q), bf.new('gzt', c.L * c.N * c.T * c.ld)
    R._call(tags, 'fwd', 'gpode_gather_frames_fwd', zt, c.ld, c.q, src_d, c.L, c.N, c.T, P, out)
    R._call(tags, 'bwd', 'gpode_gather_frames_bwd', gout, c.ld, c.q, src_d, off_d, c.L, c.N, c.T, P, gzt)
    return dict(out=out.cpu().view(c.L * P, c.q), gzt=gzt.cpu().view(c.L, c.N, c.T, c.ld)), tags, bf.problems()


def run_ga(c):
    d = {k: v.cuda() for k, v in ga_inputs(c).items()}
    return _twice(lambda: _once_ga(c, d))


# ---- 5. the predict epilogue -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def predict_inputs(Nmax):
    """cond_ref.inputs() at Nmax sequences of Th = 7 frames of which T_obs = 5 have a target, 4 draws; a case of N <= Nmax sequences takes
    the leading N"""
    g = R._gen('late predict', Nmax)
    c = 1.5 * torch.randn(PR_L, Nmax, PR_TH, 16, 28, 28, generator=g)
    table = torch.stack([0.3 * torch.randn(16, generator=g), 0.5 + torch.rand(16, generator=g), 0.5 + torch.rand(16, generator=g),
                         0.3 * torch.randn(16, generator=g)], dim=1).contiguous()          # mean, invstd, gamma, beta
    return dict(c=c, table=table, w=0.15 * torch.randn(16, 1, 5, 5, generator=g), b=0.1 * torch.randn(1, generator=g),
                X=torch.rand(Nmax, PR_TOBS, 1, 28, 28, generator=g), logw=1.2 * torch.randn(PR_L, Nmax, generator=g))


def predict_n_obs(N):
    """0 ... Th, every value; the last sequence, whose frames a workgroup takes in a later round, has Th -- so a count read for the wrong
    sequence there changes which frames have a target"""
    return [(PR_TH - (N - 1 - i)) % (PR_TH + 1) for i in range(N)]


def predict_has(N, n_obs):
    """(N, Th) bool: the frame has a target"""
    t = torch.arange(PR_TH)[None, :]
    has = (t < PR_TOBS).expand(N, PR_TH)
    return has if n_obs is None else has & (t < torch.as_tensor(n_obs)[:, None])


@functools.lru_cache(maxsize=2)
def predict_images(Nmax, dtype):
    """logits and sigmoid of decnn.10(relu(bn(c))) of every (draw, frame): (L, Nmax, Th, 784) in ``dtype`` (cond_ref.images)"""
    i = predict_inputs(Nmax)
    t = i['table'].to(dtype)
    v = lambda k: t[:, k].view(1, 16, 1, 1)
    h = torch.relu((i['c'].to(dtype).view(-1, 16, 28, 28) - v(0)) * v(1) * v(2) + v(3))
    a = Fn.conv_transpose2d(h, i['w'].to(dtype), i['b'].to(dtype), padding=2).view(PR_L, Nmax, PR_TH, 784)
    return a, torch.sigmoid(a)


def predict_reference(Nmax, N, dtype, n_obs=None, logw=None):
    """logw None: mean and M2 of the images over the draws, {mean, M2} of the squared error per frame and the log-likelihood of every
    (draw, frame) image (test_gpu_eval.stats64, test_eval_loglik_host.loglik64_from_logits); logw (L, N): the self-normalised weighted
    moments of cond_ref.reference.  Frames without a target hold 0."""
    a, z = (t[:, :N] for t in predict_images(Nmax, dtype))
    X = predict_inputs(Nmax)['X'][:N].to(dtype).view(N, PR_TOBS, 784)
    has = predict_has(N, n_obs)
    zero = torch.zeros((), dtype=dtype)
    pad = lambda v: torch.cat((v, torch.zeros(v.shape[:-1] + (PR_TH - PR_TOBS,), dtype=dtype)), -1)
    e = (z[:, :, :PR_TOBS] - X[None]) ** 2                                           # (L, N, T_obs, 784)
    if logw is None:
        mean = z.mean(0)
        fm = e.mean(dim=(0, 3))
        ell = (X[None] * a[:, :, :PR_TOBS] - (a[:, :, :PR_TOBS].clamp_min(0) + torch.log1p(torch.exp(-a[:, :, :PR_TOBS].abs())))).sum(-1)
        return dict(mean=mean, m2=((z - mean[None]) ** 2).sum(0), se_mean=torch.where(has, pad(fm), zero),
                    se_m2=torch.where(has, pad(((e - fm[None, :, :, None]) ** 2).sum(dim=(0, 3))), zero), ell=torch.where(has[None], pad(ell), zero))
    lw = logw.to(dtype)
    wn = torch.softmax(lw, dim=0)
    mean = (wn[:, :, None, None] * z).sum(0)
    return dict(mean=mean, var=(wn[:, :, None, None] * (z - mean[None]) ** 2).sum(0),
                wmse=torch.where(has, pad((wn[:, :, None] * e.mean(-1)).sum(0)), zero), total=torch.exp(lw).sum(0)[:, None].expand(N, PR_TH))


def _predict_dev(Nmax, N):
    i = predict_inputs(Nmax)
    return dict(c=i['c'][:, :N].reshape(PR_L, N * PR_TH, 16, 28, 28).cuda(), table=i['table'].cuda(), w=i['w'].cuda(), b=i['b'].cuda(),
                X=i['X'][:N].contiguous().cuda(), logw=i['logw'][:, :N].contiguous())


def predict_run(dev, N, splits, ll=False, n_obs=None, X=None):
    """dec10_predict over the draws in launches of ``splits`` draws on NaN-filled state arrays with NaN guards behind them
    -> (state arrays on the CPU, tags, problems)"""
    from vae_gp_ode_amd import _lib, vae_ops as V
    F = N * PR_TH
    st = V.PredictState(F, 'cuda', True, loglik=PR_L if ll else 0)
    guards = {}
    for name, shape in (('mean', (F, 784)), ('m2', (F, 784)), ('se', (F, 3))) + ((('ell', (PR_L, F)),) if ll else ()):
        buf, guards[name] = guarded(*shape)
        setattr(st, name, buf)
    nb = None if n_obs is None else torch.as_tensor(n_obs, dtype=torch.int32).cuda()
    l0, tags = 0, []
    for k in splits:
        V.dec10_predict(dev['c'][l0:l0 + k].reshape(-1, 16, 28, 28), dev['table'], dev['w'], dev['b'], dev['X'] if X is None else X, PR_TH, st,
                        **({} if nb is None else {'n_obs': nb}))
        tags.append(_lib.load().gpode_last_launch().decode())
        l0 += k
    assert l0 == PR_L and st.done == PR_L
    torch.cuda.synchronize()
    problems = ['the guard behind %s changed' % k for k, g in guards.items() if not bool(torch.isnan(g).all())]
    out = {k: getattr(st, k).cpu().clone() for k in guards}
    problems += ['%s: a NaN of the fill is left' % k for k, v in out.items() if bool(torch.isnan(v).any())]
    return out, tags, problems


def predict_run_w(dev, N, splits, logw, n_obs=None, X=None):
    """cond_ref.run at N sequences -> (wstate, mean, m2, wse on the CPU with var, wmse, total derived as there; tags; problems)"""
    from vae_gp_ode_amd import _lib, vae_ops as V
    F = N * PR_TH
    st = V.CondState(F, N, 'cuda')
    guards = {}
    for name, shape in (('wstate', (F, 2)), ('mean', (F, 784)), ('m2', (F, 784)), ('wse', (F,))):
        buf, guards[name] = guarded(*shape)
        setattr(st, name, buf)
    lw = logw.float().contiguous().cuda()
    nb = None if n_obs is None else torch.as_tensor(n_obs, dtype=torch.int32).cuda()
    l0, tags = 0, []
    for k in splits:
        V.dec10_predict_w(dev['c'][l0:l0 + k].reshape(-1, 16, 28, 28), dev['table'], dev['w'], dev['b'], dev['X'] if X is None else X, PR_TH, st, lw,
                          n_obs=nb)
        tags.append(_lib.load().gpode_last_launch().decode())
        l0 += k
    assert l0 == PR_L and st.done == PR_L
    st.check()
    torch.cuda.synchronize()
    problems = ['the guard behind %s changed' % k for k, g in guards.items() if not bool(torch.isnan(g).all())]
    out = {k: getattr(st, k).cpu().clone() for k in guards}
    problems += ['%s: a NaN of the fill is left' % k for k, v in out.items() if bool(torch.isnan(v).any())]
    ref, Wt = out['wstate'][:, 0].double(), out['wstate'][:, 1].double()
    out['var'] = (out['m2'].double() / Wt[:, None]).view(N, PR_TH, 784)
    out['wmse'] = (out['wse'].double() / Wt).view(N, PR_TH)
    out['total'] = (Wt * torch.exp(ref)).view(N, PR_TH)
    return out, tags, problems


def predict_errors(got, r64, N):
    """{statistic: relerr} of the state arrays of predict_run against the fp64 reference; got holding the reference's own keys (the fp32
    restatement) is compared key by key"""
    if 'se' in got:
        se = got['se'].view(N, PR_TH, 3)
        got = dict(got, mean=got['mean'].view(N, PR_TH, 784), m2=got['m2'].view(N, PR_TH, 784), se_mean=se[..., 1], se_m2=se[..., 2],
                   **({'ell': got['ell'].view(PR_L, N, PR_TH)} if 'ell' in got else {}))
    return {k: relerr(got[k], r64[k]) for k in r64 if k in got}


def weighted_errors(got, r64, r32, N):
    """{statistic: (relerr, bound)} with the bound of cond_ref.check: FLOOR + 3 x the fp32 restatement's error; got None: the restatement"""
    res = {}
    for name, k in (('mean', 'mean'), ('M2/W', 'var'), ('wse/W', 'wmse'), ('W exp(ref)', 'total')):
        e32 = relerr(r32[k], r64[k])
        g = r32[k] if got is None else (got['mean'].view(N, PR_TH, 784) if k == 'mean' else got[k])
        res[name] = (relerr(g, r64[k]), FLOOR + 3 * e32)
    return res


def clear_caches():
    for f in (iw_inputs, dr_inputs, len_inputs, pkb_inputs, ga_inputs, predict_inputs, predict_images):
        f.cache_clear()
