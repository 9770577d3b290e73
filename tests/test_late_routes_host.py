"""CPU-only checks of late_routes.py, the helper of test_gpu_late_routes.py, with no library loaded: the restated launcher arithmetic
sits on the right side of every threshold; every case sends the loop it is listed for past one trip and the operand it is listed for
sets nb_small; the case tables reach every tag and every (kernel, loop) pair of the required-coverage lists, the predict cases for
n in {64, 256, 304} compute units; and the fp32 restatement of every reference is within its bound of the fp64 reference, so the
references alone pass and a kernel that misses a bound is wrong, not unlucky."""
import pytest
import torch

import late_routes as L
import loss_routes as R


@pytest.fixture(scope='module', autouse=True)
def _drop_cached_inputs():
    yield
    L.clear_caches()


def test_restated_arithmetic_at_every_threshold():
    assert [L.ew_trips(n) for n in (1, 2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1, 2 ** 22, 2 ** 22 + 1)] == [1, 1, 1, 2, 2, 3]
    assert L.loglik_chunk(12544, 4, True) == 3136 and L.loglik_chunk(12544, 4, False) == 3137 and L.loglik_chunk(12544, 13, True) == 968
    assert L.loglik_chunk(8, 1, True) == 8 and L.loglik_chunk(1028, 64, True) == 20
    assert [L.slice_trips(c) for c in (4, 1024, 1028, 3136, 257, 3137)] == [1, 1, 2, 4, 2, 13]
    assert L.sigmoid_loglik_splits(74, 12544) == 13 and L.sigmoid_loglik_splits(1024, 12544) == 1 and L.sigmoid_loglik_splits(65535, 8) == 1
    assert L.sigmoid_loglik_splits(1280, 12544) == 1 and L.sigmoid_loglik_splits(168, 12544) == 7
    # elbo_small_blocks: each operand in turn the largest
    assert L.elbo_small_blocks(168, 7, 3, N=168, q=6) == 4 and L.elbo_small_blocks(168, 7, 3, nks=2) == 1
    assert L.elbo_small_blocks(65535, 7, 3, N=21845, q=6) == 512 and L.elbo_small_blocks(3, 30, 3, N=3, q=6) == 6
    assert L.elbo_small_blocks(3, 7, 3, nks=8200, nkv=7169) == 33
    # iw_small_blocks: N 64 lanes against P Do; M Do never decides (P >= M)
    assert [L.iw_small_blocks(2, 1, N) for N in (1, 4, 5, 8, 9, 17)] == [1, 1, 2, 2, 3, 5]
    assert L.iw_small_blocks(30, 3, 3) == 6 and L.iw_small_blocks(147, 6, 3) == 255 and L.iw_small_blocks(148, 6, 3) == 259
    for M in range(1, 40):
        for Do in (1, 3, 6):
            assert M * Do <= M * (M + 1) // 2 * Do
    assert [L.cpr(i) for i in (4, 2048, 2049, 2352, 12544)] == [1, 1, 2, 2, 7]
    assert [L.iw_group_trips(*s) for s in ((1, 16), (1, 17), (3, 11), (2, 40), (5, 256))] == [1, 2, 3, 5, 80]
    assert [L.iw_lw_trips(*s) for s in ((64, 16), (64, 17), (4, 256))] == [1, 2, 1]
    assert [L.draws_blocks(*s) for s in ((42, 6), (43, 6), (300, 16))] == [1, 2, 19]
    assert not L.us_in_parts(147, 6) and L.us_in_parts(148, 6)
    assert [L.predict_grid(F, 256) for F in (15, 256, 259)] == [15, 256, 256] and L.predict_grid(400, 304) == 256
    assert [L.predict_trips(F, 256) for F in (15, 256, 257, 512, 513)] == [1, 1, 2, 2, 3]


def test_every_case_takes_the_trip_it_is_listed_for():
    I = L.IW
    g, lw, nb = L.iw_group_trips, L.iw_lw_trips, L.iw_small_blocks
    assert g(1, 17) == 2 and g(3, 11) == 3 and 33 % 16 and g(2, 40) == 5 and 80 % 16 == 0 and lw(64, 17) == 2
    for c, want in ((I(2, 3, 5, 1, 2, 1), 2), (I(2, 3, 17, 3, 2, 1), 5), (I(2, 3, 3, 1, 30, 3), 6), (I(2, 3, 4, 1, 2, 1), 1)):
        assert c in L.IW_CASES and nb(c.M, c.Do, c.N) == want, c
    assert 3 * 64 < 30 * 31 // 2 * 3 and 17 * 64 > 3                                          # which operand sets it
    assert L.IW_CASES[-1].L * L.IW_CASES[-1].K * L.IW_CASES[-1].N == 65535 and L.IW_REFUSED.N == 65536
    assert L.expected(I(1, 2, 3, 1, 147, 6))['fwd'] == 'elbo_iw_fwd' and L.expected(I(1, 2, 3, 1, 148, 6))['fwd'] == 'elbo_iw_fwd (Us in parts)'
    # the fused backward: both inner values with nb_small = 1 and > 1; every logit-block shape has its pair among the stage cases
    for inner in (2352, 4):
        got = {nb(c.M, c.Do, c.N) > 1 for c in L.IWLL_CASES if c.frame * c.T == inner and c.L * c.K * c.N < 1000}
        assert got == {False, True}, inner
    assert L.cpr(2352) == 2 and L.cpr(4) == 1
    for c in L.IWLL_CASES:
        assert I(c.L, c.K, c.N, 1, c.M, c.Do) in L.IW_CASES, c
    # the ragged shapes: chunk 3136 on the float4 path, 3137 on the scalar one, 2^21 < n, rows = 65535
    a, s, p, big, lim = (L.LEN_CASES[i] for i in (0, 1, 3, 4, 5))
    assert L.loglik_chunk(a.T * a.frame, L.len_ns(a), True) == 3136 and L.loglik_chunk(s.T * s.frame, L.len_ns(s), False) == 3137
    assert big.L * big.N * big.T * big.frame == 2107392 > 2 ** 21 and L.ew_trips(2107392) == 2
    assert L.elbo_small_blocks(big.L * big.N, L.LM, L.LDO, N=big.N, q=L.LQ) == 4
    assert lim.L * lim.N == 65535 and lim.T * lim.frame == 8 and L.len_ns(lim) == 1 and L.LEN_REFUSED.L * L.LEN_REFUSED.N == 65536
    # the mask edge: inside a slice, exactly on a slice boundary, at a frame boundary inside a slice; and slice boundaries inside frames
    counts = L.len_counts(a.N, a.T)
    assert {0, 1, a.T, a.T + 3} <= set(counts)
    chunk = 3136
    lims = {min(k, a.T) * a.frame for k in counts}
    assert any(0 < v < a.T * a.frame and v % chunk == 0 for v in lims) and any(v % chunk for v in lims)
    chunk13 = L.loglik_chunk(p.T * p.frame, L.len_ns(p), True)
    assert chunk13 == 968 and any(0 < b < v and b % p.frame for v in lims for b in range(chunk13, p.T * p.frame, chunk13))
    assert any(v % chunk13 and v // chunk13 < 12 for v in lims)
    assert {0, 1, lim.T, lim.T + 3} <= set(L.len_counts(lim.N, lim.T))
    # the compact backward: the V4 path beyond 2^21 float4s that are no multiple of 256, the scalar path beyond 2^21 elements
    v4, sc = L.PKB_CASES
    n4, n1 = (c.L * sum(L.pkb_counts(c)) * c.frame for c in (v4, sc))
    assert not v4.mis and n4 // 4 > 2 ** 21 and (n4 // 4) % 256 and v4.L * sum(L.pkb_counts(v4)) >= 10700
    assert sc.mis and 2 ** 21 < n1 < 2 ** 21 + 2 ** 16
    for c in L.PKB_CASES:
        assert 0 in L.pkb_counts(c) and c.T in L.pkb_counts(c) and all(0 <= k <= c.T for k in L.pkb_counts(c))
    # the gather: n > 2^21 both ways, ld > q, sequences without a frame, L > 1
    ga = L.GA_CASES[0]
    P = int(L.host_index(L.ga_counts(ga), ga.T)[1][-1])
    assert ga.L * P * ga.q > 2 ** 21 and ga.L * ga.N * ga.T * ga.ld > 2 ** 21 and ga.ld > ga.q and ga.L > 1 and 0 in L.ga_counts(ga)


@pytest.mark.parametrize('n', [64, 256, 304])
def test_predict_cases_run_past_one_round(n):
    Ns = L.predict_Ns(n, L.PR_TH)
    grid = min(n, L.MAX_CUS)
    assert (Ns[0] - 1) * L.PR_TH <= grid < Ns[0] * L.PR_TH and Ns[1] == Ns[0] + 1
    assert all(L.predict_trips(N * L.PR_TH, n) == 2 for N in Ns) and any((N * L.PR_TH) % grid for N in Ns)
    seen = set()
    for c in L.predict_cases(n):
        seen |= L.loops(c, n)
    assert seen == {p for p in L.REQUIRED_LOOPS if p[1] == 'frames'}
    assert L.PR_TOBS < L.PR_TH and set(L.predict_n_obs(Ns[0])) == set(range(L.PR_TH + 1)) and sum(L.PR_SPLITS) == L.PR_L
    for N in Ns:                                      # a frame of a later round has a target, under a count other than sequence 0's
        n_obs, has = L.predict_n_obs(N), L.predict_has(N, L.predict_n_obs(N)).reshape(-1)
        later = [f for f in range(grid, N * L.PR_TH) if has[f]]
        assert later and all(n_obs[f // L.PR_TH] != n_obs[0] for f in later), (n, N)


def test_case_tables_reach_the_required_coverage():
    cases = L.all_cases()
    assert len(set(map(L.case_id, cases))) == len(cases)           # (a LEN and a PK case of one shape are equal as tuples)
    tags, loops = set(), set()
    for c in cases:
        tags.update(L.expected(c).values())
        loops |= L.loops(c)
    assert set(L.REQUIRED_TAGS) <= tags and tags - set(L.REQUIRED_TAGS) <= {'sigmoid_loglik_fwd', 'sigmoid_loglik_bwd'}
    assert loops == set(L.REQUIRED_LOOPS) and len(set(L.REQUIRED_LOOPS)) == len(L.REQUIRED_LOOPS)


def test_no_tensor_of_a_case_exceeds_the_size_limit():
    limit = 2 ** 23 + 2 ** 19                         # 34 MB of floats
    for c in L.IW_CASES:
        assert max(c.L * c.K * c.N * c.ns, c.M * (c.M + 1) // 2 * c.Do) <= limit
    for c in L.LEN_CASES + L.PK_CASES + L.PKB_CASES:
        assert c.L * c.N * c.T * c.frame <= 2 ** 23 + 2 ** 21, c
    assert L.PKB_CASES[0].L * sum(L.pkb_counts(L.PKB_CASES[0])) * 784 <= limit
    ga = L.GA_CASES[0]
    assert ga.L * ga.N * ga.T * ga.ld <= limit


# ---- the references alone pass ------------------------------------------------------------------------------------------------------------
def test_iw_and_draws_restatements_are_their_own_floor():
    res = []
    for c in L.IW_CASES:
        d = L.iw_inputs(c)
        refs, scales = L.iw_refs(c, d)
        res.append((c, L.iw_errors(None, refs, scales)))
        # the closed form the kernels implement is the autograd reference
        grow, glw = L.W.stage_grads_closed_form(L.W.rows_of(d['lpart'].double(), c.L, c.K, c.N), d['lw'].double(), L.NOBS, L.SEEDS)
        assert L._err(grow, refs[L.F64][1]) < 1e-10 and L._err(glw, refs[L.F64][2]) < 1e-10, c
    floors = L.judge(res, 'fp32 restatement of iw_ref')
    assert all(f > 0 for _, f in floors.values())
    res = []
    for c in L.DR_CASES:
        d = L.dr_inputs(c)
        refs = L.dr_refs(c, d)
        res.append((c, {k: (L._err(refs[L.F32][i], refs[L.F64][i]),) * 2 for i, k in enumerate(('gmu', 'glogvar'))}))
        col = d['gfull'].shape[-1] - c.q
        closed = L.W.draws_grads_closed_form(d['h'][:, :c.q].double(), d['h'][:, c.q:].double(), d['eps'].double(), d['gfull'][..., col:].double(),
                                             d['glw'].double())
        assert all(L._err(closed[i], refs[L.F64][i]) < 1e-10 for i in range(2)), c
    L.judge(res, 'fp32 restatement of iw_ref.draws_grads')


@pytest.mark.parametrize('c', L.LEN_CASES[:1] + L.LEN_CASES[3:], ids=L.case_id)
def test_fp32_row_sums_of_the_observed_terms_are_within_the_bound(c):
    d = L.len_inputs(c.L, c.N, c.T, c.frame)
    rows = c.L * c.N
    z = torch.sigmoid(d['a']).reshape(rows, -1)
    assert float(d['a'].abs().max()) <= R.A_MAX and float((1 - z).min()) >= R.MIN_1MZ and float(z.min()) >= R.MIN_1MZ
    obs = L.len_observed(c, 'mixed')
    t = R.bernoulli_terms(d['X'].reshape(1, -1).repeat(c.L, 1).reshape(rows, -1), z)
    t = torch.where(obs, t, torch.zeros(()))
    fake = dict(z=z, part=t.sum(1, keepdim=True), rs=t.sum(1))
    e, e2, empty = L.len_row_errors(c, 'mixed', fake)
    print(L.case_id(c), 'fp32 row sums %.2e (bound %.1e)' % (e, R.TOL))
    assert bool(empty.any()) and not bool(empty.all()) and e <= R.TOL / 4 and e2 <= R.TOL / 4


def test_fp32_compact_references_are_within_their_bounds():
    c = L.PK_CASES[0]
    counts = L.len_lengths(c, 'mixed')
    ref = L.pk_reference(c, counts)
    d = L.len_inputs(c.L, c.N, c.T, c.frame)
    cl, off, src = L.host_index(counts, c.T)
    assert off.tolist()[-1] == int(cl.sum()) and src.tolist()[:3] == [c.T, 2 * c.T, 2 * c.T + 1]          # counts (0, 1, T, ...)
    a = d['a'].reshape(c.L, c.N * c.T, c.frame)[:, src]
    z32 = torch.sigmoid(a)
    assert float((z32.double() - ref['z']).abs().max()) <= R.TOL_Z / 4
    viaz = L.pk_reference(c, counts, z32)['ga']        # the kernel's expression on the fp32 z against grow (x - sigmoid(a))
    assert L._err(viaz, ref['ga']) <= 2e-5 / 4
    for pc in L.PKB_CASES[1:]:
        cnt = L.pkb_counts(pc)
        assert L._err(L.pkb_reference(pc, cnt, L.F32), L.pkb_reference(pc, cnt)) <= 2e-5 / 4
    ga = L.GA(2, 7, 4, 3, 5)
    out, gzt = L.ga_reference(ga)
    cl, off, src = L.host_index(L.ga_counts(ga), ga.T)
    want = torch.stack([L.ga_inputs(ga)['zt'][l, s // ga.T, s % ga.T, :ga.q] for l in range(ga.L) for s in src.tolist()])
    assert torch.equal(out, want) and float(gzt.abs().sum()) > 0 and bool((gzt[..., ga.q:] == 0).all()) and bool((gzt[:, 0] == 0).all())


def test_fp32_predict_restatements_are_within_their_bounds():
    Ns = L.predict_Ns(64, L.PR_TH)
    N, Nmax = Ns[0], Ns[1]
    for n_obs in (None, L.predict_n_obs(N)):
        r64, r32 = (L.predict_reference(Nmax, N, dt, n_obs) for dt in (L.F64, L.F32))
        errs = L.predict_errors(r32, r64, N)
        print('unweighted', errs)
        assert set(errs) == {'mean', 'm2', 'se_mean', 'se_m2', 'ell'} and all(e <= L.PREDICT_TOL / 4 for e in errs.values()), errs
        logw = L.predict_inputs(Nmax)['logw'][:, :N].double()
        w64, w32 = (L.predict_reference(Nmax, N, dt, n_obs, logw) for dt in (L.F64, L.F32))
        res = L.weighted_errors(None, w64, w32, N)
        assert all(e <= bound for e, bound in res.values()), res
    has = L.predict_has(N, L.predict_n_obs(N))
    assert bool(has.any()) and not bool(has[:, L.PR_TOBS:].any()) and bool((~has.any(1)).any()) and int(has.sum()) < N * L.PR_TOBS
    assert bool((r64['ell'][:, ~has] == 0).all()) and bool((r64['ell'][:, has] < -100).all())
