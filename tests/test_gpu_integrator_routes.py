"""Every route of the fixed-grid integrator and its reverse sweep (rhs_fwd, rollout_fwd, rollout_bwd, rhs_vjp, param_grad,
rollout_bwd_pgrad) against the fp64 oracle evaluated on the cache the GPU built: tests/integrator_routes.py has the case table, the
restated dispatch, the launches and the reference; tests/test_integrator_routes_host.py checks that table and the reference without a
GPU, and that a dropped feature, a dropped inducing point, another Runge-Kutta rule or another step's dt is 10 x past the bounds used here.

Per case (integrator_routes.run_case / check_case): (a) gpode_last_launch() after rhs, rollout, rollout_bwd, rhs_vjp and param_grad
equals what expected() names -- the evaluators have a tag each (rhs_rbf_reg42, rollout_df_lds ...), and param_grad reports its
parameter-sum kernel, so a fallback to a neighbouring route fails here; (b) no guard behind f, zt, xstage, gz0, astage, gx, gpack or
the slab changed; (c) no output entry is left NaN -- every row of zt, every stage row of xstage and astage, every live lane of the
pack-layout gradient (its slab is NaN-filled, so a chunk that was summed without having been written shows); (d) a second run is
bit-identical; (e) every output is within FLOOR + 3 relerr(fp32 oracle, fp64) of the fp64 oracle."""
import pytest

import integrator_routes as IR

pytestmark = pytest.mark.gpu
SEEN = set()


@pytest.mark.parametrize('c', IR.CASES, ids=IR.case_id)
def test_route(c):
    IR.check_case(c, IR.run_case(c), SEEN)


@pytest.mark.parametrize('c', IR.ACC_CASES, ids=IR.case_id)
def test_param_grad_with_unused_chunks_and_accumulate(c):
    """R = 10 rows in 7 chunks of 2: five chunks are used, and the reduction must not read the other two (they hold NaN), for either
    draw; accumulate = 1 adds the same sums to what gpack holds."""
    IR.check_accumulate(c, IR.run_accumulate(c), SEEN)


def test_every_route_was_taken():
    """The union of gpode_last_launch() over the tests above equals the list of routes (run after them; skips on its own)."""
    if not SEEN:
        pytest.skip('runs after the cases of this file')
    assert SEEN == set(IR.REQUIRED_TAGS), (SEEN ^ set(IR.REQUIRED_TAGS))
