"""The second convolution engine on decnn.7's input gradient (conv geometry 16 -> 32 channels, 28 -> 13, k5 s2 p1): producer /
consumer wavefronts with the weights in registers and pixel tiles that span image boundaries.  Batch sizes that leave one image per
workgroup (1, 37), a partial last window (512) and several images per workgroup (4096, 8192).  The checks are conv_engine_v2.py's."""
import pytest

import conv_engine_v2 as E

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('B', E.SIZES)
def test_dec7_bwd_data_v2_against_fp64_and_first_engine(B):
    E.check_against_fp64_and_first_engine('dec7', B)


@pytest.mark.parametrize('B', [37, 4096])
def test_dec7_bwd_data_v2_deterministic(B):
    E.check_deterministic('dec7', B)


def test_dec7_bwd_data_v2_writes_only_its_output():
    E.check_writes_only_its_output('dec7')
