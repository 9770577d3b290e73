"""The second convolution engine on decnn.4's input gradient (conv geometry 32 -> 64 channels, 13 -> 6, k5 s2 p1): one consumer
wavefront per SIMD with 200 weight registers, windows of 64 pixels that span up to three images, five plane buffers.  Same batch
sizes as decnn.7; the first engine sums in the same order, so that comparison is bit-identical.  The checks are conv_engine_v2.py's."""
import pytest

import conv_engine_v2 as E

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('B', E.SIZES)
def test_dec4_bwd_data_v2_against_fp64_and_first_engine(B):
    E.check_against_fp64_and_first_engine('dec4', B)


@pytest.mark.parametrize('B', [37, 4096])
def test_dec4_bwd_data_v2_deterministic(B):
    E.check_deterministic('dec4', B)


def test_dec4_bwd_data_v2_writes_only_its_output():
    E.check_writes_only_its_output('dec4')
