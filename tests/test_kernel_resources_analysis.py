"""CPU: register / scratch budget of the step kernel of the analysis-prior wavelet SALSA (wav_astep_kernel, csrc/wavelet_deconv.hip), read
from the compiler's own resource report as tests/test_kernel_resources.py does.  It is a memory-bound streaming pass over every
coefficient (five arrays, four sums), once per outer iteration: it may not use scratch or spill, and it must keep the occupancy
of wav_post_kernel, the sums pass of sbtv_SALSA_wavelet that it replaces."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _report


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_analysis_step_kernel_has_no_scratch_and_the_occupancy_of_the_salsa_sums_pass():
    rep = _report("wavelet_deconv.hip")
    post = _find(rep, "wav_post_kernel")
    k = _find(rep, "wav_astep_kernel")
    print("step", k, "\npost", post)
    assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["Occupancy"] >= post["Occupancy"], (k, post)
