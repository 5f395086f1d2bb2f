"""CPU: register / scratch budget of the two element-wise kernels of the wavelet-l1 FISTA (csrc/wavelet_deconv.hip), read from the
compiler's own resource report as tests/test_kernel_resources.py does.  They are memory-bound passes (the step kernel over every
coefficient, the momentum kernel over every pixel, once per iteration): none may use scratch or spill, and the step kernel
must keep the occupancy of wav_post_kernel, the sums pass of sbtv_SALSA_wavelet next to which it stands."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _report


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_fista_l1_kernels_have_no_scratch_and_the_occupancy_of_the_salsa_sums_pass():
    rep = _report("wavelet_deconv.hip")
    post = _find(rep, "wav_post_kernel")
    kernels = {"step with true": "fl1_step_kernelILb1EE", "step without true": "fl1_step_kernelILb0EE",
               "momentum": "fl1_momentum_kernel"}
    for what, name in kernels.items():
        k = _find(rep, name)
        print(what, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (what, k)
    for what in ("step with true", "step without true"):
        k = _find(rep, kernels[what])
        assert k["Occupancy"] >= post["Occupancy"], (what, k, post)
