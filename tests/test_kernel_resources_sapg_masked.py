"""CPU: register / scratch budget of the kernels of the masked-observation MYULA / SAPG loops (csrc/sapg_masked.hip), read from
the compiler's own resource report as tests/test_kernel_resources.py does.  The residual kernel is a bandwidth-bound
element-wise pass (both variants: with and without the derivative sums), the count kernel runs once per call, and the update
kernel, one workgroup per chain, calls pow / exp / log for the PSF taps: none may use scratch or spill."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _report


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_sapg_masked_kernels_have_no_scratch_and_do_not_spill():
    rep = _report("sapg_masked.hip")
    kernels = {"residual with the derivative sums": "masked_resid_kernelILb1EE", "residual": "masked_resid_kernelILb0EE",
               "count": "masked_count_kernel", "update": "sapg_chain_update_kernel"}    # the update: csrc/sapg_chain_update.inc
    assert len(rep) == len(kernels), sorted(rep)                          # every kernel of the file is looked at
    for what, name in kernels.items():
        k = _find(rep, name)
        print(what, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (what, k)
    # the element-wise pass keeps every wave slot of a SIMD
    for name in ("masked_resid_kernelILb1EE", "masked_resid_kernelILb0EE"):
        assert _find(rep, name)["Occupancy"] == 8, name
