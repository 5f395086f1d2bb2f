"""CPU: register / scratch budget of the SK-ROCK element-wise kernels (csrc/wavelet_chain.hip), read from the compiler's own
resource report as tests/test_kernel_resources.py does.  They are memory-bound passes over every coefficient, `stages` of them
per step: none may use scratch, and the three that run in every step (first, middle and last stage) must keep the occupancy of
the MYULA step kernel wav_step_kernel<false>, next to which they stand."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _report


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_skrock_stage_kernels_have_no_scratch_and_the_occupancy_of_the_myula_step():
    rep = _report("wavelet_chain.hip")
    step = _find(rep, "wav_step_kernelILb0EE")
    assert step["ScratchSize"] == 0, step
    # template <FIRST, LAST, NEXT, MOM>; NEXT: the last stage also forms the perturbed state of the next step
    per_step = {"first": "wav_skrock_stage_kernelILb1ELb0ELb0ELb0EE", "middle": "wav_skrock_stage_kernelILb0ELb0ELb0ELb0EE",
                "last": "wav_skrock_stage_kernelILb0ELb1ELb1ELb0EE"}
    others = {"last with moments": "wav_skrock_stage_kernelILb0ELb1ELb1ELb1EE",
              "last of a call": "wav_skrock_stage_kernelILb0ELb1ELb0ELb0EE",
              "last of a call with moments": "wav_skrock_stage_kernelILb0ELb1ELb0ELb1EE", "perturb": "wav_skrock_perturb_kernel"}
    for what, name in {**per_step, **others}.items():
        k = _find(rep, name)
        print(what, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (what, k)
    for what, name in per_step.items():
        k = _find(rep, name)
        assert k["Occupancy"] >= step["Occupancy"], (what, k, step)
    mom = _find(rep, "wav_step_kernelILb1EE")
    assert _find(rep, others["last with moments"])["Occupancy"] >= mom["Occupancy"], mom
