"""CPU: register / scratch budget of the SK-ROCK element-wise kernels of the TV sampler (csrc/skrock.hip), read from the
compiler's own resource report as tests/test_kernel_resources.py does.  They are memory-bound passes over every pixel, `stages`
of them per step: none may use scratch or spill, and every stage kernel must keep the occupancy of the MYULA step kernel
myula_plain_kernel (csrc/elementwise.hip) next to which it stands: <false> without moments, <true> with."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _report


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_skrock_tv_kernels_have_no_scratch_and_the_occupancy_of_the_plain_myula_step():
    rep, ew = _report("skrock.hip"), _report("elementwise.hip")
    plain, mom = _find(ew, "myula_plain_kernelILb0EE"), _find(ew, "myula_plain_kernelILb1EE")
    # template <FIRST, LAST, NEXT, MOM>; NEXT: the last stage also forms the perturbed state of the next step
    stages = {"first": ("skrock_stage_kernelILb1ELb0ELb0ELb0EE", plain), "middle": ("skrock_stage_kernelILb0ELb0ELb0ELb0EE", plain),
              "last": ("skrock_stage_kernelILb0ELb1ELb1ELb0EE", plain),
              "last with moments": ("skrock_stage_kernelILb0ELb1ELb1ELb1EE", mom),
              "last of a call": ("skrock_stage_kernelILb0ELb1ELb0ELb0EE", plain),
              "last of a call with moments": ("skrock_stage_kernelILb0ELb1ELb0ELb1EE", mom)}
    others = {"perturb": "skrock_perturb_kernel", "trace": "skrock_trace_kernel"}
    names = [n for n in rep if "skrock" in n]
    assert len(names) == len(stages) + len(others), names                 # every instantiation is looked at
    for what, name in {**{k: v[0] for k, v in stages.items()}, **others}.items():
        k = _find(rep, name)
        print(what, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (what, k)
    for what, (name, base) in stages.items():
        k = _find(rep, name)
        assert k["Occupancy"] >= base["Occupancy"], (what, k, base)
