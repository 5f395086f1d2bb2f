"""CPU: register / scratch budget of the kernels of the SAPG loop with an SK-ROCK kernel (csrc/sapg_skrock.hip), read from the
compiler's own resource report as tests/test_kernel_resources.py does.  The stage kernels are those of csrc/skrock.hip (one
shared source, csrc/skrock_stage.inc), compiled again in this translation unit: none may use scratch or spill, and every stage
kernel must keep the occupancy of the MYULA step kernel myula_plain_kernel (csrc/elementwise.hip) next to which it stands:
<false> without moments, <true> with.  The update kernel, one workgroup per chain, calls pow / exp / log for the PSF taps: it
must not use scratch or spill either."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _report


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_sapg_skrock_kernels_have_no_scratch_and_the_occupancy_of_the_plain_myula_step():
    rep, ew = _report("sapg_skrock.hip"), _report("elementwise.hip")
    plain, mom = _find(ew, "myula_plain_kernelILb0EE"), _find(ew, "myula_plain_kernelILb1EE")
    # template <FIRST, LAST, NEXT, MOM>; NEXT: the last stage also forms the perturbed state of the next step
    stages = {"first": ("skrock_stage_kernelILb1ELb0ELb0ELb0EE", plain), "middle": ("skrock_stage_kernelILb0ELb0ELb0ELb0EE", plain),
              "last": ("skrock_stage_kernelILb0ELb1ELb1ELb0EE", plain),
              "last with moments": ("skrock_stage_kernelILb0ELb1ELb1ELb1EE", mom),
              "last of a call": ("skrock_stage_kernelILb0ELb1ELb0ELb0EE", plain),
              "last of a call with moments": ("skrock_stage_kernelILb0ELb1ELb0ELb1EE", mom)}
    others = {"perturb": "skrock_perturb_kernel", "update": "sapg_chain_update_kernel"}    # csrc/sapg_chain_update.inc
    assert len(rep) == len(stages) + len(others), sorted(rep)             # every kernel of the file is looked at
    for what, name in {**{k: v[0] for k, v in stages.items()}, **others}.items():
        k = _find(rep, name)
        print(what, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (what, k)
    for what, (name, base) in stages.items():
        k = _find(rep, name)
        assert k["Occupancy"] >= base["Occupancy"], (what, k, base)
