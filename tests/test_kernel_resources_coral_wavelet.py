"""CPU: register / scratch budget of the two pixel passes of CoRAL with the TV + wavelet-l1 regulariser (cw_s_kernel, cw_post_kernel,
csrc/coral_wavelet.hip), read from the compiler's own resource report as tests/test_kernel_resources.py does.  Both are memory-bound
streaming passes over every pixel, once per outer iteration: they may not use scratch or spill, and they must keep the occupancy
of the TV/TV passes they are cut down from (coral_s_kernel<true>, coral_post_kernel in csrc/admm.hip), which read one array more
(the s pass) or three more (the post pass).  The kernels that moved into shared includes must still be compiled by the units
they came from, with nothing spilled."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _report

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def reports():
    return _report("coral_wavelet.hip"), _report("admm.hip")


def _clean(k):
    return k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0


def test_s_pass_has_no_scratch_and_the_occupancy_of_the_tv_tv_pass(reports):
    new, old = reports
    ref = _find(old, "coral_s_kernelILb1E")
    for variant in ("cw_s_kernelILb1E", "cw_s_kernelILb0E"):
        k = _find(new, variant)
        print(variant, k, "\ncoral_s_kernel<true>", ref)
        assert _clean(k), k
        assert k["Occupancy"] >= ref["Occupancy"], (k, ref)


def test_post_pass_has_no_scratch_and_the_occupancy_of_the_tv_tv_pass(reports):
    new, old = reports
    ref = _find(old, "coral_post_kernel")
    k = _find(new, "cw_post_kernel")
    print("cw_post_kernel", k, "\ncoral_post_kernel", ref)
    assert _clean(k), k
    assert k["Occupancy"] >= ref["Occupancy"], (k, ref)


def test_shared_step_kernels_are_compiled_in_both_units_without_scratch(reports):
    new, _ = reports
    deconv = _report("wavelet_deconv.hip")
    for name in ("wav_astep_kernel", "wav_init_kernel"):
        a, b = _find(new, name), _find(deconv, name)
        assert _clean(a) and _clean(b), (name, a, b)
        assert a["Occupancy"] == b["Occupancy"] and a["VGPRs"] == b["VGPRs"], (name, a, b)
