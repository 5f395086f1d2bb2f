"""CPU: register / scratch budget of the pixel pass of the masked-observation wavelet SALSA, read from the compiler's own resource
report as tests/test_kernel_resources_csalsa_wavelet.py does: ma_pixel_kernel (csrc/masked_wavelet.hip), the one streaming pass
over every pixel of an outer iteration (five arrays read, two written).  It is memory-bound: no scratch, no spill, occupancy 8.
wav_astep_kernel must be compiled in the new unit with the 48 VGPRs it has elsewhere, and masked_my_kernel, which moved into a
shared include (csrc/masked_my.inc), alike in both units; the other kernels of admm.hip keep the registers and occupancy they had
before the move (the figures below are those of the parent commit's report)."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _report

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# admm.hip before masked_my_kernel moved out: kernel -> (VGPRs, Occupancy)
ADMM_BEFORE = {
    "csalsa_update_kernel": (54, 8), "csalsa_post_kernel": (40, 8), "coral_s_kernelILb1E": (60, 8), "coral_s_kernelILb0E": (28, 8),
    "coral_post_kernel": (56, 8), "masked_my_kernel": (16, 8), "masked_post_kernelILb1E": (72, 7), "masked_post_kernelILb0E": (68, 7),
    "csalsa_scal_kernel": (17, 8), "csalsa_w_kernel": (22, 8), "csalsa_ve_kernel": (26, 8), "ad_sub_kernel": (16, 8),
}


@pytest.fixture(scope="module")
def reports():
    return {u: _report(u + ".hip") for u in ("masked_wavelet", "admm", "wavelet_deconv")}


def _clean(k):
    return k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0


def test_pixel_pass_has_no_scratch_and_full_occupancy(reports):
    k = _find(reports["masked_wavelet"], "ma_pixel_kernel")
    print("ma_pixel_kernel", k)
    assert _clean(k), k
    assert k["Occupancy"] == 8, k


def test_shared_kernels_are_compiled_alike_in_the_old_units_and_the_new_one(reports):
    new = reports["masked_wavelet"]
    for unit, names in (("wavelet_deconv", ("wav_astep_kernel", "wav_init_kernel", "wav_cstep_kernel")), ("admm", ("masked_my_kernel",))):
        for name in names:
            a, b = _find(new, name), _find(reports[unit], name)
            print(name, a, b)
            assert _clean(a) and _clean(b), (name, a, b)
            assert a["Occupancy"] == b["Occupancy"] and a["VGPRs"] == b["VGPRs"], (name, a, b)
    assert _find(new, "wav_astep_kernel")["VGPRs"] == 48


def test_kernels_of_admm_are_unchanged_by_the_move(reports):
    rep = reports["admm"]
    for name, want in ADMM_BEFORE.items():
        k = _find(rep, name)
        print(name, k)
        assert _clean(k), (name, k)
        assert (k["VGPRs"], k["Occupancy"]) == want, (name, k)
