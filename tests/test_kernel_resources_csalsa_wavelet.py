"""CPU: register / scratch budget of the two new passes of C-SALSA with the wavelet analysis prior, read from the compiler's own
resource report as tests/test_kernel_resources.py does: wav_cstep_kernel (csrc/wav_step.inc), the one streaming pass over every
coefficient of an outer iteration, and csalsa_split_kernel (csrc/csalsa_wavelet.hip), the pixel pass of the image form.  Both are
memory-bound: they may not use scratch or spill, and they must keep at least the occupancy of wav_astep_kernel, which moves one
array more.  The kernels that moved into shared includes (csalsa_step.inc, ad_xsums.inc) and those of wav_step.inc must be
compiled by every unit that includes them, with the same registers and occupancy in each."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _report

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def reports():
    return {u: _report(u + ".hip") for u in ("csalsa_wavelet", "admm", "wavelet_deconv")}


def _clean(k):
    return k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0


def test_new_passes_have_no_scratch_and_the_occupancy_of_the_analysis_step(reports):
    new = reports["csalsa_wavelet"]
    ref = _find(new, "wav_astep_kernel")
    for name in ("wav_cstep_kernel", "csalsa_split_kernel"):
        k = _find(new, name)
        print(name, k, "\nwav_astep_kernel", ref)
        assert _clean(k), k
        assert k["Occupancy"] >= ref["Occupancy"], (k, ref)
    assert _find(new, "wav_cstep_kernel")["VGPRs"] <= ref["VGPRs"]


@pytest.mark.parametrize("unit, names", [
    ("admm", ("csalsa_scal_kernel", "csalsa_w_kernel", "csalsa_ve_kernel")),
    ("wavelet_deconv", ("ad_xsums_kernel", "wav_init_kernel", "wav_astep_kernel", "wav_cstep_kernel")),
])
def test_shared_kernels_are_compiled_alike_in_the_old_units_and_the_new_one(reports, unit, names):
    new, old = reports["csalsa_wavelet"], reports[unit]
    for name in names:
        a, b = _find(new, name), _find(old, name)
        print(name, a, b)
        assert _clean(a) and _clean(b), (name, a, b)
        assert a["Occupancy"] == b["Occupancy"] and a["VGPRs"] == b["VGPRs"], (name, a, b)
