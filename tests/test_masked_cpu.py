"""CPU: the boundary of the masked-observation SALSA (sbtv_SALSA_masked), the restatement its GPU parity tests use
(tests/masked_restatement.py) anchored on the oracle's SALSA_v2, the two mask helpers, and the register report of the new
element-wise kernels (hipcc cross-compiles gfx950 without a GPU)."""
import os
import re

import numpy as np
import pytest

from conftest import synth_image
from test_kernel_resources import HIPCC, _find, _report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_masked_entry_points_declared_exported_and_bound():
    import sbtv
    from sbtv import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbtv.h")).read(), flags=re.S)
    lib = sbtv.load_library()
    for name, nargs in (("sbtv_SALSA_masked", 23), ("sbtv_SALSA_masked_sharded", 22)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in include/sbtv.h"
        assert len(m.group(1).split(",")) == nargs
        assert hasattr(lib, name), f"{name} is not exported by libsbtv.so"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert callable(sbtv.SALSA_masked) and callable(sbtv.valid_mask) and callable(sbtv.embed_observation)


def _setup(x, params=(0.4, 0.3), seed=3):
    import sbtv_oracle as o
    rng = np.random.default_rng(seed)
    return o.demo_setup("gaussian", x, rng.standard_normal(x.shape), evMax=1.0, BSNR=30.0, true_params=params)


@pytest.mark.parametrize("mu2", [1.0, 0.3])
def test_restatement_with_a_full_mask_lands_on_the_oracles_salsa(mu2):
    """m = 1: the same problem as SALSA_v2 with tau and mu = mu1.  Bars: PSNR between the two images >= 60 dB, final
    objectives to rtol 1e-5 (the prototype: 101 dB / 1.3e-6 at mu2 = 1, 92 dB / 1.9e-6 at mu2 = 0.3)."""
    import sbtv_oracle as o
    import masked_restatement as mr
    x = synth_image(128, 128, 4)
    st = _setup(x)
    m, p = st["model"], st["p_true"]
    H = m.H_FFT(*p)
    H2 = np.abs(H) ** 2
    theta, s2 = 0.03, st["sigma"] ** 2
    tau, mu1 = theta * s2, theta / 10
    ref = o.SALSA_v2(st["y"], lambda z: m.A(z, *p), tau, mu=mu1, AT=lambda z: m.AT(z, *p),
                     invLS=lambda r: np.real(o.ifft2(o.fft2(r) / (H2 + mu1))), true_x=x, stopcriterion=1, tolA=1e-7,
                     maxiter=2000, TViters=10, initialization=0)
    got = mr.salsa_masked(st["y"], np.ones_like(x), H, tau, mu1, mu2, true_x=x, stopcriterion=1, tolA=1e-7, maxiter=2000,
                          TViters=10, initialization=0)
    psnr = o.PSNR(ref["x"], got["x"])
    rel = abs(got["objective"][-1] - ref["objective"][-1]) / ref["objective"][-1]
    print(f"mu2 = {mu2}: {got['n_outer']} against {ref['n_outer']} outer iterations, {psnr:.1f} dB between the images, "
          f"objectives {rel:.2e} apart")
    assert psnr >= 60.0
    assert rel <= 1e-5
    assert got["numA"] == 1 + got["n_outer"] and got["numAt"] == got["n_outer"]
    assert got["distance"].shape == (got["n_outer"], 2)
    assert len(got["objective"]) == len(got["mses"]) == len(got["times"]) == got["n_outer"] + 1


def test_valid_mask_and_embed_observation():
    import sbtv
    import sbtv_oracle as o
    import masked_restatement as mr
    rng = np.random.default_rng(11)
    scene = rng.uniform(0.0, 255.0, (64, 48))
    taps = o.Gaussian_psf(7, 0.4, 0.3)
    t = taps.shape[0]
    model = o.BlurModel("gaussian", scene.shape)
    Ax = model.A(scene, 0.4, 0.3)
    mask = sbtv.valid_mask(scene.shape, t)
    assert mask.shape == scene.shape and set(np.unique(mask)) == {0.0, 1.0}
    assert np.all(mask[t - 1:, t - 1:] == 1) and mask.sum() == (64 - t + 1) * (48 - t + 1)
    lin = mr.valid_convolution(scene, taps)
    err = np.max(np.abs(Ax[t - 1:, t - 1:] - lin)) / np.max(np.abs(lin))
    print(f"circular blur on the mask against the 'valid' linear convolution: {err:.2e}")
    assert err <= 1e-12
    y, m2 = sbtv.embed_observation(lin, t)
    assert y.shape == m2.shape == scene.shape
    np.testing.assert_array_equal(m2, mask)
    np.testing.assert_array_equal(y[t - 1:, t - 1:], lin)
    assert not y[:t - 1].any() and not y[:, :t - 1].any()
    # a larger domain (e.g. the next power of two): zeros in both outside the observation
    y3, m3 = sbtv.embed_observation(lin, t, shape=(128, 64))
    assert y3.shape == m3.shape == (128, 64)
    np.testing.assert_array_equal(y3[t - 1:64, t - 1:48], lin)
    np.testing.assert_array_equal(m3[t - 1:64, t - 1:48], 1.0)
    assert m3.sum() == lin.size and np.count_nonzero(y3) == np.count_nonzero(lin)
    assert not y3[64:].any() and not y3[:, 48:].any() and not m3[64:].any() and not m3[:, 48:].any()
    with pytest.raises(ValueError):
        sbtv.embed_observation(lin, t, shape=(64, 47))
    # taille 1: everything is valid
    np.testing.assert_array_equal(sbtv.valid_mask((8, 6), 1), np.ones((8, 6)))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_masked_elementwise_kernels_use_no_scratch():
    rep = _report("admm.hip")
    for parts in (("masked_post_kernel", "Lb1E"), ("masked_post_kernel", "Lb0E"), ("masked_my_kernel",)):
        k = _find(rep, *parts)
        print(parts, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, (parts, k)
        assert k["Occupancy"] >= 4, (parts, k)          # a streaming pass: enough waves to hide the loads
