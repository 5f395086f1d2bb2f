"""CPU: the wavelet-l1 path without a GPU.  The NumPy restatement of the redundant wavelet frame (tests/wavelet_restatement.py)
is held to the frame identities and to the worked example of the reference's doc comment (SALSA/mrdwt.m:38-40); `daubcqf`
(host code of the package) to the closed forms and the defining properties; the boundary (header, exports, ctypes table);
the literal SALSA_v2 iteration against the operator form the library runs; and the compiler's resource report of the new
kernels (hipcc cross-compiles gfx950 without a GPU)."""
import math
import os
import re

import numpy as np
import pytest

from test_kernel_resources import HIPCC, _find, _report

import wavelet_cases as wc
import wavelet_restatement as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(24, 20), (17, 9), (64, 64), (30, 14)]


def _levels_for(shape, K):
    """The deepest decomposition up to levels = 4 that the size admits: (K-1) 2^(levels-2) < min(shape)."""
    levels = 4
    while (K - 1) * 2 ** (levels - 2) >= min(shape):
        levels -= 1
    assert levels >= 2
    return levels


@pytest.mark.parametrize("K", [2, 4, 8])
@pytest.mark.parametrize("shape", SIZES)
def test_restatement_is_a_parseval_frame_with_its_exact_adjoint(shape, K):
    import sbtv
    h = sbtv.daubcqf(K)
    levels = _levels_for(shape, K)
    rng = np.random.default_rng(K + shape[0])
    x = rng.standard_normal(shape)
    z = wr.mrdwt_TI2D(x, h, levels)
    assert z.shape == (shape[0], (3 * (levels - 1) + 1) * shape[1])
    c = rng.standard_normal(z.shape)
    pars = abs(np.linalg.norm(z) / np.linalg.norm(x) - 1.0)
    lhs, rhs = float(np.vdot(z, c)), float(np.vdot(x, wr.mirdwt_TI2D(c, h, levels)))
    adj = abs(lhs - rhs) / (np.linalg.norm(z) * np.linalg.norm(c))
    rec = np.max(np.abs(wr.mirdwt_TI2D(z, h, levels) - x)) / np.max(np.abs(x))
    print(f"{shape} K={K} levels={levels}: Parseval {pars:.1e}, adjoint {adj:.1e}, W W'x - x {rec:.1e}")
    assert pars <= 1e-12 and adj <= 1e-12 and rec <= 1e-12


def test_known_answer_of_the_reference_doc_comment():
    """SALSA/mrdwt.m:38-40: a delta at 0-based index 1 of 8 samples, D4, one level: yl = [0.8365 0.4830 0 0 0 0 -0.1294 0.2241]
    and yh = [-0.2241 -0.1294 0 0 0 0 -0.4830 0.8365] (four printed decimals: tolerance 5e-5).  In 2-D, on the delta at (1, 1)
    with levels = 2, band 0 is outer(yl, yl) / 2: the 1 / sqrt 2 per dimension is the rescaling of mrdwt_TI2D.m:19-23."""
    import sbtv
    yl = np.array([0.8365, 0.4830, 0, 0, 0, 0, -0.1294, 0.2241])
    yh = np.array([-0.2241, -0.1294, 0, 0, 0, 0, -0.4830, 0.8365])
    x = np.zeros((8, 8))
    x[1, 1] = 1.0
    z = wr.mrdwt_TI2D(x, sbtv.daubcqf(4), 2)
    assert z.shape == (8, 32)
    assert np.max(np.abs(z[:, 0:8] - np.outer(yl, yl) / 2)) <= 5e-5
    assert np.max(np.abs(z[:, 8:16] - np.outer(yl, yh) / 2)) <= 5e-5       # LH: low along dimension 1, high along 2
    assert np.max(np.abs(z[:, 16:24] - np.outer(yh, yl) / 2)) <= 5e-5      # HL
    assert np.max(np.abs(z[:, 24:32] - np.outer(yh, yh) / 2)) <= 5e-5      # HH


def test_daubcqf():
    import sbtv
    np.testing.assert_allclose(sbtv.daubcqf(2), wr.daub_closed_form(2), rtol=0, atol=1e-14)
    np.testing.assert_allclose(sbtv.daubcqf(4), wr.daub_closed_form(4), rtol=0, atol=1e-14)
    np.testing.assert_allclose(sbtv.daubcqf(4), [0.48296, 0.83652, 0.22414, -0.12941], atol=1e-5)
    for N in (6, 8):
        h = sbtv.daubcqf(N)
        assert h.shape == (N,)
        assert abs(h.sum() - math.sqrt(2.0)) <= 1e-10
        for m in range(N // 2):
            d = float(np.dot(h[:N - 2 * m], h[2 * m:]))
            assert abs(d - (1.0 if m == 0 else 0.0)) <= 1e-10, (N, m, d)
        k = np.arange(N)
        for p in range(N // 2):
            assert abs(np.sum((-1.0) ** k * k ** p * h)) <= 1e-10, (N, p)
        # minimum phase: no zero of the filter outside the unit circle (the N/2-fold zero at -1 comes back from np.roots
        # split by about eps^(2/N), 1e-4 for N = 8: the other zeros must lie well inside)
        assert np.all(np.abs(np.roots(h)) <= 1.0 + 1e-3)
        assert np.sum(np.abs(np.roots(h)) < 0.9) == N // 2 - 1
    with pytest.raises(ValueError):
        sbtv.daubcqf(3)


def test_wavelet_entry_points_declared_exported_and_bound():
    import sbtv
    from sbtv import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbtv.h")).read(), flags=re.S)
    lib = sbtv.load_library()
    for name, nargs in (("sbtv_mrdwt_TI2D", 10), ("sbtv_mirdwt_TI2D", 10), ("sbtv_soft", 8), ("sbtv_SALSA_wavelet", 25),
                        ("sbtv_diag_wavelet_geometry", 7)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in include/sbtv.h"
        assert len(m.group(1).split(",")) == nargs
        assert hasattr(lib, name), f"{name} is not exported by libsbtv.so"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    for fn in ("mrdwt_TI2D", "mirdwt_TI2D", "soft", "daubcqf", "SALSA_wavelet"):
        assert callable(getattr(sbtv, fn)) and fn in sbtv.__all__


def test_literal_iteration_and_operator_form_agree():
    """Case (a) of the GPU tests (64 x 64, Haar, levels 4, stop rule 1): the literal SALSA_v2 iteration and the operator form
    stop at the same iteration, strictly inside (2, MAXITERA), and their objectives agree to rtol 1e-10."""
    p, ref = wc.problem("a"), wc.reference("a")
    got = wr.salsa_wavelet_operator(p["y"], p["H"], p["h"], p["levels"], p["tau"], p["mu"], true_xw=p["true_xw"],
                                    stopcriterion=p["stop"], tolA=p["tolA"], maxiter=p["maxiter"], initialization=p["init"])
    print(f"stopped at {ref['n_outer']} / {got['n_outer']} of {p['maxiter']}, objectives "
          f"{np.max(np.abs(got['objective'] / ref['objective'] - 1)):.1e} apart, coefficients "
          f"{np.max(np.abs(got['xw'] - ref['xw'])):.1e}, images {np.max(np.abs(got['x'] - ref['x'])):.1e}")
    assert got["n_outer"] == ref["n_outer"]
    assert 2 < ref["n_outer"] < p["maxiter"]
    np.testing.assert_allclose(got["objective"], ref["objective"], rtol=1e-10)
    assert (got["numA"], got["numAt"]) == (ref["numA"], ref["numAt"]) == (1 + ref["n_outer"], 1)
    assert np.max(np.abs(got["xw"] - ref["xw"])) < 1e-8 and np.max(np.abs(got["x"] - ref["x"])) < 1e-8


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_wavelet_tile_kernels_fit_two_workgroups_per_cu_without_scratch():
    rep = _report("wavelet.hip")
    for kern in ("wav_analysis_kernel", "wav_synthesis_kernel"):
        for K in (2, 4, 6, 8):
            k = _find(rep, kern, f"ILi{K}E")
            print(kern, K, k)
            assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, (kern, K, k)
            assert 0 < k["LDS Size"] <= 80 * 1024, (kern, K, k)
            assert k["Occupancy"] >= 2, (kern, K, k)
    k = _find(rep, "wav_soft_kernel")
    assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, k


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_wavelet_solver_elementwise_kernels_use_no_scratch():
    rep = _report("wavelet_deconv.hip")
    for name in ("wav_init_kernel", "wav_prox_kernel", "wav_post_kernel", "wav_sum_kernel"):
        k = _find(rep, name)
        print(name, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, (name, k)
        assert k["Occupancy"] >= 4, (name, k)           # streaming passes: enough waves to hide the loads
