"""CPU: the fixed-theta MYULA chain of the wavelet-l1 model (sbtv_myula_wavelet) without a GPU.  The boundary (header,
exports, ctypes mirror of the option struct against gcc, MATLAB shim); the restatement the GPU tests compare with
(tests/wavelet_myula_restatement.py) tied to the literal restatement of SALSA/SAPG_algorithm_1.m, whose warm-up loop it is; its
Welford form against a two-pass mean / variance; and the compiler's resource report of the new kernels."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from test_kernel_resources import HIPCC, _find, _report

import wavelet_myula_restatement as wmr
import wavelet_posterior_cases as wpc
import wavelet_sapg_cases as wsc
import wavelet_sapg_restatement as wsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_declared_exported_bound_and_shimmed():
    import sbtv
    from sbtv import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbtv.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+sbtv_myula_wavelet\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "sbtv_myula_wavelet is not declared in include/sbtv.h"
    assert len(m.group(1).split(",")) == 25 == len(_lib.SIGNATURES["sbtv_myula_wavelet"][1])
    assert hasattr(sbtv.load_library(), "sbtv_myula_wavelet")
    assert callable(sbtv.myula_wavelet) and "myula_wavelet" in sbtv.__all__
    shim = open(os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd", "matlab", "sbtv_myula_wavelet.m")).read()
    assert "'sbtv_myula_wavelet'" in shim and "libstruct('sbtv_myula_wavelet_opts')" in shim


def test_opts_layout_matches_header():
    from sbtv import _lib
    fields = ["samples", "lambda", "gamma", "seed", "chain_offset"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sbtv.h"\nint main(void){printf("%zu'
           + " %zu" * len(fields) + '\\n", sizeof(sbtv_myula_wavelet_opts)'
           + "".join(f", offsetof(sbtv_myula_wavelet_opts, {f})" for f in fields) + ");return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "t")], check=True, capture_output=True,
                                              text=True).stdout.split()]
    m = _lib.sbtv_myula_wavelet_opts
    assert [n.rstrip("_") for n, _ in m._fields_] == fields
    assert out == [C.sizeof(m)] + [getattr(m, n).offset for n, _ in m._fields_]


def test_restatement_at_th_init_is_the_warmup_of_the_literal_loop():
    """The literal restatement of SAPG_algorithm_1.m with warmup = S runs S - 1 MYULA steps at theta = th_init and books
    logPiTrace_WU(ii) = logPi(X_wu(ii)), ii = 2..S: the same chain and the same log-density as the new restatement's
    samples 2..S with the same noise."""
    p = wsc.problem("a")
    S = 12
    op = dict(p["op"], warmup=S, samples=2, burnIn=2)
    nz = np.random.default_rng(31).standard_normal((S, p["y"].shape[1], wsc.bands(p["levels"]) * p["y"].shape[2]))
    _, lit = wsr.sapg_wavelet_literal(p["y"][0], p["H"], p["h"], p["levels"], op, nz)
    got = wmr.myula_wavelet_chain(p["y"][0], p["H"], p["h"], p["levels"], dict(op, samples=S + 1), op["th_init"], op["sigma2"],
                                  nz)
    np.testing.assert_allclose(got["logpi"][1:S], lit["logPiTrace_WU"][1:], rtol=1e-12, atol=0)
    # ... and one more step at theta(1) = th_init is the literal loop's ii = 2
    assert np.max(np.abs(got["samples"][S] - lit["Xlast_sample"])) <= 1e-12 * np.max(np.abs(lit["Xlast_sample"]))
    np.testing.assert_allclose(got["logpi"][S - 1], lit["logPiTraceX"][0], rtol=1e-12, atol=0)


@pytest.mark.parametrize("first,thin", [(1, 1), (3, 2), (24, 1)])
def test_welford_of_the_restatement_images_equals_two_pass(first, thin):
    imgs = wpc.reference("a")[0]["images"][first - 1::thin]
    (m, v), (m2, v2) = wmr.welford(imgs), wmr.two_pass(imgs)
    np.testing.assert_allclose(m, m2, rtol=1e-12, atol=0)
    np.testing.assert_allclose(v, v2, rtol=1e-12, atol=1e-12 * float(np.max(v2)))
    assert len(imgs) == (24 - first) // thin + 1


def test_images_of_the_restatement_are_the_synthesis_of_its_samples_and_traces_are_defined_everywhere():
    import wavelet_restatement as wr
    p, r = wpc.problem("c"), wpc.reference("c")[0]
    S = p["op"]["samples"]
    assert r["samples"].shape[0] == r["images"].shape[0] == S and r["gx"].shape == r["logpi"].shape == (S,)
    np.testing.assert_array_equal(r["samples"][0], wr.mrdwt_TI2D(p["y"][0], p["h"], p["levels"]))
    np.testing.assert_array_equal(r["images"][-1], wr.mirdwt_TI2D(r["samples"][-1], p["h"], p["levels"]))
    assert np.all(r["gx"] > 0) and np.all(r["logpi"] < 0)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_synthesis_moments_kernels_keep_the_bars_of_the_plain_synthesis():
    rep = _report("wavelet.hip")
    for K in (2, 4, 6, 8):
        k = _find(rep, "wav_synthesis_moments_kernel", f"ILi{K}E")
        print(K, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, (K, k)
        assert k["LDS Size"] <= 80 * 1024 and k["Occupancy"] >= 2, (K, k)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_step_kernels_use_no_scratch():
    """The step kernel with (ILb1E) and without (ILb0E) the coefficient moments and wav_abs_sum_kernel live in
    csrc/wavelet_chain.hip, shared with the other two chain drivers; wav_myula_trace_kernel is this entry's own."""
    rep, chain = _report("wavelet_myula.hip"), _report("wavelet_chain.hip")
    for r, parts in ((chain, ("wav_step_kernel", "ILb1E")), (chain, ("wav_step_kernel", "ILb0E")),
                     (rep, ("wav_myula_trace_kernel",)), (chain, ("wav_abs_sum_kernel",))):
        k = _find(r, *parts)
        print(parts, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, (parts, k)
    for inst in ("ILb1E", "ILb0E"):
        assert _find(chain, "wav_step_kernel", inst)["Occupancy"] >= 4, inst   # streaming passes: enough waves to hide the loads
