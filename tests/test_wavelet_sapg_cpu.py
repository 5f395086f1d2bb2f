"""CPU: the theta estimation of the wavelet-l1 path without a GPU.  The fused form the library runs (prox recomputed from X
and the lagging theta, residual taken one iteration late) against the literal loop of SALSA/SAPG_algorithm_1.m, both in
tests/wavelet_sapg_restatement.py; the behaviour of the chain the GPU cases rely on; the boundary (header, exports, ctypes
table, MATLAB shim); and the compiler's resource report of the new kernels (hipcc cross-compiles gfx950 without a GPU)."""
import os
import re

import numpy as np
import pytest

from test_kernel_resources import HIPCC, _find, _report

import wavelet_sapg_cases as wsc
import wavelet_sapg_restatement as wsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("thetas", "gXTrace", "logPiTraceX", "logPiTrace_WU", "mean_thetas", "tol_thetas")


def _same(got, ref, rtol):
    for (eb, r), (eb_ref, rr) in zip(got, ref):
        assert abs(eb - eb_ref) <= rtol * eb_ref
        for k in KEYS:
            assert (k in r) == (k in rr), k
            if k in rr:
                np.testing.assert_allclose(r[k], rr[k], rtol=rtol, atol=0, equal_nan=True, err_msg=k)
        assert np.max(np.abs(r["Xlast_sample"] - rr["Xlast_sample"])) <= rtol * np.max(np.abs(rr["Xlast_sample"]))


@pytest.mark.parametrize("name", ["a", "b"])
def test_fused_form_equals_the_literal_loop(name):
    p = wsc.problem(name)
    _same(wsc.run(wsr.sapg_wavelet_fused, p, wsc.noise(name)), wsc.reference(name), 1e-12)


def test_case_a_visits_both_bounds_and_the_traces_have_the_reference_shape():
    """theta jumps to max_th at ii = 2, falls to min_th right after and then decays smoothly: the clamp is exercised on both
    sides inside the 120 samples.  tol_thetas is NaN while mean(eta(burnIn:ii-1)) is over an empty range (2 <= ii <= burnIn)."""
    p = wsc.problem("a")
    op = p["op"]
    (eb, r), = wsc.reference("a")
    th = r["thetas"]
    hi, lo = np.flatnonzero(th == op["max_th"]), np.flatnonzero(np.abs(th - op["min_th"]) <= 1e-15)
    print(f"theta_EB {eb:.6g}; max_th at ii = {hi + 1}, min_th at ii = {lo + 1}, last theta {th[-1]:.4g}")
    assert hi.size and lo.size and hi[0] < lo[0] < op["samples"] - 1
    assert th[0] == op["th_init"] and np.all((th >= op["min_th"] * (1 - 1e-15)) & (th <= op["max_th"]))
    assert r["mean_thetas"].shape == (op["samples"] - op["burnIn"],) and r["mean_thetas"][-1] == eb == r["mean_theta"]
    assert r["logPiTrace_WU"].shape == (op["warmup"],) and r["logPiTrace_WU"][0] == 0 and np.all(r["logPiTrace_WU"][1:] != 0)
    assert r["tol_thetas"][0] == 0 and np.all(np.isnan(r["tol_thetas"][1:op["burnIn"]]))
    assert np.all(np.isfinite(r["tol_thetas"][op["burnIn"]:]))
    assert r["gXTrace"][-1] == 0 and np.all(r["gXTrace"][:-1] > 0)


def test_warmup_0_and_1_give_identical_traces():
    p = wsc.problem("b")
    nz = wsc.noise("b")[:8]
    y, out = p["y"][0], []
    for warmup in (0, 1):
        op = dict(p["op"], samples=9, burnIn=3, warmup=warmup)
        out.append([fn(y, p["H"], p["h"], p["levels"], op, nz[:, 0]) for fn in (wsr.sapg_wavelet_literal, wsr.sapg_wavelet_fused)])
    for (eb0, r0), (eb1, r1) in zip(out[0], out[1]):
        assert eb0 == eb1
        for k in KEYS:
            if k != "logPiTrace_WU":
                np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)
        np.testing.assert_array_equal(r0["Xlast_sample"], r1["Xlast_sample"])
        assert "logPiTrace_WU" not in r0 and r1["logPiTrace_WU"].tolist() == [0.0]


def test_entry_point_declared_exported_bound_and_shimmed():
    import ctypes as C
    import sbtv
    from sbtv import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbtv.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+sbtv_SAPG_wavelet\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "sbtv_SAPG_wavelet is not declared in include/sbtv.h"
    assert len(m.group(1).split(",")) == 22 == len(_lib.SIGNATURES["sbtv_SAPG_wavelet"][1])
    assert hasattr(sbtv.load_library(), "sbtv_SAPG_wavelet")
    assert callable(sbtv.SAPG_wavelet) and "SAPG_wavelet" in sbtv.__all__
    s = re.search(r"typedef\s+struct\s+sbtv_sapg_wavelet_opts\s*\{(.*?)\}", text, flags=re.S).group(1)
    names = [re.sub(r"\W", "", n) for d in s.split(";") if d.strip() for n in re.sub(r"^\s*(unsigned long long|\w+)\s", "", d.strip()).split(",")]
    assert names == [n.rstrip("_") for n, _ in _lib.sbtv_sapg_wavelet_opts._fields_]
    assert C.sizeof(_lib.sbtv_sapg_wavelet_opts) == 4 * 4 + 8 * 8 + 8 + 8          # 3 ints + pad, 8 doubles, seed, int + pad
    shim = open(os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd", "matlab", "sbtv_sapg_wavelet.m")).read()
    assert "'sbtv_SAPG_wavelet'" in shim and "libstruct('sbtv_sapg_wavelet_opts')" in shim


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_chain_kernels_use_no_scratch():
    """wav_sapg_update_kernel, and the kernels the three chain drivers share (csrc/wavelet_chain.hip): the step kernel this
    entry launches is the instantiation without moments."""
    rep, chain = _report("wavelet_sapg.hip"), _report("wavelet_chain.hip")
    for r, parts in ((chain, ("wav_step_kernel", "ILb0E")), (rep, ("wav_sapg_update_kernel",)), (chain, ("wav_abs_sum_kernel",))):
        k = _find(r, *parts)
        print(parts, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, (parts, k)
    assert _find(chain, "wav_step_kernel", "ILb0E")["Occupancy"] >= 4   # a streaming pass: enough waves to hide the loads
