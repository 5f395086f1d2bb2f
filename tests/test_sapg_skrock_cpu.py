"""CPU: the restated SAPG loop with an SK-ROCK kernel (tests/sapg_skrock_restatement.py) on the cases of
tests/sapg_skrock_cases.py, and the presence of the feature in the built library.

What the first two tests establish is what makes the bars of tests/test_gpu_sapg_skrock.py meaningful: (1) no prox call of any
case sits on the edge of the Chambolle stop rule, so a last-bit difference between two correct implementations cannot change
an iteration count; (2) the loop - chain and parameter updates together - amplifies a rounding-size perturbation of every prox
output by far less than the gap between rounding (1e-16) and the bars."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sapg_skrock_cases as ssc
import sapg_skrock_restatement as ssr
import skrock_tv_restatement as skr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACES = ("thetas", "sigmas", "ps", "logpi", "gx", "grads")


@pytest.mark.parametrize("name", ssc.NAMES)
def test_no_prox_call_sits_on_the_edge_of_the_stop_rule(name):
    """Every prox call gives the same iteration count at tol (1 - 1e-6), tol and tol (1 + 1e-6)."""
    q = ssc.problem(name)
    r = ssc.chain(name, alt_tols=(ssr.TOL * (1 - 1e-6), ssr.TOL * (1 + 1e-6)))
    calls = q["stages"] * q["noise"].shape[0]
    assert r["k"].shape == (calls,) and r["k_alt"].shape == (calls, 2)
    fired = r["err"] <= ssr.TOL
    margin = np.min(np.abs(r["err"][fired] / ssr.TOL - 1)) if np.any(fired) else float("nan")
    print(f"{name}: k = {r['k'].min()} .. {r['k'].max()}, the rule fired in {int(np.sum(fired))} of {calls} calls, "
          f"closest final err to tol: {margin:.2%}")
    np.testing.assert_array_equal(r["k_alt"][:, 0], r["k"])
    np.testing.assert_array_equal(r["k_alt"][:, 1], r["k"])
    assert np.all(r["k"] >= 1) and np.all(r["k"] <= ssc.CHAMBOLLEIT)
    np.testing.assert_array_equal(r["samples"], ssc.reference(name)["samples"])     # the extra runs change nothing


@pytest.mark.parametrize("name", ssc.NAMES)
def test_loop_amplifies_prox_rounding_far_less_than_the_bars_allow(name):
    """Every prox output perturbed by a relative 1e-15 (random signs): the last sample moves by at most 1e-10 max|X|, the
    traces by at most 1e-11 relative."""
    rng = np.random.default_rng(1)
    ref = ssc.reference(name)
    got = ssc.chain(name, perturb=lambda f, n: f * (1.0 + 1e-15 * rng.choice([-1.0, 1.0], size=f.shape)))
    np.testing.assert_array_equal(got["k"], ref["k"])
    xs = float(np.max(np.abs(ref["samples"][-1])))
    d = float(np.max(np.abs(got["samples"][-1] - ref["samples"][-1])))
    worst = 0.0
    for k in TRACES:
        nzr = ref[k] != 0
        np.testing.assert_array_equal(got[k] != 0, nzr, err_msg=k)
        worst = max(worst, float(np.max(np.abs(got[k][nzr] / ref[k][nzr] - 1))))
    print(f"{name}: last sample moved by {d / xs:.1e} max|X|, the traces by {worst:.1e} relative")
    assert 0 < d <= 1e-10 * xs
    assert worst <= 1e-11


@pytest.mark.parametrize("name", ssc.NAMES)
def test_restated_loop_is_finite_and_keeps_the_layout_of_the_myula_loop(name):
    q, r = ssc.problem(name), ssc.reference(name)
    S = ssc.SAMPLES
    assert r["samples"].shape == (S,) + q["setup"]["y"].shape
    for k in TRACES + ("logpi_wu", "samples"):
        assert np.all(np.isfinite(r[k])), k
    assert r["gx"][-1] == 0.0 and r["logpi_wu"][0] == 0.0 and not np.any(r["grads"][:, 0])      # the index quirks, kept
    assert r["thetas"][0] == q["op"]["th_init"] and r["sigmas"][0] == q["op"]["sigma_init"]
    assert float(np.max(np.abs(r["samples"]))) < 1e4                     # the data are 0..255 images


def test_at_frozen_parameters_the_samples_are_those_of_the_fixed_parameter_sampler():
    """c_theta = c_p = c_sigma = 0, sigma2 and the PSF parameters fixed at their true values, no warm-up: X(1..S) are the
    samples of skrock_tv_restatement.skrock_tv_chain on the same normals, bit for bit, and so are logpi and gx (shifted)."""
    name = "gauss-fixed-s3"
    q = ssc.problem(name)
    st, S = q["setup"], ssc.SAMPLES
    nz = q["noise"][:S - 1]
    got = ssc.chain(name, noise=nz, warmup=0, fix_sigma=True, c=dict(theta=0.0, p=(0.0, 0.0), sigma=0.0))
    s2 = st["sigma"] ** 2
    op = {"samples": S, "stages": q["stages"], "lambda": st["lam"], "delta": q["dt"], "eta": ssc.ETA, "chambolleit": ssc.CHAMBOLLEIT}
    ref = skr.skrock_tv_chain(st["y"], q["model"], st["p_true"], op, st["th_init"], s2, nz)
    assert np.all(got["thetas"] == st["th_init"]) and np.all(got["sigmas"] == s2)
    np.testing.assert_array_equal(got["samples"], ref["samples"])
    np.testing.assert_array_equal(got["k"], ref["k"])
    np.testing.assert_array_equal(got["gx"][:-1], ref["gx"][1:])
    np.testing.assert_allclose(got["logpi"], ref["logpi"], rtol=1e-14)   # ||y - A X||^2 against ||A X - y||^2: the same sum


# ---- the feature is there --------------------------------------------------------------------------------------------
def test_library_exports_sbtv_SAPG_skrock():
    import sbtv
    lib = sbtv.load_library()
    assert hasattr(lib, "sbtv_SAPG_skrock")
    from sbtv import _lib
    assert "sbtv_SAPG_skrock" in _lib.SIGNATURES and len(_lib.SIGNATURES["sbtv_SAPG_skrock"][1]) == 23


def test_python_entry_exists():
    import sbtv
    assert callable(sbtv.SAPG_skrock) and "SAPG_skrock" in sbtv.__all__


def test_step_struct_matches_the_header(tmp_path):
    from sbtv import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sbtv.h"\nint main(void){printf("%zu %zu %zu\\n",'
           'sizeof(sbtv_sapg_skrock_step), offsetof(sbtv_sapg_skrock_step, dt), offsetof(sbtv_sapg_skrock_step, eta));'
           'return 0;}\n')
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()
    T = _lib.sbtv_sapg_skrock_step
    assert [int(v) for v in out] == [C.sizeof(T), T.dt.offset, T.eta.offset]
