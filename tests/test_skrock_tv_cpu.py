"""CPU: the restated SK-ROCK chain on the TV posterior (tests/skrock_tv_restatement.py) on the cases of
tests/skrock_tv_cases.py, and the presence of the feature in the built library.

What the first two tests establish is what makes the 1e-9 bar of tests/test_gpu_skrock_tv.py meaningful: (1) no prox call of
any case sits on the edge of the Chambolle stop rule, so a last-bit difference between two correct implementations cannot
change an iteration count; (2) the chain amplifies a rounding-size perturbation of every prox output by far less than the gap
between rounding (1e-16) and the bar."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import skrock_tv_cases as skc
import skrock_tv_restatement as skr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", skc.NAMES)
def test_no_prox_call_sits_on_the_edge_of_the_stop_rule(name):
    """Every prox call gives the same iteration count at tol (1 - 1e-6), tol and tol (1 + 1e-6); the rule does fire (k < 25
    occurs), which is wanted."""
    op = skc.problem(name)["op"]
    r = skc.chain(name, alt_tols=(skr.TOL * (1 - 1e-6), skr.TOL * (1 + 1e-6)))
    calls = op["stages"] * (op["samples"] - 1)
    assert r["k"].shape == (calls,) and r["k_alt"].shape == (calls, 2)
    fired = r["err"] <= skr.TOL
    margin = np.min(np.abs(r["err"][fired] / skr.TOL - 1)) if np.any(fired) else float("nan")
    print(f"{name}: k = {r['k'].min()} .. {r['k'].max()}, the rule fired in {int(np.sum(fired))} of {calls} calls, "
          f"closest final err to tol: {margin:.2%}")
    np.testing.assert_array_equal(r["k_alt"][:, 0], r["k"])
    np.testing.assert_array_equal(r["k_alt"][:, 1], r["k"])
    assert np.all(r["k"] >= 1) and np.all(r["k"] <= op["chambolleit"])
    np.testing.assert_array_equal(r["samples"], skc.reference(name)["samples"])     # the extra runs change nothing


def test_the_stop_rule_fires_somewhere():
    assert any(np.any(skc.reference(n)["k"] < skc.CHAMBOLLEIT) for n in skc.NAMES)


@pytest.mark.parametrize("name", skc.NAMES)
def test_chain_amplifies_prox_rounding_by_less_than_1e3(name):
    """Every prox output perturbed by a relative 1e-15 (random signs): the last sample moves by less than 1e-12 max|X|."""
    rng = np.random.default_rng(1)
    ref = skc.reference(name)
    got = skc.chain(name, perturb=lambda f, n: f * (1.0 + 1e-15 * rng.choice([-1.0, 1.0], size=f.shape)))
    np.testing.assert_array_equal(got["k"], ref["k"])
    xs = float(np.max(np.abs(ref["samples"][-1])))
    d = float(np.max(np.abs(got["samples"][-1] - ref["samples"][-1])))
    print(f"{name}: last sample moved by {d / xs:.1e} max|X|")
    assert 0 < d < 1e-12 * xs


@pytest.mark.parametrize("name", skc.NAMES)
def test_restated_chain_is_finite_and_keeps_its_start(name):
    q, r = skc.problem(name), skc.reference(name)
    S = q["op"]["samples"]
    assert r["samples"].shape == (S,) + q["y"].shape
    np.testing.assert_array_equal(r["samples"][0], q["y"])
    assert np.all(np.isfinite(r["samples"])) and np.all(np.isfinite(r["gx"])) and np.all(np.isfinite(r["logpi"]))
    assert float(np.max(np.abs(r["samples"]))) < 1e4                     # the data are 0..255 images


# ---- the feature is there --------------------------------------------------------------------------------------------
def test_library_exports_sbtv_skrock():
    import sbtv
    lib = sbtv.load_library()
    assert hasattr(lib, "sbtv_skrock")
    from sbtv import _lib
    assert "sbtv_skrock" in _lib.SIGNATURES and len(_lib.SIGNATURES["sbtv_skrock"][1]) == 20


def test_python_entry_exists():
    import sbtv
    assert callable(sbtv.skrock) and "skrock" in sbtv.__all__


def test_opts_struct_matches_the_header(tmp_path):
    from sbtv import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sbtv.h"\nint main(void){printf("%zu %zu %zu %zu\\n",'
           'sizeof(sbtv_skrock_opts), offsetof(sbtv_skrock_opts, lambda), offsetof(sbtv_skrock_opts, seed),'
           'offsetof(sbtv_skrock_opts, chain_offset));return 0;}\n')
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()
    T = _lib.sbtv_skrock_opts
    assert [int(v) for v in out] == [C.sizeof(T), T.lambda_.offset, T.seed.offset, T.chain_offset.offset]
