"""CPU: the geometry cases of the TV-model samplers (tests/tv_sampler_geometry_cases.py) reach every class they are there for,
and the restated chains on them give the 1e-9 bars of tests/test_gpu_tv_sampler_sweep.py their meaning, as
tests/test_skrock_tv_cpu.py, tests/test_sapg_skrock_cpu.py and tests/test_masked_sapg_cpu.py do for the drivers' own cases:
(1) no prox call of any case sits on the edge of the Chambolle stop rule, so a last-bit difference between two correct
implementations cannot change an iteration count; (2) a chain amplifies a rounding-size perturbation of every prox output by far
less than the gap between rounding (1e-16) and the bars; (3) every chain is finite and starts where it should.  Every test
prints its figures."""
import numpy as np
import pytest

import fft_plan_cases as fpc
import masked_sapg_restatement as msr
import tv_sampler_geometry_cases as gc

TOL = msr.TOL
IDS = [f"{d}-{t}" for d, t in gc.ALL]


# ---- the tables reach what they are there for ---------------------------------------------------------------------------
@pytest.mark.parametrize("driver", gc.DRIVERS)
def test_table_reaches_every_class(driver):
    cov = gc.assert_reaches(driver)
    for c in sorted(cov):
        print(f"{driver}: {c}: {', '.join(cov[c])}")
    # and the FFT-plan classes are those fft_plan_cases names for these shapes, not assumed ones
    shapes = [gc.shape(driver, t) for t in gc.TABLES[driver]]
    fcov = fpc.assert_coverage(shapes, fpc.model_plan, {("wave", (512, 1024)), ("partial wave", True), ("chirp", "L_M=4096"),
                                                        ("chirp", "L_N=1024"), ("cols", 7), ("cols", 5), ("rows", (6, 8)),
                                                        ("rows", (8, 2))})
    print(f"{driver}: plan classes: " + ", ".join(f"{k}={v}" for k, v in sorted(fcov, key=str)))


def test_the_named_shapes_are_what_the_issue_says_they_are():
    """Every figure the case table's docstring quotes, from the model."""
    w, s = gc.geometry(1024, 1024), gc.geometry(1090, 481)
    grid = gc.EW_MAX_BLOCKS * gc.EW_LANES
    assert w["plan"]["wave"] and w["plan_class"] == "wave" and w["plan"]["rows_kind"] == "pipelined" and w["plan"]["tv_ok"]
    assert w["ew_blocks"] == 1024 and w["pairs"] == 2 * grid and w["lanes_on_trip_2"] == grid and w["max_trips"] == 2
    assert w["ntv"] == 1024 and gc.trips(w["ntv"]) == 4 and gc.trips(w["nblk"]) == 4 and w["nrb"] == 128
    assert s["plan"]["generic"] and not s["plan"]["tv_ok"] and s["pairs"] == grid + 1 and 1090 * 481 == 2 * (1024 * 256 + 1)
    assert s["lanes_on_trip_2"] == 1 and s["max_trips"] == 2 and s["ntv"] == 9 * 31 == 279 > gc.TOTAL_LANES
    assert gc.trips(s["ntv"]) == 2 and gc.trips(s["nblk"]) == 4
    for M, N in ((256, 64), (64, 256)):
        g = gc.geometry(M, N)
        assert g["plan_class"] == "workgroup" and g["plan"]["tv_ok"] and g["max_trips"] == 1 and g["ew_blocks"] == 32
    p = gc.geometry(16, 16)
    assert p["plan_class"] == "workgroup" and p["plan"]["rows_threads"] < 64 and p["pairs"] == 128
    o = gc.geometry(25, 40)
    assert o["plan_class"] == "chirp" and o["scalar_tv"] and o["pairs"] == 500
    t = gc.geometry(8, 8)
    assert t["plan_class"] == "chirp" and t["pairs"] == 32 < 64 and t["ew_blocks"] == 1
    # what the drivers' own tables reach: none of the above (which is why this table exists)
    for M, N in ((32, 32), (24, 40), (8, 6)):
        g = gc.geometry(M, N)
        assert g["max_trips"] == 1 and max(gc.trips(g[k]) for k in ("ntv", "nrb", "nblk")) == 1 and not g["scalar_tv"]
        assert g["plan_class"] != "wave" and (g["plan_class"] == "chirp" or M == N)
    assert gc.geometry(32, 32)["plan"]["rows_threads"] == 32 > p["plan"]["rows_threads"] == 16     # a quarter of a wave


def test_every_case_has_an_even_pixel_count_and_a_free_psf_parameter():
    for d, t in gc.ALL:
        M, N = gc.shape(d, t)
        assert M * N % 2 == 0 and min(M, N) >= 7, (d, t)
        if d.startswith("SAPG"):
            assert not all(gc.problem(d, t)["kw"]["fix"]), (d, t)        # the spectra are rebuilt once at that size
    for d in ("skrock", "SAPG_skrock"):                                  # both parities at the grid-stride classes
        assert {gc.stages(d, "wave") % 2, gc.stages(d, "seam") % 2} == {0, 1}


# ---- (1) the stop rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("driver,tag", gc.ALL, ids=IDS)
def test_no_prox_call_sits_on_the_edge_of_the_stop_rule(driver, tag):
    """Every prox call gives the same iteration count at tol (1 - 1e-6), tol and tol (1 + 1e-6)."""
    r = gc.chain(driver, tag, alt_tols=(TOL * (1 - 1e-6), TOL * (1 + 1e-6)))
    ref = gc.reference(driver, tag)
    calls = gc.prox_calls(driver, tag)
    assert r["k"].shape == (calls,) and r["k_alt"].shape == (calls, 2)
    fired = r["err"] <= TOL
    margin = np.min(np.abs(r["err"] / TOL - 1))
    print(f"{driver} {tag}: k = {r['k'].min()} .. {r['k'].max()}, the rule fired in {int(np.sum(fired))} of {calls} calls, "
          f"final err {r['err'].min():.2e} .. {r['err'].max():.2e}, closest to tol: {margin:.2%}")
    np.testing.assert_array_equal(r["k_alt"][:, 0], r["k"])
    np.testing.assert_array_equal(r["k_alt"][:, 1], r["k"])
    cit = gc.problem(driver, tag)["chambolleit"] if driver == "myula_masked" else (
        gc.problem(driver, tag)["op"]["chambolleit"])
    assert np.all(r["k"] >= 1) and np.all(r["k"] <= cit)
    np.testing.assert_array_equal(r["samples"], ref["samples"])          # the extra runs change nothing
    np.testing.assert_array_equal(r["k"], ref["k"])


def test_the_stop_rule_fires_at_the_small_shapes_and_not_at_the_large_ones():
    for d in gc.DRIVERS:
        small = [t for t in gc.TABLES[d] if max(gc.shape(d, t)) <= 40]
        big = [t for t in gc.TABLES[d] if max(gc.shape(d, t)) >= 1024]
        assert any(np.any(gc.reference(d, t)["err"] <= TOL) for t in small), d
        for t in big:                                                    # far from firing: the count is not what they test
            assert np.all(gc.reference(d, t)["err"] > 5 * TOL) and np.all(gc.reference(d, t)["k"] == gc.BIG_CHAMBOLLEIT), (d, t)


# ---- (2) amplification ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("driver,tag", gc.ALL, ids=IDS)
def test_chain_amplifies_prox_rounding_by_less_than_1e3(driver, tag):
    """Every prox output perturbed by a relative 1e-15 (random signs): the last sample moves by less than 1e-12 max|X|."""
    rng = np.random.default_rng(1)
    ref = gc.reference(driver, tag)
    moved = []

    def perturb(f, n):
        g = f * (1.0 + 1e-15 * rng.choice([-1.0, 1.0], size=f.shape))
        moved.append(np.count_nonzero(g != f))
        return g

    got = gc.chain(driver, tag, perturb=perturb)
    np.testing.assert_array_equal(got["k"], ref["k"])
    assert len(moved) == gc.prox_calls(driver, tag) and min(moved) > 0.9 * ref["samples"][0].size    # every output was moved
    a, b = gc.last_sample(driver, got), gc.last_sample(driver, ref)
    xs, d = float(np.max(np.abs(b))), float(np.max(np.abs(a - b)))
    print(f"{driver} {tag}: last sample moved by {d / xs:.1e} max|X|")
    assert d < 1e-12 * xs                # (at 8 x 8 a step may round the whole perturbation away: d = 0 is no failure)


# ---- (3) finite, and the start ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("driver,tag", gc.ALL, ids=IDS)
def test_restated_chain_is_finite_and_keeps_its_start(driver, tag):
    q, r = gc.problem(driver, tag), gc.reference(driver, tag)
    M, N = gc.shape(driver, tag)
    y = q["y"] if driver in ("skrock", "myula_masked") else q["setup"]["y"]
    S = {"skrock": gc.STEPS + 1, "myula_masked": gc.MYULA_SAMPLES - 1}.get(driver, gc.SAPG["samples"])
    assert r["samples"].shape == (S, M, N) and y.shape == (M, N)
    assert np.all(np.isfinite(r["samples"])) and float(np.max(np.abs(r["samples"]))) < 1e4      # the data are 0..255 images
    if driver.startswith("SAPG"):
        for k in ("thetas", "sigmas", "ps", "logpi", "logpi_wu", "gx", "grads"):
            assert np.all(np.isfinite(r[k])), k
        assert r["thetas"][0] == q["op"]["th_init"] and r["sigmas"][0] == q["op"]["sigma_init"]
        assert r["gx"][-1] == 0.0 and r["logpi_wu"][0] == 0.0 and not np.any(r["grads"][:, 0])  # the index quirks, kept
        assert np.all(r["grads"][:, 1:] != 0) and len(set(r["thetas"].tolist())) == S           # every gradient is live
        assert np.any(r["ps"][:, 1] != r["ps"][:, 0])                                           # a PSF parameter has moved
        assert np.any(r["samples"][0] != y)                                                     # the warm-up has moved X
        assert q["noise"].shape == (gc.SAPG["warmup"] - 1 + S - 1, M, N)
    else:
        np.testing.assert_array_equal(r["samples"][0], y)
        if driver == "skrock":
            assert np.all(np.isfinite(r["gx"])) and np.all(np.isfinite(r["logpi"])) and q["noise"].shape == (gc.STEPS, M, N)
    if "mask" in q:
        m = q["mask"]
        assert m.shape == (M, N) and 0 < msr.n_obs(m) < m.size
