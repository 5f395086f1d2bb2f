"""GPU parity of the Chambolle kernels at the image sizes where their index arithmetic decides: tile seams, image edges,
the `interior` classification, the tile table and the stagger.  Whole-image comparison with the oracle
(utils/chambolle_prox_TV_stop.m:120-149) at the bars of test_gpu_tv.py / test_gpu_tv_large.py: k equal, err to
rel 1e-12, px, py to rtol = atol = 1e-12, f to rtol 1e-12, atol 1e-10.

The sizes are DERIVED from the geometry the library reports (`Context.prox_geometry`) by tests/tv_geometry_cases.py,
whose coverage conditions are asserted on that geometry before anything is launched: change the core width and the
sweep moves with it, empty a class and the test fails instead of thinning.

The environment hooks are read once per process, so each kernel runs in a child process (this file, run as a script)
that computes every shape of its sweep into one .npz; the parent computes the oracle and compares.

Does the sweep bite?  The library was built with one change at a time, each a change of a value or a value select only
(no address, predicate or loop bound), and the TV modules were run once per mutant:

    mutant (both fused kernels at once)              | test_gpu_tv.py + test_gpu_tv_large.py | this module (10 tests)
    -------------------------------------------------+---------------------------------------+---------------------------------
    1 interior row test `<= M - 1` -> `<= M`         | none of 45 fails                      | 3 fail: sweep[rows1],
                                                     |                                       | sweep[exact_rows1], solver[rows1]
    2 interior column test `<= N - 1` -> `<= N`      | none                                  | 5 fail: all sweeps but [single],
                                                     |                                       | plan-chosen kernel at edge sizes
    3 last-row select of upx, `< M - 1` -> `< M`     | 31 fail (caught before this sweep)    | 8 fail (all but [single], 8-byte)
    4 f epilogue: seam column pyl0 taken as zero     | 29 fail (caught before this sweep)    | 8 fail (all but [single], 8-byte)
    5 ecore without `gj < N` (non-interior body)     | none                                  | 4 fail: the four fused sweeps,
                                                     |                                       | `warm_any` cases only

Mutants 1 and 2 show at the d = 0 shapes only (rows 164 for the 64-row kernel, columns 47 for both), in the cases that
run a launch of the maximum step count from non-zero duals (warm, warm_any, cold25): a cold launch starts from p = 0, where
the wrong divergence of the last row / column is still right, and the error needs one step more to reach the core.
Mutant 1 cannot be observed on the 128-row kernel: its halo below the core is 6 rows for at most 5 steps per launch, so
whatever the last region row computes never reaches the core - `<= M` would be a correct test there as long as that
holds (sweep[rows2] at 238 rows passes with it).  Mutant 5 is invisible from a cold start and from the oracle's duals
(py is zero in the last column, so a column beyond the image has u = 0); only the arbitrary duals show it.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import synth_image

import tv_geometry_cases as tg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=1e-12, atol=1e-12)
LAM = 8.0
KMAX = 15                                   # MaxIter of the stop-rule cases
FORCE_ROWS2 = {"SBTV_FUSED_VARIANT": "4,8,4"}
ENVS = {
    "rows1": {},                                              # the plans' own choice at these sizes: 64-row tiles
    "rows2": FORCE_ROWS2,                                     # the 128-row tiles large images get, forced
    "single": {"SBTV_SINGLE_STEP": "1"},                      # one-iteration kernels with an even M
    "exact_rows1": {"SBTV_EXACT": "1"},                       # IEEE arithmetic on the interior pairs
    "exact_rows2": dict(FORCE_ROWS2, SBTV_EXACT="1"),
}


def _image(M, N, seed):
    return synth_image(M, N, seed) + np.random.default_rng(seed).standard_normal((M, N))


def _seed(M, N):
    return 7 + M * 5 + N


def _any_duals(M, N):
    """Dual variables of modulus <= 1 without structure: the last row of px and the last column of py are NOT zero.
    DivergenceIm ends with -p(end) (:152-159, quirk Q3), which is zero on every iterate of a cold start; only a start
    like this one makes that term, and whatever a kernel computes beyond the image from it, visible."""
    rng = np.random.default_rng(M * 7919 + N)
    a, r = rng.uniform(0, 2 * np.pi, (M, N)), rng.uniform(0.2, 1.0, (M, N))
    return r * np.cos(a), r * np.sin(a)


def _cases(S):
    """(name, maxiter, start) of every fused-kernel shape; S = most iterations of one launch."""
    return [("cold1", 1, None), ("cold%d" % S, S, None), ("cold%d" % (S + 2), S + 2, None), ("cold25", 25, None),
            ("warm", S, "warm"), ("warm_any", S, "any")]


# ---------------------------------------------------------------------------------------------------------------------
# child process: run every job of a spec, store the results
# ---------------------------------------------------------------------------------------------------------------------
def _child(spec_path, in_path, out_path):
    import sbtv
    with open(spec_path) as fh:
        spec = json.load(fh)
    inp = np.load(in_path)
    ctx = sbtv.default_context(0)
    res = {}

    def put(key, got):
        f, px, py, k, err = got
        res[key + ".f"], res[key + ".px"], res[key + ".py"] = sbtv.to_host(f), sbtv.to_host(px), sbtv.to_host(py)
        res[key + ".k"], res[key + ".err"] = np.asarray(k), np.asarray(err)

    for M, N, corner in spec["prox"]:
        key = "%dx%d" % (M, N)
        v = ctx.prox_variant(M, N)
        res[key + ".rpl"], res[key + ".fused"] = np.array(v["rows_per_lane"]), np.array(int(v["fused"]))
        g = _image(M, N, _seed(M, N))
        gd = sbtv.to_device(g)
        for name, K, start in _cases(spec["S"]):
            args = [gd, "lambda", LAM, "maxiter", K]
            if start:
                args += ["dualvars", (sbtv.to_device(inp["%s.%s.px" % (key, start)]), sbtv.to_device(inp["%s.%s.py" % (key, start)]))]
            put(key + "." + name, sbtv.chambolle_prox_TV_stop(*args, return_info=True))
        if corner:
            gb = np.stack([_image(M, N, _seed(M, N) + 1 + b) for b in range(3)])
            put(key + ".batch3", sbtv.chambolle_prox_TV_stop(sbtv.to_device(gb), "lambda", np.array(spec["lam3"]), "maxiter",
                                                             spec["S"] + 2, return_info=True))
            for kstop in spec["kstops"]:
                put(key + ".stop%d" % kstop, sbtv.chambolle_prox_TV_stop(
                    gd, "lambda", LAM, "maxiter", KMAX, "tol", float(inp["%s.tol%d" % (key, kstop)]), return_info=True))
    for M, N, square in spec["solvers"]:
        key = "%dx%d" % (M, N)
        x = synth_image(M, N, 9)
        if square:
            A = sbtv.BlurOperator(sbtv.Gaussian_psf(7, 0.4, 0.3))
            theta, mu = 0.03, 0.003
            out = sbtv.SALSA_v2(inp[key + ".sq.y"], A, theta * float(inp[key + ".sq.s2"]), "MU", mu, "AT", A.T, "LS", A.LS(mu),
                                "True_x", x, "ToleranceA", 1e-5, "MAXITERA", 60, "TVINITIALIZATION", 1, "TViters", 10,
                                "VERBOSE", 0)
            res[key + ".sq.x"], res[key + ".sq.obj"], res[key + ".sq.dist"], res[key + ".sq.mses"] = out[0], out[3], out[4], out[6]
            continue
        A = sbtv.BlurOperator(sbtv.Gaussian_psf(7, 0.4, 0.3))
        mu = 0.003
        for sp in (1, 3, 0, 2):
            out = sbtv.SALSA_v2(inp[key + ".salsa.y"], A, float(inp[key + ".salsa.tau"]), "MU", mu, "AT", A.T, "LS", A.LS(mu),
                                "True_x", x, "ToleranceA", -1.0, "MAXITERA", 6, "TVINITIALIZATION", 1, "TViters", 10,
                                "SPECULATE", sp)
            res["%s.salsa%d.x" % (key, sp)], res["%s.salsa%d.obj" % (key, sp)] = out[0], out[3]
        A = sbtv.BlurOperator(inp[key + ".fista.taps"])
        xg, obj, times, mses = sbtv.my_fista(inp[key + ".fista.y"], A, A.T, float(inp[key + ".fista.tau"]), 1.0, sbtv.TVnorm,
                                             sbtv.Psi_TV(25), 1, 1e-4, 25, x)
        res[key + ".fista.x"], res[key + ".fista.obj"] = xg, obj
    np.savez(out_path, **res)


# ---------------------------------------------------------------------------------------------------------------------
# parent: geometry, oracle, comparison
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def geoms(ctx):
    """The geometry of the two fused kernels as the library reports it (64 x 64 takes the one-row-per-lane kernel,
    2048 x 2048 the two-rows-per-lane one), with the coverage of the shapes derived from it asserted."""
    g1, g2 = ctx.prox_geometry(64, 64), ctx.prox_geometry(2048, 2048)
    assert g1["rows_per_lane"] == 1 and g2["rows_per_lane"] == 2, (g1, g2)
    for g in (g1, g2):
        assert g["region_rows"] == g["halo_top"] + g["core_rows"] + g["halo_bottom"], g
        assert g["region_cols"] == g["halo_left"] + g["core_cols"] + g["halo_right"], g
        tg.assert_coverage(g, tg.fused_shapes(g))
    return {"rows1": g1, "rows2": g2}


def _oracle(g, lam, K, tol=None, start=None):
    import sbtv_oracle as o
    kw = {} if tol is None else dict(tol=tol)
    return o.chambolle_prox_TV_stop(g, lam=lam, maxiter=K, dualvars=start, return_info=True, **kw)


def _stop_tols(g, kstops):
    """Tolerances between two consecutive oracle errors, so that the rule fires at exactly kstop."""
    errs, p = [], None
    for _ in range(KMAX):
        _, pxo, pyo, _, e = _oracle(g, LAM, 1, tol=0.0, start=p)
        p = (pxo, pyo)
        errs.append(e)
    assert all(a > b for a, b in zip(errs, errs[1:])), "test assumes a decreasing err sequence"
    return {k: 0.5 * (errs[k - 1] + errs[k - 2]) for k in kstops}


def _solver_inputs(M, N, square, inp):
    import sbtv_oracle as o
    key = "%dx%d" % (M, N)
    x = synth_image(M, N, 9)
    st = o.demo_setup("gaussian", x, np.random.default_rng(1).standard_normal((M, N)), evMax=1.0)
    if square:
        inp[key + ".sq.y"], inp[key + ".sq.s2"] = st["y"], np.array(st["sigma"] ** 2)
        return
    inp[key + ".salsa.y"], inp[key + ".salsa.tau"] = st["y"], np.array(0.03 * st["sigma"] ** 2)
    st = o.demo_setup("moffat", x, np.random.default_rng(3).standard_normal((M, N)), evMax=1.0)
    inp[key + ".fista.y"], inp[key + ".fista.tau"] = st["y"], np.array(0.03 * st["sigma"] ** 2)
    inp[key + ".fista.taps"] = st["model"].taps(*st["p_true"])


def _plan(name, geoms):
    """(spec, expected kernel) of one child."""
    kernel = "rows2" if name.endswith("rows2") else "rows1"
    geom = geoms[kernel]
    corners = [s[:2] for s in tg.corner_shapes(geom)]
    solvers = []
    if name.startswith("exact"):
        prox = [(M, N, False) for M, N in corners]
    elif name == "single":
        prox = [(M, N, False) for M, N, _ in tg.single_step_shapes(geom)[1]]
    else:
        prox = [(M, N, (M, N) in corners) for M, N, _ in tg.fused_shapes(geom)]
        if name == "rows1":                                   # odd M takes the one-iteration kernels by itself
            prox += [(M, N, False) for M, N, _ in tg.single_step_shapes(geom)[0]]
        solvers = [corners[0] + (False,), corners[1] + (False,), corners[3] + (False,), tg.square_shape(geom)[:2] + (True,)]
    return dict(prox=prox, solvers=solvers, S=geom["max_steps"], lam3=[6.0, 8.0, 11.0], kstops=[3, 5]), kernel


_children = {}          # name -> loaded .npz, or an Exception: no further child is started after a failed one


@pytest.fixture(scope="module")
def child(geoms, tmp_path_factory):
    def run(name):
        if name in _children:
            if isinstance(_children[name], Exception):
                raise _children[name]
            return _children[name]
        bad = [n for n, v in _children.items() if isinstance(v, Exception)]
        assert not bad, "child %s failed: no further child process is started" % bad
        spec, _ = _plan(name, geoms)
        inp = {}
        for M, N, corner in spec["prox"]:
            key = "%dx%d" % (M, N)
            g = _image(M, N, _seed(M, N))
            warm = _oracle(g, LAM, spec["S"])
            inp[key + ".warm.px"], inp[key + ".warm.py"] = warm[1], warm[2]
            inp[key + ".any.px"], inp[key + ".any.py"] = _any_duals(M, N)
            if corner:
                for k, t in _stop_tols(g, spec["kstops"]).items():
                    inp["%s.tol%d" % (key, k)] = np.array(t)
        for M, N, square in spec["solvers"]:
            _solver_inputs(M, N, square, inp)
        d = tmp_path_factory.mktemp("tvgeom_" + name)
        sp, ip, op = str(d / "spec.json"), str(d / "in.npz"), str(d / "out.npz")
        with open(sp, "w") as fh:
            json.dump(spec, fh)
        np.savez(ip, **inp)
        e = dict(os.environ)
        for k in ("SBTV_FUSED_VARIANT", "SBTV_SINGLE_STEP", "SBTV_EXACT"):
            e.pop(k, None)
        e.update(ENVS[name])
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", sp, ip, op], check=True, env=e, timeout=900)
            _children[name] = (np.load(op), inp)
        except Exception as ex:                               # non-zero exit or time limit
            _children[name] = ex
            raise
        return _children[name]
    return run


def _check(bad, key, got, want, b=None):
    """Compare one prox result with the oracle's at the project's bars; a miss is recorded, not raised, so that one
    report names every shape and case that misses."""
    f, px, py, k, err = [got[key + s] for s in (".f", ".px", ".py", ".k", ".err")]
    if b is not None:
        f, px, py, k, err = f[b], px[b], py[b], k[b:b + 1], err[b:b + 1]
        key = "%s[%d]" % (key, b)
    fo, pxo, pyo, ko, erro = want
    try:
        assert int(np.ravel(k)[0]) == ko, "k %d != %d" % (int(np.ravel(k)[0]), ko)
        assert float(np.ravel(err)[0]) == pytest.approx(erro, rel=1e-12), "err %r != %r" % (float(np.ravel(err)[0]), erro)
        np.testing.assert_allclose(px, pxo, err_msg="px", **TOL)
        np.testing.assert_allclose(py, pyo, err_msg="py", **TOL)
        np.testing.assert_allclose(f, fo, rtol=1e-12, atol=1e-10, err_msg="f")
    except AssertionError as e:
        msg = " ".join(str(e).split())
        bad.append("%s: %s" % (key, msg[:160]))


@pytest.mark.parametrize("name", list(ENVS))
def test_sweep_matches_oracle(child, geoms, name):
    """Every shape of the sweep of one kernel: cold 1 / S / S + 2 / 25 iterations, warm starts from the oracle's duals
    and from arbitrary duals; on the corner shapes a batch of three and the stop rule firing at k = 3 (redo pass) and
    k = 5 (finish-only pass: f from a launch of zero steps) of MaxIter = 15."""
    got, inp = child(name)
    spec, kernel = _plan(name, geoms)
    bad = []
    for M, N, corner in spec["prox"]:
        key = "%dx%d" % (M, N)
        fused = M % 2 == 0 and name != "single"
        assert int(got[key + ".fused"]) == int(fused), (key, name)
        if fused:
            assert int(got[key + ".rpl"]) == (2 if kernel == "rows2" else 1), (key, name)
        g = _image(M, N, _seed(M, N))
        for cname, K, start in _cases(spec["S"]):
            duals = (inp["%s.%s.px" % (key, start)], inp["%s.%s.py" % (key, start)]) if start else None
            _check(bad, key + "." + cname, got, _oracle(g, LAM, K, start=duals))
        if corner:
            for b in range(3):
                _check(bad, key + ".batch3", got, _oracle(_image(M, N, _seed(M, N) + 1 + b), spec["lam3"][b], spec["S"] + 2), b)
            for kstop in spec["kstops"]:
                want = _oracle(g, LAM, KMAX, tol=float(inp["%s.tol%d" % (key, kstop)]))
                assert want[3] == kstop
                _check(bad, key + ".stop%d" % kstop, got, want)
    assert not bad, "%d of the cases miss the bars:\n%s" % (len(bad), "\n".join(bad[:60]))


@pytest.mark.parametrize("name", ["rows1", "rows2"])
def test_solver_launch_forms_at_corner_shapes(child, geoms, name):
    """The launch forms only solver loops use (optimistic ping-pong launches with the subset error sum, multi-buffer
    launches of a cold prox, the collector riding in the first launch) at three corner shapes: SALSA_v2 gives the same
    bits whatever SPECULATE says, my_fista matches the oracle's (bars of test_fista_and_sapg_any_size_match_oracle), and
    on one square shape SALSA_v2 matches salsa_from_estimates (bars of test_salsa_any_size_matches_oracle)."""
    import sbtv_oracle as o
    got, inp = child(name)
    spec, _ = _plan(name, geoms)
    for M, N, square in spec["solvers"]:
        key = "%dx%d" % (M, N)
        x = synth_image(M, N, 9)
        if square:
            st = o.demo_setup("gaussian", x, np.random.default_rng(1).standard_normal((M, N)), evMax=1.0)
            ref = o.salsa_from_estimates(st, 0.03, st["p_true"], st["sigma"] ** 2, outeriters=60)
            assert len(got[key + ".sq.obj"]) == len(ref["objective"]), "different stopping iteration"
            np.testing.assert_allclose(got[key + ".sq.obj"], ref["objective"], rtol=1e-9)
            np.testing.assert_allclose(got[key + ".sq.mses"], ref["mses"], rtol=1e-9)
            np.testing.assert_allclose(got[key + ".sq.dist"], ref["distance"], rtol=1e-7)
            assert np.max(np.abs(got[key + ".sq.x"] - ref["x"])) < 1e-6
            assert abs(o.PSNR(x, got[key + ".sq.x"]) - o.PSNR(x, ref["x"])) <= 1e-3
            continue
        for sp in (3, 0, 2):
            np.testing.assert_array_equal(got["%s.salsa%d.x" % (key, sp)], got[key + ".salsa1.x"], err_msg=key)
            np.testing.assert_array_equal(got["%s.salsa%d.obj" % (key, sp)], got[key + ".salsa1.obj"], err_msg=key)
        assert len(got[key + ".salsa1.obj"]) == 7
        st = o.demo_setup("moffat", x, np.random.default_rng(3).standard_normal((M, N)), evMax=1.0)
        p, model = st["p_true"], st["model"]
        Psi = lambda v, th: o.chambolle_prox_TV_stop(v, lam=th, maxiter=25)[0]
        ref = o.my_fista(st["y"], lambda v: model.A(v, *p), lambda v: model.AT(v, *p), 0.03 * st["sigma"] ** 2, 1.0, o.TVnorm, Psi,
                         1, 1e-4, 25, x)
        assert len(got[key + ".fista.obj"]) == len(ref["objective"]), key
        np.testing.assert_allclose(got[key + ".fista.obj"], ref["objective"], rtol=1e-9, err_msg=key)
        assert np.max(np.abs(got[key + ".fista.x"] - ref["x"])) < 1e-7, key


def _prox_pair(M, N, K, lam, seed, warm=False):
    """Cold K iterations (then K more warm-started with a changed g) on device buffers against the oracle."""
    import sbtv
    g = _image(M, N, seed)
    got = sbtv.chambolle_prox_TV_stop(sbtv.to_device(g), "lambda", lam, "maxiter", K, return_info=True)
    want = _oracle(g, lam, K)
    bad = []
    res = {"c.f": sbtv.to_host(got[0]), "c.px": sbtv.to_host(got[1]), "c.py": sbtv.to_host(got[2]), "c.k": got[3], "c.err": got[4]}
    _check(bad, "c", res, want)
    if warm:
        g2 = g + 0.5 * np.random.default_rng(seed + 1).standard_normal((M, N))
        got2 = sbtv.chambolle_prox_TV_stop(sbtv.to_device(g2), "lambda", lam, "maxiter", K, "dualvars", (got[1], got[2]),
                                           return_info=True)
        res = {"w.f": sbtv.to_host(got2[0]), "w.px": sbtv.to_host(got2[1]), "w.py": sbtv.to_host(got2[2]), "w.k": got2[3],
               "w.err": got2[4]}
        _check(bad, "w", res, _oracle(g2, lam, K, start=(want[1], want[2])))
    assert not bad, "%d x %d: %s" % (M, N, bad)


def test_plan_chosen_kernel_at_edge_sizes(ctx, geoms):
    """The two-rows-per-lane kernel as the plans choose it (no hook), at sizes whose last tile row and column sit on either
    side of the interior test: 10 iterations cold, 10 more warm-started."""
    geom = geoms["rows2"]
    for q, (M, N, why) in enumerate(tg.edge_large_shapes(geom)):
        v = ctx.prox_variant(M, N)
        assert v["rows_per_lane"] == 2 and v["fused"] and v["tiles"] >= 256, (M, N, v)
        assert v["tiles"] == tg.n_tiles(geom, M, N)
        tl = [t for t in tg.classify(geom, M, N) if t["i0"] >= 1 and t["j0"] >= 1]
        if q == 0:      # a region that ends exactly at the last row AND the last column: inside the image, not interior
            assert any(t["di"] == 0 and t["dj"] == 0 and not t["interior"] for t in tl), why
        else:           # ... and one row / column further in: interior by the smallest margin on both axes
            assert any(t["interior"] and 1 <= t["di"] <= 2 and t["dj"] == 1 for t in tl), why
        _prox_pair(M, N, 10, 7.5, 41, warm=True)


def test_tile_table_and_stagger_whole_image(ctx, geoms):
    """Whole-image comparison where the workgroup -> tile table and the first-round stagger are active: 2048 x 2048 (the
    size the benchmark times) and three more shapes picked by what the library reports, covering a table without
    stagger, a table with stagger, a tile count that is a multiple of 8 and an odd one; one of them also as a batch of two
    (the table is shared by the images of a batch, the stagger applies to image 0 only)."""
    import sbtv
    geom = geoms["rows2"]
    rep = {}
    for M, N, _ in [(2048, 2048, "")] + tg.table_candidates(geom):
        gm, v = ctx.prox_geometry(M, N), ctx.prox_variant(M, N)
        assert v["rows_per_lane"] == 2 and v["tiles"] == gm["tiles_i"] * gm["tiles_j"] == tg.n_tiles(geom, M, N), (M, N, v, gm)
        rep[(M, N)] = dict(order=gm["order"], stagger=gm["stagger"], nt=v["tiles"])
    assert rep[(2048, 2048)]["order"] and rep[(2048, 2048)]["stagger"] > 0, rep[(2048, 2048)]
    classes = {"table without stagger": lambda r: r["order"] and r["stagger"] == 0,
               "multiple of 8": lambda r: r["order"] and r["nt"] % 8 == 0,
               "odd": lambda r: r["order"] and r["nt"] % 2 == 1}
    picked = []
    for cname, fn in classes.items():
        hit = [s for s in rep if s != (2048, 2048) and fn(rep[s])]
        assert hit, "no candidate shape has a plan with: %s (%s)" % (cname, rep)
        if not any(fn(rep[s]) for s in picked):
            picked.append(hit[0])
    for s in rep:                                             # three shapes besides 2048 x 2048
        if len(picked) < 3 and s not in picked and s != (2048, 2048) and rep[s]["order"]:
            picked.append(s)
    assert len(picked) == 3, picked
    for M, N in picked + [(2048, 2048)]:
        _prox_pair(M, N, 10, 7.5, 43)
    # batch of two on the smallest picked shape
    M, N = min(picked, key=lambda s: s[0] * s[1])
    assert ctx.prox_geometry(M, N, 2)["order"]
    g = np.stack([_image(M, N, 45), _image(M, N, 46)])
    lam = np.array([6.0, 9.0])
    f, px, py, k, err = sbtv.chambolle_prox_TV_stop(sbtv.to_device(g), "lambda", lam, "maxiter", 10, return_info=True)
    res = {"b.f": sbtv.to_host(f), "b.px": sbtv.to_host(px), "b.py": sbtv.to_host(py), "b.k": k, "b.err": err}
    bad = []
    for b in range(2):
        _check(bad, "b", res, _oracle(g[b], lam[b], 10), b)
    assert not bad, bad


def test_caller_buffers_only_8_byte_aligned(ctx, geoms):
    """An even-M image whose device pointer is 8 but not 16 bytes aligned goes to the scalar forms of the one-iteration
    kernels (chambolle_iter_kernel<false>, chambolle_finish_kernel<false>, tvnorm_kernel<false>), which odd M never
    exercises with an even leading dimension."""
    import torch
    import sbtv
    import sbtv_oracle as o
    geom = geoms["rows2"]
    TI, TJ = geom["single_ti"], geom["single_tj"]
    for M, N in ((TI + 2, TJ + 1), (2 * TI, 2 * TJ + 1)):
        g = _image(M, N, _seed(M, N))
        buf = torch.zeros(M * N + 2, dtype=torch.float64, device="cuda:0")
        gd = buf[1:1 + M * N].view(N, M).permute(1, 0)
        gd.copy_(torch.from_numpy(g).to("cuda:0"))
        assert gd.data_ptr() % 16 == 8 and gd.stride() == (1, M)
        assert sbtv.TVnorm(gd) == pytest.approx(o.TVnorm(g), rel=1e-13)
        bad = []
        got = sbtv.chambolle_prox_TV_stop(gd, "lambda", LAM, "maxiter", 5, return_info=True)
        want = _oracle(g, LAM, 5)
        res = {"c.f": sbtv.to_host(got[0]), "c.px": sbtv.to_host(got[1]), "c.py": sbtv.to_host(got[2]), "c.k": got[3], "c.err": got[4]}
        _check(bad, "c", res, want)
        got2 = sbtv.chambolle_prox_TV_stop(gd, "lambda", LAM, "maxiter", 5, "dualvars", (got[1], got[2]), return_info=True)
        res = {"w.f": sbtv.to_host(got2[0]), "w.px": sbtv.to_host(got2[1]), "w.py": sbtv.to_host(got2[2]), "w.k": got2[3],
               "w.err": got2[4]}
        _check(bad, "w", res, _oracle(g, LAM, 5, start=(want[1], want[2])))
        assert not bad, "%d x %d: %s" % (M, N, bad)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(*sys.argv[2:5])
