"""Image geometries at which the TV-model samplers sbtv_skrock, sbtv_SAPG_skrock, sbtv_myula_masked and sbtv_SAPG_masked take
the size-dependent code their own case tables (tests/skrock_tv_cases.py, tests/sapg_skrock_cases.py,
tests/masked_sapg_cases.py: 32 x 32, 24 x 40, 8 x 6) never reach.  Shared by tests/test_tv_sampler_geometry_cases_cpu.py and
tests/test_gpu_tv_sampler_sweep.py.  Plain Python, no GPU.

One table per driver, tag -> case; every tag names the CLASS it is there for:

  wave    1024 x 1024  the wave FFT plan (pipelined row kernel, TV partials riding the wave column pass, OP_GRAD / OP_RESID
                       there); P/2 = 2 x 1024 x 256 pairs, so every lane of the element-wise kernels (grid capped at 1024
                       workgroups of 256 lanes by ew_blocks) makes two grid-stride trips; ntv = N = 1024 column partials and, in
                       the masked drivers, nblk = 1024 residual partials: four trips of the 256-lane totalling loops; the
                       128-row, two-rows-per-lane "tile" Chambolle kernel of the large images, re-armed in-kernel by skrock_arm
  seam    1090 x 481   P/2 = 1024 x 256 + 1: exactly one lane (pair 262 144) makes a second trip; chirp-z transform;
                       tvnorm_partials leaves 9 x 31 = 279 > 256 partials, so the totalling loop makes a second trip on that path
  rect-*  256 x 64, 64 x 256   power-of-two workgroup plans with M != N: column-major strides on both sides
  p16     16 x 16      the partial-wave row pass (fewer than 64 threads per row workgroup)
  oddM    25 x 40      odd M beside even N: the scalar Chambolle kernels and tvnorm_kernel<false>
  tiny    8 x 8        32 pairs: less than one wave (SK-ROCK drivers; the masked drivers have their own 8 x 6 case)

The plan class of a shape is TAKEN from fft_plan_cases.model_plan (`geometry`), never assumed; `classes` names what a case
reaches and REQUIRED what a table has to reach (`assert_reaches`).  The GPU module checks the model against the reports of the
library (Context.fft_plan, Context.prox_geometry) before it launches anything.

Protocol: that of the drivers' own case modules, whose builders make the problems (nothing is copied): demo_setup, delta = 0.8
of the stability bound, the c-scales x 0.02 for SAPG, their mask builders.  Chains are short: 2 steps at fixed parameters (one
case with an even and one with an odd stage count at every class that matters), warm-up 2 and 3 samples for SAPG (one warm-up
update, the start update and two main updates: with a free PSF parameter the spectra are rebuilt once at that size), 3 samples
for the masked MYULA chain (one move).  Every SAPG case has a free PSF parameter.  At wave and seam chambolleit is 10, not 25:
with 25 the final prox errors there are 0.1 - 0.25 against tol 1e-3, the stop rule is far from firing, and the iteration count
is not what those cases test.  No case may sit on the edge of the Chambolle stop rule
(tests/test_tv_sampler_geometry_cases_cpu.py checks it): should one, change its SEED.

Measured CPU seconds of one reference (the restatement; BLAS and OpenMP held to one thread as tests/conftest.py does):
  skrock       wave 2.0  seam 1.5  rect 0.04 - 0.08  others 0.01
  SAPG_skrock  wave 3.5  seam 2.5  rect 0.06         others 0.01 - 0.02
  SAPG_masked  wave 2.6 (valid and holes)  seam 1.1 (both)  rect 0.03 - 0.05  others 0.01
  myula_masked wave 0.5  seam 0.2 - 0.3  others below 0.01
and building a problem (demo_setup, noise, mask) takes 0.1 - 0.35 s at wave and seam.  The three CPU checks of a case cost about
five references (two more prox evaluations per call with alt_tols, one perturbed chain).
Each reference is computed once per session and never modified."""
import functools

import numpy as np

import fft_plan_cases as fpc
import masked_sapg_cases as msc
import sapg_skrock_cases as ssc
import skrock_tv_cases as skc

STEPS = 2                                    # sbtv_skrock: samples = 3
SAPG = dict(samples=3, warmup=2, burnIn=2)   # both SAPG drivers
MYULA_SAMPLES = 3                            # sbtv_myula_masked: X(1) = y and one move
BIG_CHAMBOLLEIT = 10                         # wave and seam

# ---- what the kernels are built with (csrc/elementwise.hip: ew_blocks, EWB; csrc/tv.hip: TI, TJ; the 256-lane totalling loops
# of skrock_trace_kernel / sapg_chain_update_kernel); the GPU module checks the tile against Context.prox_geometry
EW_LANES, EW_MAX_BLOCKS, TOTAL_LANES = 256, 1024, 256
TVNORM_TILE = (128, 16)

_valid = lambda s: msc.valid_mask(s, 7)
_holes = lambda s: msc._holes(s, 21)
_holes2 = lambda s: msc._holes(s, 23)
_weights = lambda s: msc._weights(s, 22)
_zero_row = lambda s: msc._zero_row(s, 2)

# tag -> (M, N, stages, steps, seed, chambolleit): the tuple skrock_tv_cases.build takes
SKROCK = {
    "wave": (1024, 1024, 2, STEPS, 8, BIG_CHAMBOLLEIT),        # even s
    "seam": (1090, 481, 3, STEPS, 8, BIG_CHAMBOLLEIT),         # odd s: the sample and P_next swap buffers
    "rect-tall": (256, 64, 2, STEPS, 8, 25),
    "rect-wide": (64, 256, 3, STEPS, 8, 25),
    "p16": (16, 16, 3, STEPS, 8, 25),
    "oddM": (25, 40, 2, STEPS, 9, 25),
    "tiny": (8, 8, 3, STEPS, 8, 25),
}
# tag -> the dict sapg_skrock_cases.build takes
SAPG_SKROCK = {
    "wave": dict(kind="gaussian", M=1024, N=1024, stages=2, seed=11, fix=(False, False), chambolleit=BIG_CHAMBOLLEIT),
    "seam": dict(kind="moffat", M=1090, N=481, stages=3, seed=11, chambolleit=BIG_CHAMBOLLEIT),
    "rect-tall": dict(kind="laplace", M=256, N=64, stages=3, seed=11),
    "rect-wide": dict(kind="moffat", M=64, N=256, stages=2, seed=11),
    "p16": dict(kind="laplace", M=16, N=16, stages=2, seed=11),
    "oddM": dict(kind="moffat", M=25, N=40, stages=3, seed=11),
    "tiny": dict(kind="gaussian", M=8, N=8, stages=2, seed=11, fix=(False, False)),
}
# tag -> the dict masked_sapg_cases.build takes
SAPG_MASKED = {
    "wave-valid": dict(kind="gaussian", M=1024, N=1024, seed=11, fix=(False, False), mask=_valid, chambolleit=BIG_CHAMBOLLEIT),
    "wave-holes": dict(kind="laplace", M=1024, N=1024, seed=11, mask=_holes, chambolleit=BIG_CHAMBOLLEIT),
    "seam-valid": dict(kind="moffat", M=1090, N=481, seed=11, mask=_valid, chambolleit=BIG_CHAMBOLLEIT),
    "seam-holes": dict(kind="laplace", M=1090, N=481, seed=11, mask=_holes, chambolleit=BIG_CHAMBOLLEIT),
    "rect-tall": dict(kind="laplace", M=256, N=64, seed=11, mask=_weights),
    "rect-wide": dict(kind="moffat", M=64, N=256, seed=11, mask=_holes),
    "p16": dict(kind="gaussian", M=16, N=16, seed=11, fix=(False, False), mask=_valid),
    "oddM": dict(kind="moffat", M=25, N=40, seed=11, mask=_zero_row),
}
# tag -> the dict masked_sapg_cases.myula_build takes (the chain runs at th_init, p_true and the true sigma2)
MYULA_MASKED = {
    "wave-valid": dict(kind="moffat", M=1024, N=1024, seed=12, mask=_valid, chambolleit=BIG_CHAMBOLLEIT),
    "wave-holes": dict(kind="gaussian", M=1024, N=1024, seed=12, mask=_holes, chambolleit=BIG_CHAMBOLLEIT),
    "seam-valid": dict(kind="laplace", M=1090, N=481, seed=12, mask=_valid, chambolleit=BIG_CHAMBOLLEIT),
    "seam-holes": dict(kind="moffat", M=1090, N=481, seed=12, mask=_holes, chambolleit=BIG_CHAMBOLLEIT),
    "rect-tall": dict(kind="gaussian", M=256, N=64, seed=12, mask=_holes),
    "rect-wide": dict(kind="laplace", M=64, N=256, seed=12, mask=_weights),
    "p16": dict(kind="moffat", M=16, N=16, seed=12, mask=_zero_row),
    "oddM": dict(kind="gaussian", M=25, N=40, seed=12, mask=_valid),
}
TABLES = {"skrock": SKROCK, "SAPG_skrock": SAPG_SKROCK, "SAPG_masked": SAPG_MASKED, "myula_masked": MYULA_MASKED}
DRIVERS = tuple(TABLES)
ALL = tuple((d, t) for d in DRIVERS for t in TABLES[d])
# the masks a second image of a batch gets (tests/test_gpu_tv_sampler_sweep.py): another one than the case's
OTHER_MASK = {"wave-valid": _holes2, "wave-holes": _valid, "seam-valid": _holes2, "seam-holes": _valid, "oddM": _holes2}


def _key(case):
    return tuple(sorted(case.items()))


def shape(driver, tag):
    c = TABLES[driver][tag]
    return (c[0], c[1]) if driver == "skrock" else (c["M"], c["N"])


def stages(driver, tag):
    c = TABLES[driver][tag]
    return c[2] if driver == "skrock" else c.get("stages")


def problem(driver, tag):
    """The problem dict of the driver's own case module (cached there)."""
    c = TABLES[driver][tag]
    if driver == "skrock":
        return skc.build(*c)
    if driver == "SAPG_skrock":
        return ssc.build(_key(c), **SAPG)
    if driver == "SAPG_masked":
        return msc.build(_key(c), **SAPG)
    return msc.myula_build(_key(c), MYULA_SAMPLES)


def chain(driver, tag, **kw):
    """The driver's restatement on a case; kw as the chain_of of its case module takes them."""
    q = problem(driver, tag)
    of = {"skrock": skc.chain_of, "SAPG_skrock": ssc.chain_of, "SAPG_masked": msc.chain_of, "myula_masked": msc.myula_chain_of}
    return of[driver](q, **kw)


@functools.lru_cache(maxsize=None)
def reference(driver, tag):
    """The restatement on the case's injected normals (read-only for its users)."""
    return chain(driver, tag)


def prox_calls(driver, tag):
    """Chambolle prox calls of one chain."""
    if driver == "skrock":
        return stages(driver, tag) * STEPS
    if driver == "SAPG_skrock":
        return stages(driver, tag) * (SAPG["warmup"] - 1 + SAPG["samples"] - 1)
    if driver == "SAPG_masked":
        return 1 + (SAPG["warmup"] - 1) + 1 + (SAPG["samples"] - 1)
    return MYULA_SAMPLES - 2


def last_sample(driver, r):
    return r["x"] if driver == "myula_masked" else r["samples"][-1]


# ---- the model of the size-dependent code ------------------------------------------------------------------------------
def ew_blocks(P):
    """csrc/elementwise.hip: ew_blocks."""
    return min(max((P // 2 + EW_LANES - 1) // EW_LANES, 1), EW_MAX_BLOCKS)


def trips(n, lanes=TOTAL_LANES):
    """Trips of the busiest lane of `for (i = tid; i < n; i += lanes)`."""
    return (n + lanes - 1) // lanes


def geometry(M, N, batch=1):
    """What the drivers derive from the image size: dict(plan (fft_plan_cases.model_plan), plan_class, pairs, ew_blocks,
    lanes_on_trip_2 (lanes of the element-wise grid that make a second grid-stride trip), max_trips, ntv (partials of TVnorm the
    trace / update kernels total), nrb (row-pass accumulators of the SK-ROCK drivers), nblk (residual partials of the masked
    drivers), scalar_tv (odd M: the scalar Chambolle kernels and tvnorm_kernel<false>))."""
    plan = fpc.model_plan(M, N, batch)
    P = M * N
    pairs, nb = P // 2, ew_blocks(P)
    grid = nb * EW_LANES
    if plan["generic"]:
        cls = "chirp"
        ntv = ((M + TVNORM_TILE[0] - 1) // TVNORM_TILE[0]) * ((N + TVNORM_TILE[1] - 1) // TVNORM_TILE[1])    # tvnorm_partials
    elif plan["wave"]:
        cls, ntv = "wave", N                                                                                 # fft_cols_blocks
    else:
        cls, ntv = "workgroup", plan["cols_wgs"]
    return dict(plan=plan, plan_class=cls, pairs=pairs, ew_blocks=nb, lanes_on_trip_2=min(max(pairs - grid, 0), grid),
                max_trips=(pairs + grid - 1) // grid, ntv=ntv, nrb=plan["rows_wgs"], nblk=nb, scalar_tv=M % 2 == 1,
                plan_classes=fpc.classes(M, N, plan))


def classes(driver, tag):
    """The names of the size-dependent paths a case reaches."""
    M, N = shape(driver, tag)
    g = geometry(M, N)
    masked = driver in ("SAPG_masked", "myula_masked")
    out = {"plan: " + g["plan_class"]}
    if g["plan_class"] == "workgroup" and M != N:
        out.add("plan: workgroup, M > N" if M > N else "plan: workgroup, M < N")
    if ("partial wave", True) in g["plan_classes"]:
        out.add("partial-wave row pass")
    grid = g["ew_blocks"] * EW_LANES
    if g["lanes_on_trip_2"] == grid:
        out.add("grid stride: every lane twice")
    if g["lanes_on_trip_2"] == 1:
        out.add("grid stride: one lane twice")
    if g["pairs"] < 64:
        out.add("fewer pairs than one wave")
    if g["scalar_tv"] and N % 2 == 0:
        out.add("odd M, even N")
    if g["plan_class"] == "wave":
        out.add("tile Chambolle")
    if driver != "myula_masked":                               # the fixed-parameter masked chain has no trace and no totals
        if trips(g["ntv"]) == 4:
            out.add("totals: ntv in four trips")
        if g["plan_class"] == "chirp" and g["ntv"] > TOTAL_LANES:
            out.add("totals: tvnorm_partials above 256")
        if driver == "SAPG_masked" and trips(g["nblk"]) == 4:
            out.add("totals: masked nblk in four trips")
    if stages(driver, tag) is not None:
        out.add("stages: odd" if stages(driver, tag) % 2 else "stages: even")
    if masked and tag.endswith("-valid"):
        out.add("mask: valid")
    if masked and tag.endswith("-holes"):
        out.add("mask: holes")
    return out


_SHAPES = {"plan: wave", "plan: chirp", "plan: workgroup, M > N", "plan: workgroup, M < N", "partial-wave row pass",
           "grid stride: every lane twice", "grid stride: one lane twice", "odd M, even N", "tile Chambolle"}
_TOTALS = {"totals: ntv in four trips", "totals: tvnorm_partials above 256"}
REQUIRED = {
    "skrock": _SHAPES | _TOTALS | {"fewer pairs than one wave", "stages: odd", "stages: even"},
    "SAPG_skrock": _SHAPES | _TOTALS | {"fewer pairs than one wave", "stages: odd", "stages: even"},
    "SAPG_masked": _SHAPES | _TOTALS | {"totals: masked nblk in four trips", "mask: valid", "mask: holes"},
    "myula_masked": _SHAPES | {"mask: valid", "mask: holes"},
}


def coverage(driver):
    """{class: [tags]} of a driver's table."""
    cov = {}
    for tag in TABLES[driver]:
        for c in classes(driver, tag):
            cov.setdefault(c, []).append(tag)
    return cov


def assert_reaches(driver):
    cov = coverage(driver)
    missing = sorted(c for c in REQUIRED[driver] if not cov.get(c))
    assert not missing, "%s: no case reaches %s" % (driver, missing)
    return cov
