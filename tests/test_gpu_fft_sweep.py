"""GPU sweep of the FFT passes, the fused spectral operators and the fused column epilogues over every plan class.

Shapes come from tests/fft_plan_cases.py; before anything is launched the plans the library REPORTS
(`Context.fft_plan`) are checked against the documented table and the lists are shown to reach every class.  Everything
a kernel is compared with is built from `scipy.fft` on `np.longdouble` (80-bit) inputs: fft2, the closures, every
operator's output image, every accumulator as the plain sum over the full spectrum, the bookkeeping arrays and sums,
the periodic TV.  The float64 restatement of the same formulas is computed alongside only to size the bars.

Bars
  * rfft2, the round trip, A, AT, dA, invLS, A(delta), A(const), the adjoint identity: the bars of test_gpu_fft.py
    (powers of two) and test_gpu_anysize.py (chirp-z), unchanged.  Chirp-z shapes larger than (100, 4096), the largest
    tested before, scale the 5e-11 of A and AT (only that one) with log2(L_M L_N) / log2(256 * 8192), L the Bluestein
    length.
  * quantities without a bar before this sweep (outputs of OP_SALSA / GRAD / GRADF / ATA / CSALSA / NONE / RESID, the
    accumulators, the bookkeeping arrays and sums, the TV): 64 x the error of the float64 restatement against the
    long-double reference at that shape, floored at 64 eps log2(L_M L_N) relative to the largest reference value.

Largest error of a kernel against the long-double reference over the module (one MI355X, 219 tests: transforms and
closures at 81 shapes, 10 operators and 7 epilogue forms at the same 81, 9 operators at 34 chirp-z shapes), next to
the bar at the shape where error / bar is largest:
  quantity                                     bar        error      at
  A(const) = const                             1.000e-13  8.882e-16  16x16
  A(delta) = taps                              1.000e-15  6.939e-18  16x16
  A, taille 1..15, against the spatial sum     2.000e-11  1.705e-13  1024x1024x2 taille 1
  AT                                           2.000e-11  1.952e-13  2048x4096
  OP_ATA x                                     2.111e-11  1.011e-13  32x32
  OP_CSALSA acc0 (relative)                    1.279e-13  6.967e-16  32x16
  OP_CSALSA acc1 (relative)                    1.279e-13  9.716e-16  32x16
  OP_CSALSA acc2 (relative)                    1.847e-13  6.317e-16  16x512
  OP_CSALSA x                                  4.191e-10  3.781e-12  32x16
  OP_GRAD acc0 (relative)                      5.684e-14  2.903e-16  2x2
  OP_GRAD acc1 (relative)                      1.421e-13  1.589e-14  60x3
  OP_GRAD acc2 (relative)                      1.281e-12  3.965e-14  60x33
  OP_GRAD x                                    5.331e-13  1.243e-14  2x2
  OP_GRADF acc0 (relative)                     5.684e-14  2.903e-16  2x2
  OP_GRADF x                                   5.331e-13  1.243e-14  2x2
  OP_INVLS x (relative)                        1.000e-12  1.065e-15  4096x4096
  OP_MUL_H x                                   2.000e-11  1.640e-13  1024x1024 SBTV_FFT_WAVE=0
  OP_MUL_HC x                                  2.000e-11  1.727e-13  4096x2048
  OP_NONE x                                    3.961e-11  2.274e-13  60x8
  OP_RESID acc0 (relative)                     5.684e-14  2.903e-16  2x2
  OP_RESID x                                   3.961e-11  2.274e-13  60x8
  OP_SALSA acc0 (relative)                     5.684e-14  2.853e-16  2x2
  OP_SALSA x                                   1.336e-10  1.204e-12  60x3
  adjoint identity (relative)                  1.000e-11  5.291e-14  2048x2048
  bookkeeping bu                               1.301e-10  1.207e-12  60x3 tru xprev
  bookkeeping g                                6.356e-12  1.085e-13  2x2 tru xprev
  bookkeeping sum (x-true)^2 (relative)        1.563e-13  1.009e-15  60x7 tru xprev
  bookkeeping sum (x-u)^2 (relative)           5.684e-14  6.097e-16  2x2 tru xprev
  bookkeeping sum (x-xprev)^2 (relative)       1.563e-13  1.204e-15  60x7 tru xprev
  bookkeeping sum TV(u) (relative)             1.421e-13  1.804e-16  60x3 tru xprev
  bookkeeping sum u^2 (relative)               1.563e-13  2.153e-16  8x50 tru xprev
  bookkeeping sum x^2 (relative)               5.684e-14  4.918e-16  2x2 tru xprev
  dA                                           2.000e-10  6.312e-14  1024x4096
  forward TV (relative)                        1.279e-13  1.238e-16  32x16
  invLS (relative)                             1.000e-12  1.229e-15  4096x2048
  rfft2 / sqrt(MN)                             5.500e-13  8.690e-16  16x128
  rfft2 round trip                             1.900e-12  3.109e-15  128x4096
  step y - alpha x                             5.621e-10  6.753e-13  1024x2048
  sub g = x - b                                5.452e-10  1.739e-12  1024x1024
No quantity reaches 12 % of its bar; no kernel bug was found.

Value-only mutants of csrc/fft.hip, fft_wave.inc and fft_any.inc, one at a time on a scratch copy (never committed),
against this module and the modules that existed before it (F = fails, . = passes):
                                                             this  fft  anysize  salsa  sapg_fista  admm
  1 Parseval weight 2 on the packed-row branch (fft_rows)     F     .     .       F       F         F
  2 hq replaced by hh in that branch                          F     F     .       F       F         F
  3 e == 0 packing of fft_cols_inv_kernel, sign flipped       F     F     .       F       F         F
  4 POST left-neighbour wrap N - 1 -> N - 2                   F     .     .       F       .         .
  5 forward-TV left-neighbour wrap N - 1 -> N - 2             F     .     .       .       F         F
  6 rows_rk returns 4 where it returns 1                      F     .     .       .       .         .
  7 inverse chirp conjugation dropped for n >= 2049           F     .     F       .       .         .
  8 lch chunk drops its last row                              F     F     .       F       F         F
  9 rows_pipe fold: image 1 of a folded batch mapped to 0     F     .     .       .       F         .
Mutant 6 computes correct values with another kernel: only the plan report shows it.  Mutant 9 first passed the
operator tests because they compared images 0 and 2 of the shared-spectrum batch only; image 1 was added.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.fft

import fft_plan_cases as fc

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
MU0 = 0.003
CS = (1.3, -0.4, 0.7)
SENTINEL = -12345.678
KINDS = (("gaussian", (0.4, 0.3)), ("moffat", (0.4, 3.5)), ("laplace", (0.3,)))
# operators that run with the `add` operand; the others run without it and with the forward pass's TV
OPS_WITH_ADD = ("mul_h", "invls", "salsa", "ata", "csalsa")
OPS_PLAIN = ("none", "mul_hc", "resid", "grad", "gradf")
FIGURES = {}                               # quantity -> (largest error / bar, error, bar, shape)


@pytest.fixture(scope="module", autouse=True)
def _figures_table():
    yield
    for q in sorted(FIGURES):
        r, e, b, s = FIGURES[q]
        print("SWEEP %-28s largest error %.3e  bar %.3e  (%.3f of the bar) at %s" % (q, e, b, r, s))


def check(quantity, err, bar, where):
    """Record the figure, then assert it."""
    err, bar = float(err), float(bar)
    r = err / bar if bar > 0 else (0.0 if err == 0 else np.inf)
    if quantity not in FIGURES or r > FIGURES[quantity][0]:
        FIGURES[quantity] = (r, err, bar, where)
    assert err <= bar, "%s at %s: error %.3e against the long-double reference, bar %.3e" % (quantity, where, err, bar)


# ---------------------------------------------------------------------------------------------------------------------
# reference: the same formulas in long double (the reference) and in float64 (only to size the bars)
# ---------------------------------------------------------------------------------------------------------------------
def fft2_pair(a, b, dt):
    """fft2 of two REAL arrays with one complex transform.  Only for arrays of like magnitude AND like mean: the rounding
    of one transform is relative to its largest entries, and the DC term of an image would drown a tap spectrum."""
    Z = scipy.fft.fft2(a.astype(dt) + 1j * b.astype(dt))
    Zr = np.conj(np.roll(Z[::-1, ::-1], (1, 1), axis=(0, 1)))          # conj(Z[-k, -l])
    return (Z + Zr) / 2, (Z - Zr) / 2j


def ifft2_pair(Za, Zb):
    """real(ifft2) of two spectra of REAL images with one complex transform."""
    z = scipy.fft.ifft2(Za + 1j * Zb)
    return z.real, z.imag


def pad(taps, M, N, dt):
    h = np.zeros((M, N), dtype=dt)
    t = np.asarray(taps)
    h[:t.shape[0], :t.shape[1]] = t
    return h


def tvnorm(u):
    return np.sum(np.sqrt((u - np.roll(u, 1, axis=1)) ** 2 + (u - np.roll(u, 1, axis=0)) ** 2))


def sweep_inputs(M, N, seed=0):
    import sbtv
    rng = np.random.default_rng(1000003 * M + N + seed)
    d = dict(x=rng.uniform(0, 255, (M, N)), add=rng.uniform(-20, 20, (M, N)), y=rng.uniform(0, 255, (M, N)),
             e0=rng.uniform(-5, 5, (M, N)), u=rng.uniform(0, 255, (M, N)), bu=rng.uniform(-10, 10, (M, N)),
             tru=rng.uniform(0, 255, (M, N)), xprev=rng.uniform(0, 255, (M, N)), mu=MU0)
    t = min(7, M, N)
    taps, dt = sbtv.psf_family("gaussian", t, (0.4, 0.3))
    d.update(taps=taps, d1=dt[0], d2=dt[1])
    return d


def operator_reference(d, dt, ops):
    """{op: dict(x=image, acc=(3,))} for one image, all in dtype `dt`; sums as plain sums over the FULL spectrum."""
    M, N = d["x"].shape
    c = lambda a: np.asarray(a).astype(dt)
    Xp, Y = fft2_pair(d["x"], d["y"], dt)
    Xadd, E0 = fft2_pair(d["add"], d["e0"], dt)
    Xa = Xp + Xadd                                                      # spectrum of x + add
    H, D1 = fft2_pair(pad(d["taps"], M, N, dt), pad(d["d1"], M, N, dt), dt)
    D2 = scipy.fft.fft2(pad(d["d2"], M, N, dt)) if "grad" in ops else None
    mu = dt(d["mu"])
    den = np.abs(H) ** 2 + mu
    s = lambda Z: np.sum(np.abs(Z) ** 2)
    out = {}
    spec = {}
    for op in ops:
        X = Xa if op in OPS_WITH_ADD else Xp
        acc = [dt(0)] * 3
        if op in ("none", "resid"):
            if op == "resid":
                acc[0] = s(H * X - Y)
            out[op] = dict(x=c(d["x"]), acc=acc)
            continue
        if op == "mul_h":
            Z = H * X
        elif op == "mul_hc":
            Z = np.conj(H) * X
        elif op == "invls":
            Z = X / den
        elif op == "ata":
            Z = X * np.abs(H) ** 2
        elif op == "salsa":
            Z = (np.conj(H) * Y + mu * X) / den
            acc[0] = s(Y - H * Z)
        elif op in ("grad", "gradf"):
            R = H * X - Y
            Z = np.conj(H) * R
            acc[0] = s(R)
            if op == "grad":
                acc[1] = np.sum((D1 * X * np.conj(R)).real)
                acc[2] = np.sum((D2 * X * np.conj(R)).real)
        elif op == "csalsa":
            continue
        spec[op] = (Z, acc)
    # two images per inverse transform, of like magnitude (invls is 1 / mu times larger: alone); grad = gradf
    todo = [k for k in ("mul_h", "mul_hc", "ata", "salsa", "gradf", "grad") if k in spec and not (k == "grad" and "gradf" in spec)]
    pairs = list(zip(todo[0::2], todo[1::2] + [None] * (len(todo) % 2))) + ([("invls", None)] if "invls" in spec else [])
    for a, b in pairs:
        za, zb = spec[a][0], (spec[b][0] if b else np.zeros_like(spec[a][0]))
        ia, ib = ifft2_pair(za, zb)
        out[a] = dict(x=ia, acc=spec[a][1])
        if b:
            out[b] = dict(x=ib, acc=spec[b][1])
    if "grad" in spec and "gradf" in spec:
        out["grad"] = dict(x=out["gradf"]["x"], acc=spec["grad"][1])
    if "csalsa" in ops:
        # two passes: the second transforms the x of the first (plus add) and meets the state the first one left
        E, X, xs = E0, Xa, None
        for _ in range(2):
            W = dt(CS[0]) * Y + dt(CS[1]) * E
            Z = (np.conj(H) * W + mu * X) / den
            T = H * Z - Y
            En = T + dt(CS[2]) * E
            acc = [s(T), s(En), s(En - E)]
            E = En
            xs = scipy.fft.ifft2(Z).real
            X = scipy.fft.fft2(xs + c(d["add"]))
        out["csalsa"] = dict(x=xs, acc=acc)
    for op in out:
        out[op]["acc"] = np.array([a / dt(M * N) for a in out[op]["acc"]], dtype=dt)
    return out


def bookkeeping_reference(x, d, dt, tru=True, xprev=True, bu=None):
    c = lambda a: np.asarray(a).astype(dt)
    u, b0 = c(d["u"]), c(d["bu"] if bu is None else bu)
    bu1 = b0 + (u - x)
    sums = [np.sum((x - c(d["tru"])) ** 2) if tru else dt(0), np.sum((x - u) ** 2), np.sum(x ** 2), np.sum(u ** 2),
            np.sum((x - c(d["xprev"])) ** 2) if xprev else dt(0), tvnorm(u)]
    return dict(bu=bu1, g=x - bu1, sums=np.array(sums, dtype=dt))


def log2L(M, N, plan):
    return np.log2((plan["L_M"] or M) * (plan["L_N"] or N))


def new_bar(ref_ld, ref_f64, M, N, plan):
    """64 x the float64 restatement's own error, floored at 64 eps log2(L_M L_N) relative."""
    scale = float(np.max(np.abs(ref_ld)))
    own = float(np.max(np.abs(np.asarray(ref_f64).astype(LD) - ref_ld)))
    return max(64.0 * own, 64.0 * EPS * log2L(M, N, plan) * scale)


def err(got, ref_ld):
    return float(np.max(np.abs(np.asarray(got).astype(LD) - ref_ld)))


def chirp_scale(M, N, plan):
    """1 up to the largest chirp-z shape tested before this sweep, log2(L_M L_N) / log2(256 * 8192) above it."""
    return max(1.0, log2L(M, N, plan) / 21.0) if plan["generic"] else 1.0


def closure_bars(M, N, plan):
    g = plan["generic"]
    k = chirp_scale(M, N, plan)
    return dict(A=(5e-11 if g else 2e-11) * k, dA=5e-10 if g else 2e-10, invLS=1e-11 if g else 1e-12,
                delta=1e-14 if g else 1e-15, const=1e-12 if g else 1e-13, adjoint=1e-10 if g else 1e-11)


def reported(ctx, M, N, batch=1):
    """The library's plan, checked against the documented table (fft_plan_cases.model_plan) before any launch."""
    plan = ctx.fft_plan(M, N, batch)
    assert plan == fc.model_plan(M, N, batch), ("the library's FFT plan differs from DESIGN.md 3.2.1", M, N, batch, plan)
    return plan


# ---------------------------------------------------------------------------------------------------------------------
# 0. the plans the library reports reach every class
# ---------------------------------------------------------------------------------------------------------------------
def test_reported_plans_reach_every_class(ctx):
    rep = lambda M, N: ctx.fft_plan(M, N, 1)
    fc.assert_coverage(fc.pow2_shapes(), rep, fc.pow2_required())
    fc.assert_coverage(fc.operator_shapes(rep), rep, fc.pow2_required())
    assert [s[:2] for s in fc.operator_shapes(rep)] == [s[:2] for s in fc.operator_shapes()]
    fc.assert_coverage(fc.chirp_shapes(), rep, fc.CHIRP_REQUIRED)
    for M, N, _ in fc.pow2_shapes() + fc.chirp_shapes():
        reported(ctx, M, N)
    for M, N, B, _, _ in fc.tap_shapes():
        reported(ctx, M, N, B)
    for M in fc.WAVE_SIZES:
        for N in fc.WAVE_SIZES:
            assert reported(ctx, M, N, 3)["fold"] and reported(ctx, M, N)["step_ok"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. all 81 power-of-two pairs: transforms and closures
# ---------------------------------------------------------------------------------------------------------------------
def closures_case(ctx, M, N, kinds, taille=7):
    """rfft2 (packed format only), A / AT / invLS per tap family, A(delta), A(const), adjoint identity."""
    import sbtv
    plan = reported(ctx, M, N)
    bars = closure_bars(M, N, plan)
    where = "%dx%d" % (M, N)
    rng = np.random.default_rng(M * 7 + N)
    x = rng.uniform(0, 255, (M, N))
    t = min(taille, M, N)
    fams = [sbtv.psf_family(k, t, p) for k, p in kinds]
    X = {}
    H = {}
    for dt in (LD, np.float64):
        X[dt] = scipy.fft.fft2(x.astype(dt))
        for i in range(0, len(fams), 2):
            j = min(i + 1, len(fams) - 1)
            H[dt, i], H[dt, j] = fft2_pair(pad(fams[i][0], M, N, dt), pad(fams[j][0], M, N, dt), dt)
    if not plan["generic"]:
        xn = rng.standard_normal((M, N))
        raw = sbtv.rfft2_packed(xn[None])
        U = sbtv.unpack_half_spectrum(raw, M, N)[0]
        ref = scipy.fft.fft2(xn.astype(LD))[:M // 2 + 1]
        check("rfft2 / sqrt(MN)", np.max(np.abs(U.astype(np.clongdouble) - ref)) / np.sqrt(M * N), 5e-14 * np.log2(M * N), where)
        back = sbtv.rfft2_packed(np.transpose(raw, (0, 2, 1)), inverse=True)
        check("rfft2 round trip", err(np.transpose(back, (0, 2, 1))[0], xn.astype(LD)), 1e-13 * np.log2(M * N), where)
    mu = MU0
    for i, (taps, dtaps) in enumerate(fams):
        op = sbtv.BlurOperator(taps)
        a, at = ifft2_pair(H[LD, i] * X[LD], np.conj(H[LD, i]) * X[LD])
        check("A", err(op.A(x), a), bars["A"], where)
        check("AT", err(op.AT(x), at), bars["A"], where)
        if i == 0:
            D0 = scipy.fft.fft2(pad(dtaps[0], M, N, LD))
            check("dA", err(sbtv.BlurOperator(dtaps[0]).A(x), scipy.fft.ifft2(D0 * X[LD]).real), bars["dA"], where)
        ls = scipy.fft.ifft2(X[LD] / (np.abs(H[LD, i]) ** 2 + LD(mu))).real
        check("invLS (relative)", err(op.invLS(x, mu), ls) / float(np.max(np.abs(ls))), bars["invLS"], where)
        # the float64 restatement stays well inside the existing bars: the reference is not what a bar measures
        a64 = scipy.fft.ifft2(H[np.float64, i] * X[np.float64]).real
        assert err(a64, a) < bars["A"] / 16
    op = sbtv.BlurOperator(fams[-1][0])
    dl = np.zeros((M, N))
    dl[0, 0] = 1
    check("A(delta) = taps", np.max(np.abs(op.A(dl)[:t, :t] - fams[-1][0])), bars["delta"], where)
    check("A(const) = const", np.max(np.abs(op.A(np.full((M, N), 2.5)) - 2.5)), bars["const"], where)
    z = rng.standard_normal((M, N))
    lhs, rhs = np.sum(op.A(x).astype(LD) * z), np.sum(x * op.AT(z).astype(LD))
    check("adjoint identity (relative)", abs(lhs - rhs) / abs(rhs), bars["adjoint"], where)
    return x, fams


@pytest.mark.parametrize("M,N", fc.POW2_PAIRS, ids=lambda v: str(v))
def test_pow2_transforms_and_closures(ctx, M, N):
    import sbtv
    x, fams = closures_case(ctx, M, N, KINDS)
    # a batch of three images with per-image taps: image k is computed exactly like image k alone
    rng = np.random.default_rng(N * 7 + M)
    xb = np.stack([x, rng.uniform(0, 255, (M, N)), rng.uniform(0, 255, (M, N))])
    tb = np.stack([f[0] for f in fams])
    for mode, mu in ((1, None), (2, None), (9, [MU0, 2 * MU0, 3 * MU0])):
        got = sbtv.BlurOperator(tb).apply(xb, mode, mu)
        for k in range(3):
            alone = sbtv.BlurOperator(tb[k]).apply(xb[k], mode, None if mu is None else mu[k])
            assert np.array_equal(got[k], alone), "image %d of a batch differs from the image alone (mode %d)" % (k, mode)


# ---------------------------------------------------------------------------------------------------------------------
# 2. + 3. every operator and every column epilogue
# ---------------------------------------------------------------------------------------------------------------------
def pass_args(d, op):
    kw = dict(op=op, taps=d["taps"], mu=d["mu"])
    if op in OPS_WITH_ADD:
        kw["add"] = d["add"]
    if op in ("salsa", "resid", "grad", "gradf", "csalsa"):
        kw["y"] = d["y"]
    if op == "grad":
        kw.update(d1taps=d["d1"], d2taps=d["d2"])
    if op == "csalsa":
        kw.update(cs=CS, e0=d["e0"], repeats=2)
    return kw


def operators_case(ctx, M, N, ops):
    plan = reported(ctx, M, N)
    where = "%dx%d" % (M, N)
    bars = closure_bars(M, N, plan)
    d = sweep_inputs(M, N)
    ref, r64 = operator_reference(d, LD, ops), operator_reference(d, np.float64, ops)
    results = {}
    for op in ops:
        tv = op in OPS_PLAIN and plan["tv_ok"]
        r = ctx.spectral_pass(d["x"], tv=tv, **pass_args(d, op))
        results[op] = r
        x = r["x"][0]
        if op in ("mul_h", "mul_hc"):
            check("OP_%s x" % op.upper(), err(x, ref[op]["x"]), bars["A"], where)
        elif op == "invls":
            check("OP_INVLS x (relative)", err(x, ref[op]["x"]) / float(np.max(np.abs(ref[op]["x"]))), bars["invLS"], where)
        else:
            check("OP_%s x" % op.upper(), err(x, ref[op]["x"]), new_bar(ref[op]["x"], r64[op]["x"], M, N, plan), where)
        for k in range(3):
            a_ref = ref[op]["acc"][k]
            if a_ref == 0:
                assert r["acc"][0, k] == 0.0, (op, k, where)
                continue
            b = new_bar(np.array([a_ref]), np.array([r64[op]["acc"][k]]), M, N, plan)
            check("OP_%s acc%d (relative)" % (op.upper(), k), abs(LD(r["acc"][0, k]) / LD(M * N) - a_ref) / abs(a_ref),
                  b / abs(float(a_ref)), where)
        if tv:
            t_ref, t64 = tvnorm(d["x"].astype(LD)), tvnorm(d["x"])
            check("forward TV (relative)", abs(LD(r["tv"][0]) - t_ref) / t_ref,
                  new_bar(np.array([t_ref]), np.array([t64]), M, N, plan) / float(t_ref), where)
    return plan, d, ref, r64, results


def check_bookkeeping(got, x_ref, x_64, d, M, N, plan, where, tag, tru, xprev, bu=None):
    bk, b64 = bookkeeping_reference(x_ref, d, LD, tru, xprev, bu), bookkeeping_reference(x_64, d, np.float64, tru, xprev, bu)
    for k in ("bu", "g"):
        check("bookkeeping %s" % k, err(got[k][0], bk[k]), new_bar(bk[k], b64[k], M, N, plan), where + tag)
    for i, name in enumerate(("(x-true)^2", "(x-u)^2", "x^2", "u^2", "(x-xprev)^2", "TV(u)")):
        if bk["sums"][i] == 0:
            assert got["sums"][0, i] == 0.0, (name, where, tag)
            continue
        b = new_bar(bk["sums"][i:i + 1], b64["sums"][i:i + 1], M, N, plan)
        check("bookkeeping sum %s (relative)" % name, abs(LD(got["sums"][0, i]) - bk["sums"][i]) / bk["sums"][i],
              b / float(bk["sums"][i]), where + tag)


def epilogues_case(ctx, M, N, plan, d, ref, r64, results):
    """The column epilogues on the x of OP_SALSA (with `add`, as the SALSA loop runs it)."""
    where = "%dx%d" % (M, N)
    x_ref, x_64 = ref["salsa"]["x"], r64["salsa"]["x"]
    kw = pass_args(d, "salsa")
    single = {}
    for tag, tru, xprev in ((" tru xprev", True, True), (" bare", False, False)):
        r = ctx.spectral_pass(d["x"], epilogue="post", u=d["u"], bu=d["bu"], tru=d["tru"] if tru else None,
                              xprev=d["xprev"] if xprev else None, **kw)
        assert np.array_equal(r["acc"], results["salsa"]["acc"])
        check("OP_SALSA x", err(r["x"][0], x_ref), new_bar(x_ref, x_64, M, N, plan), where + tag)
        check_bookkeeping(r, x_ref, x_64, d, M, N, plan, where, tag, tru, xprev)
        single[tag] = r
    if plan["step_ok"]:
        bar = new_bar(x_ref, x_64, M, N, plan)
        r = ctx.spectral_pass(d["x"], epilogue="step", ystep=d["u"], alpha=0.37, **kw)
        check("step y - alpha x", err(r["ystep"][0], d["u"].astype(LD) - LD(0.37) * x_ref), bar, where)
        r = ctx.spectral_pass(d["x"], epilogue="sub", sub_b=d["bu"], **kw)
        check("OP_SALSA x", err(r["x"][0], x_ref), bar, where + " sub")
        check("sub g = x - b", err(r["g"][0], x_ref - d["bu"].astype(LD)), bar, where)
        for tag, tru in ((" skip_x tru", True), (" skip_x", False)):
            r = ctx.spectral_pass(d["x"], epilogue="post_skip_x", u=d["u"], bu=np.zeros((M, N)), bu_in=d["bu"],
                                  tru=d["tru"] if tru else None, **kw)
            check_bookkeeping(r, x_ref, x_64, d, M, N, plan, where, tag, tru, False)
    return single[" bare"]


def batch_case(ctx, M, N, d, results, bare):
    """shared_spec with a batch, and a frozen image: bit for bit the single-image results; the frozen image untouched."""
    d2 = sweep_inputs(M, N, seed=77)
    xb = np.stack([d["x"], d2["y"], d2["x"]])
    addb = np.stack([d["add"], d2["add"], d2["add"]])
    ub, bub = np.stack([d["u"], d2["u"], d2["u"]]), np.stack([d["bu"], d2["bu"], d2["bu"]])
    kw = pass_args(d, "salsa")
    kw.pop("add")
    last = ctx.spectral_pass(d2["x"], epilogue="post", add=d2["add"], u=d2["u"], bu=d2["bu"], **kw)
    mid = ctx.spectral_pass(d2["y"], epilogue="post", add=d2["add"], u=d2["u"], bu=d2["bu"], **kw)
    sh = ctx.spectral_pass(xb, epilogue="post", add=addb, u=ub, bu=bub, tru=None, shared_spec=True, **kw)
    kw3 = dict(kw, taps=np.stack([d["taps"]] * 3), y=np.stack([d["y"]] * 3))
    fz = ctx.spectral_pass(xb, epilogue="post", add=addb, u=ub, bu=bub, frozen=[0, 1, 0], sentinel=SENTINEL, **kw3)
    for r, name in ((sh, "shared_spec"), (fz, "frozen")):
        for k, one in ((0, bare), (2, last)):
            for q in ("x", "bu", "g", "acc", "sums"):
                assert np.array_equal(r[q][k], one[q][0]), "%s: %s of image %d differs from the image alone" % (name, q, k)
    for q in ("x", "bu", "g", "acc", "sums"):
        assert np.array_equal(sh[q][1], mid[q][0]), "shared_spec: %s of image 1 differs from the image alone" % q
    assert np.all(fz["x"][1] == SENTINEL) and np.all(fz["g"][1] == SENTINEL) and np.array_equal(fz["bu"][1], d2["bu"])
    assert np.all(fz["acc"][1] == 0) and np.all(fz["sums"][1] == 0)
    # a frozen image under shared spectra (on the wave plans: inside the folded grid), with the plain inverse
    kwh = pass_args(d, "mul_hc")
    ones = [ctx.spectral_pass(xk, **kwh) for xk in (xb[0], xb[2])]
    fs = ctx.spectral_pass(xb, shared_spec=True, frozen=[0, 1, 0], sentinel=SENTINEL, **kwh)
    assert np.all(fs["x"][1] == SENTINEL)
    for k, one in ((0, ones[0]), (2, ones[1])):
        assert np.array_equal(fs["x"][k], one["x"][0]), "shared_spec + frozen: x of image %d differs from the image alone" % k
    fsp = ctx.spectral_pass(xb, epilogue="post", add=addb, u=ub, bu=bub, shared_spec=True, frozen=[1, 0, 1], sentinel=SENTINEL, **kw)
    assert np.all(fsp["x"][[0, 2]] == SENTINEL) and np.all(fsp["g"][[0, 2]] == SENTINEL) and np.all(fsp["sums"][[0, 2]] == 0)
    assert np.array_equal(fsp["bu"][0], d["bu"]) and np.array_equal(fsp["bu"][2], d2["bu"])
    for q in ("x", "bu", "g", "acc", "sums"):
        assert np.array_equal(fsp[q][1], mid[q][0]), "shared_spec + frozen: %s of image 1 differs from the image alone" % q
    if ctx.fft_plan(M, N)["step_ok"]:
        # the step epilogue skips a frozen image: its ystep is left as it was
        st = [ctx.spectral_pass(xk, epilogue="step", ystep=uk, alpha=0.37, add=ak, **kw)
              for xk, uk, ak in ((xb[0], ub[0], addb[0]), (xb[2], ub[2], addb[2]))]
        fst = ctx.spectral_pass(xb, epilogue="step", ystep=ub, alpha=0.37, add=addb, frozen=[0, 1, 0], **kw3)
        assert np.array_equal(fst["ystep"][1], ub[1])
        assert np.array_equal(fst["ystep"][0], st[0]["ystep"][0]) and np.array_equal(fst["ystep"][2], st[1]["ystep"][0])
    # OP_GRAD with all four spectra shared
    kwg = pass_args(d, "grad")
    g = ctx.spectral_pass(xb, shared_spec=True, **kwg)
    assert np.array_equal(g["x"][0], results["grad"]["x"][0]) and np.array_equal(g["acc"][0], results["grad"]["acc"][0])
    for k, xk in ((1, d2["y"]), (2, d2["x"])):
        g2 = ctx.spectral_pass(xk, **kwg)
        assert np.array_equal(g["x"][k], g2["x"][0]) and np.array_equal(g["acc"][k], g2["acc"][0])


ALL_OPS = OPS_PLAIN + OPS_WITH_ADD


@pytest.mark.parametrize("M,N", [s[:2] for s in fc.operator_shapes()], ids=lambda v: str(v))
def test_pow2_operators_and_epilogues(ctx, M, N):
    plan, d, ref, r64, results = operators_case(ctx, M, N, ALL_OPS)
    single = epilogues_case(ctx, M, N, plan, d, ref, r64, results)
    batch_case(ctx, M, N, d, results, single)


# ---------------------------------------------------------------------------------------------------------------------
# 4. tap sizes against the spatial circular sum
# ---------------------------------------------------------------------------------------------------------------------
def exact_taps_case(rng, M, N, B, t):
    """Integer pixels and dyadic taps: every product and partial sum of the spatial circular sum is exact in float64, so
    the plain double loop IS the infinitely precise value."""
    x = rng.integers(0, 256, (B, M, N)).astype(np.float64)
    sh = int(np.ceil(np.log2(16 * t * t)))
    taps = rng.integers(0, 16, (B, t, t)).astype(np.float64) / 2.0 ** sh
    ref = np.zeros((B, M, N))
    for m in range(t):
        for n in range(t):
            ref += taps[:, m, n][:, None, None] * np.roll(x, (m, n), axis=(1, 2))
    return x, taps, ref


@pytest.mark.parametrize("M,N,B,tailles", [s[:4] for s in fc.tap_shapes()], ids=lambda v: str(v).replace(" ", ""))
def test_tap_sizes_against_the_spatial_sum(ctx, M, N, B, tailles):
    import sbtv
    plan = reported(ctx, M, N, B)
    bar = closure_bars(M, N, plan)["A"]
    rng = np.random.default_rng(M + 3 * N + B)
    for t in tailles:
        x, taps, ref = exact_taps_case(rng, M, N, B, t)
        got = sbtv.BlurOperator(taps).A(x)
        check("A, taille 1..15, against the spatial sum", np.max(np.abs(got - ref)), bar, "%dx%dx%d taille %d" % (M, N, B, t))


# ---------------------------------------------------------------------------------------------------------------------
# 5. chirp-z
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [s[:2] for s in fc.chirp_shapes()], ids=lambda v: str(v))
def test_chirpz_closures_operators_and_bookkeeping(ctx, M, N):
    import sbtv
    x, fams = closures_case(ctx, M, N, KINDS[:2])
    plan = reported(ctx, M, N)
    t = fams[0][0].shape[0]
    # a batch of two images with their own taps
    rng = np.random.default_rng(M * 31 + N)
    xb = np.stack([x, rng.uniform(0, 255, (M, N))])
    tb = np.stack([fams[0][0], fams[1][0]])
    got = sbtv.BlurOperator(tb).A(xb)
    for k in range(2):
        assert np.array_equal(got[k], sbtv.BlurOperator(tb[k]).A(xb[k]))
    ops = tuple(o for o in ALL_OPS if o != "csalsa")
    plan, d, ref, r64, results = operators_case(ctx, M, N, ops)
    epilogues_case(ctx, M, N, plan, d, ref, r64, results)
    with pytest.raises(sbtv.SbtvError) as e:
        ctx.spectral_pass(d["x"], **pass_args(d, "csalsa"))
    assert e.value.code == -2 and "OP_CSALSA" in e.value.msg


def test_conv2c_diffh_diffv_at_a_chirpz_size(ctx):
    import sbtv
    import sbtv_oracle as o
    from conftest import synth_image
    x = synth_image(30, 50, 4)
    h = np.random.default_rng(1).standard_normal((4, 6))
    np.testing.assert_allclose(sbtv.conv2c(x, h), o.conv2c(x, h), rtol=0, atol=5e-10)
    np.testing.assert_allclose(sbtv.diffh(x), x - np.roll(x, 1, axis=1), rtol=0, atol=1e-10)
    np.testing.assert_allclose(sbtv.diffv(x), x - np.roll(x, 1, axis=0), rtol=0, atol=1e-10)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the A/B switches, each in a fresh child process
# ---------------------------------------------------------------------------------------------------------------------
WAVE_SHAPES = tuple((M, N) for M in fc.WAVE_SIZES for N in fc.WAVE_SIZES)
SWITCH_OPS = ("mul_h", "salsa", "grad", "csalsa")


def normal_image(M, N):
    return np.random.default_rng(M * 7 + N).standard_normal((M, N))


def switch_runs(ctx, M, N):
    """What a child computes per wave-plan shape: {name: array}."""
    import sbtv
    d = sweep_inputs(M, N)
    out = {}
    raw = sbtv.rfft2_packed(normal_image(M, N)[None], ctx=ctx)
    out["rfft2"] = sbtv.unpack_half_spectrum(raw, M, N)[0]
    for op in SWITCH_OPS:
        r = ctx.spectral_pass(d["x"], tv=op in OPS_PLAIN, **pass_args(d, op))
        out[op + ".x"], out[op + ".acc"] = r["x"][0], r["acc"][0]
        if "tv" in r:
            out[op + ".tv"] = r["tv"]
    kw = pass_args(d, "salsa")
    r = ctx.spectral_pass(d["x"], epilogue="post", u=d["u"], bu=d["bu"], tru=d["tru"], xprev=d["xprev"], **kw)
    out.update({"post." + k: r[k][0] for k in ("x", "bu", "g", "sums")})
    d2 = sweep_inputs(M, N, seed=77)
    xb = np.stack([d["x"], d2["y"], d2["x"]])
    for op in ("salsa", "grad"):
        kw = pass_args(d, op)
        kw.pop("add", None)
        r = ctx.spectral_pass(xb, shared_spec=True, **kw)
        out["shared." + op + ".x"], out["shared." + op + ".acc"] = r["x"], r["acc"]
    return out


def run_child(tmp_path, name, env):
    path = str(tmp_path / (name + ".npz"))
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fft_sweep_child.py")
    # a fresh process with its own time limit; a child that fails ends the test here, nothing is retried
    p = subprocess.run([sys.executable, child, path], env=dict(os.environ, **env), timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, "child %s failed (%d):\n%s" % (name, p.returncode, p.stderr[-3000:])
    return dict(np.load(path))


def test_switches_in_child_processes(ctx, tmp_path):
    assert not os.environ.get("SBTV_FFT_WAVE") and not os.environ.get("SBTV_ROWS_FOLD")
    nowave = run_child(tmp_path, "nowave", {"SBTV_FFT_WAVE": "0"})
    nofold = run_child(tmp_path, "nofold", {"SBTV_ROWS_FOLD": "0"})
    for M, N in WAVE_SHAPES:
        plan = reported(ctx, M, N)
        where = "%dx%d" % (M, N)
        here = switch_runs(ctx, M, N)
        pre = where + "."
        # fold on and fold off: the same workgroups on the same data in another order
        for k, v in here.items():
            assert np.array_equal(v, nofold[pre + k]), "SBTV_ROWS_FOLD=0 changes %s at %s" % (k, where)
        d = sweep_inputs(M, N)
        ref, r64 = operator_reference(d, LD, SWITCH_OPS), operator_reference(d, np.float64, SWITCH_OPS)
        bars = closure_bars(M, N, plan)
        d2 = sweep_inputs(M, N, seed=77)
        # the shared-spectrum batch: image 0 is the single image without `add`, image 2 against its own reference
        dd = dict(d, x=d2["x"], add=np.zeros((M, N)))
        rr, rr64 = operator_reference(dd, LD, ("salsa", "grad")), operator_reference(dd, np.float64, ("salsa", "grad"))
        F = scipy.fft.fft2(normal_image(M, N).astype(LD))[:M // 2 + 1]
        for tag, res in ((" SBTV_FFT_WAVE=0", nowave), (" SBTV_ROWS_FOLD=0", nofold)):
            w = where + tag
            check("rfft2 / sqrt(MN)", np.max(np.abs(res[pre + "rfft2"].astype(np.clongdouble) - F)) / np.sqrt(M * N),
                  5e-14 * np.log2(M * N), w)
            for op in SWITCH_OPS:
                x = res[pre + op + ".x"]
                if op == "mul_h":
                    check("OP_MUL_H x", err(x, ref[op]["x"]), bars["A"], w)
                else:
                    check("OP_%s x" % op.upper(), err(x, ref[op]["x"]), new_bar(ref[op]["x"], r64[op]["x"], M, N, plan), w)
                for k in range(3):
                    a_ref = ref[op]["acc"][k]
                    if a_ref != 0:
                        b = new_bar(np.array([a_ref]), np.array([r64[op]["acc"][k]]), M, N, plan)
                        check("OP_%s acc%d (relative)" % (op.upper(), k),
                              abs(LD(res[pre + op + ".acc"][k]) / LD(M * N) - a_ref) / abs(a_ref), b / abs(float(a_ref)), w)
            t_ref = tvnorm(d["x"].astype(LD))
            check("forward TV (relative)", abs(LD(res[pre + "grad.tv"][0]) - t_ref) / t_ref,
                  new_bar(np.array([t_ref]), np.array([tvnorm(d["x"])]), M, N, plan) / float(t_ref), w)
            got = {k: res[pre + "post." + k][None] for k in ("x", "bu", "g", "sums")}
            check_bookkeeping(got, ref["salsa"]["x"], r64["salsa"]["x"], d, M, N, plan, where, tag, True, True)
            for op in ("salsa", "grad"):
                check("OP_%s x" % op.upper(), err(res[pre + "shared." + op + ".x"][2], rr[op]["x"]),
                      new_bar(rr[op]["x"], rr64[op]["x"], M, N, plan), w + " shared")
                b = new_bar(rr[op]["acc"][:1], rr64[op]["acc"][:1], M, N, plan)
                check("OP_%s acc0 (relative)" % op.upper(),
                      abs(LD(res[pre + "shared." + op + ".acc"][2, 0]) / LD(M * N) - rr[op]["acc"][0]) / rr[op]["acc"][0],
                      b / float(rr[op]["acc"][0]), w + " shared")


# ---------------------------------------------------------------------------------------------------------------------
# 7. error paths that end on the host
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_end_on_the_host(ctx):
    import sbtv
    taps = sbtv.Gaussian_psf(7, 0.4, 0.3)
    A = sbtv.BlurOperator(taps)

    def refused(code, fn, *a, **k):
        with pytest.raises(sbtv.SbtvError) as e:
            fn(*a, **k)
        assert e.value.code == code, (e.value.code, code, e.value.msg)

    refused(-2, sbtv.rfft2_packed, np.zeros((48, 64)))                 # the packed format is a power-of-two format
    refused(-2, sbtv.rfft2_packed, np.zeros((8, 8)))
    refused(-2, A, np.zeros((4097, 16)))
    refused(-2, A, np.zeros((16, 4097)))
    refused(-2, ctx.fft_plan, 4097, 16)
    refused(-2, ctx.fft_plan, 16, 1)
    refused(-10, A, np.zeros((6, 64)))                                 # taille larger than M
    refused(-10, A, np.zeros((64, 6)))
    d = sweep_inputs(64, 32)
    refused(-10, ctx.spectral_pass, np.zeros((6, 64)), op="mul_h", taps=taps)
    refused(-2, ctx.spectral_pass, np.zeros((48, 64)), **pass_args(sweep_inputs(48, 64), "csalsa"))
    kw = pass_args(d, "salsa")
    refused(-1, ctx.spectral_pass, d["x"], epilogue="step", ystep=d["u"], alpha=0.5, **kw)
    refused(-1, ctx.spectral_pass, d["x"], epilogue="sub", sub_b=d["bu"], **kw)
    refused(-1, ctx.spectral_pass, d["x"], epilogue="post_skip_x", u=d["u"], bu=d["bu"], bu_in=d["bu"], **kw)
    refused(-1, ctx.spectral_pass, d["x"], tv=True, **kw)              # the forward TV does not go with `add`
    refused(-1, ctx.spectral_pass, np.zeros((48, 64)), op="none", tv=True)
    refused(-1, ctx.spectral_pass, d["x"], op=11)
    refused(-1, ctx.spectral_pass, d["x"], op="grad", taps=taps, y=d["y"])          # no derivative taps
    refused(-9, ctx.spectral_pass, d["x"], op="salsa", taps=taps, y=d["y"])         # no mu
    dw = sweep_inputs(1024, 1024)
    refused(-1, ctx.spectral_pass, dw["x"], epilogue="post_skip_x", u=dw["u"], bu=dw["bu"], bu_in=dw["bu"],
            xprev=dw["xprev"], **pass_args(dw, "salsa"))                # skip_x takes no xprev
