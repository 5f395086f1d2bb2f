"""Image sizes that reach every plan class of the FFT passes, derived from plan reports.

Plain Python, no GPU.  A report is the dict `Context.fft_plan` returns (generic, wave, n1, cols_per_wg, cols_threads,
cols_wgs, rows_per_wg, rows_threads, rows_wgs, rows_kind, u_tiled, L_M, L_N, lch, fold, tv_ok, step_ok, csalsa_ok); the
functions below turn reports into lists of `(M, N, why)` and name the CLASS of kernel specialisations a report stands
for.  `model_plan` restates the host functions of csrc/fft.hip for today's constants: it is there to
enumerate shapes where no GPU is present (test collection, the CPU test) and to PROVE that the lists cover the classes
(`coverage`, `assert_coverage`); it never produces an expected value of a transform - those come from the long-double
reference of tests/test_gpu_fft_sweep.py.  The GPU module checks the reports of the library against it before it
launches anything.
"""

POW2 = tuple(1 << k for k in range(4, 13))                      # 16 .. 4096
POW2_PAIRS = tuple((M, N) for M in POW2 for N in POW2)          # all 81
WAVE_SIZES = (1024, 2048)
COLS_THREADS = 256

# the documented classes: what a sweep over the powers of two has to reach
COL_INSTANTIATIONS = tuple(range(3, 12))                        # log2(n1), M = 16 .. 4096
ROW_INSTANTIATIONS = ((4, 8), (5, 8), (6, 8), (7, 8), (8, 2), (8, 8), (9, 1), (9, 4), (10, 4), (11, 4), (12, 2))
WAVE_PLANS = tuple((M // 2, N) for M in WAVE_SIZES for N in WAVE_SIZES)


def is_pow2(v):
    return v > 0 and v & (v - 1) == 0


def bluestein_len(n):
    L = 1
    while L < 2 * n - 1:
        L <<= 1
    return L


def model_plan(M, N, batch=1, wave_enabled=True):
    """The report the library gives for today's constants (csrc/fft.hip: fft_plan, cols_nseq, rows_rk, fft_rows_blocks,
    fft_cols_blocks, psf_lch, rows_fold_ok; csrc/fft_any.inc: any_axis_len)."""
    if not (2 <= M <= 4096 and 2 <= N <= 4096):
        raise ValueError("blur operator: 2 <= M, N <= 4096")
    if not (is_pow2(M) and is_pow2(N) and M >= 16 and N >= 16):
        return dict(generic=True, wave=False, n1=M, cols_per_wg=1, cols_threads=256, cols_wgs=N, rows_per_wg=0,
                    rows_threads=256, rows_wgs=256, rows_kind="pointwise", u_tiled=False, L_M=bluestein_len(M),
                    L_N=bluestein_len(N), lch=0, fold=False, tv_ok=False, step_ok=False, csalsa_ok=False)
    n1 = M // 2
    lch = min(16, max(1, ((n1 + 1) * N * batch) >> 19))
    if wave_enabled and M in WAVE_SIZES and N in WAVE_SIZES:
        return dict(generic=False, wave=True, n1=n1, cols_per_wg=4, cols_threads=256, cols_wgs=N // 4, rows_per_wg=4,
                    rows_threads=N // 4, rows_wgs=n1 // 4, rows_kind="pipelined", u_tiled=True, L_M=0, L_N=0, lch=lch,
                    fold=batch > 1 and (n1 // 4) % 8 == 0, tv_ok=True, step_ok=True, csalsa_ok=True)
    T = n1 // 8
    nseq = min(max(COLS_THREADS // T, 1), N)
    while nseq > 1 and (nseq // 2) * T >= 64 and N // nseq < 256:
        nseq >>= 1
    if N == 4096:
        rk = 2
    else:
        rk = 4 if N >= 512 else 8
        small = 1 if N == 512 else 2 if N == 256 else rk
        rk = small if n1 // rk < 128 else rk
    return dict(generic=False, wave=False, n1=n1, cols_per_wg=nseq, cols_threads=nseq * T, cols_wgs=N // nseq,
                rows_per_wg=rk, rows_threads=rk * (N // 8), rows_wgs=n1 // rk, rows_kind="workgroup", u_tiled=False,
                L_M=0, L_N=0, lch=lch, fold=False, tv_ok=True, step_ok=False, csalsa_ok=True)


def ilog2(v):
    return v.bit_length() - 1


def classes(M, N, plan):
    """The kernel specialisations a report stands for, as a set of (kind, value) names.  Everything is read from the
    REPORT (n1, the workgroup shapes), not from M and N, except the transform length of the row pass, which is N."""
    if plan["generic"]:
        out = {("chirp", "L_M=%d" % plan["L_M"]), ("chirp", "L_N=%d" % plan["L_N"])}
        for L in (plan["L_M"], plan["L_N"]):
            out.add(("chirp lds", "128 KB" if L == 8192 else "64 KB exactly" if L == 4096 else "below 64 KB"))
            if L < 2 * 256:
                out.add(("chirp", "fewer butterflies than threads"))
        return out
    out = {("lch", ">1" if plan["lch"] > 1 else "1")}
    if plan["wave"]:
        out.add(("wave", (plan["n1"], N)))
        return out
    out.add(("cols", ilog2(plan["n1"])))
    out.add(("PREP", plan["n1"] <= 256))                        # fft_cols_inv_kernel: POST && LOG2N <= 8
    out.add(("rows", (ilog2(N), plan["rows_per_wg"])))
    out.add(("PRE", plan["rows_threads"] <= 256))               # fft_rows_kernel: RK * N / 8 <= 256
    if plan["rows_threads"] < 64:
        out.add(("partial wave", True))
    return out


def pow2_required():
    """Every class the 81 power-of-two pairs have to reach."""
    req = {("cols", L) for L in COL_INSTANTIATIONS} | {("rows", r) for r in ROW_INSTANTIATIONS}
    req |= {("PREP", True), ("PREP", False), ("PRE", True), ("PRE", False), ("partial wave", True)}
    req |= {("wave", w) for w in WAVE_PLANS} | {("lch", "1"), ("lch", ">1")}
    return req


CHIRP_REQUIRED = {("chirp lds", "128 KB"), ("chirp lds", "64 KB exactly"), ("chirp lds", "below 64 KB"),
                  ("chirp", "fewer butterflies than threads"), ("chirp", "L_M=4"), ("chirp", "L_N=4"),
                  ("chirp", "L_M=8"), ("chirp", "L_N=8"), ("chirp", "L_M=8192"), ("chirp", "L_N=8192"),
                  ("chirp", "L_M=4096"), ("chirp", "L_N=4096")}


def coverage(shapes, report):
    """{class: [shapes]} for shapes [(M, N, ...)] and `report(M, N)` -> plan dict."""
    cov = {}
    for s in shapes:
        M, N = s[0], s[1]
        for c in classes(M, N, report(M, N)):
            cov.setdefault(c, []).append((M, N))
    return cov


def assert_coverage(shapes, report, required):
    cov = coverage(shapes, report)
    missing = sorted(c for c in required if not cov.get(c))
    assert not missing, "no shape reaches %s" % (missing,)
    return cov


def pow2_shapes():
    return [(M, N, "power of two") for M, N in POW2_PAIRS]


OPERATOR_PIXELS = 1 << 20


def operator_shapes(report=model_plan):
    """Shapes every spectral operator and column epilogue runs at: every power-of-two pair of at most 2^20 pixels, and
    above that one pair per DISTINCT plan report (today every larger pair has a report of its own: n1, the workgroup
    counts and lch all differ, so all ten run and the list is the 81 pairs)."""
    out = [(M, N, "<= 2^20 pixels") for M, N in POW2_PAIRS if M * N <= OPERATOR_PIXELS]
    seen = set()
    for M, N in POW2_PAIRS:
        if M * N > OPERATOR_PIXELS:
            key = tuple(sorted(report(M, N).items()))
            if key not in seen:
                seen.add(key)
                out.append((M, N, "above 2^20 pixels: a plan report of its own"))
    return out


# chirp-z: the classes of ONE axis
AXIS_CLASSES = ((2, "n = 2: L = 4"), (3, "n = 3: L = 8"), (7, "n = 7: the tap array fills the axis"),
                (8, "a power of two below 16"), (32, "2^k, small: L = 64"), (33, "2^k + 1, small: L = 128"),
                (1024, "2^k, large: L = 2048"), (1025, "2^k + 1, large: L = 4096"),
                (2048, "L = 4096: exactly 64 KB of LDS"), (2049, "the first L = 8192: 128 KB of LDS"),
                (4093, "prime"), (4095, "the largest odd size"), (4096, "4096 beside a size that is not a power of two"))
GENERIC_WIDTH, GENERIC_HEIGHT = 50, 60
CHIRP_CORNERS = ((2, 2), (2, 4096), (4096, 2), (7, 4095), (4095, 7), (2049, 2049), (4095, 4093))


def chirp_shapes():
    """[(M, N, why)]: every axis class on the rows against one generic width, on the columns against one generic
    height, and the corners.  No duplicates; odd x odd, odd x even and even x odd all occur."""
    out, seen = [], set()
    for M, N, why in ([(n, GENERIC_WIDTH, "M: " + w) for n, w in AXIS_CLASSES]
                      + [(GENERIC_HEIGHT, n, "N: " + w) for n, w in AXIS_CLASSES]
                      + [(M, N, "corner") for M, N in CHIRP_CORNERS] + [(33, 4093, "odd x odd away from the corners")]):
        if (M, N) not in seen:
            seen.add((M, N))
            out.append((M, N, why))
    return out


def tap_shapes():
    """[(M, N, batch, tailles, why)] of the tap-size sweep."""
    out = [(16, 16, 1, tuple(range(1, 16)), "the smallest power-of-two plan"),
           (15, 4096, 1, tuple(range(1, 16)), "chirp-z rows of 15 beside 4096 columns"),
           (1024, 1024, 1, tuple(range(1, 16)), "a wave plan: tiled tap spectrum"),
           (512, 512, 8, tuple(range(1, 16)), "a batch with lch > 1"),
           (1024, 1024, 2, (1, 7, 8, 15), "a wave-plan batch with lch > 1")]
    out += [(t, t, 1, (t,), "taille x taille: the tap array fills the image") for t in range(2, 16)]
    return out
