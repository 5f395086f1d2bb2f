"""Image sizes that reach every tile-geometry class of the wavelet frame kernels (csrc/wavelet.hip), with the proof.

Plain Python, no GPU.  A geometry is the dict `Context.wavelet_geometry` returns for ONE level (J, s, Q1, Q2, nr1, nr2, T1,
TA2, TS2, tiles1, tilesA2, tilesS2, halo1, halo2, lds_analysis, lds_synthesis).  `model_geometry` restates `wav_geom`,
`wav_tiles` and the constants of csrc/wavelet.hip for today's values: it is there to enumerate sizes where
no GPU is present (test collection, the CPU test) and to PROVE that `CASES` reaches `REQUIRED` (`assert_coverage`); it never
produces an expected value of a transform - those come from the long-double reference of tests/test_gpu_wavelet_sweep.py.
The GPU module asserts model == library for every level of every case before it launches anything, and derives the classes
a second time from the library's reports.

A class is a tuple that starts with the filter length K (each K is an instantiation of its own).  Classes of ONE dimension
are (K, pass, dim, kind, value): pass "A" (analysis) or "S" (synthesis), dim 1 (M, the contiguous index, 64 outputs per
tile) or 2 (N, 32 outputs per analysis tile, 16 per synthesis tile).  With s the stride of a level, Q = min(s, cap) the run,
nr = s / Q the runs per stride, A = T / Q the steps of a tile and steps = ceil(n / s):

  regime   "s<cap", "s=cap", "s=2cap" (two runs per stride), "s>=4cap" (four or more): one per level
  tiling   on a level whose tile is contiguous (nr = 1; level 1 always is): "n<T" (one partly filled tile), "n=T", "n=T+1"
           (a second tile that stores one sample), ">=3 cut" (at least three tiles, the last one cut)
  comb     on a level whose tile is a comb (nr > 1), tagged with its regime: "steps%A" (ceil(n / s) is no multiple of A: the
           last block of steps is cut), "n%s" (the last step is partial: some runs have one step fewer), ">=2 blocks"
           (`wav_base` with a block and a run that are both non-zero)
  wrap     over the tiles of a level that store at least one sample, tagged "contiguous" or "comb".  Analysis loads
           base .. base + (A + K - 2) s + Q - 1: "none" (the last index < n), "once" (in [n, 2n)), "twice" (>= 2n: the `%`
           branch of `wav_wrap` has to remove more than one n).  Synthesis loads base - (K - 1) s .. base + (A - 1) s + Q - 1:
           the same three and "negative" (the `+= n` branch; the first tile always), "interior" (neither branch)
           "twice" is a class of memory safety, not of values: a STORED output i < n reads i + s k < n + (K - 1) s < 2n, so an
           index >= 2n only ever feeds outputs that the store guard discards, and `%` is what keeps their loads inside the
           image.  The sweep runs these sizes (under guard bands too); it cannot tell `%` from any other in-range index there.
  reach    "n-1": (K - 1) 2^(J - 1) = n - 1, every tap of the deepest level wraps; "n=K": the smallest legal size, levels 2

Classes of a whole case: (K, "KxK"), (K, "depth", d, batch) with d in "J=1" (no workspace image), "J=2" (one), "J odd>=3",
"J even>=4" and batch 1 or 3, (K, "parity", (M % 2, N % 2)), (K, "shape", "M<N" | "M>N").

`feasible_dim_classes` enumerates every legal (n, levels) up to MAX_SIDE; REQUIRED is all of it.  What the rules name but
no legal size reaches is listed in UNREACHABLE with the reason, and tests/test_wavelet_geometry_cases_cpu.py checks both
statements by enumeration.
"""

KS = (2, 4, 6, 8)
WT1, WA_T2, WS_T2 = 64, 32, 16                       # csrc/wavelet.hip
CAP1 = {2: 16, 4: 8, 6: 4, 8: 4}                     # wav_cap1
CAP2 = {2: 4, 4: 4, 6: 2, 8: 2}                      # wav_cap2
MAX_SIDE = 320
MAX_CASES = 160
MAX_COEFFICIENTS = 2 * 10 ** 7
PASSES = ("A", "S")
REGIMES = ("s<cap", "s=cap", "s=2cap", "s>=4cap")
DEPTHS = ("J=1", "J=2", "J odd>=3", "J even>=4")


def check(M, N, K, levels):
    """What `wav_plan` refuses."""
    if K not in KS or levels < 2:
        raise ValueError("bad filter length or levels")
    if M < 1 or N < 1 or levels - 1 > 30 or (K - 1) << (levels - 2) >= min(M, N):
        raise ValueError("the image is too small for this depth")


def tiles(n, s, Q, nr, T):
    """`wav_tiles`: blocks of T / Q steps over the ceil(n / s) steps of a run, times the runs of a stride."""
    steps, A = -(-n // s), T // Q
    return -(-steps // A) * nr


def lds_bytes(K):
    """(analysis, synthesis): the __shared__ arrays of the two kernels."""
    L1 = WT1 + CAP1[K] * (K - 1)
    La, Ls = WA_T2 + CAP2[K] * (K - 1), WS_T2 + CAP2[K] * (K - 1)
    return 8 * (La * L1 + 2 * La * WT1), 8 * (2 * Ls * L1 + 2 * WS_T2 * L1)


def model_geometry(M, N, K, levels, level):
    """The report the library gives for today's constants."""
    check(M, N, K, levels)
    J = levels - 1
    if not 1 <= level <= J:
        raise ValueError("level outside 1..J")
    s = 1 << (level - 1)
    Q1, Q2 = min(s, CAP1[K]), min(s, CAP2[K])
    nr1, nr2 = s // Q1, s // Q2
    la, ls = lds_bytes(K)
    return dict(J=J, s=s, Q1=Q1, Q2=Q2, nr1=nr1, nr2=nr2, T1=WT1, TA2=WA_T2, TS2=WS_T2, tiles1=tiles(M, s, Q1, nr1, WT1),
                tilesA2=tiles(N, s, Q2, nr2, WA_T2), tilesS2=tiles(N, s, Q2, nr2, WS_T2), halo1=(K - 1) * Q1,
                halo2=(K - 1) * Q2, lds_analysis=la, lds_synthesis=ls)


def model_report(M, N, K, levels):
    return [model_geometry(M, N, K, levels, j) for j in range(1, levels)]


def level_dim_classes(n, K, ps, dim, s, Q, nr, T, ntiles, cap):
    """Classes of one level, one dimension, one pass, read from the reported numbers (s, Q, nr, T, the tile count)."""
    out = set()
    A, steps = T // Q, -(-n // s)
    assert ntiles == -(-steps // A) * nr, "the reported tile count does not cover the dimension"
    blocks = ntiles // nr
    regime = ("s<cap" if s < cap else "s=cap") if nr == 1 else ("s=2cap" if nr == 2 else "s>=4cap")
    out.add((K, ps, dim, "regime", regime))
    if nr == 1:
        if n < T:
            out.add((K, ps, dim, "tiling", "n<T"))
        if n == T:
            out.add((K, ps, dim, "tiling", "n=T"))
        if n == T + 1:
            out.add((K, ps, dim, "tiling", "n=T+1"))
        if blocks >= 3 and n % T:
            out.add((K, ps, dim, "tiling", ">=3 cut"))
    else:
        if steps % A:
            out.add((K, ps, dim, "comb " + regime, "steps%A"))
        if n % s:
            out.add((K, ps, dim, "comb " + regime, "n%s"))
        if blocks >= 2:
            out.add((K, ps, dim, "comb " + regime, ">=2 blocks"))
    shape = "contiguous" if nr == 1 else "comb"
    for t in range(ntiles):
        blk, run = divmod(t, nr)
        base = blk * A * s + run * Q
        if base >= n:
            continue                                            # stores nothing
        if ps == "A":
            first, last = base, base + (A + K - 2) * s + Q - 1
        else:
            first, last = base - (K - 1) * s, base + (A - 1) * s + Q - 1
            assert first > -n                                   # `wav_wrap` adds n once
        out.add((K, ps, dim, "wrap " + shape, "none" if last < n else "once" if last < 2 * n else "twice"))
        if ps == "S":
            if first < 0:
                out.add((K, ps, dim, "wrap " + shape, "negative"))
            elif last < n:
                out.add((K, ps, dim, "wrap " + shape, "interior"))
    return out


def dim_classes(n, K, levels, dim, report=None):
    """Classes one dimension of n samples reaches over all levels.  `report`: the per-level geometry dicts (the library's or
    the model's); None: the model for an n x n image."""
    if report is None:
        report = model_report(n, n, K, levels)
    cap = (CAP1 if dim == 1 else CAP2)[K]
    out = set()
    for g in report:
        for ps in PASSES:
            if dim == 1:
                Q, nr, T, nt = g["Q1"], g["nr1"], g["T1"], g["tiles1"]
            else:
                Q, nr, T, nt = g["Q2"], g["nr2"], g["TA2" if ps == "A" else "TS2"], g["tilesA2" if ps == "A" else "tilesS2"]
            out |= level_dim_classes(n, K, ps, dim, g["s"], Q, nr, T, nt, cap)
    J = levels - 1
    if (K - 1) << (J - 1) == n - 1:
        out |= {(K, ps, dim, "reach", "n-1") for ps in PASSES}
    if n == K and levels == 2:
        out |= {(K, ps, dim, "reach", "n=K") for ps in PASSES}
    return out


def depth(J):
    return "J=1" if J == 1 else "J=2" if J == 2 else "J odd>=3" if J % 2 else "J even>=4"


def classes(M, N, K, levels, batch=1, report=None):
    """Every class the case ((M, N), K, levels, batch) reaches."""
    check(M, N, K, levels)
    if report is None:
        report = model_report(M, N, K, levels)
    out = dim_classes(M, K, levels, 1, report) | dim_classes(N, K, levels, 2, report)
    out.add((K, "depth", depth(levels - 1), batch))
    out.add((K, "parity", (M % 2, N % 2)))
    if M != N:
        out.add((K, "shape", "M<N" if M < N else "M>N"))
    if M == N == K:
        out.add((K, "KxK"))
    return out


def max_levels(n, K):
    lv = 2
    while (K - 1) << (lv - 1) < n:
        lv += 1
    return lv


def feasible_dim_classes(K, dim, max_side=MAX_SIDE):
    """Every class of one dimension that some legal (n, levels) with n <= max_side reaches."""
    out = set()
    for n in range(K, max_side + 1):
        for levels in range(2, max_levels(n, K) + 1):
            out |= dim_classes(n, K, levels, dim)
    return out


def named_dim_classes(K, dim):
    """Every class the rules of the module docstring can name for one dimension."""
    out = set()
    for ps in PASSES:
        out |= {(K, ps, dim, "regime", r) for r in REGIMES}
        out |= {(K, ps, dim, "tiling", v) for v in ("n<T", "n=T", "n=T+1", ">=3 cut")}
        for r in ("s=2cap", "s>=4cap"):
            out |= {(K, ps, dim, "comb " + r, v) for v in ("steps%A", "n%s", ">=2 blocks")}
        for shape in ("contiguous", "comb"):
            out |= {(K, ps, dim, "wrap " + shape, v) for v in ("none", "once", "twice")}
            if ps == "S":
                out |= {(K, ps, dim, "wrap " + shape, v) for v in ("negative", "interior")}
        out |= {(K, ps, dim, "reach", v) for v in ("n-1", "n=K")}
    return out


# Named by the rules, reached by no legal size: the index >= 2n in a SYNTHESIS tile along dimension 2.  Its halo lies in
# FRONT of the tile, so the last index it loads is base + (A - 1) s + Q - 1, and a tile with base >= T s / Q has n above that:
# only the first block can get there, and its last index is at most 16 s / Q - 1, against 2n >= 2 (K - 1) s + 2.
#   contiguous (Q = s): 15 >= 2n needs n <= 7, and n >= K rules out the filter of length 8 (n = 6, 7 do it for length 6);
#   comb (Q = cap): 16 / cap >= 2 (K - 1) + 3 / s holds for K = 2 (cap 4) and for no other length (4: 4 < 6, 6 and 8: 8 < 10).
# Along dimension 1 (T = 64) every length gets there.
UNREACHABLE = {
    (8, "S", 2, "wrap contiguous", "twice"),
    (4, "S", 2, "wrap comb", "twice"),
    (6, "S", 2, "wrap comb", "twice"),
    (8, "S", 2, "wrap comb", "twice"),
}


def required():
    req = set()
    for K in KS:
        for dim in (1, 2):
            req |= named_dim_classes(K, dim)
        req.add((K, "KxK"))
        req |= {(K, "depth", d, b) for d in DEPTHS for b in (1, 3)}
        req |= {(K, "parity", (a, b)) for a in (0, 1) for b in (0, 1)}
        req |= {(K, "shape", "M<N"), (K, "shape", "M>N")}
    return req - UNREACHABLE


REQUIRED = required()


def coefficients(case):
    (M, N), K, levels, batch = case[:4]
    return batch * M * N * (3 * (levels - 1) + 1)


def coverage(cases, report=None):
    """{class: [cases]}; `report(M, N, K, levels)` -> the per-level geometry dicts (default: the model)."""
    cov = {}
    for c in cases:
        (M, N), K, levels, batch = c[:4]
        rep = report(M, N, K, levels) if report else None
        for cl in classes(M, N, K, levels, batch, rep):
            cov.setdefault(cl, []).append(c[:4])
    return cov


def assert_coverage(cases, required=REQUIRED, report=None):
    cov = coverage(cases, report)
    missing = sorted((c for c in required if not cov.get(c)), key=repr)
    assert not missing, "no case reaches %s" % (missing,)
    return cov


def impulse_positions(n, K, levels, dim, report=None):
    """Indices along one dimension where an index error of some level shows: 0, n - 1, and for every level and pass the last
    output of the first tile, the first output of the second tile and, on a comb level, the first sample of the second run
    (those below n)."""
    if report is None:
        report = model_report(n, n, K, levels)
    pos = {0, n - 1}
    for g in report:
        for T in ((g["T1"],) if dim == 1 else (g["TA2"], g["TS2"])):
            s, Q, nr = g["s"], g["Q1" if dim == 1 else "Q2"], g["nr1" if dim == 1 else "nr2"]
            A = T // Q
            last_of_first = (A - 1) * s + Q - 1
            first_of_second = Q if nr > 1 else T               # tile 1 is run 1 of block 0, or block 1
            pos |= {p for p in (last_of_first, first_of_second) if p < n}
            if nr > 1:
                pos.add(Q)                                      # the first sample of the second run (Q < s <= reach < n)
    return sorted(pos)


def impulse_points(M, N, K, levels, report=None):
    """(row, column) pairs: every position of `impulse_positions` along each dimension occurs once, paired with a position
    of the other dimension in turn."""
    p1, p2 = impulse_positions(M, K, levels, 1, report), impulse_positions(N, K, levels, 2, report)
    pts = [(r, p2[i % len(p2)]) for i, r in enumerate(p1)] + [(p1[(i + 1) % len(p1)], c) for i, c in enumerate(p2)]
    return sorted(set(pts))


# ((M, N), K, levels, batch, marks): "i" the impulse subset (and the canary child), "d" the device-tensor case.  The comment
# names the classes a case was the first of the list to reach (pass and dimension, kind, values); the twelve TRANSFORM_CASES
# of tests/test_gpu_wavelet.py stay where they are and are not counted here.
CASES = [
    # ---- filter length 2
    ((65, 66), 2, 8, 1, "i"),     # 67 classes first reached here, e.g. A1 comb s=2cap n%s/steps%A; A1 comb s>=4cap n%s/steps%A; ...
    ((9, 9), 2, 5, 1, "i"),       # 10 classes first reached here, e.g. A1 tiling n<T; A2 reach n-1; A2 tiling n<T
    ((2, 2), 2, 2, 1, ""),        # A1 reach n=K; A2 reach n=K; KxK; S1 reach n=K; S2 reach n=K; S2 wrap contiguous twice; ...
    ((130, 3), 2, 3, 1, ""),      # A1 tiling >=3 cut; S1 tiling >=3 cut; S1 wrap contiguous interior; depth J=2 1; parity (0, 1); ...
    ((64, 2), 2, 2, 3, "d"),      # A1 tiling n=T; S1 tiling n=T; depth J=1 3
    ((3, 16), 2, 3, 3, ""),       # S2 tiling n=T; depth J=2 3
    ((5, 17), 2, 4, 3, ""),       # S2 tiling n=T+1; depth J odd>=3 3
    ((150, 33), 2, 7, 1, ""),     # A1 comb s=2cap >=2 blocks; A1 wrap comb none/once; A2 tiling n=T+1; S1 comb s=2cap >=2 blocks; ...
    ((2, 32), 2, 2, 1, ""),       # A2 tiling n=T
    ((9, 9), 2, 5, 3, ""),        # depth J even>=4 3
    ((17, 129), 2, 6, 1, ""),     # A2 comb s>=4cap >=2 blocks; A2 wrap comb none
    ((257, 65), 2, 8, 1, ""),     # A1 comb s>=4cap >=2 blocks; S1 comb s>=4cap >=2 blocks; S1 wrap comb interior
    # ---- filter length 4
    ((97, 98), 4, 7, 1, "i"),     # 65 classes first reached here, e.g. A1 comb s=2cap n%s/steps%A; A1 comb s>=4cap n%s/steps%A; ...
    ((4, 4), 4, 2, 1, "i"),       # 17 classes first reached here, e.g. A1 reach n=K; A1 tiling n<T; A1 wrap contiguous twice
    ((129, 5), 4, 2, 1, ""),      # A1 tiling >=3 cut; S1 tiling >=3 cut; S1 wrap contiguous interior; parity (1, 1); shape M>N
    ((64, 7), 4, 3, 1, "d"),      # A1 tiling n=T; S1 tiling n=T; depth J=2 1; parity (0, 1)
    ((65, 4), 4, 2, 3, ""),       # A1 tiling n=T+1; S1 tiling n=T+1; depth J=1 3
    ((13, 16), 4, 4, 1, ""),      # S2 tiling n=T; depth J odd>=3 1
    ((7, 17), 4, 3, 3, ""),       # S2 tiling n=T+1; depth J=2 3
    ((4, 32), 4, 2, 1, ""),       # A2 tiling n=T
    ((4, 33), 4, 2, 1, ""),       # A2 tiling n=T+1
    ((13, 13), 4, 4, 3, ""),      # depth J odd>=3 3
    ((255, 49), 4, 6, 1, ""),     # A1 comb s=2cap >=2 blocks; A1 wrap comb none; S1 comb s=2cap >=2 blocks; ...
    ((25, 25), 4, 5, 3, ""),      # depth J even>=4 3
    ((257, 129), 4, 7, 1, ""),    # A1 comb s>=4cap >=2 blocks; A2 comb s>=4cap >=2 blocks; S1 comb s>=4cap >=2 blocks
    # ---- filter length 6
    ((82, 81), 6, 6, 1, "i"),     # 64 classes first reached here, e.g. A1 comb s=2cap n%s/steps%A; A1 comb s>=4cap n%s/steps%A; ...
    ((6, 6), 6, 2, 1, "i"),       # 17 classes first reached here, e.g. A1 reach n-1/n=K; A1 tiling n<T; A1 wrap contiguous twice
    ((11, 16), 6, 3, 1, ""),      # S2 tiling n=T; depth J=2 1; parity (1, 0); shape M<N
    ((129, 7), 6, 2, 1, ""),      # A1 tiling >=3 cut; S1 tiling >=3 cut; S1 wrap contiguous interior; parity (1, 1)
    ((64, 17), 6, 2, 1, "d"),     # A1 tiling n=T; S1 tiling n=T; S2 tiling n=T+1
    ((65, 6), 6, 2, 3, ""),       # A1 tiling n=T+1; S1 tiling n=T+1; depth J=1 3
    ((11, 32), 6, 3, 3, ""),      # A2 tiling n=T; depth J=2 3
    ((171, 41), 6, 5, 1, ""),     # A1 comb s=2cap >=2 blocks; A1 wrap comb none; S1 comb s=2cap >=2 blocks; S1 wrap comb none; ...
    ((6, 33), 6, 2, 1, ""),       # A2 tiling n=T+1
    ((21, 82), 6, 4, 3, ""),      # A2 wrap comb none; depth J odd>=3 3
    ((257, 129), 6, 6, 1, ""),    # A1 comb s>=4cap >=2 blocks; A2 comb s>=4cap >=2 blocks; S1 comb s>=4cap >=2 blocks; ...
    ((41, 41), 6, 5, 3, ""),      # depth J even>=4 3
    # ---- filter length 8
    ((114, 113), 8, 6, 1, "i"),   # 65 classes first reached here, e.g. A1 comb s=2cap n%s/steps%A; A1 comb s>=4cap n%s/steps%A; ...
    ((8, 8), 8, 2, 1, "i"),       # 16 classes first reached here, e.g. A1 reach n-1/n=K; A1 tiling n<T; A1 wrap contiguous twice
    ((15, 16), 8, 3, 1, ""),      # S2 tiling n=T; depth J=2 1; parity (1, 0); shape M<N
    ((65, 17), 8, 2, 1, ""),      # A1 tiling n=T+1; S1 tiling n=T+1; S2 tiling n=T+1; parity (1, 1)
    ((129, 8), 8, 2, 1, ""),      # A1 tiling >=3 cut; S1 tiling >=3 cut; S1 wrap contiguous interior
    ((64, 8), 8, 2, 3, "d"),      # A1 tiling n=T; S1 tiling n=T; depth J=1 3
    ((15, 32), 8, 3, 3, ""),      # A2 tiling n=T; depth J=2 3
    ((8, 33), 8, 2, 1, ""),       # A2 tiling n=T+1
    ((255, 57), 8, 5, 1, ""),     # A1 comb s=2cap >=2 blocks; A1 wrap comb none; S1 comb s=2cap >=2 blocks; ...
    ((29, 29), 8, 4, 3, ""),      # depth J odd>=3 3
    ((257, 129), 8, 6, 1, ""),    # A1 comb s>=4cap >=2 blocks; A2 comb s>=4cap >=2 blocks; S1 comb s>=4cap >=2 blocks
    ((57, 57), 8, 5, 3, ""),      # depth J even>=4 3
    # ---- filter length 2, seams again: both neighbours of a tile multiple in each dimension, as deep as the size allows
    ((63, 31), 2, 6, 1, ""),
    ((65, 33), 2, 7, 3, ""),
    ((127, 17), 2, 6, 1, ""),
    ((128, 48), 2, 7, 1, ""),
    ((129, 63), 2, 7, 1, ""),
    ((193, 97), 2, 8, 1, ""),
    ((150, 320), 2, 9, 1, ""),
    # ---- filter length 4, seams again: both neighbours of a tile multiple in each dimension, as deep as the size allows
    ((63, 31), 4, 5, 1, ""),
    ((65, 33), 4, 5, 3, ""),
    ((127, 17), 4, 4, 1, ""),
    ((128, 48), 4, 5, 1, ""),
    ((129, 63), 4, 6, 1, ""),
    ((193, 97), 4, 7, 1, ""),
    ((150, 320), 4, 7, 1, ""),
    # ---- filter length 6, seams again: both neighbours of a tile multiple in each dimension, as deep as the size allows
    ((63, 31), 6, 4, 1, ""),
    ((65, 33), 6, 4, 3, ""),
    ((127, 17), 6, 3, 1, ""),
    ((128, 48), 6, 5, 1, ""),
    ((129, 63), 6, 5, 1, ""),
    ((193, 97), 6, 6, 1, ""),
    ((150, 320), 6, 6, 1, ""),
    # ---- filter length 8, seams again: both neighbours of a tile multiple in each dimension, as deep as the size allows
    ((63, 31), 8, 4, 1, ""),
    ((65, 33), 8, 4, 3, ""),
    ((127, 17), 8, 3, 1, ""),
    ((128, 48), 8, 4, 1, ""),
    ((129, 63), 8, 5, 1, ""),
    ((193, 97), 8, 5, 1, ""),
    ((150, 320), 8, 6, 1, ""),
]


def cases_of(K):
    return [c for c in CASES if c[1] == K]


def marked(mark, K=None):
    return [c for c in CASES if mark in c[4] and (K is None or c[1] == K)]
