"""Image sizes that sit on the tile seams and image edges of the Chambolle kernels, derived from a tile geometry.

Plain Python, no GPU.  A geometry is the dict `Context.prox_geometry` returns (region_rows, core_rows, halo_top,
halo_bottom, rows_per_lane, region_cols, core_cols, halo_left, halo_right, max_steps, single_ti, single_tj, ...); the
functions below turn it into lists of `(M, N, why)` and carry a MODEL of the kernels' tile classification.  The model
is only there to PROVE that a list of shapes covers the classes (`coverage`, `assert_coverage`); it never produces an
expected value - those come from the oracle.

The model (csrc/tv_fused.inc, csrc/tv_fused1.inc): tile (ti, tj) owns the core rows [ti R, ti R + R) and loads the
region that starts at i0 = ti R - halo_top and spans region_rows rows; d = M - (i0 + region_rows) is the number of
image rows below the region (negative: the region overhangs the image).  The same in the columns.  A tile runs the
body without boundary selects iff i0 >= 1, d >= 1 on both axes.

Cases that a shape drops because its size makes them meaningless are listed by name in DROPPED; no class loses all of
its shapes that way (test_tv_geometry_cases_cpu.py checks it).
"""

# every fused-kernel shape runs these through chambolle_prox_TV_stop (S = max_steps of the geometry):
#   cold1, coldS (one launch of the maximum step count: the outermost halo pixel reaches the core), coldS+2 (two
#   launches), cold25, warm (S more from the oracle's duals after S), warm_any (S more from arbitrary duals of modulus
#   <= 1 that are NOT zero in the last row of px / last column of py: DivergenceIm ends with -p(end), quirk Q3, which
#   is zero on every iterate of a cold start, so only such a start shows a kernel that reads it wrongly or counts
#   columns beyond the image in the error sum)
# corner shapes add: batch3 (three images, own lambda), stop3 / stop5 (stop rule out of MaxIter 15)
DROPPED = {
    # shape -> names of the cases it does not run, with the reason.  Nothing is dropped today: every case is defined
    # from 2 x 2 on (a cold or warm prox of a 2 x 2 image is four pixels of boundary rules).
}


def _even_up(v):
    return v + (v & 1)


def fused_axes(geom):
    """(rows, cols): per axis (core, halo_before, region extent)."""
    return ((geom["core_rows"], geom["halo_top"], geom["region_rows"]),
            (geom["core_cols"], geom["halo_left"], geom["region_cols"]))


def region_end(axis, t):
    """First index beyond the region of tile t on this axis."""
    core, before, extent = axis
    return t * core - before + extent


def axis_tiles(axis, L):
    """Model of one axis for an image extent L: per tile (t, start, d, inner)."""
    core, before, extent = axis
    out = []
    for t in range((L + core - 1) // core):
        start = t * core - before
        d = L - (start + extent)
        out.append(dict(t=t, start=start, d=d, inner=(start >= 1 and d >= 1)))
    return out


def classify(geom, M, N):
    """Model of the classification of every tile of an M x N image: dicts with ti, tj, i0, j0, di, dj, interior."""
    rows, cols = fused_axes(geom)
    return [dict(ti=a["t"], tj=b["t"], i0=a["start"], j0=b["start"], di=a["d"], dj=b["d"], row_inner=a["inner"],
                 col_inner=b["inner"], interior=a["inner"] and b["inner"])
            for b in axis_tiles(cols, N) for a in axis_tiles(rows, M)]


def interior_sizes(axis, even_only, tiles=(1, 2)):
    """Image extents around the interior test of the tiles `tiles` (>= 1) of this axis: {"zero": L with d = 0, "pos": L
    with the smallest positive d, "neg": L with the smallest overhang}, each as (L, t, d).  With `even_only` (rows: an odd
    M takes the one-iteration kernels) an odd region end cannot be met exactly, which is why more than one tile is looked
    at: with an odd core height consecutive tile rows end at different parities."""
    best = {}
    for t in tiles:
        e = region_end(axis, t)
        for d in (-2, -1, 0, 1, 2):
            L = e + d
            if L < 2 or (even_only and L % 2):
                continue
            key = "zero" if d == 0 else ("pos" if d > 0 else "neg")
            if key not in best or abs(d) < abs(best[key][2]):
                best[key] = (L, t, d)
    return best


def generic_extent(axis, even):
    """An extent with no special relation to the tiles whose tile 1 is inner with room to spare."""
    L = region_end(axis, 1) + axis[0] // 2
    return _even_up(L) if even else L


def row_sizes(geom):
    """[(M, why)]: the row classes of a fused kernel; M even."""
    rows, _ = fused_axes(geom)
    R, HB = geom["core_rows"], geom["halo_bottom"]
    out = [(2, "M=2"), (_even_up(R // 2), "below one core")]
    if R % 2 == 0:
        out.append((R, "M=R: one tile, no remainder"))
    else:
        out.append((R - 1, "M=R-1: one tile one row short (R is odd)"))
    first = True
    for M in range(R + 1, R + HB + 1):
        if M % 2 == 0:
            out.append((M, "M=R+%d: %s" % (M - R, "last tile of minimum extent, " if first else "")
                        + "tile 0's bottom halo straddles the image end"))
            first = False
    out += [(2 * R - 2, "M=2R-2"), (2 * R, "M=2R: no remainder")]
    for key, (M, t, d) in sorted(interior_sizes(rows, True).items()):
        out.append((M, "rows: d=%d at tile row %d" % (d, t)))
    return out


def col_sizes(geom):
    """[(N, why)]: the column classes of a fused kernel; any parity."""
    _, cols = fused_axes(geom)
    C, HR = geom["core_cols"], geom["halo_right"]
    out = [(2, "N=2"), (C - 1, "N=C-1"), (C, "N=C: one tile, no remainder")]
    for k in range(1, HR + 1):
        out.append((C + k, "N=C+%d: %s" % (k, "last tile holds one column, " if k == 1 else "")
                    + "tile 0's right halo straddles the image end"))
    out += [(2 * C, "N=2C: no remainder"), (2 * C + 1, "N=2C+1: last tile holds one column")]
    e = region_end(cols, 1)
    for d in (-1, 0, 1, 2):
        out.append((e + d, "cols: d=%d at tile column 1" % d))
    return out


def corner_shapes(geom):
    """The four combinations of the interior pairs {d = 0, smallest positive d} of the two axes."""
    rows, cols = fused_axes(geom)
    ri, ci = interior_sizes(rows, True), interior_sizes(cols, False, tiles=(1,))
    return [(ri[a][0], ci[b][0], "corner: rows d=%d at tile row %d, cols d=%d at tile column %d"
             % (ri[a][2], ri[a][1], ci[b][2], ci[b][1])) for a in ("zero", "pos") for b in ("zero", "pos")]


def square_shape(geom):
    """One square shape (quirk Q2: the reference's SALSA warm start needs M == N) whose rows have d = 0."""
    rows, _ = fused_axes(geom)
    M = interior_sizes(rows, True)["zero"][0]
    return (M, M, "square: rows d=0")


def fused_shapes(geom):
    """[(M, N, why)] for one fused kernel: every row class at one generic width, every column class at one generic height,
    and the corners.  No duplicates."""
    rows, cols = fused_axes(geom)
    Ng, Mg = generic_extent(cols, False), generic_extent(rows, True)
    out, seen = [], set()
    for M, N, why in ([(M, Ng, why) for M, why in row_sizes(geom)] + [(Mg, N, why) for N, why in col_sizes(geom)]
                      + corner_shapes(geom) + [square_shape(geom)]):
        if (M, N) not in seen:
            seen.add((M, N))
            out.append((M, N, why))
    return out


def single_step_shapes(geom):
    """(odd, even): shapes of the one-iteration kernels (tile single_ti x single_tj).  Odd M reaches them by itself,
    even M through SBTV_SINGLE_STEP=1."""
    TI, TJ = geom["single_ti"], geom["single_tj"]
    Ns = [TJ - 1, TJ, TJ + 1, 2 * TJ, 2 * TJ + 1]
    odd = [(M, N, "one-iteration, odd M") for M in (TI - 1, TI + 1, 2 * TI - 1, 2 * TI + 1) for N in Ns]
    even = [(M, N, "one-iteration, even M") for M in (TI - 2, TI, TI + 2, 2 * TI) for N in Ns]
    return odd, even


def edge_large_shapes(geom, ti=8, tj=40):
    """Two shapes large enough for the plans to choose the two-rows-per-lane kernel by themselves, whose tile row `ti` /
    tile column `tj` ends exactly at the image end (d = 0) resp. just inside it (smallest positive d)."""
    rows, cols = fused_axes(geom)
    ri, ci = interior_sizes(rows, True, tiles=(ti, ti + 1)), interior_sizes(cols, False, tiles=(tj,))
    return [(ri[k][0], ci[k][0], "large: rows d=%d at tile row %d, cols d=%d at tile column %d"
             % (ri[k][2], ri[k][1], ci[k][2], ci[k][1])) for k in ("zero", "pos")]


def table_candidates(geom):
    """Shapes with a few hundred to about 800 tiles and ragged last tiles, from which the GPU test picks those whose
    REPORTED plan has a tile table without stagger, a tile count that is a multiple of 8, an odd one."""
    R, C = geom["core_rows"], geom["core_cols"]
    out = []
    for k, l in ((11, 49), (16, 33), (13, 58), (12, 45), (9, 59), (10, 53), (14, 41), (7, 77)):
        M = (k - 1) * R + 2 + 2 * ((7 * k) % (R // 2 - 1))
        N = (l - 1) * C + 1 + (5 * l) % C
        out.append((M, N, "table candidate: %d x %d tiles" % (k, l)))
    return out


def n_tiles(geom, M, N):
    R, C = geom["core_rows"], geom["core_cols"]
    return ((M + R - 1) // R) * ((N + C - 1) // C)


def coverage(geom, shapes):
    """Which classes the shapes cover, per axis: {("rows" | "cols", class): [shapes]}."""
    rows, cols = fused_axes(geom)
    want = {"rows": interior_sizes(rows, True), "cols": interior_sizes(cols, False, tiles=(1,))}
    min_last = {"rows": 1 if geom["core_rows"] % 2 else 2, "cols": 1}
    cov = {(ax, c): [] for ax in ("rows", "cols") for c in ("d=0", "d=min+", "d=max-", "min last tile", "no remainder")}
    for M, N, _ in shapes:
        for ax, L, core, dk, ik, ok in (("rows", M, geom["core_rows"], "di", "i0", "col_inner"),
                                        ("cols", N, geom["core_cols"], "dj", "j0", "row_inner")):
            tl = classify(geom, M, N)
            # the tile's classification hangs on this axis' comparison: it starts inside and its other axis is inner
            hang = [t for t in tl if t[ik] >= 1 and t[ok]]
            if any(t[dk] == 0 and not t["interior"] for t in hang):
                cov[(ax, "d=0")].append((M, N))
            if any(t[dk] == want[ax]["pos"][2] and t["interior"] for t in hang):
                cov[(ax, "d=min+")].append((M, N))
            if any(t[dk] == want[ax]["neg"][2] and not t["interior"] for t in hang):
                cov[(ax, "d=max-")].append((M, N))
            if L > core and L - ((L + core - 1) // core - 1) * core == min_last[ax]:
                cov[(ax, "min last tile")].append((M, N))
            if L % core == 0:
                cov[(ax, "no remainder")].append((M, N))
    return cov


def assert_coverage(geom, shapes):
    cov = coverage(geom, shapes)
    empty = [k for k, v in cov.items() if not v]
    assert not empty, "no shape covers %s for the geometry %s" % (empty, geom)
    dropped_all = [k for k, v in cov.items() if all(DROPPED.get(s) for s in v)]
    assert not dropped_all, dropped_all
    return cov
