"""CPU: the size list of the wavelet sweep (tests/wavelet_geometry_cases.py) reaches every tile-geometry class of
csrc/wavelet.hip for today's constants within its bounds, and the model gives the values written in DESIGN.md §3.8 and in the
comments of csrc/wavelet.hip.  tests/test_gpu_wavelet_sweep.py asserts model == library for every level of every case
before it launches anything."""
import pytest

import wavelet_geometry_cases as wg


def test_cases_reach_every_class_within_the_bounds():
    cov = wg.assert_coverage(wg.CASES)
    assert all(cov[c] for c in wg.REQUIRED)
    assert len(wg.CASES) <= wg.MAX_CASES
    assert len({c[:4] for c in wg.CASES}) == len(wg.CASES), "a case occurs twice"
    assert all(max(c[0]) <= wg.MAX_SIDE for c in wg.CASES)
    total = sum(wg.coefficients(c) for c in wg.CASES)
    print(f"{len(wg.CASES)} cases, {total} coefficients, {len(wg.REQUIRED)} classes")
    assert total <= wg.MAX_COEFFICIENTS
    for c in wg.CASES:
        wg.check(c[0][0], c[0][1], c[1], c[2])
        assert c[3] in (1, 3) and set(c[4]) <= set("id")


def test_required_is_what_legal_sizes_can_reach():
    """REQUIRED is every class the rules name minus UNREACHABLE; by enumeration of every legal (n, levels) up to MAX_SIDE each
    required class of one dimension is reachable and each class of UNREACHABLE is not."""
    for K in wg.KS:
        for dim in (1, 2):
            feasible, named = wg.feasible_dim_classes(K, dim), wg.named_dim_classes(K, dim)
            assert feasible <= named, sorted(feasible - named, key=repr)
            assert named - feasible == {c for c in wg.UNREACHABLE if c[0] == K and c[2] == dim}, (K, dim)
    assert not wg.UNREACHABLE & wg.REQUIRED
    # each K: 2 dimensions x 48 named classes, KxK, 8 depths, 4 parities, 2 shapes
    assert len(wg.REQUIRED) == 4 * (96 + 15) - len(wg.UNREACHABLE)


def test_a_case_that_is_alone_in_a_class_is_missed_by_name():
    cov = wg.coverage(wg.CASES)
    alone = {c: v[0] for c, v in cov.items() if c in wg.REQUIRED and len(v) == 1}
    assert alone
    for cl, case in sorted(alone.items(), key=repr)[::7]:
        rest = [c for c in wg.CASES if c[:4] != case]
        with pytest.raises(AssertionError) as e:
            wg.assert_coverage(rest)
        assert repr(cl) in str(e.value)


def test_marked_subsets():
    """The impulse subset holds, for every K, every run regime along both dimensions; one device-tensor case per K."""
    for K in wg.KS:
        got = set()
        for (M, N), _, levels, batch, _ in wg.marked("i", K):
            got |= {c for c in wg.classes(M, N, K, levels, batch) if len(c) == 5 and c[3] == "regime"}
        assert got == {(K, ps, dim, "regime", r) for ps in wg.PASSES for dim in (1, 2) for r in wg.REGIMES}
        assert len(wg.marked("d", K)) == 1
    # the positions: index 0, the last sample, both sides of the first tile seam and the second run of a comb
    assert wg.impulse_positions(150, 8, 5, 1) == [0, 4, 63, 64, 123, 149]      # s = 8, Q = 4: (16 - 1) 8 + 3 = 123
    assert wg.impulse_positions(40, 2, 4, 2) == [0, 15, 16, 31, 32, 39]
    assert wg.impulse_positions(13, 2, 4, 2) == [0, 12]
    pts = wg.impulse_points(150, 131, 8, 5)
    assert {r for r, _ in pts} >= set(wg.impulse_positions(150, 8, 5, 1))
    assert {c for _, c in pts} >= set(wg.impulse_positions(131, 8, 5, 2))


# DESIGN.md §3.8 and the comments of csrc/wavelet.hip, by hand: (M, N, K, levels, level) -> the documented values
DOCUMENTED = {
    # runs are capped at 16 / 8 / 4 rows and 4 / 2 columns by filter length; below the cap the tile is contiguous
    (320, 320, 2, 8, 1): dict(J=7, s=1, Q1=1, Q2=1, nr1=1, nr2=1, T1=64, TA2=32, TS2=16, tiles1=5, tilesA2=10, tilesS2=20,
                              halo1=1, halo2=1),
    (320, 320, 2, 8, 5): dict(s=16, Q1=16, nr1=1, Q2=4, nr2=4, halo1=16, halo2=4),
    (320, 320, 2, 8, 6): dict(s=32, Q1=16, nr1=2, Q2=4, nr2=8),
    (320, 320, 2, 8, 7): dict(s=64, Q1=16, nr1=4, tiles1=8),             # 5 steps, 4 per tile: 2 blocks x 4 runs
    (320, 320, 4, 6, 4): dict(s=8, Q1=8, nr1=1, Q2=4, nr2=2, halo1=24, halo2=12),
    (320, 320, 4, 6, 5): dict(s=16, Q1=8, nr1=2, Q2=4, nr2=4),
    (320, 320, 6, 5, 3): dict(s=4, Q1=4, nr1=1, Q2=2, nr2=2, halo1=20, halo2=10),
    (320, 320, 6, 5, 4): dict(s=8, Q1=4, nr1=2, Q2=2, nr2=4),
    (320, 320, 8, 5, 2): dict(s=2, Q1=2, Q2=2, nr1=1, nr2=1, halo1=14, halo2=14),
    (320, 320, 8, 5, 3): dict(s=4, Q1=4, Q2=2, nr1=1, nr2=2, halo1=28),
    (320, 320, 8, 5, 4): dict(s=8, Q1=4, nr1=2, Q2=2, nr2=4, halo1=28, halo2=14),
    # LDS: tile + lo + hi (analysis), two band tiles + lo / hi with the dimension-1 halo (synthesis); "45-79 KB", "84 rows
    # per tile column" for length 6
    (8, 8, 8, 2, 1): dict(lds_analysis=80960, lds_synthesis=67712, tiles1=1, tilesA2=1, tilesS2=1),
    (6, 6, 6, 2, 1): dict(lds_analysis=8 * (42 * 84 + 2 * 42 * 64), lds_synthesis=8 * (2 * 26 * 84 + 2 * 16 * 84)),
    (4, 4, 4, 2, 1): dict(lds_analysis=8 * (44 * 88 + 2 * 44 * 64), lds_synthesis=8 * (2 * 28 * 88 + 2 * 16 * 88)),
    (2, 2, 2, 2, 1): dict(lds_analysis=8 * (36 * 80 + 2 * 36 * 64), lds_synthesis=8 * (2 * 20 * 80 + 2 * 16 * 80)),
    # tiles: 64 outputs along dimension 1, 32 / 16 along dimension 2; a comb tile covers A = T / Q steps of one run
    (64, 32, 2, 2, 1): dict(tiles1=1, tilesA2=1, tilesS2=2),
    (65, 33, 2, 2, 1): dict(tiles1=2, tilesA2=2, tilesS2=3),
    (150, 131, 8, 5, 4): dict(tiles1=4, tilesA2=8, tilesS2=12),          # 19 / 17 steps; A = 16, 16, 8
    (96, 160, 2, 7, 6): dict(tiles1=2, tilesA2=8, tilesS2=16),           # 3 / 5 steps of 32; A = 4, 8, 4
}


@pytest.mark.parametrize("key", sorted(DOCUMENTED))
def test_model_gives_the_documented_geometry(key):
    geo = wg.model_geometry(*key)
    for k, v in DOCUMENTED[key].items():
        assert geo[k] == v, (key, k, geo[k], v)


def test_documented_bounds_and_refusals():
    for K in wg.KS:
        la, ls = wg.lds_bytes(K)
        assert 45 * 1024 <= min(la, ls) and max(la, ls) <= 80 * 1024       # "45-79 KB per workgroup (<= 80 KB: two per CU)"
    # the deepest comb class needs n >= 113 for the filter of length 8; nothing needs more than MAX_SIDE
    assert min(n for n in range(8, 321) for lv in range(2, wg.max_levels(n, 8) + 1)
               if (8, "A", 1, "regime", "s>=4cap") in wg.dim_classes(n, 8, lv, 1)) == 113
    for bad in ((32, 32, 3, 3), (32, 32, 10, 2), (32, 32, 4, 1), (12, 12, 4, 4), (40, 12, 4, 4), (0, 5, 2, 2)):
        with pytest.raises(ValueError):
            wg.check(*bad)
    wg.check(13, 13, 4, 4)
    with pytest.raises(ValueError):
        wg.model_geometry(32, 32, 4, 3, 3)
    with pytest.raises(ValueError):
        wg.model_geometry(32, 32, 4, 3, 0)
