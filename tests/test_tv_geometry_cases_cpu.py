"""CPU: the shape generator of the Chambolle geometry sweep (tests/tv_geometry_cases.py) covers its classes for the
tile geometry documented in DESIGN.md §3.1.  tests/test_gpu_tv_geometry.py asserts the same on the geometry the library
reports before it launches anything."""
import pytest

import tv_geometry_cases as tg

COMMON = dict(region_cols=32, core_cols=21, halo_left=6, halo_right=5, max_steps=5, single_ti=128, single_tj=16)
GEOMETRIES = {
    "rows2": dict(COMMON, region_rows=128, core_rows=116, halo_top=6, halo_bottom=6, rows_per_lane=2),
    "rows1": dict(COMMON, region_rows=64, core_rows=53, halo_top=6, halo_bottom=5, rows_per_lane=1),
}


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_fused_shapes_cover_every_class(name):
    geom = GEOMETRIES[name]
    shapes = tg.fused_shapes(geom)
    cov = tg.assert_coverage(geom, shapes)
    assert all(M % 2 == 0 and M >= 2 and N >= 2 for M, N, _ in shapes)
    assert len(shapes) == len({(M, N) for M, N, _ in shapes}) and 20 <= len(shapes) <= 48, len(shapes)
    # the classification of the d = 0 tiles hangs on ONE comparison: changing `<= M - 1` to `<= M` in the model flips them
    for ax in ("rows", "cols"):
        for M, N in cov[(ax, "d=0")]:
            assert any(not t["interior"] and t["i0"] >= 1 and t["j0"] >= 1 and min(t["di"], t["dj"]) == 0
                       for t in tg.classify(geom, M, N))


def test_documented_sizes_are_generated():
    """The sizes the model gives for today's constants (the ones the issue of this sweep names)."""
    r2, r1 = GEOMETRIES["rows2"], GEOMETRIES["rows1"]
    assert {M for M, _ in tg.row_sizes(r2)} >= {2, 116, 118, 120, 122, 230, 232, 236, 238, 240}
    assert {M for M, _ in tg.row_sizes(r1)} >= {2, 52, 54, 56, 58, 104, 106, 110, 112, 164}
    assert {N for N, _ in tg.col_sizes(r2)} >= {2, 20, 21, 22, 23, 24, 25, 26, 42, 43, 46, 47, 48, 49}
    assert [s[:2] for s in tg.corner_shapes(r2)] == [(238, 47), (238, 48), (240, 47), (240, 48)]
    assert [s[:2] for s in tg.corner_shapes(r1)] == [(164, 47), (164, 48), (112, 47), (112, 48)]
    assert [s[:2] for s in tg.edge_large_shapes(r2)] == [(1050, 866), (1052, 867)]
    assert all(tg.n_tiles(r2, M, N) >= 256 for M, N, _ in tg.edge_large_shapes(r2))
    odd, even = tg.single_step_shapes(r2)
    assert {M for M, _, _ in odd} == {127, 129, 255, 257} and {M for M, _, _ in even} == {126, 128, 130, 256}
    assert {N for _, N, _ in odd + even} == {15, 16, 17, 32, 33}


def test_model_classification_at_known_sizes():
    r2 = GEOMETRIES["rows2"]
    # 1050 x 866: tile row 8 and tile column 40 end exactly at the image end: wholly inside the image, not interior
    t = [t for t in tg.classify(r2, 1050, 866) if t["ti"] == 8 and t["tj"] == 40][0]
    assert (t["i0"], t["j0"], t["di"], t["dj"], t["interior"]) == (922, 834, 0, 0, False)
    assert sum(t["interior"] for t in tg.classify(r2, 1050, 866)) == 273
    assert sum(t["interior"] for t in tg.classify(r2, 1052, 867)) == 320
    assert tg.n_tiles(r2, 2048, 2048) == 1764 and tg.n_tiles(r2, 1400, 1200) == 754


def test_table_candidates_span_the_tile_counts():
    r2 = GEOMETRIES["rows2"]
    nts = [tg.n_tiles(r2, M, N) for M, N, _ in tg.table_candidates(r2)]
    assert all(M % 2 == 0 for M, _, _ in tg.table_candidates(r2))
    assert any(n > 512 and n % 2 for n in nts) and any(n > 512 and n % 8 == 0 for n in nts), nts
    assert any(512 < n < 768 for n in nts), nts


def test_no_class_is_emptied_by_dropped_cases():
    assert tg.DROPPED == {}
