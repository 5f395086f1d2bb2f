"""CPU: the shape lists of the FFT sweep (tests/fft_plan_cases.py) reach every plan class of DESIGN.md §3.2.1 for
today's constants, and the model gives the plan values written there.  tests/test_gpu_fft_sweep.py asserts the same on
the plans the library reports before it launches anything."""
import pytest

import fft_plan_cases as fc


def test_pow2_pairs_reach_every_class():
    shapes = fc.pow2_shapes()
    assert len(shapes) == 81 and len({s[:2] for s in shapes}) == 81
    cov = fc.assert_coverage(shapes, fc.model_plan, fc.pow2_required())
    assert all(cov[c] for c in fc.pow2_required())
    # exactly the documented instantiations occur, no others
    assert {c[1] for c in cov if c[0] == "rows"} == set(fc.ROW_INSTANTIATIONS)
    assert {c[1] for c in cov if c[0] == "cols"} == set(fc.COL_INSTANTIATIONS)
    assert {c[1] for c in cov if c[0] == "wave"} == {(512, 1024), (512, 2048), (1024, 1024), (1024, 2048)}


def test_operator_shapes_reach_every_class_with_bounded_size():
    shapes = fc.operator_shapes()
    fc.assert_coverage(shapes, fc.model_plan, fc.pow2_required())
    pairs = {s[:2] for s in shapes}
    assert len(pairs) == len(shapes) and {(M, N) for M, N in fc.POW2_PAIRS if M * N <= 1 << 20} <= pairs
    big = sorted(p for p in pairs if p[0] * p[1] > 1 << 20)
    # above 2^20 pixels every pair has a plan report of its own: all ten run
    assert big == sorted(p for p in fc.POW2_PAIRS if p[0] * p[1] > 1 << 20) and len(big) == 10
    assert len({tuple(sorted(fc.model_plan(*p).items())) for p in big}) == 10
    # the instantiations nothing ran an operator through before this sweep
    assert (256, 4096) in pairs and (2048, 256) in pairs and (16, 32) in pairs and (64, 16) in pairs


# DESIGN.md §3.2.1, the boundaries of the classes: (M, N) -> the documented values
DOCUMENTED = {
    # columns per workgroup / threads: as many columns as fit 256 threads, fewer where one image has few workgroups
    (16, 16): dict(n1=8, cols_per_wg=16, cols_threads=16, cols_wgs=1, rows_per_wg=8, rows_threads=16, rows_wgs=1),
    (16, 32): dict(cols_per_wg=32, cols_threads=32, rows_threads=32),
    (16, 4096): dict(cols_per_wg=64, cols_threads=64, cols_wgs=64, rows_per_wg=2, rows_threads=1024, rows_wgs=4),
    (512, 512): dict(n1=256, cols_per_wg=2, cols_threads=64, cols_wgs=256, rows_per_wg=1, rows_threads=64),
    (1024, 512): dict(n1=512, cols_per_wg=2, cols_threads=128, rows_per_wg=4, rows_threads=256, rows_wgs=128),
    (1024, 256): dict(rows_per_wg=2, rows_threads=64, rows_wgs=256),
    (2048, 256): dict(rows_per_wg=8, rows_threads=256, rows_wgs=128),
    (512, 1024): dict(wave=False, rows_per_wg=4, rows_threads=512, rows_kind="workgroup"),
    (1024, 1024): dict(wave=True, u_tiled=True, cols_per_wg=4, cols_threads=256, cols_wgs=256, rows_per_wg=4,
                       rows_threads=256, rows_wgs=128, rows_kind="pipelined", step_ok=True, lch=1),
    (2048, 2048): dict(wave=True, n1=1024, rows_threads=512, rows_wgs=256, lch=4),
    (4096, 2048): dict(wave=False, n1=2048, cols_per_wg=1, cols_threads=256, rows_per_wg=4, rows_threads=1024, lch=8),
    (4096, 4096): dict(rows_per_wg=2, rows_threads=1024, rows_wgs=1024, lch=16, step_ok=False, csalsa_ok=True),
    (2048, 50): dict(generic=True, L_M=4096, L_N=128, rows_kind="pointwise", csalsa_ok=False, tv_ok=False, lch=0),
    (2049, 50): dict(generic=True, L_M=8192),
    (60, 2048): dict(L_M=128, L_N=4096),
    (60, 2049): dict(L_N=8192),
    (2, 2): dict(generic=True, L_M=4, L_N=4, n1=2),
    (3, 50): dict(L_M=8),
    (8, 50): dict(generic=True, L_M=16),
    (32, 50): dict(generic=True, L_M=64),
    (33, 50): dict(L_M=128),
    (4096, 50): dict(generic=True, L_M=8192, n1=4096),
}


@pytest.mark.parametrize("shape", sorted(DOCUMENTED))
def test_model_gives_the_documented_plan_values(shape):
    plan = fc.model_plan(*shape)
    for k, v in DOCUMENTED[shape].items():
        assert plan[k] == v, (shape, k, plan[k], v)


def test_documented_class_boundaries():
    cl = lambda M, N: fc.classes(M, N, fc.model_plan(M, N))
    # PREP iff M <= 512
    assert ("PREP", True) in cl(512, 64) and ("PREP", False) in cl(1024, 64)
    # N = 256 splits at M = 2048, N = 512 at M = 1024
    assert ("rows", (8, 2)) in cl(1024, 256) and ("rows", (8, 8)) in cl(2048, 256)
    assert ("rows", (9, 1)) in cl(512, 512) and ("rows", (9, 4)) in cl(1024, 512)
    assert ("rows", (12, 2)) in cl(16, 4096) and ("rows", (11, 4)) in cl(4096, 2048)
    # PRE iff RK N / 8 <= 256; the partial-wave reduction iff RK N / 8 < 64: N = 16, 32
    assert ("PRE", True) in cl(4096, 256) and ("PRE", False) in cl(16, 1024) and ("PRE", True) in cl(512, 512)
    assert ("partial wave", True) in cl(64, 16) and ("partial wave", True) in cl(64, 32)
    assert ("partial wave", True) not in cl(64, 64)
    # the wave plans and their neighbours
    assert fc.model_plan(1024, 2048)["wave"] and not fc.model_plan(512, 2048)["wave"] and not fc.model_plan(4096, 1024)["wave"]
    assert not fc.model_plan(1024, 1024, wave_enabled=False)["wave"]
    assert fc.model_plan(1024, 1024, wave_enabled=False)["rows_per_wg"] == 4
    # lch grows with the image and the batch; a shared-spectrum batch folds on every wave plan
    assert fc.model_plan(1024, 1024, 2)["lch"] == 2 and fc.model_plan(512, 512, 8)["lch"] == 2
    assert all(fc.model_plan(M, N, 3)["fold"] and not fc.model_plan(M, N, 1)["fold"] for M in (1024, 2048) for N in (1024, 2048))
    # Bluestein lengths at their boundaries
    assert [fc.bluestein_len(n) for n in (2, 3, 7, 8, 32, 33, 1024, 1025, 2048, 2049, 4093, 4095, 4096)] == \
        [4, 8, 16, 16, 64, 128, 2048, 4096, 4096, 8192, 8192, 8192, 8192]
    with pytest.raises(ValueError):
        fc.model_plan(4097, 16)


def test_chirp_shapes_reach_every_class_with_bounded_size():
    shapes = fc.chirp_shapes()
    assert 30 <= len(shapes) <= 40 and len({s[:2] for s in shapes}) == len(shapes)
    assert all(fc.model_plan(M, N)["generic"] for M, N, _ in shapes)
    fc.assert_coverage(shapes, fc.model_plan, fc.CHIRP_REQUIRED)
    pairs = {s[:2] for s in shapes}
    assert pairs >= set(fc.CHIRP_CORNERS)
    for n, _ in fc.AXIS_CLASSES:
        assert (n, fc.GENERIC_WIDTH) in pairs and (fc.GENERIC_HEIGHT, n) in pairs
    par = {(M % 2, N % 2) for M, N in pairs}
    assert par == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {n for n, _ in fc.AXIS_CLASSES} >= {2, 3, 7, 8, 2048, 2049, 4093, 4095, 4096}


def test_tap_shapes():
    shapes = fc.tap_shapes()
    assert {t for s in shapes for t in s[3]} == set(range(1, 16))
    assert all(t <= min(M, N) for M, N, _, ts, _ in shapes for t in ts)
    assert {(t, t) for t in range(2, 16)} <= {s[:2] for s in shapes}
    reports = [fc.model_plan(M, N, B) for M, N, B, _, _ in shapes]
    assert any(r["u_tiled"] and r["lch"] > 1 for r in reports) and any(not r["generic"] and not r["u_tiled"] and r["lch"] > 1 for r in reports)
    assert any(r["generic"] for r in reports) and any(r["u_tiled"] and r["lch"] == 1 for r in reports)
