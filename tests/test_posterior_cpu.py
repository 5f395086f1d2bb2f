"""CPU: the posterior-moments feature (sbtv_SAPG_algorithm_moments / sbtv_myula_moments) without a GPU - the C struct and
its ctypes mirror, the compiler's resource report of the accumulating kernels, and sbtv.combine_moments."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_moments_opts_layout_matches_header():
    from sbtv import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sbtv.h"\nint main(void){printf("%zu %zu %zu %zu\\n",'
           'sizeof(sbtv_moments_opts), offsetof(sbtv_moments_opts, first), offsetof(sbtv_moments_opts, thin),'
           'offsetof(sbtv_moments_opts, pooled));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "t")], check=True, capture_output=True,
                                              text=True).stdout.split()]
    m = _lib.sbtv_moments_opts
    assert out == [C.sizeof(m), m.first.offset, m.thin.offset, m.pooled.offset]


def test_moments_entry_points_are_bound():
    import sbtv
    from sbtv import _lib
    lib = sbtv.load_library()
    for name in ("sbtv_SAPG_algorithm_moments", "sbtv_myula_moments"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    # every argument of the plain entry point, in order, before the moments arguments and flags
    assert _lib.SIGNATURES["sbtv_SAPG_algorithm_moments"][1][:-5] == _lib.SIGNATURES["sbtv_SAPG_algorithm"][1][:-1]
    assert _lib.SIGNATURES["sbtv_myula_moments"][1][:-5] == _lib.SIGNATURES["sbtv_myula"][1][:-1]


def _report(unit):
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-gpu-rdc", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(CSRC, unit)],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def _find(rep, *parts):
    names = [n for n in rep if all(p in n for p in parts)]
    assert len(names) == 1, (parts, names)
    return rep[names[0]]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_fused_myula_moments_epilogue_keeps_occupancy_without_scratch():
    rep = _report("fft.hip")
    for l2n, v in ((10, 16), (9, 8)):           # n1 = 1024 (M = 2048) and 512 (M = 1024)
        plain = _find(rep, f"cols_inv_wave_kernelILi{l2n}ELi{v}ELi16E")
        mom = _find(rep, f"cols_inv_wave_kernelILi{l2n}ELi{v}ELi144E")     # PM = 16 | 128
        assert mom["ScratchSize"] == 0 and mom["VGPRs Spill"] == 0, (l2n, mom)
        assert mom["Occupancy"] >= plain["Occupancy"], (l2n, plain, mom)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_elementwise_moments_kernels_use_no_scratch():
    rep = _report("elementwise.hip")
    for parts in (("myula_step_kernelILb1E",), ("myula_plain_kernelILb1E",), ("moments_seed_kernel",),
                  ("moments_finish_kernel",)):
        k = _find(rep, *parts)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, (parts, k)


def _two_pass(x):
    n = x.shape[0]
    return n, x.mean(axis=0), (x.var(axis=0, ddof=1) if n > 1 else np.zeros(x.shape[1:]))


@pytest.mark.parametrize("seed", range(6))
def test_combine_moments_matches_two_pass(seed):
    import sbtv
    rng = np.random.default_rng(seed)
    total = int(rng.integers(2, 40))
    x = rng.standard_normal((total, 5, 7)) * rng.uniform(0.1, 10) + rng.uniform(-100, 100)
    # random split into consecutive parts, n = 1 parts included
    cuts = np.sort(rng.choice(np.arange(1, total), size=min(total - 1, int(rng.integers(1, 6))), replace=False))
    if seed % 2 == 0 and total > 2:
        cuts = np.unique(np.concatenate([cuts, [1, 2]]))
    pieces = np.split(x, cuts)
    n, mean, var = sbtv.combine_moments([_two_pass(p) for p in pieces])
    rn, rmean, rvar = _two_pass(x)
    assert n == rn
    np.testing.assert_allclose(mean, rmean, rtol=1e-13, atol=1e-13 * np.abs(rmean).max())
    np.testing.assert_allclose(var, rvar, rtol=1e-13, atol=0)


def test_combine_moments_of_single_samples_and_one_part():
    import sbtv
    x = np.array([[1.0, 2.0], [3.0, 7.0], [4.0, -1.0]])
    n, mean, var = sbtv.combine_moments([(1, r, np.zeros(2)) for r in x])
    assert n == 3
    np.testing.assert_allclose(mean, x.mean(0), rtol=1e-15)
    np.testing.assert_allclose(var, x.var(0, ddof=1), rtol=1e-14)
    n1, m1, v1 = sbtv.combine_moments([(1, x[0], np.zeros(2))])
    assert n1 == 1 and np.array_equal(m1, x[0]) and not v1.any()
    with pytest.raises(ValueError):
        sbtv.combine_moments([])
