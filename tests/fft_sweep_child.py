"""Child program of tests/test_gpu_fft_sweep.py::test_switches_in_child_processes: a fresh process started with one of
the A/B switches (SBTV_FFT_WAVE=0, SBTV_ROWS_FOLD=0) in its environment runs the wave-plan cases and saves what it
computed; the parent compares.  usage: fft_sweep_child.py OUT.npz"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np

import fft_plan_cases as fc
import test_gpu_fft_sweep as sweep


def main(path):
    import sbtv
    ctx = sbtv.default_context(0)
    wave = os.environ.get("SBTV_FFT_WAVE") != "0"
    fold = wave and os.environ.get("SBTV_ROWS_FOLD") != "0"
    out = {}
    for M, N in sweep.WAVE_SHAPES:
        assert ctx.fft_plan(M, N, 3) == dict(fc.model_plan(M, N, 3, wave_enabled=wave), fold=fold)
        for k, v in sweep.switch_runs(ctx, M, N).items():
            out["%dx%d.%s" % (M, N, k)] = v
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
