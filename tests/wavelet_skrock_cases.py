"""The SK-ROCK runs shared by tests/test_wavelet_skrock_cpu.py and tests/test_gpu_wavelet_skrock.py.  Problems and injected
normals are those of tests/wavelet_posterior_cases.py (unchanged); a run adds the stage count and the number of samples.  The
step is delta = 0.8 l_s / (1 / sigma2 + 1 / lambda) at the call's smallest sigma2 (||B|| = 1: a normalised non-negative PSF, a
tight frame).  Each reference (tests/wavelet_skrock_restatement.py) is computed once per session and never modified."""
import functools

import wavelet_posterior_cases as wpc
import wavelet_skrock_restatement as wkr

ETA = 0.05

# (case of wavelet_posterior_cases, stages, samples)
RUNS = [("a", 2, 5), ("a", 3, 5), ("a", 10, 5), ("b", 3, 4), ("c", 2, 4), ("d", 3, 3), ("e", 2, 3), ("a", 2, 2)]


def options(name, stages, samples):
    """op of a run: samples, stages, lambda, delta, eta."""
    p = wpc.problem(name)
    lam = p["op"]["lambda"]
    delta = 0.8 * wkr.max_step(stages, ETA, float(min(p["sigma2"])), lam)
    return {"samples": samples, "stages": stages, "lambda": lam, "delta": delta, "eta": ETA}


def noise(name, samples):
    """(samples-1, B, M, (3J+1) N): the first steps of the case's injected normals."""
    return wpc.noise(name, samples)


def chain(name, b, stages, samples, nz):
    """The restatement on chain b of a case with noise nz (steps, M, (3J+1) N)."""
    p = wpc.problem(name)
    return wkr.skrock_wavelet_chain(p["y"][b], p["H"], p["h"], p["levels"], options(name, stages, samples),
                                    float(p["theta"][b]), float(p["sigma2"][b]), nz)


@functools.lru_cache(maxsize=None)
def reference(name, stages, samples):
    """The restatement on every chain of the run (read-only for its users)."""
    nz = noise(name, samples)
    return [chain(name, b, stages, samples, nz[:, b]) for b in range(wpc.problem(name)["batch"])]
