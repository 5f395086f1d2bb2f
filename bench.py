#!/usr/bin/env python3
"""Headline benchmark: SALSA outer-iterations/s (+ final PSNR) on 2048x2048 Gaussian-blur TV deblurring.

  python bench.py --gpus N --steps K --warmup W
      N = 1 runs in this process.  N > 1 without a torch.distributed environment starts the N ranks itself
      (`python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py ...` as a child process, before
      this process has imported torch or touched a GPU) and exits with the child's status.
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W          (what the driver runs; same code path as the child above)

A "step" is one SALSA_v2 outer iteration (SALSA/SALSA_v2.m:423-494: warm-started 10-iteration Chambolle TV prox +
the FFT least-squares step + residual / objective / mse / distance scalars and the host-side stopping rule) on one
2048x2048 image per GPU, inputs resident in HBM.  Exactly K steps are timed by running SALSA_v2 with MAXITERA = K and
a tolerance that is never met; the timed region is the whole C-ABI call (it includes the one-time operator set-up).
Multi-GPU: independent images shard across ranks (no data-path collective, weak scaling); RCCL is used only for the
barrier and the max-over-ranks of the elapsed time.

Prints ONE JSON line (rank 0).  A plain run sets up, runs the converged solve (final PSNR) and the untimed pre-roll, times
the K steps and prints the contract keys (metric, value, unit, higher_is_better, dtype, ms_per_step, ...), final_psnr_db,
outer_iterations_to_tol_1e-5, pre_roll_steps (every untimed iteration that ran before the timed region: converged solve,
clock ramp-up, --warmup) and switches (SBTV_* variables set).

  --dump-outputs DIR  after the timed steps, writes what the timed SALSA_v2 call returned (rank 0's image) as float64
                DIR/<name>.npy: x (the 2048x2048 image after step K, 32 MiB), objective, distance, mses, numA, numAt.
                The inputs are seeded, so two builds run with the same arguments can be compared output for output.
  --full        everything else the benchmark measures or checks, each block after the timed steps (--no-cpu-baseline,
                --no-batched, --no-extras and --no-extra-configs leave single blocks out):
  loop_ms_per_step_device  device time of the timed loop per step (sbtv_last_timing)
  roofline      the dominant kernel (temporally fused Chambolle iteration).  Five iterations share one pass over
                memory, so SURVEY.md section 8d's 5 x 40 B/px is not a bound (it exceeds the HBM peak).  Neither limit of
                the chip is saturated by a launch as a whole: `valu_issue_frac` (fp64 VALU instructions of one launch
                from the committed PMC pass of THIS source revision / live launch time / peak issue rate),
                `hbm_frac_pmc` (PMC bytes / launch time / 8 TB/s), `hbm_frac_model` (minimum traffic of the fused
                design), `useful_frac` (issue fraction spent on core pixels) and `tail_frac` (share of a launch after
                its last workgroup has entered, profiles/) stand side by side, and `split` gives the live
                fixed + per-iteration decomposition of a launch (one launch of 1..5 iterations each): the marginal
                iteration is bound by fp64 issue, the fixed part (region load / store, fill and drain) by memory
                latency.  Every fraction is <= 1 by construction.  A PMC file measured on other kernel sources is
                refused (`stale`).
  step_roofline PMC bytes of one outer iteration / measured step time / 8 TB/s (+ the fused design's byte model)
  passes        live HIP-event timings of the FFT passes and the prox on scratch data of the same shape
  extra_512     the same solve on 512x512 man.png (BASELINE configs[1]): it/s (MEDIAN of the timed runs, all listed, with
                the host-wait statistics of the slowest), PSNR, passes; with N > 1 ranks: one 512x512 image per GPU, the
                aggregate it/s (median of 3 runs, each the slowest rank between two barriers)
  extra_configs driver-timed shares of BASELINE configs[2..4] on this GPU: FISTA 2048^2 Moffat, SAPG Laplace 8 x 1024^2,
                SAPG Gaussian 4 shared chains at 2048^2
  psnr_matches_fixture  final PSNR and stopping iteration of the converged solve against the committed oracle fixture
                (tests/golden/large_configs.npz; |dPSNR| <= 1e-3 dB and the same iteration)
  cpu_baseline  the NumPy oracle on the host cores (N = 1 only)
  batched       four 2048x2048 images per GPU in one call (two lanes per context): image-iterations/s; N = 1: also the one-stream
                rate; N > 1: aggregate over the ranks (north_star: scaling on batched images)
"""
import os as _os
# Host-side thread pools must not spin while the GPU is being timed: NumPy's OpenBLAS starts up to 64 threads for one
# `np.linalg.norm` of the problem set-up and each of them busy-waits for ~100 ms afterwards; on a box whose container has
# a CPU quota (16 cores here, cgroup cpu.max) that uses up the quota of the next 100 ms periods and the kernel then holds
# EVERY thread of the container - including the one that feeds the GPU - until the period ends.  That was the "slow
# mode" of the 512 x 512 samples in round 2 (profiles/r03_slow_mode_512.md).  Set before NumPy / torch are imported.
_os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
_os.environ.setdefault("MKL_NUM_THREADS", "1")
_os.environ.setdefault("OMP_NUM_THREADS", "1")

import argparse
import glob
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd")
sys.path.insert(0, PKG)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
# fp64 vector peak: 256 CUs x 4 SIMDs x 16 fp64 lanes per clock x 2.4 GHz = 39.3 T lane-instructions/s
# (= 78.6 TFLOP/s when every instruction is an FMA; a wave64 fp64 instruction holds its SIMD for 4 cycles)
VALU_F64_PEAK_TINSTR = 256 * 4 * 16 * 2.4e9 / 1e12
SIZE = 2048
THETA = 0.03
W_TRUE = (0.4, 0.3)
FUSED_STEPS = 5                # Chambolle iterations per fused launch (TViters = 10 -> 2 launches per prox)
PMC_FILE = os.path.join(ROOT, "profiles", "pmc_current.json")


def source_sha():
    """Hash of the kernel sources: a PMC summary only describes the build it was measured on."""
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.inc"))
                    + glob.glob(os.path.join(PKG, "csrc", "*.h"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


def load_pmc():
    """profiles/pmc_current.json (tools/summarize_profiles.py) if it was measured on the current sources."""
    if not os.path.exists(PMC_FILE):
        return None, "missing"
    try:
        d = json.load(open(PMC_FILE))
    except Exception:
        return None, "unreadable"
    if d.get("source_sha256") != source_sha():
        return None, "stale (measured on other kernel sources)"
    return d, "ok"


def tiled_image(size):
    import numpy as np
    man = np.load(os.path.join(ROOT, "tests", "golden", "man_512.npy")).astype(np.float64)
    r = max(1, size // 512)
    return np.tile(man, (r, r))[:size, :size]


def make_problem(seed, size=SIZE):
    """size^2 synthetic image (man.png tiled), Gaussian PSF, BSNR 30 dB — SURVEY.md §8d.
    Data synthesis uses NumPy FFTs on the host (set-up, not the measured path)."""
    import numpy as np
    x = tiled_image(size)
    # Gaussian_psf (utils/Gaussian_psf.m) taps, blur = circular conv with taps at the top-left (resize.m)
    g = np.arange(-3, 4.0)
    V, U = np.meshgrid(g, g, indexing="ij")
    k = (W_TRUE[0] * W_TRUE[1] / (2 * np.pi)) * np.exp(-(W_TRUE[0] ** 2 * U ** 2 + W_TRUE[1] ** 2 * V ** 2) / 2)
    k /= k.sum()
    h = np.zeros_like(x)
    h[:7, :7] = k
    Ax = np.real(np.fft.ifft2(np.fft.fft2(h) * np.fft.fft2(x)))
    sigma = np.linalg.norm(Ax - Ax.mean()) / np.sqrt(x.size * 10 ** (30 / 10))      # run_Gaussian_demo.m:148
    noise = np.random.default_rng(seed).standard_normal(x.shape)
    return x, Ax + sigma * noise, sigma, noise


def psnr(x, y):
    import numpy as np
    return 10 * np.log10(x.max() ** 2) - 10 * np.log10(np.sum((x - y) ** 2) / x.size)   # utils/PSNR.m


def cpu_baseline(x, noise, budget_s=20.0):
    """The oracle (op-for-op NumPy restatement incl. the reference's redundant FFTs) on the host cores."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import sbtv_oracle as o
    st = o.demo_setup("gaussian", x, noise, evMax=1.0)
    res = o.salsa_from_estimates(st, THETA, W_TRUE, st["sigma"] ** 2, tol=0.0, outeriters=500, max_time=budget_s)
    n = res["n_outer"]
    return {"value": n / res["wall_loop"], "unit": "SALSA outer-iterations/s", "cores": o.get_workers(),
            "kind": "port",
            "sample": f"{n} outer iterations of the same 2048x2048 problem ({res['wall_loop']:.1f} s); "
                      f"scipy.fft on {o.get_workers()} threads, NumPy element-wise passes single-threaded"}


def self_launch(args, argv):
    """`python bench.py --gpus N` (N > 1) outside torch.distributed.run: start the ranks as a child process.  Nothing
    in this process has imported torch or initialised a GPU, and nothing is exec'ed: the child's status is returned."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    return subprocess.run(cmd, env=env).returncode


def model_step_bytes(size):
    """Minimum HBM bytes of one outer iteration of the fused design: 2 Chambolle launches (read g,px,py + write px,py;
    the second also writes u: 40 + 48 B/px), forward column FFT of u+bu (read 2, write S: 24), row pass (S in and out
    + the H and Y spectra of (M/2+1) x N complex each), inverse column FFT + bookkeeping (read S,u,bu,true; write
    x,bu,g: 56; at 1024 / 2048 x is not stored since round 3: 48)."""
    n1 = size // 2
    post = 48.0 if size in (1024, 2048) else 56.0
    return (40.0 + 48.0 + 24.0 + (16.0 + 16.0 * (n1 + 1) / n1) + post) * float(size * size)


def pass_block(ctx, size, names, reps):
    """Stand-alone HIP-event timings of single passes on scratch data (inputs then still sit in the caches: the
    kernels run 5-20 % slower inside the solver loop, profiles/r02_fft_lab.md)."""
    out = {}
    kind = ctx.prox_variant(size, size)["kind"]
    for nm in names:
        r = ctx.time_pass(nm, size, size, 1, reps)
        by = r["bytes"]
        if nm.startswith("prox"):
            # temporally fused prox: the bytes of the fused design (every launch reads g,px,py and writes px,py once,
            # the last one also writes f), not K x 40 B/px of an unfused sweep - that count exceeds what HBM could move
            its = 10 if nm == "prox10_warm" else 25
            per = 10 if kind == "pipeline" else FUSED_STEPS
            by = (40.0 * -(-its // per) + 8.0) * size * size
        gbs = by / (r["ms"] * 1e-3) / 1e9
        out[nm] = {"ms": r["ms"], "model_bytes": by, "achieved_gbs": gbs, "frac_of_hbm_peak": gbs / HBM_PEAK_GBS}
    return out


TIMELINE_FILE = os.path.join(ROOT, "profiles", "timeline_current.json")


def load_timeline():
    """profiles/timeline_current.json (tools/chambolle_timeline.py on the `make timeline` build): per-workgroup phase
    stamps of one launch in the loop; gives the share of a launch after its last workgroup has entered."""
    try:
        d = json.load(open(TIMELINE_FILE))
    except Exception:
        return None
    d["current_sources"] = (d.get("source_sha256") == source_sha())
    return d


def launch_split(ctx, size, reps=40):
    """Live decomposition of one fused Chambolle launch: t(K) for one launch of K = 1..5 iterations (HIP events over `reps`
    launches each, sbtv_diag_time_pass 11..15), least-squares line t = fixed + K * per_iteration."""
    try:
        ts = [ctx.time_pass("fused_steps%d" % k, size, size, 1, reps)["ms"] * 1e3 for k in range(1, FUSED_STEPS + 1)]
    except Exception as e:                       # e.g. a forced single-step / pipeline variant
        return {"error": str(e)}
    n = len(ts)
    ks = list(range(1, n + 1))
    km, tm_ = sum(ks) / n, sum(ts) / n
    slope = sum((k - km) * (t - tm_) for k, t in zip(ks, ts)) / sum((k - km) ** 2 for k in ks)
    return {"us_launch_of_k_iterations": ts, "fixed_us": tm_ - slope * km, "per_iteration_us": slope,
            "how": "one launch of K = 1..5 warm-started iterations on scratch data (no f, no control kernels), %d launches "
                   "each back to back; inputs partly cached, so `fixed_us` is a lower bound for the loop" % reps}


def chambolle_roofline(tm, size, pmc, pmc_state, kind="tile", split=None):
    """Roofline entries of the fused Chambolle kernel from the live event bracket of the timed solve."""
    P = float(size * size)
    iters = tm["chambolle_launches"]                      # Chambolle iterations actually run
    fused = 10 if kind == "pipeline" else FUSED_STEPS
    kname = "chambolle_pipe_kernel" if kind == "pipeline" else "chambolle_fused_kernel"
    launches = max(iters / fused, 1.0)
    # live HIP-event bracket of the prox launches (sampled on outer iterations 4, 36, 68, ... and scaled by the library:
    # an event record costs the stream 5-6 us); a run shorter than 4 iterations has no sample
    avg_s = max(tm["chambolle_ms"] * 1e-3 / launches, 1e-9)
    # minimum traffic of the temporally fused design: every launch reads g, px, py and writes px, py once over the
    # image; the last launch of a prox also writes f: (40 + 48) / 2 B per pixel and launch with two launches per prox,
    # 48 with one (pipeline kernel)
    model_bytes = (48.0 if kind == "pipeline" else 44.0) * P
    k = None
    if pmc:
        k = next((v for n, v in pmc.get("kernels", {}).items() if n.startswith(kname)), None)
    traffic = k.get("hbm_bytes_per_launch") if k else None
    roof = {"kernel": "%s (%d Chambolle iterations per launch)" % (kname, fused), "avg_launch_ms": avg_s * 1e3,
            "launches": launches, "iterations_per_launch": fused,
            "us_per_chambolle_iteration": 1e3 * tm["chambolle_ms"] / max(iters, 1),
            "unit": "GB/s", "peak": HBM_PEAK_GBS, "traffic": traffic, "pmc_file": pmc_state,
            "model_bytes_per_launch": model_bytes,
            "hbm_frac_model": model_bytes / avg_s / 1e9 / HBM_PEAK_GBS,
            "hbm_frac_pmc": traffic / avg_s / 1e9 / HBM_PEAK_GBS if traffic else None,
            # SURVEY.md section 8d's count for reference only: 5 iterations x 40 B/px share one pass over memory, so it is
            # NOT a bound for the fused kernel (it exceeds the HBM peak)
            "unfused_algorithmic_gbs": 40.0 * P * fused / avg_s / 1e9}
    if k and k.get("valu_insts_per_launch"):
        issued = k["valu_insts_per_launch"] * 64.0 / avg_s / 1e12       # wave instructions x 64 lanes
        roof["valu_issue_frac"] = issued / VALU_F64_PEAK_TINSTR
        roof["valu_peak_tinstr_s"] = VALU_F64_PEAK_TINSTR
        roof["valu_wave_insts_per_launch"] = k["valu_insts_per_launch"]
        # instructions spent on core pixels only (the halo of the temporal blocking is recomputed work)
        roof["useful_frac"] = roof["valu_issue_frac"] * k.get("core_fraction", 1.0)
    try:
        tl = load_timeline()
        if tl and tl.get("launch_us") and tl.get("tail_us") is not None:
            current = bool(tl.get("current_sources"))
            # a timeline measured on other sources says nothing about this build's tail: the fraction is then withheld
            roof["tail_frac"] = (tl["tail_us"] / tl["launch_us"]) if current else None
            roof["tail"] = {"launch_us": tl["launch_us"], "tail_us": tl["tail_us"], "file": "profiles/timeline_current.json",
                            "measured_on_current_sources": current}
    except Exception as e:               # an older or damaged file must not take the headline line down
        roof["tail"] = {"error": str(e)}
    if split and "per_iteration_us" in split:
        roof["split"] = dict(split)
        if k and k.get("valu_insts_per_launch"):
            # VALU instructions of one iteration = (instructions of a launch - those of its load / store / f phase) / 5;
            # the PMC pass has only the total, so the marginal issue rate is bounded from above by total / 5
            per_it = k["valu_insts_per_launch"] / fused * 64.0 / (split["per_iteration_us"] * 1e-6) / 1e12
            roof["split"]["marginal_iteration_valu_issue_frac_upper"] = min(per_it / VALU_F64_PEAK_TINSTR, 1.0)
    # primary entry in the contract's form: algorithmic bytes of one launch of THIS design (read
    # g, px, py + write px, py once per 5-iteration launch, + f on the last launch of a prox) / live launch time, with
    # the bytes the memory system really moved (PMC) as `traffic`
    roof["bound"] = "hbm"
    roof["achieved"] = model_bytes / avg_s / 1e9
    roof["achieved_is"] = "algorithmic bytes of one fused launch (44 B/px) / live launch time"
    roof["frac"] = roof["achieved"] / HBM_PEAK_GBS
    roof["note"] = ("A launch is bound by neither limit as a whole: its marginal iteration runs at the fp64 VALU issue "
                    "rate (split.per_iteration_us), its fixed part (region load / store, fill and drain of the grid, the "
                    "tail after the last workgroup has entered) waits for memory latency with the vector units idle; "
                    "valu_issue_frac, hbm_frac_pmc, useful_frac and tail_frac stand side by side "
                    "(profiles/r02_chambolle_timeline.md, profiles/r03_*).")
    return roof


def fixture_check(tag, psnr_db, n_outer):
    """Final PSNR and stopping iteration against the committed oracle fixture of the same problem
    (tests/golden/large_configs.npz, made by tests/golden/make_golden_large.py; an ORACLE output, parity unpinned against
    MATLAB).  north_star: |dPSNR| <= 1e-3 dB and the same stopping iteration."""
    import numpy as np
    path = os.path.join(ROOT, "tests", "golden", "large_configs.npz")
    try:
        with np.load(path) as f:
            want_psnr, want_n = float(f[tag + ".psnr"]), int(f[tag + ".n_outer"])
    except Exception as e:
        return {"matches": None, "error": str(e)}
    return {"matches": bool(abs(psnr_db - want_psnr) <= 1e-3 and n_outer == want_n), "fixture_psnr_db": want_psnr,
            "fixture_outer_iterations": want_n, "abs_dpsnr_db": abs(psnr_db - want_psnr),
            "fixture": "tests/golden/large_configs.npz:" + tag}


def cgroup_throttled_us():
    """Microseconds this container's threads were held back by its CPU quota so far (cgroup v2 cpu.stat), or None."""
    try:
        for ln in open("/sys/fs/cgroup/cpu.stat"):
            if ln.startswith("throttled_usec"):
                return int(ln.split()[1])
    except OSError:
        pass
    return None


def thread_cpu_ms():
    """CPU time of every thread of this process so far: {tid: (name, ms)} (/proc/self/task/*/stat, 10 ms ticks)."""
    out = {}
    tick = 1000.0 / os.sysconf("SC_CLK_TCK")
    try:
        for tid in os.listdir("/proc/self/task"):
            try:
                st = open(f"/proc/self/task/{tid}/stat").read()
            except OSError:
                continue
            f = st[st.rindex(")") + 2:].split()
            out[int(tid)] = (st[st.index("(") + 1:st.rindex(")")], (int(f[11]) + int(f[12])) * tick)
    except OSError:
        pass
    return out


def thread_cpu_delta(a, b, top=6):
    """Who used the CPU between two thread_cpu_ms() snapshots: thread count, total ms, the `top` consumers by name."""
    d = {}
    for tid, (nm, ms) in b.items():
        used = ms - a.get(tid, (nm, 0.0))[1]
        if used > 0:
            d[nm] = d.get(nm, [0, 0.0])
            d[nm][0] += 1
            d[nm][1] += used
    items = sorted(d.items(), key=lambda kv: -kv[1][1])[:top]
    return {"threads_alive": len(b), "cpu_ms_total": sum(v[1] for v in d.values()),
            "top": [{"name": k, "threads": v[0], "cpu_ms": v[1]} for k, v in items]}


def median(v):
    v = sorted(v)
    n = len(v)
    return v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2])


CONFIGS_FILE = os.path.join(ROOT, "profiles", "configs_current.json")
# Byte models of the fused design per unit and pixel (fp64; a half spectrum S or an operator spectrum = 8 B per pixel):
#   cold prox(25) = 5 Chambolle launches: 24 (read g, write px, py) + 3 x 40 + 48 (last one also writes f)      = 192
#   forward column pass 16 (+ TV partials), row pass with S in and out + two operator spectra 32, inverse column pass fused
#   with its consumer (gradient step / MYULA step) 24 / 32
CONFIG_MODELS = {
    # my_fista iteration (SALSA/my_fista.m:22-33): cols(y) 16 + rows GRADF 32 + cols^-1 with the gradient step 24 + prox 192
    # + momentum (x, x_old, true in, y out) 32 + objective: cols(x) 16 + residual rows (S, H, Y in) 24
    "3": dict(bytes_per_px=336.0, px=2048 * 2048, unit="FISTA iteration", units_per_iteration=1),
    # SAPG Laplace image-iteration, PSF moving: tap + derivative spectra written 16, rows GRADF 32, cols^-1 + MYULA step 32,
    # prox 192, cols(X) 16, gradient-sums rows (S, H, Y, D in) 32
    "4": dict(bytes_per_px=320.0, px=1024 * 1024, unit="image-iteration", units_per_iteration=8),
    # SAPG Gaussian chain-iteration, PSF fixed, 4 chains share the operator spectra (read once per row block for all
    # chains: 32 / 4): cols^-1 + MYULA 32, prox 192, cols(X) 16, rows GRAD with inverse 16 + 8
    "5": dict(bytes_per_px=264.0, px=2048 * 2048, unit="chain-iteration", units_per_iteration=4),
    # the demo's loop at 512^2 (fixed PSF, one chain): same passes, spectra not shared
    "6": dict(bytes_per_px=288.0, px=512 * 512, unit="iteration", units_per_iteration=1),
}


def config_roofline(cfg, units_per_s):
    """`roofline` of an extra_configs entry: algorithmic bytes of the fused design per unit x measured units/s against the
    HBM peak, and - from profiles/configs_current.json (tools/profile_config.sh, stamped with the hash of the kernel
    sources) - the PMC bytes of one iteration, the dominant kernel and the launches per iteration of the profiled run."""
    m = CONFIG_MODELS[cfg]
    model = m["bytes_per_px"] * m["px"]
    r = {"bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s", "model_bytes_per_" + m["unit"].replace("-", "_").replace(" ", "_"): model,
         "achieved": model * units_per_s / 1e9, "frac": model * units_per_s / 1e9 / HBM_PEAK_GBS, "traffic": None}
    try:
        d = json.load(open(CONFIGS_FILE))
        if d.get("source_sha256") != source_sha():
            r["pmc_file"] = "stale (measured on other kernel sources)"
            return r
        c = d["configs"][cfg]
        r["pmc_file"] = "ok"
        r["traffic"] = c["hbm_bytes_per_iteration"] / m["units_per_iteration"]
        r["traffic_is"] = "PMC bytes per %s (2 x FETCH_SIZE + WRITE_SIZE over the launches of one iteration of the profiled run %s)" % (m["unit"], c["tag"])
        # like `frac`: against THIS run's rate (a rate taken under the profiler is not a measurement of speed)
        r["traffic_frac"] = r["traffic"] * units_per_s / 1e9 / HBM_PEAK_GBS
        r["dominant_kernel"] = c["dominant_kernel"]
        r["dominant_kernel_share_of_gpu_time"] = c["dominant_kernel_share"]
        r["launches_per_iteration"] = c["launches_per_iteration"]
    except Exception as e:
        r["pmc_file"] = "missing (%s)" % type(e).__name__
    return r


def extra_configs(ctx, dev, iters):
    """One GPU's share of BASELINE configs[2..4], `iters` iterations each after a short pre-roll, timed by this process
    (host clock around the C-ABI call, inputs device-resident).  The code of tools/bench_sapg.py, which also runs them
    over several ranks."""
    import numpy as np
    import sbtv
    out = {}
    rng = np.random.default_rng(1)
    # configs[2]: FISTA + cold TV prox(25), 2048^2, Moffat PSF (SALSA/my_fista.m:21-56)
    x = tiled_image(2048)
    st = sbtv.demo_setup("moffat", x, rng.standard_normal(x.shape), evMax=1.0, ctx=ctx)
    A = sbtv.BlurOperator(sbtv.psf_moffat(7, 0.4, 3.5), ctx=ctx)
    yd, xd = sbtv.to_device(st["y"], dev), sbtv.to_device(x, dev)
    tau = 0.03 * st["sigma"] ** 2
    fista = lambda n: sbtv.my_fista(yd, A, A.T, tau, 1.0, sbtv.TVnorm, sbtv.Psi_TV(25), 1, -1.0, n, xd, ctx=ctx)
    fista(6)
    ctx.sync()
    t0 = time.perf_counter()
    fista(iters + 1)
    ctx.sync()
    dt = time.perf_counter() - t0
    out["fista_2048_moffat"] = {"workload": "my_fista + cold Chambolle(25), 2048x2048, Moffat PSF (configs[2])",
                                "value": iters / dt, "unit": "FISTA iterations/s", "steps": iters,
                                "ms_per_iteration": 1e3 * dt / iters, "roofline": config_roofline("3", iters / dt)}
    del yd, xd

    def sapg(kind, size, nunits, share, its=None, img=None):
        iters_ = iters if its is None else its
        xx = tiled_image(size) if img is None else img
        s2 = sbtv.demo_setup(kind, xx, rng.standard_normal(xx.shape), evMax=0.99, ctx=ctx)
        d = {"gaussian": dict(names=("w1", "w2"), init=(0.5, 0.3), pmin=(0.1, 0.1), pmax=(1.0, 1.0), fix=(1, 1),
                              c=dict(theta=0.01, w1=10.0, w2=10.0, sigma=1000.0)),
             "laplace": dict(names=("b",), init=(0.1,), pmin=(1e-3,), pmax=(1.0,), fix=(0,),
                             c=dict(theta=0.01, b=100.0, sigma=1e4))}[kind]
        op = dict(samples=iters_ + 1, warmup=0, burnIn=2, psf_size=7, phi=0.0, gamma=s2["gamma"], th_init=0.01,
                  min_th=1e-3, max_th=1.0, sigma=s2["sigma"], sigma_init=s2["sigma_init"], sigma_min=s2["sigma_min"],
                  sigma_max=s2["sigma_max"], d_scale=1.0, d_exp=0.8, fix_sigma=0)
        op["lambda"] = s2["lambda"]
        for q, nm in enumerate(d["names"]):
            op[nm] = s2["p_true"][q]
            op[nm + "_init"] = s2["p_true"][q] if d["fix"][q] else d["init"][q]
            op["min_" + nm], op["max_" + nm], op["fix_" + nm] = d["pmin"][q], d["pmax"][q], d["fix"][q]
        c = dict(d["c"], lam=1.0, gam=1.0)
        fn = sbtv.SAPG_algorithm_laplace if kind == "laplace" else sbtv.SAPG_algorithm_Guassian
        if share:
            op["chains"] = nunits
            yy = sbtv.to_device(s2["y"], dev)
            kw = dict(share_gradients=True, ctx=ctx)
        else:
            yy = sbtv.to_device(np.stack([s2["y"]] * nunits), dev)
            kw = dict(ctx=ctx)
        fn(yy, dict(op, samples=3), c, **kw)
        ctx.sync()
        t1 = time.perf_counter()
        fn(yy, op, c, **kw)
        ctx.sync()
        e = time.perf_counter() - t1
        return e

    # several devices behind ONE process through the C-ABI (sbtv_group): on this one-GPU run two VIRTUAL shards on the same
    # device (two host threads, two contexts), 4 images of the headline problem dealt 2 + 2, host (NumPy) buffers as a MATLAB
    # host would pass them - what the group path costs and gains when it has no second GPU to use
    try:
        x1, y1, s1, _ = make_problem(seed=1)
        g = sbtv.Group([ctx.device, ctx.device])
        Ag = sbtv.BlurOperator(sbtv.Gaussian_psf(7, *W_TRUE), ctx=ctx)
        mu_g, tau_g = THETA / 10, THETA * s1 ** 2
        # column-major images, as a MATLAB host holds them: the mirror then passes the buffers on without a layout copy
        ys = np.stack([np.ascontiguousarray(y1.T)] * 4).transpose(0, 2, 1)
        xs = np.stack([np.ascontiguousarray(x1.T)] * 4).transpose(0, 2, 1)
        run = lambda n: sbtv.SALSA_v2(ys, Ag, tau_g, "MU", mu_g, "AT", Ag.T, "LS", Ag.LS(mu_g), "True_x", xs, "StopCriterion", 1,
                                      "ToleranceA", -1.0, "MAXITERA", n, "TVINITIALIZATION", 1, "TViters", 10, ctx=g)
        run(5)
        # two call lengths: the slope is the loop, the intercept the fixed part of a call = the host <-> device copies of the
        # four images from / to pageable memory (tools/bench_group.py; with row-major NumPy images the mirror's layout
        # conversion adds ~300 ms)
        n_a, n_b = 50, 250
        t1 = time.perf_counter()
        run(n_a)
        t2 = time.perf_counter()
        run(n_b)
        t3 = time.perf_counter()
        # the fixed part of a call measured directly: calls of 2 iterations (the intercept of two call lengths also holds
        # whatever is not linear in the iteration count - the first iterations of a call run exact launches and on lower
        # clocks - and came out at twice this, tools/bench_hostcall.py)
        short_calls = []
        for _ in range(3):
            ts = time.perf_counter()
            run(2)
            short_calls.append(time.perf_counter() - ts)
        g.close()
        slope = ((t3 - t2) - (t2 - t1)) / (n_b - n_a)
        out["group_2_virtual_shards_4x2048"] = {
            "workload": "sbtv_SALSA_v2_sharded: 4 images of the headline problem over a group of two contexts on THIS GPU "
                        "(virtual shards: two host threads, no second device to gain from), host buffers in and out",
            "value": 4.0 / slope, "unit": "image-iterations/s", "value_is": "slope between calls of %d and %d outer iterations" % (n_a, n_b),
            "ms_per_iteration": 1e3 * slope, "fixed_ms_per_call": 1e3 * (median(short_calls) - 2 * slope),
            "fixed_ms_per_call_is": "median of 3 calls of 2 outer iterations, minus 2 iterations: 268 MB in and 134 MB out of "
                                    "pageable host memory through the copy lanes (csrc/ctx.hip stage_copy) + the Python mirror",
            "intercept_of_the_two_call_lengths_ms": 1e3 * ((t2 - t1) - n_a * slope),
            "calls_ms": [1e3 * (t2 - t1), 1e3 * (t3 - t2)], "short_calls_ms": [1e3 * t for t in short_calls]}
        del ys, xs
    except Exception as e:               # the group path must not take the headline line down with it
        out["group_2_virtual_shards_4x2048"] = {"error": str(e)}

    e = sapg("laplace", 1024, 8, False)
    ctx.set_lanes(1)
    e1 = sapg("laplace", 1024, 8, False)
    ctx.set_lanes(0)
    out["sapg_laplace_8x1024"] = {"workload": "SAPG_algorithm_laplace, chambolleit 25, 8 independent 1024x1024 images in one "
                                              "call = one GPU's share of the 64 of configs[3], device Philox noise",
                                  "value": 8 * iters / e, "unit": "image-iterations/s", "steps": iters,
                                  "ms_per_iteration": 1e3 * e / iters, "value_is": "two lanes (the default)",
                                  "one_stream": 8 * iters / e1, "roofline": config_roofline("4", 8 * iters / e)}
    e = sapg("gaussian", 2048, 4, True)
    ctx.set_lanes(2)                      # the chains split 2 + 2 over the lanes, six gradient sums exchanged in-stream
    e2 = sapg("gaussian", 2048, 4, True)
    ctx.set_lanes(0)
    out["sapg_gaussian_4_shared_chains_2048"] = {
        "workload": "SAPG_algorithm_Guassian, 4 MYULA chains on one 2048x2048 image with chain-averaged gradients = one "
                    "GPU's share of the 32 of configs[4] (fix_w1 = fix_w2 = 1 as run_Gaussian_demo.m:42-43), device "
                    "Philox noise", "value": 4 * iters / e, "unit": "chain-iterations/s", "steps": iters,
        "ms_per_iteration": 1e3 * e / iters, "value_is": "one stream (the default for chains that exchange gradients)",
        "split_over_two_lanes": 4 * iters / e2, "roofline": config_roofline("5", 4 * iters / e)}
    # the SAPG loop of the demos themselves (run_Gaussian_demo.m:47-50,199: 15 000 warm-up + 20 000 iterations on the
    # 512 x 512 wheel.png, PSF fixed): 2 000 iterations of it here, the whole 35 000 in profiles/r04_demo_wheel512_*.log
    wheel = np.load(os.path.join(ROOT, "tests", "golden", "wheel_512.npy")).astype(np.float64)
    n_demo = 2000
    e = sapg("gaussian", 512, 1, False, its=n_demo, img=wheel)
    out["sapg_demo_512"] = {"workload": "SAPG_algorithm_Guassian as run_Gaussian_demo.m:199 runs it: ONE chain on the 512x512 "
                                        "wheel.png, chambolleit 25, fix_w1 = fix_w2 = 1, device Philox noise, device-resident "
                                        "parameter loop", "value": n_demo / e, "unit": "SAPG iterations/s", "steps": n_demo,
                            "ms_per_iteration": 1e3 * e / n_demo, "roofline": config_roofline("6", n_demo / e),
                            "whole_demo_logs": "profiles/r04_demo_wheel512_{gaussian,moffat,laplace}.log"}
    return out


def dump_outputs(path, out):
    """--dump-outputs: the arrays the timed SALSA_v2 call returned to its caller, one float64 .npy each (x: 32 MiB).
    `times` is left out: wall-clock readings of the iterations, not a result of the computation."""
    import numpy as np
    import sbtv
    os.makedirs(path, exist_ok=True)
    x, numA, numAt, objective, distance, _times, mses = out
    for name, a in (("x", sbtv.to_host(x)), ("objective", objective), ("distance", distance), ("mses", mses),
                    ("numA", numA), ("numAt", numAt)):
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def dry_run(args, rank, world):
    """Rendezvous + barrier + max-reduction of a fake time without touching a GPU (tests of the launch path)."""
    import torch
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
        dist.barrier()
    t = torch.tensor([0.001 * (rank + 1)], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if rank == 0:
        print(json.dumps({"metric": "dry run (no GPU work)", "dry_run": True, "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "max_elapsed_s": float(t.item())}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def group_mode(args):
    """`--group`: ONE process, `sbtv.Group(range(N))`, one image per device through sbtv_SALSA_v2_sharded_dev (device-resident
    images, one host thread per device inside the library, no torch.distributed, no RCCL) - the path a single MATLAB / C host
    takes to a whole node.  Same problem, same pre-roll and the same timed call length as the multi-process mode, so that the
    two can be compared the day a multi-GPU node runs them.  `--all-ranks-on-device0` puts every shard on GPU 0 (rehearsal)."""
    import numpy as np
    import torch
    import sbtv
    n = max(1, args.gpus)
    devices = [0] * n if args.all_ranks_on_device0 else list(range(n))
    g = sbtv.Group(devices)
    probs = [make_problem(seed=1 + r) for r in range(n)]
    ys = [sbtv.to_device(p[1][None], f"cuda:{d}") for p, d in zip(probs, devices)]
    xs = [sbtv.to_device(p[0][None], f"cuda:{d}") for p, d in zip(probs, devices)]
    taps = sbtv.Gaussian_psf(7, *W_TRUE)
    mu = THETA / 10
    taus = [THETA * p[2] ** 2 for p in probs]
    solve = lambda k, tol: g.SALSA_v2_device(ys, taps, taus, mu, k, 10, tol, 1, xs)
    xg, obj, n_out = solve(500, 1e-5)
    import gc
    gc.collect()
    gc.disable()
    solve(300, -1.0)
    if args.warmup > 0:
        solve(args.warmup, -1.0)
    for d in set(devices):
        torch.cuda.synchronize(d)
    t0 = time.perf_counter()
    _, obj_t, n_t = solve(args.steps, -1.0)
    for d in set(devices):
        torch.cuda.synchronize(d)
    elapsed = time.perf_counter() - t0
    gc.enable()
    assert all(int(k) == args.steps for k in n_t)
    psnr0 = psnr(probs[0][0], sbtv.to_host(xg[0])[0])
    # north_star's second size at this GPU count: one 512 x 512 image per shard
    p5 = [make_problem(seed=1 + r, size=512) for r in range(n)]
    y5 = [sbtv.to_device(p[1][None], f"cuda:{d}") for p, d in zip(p5, devices)]
    x5 = [sbtv.to_device(p[0][None], f"cuda:{d}") for p, d in zip(p5, devices)]
    tau5 = [THETA * p[2] ** 2 for p in p5]
    solve5 = lambda k: g.SALSA_v2_device(y5, taps, tau5, mu, k, 10, -1.0, 1, x5)
    solve5(60)
    s5 = []
    for _ in range(3):
        for d in set(devices):
            torch.cuda.synchronize(d)
        t5 = time.perf_counter()
        solve5(400)
        for d in set(devices):
            torch.cuda.synchronize(d)
        s5.append(time.perf_counter() - t5)
    virtual = len(set(devices)) < n
    line = {"metric": "SALSA outer-iters/sec + final PSNR, 2048x2048 Gaussian blur", "value": n * args.steps / elapsed,
            "unit": "SALSA outer-iterations/s", "n_gpus": len(set(devices)), "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "SALSA_v2 TV deblur (TViters=10, mu=theta/10, tau=theta*sigma^2, theta=0.03), one 2048x2048 "
                                   "image per shard, device-resident", "image": [SIZE, SIZE], "shards": n, "devices": devices,
                       "parallelism": f"single process, sbtv_group of {n} contexts (one host thread per shard, no RCCL)"},
            "extra_512": {"workload": "the same solve on one 512x512 man.png per shard", "image": [512, 512], "steps": 400,
                          "value": n * 400 / median(s5), "unit": "SALSA outer-iterations/s", "value_is": "median of 3 calls",
                          "samples_it_per_s": [n * 400 / e for e in s5]},
            "mode": "group", "virtual_shards_on_one_gpu": virtual,
            "measured_on_multi_gpu_hardware": (not virtual) and n > 1,
            "final_psnr_db": psnr0, "outer_iterations_to_tol_1e-5": int(n_out[0]),
            "psnr_matches_fixture": fixture_check("salsa2048", psnr0, int(n_out[0])),
            "pre_roll_steps": {"converged_solve": int(n_out[0]), "clock_rampup": 300, "warmup": args.warmup},
            "switches": sbtv.switches()}
    print(json.dumps(line), flush=True)
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="also the auxiliary blocks: rooflines, fixture check, 512x512 and batched rates, configs[2..4], "
                         "CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the arrays the timed call returned (rank 0) as DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-batched", action="store_true", help="skip the auxiliary 4-image batch measurement")
    ap.add_argument("--no-extras", action="store_true", help="skip the 512x512 block and the per-pass timings")
    ap.add_argument("--no-extra-configs", action="store_true", help="skip the configs[2..4] block")
    ap.add_argument("--extra-iters", type=int, default=60, help="iterations per configs[2..4] measurement")
    ap.add_argument("--cpu-budget", type=float, default=20.0)
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL, default) or gloo (rehearsal on one GPU)")
    ap.add_argument("--all-ranks-on-device0", action="store_true", help="rehearsal: every rank uses cuda:0")
    ap.add_argument("--dry-run", action="store_true", help="launch path only: rendezvous, barrier, one JSON line")
    ap.add_argument("--group", action="store_true", help="single process: one sbtv.Group over --gpus devices (sbtv_SALSA_v2_sharded_dev)")
    args = ap.parse_args()
    if args.dump_outputs and (args.group or args.dry_run):
        ap.error("--dump-outputs needs the timed path of the multi-process mode (not --group / --dry-run)")
    if args.group:
        return group_mode(args)

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args, sys.argv[1:]))        # before anything imports torch / touches the GPU

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    args.gpus = world
    if args.dry_run:
        return dry_run(args, rank, world)

    import numpy as np
    import torch
    import torch.distributed as dist
    import sbtv

    if args.all_ranks_on_device0:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = f"cuda:{local_rank}"
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(dev))   # RCCL over xGMI
        else:
            dist.init_process_group(args.dist_backend)

    ctx = sbtv.Context(local_rank)
    x, y, sigma, noise = make_problem(seed=1 + rank)      # each rank deblurs its own image
    yd, xd = sbtv.to_device(y, dev), sbtv.to_device(x, dev)
    A = sbtv.BlurOperator(sbtv.Gaussian_psf(7, *W_TRUE), ctx=ctx)
    mu, tau = THETA / 10, THETA * sigma ** 2

    def solve(maxit, tol, yv=None, xv=None, tau_=None):
        return sbtv.SALSA_v2(yd if yv is None else yv, A, tau if tau_ is None else tau_, "MU", mu, "AT", A.T,
                             "LS", A.LS(mu), "True_x", xd if xv is None else xv, "StopCriterion", 1,
                             "ToleranceA", tol, "MAXITERA", maxit, "TVINITIALIZATION", 1, "TViters", 10, ctx=ctx)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        ctx.sync()

    # untimed: converged solve for the PSNR half of the metric (reference settings: tol 1e-5, <= 500 its).  Its result
    # stays on the device; the host-side PSNR arithmetic waits until after the timed region, so that the GPU goes from
    # this solve through the warm-up steps into the timed steps without an idle stretch (clock ramp-down) in between.
    xg, numA, numAt, obj, dist_, times, mses = solve(500, 1e-5)
    n_conv = len(obj) - 1

    # untimed: bring the GPU to its sustained clocks.  A step takes 0.24 ms, so the W warm-up steps alone (1-2 ms after the
    # 8 ms of the converged solve) leave the first timed call on a clock ramp that costs it ~4 % (measured: loop times of
    # three identical back-to-back 20-step calls 4.94 / 4.82 / 4.75 ms); 300 more untimed iterations (~75 ms) remove that.
    # Every rank does the same, so that N > 1 runs are measured in the same state as N = 1.
    RAMPUP = 300
    # (no Python garbage collection inside the timed call: with --steps 20 it is ONE 4.4 ms call, and a generation-2 pass over
    # the objects torch and numpy have created would cost a sizeable fraction of that.  Collected HERE, before the ramp-up:
    # a collection right in front of the timed call leaves the GPU idle for tens of milliseconds and the call then runs on a
    # lower clock - measured: 3 900 instead of 4 600 it/s)
    import gc
    gc.collect()
    gc.disable()
    solve(RAMPUP, -1.0)
    if args.warmup > 0:
        solve(args.warmup, -1.0)
    barrier()
    t0 = time.perf_counter()
    out = solve(args.steps, -1.0)          # tolA < 0: the stop rule never fires -> exactly K outer iterations
    barrier()
    elapsed = time.perf_counter() - t0
    gc.enable()
    assert len(out[3]) - 1 == args.steps
    tm = ctx.last_timing() if args.full else None
    final_psnr = psnr(x, sbtv.to_host(xg))
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, out)

    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if args.dist_backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # N > 1: north_star asks for the 512 x 512 throughput at every GPU count as well - every rank times the same 400-step
    # solve of its own 512^2 image between barriers, the slowest rank counts (no per-sample host statistics here)
    multi_512 = None
    if world > 1 and args.full and not args.no_extras:
        x5m, y5m, s5m, _ = make_problem(seed=1 + rank, size=512)
        y5md, x5md = sbtv.to_device(y5m, dev), sbtv.to_device(x5m, dev)
        tau5m = THETA * s5m ** 2
        k5m = 400
        solve(60, -1.0, y5md, x5md, tau5m)
        samples = []
        for _ in range(3):
            barrier()
            t5 = time.perf_counter()
            solve(k5m, -1.0, y5md, x5md, tau5m)
            barrier()
            e5m = torch.tensor([time.perf_counter() - t5], dtype=torch.float64,
                               device=dev if args.dist_backend == "nccl" else "cpu")
            dist.all_reduce(e5m, op=dist.ReduceOp.MAX)
            samples.append(float(e5m.item()))
        multi_512 = {"workload": "the same SALSA_v2 solve on one 512x512 man.png per GPU (BASELINE configs[1])", "image": [512, 512],
                     "value": world * k5m / median(samples), "unit": "SALSA outer-iterations/s", "steps": k5m, "n_gpus": world,
                     "value_is": "median of 3 timed runs, each the slowest rank between two barriers",
                     "samples_it_per_s": [world * k5m / e for e in samples]}

    # ... and north_star's "scaling on batched images": four 2048 x 2048 images per GPU in one call (two lanes per context)
    multi_batched = None
    if world > 1 and args.full and not args.no_batched:
        nbm, kbm = 4, 100
        ybm, xbm = sbtv.to_device(np.stack([y] * nbm), dev), sbtv.to_device(np.stack([x] * nbm), dev)
        solve(10, -1.0, ybm, xbm)
        samples = []
        for _ in range(3):
            barrier()
            tb = time.perf_counter()
            solve(kbm, -1.0, ybm, xbm)
            barrier()
            eb = torch.tensor([time.perf_counter() - tb], dtype=torch.float64, device=dev if args.dist_backend == "nccl" else "cpu")
            dist.all_reduce(eb, op=dist.ReduceOp.MAX)
            samples.append(float(eb.item()))
        multi_batched = {"images_per_gpu": nbm, "steps": kbm, "n_gpus": world, "unit": "image-iterations/s",
                         "value": world * nbm * kbm / median(samples), "samples": [world * nbm * kbm / e for e in samples],
                         "value_is": "median of 3 calls, each the slowest rank between two barriers; two lanes per context"}
        del ybm, xbm

    extras = rank == 0 and world == 1 and args.full and not args.no_extras
    # auxiliary, outside the timed region: the same solve on a batch of 4 independent images in one call (the
    # natural unit when many images share a GPU); reported as image-iterations/s, never as `value`
    batched = None
    if rank == 0 and world == 1 and args.full and not args.no_batched:
        nb, ksteps = 4, max(100, args.steps // 4)
        yb = sbtv.to_device(np.stack([y] * nb), dev)          # column-major image memory per image
        xb = sbtv.to_device(np.stack([x] * nb), dev)

        def batch_rate(reps=3):
            solve(10, -1.0, yb, xb)
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                tb = time.perf_counter()
                solve(ksteps, -1.0, yb, xb)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - tb)
            return [nb * ksteps / t for t in ts]
        two = batch_rate()                                    # default: the batch dealt to the context's two lanes
        ctx.set_lanes(1)
        one = batch_rate()                                    # one stream, as before round 4
        ctx.set_lanes(0)
        batched = {"images_per_call": nb, "steps": ksteps, "unit": "image-iterations/s", "value": median(two),
                   "value_is": "median of 3 calls; two lanes (include/sbtv.h sbtv_ctx_set_lanes, the default)",
                   "samples": two, "one_stream": {"value": median(one), "samples": one},
                   "step_roofline_frac": median(two) * model_step_bytes(SIZE) / 1e9 / HBM_PEAK_GBS}
        del yb, xb

    if rank == 0:
        value = world * args.steps / elapsed
        ms_per_step = 1e3 * elapsed / args.steps
        line = {
            "metric": "SALSA outer-iters/sec + final PSNR, 2048x2048 Gaussian blur",
            "value": value, "unit": "SALSA outer-iterations/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            # (`workload` stays under 120 characters: the driver's parser keeps that much of it)
            "config": {"workload": "SALSA_v2 TV deblur, one 2048x2048 image per GPU, Gaussian PSF 7x7, BSNR 30 dB, TViters=10",
                       "workload_detail": "SALSA_v2 TV deblur (TViters=10, mu=theta/10, tau=theta*sigma^2, theta=0.03), "
                                          "one 2048x2048 image per GPU (man.png tiled 4x4), Gaussian PSF 7x7 w=(0.4,0.3), "
                                          "BSNR 30 dB; independent images shard across GPUs",
                       "image": [SIZE, SIZE], "images_per_gpu": 1, "parallelism": f"images x{world}",
                       # every iteration of the TV prox runs; what its optimistic launches shorten is the error SUM the stop
                       # rule is checked with afterwards (a lower bound over a subset of the pixels proves "did not fire";
                       # otherwise the solve repeats exactly): profiles/r03_chambolle_errsubset.md, SBTV_ERR_SUBSET=0 = full sums
                       "prox_stop_rule": "exact (chambolle_prox_TV_stop.m:131), checked after the launches on lower-bound step sums"},
            "final_psnr_db": final_psnr, "outer_iterations_to_tol_1e-5": n_conv,
            # every untimed iteration this rank ran before the timed region
            "pre_roll_steps": {"converged_solve": n_conv, "clock_rampup": RAMPUP, "warmup": args.warmup,
                               "total": n_conv + RAMPUP + args.warmup},
            "world_size_seen": dist.get_world_size() if world > 1 else 1,
            "backend": dist.get_backend() if world > 1 else None,
            "switches": sbtv.switches(),
        }
        if args.full:
            # rank 0 solves the problem of the committed fixture (seed 1): the PSNR half of the metric, checked
            line["psnr_matches_fixture"] = fixture_check("salsa2048", final_psnr, n_conv)
            pmc, pmc_state = load_pmc()
            line["loop_ms_per_step_device"] = tm["loop_ms"] / args.steps
            line["roofline"] = chambolle_roofline(tm, SIZE, pmc, pmc_state, ctx.prox_variant(SIZE, SIZE)["kind"],
                                                  launch_split(ctx, SIZE) if extras else None)
            # step level: bytes the whole outer iteration moves / measured step time
            model_step = model_step_bytes(SIZE)
            step = {"bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s", "model_bytes_per_step": model_step,
                    "model": "fused design per outer iteration: 2 Chambolle launches (40 + 48 B/px), forward column FFT of "
                             "u+bu (24), row pass with H and Y (48), inverse column FFT + bookkeeping (56)",
                    "achieved": model_step / (ms_per_step * 1e-3) / 1e9}
            step["frac"] = step["achieved"] / HBM_PEAK_GBS
            if pmc and pmc.get("bytes_per_outer_iteration"):
                step["traffic"] = pmc["bytes_per_outer_iteration"]
                step["traffic_frac"] = step["traffic"] / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS
            line["step_roofline"] = step
        if extras:
            line["passes"] = pass_block(ctx, SIZE, ("cols_fwd", "rows_salsa", "cols_inv_post", "prox10_warm"), 50)
            # BASELINE configs[1] / north_star: the same solve on 512 x 512 man.png
            x5, y5, s5, _ = make_problem(seed=1, size=512)
            y5d, x5d = sbtv.to_device(y5, dev), sbtv.to_device(x5, dev)
            tau5 = THETA * s5 ** 2
            r5 = solve(500, 1e-5, y5d, x5d, tau5)
            k5 = max(4 * args.steps, 400)
            solve(50, -1.0, y5d, x5d, tau5)
            samples5, hstats5 = [], []
            for _ in range(5):       # launch-bound regime: every sample is listed, the MEDIAN is the value
                torch.cuda.synchronize()
                thr0 = cgroup_throttled_us()
                tc0 = thread_cpu_ms()
                t5 = time.perf_counter()
                solve(k5, -1.0, y5d, x5d, tau5)
                torch.cuda.synchronize()
                samples5.append(time.perf_counter() - t5)
                hs = ctx.last_host_stats()
                thr1 = cgroup_throttled_us()
                hstats5.append({"waits_slept": int(hs["waits_slept"]), "sleeps": int(hs["sleeps"]),
                                "stream_queries": int(hs["stream_queries"]), "wait_max_us": 1e6 * hs["wait_max_s"],
                                "wait_max_outer": int(hs["wait_max_outer"]),
                                "enqueue_max_us": 1e6 * hs["enqueue_max_s"], "device_ms": ctx.last_timing()["loop_ms"],
                                "thread_ctx_switches_vol_invol": [int(hs["nvcsw"]), int(hs["nivcsw"])],
                                "thread_page_faults_minor_major": [int(hs["minflt"]), int(hs["majflt"])],
                                "cgroup_throttled_us": None if thr1 is None or thr0 is None else thr1 - thr0,
                                "thread_cpu": thread_cpu_delta(tc0, thread_cpu_ms())})
            e5 = median(samples5)
            tm5 = ctx.last_timing()
            # 16 independent 512x512 images in one call (the unit when many small images share a GPU): every launch
            # carries 16 images, so the chain of dependent kernels is as long as for one image
            nb5, kb5 = 16, 200
            y5b, x5b = sbtv.to_device(np.stack([y5] * nb5), dev), sbtv.to_device(np.stack([x5] * nb5), dev)
            solve(20, -1.0, y5b, x5b, tau5)
            sb5 = []
            for _ in range(3):
                torch.cuda.synchronize()
                t5 = time.perf_counter()
                solve(kb5, -1.0, y5b, x5b, tau5)
                torch.cuda.synchronize()
                sb5.append(time.perf_counter() - t5)
            eb5 = median(sb5)
            del y5b, x5b
            line["extra_512"] = {
                "workload": "the same SALSA_v2 solve on 512x512 man.png (BASELINE configs[1])", "image": [512, 512],
                "value": k5 / e5, "unit": "SALSA outer-iterations/s", "steps": k5, "ms_per_step": 1e3 * e5 / k5,
                "samples_it_per_s": [k5 / e for e in samples5], "value_is": "median of 5 timed runs",
                "best_it_per_s": k5 / min(samples5), "host_wait_stats_per_sample": hstats5,
                "final_psnr_db": psnr(x5, sbtv.to_host(r5[0])), "outer_iterations_to_tol_1e-5": len(r5[3]) - 1,
                "psnr_matches_fixture": fixture_check("salsa512", psnr(x5, sbtv.to_host(r5[0])), len(r5[3]) - 1),
                "us_per_chambolle_iteration": 1e3 * tm5["chambolle_ms"] / max(tm5["chambolle_launches"], 1),
                "step_roofline": {"bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "model_bytes_per_step": model_step_bytes(512),
                                  "achieved": model_step_bytes(512) / (e5 / k5) / 1e9,
                                  "frac": model_step_bytes(512) / (e5 / k5) / 1e9 / HBM_PEAK_GBS,
                                  "note": "a 512x512 working set (2 MiB per array) lives in L2 / Infinity Cache and the "
                                          "iteration is a chain of 5 dependent kernels of 5-14 microseconds, each a "
                                          "single round of workgroups: bound by their latency, not by bandwidth"},
                "batched_16": {"images_per_call": nb5, "steps": kb5, "unit": "image-iterations/s",
                               "value": nb5 * kb5 / eb5, "ms_per_step": 1e3 * eb5 / kb5, "value_is": "median of 3 timed runs",
                               "samples": [nb5 * kb5 / e for e in sb5],
                               "step_roofline_frac": nb5 * model_step_bytes(512) / (eb5 / kb5) / 1e9 / HBM_PEAK_GBS},
                "passes": pass_block(ctx, 512, ("cols_fwd", "rows_salsa", "cols_inv_post", "prox10_warm"), 200)}
        if multi_512:
            line["extra_512"] = multi_512
        if batched or multi_batched:
            line["batched"] = batched or multi_batched
        if extras and not args.no_extra_configs:
            try:
                line["extra_configs"] = extra_configs(ctx, dev, args.extra_iters)
            except Exception as e:           # an auxiliary block must not take the headline line down with it
                line["extra_configs"] = {"error": repr(e)}
        if world == 1 and args.full and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(x, noise, args.cpu_budget)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
