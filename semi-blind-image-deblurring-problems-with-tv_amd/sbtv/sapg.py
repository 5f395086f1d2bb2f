"""Host mirror of SAPG/SAPG_algorithm_{Guassian,moffat,laplace}.m, utils/max_eigenval_*.m and the
data-synthesis / step-size block of run_*_demo.m, over the device-resident MYULA/SAPG loop.

`op` is the reference's option struct (a dict or any attribute bag with the same field names);
its function handles (op.gradF, op.proxG, op.logPi, ...) are not used: the C-ABI rebuilds them
from the PSF family, `y` and the scalar fields.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from .operators import BlurOperator, psf_family

_KIND = {"gaussian": 0, "moffat": 1, "laplace": 2}


def _get(op, name, default=None):
    if isinstance(op, dict):
        return op.get(name, default)
    return getattr(op, name, default)


def max_eigenval(A, At, params, im_size, tol, max_iter, verbose=0, x0=None, ctx=None):
    """val = max_eigenval(A, At, a, b, im_size, tol, max_iter, verbose)
    (utils/max_eigenval_Gaussian_Moffat.m:1-27, utils/max_eigenval_Laplace.m:1-28).
    A: callable (x, *params) -> BlurOperator application is not needed: pass A as a
    sbtv.BlurOperator built at `params` (At is then ignored).  x0: start vector
    (the reference draws randn(im_size); MATLAB's stream is unpinned -> pass it explicitly)."""
    ctx = ctx or L.default_context()
    if not isinstance(A, BlurOperator):
        raise TypeError("A must be a sbtv.BlurOperator built at the requested parameters")
    if x0 is None:
        x0 = np.random.default_rng(0).standard_normal(im_size)
    xi = L.Images(x0)
    taps = A._cm(1)
    val = C.c_double(0.0)
    it = C.c_int(0)
    ctx.check(ctx.lib.sbtv_max_eigenval(ctx.h, L.vptr(taps), A.taille, xi.ptr, xi.M, xi.N,
                                        float(tol), int(max_iter), C.byref(val), C.byref(it), xi.flags), xi.flags)
    if verbose:
        print(f"Norm = {val.value:e} ({it.value} iterations)")
    return val.value


def demo_setup(kind, x, noise, evMax, BSNR=30.0, true_params=None, BSNR_min=None, BSNR_max=None, lambdaMax=None,
               gammaFrac=0.98, th_init=0.01, ctx=None):
    """The observation model and MYULA step sizes of run_Gaussian_demo.m:145-184,
    run_moffat_demo.m:139-176, run_laplace_demo.m:109-142 (blur on the GPU, scalars on the host).
    Returns a dict with y, sigma, sigma_min/max/init (variances), Lf, lambda, gamma."""
    defaults = {"gaussian": dict(true=(0.4, 0.3), bmin=15, bmax=45, lmax=2.0, lf=min, gmul=1.0),
                "moffat": dict(true=(0.4, 3.5), bmin=18, bmax=35, lmax=2.0, lf=min, gmul=1.0),
                "laplace": dict(true=(0.3,), bmin=15, bmax=45, lmax=0.1, lf=max, gmul=10.0)}[kind]
    p = tuple(defaults["true"] if true_params is None else true_params)
    bmin = defaults["bmin"] if BSNR_min is None else BSNR_min
    bmax = defaults["bmax"] if BSNR_max is None else BSNR_max
    lmax = defaults["lmax"] if lambdaMax is None else lambdaMax
    x = np.asarray(x, dtype=np.float64)
    taps, _ = psf_family(kind, 7, p)
    Ax = BlurOperator(taps, ctx=ctx).A(x)
    dimX = x.size
    nrm = float(np.linalg.norm(Ax - np.mean(Ax)))
    sigma = nrm / math.sqrt(dimX * 10 ** (BSNR / 10))
    smin = nrm / math.sqrt(dimX * 10 ** (bmin / 10))
    smax = nrm / math.sqrt(dimX * 10 ** (bmax / 10))
    y = Ax + sigma * np.asarray(noise, dtype=np.float64)
    lf = lambda s2: evMax ** 2 / s2
    Lf = defaults["lf"](lf(smin ** 2), lf(smax ** 2))
    lam = min(5 / Lf, lmax)
    gamma = defaults["gmul"] * gammaFrac * (1 / (Lf + 1 / lam))
    return dict(kind=kind, y=y, x=x, sigma=sigma, sigma_min=smin ** 2, sigma_max=smax ** 2,
                sigma_init=(smin ** 2 + smax ** 2) / 2, Lf=Lf, **{"lambda": lam}, gamma=gamma, p_true=p,
                th_init=th_init, dimX=dimX)


def _moments_opts(posterior):
    """posterior = True | dict(first=0, thin=1, pooled=False) -> sbtv_moments_opts (first = 0: the entry point's default,
    burnIn for SAPG, 1 for MYULA)."""
    p = {} if posterior is True else dict(posterior)
    unknown = set(p) - {"first", "thin", "pooled"}
    if unknown:
        raise ValueError(f"posterior: unknown keys {sorted(unknown)}")
    mo = L.sbtv_moments_opts()
    mo.first = int(p.get("first", 0))
    mo.thin = int(p.get("thin", 1))
    mo.pooled = 1 if p.get("pooled", False) else 0
    return mo


def _moment_buffers(like, n):
    """mean / var outputs for n images in the memory kind of `like` (an L.Images), and the host count array."""
    if like.torch:
        import torch
        mk = lambda: L.Images(torch.empty((n, like.N, like.M), dtype=torch.float64, device=like.t.device).permute(0, 2, 1),
                              _fresh=True)
    else:
        mk = lambda: L.Images(np.zeros((n, like.M, like.N)))
    return mk(), mk(), np.zeros(n, dtype=np.int64)


def combine_moments(parts):
    """(count, mean, var) of the union of sample sets given as (count, mean, var) triples (var = M2 / (count-1), the
    unbiased form of sbtv_SAPG_algorithm_moments; 0 for count 1): Chan's pairwise combination in the order given,
    n = na + nb, d = mean_b - mean_a, mean = mean_a + d nb / n, M2 = M2_a + M2_b + d^2 na nb / n.  For chains spread over
    processes (sbtv.dist.split_chains) or calls; pure NumPy.  The moments' pooled = 1 forms its set the same way."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_moments: no parts")
    n0, mean, var = parts[0]
    na = float(n0)
    mu = np.array(mean, dtype=np.float64)
    m2 = np.array(var, dtype=np.float64) * (na - 1.0) if na > 1 else np.zeros_like(mu)
    for nb, mb, vb in parts[1:]:
        nb = float(nb)
        mb = np.asarray(mb, dtype=np.float64)
        sb = np.asarray(vb, dtype=np.float64) * (nb - 1.0) if nb > 1 else np.zeros_like(mb)
        nt = na + nb
        d = mb - mu
        mu = mu + d * (nb / nt)
        m2 = (m2 + sb) + d * d * (na * nb / nt)
        na = nt
    var_out = m2 / (na - 1.0) if na > 1 else np.zeros_like(mu)
    return int(na), mu, var_out


def _sapg(kind, y, op, c, noise=None, x0=None, share_gradients=False, reduce_fn=None, ctx=None, reduce_dev_fn=None,
          host_loop=False, posterior=None, skrock=None, mask=None):
    """mask: the chains sample the masked-observation posterior (sbtv_SAPG_masked): non-negative weights with the shape and the
    memory kind of y; no share_gradients, reduce_fn, host_loop, skrock or sbtv.Group then.
    skrock = (stages, dt, eta): the chain moves with SK-ROCK steps (sbtv_SAPG_skrock) instead of MYULA steps; no
    share_gradients, reduce_fn, host_loop or sbtv.Group then.
    reduce_fn(user, buf, n): host all-reduce of the shared-gradient sums (selects the host-side parameter loop);
    reduce_dev_fn(user, dev_ptr, n, stream): in-stream all-reduce on the device buffer (`dist.make_device_allreduce_fn`),
    the loop stays device-resident; host_loop=True forces the host-side loop (SBTV_SAPG_HOST_LOOP).
    posterior = True | dict(first, thin, pooled): also the posterior mean / variance of the samples
    (sbtv_SAPG_algorithm_moments), returned as results['posteriormean'], ['posteriorvar'], ['posterior_count']."""
    if reduce_fn is not None and reduce_dev_fn is not None:
        raise ValueError("give reduce_fn or reduce_dev_fn, not both")
    ctx = ctx or L.default_context()
    yi = L.Images(y)
    B, M, N = yi.B, yi.M, yi.N
    o = L.sbtv_sapg_opts()
    o.kind = _KIND[kind]
    o.psf_size = int(_get(op, "psf_size", 7))
    o.samples = int(_get(op, "samples"))
    o.warmup = int(_get(op, "warmup", 100))                       # default 100 (SAPG_algorithm_Guassian.m:20)
    o.burnIn = int(_get(op, "burnIn"))
    o.chambolleit = int(_get(op, "chambolleit", 25))              # run_Gaussian_demo.m:188
    o.share_gradients = 1 if share_gradients else 0
    o.lambda_ = float(c.get("lam", 1.0)) * float(_get(op, "lambda"))     # lamb = c.lam*op.lambda (:30)
    # sbtv_SAPG_skrock ignores gamma: op need not carry it then
    o.gamma = float(c.get("gam", 1.0)) * float(_get(op, "gamma", 0.0) if skrock is not None else _get(op, "gamma"))
    o.th_init = float(_get(op, "th_init"))
    o.min_th = float(_get(op, "min_th"))
    o.max_th = float(_get(op, "max_th"))
    names = {"gaussian": ("w1", "w2"), "moffat": ("alpha", "beta"), "laplace": ("b",)}[kind]
    for q, nm in enumerate(names):
        o.p_init[q] = float(_get(op, nm + "_init"))
        o.p_min[q] = float(_get(op, "min_" + nm))
        o.p_max[q] = float(_get(op, "max_" + nm))
        o.p_true[q] = float(np.ravel(_get(op, nm))[0])
        o.fix_p[q] = int(bool(_get(op, "fix_" + nm, 0)))
        o.c_p[q] = float(c[nm])
    if len(names) == 1:
        o.fix_p[1] = 1
    o.phi = float(_get(op, "phi", 0.0))
    o.fix_sigma = int(bool(_get(op, "fix_sigma", 0)))
    o.sigma2_true = float(_get(op, "sigma")) ** 2                 # sigma = op.sigma^2 (:49)
    o.sigma2_init = float(_get(op, "sigma_init"))
    o.sigma2_min = float(_get(op, "sigma_min"))
    o.sigma2_max = float(_get(op, "sigma_max"))
    o.d_scale = float(_get(op, "d_scale"))
    o.d_exp = float(_get(op, "d_exp"))
    o.c_theta = float(c["theta"])
    o.c_sigma = float(c["sigma"])
    o.seed = int(_get(op, "seed", 1))
    o.chain_offset = int(_get(op, "chain_offset", 0))              # first chain of this process (dist.split_chains)
    o.iter_offset = int(_get(op, "iter_offset", 0))                # resume: iteration ii of this call steps with delta(ii + offset)
    S, W = o.samples, max(o.warmup, 1)
    nch = B
    thetas = np.zeros((nch, S)); sigmas = np.zeros((nch, S)); ps = np.zeros((nch, 2, S))
    logpi = np.zeros((nch, S)); logpi_wu = np.zeros((nch, W)); gx = np.zeros((nch, S)); grads = np.zeros((nch, 4, S))
    eb = np.zeros((nch, 4))
    xl = L.empty_like_images(yi)
    x0i = L.Images(x0) if x0 is not None else None
    if _get(op, "X0") is not None and x0 is None:
        x0i = L.Images(_get(op, "X0"))
    nz_ptr, nz_keep = None, None
    if noise is not None:
        if L._is_torch(noise):
            nz_keep = noise
            nz_ptr = C.c_void_p(noise.data_ptr())
        else:
            a = np.asarray(noise, dtype=np.float64)           # (steps, B, M, N) or (steps, M, N)
            if a.ndim == 3:
                a = a[:, None]
            nz_keep = L.column_major_images(a.reshape((-1,) + a.shape[2:])).reshape(a.shape[:2] + (a.shape[3], a.shape[2]))   # column-major images
            nz_ptr = L.vptr(nz_keep)
    cb = L.ALLREDUCE_FN(reduce_fn) if reduce_fn is not None else L.ALLREDUCE_FN()
    xflags = L.SAPG_HOST_LOOP if host_loop else 0
    if reduce_dev_fn is not None:
        cb_dev = L.ALLREDUCE_DEV_FN(reduce_dev_fn)            # kept alive until the call returns
        cb = C.cast(cb_dev, L.ALLREDUCE_FN)
        xflags |= L.REDUCE_DEVICE
    vp = L.vptr
    yptr = yi.ptr
    if share_gradients:
        # all chains sample ONE image: y is a single image, the batch size is the chain count
        nch = int(_get(op, "chains", 1))
        thetas = np.zeros((nch, S)); sigmas = np.zeros((nch, S)); ps = np.zeros((nch, 2, S))
        logpi = np.zeros((nch, S)); logpi_wu = np.zeros((nch, W)); gx = np.zeros((nch, S)); grads = np.zeros((nch, 4, S))
        eb = np.zeros((nch, 4))
        if yi.torch:
            import torch
            xl = L.Images(torch.empty((nch, N, M), dtype=torch.float64, device=yi.t.device).permute(0, 2, 1))
        else:
            xl = L.Images(np.zeros((nch, M, N)))
    if posterior is not None and posterior is not False and getattr(ctx, "is_group", False):
        raise NotImplementedError("posterior moments over a sbtv.Group: run the shards' chains per call and "
                                  "sbtv.combine_moments their results")
    if mask is not None:
        if (share_gradients or reduce_fn is not None or reduce_dev_fn is not None or host_loop or skrock is not None
                or getattr(ctx, "is_group", False)):
            raise ValueError("SAPG_masked offers no share_gradients, reduce_fn, host_loop, skrock or sbtv.Group")
        mi = L.Images(mask)
        if mi.torch != yi.torch or (mi.B, mi.M, mi.N) != (B, M, N):
            raise ValueError("mask must have the shape and the memory kind of y")
        mo = pm = pv = pc = None
        if posterior is not None and posterior is not False:
            mo = _moments_opts(posterior)
            pm, pv, pc = _moment_buffers(yi, 1 if mo.pooled else nch)
        ctx.check(ctx.lib.sbtv_SAPG_masked(ctx.h, yptr, mi.ptr, M, N, nch, C.byref(o), x0i.ptr if x0i else None, nz_ptr,
                                           vp(thetas), vp(ps), vp(sigmas), vp(logpi), vp(logpi_wu), vp(gx), vp(grads),
                                           vp(eb), xl.ptr, None if mo is None else C.byref(mo),
                                           None if mo is None else pm.ptr, None if mo is None else pv.ptr,
                                           None if mo is None else vp(pc), yi.flags), yi.flags)
    elif skrock is not None:
        if share_gradients or reduce_fn is not None or reduce_dev_fn is not None or host_loop or getattr(ctx, "is_group", False):
            raise ValueError("SAPG_skrock offers no share_gradients, reduce_fn, host_loop or sbtv.Group")
        sk = L.sbtv_sapg_skrock_step(int(skrock[0]), float(skrock[1]), float(skrock[2]))
        mo = pm = pv = pc = None
        if posterior is not None and posterior is not False:
            mo = _moments_opts(posterior)
            pm, pv, pc = _moment_buffers(yi, 1 if mo.pooled else nch)
        ctx.check(ctx.lib.sbtv_SAPG_skrock(ctx.h, yptr, M, N, nch, C.byref(o), C.byref(sk), x0i.ptr if x0i else None, nz_ptr,
                                           vp(thetas), vp(ps), vp(sigmas), vp(logpi), vp(logpi_wu), vp(gx), vp(grads),
                                           vp(eb), xl.ptr, None if mo is None else C.byref(mo),
                                           None if mo is None else pm.ptr, None if mo is None else pv.ptr,
                                           None if mo is None else vp(pc), yi.flags), yi.flags)
    elif getattr(ctx, "is_group", False):
        # several GPUs behind this process (sbtv.Group): images / chains dealt to the devices in contiguous blocks; with
        # share_gradients the six gradient sums are exchanged in-process, in-stream (no reduce_fn needed or accepted)
        if yi.flags != L.SBTV_HOST_PTRS or (noise is not None and L._is_torch(noise)):
            raise ValueError("a sbtv.Group takes host (NumPy) images")
        if reduce_fn is not None or reduce_dev_fn is not None or host_loop:
            raise ValueError("a sbtv.Group exchanges the shared gradients itself: no reduce_fn / host_loop")
        ctx.check(ctx.lib.sbtv_SAPG_algorithm_sharded(ctx.h, yptr, M, N, nch, C.byref(o), x0i.ptr if x0i else None, nz_ptr,
                                                      vp(thetas), vp(ps), vp(sigmas), vp(logpi), vp(logpi_wu), vp(gx),
                                                      vp(grads), vp(eb), xl.ptr))
    elif posterior is not None and posterior is not False:
        mo = _moments_opts(posterior)
        pm, pv, pc = _moment_buffers(yi, 1 if mo.pooled else nch)
        ctx.check(ctx.lib.sbtv_SAPG_algorithm_moments(ctx.h, yptr, M, N, nch, C.byref(o), x0i.ptr if x0i else None, nz_ptr,
                                                      vp(thetas), vp(ps), vp(sigmas), vp(logpi), vp(logpi_wu), vp(gx),
                                                      vp(grads), vp(eb), xl.ptr, cb, None, C.byref(mo), pm.ptr, pv.ptr,
                                                      vp(pc), yi.flags | xflags), yi.flags)
    else:
        ctx.check(ctx.lib.sbtv_SAPG_algorithm(ctx.h, yptr, M, N, nch, C.byref(o), x0i.ptr if x0i else None, nz_ptr,
                                              vp(thetas), vp(ps), vp(sigmas), vp(logpi), vp(logpi_wu), vp(gx), vp(grads),
                                              vp(eb), xl.ptr, cb, None, yi.flags | xflags), yi.flags)
    results = []
    for b in range(nch):
        r = dict(theta_EB=eb[b, 0], sigma_EB=eb[b, 3], last_samp=S, thetas=thetas[b], sigmas=sigmas[b],
                 logPiTraceX=logpi[b], logPiTrace_WU=logpi_wu[b, :o.warmup] if o.warmup > 0 else np.array([]),
                 gXTrace=gx[b], grad_theta=grads[b, 0], grad_sigma=grads[b, 3], last_theta=thetas[b, -1],
                 last_sigma=sigmas[b, -1], c_theta=o.c_theta, c_sigma=o.c_sigma, options=op)
        for q, nm in enumerate(names):
            r[nm + "_EB"] = eb[b, 1 + q]
            r[nm + "s"] = ps[b, q]
            r["last_" + nm] = ps[b, q, -1]
            r["grad_" + nm] = grads[b, 1 + q]
        results.append(r)
    xs = L.images_result(xl, False)
    for b in range(nch):
        results[b]["Xlast_sample"] = xs[b]
        # running means from burnIn and their relative change, as the reference logs them while iterating
        # (SAPG_algorithm_Guassian.m:217-244: mean_* over burnIn..ii for ii > burnIn; tol_*(ii) = relative change
        # of that mean, NaN while the window is empty)
        for key, tolkey in [("thetas", "tol_thetas"), ("sigmas", "tol_sigma")] + [(nm + "s", "tol_" + nm + "s") for nm in names]:
            m, t = _running_mean_and_tol(results[b][key], o.burnIn)
            results[b]["mean_" + key] = m
            results[b][tolkey] = t
        results[b]["err_psf"] = _err_psf(kind, o.psf_size, ps[b, :len(names)], [o.p_true[q] for q in range(len(names))],
                                         o.phi)
    if posterior is not None and posterior is not False:
        # results.posteriormean / results.posteriorvar of SAPG_algorithm_Guassian.m:292-293 (pooled: the same set in every
        # chain's results)
        ms, vs = L.images_result(pm, False), L.images_result(pv, False)
        for b in range(nch):
            q = 0 if mo.pooled else b
            results[b]["posteriormean"] = ms[q]
            results[b]["posteriorvar"] = vs[q]
            results[b]["posterior_count"] = int(pc[q])
    return results


def _running_mean_and_tol(trace, burnIn):
    """mean_x(ii - burnIn) = mean(x(burnIn:ii)) for ii > burnIn and tol_x(ii) = |mean(x(burnIn:ii)) - mean(x(burnIn:ii-1))|
    / mean(x(burnIn:ii-1)) for ii >= 2 (1-based; NaN where a window is empty, like MATLAB's mean of an empty range)."""
    x = np.asarray(trace, dtype=np.float64)
    n, b0 = x.size, int(burnIn) - 1                      # 0-based index of burnIn
    run = np.full(n, np.nan)                             # run[i] = mean(x[b0 .. i]) for i >= b0
    if b0 < n:
        run[b0:] = np.cumsum(x[b0:]) / np.arange(1, n - b0 + 1)
    tol = np.zeros(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        tol[1:] = np.abs(run[1:] - run[:-1]) / run[:-1]
    return run[b0 + 1:].copy(), tol


def _err_psf(kind, taille, ps, p_true, phi):
    """results.err_psf: l2 = norm(.)^2 with the MATRIX 2-norm (utils/l2.m, quirk Q9) between the PSF at the traced
    parameters and the true PSF, evaluated on the host from the parameter traces.  Family quirks as in the
    reference: Gaussian pairs w1s(ii) with w2s(ii-1) (SAPG_algorithm_Guassian.m:203, Q8); Moffat stores its first
    value under another name, so err_psf(1) = 0 (SAPG_algorithm_moffat.m:156); Laplace is plain (:136,191)."""
    lib = L.load_library()
    tr = np.zeros((2, ps.shape[1]))
    tr[:ps.shape[0]] = ps                                           # [first-parameter trace | second-parameter trace]
    pt = np.zeros(2)
    pt[:len(p_true)] = p_true
    out = np.zeros(ps.shape[1])
    rc = lib.sbtv_err_psf(_KIND[kind], int(taille), L.vptr(tr), int(ps.shape[1]),
                          L.vptr(pt), float(phi), L.vptr(out))
    if rc != 0:
        raise L.SbtvError(rc, lib.sbtv_last_error(None).decode())
    return out


def _unpack(kind, res, batched):
    names = {"gaussian": ("w1", "w2"), "moffat": ("alpha", "beta"), "laplace": ("b",)}[kind]
    if not batched:
        r = res[0]
        return (r["theta_EB"],) + tuple(r[n + "_EB"] for n in names) + (r["sigma_EB"], r)
    return ([r["theta_EB"] for r in res],) + tuple([r[n + "_EB"] for r in res] for n in names) + \
        ([r["sigma_EB"] for r in res], res)


def SAPG_algorithm_Guassian(y, op, c, **kw):
    """[theta_EB, w1_EB, w2_EB, sigma_EB, results] = SAPG_algorithm_Guassian(y, op, c)
    (SAPG/SAPG_algorithm_Guassian.m:7-308).  c: dict(theta, w1, w2, sigma, lam, gam) (run_Gaussian_demo.m:34-39)."""
    res = _sapg("gaussian", y, op, c, **kw)
    return _unpack("gaussian", res, len(res) > 1)


def SAPG_algorithm_moffat(y, op, c=None, **kw):
    """[theta_EB, alpha_EB, beta_EB, sigma2_EB, results] = SAPG_algorithm_moffat(y, op)
    (SAPG/SAPG_algorithm_moffat.m:7-297; step scales hard-coded at :135-138)."""
    c = c or dict(theta=0.1, alpha=10.0, beta=1e4, sigma=1e4, lam=1.0, gam=1.0)
    res = _sapg("moffat", y, op, c, **kw)
    return _unpack("moffat", res, len(res) > 1)


def SAPG_algorithm_laplace(y, op, c=None, **kw):
    """[theta_EB, b_EB, sigma2_EB, results] = SAPG_algorithm_laplace(y, op)
    (SAPG/SAPG_algorithm_laplace.m:7-268; step scales hard-coded at :139-141)."""
    c = c or dict(theta=0.01, b=100.0, sigma=1e4, lam=1.0, gam=1.0)
    res = _sapg("laplace", y, op, c, **kw)
    return _unpack("laplace", res, len(res) > 1)


def SAPG_skrock(kind, y, op, c, stages, dt, eta=0.05, noise=None, x0=None, posterior=None, ctx=None):
    """SAPG_algorithm_Guassian / _moffat / _laplace (kind = "gaussian" | "moffat" | "laplace") with SK-ROCK as the Markov
    kernel (sbtv_SAPG_skrock, include/sbtv.h): every iteration moves the chain by one SK-ROCK step of `stages` drift
    evaluations and step `dt` at the current theta, PSF parameters and sigma2.  op.gamma is not used.  dt: at most
    sbtv.skrock_max_step(stages, eta, min(op.sigma_min, op.sigma_max), lambda), the bound at the smallest sigma2 the chain
    may reach.  noise: optional (max(warmup-1, 0) + samples-1, [B,] M, N) normals instead of the device Philox stream.
    Returns what the mirror of that family returns: (theta_EB, <PSF parameters>_EB, sigma_EB, results)."""
    res = _sapg(kind, y, op, c, noise=noise, x0=x0, posterior=posterior, ctx=ctx, skrock=(stages, dt, eta))
    return _unpack(kind, res, len(res) > 1)


def SAPG_masked(kind, y, mask, op, c, noise=None, x0=None, posterior=None, ctx=None):
    """SAPG_algorithm_Guassian / _moffat / _laplace (kind = "gaussian" | "moffat" | "laplace") on the masked-observation
    likelihood of sbtv.SALSA_masked (sbtv_SAPG_masked, include/sbtv.h): R = sum(mask .* (B_p x - y).^2) and the number of
    observed pixels take the place of ||B_p x - y||^2 and dimX in the likelihood, its gradient and the sigma2 step.  mask:
    non-negative weights like y (0 = not observed; embed a valid convolution with sbtv.embed_observation / valid_mask).
    op.gamma as the demos compute it holds for max(mask) <= 1.  noise: optional (max(warmup-1, 0) + samples-1, [B,] M, N)
    normals instead of the device Philox stream.
    Returns what the mirror of that family returns: (theta_EB, <PSF parameters>_EB, sigma_EB, results)."""
    res = _sapg(kind, y, op, c, noise=noise, x0=x0, posterior=posterior, ctx=ctx, mask=mask)
    return _unpack(kind, res, len(res) > 1)


def myula_masked(op, mask, im=None, noise=None, posterior=None, ctx=None):
    """sbtv.myula / sbtv.myula_moments on the masked-observation likelihood (sbtv_myula_masked): gradF(x) =
    AT(mask .* (A x - y)) / sigma2.  mask: non-negative weights with the shape and the memory kind of op.y.  The chain starts
    from op.y as given.  posterior = None: the last sample, as sbtv.myula returns it; True | dict(first=1, thin=1): what
    sbtv.myula_moments returns, dict(x, mean, var, count).  Other arguments as for sbtv.myula."""
    ctx = ctx or L.default_context()
    A = _get(op, "A")
    if not isinstance(A, BlurOperator):
        raise TypeError("op.A must be the sbtv.BlurOperator the closures op.gradF / op.proxG are built from")
    yi = L.Images(_get(op, "y"))
    B, M, N = yi.B, yi.M, yi.N
    mi = L.Images(mask)
    if mi.torch != yi.torch or (mi.B, mi.M, mi.N) != (B, M, N):
        raise ValueError("mask must have the shape and the memory kind of op.y")
    s2 = _get(op, "sigma2")
    if s2 is None:
        s2 = np.asarray(_get(op, "sigma"), dtype=np.float64) ** 2
    keep = [L.dvec(_get(op, "theta_op"), B), L.dvec(s2, B)]
    taps = A._cm(B)
    xo = L.empty_like_images(yi)
    nz_ptr, nz_keep = None, None
    if noise is not None:
        if L._is_torch(noise):
            nz_keep, nz_ptr = noise, C.c_void_p(noise.data_ptr())
        else:
            a = np.asarray(noise, dtype=np.float64)
            if a.ndim == 3:
                a = a[:, None]
            nz_keep = L.column_major_images(a.reshape((-1,) + a.shape[2:])).reshape(a.shape[:2] + (a.shape[3], a.shape[2]))
            nz_ptr = L.vptr(nz_keep)
    mo = pm = pv = pc = None
    if posterior is not None and posterior is not False:
        mo = _moments_opts(posterior)
        pm, pv, pc = _moment_buffers(yi, 1 if mo.pooled else B)
    ctx.check(ctx.lib.sbtv_myula_masked(ctx.h, yi.ptr, mi.ptr, M, N, B, L.vptr(taps), A.taille,
                                        float(_get(op, "lambda")), float(_get(op, "gamma")), keep[0][1], keep[1][1],
                                        int(_get(op, "samples")), int(_get(op, "chambolleit", 25)),
                                        int(_get(op, "seed", 1)), int(_get(op, "chain_offset", 0)), nz_ptr, xo.ptr,
                                        None if mo is None else C.byref(mo), None if mo is None else pm.ptr,
                                        None if mo is None else pv.ptr, None if mo is None else L.vptr(pc), yi.flags),
              yi.flags)
    y = _get(op, "y")
    sq = (y.dim() == 2) if yi.torch else yi.squeeze
    if mo is None:
        return L.images_result(xo, sq)
    one = sq or mo.pooled
    return dict(x=L.images_result(xo, sq), mean=L.images_result(pm, one), var=L.images_result(pv, one),
                count=int(pc[0]) if one else pc.copy())


def myula(op, im=None, noise=None, ctx=None):
    """xMAP = myula(op, im)  (SALSA/myula.m:1-22): the plain MYULA chain at fixed theta / PSF, last sample returned.

    op: dict / object with y, lambda, gamma, theta_op, samples as in the reference, plus what the closures
    op.proxG / op.gradF of SALSA/run_deblur_tv.m:126,131 are built from: `A` (the sbtv.BlurOperator at tau_op),
    `sigma2` (or `sigma`), `chambolleit` (25).  `im` is only used for its shape in the reference and is ignored.
    noise: optional (samples-2, [B,] M, N) array instead of the device Philox stream (op.seed, op.chain_offset)."""
    ctx = ctx or L.default_context()
    A = _get(op, "A")
    if not isinstance(A, BlurOperator):
        raise TypeError("op.A must be the sbtv.BlurOperator the closures op.gradF / op.proxG are built from")
    yi = L.Images(_get(op, "y"))
    B, M, N = yi.B, yi.M, yi.N
    s2 = _get(op, "sigma2")
    if s2 is None:
        s2 = np.asarray(_get(op, "sigma"), dtype=np.float64) ** 2
    keep = [L.dvec(_get(op, "theta_op"), B), L.dvec(s2, B)]
    taps = A._cm(B)
    xo = L.empty_like_images(yi)
    nz_ptr, nz_keep = None, None
    if noise is not None:
        if L._is_torch(noise):
            nz_keep, nz_ptr = noise, C.c_void_p(noise.data_ptr())
        else:
            a = np.asarray(noise, dtype=np.float64)
            if a.ndim == 3:
                a = a[:, None]
            nz_keep = L.column_major_images(a.reshape((-1,) + a.shape[2:])).reshape(a.shape[:2] + (a.shape[3], a.shape[2]))
            nz_ptr = L.vptr(nz_keep)
    ctx.check(ctx.lib.sbtv_myula(ctx.h, yi.ptr, M, N, B, L.vptr(taps), A.taille,
                                 float(_get(op, "lambda")), float(_get(op, "gamma")), keep[0][1], keep[1][1],
                                 int(_get(op, "samples")), int(_get(op, "chambolleit", 25)), int(_get(op, "seed", 1)),
                                 int(_get(op, "chain_offset", 0)), nz_ptr, xo.ptr, yi.flags), yi.flags)
    y = _get(op, "y")
    return L.images_result(xo, (y.dim() == 2) if yi.torch else yi.squeeze)


def myula_moments(op, im=None, noise=None, posterior=True, ctx=None):
    """myula (SALSA/myula.m) with the posterior mean / variance of its samples (sbtv_myula_moments):
    dict(x = last sample, mean, var, count).  posterior = True | dict(first=1, thin=1, pooled=False); iteration 1 is y,
    iteration ii the sample of step ii (ii = 2..samples-1).  Other arguments as for sbtv.myula."""
    ctx = ctx or L.default_context()
    A = _get(op, "A")
    if not isinstance(A, BlurOperator):
        raise TypeError("op.A must be the sbtv.BlurOperator the closures op.gradF / op.proxG are built from")
    yi = L.Images(_get(op, "y"))
    B, M, N = yi.B, yi.M, yi.N
    s2 = _get(op, "sigma2")
    if s2 is None:
        s2 = np.asarray(_get(op, "sigma"), dtype=np.float64) ** 2
    keep = [L.dvec(_get(op, "theta_op"), B), L.dvec(s2, B)]
    taps = A._cm(B)
    xo = L.empty_like_images(yi)
    nz_ptr, nz_keep = None, None
    if noise is not None:
        if L._is_torch(noise):
            nz_keep, nz_ptr = noise, C.c_void_p(noise.data_ptr())
        else:
            a = np.asarray(noise, dtype=np.float64)
            if a.ndim == 3:
                a = a[:, None]
            nz_keep = L.column_major_images(a.reshape((-1,) + a.shape[2:])).reshape(a.shape[:2] + (a.shape[3], a.shape[2]))
            nz_ptr = L.vptr(nz_keep)
    mo = _moments_opts(posterior)
    pm, pv, pc = _moment_buffers(yi, 1 if mo.pooled else B)
    ctx.check(ctx.lib.sbtv_myula_moments(ctx.h, yi.ptr, M, N, B, L.vptr(taps), A.taille,
                                         float(_get(op, "lambda")), float(_get(op, "gamma")), keep[0][1], keep[1][1],
                                         int(_get(op, "samples")), int(_get(op, "chambolleit", 25)),
                                         int(_get(op, "seed", 1)), int(_get(op, "chain_offset", 0)), nz_ptr, xo.ptr,
                                         C.byref(mo), pm.ptr, pv.ptr, L.vptr(pc), yi.flags), yi.flags)
    y = _get(op, "y")
    sq = (y.dim() == 2) if yi.torch else yi.squeeze
    one = sq and not mo.pooled
    return dict(x=L.images_result(xo, sq), mean=L.images_result(pm, one or mo.pooled),
                var=L.images_result(pv, one or mo.pooled), count=int(pc[0]) if (one or mo.pooled) else pc.copy())


def skrock(op, im=None, noise=None, x0=None, posterior=None, ctx=None):
    """SK-ROCK chain on the TV posterior at fixed theta / PSF / sigma2 (sbtv_skrock): the target and closures of sbtv.myula
    with the explicit stabilised step of Pereyra, Vargas Mieles and Zygalakis (SIAM J. Imaging Sci. 2020), stated in
    include/sbtv.h.  Sample 1 is the start state (x0, default y), op.samples - 1 steps follow (no off-by-one).

    op: the fields of sbtv.myula (y, lambda, theta_op, samples, A, sigma2 or sigma, chambolleit (25), seed (1),
    chain_offset (0)) without gamma, plus `stages` (s >= 2 drift evaluations per step), `delta` (the step; None: 0.8 of
    skrock_max_step at ||A|| = 1 and the call's smallest sigma2) and `eta` (0.05).  `im` is ignored, as in myula.
    noise: optional (samples-1, [B,] M, N) normals instead of the device Philox stream; x0: optional start images.
    posterior: None | True | dict(first=1, thin=1, pooled=False): moments of the samples 1..samples.
    Returns dict(x = last sample, gx, logpi: (samples,) or (B, samples)[, mean, var, count])."""
    from .wavelet import skrock_max_step
    ctx = ctx or L.default_context()
    A = _get(op, "A")
    if not isinstance(A, BlurOperator):
        raise TypeError("op.A must be the sbtv.BlurOperator the closures op.gradF / op.proxG are built from")
    yi = L.Images(_get(op, "y"))
    B, M, N = yi.B, yi.M, yi.N
    s2 = _get(op, "sigma2")
    if s2 is None:
        s2 = np.asarray(_get(op, "sigma"), dtype=np.float64) ** 2
    th, s2v = L.dvec(_get(op, "theta_op"), B), L.dvec(s2, B)
    taps = A._cm(B)
    o = L.sbtv_skrock_opts()
    o.samples, o.stages, o.chambolleit = int(_get(op, "samples")), int(_get(op, "stages")), int(_get(op, "chambolleit", 25))
    o.lambda_, o.eta = float(_get(op, "lambda")), float(_get(op, "eta", 0.05))
    delta = _get(op, "delta")
    o.delta = float(delta) if delta is not None else 0.8 * skrock_max_step(o.stages, o.eta, float(np.min(s2v[0])), o.lambda_)
    o.seed, o.chain_offset = int(_get(op, "seed", 1)), int(_get(op, "chain_offset", 0))
    S = max(o.samples, 1)
    xo = L.empty_like_images(yi)
    x0i = None if x0 is None else L.Images(x0)
    if x0i is not None and (x0i.torch != yi.torch or (x0i.B, x0i.M, x0i.N) != (B, M, N)):
        raise ValueError("x0 must have the shape and the memory kind of op.y")
    nz_ptr, nz_keep = None, None
    if noise is not None:
        if L._is_torch(noise):
            nz_keep, nz_ptr = noise, C.c_void_p(noise.data_ptr())
        else:
            a = np.asarray(noise, dtype=np.float64)
            if a.ndim == 3:
                a = a[:, None]
            nz_keep = L.column_major_images(a.reshape((-1,) + a.shape[2:])).reshape(a.shape[:2] + (a.shape[3], a.shape[2]))
            nz_ptr = L.vptr(nz_keep)
    gx, logpi = np.zeros((B, S)), np.zeros((B, S))
    mo, pm, pv, pc = None, None, None, None
    if posterior is not None and posterior is not False:
        mo = _moments_opts(posterior)
        pm, pv, pc = _moment_buffers(yi, 1 if mo.pooled else B)
    ctx.check(ctx.lib.sbtv_skrock(ctx.h, yi.ptr, M, N, B, L.vptr(taps), A.taille, C.byref(o), th[1], s2v[1],
                                  None if x0i is None else x0i.ptr, nz_ptr, L.vptr(gx), L.vptr(logpi), xo.ptr,
                                  None if mo is None else C.byref(mo), None if mo is None else pm.ptr,
                                  None if mo is None else pv.ptr, None if mo is None else L.vptr(pc), yi.flags), yi.flags)
    y = _get(op, "y")
    sq = (y.dim() == 2) if yi.torch else yi.squeeze
    res = dict(x=L.images_result(xo, sq), gx=gx[0] if sq else gx, logpi=logpi[0] if sq else logpi)
    if mo is not None:
        one = sq or mo.pooled
        res.update(mean=L.images_result(pm, one), var=L.images_result(pv, one), count=int(pc[0]) if one else pc.copy())
    return res
