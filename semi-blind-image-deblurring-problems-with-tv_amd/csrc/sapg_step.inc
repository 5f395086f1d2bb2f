// ---- the SAPG parameter step (SAPG_algorithm_Guassian.m:165-248 and twins) ---------------------------------------
// Shared by the drivers of the semi-blind TV estimation: sapg.hip (MYULA kernel), sapg_skrock.hip (SK-ROCK kernel), sapg_masked.hip
// (masked observation) and their common host side, sampler_common.hip, include this file inside namespace sbtv, as tv.hip
// includes tv_fused.inc; nothing here is relocatable device code.  The per-chain update kernel of the two newer drivers is
// sapg_chain_update.inc.
// State of one chain, the constants of a run and the traces; the arithmetic below is written once and runs inside the
// update kernel of the device-resident loop, so that no iteration has to wait for the host, and on the host in the
// host-side loop.  No FMA contraction on either side: theta / p / sigma traces are bit-identical for the same scalars.
struct SapgChain {
    double theta, p0, p1, sig2, sum_th, sum_p0, sum_p1, sum_s;
};
struct SapgConst {
    int kind, taille, npar, nspec, batch, shared, samples, warmup, burnIn, params_move, fix_p0, fix_p1, fix_sigma;
    double dimX, parseval, lamb, c_theta, c_p0, c_p1, c_sigma, min_th, max_th, p_min0, p_max0, p_min1, p_max1, p_true0,
        p_true1, s_lo, s_hi, sigma2_init, phi, step_base;
};
// traces of a run in one block, layouts of sbtv.h (warmup above: the stride of wu, >= 1)
struct SapgTraces {
    double *theta, *p, *sigma, *logpi, *gx, *grads, *wu;
};
static inline size_t sapg_traces_len(const SapgConst &k) { return (size_t)k.batch * k.samples * 10 + (size_t)k.batch * k.warmup; }
__host__ __device__ static inline SapgTraces sapg_traces(double *base, const SapgConst &k) {
    const size_t bs = (size_t)k.batch * k.samples;
    return SapgTraces{base, base + 4 * bs, base + bs, base + 2 * bs, base + 3 * bs, base + 6 * bs, base + 10 * bs};
}

// logPi = -||y-AX||^2/(2 sigma2) - theta*TVnorm(X) of chain b from the collector's scalars  (run_Gaussian_demo.m:171,195)
__host__ __device__ __forceinline__ double sapg_logpi(const SapgConst &k, const SapgChain &c, const double *scal, int b) {
#pragma clang fp contract(off)
    const double resid2 = scal[(size_t)b * 3] * k.parseval;
    return -resid2 / (2 * c.sig2) - c.theta * scal[3 * (size_t)k.batch + b];
}
// G[4] = G_theta, G_p0, G_p1, G_sigma of chain b in SAPG iteration ii from the collector's scalars; books logPi and g(X).
// nobs non-null (masked observation): nobs[b] observed pixels take the place of dimX in G_sigma
__host__ __device__ __forceinline__ void sapg_gradients(const SapgConst &k, const SapgTraces &tr, const SapgChain &c,
                                                        const double *scal, int b, int ii, double *G,
                                                        const double *nobs = nullptr) {
#pragma clang fp contract(off)
    const int i0 = ii - 1;
    const double resid2 = scal[(size_t)b * 3] * k.parseval;
    const double tv = scal[3 * (size_t)k.batch + b], lp = sapg_logpi(k, c, scal, b);
    G[0] = k.dimX / c.theta - tv;                                                             // :165
    G[1] = (scal[(size_t)b * 3 + 1] * k.parseval) / c.sig2;                                   // :170
    G[2] = (scal[(size_t)b * 3 + 2] * k.parseval) / c.sig2;                                   // :179
    G[3] = resid2 / (2 * c.sig2 * c.sig2) - (nobs ? nobs[b] : k.dimX) / (2 * c.sig2);         // :188
    tr.logpi[(size_t)b * k.samples + i0] = lp;                                                // :207
    tr.gx[(size_t)b * k.samples + (i0 - 1)] = tv;                                             // :208
}
// the projected updates of chain b with step delta(ii) and gradients G[4], its traces and its burn-in sums
__host__ __device__ __forceinline__ void sapg_step(const SapgConst &k, const SapgTraces &tr, SapgChain &c, int b, int ii,
                                                   double delta, const double *G) {
#pragma clang fp contract(off)
    const int i0 = ii - 1;
    const double th_new = fmin(fmax(c.theta + k.c_theta * delta * G[0], k.min_th), k.max_th);        // :166-167
    double q0 = k.fix_p0 ? k.p_true0 : c.p0 - k.c_p0 * delta * G[1];                                 // :171-176
    q0 = fmin(fmax(q0, k.p_min0), k.p_max0);
    double q1 = c.p1;
    if (k.npar > 1) {
        q1 = k.fix_p1 ? k.p_true1 : c.p1 - k.c_p1 * delta * G[2];                                    // :180-185
        q1 = fmin(fmax(q1, k.p_min1), k.p_max1);
    }
    double s_new = k.fix_sigma ? k.sigma2_init : c.sig2 + k.c_sigma * delta * G[3];                  // :189-194
    s_new = fmin(fmax(s_new, k.s_lo), k.s_hi);
    for (int q = 0; q < 4; ++q) tr.grads[((size_t)b * 4 + q) * k.samples + i0] = G[q];
    tr.theta[(size_t)b * k.samples + i0] = th_new;
    tr.sigma[(size_t)b * k.samples + i0] = s_new;
    tr.p[((size_t)b * 2 + 0) * k.samples + i0] = q0;
    tr.p[((size_t)b * 2 + 1) * k.samples + i0] = q1;
    c.theta = th_new;
    c.p0 = q0;
    c.p1 = q1;
    c.sig2 = s_new;
    if (ii >= k.burnIn) {
        c.sum_th += th_new;
        c.sum_s += s_new;
        c.sum_p0 += q0;
        c.sum_p1 += q1;
    }
}
// delta(ii) of SAPG_algorithm_Guassian.m:55
static double sapg_delta(const sbtv_sapg_opts *op, double dimX, int ii) {
    return op->d_scale * (pow((double)ii + op->iter_offset, -op->d_exp) / dimX);
}
