// ---- the warm-started TV prox of the ADMM-style drivers ---------------------------------------------------------
// admm.hip (C-SALSA, CoRAL, the masked SALSA) and coral_wavelet.hip (CoRAL with the TV + wavelet-l1 regulariser) include
// this file inside their anonymous namespace, after admm_run.inc; host code only.
// The warm-started TV prox of an outer iteration: a plan (of one image, or of CoRAL's two), its threshold(s) `lam` on the
// device and K iterations per prox.
struct AdmmProx {
    ProxPlan pp;
    const double *lam = nullptr;
    int K = 0;
    double tol = 0.0, tau = 0.0;
    long long nlaunch = 0;       // optimistic launches so far: the kernels read dual buffer cur ^ (nlaunch & 1)

    int plan(sbtv_ctx *ctx, int M, int N, int batch, const char *tag, int iters, const sbtv_salsa_opts *opts) {
        K = iters;
        tol = opts->chambolle_tol;
        tau = opts->chambolle_tau;
        return prox_plan(ctx, M, N, batch, &pp, tag);
    }
    // arms the control block(s); fresh: before the first prox, on zero duals
    int arm(sbtv_ctx *ctx, bool fresh) { return prox_reset(ctx, pp, lam, 1.0, K, tol, tau, !fresh, nullptr); }
    // f = prox(g).  Exact: re-armed, the kernels apply the stop rule.  Optimistic: all K iterations back to back on the
    // control block as `arm` left it, and the step sums of the K iterations (of image b at stepsums + b FSTRIDE) for the
    // host's rule: reduced at once, or with a job list together with the other sums of the iteration
    int run(sbtv_ctx *ctx, const double *g, double *f, bool optimistic, double *stepsums, RedJobs *jb) {
        if (!optimistic) {
            SBTV_TRY(arm(ctx, false));
            return prox_iterate(ctx, pp, g, K, f);
        }
        SBTV_TRY(prox_iterate(ctx, pp, g, K, f, false, 1, (int)(nlaunch & 1), nullptr));
        nlaunch += prox_launches(pp, K);
        const int nvec = (pp.batch - 1) * FSTRIDE + K;
        if (!jb) return reduce_partials(ctx, pp.partials, nvec, pp.fnblk, stepsums);
        jb->add(pp.partials, nvec, pp.fnblk, stepsums);
        return 0;
    }
    // the host's rule on the step sums of an optimistic prox (SOLVE_RESTART_EXACT: it fired early)
    int check(sbtv_ctx *ctx, const double *stepsums) { return spec_stop_rule(ctx, pp, stepsums, K, tol); }
};
