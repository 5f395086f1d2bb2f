// ---- the right-hand side of the masked drivers' start 2 ----------------------------------------------------------------
// admm.hip (masked_one) and masked_wavelet.hip (masked_analysis_one) include this file inside their anonymous namespace, after
// admm_run.inc; each unit carries its own copy of the kernel.

// w = m .* y: the right-hand side of the start x = B'(m .* y) ('INITIALIZATION' 2)
__global__ __launch_bounds__(AB) void masked_my_kernel(const double *__restrict__ m, const double *__restrict__ y,
                                                        double *__restrict__ w, size_t P) {
    AD_LOOP(q, P) {
        const double2 mv = AD_LD(m, q), yv = AD_LD(y, q);
        AD_ST(w, q, make_double2(mv.x * yv.x, mv.y * yv.y));
    }
}
