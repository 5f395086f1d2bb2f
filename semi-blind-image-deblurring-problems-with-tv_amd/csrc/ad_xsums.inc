// ---- the pixel pass of the drivers whose unknown is the image but whose prior lives on the frame --------------------
// wavelet_deconv.hip (analysis_one) and csalsa_wavelet.hip include this file inside their anonymous namespace, after
// admm_run.inc; each unit carries its own copy of the kernel.

// the image-domain sums of an outer iteration: partials [3][nb]: (x-true)^2, (x-xprev)^2, x^2 (tru / xprev null: not summed)
__global__ __launch_bounds__(AB) void ad_xsums_kernel(const double *__restrict__ x, const double *__restrict__ tru,
                                                       const double *__restrict__ xprev, double *__restrict__ partials,
                                                       size_t P) {
    double acc[3] = {0.0, 0.0, 0.0};
    AD_LOOP(q, P) {
        const double2 xv = AD_LD(x, q);
        if (tru) {
            const double2 tv = AD_LD(tru, q);
            const double m0 = xv.x - tv.x, m1 = xv.y - tv.y;
            acc[0] += m0 * m0 + m1 * m1;
        }
        if (xprev) {
            const double2 xo = AD_LD(xprev, q);
            const double m0 = xv.x - xo.x, m1 = xv.y - xo.y;
            acc[1] += m0 * m0 + m1 * m1;
        }
        acc[2] += xv.x * xv.x + xv.y * xv.y;
    }
    ad_store_partials<3>(acc, partials);
}
