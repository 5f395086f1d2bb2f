// PSF formulas of the reference shared by the host builder (sbtv_psf_taps, ctx.hip) and the device-resident SAPG
// parameter updates (sapg.hip, sapg_chain_update.inc, wavelet_sapg_sb.hip).  Element q = jj*taille + ii (column-major, 0-based) of the un-normalised PSF f and of
// its derivatives e0, e1 with respect to the (up to) two parameters:
//   gaussian  utils/Gaussian_psf.m:2-19, Sum_gauss_psf.m:1-28, diff_fftgaus_w1.m / diff_fftgaus_w2.m   p = (w1, w2, phi)
//   moffat    utils/psf_moffat.m:2-20, sum_mof_psf.m:1-40, diff_moffat_alpha.m, diff_moffat_beta.m     p = (alpha, beta)
//   laplace   utils/psf_laplace.m:1-13, sum_lap_psf.m:1-28, diff_laplace_b.m:1-19                      p = (b)
// The expressions keep the reference's operation order; no FMA contraction on either side.
__host__ __device__ inline void psf_taps_point(int kind, int t, const double *p, int q, double *f, double *e0, double *e1) {
#pragma clang fp contract(off)
    const double PI = 3.14159265358979323846;
    const double center = (t + 1) / 2.0;
    const int jj = q / t, ii = q - jj * t;
    const double xi = (-t + center) + ii, xj = (-t + center) + jj;      // -taille+center : taille-center
    *e0 = 0.0;
    *e1 = 0.0;
    if (kind == 0) {
        const double w1 = p[0], w2 = p[1], phi = p[2];
        const double v = xi, u = xj;                                    // ndgrid: v rows, u columns
        const double U = u * cos(phi) - v * sin(phi);
        const double V = u * sin(phi) + v * cos(phi);
        const double c = w1 * w1 * (U * U) + w2 * w2 * (V * V);
        const double ex = exp(-c / 2);
        *f = ((w1 * w2) / (2 * PI)) * ex;
        *e0 = (w2 / (2 * PI)) * (1 - w1 * w1 * (U * U)) * ex;
        *e1 = (w1 / (2 * PI)) * (1 - w2 * w2 * (V * V)) * ex;
    } else if (kind == 1) {
        const double a = p[0], b = p[1], b2 = b + 2;
        const double xy = xi * xi + xj * xj;
        *f = a * a * pow((xy * (a * a)) / b + 1, -b2 / 2) / (2 * PI);
        *e0 = (2 - (((b + 2) * xy * (a * a)) / (2 * (b + xy * (a * a))))) * pow(1 + xy * (a * a) / b, -(b + 2) / 2) *
              (a / (2 * PI));
        const double cons1 = (a * a) / (4 * PI);
        *e1 = (-log(xy * (a * a) / b + 1) + (b2 * xy * (a * a)) / (b * (b + xy * (a * a)))) *
              pow(xy * (a * a) / b + 1, -b2 / 2) * cons1;
    } else {
        const double b = p[0];
        const double sa = fabs(xi) + fabs(xj);
        *f = ((b * b) / 4) * exp(-b * sa);
        *e0 = ((2 * b - (b * b) * sa) / 4) * exp(-b * sa);
    }
}

// The normalised taps and both derivative taps of the PSF parameters pv, built by one whole workgroup of at least t2 = t * t
// lanes (every lane of it calls this): one lane per tap, then lanes 0, 1, 2 total f, e0 and e1 in MATLAB's column-major order
// (sum(k(:))), then tap q of spectrum set `sset` goes to par[s * t2 * nspec + sset * t2 + q], s = 0 taps, 1, 2 derivatives.
// sf / se0 / se1 [>= t2] and ssum[3] are the caller's shared memory; it puts a barrier before it uses them again.
__device__ __forceinline__ void psf_taps_block(int kind, int t, const double *pv, double *par, int sset, int nspec, double *sf,
                                               double *se0, double *se1, double *ssum) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, t2 = t * t;
    if (tid < t2) psf_taps_point(kind, t, pv, tid, &sf[tid], &se0[tid], &se1[tid]);
    __syncthreads();
    if (tid < 3) {
        const double *v = tid == 0 ? sf : (tid == 1 ? se0 : se1);
        double a = 0.0;
        for (int q = 0; q < t2; ++q) a += v[q];
        ssum[tid] = a;
    }
    __syncthreads();
    if (tid < t2) {
        const double a = ssum[0], f = sf[tid], e0 = se0[tid], e1 = se1[tid];
        const size_t set = (size_t)t2 * nspec, o = (size_t)sset * t2 + tid;
        par[o] = f / a;
        par[set + o] = (e0 * a - f * ssum[1]) / (a * a);
        par[2 * set + o] = (e1 * a - f * ssum[2]) / (a * a);
    }
}
