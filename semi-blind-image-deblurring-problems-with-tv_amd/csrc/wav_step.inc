// ---- coefficient passes shared by the wavelet-l1 solvers -----------------------------------------------------------
// wavelet_deconv.hip (the three wavelet-l1 solvers), coral_wavelet.hip (CoRAL with the TV + wavelet-l1 regulariser) and
// csalsa_wavelet.hip (C-SALSA with the analysis prior) include this file inside their anonymous namespace, after
// admm_run.inc; nothing here is relocatable device code, so each unit carries its own copy of the kernels.

// l1 norm of the start xw and its distance to the true coefficients: partials [2][nb]
__global__ __launch_bounds__(AB) void wav_init_kernel(const double *__restrict__ xw, const double *__restrict__ tru,
                                                       double *__restrict__ partials, size_t C) {
    double acc[2] = {0.0, 0.0};
    AD_LOOP(q, C) {
        const double2 v = AD_LD(xw, q);
        acc[0] += fabs(v.x) + fabs(v.y);
        if (tru) {
            const double2 t = AD_LD(tru, q);
            const double m0 = v.x - t.x, m1 = v.y - t.y;
            acc[1] += m0 * m0 + m1 * m1;
        }
    }
    ad_store_partials<2>(acc, partials);
}

// The one coefficient pass of an outer iteration k, after the analysis w = W'x_k, on the state (s, bu) = (u_k + bu_{k-1}, bu_{k-1}):
//   u = s - bu (exactly zero where the threshold cut it: there s == bu bit for bit) ; bu' = bu + (u - w)    (SALSA_v2.m:440)
//   u' = soft(w - bu', T) ; s' = u' + bu'                                                                  (:431 of k + 1)
//   partials [4][nb]: |u|, u^2, (w-u)^2, w^2
// The start is the same pass with s = w_0 and bu = 0.
__global__ __launch_bounds__(AB) void wav_astep_kernel(const double *__restrict__ s, const double *__restrict__ bu,
                                                        const double *__restrict__ w, double *__restrict__ bun,
                                                        double *__restrict__ sn, double T, double *__restrict__ partials,
                                                        size_t C) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    AD_LOOP(q, C) {
        const double2 sv = AD_LD(s, q), bv = AD_LD(bu, q), wv = AD_LD(w, q);
        const double u0 = sv.x - bv.x, u1 = sv.y - bv.y;
        const double d0 = wv.x - u0, d1 = wv.y - u1;
        const double b0 = bv.x + (u0 - wv.x), b1 = bv.y + (u1 - wv.y);
        AD_ST(bun, q, make_double2(b0, b1));
        AD_ST(sn, q, make_double2(wav_soft(wv.x - b0, T) + b0, wav_soft(wv.y - b1, T) + b1));
        acc[0] += fabs(u0) + fabs(u1);
        acc[1] += u0 * u0 + u1 * u1;
        acc[2] += d0 * d0 + d1 * d1;
        acc[3] += wv.x * wv.x + wv.y * wv.y;
    }
    ad_store_partials<4>(acc, partials);
}

// The coefficient pass of C-SALSA's outer iteration k, after the analysis w = W'x_k, on the multiplier bu (updated in place):
//   u = soft(w - bu, T) ; bu' = bu - (w - u) ; s' = u + bu', the next synthesis input       (CSALSA_v2.m:478, 492, 467 of k + 1)
//   partials [2][nb]: |w| (the objective ||W'x_k||_1), (w-u)^2                                (:498 with Phi = ||W'.||_1, :497)
// The threshold follows the analysis of the same iteration, so u is formed here and never recovered from s - bu: four arrays,
// 32 B per coefficient.  The arithmetic is the reference's, term for term.
__global__ __launch_bounds__(AB) void wav_cstep_kernel(const double *__restrict__ w, double *__restrict__ bu,
                                                        double *__restrict__ sn, double T, double *__restrict__ partials,
                                                        size_t C) {
    double acc[2] = {0.0, 0.0};
    AD_LOOP(q, C) {
        const double2 wv = AD_LD(w, q), bv = AD_LD(bu, q);
        const double u0 = wav_soft(wv.x - bv.x, T), u1 = wav_soft(wv.y - bv.y, T);
        const double d0 = wv.x - u0, d1 = wv.y - u1;
        const double b0 = bv.x - d0, b1 = bv.y - d1;
        AD_ST(bu, q, make_double2(b0, b1));
        AD_ST(sn, q, make_double2(u0 + b0, u1 + b1));
        acc[0] += fabs(wv.x) + fabs(wv.y);
        acc[1] += d0 * d0 + d1 * d1;
    }
    ad_store_partials<2>(acc, partials);
}
