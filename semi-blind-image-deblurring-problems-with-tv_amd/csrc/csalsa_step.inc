// ---- what the two C-SALSA drivers share of the constraint split -----------------------------------------------------
// admm.hip (C-SALSA with the TV prox, csalsa_one) and csalsa_wavelet.hip (C-SALSA with the wavelet analysis prior) include
// this file inside their anonymous namespace, after admm_run.inc; nothing here is relocatable device code, so each unit
// carries its own copy of the three kernels.

// w = mu2 * (y + v + bv)                                                   (CSALSA_v2.m:467)
__global__ __launch_bounds__(AB) void csalsa_w_kernel(const double *__restrict__ y, const double *__restrict__ v,
                                                       const double *__restrict__ bv, const double *__restrict__ par,
                                                       double *__restrict__ w, size_t P) {
    const double mu2 = par[1];
    AD_LOOP(q, P) {
        const double2 a = AD_LD(y, q), b = AD_LD(v, q), c = AD_LD(bv, q);
        AD_ST(w, q, make_double2(mu2 * ((a.x + b.x) + c.x), mu2 * ((a.y + b.y) + c.y)));
    }
}

// partials[nb] = sum (Ax - y - bv)^2                                        (:483-484)
__global__ __launch_bounds__(AB) void csalsa_ve_kernel(const double *__restrict__ Ax, const double *__restrict__ y,
                                                        const double *__restrict__ bv, double *__restrict__ partials,
                                                        size_t P) {
    double acc[1] = {0.0};
    AD_LOOP(q, P) {
        const double2 a = AD_LD(Ax, q), b = AD_LD(y, q), c = AD_LD(bv, q);
        const double e0 = (a.x - b.x) - c.x, e1 = (a.y - b.y) - c.y;
        acc[0] += e0 * e0 + e1 * e1;
    }
    ad_store_partials<1>(acc, partials);
}

// ---- C-SALSA with the constraint split kept as a spectrum (default; see csalsa_one) ------------------------------
// After the row pass: the three spectral sums of the iteration -> the projection factor s = min(1, eps / ||ve||), the
// coefficients of the next row pass and the two traces that depend on Ax.  st: [0] mu2, [1] c_e = mu2 (2s-1),
// [2] c_keep = 1-s, [3] sum |E|^2 of the previous iteration (unscaled), [4] 1 - s of the previous iteration.
//   out[0] = ||Ax-y||^2, out[1] = ||Ax-y-v||^2 = ||(1-s) E' - (1-s_prev) E||^2 from |E'|^2, |E|^2 and |E'-E|^2:
//   (a-c)(a A1 - c A1p) + a c A2 (no difference of large numbers once the iteration settles: a -> c, E' -> E)
__global__ __launch_bounds__(256) void csalsa_scal_kernel(const double *__restrict__ accp, int nrb, double *__restrict__ st,
                                                          double eps, double pv, double *__restrict__ out) {
    // the three sums of the row pass, partials [3][nrb], in the order of reduce_partials_kernel
    __shared__ double red[4 * 3], tot[3];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double s = 0.0;
        for (int i = threadIdx.x; i < nrb; i += 256) s += accp[(size_t)c * nrb + i];
        s = ad_wave_sum(s);
        if (lane == 0) red[c * 4 + w] = s;
    }
    __syncthreads();
    if (threadIdx.x < 3) tot[threadIdx.x] = (red[threadIdx.x * 4] + red[threadIdx.x * 4 + 1]) + (red[threadIdx.x * 4 + 2] + red[threadIdx.x * 4 + 3]);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double A0 = tot[0], A1 = tot[1], A2 = tot[2];
    const double n_ve = sqrt(A1 * pv);
    const double sfac = (n_ve <= eps) ? 1.0 : eps / n_ve;
    const double a = 1.0 - sfac, c = st[4], A1p = st[3];
    const double d1 = ((a - c) * (a * A1 - c * A1p) + a * c * A2) * pv;
    out[0] = A0 * pv;
    out[1] = d1 > 0.0 ? d1 : 0.0;
    st[1] = st[0] * (2.0 * sfac - 1.0);
    st[2] = a;
    st[3] = A1;
    st[4] = a;
}

// C-SALSA: the constraint split (v, bv) as ONE spectrum and a scalar (default) or as images (SBTV_CSALSA_SPECTRAL=0)
inline bool csalsa_spectral_wanted() {
    static const bool on = [] {
        const char *e = getenv("SBTV_CSALSA_SPECTRAL");
        return !(e && e[0] == '0');
    }();
    return on;
}
