// ---- what the single-image ADMM-style drivers share -------------------------------------------------------------
// admm.hip (the TV front-ends), wavelet_deconv.hip (the wavelet-l1 solvers) and coral_wavelet.hip (CoRAL with both
// regularisers) include this file inside their anonymous namespace in namespace sbtv, after <chrono> and sbtv_internal.h, as
// the SAPG drivers include sapg_step.inc; nothing here is relocatable device code, so each unit carries its own copy of
// ad_sub_kernel.  The element-wise kernels of these units are written with AD_LOOP / AD_LD / AD_ST and end in
// ad_store_partials; their drivers open the operator layer with admm_common and carry their pipelined loop in an AdmmRun.
constexpr int AB = 256;

__device__ __forceinline__ double ad_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// block-reduce NQ running sums and store them as partials[q * gridDim.x + blockIdx.x]
template <int NQ>
__device__ __forceinline__ void ad_store_partials(double (&acc)[NQ], double *__restrict__ partials) {
    __shared__ double red[NQ * 4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
        const double a = ad_wave_sum(acc[c]);
        if (lane == 0) red[c * 4 + w] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < NQ; ++c)
            partials[(size_t)c * gridDim.x + blockIdx.x] = (red[c * 4] + red[c * 4 + 1]) + (red[c * 4 + 2] + red[c * 4 + 3]);
    }
}

#define AD_LOOP(q, P) for (size_t q = (size_t)blockIdx.x * AB + threadIdx.x; q < (P) / 2; q += (size_t)gridDim.x * AB)
#define AD_LD(p, q) (*reinterpret_cast<const double2 *>((p) + 2 * (q)))
#define AD_ST(p, q, v) (*reinterpret_cast<double2 *>((p) + 2 * (q)) = (v))

// g = x - b
__global__ __launch_bounds__(AB) void ad_sub_kernel(const double *__restrict__ x, const double *__restrict__ b,
                                                     double *__restrict__ g, size_t P) {
    AD_LOOP(q, P) {
        const double2 xv = AD_LD(x, q), bv = AD_LD(b, q);
        AD_ST(g, q, make_double2(xv.x - bv.x, xv.y - bv.y));
    }
}

inline int ad_blocks(size_t P) {
    size_t nb = (P / 2 + AB - 1) / AB;
    if (nb > 1024) nb = 1024;
    return nb < 1 ? 1 : (int)nb;
}

// everything one single-image solve shares: the operator layer "admm" with the spectra of the PSF and (yd given) of y
int admm_common(sbtv_ctx *ctx, int M, int N, const double *taps, int taille, const double *yd, BlurOp *c) {
    SBTV_TRY(check_even_pixels(ctx, M, N));
    SBTV_TRY(op_open(ctx, "admm", M, N, 1, "Y", c));
    double *taps_d = nullptr;
    SBTV_TRY(ws_get_t(ctx, "admm.taps", (size_t)taille * taille, &taps_d));
    SBTV_HIP(ctx, hipMemcpyAsync(taps_d, taps, sizeof(double) * taille * taille, hipMemcpyHostToDevice, ctx->stream));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SBTV_TRY(psf_spectrum(ctx, c->fp, taps_d, taille, c->Hs));
    if (yd) SBTV_TRY(op_spectrum(ctx, c->fp, yd, nullptr, c->S, c->Ys));
    return 0;
}

// the four doubles of "admm.par" (each driver says what they are), on the device before anything is enqueued that reads them
int upload_par(sbtv_ctx *ctx, double *par, const double (&h)[4]) {
    SBTV_HIP(ctx, hipMemcpyAsync(par, h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
    SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// What a solve carries through its pipelined loop.  Per-iteration scalars travel through two pinned slots; an event per
// slot tells the host (which runs one iteration ahead) when the slot of an iteration holds its scalars.  Beside them: the
// clock of `times`, the operator counts, the Chambolle iterations of sbtv_last_timing.
struct AdmmRun {
    static constexpr int NSUM = 94;                // doubles per slot, then the iteration counts of up to two exact proxes
    sbtv_ctx *ctx = nullptr;
    double *hs[2] = {nullptr, nullptr};            // the two slots (pinned): the sums ...
    int *khs[2] = {nullptr, nullptr};              // ... and the counts, at [0] and [2]
    hipEvent_t ev[2] = {nullptr, nullptr};
    long long opt_iters[2] = {0, 0};
    std::chrono::steady_clock::time_point t0;
    int numA = 0, numAt = 0;
    long long prox_iters = 0;
    int *numA_out = nullptr, *numAt_out = nullptr, *n_outer_out = nullptr;

    ~AdmmRun() {
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int open(sbtv_ctx *c, int *numA_o, int *numAt_o, int *n_outer_o) {
        ctx = c;
        numA_out = numA_o;
        numAt_out = numAt_o;
        n_outer_out = n_outer_o;
        PinnedLayout lay;
        PinnedField<double> fs[2];
        PinnedField<int> fk[2];
        for (int s = 0; s < 2; ++s) {
            fs[s] = lay.add<double>(NSUM);
            fk[s] = lay.add<int>(4);
        }
        void *pz = nullptr;
        SBTV_TRY(pinned_get(ctx, lay.bytes(), &pz));
        for (int s = 0; s < 2; ++s) {
            hs[s] = fs[s].at(pz);
            khs[s] = fk[s].at(pz);
        }
        for (auto &e : ev) SBTV_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return 0;
    }
    // the loop begins: sbtv_last_timing and `times` count from here
    int start() {
        t0 = std::chrono::steady_clock::now();
        SBTV_HIP(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
        return 0;
    }
    // before the loop: the first n doubles of `sums`, read back through slot 0
    int fetch(const double *sums, int n, const double **h) {
        SBTV_HIP(ctx, hipMemcpyAsync(hs[0], sums, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *h = hs[0];
        return 0;
    }
    double seconds() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    // end of enqueue(outer): the first n doubles of `sums` into the iteration's slot.  Its Chambolle iterations are `iters` if
    // its proxes were optimistic; exact ones hand the control blocks that count theirs (k0, k1: device)
    int publish(int outer, const double *sums, int n, long long iters, const ProxCtrl *k0 = nullptr,
                const ProxCtrl *k1 = nullptr) {
        double *hsl = hs[outer & 1];
        int *kh = khs[outer & 1];
        kh[0] = kh[2] = 0;
        opt_iters[outer & 1] = iters;
        SBTV_HIP(ctx, hipGetLastError());
        SBTV_HIP(ctx, hipMemcpyAsync(hsl, sums, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
        if (k0) SBTV_HIP(ctx, hipMemcpyAsync(kh, &k0->k, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        if (k1) SBTV_HIP(ctx, hipMemcpyAsync(kh + 2, &k1->k, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        SBTV_HIP(ctx, hipEventRecord(ev[outer & 1], ctx->stream));
        return 0;
    }
    // head of process(outer): waits for the iteration's slot, books its Chambolle iterations
    int wait(int outer, const double **hsl) {
        *hsl = hs[outer & 1];
        SBTV_HIP(ctx, hipEventSynchronize(ev[outer & 1]));
        const int *kh = khs[outer & 1];
        prox_iters += opt_iters[outer & 1] + kh[0] + kh[2];
        return 0;
    }
    // after the loop: its device time (sbtv_last_timing), the result x (null: the caller fetches its own), the counters
    int finish(size_t P, int last, const double *x, double *x_out) {
        SBTV_HIP(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
        SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        SBTV_TRY(loop_timing(ctx, 0.0, prox_iters, 1, P));
        if (x) {
            SBTV_HIP(ctx, hipMemcpyAsync(x_out, x, sizeof(double) * P, hipMemcpyDeviceToDevice, ctx->stream));
            SBTV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        if (numA_out) *numA_out = numA;
        if (numAt_out) *numAt_out = numAt;
        if (n_outer_out) *n_outer_out = last;
        return 0;
    }
};
