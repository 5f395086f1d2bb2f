// ---- the per-chain end of a SAPG iteration: the totals, the parameter step of sapg_step.inc, the new PSF taps ----------
// Shared by the SAPG drivers whose chains each own their parameters, sapg_skrock.hip (SK-ROCK kernel) and sapg_masked.hip
// (masked observation): both include this file inside their unnamed namespace, after sapg_step.inc; nothing here is
// relocatable device code.  The update kernel of sbtv_SAPG_algorithm (sapg_update_kernel, sapg.hip) is another one: one
// workgroup for all chains, shared gradients, the stop rule of the deferred prox.
#pragma clang fp contract(off)
constexpr int SAPG_CHAIN_WG = WAV_EWB;   // lanes per workgroup (wav_block_sum sums four waves)

struct SapgChainDev : SapgConst {
    const double *acc;         // [batch][3][nrb]: partial sums of ||AX-y||^2 (masked: R) and of the two <dA/dp_q X, residual>
    const double *tvp;         // [batch][ntv]: partial sums of TVnorm(X)
    int nrb, ntv;
    const double *nobs;        // [batch]: observed pixels of every chain, in place of dimX in G_sigma; null: G[3] of sapg_gradients
    ProxCtrl *pctrl;           // [batch]: control blocks already armed for the next prox, re-armed at lambda theta(ii); null: none
    double *scal;              // [4*batch]: the totals, in the layout sapg_gradients reads (sapg_collect_kernel's)
    SapgChain *chain;          // [batch]
    double *par;               // [taps | d0 | d1] of every chain, lam[batch], sigma2[batch]
    const double *delta;       // [samples + 1]: delta(ii), tabulated by the host (pow)
    double *traces;            // device traces, layout of sapg_traces (one pointer: the kernel's arguments live in scalar registers)
};
// what the update kernel does with the sums: logpi_wu(ii) of warm-up iteration ii; logpi(1) of the state the SAPG loop starts
// from; the parameter step of SAPG iteration ii
enum { SAPG_CHAIN_WARMUP = 0, SAPG_CHAIN_START = 1, SAPG_CHAIN_MAIN = 2 };

// Collector and parameter update of the MYULA loop (sapg_collect_kernel + sapg_update_kernel) as one launch, one workgroup
// per chain, so that chain b of a batch is computed exactly as alone.  The four sums are totalled in the order of
// skrock_trace_kernel; one lane then runs sapg_gradients / sapg_step; with a free PSF parameter the workgroup builds the
// taps and both derivative taps of p(ii) (psf_taps_block: one path for every mask size, 15 x 15 is 225 lanes).
__global__ __launch_bounds__(SAPG_CHAIN_WG) void sapg_chain_update_kernel(SapgChainDev u, int phase, int ii) {
    __shared__ double red[4], sf[SAPG_CHAIN_WG], se0[SAPG_CHAIN_WG], se1[SAPG_CHAIN_WG], ssum[3], pnew[2];
    const int b = blockIdx.x, tid = threadIdx.x, t2 = u.taille * u.taille;
    double tot[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double *p = q < 3 ? u.acc + ((size_t)b * 3 + q) * u.nrb : u.tvp + (size_t)b * u.ntv;
        const int n = q < 3 ? u.nrb : u.ntv;
        double s = 0.0;
        for (int i = tid; i < n; i += SAPG_CHAIN_WG) s += p[i];
        tot[q] = wav_block_sum(s, red);
    }
    if (tid == 0) {
        for (int q = 0; q < 3; ++q) u.scal[(size_t)b * 3 + q] = tot[q];
        u.scal[3 * (size_t)u.batch + b] = tot[3];
        SapgChain c = u.chain[b];
        const SapgTraces tr = sapg_traces(u.traces, u);
        if (phase == SAPG_CHAIN_WARMUP) {
            tr.wu[(size_t)b * u.warmup + (ii - 1)] = sapg_logpi(u, c, u.scal, b);                  // :85
        } else if (phase == SAPG_CHAIN_START) {
            tr.logpi[(size_t)b * u.samples] = sapg_logpi(u, c, u.scal, b);                         // :131
        } else {
            double G[4];
            sapg_gradients(u, tr, c, u.scal, b, ii, G, u.nobs);
            sapg_step(u, tr, c, b, ii, u.delta[ii], G);
            u.chain[b] = c;
            double *lam_d = u.par + (size_t)3 * t2 * u.batch, *sig_d = lam_d + u.batch;
            const double lam = u.lamb * c.theta; // proxG(x, theta): 'lambda', op.lambda*theta  (run_Gaussian_demo.m:191)
            lam_d[b] = lam;
            sig_d[b] = c.sig2;
            if (u.pctrl) u.pctrl[b].lambda = lam;        // the first prox of the next step runs at theta(ii) too
            pnew[0] = c.p0;
            pnew[1] = c.p1;
        }
    }
    if (phase != SAPG_CHAIN_MAIN || !u.params_move) return;
    __syncthreads();
    const double pv[3] = {pnew[0], u.kind == 2 ? 0.0 : pnew[1], u.kind == 0 ? u.phi : 0.0};
    psf_taps_block(u.kind, u.taille, pv, u.par, b, u.batch, sf, se0, se1, ssum);
}
