// The blur operator as the solver drivers see it: one plan, the spectra of the PSF and of the observation, and the
// handful of transforms through them.  Each function hides one launch triple (forward column pass, row pass with its
// spectral operation, unpack or inverse column pass) together with its RowsArgs and scale factors.  Beside it: the
// argument checks the entry points share.  The per-iteration bodies of the SALSA and FISTA loops, which fuse their
// bookkeeping into the column passes, stay with their drivers.
#include "sbtv_internal.h"

namespace sbtv {

int op_open(sbtv_ctx *ctx, const char *prefix, int M, int N, int batch, const char *y_name, BlurOp *op) {
    SBTV_TRY(fft_plan(ctx, M, N, batch, &op->fp));
    op->batch = batch;
    op->P = (size_t)M * N;
    const std::string p = std::string(prefix) + ".";
    SBTV_TRY(ws_get_t(ctx, (p + "S").c_str(), (size_t)batch * op->fp.s_img, &op->S));
    SBTV_TRY(ws_get_t(ctx, (p + "H").c_str(), (size_t)batch * op->fp.u_img, &op->Hs));
    op->Ys = nullptr;
    if (y_name) SBTV_TRY(ws_get_t(ctx, (p + y_name).c_str(), (size_t)batch * op->fp.u_img, &op->Ys));
    op->inv_scale = 1.0 / ((double)op->fp.n1 * N);
    op->parseval = 1.0 / ((double)M * N);
    return 0;
}

int op_spectrum(sbtv_ctx *ctx, const FftPlan &fp, const double *in, const double *add, double2 *S, double2 *U) {
    RowsArgs a{};
    a.dir_fwd = 1;
    a.op = OP_NONE;
    SBTV_TRY(fft_cols_fwd(ctx, fp, in, add, S));
    SBTV_TRY(fft_rows(ctx, fp, S, S, a));
    return spec_unpack(ctx, fp, S, U);
}

// in (+ add) through the forward column pass, the row pass `a` on H (forward and inverse transform around its operation)
// and the inverse column pass into out
static int op_through(sbtv_ctx *ctx, const BlurOp &c, const double *in, const double *add, RowsArgs a, double *out) {
    a.dir_fwd = a.dir_inv = 1;
    a.H = c.Hs;
    SBTV_TRY(fft_cols_fwd(ctx, c.fp, in, add, c.S));
    SBTV_TRY(fft_rows(ctx, c.fp, c.S, c.S, a));
    return fft_cols_inv(ctx, c.fp, c.S, out, c.inv_scale);
}

int op_apply(sbtv_ctx *ctx, const BlurOp &c, int op, const double *in, double *out, const double *mu) {
    RowsArgs a{};
    a.op = op;
    a.mu = mu;
    return op_through(ctx, c, in, nullptr, a, out);
}

int op_solve(sbtv_ctx *ctx, const BlurOp &c, const double *in, const double *add, const double2 *Y, const double *mu,
             double *acc, double *out) {
    RowsArgs a{};
    a.op = OP_SALSA;
    a.Y = Y;
    a.mu = mu;
    a.acc = acc;
    return op_through(ctx, c, in, add, a, out);
}

int op_gradf(sbtv_ctx *ctx, const BlurOp &c, const double *x, double *acc, double *grad) {
    RowsArgs a{};
    a.op = OP_GRADF;
    a.Y = c.Ys;
    a.acc = acc;
    return op_through(ctx, c, x, nullptr, a, grad);
}

int op_resid(sbtv_ctx *ctx, const BlurOp &c, const double *x, double *acc, const int *frozen, double *tvp) {
    RowsArgs a{};
    a.dir_fwd = 1;
    a.op = OP_RESID;
    a.H = c.Hs;
    a.Y = c.Ys;
    a.acc = acc;
    a.frozen = frozen;
    SBTV_TRY(fft_cols_fwd_f(ctx, c.fp, x, nullptr, c.S, frozen, tvp));
    return fft_rows(ctx, c.fp, c.S, nullptr, a);
}

int op_init_x(sbtv_ctx *ctx, const BlurOp &c, int initialization, const double *yd, const double *xi, double *x) {
    const size_t bytes = sizeof(double) * c.P * c.batch;
    if (initialization == 0) {
        SBTV_HIP(ctx, hipMemsetAsync(x, 0, bytes, ctx->stream));                    // AT(zeros) == 0
    } else if (initialization == 2) {
        SBTV_TRY(op_apply(ctx, c, OP_MUL_HC, yd, x));                               // x = ATy
    } else {
        SBTV_HIP(ctx, hipMemcpyAsync(x, xi, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return 0;
}

int check_psf_fits(sbtv_ctx *ctx, int taille, int M, int N) {
    if (taille < 1 || taille > 15 || taille > M || taille > N) return fail(ctx, SBTV_ERR_PSF, "Mask does not fit inside array");
    return 0;
}

int check_even_pixels(sbtv_ctx *ctx, int M, int N) {
    if (((size_t)M * N) & 1)
        return fail(ctx, SBTV_ERR_SIZE, "this entry point needs an even number of pixels (its element-wise passes move two per lane)");
    return 0;
}

int check_common(sbtv_ctx *ctx, const char *who, const double *y, const double *taps, const sbtv_salsa_opts *opts,
                 const double *x_init, int M, int N, int batch, int taille, const char *x_init_name, bool tv,
                 bool maxiter_positive) {
    if (!y || !opts || batch < 1) return fail(ctx, SBTV_ERR_BADARG, std::string(who) + ": missing required argument");
    if (!taps) return fail(ctx, SBTV_ERR_MISSING_AT, "The function handle for transpose of A is missing");
    if (opts->stopcriterion < 1 || opts->stopcriterion > 3) return fail(ctx, SBTV_ERR_STOPCRITERION, "Unknown stopping criterion");
    if (opts->initialization != 0 && opts->initialization != 2 && opts->initialization != 33333)
        return fail(ctx, SBTV_ERR_INIT, "Unknown 'Initialization' option");
    if (opts->initialization == 33333 && !x_init)
        return fail(ctx, SBTV_ERR_INIT, std::string("Initialization = array but ") + x_init_name + " is NULL");
    if (tv && opts->TViters <= 0) return fail(ctx, SBTV_ERR_MAXITER, std::string(who) + ": TViters must be positive");
    if (maxiter_positive && opts->maxiter < 1) return fail(ctx, SBTV_ERR_MAXITER, std::string(who) + ": maxiter must be positive");
    return check_psf_fits(ctx, taille, M, N);
}

}  // namespace sbtv
