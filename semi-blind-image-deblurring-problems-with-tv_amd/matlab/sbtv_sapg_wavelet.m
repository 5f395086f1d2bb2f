function [theta_EB, results] = sbtv_sapg_wavelet(Y, H, h, levels, op, noise)
% [theta_EB, results] = sbtv_sapg_wavelet(Y, H, h, levels, op [, noise])
% Empirical-Bayes estimate of theta for the wavelet-l1 prior (sbtv_SAPG_wavelet): the MYULA chain on the coefficients of the
% redundant wavelet frame and the log-scale update of SALSA/SAPG_algorithm_1.m:165-216 (its theta part; the loop is stated in
% include/sbtv.h), as SALSA/run_deblur_synthesis_L1.m:125-156 runs it before the MAP solve (then sbtv_salsa_wavelet at
% tau = theta_EB*sigma^2, mu = theta_EB).
%   Y        M x N x B observations, one chain per image; M*N even
%   H        t x t PSF (one for all images) or t x t x B; t <= 15, top-left convention of utils/resize.m
%   h        orthonormal scaling filter (e.g. daubcqf(2)); levels as for mrdwt_TI2D
%   op       samples, burnIn, th_init, min_th, max_th, d_scale, d_exp, lambda, gamma, sigma (noise standard deviation);
%            optional warmup (0), X0 (M x nb*N x B start coefficients, default W'Y), seed (1), chain_offset (0)
%   noise    optional M x nb*N x B x steps normals instead of the device generator, steps = max(warmup-1,0) + samples-1
% results (per chain in columns): thetas, gXTrace, logPiTraceX, tol_thetas samples x B; logPiTrace_WU warmup x B; mean_thetas
% (samples-burnIn) x B; mean_theta, last_theta 1 x B; last_samp; Xlast_sample M x nb*N x B; options.
% WRITTEN WITHOUT ACCESS TO MATLAB: never executed, see INTEGRATION.md.
persistent ctx
if nargin < 6, noise = []; end
[M, N, B] = size(Y);
nb = 3 * (levels - 1) + 1;
if nb < 1, error('sbtv:wavelet', 'levels must be at least 2'); end
t = size(H, 1);
if size(H, 3) == 1, H = repmat(H, [1 1 B]); end
if size(H, 3) ~= B, error('sbtv:wavelet', 'H must be given once or once per image'); end
h = double(h(:));
warmup = 0; if isfield(op, 'warmup'), warmup = op.warmup; end
X0 = []; if isfield(op, 'X0'), X0 = op.X0; end
S = op.samples; nmean = max(S - op.burnIn, 1);
o = libstruct('sbtv_sapg_wavelet_opts');
o.samples = S; o.warmup = warmup; o.burnIn = op.burnIn;
o.lambda = op.lambda; o.gamma = op.gamma; o.sigma2 = op.sigma^2;
o.th_init = op.th_init; o.min_th = op.min_th; o.max_th = op.max_th;
o.d_scale = op.d_scale; o.d_exp = op.d_exp;
o.seed = 1; if isfield(op, 'seed'), o.seed = op.seed; end
o.chain_offset = 0; if isfield(op, 'chain_offset'), o.chain_offset = op.chain_offset; end
pth = libpointer('doublePtr', zeros(S, B)); pgx = libpointer('doublePtr', zeros(S, B));
plp = libpointer('doublePtr', zeros(S, B)); pwu = libpointer('doublePtr', zeros(max(warmup, 1), B));
pmean = libpointer('doublePtr', zeros(nmean, B)); ptol = libpointer('doublePtr', zeros(S, B));
peb = libpointer('doublePtr', zeros(1, B)); pX = libpointer('doublePtr', zeros(M, nb * N, B));
if isempty(ctx), ctx = sbtv_load(0); end
rc = calllib('libsbtv', 'sbtv_SAPG_wavelet', ctx, Y, int32(M), int32(N), int32(B), H, int32(t), h, int32(numel(h)), ...
             int32(levels), o, X0, noise, pth, pgx, plp, pwu, pmean, ptol, peb, pX, int32(0));
if rc ~= 0, error('sbtv:wavelet', '%s', calllib('libsbtv', 'sbtv_last_error', ctx)); end
theta_EB = peb.Value;
results.last_samp = S;
results.logPiTraceX = reshape(plp.Value, S, B); results.gXTrace = reshape(pgx.Value, S, B);
results.mean_theta = theta_EB; results.thetas = reshape(pth.Value, S, B); results.last_theta = results.thetas(end, :);
mt = reshape(pmean.Value, nmean, B); results.mean_thetas = mt(1:(S - op.burnIn), :);
results.tol_thetas = reshape(ptol.Value, S, B);
if warmup > 0, results.logPiTrace_WU = reshape(pwu.Value, warmup, B); end
results.Xlast_sample = reshape(pX.Value, M, nb * N, B);
results.options = op;
end
