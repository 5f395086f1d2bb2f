function [eb, results] = sbtv_sapg_wavelet_semiblind(Y, kind, h, levels, op, noise)
% [eb, results] = sbtv_sapg_wavelet_semiblind(Y, kind, h, levels, op [, noise])
% Semi-blind empirical Bayes for the wavelet-l1 prior (sbtv_SAPG_wavelet_semiblind): theta, the parameters p of a PSF family
% and sigma2 estimated together from one MYULA chain on the coefficients of the redundant wavelet frame.  It is
% SALSA/SAPG_algorithm_1.m with both of its parameters, `tau` being the PSF parameters with the closures of the TV half
% (SAPG/SAPG_algorithm_laplace.m:172-186); the loop is stated in include/sbtv.h.  No PSF is given: the blur is
% sbtv_psf_taps(kind, psf_size, p).
%   Y        M x N x B observations, one chain per image; M*N even
%   kind     0 gaussian (w1, w2), 1 moffat (alpha, beta), 2 laplace (b)
%   h        orthonormal scaling filter (e.g. daubcqf(2)); levels as for mrdwt_TI2D
%   op       samples, burnIn, th_init, min_th, max_th, d_scale, d_exp, lambda, gamma, sigma (sigma^2 is sigma2(1));
%            p_init, p_min, p_max, p_true, fix_p, c_p (1 x 2; a one-parameter family ignores slot 2; p_init may be 2 x B, one
%            column per chain); optional warmup (0), X0, seed (1), chain_offset (0), psf_size (7), phi (0), fix_sigma (1),
%            and for a free sigma2: sigma2_min, sigma2_max, c_sigma
%   noise    optional M x nb*N x B x steps normals instead of the device generator, steps = max(warmup-1,0) + samples-1
% eb: 4 x B (theta_EB; p0_EB; p1_EB; sigma2_EB).  results (per chain in columns): thetas, sigmas, gXTrace, logPiTraceX,
% tol_thetas samples x B; ps, tol_ps samples x 2 x B; grads samples x 3 x B (G_p0, G_p1, G_sigma2); logPiTrace_WU warmup x B;
% mean_thetas (samples-burnIn) x B; mean_ps (samples-burnIn) x 2 x B; mean_theta, p_EB, sigma2_EB; last_samp; Xlast_sample
% M x nb*N x B; options.
% WRITTEN WITHOUT ACCESS TO MATLAB: never executed, see INTEGRATION.md.
persistent ctx
if nargin < 6, noise = []; end
[M, N, B] = size(Y);
nb = 3 * (levels - 1) + 1;
if nb < 1, error('sbtv:wavelet', 'levels must be at least 2'); end
h = double(h(:));
warmup = 0; if isfield(op, 'warmup'), warmup = op.warmup; end
X0 = []; if isfield(op, 'X0'), X0 = op.X0; end
S = op.samples; nmean = max(S - op.burnIn, 1);
two = @(v) [double(v(:)); zeros(2 - numel(v), 1)];
pstart = double(op.p_init);
if size(pstart, 2) ~= B || numel(pstart) <= 2, pstart = repmat(two(op.p_init), 1, B); end
if size(pstart, 1) == 1, pstart = [pstart; zeros(1, B)]; end
o = libstruct('sbtv_sapg_wavelet_sb_opts');
o.samples = S; o.warmup = warmup; o.burnIn = op.burnIn;
o.lambda = op.lambda; o.gamma = op.gamma; o.sigma2 = op.sigma^2;
o.th_init = op.th_init; o.min_th = op.min_th; o.max_th = op.max_th;
o.d_scale = op.d_scale; o.d_exp = op.d_exp;
o.seed = 1; if isfield(op, 'seed'), o.seed = op.seed; end
o.chain_offset = 0; if isfield(op, 'chain_offset'), o.chain_offset = op.chain_offset; end
o.kind = kind;
o.psf_size = 7; if isfield(op, 'psf_size'), o.psf_size = op.psf_size; end
o.phi = 0; if isfield(op, 'phi'), o.phi = op.phi; end
o.fix_p = int32(two(op.fix_p));
o.p_init = pstart(:, 1); o.p_min = two(op.p_min); o.p_max = two(op.p_max); o.p_true = two(op.p_true); o.c_p = two(op.c_p);
o.fix_sigma = 1; if isfield(op, 'fix_sigma'), o.fix_sigma = op.fix_sigma; end
o.sigma2_min = o.sigma2; o.sigma2_max = o.sigma2; o.c_sigma = 0;
if isfield(op, 'sigma2_min'), o.sigma2_min = op.sigma2_min; end
if isfield(op, 'sigma2_max'), o.sigma2_max = op.sigma2_max; end
if isfield(op, 'c_sigma'), o.c_sigma = op.c_sigma; end
pth = libpointer('doublePtr', zeros(S, B)); psg = libpointer('doublePtr', zeros(S, B));
pgx = libpointer('doublePtr', zeros(S, B)); plp = libpointer('doublePtr', zeros(S, B));
pps = libpointer('doublePtr', zeros(S, 2, B)); pgr = libpointer('doublePtr', zeros(S, 3, B));
pwu = libpointer('doublePtr', zeros(max(warmup, 1), B));
pmean = libpointer('doublePtr', zeros(nmean, B)); ptol = libpointer('doublePtr', zeros(S, B));
pmeanp = libpointer('doublePtr', zeros(nmean, 2, B)); ptolp = libpointer('doublePtr', zeros(S, 2, B));
peb = libpointer('doublePtr', zeros(4, B)); pX = libpointer('doublePtr', zeros(M, nb * N, B));
if isempty(ctx), ctx = sbtv_load(0); end
rc = calllib('libsbtv', 'sbtv_SAPG_wavelet_semiblind', ctx, Y, int32(M), int32(N), int32(B), h, int32(numel(h)), ...
             int32(levels), o, pstart, X0, noise, pth, pps, psg, pgx, plp, pwu, pgr, pmean, ptol, pmeanp, ptolp, peb, pX, ...
             int32(0));
if rc ~= 0, error('sbtv:wavelet', '%s', calllib('libsbtv', 'sbtv_last_error', ctx)); end
eb = reshape(peb.Value, 4, B);
results.last_samp = S;
results.logPiTraceX = reshape(plp.Value, S, B); results.gXTrace = reshape(pgx.Value, S, B);
results.thetas = reshape(pth.Value, S, B); results.last_theta = results.thetas(end, :);
results.sigmas = reshape(psg.Value, S, B); results.ps = reshape(pps.Value, S, 2, B);
results.grads = reshape(pgr.Value, S, 3, B);
results.mean_theta = eb(1, :); results.p_EB = eb(2:3, :); results.sigma2_EB = eb(4, :);
mt = reshape(pmean.Value, nmean, B); results.mean_thetas = mt(1:(S - op.burnIn), :);
mp = reshape(pmeanp.Value, nmean, 2, B); results.mean_ps = mp(1:(S - op.burnIn), :, :);
results.tol_thetas = reshape(ptol.Value, S, B); results.tol_ps = reshape(ptolp.Value, S, 2, B);
if warmup > 0, results.logPiTrace_WU = reshape(pwu.Value, warmup, B); end
results.Xlast_sample = reshape(pX.Value, M, nb * N, B);
results.options = op;
end
