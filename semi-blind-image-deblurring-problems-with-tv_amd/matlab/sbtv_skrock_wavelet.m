function results = sbtv_skrock_wavelet(Y, H, h, levels, op, theta, sigma2, noise)
% results = sbtv_skrock_wavelet(Y, H, h, levels, op, theta, sigma2 [, noise])
% SK-ROCK chain on the coefficients of the redundant wavelet frame at a FIXED theta (sbtv_skrock_wavelet): the target, the
% arguments and the results of sbtv_myula_wavelet with the explicit stabilised step of Pereyra, Vargas Mieles and Zygalakis
% (SIAM J. Imaging Sci. 2020); the step is stated in include/sbtv.h.  One step costs op.stages gradient evaluations and is
% stable for op.delta <= l_s / (||B||^2 / sigma2 + 1 / lambda) (sbtv_skrock_max_step), about stages^2 (2 - 4 eta / 3) times the
% gamma of MYULA.  Sample 1 is the start state, op.samples-1 steps follow.
%   Y        M x N x B observations, one chain per image; M*N even
%   H        t x t PSF (one for all images) or t x t x B; t <= 15, top-left convention of utils/resize.m
%   h        orthonormal scaling filter (e.g. daubcqf(2)); levels as for mrdwt_TI2D
%   op       samples, stages, lambda; optional delta (0.8 of the bound at ||B|| = 1 and the smallest sigma2), eta (0.05), X0
%            (M x nb*N x B start coefficients, default W'Y), seed (1), chain_offset (0), posterior_first (1), posterior_thin (1),
%            posterior_pooled (0), posterior_coefficients (0)
%   theta, sigma2   a scalar or one value per image
%   noise    optional M x nb*N x B x (samples-1) normals instead of the device generator
% results: as sbtv_myula_wavelet (gXTrace, logPiTraceX samples x B; Xlast_sample; posteriormean, posteriorvar, posteriorcount;
% coefmean, coefvar when op.posterior_coefficients; options).
% WRITTEN WITHOUT ACCESS TO MATLAB: never executed, see INTEGRATION.md.
persistent ctx
if nargin < 8, noise = []; end
[M, N, B] = size(Y);
nb = 3 * (levels - 1) + 1;
if nb < 1, error('sbtv:wavelet', 'levels must be at least 2'); end
t = size(H, 1);
if size(H, 3) == 1, H = repmat(H, [1 1 B]); end
if size(H, 3) ~= B, error('sbtv:wavelet', 'H must be given once or once per image'); end
h = double(h(:));
if isscalar(theta), theta = repmat(theta, 1, B); end
if isscalar(sigma2), sigma2 = repmat(sigma2, 1, B); end
if numel(theta) ~= B || numel(sigma2) ~= B, error('sbtv:wavelet', 'theta and sigma2 must be scalars or one per image'); end
theta = double(theta(:)); sigma2 = double(sigma2(:));
X0 = []; if isfield(op, 'X0'), X0 = op.X0; end
S = op.samples;
if isempty(ctx), ctx = sbtv_load(0); end
o = libstruct('sbtv_skrock_wavelet_opts');
o.samples = S; o.stages = op.stages; o.lambda = op.lambda;
o.eta = 0.05; if isfield(op, 'eta'), o.eta = op.eta; end
if isfield(op, 'delta') && ~isempty(op.delta)
    o.delta = op.delta;
else
    pd = libpointer('doublePtr', 0);
    rc = calllib('libsbtv', 'sbtv_skrock_max_step', int32(op.stages), o.eta, min(sigma2), op.lambda, 1, pd);
    if rc ~= 0, error('sbtv:wavelet', '%s', calllib('libsbtv', 'sbtv_last_error', [])); end
    o.delta = 0.8 * pd.Value;
end
o.seed = 1; if isfield(op, 'seed'), o.seed = op.seed; end
o.chain_offset = 0; if isfield(op, 'chain_offset'), o.chain_offset = op.chain_offset; end
mo = libstruct('sbtv_moments_opts');
mo.first = int32(1); if isfield(op, 'posterior_first'), mo.first = int32(op.posterior_first); end
mo.thin = int32(1); if isfield(op, 'posterior_thin'), mo.thin = int32(op.posterior_thin); end
mo.pooled = int32(0); if isfield(op, 'posterior_pooled'), mo.pooled = int32(op.posterior_pooled ~= 0); end
coefs = isfield(op, 'posterior_coefficients') && op.posterior_coefficients;
Bo = B; if mo.pooled, Bo = 1; end
pgx = libpointer('doublePtr', zeros(S, B)); plp = libpointer('doublePtr', zeros(S, B));
pX = libpointer('doublePtr', zeros(M, nb * N, B));
pm = libpointer('doublePtr', zeros(M, N, Bo)); pv = libpointer('doublePtr', zeros(M, N, Bo));
if coefs
    pcm = libpointer('doublePtr', zeros(M, nb * N, Bo)); pcv = libpointer('doublePtr', zeros(M, nb * N, Bo));
    rc = calllib('libsbtv', 'sbtv_skrock_wavelet', ctx, Y, int32(M), int32(N), int32(B), H, int32(t), h, int32(numel(h)), ...
                 int32(levels), o, theta, sigma2, X0, noise, pgx, plp, pX, mo, pm, pv, [], pcm, pcv, int32(0));
else
    rc = calllib('libsbtv', 'sbtv_skrock_wavelet', ctx, Y, int32(M), int32(N), int32(B), H, int32(t), h, int32(numel(h)), ...
                 int32(levels), o, theta, sigma2, X0, noise, pgx, plp, pX, mo, pm, pv, [], [], [], int32(0));
end
if rc ~= 0, error('sbtv:wavelet', '%s', calllib('libsbtv', 'sbtv_last_error', ctx)); end
results.gXTrace = reshape(pgx.Value, S, B); results.logPiTraceX = reshape(plp.Value, S, B);
results.Xlast_sample = reshape(pX.Value, M, nb * N, B);
results.posteriormean = reshape(pm.Value, M, N, Bo); results.posteriorvar = reshape(pv.Value, M, N, Bo);
n = floor((S - double(mo.first)) / double(mo.thin)) + 1;                 % samples first:thin:samples
results.posteriorcount = n * (B / Bo);
if coefs
    results.coefmean = reshape(pcm.Value, M, nb * N, Bo); results.coefvar = reshape(pcv.Value, M, nb * N, Bo);
end
results.options = op;
end
