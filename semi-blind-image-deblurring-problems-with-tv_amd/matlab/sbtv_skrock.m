function results = sbtv_skrock(Y, H, op, theta, sigma2, noise)
% results = sbtv_skrock(Y, H, op, theta, sigma2 [, noise])
% SK-ROCK chain on the TV posterior at FIXED theta, PSF and sigma2 (sbtv_skrock): the target and the closures of myula
% (SALSA/run_deblur_tv.m:126,131) with the explicit stabilised step of Pereyra, Vargas Mieles and Zygalakis (SIAM J. Imaging
% Sci. 2020); the step is stated in include/sbtv.h.  One step costs op.stages drift evaluations (a cold Chambolle prox and a
% gradient each) and is stable for op.delta <= l_s / (1 / sigma2 + 1 / lambda) (sbtv_skrock_max_step), about
% stages^2 (2 - 4 eta / 3) times the gamma of MYULA.  Sample 1 is the start state, op.samples-1 steps follow.
%   Y        M x N x B observations, one chain per image; M*N even
%   H        t x t PSF (one for all images) or t x t x B; t <= 15, top-left convention of utils/resize.m
%   op       samples, stages, lambda; optional chambolleit (25), delta (0.8 of the bound at ||A|| = 1 and the smallest sigma2),
%            eta (0.05), X0 (M x N x B start images, default Y), seed (1), chain_offset (0), posterior_first (1),
%            posterior_thin (1), posterior_pooled (0)
%   theta, sigma2   a scalar or one value per image
%   noise    optional M x N x B x (samples-1) normals instead of the device generator
% results: gXTrace, logPiTraceX (samples x B); Xlast_sample; posteriormean, posteriorvar, posteriorcount (the moments of the
% samples posterior_first : posterior_thin : samples); options.
% WRITTEN WITHOUT ACCESS TO MATLAB: never executed, see INTEGRATION.md.
persistent ctx
if nargin < 6, noise = []; end
[M, N, B] = size(Y);
t = size(H, 1);
if size(H, 3) == 1, H = repmat(H, [1 1 B]); end
if size(H, 3) ~= B, error('sbtv:skrock', 'H must be given once or once per image'); end
if isscalar(theta), theta = repmat(theta, 1, B); end
if isscalar(sigma2), sigma2 = repmat(sigma2, 1, B); end
if numel(theta) ~= B || numel(sigma2) ~= B, error('sbtv:skrock', 'theta and sigma2 must be scalars or one per image'); end
theta = double(theta(:)); sigma2 = double(sigma2(:));
X0 = []; if isfield(op, 'X0'), X0 = op.X0; end
S = op.samples;
if isempty(ctx), ctx = sbtv_load(0); end
o = libstruct('sbtv_skrock_opts');
o.samples = S; o.stages = op.stages; o.lambda = op.lambda;
o.chambolleit = 25; if isfield(op, 'chambolleit'), o.chambolleit = op.chambolleit; end
o.eta = 0.05; if isfield(op, 'eta'), o.eta = op.eta; end
if isfield(op, 'delta') && ~isempty(op.delta)
    o.delta = op.delta;
else
    pd = libpointer('doublePtr', 0);
    rc = calllib('libsbtv', 'sbtv_skrock_max_step', int32(op.stages), o.eta, min(sigma2), op.lambda, 1, pd);
    if rc ~= 0, error('sbtv:skrock', '%s', calllib('libsbtv', 'sbtv_last_error', [])); end
    o.delta = 0.8 * pd.Value;
end
o.seed = 1; if isfield(op, 'seed'), o.seed = op.seed; end
o.chain_offset = 0; if isfield(op, 'chain_offset'), o.chain_offset = op.chain_offset; end
pgx = libpointer('doublePtr', zeros(S, B)); plp = libpointer('doublePtr', zeros(S, B));
pX = libpointer('doublePtr', zeros(M, N, B));
mo = libstruct('sbtv_moments_opts');
mo.first = int32(1); if isfield(op, 'posterior_first'), mo.first = int32(op.posterior_first); end
mo.thin = int32(1); if isfield(op, 'posterior_thin'), mo.thin = int32(op.posterior_thin); end
mo.pooled = int32(0); if isfield(op, 'posterior_pooled'), mo.pooled = int32(op.posterior_pooled ~= 0); end
Bo = B; if mo.pooled, Bo = 1; end
pm = libpointer('doublePtr', zeros(M, N, Bo)); pv = libpointer('doublePtr', zeros(M, N, Bo));
rc = calllib('libsbtv', 'sbtv_skrock', ctx, Y, int32(M), int32(N), int32(B), H, int32(t), o, theta, sigma2, X0, noise, ...
             pgx, plp, pX, mo, pm, pv, [], int32(0));
if rc ~= 0, error('sbtv:skrock', '%s', calllib('libsbtv', 'sbtv_last_error', ctx)); end
results.gXTrace = reshape(pgx.Value, S, B); results.logPiTraceX = reshape(plp.Value, S, B);
results.Xlast_sample = reshape(pX.Value, M, N, B);
results.posteriormean = reshape(pm.Value, M, N, Bo); results.posteriorvar = reshape(pv.Value, M, N, Bo);
n = floor((S - double(mo.first)) / double(mo.thin)) + 1;                 % samples first:thin:samples
results.posteriorcount = n * (B / Bo);
results.options = op;
end
