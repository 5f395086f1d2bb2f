function [xMAP, post] = myula(op, im)
% Replacement of SALSA/myula.m:1-22 (plain MYULA chain at fixed theta / PSF, last sample returned) through libsbtv.so
% (sbtv_myula), with the closures of SALSA/run_deblur_tv.m:126,131 built in: proxG = Chambolle prox with op.lambda*theta,
% gradF = AT(A x - y)/sigma2.  WRITTEN WITHOUT ACCESS TO MATLAB: never executed, see INTEGRATION.md.
%
% op: y, lambda, gamma, theta_op, samples as in the reference, plus what its closures captured and the C-ABI needs as data:
% op.psf (taps, or op.A to probe), op.sigma2 (the tau_op of gradF), op.chambolleit (default 25), op.seed (default 1).
% The normals come from the device Philox stream (MATLAB's randn stream cannot be reproduced).
% Second output (sbtv_myula_moments): post.mean / post.var (unbiased, M2/(n-1)) of the iterations op.posterior_first
% (default 1 = y), every op.posterior_thin-th (default 1), up to the last one; post.count = n.
persistent ctx
if isempty(ctx), ctx = sbtv_load(0); end
[M, N] = size(op.y);
if isfield(op, 'psf'), h = op.psf; else, h = sbtv_psf_of_handle(op.A, M, N); end
K = 25; if isfield(op, 'chambolleit'), K = op.chambolleit; end
seed = 1; if isfield(op, 'seed'), seed = op.seed; end
px = libpointer('doublePtr', zeros(M,N));
if nargout < 2
    rc = calllib('libsbtv', 'sbtv_myula', ctx, op.y, int32(M), int32(N), int32(1), h, int32(size(h,1)), op.lambda, ...
                 op.gamma, op.theta_op, op.sigma2, int32(op.samples), int32(K), uint64(seed), int32(0), [], px, int32(0));
else
    mo = libstruct('sbtv_moments_opts');
    mo.first = int32(1); if isfield(op, 'posterior_first'), mo.first = int32(op.posterior_first); end
    mo.thin = int32(1); if isfield(op, 'posterior_thin'), mo.thin = int32(op.posterior_thin); end
    mo.pooled = int32(0);
    pm = libpointer('doublePtr', zeros(M,N)); pv = libpointer('doublePtr', zeros(M,N));
    rc = calllib('libsbtv', 'sbtv_myula_moments', ctx, op.y, int32(M), int32(N), int32(1), h, int32(size(h,1)), ...
                 op.lambda, op.gamma, op.theta_op, op.sigma2, int32(op.samples), int32(K), uint64(seed), int32(0), [], ...
                 px, mo, pm, pv, [], int32(0));
end
if rc ~= 0, error('sbtv:myula', '%s', calllib('libsbtv', 'sbtv_last_error', ctx)); end
xMAP = reshape(px.Value, M, N);
if nargout >= 2
    n = floor((max(1, op.samples - 1) - double(mo.first)) / double(mo.thin)) + 1;   % iterations first:thin:last
    post = struct('mean', reshape(pm.Value, M, N), 'var', reshape(pv.Value, M, N), 'count', n);
end
end
