function [X, numA, numAt, objective, distance, times, mses, n_outer] = sbtv_salsa_analysis(Y, H, tau, mu, varargin)
% [X, numA, numAt, objective, distance, times, mses, n_outer] = sbtv_salsa_analysis(Y, H, tau, mu, ...)
% Wavelet-l1 deconvolution in the analysis form (sbtv_SALSA_analysis):
%     minimise over the image x   0.5 * || Y - B x ||^2 + tau * || W' x ||_1,   B = circular blur of H, W' = mrdwt_TI2D
% the problem SALSA_v2 solves when it is given 'P' = W = mirdwt_TI2D and 'PT' = W' with 'Psi' = soft (SALSA/SALSA_v2.m:98-101,
% 389-440); the iteration is stated in include/sbtv.h.
%   Y        M x N x B observations; M*N even
%   H        t x t PSF (one for all images) or t x t x B (one per image); t <= 15, top-left convention of utils/resize.m
%   tau, mu  scalars or 1 x B
% name / value options: 'WAVELET' (orthonormal scaling filter, default [1 1]/sqrt(2)), 'LEVELS' (4), 'TRUE_X' (the true IMAGE,
%   M x N x B), 'INITIALIZATION' (0, 2 = B' Y, or an M x N x B start image), 'STOPCRITERION' (1), 'TOLERANCEA' (1e-3),
%   'MAXITERA' (10000).
% Outputs: X M x N x B; numA, numAt, n_outer 1 x B; objective, times, mses (maxiter+1) x B and distance maxiter x B, column b
% valid up to n_outer(b) (+1).
% WRITTEN WITHOUT ACCESS TO MATLAB: never executed, see INTEGRATION.md.
persistent ctx
stopCriterion = 1; maxiter = 10000; init = 0; tolA = 0.001; true_x = []; xinit = []; h = [1 1] / sqrt(2); levels = 4;
if (rem(length(varargin),2)==1), error('Optional parameters should always go by pairs'); end
for i = 1:2:(length(varargin)-1)
    switch upper(varargin{i})
        case 'WAVELET',        h = varargin{i+1};
        case 'LEVELS',         levels = varargin{i+1};
        case 'TRUE_X',         true_x = varargin{i+1};
        case 'INITIALIZATION'
            if numel(varargin{i+1}) > 1, init = 33333; xinit = varargin{i+1}; else, init = varargin{i+1}; end
        case 'STOPCRITERION',  stopCriterion = varargin{i+1};
        case 'TOLERANCEA',     tolA = varargin{i+1};
        case 'MAXITERA',       maxiter = varargin{i+1};
        otherwise, error(['Unrecognized option: ''' varargin{i} '''']);
    end
end
if (sum(stopCriterion == [1 2 3])==0), error('Unknown stopping criterion'); end
[M, N, B] = size(Y);
if levels < 2, error('sbtv:analysis', 'levels must be at least 2'); end
t = size(H, 1);
if size(H, 3) == 1, H = repmat(H, [1 1 B]); end
if numel(tau) == 1, tau = repmat(tau, 1, B); end
if numel(mu) == 1, mu = repmat(mu, 1, B); end
if size(H, 3) ~= B || numel(tau) ~= B || numel(mu) ~= B
    error('sbtv:analysis', 'H, tau and mu must be given once or once per image');
end
for c = {true_x, xinit}
    if ~isempty(c{1}) && ~isequal([size(c{1}, 1) size(c{1}, 2) size(c{1}, 3)], [M N B])
        error('sbtv:analysis', 'TRUE_X and an array INITIALIZATION must be M x N x B images');
    end
end
h = double(h(:));
o = libstruct('sbtv_salsa_opts');
calllib('libsbtv', 'sbtv_salsa_opts_default', o);
o.stopcriterion = stopCriterion; o.maxiter = maxiter; o.initialization = init;
o.compute_mse = ~isempty(true_x); o.tolA = tolA;
pX = libpointer('doublePtr', zeros(M, N, B));
pobj = libpointer('doublePtr', zeros(maxiter+1, B)); pdist = libpointer('doublePtr', zeros(maxiter, B));
ptim = libpointer('doublePtr', zeros(maxiter+1, B)); pmse = libpointer('doublePtr', zeros(maxiter+1, B));
pnA = libpointer('int32Ptr', zeros(1, B, 'int32')); pnAt = libpointer('int32Ptr', zeros(1, B, 'int32'));
pn = libpointer('int32Ptr', zeros(1, B, 'int32'));
if isempty(ctx), ctx = sbtv_load(0); end
rc = calllib('libsbtv', 'sbtv_SALSA_analysis', ctx, Y, int32(M), int32(N), int32(B), H, int32(t), h, int32(numel(h)), ...
             int32(levels), tau, mu, o, true_x, xinit, pX, pobj, pdist, ptim, pmse, pnA, pnAt, pn, int32(0));
if rc ~= 0, error('sbtv:analysis', '%s', calllib('libsbtv', 'sbtv_last_error', ctx)); end
X = reshape(pX.Value, M, N, B);
numA = double(pnA.Value); numAt = double(pnAt.Value); n_outer = double(pn.Value);
objective = reshape(pobj.Value, maxiter+1, B); distance = reshape(pdist.Value, maxiter, B);
times = reshape(ptim.Value, maxiter+1, B);
if ~isempty(true_x), mses = reshape(pmse.Value, maxiter+1, B); else, mses = []; end
end
