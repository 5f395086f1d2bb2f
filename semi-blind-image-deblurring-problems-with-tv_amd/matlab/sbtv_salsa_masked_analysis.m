function [X, numA, numAt, objective, distance, times, mses, n_outer] = sbtv_salsa_masked_analysis(Y, H, mask, tau, mu1, varargin)
% [X, numA, numAt, objective, distance, times, mses, n_outer] = sbtv_salsa_masked_analysis(Y, H, mask, tau, mu1, ...)
% Wavelet-l1 deconvolution, analysis form, of observations with unknown boundaries and missing pixels
% (sbtv_SALSA_masked_analysis):
%     minimise over the image x   0.5 * sum( mask .* (B x - Y).^2 ) + tau * || W' x ||_1,
%     B = circular blur of H, W' = mrdwt_TI2D
% by the ADMM of Almeida & Figueiredo (IEEE TIP 2013) with the splits u = W' x and v = B x: the likelihood of sbtv_salsa_masked
% with the prior of sbtv_salsa_analysis; the iteration is stated in include/sbtv.h.  No counterpart in the reference.
%   Y, mask  M x N x B observations and non-negative weights (0 = not observed, 1 = observed); M*N even
%   H        t x t PSF (one for all images) or t x t x B (one per image); t <= 15, top-left convention of utils/resize.m
%   tau, mu1 scalars or 1 x B (mu1: the weight of the coefficient split, sbtv_salsa_analysis's mu)
% name / value options: 'MU2' (0.1; scalar or 1 x B: the weight of the data split - it decides the speed, not the answer),
%   'WAVELET' (orthonormal scaling filter, default [1 1]/sqrt(2)), 'LEVELS' (4), 'TRUE_X' (the true IMAGE, M x N x B),
%   'INITIALIZATION' (0, 2 = B'(mask .* Y), or an M x N x B start image), 'STOPCRITERION' (1), 'TOLERANCEA' (1e-3),
%   'MAXITERA' (10000).
% An observation without wrapped pixels (the 'valid' part of a linear blur, m x n) goes into a domain of
% (m+t-1) x (n+t-1) pixels (or a larger one) at rows / columns t, t+1, ... with mask = 1 there and 0 elsewhere.
% Outputs: X M x N x B; numA, numAt, n_outer 1 x B; objective, times, mses (maxiter+1) x B and distance 2 x maxiter x B
% (the relative distances of the two splits: coefficients, data), valid up to n_outer(b) (+1).
% WRITTEN WITHOUT ACCESS TO MATLAB: never executed, see INTEGRATION.md.
persistent ctx
stopCriterion = 1; maxiter = 10000; init = 0; tolA = 0.001; true_x = []; xinit = []; mu2 = 0.1; h = [1 1] / sqrt(2); levels = 4;
if (rem(length(varargin),2)==1), error('Optional parameters should always go by pairs'); end
for i = 1:2:(length(varargin)-1)
    switch upper(varargin{i})
        case 'MU2',            mu2 = varargin{i+1};
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
if levels < 2, error('sbtv:masked_analysis', 'levels must be at least 2'); end
if ~isequal(size(mask), size(Y)), error('sbtv:masked_analysis', 'the mask must have the size of Y'); end
if any(mask(:) < 0) || any(~isfinite(mask(:))), error('sbtv:masked_analysis', 'the mask must be finite and non-negative'); end
t = size(H, 1);
if size(H, 3) == 1, H = repmat(H, [1 1 B]); end
if numel(tau) == 1, tau = repmat(tau, 1, B); end
if numel(mu1) == 1, mu1 = repmat(mu1, 1, B); end
if numel(mu2) == 1, mu2 = repmat(mu2, 1, B); end
if size(H, 3) ~= B || numel(tau) ~= B || numel(mu1) ~= B || numel(mu2) ~= B
    error('sbtv:masked_analysis', 'H, tau, mu1 and mu2 must be given once or once per image');
end
for c = {true_x, xinit}
    if ~isempty(c{1}) && ~isequal([size(c{1}, 1) size(c{1}, 2) size(c{1}, 3)], [M N B])
        error('sbtv:masked_analysis', 'TRUE_X and an array INITIALIZATION must be M x N x B images');
    end
end
h = double(h(:));
mask = double(mask);
o = libstruct('sbtv_salsa_opts');
calllib('libsbtv', 'sbtv_salsa_opts_default', o);
o.stopcriterion = stopCriterion; o.maxiter = maxiter; o.initialization = init;
o.compute_mse = ~isempty(true_x); o.tolA = tolA;
pX = libpointer('doublePtr', zeros(M, N, B));
pobj = libpointer('doublePtr', zeros(maxiter+1, B)); pdist = libpointer('doublePtr', zeros(2, maxiter, B));
ptim = libpointer('doublePtr', zeros(maxiter+1, B)); pmse = libpointer('doublePtr', zeros(maxiter+1, B));
pnA = libpointer('int32Ptr', zeros(1, B, 'int32')); pnAt = libpointer('int32Ptr', zeros(1, B, 'int32'));
pn = libpointer('int32Ptr', zeros(1, B, 'int32'));
if isempty(ctx), ctx = sbtv_load(0); end
rc = calllib('libsbtv', 'sbtv_SALSA_masked_analysis', ctx, Y, mask, int32(M), int32(N), int32(B), H, int32(t), h, ...
             int32(numel(h)), int32(levels), tau, mu1, mu2, o, true_x, xinit, pX, pobj, pdist, ptim, pmse, pnA, pnAt, pn, int32(0));
if rc ~= 0, error('sbtv:masked_analysis', '%s', calllib('libsbtv', 'sbtv_last_error', ctx)); end
X = reshape(pX.Value, M, N, B);
numA = double(pnA.Value); numAt = double(pnAt.Value); n_outer = double(pn.Value);
objective = reshape(pobj.Value, maxiter+1, B); distance = reshape(pdist.Value, 2, maxiter, B);
times = reshape(ptim.Value, maxiter+1, B);
if ~isempty(true_x), mses = reshape(pmse.Value, maxiter+1, B); else, mses = []; end
end
