function [X, numA, numAt, objective, distance1, distance2, criterion, times, mses, n_outer] = sbtv_csalsa_wavelet(Y, H, mu1, mu2, sigma, varargin)
% [X, numA, numAt, objective, distance1, distance2, criterion, times, mses, n_outer] = sbtv_csalsa_wavelet(Y, H, mu1, mu2, sigma, ...)
% C-SALSA with the wavelet analysis prior (sbtv_CSALSA_wavelet):
%     minimise over the image x   || W' x ||_1   subject to   || B x - Y ||_2 <= epsilon,   B = circular blur of H, W' = mrdwt_TI2D
% the problem csalsa solves when it is given 'P' = W = mirdwt_TI2D and 'PT' = W' with 'Psi' = soft (SALSA/CSALSA_v2.m:111-114,
% 208-213, 402, 467-478, 492) and invLS(r, mu1) = real(ifft2(fft2(r) ./ (abs(fft2(H)).^2 + mu1))); the iteration is stated in
% include/sbtv.h.  objective is || W' x ||_1 (the reference records phi of the image).
%   Y               M x N x B observations; M*N even
%   H               t x t PSF (one for all images) or t x t x B (one per image); t <= 15, top-left convention of utils/resize.m
%   mu1, mu2, sigma scalars or 1 x B; sigma is the noise standard deviation
% name / value options: 'WAVELET' (orthonormal scaling filter, default [1 1]/sqrt(2)), 'LEVELS' (4), 'TRUE_X' (the true IMAGE,
%   M x N x B), 'INITIALIZATION' (0, 2 = B' Y, or an M x N x B start image), 'STOPCRITERION' (3), 'TOLERANCEA' (1e-3),
%   'MAXITERA' (10000), 'CONTINUATIONFACTOR' (1), 'EPSILON' (0: sqrt(M*N + 8*sqrt(M*N)) * sigma; a scalar or 1 x B).
% Outputs: X M x N x B; numA, numAt, n_outer 1 x B; the traces maxiter x B, column b valid up to n_outer(b) (entry 1 is the
% state before the loop, as in the reference).
% WRITTEN WITHOUT ACCESS TO MATLAB: never executed, see INTEGRATION.md.
persistent ctx
stopCriterion = 3; maxiter = 10000; init = 0; tolA = 0.001; true_x = []; xinit = []; h = [1 1] / sqrt(2); levels = 4;
delta = 1; epsilon = 0;
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
        case 'CONTINUATIONFACTOR', delta = varargin{i+1};
        case 'EPSILON',        epsilon = varargin{i+1};
        otherwise, error(['Unrecognized option: ''' varargin{i} '''']);
    end
end
if (sum(stopCriterion == [1 2 3])==0), error('Unknown stopping criterion'); end
[M, N, B] = size(Y);
if levels < 2, error('sbtv:csalsa_wavelet', 'levels must be at least 2'); end
t = size(H, 1);
if size(H, 3) == 1, H = repmat(H, [1 1 B]); end
if numel(mu1) == 1, mu1 = repmat(mu1, 1, B); end
if numel(mu2) == 1, mu2 = repmat(mu2, 1, B); end
if numel(sigma) == 1, sigma = repmat(sigma, 1, B); end
if numel(epsilon) == 1, epsilon = repmat(epsilon, 1, B); end
if size(H, 3) ~= B || numel(mu1) ~= B || numel(mu2) ~= B || numel(sigma) ~= B || numel(epsilon) ~= B
    error('sbtv:csalsa_wavelet', 'H, mu1, mu2, sigma and EPSILON must be given once or once per image');
end
for c = {true_x, xinit}
    if ~isempty(c{1}) && ~isequal([size(c{1}, 1) size(c{1}, 2) size(c{1}, 3)], [M N B])
        error('sbtv:csalsa_wavelet', 'TRUE_X and an array INITIALIZATION must be M x N x B images');
    end
end
h = double(h(:));
o = libstruct('sbtv_salsa_opts');
calllib('libsbtv', 'sbtv_salsa_opts_default', o);
o.stopcriterion = stopCriterion; o.maxiter = maxiter; o.initialization = init;
o.compute_mse = ~isempty(true_x); o.tolA = tolA;
pX = libpointer('doublePtr', zeros(M, N, B));
pobj = libpointer('doublePtr', zeros(maxiter, B)); pd1 = libpointer('doublePtr', zeros(maxiter, B));
pd2 = libpointer('doublePtr', zeros(maxiter, B)); pcrit = libpointer('doublePtr', zeros(maxiter, B));
ptim = libpointer('doublePtr', zeros(maxiter, B)); pmse = libpointer('doublePtr', zeros(maxiter, B));
pnA = libpointer('int32Ptr', zeros(1, B, 'int32')); pnAt = libpointer('int32Ptr', zeros(1, B, 'int32'));
pn = libpointer('int32Ptr', zeros(1, B, 'int32'));
if isempty(ctx), ctx = sbtv_load(0); end
rc = calllib('libsbtv', 'sbtv_CSALSA_wavelet', ctx, Y, int32(M), int32(N), int32(B), H, int32(t), h, int32(numel(h)), ...
             int32(levels), mu1, mu2, sigma, epsilon, delta, o, true_x, xinit, pX, pobj, pd1, pd2, pcrit, ptim, pmse, ...
             pnA, pnAt, pn, int32(0));
if rc ~= 0, error('sbtv:csalsa_wavelet', '%s', calllib('libsbtv', 'sbtv_last_error', ctx)); end
X = reshape(pX.Value, M, N, B);
numA = double(pnA.Value); numAt = double(pnAt.Value); n_outer = double(pn.Value);
objective = reshape(pobj.Value, maxiter, B); distance1 = reshape(pd1.Value, maxiter, B);
distance2 = reshape(pd2.Value, maxiter, B); criterion = reshape(pcrit.Value, maxiter, B);
times = reshape(ptim.Value, maxiter, B);
if ~isempty(true_x), mses = reshape(pmse.Value, maxiter, B); else, mses = []; end
end
