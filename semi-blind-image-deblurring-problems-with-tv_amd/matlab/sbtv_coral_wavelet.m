function [X, numA, numAt, objective, distance, times, mses, n_outer] = sbtv_coral_wavelet(Y, H, tau1, tau2, mu1, mu2, varargin)
% [X, numA, numAt, objective, distance, times, mses, n_outer] = sbtv_coral_wavelet(Y, H, tau1, tau2, mu1, mu2, ...)
% CoRAL with the compound regulariser TV + wavelet-l1 (sbtv_CoRAL_wavelet):
%     minimise over the image x   0.5 * || Y - B x ||^2 + tau1 * TV(x) + tau2 * || W' x ||_1,
%     B = circular blur of H, W' = mrdwt_TI2D
% the problem CoRAL solves when it is given 'TVINITIALIZATION1' = 1 and 'P2' = W = mirdwt_TI2D, 'P2T' = W' with 'PSI2' = soft and
% 'LS' for mu1 + mu2 (SALSA/CoRAL_v2.m:137, 349-476); the iteration is stated in include/sbtv.h.
%   Y                     M x N x B observations; M*N even
%   H                     t x t PSF (one for all images) or t x t x B (one per image); t <= 15, top-left convention of utils/resize.m
%   tau1, tau2, mu1, mu2  scalars or 1 x B; mu1, mu2 > 0
% name / value options: 'WAVELET' (orthonormal scaling filter, default [1 1]/sqrt(2)), 'LEVELS' (4), 'TVITERS' (5), 'TRUE_X' (the
%   true IMAGE, M x N x B), 'INITIALIZATION' (0, 2 = B' Y, or an M x N x B start image), 'STOPCRITERION' (1), 'TOLERANCEA' (1e-3),
%   'MAXITERA' (10000).
% Outputs: X M x N x B; numA, numAt, n_outer 1 x B; objective, times, mses (maxiter+1) x B; distance 2 x maxiter x B, row 1 the TV
% split ||x - u||, row 2 the wavelet split ||W'x - v||, both relative; column b valid up to n_outer(b) (+1).
% WRITTEN WITHOUT ACCESS TO MATLAB: never executed, see INTEGRATION.md.
persistent ctx
stopCriterion = 1; maxiter = 10000; init = 0; tolA = 0.001; true_x = []; xinit = []; h = [1 1] / sqrt(2); levels = 4; TViters = 5;
if (rem(length(varargin),2)==1), error('Optional parameters should always go by pairs'); end
for i = 1:2:(length(varargin)-1)
    switch upper(varargin{i})
        case 'WAVELET',        h = varargin{i+1};
        case 'LEVELS',         levels = varargin{i+1};
        case 'TVITERS',        TViters = varargin{i+1};
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
if levels < 2, error('sbtv:coral_wavelet', 'levels must be at least 2'); end
t = size(H, 1);
if size(H, 3) == 1, H = repmat(H, [1 1 B]); end
if numel(tau1) == 1, tau1 = repmat(tau1, 1, B); end
if numel(tau2) == 1, tau2 = repmat(tau2, 1, B); end
if numel(mu1) == 1, mu1 = repmat(mu1, 1, B); end
if numel(mu2) == 1, mu2 = repmat(mu2, 1, B); end
if size(H, 3) ~= B || numel(tau1) ~= B || numel(tau2) ~= B || numel(mu1) ~= B || numel(mu2) ~= B
    error('sbtv:coral_wavelet', 'H, tau1, tau2, mu1 and mu2 must be given once or once per image');
end
for c = {true_x, xinit}
    if ~isempty(c{1}) && ~isequal([size(c{1}, 1) size(c{1}, 2) size(c{1}, 3)], [M N B])
        error('sbtv:coral_wavelet', 'TRUE_X and an array INITIALIZATION must be M x N x B images');
    end
end
h = double(h(:));
o = libstruct('sbtv_salsa_opts');
calllib('libsbtv', 'sbtv_salsa_opts_default', o);
o.stopcriterion = stopCriterion; o.maxiter = maxiter; o.initialization = init; o.TViters = TViters;
o.compute_mse = ~isempty(true_x); o.tolA = tolA;
pX = libpointer('doublePtr', zeros(M, N, B));
pobj = libpointer('doublePtr', zeros(maxiter+1, B)); pdist = libpointer('doublePtr', zeros(2, maxiter, B));
ptim = libpointer('doublePtr', zeros(maxiter+1, B)); pmse = libpointer('doublePtr', zeros(maxiter+1, B));
pnA = libpointer('int32Ptr', zeros(1, B, 'int32')); pnAt = libpointer('int32Ptr', zeros(1, B, 'int32'));
pn = libpointer('int32Ptr', zeros(1, B, 'int32'));
if isempty(ctx), ctx = sbtv_load(0); end
rc = calllib('libsbtv', 'sbtv_CoRAL_wavelet', ctx, Y, int32(M), int32(N), int32(B), H, int32(t), h, int32(numel(h)), ...
             int32(levels), tau1, tau2, mu1, mu2, o, true_x, xinit, pX, pobj, pdist, ptim, pmse, pnA, pnAt, pn, int32(0));
if rc ~= 0, error('sbtv:coral_wavelet', '%s', calllib('libsbtv', 'sbtv_last_error', ctx)); end
X = reshape(pX.Value, M, N, B);
numA = double(pnA.Value); numAt = double(pnAt.Value); n_outer = double(pn.Value);
objective = reshape(pobj.Value, maxiter+1, B); distance = reshape(pdist.Value, 2, maxiter, B);
times = reshape(ptim.Value, maxiter+1, B);
if ~isempty(true_x), mses = reshape(pmse.Value, maxiter+1, B); else, mses = []; end
end
