function [Wx, objective, times, mses, XW, n_iter] = sbtv_fista_l1(b, H, tau, stopcriterion, tolerance, maxiters, true_xw, varargin)
% [Wx, objective, times, mses, XW, n_iter] = sbtv_fista_l1(b, H, tau, stopcriterion, tolerance, maxiters, true_xw, ...)
% FISTA on the wavelet-l1 problem (sbtv_fista_l1), the comparison method of the SALSA toolbox (SALSA/my_fista_l1.m):
%     minimise over x   0.5 * || b - B W x ||^2 + tau * || x ||_1,   B = circular blur of H, W = mirdwt_TI2D
% the iteration is stated in include/sbtv.h.  The reference's handles W / WT are the frame itself here ('WAVELET', 'LEVELS').
%   b        M x N x B observations; M*N even
%   H        t x t PSF (one for all images) or t x t x B (one per image); t <= 15, top-left convention of utils/resize.m
%   tau      scalar or 1 x B
%   true_xw  the true COEFFICIENTS, M x nb*N x B with nb = 3*(levels-1)+1, or [] (no mses)
% name / value options: 'WAVELET' (orthonormal scaling filter, default [1 1]/sqrt(2)), 'LEVELS' (4), 'L' (1, as the
%   reference fixes it), 'XW_INIT' (start coefficients, M x nb*N x B; default the zero start of the reference), 'LAG' (1; 0:
%   the host waits for every iteration, same result).
% Outputs: Wx = W XW M x N x B, XW M x nb*N x B the coefficients of the stopping iteration; n_iter 1 x B; objective, times,
% mses maxiters x B, column b valid up to n_iter(b).
% WRITTEN WITHOUT ACCESS TO MATLAB: never executed, see INTEGRATION.md.
persistent ctx
h = [1 1] / sqrt(2); levels = 4; L = 1; xinit = []; lag = 1;
if (rem(length(varargin),2)==1), error('Optional parameters should always go by pairs'); end
for i = 1:2:(length(varargin)-1)
    switch upper(varargin{i})
        case 'WAVELET',  h = varargin{i+1};
        case 'LEVELS',   levels = varargin{i+1};
        case 'L',        L = varargin{i+1};
        case 'XW_INIT',  xinit = varargin{i+1};
        case 'LAG',      lag = varargin{i+1};
        otherwise, error(['Unrecognized option: ''' varargin{i} '''']);
    end
end
if (sum(stopcriterion == [1 2 3])==0), error('Invalid stopping criterion!'); end
[M, N, B] = size(b);
nb = 3 * (levels - 1) + 1;
if nb < 1, error('sbtv:fista_l1', 'levels must be at least 2'); end
t = size(H, 1);
if size(H, 3) == 1, H = repmat(H, [1 1 B]); end
if numel(tau) == 1, tau = repmat(tau, 1, B); end
if size(H, 3) ~= B || numel(tau) ~= B
    error('sbtv:fista_l1', 'H and tau must be given once or once per image');
end
for c = {true_xw, xinit}
    if ~isempty(c{1}) && ~isequal([size(c{1}, 1) size(c{1}, 2) size(c{1}, 3)], [M nb*N B])
        error('sbtv:fista_l1', 'coefficient arrays must be M x (3*(levels-1)+1)*N x B');
    end
end
h = double(h(:));
flags = int32(0);
if ~lag, flags = int32(2); end
pXW = libpointer('doublePtr', zeros(M, nb * N, B)); pX = libpointer('doublePtr', zeros(M, N, B));
pobj = libpointer('doublePtr', zeros(maxiters, B)); ptim = libpointer('doublePtr', zeros(maxiters, B));
pmse = libpointer('doublePtr', zeros(maxiters, B));
pn = libpointer('int32Ptr', zeros(1, B, 'int32'));
if isempty(ctx), ctx = sbtv_load(0); end
rc = calllib('libsbtv', 'sbtv_fista_l1', ctx, b, int32(M), int32(N), int32(B), H, int32(t), h, int32(numel(h)), ...
             int32(levels), tau, L, int32(stopcriterion), tolerance, int32(maxiters), true_xw, xinit, pXW, pX, pobj, ptim, ...
             pmse, pn, flags);
if rc ~= 0, error('sbtv:fista_l1', '%s', calllib('libsbtv', 'sbtv_last_error', ctx)); end
XW = reshape(pXW.Value, M, nb * N, B); Wx = reshape(pX.Value, M, N, B);
n_iter = double(pn.Value);
objective = reshape(pobj.Value, maxiters, B); times = reshape(ptim.Value, maxiters, B);
if ~isempty(true_xw), mses = reshape(pmse.Value, maxiters, B); else, mses = []; end
end
