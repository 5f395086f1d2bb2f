function x = mirdwt_TI2D(z, h, levels)
% x = mirdwt_TI2D(z, h, levels)
% Synthesis operator of the redundant 2-D wavelet frame on the GPU (sbtv_mirdwt_TI2D), under the name and with the calling
% convention of SALSA/mirdwt_TI2D.m: the exact transpose of mrdwt_TI2D, and its inverse for an orthonormal h.
%   z       M x (3*(levels-1)+1)*N coefficients (x B for a batch), in the layout mrdwt_TI2D returns
%   h, levels  as for mrdwt_TI2D
% WRITTEN WITHOUT ACCESS TO MATLAB: never executed, see INTEGRATION.md.
persistent ctx
if isempty(ctx), ctx = sbtv_load(0); end
[M, NN, B] = size(z);
nb = 3 * (levels - 1) + 1;
if nb < 1 || rem(NN, nb) ~= 0, error('sbtv:wavelet', 'z must have (3*(levels-1)+1)*N columns'); end
N = NN / nb;
h = double(h(:));
px = libpointer('doublePtr', zeros(M, N, B));
rc = calllib('libsbtv', 'sbtv_mirdwt_TI2D', ctx, double(z), int32(M), int32(N), int32(B), h, int32(numel(h)), int32(levels), ...
             px, int32(0));
if rc ~= 0, error('sbtv:wavelet', '%s', calllib('libsbtv', 'sbtv_last_error', ctx)); end
x = reshape(px.Value, M, N, B);
end
