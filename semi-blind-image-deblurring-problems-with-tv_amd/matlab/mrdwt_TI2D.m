function z = mrdwt_TI2D(v, h, levels)
% z = mrdwt_TI2D(v, h, levels)
% Analysis operator of the redundant (undecimated, translation-invariant) 2-D wavelet frame on the GPU (sbtv_mrdwt_TI2D),
% under the name and with the calling convention of SALSA/mrdwt_TI2D.m; the transform is defined in include/sbtv.h.
%   v       M x N image, or M x N x B for a batch
%   h       orthonormal scaling filter of even length 2..8 (e.g. daubcqf(2)); any filter of that length is accepted
%   levels  levels - 1 decomposition steps; (length(h)-1) * 2^(levels-2) must be smaller than M and N
% z is M x (3*(levels-1)+1)*N (x B): [a_J LH1 HL1 HH1 LH2 ...], with mirdwt_TI2D as its exact transpose.
% WRITTEN WITHOUT ACCESS TO MATLAB: never executed, see INTEGRATION.md.
persistent ctx
if isempty(ctx), ctx = sbtv_load(0); end
[M, N, B] = size(v);
nb = 3 * (levels - 1) + 1;
if nb < 1, error('sbtv:wavelet', 'levels must be at least 2'); end
h = double(h(:));
pz = libpointer('doublePtr', zeros(M, nb * N, B));
rc = calllib('libsbtv', 'sbtv_mrdwt_TI2D', ctx, double(v), int32(M), int32(N), int32(B), h, int32(numel(h)), int32(levels), ...
             pz, int32(0));
if rc ~= 0, error('sbtv:wavelet', '%s', calllib('libsbtv', 'sbtv_last_error', ctx)); end
z = reshape(pz.Value, M, nb * N, B);
end
