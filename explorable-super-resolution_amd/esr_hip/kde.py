"""Host side of the patch-histogram and dictionary Z objectives (reference codes/Z_optimization.py:24-272).

* column_lse / row_lse: the pairwise KDE kernels of csrc/esr_kde.hip as differentiable torch functions (w.r.t. the points, never the bins):
      column mode  lse[b, j] = log sum_{i in image b} k_ij     (the KDE histogram of each image, before normalisation)
      row mode     lse[i]    = log sum_j k_ij                  (the dictionary's soft minimum over the bins)
  with k_ij = exp(-s_ij / T), s_ij = (1/D) sum_d (w(x_id - b_jd) + 1e-7)^2, w the distance wrapped with period `period`.  Log sums are folded
  over the kernels' slabs in float64.
* dedup_keep: the de-duplication of the desired patches (Desired_Im_2_Bins, :102-125) on the GPU.
* patch_extraction_indexes: a NumPy restatement of ReturnPatchExtractionMat (:231-272) returning index arrays instead of a sparse matrix.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import EsrError, check
from .act import require_gpu, stream_ptr

TILE = 256              # outer points per workgroup (KDE_THREADS)
CHUNK = 128             # inner points per LDS chunk (KDE_CH)
TARGET_BLOCKS = 2048    # enough workgroups for 256 CUs: the slab counts below aim at this many


def _dev_i32(values, device):
    return torch.tensor(values, dtype=torch.int32).to(device, non_blocking=False)


def _round_up(n, m):
    return (n + m - 1) // m * m


def _check_points(X, bins):
    require_gpu(X, 'KDE points')
    require_gpu(bins, 'KDE bins')
    if X.dim() != 2 or bins.dim() != 2 or X.size(1) != bins.size(1):
        raise EsrError('KDE: points [R, D] and bins [M, D] expected, got %s and %s' % (tuple(X.shape), tuple(bins.shape)))
    D = X.size(1)
    if not _lib.lib.esr_kde_dim_supported(D):
        raise EsrError('KDE: point dimension %d is not supported (1 or a square patch of side 2..8)' % D)
    if bins.size(0) < 1 or bins.size(0) >= 2 ** 31 or X.size(0) >= 2 ** 31:
        raise EsrError('KDE: bad sizes %s, %s' % (tuple(X.shape), tuple(bins.shape)))
    return D


def _row_tiles(counts):
    """(image, row0, row1) tiles of at most TILE rows, never straddling two images (rows are the images' points concatenated)."""
    tiles, r = [], 0
    for b, n in enumerate(counts):
        for t in range(r, r + n, TILE):
            tiles.append((b, t, min(t + TILE, r + n)))
        r += n
    return tiles


def _bin_slabs(M, other_blocks):
    n = max(1, min(math.ceil(TARGET_BLOCKS / max(1, other_blocks)), math.ceil(M / CHUNK)))
    per = _round_up(math.ceil(M / n), CHUNK)
    return per, math.ceil(M / per)


def _fold(pmax, psum, groups):
    """log-sum-exp of the slabs' (max, scaled sum) partials over each group of slabs, in float64 -> [len(groups), n]"""
    l = pmax.double() + torch.log(psum)
    return torch.stack([torch.logsumexp(l[a:b], 0) for a, b in groups])


def _backward(X, bins, counts, T, period, g_row=None, l_row=None, g_bin=None, l_bin=None):
    R, D = X.shape
    M = bins.size(0)
    tiles = _row_tiles(counts)
    per, n_slabs = _bin_slabs(M, len(tiles))
    tiles_d = _dev_i32([v for t in tiles for v in t], X.device)
    part = torch.empty(n_slabs, R, D, dtype=torch.float32, device=X.device)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    check(_lib.lib.esr_kde_bwd(X.data_ptr(), R, tiles_d.data_ptr(), len(tiles), bins.data_ptr(), M, per, n_slabs, D, float(period), 1.0 / (D * T),
                               ptr(g_row), ptr(l_row), ptr(g_bin), ptr(l_bin), part.data_ptr(), stream_ptr()), 'esr_kde_bwd')
    return part.sum(0) if n_slabs > 1 else part[0]


class _KdeColumns(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, bins, counts, T, period):
        X = X.detach().float().contiguous()
        bins = bins.detach().float().contiguous()
        D = _check_points(X, bins)
        R, M = X.size(0), bins.size(0)
        if sum(counts) != R or min(counts) < 1:
            raise EsrError('KDE: per-image point counts %s do not cover %d points' % (counts, R))
        bin_blocks = math.ceil(M / TILE)
        want = max(1, math.ceil(TARGET_BLOCKS / (bin_blocks * len(counts))))          # slabs per image
        ranges, groups, r = [], [], 0
        for n in counts:
            per = _round_up(math.ceil(n / min(want, math.ceil(n / CHUNK))), CHUNK)
            s0 = len(ranges)
            ranges += [(a, min(a + per, r + n)) for a in range(r, r + n, per)]
            groups.append((s0, len(ranges)))
            r += n
        ranges_d = _dev_i32([v for p in ranges for v in p], X.device)
        pmax = torch.empty(len(ranges), M, dtype=torch.float32, device=X.device)
        psum = torch.empty(len(ranges), M, dtype=torch.float64, device=X.device)
        check(_lib.lib.esr_kde_fwd(bins.data_ptr(), M, X.data_ptr(), ranges_d.data_ptr(), len(ranges), D, float(period), 1.0 / (D * T), pmax.data_ptr(),
                                   psum.data_ptr(), stream_ptr()), 'esr_kde_fwd')
        lse = _fold(pmax, psum, groups)                                                 # [B, M] float64
        ctx.save_for_backward(X, bins, lse)
        ctx.args = (counts, T, period)
        return lse

    @staticmethod
    def backward(ctx, g):
        X, bins, lse = ctx.saved_tensors
        counts, T, period = ctx.args
        dX = _backward(X, bins, counts, T, period, g_bin=g.detach().float().contiguous(), l_bin=lse.float().contiguous())
        return dX, None, None, None, None


class _KdeRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, bins, T, period):
        X = X.detach().float().contiguous()
        bins = bins.detach().float().contiguous()
        D = _check_points(X, bins)
        R, M = X.size(0), bins.size(0)
        per, n_slabs = _bin_slabs(M, math.ceil(R / TILE))
        ranges_d = _dev_i32([v for s in range(n_slabs) for v in (s * per, min(M, (s + 1) * per))], X.device)
        pmax = torch.empty(n_slabs, R, dtype=torch.float32, device=X.device)
        psum = torch.empty(n_slabs, R, dtype=torch.float64, device=X.device)
        check(_lib.lib.esr_kde_fwd(X.data_ptr(), R, bins.data_ptr(), ranges_d.data_ptr(), n_slabs, D, float(period), 1.0 / (D * T), pmax.data_ptr(),
                                   psum.data_ptr(), stream_ptr()), 'esr_kde_fwd')
        lse = _fold(pmax, psum, [(0, n_slabs)])[0]                                       # [R] float64
        ctx.save_for_backward(X, bins, lse)
        ctx.args = (T, period)
        return lse

    @staticmethod
    def backward(ctx, g):
        X, bins, lse = ctx.saved_tensors
        T, period = ctx.args
        dX = _backward(X, bins, (X.size(0),), T, period, g_row=g.detach().float().contiguous(), l_row=lse.float().contiguous())
        return dX, None, None, None


def column_lse(X, counts, bins, temperature, period):
    """X: [R, D] points of len(counts) images (counts[b] consecutive rows each); bins: [M, D].  Returns [B, M] float64,
    log sum_{i in image b} exp(-s_ij / temperature); differentiable w.r.t. X."""
    return _KdeColumns.apply(X, bins, tuple(int(c) for c in counts), float(temperature), float(period))


def row_lse(X, bins, temperature, period):
    """X: [R, D] points, bins: [M, D].  Returns [R] float64, log sum_j exp(-s_ij / temperature); differentiable w.r.t. X."""
    return _KdeRows.apply(X, bins, float(temperature), float(period))


def dedup_keep(bins, half_width):
    """[M] bool: False where a LATER bin lies within half_width of this one in every dimension (reference Desired_Im_2_Bins, :102-125, in its
    single-pass form).  The reference retries in sub-images when its [D, M, M] mask does not fit in memory, and then de-duplicates only within
    each sub-image; that fallback is not reproduced — this is always the whole-set result."""
    b = bins.detach().float().contiguous()
    require_gpu(b, 'KDE bins')
    M, D = b.shape
    keep = torch.empty(M, dtype=torch.int32, device=b.device)
    check(_lib.lib.esr_kde_dedup(b.data_ptr(), M, D, float(half_width), keep.data_ptr(), stream_ptr()), 'esr_kde_dedup')
    return keep.bool()


# ------------------------------------------------------------------------------------------------ patch selection (NumPy only)
def _box_sum(a, k):
    """sums of every k x k window of a (top-left anchored): [H - k + 1, W - k + 1]"""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), dtype=np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(a.astype(np.int64), 0), 1)
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def binary_opening_square(mask, k):
    """scipy.ndimage.binary_opening(mask, ones([k, k])) (zero border): a pixel stays iff some k x k square inside the image and inside the mask
    covers it.  Erosion and dilation by cumulative sums."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    out = np.zeros((H, W), dtype=bool)
    if H < k or W < k:
        return out
    fits = (_box_sum(m, k) == k * k).astype(np.int64)                     # erosion, indexed by the square's top-left corner
    pad = np.zeros((H + k - 1, W + k - 1), dtype=np.int64)
    pad[k - 1:k - 1 + fits.shape[0], k - 1:k - 1 + fits.shape[1]] = fits
    return _box_sum(pad, k) > 0                                           # dilation: any square whose top-left lies in (y-k, y] x (x-k, x]


def patch_extraction_indexes(mask, patch_size, patches_overlap=1.0):
    """ReturnPatchExtractionMat (reference :231-272) as an index array: [P, patch_size**2] int64 flat pixel indexes, row p = the p-th selected
    patch, its pixels in row-major order (the reference's sparse matrix has row d * P + p pick pixel [p, d]).
      1. the mask is opened with a patch_size square (binary_opening);
      2. every patch_size x patch_size window inside the opened mask, in extract_patches_2d order (top-left corner row-major);
      3. for patches_overlap < 1, the greedy scan in that order: a patch is dropped when more than patches_overlap of its pixels (any, for
         overlap 0) are already covered by an earlier kept patch.  The coverage flags are indexed as the reference indexes them — pixel p at
         slot p - min - 1 of an array of max - min slots — so the lowest and the highest covered pixels share a slot."""
    k = int(patch_size)
    opened = binary_opening_square(mask, k)
    H, W = opened.shape
    if H < k or W < k:
        return np.zeros((0, k * k), dtype=np.int64)
    y0, x0 = np.nonzero(_box_sum(opened, k) == k * k)                        # row-major: extract_patches_2d's order
    dy, dx = np.divmod(np.arange(k * k), k)
    idx = (y0[:, None] + dy[None, :]) * W + (x0[:, None] + dx[None, :])
    if patches_overlap < 1 and idx.shape[0] > 0:
        lo, hi = int(idx.min()), int(idx.max())
        taken = np.zeros(hi - lo, dtype=bool)
        slots = idx - lo - 1
        valid = np.ones(idx.shape[0], dtype=bool)
        for p in range(idx.shape[0]):
            s = slots[p]
            t = taken[s]
            if (patches_overlap == 0 and t.any()) or np.mean(t) > patches_overlap:
                valid[p] = False
                continue
            taken[s] = True
        idx = idx[valid]
    return idx.astype(np.int64)
