"""Host side of the local-STD and periodicity Z objectives (reference codes/Z_optimization.py:391-398, 459-509, 616-627, 799-815).

* patch_corners: the patch set of ReturnPatchExtractionMat(image_mask, 7, patches_overlap=1) — every 7 x 7 window inside the mask opened with a
  7 x 7 square — as a uint8 map of the windows' top-left corners, [H-6, W-6] (no [P, 49] index array).
* patch_std(x, corners) -> S [P, B]: the unbiased STD of every selected window of v_b = mean_c clamp(x_b, 0, 1), patches in row-major order of
  their corners (the reference's local Masked_STD).  GPU: csrc/esr_local.hip; CPU: the defining torch expression (unfold).
  Intended divergence: where a window is flat (S = 0) the reference's gradient is 0/0 = NaN (torch.std's backward) and poisons Adam; here the
  window contributes a zero gradient, on both paths.
* ShiftPair / shift_l1(x, mask, pairs) -> [B]: the periodicity term sum_points mean_{c,i,j} M |GS+(I) - GS-(I)| with I = clamp(x, 0, 1),
  M = GS+(mask) GS-(mask).  Non-integer points ('nonInt'): GS are grid_sample on the reference's linspace coordinate lines (bilinear, zero
  padding, align_corners=False), its quirk kept: the x line is sized with the image height and the y line with its width.  Integer points:
  the crops of Return_Translated_SubImage (utils/util.py:260-274).  GPU: the separable sampler and its gather-form adjoint of
  csrc/esr_local.hip; CPU: grid_sample / the crops.
"""
import numpy as np
import torch

from . import _lib
from ._image import PATCH, DeviceCopies, detach_f32, mask_on, to_numpy
from ._lib import check
from .act import stream_ptr
from .kde import _box_sum, binary_opening_square


def patch_corners(mask, H=None, W=None):
    """uint8 [H-6, W-6]: 1 where the 7 x 7 window with this top-left corner lies inside binary_opening(mask, ones(7, 7)).  mask None: the whole
    H x W image.  ValueError when no window fits."""
    if mask is None:
        m = np.ones((H, W), dtype=bool)
    else:
        m = to_numpy(mask) != 0
    if m.shape[0] < PATCH or m.shape[1] < PATCH:
        raise ValueError('local STD: a %d x %d image holds no %d x %d patch' % (m.shape[0], m.shape[1], PATCH, PATCH))
    c = (_box_sum(binary_opening_square(m, PATCH), PATCH) == PATCH * PATCH).astype(np.uint8)
    if not c.any():
        raise ValueError('local STD: the image mask holds no %d x %d patch' % (PATCH, PATCH))
    return c


def corner_patch_indexes(corners, W):
    """[P, 49] flat pixel indexes of the windows of a corner map (row p: patch p's pixels, row-major) — for tests and small images"""
    y0, x0 = np.nonzero(corners)
    dy, dx = np.divmod(np.arange(PATCH * PATCH), PATCH)
    return ((y0[:, None] + dy) * W + x0[:, None] + dx).astype(np.int64)


def _patch_std_cpu(x, flat_idx):
    """the defining expression: torch.std over each selected window of mean_c clamp(x, 0, 1), shifted by the window's first value so that a
    flat window has S = 0 exactly, and a zero gradient there -> [P, B]"""
    v = torch.clamp(x, 0, 1).mean(1)
    B = v.size(0)
    p = v.unfold(1, PATCH, 1).unfold(2, PATCH, 1).reshape(B, -1, PATCH * PATCH)[:, flat_idx]
    d = p - p[..., :1]
    d = d - d.mean(-1, keepdim=True)
    var = (d * d).sum(-1) / (PATCH * PATCH - 1)
    S = torch.where(var > 0, var.clamp_min(1e-30).sqrt(), torch.zeros_like(var))
    return S.t()


class _PatchStd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, corners, flat_idx):
        xd = detach_f32(x)
        B, Cc, H, W = xd.shape
        S = torch.empty(B, H - PATCH + 1, W - PATCH + 1, dtype=torch.float32, device=xd.device)
        M = torch.empty_like(S)
        check(_lib.lib.esr_patch_std(xd.data_ptr(), B, Cc, H, W, corners.data_ptr(), S.data_ptr(), M.data_ptr(), stream_ptr()), 'esr_patch_std')
        ctx.save_for_backward(xd, corners, flat_idx, S, M)
        return S.view(B, -1)[:, flat_idx].t()

    @staticmethod
    def backward(ctx, g):
        xd, corners, flat_idx, S, M = ctx.saved_tensors
        B, Cc, H, W = xd.shape
        dS = torch.zeros(B, S[0].numel(), dtype=torch.float32, device=xd.device)
        dS[:, flat_idx] = g.detach().t().float()
        dx = torch.empty_like(xd)
        check(_lib.lib.esr_patch_std_grad(xd.data_ptr(), B, Cc, H, W, corners.data_ptr(), S.data_ptr(), M.data_ptr(), dS.data_ptr(), dx.data_ptr(), 0,
                                          stream_ptr()), 'esr_patch_std_grad')
        return dx, None, None


class PatchSet(DeviceCopies):
    """a corner map with its device copies, built once per (mask, image size) and reused every iteration"""

    def __init__(self, mask, H, W, corners=None):
        self.corners = patch_corners(mask, H, W) if corners is None else np.asarray(corners, dtype=np.uint8)
        self.H, self.W = self.corners.shape[0] + PATCH - 1, self.corners.shape[1] + PATCH - 1
        self.flat_idx = torch.from_numpy(np.flatnonzero(self.corners).astype(np.int64))
        self.forget_devices()

    @property
    def P(self):
        return int(self.flat_idx.numel())

    def _to_device(self, device):
        return torch.from_numpy(self.corners).to(device), self.flat_idx.to(device)


def patch_std(x, patches):
    """S [P, B]: the unbiased STD of each selected 7 x 7 window of mean_c clamp(x_b, 0, 1) (x [B, C, H, W]; patches a PatchSet or a corner map)"""
    if not isinstance(patches, PatchSet):
        patches = PatchSet(None, None, None, corners=patches)
    if (x.size(2), x.size(3)) != (patches.H, patches.W):
        raise ValueError('patch_std: image %s, patch set for %d x %d' % (tuple(x.shape[2:]), patches.H, patches.W))
    corners, flat_idx = patches.on(x.device)
    if not x.is_cuda:
        return _patch_std_cpu(x, flat_idx)
    return _PatchStd.apply(x, corners, flat_idx)


# ------------------------------------------------------------------------------------------------ periodicity
def _indexing_helper(index, negative=False):       # utils/util.py:260-264
    if negative:
        return index if index < 0 else None
    return index if index > 0 else None


def periodicity_lines(point, H, W):
    """The reference's coordinate lines for a non-integer period point (Z_optimization.py:470-504): [(x_line, y_line) for the signs +, -],
    float32 normalised coordinates; x_line has the length and scale of the image HEIGHT and y_line of its WIDTH, as the reference builds them."""
    image_size = [H, W]
    out = []
    for minus in (0, 1):
        cur = 1 * np.array(point, dtype=np.float64)
        if minus:
            cur = cur * -1
        y_range = [_indexing_helper(cur[0]), _indexing_helper(cur[0], negative=True)]
        x_range = [_indexing_helper(cur[1]), _indexing_helper(cur[1], negative=True)]
        ranges = []
        for axis, r in enumerate([x_range, y_range]):
            r = [r[0] if r[0] is not None else 0, image_size[axis] + r[1] if r[1] is not None else image_size[axis]]
            n = image_size[axis] - np.ceil(np.abs(np.array([0, image_size[axis]]) - r)).astype(np.int16).max()
            ranges.append((np.linspace(start=r[0], stop=r[1], num=n) / image_size[axis] * 2 - 1).astype(np.float32))
        out.append((ranges[0], ranges[1]))
    return out


def _ranges(base, n_src):
    """[n_src, 2] int32: per source index q, a half-open range of output indexes whose taps (base, base + 1) may include q (one extra on each
    side: the kernel checks every tap)"""
    q = np.arange(n_src)
    lo = np.searchsorted(base, q - 1, 'left') - 1
    hi = np.searchsorted(base, q, 'right') + 1
    return np.stack([np.clip(lo, 0, len(base)), np.clip(hi, 0, len(base))], 1).astype(np.int32)


class ShiftPair(DeviceCopies):
    """The two samplers of one period point: sign + and sign -, each separable (taps per output column and per output row)."""

    def __init__(self, point, H, W, interpolated):
        self.point, self.H, self.W, self.interpolated = tuple(float(p) for p in point), H, W, bool(interpolated)
        bx, fx, by, fy = [], [], [], []
        if interpolated:
            self.lines = periodicity_lines(point, H, W)
            for xl, yl in self.lines:
                ix = ((xl.astype(np.float64) + 1) * W - 1) / 2          # grid_sample's unnormalisation (align_corners=False), exact in float64
                iy = ((yl.astype(np.float64) + 1) * H - 1) / 2
                bx.append(np.floor(ix)); fx.append(ix - np.floor(ix))
                by.append(np.floor(iy)); fy.append(iy - np.floor(iy))
        else:
            if any(float(p) != int(round(float(p))) for p in point):
                raise ValueError("periodicity: the integer form takes integer period points, got %s (the 'nonInt' objectives interpolate)" % (point,))
            dy, dx = int(round(float(point[0]))), int(round(float(point[1])))
            if abs(dy) >= H or abs(dx) >= W:
                raise ValueError('periodicity: the point %s leaves nothing of a %d x %d image' % (point, H, W))
            self.crops = []
            for s in (1, -1):
                y0, x0 = max(s * dy, 0), max(s * dx, 0)
                self.crops.append((y0, H + min(s * dy, 0), x0, W + min(s * dx, 0)))
                by.append(y0 + np.arange(H - abs(dy))); fy.append(np.zeros(H - abs(dy)))
                bx.append(x0 + np.arange(W - abs(dx))); fx.append(np.zeros(W - abs(dx)))
        self.nx, self.ny = len(bx[0]), len(by[0])
        if self.nx < 1 or self.ny < 1:
            raise ValueError('periodicity: the point %s leaves no output grid on a %d x %d image' % (point, H, W))
        self.base_x = np.stack(bx).astype(np.int32)
        self.frac_x = np.stack(fx).astype(np.float32)
        self.base_y = np.stack(by).astype(np.int32)
        self.frac_y = np.stack(fy).astype(np.float32)
        self.ranges_x = np.stack([_ranges(b, W) for b in self.base_x])
        self.ranges_y = np.stack([_ranges(b, H) for b in self.base_y])
        self.forget_devices()

    def _to_device(self, device):
        return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in
                     (self.base_x, self.frac_x, self.base_y, self.frac_y, self.ranges_x, self.ranges_y))

    def grids(self, device, dtype=torch.float32):
        """the reference's [1, ny, nx, 2] grid_sample grids for the signs +, - (non-integer form)"""
        return [torch.from_numpy(np.stack(np.meshgrid(xl, yl), -1)).view(1, len(yl), len(xl), 2).to(device=device, dtype=dtype) for xl, yl in self.lines]


def _shift_l1_cpu(x, mask, pairs):
    """the defining expression (Z_optimization.py:799-815, utils/util.py:271-277) -> [B]"""
    image = torch.clamp(x, 0, 1)
    m = mask.to(image.dtype).view(1, 1, mask.size(-2), mask.size(-1))
    loss = torch.zeros(image.size(0), dtype=image.dtype, device=image.device)
    for pr in pairs:
        if pr.interpolated:
            gp, gm = pr.grids(image.device, image.dtype)
            gs = lambda im, g: torch.nn.functional.grid_sample(im, g.repeat([im.size(0), 1, 1, 1]), align_corners=False)  # noqa: E731
            cur_mask = gs(m, gp) * gs(m, gm)
            loss = loss + (cur_mask * (gs(image, gp) - gs(image, gm)).abs()).mean(dim=(1, 2, 3))
        else:
            (a0, a1, b0, b1), (c0, c1, d0, d1) = pr.crops
            cur_mask = m[:, :, a0:a1, b0:b1] * m[:, :, c0:c1, d0:d1]
            loss = loss + (cur_mask * (image[:, :, a0:a1, b0:b1] - image[:, :, c0:c1, d0:d1]).abs()).mean(dim=(1, 2, 3))
    return loss


class _ShiftL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, pairs):
        xd = detach_f32(x)
        B, Cc, H, W = xd.shape
        md = mask_on(mask, xd.device, H, W)
        loss = torch.zeros(B, dtype=torch.float64, device=xd.device)
        for pr in pairs:
            bx, fx, by, fy, _, _ = pr.on(xd.device)
            partial = torch.empty(B, pr.ny, dtype=torch.float64, device=xd.device)
            check(_lib.lib.esr_shift_l1(xd.data_ptr(), B, Cc, H, W, md.data_ptr(), pr.nx, pr.ny, bx.data_ptr(), fx.data_ptr(), by.data_ptr(), fy.data_ptr(),
                                        partial.data_ptr(), stream_ptr()), 'esr_shift_l1')
            loss = loss + partial.sum(1) / (Cc * pr.ny * pr.nx)
        ctx.save_for_backward(xd, md)
        ctx.pairs = pairs
        return loss.float()

    @staticmethod
    def backward(ctx, g):
        xd, md = ctx.saved_tensors
        B, Cc, H, W = xd.shape
        dx = torch.zeros_like(xd)
        g = g.detach().double()
        for k, pr in enumerate(ctx.pairs):
            bx, fx, by, fy, rx, ry = pr.on(xd.device)
            gs = (g / (Cc * pr.ny * pr.nx)).float().contiguous()
            work = torch.empty(B, Cc, pr.ny, pr.nx, dtype=torch.float32, device=xd.device)
            check(_lib.lib.esr_shift_l1_grad(xd.data_ptr(), B, Cc, H, W, md.data_ptr(), pr.nx, pr.ny, bx.data_ptr(), fx.data_ptr(), by.data_ptr(), fy.data_ptr(),
                                             rx.data_ptr(), ry.data_ptr(), gs.data_ptr(), work.data_ptr(), dx.data_ptr(), 1 if k else 0, stream_ptr()),
                  'esr_shift_l1_grad')
        return dx, None, None


def shift_l1(x, mask, pairs):
    """sum over the ShiftPairs of mean_{c,i,j} M |GS+(I) - GS-(I)| per image, I = clamp(x, 0, 1), M = GS+(mask) GS-(mask) -> [B]
    (x [B, C, H, W]; mask [H, W], None: ones)"""
    pairs = tuple(pairs)
    if mask is None:
        mask = torch.ones(x.size(2), x.size(3), dtype=torch.float32, device=x.device)
    for pr in pairs:
        if (pr.H, pr.W) != (x.size(2), x.size(3)):
            raise ValueError('shift_l1: image %s, sampler for %d x %d' % (tuple(x.shape[2:]), pr.H, pr.W))
    if not x.is_cuda:
        return _shift_l1_cpu(x, mask, pairs)
    if not pairs:
        return torch.zeros(x.size(0), dtype=torch.float32, device=x.device)
    return _ShiftL1.apply(x, mask, pairs)
