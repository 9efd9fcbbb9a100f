"""Host side of the scribble Z objective and its region constraint (reference codes/Z_optimization.py:344-364, 385-390, 401-448, 743-746).

What the GUI's Draw, brightness +/- brush, local-TV brush and imprint tools send (GUI.py:1439-1440, :1993-1999): one label map s =
data['scribble_mask'] (1 a drawn colour, 2 / 3 brighten / darken, 4..50 local-TV regions) over the image mask lm = (image_mask > 0).
* Construction, once, in NumPy: the brightness multiplier mult = 1 + f [s = 2] - f [s = 3] smoothed by a 3 x 3 box mean over an edge-padded
  copy; the desired image D = data['desired'] with the pixels s in {2, 3} replaced by hsv2rgb(HSV(255 clip(I0[0])) with V x mult) / 255
  (not clipped); the label byte map (label_map); the region constraint's Z mask E + dilate(image_mask, ones(16, 16)) (rebuilt_z_mask).
  rgb2hsv / hsv2rgb restate skimage.color's and dilate16 OpenCV's dilate with an even 16 x 16 kernel (anchor (8, 8)); none of them is needed
  at run time.
* Per iteration, scribble_loss(x, spec) -> (L [B], C): with I = clamp(x, 0, 1), M1 = lm [0 < s < 4], T the TV region id of each pixel (0 = none),
      L_b = mean_{c,p} M1 |I_b - D| + sum_{d in (1,1), (1,0), (0,1), (-1,1)} mean_{c, p with p + d inside} [T(p) = T(p + d) > 0] |I_b(p) - I_b(p + d)|
      C   = sum_{b,c,p} (1 - lm) |I_b - I0| / constraint_norm          (F.l1_loss(I (1 - lm), I0 (1 - lm)) for the default B C H W)
  GPU: csrc/esr_scribble.hip (one read of x for all terms and any number of regions); CPU: the defining torch expression.
* region_constraint(x, image_mask, initial, norm): the constraint C alone, for the other objectives that take it (the patch-magnitude and
  periodicityPlus ones), on the same kernels with an empty label map.
"""
import numpy as np
import torch

from . import _lib
from ._image import DeviceCopies, detach_f32, ptr, to_numpy
from ._lib import check
from .act import stream_ptr

LAB_L1, LAB_CON, LAB_TV = 0x80, 0x40, 0x3f
SMOOTHING_MARGIN = 1            # the reference's 3 x 3 smoothing of the brightness multiplier
NON_EDIT_MARGINS = 24           # the region constraint's always-editable interior, E[24:-24, 24:-24]
DILATION = 16                   # dilate(image_mask, ones(16, 16))
TV_OFFSETS = ((1, 1), (1, 0), (0, 1), (-1, 1))       # (dy, dx): p pairs with p + d (Return_Translated_SubImage with shifts -d, utils/util.py:260-273)


# ------------------------------------------------------------------------------------------------ one-off host preparation
def rgb2hsv(rgb):
    """skimage.color.rgb2hsv on [..., 3]: V = max, S = delta / V (0 where delta = 0), hue from the maximal channel (blue over green over red on
    ties), (h / 6) mod 1, 0 where delta = 0.  Works on any value range (the reference passes 0..255)."""
    arr = np.asarray(rgb, dtype=np.float64)
    out = np.empty_like(arr)
    v = arr.max(-1)
    delta = arr.max(-1) - arr.min(-1)
    safe_v = np.where(v == 0, 1, v)
    safe_d = np.where(delta == 0, 1, delta)
    h = np.zeros(v.shape)
    r, g, b = arr[..., 0], arr[..., 1], arr[..., 2]
    for idx, val in ((r == v, (g - b) / safe_d), (g == v, 2. + (b - r) / safe_d), (b == v, 4. + (r - g) / safe_d)):
        h = np.where(idx, val, h)
    h = (h / 6.) % 1.
    h[delta == 0] = 0
    out[..., 0] = h
    out[..., 1] = np.where(delta == 0, 0, delta / safe_v)
    out[..., 2] = v
    return out


def hsv2rgb(hsv):
    """skimage.color.hsv2rgb on [..., 3]: sector floor(6 h) mod 6, (v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)"""
    arr = np.asarray(hsv, dtype=np.float64)
    h, s, v = arr[..., 0], arr[..., 1], arr[..., 2]
    hi = np.floor(h * 6)
    f = h * 6 - hi
    p = v * (1 - s)
    q = v * (1 - f * s)
    t = v * (1 - (1 - f) * s)
    hi = hi.astype(np.int64) % 6
    table = np.stack([np.stack(c, -1) for c in ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))])      # [6, ..., 3]
    return np.take_along_axis(table, hi[None, ..., None].repeat(3, -1), 0)[0]


def brightness_multiplier(scribble_mask, brightness_factor):
    """1 + f [s = 2] - f [s = 3], smoothed by the 3 x 3 box mean of an edge-padded copy (the reference's convolve2d(..., 'valid')), float64"""
    s = np.asarray(scribble_mask)
    m = np.ones(s.shape, dtype=np.float32)
    m += brightness_factor * (s == 2) - brightness_factor * (s == 3)
    k = SMOOTHING_MARGIN
    p = np.pad(m.astype(np.float64), ((k, k), (k, k)), mode='edge')
    H, W = s.shape
    return sum(p[dy:dy + H, dx:dx + W] for dy in range(2 * k + 1) for dx in range(2 * k + 1)) / (2 * k + 1) ** 2


def desired_image(desired, scribble_mask, initial_first, brightness_factor=None):
    """D [1, C, H, W] float32: data['desired'] with the pixels s in {2, 3} replaced by the brightened initial image 0 (initial_first [C, H, W],
    already clamped to [0, 1]); brightness_factor is read only where those labels occur"""
    s = np.asarray(scribble_mask)
    D = to_numpy(desired).astype(np.float32).reshape(1, -1, s.shape[0], s.shape[1]).copy()
    sel = (s == 2) | (s == 3)
    if sel.any():
        hsv = rgb2hsv(np.clip(255 * to_numpy(initial_first).astype(np.float32).transpose(1, 2, 0), 0, 255))
        hsv[..., 2] = hsv[..., 2] * brightness_multiplier(s, brightness_factor)
        rgb = (hsv2rgb(hsv) / 255).transpose(2, 0, 1).astype(np.float32)
        D[0][:, sel] = rgb[:, sel]
    return D


def label_map(scribble_mask, image_mask, constraint):
    """uint8 [H, W]: bit 7 where lm and 0 < s < 4 (the L1 set), bit 6 outside lm when `constraint` (the constrained set), bits 0-5 the TV region:
    the regions (ids k > 3 of s lm) numbered 1, 2, ... in increasing id order.  ValueError beyond 63 regions."""
    s = np.asarray(scribble_mask)
    lm = np.asarray(image_mask) > 0
    if s.shape != lm.shape:
        raise ValueError('scribble: scribble_mask %s and image_mask %s differ in shape' % (s.shape, lm.shape))
    lab = np.zeros(s.shape, dtype=np.uint8)
    lab[lm & (s > 0) & (s < 4)] = LAB_L1
    ids = [k for k in np.unique(s * lm) if k > 3]
    if len(ids) > LAB_TV:
        raise ValueError('scribble: %d local-TV regions, at most %d are supported' % (len(ids), LAB_TV))
    for n, k in enumerate(ids):
        lab[lm & (s == k)] = n + 1
    if constraint:
        lab[~lm] |= LAB_CON
    return lab


def dilate16(mask):
    """cv2.dilate(mask, ones(16, 16)): out(y, x) = max of mask(y - 8 .. y + 7, x - 8 .. x + 7), the border ignored (OpenCV anchors an even
    kernel at (8, 8)), so a single set pixel (y0, x0) sets rows y0 - 7 .. y0 + 8 and columns x0 - 7 .. x0 + 8"""
    m = np.asarray(mask, dtype=np.float64)
    H, W = m.shape
    lo, hi = DILATION // 2, DILATION // 2 - 1
    p = np.pad(m, ((lo, hi), (lo, hi)), constant_values=-np.inf)
    rows = np.max(np.stack([p[i:i + H] for i in range(DILATION)]), 0)
    return np.max(np.stack([rows[:, j:j + W] for j in range(DILATION)]), 0)


def rebuilt_z_mask(image_mask, block_size=1):
    """the region constraint's Z mask (reference :352-364): min(1, E + dilate16(image_mask)), E = 1 on [24:-24, 24:-24] (empty below 48 px).
    block_size 8 (JPEG mode, :355-357): Z lives on the 8 x 8 block grid [H/8, W/8]; E = 1 on [3:-3, 3:-3] blocks (the margin 24 // 8 with the
    reference's slicing) and the dilated mask is reduced to every block's maximum."""
    m = np.asarray(image_mask)
    if m.ndim != 2 or m.shape[0] % block_size or m.shape[1] % block_size:
        raise ValueError('rebuilt_z_mask: a 2-D image mask of whole %d x %d blocks, got %s' % (block_size, block_size, m.shape))
    h, w = m.shape[0] // block_size, m.shape[1] // block_size
    E = np.zeros((h, w), dtype=np.float64)
    E[NON_EDIT_MARGINS // block_size:-NON_EDIT_MARGINS // block_size, NON_EDIT_MARGINS // block_size:-NON_EDIT_MARGINS // block_size] = 1
    D = dilate16(m).reshape(h, block_size, w, block_size).max(axis=(1, 3))
    return np.minimum(1, E + D).astype(np.float32)


class ScribbleSpec(DeviceCopies):
    """labels, the desired image and the constraint's reference output, built once per edit and reused every iteration.
    desired: [1, C, H, W] (desired_image's result); initial: the initial output [1 or B, C, H, W] (clamped), needed when `constraint`."""

    def __init__(self, scribble_mask, image_mask, desired, constraint=False, initial=None):
        self.labels = label_map(scribble_mask, image_mask, constraint)
        self.H, self.W = self.labels.shape
        self.constraint = bool(constraint)
        self.desired = torch.as_tensor(to_numpy(desired), dtype=torch.float32).reshape(1, -1, self.H, self.W).contiguous()
        if self.constraint and initial is None:
            raise ValueError('scribble: the region constraint needs the initial output')
        self.initial = detach_f32(initial) if (self.constraint and initial is not None) else None
        self.regions = int((self.labels & LAB_TV).max())
        self.forget_devices()

    def _to_device(self, device):
        return torch.from_numpy(self.labels).to(device), self.desired.to(device), None if self.initial is None else self.initial.to(device)

    def masks(self, device, dtype=torch.float32):
        """(M1, T, constraint mask) as [H, W] tensors: the L1 set, the TV region ids, 1 - lm (zeros without the constraint)"""
        lab = torch.from_numpy(self.labels.astype(np.int64)).to(device)
        return ((lab & LAB_L1) != 0).to(dtype), lab & LAB_TV, ((lab & LAB_CON) != 0).to(dtype)


def _check_initial(initial, B, C, H, W):
    if initial is not None and (initial.dim() != 4 or initial.size(0) not in (1, B) or tuple(initial.shape[1:]) != (C, H, W)):
        raise ValueError('scribble: initial output %s for images %s (its batch must be 1 or %d)' % (tuple(initial.shape), (B, C, H, W), B))


def _scribble_cpu(x, spec, norm):
    """the defining expression (reference :424-446, :385-390) -> (L [B], C)"""
    I = torch.clamp(x, 0, 1)
    M1, T, cm = spec.masks(x.device, I.dtype)
    _, D, I0 = spec.on(x.device)
    H, W = spec.H, spec.W
    L = (M1 * (I - D.to(I.dtype)).abs()).mean(dim=(1, 2, 3))
    for dy, dx in TV_OFFSETS:
        y0, y1, x0, x1 = max(-dy, 0), H - max(dy, 0), max(-dx, 0), W - max(dx, 0)
        if y1 <= y0 or x1 <= x0:
            continue
        a, b = T[y0:y1, x0:x1], T[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        same = ((a == b) & (a > 0)).to(I.dtype)
        L = L + (same * (I[:, :, y0:y1, x0:x1] - I[:, :, y0 + dy:y1 + dy, x0 + dx:x1 + dx]).abs()).mean(dim=(1, 2, 3))
    if I0 is None:
        return L, torch.zeros((), dtype=I.dtype, device=I.device)
    return L, (cm * (I - I0.to(I.dtype)).abs()).sum() / norm


class _Scribble(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, spec, norm):
        xd = detach_f32(x)
        B, Cc, H, W = xd.shape
        lab, D, I0 = spec.on(xd.device)
        partial = torch.empty(B, H, 5, dtype=torch.float64, device=xd.device)
        check(_lib.lib.esr_scribble(xd.data_ptr(), B, Cc, H, W, D.data_ptr(), lab.data_ptr(), ptr(I0),
                                    0 if I0 is None else I0.size(0), partial.data_ptr(), stream_ptr()), 'esr_scribble')
        s = partial.sum(1)                                   # [B, 5]: l1, diagonal, vertical, horizontal pairs, constraint
        L = s[:, 0] / (Cc * H * W)
        for k, n in ((1, (H - 1) * (W - 1)), (2, (H - 1) * W), (3, H * (W - 1))):
            if n > 0:
                L = L + s[:, k] / (Cc * n)
        ctx.save_for_backward(xd)
        ctx.spec, ctx.norm = spec, norm
        return L.float(), (s[:, 4].sum() / norm).float()

    @staticmethod
    def backward(ctx, gL, gC):
        xd, = ctx.saved_tensors
        B, Cc, H, W = xd.shape
        lab, D, I0 = ctx.spec.on(xd.device)
        g = (torch.zeros(B, device=xd.device) if gL is None else gL.detach()).float().contiguous()
        g_con = 0.0 if (gC is None or I0 is None) else float(gC) / ctx.norm
        dx = torch.empty_like(xd)
        check(_lib.lib.esr_scribble_grad(xd.data_ptr(), B, Cc, H, W, D.data_ptr(), lab.data_ptr(), ptr(I0),
                                         0 if I0 is None else I0.size(0), g.data_ptr(), g_con, dx.data_ptr(), 0, stream_ptr()), 'esr_scribble_grad')
        return dx, None, None


def constraint_spec(image_mask, initial):
    """the ScribbleSpec of the region constraint alone (an empty label map, the constrained set 1 - (image_mask > 0)), for the objectives that
    share scribble's constraint; build it once per edit.  initial: the clamped initial output [1 or B, C, H, W]."""
    m = to_numpy(image_mask)
    return ScribbleSpec(np.zeros(m.shape, dtype=np.int64), m, np.zeros((1, initial.size(1)) + m.shape, dtype=np.float32), constraint=True,
                        initial=initial)


def region_constraint(x, image_mask, initial=None, norm=None):
    """sum_{b,c,p} (1 - lm) |clamp(x, 0, 1) - initial| / norm, lm = (image_mask > 0): F.l1_loss(I (1 - lm), initial (1 - lm)) for the default
    norm B C H W (reference :385-390); a shard of a larger batch passes B_global C H W.  image_mask: the mask [H, W], or a constraint_spec
    built from it (then `initial` is the spec's).  On the esr_scribble kernels."""
    spec = image_mask if isinstance(image_mask, ScribbleSpec) else constraint_spec(image_mask, initial)
    return scribble_loss(x, spec, constraint_norm=norm)[1]


def scribble_loss(x, spec, constraint_norm=None):
    """(L [B], C) of the module docstring for x [B, C, H, W]; C is 0 without the constraint.  constraint_norm: the divisor of the constraint's
    sum, default B C H W (F.l1_loss's mean); a shard of a larger batch passes B_global C H W."""
    B, Cc, H, W = x.shape
    if (H, W) != (spec.H, spec.W) or spec.desired.size(1) != Cc:
        raise ValueError('scribble: images %s, spec for %d channels at %d x %d' % (tuple(x.shape), spec.desired.size(1), spec.H, spec.W))
    _check_initial(spec.initial, B, Cc, H, W)
    norm = float(B * Cc * H * W if constraint_norm is None else constraint_norm)
    if not x.is_cuda:
        return _scribble_cpu(x, spec, norm)
    return _Scribble.apply(x, spec, norm)
