#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY (CPU, build container): writes tests/golden/scribble.npz by running the REFERENCE's own Z_optimizer
(codes/Z_optimization.py:331-448, 647-797) with objective 'scribble', imported read-only through oracle/_refshim.  Run:
    python tools/gen_scribble_golden.py

skimage.color and cv2 are not installed here (oracle/_refshim stubs them), so Z_optimization.rgb2hsv, hsv2rgb and dilate are pinned to the
NumPy restatements below, written here from skimage's and OpenCV's documented formulas and not imported from the product, so that a slip in
either copy shows as a mismatch.  Like oracle/cv2_cubic.py they are restatements, not the libraries themselves.  The reference was written for a
torch whose comparisons returned uint8: its `1 - ((s == 2) + (s == 3))` (:418) is evaluated with the bool mask as uint8 while it runs.

(a) function level, on seeded images of 40 x 52 (non-square), B = 2, x spanning [-0.1, 1.1], an irregular image mask, a label map with every
    kind (1, 2, 3, TV regions touching the border and each other, labels outside the mask), brightness factor 0.3, the region constraint on:
  a/x, a/mask, a/scribble, a/desired_in     the inputs (a/desired_in: data['desired'])
  a/x_init                                  the image the optimizer is constructed on (its initial output: brightness edit, constraint)
  a/D                                       the reference's desired image after the brightness edit
  a/Z_mask                                  its rebuilt Z mask (min(1, E + dilate(mask, ones(16, 16))); E is empty below 48 px)
  a/loss [2], a/constraint                  Scribble_Loss per image and constraining_loss, on the stand-in model's image
  a/grad_loss, a/grad_constraint            d sum(loss) / d x and d constraint / d x
(b) Z_optimizer('scribble', ...).optimize() on the F7 model (oracle/gen_golden.py::gen_F7: RRDB-1, latent 3, LR 24 x 28 -> HR 96 x 112, B = 3,
    4 iterations, Adam lr 0.1, the seeded LR and initial Z of tools/gen_local_z_golden.py), the irregular image mask and rectangular Z mask of
    that generator, with non_local_Z_optimization off ('local') and on ('nonlocal').  The model's output (the initial output the brightness
    edit and the constraint start from) is that of the seeded Z of seed 921; the search starts from a second seeded Z (seed 922), so that the
    constraint's |out - initial| has no ties at 0, whose gradient sign would be rounding noise in either implementation:
  b/mask/{image,Z}, b/scribble, b/desired_in, b/<mode>/loss, b/<mode>/Z_mask, b/<mode>/final_Z_sub (Z[:, :, ::8, ::8])
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import _refshim  # noqa: E402
from oracle.weights import fill_formula_weights, seeded_uniform  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
H, W, B = 40, 52, 2
BRIGHTNESS = 0.3


# ---- restatements of the three library functions the reference calls
def rgb2hsv(rgb):
    """skimage.color.rgb2hsv (channel last), as its source reads"""
    arr = np.asarray(rgb, dtype=np.float64)
    out = np.empty_like(arr)
    out_v = arr.max(-1)
    delta = np.ptp(arr, -1)
    with np.errstate(invalid='ignore', divide='ignore'):
        out_s = delta / out_v
        out_s[delta == 0.] = 0.
        idx = arr[..., 0] == out_v
        out[idx, 0] = (arr[idx, 1] - arr[idx, 2]) / delta[idx]
        idx = arr[..., 1] == out_v
        out[idx, 0] = 2. + (arr[idx, 2] - arr[idx, 0]) / delta[idx]
        idx = arr[..., 2] == out_v
        out[idx, 0] = 4. + (arr[idx, 0] - arr[idx, 1]) / delta[idx]
        out_h = (out[..., 0] / 6.) % 1.
        out_h[delta == 0.] = 0.
    out[..., 0] = out_h
    out[..., 1] = out_s
    out[..., 2] = out_v
    out[np.isnan(out)] = 0
    return out


def hsv2rgb(hsv):
    """skimage.color.hsv2rgb (channel last), as its source reads"""
    arr = np.asarray(hsv, dtype=np.float64)
    hi = np.floor(arr[..., 0] * 6)
    f = arr[..., 0] * 6 - hi
    p = arr[..., 2] * (1 - arr[..., 1])
    q = arr[..., 2] * (1 - f * arr[..., 1])
    t = arr[..., 2] * (1 - (1 - f) * arr[..., 1])
    v = arr[..., 2]
    hi = np.stack([hi, hi, hi], axis=-1).astype(np.uint8) % 6
    return np.choose(hi, np.stack([np.stack((v, t, p), axis=-1), np.stack((q, v, p), axis=-1), np.stack((p, v, t), axis=-1),
                                   np.stack((p, q, v), axis=-1), np.stack((t, p, v), axis=-1), np.stack((v, p, q), axis=-1)]))


def dilate(src, kernel):
    """cv2.dilate with default anchor and border: out(y, x) = max over the kernel's nonzero (i, j) of src(y + i - ky // 2, x + j - kx // 2),
    taps outside the image ignored"""
    src = np.asarray(src)
    ky, kx = np.asarray(kernel).shape
    out = np.full(src.shape, -np.inf)
    Hs, Ws = src.shape
    for i, j in zip(*np.nonzero(kernel)):
        dy, dx = i - ky // 2, j - kx // 2
        ys, xs = slice(max(0, -dy), min(Hs, Hs - dy)), slice(max(0, -dx), min(Ws, Ws - dx))
        yd, xd = slice(max(0, dy), min(Hs, Hs + dy)), slice(max(0, dx), min(Ws, Ws + dx))
        out[ys, xs] = np.maximum(out[ys, xs], src[yd, xd])
    return out.astype(src.dtype)


@contextlib.contextmanager
def uint8_comparisons():
    """`1 - bool_tensor` as the reference's torch evaluated it (comparisons returned uint8 there)"""
    orig = torch.Tensor.__rsub__

    def rsub(self, other):
        return orig(self.to(torch.uint8) if self.dtype == torch.bool else self, other)
    torch.Tensor.__rsub__ = rsub
    try:
        yield
    finally:
        torch.Tensor.__rsub__ = orig


# ---- inputs
def mask_a():
    m = (seeded_uniform((H, W), 1500).numpy() > 0.2).astype(np.float32)
    m[:14] = 0
    m[:, 44:] = 0
    m[20:34, 6:36] = 1
    return m


def scribble_a():
    s = np.zeros((H, W), dtype=np.int64)
    s[16:24, 2:14] = 1                     # a drawn colour
    s[24:32, 2:12] = 2                     # brighten
    s[30:38, 14:24] = 3                    # darken
    s[20:40, 26:34] = 4                    # TV region touching the bottom border ...
    s[20:40, 34:40] = 5                    # ... and region 4
    s[32:40, 0:2] = 7                      # a region on the left border
    s[2:10, 2:10] = 1                      # labels outside the image mask (ignored)
    s[4:8, 46:50] = 6
    return s


def scribble_b(h, w):
    s = np.zeros((h, w), dtype=np.int64)
    s[30:44, 30:52] = 1
    s[44:60, 30:50] = 2
    s[60:76, 30:48] = 3
    s[30:70, 56:72] = 4
    s[30:70, 72:84] = 9
    s[76:88, 60:90] = 12
    return s


class _StandIn:
    """what Z_optimizer's constructor and its losses read of a model"""

    def __init__(self, x):
        self.fake_H = x
        self.num_latent_channels = 3
        self.netG = torch.nn.Linear(1, 1)
        self.cur_Z = torch.zeros(1, 3, H, W)          # the GUI's model holds a latent: the reference starts a masked search from it

    def Output_Batch(self, within_0_1=False):
        return torch.clamp(self.fake_H, 0, 1) if within_0_1 else self.fake_H

    def GetLatent(self):
        return self.cur_Z


def part_a(Z_optimizer, out):
    x0 = seeded_uniform((B, 3, H, W), 1501, -0.1, 1.1)
    x_init = seeded_uniform((B, 3, H, W), 1504, -0.1, 1.1)
    out['a/x_init'] = x_init.numpy()
    desired = seeded_uniform((1, 3, H, W), 1502)
    mask, s = mask_a(), scribble_a()
    out['a/x'], out['a/mask'], out['a/scribble'], out['a/desired_in'] = x0.numpy(), mask, s, desired.numpy()
    data = {'desired': desired.clone(), 'scribble_mask': s.copy(), 'brightness_factor': BRIGHTNESS}
    with contextlib.redirect_stdout(io.StringIO()), uint8_comparisons():
        zo = Z_optimizer(objective='scribble', Z_size=[H, W], model=_StandIn(x_init.clone()), Z_range=1, max_iters=1, data=data, initial_LR=0.1,
                         batch_size=B, image_mask=mask.copy(), Z_mask=np.ones((H, W), np.float32), non_local_Z_optimization=True)
    assert zo.non_local_Z_optimization
    out['a/D'] = zo.desired_im.detach().numpy().astype(np.float32)
    out['a/Z_mask'] = zo.Z_mask.numpy().astype(np.float32)
    x = x0.clone().requires_grad_(True)
    I = torch.clamp(x, 0, 1)
    loss = zo.loss(I, zo.desired_im)
    loss.sum().backward()
    out['a/loss'], out['a/grad_loss'] = loss.detach().double().numpy().reshape(-1), x.grad.double().numpy()
    x = x0.clone().requires_grad_(True)
    con = zo.constraining_loss(torch.clamp(x, 0, 1))
    con.backward()
    out['a/constraint'], out['a/grad_constraint'] = np.float64(con.item()), x.grad.double().numpy()
    print('a', out['a/loss'], out['a/constraint'], float(out['a/Z_mask'].mean()))


def part_b(Z_optimizer, out):
    from oracle.gen_golden import _ref_opt
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from gen_local_z_golden import z_masks
    import models
    quiet = contextlib.redirect_stdout(io.StringIO())
    with quiet:
        m = models.create_model(_ref_opt(False))
    fill_formula_weights(m.netG, gain=0.5)
    lr = seeded_uniform((1, 3, 24, 28), 920)
    Bz = 3
    im_mask, z_mask = z_masks()
    s = scribble_b(96, 112)
    desired = seeded_uniform((1, 3, 96, 112), 1503)
    out['b/mask/image'], out['b/mask/Z'], out['b/scribble'], out['b/desired_in'] = im_mask, z_mask, s, desired.numpy()
    for mode in ('local', 'nonlocal'):
        z0 = seeded_uniform((Bz, 3, 96, 112), 921, -0.3, 0.3)
        z1 = seeded_uniform((Bz, 3, 96, 112), 922, -0.3, 0.3)
        m.feed_data({'LR': lr.expand(Bz, -1, -1, -1).clone(), 'Z': z0.clone()}, need_GT=False)
        m.test()
        data = {'LR': lr.expand(Bz, -1, -1, -1).clone(), 'desired': desired.clone(), 'scribble_mask': s.copy(), 'brightness_factor': BRIGHTNESS}
        with quiet, uint8_comparisons():
            zo = Z_optimizer(objective='scribble', Z_size=[96, 112], model=m, Z_range=1, max_iters=4, data=data, initial_Z=z1.clone(), initial_LR=0.1,
                             batch_size=Bz, image_mask=im_mask.copy(), Z_mask=z_mask.copy(), non_local_Z_optimization=mode == 'nonlocal')
            z = zo.optimize()
        key = 'b/%s/' % mode
        out[key + 'loss'] = np.array(zo.loss_values, dtype=np.float64)
        out[key + 'Z_mask'] = zo.Z_mask.numpy().astype(np.float32)
        out[key + 'final_Z_sub'] = z[:, :, ::8, ::8].numpy().copy()
        print(mode, zo.loss_values)


def main():
    _refshim.install()
    np.bool = bool                     # the reference's np.bool (removed from NumPy); set after SciPy has imported
    import Z_optimization
    Z_optimization.rgb2hsv, Z_optimization.hsv2rgb, Z_optimization.dilate = rgb2hsv, hsv2rgb, dilate
    out = {}
    part_a(Z_optimization.Z_optimizer, out)
    if '--part-a-only' not in sys.argv:
        part_b(Z_optimization.Z_optimizer, out)
    np.savez_compressed(os.path.join(GOLDEN, 'scribble.npz'), **out)


if __name__ == '__main__':
    main()
