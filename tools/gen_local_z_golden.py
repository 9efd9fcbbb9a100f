#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY (CPU, build container): writes tests/golden/local_z.npz by running the REFERENCE's own Z_optimizer
(codes/Z_optimization.py:331-815), imported read-only through oracle/_refshim.  Run:
    python tools/gen_local_z_golden.py

(a) function level, on fixed seeded images of 40 x 52 (non-square), B = 2, with an irregular image mask.  Z_optimizer is constructed on a
    stand-in model that only holds the image (fake_H) and is asked for its Masked_STD / PeriodicityLoss, as optimize() asks:
  a/x [2, 3, 40, 52], a/mask [40, 52]          the inputs (x spans [-0.1, 1.1]: the clamp is exercised)
  a/patches [P, 49]                            the patch set of ReturnPatchExtractionMat(mask, 7, overlap=1) (row p: the pixels of patch p)
  a/std/S [P, 2], a/std/cot, a/std/grad        local Masked_STD(first_image_only=False), and d sum(S * cot) / d x
  a/<case>/loss [2], a/<case>/grad             PeriodicityLoss() with initial_STD = the STD of image 0 (the constructor's), d sum(loss) / d x;
  a/<case>/points                              cases nonint1 (one non-integer point), nonint2 (two), int1 (one integer point)
  a/<case>/lines<k>_<s>_{x,y}                  the reference's grid_sample coordinate lines of point k, sign s (non-integer cases)
(b) Z_optimizer(...).optimize() on the F7 model (oracle/gen_golden.py::gen_F7: RRDB-1, latent 3, LR 24 x 28 -> HR 96 x 112, B = 3, 4 iterations,
    Adam lr 0.1, the same seeded LR and initial Z), objectives of OBJECTIVES, each with an all-ones mask pair ('full'; the reference's local
    names need an image mask) and with an irregular image mask and a rectangular Z mask ('irr'):
  b/<objective>/<mask>/loss, initial_STD, final_Z_sub (Z[:, :, ::8, ::8]), and b/mask/{irr_image,irr_Z}
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
POINTS = {'nonint1': [[2.5, 3.25]], 'nonint2': [[2.5, 3.25], [-1.75, 4.5]], 'int1': [[3, -2]]}
OBJECTIVES = ('local_STD_increase', 'local_max_STD', 'local_STD_TV', 'local_STD_nonInt_periodicity')
Z_POINTS = [[2.5, 3.25], [-1.75, 4.5]]


def image_mask(h, w, seed):
    m = (seeded_uniform((h, w), seed).numpy() > 0.2).astype(np.float32)
    m[: h // 8] = 0
    m[:, -(w // 10):] = 0
    m[h // 4: 3 * h // 4, w // 5: 3 * w // 5] = 1
    return m


def z_masks():
    im = image_mask(96, 112, 1402)
    zm = np.zeros([96, 112], dtype=np.float32)
    zm[8:88, 16:104] = 1
    return im, zm


class _StandIn:
    """what Z_optimizer's constructor and its Masked_STD / PeriodicityLoss read of a model"""

    def __init__(self, x):
        self.fake_H = x
        self.num_latent_channels = 3
        self.netG = torch.nn.Linear(1, 1)

    def Output_Batch(self, within_0_1=False):
        return torch.clamp(self.fake_H, 0, 1) if within_0_1 else self.fake_H

    def GetLatent(self):
        return torch.zeros(1, 3, H, W)


def part_a(Z_optimizer, ReturnPatchExtractionMat, out):
    x0 = seeded_uniform((B, 3, H, W), 1401, -0.1, 1.1)
    mask = image_mask(H, W, 1400)
    out['a/x'], out['a/mask'] = x0.numpy(), mask
    mat = ReturnPatchExtractionMat(mask, patch_size=7, device='cpu', patches_overlap=1).coalesce()
    rows, cols = mat.indices().numpy()
    P = mat.size(0) // 49
    idx = np.zeros(mat.size(0), np.int64)
    idx[rows] = cols
    out['a/patches'] = idx.reshape(49, P).T.copy()
    kw = dict(Z_size=[H, W], Z_range=1, max_iters=1, initial_LR=0.1, batch_size=B, image_mask=mask, Z_mask=np.ones((H, W), np.float32))
    quiet = contextlib.redirect_stdout(io.StringIO())
    # local Masked_STD
    x = x0.clone().requires_grad_(True)
    with quiet:
        zo = Z_optimizer(objective='local_STD_increase', model=_StandIn(x0.clone()), data={'STD_increment': 0.01}, **kw)
    zo.model.fake_H = x
    S = zo.Masked_STD(first_image_only=False)
    cot = seeded_uniform(tuple(S.shape), 1403, -1.0, 1.0)
    (S * cot).sum().backward()
    out['a/std/S'], out['a/std/cot'], out['a/std/grad'] = S.detach().double().numpy(), cot.numpy(), x.grad.double().numpy()
    print('std', S.shape, float(S.mean()), float(x.grad.abs().max()))
    # PeriodicityLoss
    for case, pts in POINTS.items():
        objective = 'local_STD_nonInt_periodicity' if 'nonint' in case else 'local_STD_periodicity'
        with quiet:          # constructed on a constant image, as the model's output is at construction (initial_STD carries no gradient)
            zo = Z_optimizer(objective=objective, model=_StandIn(x0.clone()), data={'periodicity_points': pts}, **kw)
        x = x0.clone().requires_grad_(True)
        zo.model.fake_H = x
        zo.output_image = zo.model.Output_Batch(within_0_1=True)
        loss = zo.PeriodicityLoss()
        loss.sum().backward()
        out['a/%s/points' % case] = np.array(pts, dtype=np.float64)
        out['a/%s/loss' % case], out['a/%s/grad' % case] = loss.detach().double().numpy(), x.grad.double().numpy()
        out['a/%s/initial_STD' % case] = zo.initial_STD.detach().double().numpy()
        if 'nonint' in case:
            for k, pair in enumerate(zo.periodicity_points):
                for s, grid in enumerate(pair):
                    out['a/%s/lines%d_%d_x' % (case, k, s)] = grid[0, 0, :, 0].numpy().copy()
                    out['a/%s/lines%d_%d_y' % (case, k, s)] = grid[0, :, 0, 1].numpy().copy()
        print(case, out['a/%s/loss' % case], float(x.grad.abs().max()))


def part_b(Z_optimizer, out):
    from oracle.gen_golden import _ref_opt
    import models
    quiet = contextlib.redirect_stdout(io.StringIO())
    with quiet:
        m = models.create_model(_ref_opt(False))
    fill_formula_weights(m.netG, gain=0.5)
    lr = seeded_uniform((1, 3, 24, 28), 920)
    Bz = 3
    irr_im, irr_z = z_masks()
    out['b/mask/irr_image'], out['b/mask/irr_Z'] = irr_im, irr_z
    ones = np.ones([96, 112], dtype=np.float32)
    for obj in OBJECTIVES:
        for mname, (im_mask, z_mask) in (('full', (ones, ones)), ('irr', (irr_im, irr_z))):
            z0 = seeded_uniform((Bz, 3, 96, 112), 921, -0.3, 0.3)
            m.feed_data({'LR': lr.expand(Bz, -1, -1, -1).clone(), 'Z': z0.clone()}, need_GT=False)
            m.test()
            data = {'LR': lr.expand(Bz, -1, -1, -1).clone(), 'STD_increment': 0.01, 'periodicity_points': Z_POINTS}
            with quiet:
                zo = Z_optimizer(objective=obj, Z_size=[96, 112], model=m, Z_range=1, max_iters=4, data=data, initial_Z=z0.clone(), initial_LR=0.1,
                                 batch_size=Bz, image_mask=im_mask.copy(), Z_mask=z_mask.copy())
                initial = zo.initial_STD.detach().double().numpy().copy()
                z = zo.optimize()
            key = 'b/%s/%s/' % (obj, mname)
            out[key + 'loss'] = np.array(zo.loss_values, dtype=np.float64)
            out[key + 'initial_STD'] = initial
            out[key + 'final_Z_sub'] = z[:, :, ::8, ::8].numpy().copy()
            print(obj, mname, initial.shape, zo.loss_values)


def main():
    _refshim.install()
    np.bool = bool                     # the reference's np.bool (removed from NumPy); set after SciPy has imported
    from Z_optimization import ReturnPatchExtractionMat, Z_optimizer
    out = {}
    part_a(Z_optimizer, ReturnPatchExtractionMat, out)
    if '--part-a-only' not in sys.argv:
        part_b(Z_optimizer, out)
    np.savez_compressed(os.path.join(GOLDEN, 'local_z.npz'), **out)


if __name__ == '__main__':
    main()
