#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY (CPU, build container): writes tests/golden/patch_kde.npz by running the REFERENCE's own SoftHistogramLoss and
ReturnPatchExtractionMat (codes/Z_optimization.py:24-272), imported read-only through oracle/_refshim.  Run:
    python tools/gen_patch_kde_golden.py

Contents:
  sel/<mask>_<overlap>     [P, 36] int64   the patches ReturnPatchExtractionMat selects (row p: the pixels of patch p), for the masks
                                           mask/full and mask/irr and overlaps 0.5 ('half') and 30/36 ('desired')
  in/desired, in/cur       [1|2, 3, 24, 28] the desired image (smooth) and the current batch (a noisy copy of it: the losses are not
                                           degenerate — pure noise gives histogram gradients of ~1e-23)
  <case>/loss, <case>/grad                 the loss and d loss / d cur, for the cases of CASES
  <case>/bins              [M, D] float64  the de-duplicated bins (patch cases)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import _refshim  # noqa: E402
from oracle.weights import seeded_uniform  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
H, W = 24, 28
# case: (objective settings, desired mask, image mask) — the settings are Z_optimizer's (reference :536-543)
CASES = {
    'patchhist': (dict(patch_size=6, temperature=5e-4, dictionary_not_histogram=False, no_patch_DC=False), 'full', 'full'),
    'patchhist_noDC': (dict(patch_size=6, temperature=5e-4, dictionary_not_histogram=False, no_patch_DC=True), 'irr', 'full'),
    'patchdict_noDC': (dict(patch_size=6, temperature=1e-3, dictionary_not_histogram=True, no_patch_DC=True), 'full', 'full'),
    'patchdict_noDC_masked': (dict(patch_size=6, temperature=1e-3, dictionary_not_histogram=True, no_patch_DC=True), 'full', 'irr'),
    'dict_noDC': (dict(patch_size=1, temperature=1e-3, dictionary_not_histogram=True, no_patch_DC=True), 'full', 'full'),
}


def masks():
    irr = (seeded_uniform((H, W), 1301).numpy() > 0.15).astype(np.float32)
    irr[:3] = 0
    irr[:, -4:] = 0
    irr[6:18, 4:20] = 1
    return {'full': np.ones((H, W), np.float32), 'irr': irr}


def inputs():
    coarse = seeded_uniform((1, 3, 5, 6), 1302)
    desired = torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=True)
    cur = (desired + 0.04 * (seeded_uniform((2, 3, H, W), 1303) - 0.5)).clamp(0, 1)
    return desired, cur


def _mask_xor():
    """Desired_Im_2_Bins (:119) forms its keep mask as `bool_tensor ^ 1`.  In the PyTorch the reference was written for, comparisons gave
    uint8 and uint8 ^ 1 stayed a uint8 MASK; current PyTorch promotes bool ^ int to int64, and `im[:, mask]` then gathers patches 0 and 1
    instead of masking.  Restore the original meaning for this generator process only: a bool tensor XOR a Python int stays bool."""
    xor = torch.Tensor.__xor__

    def bool_xor(self, other):
        if self.dtype == torch.bool and isinstance(other, int) and not isinstance(other, bool):
            return xor(self, bool(other))
        return xor(self, other)
    torch.Tensor.__xor__ = bool_xor


def main():
    _refshim.install()
    _mask_xor()
    np.bool = bool                     # the reference's np.bool (removed from NumPy); set after SciPy has imported
    from Z_optimization import ReturnPatchExtractionMat, SoftHistogramLoss
    out = {}
    ms = masks()
    for name, m in ms.items():
        out['mask/' + name] = m
        for oname, ov in (('half', 0.5), ('desired', 30 / 36)):
            mat = ReturnPatchExtractionMat(m, patch_size=6, device='cpu', patches_overlap=ov).coalesce()
            rows, cols = mat.indices().numpy()
            P = mat.size(0) // 36
            idx = np.zeros(mat.size(0), np.int64)
            idx[rows] = cols
            out['sel/%s_%s' % (name, oname)] = idx.reshape(36, P).T.copy()
    desired, cur0 = inputs()
    out['in/desired'], out['in/cur'] = desired.numpy(), cur0.numpy()
    for case, (cfg, dmask, imask) in CASES.items():
        loss_fn = SoftHistogramLoss(bins=256, min=0, max=1, desired_hist_image=[desired.clone()], desired_hist_image_mask=[ms[dmask]],
                                    input_im_HR_mask=torch.from_numpy(ms[imask]), gray_scale=True, **cfg)
        cur = cur0.clone().requires_grad_(True)
        loss = loss_fn(cur)
        loss.sum().backward()
        out[case + '/loss'] = loss.detach().double().numpy().reshape(-1)
        out[case + '/grad'] = cur.grad.double().numpy()
        if cfg['patch_size'] > 1:
            out[case + '/bins'] = loss_fn.bins.reshape(36, -1).t().double().numpy()
        print(case, out[case + '/loss'], float(np.abs(out[case + '/grad']).max()), out.get(case + '/bins', np.zeros((0,))).shape)
    np.savez_compressed(os.path.join(GOLDEN, 'patch_kde.npz'), **out)


if __name__ == '__main__':
    main()
