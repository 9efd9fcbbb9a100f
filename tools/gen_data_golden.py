#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY (CPU, build container): writes tests/golden/lrhr_dataset.npz by running the REFERENCE's own LRHRDataset
(codes/data/LRHR_dataset.py) and data/util.py functions, imported read-only through oracle/_refshim.  Run:
    python tools/gen_data_golden.py

The shim's cv2 stub is completed here, for this process only, with what this path calls: imread (through PIL: BGR order, grey images 2-D, as
cv2.IMREAD_UNCHANGED gives them) and an INTER_LINEAR resize that accepts only the size the image already has and returns a copy (the
reference resizes every training image to its own size when random_scale_list is [1]); INTER_CUBIC stays the shim's (the bicubic taps).

  img/<set>/<i>                     the source images, uint8 (HWC RGB as PIL writes them, or HW); the tool writes them to temporary PNGs
  case/<name>/opt                   the dataset options as JSON (without dataroot_HR), /seed, /indices: the order the items were asked for
  case/<name>/<n>/{LR,HR}           the reference's item n of that order, after random.seed(seed)
      train_x4 (scale 4, patch 24), train_x2 (scale 2, patch 16), train_x4_y (color 'y'), val_x4 (modcrop: 50 x 59, 45 x 41 and a grey 41 x 46)
  parts/img                         a [12, 10, 3] uint8 image and, of it (u8) and of it / 255 in float32 (f32):
  parts/{bgr2ycbcr,rgb2ycbcr}_{y,full}_{u8,f32}, parts/ycbcr2rgb_{u8,f32}, parts/channel_convert_y_f32, parts/modcrop_{3,4}
  parts/augment_<s>                 augment([img]) after random.seed(s), s = 0...11 (flip and rot on); parts/augment_flip_only_<s>: rot off
"""
import contextlib
import io
import json
import os
import random
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import _refshim  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
TRAIN_SIZES = [(40, 48), (48, 40), (56, 44), (44, 52), (48, 48)]
VAL_SIZES = [(50, 59, 3), (45, 41, 3), (41, 46, 1)]
BASE = dict(name='golden', mode='LRHR', data_type='img', dataroot_LR=None, subset_file=None, color=None, use_flip=True, use_rot=True,
            use_shuffle=False, n_workers=0, batch_size=4)
CASES = {
    'train_x4': dict(BASE, phase='train', scale=4, patch_size=24),
    'train_x2': dict(BASE, phase='train', scale=2, patch_size=16),
    'train_x4_y': dict(BASE, phase='train', scale=4, patch_size=24, color='y'),
    'val_x4': dict(BASE, phase='val', scale=4, patch_size=24),
}
SEEDS = {'train_x4': 11, 'train_x2': 12, 'train_x4_y': 13, 'val_x4': 14}


def images():
    rng = np.random.RandomState(20260)
    sets = {'train': [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in TRAIN_SIZES],
            'val': [rng.randint(0, 256, (h, w, c)).astype(np.uint8).squeeze() for h, w, c in VAL_SIZES]}
    sets['train'][0][:4] = np.arange(4 * 48 * 3).reshape(4, 48, 3) % 256       # every byte value occurs
    return sets


def write_pngs(arrays, folder):
    from PIL import Image
    for i, a in enumerate(arrays):
        Image.fromarray(a).save(os.path.join(folder, 'img_%02d.png' % i))


def complete_cv2_stub():
    import cv2
    from PIL import Image
    shim_resize = cv2.resize

    def imread(path, flags=None):
        a = np.asarray(Image.open(path))
        return a.copy() if a.ndim == 2 else a[:, :, ::-1].copy()

    def resize(src, dsize, *a, interpolation=None, **k):
        if interpolation == cv2.INTER_LINEAR:
            assert tuple(dsize) == (src.shape[1], src.shape[0]), 'a bilinear resize that changes the size is not part of the golden'
            return src.copy()
        return shim_resize(src, dsize, *a, interpolation=interpolation, **k)
    cv2.imread, cv2.resize = imread, resize


def dataset_cases(out):
    from data.LRHR_dataset import LRHRDataset
    sets = images()
    quiet = contextlib.redirect_stdout(io.StringIO())
    with tempfile.TemporaryDirectory() as tmp:
        for name, arrays in sets.items():
            os.mkdir(os.path.join(tmp, name))
            write_pngs(arrays, os.path.join(tmp, name))
            for i, a in enumerate(arrays):
                out['img/%s/%d' % (name, i)] = a
        for name, opt in CASES.items():
            which = 'val' if opt['phase'] == 'val' else 'train'
            with quiet, contextlib.redirect_stderr(io.StringIO()):
                ds = LRHRDataset(dict(opt, dataroot_HR=os.path.join(tmp, which)))
            n = len(ds)
            indices = list(range(n)) + ([3, 1, 4, 0, 2] if which == 'train' else [])
            out['case/%s/opt' % name] = np.array(json.dumps(opt))
            out['case/%s/seed' % name] = np.array(SEEDS[name])
            out['case/%s/indices' % name] = np.array(indices)
            random.seed(SEEDS[name])
            for j, i in enumerate(indices):
                with quiet:
                    item = ds[i]
                out['case/%s/%d/LR' % (name, j)] = item['LR'].numpy()
                out['case/%s/%d/HR' % (name, j)] = item['HR'].numpy()
            print(name, n, 'images,', len(indices), 'items, LR', tuple(item['LR'].shape), 'HR', tuple(item['HR'].shape))


def parts(out):
    import data.util as util
    img = np.random.RandomState(20261).randint(0, 256, (12, 10, 3)).astype(np.uint8)
    out['parts/img'] = img
    f32 = lambda: img.astype(np.float32) / 255.              # noqa: E731  (a fresh array per call: the reference scales its argument in place)
    for fn in ('bgr2ycbcr', 'rgb2ycbcr'):
        for key, only_y in (('y', True), ('full', False)):
            out['parts/%s_%s_u8' % (fn, key)] = getattr(util, fn)(img.copy(), only_y=only_y)
            out['parts/%s_%s_f32' % (fn, key)] = getattr(util, fn)(f32(), only_y=only_y)
    out['parts/ycbcr2rgb_u8'] = util.ycbcr2rgb(img.copy())
    out['parts/ycbcr2rgb_f32'] = util.ycbcr2rgb(f32())
    out['parts/channel_convert_y_f32'] = util.channel_convert(3, 'y', [f32()])[0]
    for s in (3, 4):
        out['parts/modcrop_%d' % s] = util.modcrop(img, s)
    for s in range(12):
        random.seed(s)
        out['parts/augment_%d' % s] = np.ascontiguousarray(util.augment([img], True, True)[0])
        random.seed(s)
        out['parts/augment_flip_only_%d' % s] = np.ascontiguousarray(util.augment([img], True, False)[0])


def main():
    _refshim.install()
    np.bool = bool                     # the reference's np.bool (removed from NumPy); set after SciPy has imported
    complete_cv2_stub()
    out = {}
    dataset_cases(out)
    parts(out)
    path = os.path.join(GOLDEN, 'lrhr_dataset.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
