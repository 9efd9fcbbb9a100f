#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY (CPU, build container): writes tests/golden/jpeg_eval.npz by running the REFERENCE's own JpegDataset
(codes/data/JPEG_dataset.py) and util.tensor2img's chroma branches (codes/utils/util.py:196-228, which import under oracle/_refshim: its cv2
and torchvision stubs are enough for what these branches call), imported read-only through oracle/_refshim.  Run:
    python tools/gen_jpeg_eval_golden.py

The shim's cv2 stub is completed as tools/gen_data_golden.py completes it (imread through PIL).  Only data goes into the file:

  img/<i>                            the source images, uint8 (HWC RGB as PIL writes them, or HW for the grey one); tests write them to PNGs
  case/<name>/opt                    the dataset options as JSON (without dataroot_Uncomp), /seed, /indices: the order the items were asked for,
                                     /len, /names: the base names of paths_Uncomp
  case/<name>/<n>/{Uncomp,QF,name}   the reference's item n of that order, after random.seed(seed) and np.random.seed(seed)
      train_y, train_chroma (patch 32, quality factors [10, [20, 50], 90] with QF_probs), val_y, test_chroma (input_downsampling 2: 16-pixel blocks)
  qf/<name>/{opt,schedule}           per_index_QF of the test phase over the 4 images for several forms of jpeg_quality_factor (with a list at
                                     least as long as the set the reference looks its VALUES up among sampled positions: recorded as it is)
  t2i/{ycbcr,y}                      float32 [3, 24, 28] and [20, 28] inputs in 0...255: bgr2ycbcr of a random image plus noise, a band pushed
                                     outside [0, 255]
  t2i/<in>_<range>_{u8,f32}          util.tensor2img(input, np.uint8 / np.float32, min_max, chroma_mode) for min_max [0, 255] and [16, 235]
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from oracle import _refshim  # noqa: E402
from gen_data_golden import complete_cv2_stub, write_pngs  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SIZES = [(40, 48, 3), (48, 40, 3), (56, 44, 3), (41, 46, 1)]
BASE = dict(name='golden', data_type='img', subset_file=None, scales=None, input_downsampling=None, QF_probs=None, use_flip=True, use_rot=True,
            use_shuffle=False, n_workers=0, batch_size=2, patch_size=32)
MIXED_QF = [10, [20, 50], 90]
CASES = {
    'train_y': dict(BASE, mode='JPEG', phase='train', jpeg_quality_factor=MIXED_QF, QF_probs=[1.0, 2.0, 1.0]),
    'train_chroma': dict(BASE, mode='JPEG_chroma', phase='train', jpeg_quality_factor=MIXED_QF),
    'val_y': dict(BASE, mode='JPEG', phase='val', jpeg_quality_factor=15),
    'test_chroma': dict(BASE, mode='JPEG_chroma', phase='test', jpeg_quality_factor=[10, [30, 70]], input_downsampling=2),
}
SEEDS = {'train_y': 21, 'train_chroma': 22, 'val_y': 23, 'test_chroma': 24}
QF_FORMS = {'single': 15, 'longer_list': [10, 20, 30, 40, 50, 60], 'longer_small': [1, 2, 3, 4, 5, 6], 'one_range': [10, [30, 70]], 'two_ranges': [[5, 25], 80, [40, 60]],
            'numbers': [10, 40]}
RANGES = {'0_255': [0, 255], '16_235': [16, 235]}


def images():
    rng = np.random.RandomState(20262)
    return [rng.randint(0, 256, s).astype(np.uint8).squeeze() for s in SIZES]


def ref_opt(opt, root):
    opt = dict(opt, dataroot_Uncomp=root)
    if opt['QF_probs'] is not None:
        opt['QF_probs'] = np.array(opt['QF_probs'])           # the reference normalises it in place
    return opt


def dataset_cases(out, root):
    from data.JPEG_dataset import JpegDataset
    quiet = contextlib.redirect_stdout(io.StringIO())
    for name, opt in CASES.items():
        with quiet, contextlib.redirect_stderr(io.StringIO()):
            ds = JpegDataset(ref_opt(opt, root))
        n = len(ds)
        indices = list(range(n)) + ([2, 0, 3, 1] if opt['phase'] == 'train' else [])
        out['case/%s/opt' % name] = np.array(json.dumps(opt))
        out['case/%s/seed' % name] = np.array(SEEDS[name])
        out['case/%s/indices' % name] = np.array(indices)
        out['case/%s/len' % name] = np.array(n)
        out['case/%s/names' % name] = np.array([os.path.basename(p) for p in ds.paths_Uncomp])
        random.seed(SEEDS[name])
        np.random.seed(SEEDS[name])
        for j, i in enumerate(indices):
            with quiet:
                item = ds[i]
            out['case/%s/%d/Uncomp' % (name, j)] = item['Uncomp'].numpy()
            out['case/%s/%d/QF' % (name, j)] = np.array(int(item['QF']))
            out['case/%s/%d/name' % (name, j)] = np.array(os.path.basename(item['Uncomp_path']))
        print(name, n, 'images,', len(indices), 'items, last', tuple(item['Uncomp'].shape), 'QF', [int(out['case/%s/%d/QF' % (name, j)]) for j in range(len(indices))])
    for name, form in QF_FORMS.items():
        opt = dict(BASE, mode='JPEG', phase='test', jpeg_quality_factor=form)
        with quiet, contextlib.redirect_stderr(io.StringIO()):
            ds = JpegDataset(ref_opt(opt, root))
        out['qf/%s/opt' % name] = np.array(json.dumps(opt))
        out['qf/%s/schedule' % name] = np.array([int(q) for q in ds.per_index_QF])
        print('schedule', name, form, '->', out['qf/%s/schedule' % name].tolist())


def decoder_like(shape, seed):
    """float32 [3, H, W] YCbCr in 0...255 as the decoder gives it: the conversion of a random image plus noise of a few levels, and a band of
    rows pushed outside [0, 255] so that tensor2img's clip works"""
    rng = np.random.RandomState(seed)
    bgr = rng.randint(0, 256, shape + (3,)).astype(np.float64)
    ycc = np.matmul(bgr, [[24.966, 112.0, -18.214], [128.553, -74.203, -93.786], [65.481, -37.797, 112.0]]) / 255.0 + [16, 128, 128]
    ycc = ycc + rng.normal(0, 3.0, ycc.shape)
    ycc[2:5] += 120.0
    ycc[7:9] -= 120.0
    return np.ascontiguousarray(ycc.transpose(2, 0, 1)).astype(np.float32)


def tensor2img_cases(out):
    import torch
    import utils.util as util
    out['t2i/ycbcr'] = decoder_like((24, 28), 20263)
    out['t2i/y'] = decoder_like((20, 28), 20264)[0]
    for key, mode in (('ycbcr', 'YCbCr'), ('y', 'Y')):
        for rname, min_max in RANGES.items():
            for tname, out_type in (('u8', np.uint8), ('f32', np.float32)):
                img = util.tensor2img(torch.from_numpy(out['t2i/' + key].copy()), out_type=out_type, min_max=min_max, chroma_mode=mode)
                assert img.dtype == out_type and img.shape[2] == 3
                out['t2i/%s_%s_%s' % (key, rname, tname)] = img
    u8 = out['t2i/ycbcr_0_255_u8']
    print('tensor2img: clipped to 0 / 255 in %.1f %% / %.1f %% of the YCbCr case' % (100 * (u8 == 0).mean(), 100 * (u8 == 255).mean()))


def main():
    _refshim.install()
    np.bool = bool                     # the reference's np.bool (removed from NumPy); set after SciPy has imported
    complete_cv2_stub()
    out = {}
    arrays = images()
    for i, a in enumerate(arrays):
        out['img/%d' % i] = a
    with tempfile.TemporaryDirectory() as tmp:
        write_pngs(arrays, tmp)
        dataset_cases(out, tmp)
    tensor2img_cases(out)
    path = os.path.join(GOLDEN, 'jpeg_eval.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
