#!/usr/bin/env python
"""Estimate the downscaling kernel of every image of a folder (KernelGAN) and write it where data/LR_dataset.py (test.kernel == 'estimated')
looks for it: <image>_kernel_x4.mat next to the image, or kernel_<n>_x4.mat for images named img_<n> — key 'Kernel'.

    python tools/estimate_kernels.py DIR [--X4] [--batch E] [--real_image] [--max_iters N] [--engine hip|stock]

--batch E estimates E images in lock step in the same kernel launches (engine 'hip')."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'explorable-super-resolution_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.tif')


def kernel_path(im_path, scale):
    """LRDataset's two naming rules (data/LR_dataset.py), for x2 or x4."""
    if 'img_' in im_path:
        return im_path.replace('img', 'kernel_')[:-4] + '_x%d.mat' % scale
    return im_path[:-4] + '_kernel_x%d.mat' % scale


def write_kernel(im_path, kernel, scale):
    import scipy.io
    path = kernel_path(im_path, scale)
    scipy.io.savemat(path, {'Kernel': np.asarray(kernel)})
    return path


def image_files(folder):
    return sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.lower().endswith(IMG_EXTENSIONS) and os.path.isfile(os.path.join(folder, f)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('dir')
    ap.add_argument('--X4', action='store_true')
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--real_image', action='store_true')
    ap.add_argument('--max_iters', type=int, default=3000)
    ap.add_argument('--engine', default='hip', choices=('hip', 'stock'))
    args = ap.parse_args(argv)
    from PIL import Image
    from KernelGAN import train as KernelGAN
    files = image_files(args.dir)
    if not files:
        sys.exit('no images in %s' % args.dir)
    flags = ['--max_iters', str(args.max_iters)] + (['--X4'] if args.X4 else []) + (['--real_image'] if args.real_image else [])
    for i in range(0, len(files), max(1, args.batch)):
        group, confs = files[i:i + max(1, args.batch)], []
        for f in group:
            conf = KernelGAN.Config().parse(flags + ['--input_image_path', f])
            conf.LR_image = np.array(Image.open(f).convert('RGB'), dtype=np.uint8)
            confs.append(conf)
        for f, k in zip(group, KernelGAN.train_batch(confs, engine=args.engine)):
            print(write_kernel(f, k, 4 if args.X4 else 2))


if __name__ == '__main__':
    main()
