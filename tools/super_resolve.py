#!/usr/bin/env python
"""Super-resolve a folder of images in batches, every image under its own estimated blur kernel (models/SRRaGAN_model.py: set_kernels).

    python tools/super_resolve.py DIR --opt options/test/test_sr.json [--kernels estimated] [--batch N]

Next to every image of DIR it writes <name>_SR.png.  The images are grouped by size and run N (default 8) at a time through one model:
--kernels estimated reads every image's kernel from where tools/estimate_kernels.py wrote it (<name>_kernel_x<scale>.mat, key 'Kernel') and
sets the kernels of a batch with model.set_kernels — the Consistency Enforcing Module then projects every image with its own kernel while the
generator, its checkpoint and its weight packs are built once.  An image without a kernel file gets the kernel of the options file
(test.kernel), as every image does without --kernels.  Models with a latent input run at Z = 0."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'explorable-super-resolution_amd'), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from estimate_kernels import image_files, kernel_path  # noqa: E402


def read_image(path):
    """-> [3, h, w] float32 in 0...1"""
    import torch
    from PIL import Image
    arr = np.asarray(Image.open(path).convert('RGB'), dtype=np.float32) / 255.0
    return torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))


def write_png(path, image):
    """[3, H, W] in 0...1 -> PNG"""
    import torch
    from PIL import Image
    Image.fromarray((torch.clamp(image, 0, 1) * 255).round().byte().permute(1, 2, 0).cpu().numpy()).save(path)


def read_kernel(im_path, scale):
    """The kernel tools/estimate_kernels.py wrote for this image (summing to 1 in float64, as imresize asks of a given kernel), or None"""
    import scipy.io
    path = kernel_path(im_path, scale)
    if not os.path.isfile(path):
        return None
    kernel = np.asarray(scipy.io.loadmat(path)['Kernel'], dtype=np.float64)
    return kernel / kernel.sum()


def groups_by_size(files, images, batch):
    """[(file, image)] of one size, at most `batch` of them, in the order of `files`"""
    by_size = {}
    for f, im in zip(files, images):
        by_size.setdefault(tuple(im.shape[1:]), []).append((f, im))
    for items in by_size.values():
        for i in range(0, len(items), batch):
            yield items[i:i + batch]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('dir')
    ap.add_argument('--opt', required=True)
    ap.add_argument('--kernels', default='options', choices=('options', 'estimated'))
    ap.add_argument('--batch', type=int, default=8)
    a = ap.parse_args(argv)
    import torch
    from models import create_model
    from options import options as option
    opt = option.dict_to_nonedict(option.parse(a.opt, is_train=False))
    model = create_model(opt)
    files = [f for f in image_files(a.dir) if not f.endswith('_SR.png')]
    if not files:
        sys.exit('no images in %s' % a.dir)
    images = [read_image(f) for f in files]
    per_image = False
    for group in groups_by_size(files, images, max(1, a.batch)):
        kernels = [read_kernel(f, opt['scale']) if a.kernels == 'estimated' else None for f, _ in group]
        if any(k is not None for k in kernels):
            model.set_kernels(kernels)
            per_image = True
        elif per_image:                      # back to the options' kernel (a model without a CEM is never asked)
            model.set_kernels(None)
            per_image = False
        data = {'LR': torch.stack([im for _, im in group])}
        if model.latent_input is not None:
            data['Z'] = 0.0
        model.feed_data(data, need_GT=False)
        model.test()
        for (f, _), sr, k in zip(group, model.Output_Batch(within_0_1=True), kernels):
            out = os.path.splitext(f)[0] + '_SR.png'
            write_png(out, sr)
            print('%s (%s kernel)' % (out, 'estimated' if k is not None else "the options'"))


if __name__ == '__main__':
    main()
