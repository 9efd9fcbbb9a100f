#!/usr/bin/env python
"""Explorable decodes of a folder of JPEG files (esr_hip/jpeg_file.py, models/DecompCNN_model.py).

    python tools/decode_jpegs.py DIR --opt options/test/test_JPEG.json [--chroma] [--samples S] [--seed N]

Next to every .jpg / .jpeg of DIR it writes, as PNG:
    <name>_baseline.png     what an ordinary decoder shows (JpegFile.baseline_image: the extract kernels, no generator)
    <name>_z0.png           the explorable decode at Z = 0
    <name>_z<k>.png         S decodes at random Z, uniform in [-1, 1] per block and channel
The options file is the reference's test_JPEG.json (path.pretrained_model_G, and for --chroma path.Y_channel_model_G, name the generators).
Without --chroma the Y model decodes grey files and the luminance of colour files (grey pictures); with it the colour model decodes 4:2:0
files (RGB pictures) and other files are reported and skipped.  Files are entropy-decoded on a thread pool (jpeg_file.load_many); every output
of the models re-quantises to the file's own coefficients under the file's own tables."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'explorable-super-resolution_amd'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def write_png(path, image):
    """[1, C, H, W] in 0...1 -> PNG"""
    from PIL import Image
    arr = (torch.clamp(image[0], 0, 1) * 255).round().byte().permute(1, 2, 0).cpu().numpy()
    Image.fromarray(arr[..., 0] if arr.shape[2] == 1 else arr).save(path)


def decode(model, f, chroma, Z):
    data = f.model_data(chroma)
    feed = {k: v for k, v in data.items() if k != 'compressed_chroma'}
    model.feed_data(dict(feed, Z=Z), need_GT=False)
    model.test(**({'compressed_chroma': data['compressed_chroma']} if chroma else {}))
    return f.crop(model.Output_Batch(within_0_1=True))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('dir')
    ap.add_argument('--opt', required=True)
    ap.add_argument('--chroma', action='store_true')
    ap.add_argument('--samples', type=int, default=0)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args(argv)
    from esr_hip import jpeg_file
    from models import create_model
    from options import options as option
    opt = option.dict_to_nonedict(option.parse(a.opt, is_train=False, JPEG=True, chroma=a.chroma))
    model = create_model(opt, chroma_mode=True) if a.chroma else create_model(opt)
    names = sorted(n for n in os.listdir(a.dir) if n.lower().endswith(('.jpg', '.jpeg')))
    paths, refused = [os.path.join(a.dir, n) for n in names], {}
    files = jpeg_file.load_many(paths, device=model.device, on_error=refused.__setitem__)      # a refused file is reported, the rest go on
    for e in refused.values():
        print('skipped: %s' % e)
    paths = [p for p in paths if p not in refused]
    g = torch.Generator().manual_seed(a.seed)
    for path, f in zip(paths, files):
        stem = os.path.splitext(path)[0]
        H, W = f.padded_size
        done = 0
        for what in ('baseline', 'model'):              # what either refuses for this file is reported; the other, and the folder, go on
            try:
                if what == 'baseline':
                    write_png(stem + '_baseline.png', f.baseline_image())
                    done += 1
                    continue
                write_png(stem + '_z0.png', decode(model, f, a.chroma, 0.0))
                for k in range(a.samples):
                    Z = 2 * torch.rand(1, model.num_latent_channels, H // 8, W // 8, generator=g) - 1
                    write_png(stem + '_z%d.png' % (k + 1), decode(model, f, a.chroma, Z))
                done += 1 + a.samples
            except NotImplementedError as e:
                print('skipped (%s): %s' % (what, e))
        print('%s: %d x %d %s, %d decodes' % (f.name, f.width, f.height, f.sampling, done))


if __name__ == '__main__':
    main()
