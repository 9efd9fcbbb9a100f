"""Writes the files of this folder and expected.npz:  python tests/golden/jpeg_files/generate.py  (needs Pillow).

Small JPEG files made with Pillow from the seeded pictures of tests/test_host_jpeg_file.py, and per file what the independent Python decoder of
that test reads from it (coefficients [64, hb, wb] and tables [8, 8] per component) and what Pillow's own decode shows (Y at full size,
Cb and Cr at the half-size draft).  The GPU tests read only this folder and need no Pillow.  The record names the Pillow and libjpeg
versions that wrote it: another encoder version may write other bytes, in which case the files and the record are replaced together."""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
for p in (ROOT, os.path.join(ROOT, 'explorable-super-resolution_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import PIL  # noqa: E402
from PIL import Image, features  # noqa: E402

import test_host_jpeg_file as T  # noqa: E402


def midgrey(width, height):
    """Y within 128 +- 24 and mild colour: the colour model's generated Y plane stays clear of 0 and 255 around it"""
    rng = np.random.RandomState(77)
    yy, xx = np.mgrid[0:height, 0:width]
    y = 128 + 16 * np.sin(xx / 4.0) * np.cos(yy / 6.0) + rng.randint(-8, 9, (height, width))
    rgb = y[..., None] + np.stack([12 * np.sin(yy / 5.0), -8 * np.cos(xx / 7.0), 10 * np.sin((xx + yy) / 9.0)], -1)
    buf = io.BytesIO()
    Image.fromarray(np.clip(rgb, 0, 255).astype(np.uint8)).save(buf, 'JPEG', quality=90, subsampling=2)
    return buf.getvalue()


FILES = {
    'grey_8x8': lambda: T.jpeg_bytes(8, 8, 'L', quality=50, optimize=True),
    'grey_9x7': lambda: T.jpeg_bytes(9, 7, 'L', quality=95, optimize=True),
    'grey_33x17': lambda: T.jpeg_bytes(33, 17, 'L', quality=75, optimize=True),
    'c420_16x16': lambda: T.jpeg_bytes(16, 16, 'RGB', quality=50, subsampling=2, optimize=True),
    'c420_41x57': lambda: T.jpeg_bytes(41, 57, 'RGB', quality=50, subsampling=2, optimize=True, restart_marker_rows=1),
    'c420_midgrey_32x48': lambda: midgrey(32, 48),
}


def main():
    rec = {'names': np.array(sorted(FILES)), 'pillow_version': np.array(PIL.__version__), 'libjpeg_version': np.array(str(features.version('jpg')))}
    for name in sorted(FILES):
        data = FILES[name]()
        assert len(data) < 4096, (name, len(data))
        with open(os.path.join(HERE, name + '.jpg'), 'wb') as f:
            f.write(data)
        dec = T.py_decode(data)
        planes = T.pillow_planes(data)
        for c, coef in enumerate(dec['coef']):
            assert np.abs(coef).max() < 32768
            rec['%s/coef%d' % (name, c)] = coef.astype(np.int16)
            rec['%s/table%d' % (name, c)] = dec['tables'][dec['comps'][c][2]].reshape(8, 8).astype(np.uint16)
            rec['%s/pillow%d' % (name, c)] = planes[c].astype(np.uint8)
        rec['%s/size' % name] = np.array([dec['height'], dec['width']])
        print('%s: %d bytes, %s' % (name, len(data), [c.shape for c in dec['coef']]))
    np.savez_compressed(os.path.join(HERE, 'expected.npz'), **rec)


if __name__ == '__main__':
    main()
