"""Image files and the per-image NumPy operations of the datasets — the surface of the reference's codes/data/util.py that LRHRDataset and
LRDataset use (IMG_EXTENSIONS, is_image_file, get_image_paths, read_img, augment, channel_convert, bgr2ycbcr / rgb2ycbcr / ycbcr2rgb, modcrop),
written from scratch on PIL and NumPy: no cv2, lmdb, skimage or imagesize.  Images are HWC, BGR channel order (cv2.imread's), float32 in [0, 1].

Not part of this build: lmdb reading (get_image_paths raises), the ImageNet sub-folder lists, the MATLAB-style imresize / imresize_np.
The float colour conversions return the reference's values but leave their argument alone (the reference's `img *= 255.` scales the caller's
array in place)."""
import os
import random

import numpy as np

IMG_EXTENSIONS = ['.jpg', '.JPG', '.jpeg', '.JPEG', '.png', '.PNG', '.ppm', '.PPM', '.bmp', '.BMP', 'tif']


def is_image_file(filename):
    return any(filename.endswith(extension) for extension in IMG_EXTENSIONS)


def _get_paths_from_images(path):
    assert os.path.isdir(path), '{:s} is not a valid directory'.format(path)
    images = [os.path.join(path, fname) for fname in os.listdir(path) if is_image_file(fname)]      # this folder only, no sub-folders
    assert images, '{:s} has no valid image file'.format(path)
    return images


def get_image_paths(data_type, dataroot, patch_size=None):
    """(env, sorted paths) of a dataset root; (None, None) for no root.  env is the lmdb environment of the reference: always None here."""
    env, paths = None, None
    if dataroot is not None:
        if data_type == 'lmdb':
            try:
                import lmdb  # noqa: F401
            except ImportError:
                raise ImportError('data_type lmdb [{:s}]: the lmdb package is not installed'.format(dataroot))
            raise NotImplementedError('data_type lmdb [{:s}]: lmdb datasets are not read by this package, use image folders'.format(dataroot))
        elif data_type == 'img':
            paths = sorted(_get_paths_from_images(dataroot))
        else:
            raise NotImplementedError('data_type [{:s}] is not recognized.'.format(data_type))
    return env, paths


def read_img_uint8(env, path):
    """The decoded file as cv2.imread(path, IMREAD_UNCHANGED) of an 8-bit image returns it, HWC uint8 with 1 or 3 channels: grey images get a
    trailing axis, colour is BGR, a fourth (alpha) channel is dropped."""
    if env is not None:
        raise NotImplementedError('lmdb datasets are not read by this package')
    from PIL import Image
    with Image.open(path) as im:
        if im.mode == '1':
            im = im.convert('L')
        elif im.mode not in ('L', 'RGB', 'RGBA'):
            im = im.convert('RGB')
        img = np.asarray(im)
    if img.ndim == 2:
        return np.array(img[:, :, None])                     # (a copy: PIL's buffer is read-only)
    return np.ascontiguousarray(img[:, :, 2::-1])            # RGB(A) -> BGR


def read_img(env, path):
    """Numpy float32, HWC, BGR, [0, 1]"""
    return read_img_uint8(env, path).astype(np.float32) / 255.


def draw_augment(hflip=True, rot=True):
    """The three decisions of augment, drawn in its order; a decision whose flag is off draws nothing."""
    hflip = hflip and random.random() < 0.5
    vflip = rot and random.random() < 0.5
    rot90 = rot and random.random() < 0.5
    return hflip, vflip, rot90


def augment(img_list, hflip=True, rot=True):
    """horizontal flip, vertical flip, transpose — each with probability 1 / 2, the same for every image of the list"""
    hflip, vflip, rot90 = draw_augment(hflip, rot)

    def _augment(img):
        if hflip:
            img = img[:, ::-1, :]
        if vflip:
            img = img[::-1, :, :]
        if rot90:
            img = img.transpose(1, 0, 2)
        return img
    return [_augment(img) for img in img_list]


GRAY_WEIGHTS = [0.114, 0.587, 0.299]                  # B, G, R (cv2.COLOR_BGR2GRAY)
Y_WEIGHTS_BGR = [24.966, 128.553, 65.481]


def channel_convert(in_c, tar_type, img_list):
    """every image of img_list (in_c channels, BGR) as tar_type: 'gray', 'y', 'ycbcr' from 3 channels, 'RGB' (three equal channels) from 1;
    anything else returns the list as it is"""
    if in_c == 3 and tar_type == 'gray':
        return [np.expand_dims(np.dot(img, GRAY_WEIGHTS).astype(img.dtype), axis=2) for img in img_list]
    elif in_c == 3 and tar_type == 'y':
        return [np.expand_dims(bgr2ycbcr(img, only_y=True), axis=2) for img in img_list]
    elif in_c == 3 and tar_type == 'ycbcr':
        return [bgr2ycbcr(img, only_y=False) for img in img_list]
    elif in_c == 1 and tar_type == 'RGB':
        return [np.repeat(img.reshape(img.shape[0], img.shape[1], 1), 3, axis=2) for img in img_list]
    else:
        return img_list


def _in_0_255(img):
    """uint8 as it is; float [0, 1] scaled by 255 in its own dtype, into a new array"""
    return img if img.dtype == np.uint8 else img * 255.


def _out_like(rlt, in_img_type):
    rlt = rlt.round() if in_img_type == np.uint8 else rlt / 255.
    return rlt.astype(in_img_type)


def rgb2ycbcr(img, only_y=True):
    """ITU-R BT.601 YCbCr (MATLAB's rgb2ycbcr) of an RGB image: uint8 in [0, 255] -> uint8, float in [0, 1] -> the same float type;
    only_y: the luma plane alone, [H, W]"""
    x = _in_0_255(img)
    if only_y:
        rlt = np.dot(x, [65.481, 128.553, 24.966]) / 255.0 + 16.0
    else:
        rlt = np.matmul(x, [[65.481, -37.797, 112.0], [128.553, -74.203, -93.786], [24.966, 112.0, -18.214]]) / 255.0 + [16, 128, 128]
    return _out_like(rlt, img.dtype)


def bgr2ycbcr(img, only_y=True):
    """rgb2ycbcr for BGR channel order"""
    x = _in_0_255(img)
    if only_y:
        rlt = np.dot(x, Y_WEIGHTS_BGR) / 255.0 + 16.0
    else:
        rlt = np.matmul(x, [[24.966, 112.0, -18.214], [128.553, -74.203, -93.786], [65.481, -37.797, 112.0]]) / 255.0 + [16, 128, 128]
    return _out_like(rlt, img.dtype)


def ycbcr2rgb(img):
    """the inverse conversion (MATLAB's ycbcr2rgb), same input conventions"""
    x = _in_0_255(img)
    rlt = np.matmul(x, [[0.00456621, 0.00456621, 0.00456621], [0, -0.00153632, 0.00791071], [0.00625893, -0.00318811, 0]]) * 255.0 \
        + [-222.921, 135.576, -276.836]
    return _out_like(rlt, img.dtype)


def modcrop(img_in, scale):
    """a copy of img_in (HWC or HW) without the last H % scale rows and W % scale columns"""
    img = np.copy(img_in)
    if img.ndim not in (2, 3):
        raise ValueError('Wrong img ndim: [{:d}].'.format(img.ndim))
    H, W = img.shape[:2]
    return img[:H - H % scale, :W - W % scale]
