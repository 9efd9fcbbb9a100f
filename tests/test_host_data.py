"""The `data` package on the host: data/util.py against float64 restatements written here and against what the reference's functions returned
(tests/golden/lrhr_dataset.npz, tools/gen_data_golden.py), LRHRDataset's items against the reference's under the recorded seed — which pins
the order in which `random` is consulted — and the loader / dataset factories.

Tolerances.  The colour conversions of a float32 image end in a float32 cast of a float64 expression: the restatement (same expression, float64
throughout from the float32 pixels times 255 in float32) agrees to one float32 rounding of a value in [0, 1], 2^-24 = 6e-8; against the golden
the values are equal.  LR images: the reference's imresize and this package's agree to 2e-16 in float64, items are float32: 2^-24."""
import json
import os
import random

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'lrhr_dataset.npz')
ULP = 2.0 ** -24


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def write_set(golden, name, folder):
    """the golden's images of one set as PNG files, named so that sorting keeps their order"""
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    i = 0
    while 'img/%s/%d' % (name, i) in golden:
        Image.fromarray(golden['img/%s/%d' % (name, i)]).save(os.path.join(folder, 'img_%02d.png' % i))
        i += 1
    return folder


def case_opt(golden, name, folder):
    opt = json.loads(str(golden['case/%s/opt' % name]))
    opt['dataroot_HR'] = folder
    return opt


# ---- float64 restatements
def ref_ycbcr(img, only_y, order):
    """matlab's rgb2ycbcr on a uint8 or float [0, 1] image; order 'bgr' / 'rgb'"""
    M = np.array([[65.481, -37.797, 112.0], [128.553, -74.203, -93.786], [24.966, 112.0, -18.214]])
    if order == 'bgr':
        M = M[::-1]
    x = img.astype(np.float64) if img.dtype == np.uint8 else (img * img.dtype.type(255.)).astype(np.float64)
    r = x @ M / 255.0 + np.array([16.0, 128.0, 128.0])
    r = r[..., 0] if only_y else r
    return np.round(r) if img.dtype == np.uint8 else r / 255.0


def ref_augment(img, hflip, vflip, rot90):
    out = np.empty((img.shape[1], img.shape[0], img.shape[2]) if rot90 else img.shape, img.dtype)
    H, W = img.shape[:2]
    for y in range(H):
        for x in range(W):
            fy, fx = (H - 1 - y if vflip else y), (W - 1 - x if hflip else x)
            if rot90:
                out[fx, fy] = img[y, x]
            else:
                out[fy, fx] = img[y, x]
    return out


def f32(img):
    return img.astype(np.float32) / 255.


# ---- util
@pytest.mark.parametrize('fn,order', [('bgr2ycbcr', 'bgr'), ('rgb2ycbcr', 'rgb')])
@pytest.mark.parametrize('only_y', [True, False], ids=['y', 'full'])
def test_ycbcr_matches_float64_and_the_reference(golden, fn, order, only_y):
    import data.util as util
    img = golden['parts/img']
    key = 'parts/%s_%s_' % (fn, 'y' if only_y else 'full')
    got8 = getattr(util, fn)(img, only_y=only_y)
    assert got8.dtype == np.uint8 and np.array_equal(got8, golden[key + 'u8']) and np.array_equal(got8, ref_ycbcr(img, only_y, order).astype(np.uint8))
    x = f32(img)
    got = getattr(util, fn)(x, only_y=only_y)
    assert got.dtype == np.float32 and np.array_equal(got, golden[key + 'f32'])
    assert np.abs(got - ref_ycbcr(x, only_y, order)).max() <= ULP
    x64 = x.astype(np.float64)
    assert getattr(util, fn)(x64, only_y=only_y).dtype == np.float64


def test_ycbcr2rgb_matches_the_reference(golden):
    import data.util as util
    img = golden['parts/img']
    assert np.array_equal(util.ycbcr2rgb(img), golden['parts/ycbcr2rgb_u8'])
    assert np.array_equal(util.ycbcr2rgb(f32(img)), golden['parts/ycbcr2rgb_f32'])


def test_float_colour_functions_leave_their_input_unchanged(golden):
    import data.util as util
    x = f32(golden['parts/img'])
    keep = x.copy()
    for fn in (util.bgr2ycbcr, util.rgb2ycbcr):
        for only_y in (True, False):
            fn(x, only_y=only_y)
            assert np.array_equal(x, keep)
    util.ycbcr2rgb(x)
    assert np.array_equal(x, keep)
    for tar in ('y', 'gray', 'ycbcr'):
        util.channel_convert(3, tar, [x])
        assert np.array_equal(x, keep)


def test_channel_convert(golden):
    import data.util as util
    x = f32(golden['parts/img'])
    y = util.channel_convert(3, 'y', [x])[0]
    assert y.shape == (12, 10, 1) and y.dtype == np.float32 and np.array_equal(y, golden['parts/channel_convert_y_f32'])
    assert np.abs(y[..., 0] - ref_ycbcr(x, True, 'bgr')).max() <= ULP
    g = util.channel_convert(3, 'gray', [x])[0]
    assert g.shape == (12, 10, 1) and g.dtype == np.float32
    assert np.abs(g[..., 0] - x.astype(np.float64) @ np.array([0.114, 0.587, 0.299])).max() <= ULP
    full = util.channel_convert(3, 'ycbcr', [x])[0]
    assert full.shape == (12, 10, 3) and np.array_equal(full, golden['parts/bgr2ycbcr_full_f32'])
    rgb = util.channel_convert(1, 'RGB', [y])[0]
    assert rgb.shape == (12, 10, 3) and all(np.array_equal(rgb[..., c], y[..., 0]) for c in range(3))
    assert util.channel_convert(3, 'RGB', [x])[0] is x and util.channel_convert(1, 'y', [y])[0] is y


def test_modcrop(golden):
    import data.util as util
    img = golden['parts/img']
    for s in (3, 4):
        got = util.modcrop(img, s)
        assert np.array_equal(got, golden['parts/modcrop_%d' % s]) and np.array_equal(got, img[:12 - 12 % s, :10 - 10 % s])
        assert not np.shares_memory(got, img)
    assert util.modcrop(img[..., 0], 4).shape == (12, 8)
    with pytest.raises(ValueError):
        util.modcrop(np.zeros(5), 2)


def test_augment_draws_and_mapping(golden):
    import data.util as util
    img = golden['parts/img']
    seen = set()
    for s in range(12):
        random.seed(s)
        d = [random.random() < 0.5 for _ in range(3)]          # hflip, vflip, rot90 in this order
        random.seed(s)
        got = util.augment([img, img[:, :, :1]], True, True)
        assert np.array_equal(got[0], golden['parts/augment_%d' % s]) and np.array_equal(got[0], ref_augment(img, *d))
        assert np.array_equal(got[1], ref_augment(img[:, :, :1], *d))          # one decision for the whole list
        seen.add(tuple(d))
        random.seed(s)
        got = util.augment([img], True, False)[0]              # rot off: one draw only
        assert np.array_equal(got, golden['parts/augment_flip_only_%d' % s]) and np.array_equal(got, ref_augment(img, d[0], False, False))
        follow = random.random()
        random.seed(s)
        random.random()
        assert follow == random.random()
    assert len(seen) >= 6


@pytest.mark.parametrize('mode', ['RGB', 'L', 'RGBA'])
def test_read_img_round_trips_a_png(tmp_path, mode):
    from PIL import Image
    import data.util as util
    rng = np.random.RandomState(5)
    a = rng.randint(0, 256, (9, 7) if mode == 'L' else (9, 7, len(mode))).astype(np.uint8)
    path = str(tmp_path / 'x.png')
    Image.fromarray(a).save(path)
    u8 = util.read_img_uint8(None, path)
    want = a[:, :, None] if mode == 'L' else a[:, :, 2::-1]
    assert u8.dtype == np.uint8 and u8.flags['C_CONTIGUOUS'] and np.array_equal(u8, want)
    img = util.read_img(None, path)
    assert img.dtype == np.float32 and np.array_equal(img, want.astype(np.float32) / 255.)


def test_image_paths(tmp_path):
    import data.util as util
    for name in ('b.png', 'a.jpg', 'notes.txt', 'c.PNG'):
        (tmp_path / name).write_bytes(b'')
    (tmp_path / 'sub').mkdir()
    (tmp_path / 'sub' / 'd.png').write_bytes(b'')
    env, paths = util.get_image_paths('img', str(tmp_path))
    assert env is None and [os.path.basename(p) for p in paths] == ['a.jpg', 'b.png', 'c.PNG']
    assert util.get_image_paths('img', None) == (None, None)
    assert util.is_image_file('x.bmp') and not util.is_image_file('x.gif')
    with pytest.raises((ImportError, NotImplementedError)):
        util.get_image_paths('lmdb', str(tmp_path))
    with pytest.raises(NotImplementedError):
        util.get_image_paths('zip', str(tmp_path))


# ---- LRHRDataset
@pytest.mark.parametrize('name', ['train_x4', 'train_x2', 'train_x4_y', 'val_x4'])
def test_items_equal_the_reference_under_the_recorded_seed(golden, tmp_path, name):
    from data.LRHR_dataset import LRHRDataset
    folder = write_set(golden, 'val' if name.startswith('val') else 'train', str(tmp_path / 'hr'))
    ds = LRHRDataset(case_opt(golden, name, folder))
    indices = golden['case/%s/indices' % name].tolist()
    assert len(ds) == len(set(indices))
    random.seed(int(golden['case/%s/seed' % name]))
    for j, i in enumerate(indices):
        item = ds[i]
        hr, lr = golden['case/%s/%d/HR' % (name, j)], golden['case/%s/%d/LR' % (name, j)]
        assert item['HR'].dtype == item['LR'].dtype == torch.float32
        assert item['HR_path'] == item['LR_path'] == os.path.join(folder, 'img_%02d.png' % i)
        assert tuple(item['HR'].shape) == hr.shape and tuple(item['LR'].shape) == lr.shape, (j, i)
        assert np.array_equal(item['HR'].numpy(), hr), (name, j, i)                # the crop origin and the augmentation: the draws
        err = np.abs(item['LR'].numpy() - lr).max()
        assert err <= ULP, (name, j, i, err)


def test_supplied_lr_images_are_cropped_not_synthesised(golden, tmp_path):
    from PIL import Image
    from data.LRHR_dataset import LRHRDataset
    import data.util as util
    folder = write_set(golden, 'train', str(tmp_path / 'hr'))
    lr_folder = str(tmp_path / 'lr')
    os.makedirs(lr_folder)
    rng = np.random.RandomState(9)
    lrs = []
    for i in range(5):
        h, w = golden['img/train/%d' % i].shape[:2]
        lrs.append(rng.randint(0, 256, (h // 4, w // 4, 3)).astype(np.uint8))
        Image.fromarray(lrs[-1]).save(os.path.join(lr_folder, 'img_%02d.png' % i))
    opt = dict(case_opt(golden, 'train_x4', folder), dataroot_LR=lr_folder)
    ds = LRHRDataset(opt)
    random.seed(3)
    item = ds[2]
    random.seed(3)
    rnd_h, rnd_w = random.randint(0, 56 // 4 - 6), random.randint(0, 44 // 4 - 6)
    d = [random.random() < 0.5 for _ in range(3)]
    want = ref_augment(f32(lrs[2][rnd_h:rnd_h + 6, rnd_w:rnd_w + 6]), *d).transpose(2, 0, 1)          # RGB file order = the item's channel order
    assert np.array_equal(item['LR'].numpy(), want) and item['LR_path'].startswith(lr_folder)
    hr = f32(golden['img/train/2'][4 * rnd_h:4 * rnd_h + 24, 4 * rnd_w:4 * rnd_w + 24])
    assert np.array_equal(item['HR'].numpy(), ref_augment(hr, *d).transpose(2, 0, 1))
    assert util.read_img(None, item['LR_path']).shape == (14, 11, 3)


def test_subset_file_lists_the_training_images(golden, tmp_path):
    from data.LRHR_dataset import LRHRDataset
    folder = write_set(golden, 'train', str(tmp_path / 'hr'))
    subset = tmp_path / 'subset.txt'
    subset.write_text('img_03.png\nimg_01.png\n')
    ds = LRHRDataset(dict(case_opt(golden, 'train_x4', folder), subset_file=str(subset)))
    assert [os.path.basename(p) for p in ds.paths_HR] == ['img_01.png', 'img_03.png'] and not ds.paths_LR
    with pytest.raises(NotImplementedError):
        LRHRDataset(dict(case_opt(golden, 'train_x4', folder), subset_file=str(subset), dataroot_LR=folder))


def test_refused_cases_raise_value_error(golden, tmp_path):
    from PIL import Image
    from data.LRHR_dataset import LRHRDataset
    folder = str(tmp_path / 'odd')
    os.makedirs(folder)
    rng = np.random.RandomState(2)
    Image.fromarray(rng.randint(0, 256, (42, 48, 3)).astype(np.uint8)).save(os.path.join(folder, 'not_a_multiple.png'))
    Image.fromarray(rng.randint(0, 256, (20, 48, 3)).astype(np.uint8)).save(os.path.join(folder, 'small.png'))
    Image.fromarray(rng.randint(0, 256, (48, 48, 3)).astype(np.uint8)).save(os.path.join(folder, 'fine.png'))
    ds = LRHRDataset(case_opt(golden, 'train_x4', folder))
    names = [os.path.basename(p) for p in ds.paths_HR]
    with pytest.raises(ValueError, match='not_a_multiple.png'):
        ds[names.index('not_a_multiple.png')]
    with pytest.raises(ValueError, match='small.png'):
        ds[names.index('small.png')]
    assert ds[names.index('fine.png')]['HR'].shape == (3, 24, 24)
    ds.random_scale_list = [1, 0.9]
    with pytest.raises(ValueError, match='fine.png'):
        ds[names.index('fine.png')]
    # the validation phase crops instead
    val = LRHRDataset(dict(case_opt(golden, 'val_x4', folder)))
    assert val[names.index('not_a_multiple.png')]['HR'].shape == (3, 40, 48)


# ---- the factories
def test_create_dataloader_defaults_to_the_torch_loader(golden, tmp_path):
    import data
    folder = write_set(golden, 'train', str(tmp_path / 'hr'))
    opt = case_opt(golden, 'train_x4', folder)
    assert 'device_batches' not in opt
    ds = data.create_dataset(opt)
    assert type(ds).__name__ == 'LRHRDataset'
    loader = data.create_dataloader(ds, opt)
    assert type(loader) is torch.utils.data.DataLoader and loader.batch_size == 4 and loader.drop_last and loader.dataset is ds
    val = data.create_dataloader(ds, dict(opt, phase='val'))
    assert type(val) is torch.utils.data.DataLoader and val.batch_size == 1 and not val.drop_last
    lr_only = data.create_dataset(dict(opt, mode='LR', dataroot_LR=folder, phase='test'))
    assert type(lr_only).__name__ == 'LRDataset' and lr_only[1]['LR'].shape == (3, 48, 40) and lr_only[1]['LR_path'].endswith('img_01.png')
    # device_batches is honoured for LRHR datasets only
    assert type(data.create_dataloader(lr_only, dict(opt, phase='test', device_batches=True))) is torch.utils.data.DataLoader


def test_create_dataset_rejects_unknown_modes(golden, tmp_path):
    import data
    for mode in ('LRHRseg_bg', 'JPEG', 'nothing'):
        with pytest.raises(NotImplementedError):
            data.create_dataset({'mode': mode, 'name': 'x'})


def test_device_taps_are_what_imresize_convolves_with():
    """esr_hip.data.downscale_taps against imresize itself: the formula of esr_data_lrhr_batch, in float64, on whole images"""
    from CEM.imresize_CEM import imresize
    from esr_hip.data import downscale_taps
    rng = np.random.RandomState(4)
    for sf in (2, 3, 4, 8):
        taps, pre = downscale_taps(sf)
        k, half = taps.shape[0], taps.shape[0] // 2
        assert k % 2 == 1 and 0 <= pre < sf
        x = rng.rand(5 * sf, 6 * sf)
        want = imresize(x, scale_factor=[1 / sf])
        p = np.pad(x, half, mode='edge')
        got = np.array([[(taps[::-1, ::-1] * p[pre + sf * i: pre + sf * i + k, pre + sf * j: pre + sf * j + k]).sum() for j in range(6)] for i in range(5)])
        assert np.abs(got - want).max() < 1e-14, sf
