"""LR/HR training batches made on the GPU (csrc/esr_data.hip) — the device route of data.LRHR_dataset.LRHRDataset.

* lrhr_batch(items, sf, taps, pre, patch, channel_map, out=None) -> (hr [B, Co, ph, pw], lr [B, Co, ph / sf, pw / sf]) fp32: the thin wrapper of
  esr_data_lrhr_batch.  `items`: _lib.DataItem structs (include/esr_hip.h: esr_data_item) whose pointers are device addresses of HWC uint8
  images; the table goes to the device as one pinned, asynchronous copy and the batch is one launch on the current stream.
* downscale_taps(sf, kernel=None) -> (taps [k, k] float64, pre): what CEM.imresize_CEM.imresize convolves with and where it samples, from
  imresize's own code (rot90(upscale kernel / sf^2, 2) and calc_strides).
* channel_map(color): None -> BGR->RGB, 'y' / 'gray' -> the 3->1 mixes of data.util.channel_convert.
* DeviceLRHRLoader(dataset, dataset_opt, device): an iterable over {'LR', 'HR', 'LR_path', 'HR_path'} batches with both tensors on the
  device.  Decoded images stay resident on the device as uint8, filled on first use and bounded by dataset_opt['device_cache_GB'] (oldest
  out first).  Python's `random` is consulted per item exactly as LRHRDataset.__getitem__ consults it, so after random.seed(s) a batch over
  indices [a, b, ...] equals the host dataset's items for these indices in this order (HR bit for bit, LR up to fp32 summation).  Batching
  follows data.create_dataloader: batch_size / use_shuffle / drop_last in the train phase, single images in order otherwise (the whole
  modcropped image is the crop, no augmentation)."""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import DataChannelMap, DataItem, check
from .act import stream_ptr

DEFAULT_CACHE_GB = 8.0


def channel_map(color):
    """the esr_data_channel_map of a dataset's `color` option"""
    from data import util
    m = DataChannelMap()
    if not color:
        m.mode = _lib.DATA_MAP_RGB
    elif color == 'y':
        m.mode, m.w, m.b, m.scale = _lib.DATA_MAP_MIX, (C.c_double * 3)(*util.Y_WEIGHTS_BGR), 16.0, 255.0
    elif color == 'gray':
        m.mode, m.w, m.b, m.scale = _lib.DATA_MAP_MIX, (C.c_double * 3)(*util.GRAY_WEIGHTS), 0.0, 1.0
    else:
        raise NotImplementedError('device batches: color %r (only None, \'y\' and \'gray\'; use the host loader)' % (color,))
    return m


def downscale_taps(sf, kernel=None):
    """(taps [k, k] float64, pre) of imresize(img, [1 / sf], kernel=kernel).  A kernel array replaces imresize's process-wide kernel of this
    scale factor, as it does in imresize itself."""
    from CEM.imresize_CEM import calc_strides, imresize
    taps = imresize(np.zeros((sf, sf)), scale_factor=[1 / float(sf)], kernel=kernel, return_upscale_kernel=True)
    pre, _ = calc_strides(None, 1 / float(sf))
    return np.ascontiguousarray(taps, dtype=np.float64), int(pre[0])


def lrhr_batch(items, sf, taps, pre, patch, channel_map, out=None, device=None):
    """One launch of esr_data_lrhr_batch.  items: a sequence of _lib.DataItem; taps: a device fp32 [k, k] tensor (None when every item brings
    its LR image); patch: the HR crop side, or (ph, pw); out: (hr, lr) to write into.  Returns (hr, lr)."""
    B = len(items)
    ph, pw = (patch, patch) if isinstance(patch, int) else patch
    device = torch.device(device) if device is not None else (taps.device if taps is not None else torch.device('cuda', torch.cuda.current_device()))
    if B < 1 or sf < 1 or ph % sf or pw % sf:
        raise _lib.EsrError('lrhr_batch: %d items, patch %d x %d, sf %d' % (B, ph, pw, sf))
    if taps is not None and not (taps.is_cuda and taps.dtype == torch.float32 and taps.is_contiguous() and taps.dim() == 2 and taps.size(0) == taps.size(1)):
        raise _lib.EsrError('lrhr_batch: taps is a contiguous square fp32 tensor on the device')
    k = taps.size(0) if taps is not None else 1
    Co = 1 if channel_map.mode == _lib.DATA_MAP_MIX else int(items[0].channels)
    with torch.cuda.device(device):
        host = torch.empty(B * C.sizeof(DataItem), dtype=torch.uint8, pin_memory=True)
        table = (DataItem * B).from_buffer(host.numpy())
        for i, it in enumerate(items):
            table[i] = it
        dev = torch.empty_like(host, device=device)
        dev.copy_(host, non_blocking=True)
        if out is None:
            hr = torch.empty(B, Co, ph, pw, dtype=torch.float32, device=device)
            lr = torch.empty(B, Co, ph // sf, pw // sf, dtype=torch.float32, device=device)
        else:
            hr, lr = out
            for t, shape in ((hr, (B, Co, ph, pw)), (lr, (B, Co, ph // sf, pw // sf))):
                if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
                    raise _lib.EsrError('lrhr_batch: out is contiguous fp32 %s on the device, got %s' % (shape, tuple(t.shape)))
        check(_lib.lib.esr_data_lrhr_batch(C.addressof(table), dev.data_ptr(), B, sf, taps.data_ptr() if taps is not None else None, k, pre, ph, pw,
                                           C.byref(channel_map), hr.data_ptr(), lr.data_ptr(), stream_ptr()), 'esr_data_lrhr_batch')
    return hr, lr


class DeviceLRHRLoader:
    """Batches of an LRHRDataset made on the GPU; see the module text."""

    def __init__(self, dataset, dataset_opt, device=None):
        self.dataset = dataset
        self.opt = dataset_opt
        self.device = torch.device(device if device is not None else 'cuda')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.train = dataset_opt['phase'] == 'train'
        self.sf = int(dataset_opt['scale'])
        self.batch_size = int(dataset_opt['batch_size']) if self.train else 1
        self.shuffle = bool(dataset_opt['use_shuffle']) if self.train else False
        self.map = channel_map(dataset_opt.get('color'))
        self.taps, self.pre = None, 0
        if not dataset.paths_LR:
            taps, self.pre = downscale_taps(self.sf, dataset.kernel)
            self.taps = torch.from_numpy(taps.astype(np.float32)).to(self.device)
        gb = dataset_opt.get('device_cache_GB')
        self.cache_bytes = int((DEFAULT_CACHE_GB if gb is None else float(gb)) * 2 ** 30)
        self._cache = collections.OrderedDict()       # index -> (HR uint8 [H, W, C], LR uint8 or None), oldest first
        self._cached = 0

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.train else n

    # ---- resident images
    def _image(self, index):
        from data import util
        hit = self._cache.get(index)
        if hit is not None:
            return hit
        ds = self.dataset
        up = lambda a: torch.from_numpy(a).to(self.device, non_blocking=False)          # noqa: E731
        hr = up(util.read_img_uint8(ds.HR_env, ds.paths_HR[index]))
        lr = up(util.read_img_uint8(ds.LR_env, ds.paths_LR[index])) if ds.paths_LR else None
        entry = (hr, lr)
        self._cache[index] = entry
        self._cached += hr.numel() + (lr.numel() if lr is not None else 0)
        while self._cached > self.cache_bytes and len(self._cache) > 1:                 # (a batch in the making holds its own references)
            _, (h, l) = self._cache.popitem(last=False)
            self._cached -= h.numel() + (l.numel() if l is not None else 0)
        return entry

    def _item(self, index):
        """(esr_data_item, the tensors it points into) for one index, with LRHRDataset.__getitem__'s draws in its order"""
        ds, sf = self.dataset, self.sf
        hr, lr = self._image(index)
        path = ds.paths_HR[index]
        H, W, Cs = hr.shape
        it = DataItem(hr=hr.data_ptr(), lr=lr.data_ptr() if lr is not None else None, stride=W, channels=Cs)
        if lr is not None:
            if lr.size(2) != Cs:
                raise ValueError('%s: %d channels, its LR image has %d' % (path, Cs, lr.size(2)))
            it.lr_H, it.lr_W, it.lr_stride = lr.size(0), lr.size(1), lr.size(1)
        if not self.train:
            it.H, it.W = H - H % sf, W - W % sf                   # util.modcrop, as the logical size
            return it, (hr, lr), (it.H, it.W)
        ds.check_train_image(path, H, W)
        it.H, it.W = H, W
        if lr is None:
            ds.draw_random_scale(path)
        rnd_h, rnd_w = ds.draw_crop(*((H // sf, W // sf) if lr is None else (lr.size(0), lr.size(1))))
        from data import util
        hflip, vflip, rot90 = util.draw_augment(self.opt['use_flip'], self.opt['use_rot'])
        it.y0, it.x0 = rnd_h * sf, rnd_w * sf
        it.flags = (_lib.DATA_HFLIP if hflip else 0) | (_lib.DATA_VFLIP if vflip else 0) | (_lib.DATA_TRANSPOSE if rot90 else 0)
        p = int(self.opt['patch_size'])
        return it, (hr, lr), (p, p)

    def batch(self, indices):
        """the batch of these dataset indices, in this order"""
        items, held, patch = [], [], None
        for i in indices:
            it, tensors, size = self._item(i)
            if patch is not None and size != patch:
                raise ValueError('device batches: images of one batch differ in size (%s, %s)' % (patch, size))
            patch = size
            items.append(it)
            held.append(tensors)                       # alive until the launch is enqueued, whatever the cache evicts meanwhile
        hr, lr = lrhr_batch(items, self.sf, self.taps, self.pre, patch, self.map, device=self.device)
        ds = self.dataset
        hr_paths = [ds.paths_HR[i] for i in indices]
        return {'LR': lr, 'HR': hr, 'LR_path': [ds.paths_LR[i] for i in indices] if ds.paths_LR else list(hr_paths), 'HR_path': hr_paths}

    def __iter__(self):
        n = len(self.dataset)
        order = torch.randperm(n).tolist() if self.shuffle else list(range(n))
        for s in range(0, len(self) * self.batch_size, self.batch_size):
            yield self.batch(order[s:s + self.batch_size])
