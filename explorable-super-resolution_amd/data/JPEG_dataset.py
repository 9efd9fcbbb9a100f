"""Uncompressed images for the explorable JPEG decoder — the reference's codes/data/JPEG_dataset.py (JpegDataset), item by item, on PIL and
NumPy: the image as a Y plane, or as Y, Cb, Cr planes when 'chroma' is in opt['mode'], in 0...255, and the quality factor it is to be
compressed with.  The decoder compresses it itself (DecompCNNModel.feed_data), so there is no compressed file to read.

NumPy's and Python's generators are consulted in the reference's order — np.random.choice over the quality factors (and np.random.randint
inside a [lo, hi] range), then random.choice(random_scale_list) (over [1]: it consumes a value), rnd_h, rnd_w and augment's three — so after
seeding both, an item equals the reference's.  Outside the train phase nothing is drawn: the image is cropped to whole blocks of
8 * input_downsampling pixels and image n gets entry n of a quality-factor schedule laid over the set in __init__.

data.create_dataset does not build this class (mode 'JPEG' stays refused there): construct JpegDataset(opt) and hand it to
data.create_dataloader.  lmdb roots are refused as everywhere in this package; a random_scale_list other than [1] would need cv2.resize and
is refused with a ValueError naming the file."""
import os.path
import random

import numpy as np
import torch
import torch.utils.data as data

import data.util as util


class JpegDataset(data.Dataset):
    """Items {'Uncomp': float32 CHW in 0...255 (1 channel, or 3 YCbCr in chroma mode), 'Uncomp_path', 'QF'}."""

    def __init__(self, opt, specific_image=None):
        super(JpegDataset, self).__init__()
        self.opt = opt
        self.chroma_mode = 'chroma' in self.opt['mode']
        self.paths_Uncomp = None
        self.Uncomp_env = None
        self.block_size = 8
        if opt.get('input_downsampling') is not None:
            self.block_size *= opt['input_downsampling']
        self.quality_factors = opt['jpeg_quality_factor']
        if not isinstance(self.quality_factors, list):
            self.quality_factors = [self.quality_factors]
        self.QF_probs = opt.get('QF_probs')
        if self.QF_probs is None:
            self.QF_probs = np.ones([len(self.quality_factors)])
        else:
            assert len(self.QF_probs) == len(self.quality_factors)
            self.QF_probs = np.asarray(self.QF_probs, dtype=np.float64)       # (the reference divides in place and so needs an array here)
        self.QF_probs = self.QF_probs / self.QF_probs.sum()

        if opt.get('subset_file') is not None and opt['phase'] == 'train':       # image list from a text file
            with open(opt['subset_file']) as f:
                self.paths_Uncomp = sorted([os.path.join(opt['dataroot_Uncomp'], line.rstrip('\n')) for line in f])
            if opt.get('dataroot_LR') is not None:
                raise NotImplementedError('Now subset only supports generating LR on-the-fly.')
        else:
            self.Uncomp_env, self.paths_Uncomp = util.get_image_paths(opt['data_type'], opt['dataroot_Uncomp'], patch_size=opt.get('patch_size'))
        if opt.get('scales') is not None:               # how often the files of each of three scales are listed
            assert len(opt['scales']) == 3
            new_paths_list = []
            for scale_num, prob_ratio in enumerate(opt['scales']):
                if prob_ratio == 0:
                    continue
                new_paths_list += prob_ratio * [path for path in self.paths_Uncomp if '_scale%d_' % (scale_num) in path]
            self.paths_Uncomp = new_paths_list
        assert self.paths_Uncomp, 'Error: Uncomp path is empty.'
        if self.opt['phase'] == 'train':
            assert not self.opt['patch_size'] % (16 if self.chroma_mode else 8), \
                'Training for JPEG compression artifacts removal - Training images should have an integer number of 8x8 blocks.'
        else:
            self.per_index_QF = self._qf_schedule()
        self.random_scale_list = [1]

    def _qf_schedule(self):
        """The quality factor of every index outside training (reference :60-77): with at least as many entries as images, the entries that
        round(linspace(0, entries, images)) names, once each; otherwise every number once and every [lo, hi] range an equal share of the
        remaining images, spread as round(linspace(lo, hi - 1, share)), the first range (or the first entry) taking up the remainder."""
        n, qfs = len(self), self.quality_factors
        is_range = [isinstance(QF, list) for QF in qfs]
        if len(qfs) >= n:
            sampled_QFs = np.round(np.linspace(start=0, stop=len(qfs), num=n)).astype(int)
            per_range_len = [1 if (QF in sampled_QFs) else 0 for QF in qfs]
        else:
            num_exact_values = sum(not r for r in is_range)
            per_range_len = [((n - num_exact_values) // (len(qfs) - num_exact_values)) if r else 1 for r in is_range]
            first = int(np.argwhere(is_range)[0][0]) if any(is_range) else 0
            per_range_len[first] += n - sum(per_range_len)
        per_index_QF = []
        for QF, r, QF_range_len in zip(qfs, is_range, per_range_len):
            if r:
                per_index_QF += list(np.round(np.linspace(start=QF[0], stop=QF[1] - 1, num=QF_range_len)).astype(int))
            else:
                per_index_QF += [QF] * QF_range_len
        return per_index_QF

    def draw_QF(self):
        """the train phase's quality factor: an entry by QF_probs, a value of [lo, hi) when the entry is a range"""
        QF = self.quality_factors[np.random.choice(len(self.quality_factors), p=self.QF_probs)]
        if isinstance(QF, list):
            QF = np.random.randint(low=QF[0], high=QF[1])
        return QF

    def __getitem__(self, index):
        Uncomp_size = self.opt['patch_size']
        train = self.opt['phase'] == 'train'
        Uncomp_path = self.paths_Uncomp[index]
        img_Uncomp = util.read_img(self.Uncomp_env, Uncomp_path)
        if not train:
            img_Uncomp = util.modcrop(img_Uncomp, self.block_size)
        if img_Uncomp.shape[2] == 1:                      # a grey file
            img_Uncomp = np.repeat(img_Uncomp, 3, axis=2)
        img_Uncomp = 255 * util.channel_convert(img_Uncomp.shape[2], 'ycbcr' if self.chroma_mode else 'y', [img_Uncomp])[0]

        if train:
            QF = self.draw_QF()
            if list(self.random_scale_list) != [1]:
                raise ValueError('{:s}: random_scale_list {!r}: only [1] is supported (no bilinear resize in this package)'.format(
                    Uncomp_path, self.random_scale_list))
            random.choice(self.random_scale_list)         # [1]: the size stays, the draw is the reference's
            H, W, _ = img_Uncomp.shape
            rnd_h_Uncomp = random.randint(0, max(0, H - Uncomp_size))
            rnd_w_Uncomp = random.randint(0, max(0, W - Uncomp_size))
            img_Uncomp = img_Uncomp[rnd_h_Uncomp:rnd_h_Uncomp + Uncomp_size, rnd_w_Uncomp:rnd_w_Uncomp + Uncomp_size, :]
            img_Uncomp = util.augment([img_Uncomp], self.opt['use_flip'], self.opt['use_rot'])[0]
        else:
            QF = self.per_index_QF[index]

        img_Uncomp = torch.from_numpy(np.ascontiguousarray(np.transpose(img_Uncomp, (2, 0, 1)))).float()
        return {'Uncomp': img_Uncomp, 'Uncomp_path': Uncomp_path, 'QF': QF}

    def __len__(self):
        return len(self.paths_Uncomp)
