"""LR/HR image pairs on the host — the reference's codes/data/LRHR_dataset.py (LRHRDataset), item by item: with only HR images given the LR
image is CEM.imresize_CEM.imresize of the whole HR image; in the train phase a random patch_size crop and util.augment.  Python's `random`
is consulted in the reference's order (random_scale_list choice, rnd_h, rnd_w, augment's three), so a seed reproduces its items — and those of
esr_hip.data.DeviceLRHRLoader, which makes the same batches on the GPU from the same draws.

What the reference does through cv2.resize(INTER_LINEAR) and imresize_np is not restated; an image that would need them is refused with a
ValueError naming the file: in the train phase, a side that is no multiple of `scale` (when the LR image is synthesised) or below patch_size;
a random_scale_list other than [1]."""
import os.path
import random

import numpy as np
import torch
import torch.utils.data as data

import data.util as util
from CEM.imresize_CEM import imresize


class LRHRDataset(data.Dataset):
    """Items {'LR', 'HR', 'LR_path', 'HR_path'} of CHW RGB float tensors.  Without dataroot_LR the LR image is computed from the HR image;
    with it, file n of the sorted LR folder belongs to file n of the sorted HR folder."""

    def __init__(self, opt, specific_image=None, kernel=None):
        super(LRHRDataset, self).__init__()
        self.opt = opt
        self.paths_LR = None
        self.paths_HR = None
        self.LR_env = None
        self.HR_env = None
        self.kernel = kernel
        if opt.get('subset_file') is not None and opt['phase'] == 'train':       # image list from a text file
            with open(opt['subset_file']) as f:
                self.paths_HR = sorted([os.path.join(opt['dataroot_HR'], line.rstrip('\n')) for line in f])
            if opt.get('dataroot_LR') is not None:
                raise NotImplementedError('Now subset only supports generating LR on-the-fly.')
        else:
            self.HR_env, self.paths_HR = util.get_image_paths(opt['data_type'], opt.get('dataroot_HR'))
            self.LR_env, self.paths_LR = util.get_image_paths(opt['data_type'], opt.get('dataroot_LR'))
        if specific_image is not None:
            keep = lambda paths: [p for p in paths or [] if p.split('/')[-1].split('.')[0] == specific_image]      # noqa: E731
            self.paths_HR, self.paths_LR = keep(self.paths_HR), keep(self.paths_LR)
        assert self.paths_HR, 'Error: HR path is empty.'
        if self.paths_LR and self.paths_HR:
            assert len(self.paths_LR) == len(self.paths_HR), \
                'HR and LR datasets have different number of images - {}, {}.'.format(len(self.paths_LR), len(self.paths_HR))
        self.random_scale_list = [1]

    # ---- what both routes (this class and the device loader) decide per item, in the reference's order of draws
    def check_train_image(self, path, H, W):
        """the cases the reference would hand to cv2.resize / imresize_np"""
        scale, HR_size = self.opt['scale'], self.opt['patch_size']
        if not self.paths_LR and (H % scale or W % scale):
            raise ValueError('{:s}: {:d} x {:d} is no multiple of scale {:d}; the bilinear pre-resize of the reference is not part of this '
                             'package'.format(path, H, W, scale))
        if H < HR_size or W < HR_size:
            raise ValueError('{:s}: {:d} x {:d} is smaller than patch_size {:d}; the resize of small images (cv2.resize, imresize_np) is not '
                             'part of this package'.format(path, H, W, HR_size))

    def draw_random_scale(self, path):
        if list(self.random_scale_list) != [1]:
            raise ValueError('{:s}: random_scale_list {!r}: only [1] is supported (no bilinear pre-resize in this package)'.format(
                path, self.random_scale_list))
        return random.choice(self.random_scale_list)

    def draw_crop(self, H_LR, W_LR):
        """(rnd_h, rnd_w): the origin of the LR crop"""
        LR_size = self.opt['patch_size'] // self.opt['scale']
        rnd_h = random.randint(0, max(0, H_LR - LR_size))
        rnd_w = random.randint(0, max(0, W_LR - LR_size))
        return rnd_h, rnd_w

    def __getitem__(self, index):
        scale = self.opt['scale']
        HR_size = self.opt['patch_size']
        train = self.opt['phase'] == 'train'
        color = self.opt.get('color')

        HR_path, LR_path = self.paths_HR[index], None
        img_HR = util.read_img(self.HR_env, HR_path)
        if not train:
            img_HR = util.modcrop(img_HR, scale)
        if train:
            self.check_train_image(HR_path, img_HR.shape[0], img_HR.shape[1])
        if color:
            img_HR = util.channel_convert(img_HR.shape[2], color, [img_HR])[0]

        if self.paths_LR:
            LR_path = self.paths_LR[index]
            img_LR = util.read_img(self.LR_env, LR_path)
        else:                                           # no LR files: imresize of the whole HR image
            if train:
                self.draw_random_scale(HR_path)         # [1]: the size stays
            img_LR = imresize(img_HR, scale_factor=[1 / float(scale)], kernel=self.kernel)
            if img_LR.ndim == 2:
                img_LR = np.expand_dims(img_LR, axis=2)
        C = img_LR.shape[2]

        if train:
            H, W, C = img_LR.shape
            LR_size = HR_size // scale
            rnd_h, rnd_w = self.draw_crop(H, W)
            img_LR = img_LR[rnd_h:rnd_h + LR_size, rnd_w:rnd_w + LR_size, :]
            rnd_h_HR, rnd_w_HR = int(rnd_h * scale), int(rnd_w * scale)
            img_HR = img_HR[rnd_h_HR:rnd_h_HR + HR_size, rnd_w_HR:rnd_w_HR + HR_size, :]
            img_LR, img_HR = util.augment([img_LR, img_HR], self.opt['use_flip'], self.opt['use_rot'])

        if color:
            img_LR = util.channel_convert(C, color, [img_LR])[0]

        # channel order and layout of the tensors: RGB, CHW
        if img_HR.shape[2] == 3:
            img_HR = img_HR[:, :, [2, 1, 0]]
            img_LR = img_LR[:, :, [2, 1, 0]]
        img_HR = torch.from_numpy(np.ascontiguousarray(np.transpose(img_HR, (2, 0, 1)))).float()
        img_LR = torch.from_numpy(np.ascontiguousarray(np.transpose(img_LR, (2, 0, 1)))).float()

        if LR_path is None:
            LR_path = HR_path
        return {'LR': img_LR, 'HR': img_HR, 'LR_path': LR_path, 'HR_path': HR_path}

    def __len__(self):
        return len(self.paths_HR)
