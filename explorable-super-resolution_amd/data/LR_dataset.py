"""LR images only, for the test phase — the reference's codes/data/LR_dataset.py (LRDataset).  Host route."""
import numpy as np
import torch
import torch.utils.data as data

import data.util as util


class LRDataset(data.Dataset):
    """Items {'LR', 'LR_path'[, 'kernel']}: the images of dataroot_LR as CHW RGB float tensors."""

    def __init__(self, opt, specific_image=None, kernel=None):
        super(LRDataset, self).__init__()
        assert specific_image is None, 'Unsupported here yet'
        self.opt = opt
        self.LR_env, self.paths_LR = util.get_image_paths(opt['data_type'], opt.get('dataroot_LR'))
        self.paths_kernel = None
        if isinstance(kernel, str) and kernel == 'estimated':          # a KernelGAN result next to every image
            self.paths_kernel = []
            for im_path in self.paths_LR:
                if 'img_' in im_path:
                    self.paths_kernel.append(im_path.replace('img', 'kernel_')[:-4] + '_x4.mat')
                else:
                    self.paths_kernel.append(im_path[:-4] + '_kernel_x4.mat')
        assert self.paths_LR, 'Error: LR paths are empty.'

    def __getitem__(self, index):
        LR_path = self.paths_LR[index]
        img_LR = util.read_img(self.LR_env, LR_path)
        C = img_LR.shape[2]
        if self.opt.get('color'):
            img_LR = util.channel_convert(C, self.opt['color'], [img_LR])[0]
        # channel order and layout of the tensor: RGB, CHW
        if img_LR.shape[2] == 3:
            img_LR = img_LR[:, :, [2, 1, 0]]
        img_LR = torch.from_numpy(np.ascontiguousarray(np.transpose(img_LR, (2, 0, 1)))).float()
        returned_dict = {'LR': img_LR, 'LR_path': LR_path}
        if self.paths_kernel is not None:
            import scipy.io
            returned_dict['kernel'] = scipy.io.loadmat(self.paths_kernel[index])['Kernel']
        return returned_dict

    def __len__(self):
        return len(self.paths_LR)
