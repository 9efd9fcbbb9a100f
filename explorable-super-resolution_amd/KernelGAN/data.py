"""Crops for kernel estimation — the reference's codes/KernelGAN/data.py (DataGenerator).

The image is read once; the centres of all max_iters crops for G (64 x 64) and for D (26 x 26) are drawn up front with probabilities that
follow the image's gradients.  Intended divergence: the reference adds the real crop's noise to a VIEW of the image, so the noise of every
iteration stays in the image; here the noise is added to the crop only."""
import numpy as np
import torch

from . import util


class DataGenerator:
    def __init__(self, conf, gan=None, g_input_shape=None, d_input_shape=None):
        self.g_input_shape = g_input_shape or conf.input_crop_size
        self.d_input_shape = d_input_shape or (gan.d_input_shape if gan is not None else (conf.input_crop_size - 12) // 2)
        im = np.asarray(conf.LR_image)
        if im.ndim != 3 or im.shape[2] != 3:
            raise ValueError('conf.LR_image must be an HWC RGB image')
        self.input_image = im / 255.
        self.shave_edges(conf.scale_factor, conf.real_image)
        self.in_rows, self.in_cols = self.input_image.shape[:2]
        if self.in_rows < self.g_input_shape or self.in_cols < self.g_input_shape:
            raise ValueError('the image (%d x %d after shaving) is smaller than one %d-pixel crop' % (self.in_rows, self.in_cols, self.g_input_shape))
        self.crop_indices_for_g, self.crop_indices_for_d = self.make_list_of_crop_indices(conf)

    def __len__(self):
        return 1

    def shave_edges(self, scale_factor, real_image):
        if not real_image:
            self.input_image = self.input_image[10:-10, 10:-10, :]
        sf = int(1 / scale_factor)
        h, w = self.input_image.shape[:2]
        self.input_image = self.input_image[:h - h % sf, :w - w % sf, :]

    def create_prob_maps(self, scale_factor):
        loss_map_big = util.create_gradient_map(self.input_image)
        loss_map_sml = util.create_gradient_map(util.imresize_cubic(self.input_image, scale_factor))
        prob_map_big = util.create_probability_map(loss_map_big, self.d_input_shape)
        prob_map_sml = util.create_probability_map(util.nn_interpolation(loss_map_sml, int(1 / scale_factor)), self.g_input_shape)
        return prob_map_big, prob_map_sml

    def make_list_of_crop_indices(self, conf):
        prob_map_big, prob_map_sml = self.create_prob_maps(conf.scale_factor)
        g = np.random.choice(a=len(prob_map_sml), size=conf.max_iters, p=prob_map_sml)
        d = np.random.choice(a=len(prob_map_big), size=conf.max_iters, p=prob_map_big)
        return g, d

    def get_top_left(self, size, for_g, idx):
        """The (even) top-left corner of the crop whose centre was drawn for iteration idx."""
        center = self.crop_indices_for_g[idx] if for_g else self.crop_indices_for_d[idx]
        row, col = int(center / self.in_cols), center % self.in_cols
        top, left = min(max(0, row - size // 2), self.in_rows - size), min(max(0, col - size // 2), self.in_cols - size)
        return int(top - top % 2), int(left - left % 2)

    def corner_table(self):
        """int32 [max_iters, 4]: (top_g, left_g, top_d, left_d) of every iteration — what the device gather reads."""
        n = len(self.crop_indices_for_g)
        return np.array([self.get_top_left(self.g_input_shape, True, i) + self.get_top_left(self.d_input_shape, False, i) for i in range(n)],
                        dtype=np.int32).reshape(n, 4)

    def next_crop(self, for_g, idx, device='cpu', dtype=torch.float32):
        size = self.g_input_shape if for_g else self.d_input_shape
        top, left = self.get_top_left(size, for_g, idx)
        crop = self.input_image[top:top + size, left:left + size, :]
        if not for_g:
            crop = crop + np.random.randn(*crop.shape) / 255.0
        return torch.as_tensor(np.transpose(crop, (2, 0, 1)) * 2.0 - 1.0, dtype=dtype, device=device).unsqueeze(0)

    def __getitem__(self, idx):
        return self.next_crop(True, idx), self.next_crop(False, idx)
