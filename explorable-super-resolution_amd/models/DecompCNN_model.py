"""DecompCNNModel — the explorable JPEG decoder's model wrapper (reference codes/models/DecompCNN_model.py), inference surface: feed_data /
test / Output_Batch / GetLatent / load with the reference's names, for the Y-channel (grey-scale) model.  Training (is_train), the chroma
model and Enforce_pair_Consistency are not part of this build.

    compressed coefficients = JPEG['compressor'](image)            [B, 64, H/8, W/8], quantised with the image's QF table
    fake_H       = netG([Z | coefficients])                        the generator's coefficients: within +-0.5 of the quantised ones (Sigmoid - 0.5),
                                                                   so re-compressing the output gives the input back
    output_image = JPEG['extractor'](fake_H)                       [B, 1, H, W], 0...255
On the GPU test() runs the DnCNN engine up to the last conv and ONE esr_jpeg_extract launch that applies the sigmoid tail, produces fake_H and
the image (esr_hip/jpeg.py); on the CPU it is the composition of the three modules."""
import os
import re
from collections import OrderedDict

import numpy as np
import torch

import models.networks as networks
from esr_hip import jpeg as esr_jpeg
from JPEG_module.JPEG import JPEG
from .base_model import BaseModel
from .modules.loss import Latent_channels_desc_2_num_channels


class DecompCNNModel(BaseModel):
    def __init__(self, opt, accumulation_steps_per_batch=None, init_Fnet=None, init_Dnet=None, chroma_mode=False, **kwargs):
        super(DecompCNNModel, self).__init__(opt)
        if self.is_train:
            raise NotImplementedError('DecompCNNModel with is_train: this build runs the explorable JPEG decoder for inference and the Z search only')
        if chroma_mode:
            raise NotImplementedError('DecompCNNModel(chroma_mode=True): this build runs the Y-channel (grey-scale) model only')
        self.log_path = opt['path']['log']
        self.latent_input = opt['network_G']['latent_input'] if opt['network_G']['latent_input'] != 'None' else None
        if self.latent_input is not None:
            self.Z_size_factor = 1
        self.chroma_mode = False
        self.cri_latent = None
        self.num_latent_channels = Latent_channels_desc_2_num_channels(opt['network_G']['latent_channels'])
        if self.latent_input is not None:
            assert isinstance(opt['network_G']['latent_channels'], int)
        self.step = 0
        self.JPEG = {'compressor': JPEG(compress=True, chroma_mode=False, downsample_or_quantize=True, block_size=self.opt['scale']),
                     'extractor': JPEG(compress=False, chroma_mode=False, block_size=self.opt['scale']),
                     'non_quantized_compressor': JPEG(compress=True, downsample_or_quantize=False, chroma_mode=False, block_size=8)}
        self.netG = networks.define_G(opt, num_latent_channels=self.num_latent_channels, chroma_mode=False).to(self.device)
        self.netG.eval()
        self.load()

    # ------------------------------------------------------------------ input
    def feed_data(self, data, need_GT=False, **kwargs):
        self.QF = data['QF']
        for module in self.JPEG.values():
            module.Set_Q_Table(self.QF)
        if self.latent_input is not None:
            input_size = np.array(data['Uncomp'].size()) if 'Uncomp' in data.keys() else [1, 1, 8, 8] * np.array(data['Comp'].size())
            DCT_dims = [int(v) for v in input_size[2:] // 8]
            if 'Z' in data.keys():
                cur_Z = data['Z']
            else:
                cur_Z = 2 * torch.rand([int(input_size[0]), self.num_latent_channels] + DCT_dims) - 1
            # the reference's broadcasting rules (DecompCNN_model.py:361-366)
            if isinstance(cur_Z, (int, float)) or len(cur_Z.shape) < 4 or (cur_Z.shape[2] == 1 and not torch.is_tensor(cur_Z)):
                cur_Z = cur_Z * np.ones([1, self.num_latent_channels] + DCT_dims)
            elif torch.is_tensor(cur_Z) and cur_Z.size(dim=2) == 1:
                cur_Z = cur_Z * torch.ones([1, 1] + DCT_dims, device=cur_Z.device)
            if not torch.is_tensor(cur_Z):
                cur_Z = torch.from_numpy(cur_Z)
        else:
            cur_Z = None
        if 'Comp' in data.keys():
            self.Prepare_Input(data['Comp'].to(self.device), latent_input=cur_Z, compressed_input=True)
        else:
            self.Prepare_Input(data['Uncomp'].to(self.device), latent_input=cur_Z)
        if need_GT:
            self.var_Uncomp = data['Uncomp'].to(self.device)

    def Prepare_Input(self, im_input, latent_input, compressed_input=False):
        if compressed_input:
            self.var_Comp = im_input
        else:
            if im_input.size(1) != 1:
                raise NotImplementedError('DecompCNNModel: a %d-channel image; this build runs the Y-channel (grey-scale) model only' % im_input.size(1))
            self.var_Comp = self.JPEG['compressor'](im_input)
        if latent_input is not None and latent_input.numel() > 0:
            if self.var_Comp.size()[2:] != latent_input.size()[2:]:
                raise ValueError('Z of size %s for %s blocks' % (tuple(latent_input.shape[2:]), tuple(self.var_Comp.shape[2:])))
            latent_input = latent_input.to(device=self.var_Comp.device, dtype=self.var_Comp.dtype)
            if latent_input.size(0) != self.var_Comp.size(0):
                latent_input = latent_input.expand(self.var_Comp.size(0), -1, -1, -1)
            self.model_input = torch.cat([latent_input, self.var_Comp], dim=1)
        else:
            self.model_input = 1 * self.var_Comp

    def GetLatent(self):
        return 1 * self.model_input[:, :self.num_latent_channels, ...]

    # ------------------------------------------------------------------ output
    def Enforce_Consistency(self, input_im, inconsostent_output):
        return inconsostent_output

    def Enforce_pair_Consistency(self, compressed_im, desired_im):
        raise NotImplementedError('Enforce_pair_Consistency belongs to the chroma model, which this build does not run')

    def test_(self):
        self.netG.eval()
        G = self.netG
        if getattr(G, 'output_layer', None) == 'Sigmoid' and G.on_kernels(self.model_input):
            # the generator's tail (sigmoid - 0.5 + quantised coefficients) and the extractor in one launch
            y = G.pre_output(self.model_input)
            self.fake_H, self.output_image = esr_jpeg.extract(self.var_Comp, self.JPEG['extractor']._table_on(self.var_Comp.device), y)
        else:
            self.fake_H = self.Enforce_Consistency(self.var_Comp, G(self.model_input))
            self.output_image = self.JPEG['extractor'](self.fake_H)

    def test(self, prevent_grads_calc=True, **kwargs):
        if prevent_grads_calc:
            with torch.no_grad():
                self.test_(**kwargs)
        else:
            self.test_(**kwargs)

    def Output_Batch(self, within_0_1):
        if within_0_1:
            return torch.clamp(self.output_image / 255, 0, 1)
        return self.output_image

    def Return_Compressed(self, uncompressed):
        assert uncompressed.size(1) != 3, 'Got a color image when model is not supporting it'
        return self.JPEG['extractor'](self.JPEG['compressor'](uncompressed))

    def get_current_visuals(self, need_Uncomp=True, entire_batch=False):
        out_dict = OrderedDict()
        pick = (lambda t: t.detach().float().cpu()) if entire_batch else (lambda t: t.detach()[0].float().cpu())
        out_dict['Comp'] = pick(self.var_Comp)
        out_dict['Decomp'] = pick(self.Output_Batch(within_0_1=False))
        if need_Uncomp:
            out_dict['Uncomp'] = pick(self.var_Uncomp)
        return out_dict

    def print_network(self):
        s, n = self.get_network_description(self.netG)
        print('Number of parameters in G: {:,d}'.format(n))

    def load(self, max_step=None, resume_train=None):
        """The newest '<step>_G.pth' under path.models (up to max_step) when there is one, else path.pretrained_model_G (reference :1007-1045)."""
        models_dir = self.opt['path']['models']
        step_of = lambda name: int(re.search(r'(\d)+(?=_G.pth)', name).group(0))
        own = sorted((n for n in (os.listdir(models_dir) if models_dir and os.path.isdir(models_dir) else []) if re.search(r'\d+_G\.pth$', n)), key=step_of)
        if max_step is not None:
            own = [n for n in own if step_of(n) <= max_step]
        if own:
            path = os.path.join(models_dir, own[-1])
            print('Testing model for G [{:s}] ...'.format(path))
            self.load_network(path, self.netG)
            self.gradient_step_num = step_of(own[-1])
            return
        load_path_G = self.opt['path']['pretrained_model_G'] if 'pretrained_model_G' in self.opt['path'] else None
        if load_path_G is not None:
            print('loading model for G [{:s}] ...'.format(load_path_G))
            self.load_network(load_path_G, self.netG)
