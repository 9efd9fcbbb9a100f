"""DecompCNNModel — the explorable JPEG decoder's model wrapper (reference codes/models/DecompCNN_model.py), inference surface: feed_data /
test / Output_Batch / GetLatent / load with the reference's names, for the Y-channel (grey-scale) model and, with chroma_mode=True, the colour
model that contains it, and the colour model's Enforce_pair_Consistency (imprinting).  Training (is_train) is not part of this build.

Y model (8x8 blocks):
    compressed coefficients = JPEG['compressor'](image)            [B, 64, H/8, W/8], quantised with the image's QF table
    fake_H       = netG([Z | coefficients])                        the generator's coefficients: within +-0.5 of the quantised ones (Sigmoid - 0.5),
                                                                   so re-compressing the output gives the input back
    output_image = JPEG['extractor'](fake_H)                       [B, 1, H, W], 0...255
Colour model (16x16 blocks, 4:2:0: Cb and Cr keep their low 8x8 frequencies):
    y_channel_input = clamp(JPEG['extractor_Y'](netG_Y([Z | Y coefficients])), 0, 255)          the Y model, on the 8x8 grid
    var_Comp     = JPEG['compressor']([y_channel_input | Cb | Cr])  [B, 384, H/16, W/16]: Y's 256 coefficients unrounded | Cb, Cr low, rounded
    fake_H       = netG([Z resized to the 16x16 grid | var_Comp])   [B, 128, H/16, W/16]
    output_image = [y_channel_input | JPEG['extractor'](fake_H)]    [B, 3, H, W] YCbCr; Output_Batch(True) converts to RGB
On the GPU each generator runs on the DnCNN engine up to its last conv, and ONE esr_jpeg_extract / esr_jpeg16_extract launch applies the
sigmoid tail and produces fake_H and the image (esr_hip/jpeg.py); on the CPU it is the composition of the modules."""
import os
import re
from collections import OrderedDict
from copy import deepcopy

import numpy as np
import torch

import models.networks as networks
from esr_hip import jpeg as esr_jpeg
from esr_hip import jpeg_edit as esr_jpeg_edit
from JPEG_module.JPEG import JPEG
from .base_model import BaseModel
from .modules.loss import Latent_channels_desc_2_num_channels


def Tensor_YCbCR2RGB(image):
    """[B, 3, H, W] YCbCr in 0...1 -> RGB (reference utils/util.py:328-330).  ITU-R BT.601 studio-range YCbCr (Y 16...235, Cb, Cr 16...240) to
    full-range RGB: R = 255/219 (Y - 16) + 255/224 * 1.402 (Cr - 128), and so on, in the rounded form the reference carries (its matrix is per
    unit of an 8-bit value, hence the factor 255)."""
    mat = 255 * np.array([[0.00456621, 0.00456621, 0.00456621], [0, -0.00153632, 0.00791071], [0.00625893, -0.00318811, 0]]).transpose()
    mat = torch.from_numpy(mat).view(1, 3, 3, 1, 1).to(device=image.device, dtype=image.dtype)
    offset = torch.tensor([-222.921, 135.576, -276.836], device=image.device, dtype=image.dtype).view(1, 3, 1, 1) / 255
    return (mat * image.unsqueeze(1)).sum(2) + offset


class DecompCNNModel(BaseModel):
    def __init__(self, opt, accumulation_steps_per_batch=None, init_Fnet=None, init_Dnet=None, chroma_mode=False, **kwargs):
        super(DecompCNNModel, self).__init__(opt)
        if self.is_train:
            raise NotImplementedError('DecompCNNModel with is_train: this build runs the explorable JPEG decoder for inference and the Z search only')
        if chroma_mode and opt['scale'] != 16:
            raise NotImplementedError("DecompCNNModel(chroma_mode=True) with opt['scale'] = %r: the colour model works on 16x16 blocks; parse the "
                                      'options with parse(..., JPEG=True, chroma=True)' % (opt['scale'],))
        if not chroma_mode and opt['scale'] != 8:
            raise NotImplementedError("DecompCNNModel with opt['scale'] = %r: options parsed with chroma=True build the colour model, "
                                      'DecompCNNModel(opt, chroma_mode=True)' % (opt['scale'],))
        self.log_path = opt['path']['log']
        self.latent_input = opt['network_G']['latent_input'] if opt['network_G']['latent_input'] != 'None' else None
        if self.latent_input is not None:
            self.Z_size_factor = 1
        self.chroma_mode = bool(chroma_mode)
        self.cri_latent = None
        self.num_latent_channels = Latent_channels_desc_2_num_channels(opt['network_G']['latent_channels'])
        if self.latent_input is not None:
            assert isinstance(opt['network_G']['latent_channels'], int)
        self.step = 0
        cm = self.chroma_mode
        self.JPEG = {'compressor': JPEG(compress=True, chroma_mode=cm, downsample_or_quantize=True, block_size=self.opt['scale']),
                     'extractor': JPEG(compress=False, chroma_mode=cm, block_size=self.opt['scale'])}
        self.netG = networks.define_G(opt, num_latent_channels=self.num_latent_channels, chroma_mode=cm,
                                      no_high_freq_chroma_reconstruction=True).to(self.device)
        self.netG.eval()
        if cm:                                   # the colour model contains the Y model (reference :63-71, USE_Y_GENERATOR_4_CHROMA)
            netG_Y_opt = deepcopy(opt)
            for key, value in (netG_Y_opt['network_G_Y'] or {}).items():
                netG_Y_opt['network_G'][key] = value
            self.netG_Y = networks.define_G(netG_Y_opt, num_latent_channels=self.num_latent_channels, chroma_mode=False).to(self.device)
            self.netG_Y.eval()
            self.JPEG['compressor_Y'] = JPEG(compress=True, chroma_mode=False, downsample_or_quantize=True, block_size=8)
            self.JPEG['extractor_Y'] = JPEG(compress=False, chroma_mode=False, block_size=8)
        self.JPEG['non_quantized_compressor' + ('_Y' if cm else '')] = JPEG(compress=True, downsample_or_quantize=False, chroma_mode=False, block_size=8)
        if cm:                                   # (reference :114-117 with NO_HIGH_FREQ_CHROMA_RECONSTRUCTION)
            self.JPEG['non_quantized_compressor'] = JPEG(compress=True, downsample_or_quantize='downsample_only', chroma_mode=True,
                                                         block_size=self.opt['scale'])
        self.load()

    # ------------------------------------------------------------------ input
    def feed_data(self, data, need_GT=False, detach_Y=True, **kwargs):
        """data: 'QF' and either 'Uncomp' (an image: [B, 1, H, W], or [B, 3, H, W] YCbCr for the colour model, whose Y model then runs here —
        with gradients when detach_Y is False) or 'Comp' (coefficients; for the colour model the Y channel's [B, 64, H/8, W/8], followed by
        test(uncompressed_chroma=[B, 2, H, W])); optionally 'Z' on the Y grid [H/8, W/8].  The caller's tensors are left as they are (the
        reference writes the generated Y channel into data['Uncomp']).

        In place of 'QF', 'Q_table' [1 or 2, 8, 8]: the real-valued luminance (and, for the colour model, chrominance) tables of a JPEG file in
        the model's domain, with the file's coefficients as 'Comp' (esr_hip.jpeg_file.JpegFile.model_data); the colour model then takes the
        file's chroma coefficients through test(compressed_chroma=...)."""
        if data.get('Q_table') is not None:
            tables = data['Q_table']                 # to the host once: every module below takes the same arrays
            tables = tables.detach().cpu().numpy() if torch.is_tensor(tables) else np.asarray(tables)
            if tables.ndim != 3 or tables.shape[0] < (2 if self.chroma_mode else 1):
                raise ValueError("DecompCNNModel.feed_data: data['Q_table'] is [1, 8, 8] (luminance) or [2, 8, 8] (luminance, chrominance; needed "
                                 'by the colour model), got %s' % (tuple(tables.shape),))
            for module in self.JPEG.values():
                module.Set_File_Q_Table(tables[0], tables[1] if module.chroma_mode else None)
            self.QF = self.JPEG['extractor'].QF
        else:
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
            uncomp = data['Uncomp'].to(self.device)
            if self.chroma_mode and uncomp.size(1) == 3:                     # (reference :374-384)
                self.Prepare_Input(uncomp[:, :1], cur_Z)
                self.test_Y(detach=detach_Y, prevent_grads_calc=detach_Y)
                uncomp = torch.cat([self.y_channel_input, uncomp[:, 1:].to(self.y_channel_input.dtype)], 1)
            self.Prepare_Input(uncomp, latent_input=cur_Z)
        if need_GT:
            self.var_Uncomp = data['Uncomp'].to(self.device)

    def Prepare_Input(self, im_input, latent_input, compressed_input=False):
        if compressed_input:
            self.var_Comp = im_input
        else:
            if im_input.size(1) not in ((1, 3) if self.chroma_mode else (1,)):      # (the colour model also takes its Y channel alone)
                raise ValueError('DecompCNNModel: a %d-channel image for the %s model' % (im_input.size(1), 'colour' if self.chroma_mode else 'Y-channel'))
            if self.chroma_mode and im_input.size(1) == 1:
                self.var_Comp = self.JPEG['compressor_Y'](im_input)
            else:
                self.var_Comp = self.JPEG['compressor'](im_input)
        if latent_input is not None and latent_input.numel() > 0:
            latent_input = latent_input.to(device=self.var_Comp.device, dtype=self.var_Comp.dtype)
            if self.var_Comp.size()[2:] != latent_input.size()[2:]:
                # Z lives on the Y grid; the chroma generator's blocks are twice as large (reference :282-284)
                if not self.chroma_mode or [2 * v for v in self.var_Comp.shape[2:]] != list(latent_input.shape[2:]):
                    raise ValueError('Z of size %s for %s blocks' % (tuple(latent_input.shape[2:]), tuple(self.var_Comp.shape[2:])))
                latent_input = torch.nn.functional.interpolate(latent_input, size=self.var_Comp.shape[2:], mode='bilinear', align_corners=True)
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
        """The image closest to desired_im, coefficient by coefficient, among those that compress to what compressed_im compresses to
        (reference :316-334; what its JPEG GUI binds to imprinting): HWC RGB arrays in 0...1 -> HWC RGB array in 0...1, for the colour model.
        Y: the 64 coefficients of every 8x8 block of the desired Y plane are clamped to within 0.5 of the compressed image's quantised ones
        (esr_hip.jpeg_edit.consistent_plane); Cb, Cr: the low 8x8 of every 16x16 block likewise, the high frequencies stay the desired image's
        (consistent_chroma).  Like the reference, it needs JPEG['compressor_Y_non_quantized'] and JPEG['compressor_non_quantized'], which the
        model does not define (the reference's GUI adds them, GUI.py:2357-2360; their presence is all that is asked of them here: the modules'
        arithmetic is esr_hip.jpeg's): without them it raises NotImplementedError.

        What the reference computes, followed here as it computes it and pinned by tests/golden/jpeg_edit.npz:
          * it hands data.util.rgb2ycbcr a 0...255 float image where that function expects 0...1, so the planes it works on are
            255 (im M) + (16, 128, 128) / 255, not + (16, 128, 128): Y lies about 16 and Cb, Cr about 127.5 below their usual values (the matrix
            product runs in float64 and the result is cast to float32);
          * the compressed image is re-quantised on those shifted planes (only the DC coefficients differ from the usual ones);
          * at the end it applies Tensor_YCbCR2RGB to the 0...255 planes and divides by 255 afterwards, so the conversion's offset enters
            divided by 255 twice.  The two shifts cancel up to a constant of -2.4e-6 (R), -2.9e-6 (G), +1.1e-6 (B) in the 0...1 output,
            -(254 / 255) (mat (16, 128, 128) + offset) / 255: an image that is consistent already comes back within 1e-6 of itself.
          * one image at a time (the reference indexes image 0)."""
        missing = [k for k in ('compressor_Y_non_quantized', 'compressor_non_quantized') if k not in self.JPEG]
        if missing or not self.chroma_mode:
            raise NotImplementedError("Enforce_pair_Consistency: the reference's own version reads JPEG['compressor_Y_non_quantized'] and "
                                      "JPEG['compressor_non_quantized'], keys its model never defines (only its GUI adds them, GUI.py:2357-2360), on "
                                      "the colour model: add both to model.JPEG of a chroma_mode model first (missing here: %s)" % (
                                          missing or 'chroma_mode',))

        def im_2_tensor(im):
            # data.util.rgb2ycbcr(255 * im, only_y=False) on a float image: x 255 once more, the float64 product / 255 + offsets, then / 255
            im = np.asarray(im)
            if im.ndim != 3 or im.shape[2] != 3 or im.shape[0] % 16 or im.shape[1] % 16:
                raise ValueError('Enforce_pair_Consistency: HWC RGB images with H and W multiples of 16, got %s' % (im.shape,))
            x = (255 * im.astype(np.float32)) * np.float32(255.)
            ycc = (np.matmul(x, [[65.481, -37.797, 112.0], [128.553, -74.203, -93.786], [24.966, 112.0, -18.214]]) / 255.0 + [16, 128, 128]) / 255.
            return torch.from_numpy(np.ascontiguousarray(ycc.astype(np.float32).transpose((2, 0, 1)))).unsqueeze(0).to(self.device)
        compressed_im, desired_im = im_2_tensor(compressed_im), im_2_tensor(desired_im)
        if compressed_im.shape != desired_im.shape:
            raise ValueError('Enforce_pair_Consistency: images of %s and %s' % (tuple(compressed_im.shape[2:]), tuple(desired_im.shape[2:])))
        with torch.no_grad():
            compressed_Y_DCT = self.JPEG['compressor_Y'](compressed_im[:, :1])
            Y = esr_jpeg_edit.consistent_plane(desired_im[:, :1], compressed_Y_DCT, self.JPEG['compressor_Y']._table_on(self.device))
            compressed_chroma_DCT = self.JPEG['compressor'](compressed_im)
            chroma = esr_jpeg_edit.consistent_chroma(desired_im, compressed_chroma_DCT, self.JPEG['compressor']._table_on(self.device))
            # (the reference's final conversion, :334: the matrix on 0...255 values, its offset / 255, all of it / 255 again)
            rgb = torch.clamp(esr_jpeg_edit.ycbcr_to_rgb(255 * torch.cat([Y, chroma], 1)) / 255, 0, 1)
        return rgb[0].cpu().numpy().transpose((1, 2, 0))

    def _generate(self, G, extractor, chroma):
        """(generator's coefficients, their image) for the current model_input / var_Comp"""
        if getattr(G, 'output_layer', None) == 'Sigmoid' and G.on_kernels(self.model_input):
            # the generator's tail (sigmoid - 0.5 + quantised coefficients) and the extractor in one launch
            y = G.pre_output(self.model_input)
            return (esr_jpeg.extract16 if chroma else esr_jpeg.extract)(self.var_Comp, extractor._table_on(self.var_Comp.device), y)
        fake = self.Enforce_Consistency(self.var_Comp, G(self.model_input))
        return fake, extractor(fake)

    def test_Y(self, prevent_grads_calc=True, **kwargs):
        if prevent_grads_calc:
            with torch.no_grad():
                self.test_Y_(**kwargs)
        else:
            self.test_Y_(**kwargs)

    def test_Y_(self, detach=False):
        """the Y model on the current model_input = [Z | Y coefficients] (reference :711-715)"""
        self.netG_Y.eval()
        self.y_channel_input = torch.clamp(self._generate(self.netG_Y, self.JPEG['extractor_Y'], False)[1], 0, 255)
        if detach:
            self.y_channel_input = self.y_channel_input.detach()

    def test_(self, uncompressed_chroma=None, detach_Y=False, chroma_Z=None, compressed_chroma=None):
        """compressed_chroma [B or 1, 128, H/16, W/16]: a JPEG file's chroma coefficients in the model's domain (JpegFile.model_data) in the
        place of round(compress(uncompressed_chroma)) in var_Comp — they are exact, where the uncompressed_chroma route passes them through the
        compressor's rounding; Y's 256 coefficients come from the generated Y plane as always."""
        self.netG.eval()
        if compressed_chroma is not None:
            if not self.chroma_mode or uncompressed_chroma is not None:
                raise ValueError('DecompCNNModel.test(compressed_chroma=...) belongs to the colour model (chroma_mode=True), in place of uncompressed_chroma')
            if self.var_Comp.size(1) != 64:
                raise ValueError("DecompCNNModel.test(compressed_chroma=...) follows feed_data with the file's Y coefficients as 'Comp'")
            B, H, W = self.var_Comp.size(0), 8 * self.var_Comp.size(2), 8 * self.var_Comp.size(3)
            if compressed_chroma.dim() != 4 or tuple(compressed_chroma.shape[1:]) != (128, H // 16, W // 16) or compressed_chroma.size(0) not in (1, B) \
                    or H % 16 or W % 16:
                raise ValueError('DecompCNNModel.test: compressed_chroma %s for a Y plane of %d x %d (expected [%d or 1, 128, H/16, W/16])' % (
                    tuple(compressed_chroma.shape), H, W, B))
            self.test_Y(detach=detach_Y, prevent_grads_calc=False)
            y = self.y_channel_input
            compressed_chroma = compressed_chroma.to(device=y.device, dtype=y.dtype)
            latent = self.GetLatent() if chroma_Z is None else chroma_Z
            y_coef = self.JPEG['compressor'](torch.cat([y, y.new_zeros(B, 2, H, W)], 1))[:, :256]      # (Y is never rounded there)
            self.Prepare_Input(torch.cat([y_coef, compressed_chroma.expand(B, -1, -1, -1)], 1), latent, compressed_input=True)
        if uncompressed_chroma is not None:          # colour model fed with the Y coefficients (reference :720-724)
            if not self.chroma_mode:
                raise ValueError('DecompCNNModel.test(uncompressed_chroma=...) belongs to the colour model (chroma_mode=True)')
            self.test_Y(detach=detach_Y, prevent_grads_calc=False)   # (whether to keep gradients was decided by test())
            uncompressed_chroma = uncompressed_chroma.to(device=self.y_channel_input.device, dtype=self.y_channel_input.dtype)
            if uncompressed_chroma.size(0) != self.y_channel_input.size(0):
                uncompressed_chroma = uncompressed_chroma.repeat([self.y_channel_input.size(0)] + [1] * (uncompressed_chroma.ndimension() - 1))
            self.Prepare_Input(torch.cat([self.y_channel_input, uncompressed_chroma], 1), self.GetLatent() if chroma_Z is None else chroma_Z)
        self.fake_H, self.output_image = self._generate(self.netG, self.JPEG['extractor'], self.chroma_mode)
        if self.chroma_mode:
            self.output_image = torch.cat([self.y_channel_input, self.output_image], 1)

    def test(self, prevent_grads_calc=True, **kwargs):
        if prevent_grads_calc:
            with torch.no_grad():
                self.test_(**kwargs)
        else:
            self.test_(**kwargs)

    def Output_Image_0_1(self):
        """the output before the clamp to [0, 1], as Output_Batch(within_0_1=True) clamps it: RGB for the colour model"""
        if self.output_image.size(1) == 3:
            if self.output_image.is_cuda:            # one read and one write per value, no [B, 3, 3, H, W] broadcast (esr_ycbcr_rgb)
                return esr_jpeg_edit.ycbcr_to_rgb(self.output_image)
            return Tensor_YCbCR2RGB(self.output_image / 255)
        return self.output_image / 255

    def Output_Batch(self, within_0_1):
        if within_0_1:
            return torch.clamp(self.Output_Image_0_1(), 0, 1)
        return self.output_image

    def Return_Compressed(self, uncompressed):
        chroma_input = uncompressed.size(1) == 3
        assert self.chroma_mode or not chroma_input, 'Got a color image when model is not supporting it'
        if self.chroma_mode:
            Y_channel = self.JPEG['extractor_Y'](self.JPEG['compressor_Y'](uncompressed[:, :1]))
            if not chroma_input:
                return Y_channel
            return self.JPEG['extractor'](self.JPEG['compressor'](torch.cat([Y_channel, uncompressed[:, 1:]], 1)))
        return self.JPEG['extractor'](self.JPEG['compressor'](uncompressed))

    def get_current_visuals(self, need_Uncomp=True, entire_batch=False):
        out_dict = OrderedDict()
        pick = (lambda t: t.detach().float().cpu()) if entire_batch else (lambda t: t.detach()[0].float().cpu())
        out_dict['Comp'] = pick(self.var_Comp)
        out_dict['Decomp'] = pick(self.Output_Batch(within_0_1=False))
        if need_Uncomp:
            out_dict['Uncomp'] = pick(self.var_Uncomp)
        return out_dict

    def current_metrics(self, gt=None, crop_border=0):
        """{'psnr', 'ssim'}: float64 [B] on the model's device, of the last test()'s output against gt as test_JPEG.py scores them — both as the
        uint8 pictures util.tensor2img makes (esr_hip.jpeg_metrics.psnr_ssim: on the GPU nothing is copied or converted to memory).  gt: the
        ground truth in the output's form ([B or 1, C, H, W] in 0...255); the Y model defaults to the 'Uncomp' of feed_data(need_GT=True).  The
        colour model has to be given it: the Y plane it was fed is its own Y model's output, not the ground truth's."""
        from esr_hip import jpeg_metrics
        if gt is None:
            if self.chroma_mode:
                raise ValueError("current_metrics: the colour model needs gt (its input's Y plane is generated, keep the item's own 'Uncomp')")
            gt = self.var_Uncomp
        out = self.Output_Batch(within_0_1=False)
        psnr, ssim = jpeg_metrics.psnr_ssim(out, gt.to(out.device), 'YCbCr' if out.size(1) == 3 else 'Y', crop_border=crop_border)
        return {'psnr': psnr, 'ssim': ssim}

    def print_network(self):
        s, n = self.get_network_description(self.netG)
        print('Number of parameters in G: {:,d}'.format(n))

    def load(self, max_step=None, resume_train=None):
        """The newest '<step>_G.pth' under path.models (up to max_step) when there is one, else path.pretrained_model_G (reference :1007-1045);
        the colour model's netG_Y from path.Y_channel_model_G (:1049-1051)."""
        if self.chroma_mode and self.opt['path']['Y_channel_model_G'] is not None:
            print('loading model for G of channel Y [{:s}] ...'.format(self.opt['path']['Y_channel_model_G']))
            self.load_network(self.opt['path']['Y_channel_model_G'], self.netG_Y)
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
