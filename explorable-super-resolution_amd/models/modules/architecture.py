"""RRDBNet — the ESRGAN-style generator of the reference (codes/models/modules/architecture.py:228-302) with the
same constructor, attributes, module tree and state_dict keys, executed by the gfx950 engine (esr_hip/engine.py).

Discriminator_VGG_128 (architecture.py:446-508), the other half of the configs[2] training step, is a stock-PyTorch module (MIOpen
convolutions, BatchNorm, Linear): the WGAN-GP penalty differentiates it twice, which autograd does for stock ops.

VGGFeatureExtractor (architecture.py:658-705), the perceptual loss's network, is a stock module tree (torchvision's `features` layout and
state_dict keys) whose GPU forward and input gradient run on the library's kernels (esr_hip/vgg.py).  The other discriminators / feature
extractors of the reference's architecture.py are outside this build.
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import block as B
from esr_hip.engine import RRDBEngine
from esr_hip import vgg as esr_vgg
from esr_hip import dncnn as esr_dncnn


class RRDBNet(nn.Module):
    def __init__(self, in_nc, out_nc, nf, nb, gc=32, upscale=4, norm_type=None, act_type='leakyrelu', mode='CNA',
                 upsample_mode='upconv', latent_input=None, num_latent_channels=None):
        super(RRDBNet, self).__init__()
        self.latent_input = None
        num_latent_channels = 0 if num_latent_channels is None else num_latent_channels   # (the reference raises TypeError on None)
        num_latent_channels_HR = 0
        if num_latent_channels > 0:
            self.latent_input = latent_input
            num_latent_channels_HR = 1 * num_latent_channels
            if 'HR_rearranged' in latent_input:
                num_latent_channels *= upscale ** 2
        self.num_latent_channels = 1 * num_latent_channels
        self.upscale = upscale
        n_upscale = int(math.log(upscale, 2))
        if upscale == 3:
            n_upscale = 1
        if latent_input is not None:
            in_nc += num_latent_channels
        if latent_input is None or 'all_layers' not in latent_input:
            num_latent_channels, num_latent_channels_HR = 0, 0
        if norm_type is not None:
            raise NotImplementedError('RRDBNet with normalisation layers is not on the RRDB+CEM path (reference default: norm_type=null)')
        if act_type != 'leakyrelu' or mode != 'CNA':
            # the fused kernels implement conv -> LeakyReLU(0.2) (what define_G hard-wires, networks.py:97-99) and nothing else
            raise NotImplementedError("RRDBNet(act_type=%r, mode=%r): the HIP engine implements act_type='leakyrelu', mode='CNA' only" % (act_type, mode))
        if nf < 16 or nf % 16 or (nf > 64 and nf % 64) or out_nc < 1 or in_nc < 1 or (upsample_mode == 'pixelshuffle' and nf != 64):
            # The residual stream is nf / 8 channel groups of the activation layout, a dense block ONE (nf / 8 + 16)-group buffer; nf = 16, 32, 48, 64
            # and 128, 192, ... run the same launch plan (round 6; reference architecture.py:228-230 takes any nf, every options file it ships uses
            # 64).  Multiples of 16: a K chunk of the MFMA contraction is two channel groups, and the mirrored data gradient concatenates the layers'
            # gradients chunk by chunk.  Above 64: multiples of 64 — a launch produces its output in 64-channel slices (esr_conv3x3_desc.cout > 64).
            # The pixel-shuffle store orders its rows in blocks of 64 channels: nf = 64 only.
            raise NotImplementedError("RRDBNet(nf=%r, upsample_mode=%r): the HIP engine runs nf = 16, 32, 48, 64, 128, 192, ... (the reference's options files use 64; "
                                      "gc is 32 — the reference ignores the argument too); pixel-shuffle upsamplers nf = 64 only" % (nf, upsample_mode))

        fea_conv = B.conv_block(in_nc, nf, kernel_size=3, norm_type=None, act_type=None, return_module_list=True)
        # NB: like the reference (architecture.py:250) the `gc` argument is ignored: growth channels are 32.
        rb_blocks = [B.RRDB(nf, kernel_size=3, gc=32, stride=1, bias=True, pad_type='zero', norm_type=norm_type, act_type=act_type,
                            mode='CNA', latent_input_channels=num_latent_channels) for _ in range(nb)]
        LR_conv = B.conv_block(nf + num_latent_channels, nf, kernel_size=3, norm_type=norm_type, act_type=None, mode=mode,
                               return_module_list=True)
        if upsample_mode == 'upconv':
            upsample_block = B.upconv_blcok
        elif upsample_mode == 'pixelshuffle':
            upsample_block = B.pixelshuffle_block
        else:
            raise NotImplementedError('upsample mode [{:s}] is not found'.format(upsample_mode))
        if upscale == 3:
            # the reference builds a bare Sequential here and then fails to concatenate it (architecture.py:260-261,271);
            # wrapping it in a list is the evident intent
            upsampler = [upsample_block(nf, nf, 3, act_type=act_type)]
        else:
            upsampler = [upsample_block(nf, nf, act_type=act_type) for _ in range(n_upscale)]
        HR_conv0 = B.conv_block(nf + num_latent_channels_HR, nf, kernel_size=3, norm_type=None, act_type=act_type, return_module_list=True)
        HR_conv1 = B.conv_block(nf + num_latent_channels_HR, out_nc, kernel_size=3, norm_type=None, act_type=None, return_module_list=True)
        self.model = nn.ModuleList(fea_conv + [B.ShortcutBlock(B.sequential(*(rb_blocks + LR_conv), return_module_list=True),
                                                               latent_input_channels=num_latent_channels, use_module_list=True)]
                                   + upsampler + HR_conv0 + HR_conv1)
        self.upsample_mode = upsample_mode
        self.nb, self.nf, self.out_nc = nb, nf, out_nc
        self._lat_all_layers = num_latent_channels
        self._engine = None

    # ---- engine plumbing
    @property
    def engine(self):
        if self._engine is None:
            self._engine = RRDBEngine(self)
        return self._engine

    def set_precision(self, precision):
        """Operand scheme of the MFMA kernels (fp32 accumulate and fp32 I/O in all of them):
        'split'  default: bf16 hi+lo weights x bf16 hi+lo activations, 3 MFMAs per product, fp32-class forward AND gradients;
        'mixed'  fp16: residual stream stored hi+lo, hi+lo operands in the six convs outside the dense blocks, one-plane operands inside
                 them; forward within 3e-5..3e-4 of fp32 at 0.55x the time of split; back-propagates with power-of-two gradient scaling
                 (input gradient ~1e-5, weight gradients ~3e-3 of fp32): inference, Z search, optionally training;
        'f16x2'  fp16 weights x fp16 hi+lo activations, 2 MFMAs, ~5e-4 on RRDB-23, inference only;
        'f16' / 'bf16'  one plane, one MFMA; 'f16' (1.6e-3) is inference only, 'bf16' (1.3e-2) also trains."""
        assert precision in ('split', 'mixed', 'f16x2', 'f16', 'bf16')
        self.engine.set_precision(precision)

    def check_range(self, wait=True):
        """fp16 precisions ('mixed', 'f16x2', 'f16'): raise EsrError if a forward since the last check stored activations that reached fp16's last
        binade or are not finite, naming the first such layer (esr_hip/engine.py: RRDBEngine.check_range; the kernels report it without an
        extra pass).  A forward looks at what has arrived by itself, without synchronising; call this where a result is consumed."""
        if self._engine is not None:
            self._engine.check_range(wait=wait)

    def invalidate_packs(self):
        """Call after editing parameters through `.data` (such writes bypass torch's version counters, which is what the engine watches)."""
        if self._engine is not None:
            self._engine.invalidate()

    def forward(self, x, pad=0):
        """x: [B, num_latent_channels*upscale^2 + 3, h, w] (Z packed by the raw view of SRRaGAN_model.py:233, LR image last).
        `pad` > 0 evaluates the generator on the replicate-padded input (CEM eval mode, CEMnet.py:286-295) without
        materialising the padded tensors."""
        if self.latent_input is not None and 'HR_downscaled' not in self.latent_input:
            if 'HR_rearranged' in self.latent_input and 'all_layers' in self.latent_input:
                raise Exception('Unsupported yet')          # same behaviour as architecture.py:295
            raise NotImplementedError("latent_input '%s': only '<all_layers|first_layer>_HR_downscaled' is implemented" % self.latent_input)
        return self.engine.forward(x, pad=pad)


class Discriminator_VGG_128(nn.Module):
    """VGG-style critic (reference architecture.py:446-508): 3x3 stride-1 convs alternating with 4x4 stride-2 convs, widths
    nf, nf, 2nf, 2nf, 4nf, 4nf, 8nf x4, BatchNorm + LeakyReLU(0.2) after every conv but the first (no norm there); the first `nb` of the
    ten conv blocks are kept; `num_2_strides` of the five 4x4 convs stride (the rest run at stride 1).  With all five strides the
    classifier is Linear(8nf * s^2, 100) -> LeakyReLU -> Linear(100, 1) on the s x s feature map (s = 4 for 128x128 inputs); with fewer
    it is a "patch" critic: conv 8x8 (no padding) -> LeakyReLU -> conv 1x1.  `features` is ONE flat nn.Sequential and `classifier` a
    3-element one, so state_dict keys and their order are the reference's (features.0.weight, features.2.weight, features.3.weight ...)."""

    def __init__(self, in_nc, base_nf, norm_type='batch', act_type='leakyrelu', mode='CNA', input_patch_size=128, num_2_strides=5, nb=10):
        super(Discriminator_VGG_128, self).__init__()
        assert num_2_strides <= 5, 'Can be modified by adding more stridable layers, if needed.'
        if mode != 'CNA' or act_type != 'leakyrelu' or norm_type not in ('batch', 'instance', None):
            raise NotImplementedError('Discriminator_VGG_128(norm_type=%r, act_type=%r, mode=%r)' % (norm_type, act_type, mode))
        self.num_2_strides = 1 * num_2_strides
        widths = [base_nf, base_nf, 2 * base_nf, 2 * base_nf, 4 * base_nf, 4 * base_nf, 8 * base_nf, 8 * base_nf, 8 * base_nf, 8 * base_nf]
        layers, cin, size, strides_left = [], in_nc, float(input_patch_size), num_2_strides
        for i, cout in enumerate(widths):
            k, stride = 3, 1
            if i % 2 == 1:                     # the down-sampling slots: 4x4, stride 2 while strides remain
                k, stride = 4, (2 if strides_left > 0 else 1)
                size = np.ceil((size - 1) / stride)
                strides_left -= 1
            block = [nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=(k - 1) // 2)]
            if i > 0 and norm_type is not None:
                block.append(B.norm(norm_type, cout))
            block.append(nn.LeakyReLU(0.2, True))
            layers.append(block)
            cin = cout
        layers = layers[:nb]
        self.features = nn.Sequential(*[m for block in layers for m in block])
        self.last_FC_layers = self.num_2_strides == 5
        if self.last_FC_layers:
            self.classifier = nn.Sequential(nn.Linear(base_nf * 8 * int(size) ** 2, 100), nn.LeakyReLU(0.2, True), nn.Linear(100, 1))
        else:
            feat = widths[len(layers) - 1]
            hidden = min(100, feat)
            c0 = [nn.Conv2d(feat, hidden, kernel_size=8, stride=1, padding=0)] + ([B.norm(norm_type, hidden)] if norm_type else []) + [nn.LeakyReLU(0.2, True)]
            c1 = [nn.Conv2d(hidden, 1, kernel_size=1, stride=1, padding=0)] + ([B.norm(norm_type, 1)] if norm_type else []) + [nn.LeakyReLU(0.2, True)]
            self.classifier = nn.Sequential(nn.Sequential(*c0), nn.LeakyReLU(0.2, False), nn.Sequential(*c1))

    def forward(self, x):
        x = self.features(x)
        if self.last_FC_layers:
            x = x.reshape(x.size(0), -1)          # (NCHW order also when the features ran channels_last)
        return self.classifier(x)


# torchvision's file names of the ImageNet weights (torch.hub cache, <hub dir>/checkpoints/)
VGG_HUB_FILES = {'vgg11': 'vgg11-8a719046.pth', 'vgg13': 'vgg13-19584684.pth', 'vgg16': 'vgg16-397923af.pth', 'vgg19': 'vgg19-dcbb9e9d.pth'}


def vgg_weight_sources(arch, pretrained_path=None):
    """The places VGGFeatureExtractor takes its weights from, in order, when no state_dict is passed: the options' pretrained_model_F, then
    torchvision's file in the torch hub cache.  Nothing is ever downloaded."""
    import torch.hub
    return [p for p in (pretrained_path, os.path.join(torch.hub.get_dir(), 'checkpoints', VGG_HUB_FILES.get(arch, arch + '.pth'))) if p]


class VGGFeatureExtractor(nn.Module):
    """Perceptual-loss network (reference architecture.py:658-705): torchvision's VGG `features` cut after index `feature_layer` (34: conv5_4
    of VGG19, before its ReLU), frozen, behind the ImageNet input normalisation.  `features` is a stock Sequential of Conv2d / ReLU /
    MaxPool2d and `mean` / `std` are buffers, so state_dict keys are the reference's (features.<i>.weight / bias, mean, std).

    Weights (torchvision is not part of this build, and nothing is downloaded), first found wins: the `state_dict` keyword (the reference's own;
    a torchvision VGG state_dict or this module's, 'module.' prefixes dropped), `pretrained_path` (define_F passes the options'
    path.pretrained_model_F: a torchvision-format .pth), torchvision's vgg*.pth in the torch hub cache.

    On the GPU the forward and its input gradient run on the library's kernels (esr_hip/vgg.py; set_precision picks 'split' — fp32-class, the
    default — or 'bf16'); CPU tensors run the stock modules, as Discriminator_VGG_128 does."""

    def __init__(self, feature_layer=34, use_bn=False, use_input_norm=True, device=torch.device('cpu'), state_dict=None, arch='vgg19',
                 arch_config='', pretrained_path=None, **kwargs):
        super(VGGFeatureExtractor, self).__init__()
        if arch == 'SegNetAE':
            raise NotImplementedError('VGGFeatureExtractor(arch=SegNetAE): the SegNet auto-encoder is not part of this build')
        if use_bn:
            raise NotImplementedError('VGGFeatureExtractor(use_bn=True): the batch-norm VGG variants are not part of this build')
        if arch_config != '':
            raise NotImplementedError('VGGFeatureExtractor(arch_config=%r): the RandomPooling model modifications are not part of this build' % (arch_config,))
        table = esr_vgg.layer_table(arch, feature_layer)
        layers = []
        for entry in table:
            if entry[0] == 'conv':
                layers.append(nn.Conv2d(entry[1], entry[2], kernel_size=3, padding=1))
            elif entry[0] == 'relu':
                layers.append(nn.ReLU(inplace=True))
            else:
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        self.features = nn.Sequential(*layers)
        self.arch = arch
        self._load_weights(state_dict, pretrained_path)
        self.use_input_norm = use_input_norm
        if self.use_input_norm:
            self.register_buffer('mean', torch.Tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
            self.register_buffer('std', torch.Tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))
        for v in self.features.parameters():
            v.requires_grad = False
        self.to(device)
        self._engine = None
        self._precision = 'split'

    def _load_weights(self, state_dict, pretrained_path):
        if state_dict is None:
            sources = vgg_weight_sources(self.arch, pretrained_path)
            found = [p for p in sources if os.path.isfile(p)]
            if not found:
                raise FileNotFoundError('VGGFeatureExtractor(%s): no weights. Looked for (1) the state_dict= keyword, (2) the options\' '
                                        'path.pretrained_model_F (%s), (3) the torch hub cache file %s. Nothing is downloaded: put torchvision\'s '
                                        '%s there or pass one of the others.' % (self.arch, pretrained_path or 'not set', sources[-1],
                                                                                 VGG_HUB_FILES.get(self.arch, self.arch + '.pth')))
            state_dict = torch.load(found[0], map_location='cpu')
        state_dict = {k.replace('module.', ''): v for k, v in state_dict.items()}
        own = self.features.state_dict()
        missing = ['features.' + k for k in own if 'features.' + k not in state_dict]
        if missing:
            raise KeyError('VGGFeatureExtractor(%s): the weights lack %s' % (self.arch, ', '.join(missing)))
        with torch.no_grad():
            for k, v in own.items():
                src = state_dict['features.' + k]
                if tuple(src.shape) != tuple(v.shape):
                    raise ValueError('VGGFeatureExtractor: features.%s has shape %s, expected %s' % (k, tuple(src.shape), tuple(v.shape)))
                v.copy_(src)

    @property
    def engine(self):
        if self._engine is None:
            self._engine = esr_vgg.VGGEngine(self.features, precision=self._precision)
        return self._engine

    def set_precision(self, precision):
        """'split' (default): bf16 hi+lo operands, fp32-class features and gradients; 'bf16': one plane, one MFMA per product."""
        assert precision in ('split', 'bf16')
        self._precision = precision
        if self._engine is not None:
            self._engine.set_precision(precision)

    def forward(self, x):
        if x.is_cuda:
            eng = self.engine
            eng.mean, eng.std = (self.mean, self.std) if self.use_input_norm else (None, None)
            return esr_vgg.vgg_forward(eng, x)
        if self.use_input_norm:
            x = (x - self.mean) / self.std
        return self.features(x)


class DnCNN(nn.Module):
    """Generator of the explorable JPEG decoder (reference architecture.py:109-214, generator form): Conv2d(latent + in_nc -> n_channels, bias) /
    ReLU, depth - 2 times Conv2d(no bias) / BatchNorm2d(eps 1e-4, momentum 0.95) / LeakyReLU(0.01), Conv2d(-> out_nc, no bias), Sigmoid; the
    input is [Z | quantised coefficients], Z re-concatenated in front of the features at the first conv ('first_layer') or at every conv
    ('all_layers'); the output is quantised coefficients + (sigmoid - 0.5).  `dncnn` is the reference's ModuleList, so state_dict keys
    (dncnn.0.weight, dncnn.3.running_mean, ...) and positional checkpoint loading are the reference's.

    chroma_generator=True (in_nc 384, out_nc 128; :207-212): the input coefficients are Y's 256 | the quantised low 8x8 of Cb | of Cr on the 16x16
    block grid, the output is those last 128 + (sigmoid - 0.5): the chroma planes' low frequencies, the only ones the colour model reconstructs.

    On the GPU in eval() the conv chain runs on the library's kernels (esr_hip/dncnn.py: forward and input gradient, BatchNorm folded, frozen
    weights; set_precision picks 'split' — fp32-class, the default — or 'bf16').  CPU tensors and training mode run the stock modules."""

    def __init__(self, n_channels, depth, kernel_size=3, in_nc=64, out_nc=64, norm_type='batch', act_type='leakyrelu', latent_input=None,
                 num_latent_channels=None, discriminator=False, expected_input_size=None, chroma_generator=False, spectral_norm=False,
                 pooling_no_FC=False, avoid_padding=None, output_layer=None):
        super(DnCNN, self).__init__()
        assert act_type == 'leakyrelu'
        assert norm_type in ['batch', 'instance', 'layer', None]
        assert output_layer in ['Sigmoid', 'ReLU', None]
        if discriminator:
            raise NotImplementedError('DnCNN(discriminator=True): the DnCNN critic belongs to training the JPEG model, which this build does not do')
        if chroma_generator and not (in_nc - 256 == out_nc == 128):
            raise NotImplementedError('DnCNN(chroma_generator=True, in_nc=%r, out_nc=%r): the chroma generator reads Y\'s 256 coefficients and the 2 x 64 '
                                      'low chroma ones and estimates the latter: in_nc = 384, out_nc = 128 (define_G with chroma_mode)' % (in_nc, out_nc))
        if norm_type in ('layer', 'instance'):
            raise NotImplementedError("DnCNN(norm_type=%r): 'batch' (folded into the convs in eval mode) or None" % (norm_type,))
        if avoid_padding:
            raise NotImplementedError(
                "DnCNN(avoid_padding=True), the padding-free form: not part of this build. With latent_input='all_layers' the reference's own forward "
                'fails there (the latent is not cropped with the shrinking maps: "Sizes of tensors must match"), and the shipped training settings '
                'use padding. define_G reads avoid_padding = not bool(network_G.padding): in the options file set network_G "padding": 1.')
        if kernel_size != 3:
            raise NotImplementedError('DnCNN(kernel_size=%r): 3' % (kernel_size,))
        self.discriminator_net = False
        self.chroma_generator = bool(chroma_generator)
        self.margins = 0
        self.latent_input = latent_input
        self.num_latent_channels = num_latent_channels
        if latent_input not in ['all_layers', 'first_layer'] or num_latent_channels is None:
            self.num_latent_channels = 0
        lat_rest = self.num_latent_channels * (self.latent_input == 'all_layers')
        esr_dncnn.check_shapes(n_channels, depth, in_nc, out_nc, self.num_latent_channels, lat_rest)
        layers = [nn.Conv2d(in_nc + self.num_latent_channels, n_channels, kernel_size=3, padding=1, bias=True), nn.ReLU(inplace=True)]
        for _ in range(1, depth - 1):
            layers.append(nn.Conv2d(n_channels + lat_rest, n_channels, kernel_size=3, padding=1, bias=False))
            if norm_type == 'batch':
                layers.append(nn.BatchNorm2d(n_channels, eps=0.0001, momentum=0.95))
            layers.append(nn.LeakyReLU(inplace=True))
        layers.append(nn.Conv2d(n_channels + lat_rest, out_nc, kernel_size=3, padding=1, bias=False))
        if output_layer == 'Sigmoid':
            layers.append(nn.Sigmoid())
        elif output_layer == 'ReLU':
            layers.append(nn.ReLU())
        self.output_layer = output_layer
        self.dncnn = nn.ModuleList(layers)
        self._engine = None
        self._precision = 'split'

    @property
    def engine(self):
        if self._engine is None:
            self._engine = esr_dncnn.DnCNNEngine(self.dncnn, self.num_latent_channels, self.latent_input, precision=self._precision)
        return self._engine

    def set_precision(self, precision):
        """'split' (default): bf16 hi+lo operands, fp32-class outputs and gradients; 'bf16': one plane, one MFMA per product."""
        assert precision in ('split', 'bf16')
        self._precision = precision
        if self._engine is not None:
            self._engine.set_precision(precision)

    def on_kernels(self, x):
        return x.is_cuda and not self.training

    def pre_output(self, x):
        """The last conv's output, before the output layer, for the input [Z | quantised coefficients] (HIP engine; GPU, eval mode)."""
        return esr_dncnn.dncnn_forward(self.engine, x)

    def _torch_chain(self, x, stop_before_output):
        latent_input, x = torch.split(x, [self.num_latent_channels, x.size(1) - self.num_latent_channels], dim=1)
        for i, module in enumerate(self.dncnn):
            if stop_before_output and isinstance(module, (nn.Sigmoid, nn.ReLU)) and i == len(self.dncnn) - 1 and self.output_layer is not None:
                break
            if self.num_latent_channels > 0 and isinstance(module, nn.Conv2d) and (self.latent_input == 'all_layers' or i == 0):
                x = torch.cat([latent_input, x], dim=1)
            x = module(x)
        return x

    def forward(self, x):
        quantized_coeffs = x[:, self.num_latent_channels + (256 if self.chroma_generator else 0):]
        if self.on_kernels(x):
            y = self.pre_output(x)
            if self.output_layer == 'Sigmoid':
                y = torch.sigmoid(y)
            elif self.output_layer == 'ReLU':
                y = torch.relu(y)
        else:
            y = self._torch_chain(x, False)
        return quantized_coeffs + (y - 0.5)
