"""Network factory — define_G / init_weights with the reference's signatures (codes/models/networks.py:14-123).

Differences that follow from the MI355X design (one process per GPU, RCCL data parallelism):
  * define_G never wraps the generator in nn.DataParallel; callers that reach through `.module` (GUI.py:1687) still work
    because the CEM wrapper and RRDBNet expose `.module` as themselves.
  * define_D builds the reference's default critic (Discriminator_VGG_128) from stock PyTorch modules (MIOpen kernels): it is the other
    half of the configs[2] training step, not part of the RRDB+CEM kernel path.
  * define_F builds the VGG feature extractor without torchvision: the module tree is built here and the weights come from a file
    (architecture.VGGFeatureExtractor), never from the network.
"""
import functools

import torch
import torch.nn as nn

import models.modules.architecture as arch


_WEIGHTED = (nn.Conv2d, nn.ConvTranspose2d, nn.Linear)


def _is_cem_filter(m):
    """CEM taps are constants and keep their values (reference networks.py:29-31 checks the same marker attribute)."""
    return bool(getattr(m, 'filter_layer', False))


def _init_module(m, kind, scale=1.0, std=0.02):
    """One module's initialisation; semantics of the reference's weights_init_{normal,kaiming,orthogonal} (networks.py:14-60):
    conv / linear weights drawn per `kind` (kaiming: fan_in normal, then * scale), biases zero, BatchNorm affine = identity
    (weight ~ N(1, std) for 'normal')."""
    if isinstance(m, _WEIGHTED):
        if kind == 'kaiming' and _is_cem_filter(m):
            return
        with torch.no_grad():
            if kind == 'normal':
                m.weight.normal_(0.0, std)
            elif kind == 'kaiming':
                nn.init.kaiming_normal_(m.weight, a=0, mode='fan_in')
                m.weight.mul_(scale)
            else:
                nn.init.orthogonal_(m.weight, gain=1)
            if m.bias is not None:
                m.bias.zero_()
    elif isinstance(m, nn.BatchNorm2d):
        with torch.no_grad():
            if kind == 'normal':
                m.weight.normal_(1.0, std)
            else:
                m.weight.fill_(1.0)
            m.bias.zero_()


def weights_init_normal(m, std=0.02):
    _init_module(m, 'normal', std=std)


def weights_init_kaiming(m, scale=1):
    _init_module(m, 'kaiming', scale=scale)


def weights_init_orthogonal(m):
    _init_module(m, 'orthogonal')


def init_weights(net, init_type='kaiming', scale=1, std=0.02):
    if init_type not in ('normal', 'kaiming', 'orthogonal'):
        raise NotImplementedError('initialization method [{:s}] not implemented'.format(init_type))
    print('initialization method [{:s}]'.format(init_type))
    net.apply(functools.partial(_init_module, kind=init_type, scale=scale, std=std))


def define_G(opt, CEM=None, num_latent_channels=None, **kwargs):
    gpu_ids = opt['gpu_ids']
    opt_net = opt['network_G']
    which_model = opt_net['which_model_G']
    opt_net['latent_input'] = opt_net['latent_input'] if opt_net['latent_input'] != "None" else None
    if which_model == 'RRDB_net':
        netG = arch.RRDBNet(in_nc=opt_net['in_nc'], out_nc=opt_net['out_nc'], nf=opt_net['nf'], nb=opt_net['nb'], gc=opt_net['gc'],
                            upscale=opt_net['scale'], norm_type=opt_net['norm_type'], act_type='leakyrelu', mode=opt_net['mode'],
                            upsample_mode='upconv',
                            latent_input=(opt_net['latent_input'] + '_' + opt_net['latent_input_domain']) if opt_net['latent_input'] is not None else None,
                            num_latent_channels=num_latent_channels)
    elif which_model == 'DnCNN':
        chroma_mode = bool(kwargs.get('chroma_mode', False))
        if chroma_mode and not kwargs.get('no_high_freq_chroma_reconstruction', True):
            raise NotImplementedError('Generator model [DnCNN] with no_high_freq_chroma_reconstruction=False (a 2 x 256-channel chroma output): the '
                                      'reference\'s model fixes it to True, and so does this build')
        in_nc = opt['scale'] ** 2 + 2 * 64 if chroma_mode else 64               # (reference networks.py:103-106)
        netG = arch.DnCNN(n_channels=opt_net['nf'], depth=opt_net['nb'], in_nc=in_nc, out_nc=2 * 64 if chroma_mode else 64,
                          norm_type=opt_net['norm_type'], latent_input=opt_net['latent_input'], num_latent_channels=num_latent_channels,
                          chroma_generator=chroma_mode, avoid_padding=not bool(opt_net['padding']), output_layer='Sigmoid')
    elif which_model in ('sr_resnet', 'MSRResNet'):
        raise NotImplementedError('Generator model [{:s}] is outside the RRDB+CEM hot path of this build'.format(which_model))
    else:
        raise NotImplementedError('Generator model [{:s}] not recognized'.format(which_model))
    if opt_net['CEM_arch']:
        netG = CEM.WrapArchitecture_PyTorch(netG, opt['datasets']['train']['patch_size'] if opt['is_train'] else None)
    if opt['is_train']:
        init_weights(netG, init_type='kaiming', scale=0.1)
    if gpu_ids:
        assert torch.cuda.is_available()
        # no nn.DataParallel: one process per GPU; gradients are all-reduced over RCCL by esr_hip.dist
    return netG


def define_D(opt, CEM=None, **kwargs):
    """Critic factory (reference networks.py:126-182).  The critic sees the generator's output with the CEM's invalidity frame cropped
    (patch_size - 2*margins_HR, :133-135)."""
    opt_net = opt['network_D']
    which_model = opt_net['which_model_D']
    input_patch_size = opt['datasets']['train']['patch_size']
    assert not ((opt_net['pre_clipping'] or opt_net['decomposed_input']) and which_model != 'PatchGAN'), 'Unsupported yet'
    if CEM is not None:
        input_patch_size -= 2 * CEM.invalidity_margins_HR
    if which_model == 'discriminator_vgg_128':
        kw = {'num_2_strides': opt_net['num_2_strides']} if opt_net['num_2_strides'] is not None else {}
        netD = arch.Discriminator_VGG_128(in_nc=opt_net['in_nc'], base_nf=opt_net['nf'], nb=opt_net['n_layers'] or 10, norm_type=opt_net['norm_type'],
                                          mode=opt_net['mode'], act_type=opt_net['act_type'], input_patch_size=int(input_patch_size), **kw)
    elif which_model in ('discriminator_vgg_128_nonModified', 'dis_acd', 'PatchGAN', 'discriminator_vgg_96', 'discriminator_vgg_192',
                         'discriminator_vgg_128_SN') or 'DnCNN_D' in which_model:
        raise NotImplementedError('Discriminator model [{:s}] is outside this build (the explorable-SR configuration uses discriminator_vgg_128)'.format(which_model))
    else:
        raise NotImplementedError('Discriminator model [{:s}] not recognized'.format(which_model))
    init_weights(netD, init_type='kaiming', scale=1)
    return netD          # no nn.DataParallel: one process per GPU, D gradients all-reduced over RCCL (esr_hip.dist)


def define_F(opt, use_bn=False, **kwargs):
    """VGG feature extractor (reference networks.py:185-197): VGG19 features up to conv5_4 before its ReLU (feature_layer 34), or
    arch='vgg<N>_<layer>' for another cut; weights from the options' path.pretrained_model_F or the torch hub cache (see
    VGGFeatureExtractor).  Returned in eval() mode; no nn.DataParallel (one process per GPU; the weights are frozen, so nothing is exchanged)."""
    from esr_hip.vgg import parse_arch
    gpu_ids = opt['gpu_ids']
    device = torch.device('cuda' if gpu_ids else 'cpu')
    feature_layer = 49 if use_bn else 34
    if 'arch' in kwargs:
        kwargs['arch'], feature_layer = parse_arch(kwargs['arch'], use_bn)
    path = (opt.get('path') or {}).get('pretrained_model_F') if hasattr(opt, 'get') else None
    netF = arch.VGGFeatureExtractor(feature_layer=feature_layer, use_bn=use_bn, use_input_norm=True, device=device, pretrained_path=path, **kwargs)
    return netF.eval()
