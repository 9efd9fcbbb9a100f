"""The two networks of kernel estimation as plain torch.nn modules (the 'stock' engine; the reference's codes/KernelGAN/networks.py).

G is six bias-free convolutions without activations, applied to every colour plane on its own: a linear map, equal to ONE correlation with
the 13 x 13 kernel composed from its layers, sub-sampled by 2 (Generator.curr_k, Generator.forward(composed=True)).  D is a patch critic:
a spectrally normalised 7 x 7 conv, five [1 x 1 conv, BatchNorm, ReLU] and a 1 x 1 conv with a sigmoid, always in training mode."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class Generator(nn.Module):
    def __init__(self, conf):
        super().__init__()
        struct, C = conf.G_structure, conf.G_chan
        self.stride = int(1 / conf.scale_factor)
        self.first_layer = nn.Conv2d(1, C, struct[0], bias=False)
        self.feature_block = nn.Sequential(*[nn.Conv2d(C, C, k, bias=False) for k in struct[1:-1]])
        self.final_layer = nn.Conv2d(C, 1, struct[-1], stride=self.stride, bias=False)
        self.kernel_size = sum(struct) - len(struct) + 1
        self.output_size = (conf.input_crop_size - self.kernel_size) // self.stride + 1
        self.forward_shave = int(conf.input_crop_size * conf.scale_factor) - self.output_size

    def layers(self):
        return [self.first_layer] + list(self.feature_block) + [self.final_layer]

    def curr_k(self):
        """The kernel the layers compose to: a delta pushed through them, flipped."""
        w = [m.weight for m in self.layers()]
        k = F.conv2d(torch.ones(1, 1, 1, 1, dtype=w[0].dtype, device=w[0].device), w[0], padding=self.kernel_size - 1)
        for wl in w[1:]:
            k = F.conv2d(k, wl)
        return k.squeeze().flip([0, 1])

    def forward(self, x, composed=False):
        x = x.transpose(0, 1)                       # the three colour planes as a batch of one-channel images
        if composed:
            y = F.conv2d(x, self.curr_k()[None, None], stride=self.stride)
        else:
            y = self.final_layer(self.feature_block(self.first_layer(x)))
        return y.transpose(0, 1)


class Discriminator(nn.Module):
    def __init__(self, conf):
        super().__init__()
        C, sn = conf.D_chan, nn.utils.spectral_norm
        self.first_layer = sn(nn.Conv2d(3, C, conf.D_kernel_size, bias=True))
        block = []
        for _ in range(1, conf.D_n_layers - 1):
            block += [sn(nn.Conv2d(C, C, 1, bias=True)), nn.BatchNorm2d(C), nn.ReLU(True)]
        self.feature_block = nn.Sequential(*block)
        self.final_layer = nn.Sequential(sn(nn.Conv2d(C, 1, 1, bias=True)), nn.Sigmoid())
        self.forward_shave = conf.D_kernel_size - 1

    def convs(self):
        return [self.first_layer] + [m for m in self.feature_block if isinstance(m, nn.Conv2d)] + [self.final_layer[0]]

    def norms(self):
        return [m for m in self.feature_block if isinstance(m, nn.BatchNorm2d)]

    def forward(self, x):
        return self.final_layer(self.feature_block(self.first_layer(x)))


def weights_init_G(m):
    if isinstance(m, nn.Conv2d):
        nn.init.xavier_normal_(m.weight, 0.1)


def weights_init_D(m):
    """Biases 0, BatchNorm weights N(1, 0.02).  The reference also draws xavier_normal(0.1) into `m.weight` of every conv, but under
    spectral_norm, after the forward its constructor runs, that attribute is the normalised COPY recomputed at every forward: the stored
    weight_orig keeps nn.Conv2d's default initialisation.  That effective behaviour is kept (the draw that is thrown away is not made)."""
    if isinstance(m, nn.Conv2d):
        if m.bias is not None:
            m.bias.data.fill_(0)
    elif isinstance(m, nn.BatchNorm2d):
        m.weight.data.normal_(1.0, 0.02)
        m.bias.data.fill_(0)
