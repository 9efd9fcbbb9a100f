"""The VGG feature extractor on the library's kernels: VGGFeatureExtractor (reference codes/models/modules/architecture.py:658-705) over
torchvision's VGG `features` (Conv2d 3x3 pad 1 / ReLU / MaxPool2d 2x2), forward and input gradient, with torch only carrying the graph.

  * activations live in the conv kernels' layout ([planes][B][CG][H+2][W+2][8] bf16, zero border; one plane in 'bf16', hi+lo in 'split')
  * the input normalisation (x - mean) / std is applied by the pack that brings the image into that layout (esr_pack_nchw_norm), before
    conv1_1's zero padding, as the reference's forward does; its adjoint (/ std) by the gradient unpack (esr_unpack_grad_nchw_norm)
  * every conv + ReLU is ONE esr_conv3x3 launch (act_slope = 0; a cut at a conv stores act_slope = 1); 128- to 512-channel outputs run as
    64-channel output slices of that launch, as the critic's layers do (esr_hip/critic.py)
  * every 2x2 max pool is esr_maxpool2x2; its backward (esr_maxpool2x2_grad) recomputes the window argmax from the saved pre-pool activation
    and applies the preceding ReLU's backward in the same pass
  * the input gradient is the conv kernel on transposed + flipped packs, the ReLU's backward fused as its mask (mask_slope = 0)
The weights are frozen (the reference sets requires_grad = False on them): they are packed once, and re-packed only when their storage or
version changes (load_state_dict).  The backward computes the input gradient only — no weight-gradient launch, no .grad on the module.
A pass that does not carry a graph (the real batch of the G step, the Z search's GT_HR_VGG) keeps nothing: its buffers go back to torch's
allocator layer by layer."""
import ctypes as C

import torch

from . import _lib
from . import act as A
from .act import new_at, new_zeroed, view_of
from ._image import detach_f32
from ._lib import EsrError, check

# torchvision.models.vgg cfgs ('M' = MaxPool2d(2, 2)); features = [Conv2d(cin, v, 3, padding=1), ReLU(inplace=True)] per number
CFGS = {
    'vgg11': [64, 'M', 128, 'M', 256, 256, 'M', 512, 512, 'M', 512, 512, 'M'],
    'vgg13': [64, 64, 'M', 128, 128, 'M', 256, 256, 'M', 512, 512, 'M', 512, 512, 'M'],
    'vgg16': [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M'],
    'vgg19': [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512, 512, 512, 512, 'M'],
}


def layer_table(arch='vgg19', feature_layer=34, in_nc=3):
    """torchvision `features` of `arch`, cut after index `feature_layer` (features[:feature_layer + 1], architecture.py:681):
    [('conv', cin, cout) | ('relu',) | ('pool',)] in torchvision indexing."""
    if arch not in CFGS:
        raise NotImplementedError('VGG arch %r: %s (batch-norm variants are not part of this build)' % (arch, sorted(CFGS)))
    table, cin = [], in_nc
    for v in CFGS[arch]:
        if v == 'M':
            table.append(('pool',))
        else:
            table += [('conv', cin, v), ('relu',)]
            cin = v
    if not 0 <= feature_layer < len(table):
        raise ValueError('feature_layer %d: %s has %d layers' % (feature_layer, arch, len(table)))
    return table[:feature_layer + 1]


def parse_arch(arch, use_bn=False):
    """(arch, feature_layer) as define_F reads them (codes/models/networks.py:185-197): 'vgg16_22' -> ('vgg16', 22); no suffix -> 34 (49 with
    batch norm: VGG19-54, before its ReLU)."""
    feature_layer = 49 if use_bn else 34
    if arch is not None and 'vgg' in arch:
        if len(arch) > len('vgg11_'):
            feature_layer = int(arch[len('vgg11_'):])
        arch = arch[:len('vgg11')]
    return arch, feature_layer


class _Op:
    pass


class VGGEngine:
    """Launch planner of one VGGFeatureExtractor.  precision: 'split' (default; bf16 hi+lo, three MFMAs per product: fp32-class) or 'bf16'
    (one plane, one MFMA)."""

    def __init__(self, features, mean=None, std=None, precision='split'):
        self.ops = []
        mods = list(features)
        i = 0
        while i < len(mods):
            m = mods[i]
            op = _Op()
            op.index = i
            if isinstance(m, torch.nn.Conv2d):
                if m.kernel_size != (3, 3) or m.stride != (1, 1) or m.padding != (1, 1) or m.dilation != (1, 1) or m.groups != 1 or m.bias is None:
                    raise EsrError('VGG conv %r: the kernels implement 3x3, stride 1, padding 1, with bias' % (m,))
                if m.out_channels % 64 and m.out_channels > 64:
                    raise EsrError('VGG conv %r: up to 64 or a multiple of 64 output channels' % (m,))
                op.kind, op.conv, op.cin, op.cout = 'conv', m, m.in_channels, m.out_channels
                op.relu = i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.ReLU)
                op.fwd = op.tr = None
                i += 2 if op.relu else 1
            elif isinstance(m, torch.nn.MaxPool2d):
                ks, st = m.kernel_size, m.stride
                if (ks not in (2, (2, 2))) or (st not in (2, (2, 2))) or m.padding not in (0, (0, 0)) or m.dilation not in (1, (1, 1)) or m.ceil_mode:
                    raise EsrError('VGG pool %r: the kernels implement MaxPool2d(2, 2)' % (m,))
                op.kind = 'pool'
                i += 1
            else:
                raise EsrError('unexpected module %r in VGG features: Conv2d / ReLU / MaxPool2d' % (m,))
            self.ops.append(op)
        if not self.ops or self.ops[0].kind != 'conv':
            raise EsrError('VGG features must start with a conv')
        self.mean, self.std = mean, std
        self.precision = None
        self._fp = None
        self._batch = A.PackBatch()
        self.set_precision(precision)

    def set_precision(self, precision):
        assert precision in ('bf16', 'split')
        if precision == self.precision:
            return
        self.precision, self.planes, self.split = precision, (2 if precision == 'split' else 1), precision == 'split'
        self._fp = None
        for op in self.ops:
            if op.kind == 'conv':
                op.fwd = op.tr = None

    def out_channels(self):
        return [op.cout for op in self.ops if op.kind == 'conv'][-1]

    def out_size(self, H, W):
        for op in self.ops:
            if op.kind == 'pool':
                H, W = H // 2, W // 2
        return H, W

    # ------------------------------------------------------------------ weights
    def refresh(self):
        """Pack the (frozen) weights: once, and again only when a weight's storage or version changed (load_state_dict, .to())."""
        convs = [op for op in self.ops if op.kind == 'conv']
        fp = tuple((op.conv.weight.data_ptr(), op.conv.weight._version, op.conv.bias.data_ptr(), op.conv.bias._version) for op in convs)
        if fp == self._fp:
            return
        packs = []
        for op in convs:
            A.require_gpu(op.conv.weight, 'VGG weight')
            if op.conv.weight.dtype != torch.float32 or op.conv.bias.dtype != torch.float32:
                raise EsrError('VGG weights: fp32')
            if op.fwd is None or op.fwd.bias_p is not op.conv.bias:
                op.fwd = A.PackedConvSlices(op.conv.weight, op.conv.bias, split=self.split)
                op.tr = A.PackedConvSlices(op.conv.weight, None, split=self.split, transposed=True)
            packs += [op.fwd, op.tr]
        self._batch.run(packs)
        self._fp = fp

    def _norm_ptrs(self, device):
        if self.mean is None:
            return None, None
        mean = self.mean.detach().reshape(-1).float().contiguous()
        std = self.std.detach().reshape(-1).float().contiguous()
        if mean.device != device:
            raise EsrError('VGG mean / std buffers are not on the input device')
        self._norm_keep = (mean, std)                 # alive until the launches that read them have been enqueued (and the next call)
        return mean.data_ptr(), std.data_ptr()

    # ------------------------------------------------------------------ passes
    @A.one_stream
    def forward(self, x, save):
        """x: fp32 [B, C, H, W] on the GPU -> (features fp32 [B, C', H', W'], saved) where saved is what backward() needs (save=True: the
        output of every conv and the input of the last op) or None."""
        A.launch_by_launch('VGG')
        x = A.gpu_input(x, 'VGG input')
        B, Cin, H, W = x.shape
        if Cin != self.ops[0].cin:
            raise EsrError('VGG input has %d channels, the first conv takes %d' % (Cin, self.ops[0].cin))
        if self.mean is not None and self.mean.numel() != Cin:
            raise EsrError('VGG input normalisation: %d channels, %d means' % (Cin, self.mean.numel()))
        self.refresh()
        P, dev, s = self.planes, x.device, A.stream_ptr()
        mean_p, std_p = self._norm_ptrs(dev)
        t = new_at(P, B, (Cin + 7) // 8, H, W, dev)
        check(_lib.lib.esr_pack_nchw_norm(x.data_ptr(), B, Cin, H, W, mean_p, std_p, C.byref(view_of(t)), s), 'esr_pack_nchw_norm')
        outs = []
        h, w = H, W
        for op in self.ops:
            if op.kind == 'conv':
                y = new_zeroed(P, B, (op.cout + 7) // 8, h, w, dev)
                A.conv3x3(op.fwd, view_of(t), B, h, w, op.cout, out=view_of(y), act_slope=0.0 if op.relu else 1.0, reverse=False)
            else:
                if h < 2 or w < 2:
                    raise EsrError('VGG max pool on a %dx%d map (input %dx%d)' % (h, w, H, W))
                h, w = h // 2, w // 2
                y = new_at(P, B, t.shape[2], h, w, dev)
                check(_lib.lib.esr_maxpool2x2(C.byref(view_of(t)), C.byref(view_of(y)), B, s), 'esr_maxpool2x2')
            if save:
                outs.append(y)
            t = y
        nc = self.out_channels()
        feat = torch.empty(B, nc, h, w, dtype=torch.float32, device=dev)
        check(_lib.lib.esr_unpack_nchw(C.byref(view_of(t)), B, nc, feat.data_ptr(), s), 'esr_unpack_nchw')
        return feat, ((B, Cin, H, W), outs) if save else None

    @A.one_stream
    def backward(self, saved, d_feat):
        """Input gradient fp32 [B, C, H, W] of sum(features * d_feat) through the forward that produced `saved`."""
        A.launch_by_launch('VGG')
        (B, Cin, H, W), outs = saved
        P, dev, s = self.planes, d_feat.device, A.stream_ptr()
        d_feat = detach_f32(d_feat)
        last = outs[-1]
        g = new_at(P, B, last.shape[2], last.shape[3] - 2, last.shape[4] - 2, dev)
        nc = d_feat.shape[1]
        check(_lib.lib.esr_pack_nchw_norm(d_feat.data_ptr(), B, nc, d_feat.shape[2], d_feat.shape[3], None, None, C.byref(view_of(g)), s),
              'esr_pack_nchw_norm')
        n = len(self.ops)
        is_relu_conv = lambda k: k >= 0 and self.ops[k].kind == 'conv' and self.ops[k].relu
        if is_relu_conv(n - 1):
            # the cut is after a ReLU: its backward on the incoming gradient
            g2 = new_at(P, B, g.shape[2], g.shape[3] - 2, g.shape[4] - 2, dev)
            A.act_combine(view_of(g2), B, A_=view_of(g), alpha=1.0, mask=view_of(last), mask_slope=0.0)
            g = g2
        # g: gradient w.r.t. the PRE-activation output of op k (conv) / the output of op k (pool)
        for k in range(n - 1, -1, -1):
            op = self.ops[k]
            _, _, cg, Hp, Wp, _ = g.shape
            h, w = Hp - 2, Wp - 2
            if op.kind == 'conv':
                dx = new_zeroed(P, B, (op.cin + 7) // 8, h, w, dev)
                mk = {}
                if is_relu_conv(k - 1):              # the previous layer's ReLU backward, from its saved output
                    mk = dict(mask_src=view_of(outs[k - 1]), mask_cg=(0, (op.cin + 7) // 8), mask_slope=0.0)
                A.conv3x3(op.tr, view_of(g), B, h, w, op.cin, out=view_of(dx), use_bias=False, reverse=False, **mk)
            else:
                xin = outs[k - 1]                    # the pool's input (a pool never comes first)
                dx = new_at(P, B, xin.shape[2], xin.shape[3] - 2, xin.shape[4] - 2, dev)
                check(_lib.lib.esr_maxpool2x2_grad(C.byref(view_of(xin)), C.byref(view_of(g)), 1 if is_relu_conv(k - 1) else 0, C.byref(view_of(dx)),
                                                   B, s), 'esr_maxpool2x2_grad')
            g = dx
        dxin = torch.empty(B, Cin, H, W, dtype=torch.float32, device=dev)
        _, std_p = self._norm_ptrs(dev)
        check(_lib.lib.esr_unpack_grad_nchw_norm(C.byref(view_of(g)), B, Cin, std_p, dxin.data_ptr(), s), 'esr_unpack_grad_nchw_norm')
        return dxin


def vgg_forward(eng, x):
    """Features of x through the engine; differentiable w.r.t. x when x requires grad and grad mode is on (input gradient only)."""
    return A.engine_forward(eng, 'VGG', x)
