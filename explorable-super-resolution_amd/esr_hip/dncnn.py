"""The DnCNN generator of the explorable JPEG decoder on the library's kernels (reference codes/models/modules/architecture.py:109-214,
generator form): a chain of 3x3 / pad 1 convs over the 64 DCT-coefficient planes, the latent Z concatenated IN FRONT of the features
(:198) at the first conv ('first_layer') or at every conv ('all_layers'), ReLU after the first conv, eval-mode BatchNorm + LeakyReLU(0.01)
after the middle ones, nothing after the last.  Forward and input gradient, frozen weights, modelled on esr_hip/vgg.py:

  * activations live in the conv kernels' layout ([planes][B][CG][h+2][w+2][8] bf16, zero border; hi+lo planes in 'split')
  * every layer is ONE esr_conv3x3 launch: layer 0 act_slope = 0 (nn.ReLU), middle layers act_slope = 0.01 (nn.LeakyReLU()'s default),
    the last layer identity, stored as fp32 NCHW (out_nchw; one launch per 64 output channels — the chroma generator has 128): the
    PRE-sigmoid output y — the sigmoid, the "- 0.5", the addition to the
    quantised coefficients and the inverse DCT are one esr_jpeg_extract launch (esr_hip/jpeg.py)
  * eval-mode BatchNorm (eps 1e-4) is folded into the conv before packing: rows scaled by weight / sqrt(running_var + eps), bias
    = bn.bias - running_mean * that scale
  * no concat copy: Z sits in the leading channel groups of every layer's input buffer (packed there from the input tensor) and the conv
    writes the feature groups behind it
  * input gradient with respect to the whole input [Z | coefficients]: the conv kernel on transposed + flipped packs, the previous
    activation's backward as its mask over the FEATURE groups only (mask_slope 0.01 / 0), Z's gradient summed over the layers it enters.
The weights are frozen: no weight gradients, no .grad on the module.  The packs are rebuilt when a conv weight or one of the four BatchNorm
tensors changes storage or version (load_state_dict, an in-place edit).  A pass that carries no graph runs on two ping-pong buffers."""
import ctypes as C

import torch

from . import _lib
from . import act as A
from .act import new_at, new_zeroed, view_of
from ._image import detach_f32
from ._lib import EsrError, check

def check_shapes(n_channels, depth, in_nc, out_nc, lat_first, lat_rest):
    """The conv entry point takes input and output channel counts of up to 64 or a multiple of 64, in both directions (forward packs slice the
    outputs, data-gradient packs the inputs), and the features must start on a channel-group boundary behind Z."""
    if depth < 2:
        raise EsrError('DnCNN(depth=%d): at least a first and a last conv' % depth)
    if lat_first % 8 or lat_rest % 8:
        raise EsrError('DnCNN: num_latent_channels = %d must be a multiple of 8 (the features start on a channel-group boundary behind Z)'
                       % max(lat_first, lat_rest))
    ok = lambda c: 0 < c <= 64 or c % 64 == 0
    for k in range(depth):
        cin = (in_nc + lat_first) if k == 0 else (n_channels + lat_rest)
        cout = out_nc if k == depth - 1 else n_channels
        if not ok(cin) or not ok(cout):
            raise EsrError('DnCNN conv %d of %d (%d -> %d channels, latent included): the conv kernels take up to 64 or a multiple of 64 channels '
                           'on both sides' % (k, depth, cin, cout))


class _Layer:
    pass


class DnCNNEngine:
    """Launch planner of one architecture.DnCNN (generator form).  precision: 'split' (default; bf16 hi+lo, fp32-class) or 'bf16'."""

    def __init__(self, modules, num_latent_channels, latent_input, precision='split'):
        mods = list(modules)
        self.layers = []
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, torch.nn.Sigmoid):
                i += 1
                continue
            if not isinstance(m, torch.nn.Conv2d) or m.kernel_size != (3, 3) or m.stride != (1, 1) or m.padding != (1, 1) or m.groups != 1:
                raise EsrError('DnCNN module %d (%r): Conv2d 3x3, stride 1, padding 1 expected' % (i, m))
            ly = _Layer()
            ly.conv, ly.bn, ly.slope = m, None, 1.0
            i += 1
            if i < len(mods) and isinstance(mods[i], torch.nn.BatchNorm2d):
                ly.bn = mods[i]
                i += 1
            if i < len(mods) and isinstance(mods[i], torch.nn.ReLU):
                ly.slope = 0.0
                i += 1
            elif i < len(mods) and isinstance(mods[i], torch.nn.LeakyReLU):
                ly.slope = float(mods[i].negative_slope)
                i += 1
            ly.fwd = ly.tr = ly.w = ly.b = None
            self.layers.append(ly)
        L = num_latent_channels if latent_input in ('all_layers', 'first_layer') else 0
        self.L = L
        for k, ly in enumerate(self.layers):
            ly.lat = L if (k == 0 or latent_input == 'all_layers') else 0
            ly.cin, ly.cout = ly.conv.in_channels, ly.conv.out_channels
        check_shapes(self.layers[0].cout, len(self.layers), self.layers[0].cin - self.layers[0].lat, self.layers[-1].cout,
                     self.layers[0].lat, self.layers[-1].lat if len(self.layers) > 1 else 0)
        if self.layers[-1].slope != 1.0 or self.layers[-1].bn is not None:
            raise EsrError('DnCNN: the last conv carries no normalisation and no activation')
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

    # ------------------------------------------------------------------ weights
    def _fingerprint(self):
        fp = []
        for ly in self.layers:
            ts = [ly.conv.weight, ly.conv.bias]
            if ly.bn is not None:
                ts += [ly.bn.weight, ly.bn.bias, ly.bn.running_mean, ly.bn.running_var]
            fp.append(tuple(None if t is None else (t.data_ptr(), t._version) for t in ts))
        return tuple(fp)

    def refresh(self):
        """Fold + pack the (frozen) weights: once, and again only when a conv weight or a BatchNorm tensor changed storage or version."""
        fp = self._fingerprint()
        if fp == self._fp:
            return
        packs = []
        with torch.no_grad():
            for ly in self.layers:
                w = ly.conv.weight.detach()
                A.require_gpu(w, 'DnCNN weight')
                if w.dtype != torch.float32:
                    raise EsrError('DnCNN weights: fp32')
                b = None if ly.conv.bias is None else ly.conv.bias.detach().float()
                if ly.bn is not None:
                    bn = ly.bn
                    if bn.running_mean is None or bn.running_var is None:
                        raise EsrError('DnCNN BatchNorm without running statistics')
                    scale = torch.rsqrt(bn.running_var.detach().float() + bn.eps)
                    if bn.weight is not None:
                        scale = scale * bn.weight.detach().float()
                    shift = -bn.running_mean.detach().float() * scale
                    if bn.bias is not None:
                        shift = shift + bn.bias.detach().float()
                    b = shift if b is None else b * scale + shift
                    w = w * scale.view(-1, 1, 1, 1)
                ly.w, ly.b = w.contiguous(), (None if b is None else b.contiguous())
                ly.fwd = A.PackedConvSlices(ly.w, ly.b, split=self.split)
                ly.tr = A.PackedConvSlices(ly.w, None, split=self.split, transposed=True)
                packs += [ly.fwd, ly.tr]
        self._batch.run(packs)
        self._fp = fp

    # ------------------------------------------------------------------ passes
    def _pack_z(self, x, B, Cin, h, w, dst):
        check(_lib.lib.esr_pack_nchw(x.data_ptr(), 0, B, Cin, h, w, 0, self.L, 0, 1, C.byref(dst), A.stream_ptr()), 'esr_pack_nchw')

    @A.one_stream
    def forward(self, x, save):
        """x: fp32 [B, L + 64, h, w] = [Z | quantised coefficients] on the GPU -> (y fp32 [B, 64, h, w], the last conv's output BEFORE the
        sigmoid; saved) where saved is what backward() needs (save=True: every layer's input buffer) or None."""
        A.launch_by_launch('DnCNN')
        x = A.gpu_input(x, 'DnCNN input')
        B, Cin, h, w = x.shape
        if Cin != self.layers[0].cin:
            raise EsrError('DnCNN input has %d channels, the first conv takes %d (latent %d + coefficients)' % (Cin, self.layers[0].cin, self.L))
        self.refresh()
        P, dev = self.planes, x.device
        t = new_at(P, B, (Cin + 7) // 8, h, w, dev)                         # [Z | coefficients]: one pack, borders included
        A.pack_nchw(x, view_of(t), 0, Cin)
        ins, pool = [t], {}
        y = torch.empty(B, self.layers[-1].cout, h, w, dtype=torch.float32, device=dev)
        n = len(self.layers)
        for k, ly in enumerate(self.layers):
            if k == n - 1:
                if ly.cout <= 64:
                    A.conv3x3(ly.fwd, view_of(t), B, h, w, ly.cout, out_nchw=y, act_slope=1.0, use_bias=ly.b is not None, reverse=False)
                    break
                # more than 64 output channels (the chroma generator's 128): one launch per 64-row slice of the pack; the slices carry no bias
                if ly.b is not None:
                    raise EsrError('DnCNN: a last conv of %d > 64 channels with a bias' % ly.cout)
                A.conv3x3_nchw_parts(ly.fwd.parts, view_of(t), B, h, w, y, act_slope=1.0, use_bias=False, reverse=False)
                break
            nxt = self.layers[k + 1]
            zg = nxt.lat // 8
            u = None if save else pool.get(k & 1)
            if u is None:
                u = new_zeroed(P, B, zg + (ly.cout + 7) // 8, h, w, dev)          # zero borders behind Z; the convs never write them
                if zg:
                    self._pack_z(x, B, Cin, h, w, view_of(u, 0, zg))
                if not save:
                    pool[k & 1] = u
            A.conv3x3(ly.fwd, view_of(t), B, h, w, ly.cout, out=view_of(u, zg), act_slope=ly.slope, use_bias=ly.b is not None, reverse=False)
            if save:
                ins.append(u)
            t = u
        return y, ((B, Cin, h, w), ins) if save else None

    @A.one_stream
    def backward(self, saved, d_y):
        """Gradient fp32 [B, L + 64, h, w] of sum(y * d_y) with respect to the input [Z | coefficients] of the forward that produced `saved`."""
        A.launch_by_launch('DnCNN')
        (B, Cin, h, w), ins = saved
        P, dev, s = self.planes, d_y.device, A.stream_ptr()
        d_y = detach_f32(d_y)
        g = new_at(P, B, (d_y.shape[1] + 7) // 8, h, w, dev)
        check(_lib.lib.esr_pack_nchw_norm(d_y.data_ptr(), B, d_y.shape[1], h, w, None, None, C.byref(view_of(g)), s), 'esr_pack_nchw_norm')
        gv = view_of(g)
        dz = []                                       # Z-group gradients of the layers behind the first
        keep = [g]
        for k in range(len(self.layers) - 1, -1, -1):
            ly = self.layers[k]
            zg = ly.lat // 8
            dx = new_zeroed(P, B, (ly.cin + 7) // 8, h, w, dev)
            mk = {}
            if k > 0:                                 # the previous layer's activation backward, from its stored output: feature groups only
                mk = dict(mask_src=view_of(ins[k], zg), mask_cg=(zg, (ly.cin + 7) // 8), mask_slope=self.layers[k - 1].slope)
            A.conv3x3(ly.tr, gv, B, h, w, ly.cin, out=view_of(dx), use_bias=False, reverse=False, **mk)
            keep.append(dx)
            if k > 0:
                if zg:
                    dz.append(view_of(dx, 0, zg))
                gv = view_of(dx, zg)
        d_in = torch.empty(B, Cin, h, w, dtype=torch.float32, device=dev)
        A.unpack_grad_nchw(view_of(dx), d_in, Cin, h, w, 0, Cin)
        for v in dz:
            A.unpack_grad_nchw(v, d_in, Cin, h, w, 0, self.L, accumulate=True)
        return d_in


def dncnn_forward(eng, x):
    """The last conv's pre-sigmoid output for the input [Z | coefficients]; differentiable w.r.t. x when x requires grad and grad mode is on
    (input gradient only)."""
    return A.engine_forward(eng, 'DnCNN', x)
