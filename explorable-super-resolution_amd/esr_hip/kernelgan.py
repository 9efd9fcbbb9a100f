"""Kernel estimation (KernelGAN) for E images in lock step on the esr_kgan_* kernels (csrc/esr_kgan.hip, include/esr_hip.h).

KernelGanEngine owns the [E, ...] parameters of E generator / critic pairs, their Adam states and every buffer of one iteration.  The
generator is applied as the ONE 13 x 13 kernel its six linear layers compose to; its layers get their gradient through dL/dk and the
adjoint of the composition.  The critic's parameters are one flat vector per estimation (d_layout).  Nothing here synchronises with the
host: the bicubic loss of every iteration goes to a device log [E, 200] that the caller reads once per 200 iterations."""
import types

import numpy as np
import torch

from . import _lib
from .act import require_gpu, stream_ptr
from .optim import Adam

LAMBDAS = ('bicubic', 'sum2one', 'boundaries', 'centralized', 'sparse')
LOG_SLOTS = 200
_G_STRUCT = [7, 5, 3, 1, 1, 1]


def d_layout(C):
    """Offsets into the critic's flat parameter vector and into its u/v vector: {layer: dict(w, b[, gamma, beta], cout, k, u, v)} and the two lengths."""
    out, base, ub = {}, 0, 0
    for l in range(7):
        cout, k = (1 if l == 6 else C), (147 if l == 0 else C)
        d = dict(w=base, cout=cout, k=k, b=base + cout * k, u=ub, v=ub + cout)
        base = d['b'] + cout
        if 1 <= l <= 5:
            d['gamma'], d['beta'] = base, base + C
            base += 2 * C
        ub += cout + k
        out[l] = d
    return out, base, ub


def pack_d(D):
    """A stock Discriminator's state as (flat parameters, flat u/v), fp32 CPU."""
    convs, norms = D.convs(), D.norms()
    ps, uv = [], []
    for l, m in enumerate(convs):
        ps += [m.weight_orig.detach().reshape(-1), m.bias.detach().reshape(-1)]
        if 1 <= l <= 5:
            ps += [norms[l - 1].weight.detach().reshape(-1), norms[l - 1].bias.detach().reshape(-1)]
        uv += [m.weight_u.detach().reshape(-1), m.weight_v.detach().reshape(-1)]
    return torch.cat(ps).float().cpu(), torch.cat(uv).float().cpu()


def unpack_d(flat, D):
    """{parameter name of the stock Discriminator: its slice of a flat vector (parameters or gradients)}."""
    lay, _, _ = d_layout(D.first_layer.weight_orig.shape[0])
    convs, norms = D.convs(), D.norms()
    names = {id(p): n for n, p in D.named_parameters()}
    out = {}
    for l, m in enumerate(convs):
        d = lay[l]
        out[names[id(m.weight_orig)]] = flat[d['w']:d['b']].reshape(m.weight_orig.shape)
        out[names[id(m.bias)]] = flat[d['b']:d['b'] + d['cout']]
        if 1 <= l <= 5:
            C = d['cout']
            out[names[id(norms[l - 1].weight)]] = flat[d['gamma']:d['gamma'] + C]
            out[names[id(norms[l - 1].bias)]] = flat[d['beta']:d['beta'] + C]
    return out


def _p(t):
    return None if t is None else t.data_ptr()


class KernelGanEngine:
    def __init__(self, E, conf, device='cuda'):
        device = torch.device(device)
        if device.type != 'cuda':
            raise _lib.EsrError("the 'hip' kernel-estimation engine runs on an AMD GPU: there is no CPU fallback (engine='stock' is the CPU route)")
        if list(conf.G_structure) != _G_STRUCT or conf.G_kernel_size != 13 or conf.D_kernel_size != 7 or conf.D_n_layers != 7 or conf.scale_factor != 0.5:
            raise _lib.EsrError('the esr_kgan kernels are built for G_structure [7,5,3,1,1,1], a 13 x 13 kernel, scale 0.5 and a 7-layer critic with a 7 x 7 first filter')
        if E < 1:
            raise _lib.EsrError('E must be at least 1')
        self.E, self.C, self.CD, self.S, self.device, self.conf = E, conf.G_chan, conf.D_chan, conf.input_crop_size, device, conf
        _lib.check(min(_lib.lib.esr_kgan_d_param_count(self.CD), 0), 'esr_kgan_d_param_count')
        _lib.check(min(_lib.lib.esr_kgan_d_param_count(self.C), 0), 'esr_kgan_d_param_count (G_chan)')
        _lib.check(min(_lib.lib.esr_kgan_apply_blocks(self.S, self.S), 0), 'esr_kgan_apply_blocks')
        self.nd, self.nuv = _lib.lib.esr_kgan_d_param_count(self.CD), _lib.lib.esr_kgan_d_uv_count(self.CD)
        assert (self.nd, self.nuv) == d_layout(self.CD)[1:]
        from KernelGAN import networks, util
        gs, ds, uvs = [], [], []
        for _ in range(E):                                          # the stock modules' initialisation, one draw per estimation
            G, D = networks.Generator(conf), networks.Discriminator(conf)
            G.apply(networks.weights_init_G)
            D.apply(networks.weights_init_D)
            gs.append([m.weight.detach() for m in G.layers()])
            p, uv = pack_d(D)
            ds.append(p)
            uvs.append(uv)
        f32 = dict(dtype=torch.float32, device=device)
        self.gw = [torch.nn.Parameter(torch.stack([g[l] for g in gs]).to(**f32).contiguous()) for l in range(6)]
        self.dp = torch.nn.Parameter(torch.stack(ds).to(**f32).contiguous())
        self.uv = torch.stack(uvs).to(**f32).contiguous()
        for p in self.gw + [self.dp]:
            p.grad = torch.zeros_like(p)
        self.optimizer_G = Adam(self.gw, lr=conf.g_lr, betas=(conf.beta1, 0.999))
        self.optimizer_D = Adam([self.dp], lr=conf.d_lr, betas=(conf.beta1, 0.999))
        self.lambdas = [dict(bicubic=5., sum2one=0.5, boundaries=0.5, centralized=0., sparse=0.) for _ in range(E)]
        self.lam = torch.empty(E, 5, **f32)
        self.push_lambdas()
        self.mask = torch.as_tensor(util.create_penalty_mask(13, 30), **f32).contiguous()
        self.bict = torch.as_tensor(util.bicubic_table(), **f32).contiguous()
        C = self.C
        self.K = [None] + [torch.empty(E, c, s, s, **f32) for c, s in ((C, 11), (C, 13), (C, 13), (C, 13), (1, 13))]
        self.dK = [None] + [torch.empty_like(t) for t in self.K[1:]]
        self.losses = torch.zeros(E, 5, **f32)
        self.bic_log = torch.zeros(E, LOG_SLOTS, **f32)
        self._g_bufs, self._critic_bufs = {}, {}
        self.imgs = None

    # ---- small state
    def push_lambdas(self):
        self.lam.copy_(torch.tensor([[d[n] for n in LAMBDAS] for d in self.lambdas], dtype=torch.float32), non_blocking=False)

    def load_stock(self, e, G, D):
        """Estimation e takes the parameters and power-iteration vectors of a stock Generator / Discriminator pair."""
        with torch.no_grad():
            for l, m in enumerate(G.layers()):
                self.gw[l][e].copy_(m.weight.detach().float())
            p, uv = pack_d(D)
            self.dp[e].copy_(p)
            self.uv[e].copy_(uv)

    def _check_in(self, t, shape, what):
        require_gpu(t, what)
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            raise _lib.EsrError('%s must be a contiguous fp32 tensor of shape %s, got %s %s' % (what, tuple(shape), t.dtype, tuple(t.shape)))

    # ---- G as one kernel
    def _compose(self):
        E, C, st = self.E, self.C, stream_ptr()
        src = self.gw[0]
        for l, (cin, cout, s, f) in enumerate(((C, C, 7, 5), (C, C, 11, 3), (C, C, 13, 1), (C, C, 13, 1), (C, 1, 13, 1)), start=1):
            _lib.check(_lib.lib.esr_kgan_compose(src.data_ptr(), self.gw[l].data_ptr(), self.K[l].data_ptr(), E, cin, cout, s, f, st), 'esr_kgan_compose')
            src = self.K[l]
        return self.K[5]

    def _compose_bwd(self, dk):
        """dk [E,13,13] -> the gradients of the six layers (into their .grad)."""
        E, C, st = self.E, self.C, stream_ptr()
        dout = dk
        for l, (cin, cout, s, f) in reversed(list(enumerate(((C, C, 7, 5), (C, C, 11, 3), (C, C, 13, 1), (C, C, 13, 1), (C, 1, 13, 1)), start=1))):
            src = self.gw[0] if l == 1 else self.K[l - 1]
            din = self.gw[0].grad if l == 1 else self.dK[l - 1]
            _lib.check(_lib.lib.esr_kgan_compose_bwd(src.data_ptr(), self.gw[l].data_ptr(), dout.data_ptr(), din.data_ptr(), self.gw[l].grad.data_ptr(),
                                                     E, cin, cout, s, f, st), 'esr_kgan_compose_bwd')
            dout = din

    def curr_k(self):
        """[E, 13, 13]: the kernels the generators imitate now."""
        return self._compose().reshape(self.E, 13, 13).clone()

    def _gb(self, H, W):
        b = self._g_bufs.get((H, W))
        if b is None:
            nblk = _lib.lib.esr_kgan_apply_blocks(H, W)
            _lib.check(min(nblk, 0), 'esr_kgan_apply_blocks')
            oh, ow = (H - 13) // 2 + 1, (W - 13) // 2 + 1
            f32 = dict(dtype=torch.float32, device=self.device)
            b = types.SimpleNamespace(oh=oh, ow=ow, nblk=nblk, y=torch.empty(self.E, 3, oh, ow, **f32), bic=torch.empty(self.E, oh, ow, **f32),
                                      partial=torch.zeros(self.E, nblk, **f32), dk=torch.empty(self.E, 13, 13, **f32),
                                      xin=torch.empty(2, self.E, 3, oh, ow, **f32))
            self._g_bufs[(H, W)] = b
        return b

    def apply_k(self, g_in, k, noise=None, y_noisy=None, bicubic=True):
        """y = (g_in corr k)[::2, ::2] (and the bicubic downscale with the partial sums of their squared distance) into the (H, W) buffers."""
        E, H, W = self.E, g_in.shape[2], g_in.shape[3]
        self._check_in(g_in, (E, 3, H, W), 'g_in')
        b = self._gb(H, W)
        _lib.check(_lib.lib.esr_kgan_apply(g_in.data_ptr(), k.data_ptr(), self.bict.data_ptr() if bicubic else None, _p(noise), b.y.data_ptr(), _p(y_noisy),
                                           b.bic.data_ptr() if bicubic else None, b.partial.data_ptr() if bicubic else None, E, H, W, stream_ptr()),
                   'esr_kgan_apply')
        return b

    def dk_from(self, g_in, dgan, bicubic=True):
        """dL/dk of the data terms from the buffers apply_k left: dgan [E,3,oh,ow] (or None) plus lambda_bicubic's term."""
        E, H, W = self.E, g_in.shape[2], g_in.shape[3]
        b = self._gb(H, W)
        _lib.check(_lib.lib.esr_kgan_dk(g_in.data_ptr(), b.y.data_ptr(), b.bic.data_ptr() if bicubic else None, _p(dgan), self.lam.data_ptr(),
                                        b.dk.data_ptr(), E, H, W, stream_ptr()), 'esr_kgan_dk')
        return b.dk

    def constraints(self, k, b, slot=None):
        """The constraint losses into self.losses and their gradient onto b.dk."""
        _lib.check(_lib.lib.esr_kgan_constraints(k.data_ptr(), b.dk.data_ptr(), self.mask.data_ptr(), self.lam.data_ptr(), b.partial.data_ptr(), b.nblk,
                                                 3 * b.oh * b.ow, self.losses.data_ptr(), None if slot is None else self.bic_log.data_ptr(), LOG_SLOTS,
                                                 0 if slot is None else int(slot), self.E, stream_ptr()), 'esr_kgan_constraints')

    # ---- the critic
    def critic(self, x, labels, scale, param_grads, data_grad):
        """x [npass, E, 3, H, W] through the critics (one power iteration per pass), the L1 loss of each pass against labels[pass], and its
        backward.  Returns the buffer set: pred, loss, and grad-per-pass gp / dx as asked; param_grads also leaves the summed gradient in dp.grad."""
        npass, E, _, H, W = x.shape
        self._check_in(x, (npass, E, 3, H, W), 'critic input')
        if E != self.E or npass not in (1, 2):
            raise _lib.EsrError('critic input must be [1 or 2, E, 3, H, W]')
        CD, st = self.CD, stream_ptr()
        b = self._critic_bufs.get((npass, H, W))
        if b is None:
            _lib.check(min(_lib.lib.esr_kgan_d_param_count(CD), 0), 'esr_kgan_d_param_count')
            if H < 7 or W < 7 or (H - 6) * (W - 6) > 2048:
                _lib.check(_lib.ESR_E_UNSUPPORTED, 'esr_kgan_d_forward (%d x %d input)' % (H, W))
            P = (H - 6) * (W - 6)
            f32 = dict(dtype=torch.float32, device=self.device)
            b = types.SimpleNamespace(P=P, wn=torch.zeros(npass, E, self.nd, **f32), uvs=torch.empty(npass, E, self.nuv, **f32),
                                      sigma=torch.empty(npass, E, 7, **f32), act=torch.empty(npass, E, 6, CD, P, **f32),
                                      xhat=torch.empty(npass, E, 6, CD, P, **f32), rstd=torch.empty(npass, E, 6, CD, **f32),
                                      pred=torch.empty(npass, E, H - 6, W - 6, **f32), loss=torch.empty(npass, E, **f32),
                                      dz6=torch.empty(npass, E, P, **f32), dz=torch.empty(npass, E, 6, CD, P, **f32),
                                      gp=torch.zeros(npass, E, self.nd, **f32), dx=torch.empty(npass, E, 3, H, W, **f32))
            self._critic_bufs[(npass, H, W)] = b
        L = _lib.lib
        _lib.check(L.esr_kgan_d_spectral(self.dp.data_ptr(), self.uv.data_ptr(), b.wn.data_ptr(), b.uvs.data_ptr(), b.sigma.data_ptr(), E, CD, npass, st),
                   'esr_kgan_d_spectral')
        gp = b.gp.data_ptr() if param_grads else None
        _lib.check(L.esr_kgan_d_forward(x.data_ptr(), self.dp.data_ptr(), b.wn.data_ptr(), b.act.data_ptr(), b.xhat.data_ptr(), b.rstd.data_ptr(),
                                        float(labels[0]), float(labels[-1]), float(scale), b.pred.data_ptr(), b.loss.data_ptr(), b.dz6.data_ptr(), gp,
                                        E, CD, H, W, npass, st), 'esr_kgan_d_forward')
        if param_grads or data_grad:
            _lib.check(L.esr_kgan_d_backward(x.data_ptr(), self.dp.data_ptr(), b.wn.data_ptr(), b.act.data_ptr(), b.xhat.data_ptr(), b.rstd.data_ptr(),
                                             b.dz6.data_ptr(), b.dz.data_ptr(), gp, b.dx.data_ptr() if data_grad else None, E, CD, H, W, npass, st),
                       'esr_kgan_d_backward')
        if param_grads:
            _lib.check(L.esr_kgan_d_finish(b.gp.data_ptr(), b.wn.data_ptr(), b.uvs.data_ptr(), b.sigma.data_ptr(), self.dp.grad.data_ptr(), E, CD, npass, st),
                       'esr_kgan_d_finish')
        return b

    # ---- one iteration
    def g_step(self, g_in, slot=None, update=True, keep_k=False):
        """The generators' step on the crops g_in [E,3,H,W]: L1(D(G(g_in)), 1) + the lambda-weighted constraints; Adam on G.
        keep_k: leave a copy of the kernel this step saw (before its update) in self.k_g — the reference's curr_k after its last iteration."""
        k = self._compose()
        if keep_k:
            self.k_g = k.reshape(self.E, 13, 13).clone()
        b = self.apply_k(g_in, k)
        c = self.critic(b.y.unsqueeze(0), (1.,), 1., False, True)
        self.loss_g = c.loss[0]
        self.dk_from(g_in, c.dx[0])
        self.constraints(k, b, slot)
        self._compose_bwd(b.dk)
        if update:
            self.optimizer_G.step()
        return b

    def d_step(self, g_in, d_in, fake_noise=None, update=True):
        """The critics' step: real crops d_in [E,3,oh,ow] (None: already gathered into the input buffer) against 1, G(g_in) + noise / 255
        with the updated generators against 0, half their sum; Adam on D."""
        E, H, W = self.E, g_in.shape[2], g_in.shape[3]
        b = self._gb(H, W)
        if d_in is not None:
            self._check_in(d_in, (E, 3, b.oh, b.ow), 'd_in')
            b.xin[0].copy_(d_in)
        if fake_noise is None:
            fake_noise = torch.randn(E, 3, b.oh, b.ow, dtype=torch.float32, device=self.device)
        self._check_in(fake_noise, (E, 3, b.oh, b.ow), 'fake_noise')
        self.apply_k(g_in, self._compose(), noise=fake_noise, y_noisy=b.xin[1], bicubic=False)
        c = self.critic(b.xin, (1., 0.), 0.5, True, False)
        self.loss_d = c.loss
        if update:
            self.optimizer_D.step()
        return c

    def step(self, g_in, d_in, fake_noise=None, slot=None):
        self.g_step(g_in, slot)
        self.d_step(g_in, d_in, fake_noise)

    # ---- crops from resident images
    def set_images(self, images, corners):
        """images: E arrays HWC in [0, 1]; corners int32 [iters, E, 4] = (top_g, left_g, top_d, left_d) per iteration."""
        if len(images) != self.E or corners.shape[1:] != (self.E, 4):
            raise _lib.EsrError('set_images wants E images and an [iters, E, 4] corner table')
        oh = (self.S - 13) // 2 + 1
        planes, meta, off = [], [], 0
        corners = np.asarray(corners)
        for e, im in enumerate(images):
            chw = np.ascontiguousarray(np.transpose(np.asarray(im, dtype=np.float32), (2, 0, 1)))
            H, W = chw.shape[1:]
            c = corners[:, e]
            if c.min() < 0 or (c[:, 0] + self.S > H).any() or (c[:, 1] + self.S > W).any() or (c[:, 2] + oh > H).any() or (c[:, 3] + oh > W).any():
                raise _lib.EsrError('a crop of image %d leaves the image' % e)
            planes.append(chw.reshape(-1))
            meta.append((off, H, W))
            off += chw.size
        self.imgs = torch.as_tensor(np.concatenate(planes), device=self.device)
        self.meta = torch.as_tensor(np.array(meta, dtype=np.int64), device=self.device)
        self.tl_g = torch.as_tensor(np.ascontiguousarray(corners[:, :, :2], dtype=np.int32), device=self.device)
        self.tl_d = torch.as_tensor(np.ascontiguousarray(corners[:, :, 2:], dtype=np.int32), device=self.device)
        self.g_in = torch.empty(self.E, 3, self.S, self.S, dtype=torch.float32, device=self.device)

    def step_at(self, it, real_noise, fake_noise, keep_k=False):
        """Iteration `it` on crops gathered from the resident images; real_noise / fake_noise [E,3,oh,ow] (N(0,1), scaled by 1/255 inside)."""
        if self.imgs is None:
            raise _lib.EsrError('step_at needs set_images first')
        b, st = self._gb(self.S, self.S), stream_ptr()
        _lib.check(_lib.lib.esr_kgan_gather(self.imgs.data_ptr(), self.meta.data_ptr(), self.tl_g[it].data_ptr(), None, self.g_in.data_ptr(), self.E, self.S,
                                            st), 'esr_kgan_gather')
        self._check_in(real_noise, (self.E, 3, b.oh, b.ow), 'real_noise')
        _lib.check(_lib.lib.esr_kgan_gather(self.imgs.data_ptr(), self.meta.data_ptr(), self.tl_d[it].data_ptr(), real_noise.data_ptr(), b.xin[0].data_ptr(),
                                            self.E, b.oh, st), 'esr_kgan_gather')
        self.g_step(self.g_in, slot=it % LOG_SLOTS, keep_k=keep_k)
        self.d_step(self.g_in, None, fake_noise)
