"""One kernel estimation: the GAN whose generator imitates the image's own downscaling kernel (the reference's codes/KernelGAN/kernelGAN.py).

KernelGAN(conf, engine='hip') runs on the esr_kgan_* kernels (esr_hip.kernelgan.KernelGanEngine with E = 1; KernelGAN.train.train_batch
runs E > 1); engine='stock' is the same algorithm from the torch.nn modules of networks.py, on CPU or GPU in fp32 or fp64 — the checker
of the HIP engine and its baseline on the device."""
import torch
import torch.nn.functional as F

from . import networks, util


class StockEngine:
    """One iteration from plain torch: train_g / train_d keep every loss as an attribute and leave the gradients in the parameters' .grad."""

    def __init__(self, conf, device='cpu', dtype=torch.float32, composed=True):
        self.conf, self.device, self.dtype, self.composed = conf, torch.device(device), dtype, composed
        self.G = networks.Generator(conf)
        self.D = networks.Discriminator(conf)
        self.G.apply(networks.weights_init_G)
        self.D.apply(networks.weights_init_D)
        self.G.to(device=self.device, dtype=dtype)
        self.D.to(device=self.device, dtype=dtype).train()
        self.d_input_shape = self.G.output_size
        self.d_output_shape = self.d_input_shape - self.D.forward_shave
        self.optimizer_G = torch.optim.Adam(self.G.parameters(), lr=conf.g_lr, betas=(conf.beta1, 0.999))
        self.optimizer_D = torch.optim.Adam(self.D.parameters(), lr=conf.d_lr, betas=(conf.beta1, 0.999))
        self.lambdas = dict(bicubic=5., sum2one=0.5, boundaries=0.5, centralized=0., sparse=0.)
        t = dict(device=self.device, dtype=dtype)
        self.bicubic_k = torch.as_tensor(util.bicubic_table(), **t)
        self.mask = torch.as_tensor(util.create_penalty_mask(conf.G_kernel_size, 30), **t)
        ks = conf.G_kernel_size
        self.indices = torch.arange(ks, **t)
        self.center = ks // 2 + 0.5 * (int(1 / conf.scale_factor) - ks % 2)
        self.curr_k = self.G.curr_k().detach()
        self.loss_bicubic = 0

    def bicubic_downscale(self, g_in, like):
        """8 x 8 taps, stride 2, padding 3, every output plane the sum over ALL input planes (upstream's expand(3, 3, 8, 8)), shaved to `like`."""
        c = g_in.shape[1]
        down = F.conv2d(g_in, self.bicubic_k.expand(c, c, 8, 8), stride=2, padding=3)
        sr, sc = down.shape[2] - like.shape[2], down.shape[3] - like.shape[3]
        return down[:, :, sr // 2:down.shape[2] - sr // 2 - sr % 2, sc // 2:down.shape[3] - sc // 2 - sc % 2]

    def constraint_losses(self, g_in, g_pred, k):
        S = k.sum()
        com = torch.stack(((k.sum(1) * self.indices).sum() / S, (k.sum(0) * self.indices).sum() / S))
        return dict(bicubic=F.mse_loss(g_pred, self.bicubic_downscale(g_in, g_pred)), sum2one=(1 - S).abs(), boundaries=(k * self.mask).abs().mean(),
                    centralized=((com - self.center) ** 2).mean(), sparse=(k.abs() ** 0.2).mean())

    def train_g(self, g_in, update=True):
        self.optimizer_G.zero_grad()
        g_pred = self.G(g_in, composed=self.composed)
        self.loss_g = (self.D(g_pred) - 1).abs().mean()
        k = self.G.curr_k()
        self.losses = self.constraint_losses(g_in, g_pred, k)
        total = self.loss_g + sum(self.lambdas[n] * v for n, v in self.losses.items())
        total.backward()
        self.curr_k, self.loss_bicubic, self.g_pred = k.detach(), self.losses['bicubic'].detach(), g_pred.detach()
        if update:
            self.optimizer_G.step()

    def train_d(self, g_in, d_in, fake_noise=None, update=True):
        self.optimizer_D.zero_grad()
        pred_real = self.D(d_in)
        with torch.no_grad():
            g_out = self.G(g_in, composed=self.composed)
            if fake_noise is None:
                fake_noise = torch.randn_like(g_out)
            fake = g_out + fake_noise / 255.
        pred_fake = self.D(fake)
        self.loss_d_real, self.loss_d_fake = (pred_real - 1).abs().mean(), pred_fake.abs().mean()
        self.loss_d = (self.loss_d_fake + self.loss_d_real) * 0.5
        self.loss_d.backward()
        if update:
            self.optimizer_D.step()

    def train(self, g_in, d_in, fake_noise=None):
        self.train_g(g_in)
        self.train_d(g_in, d_in, fake_noise)


class KernelGAN:
    """The reference's interface: train(g_input, d_input) per iteration, curr_k, loss_bicubic, the lambda_* coefficients and both optimizers."""

    def __init__(self, conf, engine='hip', device=None, dtype=torch.float32, composed=True):
        self.conf, self.engine = conf, engine
        if engine == 'stock':
            self.impl = StockEngine(conf, device or 'cpu', dtype, composed)
            self.d_input_shape = self.impl.d_input_shape
        elif engine == 'hip':
            from esr_hip.kernelgan import KernelGanEngine
            if dtype != torch.float32:
                from esr_hip import EsrError
                raise EsrError("the 'hip' kernel-estimation engine is fp32")
            self.impl = KernelGanEngine(1, conf, device or 'cuda')
            self.d_input_shape = (conf.input_crop_size - 13) // 2 + 1
        else:
            raise ValueError("engine must be 'hip' or 'stock', got %r" % (engine,))
        self.optimizer_G, self.optimizer_D = self.impl.optimizer_G, self.impl.optimizer_D
        self.iteration = 0

    def _lambdas(self):
        return self.impl.lambdas if self.engine == 'stock' else self.impl.lambdas[0]

    def _set_lambda(self, name, v):
        self._lambdas()[name] = float(v)
        if self.engine == 'hip':
            self.impl.push_lambdas()

    lambda_bicubic = property(lambda s: s._lambdas()['bicubic'], lambda s, v: s._set_lambda('bicubic', v))
    lambda_sum2one = property(lambda s: s._lambdas()['sum2one'], lambda s, v: s._set_lambda('sum2one', v))
    lambda_boundaries = property(lambda s: s._lambdas()['boundaries'], lambda s, v: s._set_lambda('boundaries', v))
    lambda_centralized = property(lambda s: s._lambdas()['centralized'], lambda s, v: s._set_lambda('centralized', v))
    lambda_sparse = property(lambda s: s._lambdas()['sparse'], lambda s, v: s._set_lambda('sparse', v))

    @property
    def curr_k(self):
        return self.impl.curr_k if self.engine == 'stock' else self.impl.curr_k()[0]

    @property
    def loss_bicubic(self):
        return self.impl.loss_bicubic if self.engine == 'stock' else self.impl.losses[0, 0]

    def train(self, g_input, d_input, fake_noise=None):
        if self.engine == 'stock':
            t = dict(device=self.impl.device, dtype=self.impl.dtype)
            self.impl.train(g_input.to(**t), d_input.to(**t), None if fake_noise is None else fake_noise.to(**t))
        else:
            self.impl.step(g_input.contiguous(), d_input.contiguous(), fake_noise)
        self.iteration += 1
