"""Estimate the downscaling kernel of an image from the image alone — the reference's codes/KernelGAN/train.py call pattern:

    from KernelGAN import train as KernelGAN
    conf = KernelGAN.Config().parse(['--X4'])
    conf.LR_image = <HWC uint8 RGB>
    k = KernelGAN.train(conf)

train_batch estimates the kernels of several images in lock step in the same kernel launches (engine='hip')."""
import copy

import numpy as np
import torch

from .configs import Config  # noqa: F401
from .data import DataGenerator
from .kernelGAN import KernelGAN
from .learner import Learner
from .util import analytic_kernel, post_process_k


def _final(k, conf):
    k = post_process_k(k, n=conf.n_filtering)
    return analytic_kernel(k) if conf.X4 else k


def train(conf, engine='hip', device=None, dtype=torch.float32):
    """The kernel of conf.LR_image (x2, or x4 with conf.X4) as a float64 array."""
    if engine == 'hip':
        return train_batch([conf], engine='hip', device=device)[0]
    gan = KernelGAN(conf, engine=engine, device=device, dtype=dtype)
    learner = Learner()
    data = DataGenerator(conf, gan)
    dev = gan.impl.device
    for iteration in range(conf.max_iters):
        gan.train(data.next_crop(True, iteration, dev, dtype), data.next_crop(False, iteration, dev, dtype))
        learner.update(iteration, gan)
    return _final(gan.curr_k, conf)


def _confs(confs_or_images, conf):
    out = []
    for item in confs_or_images:
        if hasattr(item, 'LR_image'):
            out.append(item)
        else:
            c = copy.copy(conf if conf is not None else Config().parse([]))
            c.LR_image = item
            out.append(c)
    return out


def train_batch(confs_or_images, conf=None, engine='hip', device=None, generator=None):
    """Kernels of E images (configurations with .LR_image, or HWC uint8 RGB arrays sharing `conf`) — a list of arrays.  With engine='hip' all E
    run in the same launches; the shared options (channels, iterations, learning rates) are the first configuration's.  `generator`: the
    torch.Generator of the two noise streams (the device's default one otherwise)."""
    confs = _confs(confs_or_images, conf)
    if not confs:
        return []
    if engine != 'hip':
        return [train(c, engine=engine, device=device) for c in confs]
    from esr_hip.kernelgan import LOG_SLOTS, KernelGanEngine
    c0, E = confs[0], len(confs)
    eng = KernelGanEngine(E, c0, device or 'cuda')
    datas = [DataGenerator(c, g_input_shape=c0.input_crop_size, d_input_shape=(c0.input_crop_size - 13) // 2 + 1) for c in confs]
    eng.set_images([d.input_image for d in datas], np.stack([d.corner_table()[:c0.max_iters] for d in datas], axis=1))
    learners = [Learner() for _ in confs]
    ds = datas[0].d_input_shape
    noise = None
    for it in range(c0.max_iters):
        if it % LOG_SLOTS == 0:               # the noise of the next 200 iterations in two launches: [200, real / fake, E, 3, 26, 26]
            noise = torch.randn(min(LOG_SLOTS, c0.max_iters - it), 2, E, 3, ds, ds, dtype=torch.float32, device=eng.device, generator=generator)
        eng.step_at(it, noise[it % LOG_SLOTS, 0], noise[it % LOG_SLOTS, 1], keep_k=it == c0.max_iters - 1)
        if learners[0].lr_falls(it):
            for opt in (eng.optimizer_G, eng.optimizer_D):
                for group in opt.param_groups:
                    group['lr'] /= Learner.update_l_rate_rate
        if it and it % LOG_SLOTS == 0:        # the only host synchronisation: 200 recorded bicubic losses per estimation
            log = eng.bic_log.cpu().numpy()
            order = list(range(1, LOG_SLOTS)) + [0]            # slot = iteration % 200: iterations it - 199 .. it
            changed = [learners[e].replay(it, log[e, order], eng.lambdas[e]) for e in range(E)]
            if any(changed):
                eng.push_lambdas()
    ks = eng.k_g.cpu()             # the kernel the last G step saw, as the reference returns it
    return [_final(ks[e], confs[e]) for e in range(E)]
