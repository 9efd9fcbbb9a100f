#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY (CPU, build container): writes tests/golden/random_z.npz by running the REFERENCE's own Z_optimizer
(codes/Z_optimization.py:331-400, 546-550, 647-797) with the objectives 'random_l1', 'random_l1_limited' and 'random_VGG', imported read-only
through oracle/_refshim.  Run:
    python tools/gen_random_z_golden.py

The reference has no loss object for these names: the expression is inline in optimize() (:683-701).  So
(a) function level: optimize() runs for ONE iteration on a stand-in model whose generator is the identity, feed_data / test setting
    fake_H = 0.5 + Z with Z_range 0.6, started from initial_Z = x - 0.5 for a seeded x of 12 x 18 (non-square) spanning [-0.1, 1.1].  Cases
    a/B<B>_m<0|1>_l<0|1>: B in {1, 2, 5}, without / with masks (an irregular image mask, Z mask of ones), 'random_l1' / 'random_l1_limited'
    (rmse weight 0.3, the model's output_image a second seeded image, un-clamped, of batch B - batch 1 for B = 5 with masks).  The limited
    cases end in the reference's IndexError at :766 (loss_values[0] = loss_values[1] with one value), after everything recorded here is set.
    a/feat: 'random_VGG' with B = 3 and the stand-in extractor netF(im) = 4 im, whose values exceed 1, so that the diagonal's cap at 1 shows.
      <case>/x        the fake_H the reference evaluated (0.5 + Z after the tanh round trip and, for 'limited', its random perturbation)
      <case>/init     the model's output_image (limited cases)
      <case>/Z_loss   latest_Z_loss_values [B];  <case>/loss  loss_values[0];  <case>/grad  the gradient that reached data['Z'] = d loss / d x
    a/mask: the image mask.
(b) Z_optimizer(...).optimize() on the F7 model (oracle/gen_golden.py::gen_F7: RRDB-1, latent 3, LR 24 x 28 -> HR 96 x 112), B = 3, 4 iterations,
    Adam lr 0.1, the seeded LR of tools/gen_scribble_golden.py, the search started from a seeded Z (seed 940), random_Z_inits=False: 'random_l1' with the masks of
    tools/gen_local_z_golden.py::z_masks ('l1_masks') and 'random_l1_limited' without masks, rmse weight 0.3, on the model's output for a second
    seeded Z, seed 921 ('limited').  The +0.001 randn perturbation the reference gives the initial Z of 'limited' (:286, :365) is pinned to zero here (torch.normal
    patched while the optimizer is constructed) so that nothing random enters; a test pins the product's perturbation the same way.
      b/<run>/loss, b/<run>/Z_loss (latest_Z_loss_values), b/<run>/final_Z_sub (Z[:, :, ::8, ::8]); b/mask/{image,Z}
      b/<run>/final_Z_moved: (median |dZ|, share of entries with |dZ| > 1e-2) of final_Z_sub between the run and its perturbed repeat below.  An Adam
      step moves an entry by about lr = 0.1 in the direction of its gradient's sign however small the gradient: entries whose gradient is at
      rounding level end somewhere else in any two runs that differ at rounding level, and this is how many of them there are.
    Stability: the loss is a min, so its history must not hinge on arg-min flips.  Each run is repeated with the LR input perturbed by 2e-5
    relative (the documented distance of the 'split' generator from the fp32 oracle) and the two histories must agree to 1e-4 relative, a tenth
    of the bar the GPU test holds the product to, and the sample with the smallest final value (the one the GUI would pick) must be the same
    and ahead of the runner-up by 5 times what the perturbation moved the values; otherwise pick other seeds before committing the fixture.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import _refshim  # noqa: E402
from oracle.weights import fill_formula_weights, seeded_uniform  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
H, W = 12, 18
Z_RANGE = 0.6
RMSE_WEIGHT = 0.3
FEATURE_GAIN = 4.0


def mask_a():
    m = (seeded_uniform((H, W), 1700).numpy() > 0.25).astype(np.float32)
    m[:2] = 0
    m[:, 15:] = 0
    m[5:9, 3:10] = 1
    return m


class _Identity:
    """what Z_optimizer reads of a model, with the identity as the generator: fake_H = 0.5 + Z"""

    def __init__(self, x, output_image=None):
        self.fake_H = x
        self.output_image = output_image
        self.num_latent_channels = 3
        self.netG = torch.nn.Linear(1, 1)
        self.cur_Z = x - 0.5
        self.Z = None

    def netF(self, im):
        return FEATURE_GAIN * im

    def Output_Batch(self, within_0_1=False):
        return torch.clamp(self.fake_H, 0, 1) if within_0_1 else self.fake_H

    def GetLatent(self):
        return self.cur_Z

    def feed_data(self, data, need_GT=False, **kw):
        self.Z = data['Z']
        self.Z.retain_grad()

    def test(self, prevent_grads_calc=False, **kw):
        self.fake_H = 0.5 + self.Z


def part_a(Z_optimizer, out):
    mask = mask_a()
    out['a/mask'] = mask
    cases = [('a/B%d_m%d_l%d' % (B, m, l), B, m, l, 'random_l1_limited' if l else 'random_l1') for B in (1, 2, 5) for m in (0, 1) for l in (0, 1)]
    cases.append(('a/feat', 3, 0, 0, 'random_VGG'))
    for n, (key, B, masked, limited, objective) in enumerate(cases):
        torch.manual_seed(1710 + n)                       # the reference's randn perturbation of 'limited'
        x0 = seeded_uniform((B, 3, H, W), 1720 + n, -0.1, 1.1)
        init = seeded_uniform((1 if (B == 5 and masked) else B, 3, H, W), 1760 + n, -0.1, 1.1) if limited else None
        model = _Identity(x0.clone(), init)
        kw = dict(image_mask=mask.copy(), Z_mask=np.ones((H, W), np.float32)) if masked else {}
        with contextlib.redirect_stdout(io.StringIO()):
            zo = Z_optimizer(objective=objective, Z_size=[H, W], model=model, Z_range=Z_RANGE, max_iters=1, data={'rmse_weight': RMSE_WEIGHT},
                             initial_Z=x0 - 0.5, initial_LR=0.1, batch_size=B, **kw)
            try:
                zo.optimize()
                assert not limited
            except IndexError:
                assert limited                            # :766 with a single loss value
        out[key + '/x'] = model.fake_H.detach().numpy().copy()
        if limited:
            out[key + '/init'] = init.numpy()
        out[key + '/Z_loss'] = np.array(zo.latest_Z_loss_values, dtype=np.float64)
        out[key + '/loss'] = np.float64(zo.loss_values[0])
        out[key + '/grad'] = model.Z.grad.numpy().copy()
        print(key, out[key + '/Z_loss'], float(np.abs(out[key + '/grad']).sum()))


@contextlib.contextmanager
def no_perturbation():
    orig = torch.normal
    torch.normal = lambda mean, std, **k: 1 * mean            # (:286: torch.normal(mean=zeros, std=0.001 ones))
    try:
        yield
    finally:
        torch.normal = orig


def part_b(Z_optimizer, out):
    from oracle.gen_golden import _ref_opt
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from gen_local_z_golden import z_masks
    import models
    quiet = contextlib.redirect_stdout(io.StringIO())
    with quiet:
        m = models.create_model(_ref_opt(False))
    fill_formula_weights(m.netG, gain=0.5)
    Bz = 3
    im_mask, z_mask = z_masks()
    out['b/mask/image'], out['b/mask/Z'] = im_mask, z_mask

    def run(name, lr):
        z0 = seeded_uniform((Bz, 3, 96, 112), 921, -0.3, 0.3)
        z1 = seeded_uniform((Bz, 3, 96, 112), 940, -0.3, 0.3)
        m.feed_data({'LR': lr.expand(Bz, -1, -1, -1).clone(), 'Z': z0.clone()}, need_GT=False)
        m.test()
        data = {'LR': lr.expand(Bz, -1, -1, -1).clone(), 'rmse_weight': RMSE_WEIGHT}
        kw = dict(image_mask=im_mask.copy(), Z_mask=z_mask.copy()) if name == 'l1_masks' else {}
        with quiet, no_perturbation():
            zo = Z_optimizer(objective='random_l1' if name == 'l1_masks' else 'random_l1_limited', Z_size=[96, 112], model=m, Z_range=1, max_iters=4,
                             data=data, initial_Z=z1.clone(), initial_LR=0.1, batch_size=Bz, random_Z_inits=False, **kw)
        with quiet:
            z = zo.optimize()
        return np.array(zo.loss_values, dtype=np.float64), np.array(zo.latest_Z_loss_values, dtype=np.float64), z[:, :, ::8, ::8].numpy().copy()

    lr = seeded_uniform((1, 3, 24, 28), 920)
    for name in ('l1_masks', 'limited'):
        loss, last, zsub = run(name, lr)
        loss_p, last_p, zsub_p = run(name, lr * (1 + 2e-5))
        drift = float(np.max(np.abs(loss_p - loss) / np.abs(loss)))
        margin, moved = float(np.diff(np.sort(last)[:2])[0]), float(np.abs(last_p - last).max())
        print(name, loss, last, 'history drift under a 2e-5 input perturbation: %.2e; best sample ahead by %.2e, values moved by %.2e' % (drift, margin, moved))
        assert len(loss_p) == len(loss) and drift < 1e-4, 'the loss history hinges on arg-min flips: pick other seeds'
        assert np.argmin(last_p) == np.argmin(last) and margin > 5 * moved, 'the best sample is not clearly best: pick other seeds'
        key = 'b/%s/' % name
        out[key + 'loss'], out[key + 'Z_loss'], out[key + 'final_Z_sub'] = loss, last, zsub
        dz = np.abs(zsub_p - zsub)
        out[key + 'final_Z_moved'] = np.array([np.median(dz), np.mean(dz > 1e-2)], dtype=np.float64)
        print(name, 'final Z under the perturbation: median |dZ| %.2e, share moved by more than 1e-2: %.4f' % tuple(out[key + 'final_Z_moved']))


def main():
    _refshim.install()
    np.bool = bool                     # the reference's np.bool (removed from NumPy); set after SciPy has imported
    import Z_optimization
    out = {}
    part_a(Z_optimization.Z_optimizer, out)
    if '--part-a-only' not in sys.argv:
        part_b(Z_optimization.Z_optimizer, out)
    np.savez_compressed(os.path.join(GOLDEN, 'random_z.npz'), **out)


if __name__ == '__main__':
    main()
