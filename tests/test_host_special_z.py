"""CPU tests of the patch-magnitude and periodicityPlus Z objectives' host side (esr_hip/patchmag.py, esr_hip/scribble.py::region_constraint,
Z_optimization.py; reference codes/Z_optimization.py:385-394, 450-455, 470-477, 717-726, 743-746, 799-806): the patch set and the desired
patches against what the reference built (fixture tests/golden/special_z.npz part (a), written by tools/gen_special_z_golden.py), the CPU
paths of the losses and their gradients against the reference's values, the constraint helper against F.l1_loss, the C-ABI's argument checks,
the names, their refusals and missing data, and a two-rank sharded patch-magnitude search with the region constraint equal to the
single-process one."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'special_z.npz')
INCREMENT = 0.03
NAMES = ('local_Mag_increase', 'local_Mag_decrease', 'local_STD_nonInt_periodicityPlus', 'local_STD_nonInt_periodicityPlus_1D',
         'nonInt_periodicityPlus', 'nonInt_periodicityPlus_1D')


def golden():
    return np.load(GOLDEN)


def mag_spec(g, sign):
    from esr_hip import patchmag
    mask = g['a/mask']
    I0 = torch.clamp(torch.from_numpy(g['a/x_init']), 0, 1)
    return patchmag.MagSpec(mask, mask.shape[0], mask.shape[1], I0[0], INCREMENT, 1 if sign == 'increase' else -1)


@pytest.mark.parametrize('sign', ['increase', 'decrease'])
def test_patch_set_and_desired_patches_are_the_references(sign):
    g = golden()
    spec = mag_spec(g, sign)
    ref = g['a/mag/%s/patches' % sign]
    assert ref.shape[0] > 30                                              # enough patches to mean something
    np.testing.assert_array_equal(spec.patches, ref)
    H, W = g['a/mask'].shape
    assert spec.corner_index.shape == (H - 6, W - 6) and spec.corner_index.dtype == np.int32
    y0, x0 = np.divmod(ref[:, 0], W)
    np.testing.assert_array_equal(spec.corner_index[y0, x0], np.arange(ref.shape[0]))
    assert (spec.corner_index >= 0).sum() == ref.shape[0]
    des = g['a/mag/%s/desired' % sign]
    np.testing.assert_allclose(spec.desired.numpy(), des, rtol=1e-5, atol=1e-7)
    # the fixture holds patches at the 1/255 STD floor (the constant block of the initial image): their desired patch is the flat patch itself
    flat = np.ptp(des, axis=0) == 0
    assert flat.any() and not flat.all()


@pytest.mark.parametrize('sign', ['increase', 'decrease'])
def test_cpu_patch_mag_and_gradient_match_the_reference(sign):
    from esr_hip import patchmag
    g = golden()
    spec = mag_spec(g, sign)
    x = torch.from_numpy(g['a/x']).requires_grad_(True)
    loss = patchmag.patch_mag(x, spec)
    print(sign, loss.detach().numpy(), g['a/mag/%s/loss' % sign])
    np.testing.assert_allclose(loss.detach().numpy(), g['a/mag/%s/loss' % sign], rtol=1e-5)
    loss.sum().backward()
    gr = g['a/mag/%s/grad' % sign]
    np.testing.assert_allclose(x.grad.numpy(), gr, rtol=1e-5, atol=1e-5 * np.abs(gr).max())


def plus_loss(g, case, x, device='cpu'):
    """the Plus objective as Z_optimizer.optimize() forms it, from the library's functions -> (loss [B], desired STD)"""
    from esr_hip import local
    mask = g['a/mask']
    H, W = mask.shape
    I0 = torch.from_numpy(g['a/x_init']).to(device)
    pairs = [local.ShiftPair(p, H, W, interpolated=True) for p in g['a/plus/%s/points' % case]]
    mt = torch.from_numpy(mask).to(device)
    if case != 'whole':
        ps = local.PatchSet(mask, H, W)
        std = lambda im: local.patch_std(im, ps)  # noqa: E731
    elif device == 'cpu':
        std = lambda im: torch.std(torch.clamp(im, 0, 1) * mt, dim=(1, 2, 3)).view(1, -1)  # noqa: E731
    else:
        from esr_hip import zobj
        std = lambda im: zobj.image_std(im, mt, clamp01=True).view(1, -1)  # noqa: E731
    desired = std(I0).detach() + INCREMENT
    return local.shift_l1(x, mt, pairs) + (20 * (std(x) - desired) ** 2).mean(), desired


@pytest.mark.parametrize('case', ['nonint1', 'nonint2', 'whole'])
def test_cpu_plus_loss_and_gradient_match_the_reference(case):
    g = golden()
    x = torch.from_numpy(g['a/x']).requires_grad_(True)
    loss, desired = plus_loss(g, case, x)
    np.testing.assert_allclose(desired.numpy(), g['a/plus/%s/desired_STD' % case], rtol=1e-5, atol=1e-7)
    print(case, loss.detach().numpy(), g['a/plus/%s/loss' % case])
    np.testing.assert_allclose(loss.detach().numpy(), g['a/plus/%s/loss' % case], rtol=1e-5)
    loss.sum().backward()
    gr = g['a/plus/%s/grad' % case]
    np.testing.assert_allclose(x.grad.numpy(), gr, rtol=1e-5, atol=1e-5 * np.abs(gr).max())


def test_whole_image_patch_set_and_no_patch():
    from esr_hip import patchmag
    I0 = torch.rand(3, 30, 41, generator=torch.Generator().manual_seed(1))
    spec = patchmag.MagSpec(None, 30, 41, I0, 0.02, 1)
    sel = spec.corner_index >= 0
    assert sel[0, 0] and 0.04 < sel.mean() < 0.12                        # roughly every 4th corner in each direction
    m = np.zeros((30, 41), np.float32)
    m[2:8, 3:15] = 1                                                     # 6 rows: no 7 x 7 window
    with pytest.raises(ValueError, match='no 7 x 7 patch'):
        patchmag.MagSpec(m, 30, 41, I0, 0.02, 1)
    with pytest.raises(ValueError, match='spec for'):
        patchmag.patch_mag(torch.rand(1, 3, 30, 40), spec)


def test_a_negative_target_std_is_kept():
    """s_p - increment < 0 flips the patch about its mean, as the reference's formula does"""
    from esr_hip import patchmag
    I0 = torch.rand(3, 9, 9, generator=torch.Generator().manual_seed(2)) * 0.01 + 0.5        # STD about 0.002 < 1/255: the floor, then - 0.03
    spec = patchmag.MagSpec(None, 9, 9, I0, 0.03, -1)
    assert spec.P == 1
    q = I0.mean(0)[:7, :7].reshape(-1)
    want = (q - q.mean()) / (1 / 255) * (1 / 255 - 0.03) + q.mean()
    np.testing.assert_allclose(spec.desired[:, 0].numpy(), want.numpy(), rtol=1e-5, atol=1e-7)
    assert float(((spec.desired[:, 0] - q.mean()) * (q - q.mean())).max()) <= 0


def test_region_constraint_equals_l1_loss():
    import torch.nn.functional as F
    from esr_hip import scribble
    gen = torch.Generator().manual_seed(3)
    B, H, W = 3, 21, 34
    x = (torch.rand(B, 3, H, W, generator=gen) * 1.2 - 0.1).requires_grad_(True)
    mask = (torch.rand(H, W, generator=gen) > 0.6).float().numpy() * 0.7             # a partial mask with values other than 1
    cm = torch.from_numpy((mask <= 0).astype(np.float32))
    for initial in (torch.rand(B, 3, H, W, generator=gen), torch.rand(1, 3, H, W, generator=gen)):
        got = scribble.region_constraint(x, mask, initial)
        want = F.l1_loss(torch.clamp(x, 0, 1) * cm, (initial * cm).expand(B, -1, -1, -1))
        np.testing.assert_allclose(float(got), float(want), rtol=1e-6)
        g1, = torch.autograd.grad(got, x)
        g2, = torch.autograd.grad(want, x)
        np.testing.assert_allclose(g1.numpy(), g2.numpy(), rtol=1e-6, atol=1e-9)
        spec = scribble.constraint_spec(mask, initial)                               # built once, and a shard's norm
        np.testing.assert_allclose(float(scribble.region_constraint(x, spec, norm=2 * B * 3 * H * W)), float(want) / 2, rtol=1e-6)


def test_the_six_names_are_listed():
    import Z_optimization as Z
    assert set(NAMES) == set(Z.MAG_OBJECTIVES + Z.PLUS_OBJECTIVES)
    for name in NAMES:
        assert name in Z.Z_optimizer.SUPPORTED, name


@pytest.mark.parametrize('objective', NAMES)
def test_missing_increment_and_training_mode(objective):
    from Z_optimization import Z_optimizer
    for data in (None, {'periodicity_points': [[2.5, 3.25]]}, {'STD_increment': None}):
        with pytest.raises(ValueError, match='STD_increment'):
            Z_optimizer(objective, [8, 8], model=None, Z_range=1, max_iters=1, initial_LR=0.1, data=data)
    with pytest.raises(NotImplementedError, match='HR_unpadder'):
        Z_optimizer(objective, [8, 8], model=None, Z_range=1, max_iters=1, initial_LR=0.1, data={'STD_increment': 0.01}, HR_unpadder=lambda t: t)


@pytest.mark.parametrize('objective', ['periodicityPlus', 'local_STD_periodicityPlus', 'periodicityPlus_1D', 'local_STD_periodicityPlus_1D'])
def test_the_integer_plus_form_is_refused_and_says_why(objective):
    from Z_optimization import Z_optimizer
    with pytest.raises(NotImplementedError, match='integer periodicityPlus'):
        Z_optimizer(objective, [8, 8], model=None, Z_range=1, max_iters=1, initial_LR=0.1, data={'STD_increment': 0.01})


@pytest.mark.parametrize('objective,match', [('local_STD_nonInt_periodicity_Plus', "'Plus' variant"), ('local_STD_Mag_increase', "'Mag' variant"),
                                             ('local_Mag_max', "'Mag' variant"), ('nonInt_periodicityPlus_2D', "'Plus' variant")])
def test_other_spellings_keep_their_refusal(objective, match):
    from Z_optimization import Z_optimizer
    with pytest.raises(NotImplementedError, match=match):
        Z_optimizer(objective, [8, 8], model=None, Z_range=1, max_iters=1, initial_LR=0.1, data={'STD_increment': 0.01})


def test_c_abi_rejects_null_and_empty_arguments_without_a_gpu():
    from esr_hip import _lib
    lib = _lib.load_library()
    p = C.c_void_p(16)                      # never dereferenced: the checks come first
    E = _lib.ESR_E_ARG
    assert lib.esr_patch_mag(None, 1, 3, 16, 16, p, p, 4, p, None) == E
    assert lib.esr_patch_mag(p, 1, 3, 16, 16, None, p, 4, p, None) == E
    assert lib.esr_patch_mag(p, 1, 3, 16, 16, p, None, 4, p, None) == E
    assert lib.esr_patch_mag(p, 1, 3, 16, 16, p, p, 4, None, None) == E
    assert lib.esr_patch_mag(p, 0, 3, 16, 16, p, p, 4, p, None) == E
    assert lib.esr_patch_mag(p, 1, 3, 16, 16, p, p, 0, p, None) == E              # no patch
    assert lib.esr_patch_mag(p, 1, 3, 6, 16, p, p, 4, p, None) == E               # smaller than one window
    assert lib.esr_patch_mag(p, 70000, 3, 16, 16, p, p, 4, p, None) == _lib.ESR_E_UNSUPPORTED
    assert lib.esr_patch_mag_grad(p, 1, 3, 16, 16, p, p, 4, None, p, 0, None) == E
    assert lib.esr_patch_mag_grad(p, 1, 3, 16, 16, p, p, 4, p, None, 0, None) == E
    assert lib.esr_patch_mag_grad(p, 1, 0, 16, 16, p, p, 4, p, p, 0, None) == E
    assert lib.esr_patch_mag_grad(p, 1, 3, 16, 16, p, p, -1, p, p, 0, None) == E
    assert lib.esr_patch_mag_blocks(16, 16) == 1 and lib.esr_patch_mag_blocks(512, 384) == 32 * 6 and lib.esr_patch_mag_blocks(6, 16) == 0


# ---- Z_optimizer on a toy model: the loop's branches, the constraint's weight, and a sharded search
def _paths():
    for p in (ROOT, os.path.join(ROOT, 'explorable-super-resolution_amd'), os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)


def _toy_mask():
    mask = np.zeros((16, 16), np.float32)
    mask[2:14, 3:13] = 1
    return mask


def _run_mag(D, batch, objective='local_Mag_increase', non_local=True, iters=5):
    from test_host_api import _ToyModel
    from Z_optimization import Z_optimizer
    torch.manual_seed(0)
    model = _ToyModel()
    lr = torch.rand(1, 3, 4, 4)
    lo, hi = D.shard_range(batch)
    z0 = (torch.arange(batch).float().view(-1, 1, 1, 1) * 0.1 - 0.1) * torch.ones(batch, 1, 16, 16)
    model.feed_data({'LR': lr.expand(hi - lo, -1, -1, -1), 'Z': z0[lo:hi]})
    model.test()
    mask = _toy_mask()
    z1 = z0 + 0.05 * torch.rand(batch, 1, 16, 16)                        # away from the initial output: no ties in the constraint
    zo = Z_optimizer(objective=objective, Z_size=[16, 16], model=model, Z_range=1, max_iters=iters, initial_LR=0.05, batch_size=batch, initial_Z=z1,
                     data={'LR': lr, 'STD_increment': 0.03, 'periodicity_points': [[2.5, 1.25]]}, image_mask=mask, Z_mask=mask,
                     non_local_Z_optimization=non_local)
    Z = zo.optimize()
    return Z, zo.loss_values, (lo, hi), zo


def test_z_optimizer_runs_every_name_with_and_without_the_constraint():
    _paths()
    from esr_hip import dist as D
    from esr_hip import scribble
    for objective in NAMES:
        for non_local in (False, True):
            Z, losses, _, zo = _run_mag(D, 3, objective, non_local, iters=3)
            assert len(losses) >= 1 and np.isfinite(losses).all() and Z.shape == (3, 1, 16, 16)
            assert zo.non_local_Z_optimization == non_local
            np.testing.assert_array_equal(np.asarray(zo.Z_mask), scribble.rebuilt_z_mask(_toy_mask()) if non_local else _toy_mask())
            assert zo.constraining_loss_weight == pytest.approx(255 / 10 * 0.03 ** 2 if 'Mag' in objective else 0.1)
    # on a full mask the flag changes nothing
    from test_host_api import _ToyModel
    from Z_optimization import Z_optimizer
    model = _ToyModel()
    lr = torch.rand(1, 3, 4, 4)
    model.feed_data({'LR': lr, 'Z': torch.zeros(1, 1, 16, 16)})
    model.test()
    ones = np.ones((16, 16), np.float32)
    zo = Z_optimizer('local_Mag_decrease', [16, 16], model=model, Z_range=1, max_iters=1, initial_LR=0.05, data={'LR': lr, 'STD_increment': 0.03},
                     initial_Z=torch.zeros(1, 1, 16, 16), image_mask=ones, Z_mask=ones, non_local_Z_optimization=True)
    assert not zo.non_local_Z_optimization


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    _paths()
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from esr_hip import dist as D
    D.init_from_env(backend='gloo')
    Z, losses, shard, zo = _run_mag(D, 4)
    q.put((rank, Z.numpy(), losses, shard, zo.mag.desired.numpy()))
    dist.destroy_process_group()


def test_sharded_mag_search_with_the_constraint_matches_single_process():
    _paths()
    from esr_hip import dist as D
    Z_ref, loss_ref, _, zo = _run_mag(D, 4)
    assert zo.non_local_Z_optimization and loss_ref[0] > 0
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in procs]
    res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    [p.join(timeout=60) for p in procs]
    assert [r[3] for r in res] == [(0, 2), (2, 4)]
    # rank 1's own first image is sample 2: it must aim at rank 0's desired patches all the same
    np.testing.assert_array_equal(res[1][4], res[0][4])
    np.testing.assert_array_equal(res[0][4], zo.mag.desired.numpy())
    np.testing.assert_allclose(np.concatenate([r[1] for r in res], 0), Z_ref.numpy(), atol=1e-6)
    np.testing.assert_allclose(res[0][2], loss_ref, rtol=1e-5)
    np.testing.assert_allclose(res[1][2], loss_ref, rtol=1e-5)
