"""CPU tests of the scribble Z objective's host side (esr_hip/scribble.py, Z_optimization.py; reference codes/Z_optimization.py:344-364,
385-390, 401-448, 743-746): the CPU path against the reference's values (fixture tests/golden/scribble.npz part (a), written by
tools/gen_scribble_golden.py), the HSV and dilation restatements, the label map, the C-ABI's argument checks, the refusals, and a two-rank
sharded search with the region constraint equal to the single-process one."""
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
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scribble.npz')


def golden():
    return np.load(GOLDEN)


def test_cpu_path_matches_the_reference():
    from esr_hip import scribble
    g = golden()
    I0 = torch.clamp(torch.from_numpy(g['a/x_init']), 0, 1)
    D = scribble.desired_image(g['a/desired_in'], g['a/scribble'], I0[0], 0.3)
    np.testing.assert_allclose(D, g['a/D'], rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(scribble.rebuilt_z_mask(g['a/mask']), g['a/Z_mask'])
    spec = scribble.ScribbleSpec(g['a/scribble'], g['a/mask'], D, constraint=True, initial=I0)
    x = torch.from_numpy(g['a/x']).requires_grad_(True)
    L, Cn = scribble.scribble_loss(x, spec)
    np.testing.assert_allclose(L.detach().numpy(), g['a/loss'], rtol=1e-5)
    np.testing.assert_allclose(float(Cn.detach()), float(g['a/constraint']), rtol=1e-5)
    L.sum().backward()
    gr = g['a/grad_loss']
    np.testing.assert_allclose(x.grad.numpy(), gr, rtol=1e-5, atol=1e-5 * np.abs(gr).max())
    x.grad = None
    scribble.scribble_loss(x, spec)[1].backward()
    gr = g['a/grad_constraint']
    np.testing.assert_allclose(x.grad.numpy(), gr, rtol=1e-5, atol=1e-5 * np.abs(gr).max())


def test_hsv_known_colours_and_round_trip():
    from esr_hip import scribble
    rgb = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [128, 128, 128], [0, 0, 0]], np.float64)
    hsv = scribble.rgb2hsv(rgb)
    np.testing.assert_allclose(hsv, [[0, 1, 255], [1 / 3, 1, 255], [2 / 3, 1, 255], [0, 0, 128], [0, 0, 0]], atol=1e-12)
    x = np.random.default_rng(3).uniform(0, 255, (50, 40, 3))
    np.testing.assert_allclose(scribble.hsv2rgb(scribble.rgb2hsv(x)), x, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(scribble.hsv2rgb(rgb.reshape(5, 1, 3) * 0 + [[[5 / 6, 0.5, 10]]]), [[[10, 5, 10]]] * 5)


def test_dilation_footprint_of_a_single_pixel():
    from esr_hip import scribble
    m = np.zeros((40, 44), np.float32)
    y0, x0 = 20, 17
    m[y0, x0] = 1
    d = scribble.dilate16(m)
    rows, cols = np.nonzero(d)
    assert (rows.min(), rows.max(), cols.min(), cols.max()) == (y0 - 7, y0 + 8, x0 - 7, x0 + 8) and d.sum() == 256
    z = scribble.rebuilt_z_mask(m)                             # below 48 px the interior E is empty
    np.testing.assert_array_equal(z, d)
    big = scribble.rebuilt_z_mask(np.zeros((60, 50), np.float32))
    assert big[24:36, 24:26].all() and big.sum() == 12 * 2


def test_label_map_encodes_every_kind():
    from esr_hip import scribble
    s = np.array([[0, 1, 2, 3, 4, 9], [9, 4, 1, 0, 50, 7]])
    lm = np.array([[1, 1, 1, 1, 1, 1], [1, 1, 0, 0, 1, 0]], np.float32)
    lab = scribble.label_map(s, lm, constraint=True)
    L1, CON = scribble.LAB_L1, scribble.LAB_CON
    np.testing.assert_array_equal(lab, [[0, L1, L1, L1, 1, 2], [2, 1, CON, CON, 3, CON]])
    assert not (scribble.label_map(s, lm, constraint=False) & CON).any()
    with pytest.raises(ValueError, match='at most 63'):
        scribble.label_map(np.arange(4, 4 + 64).reshape(8, 8), np.ones((8, 8)), False)


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from esr_hip import _lib
    lib = _lib.load_library()
    p = C.c_void_p(16)                      # never dereferenced: the checks come first
    E = _lib.ESR_E_ARG
    assert lib.esr_scribble(None, 1, 3, 16, 16, p, p, None, 0, p, None) == E
    assert lib.esr_scribble(p, 1, 3, 16, 16, None, p, None, 0, p, None) == E
    assert lib.esr_scribble(p, 1, 3, 16, 16, p, None, None, 0, p, None) == E
    assert lib.esr_scribble(p, 0, 3, 16, 16, p, p, None, 0, p, None) == E
    assert lib.esr_scribble(p, 4, 3, 16, 16, p, p, p, 2, p, None) == E          # I0 batch neither 1 nor B
    assert lib.esr_scribble_grad(p, 1, 3, 16, 16, p, p, None, 0, None, 0.0, p, 0, None) == E
    assert lib.esr_scribble_grad(p, 1, 3, 16, 0, p, p, None, 0, p, 0.0, p, 0, None) == E
    assert lib.esr_scribble_grad(p, 2, 3, 16, 16, p, p, p, 3, p, 0.0, p, 0, None) == E


def test_scribble_is_listed():
    from Z_optimization import Z_optimizer
    assert 'scribble' in Z_optimizer.SUPPORTED


def test_refusals_and_missing_data():
    from Z_optimization import Z_optimizer
    with pytest.raises(NotImplementedError, match="use 'l1'"):
        Z_optimizer('scribble', [8, 8], model=None, Z_range=1, max_iters=1, initial_LR=0.1)
    m = np.ones((8, 8), np.float32)
    m[:2] = 0
    with pytest.raises(NotImplementedError, match='HR_unpadder'):
        Z_optimizer('scribble', [8, 8], model=None, Z_range=1, max_iters=1, initial_LR=0.1, image_mask=m, Z_mask=m, HR_unpadder=lambda t: t)
    s = np.zeros((8, 8), np.int64)
    d = torch.zeros(1, 3, 8, 8)
    for data, key in (({'scribble_mask': s}, 'desired'), ({'desired': d}, 'scribble_mask'), (None, 'desired'),
                      ({'desired': d, 'scribble_mask': s + 2}, 'brightness_factor')):
        with pytest.raises(ValueError, match=key):
            Z_optimizer('scribble', [8, 8], model=None, Z_range=1, max_iters=1, initial_LR=0.1, image_mask=m, Z_mask=m, data=data)


# ---- a sharded search with the region constraint (the pattern of tests/test_dist_cpu.py::test_sharded_z_search_matches_single_process)
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_scribble(D, batch):
    from test_host_api import _ToyModel
    from Z_optimization import Z_optimizer
    torch.manual_seed(0)
    model = _ToyModel()
    lr = torch.rand(1, 3, 4, 4)
    lo, hi = D.shard_range(batch)
    z0 = (torch.arange(batch).float().view(-1, 1, 1, 1) * 0.1 - 0.1) * torch.ones(batch, 1, 16, 16)
    model.feed_data({'LR': lr.expand(hi - lo, -1, -1, -1), 'Z': z0[lo:hi]})
    model.test()
    mask = np.zeros((16, 16), np.float32)
    mask[4:12, 3:13] = 1
    s = np.zeros((16, 16), np.int64)
    s[4:8, 3:8] = 1
    s[8:12, 3:8] = 2
    s[4:12, 8:11] = 4
    s[4:12, 11:13] = 5
    desired = torch.rand(1, 3, 16, 16)
    zo = Z_optimizer(objective='scribble', Z_size=[16, 16], model=model, Z_range=1, max_iters=5, initial_LR=0.05, batch_size=batch, initial_Z=z0,
                     data={'LR': lr, 'desired': desired, 'scribble_mask': s, 'brightness_factor': 0.2}, image_mask=mask, Z_mask=mask,
                     non_local_Z_optimization=True)
    assert zo.non_local_Z_optimization and zo.scribble.initial.size(0) == hi - lo
    Z = zo.optimize()
    return Z, zo.loss_values, (lo, hi)


def _worker(rank, world, port, q):
    for p in (ROOT, os.path.join(ROOT, 'explorable-super-resolution_amd'), os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from esr_hip import dist as D
    D.init_from_env(backend='gloo')
    Z, losses, shard = _run_scribble(D, 4)
    q.put((rank, Z.numpy(), losses, shard))
    dist.destroy_process_group()


def test_sharded_scribble_search_with_the_constraint_matches_single_process():
    for p in (ROOT, os.path.join(ROOT, 'explorable-super-resolution_amd'), os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    from esr_hip import dist as D
    Z_ref, loss_ref, _ = _run_scribble(D, 4)
    assert loss_ref[0] > 0
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in procs]
    res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    [p.join(timeout=60) for p in procs]
    assert [r[3] for r in res] == [(0, 2), (2, 4)]
    np.testing.assert_allclose(np.concatenate([r[1] for r in res], 0), Z_ref.numpy(), atol=1e-6)
    np.testing.assert_allclose(res[0][2], loss_ref, rtol=1e-5)
    np.testing.assert_allclose(res[1][2], loss_ref, rtol=1e-5)
