"""CPU tests of the random-alternatives Z objectives 'random_l1', 'random_l1_limited', 'random_VGG' (esr_hip/pairmin.py, Z_optimization.py;
reference codes/Z_optimization.py:365, :546-550, :683-701, :765-766): which names are accepted and refused, the CPU fallback against a float64
restatement and against the reference's own values (tests/golden/random_z.npz part (a), tools/gen_random_z_golden.py), the random_perturbations
and loss_values[0] rules, and a world-size-2 gloo run whose shards (2 + 1 samples) reproduce the single-process search."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle.weights import seeded_uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'random_z.npz')
RMSE_WEIGHT = 0.3            # of the fixture
FEATURE_GAIN = 4.0           # the fixture's stand-in extractor: netF(im) = 4 im


def _toy(batch, seed=0, output_image=True):
    from test_host_api import _ToyModel
    torch.manual_seed(seed)
    model = _ToyModel()
    lr = torch.rand(1, 3, 4, 4)
    model.feed_data({'LR': lr.expand(batch, -1, -1, -1), 'Z': torch.zeros(batch, 1, 16, 16)})
    model.test()
    if output_image:
        model.output_image = 1 * model.fake_H.detach()
    return model, lr


def _zo(objective, model, lr, batch=3, **kw):
    from Z_optimization import Z_optimizer
    kw.setdefault('data', {'LR': lr, 'rmse_weight': 0.5})
    kw.setdefault('max_iters', 3)
    return Z_optimizer(objective=objective, Z_size=[16, 16], model=model, Z_range=1, initial_LR=0.05, batch_size=batch, **kw)


# ------------------------------------------------------------------------------------------------ names
def test_names_are_accepted_or_refused():
    from Z_optimization import Z_optimizer
    model, lr = _toy(3)
    ones = np.ones((16, 16), np.float32)
    for name in ('random_l1', 'random_l1_limited', 'random_VGG'):
        assert name in Z_optimizer.SUPPORTED
        _zo(name, model, lr)
    for name in ('random_l1', 'random_l1_limited'):
        zo = _zo(name, model, lr, image_mask=ones.copy(), Z_mask=ones.copy(), initial_Z=torch.zeros(3, 1, 16, 16))
        assert zo.image_mask is not None
    with pytest.raises(NotImplementedError):                       # the mask broadcast cannot run on a feature map
        _zo('random_VGG', model, lr, image_mask=ones.copy(), Z_mask=ones.copy())
    with pytest.raises(NotImplementedError, match='random_VGG_limited'):
        _zo('random_VGG_limited', model, lr)
    for name in ('random_l1_local', 'random_l1_limited_local', 'random_l1_limited_local_STD', 'random_VGG_local'):
        with pytest.raises(NotImplementedError, match=name):
            _zo(name, model, lr)
    for name in ('random_l1', 'random_l1_limited', 'random_VGG'):
        with pytest.raises(NotImplementedError, match='training mode'):
            _zo(name, model, lr, HR_unpadder=lambda t: t)
    with pytest.raises(NotImplementedError):
        _zo('random_l2', model, lr)
    with pytest.raises(ValueError, match='rmse_weight'):
        _zo('random_l1_limited', model, lr, data={'LR': lr})
    bare, lr2 = _toy(3, output_image=False)
    with pytest.raises(ValueError, match='output_image'):
        _zo('random_l1_limited', bare, lr2)
    _zo('random_l1', bare, lr2)                                    # only '_limited' reads it


# ------------------------------------------------------------------------------------------------ the term
def loss64(x, clamp01=True, mask=None, init=None, w=0.0):
    """float64 restatement of the definition, one pair of rows at a time: Z_loss [B]"""
    x = x.double()
    D = torch.clamp(x, 0, 1) if clamp01 else x
    B = D.size(0)
    out = []
    for b in range(B):
        near = torch.ones_like(D[b])
        for a in range(B):
            if a != b:
                near = torch.minimum(near, (D[b] - D[a]).abs())
        v = near
        if init is not None:
            v = v - w * (D[b] - init[b if init.size(0) > 1 else 0].double()).abs()
        if mask is not None:
            v = v * mask.double()
        out.append(-v.mean())
    return torch.stack(out)


@pytest.mark.parametrize('B', [1, 2, 3, 5])
@pytest.mark.parametrize('masked,limited,clamp01', [(0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1), (0, 0, 0)])
def test_cpu_fallback_matches_float64(B, masked, limited, clamp01):
    from esr_hip import pairmin
    H, W = 9, 13
    x = seeded_uniform((B, 3, H, W), 1800 + B, -0.1, 1.1) * (1.0 if clamp01 else 3.0)
    mask = (seeded_uniform((H, W), 1801) > 0.3).float() if masked else None
    init = seeded_uniform((1 if B == 3 else B, 3, H, W), 1802, -0.1, 1.1) if limited else None
    xg = x.clone().requires_grad_(True)
    Z, share = pairmin.random_share(xg, clamp01=bool(clamp01), mask=mask, init=init, w=0.4)
    assert not Z.requires_grad and Z.shape == (B,)
    share.backward()
    x64 = x.double().requires_grad_(True)
    Z64 = loss64(x64, bool(clamp01), mask, init, 0.4)
    if Z64.requires_grad:                                        # (B = 1 without the limited term is the constant -mean(mask))
        Z64.mean().backward()
    else:
        x64.grad = torch.zeros_like(x64)
    np.testing.assert_allclose(Z.numpy(), Z64.detach().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(float(share.detach()), float(Z64.detach().mean()), rtol=1e-5, atol=1e-7)
    g64 = x64.grad.numpy()
    np.testing.assert_allclose(xg.grad.numpy(), g64, rtol=1e-5, atol=1e-5 * max(np.abs(g64).max(), 1e-12))
    if B == 1:
        assert float(Z64.detach()[0]) == pytest.approx(-(1.0 if mask is None else float(mask.mean())) + (0 if init is None else float(
            (0.4 * (torch.clamp(x, 0, 1) - init).abs() * (1 if mask is None else mask)).mean())), rel=1e-5)


def test_shares_of_a_split_batch_add_up_and_carry_the_remote_neighbour_terms():
    from esr_hip import pairmin
    B, H, W = 5, 9, 13
    x = seeded_uniform((B, 3, H, W), 1810, -0.1, 1.1)
    init = seeded_uniform((B, 3, H, W), 1811, -0.1, 1.1)
    mask = (seeded_uniform((H, W), 1812) > 0.3).float()
    xg = x.clone().requires_grad_(True)
    Z, share = pairmin.random_share(xg, mask=mask, init=init, w=0.4)
    share.backward()
    total, grads, vals = 0.0, [], []
    for lo, hi in ((0, 2), (2, 5)):
        xl = x[lo:hi].clone().requires_grad_(True)
        Zl, sh = pairmin.random_share(xl, x, lo, mask=mask, init=init[lo:hi], w=0.4)
        sh.backward()
        total += float(sh)
        grads.append(xl.grad)
        vals.append(Zl)
    np.testing.assert_allclose(total, float(share), rtol=1e-6)
    np.testing.assert_allclose(torch.cat(vals).numpy(), Z.numpy(), rtol=1e-6)
    np.testing.assert_allclose(torch.cat(grads).numpy(), xg.grad.numpy(), rtol=1e-6, atol=1e-9)
    # the local rows' own terms alone would miss what they receive as the nearest neighbour of remote rows
    xl = x[:2].clone().requires_grad_(True)
    full = torch.cat([xl, x[2:]], 0)
    (loss64(full, True, mask, init, 0.4)[:2].sum() / B).backward()
    assert float((xl.grad.float() - grads[0]).abs().max()) > 0


def fixture_cases(g):
    return sorted({k.rsplit('/', 1)[0] for k in g.files if k.startswith('a/') and k.endswith('/x')})


def run_fixture_case(g, key, device='cpu'):
    """(Z_loss, share, d share / dx) of esr_hip.pairmin on the case's inputs"""
    from esr_hip import pairmin
    x = torch.from_numpy(g[key + '/x']).to(device).requires_grad_(True)
    feat = key == 'a/feat'
    masked, limited = (not feat) and '_m1' in key, (not feat) and '_l1' in key
    mask = torch.from_numpy(g['a/mask']).to(device) if masked else None
    init = torch.from_numpy(g[key + '/init']).to(device) if limited else None
    D = FEATURE_GAIN * torch.clamp(x, 0, 1) if feat else x
    Z, share = pairmin.random_share(D, clamp01=not feat, mask=mask, init=init, w=RMSE_WEIGHT)
    share.backward()
    return Z.cpu().numpy(), float(share.detach()), x.grad.cpu().numpy()


def test_function_level_values_match_the_reference_on_cpu():
    g = np.load(GOLDEN)
    cases = fixture_cases(g)
    assert len(cases) == 13 and 'a/feat' in cases
    for key in cases:
        Z, share, dx = run_fixture_case(g, key)
        np.testing.assert_allclose(Z, g[key + '/Z_loss'], rtol=1e-5, atol=1e-7, err_msg=key)
        np.testing.assert_allclose(share, float(g[key + '/loss']), rtol=1e-5, atol=1e-7, err_msg=key)
        gr = g[key + '/grad']
        np.testing.assert_allclose(dx, gr, rtol=1e-5, atol=1e-5 * max(np.abs(gr).max(), 1e-12), err_msg=key)
    assert float(g['a/B1_m0_l0/Z_loss'][0]) == -1.0                 # a single sample: the constant 1
    feat = torch.from_numpy(g['a/feat/x'])
    assert float((FEATURE_GAIN * torch.clamp(feat, 0, 1)).max()) > 1     # the diagonal's cap is exercised


# ------------------------------------------------------------------------------------------------ the optimizer's rules
def test_random_perturbations_rule(monkeypatch):
    """reference :365: (random_Z_inits and 'random' not in objective) or ('random' in objective and 'limited' in objective)"""
    import Z_optimization
    seen = []
    orig = Z_optimization.Optimizable_Z.__init__

    def spy(self, *a, **k):
        seen.append(k.get('random_perturbations'))
        orig(self, *a, **k)
    monkeypatch.setattr(Z_optimization.Optimizable_Z, '__init__', spy)
    model, lr = _toy(3)
    z0 = torch.zeros(3, 1, 16, 16)
    expect = {('random_l1', False): False, ('random_l1', True): False, ('random_VGG', True): False, ('random_l1_limited', False): True,
              ('random_l1_limited', True): True, ('max_STD', False): False, ('max_STD', True): True, ('TV', True): True}
    for (name, flag), want in expect.items():
        del seen[:]
        zo = _zo(name, model, lr, initial_Z=z0.clone(), random_Z_inits=flag)
        assert seen == [want], (name, flag, seen)
        moved = bool((zo.Z_model.Z.data != 0).any())
        assert moved == want, (name, flag)


def test_limited_replaces_the_first_loss_value_by_the_second():
    z0 = seeded_uniform((3, 1, 16, 16), 1820, -0.2, 0.2)
    seen = {}
    for name in ('random_l1', 'random_l1_limited'):
        model, lr = _toy(3)                  # (optimize() drops the model's output: a fresh one per search)
        zo = _zo(name, model, lr, initial_Z=z0.clone(), max_iters=5)
        zo.optimize()
        assert len(zo.loss_values) >= 2 and len(zo.latest_Z_loss_values) == 3
        seen[name] = zo.loss_values
    assert seen['random_l1'][0] != seen['random_l1'][1]
    assert seen['random_l1_limited'][0] == seen['random_l1_limited'][1]
    # a single value is left as it is (the reference raises IndexError there)
    model, lr = _toy(3)
    zo = _zo('random_l1_limited', model, lr, initial_Z=z0.clone(), max_iters=1)
    zo.optimize()
    assert len(zo.loss_values) == 1
    # re-entering with cur_iter = 0 re-randomises Z when random_Z_inits is on (GUI.py:2041-2042)
    zo = _zo('random_l1', model, lr, initial_Z=z0.clone(), max_iters=1, random_Z_inits=True)
    zo.optimize()
    first = zo.Z_model.Z.data.clone()
    zo.cur_iter = 0
    zo.optimize()
    assert not torch.equal(first, zo.Z_model.Z.data)


# ------------------------------------------------------------------------------------------------ sharding (world size 2, gloo)
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_zopt(D, objective, batch=3):
    from test_host_api import _ToyModel
    from Z_optimization import Z_optimizer
    torch.manual_seed(0)
    model = _ToyModel()
    lr = torch.rand(1, 3, 4, 4)
    lo, hi = D.shard_range(batch)
    z_model = seeded_uniform((batch, 1, 16, 16), 1830, -0.3, 0.3)           # the model's current output: every sample its own image
    model.feed_data({'LR': lr.expand(hi - lo, -1, -1, -1), 'Z': z_model[lo:hi]})
    model.test()
    model.output_image = 1 * model.fake_H.detach()
    z0 = seeded_uniform((batch, 1, 16, 16), 1831, -0.3, 0.3)
    mask = (seeded_uniform((16, 16), 1832) > 0.2).numpy().astype(np.float32)
    orig = torch.randn_like
    torch.randn_like = lambda t, **k: torch.zeros_like(t)                   # the 'limited' perturbation of the start: nothing random enters
    try:
        zo = Z_optimizer(objective=objective, Z_size=[16, 16], model=model, Z_range=1, max_iters=6, data={'LR': lr, 'rmse_weight': 0.3},
                         initial_LR=0.05, batch_size=batch, initial_Z=z0, image_mask=mask, Z_mask=np.ones((16, 16), np.float32))
    finally:
        torch.randn_like = orig
    Z = zo.optimize()
    return Z, zo.loss_values, zo.latest_Z_loss_values, (lo, hi)


def _worker(rank, world, port, q):
    for p in (ROOT, os.path.join(ROOT, 'explorable-super-resolution_amd'), os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from esr_hip import dist as D
    D.init_from_env(backend='gloo')
    gathered = D.all_gather_tensor(torch.full((2 - rank, 3), float(rank)), [2, 1])          # uneven shards: padded, then trimmed
    res = {}
    for objective in ('random_l1', 'random_l1_limited'):
        Z, losses, last, shard = _run_zopt(D, objective)
        res[objective] = (Z.numpy(), losses, last, shard)
    q.put((rank, gathered.numpy(), res))
    dist.destroy_process_group()


def test_sharded_search_matches_single_process():
    for p in (ROOT, os.path.join(ROOT, 'explorable-super-resolution_amd'), os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    from esr_hip import dist as D
    ref = {objective: _run_zopt(D, objective) for objective in ('random_l1', 'random_l1_limited')}
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in procs]
    res = sorted((q.get(timeout=180) for _ in range(world)), key=lambda t: t[0])
    [p.join(timeout=60) for p in procs]
    for _, gathered, _ in res:
        np.testing.assert_array_equal(gathered, np.array([[0.] * 3, [0.] * 3, [1.] * 3], dtype=np.float32))
    for objective, (Z_ref, loss_ref, last_ref, _) in ref.items():
        assert [r[2][objective][3] for r in res] == [(0, 2), (2, 3)]
        assert len(loss_ref) == 6 and loss_ref[-1] < loss_ref[0]
        for r in res:
            np.testing.assert_allclose(r[2][objective][1], loss_ref, rtol=1e-6, err_msg=objective)
        np.testing.assert_allclose(np.concatenate([r[2][objective][0] for r in res], 0), Z_ref.numpy(), rtol=1e-6,
                                   atol=1e-6 * float(Z_ref.abs().max()), err_msg=objective)      # 1e-6 of Z's scale: entries near 0 included
        np.testing.assert_allclose(sum((r[2][objective][2] for r in res), []), last_ref, rtol=1e-5, err_msg=objective)
