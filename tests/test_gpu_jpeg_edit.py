"""GPU tests (-m gpu) of the JPEG decoder's editing tools: the kernels of csrc/esr_jpeg_edit.hip (esr_hip/jpeg_edit.py), the colour model's fused
colour conversion and Enforce_pair_Consistency, and the editing Z objectives through the colour model.

Bounds.  Each kernel is compared with a float64 restatement; its bar is 4 x the distance of the fp32 CPU expression (esr_hip.jpeg_edit's defining
torch expression) from that float64 result ON THE SAME INPUT, computed in the test, never a constant.  The CPU expressions of esr_hip.jpeg and
esr_hip.jpeg_edit are patched to raise while the GPU side runs, so a silent fallback cannot pass; the originals are kept in CPU[...] for the bar.

Shapes, the smallest that can go wrong.  The 8-point kernels give a workgroup 32 CONSECUTIVE blocks (row-major over h x w) of one image:
  'one'    1 x 1 block;
  'ragged' 5 x 7 = 35 blocks: one more tile than a workgroup's and not a multiple of 4 (the element-by-element coefficient path), tiles that run
           over several block rows, B = 3 with per-image tables (QF 10, 40, 80);
  'vector' 2 x 18 = 36 blocks: the 16-byte coefficient path with a partial second tile — and, with the coefficient pointer moved by 4 bytes, the
           element-by-element path on the same data, which must give the same bits.
A workgroup never holds more than one candidate, so 'one more than a launch's candidates per workgroup' is N = 2; N = 1 and N = 3 are covered too.
The 16-point kernel has the tile of esr_jpeg16.hip (16 blocks along w): 'one' 1 x 1, 'ragged' 2 x 17 with B = 3, 'vector' 2 x 20.
The colour conversion gives a thread 4 pixels and a workgroup 1024: 8 x 8 (one partial workgroup, 16-byte path), 5 x 7 with B = 3 (35 pixels:
element by element with a ragged tail), 33 x 32 (1056 pixels: a second workgroup)."""
import ctypes as C_

import numpy as np
import pytest
import torch

from oracle.weights import seeded_uniform
from test_host_jpeg_chroma import C, chroma_modules, gt as gt_chroma
from test_host_jpeg_edit import E, SRStandIn, check_enforce_pair_consistency, edit_case, make_model, poison_fake_H, run_edit_search

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CPU = {}                   # the fp32 CPU expressions, kept before they are patched


@pytest.fixture(autouse=True)
def no_cpu_fallback(monkeypatch):
    from esr_hip import jpeg as J, jpeg_edit

    def refuse(*a, **k):
        raise AssertionError('the CPU fallback ran in a GPU test')
    for mod, names in ((J, ('_compress_cpu', '_extract_cpu', '_compress16_cpu', '_extract16_cpu')),
                       (jpeg_edit, ('_ycbcr_to_rgb_cpu', '_violation_cpu', '_plane_cpu', '_chroma_cpu'))):
        for name in names:
            CPU.setdefault(name, getattr(mod, name))
            monkeypatch.setattr(mod, name, refuse)


def _cpu_expression(fn):
    """run fn with the CPU expressions in place (for the bar)"""
    from esr_hip import jpeg as J, jpeg_edit
    with pytest.MonkeyPatch.context() as mp:
        for mod in (J, jpeg_edit):
            for name, f in CPU.items():
                if hasattr(mod, name):
                    mp.setattr(mod, name, f)
        return fn()


def _stream():
    return C_.c_void_p(torch.cuda.current_stream().cuda_stream)


def _off_by_4_bytes(t):
    """a contiguous copy of t on the device whose pointer is 4 bytes past a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 1, device=DEV)
    buf[1:].copy_(t.reshape(-1))
    off = buf[1:].view(t.shape)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    return off


def _tables8(qf):
    from JPEG_module.JPEG import JPEG
    m = JPEG(compress=True, downsample_or_quantize=True)
    m.Set_Q_Table(torch.tensor(qf, dtype=torch.float32))
    return m.Q_table.reshape(len(qf), 64)


# ------------------------------------------------------------------------------------------------ colour conversion
def _rgb64(x):
    mat = torch.from_numpy(255 * E.YCBCR2RGB.transpose())
    return torch.einsum('rc,bchw->brhw', mat, x.double() / 255) + torch.from_numpy(E.YCBCR2RGB_OFFSET).view(1, 3, 1, 1) / 255


RGB_SHAPES = {'vector': (1, 8, 8), 'ragged': (3, 5, 7), 'two_workgroups': (2, 33, 32)}


@pytest.mark.parametrize('name', list(RGB_SHAPES))
def test_ycbcr_rgb_against_float64(name):
    from esr_hip import jpeg_edit
    B, H, W = RGB_SHAPES[name]
    x = seeded_uniform((B, 3, H, W), 9500, -20.0, 275.0)
    want = _rgb64(x)
    bar = 4 * float((_cpu_expression(lambda: jpeg_edit.ycbcr_to_rgb(x)).double() - want).abs().max())
    got = jpeg_edit.ycbcr_to_rgb(x.to(DEV))
    err = float((got.cpu().double() - want).abs().max())
    print('%s: kernel %.3g from float64 (bar %.3g)' % (name, err, bar))
    assert got.shape == x.shape and 0 < bar < 1e-5 and err <= bar
    assert torch.equal(got, jpeg_edit.ycbcr_to_rgb(x.to(DEV)))
    assert torch.equal(jpeg_edit.ycbcr_to_rgb(_off_by_4_bytes(x)), got)          # the element-by-element path: the same bits
    # the gradient through autograd: the transposed matrix / 255
    g = seeded_uniform((B, 3, H, W), 9501, -1.0, 1.0)
    xg = x.to(DEV).requires_grad_(True)
    (jpeg_edit.ycbcr_to_rgb(xg) * g.to(DEV)).sum().backward()
    x64 = x.double().requires_grad_(True)
    (_rgb64(x64) * g.double()).sum().backward()
    x32 = x.clone().requires_grad_(True)
    _cpu_expression(lambda: (jpeg_edit.ycbcr_to_rgb(x32) * g).sum().backward())
    gbar = 4 * float((x32.grad.double() - x64.grad).abs().max())
    assert 0 < gbar < 1e-7 and float((xg.grad.cpu().double() - x64.grad).abs().max()) <= gbar
    assert torch.equal(jpeg_edit._rgb_launch('esr_ycbcr_rgb_grad', _off_by_4_bytes(g)), jpeg_edit._rgb_launch('esr_ycbcr_rgb_grad', g.to(DEV)))


def test_ycbcr_rgb_grad_is_the_adjoint():
    """<A x, y> = <x, A^T y> with both sides from the kernels, A the linear part (the conversion of x minus that of a zero image), the sums
    taken in float64.  What is left is the fp32 round-off of the kernels' values: three multiply-adds, an offset and a division per value, at
    most 8 half-ulps of a value of the size of the result, so the two sums differ by at most 8 x 2^-24 x the sum of the absolute terms of both."""
    from esr_hip import jpeg_edit
    x, y = seeded_uniform((2, 3, 33, 32), 9510, -255.0, 255.0), seeded_uniform((2, 3, 33, 32), 9511, -1.0, 1.0)
    Ax = (jpeg_edit.ycbcr_to_rgb(x.to(DEV)) - jpeg_edit.ycbcr_to_rgb(torch.zeros_like(x).to(DEV))).cpu().double()
    Aty = jpeg_edit._rgb_launch('esr_ycbcr_rgb_grad', y.to(DEV)).cpu().double()
    lhs, rhs = float((Ax * y.double()).sum()), float((x.double() * Aty).sum())
    tol = 8 * 2.0 ** -24 * float((Ax.abs() * y.double().abs()).sum() + (x.double().abs() * Aty.abs()).sum())
    print('<Ax, y> = %.9g, <x, A^T y> = %.9g, tolerance %.3g' % (lhs, rhs, tol))
    assert abs(lhs) > 1 and abs(lhs - rhs) <= tol


# ------------------------------------------------------------------------------------------------ the 8-point kernels
SHAPES8 = {'one': (1, 1, 1, [25]), 'ragged': (3, 5, 7, [10, 40, 80]), 'vector': (2, 2, 18, [30, 75])}
_cases8 = {}


def _case8(name):
    """(desired / candidate images [B, 1, 8h, 8w], tables [B, 64], quantised coefficients of ANOTHER image [B, 64, h, w]) — built once per shape"""
    if name not in _cases8:
        B, h, w, qf = SHAPES8[name]
        seed = 9600 + 100 * len(_cases8)
        x, tables = C.Y.smooth_pattern(B, 8 * h, 8 * w, seed), _tables8(qf)
        # the code of a noisy copy: the clamp is active on some coefficients (small table entries) and idle on others
        coef = torch.round(C.Y.compress64(x + seeded_uniform(tuple(x.shape), seed + 50, -40.0, 40.0), tables)).float()
        _cases8[name] = (x, tables, coef)
    return _cases8[name]


def _score64(cand, coef, tables):
    return torch.clamp((C.Y.compress64(cand, tables) - coef.double()).abs() - 0.5, min=0).sum(dim=(1, 2, 3))


@pytest.mark.parametrize('name,shared', [('one', True), ('ragged', True), ('ragged', False), ('vector', False)])
def test_violation_against_float64(name, shared):
    """N = 1 ('one'), N = 3 with one coefficient tensor and table ('ragged', shared), N = 3 with per-candidate tables and coefficients, N = 2"""
    from esr_hip import jpeg_edit
    x, tables, coef = _case8(name)
    if shared:
        tables, coef = tables[:1], coef[:1]
    want = _score64(x, coef, tables)
    bar = 4 * float((_cpu_expression(lambda: jpeg_edit.consistency_violation(x, coef, tables)) - want).abs().max())
    got = jpeg_edit.consistency_violation(x.to(DEV), coef.to(DEV), tables.to(DEV))
    err = float((got.cpu() - want).abs().max())
    print('%s (N = %d, %s): scores %s, kernel %.3g from float64 (bar %.3g)' % (name, x.size(0), 'shared' if shared else 'per candidate', got.tolist(), err, bar))
    assert got.shape == (x.size(0),) and got.dtype == torch.float64 and float(want.min()) > 0.5 and bar > 0 and err <= bar
    assert torch.equal(got, jpeg_edit.consistency_violation(x.to(DEV), coef.to(DEV), tables.to(DEV)))          # two runs: identical bits
    if name == 'vector':
        assert torch.equal(jpeg_edit.consistency_violation(x.to(DEV), _off_by_4_bytes(coef), tables.to(DEV)), got)


def test_violation_ranks_as_float64():
    """nine candidates between an image and its imprint: float64 scores further apart than the bar, so the order must be float64's"""
    from esr_hip import jpeg_edit
    x, tables, _ = _case8('ragged')
    fixed, other = x[:1], x[1:2]
    coef = torch.round(C.Y.compress64(fixed, tables[:1])).float()
    steps = torch.tensor([0.9, 0.1, 0.5, 0.3, 0.7, 0.2, 0.8, 0.4, 0.6]).view(-1, 1, 1, 1)
    cand = fixed + steps * (other - fixed)
    want = _score64(cand, coef, tables[:1])
    bar = 4 * float((_cpu_expression(lambda: jpeg_edit.consistency_violation(cand, coef, tables[:1])) - want).abs().max())
    gaps = torch.diff(torch.sort(want).values)
    assert float(gaps.min()) > 2 * bar                              # (the condition on the inputs, checked on the CPU side)
    got = jpeg_edit.consistency_violation(cand.to(DEV), coef.to(DEV), tables[:1].to(DEV)).cpu()
    assert float((got - want).abs().max()) <= bar and torch.equal(torch.argsort(got), torch.argsort(want))
    assert torch.equal(torch.argsort(got), torch.argsort(steps.reshape(-1)))


@pytest.mark.parametrize('name', list(SHAPES8))
def test_pair_kernel_against_float64_and_the_composition(name):
    from esr_hip import jpeg as J, jpeg_edit
    x, tables, coef = _case8(name)
    d64 = C.Y.compress64(x, tables)
    want = C.Y.extract64(torch.clamp(d64 - coef.double(), -0.5, 0.5) + coef.double(), tables)
    active = float(((d64 - coef.double()).abs() > 0.5).double().mean())
    bar = 4 * float((_cpu_expression(lambda: jpeg_edit.consistent_plane(x, coef, tables)).double() - want).abs().max())
    xg, cg, tg = x.to(DEV), coef.to(DEV), tables.to(DEV)
    got = jpeg_edit.consistent_plane(xg, cg, tg)
    composed = J.extract(torch.clamp(J.compress(xg, tg, False) - cg, -0.5, 0.5) + cg, tg)[1]
    err, apart = float((got.cpu().double() - want).abs().max()), float((got - composed).abs().max())
    print('%s: clamp active on %.0f %%; fused %.3g from float64, %.3g from the composition of the kernels (bar %.3g)' % (name, 100 * active, err, apart, bar))
    assert got.shape == x.shape and 0.02 < active < 0.98 and bar > 0 and err <= bar and apart <= bar
    assert torch.equal(got, jpeg_edit.consistent_plane(xg, cg, tg))
    if name == 'vector':
        assert torch.equal(jpeg_edit.consistent_plane(xg, _off_by_4_bytes(coef), tg), got)


# ------------------------------------------------------------------------------------------------ the 16-point kernel
SHAPES16 = {'one': (1, 1, 1, [25]), 'ragged': (3, 2, 17, [10, 40, 80]), 'vector': (2, 2, 20, [30, 75])}


@pytest.mark.parametrize('name', list(SHAPES16))
def test_pair16_kernel_against_float64_and_the_composition(name):
    from esr_hip import jpeg as J, jpeg_edit
    B, h, w, qf = SHAPES16[name]
    x = C.ycbcr_pattern(B, 16 * h, 16 * w, 9800) + seeded_uniform((B, 3, 16 * h, 16 * w), 9801, -8.0, 8.0)        # high chroma frequencies to keep
    noisy = x + seeded_uniform(tuple(x.shape), 9850, -40.0, 40.0)
    padded = chroma_modules(torch.tensor(qf, dtype=torch.float32))['q'].padded_Q_table.reshape(B, 3, 256)
    coef = torch.round(C.compress64_16(noisy, padded)[:, 1:, :8, :8]).reshape(B, 128, h, w).float()
    d64 = C.compress64_16(x, padded)[:, 1:].clone()
    low = coef.double().reshape(B, 2, 8, 8, h, w)
    active = float(((d64[:, :, :8, :8] - low).abs() > 0.5).double().mean())
    d64[:, :, :8, :8] = torch.clamp(d64[:, :, :8, :8] - low, -0.5, 0.5) + low
    want = C.extract64_16(d64.reshape(B, 512, h, w), padded)
    bar = 4 * float((_cpu_expression(lambda: jpeg_edit.consistent_chroma(x, coef, padded)).double() - want).abs().max())
    xg, cg, tg = x.to(DEV), coef.to(DEV), padded.to(DEV)
    got = jpeg_edit.consistent_chroma(xg, cg, tg)
    full = J.compress16(xg, tg, False)[:, 256:].reshape(B, 2, 16, 16, h, w).clone()
    k = cg.reshape(B, 2, 8, 8, h, w)
    full[:, :, :8, :8] = torch.clamp(full[:, :, :8, :8] - k, -0.5, 0.5) + k
    composed = J.extract16(full.reshape(B, 512, h, w), tg)[1]
    err, apart = float((got.cpu().double() - want).abs().max()), float((got - composed).abs().max())
    print('%s: clamp active on %.0f %%; fused %.3g from float64, %.3g from the composition of the kernels (bar %.3g)' % (name, 100 * active, err, apart, bar))
    assert got.shape == (B, 2, 16 * h, 16 * w) and 0.02 < active < 0.98 and bar > 0 and err <= bar and apart <= bar
    assert torch.equal(got, jpeg_edit.consistent_chroma(xg, cg, tg))
    # two planes alone, the compressor's 384 channels read in place, and (w = 20) the coefficient pointer 4 bytes off: the same bits
    assert torch.equal(jpeg_edit.consistent_chroma(xg[:, 1:].contiguous(), cg, tg), got)
    assert torch.equal(jpeg_edit.consistent_chroma(xg, torch.cat([torch.zeros(B, 256, h, w, device=DEV), cg], 1), tg), got)
    if name == 'vector':
        assert torch.equal(jpeg_edit.consistent_chroma(xg, _off_by_4_bytes(coef), tg), got)


def test_bad_arguments_come_back_as_errors():
    from esr_hip import _lib
    x = torch.zeros(1, 3, 16, 16, device=DEV)
    o = torch.zeros(1, 3, 16, 16, device=DEV)
    q = torch.ones(1, 3, 256, device=DEV)
    d = torch.zeros(4, dtype=torch.float64, device=DEV)
    lib, s = _lib.lib, _stream()
    assert lib.esr_ycbcr_rgb(x.data_ptr(), 0, 16, 16, o.data_ptr(), s) == _lib.ESR_E_ARG
    assert lib.esr_ycbcr_rgb(None, 1, 16, 16, o.data_ptr(), s) == _lib.ESR_E_ARG
    assert lib.esr_jpeg_violation_partials(12, 16) == _lib.ESR_E_ARG and lib.esr_jpeg_violation_partials(64, 64) == 2
    assert lib.esr_jpeg_violation(x.data_ptr(), 1, 16, 12, x.data_ptr(), 1, q.data_ptr(), 1, d.data_ptr(), d.data_ptr(), s) == _lib.ESR_E_ARG
    assert lib.esr_jpeg_violation(x.data_ptr(), 3, 16, 16, x.data_ptr(), 2, q.data_ptr(), 1, d.data_ptr(), d.data_ptr(), s) == _lib.ESR_E_ARG
    assert lib.esr_jpeg_pair(x.data_ptr(), 1, 16, 20, x.data_ptr(), q.data_ptr(), o.data_ptr(), s) == _lib.ESR_E_ARG
    assert lib.esr_jpeg16_pair(x.data_ptr(), 4, 1, 16, 16, x.data_ptr(), 128, 0, q.data_ptr(), o.data_ptr(), s) == _lib.ESR_E_ARG
    assert lib.esr_jpeg16_pair(x.data_ptr(), 3, 1, 16, 16, x.data_ptr(), 128, 1, q.data_ptr(), o.data_ptr(), s) == _lib.ESR_E_ARG
    assert lib.esr_jpeg16_pair(x.data_ptr(), 3, 1, 16, 24, x.data_ptr(), 128, 0, q.data_ptr(), o.data_ptr(), s) == _lib.ESR_E_ARG


# ------------------------------------------------------------------------------------------------ the model
def test_model_output_and_enforce_pair_consistency(tmp_path):
    from esr_hip import jpeg_edit
    model = make_model(tmp_path, gpu=True)
    x, Z, qf = C.image_c(), C.latent_c(), torch.tensor(C.QF_C, dtype=torch.float32)
    model.feed_data({'Uncomp': x, 'QF': qf, 'Z': Z}, need_GT=False)
    model.test()
    rgb = model.Output_Batch(True)
    assert rgb.is_cuda and float(rgb.min()) >= 0 and float(rgb.max()) <= 1
    assert float((rgb.cpu() - gt_chroma('c/all_layers/rgb')).abs().max()) < 1e-3                   # the bar of tests/test_gpu_jpeg_chroma.py
    assert torch.equal(model.Output_Image_0_1(), jpeg_edit.ycbcr_to_rgb(model.output_image))
    check_enforce_pair_consistency(model)


# ------------------------------------------------------------------------------------------------ Z search
@pytest.mark.parametrize('objective', ['scribble', 'local_STD_increase', 'random_l1'])
def test_z_search_history_matches_the_cpu_path(tmp_path, objective, monkeypatch):
    """six iterations, GPU against this build's CPU path; rtol 1e-3, atol 1e-3 |loss[0]| and the final Z within 1e-2, as the existing JPEG search
    tests ('scribble' with the region constraint on the block grid, 'random_l1' with a batch of 2)"""
    (tmp_path / 'gpu').mkdir()
    (tmp_path / 'cpu').mkdir()
    gpu, gpu_Z, _ = run_edit_search(poison_fake_H(make_model(tmp_path / 'gpu', gpu=True)), objective, jpeg=True)
    monkeypatch.undo()                                              # the CPU side of the comparison runs the CPU expressions
    cpu, cpu_Z, _ = run_edit_search(make_model(tmp_path / 'cpu'), objective, jpeg=True)
    print('%s: GPU %s\n    CPU %s' % (objective, gpu.loss_values, cpu.loss_values))
    assert len(gpu.loss_values) == len(cpu.loss_values) == 6
    np.testing.assert_allclose(gpu.loss_values, cpu.loss_values, rtol=1e-3, atol=1e-3 * abs(cpu.loss_values[0]))
    assert gpu.loss_values[-1] < gpu.loss_values[0]
    assert float((gpu_Z.cpu() - cpu_Z).abs().max()) < 1e-2
    if objective == 'scribble':
        assert gpu.non_local_Z_optimization and np.array_equal(gpu.Z_mask, cpu.Z_mask)


@pytest.mark.parametrize('objective', ['patchdict_noDC', 'hist'])
def test_histogram_objectives_equal_sr_mode_on_the_rgb_output(tmp_path, objective):
    """The soft-histogram and KDE kernels have no CPU expression, so there is no CPU path to compare with: JPEG mode is held to its definition
    instead, the SR-mode objective on Output_Image_0_1(), six iterations, same bars."""
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    zo, Z, _ = run_edit_search(poison_fake_H(make_model(tmp_path / 'a', gpu=True)), objective, jpeg=True)
    sr, Z_sr, _ = run_edit_search(SRStandIn(make_model(tmp_path / 'b', gpu=True)), objective, jpeg=False)
    print('%s: JPEG mode %s\n    SR mode on Output_Image_0_1() %s' % (objective, zo.loss_values, sr.loss_values))
    assert zo.jpeg_mode and not sr.jpeg_mode and len(zo.loss_values) == len(sr.loss_values) and np.all(np.isfinite(zo.loss_values))
    np.testing.assert_allclose(zo.loss_values, sr.loss_values, rtol=1e-3, atol=1e-3 * abs(sr.loss_values[0]))
    assert float((Z - Z_sr).abs().max()) < 1e-2
