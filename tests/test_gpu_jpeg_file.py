"""GPU tests (-m gpu) of reading JPEG files: esr_jpeg_file_unpack (csrc/esr_jpeg_file.hip) against its CPU expression bit for bit, and the
models fed from a file (esr_hip/jpeg_file.py, DecompCNNModel.feed_data with 'Q_table', test(compressed_chroma=...), the Z search).  They read
tests/golden/jpeg_files only (files and expected.npz, written by its generate.py) and need no Pillow.

Tolerances.  The unpack kernel moves integers and adds one fp32 constant: equality.  The consistency tests compress a model's output again,
without rounding, under the file-derived table and ask for the fed coefficients within 0.5 + tol, where tol is what the kernel tests of
tests/test_gpu_jpeg.py / tests/test_gpu_jpeg_chroma.py allow for extract followed by compress: the compressor's bound (4 x the reference's
relative fp32 distance from float64, times the largest coefficient) plus the extractor's bound in pixels carried through the compressor —
the transform is orthonormal on N x N pixels (N = 8, or 16 for chroma), so a pixel error of at most e moves a coefficient by at most
N e / (smallest table entry).  Model outputs GPU against CPU: the relative 1e-3 of test_model_test_equals_the_composition_of_the_modules;
Z-search losses: rtol 1e-3, atol 1e-3 |loss[0]|, as test_z_search_history_matches_the_cpu_path."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle.weights import seeded_uniform

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, 'tests', 'golden', 'jpeg_files')
DEV = 'cuda:0'
SPLIT_BAR = 1e-3
A = 219.0 / 255.0
GUARD = 64
_state = {}


def record():
    if 'rec' not in _state:
        with np.load(os.path.join(GOLDEN_DIR, 'expected.npz')) as z:
            _state['rec'] = {k: z[k] for k in z.files}
    return _state['rec']


def load(name, device='cpu'):
    from esr_hip import jpeg_file as JF
    return JF.load(os.path.join(GOLDEN_DIR, name + '.jpg'), device=device)


def cpu_unpack(*args):
    """the CPU expression, whatever the no_cpu_fallback fixture has put in its place"""
    from esr_hip import jpeg_file as JF
    return _state.setdefault('cpu_unpack', JF._unpack_cpu)(*args)


@pytest.fixture(autouse=True)
def no_cpu_fallback(monkeypatch):
    from esr_hip import jpeg as J, jpeg_file as JF
    _state.setdefault('cpu_unpack', JF._unpack_cpu)

    def refuse(*a, **k):
        raise AssertionError('the CPU fallback ran in a GPU test')
    for name in ('_compress_cpu', '_extract_cpu', '_compress16_cpu', '_extract16_cpu'):
        monkeypatch.setattr(J, name, refuse)
    monkeypatch.setattr(JF, '_unpack_cpu', refuse)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(n):
    """(NaN-filled buffer, its interior of n floats)"""
    buf = torch.full((n + 2 * GUARD,), float('nan'), device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _geometry(case):
    """(scan int16 CPU tensor, mcus_h, mcus_w, y_h, y_v, n_chroma, y_dc, c_dc) of a fixture file or a synthetic layout"""
    if isinstance(case, str):
        f = load(case)
        y_dc, c_dc = f._offsets()
        return torch.from_numpy(f.scan), f.mcus_h, f.mcus_w, f.y_h, f.y_v, f.n_chroma, y_dc, c_dc
    mcus_h, mcus_w, y_h, y_v, n_chroma, seed = case
    n = mcus_h * mcus_w * (y_h * y_v + n_chroma) * 64
    scan = torch.floor(seeded_uniform((n,), seed, -2047.0, 2048.0)).to(torch.int16)
    return scan, mcus_h, mcus_w, y_h, y_v, n_chroma, -1.1503906, 12.487805


# the fixture's files (one block; one partial block row; one MCU; 3 x 4 MCUs partial in both directions) and layouts wider than one
# workgroup's 32 MCUs: grey 2 x 35, 4:2:0 3 x 33 and 2 x 65 (three tiles, the last of one MCU), 4:4:4 2 x 40
UNPACK_CASES = ['grey_8x8', 'grey_9x7', 'c420_16x16', 'c420_41x57', (2, 35, 1, 1, 0, 8100), (3, 33, 2, 2, 2, 8101), (2, 65, 2, 2, 2, 8102),
                (2, 40, 1, 1, 2, 8103)]


@pytest.mark.parametrize('case', UNPACK_CASES, ids=lambda c: c if isinstance(c, str) else 'layout_%dx%d_%d%d%d' % c[:5])
def test_unpack_kernel_equals_the_cpu_expression_bit_for_bit(case):
    from esr_hip import _lib, jpeg_file as JF
    scan, mh, mw, y_h, y_v, nc, y_dc, c_dc = _geometry(case)
    want_y, want_c = cpu_unpack(scan, mh, mw, y_h, y_v, nc, y_dc, c_dc)
    sg = scan.to(DEV)
    ybuf, y = _guarded(want_y.numel())
    cbuf, c = _guarded(want_c.numel()) if nc else (None, None)
    rc = _lib.lib.esr_jpeg_file_unpack(sg.data_ptr(), mh, mw, y_h, y_v, nc, y_dc, c_dc, y.data_ptr(), c.data_ptr() if nc else None, None, _stream())
    assert rc == 0
    assert torch.equal(y.view(want_y.shape).cpu(), want_y)
    assert bool(torch.isnan(ybuf[:GUARD]).all()) and bool(torch.isnan(ybuf[-GUARD:]).all())
    if nc:
        assert torch.equal(c.view(want_c.shape).cpu(), want_c)
        assert bool(torch.isnan(cbuf[:GUARD]).all()) and bool(torch.isnan(cbuf[-GUARD:]).all())
        # Y alone from the same buffer (the Y model on a colour file): the same bits, the chroma blocks skipped
        y2buf, y2 = _guarded(want_y.numel())
        assert _lib.lib.esr_jpeg_file_unpack(sg.data_ptr(), mh, mw, y_h, y_v, nc, y_dc, c_dc, y2.data_ptr(), None, None, _stream()) == 0
        assert torch.equal(y2, y) and bool(torch.isnan(y2buf[:GUARD]).all()) and bool(torch.isnan(y2buf[-GUARD:]).all())
    # the binding's route, twice: equal bits
    got_y, got_c = JF.unpack(sg, mh, mw, y_h, y_v, nc, y_dc, c_dc)
    assert torch.equal(got_y.cpu(), want_y) and (got_c is None) == (nc == 0) and (nc == 0 or torch.equal(got_c.cpu(), want_c))
    if isinstance(case, str):          # and the record of the independent decoder: the file's integers, plus the DC terms
        rec = record()
        ref = torch.from_numpy(rec[case + '/coef0'].astype(np.float32))
        ref[0] += y_dc
        assert torch.equal(got_y[0].cpu(), ref)
        for k in range(nc):
            ref = torch.from_numpy(rec['%s/coef%d' % (case, 1 + k)].astype(np.float32))
            ref[0] += c_dc
            assert torch.equal(got_c[0, 64 * k:64 * k + 64].cpu(), ref)


@pytest.mark.parametrize('planes', [2, 1])
def test_unpack_act_output_equals_the_pack_of_the_fp32_result(planes):
    from esr_hip import _lib, jpeg_file as JF
    from esr_hip.act import new_zeroed, view_of
    for case in ('grey_9x7', 'c420_41x57', (2, 35, 1, 1, 0, 8100), (3, 33, 2, 2, 2, 8101)):
        scan, mh, mw, y_h, y_v, nc, y_dc, c_dc = _geometry(case)
        sg = scan.to(DEV)
        h, w = mh * y_v, mw * y_h
        for lead in (0, 8):                                                            # behind `lead` groups of a wider buffer, as behind Z
            a, b = new_zeroed(planes, 1, lead + 8, h, w, DEV), new_zeroed(planes, 1, lead + 8, h, w, DEV)
            y, _ = JF.unpack(sg, mh, mw, y_h, y_v, nc, y_dc, c_dc, want_chroma=False, act_view=view_of(a, lead, 8))
            assert torch.equal(y, JF.unpack(sg, mh, mw, y_h, y_v, nc, y_dc, c_dc, want_chroma=False)[0])
            assert _lib.lib.esr_pack_nchw(y.data_ptr(), 0, 1, 64, h, w, 0, 64, 0, 1, C.byref(view_of(b, lead, 8)), _stream()) == 0
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
            only = new_zeroed(planes, 1, lead + 8, h, w, DEV)                           # the view as the only output
            assert _lib.lib.esr_jpeg_file_unpack(sg.data_ptr(), mh, mw, y_h, y_v, nc, y_dc, c_dc, None, None, C.byref(view_of(only, lead, 8)), _stream()) == 0
            assert torch.equal(only.view(torch.int16), b.view(torch.int16))


def test_unpack_bad_arguments_return_negative_and_write_nothing():
    from esr_hip import _lib
    from esr_hip._lib import ESR_E_ARG
    from esr_hip.act import new_zeroed, view_of
    scan, mh, mw, y_h, y_v, nc, y_dc, c_dc = _geometry('c420_41x57')
    sg = scan.to(DEV)
    ybuf, y = _guarded(64 * 4 * mh * mw)
    cbuf, c = _guarded(128 * mh * mw)
    L, s = _lib.lib, _stream()
    assert L.esr_jpeg_file_unpack(sg.data_ptr(), mh, mw, 2, 1, nc, y_dc, c_dc, y.data_ptr(), c.data_ptr(), None, s) == ESR_E_ARG
    assert L.esr_jpeg_file_unpack(sg.data_ptr(), mh, 0, y_h, y_v, nc, y_dc, c_dc, y.data_ptr(), c.data_ptr(), None, s) == ESR_E_ARG
    assert L.esr_jpeg_file_unpack(sg.data_ptr(), mh, mw, y_h, y_v, 0, y_dc, c_dc, y.data_ptr(), c.data_ptr(), None, s) == ESR_E_ARG
    assert L.esr_jpeg_file_unpack(sg.data_ptr() + 2, mh, mw, y_h, y_v, nc, y_dc, c_dc, y.data_ptr(), c.data_ptr(), None, s) == ESR_E_ARG
    assert L.esr_jpeg_file_unpack(None, mh, mw, y_h, y_v, nc, y_dc, c_dc, y.data_ptr(), c.data_ptr(), None, s) == ESR_E_ARG
    small = new_zeroed(1, 1, 8, 2 * mh, 2 * mw - 1, DEV)                                # a view of another width
    assert L.esr_jpeg_file_unpack(sg.data_ptr(), mh, mw, y_h, y_v, nc, y_dc, c_dc, y.data_ptr(), c.data_ptr(), C.byref(view_of(small, 0, 8)), s) == ESR_E_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(ybuf).all()) and bool(torch.isnan(cbuf).all()) and float(small.float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the models on a file
def _y_tol(coef, img, table):
    """extract then compress on the GPU kernels against exact arithmetic, from the reference's own fp32 distances (tests/test_gpu_jpeg.py)"""
    from test_gpu_jpeg import _case
    d = _case('noise')[3]
    return 4 * d['compress_rel'] * float(coef.abs().max()) + 8 * 4 * d['extract_q_rel'] * float((img - 128).abs().max()) / float(table.min())


def _chroma_tol(coef, img, table):
    from test_gpu_jpeg_chroma import _rel
    return _rel('compress') * float(coef.abs().max()) + 16 * _rel('extract128') * float(img.abs().max()) / float(table.min())


@pytest.mark.parametrize('name', ['grey_33x17', 'c420_41x57'])
def test_y_model_output_requantises_to_the_files_coefficients(tmp_path, name):
    from test_host_jpeg import make_model
    model = make_model(tmp_path, gpu=True)
    f = load(name, DEV)
    data = f.model_data(False)
    assert data['Comp'].is_cuda and not data['Q_table'].is_cuda          # the tables stay on the host: the modules read them there
    rec = record()
    assert torch.equal(data['Comp'][0, 1:].cpu(), torch.from_numpy(rec[name + '/coef0'][1:].astype(np.float32)))
    H, W = f.padded_size
    model.feed_data(dict(data, Z=seeded_uniform((1, 64, H // 8, W // 8), 8200, -1.0, 1.0)), need_GT=False)
    model.test()
    assert model.output_image.shape == (1, 1, H, W) and f.crop(model.output_image).shape == (1, 1, f.height, f.width)
    back = model.JPEG['non_quantized_compressor'](model.output_image)
    err, tol = float((back - data['Comp']).abs().max()), _y_tol(data['Comp'], model.output_image, data['Q_table'][0])
    print('%s: |compress(output) - fed| max %.6f (0.5 + %.3g)' % (name, err, tol))
    assert err <= 0.5 + tol
    assert err > 0.05                                                                  # the generator did move the coefficients
    clear = (back - data['Comp']).abs()[:, 1:] < 0.499                                 # away from the +-0.5 edge they round to the file's integers
    assert torch.equal(torch.round(back[:, 1:])[clear], data['Comp'][:, 1:][clear]) and float(clear.float().mean()) > 0.99


def test_colour_model_output_requantises_to_the_files_chroma_coefficients(tmp_path):
    from test_host_jpeg_chroma import make_model
    model = make_model(tmp_path, gpu=True)
    f = load('c420_midgrey_32x48', DEV)
    data = f.model_data(True)
    H, W = f.padded_size
    assert (H, W) == (48, 32) and data['compressed_chroma'].shape == (1, 128, 3, 2)
    model.feed_data({'Comp': data['Comp'], 'Q_table': data['Q_table'], 'Z': seeded_uniform((1, 64, H // 8, W // 8), 8201, -1.0, 1.0)}, need_GT=False)
    model.test(compressed_chroma=data['compressed_chroma'])
    assert model.output_image.shape == (1, 3, H, W)
    y = model.output_image[:, :1]
    print('generated Y plane in [%.2f, %.2f]' % (float(y.min()), float(y.max())))
    assert float(y.min()) > 0 and float(y.max()) < 255                                 # the clamp of the Y plane is inactive
    assert torch.equal(model.var_Comp[:, 256:], data['compressed_chroma'])
    back = model.JPEG['non_quantized_compressor'](model.output_image)[:, 256:]
    err = float((back - data['compressed_chroma']).abs().max())
    tol = _chroma_tol(data['compressed_chroma'], model.output_image[:, 1:], data['Q_table'][1])
    print('|compress(output) - fed chroma| max %.6f (0.5 + %.3g)' % (err, tol))
    assert err <= 0.5 + tol and err > 0.05


def _run_file(model, f, chroma):
    data = f.model_data(chroma)
    H, W = f.padded_size
    feed = {k: v for k, v in data.items() if k != 'compressed_chroma'}
    model.feed_data(dict(feed, Z=seeded_uniform((1, 64, H // 8, W // 8), 8300, -1.0, 1.0)), need_GT=False)
    model.test(**({'compressed_chroma': data['compressed_chroma']} if chroma else {}))
    return model.fake_H.cpu(), model.output_image.cpu()


@pytest.mark.parametrize('chroma', [False, True])
def test_model_test_on_a_file_equals_the_cpu_route(tmp_path, chroma, monkeypatch):
    import test_host_jpeg
    import test_host_jpeg_chroma
    make_model = (test_host_jpeg_chroma if chroma else test_host_jpeg).make_model
    (tmp_path / 'gpu').mkdir()
    (tmp_path / 'cpu').mkdir()
    name = 'c420_midgrey_32x48' if chroma else 'c420_41x57'
    gpu = _run_file(make_model(tmp_path / 'gpu', gpu=True), load(name, DEV), chroma)
    monkeypatch.undo()                                              # the CPU side of the comparison runs the CPU expressions
    cpu = _run_file(make_model(tmp_path / 'cpu'), load(name), chroma)
    for got, want, what in zip(gpu, cpu, ('fake_H', 'output_image')):
        err = float((got - want).abs().max() / want.abs().max())
        print('%s: %.3g of the largest value from the CPU route' % (what, err))
        assert got.shape == want.shape and err < SPLIT_BAR


@pytest.mark.parametrize('name', ['grey_8x8', 'grey_9x7', 'grey_33x17'])
def test_baseline_image_is_within_one_level_of_libjpeg(name):
    f = load(name, DEV)
    img = f.baseline_image()
    assert img.is_cuda and img.shape == (1, 1, f.height, f.width)
    full = torch.clamp(torch.round((255 * img[0, 0].double() - 16) / A), 0, 255).cpu().numpy()
    err = float(np.abs(full - record()[name + '/pillow0'].astype(np.float64)).max())
    print('%s: %.1f levels from libjpeg' % (name, err))
    assert err <= 1.0


def test_baseline_image_of_a_colour_file():
    f = load('c420_41x57', DEV)
    img = f.baseline_image()
    assert img.is_cuda and img.shape == (1, 3, 57, 41) and float(img.min()) >= 0 and float(img.max()) <= 1
    # its luminance, read back from the extractor, against libjpeg's Y plane
    from esr_hip import jpeg as J
    data = f.model_data(False)
    y = J.extract(data['Comp'], data['Q_table'].reshape(1, 64))[1]
    full = torch.clamp(torch.round((f.crop(y)[0, 0].double() - 16) / A), 0, 255).cpu().numpy()
    assert float(np.abs(full - record()['c420_41x57/pillow0'].astype(np.float64)).max()) <= 1.0


def _one_iteration(model, f):
    from Z_optimization import Z_optimizer
    data = f.model_data(False)
    H, W = f.padded_size
    Z0 = seeded_uniform((1, 64, H // 8, W // 8), 8400, -0.5, 0.5).to(model.device)
    model.feed_data(dict(data, Z=Z0), need_GT=False)
    model.test()
    zo = Z_optimizer('max_STD', [H // 8, W // 8], model, Z_range=1.0, max_iters=1, data=data, initial_Z=Z0, initial_LR=0.05, batch_size=1,
                     jpeg_extractor=model.JPEG['extractor'])
    zo.optimize()
    return zo.loss_values


def test_one_z_search_iteration_on_a_file_matches_the_cpu_route(tmp_path, monkeypatch):
    from test_host_jpeg import make_model
    (tmp_path / 'gpu').mkdir()
    (tmp_path / 'cpu').mkdir()
    gpu = _one_iteration(make_model(tmp_path / 'gpu', gpu=True), load('c420_41x57', DEV))
    monkeypatch.undo()
    cpu = _one_iteration(make_model(tmp_path / 'cpu'), load('c420_41x57'))
    print('max_STD on a file: GPU %s, CPU %s' % (gpu, cpu))
    assert len(gpu) == len(cpu) == 1 and np.all(np.isfinite(gpu))
    np.testing.assert_allclose(gpu, cpu, rtol=1e-3, atol=1e-3 * abs(cpu[0]))
