"""CPU tests of reading JPEG files (esr_hip/jpeg_file.py, csrc/esr_jpeg_parse.h behind esr_jpeg_file_info / esr_jpeg_file_decode, the model
plumbing in JPEG_module/JPEG.py and models/DecompCNN_model.py).

The yardstick for the entropy decoder is py_decode below: a baseline decoder in plain Python that shares no code with the C++ (bits as a
string, codes in a dict).  Files are made on the fly with Pillow; the C++ coefficients and tables must equal py_decode's on every entry.
Equality with an independent decoder is what proves exactness: the tie to libjpeg (Pillow's own decode) can only be held to 1 grey level —
libjpeg's integer IDCT against the real one — and one quantisation step at Q = 3 moves a pixel by at most 0.75 levels.

Bounds of the mapping tests are the existing CPU-against-float64 ones: 4 x the reference's own fp32 distance from a float64 restatement,
read from tests/golden/jpeg_dncnn.npz (Y, as tests/test_host_jpeg.py) and tests/golden/jpeg_chroma.npz (b/err/extract128, as
tests/test_host_jpeg_chroma.py)."""
import io
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_host_jpeg import G, golden as y_golden, make_model as make_y_model
from test_host_jpeg_chroma import golden as chroma_golden, make_model as make_colour_model
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'explorable-super-resolution_amd', 'csrc')
GOLDEN_DIR = os.path.join(ROOT, 'tests', 'golden', 'jpeg_files')
A, B = 219.0 / 255.0, 224.0 / 255.0
CALL_LIMIT_S = 1.0            # per decode call on the robustness corpus (files of a few hundred bytes: a call takes microseconds)

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


# ------------------------------------------------------------------------------------------------ the independent decoder
def header_segments(data):
    """(marker, start of the segment's 0xFF, end) for every segment up to and including SOS"""
    p, out = 2, []
    while True:
        assert data[p] == 0xFF, 'a marker was expected at byte %d' % p
        start = p
        while data[p] == 0xFF:
            p += 1
        m = data[p]
        p += 1
        if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7:
            continue
        end = p + int.from_bytes(data[p:p + 2], 'big')
        out.append((m, start, end))
        if m == 0xDA:
            return out
        p = end


def py_decode(data):
    """baseline JPEG -> {'width', 'height', 'sof', 'ri', 'comps': [(h, v, tq)], 'tables': {id: int64 [64] natural order},
    'coef': [int64 [64, hb, wb] natural order per component], 'seen': what the file exercised}"""
    assert data[:2] == b'\xff\xd8'
    qt, hf, frame, ri = {}, {}, None, 0
    seen = {'stuffing': False, 'intervals': 1, 'zrl': False, 'neg_dc': False, 'dqt16': False, 'comment': False, 'app_bytes': 0}
    for m, start, end in header_segments(data):
        seg = data[start + 4:end]
        if m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                n = pq + 1
                vals = [int.from_bytes(seg[i + 1 + k * n:i + 1 + (k + 1) * n], 'big') for k in range(64)]
                i += 1 + 64 * n
                qt[tq] = np.zeros(64, np.int64)
                qt[tq][ZZ] = vals
                seen['dqt16'] |= pq == 1
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                key, counts = (seg[i] >> 4, seg[i] & 15), seg[i + 1:i + 17]
                i += 17
                codes, code = {}, 0
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        codes[(length, code)] = seg[i]
                        i += 1
                        code += 1
                    code <<= 1
                hf[key] = codes
        elif m in (0xC0, 0xC1):
            assert seg[0] == 8
            frame = {'sof': m - 0xC0, 'height': int.from_bytes(seg[1:3], 'big'), 'width': int.from_bytes(seg[3:5], 'big'),
                     'comps': [(seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])]}
        elif m == 0xDD:
            ri = int.from_bytes(seg[:2], 'big')
        elif m == 0xFE:
            seen['comment'] = True
        elif 0xE0 <= m <= 0xEF:
            seen['app_bytes'] += len(seg)
        elif m == 0xDA:
            ns = seg[0]
            tabs = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(ns)]
            assert ns == len(frame['comps'])
            p = end
    comps = frame['comps'] if len(frame['comps']) > 1 else [(1, 1, frame['comps'][0][2])]
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    mw, mh = -(-frame['width'] // (8 * hmax)), -(-frame['height'] // (8 * vmax))
    coef = [np.zeros((mh * v, mw * h, 64), np.int64) for h, v, _ in comps]
    # the entropy-coded data, interval by interval, as strings of bits
    intervals, cur, rst = [], [], []
    while True:
        b = data[p]
        p += 1
        if b != 0xFF:
            cur.append(b)
            continue
        nxt = data[p]
        p += 1
        if nxt == 0:
            cur.append(0xFF)
            seen['stuffing'] = True
        elif 0xD0 <= nxt <= 0xD7:
            intervals.append(cur)
            rst.append(nxt - 0xD0)
            cur = []
        else:
            assert nxt == 0xD9
            intervals.append(cur)
            break
    assert rst == [k % 8 for k in range(len(rst))]
    seen['intervals'] = len(intervals)
    mcu = 0
    for chunk in intervals:
        bits, pos, pred = ''.join(format(b, '08b') for b in chunk), 0, [0] * len(comps)

        def symbol(table):
            nonlocal pos
            code, length = 0, 0
            while True:
                code, length, pos = (code << 1) | int(bits[pos]), length + 1, pos + 1
                if (length, code) in table:
                    return table[(length, code)]
                assert length < 16

        def number(s):
            nonlocal pos
            if s == 0:
                return 0
            v = int(bits[pos:pos + s], 2)
            pos += s
            return v if v >= 1 << (s - 1) else v - (1 << s) + 1
        for _ in range(ri or mw * mh):
            if mcu == mw * mh:
                break
            my, mx = divmod(mcu, mw)
            for c, (h, v, _) in enumerate(comps):
                for by in range(v):
                    for bx in range(h):
                        block = coef[c][my * v + by, mx * h + bx]
                        diff = number(symbol(hf[(0, tabs[c][0])]))
                        seen['neg_dc'] |= diff < 0
                        pred[c] += diff
                        block[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = symbol(hf[(1, tabs[c][1])])
                            if rs == 0:
                                break
                            if rs == 0xF0:
                                seen['zrl'] = True
                                k += 16
                                continue
                            k += rs >> 4
                            block[ZZ[k]] = number(rs & 15)
                            k += 1
            mcu += 1
    assert mcu == mw * mh
    return {'width': frame['width'], 'height': frame['height'], 'sof': frame['sof'], 'ri': ri, 'comps': comps,
            'tables': {c: qt[c] for c in sorted({t for _, _, t in comps})},
            'coef': [np.ascontiguousarray(a.transpose(2, 0, 1)) for a in coef], 'seen': seen}


# ------------------------------------------------------------------------------------------------ the files
SIZES = [(1, 1), (8, 8), (9, 7), (16, 16), (17, 33), (41, 57)]          # (width, height)
QUALITIES = [5, 50, 95, 100]
RESTARTS = [{}, {'restart_marker_blocks': 1}, {'restart_marker_rows': 1}]


def picture(width, height, seed=0):
    """smooth waves plus noise, RGB uint8: every frequency carries something, neighbouring blocks differ in their means"""
    rng = np.random.RandomState(1000 * width + height + seed)
    yy, xx = np.mgrid[0:height, 0:width]
    base = 127 + 90 * np.sin(xx / 3.0 + seed) * np.cos(yy / 5.0) + 30 * np.sin((xx + yy) / 11.0)
    rgb = base[..., None] * np.array([1.0, 0.8, 0.6]) + np.array([0, 30, 60]) + rng.randint(-40, 41, (height, width, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8)


def jpeg_bytes(width, height, mode, seed=0, **save):
    im = Image.fromarray(picture(width, height, seed)).convert(mode)
    buf = io.BytesIO()
    im.save(buf, 'JPEG', **save)
    return buf.getvalue()


def rewrite_dqt16_sof1(data):
    """byte surgery: every DQT table as 16-bit entries, SOF0 as SOF1"""
    out, last = bytearray(data[:2]), 2
    for m, start, end in header_segments(data):
        out += data[last:start]
        seg = data[start + 4:end]
        if m == 0xDB:
            body, i = bytearray(), 0
            while i < len(seg):
                assert seg[i] >> 4 == 0
                body += bytes([0x10 | seg[i]]) + b''.join(bytes([0, v]) for v in seg[i + 1:i + 65])
                i += 65
            out += b'\xff\xdb' + (len(body) + 2).to_bytes(2, 'big') + body
        elif m == 0xC0:
            out += b'\xff\xc1' + data[start + 2:end]
        else:
            out += data[start:end]
        last = end
    return bytes(out + data[last:])


_corpus = {}


def corpus():
    """name -> bytes, made once"""
    if not _corpus:
        for mode, (w, h), q, opt, rst in itertools.product(('L', 'RGB'), SIZES, QUALITIES, (False, True), range(3)):
            save = dict(quality=q, optimize=opt, **RESTARTS[rst])
            if mode == 'RGB':
                save['subsampling'] = 2                                          # 4:2:0
            _corpus['%s_%dx%d_q%d_opt%d_rst%d' % (mode, w, h, q, opt, rst)] = jpeg_bytes(w, h, mode, **save)
        _corpus['RGB_41x57_comment_app'] = jpeg_bytes(41, 57, 'RGB', quality=75, subsampling=2, comment=b'a comment ' * 40,
                                                      icc_profile=bytes(range(256)) * 300)      # 76800 bytes: more than one APP2 segment
        _corpus['RGB_17x33_dqt16_sof1'] = rewrite_dqt16_sof1(jpeg_bytes(17, 33, 'RGB', quality=50, subsampling=2))
        _corpus['L_9x7_dqt16_sof1'] = rewrite_dqt16_sof1(jpeg_bytes(9, 7, 'L', quality=50))
        _corpus['RGB444_17x33_q90'] = jpeg_bytes(17, 33, 'RGB', quality=90, subsampling=0)
        # flat areas next to busy ones, high quality: long zero runs (ZRL) in the busy blocks' tails
        flat = picture(41, 57)
        flat[:, :24] = 128
        buf = io.BytesIO()
        Image.fromarray(flat).save(buf, 'JPEG', quality=30, subsampling=2)
        _corpus['RGB_41x57_flat_q30'] = buf.getvalue()
    return _corpus


def smallest():
    return min(corpus().values(), key=len)


_decoded = {}


def decoded(name):
    """(JpegFile, py_decode's dict) of a corpus file, computed once"""
    from esr_hip import jpeg_file as JF
    if name not in _decoded:
        _decoded[name] = (JF.load(corpus()[name]), py_decode(corpus()[name]))
    return _decoded[name]


# ------------------------------------------------------------------------------------------------ exactness
def test_coefficients_and_tables_equal_the_independent_decoder_on_every_entry():
    seen_any = {}
    for name, data in corpus().items():
        f, want = decoded(name)
        assert (f.width, f.height, f.sof, f.restart_interval) == (want['width'], want['height'], want['sof'], want['ri']), name
        assert f.sampling == {1: 'gray', 3: '4:2:0' if want['comps'][0][0] == 2 else '4:4:4'}[len(want['comps'])], name
        assert len(f.coefficients) == len(want['coef']) == len(f.tables), name
        for c, (got, ref) in enumerate(zip(f.coefficients, want['coef'])):
            assert got.dtype == np.int16 and got.shape == ref.shape, (name, c)
            assert np.array_equal(got, ref), (name, c)
            assert f.tables[c].shape == (8, 8) and np.array_equal(f.tables[c].reshape(64), want['tables'][want['comps'][c][2]]), (name, c)
        for k, v in want['seen'].items():
            seen_any[k] = max(seen_any.get(k, 0), int(v))
    # what the set really contains
    assert seen_any['stuffing'] and seen_any['zrl'] and seen_any['neg_dc'] and seen_any['dqt16'] and seen_any['comment']
    assert seen_any['app_bytes'] > 65535
    assert decoded('RGB_41x57_q50_opt0_rst1')[1]['seen']['intervals'] == 12          # 3 x 4 MCUs, one per interval: RST0...7, then 0...2
    assert decoded('RGB_17x33_dqt16_sof1')[0].sof == 1 and decoded('RGB_17x33_dqt16_sof1')[1]['seen']['dqt16']
    assert {1, 8, 9, 16, 17, 41} == {f.width for f, _ in _decoded.values()}


def test_load_many_and_paths(tmp_path):
    from esr_hip import jpeg_file as JF
    names = ['L_9x7_q50_opt0_rst0', 'RGB_41x57_q50_opt1_rst2', 'RGB444_17x33_q90']
    paths = []
    for n in names:
        paths.append(str(tmp_path / (n + '.jpg')))
        with open(paths[-1], 'wb') as fh:
            fh.write(corpus()[n])
    files = JF.load_many(paths)
    assert [f.name for f in files] == [n + '.jpg' for n in names] and JF.load_many([]) == []
    for f, n in zip(files, names):
        for got, want in zip(f.coefficients, decoded(n)[0].coefficients):
            assert np.array_equal(got, want)
    assert JF.MAX_WORKERS == 16
    bad = str(tmp_path / 'progressive.jpg')
    with open(bad, 'wb') as fh:
        fh.write(jpeg_bytes(16, 16, 'RGB', progressive=True))
    with pytest.raises(NotImplementedError, match='progressive'):
        JF.load_many(paths + [bad])
    refused = {}
    assert [f.name for f in JF.load_many([bad] + paths, on_error=refused.__setitem__)] == [n + '.jpg' for n in names] and list(refused) == [bad]
    f = files[1]
    assert f.padded_size == (64, 48) and f.crop(torch.zeros(1, 3, 64, 48)).shape == (1, 3, 57, 41)


# ------------------------------------------------------------------------------------------------ the tie to libjpeg
def idct_planes(q, table):
    """float64 [hb * 8, wb * 8] = 128 + iDCT(q Q) of one component"""
    from esr_hip.jpeg import dct_matrix
    D = dct_matrix(torch.float64).numpy()
    c = q.astype(np.float64).reshape(8, 8, *q.shape[1:]) * table.astype(np.float64).reshape(8, 8, 1, 1)
    img = np.einsum('ur,uvij,vs->irjs', D, c, D) + 128
    return img.reshape(8 * q.shape[1], 8 * q.shape[2])


def pillow_planes(data):
    """Pillow's (libjpeg's) own decode: Y at full size, Cb and Cr at the half-size draft, where libjpeg upsamples nothing"""
    im = Image.open(io.BytesIO(data))
    if im.mode == 'L':
        return [np.asarray(im).astype(np.float64)]
    w, h = im.size
    im.draft('YCbCr', (w, h))
    assert im.mode == 'YCbCr' and im.size == (w, h)
    out = [np.asarray(im)[..., 0].astype(np.float64)]
    if min(w, h) < 2:
        return out                                      # (draft picks its scale as size // requested size: no half of one pixel)
    half = Image.open(io.BytesIO(data))
    half.draft('YCbCr', (w // 2, h // 2))
    assert half.mode == 'YCbCr' and half.size == ((w + 1) // 2, (h + 1) // 2), half.size
    arr = np.asarray(half).astype(np.float64)
    return out + [arr[..., 1], arr[..., 2]]


def test_real_idct_of_the_coefficients_is_within_one_level_of_libjpeg():
    worst = 0.0
    for name, data in corpus().items():
        f, _ = decoded(name)
        if f.sampling == '4:4:4':
            continue                                    # (the half-size draft is the 4:2:0 comparison)
        for c, want in enumerate(pillow_planes(data)):
            got = np.clip(np.round(idct_planes(f.coefficients[c], f.tables[c])), 0, 255)[:want.shape[0], :want.shape[1]]
            err = float(np.abs(got - want).max())
            worst = max(worst, err)
            assert err <= 1.0, (name, c, err)
    print('largest distance from libjpeg over the set: %.1f grey levels' % worst)


# ------------------------------------------------------------------------------------------------ the mapping into the models' domain
MAPPING = ['L_9x7_q95_opt0_rst0', 'RGB_41x57_q50_opt0_rst0', 'RGB_17x33_q5_opt1_rst1', 'RGB_16x16_q100_opt0_rst0']


def _y_bound():
    """4 x the reference's own fp32 distance from float64 on the Y fixture's extractor cases (tests/test_host_jpeg.py)"""
    g = y_golden()
    tables = torch.from_numpy(g['a/tables'])
    errs = []
    for kind in ('noise', 'smooth'):
        cq = torch.from_numpy(np.asarray(g['a/%s/cq' % kind])).float()
        errs.append(float((torch.from_numpy(np.asarray(g['a/%s/img_q' % kind])).double() - G.extract64(cq, tables)).abs().max()))
    return 4 * max(errs)


@pytest.mark.parametrize('name', MAPPING)
def test_model_domain_y_is_the_studio_range_decode(name):
    from esr_hip import jpeg as J
    f, _ = decoded(name)
    data = f.model_data(False)
    assert data['Comp'].shape == (1, 64, f.padded_size[0] // 8, f.padded_size[1] // 8) and data['Q_table'].shape == (1, 8, 8)
    assert not data['Comp'].is_cuda and data['Comp'].dtype == torch.float32
    # the integers are the file's, the DC channel carries the one fractional term
    comp = data['Comp'][0].numpy().astype(np.float64)
    assert np.array_equal(comp[1:], f.coefficients[0][1:])
    t_y = A * f.tables[0].astype(np.float64)
    assert np.allclose(comp[0] - f.coefficients[0][0], 8 * (16 - 128 * (1 - A)) / t_y[0, 0], rtol=0, atol=2e-7 * np.abs(comp[0]).max() + 1e-6)
    assert np.allclose(data['Q_table'][0].numpy(), t_y, rtol=1e-7, atol=0)          # real-valued: a Q_Y as it is, to fp32
    c, img = J.extract(data['Comp'], data['Q_table'].reshape(1, 64))
    want = 16 + A * idct_planes(f.coefficients[0], f.tables[0])
    err, bound = float(np.abs(img[0, 0].numpy().astype(np.float64) - want).max()), _y_bound()
    print('%s: Y extract %.3g from float64 (bound %.3g)' % (name, err, bound))
    assert err <= bound


@pytest.mark.parametrize('name', [n for n in MAPPING if n.startswith('RGB')])
def test_model_domain_chroma_is_the_dct_domain_upsampling_of_the_studio_range_decode(name):
    from esr_hip import jpeg as J
    from esr_hip.jpeg import dct_matrix, dct_matrix16
    f, _ = decoded(name)
    data = f.model_data(True)
    H, W = f.padded_size
    assert data['compressed_chroma'].shape == (1, 128, H // 16, W // 16) and data['Q_table'].shape == (2, 8, 8)
    cc = data['compressed_chroma'][0].numpy().astype(np.float64)
    t_c = 2 * B * f.tables[1].astype(np.float64)
    assert np.allclose(data['Q_table'][1].numpy(), t_c, rtol=1e-7, atol=0)
    for k in range(2):
        assert np.array_equal(cc[64 * k + 1:64 * k + 64], f.coefficients[1 + k][1:])
        assert np.allclose(cc[64 * k] - f.coefficients[1 + k][0], 2048 / t_c[0, 0], rtol=0, atol=2e-7 * np.abs(cc[64 * k]).max() + 1e-6)
    pad = lambda t: np.pad(t, ((0, 8), (0, 8)), 'edge')
    padded = torch.from_numpy(np.stack([pad(A * f.tables[0].astype(np.float64)), pad(t_c), pad(t_c)]).astype(np.float32)).reshape(1, 3, 256)
    _, img = J.extract16(data['compressed_chroma'], padded)
    assert img.shape == (1, 2, H, W)
    D8, D16 = dct_matrix(torch.float64).numpy(), dct_matrix16(torch.float64).numpy()
    bound = 4 * float(chroma_golden()['b/err/extract128'][0])
    for k in range(2):
        half = 128 + B * (idct_planes(f.coefficients[1 + k], f.tables[1 + k]) - 128)          # studio range, [H/2, W/2]
        blocks = half.reshape(H // 16, 8, W // 16, 8)
        low = 2 * np.einsum('ur,irjs,vs->ijuv', D8, blocks, D8)                               # DCT-domain x2 upsampling: the low 8 x 8 of
        full = np.zeros((H // 16, W // 16, 16, 16))                                           # the 16-point transform, doubled
        full[:, :, :8, :8] = low
        want = np.einsum('ur,ijuv,vs->irjs', D16, full, D16).reshape(H, W)
        err = float(np.abs(img[0, k].numpy().astype(np.float64) - want).max())
        print('%s: chroma plane %d extract16 %.3g from float64 (bound %.3g)' % (name, k, err, bound))
        assert err <= bound
        assert abs(want.reshape(H // 16, 16, W // 16, 16).mean((1, 3)) - blocks.mean((1, 3))).max() < 1e-9      # equal block means


def test_baseline_image_and_the_uncompressed_chroma_route_on_the_cpu():
    f, _ = decoded('RGB_41x57_q50_opt0_rst0')
    img = f.baseline_image()
    assert img.shape == (1, 3, 57, 41) and float(img.min()) >= 0 and float(img.max()) <= 1
    ref = np.asarray(Image.open(io.BytesIO(corpus()['RGB_41x57_q50_opt0_rst0'])).convert('RGB')).astype(np.float64) / 255
    # libjpeg upsamples chroma with a triangle filter in the pixel domain, this decode in the DCT domain: close on average, not equal
    assert float(np.abs(img[0].permute(1, 2, 0).numpy() - ref).mean()) < 0.02
    g, _ = decoded('L_9x7_q95_opt0_rst0')
    grey = g.baseline_image()
    assert grey.shape == (1, 1, 7, 9)
    full = np.clip(np.round((255 * grey[0, 0].numpy().astype(np.float64) - 16) / A), 0, 255)
    assert np.abs(full - pillow_planes(corpus()['L_9x7_q95_opt0_rst0'])[0]).max() <= 1
    f444, _ = decoded('RGB444_17x33_q90')
    assert f444.baseline_image().shape == (1, 3, 33, 17)
    ref = np.asarray(Image.open(io.BytesIO(corpus()['RGB444_17x33_q90'])).convert('RGB')).astype(np.float64)
    assert np.abs(255 * f444.baseline_image()[0].permute(1, 2, 0).numpy() - ref).max() < 3          # no upsampling: the rounded matrices only
    chroma = f.uncompressed_chroma()
    assert chroma.shape == (1, 2, 64, 48)


# ------------------------------------------------------------------------------------------------ refusals
def test_file_refusals_by_name():
    from esr_hip import jpeg_file as JF
    with pytest.raises(NotImplementedError, match='progressive'):
        JF.load(jpeg_bytes(16, 16, 'RGB', progressive=True))
    with pytest.raises(NotImplementedError, match='4:2:2'):
        JF.load(jpeg_bytes(16, 16, 'RGB', subsampling=1))
    with pytest.raises(NotImplementedError, match='CMYK'):
        JF.load(jpeg_bytes(16, 16, 'CMYK'))
    adobe_rgb = b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00'          # APP14, transform 0: the three components are R, G, B
    colour = jpeg_bytes(16, 16, 'RGB', subsampling=0)
    with pytest.raises(NotImplementedError, match='RGB JPEG'):
        JF.load(colour[:2] + adobe_rgb + colour[2:])
    assert JF.load(colour[:2] + adobe_rgb[:-1] + b'\x01' + colour[2:]).sampling == '4:4:4'          # transform 1: YCbCr
    assert JF.load(jpeg_bytes(8, 8, 'L')[:2] + adobe_rgb + jpeg_bytes(8, 8, 'L')[2:]).sampling == 'gray'
    with pytest.raises(JF.JpegFileError, match='not a JPEG'):
        JF.load(b'\x89PNG\r\n\x1a\n' + bytes(64))
    with pytest.raises(JF.JpegFileError, match='truncated'):
        JF.load(corpus()['L_8x8_q50_opt0_rst0'][:-2])
    grey, _ = decoded('L_9x7_q95_opt0_rst0')
    with pytest.raises(NotImplementedError, match='grey'):
        grey.model_data(True)
    f444, _ = decoded('RGB444_17x33_q90')
    with pytest.raises(NotImplementedError, match='4:4:4'):
        f444.model_data(True)
    assert f444.model_data(False)['Comp'].shape == (1, 64, 5, 3)                     # the Y model takes its luminance


# ------------------------------------------------------------------------------------------------ robustness
CHILD_LIMIT_S = 120.0         # the child process of the robustness test: a second or two of calls behind the import of torch


def test_every_prefix_is_refused_and_every_substitution_comes_back(tmp_path):
    """in a child process (tests/jpeg_file_robustness.py) that is ended after CHILD_LIMIT_S: a decoder that spins fails here, it does not hang"""
    data = smallest()
    assert len(data) < 1024
    path = str(tmp_path / 'smallest.jpg')
    with open(path, 'wb') as fh:
        fh.write(data)
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'jpeg_file_robustness.py'), path], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=CHILD_LIMIT_S)
    assert run.returncode == 0, run.stderr.decode(errors='replace')[-2000:]
    out = json.loads(run.stdout.decode().strip().splitlines()[-1])
    print(out)
    assert out['bytes'] == len(data) and out['whole'] == [0, 0]
    assert out['prefixes_not_refused'] == [] and out['substitutions_with_another_status'] == []
    assert sum(out['outcomes'].values()) == 3 * len(data) and out['outcomes'].get('-4', 0) > 0 and out['outcomes'].get('0', 0) > 0
    assert out['slowest_s'] < CALL_LIMIT_S


def test_cabi_argument_checks():
    import ctypes as C
    from esr_hip import _lib
    from esr_hip._lib import ESR_E_ARG, ESR_E_UNSUPPORTED
    h = _lib.load_library()
    data, info = smallest(), _lib.JpegInfo()
    scan, tables = np.empty(64, np.int16), np.zeros((4, 64), np.uint16)
    assert h.esr_jpeg_file_info(None, 10, C.byref(info)) == ESR_E_ARG and h.esr_jpeg_file_info(data, len(data), None) == ESR_E_ARG
    assert h.esr_jpeg_file_info(data, -1, C.byref(info)) == ESR_E_ARG
    assert h.esr_jpeg_file_decode(data, len(data), None, 64, tables.ctypes.data, None) == ESR_E_ARG
    assert h.esr_jpeg_file_decode(data, len(data), scan.ctypes.data, 64, None, None) == ESR_E_ARG
    assert h.esr_jpeg_file_decode(data, len(data), scan.ctypes.data, 63, tables.ctypes.data, None) == ESR_E_ARG          # a scan buffer too small
    assert h.esr_jpeg_file_decode(data, len(data), scan.ctypes.data, 64, tables.ctypes.data, None) == 0
    # esr_jpeg_file_unpack: bad arguments come back before anything touches the device
    p, q = 0x1000, 0x2000
    assert h.esr_jpeg_file_unpack(None, 1, 1, 1, 1, 0, 0.0, 0.0, q, None, None, None) == ESR_E_ARG
    assert h.esr_jpeg_file_unpack(p, 1, 1, 1, 1, 0, 0.0, 0.0, None, None, None, None) == ESR_E_ARG          # no output
    assert h.esr_jpeg_file_unpack(p, 0, 1, 1, 1, 0, 0.0, 0.0, q, None, None, None) == ESR_E_ARG
    assert h.esr_jpeg_file_unpack(p, 1, -1, 1, 1, 0, 0.0, 0.0, q, None, None, None) == ESR_E_ARG
    assert h.esr_jpeg_file_unpack(p, 1, 1, 2, 1, 2, 0.0, 0.0, q, None, None, None) == ESR_E_ARG             # 4:2:2
    assert h.esr_jpeg_file_unpack(p, 1, 1, 1, 1, 1, 0.0, 0.0, q, None, None, None) == ESR_E_ARG
    assert h.esr_jpeg_file_unpack(p, 1, 1, 1, 1, 0, 0.0, 0.0, q, q, None, None) == ESR_E_ARG                # chroma output of a grey file
    assert h.esr_jpeg_file_unpack(p + 2, 1, 1, 1, 1, 0, 0.0, 0.0, q, None, None, None) == ESR_E_ARG         # scan not 16-byte aligned
    small = _lib.ActView(p, None, 4, 1, 1, 9, 9, 0)
    assert h.esr_jpeg_file_unpack(p, 1, 1, 1, 1, 0, 0.0, 0.0, q, None, small, None) == ESR_E_ARG            # fewer than 8 groups
    wrong = _lib.ActView(p, None, 8, 2, 1, 12, 12, 0)
    assert h.esr_jpeg_file_unpack(p, 1, 1, 1, 1, 0, 0.0, 0.0, q, None, wrong, None) == ESR_E_ARG            # a view of another size
    assert h.esr_jpeg_file_unpack(p, 70000, 1, 1, 1, 0, 0.0, 0.0, q, None, None, None) == ESR_E_UNSUPPORTED


def test_stand_alone_parser_under_address_and_undefined_sanitizers(tmp_path):
    """the parser header in a program of its own (csrc/jpeg_parse_check.cpp), built with -fsanitize=address,undefined, replays the prefix
    and substitution corpus of the smallest file and of a 4:2:0 file with restart markers: exit status 0, nothing reported"""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    clang = next((p for p in (os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++')) if os.path.exists(p)), None)
    assert clang, 'the ROCm clang++ was not found under %s' % rocm
    exe = str(tmp_path / 'jpeg_parse_check')
    subprocess.check_call([clang, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(CSRC, 'jpeg_parse_check.cpp'), '-o', exe])
    paths = []
    for k, data in enumerate((smallest(), corpus()['RGB_17x33_q50_opt1_rst1'], corpus()['RGB_17x33_dqt16_sof1'])):
        paths.append(str(tmp_path / ('%d.jpg' % k)))
        with open(paths[-1], 'wb') as fh:
            fh.write(data)
    run = subprocess.run([exe] + paths, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    print(run.stdout.decode(errors='replace')[-2000:])
    assert run.returncode == 0


# ------------------------------------------------------------------------------------------------ plumbing
def test_feed_data_with_qf_is_what_it_was(tmp_path):
    """'QF' takes the path it took: the tables of Set_Q_Table, the outputs the composition of the modules, the fixture's coefficients to the bit"""
    g = y_golden()
    model = make_y_model(tmp_path)
    x, Z, qf = G.image_b(), G.latent_b(), torch.tensor(G.QF_B, dtype=torch.float32)
    model.feed_data({'Uncomp': x, 'QF': qf, 'Z': Z}, need_GT=False)
    assert model.QF is qf
    assert torch.equal(model.JPEG['extractor'].Q_table.reshape(2, 64), torch.from_numpy(g['b/tables']))
    assert torch.equal(model.var_Comp, torch.from_numpy(g['b/coef']))
    model.test()
    assert torch.equal(model.output_image, model.JPEG['extractor'](model.netG(torch.cat([Z, model.JPEG['compressor'](x)], 1))).detach())
    assert float((model.fake_H - torch.from_numpy(g['b/all_layers/out'])).abs().max()) <= 1e-5


def test_feed_data_with_q_table_takes_real_tables_as_they_are(tmp_path):
    from JPEG_module.JPEG import JPEG, LUMINANCE_QUANTIZATION_TABLE
    model = make_y_model(tmp_path)
    f, _ = decoded('L_9x7_q95_opt0_rst0')
    data = f.model_data(False)
    odd = data['Q_table'].clone()
    odd[0, 0, 0], odd[0, 7, 7], odd[0, 3, 4] = 0.37, 300.7, 17.123456          # below 1, above 255, fractional
    model.feed_data(dict(data, Q_table=odd, Z=0.0), need_GT=False)
    for module in model.JPEG.values():
        assert torch.equal(module.Q_table.reshape(8, 8), odd[0]) and module.Q_table.shape == (1, 8, 8, 1, 1)
    assert model.var_Comp is not None and torch.equal(model.var_Comp, data['Comp'])
    model.test()
    assert model.output_image.shape == (1, 1, 8, 16) and f.crop(model.output_image).shape == (1, 1, 7, 9)
    # QF by Set_Q_Table(QF=False)'s formula from the luminance table given
    m = JPEG(compress=False)
    m.Set_File_Q_Table(LUMINANCE_QUANTIZATION_TABLE)
    assert m.QF == pytest.approx(50.0) and torch.equal(m.Q_table.reshape(8, 8), torch.from_numpy(LUMINANCE_QUANTIZATION_TABLE).float())
    m.Set_File_Q_Table(2.0 * LUMINANCE_QUANTIZATION_TABLE)
    assert m.QF == pytest.approx(25.0)
    with pytest.raises(ValueError):
        m.Set_File_Q_Table(np.zeros((8, 8)))
    with pytest.raises(ValueError, match='chrominance'):
        JPEG(compress=False, chroma_mode=True, block_size=16).Set_File_Q_Table(LUMINANCE_QUANTIZATION_TABLE)
    with pytest.raises(ValueError, match='Q_table'):
        model.feed_data(dict(data, Q_table=odd[0]), need_GT=False)


def test_y_model_output_requantises_to_the_files_integers(tmp_path):
    """the explorable property end to end on the CPU: compress(output, file table) without rounding lies within 0.5 of what was fed"""
    model = make_y_model(tmp_path)
    f, _ = decoded('RGB_41x57_q50_opt0_rst0')
    data = f.model_data(False)
    model.feed_data(dict(data, Z=0.3), need_GT=False)
    model.test()
    back = model.JPEG['non_quantized_compressor'](model.output_image)
    assert float((back - data['Comp']).abs().max()) <= 0.5 + 1e-3
    assert float((back - data['Comp']).abs().max()) > 0.01          # the generator moved something


def test_colour_model_takes_the_files_chroma_coefficients(tmp_path):
    model = make_colour_model(tmp_path)
    f, _ = decoded('RGB_41x57_q50_opt0_rst0')
    data = f.model_data(True)
    feed = {k: v for k, v in data.items() if k != 'compressed_chroma'}
    model.feed_data(dict(feed, Z=0.2), need_GT=False)
    assert model.var_Comp.shape == (1, 64, 8, 6)
    model.test(compressed_chroma=data['compressed_chroma'])
    assert model.var_Comp.shape == (1, 384, 4, 3) and model.output_image.shape == (1, 3, 64, 48)
    assert torch.equal(model.var_Comp[:, 256:], data['compressed_chroma'])          # exact: no rounding on this route
    for module in model.JPEG.values():
        assert module.Q_table.shape == ((1, 3, 8, 8, 1, 1) if module.chroma_mode else (1, 8, 8, 1, 1))
        assert torch.equal(module.Q_table[:, 0].reshape(8, 8) if module.chroma_mode else module.Q_table.reshape(8, 8), data['Q_table'][0])
    table = model.JPEG['extractor'].padded_Q_table
    assert torch.equal(table[0, 1, :8, :8, 0, 0], data['Q_table'][1]) and torch.equal(table[0, 1, 8:, :8, 0, 0], data['Q_table'][1][7:8].expand(8, 8))
    # the chroma planes re-quantise to the file's coefficients
    back = model.JPEG['non_quantized_compressor'](model.output_image)
    assert float((back[:, 256:] - data['compressed_chroma']).abs().max()) <= 0.5 + 1e-3
    # the reference's call pattern: the compressor's rounding drops the fractional DC term, the integers survive
    model.feed_data(dict(feed, Z=0.2), need_GT=False)
    model.test(uncompressed_chroma=f.uncompressed_chroma())
    diff = (model.var_Comp[:, 256:] - data['compressed_chroma']).reshape(2, 64, -1)
    assert float(diff[:, 1:].abs().max()) == 0 and 0 < float(diff[:, 0].abs().max()) <= 0.5
    with pytest.raises(ValueError, match="follows feed_data"):
        model.test(compressed_chroma=data['compressed_chroma'])                      # the model still holds the chroma generator's input
    model.feed_data(dict(feed, Z=0.2), need_GT=False)
    with pytest.raises(ValueError, match='compressed_chroma'):
        model.test(compressed_chroma=data['compressed_chroma'][:, :, :2])
    (tmp_path / 'y').mkdir()
    with pytest.raises(ValueError, match='colour model'):
        make_y_model(tmp_path / 'y').test(compressed_chroma=data['compressed_chroma'])


def test_z_search_runs_on_a_file_input_on_the_cpu(tmp_path):
    from Z_optimization import Z_optimizer
    model = make_y_model(tmp_path)
    f, _ = decoded('L_17x33_q50_opt0_rst0')
    data = f.model_data(False)
    Z0 = torch.zeros(1, 64, 5, 3)
    model.feed_data(dict(data, Z=Z0), need_GT=False)
    model.test()
    zo = Z_optimizer('max_STD', [5, 3], model, Z_range=1.0, max_iters=2, data=data, initial_Z=Z0, initial_LR=0.05, batch_size=1,
                     jpeg_extractor=model.JPEG['extractor'])
    Z = zo.optimize()
    assert Z.shape == (1, 64, 5, 3) and len(zo.loss_values) >= 1 and np.all(np.isfinite(zo.loss_values))


def test_z_search_on_the_colour_model_takes_the_files_chroma_coefficients(tmp_path):
    """one max_STD iteration with data = model_data(True): Z_optimizer hands 'compressed_chroma' to model.test by itself, for a batch of two
    Z samples of the one file (the [1, ...] tensors are expanded, 'Q_table' is one set for the batch)"""
    from Z_optimization import Z_optimizer
    model = make_colour_model(tmp_path)
    f, _ = decoded('RGB_41x57_q50_opt0_rst0')
    data = f.model_data(True)
    feed = {k: v for k, v in data.items() if k != 'compressed_chroma'}
    Z0 = torch.zeros(2, 64, 8, 6)
    model.feed_data(dict(feed, Comp=data['Comp'].expand(2, -1, -1, -1), Z=Z0), need_GT=False)
    model.test(compressed_chroma=data['compressed_chroma'])
    seen = []
    real_test = model.test

    def spy(*a, **k):
        seen.append(None if k.get('compressed_chroma') is None else tuple(k['compressed_chroma'].shape))
        real_test(*a, **k)
    model.test = spy
    zo = Z_optimizer('max_STD', [8, 6], model, Z_range=1.0, max_iters=1, data=data, initial_Z=Z0, initial_LR=0.05, batch_size=2,
                     jpeg_extractor=model.JPEG['extractor'])
    Z = zo.optimize()
    assert seen and all(s == (2, 128, 4, 3) for s in seen)
    assert Z.shape == (2, 64, 8, 6) and len(zo.loss_values) == 1 and np.all(np.isfinite(zo.loss_values))
    assert model.output_image.shape == (2, 3, 64, 48) and torch.equal(model.var_Comp[:, 256:], data['compressed_chroma'].expand(2, -1, -1, -1))
    assert float(Z.abs().max()) > 0                                                   # the step moved Z: the gradient arrived


def with_a_third_table(data):
    """byte surgery: Cr gets a quantisation table of its own (table 2: Cb's with one entry changed)"""
    out = bytearray(data)
    segs = header_segments(data)
    m, start, end = next(s for s in segs if s[0] in (0xC0, 0xC1))
    out[start + 4 + 6 + 3 * 2 + 2] = 2                                                # Tq of the third component
    tables = py_decode(data)['tables']
    t = tables[1].copy()
    t[63] += 1
    zz = np.zeros(64, np.int64)
    zz[:] = t[ZZ]
    dqt = b'\xff\xdb\x00\x43\x02' + bytes(int(v) for v in zz)
    return bytes(out[:start]) + dqt + bytes(out[start:])


def test_decode_tool_writes_its_pictures_and_goes_on_after_a_refusal(tmp_path, capsys):
    import importlib.util
    from test_host_jpeg_chroma import SETTINGS
    spec = importlib.util.spec_from_file_location('decode_jpegs', os.path.join(ROOT, 'tools', 'decode_jpegs.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    folder = tmp_path / 'pictures'
    folder.mkdir()
    files = {'a_colour.jpg': corpus()['RGB_41x57_q50_opt0_rst0'], 'b_grey.jpg': corpus()['L_9x7_q95_opt0_rst0'],
             'c_progressive.jpg': jpeg_bytes(16, 16, 'RGB', progressive=True),
             'd_two_chroma_tables.jpg': with_a_third_table(corpus()['RGB_16x16_q50_opt0_rst0']), 'e_444.jpeg': corpus()['RGB444_17x33_q90']}
    for n, data in files.items():
        (folder / n).write_bytes(data)
    from esr_hip import jpeg_file as JF
    two = JF.load(files['d_two_chroma_tables.jpg'])
    assert not np.array_equal(two.tables[1], two.tables[2]) and np.array_equal(two.coefficients[2], decoded('RGB_16x16_q50_opt0_rst0')[0].coefficients[2])
    cfg = json.loads(json.dumps(SETTINGS))
    cfg['path']['root'], cfg['path']['datasets'] = str(tmp_path), str(tmp_path / 'data')
    opt = tmp_path / 'test_JPEG.json'
    opt.write_text(json.dumps(cfg))
    written = lambda: sorted(n for n in os.listdir(str(folder)) if n.endswith('.png'))
    tool.main([str(folder), '--opt', str(opt), '--samples', '1'])                     # the Y model: every readable file's luminance
    said = capsys.readouterr().out
    assert 'c_progressive.jpg' in said and 'progressive' in said and 'different quantisation tables' in said
    assert written() == sorted(['a_colour_baseline.png', 'a_colour_z0.png', 'a_colour_z1.png', 'b_grey_baseline.png', 'b_grey_z0.png', 'b_grey_z1.png',
                                'd_two_chroma_tables_z0.png', 'd_two_chroma_tables_z1.png', 'e_444_baseline.png', 'e_444_z0.png', 'e_444_z1.png'])
    from PIL import Image as I
    assert I.open(str(folder / 'a_colour_baseline.png')).size == (41, 57) and I.open(str(folder / 'a_colour_z0.png')).mode == 'L'
    for n in written():
        os.remove(str(folder / n))
    tool.main([str(folder), '--opt', str(opt), '--chroma'])                           # the colour model: 4:2:0 files with one chroma table
    said = capsys.readouterr().out
    assert 'grey-scale' in said and '4:4:4' in said
    assert written() == sorted(['a_colour_baseline.png', 'a_colour_z0.png', 'b_grey_baseline.png', 'e_444_baseline.png'])
    assert I.open(str(folder / 'a_colour_z0.png')).mode == 'RGB'


# ------------------------------------------------------------------------------------------------ the committed fixture
def test_committed_files_hold_what_their_record_says():
    """tests/golden/jpeg_files: the GPU tests read only these; here they are checked against both decoders and against Pillow again"""
    from esr_hip import jpeg_file as JF
    with np.load(os.path.join(GOLDEN_DIR, 'expected.npz')) as z:
        rec = {k: z[k] for k in z.files}
    names = [str(n) for n in rec['names']]
    assert len(names) >= 5 and sorted(n + '.jpg' for n in names) == sorted(n for n in os.listdir(GOLDEN_DIR) if n.endswith('.jpg'))
    for n in names:
        path = os.path.join(GOLDEN_DIR, n + '.jpg')
        assert os.path.getsize(path) < 4096
        with open(path, 'rb') as fh:
            data = fh.read()
        f, want = JF.load(path), py_decode(data)
        planes = pillow_planes(data)
        for c in range(len(f.coefficients)):
            assert np.array_equal(f.coefficients[c], rec['%s/coef%d' % (n, c)]) and np.array_equal(f.coefficients[c], want['coef'][c])
            assert np.array_equal(f.tables[c], rec['%s/table%d' % (n, c)])
            if f.sampling != '4:4:4':          # libjpeg's IDCT: the same bits from the Pillow that wrote the record, within a level from another
                same = str(rec['pillow_version']) == PIL.__version__
                assert np.abs(planes[c] - rec['%s/pillow%d' % (n, c)]).max() <= (0 if same else 1), (n, c)
