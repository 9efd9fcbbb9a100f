"""JPEG files into the explorable decoder's inputs: load(path_or_bytes) -> JpegFile.

The entropy decoder is host C++ in the library (csrc/esr_jpeg_parse.h behind esr_jpeg_file_info / esr_jpeg_file_decode; no GPU needed): it
yields the file's quantised integers q in scan order and its tables Q.  One esr_jpeg_file_unpack launch (csrc/esr_jpeg_file.hip) turns the
uploaded scan buffer into the models' coefficient tensors; for CPU tensors the same is the indexing expression of _unpack_cpu.

The mapping.  A file is JFIF full-range YCbCr, the networks live in BT.601 studio range (data.util.rgb2ycbcr, Tensor_YCbCR2RGB):
Y_s = 16 + a Y_f, C_s = 128 + b (C_f - 128), a = 219/255, b = 224/255, no mixing.  esr_hip.jpeg's 8-point layer is T.81's transform
(orthonormal DCT-II, level shift 128, channel 8u + v with u the vertical frequency), so a component decodes as 128 + iDCT(q Q), and the
model-domain inputs are exact:
  * Y, 8 x 8 grid: table T_Y = a Q_Y; coefficients q, plus 8 (16 - 128 (1 - a)) / T_Y[0, 0] on the DC channel (the constant 16 + 128 a - 128).
  * Cb, Cr of a 4:2:0 file, on the colour model's 16 x 16 grid (low 8 x 8 of the 16-point transform, which has no level shift for chroma):
    DCT-domain x2 upsampling scales every coefficient by 2, so T_C = 2 b Q_C, edge-padded as JPEG._padded does; coefficients q, plus
    2048 / T_C[0, 0] on DC (the constant 128 over 16 x 16 pixels).
These tables are real-valued: JPEG.Set_File_Q_Table takes them as they are.  extract adds sigmoid(y) - 0.5 to whatever centre it is given,
so every output of the models re-quantises to the file's own integers under the file's own tables.

Y model: grey files and the Y component of colour files.  Colour model: 4:2:0 files only (grey and 4:4:4 are refused by name)."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from . import jpeg as J
from ._lib import JpegInfo, check
from .act import stream_ptr

A_LUMA = 219.0 / 255.0
B_CHROMA = 224.0 / 255.0
MAX_WORKERS = 16

# natural index (8u + v) of the k-th coefficient of a block in the file (T.81 figure A.6), and its inverse
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
ZIGZAG_POS = np.argsort(ZIGZAG)

_REASONS = {
    1: 'a progressive JPEG (SOF2)', 2: 'a lossless or hierarchical JPEG (SOF3, SOF5-7)', 3: 'an arithmetic-coded JPEG',
    4: 'a JPEG with 12-bit samples', 5: 'a JPEG with a non-interleaved scan or several scans',
    6: 'chroma sampling other than 4:2:0 or 4:4:4 (4:2:2, 4:4:0, ...)', 7: 'a JPEG with 2 or 4 components (CMYK / YCCK)',
    8: 'an RGB JPEG (Adobe APP14 segment with transform 0; three components are read as YCbCr)',
    32: 'the file is truncated', 33: 'a Huffman code that is in no table (or a coefficient category out of range)',
    34: 'a zero run past coefficient 63', 35: 'a table the scan refers to is missing', 36: 'a wrong restart marker',
    37: 'a zero width or height', 38: 'a malformed segment', 39: 'no SOI marker: not a JPEG file'}


class JpegFileError(_lib.EsrError, ValueError):
    """the bytes are not a JPEG file this library can read (ESR_E_DATA): truncated or corrupt"""


class JpegFileUnsupported(_lib.EsrError, NotImplementedError):
    """a valid JPEG of a kind the decoder does not take (ESR_E_UNSUPPORTED): progressive, arithmetic, 12-bit, 4:2:2, CMYK, ..."""


def _raise(rc, info, name):
    words = _REASONS.get(int(info.reason), 'reason %d' % info.reason)
    if rc == _lib.ESR_E_UNSUPPORTED:
        raise JpegFileUnsupported('%s: %s is not supported (baseline Huffman JPEGs with one interleaved scan: grey, 4:2:0 or 4:4:4)' % (name, words))
    if rc == _lib.ESR_E_DATA:
        raise JpegFileError('%s: %s' % (name, words))
    check(rc, 'esr_jpeg_file_decode(%s)' % name)


def decode_bytes(data, name='<bytes>'):
    """(info, scan int16 [scan_blocks * 64], tables uint16 [4, 64]): the host side alone.  The ctypes calls release the GIL."""
    data = bytes(data)
    info = JpegInfo()
    rc = _lib.lib.esr_jpeg_file_info(data, len(data), C.byref(info))
    if rc != 0:
        _raise(rc, info, name)
    scan = np.empty(64 * info.scan_blocks, dtype=np.int16)
    tables = np.zeros((4, 64), dtype=np.uint16)
    rc = _lib.lib.esr_jpeg_file_decode(data, len(data), scan.ctypes.data, scan.size, tables.ctypes.data, C.byref(info))
    if rc != 0:
        _raise(rc, info, name)
    return info, scan, tables


def _unpack_cpu(scan, mcus_h, mcus_w, y_h, y_v, n_chroma, y_dc, c_dc):
    """the defining expression of esr_jpeg_file_unpack: (Y [1, 64, mcus_h y_v, mcus_w y_h], chroma [1, 128, mcus_h, mcus_w] or None)"""
    ny = y_h * y_v
    s = scan.view(mcus_h, mcus_w, ny + n_chroma, 64)[..., torch.from_numpy(ZIGZAG_POS)]
    y = s[:, :, :ny].reshape(mcus_h, mcus_w, y_v, y_h, 64).permute(4, 0, 2, 1, 3).reshape(1, 64, mcus_h * y_v, mcus_w * y_h).float()
    y[:, 0] += y_dc
    c = None
    if n_chroma:
        c = s[:, :, ny:].permute(2, 3, 0, 1).reshape(1, 128, mcus_h, mcus_w).float()
        c[:, 0] += c_dc
        c[:, 64] += c_dc
    return y, c


def unpack(scan, mcus_h, mcus_w, y_h, y_v, n_chroma, y_dc=0.0, c_dc=0.0, want_chroma=True, act_view=None):
    """scan: int16 tensor in scan order, on the CPU or uploaded.  -> (Y coefficients fp32, chroma coefficients fp32 or None); on the GPU one
    esr_jpeg_file_unpack launch, which also writes Y into groups [0, 8) of act_view when one is given."""
    if scan.dtype != torch.int16 or scan.numel() != mcus_h * mcus_w * (y_h * y_v + n_chroma) * 64:
        raise ValueError('jpeg_file.unpack: %d int16 values for %d x %d MCUs of %d blocks' % (scan.numel(), mcus_h, mcus_w, y_h * y_v + n_chroma))
    want_chroma = bool(want_chroma and n_chroma)
    if not scan.is_cuda:
        if act_view is not None:
            raise ValueError('jpeg_file.unpack: an activation view belongs to the GPU path')
        y, c = _unpack_cpu(scan.contiguous(), mcus_h, mcus_w, y_h, y_v, n_chroma, y_dc, c_dc)
        return y, (c if want_chroma else None)
    scan = scan.contiguous()
    y = torch.empty(1, 64, mcus_h * y_v, mcus_w * y_h, dtype=torch.float32, device=scan.device)
    c = torch.empty(1, 128, mcus_h, mcus_w, dtype=torch.float32, device=scan.device) if want_chroma else None
    check(_lib.lib.esr_jpeg_file_unpack(scan.data_ptr(), mcus_h, mcus_w, y_h, y_v, n_chroma, y_dc, c_dc, y.data_ptr(),
                                        None if c is None else c.data_ptr(), None if act_view is None else C.byref(act_view), stream_ptr()),
          'esr_jpeg_file_unpack')
    return y, c


class JpegFile:
    """A decoded file.  height, width: the picture's; sampling: 'gray' | '4:2:0' | '4:4:4'; coefficients: the file's integers, one
    [64, hb, wb] int16 array per component (channel 8u + v, block grid padded to whole MCUs); tables: the file's [8, 8] tables, one per
    component; restart_interval, sof (0 or 1), name."""

    def __init__(self, info, scan, tables, device=None, name='<bytes>'):
        self.name = name
        self.height, self.width = int(info.height), int(info.width)
        self.components = int(info.components)
        self.sampling = 'gray' if self.components == 1 else ('4:2:0' if info.h[0] == 2 else '4:4:4')
        self.sof, self.restart_interval = int(info.sof), int(info.restart_interval)
        self.mcus_h, self.mcus_w = int(info.mcus_h), int(info.mcus_w)
        self.y_h, self.y_v = int(info.h[0]), int(info.v[0])
        self.n_chroma = self.components - 1
        self.scan = scan
        self.tables = [tables[info.tq[c]].reshape(8, 8).copy() for c in range(self.components)]
        self.device = torch.device('cpu' if device is None else device)
        self._unpacked = {}
        self._scan_on_device = None
        self._coefficients = None

    # ---- the file's own numbers
    @property
    def padded_size(self):
        """(H, W) of the block grid in pixels: what the models work on"""
        return 8 * self.mcus_h * self.y_v, 8 * self.mcus_w * self.y_h

    @property
    def coefficients(self):
        if self._coefficients is None:
            ny = self.y_h * self.y_v
            s = self.scan.reshape(self.mcus_h, self.mcus_w, ny + self.n_chroma, 64)[..., ZIGZAG_POS]
            y = s[:, :, :ny].reshape(self.mcus_h, self.mcus_w, self.y_v, self.y_h, 64).transpose(4, 0, 2, 1, 3)
            out = [np.ascontiguousarray(y.reshape(64, self.mcus_h * self.y_v, self.mcus_w * self.y_h))]
            for c in range(self.n_chroma):
                out.append(np.ascontiguousarray(s[:, :, ny + c].transpose(2, 0, 1)))
            self._coefficients = out
        return self._coefficients

    # ---- the models' domain
    def model_tables(self):
        """(T_Y, T_C or None): float64 [8, 8]; T_C is the colour model's (4:2:0 on its 16 x 16 grid)"""
        t_y = A_LUMA * self.tables[0].astype(np.float64)
        t_c = 2 * B_CHROMA * self.tables[1].astype(np.float64) if self.n_chroma else None
        return t_y, t_c

    def _offsets(self):
        t_y, t_c = self.model_tables()
        y_dc = 8 * (16 - 128 * (1 - A_LUMA)) / t_y[0, 0]
        return y_dc, (2048 / t_c[0, 0] if t_c is not None else 0.0)

    def _model_coefficients(self, colour):
        key = 'colour' if colour else 'y'
        if key not in self._unpacked:
            y_dc, c_dc = self._offsets()
            self._unpacked[key] = unpack(self._uploaded_scan(), self.mcus_h, self.mcus_w, self.y_h, self.y_v, self.n_chroma, y_dc, c_dc, want_chroma=colour)
        return self._unpacked[key]

    def _uploaded_scan(self):
        """the scan buffer on self.device, copied there once"""
        if self._scan_on_device is None:
            self._scan_on_device = torch.from_numpy(self.scan).to(self.device)
        return self._scan_on_device

    def _check_colour(self):
        if self.sampling != '4:2:0':
            raise NotImplementedError('%s: the colour model takes 4:2:0 files (its chroma lives on 16 x 16 blocks); this file is %s — '
                                      'the Y model takes its luminance' % (self.name, 'grey-scale' if self.sampling == 'gray' else self.sampling))
        if not np.array_equal(self.tables[1], self.tables[2]):
            raise NotImplementedError('%s: Cb and Cr use different quantisation tables; the colour model has one chrominance table' % self.name)

    def model_data(self, chroma_mode=False):
        """DecompCNNModel.feed_data's dict: 'Comp' (Y on the 8 x 8 grid, [1, 64, H/8, W/8]) and 'Q_table' ([1 or 2, 8, 8] real tables, on the host); with
        chroma_mode also 'compressed_chroma' [1, 128, H/16, W/16] for model.test(compressed_chroma=...) (Z_optimizer passes it on by itself)."""
        t_y, t_c = self.model_tables()
        if chroma_mode:
            self._check_colour()
        y, c = self._model_coefficients(bool(chroma_mode))
        tables = np.stack([t_y, t_c]) if chroma_mode else t_y[None]
        data = {'Comp': y, 'Q_table': torch.from_numpy(tables.astype(np.float32))}      # (a host tensor: the JPEG modules build their tables from it)
        if chroma_mode:
            data['compressed_chroma'] = c
        return data

    def uncompressed_chroma(self):
        """[1, 2, H, W] studio-range Cb, Cr planes for the reference's call pattern, model.test(uncompressed_chroma=...) after feed_data of
        model_data()'s 'Comp'.  The model compresses and ROUNDS them again: the integers come back, the fractional DC term 2048 / T_C[0, 0]
        is lost to that rounding (up to half a quantisation step of DC) — compressed_chroma is the exact route."""
        self._check_colour()
        _, t_c = self.model_tables()
        _, c = self._model_coefficients(True)
        return J.extract16(c, self._padded3(t_c))[1]

    def _padded3(self, t_c):
        t_y, _ = self.model_tables()
        pad = lambda t: np.pad(t, ((0, 8), (0, 8)), 'edge')
        return torch.from_numpy(np.stack([pad(t_y), pad(t_c), pad(t_c)]).reshape(1, 3, 256).astype(np.float32)).to(self.device)

    def baseline_image(self):
        """What an ordinary decoder shows, on the library's extract kernels with no generator: [1, C, height, width] in 0...1, grey or RGB
        (Output_Image_0_1's conversion, clamped)."""
        t_y, t_c = self.model_tables()
        as_q = lambda t: torch.from_numpy(t.reshape(1, 64).astype(np.float32)).to(self.device)
        if self.sampling == 'gray':
            y, _ = self._model_coefficients(False)
            return self.crop(torch.clamp(J.extract(y, as_q(t_y))[1] / 255, 0, 1))
        if self.sampling == '4:2:0':
            self._check_colour()
            y, c = self._model_coefficients(True)
            chroma = J.extract16(c, self._padded3(t_c))[1]
        else:                                           # 4:4:4: chroma on the 8 x 8 grid, C_s = 128 + b iDCT(q Q): the 8-point extractor as it is
            y_dc, _ = self._offsets()
            y, c = unpack(self._uploaded_scan(), self.mcus_h, self.mcus_w, 1, 1, 2, y_dc, 0.0)
            chroma = torch.cat([J.extract(c[:, 64 * k:64 * k + 64].contiguous(), as_q(B_CHROMA * self.tables[1 + k].astype(np.float64)))[1]
                                for k in range(2)], 1)
        ycc = torch.cat([J.extract(y, as_q(t_y))[1], chroma], 1)
        if ycc.is_cuda:
            from . import jpeg_edit
            rgb = jpeg_edit.ycbcr_to_rgb(ycc)
        else:
            from models.DecompCNN_model import Tensor_YCbCR2RGB
            rgb = Tensor_YCbCR2RGB(ycc / 255)
        return self.crop(torch.clamp(rgb, 0, 1))

    def crop(self, t):
        """a padded-size output [..., H, W] cut to the picture's height x width"""
        return t[..., :self.height, :self.width]


def _read(path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return bytes(path_or_bytes), '<bytes>'
    with open(path_or_bytes, 'rb') as f:
        return f.read(), os.path.basename(str(path_or_bytes))


def load(path_or_bytes, device=None):
    """A file's path or its bytes -> JpegFile with tensors on `device` (default: the CPU).  JpegFileUnsupported (a NotImplementedError) names
    what kind of JPEG was refused, JpegFileError (a ValueError) what is wrong with the bytes."""
    data, name = _read(path_or_bytes)
    return JpegFile(*decode_bytes(data, name), device=device, name=name)


def load_many(paths, device=None, on_error=None):
    """load() of every path, the entropy decoding on a pool of min(16, len(paths)) threads (the library calls release the GIL).
    on_error(path, exception): when given, a file that is refused is reported to it and left out of the result instead of raising."""
    paths = list(paths)
    if not paths:
        return []

    def host(p):
        try:
            data, name = _read(p)
            return decode_bytes(data, name) + (name,)
        except (JpegFileError, JpegFileUnsupported) as e:
            if on_error is None:
                raise
            return e
    with ThreadPoolExecutor(max_workers=min(MAX_WORKERS, len(paths))) as pool:
        decoded = list(pool.map(host, paths))
    files = []
    for p, d in zip(paths, decoded):
        if isinstance(d, Exception):
            on_error(p, d)
        else:
            files.append(JpegFile(d[0], d[1], d[2], device=device, name=d[3]))
    return files
