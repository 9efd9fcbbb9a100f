"""The JPEG consistency layer under the reference's module path and names (codes/JPEG_module/JPEG.py): block DCT, per-image quantisation
table, and back — the Y-channel layer (chroma_mode False, 8x8 blocks) and the colour model's (chroma_mode True, 16x16 blocks: Y whole, Cb and Cr
down-sampled by keeping their low 8x8 frequencies).  The arithmetic lives in esr_hip/jpeg.py (HIP kernels for GPU tensors, the defining torch
expression for CPU tensors).  The device follows the input (the reference hard-codes 'cuda'); of the reference's module constants
FACTORIZE_CHROMA_HIGH_FREQS is True (the only setting it still supports) and the HIGH_FREQS_ONLY debug switch is not reproduced."""
import numpy as np
import torch
import torch.nn as nn

from esr_hip import jpeg as J

LUMINANCE_QUANTIZATION_TABLE = np.array((
    (16, 11, 10, 16, 24, 40, 51, 61),
    (12, 12, 14, 19, 26, 58, 60, 55),
    (14, 13, 16, 24, 40, 57, 69, 56),
    (14, 17, 22, 29, 51, 87, 80, 62),
    (18, 22, 37, 56, 68, 109, 103, 77),
    (24, 36, 55, 64, 81, 104, 113, 92),
    (49, 64, 78, 87, 103, 121, 120, 101),
    (72, 92, 95, 98, 112, 100, 103, 99)
))          # ITU-T T.81 Annex K, table K.1

CHROMINANCE_QUANTIZATION_TABLE = np.array((
    (17, 18, 24, 47, 99, 99, 99, 99),
    (18, 21, 26, 66, 99, 99, 99, 99),
    (24, 26, 56, 99, 99, 99, 99, 99),
    (47, 66, 99, 99, 99, 99, 99, 99),
    (99, 99, 99, 99, 99, 99, 99, 99),
    (99, 99, 99, 99, 99, 99, 99, 99),
    (99, 99, 99, 99, 99, 99, 99, 99),
    (99, 99, 99, 99, 99, 99, 99, 99)
))          # ITU-T T.81 Annex K, table K.2


class JPEG(nn.Module):
    """chroma_mode False (block_size 8).  compress=True: [B, 1, H, W] image (0...255) -> [B, 64, H/8, W/8] coefficients divided by the table,
    rounded when downsample_or_quantize is True.  compress=False: the way back.  H and W multiples of 8.

    chroma_mode True (block_size 16).  compress=True: [B, 3, H, W] YCbCr -> [B, 384, H/16, W/16] = Y's 256 coefficients (never rounded) | the
    low 8x8 of Cb | of Cr, rounded when downsample_or_quantize is True, unrounded for 'downsample_only'; False gives all 3 * 256 unrounded.
    compress=False: by the channel count 128 / 512 (Cb, Cr -> [B, 2, H, W]) or 384 (-> [B, 3, H, W]).  Coefficients are divided by the tables
    edge-padded to 16x16 (padded_Q_table).  H and W multiples of 16.

    Set_Q_Table before the first forward."""

    def __init__(self, compress, downsample_or_quantize=None, chroma_mode=False, block_size=8):
        super(JPEG, self).__init__()
        assert (compress ^ (downsample_or_quantize is None)), 'Quantize argument should be passed iff in compress mode'
        if downsample_or_quantize is not None:
            assert downsample_or_quantize in ['downsample_only', True, False]
        if chroma_mode and block_size != 16:
            raise NotImplementedError('JPEG(chroma_mode=True, block_size=%r): the colour model works on 16x16 blocks (4:2:0 chroma; the model passes '
                                      "block_size=opt['scale'] = 16)" % (block_size,))
        if not chroma_mode and block_size != 8:
            raise NotImplementedError('JPEG(block_size=%r) without chroma_mode: the Y-channel layer works on 8x8 blocks; 16x16 blocks belong to '
                                      'chroma_mode=True' % (block_size,))
        if downsample_or_quantize == 'downsample_only' and not chroma_mode:
            raise NotImplementedError("JPEG(downsample_or_quantize='downsample_only') belongs to chroma_mode=True (the reference asserts the same)")
        self.compress = compress
        self.downsample_or_quantize = downsample_or_quantize
        self.block_size = block_size
        self.chroma_mode = chroma_mode
        self.synthetic_Q_table = self.process_Q_table(LUMINANCE_QUANTIZATION_TABLE)
        if self.chroma_mode:
            self.synthetic_Q_table = self._three(self.synthetic_Q_table, self.process_Q_table(CHROMINANCE_QUANTIZATION_TABLE))
            self.synthetic_padded_Q_table = self._three(self.process_Q_table(self._padded(LUMINANCE_QUANTIZATION_TABLE)),
                                                        self.process_Q_table(self._padded(CHROMINANCE_QUANTIZATION_TABLE)))

    def process_Q_table(self, Q_table):
        return torch.from_numpy(Q_table / 100).view(1, Q_table.shape[0], Q_table.shape[1], 1, 1).type(torch.FloatTensor)

    def _padded(self, table):
        """edge-padded to block_size x block_size: the high frequencies are divided by the nearest listed entry (JPEG.py:62)"""
        return np.pad(np.asarray(table), ((0, self.block_size - 8), (0, self.block_size - 8)), 'edge')

    @staticmethod
    def _three(luminance, chrominance):
        """[1, 3, n, n, 1, 1]: the luminance table and twice the chrominance one"""
        return torch.cat([luminance.unsqueeze(1), chrominance.unsqueeze(1).repeat([1, 2, 1, 1, 1, 1])], 1)

    def Set_Q_Table(self, QF_or_table, QF=True):
        """QF=True: a tensor of quality factors, one per image.  QF=False: [table] ([luminance, chrominance] with chroma_mode) with explicit 8x8
        tables (taken as the reference takes them, through process_Q_table), self.QF derived from the luminance one."""
        if QF:
            self.QF = QF_or_table
            table = self.synthetic_Q_table.to(QF_or_table.device)
            condition = (QF_or_table < 50).type(self.QF.type())
            self.factor = (condition * (5000 / QF_or_table) + (1 - condition) * (200 - 2 * QF_or_table))
            self.factor = self.factor.view([-1, 1, 1, 1, 1] + ([1] if self.chroma_mode else [])).type(table.dtype)
            self.Q_table = torch.clamp((self.factor * table).round(), 1, 255)
            if self.chroma_mode:
                self.padded_Q_table = torch.clamp((self.factor * self.synthetic_padded_Q_table.to(QF_or_table.device)).round(), 1, 255)
        else:
            tables_ratio = np.mean(LUMINANCE_QUANTIZATION_TABLE / QF_or_table[0])
            self.QF = 50 * tables_ratio if tables_ratio < 1 else 50 * np.mean((2 * LUMINANCE_QUANTIZATION_TABLE - QF_or_table[0]) / LUMINANCE_QUANTIZATION_TABLE)
            self.Q_table = self.process_Q_table(np.asarray(QF_or_table[0]))
            if self.chroma_mode:
                self.Q_table = self._three(self.Q_table, self.process_Q_table(np.asarray(QF_or_table[1])))
                self.padded_Q_table = self._three(self.process_Q_table(self._padded(QF_or_table[0])), self.process_Q_table(self._padded(QF_or_table[1])))

    def Set_File_Q_Table(self, luminance, chrominance=None):
        """The tables of a JPEG file in the model's domain (esr_hip.jpeg_file.JpegFile.model_data): real-valued [8, 8] arrays or tensors, taken
        as they are — not rounded, not clamped to 1...255, not divided by 100 (Set_Q_Table(QF=False) does the last, as the reference does).
        chroma_mode needs both; the 16x16 tables are the edge-padded ones.  self.QF: from the luminance table given, by Set_Q_Table(QF=False)'s
        formula."""
        def as_numpy(t):
            t = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
            if t.shape != (8, 8) or not np.all(np.isfinite(t)) or not np.all(t > 0):
                raise ValueError('JPEG.Set_File_Q_Table: positive [8, 8] tables, got shape %s' % (t.shape,))
            return t.astype(np.float64)

        def as_table(t):
            return torch.from_numpy(t).view(1, t.shape[0], t.shape[1], 1, 1).type(torch.FloatTensor)
        luminance = as_numpy(luminance)
        tables_ratio = np.mean(LUMINANCE_QUANTIZATION_TABLE / luminance)
        self.QF = 50 * tables_ratio if tables_ratio < 1 else 50 * np.mean((2 * LUMINANCE_QUANTIZATION_TABLE - luminance) / LUMINANCE_QUANTIZATION_TABLE)
        self.Q_table = as_table(luminance)
        if self.chroma_mode:
            if chrominance is None:
                raise ValueError('JPEG.Set_File_Q_Table: chroma_mode needs the chrominance table as well')
            chrominance = as_numpy(chrominance)
            self.Q_table = self._three(self.Q_table, as_table(chrominance))
            self.padded_Q_table = self._three(as_table(self._padded(luminance)), as_table(self._padded(chrominance)))

    def _table_on(self, device):
        name = 'padded_Q_table' if self.chroma_mode else 'Q_table'
        if not hasattr(self, name):
            raise RuntimeError('JPEG: Set_Q_Table before the first call')
        if getattr(self, name).device != device:
            setattr(self, name, getattr(self, name).to(device))
        return getattr(self, name)

    def Multiply_By_Q_table(self, input):
        input_shape = input.shape
        if self.Q_table.device != input.device:
            self.Q_table = self.Q_table.to(input.device)
        return (input.view(input_shape[0], 8, 8, input_shape[2], input_shape[3]) * self.Q_table).view(input_shape)

    def forward(self, input):
        table = self._table_on(input.device)
        if self.chroma_mode:
            if self.compress:
                return J.compress16(input, table, self.downsample_or_quantize)
            return J.extract16(input, table)[1]
        if self.compress:
            return J.compress(input, table, bool(self.downsample_or_quantize))
        return J.extract(input, table)[1]
