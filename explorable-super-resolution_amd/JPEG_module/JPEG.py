"""The JPEG consistency layer under the reference's module path and names (codes/JPEG_module/JPEG.py): 8x8 block DCT, per-image quantisation
table, and back.  Y-channel model only (chroma_mode False, block size 8); the arithmetic lives in esr_hip/jpeg.py (HIP kernels for GPU tensors,
the defining torch expression for CPU tensors).  The device follows the input (the reference hard-codes 'cuda'); the reference's
HIGH_FREQS_ONLY debug constant is not reproduced."""
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


class JPEG(nn.Module):
    """compress=True: [B, 1, H, W] image (0...255) -> [B, 64, H/8, W/8] coefficients divided by the table, rounded when
    downsample_or_quantize is True.  compress=False: the way back.  H and W multiples of 8.  Set_Q_Table before the first forward."""

    def __init__(self, compress, downsample_or_quantize=None, chroma_mode=False, block_size=8):
        super(JPEG, self).__init__()
        assert (compress ^ (downsample_or_quantize is None)), 'Quantize argument should be passed iff in compress mode'
        if downsample_or_quantize is not None:
            assert downsample_or_quantize in ['downsample_only', True, False]
        if chroma_mode:
            raise NotImplementedError('JPEG(chroma_mode=True): this build runs the Y-channel (grey-scale) model only')
        if block_size != 8:
            raise NotImplementedError('JPEG(block_size=%r): the kernels implement 8x8 blocks (the Y-channel model)' % (block_size,))
        if downsample_or_quantize == 'downsample_only':
            raise NotImplementedError("JPEG(downsample_or_quantize='downsample_only') belongs to the chroma model, which this build does not run")
        self.compress = compress
        self.downsample_or_quantize = downsample_or_quantize
        self.block_size = block_size
        self.chroma_mode = chroma_mode
        self.synthetic_Q_table = self.process_Q_table(LUMINANCE_QUANTIZATION_TABLE)

    def process_Q_table(self, Q_table):
        return torch.from_numpy(Q_table / 100).view(1, Q_table.shape[0], Q_table.shape[1], 1, 1).type(torch.FloatTensor)

    def Set_Q_Table(self, QF_or_table, QF=True):
        """QF=True: a tensor of quality factors, one per image.  QF=False: [table] with an explicit 8x8 table (taken as the reference takes
        it, through process_Q_table), self.QF derived from it."""
        if QF:
            self.QF = QF_or_table
            table = self.synthetic_Q_table.to(QF_or_table.device)
            condition = (QF_or_table < 50).type(self.QF.type())
            self.factor = (condition * (5000 / QF_or_table) + (1 - condition) * (200 - 2 * QF_or_table))
            self.factor = self.factor.view([-1, 1, 1, 1, 1]).type(table.dtype)
            self.Q_table = torch.clamp((self.factor * table).round(), 1, 255)
        else:
            tables_ratio = np.mean(LUMINANCE_QUANTIZATION_TABLE / QF_or_table[0])
            self.QF = 50 * tables_ratio if tables_ratio < 1 else 50 * np.mean((2 * LUMINANCE_QUANTIZATION_TABLE - QF_or_table[0]) / LUMINANCE_QUANTIZATION_TABLE)
            self.Q_table = self.process_Q_table(np.asarray(QF_or_table[0]))

    def _table_on(self, device):
        if not hasattr(self, 'Q_table'):
            raise RuntimeError('JPEG: Set_Q_Table before the first call')
        if self.Q_table.device != device:
            self.Q_table = self.Q_table.to(device)
        return self.Q_table

    def Multiply_By_Q_table(self, input):
        input_shape = input.shape
        return (input.view(input_shape[0], 8, 8, input_shape[2], input_shape[3]) * self._table_on(input.device)).view(input_shape)

    def forward(self, input):
        table = self._table_on(input.device)
        if self.compress:
            return J.compress(input, table, bool(self.downsample_or_quantize))
        return J.extract(input, table)[1]
