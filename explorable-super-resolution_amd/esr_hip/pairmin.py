"""Host side of the random-alternatives Z objectives 'random_l1', 'random_l1_limited', 'random_VGG' (reference codes/Z_optimization.py:683-701;
what the GUI's "produce random alternatives" tool sends, GUI.py:1833-1835): the one term that couples the samples of a batch.

With D = clamp(x, 0, 1) (clamp01; the image objectives) or x (feature tensors) of the GLOBAL batch [Bg, C, H, W]:
    near[b] = min(1, min_{a != b} |D[b] - D[a]|)                     (the reference's `min_a(|D[b] - D[a]| + eye[a, b])`; Bg = 1: the constant 1)
    v[b]    = (near[b] - w |D[b] - init|) mask                       (the second term with `init` only, the mask when given)
    Z_loss[b] = -mean_{c,h,w} v[b],        loss = mean_b Z_loss[b]   over the global batch
random_share(x_local, ...) returns, for the rows [lo, lo + B_local) this rank owns, the detached Z_loss of these rows and the scalar
    share = sum_{b local} Z_loss[b] / Bg
whose sum over ranks is the loss.  Its BACKWARD is the derivative of the global loss with respect to the local rows: their own terms plus the
terms they receive as the nearest neighbour of any row, remote rows included (the other ranks' rows enter detached, gathered by the caller).
GPU: csrc/esr_pairmin.hip, which never builds the reference's [Bg, Bg, C, H, W] tensor; an exact tie between neighbours goes to the lowest row
index there.  CPU: the defining torch expression (torch.min's own choice on ties).
"""
import torch

from . import _lib
from ._image import as_f32, detach_f32, ptr
from ._lib import check
from .act import stream_ptr


def z_loss_defining(D, mask=None, init=None, w=0.0):
    """Z_loss [B] of the whole batch D [B, C, H, W] (already clamped where that applies), as the reference writes it (:688-699); any dtype"""
    B = D.size(0)
    eye = torch.eye(B, dtype=D.dtype, device=D.device).view(B, B, 1, 1, 1)
    v = torch.min((D.unsqueeze(0) - D.unsqueeze(1)).abs() + eye, dim=0)[0]
    if init is not None:
        v = v - w * (D - init.to(D.dtype)).abs()
    if mask is not None:
        v = v * mask.to(D.dtype)
    return -1 * v.mean(dim=(1, 2, 3))


def _check(x_local, x_all, lo, mask, init):
    if x_local.dim() != 4 or x_all.dim() != 4 or tuple(x_all.shape[1:]) != tuple(x_local.shape[1:]):
        raise ValueError('pairmin: local rows %s, global batch %s' % (tuple(x_local.shape), tuple(x_all.shape)))
    Bl, C, H, W = x_local.shape
    if lo < 0 or lo + Bl > x_all.size(0):
        raise ValueError('pairmin: rows [%d, %d) of a batch of %d' % (lo, lo + Bl, x_all.size(0)))
    if mask is not None and tuple(mask.shape) != (H, W):
        raise ValueError('pairmin: mask %s for images of %d x %d' % (tuple(mask.shape), H, W))
    if init is not None and (init.dim() != 4 or init.size(0) not in (1, Bl) or tuple(init.shape[1:]) != (C, H, W)):
        raise ValueError('pairmin: initial image %s for rows %s (its batch must be 1 or %d)' % (tuple(init.shape), tuple(x_local.shape), Bl))


def _share_cpu(x_local, x_all, lo, clamp01, mask, init, w):
    Bl, Bg = x_local.size(0), x_all.size(0)
    full = torch.cat([x_all[:lo], x_local, x_all[lo + Bl:]], 0)                 # the local rows attached, the others detached
    D = torch.clamp(full, 0, 1) if clamp01 else full
    if init is not None and init.size(0) != 1:                                  # the 'limited' term is per local row: zero weight on the others
        pad = D.detach().clone()
        pad[lo:lo + Bl] = init.to(D.dtype)
        init = pad
    Z = z_loss_defining(D, mask, init, w)
    local = Z[lo:lo + Bl]
    total = Z.sum() / Bg
    # the value of the local share with the gradient of the global loss (module docstring)
    return local.detach(), total + (local.sum() / Bg - total).detach()


def _scratch(xa, lo, hi, grad):
    Bg, C, H, W = xa.shape
    n = _lib.lib.esr_pairmin_work_floats(Bg, C, H, W, lo, hi, grad)
    if n < 0:
        check(int(n), 'esr_pairmin_work_floats')
    return torch.empty(int(n), dtype=torch.float32, device=xa.device) if n else None


class _PairMin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_local, x_all, lo, clamp01, mask, init, w):
        Bl = x_local.size(0)
        Bg, C, H, W = x_all.shape
        work = _scratch(x_all, lo, lo + Bl, 0)
        blocks = int(_lib.lib.esr_pairmin_blocks(C, H, W))
        partial = torch.empty(Bl, blocks, dtype=torch.float64, device=x_all.device)
        check(_lib.lib.esr_pairmin(x_all.data_ptr(), Bg, C, H, W, lo, lo + Bl, int(clamp01), ptr(mask), ptr(init), 0 if init is None else init.size(0),
                                   float(w), ptr(work), partial.data_ptr(), stream_ptr()), 'esr_pairmin')
        Z = -partial.sum(1) / (C * H * W)
        ctx.save_for_backward(x_all, mask, init)
        ctx.args = (lo, Bl, bool(clamp01), float(w))
        return Z.float(), (Z.sum() / Bg).float()

    @staticmethod
    def backward(ctx, gZ, gS):
        x_all, mask, init = ctx.saved_tensors
        lo, Bl, clamp01, w = ctx.args
        Bg, C, H, W = x_all.shape
        work = _scratch(x_all, lo, lo + Bl, 1)
        dx = torch.empty(Bl, C, H, W, dtype=torch.float32, device=x_all.device)
        scale = -(0.0 if gS is None else float(gS)) / (float(C) * H * W * Bg)
        check(_lib.lib.esr_pairmin_grad(x_all.data_ptr(), Bg, C, H, W, lo, lo + Bl, int(clamp01), ptr(mask), ptr(init), 0 if init is None else init.size(0),
                                        w, scale, ptr(work), dx.data_ptr(), stream_ptr()), 'esr_pairmin_grad')
        return dx, None, None, None, None, None, None


def random_share(x_local, x_all=None, lo=0, clamp01=True, mask=None, init=None, w=0.0):
    """(Z_loss of the local rows [B_local], detached;  share = sum of them / Bg, differentiable as the module docstring says).
    x_local [B_local, C, H, W]: this rank's rows, attached to the graph; x_all [Bg, C, H, W]: every rank's rows, detached, in rank order, holding
    x_local's values at [lo, lo + B_local) - None when the local rows are the whole batch.  mask [H, W] or None; init [1 or B_local, C, H, W]
    with its weight w (the '*_limited' term) or None."""
    xl = as_f32(x_local)
    xa = detach_f32(xl if x_all is None else x_all)
    _check(xl, xa, lo, mask, init)
    if mask is not None:
        mask = detach_f32(mask)
    if init is not None:
        init = detach_f32(init)
    if not xl.is_cuda:
        return _share_cpu(xl, xa, lo, clamp01, mask, init, float(w))
    Z, share = _PairMin.apply(xl, xa, lo, clamp01, mask, init, float(w))
    return Z.detach(), share
