"""Device-side containers used by the launch planner: activation buffers in the kernels' channel-group layout
and packed conv weights.  PyTorch is only the allocator / stream provider here."""
import ctypes as C
import functools
import itertools
import math
import threading

import torch

from . import _lib
from ._image import detach_f32
from ._lib import ActView, EsrError, check


def require_gpu(t, what='tensor'):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise EsrError('%s must live on an AMD GPU: the RRDB/CEM kernels have no CPU fallback' % what)


_tls = threading.local()


def stream_ptr():
    """torch's current stream as the C-ABI's stream argument (inside a one_stream scope: the stream that was current at its start)."""
    s = getattr(_tls, 'stream', None)
    return s if s is not None else C.c_void_p(torch.cuda.current_stream().cuda_stream)


def one_stream(fn):
    """Decorator for a launch plan (hundreds of kernels, no stream switch inside): look torch's current stream up once instead of per
    launch (torch.cuda.current_stream() costs a few microseconds, comparable to a small kernel).  Per thread: autograd runs backward
    passes on its own thread."""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        if getattr(_tls, 'stream', None) is not None:
            return fn(*a, **kw)
        _tls.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        try:
            return fn(*a, **kw)
        finally:
            _tls.stream = None
    return wrapped


# ------------------------------------------------------------------------------------------------ launch lists (esr_run)
class Recorder:
    """Collects the launches of one pass instead of issuing them (esr_cmd, include/esr_hip.h): while a Recorder is active on this thread
    (`recording`), the wrappers below append their argument blocks to it.  finish() turns the collection into a Plan: ctypes arrays of
    esr_cmd that Plan.run replays with one esr_run call per segment.  `externals` {name: tensor} are the tensors whose addresses change
    from call to call (the pass's NCHW inputs / outputs): raw-pointer arguments that fall inside one of them are re-written before every
    replay; everything else a command points to (activation / gradient buffers, weight packs) must stay alive and in place for the
    plan's life — the caller keeps those objects with the plan (`keep`).  host(fn): work that is not a library launch (event records,
    torch ops) at this position of the sequence; it splits the list into segments and is called as fn(ctx) on replay."""

    def __init__(self, externals):
        self.ext = [(name, t.data_ptr(), t.numel() * t.element_size()) for name, t in externals.items()]
        self.items = []
        self.keep = []

    def emit(self, op, st, refs=()):
        if not self.items or self.items[-1][0] != 'cmds':
            self.items.append(('cmds', []))
        self.items[-1][1].append((op, st, refs))

    def host(self, fn):
        self.items.append(('host', fn))

    def position(self):
        """Where the next command will go: (item index, command index inside that item) — insert_host() takes it back."""
        if self.items and self.items[-1][0] == 'cmds':
            return (len(self.items) - 1, len(self.items[-1][1]))
        return (len(self.items), 0)

    def insert_host(self, pos, fn):
        """host(fn) at an EARLIER position() of the sequence (the segment it falls into is split).  Insert from the last position to the first:
        an insertion moves everything behind it."""
        k, j = pos
        if k >= len(self.items) or self.items[k][0] != 'cmds':
            self.items.insert(k, ('host', fn))
            return
        cmds = self.items[k][1]
        parts = ([('cmds', cmds[:j])] if j else []) + [('host', fn)] + ([('cmds', cmds[j:])] if j < len(cmds) else [])
        self.items[k:k + 1] = parts

    def _external_of(self, ptr):
        for name, base, nbytes in self.ext:
            if ptr is not None and base <= ptr < base + max(nbytes, 1):
                return name, ptr - base
        return None

    def append(self, other):
        """The items of `other` (a recording of the same pass over other images, same externals) joined to this one's, segment by segment:
        one lane that runs several sub-batches one after the other.  The host ops stay this recording's."""
        assert [k for k, _ in other.items] == [k for k, _ in self.items], 'sub-batches of one pass have the same segments'
        for (kind, mine), (_, theirs) in zip(self.items, other.items):
            if kind == 'cmds':
                mine.extend(theirs)
        self.keep.extend(other.keep)

    def finish(self):
        plan = Plan()
        plan.keep = self.keep
        for kind, payload in self.items:
            if kind == 'host':
                plan.items.append(payload)
                continue
            arr = (_lib.Cmd * len(payload))()
            for i, (op, st, refs) in enumerate(payload):
                arr[i].op = op
                C.memmove(C.addressof(arr[i].u), C.addressof(st), C.sizeof(st))
                member = getattr(arr[i].u, _lib.CMD_MEMBER[op])
                for field in refs:
                    hit = self._external_of(getattr(member, field))
                    if hit is not None:
                        plan.patches.append((member, field, hit[0], hit[1]))
            plan.items.append(arr)
            plan.n_cmds += len(payload)
        return plan


class Plan:
    """Recorded launch lists.  `side`: the plans of lanes 1.. of a pass recorded as independent lanes (with_lanes) — the same sequence of
    segments and host ops over other images; run() then replays every segment with one esr_run_lanes call, this plan's commands on the
    caller's stream and the side lanes' on the library's side streams, and calls this plan's host ops between the segments, on the caller's
    stream (behind one segment's join, in front of the next one's fork)."""

    def __init__(self):
        self.items, self.patches, self.keep, self.n_cmds = [], [], [], 0
        self.side = []
        self._failed, self._failed_lane = C.c_int(-1), C.c_int(-1)
        self._lane_args = None

    def with_lanes(self, side):
        for p in side:
            assert [callable(i) for i in p.items] == [callable(i) for i in self.items], 'lanes of one pass have the same segments'
        self.side = list(side)
        self._lane_args = {}
        for k, item in enumerate(self.items):
            if not callable(item):
                arrs = [item] + [p.items[k] for p in self.side]
                self._lane_args[k] = (arrs, (C.POINTER(_lib.Cmd) * len(arrs))(*[C.cast(a, C.POINTER(_lib.Cmd)) for a in arrs]),
                                      (C.c_int * len(arrs))(*[len(a) for a in arrs]))
        return self

    def run(self, externals, ctx=None):
        for plan in [self] + self.side:
            for member, field, name, off in plan.patches:
                setattr(member, field, externals[name].data_ptr() + off)
        s = stream_ptr()
        for k, item in enumerate(self.items):
            if callable(item):
                item(ctx)
                continue
            if self.side:
                arrs, ptrs, ns = self._lane_args[k]
                rc = _lib.lib.esr_run_lanes(ptrs, ns, len(arrs), C.byref(self._failed_lane), C.byref(self._failed), s)
                if rc != 0:
                    lane, i = self._failed_lane.value, self._failed.value
                    op = arrs[lane][i].op if 0 <= lane < len(arrs) and 0 <= i < len(arrs[lane]) else -1
                    check(rc, 'esr_run_lanes: lane %d, command %d (%s)' % (lane, i, _lib.CMD_MEMBER.get(op, '?')))
                continue
            rc = _lib.lib.esr_run(item, len(item), C.byref(self._failed), s)
            if rc != 0:
                op = item[self._failed.value].op if 0 <= self._failed.value < len(item) else -1
                check(rc, 'esr_run: command %d (%s)' % (self._failed.value, _lib.CMD_MEMBER.get(op, '?')))


class recording:
    """with recording(recorder): ... — the library wrappers of this module collect into `recorder` instead of launching."""

    def __init__(self, rec):
        self.rec = rec

    def __enter__(self):
        assert getattr(_tls, 'rec', None) is None, 'launch-list recording does not nest'
        _tls.rec = self.rec
        return self.rec

    def __exit__(self, *exc):
        _tls.rec = None


def _rec():
    return getattr(_tls, 'rec', None)


def host_op(fn):
    """Run fn(ctx) at this position of the launch sequence: now (ctx = None) when launching directly, on every replay when recording."""
    rec = _rec()
    if rec is None:
        fn(None)
    else:
        rec.host(fn)


# operand formats ("split" arguments throughout): True / 1 = bf16 hi+lo planes (fp32-class), False / 0 = bf16, 'f16' = one fp16 plane,
# 'f16x2' = fp16 hi+lo activation planes with single-plane fp16 weights, 'f16x3' = fp16 hi+lo activations AND weights
def fmt_code(split):
    """Weight-pack format code of include/esr_hip.h (0 bf16, 1 split bf16, 2 f16, 3 f16 hi+lo)."""
    if split == 'f16x3':
        return 3
    if split in ('f16', 'f16x2'):
        return 2
    return 1 if split else 0


def act_planes(split):
    """(number of activation planes, esr_act_view.fmt)"""
    if split == 'f16':
        return 1, 1
    if split in ('f16x2', 'f16x3', 'mixed'):
        return 2, 1
    return (2, 0) if split else (1, 0)


def hi_plane(v):
    """The same view without its lo plane (None stays None)."""
    if v is None:
        return None
    return ActView(v.hi, None, v.ncg, v.H, v.W, v.batch_stride, v.cg_stride, v.fmt)


class ActBuf:
    """[B][CG][H+2][W+2][8] bf16 `hi` (+ `lo`) planes.  Allocated zeroed, so the 1-pixel border the conv kernels
    rely on is zero from the start; producers never write it."""

    def __init__(self, B, ncg, H, W, device, split=True):
        self.B, self.ncg, self.H, self.W, self.split = B, ncg, H, W, split
        self.nplanes, self.fmt = act_planes(split)
        self.hi = torch.zeros(B, ncg, H + 2, W + 2, 8, dtype=torch.int16, device=device)
        self.lo = torch.zeros_like(self.hi) if self.nplanes == 2 else None
        self.cg_stride = (H + 2) * (W + 2)
        self.batch_stride = ncg * self.cg_stride
        self._views = {}

    def view(self, cg0=0, ncg=None, with_lo=True):
        """esr_act_view of groups [cg0, cg0+ncg).  with_lo=False: a producer shall write (a consumer shall see) the hi plane only.
        Memoised per buffer (treat views as immutable): a pass over the generator asks for the same few thousand views every step."""
        key = (cg0, ncg, with_lo)
        v = self._views.get(key)
        if v is None:
            n = self.ncg - cg0 if ncg is None else ncg
            assert 0 <= cg0 and cg0 + n <= self.ncg
            off = cg0 * self.cg_stride * 16
            v = self._views[key] = ActView(self.hi.data_ptr() + off, (self.lo.data_ptr() + off) if (self.nplanes == 2 and with_lo) else None,
                                           n, self.H, self.W, self.batch_stride, self.cg_stride, self.fmt)
        return v

    def nbytes(self):
        return self.hi.numel() * 2 * self.nplanes

    def to_nchw(self, nc, cg0=0):
        """Debug/test helper: unpack channels [cg0*8, cg0*8+nc) to fp32 NCHW."""
        out = torch.empty(self.B, nc, self.H, self.W, dtype=torch.float32, device=self.hi.device)
        v = self.view(cg0, (nc + 7) // 8)
        check(_lib.lib.esr_unpack_nchw(C.byref(v), self.B, nc, out.data_ptr(), stream_ptr()), 'esr_unpack_nchw')
        return out


class LaneBuf:
    """Images [b0, ..) of an ActBuf, for a pass over a sub-batch of the same buffer set: ActBuf's views with the base moved by
    b0 * batch_stride (a view has no batch size: the launch says how many images)."""

    def __init__(self, buf, b0):
        self.buf, self.off = buf, b0 * buf.batch_stride * 16
        self._views = {}

    def view(self, cg0=0, ncg=None, with_lo=True):
        key = (cg0, ncg, with_lo)
        v = self._views.get(key)
        if v is None:
            w = self.buf.view(cg0, ncg, with_lo)
            v = self._views[key] = ActView(w.hi + self.off, (w.lo + self.off) if w.lo else None, w.ncg, w.H, w.W, w.batch_stride, w.cg_stride, w.fmt)
        return v


NO_VIEW = ActView(None, None, 0, 0, 0, 0, 0, 0)


# activation tensors: the same layout as a torch tensor [planes][B][CG][H+2][W+2][8] bf16 (the critic and the VGG extractor)
def new_at(planes, B, ncg, H, W, device):
    """Uninitialised: for destinations whose producer writes the one-pixel zero border itself (pack_nchw, esr_bn_apply, the pools) or that are
    only ever read at interior pixels (conv outputs, data gradients)."""
    return torch.empty(planes, B, ncg, H + 2, W + 2, 8, dtype=torch.bfloat16, device=device)


def new_zeroed(planes, B, ncg, H, W, device):
    """With its zero border (and zero interior): conv outputs that become conv inputs; the conv kernels never write borders."""
    return torch.zeros(planes, B, ncg, H + 2, W + 2, 8, dtype=torch.bfloat16, device=device)


def view_of(t, cg0=0, ncg=None, b0=0):
    """View of channel groups [cg0, cg0 + ncg) starting at image b0 (the view has no batch size: the launch says how many images)."""
    if getattr(t, '_esr_stacked', False):              # [planes][CG][B][H+2][W+2][8]: see stacked_at()
        P, CG, B, Hp, Wp, _ = t.shape
        n = CG - cg0 if ncg is None else ncg
        cs = B * Hp * Wp
        hi = t.data_ptr() + (cg0 * cs + b0 * Hp * Wp) * 16
        return ActView(hi, hi + t.stride(0) * 2 if P == 2 else None, n, Hp - 2, Wp - 2, Hp * Wp, cs, 0)
    P, B, CG, Hp, Wp, _ = t.shape
    n = CG - cg0 if ncg is None else ncg
    cs = Hp * Wp
    off = (cg0 * cs + b0 * CG * cs) * 16
    hi = t.data_ptr() + off
    lo = hi + t.stride(0) * 2 if P == 2 else None
    return ActView(hi, lo, n, Hp - 2, Wp - 2, CG * cs, cs, 0)


def stacked_at(planes, B, ncg, H, W, device):
    """Group-major activation tensor [planes][CG][B][H+2][W+2][8] for SMALL feature maps: the B images of one channel group are stacked
    vertically, each with its own zero border rows, so that the whole batch is ONE image of B*(H+2) - 2 rows to a conv launch (tall_view):
    a tile then spans several images, and the layer's weights are fetched once per ~384 pixels instead of once per 16- or 64-pixel image.
    The rows between two images are their bottom / top borders: zero in every conv INPUT (the producers write them), garbage in conv
    OUTPUTS (which are only ever read at interior pixels)."""
    t = torch.empty(planes, ncg, B, H + 2, W + 2, 8, dtype=torch.bfloat16, device=device)
    t._esr_stacked = True
    return t


def tall_view(t, b0=0, nb=None):
    """Images [b0, b0 + nb) of the stacked tensor as one image per channel group (B' = 1): (view, rows)."""
    P, CG, B, Hp, Wp, _ = t.shape
    cs = B * Hp * Wp
    hi = t.data_ptr() + b0 * Hp * Wp * 16
    rows = (B - b0 if nb is None else nb) * Hp - 2
    return ActView(hi, hi + t.stride(0) * 2 if P == 2 else None, CG, rows, Wp - 2, cs * CG, cs, 0), rows


def pack_nchw(src, dst_view, c0, nc, pad=0, down=1, hw=None, batch_stride=0, channels=None):
    """fp32 NCHW (or a raw HR `view` of it: hw/batch_stride/channels given explicitly) -> act view."""
    require_gpu(src, 'input')
    assert src.dtype == torch.float32 and src.is_contiguous()
    B = src.shape[0]
    Cc = src.shape[1] if channels is None else channels
    h, w = (src.shape[2], src.shape[3]) if hw is None else hw
    rec = _rec()
    if rec is not None:
        rec.emit(_lib.OP_PACK_NCHW, _lib.CmdPackNchw(src.data_ptr(), batch_stride, B, Cc, h, w, c0, nc, pad, down, dst_view), ('src',))
        return
    check(_lib.lib.esr_pack_nchw(src.data_ptr(), batch_stride, B, Cc, h, w, c0, nc, pad, down, C.byref(dst_view), stream_ptr()),
          'esr_pack_nchw')


class _Pack:
    """What every weight pack is: an MFMA-fragment-ordered copy (`wpack`) of the weight tensor(s) weights() names, re-packed on demand when
    one of them changes (torch bumps `_version` on every in-place update, e.g. an optimizer step or load_state_dict), plus the `bias` the
    kernel reads.  get() is the stand-alone path; the engines' batched re-pack (PackBatch) is assembled from prepare / jobs / after_pack.
    A subclass says what differs: _build(dev), once (geometry, maps, destination, _bind_bias), and jobs()."""

    def __init__(self, split, transposed=False, bias=None):
        self.split, self.transposed, self.bias_p = split, transposed, bias
        self._key = self.wpack = self.bias = None
        self._built = self._bias_shared = False
        self._bias_rows = None

    def _fwd_bias(self):
        """The bias parameter the kernel adds: forward packs only (a data-gradient pack ignores it)."""
        return None if self.transposed else self.bias_p

    def weights(self):
        """The tensors the pack follows.  The bias too: without an epoch, PackBatch.run lets a pack with a shared bias re-read its address
        (after_pack) only when one of these moved."""
        bp = self._fwd_bias()
        return (self.weight,) if bp is None else (self.weight, bp)

    def key(self):
        return tuple((t.data_ptr(), t._version) for t in self.weights())

    def stale(self):
        return self.key() != self._key

    def prepare(self):
        if not self._built:
            w = self.weights()[0]
            require_gpu(w, 'conv weight')
            self._build(w.device)
            self._built = True
        return self

    def _bind_bias(self, n, dev, rows=None):
        """Bind a bias of n floats, `rows`: the parameter's elements in the order the launch wants them.  The kernel reads the parameter's own
        storage (always current) when that IS those n floats; a private zero-padded copy otherwise, refreshed by after_pack()."""
        bp = self._fwd_bias()
        self._bias_shared = bp is not None and rows is None and bp.dtype == torch.float32 and bp.is_contiguous() and bp.numel() == n
        self.bias = bp.detach() if self._bias_shared else torch.zeros(n, dtype=torch.float32, device=dev)
        if bp is not None and rows is not None:
            self._bias_rows = torch.tensor(rows, dtype=torch.long, device=dev)

    @property
    def needs_after_pack(self):
        """False when after_pack() has nothing to do besides staleness bookkeeping (the batched re-pack skips it then): no bias to copy —
        the kernel reads the parameter's own storage, whose address the engine's pointer epoch watches."""
        return self._fwd_bias() is not None and not self._bias_shared

    def after_pack(self):
        bp = self._fwd_bias()
        if self._bias_shared:
            if self.bias.data_ptr() != bp.data_ptr():
                self.bias = bp.detach()           # the parameter's storage was replaced
        elif bp is not None:
            b = bp.detach().float()
            if self._bias_rows is not None:
                b = b[self._bias_rows]
            self.bias[:b.numel()].copy_(b)
        self._key = self.key()

    def get(self):
        if self.stale():
            self.prepare()
            run_pack_jobs(self.jobs(), self.split)
            self.after_pack()
        return self


def _fp32(w):
    """w detached, as the pack kernels read it (fp32, contiguous): itself, or a converted copy the caller keeps alive until the pack has run."""
    wd = w.detach()
    return wd if wd.dtype == torch.float32 and wd.is_contiguous() else wd.float().contiguous()


class PackedConv(_Pack):
    """One nn.Conv2d(k=3) weight of up to 64 rows (+ its bias, zero-padded to whole M tiles)."""

    def __init__(self, weight, bias, lat, split=True, transposed=False, m_slice=None, rows=None, fold=None):
        super().__init__(split, transposed, bias)
        self.weight, self.lat = weight, lat
        # forward packs only: the first phase of a pack folded for a phase launch (esr_pack_conv_weights, ESR_PACK_FOLD2), None = plain
        self.fold = fold
        assert fold is None or not transposed
        self.m_slice = m_slice        # data-gradient packs: (lo, hi) slice of the main input channels, or 'latent'
        # explicit order of the tensor's OUTPUT channels (pixel-shuffle convs, see esr_conv3x3_desc.pixel_shuffle): forward packs take
        # them as the M rows of this launch, data-gradient packs as the K axis (the layout esr_pixel_unshuffle leaves the gradient in)
        self.rows = rows

    def _maps(self, dev):
        w = self.weight
        cout_w, cin_w = w.shape[0], w.shape[1]
        lat = self.lat
        main = cin_w - lat
        if not self.transposed:
            # K axis = input channels [lat | main]: the latent gets its own (zero padded) group so that the main
            # channels stay 8-aligned with the dense-block buffers
            kmap = []
            if lat:
                kmap += [e if e < lat else -1 for e in range(8)]
            ncg_main = (main + 7) // 8
            kmap += [lat + c if c < main else -1 for c in range(ncg_main * 8)]
            if self.rows is not None:
                mt = (len(self.rows) + 31) // 32
                mmap = list(self.rows) + [-1] * (mt * 32 - len(self.rows))
            else:
                mt = (cout_w + 31) // 32
                mmap = [m if m < cout_w else -1 for m in range(mt * 32)]
        else:
            # data-gradient: K axis = cout_w (upstream gradient channels), M axis = input channels laid out
            # [main groups | latent group]
            ncg_k = (cout_w + 7) // 8
            kmap = [c if c < cout_w else -1 for c in range(ncg_k * 8)]
            if self.rows is not None:
                assert len(self.rows) % 8 == 0
                kmap = list(self.rows)
            if self.m_slice == 'latent':
                mlist = list(range(lat))
            else:
                lo, hi = self.m_slice if self.m_slice is not None else (0, main)
                mlist = [lat + c for c in range(lo, hi)]
            mt = (len(mlist) + 31) // 32
            assert 1 <= mt <= 2, 'a data-gradient pack covers at most 64 output channels'
            mmap = mlist + [-1] * (mt * 32 - len(mlist))
        self.ncg_in = len(kmap) // 8
        self.mtiles = mt
        self.m_channels = len([m for m in mmap if m >= 0])
        return (torch.tensor(kmap, dtype=torch.int32, device=dev), torch.tensor(mmap, dtype=torch.int32, device=dev))

    def _build(self, dev):
        self.kmap, self.mmap = self._maps(dev)
        nbytes = _lib.lib.esr_conv_wpack_bytes(self.ncg_in, self.mtiles * 32, fmt_code(self.split))
        if self.wpack is None:
            self.wpack = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert self.wpack.numel() == nbytes      # a caller-supplied destination (one slice of a multi-slice pack)
        self._bind_bias(self.mtiles * 32, dev, self.rows)

    def jobs(self):
        """[(fp32 contiguous weight tensor, kmap, ncg_in, mmap, mtiles, transposed, scale, destination pointer)]"""
        self._wd = _fp32(self.weight)
        form = _lib.PACK_FOLD2 + self.fold if self.fold is not None else (1 if self.transposed else 0)
        return [(self._wd, self.kmap, self.ncg_in, self.mmap, self.mtiles, form, 1.0, self.wpack.data_ptr())]


class _PackedParts(_Pack):
    """A pack made of PackedConv `parts` (which carry no bias) back to back in ONE buffer, each part packing its own rows of `weight`."""

    def _build_parts(self, ncg_in, m, dev):
        """One buffer of len(parts) packs of (ncg_in K groups, m rows) each: slice s is part s's destination."""
        per = _lib.lib.esr_conv_wpack_bytes(ncg_in, m, fmt_code(self.split))
        self.wpack = torch.empty(len(self.parts) * per, dtype=torch.uint8, device=dev)
        for s, pk in enumerate(self.parts):
            pk.wpack = self.wpack[s * per:(s + 1) * per]
            pk.prepare()                          # (checks that its slice is as long as its pack)

    def jobs(self):
        return [j for pk in self.parts for j in pk.jobs()]


class PackedConvSlices(_PackedParts):
    """A conv weight as PackedConv slices of up to 64 rows, back to back in one buffer — the layout esr_conv3x3
    takes for more than 64 output channels (output slices of one launch, include/esr_hip.h).  Forward: one slice per 64 output channels (one
    slice of cout rows for cout <= 64); the bias is indexed by absolute channel.  transposed=True: the data-gradient pack (transposed + flipped,
    no bias), one slice per 64 INPUT channels.  `weight` is any fp32 tensor of a 3x3 conv's shape (the critic packs the 3x3 embedding of its
    4x4 weights)."""

    def __init__(self, weight, bias, lat=0, split=True, transposed=False):
        super().__init__(split, transposed, None if transposed else bias)
        self.weight, self.lat = weight, lat
        cout, cin = weight.shape[0], weight.shape[1]
        if transposed:
            assert lat == 0
            if cin > 64 and cin % 64:
                raise EsrError('conv weight %s: the data gradient needs up to 64 or a multiple of 64 input channels' % (tuple(weight.shape),))
            self.parts = [PackedConv(weight, None, 0, split=split, transposed=True, m_slice=(m0, min(cin, m0 + 64))) for m0 in range(0, cin, 64)]
        else:
            assert cout <= 64 or cout % 64 == 0
            self.parts = [PackedConv(weight, None, lat, split=split, rows=list(range(m0, min(cout, m0 + 64)))) for m0 in range(0, cout, 64)]

    def _build(self, dev):
        cout, cin = self.weight.shape[0], self.weight.shape[1]
        if self.transposed:
            self._build_parts((cout + 7) // 8, min(cin, 64), dev)
        else:
            self._build_parts((1 if self.lat else 0) + (cin - self.lat + 7) // 8, min(cout, 64), dev)
        self._bind_bias(cout, dev)


class PackedConvPhases(_PackedParts):
    """The forward weight of a conv behind a nearest x2 upsample, folded for the phase launch (esr_conv3x3_desc.upsample_phases = 2): per
    32-channel block c of the output two 64-row slices back to back — phases 0, 1 and phases 2, 3 of the block's rows, each M tile of a slice
    one phase (esr_pack_conv_weights, ESR_PACK_FOLD2).  The bias is indexed by channel and padded to whole blocks."""

    def __init__(self, weight, bias, split=True):
        super().__init__(split, False, bias)
        self.weight, self.lat, self.parts = weight, 0, []
        cout = weight.shape[0]
        for c in range((cout + 31) // 32):
            rows = [m if m < cout else -1 for m in range(32 * c, 32 * c + 32)]
            self.parts += [PackedConv(weight, None, 0, split=split, rows=rows + rows, fold=p0) for p0 in (0, 2)]

    def _build(self, dev):
        self._build_parts((self.weight.shape[1] + 7) // 8, 64, dev)
        self._bind_bias(32 * (len(self.parts) // 2), dev)


def run_pack_jobs(jobs, split):
    for wd, kmap, ncg_in, mmap, mtiles, transposed, scale, dst in jobs:
        check(_lib.lib.esr_pack_conv_weights(wd.data_ptr(), wd.shape[0], wd.shape[1], kmap.data_ptr(), ncg_in, mmap.data_ptr(), mtiles,
                                             transposed, fmt_code(split), float(scale), dst, stream_ptr()), 'esr_pack_conv_weights')


class PackBatch:
    """All weight packs of an engine re-packed by ONE launch (esr_pack_batch_*).  The descriptor table lives on the device and is
    re-uploaded only when a pointer changes, so a training step costs one kernel instead of ~1700 tiny ones."""

    def __init__(self):
        self.pack_ids, self.wptrs, self.ws, self.n, self.nblocks = None, None, None, 0, 0
        self.epoch, self.npacks, self.post = None, 0, []

    def run(self, packs, epoch=None):
        """Steady state of a training step (same packs, same weight storages, new values): one esr_pack_batch_run — the per-pack job lists are
        rebuilt only when a pack or a weight pointer changed.  `epoch`: the caller's token for "same pack objects, same parameter storages"
        (the engine's pointer epoch and pack-set counter); without it the pack ids and weight pointers are compared."""
        if epoch is not None:
            same = epoch == self.epoch and len(packs) == self.npacks and self.wptrs is not None
        else:
            ids = tuple(id(pk) for pk in packs)
            wptrs = tuple(w.data_ptr() for pk in packs for w in pk.weights())
            same = ids == self.pack_ids and wptrs == self.wptrs
        if not same:
            jobs = []
            for pk in packs:
                pk.prepare()
                jobs += [j + (fmt_code(pk.split),) for j in pk.jobs()]
            wptrs = tuple(w.data_ptr() for pk in packs for w in pk.weights())
            if any(j[0].dtype != torch.float32 or not j[0].is_contiguous() for j in jobs):
                wptrs = None            # a converted copy is packed: it must be refreshed every time, no fast path
            arr = (_lib.PackDesc * len(jobs))()
            for d, (wd, kmap, ncg_in, mmap, mtiles, transposed, scale, dst, code) in zip(arr, jobs):
                d.w, d.cout_w, d.cin_w = wd.data_ptr(), wd.shape[0], wd.shape[1]
                d.kmap, d.ncg_in, d.mmap, d.mtiles = kmap.data_ptr(), ncg_in, mmap.data_ptr(), mtiles
                d.transposed, d.split, d.scale, d.wpack = transposed, code, float(scale), dst
            need = _lib.lib.esr_pack_batch_workspace_bytes(arr, len(jobs))
            check(min(need, 0), 'esr_pack_batch_workspace_bytes')
            self.ws = torch.empty(int(need), dtype=torch.uint8, device=jobs[0][0].device)
            nb = _lib.lib.esr_pack_batch_upload(arr, len(jobs), self.ws.data_ptr(), self.ws.numel(), stream_ptr())
            check(min(nb, 0), 'esr_pack_batch_upload')
            self.n, self.nblocks = len(jobs), int(nb)
            self.pack_ids, self.wptrs, self.epoch, self.npacks = tuple(id(pk) for pk in packs), wptrs, epoch, len(packs)
            # packs with work of their own after the launch (a bias copy: permuted rows / a bias that is not the parameter itself)
            self.post = [pk for pk in packs if pk.needs_after_pack]
        check(_lib.lib.esr_pack_batch_run(self.ws.data_ptr(), self.n, self.nblocks, stream_ptr()), 'esr_pack_batch_run')
        for pk in (self.post if same else packs):      # after a rebuild every pack re-reads its parameter pointers (shared biases)
            pk.after_pack()


class PackedSum(_Pack):
    """Data-gradient pack whose K axis concatenates the output channels of SEVERAL conv layers: one launch then evaluates
    sum_i scale_i * conv_T(W_i)[rows] (dy_i) with the dy_i stored back to back in one gradient buffer — the backward of a dense
    block is itself a dense block (reference block.py:230-235 run backwards).  pieces: [(weight, scale)], K order = list order;
    rows: per piece, the indices into that weight's input-channel axis that form the M axis (same count for every piece)."""

    def __init__(self, pieces, rows, split=True):
        super().__init__(split, True)
        self.pieces, self.rows = pieces, rows

    def weights(self):
        return tuple(w for w, _ in self.pieces)

    def _build(self, dev):
        nrows = len(self.rows[0])
        mt = (nrows + 31) // 32
        self.mtiles, self.m_channels = mt, nrows
        self.maps, g = [], 0
        for (w, _), rows in zip(self.pieces, self.rows):
            assert w.shape[0] % 16 == 0 and len(rows) == nrows
            kmap = torch.arange(w.shape[0], dtype=torch.int32, device=dev)
            mmap = torch.tensor(list(rows) + [-1] * (mt * 32 - nrows), dtype=torch.int32, device=dev)
            self.maps.append((kmap, mmap, g))
            g += w.shape[0] // 8
        self.ncg_in = g
        self.wpack = torch.empty(_lib.lib.esr_conv_wpack_bytes(g, mt * 32, fmt_code(self.split)), dtype=torch.uint8, device=dev)
        self._bind_bias(mt * 32, dev)             # (no bias: the zero block)
        self.chunk_bytes = _lib.lib.esr_conv_wpack_bytes(2, mt * 32, fmt_code(self.split))

    def jobs(self):
        self._wd = [_fp32(w) for w, _ in self.pieces]       # keeps converted copies alive until the pack has run
        return [(wd, kmap, wd.shape[0] // 8, mmap, self.mtiles, 1, scale, self.wpack.data_ptr() + (g0 // 2) * self.chunk_bytes)
                for wd, (_, scale), (kmap, mmap, g0) in zip(self._wd, self.pieces, self.maps)]


_launch_parity = 0
LDS_STAGES = 0              # esr_conv3x3_desc.lds_stages of every launch built here: 0 = the library picks by launch size, 1 / 2 = that form


# ---- which inference forwards run as half-batch lanes on two streams (Plan.with_lanes, esr_run_lanes) ----
# A conv launch of T tiles over S = 2 * CUs resident workgroup slots ends in a part-empty round, and the next launch of the chain cannot
# start before its last tile is done; a second, independent chain over the other half of the images fills those tails and the launch ramps.
# Measured on the configs[1] forward in 'split' (32 x 148^2: 1920 tiles per dense-block launch, 3.75 rounds of 512 slots), fresh processes
# alternating, 20 steps each, ms per step (profiles/r08_lanes_ab.log):
#     whole batch 67.97 .. 68.08 | 2 x 16 images on two streams 66.38 .. 66.55 | 4 x 8 round-robin on two streams 66.03 .. 66.42
# 2 x 16 is the form taken: the same gain within the spread of 4 x 8 for half the launches (702 against 1404 per forward, which is what the
# host has to stay ahead of), and lanes of 960 tiles keep both workgroups of every CU busy while 8 images (480 tiles) do not.
#   * precisions not in the table stay single-lane: 'mixed' lost 20 % in the two-stream experiment of profiles/r04_exp_two_stream_lanes_ab.log
#     and was not measured again, the one-plane modes were never measured;
#   * a lane with fewer tiles than slots stays single-lane: such launches do not fill the device once, halving them only adds launches
#     (configs[2]'s 32 x 52^2, single images, configs[0]);
#   * beyond LANE_MAX_ROUNDS rounds per whole-batch launch nothing was measured (the measured launch has 3.75), and the part-empty round
#     that lanes fill is a smaller share of a longer launch: single-lane until somebody measures it.
LANE_TABLE = {'split': 2}
LANE_MAX_ROUNDS = 4


def forward_lane_count(precision, lane_tiles, cus):
    """Lanes (1: none) for an inference forward in `precision` whose dense-block launch would have `lane_tiles` tiles in its SMALLEST lane
    if it ran as LANE_TABLE[precision] lanes, on a device of `cus` compute units."""
    lanes = LANE_TABLE.get(precision, 1)
    slots = 2 * cus
    if lanes < 2 or lane_tiles < slots or lane_tiles * lanes > LANE_MAX_ROUNDS * slots:
        return 1
    return lanes


def dense_conv_tiles(H, W, planes):
    """Tiles per image of a dense-block conv launch (32 output channels) over H x W pixels, as the library cuts them (esr_conv3x3_tiling: a
    host-only query; the operand addresses are never read)."""
    d = _lib.Conv3x3Desc()
    d.in1 = ActView(16, 16 if planes == 2 else None, 8, H, W, 8 * (H + 2) * (W + 2), (H + 2) * (W + 2), 0)
    d.cout, d.B, d.H, d.W = 32, 1, H, W
    t = (C.c_int32 * 4)()
    check(_lib.lib.esr_conv3x3_tiling(C.byref(d), t), 'esr_conv3x3_tiling')
    return t[0] * t[1]


def lane_batches(B, lanes, subs=None):
    """[[(b0, nb), ...] per lane]: B images cut into `subs` sub-batches (default: one per lane) of sizes that differ by at most one, the larger
    first, dealt round-robin over the lanes."""
    subs = min(B, subs or lanes)
    out, b0 = [[] for _ in range(min(lanes, subs))], 0
    for j in range(subs):
        nb = B // subs + (1 if j < B % subs else 0)
        out[j % len(out)].append((b0, nb))
        b0 += nb
    return out


def reset_launch_parity():
    """Start of a pass: the alternating tile order restarts, so that a recorded pass and a directly launched one make the same choices."""
    global _launch_parity
    _launch_parity = 0


class RangeWatch:
    """fp16 range watch of one pass (esr_conv3x3_desc.range_flag / range_tag): one device word, initialised to -1 (0xFFFFFFFF), that every
    launch of the pass whose stored values reach 2^15 (or are not finite) lowers to its own tag = its index in `names`."""

    def __init__(self, device):
        self.flag = torch.full((1,), -1, dtype=torch.int32, device=device)
        self.names = []


_range_watch = None


class watching:
    """with watching(w): every conv3x3() launch issued (or recorded) inside carries w's flag word and the next tag."""

    def __init__(self, w):
        self.w = w

    def __enter__(self):
        global _range_watch
        self.prev, _range_watch = _range_watch, self.w
        return self.w

    def __exit__(self, *exc):
        global _range_watch
        _range_watch = self.prev


def conv3x3(pc, in1, B, H, W, cout, in0=None, upsample=1, act_slope=1.0, alpha=1.0, res1=None, beta1=0.0, res2=None, beta2=0.0,
            out=None, out2=None, out_nchw=None, use_bias=True, mask_src=None, mask_cg=(0, 0), mask_slope=0.2, reverse=None, in1_lo_groups=0,
            pixel_shuffle=0, ps_rowgroup0=0, tap_mask_k=None, tap_mask_k_shift=0, tap_mask_m=None, k_split_ws=None, name=None, upsample_phases=0):
    d = _lib.Conv3x3Desc()
    d.upsample_phases = upsample_phases       # 2: pc is a PackedConvPhases and H, W are the SOURCE size (esr_conv3x3_desc)
    if _range_watch is not None:
        d.range_flag, d.range_tag = _range_watch.flag.data_ptr(), len(_range_watch.names)
        _range_watch.names.append(name or 'conv %d' % len(_range_watch.names))
    d.in0 = in0 if in0 is not None else NO_VIEW
    d.in1 = in1
    d.upsample = upsample
    d.wpack = pc.wpack.data_ptr()
    d.bias = pc.bias.data_ptr() if use_bias else None
    d.cout = cout
    d.B, d.H, d.W = B, H, W
    d.act_slope, d.alpha = act_slope, alpha
    d.res1 = res1 if res1 is not None else NO_VIEW
    d.beta1 = beta1
    d.res2 = res2 if res2 is not None else NO_VIEW
    d.beta2 = beta2
    d.out = out if out is not None else NO_VIEW
    d.out2 = out2 if out2 is not None else NO_VIEW
    d.out_nchw = out_nchw.data_ptr() if out_nchw is not None else None
    d.mask_src = mask_src if mask_src is not None else NO_VIEW
    d.mask_cg0, d.mask_cg1 = mask_cg
    d.mask_slope = mask_slope
    # consecutive launches alternate the direction in which they walk the images (cache-reuse hint, see esr_conv3x3_desc)
    global _launch_parity
    if reverse is None:
        reverse = bool(_launch_parity & 1)
        _launch_parity += 1
    d.reverse_order = 1 if reverse else 0
    d.lds_stages = LDS_STAGES
    d.weight_planes = {0: 1, 1: 2, 2: 1, 3: 2}[fmt_code(pc.split)]
    d.in1_lo_groups = in1_lo_groups
    d.pixel_shuffle, d.ps_rowgroup0 = pixel_shuffle, ps_rowgroup0
    if tap_mask_k is not None:
        d.tap_mask_k[:] = tap_mask_k
        d.tap_mask_k_shift = tap_mask_k_shift
    if tap_mask_m is not None:
        d.tap_mask_m[:] = tap_mask_m
    if k_split_ws is not None:            # fp32 workspace the library may use to split the K axis of a small, deep launch (esr_hip.h)
        d.k_split_ws, d.k_split_ws_floats = k_split_ws.data_ptr(), k_split_ws.numel()
    rec = _rec()
    if rec is not None:
        rec.emit(_lib.OP_CONV3X3, d, ('out_nchw',))
        return
    check(_lib.lib.esr_conv3x3(C.byref(d), stream_ptr()), 'esr_conv3x3')


def pixel_unshuffle(src, r, dst, B):
    """dst[g*r^2 + s][y][x] = src[g][r*y + s//r][r*x + s%r]  (esr_pixel_unshuffle): adjoint of the conv kernel's pixel-shuffle store."""
    rec = _rec()
    if rec is not None:
        rec.emit(_lib.OP_PIXEL_UNSHUFFLE, _lib.CmdPixelUnshuffle(src, r, dst, B))
        return
    check(_lib.lib.esr_pixel_unshuffle(C.byref(src), r, C.byref(dst), B, stream_ptr()), 'esr_pixel_unshuffle')


def act_combine(out, B, A_=None, alpha=1.0, Bv=None, beta=1.0, s=1, mask=None, mask_slope=0.2):
    """out = alpha*A_ + beta*sumpool_s(Bv), optionally * LeakyReLU'(mask)  (esr_act_combine)."""
    rec = _rec()
    if rec is not None:
        nv = lambda v: v if v is not None else NO_VIEW
        rec.emit(_lib.OP_ACT_COMBINE, _lib.CmdActCombine(nv(A_), alpha, nv(Bv), beta, s, nv(mask), mask_slope, out, B))
        return
    ref = lambda v: C.byref(v) if v is not None else None
    check(_lib.lib.esr_act_combine(ref(A_), alpha, ref(Bv), beta, s, ref(mask), mask_slope, C.byref(out), B, stream_ptr()), 'esr_act_combine')


class GradScaler:
    """Running power-of-two scale of the fp16 gradients of one backward pass, kept on the device (esr_grad_absmax / esr_grad_scale).
    `current` is a 0-dim fp32 tensor (a slice of one small buffer): the scale the gradients in flight carry right now; every rescale()
    moves to the next slice, so tensors handed out earlier keep the value that was in force then."""

    def __init__(self, device, first, max_rescales=64):
        self.n = max_rescales
        self.slots = torch.zeros(self.n, dtype=torch.int32, device=device)
        self.scales = torch.ones(self.n + 1, dtype=torch.float32, device=device)
        self.scales[0:1].copy_(first.reshape(1))
        self.i = 0

    @property
    def current(self):
        return self.scales[self.i]

    def _ptr(self, t, i):
        return t.data_ptr() + 4 * i

    def rescale(self, B, views, exp):
        """Bring max|hi| of views[0] into [2^(exp-1), 2^exp), scale the other views by the same factor, advance `current`."""
        assert self.i < self.n
        slot = self._ptr(self.slots, self.i)
        rec = _rec()
        if rec is not None:
            rec.emit(_lib.OP_GRAD_ABSMAX, _lib.CmdGradAbsmax(views[0], B, slot))
            for j, v in enumerate(views):
                rec.emit(_lib.OP_GRAD_SCALE, _lib.CmdGradScale(v, v, B, slot, exp, self._ptr(self.scales, self.i), None,
                                                               self._ptr(self.scales, self.i + 1) if j == 0 else None))
            self.i += 1
            return
        check(_lib.lib.esr_grad_absmax(C.byref(views[0]), B, slot, stream_ptr()), 'esr_grad_absmax')
        for j, v in enumerate(views):
            check(_lib.lib.esr_grad_scale(C.byref(v), C.byref(v), B, slot, exp, self._ptr(self.scales, self.i), None,
                                          self._ptr(self.scales, self.i + 1) if j == 0 else None, stream_ptr()), 'esr_grad_scale')
        self.i += 1

    def rescaled_copy(self, B, src, dst, scale_then):
        """dst = src * (current / scale_then): bring a buffer produced under an earlier scale to the current one."""
        rec = _rec()
        if rec is not None:
            rec.emit(_lib.OP_GRAD_SCALE, _lib.CmdGradScale(src, dst, B, None, 0, self._ptr(self.scales, self.i), scale_then.data_ptr(), None))
            return
        check(_lib.lib.esr_grad_scale(C.byref(src), C.byref(dst), B, None, 0, self._ptr(self.scales, self.i), scale_then.data_ptr(), None,
                                      stream_ptr()), 'esr_grad_scale')


def unpack_grad_nchw(G, dst, C_, h, w, c0, nc, pad=0, down=1, accumulate=False, batch_stride=0):
    """Adjoint of pack_nchw: act-layout gradient G -> channels [c0, c0+nc) of the fp32 gradient `dst` of an un-padded source
    laid out [B][C_][h][w] (image b at dst + b*batch_stride floats; 0 = C_*h*w)."""
    require_gpu(dst, 'gradient')
    assert dst.dtype == torch.float32 and dst.is_contiguous()
    rec = _rec()
    if rec is not None:
        rec.emit(_lib.OP_UNPACK_GRAD_NCHW, _lib.CmdUnpackGradNchw(G, dst.data_ptr(), batch_stride, dst.shape[0], C_, h, w, c0, nc, pad, down,
                                                                  1 if accumulate else 0), ('dst',))
        return
    check(_lib.lib.esr_unpack_grad_nchw(C.byref(G), dst.data_ptr(), batch_stride, dst.shape[0], C_, h, w, c0, nc, pad, down,
                                        1 if accumulate else 0, stream_ptr()), 'esr_unpack_grad_nchw')


def conv3x3_nchw_parts(parts, in1, B, H, W, out, **kw):
    """The fp32 NCHW tensor `out` from packs of up to 64 rows each, which together hold its channels in order: one conv3x3() launch per
    pack (the kernel produces up to 64 channels per launch, and output slices of ONE launch exist for the activation layout only), each
    but a lone one into a tensor of its own, copied into place."""
    m0 = 0
    for pc in parts:
        mc = pc.m_channels
        tmp = out if mc == out.shape[1] else torch.empty(B, mc, H, W, dtype=torch.float32, device=out.device)
        conv3x3(pc, in1, B, H, W, mc, out_nchw=tmp, **kw)
        if tmp is not out:
            out[:, m0:m0 + mc] = tmp
        m0 += mc
    return out


def conv3x3_nchw(x, weight, bias, act_slope=1.0, split=True):
    """Stand-alone conv3x3 on fp32 NCHW tensors (pack -> MFMA conv -> fp32 NCHW).  Used by block-level calls and tests; the
    whole-generator path keeps activations in the kernels' layout instead (engine.py)."""
    require_gpu(x, 'conv input')
    x = x.detach()
    x = (x if x.dtype == torch.float32 else x.float()).contiguous()
    B, Cin, H, W = x.shape
    cout = weight.shape[0]
    assert weight.shape[1] == Cin
    ncg = (Cin + 7) // 8
    src = ActBuf(B, ncg, H, W, x.device, split)
    pack_nchw(x, src.view(), 0, Cin)
    # any cout: contiguous copies of 64-row slices of the weight and the bias, the last one as short as it comes (a PackedConvSlices takes
    # whole slices only); up to 64 channels the slice is the tensor itself
    parts = [PackedConv(weight.detach()[m0:m0 + 64].contiguous(), None if bias is None else bias.detach()[m0:m0 + 64].contiguous(), 0, split=split).get()
             for m0 in range(0, cout, 64)]
    return conv3x3_nchw_parts(parts, src.view(), B, H, W, torch.empty(B, cout, H, W, dtype=torch.float32, device=x.device), act_slope=act_slope)


def conv3x3_dgrad_nchw(dy, weight, split=True):
    """Data gradient of a stand-alone conv3x3 on fp32 NCHW tensors: dx = conv_T(dy) (weights transposed + flipped)."""
    require_gpu(dy, 'gradient')
    dy = dy.detach()
    dy = (dy if dy.dtype == torch.float32 else dy.float()).contiguous()
    B, Cout, H, W = dy.shape
    cin = weight.shape[1]
    assert weight.shape[0] == Cout
    src = ActBuf(B, (Cout + 7) // 8, H, W, dy.device, split)
    pack_nchw(dy, src.view(), 0, Cout)
    parts = [PackedConv(weight, None, 0, split=split, transposed=True, m_slice=(lo, min(cin, lo + 64))).get() for lo in range(0, cin, 64)]
    return conv3x3_nchw_parts(parts, src.view(), B, H, W, torch.empty(B, cin, H, W, dtype=torch.float32, device=dy.device), use_bias=False)


def wgrad_desc(dy, x_main, x_lat, lat, wshape, B, H, W, alpha, upsample, device, out=None, tap_masks=None):
    """esr_wgrad_desc for one conv layer plus its zeroed outputs: returns (desc, dW [cout][cin][3][3], db [cout]).
    out = (dW, db): zeroed tensors to accumulate into (e.g. views of one flat buffer) instead of allocating two per layer."""
    cout, cin = wshape[0], wshape[1]
    if out is None:
        dw = torch.zeros(cout, cin, 3, 3, dtype=torch.float32, device=device)
        db = torch.zeros(cout, dtype=torch.float32, device=device)
    else:
        dw, db = out
    nlat = lat if x_lat is not None else 0
    d = _lib.WgradDesc()
    d.dy, d.x = dy, x_main
    d.xlat = x_lat if x_lat is not None else NO_VIEW
    d.lat, d.upsample = nlat, upsample
    d.cout, d.cin_main = cout, cin - nlat
    d.B, d.H, d.W = B, H, W
    d.alpha = alpha
    d.dw, d.db = dw.data_ptr(), db.data_ptr()
    if tap_masks is not None:
        d.tap_masks[:] = tap_masks
    return d, dw, db


def conv3x3_wgrad(dy, x_main, x_lat, lat, wshape, B, H, W, alpha, upsample, device, tap_masks=None):
    """Weight + bias gradient of one conv layer from act-layout operands (esr_conv3x3_wgrad): returns (dW [cout][cin][3][3], db [cout])."""
    d, dw, db = wgrad_desc(dy, x_main, x_lat, lat, wshape, B, H, W, alpha, upsample, device, tap_masks=tap_masks)
    need = _lib.lib.esr_conv3x3_wgrad_workspace_floats(C.byref(d))
    check(min(need, 0), 'esr_conv3x3_wgrad_workspace_floats')
    ws = _wgrad_workspace(device, need)
    d.workspace, d.workspace_floats = ws.data_ptr(), ws.numel()
    check(_lib.lib.esr_conv3x3_wgrad(C.byref(d), stream_ptr()), 'esr_conv3x3_wgrad')
    return dw, db


class WgradTable:
    """One descriptor array on the device for the batched weight-gradient launch (esr_conv3x3_wgrad_batch_upload; _part_upload when unit > 0:
    the array is one PART of a larger set, every layer's pixel sum sliced as in the one-launch form — unit = wgrad_batch_unit of the whole set —
    so the results are bit-identical to it).  The caller keeps every dy / x buffer alive and unmodified until a launch has run.  ptr: the
    flat-buffer address the descriptors' dW / db pointers were built against (follow())."""

    def __init__(self, descs, device, unit=0, ptr=0):
        self.arr, self.unit, self.ptr, n = (_lib.WgradDesc * len(descs))(*descs), unit, ptr, len(descs)
        need = _lib.lib.esr_conv3x3_wgrad_batch_part_workspace_bytes(self.arr, n, unit) if unit else _lib.lib.esr_conv3x3_wgrad_batch_workspace_bytes(self.arr, n)
        check(min(need, 0), 'esr_conv3x3_wgrad_batch_workspace_bytes')
        self.ws, self.plan = torch.empty(int(need), dtype=torch.uint8, device=device), _lib.WgradBatchPlan()
        args = (self.arr, n, self.ws.data_ptr(), self.ws.numel(), C.byref(self.plan))
        if unit:
            check(_lib.lib.esr_conv3x3_wgrad_batch_part_upload(*args, unit, stream_ptr()), 'esr_conv3x3_wgrad_batch_part_upload')
        else:
            check(_lib.lib.esr_conv3x3_wgrad_batch_upload(*args, stream_ptr()), 'esr_conv3x3_wgrad_batch_upload')

    def follow(self, ptr):
        """The flat gradient buffer now lives at ptr: the table's dW / db pointers move with it, on the device (stream-ordered, no host copy) —
        and only if it moved."""
        if ptr != self.ptr:
            check(_lib.lib.esr_conv3x3_wgrad_batch_rebase(self.ws.data_ptr(), C.byref(self.plan), ptr - self.ptr, stream_ptr()), 'esr_conv3x3_wgrad_batch_rebase')
            self.ptr = ptr

    def run(self):
        check(_lib.lib.esr_conv3x3_wgrad_batch_run(self.ws.data_ptr(), C.byref(self.plan), stream_ptr()), 'esr_conv3x3_wgrad_batch_run')

    def run_side(self, stream):
        check(_lib.lib.esr_conv3x3_wgrad_batch_run_side(self.ws.data_ptr(), C.byref(self.plan), stream.cuda_stream), 'esr_conv3x3_wgrad_batch_run_side')

    def emit(self, rec):
        """The launch as a command of a recorded list, which keeps the workspace alive."""
        rec.emit(_lib.OP_WGRAD_BATCH_RUN, _lib.CmdWgradBatchRun(self.ws.data_ptr(), self.plan))
        rec.keep.append(self.ws)


_WGB = {}        # fallback cache for callers without an engine: {device index: [(descriptor bytes, WgradTable), ...]}
_WGB_KEEP = 4    # descriptor sets kept per cache (a dual pass / gradient accumulation alternates between a few)


def conv3x3_wgrad_batch(descs, device, cache=None, unit=0):
    """All recorded layers' weight gradients in one launch (WgradTable).  The descriptor table is uploaded only when it differs from the ones
    already on the device: with pooled gradient buffers and the allocator handing back the same dW storage, a steady-state training step re-runs
    a table that is already there (no host->device copy).  `cache`: the owner's dict (one per engine, so that two models — or two streams —
    never share a table a launch in flight may still be reading); each distinct descriptor set gets its OWN workspace, a small LRU of them is
    kept.  unit: see WgradTable."""
    if not descs:
        return
    arr = (_lib.WgradDesc * len(descs))(*descs)
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    raw = bytes(arr) + unit.to_bytes(8, 'little')
    entries = (_WGB if cache is None else cache).setdefault(key, [])
    hit = next((e for e in entries if e[0] == raw), None)
    if hit is None:
        hit = (raw, WgradTable(arr, device, unit))
        entries.insert(0, hit)
        del entries[_WGB_KEEP:]
    elif entries[0] is not hit:
        entries.remove(hit)
        entries.insert(0, hit)
    hit[1].run()


def wgrad_batch_unit(descs):
    """The slicing granule of the one-launch form for this whole set of layers (esr_conv3x3_wgrad_batch_unit)."""
    arr = (_lib.WgradDesc * len(descs))(*descs)
    unit = _lib.lib.esr_conv3x3_wgrad_batch_unit(arr, len(descs))
    check(min(unit, 0), 'esr_conv3x3_wgrad_batch_unit')
    return int(unit)


class FlatGrads:
    """The weight and bias gradients of a list of conv layers in ONE fp32 buffer, layer after layer: dW [cout][cin][kh][kw], then db [cout]."""

    def __init__(self, wshapes, device):
        self.wshapes, self.device = [tuple(s) for s in wshapes], device
        self.sizes = [k for s in self.wshapes for k in (math.prod(s), s[0])]
        ends = list(itertools.accumulate(self.sizes))
        self.offsets, self.n = [0] + ends[1:-1:2], ends[-1]

    def bounds(self):
        """[(start, end)] of every layer in the buffer."""
        return list(zip(self.offsets, self.offsets[1:] + [self.n]))

    def zeros(self):
        return torch.zeros(self.n, dtype=torch.float32, device=self.device)

    def views(self, flat):
        """[(dW, db)] of every layer: views of flat."""
        parts = flat.split(self.sizes)
        return [(parts[2 * k].view(s), parts[2 * k + 1]) for k, s in enumerate(self.wshapes)]


_WS = {}


def _wgrad_workspace(device, nfloats):
    """One grow-only scratch tensor per device: the weight-gradient launches of a backward pass run back to back on one stream,
    so they can share it."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    ws = _WS.get(key)
    if ws is None or ws.numel() < nfloats:
        ws = torch.empty(max(int(nfloats), 1 << 20), dtype=torch.float32, device=device)
        _WS[key] = ws
    return ws


def conv3x3_wgrad_nchw(dy, x, wshape, split=True):
    """Weight / bias gradient of a stand-alone conv3x3 from fp32 NCHW tensors."""
    require_gpu(dy, 'gradient')
    dy = (dy.detach().float()).contiguous()
    x = (x.detach().float()).contiguous()
    B, Cout, H, W = dy.shape
    Cin = x.shape[1]
    gy = ActBuf(B, (Cout + 7) // 8, H, W, dy.device, split)
    gx = ActBuf(B, (Cin + 7) // 8, H, W, dy.device, split)
    pack_nchw(dy, gy.view(), 0, Cout)
    pack_nchw(x, gx.view(), 0, Cin)
    return conv3x3_wgrad(gy.view(), gx.view(), None, 0, wshape, B, H, W, 1.0, 1, dy.device)


# ------------------------------------------------------------------------------------------------ frozen conv engines (vgg.py, dncnn.py)
# An engine has forward(x, save) -> (output, saved | None) and backward(saved, d_output) -> d_x; its weights are frozen.
def launch_by_launch(name):
    """guard of an engine's passes, which issue their launches directly"""
    if _rec() is not None:
        raise EsrError('the %s passes are issued launch by launch; they cannot be collected into a launch list' % name)


def gpu_input(x, what):
    """what an engine's kernels read: x on the GPU, detached, float32, contiguous"""
    require_gpu(x, what)
    return detach_f32(x)


class _InputGradFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, name, x):
        out, saved = eng.forward(x, save=True)
        ctx.eng, ctx.name, ctx.saved = eng, name, saved
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        saved, ctx.saved = ctx.saved, None
        if saved is None:
            raise EsrError('%s backward: the saved activations were already released (backward called twice?)' % ctx.name)
        return None, None, ctx.eng.backward(saved, d_out)


def engine_forward(eng, name, x):
    """The engine's output for x; differentiable w.r.t. x when x requires grad and grad mode is on (input gradient only)."""
    if torch.is_grad_enabled() and x.requires_grad:
        return _InputGradFn.apply(eng, name, x)
    with torch.no_grad():
        return eng.forward(x, save=False)[0]
