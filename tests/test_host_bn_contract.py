"""What esr_bn_reduce, esr_bn_apply and esr_bn_finalize_apply refuse (include/esr_hip.h: ESR_E_ARG / ESR_E_UNSUPPORTED), checked on the host
before anything is launched — so this file runs without a GPU as well as with one.

Every pointer addresses a real tensor (on the device when one is visible, on the host otherwise) that is large enough for the full, correct
launch, and the span check of tests/test_gpu_bn_contract.py holds for the unmodified descriptor: a view "with too few groups" DECLARES fewer
groups over its full-sized allocation, so a rejection that is missing cannot write outside memory the test owns.  Without a GPU a missing
rejection shows as another return code (the launch fails); with one, as ESR_OK.  The unmodified descriptor of every case is first shown not to
be refused, and after a refusal the outputs still hold their NaN fill."""
import ctypes as C

import pytest
import torch

import test_gpu_bn_contract as G

E_ARG, E_UNSUPPORTED = -1, -2
C_, N_GROUPS = 12, 2            # 12 channels: two channel groups, the second partial


def _set(path, value):
    """A mutation of the descriptor: path 'out0.ncg' <- value (callables get the current value)."""
    def f(d):
        obj, names = d, path.split('.')
        for nm in names[:-1]:
            obj = getattr(obj, nm)
        setattr(obj, names[-1], value(getattr(obj, names[-1])) if callable(value) else value)
    return f


class Setup:
    """The 'small' case of the contract file (B 4, groups 2, C 12, 6 x 10, bf16) with its outputs, and the three entry points on it."""

    def __init__(self, s2d, H=6, W=10):
        self.c = G.Case('bf16', 4, N_GROUPS, C_, H, W, s2d=s2d)
        self.lib = G._lib().load_library()

    def call(self, entry, mode, mutate=None, null_desc=False, sums=True, fin=None):
        c = self.c
        s0 = c.s2d and mode != 1
        o0 = c.new_output(s0) if entry != 'reduce' else None
        o1 = c.new_output(False) if entry == 'apply' and mode == 2 else None
        d = c.desc(dz=mode >= 1, u=mode == 2, out0=o0, out0_s2d=s0, out1=o1)
        if mutate:
            mutate(d)
        K = 3 if mode == 2 else 2
        tgt = torch.zeros(c.groups * c.C * K, dtype=torch.float64, device=G._dev())
        ref = None if null_desc else C.byref(d)
        if entry == 'reduce':
            rc = self.lib.esr_bn_reduce(ref, mode, tgt.data_ptr() if sums else None, G._stream())
        elif entry == 'apply':
            rc = self.lib.esr_bn_apply(ref, mode, G._stream())
        else:
            outs = G._fin_outputs(c.groups, c.C)
            s = G._y_sums(c).to(G._dev())
            gm, bt = G._f32(c.gamma), G._f32(c.beta)
            f = G._lib().CmdBnFinalize(s.data_ptr(), c.groups, c.C, c.N, G.EPS, G.MOM, gm.data_ptr(), bt.data_ptr(), outs['mean'].data_ptr(),
                                       outs['rstd'].data_ptr(), outs['scale'].data_ptr(), outs['shift'].data_ptr(), None, None)
            if fin:
                fin(f)
            rc = self.lib.esr_bn_finalize_apply(ref, C.byref(f), G._stream())
        G._sync()
        if rc in (E_ARG, E_UNSUPPORTED):
            for o in (o0, o1):
                assert o is None or bool((o.download() == G.NAN16).all()), 'a refused call wrote to an output'
            assert float(tgt.abs().max()) == 0
        return rc


_SETUPS = {}


def setup(s2d, H=6, W=10):
    key = (s2d, H, W)
    if key not in _SETUPS:
        _SETUPS[key] = Setup(s2d, H, W)
    return _SETUPS[key]


NEED_S2D = max(G.groups_of(2, True)) + 1        # 14: the space-to-depth view of two channel groups reaches group 13
BOTH = ('reduce', 'apply')
# (id, entries, modes, s2d, mutation, expected)
CASES = [
    ('null_y', BOTH, (0, 1, 2), False, _set('y.hi', None), E_ARG),
    ('B_not_a_multiple_of_groups', BOTH, (0,), False, _set('groups', 3), E_ARG),
    ('C_above_8_y_ncg', BOTH, (0, 1), False, _set('y.ncg', 1), E_ARG),
    ('mode_minus_1', BOTH, (-1,), False, None, E_ARG),
    ('mode_3', BOTH, (3,), False, None, E_ARG),
    ('missing_dz', BOTH, (1, 2), False, _set('dz.hi', None), E_ARG),
    ('missing_dz_s2d', BOTH, (1, 2), True, _set('dz.hi', None), E_ARG),
    ('missing_u', BOTH, (2,), False, _set('u.hi', None), E_ARG),
    ('missing_out0', ('apply',), (0, 1, 2), False, _set('out0.hi', None), E_ARG),
    ('missing_out0_s2d', ('apply',), (0, 1, 2), True, _set('out0.hi', None), E_ARG),
    ('missing_out1', ('apply',), (2,), False, _set('out1.hi', None), E_ARG),
    ('wrong_H_plain_out0', ('apply',), (0, 1, 2), False, _set('out0.H', lambda h: h - 1), E_ARG),
    ('wrong_W_plain_out0', ('apply',), (0, 1, 2), False, _set('out0.W', lambda w: w - 1), E_ARG),
    ('wrong_W_plain_dz', BOTH, (1, 2), False, _set('dz.W', lambda w: w - 1), E_ARG),
    ('wrong_H_plain_u', BOTH, (2,), False, _set('u.H', lambda h: h - 1), E_ARG),
    ('wrong_H_plain_out1', ('apply',), (2,), False, _set('out1.H', lambda h: h - 1), E_ARG),
    ('wrong_H_s2d_out0', ('apply',), (0, 2), True, _set('out0.H', lambda h: h - 1), E_ARG),
    ('wrong_W_s2d_out0', ('apply',), (0, 2), True, _set('out0.W', lambda w: w - 1), E_ARG),
    ('wrong_H_s2d_dz', BOTH, (1, 2), True, _set('dz.H', lambda h: h - 1), E_ARG),
    ('plain_out0_under_s2d_mode1', ('apply',), (1,), True, _set('out0.H', lambda h: h // 2), E_ARG),
    ('missing_mean', BOTH, (1, 2), False, _set('mean', None), E_ARG),
    ('missing_rstd', BOTH, (1, 2), False, _set('rstd', None), E_ARG),
    ('missing_sums2', ('apply',), (1, 2), False, _set('sums2', None), E_ARG),
    ('missing_sums3', ('apply',), (2,), False, _set('sums3', None), E_ARG),
    # the three rules this file was written with
    ('plain_out0_too_few_groups', ('apply',), (0, 1, 2), False, _set('out0.ncg', 1), E_ARG),
    ('plain_out0_too_few_groups_under_s2d', ('apply',), (1,), True, _set('out0.ncg', 1), E_ARG),
    ('plain_out1_too_few_groups', ('apply',), (2,), False, _set('out1.ncg', 1), E_ARG),
    ('plain_out1_too_few_groups_under_s2d', ('apply',), (2,), True, _set('out1.ncg', 1), E_ARG),
    ('plain_dz_too_few_groups', BOTH, (1, 2), False, _set('dz.ncg', 1), E_ARG),
    ('plain_u_too_few_groups', BOTH, (2,), False, _set('u.ncg', 1), E_ARG),
    ('plain_u_too_few_groups_under_s2d', BOTH, (2,), True, _set('u.ncg', 1), E_ARG),
    ('s2d_out0_one_group_short', ('apply',), (0, 2), True, _set('out0.ncg', NEED_S2D - 1), E_ARG),
    ('s2d_out0_four_groups_per_group', ('apply',), (0, 2), True, _set('out0.ncg', 8), E_ARG),         # 4 * ceil(C / 8): the former header's count
    ('s2d_dz_one_group_short', BOTH, (1, 2), True, _set('dz.ncg', NEED_S2D - 1), E_ARG),
    ('s2d_dz_four_groups_per_group', BOTH, (1, 2), True, _set('dz.ncg', 8), E_ARG),
    ('scale_null_without_const_stats', BOTH, (0, 1, 2), False, _set('scale', None), E_ARG),
    ('scale_null_without_const_stats_s2d', BOTH, (0, 1, 2), True, _set('scale', None), E_ARG),
]
FLAT = [(i, e, m, s, mut, exp) for i, es, ms, s, mut, exp in CASES for e in es for m in ms]


@pytest.mark.parametrize('entry,mode,s2d,mutate,expected', [t[1:] for t in FLAT], ids=['%s-%s%d' % t[:3] for t in FLAT])
def test_refused(entry, mode, s2d, mutate, expected):
    s = setup(s2d)
    if 0 <= mode <= 2:
        assert s.call(entry, mode) not in (E_ARG, E_UNSUPPORTED), 'the unmodified descriptor is refused'
    assert s.call(entry, mode, mutate) == expected


def test_null_descriptor_and_missing_sums():
    s = setup(False)
    for entry in ('reduce', 'apply', 'finalize_apply'):
        assert s.call(entry, 0, null_desc=True) == E_ARG, entry
    for mode in (0, 1, 2):
        assert s.call('reduce', mode, sums=False) == E_ARG, mode


@pytest.mark.parametrize('H,W', [(7, 10), (6, 9), (7, 9)])
def test_odd_size_with_s2d_is_unsupported(H, W):
    """A plain case of odd size whose descriptor then asks for space-to-depth: refused before any view is looked at."""
    s = setup(False, H, W)
    for entry, modes in (('reduce', (1, 2)), ('apply', (0, 1, 2)), ('finalize_apply', (0,))):
        for mode in modes:
            assert s.call(entry, mode) not in (E_ARG, E_UNSUPPORTED)
            assert s.call(entry, mode, _set('s2d', 1)) == E_UNSUPPORTED, (entry, mode)


FIN = [
    ('groups', False, None, _set('groups', 1)),
    ('C', False, None, _set('C', C_ - 1)),
    ('n_per_group', False, None, _set('n_per_group', lambda n: n + 1)),
    ('const_stats', False, _set('const_stats', 1), None),
    ('missing_sums', False, None, _set('sums', None)),
    ('missing_mean', False, None, _set('mean', None)),
    ('missing_out0', False, _set('out0.hi', None), None),
    ('wrong_H_out0', False, _set('out0.H', lambda h: h - 1), None),
    ('wrong_W_out0_s2d', True, _set('out0.W', lambda w: w - 1), None),
    ('plain_out0_too_few_groups', False, _set('out0.ncg', 1), None),
    ('s2d_out0_one_group_short', True, _set('out0.ncg', NEED_S2D - 1), None),
    ('s2d_out0_four_groups_per_group', True, _set('out0.ncg', 8), None),
]


@pytest.mark.parametrize('s2d,mutate,fin', [t[1:] for t in FIN], ids=[t[0] for t in FIN])
def test_finalize_apply_refused(s2d, mutate, fin):
    s = setup(s2d)
    assert s.call('finalize_apply', 0) not in (E_ARG, E_UNSUPPORTED), 'the unmodified descriptor is refused'
    assert s.call('finalize_apply', 0, mutate, fin=fin) == E_ARG


def test_finalize_apply_does_not_read_the_descriptors_affine():
    """d->scale / shift / mean / rstd are not read by esr_bn_finalize_apply (the header): NULL there is no reason to refuse."""
    def drop(d):
        d.scale = d.shift = d.mean = d.rstd = None
    assert setup(False).call('finalize_apply', 0, drop) not in (E_ARG, E_UNSUPPORTED)
