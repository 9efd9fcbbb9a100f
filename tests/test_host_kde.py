"""CPU tests of the patch-histogram / dictionary objectives' host side (reference codes/Z_optimization.py:24-272, :510-543): the NumPy patch
selection against the index lists the reference's ReturnPatchExtractionMat produced (fixture tests/golden/patch_kde.npz, written by
tools/gen_patch_kde_golden.py), the objective-name parsing, and the refusals of what this build does not implement."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'patch_kde.npz')


@pytest.mark.parametrize('mask', ['full', 'irr'])
@pytest.mark.parametrize('overlap_name,overlap', [('half', 0.5), ('desired', 30 / 36)])
def test_patch_selection_equals_the_references(mask, overlap_name, overlap):
    from esr_hip import kde
    g = np.load(GOLDEN)
    got = kde.patch_extraction_indexes(g['mask/' + mask], 6, overlap)
    want = g['sel/%s_%s' % (mask, overlap_name)]
    assert got.dtype == np.int64 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)


def test_patch_selection_without_overlap_limit_is_every_window_of_the_opened_mask():
    from esr_hip import kde
    m = np.zeros((12, 13), np.float32)
    m[1:9, 2:12] = 1
    m[10, 0] = 1                                      # an isolated pixel: removed by the opening
    idx = kde.patch_extraction_indexes(m, 3, 1.0)
    assert idx.shape == ((8 - 2) * (10 - 2), 9)
    assert idx[0].tolist() == [1 * 13 + 2, 1 * 13 + 3, 1 * 13 + 4, 2 * 13 + 2, 2 * 13 + 3, 2 * 13 + 4, 3 * 13 + 2, 3 * 13 + 3, 3 * 13 + 4]
    opened = kde.binary_opening_square(m, 3)
    assert opened.sum() == 8 * 10 and not opened[10, 0]


def test_the_product_path_imports_neither_scipy_nor_sklearn():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ('import sys; sys.path[:0] = [%r, %r]; import Z_optimization, esr_hip.kde; '
            'assert not [m for m in sys.modules if m.split(".")[0] in ("scipy", "sklearn")], sorted(sys.modules)') % (
        root, os.path.join(root, 'explorable-super-resolution_amd'))
    subprocess.check_call([sys.executable, '-c', code])


@pytest.mark.parametrize('objective,patch,T,dictionary,no_dc', [
    ('patchhist', 6, 5e-4, False, False), ('patchhist_noDC', 6, 5e-4, False, True), ('dict', 1, 1e-3, True, False),
    ('dict_noDC', 1, 1e-3, True, True), ('patchdict', 6, 1e-3, True, False), ('patchdict_noDC', 6, 1e-3, True, True)])
def test_objective_names_parse_to_the_references_settings(objective, patch, T, dictionary, no_dc):
    from Z_optimization import HIST_OBJECTIVES, Z_optimizer, hist_objective_config
    cfg = hist_objective_config(objective)
    assert objective in HIST_OBJECTIVES and objective in Z_optimizer.SUPPORTED
    assert cfg == dict(bins=256, min=0, max=1, patch_size=patch, temperature=T, dictionary_not_histogram=dictionary, no_patch_DC=no_dc)


@pytest.mark.parametrize('objective', ['patchhist_noDC_no_localSTD', 'patchdict_noDC_no_localSTD', 'patchhist_localSTD'])
def test_local_std_variants_are_refused_by_name(objective):
    from Z_optimization import Z_optimizer
    with pytest.raises(NotImplementedError, match='localSTD'):
        Z_optimizer(objective, [8, 8], model=None, Z_range=1, max_iters=1, initial_LR=0.1)


def test_automatic_temperature_is_refused_by_the_objective():
    from Z_optimization import Z_optimizer
    with pytest.raises(NotImplementedError, match='auto_set_hist_temperature'):
        Z_optimizer('patchhist', [8, 8], model=None, Z_range=1, max_iters=1, initial_LR=0.1, auto_set_hist_temperature=True)


@pytest.mark.parametrize('kw,word', [(dict(automatic_temperature=True), 'automatic_temperature'), (dict(no_patch_STD=True, no_patch_DC=True), 'no_patch_STD'),
                                     (dict(gray_scale=False), 'colour')])
def test_soft_histogram_loss_refuses_by_name(kw, word):
    from Z_optimization import SoftHistogramLoss
    args = dict(bins=256, min=0, max=1, desired_hist_image=[torch.rand(1, 3, 16, 16)], desired_hist_image_mask=[None], patch_size=6, temperature=5e-4)
    args.update(kw)
    with pytest.raises(NotImplementedError, match=word):
        SoftHistogramLoss(**args)
