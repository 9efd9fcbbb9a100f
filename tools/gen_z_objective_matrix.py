#!/usr/bin/env python
"""TEST INFRASTRUCTURE ONLY (CPU): writes tests/golden/z_objective_matrix.json, what Z_optimizer's constructor answers over the cross product of
    objective    every name of Z_optimizer.SUPPORTED plus the refused spellings of REFUSED
    model        'sr' (the toy generator of tests/test_host_api.py), 'jpeg_y' and 'jpeg_colour' (the five-layer DnCNN models of
                 tests/test_host_jpeg.py and tests/test_host_jpeg_chroma.py), each holding the output of a seeded Z for a batch of two
    HR_unpadder  absent, given
    masks        none, all ones, partial (whole 8 x 8 blocks in JPEG mode, the Z mask its block maximum)
    non_local_Z_optimization   off, on
    data         complete for the name (REQUIRED), or with each of its keys removed in turn
per case either 'ok' or '<exception type>: <message>', the first refusal where a call is wrong in two ways.  Only the public constructor is
used, so the same script records any commit's answers: the committed file was written at the commit before the objectives became entries of
Z_objectives.py's table OBJECTIVES, and tests/test_host_z_objective_matrix.py regenerates it in process and requires equality case by case.  Run:
    python tools/gen_z_objective_matrix.py

File layout: {'outcomes': [distinct answers], 'cases': {objective: {'model/unpadder/masks/non_local/data': index into outcomes}}}."""
import itertools
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'explorable-super-resolution_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle.weights import seeded_uniform  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'z_objective_matrix.json')
REFUSED = ('random_VGG_limited', 'random_l1_local', 'random_l1_limited_local', 'local_TV', 'local_l1', 'periodicityPlus', 'periodicityPlus_1D',
           'local_STD_periodicityPlus_1D', 'STD_increasePlus', 'local_Mag_max', 'local_STD_Mag_increase', 'nonInt_periodicityPlus_2D',
           'patchhist_localSTD', 'hist_no_localSTD', 'digit', 'max_l1', 'no_such_objective')
KINDS = ('sr', 'jpeg_y', 'jpeg_colour')
MASKS = ('none', 'ones', 'partial')
BATCH = 2


def required(name):
    """the data keys a name's family reads (beyond the model's own input); STD_increment is optional for the STD_increase / decrease names and
    listed all the same, so that both of their branches are covered"""
    keys = []
    if name in ('l1', 'VGG', 'max_VGG', 'hist', 'scribble') or name.startswith(('patch', 'dict')):
        keys.append('desired')
    if name == 'scribble':
        keys += ['scribble_mask', 'brightness_factor']
    if 'periodicity' in name:
        keys.append('periodicity_points')
    if 'Plus' in name or 'Mag' in name or 'increase' in name or 'decrease' in name:
        keys.append('STD_increment')
    if 'limited' in name:
        keys.append('rmse_weight')
    return keys


class Model:
    """one model kind with a current output: the model, its image size, Z grid, input data, masks and constructor keywords"""

    def __init__(self, kind, tmp):
        self.kind = kind
        if kind == 'sr':
            from test_host_api import _ToyModel
            self.model = _ToyModel()
            self.model.netF = lambda im: 4.0 * im                       # a stand-in feature extractor, as tests/test_host_random_z.py's
            self.H, self.W, self.Z_size, z_channels = 16, 16, [16, 16], 1
            self.input = {'LR': seeded_uniform((1, 3, 4, 4), 9500)}
            self.partial = np.zeros((16, 16), np.float32)
            self.partial[2:14, 3:13] = 1
            self.partial_Z = self.partial
            labels = ((slice(4, 8), slice(3, 8), 1), (slice(8, 12), slice(3, 8), 2), (slice(4, 12), slice(8, 11), 4), (slice(4, 12), slice(11, 13), 5))
            self.kw = {}
        else:
            import test_host_jpeg
            import test_host_jpeg_chroma
            os.makedirs(os.path.join(tmp, kind))
            from pathlib import Path
            colour = kind == 'jpeg_colour'
            self.model = (test_host_jpeg_chroma if colour else test_host_jpeg).make_model(Path(tmp) / kind)
            self.H, self.W, self.Z_size, z_channels = 32, 48, [4, 6], 64
            x = test_host_jpeg_chroma.C.image_c()[:1, :, :32, :48] if colour else test_host_jpeg.G.image_b()[:1, :, :32, :48]
            self.input = {'Uncomp': x.contiguous(), 'QF': torch.tensor([40.0])}
            self.partial = np.zeros((32, 48), np.float32)
            self.partial[8:24, 8:32] = 1
            self.partial_Z = self.partial.reshape(4, 8, 6, 8).max((1, 3))
            labels = ((slice(8, 16), slice(8, 24), 1), (slice(16, 24), slice(8, 16), 2), (slice(16, 24), slice(24, 32), 5))
            self.kw = {'jpeg_extractor': self.model.JPEG['extractor']}
        self.scribble_mask = np.zeros((self.H, self.W), np.int64)
        for rows, cols, label in labels:
            self.scribble_mask[rows, cols] = label
        shape = [BATCH, z_channels] + self.Z_size
        self.Z0 = seeded_uniform(shape, 9501, -0.5, 0.5)
        self.initial_Z = self.Z0 + seeded_uniform(shape, 9502, -0.05, 0.05)  # the search starts next to the model's output, not on it
        self.reset()

    def reset(self):
        """the model's current output: that of Z0 (the constructor under test reads it and leaves it alone; a search replaces it)"""
        self.model.feed_data(dict({k: v.expand(BATCH, *([-1] * (v.dim() - 1))) for k, v in self.input.items()}, Z=self.Z0), need_GT=False)
        self.model.test()
        if self.kind == 'sr':
            self.model.output_image = 1 * self.model.fake_H.detach()

    def data(self, name, without=None):
        desired = seeded_uniform((1, 3, self.H, self.W), 9503, 0.2, 0.8)
        d = dict(self.input, desired=[desired[0]] if name == 'hist' else desired, scribble_mask=self.scribble_mask, brightness_factor=0.2,
                 periodicity_points=[[2.5, 1.25]] if 'nonInt' in name else [[3, 2]], STD_increment=0.03, rmse_weight=0.5)
        keep = set(self.input) | set(required(name) if name not in REFUSED else d)
        return {k: v for k, v in d.items() if k in keep and k != without}

    def masks(self, which):
        if which == 'none':
            return {}
        if which == 'ones':
            return {'image_mask': np.ones((self.H, self.W), np.float32), 'Z_mask': np.ones(self.Z_size, np.float32)}
        return {'image_mask': self.partial.copy(), 'Z_mask': self.partial_Z.copy()}


def names(Z):
    return list(Z.Z_optimizer.SUPPORTED) + list(REFUSED)


def cases(Z):
    """(objective, model kind, HR_unpadder given, masks, non_local_Z_optimization, removed data key or None)"""
    for name in names(Z):
        removed = [None] + (required(name) if name not in REFUSED else [])
        yield from itertools.product([name], KINDS, (False, True), MASKS, (False, True), removed)


def construct(Z, models, case, max_iters=1):
    name, kind, unpadder, masks, non_local, removed = case
    m = models[kind]
    return Z.Z_optimizer(name, m.Z_size, m.model, Z_range=1.0, max_iters=max_iters, data=m.data(name, removed), initial_Z=m.initial_Z.clone(),
                         initial_LR=0.05, batch_size=BATCH, HR_unpadder=(lambda t: t) if unpadder else None, non_local_Z_optimization=non_local,
                         **m.masks(masks), **m.kw)


def make_models(tmp):
    return {kind: Model(kind, tmp) for kind in KINDS}


def key_of(case):
    return '%s/%d/%s/%d/%s' % (case[1], case[2], case[3], case[4], 'complete' if case[5] is None else '-' + case[5])


def generate(Z, models):
    """{objective: {case key: 'ok' | 'Type: message'}} of the module Z (a Z_optimization)"""
    out = {}
    for case in cases(Z):
        try:
            construct(Z, models, case)
            answer = 'ok'
        except Exception as e:  # noqa: BLE001 - whatever the constructor raises is the record
            answer = '%s: %s' % (type(e).__name__, e)
        out.setdefault(case[0], {})[key_of(case)] = answer
    return out


def load():
    with open(GOLDEN) as f:
        g = json.load(f)
    return {name: {k: g['outcomes'][i] for k, i in by_key.items()} for name, by_key in g['cases'].items()}


def main():
    import Z_optimization as Z
    with tempfile.TemporaryDirectory() as tmp:
        matrix = generate(Z, make_models(tmp))
    outcomes = sorted({a for by_key in matrix.values() for a in by_key.values()})
    index = {a: i for i, a in enumerate(outcomes)}
    with open(GOLDEN, 'w') as f:
        f.write('{"outcomes": [\n%s\n],\n"cases": {\n' % ',\n'.join(json.dumps(a) for a in outcomes))
        f.write(',\n'.join('%s: %s' % (json.dumps(name), json.dumps({k: index[a] for k, a in by_key.items()}, separators=(',', ':')))
                           for name, by_key in matrix.items()))
        f.write('\n}}\n')
    n = sum(len(v) for v in matrix.values())
    print('%d cases, %d accepted, %d distinct answers, %d bytes' % (n, sum(a == 'ok' for v in matrix.values() for a in v.values()), len(outcomes),
                                                                    os.path.getsize(GOLDEN)))


if __name__ == '__main__':
    main()
