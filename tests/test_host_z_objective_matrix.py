"""What Z_optimizer's constructor accepts and refuses, pinned case by case: objective name (every supported one and the refused spellings) x
model (SR, JPEG Y, JPEG colour) x HR_unpadder x masks x non_local_Z_optimization x data (complete, or one required key missing), against
tests/golden/z_objective_matrix.json, which tools/gen_z_objective_matrix.py wrote at the commit before the objectives became table entries.
Each answer is 'ok' or the exception's type and full message; where a call is wrong in two ways the recorded refusal is the first one.  CPU
only: the models are the small ones the other host tests build, made once for the module."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_tool():
    spec = importlib.util.spec_from_file_location('gen_z_objective_matrix', os.path.join(ROOT, 'tools', 'gen_z_objective_matrix.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


M = _load_tool()


@pytest.fixture(scope='module')
def matrices(tmp_path_factory):
    import Z_optimization
    return M.load(), M.generate(Z_optimization, M.make_models(str(tmp_path_factory.mktemp('z_matrix'))))


def test_the_fixture_covers_every_name_and_every_axis():
    import Z_optimization
    want = M.load()
    assert list(want) == M.names(Z_optimization) and set(M.REFUSED).isdisjoint(Z_optimization.Z_optimizer.SUPPORTED)
    assert {'random_VGG_limited', 'random_l1_local', 'local_TV', 'periodicityPlus', 'local_STD_periodicityPlus_1D', 'STD_increasePlus', 'local_Mag_max',
            'patchhist_localSTD', 'hist_no_localSTD', 'digit'} <= set(M.REFUSED) and len(M.REFUSED) >= 15
    for name, by_key in want.items():
        assert list(by_key) == [M.key_of(case) for case in M.cases(Z_optimization) if case[0] == name], name
        assert len(by_key) == 3 * 2 * 3 * 2 * (1 + (len(M.required(name)) if name not in M.REFUSED else 0))
    answers = [a for by_key in want.values() for a in by_key.values()]
    assert all(a != 'ok' for name in M.REFUSED for a in want[name].values())
    assert answers.count('ok') > 400                           # the accepted cells are a real share, not a corner
    assert os.path.getsize(M.GOLDEN) < 1 << 20


def test_every_case_answers_as_recorded(matrices):
    want, got = matrices
    assert list(got) == list(want)
    wrong = [(name, key, want[name][key], got[name].get(key)) for name in want for key in want[name] if got[name].get(key) != want[name][key]]
    for name, key, w, g in wrong[:20]:
        print('%s  %s\n    recorded: %s\n    now:      %s' % (name, key, w, g))
    assert not wrong, '%d of %d cases answer differently' % (len(wrong), sum(len(v) for v in want.values()))
    assert all(list(got[name]) == list(want[name]) for name in want)          # and no case beyond the recorded ones
