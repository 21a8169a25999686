"""One handle walked through the states of the noise model (wfs_noise.h: the model, inside it the colour, inside that the slow levels;
MI355X only).

After every step the handle's probes -- noise_samples on every channel, noise_white_samples and noise_slow_samples on every stream
where they apply -- are those of a fresh engine set directly to that state, and both are the numpy restatements of tests/noise_model.py,
noise_colour.py and noise_slow.py: exact integers, so ``==``.  What a transition drops must be gone (levels with a new colour, the
common streams' cells with a colour without groups, everything with a new model), and a refused call leaves the state as it was.
600 samples from t0 = -5 and from 2^33 + 1 give the residues 3 and 1 of t0 & 3 (two Philox calls per four samples, either split), two
256-sample block seams and the tail loop of the four-sample forms.
"""
import numpy as np
import pytest

from tests import noise_colour as NC
from tests import noise_slow as NS
from tests.helpers import make_engine, with_fma
from tests.test_gpu_noise_model import _designed_windows, _photon_sets
from wfsim_amd.config import kernel_params, xenonnt_test_config
from wfsim_amd.engine import WfsError

pytestmark = pytest.mark.gpu

N = 600
T0 = (-5, 2 ** 33 + 1)
VMIN = -4


@pytest.fixture(autouse=True)
def _check_launches(monkeypatch):
    monkeypatch.setenv('WFS_CHECK_LAUNCHES', '1')       # every launch checked on the spot


def _pmf(rows, seed):
    """rows x 9 values -4 .. 4, every row different, one value of the first row impossible"""
    p = np.random.default_rng(seed).uniform(0.05, 1.0, (rows, 9))
    p[0, 2] = 0.0
    return p / p.sum(axis=1, keepdims=True)


def _q16(shape, seed, scale=1.0):
    return np.rint(np.random.default_rng(seed).uniform(-scale, scale, shape) * 65536).astype(np.int64)


PMF_A, PMF_B = _pmf(3, 1), _pmf(2, 2)
COLOUR_3 = dict(taps_q=_q16((5, 3), 3), group=np.array([0, -1, 1]), mix_q=np.array([40000, 0, -65536]), common_pmf=_pmf(2, 4))
COLOUR_16 = dict(taps_q=_q16((3, 16), 5, 0.5), group=np.full(3, -1), mix_q=np.zeros(3, dtype=np.int64), common_pmf=np.zeros((0, 9)))
SLOW_5 = dict(shifts=[4, 6], slow_q=_q16((5, 2), 6, 0.8))           # levels of the three channels and the two common streams
SLOW_3 = dict(shifts=[4, 6], slow_q=_q16((3, 2), 7, 0.8))           # without a colour: the channels alone, on unit taps
SLOW_3['slow_q'][1, 0] = 0                                         # (an amplitude of 0 is skipped)
BAD_COLOUR = dict(COLOUR_3, group=np.array([0, 2, 1]))              # group 2 of two
BAD_SLOW = dict(shifts=[6, 4], slow_q=SLOW_3['slow_q'])             # descending

# the states the walk passes through: (pmf, colour, slow), None for what is not set
STATES = {
    '1_model': (PMF_A, None, None),
    '2_colour_L3_two_groups': (PMF_A, COLOUR_3, None),
    '3_slow_4_6': (PMF_A, COLOUR_3, SLOW_5),
    '4_colour_L16_no_groups': (PMF_A, COLOUR_16, None),
    '5_slow_without_colour': (PMF_A, None, SLOW_3),
    '6_slow_cleared': (PMF_A, None, None),
    '7a_refused_colour': (PMF_A, None, None),
    '7b_refused_slow': (PMF_A, None, None),
    '7c_colour_and_slow_again': (PMF_A, COLOUR_3, SLOW_5),
    '8_model_of_two_channels': (PMF_B, None, None),
}


def _probes(eng, state):
    """every probe that applies to the state, on every channel and stream"""
    pmf, colour, slow = state
    rows = len(pmf) + (len(colour['common_pmf']) if colour else 0)
    out = {}
    for t0 in T0:
        for ch in range(len(pmf)):
            out['noise', ch, t0] = eng.noise_samples(ch, t0, N)
        for row in range(rows):
            out['white', row, t0] = eng.noise_white_samples(row, t0, N)
            if slow:
                out['slow', row, t0] = eng.noise_slow_samples(row, t0, N)
    return out


def _set(eng, state):
    pmf, colour, slow = state
    eng.set_noise_model(pmf, VMIN)
    if colour:
        eng.set_noise_colour(**colour)
    if slow:
        eng.set_noise_slow(**slow)


def _absent(eng, state):
    """what the state does not have is refused by the probes: the streams beyond its rows, the slow part without levels"""
    pmf, colour, slow = state
    rows = len(pmf) + (len(colour['common_pmf']) if colour else 0)
    with pytest.raises(WfsError, match='channel outside the model'):
        eng.noise_samples(len(pmf), 0, 4)
    with pytest.raises(WfsError, match='row outside'):
        eng.noise_white_samples(rows, 0, 4)
    if slow:
        with pytest.raises(WfsError, match='row outside'):
            eng.noise_slow_samples(rows, 0, 4)
    else:
        with pytest.raises(WfsError, match='no noise model with slow levels'):
            eng.noise_slow_samples(0, 0, 4)


@pytest.fixture(scope='module')
def small():
    base = with_fma(xenonnt_test_config(seed=99), False)
    sets, calls = _photon_sets(_designed_windows(kernel_params(base))[:3], np.asarray(base['gains'], dtype=np.float64))
    noise = np.random.default_rng(5).integers(-9, 10, size=(3000, 494)).astype(np.int16)      # the table that is replayed when no model is set
    return dict(base, enable_noise=True, noise_data=noise), sets


@pytest.fixture(scope='module')
def walk(small):
    """the handle after its walk, and its probes after every step"""
    cfg, sets = small
    eng = make_engine(cfg)
    got = {}

    def step(name, act):
        act()
        _absent(eng, STATES[name])
        got[name] = _probes(eng, STATES[name])
    step('1_model', lambda: eng.set_noise_model(PMF_A, VMIN))
    step('2_colour_L3_two_groups', lambda: eng.set_noise_colour(**COLOUR_3))
    step('3_slow_4_6', lambda: eng.set_noise_slow(**SLOW_5))
    step('4_colour_L16_no_groups', lambda: eng.set_noise_colour(**COLOUR_16))       # the levels and the common cells go
    step('5_slow_without_colour', lambda: (eng.set_noise_colour(None), eng.set_noise_slow(**SLOW_3)))
    step('6_slow_cleared', lambda: eng.set_noise_slow(None))

    def refused(call, args, match):
        with pytest.raises(WfsError, match=match):
            call(**args)
    step('7a_refused_colour', lambda: refused(eng.set_noise_colour, BAD_COLOUR, 'group of channel 1 outside -1 .. n_groups - 1'))
    step('7b_refused_slow', lambda: refused(eng.set_noise_slow, BAD_SLOW, 'shifts not strictly ascending at level 1'))
    step('7c_colour_and_slow_again', lambda: (eng.set_noise_colour(**COLOUR_3), eng.set_noise_slow(**SLOW_5)))
    step('8_model_of_two_channels', lambda: eng.set_noise_model(PMF_B, VMIN))       # the colour and its levels go with the model
    eng.set_noise_model(None)                                                           # 9
    return eng, got


@pytest.mark.parametrize('name', list(STATES))
def test_step_is_a_fresh_engine_and_the_restatement(small, walk, name):
    cfg, sets = small
    state = STATES[name]
    got = walk[1][name]
    fresh = make_engine(cfg)
    _set(fresh, state)
    _absent(fresh, state)
    direct = _probes(fresh, state)
    fresh.close()
    pmf, colour, slow = state
    model, seed = NS.slow_model(pmf, VMIN, colour, slow), int(kernel_params(cfg)['seed'])
    want = {'noise': NS.slow_noise_values, 'white': NC.white_values, 'slow': NS.slow_values}
    assert sorted(got, key=str) == sorted(direct, key=str) and len(got) == len(T0) * (len(pmf) + (2 if slow else 1) * (len(pmf) + model['n_groups']))
    for key in got:
        kind, row, t0 = key
        exp = want[kind](model, seed, row, t0 + np.arange(N, dtype=np.int64))
        assert got[key].dtype == (np.int32 if kind == 'slow' else np.int16)
        assert np.array_equal(got[key], direct[key]), (name, key)
        assert np.array_equal(got[key].astype(np.int64), exp), (name, key, np.flatnonzero(got[key] != exp)[:8])


def test_the_steps_differ(walk):
    """the walk is not a walk in place: what a step sets shows in channel 0, what it clears restores the values from before"""
    got = walk[1]
    ch0 = lambda name: got[name]['noise', 0, T0[0]].tolist()
    assert len({tuple(ch0(n)) for n in ('1_model', '2_colour_L3_two_groups', '3_slow_4_6', '4_colour_L16_no_groups', '5_slow_without_colour',
                                        '8_model_of_two_channels')}) == 6
    assert ch0('6_slow_cleared') == ch0('1_model') == ch0('7a_refused_colour') == ch0('7b_refused_slow') and ch0('7c_colour_and_slow_again') == ch0('3_slow_4_6')
    assert np.any(got['3_slow_4_6']['slow', 4, T0[1]]) and np.any(got['5_slow_without_colour']['slow', 1, T0[0]])


def test_after_the_walk_the_records_are_those_without_a_model(small, walk):
    cfg, sets = small
    eng = walk[0]
    for probe in (eng.noise_samples, eng.noise_white_samples):
        with pytest.raises(WfsError, match='no noise model is set'):
            probe(0, 0, 4)
    with pytest.raises(WfsError, match='no noise model'):
        eng.set_noise_colour(**COLOUR_16)
    eng.set_debug(False)
    eng.load_photons(*sets)
    eng.run()
    never = make_engine(cfg)
    never.set_debug(False)
    never.load_photons(*sets)
    never.run()
    rec = eng.records()
    assert len(rec) > 0 and rec.tobytes() == never.records().tobytes()
    never.close()
