"""The noise model on the CPU: the config forms (wfsim_amd/noise_model.py), the numpy restatement of a sample's noise
(tests/noise_model.py) and its statistics under the seed the GPU test reuses, the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

from tests import noise_model as NM
from wfsim_amd.config import xenonnt_test_config
from wfsim_amd.noise_model import check_pmf, gaussian_pmf, noise_pmf, pmf_from_samples
from wfsim_amd.workloads import synthetic_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS = 801


@pytest.mark.parametrize('sigma', [0.7, 2.2, 9.0])
def test_gaussian_form(sigma):
    pmf, vmin = noise_pmf(dict(xenonnt_test_config(), noise_model={'sigma': sigma}), N_ROWS)
    half = max(1, int(np.ceil(6 * sigma)))
    assert pmf.shape == (494, 2 * half + 1) and vmin == -half
    assert np.all(np.abs(pmf.sum(axis=1) - 1) <= 1e-12) and np.all(pmf >= 0)
    assert np.array_equal(pmf, pmf[:, ::-1])                                       # symmetric, exactly
    k = np.arange(vmin, vmin + pmf.shape[1])
    var = (pmf[0] * k ** 2).sum() - (pmf[0] * k).sum() ** 2
    assert abs(var / (sigma ** 2 + 1 / 12) - 1) < 0.01, var


def test_gaussian_zero_and_channel_counts():
    pmf, vmin = gaussian_pmf([0.0, 2.0])
    assert vmin == -12 and pmf[0, 12] == 1.0 and pmf[0].sum() == 1.0 and pmf[1, 12] < 0.3
    pmf, vmin = gaussian_pmf(0.0)
    assert vmin == -1 and pmf.tolist() == [[0.0, 1.0, 0.0]]
    cfg = xenonnt_test_config()
    assert noise_pmf(cfg, N_ROWS) is None and noise_pmf(dict(cfg, noise_model=None), N_ROWS) is None
    assert noise_pmf(dict(cfg, noise_model={'sigma': 1.5}), N_ROWS)[0].shape[0] == len(cfg['gains'])
    assert noise_pmf(dict(cfg, noise_model={'sigma': np.full(801, 1.5)}), N_ROWS)[0].shape[0] == 801
    assert noise_pmf(dict(cfg, noise_model={'sigma': [1.0, 2.0, 0.0]}), N_ROWS)[0].shape == (3, 25)
    pmf, vmin = noise_pmf(dict(cfg, noise_model={'pmf': [[0.25, 0.75], [1.0, 0.0]], 'vmin': -1}), N_ROWS)
    assert pmf.shape == (2, 2) and vmin == -1


def test_pmf_from_samples_is_the_histogram():
    noise = synthetic_noise()
    m = pmf_from_samples(noise)
    pmf, vmin = noise_pmf(dict(xenonnt_test_config(), noise_model=m), N_ROWS)
    assert pmf.shape[0] == noise.shape[1] and vmin == noise.min() and vmin + pmf.shape[1] - 1 == noise.max()
    for ch in (0, 17, noise.shape[1] - 1):
        values, counts = np.unique(noise[:, ch], return_counts=True)
        exp = np.zeros(pmf.shape[1])
        exp[values - vmin] = counts / len(noise)
        assert np.array_equal(pmf[ch], exp)


@pytest.mark.parametrize('model,match', [
    ({'pmf': [[0.5, 0.6, -0.1]], 'vmin': 0}, 'negative'),
    ({'pmf': [[0.5, 0.4]], 'vmin': 0}, 'sum to 1'),
    ({'pmf': [[0.5, 0.5 + 1e-8]], 'vmin': 0}, 'sum to 1'),
    ({'pmf': [[0.5, 0.5]], 'vmin': 32767}, 'int16'),
    ({'pmf': [[0.5, 0.5]], 'vmin': -32769}, 'int16'),
    ({'pmf': np.full((1, 4097), 1 / 4097), 'vmin': 0}, '4096'),
    ({'sigma': 400.0}, '4096'),
    ({'sigma': -1.0}, 'non-negative'),
    ({'pmf': np.full((802, 2), 0.5), 'vmin': 0}, 'n_channels'),
    ({'pmf': [[1.0]]}, 'vmin'),
    ({'sigma': 1.0, 'pmf': [[1.0]], 'vmin': 0}, 'either'),
])
def test_bad_input_raises(model, match):
    with pytest.raises(ValueError, match=match):
        noise_pmf(dict(xenonnt_test_config(), noise_model=model), N_ROWS)


def test_pmf_from_samples_refuses_what_the_model_cannot_hold():
    with pytest.raises(ValueError, match='4096'):
        pmf_from_samples(np.array([[0], [5000]]))
    with pytest.raises(ValueError, match='integral'):
        pmf_from_samples(np.array([[0.5], [1.0]]))
    check_pmf(np.full((1, 4096), 1 / 4096), -2048)


def test_resource_does_not_demand_noise_data_with_a_model():
    from wfsim_amd.resource import Resource
    r = Resource(xenonnt_test_config(enable_noise=True, noise_model={'sigma': 2.2}))
    assert not hasattr(r, 'noise_data')
    with pytest.raises(KeyError):
        Resource(xenonnt_test_config(enable_noise=True))
    noise = synthetic_noise(n_samples=16)
    assert hasattr(Resource(xenonnt_test_config(enable_noise=True, noise_model={'sigma': 2.2}, noise_data=noise)), 'noise_data')


# ---------------------------------------------------------------------------------------------------- the restatement
def test_vectorised_philox_is_the_oracles():
    rng = np.random.default_rng(1)
    ctr = rng.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64)
    ctr[0] = [0, 0, 0, 0]
    ctr[1] = [0xFFFFFFFF] * 4
    ctr[2] = [0xFFFFFFFF, 0x3FFFFFFF, 800, NM.SITE_NOISE_SAMPLE]
    for seed in (0, NM.STAT_SEED, 0xFFFFFFFFFFFFFFFF, 0x243F6A8885A308D3):
        assert NM.philox_matches_oracle(seed, ctr)


def test_alias_cells_encode_the_pmf():
    pmf, vmin = gaussian_pmf([0.0, 0.7, 2.2, 9.0])
    thr, alias, shift = NM.build_cells(pmf)
    K = thr.shape[1]
    assert K == 128 and shift == 25 and np.all(alias < K)
    for ch in range(len(pmf)):
        mass = NM.cells_pmf(thr[ch], alias[ch], pmf.shape[1])
        assert np.all(np.abs(mass[:pmf.shape[1]] - pmf[ch]) <= K * 2.0 ** -32) and np.all(mass[pmf.shape[1]:] <= K * 2.0 ** -32)
    # a distribution of one value: two cells, both give value 0
    thr1, alias1, shift1 = NM.build_alias([1.0])
    assert shift1 == 31 and NM.alias_sample(thr1, alias1, shift1, [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]).tolist() == [0, 0, 0, 0]


def test_quad_and_word_of_a_sample():
    """the counter of a sample is its quad t >> 2 (arithmetic shift, 64 bits over two counter words), its word t & 3"""
    pmf, vmin = gaussian_pmf([3.0])
    thr, alias, shift = NM.build_cells(pmf)
    seed = 77
    for t in (0, 5, -1, -6, 2 ** 34 - 5, 2 ** 34 + 2, -2 ** 40 + 3):
        q = t >> 2
        w = NM.philox4x32_10(q & 0xFFFFFFFF, (q >> 32) & 0xFFFFFFFF, 0, 65, seed)[:, 0]
        exp = vmin + int(NM.alias_sample(thr[0], alias[0], shift, [w[t & 3]])[0])
        assert NM.noise_values((thr[0], alias[0]), shift, vmin, seed, 0, [t]).tolist() == [exp]
    t = np.arange(-9, 23)
    a = NM.noise_values((thr[0], alias[0]), shift, vmin, seed, 0, t)
    assert a.tolist() == [int(NM.noise_values((thr[0], alias[0]), shift, vmin, seed, 0, [x])[0]) for x in t]
    assert a.tolist() != NM.noise_values((thr[0], alias[0]), shift, vmin, seed, 1, t).tolist()
    assert a.tolist() != NM.noise_values((thr[0], alias[0]), shift, vmin, seed + 1, 0, t).tolist()


def test_restatement_is_white_with_the_right_distribution():
    sigma = np.full(494, 2.2)
    sigma[NM.STAT_CHANNELS[1]] = 0.7
    pmf, vmin = gaussian_pmf(sigma)
    thr, alias, shift = NM.build_cells(pmf[list(NM.STAT_CHANNELS)])
    t = NM.STAT_T0 + np.arange(NM.STAT_N, dtype=np.int64)
    sa, sb = (NM.noise_values((thr[k], alias[k]), shift, vmin, NM.STAT_SEED, ch, t) for k, ch in enumerate(NM.STAT_CHANNELS))
    NM.assert_white(sa, sb, pmf[NM.STAT_CHANNELS[0]], pmf[NM.STAT_CHANNELS[1]], vmin)


def test_materialised_table_holds_the_rows():
    pmf, vmin = gaussian_pmf([1.0, 0.0, 4.0])
    rows = [(0, 0, 1001, 7), (0, 2, 998, 30), (1, 1, 5000, 9), (1, 2, 2 ** 34 + 1, 5), (1, 5, 4000, 50)]
    table, ix = NM.materialise(rows, 2, pmf, vmin, seed=9, n_columns=4)
    assert table.shape == (30 + 8 + 50 + 8, 4) and ix.tolist() == [0, 38]
    thr, alias, shift = NM.build_cells(pmf)
    for w, ch, first, length in rows[:4]:
        exp = NM.noise_values((thr[ch], alias[ch]), shift, vmin, 9, ch, first + np.arange(length))
        assert table[ix[w]:ix[w] + length, ch].tolist() == exp.tolist()
    assert not table[:, 1].any() and not table[:, 3].any() and table[:, 2].any()


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_engine_lists_the_entry_points():
    from wfsim_amd import engine
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wfsim_amd.h')).read(), flags=re.S)
    for name in ('wfs_set_noise_model', 'wfs_noise_model_samples', 'wfs_copy_noise_model'):
        assert re.search(r'\bint\s+' + name + r'\s*\(\s*wfs_handle\s*\*', txt), name
        assert name in engine.EXPORTS
    src = open(os.path.join(ROOT, 'wfsim_amd', 'csrc', 'wfs_device.h')).read()
    assert re.search(r'SITE_NOISE\s*=\s*64\b', src) and re.search(r'SITE_NOISE_SAMPLE\s*=\s*65\b', src)
