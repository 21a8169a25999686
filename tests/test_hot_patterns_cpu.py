"""The random mixes under peaked hit patterns (tests/hot_patterns.py) reach the seams they are made for: every default seed through
the CPU oracle, the coverage table of DESIGN.md 5 counted from the oracle's photons.  A condition on the INPUTS of
tests/test_gpu_hot_patterns.py, not on the code under test."""
import collections

import numpy as np

from tests import hot_patterns as H


def _equal(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a, key=str) == sorted(b, key=str) and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.asarray(a).dtype == np.asarray(b).dtype and np.array_equal(a, b)
    return type(a) is type(b) and a == b


def test_hot_case_is_reproducible():
    for seed in range(min(H.N_SEEDS, 24)):
        a, b = H.hot_case(seed), H.hot_case(seed)
        assert len(a) == len(b) == 5
        for x, y in zip(a, b):
            assert _equal(x, y), seed
    assert not np.array_equal(H.hot_case(4)[1], H.hot_case(6)[1])


def test_default_seeds_reach_every_seam():
    reached = collections.Counter()
    photons, largest = [], 0
    for seed in range(24):
        cfg, ins, ap, noise, knobs, s, orc, o = H.oracle_case(seed)
        assert (ap is not None) == bool(cfg.get('enable_pmt_afterpulses', False)) and (noise is not None) == bool(cfg.get('enable_noise', False))
        assert isinstance(cfg['s2_pattern_map'], dict) == (seed % 2 == 0) == ('hot_rows' not in cfg)
        found = H.seams(cfg, ins, o)
        assert found <= set(H.COVERAGE)
        reached.update(found)
        n = H.tile_sizes(o)
        assert n.shape == (len(o['call_kind']), H.NCH) and n.sum() == len(o['ph_t'])
        photons.append(len(o['ph_t']))
        largest = max(largest, int(n.max()))
        bright, tg, first = H.bright_tiles(cfg, s, o)
        if seed in H.KNOB_SEEDS:
            assert bright.any(), seed
    print('cases reaching each seam:', dict(reached))
    print(f'photons per case {min(photons)} .. {max(photons)}, {sum(photons)} in all; largest tile {largest}')
    for seam, need in H.COVERAGE.items():
        assert reached[seam] >= need, (seam, reached[seam], need)
    assert max(photons) < 1.5e6
    for seed in H.BATCH_SEEDS + H.SHARD_SEEDS + H.EAP_SEEDS:          # RawData takes the map from the config
        assert isinstance(H.hot_case(seed)[0]['s2_pattern_map'], dict), seed
    assert set(H.CARRY_SEEDS) <= set(H.BATCH_SEEDS)


def test_designed_batch_cases_hold_an_open_window_with_a_bright_s2():
    """hot_patterns.batch_case: behind the drawn instructions a closed window, then ONE window that holds a bright S2 and the cluster
    that follows it -- what RawData meets open at the end of a batch that began before them"""
    for seed in H.CARRY_DESIGNED:
        cfg, ins, ap, noise, knobs = H.batch_case(seed)
        n = len(H.hot_case(seed)[1])
        assert len(ins) == n + 4 and np.array_equal(ins[:n], H.hot_case(seed)[1])
        res = H.resource_of(cfg)
        s = H.scheduled(cfg, ins, res)
        orc, o = H.run_oracle(cfg, ap, res, s)
        pos = {int(e): k for k, e in enumerate(s['s_ins']['event_number'])}
        a, e, b, c = (pos[n + k] for k in range(4))
        assert s['cluster'][a] < s['cluster'][e] == s['cluster'][b] < s['cluster'][c] and e < b      # three clusters, the S2 not the first of its own
        est = np.where(s['s_ins']['type'] == 1, s['s_ins']['amp'] * 0.15, s['s_ins']['amp'] * cfg['s2_secondary_sc_gain'])      # RawData._expected_quanta
        assert est[a] + est[e] < 500 < 60_000 < est[b]                             # the bound is passed with the S2 and not before
        bright, tg, first = H.bright_tiles(cfg, s, o)
        assert bright[s['call'][b]].any()
        t = [int(s['key'][k]) // int(cfg['sample_duration']) for k in (a, b, c)]
        w = [int(np.searchsorted(o['dg_left'], x, side='right')) - 1 for x in t]
        assert w[0] + 1 == w[1] == w[2] and o['dg_right'][w[1]] > t[2]             # the S1 alone, the S2 and its follower in one window
