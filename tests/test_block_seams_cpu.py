"""The designed cases of tests/block_seams.py reach the seams they are made for: every case through the CPU oracle, the seam table of
DESIGN.md 5 computed from the oracle's photons per emitter.  A condition on the INPUTS of tests/test_gpu_block_seams.py, not on the code
under test.  Also: the order-exact comparison of tests/helpers.py on a copied oracle result, and the oracle's per-emitter counts."""
import functools

import numpy as np
import pytest

from tests import block_seams as B
from tests.helpers import assert_tiles_in_oracle_order


@functools.lru_cache(maxsize=None)
def _table():
    """{case: (seams reached, sizes, block table, photons)} -- every case once through the oracle"""
    out = {}
    for name, case in B.cases().items():
        cfg, res, s, orc, o = B.oracle_case(case)
        t = B.block_table(o, s['s_ins'], cfg)
        assert t['n_photons'] == int((o['call_ph_off'][1:] - o['call_ph_off'][:-1])[o['call_kind'] != 3].sum()), name
        found, z = B.seams(case, s, orc, o, t)
        out[name] = (found, z, t, len(o['ph_t']), o, s)
    return out


def test_emitter_counts_add_up_to_the_photons_of_every_call():
    """Oracle.get('em_nph'): per loaded instruction the photons of its candidate emitters; their sums per Pulse call are the call's photons"""
    for name, (found, z, t, n, o, s) in _table().items():
        prim = np.flatnonzero(o['call_kind'] != 3)
        per_call = np.bincount(t['call'], weights=t['ins_nph'], minlength=len(prim)).astype(np.int64)
        assert np.array_equal(per_call, np.diff(o['call_ph_off'])[prim]), name
        n_em, em_off = B.emitters(s['s_ins'])
        exact = (s['s_ins']['type'] == 1) & (s['ip']['p_hit'] == 1.0)
        assert np.array_equal(t['ins_nph'][exact], s['s_ins']['amp'][exact]), name       # p_hit = 1: hits = amp


def test_every_seam_is_reached_by_a_designed_case():
    table = _table()
    by_row = {row: [name for name, v in table.items() if row in v[0]] for row in B.ROWS}
    print()
    for row in B.ROWS:
        print(f'{row:45s} {", ".join(by_row[row])}')
    for name, (found, z, t, n, o, s) in table.items():
        print(f'{name:24s} {n:8d} photons, {t["n_blocks"]:4d} blocks ({int(t["fast"].sum())} fast), fullsort instructions {int(t["fullsort"].sum())}, '
              f'largest head / tail {int(max(t["head"].max(), t["tail"].max()))}')
        assert found <= set(B.ROWS), found - set(B.ROWS)
        big = any(len(x) and x.max() > B.ORDER_MAX for x in (z['fullsort'], z['afterpulse']))
        assert n <= (1.5e6 if big else 5e5), (name, n)
        assert max(t['head'].max(), t['tail'].max()) <= B.GEN_BLOCK                   # a head or a tail lies in one block
    missing = [row for row in B.ROWS if not by_row[row]]
    assert not missing, missing
    # the sizes on either side of TILE_ORDER_MAX
    for kind in ('fullsort', 'afterpulse'):
        x = np.concatenate([v[1][kind] for v in table.values()])
        below, above = int(x[x <= B.ORDER_MAX].max()), int(x[x > B.ORDER_MAX].min())
        print(f'{kind} tiles nearest to {B.ORDER_MAX}: {below} and {above}')
        assert (below, above) == EDGE_4096[kind]
    # what the designed cases were chosen for
    assert {'nwin_512', 'nwin_513', 'wide_block_inside'} <= table['window_limit'][0]
    assert 'wide_block_at_last_photon' in table['wide_at_last_photon'][0] and 'layout_head_tail_no_ranges' in table['wide_at_last_photon'][0]
    assert 'wide_block_at_first_photon' in table['wide_at_first_photon'][0]
    assert {f'segment_exactly_{v}' for v in (64, 65)} <= table['segments'][0]
    assert {f'afterpulse_exactly_{v}' for v in (12, 13, 64, 65)} | {'afterpulse_above_4096'} <= table['ap_sizes'][0]
    assert {f'r0_and_3_is_{v}' for v in range(4)} <= table['quad_phase'][0]


EDGE_4096 = dict(fullsort=(4096, 4097), afterpulse=(4088, 4104))          # (fullsort: designed; afterpulse: the nearest the seed search found)


def test_cases_are_reproducible():
    a, b = B.cases(), B.cases()
    assert list(a) == list(b)
    for name in a:
        assert np.array_equal(a[name]['ins'], b[name]['ins']) and a[name]['overrides'] == b[name]['overrides'], name


# ------------------------------------------------------------------------------------------------ the helper on its own
class _Stored:
    """stands in for an engine: photons() of one pulse set per oracle call"""
    def __init__(self, o):
        self.ph = dict(set_off=o['call_ph_off'].copy(), t=o['ph_t'].copy(), ch=o['ph_ch'].copy(), gain=o['ph_gain'].copy(), dpe=o['ph_dpe'].copy())

    def photons(self):
        return self.ph


def test_order_helper_sees_a_swap_inside_a_channel():
    o = _table()['below_one_block'][4]
    sets = list(range(len(o['call_kind'])))
    assert_tiles_in_oracle_order(_Stored(o), o, sets)
    # two photons of one channel that differ in time: swapping them is an error, named by call, channel and position
    ch = o['ph_ch'][:int(o['call_ph_off'][1])]
    c = int(np.argmax(np.bincount(ch)))
    at = np.flatnonzero(ch == c)
    i, j = at[0], next(k for k in at[1:] if o['ph_t'][k] != o['ph_t'][at[0]])
    st = _Stored(o)
    for f in ('t', 'gain', 'dpe'):
        st.ph[f][[i, j]] = st.ph[f][[j, i]]
    with pytest.raises(AssertionError, match=f'call 0 .*channel {c}: first difference at position 0; tile sizes oracle {len(at)}, device {len(at)}'):
        assert_tiles_in_oracle_order(st, o, sets)
    # ... while the comparison sorted by (channel, time, gain) does not see it
    ko, kg = np.lexsort((o['ph_gain'], o['ph_t'], o['ph_ch'])), np.lexsort((st.ph['gain'], st.ph['t'], st.ph['ch']))
    assert all(np.array_equal(o['ph_' + f][ko], st.ph[f][kg]) for f in ('t', 'gain', 'dpe', 'ch'))
    # two identical photons: swapping them changes nothing
    st = _Stored(o)
    for f in ('t', 'gain', 'dpe'):
        st.ph[f][j] = st.ph[f][i]
    o2 = dict(o, ph_t=st.ph['t'].copy(), ph_gain=st.ph['gain'].copy(), ph_dpe=st.ph['dpe'].copy())
    for f in ('t', 'gain', 'dpe'):
        st.ph[f][[i, j]] = st.ph[f][[j, i]]
    assert_tiles_in_oracle_order(st, o2, sets)
    # a photon moved to another channel
    st = _Stored(o)
    st.ph['ch'][i] = c + 1 if c + 1 < B.NCH else c - 1
    with pytest.raises(AssertionError, match='call 0 '):
        assert_tiles_in_oracle_order(st, o, sets)
    # a set of another size, a missing set
    with pytest.raises(AssertionError):
        assert_tiles_in_oracle_order(_Stored(o), o, sets[:-1])
