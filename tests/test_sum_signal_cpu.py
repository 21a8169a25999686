"""The bottom-array sum channel (config 'emit_sum_signal'), host side.  CPU only.

* the numpy restatement the GPU tests compare with (tests/sum_signal.py) against the reference's own row 800: the golden recorder
  stored its minimum and total per digitise window (dg_sum_min / dg_sum_total of chain_he.npz);
* the config key and the C ABI declarations;
* ChunkRawRecords: records on channel_map['sum_signal'] go to raw_records_aqmon and to nothing else.
"""
import os

import numpy as np

from tests.helpers import golden, make_oracle, replay_chain_on_oracle, with_fma
from tests.sum_signal import expected_sum_rows
from wfsim_amd.config import kernel_params, xenonnt_test_config
from wfsim_amd.dtypes import instruction_dtype, raw_record_dtype
from wfsim_amd.strax_interface import ChunkRawRecords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_reference_row_800():
    """chain_he.npz replayed on the oracle (the reference's two roundings, so that the currents are the reference's bit for bit):
    minimum and total of S equal those of the reference's row 800 in every window; window 0 saturates"""
    cfg = with_fma(xenonnt_test_config(high_energy_deamplification_factor=20), False)
    d = golden('chain_he.npz')
    orc = make_oracle(cfg)
    res = replay_chain_on_oracle(orc, d)
    rows = expected_sum_rows(res, kernel_params(cfg), orc.tables['thr_zle'])
    assert [r['window'] for r in rows] == list(range(len(d['dg_left'])))
    assert [int(r['S'].min()) for r in rows] == d['dg_sum_min'].tolist() == [-30440, -13320, -9940]
    assert [int(r['S'].sum()) for r in rows] == d['dg_sum_total'].tolist() == [-300780, -2181460, -97020]
    assert int(np.sum(rows[0]['finished'] == 0)) == 7 and all(np.all(r['finished'] > 0) for r in rows[1:])
    # the row lies inside the window, on the union of the bottom rows
    for r in rows:
        assert d['dg_left'][r['window']] <= r['left'] and r['right'] <= d['dg_right'][r['window']]
        assert len(r['intervals']) >= 1


def test_config_key_and_header():
    assert kernel_params(xenonnt_test_config())['sum_signal'] == 0
    assert kernel_params(xenonnt_test_config(emit_sum_signal=True))['sum_signal'] == 1
    assert kernel_params(xenonnt_test_config(emit_sum_signal=True))['sum_channel'] == 800
    header = open(os.path.join(ROOT, 'include', 'wfsim_amd.h')).read()
    assert 'int wfs_set_sum_signal(wfs_handle *h, int32_t on);' in header
    assert 'int wfs_copy_sum_signal(wfs_handle *h, int32_t *group, int64_t *left, int64_t *right, int64_t *data_off, int64_t *data,' in header
    from wfsim_amd import engine
    assert 'wfs_set_sum_signal' in engine.EXPORTS and 'wfs_copy_sum_signal' in engine.EXPORTS


class _StubEngine:
    emits_he_records = False

    def __init__(self, emits_sum_records):
        if emits_sum_records is not None:
            self.emits_sum_records = emits_sum_records

    def set_record_order(self, by_time):
        assert by_time


class _BatchRawData:
    """one batch of two windows, records ordered by (time, channel) as the device hands them over; channels 3, 700 (HE) and 800"""
    emits_sum_records = True
    channels = (3, 800)

    def __init__(self, config):
        self.config, self.source_finished, self.left, self.right = config, False, 0, 0
        self.engine = _StubEngine(self.emits_sum_records)

    def iter_batches(self, instructions, want_truth=True, record_sink=None, **kw):
        dtype = np.dtype(raw_record_dtype())
        left = np.array([100_000, 300_000], dtype=np.int64)
        rec = np.zeros(2 * len(self.channels), dtype=dtype)
        rec['time'] = np.repeat(10 * (left + 10), len(self.channels))
        rec['channel'] = np.tile(self.channels, 2)
        rec['dt'], rec['length'], rec['pulse_length'] = 10, 50, 50
        rec['data'][:, :50] = 15990
        yield dict(records=rec, first=np.array([0, len(self.channels), len(rec)]), left=left, right=left + 200, truth_table=None,
                   truth_rows=np.zeros(0, dtype=np.int64), truth_before=np.zeros(0, dtype=np.int64), finished=True)


def _chunks(rawdata):
    cfg = xenonnt_test_config(chunk_size=1, pin_record_buffer=False)
    ChunkRawRecords.record_buffer_length = 1000
    sim = ChunkRawRecords(cfg, rawdata_generator=rawdata)
    ins = np.zeros(1, dtype=instruction_dtype)
    ins['time'], ins['type'], ins['amp'] = 1_000_000, 1, 10
    out = list(sim(ins))
    assert sim.source_finished() and len(out) == 1
    return out[0]


def test_chunker_routes_sum_records_to_aqmon():
    c = _chunks(_BatchRawData)
    assert len(c['raw_records_aqmon']) == 2 and np.all(c['raw_records_aqmon']['channel'] == 800)
    assert len(c['raw_records']) == 2 and np.all(c['raw_records']['channel'] == 3)
    assert len(c['raw_records_he']) == 0

    class WithHe(_BatchRawData):
        channels = (3, 700, 800)
    c = _chunks(WithHe)
    assert [c[k]['channel'].tolist() for k in ('raw_records', 'raw_records_he', 'raw_records_aqmon')] == [[3, 3], [700, 700], [800, 800]]


def test_chunker_hands_out_tpc_records_when_no_sum_row_can_occur():
    """neither HE nor sum records: the buffer's prefix goes out as raw_records, the other two kinds are empty (an engine that does not
    know the switch counts as one without it)"""
    for flag in (False, None):
        class Tpc(_BatchRawData):
            emits_sum_records = flag
            channels = (3, 7)
        c = _chunks(Tpc)
        assert c['raw_records']['channel'].tolist() == [3, 7, 3, 7]
        assert len(c['raw_records_he']) == 0 and len(c['raw_records_aqmon']) == 0
