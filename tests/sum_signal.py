"""The bottom-array sum channel (config 'emit_sum_signal') restated in numpy from the oracle's pulses.

The reference builds row channel_map['sum_signal'] = 800 of its digitiser array at every digitisation (rawdata.py:241-254,
sum_signal at :392-396) and never masks it in, so neither it nor the oracle can emit the row.  The expectation of the tests is
therefore this restatement: the reference's own arithmetic for the row, plus the lines every masked row goes through.

    S[t]     = int(he_factor) * sum over the window's pulses on n_top <= channel <= last_bottom of -around(current * current_2_adc)
    range    = min(pulse left) - trigger_window .. max(pulse right) + trigger_window                (rawdata.py:234-235, 258-259)
    finished = clamp0(S + noise[(ix_rand + i) mod N, sum_signal] + baseline)                         (rawdata.py:398-458)
    ZLE      = find_intervals_below_threshold + window / clip / even landing                        (rawdata.py:290-311)

test_sum_signal_cpu.py pins S on the reference's recorded minimum and total of row 800 (tests/golden/chain_he.npz).
"""
import numpy as np

from oracle.oracle import Oracle, add_noise

SUM_CHANNEL = 800
SPR = 110           # samples per strax record


def expected_sum_rows(res, params, thr_zle, noise=None, ix_rand=None):
    """res: Oracle.results() (or a golden chain with pl_current instead of cur); params: kernel_params(config); noise: the noise
    array or None; ix_rand: noise start per window (default res['dg_ix_rand']).  One dict per digitise window that has a sum row:
    window, left / right (absolute samples), S (int64), finished (int64), intervals [(left, right)] (absolute samples)"""
    cur = res['cur'] if 'cur' in res else res['pl_current']
    tw, c2a, he = int(params['trigger_window']), float(params['c2a']), int(params['he_factor'])
    n_top, last_bottom = int(params['n_top']), int(params['last_bottom'])
    ch_sum = int(params['sum_channel'])
    out = []
    if not params['detector_nt']:
        return out
    ix_rand = res['dg_ix_rand'] if ix_rand is None else ix_rand
    for w in range(len(res['dg_left'])):
        p0, n = int(res['dg_first_pulse'][w]), int(res['dg_n_pulses'][w])
        pulses = [p for p in range(p0, p0 + n) if n_top <= res['pl_ch'][p] <= last_bottom]
        if not pulses:
            continue
        left = min(int(res['pl_left'][p]) for p in pulses) - tw
        right = max(int(res['pl_right'][p]) for p in pulses) + tw
        S = np.zeros(right - left + 1, dtype=np.int64)
        for p in pulses:
            a, m = int(res['pl_cur_off'][p]), int(res['pl_right'][p] - res['pl_left'][p] + 1)
            adc = -np.around(cur[a:a + m] * c2a).astype(np.int64)               # rawdata.py:236
            S[int(res['pl_left'][p]) - left:int(res['pl_left'][p]) - left + m] += adc
        S *= he                                                                 # rawdata.py:242, 251-254
        fin = S.copy()[None, :]
        if params['enable_noise'] and noise is not None and np.asarray(noise).shape[1] > ch_sum and ix_rand[w] >= 0:
            add_noise(fin, [1], [0], [len(S) - 1], np.ascontiguousarray(np.asarray(noise)[:, ch_sum:ch_sum + 1]), int(ix_rand[w]))
        fin = np.maximum(fin[0] + int(params['baseline']), 0)
        itv = []
        for a, b in Oracle.find_intervals_below_threshold(fin, int(thr_zle[ch_sum]), 2 * tw + 1):
            a, b = np.clip([a - tw, b + tw], 0, len(fin) - 1)                   # rawdata.py:302-304
            a, b = int(np.ceil(a / 2) * 2), int(np.floor(b / 2) * 2)            # rawdata.py:305-306
            itv.append((left + a, left + b))
        out.append(dict(window=w, left=left, right=right, S=S, finished=fin, intervals=itv))
    return out


def expected_sum_records(rows, dt=10):
    """the strax records of the rows' intervals, as the layout of every other channel has them (strax_interface.py:425-435):
    (time, pulse_length, record_i, length, samples) per record, in row / interval / fragment order"""
    out = []
    for r in rows:
        for a, b in r['intervals']:
            plen = b - a + 1
            for f in range(max(0, -(-plen // SPR))):
                n = min(SPR, plen - SPR * f)
                data = np.zeros(SPR, dtype=np.int16)
                data[:n] = r['finished'][a - r['left'] + SPR * f:a - r['left'] + SPR * f + n].astype(np.int16)
                out.append((dt * (a + SPR * f), plen, f, n, data.tobytes()))
    return out


def record_tuples(rec):
    return [(int(x['time']), int(x['pulse_length']), int(x['record_i']), int(x['length']), np.asarray(x['data'], dtype=np.int16).tobytes())
            for x in rec]


def engine_sum_rows(eng):
    """Engine.sum_signal() as a list of (window among the non-empty ones, left, right, S)"""
    g = eng.groups()
    keep = np.where(g['right'] >= g['left'])[0]
    gmap = {int(gi): j for j, gi in enumerate(keep)}
    s = eng.sum_signal()
    return [(gmap[int(s['group'][k])], int(s['left'][k]), int(s['right'][k]), s['data'][s['data_off'][k]:s['data_off'][k + 1]])
            for k in range(len(s['group']))]


def assert_sum_rows(eng, exp):
    """the engine's unfinished sum rows, their ranges, the finished samples inside the intervals and the channel's records against
    the restatement"""
    got = engine_sum_rows(eng)
    assert [(g[0], g[1], g[2]) for g in got] == [(e['window'], e['left'], e['right']) for e in exp]
    for g, e in zip(got, exp):
        assert np.array_equal(g[3], e['S']), f"window {e['window']}: S differs"
    rec = eng.records()
    ch = int(eng.params['sum_channel'])
    assert record_tuples(rec[rec['channel'] == ch]) == expected_sum_records(exp, int(eng.params['dt']))
    return rec
