"""config['overlay_records']: the host side of salting -- the recorded raw_records a run is overlaid on, the pulses a
pass takes from them, and the cut of a pulse at the sample where a window of a later batch can first begin.  The merge itself is the
device pass ``Engine.overlay_records`` (wfs_overlay_records)."""
import numpy as np

from .dtypes import DEFAULT_RECORD_LENGTH as SPR, raw_record_dtype

DTYPE = np.dtype(raw_record_dtype())


def sort_records(rec):
    return rec[np.lexsort((rec['channel'], rec['time']))]


def records_of_pulse(channel, s0, data, dt):
    """the fragments of one pulse: samples ``data`` from absolute sample s0 on"""
    n = (len(data) + SPR - 1) // SPR
    rec = np.zeros(n, dtype=DTYPE)
    f = np.arange(n)
    rec['time'], rec['dt'], rec['channel'], rec['pulse_length'], rec['record_i'] = (s0 + SPR * f) * dt, dt, channel, len(data), f
    rec['length'] = np.minimum(len(data) - SPR * f, SPR)
    for k in range(n):
        rec['data'][k, :rec['length'][k]] = data[SPR * k:SPR * (k + 1)]
    return rec


def pulse_start(rec):
    """first sample of the pulse every record belongs to"""
    return rec['time'] // rec['dt'].astype(np.int64) - SPR * rec['record_i'].astype(np.int64)


def cut_pulses(rec, cut, dt):
    """(front, rest) of whole pulses cut at absolute sample ``cut``: a pulse that runs past cut - 1 ends there, and its samples from
    ``cut`` on are a pulse of their own in ``rest``.  Pulses that end in front of ``cut`` are handed on as they are.  Both in
    (time, channel) order."""
    if not len(rec):
        return rec, rec[:0]
    s0 = pulse_start(rec)
    over = s0 + rec['pulse_length'] > cut
    if not over.any():
        return rec, rec[:0]
    fronts, rests = [rec[~over]], []
    o = rec[over]
    os0 = s0[over]
    for ch, p0 in sorted(set(zip(o['channel'].tolist(), os0.tolist()))):
        fr = o[(o['channel'] == ch) & (os0 == p0)]
        fr = fr[np.argsort(fr['record_i'])]
        data = np.concatenate([r['data'][:r['length']] for r in fr])
        k = max(cut - p0, 0)
        if k > 0:
            fronts.append(records_of_pulse(ch, p0, data[:k], dt))
        rests.append(records_of_pulse(ch, p0 + k, data[k:], dt))
    return sort_records(np.concatenate(fronts)), sort_records(np.concatenate(rests))


class OverlaySource:
    """config['overlay_records']: a time-sorted raw_records array, or a callable (t0_ns, t1_ns) -> the pulses that start in [t0, t1)
    with all their fragments"""

    def __init__(self, src):
        self.call = src if callable(src) else None
        if self.call is None:
            rec = np.ascontiguousarray(src)
            if rec.dtype != DTYPE or rec.ndim != 1:
                raise ValueError('overlay_records: an array of raw_records (dtypes.raw_record_dtype()) or a callable (t0_ns, t1_ns) -> records')
            if len(rec) > 1 and np.any(np.diff(rec['time']) < 0):
                raise ValueError('overlay_records: the records are not sorted by time')
            self.rec = rec
            start_ns = pulse_start(rec) * rec['dt'].astype(np.int64) if len(rec) else np.zeros(0, dtype=np.int64)
            self.order = np.argsort(start_ns, kind='stable')
            self.start_ns = start_ns[self.order]

    def take(self, t0, t1):
        """the records of the pulses that start in [t0, t1) ns, in (time, channel) order"""
        if self.call is not None:
            rec = np.ascontiguousarray(self.call(int(t0), int(t1)))
            if rec.dtype != DTYPE or rec.ndim != 1:
                raise ValueError('overlay_records: the callable must return an array of raw_records')
            return sort_records(rec)
        a, b = np.searchsorted(self.start_ns, [t0, t1], side='left')
        return sort_records(self.rec[np.sort(self.order[a:b])])


def pass_pulses(source, carry, t0, t1, cut, dt):
    """(records, carry) of one pass: the pulses of ``source`` that start in [t0, t1) ns and the carry of the pass before, cut at absolute
    sample ``cut`` (None: the last pass, nothing is cut); the new carry is what lies behind the cut, pulses of the next pass"""
    bg = source.take(t0, t1)
    if len(carry):
        bg = sort_records(np.concatenate([carry, bg]))
    if cut is None:
        return bg, bg[:0]
    return cut_pulses(bg, cut, dt)


def overlay_from(config, params, sharded=False):
    """(OverlaySource, baseline int32[n_rows] or None) of config['overlay_records'] / ['overlay_baseline'], or (None, None) without
    the key; raises ValueError where the overlay cannot be had"""
    src = config.get('overlay_records')
    if src is None:
        return None, None
    for key in ('dark_count_lone_hits', 'noise_lone_hits'):
        if config.get(key, False):
            raise ValueError(f'overlay_records: not together with {key} -- the recorded stream already holds what crosses a threshold between the windows')
    if sharded:
        raise ValueError('overlay_records: not under sharding (distributed.py): a pass hands the rest of a cut pulse to the next batch of its own run')
    dt = int(params['dt'])
    if int(params['rext']) // dt < 64:
        raise ValueError('overlay_records: right_raw_extension below 64 samples (the bound in front of which no later window begins)')
    base = config.get('overlay_baseline')
    if base is not None:
        n_rows = int(params['n_rows'])
        base = np.full(n_rows, int(base), dtype=np.int32) if np.ndim(base) == 0 else np.asarray(base).astype(np.int32)
        if np.ndim(config.get('overlay_baseline')) != 0:
            if len(base) > n_rows:
                raise ValueError(f'overlay_baseline: {len(base)} values, {n_rows} row slots')
            base = np.concatenate([base, np.full(n_rows - len(base), int(params['baseline']), dtype=np.int32)])
    return OverlaySource(src), base
