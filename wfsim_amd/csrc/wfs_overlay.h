// The rules of the overlay pass (wfs_overlay_records), each written once for host and device: what makes a stream of
// raw_records valid, the sort keys of its records, pulses and output records, when two pulses merge, and the sample of a merged pulse.
// Two streams: A, the simulation's, and B, the recorded background.  All of it is integer arithmetic on a few scalars.
//
// No HIP types: tests/host/overlay_rules_main.cpp compiles this header with the host compiler.
#pragma once
#include "wfs_rows.h"        // the record layout, records_of, rec_fragment_len

// ---- the header of a record as its six dwords hold it --------------------------------------------------------------------------------
struct OvHeader { i64 time; i32 length, dt, channel, pulse_length, record_i; };
WFS_HD OvHeader ov_header(const u32 *w)
{
    OvHeader q;
    q.time = (i64)(((u64)w[REC_TIME_HI] << 32) | (u64)w[REC_TIME_LO]);
    q.length = (i32)w[REC_LENGTH];
    q.dt = (i32)(int16_t)(w[REC_DT_CHANNEL] & 0xffffu); q.channel = (i32)(int16_t)(w[REC_DT_CHANNEL] >> 16);
    q.pulse_length = (i32)w[REC_PULSE_LENGTH];
    q.record_i = (i32)(int16_t)(w[REC_RECORD_I] & 0xffffu);
    return q;
}
// first sample of a fragment and of its pulse, last sample of its pulse (time is a multiple of dt: ov_record_check)
WFS_HD i64 ov_fragment_sample(const OvHeader &q) { return q.time / q.dt; }
WFS_HD i64 ov_pulse_sample(const OvHeader &q) { return ov_fragment_sample(q) - rec_fragment_first((i64)q.record_i); }
WFS_HD i64 ov_pulse_last(const OvHeader &q) { return ov_pulse_sample(q) + q.pulse_length - 1; }

// ---- validity ------------------------------------------------------------------------------------------------------------------------
// What is wrong with a record; 0: nothing.  The first six are decided by the record alone (ov_record_check), the others by a record and
// its predecessor on its channel in its own stream (ov_pair_check).
enum OvBad : int { OV_OK = 0, OV_BAD_DT, OV_BAD_TIME, OV_BAD_LENGTH, OV_BAD_CHANNEL, OV_BAD_FRAGMENT, OV_BAD_FRAGMENT_LENGTH,
                   OV_BAD_INCOMPLETE, OV_BAD_ORDER, OV_BAD_OVERLAP, OV_BAD_KINDS };
WFS_HD const char *ov_bad_name(int bad)
{
    switch (bad) {
    case OV_BAD_DT: return "dt differs from the configuration's";
    case OV_BAD_TIME: return "time is no multiple of dt";
    case OV_BAD_LENGTH: return "length outside 1 .. 110";
    case OV_BAD_CHANNEL: return "channel outside 0 .. n_rows - 1";
    case OV_BAD_FRAGMENT: return "record_i outside the fragments of pulse_length";
    case OV_BAD_FRAGMENT_LENGTH: return "length is not that of fragment record_i of pulse_length";
    case OV_BAD_INCOMPLETE: return "a fragment of its pulse is missing";
    case OV_BAD_ORDER: return "the fragments of its pulse are not 110 dt apart with one pulse_length";
    case OV_BAD_OVERLAP: return "its pulse shares a sample with another pulse of the stream on the channel";
    default: return "invalid";
    }
}
WFS_HD int ov_record_check(const OvHeader &q, i32 dt, i32 n_rows)
{
    if (q.dt != dt || dt <= 0) return OV_BAD_DT;
    if (q.time % dt != 0) return OV_BAD_TIME;
    if (q.length < 1 || q.length > WFS_SPR) return OV_BAD_LENGTH;
    if (q.channel < 0 || q.channel >= n_rows) return OV_BAD_CHANNEL;
    if (q.pulse_length < 1 || q.record_i < 0 || q.record_i >= records_of(q.pulse_length)) return OV_BAD_FRAGMENT;
    if (q.length != rec_fragment_len(q.pulse_length, q.record_i)) return OV_BAD_FRAGMENT_LENGTH;
    return OV_OK;
}
// A record that passed ov_record_check and the record in front of it in the order (stream, channel, time); has_prev false: it is the
// first of its stream and channel.  Every record passing this, and the last of every stream and channel passing ov_last_check, is
// the whole of validity: the pulses of a stream that do not share a sample appear fragment by fragment in that order.
WFS_HD int ov_pair_check(bool has_prev, const OvHeader &p, const OvHeader &q)
{
    if (q.record_i == 0) {
        if (!has_prev) return OV_OK;
        if (ov_pulse_last(p) >= ov_fragment_sample(q)) return OV_BAD_OVERLAP;
        return p.record_i != records_of(p.pulse_length) - 1 ? OV_BAD_INCOMPLETE : OV_OK;      // (of p's pulse; named at its successor)
    }
    if (!has_prev) return OV_BAD_INCOMPLETE;
    if (p.record_i == q.record_i - 1 && p.pulse_length == q.pulse_length && ov_fragment_sample(p) + WFS_SPR == ov_fragment_sample(q)) return OV_OK;
    // not its own predecessor: another pulse in between, or none in front of it
    if (ov_pulse_sample(p) == ov_pulse_sample(q) && p.pulse_length == q.pulse_length) return p.record_i == q.record_i ? OV_BAD_OVERLAP : OV_BAD_INCOMPLETE;
    if (ov_pulse_last(p) >= ov_pulse_sample(q) && ov_pulse_sample(p) <= ov_pulse_last(q)) return OV_BAD_OVERLAP;
    return ov_fragment_sample(p) + WFS_SPR == ov_fragment_sample(q) ? OV_BAD_ORDER : OV_BAD_INCOMPLETE;
}
WFS_HD int ov_last_check(const OvHeader &q) { return q.record_i == records_of(q.pulse_length) - 1 ? OV_OK : OV_BAD_INCOMPLETE; }

// ---- keys ----------------------------------------------------------------------------------------------------------------------------
// Times are int64 ns at epoch scale; every key holds a sample relative to smin, the smallest fragment start of the pass.
//   record key  stream | channel | sample      the order of the validity rule, and of the bisection of the fill kernel
//   pulse key   channel | sample | stream      the order in which pulses of both streams merge (A in front of B at one start)
//   output key  sample | channel               (time, channel), the order of the output
// sbits: bits of the largest relative sample (the end of the last pulse), chbits: bits of n_rows - 1
struct OvBits { int sbits, chbits; };
// the bits of a key field that holds the values up to v: one, and those of the values up to v >> 1 (bits_below of wfs_rows.h; no v overflows)
WFS_HD int ov_bits_of(u64 v) { return 1 + bits_below((v >> 1) + 1); }
WFS_HD bool ov_bits_fit(const OvBits &b) { return b.sbits + b.chbits + 1 <= 64; }
WFS_HD u64 ov_record_key(const OvBits &b, int stream, i32 channel, i64 rel) { return ((u64)stream << (b.sbits + b.chbits)) | ((u64)channel << b.sbits) | (u64)rel; }
WFS_HD u64 ov_pulse_key(const OvBits &b, int stream, i32 channel, i64 rel) { return ((((u64)channel << b.sbits) | (u64)rel) << 1) | (u64)stream; }
WFS_HD u64 ov_output_key(const OvBits &b, i32 channel, i64 rel) { return ((u64)rel << b.chbits) | (u64)channel; }
WFS_HD i64 ov_key_rel(const OvBits &b, u64 channel_rel) { return (i64)(channel_rel & ((1ull << b.sbits) - 1ull)); }
WFS_HD i32 ov_key_channel(const OvBits &b, u64 channel_rel) { return (i32)((channel_rel >> b.sbits) & ((1ull << b.chbits) - 1ull)); }
WFS_HD i64 ov_output_rel(const OvBits &b, u64 key) { return (i64)(key >> b.chbits); }
WFS_HD i32 ov_output_channel(const OvBits &b, u64 key) { return (i32)(key & ((1ull << b.chbits) - 1ull)); }

// ---- merging -------------------------------------------------------------------------------------------------------------------------
// Pulses of a channel in the order of their starts; run_last: the largest last sample of those in front.  A pulse that shares a sample
// with them belongs to their merged pulse; one that only touches (run_last + 1 == start) begins the next.  channel | last sample as
// one number makes the running maximum one plain maximum: a later channel outranks every end of an earlier one.
WFS_HD u64 ov_end_key(const OvBits &b, i32 channel, i64 last_rel) { return ((u64)channel << b.sbits) | (u64)last_rel; }
WFS_HD bool ov_begins_merged(u64 run_max_end_key, u64 pulse_key) { return run_max_end_key < (pulse_key >> 1); }

// ---- the sample ----------------------------------------------------------------------------------------------------------------------
// in_a, in_b: which streams cover the sample (at least one); a, b: their values; baseline: the simulation's (cfg.baseline); base: the
// recorded baseline of the channel
WFS_HD i32 ov_clamp(i32 v) { return v < 0 ? 0 : (v > 32767 ? 32767 : v); }
WFS_HD i32 ov_sample(bool in_a, bool in_b, i32 a, i32 b, i32 baseline, i32 base)
{
    if (!in_a) return b;
    return ov_clamp(in_b ? b + a - baseline : a - baseline + base);
}
