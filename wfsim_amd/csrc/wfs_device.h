// wfs_device.h -- device-side helpers of the MI355X WFSim hot path (gfx950 only).
//
// RNG: Philox4x32-10 (Salmon et al., SC'11), counter = (emitter, instruction gid, item, site), key = seed.
// The stream layout is specified in DESIGN.md "RNG streams" (spec v6: channel, delay and gain words of a photon come from
// three streams indexed by the photon's position P among its instruction's photons, four photons per call -- 0.75 calls
// per photon); the CPU oracle implements the same layout independently (oracle/wfsim_oracle.c) so that GPU and oracle
// results can be compared photon by photon.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wfs_noise.h"       // NoiseKind, the NC_ / NS_ constants of the coloured model and its slow levels
#include "wfs_dark.h"        // PMT dark counts: the definition, the cell and site constants
#include "wfs_layout.h"      // the sizes the LDS layouts are made of (WFS_DT, WFS_MAX_CH, SPE_ROW_LEN, ..), floordiv, the window rules
#include "wfs_rows.h"        // the rules of the back end of a row: ZLE intervals, records, the noise index, the finished sample
#include "wfs_lone.h"        // lone-hit rows: the rule, the site of a row's noise offset, the limits of a pass
#include "wfs_overlay.h"     // the overlay pass: validity of a record stream, its keys, merging, the sample of a merged pulse

typedef long long i64;
typedef unsigned long long u64;
typedef int i32;
typedef unsigned int u32;

#define WFS_MAX_AP 8

enum WfsSite : u32 {
    SITE_S1_HIT = 1, SITE_S2_SURVIVE = 2, SITE_EL_A = 3, SITE_EL_B = 4, SITE_EL_POIS = 5,
    SITE_EL_DIFF = 6,    // per electron (emitter, gid, 0): Box-Muller pair -> radial / azimuthal transverse diffusion (s2.py:588-589)
    // photon streams, counter (em_base, gid, P >> 2, site), P = index of the photon among its instruction's photons; photon P owns word P & 3
    SITE_DELAY = 16,     // -> summed delay (alias table)
    SITE_CH = 17,        // -> channel
    SITE_GAIN = 18,      // -> first SPE index, double-PE flag, second SPE index
    SITE_PH = 19,        // photons that arrive with time and channel (optical input), counter (0, gid, item): x -> transit time, y -> gains
    SITE_PH_X = 20,      // per photon (emitter, gid, item), S1 optical propagation only: x -> spline coordinate
    SITE_LUM = 21,       // photon stream (as SITE_DELAY): position on the excitation-time inverse CDF ('garfield_gas_gap' luminescence)
    // tile-local generation (spec v9, wfs_tilegen.h): counter (em_base + channel, gid, item, site)
    SITE_TILE_N = 24,    // photons of the tile: Poisson draw, item = iteration of the sampler
    SITE_TILE_E = 25,    // item = P >> 2 (P: photon of the tile), word P & 3 -> surviving electron
    SITE_TILE_DELAY = 26,    // -> summed delay (alias table)
    SITE_TILE_GAIN = 27,     // -> SPE indices and double-PE flag
    SITE_AP = 32, SITE_AP_SCREEN = 40, SITE_AP_X = 48, SITE_NOISE = 64,
    // digitiser noise drawn per sample (wfs_set_noise_model): counter (low, high 32 bits of t >> 2, channel, site), t = absolute sample
    // index; sample t owns word t & 3
    SITE_NOISE_SAMPLE = 65,
    // the common streams of the coloured model (wfs_set_noise_colour): the same counter with the group in place of the channel
    SITE_NOISE_COMMON = 66,
    // the slow levels of the model (wfs_set_noise_slow): level j of a channel at site 80 + j, of common stream g (in place of the
    // channel) at 96 + j, j < 8; counter (low, high 32 bits of m >> 2, ..), m the knot index t >> shift[j]; knot m owns word m & 3
    SITE_NOISE_SLOW = 80, SITE_NOISE_SLOW_COMMON = 96,
    // PMT dark counts (wfs_set_dark_counts, wfs_dark.h): counter (low, high 32 bits of the cell m, channel, site); 112: word 0 -> photons
    // of the cell; 113 + (j >> 1): words 2 (j & 1), 2 (j & 1) + 1 -> time and SPE index of photon j < 4 (113, 114)
    SITE_DARK_N = DK_SITE_COUNT, SITE_DARK_PH = DK_SITE_PHOTON,
    // lone-hit rows (wfs_lone_hits, wfs_lone.h): counter (low, high 32 bits of the row's first sample, channel, 115): word 0 -> ix_rand
    SITE_LONE_IX = DK_SITE_LONE_IX
};

struct u32x4 { u32 x, y, z, w; };
struct __attribute__((aligned(8))) PhotonRec { i32 t; u32 code; };   // one bucketed photon: ns relative to its set, SPE codes

__device__ __forceinline__ u32x4 philox4x32_10(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1)
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;     // one v_mad_u64_u32 each
        const u32 n0 = (u32)(p1 >> 32) ^ c1 ^ k0, n2 = (u32)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (u32)p1; c2 = n2; c3 = (u32)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return u32x4{c0, c1, c2, c3};
}

__device__ __forceinline__ double u53(u32 a, u32 b)
{
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}

__device__ __forceinline__ u64 bern_threshold(double p)
{
    if (!(p > 0)) return 0;
    if (p >= 1) return 4294967296ull;
    return (u64)(p * 4294967296.0);
}

// first variate only (the second one is not needed when its spread is zero: (i64)(0.0 + 0 * z) == 0)
__device__ __forceinline__ double box_muller_z0(u32x4 w)
{
    double u1 = u53(w.x, w.y), u2 = u53(w.z, w.w);
    double r = sqrt(-2.0 * log(1.0 - u1));
    return r * cos(6.283185307179586476925286766559 * u2);
}

__device__ __forceinline__ void box_muller(u32x4 w, double &z0, double &z1)
{
    double u1 = u53(w.x, w.y), u2 = u53(w.z, w.w);
    double r = sqrt(-2.0 * log(1.0 - u1));
    double a = 6.283185307179586476925286766559 * u2;
    double s, c;
    sincos(a, &s, &c);
    z0 = r * c; z1 = r * s;
}

// word k & 3 of a Philox call (k a lane's own: a select, no indexing)
__device__ __forceinline__ u32 word_of(const u32x4 &W, int k) { return k == 0 ? W.x : (k == 1 ? W.y : (k == 2 ? W.z : W.w)); }

// The Philox call that covers items 4 q .. 4 q + 3 (q = t >> 2, arithmetic shift) of a stream of the noise model: samples of
// (channel, SITE_NOISE_SAMPLE) or (group, SITE_NOISE_COMMON), knots of a slow level (.., SITE_NOISE_SLOW(_COMMON) + level)
__device__ __forceinline__ u32x4 noise_quad_of(u32 k0, u32 k1, u32 id, u32 site, i64 q)
{
    return philox4x32_10((u32)(u64)q, (u32)((u64)q >> 32), id, site, k0, k1);
}
// the white samples of a channel
__device__ __forceinline__ u32x4 noise_quad(u32 k0, u32 k1, i32 channel, i64 q) { return noise_quad_of(k0, k1, (u32)channel, SITE_NOISE_SAMPLE, q); }

// Integer-valued delays.  The reference draws float variates and truncates each to int64 before adding it (pulse.py:54-56
// transit time, s1.py:193-194, s2.py:338, pulse.py:339-341, s2.py:550); only the SUM reaches the pulse, and the sum of
// independent integer variates is one discrete variate whose probability mass function the host builds by convolution
// (wfs_engine.hip, build_time_tables).  It is sampled with Walker's alias method from ONE 32-bit word: K = 2^k >= n cells,
// cell c holds {thr, alias}; the word's top k bits pick the cell, the remaining bits (left aligned) are compared with thr.
// One 8-byte gather per photon (an inverse-CDF search needs a guide cell and three cumulative values: five gathers).
// The table is built by the same sequential algorithm on the host and in the CPU oracle.
struct AliasTab { const uint2 *cell; i32 vmin, shift; };      // shift = 32 - k

__device__ __forceinline__ u32 alias_cell(const AliasTab &t, u32 w) { return w >> t.shift; }
__device__ __forceinline__ i32 alias_pick(const AliasTab &t, u32 w, u32 c, uint2 e) { return t.vmin + (i32)(((w << (32 - t.shift)) < e.x) ? c : e.y); }
__device__ __forceinline__ i32 alias_sample(const AliasTab &t, u32 w) { const u32 c = alias_cell(t, w); return alias_pick(t, w, c, t.cell[c]); }
// two samples of an int16 range as one word for a cross-lane fetch: that of wa in the low half, that of wb in the high half
__device__ __forceinline__ u32 alias_pair(const AliasTab &t, u32 wa, u32 wb) { return ((u32)alias_sample(t, wa) & 0xffffu) | ((u32)alias_sample(t, wb) << 16); }

// A channel's SPE row (pulse.py:97: a photon's gain is entry int(u * SPE_BINS) + 1 of it): SPE_BINS quantiles behind an entry 0 that no
// photon indexes (SPE_ROW_LEN entries, wfs_layout.h).
// SPE indices and double-PE flag of a photon from ONE word (pulse.py:76-79, 97-103, 226): w * SPE_BINS = g * 2^32 + frac;
// g + 1 = int(u * SPE_BINS) + 1 is the first index; frac (the 32 low bits, equidistributed for every g) < thr is the double-PE
// Bernoulli trial, and given frac < thr it is uniform on [0, thr): int(frac * SPE_BINS / thr) + 1 is the second index.
// Returns g1 | g2 << 16 with g2 = 0 when the photon makes a single PE.
__device__ __forceinline__ u32 gain_code(u32 w, u64 thr_dpe, double dpe_inv)
{
    const u64 prod = (u64)w * (u32)SPE_BINS;
    const u32 g1 = (u32)(prod >> 32) + 1u, frac = (u32)prod;
    if (!((u64)frac < thr_dpe)) return g1;
    u32 g2 = (u32)((double)frac * dpe_inv) + 1u;
    g2 = g2 > (u32)SPE_BINS ? (u32)SPE_BINS : g2;
    return g1 | (g2 << 16);
}

// One term of Pulse.add_current (pulse.py:303-318): current += template * gain.  FMA = false: numpy's two roundings (the product,
// then the sum; the library is compiled with -ffp-contract=off, so the two stay apart) -- currents bit-exact with the reference.
// FMA = true (wfs_config.fma): one v_fma_f64, one rounding; half the f64 issue slots of every gather loop.
template <bool FMA> __device__ __forceinline__ double mac(double a, double b, double c)
{
    if constexpr (FMA) return __builtin_fma(a, b, c);
    else { const double prod = a * b; return c + prod; }
}

// Wave votes straight on the lane mask: HIP's __ballot / __any / __all take an int, which costs a v_cndmask (bool -> 0 / 1) and a v_cmp per
// vote on the vector unit; the builtin compares into the scalar mask directly.  (Votes are over the ACTIVE lanes, as the HIP ones.)
__device__ __forceinline__ u64 ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ bool any64(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }
__device__ __forceinline__ bool all64(bool p) { return __builtin_amdgcn_ballot_w64(!p) == 0ull; }

// Index of the wave inside its workgroup as a SCALAR: threadIdx.x >> 6 is the same in all 64 lanes but the compiler cannot know, and
// everything computed from it (row descriptors, base pointers, loop bounds of the wave-per-row kernels) would sit in vector
// registers and be recomputed by the vector unit; through readfirstlane it becomes SGPR work and scalar loads.
__device__ __forceinline__ int wave_in_block() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// Wave-wide reductions on the DPP path (quad permutes, half-row and row mirrors: VALU moves, no LDS crossbar round trips as with
// the shuffles; readlane joins the four 16-lane rows).  Every lane -- and the scalar result -- ends up with the value of all 64.
template <int CTRL> __device__ __forceinline__ int dpp_mov(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }
template <int CTRL> __device__ __forceinline__ double dpp_mov(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = dpp_mov<CTRL>((int)(u32)b), hi = dpp_mov<CTRL>((int)(u32)((u64)b >> 32));
    return __longlong_as_double((long long)(((u64)(u32)hi << 32) | (u32)lo));
}
// lane ^ J of the wave without a trip through the LDS crossbar where the hardware has a permute for it: quad permutes (J = 1, 2) and the
// rotation of a 16-lane row by 8 are DPP moves on the vector unit, J = 4 / 16 swizzles (LDS unit, no address register), J = 32 the
// generic shuffle.  All 64 lanes must be active (the callers sit in wave-uniform code).
template <int J> __device__ __forceinline__ u32 lane_xor(u32 v)
{
    if constexpr (J == 1) return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);          // quad_perm [1, 0, 3, 2]
    else if constexpr (J == 2) return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);     // quad_perm [2, 3, 0, 1]
    else if constexpr (J == 8) return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);    // row_ror:8
    else if constexpr (J == 4) return (u32)__builtin_amdgcn_ds_swizzle((int)v, 0x101F);                       // bit mode: and 0x1f, xor 4
    else if constexpr (J == 16) return (u32)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);                      // bit mode: and 0x1f, xor 16
    else return (u32)__shfl_xor((int)v, J, 64);
}
// one compare-exchange step of a bitonic network on keys held one per lane (ascending over the wave)
template <int K, int J> __device__ __forceinline__ u32 bitonic_step(u32 key, int lane)
{
    const u32 other = lane_xor<J>(key);
    const bool up = (lane & K) == 0, low = (lane & J) == 0;
    return (low == up) ? (key < other ? key : other) : (key > other ? key : other);
}
template <int K, int J = (K >> 1)> __device__ __forceinline__ u32 bitonic_merge(u32 key, int lane)
{
    key = bitonic_step<K, J>(key, lane);
    if constexpr (J > 1) return bitonic_merge<K, (J >> 1)>(key, lane);
    else return key;
}

// (every DPP move is made ONCE, by all lanes, before its value is used: inside a divergent region a DPP read of a switched-off
// lane returns the old value instead)
#define WFS_DPP_STEPS(T, COMBINE) \
    { const T o = dpp_mov<0xB1>(v); v = COMBINE; } { const T o = dpp_mov<0x4E>(v); v = COMBINE; } \
    { const T o = dpp_mov<0x141>(v); v = COMBINE; } { const T o = dpp_mov<0x140>(v); v = COMBINE; }
__device__ __forceinline__ int wave_sum(int v)
{
    WFS_DPP_STEPS(int, v + o)
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}
__device__ __forceinline__ int wave_min(int v)
{
    WFS_DPP_STEPS(int, min(v, o))
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ int wave_max(int v)
{
    WFS_DPP_STEPS(int, max(v, o))
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
// (a fixed order of additions: the result does not depend on anything but the 64 values)
__device__ __forceinline__ double wave_sum(double v)
{
    WFS_DPP_STEPS(double, v + o)
    const long long b = __double_as_longlong(v);
    const int lo = (int)(u32)b, hi = (int)(u32)((u64)b >> 32);
    double r[4];
#pragma unroll
    for (int q = 0; q < 4; q++) r[q] = __longlong_as_double((long long)(((u64)(u32)__builtin_amdgcn_readlane(hi, 16 * q) << 32) | (u32)__builtin_amdgcn_readlane(lo, 16 * q)));
    return (r[0] + r[1]) + (r[2] + r[3]);
}

// In-kernel phase stamps (diagnostic builds, -DWFS_STAMPS; MI355X_MICROARCH.md "In-kernel stamps"): thread 0 of every
// workgroup adds the shader cycles since its previous stamp to slot i.  Production builds compile them away.
#ifdef WFS_STAMPS
#define STAMP_INIT unsigned long long st_last_ = __builtin_amdgcn_s_memtime()
#define STAMP(d, i) do { if (threadIdx.x == 0 && (d).stamps) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
    unsigned long long *row_ = (d).stamps + (size_t)(blockIdx.x & 4095u) * 64; \
    atomicAdd(&row_[i], t_ - st_last_); atomicAdd(&row_[(i) + 32], 1ull); st_last_ = t_; } } while (0)
#define STAMP_WAIT() asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory")      // (charges the phase with the latency of what it issued)
#else
#define STAMP_INIT
#define STAMP(d, i)
#define STAMP_WAIT()
#endif

// python-style floor division / modulo on int64 (numpy // and % on int64, pulse.py:305-306)
__host__ __device__ __forceinline__ i64 floormod(i64 a, i64 b) { i64 m = a % b; return (m != 0 && ((m < 0) != (b < 0))) ? m + b : m; }

// A lane of k_zle reads 4 consecutive noise samples from any start below noise_len: every channel row of the device copy is
// followed by its own first NOISE_PAD samples, so the read never meets the wrap (rawdata.py:433-434 indexes modulo noise_len).
// (WFS_SPR, WFS_RECORD_BYTES and NOISE_MIN_FAST: wfs_rows.h)
constexpr int NOISE_PAD = 4;

// The device scalar block: counters that kernels bump with atomics, totals that the scans write, the error code, the origin of
// the record sort keys.  wfs_run clears it at the start of a batch; the host copies it back (read_scal) and sizes the next stage
// from it.  One member per 64-bit slot.  The layout is frozen: the tile-list counters were placed with their cache line in mind
// (tile_list_append, wfs_kernels.h), so a new member takes a reserved slot and nothing moves.
enum WfsDevError : i64 {            // raised with atomicMax (the highest code wins), decoded by device_error() on the host
    // WfsScal::error
    WFS_DEV_WINDOW = 1,             // digitise window of 10^6 samples or more; tile buffers of one instruction beyond 2^31 samples
    WFS_DEV_TIME_RANGE = 2,         // a photon or electron time does not fit 32 bits relative to its origin
    WFS_DEV_TILE_BUFFER = 3,        // internal: a tile of k_s2_tile did not fit its sample buffer
    // WfsScal::opt_error (k_optical_bucket)
    WFS_DEV_OPT_CHANNEL = 4,        // photon channel out of range
    WFS_DEV_OPT_TIME = 5            // photon time beyond 2^31 ns
};
struct WfsScal {
    i64 n_groups;           // digitise windows.  k_groups -> k_group_final, k_row_len, host
    i64 error;              // WfsDevError.  generator, geometry and tile kernels -> host after the geometry (device_error)
    i64 n_front_rows;       // rows of the accumulator path (k_zle / k_pack).  k_row_len -> host
    i64 n_sparse_tiles;     // sparse work list.  tile_list_append -> host
    i64 max_nb_sparse;      // most start bins of a sparse tile.  tile_list_append -> host (LDS of k_pulse_sparse)
    i64 max_ph_sparse;      // most photons of a sparse tile.  tile_list_append -> host (LDS of k_pulse_sparse)
    i64 n_block_photons;    // photons of the block generator.  scan of em_nph -> host
    i64 n_tile_photons;     // photons in tile_off.  scan of tile_count -> host (wfs_load_optical)
    i64 n_acc_samples;      // samples of the row accumulators.  scan of acc_len -> host
    i64 n_itv_slots;        // reserved ZLE interval slots.  scan of itv_cap -> host
    i64 n_records;          // records of the batch.  scan of row_nrec -> host
    i64 n_dense_tiles;      // dense work list.  tile_list_append -> host
    i64 max_nb_dense;       // most start bins of a dense tile.  tile_list_append -> host (variant of k_pulse)
    i64 n_ap_candidates;    // PMT afterpulse candidates in the list (ApArgs::count).  ap_park, k_photon_fill, k_s2_tile -> afterpulse kernels, host (capacity check)
    i64 n_ap_photons;       // accepted afterpulse photons.  scan of the afterpulse tiles' tile_count -> host
    i64 max_ph_dense;       // most photons of a dense tile.  tile_list_append -> host (variant of k_pulse)
    i64 n_tiny_tiles;       // tiny work list.  tile_list_append -> host
    i64 n_wave_tiles;       // wave (medium) work list.  tile_list_append -> host
    i64 opt_error;          // WfsDevError of the optical input.  k_optical_bucket -> wfs_load_optical (between its own memset and read_scal)
    i64 n_order_huge;       // generation-order ranges beyond TILE_ORDER_MAX photons.  k_tile_order_scan -> host
    i64 n_intervals;        // ZLE intervals of the batch.  k_counts -> wfs_get_counts
    i64 n_pe;               // PE of the primary pulse sets.  k_counts -> wfs_get_counts
    i64 key_origin;         // first sample of the batch, origin of the record sort keys.  host fill, k_row_desc -> k_rec_keys, host
    i64 n_tbuf_samples;     // samples of all tile buffers.  scan of ins_bcap_all -> host
    i64 n_tilegen_photons;  // photons of the tile-generated instructions.  k_tile_counts -> host
    i64 n_full_tiles;       // tiles of k_s2_tile, listed from the front of FuseArgs::tiles.  k_tile_counts -> host
    i64 n_direct_samples;   // samples of the rows read from a tile buffer in place.  k_row_len -> host
    i64 n_shared_rows;      // rows that several tiles of k_s2_tile share (k_tile_add is needed).  k_row_len -> host
    i64 n_gen_tiles;        // generation-only tiles, listed from the back of FuseArgs::tiles.  k_tile_counts -> host
    i64 key_end;            // end of the last row of the batch, span of the record sort keys.  host fill, k_row_desc -> host
    i64 n_order_wave;       // generation-order ranges on the wave list.  k_tile_order_scan -> host
    i64 n_order_big;        // generation-order ranges on the workgroup list.  k_tile_order_scan -> host
    i64 n_short_rows;       // resident rows of at most RES_SHORT_LEN samples.  k_row_len -> host
    i64 max_res_len;        // longest resident row.  k_row_len -> host (LDS of k_row_pulse)
    i64 n_fin_samples;      // finished int16 samples of the resident rows.  scan of fin_len -> host
    i64 n_res_tiles;        // tiles of the resident rows.  scan of res_cnt -> host
    i64 n_res_samples;      // samples of the resident rows.  k_row_len -> host (wfs_get_counts)
    i64 n_long_rows;        // resident rows longer than RES_SHORT_LEN.  k_row_len -> host
    i64 n_bright_tiles;     // tiles of k_s2_bright, listed from FuseArgs::tiles[n_list].  k_tile_counts -> host
    i64 max_bright_bins;    // most start bins the H table of a tile above TILE_MAX_PHOTONS could need, whichever kernel takes it.  k_tile_counts -> host (WFS_BRIGHT_STATS)
    i64 n_sum_samples;      // samples of the bottom-array sum rows (wfs_set_sum_signal).  scan of sum_len -> host
    i64 n_sum_chunks;       // workgroups of k_sum_signal.  scan of sum_nchunk -> host
    i64 n_empty_rows;       // rows without a pulse of a fully read-out window (wfs_set_full_readout).  k_row_len -> host
    i64 n_empty_samples;    // finished int16 samples reserved for them.  scan of fr_len -> host
    // a pass of wfs_lone_hits counts in a block of its own (wfs_handle::lone_scal), never in the run's: these, n_itv_slots, n_records,
    // n_empty_samples and the key range mean there what they mean for a batch
    i64 n_lone_seeds;       // seeds k_lone_scan and k_lone_noise_scan appended (may exceed the list: the pass is repeated with room).  the scans -> host
    i64 n_lone_rows;        // lone rows of the pass.  scan of the chain-start flags -> host
    i64 lone_error;         // 1: a lone row longer than LONE_MAX_ROW_LEN.  k_lone_rows -> host
    i64 reserved_[17];
};
static_assert(sizeof(WfsScal) == 512, "WfsScal: 64 slots of 8 bytes");
#define WFS_SCAL_SLOT(m, slot) static_assert(offsetof(WfsScal, m) == 8 * (slot), "WfsScal::" #m " moved: the layout is frozen")
WFS_SCAL_SLOT(error, 1); WFS_SCAL_SLOT(n_front_rows, 2); WFS_SCAL_SLOT(n_sparse_tiles, 3); WFS_SCAL_SLOT(n_dense_tiles, 11);
WFS_SCAL_SLOT(n_tiny_tiles, 16); WFS_SCAL_SLOT(n_wave_tiles, 17); WFS_SCAL_SLOT(key_origin, 22); WFS_SCAL_SLOT(key_end, 29);
WFS_SCAL_SLOT(n_ap_candidates, 13); WFS_SCAL_SLOT(n_order_huge, 19); WFS_SCAL_SLOT(n_long_rows, 37); WFS_SCAL_SLOT(n_bright_tiles, 38);
#undef WFS_SCAL_SLOT

// Everything a kernel needs, passed by value (fits the kernarg segment).
struct WfsDev {
    // scalars (wfs_config)
    i32 dt, samples_before, samples_after, store_before, store_after, tlen, tw, baseline, n_rows;
    i32 n_tpc, n_top, he_first, he_factor, last_bottom, detector_nt, enable_noise, s1_simple, s2_time_model, enable_pmt_ap;
    i32 n_spe, n_lum, noise_len, noise_channels, n_ap, he_rows /* HE rows materialised */, row_slots /* per group */;
    i32 noise_stride;                          // samples between the noise rows of two channels: noise_len + NOISE_PAD, the pad repeats the row's start
    i32 sum_channel;                           // channel of the bottom-array sum row, the last of a window's row_slots (wfs_set_sum_signal); -1: no such row
    i32 full_readout;                          // every TPC and HE row slot of a digitise window has a row of the window's range (wfs_set_full_readout)
    double c2a, tts_mean, tts_sigma, p_dpe, s1_decay_time, s1_decay_spread, sf_gas, t1_gas, t3_gas, s2_time_spread;
    double trap_time, gain_spread, pmt_ap_modifier, pmt_ap_t_modifier, rext;
    u32 k0, k1;
    unsigned long long *stamps;                // -DWFS_STAMPS builds only: per-phase cycle sums of the instrumented kernels (nullptr otherwise)
    u64 thr_dpe;                               // Bernoulli threshold on a 32-bit word: floor(p * 2^32)
    double dpe_inv;                            // SPE_BINS / thr_dpe
    double current_max[16];                    // pulse.py:32, per ns remainder (sample_duration <= 16 ns)
    AliasTab tab_tts, tab_s1, tab_s2;          // alias tables of integer delays: transit time alone, all terms of an S1 / S2 photon
    // tables
    const double *templates, *spe, *gains, *thr_truth, *lum_x, *lum_t;
    const i64 *thr_zle;
    const int16_t *noise;
    const double *noise_f;       // a float noise array (wfs_set_noise_float): the sum is stored truncated (rawdata.py:436 into an int64 row)
    // the noise model (wfs_set_noise_model): alias cells [channel][nm_cells_per_ch] of the channels' ADC distributions, nullptr without a
    // model; noise_channels then counts the model's channels and the table above is not read
    const uint2 *nm_cells;
    i32 nm_cells_per_ch, nm_shift, nm_vmin;
    // the colour of the model (wfs_set_noise_colour, noise kind 4): nc_taps [noise_channels + nc_groups][NC_TAP_STRIDE], nullptr without a
    // colour; the cells of common stream g are row noise_channels + g of nm_cells; group (-1: none) and Q16 gain per channel
    const i32 *nc_taps, *nc_group, *nc_mix;
    i32 nc_n_taps, nc_groups;
    // the slow levels of the model (wfs_set_noise_slow, noise kind 5): ns_shift [NS_MAX_LEVELS], nullptr without levels; Q16 amplitudes
    // ns_amp [noise_channels + nc_groups][NS_MAX_LEVELS].  With levels nc_taps is never null: a model without a colour gets unit taps
    const i32 *ns_shift, *ns_amp;
    i32 ns_levels;
    // PMT dark counts (wfs_set_dark_counts): dk_thr [dk_channels][DK_MAX], floor(2^32 P(N >= k)) of a cell's Poisson count, nullptr: off
    i32 dk_channels;
    const u32 *dk_thr;
};
