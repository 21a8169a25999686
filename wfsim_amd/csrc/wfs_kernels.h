// wfs_kernels.h -- HIP kernels of the MI355X WFSim hot path (gfx950).  Included once by wfs_engine.hip.
//
// Data layout in HBM (one batch):
//   pulse set   = one Pulse.__call__ of the reference (one S1 or S2 instruction, or its PMT afterpulses)
//   tile        = (pulse set, channel): the photons of one pulse in one PMT; tile id = set * n_tpc + channel
//   photons     = bucketed by tile: 8-byte records {t i32 (ns relative to the set's t0), code u32 (SPE table indices
//                 g1 | g2 << 16, g2 = 0: no double-PE)}; ph_gain f64 only for pre-assigned gains
//   group       = digitise window (one digitize_pulse_cache call): clusters merged by the rule of rawdata.py:96-98
//   row         = (group, channel) active range [row_lo - tw, row_hi + tw]; int32 accumulators in one arena
//   intervals   = ZLE output per row, reserved slots; records = 244-byte strax raw_records
#pragma once
#include "wfs_device.h"
#include "wfs_family.h"      // the family of a template kernel that is declared beside it (k_lone_noise_scan)
#include <cstddef>

#define I64_MAX 0x7fffffffffffffffLL
#define I64_MIN (-I64_MAX - 1)

// ------------------------------------------------------------------------------------------------ fills
// The fills of one stage in one dispatch (FillGroup, wfs_engine.hip).  A segment is [p, p + bytes) and a pattern of 16 bytes that
// repeats from p: byte fills, one i32, one i64 and the (I64_MAX, I64_MIN) pairs of el_minmax are all of that form.
#define FILL_GROUP_MAX 16
struct FillSeg { unsigned char *p; u64 bytes; u32 pat[4]; };
struct FillSegs { FillSeg s[FILL_GROUP_MAX]; };
// blockIdx.y: the segment; blockIdx.x walks it with a grid stride.  16-byte stores where p is 16-byte aligned (every DevBuf is),
// the tail -- or a segment at an odd address, the two sort-key slots of the scalar block -- byte by byte.
__global__ void __launch_bounds__(256) k_fill_group(const FillSegs a)
{
    const FillSeg &s = a.s[blockIdx.y];
    const u64 stride = (u64)gridDim.x * blockDim.x, first = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 n16 = (((u64)s.p & 15) == 0) ? s.bytes >> 4 : 0;
    const uint4 v = make_uint4(s.pat[0], s.pat[1], s.pat[2], s.pat[3]);
    for (u64 i = first; i < n16; i += stride) ((uint4 *)s.p)[i] = v;
    for (u64 i = (n16 << 4) + first; i < s.bytes; i += stride) {
        const u32 k = (u32)(i >> 2) & 3, w = k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w));
        s.p[i] = (unsigned char)(w >> (8 * ((u32)i & 3)));
    }
}

// A step boundary (read_scal): the scalar block into the host's mapped copy, then the sequence word behind it.  One wave, one
// 8-byte store per lane; the fence orders every lane's store before the barrier, lane 0's release store publishes them.
__global__ void __launch_bounds__(64) k_publish(const WfsScal *scal, WfsScal *host, u64 *host_seq, u64 seq)
{
    static_assert(sizeof(WfsScal) == 64 * 8, "k_publish: one 8-byte slot per lane");
    ((i64 *)host)[threadIdx.x] = ((const i64 *)scal)[threadIdx.x];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(host_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// totals for wfs_get_counts, reduced on the device (copying itv_n back cost 300 MB per 10^5-cluster batch):
// n_intervals = sum of itv_n (ZLE intervals), n_pe = sum of the per-set n_pe (truth[s][1], integral doubles)
__global__ void k_counts(const i32 *itv_n, i64 n_itv, const double *truth, i64 n_sets, WfsScal *scal)
{
    i64 a = 0, b = 0;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n_itv; i += (i64)gridDim.x * blockDim.x) a += itv_n[i];
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n_sets; i += (i64)gridDim.x * blockDim.x) b += (i64)(truth[i * 16 + 1] + 0.5);
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); b += __shfl_down(b, o, 64); }
    if ((threadIdx.x & 63) == 0) { if (a) atomicAdd((unsigned long long *)&scal->n_intervals, (unsigned long long)a); if (b) atomicAdd((unsigned long long *)&scal->n_pe, (unsigned long long)b); }
}

// ------------------------------------------------------------------------------------------------ scan
// exclusive scan i32[n] -> i64[n+1] in three launches (reduce / spine / down-sweep); 4096 items per block
#define SCAN_TPB 256
#define SCAN_IPT 16
#define SCAN_TILE (SCAN_TPB * SCAN_IPT)

__device__ __forceinline__ i64 block_reduce_sum(i64 v, i64 *sh)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[w] = v;
    __syncthreads();
    i64 r = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) r += sh[i];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(SCAN_TPB) void k_scan_reduce(const i32 *__restrict__ in, i64 n, i64 *__restrict__ block_sums)
{
    __shared__ i64 sh[SCAN_TPB / 64];
    i64 base = (i64)blockIdx.x * SCAN_TILE;
    i64 s = 0;
    // (branch-free loads: behind `if (i < n)` every load is waited for before the next is issued)
    i32 x[SCAN_IPT];
#pragma unroll
    for (int k = 0; k < SCAN_IPT; k++) { const i64 i = base + (i64)k * SCAN_TPB + threadIdx.x; x[k] = in[i < n ? i : 0]; }
#pragma unroll
    for (int k = 0; k < SCAN_IPT; k++) { const i64 i = base + (i64)k * SCAN_TPB + threadIdx.x; s += i < n ? x[k] : 0; }
    s = block_reduce_sum(s, sh);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = s;
}

__global__ __launch_bounds__(1024) void k_scan_spine(i64 *__restrict__ block_sums, i64 nb, i64 *__restrict__ total)
{
    __shared__ i64 sh[1024];
    __shared__ i64 carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (i64 base = 0; base < nb; base += 1024) {
        i64 i = base + threadIdx.x;
        i64 v = i < nb ? block_sums[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            i64 t = threadIdx.x >= (unsigned)o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nb) block_sums[i] = carry + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(SCAN_TPB) void k_scan_down(const i32 *__restrict__ in, i64 n, const i64 *__restrict__ block_sums,
                                                        i64 *__restrict__ out, i64 offset)
{
    __shared__ i64 sh[SCAN_TPB];
    i64 base = (i64)blockIdx.x * SCAN_TILE + (i64)threadIdx.x * SCAN_IPT;
    i64 v[SCAN_IPT], s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_IPT; k++) { const i64 i = base + k; v[k] = in[i < n ? i : 0]; }
#pragma unroll
    for (int k = 0; k < SCAN_IPT; k++) { if (base + k >= n) v[k] = 0; s += v[k]; }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < SCAN_TPB; o <<= 1) {
        i64 t = threadIdx.x >= (unsigned)o ? sh[threadIdx.x - o] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    i64 run = offset + block_sums[blockIdx.x] + sh[threadIdx.x] - s;
#pragma unroll
    for (int k = 0; k < SCAN_IPT; k++) { i64 i = base + k; if (i < n) out[i] = run; run += v[k]; if (i == n - 1) out[n] = run; }
}

// ------------------------------------------------------------------------------------------------ geometry
struct GeomArgs {
    i64 n_sets, n_tiles, n_clusters;
    i64 n_gslots;        // capacity of the per-group arrays: n_clusters + 1 (a carried-in window can open group 1 at cluster 0)
    const i32 *tile_count, *tile_tmin, *tile_tmax;
    const i32 *set_cluster; const i64 *set_t0;
    const i64 *cl_tmin; const u32 *cl_gid;
    i64 *cl_end; i32 *cl_group;
    i64 *grp_lo, *grp_hi, *grp_left, *grp_right, *grp_ixrand; u32 *grp_gid;
    i64 *row_lo, *row_hi;
    i32 *acc_len, *itv_cap; i32 *active_rows;
    WfsScal *scal;       // the device scalar block (wfs_device.h)
    i32 *active_tiles;   // tiny tiles (thread per tile); the other two lists are copied behind them by the host side
    i32 *sparse_tiles;   // sparse-class tiles (few photons per start bin: sorted-list kernel)
    i32 *dense_tiles;    // everything else (dense H-table kernel, windows over time)
    i32 *wave_tiles;     // medium tiles (at most 64 photons, any width: wave per tile); scal->n_wave_tiles = their number
    const i32 *tile_done;       // [n_done] 1: the tile's pulse was made by k_s2_tile (wfs_tilegen.h): on no work list (or nullptr)
    i64 n_done;                 // primary tiles (the tiles of the afterpulse sets, which follow them, are never done)
    i32 *row_cnt, *row_tile;    // [groups * n_tpc] tiles in the row; one of them
    const i32 *ins_bcap; const i64 *ins_boff;      // tile sample buffers (wfs_tilegen.h)
    // resident rows (k_row_pulse): rows no longer than res_max_len whose tiles all fit a wave are made, finished and zero-suppressed by
    // ONE wave in LDS; their tiles are on no work list but in a per-row list (res_toff: row -> first entry of res_desc)
    i32 res_on, res_max_len;
    i32 *row_bad;               // [groups * n_tpc] 1: the row holds a tile that needs one of the tile kernels
    i32 *fin_len, *res_cnt;     // [groups * n_tpc] finished int16 samples reserved for a resident row (a multiple of 4) / its tiles
    const i64 *res_toff;        // exclusive scan of res_cnt
    struct TileDesc *res_desc;  // [resident tiles] descriptors in row order (k_tile_assign)
    i64 rows_cap;               // capacity of active_rows: resident rows of at most RES_SHORT_LEN samples are appended from its end backwards,
    i32 *res_long;              // the longer ones to this list (two launches of k_row_pulse: its LDS goes with the longest row)
    i32 force_dense;     // debug: send every tile to the dense kernel
    i32 init_has; i64 init_runmax;      // last_pulse_end_time carried in from earlier batches
    const i64 *noise_override; i64 n_noise_override;
    // the bottom-array sum row of every window (wfs_set_sum_signal; nullptr when the switch is off): union of the bottom rows' ranges,
    // its length and its chunks for k_sum_signal
    i64 *sum_lo, *sum_hi; i32 *sum_len, *sum_nchunk;
    // full readout (wfs_set_full_readout; nullptr when the switch is off): finished int16 samples reserved for a row without a pulse
    // [groups * row_slots], and the list of those rows
    i32 *fr_len, *empty_rows;
};

// (SPARSE_MAX_PHOTONS, SPARSE_MAX_BINS, the class of the sorted-list kernel, and RES_SHORT_LEN: wfs_layout.h, which sizes LDS by them)
#define TINY_MAX_PHOTONS 4        // tiles of a few photons in a few start bins (the bulk of an S1): one THREAD per tile
#define TINY_MAX_BINS 32
#define TINY_LANES 16              // lanes that share the samples of one tiny tile (k_pulse_tiny)
#define WAVE_MAX_PHOTONS 64        // medium tiles: photons fit the lanes of one wave (any width): k_pulse_wave
#define WAVE_MAX_BINS 16384
#define RES_MAX_TILE_VISITS 256      // a resident row longer than the LDS of its wave: tiles x segments it may cost

// work lists and maxima: aggregated per workgroup in LDS, then one global atomic per workgroup and counter
// (76k wave-level atomics on one cache line cost ~3 ms; the counters all live in the same line of WfsScal)
__device__ __forceinline__ void tile_list_append(const GeomArgs &a, bool listed, int cls, i64 nb, i32 cnt, i64 tile)
{
    __shared__ i32 s_n[4]; __shared__ i64 s_b[4], s_mx[4];
    if (threadIdx.x == 0) { s_n[0] = 0; s_n[1] = 0; s_n[2] = 0; s_n[3] = 0; s_mx[0] = 0; s_mx[1] = 0; s_mx[2] = 0; s_mx[3] = 0; }
    __syncthreads();
    i32 rk = 0;
    if (listed) {
        rk = atomicAdd(&s_n[cls], 1);
        if (cls == 1) { atomicMax(&s_mx[0], nb); atomicMax(&s_mx[1], (i64)cnt); } else if (cls == 2) { atomicMax(&s_mx[2], nb); atomicMax(&s_mx[3], (i64)cnt); }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        s_b[0] = s_n[0] ? (i64)atomicAdd((u64 *)&a.scal->n_tiny_tiles, (u64)s_n[0]) : 0;
        s_b[1] = s_n[1] ? (i64)atomicAdd((u64 *)&a.scal->n_sparse_tiles, (u64)s_n[1]) : 0;
        s_b[2] = s_n[2] ? (i64)atomicAdd((u64 *)&a.scal->n_dense_tiles, (u64)s_n[2]) : 0;
        s_b[3] = s_n[3] ? (i64)atomicAdd((u64 *)&a.scal->n_wave_tiles, (u64)s_n[3]) : 0;
        if (s_mx[0]) atomicMax(&a.scal->max_nb_sparse, s_mx[0]);
        if (s_mx[1]) atomicMax(&a.scal->max_ph_sparse, s_mx[1]);
        if (s_mx[2]) atomicMax(&a.scal->max_nb_dense, s_mx[2]);
        if (s_mx[3]) atomicMax(&a.scal->max_ph_dense, s_mx[3]);
    }
    __syncthreads();
    if (listed) (cls == 0 ? a.active_tiles : (cls == 1 ? a.sparse_tiles : (cls == 2 ? a.dense_tiles : a.wave_tiles)))[s_b[cls] + rk] = (i32)tile;
}

__device__ __forceinline__ int tile_class(const GeomArgs &a, i32 cnt, i64 nb)      // 0 tiny, 1 sparse, 2 dense, 3 wave (medium)
{
    if (a.force_dense) return 2;
    return (cnt <= TINY_MAX_PHOTONS && nb <= TINY_MAX_BINS) ? 0 : ((cnt <= SPARSE_MAX_PHOTONS && nb <= SPARSE_MAX_BINS) ? 1
           : ((cnt <= WAVE_MAX_PHOTONS && nb <= WAVE_MAX_BINS) ? 3 : 2));
}

// per tile: end time of its pulse -> cluster (rawdata.py:188-190); work lists of non-empty tiles.
// List appends and the two maxima are aggregated per wave (one atomic per wave instead of one per tile).
__global__ void k_tile_geom(WfsDev d, GeomArgs a)
{
    const i64 tile = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = tile < a.n_tiles && a.tile_count[tile] > 0;
    int cls = 2; i64 nb = 0; i32 cnt = 0; i32 cl = -1; i64 end = I64_MIN;      // class 0 tiny, 1 sparse, 2 dense, 3 wave (medium)
    if (live) {
        const i64 set = tile / d.n_tpc;
        const TileWindow w = tile_window(d, a.set_t0[set], a.tile_tmin[tile], a.tile_tmax[tile]);
        nb = w.nb;
        cl = a.set_cluster[set]; end = w.right * d.dt;
        cnt = a.tile_count[tile];
        cls = tile_class(a, cnt, nb);
        if (a.tile_done && tile < a.n_done && a.tile_done[tile]) cls = -1;      // its pulse exists already (k_s2_tile): no work list
    }
    {   // cluster end time: the live lanes of a wave usually belong to one cluster -> one atomic for the wave
        const u64 ml = ballot64(live);
        if (ml) {
            const i32 cl0 = __shfl(cl, __ffsll((long long)ml) - 1, 64);
            if (all64(!live || cl == cl0)) {
                i64 e = end;
                for (int o = 32; o > 0; o >>= 1) { const i64 x = __shfl_down(e, o, 64); e = x > e ? x : e; }
                if (lane == 0) atomicMax(&a.cl_end[cl0], e);
            } else if (live) atomicMax(&a.cl_end[cl], end);
        }
    }
    if (!a.res_on) tile_list_append(a, live && cls >= 0, cls, nb, cnt, tile);      // (resident rows on: k_tile_assign makes the lists, once the rows are known)
}

// Digitise groups.  The cache is digitised before cluster k when min(instruction key of k) - last_pulse_end_time > rext
// and a pulse exists (rawdata.py:96-98); last_pulse_end_time is a running maximum over everything simulated so far
// (rawdata.py:188-190).  One workgroup: exclusive running maximum of the cluster end times, then a prefix sum of the flags.
#define GROUPS_TPB 1024
__global__ __launch_bounds__(GROUPS_TPB) void k_groups(WfsDev d, GeomArgs a)
{
    __shared__ i64 smax[GROUPS_TPB]; __shared__ i32 shas[GROUPS_TPB]; __shared__ i32 ssum[GROUPS_TPB];
    const int tid = threadIdx.x;
    const i64 C = a.n_clusters, per = (C + GROUPS_TPB - 1) / GROUPS_TPB;
    const i64 k0 = tid * per, k1 = (k0 + per < C) ? k0 + per : C;
    // 1) per-thread maximum of its clusters' end times
    i64 m = I64_MIN; i32 hs = 0;
    for (i64 k = k0; k < k1; k++) { const i64 e = a.cl_end[k]; if (e != I64_MIN) { m = hs ? (e > m ? e : m) : e; hs = 1; } }
    smax[tid] = m; shas[tid] = hs;
    __syncthreads();
    // 2) exclusive running maximum over threads (plus the carry from earlier batches)
    for (int o = 1; o < GROUPS_TPB; o <<= 1) {
        i64 pm = I64_MIN; i32 ph = 0;
        if (tid >= o) { pm = smax[tid - o]; ph = shas[tid - o]; }
        __syncthreads();
        if (ph) { smax[tid] = shas[tid] ? (pm > smax[tid] ? pm : smax[tid]) : pm; shas[tid] = 1; }
        __syncthreads();
    }
    i64 run = a.init_runmax; i32 has = a.init_has;
    if (tid > 0 && shas[tid - 1]) { const i64 pm = smax[tid - 1]; run = has ? (pm > run ? pm : run) : pm; has = 1; }
    // 3) flags of my clusters, sequentially inside the thread
    i32 nflag = 0;
    {
        i64 r = run; i32 h = has;
        for (i64 k = k0; k < k1; k++) {
            if (h && (double)(a.cl_tmin[k] - r) > d.rext) nflag++;
            const i64 e = a.cl_end[k];
            if (e != I64_MIN) { r = h ? (e > r ? e : r) : e; h = 1; }
        }
    }
    ssum[tid] = nflag;
    __syncthreads();
    for (int o = 1; o < GROUPS_TPB; o <<= 1) {
        i32 t = tid >= o ? ssum[tid - o] : 0;
        __syncthreads();
        ssum[tid] += t;
        __syncthreads();
    }
    // 4) group of every cluster; the first cluster of a group that made a pulse names its noise stream (grp_gid holds its
    //    index here; clusters without pulses must not matter, or the stream would depend on how a run is cut into batches)
    i32 g = ssum[tid] - nflag;
    {
        i64 r = run; i32 h = has;
        for (i64 k = k0; k < k1; k++) {
            const bool flag = h && (double)(a.cl_tmin[k] - r) > d.rext;
            if (flag) g++;
            a.cl_group[k] = g;
            const i64 e = a.cl_end[k];
            if (e != I64_MIN) { atomicMin(&a.grp_gid[g], (u32)k); r = h ? (e > r ? e : r) : e; h = 1; }     // first cluster of the group with a pulse
        }
    }
    if (tid == GROUPS_TPB - 1) a.scal->n_groups = ssum[tid] + 1;
}

__global__ void k_tile_rows(WfsDev d, GeomArgs a)
{
    i64 tile = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = tile < a.n_tiles && a.tile_count[tile] > 0;
    i64 left = I64_MAX, right = I64_MIN, g = -1; bool bottom = false;
    if (live) {
        i64 set = tile / d.n_tpc; i32 ch = (i32)(tile - set * d.n_tpc);
        const TileWindow w = tile_window(d, a.set_t0[set], a.tile_tmin[tile], a.tile_tmax[tile]);
        left = w.left; right = w.right; const i64 nb = w.nb;
        g = a.cl_group[a.set_cluster[set]];
        bottom = a.sum_lo && ch >= d.n_top && ch <= d.last_bottom;      // the row feeds the window's sum row (rawdata.py:250-254)
        atomicMin(&a.row_lo[g * d.n_tpc + ch], left); atomicMax(&a.row_hi[g * d.n_tpc + ch], right);
        if (a.row_cnt) { atomicAdd(&a.row_cnt[g * d.n_tpc + ch], 1); a.row_tile[g * d.n_tpc + ch] = (i32)tile; }      // (row_tile: only read when the row has ONE tile)
        if (a.res_on) {         // a tile of more than a wave's photons, or one whose pulse exists already, keeps its row off the resident path
            const bool done = a.tile_done && tile < a.n_done && a.tile_done[tile];
            // (so does the sum row: k_sum_signal adds up rows before they are finished, and a resident row only ever exists finished)
            if (done || a.tile_count[tile] > WAVE_MAX_PHOTONS || nb > WAVE_MAX_BINS || bottom) a.row_bad[g * d.n_tpc + ch] = 1;
        }
    }
    const i64 bl0 = bottom ? left : I64_MAX, br0 = bottom ? right : I64_MIN;
    // the group's range: the 494 tiles of a pulse set all aim at one address -- reduce inside the wave first when its
    // live lanes share the group (the usual case), one atomic pair per wave instead of 64
    const u64 lm = ballot64(live);
    if (lm == 0) return;
    const i64 g0 = __shfl(g, __ffsll((long long)lm) - 1, 64);
    const bool one_group = all64(!live || g == g0);
    if (one_group) {
        for (int o = 32; o > 0; o >>= 1) {
            const i64 l2 = __shfl_xor(left, o, 64), r2 = __shfl_xor(right, o, 64);
            left = l2 < left ? l2 : left; right = r2 > right ? r2 : right;
        }
        if ((threadIdx.x & 63) == 0) { atomicMin(&a.grp_lo[g0], left); atomicMax(&a.grp_hi[g0], right); }
    } else if (live) { atomicMin(&a.grp_lo[g], left); atomicMax(&a.grp_hi[g], right); }
    // the range of the window's sum row: the same reduction over the bottom-array tiles (wave-uniform branches)
    if (!any64(bottom)) return;
    if (one_group) {
        i64 bl = bl0, br = br0;
        for (int o = 32; o > 0; o >>= 1) {
            const i64 l2 = __shfl_xor(bl, o, 64), r2 = __shfl_xor(br, o, 64);
            bl = l2 < bl ? l2 : bl; br = r2 > br ? r2 : br;
        }
        if ((threadIdx.x & 63) == 0) { atomicMin(&a.sum_lo[g0], bl); atomicMax(&a.sum_hi[g0], br); }
    } else if (bottom) { atomicMin(&a.sum_lo[g], bl0); atomicMax(&a.sum_hi[g], br0); }
}

// per group: window (rawdata.py:215-224) and the noise offset (rawdata.py:407-417)
__global__ void k_group_final(WfsDev d, GeomArgs a)
{
    i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.scal->n_groups) return;
    if (a.grp_lo[g] == I64_MAX) { a.grp_left[g] = 0; a.grp_right[g] = -1; a.grp_ixrand[g] = -1; return; }
    i64 left = a.grp_lo[g] - d.tw, right = a.grp_hi[g] + d.tw;
    if (!(right - left < 1000000)) atomicMax(&a.scal->error, (i64)WFS_DEV_WINDOW);           // "Pulse cache too long", rawdata.py:219
    if (floormod(left, 2) != 0) left -= 1;
    a.grp_left[g] = left; a.grp_right[g] = right;
    i64 ix = -1;
    if (d.enable_noise && d.nm_cells) ix = 0;                  // the noise model (wfs_set_noise_model) has no start index: nothing is drawn
    else if (d.enable_noise) {
        i64 nl = a.grp_lo[g] - left - d.tw, nr = a.grp_hi[g] - left + d.tw;
        i64 N = d.noise_len, high = (N - nr + nl - 1 < 0) ? N - 1 : N - nr + nl - 1;
        if (high <= 0) ix = 0;
        else { u32x4 w = philox4x32_10(0, a.cl_gid[a.grp_gid[g]], 0, SITE_NOISE, d.k0, d.k1); ix = (i64)(u53(w.x, w.y) * (double)high); }
        // (reduced modulo the noise length: add_noise wraps the index, rawdata.py:433-434, and the single-subtract wrap of
        // load_sample relies on ix < noise_len)
        if (a.noise_override && g < a.n_noise_override && a.noise_override[g] >= 0) ix = N > 0 ? a.noise_override[g] % N : 0;
    }
    a.grp_ixrand[g] = ix;
}

// Full readout: a row with pulses spans its window's range instead of its own (full_row_span, wfs_layout.h).  Behind k_tile_rows and
// k_group_final, in front of everything that places a tile in its row or sizes a row (k_row_len, k_tile_assign, k_tile_desc, k_tile_add,
// k_sum_signal): they all count from row_lo.  Rows without a pulse keep I64_MAX: they have no accumulators (k_row_len lists them).
__global__ void k_rows_widen(WfsDev d, GeomArgs a)
{
    const i64 ridx = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (ridx >= a.scal->n_groups * d.n_tpc || a.row_lo[ridx] == I64_MAX) return;
    const i64 g = ridx / d.n_tpc;
    a.row_lo[ridx] = a.grp_lo[g]; a.row_hi[ridx] = a.grp_hi[g];
}

// the last row slot of a window is its bottom-array sum row when the switch is on (wfs_set_sum_signal; row_slot_is_sum, wfs_layout.h)
#define SUM_CHUNK 1024             // samples of a sum row per workgroup of k_sum_signal

__device__ __forceinline__ bool row_is_direct(const i32 *tile_done, i64 n_done, const i32 *row_cnt, const i32 *row_tile, i64 ridx)
{
    if (!tile_done || row_cnt[ridx] != 1) return false;
    const i64 tile = row_tile[ridx];
    return tile < n_done && tile_done[tile] != 0;
}

// per (group, row slot): accumulator length and reserved ZLE interval slots; list of rows with data
// (appended with one global atomic per workgroup)
__global__ void k_row_len(WfsDev d, GeomArgs a)
{
    __shared__ i32 s_n, s_nres, s_nlong, s_direct, s_shared, s_maxres, s_reslen, s_nempty; __shared__ i64 s_base, s_rbase, s_lbase, s_ebase;
    if (threadIdx.x == 0) { s_n = 0; s_nres = 0; s_nlong = 0; s_direct = 0; s_shared = 0; s_maxres = 0; s_reslen = 0; s_nempty = 0; }
    __syncthreads();
    const i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const i64 n = a.scal->n_groups * d.row_slots;
    i32 cap = 0, rk = -1; bool resident = false, longrow = false, empty = false;
    if (idx < n) {
        const i64 g = idx / d.row_slots; const i32 slot = (i32)(idx - g * d.row_slots);
        const bool sum = row_slot_is_sum(d, slot);
        const i32 ch = slot < d.n_tpc ? slot : slot - d.n_tpc;         // HE slot -> its top channel
        const i64 lo = sum ? a.sum_lo[g] : a.row_lo[g * d.n_tpc + ch];
        if (sum) {
            // the sum row spans the union of the window's bottom rows (rawdata.py:234-235, 258-259); an accumulator row like any other,
            // filled by k_sum_signal in SUM_CHUNK samples per workgroup
            if (lo != I64_MAX) {
                const i64 len = row_span(lo, a.sum_hi[g], d.tw).len;
                cap = (i32)zle_slots(len, zle_holdoff(d.tw));
                a.sum_len[g] = (i32)len; a.sum_nchunk[g] = (i32)((len + SUM_CHUNK - 1) / SUM_CHUNK);
                rk = atomicAdd(&s_n, 1);
            }
        } else if (lo != I64_MAX) {
            const i64 len = row_span(lo, a.row_hi[g * d.n_tpc + ch], d.tw).len;
            cap = (i32)zle_slots(len, zle_holdoff(d.tw));
            // a row made by ONE tile whose samples exist already (k_s2_tile) is read from the tile's buffer: no accumulators
            // (full readout: the row is longer than its tile -- accumulators and k_tile_add)
            const bool direct = !d.full_readout && row_is_direct(a.tile_done, a.n_done, a.row_cnt, a.row_tile, g * d.n_tpc + ch);
            // a short row of small tiles is made in LDS by one wave (k_row_pulse): no accumulators either, 16-bit finished samples instead
            // (a row longer than res_max_len samples is made in segments of that length, its tiles looked at once per segment)
            resident = a.res_on && !direct && !a.row_bad[g * d.n_tpc + ch]
                       && (len <= a.res_max_len || (i64)a.row_cnt[g * d.n_tpc + ch] * ((len + a.res_max_len - 1) / a.res_max_len) <= RES_MAX_TILE_VISITS);
            if (slot < d.n_tpc) {
                a.acc_len[g * d.n_tpc + ch] = (direct || resident) ? 0 : (i32)len; if (direct) atomicAdd(&s_direct, (i32)len);
                if (a.res_on) { a.fin_len[g * d.n_tpc + ch] = resident ? fin_padded_len((i32)len) : 0; a.res_cnt[g * d.n_tpc + ch] = resident ? a.row_cnt[g * d.n_tpc + ch] : 0; }
                if (resident) { atomicMax(&s_maxres, (i32)len); atomicAdd(&s_reslen, (i32)len); longrow = len > RES_SHORT_LEN; }
            }
            if (slot < d.n_tpc && !resident && a.row_cnt && a.row_cnt[g * d.n_tpc + ch] > 1) atomicAdd(&s_shared, 1);
            rk = atomicAdd(resident ? (longrow ? &s_nlong : &s_nres) : &s_n, 1);
        } else if (d.full_readout && a.grp_lo[g] != I64_MAX) {
            // full readout: a TPC or HE slot without a pulse in a window that has one -- a row of the window's range, made finished by
            // k_row_empty: no accumulators, no tile, 16-bit samples behind those of the resident rows
            const i64 len = full_row_span(a.grp_lo[g], a.grp_hi[g], d.tw).len;
            cap = (i32)zle_slots(len, zle_holdoff(d.tw));
            a.fr_len[idx] = fin_padded_len((i32)len);
            empty = true; rk = atomicAdd(&s_nempty, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_n) s_base = (i64)atomicAdd((u64 *)&a.scal->n_front_rows, (u64)s_n);
    if (threadIdx.x == 0 && s_nres) s_rbase = (i64)atomicAdd((u64 *)&a.scal->n_short_rows, (u64)s_nres);
    if (threadIdx.x == 0 && s_nlong) s_lbase = (i64)atomicAdd((u64 *)&a.scal->n_long_rows, (u64)s_nlong);
    if (threadIdx.x == 0 && s_nempty) s_ebase = (i64)atomicAdd((u64 *)&a.scal->n_empty_rows, (u64)s_nempty);
    if (threadIdx.x == 0 && s_reslen) { atomicMax(&a.scal->max_res_len, (i64)s_maxres); atomicAdd((u64 *)&a.scal->n_res_samples, (u64)s_reslen); }
    if (threadIdx.x == 0 && s_direct) atomicAdd((u64 *)&a.scal->n_direct_samples, (u64)s_direct);      // samples of the rows read in place
    if (threadIdx.x == 0 && s_shared) atomicAdd((u64 *)&a.scal->n_shared_rows, (u64)s_shared);      // rows made by several tiles (k_tile_add is needed)
    __syncthreads();
    if (rk >= 0) {
        if (empty) a.empty_rows[s_ebase + rk] = (i32)idx;
        else if (!resident) a.active_rows[s_base + rk] = (i32)idx;
        else if (!longrow) a.active_rows[a.rows_cap - 1 - (s_rbase + rk)] = (i32)idx;
        else a.res_long[s_lbase + rk] = (i32)idx;
    }
    if (idx < a.n_gslots * d.row_slots) a.itv_cap[idx] = cap;
}

// ------------------------------------------------------------------------------------------------ pulse kernel
// Pulse.__call__ per-channel body + add_current (pulse.py:82-144, 276-318) + the per-pulse rounding and
// accumulation of digitize_pulse_cache (rawdata.py:231-239), one workgroup per tile.
//
// add_current visits photons in ascending time, merges photons of equal ns and adds templates[t % dt] * gain_total
// at sample t // dt - pulse_left.  Here the merged gains are built first in LDS, H[r][j] = sum of gains of photons
// with t % dt = r in start bin j (one LDS float atomic per photon), then every sample gathers its 22 x 10 possible
// contributions in ascending (j, r) = ascending time order with a separate multiply and add.  Adding a zero
// contribution does not change a float sum, so the result equals the reference's current bit for bit (except for
// the order in which three or more photons of the SAME ns are merged, which numpy's unstable argsort leaves open).
// Everything a pulse workgroup needs to know about its tile, resolved once per tile by k_tile_desc (five levels of
// dependent lookups otherwise: work list -> tile -> pulse set -> cluster -> window row).  64 bytes, read with scalar loads.
struct TileDesc {
    i64 off;              // first photon
    i64 dst;              // index in raw[] of the tile's sample 0
    i64 rel0;             // ns of the tile's first start bin relative to the set's t0
    double G, thr;        // PMT gain, truth threshold of the channel
    i32 n, nb, L, tile;   // photons, start bins, samples, tile id
    i32 ch, mode;
};

struct PulseArgs {
    const TileDesc *desc;   // per entry of the kernel's stretch of the work list (k_tile_desc)
    const PhotonRec *ph; const double *ph_gain;       // ph_gain: the photons of the sets of mode 1 (TileDesc::mode; 0: SPE codes)
    i32 *raw;
    double *tile_truth;   // [n_tiles][8] per-tile partial sums: n, n_dpe, n_trig, n_trig_dpe, sum g, sum g trig, sum t, sum t^2 -> k_truth_reduce
    double *currents; const i64 *cur_off;     // debug: f64 tile currents
    i32 W;                // bins capacity of the sparse kernel's LDS tables
    i32 NP;               // photon capacity of the sparse kernel's LDS list
    i32 n_win;            // dense kernel: workgroups per tile (each takes every n_win-th chunk of TPB samples)
    i32 spe_lds;          // dense resident kernel: the H table has room for the channel's SPE row (SPE_ROW_LEN doubles), staged there before the gains are looked up
    i32 sparse_max;       // dense kernel: a wave whose samples see at most this many occupied cells walks them instead of gathering all 220 per sample (tap_block)
};

#define DENSE_PPT 8        // photons per thread per batch held in registers

struct TemplateArg { double t[22 * WFS_DT]; };    // t[k * dt + r] = templates[r][k]; kernarg segment -> scalar loads, the taps live in SGPRs

// ---- the reference's per-photon rules, one definition each: every pulse kernel below and the tile generator (wfs_tilegen.h) call these
// The SPE row of a channel (pulse.py:97-103): one row per channel, or one row shared by all of them.
__device__ __forceinline__ const double *spe_row_of(const WfsDev &d, i32 ch) { return d.spe + (size_t)(d.n_spe > 1 ? ch : 0) * SPE_ROW_LEN; }
// The row (16 KB) into LDS past the registers (global_load_lds: 16 bytes per lane, a wave fills 1 KB of LDS per instruction).  The
// caller waits (vmcnt) and synchronises before it reads H.
template <int TPB>
__device__ __forceinline__ void spe_row_to_lds(const double *row, double *H, int tid)
{
    constexpr int NIT = (SPE_ROW_LEN * 8 + TPB * 16 - 1) / (TPB * 16);
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        // first double of this lane's 16 bytes; the lanes behind the row re-read its last entry (index SPE_BINS: its second
        // half is the first entry of the next row or, behind the last row, the slack every device buffer has)
        const int i = (it * TPB + tid) * 2;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(row + (i < SPE_ROW_LEN ? i : SPE_BINS)),
                                         (__attribute__((address_space(3))) void *)(H + (it * TPB + (tid & ~63)) * 2), 16, 0, 0);
    }
}
// Gain of a photon from the row's entries s1 = spe[code & 0xffff], s2 = spe[code >> 16] (pulse.py:97-98; the second photoelectron of a
// double-PE photon, code >> 16 != 0: pulse.py:101-103).  Two products, each rounded, and a conditional add.  s2() is asked for a
// double PE only: spe_gain has the entry at hand (batched loads), photon_gain loads both at the point of use.
template <class Second>
__host__ __device__ __forceinline__ double spe_gain_of(double G, double s1, u32 code, Second s2)
{
    double g = G * s1;
    if (code >> 16) g += G * s2();
    return g;
}
__host__ __device__ __forceinline__ double spe_gain(double G, double s1, double s2, u32 code) { return spe_gain_of(G, s1, code, [=] { return s2; }); }
__device__ __forceinline__ double photon_gain(const double *row, double G, u32 code) { return spe_gain_of(G, row[code & 0xffffu], code, [=] { return row[code >> 16]; }); }
// Truth sums of a tile (pulse.py:229-271): acc = n, n_dpe, n_trig, n_trig_dpe, sum g, sum g trig, sum t, sum t^2 -> k_truth_reduce.
// A photon triggers when its pulse height exceeds the channel's threshold; cmax_r = current_max[ns % dt] (pulse.py:32).
__device__ __forceinline__ bool truth_above(const WfsDev &d, double gain, double cmax_r, double thr) { return gain * cmax_r * d.c2a > thr; }
// One photon.  rank_below_ndpe: its index in the channel slice is below the tile's DPE count -- the reference marks the FIRST n_dpe
// photons of the slice as the double-PE ones, whichever they are (pulse.py:255).  tr: its time relative to the set origin.
__device__ __forceinline__ void truth_add(double (&acc)[8], double gain, bool above, bool is_dpe, bool rank_below_ndpe, double tr)
{
    acc[0] += 1; acc[1] += is_dpe; acc[4] += gain;
    if (above) { acc[2] += 1; acc[5] += gain; if (rank_below_ndpe) acc[3] += 1; }
    acc[6] += tr; acc[7] += tr * tr;
}
// Sum of a per-thread count over the workgroup (the tile's DPE photons); wsum: [TPB / 64].  Holds a barrier.
template <int TPB>
__device__ __forceinline__ i32 block_sum_u32(i32 c, u32 *wsum)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if (lane == 0) wsum[wid] = (u32)c;
    __syncthreads();
    i32 sum = 0;
    for (int w = 0; w < TPB / 64; w++) sum += (i32)wsum[w];
    return sum;
}
// The eight sums over a wave, then over the waves in a fixed order (red: [TPB / 64][8]) -> out[8].  The order of a floating-point sum is
// behaviour: each kernel keeps its wave reduction, the shuffle tree or the DPP tree of wave_sum.
__device__ __forceinline__ void truth_wave_shfl(double (&acc)[8])
{
#pragma unroll
    for (int q = 0; q < 8; q++) for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_down(acc[q], o, 64);
}
__device__ __forceinline__ void truth_wave_dpp(double (&acc)[8])
{
#pragma unroll
    for (int q = 0; q < 8; q++) acc[q] = wave_sum(acc[q]);
}
template <int TPB>
__device__ __forceinline__ void truth_store_block(const double (&acc)[8], double *red, double *out)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (lane == 0) for (int q = 0; q < 8; q++) red[wid * 8 + q] = acc[q];
    __syncthreads();
    if (tid < 8) { double sum = 0; for (int w = 0; w < TPB / 64; w++) sum += red[w * 8 + tid]; out[tid] = sum; }
}
// ADC count of a current (rawdata.py:236; np.around = round half to even)
__device__ __forceinline__ double adc_round(const WfsDev &d, double c) { return rint(c * d.c2a); }
__device__ __forceinline__ i64 adc_of(const WfsDev &d, double c) { return -(i64)adc_round(d, c); }
// Samples of a tile in front of its first start bin (pulse.py:118-127)
__host__ __device__ __forceinline__ int tile_lead(const WfsDev &d) { return d.store_before + d.samples_before; }

// ---- PMT dark counts (wfs_set_dark_counts; the definition: wfs_dark.h).  One rule in two forms that must agree: dark_sample,
// a sample on its own (the general paths: finish_sample_of, load_sample), and dark_block, 256 consecutive samples of a wave, four per
// lane (the finish_four loops of k_zle, k_row_pulse and k_row_empty).  The row kernels take the switch as a template parameter DK beside
// NK: with the feature off they are the kernels they were.
__device__ __forceinline__ u32x4 dark_call(const WfsDev &d, i32 ch, i64 m, u32 site) { return philox4x32_10((u32)(u64)m, (u32)((u64)m >> 32), (u32)ch, site, d.k0, d.k1); }
// photons of a cell from word 0 of its count call; T: the channel's four thresholds, descending
__device__ __forceinline__ int dark_count_of(const u32 *T, u32 w) { return (int)(w < T[0]) + (int)(w < T[1]) + (int)(w < T[2]) + (int)(w < T[3]); }
// the PMT channel whose dark counts a row slot gets, or -1: an HE slot its top channel's, the sum row and channels beyond the given count none
__device__ __forceinline__ i32 dark_channel_of(const WfsDev &d, i32 channel, bool he)
{
    const i32 c = he ? (channel == d.sum_channel ? -1 : channel - d.he_first) : channel;
    return (d.dk_thr && c >= 0 && c < d.dk_channels && c < d.n_tpc) ? c : -1;
}
// photon j of cell m: its start bin idx = t_ns div dt relative to the cell's first sample (0 .. DK_CELL - 1), r = t_ns mod dt, its gain
struct DarkPhoton { i32 bin, r; i64 t_ns; double gain; };
__device__ __forceinline__ DarkPhoton dark_photon_of(const WfsDev &d, i32 ch, i64 m, int j, const u32x4 &W)
{
    const u32 wt = (j & 1) ? W.z : W.x, wg = (j & 1) ? W.w : W.y;
    const u32 off = (u32)(((u64)wt * (u32)(DK_CELL * d.dt)) >> 32);          // ns behind the cell's start, below DK_CELL dt
    DarkPhoton p;
    p.bin = (i32)(off / (u32)d.dt); p.r = (i32)(off - (u32)p.bin * (u32)d.dt);
    p.t_ns = m * (i64)(DK_CELL * d.dt) + (i64)off;
    const u32 code = (u32)(((u64)wg * (u32)SPE_BINS) >> 32) + 1u;             // the first index of gain_code: a single PE
    p.gain = photon_gain(spe_row_of(d, ch), d.gains[ch], code);
    return p;
}
// what a photon of gain g and remainder r adds at tap k (0 <= k < tlen) of its pulse: a pulse of its own, rounded on its own
__device__ __forceinline__ i32 dark_tap(const WfsDev &d, double gain, i32 r, i32 k) { return (i32)adc_of(d, gain * d.templates[r * d.tlen + k]); }
// D(ch, t); ch: a channel dark_channel_of gave
__device__ __forceinline__ i32 dark_sample(const WfsDev &d, i32 ch, i64 t)
{
    const u32 *T = d.dk_thr + (size_t)ch * DK_MAX;
    if (T[0] == 0u || d.gains[ch] == 0.0) return 0;
    i32 D = 0;
    const i64 m_hi = (t + d.samples_before) >> DK_CELL_SHIFT;
    for (i64 m = (t + d.samples_before - d.tlen + 1) >> DK_CELL_SHIFT; m <= m_hi; m++) {
        const int n = dark_count_of(T, dark_call(d, ch, m, SITE_DARK_N).x);
        for (int j = 0; j < n; j++) {
            const DarkPhoton p = dark_photon_of(d, ch, m, j, dark_call(d, ch, m, SITE_DARK_PH + (u32)(j >> 1)));
            const i64 k = t - (m * DK_CELL + p.bin) + d.samples_before;
            if (k >= 0 && k < d.tlen) D += dark_tap(d, p.gain, p.r, (i32)k);
        }
    }
    return D;
}
// acc[j] += D(ch, tb + 4 lane + j), j < 4: the wave's 256 samples from tb (wave-uniform, as ch) on.  ALL 64 LANES MUST BE EXECUTING.
// The first lanes draw the count words of the cells the block's samples can see a photon of (at most (255 + tlen) / 64 + 2); one ballot,
// and in the overwhelmingly common empty case nothing more happens.  Otherwise a wave-uniform loop over the photons of the non-empty
// cells: the photon's constants are broadcast (readfirstlane), and every lane adds the taps that fall on its own samples.
static_assert((255 + WFS_MAX_TLEN) / DK_CELL + 2 <= 64, "a lane per cell of a block");
__device__ __forceinline__ void dark_block(const WfsDev &d, i32 ch, i64 tb, int lane, i32 (&acc)[4])
{
    const u32 *T = d.dk_thr + (size_t)ch * DK_MAX;
    if (T[0] == 0u || d.gains[ch] == 0.0) return;                            // (wave-uniform)
    const i64 m_lo = (tb + d.samples_before - d.tlen + 1) >> DK_CELL_SHIFT, m_hi = (tb + 255 + d.samples_before) >> DK_CELL_SHIFT;
    int n = 0;
    if ((i64)lane <= m_hi - m_lo) n = dark_count_of(T, dark_call(d, ch, m_lo + lane, SITE_DARK_N).x);
    u64 mask = ballot64(n > 0);
    if (mask == 0) return;                                                   // wave-uniform
    const i64 t_lane = tb + 4 * lane;
    while (mask) {
        const int l = (int)__builtin_ctzll(mask); mask &= mask - 1;
        const i64 m = m_lo + l;
        const int nl = __builtin_amdgcn_readlane(n, l);
        for (int j = 0; j < nl; j++) {
            const DarkPhoton p = dark_photon_of(d, ch, m, j, dark_call(d, ch, m, SITE_DARK_PH + (u32)(j >> 1)));
            const i32 bin = __builtin_amdgcn_readfirstlane(p.bin), r = __builtin_amdgcn_readfirstlane(p.r);
            const long long gb = __double_as_longlong(p.gain);
            const double gain = __longlong_as_double((long long)(((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)((u64)gb >> 32)) << 32)
                                                                 | (u32)__builtin_amdgcn_readfirstlane((int)(u32)gb)));
            const i64 k0 = t_lane - (m * DK_CELL + bin) + d.samples_before;  // tap of the lane's first sample
#pragma unroll
            for (int s = 0; s < 4; s++) { const i64 k = k0 + s; if (k >= 0 && k < d.tlen) acc[s] += dark_tap(d, gain, r, (i32)k); }
        }
    }
}
// wfs_dark_count_samples: D(channel, t0 .. t0 + n - 1) through both forms -- a wave takes 256 consecutive samples through dark_block
// (every lane, whatever n: only the stores look at n), the last n & 3 samples go through dark_sample
__global__ __launch_bounds__(256) void k_dark_samples(WfsDev d, i32 channel, i64 t0, i64 n, i32 *out)
{
    const int lane = threadIdx.x & 63;
    const i64 b = ((i64)blockIdx.x * 4 + wave_in_block()) * 256;
    i32 v[4] = {0, 0, 0, 0};
    dark_block(d, channel, t0 + b, lane, v);
    const i64 s = b + 4 * lane;
    if (s + 3 < n) {
#pragma unroll
        for (int j = 0; j < 4; j++) out[s + j] = v[j];
    } else {
        for (i64 u = s; u < n; u++) out[u] = dark_sample(d, channel, t0 + u);
    }
}
// wfs_dark_count_photons: a thread per cell m0 + c writes the cell's count and its photons (time, gain) into slots [c][DK_MAX]
__global__ __launch_bounds__(256) void k_dark_photons(WfsDev d, i32 channel, i64 m0, i64 n_cells, i32 *count, i64 *t_ns, double *gain)
{
    const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cells) return;
    const u32 *T = d.dk_thr + (size_t)channel * DK_MAX;
    const i64 m = m0 + c;
    const int n = (T[0] == 0u || d.gains[channel] == 0.0) ? 0 : dark_count_of(T, dark_call(d, channel, m, SITE_DARK_N).x);
    count[c] = n;
    for (int j = 0; j < n; j++) {
        const DarkPhoton p = dark_photon_of(d, channel, m, j, dark_call(d, channel, m, SITE_DARK_PH + (u32)(j >> 1)));
        t_ns[c * DK_MAX + j] = p.t_ns; gain[c * DK_MAX + j] = p.gain;
    }
}

struct DescArgs { const i32 *list; i64 n; const i32 *tile_count, *tile_tmin, *tile_tmax; const i64 *tile_off; const i32 *set_cluster; const i64 *set_t0;
                  const i32 *set_mode; const i32 *cl_group; const i64 *row_lo; const i64 *acc_off; TileDesc *desc; };
__global__ void k_tile_desc(WfsDev d, DescArgs a)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const i64 tile = a.list[i];
    const i64 set = tile / d.n_tpc; const i32 ch = (i32)(tile - set * d.n_tpc);
    const i64 t0 = a.set_t0[set];
    const TileWindow w = tile_window(d, t0, a.tile_tmin[tile], a.tile_tmax[tile]);
    const i64 ridx = (i64)a.cl_group[a.set_cluster[set]] * d.n_tpc + ch;
    TileDesc t;
    t.off = a.tile_off[tile]; t.dst = a.acc_off[ridx] + (w.left - (a.row_lo[ridx] - d.tw)); t.rel0 = w.bin0 * d.dt - t0;
    t.G = d.gains[ch]; t.thr = d.thr_truth[ch];
    t.n = a.tile_count[tile]; t.nb = (i32)w.nb; t.L = (i32)w.L; t.tile = (i32)tile;
    t.ch = ch; t.mode = a.set_mode[set];
    a.desc[i] = t;
}

// The gather of one sample (pulse.py:303-318 in the H-table form): thread `tid` owns the sample whose start bins are the H rows
// tid (tap k = 21) .. tid + 21 (tap k = 0); it adds its tlen x dt possible contributions in ascending time, separate multiply and
// add.  The tap loop is outermost so that only the dt taps of one k are live in SGPRs.
template <bool FMA>
__device__ __forceinline__ double tap_gather(const double *H, const TemplateArg &tp, int tid)
{
    constexpr int dt = WFS_DT, tlen = 22;
    const double *Hs = H + (tid + (tlen - 1)) * dt;
    double c = 0.0;
#pragma unroll 1
    for (int k = tlen - 1; k >= 0; k--) {
        const double *Tk = tp.t + k * dt;          // the dt taps of one k are contiguous: two wide scalar loads
        const double T0 = Tk[0], T1 = Tk[1], T2 = Tk[2], T3 = Tk[3], T4 = Tk[4], T5 = Tk[5], T6 = Tk[6], T7 = Tk[7], T8 = Tk[8], T9 = Tk[9];
        const double2 *hp = (const double2 *)(Hs - k * dt);
        const double2 h0 = hp[0], h1 = hp[1], h2 = hp[2], h3 = hp[3], h4 = hp[4];
        c = mac<FMA>(T0, h0.x, c); c = mac<FMA>(T1, h0.y, c);
        c = mac<FMA>(T2, h1.x, c); c = mac<FMA>(T3, h1.y, c);
        c = mac<FMA>(T4, h2.x, c); c = mac<FMA>(T5, h2.y, c);
        c = mac<FMA>(T6, h3.x, c); c = mac<FMA>(T7, h3.y, c);
        c = mac<FMA>(T8, h4.x, c); c = mac<FMA>(T9, h4.y, c);
    }
    return c;
}

// The same sample from the OCCUPIED cells alone, for waves whose 64 samples see few photons (the tails of an S2 tile, where most of
// the 220 cells a sample gathers are empty: the dense gather spends 8 f64 issue cycles on every one of them).  The wave scans the
// 850 cells its samples can reach (H rows 64 w .. 64 w + 84) with ballots -- two rounds in the middle first: a wave in the
// bulk of the tile is recognised there and leaves for the dense gather.  With at most `sparse_max` (<= TAP_LIST_LEN) occupied cells
// it lists them in ascending time (LDS, 2 bytes each), lane i takes entry i (cell, merged gain) into registers, and the entries
// are then broadcast one by one with readlane: every lane looks up ITS tap W2[(10 (lane + 21) + 9) - cell] (the zero tap W2[220]
// outside the reach of its sample) and adds the product with a separate multiply and add -- the additions of the dense gather in
// the same order minus the additions of +0.0, hence the same bits (pulse.py:303-318).  W2[k * dt + (dt - 1 - r)] = templates[r][k].
// A cell counts as occupied when the high word of its merged gain is non-zero (any gain of at least 2^-1022).
// (TAP_W2_LEN taps, TAP_LIST_LEN entries of a wave's list: wfs_layout.h)
__device__ __forceinline__ void tap_w2_fill(double *W2, const double *templates, int tid, int tpb)
{
    constexpr int dt = WFS_DT, tlen = 22;
    for (int i = tid; i < TAP_W2_LEN; i += tpb) W2[i] = i < tlen * dt ? templates[(dt - 1 - i % dt) * tlen + i / dt] : 0.0;
}
// W2 is followed by the waves' lists: [TAP_W2_LEN doubles][tpb / 64][TAP_LIST_LEN] unsigned short (tap_lds_bytes, wfs_layout.h)
// n_cells: the cells of H that hold data (the caller may have cleared only the rows its live samples can see)
template <bool FMA>
__device__ __forceinline__ double tap_block(const double *H, double *W2, const TemplateArg &tp, int tid, int sparse_max, int n_cells)
{
    constexpr int dt = WFS_DT, tlen = 22, REACH = (64 + tlen - 1) * dt, NR = (REACH + 63) / 64;
    const int lane = tid & 63;
    if (sparse_max < 0) return tap_gather<FMA>(H, tp, tid);
    const double *Hw = H + (tid & ~63) * dt;            // first cell of the wave's reach
    const u32 *Hhi = (const u32 *)Hw + 1;               // high words
    static_assert(TAP_LISTS_OFF == TAP_W2_LEN * 8, "the lists follow W2");
    unsigned short *list = (unsigned short *)(W2 + TAP_W2_LEN) + (tid >> 6) * TAP_LIST_LEN;
    const u64 below = (1ull << lane) - 1ull;
    const int c_end = min(REACH, n_cells - (tid & ~63) * dt);      // cells of the reach that hold data
    {   // rounds 6 and 7 (the middle of the reach) first
        const u32 a = 6 * 64 + lane < c_end ? Hhi[2 * (6 * 64 + lane)] : 0u, b = 7 * 64 + lane < c_end ? Hhi[2 * (7 * 64 + lane)] : 0u;
        if (__popcll(ballot64(a != 0u)) + __popcll(ballot64(b != 0u)) > (sparse_max >> 2)) return tap_gather<FMA>(H, tp, tid);      // wave-uniform
    }
    int m = 0;
#pragma unroll 1
    for (int r0 = 0; r0 < NR; r0 += 4) {                 // (four loads in flight at a time)
        u32 hw[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int c = (r0 + u) * 64 + lane; hw[u] = c < c_end ? Hhi[2 * c] : 0u; }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const u64 mk = ballot64(hw[u] != 0u);
            if (mk) {                                    // wave-uniform
                const int pos = m + __popcll(mk & below);
                if (hw[u] != 0u && pos < TAP_LIST_LEN) list[pos] = (unsigned short)((r0 + u) * 64 + lane);
                m += __popcll(mk);
            }
        }
    }
    if (m > sparse_max) return tap_gather<FMA>(H, tp, tid);   // wave-uniform
    if (m == 0) return 0.0;
    // lane i <- entry i (behind the last entry: a cell no sample reaches)
    const int ci = lane < m ? (int)list[lane] : 0x7fff;
    const double gi = Hw[lane < m ? ci : 0];
    const int g_lo = (int)(u32)__double_as_longlong(gi), g_hi = (int)(u32)((u64)__double_as_longlong(gi) >> 32);
    const u32 A = (u32)((lane + tlen - 1) * dt + (dt - 1));
    double acc = 0.0;
    for (int i0 = 0; i0 < m; i0 += 4) {                  // four entries in flight (one LDS round trip per four)
        double w[4], g[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = (i0 + u) & 63;                 // (entries behind the last one carry the cell 0x7fff: the zero tap for every lane)
            const int c = __builtin_amdgcn_readlane(ci, i);
            g[u] = __longlong_as_double((long long)(((u64)(u32)__builtin_amdgcn_readlane(g_hi, i) << 32) | (u32)__builtin_amdgcn_readlane(g_lo, i)));
            u32 idx = A - (u32)c;
            idx = idx < (u32)(tlen * dt) ? idx : (u32)(tlen * dt);
            w[u] = W2[idx];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) acc = mac<FMA>(w[u], g[u], acc);
    }
    return acc;
}

template <int TPB, bool RESIDENT, bool FMA>
__global__ __launch_bounds__(TPB) void k_pulse(WfsDev d, PulseArgs a, TemplateArg tp)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int dt = WFS_DT, tlen = 22;
    // The live samples of a tile (sample s' = s - lead sees the start bins s' - 21 .. s') are worked off in chunks of TPB
    // consecutive samples, one per thread; a chunk needs the TPB + tlen - 1 start bins from 21 before its first sample on.
    constexpr int HROWS = TPB + tlen - 1;
    constexpr PulseLds o = pulse_lds(TPB);
    static_assert(tlen == TILE_TLEN, "the layout is sized for 22 taps");
    double *H = (double *)(smem + o.H);                   // [HROWS][dt]: merged gain per (start bin, ns remainder)
    double *red = (double *)(smem + o.red);               // [TPB / 64][8]
    u32 *wsum = (u32 *)(smem + o.wsum);                   // [16]
    double *W2 = (double *)(smem + o.W2);                 // [TAP_W2_LEN] taps by time difference + the waves' records (tap_block)
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // pulse.py:32 current_max, indexed per photon: from LDS (indexing the kernarg copy per lane becomes a global load)
    __shared__ double s_cmax[WFS_DT];
    if (tid < WFS_DT) s_cmax[tid] = d.current_max[tid];
    tap_w2_fill(W2, d.templates, tid, TPB);

    // grid = tiles x a.n_win: workgroup `win` of a tile takes the chunks win, win + n_win, ... (n_win = 1: the resident form)
    const i64 tidx = blockIdx.x / a.n_win;
    const int win = (int)(blockIdx.x - tidx * a.n_win);
    const TileDesc td = a.desc[tidx];                     // block-uniform: scalar loads
    const i64 tile = td.tile; const i32 n = td.n; const i64 off = td.off; const i32 ch = td.ch;
    const i64 nb = td.nb, L = td.L;
    const int lead = tile_lead(d);
    i32 *dst = a.raw + td.dst;
    const int mode = td.mode;
    const double G = td.G;
    const double *spe_row = spe_row_of(d, ch);
    const double thr = td.thr;
    const i64 rel0 = td.rel0;                             // ns of the tile's first start bin relative to t0

    const i64 n_live = nb + (tlen - 1);                   // samples lead .. lead + n_live - 1 can be non-zero
    if (win > 0 && (i64)win * TPB >= n_live) return;      // no chunk for this workgroup (block-uniform)
    // number of DPE photons of the tile (truth quirk pulse.py:255); truth is window 0's job.  A tile that fits one
    // register batch is counted from the registers inside the photon loop, longer ones with a scan of their own.
    i32 n_dpe_tile = 0;
    const bool one_batch = n <= TPB * DENSE_PPT;
    if (!RESIDENT && win == 0 && !one_batch) {
        i32 c = 0;
        for (i32 p = tid; p < n; p += TPB) c += (a.ph[off + p].code >> 16) != 0;
        n_dpe_tile = block_sum_u32<TPB>(c, wsum);
    }
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // n, n_dpe, n_trig, n_trig_dpe, sum g, sum g trig, sum t, sum t^2
    STAMP_INIT;

    // A tile that fits one register batch and is worked on by a single workgroup (n_win == 1) is read ONCE: its photons
    // (ns, gain) stay in registers over all windows, and the truth sums are taken here.
    i32 r_ns[DENSE_PPT]; double r_gain[DENSE_PPT];
    if (RESIDENT) {
        u32 code[DENSE_PPT];
        // The channel's SPE row (16 KB) goes through LDS (H is still free): two data-dependent 8-byte gathers per photon from
        // global memory cost the texture addresser ~64 cycles per wave instruction, from LDS a few.  Its loads are issued
        // together with the photon loads: one global round trip for both.
        const bool spe_lds = mode == 0 && a.spe_lds;         // block-uniform
        if (spe_lds) spe_row_to_lds<TPB>(spe_row, H, tid);
#pragma unroll
        for (int k = 0; k < DENSE_PPT; k++) {
            const i32 p = tid + k * TPB;
            const bool v = p < n;
            const PhotonRec rec = a.ph[off + (v ? p : 0)];            // branch-free: tiles on the work list have n >= 1
            r_ns[k] = v ? (i32)(rec.t - rel0) : -1;
            code[k] = v ? rec.code : 0u;
            r_gain[k] = 0.0;
        }
        // explicit gains (afterpulse / injected photons) in a loop of their own: a conditional load inside the loop above makes
        // the compiler wait for every photon load before the branch -- eight memory round trips in a row instead of one
        if (mode != 0) {
#pragma unroll
            for (int k = 0; k < DENSE_PPT; k++) { const i32 p = tid + k * TPB; const double g = a.ph_gain[off + (p < n ? p : 0)]; r_gain[k] = p < n ? g : 0.0; }
        }
        {
            i32 c = 0;
#pragma unroll
            for (int k = 0; k < DENSE_PPT; k++) c += (code[k] >> 16) != 0;
            // the SPE row has landed in LDS (issued ahead of the photon loads the count depends on: the wait costs nothing here)
            if (spe_lds) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            n_dpe_tile = block_sum_u32<TPB>(c, wsum);
        }
        if (mode == 0) {
            if (spe_lds) {
                // (in two halves: sixteen 8-byte values in flight at once cost the registers of a seventh wave per SIMD)
#pragma unroll
                for (int h0 = 0; h0 < DENSE_PPT; h0 += DENSE_PPT / 2) {
                    double s1[DENSE_PPT / 2], s2[DENSE_PPT / 2];
#pragma unroll
                    for (int k = 0; k < DENSE_PPT / 2; k++) { s1[k] = H[code[h0 + k] & 0xffffu]; s2[k] = H[code[h0 + k] >> 16]; }     // H[0] for "no second PE": unused
#pragma unroll
                    for (int k = 0; k < DENSE_PPT / 2; k++) r_gain[h0 + k] = spe_gain(G, s1[k], s2[k], code[h0 + k]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                __syncthreads();                             // H is reused below
            } else {
                double s1[DENSE_PPT], s2[DENSE_PPT];
#pragma unroll
                for (int k = 0; k < DENSE_PPT; k++) {
                    s1[k] = spe_row[code[k] & 0xffffu];                // index 0 for the unused slots: a valid address
                    s2[k] = 0;
                    if (code[k] >> 16) s2[k] = spe_row[code[k] >> 16];
                }
#pragma unroll
                for (int k = 0; k < DENSE_PPT; k++) r_gain[k] = spe_gain(G, s1[k], s2[k], code[k]);
            }
        }
        STAMP(d, 8);
        // truth sums of the tile (pulse.py:229-271).  The four counts need no vector reduction (tile_count, the DPE count
        // above, wave ballots); the four float sums go through LDS (H is still free) and one shuffle tree per quantity.
        u32 c_trig = 0, c_trig_dpe = 0;                   // wave-uniform
        double sg = 0, sgt = 0, st = 0, st2 = 0;
#pragma unroll
        for (int k = 0; k < DENSE_PPT; k++) {
            const bool v = r_ns[k] >= 0;
            const int r = v ? r_ns[k] % dt : 0;
            const bool above = v && truth_above(d, r_gain[k], s_cmax[r], thr);
            c_trig += (u32)__popcll(ballot64(above));
            c_trig_dpe += (u32)__popcll(ballot64(above && tid + k * TPB < n_dpe_tile));
            if (v) {
                sg += r_gain[k];
                if (above) sgt += r_gain[k];
                const double tr = (double)(r_ns[k] + rel0);
                st += tr; st2 += tr * tr;
            }
        }
        if (a.tile_truth) {
            constexpr int NW = TPB / 64;
            double *S = H;                                 // [4][TPB]
            S[0 * TPB + tid] = sg; S[1 * TPB + tid] = sgt; S[2 * TPB + tid] = st; S[3 * TPB + tid] = st2;
            if (lane == 0) { wsum[NW + wid * 2] = c_trig; wsum[NW + wid * 2 + 1] = c_trig_dpe; }
            __syncthreads();
            for (int q = wid; q < 4; q += NW) {
                double x = 0;
#pragma unroll
                for (int j = 0; j < NW; j++) x += S[q * TPB + j * 64 + lane];
                for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
                if (lane == 0) a.tile_truth[tile * 8 + 4 + q] = x;
            }
            if (tid == 0) {
                u32 t2 = 0, t3 = 0;
                for (int w = 0; w < NW; w++) { t2 += wsum[NW + w * 2]; t3 += wsum[NW + w * 2 + 1]; }
                double *o = a.tile_truth + tile * 8;
                o[0] = (double)n; o[1] = (double)n_dpe_tile; o[2] = (double)t2; o[3] = (double)t3;
            }
        }
    }

    STAMP(d, 9);
    // samples before the first start bin can reach (lead of them) and behind the reach of the last one are exactly zero and the
    // accumulators start from zero: nothing to do for them (the debug copy of the currents wants every sample)
    if (a.currents && win == 0) for (i64 sz = tid; sz < L; sz += TPB) if (sz < lead || sz >= lead + n_live) a.currents[a.cur_off[tidx] + sz] = 0.0;
    for (i64 c0 = (i64)win * TPB; c0 < n_live; c0 += (i64)a.n_win * TPB) {
        const bool first = (c0 == 0);
        const i64 b_lo = c0 - (tlen - 1);                  // start bin of H row 0 (may be negative: those rows stay empty)
        __syncthreads();
        for (int i = tid; i < HROWS * dt; i += TPB) H[i] = 0.0;
        __syncthreads();
        STAMP(d, 10);
        if (RESIDENT) {
            const i32 ns_lo = (i32)b_lo * dt, ns_hi = ns_lo + HROWS * dt;   // the chunk's start bins in ns relative to the tile's first start bin
#pragma unroll
            for (int k = 0; k < DENSE_PPT; k++) {
                if (r_ns[k] < 0 || r_ns[k] < ns_lo || r_ns[k] >= ns_hi) continue;
                atomicAdd(&H[r_ns[k] - ns_lo], r_gain[k]);                  // (start bin - b_lo) * dt + r
            }
        } else
        // ---- photons -> H, in register batches so that the global loads of a batch are all in flight together
        for (i32 base = 0; base < n; base += TPB * DENSE_PPT) {
            i32 ns[DENSE_PPT]; u32 code[DENSE_PPT]; double gain[DENSE_PPT]; bool use[DENSE_PPT];
#pragma unroll
            for (int k = 0; k < DENSE_PPT; k++) {
                const i32 p = base + tid + k * TPB;
                const bool v = p < n;
                const PhotonRec rec = a.ph[off + (v ? p : 0)];        // branch-free: tiles on the work list have n >= 1
                ns[k] = v ? (i32)(rec.t - rel0) : -1;
                code[k] = v ? rec.code : 0u;
                const i64 jw = (i64)(ns[k] / dt) - b_lo;
                use[k] = v && (first || (jw >= 0 && jw < HROWS));      // chunk 0 needs every photon (truth), the others only their own
                gain[k] = 0.0;
            }
            if (mode != 0) {                                 // (a loop of its own: see the resident form)
#pragma unroll
                for (int k = 0; k < DENSE_PPT; k++) { const i32 p = base + tid + k * TPB; const double g = a.ph_gain[off + (p < n ? p : 0)]; gain[k] = use[k] ? g : 0.0; }
            }
            if (first && one_batch) {                // (one batch, several workgroups per tile)
                i32 c = 0;
#pragma unroll
                for (int k = 0; k < DENSE_PPT; k++) c += (code[k] >> 16) != 0;
                n_dpe_tile = block_sum_u32<TPB>(c, wsum);
            }
            if (mode == 0) {
                double s1[DENSE_PPT], s2[DENSE_PPT];
#pragma unroll
                for (int k = 0; k < DENSE_PPT; k++) {
                    s1[k] = 0; s2[k] = 0;
                    if (use[k]) { s1[k] = spe_row[code[k] & 0xffffu]; if (code[k] >> 16) s2[k] = spe_row[code[k] >> 16]; }
                }
#pragma unroll
                for (int k = 0; k < DENSE_PPT; k++) gain[k] = spe_gain(G, s1[k], s2[k], code[k]);
            }
#pragma unroll
            for (int k = 0; k < DENSE_PPT; k++) {
                if (!use[k]) continue;
                const int bin = ns[k] / dt, r = ns[k] - bin * dt;
                const i64 jw = bin - b_lo;
                if (jw >= 0 && jw < HROWS) atomicAdd(&H[(int)jw * dt + r], gain[k]);
                if (first) {
                    const bool above = truth_above(d, gain[k], s_cmax[r], thr);
                    // (truth_add, written out: through the helper this kernel, at the edge of its register budget, takes one VGPR more)
                    const bool is_dpe = (code[k] >> 16) != 0;
                    acc[0] += 1; acc[1] += is_dpe; acc[4] += gain[k];
                    if (above) { acc[2] += 1; acc[5] += gain[k]; if (base + tid + k * TPB < n_dpe_tile) acc[3] += 1; }
                    const double tr = (double)(ns[k] + rel0);
                    acc[6] += tr; acc[7] += tr * tr;
                }
            }
        }
        __syncthreads();
        STAMP(d, 11);
        // ---- every sample gathers its tlen x dt possible contributions in ascending time (pulse.py:303-318): sample c0 + tid
        // reads the rows tid (tap k = 21) .. tid + 21 (tap k = 0).  The tap loop is outermost so that only the dt taps of one
        // k are live in SGPRs.
        const bool act = c0 + tid < n_live;
        if (any64(act)) {                                  // wave-uniform
            const double c = tap_block<FMA>(H, W2, tp, tid, a.sparse_max, HROWS * dt);
            if (act) {
                const i64 sx = lead + c0 + tid;            // sample of the tile
                if (a.currents) a.currents[a.cur_off[tidx] + sx] = c;
                const i64 adc = adc_of(d, c);
                if (adc != 0) atomicAdd(&dst[sx], (i32)adc);
            }
        }
        STAMP(d, 12);
    }

    if (!RESIDENT && a.tile_truth && win == 0) {
        truth_wave_shfl(acc);
        __syncthreads();
        truth_store_block<TPB>(acc, red, a.tile_truth + tile * 8);
    }
}

// Any digitiser geometry (sample_duration dt <= WFS_MAX_DT ns, template length tlen <= WFS_MAX_TLEN samples; pulse.py:146-187 builds the
// templates for whatever the config says): the same H-table scheme with the geometry taken from the config at run time -- merged
// gains H[start bin][ns remainder] in LDS, every sample gathers its tlen x dt possible contributions in ascending time with a
// separate multiply and add, templates read from LDS.  One workgroup per tile, chunks of TPB samples, the tile's photons re-read per
// chunk; none of the specialisations of the 10 ns / 22 tap kernels (they keep the taps in SGPRs and unroll over dt): this is the
// path of every tile when the configuration differs from the XENONnT TPC digitiser.  Same bits as the reference (add_current).
// (WFS_MAX_DT, WFS_MAX_TLEN: wfs_layout.h)
template <int TPB, bool FMA>
__global__ __launch_bounds__(TPB) void k_pulse_generic(WfsDev d, PulseArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int dt = d.dt, tlen = d.tlen;
    const int HROWS = TPB + tlen - 1;
    // The gains of one (start bin, ns) cell are merged by atomic adds, whose order changes from run to run.  So that the merged gain does
    // not depend on it, every gain is split at a power of two `grid` (2^-20 of the tile's largest gain): the multiples of grid add up
    // EXACTLY in H (below 2^53 grid for any photon number), the remainders (below grid / 2) in Hlo, and the cell is their sum, rounded
    // once -- for one or two photons numpy's value bit for bit (pulse.py:313), for more the correctly rounded sum up to 2^-23 n ulp.
    // (a.n_win == 0: geometries whose two tables would not fit the LDS keep one table and the plain atomic merge)
    const bool split = a.n_win != 0;
    static_assert(TPB == 256, "generic_lds is the layout of the 256-thread form");
    const GenericLds o = generic_lds(dt, tlen, split);
    double *H = (double *)(smem + o.H);                   // [HROWS][dt]
    double *Hlo = (double *)(smem + o.Hlo);               // [HROWS][dt] (split)
    double *T = (double *)(smem + o.T);                   // [dt][tlen] templates
    double *red = (double *)(smem + o.red);               // [TPB / 64][8]
    __shared__ double s_cmax[WFS_MAX_DT];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < dt * tlen; i += TPB) T[i] = d.templates[i];
    if (tid < dt) s_cmax[tid] = d.current_max[tid];
    const TileDesc td = a.desc[blockIdx.x];
    const i64 tile = td.tile; const i32 n = td.n; const i64 off = td.off;
    const i64 nb = td.nb;
    const int lead = tile_lead(d);
    i32 *dst = a.raw + td.dst;
    const double G = td.G, thr = td.thr;
    const double *spe_row = spe_row_of(d, td.ch);
    const i64 rel0 = td.rel0;
    const i64 n_live = nb + (tlen - 1);
    auto gain_of = [&](const PhotonRec &rec, i32 p) -> double {
        if (td.mode != 0) return a.ph_gain[off + p];
        return photon_gain(spe_row, G, rec.code);
    };
    // number of DPE photons of the tile (truth quirk pulse.py:255) and the exponent field of its largest gain
    __shared__ i32 s_ndpe, s_emax;
    if (tid == 0) { s_ndpe = 0; s_emax = 0; }
    __syncthreads();
    {
        i32 c = 0, em = 0;
        for (i32 p = tid; p < n; p += TPB) {
            const PhotonRec rec = a.ph[off + p];
            c += (rec.code >> 16) != 0;
            em = max(em, (i32)((__double_as_longlong(gain_of(rec, p)) >> 52) & 0x7ff));
        }
        c = wave_sum(c); em = wave_max(em);
        if (lane == 0 && c) atomicAdd(&s_ndpe, c);
        if (lane == 0) atomicMax(&s_emax, em);
    }
    __syncthreads();
    const i32 n_dpe_tile = s_ndpe;
    const int gf = min(max(s_emax - 20, 1), 2045);
    const double grid = __longlong_as_double((long long)gf << 52), inv_grid = __longlong_as_double((long long)(2046 - gf) << 52);
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // n, n_dpe, n_trig, n_trig_dpe, sum g, sum g trig, sum t, sum t^2
    if (a.currents) for (i64 sz = tid; sz < td.L; sz += TPB) if (sz < lead || sz >= lead + n_live) a.currents[a.cur_off[blockIdx.x] + sz] = 0.0;
    for (i64 c0 = 0; c0 < n_live; c0 += TPB) {
        const bool first = c0 == 0;
        const i64 b_lo = c0 - (tlen - 1);
        __syncthreads();
        for (int i = tid; i < (split ? 2 : 1) * HROWS * dt; i += TPB) H[i] = 0.0;           // (H and Hlo)
        __syncthreads();
        for (i32 p = tid; p < n; p += TPB) {
            const PhotonRec rec = a.ph[off + p];
            const i32 ns = (i32)(rec.t - rel0);
            const int bin = ns / dt, r = ns - bin * dt;
            const i64 jw = bin - b_lo;
            const bool mine = jw >= 0 && jw < HROWS;
            if (!first && !mine) continue;
            const double gain = gain_of(rec, p);
            if (mine && split) {
                const double hi = rint(gain * inv_grid) * grid;
                atomicAdd(&H[(int)jw * dt + r], hi);
                atomicAdd(&Hlo[(int)jw * dt + r], gain - hi);
            } else if (mine) atomicAdd(&H[(int)jw * dt + r], gain);
            if (first) {
                const bool above = truth_above(d, gain, s_cmax[r], thr);
                truth_add(acc, gain, above, (rec.code >> 16) != 0, p < n_dpe_tile, (double)(ns + rel0));
            }
        }
        __syncthreads();
        if (split) {                                       // block-uniform
            for (int i = tid; i < HROWS * dt; i += TPB) H[i] += Hlo[i];
            __syncthreads();
        }
        if (c0 + tid < n_live) {
            // sample c0 + tid sees the start bins (rows) tid (tap tlen - 1) .. tid + tlen - 1 (tap 0), ascending time (pulse.py:303-318)
            double c = 0.0;
            for (int k = tlen - 1; k >= 0; k--) {
                const double *hp = H + (size_t)(tid + (tlen - 1) - k) * dt;
                for (int r = 0; r < dt; r++) c = mac<FMA>(T[r * tlen + k], hp[r], c);
            }
            const i64 sx = lead + c0 + tid;
            if (a.currents) a.currents[a.cur_off[blockIdx.x] + sx] = c;
            const i64 adc = adc_of(d, c);
            if (adc != 0) atomicAdd(&dst[sx], (i32)adc);
        }
    }
    if (a.tile_truth) {
        truth_wave_dpp(acc);
        __syncthreads();
        truth_store_block<TPB>(acc, red, a.tile_truth + tile * 8);
    }
}

// Tiny tiles (a few photons in a few start bins: almost every tile of an S1): one THREAD per tile.  The photons are
// sorted by time in registers, equal-ns photons merged (first of the run carries the summed gain), and every sample in
// reach of a photon adds templates[r][k] * gain in ascending time with a separate multiply and add: the arithmetic of
// add_current (pulse.py:276-318), hence the same bits as the other two kernels.  Truth sums need no reduction.
// The pulse of a tile of at most TINY_MAX_PHOTONS photons (see k_pulse_tiny) in two steps.  tiny_tile_prepare: the photons sorted by
// time, runs of equal ns merged, start bin and ns remainder of each, the samples they reach -- and the tile's truth sums (sub == 0).
// tiny_tile_samples: lane `sub` of LANES takes the samples s_first + sub, + LANES, ...; tap(r, k) = templates[r][k], sink(s, adc)
// receives the non-zero ADC counts.
struct TinyPrep { int jb[TINY_MAX_PHOTONS], rr[TINY_MAX_PHOTONS]; double g[TINY_MAX_PHOTONS]; int n, s_first, s_last; };
__device__ __forceinline__ TinyPrep tiny_tile_prepare(const WfsDev &d, const PulseArgs &a, const TileDesc &td, int sub, const double *s_cmax)
{
    constexpr int dt = WFS_DT, tlen = 22, NP = TINY_MAX_PHOTONS;
    const int n = td.n, L = td.L;
    const int lead = tile_lead(d);
    const double G = td.G;
    const double *spe_row = spe_row_of(d, td.ch);
    i32 ns[NP]; double g[NP]; u32 code[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) {
        const bool v = k < n;
        const PhotonRec rec = a.ph[td.off + (v ? k : 0)];
        ns[k] = v ? (i32)(rec.t - td.rel0) : 0x7fffffff;
        code[k] = v ? rec.code : 0u;
        g[k] = 0.0;
        if (v) {
            if (td.mode != 0) g[k] = a.ph_gain[td.off + k];
            else g[k] = photon_gain(spe_row, G, code[k]);
        }
    }
    if (a.tile_truth && sub == 0) {        // pulse.py:229-271, photons in their order in the channel slice
        i32 n_dpe = 0;
#pragma unroll
        for (int k = 0; k < NP; k++) n_dpe += (code[k] >> 16) != 0;
        double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < NP; k++) {
            if (k >= n) continue;
            const bool above = truth_above(d, g[k], s_cmax[ns[k] % dt], td.thr);
            truth_add(v, g[k], above, (code[k] >> 16) != 0, k < n_dpe, (double)(ns[k] + td.rel0));
        }
        for (int q = 0; q < 8; q++) a.tile_truth[(i64)td.tile * 8 + q] = v[q];
    }
    // ---- ascending time (stable: equal ns keep their order), then merge runs of equal ns
#pragma unroll
    for (int i = 1; i < NP; i++)
#pragma unroll
        for (int j = i; j > 0; j--)
            if (ns[j] < ns[j - 1]) { const i32 t = ns[j]; ns[j] = ns[j - 1]; ns[j - 1] = t; const double x = g[j]; g[j] = g[j - 1]; g[j - 1] = x; }
    // run heads collect the gains of their run in order; the others become 0.0 (adding 0.0 changes nothing)
    {
        int head = 0;
#pragma unroll
        for (int k = 1; k < NP; k++) {
            if (k < n && ns[k] == ns[k - 1]) {
#pragma unroll
                for (int q = 0; q < NP; q++) if (q == head) g[q] += g[k];
                g[k] = 0.0;
            } else head = k;
        }
    }
    int jb[NP], rr[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) { jb[k] = (k < n) ? ns[k] / dt : 0x3fffffff; rr[k] = (k < n) ? ns[k] - jb[k] * dt : 0; }
    // samples in reach of a photon: start bin j touches samples j + lead .. j + lead + tlen - 1
    const int s_first = a.currents ? 0 : jb[0] + lead;
    int jmax = 0;
#pragma unroll
    for (int k = 0; k < NP; k++) if (k < n) jmax = jb[k] > jmax ? jb[k] : jmax;
    const int s_last = a.currents ? L - 1 : (jmax + lead + tlen - 1 < L - 1 ? jmax + lead + tlen - 1 : L - 1);
    TinyPrep q; q.n = n; q.s_first = s_first; q.s_last = s_last;
#pragma unroll
    for (int k = 0; k < NP; k++) { q.jb[k] = jb[k]; q.rr[k] = rr[k]; q.g[k] = g[k]; }
    return q;
}

template <bool FMA, int LANES, bool CUR, class Tap, class Sink>
__device__ __forceinline__ void tiny_tile_samples(const WfsDev &d, const PulseArgs &a, const TinyPrep &q, i64 idx, int sub, Tap tap, Sink sink)
{
    constexpr int tlen = 22, NP = TINY_MAX_PHOTONS;
    const int lead = tile_lead(d);
    for (int s = q.s_first + sub; s <= q.s_last; s += LANES) {
        double cur = 0.0;
#pragma unroll
        for (int k = 0; k < NP; k++) {
            const int kk = s - lead - q.jb[k];
            if (k < q.n && kk >= 0 && kk < tlen) cur = mac<FMA>(tap(q.rr[k], kk), q.g[k], cur);
        }
        if (CUR && a.currents) a.currents[a.cur_off[idx] + s] = cur;
        const i64 adc = adc_of(d, cur);
        if (adc != 0) sink(s, (i32)adc);
    }
}

template <bool FMA, int LANES, class Tap, class Sink>
__device__ __forceinline__ void tiny_tile_pulse(const WfsDev &d, const PulseArgs &a, const TileDesc &td, i64 idx, int sub, const double *s_cmax, Tap tap, Sink sink)
{
    const TinyPrep q = tiny_tile_prepare(d, a, td, sub, s_cmax);
    tiny_tile_samples<FMA, LANES, true>(d, a, q, idx, sub, tap, sink);
}

// A prepared tiny tile of a resident row (k_tile_assign -> k_row_pulse), in the 64 bytes of a TileDesc; n_neg = -photons sits where
// TileDesc::n does and tells the two apart.
struct __attribute__((aligned(64))) TinyDesc { double g[TINY_MAX_PHOTONS]; i32 dst, s_first, n_neg, s_last; u32 jr[TINY_MAX_PHOTONS]; };      // jr = start bin << 4 | ns remainder
static_assert(sizeof(TinyDesc) == 64 && sizeof(TileDesc) == 64 && offsetof(TinyDesc, n_neg) == offsetof(TileDesc, n), "descriptor layouts");

// Resident rows on: every live tile goes either into its row's list (descriptor written here, dst relative to the row's first
// sample) or onto the work list of its class -- the choice k_tile_geom cannot make, because rows exist only after k_groups.
__global__ void k_tile_assign(WfsDev d, GeomArgs a, DescArgs da, PulseArgs pa)
{
    const i64 tile = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = tile < a.n_tiles && a.tile_count[tile] > 0;
    int cls = 2; i64 nb = 0; i32 cnt = 0; bool listed = false;
    if (live) {
        const i64 set = tile / d.n_tpc; const i32 ch = (i32)(tile - set * d.n_tpc);
        const i64 t0 = a.set_t0[set];
        const TileWindow w = tile_window(d, t0, a.tile_tmin[tile], a.tile_tmax[tile]);
        nb = w.nb;
        cnt = a.tile_count[tile];
        const i64 ridx = (i64)a.cl_group[a.set_cluster[set]] * d.n_tpc + ch;
        const i64 first = a.res_toff[ridx];
        if (a.res_toff[ridx + 1] > first) {
            const i32 k = atomicSub(&a.res_cnt[ridx], 1) - 1;          // (the scan has consumed the counts: they serve as the rows' cursors)
            TileDesc t;
            t.off = da.tile_off[tile]; t.dst = w.left - (a.row_lo[ridx] - d.tw); t.rel0 = w.bin0 * d.dt - t0;
            t.G = d.gains[ch]; t.thr = d.thr_truth[ch];
            t.n = cnt; t.nb = (i32)nb; t.L = (i32)w.L; t.tile = (i32)tile;
            t.ch = ch; t.mode = da.set_mode[set];
            if (cnt <= TINY_MAX_PHOTONS && nb <= TINY_MAX_BINS) {       // (the tiny class of the work lists: the same tiles, the same order of their truth sums)
                // a handful of photons: everything that does not depend on the sample is done here, one LANE per tile (sorted and merged
                // photons, their start bins, the tile's truth sums) -- in k_row_pulse a whole wave would do it for one tile
                const TinyPrep q = tiny_tile_prepare(d, pa, t, 0, d.current_max);
                TinyDesc y;
                y.dst = (i32)t.dst; y.s_first = q.s_first; y.s_last = q.s_last; y.n_neg = -q.n;
#pragma unroll
                for (int j = 0; j < TINY_MAX_PHOTONS; j++) { y.g[j] = q.g[j]; y.jr[j] = ((u32)q.jb[j] << 4) | (u32)q.rr[j]; }
                *(TinyDesc *)&a.res_desc[first + k] = y;
            } else a.res_desc[first + k] = t;
        } else {
            cls = tile_class(a, cnt, nb);
            listed = !(a.tile_done && tile < a.n_done && a.tile_done[tile]);
        }
    }
    tile_list_append(a, listed, cls, nb, cnt, tile);
}

template <bool FMA>
__global__ __launch_bounds__(256) void k_pulse_tiny(WfsDev d, PulseArgs a, i64 n_tiny)
{
    constexpr int dt = WFS_DT, tlen = 22;
    __shared__ double sT[dt * tlen];                      // templates[r][k]
    __shared__ double s_cmax[dt];
    for (int i = threadIdx.x; i < dt * tlen; i += blockDim.x) sT[i] = d.templates[i];
    if (threadIdx.x < dt) s_cmax[threadIdx.x] = d.current_max[threadIdx.x];
    __syncthreads();
    // TINY_LANES lanes per tile: all of them load, sort and merge the tile's (at most 4) photons -- the same registers in each, no
    // exchange -- and share the tile's samples, lane j taking s_first + j, + TINY_LANES, ...: the adds of a tile land in runs of 64
    // bytes instead of 64 rows per instruction, and a wave's loop is as long as its longest tile divided by TINY_LANES.
    const i64 gtid = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const i64 idx = gtid / TINY_LANES; const int sub = (int)(gtid % TINY_LANES);
    if (idx >= n_tiny) return;
    const TileDesc td = a.desc[idx];
    i32 *dst = a.raw + td.dst;
    tiny_tile_pulse<FMA, TINY_LANES>(d, a, td, idx, sub, s_cmax, [&](int r_, int k_) { return sT[r_ * tlen + k_]; }, [&](int s_, i32 adc) { atomicAdd(&dst[s_], adc); });
}

// Medium tiles: at most 64 photons over any number of start bins -- the tiles of a small S2 (a few hundred to a few thousand
// electrons: ~30 photons per PMT over microseconds), far too wide for the counting-sort kernel below and far too empty for
// the dense kernel, whose cost goes with the samples (~600 x 220 multiply-adds for 30 photons x 22).  One WAVE per tile, no
// LDS traffic beyond the template table: lane = photon while the photons are loaded, sorted by time (bitonic network on
// keys ns << 6 | lane) and merged (equal ns: the first of the run takes the summed gain, the others 0.0, which add nothing);
// then lane = sample, block by block of 64: the photons that can reach the block are a contiguous range of the sorted
// list, their (bin, ns remainder, gain) are broadcast one at a time from the lane that holds them, and every sample in
// reach adds templates[r][k] * gain with a separate multiply and add, in ascending time: the arithmetic of add_current
// (pulse.py:276-318), the same bits as the other kernels.
struct __attribute__((aligned(16))) WavePhoton { i32 bin, row; double g; };       // start bin, first tap of its template row in sTz, merged gain
static_assert(sizeof(WavePhoton) == WAVE_PHOTON_BYTES, "row_pulse_lds sizes the waves' lists by it");
// (PW_U, WAVE_TZ_LEN: wfs_layout.h)
__device__ __forceinline__ void wave_tables_fill(const WfsDev &d, double *sTz, double *s_cmax)      // (every thread of the workgroup; a barrier follows)
{
    constexpr int dt = WFS_DT, tlen = 22;
    for (int i = threadIdx.x; i < dt * (tlen + 2); i += blockDim.x) { const int r = i / (tlen + 2), k = i - r * (tlen + 2) - 1; sTz[i] = (k >= 0 && k < tlen) ? d.templates[r * tlen + k] : 0.0; }
    if (threadIdx.x < dt) s_cmax[threadIdx.x] = d.current_max[threadIdx.x];
}

// The pulse of one tile made by one wave (see k_pulse_wave): sink(s, adc) receives the rounded, non-zero ADC counts of the tile's
// sample s, every lane a different sample.
template <bool FMA, bool CUR, class Sink>
__device__ __forceinline__ void wave_tile_pulse(const WfsDev &d, const PulseArgs &a, const TileDesc &td, i64 idx, WavePhoton *wph, const double *sTz,
                                                const double *s_cmax, int lane, Sink sink)
{
    constexpr int dt = WFS_DT, tlen = 22;
    const int n = td.n, L = td.L;
    const int lead = tile_lead(d);
    const bool v = lane < n;
    // ---- lane = photon
    const PhotonRec rec = a.ph[td.off + (v ? lane : 0)];
    const i32 ns0 = v ? (i32)(rec.t - td.rel0) : 0x7fffff;                  // ns relative to the tile's first start bin
    const u32 code = v ? rec.code : 0u;
    double g = 0.0;
    if (td.mode != 0) { if (v) g = a.ph_gain[td.off + lane]; }
    else {
        const double *spe_row = spe_row_of(d, td.ch);
        const double s1 = spe_row[code & 0xffffu], s2 = spe_row[code >> 16];
        g = td.G * s1;                                                       // (spe_gain, written out: td.G read at either use -- the
        if (code >> 16) g += td.G * s2;                                      //  helper holds it in two more SGPRs of k_row_pulse)
        if (!v) g = 0.0;
    }
    if (a.tile_truth) {        // pulse.py:229-271, photons in their order in the channel slice (= lane order)
        const bool is_dpe = v && (code >> 16) != 0;
        const i32 n_dpe = __popcll(ballot64(is_dpe));
        const bool above = v && truth_above(d, g, s_cmax[v ? ns0 % dt : 0], td.thr);
        const i32 n_trig = __popcll(ballot64(above)), n_trig_dpe = __popcll(ballot64(above && lane < n_dpe));
        const double tr = v ? (double)(ns0 + td.rel0) : 0.0;
        // (DPP: no LDS crossbar trips; every photon above the threshold -- the usual tile -- : the triggered area IS the area, same bits)
        const double sg = wave_sum(g), sgt = all64(!v || above) ? sg : wave_sum(above ? g : 0.0), st = wave_sum(tr), st2 = wave_sum(tr * tr);
        if (lane == 0) {
            double *o = a.tile_truth + (i64)td.tile * 8;
            o[0] = (double)n; o[1] = (double)n_dpe; o[2] = (double)n_trig; o[3] = (double)n_trig_dpe; o[4] = sg; o[5] = sgt; o[6] = st; o[7] = st2;
        }
    }
    // ---- ascending time: bitonic sort of the keys ns << 6 | lane (unique: a deterministic order), then the gains follow
    u32 key = ((u32)ns0 << 6) | (u32)lane;
    // (the photons sit in lanes 0 .. n - 1 and every other lane holds a larger key: with n <= 32 (16) the merges of 64 (32) lanes have
    // nothing to do -- the lower half is sorted ascending after the stages before them, which is all that is read)
    // (the exchanges with lane ^ 1, 2, 8 are DPP moves, ^ 4, 16 swizzles: 19 of the 21 steps without an LDS address, wfs_device.h)
    key = bitonic_merge<2>(key, lane); key = bitonic_merge<4>(key, lane); key = bitonic_merge<8>(key, lane); key = bitonic_merge<16>(key, lane);
    if (n > 16) { key = bitonic_merge<32>(key, lane); if (n > 32) key = bitonic_merge<64>(key, lane); }      // wave-uniform
    const int src = (int)(key & 63u);
    i32 ns = (i32)(key >> 6);
    g = __shfl(g, src, 64);
    // runs of equal ns (pulse.py:303-313): the head of a run collects the gains of the run in order, the others become 0.0
    {
        const i32 prev = __shfl_up(ns, 1, 64);
        const bool head = lane == 0 || prev != ns;
        if (any64(!head && lane < n)) {
            double tot = g;
            for (int step = 1; step < 64; step++) {
                const i32 nsq = __shfl_down(ns, step, 64); const double gq = __shfl_down(g, step, 64);
                const bool same = lane + step < n && nsq == ns;
                if (!any64(head && same)) break;
                if (head && same) tot += gq;
            }
            g = head ? tot : 0.0;
        }
    }
    const i32 bin = lane < n ? ns / dt : 0x3fffffff, r = lane < n ? ns - (ns / dt) * dt : 0;
    if (lane < PW_U) wph[64 + lane] = WavePhoton{0x3fffffff, 1, 0.0};
    wph[lane] = WavePhoton{bin, r * (tlen + 2) + 1, g};    // (read back by every lane of this wave: one 16-byte LDS broadcast per photon
                                                          //  instead of three readlanes and their scalar unpacking on the vector unit)
    // ---- lane = sample.  Live samples: s' = 0 .. nb + 20 (sample lead + s' of the tile sees the start bins s' - 21 .. s').
    // Blocks of 64 samples start where something lands: behind a block the next one begins at the first start bin that can still
    // reach a sample not yet written (a photon of the thin tail of an S2 is alone in its 22 samples; whole blocks between the
    // photons are skipped).  Inside a block every sample walks the photons in reach, in ascending time; sTz has a zero tap on
    // either side of every template row, so a photon out of a sample's reach adds +0.0, which changes nothing (no exec masking).
    const int n_live = td.nb + tlen - 1;
    if (CUR && a.currents) for (int s = lane; s < L; s += 64) a.currents[a.cur_off[idx] + s] = 0.0;
    int s0 = 0;
    while (s0 < n_live) {
        // sorted photons with a start bin in [s0 - 21, s0 + 63]: a contiguous range [q_lo, q_hi) of lanes
        const int q_lo = __popcll(ballot64(bin < s0 - (tlen - 1))), q_hi = __popcll(ballot64(bin <= s0 + 63));
        if (q_lo >= n) break;                                 // nothing reaches s0 or anything behind it
        if (q_hi == q_lo) { s0 = __builtin_amdgcn_readlane(bin, q_lo); continue; }      // (bin[q_lo] > s0 + 63: the next block starts at that photon)
        const int sp = s0 + lane;
        double c = 0.0;
        // (PW_U photons per trip, their LDS reads in flight together; a photon past q_hi is out of reach of this block -- or one of
        // the pad entries behind the list -- and adds +0.0)
        for (int q = q_lo; q < q_hi; q += PW_U) {
            WavePhoton w[PW_U]; double tap[PW_U];
#pragma unroll
            for (int u = 0; u < PW_U; u++) w[u] = wph[q + u];
#pragma unroll
            for (int u = 0; u < PW_U; u++) { int kk = sp - w[u].bin; kk = kk < -1 ? -1 : (kk > tlen ? tlen : kk); tap[u] = sTz[w[u].row + kk]; }
#pragma unroll
            for (int u = 0; u < PW_U; u++) c = mac<FMA>(tap[u], w[u].g, c);
        }
        if (sp < n_live) {
            if (CUR && a.currents) a.currents[a.cur_off[idx] + lead + sp] = c;
            const double x = adc_round(d, c);
            // (|x| < 2^31 unless a current is absurd: the one-instruction conversion; the general one otherwise, same value)
            const i32 adc = fabs(x) < 2147483648.0 ? -(i32)x : (i32)(-(i64)x);
            if (adc != 0) sink(lead + sp, adc);
        }
        s0 += 64;
    }
}

template <bool FMA>
__global__ __launch_bounds__(256) void k_pulse_wave(WfsDev d, PulseArgs a, i64 n_wave)
{
    constexpr int dt = WFS_DT;
    __shared__ double sTz[WAVE_TZ_LEN];                   // templates[r][k] with a zero tap in front of and behind every row
    __shared__ double s_cmax[dt];
    __shared__ WavePhoton s_ph[4][64 + PW_U];             // the sorted, merged photons of each wave's tile, pad entries that reach nothing behind them
    wave_tables_fill(d, sTz, s_cmax);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const i64 idx = (i64)blockIdx.x * 4 + wave_in_block();       // (an SGPR: the tile descriptor stays scalar)
    WavePhoton *wph = s_ph[wave_in_block()];
    if (idx >= n_wave) return;                            // wave-uniform
    const TileDesc td = a.desc[idx];
    i32 *dst = a.raw + td.dst;
    wave_tile_pulse<FMA, true>(d, a, td, idx, wph, sTz, s_cmax, lane, [&](int s_, i32 adc) { atomicAdd(&dst[s_], adc); });
}

// Sparse form of the same computation, for tiles with few photons per start bin (every S1, S2s up to ~10^6 PE):
// the photons are counting-sorted by their ns in LDS (one counter per ns of the tile, two u16 counters per dword),
// photons of equal ns are merged (first of the run gets the summed gain, the others 0.0, which add nothing) --
// i.e. the sorted, merged photon list add_current walks (pulse.py:297-318) -- and every sample gathers its
// contributions from the contiguous slice of that list in ascending time.  Same bits as the dense kernel.
// (SPARSE_PPT photons per thread held in registers, tile photons <= TPB * SPARSE_PPT: wfs_layout.h)
template <int TPB, bool FMA>
__global__ __launch_bounds__(TPB) void k_pulse_sparse(WfsDev d, PulseArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tlen = d.tlen; constexpr int dt = WFS_DT;      // sample_duration is 10 ns (checked by wfs_create)
    // T replicas: 8 copies of the templates, rows padded to tlen + 2 with a zero tap on either side, copies offset by
    // 4 bank pairs so that the 64 lanes' data-dependent template reads spread over the LDS banks
    constexpr int TROW = 24, TREP = SPARSE_TREP, NREP = 1;       // requires tlen == 22 (tiny tiles: bank conflicts do not matter)
    const SparseLds o = sparse_lds(a.NP, a.W, TPB);
    double *cg = (double *)(smem + o.cg);                // [NP] merged gain of the sorted photons
    double *red = (double *)(smem + o.red);              // [TPB / 64][8]
    i32 *ctoff = (i32 *)(smem + o.ctoff);                // [NP] r * TROW - start bin
    unsigned short *boff = (unsigned short *)(smem + o.boff);          // [dt * W + 2] exclusive offsets
    u32 *wsum = (u32 *)(smem + o.wsum);                  // [TPB / 64]
    u32 *cnt = (u32 *)(smem + o.cnt);                    // [dt * W / 2] packed u16 pairs: photons per ns ...
    double *Trep = (double *)(smem + o.cnt);             // ... later reused for [NREP][TREP] template copies: one region, sized for the larger
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    __shared__ double s_cmax[WFS_DT];                    // pulse.py:32 current_max (see k_pulse)
    if (tid < WFS_DT) s_cmax[tid] = d.current_max[tid];

    const TileDesc td = a.desc[blockIdx.x];              // block-uniform: scalar loads
    const i64 tile = td.tile; const i32 n = td.n; const i64 off = td.off;
    const int nb = td.nb, nns = nb * dt;
    const int L = td.L;
    const int lead = tile_lead(d);
    const int mode = td.mode;
    const double G = td.G;
    const double *spe_row = spe_row_of(d, td.ch);
    const double thr = td.thr;
    const i32 rel0 = (i32)td.rel0;                       // ns of the tile's first start bin relative to t0

    // ---- all photons of the tile into registers: independent loads, all in flight together
    i32 ns[SPARSE_PPT]; u32 code[SPARSE_PPT]; double gain[SPARSE_PPT];
    const int kmax = (n + TPB - 1) / TPB;                // block-uniform: registers beyond it stay empty
#pragma unroll
    for (int k = 0; k < SPARSE_PPT; k++) {
        const i32 p = tid + k * TPB;
        const bool v = p < n;
        const PhotonRec rec = a.ph[off + (v ? p : 0)];
        ns[k] = v ? rec.t - rel0 : -1;
        code[k] = v ? rec.code : 0u;
        gain[k] = (v && mode != 0) ? a.ph_gain[off + p] : 0.0;
    }
    if (mode == 0) {
        double s1[SPARSE_PPT], s2[SPARSE_PPT];
#pragma unroll
        for (int k = 0; k < SPARSE_PPT; k++) {
            s1[k] = 0; s2[k] = 0;
            if (k < kmax) { s1[k] = spe_row[code[k] & 0xffffu]; if (any64((code[k] >> 16) != 0)) s2[k] = spe_row[code[k] >> 16]; }
        }
#pragma unroll
        for (int k = 0; k < SPARSE_PPT; k++) gain[k] = spe_gain(G, s1[k], s2[k], code[k]);
    }
    for (int i = tid; i < (nns + 1) / 2; i += TPB) cnt[i] = 0;
    i32 n_dpe_tile = 0;
    {                         // number of DPE photons of the tile (truth quirk pulse.py:255)
        i32 c = 0;
#pragma unroll
        for (int k = 0; k < SPARSE_PPT; k++) c += (code[k] >> 16) != 0;
        n_dpe_tile = block_sum_u32<TPB>(c, wsum);
    }
    __syncthreads();

    // ---- pass 1: photons per ns, truth accumulators (pulse.py:229-271)
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // n, n_dpe, n_trig, n_trig_dpe, sum g, sum g trig, sum t, sum t^2
#pragma unroll
    for (int k = 0; k < SPARSE_PPT; k++) {
        if (ns[k] < 0) continue;
        atomicAdd(&cnt[ns[k] >> 1], 1u << ((ns[k] & 1) * 16));
        const int r = ns[k] % dt;
        const bool above = truth_above(d, gain[k], s_cmax[r], thr);
        truth_add(acc, gain[k], above, (code[k] >> 16) != 0, tid + k * TPB < n_dpe_tile, (double)(ns[k] + rel0));
    }
    __syncthreads();

    // ---- exclusive scan of the per-ns counts -> boff[0, nns]
    {
        const int C = (nns + TPB - 1) / TPB;
        const int j0 = tid * C;
        u32 sum = 0;
        for (int k = 0; k < C; k++) { int j = j0 + k; if (j < nns) sum += (cnt[j >> 1] >> ((j & 1) * 16)) & 0xffffu; }
        u32 incl = sum;
        for (int o = 1; o < 64; o <<= 1) { u32 t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
        if (lane == 63) wsum[wid] = incl;
        __syncthreads();
        u32 run = incl - sum;
        for (int w = 0; w < wid; w++) run += wsum[w];
        for (int k = 0; k < C; k++) { int j = j0 + k; if (j < nns) { boff[j] = (unsigned short)run; run += (cnt[j >> 1] >> ((j & 1) * 16)) & 0xffffu; } }
        if (tid == TPB - 1) boff[nns] = (unsigned short)n;
        __syncthreads();
        for (int i = tid; i < (nns + 1) / 2; i += TPB) cnt[i] = 0;
        __syncthreads();
    }

    // ---- pass 2: place in time order
#pragma unroll
    for (int k = 0; k < SPARSE_PPT; k++) {
        if (ns[k] < 0) continue;
        const u32 old = atomicAdd(&cnt[ns[k] >> 1], 1u << ((ns[k] & 1) * 16));
        const u32 pos = boff[ns[k]] + ((old >> ((ns[k] & 1) * 16)) & 0xffffu);
        cg[pos] = gain[k]; ctoff[pos] = (ns[k] % dt) * TROW - ns[k] / dt;
    }
    __syncthreads();

    // ---- merge photons of equal ns (pulse.py:303-313)
    for (int j = tid; j < nns; j += TPB) {
        const int q0 = boff[j], m = (int)boff[j + 1] - q0;
        if (m >= 2) {
            double tot = cg[q0];
            for (int q = 1; q < m; q++) { tot += cg[q0 + q]; cg[q0 + q] = 0.0; }
            cg[q0] = tot;
        }
    }
    __syncthreads();

    // ---- templates into LDS (the counters are dead now)
    for (int i = tid; i < NREP * TREP; i += TPB) {
        const int c = i / TREP, x = i - c * TREP, r = x / TROW, kk = x - r * TROW;
        Trep[i] = (x < dt * TROW && kk >= 1 && kk <= tlen) ? d.templates[r * tlen + kk - 1] : 0.0;
    }
    __syncthreads();

    // ---- gather: two samples per lane; sample s <- photons of start bins [s - lead - (tlen-1), s - lead], ascending time
    i32 *dst = a.raw + td.dst;
    for (int sa = 2 * tid; sa < L; sa += 2 * TPB) {
        int jlo = sa - lead - (tlen - 1), jhi = sa + 1 - lead;
        if (jlo < 0) jlo = 0;
        if (jhi > nb - 1) jhi = nb - 1;
        double cur0 = 0.0, cur1 = 0.0;
        if (jhi >= jlo) {
            const int q1 = boff[(jhi + 1) * dt];
            // k + 1 of sample sa for a photon in start bin j is (sa - lead - j) + 1 in [0, tlen]; sample sa + 1 reads the next tap
            const double *Ts = Trep + (lane & (NREP - 1)) * TREP + (sa - lead + 1);
            int q = boff[jlo * dt];
            for (; q + 2 <= q1; q += 2) {
                const i32 o0 = ctoff[q], o1 = ctoff[q + 1];
                const double g0 = cg[q], g1 = cg[q + 1];
                cur0 = mac<FMA>(Ts[o0], g0, cur0); cur1 = mac<FMA>(Ts[o0 + 1], g0, cur1);
                cur0 = mac<FMA>(Ts[o1], g1, cur0); cur1 = mac<FMA>(Ts[o1 + 1], g1, cur1);
            }
            if (q < q1) { const i32 o0 = ctoff[q]; const double g0 = cg[q]; cur0 = mac<FMA>(Ts[o0], g0, cur0); cur1 = mac<FMA>(Ts[o0 + 1], g0, cur1); }
        }
        if (a.currents) { a.currents[a.cur_off[blockIdx.x] + sa] = cur0; if (sa + 1 < L) a.currents[a.cur_off[blockIdx.x] + sa + 1] = cur1; }
        const i64 adc0 = adc_of(d, cur0), adc1 = adc_of(d, cur1);
        if (adc0 != 0) atomicAdd(&dst[sa], (i32)adc0);
        if (adc1 != 0 && sa + 1 < L) atomicAdd(&dst[sa + 1], (i32)adc1);
    }

    if (a.tile_truth) {
        // (wave_sum: the order of wave_tile_pulse -- a tile of this class holds at most 32 photons, photon p in lane p of the first wave,
        // so its f64 truth sums are the same bits whether this kernel, k_pulse_wave or k_row_pulse made the tile)
        truth_wave_dpp(acc);
        truth_store_block<TPB>(acc, red, a.tile_truth + tile * 8);
    }
}

// Truth accumulators of a pulse set (pulse.py:229-271 add_truth: totals, bottom-array totals; rawdata.py:330-345 photon
// time moments) from the per-tile partial sums, one wave per set.  Channels are summed in a fixed order (lane, then the
// DPP tree of wave_sum), so the result does not depend on the order the tiles were processed in.
struct TruthArgs { i64 n_sets; const i32 *tile_count, *tile_tmin, *tile_tmax; const i64 *set_t0; const double *tile_truth;
                   double *truth; i64 *tminmax; };
__global__ __launch_bounds__(256) void k_truth_reduce(WfsDev d, TruthArgs a)
{
    const i64 set = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (set >= a.n_sets) return;
    double v[15];
#pragma unroll
    for (int q = 0; q < 15; q++) v[q] = 0.0;
    i64 tmin = I64_MAX, tmax = I64_MIN;
    const i64 t0 = a.set_t0[set];
    for (int ch = lane; ch < d.n_tpc; ch += 64) {
        const i64 tile = set * d.n_tpc + ch;
        if (a.tile_count[tile] <= 0) continue;
        const double *p = a.tile_truth + tile * 8;
        const double G = d.gains[ch];
        const double vals[6] = {p[0], p[0] + p[1], p[2], p[2] + p[3], p[4] / G, p[5] / G};
        const bool bottom = ch >= d.n_top && ch <= d.last_bottom;
#pragma unroll
        for (int q = 0; q < 6; q++) { v[q] += vals[q]; if (bottom) v[6 + q] += vals[q]; }
        v[12] += p[0]; v[13] += p[6]; v[14] += p[7];
        const i64 lo = t0 + a.tile_tmin[tile], hi = t0 + a.tile_tmax[tile];
        tmin = lo < tmin ? lo : tmin; tmax = hi > tmax ? hi : tmax;
    }
#pragma unroll
    for (int q = 0; q < 15; q++) v[q] = wave_sum(v[q]);         // (DPP: a fixed order, no LDS crossbar trips -- 180 of them per set otherwise)
    for (int o = 32; o > 0; o >>= 1) {
        const i64 lo = __shfl_down(tmin, o, 64), hi = __shfl_down(tmax, o, 64);
        tmin = lo < tmin ? lo : tmin; tmax = hi > tmax ? hi : tmax;
    }
    if (lane == 0) {
        for (int q = 0; q < 15; q++) a.truth[set * 16 + q] = v[q];
        a.tminmax[set * 2] = tmin; a.tminmax[set * 2 + 1] = tmax;
    }
}

// ------------------------------------------------------------------------------------------------ ZLE + records
struct ZleArgs {
    const i32 *active_rows; i64 n_active_rows;
    const i64 *row_lo, *row_hi, *acc_off; const i32 *raw;
    const i64 *grp_left, *grp_ixrand;
    const i64 *itv_off;
    i64 *itv_left, *itv_right; i32 *itv_n, *row_nrec;
    const i64 *rec_off;          // per row slot: first record
    uint8_t *records; i64 rec_capacity;
    i32 *row_dbg; const i64 *row_dbg_off;   // debug: finished rows
    i32 spr;                     // samples per record
    struct RowDesc *desc;        // [n_active_rows] everything a row's wave needs, prepared by k_row_desc
    const u32 *rec_dest;         // record order by (time, channel): slot of record r in the output (nullptr: row order)
    u64 *rec_key; u32 *rec_val; WfsScal *key_base; // k_rec_keys: sort key (sample - key_base->key_origin) << 12 | channel, and the record index; the scalar block when the records are sorted, else nullptr
    const i32 *tile_done, *row_cnt, *row_tile; const i32 *ins_bcap; const i64 *ins_boff; const i32 *tbuf; i64 n_done;      // rows read from a tile buffer in place (wfs_tilegen.h)
    // resident rows (k_row_pulse): the rows behind the first n_front of the row list; their finished 16-bit samples
    i64 n_front, n_short, rows_cap; const i64 *res_toff, *fin_off; int16_t *fin; const i32 *res_long; struct ResRow *res_rows;
    struct PackDesc *pdesc;      // [n_active_rows] what k_pack needs of a row, in one scalar load (k_pack_desc)
    // sum rows (k_sum_signal): range per window, first sample of the window's row behind raw[sum_base]
    const i64 *sum_lo, *sum_hi, *sum_off; i64 sum_base;
    // full readout: the rows without a pulse (k_row_empty) behind the n_res resident rows of the row list; their finished samples
    // are fin[fin_base + fr_off[row slot] ..], their range is the window's (grp_lo / grp_hi)
    i64 n_res, fin_base; const i32 *empty_rows; const i64 *fr_off, *grp_lo, *grp_hi;
};

// One 64-byte descriptor per active row (thread per row: the divisions and the five dependent look-ups of a row are
// done 64 rows at a time instead of once per wave; with 10^7 short S1 rows the per-row prologue was most of k_zle / k_pack)
struct __attribute__((aligned(64))) RowDesc {
    i64 acc_off;                 // first accumulated sample of the row in raw[]
    i64 row_abs;                 // absolute sample index of the row's first sample
    i64 ixr;                     // noise offset of the row's window
    i64 itv_base;                // first interval slot of the row
    i64 thr;                     // ZLE threshold of the channel
    i64 idx;                     // row slot (group * row_slots + slot): index of itv_n / row_nrec / rec_off
    i32 len, channel, he, src;   // src 1: acc_off points into the tile buffers (a row made by one k_s2_tile tile); 2: into the finished
                                 // 16-bit samples of the resident rows (k_row_pulse)
};

struct __attribute__((aligned(16))) ResRow { i64 t0; i32 n, pad; };       // a resident row's tiles: res_desc[t0 .. t0 + n)

__global__ void k_row_desc(WfsDev d, ZleArgs a)
{
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_active_rows) return;
    if (r >= a.n_front + a.n_res) {
        // full readout: the rows without a pulse, behind the resident rows and read like them (src 2) -- the window's range, finished
        // samples behind those of the resident rows
        const i64 idx = a.empty_rows[r - a.n_front - a.n_res];
        const RowSlot rs = row_slot(d, idx);
        const RowSpan sp = full_row_span(a.grp_lo[rs.g], a.grp_hi[rs.g], d.tw);
        RowDesc q;
        q.acc_off = a.fin_base + a.fr_off[idx]; q.row_abs = sp.left; q.ixr = a.grp_ixrand[rs.g]; q.itv_base = a.itv_off[idx];
        q.thr = d.thr_zle[rs.channel]; q.idx = idx; q.len = (i32)sp.len; q.channel = rs.channel; q.he = rs.he ? 1 : 0; q.src = 2;
        a.desc[r] = q;
        if (a.key_base) { atomicMin(&a.key_base->key_origin, q.row_abs); atomicMax(&a.key_base->key_end, q.row_abs + (i64)q.len); }
        return;
    }
    // row list order: accumulator rows | short resident rows (from the end of active_rows backwards, k_row_len) | long resident rows
    // | rows without a pulse (full readout)
    const i64 idx = r < a.n_front ? a.active_rows[r] : (r < a.n_front + a.n_short ? a.active_rows[a.rows_cap - 1 - (r - a.n_front)] : a.res_long[r - a.n_front - a.n_short]);
    const RowSlot rs = row_slot(d, idx);
    const i64 g = rs.g;
    if (rs.sum) {
        // the window's sum row: an accumulator row (src 0) behind the accumulators proper, times int(he_factor) when it is finished
        // like an HE row (rawdata.py:242, 251-254), noise column and threshold of the sum channel
        RowDesc q;
        q.acc_off = a.sum_base + a.sum_off[g]; q.row_abs = a.sum_lo[g] - d.tw; q.ixr = a.grp_ixrand[g]; q.itv_base = a.itv_off[idx];
        q.thr = d.thr_zle[rs.channel]; q.idx = idx; q.len = (i32)row_span(a.sum_lo[g], a.sum_hi[g], d.tw).len;
        q.channel = rs.channel; q.he = 1; q.src = 0;
        a.desc[r] = q;
        if (a.key_base) { atomicMin(&a.key_base->key_origin, q.row_abs); atomicMax(&a.key_base->key_end, q.row_abs + (i64)q.len); }
        return;
    }
    const bool he = rs.he; const i32 channel = rs.channel;
    const i64 ridx = g * d.n_tpc + rs.acc_ch;
    RowDesc q;
    q.acc_off = a.acc_off[ridx]; q.row_abs = a.row_lo[ridx] - d.tw; q.ixr = a.grp_ixrand[g]; q.itv_base = a.itv_off[idx];
    q.src = 0;
    if (r >= a.n_front) {
        q.acc_off = a.fin_off[ridx]; q.src = 2;
        const i64 t0 = a.res_toff[ridx];
        a.res_rows[r - a.n_front] = ResRow{t0, (i32)(a.res_toff[ridx + 1] - t0), 0};
    }
    if (!d.full_readout && row_is_direct(a.tile_done, a.n_done, a.row_cnt, a.row_tile, ridx)) {
        const i32 tile = a.row_tile[ridx]; const i32 ins = tile / d.n_tpc;
        q.acc_off = a.ins_boff[ins] + (i64)(tile - ins * d.n_tpc) * a.ins_bcap[ins]; q.src = 1;
    }
    q.thr = d.thr_zle[channel]; q.idx = idx; q.len = (i32)row_span(a.row_lo[ridx], a.row_hi[ridx], d.tw).len;
    q.channel = channel; q.he = he ? 1 : 0;
    a.desc[r] = q;
    if (a.key_base) { atomicMin(&a.key_base->key_origin, q.row_abs); atomicMax(&a.key_base->key_end, q.row_abs + (i64)q.len); }
}

// The noise model (wfs_set_noise_model): noise(ch, t) = vmin + alias_sample(cells[ch], word t & 3 of the Philox call of
// (t >> 2, ch)), t the absolute sample index -- integer arithmetic from the random word to the ADC value.  cells: those of the channel.
__device__ __forceinline__ i32 noise_model_sample(const WfsDev &d, const uint2 *cells, i32 channel, i64 t)
{
    const AliasTab tab{cells, d.nm_vmin, d.nm_shift};
    const u32x4 a = noise_quad(d.k0, d.k1, channel, t >> 2);
    const u32 m = (u32)t & 3u;
    return alias_sample(tab, m == 0 ? a.x : (m == 1 ? a.y : (m == 2 ? a.z : a.w)));      // (word_of, written out: the call costs k_pack<3> four registers)
}
// Samples t0 + i .. t0 + i + 3 of a lane whose i is a multiple of four and whose t0 is wave-uniform: the four words lie in the lane's
// aligned call and, unless t0 is aligned itself, the one behind it -- which of them is the same for the whole wave (t0 & 3), so the
// second call sits behind a scalar branch and the words are picked without a select.  One call per four samples for aligned rows, two
// otherwise.
__device__ __forceinline__ void noise_model_four(const WfsDev &d, const uint2 *cells, i32 channel, i64 t0, i32 i, i32 *out)
{
    const AliasTab tab{cells, d.nm_vmin, d.nm_shift};
    const i64 q = (t0 + i) >> 2;
    const u32 m = (u32)t0 & 3u;
    const u32x4 a = noise_quad(d.k0, d.k1, channel, q);
    u32 w[4] = {a.x, a.y, a.z, a.w};
    if (m != 0) {
        const u32x4 b = noise_quad(d.k0, d.k1, channel, q + 1);
        if (m == 1) { w[0] = a.y; w[1] = a.z; w[2] = a.w; w[3] = b.x; }
        else if (m == 2) { w[0] = a.z; w[1] = a.w; w[2] = b.x; w[3] = b.y; }
        else { w[0] = a.w; w[1] = b.x; w[2] = b.y; w[3] = b.z; }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) out[j] = alias_sample(tab, w[j]);
}

// A stream of the coloured model (wfs_set_noise_colour): a channel, or a common stream shared by a group of channels.  Its
// row of the alias cells, of the taps and of the slow amplitudes (the common streams' rows follow the channels'), the id that takes
// the channel's place in its Philox counters, and the sites of its whites and of its slow levels.  (taps / amp: of a view that has
// them; nobody reads the others.)
struct NoiseStream {
    AliasTab tab; const i32 *taps, *amp; u32 id, site_white, site_slow;
    __device__ __forceinline__ NoiseStream(const WfsDev &d, i32 n /* channel, or group of a common stream */, bool common)
    {
        const i64 row = common ? d.noise_channels + n : n;
        tab = AliasTab{d.nm_cells + row * d.nm_cells_per_ch, d.nm_vmin, d.nm_shift};
        taps = d.nc_taps + row * NC_TAP_STRIDE + NC_TAP_PAD; amp = d.ns_amp + row * NS_MAX_LEVELS;
        id = (u32)n; site_white = common ? SITE_NOISE_COMMON : SITE_NOISE_SAMPLE; site_slow = common ? SITE_NOISE_SLOW_COMMON : SITE_NOISE_SLOW;
    }
    // the probes address a stream by its row: a channel, or (row >= noise_channels) a common stream
    static __device__ __forceinline__ NoiseStream of_row(const WfsDev &d, i32 row) { const bool common = row >= d.noise_channels; return NoiseStream(d, common ? row - d.noise_channels : row, common); }
};

// The coloured model (noise kind 4): every stream r -- the channels, then the common streams -- has a white sequence w(r, t) as above
// (a common stream g under the counter (.., g, SITE_NOISE_COMMON)) and L Q16 taps;
//   F(r, t) = sum_k taps[r][k] w(r, t - k),   noise(ch, t) = (F(ch, t) + ((i64)mix[ch] F(common of ch, t) >> 16) + 32768) >> 16,
// all in integers: the host has checked that F fits 30 bits (wfs_set_noise_colour).
//
// Single-sample form: a lane draws the quads that cover t - L + 1 .. t itself (up to (L + 6) / 4 calls).  No cross-lane traffic, so it
// may be called from divergent code and with any t per lane: the record-ordered lanes of k_pack, the 64-sample chunks of k_zle's
// general path, finish_sample.
__device__ __forceinline__ i32 colour_stream_sample(const WfsDev &d, const NoiseStream &st, i64 t)
{
    const i64 q1 = t >> 2;
    i32 F = 0;
#pragma nounroll
    for (i64 q = (t - (d.nc_n_taps - 1)) >> 2; q <= q1; q++) {
        const u32x4 a = noise_quad_of(d.k0, d.k1, st.id, st.site_white, q);
        const u32 w[4] = {a.x, a.y, a.z, a.w};
        const i32 k0 = (i32)(t - 4 * q);                       // distance of the quad's first white: -3 .. L + 2, inside the zero pads
#pragma unroll
        for (int c = 0; c < 4; c++) F += st.taps[k0 - c] * alias_sample(st.tab, w[c]);
    }
    return F;
}
// The slow levels (wfs_set_noise_slow, noise kind 5): level j of stream r is a sequence of knots 2^s_j samples apart, knot m
// drawn from the stream's own alias cells with word m & 3 of the Philox call of (m >> 2, channel | group, SITE_NOISE_SLOW(_COMMON) + j),
// joined by linear interpolation in integers:
//   m = t >> s_j, f = t & (2^s_j - 1), P0 = amp[r][j] knot(m), P1 = amp[r][j] knot(m + 1),  S(r, t) = sum_j P0 + (((i64)(P1 - P0) f) >> s_j)
// and F'(r, t) = F(r, t) + S(r, t) takes the place of F in the coloured model: the host has checked that F' fits 30 bits.
//
// Single-sample form: a lane draws its own two knots per level (one call, two when the pair straddles a quad).  No cross-lane traffic:
// legal in divergent code and with any t and row per lane, like colour_stream_sample.
__device__ __forceinline__ i32 slow_stream_sample(const WfsDev &d, const NoiseStream &st, i64 t)
{
    i32 S = 0;
#pragma nounroll
    for (int j = 0; j < d.ns_levels; j++) {
        const i32 a = st.amp[j];
        if (a == 0) continue;
        const i32 s = d.ns_shift[j];
        const i64 m = t >> s;
        const i32 f = (i32)((u32)t & ((1u << s) - 1u));         // (s <= 30: the phase fits 32 bits, and the product below is one 32 x 32 -> 64 multiply)
        const u32x4 q = noise_quad_of(d.k0, d.k1, st.id, st.site_slow + (u32)j, m >> 2);
        const int c = (int)((u32)m & 3u);
        const u32 w0 = word_of(q, c);
        u32 w1 = word_of(q, c + 1);                             // (of c = 3: the next call's first)
        if (c == 3) w1 = noise_quad_of(d.k0, d.k1, st.id, st.site_slow + (u32)j, (m >> 2) + 1).x;
        const i32 P0 = a * alias_sample(st.tab, w0), P1 = a * alias_sample(st.tab, w1);
        S += P0 + (i32)(((i64)(P1 - P0) * (i64)f) >> s);
    }
    return S;
}
// Four-sample form: lane l of a wave takes samples tb + 4 l .. tb + 4 l + 3, tb wave-uniform.  With s >= NS_MIN_SHIFT the 256 samples of
// the wave touch at most 18 knots of a level, which lie in the NS_QUADS aligned quads from qb_j = (tb >> s_j) >> 2 on: lane 8 j + k draws
// quad qb_j + k of level j and alias-samples it -- ONE Philox call per lane for all levels together -- and its four knots travel as two
// packed words.  Four consecutive samples cross at most one knot, so a lane needs three consecutive knots of a level; they sit in one
// or two neighbouring quads, fetched by four ds_bpermute per level with an amplitude (levels with amplitude 0 are skipped: the
// amplitude is the row's, wave-uniform).
// ALL 64 LANES MUST BE EXECUTING, as for colour_stream_four: call it before any per-lane bound.
__device__ __forceinline__ void slow_stream_four(const WfsDev &d, const NoiseStream &st, i64 tb, int lane, i32 *S)
{
    const int nl = d.ns_levels;
    const int lj = (lane >> 3) < nl ? (lane >> 3) : nl - 1;    // (the lanes of levels that are not there repeat the last one; nobody reads them)
    const i64 qown = ((tb >> d.ns_shift[lj]) >> 2) + (lane & 7);
    const u32x4 a = noise_quad_of(d.k0, d.k1, st.id, st.site_slow + (u32)lj, qown);
    const u32 p0 = alias_pair(st.tab, a.x, a.y), p1 = alias_pair(st.tab, a.z, a.w);
    const i64 t0 = tb + 4 * lane;
    S[0] = S[1] = S[2] = S[3] = 0;
#pragma nounroll
    for (int j = 0; j < nl; j++) {                              // (wave-uniform, and so is the skip)
        const i32 aq = __builtin_amdgcn_readfirstlane(st.amp[j]);
        if (aq == 0) continue;
        const i32 s = __builtin_amdgcn_readfirstlane(d.ns_shift[j]);
        const i64 m0 = t0 >> s;
        const i32 k0 = (i32)(m0 - (((tb >> s) >> 2) << 2));    // the lane's first knot among the level's 4 NS_QUADS: 0 .. 19, the third at most 21
        const i32 qa = k0 >> 2, qc = (k0 + 2) >> 2;
        const i32 src_a = (8 * j + qa) << 2, src_c = (8 * j + qc) << 2;
        const u32 a0 = (u32)__builtin_amdgcn_ds_bpermute(src_a, (int)p0), a1 = (u32)__builtin_amdgcn_ds_bpermute(src_a, (int)p1);
        const u32 c0 = (u32)__builtin_amdgcn_ds_bpermute(src_c, (int)p0), c1 = (u32)__builtin_amdgcn_ds_bpermute(src_c, (int)p1);
        i32 P[3];
#pragma unroll
        for (int u = 0; u < 3; u++) {
            const i32 k = k0 + u;
            const bool first = (k >> 2) == qa;
            const u32 w = (k & 2) ? (first ? a1 : c1) : (first ? a0 : c0);
            P[u] = aq * ((k & 1) ? (i32)w >> 16 : (i32)(int16_t)w);
        }
        const u32 mask = (1u << s) - 1u, f0 = (u32)t0 & mask;    // the phase of the lane's first sample; the others in 32 bits from it
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const bool next = f0 + (u32)c > mask;               // (c < 4 <= 2^s: at most one knot is crossed)
            const i32 f = (i32)((f0 + (u32)c) & mask);
            const i32 Pa = next ? P[1] : P[0], Pb = next ? P[2] : P[1];
            S[c] += Pa + (i32)(((i64)(Pb - Pa) * (i64)f) >> s);
        }
    }
}

// The streams of a channel are walked by a loop that stays a loop (the channel's own with gain 1.0, then its common stream with mix):
// one copy of the draws per call site, whatever the number of streams -- unrolled and interleaved they took every register there is.
// (SLOW: kind 5, the slow levels of every stream added to its F.)
template <bool SLOW = false>
__device__ __forceinline__ i32 noise_colour_sample(const WfsDev &d, i32 channel, i64 t)
{
    const i32 g = d.nc_group ? d.nc_group[channel] : -1;        // (wave-uniform wherever a wave works on one row)
    const i32 mix = g >= 0 ? d.nc_mix[channel] : 0;
    i32 sum = 0;
#pragma nounroll
    for (int s = 0; s < (g >= 0 ? 2 : 1); s++) {
        const NoiseStream st(d, s ? g : channel, s != 0);
        i32 F = colour_stream_sample(d, st, t);
        if constexpr (SLOW) F += slow_stream_sample(d, st, t);
        sum += (i32)(((i64)(s ? mix : 65536) * F) >> 16);       // (65536 F >> 16 is F)
    }
    return (sum + 32768) >> 16;
}
// Four-sample form: lane l of a wave takes samples tb + 4 l .. tb + 4 l + 3, tb wave-uniform.  The 256 + L - 1 whites of the wave lie in
// the aligned quads qb .. qb + 64 + dmax - 1, qb = (tb - L + 1) >> 2, dmax <= 5: lane l draws quad qb + l and alias-samples it, lanes
// 0 .. dmax - 1 draw quad qb + 64 + l in a second call, and the four cell values of a quad travel as two packed words.  The whites of
// lane l sit in the quads of lanes l .. l + dmax (lanes past 63: the second call's): one cross-lane fetch of two words per step, the
// same step for every lane, and sixteen multiply-adds against the seven taps the step's distances ask for (scalar loads; zeros outside
// 0 .. L - 1).  Two Philox calls and eight alias gathers per lane and stream whatever L and tb & 3.
// ALL 64 LANES MUST BE EXECUTING (ds_bpermute reads nothing from a switched-off lane): call it before any per-lane bound.
__device__ __forceinline__ void colour_stream_four(const WfsDev &d, const NoiseStream &st, i64 tb, int lane, i32 *F)
{
    const i64 s0 = tb - (d.nc_n_taps - 1);                      // the first white lane 0 needs
    const i64 qb = s0 >> 2;
    const i32 reach = __builtin_amdgcn_readfirstlane(d.nc_n_taps - 1 + (i32)(s0 & 3));      // distance of sample 0 of a lane from word 0 of its own quad
    const i32 dmax = (reach + 3) >> 2;
    auto quad = [&](i64 q, u32 &lo, u32 &hi) {
        const u32x4 a = noise_quad_of(d.k0, d.k1, st.id, st.site_white, q);
        lo = alias_pair(st.tab, a.x, a.y); hi = alias_pair(st.tab, a.z, a.w);
    };
    u32 p0, p1, r0 = 0, r1 = 0;
    quad(qb + lane, p0, p1);
    if (lane < dmax) quad(qb + 64 + lane, r0, r1);
    F[0] = F[1] = F[2] = F[3] = 0;
#pragma nounroll
    for (i32 dd = 0; dd <= dmax; dd++) {                        // (wave-uniform)
        // lanes below dd are read by nobody at this step but the lanes that wrap: they lend the second call's quads
        const i32 src = ((lane + dd) & 63) << 2;
        const u32 g0 = (u32)__builtin_amdgcn_ds_bpermute(src, (int)(lane < dd ? r0 : p0));
        const u32 g1 = (u32)__builtin_amdgcn_ds_bpermute(src, (int)(lane < dd ? r1 : p1));
        const i32 w[4] = {(i32)(int16_t)g0, (i32)g0 >> 16, (i32)(int16_t)g1, (i32)g1 >> 16};
        const i32 kb = reach - 4 * dd;                          // sample j against word c: tap kb + j - c
        i32 tp[7];
#pragma unroll
        for (int u = 0; u < 7; u++) tp[u] = st.taps[kb - 3 + u];
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int j = 0; j < 4; j++) F[j] += tp[3 + j - c] * w[c];
    }
}
template <bool SLOW = false>
__device__ __forceinline__ void noise_colour_four(const WfsDev &d, i32 channel, i64 tb, int lane, i32 *out)
{
    const i32 g = __builtin_amdgcn_readfirstlane(d.nc_group ? d.nc_group[channel] : -1);        // (one row per wave)
    const i32 mix = g >= 0 ? d.nc_mix[channel] : 0;
    i32 sum[4] = {0, 0, 0, 0};
#pragma nounroll
    for (int s = 0; s < (g >= 0 ? 2 : 1); s++) {
        const NoiseStream st(d, s ? g : channel, s != 0);
        i32 F[4];
        colour_stream_four(d, st, tb, lane, F);
        if constexpr (SLOW) {
            i32 S[4];
            slow_stream_four(d, st, tb, lane, S);
#pragma unroll
            for (int j = 0; j < 4; j++) F[j] += S[j];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) sum[j] += (i32)(((i64)(s ? mix : 65536) * F[j]) >> 16);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) out[j] = (sum[j] + 32768) >> 16;
}

// wfs_noise_model_samples: noise(channel, t0 .. t0 + n - 1) through the two forms the row kernels use -- a thread takes four
// consecutive samples as a lane of the fast paths does (t0 is wave-uniform, 4 k a multiple of four), the last n & 3 one by one
__global__ __launch_bounds__(256) void k_noise_model_samples(WfsDev d, i32 channel, i64 t0, i64 n, int16_t *out)
{
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (4 * k >= n) return;
    const uint2 *cells = d.nm_cells + (i64)channel * d.nm_cells_per_ch;
    if (4 * k + 3 < n) {
        i32 v[4];
        noise_model_four(d, cells, channel, t0, (i32)(4 * k), v);
#pragma unroll
        for (int j = 0; j < 4; j++) out[4 * k + j] = (int16_t)v[j];
    } else {
        for (i64 s = 4 * k; s < n; s++) out[s] = (int16_t)noise_model_sample(d, cells, channel, t0 + s);
    }
}

// The same for the coloured model: a wave takes 256 consecutive samples through the four-sample form -- every lane draws and exchanges,
// whatever n, and only the stores look at n -- and the last n & 3 samples go through the single-sample form.  (SLOW: with the slow levels)
template <bool SLOW>
__global__ __launch_bounds__(256) void k_noise_colour_samples(WfsDev d, i32 channel, i64 t0, i64 n, int16_t *out)
{
    const int lane = threadIdx.x & 63;
    const i64 b = ((i64)blockIdx.x * 4 + wave_in_block()) * 256;
    i32 v[4];
    noise_colour_four<SLOW>(d, channel, t0 + b, lane, v);
    const i64 s = b + 4 * lane;
    if (s + 3 < n) {
#pragma unroll
        for (int j = 0; j < 4; j++) out[s + j] = (int16_t)v[j];
    } else {
        for (i64 u = s; u < n; u++) out[u] = (int16_t)noise_colour_sample<SLOW>(d, channel, t0 + u);
    }
}
// wfs_noise_slow_samples: S(row, t0 .. t0 + n - 1) in Q16 of a stream through the same two forms
__global__ __launch_bounds__(256) void k_noise_slow_samples(WfsDev d, i32 row, i64 t0, i64 n, i32 *out)
{
    const int lane = threadIdx.x & 63;
    const i64 b = ((i64)blockIdx.x * 4 + wave_in_block()) * 256;
    const NoiseStream st = NoiseStream::of_row(d, row);
    i32 v[4];
    slow_stream_four(d, st, t0 + b, lane, v);
    const i64 s = b + 4 * lane;
    if (s + 3 < n) {
#pragma unroll
        for (int j = 0; j < 4; j++) out[s + j] = v[j];
    } else {
        for (i64 u = s; u < n; u++) out[u] = slow_stream_sample(d, st, t0 + u);
    }
}
// wfs_noise_white_samples: the white sequence w(row, t0 .. t0 + n - 1) of a stream
__global__ __launch_bounds__(256) void k_noise_white_samples(WfsDev d, i32 row, i64 t0, i64 n, int16_t *out)
{
    const i64 s = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const NoiseStream st = NoiseStream::of_row(d, row);
    const i64 t = t0 + s;
    const u32x4 a = noise_quad_of(d.k0, d.k1, st.id, st.site_white, t >> 2);
    const u32 m = (u32)t & 3u;
    out[s] = (int16_t)alias_sample(st.tab, m == 0 ? a.x : (m == 1 ? a.y : (m == 2 ? a.z : a.w)));      // (word_of, written out: the call costs this kernel four registers)
}


// NK, the noise of the batch, is a template parameter of the row kernels (NoiseKind of wfs_noise.h; 0: none, 1: int16 table, 2: float64
// table, 3: the noise model, drawn where the tables are loaded, 4: the coloured model, drawn at the same places, 5: the same with the
// slow levels added to every stream, which goes wherever kind 4 goes).  row_abs, the row's first absolute sample, is what kinds 3, 4
// and 5 count from.  The finished sample itself -- finish_value, and finish_resident of k_row_pulse -- is a rule of wfs_rows.h.
//
// Sample i of a row in one step, its noise fetched behind a branch: the general paths of k_zle and k_pack
// (DK: PMT dark counts are on, dch the channel dark_channel_of gave the row -- D is added to the accumulated value in front of everything else)
template <int NK, bool DK = false>
__device__ __forceinline__ i32 finish_sample_of(const WfsDev &d, i32 acc_i, i64 i, i32 slot_ch, bool he, i64 ix_rand, i64 row_abs, i32 dch = -1)
{
    if constexpr (DK) { if (dch >= 0) acc_i += dark_sample(d, dch, row_abs + i); }
    const bool noisy = NK != 0 && (NK >= 3 || d.enable_noise) && slot_ch < d.noise_channels;
    i32 nz = 0; double nzf = 0;
    if (noisy) {
        if constexpr (NK == 3) nz = noise_model_sample(d, d.nm_cells + (i64)slot_ch * d.nm_cells_per_ch, slot_ch, row_abs + i);
        else if constexpr (NK == 4 || NK == 5) nz = noise_colour_sample<NK == 5>(d, slot_ch, row_abs + i);
        else if constexpr (NK != 0) {
            const u32 in = ((u32)ix_rand + (u32)i) % (u32)d.noise_len;      // rawdata.py:433-434 (ix_rand < noise_len <= 2^31, i < 2^20: 32 bits hold the sum)
            // channel-major copy (wfs_set_tables): consecutive samples, consecutive addresses
            if constexpr (NK == 2) nzf = d.noise_f[(i64)slot_ch * d.noise_stride + in]; else nz = d.noise[(i64)slot_ch * d.noise_stride + in];
        }
    }
    return finish_value<NK>(d, acc_i, he, noisy, nz, nzf);
}
template <int NK, bool DK = false>
__device__ __forceinline__ i32 finish_sample(const WfsDev &d, const i32 *acc, i64 i, i32 slot_ch, bool he, i64 ix_rand, i64 row_abs, i32 dch = -1)
{
    return finish_sample_of<NK, DK>(d, acc[i], i, slot_ch, he, ix_rand, row_abs, dch);
}

// The same in two steps, for loops that want ALL their loads in flight before the first use: with the load inside finish_sample
// the compiler waits for every load right behind it (a branch follows), and a wave spends one memory round trip per load.
// A row no longer than the noise array wraps at most once (ix_rand < noise_len, i < len <= noise_len): no loop on the load path.
// noise_row points at the channel's row of the table, for the drawn kinds at its alias cells (noise_row_of), and a row outside the
// table (noisy false, wave-uniform) reads row 0 and drops the value, a row outside the model (nullptr) draws nothing: NO branch sits
// between two loads -- with a branch around the noise load the compiler drained the memory counter after every one of them.
template <int NK>
__device__ __forceinline__ const void *noise_row_of(const WfsDev &d, i32 channel, bool noisy)
{
    const i64 noise_off = noisy ? (i64)channel * d.noise_stride : 0;
    return NK >= 3 ? (const void *)(noisy ? d.nm_cells + (i64)channel * d.nm_cells_per_ch : nullptr)
                   : (NK == 2 ? (const void *)(d.noise_f + noise_off) : (const void *)(d.noise + noise_off));
}
template <int NK> struct RawSample { i32 acc; i32 nz; };
template <> struct RawSample<0> { i32 acc; };
template <> struct RawSample<2> { i32 acc; double nzf; };
template <int NK, bool DK = false>
__device__ __forceinline__ RawSample<NK> load_sample(const WfsDev &d, const i32 *acc, i32 i, const void *noise_row, u32 nstart, u32 noff, i32 channel = 0, i64 row_abs = 0, i32 dch = -1)
{
    // (32-bit offsets from wave-uniform row pointers: the address arithmetic is one add per load, the bases stay in SGPRs)
    // noise sample nstart + noff of the row, nstart < noise_len a scalar, noff < noise_len (noise_wrap)
    RawSample<NK> s; s.acc = acc[(u32)i];
    if constexpr (DK) { if (dch >= 0) s.acc += dark_sample(d, dch, row_abs + i); }      // (dch is wave-uniform)
    if constexpr (NK == 3) s.nz = noise_row ? noise_model_sample(d, (const uint2 *)noise_row, channel, row_abs + i) : 0;      // (wave-uniform)
    else if constexpr (NK == 4 || NK == 5) s.nz = noise_row ? noise_colour_sample<NK == 5>(d, channel, row_abs + i) : 0;
    else if constexpr (NK != 0) {
        const u32 in = noise_wrap(nstart + noff, (u32)d.noise_len);
        if constexpr (NK == 2) s.nzf = ((const double *)noise_row)[in]; else s.nz = ((const int16_t *)noise_row)[in];
    }
    return s;
}
template <int NK>
__device__ __forceinline__ i32 finish_loaded(const WfsDev &d, const RawSample<NK> &s, bool he, bool noisy)
{
    i32 nz = 0; double nzf = 0;
    if constexpr (NK == 2) nzf = s.nzf; else if constexpr (NK != 0) nz = s.nz;
    return finish_value<NK>(d, s.acc, he, noisy, nz, nzf);
}

// Four consecutive samples of a row per lane (k_zle): 16 bytes of the row at a 4-byte aligned address, 8 (32) bytes of the noise at a
// 2 (8)-byte aligned one -- the hardware takes both as single loads; NOISE_PAD keeps the noise read off the wrap.
template <int NK> struct Raw4 { i32 acc[4]; i32 nz[4]; };
template <> struct Raw4<0> { i32 acc[4]; };
template <> struct Raw4<1> { i32 acc[4]; int16_t nz[4]; };
template <> struct Raw4<2> { i32 acc[4]; double nzf[4]; };
// The noise of lane `lane` of a wave that takes the 256 samples of a row from nstart on, four per lane.  Tables: nstart < noise_len is
// the (scalar) table index of the block's first sample, wrapped once.  Drawn kinds: nstart is the UNCLAMPED wave-uniform index of the
// block's first sample in the row, so that (row_abs + nstart) & 3 is wave-uniform and, for kinds 4 and 5, every lane draws the quad its
// neighbours need whether or not its own samples lie in the row: ALL 64 LANES MUST BE EXECUTING (colour_stream_four).
template <int NK>
__device__ __forceinline__ void noise_four(const WfsDev &d, Raw4<NK> &o, const void *noise_row, i32 channel, i64 row_abs, u32 nstart, int lane)
{
    if constexpr (NK >= 3) {
        if (!noise_row) o.nz[0] = o.nz[1] = o.nz[2] = o.nz[3] = 0;      // (wave-uniform)
        else if constexpr (NK == 3) noise_model_four(d, (const uint2 *)noise_row, channel, row_abs + (i64)nstart, 4 * lane, o.nz);
        else noise_colour_four<NK == 5>(d, channel, row_abs + (i64)nstart, lane, o.nz);
    } else if constexpr (NK != 0) {
        const u32 in = noise_wrap(nstart + 4u * (u32)lane, (u32)d.noise_len);
        if constexpr (NK == 2) __builtin_memcpy(o.nzf, (const double *)noise_row + in, 32); else __builtin_memcpy(o.nz, (const int16_t *)noise_row + in, 8);
    }
}
// (i may be clamped into the row -- k_zle, lanes past its end: the noise goes by nstart and the lane)
template <int NK>
__device__ __forceinline__ Raw4<NK> load_four(const WfsDev &d, const i32 *acc, i32 i, const void *noise_row, u32 nstart, int lane, i32 channel = 0, i64 row_abs = 0)
{
    Raw4<NK> s; __builtin_memcpy(s.acc, acc + (u32)i, 16);
    noise_four<NK>(d, s, noise_row, channel, row_abs, nstart, lane);
    return s;
}
template <int NK>
__device__ __forceinline__ i32 finish_four(const WfsDev &d, const Raw4<NK> &s, int j, bool he, bool noisy)
{
    i32 nz = 0; double nzf = 0;
    if constexpr (NK == 2) nzf = s.nzf[j]; else if constexpr (NK != 0) nz = s.nz[j];
    return finish_value<NK>(d, s.acc[j], he, noisy, nz, nzf);
}

// The interval bookkeeping of a row whose hold-off is at least a chunk of 64 samples: two hits of one chunk are never more than the
// hold-off apart, so only the FIRST hit of a chunk can open an interval -- scalar work on the ballot of the lanes' hit nibbles.
// Closed intervals wait in lane (k mod 64) and leave in one store (flush / finish).  A store inside a loop of loads -- even one that
// is almost never executed -- may be outstanding together with loads, the two kinds retire out of order, and the compiler then waits
// for EVERYTHING at the top of the loop; the flush of a row with more than 64 intervals drains the counter itself.
struct ZleFast {
    i32 s_last = -1, s_left = -1, s_count = 0, s_nrec = 0, my_l = 0, my_r = 0;
    // close interval k = [rawl, rawr] (first / last hit, zle_window); returns the records it needs
    __device__ __forceinline__ i32 close(const WfsDev &d, const ZleArgs &a, int lane, i64 base, i64 row_abs, i32 len32, i32 k, i32 rawl, i32 rawr)
    {
        const ZleWindow w = zle_window(rawl, rawr, d.tw, len32);
        const int slot = k & 63;
        if (lane == slot) { my_l = w.left; my_r = w.right; }
        if (slot == 63) {
            a.itv_left[base + (k - 63) + lane] = row_abs + my_l; a.itv_right[base + (k - 63) + lane] = row_abs + my_r;      // absolute sample indices (rawdata.py:311)
            __builtin_amdgcn_s_waitcnt(0x0F70);             // vmcnt(0)
        }
        return w.nrec;
    }
    // 256 samples: lane q holds the hits of samples i .. i + 3 (i = block start + 4 q) as a nibble; 16 lanes are a chunk of 64 samples,
    // whose first and last hit come from the ballot of the non-empty nibbles and two readlanes
    __device__ __forceinline__ void block(const WfsDev &d, const ZleArgs &a, int lane, i64 base, i64 row_abs, i32 len32, i32 hold32, u32 nib, i32 i)
    {
        const u64 mask = ballot64(nib != 0);
        if (mask == 0) return;                              // wave-uniform
        const i32 fpos = i + (i32)__builtin_ctz(nib | 16u), lpos = i + 31 - (i32)__builtin_clz(nib | 1u);      // first / last hit of the lane
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const u32 m = (u32)(mask >> (16 * c)) & 0xffffu;
            if (m == 0) continue;
            const i32 first = __builtin_amdgcn_readlane(fpos, 16 * c + (i32)__builtin_ctz(m));
            const i32 last = __builtin_amdgcn_readlane(lpos, 16 * c + 31 - (i32)__builtin_clz(m));
            if (s_last < 0 || first - s_last > hold32) {
                if (s_count > 0) s_nrec += close(d, a, lane, base, row_abs, len32, s_count - 1, s_left, s_last);
                s_left = first; s_count++;
            }
            s_last = last;
        }
    }
    __device__ __forceinline__ void finish(const WfsDev &d, const ZleArgs &a, int lane, i64 base, i64 row_abs, i32 len32, i64 idx)
    {
        if (s_count > 0) s_nrec += close(d, a, lane, base, row_abs, len32, s_count - 1, s_left, s_last);
        if (lane < (s_count & 63)) { const i64 k0 = base + (s_count & ~63); a.itv_left[k0 + lane] = row_abs + my_l; a.itv_right[k0 + lane] = row_abs + my_r; }
        if (lane == 0) { a.itv_n[idx] = s_count; a.row_nrec[idx] = s_nrec; }
    }
};

// The interval bookkeeping for ANY hold-off (the general path of k_zle; k_row_empty): a lane per sample of a chunk of 64, `mask` the
// ballot of the chunk's hits and `hit` the lane's own bit of it.  An interval is closed (zle_window) by the lane that finds the next
// one's start, the last one by lane 0 at the end of the row.
struct ZleChunks {
    i32 carry_last = -1, open_left = -1, count = 0, nrec = 0;      // (a row is shorter than 10^6 samples: 32-bit indices)
    // close interval k = [rawl, rawr] (first / last hit) in the lane that found it: absolute sample indices (rawdata.py:311); returns the records it needs
    __device__ __forceinline__ i32 close(const WfsDev &d, const ZleArgs &a, i64 base, i64 row_abs, i32 len32, i32 k, i32 rawl, i32 rawr)
    {
        const ZleWindow w = zle_window(rawl, rawr, d.tw, len32);
        a.itv_left[base + k] = row_abs + w.left; a.itv_right[base + k] = row_abs + w.right;
        return w.nrec;
    }
    __device__ __forceinline__ void chunk(const WfsDev &d, const ZleArgs &a, int lane, i64 base, i64 row_abs, i32 len32, i32 hold32, bool hit, u64 mask, i32 c0)
    {
        const i32 i = c0 + lane;
        const u64 lt = (1ull << lane) - 1ull;
        const u64 below = mask & lt;
        const i32 prev = below ? c0 + 63 - __clzll(below) : carry_last;       // last hit before this sample
        const bool start = hit && (prev < 0 || i - prev > hold32);
        const u64 smask = ballot64(start);
        if (start) {
            const u64 sbelow = smask & lt;
            const i32 k = count + __popcll(sbelow);
            const i32 prev_left = sbelow ? c0 + 63 - __clzll(sbelow) : open_left;
            if (k > 0) nrec += close(d, a, base, row_abs, len32, k - 1, prev_left, prev);
        }
        count += __popcll(smask);
        if (smask) open_left = c0 + 63 - __clzll(smask);
        if (mask) carry_last = c0 + 63 - __clzll(mask);
    }
    __device__ __forceinline__ void finish(const WfsDev &d, const ZleArgs &a, int lane, i64 base, i64 row_abs, i32 len32, i64 idx)
    {
        if (lane == 0 && count > 0) nrec += close(d, a, base, row_abs, len32, count - 1, open_left, carry_last);
        for (int o = 32; o > 0; o >>= 1) nrec += __shfl_down(nrec, o, 64);
        if (lane == 0) { a.itv_n[idx] = count; a.row_nrec[idx] = nrec; }
    }
};

// one wave per row: find_intervals_below_threshold (utils.py:13-58) in its parallel form: consecutive
// hit samples a < b belong to one interval iff b - a <= max(holdoff, 1); then the window of rawdata.py:302-308.
template <int NK, bool DK>
__global__ __launch_bounds__(256) void k_zle(WfsDev d, ZleArgs a)
{
    const int lane = threadIdx.x & 63;
    const i64 r = (i64)blockIdx.x * 4 + wave_in_block();         // (an SGPR: the descriptor and everything derived from it stay scalar)
    if (r >= a.n_front) return;                             // (the rows behind n_front are resident: k_row_pulse has made their intervals)
    const RowDesc q = a.desc[r];
    const i64 idx = q.idx; const i32 channel = q.channel; const bool he = q.he != 0;
    const i32 *acc = (q.src ? a.tbuf : a.raw) + q.acc_off;
    const i64 thr = q.thr;
    const i64 ixr = q.ixr;
    const i64 base = q.itv_base;
    const i64 row_abs = q.row_abs;
    const i32 len32 = q.len, hold32 = (i32)zle_holdoff(d.tw);
    const i32 dch = DK ? dark_channel_of(d, channel, he) : -1;
    ZleChunks zc;                                           // (the general path)
    const bool noisy = NK != 0 && channel < d.noise_channels;
    // the noise index of a row's sample i is (ix + i) mod noise_len (rawdata.py:433-434): a scalar start per block of samples that
    // steps with the block and wraps, plus the lane's offset inside the block -- rows may be any number of noise lengths long.
    // (A table shorter than NOISE_MIN_FAST samples would wrap more than once inside a block: the general path below.)
    // (The noise model, kinds 3, 4 and 5, has no table and no wrap: the fast paths wherever kind 0 takes them.)
    constexpr bool TABLE = NK == 1 || NK == 2;
    const bool fast_loads = len32 >= 1 && (!TABLE || d.noise_len >= NOISE_MIN_FAST);
    const u32 nixr = noisy ? (u32)ixr : 0u;
    const void *noise_row = noise_row_of<NK>(d, channel, noisy);
    if (hold32 >= ZLE_FAST_HOLD && fast_loads && !a.row_dbg) {
        // The usual geometry (hold-off of at least a chunk): the interval bookkeeping is scalar work on the ballot mask (ZleFast), and
        // the vector unit is left with load, finish and compare.
        constexpr int G = NK >= 4 ? 1 : 4;          // (kind 4 draws instead of loading: one block's draws at a time, one copy of their code)
        ZleFast z;
        // A lane takes FOUR consecutive samples (one 16-byte load of the row, one 8-byte load of the noise): a wave instruction moves
        // 1 KB of the row, and the hits of a lane are a nibble.
        // G such loads per trip: 1024 samples, most rows in one trip (6 KB in flight per wave; a second register set filled ahead
        // bought nothing -- the register allocator reuses the first set's registers for addresses and waits for its loads anyway).
        // Loads are unconditional (lanes past the end of the row read its first samples): behind a branch the compiler drains the
        // memory counter instead of counting.
        Raw4<NK> A[G];
        u32 nrun = nixr;                                        // noise index of the next block's first sample (a scalar)
        auto fetch = [&](Raw4<NK> *buf, i32 g0) {
#pragma unroll
            for (int u = 0; u < G; u++) {
                const i32 i = g0 + 256 * u + 4 * lane;
                if constexpr (NK == 3) {
                    // load_four, written out (with the call k_zle<3> takes 76 registers for 71 and loses a wave of occupancy): the draw
                    // counts from the row's start with the lane's clamped index, which has the same t0 & 3 as noise_four's
                    const i32 ic = i < len32 ? i : 0;
                    __builtin_memcpy(buf[u].acc, acc + (u32)ic, 16);
                    if (noise_row) noise_model_four(d, (const uint2 *)noise_row, channel, row_abs, ic, buf[u].nz);      // (wave-uniform)
                    else buf[u].nz[0] = buf[u].nz[1] = buf[u].nz[2] = buf[u].nz[3] = 0;
                } else
                buf[u] = load_four<NK>(d, acc, i < len32 ? i : 0, noise_row, NK >= 4 ? (u32)(g0 + 256 * u) : nrun, lane, channel, row_abs);
                if constexpr (TABLE) nrun = noise_advance(nrun, 256u, (u32)d.noise_len);
                // (the dark counts of the block's own samples, whatever the clamped load read: a lane past the row drops both)
                if constexpr (DK) { if (dch >= 0 && g0 + 256 * u < len32) dark_block(d, dch, row_abs + g0 + 256 * u, lane, buf[u].acc); }
            }
        };
        auto look = [&](const Raw4<NK> *buf, i32 g0) {
#pragma unroll
            for (int u = 0; u < G; u++) {
                const i32 b0 = g0 + 256 * u;
                if (b0 >= len32) break;                         // wave-uniform
                const i32 i = b0 + 4 * lane;
                u32 nib = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) { const i32 v = finish_four<NK>(d, buf[u], j, he, noisy); nib |= (i + j < len32 && (i64)v < thr) ? (1u << j) : 0u; }
                z.block(d, a, lane, base, row_abs, len32, hold32, nib, i);
            }
        };
        for (i32 g0 = 0; g0 < len32; g0 += 256 * G) { fetch(A, g0); look(A, g0); }
        z.finish(d, a, lane, base, row_abs, len32, idx);
        return;
    }
    // chunks of 64 samples; the loads of ZLE_GROUP chunks are issued together (one dependent load per chunk leaves the wave
    // waiting a memory round trip per 64 samples)
    constexpr int ZLE_GROUP = NK >= 4 ? 1 : 2;      // (kind 4: nothing to overlap, one copy of the draws)
    u32 nrun1 = nixr;
    for (i32 g0 = 0; g0 < len32; g0 += 64 * ZLE_GROUP) {
        i32 vv[ZLE_GROUP];
        if (NK >= 4 || fast_loads) {                            // (wave-uniform) every load of the group first, then the arithmetic; kind 4 has no other path: a row it cannot take fast is empty
            RawSample<NK> rs[ZLE_GROUP];
#pragma unroll
            for (int u = 0; u < ZLE_GROUP; u++) {
                const i32 i = g0 + 64 * u + lane;
                rs[u] = load_sample<NK, DK>(d, acc, i < len32 ? i : len32 - 1, noise_row, nrun1, (u32)lane, channel, row_abs, dch);
                if constexpr (TABLE) nrun1 = noise_advance(nrun1, 64u, (u32)d.noise_len);
            }
#pragma unroll
            for (int u = 0; u < ZLE_GROUP; u++) { const i32 i = g0 + 64 * u + lane; vv[u] = i < len32 ? finish_loaded(d, rs[u], he, noisy) : 0x7fffffff; }
        } else {
#pragma unroll
            for (int u = 0; u < ZLE_GROUP; u++) { const i32 i = g0 + 64 * u + lane; vv[u] = i < len32 ? finish_sample<NK, DK>(d, acc, i, channel, he, ixr, row_abs, dch) : 0x7fffffff; }
        }
        if (a.row_dbg) {
#pragma unroll
            for (int u = 0; u < ZLE_GROUP; u++) { const i32 i = g0 + 64 * u + lane; if (i < len32) a.row_dbg[a.row_dbg_off[r] + i] = vv[u]; }
        }
#pragma unroll
        for (int u = 0; u < ZLE_GROUP; u++) {
            const i32 c0 = g0 + 64 * u;
            if (c0 >= len32) break;                             // wave-uniform
            const i32 i = c0 + lane;
            const bool hit = i < len32 && (i64)vv[u] < thr;
            zc.chunk(d, a, lane, base, row_abs, len32, hold32, hit, ballot64(hit), c0);
        }
    }
    zc.finish(d, a, lane, base, row_abs, len32, idx);
}

// The bottom-array sum row of a window (wfs_set_sum_signal): row 800 of the reference's digitiser array, the per-pulse rounded ADC
// wave of every bottom PMT added up (rawdata.py:250-254, sum_signal at :392-396).  The reference never masks that row in, so it is
// never finished or emitted there; here it becomes one more accumulator row of the window.  A pass over rows that exist already: the
// i32 accumulators and the sample buffers of single-tile rows (k_tile_rows keeps bottom rows off the resident path).  One workgroup
// per (window, SUM_CHUNK samples of its sum row): the window's bottom rows that reach into the chunk are listed in LDS once -- offset
// into raw or tbuf, first sample relative to the chunk, length --, then every lane walks the list for its four samples, 256 apart, so
// that a wave's load is 256 consecutive bytes.  Row bases and ranges are wave-uniform and travel in SGPRs (readfirstlane of the LDS
// broadcast); loads are unconditional (a lane outside the row reads the row's sample 0 and drops it), two rows -- eight loads -- in flight.
// The sum is carried in 64 bits and stored saturated to 32: the factor int(he_factor) is applied where the row is finished.
struct SumArgs {
    const i64 *chunk_off; i64 n_gslots;          // exclusive scan of the windows' chunk counts: workgroup -> (window, chunk)
    const i64 *sum_lo, *sum_off; const i32 *sum_len;
    const i64 *row_lo, *row_hi, *acc_off; const i32 *raw, *tbuf;
    const i32 *tile_done, *row_cnt, *row_tile, *ins_bcap; const i64 *ins_boff; i64 n_done;      // rows read from a tile buffer in place
    i32 *out;                                    // raw + sum_base
};
__global__ __launch_bounds__(256) void k_sum_signal(WfsDev d, SumArgs a)
{
    __shared__ i64 s_off[WFS_MAX_CH + 1]; __shared__ i32 s_rel[WFS_MAX_CH + 1], s_len[WFS_MAX_CH + 1]; __shared__ i32 s_n;      // (+1: the list is walked in pairs)
    const i64 b = blockIdx.x;
    // window of the workgroup: the last one whose first chunk is not behind b (scalar loads; windows without a sum row have no chunks)
    i64 g = 0;
    { i64 hi = a.n_gslots; while (hi - g > 1) { const i64 mid = (g + hi) >> 1; if (a.chunk_off[mid] <= b) g = mid; else hi = mid; } }
    const i32 len = a.sum_len[g];
    const i32 s0 = (i32)(b - a.chunk_off[g]) * SUM_CHUNK;
    if (s0 >= len) return;                                  // (cannot happen: the grid is the scan's total)
    const i64 slo = a.sum_lo[g];
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const i32 n_bottom = d.last_bottom - d.n_top + 1;       // (<= n_tpc <= WFS_MAX_CH, wfs_create)
    for (i32 t = threadIdx.x; t < n_bottom; t += blockDim.x) {
        const i64 ridx = g * d.n_tpc + d.n_top + t;
        const i64 lo = a.row_lo[ridx];
        if (lo == I64_MAX) continue;
        const i32 rel = (i32)(lo - slo) - s0, rl = (i32)row_span(lo, a.row_hi[ridx], d.tw).len;      // both rows start tw samples ahead of their first pulse
        if (rel >= SUM_CHUNK || rel + rl <= 0) continue;
        i64 off;                                                // sample offset into raw, or ~(offset into tbuf)
        if (!d.full_readout && row_is_direct(a.tile_done, a.n_done, a.row_cnt, a.row_tile, ridx)) {
            const i32 tile = a.row_tile[ridx]; const i32 ins = tile / d.n_tpc;
            off = ~(a.ins_boff[ins] + (i64)(tile - ins * d.n_tpc) * a.ins_bcap[ins]);
        } else off = a.acc_off[ridx];
        const i32 k = atomicAdd(&s_n, 1);
        s_off[k] = off; s_rel[k] = rel; s_len[k] = rl;
    }
    __syncthreads();
    const i32 n = s_n;
    if (threadIdx.x == 0) { s_off[n] = s_off[0]; s_rel[n] = 0; s_len[n] = 0; }      // an empty row closes an odd list (a chunk between two pulses far apart has no row at all: the loop below is not entered, zeros are stored)
    __syncthreads();
    i64 acc[4] = {0, 0, 0, 0};
    for (i32 k = 0; k < n; k += 2) {                            // two rows, eight loads in flight
        const i32 *p[2]; i32 rel[2], rl[2]; i32 v[2][4];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const i64 ob = s_off[k + q];
            const i64 off = (i64)(((u64)(u32)__builtin_amdgcn_readfirstlane((i32)(u32)((u64)ob >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((i32)(u32)(u64)ob));
            p[q] = off < 0 ? a.tbuf + ~off : a.raw + off;       // (kernel arguments: the loads keep their global address space and a scalar base)
            rel[q] = __builtin_amdgcn_readfirstlane(s_rel[k + q]); rl[q] = __builtin_amdgcn_readfirstlane(s_len[k + q]);
        }
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
            for (int u = 0; u < 4; u++) { const i32 j = (i32)threadIdx.x + 256 * u - rel[q]; v[q][u] = p[q][(u32)j < (u32)rl[q] ? j : 0]; }
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
            for (int u = 0; u < 4; u++) { const i32 j = (i32)threadIdx.x + 256 * u - rel[q]; acc[u] += (u32)j < (u32)rl[q] ? (i64)v[q][u] : 0; }
    }
    i32 *out = a.out + a.sum_off[g];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const i32 s = s0 + (i32)threadIdx.x + 256 * u;
        const i64 c = acc[u] > 0x7fffffffLL ? 0x7fffffffLL : (acc[u] < -0x80000000LL ? -0x80000000LL : acc[u]);
        if (s < len) out[s] = (i32)c;
    }
}

// Resident rows: ONE wave makes a whole (window, channel) row -- zeroes it in LDS, adds the rounded pulses of the row's tiles
// (wave_tile_pulse: the arithmetic of k_pulse_wave; integer sums, so the order of the tiles does not matter), finishes the samples
// (noise, baseline, clamp: rawdata.py:398-458), runs the zero-length encoding on them and writes them ONCE, as 16-bit samples.
// Against the accumulator path (memset 4 B + atomics + 6 B read by k_zle + 6 B read by k_pack per sample) a row costs 2 B of noise
// read and 2 B written here and 2 B read by k_pack.  rawdata.py:231-239 (per-pulse rounding into the row), :302-311 (intervals).
template <int NK, bool FMA, bool SEG, bool DK>
__global__ __launch_bounds__(256) void k_row_pulse(WfsDev d, PulseArgs a, ZleArgs z, i64 first, i64 n_res, i32 region)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char row_lds[];
    constexpr RowLds o = row_pulse_lds(0);                      // (the offsets do not depend on the region, which comes last)
    double *sTz = (double *)(row_lds + o.sTz); double *s_cmax = (double *)(row_lds + o.cmax);
    WavePhoton *s_ph = (WavePhoton *)(row_lds + o.ph);
    i32 *s_acc = (i32 *)(row_lds + o.acc);
    wave_tables_fill(d, sTz, s_cmax);
    __syncthreads();
    const int lane = threadIdx.x & 63, w = wave_in_block();
    const i64 r = (i64)blockIdx.x * 4 + w;
    if (r >= n_res) return;                               // wave-uniform; no barrier below
    const RowDesc q = z.desc[z.n_front + first + r];
    const ResRow rr = z.res_rows[first + r];
    i32 *acc = s_acc + (size_t)w * region;
    WavePhoton *wph = s_ph + w * (64 + PW_U);
    const i32 len32 = q.len;
    const i64 thr = q.thr; const i64 base = q.itv_base, row_abs = q.row_abs, idx = q.idx;
    const i32 thr32 = zle_thr32(thr);
    const i32 hold32 = (i32)zle_holdoff(d.tw);
    const bool noisy = NK != 0 && q.channel < d.noise_channels;
    const i32 dch = DK ? dark_channel_of(d, q.channel, false) : -1;
    const void *noise_row = noise_row_of<NK>(d, q.channel, noisy);
    u32 nrun = (noisy && NK < 3) ? (u32)q.ixr : 0u;       // noise index of the next block's first sample (rawdata.py:433-434); kinds 3, 4: that sample's index in the row
    int16_t *fin = z.fin + q.acc_off;
    const i32 fin_len = fin_padded_len(len32);
    auto load_noise = [&](Raw4<NK> &o) {                  // (every lane of the wave is here: the callers' conditions are wave-uniform)
        noise_four<NK>(d, o, noise_row, q.channel, row_abs, nrun, lane);
        if constexpr (NK == 1 || NK == 2) nrun = noise_advance(nrun, 256u, (u32)d.noise_len);
        else if constexpr (NK != 0) nrun += 256u;
    };
    Raw4<NK> s4;
    load_noise(s4);                                       // the first block's noise: on its way under the pulses
    const i64 t1 = rr.t0 + rr.n;
    ZleFast zf;
    // A row longer than the wave's LDS (SEG) is made segment by segment: the tiles that reach into the segment are made again for it,
    // their samples outside it dropped; the interval bookkeeping and the noise index run on across the segments.
    for (i32 seg0 = 0; seg0 < len32; seg0 += region) {
        const i32 seg_len = SEG ? (len32 - seg0 < region ? len32 - seg0 : region) : len32;
        for (i32 i = 4 * lane; i < ((seg_len + 255) & ~255); i += 256) *(int4 *)(acc + i) = make_int4(0, 0, 0, 0);
        // ---- the row's tiles (no HE rows on this path: row slot == row index)
        TileDesc td = a.desc[rr.t0];
        for (i64 t = rr.t0; t < t1; t++) {
            if (t > rr.t0) td = a.desc[t];
            if (td.n < 0) {                               // a prepared tiny tile (k_tile_assign): the samples its photons reach, nothing else
                TinyDesc y; __builtin_memcpy(&y, &td, 64);
                if (SEG && (y.dst + y.s_last < seg0 || y.dst + y.s_first >= seg0 + seg_len)) continue;
                TinyPrep p; p.n = -y.n_neg; p.s_first = y.s_first; p.s_last = y.s_last;
#pragma unroll
                for (int j = 0; j < TINY_MAX_PHOTONS; j++) { p.g[j] = y.g[j]; p.jb[j] = (int)(y.jr[j] >> 4); p.rr[j] = (int)(y.jr[j] & 15u); }
                const i32 o = y.dst - seg0;
                tiny_tile_samples<FMA, 64, false>(d, a, p, t, lane, [&](int r_, int k_) { return sTz[r_ * (22 + 2) + 1 + k_]; },
                                                  [&](int s_, i32 adc) { if (!SEG || (u32)(o + s_) < (u32)seg_len) atomicAdd(&acc[o + s_], adc); });
            } else {
                if (SEG && (td.dst + td.L <= seg0 || td.dst >= seg0 + seg_len)) continue;
                const i32 o = (i32)td.dst - seg0;
                wave_tile_pulse<FMA, false>(d, a, td, t, wph, sTz, s_cmax, lane,
                                            [&](int s_, i32 adc) { if (!SEG || (u32)(o + s_) < (u32)seg_len) atomicAdd(&acc[o + s_], adc); });      // (ds_add_u32: every lane its own sample)
            }
        }
        // ---- finish, zero-length encoding, 16-bit samples
        for (i32 b0 = 0; b0 < seg_len; b0 += 256) {
            const i32 i = seg0 + b0 + 4 * lane;           // the lane's first sample in the row
            Raw4<NK> nxt = s4;
            if (i - 4 * lane + 256 < len32) load_noise(nxt);      // the next block's noise on its way under this block's arithmetic
            *(int4 *)s4.acc = *(const int4 *)(acc + b0 + 4 * lane);
            if constexpr (DK) { if (dch >= 0) dark_block(d, dch, row_abs + seg0 + b0, lane, s4.acc); }      // (every lane of the wave is here)
            u32 nib = 0; u32 v16[4];
            if constexpr (NK == 2) {
#pragma unroll
                for (int j = 0; j < 4; j++) { const i32 v = finish_four<NK>(d, s4, j, false, noisy); nib |= (i + j < len32 && (i64)v < thr) ? (1u << j) : 0u; v16[j] = (u32)(uint16_t)v; }
            } else {
                // integer noise: NOT finish_value but the deliberately cheaper finish_resident (wfs_rows.h has its domain)
                const i32 live = len32 - i;                  // samples of the lane inside the row
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    i32 nz = 0;
                    if constexpr (NK != 0) nz = s4.nz[j];
                    const i32 v = finish_resident<NK>(d, s4.acc[j], noisy, nz);
                    nib |= (j < live && v < thr32) ? (1u << j) : 0u; v16[j] = (u32)v;
                }
            }
            if (i < fin_len) *(uint2 *)(fin + i) = make_uint2(__builtin_amdgcn_perm(v16[1], v16[0], 0x05040100u), __builtin_amdgcn_perm(v16[3], v16[2], 0x05040100u));
            zf.block(d, z, lane, base, row_abs, len32, hold32, nib, i);
            s4 = nxt;
        }
        if (!SEG) break;
    }
    zf.finish(d, z, lane, base, row_abs, len32, idx);
}

// Full readout: the rows WITHOUT a pulse (wfs_set_full_readout; most rows of a fully read-out window).  Their sample is the finished
// value of an accumulator of 0 -- finish_four / finish_sample_of, the rule of every row -- so a row is noise, baseline and clamp:
// nothing is accumulated, no int32 sample exists anywhere, and the row is on no tile list.  One wave per row walks it in blocks of 256
// samples, four consecutive samples per lane: the noise of the block through noise_four (one Philox call of the white kind per lane,
// the quads of the coloured and slow kinds shared across the lanes, 8 / 32 bytes of a table), finished in registers, stored ONCE as
// 16-bit samples where k_pack_res reads them (RowDesc::src 2, like a resident row), and zero-suppressed from the lanes' hit nibbles.
// A block is addressed by its absolute first sample alone, so a row of any length is a run of blocks: there is no row buffer in LDS
// whose size would cut a long row into segments, and the taps and knots a block needs beyond its edges are drawn by the generators
// themselves (colour_stream_four / slow_stream_four).  Any hold-off (the resident path needs ZLE_FAST_HOLD): the bookkeeping is the
// general one of k_zle, a lane per sample of a 64-sample chunk, fed with the chunk's hit mask, which is put together from the ballots
// of the nibbles' four bits (sample 4 l + j of a chunk is bit j of lane l of its 16 lanes); a block without a hit -- almost all of
// them at an ordinary threshold -- costs four ballots.
__device__ __forceinline__ u64 spread16_by4(u64 x)      // bit k of the low 16 -> bit 4 k
{
    x &= 0xffffull;
    x = (x | (x << 24)) & 0x000000ff000000ffull; x = (x | (x << 12)) & 0x000f000f000f000full;
    x = (x | (x << 6)) & 0x0303030303030303ull; x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}
template <int NK, bool DK>
__global__ __launch_bounds__(256) void k_row_empty(WfsDev d, ZleArgs a, i64 first, i64 n_rows)
{
    const int lane = threadIdx.x & 63;
    const i64 r = (i64)blockIdx.x * 4 + wave_in_block();
    if (r >= n_rows) return;                                // wave-uniform
    const RowDesc q = a.desc[first + r];
    const i32 channel = q.channel; const bool he = q.he != 0;
    const i64 thr = q.thr, base = q.itv_base, row_abs = q.row_abs, ixr = q.ixr;
    const i32 len32 = q.len, hold32 = (i32)zle_holdoff(d.tw), fin_len = fin_padded_len(len32);
    int16_t *fin = a.fin + q.acc_off;
    const bool noisy = NK != 0 && channel < d.noise_channels;
    constexpr bool TABLE = NK == 1 || NK == 2;
    const bool fast_noise = !TABLE || d.noise_len >= NOISE_MIN_FAST;      // (a shorter table wraps more than once inside a block: sample by sample, as k_zle)
    const i32 dch = DK ? dark_channel_of(d, channel, he) : -1;
    const void *noise_row = noise_row_of<NK>(d, channel, noisy);
    u32 nrun = (noisy && TABLE) ? (u32)ixr : 0u;            // tables: noise index of the block's first sample (rawdata.py:433-434); drawn kinds: its index in the row
    ZleChunks zc;
    for (i32 b0 = 0; b0 < len32; b0 += 256) {
        const i32 i = b0 + 4 * lane;                        // the lane's first sample in the row
        i32 v[4];
        if (fast_noise) {                                   // (wave-uniform: all 64 lanes draw, noise_four)
            Raw4<NK> s4;
            s4.acc[0] = s4.acc[1] = s4.acc[2] = s4.acc[3] = 0;
            noise_four<NK>(d, s4, noise_row, channel, row_abs, nrun, lane);
            if constexpr (DK) { if (dch >= 0) dark_block(d, dch, row_abs + b0, lane, s4.acc); }
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = finish_four<NK>(d, s4, j, he, noisy);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = i + j < len32 ? finish_sample_of<NK, DK>(d, 0, (i64)(i + j), channel, he, ixr, row_abs, dch) : 0;
        }
        if constexpr (TABLE) nrun = fast_noise ? noise_advance(nrun, 256u, (u32)d.noise_len) : 0u; else nrun += 256u;
        u32 nib = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) nib |= (i + j < len32 && (i64)v[j] < thr) ? (1u << j) : 0u;
        if (i < fin_len) *(uint2 *)(fin + i) = make_uint2(((u32)v[0] & 0xffffu) | ((u32)v[1] << 16), ((u32)v[2] & 0xffffu) | ((u32)v[3] << 16));
        const u64 bj0 = ballot64((nib & 1u) != 0), bj1 = ballot64((nib & 2u) != 0), bj2 = ballot64((nib & 4u) != 0), bj3 = ballot64((nib & 8u) != 0);
        if ((bj0 | bj1 | bj2 | bj3) == 0) continue;         // wave-uniform
        for (int c = 0; c < 4; c++) {
            const u64 mask = spread16_by4(bj0 >> (16 * c)) | (spread16_by4(bj1 >> (16 * c)) << 1) | (spread16_by4(bj2 >> (16 * c)) << 2) | (spread16_by4(bj3 >> (16 * c)) << 3);
            if (mask == 0) continue;                        // (no hit: nothing of the bookkeeping moves)
            zc.chunk(d, a, lane, base, row_abs, len32, hold32, ((mask >> lane) & 1ull) != 0, mask, b0 + 64 * c);      // lane l stands for sample c0 + l
        }
    }
    zc.finish(d, a, lane, base, row_abs, len32, q.idx);
}

// ---- Lone-hit rows (wfs_lone_hits; the rule: wfs_lone.h): what crosses a threshold outside the rows of the last run,
// read out in rows of its own.  The seeds of a row are lone dark photons (k_lone_scan) and, with wfs_set_lone_noise_hits, samples of
// the noise model that cross (k_lone_noise_scan); the host sorts their keys by (channel, start), k_lone_rows / k_lone_desc form the
// chains and describe their rows like rows without a pulse (RowDesc::src 2), and k_row_empty<NK, DK>, k_rec_keys, k_pack_desc and
// k_pack_res take that row list as they take a batch's: nothing of a finished sample or a record is defined a second time.
struct LoneArgs {
    i64 s0, s1, s_limit;         // the pass owns the rows whose first seed starts in [s0, s1); chains are followed up to s_limit
    i64 a0;                      // s0 - G: first start the scans list, origin of the seed keys
    i64 m0, n_cells;             // first cell and cells of a channel: those of the starts a0 .. s_limit - 1
    i64 n_blocks;                // blocks of LONE_NOISE_BLOCK samples of a channel from a0 on that reach s_limit - 1 (k_lone_noise_scan)
    // the windows of the last run that hold a pulse, in time order: range of their widest row, group; rows of the run (k_tile_rows, k_rows_widen)
    i64 n_win; const i64 *win_l, *win_r; const i32 *win_g; const i64 *row_lo, *row_hi;
    u64 *keys; i64 key_cap, n_keys;      // seeds: lone_key(channel, start - a0, kind); n_keys: the sorted ones (k_lone_rows, k_lone_desc)
    WfsScal *scal;               // the pass's own counter block
    i32 *flag, *cap, *flen;      // [n_keys] 1 / interval slots / finished samples of the row whose first seed this is, else 0
    const i64 *row_of, *itv_off, *fin_off;       // their scans
    i32 *out_channel, *out_nph, *out_nnz; i64 *out_left, *out_right, *out_ixr;      // [rows] the listing of wfs_copy_lone_rows (out_nnz: wfs_copy_lone_row_noise_hits)
};
static_assert(LONE_SCAN_CELLS == 256, "k_lone_scan: a workgroup of 256 lanes, a cell each");

// the last window that begins at or in front of sample t, or -1 (bisection: the windows are in time order)
__device__ __forceinline__ i64 lone_window_at(const LoneArgs &a, i64 t)
{
    i64 lo = 0, hi = a.n_win;
    while (lo < hi) { const i64 mid = (lo + hi) >> 1; if (a.win_l[mid] <= t) lo = mid + 1; else hi = mid; }
    return lo - 1;
}
// the row of channel ch in window w at its final range
struct LoneRow { bool has; i64 l, r; };
__device__ __forceinline__ LoneRow lone_row_of(const WfsDev &d, const LoneArgs &a, i64 w, i32 ch)
{
    LoneRow q{false, 0, 0};
    if (w < 0) return q;
    const i64 ridx = (i64)a.win_g[w] * d.n_tpc + ch;
    const i64 lo = a.row_lo[ridx];
    if (lo != I64_MAX) { const RowSpan sp = row_span(lo, a.row_hi[ridx], d.tw); q.has = true; q.l = sp.left; q.r = sp.right; }
    else if (d.full_readout) { q.has = true; q.l = a.win_l[w]; q.r = a.win_r[w]; }
    return q;
}
// a pulse that starts at `start`: does it stay clear of every row of ch?  (the windows lie more than G apart: one can meet it)
__device__ __forceinline__ bool lone_is_lone(const WfsDev &d, const LoneArgs &a, i32 ch, i64 start)
{
    const LoneRow q = lone_row_of(d, a, lone_window_at(a, start + d.tlen - 1), ch);
    return !(q.has && lone_pulse_meets(start, d.tlen, q.l, q.r));
}

// A lane per cell over a grid of (block of LONE_SCAN_CELLS cells, channel).  The count word is word 0 of site 112 -- the definition of
// the cell's photons cannot differ from dark_sample's --, one ballot per wave, and the all-empty wave does nothing more.  Lanes of
// non-empty cells take their photons from sites 113 / 114, test them against the one row that can hold them, and the wave appends
// its lone ones to the list with one reservation.  The channel's thresholds and constants are uniform over the workgroup.
__global__ __launch_bounds__(LONE_SCAN_CELLS) void k_lone_scan(WfsDev d, LoneArgs a)
{
    const i32 ch = (i32)blockIdx.y;
    const int lane = threadIdx.x & 63;
    const u32 *T = d.dk_thr + (size_t)ch * DK_MAX;
    if (T[0] == 0u || d.gains[ch] == 0.0) return;                            // (uniform)
    const i64 c = (i64)blockIdx.x * LONE_SCAN_CELLS + threadIdx.x;
    const i64 m = a.m0 + c;
    int n = 0;
    if (c < a.n_cells) n = dark_count_of(T, dark_call(d, ch, m, SITE_DARK_N).x);
    if (ballot64(n > 0) == 0) return;                                        // wave-uniform
    i64 st[DK_MAX]; u32 lone = 0;
#pragma unroll
    for (int j = 0; j < DK_MAX; j++) {
        st[j] = 0;
        if (j < n) {
            const DarkPhoton p = dark_photon_of(d, ch, m, j, dark_call(d, ch, m, SITE_DARK_PH + (u32)(j >> 1)));
            st[j] = m * DK_CELL + p.bin - d.samples_before;
            if (st[j] >= a.a0 && st[j] < a.s_limit && lone_is_lone(d, a, ch, st[j])) lone |= 1u << j;
        }
    }
    u64 b[DK_MAX]; i32 total = 0;
#pragma unroll
    for (int j = 0; j < DK_MAX; j++) { b[j] = ballot64(((lone >> j) & 1u) != 0); total += __popcll(b[j]); }
    if (total == 0) return;                                                  // wave-uniform
    i64 base = 0;
    if (lane == 0) base = (i64)atomicAdd((u64 *)&a.scal->n_lone_seeds, (u64)total);
    base = __shfl(base, 0, 64);
    const u64 lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < DK_MAX; j++) {
        const i64 at = base + __popcll(b[j] & lt);
        if (((lone >> j) & 1u) && at < a.key_cap) a.keys[at] = lone_key(ch, st[j] - a.a0, LONE_KIND_PHOTON);
        base += __popcll(b[j]);
    }
}

// The noise-hit seeds (wfs_set_lone_noise_hits): a wave per block of LONE_NOISE_BLOCK consecutive absolute samples of a
// channel from a0 on, four samples per lane, over a grid of (four blocks, channel).  The value is made exactly as k_row_empty makes the
// sample of a row without a pulse -- noise_four (every lane of the wave draws), dark_block when rates are set, finish_four -- and
// compared with thr_zle[ch] as the ZLE kernels compare; nothing is stored.  Four ballots of the hit nibbles, and the wave without a
// hit, almost all of them, is done.  Otherwise the hit lanes test their samples against the one row that can hold them, and the wave
// appends its seeds to the list with one reservation, as k_lone_scan does.  No LDS, no scratch.  ch < min(noise_channels, n_tpc).
template <int NK, bool DK>
__global__ __launch_bounds__(256) void k_lone_noise_scan(WfsDev d, LoneArgs a)
{
    static_assert(NK >= 3, "a noise table has no value at an absolute sample");
    static_assert(LONE_NOISE_BLOCK == 256, "a wave takes 256 samples, four per lane");
    const i32 ch = (i32)blockIdx.y;
    const int lane = threadIdx.x & 63;
    const i64 blk = (i64)blockIdx.x * 4 + wave_in_block();
    if (blk >= a.n_blocks) return;                                           // wave-uniform
    const i64 tb = a.a0 + blk * LONE_NOISE_BLOCK;
    Raw4<NK> s4;
    s4.acc[0] = s4.acc[1] = s4.acc[2] = s4.acc[3] = 0;
    noise_four<NK>(d, s4, noise_row_of<NK>(d, ch, true), ch, tb, 0u, lane);
    if constexpr (DK) { const i32 dch = dark_channel_of(d, ch, false); if (dch >= 0) dark_block(d, dch, tb, lane, s4.acc); }      // (every lane of the wave is here)
    const i64 thr = d.thr_zle[ch], t = tb + 4 * lane;
    u32 nib = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) nib |= (t + j < a.s_limit && (i64)finish_four<NK>(d, s4, j, false, true) < thr) ? (1u << j) : 0u;
    if ((ballot64((nib & 1u) != 0) | ballot64((nib & 2u) != 0) | ballot64((nib & 4u) != 0) | ballot64((nib & 8u) != 0)) == 0) return;      // wave-uniform
    if (nib) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (!((nib >> j) & 1u)) continue;
            const LoneRow q = lone_row_of(d, a, lone_window_at(a, t + j), ch);
            if (!lone_seed_clear(t + j, q.has, q.l, q.r)) nib &= ~(1u << j);
        }
    }
    u64 b[4]; i32 total = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) { b[j] = ballot64(((nib >> j) & 1u) != 0); total += __popcll(b[j]); }
    if (total == 0) return;                                                  // wave-uniform
    i64 base = 0;
    if (lane == 0) base = (i64)atomicAdd((u64 *)&a.scal->n_lone_seeds, (u64)total);
    base = __shfl(base, 0, 64);
    const u64 lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const i64 at = base + __popcll(b[j] & lt);
        if (((nib >> j) & 1u) && at < a.key_cap) a.keys[at] = lone_key(ch, t + j - a.a0, LONE_KIND_NOISE);
        base += __popcll(b[j]);
    }
}

// Its family (wfs_family.h), declared beside the kernel: the axes are nk - 3, the drawn noise kinds alone, and dk, dev.dk_thr -- dark-count
// rates are set and D is part of the value.  No dynamic LDS, hence no cap.
const auto K_LONE_NOISE_SCAN = family<3, 2>("k_lone_noise_scan", 0, [](auto nk, auto dk) { return &k_lone_noise_scan<nk() + 3, dk() != 0>; });

// The chain that seed i of the sorted list begins, if it begins one this pass owns: seed i has no seed of its channel within G in
// front of it and starts in [s0, s1); the chain runs on while the next seed of the channel starts at most G behind the last (the list
// ends in front of s_limit).  Its range: lone_range, clipped by the one row that can lie within its margins on either side.  A chain
// cannot straddle a row (lone_cannot_straddle, lone_seeds_cannot_straddle): every row of the run holds a pulse or spans its window.
// n: the lone dark photons among the chain's seeds, nn: the noise-hit seeds.
struct LoneChain { bool owned; i32 ch, n, nn; i64 left, right; };
__device__ __forceinline__ LoneChain lone_chain_of(const WfsDev &d, const LoneArgs &a, i64 i)
{
    const i64 G = lone_gap(d.tlen, d.tw);
    const u64 key = a.keys[i];
    LoneChain c{false, lone_key_channel(key), 0, 0, 0, 0};
    const i64 first = a.a0 + lone_key_rel(key);
    if (first < a.s0 || first >= a.s1) return c;
    if (i > 0) { const u64 pk = a.keys[i - 1]; if (lone_key_channel(pk) == c.ch && first - (a.a0 + lone_key_rel(pk)) <= G) return c; }
    i64 last = first, j = i + 1;
    i32 nn = lone_key_kind(key) == LONE_KIND_NOISE ? 1 : 0;
    for (; j < a.n_keys; j++) {
        const u64 nk = a.keys[j];
        const i64 s = a.a0 + lone_key_rel(nk);
        if (lone_key_channel(nk) != c.ch || s - last > G) break;
        last = s; nn += lone_key_kind(nk) == LONE_KIND_NOISE ? 1 : 0;
    }
    const LoneRow pr = lone_row_of(d, a, lone_window_at(a, first - 1), c.ch);
    const LoneRow nr = lone_row_of(d, a, lone_window_at(a, last + d.tlen - 1 + d.tw), c.ch);
    const LoneRange rg = lone_range(first, last, d.tlen, d.tw, (pr.has && pr.r < first) ? pr.r : I64_MIN, (nr.has && nr.l > last) ? nr.l : I64_MAX, a.s_limit);
    c.owned = true; c.n = (i32)(j - i) - nn; c.nn = nn; c.left = rg.left; c.right = rg.right;
    return c;
}
// thread per listed seed: the flag of a row's first seed, the interval slots and the finished samples its row reserves
__global__ void k_lone_rows(WfsDev d, LoneArgs a)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_keys) return;
    const LoneChain c = lone_chain_of(d, a, i);
    i64 len = c.owned ? c.right - c.left + 1 : 0;
    if (len > LONE_MAX_ROW_LEN) { atomicMax(&a.scal->lone_error, (i64)1); len = 0; }
    a.flag[i] = len > 0 ? 1 : 0;
    a.cap[i] = len > 0 ? (i32)zle_slots(len, zle_holdoff(d.tw)) : 0;
    a.flen[i] = len > 0 ? fin_padded_len((i32)len) : 0;
}
// thread per listed seed, behind the scans: the descriptor of its row (as k_row_desc writes one for a row without a pulse) and the listing
__global__ void k_lone_desc(WfsDev d, LoneArgs a, RowDesc *desc)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_keys || !a.flag[i]) return;
    const LoneChain c = lone_chain_of(d, a, i);
    const i64 row = a.row_of[i];
    const bool table = d.enable_noise && !d.nm_cells && (d.noise || d.noise_f);
    RowDesc q;
    q.acc_off = a.fin_off[i]; q.row_abs = c.left; q.itv_base = a.itv_off[i];
    q.ixr = lone_ix_rand(philox4x32_10((u32)(u64)c.left, (u32)((u64)c.left >> 32), (u32)c.ch, SITE_LONE_IX, d.k0, d.k1).x, table ? (i64)d.noise_len : 0);
    q.thr = d.thr_zle[c.ch]; q.idx = row; q.len = (i32)(c.right - c.left + 1); q.channel = c.ch; q.he = 0; q.src = 2;
    desc[row] = q;
    atomicMin(&a.scal->key_origin, q.row_abs); atomicMax(&a.scal->key_end, q.row_abs + (i64)q.len);
    a.out_channel[row] = c.ch; a.out_nph[row] = c.n; a.out_nnz[row] = c.nn; a.out_left[row] = c.left; a.out_right[row] = c.right; a.out_ixr[row] = q.ixr;
}

// ---- The overlay pass (wfs_overlay_records; the rule: wfs_overlay.h): two streams of raw_records, A the simulation's and B
// the recorded background, merged per channel into one valid stream.  Records i < n_a are A's.  The host sorts three times between
// these kernels -- the records by (stream, channel, time), the pulses by (channel, start, stream), the output records by (time, channel)
// -- and scans three flags; everything the kernels write is a buffer of wfs_handle::overlay.
struct OverlayScal {
    i64 smin, smax;              // smallest fragment start, largest last sample of a pulse (absolute samples).  k_ov_check -> host
    i64 n_bad; u64 first_bad;    // records that break validity; the first of them, index << 8 | OvBad.  k_ov_check, k_ov_valid -> host
    i64 too_long;                // merged pulses of more than 2^31 - 1 samples.  k_ov_count -> host
};
struct OverlayArgs {
    const u32 *src_a, *src_b; i64 n_a, n;        // the records of the two streams, REC_DWORDS each; n = n_a + n_b
    i32 dt, n_rows, baseline; const i32 *base;   // cfg.dt, row slots, cfg.baseline; the recorded baseline per channel
    OvBits bits; i64 smin;
    OverlayScal *scal;
    u64 *key; u32 *val;                          // [n] record keys and indices: unsorted for k_ov_keys, sorted from k_ov_valid on
    i32 *flag; const i32 *pulse_of;              // [n] 1 for the first fragment of a pulse (sorted order); its inclusive scan
    i64 n_pulses; u64 *pkey; u32 *plen;          // [pulses] pulse keys and lengths: unsorted for k_ov_pulses, sorted from k_ov_ends on
    u64 *ekey; const u64 *run_max;               // [pulses] channel | last sample; its running maximum
    i32 *head; const i32 *merged_of;             // [pulses] 1 for the first pulse of a merged pulse; its inclusive scan
    i64 n_merged; u64 *m_first, *m_last;         // [merged] channel | first sample, channel | last sample
    i64 *m_nrec; const i64 *rec_end;             // [merged] records; their inclusive scan
    i64 n_out; u64 *okey; u32 *oval;             // [records] output keys and merged pulses: unsorted for k_ov_out_keys, sorted for k_ov_fill
    u32 *out;                                    // the output records in (time, channel) order
};
__device__ __forceinline__ const u32 *ov_record(const OverlayArgs &a, i64 i) { return i < a.n_a ? a.src_a + (size_t)i * REC_DWORDS : a.src_b + (size_t)(i - a.n_a) * REC_DWORDS; }
__device__ __forceinline__ void ov_report(const OverlayArgs &a, i64 i, int bad)
{
    atomicAdd((u64 *)&a.scal->n_bad, 1ull); atomicMin(&a.scal->first_bad, ((u64)i << 8) | (u64)bad);
}
// thread per record: what the record alone decides, and the range of the pass (one atomic pair per wave)
__global__ void k_ov_check(OverlayArgs a)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    i64 lo = I64_MAX, hi = I64_MIN;
    if (i < a.n) {
        const OvHeader q = ov_header(ov_record(a, i));
        const int bad = ov_record_check(q, a.dt, a.n_rows);
        if (bad) ov_report(a, i, bad);
        else { lo = ov_fragment_sample(q); hi = ov_pulse_last(q); }
    }
    for (int o = 32; o > 0; o >>= 1) { const i64 l2 = __shfl_down(lo, o, 64), h2 = __shfl_down(hi, o, 64); lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi; }
    if ((threadIdx.x & 63) == 0 && lo != I64_MAX) { atomicMin(&a.scal->smin, lo); atomicMax(&a.scal->smax, hi); }
}
__global__ void k_ov_keys(OverlayArgs a)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const OvHeader q = ov_header(ov_record(a, i));
    a.key[i] = ov_record_key(a.bits, i < a.n_a ? 0 : 1, q.channel, ov_fragment_sample(q) - a.smin);
    a.val[i] = (u32)i;
}
// thread per sorted record: the record against the one in front of it on its channel in its stream; the flag of a pulse's first fragment
__global__ void k_ov_valid(OverlayArgs a)
{
    const i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    const u64 k = a.key[p];
    const OvHeader q = ov_header(ov_record(a, a.val[p]));
    const bool has_prev = p > 0 && (a.key[p - 1] >> a.bits.sbits) == (k >> a.bits.sbits);
    const bool is_last = p == a.n - 1 || (a.key[p + 1] >> a.bits.sbits) != (k >> a.bits.sbits);
    OvHeader pr = q;
    if (has_prev) pr = ov_header(ov_record(a, a.val[p - 1]));
    int bad = ov_pair_check(has_prev, pr, q);
    if (!bad && is_last) bad = ov_last_check(q);
    if (bad) ov_report(a, a.val[p], bad);
    a.flag[p] = q.record_i == 0 ? 1 : 0;
}
// thread per sorted record: the key and the length of the pulse it begins
__global__ void k_ov_pulses(OverlayArgs a)
{
    const i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n || !a.flag[p]) return;
    const u64 k = a.key[p];
    const i64 j = a.pulse_of[p] - 1;
    a.pkey[j] = ov_pulse_key(a.bits, (int)(k >> (a.bits.sbits + a.bits.chbits)), ov_key_channel(a.bits, k), ov_key_rel(a.bits, k));
    a.plen[j] = ov_record(a, a.val[p])[REC_PULSE_LENGTH];
}
// thread per sorted pulse: channel | last sample (the last sample is at most smax - smin: no carry into the channel)
__global__ void k_ov_ends(OverlayArgs a)
{
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < a.n_pulses) a.ekey[j] = (a.pkey[j] >> 1) + (u64)(a.plen[j] - 1u);
}
__global__ void k_ov_heads(OverlayArgs a)
{
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < a.n_pulses) a.head[j] = (j == 0 || ov_begins_merged(a.run_max[j - 1], a.pkey[j])) ? 1 : 0;
}
// thread per sorted pulse: the first pulse of a merged pulse writes where it begins, the last where it ends
__global__ void k_ov_merged(OverlayArgs a)
{
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.n_pulses) return;
    const i64 m = a.merged_of[j] - 1;
    if (a.head[j]) a.m_first[m] = a.pkey[j] >> 1;
    if (j == a.n_pulses - 1 || a.head[j + 1]) a.m_last[m] = a.run_max[j];
}
__global__ void k_ov_count(OverlayArgs a)
{
    const i64 m = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n_merged) return;
    const u64 len = a.m_last[m] - a.m_first[m] + 1ull;         // (one channel in both)
    if (len > 0x7fffffffull) { atomicAdd((u64 *)&a.scal->too_long, 1ull); a.m_nrec[m] = 0; return; }
    a.m_nrec[m] = records_of((i32)len);
}
// thread per merged pulse: the keys of its records
__global__ void k_ov_out_keys(OverlayArgs a)
{
    const i64 m = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n_merged) return;
    const i64 nrec = a.m_nrec[m], o0 = a.rec_end[m] - nrec;
    const u64 first = a.m_first[m];
    const i32 ch = ov_key_channel(a.bits, first); const i64 rel = ov_key_rel(a.bits, first);
    for (i64 f = 0; f < nrec; f++) {
        if (o0 + f >= a.n_out) break;
        a.okey[o0 + f] = ov_output_key(a.bits, ch, rec_fragment_sample(rel, f)); a.oval[o0 + f] = (u32)m;
    }
}
// the first sorted record at or behind `key` (bisection over the record keys)
__device__ __forceinline__ i64 ov_lower_bound(const OverlayArgs &a, u64 key)
{
    i64 lo = 0, hi = a.n;
    while (lo < hi) { const i64 mid = (lo + hi) >> 1; if (a.key[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}
// Wave per output record, in its sorted slot.  Lane l < 55 holds the samples 2 l and 2 l + 1 of the record.  The source fragments that
// can meet its samples S .. S + L - 1 start in S - 109 .. S + L - 1 on its channel: per stream a bisection over the sorted record keys
// and a walk over the few that follow (a fragment has at least one sample and the fragments of a stream share none: at most L + 109).
// Every one of them belongs to this merged pulse, which holds every pulse that shares a sample with it.  Sums in registers as i32, the
// rule of ov_sample, one dword store per lane; lane 0 writes the header.
__global__ __launch_bounds__(256) void k_ov_fill(OverlayArgs a)
{
    const int lane = threadIdx.x & 63;
    const i64 r = (i64)blockIdx.x * 4 + wave_in_block();
    if (r >= a.n_out) return;
    const u64 ok = a.okey[r];
    const i64 m = a.oval[r];
    const i32 ch = ov_output_channel(a.bits, ok);
    const i64 S = ov_output_rel(a.bits, ok), first = ov_key_rel(a.bits, a.m_first[m]);
    const i32 plen = (i32)(a.m_last[m] - a.m_first[m] + 1ull), f = (i32)((S - first) / WFS_SPR), L = rec_fragment_len(plen, f);
    const i64 s0 = S + 2 * lane;
    i32 va[2] = {0, 0}, vb[2] = {0, 0}; bool ca[2] = {false, false}, cb[2] = {false, false};
    for (int stream = 0; stream < 2; stream++) {
        const u64 kbase = ov_record_key(a.bits, stream, ch, 0);
        const u64 kend = kbase + (u64)(S + L);
        for (i64 p = ov_lower_bound(a, kbase + (u64)(S > WFS_SPR - 1 ? S - (WFS_SPR - 1) : 0)); p < a.n; p++) {
            const u64 k = a.key[p];
            if (k >= kend) break;
            const u32 *rec = ov_record(a, a.val[p]);
            const i64 fs = ov_key_rel(a.bits, k); const i32 flen = (i32)rec[REC_LENGTH];
            const int16_t *data = (const int16_t *)(rec + REC_HEADER_DWORDS);
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const i64 at = s0 + u - fs;
                if (lane < WFS_SPR / 2 && at >= 0 && at < flen && 2 * lane + u < L) {
                    const i32 v = data[at];
                    if (stream == 0) { va[u] = v; ca[u] = true; } else { vb[u] = v; cb[u] = true; }
                }
            }
        }
    }
    u32 *dst = a.out + (size_t)r * REC_DWORDS;
    if (lane < WFS_SPR / 2) {
        const i32 base = a.base[ch];
        u32 w = 0;
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const i32 v = (ca[u] || cb[u]) ? ov_sample(ca[u], cb[u], va[u], vb[u], a.baseline, base) : 0;
            w |= (u32)(uint16_t)(int16_t)v << (16 * u);
        }
        dst[REC_HEADER_DWORDS + lane] = w;
    }
    if (lane == 0) {
        const RecHeader h = rec_header(a.dt, rec_dt_channel(a.dt, ch), a.smin + first, plen, f);
#pragma unroll
        for (int q = 0; q < REC_HEADER_DWORDS; q++) dst[q] = h.w[q];
    }
}

// Records ordered by (time, channel) as strax.sort_by_time leaves them (strax_interface.py:453): one key per record; the
// windows of a batch do not overlap in time, so one sort of the whole batch keeps every window contiguous.
__global__ __launch_bounds__(256) void k_rec_keys(WfsDev d, ZleArgs a)
{
    const int lane = threadIdx.x & 63;
    const i64 r = (i64)blockIdx.x * 4 + wave_in_block();
    if (r >= a.n_active_rows) return;
    const RowDesc q = a.desc[r];
    const i32 count = a.itv_n[q.idx];
    if (count == 0) return;
    i64 rec = a.rec_off[q.idx];
    const i64 key_base = a.key_base->key_origin;
    for (i32 k = 0; k < count; k++) {
        const i64 left = a.itv_left[q.itv_base + k]; const i32 plen = (i32)(a.itv_right[q.itv_base + k] - left + 1);
        if (plen <= 0) continue;
        const i32 need = records_of(plen);
        for (i32 f = lane; f < need; f += 64) {
            if (rec + f >= a.rec_capacity) break;
            a.rec_key[rec + f] = ((u64)(rec_fragment_sample(left, (i64)f) - key_base) << REC_KEY_SHIFT) | (u64)(u32)q.channel;
            a.rec_val[rec + f] = (u32)(rec + f);
        }
        rec += need;
    }
}
__global__ void k_invert_perm(const u32 *val, u32 *dest, i64 n) { const i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x; if (p < n) dest[val[p]] = (u32)p; }

// One 64-byte descriptor per active row for k_pack, made once the record offsets are known (thread per row): the row's place, its
// first record, its first interval.  With ~10^7 short rows a wave of k_pack spent most of its life in the chain row descriptor ->
// interval count and record offset -> interval bounds -> samples; now it is descriptor -> samples.
struct __attribute__((aligned(64))) PackDesc {
    i64 acc_off, rec, row_abs, left0, ixr, itv_base;
    i32 plen0, count, channel, len_he_src;       // len | he << 20 | src << 21 (a row is shorter than 10^6 samples)
};
__global__ void k_pack_desc(ZleArgs a)
{
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_active_rows) return;
    const RowDesc q = a.desc[r];
    PackDesc p;
    p.acc_off = q.acc_off; p.rec = a.rec_off[q.idx]; p.row_abs = q.row_abs; p.ixr = q.ixr; p.itv_base = q.itv_base;
    p.count = a.itv_n[q.idx]; p.channel = q.channel; p.len_he_src = q.len | (q.he << 20) | (q.src << 21);
    p.left0 = 0; p.plen0 = 0;
    if (p.count > 0) { p.left0 = a.itv_left[q.itv_base]; p.plen0 = (i32)(a.itv_right[q.itv_base] - p.left0 + 1); }
    a.pdesc[r] = p;
}

// The records of the resident rows: their finished 16-bit samples exist (k_row_pulse), two of them are a dword of a record.  A kernel
// of its own with the few arguments it needs: in the general k_pack the scalar unit (one per CU) was the bottleneck -- ~350 scalar
// instructions per row for address arithmetic, spilled descriptors and the branches around four unrolled records.  Here the loads of
// up to four records are unconditional (indices clamped into the row), the header dwords are selected, not branched to, and the
// stores are predicated per lane.
struct PackResArgs { const PackDesc *pdesc; const int16_t *fin; const i64 *itv_left, *itv_right; uint8_t *records; const u32 *rec_dest; i64 rec_capacity, n_rows; i32 spr, dt; };
__global__ __launch_bounds__(256) void k_pack_res(PackResArgs a)
{
    const int lane = threadIdx.x & 63;
    const i64 r = (i64)blockIdx.x * 4 + wave_in_block();
    if (r >= a.n_rows) return;
    const PackDesc q = a.pdesc[r];
    if (q.count == 0) return;
    const int16_t *fin = a.fin + q.acc_off;
    const i32 last = fin_last_pair(q.len_he_src & 0xfffff);
    constexpr int spr = WFS_SPR; constexpr int rec_dwords = REC_DWORDS;
    const i64 rec_bytes = WFS_RECORD_BYTES;
    const u32 w3 = rec_dt_channel(a.dt, q.channel);
    i64 rec = q.rec;
    for (i32 k = 0; k < q.count; k++) {
        const i64 left = k == 0 ? q.left0 : a.itv_left[q.itv_base + k]; const i32 plen = k == 0 ? q.plen0 : (i32)(a.itv_right[q.itv_base + k] - left + 1);
        if (plen <= 0) continue;
        const i32 need = records_of(plen);
        const i32 off = (i32)(left - q.row_abs);                   // even (rawdata.py:305-306), and the row starts on a multiple of four samples of fin
        for (int q0 = 0; q0 < rec_dwords; q0 += 64) {              // (one pass unless a record is longer than 64 dwords)
            const int qd = q0 + lane;
            const int s0 = (qd - REC_HEADER_DWORDS) * 2;            // first of the lane's two samples (lanes of the header: negative)
            const i32 lane_off = off + (s0 < 0 ? 0 : s0);
            for (i32 f0 = 0; f0 < need; f0 += 4) {
                u32 two[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { i32 i0 = lane_off + spr * (f0 + u); i0 = i0 > last ? last : i0; two[u] = *(const u32 *)(fin + i0); }      // (past the row: a valid pair, dropped)
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const i32 f = f0 + u;
                    const i64 slot = a.rec_dest ? (i64)a.rec_dest[rec + (f < need ? f : 0)] : rec + f;
                    u32 *out = (u32 *)(a.records + slot * rec_bytes);
                    const RecHeader hd = rec_header(a.dt, w3, left, plen, f);
                    const i32 length = (i32)hd.w[REC_LENGTH];
                    u32 w = (s0 < length ? two[u] & 0xffffu : 0u) | (s0 + 1 < length ? two[u] & 0xffff0000u : 0u);
#pragma unroll
                    for (int j = 0; j < REC_HEADER_DWORDS; j++) w = qd == j ? hd.w[j] : w;      // (selected, not branched to)
                    if (f < need && qd < rec_dwords && rec + f < a.rec_capacity) out[qd] = w;
                }
            }
        }
        rec += need;
    }
}

// one wave per row: write its intervals as strax raw_records (strax_interface.py:425-435).  A record is 24 bytes of header and
// samples_per_record int16: lane q writes dword q of the record (61 dwords with 110 samples: three idle lanes, no division by the
// record length anywhere), PACK_U records in flight so that the loads of one do not wait behind the stores of the one before.
template <int NK, bool DK>
__global__ __launch_bounds__(256) void k_pack(WfsDev d, ZleArgs a)
{
    const int lane = threadIdx.x & 63;
    const i64 r = (i64)blockIdx.x * 4 + wave_in_block();
    if (r >= a.n_front) return;                             // (the rows behind n_front: k_pack_res)
    const PackDesc q = a.pdesc[r];
    const i32 count = q.count;
    if (count == 0) return;
    const i32 channel = q.channel; const bool he = ((q.len_he_src >> 20) & 1) != 0; const int src = q.len_he_src >> 21;
    const i32 *acc = (src ? a.tbuf : a.raw) + q.acc_off;
    const i64 row_abs = q.row_abs;
    const i64 ixr = q.ixr;
    const i64 base = q.itv_base;
    const i32 len32 = q.len_he_src & 0xfffff;
    constexpr int spr = WFS_SPR; constexpr int rec_dwords = REC_DWORDS;
    const i64 rec_bytes = WFS_RECORD_BYTES;
    const bool noisy = NK != 0 && channel < d.noise_channels;
    const i32 dch = DK ? dark_channel_of(d, channel, he) : -1;
    constexpr bool TABLE = NK == 1 || NK == 2;
    const bool fast_loads = !TABLE || (d.noise_len >= NOISE_MIN_FAST && spr <= NOISE_MIN_FAST / 2);       // (as in k_zle: a scalar noise start per record)
    const u32 nixr = noisy ? (u32)ixr : 0u;
    const void *noise_row = noise_row_of<NK>(d, channel, noisy);
    const u32 w3 = rec_dt_channel(d.dt, channel);
    constexpr int PACK_U = NK >= 4 ? 1 : 4;         // (kind 4 draws where the others load: one record's draws at a time, one copy of their code)
    i64 rec = q.rec;
    for (i32 k = 0; k < count; k++) {
        const i64 left = k == 0 ? q.left0 : a.itv_left[base + k]; const i32 plen = k == 0 ? q.plen0 : (i32)(a.itv_right[base + k] - left + 1);
        if (plen <= 0) continue;
        const i32 need = records_of(plen);
        const i32 off = (i32)(left - row_abs);                     // first sample of the interval inside the row
        for (int q0 = 0; q0 < rec_dwords; q0 += 64) {              // (one pass unless a record is longer than 64 dwords)
            const int qd = q0 + lane;
            const int s0 = (qd - REC_HEADER_DWORDS) * 2;                           // first of the lane's two samples (lanes of the header: negative)
            u32 nrun = 0;                                           // noise index of the next record's first sample (a scalar)
            if constexpr (TABLE) { if (fast_loads) nrun = (nixr + (u32)off) % (u32)d.noise_len; }
            const u32 noff = (u32)(s0 < 0 ? 0 : s0);
            for (i32 f0 = 0; f0 < need; f0 += PACK_U) {
                RawSample<NK> lo[PACK_U], hi[PACK_U];
                if (fast_loads) {
#pragma unroll
                    for (int u = 0; u < PACK_U; u++) {
                        const i32 f = f0 + u;
                        if (f >= need) break;                       // wave-uniform
                        i32 i0 = off + rec_fragment_first(f) + (i32)noff;
                        i0 = i0 > len32 - 1 ? len32 - 1 : i0;       // (lanes past the record's samples read a valid sample and drop it)
                        const i32 i1 = i0 + 1 > len32 - 1 ? len32 - 1 : i0 + 1;
                        lo[u] = load_sample<NK, DK>(d, acc, i0, noise_row, nrun, noff, channel, row_abs, dch); hi[u] = load_sample<NK, DK>(d, acc, i1, noise_row, nrun, noff + 1u, channel, row_abs, dch);
                        if constexpr (TABLE) nrun = noise_advance(nrun, (u32)spr, (u32)d.noise_len);
                    }
                }
#pragma unroll
                for (int u = 0; u < PACK_U; u++) {
                    const i32 f = f0 + u;
                    if (f >= need) break;
                    if (rec + f >= a.rec_capacity) break;
                    u32 *out = (u32 *)(a.records + (a.rec_dest ? (i64)a.rec_dest[rec + f] : rec + f) * rec_bytes);
                    const RecHeader hd = rec_header<true>(d.dt, w3, left, plen, f);
                    const i32 length = (i32)hd.w[REC_LENGTH];
                    u32 w;
                    if (qd >= REC_HEADER_DWORDS) {
                        u32 vlo, vhi;
                        if (fast_loads) { vlo = (u32)(uint16_t)finish_loaded(d, lo[u], he, noisy); vhi = (u32)(uint16_t)finish_loaded(d, hi[u], he, noisy); }
                        else {
                            const i64 i0 = (i64)off + rec_fragment_first(f) + s0;
                            vlo = s0 < length ? (u32)(uint16_t)finish_sample<NK, DK>(d, acc, i0, channel, he, ixr, row_abs, dch) : 0u;
                            vhi = s0 + 1 < length ? (u32)(uint16_t)finish_sample<NK, DK>(d, acc, i0 + 1, channel, he, ixr, row_abs, dch) : 0u;
                        }
                        w = (s0 < length ? vlo : 0u) | ((s0 + 1 < length ? vhi : 0u) << 16);
                    }
                    else if (qd == REC_TIME_LO) w = hd.w[REC_TIME_LO];              // (branched to, not selected)
                    else if (qd == REC_TIME_HI) w = hd.w[REC_TIME_HI];
                    else if (qd == REC_LENGTH) w = hd.w[REC_LENGTH];
                    else if (qd == REC_DT_CHANNEL) w = hd.w[REC_DT_CHANNEL];
                    else if (qd == REC_PULSE_LENGTH) w = hd.w[REC_PULSE_LENGTH];
                    else w = hd.w[REC_RECORD_I];
                    if (qd < rec_dwords) out[qd] = w;
                }
            }
        }
        rec += need;
    }
}

// ------------------------------------------------------------------------------------------------ generation
// One 64-byte descriptor per photon block (k_block_emitters): a generator workgroup starts from ONE scalar load instead of a
// chain of dependent look-ups (block -> emitters -> instruction -> pulse set ...), each a global round trip.
struct __attribute__((aligned(64))) BlockDesc {
    i64 e_lo;             // first emitter of the block
    i64 itime;            // origin of the photon times of the instruction's pulse set
    i64 R0;               // index of the block's first photon among its instruction's photons
    i32 ins;              // instruction of a single-instruction block, -1: the block spans instructions (generic path)
    i32 nwin;             // emitters of the block + 2 (<= GEN_WIN)
    i32 set, row;         // pulse set, channel CDF row
    u32 gid, eb, jbase;   // Philox coordinates: instruction id, emitter base, emitter id of e_lo
    i32 is_s2;
    u32 sbase;            // photons of the instructions in front of this one in its pulse set (order keys count through the set)
    i32 multi;            // the pulse set holds several instructions: order keys are written for every photon (the tile is sorted as a whole)
};

struct GenArgs {
    i64 n_ins, n_psets, n_emitters, n_photons;
    const u32 *ins_embase;        // [n_ins] offset of the instruction's emitter ids in the Philox counters (0 for primaries; the k-th
                                  // electron-afterpulse instruction of a parent shares the parent's gid and uses (k + 1) << 20)
    const i32 *ins_set;           // [n_ins] pulse set (one Pulse.__call__, rawdata.py:108-127) of every instruction; tiles are (set, channel)
    const i64 *set_ins_off; const i32 *set_ins_list;      // set -> its instructions (CSR)
    const i64 *set_t0;            // [n_sets] time origin of the set's photon times
    const int8_t *ins_type; const i64 *ins_time; const i32 *ins_amp; const u32 *ins_gid;
    const double *ins_p, *ins_dm, *ins_ds, *ins_sc; const i32 *ins_cdfrow; const double *cdf_table;
    const uint2 *chan_alias; i32 ch_lg;   // [n_cdf][1 << ch_lg] Walker alias cells of every channel CDF row (k_chan_alias): {threshold, alias channel}
    const i64 *em_off;            // [n_ins + 1] first emitter of each instruction
    i64 *em_time; i32 *em_nph; i32 *em_ins; const i64 *em_ph_off;
    double *em_zg;                // [n_emitters] gain-spread normal of a surviving electron whose photon number k_s2_photons draws (PTRS), NaN elsewhere
    const double *pois_cdf; const i32 *pois_kmin;     // [n_ins][POIS_W] cumulative Poisson table of the instruction's secondary gain, first k (-1: PTRS, -2: gain <= 0)
    i32 *tile_count; const i64 *tile_off; i32 *tile_cursor; i32 *tile_tmin, *tile_tmax;
    PhotonRec *ph;
    u32 *ph_idx;                  // [photons] order key of every stored photon: its index among its pulse set's photons, instruction by
                                  // instruction (afterpulses: element << 29 | key of the parent) -- k_tile_order sorts every tile by it
    u32 *ins_sbase;               // [n_ins] photons of the instructions in front of this one in its pulse set (k_set_bases)
    i32 *tile_tail;               // [primary tiles] photons that the generic path puts BEHIND the tile's block ranges: those of an instruction that
                                  // began in an earlier block (count pass; the fill pass uses it as their cursor)
    i32 *tile_tailbase;           // [primary tiles] first slot of those photons inside the tile (k_block_ranges)
    i32 *ins_fullsort;            // [n_ins] 1: the tiles of this instruction are sorted as a whole (several instructions in its pulse set, or a block
                                  // in the MIDDLE of the instruction that takes the generic path: more emitters than the LDS window holds)
    i64 n_blocks;
    i64 xcd_chunk;                // XCD x (workgroup id % 8) walks the photon blocks [x * xcd_chunk, (x + 1) * xcd_chunk) in order
    i32 *eblk_ins;                // [ceil(n_emitters / 256) + 1] instruction of the first emitter of every block of k_s2_electrons
    i64 *blk_e;                   // [n_blocks][2] first / last emitter of every photon block
    u32 *blk_base;                // [n_blocks][n_tpc] start of the block's photons inside each tile (written by the count pass)
    unsigned short *blk_cnt;      // [n_blocks][n_tpc] the block's photons per channel (count pass, single-instruction blocks)
    i32 *blk_ins;                 // [n_blocks] instruction of a single-instruction block, -1 otherwise (k_block_emitters)
    struct BlockDesc *blk_desc;   // [n_blocks] everything a generator workgroup needs to know about its block
    const i32 *ins_fused;         // [n_ins] 1: the instruction's photons are generated tile by tile (wfs_tilegen.h), or nullptr
    i64 *ins_ph0;                 // [n_ins + 1] first photon (generation order) of every instruction: em_ph_off[em_off[i]]
    double *el_stat;              // [n_ins][4] electrons: n, sum t, sum t^2 ; el_minmax [n_ins][2]
    i64 *el_minmax;
    WfsScal *scal;
    // model variants of the photon delays (wfs_set_delay_models / wfs_set_instruction_models); tabs == nullptr: the two default tables
    const AliasTab *tabs;         // [n_tables + 2] user tables, then the default S1 and S2 tables
    const i32 *ins_tab, *ins_tabb;        // [n_ins] table of the instruction's photons on top / bottom array channels
    const i32 *ins_pzi; const double *ins_pzf;    // [n_ins] S1 optical propagation: z cell of the spline grid and normalised distance in it (-1: none)
    const double *prop_top, *prop_bot; i32 prop_nu; double prop_u0, prop_du;      // spline node values [nz][nu], u grid
    // 'garfield_gas_gap' luminescence (s2.py:413-483): inverse CDFs of the excitation time per tabulated gas gap [gg_n][gg_L];
    // per instruction the table at or below its gas gap (-1: not this model), the interpolation weight towards the next
    // table, and the sum of its photons' excitation times in units of 2^-20 ns (k_gg_sum; the mean is subtracted, s2.py:447)
    const double *gg_inv; i32 gg_n, gg_L; const i32 *ins_gg; const double *ins_ggw; i64 *ins_ggsum;
};

// S1 optical propagation delay (s1.py:241-260): multilinear interpolation of the spline nodes, evaluated as scipy's
// RegularGridInterpolator does (sum over the cell's corners of value * weights); same operation order as the oracle
__device__ __forceinline__ double s1_propagation(const GenArgs &a, bool bottom, i32 zi, double zf, u32 w)
{
    const double u = ((double)w + 0.5) * (1.0 / 4294967296.0);
    const double *T = bottom ? a.prop_bot : a.prop_top; const i32 nu = a.prop_nu;
    i32 ui = (i32)floor((u - a.prop_u0) / a.prop_du);
    ui = ui < 0 ? 0 : (ui > nu - 2 ? nu - 2 : ui);
    const double uf = (u - (a.prop_u0 + (double)ui * a.prop_du)) / a.prop_du;
    const double *r0 = T + (i64)zi * nu + ui, *r1 = r0 + nu;
    double v = r0[0] * ((1.0 - zf) * (1.0 - uf));
    v += r0[1] * ((1.0 - zf) * uf);
    v += r1[0] * (zf * (1.0 - uf));
    v += r1[1] * (zf * uf);
    return v;
}

// excitation time of one photon from the garfield gas gap tables (s2.py:436-446): a uniform position on the inverse CDF,
// interpolated between the two tables that bracket the instruction's gas gap; same operation order as the oracle
__device__ __forceinline__ double gg_time(const GenArgs &a, i32 lo, double wgt, u32 w)
{
    const i32 L = a.gg_L, hi = lo + 1 < a.gg_n ? lo + 1 : a.gg_n - 1;
    const double samples = ((double)w + 0.5) * (1.0 / 4294967296.0) * (double)(L - 2);
    const double fl = floor(samples); const i32 i0 = (i32)fl, i1 = (i32)ceil(samples);
    const double *A = a.gg_inv + (i64)lo * L, *B = a.gg_inv + (i64)hi * L;
    const double t1 = (B[i0] - A[i0]) * wgt + A[i0], t2 = (B[i1] - A[i1]) * wgt + A[i1];
    return (t2 - t1) * (samples - fl) + t1;
}
// mean excitation time of an instruction's photons (fixed point sum -> independent of the order of summation)
__device__ __forceinline__ double gg_mean(const GenArgs &a, i32 ins)
{
    const i64 n = a.ins_ph0[ins + 1] - a.ins_ph0[ins];
    return n > 0 ? (double)a.ins_ggsum[ins] / (double)n / 1048576.0 : 0.0;
}

// Poisson: PTRS (Hoermann 1993) for lam >= 10, multiplication method below; same algorithm and uniforms as the oracle
__device__ i64 poisson_draw(const WfsDev &d, u32 emitter, u32 gid, double lam)
{
    u32 it = 0;
    if (lam <= 0) return 0;
    if (lam < 10) {
        double enlam = exp(-lam), prod = 1.0; i64 x = 0;
        for (;;) {
            u32x4 w = philox4x32_10(emitter, gid, it++, SITE_EL_POIS, d.k0, d.k1);
            prod *= u53(w.x, w.y);
            if (prod > enlam) x++; else return x;
            prod *= u53(w.z, w.w);
            if (prod > enlam) x++; else return x;
        }
    }
    double slam = sqrt(lam), loglam = log(lam);
    double b = 0.931 + 2.53 * slam, aa = -0.059 + 0.02483 * b;
    double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2);
    for (;;) {
        u32x4 w = philox4x32_10(emitter, gid, it++, SITE_EL_POIS, d.k0, d.k1);
        double U = u53(w.x, w.y) - 0.5, V = u53(w.z, w.w);
        double us = 0.5 - fabs(U);
        i64 k = (i64)floor((2 * aa / us + b) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) return k;
        if (k < 0 || (us < 0.013 && V > us)) continue;
        if (log(V) + log(invalpha) - log(aa / (us * us) + b) <= -lam + k * loglam - lgamma((double)k + 1)) return k;
    }
}

// S1: n_hits = Binomial(amp, ly) as a sum of Bernoulli trials (s1.py:133), one wave per instruction
__global__ __launch_bounds__(256) void k_s1_hits(WfsDev d, GenArgs a)
{
    const int lane = threadIdx.x & 63;
    i64 i = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.n_ins || a.ins_type[i] != 1) return;
    const u64 T = bern_threshold(a.ins_p[i]);
    const i64 amp = a.ins_amp[i]; const u32 gid = a.ins_gid[i];
    i32 hits = 0;
    for (i64 q = lane; q * 4 < amp; q += 64) {
        u32x4 w = philox4x32_10(0, gid, (u32)q, SITE_S1_HIT, d.k0, d.k1);
        i64 j = q * 4;
        hits += (u64)w.x < T;
        if (j + 1 < amp) hits += (u64)w.y < T;
        if (j + 2 < amp) hits += (u64)w.z < T;
        if (j + 3 < amp) hits += (u64)w.w < T;
    }
    for (int o = 32; o > 0; o >>= 1) hits += __shfl_down(hits, o, 64);
    if (lane == 0) { i64 e = a.em_off[i]; a.em_nph[e] = hits; a.em_time[e] = a.ins_time[i]; a.em_ins[e] = (i32)i; }
}

// Photons per electron, Poisson(sc_gain) (s2.py:308).  The secondary gain is a property of the INSTRUCTION, so its Poisson
// distribution is tabulated once per instruction -- pmf(k) = exp(k ln(lam) - lam - lgamma(k + 1)) on the 256 values from
// floor(lam - 8 sqrt(lam)) - 4 on (what lies outside is below 1e-15), summed in order, normalised -- and an electron inverts it with
// ONE uniform (bisection, 8 steps).  numpy's PTRS rejection loop with its logs and lgamma per trial cost 2000 VALU instructions per
// electron (every wave takes the slow path and the longest loop of its 64 lanes) and 198 VGPRs; it is kept, in a kernel of its own,
// for gains above POIS_LAM_MAX.  Same distribution (tests: KS against np.random.poisson draws of the reference).
#define POIS_W 256
#define POIS_LAM_MAX 217.0
__global__ __launch_bounds__(POIS_W) void k_poisson_tables(GenArgs a, double *cdf, i32 *kmin)
{
    __shared__ double p[POIS_W];
    const i64 i = blockIdx.x; const int t = threadIdx.x;
    const double lam = a.ins_sc[i];
    if (a.ins_type[i] == 1 || !(lam > 0) || lam > POIS_LAM_MAX) { if (t == 0) kmin[i] = (a.ins_type[i] != 1 && !(lam > 0)) ? -2 : -1; return; }
    i64 k0 = (i64)floor(lam - 8.0 * sqrt(lam)) - 4; if (k0 < 0) k0 = 0;
    const double k = (double)(k0 + t);
    p[t] = exp(k * log(lam) - lam - lgamma(k + 1.0));
    __syncthreads();
    if (t == 0) { double run = 0; for (int j = 0; j < POIS_W; j++) { run += p[j]; p[j] = run; } kmin[i] = (i32)k0; }
    __syncthreads();
    cdf[i * POIS_W + t] = p[t] / p[POIS_W - 1];
}
__device__ __forceinline__ i64 poisson_table_draw(const WfsDev &d, const double *cdf, i32 kmin, u32 emitter, u32 gid)
{
    const u32x4 w = philox4x32_10(emitter, gid, 0, SITE_EL_POIS, d.k0, d.k1);
    const double u = u53(w.x, w.y);
    int lo = 0, hi = POIS_W - 1;                         // first j with u < cdf[j] (cdf[POIS_W - 1] == 1)
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (u < cdf[mid]) hi = mid; else lo = mid + 1; }
    return (i64)kmin + lo;
}

// S2: one thread per candidate electron (s2.py:254, 258-286, 308-310)
// instruction of the first emitter of every 256-emitter block of k_s2_electrons (+ a sentinel: the last instruction)
__global__ void k_emitter_blocks(GenArgs a, i64 n_blocks)
{
    const i64 b = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > n_blocks) return;
    if (b == n_blocks) { a.eblk_ins[b] = (i32)(a.n_ins - 1); return; }
    const i64 e = b * 256;
    i64 lo = 0, hi = a.n_ins;
    while (hi - lo > 1) { i64 mid = (lo + hi) >> 1; if (a.em_off[mid] <= e) lo = mid; else hi = mid; }
    a.eblk_ins[b] = (i32)lo;
}

__global__ __launch_bounds__(256) void k_s2_electrons(WfsDev d, GenArgs a)
{
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    i64 i = -1; bool is_s2 = false;
    // instruction of emitter e: em_off[i] <= e < em_off[i+1].  The instruction of every block's first emitter comes from
    // k_emitter_blocks (all those searches in flight at once); inside the block the search runs over what is left,
    // usually nothing (10^4 candidate electrons per S2).
    if (e < a.n_emitters) {
        i64 lo = a.eblk_ins[blockIdx.x], hi = a.eblk_ins[blockIdx.x + 1] + 1;
        while (hi - lo > 1) { i64 mid = (lo + hi) >> 1; if (a.em_off[mid] <= e) lo = mid; else hi = mid; }
        i = lo; is_s2 = a.ins_type[i] != 1;          // types 2, 4, 6 are S2-like (electrons drifting to the gas gap)
    }
    double st_n = 0, st_t = 0, st_t2 = 0; i64 st_min = I64_MAX, st_max = I64_MIN;
    if (is_s2) {
        const u32 j0 = (u32)(e - a.em_off[i]), jb = a.ins_embase[i], j = jb + j0; const u32 gid = a.ins_gid[i];
        a.em_ins[e] = (i32)i;
        u32x4 sv = philox4x32_10(jb, gid, j0 >> 2, SITE_S2_SURVIVE, d.k0, d.k1);
        u32 word = (j0 & 3) == 0 ? sv.x : (j0 & 3) == 1 ? sv.y : (j0 & 3) == 2 ? sv.z : sv.w;
        if (!((u64)word < bern_threshold(a.ins_p[i]))) { a.em_nph[e] = 0; a.em_time[e] = I64_MIN; }
        else {
            u32x4 A = philox4x32_10(j, gid, 0, SITE_EL_A, d.k0, d.k1);
            u32x4 B = philox4x32_10(j, gid, 0, SITE_EL_B, d.k0, d.k1);
            double z_drift, z_gain;
            box_muller(B, z_drift, z_gain);
            double timing = -log(1.0 - u53(A.x, A.y)) * d.trap_time;
            timing += a.ins_dm[i] + a.ins_ds[i] * z_drift;
            i64 et = a.ins_time[i] + (i64)timing;                         // s2.py:282
            a.em_time[e] = et;
            const i32 pk = a.pois_kmin[i];
            if (a.ins_fused && a.ins_fused[i]) a.em_nph[e] = 0;                // its photons are made tile by tile (wfs_tilegen.h)
            else if (pk == -1) a.em_zg[e] = z_gain;                             // gain above POIS_LAM_MAX: k_s2_photons (PTRS)
            else {
                i64 nph = pk >= 0 ? poisson_table_draw(d, a.pois_cdf + i * POIS_W, pk, j, gid) : 0;
                nph += (i64)(0.0 + d.gain_spread * z_gain);               // s2.py:309
                if (nph < 0) nph = 0;
                a.em_nph[e] = (i32)nph;
            }
            double tr = (double)(et - a.ins_time[i]);
            st_n = 1; st_t = tr; st_t2 = tr * tr; st_min = et; st_max = et;
        }
    }
    // electron time statistics of the truth row (rawdata.py:325-332): one set of atomics per wave when the
    // whole wave works on one instruction, else one per lane
    const i64 i_first = __shfl(i, 0, 64);
    bool leader = true;
    if (all64(i == i_first)) {
        for (int o = 32; o > 0; o >>= 1) {
            st_n += __shfl_down(st_n, o, 64); st_t += __shfl_down(st_t, o, 64); st_t2 += __shfl_down(st_t2, o, 64);
            i64 mn = __shfl_down(st_min, o, 64), mx = __shfl_down(st_max, o, 64);
            st_min = mn < st_min ? mn : st_min; st_max = mx > st_max ? mx : st_max;
        }
        leader = (threadIdx.x & 63) == 0;
    }
    if (leader && st_n > 0) {
        atomicAdd(&a.el_stat[i * 4 + 0], st_n); atomicAdd(&a.el_stat[i * 4 + 1], st_t); atomicAdd(&a.el_stat[i * 4 + 2], st_t2);
        atomicMin(&a.el_minmax[i * 2], st_min); atomicMax(&a.el_minmax[i * 2 + 1], st_max);
    }
}

// photons of the surviving electrons of instructions with a gain above POIS_LAM_MAX: numpy's PTRS + int(N(0, gain_spread)) (s2.py:308-310)
__global__ __launch_bounds__(256) void k_s2_photons(WfsDev d, GenArgs a)
{
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n_emitters) return;
    if (a.em_time[e] == I64_MIN) return;                     // did not survive (em_nph = 0 already); S1 emitters are not touched: em_zg is NaN
    const double zg = a.em_zg[e];
    if (!(zg == zg)) return;
    const i32 i = a.em_ins[e];
    const u32 j = a.ins_embase[i] + (u32)(e - a.em_off[i]);
    i64 nph = poisson_draw(d, j, a.ins_gid[i], a.ins_sc[i]);
    nph += (i64)(0.0 + d.gain_spread * zg);                  // s2.py:309
    if (nph < 0) nph = 0;
    a.em_nph[e] = (i32)nph;
}

__device__ __forceinline__ int channel_from_cdf(const double *cdf, int n, double u)
{
    int lo = 0, hi = n;                             // searchsorted(cdf, u, side='right')
    while (lo < hi) { int mid = (lo + hi) >> 1; if (u < cdf[mid]) hi = mid; else lo = mid + 1; }
    return lo < n ? lo : n - 1;
}

// (GEN_LOG, GEN_BLOCK photons per block of the generator, GEN_WIN emitter offsets staged in LDS per block: wfs_layout.h)

// Guide of a non-decreasing CDF row: cell j = int(u * scale), clamped to AP_GUIDE - 1, holds a bracket [lo, hi] of "the first entry >= u"
// for every u of the cell (built on the host from the row itself with a margin on either side of the cell, wfs_set_ap_element): the
// bisection of argmin_abs_diff starts from two entries instead of the row -- ~8 dependent, divergent loads per search fewer.
#define AP_GUIDE 256
struct ApGuide { double scale; unsigned short lo[AP_GUIDE], hi[AP_GUIDE]; };

// PMT afterpulse element tables (afterpulse.py:181-186) and the staging list of generated afterpulse photons
struct ApElemDev { i32 n_bins_delay, n_bins_amp, amp_2d, is_uniform; double delay_bin, amp_bin; const double *delay_cdf, *amp_cdf;
                   i32 delay_sorted, amp_sorted;        // the rows are non-decreasing (checked on the host): argmin by bisection
                   const ApGuide *delay_guide, *amp_guide; };     // per row of the two tables (or nullptr): where the bisection starts

// np.argmin(|cdf - u|) (afterpulse.py:222, 229): the FIRST index of the smallest distance.  On a non-decreasing row the
// distance falls up to the first entry >= u and rises behind it, so the answer is that entry or the one in front of it
// (lower index on a tie), moved to the start of its plateau of equal values -- two bisections instead of a scan of the row
// (a scan costs every wave that holds one accepted photon ~n_bins iterations: 20 of 23 ms of the fill pass with
// afterpulses on).  Rows that are not sorted (never seen; the host checks) keep the scan.
__device__ __forceinline__ int argmin_abs_diff(const double *c, int n, double u, bool sorted, const ApGuide *guide = nullptr)
{
    if (!sorted) {
        int best = 0; double bd = fabs(c[0] - u);
        for (int k = 1; k < n; k++) { const double dd = fabs(c[k] - u); if (dd < bd) { bd = dd; best = k; } }
        return best;
    }
    int lo = 0, hi = n;                                  // first k with c[k] >= u (n: none)
    if (guide && u >= 0.0) {
        const double x = u * guide->scale;
        const int j = x < (double)(AP_GUIDE - 1) ? (int)x : AP_GUIDE - 1;
        lo = guide->lo[j]; hi = guide->hi[j];
    }
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (c[mid] >= u) hi = mid; else lo = mid + 1; }
    int best = lo;
    if (lo == n) best = n - 1;
    else if (lo > 0 && !(fabs(c[lo] - u) < fabs(c[lo - 1] - u))) best = lo - 1;
    const double v = c[best];
    if (best == 0 || c[best - 1] < v) return best;       // (no plateau in front of it: the usual case, one load instead of a second bisection)
    int a = 0, b = best;                                 // first k with c[k] == v: first k with c[k] >= v
    while (a < b) { const int mid = (a + b) >> 1; if (c[mid] >= v) b = mid; else a = mid + 1; }
    return a;
}
struct ApArgs {
    i32 n; i32 pad;
    ApElemDev el[WFS_MAX_AP];
    const double *prob[WFS_MAX_AP]; // [n_tpc] per element: afterpulse probability of every channel (last entry of its delay CDF row), contiguous
    const u32 *thr[WFS_MAX_AP];     // [n_tpc][2] per element: screening thresholds (single / double photoelectron parent), ap_threshold
    i64 cap;                        // capacity of the staging list
    i32 *ap_ins; i32 *ap_ch; i32 *ap_t; double *ap_gain;     // [cap] instruction, channel, ns relative to the instruction, gain
    u32 *ap_key;                    // [cap] order key: element << 29 | index of the parent photon among its instruction's photons
    i64 *count;                     // number of afterpulse candidates in the list (device scalar, WfsScal::n_ap_candidates)
    struct ApSeg *seg; i64 n_seg;   // candidates of a k_s2_tile workgroup: one contiguous, key-ordered stretch of the list per tile (k_ap_seg)
    struct ApCand *cand;            // [cap] candidates of the generator (k_ap_finish turns entry i into afterpulse photon i, or a hole: ap_ch[i] = -1)
};
// (AP_STAGE afterpulse candidates a block parks in LDS: wfs_layout.h)

// first and last emitter of every photon block: one bisection per thread, all in flight together (a block doing
// its own two bisections serially costs ~20 us of dependent HBM latency before its 2048 photons can start)
__global__ void k_block_emitters(GenArgs a)
{
    const i64 b = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.n_blocks) return;
    const i64 p0 = b * GEN_BLOCK;
    const i64 p1 = (p0 + GEN_BLOCK < a.n_photons) ? p0 + GEN_BLOCK : a.n_photons;
    for (int w = 0; w < 2; w++) {
        const i64 p = w == 0 ? p0 : p1 - 1;
        i64 lo = 0, hi = a.n_emitters;
        while (hi - lo > 1) { i64 mid = (lo + hi) >> 1; if (a.em_ph_off[mid] <= p) lo = mid; else hi = mid; }
        a.blk_e[2 * b + w] = lo;
    }
    // the fast path of the generator needs all photons of the block in one instruction and the block's emitters in its LDS window
    const i64 e_lo = a.blk_e[2 * b], e_hi = a.blk_e[2 * b + 1];
    const i32 i0 = a.em_ins[e_lo];
    const bool single = e_hi - e_lo + 2 <= GEN_WIN && i0 == a.em_ins[e_hi];
    a.blk_ins[b] = single ? i0 : -1;
    if (!single && i0 == a.em_ins[e_hi] && a.ins_ph0[i0] < p0 && a.ins_ph0[i0 + 1] > p1) a.ins_fullsort[i0] = 1;      // generic block inside one instruction
    BlockDesc bd{};
    bd.ins = -1;
    if (single) {
        bd.ins = i0; bd.e_lo = e_lo; bd.nwin = (i32)(e_hi - e_lo + 2); bd.set = a.ins_set[i0]; bd.itime = a.set_t0[bd.set];
        bd.R0 = p0 - a.ins_ph0[i0]; bd.row = a.ins_cdfrow[i0]; bd.gid = a.ins_gid[i0]; bd.eb = a.ins_embase[i0];
        bd.jbase = (u32)(e_lo - a.em_off[i0]) + bd.eb; bd.is_s2 = a.ins_type[i0] != 1; bd.sbase = a.ins_sbase[i0];
        bd.multi = 0;      // (whether the tile is sorted as a whole is only known when every block has been looked at: ins_fullsort, read by the fill pass)
    }
    a.blk_desc[b] = bd;
}

__global__ void k_ins_ph0(GenArgs a)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= a.n_ins) a.ins_ph0[i] = a.em_ph_off[a.em_off[i]];
}
// order keys run through a pulse set instruction by instruction (the reference appends the photons of a Pulse call's instructions
// in that order, s1.py:95-103 / s2.py:107-136): photons in front of every instruction inside its set
__global__ void k_set_bases(GenArgs a)
{
    const i64 s = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n_psets) return;
    i64 run = 0;
    for (i64 q = a.set_ins_off[s]; q < a.set_ins_off[s + 1]; q++) {
        const i32 i = a.set_ins_list[q];
        if (run > 0xffffffffLL) atomicMax(&a.scal->error, (i64)WFS_DEV_TIME_RANGE);
        a.ins_sbase[i] = (u32)run;
        a.ins_fullsort[i] = a.set_ins_off[s + 1] - a.set_ins_off[s] > 1;       // (k_block_emitters adds the instructions with a generic block in their middle)
        run += a.em_ph_off[a.em_off[i + 1]] - a.em_ph_off[a.em_off[i]];
    }
}

// PMT afterpulses of one photon (afterpulse.py:172-249): one uniform pair per element.  RNG spec v10: the top 32 bits of the FIRST
// uniform of elements 4k .. 4k + 3 are the four words of one call (site SITE_AP_SCREEN + k); its low bits and the second uniform come
// from the element's own call (SITE_AP + e: words y, z, w), which only a candidate ever makes.  The generator only SCREENS
// (ap_generate, inside the photon loop): one Philox call per four elements and an integer comparison of the screen word with a
// threshold of the (element, channel) that no accepted uniform can miss (ap_threshold in wfs_engine.hip); the rare candidate is
// parked in LDS and leaves with the block's other candidates for the global list.  k_ap_finish, one thread per candidate, makes
// the reference's own floating-point comparison and turns the accepted ones into afterpulse photons (two bisections of cumulative
// rows in global memory, ~20 dependent loads).  Inside the photon loop a wave paid that chain whenever ONE of its 64 lanes had a
// candidate, which with p ~ 1 % per element is most of the time; behind the loop, once per block, it still kept the block's LDS
// and its eight mostly idle waves on the CU for tens of microseconds (fill pass 5.1 -> 2.7 ms -> see DESIGN.md for the last step).
struct __attribute__((aligned(8))) ApCand { i64 itime; u32 x; i32 ins, ch, t; u32 key, j, m, gid; i32 e_dpe, pad; };     // (48 bytes)
static_assert(sizeof(ApCand) == AP_CAND_BYTES, "the layouts size the afterpulse stage by it");
struct ApStage { i32 *n; ApCand *cand; };
struct ApSeg { i64 base; i32 n, tile; };     // list entries [base, base + n) belong to afterpulse tile `tile`
#define AP_SEG_MARK (1 << 30)                // in ApCand.ins / ap_ins: the entry belongs to a segment (k_ap_seg places it, k_ap_count / k_ap_place skip it)
// the uniform of the acceptance test, exactly as the reference forms and scales it (afterpulse.py:196-204); w: the element's own call
__device__ __forceinline__ double ap_uniform(const WfsDev &d, const ApCand &q, const u32x4 &w)
{
    double rU0 = 1.0 - u53(q.x, w.y);
    rU0 /= d.pmt_ap_modifier;
    if (q.e_dpe >> 8) rU0 /= 2;
    return rU0;
}
__device__ __forceinline__ u32x4 ap_call(const WfsDev &d, const ApCand &q) { return philox4x32_10(q.j, q.gid, q.m, SITE_AP + (u32)(q.e_dpe & 0xff), d.k0, d.k1); }
__device__ __forceinline__ bool ap_accept(const WfsDev &d, const ApArgs &ap, const ApCand &q, const u32x4 &w) { return ap_uniform(d, q, w) <= ap.prob[q.e_dpe & 0xff][q.ch]; }
__device__ __forceinline__ void ap_finish(const WfsDev &d, WfsScal *scal, const ApArgs &ap, const ApCand &q, const u32x4 &w, i64 gk)
{
    const int e = q.e_dpe & 0xff;
    const ApElemDev &el = ap.el[e];
    const double *dc = el.delay_cdf + (size_t)q.ch * el.n_bins_delay;
    double delay, amp;
    if (el.is_uniform) {
        const u32x4 x = philox4x32_10(q.j, q.gid, q.m, SITE_AP_X + (u32)e, d.k0, d.k1);
        delay = (dc[0] + (dc[1] - dc[0]) * u53(x.x, x.y)) * el.delay_bin; amp = 1.0;
    } else {
        const int best = argmin_abs_diff(dc, el.n_bins_delay, ap_uniform(d, q, w), el.delay_sorted != 0, el.delay_guide ? el.delay_guide + q.ch : nullptr);      // np.argmin(|cdf - u|): first minimum
        delay = best * el.delay_bin - d.pmt_ap_t_modifier;
        const double *ac = el.amp_2d ? el.amp_cdf + (size_t)q.ch * el.n_bins_amp : el.amp_cdf;
        const int ba = argmin_abs_diff(ac, el.n_bins_amp, 1.0 - u53(w.z, w.w), el.amp_sorted != 0, el.amp_guide ? el.amp_guide + (el.amp_2d ? q.ch : 0) : nullptr);
        amp = ba * el.amp_bin;
    }
    const double tf = (double)(q.itime + q.t) + delay;          // afterpulse.py:235, int64 + float
    i64 tap = (i64)tf - q.itime;
    if (tap > 0x7fffffffLL || tap < -0x7fffffffLL) { atomicMax(&scal->error, (i64)WFS_DEV_TIME_RANGE); tap = 0; }
    if (gk < ap.cap) { ap.ap_ins[gk] = q.ins; ap.ap_ch[gk] = q.ch; ap.ap_t[gk] = (i32)tap; ap.ap_gain[gk] = d.gains[q.ch] * amp; ap.ap_key[gk] = q.key; }
}
// a candidate into the block's LDS list (or, past AP_STAGE, straight to the end)
__device__ __forceinline__ void ap_park(const ApArgs &ap, const ApStage &st, u32 x, i32 e_dpe, u32 j, u32 gid, u32 m,
                                     i32 ins, i32 ch, i64 itime, i32 t, u32 key, bool seg = false)
{
    ApCand q;
    q.x = x; q.itime = itime; q.ins = ins; q.ch = ch; q.t = t; q.j = j; q.m = m; q.gid = gid; q.e_dpe = e_dpe; q.pad = 0;
    q.key = key;                                                    // element << 29 | parent: the reference walks element by element, parent by parent (afterpulse.py:189-207)
    const i32 kq = atomicAdd(st.n, 1);
    if (kq < AP_STAGE) { if (seg) q.ins |= AP_SEG_MARK; st.cand[kq] = q; }
    else { const i64 gk = (i64)atomicAdd((u64 *)ap.count, 1ull); if (gk < ap.cap) ap.cand[gk] = q; }      // (a block with more candidates than the stage holds)
}
// the screen word of element e of a photon, recomputed for a candidate (tile_ap_screen in wfs_tilegen.h screens eight photons in registers)
__device__ __forceinline__ u32 ap_screen_word(const WfsDev &d, u32 j, u32 gid, u32 m, int e)
{
    return word_of(philox4x32_10(j, gid, m, SITE_AP_SCREEN + (u32)(e >> 2), d.k0, d.k1), e & 3);
}
__device__ __forceinline__ void ap_generate(const WfsDev &d, const ApArgs &ap, const ApStage &st,
                                            u32 j, u32 gid, u32 m, i32 ins, int ch, bool is_dpe, i64 itime, i64 t, u32 P)
{
    for (int e0 = 0; e0 < ap.n; e0 += 4) {
        const u32x4 S = philox4x32_10(j, gid, m, SITE_AP_SCREEN + (u32)(e0 >> 2), d.k0, d.k1);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int e = e0 + k;
            if (e >= ap.n) break;
            const u32 x = word_of(S, k);
            const u32 thr = ap.thr[e][ch * 2 + (is_dpe ? 1 : 0)];
            if ((x >> 5) < thr) continue;                           // surely rejected (ap_threshold)
            ap_park(ap, st, x, e | (is_dpe ? 256 : 0), j, gid, m, ins, ch, itime, (i32)t, ((u32)e << 29) | (P & 0x1fffffffu));
        }
    }
}

// Photon generator, two passes over the same photon index space (GEN_BLOCK consecutive photons per block, generation
// order = emitter by emitter).  RNG spec v6: photon P of an instruction (P = its index among the
// instruction's photons) owns word P & 3 of three calls (em_base, gid, P >> 2, site): SITE_CH -> channel (s1.py:154-158 /
// s2.py:673-677), SITE_DELAY -> summed delay (alias table; s1.py:180-194 / s2.py:504-557, pulse.py:53-56), SITE_GAIN ->
// SPE indices and double-PE flag (pulse.py:76-103).  A thread that takes four consecutive photons spends 0.75 Philox
// calls per photon (the generator is bound by VALU issue: 20 quarter-rate multiplies per call).
// Count pass (k_photon_count): channel words only -> photons per (block, channel); no per-photon intermediate is left in
//   HBM (the first version wrote a packed word per photon and read it back: 5.8 GB per 10^9-PE batch).
// k_block_ranges: where in its tile every block puts its photons (consecutive blocks, consecutive ranges).
// Fill pass (k_photon_fill): all three calls per quad in generation order; every photon is ranked inside its channel with
//   LDS counters and staged at its bucket position in LDS; the block then stores in BUCKET order: neighbouring lanes write
//   photons of the same tile to consecutive addresses (a scattered 8-byte store per lane is bound by the L2 request rate).
// Fast path ("single": all photons of the block belong to one instruction, the normal case for an S2): emitter window,
//   the channel alias table (channel_lookup) and the tile offsets of the block live in LDS.
// Generic path (a block spanning instructions: S1s, small S2s): per-photon global lookups and atomics.

// exclusive prefix sum over n <= 4 * TPB LDS integers, in place; v[n] receives the total.  All TPB threads call it.
template <int TPB>
__device__ __forceinline__ void block_excl_scan(i32 *v, int n, i32 *wtmp)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int per = (n + TPB - 1) / TPB, b = tid * per;
    i32 loc[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { loc[k] = (k < per && b + k < n) ? v[b + k] : 0; s += loc[k]; }
    i32 x = s;
    for (int o = 1; o < 64; o <<= 1) { const i32 y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
    if (lane == 63) wtmp[wid] = x;
    __syncthreads();
    i32 run = x - s;
    for (int w = 0; w < wid; w++) run += wtmp[w];
#pragma unroll
    for (int k = 0; k < 4; k++) if (k < per && b + k < n) { v[b + k] = run; run += loc[k]; }
    if (tid == TPB - 1) v[n] = run;
    __syncthreads();
}

// ---- pattern maps on the device (S1.photon_channels s1.py:138-159, S2.photon_channels s2.py:616-682; the maps are
// straxen.InterpolatingMap objects built by load_resource.make_patternmap, method WeightedNearestNeighbors): the hit
// pattern at a position is the inverse-distance weighted average of the 2 * dims nearest grid nodes (distance clipped at
// 1e-6).  On the host that costs ~0.4 ms per instruction (10^4 S1: seconds); here one thread finds the neighbours of
// an instruction and one workgroup turns them into the instruction's channel CDF row.
#define MAP_K 6                    // 2 * dims neighbours, dims <= 3
struct MapArgs {
    i32 dims, n[3], w[3];          // regular grid: nodes per axis; half-width of the candidate block per axis
    double lo[3], h[3];            // first node and spacing per axis
    i64 n_points; const double *points;    // point-list map (an irregular coordinate system): [n_points][dims]; else nullptr
    // 2-D point lists: a uniform cell index over the points (cell (i, j) = cell_start[i * cny + j] .. of cell_pts, ascending point index)
    const i32 *cell_start, *cell_pts; i32 cnx, cny; double cell_lo[2], cell_h;
    const float *values;           // [nodes][n_map_ch]
    i32 n_map_ch;                  // channels stored in the map; channels beyond get weight 1 (s2.py:648-650: top-only maps)
    i64 n_rows;                    // positions to evaluate
    const i32 *row_ins;            // [n_rows] instruction of the row (pattern rows)
    const float *x, *y, *z;        // [n_ins] positions of the instructions (pattern rows)
    const double *pos;             // or: [n_rows][dims] positions (scalar maps)
    const i64 *row_id;             // [n_rows] cdf row to write
    i64 *nb_idx; double *nb_w;     // [n_rows][MAP_K]
    double *cdf_table;
    const double *gains;           // [n_tpc] 0: turned-off PMT
    const double *aft;             // [n_ins] s2_aft_sigma: factor on the top-array fraction of the instruction's pattern, or nullptr
    i32 n_top;
    const double *pre;             // [n_rows][n_map_ch] patterns already averaged (k_diffuse_patterns) instead of neighbour lists, or nullptr
};

__device__ __forceinline__ void map_position(const MapArgs &m, i64 r, double pos[3])
{
    if (m.pos) { for (int a = 0; a < 3; a++) pos[a] = a < m.dims ? m.pos[r * m.dims + a] : 0.0; return; }
    const i32 ins = m.row_ins[r];
    pos[0] = (double)m.x[ins]; pos[1] = (double)m.y[ins]; pos[2] = m.dims > 2 ? (double)m.z[ins] : 0.0;
}

__device__ __forceinline__ void map_store_neighbours(const MapArgs &m, i64 r, int K, const double *bd, const i64 *bi)
{
    for (int k = 0; k < MAP_K; k++) {
        const double dist = k < K ? sqrt(bd[k]) : 0.0;
        m.nb_idx[r * MAP_K + k] = k < K ? bi[k] : -1;
        m.nb_w[r * MAP_K + k] = (k < K && bi[k] >= 0) ? 1.0 / (dist < 1e-6 ? 1e-6 : dist) : 0.0;
    }
}

// the K = 2 * dims nearest nodes of a regular grid (squared distances ascending in bd, node indices in bi)
__device__ __forceinline__ void grid_nearest(const MapArgs &m, const double *pos, double *bd, i64 *bi)
{
    i32 c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
    for (int a = 0; a < m.dims; a++) {
        i32 c = (i32)floor((pos[a] - m.lo[a]) / m.h[a]);
        c = c < 0 ? 0 : (c > m.n[a] - 2 ? m.n[a] - 2 : c);
        c0[a] = c - m.w[a] + 1 < 0 ? 0 : c - m.w[a] + 1;
        c1[a] = c + m.w[a] > m.n[a] - 1 ? m.n[a] - 1 : c + m.w[a];
    }
    const int K = 2 * m.dims;
    for (int k = 0; k < MAP_K; k++) { bd[k] = 1e300; bi[k] = -1; }
    for (i32 i = c0[0]; i <= c1[0]; i++) {
        const double dx = pos[0] - (m.lo[0] + i * m.h[0]);
        for (i32 j = c0[1]; j <= c1[1]; j++) {
            const double dy = m.dims > 1 ? pos[1] - (m.lo[1] + j * m.h[1]) : 0.0;
            for (i32 l = c0[2]; l <= c1[2]; l++) {
                const double dz = m.dims > 2 ? pos[2] - (m.lo[2] + l * m.h[2]) : 0.0;
                const double d2 = dx * dx + dy * dy + dz * dz;
                if (!(d2 < bd[K - 1])) continue;            // ties keep the node met first (lower linear index)
                const i64 node = ((i64)i * (m.dims > 1 ? m.n[1] : 1) + j) * (m.dims > 2 ? m.n[2] : 1) + l;
                int q = K - 1;
                while (q > 0 && d2 < bd[q - 1]) { bd[q] = bd[q - 1]; bi[q] = bi[q - 1]; q--; }
                bd[q] = d2; bi[q] = node;
            }
        }
    }
}

// The same for a 2-D point list, through the cell index: rings of cells around the position's cell until the K-th neighbour found is
// closer than anything in the rings not yet visited can be (a cell at Chebyshev distance k lies at least (k - 1) cell widths away);
// equal distances: the lower point index, as the brute-force search of k_map_neighbours_points.
__device__ __forceinline__ void points_nearest_2d(const MapArgs &m, const double *pos, double *bd, i64 *bi)
{
    constexpr int K = 4;
    for (int k = 0; k < MAP_K; k++) { bd[k] = 1e300; bi[k] = -1; }
    i32 cx = (i32)floor((pos[0] - m.cell_lo[0]) / m.cell_h), cy = (i32)floor((pos[1] - m.cell_lo[1]) / m.cell_h);
    cx = cx < 0 ? 0 : (cx > m.cnx - 1 ? m.cnx - 1 : cx); cy = cy < 0 ? 0 : (cy > m.cny - 1 ? m.cny - 1 : cy);
    const i32 rmax = m.cnx > m.cny ? m.cnx : m.cny;
    for (i32 r = 0; r <= rmax; r++) {
        for (i32 i = cx - r; i <= cx + r; i++) {
            if (i < 0 || i >= m.cnx) continue;
            const bool whole = i == cx - r || i == cx + r;          // the ring's two full columns; in between only its top and bottom cell
            for (i32 j = cy - r; j <= cy + r; j += (whole || r == 0) ? 1 : 2 * r) {
                if (j < 0 || j >= m.cny) continue;
                const i64 cell = (i64)i * m.cny + j;
                for (i32 q = m.cell_start[cell]; q < m.cell_start[cell + 1]; q++) {
                    const i64 p = m.cell_pts[q];
                    const double dx = pos[0] - m.points[2 * p], dy = pos[1] - m.points[2 * p + 1];
                    const double d2 = dx * dx + dy * dy;
                    if (!(d2 < bd[K - 1] || (d2 == bd[K - 1] && p < bi[K - 1]))) continue;
                    int t = K - 1;
                    while (t > 0 && (d2 < bd[t - 1] || (d2 == bd[t - 1] && p < bi[t - 1]))) { bd[t] = bd[t - 1]; bi[t] = bi[t - 1]; t--; }
                    bd[t] = d2; bi[t] = p;
                }
            }
        }
        const double reach = (double)r * m.cell_h;
        if (bi[K - 1] >= 0 && bd[K - 1] < reach * reach) break;
    }
}

__global__ void k_map_neighbours(MapArgs m)
{
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m.n_rows) return;
    double pos[3]; map_position(m, r, pos);
    double bd[MAP_K]; i64 bi[MAP_K];
    grid_nearest(m, pos, bd, bi);
    map_store_neighbours(m, r, 2 * m.dims, bd, bi);
}

// point-list maps (straxen.InterpolatingMap on an irregular coordinate system: a KD-tree query for the 2 * dims nearest
// points): one wave per position, every lane scans a stride of the points keeping its own K best, then K rounds of a
// wave-wide argmin merge the 64 lists (ties: the lower point index).
__global__ __launch_bounds__(256) void k_map_neighbours_points(MapArgs m)
{
    const i64 r = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= m.n_rows) return;                              // the whole wave leaves
    double pos[3]; map_position(m, r, pos);
    const int K = 2 * m.dims;
    double bd[MAP_K]; i64 bi[MAP_K];
#pragma unroll
    for (int k = 0; k < MAP_K; k++) { bd[k] = 1e300; bi[k] = 0x7fffffffffffffffLL; }
    for (i64 q = lane; q < m.n_points; q += 64) {
        double d2 = 0;
        for (int a = 0; a < m.dims; a++) { const double d = pos[a] - m.points[q * m.dims + a]; d2 += d * d; }
        if (!(d2 < bd[MAP_K - 1])) continue;
        // insertion into the sorted list of MAP_K (only the first K are used); fixed trip counts keep the lists in registers
        bool placed = false; double cd = d2; i64 ci = q;
#pragma unroll
        for (int k = 0; k < MAP_K; k++) {
            if (placed || cd < bd[k]) { const double td = bd[k]; const i64 ti = bi[k]; bd[k] = cd; bi[k] = ci; cd = td; ci = ti; placed = true; }
        }
    }
    double od[MAP_K]; i64 oi[MAP_K];
    for (int k = 0; k < MAP_K; k++) {
        double d = bd[0]; i64 i = bi[0];
        for (int o = 32; o > 0; o >>= 1) {
            const double xd = __shfl_xor(d, o, 64); const i64 xi = __shfl_xor(i, o, 64);
            if (xd < d || (xd == d && xi < i)) { d = xd; i = xi; }
        }
        if (bi[0] == i && i != 0x7fffffffffffffffLL) {     // the winner pops its head
#pragma unroll
            for (int q = 0; q < MAP_K - 1; q++) { bd[q] = bd[q + 1]; bi[q] = bi[q + 1]; }
            bd[MAP_K - 1] = 1e300; bi[MAP_K - 1] = 0x7fffffffffffffffLL;
        }
        od[k] = d; oi[k] = i == 0x7fffffffffffffffLL ? -1 : i;
    }
    if (lane == 0) map_store_neighbours(m, r, K, od, oi);
}

// Transverse diffusion with field maps (S2.s2_pattern_map_diffuse, s2.py:560-613): the pattern of an instruction is the average
// of the pattern map over its SURVIVING electrons' positions, each displaced by N(0, sigma_r) along the radius and N(0, sigma_a)
// across it; electrons that end outside tpc_radius do not count.  One workgroup per instruction, after k_s2_electrons: batches of
// 256 electrons -- a thread displaces one electron and finds its 4 neighbours (grid nodes, or the points of a point-list map through its cell index), then the threads, one or two
// channels each, add the 256 weighted patterns in electron order (a fixed order: reproducible sums).  An instruction without an
// electron inside gets no pattern: its electrons make no photons (the reference's NaN pattern sends them to channel -1).
struct DiffArgs { i64 n_rows; const i32 *row_ins; const double *sig_r, *sig_a; double r2max; double *pre; };

__global__ __launch_bounds__(256) void k_diffuse_patterns(WfsDev d, GenArgs a, MapArgs m, DiffArgs q)
{
    __shared__ i32 s_idx[256][4]; __shared__ double s_w[256][4]; __shared__ i32 s_n, s_wn[4];
    const i64 r = blockIdx.x; const int tid = threadIdx.x;
    const i32 ins = q.row_ins[r];
    const double x0 = (double)m.x[ins], y0 = (double)m.y[ins];
    const double th = atan2(y0, x0), ct = cos(th), st = sin(th);
    const double sr = q.sig_r[ins], sa = q.sig_a[ins];
    const i64 e0 = a.em_off[ins], e1 = a.em_off[ins + 1];
    const u32 jb = a.ins_embase[ins], gid = a.ins_gid[ins];
    double acc[2] = {0.0, 0.0};
    i64 n_in = 0;
    for (i64 base = e0; base < e1; base += 256) {
        const i64 e = base + tid;
        bool ok = e < e1 && a.em_time[e] != I64_MIN;
        double w[4] = {0, 0, 0, 0}, ws = 1; i64 bi[MAP_K];
        if (ok) {
            const u32x4 B = philox4x32_10(jb + (u32)(e - e0), gid, 0, SITE_EL_DIFF, d.k0, d.k1);
            double z0, z1;
            box_muller(B, z0, z1);
            const double hr = z0 * sr, ha = z1 * sa;
            const double pos[3] = {x0 + (ct * hr - st * ha), y0 + (st * hr + ct * ha), 0.0};
            ok = pos[0] * pos[0] + pos[1] * pos[1] <= q.r2max;
            if (ok) {
                double bd[MAP_K];
                if (m.points) points_nearest_2d(m, pos, bd, bi); else grid_nearest(m, pos, bd, bi);
                ws = 0;
                for (int k = 0; k < 4; k++) { const double dist = sqrt(bd[k]); w[k] = bi[k] >= 0 ? 1.0 / (dist < 1e-6 ? 1e-6 : dist) : 0.0; ws += w[k]; }
            }
        }
        // slots in electron order (ballot ranks): the sums below run in a fixed order
        const u64 mask = ballot64(ok);
        if ((tid & 63) == 0) s_wn[tid >> 6] = __popcll(mask);
        __syncthreads();
        int slot = __popcll(mask & ((1ull << (tid & 63)) - 1ull));
        for (int v = 0; v < (tid >> 6); v++) slot += s_wn[v];
        if (ok) for (int k = 0; k < 4; k++) { s_idx[slot][k] = bi[k] >= 0 ? (i32)bi[k] : 0; s_w[slot][k] = w[k] / ws; }
        if (tid == 0) s_n = s_wn[0] + s_wn[1] + s_wn[2] + s_wn[3];
        __syncthreads();
        const int nb = s_n;
        n_in += nb;
        for (int c = tid, u = 0; c < m.n_map_ch && u < 2; c += 256, u++) {
            double sum = acc[u];
            for (int p = 0; p < nb; p++)
                for (int k = 0; k < 4; k++) sum += s_w[p][k] * (double)m.values[(i64)s_idx[p][k] * m.n_map_ch + c];
            acc[u] = sum;
        }
        __syncthreads();
    }
    for (int c = tid, u = 0; c < m.n_map_ch && u < 2; c += 256, u++) q.pre[r * m.n_map_ch + c] = n_in > 0 ? acc[u] / (double)n_in : 0.0;
    if (n_in == 0) for (i64 e = e0 + tid; e < e1; e += 256) a.em_nph[e] = 0;
}

// scalar maps (LCE, S2 correction, SE gain, longitudinal diffusion ...: s1.py:125, s2.py:170-234): the weighted average itself
// (nv values per node: array-valued maps, load_resource.py:383-401 make_map -- one thread per (position, value))
__global__ void k_map_scalar(MapArgs m, const double *values, double *out, int nv)
{
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m.n_rows * nv) return;
    const i64 r = t / nv; const int v = (int)(t - r * nv);
    double num = 0, den = 0;
    for (int k = 0; k < MAP_K; k++) {
        const i64 i = m.nb_idx[r * MAP_K + k];
        if (i < 0) continue;
        const double w = m.nb_w[r * MAP_K + k];
        num += values[i * nv + v] * w; den += w;
    }
    out[t] = den > 0 ? num / den : __builtin_nan("");
}

// scipy.interpolate.RegularGridInterpolator(method='linear', bounds_error=False, fill_value=None) -- what straxen's InterpolatingMap
// builds for method 'RegularGridInterpolator' (load_resource.py:357, 383-401): multilinear inside the grid, the edge cell's plane
// continued outside it.  Per axis the cell (clamped to [0, n - 2]) and the normalised distance to its lower node, then the sum over
// the cell's 2^dims corners of value * product of weights, corners in scipy's order (itertools.product of (i, i + 1) per axis).
struct LinearMapArgs { i32 dims, nv; i32 n[3]; double lo[3], h[3]; const double *values; i64 n_rows; const double *pos; double *out; };
__global__ void k_map_linear(LinearMapArgs a)
{
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_rows * a.nv) return;
    const i64 r = t / a.nv; const int v = (int)(t - r * a.nv);
    i64 cell[3] = {0, 0, 0}; double f[3] = {0, 0, 0};
    for (int q = 0; q < a.dims; q++) {
        const double x = (a.pos[r * a.dims + q] - a.lo[q]) / a.h[q];
        i64 c = (i64)floor(x);
        c = c < 0 ? 0 : (c > a.n[q] - 2 ? a.n[q] - 2 : c);
        cell[q] = c; f[q] = x - (double)c;
    }
    double sum = 0.0;
    for (int corner = 0; corner < (1 << a.dims); corner++) {
        double w = 1.0; i64 idx = 0;
        for (int q = 0; q < a.dims; q++) {
            const int up = (corner >> (a.dims - 1 - q)) & 1;
            w *= up ? f[q] : 1.0 - f[q];
            idx = idx * a.n[q] + cell[q] + up;
        }
        sum += a.values[idx * a.nv + v] * w;
    }
    a.out[t] = sum;
}

// scipy.interpolate.RectBivariateSpline.ev (the field-dependence and COMSOL distortion maps, load_resource.py:316, 326): FITPACK's
// bispeu on the spline's own knots and coefficients -- arguments clamped to the knot range, knot span by search, the
// k + 1 non-zero B-splines by the stable recurrence of de Boor and Cox (fpbspl), coefficients summed in fpbisp's order.
struct SplineArgs { i32 nx, ny, kx, ky; const double *tx, *ty, *c; i64 n; const double *pos; double *out; };

__device__ __forceinline__ int spline_span(const double *t, int n, int k, double &x, double h[6])
{
    const int nk1 = n - k - 1;
    const double tb = t[k], te = t[nk1];
    if (x < tb) x = tb;
    if (x > te) x = te;
    int l = k;
    while (!(x < t[l + 1]) && l + 1 != nk1) l++;
    double hh[5];
    h[0] = 1.0;
    for (int j = 1; j <= k; j++) {
        for (int i = 0; i < j; i++) hh[i] = h[i];
        h[0] = 0.0;
        for (int i = 0; i < j; i++) {
            const int li = l + i + 1, lj = li - j;
            if (t[li] == t[lj]) { h[i + 1] = 0.0; continue; }
            const double f = hh[i] / (t[li] - t[lj]);
            h[i] += f * (t[li] - x);
            h[i + 1] = f * (x - t[lj]);
        }
    }
    return l - k;
}

__global__ void k_map_spline(SplineArgs a)
{
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    double x = a.pos[2 * r], y = a.pos[2 * r + 1], hx[6], hy[6];
    const int lx = spline_span(a.tx, a.nx, a.kx, x, hx), ly = spline_span(a.ty, a.ny, a.ky, y, hy);
    const int nky1 = a.ny - a.ky - 1;
    double sp = 0;
    for (int i = 0; i <= a.kx; i++)
        for (int j = 0; j <= a.ky; j++) sp += a.c[(i64)(lx + i) * nky1 + ly + j] * hx[i] * hy[j];
    a.out[r] = sp;
}

// one workgroup per row: weighted average of the neighbours' patterns, turned-off PMTs removed, normalised, cumulative sum
__global__ __launch_bounds__(256) void k_map_rows(MapArgs m, int nch)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *p = (double *)(smem + map_rows_lds(nch).p);      // [nch]
    __shared__ double s_part[4]; __shared__ double s_sum;
    const i64 r = blockIdx.x; const int tid = threadIdx.x;
    double w[MAP_K]; i64 idx[MAP_K]; double wsum = 0;
    for (int k = 0; k < MAP_K; k++) { w[k] = m.pre ? 0.0 : m.nb_w[r * MAP_K + k]; idx[k] = m.pre ? -1 : m.nb_idx[r * MAP_K + k]; wsum += w[k]; }
    double part = 0;
    for (int c = tid; c < nch; c += 256) {
        double v = 1.0;
        if (c < m.n_map_ch && m.pre) v = m.pre[r * m.n_map_ch + c];
        else if (c < m.n_map_ch) {
            double acc = 0;
            for (int k = 0; k < MAP_K; k++) if (idx[k] >= 0) acc += w[k] * (double)m.values[idx[k] * m.n_map_ch + c];
            v = acc / wsum;
        }
        if (m.gains[c] == 0) v = 0;
        p[c] = v; part += v;
    }
    for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o, 64);
    if ((tid & 63) == 0) s_part[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
        const double tot = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
        // s2_aft_sigma (s2.py:660-665): the top-array fraction of the normalised pattern times the instruction's skew-normal
        // factor, clipped to [0, 1]; top channels scaled by new / cur, the others by (1 - new) / (1 - cur)
        double s_top = 1.0, s_bot = 1.0;
        if (m.aft && tot > 0) {
            double top = 0;
            for (int c = 0; c < m.n_top; c++) top += p[c];
            const double cur = top / tot, f = m.aft[m.row_ins[r]];
            if (cur > 0 && cur < 1 && f == f) {
                double nw = cur * f; nw = nw < 0 ? 0 : (nw > 1 ? 1 : nw);
                s_top = nw / cur; s_bot = (1 - nw) / (1 - cur);
            }
        }
        // np.random.choice: cdf = cumsum(p / sum); cdf /= cdf[-1]  (sequential, as numpy's cumsum)
        double run = 0;
        for (int c = 0; c < nch; c++) { run += tot > 0 ? p[c] / tot * (c < m.n_top ? s_top : s_bot) : 1.0 / nch; p[c] = run; }
        s_sum = run;
    }
    __syncthreads();
    const i64 rid = m.row_id[r];
    double *row = m.cdf_table + rid * nch;
    for (int c = tid; c < nch; c += 256) row[c] = p[c] / s_sum;
}

// Between the passes: where in its tile every single-instruction block puts its photons.  Thread = (instruction,
// channel): a running sum over the instruction's blocks in block order, starting behind whatever the generic path
// already counted into the tile.  Consecutive blocks get consecutive ranges (no atomics, a reproducible layout).
__global__ void k_block_ranges(WfsDev d, GenArgs a)
{
    const i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const int nch = d.n_tpc;
    if (idx >= a.n_psets * nch) return;
    const i32 set = (i32)(idx / nch); const int c = (int)(idx - (i64)set * nch);
    u32 run = (u32)a.tile_count[idx];
    for (i64 q = a.set_ins_off[set]; q < a.set_ins_off[set + 1]; q++) {      // the set's instructions, in order
        const i32 ins = a.set_ins_list[q];
        const i64 pa = a.ins_ph0[ins], pb = a.ins_ph0[ins + 1];     // photons [pa, pb) of the instruction
        if (pb <= pa) continue;
        const i64 b1 = (pb - 1) / GEN_BLOCK;
        constexpr int NB = 8;                                    // blocks at a time: their loads are in flight together
        for (i64 b0 = pa / GEN_BLOCK; b0 <= b1; b0 += NB) {
            u32 cnt[NB]; bool mine[NB];
#pragma unroll
            for (int k = 0; k < NB; k++) {
                const i64 b = b0 + k < b1 ? b0 + k : b1;
                const i32 bi = a.blk_ins[b];                     // (unconditional: a load behind && is waited for before the next one)
                cnt[k] = a.blk_cnt[b * nch + c];
                mine[k] = b0 + k <= b1 && bi == ins;
            }
#pragma unroll
            for (int k = 0; k < NB; k++) if (mine[k]) { a.blk_base[(b0 + k) * nch + c] = run; run += cnt[k]; }
        }
    }
    a.tile_tailbase[idx] = (i32)run;                             // the last photons of the instruction (generic path) go behind the block ranges
    run += (u32)a.tile_tail[idx]; a.tile_tail[idx] = 0;         // (the fill pass counts them again as it places them)
    a.tile_count[idx] = (i32)run;
}

// channel thresholds of a CDF row for 32-bit words: channel = first c with w / 2^32 < cdf[c], i.e. w < cdf[c] * 2^32, i.e.
// (w an integer) w <= ceil(cdf[c] * 2^32) - 1 =: T[c] -- exact, and the same decision as np.random.choice's
// searchsorted(cdf, u, 'right') on u = w / 2^32.  Channels with cdf == 0 are never examined: the search starts at
// guide[w >> 23], the first channel whose cumulative probability exceeds (w >> 23) / 512 >= 0.
__device__ __forceinline__ u32 cdf_threshold(double c)
{
    const double x = ceil(c * 4294967296.0);
    return x >= 4294967296.0 ? 0xffffffffu : (x >= 1.0 ? (u32)x - 1u : 0u);
}
// Channel of a photon from its 32-bit word: Walker's alias method over the 2^lg >= n_tpc cells of the instruction's row (built by
// k_chan_alias from the cumulative row, identically in the oracle): the top lg bits pick the cell, the remaining bits, left-aligned,
// are compared with the cell's threshold -- ONE 8-byte look-up instead of a guide read and a threshold search (RNG spec v8; the
// probabilities are those of np.random.choice's row to 2^-32, as with the thresholds before).
__device__ __forceinline__ int channel_lookup(const uint2 *A, int lg, u32 w)
{
    const u32 cell = w >> (32 - lg);
    const uint2 e = A[cell];
    return (int)(((w << lg) < e.x) ? cell : e.y);
}

// Alias cells of every channel CDF row.  One workgroup per row, thread 0 runs Vose's construction exactly as the host does for the
// delay tables (build_alias: cells below 1 and the others on two stacks, ascending fill, last in first out) so that the oracle,
// which restates it in C, gets the same cells bit for bit (IEEE adds and compares only).
__global__ __launch_bounds__(64) void k_chan_alias(const double *cdf_table, int nch, int lg, uint2 *out)
{
    __shared__ double q[WFS_MAX_CH];
    __shared__ unsigned short st_small[WFS_MAX_CH], st_large[WFS_MAX_CH];
    __shared__ uint2 cell[WFS_MAX_CH];                     // (built in LDS, written out together: the sequential part touches no global memory)
    const i64 r = blockIdx.x; const int K = 1 << lg;
    const double *cum = cdf_table + r * nch;
    // the two stacks, filled in ascending cell order by the whole wave (ballot ranks), then the sequential pairing on lane 0 with the
    // open "large" cell kept in registers
    int ns = 0, nl = 0;
    for (int i0 = 0; i0 < K; i0 += 64) {
        const int i = i0 + threadIdx.x;
        // (K = 2^lg can be below the wave width: lanes behind the last cell take no part -- phantom zero-mass cells on the small
        // stack would drain the large ones and leave the row uniform over all K cells, channels >= n_tpc included)
        const bool valid = i < K;
        const double qi = i < nch ? (cum[i] - (i ? cum[i - 1] : 0.0)) * (double)K : 0.0;
        if (valid) { q[i] = qi; cell[i] = uint2{0xffffffffu, (u32)i}; }
        const bool sm = valid && qi < 1.0, lgc = valid && !(qi < 1.0);
        const u64 ms = ballot64(sm), ml = ballot64(lgc), below = (1ull << threadIdx.x) - 1ull;
        if (sm) st_small[ns + __popcll(ms & below)] = (unsigned short)i; else if (lgc) st_large[nl + __popcll(ml & below)] = (unsigned short)i;
        ns += __popcll(ms); nl += __popcll(ml);
    }
    __syncthreads();
    if (threadIdx.x == 0 && ns > 0 && nl > 0) {
        int l = st_large[nl - 1]; double ql = q[l];
        for (;;) {
            const int sidx = st_small[--ns];
            const double qs = q[sidx];
            const double t = qs * 4294967296.0;
            cell[sidx] = uint2{t >= 4294967295.0 ? 0xffffffffu : (u32)t, (u32)l};
            ql = (ql + qs) - 1.0;
            if (ql < 1.0) { q[l] = ql; nl--; st_small[ns++] = (unsigned short)l; if (nl == 0) break; l = st_large[nl - 1]; ql = q[l]; }
            if (ns == 0) break;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < K; i += 64) out[r * K + i] = cell[i];
}

// photon p (generation order) -> emitter, instruction, Philox coordinates; generic path and k_photon_times
struct PhotonId { i64 em; i32 ins; u32 gid, eb, j, m, P; };
__device__ __forceinline__ PhotonId photon_id(const GenArgs &a, i64 p, i64 lo = 0, i64 hi = -1)
{
    if (hi < 0) hi = a.n_emitters;                 // emitter of p lies in [lo, hi): the caller may know a narrower range
    while (hi - lo > 1) { i64 mid = (lo + hi) >> 1; if (a.em_ph_off[mid] <= p) lo = mid; else hi = mid; }
    PhotonId r; r.em = lo; r.ins = a.em_ins[lo]; r.gid = a.ins_gid[r.ins]; r.eb = a.ins_embase[r.ins];
    r.j = (u32)(lo - a.em_off[r.ins]) + r.eb; r.m = (u32)(p - a.em_ph_off[lo]); r.P = (u32)(p - a.ins_ph0[r.ins]);
    return r;
}
__device__ __forceinline__ u32 photon_word(const WfsDev &d, const PhotonId &id, u32 site)
{
    return word_of(philox4x32_10(id.eb, id.gid, id.P >> 2, site, d.k0, d.k1), (int)(id.P & 3u));
}
__device__ __forceinline__ int photon_channel_global(const WfsDev &d, const GenArgs &a, const PhotonId &id)
{
    return channel_lookup(a.chan_alias + ((size_t)a.ins_cdfrow[id.ins] << a.ch_lg), a.ch_lg, photon_word(d, id, SITE_CH));
}

// A block that spans instructions (generic path) holds the LAST photons of the instruction it starts in and the FIRST photons of the
// ones that begin in it.  The tile of a single-instruction pulse set is laid out [first photons (generic) | block ranges in block
// order | last photons (generic)]: photon order up to the order inside the two small generic groups, which k_tile_order_scan repairs.
__device__ __forceinline__ bool generic_is_tail(const GenArgs &a, const PhotonId &id, i64 p0)
{
    return a.ins_ph0[id.ins] < p0 && !a.ins_fullsort[id.ins];
}

#define COUNT_TPB (GEN_BLOCK / 8)
#define FILL_TPB (GEN_BLOCK / 4)   // one quad of photons per thread: many waves per workgroup keep enough table gathers in flight

// Workgroups are dealt to the 8 XCDs round robin: XCD x (= workgroup id % 8) takes the photon blocks [x * chunk, (x + 1) * chunk)
// in order, so that the blocks writing neighbouring ranges of a tile run close together in time behind the same L2.
__device__ __forceinline__ i64 block_of_workgroup(const GenArgs &a) { return (i64)(blockIdx.x & 7) * a.xcd_chunk + (blockIdx.x >> 3); }

// 'garfield_gas_gap' luminescence: sum of the excitation times of every instruction's photons (block by block like the count
// pass; only launched when a loaded instruction uses the model)
__global__ __launch_bounds__(256) void k_gg_sum(WfsDev d, GenArgs a)
{
    const i64 vb = blockIdx.x;
    if (vb >= a.n_blocks) return;
    const BlockDesc bd = a.blk_desc[vb];
    const i64 p0 = vb * GEN_BLOCK;
    const int np = (int)((p0 + GEN_BLOCK < a.n_photons) ? GEN_BLOCK : a.n_photons - p0);
    if (bd.ins >= 0) {
        const i32 lo = a.ins_gg[bd.ins];
        if (lo < 0) return;                                  // block-uniform
        const double wgt = a.ins_ggw[bd.ins];
        const u32 q0 = (u32)(bd.R0 >> 2); const int r = (int)(bd.R0 & 3);
        i64 sum = 0;
        for (int qi = threadIdx.x; 4 * qi - r < np; qi += 256) {
            const u32x4 W = philox4x32_10(bd.eb, bd.gid, q0 + (u32)qi, SITE_LUM, d.k0, d.k1);
#pragma unroll
            for (int k = 0; k < 4; k++) { const int pr = 4 * qi + k - r; if (pr >= 0 && pr < np) sum += __double2ll_rn(gg_time(a, lo, wgt, word_of(W, k)) * 1048576.0); }
        }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
        if ((threadIdx.x & 63) == 0 && sum) atomicAdd((u64 *)&a.ins_ggsum[bd.ins], (u64)sum);
    } else {
        for (int pr = threadIdx.x; pr < np; pr += 256) {
            const PhotonId id = photon_id(a, p0 + pr, a.blk_e[2 * vb], a.blk_e[2 * vb + 1] + 1);
            const i32 lo = a.ins_gg[id.ins];
            if (lo >= 0) atomicAdd((u64 *)&a.ins_ggsum[id.ins], (u64)__double2ll_rn(gg_time(a, lo, a.ins_ggw[id.ins], photon_word(d, id, SITE_LUM)) * 1048576.0));
        }
    }
}

__global__ __launch_bounds__(COUNT_TPB) void k_photon_count(WfsDev d, GenArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nch = d.n_tpc, tid = threadIdx.x;
    const int lg = a.ch_lg, K = 1 << lg;
    const CountLds o = count_lds(nch, lg);
    uint2 *A = (uint2 *)(smem + o.A);                               // [K] alias cells of the instruction's channel row
    i32 *hist = (i32 *)(smem + o.hist);                             // [nch]
    const i64 vb = block_of_workgroup(a);
    if (vb >= a.n_blocks) return;                            // block-uniform (padding of the XCD order)
    const BlockDesc bd = a.blk_desc[vb];                     // block-uniform: scalar loads
    const i64 p0 = vb * GEN_BLOCK;
    const int np = (int)((p0 + GEN_BLOCK < a.n_photons) ? GEN_BLOCK : a.n_photons - p0);
    if (bd.ins >= 0) {
        for (int c = tid; c < nch; c += COUNT_TPB) hist[c] = 0;
        for (int c = tid; c < K; c += COUNT_TPB) A[c] = a.chan_alias[((size_t)bd.row << lg) + c];
        __syncthreads();
        const u32 q0 = (u32)(bd.R0 >> 2); const int r = (int)(bd.R0 & 3);
        for (int qi = tid; 4 * qi - r < np; qi += COUNT_TPB) {  // quad qi of the block: photons 4 * qi - r .. + 3 (block-relative)
            const u32x4 W = philox4x32_10(bd.eb, bd.gid, q0 + (u32)qi, SITE_CH, d.k0, d.k1);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int pr = 4 * qi + k - r;
                if (pr >= 0 && pr < np) atomicAdd(&hist[channel_lookup(A, lg, word_of(W, k))], 1);
            }
        }
        __syncthreads();
        for (int c = tid; c < nch; c += COUNT_TPB) a.blk_cnt[vb * nch + c] = (unsigned short)hist[c];     // -> k_block_ranges
    } else {
        for (int pr = tid; pr < np; pr += COUNT_TPB) {
            const PhotonId id = photon_id(a, p0 + pr, a.blk_e[2 * vb], a.blk_e[2 * vb + 1] + 1);      // (23 dependent loads over all emitters otherwise)
            const int ch = photon_channel_global(d, a, id);
            const i64 tile = (i64)a.ins_set[id.ins] * nch + ch;
            atomicAdd(generic_is_tail(a, id, p0) ? &a.tile_tail[tile] : &a.tile_count[tile], 1);
        }
    }
}

// (LDS layout of the fill pass: gen_fill_lds, wfs_layout.h)
// EXT: delay tables per instruction and array (model variants), S1 optical propagation term
template <bool AP, bool EXT>
__global__ __launch_bounds__(FILL_TPB) void k_photon_fill(WfsDev d, GenArgs a, ApArgs ap)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TPB = FILL_TPB, CPT = (WFS_MAX_CH + TPB - 1) / TPB;      // channels per thread
    const int nch = d.n_tpc, tid = threadIdx.x;
    const int lg = a.ch_lg;
    const GenFillLds o = gen_fill_lds(nch, lg, AP);
    i32 *win = (i32 *)smem, *wtime = (i32 *)(smem + o.wtime);
    uint2 *T = (uint2 *)(smem + o.T);                        // alias cells of the block's channel row
    i32 *hist = (i32 *)(smem + o.hist), *cur = (i32 *)(smem + o.cur), *hmin = (i32 *)(smem + o.hmin), *hmax = (i32 *)(smem + o.hmax);
    i32 *hoff = (i32 *)(smem + o.hoff);
    unsigned short *chmap = (unsigned short *)(smem + o.chmap), *pidx = (unsigned short *)(smem + o.pidx);
    PhotonRec *stage = (PhotonRec *)(smem + o.stage);
    __shared__ i32 s_wtmp[TPB / 64];
    ApStage aps;
    aps.cand = (ApCand *)(smem + o.ap);
    __shared__ i32 s_apn; __shared__ i64 s_apbase;
    __shared__ i32 s_long;                                  // a (block, channel) segment of more than 64 photons exists (fast path)
    aps.n = &s_apn;
    if (AP && tid == 0) s_apn = 0;
    if (tid == 0) s_long = 0;
    const i64 vb = block_of_workgroup(a);
    if (vb >= a.n_blocks) return;
    STAMP_INIT;
    const BlockDesc bd = a.blk_desc[vb];                     // block-uniform: scalar loads
    const i64 p0 = vb * GEN_BLOCK;
    const int np = (int)((p0 + GEN_BLOCK < a.n_photons) ? GEN_BLOCK : a.n_photons - p0);

    if (bd.ins >= 0) {
        // ---- fast path: all photons of the block belong to one instruction.  Loads that depend on the block alone go first.
        i32 cnt_r[CPT]; u32 base_r[CPT];
#pragma unroll
        for (int q = 0; q < CPT; q++) { const int c = tid + q * TPB; cnt_r[q] = c < nch ? (i32)a.blk_cnt[vb * nch + c] : 0; base_r[q] = c < nch ? a.blk_base[vb * nch + c] : 0u; }
        const int nwin = bd.nwin;                            // <= GEN_WIN (k_block_emitters)
        const u32 gid = bd.gid, eb = bd.eb; const i32 set_lo = bd.set; const i64 itime = bd.itime;     // photon times are relative to the pulse set's origin
        const AliasTab &tab = bd.is_s2 ? d.tab_s2 : d.tab_s1;
        AliasTab tab_t = tab, tab_b = tab; i32 pzi = -1; double pzf = 0.0;
        if (EXT) {
            tab_t = a.tabs[a.ins_tab[bd.ins]]; tab_b = a.tabs[a.ins_tabb[bd.ins]];
            if (a.prop_top && !bd.is_s2) { pzi = a.ins_pzi[bd.ins]; pzf = a.ins_pzf[bd.ins]; }
        }
        i32 gg_lo = -1; double gg_w = 0.0, gg_m = 0.0;       // garfield gas gap luminescence of this instruction
        if (EXT && a.gg_inv && a.ins_gg[bd.ins] >= 0) { gg_lo = a.ins_gg[bd.ins]; gg_w = a.ins_ggw[bd.ins]; gg_m = gg_mean(a, bd.ins); }
#define TAB_OF(c) (EXT ? ((c) >= d.n_top ? tab_b : tab_t) : tab)
        const i64 tbase = (i64)set_lo * nch;
        const i64 set_ph0 = a.tile_off[tbase];               // first photon slot of the set: per-channel offsets fit 32 bits
        PhotonRec *out = a.ph + set_ph0;
        const u32 q0 = (u32)(bd.R0 >> 2); const int r = (int)(bd.R0 & 3);
        i32 toff_r[CPT];
#pragma unroll
        for (int q = 0; q < CPT; q++) {
            const int c = tid + q * TPB;
            if (c < nch) {
                toff_r[q] = (i32)(a.tile_off[tbase + c] - set_ph0);
                hist[c] = cnt_r[q]; cur[c] = 0; hmin[c] = 0x7fffffff; hmax[c] = (i32)0x80000000;
            }
        }
        for (int c = tid; c < (1 << lg); c += TPB) T[c] = a.chan_alias[((size_t)bd.row << lg) + c];
        for (int k = tid; k < nwin; k += TPB) {
            win[k] = (i32)(a.em_ph_off[bd.e_lo + k] - p0);
            // the block's own emitters only (slot nwin - 1 is the sentinel behind them); I64_MIN: an electron that did not survive (no photons)
            i64 wt = (k < nwin - 1) ? a.em_time[bd.e_lo + k] : I64_MIN;
            wt = wt == I64_MIN ? 0 : wt - itime;
            if (wt > 0x3fffffffLL || wt < -0x3fffffffLL) atomicMax(&a.scal->error, (i64)WFS_DEV_TIME_RANGE);      // emitter further than 2^30 ns from its set's origin
            wtime[k] = (i32)wt;
        }
        __syncthreads();                                     // hist is complete
        STAMP(d, 0);
        block_excl_scan<TPB>(hist, nch, s_wtmp);             // (ends with a barrier)
#pragma unroll
        for (int q = 0; q < CPT; q++) {
            const int c = tid + q * TPB;
            if (c < nch) {
                hoff[c] = toff_r[q] + (i32)base_r[q] - hist[c];      // (the channel of every bucket position is noted when its photon is staged)
            }
        }
        STAMP(d, 1);
        // ---- generation order: a thread takes a quad of consecutive photons; their channel, delay and gain words come from
        // three Philox calls.  The finished photon goes to its bucket position (rank inside its channel) in LDS.
        for (int qi = tid; 4 * qi - r < np; qi += TPB) {
            const u32x4 C = philox4x32_10(eb, gid, q0 + (u32)qi, SITE_CH, d.k0, d.k1);
            const u32x4 D = philox4x32_10(eb, gid, q0 + (u32)qi, SITE_DELAY, d.k0, d.k1);
            const int pr0 = 4 * qi - r;
            int ch[4]; u32 cell[4]; uint2 e[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {                    // (photons outside the block: harmless values, nothing stored)
                ch[k] = channel_lookup(T, lg, word_of(C, k));
                cell[k] = alias_cell(TAB_OF(ch[k]), word_of(D, k));
                e[k] = TAB_OF(ch[k]).cell[cell[k]];
            }
            const u32x4 G = philox4x32_10(eb, gid, q0 + (u32)qi, SITE_GAIN, d.k0, d.k1);      // (under the latency of the table gathers)
            u32x4 LW = u32x4{0u, 0u, 0u, 0u};
            if (EXT && gg_lo >= 0) LW = philox4x32_10(eb, gid, q0 + (u32)qi, SITE_LUM, d.k0, d.k1);
            // emitter of the quad's first photon: last slot with win[slot] <= pr (emitters without photons are skipped);
            // photons are spread evenly over the block's emitters, so an interpolated guess lands within a step or two
            int slot;
            {
                const int prf = pr0 < 0 ? 0 : pr0;
                slot = (int)(((u32)prf * (u32)(nwin - 1)) >> GEN_LOG);   // GEN_BLOCK >= np: slot <= nwin - 2
                while (win[slot] > prf) slot--;                          // win[0] <= 0 <= prf
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int pr = pr0 + k;
                if (pr < 0 || pr >= np) continue;
                while (win[slot + 1] <= pr) slot++;          // win[nwin - 1] = first photon behind the block's last emitter > pr
                const int c = ch[k];
                i32 t = wtime[slot] + alias_pick(TAB_OF(c), word_of(D, k), cell[k], e[k]);
                const u32 code = gain_code(word_of(G, k), d.thr_dpe, d.dpe_inv);
                const u32 j = bd.jbase + (u32)slot, m = (u32)(pr - win[slot]);
                if (EXT && pzi >= 0) {                       // s1.py:185-188: int64 array, the assignment truncates
                    const u32x4 X = philox4x32_10(j, gid, m, SITE_PH_X, d.k0, d.k1);
                    t += (i32)(i64)s1_propagation(a, c >= d.n_top, pzi, pzf, X.x);
                }
                if (EXT && gg_lo >= 0) t += (i32)(i64)(gg_time(a, gg_lo, gg_w, word_of(LW, k)) - gg_m);      // s2.py:447-450, the cast of :532
                if (AP) ap_generate(d, ap, aps, j, gid, m, set_lo, c, (code >> 16) != 0, itime, (i64)t, bd.sbase + (u32)(bd.R0 + pr));
                atomicMin(&hmin[c], t); atomicMax(&hmax[c], t);
                const int pos = hist[c] + atomicAdd(&cur[c], 1);
                stage[pos] = PhotonRec{t, code}; chmap[pos] = (unsigned short)c; pidx[pos] = (unsigned short)pr;
            }
        }
        STAMP(d, 2);
        __syncthreads();
        // the few photons of every (block, channel) segment into photon order (an insertion sort per channel): with consecutive
        // blocks owning consecutive ranges the tile is then in generation order as it is written, k_tile_order finds nothing to do
        for (int c = tid; c < nch; c += TPB) {
            const int s0 = hist[c], s1 = hist[c + 1];
            if (s1 - s0 > 64) s_long = 1;                    // (every writer stores the same value)
            if (s1 - s0 < 2 || s1 - s0 > 64) continue;       // (longer segments: by the whole workgroup, below)
            for (int i = s0 + 1; i < s1; i++) {
                const unsigned short key = pidx[i]; const PhotonRec r = stage[i];
                int j = i - 1;
                while (j >= s0 && pidx[j] > key) { pidx[j + 1] = pidx[j]; stage[j + 1] = stage[j]; j--; }
                pidx[j + 1] = key; stage[j + 1] = r;
            }
        }
        __syncthreads();
        if (s_long) {                                        // block-uniform
            // A peaked pattern row puts more than 64 photons of a block on one channel (a flat one never does: 2048 photons over
            // 494 channels).  Nothing behind this kernel looks at the block ranges of a single-instruction set (k_tile_order_scan: head
            // and tail only; no order keys are written for them), so such a segment is put into photon order here: every thread ranks
            // up to GEN_BLOCK / TPB of its photons by counting the smaller indices (they are distinct), then the records move.
            constexpr int EPT = GEN_BLOCK / TPB;
            for (int c = 0; c < nch; c++) {
                const int s0 = hist[c], n_seg = hist[c + 1] - s0;
                if (n_seg <= 64) continue;                   // block-uniform
                unsigned short key[EPT]; PhotonRec rec[EPT]; int rank[EPT];
#pragma unroll
                for (int q = 0; q < EPT; q++) {
                    const int i = tid + q * TPB;
                    rank[q] = -1;
                    if (i < n_seg) {
                        key[q] = pidx[s0 + i]; rec[q] = stage[s0 + i];
                        int rk = 0;
                        for (int j = 0; j < n_seg; j++) rk += pidx[s0 + j] < key[q] ? 1 : 0;
                        rank[q] = rk;                        // < n_seg
                    }
                }
                __syncthreads();                             // every record is read before any is written
#pragma unroll
                for (int q = 0; q < EPT; q++) if (rank[q] >= 0) { pidx[s0 + rank[q]] = key[q]; stage[s0 + rank[q]] = rec[q]; }
                __syncthreads();
            }
        }
        STAMP(d, 3);
        // ---- bucket order: neighbouring lanes store photons of the same tile to consecutive addresses
        // (order keys only where the tile is sorted as a whole: the block ranges of a single-instruction set are in order as written)
        if (a.ins_fullsort[bd.ins]) { u32 *out_idx = a.ph_idx + set_ph0; for (int i = tid; i < np; i += TPB) { const int at = hoff[chmap[i]] + i; out[at] = stage[i]; out_idx[at] = bd.sbase + (u32)(bd.R0 + pidx[i]); } }
        else for (int i = tid; i < np; i += TPB) out[hoff[chmap[i]] + i] = stage[i];
        STAMP(d, 4);
        for (int c = tid; c < nch; c += TPB)
            if (hist[c + 1] > hist[c]) { atomicMin(&a.tile_tmin[tbase + c], hmin[c]); atomicMax(&a.tile_tmax[tbase + c], hmax[c]); }
        STAMP(d, 5);
#undef TAB_OF
    } else {
        // ---- generic path: per-photon global lookups and atomics
        if (AP) __syncthreads();                             // s_apn
        for (int pr = tid; pr < np; pr += TPB) {
            const PhotonId id = photon_id(a, p0 + pr, a.blk_e[2 * vb], a.blk_e[2 * vb + 1] + 1);
            const i32 ins = id.ins;
            const int ch = photon_channel_global(d, a, id);
            const i32 set = a.ins_set[ins];
            const i64 tile = (i64)set * nch + ch;
            const i64 itime = a.set_t0[set];
            const u32 code = gain_code(photon_word(d, id, SITE_GAIN), d.thr_dpe, d.dpe_inv);
            i64 t = a.em_time[id.em] - itime;
            const AliasTab &tb = EXT ? a.tabs[ch >= d.n_top ? a.ins_tabb[ins] : a.ins_tab[ins]] : (a.ins_type[ins] != 1 ? d.tab_s2 : d.tab_s1);
            t += alias_sample(tb, photon_word(d, id, SITE_DELAY));
            if (EXT && a.prop_top && a.ins_type[ins] == 1 && a.ins_pzi[ins] >= 0) {
                const u32x4 X = philox4x32_10(id.j, id.gid, id.m, SITE_PH_X, d.k0, d.k1);
                t += (i64)s1_propagation(a, ch >= d.n_top, a.ins_pzi[ins], a.ins_pzf[ins], X.x);
            }
            if (EXT && a.gg_inv && a.ins_gg[ins] >= 0) t += (i64)(gg_time(a, a.ins_gg[ins], a.ins_ggw[ins], photon_word(d, id, SITE_LUM)) - gg_mean(a, ins));
            if (t > 0x7fffffffLL || t < -0x7fffffffLL) { atomicMax(&a.scal->error, (i64)WFS_DEV_TIME_RANGE); t = 0; }
            if (AP) ap_generate(d, ap, aps, id.j, id.gid, id.m, set, ch, (code >> 16) != 0, itime, t, a.ins_sbase[ins] + id.P);
            atomicMin(&a.tile_tmin[tile], (i32)t); atomicMax(&a.tile_tmax[tile], (i32)t);
            // photons of multi-instruction blocks take the first slots of their tile (k_block_ranges starts behind them)
            const i64 at = a.tile_off[tile] + (generic_is_tail(a, id, p0) ? a.tile_tailbase[tile] + atomicAdd(&a.tile_tail[tile], 1) : atomicAdd(&a.tile_cursor[tile], 1));
            a.ph[at] = PhotonRec{(i32)t, code}; a.ph_idx[at] = a.ins_sbase[ins] + id.P;
        }
    }
    if (AP) {
        __syncthreads();
        const int nst = s_apn < AP_STAGE ? s_apn : AP_STAGE;
        if (tid == 0 && nst > 0) s_apbase = (i64)atomicAdd((u64 *)ap.count, (u64)nst);
        __syncthreads();
        for (int k = tid; k < nst; k += TPB) { const i64 gk = s_apbase + k; if (gk < ap.cap) ap.cand[gk] = aps.cand[k]; }
    }
}

// one thread per candidate: the reference's acceptance comparison, then delay and amplitude of the accepted ones (ap_finish); a rejected
// candidate leaves a hole that k_ap_count / k_ap_place skip
__global__ void k_ap_finish(WfsDev d, GenArgs a, ApArgs ap)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const i64 n = *ap.count < ap.cap ? *ap.count : ap.cap;
    if (i >= n) return;
    const ApCand q = ap.cand[i];
    const u32x4 w = ap_call(d, q);                          // the element's own call: low bits of the first uniform, the second uniform
    const bool ok = ap_accept(d, ap, q, w);
    if (ok) ap_finish(d, a.scal, ap, q, w, i); else ap.ap_ch[i] = -1;
    // (no counter of the accepted ones here: one atomic per wave on one address was 5.5 of this kernel's 6.8 ms with 3.5 x 10^7
    // candidates -- the scan over the afterpulse tiles' counts yields the total anyway)
}

// afterpulse photons -> tiles of the afterpulse pulse set of their primary set (set n_psets + set): count, then place
// Runs of consecutive list entries that go to the same tile (the candidates of a k_s2_tile workgroup all do, in key order) share one
// atomic: the first lane of a run reserves for the run, the others take their place behind it -- in list order, so a tile filled by
// one run is in generation order as it is written.  (70 afterpulses per tile of a 10^6-PE S2: one atomic per photon on the tile's
// cursor and two on its time range serialised the kernel, 8.3 ms for 3.5 x 10^7 afterpulses.)
struct ApRun { int head, rank, len; };
__device__ __forceinline__ ApRun ap_run(i64 tile, int lane)
{
    const i64 prev = __shfl_up(tile, 1, 64);
    const u64 heads = ballot64(lane == 0 || tile != prev);
    ApRun r;
    r.head = 63 - __clzll(heads & ((2ull << lane) - 1ull));
    const u64 behind = r.head == 63 ? 0ull : heads & ~((2ull << r.head) - 1ull);
    r.len = (behind ? __builtin_ctzll(behind) : 64) - r.head;
    r.rank = lane - r.head;
    return r;
}
__global__ __launch_bounds__(256) void k_ap_count(WfsDev d, GenArgs a, ApArgs ap)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const i64 n = *ap.count < ap.cap ? *ap.count : ap.cap;
    const bool v = i < n && ap.ap_ch[i] >= 0 && !(ap.ap_ins[i] & AP_SEG_MARK);
    const i64 tile = v ? ((i64)a.n_psets + ap.ap_ins[i]) * d.n_tpc + ap.ap_ch[i] : -1 - lane;       // (a hole is a run of its own)
    const ApRun r = ap_run(tile, lane);
    if (v && r.rank == 0) atomicAdd(&a.tile_count[tile], r.len);
}

__global__ __launch_bounds__(256) void k_ap_place(WfsDev d, GenArgs a, ApArgs ap, double *ph_gain_base)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const i64 n = *ap.count < ap.cap ? *ap.count : ap.cap;
    const bool v = i < n && ap.ap_ch[i] >= 0 && !(ap.ap_ins[i] & AP_SEG_MARK);
    const i64 tile = v ? ((i64)a.n_psets + ap.ap_ins[i]) * d.n_tpc + ap.ap_ch[i] : -1 - lane;
    const ApRun r = ap_run(tile, lane);
    const i32 t = v ? ap.ap_t[i] : 0;
    i32 first = 0;
    if (v && r.rank == 0) first = atomicAdd(&a.tile_cursor[tile], r.len);
    first = __shfl(first, r.head, 64);
    // earliest / latest photon of the run, reduced towards its first lane
    i32 lo = t, hi = t;
    for (int o = 1; o < 64; o <<= 1) {
        const i32 l2 = __shfl_down(lo, o, 64), h2 = __shfl_down(hi, o, 64);
        if (r.rank + o < r.len) { lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi; }
    }
    if (!v) return;
    const i64 pos = a.tile_off[tile] + first + r.rank;
    a.ph[pos] = PhotonRec{t, 0u}; ph_gain_base[pos] = ap.ap_gain[i]; a.ph_idx[pos] = ap.ap_key[i];
    if (r.rank == 0) { atomicMin(&a.tile_tmin[tile], lo); atomicMax(&a.tile_tmax[tile], hi); }
}

// The afterpulses of a tile-generated tile: ONE wave per segment of the list (ApSeg).  PLACE false: the accepted entries are counted
// into the afterpulse tile; PLACE true: they go to the tile in list order = key order -- the tile is in generation order as written,
// whatever order the atomics of other workgroups happen in (k_tile_order finds nothing to do).
template <bool PLACE>
__global__ __launch_bounds__(256) void k_ap_seg(WfsDev d, GenArgs a, ApArgs ap, double *ph_gain_base)
{
    const int lane = threadIdx.x & 63;
    const i64 w = (i64)blockIdx.x * 4 + wave_in_block();
    if (w >= ap.n_seg) return;
    const ApSeg sg = ap.seg[w];
    if (sg.n <= 0) return;
    i32 total = 0;
    for (i32 c = 0; c < sg.n; c += 64) {
        const i64 i = sg.base + c + lane;
        total += __popcll(ballot64(c + lane < sg.n && i < ap.cap && ap.ap_ch[i] >= 0));
    }
    if (total == 0) return;
    if (!PLACE) { if (lane == 0) atomicAdd(&a.tile_count[sg.tile], total); return; }
    i32 first = 0;
    if (lane == 0) first = atomicAdd(&a.tile_cursor[sg.tile], total);
    first = __builtin_amdgcn_readfirstlane(first);
    const i64 off = a.tile_off[sg.tile] + first;
    i32 done = 0, lo = 0x7fffffff, hi = (i32)0x80000000;
    for (i32 c = 0; c < sg.n; c += 64) {
        const i64 i = sg.base + c + lane;
        const bool v = c + lane < sg.n && i < ap.cap && ap.ap_ch[i] >= 0;
        const u64 m = ballot64(v);
        if (v) {
            const i64 pos = off + done + __popcll(m & ((1ull << lane) - 1ull));
            const i32 t = ap.ap_t[i];
            a.ph[pos] = PhotonRec{t, 0u}; ph_gain_base[pos] = ap.ap_gain[i]; a.ph_idx[pos] = ap.ap_key[i];
            lo = t < lo ? t : lo; hi = t > hi ? t : hi;
        }
        done += __popcll(m);
    }
    lo = wave_min(lo); hi = wave_max(hi);
    if (lane == 0) { atomicMin(&a.tile_tmin[sg.tile], lo); atomicMax(&a.tile_tmax[sg.tile], hi); }
}

// Generation order inside every tile.  The bucketing above leaves the photons of a tile in the order the atomics happened to
// hand out slots; the reference's Pulse call sees them in channel-sorted GENERATION order (a stable argsort would; the oracle
// does), and two things depend on that order: the truth quirk that counts the triggered photons among the FIRST n_dpe of the
// channel slice (pulse.py:255) and the order in which three or more photons of one ns are merged.  Every stored photon carries
// its order key (ph_idx); tiles whose keys are out of order are listed (one thread per tile) and sorted: by a wave up to 64
// photons (rank by counting smaller keys), by a workgroup in LDS up to TILE_ORDER_MAX; larger ones -- tiles of the per-electron
// generator beyond 4096 photons: S2s of 10^5 electrons with a gain spread or inside run sets -- go on a third list and through a
// segmented radix sort over (order key, position) pairs (k_order_huge_pack / rocPRIM / k_order_huge_apply, wfs_engine.hip).
// Explicit gains (afterpulses) move along.
// (TILE_ORDER_MAX: wfs_layout.h)
#define TILE_ORDER_INLINE 12        // ranges up to this many photons are sorted by the scanning thread itself
struct OrderRange { i64 start; i32 n, pad; };          // photons [start, start + n) of the photon array
struct OrderArgs { i64 n_tiles, n_ptiles; const i32 *tile_count; const i64 *tile_off; PhotonRec *ph; u32 *ph_idx; double *ph_gain; i64 gain_first;
                   OrderRange *wave_list, *big_list; WfsScal *scal;  // ph_gain[p - gain_first] for photons p >= gain_first (afterpulses), or nullptr;
                                                                     // scal->n_order_wave / n_order_big: ranges on the wave list / the workgroup list; ranges beyond
                                                                     // TILE_ORDER_MAX photons: big_list[2 n_tiles - 1 - k], scal->n_order_huge of them
                   const i32 *skip_ins; i32 nch;                     // [n_ins] 1: the tiles of this instruction (tile / nch) come from k_s2_tile, already in order (or nullptr)
                   const i32 *tile_cursor, *tile_tailbase; const i32 *ins_fullsort; const i64 *set_ins_off; const i32 *set_ins_list; };
                   // primary tiles of a set whose (first) instruction is not flagged ins_fullsort: head = [0, cursor), tail = [tailbase, n)
// pass 1, one THREAD per tile.  A primary tile of a single-instruction pulse set is [first photons | block ranges | last photons]
// with the block ranges in order as written: only the two small generic groups are looked at.  Every other tile (afterpulse sets,
// sets of several instructions) is looked at as a whole.  A range that is out of order is sorted on the spot when it is tiny,
// listed for a wave (<= 64) or a workgroup (<= TILE_ORDER_MAX) otherwise.
__device__ __forceinline__ void order_range(const OrderArgs &a, i64 start, i32 n, int &cls)
{
    cls = -1;
    if (n < 2) return;
    const u32 *k = a.ph_idx + start;
    bool sorted = true;
    u32 prev = k[0];
    for (i32 q = 1; q < n; q++) { const u32 x = k[q]; if (x < prev) { sorted = false; break; } prev = x; }
    if (sorted) return;
    if (n > TILE_ORDER_INLINE) { cls = n <= 64 ? 0 : (n <= TILE_ORDER_MAX ? 1 : 2); return; }
    const bool has_gain = a.ph_gain && start >= a.gain_first;
    for (i32 i = 1; i < n; i++) {                            // insertion sort of a handful of records
        const u32 key = a.ph_idx[start + i]; const PhotonRec r = a.ph[start + i];
        const double g = has_gain ? a.ph_gain[start - a.gain_first + i] : 0.0;
        i32 jj = i - 1;
        while (jj >= 0 && a.ph_idx[start + jj] > key) {
            a.ph_idx[start + jj + 1] = a.ph_idx[start + jj]; a.ph[start + jj + 1] = a.ph[start + jj];
            if (has_gain) a.ph_gain[start - a.gain_first + jj + 1] = a.ph_gain[start - a.gain_first + jj];
            jj--;
        }
        a.ph_idx[start + jj + 1] = key; a.ph[start + jj + 1] = r;
        if (has_gain) a.ph_gain[start - a.gain_first + jj + 1] = g;
    }
}
__global__ __launch_bounds__(256) void k_tile_order_scan(OrderArgs a)
{
    __shared__ i32 s_n[3]; __shared__ i64 s_base[3];
    if (threadIdx.x < 3) s_n[threadIdx.x] = 0;
    __syncthreads();
    const i64 tile = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    OrderRange rg[2] = {{0, 0, 0}, {0, 0, 0}}; int cls[2] = {-1, -1}, rk[2] = {0, 0};
    if (tile < a.n_tiles) {
        const i32 n = a.tile_count[tile];
        const i64 set = tile / a.nch;
        if (n >= 2 && !(a.skip_ins && tile < a.n_ptiles && a.skip_ins[set])) {
            const i64 off = a.tile_off[tile];
            if (tile < a.n_ptiles && !a.ins_fullsort[a.set_ins_list[a.set_ins_off[set]]]) {
                rg[0] = OrderRange{off, a.tile_cursor[tile], 0};
                rg[1] = OrderRange{off + a.tile_tailbase[tile], n - a.tile_tailbase[tile], 0};
            } else rg[0] = OrderRange{off, n, 0};
            for (int q = 0; q < 2; q++) { order_range(a, rg[q].start, rg[q].n, cls[q]); if (cls[q] >= 0) rk[q] = atomicAdd(&s_n[cls[q]], 1); }
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_n[threadIdx.x]) {
        i64 *const counter = threadIdx.x == 0 ? &a.scal->n_order_wave : (threadIdx.x == 1 ? &a.scal->n_order_big : &a.scal->n_order_huge);
        s_base[threadIdx.x] = (i64)atomicAdd((u64 *)counter, (u64)s_n[threadIdx.x]);
    }
    __syncthreads();
    for (int q = 0; q < 2; q++) {
        if (cls[q] == 0) a.wave_list[s_base[0] + rk[q]] = rg[q];
        else if (cls[q] == 1) a.big_list[s_base[1] + rk[q]] = rg[q];
        else if (cls[q] == 2) a.big_list[2 * a.n_tiles - 1 - (s_base[2] + rk[q])] = rg[q];
    }
}
// Ranges beyond TILE_ORDER_MAX photons: their order keys, positions and records are copied to compact arrays (range k at cbeg[k]), the
// (key, position) pairs are sorted range by range (rocPRIM's segmented radix sort), and the records move to their ranks.
struct HugeOrderArgs { i64 n_ranges, total; const i64 *start; const i64 *cbeg; const PhotonRec *ph; const u32 *ph_idx; const double *ph_gain; i64 gain_first;
                       u32 *keys, *vals; PhotonRec *rec; double *gain; };
__device__ __forceinline__ i64 huge_range_of(const HugeOrderArgs &a, i64 i)
{
    i64 lo = 0, hi = a.n_ranges;
    while (hi - lo > 1) { const i64 mid = (lo + hi) >> 1; if (a.cbeg[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}
__global__ void k_order_huge_pack(HugeOrderArgs a)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const i64 r = huge_range_of(a, i), p = a.start[r] + (i - a.cbeg[r]);
    a.keys[i] = a.ph_idx[p]; a.vals[i] = (u32)(i - a.cbeg[r]); a.rec[i] = a.ph[p];
    if (a.ph_gain && p >= a.gain_first) a.gain[i] = a.ph_gain[p - a.gain_first];
}
__global__ void k_order_huge_apply(HugeOrderArgs a, const u32 *keys_sorted, const u32 *vals_sorted, PhotonRec *ph, u32 *ph_idx, double *ph_gain)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const i64 r = huge_range_of(a, i), p = a.start[r] + (i - a.cbeg[r]);
    const i64 src = a.cbeg[r] + vals_sorted[i];
    ph[p] = a.rec[src]; ph_idx[p] = keys_sorted[i];
    if (ph_gain && p >= a.gain_first) ph_gain[p - a.gain_first] = a.gain[src];
}
// pass 2, one wave per listed range of at most 64 photons: rank = number of smaller keys (the keys of a range are distinct)
__global__ __launch_bounds__(256) void k_tile_order(OrderArgs a, i64 n_list)
{
    const int lane = threadIdx.x & 63;
    const i64 li = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (li >= n_list) return;
    const OrderRange rg = a.wave_list[li];
    const i32 n = rg.n; const i64 off = rg.start;
    const bool v = lane < n;
    const u32 k0 = v ? a.ph_idx[off + lane] : 0xffffffffu;
    const PhotonRec r0 = a.ph[off + (v ? lane : 0)];
    const bool has_gain = a.ph_gain && off >= a.gain_first;
    const double g0 = has_gain ? a.ph_gain[off - a.gain_first + (v ? lane : 0)] : 0.0;
    int rank = 0;
    for (int j = 0; j < n; j++) rank += (u32)__builtin_amdgcn_readlane((int)k0, j) < k0;
    if (v) {
        a.ph[off + rank] = r0; a.ph_idx[off + rank] = k0;
        if (has_gain) a.ph_gain[off - a.gain_first + rank] = g0;
    }
}
// ranges of 65 .. TILE_ORDER_MAX photons: (key, position) pairs sorted in LDS (bitonic), then the records move
__global__ __launch_bounds__(256) void k_tile_order_big(OrderArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const OrderRange rg = a.big_list[blockIdx.x];
    const i32 n = rg.n; const i64 off = rg.start;
    int np2 = 128; while (np2 < n) np2 <<= 1;
    // (the carve is written out: taking the offsets from order_lds(np2) costs the kernel a scalar register; the asserts tie the two)
    static_assert(order_lds(128).key == 0 && order_lds(128).rec == 128 * sizeof(u64) && order_lds(128).gain == order_lds(128).rec + 128 * sizeof(PhotonRec)
                  && order_lds(128).total == order_lds(128).gain + 128 * sizeof(double), "k_tile_order_big carves [key | rec | gain] of np2 entries each");
    u64 *key = (u64 *)smem;                                  // [np2] key << 32 | position (np2 <= TILE_ORDER_MAX, which the launch reserves for)
    const int tid = threadIdx.x;
    for (int i = tid; i < np2; i += 256) key[i] = i < n ? ((u64)a.ph_idx[off + i] << 32) | (u32)i : ~0ull;
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const u64 x = key[i], y = key[l];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) { key[i] = y; key[l] = x; }
                }
            }
            __syncthreads();
        }
    const bool has_gain = a.ph_gain && off >= a.gain_first;
    PhotonRec *ph = a.ph + off; u32 *idx = a.ph_idx + off; double *pg = has_gain ? a.ph_gain + (off - a.gain_first) : nullptr;
    PhotonRec *cr = (PhotonRec *)(key + np2);                 // [n] copies: every record is read before any is written
    double *cg = (double *)(cr + np2);
    for (int i = tid; i < n; i += 256) { cr[i] = ph[i]; if (has_gain) cg[i] = pg[i]; }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int src = (int)(u32)key[i];
        ph[i] = cr[src]; idx[i] = (u32)(key[i] >> 32);
        if (has_gain) pg[i] = cg[src];
    }
}

// Arrival times of chosen photons, addressed by their index in GENERATION order (emitter by emitter, the order of
// em_ph_off): electron afterpulses pick random detected photons of their parent S2 as time zeros (afterpulse.py:44-47).
// The time is recomputed from the photon's own Philox draw (site B), so the choice does not depend on where the
// bucketing put the photon.
__global__ void k_photon_times(WfsDev d, GenArgs a, i64 n, const i64 *index, i64 *out)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PhotonId id = photon_id(a, index[i]);
    const i32 ins = id.ins;
    const u32 w = photon_word(d, id, SITE_DELAY);
    if (a.tabs) {                                            // model variants: the table depends on the photon's array
        const int ch = photon_channel_global(d, a, id);
        i64 t = a.em_time[id.em] + alias_sample(a.tabs[ch >= d.n_top ? a.ins_tabb[ins] : a.ins_tab[ins]], w);
        if (a.prop_top && a.ins_type[ins] == 1 && a.ins_pzi[ins] >= 0) {
            const u32x4 X = philox4x32_10(id.j, id.gid, id.m, SITE_PH_X, d.k0, d.k1);
            t += (i64)s1_propagation(a, ch >= d.n_top, a.ins_pzi[ins], a.ins_pzf[ins], X.x);
        }
        if (a.gg_inv && a.ins_gg[ins] >= 0) t += (i64)(gg_time(a, a.ins_gg[ins], a.ins_ggw[ins], photon_word(d, id, SITE_LUM)) - gg_mean(a, ins));
        out[i] = t;
        return;
    }
    out[i] = a.em_time[id.em] + alias_sample(a.ins_type[ins] != 1 ? d.tab_s2 : d.tab_s1, w);
}

// Optical input (RawDataOptical.sim_primary, rawdata.py:475-493): photons are supplied, already bucketed by the host
// side of the ABI; what is left of Pulse.__call__ before add_current is drawn here per photon: transit time spread
// (pulse.py:53-56), double-PE flag (pulse.py:76-79) and the SPE gain indices (pulse.py:97-103): one Philox call.  One thread per tile.
struct OpticalArgs { i64 n_tiles; const i32 *tile_count; const i64 *tile_off; i32 *tile_tmin, *tile_tmax; const u32 *set_gid;
                     const i32 *in_t; const u32 *in_item; PhotonRec *ph; WfsScal *scal; };

// Bucketing of the supplied photons by (instruction, channel) -- one thread per instruction, which owns the instruction's tiles
// (plain read-modify-write).  The host used to do this over dense per-tile arrays: 0.4 s of 0.5 s per 4 x 10^5 nVeto instructions.
// rawdata.py:485-486: photons with a negative time or beyond the cutoff are dropped; pulse.py:89-90: so are those of turned-off PMTs.
struct OptLoadArgs { i64 n; const i32 *first, *last, *channels; const i64 *timings; i64 cutoff; const double *gains;
                     i32 *tile_count; const i64 *tile_off; i32 *tile_cursor; i32 *in_t; u32 *in_item; WfsScal *scal; };

template <bool PLACE>
__global__ void k_optical_bucket(WfsDev d, OptLoadArgs a)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const i32 f = a.first[i], l = a.last[i];
    for (i32 k = f; k < l; k++) {
        const i64 t = a.timings[k];
        if (t < 0 || t >= a.cutoff) continue;
        const i32 ch = a.channels[k];
        if (ch < 0 || ch >= d.n_tpc) { atomicMax(&a.scal->opt_error, (i64)WFS_DEV_OPT_CHANNEL); continue; }      // photon channel out of range
        if (a.gains[ch] == 0) continue;
        if (t > 0x7ffffff0LL) { atomicMax(&a.scal->opt_error, (i64)WFS_DEV_OPT_TIME); continue; }              // photon time beyond 2^31 ns
        const i64 tile = i * d.n_tpc + ch;
        if (!PLACE) a.tile_count[tile]++;
        else { const i64 pos = a.tile_off[tile] + a.tile_cursor[tile]++; a.in_t[pos] = (i32)t; a.in_item[pos] = (u32)(k - f); }
    }
}

__global__ void k_optical_finish(WfsDev d, OpticalArgs a)
{
    const i64 tile = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (tile >= a.n_tiles) return;
    const i32 n = a.tile_count[tile];
    if (n <= 0) return;
    const i64 off = a.tile_off[tile];
    const u32 gid = a.set_gid[tile / d.n_tpc];
    i32 tmin = 0x7fffffff, tmax = (i32)0x80000000;
    for (i32 p = 0; p < n; p++) {
        const u32 item = a.in_item[off + p];                 // index of the photon inside its instruction's range
        const u32x4 B = philox4x32_10(0, gid, item, SITE_PH, d.k0, d.k1);
        i64 t = a.in_t[off + p];
        t += alias_sample(d.tab_tts, B.x);
        if (t > 0x7fffffffLL || t < -0x7fffffffLL) { atomicMax(&a.scal->error, (i64)WFS_DEV_TIME_RANGE); t = 0; }
        a.ph[off + p] = PhotonRec{(i32)t, gain_code(B.y, d.thr_dpe, d.dpe_inv)};
        tmin = (i32)t < tmin ? (i32)t : tmin; tmax = (i32)t > tmax ? (i32)t : tmax;
    }
    a.tile_tmin[tile] = tmin; a.tile_tmax[tile] = tmax;
}

// PMT afterpulses of supplied photons: the screening of ap_generate, one thread per PHOTON of the bucketed array (behind
// k_optical_finish, which made its time and double-PE flag).  Tiles of optical input hold 0 .. 3 photons (nVeto) or 10^2 .. 10^4
// (an optical S1 in the TPC): a thread per tile would diverge over four orders of magnitude.  The photon's tile is found by bisection
// of the primary tiles' offsets (the top levels stay in L2); its counter is (0, gid, item, site) with item = its index inside the
// instruction's _first:_last range, the coordinate of its SITE_PH draw.  Candidates leave wave-aggregated: one atomic on the list's
// counter per wave and element, every lane at base + its rank among the wave's candidates (no LDS stage, no segments).
struct OptApArgs { i64 n_photons, n_ptiles; const i64 *tile_off; const u32 *set_gid; const i64 *set_t0; const u32 *in_item; const PhotonRec *ph; };

__global__ __launch_bounds__(256) void k_optical_ap_screen(WfsDev d, OptApArgs a, ApArgs ap)
{
    const i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool v = p < a.n_photons;                          // (every lane stays for the ballots)
    i32 ins = 0, ch = 0, t = 0; u32 gid = 0, item = 0; bool dpe = false; i64 itime = 0;
    if (v) {
        i64 lo = 0, hi = a.n_ptiles;                         // the last tile that starts at or before p (it holds p: empty tiles start where the next one does)
        while (hi - lo > 1) { const i64 mid = (lo + hi) >> 1; if (a.tile_off[mid] <= p) lo = mid; else hi = mid; }
        ins = (i32)(lo / d.n_tpc); ch = (i32)(lo - (i64)ins * d.n_tpc);
        gid = a.set_gid[ins]; itime = a.set_t0[ins]; item = a.in_item[p];
        const PhotonRec r = a.ph[p];
        t = r.t; dpe = (r.code >> 16) != 0;
    }
    for (int e0 = 0; e0 < ap.n; e0 += 4) {
        const u32x4 S = philox4x32_10(0u, gid, item, SITE_AP_SCREEN + (u32)(e0 >> 2), d.k0, d.k1);
        for (int k = 0; k < 4 && e0 + k < ap.n; k++) {
            const int e = e0 + k;
            const u32 x = word_of(S, k);
            const bool c = v && (x >> 5) >= ap.thr[e][ch * 2 + (dpe ? 1 : 0)];       // (below the threshold: surely rejected, ap_threshold)
            const u64 m = ballot64(c);
            if (!m) continue;                                // (wave-uniform)
            const int leader = __builtin_ctzll(m);
            i64 base = 0;
            if (lane == leader) base = (i64)atomicAdd((u64 *)ap.count, (u64)__popcll(m));
            base = __shfl(base, leader, 64);
            if (!c) continue;
            const i64 gk = base + __popcll(m & ((1ull << lane) - 1ull));
            if (gk >= ap.cap) continue;                      // (more candidates than the list holds: the host reports it from the counter)
            ApCand q;
            q.itime = itime; q.x = x; q.ins = ins; q.ch = ch; q.t = t; q.key = ((u32)e << 29) | (item & 0x1fffffffu);
            q.j = 0u; q.m = item; q.gid = gid; q.e_dpe = e | (dpe ? 256 : 0); q.pad = 0;
            ap.cand[gk] = q;
        }
    }
}
