/*
 * wfsim_amd.h -- C ABI of the MI355X-native WFSim hot path (libwfsim_amd.so, HIP, gfx950 only).
 *
 * The reference (XENONnT/WFSim v1.2.2) is pure Python and has no FFI; its hot path lives behind
 * wfsim.RawData / wfsim.ChunkRawRecords.  This header is what a binding for that path binds: every entry point
 * names the reference routine(s) it replaces (paths relative to the reference's wfsim/ directory).  The Python
 * host side of this repository (wfsim_amd/engine.py, ctypes) is such a binding; INTEGRATION.md shows the stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; no exceptions cross the ABI: every entry point is a function-try-block that turns a C++
 *     exception of the host-side containers into a code (std::bad_alloc -> WFS_E_NOMEM, anything else -> WFS_E_INVALID)
 *     and a message.  Every function returns 0 on success or a negative WFS_E_* code; wfs_last_error(h) gives the message.
 *   - a handle owns one GPU (hipSetDevice at creation) and one HIP stream; it is not thread safe.
 *   - "host" pointers are ordinary CPU memory (numpy buffers), copied by the call; "dev" pointers are HBM
 *     addresses on the handle's GPU (e.g. torch tensors' data_ptr()).
 *   - instructions of one batch must be sorted by the scheduler key time - z/v*[S2] (rawdata.py:61) and carry
 *     their time-cluster id (gap > right_raw_extension, rawdata.py:63); wfsim_amd/scheduler.py does that.
 */
#ifndef WFSIM_AMD_H
#define WFSIM_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WFS_OK 0
#define WFS_E_INVALID (-1)   /* bad argument / shape                                      */
#define WFS_E_HIP (-2)       /* HIP runtime error (message has the call)                  */
#define WFS_E_CAPACITY (-3)  /* caller buffer too small, or the 10^6-sample window assert */
#define WFS_E_STATE (-4)     /* call order (tables / batch not loaded)                    */
#define WFS_E_NOMEM (-5)     /* host allocation failed inside the library (std::bad_alloc) */

typedef struct wfs_handle wfs_handle;

/* Scalars of the hot path.  Filled from the fax config by wfsim_amd.config.kernel_params();
 * the config keys are listed in SURVEY.md appendix A. */
typedef struct wfs_config {
    int32_t dt;                /* sample_duration                                   pulse.py:58      */
    int32_t samples_before;    /* samples_before_pulse_center                       pulse.py:121-127 */
    int32_t samples_after;     /* samples_after_pulse_center                                         */
    int32_t store_before;      /* samples_to_store_before                                            */
    int32_t store_after;       /* samples_to_store_after                                             */
    int32_t tlen;              /* template length = before + after (22)             pulse.py:175     */
    int32_t trigger_window;    /* rawdata.py:215-216, 299-304                                        */
    int32_t baseline;          /* digitizer_reference_baseline                      rawdata.py:270   */
    int32_t n_rows;            /* rows of the digitiser array (801)                 rawdata.py:224   */
    int32_t n_tpc;             /* len(gains)                                                         */
    int32_t n_top;             /* n_top_pmts                                        rawdata.py:243   */
    int32_t he_first;          /* channel_map['he'][0]                              rawdata.py:244   */
    int32_t he_factor;         /* int(high_energy_deamplification_factor)           rawdata.py:242   */
    int32_t sum_channel;       /* channel_map['sum_signal'] (emitted after wfs_set_sum_signal only)  */
    int32_t last_bottom;       /* channels_bottom[-1]                               rawdata.py:250   */
    int32_t detector_nt;       /* detector == 'XENONnT'                             rawdata.py:241   */
    int32_t enable_noise;      /* rawdata.py:263                                                     */
    int32_t s1_simple;         /* 'simple' in s1_model_type                         s1.py:191        */
    int32_t s2_time_model;     /* 0 zero_delay, 1 "s2_time_spread around zero"      s2.py:545-550    */
    int32_t enable_pmt_ap;     /* enable_pmt_afterpulses                            rawdata.py:176   */
    int32_t tile_gen;          /* 1: primary S2s whose tiles fit a pulse workgroup draw their photons there (tile-local generation,
                                  RNG spec v9): Poisson(n_e g p_ch) photons per (instruction, channel), a uniform surviving
                                  electron per photon -- the distribution of s2.py:308 + :673 when s2_gain_spread == 0.  0: every
                                  photon comes from the per-electron generator (needed by the electron-afterpulse pre-pass)   */
    int32_t tile_gen_min;      /* ... and only where amp * gain * max(p_ch) reaches this many photons: below it a workgroup per tile
                                  costs more than the block generator (crossover measured at ~60 photons per tile)        */
    int32_t fma;               /* 1 (config 'fused_multiply_add', the default): Pulse.add_current (pulse.py:303-318) accumulates
                                  template * gain into the current with ONE rounding per term (v_fma_f64) instead of the separately
                                  rounded product and sum of numpy: currents within 1 ulp of the tile maximum per term of the
                                  reference's, ADC samples / ZLE / records equal unless a current lands within that distance of a
                                  rounding tie (tolerance of the path: 1 ADC count).  0: the reference's two roundings, currents
                                  bit-exact                                                                   */
    int32_t row_resident;      /* config 'row_resident'.  1: a (window, channel) row whose pulses all
                                  hold at most 64 photons is made (in segments of 1024 samples), finished and zero-suppressed by one wave in LDS (k_row_pulse);
                                  0: every row through the integer accumulators in HBM; 2 ('auto', the default): 1 for a batch with
                                  at least two photons in the photon array per (pulse set, channel) slot, else 0.  Same records either way.          */
    double c2a;                /* current_2_adc                                     pulse.py:33-35   */
    double tts_mean, tts_sigma;/* pmt_transit_time_mean, spread/2.35482             pulse.py:53-56   */
    double p_dpe;              /* p_double_pe_emision                               pulse.py:76      */
    double s1_decay_time, s1_decay_spread;                    /*                    s1.py:193-194    */
    double sf_gas, t1_gas, t3_gas;                            /* singlet/triplet    pulse.py:333-341 */
    double s2_time_spread;                                    /*                    s2.py:550        */
    double trap_time;          /* electron_trapping_time                            s2.py:280        */
    double gain_spread;        /* s2_gain_spread                                    s2.py:309        */
    double pmt_ap_modifier, pmt_ap_t_modifier;                /*                    afterpulse.py:198,223 */
    double rext;               /* right_raw_extension                               rawdata.py:47    */
    double drift_velocity;     /* drift_velocity_liquid                             rawdata.py:46    */
    uint64_t seed;             /* Philox key (the reference seeds numpy's global generator, strax_interface.py:589) */
} wfs_config;

/* ---- life cycle: replaces RawData.__init__ / Pulse.__init__ (rawdata.py:27-36, pulse.py:24-37) ---------- */
int wfs_create(const wfs_config *cfg, int device, wfs_handle **out);
int wfs_destroy(wfs_handle *h);
const char *wfs_last_error(const wfs_handle *h);
int wfs_device_count(int *n);
int wfs_device_allocations(int64_t *buffers, int64_t *bytes);      /* device buffers, and their bytes, that the handles of this process hold now */

/* Init-time tables (host pointers, copied to HBM once).
 *   templates  f64[10][tlen]        Pulse.init_pmt_current_templates            pulse.py:146-187
 *   spe        f64[n_spe][2001]     Pulse.init_spe_scaling_factor_distributions pulse.py:189-223 (n_spe == 1: shared)
 *   gains      f64[n_tpc]           config['gains']
 *   thr_truth  f64[n_rows]          zle/special threshold - 0.5                 pulse.py:240-243
 *   thr_zle    i64[n_rows]          baseline - threshold - 1                    rawdata.py:290-294
 *   lum_x/t    f64[n_lum]           inverse-CDF table of the simple luminescence model, s2.py:317-341
 *   noise      i16[noise_len][noise_channels] or NULL                           load_resource.py:375-376 */
int wfs_set_tables(wfs_handle *h, const double *templates, const double *spe, int32_t n_spe,
                   const double *gains, const double *thr_truth, const int64_t *thr_zle,
                   const double *lum_x, const double *lum_t, int32_t n_lum,
                   const int16_t *noise, int32_t noise_len, int32_t noise_channels);

/* PMT afterpulse element tables (resource.uniform_to_pmt_ap[element], afterpulse.py:181-186), element < 8 */
int wfs_set_ap_element(wfs_handle *h, int32_t element, int32_t n_bins_delay, int32_t n_bins_amp, int32_t amp_2d,
                       int32_t is_uniform, double delay_bin, double amp_bin,
                       const double *delay_cdf, const double *amp_cdf);

/* ---- batch input ------------------------------------------------------------------------------------- */
/* A handle holds one batch: the one the last successful wfs_load_instructions, wfs_load_photons or wfs_load_optical call
 * described.  Each of the three replaces the batch before it as a whole: its kind, its sizes, every per-instruction option
 * (wfs_set_instruction_*, wfs_eval_pattern_rows) and the results of its last run.  A load that returns an error after its
 * argument checks (a value out of range inside the arrays, a failed upload) leaves the handle with NO batch, not with the one
 * before: wfs_run and the per-instruction setters then return WFS_E_STATE ("no batch loaded") until a load succeeds.  A call that
 * is refused for a null or empty argument, or before wfs_set_tables, touches nothing. */
/* One batch of primary instructions (host pointers; SoA because instruction_dtype is a packed 70-byte record
 * with an unaligned int64, strax_interface.py:25-42).  Sorted by the scheduler key; cluster[] non-decreasing.
 *   type i8, time i64, amp i32               instruction fields
 *   gid u32                                  run-wide instruction index (RNG stream id; shard independent)
 *   cluster i32                              time-cluster index within the batch (rawdata.py:61-63)
 *   tmin i64                                 scheduler key (time - z/v*[S2]) of the instruction
 *   p_hit f64                                S1: light yield (s1.py:125-131); S2: electron survival (s2.py:241-252)
 *   drift_mean/drift_spread f64              s2.py:158-179
 *   sc_gain f64                              s2.py:182-209
 *   cdf_row i32, cdf_table f64[n_cdf][n_tpc] cumulative channel probabilities (np.random.choice, s1.py:154, s2.py:673)
 *   run_set i32 (or NULL), n_run_sets       pulse set of every instruction: the instructions the reference hands to ONE
 *                                           Pulse call (rawdata.py:108-127; save_full_truth=False groups S1s within 100 ns
 *                                           and S2s within 2 mm).  Sets are numbered 0..n_run_sets-1; their instructions
 *                                           share cluster and type.  NULL: one set per instruction (the default).
 *                                           A set number may stay unused (its truth row is empty).  With n_run_sets = n
 *                                           and every set numbered by its FIRST instruction, an S2 that is alone in its
 *                                           set takes the tile-local generator like an S2 of a batch without run sets
 *                                           (electron afterpulses on: the primaries, next to the shared calls of the
 *                                           secondaries); with any other numbering no instruction does.
 *   em_base u32 (or NULL)                   offset of the instruction's emitter ids in the Philox counters: an electron-
 *                                           afterpulse instruction carries its parent's gid and (k + 1) << 20 for the k-th
 *                                           secondary of that parent (streams independent of batching / sharding) */
int wfs_load_instructions(wfs_handle *h, int64_t n, const int8_t *type, const int64_t *time, const int32_t *amp,
                          const uint32_t *gid, const int32_t *cluster, const int64_t *tmin,
                          const double *p_hit, const double *drift_mean, const double *drift_spread,
                          const double *sc_gain, const int32_t *cdf_row, const double *cdf_table, int32_t n_cdf,
                          const int32_t *run_set, int64_t n_run_sets, const uint32_t *em_base);

/* ---- model variants of the photon delays ---------------------------------------------------------------
 * S1.photon_timings (s1.py:162-238: 'custom' recoil models er / nr / alpha / led, s1.py:262-337) and S2.photon_timings
 * (s2.py:504-557: 'garfield' luminescence s2.py:380-411, optical propagation s2.py:486-502) add one more independent,
 * integer-truncated delay term per photon.  The host hands over that term's probability mass function; table k is the
 * convolution of pmf k (support vmin[k] .. vmin[k] + len - 1, pmf[pmf_off[k] .. pmf_off[k + 1])) with base[k]:
 *   0 transit time only, 1 the S1 terms of wfs_config, 2 the S2 terms, 3 the S2 terms without the 'simple' luminescence.
 * Call after wfs_set_tables; n_tables = 0 drops the tables. */
int wfs_set_delay_models(wfs_handle *h, int32_t n_tables, const int32_t *base, const int64_t *pmf_off, const double *pmf,
                         const int32_t *vmin);

/* S1 optical propagation (S1.optical_propagation, s1.py:241-260; the spline is a RegularGridInterpolator over (z, u),
 * load_resource.py:356-357): node values [nz][nu] for top- and bottom-array channels, the uniform u grid u0 + k * du.
 * The delay of a photon is trunc(multilinear interpolation at (z of the instruction, u)), u from the photon's stream. */
int wfs_set_s1_propagation(wfs_handle *h, int32_t nz, int32_t nu, double u0, double du, const double *top, const double *bottom);

/* Per instruction of the batch just loaded (wfs_load_instructions resets them): delay table of its photons on top-array
 * and on bottom-array channels (-1: the default table of the instruction type; tab_bottom NULL: same as tab), and for
 * S1 propagation the z cell of the spline grid and the normalised distance inside it (prop_zi -1 / NULL: none). */
int wfs_set_instruction_models(wfs_handle *h, int64_t n, const int32_t *tab, const int32_t *tab_bottom,
                               const int32_t *prop_zi, const double *prop_zf);
/* s2_luminescence_model 'garfield_gas_gap' (s2.py:413-483; resource s2_luminescence_gg, load_resource.py:284-291): the
 * excitation-time inverse CDFs timing_inv_cdf[n_gas_gaps][n_points] once; then per batch, for every instruction, the table at
 * or below the gas gap under it (np.digitize(gap, gas_gap) - 1; -1: the instruction does not use the model) and
 * (gap - gas_gap[table]) / spacing.  Every photon draws its excitation time from the interpolated table; the mean over the
 * instruction's photons is subtracted (s2.py:447) and the result truncated (s2.py:532).  Needs wfs_set_instruction_models
 * for the same batch (the remaining delay terms come from its tables, base 3). */
int wfs_set_gas_gap_model(wfs_handle *h, int32_t n_gas_gaps, int32_t n_points, const double *timing_inv_cdf);
int wfs_set_instruction_gas_gap(wfs_handle *h, int64_t n, const int32_t *table, const double *weight);

/* ---- pattern maps evaluated on the device ----------------------------------------------------------------
 * The hit pattern of an instruction is resource.s1_pattern_map(x, y, z) / s2_pattern_map(x, y) (s1.py:148, s2.py:640):
 * straxen InterpolatingMaps on a regular grid, method WeightedNearestNeighbors (load_resource.make_patternmap,
 * load_resource.py:403-435): inverse-distance weighted average of the 2 * dims nearest nodes, distances clipped at 1e-6.
 * which: 1 S1 map (3-D), 2 S2 map (2-D); nodes per axis, first / last node per axis; values f32[nodes][n_map_channels]
 * (row-major over the axes, PMT mask already applied).  n_map_channels < n_tpc: the missing (bottom) channels count 1
 * (s2.py:648-650).  Turned-off PMTs (gain 0) are removed on the device (s1.py:150, s2.py:653).  dims = 0 drops the map.
 * An instruction loaded with cdf_row = -1 takes its channel CDF from the map of its type: call wfs_eval_pattern_rows
 * with the positions (float32 as in instruction_dtype; z unused for S2) after wfs_load_instructions, before wfs_run.
 * wfs_copy_cdf_rows returns the rows the generator uses (parity tests feed them to the oracle). */
int wfs_set_pattern_map(wfs_handle *h, int32_t which, int32_t dims, const int32_t *n_nodes, const double *lo, const double *hi,
                        const float *values, int32_t n_map_channels);
int wfs_eval_pattern_rows(wfs_handle *h, int64_t n, const float *x, const float *y, const float *z);
/* The same for a map on an irregular coordinate system (a list of points: straxen queries a KD-tree for the 2 * dims
 * nearest points): points f64[n_points][dims], values f32[n_points][n_map_channels]. */
int wfs_set_pattern_map_points(wfs_handle *h, int32_t which, int32_t dims, int64_t n_points, const double *points,
                               const float *values, int32_t n_map_channels);
/* s2_aft_sigma / s2_aft_skewness (S2.photon_channels, s2.py:660-665): factor[i] = the skew-normal draw of instruction i
 * (NaN: leave the pattern alone); on the rows the device evaluates the top-array fraction cur becomes
 * new = clip(cur * factor, 0, 1), top channels are scaled by new / cur and the others by (1 - new) / (1 - cur).
 * Call between wfs_load_instructions and wfs_eval_pattern_rows; factor = NULL clears it. */
int wfs_set_instruction_aft(wfs_handle *h, int64_t n, const double *factor);
/* diffusion_constant_transverse with enable_field_dependencies['diffusion_transverse_map'] (S2.s2_pattern_map_diffuse,
 * s2.py:560-613): the pattern of an S2 instruction is the average of the pattern map over its surviving electrons, each
 * displaced by N(0, sigma_r[i]) along the radius and N(0, sigma_a[i]) across it (cm; sqrt(2 D t) from the field maps, NaN: not
 * this path); electrons that end outside tpc_radius do not count.  Evaluated inside wfs_run, behind the electron survival
 * draws.  Needs the S2 pattern map as a regular grid (wfs_set_pattern_map) and the instruction loaded with cdf_row = -1;
 * call between wfs_load_instructions and wfs_eval_pattern_rows (which still supplies the positions). */
int wfs_set_instruction_diffusion(wfs_handle *h, int64_t n, const double *sigma_r, const double *sigma_a, double tpc_radius);

/* ---- scalar maps evaluated on the device -------------------------------------------------------------------
 * The per-instruction inputs of the generator that the reference reads from straxen InterpolatingMaps: S1 light yield
 * (resource.s1_lce_correction_map, s1.py:125), S2 correction / single-electron gain (s2.py:193-196, 229-234), longitudinal
 * diffusion (s2.py:170), field-distortion corrections (s2.py:41), all WeightedNearestNeighbors on a regular grid
 * (wfs_scalar_map_grid) or a point list (wfs_scalar_map_points); and the field-dependence / COMSOL maps, which
 * load_resource.py:316,326 builds with method RectBivariateSpline (wfs_scalar_map_spline: the knots tx[nx], ty[ny], degrees
 * and coefficients c[(nx-kx-1)*(ny-ky-1)] of scipy's spline object; evaluated like its .ev(): FITPACK bispeu, arguments
 * clamped to the knot range).  Each call registers a map for the lifetime of the handle and returns its id.
 * wfs_scalar_map_eval: pos f64[n][dims] -> out f64[n].  Tolerance against the host evaluation: rtol 1e-6 (different
 * summation order; the nearest neighbours of a position equidistant to several nodes may be chosen differently). */
int wfs_scalar_map_grid(wfs_handle *h, int32_t dims, const int32_t *n_nodes, const double *lo, const double *hi,
                        const double *values, int32_t *map_id);
int wfs_scalar_map_points(wfs_handle *h, int32_t dims, int64_t n_points, const double *points, const double *values, int32_t *map_id);
int wfs_scalar_map_spline(wfs_handle *h, int32_t nx, const double *tx, int32_t ny, const double *ty, int32_t kx, int32_t ky,
                          const double *c, int32_t *map_id);
int wfs_scalar_map_eval(wfs_handle *h, int32_t map_id, int64_t n, const double *pos, double *out);
/* The other shapes make_map / InterpolatingMap can take (load_resource.py:357, 383-401): array-valued maps -- n_values entries per node,
 * values f64[nodes][n_values], WeightedNearestNeighbors on a grid or a point list -- and method 'RegularGridInterpolator' on a regular
 * grid (wfs_scalar_map_linear: scipy's multilinear interpolation with bounds_error=False, fill_value=None, i.e. the edge cell's plane
 * continued outside the grid; scalar or array-valued).  wfs_scalar_map_eval_array: pos f64[n][dims] -> out f64[n][n_values];
 * n_values must be the map's (wfs_scalar_map_eval is the n_values = 1 form).  Tolerance as above (multilinear: rtol 1e-12). */
int wfs_scalar_map_grid_array(wfs_handle *h, int32_t dims, const int32_t *n_nodes, const double *lo, const double *hi,
                              const double *values, int32_t n_values, int32_t *map_id);
int wfs_scalar_map_points_array(wfs_handle *h, int32_t dims, int64_t n_points, const double *points, const double *values,
                                int32_t n_values, int32_t *map_id);
int wfs_scalar_map_linear(wfs_handle *h, int32_t dims, const int32_t *n_nodes, const double *lo, const double *hi,
                          const double *values, int32_t n_values, int32_t *map_id);
int wfs_scalar_map_eval_array(wfs_handle *h, int32_t map_id, int64_t n, const double *pos, double *out, int32_t n_values);
int wfs_copy_cdf_rows(wfs_handle *h, int32_t *cdf_row, double *cdf_table, int64_t cap_rows);

/* Order of the packed records of a batch: 0 (default) as the reference yields pulses (window, channel, interval,
 * rawdata.py:282-311); 1 as strax.sort_by_time leaves them in ChunkRawRecords.final_results (strax_interface.py:453):
 * by (time, channel) -- the windows of a batch do not overlap in time, so they stay contiguous.  Sorted on the device. */
int wfs_set_record_order(wfs_handle *h, int32_t by_time);

/* Parity entry: photons supplied instead of generated -- what RawDataOptical.sim_primary hands to Pulse
 * (rawdata.py:475-493) and what the golden vectors inject.  One "pulse set" = one Pulse.__call__ (pulse.py:39).
 *   set_cluster i32[n_sets], set_tmin i64[n_sets]   cluster id and scheduler key of the set's instruction
 *   set_off i64[n_sets+1]                           photon ranges; inside a set photons are sorted by channel
 *   t i64 (post transit-time spread), ch i16, gain f64 (pulse.py:97-107), dpe u8 */
int wfs_load_photons(wfs_handle *h, int64_t n_sets, const int32_t *set_cluster, const int64_t *set_tmin,
                     const int64_t *set_off, const int64_t *t, const int16_t *ch, const double *gain,
                     const uint8_t *dpe);

/* Optical input: replaces RawDataOptical.sim_primary (rawdata.py:475-493).  One pulse set per instruction; its photons
 * are channels[first[i]:last[i]] / timings[...] (ns relative to the instruction), cut to 0 <= t < time_cutoff
 * (nveto_time_max_cutoff).  Transit time spread, double-PE and SPE gains are drawn on the GPU (Pulse.__call__). */
int wfs_load_optical(wfs_handle *h, int64_t n, const int64_t *time, const uint32_t *gid, const int32_t *cluster,
                     const int64_t *tmin, const int32_t *first, const int32_t *last,
                     const int32_t *channels, const int64_t *timings, int64_t n_photons, int64_t time_cutoff);

/* State carried across batches: RawData.last_pulse_end_time (rawdata.py:55, 188-190), the running maximum of the end of
 * every pulse simulated so far, which decides whether the first clusters of this batch open a new digitise window. */
int wfs_set_window_carry(wfs_handle *h, int32_t has_pulse, int64_t last_pulse_end_time);

/* ---- run: replaces RawData.__call__ for the loaded batch (rawdata.py:38-157) ---------------------------- */
/* Stages: S1/S2 photon generation (s1.py:60-114, s2.py:73-136) [skipped after wfs_load_photons] ->
 * Pulse.__call__ + add_current (pulse.py:39-144, 276-318) -> digitize_pulse_cache (rawdata.py:204-272) ->
 * ZLE (rawdata.py:274-311) -> record packing (strax_interface.py:391-436).  Asynchronous on the handle's
 * stream except for the size read-backs between stages. */
int wfs_run(wfs_handle *h);

/* n_pulse_sets: rows of the per-set outputs (wfs_copy_truth, wfs_copy_truth_per_pmt, wfs_copy_electron_stats; set offsets of
 * wfs_copy_photons) = n_run_sets as given to wfs_load_instructions, unused set numbers included (their rows are empty), twice that with
 * PMT afterpulses (the afterpulse set of set q is n_run_sets + q).  n_raw_samples: samples of every digitised row, whichever way it was
 * made (accumulators, tile buffer read in place, resident row).  n_rows and n_raw_samples include the bottom-array sum rows
 * (wfs_set_sum_signal). */
typedef struct wfs_counts {
    int64_t n_instructions, n_pulse_sets, n_emitters, n_photons /* primary + PMT afterpulse */, n_pe, n_tiles, n_groups, n_rows,
            n_raw_samples, n_intervals, n_records;
} wfs_counts;
int wfs_get_counts(wfs_handle *h, wfs_counts *out);

/* Electron afterpulses need, per parent S2, the number of detected photons and the arrival times of randomly chosen ones
 * (afterpulse.py:37-47, 106-121: len(signal_pulse._photon_timings), _photon_timings[randint]).
 * off[n + 1]: first generated photon of every instruction (generation order: instruction by instruction; inside an instruction of
 * the per-electron generator emitter by emitter, inside a tile-generated one (wfs_config.tile_gen) tile by tile -- channel ascending,
 * photon q of a tile at position q); index: photons in that numbering, t_out: their arrival times in ns (recomputed from the photon's
 * own draws, so the answer does not depend on the order inside the channel buckets -- and, for tile-generated instructions, not on
 * any photon having been generated: debug bit 2 without bit 4 only draws the tiles' photon numbers).  After wfs_run (also with debug bit 2). */
int wfs_copy_instruction_photon_offsets(wfs_handle *h, int64_t *off, int64_t capacity);
int wfs_gather_photon_times(wfs_handle *h, int64_t n, const int64_t *index, int64_t *t_out);

/* Per-PMT truth (config 'per_pmt_truth', pulse.py:61-66, 268-269): acc6[set][channel][6] = n_photon, n_pe, n_photon_trigger,
 * n_pe_trigger, raw_area, raw_area_trigger of every pulse set and TPC channel.  cap = sets the buffer holds. */
int wfs_copy_truth_per_pmt(wfs_handle *h, double *acc6, int64_t cap);

/* ---- results (host copies) ---------------------------------------------------------------------------- */
/* Every copy-out returns WFS_E_STATE until wfs_run has come to its end for the loaded batch, and again after a per-instruction
 * option of the batch or the delay tables changed.  wfs_copy_groups, wfs_copy_intervals, wfs_copy_rows, wfs_copy_row_data and
 * wfs_copy_sum_signal are decoded with the row layout of the device view (row slots per window, HE rows, sum channel, noise
 * channels): when a wfs_set_* call changes that layout after the run (wfs_set_tables, wfs_set_noise_float, wfs_set_noise_model,
 * wfs_set_sum_signal), these five return WFS_E_STATE until the next wfs_run; the others still read the last run. */
/* raw_records, 244-byte packed strax layout, in the order the reference yields them (group, channel, interval,
 * fragment); dst may be a host or a device pointer (wfs_copy_records_dev). */
int wfs_copy_records(wfs_handle *h, void *dst_host, int64_t capacity_records);
/* the records [first, first + count) of the batch into a caller buffer (e.g. straight into the chunker's record buffer) */
int wfs_copy_records_range(wfs_handle *h, void *dst, int64_t first, int64_t count);
/* The same without waiting: the copy runs on the handle's copy stream and overlaps the kernels of the next wfs_run (the
 * engine keeps the records of the last two batches); dst should be pinned (wfs_host_register: e.g. the chunker's record
 * buffer, strax_interface.py:360-364, registered once) -- from pageable memory the driver stages the copy and nothing
 * overlaps.  wfs_wait_records returns when every copy issued so far has landed. */
int wfs_copy_records_range_async(wfs_handle *h, void *dst, int64_t first, int64_t count);
int wfs_wait_records(wfs_handle *h);
int wfs_host_register(void *ptr, int64_t bytes);
int wfs_host_unregister(void *ptr);
int wfs_copy_records_dev(wfs_handle *h, void *dst_dev, int64_t capacity_records);
/* The records of the last run in device memory.  wfs_run returns once the counts are known; the records are packed on a stream of the
 * handle's own, under the front end of the next wfs_run.  The bytes behind this pointer are complete after wfs_synchronize or after
 * any of the record copy calls above (the asynchronous one: after wfs_wait_records); until then they may still be written. */
const void *wfs_records_dev_ptr(wfs_handle *h);
/* digitise windows: rawdata.left / rawdata.right and the first record of each window (strax_interface.py:394-399) */
int wfs_copy_groups(wfs_handle *h, int64_t *left, int64_t *right, int64_t *first_record, int64_t *ix_rand);
/* digitise window of every time-cluster of the batch (rawdata.py:96-98 decided on the GPU) */
int wfs_copy_cluster_groups(wfs_handle *h, int32_t *group, int64_t capacity_clusters);
/* ZLE intervals (channel, left, right) and their samples: the tuples RawData.__call__ yields (rawdata.py:311) */
int wfs_copy_intervals(wfs_handle *h, int32_t *group, int32_t *channel, int64_t *left, int64_t *right,
                       int64_t *data_off, int64_t capacity);
int wfs_copy_interval_data(wfs_handle *h, int16_t *data, int64_t capacity);
/* pulses (tiles): channel, left, right, photons, and the f64 currents (pulse.py:138-144) -- parity/debug */
int wfs_copy_pulses(wfs_handle *h, int32_t *set, int32_t *channel, int64_t *left, int64_t *right,
                    int64_t *n_photons, int64_t *cur_off, int64_t capacity);
int wfs_copy_currents(wfs_handle *h, double *cur, int64_t capacity);   /* needs wfs_set_debug(h, 1) before wfs_run */
/* digitised rows in their active range (rawdata.py:258-259) -- parity/debug */
int wfs_copy_rows(wfs_handle *h, int32_t *group, int32_t *channel, int64_t *left, int64_t *right,
                  int64_t *data_off, int64_t capacity);
int wfs_copy_row_data(wfs_handle *h, int32_t *data, int64_t capacity);
/* generated photons per pulse set, channel sorted: t i64, ch i16, gain f64, dpe u8 (after wfs_run) */
int wfs_copy_photons(wfs_handle *h, int64_t *set_off, int64_t *t, int16_t *ch, double *gain, uint8_t *dpe,
                     int64_t capacity);
/* truth accumulators per pulse set: 12 f64 (n_photon n_pe n_photon_trigger n_pe_trigger raw_area raw_area_trigger,
 * then the same for the bottom array; pulse.py:229-271) + photon time stats (n, mean, min, max, std; rawdata.py:325-332) */
int wfs_copy_truth(wfs_handle *h, double *acc12, double *tstat5, int64_t capacity_sets);
/* electron arrival-time statistics per run set (= per instruction by default): n, mean, min, max, std over the electrons of
 * all its instructions (rawdata.py:325-341; NaN when there are none) */
int wfs_copy_electron_stats(wfs_handle *h, double *estat5, int64_t capacity_sets);

/* ---- instrumentation ---------------------------------------------------------------------------------- */
/* flags: bit 0 keep f64 tile currents and finished rows for wfs_copy_currents / wfs_copy_rows; bit 1 send every tile
 * to the dense pulse kernel (both kernels give the same bits; used by the parity tests); bit 2 wfs_run stops after the
 * photon generation (enough for wfs_copy_set_photon_counts / wfs_gather_photon_times: the electron-afterpulse pre-pass);
 * bit 3 check every kernel launch on the spot (hipGetLastError + stream synchronisation after each one: a failed launch or a
 * faulting kernel is reported under its own name by wfs_run; slow, for debugging); bit 4 the photons of tile-generated instructions
 * (wfs_config.tile_gen) are also stored for wfs_copy_photons -- by default they only ever exist in registers */
int wfs_set_debug(wfs_handle *h, int32_t flags);
/* parity tests: noise start index per digitise window (rawdata.py:417) instead of the Philox draw; entries < 0 keep the draw.
 * Indexed by the window number of wfs_copy_groups (host pointer, copied). n = 0 clears the override. */
int wfs_set_noise_offsets(wfs_handle *h, const int64_t *ix_rand, int64_t n);
/* A noise array of floats, f64[noise_len][noise_channels] (call after wfs_set_tables; replaces its int16 table): add_noise
 * (rawdata.py:436, numba) adds noise_data[ix, ch] into the int64 row, which stores the truncated SUM. */
int wfs_set_noise_float(wfs_handle *h, const double *noise, int32_t noise_len, int32_t noise_channels);
/* The noise model: digitiser noise drawn per sample on the device instead of replayed from the noise array (white noise only).
 * pmf f64[n_channels][n_values]: per channel the probability of the ADC offsets vmin .. vmin + n_values - 1.  For the row sample with
 * absolute index t (record time t * dt) of channel ch < n_channels -- TPC, HE and sum channel are channels of their own --
 *     w[4] = philox4x32_10(counter (low 32 bits of t >> 2, high 32 bits of t >> 2, ch, 65), key = seed)      (arithmetic shift)
 *     noise(ch, t) = vmin + Walker draw from the channel's alias cells with the 32-bit word w[t & 3]
 * (cell c = word >> shift; value c if (word << (32 - shift)) < thr[c], else alias[c]): the value depends on (seed, ch, t) alone,
 * whichever kernel, window or batch holds the sample.  It is added where the noise array is (after the HE / sum factor, before
 * baseline and clamp) and channels >= n_channels get none (rawdata.py:421).  With a model set and wfs_config.enable_noise on no
 * noise start index is drawn (wfs_copy_groups reports 0), wfs_set_noise_offsets is accepted without effect and the noise array of
 * wfs_set_tables, if any, is not read; with enable_noise off no noise is added.  n_channels = 0 clears the model: the noise array is
 * back.  WFS_E_INVALID: n_channels > n_rows, n_values outside 1 .. 4096, values outside int16, a negative entry, a row whose sum
 * differs from 1 by more than 1e-9.  Takes effect from the next wfs_run. */
int wfs_set_noise_model(wfs_handle *h, int32_t n_channels, int32_t n_values, int32_t vmin, const double *pmf);
/* noise(channel, t0 .. t0 + n - 1) of the model (with its colour, if one is set), evaluated on the device (n <= 2^30).  WFS_E_STATE
 * without a model. */
int wfs_noise_model_samples(wfs_handle *h, int32_t channel, int64_t t0, int64_t n, int16_t *out);
/* A colour for the noise model: every stream r -- the model's n_channels channels, then n_groups common streams -- is a white
 * sequence w(r, t) drawn as above (common stream g under the counter of "channel" g at site 66, from cells built of
 * common_pmf[g][n_values] over the model's values) and run through the FIR taps_q[r][n_taps] (Q16, 65536 = 1.0):
 *   F(r, t) = sum_k taps_q[r][k] w(r, t - k)
 *   noise(ch, t) = (F(ch, t) + ((int64) mix_q[ch] * F(n_channels + group[ch], t) >> 16) + 32768) >> 16      (group[ch] = -1: no common part)
 * in exact integer arithmetic.  Needs a model (WFS_E_STATE without one); wfs_set_noise_model clears the colour; n_taps = 0 clears it
 * and the white values return.  WFS_E_INVALID, with the argument named: n_taps outside 1 .. 16; a row of taps_q with
 * sum |taps_q| * max(|vmin|, |vmin + n_values - 1|) >= 2^29; group outside -1 .. n_groups - 1; |mix_q| > 65536; a row of common_pmf
 * that has a negative entry or does not sum to 1 within 1e-9.  group, mix_q and common_pmf may be null with n_groups = 0.  With
 * n_taps = 1, taps_q = 65536 and no groups the values are those of the white model. */
int wfs_set_noise_colour(wfs_handle *h, int32_t n_taps, const int32_t *taps_q, int32_t n_groups, const int32_t *group, const int32_t *mix_q,
                         const double *common_pmf);
/* The white sequence w(row, t0 .. t0 + n - 1) of a stream: row < n_channels a channel, n_channels + g common stream g. */
int wfs_noise_white_samples(wfs_handle *h, int32_t row, int64_t t0, int64_t n, int16_t *out);
/* Slow levels for the noise model, with or without a colour: baseline motion with memory far beyond the taps.  Level j of
 * stream r (rows as for taps_q) is a sequence of knots 2^shifts[j] samples apart, joined by linear interpolation:
 *   knot(r, j, m) = a draw from the stream's own cells with word m & 3 of the Philox call of (m >> 2, channel at site 80 + j | group at
 *                   site 96 + j)
 *   m = t >> shifts[j], f = t & (2^shifts[j] - 1), P0 = slow_q[r][j] knot(r, j, m), P1 = slow_q[r][j] knot(r, j, m + 1)
 *   S(r, t) = sum_j P0 + (((int64) (P1 - P0) * f) >> shifts[j])                                  (Q16, arithmetic shifts)
 * and F(r, t) + S(r, t) takes the place of F(r, t) above; without a colour F(r, t) = 65536 w(r, t) and there are no common streams.
 * slow_q: [n_channels + n_groups][n_levels], Q16.  Needs a model (WFS_E_STATE without one); n_levels = 0 clears the levels, and so do
 * wfs_set_noise_model and wfs_set_noise_colour (set the colour first).  WFS_E_INVALID, with the argument named: n_levels outside
 * 0 .. 8; a shift outside 4 .. 30 or shifts not strictly ascending; a row with
 * (sum |taps_q| + sum |slow_q|) * max(|vmin|, |vmin + n_values - 1|) >= 2^29 (sum |taps_q| = 65536 without a colour).  With all
 * amplitudes zero the values are those of the model without the levels. */
int wfs_set_noise_slow(wfs_handle *h, int32_t n_levels, const int32_t *shifts, const int32_t *slow_q);
/* S(row, t0 .. t0 + n - 1) in Q16: row < n_channels a channel, n_channels + g common stream g.  WFS_E_STATE without slow levels. */
int wfs_noise_slow_samples(wfs_handle *h, int32_t row, int64_t t0, int64_t n, int32_t *out);
/* The alias cells of a channel as the device holds them: thr[n_cells], alias[n_cells] (n_cells = 2^k >= max(2, n_values), the same for
 * every channel), shift = 32 - k and vmin.  capacity_cells: entries the two buffers hold. */
int wfs_copy_noise_model(wfs_handle *h, int32_t channel, uint32_t *thr, uint32_t *alias, int32_t capacity_cells, int32_t *n_cells,
                         int32_t *shift, int32_t *vmin);
int wfs_set_stream(wfs_handle *h, void *hip_stream);
int wfs_synchronize(wfs_handle *h);
/* Tiles of tile-generated S2s above 2048 photons whose H table fits the LDS of one workgroup are drawn and turned into their pulse by
 * one kernel, without a photon array (k_s2_bright; config 'tile_local_bright').  on = 0: they take the generation-only kernel and the
 * dense pulse kernel, as every bright tile that does not fit.  Results do not depend on it.  Default: on. */
int wfs_set_bright_tiles(wfs_handle *h, int32_t on);
/* The bottom-array sum channel (row channel_map['sum_signal'] = 800 of the reference's digitiser array, rawdata.py:250-254, which the
 * reference fills at every digitisation and never emits).  on = 1, detector XENONnT: every digitise window with at least one pulse on
 * a bottom-array channel (n_top <= channel <= last_bottom) gets one more row on channel wfs_config.sum_channel, behind its TPC and HE
 * rows: S[t] = int(he_factor) * sum over those pulses of their rounded ADC wave, carried in 64 bits (stored in 32 bits it saturates,
 * which no finished sample can show: such a value clamps to 0), from min(pulse left) - trigger_window to max(pulse right) +
 * trigger_window.  The row is finished, zero-suppressed and packed like every other row: noise from column sum_channel of the noise
 * array when it has one, baseline, clamp at 0, ZLE threshold thr_zle[sum_channel].  It takes no part in the window's left / right or
 * in its noise draw; truth is unchanged.  wfs_copy_rows / wfs_copy_intervals list it under channel = sum_channel.  With the switch on,
 * bottom-array rows are kept off the resident-row path (wfs_config.row_resident); the records of every other channel are the same.
 * Takes effect from the next wfs_run.  on = 1 needs sum_channel < n_rows, outside the TPC and the HE channels (WFS_E_INVALID
 * otherwise); other detectors accept the switch and never have the row.  Default: off -- no kernel, no buffer, no record differs. */
int wfs_set_sum_signal(wfs_handle *h, int32_t on);
/* Parity entry: the sum rows of the last wfs_run before they are finished (a clamped finished row cannot be turned back into S).  Per
 * row, in window order: its window (index of wfs_copy_groups), absolute first and last sample, and S[t] (times int(he_factor)) at
 * data[data_off[k] .. data_off[k + 1]); data_off[rows] is written when capacity_rows exceeds the number of rows. */
int wfs_copy_sum_signal(wfs_handle *h, int32_t *group, int64_t *left, int64_t *right, int64_t *data_off, int64_t *data,
                        int64_t capacity_rows, int64_t capacity_samples);
/* Full readout (config 'full_readout'): every digitise window is read out on every channel, not only on those that hold a
 * pulse.  A digitise window is still one with at least one pulse, and its left / right, its noise start index, the truth and the order
 * of the Pulse calls do not change.  With the switch on every TPC row slot of such a window has a row, and every HE slot when HE rows
 * exist, channels with gain 0 or turned off included (optical / nVeto input: every channel of the array).  Every one of these rows
 * has the range of the window's union mask, min(left) - trigger_window .. max(right) + trigger_window over ALL pulses of the window:
 * the range the row would have if a pulse reached both extremes on that channel.  Its value is the sum of the channel's pulses, zero
 * where it has none (an HE slot: its top channel's sum times int(he_factor)), finished by the rule of every row: the configured noise
 * (a table: sample i of the row reads index ix_rand + i; the model: its value at the absolute sample), baseline, clamp; channels at
 * or beyond the noise source's channel count get no noise.  Zero-length encoding and record fragments are those of every row, with
 * thr_zle[channel]; there is no separate "no suppression" switch: a threshold no sample can reach (zle_threshold below -2^15) stores
 * whole rows.  The sum row (wfs_set_sum_signal) keeps its range and value.  Records of a window: ascending channel, TPC, HE, sum (or
 * by time and channel, wfs_set_record_order).  wfs_counts.n_rows and n_intervals count what exists; n_raw_samples does not count rows
 * without a pulse, which never exist unfinished.  wfs_copy_rows / wfs_copy_row_data (debug) list the rows WITH pulses, at their full
 * range; wfs_copy_intervals and the records are the contract for the others.  Allowed between runs; waits for pending packers when
 * the mode changes; takes effect from the next wfs_run.  A batch whose rows without a pulse need more finished samples than one batch
 * may hold (2^36, WFS_FULL_READOUT_MAX_SAMPLES) ends in WFS_E_CAPACITY, one the device has no memory for in WFS_E_NOMEM, both with a
 * message that names full readout.  Default: off -- no kernel, no buffer, no record differs. */
int wfs_set_full_readout(wfs_handle *h, int32_t on);
/* PMT dark counts (config 'dark_count_rate'): single-electron pulses a PMT makes on its own, drawn on the device as a pure
 * function of (seed, channel, absolute time) and added where a sample is finished.  rate_hz: [n_channels] in Hz, n_channels <= n_tpc.
 * Definition -- dt the sample duration, tlen the template length, before = samples_before, L = 64 samples in a cell, m the cell index
 * of a channel's absolute sample axis (cell m holds the samples 64 m .. 64 m + 63; m may be negative, shifts are arithmetic):
 *   count   w = philox4x32_10(counter (low 32 bits of m, high 32 bits of m, ch, 112), key = seed);
 *           n(ch, m) = sum_{k = 1 .. 4} [w[0] < T[ch][k]], T[ch][k] = floor(2^32 P(N >= k)), N ~ Poisson(mu_ch), mu_ch = rate_ch L dt 1e-9;
 *           the tails are summed as the series sum_{i >= k}.  mu_ch <= 1/8: the mass above 4, below 2.6e-7, is folded into 4.
 *   photon  j < n: the call at site 113 + (j >> 1), same first three counter words, words a = 2 (j & 1) and a + 1:
 *           t_ns = m L dt + (((u64) w[a] (L dt)) >> 32); gain = gains[ch] * spe[row of ch][(((u64) w[a + 1] * 2000) >> 32) + 1], a single
 *           PE always (the first index of the gain draw of every photon): a thermionic electron is one electron.
 *   pulse   idx = t_ns div dt, r = t_ns mod dt (floor): samples idx - before + k, k < tlen, value round(gain templates[r][k] c2a), negated
 *           as every pulse is, each photon rounded on its own, like a pulse of its own.
 *   row     D(ch, t) = the sum of these values over the channel's dark photons that reach sample t;  acc' = acc + D(pmt channel of the
 *           slot, row_abs + i) in front of everything else: an HE slot gets its top channel's D times int(he_factor), noise, baseline
 *           and clamp follow unchanged.  A channel with rate 0 or gain 0 gets nothing, nor does one at or beyond n_channels.
 * The sum row (wfs_set_sum_signal) carries no dark counts.  Windows, row ranges, ix_rand, truth, the order of the Pulse calls and the
 * record order do not change: a dark pulse shows where a row is read out, its tail too when it began in front of the row; outside
 * the rows of a run a dark photon is read out by wfs_lone_hits alone.  n_channels = 0 clears; rates that are all zero are the
 * feature off.  WFS_E_INVALID, with the argument named: n_channels > n_tpc, a negative or non-finite rate, mu > 1/8.  Takes effect
 * from the next wfs_run; waits for pending packers.  Default: off -- no kernel, no buffer, no record differs. */
int wfs_set_dark_counts(wfs_handle *h, int32_t n_channels, const double *rate_hz);
/* D(channel, t0 .. t0 + n - 1), evaluated on the device (n <= 2^30, |t0| <= 2^48).  WFS_E_STATE without rates or tables. */
int wfs_dark_count_samples(wfs_handle *h, int32_t channel, int64_t t0, int64_t n, int32_t *out);
/* The dark photons of a channel whose start sample idx lies in [t0, t0 + n), in time order (equal times: in the order of j): the truth
 * does not hold them, this is how a hit is matched to a dark count.  *count: how many there are; more than capacity: WFS_E_CAPACITY
 * (the first `capacity` are written). */
int wfs_dark_count_photons(wfs_handle *h, int32_t channel, int64_t t0, int64_t n, int64_t *t_ns, double *gain, int64_t capacity, int64_t *count);
/* The thresholds T[channel][1 .. 4] as the device holds them.  WFS_E_STATE without rates. */
int wfs_copy_dark_counts(wfs_handle *h, int32_t channel, uint32_t thr[4]);
/* Lone-hit rows (config 'dark_count_lone_hits'): the dark photons outside the rows of a run, read out in rows of their own;
 * with wfs_set_lone_noise_hits (below) the samples of the noise model that cross their threshold there are seeds of such rows too.
 * start = idx - before is the first sample of a dark photon's pulse, G = tlen + 2 tw.
 *   lone     a dark photon of PMT channel ch whose pulse samples start .. start + tlen - 1 lie in no row of ch's TPC slot.  Rows: those
 *            of the last completed wfs_run at their final range (every channel of a window under full readout), none when no run is
 *            complete.  HE slots and the sum row get no lone rows.
 *   row      the lone photons of a channel in time order; a maximal chain whose consecutive starts are at most G apart is one row of
 *            range first start - tw .. last start + tlen - 1 + tw, clipped so that it reaches no sample of a row of the channel.
 *   content  D(ch, t) over the range (every dark photon that reaches a sample), finished like every row: noise (kinds 3 - 5 at the
 *            absolute sample; tables at index ix_rand + i, ix_rand = ((u64) w[0] noise_len) >> 32, w = philox4x32_10(counter (low, high
 *            32 bits of the row's first sample, ch, 115))), baseline, clamp; ZLE with thr_zle[ch], hold-off, even landing, fragments.
 *   owner    the pass over the absolute samples [s0, s1) owns the rows whose first photon starts there; it looks back G samples in front
 *            of s0 and follows a chain beyond s1, but takes no photon that starts at or behind s_limit >= s1 and ends the row at
 *            s_limit - 1 at the latest (what such a chain holds beyond s_limit is read out by no pass).  However [s0, s1) is split into
 *            passes of one s_limit, the records are the same.
 * The windows of the run must lie more than G samples apart (WFS_E_STATE otherwise).  The pass has buffers of its own, runs behind the
 * packers of the batch and leaves that batch's records as they are; it returns when its records exist.  *n_records: how many.
 * WFS_E_STATE without tables, and without rates unless noise hits are on; WFS_E_INVALID for s1 < s0, s_limit < s1 or a range beyond 2^48; WFS_E_CAPACITY, with a message
 * that names lone hits, for a pass of more than 2^40 samples, 2^34 cells (channels x 64-sample cells), 2^31 seeds (lone photons and
 * noise hits), 2^24 rows or 2^31 records, or a lone row of more than 2^19 samples (a chain of dark photons, or noise that stays across
 * the threshold). */
int wfs_lone_hits(wfs_handle *h, int64_t s0, int64_t s1, int64_t s_limit, int64_t *n_records);
/* The records of the last pass in (time, channel) order, in the layout of wfs_copy_records.  capacity: records the buffer holds. */
int wfs_copy_lone_records(wfs_handle *h, void *dst, int64_t capacity);
/* The rows of the last pass in (channel, time) order: channel, first and last sample, ix_rand (0 without a noise table) and the number
 * of lone photons of the chain (the photons themselves: wfs_dark_count_photons; noise-hit seeds are not counted here).  *count: how
 * many rows; more than capacity: WFS_E_CAPACITY and nothing is written. */
int wfs_copy_lone_rows(wfs_handle *h, int32_t *channel, int64_t *left, int64_t *right, int64_t *ix_rand, int32_t *n_photons, int64_t capacity, int64_t *count);
/* Noise-hit seeds of the lone-hit passes (config 'noise_lone_hits').  Symbols as above.
 *   value    v(ch, t) is the finished sample a row without a pulse would hold at absolute sample t: finish_value<NK>(d, D(ch, t), he =
 *            false, noisy = ch < model channels, noise(ch, t)), D = 0 where no dark-count rate is set.  Defined for the drawn noise kinds
 *            3, 4 and 5 alone: a noise table has no value at an absolute sample.
 *   seed     a sample t of a PMT channel ch inside the noise model is a noise-hit seed when v(ch, t) < thr_zle[ch] -- the very comparison
 *            the ZLE kernels make -- and t lies in no row of ch's TPC slot (under full readout every channel of a window has a row).
 *            The seed's start is t itself, not t - before: a seed directly behind a row must start behind that row, or the clipping of
 *            the range does not see the row.  A photon is lone when its whole pulse is clear of the rows; a seed needs only its own
 *            sample to be clear.  What made the sample cross -- noise alone, the tail of a dark pulse that is not lone, both together --
 *            does not matter.
 *   rows     the seeds of a channel are its lone dark photons (the rule above, if rates are set) and its noise-hit seeds, merged by
 *            start; from there on everything above applies without change: a maximal chain with consecutive starts at most G apart is
 *            one row of range first start - tw .. last start + tlen - 1 + tw, clipped against the row in front, the row behind and
 *            s_limit; content D finished like every row; ZLE, hold-off, even landing, 110-sample fragments, ownership by the first
 *            seed's start in [s0, s1) and the look-back of G samples as before.  Two seeds on the two sides of a row of length len >= G
 *            start at least len + 1 > G apart: a chain straddles no row.
 * Every noise-hit seed is a hit of the row that holds it, so it lies inside exactly one stored interval of its channel.  A dark pulse
 * that crosses the threshold contributes its crossing samples as seeds: the first start of a chain does not move, the last can move by
 * up to tlen - 1 samples, so a row can be that much longer than under dark_count_lone_hits alone.  No HE rows, no sum-row entries, no
 * truth.  A pass needs no dark-count rates then (noise only).  on != 0: WFS_E_STATE without a drawn noise model (wfs_set_noise_model)
 * or with enable_noise off; wfs_set_noise_model(h, 0, ..) switches it off.  Default: off -- no kernel, no buffer, no record differs. */
int wfs_set_lone_noise_hits(wfs_handle *h, int32_t on);
/* The noise-hit seeds of every row of the last pass, in the row order of wfs_copy_lone_rows.  *count: how many rows; more than capacity:
 * WFS_E_CAPACITY and nothing is written. */
int wfs_copy_lone_row_noise_hits(wfs_handle *h, int32_t *n_noise_hits, int64_t capacity, int64_t *count);
/* The overlay pass (config 'overlay_records'): two streams of 244-byte raw_records merged per channel into one valid stream.
 *   A        the simulation's stream: sim_host[n_sim], or with sim_host = NULL the records of the last wfs_run where the device holds
 *            them (WFS_E_STATE before a run has completed; the batch's own records keep every byte) -- all of them with n_sim < 0,
 *            else the first n_sim in the order of wfs_copy_records (the windows of a batch that its caller emits are a prefix).
 *   B        the recorded background: bg_host[n_bg].
 *   pulse    the fragments record_i = 0 .. k of one (channel, time0); it covers the samples time0 / dt .. time0 / dt + pulse_length - 1.
 *   valid    dt == cfg.dt, time % dt == 0, 1 <= length <= 110, 0 <= channel < n_rows; the fragments of every pulse complete, 110 dt
 *            apart, with the lengths of their place; no two pulses of ONE stream share a sample on a channel.  Otherwise WFS_E_INVALID
 *            with a message that names the first offending record, and nothing of it is read out of range.
 *   merging  per channel, pulses of A and B that share a sample become one pulse, transitively; pulses that only touch stay apart.
 *   sample   covered by B alone: b; by A alone: clamp(a - cfg.baseline + base[ch]); by both: clamp(b + a - cfg.baseline), clamped to
 *            0 .. 32767.  base = bg_baseline, int32[n_rows], the recorded baseline per channel; NULL: cfg.baseline everywhere.
 *   output   fragments of 110 samples again, samples behind length 0, baseline 0, ordered by (time, channel).  B empty (and base NULL)
 *            gives A sorted, A empty gives B sorted, byte for byte.
 * The pass has buffers of its own, allocated by its first call, and runs behind the packers of the last run.  WFS_E_CAPACITY, with a
 * message that names the overlay: more than 2^31 records in or out, a merged pulse beyond 2^31 - 1 samples, or a span of samples that
 * does not fit the sort keys beside the channel and the stream (63 bits in all).  *n_records: the records of the merged stream. */
int wfs_overlay_records(wfs_handle *h, const void *sim_host, int64_t n_sim, const void *bg_host, int64_t n_bg, const int32_t *bg_baseline, int64_t *n_records);
/* The records of the last pass; dst is a host or a device pointer. */
int wfs_copy_overlay_records(wfs_handle *h, void *dst, int64_t capacity_records);
/* Which kernel made every primary (pulse set, channel) tile of the last wfs_run, indexed set * n_tpc + channel: 0 no photons or not
 * tile-generated, 1 photons and pulse in one workgroup (up to 2048 photons), 2 generation only + the pulse kernels, 3 k_s2_bright.
 * capacity: entries the buffer holds (>= n_run_sets * n_tpc). */
int wfs_copy_tile_kernels(wfs_handle *h, int8_t *kind, int64_t capacity);
/* HIP-event timing of the kernels of the last wfs_run: names (NUL separated) and milliseconds */
int wfs_kernel_times(wfs_handle *h, char *names, int64_t names_cap, float *ms, int32_t *n_launches, int32_t *n_kernels);
int wfs_set_profiling(wfs_handle *h, int32_t on);

#ifdef __cplusplus
}
#endif
#endif
