"""ctypes binding of libwfsim_amd.so (include/wfsim_amd.h) -- the only way the Python host side reaches the GPU.

Signatures, struct layouts and the export list come from the header (abi.py): scalars are passed as plain numbers, input arrays as
any array-like (converted to the header's element type for the duration of the call), output arrays as ndarrays of exactly the
header's element type, and a mismatch is a TypeError before the library is entered.

There is no CPU fallback: if the HIP library is missing, fails to load, or no MI355X is visible, constructing an
``Engine`` raises.  Nothing in this module (or anywhere under wfsim_amd/) imports the test oracle.
"""
import ctypes as C
import dataclasses
import os

import numpy as np

from .abi import EXPORTS, WfsConfig, WfsCounts, WfsError, bind          # noqa: F401 (the names other modules and the tests take from here)
from .config import kernel_params, N_ROWS
from .dtypes import raw_record_dtype
from . import tables as T

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('WFSIM_AMD_LIB') or os.path.join(HERE, 'libwfsim_amd.so')


def pin_host(array):
    """page-locks a host array (hipHostRegister): device -> host copies into it then run at PCIe speed and asynchronously.
    Returns True on success; a failure is not an error (copies still work, staged by the driver)."""
    a = np.asarray(array)
    if a.nbytes == 0 or not a.flags['C_CONTIGUOUS']:
        return False
    return load_library().wfs_host_register(a.ctypes.data, a.nbytes) == 0


def unpin_host(array):
    load_library().wfs_host_unregister(np.asarray(array).ctypes.data)


_RECORD_BUFFERS = []        # [array, in use]: page-locked record buffers, recycled between chunkers
MAX_RECORD_BUFFERS = 4      # ceiling of the page-locked pool (1.2 GB each by default): beyond it buffers are pageable / the chunker copies


def acquire_record_buffer(length, dtype, pin=True, spare_only=False):
    """A record buffer for ChunkRawRecords (strax_interface.py:360-361: np.zeros(5000000, raw_record_dtype), 1.2 GB).
    Page-locking that much memory takes a few hundred ms, so pinned buffers are recycled between instances.  The pool never
    holds more than MAX_RECORD_BUFFERS page-locked buffers (a free one of another size is unpinned to make room); past the
    ceiling the caller gets an ordinary pageable array (``spare_only``: None) -- copies into it still work, staged by the driver."""
    dtype = np.dtype(dtype)
    for slot in _RECORD_BUFFERS:
        if not slot[1] and len(slot[0]) == length and slot[0].dtype == dtype:
            slot[1] = True
            return slot[0]
    if len(_RECORD_BUFFERS) >= MAX_RECORD_BUFFERS:
        for k, slot in enumerate(_RECORD_BUFFERS):
            if not slot[1]:
                unpin_host(slot[0])
                del _RECORD_BUFFERS[k]
                break
    if len(_RECORD_BUFFERS) >= MAX_RECORD_BUFFERS:
        return None if spare_only else np.zeros(length, dtype=dtype)
    buf = np.zeros(length, dtype=dtype)
    if pin and pin_host(buf):
        _RECORD_BUFFERS.append([buf, True])
    elif spare_only:
        return None
    return buf


def release_record_buffer(buf):
    for slot in _RECORD_BUFFERS:
        if slot[0] is buf:
            slot[1] = False


def is_pooled_record_buffer(buf):
    return any(slot[0] is buf for slot in _RECORD_BUFFERS)


def lease_record_buffer(buf, n):
    """The first n records of a pooled buffer as an array the caller may hand out: the buffer stays taken until that array
    and every view derived from it are gone, then it returns to the pool.  (The array is built on a memoryview, so numpy's
    base chain of every derived view ends at it and not at the buffer: its finaliser runs when the last view dies.)"""
    import weakref
    arr = np.frombuffer(memoryview(buf.view(np.uint8).reshape(-1)), dtype=buf.dtype, count=n)
    weakref.finalize(arr, release_record_buffer, buf)
    return arr


_lib = None


def load_library():
    """Loads libwfsim_amd.so and gives every entry point the restype and argtypes of the header; raises if it is missing (build it
    with ``python -c "import __graft_entry__ as g; g.build()"``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WfsError(f'{LIB_PATH} not found: the HIP extension is not built; there is no CPU fallback')
        # torch ships its own HIP runtime: in a process that uses both (the multi-GPU gather keeps records in torch tensors),
        # torch.cuda must be initialised BEFORE this library pulls in the system's libamdhip64 -- afterwards torch finds no GPU
        import sys
        if 'torch' in sys.modules:
            try:
                sys.modules['torch'].cuda.init()
            except Exception:
                pass
        _lib = bind(C.CDLL(LIB_PATH))          # AttributeError if a declared symbol is missing
    return _lib


def device_count():
    n = C.c_int(0)
    rc = load_library().wfs_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def device_allocations():
    """(buffers, bytes) of device memory that the engines of this process hold now; every ``close()`` gives its share back."""
    n, b = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    rc = load_library().wfs_device_allocations(n, b)
    if rc != 0:
        raise WfsError(f'wfs_device_allocations failed ({rc})')
    return int(n[0]), int(b[0])


def _arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _grid(grid):
    """(nodes per axis, first node, last node) of a regular grid, as the map entry points take it"""
    return [len(g) for g in grid], [g[0] for g in grid], [g[-1] for g in grid]


def first_instruction_of_sets(run_set, n_sets):
    """index of the first instruction of every run set -- the number the library knows the set by (include/wfsim_amd.h,
    wfs_load_instructions) -- or None when a set number is unused.  (The sets need not be numbered in order of first appearance: the
    scheduler numbers the S1 calls of a cluster before its S2 calls, rawdata.py:102.)"""
    run_set = np.asarray(run_set)
    n = len(run_set)
    if n and (run_set.min() < 0 or run_set.max() >= n_sets):      # (np.minimum.at would wrap a negative number round to the last sets)
        raise ValueError(f'run set numbers must lie in [0, {n_sets}): got {int(run_set.min())} .. {int(run_set.max())}')
    first = np.full(n_sets, n, dtype=np.int64)
    np.minimum.at(first, run_set, np.arange(n))
    return first if np.all(first < n) else None


@dataclasses.dataclass
class Batch:
    """What Python knows of the loaded batch.  Every load_* replaces it whole, as the library replaces its batch (wfs_batch.h)."""
    n_loaded: int = 0               # instructions
    n_cdf_rows: int = 0             # rows of the channel CDF table, device-evaluated ones included
    n_run_sets: object = None       # run sets of the caller (None: a batch without: optical input, injected photons)
    set_rows: object = None         # the library's row of every run set of the caller (None: the library's own rows, in order)
    lib_sets: int = 0               # the library's pulse-set rows of the last run (run sets numbered by their first instruction leave gaps)


class Engine:
    """One GPU, one stream, one fax configuration."""

    def __init__(self, config, resource, device=0, seed=None, keep_photons=False):
        """keep_photons: the photons of tile-generated S2 instructions (wfs_config.tile_gen) are also written to the photon
        array, for ``photons()`` -- by default they only exist in the registers of the pulse workgroup (tests: True)"""
        self.lib = load_library()
        self.keep_photons = bool(keep_photons)
        self.config = config
        params = kernel_params(config)
        if seed is not None:
            params['seed'] = int(seed)
        self.params = params
        cfg = WfsConfig()
        for n, _ in WfsConfig._fields_:
            setattr(cfg, n, params[n])
        self._h = C.c_void_p(0)
        self.device = int(device)
        self._pinned = []
        self._batch = Batch()
        self._smap_nv = {}              # values per node of every array-valued scalar map
        self._noise_rows = None         # (channels, common streams) of the noise model that is set
        rc = self.lib.wfs_create(C.byref(cfg), device, C.byref(self._h))
        if rc != 0:
            raise WfsError(f'wfs_create failed with code {rc}: no usable MI355X / HIP runtime (device {device})')
        nl, nc = self._init_tables(resource)
        self._init_ap_elements(resource)
        nc = self._init_switches_and_noise(resource, nl, nc)
        self._init_dark_counts()
        he_noise = bool(params['enable_noise']) and nc > params['he_first']
        self.emits_he_records = bool(params['detector_nt'] and params['n_top'] > 0 and (params['he_factor'] != 0 or he_noise))
        self._init_pattern_maps(resource)
        self._init_scalar_maps(resource)
        self._init_delay_models(resource)

    def _init_tables(self, resource):
        """uploads the init-time tables; returns the shape of the noise array (0, 0 without one)"""
        config, params = self.config, self.params
        thr_truth, thr_zle = T.thresholds(config, N_ROWS)
        lum_x, lum_t = T.luminescence_table(config)
        # a noise model (noise_model.py) takes precedence over the noise array of the resource, which is then not uploaded
        from .noise_model import noise_colour, noise_pmf, noise_slow
        self.noise_model = noise_pmf(config, params['n_rows']) if params['enable_noise'] else None
        self.noise_colour = noise_colour(config, params['n_rows']) if params['enable_noise'] else None
        self.noise_slow = noise_slow(config, params['n_rows']) if params['enable_noise'] else None
        self.tables = dict(
            templates=T.pmt_current_templates(config), spe=T.spe_scaling_table(resource.spe_charge, resource.spe_pdfs),
            gains=_arr(config['gains'], np.float64), thr_truth=_arr(thr_truth, np.float64), thr_zle=_arr(thr_zle, np.int64),
            lum_x=_arr(lum_x, np.float64), lum_t=_arr(lum_t, np.float64),
            noise=_arr(resource.noise_data, np.int16) if (params['enable_noise'] and self.noise_model is None and hasattr(resource, 'noise_data')) else None)
        t = self.tables
        assert t['templates'].shape == (params['dt'], params['tlen'])
        nl, nc = t['noise'].shape if t['noise'] is not None else (0, 0)
        self._call('wfs_set_tables', t['templates'], t['spe'], t['spe'].shape[0], t['gains'], t['thr_truth'], t['thr_zle'],
                   t['lum_x'], t['lum_t'], len(t['lum_x']), t['noise'], nl, nc)
        return nl, nc

    def _init_ap_elements(self, resource):
        if self.params['enable_pmt_ap'] and hasattr(resource, 'uniform_to_pmt_ap'):
            for e, (name, d) in enumerate(resource.uniform_to_pmt_ap.items()):
                dc, ac = _arr(d['delaytime_cdf'], np.float64), _arr(d['amplitude_cdf'], np.float64)
                self._call('wfs_set_ap_element', e, dc.shape[1], ac.shape[-1], ac.ndim == 2, 'Uniform' in name,
                           d['delaytime_bin_size'], d['amplitude_bin_size'], dc, ac)

    def _init_switches_and_noise(self, resource, nl, nc):
        """the handle's switches, then the noise source; returns the channels of that source (nc of the noise array, or the model's)"""
        params, t = self.params, self.tables
        self.tile_local_bright = bool(params['tile_local_bright'])
        if not self.tile_local_bright:         # (the library's default is on)
            self._call('wfs_set_bright_tiles', 0)
        # the bottom-array sum channel (config 'emit_sum_signal'; the library's default is off): XENONnT only (rawdata.py:241)
        self._call('wfs_set_sum_signal', params['sum_signal'])
        self.emits_sum_records = bool(params['sum_signal'] and params['detector_nt'])
        # every channel of a digitise window, not only the hit ones (config 'full_readout'; the library's default is off)
        self.full_readout = False
        if params['full_readout']:
            self.set_full_readout(True)
        if self.keep_photons or os.environ.get('WFS_CHECK_LAUNCHES', '0') not in ('', '0'):
            self.set_debug(False)          # (every launch checked from the first run on)
        # HE records exist only when the HE rows can differ from a flat baseline (wfs_engine.hip refresh_dev): a non-zero
        if t['noise'] is not None and np.asarray(resource.noise_data).dtype.kind == 'f' \
                and not np.array_equal(np.asarray(resource.noise_data), np.trunc(resource.noise_data)):
            # a float noise array with non-integral values: numba's `int64 row += float64 noise` (rawdata.py:436) stores the
            # truncated SUM, which the int16 table cannot express -- the device then adds in f64 and truncates as well
            self._call('wfs_set_noise_float', resource.noise_data, nl, nc)
        # int(high_energy_deamplification_factor) (rawdata.py:242) or noise columns for the HE channels
        if self.noise_model is not None:
            self.set_noise_model(*self.noise_model)
            nc = self.noise_model[0].shape[0]
            if self.noise_colour is not None:
                self.set_noise_colour(**self.noise_colour)
            if self.noise_slow is not None:
                self.set_noise_slow(**self.noise_slow)
        return nc

    def _init_dark_counts(self):
        # PMT dark counts (config 'dark_count_rate', dark_counts.py; the library's default is off)
        from .dark_counts import rates_from
        self.dark_count_rate = None
        rates = rates_from(self.config, self.params['n_tpc'])
        if rates is not None:
            self.set_dark_counts(rates)
        # lone-hit rows (config 'dark_count_lone_hits'): RawData runs a pass of lone_hits behind every batch
        from .dark_counts import lone_hits_from, noise_lone_hits_from
        self.lone_hits_on = lone_hits_from(self.config, self.params)
        # ... and the samples of the noise model that cross their threshold there (config 'noise_lone_hits'): either key
        # makes RawData run the pass
        self.noise_lone_hits = False
        if noise_lone_hits_from(self.config, self.params):
            self.set_lone_noise_hits(True)
            self.lone_hits_on = True

    def _init_pattern_maps(self, resource):
        # pattern maps on regular grids are evaluated on the device (one channel CDF row per instruction)
        config, params = self.config, self.params
        self.device_maps = set()
        if config.get('device_pattern_maps', True):
            from .itp_map import InterpolatingMap
            for which, (kind, dims) in enumerate([('s1', 3), ('s2', 2)], start=1):
                pm = getattr(resource, kind + '_pattern_map', None)
                if not isinstance(pm, InterpolatingMap):
                    # a straxen.InterpolatingMap handed over from the reference's own Resource: same data dict
                    data = getattr(pm, 'data', None)
                    csys = data.get('coordinate_system') if isinstance(data, dict) else None
                    if not (csys and isinstance(csys[0], (list, tuple)) and isinstance(csys[0][0], str) and 'map' in data):
                        continue
                    pm = InterpolatingMap({k: data[k] for k in ('coordinate_system', 'map')}, method=getattr(pm, 'method', 'WeightedNearestNeighbors'))
                if not (pm.dimensions == dims and pm.method == 'WeightedNearestNeighbors' and pm.map_names == ['map']):
                    continue
                if pm.grid is None:           # a point list (irregular coordinate system): brute-force neighbour search on the device
                    vals = np.asarray(pm.data['map'])
                    pts = pm.coordinate_system
                    if vals.ndim != 2 or len(vals) != len(pts) or vals.shape[1] > params['n_tpc'] or len(pts) < 2 * dims:
                        continue
                    if kind == 's2' and vals.shape[1] != params['n_tpc'] and (vals.shape[1] - 1) in np.asarray(config['channels_bottom']):
                        continue
                    self._call('wfs_set_pattern_map_points', which, dims, len(pts), pts, vals, vals.shape[1])
                    self.device_maps.add(kind)
                    continue
                grid, vals = pm.regular_grid()
                if vals.ndim != dims + 1 or vals.shape[-1] > params['n_tpc']:
                    continue
                if kind == 's2' and vals.shape[-1] != params['n_tpc'] and (vals.shape[-1] - 1) in np.asarray(config['channels_bottom']):
                    continue          # s2.py:648: such a map is not padded; leave the odd case to the host
                self._call('wfs_set_pattern_map', which, dims, *_grid(grid), vals.reshape(-1, vals.shape[-1]), vals.shape[-1])
                self.device_maps.add(kind)
        # s2_aft_sigma on device rows needs top = the first n_top channels and bottom = the rest (s2.py:660-665 scales exactly those)
        cb = np.asarray(config['channels_bottom'])
        self._aft_on_device = bool(len(cb)) and np.array_equal(cb, np.arange(params['n_top'], params['n_tpc']))

    def _init_scalar_maps(self, resource):
        # scalar maps of the resource on the device: physics.instruction_params evaluates through this view
        self._scalar_maps = []
        if self.config.get('device_scalar_maps', True):
            from .device_maps import DeviceResource
            self.resource = DeviceResource(resource, self)
        else:
            self.resource = resource

    def _init_delay_models(self, resource):
        # model variants of the photon delays (S1 custom / optical propagation, S2 garfield / optical propagation)
        from .delay_models import DelayModels
        self.models = DelayModels(self.config, resource)
        if self.models.active:
            self._set_delay_models()
            sp = self.models.s1_prop
            if sp is not None:
                self._call('wfs_set_s1_propagation', len(sp['z']), sp['nu'], sp['u0'], sp['du'], sp['top'], sp['bottom'])
            gg = self.models.gas_gap
            if gg is not None:
                self._call('wfs_set_gas_gap_model', gg['inv'].shape[0], gg['inv'].shape[1], gg['inv'])

    def _set_delay_models(self):
        base, off, pmf, vmin = self.models.table_arrays()
        self._call('wfs_set_delay_models', len(base), base, off, pmf, vmin)

    # ------------------------------------------------------------------------------------------
    def _call(self, name, *args, check=True):
        """the entry point ``name`` on this engine's handle, its arguments checked and converted by the argtypes of abi.py; raises on an
        error code (``check=False``: returns whatever the entry point returns)"""
        rc = getattr(self.lib, name)(self._h, *args)
        if check:
            self._check(rc)
        return rc

    def _check(self, rc):
        if rc != 0:
            msg = self.lib.wfs_last_error(self._h)
            raise WfsError(f'libwfsim_amd error {rc}: {msg.decode() if msg else ""}')

    def close(self):
        if self._h:
            self._call('wfs_wait_records', check=False)
            self.unpin_all()
            self._call('wfs_destroy', check=False)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------
    def load_instructions(self, ins, gid, cluster, tmin, ip, run_set=None, em_base=None):
        """ins: instruction array sorted by the scheduler key; ip: dict from physics.instruction_params;
        run_set: pulse set of every instruction (scheduler.run_sets), None = one set per instruction."""
        n = len(ins)
        cdf_row, cdf_table = _arr(ip['cdf_row'], np.int32), _arr(ip['cdf_table'], np.float64)
        from_maps = cdf_row < 0           # rows from the device pattern maps
        rs = _arr(run_set, np.int32) if run_set is not None else None
        n_run_sets = (int(rs.max()) + 1 if len(rs) else 0) if rs is not None else n
        # Run sets go to the library numbered by their FIRST instruction (the numbers of the other members stay unused): a set of one
        # instruction then carries that instruction's index, which is what lets it take the tile-local generator (wfs_tilegen.h) next to
        # the shared Pulse calls of electron afterpulses.  set_rows: the library's row of every set of the caller, for the outputs below.
        first = first_instruction_of_sets(rs, n_run_sets) if rs is not None and len(rs) else None
        if first is not None:
            rs = first[rs]
        self._batch = Batch(n_loaded=n, n_cdf_rows=cdf_table.shape[0] + int(np.sum(from_maps)), n_run_sets=n_run_sets, set_rows=first)
        self._call('wfs_load_instructions', n, ins['type'], ins['time'], ins['amp'], gid, cluster, tmin, ip['p_hit'], ip['drift_mean'],
                   ip['drift_spread'], ip['sc_gain'], cdf_row, cdf_table, cdf_table.shape[0],
                   rs, (n if first is not None else int(rs.max()) + 1) if rs is not None and len(rs) else 0, em_base)
        if np.any(from_maps):
            aft = ip.get('aft_factor')
            if aft is not None:
                self._call('wfs_set_instruction_aft', n, aft)
            ds = ip.get('diff_sigma')
            if ds is not None:                  # diffusion_transverse_map: those rows are averaged over the electrons inside wfs_run
                self._call('wfs_set_instruction_diffusion', n, ds[0], ds[1], self.config['tpc_radius'])
            pxy = ip.get('pattern_xy')          # S2: the observed position under a field distortion model
            self._call('wfs_eval_pattern_rows', n, ins['x'] if pxy is None else pxy[:, 0], ins['y'] if pxy is None else pxy[:, 1], ins['z'])
        if self.models.active:
            tab, tabb, zi, zf = self.models.instruction_tables(ins, gid)
            if self.models.per_batch:           # tables that depend on the batch (gas gap warping): upload them first
                self._set_delay_models()
            self._call('wfs_set_instruction_models', n, tab, tabb, zi, zf)
            if self.models.gas_gap is not None:
                self._call('wfs_set_instruction_gas_gap', n, *self.models.instruction_gas_gap(ins))

    def register_scalar_map(self, m, name='map'):
        """one map of an itp_map.InterpolatingMap on the device: (map id, host result has a trailing axis) or None if it is not of
        a kind the device evaluates (see device_maps.py)"""
        mid = np.full(1, -1, dtype=np.int32)          # (scalar outs are arrays of one element: their dtype is checked like any output's)
        if m.method == 'RectBivariateSpline' and name in m.splines:
            spl = m.splines[name]
            tx, ty, c = spl.tck
            kx, ky = spl.degrees
            self._call('wfs_scalar_map_spline', len(tx), tx, len(ty), ty, kx, ky, c, mid)
            return int(mid[0]), False
        if m.method not in ('WeightedNearestNeighbors', 'RegularGridInterpolator') or not 1 <= m.dimensions <= 3:
            return None
        v = np.asarray(m.data[name], dtype=np.float64)
        n_points = len(m.coordinate_system)
        if v.size % n_points or v.size // n_points > 4096:
            return None
        nv = v.size // n_points
        # values per node on a trailing axis: flat layout [points, nv] or nested along the grid axes [..., nv]
        array_valued = (v.ndim == 2 and v.shape[0] == n_points) or v.ndim == m.dimensions + 1
        if nv > 1 and not array_valued:
            return None
        trailing = array_valued and nv == 1
        v = v.reshape(n_points, nv)
        if m.method == 'RegularGridInterpolator' and m.grid is None:
            return None                 # (straxen falls back to nearest neighbours on a point list: the WeightedNearestNeighbors path below)
        if m.grid is not None:
            if m.method == 'RegularGridInterpolator':
                self._call('wfs_scalar_map_linear', m.dimensions, *_grid(m.grid), v, nv, mid)
            elif nv == 1:
                self._call('wfs_scalar_map_grid', m.dimensions, *_grid(m.grid), v, mid)
            else:
                self._call('wfs_scalar_map_grid_array', m.dimensions, *_grid(m.grid), v, nv, mid)
        else:
            if n_points < 2 * m.dimensions:
                return None
            if nv == 1:
                self._call('wfs_scalar_map_points', m.dimensions, n_points, m.coordinate_system, v, mid)
            else:
                self._call('wfs_scalar_map_points_array', m.dimensions, n_points, m.coordinate_system, v, nv, mid)
        self._smap_nv[int(mid[0])] = nv
        return int(mid[0]), bool(trailing)

    def eval_scalar_map(self, map_id, positions):
        pos = _arr(positions, np.float64)
        pos = pos.reshape(len(pos), -1)
        nv = self._smap_nv.get(map_id, 1)
        if nv == 1:
            out = np.empty(len(pos), dtype=np.float64)
            self._call('wfs_scalar_map_eval', map_id, len(pos), pos, out)
            return out
        out = np.empty((len(pos), nv), dtype=np.float64)          # array-valued map: one row of values per position
        self._call('wfs_scalar_map_eval_array', map_id, len(pos), pos, out, nv)
        return out

    def cdf_rows(self):
        """(cdf_row, cdf_table) of the loaded batch as the generator uses them, device-evaluated rows included"""
        n, rows = self._batch.n_loaded, self._batch.n_cdf_rows
        cdf_row, table = np.zeros(n, dtype=np.int32), np.zeros((rows, self.params['n_tpc']), dtype=np.float64)
        self._call('wfs_copy_cdf_rows', cdf_row, table, rows)
        return cdf_row, table

    def load_optical(self, ins, gid, cluster, tmin, channels, timings, time_cutoff):
        """ins: optical instructions (with _first/_last) sorted by time; channels/timings: the flat photon arrays"""
        self._batch = Batch(n_loaded=len(ins))           # no run sets: the outputs are the library's rows, not those of an earlier load_instructions
        self._call('wfs_load_optical', len(ins), ins['time'], gid, cluster, tmin, ins['_first'], ins['_last'], channels, timings,
                   len(timings), int(time_cutoff))

    def load_photons(self, set_cluster, set_tmin, set_off, t, ch, gain, dpe=None):
        self._batch = Batch()           # (as above)
        self._call('wfs_load_photons', len(set_cluster), set_cluster, set_tmin, set_off, t, ch, gain, dpe)

    def run(self):
        self._call('wfs_run')
        c = WfsCounts()
        self._call('wfs_get_counts', C.byref(c))
        self.counts = {n: getattr(c, n) for n, _ in WfsCounts._fields_}
        self._batch.lib_sets = self.counts['n_pulse_sets']
        rows = self._caller_sets(self._lib_sets)
        if rows is not None:
            self.counts['n_pulse_sets'] = len(rows)
        return self.counts

    _lib_sets = property(lambda self: self._batch.lib_sets)

    def set_debug(self, on=True, force_dense=False, generate_only=False, check_launches=None):
        """check_launches (default: the environment variable WFS_CHECK_LAUNCHES): every kernel launch of wfs_run is checked and
        synchronised on the spot, so that a failing kernel is reported under its own name (slow; debugging only)"""
        if check_launches is None:
            check_launches = os.environ.get('WFS_CHECK_LAUNCHES', '0') not in ('', '0')
        self._call('wfs_set_debug', int(bool(on)) | (2 if force_dense else 0) | (4 if generate_only else 0)
                   | (8 if check_launches else 0) | (16 if self.keep_photons else 0))

    def generate(self):
        """photon generation only (no pulses / records): the pre-pass of the electron afterpulses"""
        self.set_debug(False, generate_only=True)
        try:
            self._call('wfs_run')
        finally:
            self.set_debug(False)

    def instruction_photon_offsets(self):
        """first generated photon of every instruction of the batch (+ the total): generation order"""
        out = np.zeros(self._batch.n_loaded + 1, dtype=np.int64)
        self._call('wfs_copy_instruction_photon_offsets', out, len(out))
        return out

    def gather_photon_times(self, index):
        """arrival times [ns] of photons given by their index in generation order"""
        out = np.zeros(len(index), dtype=np.int64)
        if len(out):
            self._call('wfs_gather_photon_times', len(out), index, out)
        return out

    def set_profiling(self, on=True):
        self._call('wfs_set_profiling', on)

    def set_stream(self, stream_ptr):
        self._call('wfs_set_stream', stream_ptr)

    # ---- results ---------------------------------------------------------------------------------
    def records(self):
        n = self.counts['n_records']
        out = np.zeros(n, dtype=raw_record_dtype())
        self._call('wfs_copy_records', out, n)
        return out

    def _records_range(self, entry, out, count):
        n = self.counts['n_records'] if count is None else int(count)
        assert out.flags['C_CONTIGUOUS'] and out.dtype.itemsize == np.dtype(raw_record_dtype()).itemsize and len(out) >= n
        self._call(entry, out, 0, n)
        return out[:n]

    def records_into(self, out, count=None):
        """device -> host copy of the first ``count`` packed records (default: all) straight into ``out`` (a contiguous
        raw_record array, e.g. a slice of the chunker's record buffer)"""
        return self._records_range('wfs_copy_records_range', out, count)

    def records_into_async(self, out, count=None):
        """the same on the copy stream, without waiting: ``out`` must stay alive (and should be pinned, ``pin``) until
        ``wait_records`` returns; the copy overlaps the next ``run``"""
        return self._records_range('wfs_copy_records_range_async', out, count)

    def wait_records(self):
        self._call('wfs_wait_records')

    def pin(self, array):
        """page-locks a host array for this engine's lifetime (see ``pin_host``)"""
        if not pin_host(array):
            return False
        self._pinned.append(np.asarray(array))
        return True

    def unpin_all(self):
        for a in self._pinned:
            unpin_host(a)
        self._pinned = []

    def set_record_order(self, by_time):
        self._call('wfs_set_record_order', bool(by_time))

    def records_dev_ptr(self):
        return self._call('wfs_records_dev_ptr', check=False)

    def copy_records_to_device(self, dev_ptr, capacity):
        self._call('wfs_copy_records_dev', dev_ptr, capacity)

    def groups(self):
        g = self.counts['n_groups']
        left, right, first, ix = (np.zeros(g, dtype=np.int64) for _ in range(4))
        self._call('wfs_copy_groups', left, right, first, ix)
        return dict(left=left, right=right, first_record=first, ix_rand=ix)

    def intervals(self):
        n = self.counts['n_intervals']
        group, ch = np.zeros(n, np.int32), np.zeros(n, np.int32)
        left, right, off = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n + 1, np.int64)
        self._call('wfs_copy_intervals', group, ch, left, right, off, n + 1)
        data = np.zeros(int(off[n]), dtype=np.int16)
        self._call('wfs_copy_interval_data', data, len(data))
        return dict(group=group, channel=ch, left=left, right=right, data_off=off, data=data)

    def pulses(self, currents=False):
        n = self.counts['n_tiles']
        s, ch = np.zeros(n, np.int32), np.zeros(n, np.int32)
        left, right, nph, off = (np.zeros(n, np.int64) for _ in range(4))
        self._call('wfs_copy_pulses', s, ch, left, right, nph, off, n)
        rows = self._caller_sets(self._lib_sets)
        if rows is not None:                        # the library's set numbers -> the caller's
            inv = np.full(self._lib_sets, -1, dtype=np.int32)
            inv[rows] = np.arange(len(rows), dtype=np.int32)
            s = inv[s]
        out = dict(set=s, channel=ch, left=left, right=right, n_photons=nph, cur_off=off)
        if currents:
            total = int((right - left + 1).sum())
            cur = np.zeros(total, dtype=np.float64)
            self._call('wfs_copy_currents', cur, total)
            out['current'] = cur
        return out

    def rows(self):
        """debug copy (``set_debug(True)`` before ``run()``) of the rows before zero suppression.  With ``full_readout`` it lists the rows
        WITH pulses only, each over its window's full range; a row without a pulse is made finished and never exists in this form
        (``counts['n_rows']`` counts it, ``intervals()`` and ``records()`` hold what it stores)."""
        n = self.counts['n_rows']
        g, ch = np.zeros(n, np.int32), np.zeros(n, np.int32)
        left, right, off = (np.zeros(n, np.int64) for _ in range(3))
        right -= 1                      # (an entry the library does not write -- a row without a pulse under full_readout -- stays empty)
        self._call('wfs_copy_rows', g, ch, left, right, off, n)
        listed = right >= left
        g, ch, left, right, off = g[listed], ch[listed], left[listed], right[listed], off[listed]
        total = int((right - left + 1).sum())
        data = np.zeros(total, dtype=np.int32)
        self._call('wfs_copy_row_data', data, total)
        return dict(group=g, channel=ch, left=left, right=right, data_off=off, data=data)

    def set_full_readout(self, on):
        """config 'full_readout' between runs (wfs_set_full_readout): from the next ``run()`` every TPC and HE row slot of
        a digitise window has a row of the window's range, with or without a pulse.  ``intervals()`` and ``records()`` are the
        contract for those rows; ``rows()`` (debug) lists the rows WITH pulses only, at the window's range, and ``sum_signal()`` the
        unchanged sum rows -- a row without a pulse never exists unfinished."""
        self._call('wfs_set_full_readout', bool(on))
        self.full_readout = bool(on)

    def sum_signal(self):
        """the bottom-array sum rows of the last run before they are finished (config 'emit_sum_signal'): per row its window, its
        absolute first and last sample and S[t] = int(he_factor) * sum of the bottom rows, at data[data_off[k]:data_off[k + 1]].
        ``full_readout`` does not change them: range and value stay the union and the sum of the bottom-array PULSES of the window."""
        n, total = self.counts['n_groups'], self.counts['n_raw_samples']
        g = np.zeros(n, np.int32)
        left, right, off = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n + 1, np.int64)
        data = np.zeros(total, dtype=np.int64)
        self._call('wfs_copy_sum_signal', g, left, right, off, data, n + 1, total)
        k = int(np.argmax(off))         # rows: data_off rises up to the total, the entries behind it stay 0
        return dict(group=g[:k], left=left[:k], right=right[:k], data_off=off[:k + 1], data=data[:int(off[k])])

    def _caller_sets(self, s):
        """rows of the library's pulse sets that belong to the caller's run sets (None: all of them, in order): primaries, then -- when the
        library made PMT-afterpulse sets, a second block of the same size -- theirs"""
        rows = self._batch.set_rows
        if rows is None or not self.counts['n_instructions']:
            return None
        n = self.counts['n_instructions']
        return rows if s == n else np.concatenate([rows, n + rows])

    def photons(self):
        n, s = self.counts['n_photons'], self._lib_sets
        off = np.zeros(s + 1, np.int64)
        t, ch, gain, dpe = np.zeros(n, np.int64), np.zeros(n, np.int16), np.zeros(n, np.float64), np.zeros(n, np.uint8)
        self._call('wfs_copy_photons', off, t, ch, gain, dpe, n)
        rows = self._caller_sets(s)
        if rows is not None:                        # the caller's sets, in the caller's order (the unused set numbers hold no photons)
            lens = off[rows + 1] - off[rows]
            if np.all(np.diff(rows) > 0):
                off = np.append(off[rows], off[-1])
            else:
                new_off = np.concatenate([[0], np.cumsum(lens)])
                idx = np.repeat(off[rows] - new_off[:-1], lens) + np.arange(int(new_off[-1]))
                t, ch, gain, dpe, off = t[idx], ch[idx], gain[idx], dpe[idx], new_off
        return dict(set_off=off, t=t, ch=ch, gain=gain, dpe=dpe)

    def truth(self):
        s = self._lib_sets
        acc, ts = np.zeros((s, 12)), np.zeros((s, 5))
        self._call('wfs_copy_truth', acc, ts, s)
        rows = self._caller_sets(s)
        return (acc, ts) if rows is None else (acc[rows], ts[rows])

    def truth_per_pmt(self):
        """[pulse set][channel][n_photon, n_pe, n_photon_trigger, n_pe_trigger, raw_area, raw_area_trigger] (pulse.py:259-271)"""
        s = self._lib_sets
        acc = np.zeros((s, int(self.params['n_tpc']), 6))
        if s:
            self._call('wfs_copy_truth_per_pmt', acc, s)
        rows = self._caller_sets(s)
        return acc if rows is None else acc[rows]

    def tile_kernels(self):
        """[primary pulse set][channel] int8: which kernel made the tile in the last run -- 0 no photons or not tile-generated, 1 photons and
        pulse in one workgroup (up to 2048 photons), 2 generation only + the pulse kernels, 3 the bright-tile kernel (k_s2_bright)"""
        s, nch = self._lib_sets, int(self.params['n_tpc'])
        kind = np.full(s * nch, -1, dtype=np.int8)
        if s:
            self._call('wfs_copy_tile_kernels', kind, len(kind))
        kind = kind[kind >= 0].reshape(-1, nch)         # (the library fills the primary sets: PMT-afterpulse sets follow them and have no entry)
        rows = self._batch.set_rows
        return kind if rows is None or not self.counts['n_instructions'] else kind[rows]

    def set_noise_offsets(self, ix_rand):
        self._call('wfs_set_noise_offsets', ix_rand, len(ix_rand))

    def set_noise_model(self, pmf, vmin=0):
        """pmf[n_channels][n_values] over the ADC offsets vmin .. vmin + n_values - 1 (noise_model.py); None clears the model: the noise
        array, if any, is replayed again.  Acts with enable_noise, from the next run."""
        if pmf is None:
            self._call('wfs_set_noise_model', 0, 0, 0, None)
            self._noise_rows = None
            self.noise_lone_hits = False        # (the library switches the noise-hit seeds off with the model)
            return
        pmf = _arr(pmf, np.float64)
        if pmf.ndim != 2:
            raise ValueError('set_noise_model: pmf must be [n_channels][n_values]')
        self._call('wfs_set_noise_model', pmf.shape[0], pmf.shape[1], vmin, pmf)
        # (channels, common streams) of the model as the library holds it: the C entry points of the colour and of the slow levels take
        # no row count and read n_channels + n_groups rows, so the arrays are checked against it here
        self._noise_rows = (int(pmf.shape[0]), 0)

    def set_noise_colour(self, taps_q, group=None, mix_q=None, common_pmf=None):
        """The colour of the noise model that is set (noise_model.py, wfs_set_noise_colour): taps_q int32[n_channels + n_groups][L] in Q16,
        group int32[n_channels] (-1: none), mix_q int32[n_channels] in Q16, common_pmf[n_groups][n_values] on the model's values; the
        last three may be None without common streams.  taps_q None clears the colour: the white values return.  From the next run."""
        if taps_q is None:
            self._call('wfs_set_noise_colour', 0, None, 0, None, None, None)
            self._noise_rows = (self._noise_rows[0], 0) if self._noise_rows else None
            return
        taps_q = _arr(taps_q, np.int32)
        if taps_q.ndim != 2:
            raise ValueError('set_noise_colour: taps_q must be [n_channels + n_groups][n_taps]')
        n_groups = 0 if common_pmf is None else len(common_pmf)
        n_ch = self._noise_rows
        if n_ch is not None and (taps_q.shape[0] != n_ch[0] + n_groups or (n_groups and len(np.atleast_1d(group)) != n_ch[0])):
            raise ValueError(f'set_noise_colour: the model has {n_ch[0]} channels: taps_q must have {n_ch[0] + n_groups} rows ({n_groups} groups), '
                             f'group and mix_q {n_ch[0]} entries')
        if n_groups:
            group, mix_q, common_pmf = _arr(group, np.int32), _arr(mix_q, np.int32), _arr(common_pmf, np.float64)
            if group.ndim != 1 or mix_q.shape != group.shape or common_pmf.ndim != 2 or taps_q.shape[0] != len(group) + n_groups:
                raise ValueError('set_noise_colour: group and mix_q must be [n_channels], common_pmf [n_groups][n_values], taps_q [n_channels + n_groups][n_taps]')
        else:
            group = mix_q = common_pmf = None
        self._call('wfs_set_noise_colour', taps_q.shape[1], taps_q, n_groups, group, mix_q, common_pmf)
        self._noise_rows = (self._noise_rows[0], n_groups) if self._noise_rows else None

    def set_noise_slow(self, shifts, slow_q=None):
        """The slow levels of the noise model that is set (noise_model.py, wfs_set_noise_slow): shifts int32[n_levels] (knots 2^shift
        samples apart), slow_q int32[n_channels + n_groups][n_levels] in Q16.  Set the colour first: setting a model or a colour clears
        the levels.  shifts None clears them.  From the next run."""
        if shifts is None:
            self._call('wfs_set_noise_slow', 0, None, None)
            return
        shifts, slow_q = _arr(shifts, np.int32), _arr(slow_q, np.int32)
        if shifts.ndim != 1 or slow_q.ndim != 2 or slow_q.shape[1] != len(shifts):
            raise ValueError('set_noise_slow: shifts must be [n_levels], slow_q [n_channels + n_groups][n_levels]')
        rows = self._noise_rows
        if rows is not None and slow_q.shape[0] != rows[0] + rows[1]:
            raise ValueError(f'set_noise_slow: the model has {rows[0]} channels and {rows[1]} common streams: slow_q must have {rows[0] + rows[1]} rows, '
                             f'not {slow_q.shape[0]}')
        self._call('wfs_set_noise_slow', len(shifts), shifts, slow_q)

    def _samples(self, entry, dtype, row, t0, n):
        out = np.zeros(int(n), dtype=dtype)
        self._call(entry, row, t0, n, out)
        return out

    def noise_slow_samples(self, row, t0, n):
        """the slow part S(row, t0 .. t0 + n - 1) in Q16 (int32): row < n_channels a channel, n_channels + g common stream g"""
        return self._samples('wfs_noise_slow_samples', np.int32, row, t0, n)

    def noise_white_samples(self, row, t0, n):
        """the white sequence w(row, t0 .. t0 + n - 1) under the colour: row < n_channels a channel, n_channels + g common stream g"""
        return self._samples('wfs_noise_white_samples', np.int16, row, t0, n)

    def noise_samples(self, channel, t0, n):
        """noise(channel, t0 .. t0 + n - 1) of the noise model (colour and slow levels included), evaluated on the device: t is the
        absolute sample index (time / dt)"""
        return self._samples('wfs_noise_model_samples', np.int16, channel, t0, n)

    def set_dark_counts(self, rate_hz):
        """PMT dark counts between runs (wfs_set_dark_counts): a rate in Hz for every PMT, or one value per channel for the
        first len(rate_hz) of them; None (or rates that are all zero) switches them off.  From the next ``run()`` every finished
        sample of a TPC or HE row carries the single-electron pulses its PMT makes on its own, a pure function of (seed, channel,
        absolute time); windows, truth and record order do not change, the sum row carries none."""
        if rate_hz is None:
            self._call('wfs_set_dark_counts', 0, None)
            self.dark_count_rate = None
            return
        r = np.asarray(rate_hz, dtype=np.float64)
        if r.ndim == 0:
            r = np.full(self.params['n_tpc'], float(r))
        r = np.ascontiguousarray(r.ravel())
        self._call('wfs_set_dark_counts', len(r), r)
        self.dark_count_rate = r.copy() if np.any(r > 0) else None

    def dark_count_samples(self, channel, t0, n):
        """D(channel, t0 .. t0 + n - 1): what the dark counts of a PMT add to its accumulated ADC at the absolute samples (time / dt),
        evaluated on the device"""
        return self._samples('wfs_dark_count_samples', np.int32, channel, t0, n)

    def dark_count_photons(self, channel, t0, n):
        """(t_ns int64[k], gain float64[k]) of the dark photons of a PMT whose pulse starts at a sample in [t0, t0 + n), in time order:
        the truth does not hold them, this is how a hit is matched to a dark count"""
        cap = 64
        while True:
            t, g, k = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.float64), np.zeros(1, dtype=np.int64)
            rc = self._call('wfs_dark_count_photons', channel, t0, n, t, g, cap, k, check=False)
            if rc == -3 and k[0] > cap:          # (WFS_E_CAPACITY: the count is known now)
                cap = int(k[0])
                continue
            self._check(rc)
            return t[:k[0]].copy(), g[:k[0]].copy()

    def dark_count_thresholds(self, channel):
        """uint32[4]: floor(2^32 P(N >= k)), k = 1 .. 4, of the channel's photons per cell of 64 samples, as the device holds them"""
        thr = np.zeros(4, dtype=np.uint32)
        self._call('wfs_copy_dark_counts', channel, thr)
        return thr

    def lone_hits(self, s0, s1, s_limit=None):
        """raw_records of the lone-hit rows (wfs_lone_hits) whose first seed starts at an absolute sample in [s0, s1),
        in (time, channel) order.  The seeds are the dark photons outside the rows of the last ``run()`` (outside every row when there
        was none) and, with ``set_lone_noise_hits(True)``, the samples of the noise model that cross their threshold there.  A chain of
        seeds is followed beyond s1 but no further than ``s_limit`` (default: s1).  Needs dark-count rates or the noise-hit seeds."""
        n = np.zeros(1, dtype=np.int64)
        self._call('wfs_lone_hits', int(s0), int(s1), int(s1 if s_limit is None else s_limit), n)
        out = np.zeros(int(n[0]), dtype=raw_record_dtype())
        if len(out):
            self._call('wfs_copy_lone_records', out, len(out))
        return out

    def overlay_records(self, bg, sim=None, baseline=None, n_sim=None):
        """raw_records of the overlay pass (wfs_overlay_records): the simulation's stream ``sim`` -- None: the records of the
        last ``run()``, where the device holds them -- merged per channel with the recorded background ``bg``, in (time, channel)
        order.  Pulses of the two streams that share a sample become one pulse; where both cover a sample it holds b + a - baseline,
        where the simulation alone does a - baseline + ``baseline[channel]`` (int32 per row slot; None: the configuration's baseline).
        ``n_sim`` (with ``sim`` None): only the first n_sim records of the run, in the order of ``records()``."""
        dtype = raw_record_dtype()

        def stream(x, name):
            x = np.ascontiguousarray(x)
            if x.dtype != dtype or x.ndim != 1:
                raise ValueError(f'overlay_records: {name} must be a 1-d array of raw_record_dtype()')
            return x
        bg = stream(bg, 'bg')
        sim = None if sim is None else stream(sim, 'sim')
        if baseline is not None:
            baseline = np.ascontiguousarray(baseline, dtype=np.int32)
            if baseline.shape != (int(self.params['n_rows']),):
                raise ValueError(f"overlay_records: baseline must hold one value per row slot ({int(self.params['n_rows'])})")
        n = np.zeros(1, dtype=np.int64)
        # (an empty array still has an address: NULL means "the last run's records")
        self._call('wfs_overlay_records', None if sim is None else sim.view(np.uint8).reshape(-1) if len(sim) else np.zeros(1, dtype=np.uint8),
                   (-1 if n_sim is None else int(n_sim)) if sim is None else len(sim), bg.view(np.uint8).reshape(-1) if len(bg) else None, len(bg), baseline, n)
        out = np.zeros(int(n[0]), dtype=dtype)
        if len(out):
            self._call('wfs_copy_overlay_records', out, len(out))
        return out

    def lone_hit_rows(self):
        """the rows of the last ``lone_hits`` pass in (channel, time) order: a structured array (channel, left, right, ix_rand,
        n_photons) -- first and last absolute sample, the noise-table offset (0 without a table), the lone dark photons of the chain
        (its noise-hit seeds: ``lone_hit_noise_seeds``)"""
        k = np.zeros(1, dtype=np.int64)
        self._call('wfs_copy_lone_rows', None, None, None, None, None, 0, k, check=False)
        n = int(k[0])
        ch, nph = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        left, right, ixr = (np.zeros(n, dtype=np.int64) for _ in range(3))
        if n:
            self._call('wfs_copy_lone_rows', ch, left, right, ixr, nph, n, k)
        out = np.zeros(n, dtype=[('channel', np.int32), ('left', np.int64), ('right', np.int64), ('ix_rand', np.int64), ('n_photons', np.int32)])
        out['channel'], out['left'], out['right'], out['ix_rand'], out['n_photons'] = ch, left, right, ixr, nph
        return out

    def set_lone_noise_hits(self, on):
        """config 'noise_lone_hits' between passes (wfs_set_lone_noise_hits): from the next ``lone_hits`` on, every sample of
        a PMT channel inside the noise model whose finished value -- noise, dark counts where rates are set, baseline, clamp -- lies
        below the channel's ZLE threshold, and which lies in no row of the channel, is a seed of a lone-hit row, as a lone dark photon
        is one.  Needs a drawn noise model and enable_noise; clearing the model switches it off."""
        self._call('wfs_set_lone_noise_hits', bool(on))
        self.noise_lone_hits = bool(on)

    def lone_hit_noise_seeds(self):
        """the noise-hit seeds of every row of the last ``lone_hits`` pass, int32 in the row order of ``lone_hit_rows``"""
        k = np.zeros(1, dtype=np.int64)
        self._call('wfs_copy_lone_row_noise_hits', None, 0, k, check=False)
        out = np.zeros(int(k[0]), dtype=np.int32)
        if len(out):
            self._call('wfs_copy_lone_row_noise_hits', out, len(out), k)
        return out

    def noise_model_cells(self, channel):
        """the Walker alias cells the device samples a channel's noise from: dict(thr, alias, shift, vmin); cell c = word >> shift gives
        vmin + c if (word << (32 - shift)) mod 2^32 < thr[c], else vmin + alias[c]"""
        cap = 4096
        thr, alias = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        n, shift, vmin = (np.zeros(1, dtype=np.int32) for _ in range(3))
        self._call('wfs_copy_noise_model', channel, thr, alias, cap, n, shift, vmin)
        return dict(thr=thr[:n[0]].copy(), alias=alias[:n[0]].copy(), shift=int(shift[0]), vmin=int(vmin[0]))

    def set_window_carry(self, has_pulse, last_pulse_end_time):
        self._call('wfs_set_window_carry', has_pulse, last_pulse_end_time)

    def cluster_groups(self, n_clusters):
        g = np.zeros(n_clusters, dtype=np.int32)
        if n_clusters:
            self._call('wfs_copy_cluster_groups', g, n_clusters)
        return g

    def electron_stats(self):
        """per run set (= per instruction unless run sets were given): n, mean, min, max, std of the electron times"""
        n, rows = self._batch.n_run_sets, self._batch.set_rows
        if n is None or self.counts['n_instructions'] == 0:
            n, rows = self.counts['n_instructions'], None
        if rows is not None:
            n = self.counts['n_instructions']
        es = np.zeros((n, 5))
        if n:
            self._call('wfs_copy_electron_stats', es, n)
        return es if rows is None else es[rows]

    def kernel_times(self):
        names = C.create_string_buffer(4096)
        ms, nl, nk = np.zeros(64, dtype=np.float32), np.zeros(64, dtype=np.int32), np.zeros(1, dtype=np.int32)
        self._call('wfs_kernel_times', names, 4096, ms, nl, nk)
        parts = names.raw.split(b'\0')[:nk[0]]
        return {parts[k].decode(): (float(ms[k]), int(nl[k])) for k in range(nk[0])}
