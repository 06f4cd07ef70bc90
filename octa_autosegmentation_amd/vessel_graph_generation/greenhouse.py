"""Batched drop-in for the reference's Greenhouse.develop_forest (vessel_graph_generation/greenhouse.py)
on MI355X: B independent samples advance in lock-step inside liboctahip.so (octa_sim_* entry points).

Sample k behaves like `random.seed(seeds[k]); np.random.seed(seeds[k])` followed by the reference's
generate_vessel_graph.main(config) (generate_vessel_graph.py:24-56): same CSV rows, same radii.
The host keeps only what the reference itself delegates to numpy/LAPACK: the leaf-bifurcation
geometry (np.mean / np.cov / np.linalg.eig, greenhouse.py:205-233), served to the device in batches.
"""
import csv
import ctypes
import os
import io

import numpy as np

from .. import _native

MODE_KEYS = ["I", "N", "eps_n", "eps_s", "eps_k", "delta_art", "delta_ven", "gamma_art", "gamma_ven", "phi", "omega",
             "kappa", "delta_sigma"]
MAX_ATTS = 256


class SimConfigStruct(ctypes.Structure):
    _fields_ = [("param_scale", ctypes.c_double), ("d", ctypes.c_double), ("r", ctypes.c_double),
                ("faz_radius_mean", ctypes.c_double), ("faz_radius_std", ctypes.c_double),
                ("rotation_radius", ctypes.c_double), ("faz_center", ctypes.c_double * 2),
                ("size", ctypes.c_double * 3), ("n_trees", ctypes.c_int), ("walls", ctypes.c_int * 4),
                ("n_modes", ctypes.c_int), ("modes", (ctypes.c_double * 13) * 8),
                ("forest_type", ctypes.c_int), ("nerve_center", ctypes.c_double * 2), ("nerve_radius", ctypes.c_double),
                ("geometry", ctypes.c_void_p), ("geometry_shape", ctypes.c_int * 3),
                ("n_source_walls", ctypes.c_int), ("source_walls", ctypes.c_int * 6)]


REQ_DTYPE = np.dtype([("sample", np.int32), ("n", np.int32), ("pos", np.float64, 3), ("r", np.float64),
                      ("kappa", np.float64), ("d", np.float64), ("atts", np.float64, (MAX_ATTS, 3))])
BIF_FN = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p)


def config_to_struct(config):
    """Generator YAML dict (Greenhouse / Forest sections, docker/vessel_graph_gen_docker_config.yml) -> C struct."""
    g, f = config["Greenhouse"], config["Forest"]
    if f["type"] not in ("stumps", "nerve"):
        raise NotImplementedError(f"The Forest initialization type '{f['type']}' is not implemented. Try 'stumps' or 'nerve' instead.")
    walls = f["source_walls"]
    geo_path = g["SimulationSpace"].get("oxygen_sample_geometry_path")
    wall_names = ("x0", "x1", "y0", "y1", "z0", "z1")
    enabled = [k for k, v in walls.items() if v]       # forest.py:81-91: the wall is drawn by its position in the mapping
    if f["type"] == "stumps" and geo_path is None and any(k in ("z0", "z1") for k in enabled):
        # simulation_space.py:82-87: without a geometry file the z branch reads an attribute nothing sets
        raise AttributeError("'SimulationSpace' object has no attribute 'valid_pixels'")
    p = SimConfigStruct()
    p.n_source_walls = len(enabled)
    for i, k in enumerate(enabled):
        p.source_walls[i] = wall_names.index(k)
    p.param_scale, p.d, p.r = g["param_scale"], g["d"], g["r"]
    p.faz_radius_mean, p.faz_radius_std = g["FAZ_radius_bound"]
    p.rotation_radius = g["rotation_radius"]
    p.faz_center[0], p.faz_center[1] = g["FAZ_center"]
    s = g["SimulationSpace"]
    p.size[0], p.size[1], p.size[2] = s["no_voxel_x"], s["no_voxel_y"], s["no_voxel_z"]
    p.n_trees = f["N_trees"]
    for i, k in enumerate(("x0", "x1", "y0", "y1")):
        p.walls[i] = 1 if walls.get(k) else 0
    if geo_path is not None:     # simulation_space.py:29-34: the sink-sampling mask (and the space's extent) come from a .npy file
        geo = np.ascontiguousarray(np.load(geo_path) != 0, dtype=np.uint8)
        if geo.ndim != 3:
            raise ValueError(f"the sampling geometry must be a 3-D mask (got shape {geo.shape})")
        if f["type"] != "stumps":
            raise NotImplementedError("a sampling geometry with nerve forests is not on the GPU path")
        p._geometry_keepalive = geo          # the struct only carries the pointer
        p.geometry = geo.ctypes.data
        p.geometry_shape[0], p.geometry_shape[1], p.geometry_shape[2] = geo.shape
    p.forest_type = 1 if f["type"] == "nerve" else 0
    p.nerve_center[0], p.nerve_center[1] = g["nerve_center"]
    p.nerve_radius = g["nerve_radius"]
    if len(g["modes"]) > 8:
        raise NotImplementedError("at most 8 modes")
    p.n_modes = len(g["modes"])
    for m, mode in enumerate(g["modes"]):
        for j, key in enumerate(MODE_KEYS):
            p.modes[m][j] = float(mode[key])
    return p


def _unit(v):
    return v / np.linalg.norm(v)


def bifurcation_children(position, atts, r, kappa, d):
    """Child positions of a bifurcating leaf (greenhouse.py:205-233). Must go through the same
    numpy / LAPACK entry points as the reference: the sign dgeev gives the dominant eigenvector
    decides which child comes first."""
    r_p = (r ** kappa + r ** kappa) ** (1 / kappa)
    phi = np.degrees(np.arccos((r_p ** 4 + r ** 4 - r ** 4) / (2 * r_p ** 2 * r ** 2)))
    c = np.mean(atts, axis=0)
    axis_c = c - position
    if np.linalg.norm(axis_c) != 0.0:
        axis_c = axis_c / np.linalg.norm(axis_c)
    X = np.array([a - c for a in atts]).transpose()
    w, v = np.linalg.eig(np.cov(X))
    d_l = v[:, np.argmax(w)]
    cs, sn = np.cos(np.radians(phi)), np.sin(np.radians(phi))
    p1 = np.real(position + _unit(cs * axis_c + sn * d_l) * d)
    p2 = np.real(position + _unit(cs * axis_c - sn * d_l) * d)
    return p1, p2


_REC_DOUBLES = 1 + 3 + 3 + MAX_ATTS * 3   # (sample, n) packed in one double slot, pos, r/kappa/d, attractors
_angle_cache = {}


def _murray_cos_sin(r, kappa):
    """cos / sin of the bifurcation half-angle for two equal children (greenhouse.py:204-215)."""
    key = (r, kappa)
    v = _angle_cache.get(key)
    if v is None:
        r_p = (r ** kappa + r ** kappa) ** (1 / kappa)
        phi = np.degrees(np.arccos((r_p ** 4 + r ** 4 - r ** 4) / (2 * r_p ** 2 * r ** 2)))
        v = (np.cos(np.radians(phi)), np.sin(np.radians(phi)))
        _angle_cache[key] = v
    return v


def _covariance_like_numpy(atts, c):
    """np.cov(np.array([a - c for a in atts]).transpose()) through the same numpy calls np.cov makes
    (mean over the strided axis, in-place centring, dot with the conjugated transpose, scaling), minus
    its Python-level argument handling."""
    n = len(atts)
    X = np.array((atts - c).transpose(), ndmin=2, dtype=np.float64)
    avg = X.mean(axis=1)
    X -= avg[:, None]
    cm = np.dot(X, X.T.conj())
    cm *= np.true_divide(1, n - 1)
    return cm


def bifurcation_children_batch(recs, counts):
    """recs: float64 [m, _REC_DOUBLES] request records, counts: attractors per request -> float64 [m, 6].
    Same arithmetic as bifurcation_children (the eigen-decompositions run as one stacked LAPACK call)."""
    m = len(recs)
    out = np.empty((m, 6))
    covs = np.empty((m, 3, 3))
    axes = []
    for i in range(m):
        rec = recs[i]
        n = int(counts[i])
        pos = rec[1:4]
        atts = rec[7:7 + 3 * n].reshape(n, 3)
        c = np.add.reduce(atts, axis=0) / n           # == np.mean(atts, axis=0)
        axis_c = c - pos
        nrm = np.sqrt(axis_c.dot(axis_c))             # == np.linalg.norm(axis_c)
        if nrm != 0.0:
            axis_c = axis_c / nrm
        axes.append(axis_c)
        covs[i] = _covariance_like_numpy(atts, c)
    w_all, v_all = np.linalg.eig(covs)
    for i in range(m):
        rec = recs[i]
        pos, r, kappa, d = rec[1:4], float(rec[4]), float(rec[5]), float(rec[6])
        cs, sn = _murray_cos_sin(r, kappa)
        w, v = w_all[i], v_all[i]
        if np.iscomplexobj(w) and np.all(w.imag == 0.0):
            w, v = w.real, v.real
        d_l = v[:, np.argmax(w)]
        a1 = cs * axes[i] + sn * d_l
        a2 = cs * axes[i] - sn * d_l
        out[i, 0:3] = np.real(pos + a1 / np.linalg.norm(a1) * d)
        out[i, 3:6] = np.real(pos + a2 / np.linalg.norm(a2) * d)
    return out


@BIF_FN
def _serve_bifurcations(n_req, reqs_ptr, out6, _user):
    buf = (ctypes.c_char * (REQ_DTYPE.itemsize * n_req)).from_address(reqs_ptr)
    recs = np.frombuffer(buf, dtype=np.float64).reshape(n_req, _REC_DOUBLES)
    counts = np.frombuffer(buf, dtype=np.int32).reshape(n_req, 2 * _REC_DOUBLES)[:, 1]
    out = np.ctypeslib.as_array(out6, shape=(n_req, 6))
    out[:] = bifurcation_children_batch(recs, counts)


_native_state = {"ready": None, "kappas": ()}


def _numpy_blas_path():
    import glob
    cands = glob.glob(os.path.join(os.path.dirname(np.__file__), "..", "numpy.libs", "libscipy_openblas64_*.so"))
    return cands[0] if cands else None


def _enable_native_bifurcation_service(config):
    """Switch the bifurcation service to the C++ path (same BLAS/LAPACK as numpy) after checking it bit-for-bit
    against the numpy formula on random requests. Returns the function pointer to hand to octa_sim_run."""
    py_cb = ctypes.cast(_serve_bifurcations, ctypes.c_void_p)
    g = config["Greenhouse"]
    r = g["r"] / g["param_scale"]
    kappas = tuple(sorted({float(m["kappa"]) for m in g["modes"]}))
    key = (r, kappas)
    if _native_state["ready"] is not None and _native_state["kappas"] == key:
        return _native_state["ready"]
    lib = _native.lib()
    path = _numpy_blas_path()
    fn = py_cb
    if path is not None:
        kap = np.array(kappas)
        cs = np.array([_murray_cos_sin(r, k)[0] for k in kappas])
        sn = np.array([_murray_cos_sin(r, k)[1] for k in kappas])
        if lib.octa_bif_native_init(path.encode(), len(kappas), kap.ctypes.data, cs.ctypes.data, sn.ctypes.data, py_cb, None) == 0:
            rng = np.random.default_rng(20240607)
            m = 256
            recs = np.zeros((m, _REC_DOUBLES))
            counts = np.zeros(m, np.int32)
            for i in range(m):
                n = int(rng.integers(2, 48))
                counts[i] = n
                pos = rng.uniform(0.1, 0.9, 3) * np.array([1, 1, 0.0131])
                atts = pos + rng.normal(0, rng.uniform(0.002, 0.08), (n, 3)) * np.array([1, 1, 0.05]) + rng.normal(0, 0.02, 3) * np.array([1, 1, 0])
                recs[i, 1:4] = pos
                recs[i, 4:7] = [r, kappas[i % len(kappas)], rng.uniform(0.012, 0.034)]
                recs[i, 7:7 + 3 * n] = atts.ravel()
            recs.view(np.int32).reshape(m, -1)[:, 1] = counts
            want = bifurcation_children_batch(recs, counts)
            got = np.zeros((m, 6))
            lib.octa_bif_native(m, recs.ctypes.data, got.ctypes.data, None)
            if (got == want).all():
                fn = ctypes.cast(lib.octa_bif_native, ctypes.c_void_p)
                why = None
            else:
                why = f"the native service differs from the numpy formula on {int((got != want).any(axis=1).sum())} of {m} self-check requests"
        else:
            why = "octa_bif_native_init could not bind cblas_dgemm / cblas_ddot / LAPACKE_dgeev in " + path
    else:
        why = "numpy's bundled OpenBLAS (numpy.libs/libscipy_openblas64_*.so) was not found"
    _native_state["ready"], _native_state["kappas"] = fn, key
    _native_state["kind"], _native_state["why_not_native"] = ("native" if why is None else "python"), why
    # said once per process and configuration: the Python callback gives the same bytes but serves a request in ~36 us instead of ~4
    import sys
    if why is None:
        print(f"[octa] leaf-bifurcation service: native C++ on {os.path.basename(path)} (bit-for-bit self-check on {m} requests passed)", file=sys.stderr)
    else:
        print(f"[octa] leaf-bifurcation service: PYTHON callback (about 10x slower per request, same results): {why}", file=sys.stderr)
    return fn


def bifurcation_service_kind():
    """'native' / 'python' (None before the first simulator was built) and, for 'python', why the native service was not taken."""
    return _native_state.get("kind"), _native_state.get("why_not_native")


class SimulationResult:
    """Edges of B samples in the reference's CSV row order plus per-sample statistics."""

    def __init__(self, edges, edge_off, n_art, stats, d_edges=None):
        """edges: float64 [n, 7] on the host, or None when the list was exported on the device (`d_edges`, a CUDA tensor): the host
        copy is then fetched on first use of `.edges`."""
        self._edges, self.d_edges = edges, d_edges
        self.edge_off, self.n_art, self.stats = edge_off, n_art, stats

    @property
    def edges(self):
        if self._edges is None:
            self._edges = self.d_edges.cpu().numpy()
        return self._edges

    def __len__(self):
        return len(self.edge_off) - 1

    def sample_edges(self, k):
        return self.edges[self.edge_off[k]:self.edge_off[k + 1]]

    def arterial_venous(self, k):
        e = self.sample_edges(k)
        return e[: self.n_art[k]], e[self.n_art[k]:]


class BatchSimulator:
    """Owns the device state of B lock-step samples for one generator config."""

    def __init__(self, config, batch, device_index=None):
        self._lib = _native.lib()
        self._ctx = _native.ctx(device_index)
        self._cfg = config_to_struct(config)
        self._config = config
        self._bif_fn = _enable_native_bifurcation_service(config)
        self.batch = int(batch)
        import torch
        self.device_index = torch.cuda.current_device() if device_index is None else int(device_index)
        self.device_export = os.environ.get("OCTA_SIM_HOST_EXPORT") != "1"       # 1: the round-2 path (download the node arrays, BFS on the host)
        self._h = None
        self._create()

    def _create(self, force_large=False):
        """Bind to one of the two builds of the kernel (csrc/sim_api.cpp picks from the configuration; force_large: the wide-field one)."""
        h = ctypes.c_void_p()
        # the build is an ARGUMENT (round 3 set the process-wide OCTA_SIM_BUILD around the call: another generator thread creating a
        # simulator in that window got the wide-field build too, and setenv raced with the library's getenv)
        _native.call("octa_sim_create_ex", self._ctx, ctypes.byref(self._cfg), self.batch, 2 if force_large else 0, ctypes.byref(h))
        self._h = h
        self.is_large = bool(self._lib.octa_sim_is_large(h))      # bound to the wide-field build

    def close(self):
        if getattr(self, "_h", None):
            self._lib.octa_sim_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _launch(self, call):
        """Run `call` (one of the octa_sim_run* entry points on self._h). When a sample outgrew the DEFAULT build's per-sample capacities
        (sized for 3 x 3 mm^2: 14 336 nodes per forest, 13 312 sinks ...), bind to the wide-field build -- the same phase code with
        2^17 / 2^18, same bytes where both fit (tests/test_sim_gpu.py) -- and run again. OCTA_SIM_BUILD=default keeps the error."""
        if getattr(self, "_rebound", False):      # the previous batch outgrew the default build: THIS one starts on the configuration's own build again
            self._rebound = False
            self.close()
            self._create()
        rc = call()
        if rc == -3 and not self.is_large and os.environ.get("OCTA_SIM_BUILD") != "default":
            stats = np.zeros((self.batch, 32), np.int64)
            _native.call("octa_sim_stats", self._h, stats.ctypes.data)
            bits = int(np.bitwise_or.reduce(stats[:, 0]))
            CAPACITY = 1 | 2 | 4 | 8 | 16 | 32 | 64 | 256 | 512       # node, O2, CO2, group, pair, set, uniform-stream, request, accepted-sink capacities
            if bits and not (bits & ~CAPACITY):
                import warnings
                warnings.warn(f"the default simulator build ran out of per-sample capacity (error bits {bits:#x}); re-running on the wide-field build")
                self.close()
                self._create(force_large=True)
                self._rebound = True
                rc = call()
        return rc

    def run(self, seeds, py_seeds=None):
        """seeds[k] seeds numpy's stream of sample k; py_seeds (default: the same values) CPython's."""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        if len(seeds) != self.batch:
            raise ValueError(f"expected {self.batch} seeds")
        py = np.ascontiguousarray(seeds if py_seeds is None else py_seeds, dtype=np.uint64)
        rc = self._launch(lambda: self._lib.octa_sim_run(self._h, seeds.ctypes.data, py.ctypes.data, self._bif_fn, None, _native.current_stream_ptr()))
        _native.check(rc, "octa_sim_run")
        return self._collect()

    def _collect(self):
        off = np.zeros(self.batch + 1, np.int64)
        n_art = np.zeros(self.batch, np.int64)
        _native.call("octa_sim_edge_offsets", self._h, off.ctypes.data, n_art.ctypes.data)
        edges = d_edges = None
        if self.device_export:
            # the edge list is written by a kernel on the stream of the run and stays in HBM (the rasteriser reads it there); the host
            # copy is made when somebody asks for `.edges`
            import torch
            d_edges = torch.empty((int(off[-1]), 7), dtype=torch.float64, device=torch.device("cuda", self.device_index))
            _native.call("octa_sim_export_edges_device", self._h, d_edges, _native.current_stream_ptr())
        else:
            edges = np.zeros((int(off[-1]), 7))
            _native.call("octa_sim_export_edges", self._h, edges.ctypes.data)
        stats = np.zeros((self.batch, 32), np.int64)
        _native.call("octa_sim_stats", self._h, stats.ctypes.data)
        timing = np.zeros(8)
        _native.call("octa_sim_timing", self._h, timing.ctypes.data)
        svc = np.zeros(5)
        _native.call("octa_sim_service_stats", self._h, svc.ctypes.data)
        res = SimulationResult(edges, off, n_art, stats, d_edges)
        res.spans = np.zeros((self.batch, 2), np.int64)      # 100 MHz device clock: first taken / last left by a workgroup
        _native.call("octa_sim_spans", self._h, res.spans.ctypes.data)
        res.service = dict(tickets=int(svc[0]), max_absence_ms=svc[1], relaunches=int(svc[2]), parked=int(svc[3]), max_callback_ms=svc[4])
        res.timing = dict(kernel_a_ms=timing[0], launches_a=int(timing[1]), kernel_b_ms=timing[2], launches_b=int(timing[3]),
                          loop_wall_ms=timing[4], host_bif_ms=timing[5], bif_requests=int(timing[6]), hbm_bytes=int(timing[7]))
        return res

    def trace(self):
        """int32 [B, n_iter, 4]: arterial nodes, O2 sinks, venous nodes, CO2 sources at the end of every iteration of the last run
        (the reference's per-step statistics, greenhouse.py:129-134)."""
        n_iter = sum(int(m["I"]) for m in self._config["Greenhouse"]["modes"] if int(m["I"]) > 0)
        out = np.zeros((self.batch, n_iter, 4), np.int32)
        if n_iter:
            _native.call("octa_sim_trace", self._h, out.ctypes.data)
        return out

    def fields(self, k):
        cap = 1 << 18 if self.is_large else 16384
        oxy, co2 = np.zeros((cap, 3)), np.zeros((cap, 3))
        no, nc = ctypes.c_int64(), ctypes.c_int64()
        _native.call("octa_sim_fields", self._h, int(k), oxy.ctypes.data, len(oxy), ctypes.byref(no), co2.ctypes.data, len(co2), ctypes.byref(nc))
        return oxy[: no.value].copy(), co2[: nc.value].copy()


    def run_from_states(self, faz_radius, stumps, np_states, py_states):
        """One run for samples whose generators stand where a caller's do (octa_sim_run_states): faz_radius [B], stumps
        [B][2][2 N_trees][3], np_states / py_states [B][625] uint32."""
        faz = np.ascontiguousarray(faz_radius, dtype=np.float64)
        st = np.ascontiguousarray(stumps, dtype=np.float64)
        nps = np.ascontiguousarray(np_states, dtype=np.uint32)
        pys = np.ascontiguousarray(py_states, dtype=np.uint32)
        if faz.shape != (self.batch,) or st.shape != (self.batch, 2, 2 * self._cfg.n_trees, 3) or nps.shape != (self.batch, 625) \
                or pys.shape != (self.batch, 625):
            raise ValueError("run_from_states: array shapes do not match the batch / the forest configuration")
        rc = self._launch(lambda: self._lib.octa_sim_run_states(self._h, faz.ctypes.data, st.ctypes.data, nps.ctypes.data, pys.ctypes.data, self._bif_fn,
                                                                None, _native.current_stream_ptr()))
        _native.check(rc, "octa_sim_run_states")
        return self._collect()

    def np_state(self, k):
        """numpy's MT19937 state of sample k after the run: 624 words + position."""
        out = np.zeros(625, np.uint32)
        _native.call("octa_sim_np_state", self._h, int(k), out.ctypes.data)
        return out


def simulate_batch(config, seeds, device_index=None):
    sim = BatchSimulator(config, len(seeds), device_index)
    try:
        return sim.run(seeds)
    finally:
        sim.close()


def edges_to_csv_text(edges):
    """CSV text exactly as generate_vessel_graph.py:59-66 writes it (graph_io: native formatter)."""
    from .. import graph_io
    return graph_io.edges_to_csv_text(edges)


class Greenhouse:
    """The reference's object API (vessel_graph_generation/greenhouse.py:15-75; use: generate_vessel_graph.py:24-39):

        greenhouse = Greenhouse(config['Greenhouse'])
        art = Forest(config['Forest'], greenhouse.d, greenhouse.r, greenhouse.simspace, nerve_center=..., nerve_radius=...)
        ven = Forest(..., arterial=False, ...)
        greenhouse.set_forests(art, ven); greenhouse.develop_forest()

    The constructors consume the GLOBAL numpy / CPython generators exactly as the reference's do (FAZ radius, stump nodes);
    develop_forest() hands the generators' current states to the device, grows both forests there (one sample), loads the trees back
    into the Forest objects and leaves both global generators where the reference leaves them. For throughput use BatchSimulator
    (B samples per launch); this class is the one-sample drop-in."""

    def __init__(self, config):
        from .simulation_space import SimulationSpace
        self.config = config
        self.modes = config["modes"]
        self.sigma_t = 1
        self.param_scale = config["param_scale"]
        self.d = config["d"] / self.param_scale
        self.r = config["r"] / self.param_scale
        self.FAZ_radius = np.random.normal(config["FAZ_radius_bound"][0] / self.param_scale, config["FAZ_radius_bound"][1] / self.param_scale)
        self.rotation_radius = config["rotation_radius"] / self.param_scale
        self.FAZ_center = config["FAZ_center"]
        self.nerve_center = np.array(config["nerve_center"]) / self.param_scale
        self.nerve_radius = np.array(config["nerve_radius"]) / self.param_scale
        self.simspace = SimulationSpace(config["SimulationSpace"], self.FAZ_center, self.FAZ_radius, nerve_center=self.nerve_center,
                                        nerve_radius=self.nerve_radius)
        self.arterial_forest = self.venous_forest = None
        self.init_params_from_config(self.modes[0])

    def init_params_from_config(self, config):
        for key in MODE_KEYS:
            setattr(self, key, config[key])
        self.sigma_t = 1

    def set_forests(self, arterialForest, venousForest=None):
        self.arterial_forest = arterialForest
        self.venous_forest = venousForest

    def develop_forest(self):
        import random
        if self.arterial_forest is None or self.venous_forest is None:
            raise NotImplementedError("the GPU simulator grows the arterial and the venous forest together: set_forests(arterial, venous)")
        config = {"Greenhouse": self.config, "Forest": self.arterial_forest.config}
        kind, key, pos, has_gauss, _ = np.random.get_state()
        if kind != "MT19937":
            raise RuntimeError("numpy's global generator is not MT19937")
        ver, py_state, gauss_next = random.getstate()
        stumps = np.stack([self.arterial_forest._stump_array(), self.venous_forest._stump_array()])[None]
        sim = BatchSimulator(config, 1)
        try:
            res = sim.run_from_states([self.FAZ_radius], stumps, np.append(np.asarray(key, np.uint32), np.uint32(pos))[None],
                                      np.asarray(py_state, np.uint32)[None])
            after = sim.np_state(0)
            self.oxys, self.co2s = sim.fields(0)
            tr = sim.trace()[0]
            wall = float(res.timing["loop_wall_ms"]) * 1e-3
        finally:
            sim.close()
        self.result = res
        # the reference's per-step statistics (greenhouse.py:72-76, 128-134): lists that start with 0 and gain one entry per iteration;
        # the device records no per-iteration clock, so the run's wall time is spread evenly over time_per_step
        self.art_nodes_per_step = [0] + [int(v) for v in tr[:, 0]]
        self.oxys_per_step = [0] + [int(v) for v in tr[:, 1]]
        self.ven_nodes_per_step = [0] + [int(v) for v in tr[:, 2]]
        self.co2_per_step = [0] + [int(v) for v in tr[:, 3]]
        self.time_per_step = [wall / max(len(tr), 1)] * len(tr)
        art, ven = res.arterial_venous(0)
        kappa = self.modes[-1]["kappa"]
        self.arterial_forest._load_rows(art, kappa)
        self.venous_forest._load_rows(ven, kappa)
        # the generators continue where the reference's stand after its loop: numpy's stream was consumed on the device, CPython's by
        # `random.uniform draws` draws of random.random() (the cached second normal of FAZ_radius' np.random.normal stays cached)
        np.random.set_state((kind, after[:624], int(after[624]), has_gauss, _))
        _native.advance_python_random(int(res.stats[0, 1]))

    def save_stats(self, out_dir: str):
        """The four PNG plots of the reference's Greenhouse.save_stats (greenhouse.py:401-441: final O2 / CO2 sink distributions,
        runtime per iteration, growth over time) from the device run's fields and per-iteration statistics. Needs matplotlib (a
        plotting dependency of the reference, not of the hot path)."""
        import time
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        os.makedirs(out_dir, exist_ok=True)
        for pts, style, title, name in ((self.oxys, "r.", "Final Oxygen Sink Distribution", "oxy_distribution"),
                                        (self.co2s, "b.", "Final CO\u2082 Sink Distribution", "co2_distribution")):
            plt.figure(figsize=(6, 6))
            if len(pts) > 0:
                plt.plot(pts[:, 1], 1 - pts[:, 0], style)
            plt.xlim(0, 1); plt.ylim(0, 1)
            plt.title(title)
            plt.savefig(f"{out_dir}/{name}.png", bbox_inches="tight")
            plt.close()
        plt.figure(figsize=(6, 6))
        plt.plot(self.time_per_step)
        plt.title(f"Runtime Per Iteration (Total={time.strftime('%H:%M:%S', time.gmtime(sum(self.time_per_step)))})")
        plt.xlabel("Iterations"); plt.ylabel("Seconds")
        plt.savefig(f"{out_dir}/time_per_step.png", bbox_inches="tight")
        plt.close()
        plt.figure(figsize=(6, 6))
        plt.plot(self.art_nodes_per_step); plt.plot(self.oxys_per_step); plt.plot(self.ven_nodes_per_step); plt.plot(self.co2_per_step)
        plt.legend(["Arterial Nodes", "Oxygen Sinks", "Venous Nodes", "CO\u2082 Sources"])
        plt.title("Growth Over Time"); plt.xlabel("Iterations"); plt.ylabel("Amount")
        plt.savefig(f"{out_dir}/growth_over_time.png", bbox_inches="tight")
        plt.close()
