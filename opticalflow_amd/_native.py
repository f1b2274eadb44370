"""ctypes binding of libvof.so (the C ABI declared in include/vof.h).

There is NO CPU fallback: if the HIP library is missing or cannot be loaded this module raises, and
every solver call needs a real GPU.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# VOF_LIB: alternative build of the library (A/B experiments); default is the in-tree libvof.so
LIB_PATH = os.environ.get("VOF_LIB") or os.path.join(HERE, "csrc", "libvof.so")

K_NAMES = ["rhs", "apply0", "gs0", "gs", "residual", "restrict", "prolong", "galerkin0", "galerkin",
           "coarse_setup", "coarse_solve", "vector", "reduce", "finalize", "functionals", "coarse_tail", "preprocess"]
RESIZE_U8, RESIZE_F64 = 0, 1         # enum vof_resize_arithmetic
INTENSITY_TARGETS = ("blurred", "original")   # VOF_INTENSITY_TARGET_*: the index is the value


class VofParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32),
                ("speed_alpha", C.c_double), ("remodelling_alpha", C.c_double), ("delta_x", C.c_double),
                ("delta_t", C.c_double), ("initial_v_x", C.c_double), ("initial_v_y", C.c_double),
                ("initial_remodelling", C.c_double), ("rtol", C.c_double), ("max_iterations", C.c_int32),
                ("nu_pre", C.c_int32), ("nu_post", C.c_int32), ("reference_quirks", C.c_int32),
                ("coarse_precision", C.c_int32), ("vcycle_precision", C.c_int32), ("nu_pre_coarse", C.c_int32), ("nu_post_coarse", C.c_int32),
                ("w_cycle_level", C.c_int32), ("w_cycle_visits", C.c_int32), ("krylov_method", C.c_int32),
                ("gmres_restart", C.c_int32), ("fallback_after", C.c_int32), ("warm_start_stride", C.c_int32),
                ("preconditioner", C.c_int32), ("reserved0", C.c_int32)]


class VofPairStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("relative_residual", C.c_double),
                ("L1_functional", C.c_double), ("speed_functional", C.c_double),
                ("remodelling_functional", C.c_double), ("batch_ms", C.c_double), ("batch_pairs", C.c_int32),
                ("reserved", C.c_int32)]


STATS_DTYPE = np.dtype([("iterations", np.int32), ("converged", np.int32), ("relative_residual", np.float64),
                        ("L1_functional", np.float64), ("speed_functional", np.float64),
                        ("remodelling_functional", np.float64), ("batch_ms", np.float64), ("batch_pairs", np.int32),
                        ("reserved", np.int32)])
assert STATS_DTYPE.itemsize == C.sizeof(VofPairStats)

VARIATION_DTYPE = np.dtype([("speed_mean", np.float64), ("speed_variance", np.float64), ("remodelling_mean", np.float64),
                            ("remodelling_variance", np.float64), ("L1_functional", np.float64),
                            ("speed_functional", np.float64), ("remodelling_functional", np.float64),
                            ("max_relative_residual", np.float64), ("converged_last", np.int32),
                            ("converged_all", np.int32), ("max_iterations_used", np.int32), ("reserved", np.int32)])
assert VARIATION_DTYPE.itemsize == 80     # sizeof(vof_variation_stats)

BOXSIZE_DTYPE = np.dtype([("speed_mean", np.float64), ("speed_variance", np.float64), ("remodelling_mean", np.float64),
                          ("remodelling_variance", np.float64), ("nonfinite_count", np.int64), ("box_size", np.int32),
                          ("reserved", np.int32)])
assert BOXSIZE_DTYPE.itemsize == 48       # sizeof(vof_boxsize_stats)

BLURSIZE_DTYPE = np.dtype([("speed_mean", np.float64), ("speed_variance", np.float64), ("remodelling_mean", np.float64),
                           ("remodelling_variance", np.float64), ("nonfinite_count", np.int64), ("sigma_index", np.int32),
                           ("reserved", np.int32)])
assert BLURSIZE_DTYPE.itemsize == 48      # sizeof(vof_blursize_stats)

COMPARE_DTYPE = np.dtype([("speed_mean", np.float64), ("speed_variance", np.float64), ("remodelling_mean", np.float64),
                          ("remodelling_variance", np.float64), ("nonfinite_count", np.int64), ("channel", np.int32),
                          ("reserved", np.int32)])
assert COMPARE_DTYPE.itemsize == 48       # sizeof(vof_compare_stats)

_dp = C.POINTER(C.c_double)
_vp = C.c_void_p

# name -> (restype, argtypes); every symbol include/vof.h declares
SIGNATURES = {
    "vof_version": (C.c_int, []),
    "vof_params_size": (C.c_size_t, []),
    "vof_default_params": (C.c_int, [C.POINTER(VofParams), C.c_size_t]),
    "vof_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "vof_destroy": (None, [_vp]),
    "vof_last_error": (C.c_char_p, [_vp]),
    "vof_workspace_bytes": (C.c_size_t, [_vp]),
    "vof_query_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "vof_query_workspace_for": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "vof_device_memory": (C.c_int, [C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "vof_num_levels": (C.c_int, [_vp]),
    "vof_texture_stack_dev": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_double, C.c_double]),
    "vof_bench_sweeps_dev": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(VofParams), C.c_int]),
    "vof_vary_regularisation_host": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(VofParams), _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp]),
    "vof_field_moments_dev": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vof_subsample_dev": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp]),
    "vof_profile_enable": (C.c_int, [_vp, C.c_int]),
    "vof_profile_reset": (C.c_int, [_vp]),
    "vof_profile_filter": (C.c_int, [_vp, C.c_int, C.c_int]),
    "vof_profile_get": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "vof_profile_get_units": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "vof_profile_get_bytes": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "vof_profile_get_moved": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "vof_kernel_name": (C.c_char_p, [C.c_int]),
    "vof_debug_setup": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(VofParams)]),
    "vof_debug_check_canaries": (C.c_int, [_vp]),
    "vof_debug_level_shape": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vof_debug_rhs": (C.c_int, [_vp, _vp]),
    "vof_debug_apply": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "vof_debug_gs": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int]),
    "vof_debug_sweep": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, C.c_int]),
    "vof_debug_smooth": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    "vof_set_fused_sweeps": (C.c_int, [_vp, C.c_int]),
    "vof_debug_restrict": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "vof_debug_resrestrict_u": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    "vof_debug_prolong_add": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "vof_debug_stencil": (C.c_int, [_vp, C.c_int, _vp]),
    "vof_debug_vcycle": (C.c_int, [_vp, _vp, _vp]),
    "vof_debug_coarse_solve": (C.c_int, [_vp, _vp, _vp]),
    "vof_debug_vcycle_apply": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int)]),
}

# the entries the library has twice, NAME_host on host arrays and NAME_dev on device memory: one argument list for the two
TWINS = {
    "vof_solve_stack": [_vp, _vp, C.c_int, C.POINTER(VofParams), _vp, _vp, _vp, _vp, _vp],
    "vof_blur_stack": [_vp, _vp, _vp, C.c_int, _vp, C.c_int],
    "vof_box_flow": [_vp, _vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _vp],
    "vof_liu_shen": [_vp, _vp, C.c_int, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp],
    "vof_vary_boxsize": [_vp, _vp, C.c_int, _vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int,
                         _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp],
    "vof_vary_blursize": [_vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, _vp, C.c_int, _vp,
                          C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp],
    "vof_compare_flows": [_vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                          _vp, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp,
                          _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "vof_adaptive_threshold": [_vp, _vp, C.c_int, C.c_int, C.c_double, C.c_int, _vp, _dp],
    "vof_clahe": [_vp, _vp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, _vp, _dp],
    "vof_resize_area": [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp],
    "vof_farneback": [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, C.c_float,
                      C.c_double, C.c_int, _vp, _vp, _vp],
    "vof_farneback_box": [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_float,
                          C.c_double, C.c_int, _vp, _vp, _vp],
    "vof_flow_filter": [_vp, _vp, C.c_int, _vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _vp],
    "vof_flow_extremes": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, _vp],
    "vof_flow_compare": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, C.c_double, C.c_int, _vp, C.c_int, _vp, C.c_int,
                         _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp],
    "vof_intensity_correct": [_vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp],
    "vof_intensity_hist": [_vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp],
    "vof_piv_upsample": [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp],
    "vof_piv_flow": [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_double, C.c_int, _vp, _vp, _vp, _vp],
    "vof_piv_flow_ex": [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_double, C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_double, C.c_double,
                        C.c_int, _vp],
}
SIGNATURES.update({name + twin: (C.c_int, args) for name, args in TWINS.items() for twin in ("_host", "_dev")})

_lib = None


class VofError(RuntimeError):
    pass


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, same SONAME as /opt/rocm's).  If
    libvof.so pulled in the system runtime first and torch were imported later, the process would hold two runtimes and
    the second one finds no GPU.  Load torch's copy first (without importing torch) so that libvof.so binds to it and the
    process has ONE runtime whichever is used first.  No torch installed: the system runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    hip = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(hip):
        C.CDLL(hip, mode=C.RTLD_GLOBAL)


def load_library(path: str | None = None):
    """Load libvof.so and declare all prototypes.  Raises if the library is absent (build it with
    ``python -m opticalflow_amd.build`` or ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise VofError(f"native library {p} not found: build it with `python -m opticalflow_amd.build` "
                       "(hipcc, gfx950). There is no CPU fallback.")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def default_params(**overrides) -> VofParams:
    lib = load_library()
    p = VofParams()
    if lib.vof_default_params(C.byref(p), C.sizeof(p)) != 0:
        raise VofError(f"vof_params layout mismatch: binding {C.sizeof(p)} bytes, library {lib.vof_params_size()} bytes")
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown solver parameter {k!r}")
        setattr(p, k, v)
    return p


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return C.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):          # torch tensor (device memory)
        return C.c_void_p(a.data_ptr())
    raise TypeError(type(a))


def _edges_and_counts(edges, n):
    """Histogram edges of a sweep of ``n`` entries as float64, the number of bins and zeroed int64 ``(n, bins)`` counts; (None, 0, None)
    without edges."""
    if edges is None:
        return None, 0, None
    edges = np.ascontiguousarray(edges, dtype=np.float64).ravel()
    return edges, edges.size - 1, np.zeros((n, edges.size - 1), dtype=np.int64)


def _probes_and_speeds(probe_locations, n, n_frames):
    """Probe indices as int32 ``(n_probes, 2)`` and zeroed ``(n, n_frames - 1, n_probes)`` speeds; (None, None) without probes."""
    if probe_locations is None:
        return None, None
    pij = np.ascontiguousarray(probe_locations, dtype=np.int32).reshape(-1, 2)
    return pij, np.zeros((n, max(int(n_frames) - 1, 0), pij.shape[0]))


def liu_shen_initial(fields, pairs_shape):
    """The three initial fields of the Liu-Shen flow - numpy arrays or device tensors, each a scalar, an ``(n_i, n_j)`` plane or a
    ``(T - 1, n_i, n_j)`` stack - in the widest of their three forms, as ``Solver.liu_shen`` takes them, and that form's kind: 0 three
    Python floats, 1 contiguous planes, 2 contiguous stacks.  Any other shape is a ``ValueError``."""
    forms = ((), tuple(pairs_shape[1:]), tuple(pairs_shape))
    try:
        kind = max(forms.index(tuple(f.shape)) for f in fields)
    except ValueError:
        raise ValueError(f"initial fields must be scalars, {forms[1]} planes or {forms[2]} stacks") from None
    if kind == 0:
        return [float(f) for f in fields], 0
    return [np.ascontiguousarray(np.broadcast_to(f, forms[kind])) if isinstance(f, np.ndarray) else f.expand(forms[kind]).contiguous()
            for f in fields], kind


class Solver:
    """One context = one device; owns the device workspace for (n_i, n_j) images and a batch of
    ``max_pairs_in_flight`` frame pairs."""

    def __init__(self, n_i: int, n_j: int, max_pairs_in_flight: int, device: int = 0, stream: int | None = None):
        self.lib = load_library()
        self.n_i, self.n_j, self.max_pairs = int(n_i), int(n_j), int(max_pairs_in_flight)
        self.device = int(device)
        h = C.c_void_p()
        rc = self.lib.vof_create(C.byref(h), self.device, self.n_i, self.n_j, self.max_pairs,
                                 C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise VofError("vof_create failed: " + self.lib.vof_last_error(None).decode())
        self.h = h

    # -- lifetime
    def check_canaries(self):
        """VOF_DEBUG_CANARY=1: raises VofError naming the buffer if a kernel wrote outside one (no-op otherwise)."""
        self._check(self.lib.vof_debug_check_canaries(self.h), "vof_debug_check_canaries")

    def close(self):
        if getattr(self, "h", None):
            h, self.h = self.h, None
            rc = self.lib.vof_debug_check_canaries(h)
            msg = self.lib.vof_last_error(h).decode() if rc != 0 else ""
            self.lib.vof_destroy(h)
            if rc != 0:
                raise VofError("device buffer guard regions damaged: " + msg)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            raise VofError(f"{what} failed ({rc}): " + self.lib.vof_last_error(self.h).decode())

    @property
    def workspace_bytes(self):
        return int(self.lib.vof_workspace_bytes(self.h))

    @property
    def num_levels(self):
        return int(self.lib.vof_num_levels(self.h))

    def level_shape(self, level):
        a, b = C.c_int(), C.c_int()
        self._check(self.lib.vof_debug_level_shape(self.h, level, C.byref(a), C.byref(b)), "level_shape")
        return a.value, b.value

    # -- the native twins.  X takes the input stacks, the frame (or pair) count and the output arrays, all numpy arrays or all device
    # memory (torch tensors or raw pointers), float64 and contiguous, and calls the _host or the _dev twin accordingly; X_host converts
    # the movie, allocates numpy outputs, calls X and returns them; X_dev is X under the name its callers know.
    @staticmethod
    def _twin(name, arrays):
        host = [isinstance(a, np.ndarray) for a in arrays if a is not None]
        assert all(host) or not any(host), "host arrays and device memory do not mix in one call"
        return name + ("_host" if host and host[0] else "_dev")

    def _call(self, name, arrays, *args, refusal=None):
        """The twin of ``name`` that ``arrays`` select.  ``refusal``: return code 1 (the stack holds values the entry does not serve) is
        a ValueError of the library's message and the text ``refusal()`` adds."""
        fn = self._twin(name, arrays)
        rc = getattr(self.lib, fn)(self.h, *args)
        if rc == 1 and refusal is not None:
            raise ValueError(self.lib.vof_last_error(self.h).decode() + refusal())
        self._check(rc, fn)

    def _host_movie(self, movie):
        movie = np.ascontiguousarray(movie, dtype=np.float64)
        assert movie.ndim == 3 and movie.shape[1:] == (self.n_i, self.n_j)
        return movie

    def solve(self, movie, n_frames, params: VofParams, v_x, v_y, remodelling, speed=None, stats=True):
        """``vof_solve_stack_*``: the variational flow of ``n_frames`` frames into float64 ``(n_frames - 1, n_i, n_j)`` arrays;
        returns the STATS_DTYPE record of every pair (None without ``stats``)."""
        st = np.zeros(n_frames - 1, dtype=STATS_DTYPE) if stats else None
        self._call("vof_solve_stack", (movie, v_x, v_y, remodelling, speed), _ptr(movie), int(n_frames), C.byref(params), _ptr(v_x),
                   _ptr(v_y), _ptr(remodelling), _ptr(speed), _ptr(st))
        return st

    def solve_host(self, movie: np.ndarray, params: VofParams, want_speed=True):
        movie = np.ascontiguousarray(movie, dtype=np.float64)
        T = movie.shape[0]
        assert movie.shape[1:] == (self.n_i, self.n_j)
        out = [np.empty((T - 1, self.n_i, self.n_j)) for _ in range(4 if want_speed else 3)]
        stats = self.solve(movie, T, params, *out)
        return (*out, stats) if want_speed else (*out, None, stats)

    solve_dev = solve

    def blur(self, movie, out, n_frames, weights: np.ndarray):
        """``vof_blur_stack_*``: Gaussian blur of ``n_frames`` frames with the taps ``weights`` (on device memory ``out`` may alias
        ``movie``)."""
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        self._call("vof_blur_stack", (movie, out), _ptr(movie), _ptr(out), int(n_frames), _ptr(weights), weights.size // 2)

    def blur_host(self, movie: np.ndarray, weights: np.ndarray):
        """Gaussian blur of every frame on the device (host arrays in and out)."""
        movie = np.ascontiguousarray(movie, dtype=np.float64)
        assert movie.shape[1:] == (self.n_i, self.n_j) and np.size(weights) % 2 == 1
        out = np.empty_like(movie)
        self.blur(movie, out, movie.shape[0], weights)
        return out

    blur_dev = blur

    def box_flow(self, movie, n_frames, box_size, delta_x, delta_t, include_remodelling, reference_quirks, v_x, v_y, speed,
                 net_remodelling=None):
        """``vof_box_flow_*``: box least-squares flow (conduct_optical_flow_jit, OF.py:24-157) of ``n_frames`` frames into float64
        ``(n_frames - 1, n_i, n_j)`` arrays; every element of the outputs is written."""
        self._call("vof_box_flow", (movie, v_x, v_y, speed, net_remodelling), _ptr(movie), int(n_frames), int(box_size), float(delta_x),
                   float(delta_t), int(bool(include_remodelling)), int(bool(reference_quirks)), _ptr(v_x), _ptr(v_y), _ptr(speed),
                   _ptr(net_remodelling))

    def box_flow_host(self, movie: np.ndarray, box_size=15, delta_x=1.0, delta_t=1.0, include_remodelling=False,
                      reference_quirks=True):
        """The box flow of a host movie; returns ``(v_x, v_y, speed, net_remodelling)``, float64 ``(T - 1, n_i, n_j)`` each
        (``net_remodelling`` all zero without ``include_remodelling``)."""
        movie = self._host_movie(movie)
        T = movie.shape[0]
        out = [np.empty((max(T - 1, 0), self.n_i, self.n_j)) for _ in range(4)]
        self.box_flow(movie, T, box_size, delta_x, delta_t, include_remodelling, reference_quirks, *out)
        return tuple(out)

    box_flow_dev = box_flow

    def liu_shen(self, movie, n_frames, delta_x, delta_t, alpha, initial_v_x, initial_v_y, initial_remodelling, initial_kind,
                 max_iterations, v_x, v_y, speed, remodelling):
        """``vof_liu_shen_*``: Liu-Shen Jacobi flow (liu_shen_optical_flow_jit, OF.py:426-673) of ``n_frames`` frames into float64
        ``(n_frames - 1, n_i, n_j)`` arrays; every element of the outputs is written.  The initial fields and their kind are what
        ``liu_shen_initial`` returns: three Python floats (kind 0), or planes / stacks (1 / 2) on the side of the movie."""
        initial = [initial_v_x, initial_v_y, initial_remodelling]
        if initial_kind == 0:                # both twins read three host doubles
            initial = [np.array([float(f)]) for f in initial]
        self._call("vof_liu_shen", (movie, v_x, v_y, speed, remodelling), _ptr(movie), int(n_frames), float(delta_x), float(delta_t),
                   float(alpha), *[_ptr(f) for f in initial], int(initial_kind), int(max_iterations), _ptr(v_x), _ptr(v_y), _ptr(speed),
                   _ptr(remodelling))

    def liu_shen_host(self, movie: np.ndarray, delta_x=1.0, delta_t=1.0, alpha=100.0, initial_v_x=0.0, initial_v_y=0.0,
                      initial_remodelling=0.0, max_iterations=10):
        """The Liu-Shen flow of a host movie; returns ``(v_x, v_y, speed, remodelling)``, float64 ``(T - 1, n_i, n_j)`` each.  The
        initial fields are scalars, ``(n_i, n_j)`` planes or ``(T - 1, n_i, n_j)`` stacks."""
        movie = self._host_movie(movie)
        T = movie.shape[0]
        shape = (max(T - 1, 0), self.n_i, self.n_j)
        initial, kind = liu_shen_initial([np.asarray(f, dtype=np.float64) for f in (initial_v_x, initial_v_y, initial_remodelling)], shape)
        out = [np.empty(shape) for _ in range(4)]
        self.liu_shen(movie, T, delta_x, delta_t, alpha, *initial, kind, max_iterations, *out)
        return tuple(out)

    liu_shen_dev = liu_shen

    def vary_regularisation_host(self, movie: np.ndarray, params: VofParams, speed_alphas, remodelling_alphas, weights=None):
        """The whole (speed_alpha, remodelling_alpha) sweep of vary_regularisation on the device; returns a structured
        array (VARIATION_DTYPE) of shape (len(speed_alphas), len(remodelling_alphas))."""
        movie = np.ascontiguousarray(movie, dtype=np.float64)
        assert movie.shape[1:] == (self.n_i, self.n_j)
        sa = np.ascontiguousarray(speed_alphas, dtype=np.float64).ravel()
        ra = np.ascontiguousarray(remodelling_alphas, dtype=np.float64).ravel()
        out = np.zeros((sa.size, ra.size), dtype=VARIATION_DTYPE)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        rc = self.lib.vof_vary_regularisation_host(self.h, _ptr(movie), movie.shape[0], C.byref(params), _ptr(sa), sa.size,
                                                   _ptr(ra), ra.size, _ptr(w), 0 if w is None else w.size // 2, _ptr(out))
        self._check(rc, "vof_vary_regularisation_host")
        return out

    def _sweep_fields(self, n, n_frames, include_remodelling, return_fields):
        """The four host field stacks of a sweep of ``n`` entries; None where not returned (net_remodelling only where it is
        computed)."""
        wanted = (4 if include_remodelling else 3) if return_fields else 0
        return [np.empty((n, max(n_frames - 1, 0), self.n_i, self.n_j)) if f < wanted else None for f in range(4)]

    def vary_boxsize(self, movie, n_frames, box_sizes, delta_x, delta_t, include_remodelling, reference_quirks, weights=None,
                     histogram_edges=None, probe_locations=None, v_x=None, v_y=None, speed=None, net_remodelling=None):
        """``vof_vary_boxsize_*``: the box-size sweep of the box flow in one native call, the blur taps ``weights`` (or None) applied
        first; the optional field stacks are ``(n_boxes, n_frames - 1, n_i, n_j)``.  Returns ``(stats, histograms, probe_speeds)`` as
        host arrays: a BOXSIZE_DTYPE record per box, int64 ``(n_boxes, bins)`` counts or None, ``(n_boxes, n_frames - 1, n_probes)``
        speeds or None."""
        boxes = np.ascontiguousarray(box_sizes, dtype=np.int32).ravel()
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        edges, bins, hist = _edges_and_counts(histogram_edges, boxes.size)
        pij, probes = _probes_and_speeds(probe_locations, boxes.size, n_frames)
        stats = np.zeros(boxes.size, dtype=BOXSIZE_DTYPE)
        fields = (v_x, v_y, speed, net_remodelling)
        self._call("vof_vary_boxsize", (movie, *fields), _ptr(movie), int(n_frames), _ptr(boxes), boxes.size, float(delta_x),
                   float(delta_t), int(bool(include_remodelling)), int(bool(reference_quirks)), _ptr(w), 0 if w is None else w.size // 2,
                   _ptr(edges), bins, _ptr(hist), _ptr(pij), 0 if pij is None else pij.shape[0], _ptr(probes), _ptr(stats),
                   *[_ptr(f) for f in fields])
        return stats, hist, probes

    def vary_boxsize_host(self, movie: np.ndarray, box_sizes, delta_x=1.0, delta_t=1.0, include_remodelling=False,
                          reference_quirks=True, weights=None, histogram_edges=None, probe_locations=None, return_fields=False):
        """The sweep of a host movie; returns ``(stats, histograms, probe_speeds, fields)``, ``fields`` None or ``(v_x, v_y, speed,
        net_remodelling)`` of shape ``(n_boxes, T - 1, n_i, n_j)`` (``net_remodelling`` is None without ``include_remodelling``)."""
        movie = self._host_movie(movie)
        T = movie.shape[0]
        fields = self._sweep_fields(np.size(box_sizes), T, include_remodelling, return_fields)
        out = self.vary_boxsize(movie, T, box_sizes, delta_x, delta_t, include_remodelling, reference_quirks, weights, histogram_edges,
                                probe_locations, *fields)
        return (*out, tuple(fields) if return_fields else None)

    vary_boxsize_dev = vary_boxsize

    def vary_blursize(self, movie, n_frames, taps, box_size, delta_x, delta_t, include_remodelling, reference_quirks,
                      histogram_edges=None, angle_bins=None, intensity_edges=None, probe_locations=None, v_x=None, v_y=None,
                      speed=None, net_remodelling=None):
        """``vof_vary_blursize_*``: the blur sweep of the box flow in one native call; ``taps`` is a list of tap vectors (one blur
        each), the optional field stacks are ``(n, n_frames - 1, n_i, n_j)``.  Returns ``(stats, histograms, angle_histograms,
        weighted_angle_histograms, intensity_histograms, probe_speeds)`` as host arrays: a BLURSIZE_DTYPE record per blur, the
        histograms ``(n, bins)`` or None where not asked for, ``(n, n_frames - 1, n_probes)`` speeds or None."""
        taps = [np.ascontiguousarray(t, dtype=np.float64).ravel() for t in taps]
        n = len(taps)
        radii = np.array([t.size // 2 for t in taps], dtype=np.int32)
        weights = np.concatenate(taps) if taps else np.zeros(0)
        edges, bins, hist = _edges_and_counts(histogram_edges, n)
        iedges, ibins, ihist = _edges_and_counts(intensity_edges, n)
        abins = int(angle_bins or 0)
        ahist = np.zeros((n, abins), dtype=np.int64) if abins else None
        awhist = np.zeros((n, abins)) if abins else None
        pij, probes = _probes_and_speeds(probe_locations, n, n_frames)
        stats = np.zeros(n, dtype=BLURSIZE_DTYPE)
        fields = (v_x, v_y, speed, net_remodelling)
        self._call("vof_vary_blursize", (movie, *fields), _ptr(movie), int(n_frames), _ptr(weights), _ptr(radii), n, int(box_size),
                   float(delta_x), float(delta_t), int(bool(include_remodelling)), int(bool(reference_quirks)), _ptr(edges), bins,
                   _ptr(hist), abins, _ptr(ahist), _ptr(awhist), _ptr(iedges), ibins, _ptr(ihist), _ptr(pij),
                   0 if pij is None else pij.shape[0], _ptr(probes), _ptr(stats), *[_ptr(f) for f in fields])
        return stats, hist, ahist, awhist, ihist, probes

    def vary_blursize_host(self, movie: np.ndarray, taps, box_size, delta_x=1.0, delta_t=1.0, include_remodelling=False,
                           reference_quirks=True, histogram_edges=None, angle_bins=None, intensity_edges=None, probe_locations=None,
                           return_fields=False):
        """The sweep of a host movie; returns the six summaries and ``fields``, None or ``(v_x, v_y, speed, net_remodelling)`` of shape
        ``(n, T - 1, n_i, n_j)`` (``net_remodelling`` is None without ``include_remodelling``)."""
        movie = self._host_movie(movie)
        T = movie.shape[0]
        fields = self._sweep_fields(len(taps), T, include_remodelling, return_fields)
        out = self.vary_blursize(movie, T, taps, box_size, delta_x, delta_t, include_remodelling, reference_quirks, histogram_edges,
                                 angle_bins, intensity_edges, probe_locations, *fields)
        return (*out, tuple(fields) if return_fields else None)

    vary_blursize_dev = vary_blursize

    def compare_flows(self, movie_a, movie_b, n_frames, box_size, delta_x, delta_t, include_remodelling, reference_quirks,
                      weights_a=None, weights_b=None, histogram_edges=None, angle_bins=None, relative_angle_bins=50,
                      joint_speed_edges=None, joint_speed_min_b=None, fields_a=None, fields_b=None):
        """``vof_compare_flows_*``: the box flows of two movies of one shape and their joint statistics in one native call;
        ``weights_a`` / ``weights_b`` are the blur taps of a channel or None, ``joint_speed_edges`` a pair of edge vectors or None,
        ``fields_a`` / ``fields_b`` None or the stacks ``(v_x, v_y, speed[, net_remodelling])`` of a channel, ``(n_frames - 1, n_i,
        n_j)`` each.  Returns ``(stats, histograms, angle_histograms, weighted_angle_histograms, relative_angle_histogram,
        weighted_relative_angle_histogram, joint_speed_histogram, joint_counts)`` as host arrays: a COMPARE_DTYPE record per channel,
        the per-channel histograms ``(2, bins)`` or None where not asked for, the two histograms of the angle between the flows, the
        ``(bins_a, bins_b)`` counts or None, ``(joint non-finite, theta dropped)``."""
        w = [None if t is None else np.ascontiguousarray(t, dtype=np.float64).ravel() for t in (weights_a, weights_b)]
        edges, bins, hist = _edges_and_counts(histogram_edges, 2)
        abins, tbins = int(angle_bins or 0), int(relative_angle_bins)
        ahist = np.zeros((2, abins), dtype=np.int64) if abins else None
        awhist = np.zeros((2, abins)) if abins else None
        thist, twhist = np.zeros(max(tbins, 0), dtype=np.int64), np.zeros(max(tbins, 0))
        jedges, jhist = [None, None], None
        if joint_speed_edges is not None:
            jedges = [np.ascontiguousarray(e, dtype=np.float64).ravel() for e in joint_speed_edges]
            jhist = np.zeros((jedges[0].size - 1, jedges[1].size - 1), dtype=np.int64)
        jmin = None if joint_speed_min_b is None else np.array([joint_speed_min_b], dtype=np.float64)
        jcounts = np.zeros(2, dtype=np.int64)
        stats = np.zeros(2, dtype=COMPARE_DTYPE)
        fields = [(list(f or ()) + [None] * 4)[:4] for f in (fields_a, fields_b)]
        self._call("vof_compare_flows", (movie_a, movie_b, *fields[0], *fields[1]), _ptr(movie_a), _ptr(movie_b), int(n_frames),
                   _ptr(w[0]), 0 if w[0] is None else w[0].size // 2, _ptr(w[1]), 0 if w[1] is None else w[1].size // 2, int(box_size),
                   float(delta_x), float(delta_t), int(bool(include_remodelling)), int(bool(reference_quirks)), _ptr(edges), bins,
                   _ptr(hist), abins, _ptr(ahist), _ptr(awhist), tbins, _ptr(thist), _ptr(twhist), _ptr(jedges[0]),
                   0 if jedges[0] is None else jedges[0].size - 1, _ptr(jedges[1]), 0 if jedges[1] is None else jedges[1].size - 1,
                   _ptr(jmin), _ptr(jhist), _ptr(jcounts), _ptr(stats), *[_ptr(f) for f in fields[0] + fields[1]])
        return stats, hist, ahist, awhist, thist, twhist, jhist, jcounts

    def compare_flows_host(self, movie_a: np.ndarray, movie_b: np.ndarray, box_size, delta_x=1.0, delta_t=1.0, include_remodelling=False,
                           reference_quirks=True, weights_a=None, weights_b=None, histogram_edges=None, angle_bins=None,
                           relative_angle_bins=50, joint_speed_edges=None, joint_speed_min_b=None, return_fields=False):
        """The comparison of two host movies; returns the eight summaries and ``fields``, None or a pair of ``(v_x, v_y, speed,
        net_remodelling)`` of shape ``(T - 1, n_i, n_j)`` (``net_remodelling`` is None without ``include_remodelling``)."""
        movie_a, movie_b = self._host_movie(movie_a), np.ascontiguousarray(movie_b, dtype=np.float64)
        assert movie_b.shape == movie_a.shape
        T = movie_a.shape[0]
        fields = [[f if f is None else f[0] for f in self._sweep_fields(1, T, include_remodelling, return_fields)] for _ in range(2)]
        out = self.compare_flows(movie_a, movie_b, T, box_size, delta_x, delta_t, include_remodelling, reference_quirks, weights_a,
                                 weights_b, histogram_edges, angle_bins, relative_angle_bins, joint_speed_edges, joint_speed_min_b,
                                 fields[0], fields[1])
        return (*out, (tuple(fields[0]), tuple(fields[1])) if return_fields else None)

    compare_flows_dev = compare_flows

    def _preprocess(self, name, movie, n_frames, args, frames_in_flight, out):
        """``vof_adaptive_threshold_*`` or ``vof_clahe_*``; their return code 1 (the stack holds values the reference's integer cast would
        wrap or leave to the platform) is a ValueError."""
        rng = (C.c_double * 3)()
        self._call(name, (movie, out), _ptr(movie), int(n_frames), *args, int(frames_in_flight), _ptr(out), rng,
                   refusal=lambda: f" (max {rng[0]}, min {rng[1]}, non-finite {int(rng[2])})")

    def adaptive_threshold(self, movie, mask, n_frames, window_size=51, threshold=0.0, frames_in_flight=0):
        """``vof_adaptive_threshold_*``: ``apply_adaptive_threshold`` of ``n_frames`` float64 frames, one byte (0 / 1) per pixel out.
        ``frames_in_flight=0`` leaves the chunk size to the library."""
        self._preprocess("vof_adaptive_threshold", movie, n_frames, (int(window_size), float(threshold)), frames_in_flight, mask)

    def adaptive_threshold_host(self, movie: np.ndarray, window_size=51, threshold=0.0, frames_in_flight=0):
        """The same of a host movie (read as float64): bool ``(T, n_i, n_j)``."""
        movie = self._host_movie(movie)
        mask = np.empty(movie.shape, dtype=np.bool_)
        self.adaptive_threshold(movie, mask, movie.shape[0], window_size, threshold, frames_in_flight)
        return mask

    adaptive_threshold_dev = adaptive_threshold

    def clahe(self, movie, out, n_frames, clip_limit, tiles_x, tiles_y, frames_in_flight=0):
        """``vof_clahe_*``: ``apply_clahe`` of ``n_frames`` float64 frames for the tile grid ``tiles_x`` (along n_j) by ``tiles_y``, float64
        frames out (``out`` must not alias ``movie``)."""
        self._preprocess("vof_clahe", movie, n_frames, (float(clip_limit), int(tiles_x), int(tiles_y)), frames_in_flight, out)

    def clahe_host(self, movie: np.ndarray, clip_limit, tiles_x, tiles_y, frames_in_flight=0):
        """The same of a host movie: float64 ``(T, n_i, n_j)``."""
        movie = self._host_movie(movie)
        out = np.empty(movie.shape, dtype=np.float64)
        self.clahe(movie, out, movie.shape[0], clip_limit, tiles_x, tiles_y, frames_in_flight)
        return out

    clahe_dev = clahe

    def resize_area(self, movie, out, n_frames, out_i, out_j, arithmetic, frames_in_flight=0):
        """``vof_resize_area_*``: ``cv2.resize(frame, (out_j, out_i), interpolation=cv2.INTER_AREA)`` of ``n_frames`` float64 frames in
        the arithmetic OpenCV applies to uint8 (``RESIZE_U8``) or float64 (``RESIZE_F64``) frames, float64 ``(n_frames, out_i, out_j)``
        out (``out`` must not alias ``movie``); return code 1 (uint8 arithmetic asked for a stack that holds other values) is a
        ValueError."""
        self._call("vof_resize_area", (movie, out), _ptr(movie), int(n_frames), int(out_i), int(out_j), int(arithmetic),
                   int(frames_in_flight), _ptr(out), refusal=str)

    def resize_area_host(self, movie: np.ndarray, out_i, out_j, arithmetic, frames_in_flight=0):
        """The same of a host movie (read as float64): float64 ``(T, out_i, out_j)``."""
        movie = self._host_movie(movie)
        out = np.empty((movie.shape[0], int(out_i), int(out_j)), dtype=np.float64)
        self.resize_area(movie, out, movie.shape[0], out_i, out_j, arithmetic, frames_in_flight)
        return out

    resize_area_dev = resize_area

    def farneback(self, first, second, n_pairs, plan, iterations, velocity_scale, v_x, v_y, speed, frames_in_flight=0, box=False):
        """``vof_farneback_*`` (``box``: ``vof_farneback_box_*``, OpenCV's default box window of ``plan["winsize"]`` in place of the
        Gaussian one, which takes no window taps): Farnebaeck's flow of the pairs ``(first[k], second[k])`` of two float64 stacks of
        ``n_pairs`` frames (they may be two views of one movie) into three float64 ``(n_pairs, n_i, n_j)`` arrays, none of which may
        alias a stack.  ``plan``: ``optical_flow.farneback_plan``; return code 1 (a non-finite frame) is a ValueError."""
        sizes = np.ascontiguousarray(plan["sizes"], dtype=np.int32).reshape(-1, 2)
        ksizes = np.ascontiguousarray(plan["ksizes"], dtype=np.int32)
        taps = np.ascontiguousarray(np.concatenate(plan["presmooth_taps"]), dtype=np.float32)
        poly = np.ascontiguousarray(np.concatenate([plan["g"], plan["xg"], plan["xxg"]]), dtype=np.float32)
        ig = np.array([plan["ig11"], plan["ig03"], plan["ig33"], plan["ig55"]], dtype=np.float64)
        window = np.ascontiguousarray(plan["window_taps"], dtype=np.float32)
        assert ksizes.size == sizes.shape[0] and taps.size == int(ksizes.sum()) and poly.size == 3 * (2 * int(plan["poly_n"]) + 1)
        assert window.size == int(plan["winsize"]) // 2 + 1
        self._call("vof_farneback_box" if box else "vof_farneback", (first, second, v_x, v_y, speed), _ptr(first), _ptr(second),
                   int(n_pairs), sizes.shape[0], _ptr(sizes), _ptr(ksizes), _ptr(taps), int(plan["poly_n"]), _ptr(poly), _ptr(ig),
                   int(plan["winsize"]), *(() if box else (_ptr(window),)), int(iterations), float(plan["flow_scale"]),
                   float(velocity_scale), int(frames_in_flight), _ptr(v_x), _ptr(v_y), _ptr(speed), refusal=str)

    def farneback_host(self, first: np.ndarray, second: np.ndarray, plan, iterations, velocity_scale=1.0, frames_in_flight=0, box=False):
        """The same of two host stacks (read as float64): ``(v_x, v_y, speed)``, float64 ``(n_pairs, n_i, n_j)`` each."""
        first, second = self._host_movie(first), np.ascontiguousarray(second, dtype=np.float64)
        assert second.shape == first.shape
        out = [np.empty(first.shape, dtype=np.float64) for _ in range(3)]
        self.farneback(first, second, first.shape[0], plan, iterations, velocity_scale, *out, frames_in_flight, box)
        return tuple(out)

    farneback_dev = farneback

    # -- two finished flow results (vof_flowcompare.hpp)
    def flow_filter(self, movie, weights, n_pairs, intensity_threshold, speed_threshold, zero_speed_under_low, v_x, v_y, speed,
                    frames_in_flight=0):
        """``vof_flow_filter_*``: the reference's result filter in place on ``v_x``, ``v_y`` and ``speed`` (float64, ``(n_pairs, n_i,
        n_j)``), ``movie`` the first ``n_pairs`` float64 frames, ``weights`` the blur taps.  Returns ``(low, fast)`` sample counts."""
        weights = np.ascontiguousarray(weights, dtype=np.float64).ravel()
        counts = np.zeros(2, dtype=np.int64)
        self._call("vof_flow_filter", (movie, v_x, v_y, speed), _ptr(movie), int(n_pairs), _ptr(weights), weights.size // 2,
                   float(intensity_threshold), float(speed_threshold), int(bool(zero_speed_under_low)), int(frames_in_flight), _ptr(v_x),
                   _ptr(v_y), _ptr(speed), _ptr(counts))
        return counts

    def flow_extremes(self, stacks, n_pairs, speed_threshold, angle_threshold, reference_quirks=True, frames_in_flight=0):
        """``vof_flow_extremes_*`` of the six stacks ``(v_x_a, v_y_a, speed_a, v_x_b, v_y_b, speed_b)``: float64 ``(3, 2)``, the
        (min, max) of speed a, of speed b and of cos over the samples that take part (+inf, -inf where none does)."""
        out = np.zeros((3, 2), dtype=np.float64)
        self._call("vof_flow_extremes", stacks, *[_ptr(s) for s in stacks], int(n_pairs), float(speed_threshold), float(angle_threshold),
                   int(bool(reference_quirks)), int(frames_in_flight), _ptr(out))
        return out

    def flow_compare(self, stacks, n_pairs, speed_threshold, angle_threshold, reference_quirks, edges_a, edges_b, angle_edges, clamp_angle,
                     frames_in_flight=0):
        """``vof_flow_compare_*`` of the six stacks against the three edge vectors: ``(joint_speed_histogram, angle_histogram,
        counts)``, int64 ``(bins_a, bins_b)``, ``(angle_bins,)`` and the six counters of include/vof.h."""
        edges = [np.ascontiguousarray(e, dtype=np.float64).ravel() for e in (edges_a, edges_b, angle_edges)]
        jhist = np.zeros((edges[0].size - 1, edges[1].size - 1), dtype=np.int64)
        thist = np.zeros(edges[2].size - 1, dtype=np.int64)
        counts = np.zeros(6, dtype=np.int64)
        self._call("vof_flow_compare", stacks, *[_ptr(s) for s in stacks], int(n_pairs), float(speed_threshold), float(angle_threshold),
                   int(bool(reference_quirks)), _ptr(edges[0]), edges[0].size - 1, _ptr(edges[1]), edges[1].size - 1, _ptr(edges[2]),
                   edges[2].size - 1, int(bool(clamp_angle)), int(frames_in_flight), _ptr(jhist), _ptr(thist), _ptr(counts))
        return jhist, thist, counts

    # -- the illumination correction and the intensity histograms (vof_intensity.hpp)
    def intensity_correct(self, movie, n_frames, smoothing_weights, filter_weights, reference_frame, target, out, drift=None,
                          frames_in_flight=0):
        """``vof_intensity_correct_*``: ``out[k] = Tg[k] - G(B[k] - B[reference_frame], filter_weights)`` of ``n_frames`` float64
        frames, ``B`` the movie blurred with ``smoothing_weights`` (None: the movie itself), ``Tg`` ``B`` (``target``
        ``INTENSITY_TARGETS.index("blurred")``) or the movie (``"original"``); ``drift`` (None: not wanted) receives the subtrahend.
        ``out`` and ``drift`` alias neither each other nor ``movie``."""
        w1 = None if smoothing_weights is None else np.ascontiguousarray(smoothing_weights, dtype=np.float64).ravel()
        w2 = np.ascontiguousarray(filter_weights, dtype=np.float64).ravel()
        self._call("vof_intensity_correct", (movie, out, drift), _ptr(movie), int(n_frames), _ptr(w1), 0 if w1 is None else w1.size // 2,
                   _ptr(w2), w2.size // 2, int(reference_frame), int(target), int(frames_in_flight), _ptr(out), _ptr(drift))

    def intensity_hist(self, movie, n_frames, edges, blur_weights=None, frames_in_flight=0):
        """``vof_intensity_hist_*``: ``(counts, nonfinite)``, int64 ``(n_frames, bins)`` and ``(n_frames,)`` host arrays -
        ``np.histogram`` of every float64 frame (blurred with ``blur_weights`` first, if given) against the ``bins + 1`` increasing
        ``edges`` of ``np.linspace``, and the NaN / Inf values per frame."""
        edges = np.ascontiguousarray(edges, dtype=np.float64).ravel()
        w = None if blur_weights is None else np.ascontiguousarray(blur_weights, dtype=np.float64).ravel()
        counts = np.zeros((int(n_frames), edges.size - 1), dtype=np.int64)
        nonfinite = np.zeros(int(n_frames), dtype=np.int64)
        self._call("vof_intensity_hist", (movie,), _ptr(movie), int(n_frames), _ptr(w), 0 if w is None else w.size // 2, _ptr(edges),
                   edges.size - 1, int(frames_in_flight), _ptr(counts), _ptr(nonfinite))
        return counts, nonfinite

    # -- the dense part of convert_PIV_result (vof_piv.hpp)
    def piv_upsample(self, tables, n_frames, v_x, v_y, speed, frames_in_flight=0):
        """``vof_piv_upsample_*``: the Clough-Tocher interpolant of ``n_frames`` frames at every pixel into ``v_x``, ``v_y`` and ``speed``
        (float64, ``(n_frames, n_i, n_j)``, numpy arrays or device memory).  ``tables``: the host tables of include/vof.h by name -
        ``points``, ``values``, ``gradients``, ``transforms`` (float64), ``simplices``, ``neighbours``, ``point_offsets``,
        ``triangle_offsets`` (int32).  Returns ``counts``: pixels outside every triangle, frames without triangles."""
        t = {k: np.ascontiguousarray(tables[k], dtype=np.float64).ravel() for k in ("points", "values", "gradients", "transforms")}
        t.update({k: np.ascontiguousarray(tables[k], dtype=np.int32).ravel()
                  for k in ("simplices", "neighbours", "point_offsets", "triangle_offsets")})
        if t["point_offsets"].size != int(n_frames) + 1 or t["triangle_offsets"].size != int(n_frames) + 1:
            raise ValueError("point_offsets and triangle_offsets hold n_frames + 1 entries")
        n_points, n_triangles = int(t["point_offsets"][-1]), int(t["triangle_offsets"][-1])
        for key, per, n in (("points", 2, n_points), ("values", 2, n_points), ("gradients", 4, n_points), ("transforms", 6, n_triangles),
                            ("simplices", 3, n_triangles), ("neighbours", 3, n_triangles)):
            if t[key].size != per * n:
                raise ValueError(f"{key} holds {t[key].size} numbers, the offsets say {per * n}")
            if t[key].size == 0:
                t[key] = np.zeros(1, dtype=t[key].dtype)            # never a NULL pointer
        counts = np.zeros(2, dtype=np.int64)
        self._call("vof_piv_upsample", (v_x, v_y, speed), int(n_frames), _ptr(t["points"]), _ptr(t["values"]), _ptr(t["gradients"]),
                   _ptr(t["simplices"]), _ptr(t["neighbours"]), _ptr(t["transforms"]), _ptr(t["point_offsets"]),
                   _ptr(t["triangle_offsets"]), int(frames_in_flight), _ptr(v_x), _ptr(v_y), _ptr(speed), _ptr(counts))
        return counts

    # -- conduct_piv (vof_pivflow.hpp)
    def piv_flow(self, movie, n_pairs, window_sizes, search_radii, steps, u, v, correlation, min_correlation=None, frames_in_flight=0, *,
                 deformation=False, outlier_threshold=None, outlier_epsilon=0.1, validate_last=False):
        """``vof_piv_flow_*``: cross-correlation PIV of the ``n_pairs`` pairs of ``movie`` (``n_pairs + 1`` float64 frames) in
        ``len(window_sizes)`` passes into ``u``, ``v`` and ``correlation`` (float64, ``(n_pairs, R, C)`` of the last pass, numpy arrays or
        device memory like the movie).  ``min_correlation=None``: no threshold.  Returns ``counts``, int64 ``(passes, 3)``: flat windows,
        peaks on the border of the search range, vectors under the threshold.

        The call goes through ``vof_piv_flow_ex_*``, which with the keyword-only options left alone is ``vof_piv_flow_*``: ``deformation`` resamples the search regions of the later
        passes by the interpolated vectors of the pass before, ``outlier_threshold`` (``None``: off) runs the normalised median test
        with ``outlier_epsilon`` on the vectors of a pass before the next uses them, and with ``validate_last`` on the returned ones.
        With ``outlier_threshold`` it returns ``(counts, validation_counts)``, the latter int64 ``(passes, 2)``: outliers, filled.  The
        options go to the library as they are: it refuses what ``conduct_piv`` refuses."""
        w, r, s = (np.ascontiguousarray(a, dtype=np.int32).ravel() for a in (window_sizes, search_radii, steps))
        if not (w.size == r.size == s.size >= 1):
            raise ValueError("window_sizes, search_radii and steps hold one entry per pass")
        counts = np.zeros((w.size, 3), dtype=np.int64)
        validation_counts = None if outlier_threshold is None else np.zeros((w.size, 2), dtype=np.int64)
        self._call("vof_piv_flow_ex", (movie, u, v, correlation), _ptr(movie), int(n_pairs), w.size, _ptr(w), _ptr(r), _ptr(s),
                   float("nan") if min_correlation is None else float(min_correlation), int(frames_in_flight), _ptr(u), _ptr(v),
                   _ptr(correlation), _ptr(counts), int(deformation), float("nan") if outlier_threshold is None else float(outlier_threshold),
                   float(outlier_epsilon), int(validate_last), _ptr(validation_counts))
        return counts if validation_counts is None else (counts, validation_counts)

    def field_moments_dev(self, field, n):
        """(mean, population variance) of ``n`` device-resident doubles."""
        m, v = C.c_double(), C.c_double()
        self._check(self.lib.vof_field_moments_dev(self.h, _ptr(field), int(n), C.byref(m), C.byref(v)), "vof_field_moments_dev")
        return m.value, v.value

    def subsample_dev(self, field, n_fields, box, offset, out):
        """out[k, a, b] = field[k, a*box + offset, b*box + offset] on device memory."""
        self._check(self.lib.vof_subsample_dev(self.h, _ptr(field), int(n_fields), int(box), int(offset), _ptr(out)),
                    "vof_subsample_dev")

    def texture_stack_dev(self, out, n_frames, mode_params, frame_offsets, period, scale):
        """Synthetic translating texture written to ``out`` (device, (n_frames, n_i, n_j))."""
        mp = np.ascontiguousarray(mode_params, dtype=np.float64)
        fo = np.ascontiguousarray(frame_offsets, dtype=np.float64)
        assert mp.ndim == 2 and mp.shape[0] == 4 and fo.shape == (n_frames, 2)
        self._check(self.lib.vof_texture_stack_dev(self.h, _ptr(out), int(n_frames), _ptr(mp), mp.shape[1], _ptr(fo),
                                                   float(period), float(scale)), "vof_texture_stack_dev")

    def bench_sweeps(self, movie, n_pairs, params, n_sweeps):
        self._check(self.lib.vof_bench_sweeps_dev(self.h, _ptr(movie), n_pairs, C.byref(params), n_sweeps),
                    "vof_bench_sweeps_dev")

    # -- profiler
    def profile_enable(self, on=True):
        self._check(self.lib.vof_profile_enable(self.h, int(bool(on))), "profile_enable")

    def profile_filter(self, kernel=-1, level=-1):
        kid = K_NAMES.index(kernel) if isinstance(kernel, str) else int(kernel)
        self._check(self.lib.vof_profile_filter(self.h, kid, level), "profile_filter")

    def profile_reset(self):
        self._check(self.lib.vof_profile_reset(self.h), "profile_reset")

    def profile_get(self, kernel: int | str, level: int = -1):
        kid = K_NAMES.index(kernel) if isinstance(kernel, str) else int(kernel)
        n, ms = C.c_int64(), C.c_double()
        self._check(self.lib.vof_profile_get(self.h, kid, level, C.byref(n), C.byref(ms)), "profile_get")
        return n.value, ms.value

    def profile_units(self, kernel: int | str, level: int = -1):
        kid = K_NAMES.index(kernel) if isinstance(kernel, str) else int(kernel)
        u = C.c_int64()
        self._check(self.lib.vof_profile_get_units(self.h, kid, level, C.byref(u)), "profile_get_units")
        return u.value

    def profile_bytes(self, kernel: int | str, level: int = -1):
        kid = K_NAMES.index(kernel) if isinstance(kernel, str) else int(kernel)
        u = C.c_double()
        self._check(self.lib.vof_profile_get_bytes(self.h, kid, level, C.byref(u)), "profile_get_bytes")
        return u.value

    def profile_moved(self, kernel: int | str, level: int = -1):
        kid = K_NAMES.index(kernel) if isinstance(kernel, str) else int(kernel)
        u = C.c_double()
        self._check(self.lib.vof_profile_get_moved(self.h, kid, level, C.byref(u)), "profile_get_moved")
        return u.value

    def profile_table(self):
        rows = []
        for kid, name in enumerate(K_NAMES):
            for lvl in range(16):
                n, ms = self.profile_get(kid, lvl)
                if n:
                    rows.append((name, lvl, n, ms))
        return rows

    # -- debug building blocks (host arrays in, host arrays out)
    def debug_setup(self, movie: np.ndarray, params: VofParams):
        movie = np.ascontiguousarray(movie, dtype=np.float64)
        self._dbg_pairs = movie.shape[0] - 1
        self._check(self.lib.vof_debug_setup(self.h, _ptr(movie), self._dbg_pairs, C.byref(params)), "debug_setup")

    def _vec(self, level):
        ni, nj = self.level_shape(level)
        return (self._dbg_pairs, 3, ni, nj)

    def debug_rhs(self):
        b = np.empty(self._vec(0))
        self._check(self.lib.vof_debug_rhs(self.h, _ptr(b)), "debug_rhs")
        return b

    def debug_apply(self, level, x):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(self._vec(level))
        y = np.empty_like(x)
        self._check(self.lib.vof_debug_apply(self.h, level, _ptr(x), _ptr(y)), "debug_apply")
        return y

    def debug_gs(self, level, x, b, colour):
        x = np.array(x, dtype=np.float64, copy=True).reshape(self._vec(level))
        b = np.ascontiguousarray(b, dtype=np.float64).reshape(self._vec(level))
        self._check(self.lib.vof_debug_gs(self.h, level, _ptr(x), _ptr(b), colour), "debug_gs")
        return x

    def debug_sweep(self, level, x, b, reverse=False, from_zero=False):
        x = np.array(x, dtype=np.float64, copy=True).reshape(self._vec(level))
        b = np.ascontiguousarray(b, dtype=np.float64).reshape(self._vec(level))
        self._check(self.lib.vof_debug_sweep(self.h, level, _ptr(x), _ptr(b), int(reverse), int(from_zero)), "debug_sweep")
        return x

    def debug_smooth(self, level, x, b, nu, reverse=False, from_zero=False):
        x = np.array(x, dtype=np.float64, copy=True).reshape(self._vec(level))
        b = np.ascontiguousarray(b, dtype=np.float64).reshape(self._vec(level))
        self._check(self.lib.vof_debug_smooth(self.h, level, _ptr(x), _ptr(b), int(nu), int(reverse), int(from_zero)), "debug_smooth")
        return x

    def set_fused_sweeps(self, on=True):
        self._check(self.lib.vof_set_fused_sweeps(self.h, int(bool(on))), "set_fused_sweeps")

    def debug_restrict(self, level, fine):
        fine = np.ascontiguousarray(fine, dtype=np.float64).reshape(self._vec(level))
        coarse = np.empty(self._vec(level + 1))
        self._check(self.lib.vof_debug_restrict(self.h, level, _ptr(fine), _ptr(coarse)), "debug_restrict")
        return coarse

    def debug_resrestrict_u(self, level, x_new, x_old=None):
        x_new = np.ascontiguousarray(x_new, dtype=np.float64).reshape(self._vec(level))
        if x_old is not None:
            x_old = np.ascontiguousarray(x_old, dtype=np.float64).reshape(self._vec(level))
        coarse = np.empty(self._vec(level + 1))
        self._check(self.lib.vof_debug_resrestrict_u(self.h, level, _ptr(x_new), _ptr(x_old) if x_old is not None else None,
                                                     _ptr(coarse)), "debug_resrestrict_u")
        return coarse

    def debug_prolong_add(self, level, fine, coarse):
        fine = np.array(fine, dtype=np.float64, copy=True).reshape(self._vec(level))
        coarse = np.ascontiguousarray(coarse, dtype=np.float64).reshape(self._vec(level + 1))
        self._check(self.lib.vof_debug_prolong_add(self.h, level, _ptr(fine), _ptr(coarse)), "debug_prolong_add")
        return fine

    def debug_stencil(self, level):
        ni, nj = self.level_shape(level)
        c = np.empty((self._dbg_pairs, 3, 3, 3, 3, ni, nj))
        self._check(self.lib.vof_debug_stencil(self.h, level, _ptr(c)), "debug_stencil")
        return c

    def debug_vcycle(self, r):
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(self._vec(0))
        e = np.empty_like(r)
        self._check(self.lib.vof_debug_vcycle(self.h, _ptr(r), _ptr(e)), "debug_vcycle")
        return e

    def debug_vcycle_apply(self, r):
        """(y, v, dots, fused): y = M r, v = A y, dots[k] = ((v, r), (v, v)) of pair k."""
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(self._vec(0))
        y, v = np.empty_like(r), np.empty_like(r)
        dots = np.zeros((r.shape[0], 2))
        fused = C.c_int(0)
        self._check(self.lib.vof_debug_vcycle_apply(self.h, _ptr(r), _ptr(y), _ptr(v), _ptr(dots), C.byref(fused)), "debug_vcycle_apply")
        return y, v, dots, bool(fused.value)

    def debug_coarse_solve(self, r):
        last = self.num_levels - 1
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(self._vec(last))
        e = np.empty_like(r)
        self._check(self.lib.vof_debug_coarse_solve(self.h, _ptr(r), _ptr(e)), "debug_coarse_solve")
        return e


def query_workspace(n_i, n_j, pairs, coarse_precision=None, vcycle_precision=None):
    """Device bytes of a context for ``pairs`` frame pairs in flight; the stencil storage depends on the format in use
    (``coarse_precision`` 0..3, default: the library's default format)."""
    if coarse_precision is None and vcycle_precision is None:
        return int(load_library().vof_query_workspace(int(n_i), int(n_j), int(pairs)))
    return int(load_library().vof_query_workspace_for(int(n_i), int(n_j), int(pairs), 3 if coarse_precision is None else int(coarse_precision),
                                                      3 if vcycle_precision is None else int(vcycle_precision)))


def device_memory(device=0):
    f, t = C.c_size_t(), C.c_size_t()
    rc = load_library().vof_device_memory(int(device), C.byref(f), C.byref(t))
    if rc != 0:
        raise VofError("no usable HIP device %d (vof_device_memory rc=%d); this package has no CPU fallback" % (device, rc))
    return f.value, t.value
