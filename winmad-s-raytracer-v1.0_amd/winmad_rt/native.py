"""ctypes binding to libwinmad_rt.so (include/winmad_rt.h).

The library is built in-tree (`make -C winmad-s-raytracer-v1.0_amd`, or
`__graft_entry__.build()`).  There is no fallback: if the HIP library cannot be
loaded every call raises.
"""
import ctypes as C
import os
import sys

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# WR_LIB selects another build of the same library (kernel variants under test)
LIB_PATH = os.environ.get("WR_LIB") or os.path.join(PKG_DIR, "libwinmad_rt.so")

WR_OK, WR_E_ARG, WR_E_IO, WR_E_HIP, WR_E_SCENE, WR_E_NODEVICE = 0, -1, -2, -3, -4, -5
K_TRACE, K_SHADE, K_RESOLVE, K_GEN, K_OTHER = 0, 1, 2, 3, 4
TRACE_REFERENCE, TRACE_BVH = 0, 1
INTEGRATOR_BDPT, INTEGRATOR_VCM, INTEGRATOR_PATH = 0, 1, 2

# every entry point declared in include/winmad_rt.h
EXPORTS = ["wr_scene_load", "wr_scene_from_desc", "wr_scene_info_get", "wr_scene_fingerprint", "wr_scene_dump", "wr_scene_free",
           "wr_device_count", "wr_create", "wr_create_multi", "wr_context_devices", "wr_destroy", "wr_comm_unique_id",
           "wr_comm_init", "wr_comm_info", "wr_film_reduce", "wr_set_pipelines", "wr_set_trace_mode", "wr_trace_closest", "wr_occluded",
           "wr_render_bdpt", "wr_render_path", "wr_render_vcm", "wr_path_radiance", "wr_film_write_ppm",
           "wr_film_write_image", "wr_checkpoint_save", "wr_checkpoint_load", "wr_last_error", "wr_api_version",
           "wr_reserve", "wr_request_hw_queues", "wr_render_bdpt_moments", "wr_render_vcm_moments",
           "wr_render_path_moments", "wr_film_error", "wr_render_features", "wr_film_denoise",
           "wr_camera_rays", "wr_trace_closest_dev", "wr_occluded_dev", "wr_path_radiance_dev",
           "wr_bsdf_eval_dev", "wr_bsdf_sample_dev", "wr_light_illuminate_dev", "wr_light_emit_dev",
           "wr_light_radiance_dev", "wr_rng_uniform_dev",
           "wr_points_build_dev", "wr_points_info_get", "wr_points_free", "wr_points_count_dev",
           "wr_points_in_radius_dev", "wr_points_knn_dev",
           "wr_photon_map_build", "wr_photon_map_info_get", "wr_photon_map_read", "wr_photon_map_free",
           "wr_photon_estimate_dev", "wr_render_photon"]
CKPT_BDPT, CKPT_VCM, CKPT_PT = 1, 2, 3
FILM_PT, FILM_BDPT = 0, 1


class WrRay(C.Structure):
    _fields_ = [("o", C.c_float * 3), ("d", C.c_float * 3), ("tmin", C.c_float), ("tmax", C.c_float)]


class WrHit(C.Structure):
    _fields_ = [("t", C.c_float), ("p", C.c_float * 3), ("n", C.c_float * 3), ("prim", C.c_int32),
                ("inside", C.c_int32), ("mat_id", C.c_int32)]


class WrSceneInfo(C.Structure):
    _fields_ = [("nprims", C.c_int32), ("ntriangles", C.c_int32), ("nspheres", C.c_int32),
                ("nlights", C.c_int32), ("nmaterials", C.c_int32), ("kd_depth_max", C.c_int32),
                ("kd_inner", C.c_int32), ("kd_leaves", C.c_int32), ("kd_refs", C.c_int64),
                ("kd_max_stack", C.c_int32), ("missing_files", C.c_int32), ("camera_xres", C.c_float),
                ("camera_yres", C.c_float), ("device_bytes", C.c_int64)]


class WrSceneDesc(C.Structure):
    _fields_ = [("n_prims", C.c_int32), ("prim_type", C.POINTER(C.c_int32)), ("prim_data", C.POINTER(C.c_float)),
                ("prim_mat", C.POINTER(C.c_int32)), ("n_lights", C.c_int32), ("light_tri", C.POINTER(C.c_float)),
                ("light_le", C.POINTER(C.c_float)), ("n_materials", C.c_int32), ("materials", C.POINTER(C.c_float)),
                ("cam_pos", C.c_float * 3), ("cam_fwd", C.c_float * 3), ("cam_up", C.c_float * 3),
                ("cam_xres", C.c_float), ("cam_yres", C.c_float), ("cam_hfov", C.c_float)]


class WrCheckpointInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("kind", C.c_int32), ("done", C.c_int32),
                ("total", C.c_int32), ("seed", C.c_uint32), ("fingerprint", C.c_uint32 * 2)]


class WrBdptParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32),
                ("iter_begin", C.c_int32), ("control_length", C.c_int32), ("max_path_length", C.c_int32),
                ("seed", C.c_uint32), ("faithful", C.c_int32), ("time_kernels", C.c_int32),
                ("count_work", C.c_int32)]


class WrPathParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("max_depth", C.c_int32),
                ("sample_begin", C.c_int32), ("sample_count", C.c_int32), ("seed", C.c_uint32),
                ("time_kernels", C.c_int32), ("count_work", C.c_int32)]


class WrVcmParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32),
                ("iter_begin", C.c_int32), ("min_path_length", C.c_int32), ("max_path_length", C.c_int32),
                ("radius_factor", C.c_float), ("radius_alpha", C.c_float), ("seed", C.c_uint32),
                ("time_kernels", C.c_int32), ("count_work", C.c_int32)]


class WrStats(C.Structure):
    _fields_ = [("closest_rays", C.c_int64), ("shadow_rays", C.c_int64), ("inner_visits", C.c_int64),
                ("leaf_visits", C.c_int64), ("prim_refs", C.c_int64), ("seconds", C.c_double),
                ("kernel_ms", C.c_double * 8), ("kernel_launches", C.c_int64 * 8), ("trace_wall_ms", C.c_double),
                ("vm_queries", C.c_int64), ("vm_found", C.c_int64), ("vm_merged", C.c_int64),
                ("prim_tests", C.c_int64), ("bvh_nodes", C.c_int64), ("bvh_tests", C.c_int64),
                ("kd_replay_steps", C.c_int64), ("fallback_rays", C.c_int64), ("verify_rays", C.c_int64),
                ("verify_mismatches", C.c_int64), ("pipelines", C.c_int64),
                ("deferred_rays", C.c_int64), ("bvh_width", C.c_int64), ("work_bytes", C.c_int64),
                ("work_paths", C.c_int64), ("redone", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("kernel_ms", "kernel_launches")}
        d["kernel_ms"] = list(self.kernel_ms)
        d["kernel_launches"] = list(self.kernel_launches)
        return d


class WrErrorInfo(C.Structure):
    """wr_error_info: what wr_film_error reduces from the two films of a moments render."""
    _fields_ = [("sum_stderr", C.c_double), ("sum_mean", C.c_double), ("rel_stderr", C.c_double),
                ("max_rel_stderr", C.c_double), ("values", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class WrDenoiseParams(C.Structure):
    """wr_denoise_params: the knobs of wr_film_denoise (the defaults are the library's)."""
    _fields_ = [("levels", C.c_int32), ("normal_power", C.c_int32), ("sigma_l", C.c_float), ("sigma_p", C.c_float),
                ("sigma_a", C.c_float)]

    def __init__(self, levels=5, normal_power=7, sigma_l=4.0, sigma_p=0.05, sigma_a=0.1):
        super().__init__(levels, normal_power, sigma_l, sigma_p, sigma_a)


class WrPointsInfo(C.Structure):
    _fields_ = [("n", C.c_int64), ("cell", C.c_float), ("origin", C.c_float * 3), ("buckets", C.c_int64),
                ("max_bucket", C.c_int64), ("device_bytes", C.c_int64)]


class WrPhotonMapParams(C.Structure):
    _fields_ = [("n_caustic", C.c_int32), ("n_indirect", C.c_int32), ("max_path_length", C.c_int32),
                ("max_shots", C.c_int64), ("shot_batch", C.c_int32), ("cell", C.c_float), ("seed", C.c_uint32)]


class WrPhotonMapInfo(C.Structure):
    _fields_ = [("shots", C.c_int64), ("caustic_count", C.c_int32), ("indirect_count", C.c_int32),
                ("caustic_paths", C.c_int64), ("indirect_paths", C.c_int64), ("device_bytes", C.c_int64),
                ("caustic_cell", C.c_float), ("indirect_cell", C.c_float)]


class WrPhotonParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("sample_begin", C.c_int32),
                ("sample_count", C.c_int32), ("knn", C.c_int32), ("max_sqr_dist", C.c_float),
                ("direct_target", C.c_int32), ("seed", C.c_uint32), ("time_kernels", C.c_int32),
                ("count_work", C.c_int32)]


PHOTON_CAUSTIC, PHOTON_INDIRECT = 0, 1


class WrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"winmad_rt error {code}: {msg}")
        self.code = code


_lib = None


def _share_torch_runtime():
    """PyTorch-ROCm ships its own libamdhip64 with the same SONAME
    (libamdhip64.so.7) as /opt/rocm's.  If torch is loaded first, the dynamic
    linker binds libwinmad_rt.so to that copy and the process has ONE HIP
    runtime (device pointers of torch tensors are then valid for wr_* calls).
    Loaded the other way round there would be two runtimes and torch's fails to
    initialise, so torch -- when installed -- is imported before our library."""
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def _hip_is_up():
    torch = sys.modules.get("torch")
    try:
        return torch is not None and torch.cuda.is_initialized()
    except Exception:
        return False


def _request_hw_queues(L):
    """One hardware queue per render pipeline (concurrent
    pipelines): HIP reads GPU_MAX_HW_QUEUES once, when it initialises, and the
    library sizes its pipelines by it.  If HIP is not up yet, ask for 16
    (env WR_HW_QUEUES=n asks for n; a larger GPU_MAX_HW_QUEUES is kept) through
    wr_request_hw_queues -- the library never changes the environment by
    itself.  If torch already initialised HIP, the variable stays as HIP read
    it, so the library starts no more pipelines than there are queues."""
    if _hip_is_up():
        return
    want = 16
    try:
        want = max(1, min(32, int(os.environ.get("WR_HW_QUEUES", "16"))))
    except ValueError:
        pass
    L.wr_request_hw_queues(want)


def lib():
    """Load the in-tree HIP library (raises if it has not been built)."""
    global _lib
    if _lib is None:
        _share_torch_runtime()
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: build it with `make -C {PKG_DIR}` "
                               "(or __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.wr_request_hw_queues.argtypes = [C.c_int]
        _request_hw_queues(L)
        P, I, I64 = C.c_void_p, C.c_int, C.c_int64
        L.wr_scene_load.argtypes = [C.c_char_p, C.POINTER(P)]
        L.wr_scene_from_desc.argtypes = [C.POINTER(WrSceneDesc), C.POINTER(P)]
        L.wr_create_multi.argtypes = [P, C.POINTER(C.c_int), I, C.POINTER(P)]
        L.wr_context_devices.argtypes = [P, C.POINTER(C.c_int), I]
        L.wr_comm_unique_id.argtypes = [C.POINTER(C.c_uint8)]
        L.wr_comm_init.argtypes = [P, C.POINTER(C.c_uint8), I, I]
        L.wr_film_reduce.argtypes = [P, P, I64, I]
        L.wr_comm_info.argtypes = [P, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.wr_checkpoint_save.argtypes = [C.c_char_p, C.POINTER(WrCheckpointInfo), C.POINTER(C.c_float)]
        L.wr_checkpoint_load.argtypes = [C.c_char_p, C.POINTER(WrCheckpointInfo), C.POINTER(C.c_float), I64]
        L.wr_scene_info_get.argtypes = [P, C.POINTER(WrSceneInfo)]
        L.wr_scene_dump.argtypes = [P, C.c_char_p]
        L.wr_scene_fingerprint.argtypes = [P, C.POINTER(C.c_uint64)]
        L.wr_scene_free.argtypes = [P]
        L.wr_scene_free.restype = None
        L.wr_create.argtypes = [P, I, C.POINTER(P)]
        L.wr_destroy.argtypes = [P]
        L.wr_destroy.restype = None
        L.wr_set_pipelines.argtypes = [P, I]
        L.wr_set_trace_mode.argtypes = [P, I]
        L.wr_reserve.argtypes = [P, I, I, I]
        L.wr_trace_closest.argtypes = [P, C.POINTER(WrRay), I64, C.POINTER(WrHit)]
        L.wr_occluded.argtypes = [P, C.POINTER(WrRay), C.POINTER(C.c_float), I64, C.POINTER(C.c_uint8)]
        L.wr_render_bdpt.argtypes = [P, C.POINTER(WrBdptParams), P, I, C.POINTER(WrStats)]
        L.wr_render_path.argtypes = [P, C.POINTER(WrPathParams), P, I, C.POINTER(WrStats)]
        L.wr_render_vcm.argtypes = [P, C.POINTER(WrVcmParams), P, I, C.POINTER(WrStats)]
        L.wr_path_radiance.argtypes = [P, C.POINTER(WrRay), I64, I, C.c_uint32, I, C.POINTER(C.c_float),
                                       C.POINTER(WrStats)]
        L.wr_film_write_ppm.argtypes = [C.POINTER(C.c_float), I, I, C.c_float, C.c_float, I, C.c_char_p]
        L.wr_film_write_image.argtypes = [C.POINTER(C.c_float), I, I, C.c_float, C.c_float, I, C.c_char_p]
        L.wr_render_bdpt_moments.argtypes = [P, C.POINTER(WrBdptParams), P, P, I, C.POINTER(WrStats)]
        L.wr_render_vcm_moments.argtypes = [P, C.POINTER(WrVcmParams), P, P, I, C.POINTER(WrStats)]
        L.wr_render_path_moments.argtypes = [P, C.POINTER(WrPathParams), P, P, I, C.POINTER(WrStats)]
        L.wr_film_error.argtypes = [P, P, P, I, I, I, I, P, C.POINTER(WrErrorInfo)]
        L.wr_render_features.argtypes = [P, I, I, I, P, P, P, P, I, C.POINTER(WrStats)]
        L.wr_film_denoise.argtypes = [P, P, P, I, I, I, P, P, P, C.POINTER(WrDenoiseParams), I, P]
        L.wr_camera_rays.argtypes = [P, I, I, I, P, I]
        L.wr_trace_closest_dev.argtypes = [P, P, I64, P]
        L.wr_occluded_dev.argtypes = [P, P, P, I64, P]
        L.wr_path_radiance_dev.argtypes = [P, P, I64, I, C.c_uint32, I, P, P, C.POINTER(WrStats)]
        U32 = C.c_uint32
        L.wr_bsdf_eval_dev.argtypes = [P, P, P, P, I64, P, P]
        L.wr_bsdf_sample_dev.argtypes = [P, P, P, P, I64, P, P]
        L.wr_light_illuminate_dev.argtypes = [P, P, P, P, I64, P]
        L.wr_light_emit_dev.argtypes = [P, P, P, P, I64, P]
        L.wr_light_radiance_dev.argtypes = [P, P, P, I64, P]
        L.wr_rng_uniform_dev.argtypes = [P, U32, U32, U32, P, P, C.c_int32, I64, P]
        L.wr_points_build_dev.argtypes = [P, P, I64, C.c_float, C.POINTER(P)]
        L.wr_points_info_get.argtypes = [P, C.POINTER(WrPointsInfo)]
        L.wr_points_free.argtypes = [P]
        L.wr_points_free.restype = None
        L.wr_points_count_dev.argtypes = [P, P, P, I64, C.c_float, P, P]
        L.wr_points_in_radius_dev.argtypes = [P, P, P, I64, C.c_float, P, P, I64, P]
        L.wr_points_knn_dev.argtypes = [P, P, P, I64, C.c_int32, C.c_float, P, P, P]
        L.wr_photon_map_build.argtypes = [P, C.POINTER(WrPhotonMapParams), C.POINTER(P), C.POINTER(WrStats)]
        L.wr_photon_map_info_get.argtypes = [P, C.POINTER(WrPhotonMapInfo)]
        L.wr_photon_map_read.argtypes = [P, P, I, P, P, P, P, I]
        L.wr_photon_map_free.argtypes = [P]
        L.wr_photon_map_free.restype = None
        L.wr_photon_estimate_dev.argtypes = [P, P, I, P, P, I64, C.c_int32, C.c_float, P, P, P]
        L.wr_render_photon.argtypes = [P, P, C.POINTER(WrPhotonParams), P, I, C.POINTER(WrStats)]
        L.wr_last_error.restype = C.c_char_p
        _lib = L
    return _lib


def library_sha16():
    """sha256 prefix (16 hex digits) of the library file this process loads:
    ties a measurement (profiles/*/traffic_*.json, lib_sha) to a build."""
    import hashlib
    try:
        with open(LIB_PATH, "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()[:16]
    except OSError:
        return None


def check(rc):
    if rc != WR_OK:
        raise WrError(rc, lib().wr_last_error().decode())
    return rc


def device_count():
    return lib().wr_device_count()


class Scene:
    """Scene::init (scene.cpp:469-489): .scene + .obj + KD tree, host side."""

    def __init__(self, path=None, _handle=None):
        if _handle is not None:
            self.h = _handle
            return
        h = C.c_void_p()
        check(lib().wr_scene_load(os.fsencode(path), C.byref(h)))
        self.h = h

    @classmethod
    def from_desc(cls, prim_type, prim_data, prim_mat, light_tri, light_le, materials, cam_pos, cam_fwd, cam_up,
                  cam_xres, cam_yres, cam_hfov):
        """wr_scene_from_desc: the reference's in-memory Scene as flat arrays
        (include/winmad_rt.h wr_scene_desc): prim_type (n,) int32 0/1,
        prim_data (n, 9) float32, prim_mat (n,) int32, light_tri (m, 9),
        light_le (m, 3), materials (k, 11), camera vectors and raster / FOV."""
        pt = np.ascontiguousarray(prim_type, np.int32).reshape(-1)
        pd = np.ascontiguousarray(prim_data, np.float32).reshape(-1, 9)
        pm = np.ascontiguousarray(prim_mat, np.int32).reshape(-1)
        lt = np.ascontiguousarray(light_tri, np.float32).reshape(-1, 9)
        le = np.ascontiguousarray(light_le, np.float32).reshape(-1, 3)
        mt = np.ascontiguousarray(materials, np.float32).reshape(-1, 11)
        if not (pt.size == pd.shape[0] == pm.size) or lt.shape[0] != le.shape[0]:
            raise ValueError("inconsistent primitive / light array lengths")
        d = WrSceneDesc()
        d.n_prims = pt.size
        d.prim_type = pt.ctypes.data_as(C.POINTER(C.c_int32))
        d.prim_data = pd.ctypes.data_as(C.POINTER(C.c_float))
        d.prim_mat = pm.ctypes.data_as(C.POINTER(C.c_int32))
        d.n_lights = lt.shape[0]
        d.light_tri = lt.ctypes.data_as(C.POINTER(C.c_float))
        d.light_le = le.ctypes.data_as(C.POINTER(C.c_float))
        d.n_materials = mt.shape[0]
        d.materials = mt.ctypes.data_as(C.POINTER(C.c_float))
        for k in range(3):
            d.cam_pos[k], d.cam_fwd[k], d.cam_up[k] = float(cam_pos[k]), float(cam_fwd[k]), float(cam_up[k])
        d.cam_xres, d.cam_yres, d.cam_hfov = float(cam_xres), float(cam_yres), float(cam_hfov)
        h = C.c_void_p()
        check(lib().wr_scene_from_desc(C.byref(d), C.byref(h)))
        return cls(_handle=h)

    def close(self):
        if getattr(self, "h", None):
            lib().wr_scene_free(self.h)
            self.h = None

    __del__ = close

    def info(self):
        i = WrSceneInfo()
        check(lib().wr_scene_info_get(self.h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in i._fields_}

    def fingerprint(self):
        """wr_scene_fingerprint: 64-bit hash of the primitives, lights, materials, camera."""
        v = C.c_uint64()
        check(lib().wr_scene_fingerprint(self.h, C.byref(v)))
        return v.value

    def dump(self, path):
        check(lib().wr_scene_dump(self.h, os.fsencode(path)))
        with open(path) as f:
            return f.read()


def _rays8(rays8):
    """(n, 8) float32 C-contiguous rays (o, d, tmin, tmax); anything else raises."""
    rays8 = np.ascontiguousarray(rays8, np.float32)
    if rays8.ndim != 2 or rays8.shape[1] != 8:
        raise ValueError(f"rays8 must have shape (n, 8), got {rays8.shape}")
    return rays8


def _host_film(film, height, width):
    """The caller's accumulating host film: the library adds height*width*3
    floats into it in place, so it must be exactly a C-contiguous float32
    (height, width, 3) array -- no silent conversion (a copy would drop the
    result, a smaller buffer would be overrun)."""
    if film is None:
        return np.zeros((height, width, 3), np.float32)
    if not isinstance(film, np.ndarray) or film.dtype != np.float32 or film.shape != (height, width, 3) \
            or not film.flags["C_CONTIGUOUS"] or not film.flags["WRITEABLE"]:
        raise ValueError(f"film must be a writeable C-contiguous float32 array of shape ({height}, {width}, 3), "
                         f"got {type(film).__name__} "
                         f"{getattr(film, 'dtype', None)} {getattr(film, 'shape', None)}")
    return film


def _dev_tensor(t, name, shape, dtype, device):
    """A device array of the _t calls: a torch tensor of exactly this dtype
    ("float32", "int32", "uint8") and shape (None: any length), C-contiguous,
    on cuda:`device` (None: not checked).  Anything else raises ValueError --
    nothing is converted or moved, since an output has to be written in place."""
    torch = sys.modules.get("torch")
    if torch is None or not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor on the context's device, got {type(t).__name__} "
                         "(numpy arrays go to the host calls)")
    if t.dtype != getattr(torch, dtype):
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if t.dim() != len(shape) or any(w is not None and w != g for w, g in zip(shape, t.shape)):
        want = "(" + ", ".join("n" if w is None else str(w) for w in shape) + ("," if len(shape) == 1 else "") + ")"
        raise ValueError(f"{name} must have shape {want}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be C-contiguous (strides {tuple(t.stride())})")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (is_cuda), got a {t.device} tensor: host arrays go to the "
                         "host calls")
    if device is not None and t.device.index != device:
        raise ValueError(f"{name} is on cuda:{t.device.index}, the context on cuda:{device}")
    return t


def _join_side_stream(device):
    """The library orders a call after the legacy null stream only: if torch's
    current stream on the device is another one, wait for it here."""
    torch = sys.modules["torch"]
    s = torch.cuda.current_stream(device)
    if s != torch.cuda.default_stream(device):
        s.synchronize()


def hit_fields(hits):
    """The fields of (n, 10) int32 wr_hit records (trace_closest_t's tensor, or a
    numpy array of the same layout) as views: t (n,), p and n (n, 3) float32;
    prim, inside and mat_id (n,) int32."""
    if hits.ndim != 2 or hits.shape[1] != 10:
        raise ValueError(f"hits must have shape (n, 10), got {tuple(hits.shape)}")
    f32 = np.float32 if isinstance(hits, np.ndarray) else sys.modules["torch"].float32
    return {"t": hits[:, 0].view(f32), "p": hits[:, 1:4].view(f32), "n": hits[:, 4:7].view(f32),
            "prim": hits[:, 7], "inside": hits[:, 8], "mat_id": hits[:, 9]}


def _record_fields(rec, words, name, layout):
    """Views of the columns of (n, words) int32 records (a torch tensor or a
    numpy array): layout = (field, first word, last word + 1, is float)."""
    if rec.ndim != 2 or rec.shape[1] != words:
        raise ValueError(f"{name} must have shape (n, {words}), got {tuple(rec.shape)}")
    f32 = np.float32 if isinstance(rec, np.ndarray) else sys.modules["torch"].float32
    out = {}
    for field, lo, hi, is_float in layout:
        col = rec[:, lo] if hi == lo + 1 else rec[:, lo:hi]
        out[field] = col.view(f32) if is_float else col
    return out


def bsdf_info_fields(info):
    """(n, 9) int32 wr_bsdf_info records: valid, is_delta (n,) int32; cos_wi,
    continue_prob, fresnel (n,) and prob (n, 4: diffuse, glossy, reflect, refract) float32."""
    return _record_fields(info, 9, "info", (("valid", 0, 1, False), ("is_delta", 1, 2, False), ("cos_wi", 2, 3, True),
                                            ("continue_prob", 3, 4, True), ("fresnel", 4, 5, True),
                                            ("prob", 5, 9, True)))


def bsdf_eval_fields(ev):
    """(n, 8) int32 wr_bsdf_eval records: f (n, 3); cos_wo, dir_pdf, rev_pdf, pdf, pdf_rev (n,) float32."""
    return _record_fields(ev, 8, "eval", (("f", 0, 3, True), ("cos_wo", 3, 4, True), ("dir_pdf", 4, 5, True),
                                          ("rev_pdf", 5, 6, True), ("pdf", 6, 7, True), ("pdf_rev", 7, 8, True)))


def bsdf_sample_fields(smp):
    """(n, 9) int32 wr_bsdf_sample records: f, wo (n, 3), pdf, cos_wo (n,) float32; type (n,) int32."""
    return _record_fields(smp, 9, "sample", (("f", 0, 3, True), ("wo", 3, 6, True), ("pdf", 6, 7, True),
                                             ("cos_wo", 7, 8, True), ("type", 8, 9, False)))


_LIGHT_LAYOUTS = {
    10: (("le", 0, 3, True), ("dir", 3, 6, True), ("dist", 6, 7, True), ("direct_pdf", 7, 8, True),
         ("emission_pdf", 8, 9, True), ("cos_light", 9, 10, True)),
    12: (("le_cos", 0, 3, True), ("pos", 3, 6, True), ("dir", 6, 9, True), ("emission_pdf", 9, 10, True),
         ("direct_pdf_a", 10, 11, True), ("cos_light", 11, 12, True)),
    5: (("le", 0, 3, True), ("direct_pdf_a", 3, 4, True), ("emission_pdf", 4, 5, True)),
}


def light_fields(rec):
    """The float32 columns of the light calls' records, told apart by their
    width: (n, 10) wr_light_illum (le, dir, dist, direct_pdf, emission_pdf,
    cos_light), (n, 12) wr_light_emission (le_cos, pos, dir, emission_pdf,
    direct_pdf_a, cos_light), (n, 5) wr_light_rad (le, direct_pdf_a, emission_pdf)."""
    if rec.ndim != 2 or rec.shape[1] not in _LIGHT_LAYOUTS:
        raise ValueError(f"light records must have shape (n, 10), (n, 12) or (n, 5), got {tuple(rec.shape)}")
    return _record_fields(rec, rec.shape[1], "light records", _LIGHT_LAYOUTS[rec.shape[1]])


def rays_from_arrays(o, d, tmin=0.0, tmax=1e7):
    n = o.shape[0]
    arr = np.zeros((n, 8), np.float32)
    arr[:, 0:3] = o
    arr[:, 3:6] = d
    arr[:, 6] = tmin
    arr[:, 7] = tmax
    return arr


class Context:
    """Scene resident in HBM on one device (or on several: `devices`, a list of
    HIP device ids, wr_create_multi) + its HIP streams."""

    def __init__(self, scene, device=0, devices=None, trace=None):
        """trace: None keeps the library default (the verified BVH for triangle
        scenes, the KD walk with spheres), else TRACE_REFERENCE / TRACE_BVH."""
        h = C.c_void_p()
        if devices is not None:
            ids = (C.c_int * len(devices))(*devices)
            check(lib().wr_create_multi(scene.h, ids, len(devices), C.byref(h)))
        else:
            check(lib().wr_create(scene.h, device, C.byref(h)))
        self.h = h
        self.scene = scene
        if trace is not None:
            self.set_trace_mode(trace)

    def devices(self):
        buf = (C.c_int * 64)()
        n = lib().wr_context_devices(self.h, buf, 64)
        if n < 0:
            check(n)
        return list(buf[:n])

    def comm_init(self, unique_id, nranks, rank):
        """wr_comm_init: this rank's RCCL communicator (one process per GPU)."""
        idb = (C.c_uint8 * 128)(*bytes(unique_id))
        check(lib().wr_comm_init(self.h, idb, nranks, rank))

    def comm_info(self):
        """wr_comm_info: (ranks, this rank) as the RCCL communicator reports them."""
        n, r = C.c_int(0), C.c_int(0)
        check(lib().wr_comm_info(self.h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def film_reduce(self, film_ptr, nfloat, root=0):
        """wr_film_reduce: sum the ranks' device films into rank `root`'s, in place."""
        check(lib().wr_film_reduce(self.h, C.c_void_p(film_ptr), nfloat, root))

    def set_pipelines(self, n):
        """Concurrent render pipelines (streams) for render_bdpt / render_path."""
        check(lib().wr_set_pipelines(self.h, n))

    def reserve(self, integrator, width, height):
        """wr_reserve: allocate the work buffers of renders of this kind
        (INTEGRATOR_BDPT / _VCM / _PATH) and film size now."""
        check(lib().wr_reserve(self.h, integrator, width, height))

    def set_trace_mode(self, mode):
        """TRACE_REFERENCE (the reference's KD walk) or TRACE_BVH (verified BVH
        search + KD fallback, same answers): include/winmad_rt.h."""
        check(lib().wr_set_trace_mode(self.h, mode))

    def close(self):
        for idx in list(getattr(self, "_points", ())):  # the indices handed out go first (wr_destroy would free them)
            idx.close()
        if getattr(self, "h", None):
            lib().wr_destroy(self.h)
            self.h = None

    __del__ = close

    def trace_closest(self, rays8):
        """rays8: (n, 8) float32 = o, d, tmin, tmax (d used as given)."""
        rays8 = _rays8(rays8)
        n = rays8.shape[0]
        hits = np.zeros(n, dtype=np.dtype([("t", "f4"), ("p", "f4", 3), ("n", "f4", 3), ("prim", "i4"),
                                           ("inside", "i4"), ("mat_id", "i4")]))
        check(lib().wr_trace_closest(self.h, rays8.ctypes.data_as(C.POINTER(WrRay)), n,
                                     hits.ctypes.data_as(C.POINTER(WrHit))))
        return hits

    def occluded(self, rays8, targets):
        rays8 = _rays8(rays8)
        targets = np.ascontiguousarray(targets, np.float32)
        n = rays8.shape[0]
        if targets.shape != (n, 3):
            raise ValueError(f"targets must have shape ({n}, 3), got {targets.shape}")
        out = np.zeros(n, np.uint8)
        check(lib().wr_occluded(self.h, rays8.ctypes.data_as(C.POINTER(WrRay)),
                                targets.ctypes.data_as(C.POINTER(C.c_float)), n,
                                out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    # ---- ray batches that already live on the GPU (wr_*_dev).
    # Every tensor is validated before the library sees its pointer (ValueError);
    # nothing is converted, moved or made contiguous.  Stream rule of all _t
    # calls: the library orders the call after torch's default stream; if
    # torch's current stream on the device is another one, the wrapper
    # synchronises that stream first.  The call returns when its outputs are
    # written, so later torch work on any stream sees them.
    def _dev_args(self, *specs):
        """specs: (tensor, name, shape, dtype).  Returns the context's device index."""
        for t, name, shape, dtype in specs:
            _dev_tensor(t, name, shape, dtype, None)
        dev = self.devices()[0]
        for t, name, shape, dtype in specs:
            _dev_tensor(t, name, shape, dtype, dev)
        _join_side_stream(dev)
        return dev

    def camera_rays(self, width, height, layout=FILM_PT):
        """wr_camera_rays: the rays render_features traces, one per value index
        of a width x height film in `layout`, as an (n, 8) float32 numpy array."""
        rays = np.zeros((width * height, 8), np.float32)
        check(lib().wr_camera_rays(self.h, width, height, layout, rays.ctypes.data_as(C.c_void_p), 0))
        return rays

    def camera_rays_t(self, width, height, layout=FILM_PT):
        """camera_rays as a torch float32 (n, 8) tensor on the context's device,
        written there (nothing crosses to the host)."""
        import torch
        dev = self.devices()[0]
        rays = torch.empty((width * height, 8), dtype=torch.float32, device=f"cuda:{dev}")
        _join_side_stream(dev)
        check(lib().wr_camera_rays(self.h, width, height, layout, C.c_void_p(rays.data_ptr()), 1))
        return rays

    def trace_closest_t(self, rays, out=None):
        """wr_trace_closest_dev: rays is a torch float32 (n, 8) tensor on the
        context's device (o, d, tmin, tmax; d used as given).  Returns an int32
        (n, 10) tensor of wr_hit records (`out` when given, written in place);
        hit_fields() names its columns.  If torch's current stream is not the
        default stream, it is synchronised before the call."""
        import torch
        _dev_tensor(rays, "rays", (None, 8), "float32", None)
        n = rays.shape[0]
        if out is None:
            out = torch.empty((n, 10), dtype=torch.int32, device=rays.device)
        self._dev_args((rays, "rays", (None, 8), "float32"), (out, "out", (n, 10), "int32"))
        check(lib().wr_trace_closest_dev(self.h, C.c_void_p(rays.data_ptr()), n, C.c_void_p(out.data_ptr())))
        return out

    def occluded_t(self, rays, targets, out=None):
        """wr_occluded_dev: rays (n, 8) and targets (n, 3) float32 tensors on the
        context's device.  Returns a uint8 (n,) tensor (`out` when given).  If
        torch's current stream is not the default stream, it is synchronised
        before the call."""
        import torch
        _dev_tensor(rays, "rays", (None, 8), "float32", None)
        n = rays.shape[0]
        _dev_tensor(targets, "targets", (n, 3), "float32", None)
        if out is None:
            out = torch.empty((n,), dtype=torch.uint8, device=rays.device)
        self._dev_args((rays, "rays", (None, 8), "float32"), (targets, "targets", (n, 3), "float32"),
                       (out, "out", (n,), "uint8"))
        check(lib().wr_occluded_dev(self.h, C.c_void_p(rays.data_ptr()), C.c_void_p(targets.data_ptr()), n,
                                    C.c_void_p(out.data_ptr())))
        return out

    def path_radiance_t(self, rays, max_depth=7, seed=5489, sample=0, rgb=None, rgb_sq=None):
        """wr_path_radiance_dev: the radiance of each ray of a torch float32
        (n, 8) tensor on the context's device, ADDED into rgb ((n, 3) float32; a
        new zeroed tensor when None) and, squared per value, into rgb_sq (when
        given): one call per sample index builds the pair film_error reads as
        an n x 1 film.  Returns (rgb, stats).  If torch's current stream is not
        the default stream, it is synchronised before the call."""
        import torch
        _dev_tensor(rays, "rays", (None, 8), "float32", None)
        n = rays.shape[0]
        if rgb is None:
            rgb = torch.zeros((n, 3), dtype=torch.float32, device=rays.device)
        specs = [(rays, "rays", (None, 8), "float32"), (rgb, "rgb", (n, 3), "float32")]
        if rgb_sq is not None:
            specs.append((rgb_sq, "rgb_sq", (n, 3), "float32"))
        self._dev_args(*specs)
        st = WrStats()
        check(lib().wr_path_radiance_dev(self.h, C.c_void_p(rays.data_ptr()), n, max_depth, seed, sample,
                                         C.c_void_p(rgb.data_ptr()),
                                         C.c_void_p(rgb_sq.data_ptr()) if rgb_sq is not None else None, C.byref(st)))
        return rgb, st

    # ---- shading on device arrays (wr_bsdf_*_dev, wr_light_*_dev, wr_rng_uniform_dev;
    # DESIGN.md 13).  Tensors and streams as the _t calls above.  Records come
    # back as (n, words) int32 tensors, like trace_closest_t's hits; the
    # *_fields functions name their columns.
    def _shade_call(self, fn, n, inputs, outputs):
        """inputs / outputs: (tensor, name, shape, dtype); an output that is None
        is made here.  Calls fn(ctx, inputs..., n, outputs...) and returns the outputs."""
        import torch
        for spec in inputs:
            _dev_tensor(*spec, None)
        outs = [(torch.empty(shape, dtype=getattr(torch, dtype), device=inputs[0][0].device) if t is None else t,
                 name, shape, dtype) for t, name, shape, dtype in outputs]
        self._dev_args(*inputs, *outs)
        check(fn(self.h, *[C.c_void_p(a[0].data_ptr()) for a in inputs], n,
                 *[C.c_void_p(a[0].data_ptr()) for a in outs]))
        return [a[0] for a in outs]

    def bsdf_eval_t(self, hits, wi, wo, info=None, out=None):
        """wr_bsdf_eval_dev: hits (n, 10) int32 as trace_closest_t returns them,
        wi and wo (n, 3) float32 (wi = -ray.d).  Returns (info, eval): int32
        (n, 9) wr_bsdf_info and (n, 8) wr_bsdf_eval records (`info` / `out`
        when given, written in place); bsdf_info_fields / bsdf_eval_fields name
        the columns."""
        _dev_tensor(hits, "hits", (None, 10), "int32", None)
        n = hits.shape[0]
        return tuple(self._shade_call(
            lib().wr_bsdf_eval_dev, n,
            [(hits, "hits", (n, 10), "int32"), (wi, "wi", (n, 3), "float32"), (wo, "wo", (n, 3), "float32")],
            [(info, "info", (n, 9), "int32"), (out, "out", (n, 8), "int32")]))

    def bsdf_sample_t(self, hits, wi, r3, info=None, out=None):
        """wr_bsdf_sample_dev: as bsdf_eval_t with r3 (n, 3) float32 uniform
        draws in place of wo.  Returns (info, sample): (n, 9) wr_bsdf_info and
        (n, 9) wr_bsdf_sample records (bsdf_sample_fields)."""
        _dev_tensor(hits, "hits", (None, 10), "int32", None)
        n = hits.shape[0]
        return tuple(self._shade_call(
            lib().wr_bsdf_sample_dev, n,
            [(hits, "hits", (n, 10), "int32"), (wi, "wi", (n, 3), "float32"), (r3, "r3", (n, 3), "float32")],
            [(info, "info", (n, 9), "int32"), (out, "out", (n, 9), "int32")]))

    def light_illuminate_t(self, light, pos, r3, out=None):
        """wr_light_illuminate_dev: light (n,) int32 indices, pos and r3 (n, 3)
        float32.  Returns (n, 10) int32 wr_light_illum records (light_fields)."""
        _dev_tensor(light, "light", (None,), "int32", None)
        n = light.shape[0]
        return self._shade_call(
            lib().wr_light_illuminate_dev, n,
            [(light, "light", (n,), "int32"), (pos, "pos", (n, 3), "float32"), (r3, "r3", (n, 3), "float32")],
            [(out, "out", (n, 10), "int32")])[0]

    def light_emit_t(self, light, dir_r3, pos_r3, out=None):
        """wr_light_emit_dev: light (n,) int32, dir_r3 and pos_r3 (n, 3) float32
        uniform draws.  Returns (n, 12) int32 wr_light_emission records (light_fields)."""
        _dev_tensor(light, "light", (None,), "int32", None)
        n = light.shape[0]
        return self._shade_call(
            lib().wr_light_emit_dev, n,
            [(light, "light", (n,), "int32"), (dir_r3, "dir_r3", (n, 3), "float32"),
             (pos_r3, "pos_r3", (n, 3), "float32")],
            [(out, "out", (n, 12), "int32")])[0]

    def light_radiance_t(self, hits, ray_d, out=None):
        """wr_light_radiance_dev: hits (n, 10) int32, ray_d (n, 3) float32 (the
        direction of the ray that hit).  Returns (n, 5) int32 wr_light_rad
        records (light_fields): zeros unless the hit is on a light."""
        _dev_tensor(hits, "hits", (None, 10), "int32", None)
        n = hits.shape[0]
        return self._shade_call(
            lib().wr_light_radiance_dev, n,
            [(hits, "hits", (n, 10), "int32"), (ray_d, "ray_d", (n, 3), "float32")],
            [(out, "out", (n, 5), "int32")])[0]

    def rng_uniform_t(self, n, draws, seed, iteration, subpath, path=None, ctr=None, out=None):
        """wr_rng_uniform_dev: (n, draws) float32 draws of the counter RNG,
        stream (seed, iteration, subpath, path[k]) for row k (path: (n,) int32
        holding the uint32 values, or None for path k = k).  ctr: (n,) int32
        counters, read and advanced in place (None: every stream from its
        first draw, nothing kept)."""
        if not isinstance(n, int) or not isinstance(draws, int) or n < 0 or not 1 <= draws <= 64:
            raise ValueError(f"n must be an int >= 0 and draws an int in 1..64, got {n!r}, {draws!r}")
        import torch
        specs = [(t, name, (n,), "int32") for t, name in ((path, "path"), (ctr, "ctr")) if t is not None]
        for spec in specs:
            _dev_tensor(*spec, None)
        if out is None:
            dev = specs[0][0].device if specs else f"cuda:{self.devices()[0]}"
            out = torch.empty((n, draws), dtype=torch.float32, device=dev)
        self._dev_args(*specs, (out, "out", (n, draws), "float32"))
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        check(lib().wr_rng_uniform_dev(self.h, seed, iteration, subpath, ptr(path), ptr(ctr), draws, n, ptr(out)))
        return out

    # ---- point sets on the device (wr_points_*)
    def points_index_t(self, pos, cell):
        """wr_points_build_dev: an index over pos, a torch float32 (n, 3) tensor on
        the context's device (copied: pos may change afterwards).  Returns a
        PointsIndex; close it (or leave a `with` block) before the context --
        the context's close closes the indices it handed out."""
        return PointsIndex(self, pos, cell)

    # ---- photon mapping (wr_photon_*, wr_render_photon)
    def photon_map(self, n_caustic=10000, n_indirect=100000, max_path_length=5, max_shots=500000, shot_batch=0,
                   cell=0.0, seed=5489):
        """wr_photon_map_build: PhotonIntegrator::buildPhotonMap.  Returns a
        PhotonMap; close it (or leave a `with` block) before the context."""
        return PhotonMap(self, n_caustic, n_indirect, max_path_length, max_shots, shot_batch, cell, seed)

    def render_photon(self, pmap, width, height, spp, knn=50, max_sqr_dist=0.1, direct_target=0, seed=5489,
                      sample_begin=0, sample_count=0, film=None, film_ptr=None):
        """SurfaceIntegrator::render + PhotonIntegrator::raytracing with the maps
        of pmap (film = SUM over samples, as render_path)."""
        p = WrPhotonParams(width, height, spp, sample_begin, sample_count, knn, max_sqr_dist, direct_target, seed, 0, 0)
        st = WrStats()
        if film_ptr is not None:
            check(lib().wr_render_photon(self.h, pmap.h, C.byref(p), C.c_void_p(film_ptr), 1, C.byref(st)))
            return None, st
        film = _host_film(film, height, width)
        check(lib().wr_render_photon(self.h, pmap.h, C.byref(p), film.ctypes.data_as(C.c_void_p), 0, C.byref(st)))
        return film, st

    def render_bdpt(self, width, height, iterations=1, seed=5489, iter_begin=0, control_length=3,
                    max_path_length=10, faithful=1, time_kernels=0, count_work=0, film=None, film_ptr=None):
        """BidirPathTracing::render.  Host film (numpy, accumulated) or a device
        pointer (film_ptr, e.g. a torch tensor's data_ptr())."""
        p = WrBdptParams(width, height, iterations, iter_begin, control_length, max_path_length, seed,
                         faithful, time_kernels, count_work)
        st = WrStats()
        if film_ptr is not None:
            check(lib().wr_render_bdpt(self.h, C.byref(p), C.c_void_p(film_ptr), 1, C.byref(st)))
            return None, st
        film = _host_film(film, height, width)
        check(lib().wr_render_bdpt(self.h, C.byref(p), film.ctypes.data_as(C.c_void_p), 0, C.byref(st)))
        return film, st

    def render_vcm(self, width, height, iterations=1, seed=5489, iter_begin=0, min_path_length=0,
                   max_path_length=10, radius_factor=0.003, radius_alpha=0.75, time_kernels=0, count_work=0,
                   film=None, film_ptr=None):
        """VertexCM::render (vertex connection and merging).  Film as render_bdpt."""
        p = WrVcmParams(width, height, iterations, iter_begin, min_path_length, max_path_length, radius_factor,
                        radius_alpha, seed, time_kernels, count_work)
        st = WrStats()
        if film_ptr is not None:
            check(lib().wr_render_vcm(self.h, C.byref(p), C.c_void_p(film_ptr), 1, C.byref(st)))
            return None, st
        film = _host_film(film, height, width)
        check(lib().wr_render_vcm(self.h, C.byref(p), film.ctypes.data_as(C.c_void_p), 0, C.byref(st)))
        return film, st

    def path_radiance(self, rays8, max_depth=7, seed=5489, sample=0):
        """PathIntegrator::raytracing for each ray of rays8 ((n, 8) float32:
        o, d, tmin, tmax; d used as given).  Returns (n, 3) radiance, stats."""
        rays8 = _rays8(rays8)
        n = rays8.shape[0]
        out = np.zeros((n, 3), np.float32)
        st = WrStats()
        check(lib().wr_path_radiance(self.h, rays8.ctypes.data_as(C.POINTER(WrRay)), n, max_depth, seed, sample,
                                     out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)))
        return out, st

    def render_path(self, width, height, spp, max_depth=7, seed=5489, sample_begin=0, sample_count=0,
                    time_kernels=0, count_work=0, film=None, film_ptr=None):
        """SurfaceIntegrator::render + PathIntegrator (film = SUM over samples)."""
        p = WrPathParams(width, height, spp, max_depth, sample_begin, sample_count, seed, time_kernels,
                         count_work)
        st = WrStats()
        if film_ptr is not None:
            check(lib().wr_render_path(self.h, C.byref(p), C.c_void_p(film_ptr), 1, C.byref(st)))
            return None, st
        film = _host_film(film, height, width)
        check(lib().wr_render_path(self.h, C.byref(p), film.ctypes.data_as(C.c_void_p), 0, C.byref(st)))
        return film, st

    def _moments(self, fn, p, width, height, film, film_sq, film_ptr, film_sq_ptr):
        """The two films of a moments render: host arrays (made when None,
        accumulated into otherwise) or, with both pointers given, device films."""
        st = WrStats()
        if (film_ptr is None) != (film_sq_ptr is None):
            raise ValueError("film_ptr and film_sq_ptr go together: both films live in the same memory space")
        if film_ptr is not None:
            check(fn(self.h, C.byref(p), C.c_void_p(film_ptr), C.c_void_p(film_sq_ptr), 1, C.byref(st)))
            return None, None, st
        film = _host_film(film, height, width)
        film_sq = _host_film(film_sq, height, width)
        check(fn(self.h, C.byref(p), film.ctypes.data_as(C.c_void_p), film_sq.ctypes.data_as(C.c_void_p), 0,
                 C.byref(st)))
        return film, film_sq, st

    def render_bdpt_moments(self, width, height, iterations=1, seed=5489, iter_begin=0, control_length=3,
                            max_path_length=10, faithful=1, time_kernels=0, count_work=0, film=None, film_sq=None,
                            film_ptr=None, film_sq_ptr=None):
        """wr_render_bdpt_moments: film += the iterations' films (what render_bdpt
        adds), film_sq += their squares per value.  Returns (film, film_sq, stats)."""
        p = WrBdptParams(width, height, iterations, iter_begin, control_length, max_path_length, seed,
                         faithful, time_kernels, count_work)
        return self._moments(lib().wr_render_bdpt_moments, p, width, height, film, film_sq, film_ptr, film_sq_ptr)

    def render_vcm_moments(self, width, height, iterations=1, seed=5489, iter_begin=0, min_path_length=0,
                           max_path_length=10, radius_factor=0.003, radius_alpha=0.75, time_kernels=0, count_work=0,
                           film=None, film_sq=None, film_ptr=None, film_sq_ptr=None):
        """wr_render_vcm_moments.  Films as render_bdpt_moments."""
        p = WrVcmParams(width, height, iterations, iter_begin, min_path_length, max_path_length, radius_factor,
                        radius_alpha, seed, time_kernels, count_work)
        return self._moments(lib().wr_render_vcm_moments, p, width, height, film, film_sq, film_ptr, film_sq_ptr)

    def render_path_moments(self, width, height, spp, max_depth=7, seed=5489, sample_begin=0, sample_count=0,
                            time_kernels=0, count_work=0, film=None, film_sq=None, film_ptr=None, film_sq_ptr=None):
        """wr_render_path_moments: a pass is one sample index of the spp grid
        (strata, not i.i.d.: the error estimate from film_sq is conservative)."""
        p = WrPathParams(width, height, spp, max_depth, sample_begin, sample_count, seed, time_kernels,
                         count_work)
        return self._moments(lib().wr_render_path_moments, p, width, height, film, film_sq, film_ptr, film_sq_ptr)

    def film_error(self, film_ptr, film_sq_ptr, width, height, n_passes, stderr_map_ptr=None):
        """wr_film_error on device films of this context (pointers, e.g. torch
        data_ptr()); stderr_map_ptr: a device film that receives the map."""
        info = WrErrorInfo()
        check(lib().wr_film_error(self.h, C.c_void_p(film_ptr), C.c_void_p(film_sq_ptr), width, height, n_passes, 1,
                                  C.c_void_p(stderr_map_ptr) if stderr_map_ptr is not None else None,
                                  C.byref(info)))
        return info

    def render_features(self, width, height, layout=FILM_PT, normal_ptr=None, albedo_ptr=None, position_ptr=None,
                        depth_ptr=None):
        """wr_render_features: the first-hit feature films of the pixel-centre
        rays, laid out like a radiance film of `layout` (FILM_PT / FILM_BDPT).
        Without pointers: returns ({"normal", "albedo", "position": (height,
        width, 3), "depth": (height, width)} float32 arrays, stats).  With
        device pointers (any subset; None = not wanted) the films are written
        there: returns (None, stats)."""
        st = WrStats()
        ptrs = (normal_ptr, albedo_ptr, position_ptr, depth_ptr)
        if any(p is not None for p in ptrs):
            check(lib().wr_render_features(self.h, width, height, layout,
                                           *[C.c_void_p(p) if p is not None else None for p in ptrs], 1, C.byref(st)))
            return None, st
        out = {"normal": np.zeros((height, width, 3), np.float32), "albedo": np.zeros((height, width, 3), np.float32),
               "position": np.zeros((height, width, 3), np.float32), "depth": np.zeros((height, width), np.float32)}
        check(lib().wr_render_features(self.h, width, height, layout, out["normal"].ctypes.data_as(C.c_void_p),
                                       out["albedo"].ctypes.data_as(C.c_void_p),
                                       out["position"].ctypes.data_as(C.c_void_p),
                                       out["depth"].ctypes.data_as(C.c_void_p), 0, C.byref(st)))
        return out, st

    def film_denoise(self, film_ptr, film_sq_ptr, width, height, n_passes, out_ptr, normal_ptr=None,
                     position_ptr=None, albedo_ptr=None, **params):
        """wr_film_denoise on device films of this context (pointers, e.g. torch
        data_ptr()): out_ptr receives the denoised film at the scale of the
        input film.  params: the fields of WrDenoiseParams."""
        p = WrDenoiseParams(**params)
        opt = [C.c_void_p(x) if x is not None else None for x in (normal_ptr, position_ptr, albedo_ptr)]
        check(lib().wr_film_denoise(self.h, C.c_void_p(film_ptr), C.c_void_p(film_sq_ptr), width, height, n_passes,
                                    *opt, C.byref(p), 1, C.c_void_p(out_ptr)))


class PointsIndex:
    """An index over a point set on the device (include/winmad_rt.h wr_points_*):
    exact radius and k-nearest queries, KdTree::searchInRadius / searchKnn.
    Tensors and streams as the Context's _t calls; a context manager."""

    def __init__(self, ctx, pos, cell):
        self.h = None
        self.ctx = ctx
        cell = float(cell)
        if not (cell > 0.0 and cell < float("inf")):
            raise ValueError(f"cell must be a finite number > 0, got {cell!r}")
        _dev_tensor(pos, "pos", (None, 3), "float32", None)
        ctx._dev_args((pos, "pos", (None, 3), "float32"))
        h = C.c_void_p()
        check(lib().wr_points_build_dev(ctx.h, C.c_void_p(pos.data_ptr()), pos.shape[0], cell, C.byref(h)))
        self.h = h
        if not hasattr(ctx, "_points"):
            ctx._points = []
        ctx._points.append(self)

    def close(self):
        if getattr(self, "h", None):
            lib().wr_points_free(self.h)
            self.h = None
            self.ctx._points.remove(self)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        out = WrPointsInfo()
        check(lib().wr_points_info_get(self.h, C.byref(out)))
        return {"n": out.n, "cell": out.cell, "origin": tuple(out.origin), "buckets": out.buckets,
                "max_bucket": out.max_bucket, "device_bytes": out.device_bytes}

    @staticmethod
    def _radius_args(q, radius, radii):
        """(nq, radius as float): exactly one of radius / radii is given, and q is checked."""
        if (radius is None) == (radii is None):
            raise ValueError("give exactly one of radius (a number) and radii (an (nq,) float32 tensor)")
        if radius is not None:
            radius = float(radius)
            if not radius >= 0.0:
                raise ValueError(f"radius must not be negative or NaN, got {radius!r}")
        _dev_tensor(q, "q", (None, 3), "float32", None)
        nq = q.shape[0]
        if radii is not None:
            _dev_tensor(radii, "radii", (nq,), "float32", None)
            return nq, 0.0
        return nq, radius

    def count_t(self, q, radius=None, radii=None, out=None):
        """wr_points_count_dev: for each row of q ((nq, 3) float32) the number of
        points with |q - p| < radius (or radii[j]), as an int32 (nq,) tensor
        (`out` when given)."""
        import torch
        nq, r = self._radius_args(q, radius, radii)
        if out is None:
            out = torch.empty((nq,), dtype=torch.int32, device=q.device)
        specs = [(q, "q", (nq, 3), "float32"), (out, "out", (nq,), "int32")]
        if radii is not None:
            specs.append((radii, "radii", (nq,), "float32"))
        self.ctx._dev_args(*specs)
        check(lib().wr_points_count_dev(self.ctx.h, self.h, C.c_void_p(q.data_ptr()), nq, r,
                                        C.c_void_p(radii.data_ptr()) if radii is not None else None,
                                        C.c_void_p(out.data_ptr())))
        return out

    def fill_t(self, q, offset, index, radius=None, radii=None):
        """wr_points_in_radius_dev with the caller's offsets ((nq + 1,) int64) and
        index buffer ((capacity,) int32), written in place: query j's indices
        at index[offset[j]:], at most offset[j + 1] - offset[j] of them."""
        nq, r = self._radius_args(q, radius, radii)
        specs = [(q, "q", (nq, 3), "float32"), (offset, "offset", (nq + 1,), "int64"),
                 (index, "index", (None,), "int32")]
        if radii is not None:
            specs.append((radii, "radii", (nq,), "float32"))
        for spec in specs:
            _dev_tensor(*spec, None)
        self.ctx._dev_args(*specs)
        check(lib().wr_points_in_radius_dev(self.ctx.h, self.h, C.c_void_p(q.data_ptr()), nq, r,
                                            C.c_void_p(radii.data_ptr()) if radii is not None else None,
                                            C.c_void_p(offset.data_ptr()), index.shape[0],
                                            C.c_void_p(index.data_ptr())))
        return index

    def in_radius_t(self, q, radius=None, radii=None):
        """The points within the radius of each query: (offset, index), an int64
        (nq + 1,) exclusive scan of the counts and the int32 indices into
        `pos`, query j's at index[offset[j]:offset[j + 1]] in the index's own
        (deterministic, not ascending) order.  Count, torch.cumsum, fill: the
        scan never leaves the device."""
        import torch
        cnt = self.count_t(q, radius, radii)
        offset = torch.zeros((cnt.shape[0] + 1,), dtype=torch.int64, device=q.device)
        offset[1:] = torch.cumsum(cnt, 0, dtype=torch.int64)
        index = torch.empty((int(offset[-1]),), dtype=torch.int32, device=q.device)
        return offset, self.fill_t(q, offset, index, radius, radii)

    def knn_t(self, q, k, max_sqr_dist):
        """wr_points_knn_dev: of the points with d2 < max_sqr_dist the k nearest
        of each query, by (d2, index): (index (nq, k) int32, sqr_dist (nq, k)
        float32, count (nq,) int32); unused slots hold -1 and 0."""
        import torch
        if not isinstance(k, int) or not 1 <= k <= 64:
            raise ValueError(f"k must be an int in 1..64, got {k!r}")
        max_sqr_dist = float(max_sqr_dist)
        if not max_sqr_dist >= 0.0:
            raise ValueError(f"max_sqr_dist must not be negative or NaN, got {max_sqr_dist!r}")
        _dev_tensor(q, "q", (None, 3), "float32", None)
        nq = q.shape[0]
        index = torch.empty((nq, k), dtype=torch.int32, device=q.device)
        sqr = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        cnt = torch.empty((nq,), dtype=torch.int32, device=q.device)
        self.ctx._dev_args((q, "q", (nq, 3), "float32"))
        check(lib().wr_points_knn_dev(self.ctx.h, self.h, C.c_void_p(q.data_ptr()), nq, k, max_sqr_dist,
                                      C.c_void_p(index.data_ptr()), C.c_void_p(sqr.data_ptr()),
                                      C.c_void_p(cnt.data_ptr())))
        return index, sqr, cnt


class PhotonMap:
    """The caustic and indirect photon maps of one photon pass (include/
    winmad_rt.h wr_photon_*), on the context's device; a context manager."""

    def __init__(self, ctx, n_caustic, n_indirect, max_path_length, max_shots, shot_batch, cell, seed):
        self.h = None
        self.ctx = ctx
        p = WrPhotonMapParams(n_caustic, n_indirect, max_path_length, max_shots, shot_batch, float(cell), seed)
        h = C.c_void_p()
        self.stats = WrStats()
        check(lib().wr_photon_map_build(ctx.h, C.byref(p), C.byref(h), C.byref(self.stats)))
        self.h = h
        if not hasattr(ctx, "_points"):
            ctx._points = []
        ctx._points.append(self)  # closed with the context, like its point-set indices

    def close(self):
        if getattr(self, "h", None):
            lib().wr_photon_map_free(self.h)
            self.h = None
            self.ctx._points.remove(self)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        out = WrPhotonMapInfo()
        check(lib().wr_photon_map_info_get(self.h, C.byref(out)))
        return {k: getattr(out, k) for k, _ in out._fields_}

    def count(self, which):
        return self.info()["indirect_count" if which == PHOTON_INDIRECT else "caustic_count"]

    def photons(self, which):
        """The photons of a map as numpy arrays: pos, wi, alpha (n, 3) float32 and shot (n,) int32."""
        n = self.count(which)
        a = {"pos": np.zeros((n, 3), np.float32), "wi": np.zeros((n, 3), np.float32),
             "alpha": np.zeros((n, 3), np.float32), "shot": np.zeros((n,), np.int32)}
        check(lib().wr_photon_map_read(self.ctx.h, self.h, which, *[a[k].ctypes.data_as(C.c_void_p) for k in
                                                                    ("pos", "wi", "alpha", "shot")], 0))
        return a

    def photons_t(self, which):
        """photons() as torch tensors on the context's device (nothing crosses to the host)."""
        import torch
        n = self.count(which)
        dev = f"cuda:{self.ctx.devices()[0]}"
        a = {"pos": torch.zeros((n, 3), dtype=torch.float32, device=dev),
             "wi": torch.zeros((n, 3), dtype=torch.float32, device=dev),
             "alpha": torch.zeros((n, 3), dtype=torch.float32, device=dev),
             "shot": torch.zeros((n,), dtype=torch.int32, device=dev)}
        _join_side_stream(self.ctx.devices()[0])
        check(lib().wr_photon_map_read(self.ctx.h, self.h, which, *[C.c_void_p(a[k].data_ptr()) for k in
                                                                    ("pos", "wi", "alpha", "shot")], 1))
        return a

    def estimate_t(self, which, hits, wo, k=50, max_sqr_dist=0.1):
        """wr_photon_estimate_dev: estimate() at hits ((n, 10) int32 wr_hit
        records) seen from wo ((n, 3) float32).  Returns rgb (n, 3) float32,
        msd (n,) float32 and found (n,) int32."""
        import torch
        _dev_tensor(hits, "hits", (None, 10), "int32", None)
        n = hits.shape[0]
        rgb = torch.zeros((n, 3), dtype=torch.float32, device=hits.device)
        msd = torch.zeros((n,), dtype=torch.float32, device=hits.device)
        found = torch.zeros((n,), dtype=torch.int32, device=hits.device)
        self.ctx._dev_args((hits, "hits", (n, 10), "int32"), (wo, "wo", (n, 3), "float32"))
        check(lib().wr_photon_estimate_dev(self.ctx.h, self.h, which, C.c_void_p(hits.data_ptr()),
                                           C.c_void_p(wo.data_ptr()), n, k, max_sqr_dist, C.c_void_p(rgb.data_ptr()),
                                           C.c_void_p(msd.data_ptr()), C.c_void_p(found.data_ptr())))
        return rgb, msd, found


def film_denoise(film, film_sq, n_passes, normal=None, position=None, albedo=None, **params):
    """wr_film_denoise on host films ((height, width, 3) float32: the sums of
    n_passes passes and of their squares, and the optional guide films of
    render_features): the variance-guided a-trous filter on the CPU -- no
    context, no device.  Returns the denoised film at the scale of `film`.
    params: the fields of WrDenoiseParams (levels, normal_power, sigma_l,
    sigma_p, sigma_a)."""
    film = np.ascontiguousarray(film, np.float32)
    if film.ndim != 3 or film.shape[2] != 3:
        raise ValueError(f"film must have shape (height, width, 3), got {film.shape}")

    def same(a, name):
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.float32)
        if a.shape != film.shape:
            raise ValueError(f"{name} must have the film's shape {film.shape}, got {a.shape}")
        return a

    film_sq = same(film_sq, "film_sq")
    if film_sq is None:
        raise ValueError("film_sq is required")
    guides = [same(normal, "normal"), same(position, "position"), same(albedo, "albedo")]
    h, w = film.shape[:2]
    out = np.zeros_like(film)
    p = WrDenoiseParams(**params)
    check(lib().wr_film_denoise(None, film.ctypes.data_as(C.c_void_p), film_sq.ctypes.data_as(C.c_void_p), w, h,
                                int(n_passes), *[g.ctypes.data_as(C.c_void_p) if g is not None else None for g in guides],
                                C.byref(p), 0, out.ctypes.data_as(C.c_void_p)))
    return out


def film_error(film, film_sq, n_passes, stderr_map=False):
    """wr_film_error on host films ((height, width, 3) float32 sums of n_passes
    passes and of their squares): the standard error of the mean image, on the
    CPU, no device needed.  Returns WrErrorInfo, or (WrErrorInfo, map) with
    stderr_map=True."""
    film = np.ascontiguousarray(film, np.float32)
    film_sq = np.ascontiguousarray(film_sq, np.float32)
    if film.ndim != 3 or film.shape[2] != 3 or film_sq.shape != film.shape:
        raise ValueError(f"film and film_sq must both have shape (height, width, 3), got {film.shape} and "
                         f"{film_sq.shape}")
    h, w = film.shape[:2]
    out = np.zeros_like(film) if stderr_map else None
    info = WrErrorInfo()
    check(lib().wr_film_error(None, film.ctypes.data_as(C.c_void_p), film_sq.ctypes.data_as(C.c_void_p), w, h,
                              int(n_passes), 0, out.ctypes.data_as(C.c_void_p) if stderr_map else None,
                              C.byref(info)))
    return (info, out) if stderr_map else info


def comm_unique_id():
    """wr_comm_unique_id: 128 bytes rank 0 hands to every rank's comm_init."""
    buf = (C.c_uint8 * 128)()
    check(lib().wr_comm_unique_id(buf))
    return bytes(buf)


def checkpoint_save(path, film, kind, done, total, seed, fingerprint=0):
    """wr_checkpoint_save: the accumulated film + how many iterations it sums
    (+ the 64-bit scene / settings fingerprint the resume must match)."""
    film = np.ascontiguousarray(film, np.float32)
    if film.ndim != 3 or film.shape[2] != 3:
        raise ValueError(f"film must have shape (height, width, 3), got {film.shape}")
    info = WrCheckpointInfo(film.shape[1], film.shape[0], kind, done, total, seed,
                            (C.c_uint32 * 2)(fingerprint & 0xFFFFFFFF, (fingerprint >> 32) & 0xFFFFFFFF))
    check(lib().wr_checkpoint_save(os.fsencode(path), C.byref(info), film.ctypes.data_as(C.POINTER(C.c_float))))


def checkpoint_load(path):
    """wr_checkpoint_load -> (film, dict(width, height, kind, done, total, seed, fingerprint))."""
    info = WrCheckpointInfo()
    check(lib().wr_checkpoint_load(os.fsencode(path), C.byref(info), None, 0))
    film = np.zeros((info.height, info.width, 3), np.float32)
    check(lib().wr_checkpoint_load(os.fsencode(path), C.byref(info), film.ctypes.data_as(C.POINTER(C.c_float)),
                                   film.size))
    d = {k: getattr(info, k) for k in ("width", "height", "kind", "done", "total", "seed")}
    d["fingerprint"] = int(info.fingerprint[0]) | (int(info.fingerprint[1]) << 32)
    return film, d


def write_ppm(film, path, scale=1.0, gamma=2.2, transpose=False):
    """ImageFilm::outputImage pipeline (film.cpp:39-64) to a binary PPM."""
    film = np.ascontiguousarray(film, np.float32)
    if film.ndim != 3 or film.shape[2] != 3:
        raise ValueError(f"film must have shape (height, width, 3), got {film.shape}")
    h, w = film.shape[:2]
    check(lib().wr_film_write_ppm(film.ctypes.data_as(C.POINTER(C.c_float)), h, w, scale, gamma,
                                  1 if transpose else 0, os.fsencode(path)))


def write_image(film, path, scale=1.0, gamma=2.2, transpose=False):
    """ImageFilm::outputImage into .ppm / .bmp / .png, or linear .pfm."""
    film = np.ascontiguousarray(film, np.float32)
    if film.ndim != 3 or film.shape[2] != 3:
        raise ValueError(f"film must have shape (height, width, 3), got {film.shape}")
    h, w = film.shape[:2]
    check(lib().wr_film_write_image(film.ctypes.data_as(C.POINTER(C.c_float)), h, w, scale, gamma,
                                    1 if transpose else 0, os.fsencode(path)))
