"""ctypes binding to libwr_devkat.so (tests/native/dev_kat.hip): the device
functions of csrc/wr_devmath.h and csrc/wr_libm.h run by themselves on the GPU.

Test infrastructure, not part of libwinmad_rt.so.  The library is built by the
product Makefile's `all` (`__graft_entry__.build()`); if it is missing, lib()
raises with the make command -- the GPU tests then fail, they do not skip.
"""
import ctypes as C
import os

import numpy as np

from winmad_rt import native

# WR_DEVKAT_SO selects another build of the harness (e.g. one with a deliberately wrong function, to see the tests fail)
SO = os.environ.get("WR_DEVKAT_SO") or os.path.join(native.PKG_DIR, "libwr_devkat.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        native._share_torch_runtime()  # one HIP runtime per process, as for libwinmad_rt.so
        if not os.path.exists(SO):
            raise RuntimeError(f"{SO} missing: build it with `make -C {native.PKG_DIR} libwr_devkat.so`")
        L = C.CDLL(SO)
        P, I, I64 = C.c_void_p, C.c_int, C.c_int64
        L.dk_last_error.restype = C.c_char_p
        L.dk_scene_load.argtypes = [C.c_char_p, C.POINTER(P)]
        L.dk_scene_free.argtypes = [P]
        L.dk_scene_free.restype = None
        L.dk_scene_nmats.argtypes = [P]
        L.dk_scene_nlights.argtypes = [P]
        L.dk_sampler.argtypes = [I64, P, P, P, P, P, P]
        L.dk_frame.argtypes = [I64, P, P, P, P]
        L.dk_bsdf.argtypes = [P, I64, P, P, P, P, P, P, P]
        L.dk_light.argtypes = [P, I64, P, P, P, P, P, P, P]
        L.dk_camera.argtypes = [P, I64, P, P, P]
        L.dk_rng.argtypes = [I64, P, I, P, P, P]
        L.dk_libm.argtypes = [I, I64, P, P, P, P]
        L.dk_libm_expected.argtypes = [I, I64, P, P, P, P]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise RuntimeError("libwr_devkat: " + lib().dk_last_error().decode())


def _a(x, dtype, shape):
    x = np.ascontiguousarray(x, dtype)
    if x.shape != shape:
        raise ValueError(f"expected shape {shape}, got {x.shape}")
    return x


def _p(x):
    return x.ctypes.data_as(C.c_void_p)


F, I32 = np.float32, np.int32
SIN, COS, SINCOS, POW = 0, 1, 2, 3


def sampler(u, power, tri, k, tot):
    """(n, 15): cr_kat_sampler (9; slot 7 stays -7), cr_kat_triangle (3), cr_kat_strat (3)."""
    n = len(u)
    u, power, tri = _a(u, F, (n, 3)), _a(power, F, (n,)), _a(tri, F, (n, 9))
    k, tot = _a(k, I32, (n,)), _a(tot, I32, (n,))
    out = np.zeros((n, 15), F)
    _check(lib().dk_sampler(n, _p(u), _p(power), _p(tri), _p(k), _p(tot), _p(out)))
    return out


def frame(z, ci, idx):
    """(n, 10): cr_kat_frame (9), cr_kat_fresnel (1)."""
    n = len(z)
    z, ci, idx = _a(z, F, (n, 3)), _a(ci, F, (n,)), _a(idx, F, (n,))
    out = np.zeros((n, 10), F)
    _check(lib().dk_frame(n, _p(z), _p(ci), _p(idx), _p(out)))
    return out


def libm(op, x, y=None, expected=False):
    """wr_sinf / wr_cosf / wr_sincosf / wr_powf of float32 arrays: on the device,
    or (expected=True) from the same header compiled for the host by g++."""
    x = np.ascontiguousarray(x, F).reshape(-1)
    n = x.size
    y = _a(y, F, (n,)) if op == POW else None
    out = np.zeros(n, F)
    out2 = np.zeros(n, F) if op == SINCOS else None
    fn = lib().dk_libm_expected if expected else lib().dk_libm
    _check(fn(op, n, _p(x), _p(y) if y is not None else None, _p(out), _p(out2) if out2 is not None else None))
    return (out, out2) if op == SINCOS else out


def rng(keys4, draws):
    """keys4 (n, 4) uint32 (seed, iteration, subpath, path) -> stream_key (n,) uint64,
    Rng::u32 (n, draws) uint32, Rng::f (n, draws) float32."""
    keys4 = np.ascontiguousarray(keys4, np.uint32)
    n = keys4.shape[0]
    key = np.zeros(n, np.uint64)
    u = np.zeros((n, draws), np.uint32)
    f = np.zeros((n, draws), F)
    _check(lib().dk_rng(n, _p(keys4), draws, _p(key), _p(u), _p(f)))
    return key, u, f


class Scene:
    """A .scene loaded and flattened by the product's host code; its DMat /
    DLight / DCam records are what the kernels read."""

    def __init__(self, path):
        h = C.c_void_p()
        _check(lib().dk_scene_load(os.fsencode(path), C.byref(h)))
        self.h = h
        self.nmats = lib().dk_scene_nmats(h)
        self.nlights = lib().dk_scene_nlights(h)

    def close(self):
        if getattr(self, "h", None):
            lib().dk_scene_free(self.h)
            self.h = None

    __del__ = close

    def bsdf(self, mat, inp, preset):
        """inp (n, 12) = n, wi, wo, r3; preset (26,) fills the rows first.  -> (n, 26), valid (n,)."""
        n = len(mat)
        mat, inp = _a(mat, I32, (n,)), _a(inp, F, (n, 12))
        cols = [np.ascontiguousarray(inp[:, 3 * k:3 * k + 3]) for k in range(4)]
        out = np.ascontiguousarray(np.tile(np.asarray(preset, F), (n, 1)))
        valid = np.zeros(n, I32)
        _check(lib().dk_bsdf(self.h, n, _p(mat), *map(_p, cols), _p(out), _p(valid)))
        return out, valid

    def light(self, li, inp):
        """inp (n, 15) = pos, r3, dr, pr, rd -> (n, 27), the layout of cr_kat_light."""
        n = len(li)
        li, inp = _a(li, I32, (n,)), _a(inp, F, (n, 15))
        cols = [np.ascontiguousarray(inp[:, 3 * k:3 * k + 3]) for k in range(5)]
        out = np.zeros((n, 27), F)
        _check(lib().dk_light(self.h, n, _p(li), *map(_p, cols), _p(out)))
        return out

    def camera(self, xy, w):
        """(n, 7): t_point(r2w, (x, y, 0)), t_point(w2r, w), check_raster of the latter."""
        n = len(xy)
        xy, w = _a(xy, F, (n, 2)), _a(w, F, (n, 3))
        out = np.zeros((n, 7), F)
        _check(lib().dk_camera(self.h, n, _p(xy), _p(w), _p(out)))
        return out
