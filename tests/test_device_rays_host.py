"""Device-resident ray batches, the part that needs no device (include/winmad_rt.h
wr_camera_rays / wr_trace_closest_dev / wr_occluded_dev / wr_path_radiance_dev,
DESIGN.md 12): the symbols, the refusal of a null context before any device is
touched, and the validation the torch wrappers do before the library sees a
pointer.  The answers are checked on the GPU: tests/test_gpu_device_rays.py.
"""
import ctypes as C

import numpy as np
import pytest

from winmad_rt import native

NEW = ("wr_camera_rays", "wr_trace_closest_dev", "wr_occluded_dev", "wr_path_radiance_dev")


def test_symbols_are_exported_and_the_version_stays():
    L = native.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in native.EXPORTS
    assert L.wr_api_version() == 8


def test_null_context_is_refused_with_a_message():
    L = native.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)  # never read: the context is checked first
    calls = {
        "wr_camera_rays": lambda: L.wr_camera_rays(None, 1, 1, native.FILM_PT, p, 0),
        "wr_trace_closest_dev": lambda: L.wr_trace_closest_dev(None, p, 1, p),
        "wr_occluded_dev": lambda: L.wr_occluded_dev(None, p, p, 1, p),
        "wr_path_radiance_dev": lambda: L.wr_path_radiance_dev(None, p, 1, 7, 5489, 0, p, None, None),
    }
    assert set(calls) == set(NEW)
    for name, call in calls.items():
        assert call() == native.WR_E_ARG, name
        assert L.wr_last_error().decode() != "", name
    assert not buf.any()


def _bad_inputs():
    """name -> a `rays` argument the _t wrappers must refuse, and the word the message carries."""
    torch = pytest.importorskip("torch")
    good = torch.zeros((6, 8), dtype=torch.float32)
    return {
        "numpy": (np.zeros((6, 8), np.float32), "torch tensor"),
        "cpu_tensor": (good, "is_cuda"),
        "float64": (good.double(), "float32"),
        "shape_n7": (torch.zeros((6, 7), dtype=torch.float32), "shape"),
        "non_contiguous": (torch.zeros((6, 16), dtype=torch.float32)[:, ::2], "contiguous"),
    }


@pytest.mark.parametrize("call", ["trace_closest_t", "occluded_t", "path_radiance_t"])
@pytest.mark.parametrize("bad", ["numpy", "cpu_tensor", "float64", "shape_n7", "non_contiguous"])
def test_wrappers_refuse_what_is_not_a_device_tensor(call, bad):
    """No context and no device: the wrapper raises before it touches either."""
    torch = pytest.importorskip("torch")
    rays, word = _bad_inputs()[bad]
    assert tuple(rays.shape) in ((6, 8), (6, 7))
    ctx = native.Context.__new__(native.Context)  # no wr_create: validation comes first
    args = (rays, torch.zeros((6, 3), dtype=torch.float32)) if call == "occluded_t" else (rays,)
    with pytest.raises(ValueError, match=word):
        getattr(ctx, call)(*args)


def test_wrappers_refuse_bad_targets_and_outputs():
    torch = pytest.importorskip("torch")
    ctx = native.Context.__new__(native.Context)
    rays = torch.zeros((6, 8), dtype=torch.float32)
    # (the rays themselves are a CPU tensor here, so check the helper the wrappers use directly)
    with pytest.raises(ValueError, match="shape"):
        native._dev_tensor(torch.zeros((5, 3), dtype=torch.float32), "targets", (6, 3), "float32", None)
    with pytest.raises(ValueError, match="int32"):
        native._dev_tensor(torch.zeros((6, 10), dtype=torch.float32), "out", (6, 10), "int32", None)
    with pytest.raises(ValueError, match="uint8"):
        native._dev_tensor(torch.zeros((6,), dtype=torch.int8), "out", (6,), "uint8", None)
    with pytest.raises(ValueError, match="contiguous"):
        native._dev_tensor(torch.zeros((6, 6), dtype=torch.float32)[:, :3], "rgb", (6, 3), "float32", None)
    with pytest.raises(ValueError):
        ctx.occluded_t(rays, np.zeros((6, 3), np.float32))


def test_hit_fields_names_the_columns_of_a_record():
    rec = np.dtype([("t", "f4"), ("p", "f4", 3), ("n", "f4", 3), ("prim", "i4"), ("inside", "i4"), ("mat_id", "i4")])
    assert rec.itemsize == C.sizeof(native.WrHit) == 40
    h = np.zeros(3, rec)
    h["t"], h["p"], h["n"] = [1.5, 2.5, 1e7], np.arange(9).reshape(3, 3), -np.arange(9).reshape(3, 3)
    h["prim"], h["inside"], h["mat_id"] = [4, 0, -1], [1, 0, 0], [-2, 3, 0]
    rows = h.view(np.int32).reshape(3, 10)
    for arr in (rows, pytest.importorskip("torch").from_numpy(rows.copy())):
        f = native.hit_fields(arr)
        for k in rec.names:
            assert np.array_equal(np.asarray(f[k]), h[k]), k
    with pytest.raises(ValueError):
        native.hit_fields(rows[:, :9])
