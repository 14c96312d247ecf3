"""Shading on device arrays, the part that needs no device (include/winmad_rt.h
wr_bsdf_eval_dev / wr_bsdf_sample_dev / wr_light_illuminate_dev / wr_light_emit_dev /
wr_light_radiance_dev / wr_rng_uniform_dev): the symbols, the
refusals that come before any HIP call, the wrappers' validation, the field
views, and the script path tracer of tests/_script_pt.py over the oracle's own
primitives.  The device answers are checked in tests/test_gpu_shading.py.
"""
import ctypes as C

import numpy as np
import pytest

import _oracle
import _scenes
import _script_pt
from winmad_rt import native

NEW = ("wr_bsdf_eval_dev", "wr_bsdf_sample_dev", "wr_light_illuminate_dev", "wr_light_emit_dev",
       "wr_light_radiance_dev", "wr_rng_uniform_dev")


def test_symbols_are_exported_and_the_version_stays():
    L = native.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in native.EXPORTS
    assert L.wr_api_version() == 8


def _calls(L, ctx, n, p):
    return {
        "wr_bsdf_eval_dev": lambda: L.wr_bsdf_eval_dev(ctx, p, p, p, n, None, p),
        "wr_bsdf_sample_dev": lambda: L.wr_bsdf_sample_dev(ctx, p, p, p, n, p, p),
        "wr_light_illuminate_dev": lambda: L.wr_light_illuminate_dev(ctx, p, p, p, n, p),
        "wr_light_emit_dev": lambda: L.wr_light_emit_dev(ctx, p, p, p, n, p),
        "wr_light_radiance_dev": lambda: L.wr_light_radiance_dev(ctx, p, p, n, p),
        "wr_rng_uniform_dev": lambda: L.wr_rng_uniform_dev(ctx, 1, 2, 3, None, None, 3, n, p),
    }


@pytest.mark.parametrize("n", [1, -1])
def test_null_context_and_negative_n_are_refused_before_any_device_call(n):
    """The context comes first, then n: with a context that is not null but is
    never dereferenced (n < 0 is refused before it is looked at) the answer is
    WR_E_ARG as well, and the message names the call."""
    L = native.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)  # never read
    fake = C.c_void_p(buf.ctypes.data)  # stands for a context; only compared with NULL when n < 0
    for ctx in ((None,) if n > 0 else (None, fake)):
        calls = _calls(L, ctx, n, p)
        assert set(calls) == set(NEW)
        for name, call in calls.items():
            assert call() == native.WR_E_ARG, name
            assert name in L.wr_last_error().decode(), name
    assert not buf.any()


def test_record_sizes_and_field_views():
    recs = {
        "info": (np.dtype([("valid", "i4"), ("is_delta", "i4"), ("cos_wi", "f4"), ("continue_prob", "f4"),
                           ("fresnel", "f4"), ("prob", "f4", 4)]), native.bsdf_info_fields, 36),
        "eval": (np.dtype([("f", "f4", 3), ("cos_wo", "f4"), ("dir_pdf", "f4"), ("rev_pdf", "f4"), ("pdf", "f4"),
                           ("pdf_rev", "f4")]), native.bsdf_eval_fields, 32),
        "sample": (np.dtype([("f", "f4", 3), ("wo", "f4", 3), ("pdf", "f4"), ("cos_wo", "f4"), ("type", "i4")]),
                   native.bsdf_sample_fields, 36),
        "illum": (np.dtype([("le", "f4", 3), ("dir", "f4", 3), ("dist", "f4"), ("direct_pdf", "f4"),
                            ("emission_pdf", "f4"), ("cos_light", "f4")]), native.light_fields, 40),
        "emission": (np.dtype([("le_cos", "f4", 3), ("pos", "f4", 3), ("dir", "f4", 3), ("emission_pdf", "f4"),
                               ("direct_pdf_a", "f4"), ("cos_light", "f4")]), native.light_fields, 48),
        "rad": (np.dtype([("le", "f4", 3), ("direct_pdf_a", "f4"), ("emission_pdf", "f4")]), native.light_fields, 20),
    }
    rng = np.random.default_rng(3)
    for name, (rec, fields, size) in recs.items():
        assert rec.itemsize == size, name
        words = size // 4
        rows = rng.integers(1, 1 << 30, (5, words)).astype(np.int32)
        want = rows.view(rec).reshape(5)
        for arr in (rows, pytest.importorskip("torch").from_numpy(rows.copy())):
            f = fields(arr)
            assert set(f) == set(rec.names), name
            for k in rec.names:
                assert np.array_equal(np.asarray(f[k]).view(np.uint32), want[k].view(np.uint32)), (name, k)
        with pytest.raises(ValueError):
            fields(rows[:, :words - 1] if words != 10 else rows[:, :7])


def _bad(torch):
    good = torch.zeros((6, 3), dtype=torch.float32)
    return {"numpy": (np.zeros((6, 3), np.float32), "torch tensor"), "cpu_tensor": (good, "is_cuda"),
            "float64": (good.double(), "float32"), "shape": (torch.zeros((6, 4), dtype=torch.float32), "shape"),
            "non_contiguous": (torch.zeros((6, 6), dtype=torch.float32)[:, ::2], "contiguous")}


@pytest.mark.parametrize("bad", ["numpy", "cpu_tensor", "float64", "shape", "non_contiguous"])
def test_wrappers_refuse_what_is_not_a_device_tensor(bad):
    """No context and no device: every wrapper raises before it touches either."""
    torch = pytest.importorskip("torch")
    x, word = _bad(torch)[bad]
    ctx = native.Context.__new__(native.Context)  # no wr_create: validation comes first
    hits = torch.zeros((6, 10), dtype=torch.int32)
    light = torch.zeros((6,), dtype=torch.int32)
    v = torch.zeros((6, 3), dtype=torch.float32)
    calls = [lambda: ctx.bsdf_eval_t(hits, x, v), lambda: ctx.bsdf_sample_t(hits, x, v),
             lambda: ctx.light_illuminate_t(light, x, v), lambda: ctx.light_emit_t(light, x, v),
             lambda: ctx.light_radiance_t(hits, x)]
    for call in calls:
        with pytest.raises(ValueError):  # (hits / light are CPU tensors too: some refusal comes first)
            call()
    # the tensor under test named in the message, through the helper the wrappers use
    with pytest.raises(ValueError, match=word):
        native._dev_tensor(x, "wi", (6, 3), "float32", None)
    with pytest.raises(ValueError):
        ctx.rng_uniform_t(6, 0, 1, 2, 3)
    with pytest.raises(ValueError):
        ctx.rng_uniform_t(6, 65, 1, 2, 3)
    with pytest.raises(ValueError):
        ctx.rng_uniform_t(6, 3, 1, 2, 3, path=torch.zeros((6,), dtype=torch.int64))


def test_script_path_tracer_over_the_oracle_equals_the_oracle_path_tracer():
    """tests/_script_pt.py over the oracle's primitives (Scene.trace, cr_kat_bsdf,
    cr_kat_light, cr_stream_*) against the oracle's PathIntegrator::raytracing:
    cbox(64, 48), max_depth 7, seed 77, sample 3, the 2,048 rays of
    test_path_radiance_per_ray_matches_oracle's recipe.  Every ray within the
    project's per-ray radiance gate 1e-5 |ref| + 1e-30."""
    sc = _oracle.Scene(_scenes.cbox(64, 48))
    o, d = _script_pt.cbox_rays(2048)
    ref, _ = sc.pt_radiance(np.concatenate([o, d], 1), 7, 77, sample=3)
    got = _script_pt.radiance(_script_pt.OracleBackend(sc, 77, 3), o, d, 7)
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert ref.sum() > 0
    err = np.abs(got.astype(np.float64) - ref)
    ok = np.all(err <= 1e-5 * np.abs(ref) + 1e-30, axis=1)
    lit = ref.any(axis=1)
    print("rays off:", int((~ok).sum()), "of", len(ok), "lit rays:", int(lit.sum()),
          "bit-equal rays:", int((got.view(np.uint32) == ref.view(np.uint32)).all(1).sum()),
          "worst relative:", float((err[lit] / np.abs(ref[lit]).max(1, keepdims=True)).max()))
    assert ok.all(), np.argwhere(~ok)[:5].ravel()
    assert 0 < lit.sum() < len(lit)
