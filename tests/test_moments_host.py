"""Second-moment films, host side (include/winmad_rt.h): the
error estimate wr_film_error on host films, its argument checks, and the
wr_tot flags that are usage errors.  No GPU: wr_film_error on host films is a
plain CPU loop.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _scenes
from winmad_rt import native

W, H, N = 8, 6, 5


def _synthetic():
    """Pass films of an 8x6 image, N passes, and their float32 sums as a
    moments render accumulates them (pass by pass, in float32).  Pixel (0, 0)
    is black, pixel (1, 1) is 0.75 in every pass (0.75, its square and their
    sums are exact floats: the cancellation case), pixel (2, 3) is hot in one
    pass."""
    rng = np.random.default_rng(12)
    passes = rng.random((N, H, W, 3), dtype=np.float32) * np.float32(2.0)
    passes[:, 0, 0, :] = 0.0
    passes[:, 1, 1, :] = 0.75
    passes[:, 2, 3, :] = 0.1
    passes[3, 2, 3, :] = 1000.0
    S = np.zeros((H, W, 3), np.float32)
    Q = np.zeros((H, W, 3), np.float32)
    for p in passes:
        S += p
        Q += p * p
    return S, Q


def _numpy_error(S, Q, n):
    s, q = S.astype(np.float64), Q.astype(np.float64)
    mu = s / n
    var = np.maximum(0.0, (q - s * s / n) / (n - 1)) / n
    se = np.sqrt(var)
    lit = mu > 0
    return {"se": se, "mu": mu, "sum_stderr": se.sum(), "sum_mean": mu.sum(),
            "rel_stderr": se.sum() / mu.sum(), "max_rel_stderr": (se[lit] / mu[lit]).max(),
            "values": int(lit.sum())}


def test_film_error_on_host_films_matches_numpy_float64():
    S, Q = _synthetic()
    ref = _numpy_error(S, Q, N)
    info, se = native.film_error(S, Q, N, stderr_map=True)
    for k in ("sum_stderr", "sum_mean", "rel_stderr", "max_rel_stderr"):
        got = getattr(info, k)
        print(k, got, ref[k])
        assert abs(got - ref[k]) <= 1e-9 * abs(ref[k]), (k, got, ref[k])
    assert info.values == ref["values"] == (W * H - 1) * 3
    assert se.dtype == np.float32 and se.shape == (H, W, 3)
    assert np.array_equal(se, ref["se"].astype(np.float32))  # float storage of the double result
    assert not se[0, 0].any()  # black: no error, and it does not enter the maximum
    assert np.all(se[1, 1] <= 1e-7 * ref["mu"][1, 1]), se[1, 1]  # equal in every pass: the cancellation case
    assert np.all(se[2, 3] > 100.0)  # the hot pixel: (1000 - 0.1) / 5 * sqrt(5 / 4) / sqrt(5) ~ 200
    assert info.max_rel_stderr == pytest.approx(float((ref["se"][2, 3] / ref["mu"][2, 3]).max()), rel=1e-9)
    # without the map: the same numbers
    info2 = native.film_error(S, Q, N)
    assert info2.as_dict() == info.as_dict()


def test_film_error_of_a_black_film_is_zero():
    z = np.zeros((H, W, 3), np.float32)
    info = native.film_error(z, z, 2)
    assert info.as_dict() == {"sum_stderr": 0.0, "sum_mean": 0.0, "rel_stderr": 0.0, "max_rel_stderr": 0.0,
                              "values": 0}


def test_film_error_argument_errors():
    L = native.lib()
    S, Q = _synthetic()
    info = native.WrErrorInfo()
    s, q = S.ctypes.data_as(C.c_void_p), Q.ctypes.data_as(C.c_void_p)
    assert L.wr_film_error(None, s, q, W, H, N, 0, None, C.byref(info)) == native.WR_OK
    for n in (1, 0, -3):  # a standard error needs two passes
        assert L.wr_film_error(None, s, q, W, H, n, 0, None, C.byref(info)) == native.WR_E_ARG
        assert "2 passes" in L.wr_last_error().decode()
    assert L.wr_film_error(None, None, q, W, H, N, 0, None, C.byref(info)) == native.WR_E_ARG
    assert L.wr_film_error(None, s, None, W, H, N, 0, None, C.byref(info)) == native.WR_E_ARG
    assert L.wr_film_error(None, s, q, W, H, N, 0, None, None) == native.WR_E_ARG
    assert L.wr_film_error(None, s, q, 0, H, N, 0, None, C.byref(info)) == native.WR_E_ARG
    # device films without a context
    assert L.wr_film_error(None, s, q, W, H, N, 1, None, C.byref(info)) == native.WR_E_ARG
    assert "context" in L.wr_last_error().decode()
    with pytest.raises(native.WrError):
        native.film_error(S, Q, 1)
    with pytest.raises(ValueError):
        native.film_error(S, Q[:-1], N)


def test_moments_entry_points_refuse_null_arguments():
    """The render entry points check their arguments before they touch a device."""
    L = native.lib()
    film = np.zeros((H, W, 3), np.float32)
    f = film.ctypes.data_as(C.c_void_p)
    p = native.WrBdptParams(W, H, 1, 0, 3, 10, 1, 1, 0, 0)
    assert L.wr_render_bdpt_moments(None, C.byref(p), f, f, 0, None) == native.WR_E_ARG
    v = native.WrVcmParams(W, H, 1, 0, 0, 10, 0.003, 0.75, 1, 0, 0)
    assert L.wr_render_vcm_moments(None, C.byref(v), f, f, 0, None) == native.WR_E_ARG
    t = native.WrPathParams(W, H, 4, 7, 0, 0, 1, 0, 0)
    assert L.wr_render_path_moments(None, C.byref(t), f, f, 0, None) == native.WR_E_ARG


def _tot(args, tmp_path):
    para = tmp_path / "p.para"
    para.write_text("7\n4\n8\n4\n32\n24\n5\n400\n")
    return subprocess.run([os.path.join(native.PKG_DIR, "wr_tot"), _scenes.cbox(32, 24, "bdpt"),
                           str(tmp_path / "o.pfm"), *args, "--params", str(para)], capture_output=True, text=True,
                          cwd=tmp_path, timeout=60)


@pytest.mark.parametrize("args,word", [
    (["-p", "--target-error", "0.1"], "strata"),     # PT's samples are strata of one grid, not passes
    (["-bpt", "--target-error", "-1"], ">= 0"),
    (["-vcm", "--target-error", "abc"], ">= 0"),
    (["-bpt", "--target-error", "0.1", "--error-every", "0"], "--error-every"),
    (["-bpt", "--target-error", "0.1", "--checkpoint", "ck.bin"], "--checkpoint"),  # the file carries no film_sq
    (["-bpt", "--error-out", "m.pfm"], "--error-out"),
])
def test_cli_target_error_usage_errors(args, word, tmp_path):
    r = _tot(args, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert "usage" in r.stderr and word in r.stderr, r.stderr
    assert not (tmp_path / "o.pfm").exists()


def test_api_version_is_still_8():
    """The entry points are additive: callers detect them by their symbols."""
    L = native.lib()
    assert L.wr_api_version() == 8
    for name in ("wr_render_bdpt_moments", "wr_render_vcm_moments", "wr_render_path_moments", "wr_film_error"):
        assert hasattr(L, name), name
    assert C.sizeof(native.WrErrorInfo) == 40


def test_wr_stats_keeps_its_v8_layout():
    """wr_stats.deferred_rays counts nothing any more (always 0) and keeps its
    place: 39 eight-byte fields, deferred_rays the 35th (include/winmad_rt.h as
    of API v8: five counters, seconds, 2 x 8 per-category entries,
    trace_wall_ms, then eleven counters in front of it and four behind)."""
    assert C.sizeof(native.WrStats) == 312
    assert native.WrStats.deferred_rays.offset == 272
    assert native.WrStats.deferred_rays.size == 8
    assert native.WrStats.bvh_width.offset == 280 and native.WrStats.redone.offset == 304
