"""The film denoiser on host films (include/winmad_rt.h wr_film_denoise,
DESIGN.md 11): the library's CPU loop against the numpy float32 restatement of
the definition (tests/_denoise_ref.py), bit for bit; the properties the
definition promises; the argument checks; the wr_tot flags that are usage
errors; and the CPU loop under the address / undefined-behaviour sanitizers as
a stand-alone program.  No GPU: wr_film_denoise on host films needs no device.
"""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import _denoise_ref as R
import _scenes
from winmad_rt import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "winmad-s-raytracer-v1.0_amd", "csrc")
F = np.float32
SIZES = [(37, 23), (5, 3), (1, 1)]  # all smaller than the filter's reach (2 * 31 pixels at 5 levels): every window is clipped


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _assert_same_bits(got, want, what):
    bad = _bits(got) != _bits(want)
    print(what, "values that differ:", int(bad.sum()), "of", bad.size)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5])


@pytest.mark.parametrize("W,H", SIZES)
def test_cpu_loop_equals_the_numpy_restatement_bit_for_bit(W, H):
    S, Q, n, N, P, A = R.synthetic(W, H)
    out = native.film_denoise(S, Q, n, N, P, A, levels=5)
    assert out.dtype == F and out.shape == (H, W, 3)
    _assert_same_bits(out, R.np_denoise(S, Q, n, N, P, A, levels=5), f"{W}x{H} all guides")
    if W > 3:  # the hot pixel and the equal-in-every-pass pixel did not poison the film
        assert np.isfinite(out).all()


@pytest.mark.parametrize("which", ["none", "normal", "position", "albedo"])
def test_cpu_loop_equals_numpy_with_guides_missing(which):
    """37x23 with every guide NULL, and with each single guide alone (a lone
    position film has no normal to measure the plane distance with: weight 1)."""
    S, Q, n, N, P, A = R.synthetic(37, 23)
    g = {"none": (None, None, None), "normal": (N, None, None), "position": (None, P, None),
         "albedo": (None, None, A)}[which]
    out = native.film_denoise(S, Q, n, *g)
    _assert_same_bits(out, R.np_denoise(S, Q, n, *g), which)
    if which in ("none", "position"):
        _assert_same_bits(out, native.film_denoise(S, Q, n), "a lone position film changes nothing")


def test_other_parameters_equal_numpy_too():
    S, Q, n, N, P, A = R.synthetic(37, 23)
    prm = dict(levels=3, normal_power=0, sigma_l=1.5, sigma_p=0.2, sigma_a=0.5)
    _assert_same_bits(native.film_denoise(S, Q, n, N, P, A, **prm), R.np_denoise(S, Q, n, N, P, A, **prm), "params")
    prm = dict(levels=8, normal_power=10)
    _assert_same_bits(native.film_denoise(S, Q, n, N, P, A, **prm), R.np_denoise(S, Q, n, N, P, A, **prm), "8 levels")


def test_edges_isolate_exactly():
    """w_n is exactly 0 between a surface and a no-surface pixel and between
    orthogonal normals; 0 * c adds +0 to a sum, and the variance prefilter skips
    a tap whose w_n is 0: what lies across an edge cannot move a single bit of
    region A, whether region B or the no-surface band changes."""
    W, H, n = 37, 23, 6
    A_, band, B_ = R.regions(W)
    N, P, Al = R.synthetic_guides(W, H)
    passes = R.synthetic_passes(W, H, n)
    base = native.film_denoise(*R.fold(passes), n, N, P, Al)
    rng = np.random.default_rng(99)
    for name, cols in (("region B", B_), ("the no-surface band", band)):
        p2 = passes.copy()
        p2[:, :, cols, :] = rng.random(p2[:, :, cols, :].shape, dtype=F) * F(9.0)
        out = native.film_denoise(*R.fold(p2), n, N, P, Al)
        _assert_same_bits(out[:, A_], base[:, A_], f"region A after {name} changed")
        assert (_bits(out[:, cols]) != _bits(base[:, cols])).any()
    # the same with the normal film alone: isolation is w_n's doing
    base = native.film_denoise(*R.fold(passes), n, N)
    p2 = passes.copy()
    p2[:, :, A_.stop:, :] = 3.0
    _assert_same_bits(native.film_denoise(*R.fold(p2), n, N)[:, A_], base[:, A_], "region A, normals only")
    # and w_n itself, from the restatement: exactly 0 across both edges
    c = np.zeros((H, W), F)
    for off in range(1, W):
        wn, _ = R._normal_weight(N, (N != 0).any(axis=2), R._shift(N, 0, off)[0], 7)
        m = R._shift(c, 0, off)[1]
        m[:, A_.stop:] = False  # pairs that start in region A ...
        m[:, :max(0, A_.stop - off)] = False  # ... and end beyond it
        assert not wn[m].any()


def test_equal_passes_come_back():
    """v = 0: a neighbour of another luminance weighs nothing, so every value is
    a weighted mean of equal floats -- a few roundings from the input."""
    W, H, n = 37, 23, 4
    img = np.zeros((H, W, 3), F)
    for by in range(0, H, 6):  # flat patches, values k / 64: sums and squares are exact floats
        for bx in range(0, W, 5):
            img[by:by + 6, bx:bx + 5] = (((by * 7 + bx * 3) % 64 + 1) / 64.0, ((by + bx * 5) % 32 + 1) / 64.0,
                                         ((by * 3 + bx) % 16 + 1) / 64.0)
    S, Q = R.fold(np.repeat(img[None], n, axis=0))
    out = native.film_denoise(S, Q, n)
    rel = np.abs(out - S) / S
    print("largest relative change", rel.max())
    assert rel.max() <= 1e-6


def test_black_film_and_negative_variance_stay_finite():
    z = np.zeros((23, 37, 3), F)
    N, P, Al = R.synthetic_guides(37, 23)
    assert not native.film_denoise(z, z, 2).any()
    assert not native.film_denoise(z, z, 2, N, P, Al).any()
    # Q < S^2 / n (impossible for real passes, possible after a bad reduce): the variance clamps to 0
    S, Q, n, _, _, _ = R.synthetic(37, 23)
    Q2 = (Q * F(0.01)).astype(F)
    assert ((Q2.astype(np.float64) - S.astype(np.float64) ** 2 / n) < 0).any()
    out = native.film_denoise(S, Q2, n, N, P, Al)
    assert np.isfinite(out).all()
    _assert_same_bits(out, R.np_denoise(S, Q2, n, N, P, Al), "negative variance")


def test_noise_reduction_on_a_flat_region():
    """Constant truth 0.5 plus seeded uniform noise (+-0.25) over 8 passes,
    64 x 64, no guides, default parameters.  RMSE(out / n, truth) /
    RMSE(film / n, truth) measured with the numpy restatement: 0.0365 (one
    level of the bare B3 kernel would give 0.27).  The library must reach that
    value times 1.05, and improve on the input."""
    W = H = 64
    n = 8
    rng = np.random.default_rng(2024)
    truth = F(0.5)
    passes = (truth + (rng.random((n, H, W, 3), dtype=F) - F(0.5)) * F(0.5)).astype(F)
    S, Q = R.fold(passes)

    def ratio(out):
        return float(np.sqrt(np.mean((out.astype(np.float64) / n - 0.5) ** 2)) /
                     np.sqrt(np.mean((S.astype(np.float64) / n - 0.5) ** 2)))

    ref, got = ratio(R.np_denoise(S, Q, n)), ratio(native.film_denoise(S, Q, n))
    print("rmse ratio: numpy restatement", ref, "library", got)
    assert abs(ref - 0.0365) < 0.0005  # the figure in this docstring and in DESIGN.md 11
    assert got <= ref * 1.05
    assert got < 1.0


def test_argument_errors():
    L = native.lib()
    S, Q, n, N, P, A = R.synthetic(5, 3)
    W, H = 5, 3
    out = np.zeros_like(S)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    call = lambda *a: L.wr_film_denoise(*a)  # noqa: E731
    assert call(None, p(S), p(Q), W, H, n, p(N), p(P), p(A), None, 0, p(out)) == native.WR_OK
    assert call(None, p(S), p(Q), W, H, n, None, None, None, None, 0, p(out)) == native.WR_OK
    for bad_n in (1, 0, -2):
        assert call(None, p(S), p(Q), W, H, bad_n, None, None, None, None, 0, p(out)) == native.WR_E_ARG
        assert "2 passes" in L.wr_last_error().decode()
    assert call(None, None, p(Q), W, H, n, None, None, None, None, 0, p(out)) == native.WR_E_ARG
    assert call(None, p(S), None, W, H, n, None, None, None, None, 0, p(out)) == native.WR_E_ARG
    assert call(None, p(S), p(Q), W, H, n, None, None, None, None, 0, None) == native.WR_E_ARG
    for k in range(5):  # out equal to an input
        ins = [p(S), p(Q), p(N), p(P), p(A)]
        assert call(None, ins[0], ins[1], W, H, n, ins[2], ins[3], ins[4], None, 0, ins[k]) == native.WR_E_ARG
        assert "inputs" in L.wr_last_error().decode()
    assert call(None, p(S), p(Q), 0, H, n, None, None, None, None, 0, p(out)) == native.WR_E_ARG
    assert call(None, p(S), p(Q), W, -1, n, None, None, None, None, 0, p(out)) == native.WR_E_ARG
    for bad in (dict(levels=0), dict(levels=9), dict(normal_power=-1), dict(normal_power=11), dict(sigma_l=0.0),
                dict(sigma_p=-1.0), dict(sigma_a=float("nan"))):
        prm = native.WrDenoiseParams(**bad)
        assert call(None, p(S), p(Q), W, H, n, None, None, None, C.byref(prm), 0, p(out)) == native.WR_E_ARG, bad
        with pytest.raises(native.WrError):
            native.film_denoise(S, Q, n, **bad)
    # device films without a context
    assert call(None, p(S), p(Q), W, H, n, None, None, None, None, 1, p(out)) == native.WR_E_ARG
    assert "context" in L.wr_last_error().decode()
    with pytest.raises(ValueError):
        native.film_denoise(S, Q[:-1], n)
    with pytest.raises(ValueError):
        native.film_denoise(S, Q, n, normal=N[:, :-1])


def test_entry_points_are_additive():
    """Callers find the new calls by symbol: the version, and every struct that existed, stay."""
    L = native.lib()
    assert L.wr_api_version() == 8
    for name in ("wr_render_features", "wr_film_denoise"):
        assert hasattr(L, name), name
        assert name in native.EXPORTS
    assert C.sizeof(native.WrDenoiseParams) == 20
    d = native.WrDenoiseParams()
    assert (d.levels, d.normal_power) == (5, 7)
    assert (d.sigma_l, d.sigma_p, d.sigma_a) == (4.0, F(0.05), F(0.1))
    assert C.sizeof(native.WrStats) == 312 and C.sizeof(native.WrErrorInfo) == 40
    # the Python and mirror entry points that go through them
    assert callable(native.film_denoise) and callable(native.Context.film_denoise)
    assert callable(native.Context.render_features)
    hdr = open(os.path.join(CSRC, "integrators.h")).read()
    assert hdr.count("outputDenoisedImage") >= 3 and "bool denoise" in hdr
    # a null context is refused before any device is touched
    buf = np.zeros((3, 5, 3), F)
    assert L.wr_render_features(None, 5, 3, native.FILM_PT, buf.ctypes.data_as(C.c_void_p), None, None, None, 0,
                                None) == native.WR_E_ARG


def _tot(args, tmp_path, spp=4):
    para = tmp_path / "p.para"
    para.write_text(f"7\n{spp}\n8\n4\n32\n24\n5\n400\n")
    return subprocess.run([os.path.join(native.PKG_DIR, "wr_tot"), _scenes.cbox(32, 24, "bdpt"),
                           str(tmp_path / "o.pfm"), *args, "--params", str(para)], capture_output=True, text=True,
                          cwd=tmp_path, timeout=60)


@pytest.mark.parametrize("args,spp,word", [
    (["-bpt", "--denoise", "d.pfm"], 4, "--iterations"),                     # one iteration: no variance
    (["-vcm", "--denoise", "d.pfm", "--iterations", "1"], 4, "--iterations"),
    (["-p", "--denoise", "d.pfm"], 1, "samples"),                            # one sample per pixel
    (["-bpt", "--denoise", "d.pfm", "--iterations", "4", "--checkpoint", "ck.bin"], 4, "--checkpoint"),
    (["-p", "--denoise", "d.pfm", "--checkpoint", "ck.bin"], 4, "--checkpoint"),
])
def test_cli_denoise_usage_errors(args, spp, word, tmp_path):
    r = _tot(args, tmp_path, spp)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert "usage" in r.stderr and word in r.stderr, r.stderr
    assert not (tmp_path / "o.pfm").exists() and not (tmp_path / "d.pfm").exists()


def _write_case(path, S, Q, n, N, P, A, want, prm):
    with open(path, "wb") as f:
        H, W = S.shape[:2]
        f.write(struct.pack("8i", W, H, n, N is not None, P is not None, A is not None, prm["levels"],
                            prm["normal_power"]))
        f.write(struct.pack("3f", prm["sigma_l"], prm["sigma_p"], prm["sigma_a"]))
        for a in (S, Q, N, P, A, want):
            if a is not None:
                f.write(np.ascontiguousarray(a, F).tobytes())


def test_cpu_loop_under_sanitizers():
    """tests/native/denoise_check.cpp + csrc/wr_denoise.cpp, built with
    -fsanitize=address,undefined, run as a program of its own on the clipped
    sizes: no report, and the same bits as the library's unsanitized build."""
    d = tempfile.mkdtemp(prefix="wr_dnchk_")
    exe = os.path.join(d, "denoise_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "native", "denoise_check.cpp"), os.path.join(CSRC, "wr_denoise.cpp"),
                    "-o", exe], check=True)
    files = []
    for W, H in SIZES:
        S, Q, n, N, P, A = R.synthetic(W, H)
        for tag, g in (("all", (N, P, A)), ("none", (None, None, None))):
            prm = dict(R.DEFAULTS)
            want = native.film_denoise(S, Q, n, *g, **prm)
            files.append(os.path.join(d, f"case_{W}x{H}_{tag}.bin"))
            _write_case(files[-1], S, Q, n, *g, want, prm)
    r = subprocess.run([exe, *files], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith(f"OK {len(files)} cases"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
