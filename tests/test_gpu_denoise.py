"""First-hit feature films and the film denoiser on the GPU (include/winmad_rt.h
wr_render_features / wr_film_denoise).

Feature films: bit-equal to wr_trace_closest on the camera rays the oracle
builds (cr_kat_camera: the reference's Camera::generateRay, origin and
once-normalised direction) at the raster point each value stands for; the
albedo is recomputed here from the scene's material table.
Denoiser: the kernels against the library's CPU loop, bit for bit (the CPU loop
against the numpy restatement of the definition: tests/test_denoise_host.py).
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _denoise_ref as R
import _oracle
import _scenes
from _parity import assert_film_parity
from winmad_rt import native

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same_bits(got, want, what):
    bad = _bits(got) != _bits(want)
    print(what, "values that differ:", int(bad.sum()), "of", bad.size)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5])


def _dev(a):
    return torch.from_numpy(np.array(a, F, order="C")).to("cuda:0")  # a copy: the shared cases are read-only


# ------------------------------------------------------------------ features
def _albedo_table(scene, tmp):
    """min(1, diffuse + phong + specular) per material, from wr_scene_dump's `mat` lines
    (diffuse rgb, phong rgb, phongExp, specular rgb, refracIndex; hex floats)."""
    rows = []
    for line in scene.dump(os.path.join(tmp, "scene.dump")).splitlines():
        if line.startswith("mat "):
            v = np.array([float.fromhex(t) for t in line.split()[1:]], F)
            rows.append(np.minimum(F(1.0), (v[0:3] + v[3:6]) + v[7:10]))
    return np.array(rows, F).reshape(-1, 3)


def _camera_rays(path, W, H, layout):
    """The oracle's camera ray of every value index of a W x H film in `layout`."""
    sc = _oracle.Scene(path)
    idx = np.arange(W * H)
    a, b = idx // W, idx % W
    if layout == native.FILM_BDPT:
        xs, ys = a + 0.5, b + 0.5
    else:
        xs, ys = b.astype(float), a.astype(float)
    out = np.zeros(10, F)
    w = np.zeros(3, F)
    od = np.zeros((W * H, 6), F)
    for k in range(W * H):
        sc.L.cr_kat_camera(sc.h, float(xs[k]), float(ys[k]), _oracle.fptr(w), _oracle.fptr(out))
        od[k] = out[0:6]
    return native.rays_from_arrays(od[:, 0:3], od[:, 3:6])


FEATURE_CASES = {  # name: scene, W, H, layout, trace mode (None: the library's default)
    "cbox_pt": (lambda: _scenes.cbox(64, 48), 64, 48, native.FILM_PT, None),
    "spheres_bdpt": (lambda: _scenes.spheres(32, 32), 32, 32, native.FILM_BDPT, None),
    "cbox_bdpt_nonsquare": (lambda: _scenes.cbox(32, 24, "bdpt"), 32, 24, native.FILM_BDPT, None),
    "torus_reference": (lambda: _scenes.torus(64, 64), 64, 64, native.FILM_BDPT, native.TRACE_REFERENCE),
    "torus_bvh": (lambda: _scenes.torus(64, 64), 64, 64, native.FILM_PT, native.TRACE_BVH),
}


@pytest.mark.parametrize("name", list(FEATURE_CASES))
def test_feature_films_equal_trace_closest_on_the_oracle_camera_rays(name, tmp_path):
    maker, W, H, layout, mode = FEATURE_CASES[name]
    path = maker()
    scene = native.Scene(path)
    ctx = native.Context(scene, 0, trace=mode)
    hits = ctx.trace_closest(_camera_rays(path, W, H, layout))
    hit = hits["prim"] >= 0
    table = _albedo_table(scene, str(tmp_path))
    want = {"normal": np.where(hit[:, None], hits["n"], F(0)), "position": np.where(hit[:, None], hits["p"], F(0)),
            "depth": np.where(hit, hits["t"], F(0))}
    mat = hits["mat_id"]
    alb = np.where((mat < 0)[:, None], F(1.0), table[np.clip(mat, 0, len(table) - 1)])
    want["albedo"] = np.where(hit[:, None], alb, F(0)).astype(F)
    print(name, "hits", int(hit.sum()), "of", W * H, "emitter pixels", int((hit & (mat < 0)).sum()))
    assert hit.any()
    # host films
    got, st = ctx.render_features(W, H, layout)
    assert st.closest_rays == W * H
    for k in ("normal", "position", "albedo"):
        _same_bits(got[k].reshape(-1, 3), want[k], f"{name} host {k}")
    _same_bits(got["depth"].reshape(-1), want["depth"], f"{name} host depth")
    # device films
    dev = {k: torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda:0") for k in ("normal", "albedo", "position")}
    dev["depth"] = torch.full((H, W), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    none, st = ctx.render_features(W, H, layout, normal_ptr=dev["normal"].data_ptr(), albedo_ptr=dev["albedo"].data_ptr(),
                                   position_ptr=dev["position"].data_ptr(), depth_ptr=dev["depth"].data_ptr())
    assert none is None and st.closest_rays == W * H
    for k in dev:
        _same_bits(dev[k].cpu().numpy(), got[k], f"{name} device {k}")
    # some outputs not wanted
    nrm = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda:0")
    dep = torch.full((H, W), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    _, st = ctx.render_features(W, H, layout, normal_ptr=nrm.data_ptr(), depth_ptr=dep.data_ptr())
    assert st.closest_rays == W * H
    _same_bits(nrm.cpu().numpy(), got["normal"], f"{name} normal alone")
    _same_bits(dep.cpu().numpy(), got["depth"], f"{name} depth alone")
    ctx.close()


def test_feature_argument_errors():
    ctx = _ctx()
    L = native.lib()
    buf = torch.zeros((4, 4, 3), dtype=torch.float32, device="cuda:0")
    p = C.c_void_p(buf.data_ptr())
    assert L.wr_render_features(ctx.h, 4, 4, native.FILM_PT, None, None, None, None, 1, None) == native.WR_E_ARG
    assert L.wr_render_features(ctx.h, 0, 4, native.FILM_PT, p, None, None, None, 1, None) == native.WR_E_ARG
    assert L.wr_render_features(ctx.h, 4, -1, native.FILM_PT, p, None, None, None, 1, None) == native.WR_E_ARG
    assert L.wr_render_features(ctx.h, 1 << 15, 1 << 14, native.FILM_PT, p, None, None, None, 1, None) == native.WR_E_ARG
    assert L.wr_render_features(ctx.h, 4, 4, 2, p, None, None, None, 1, None) == native.WR_E_ARG
    assert L.wr_render_features(ctx.h, 4, 4, native.FILM_BDPT, p, None, None, None, 1, None) == native.WR_OK


# ------------------------------------------------------------------ denoiser
@functools.lru_cache(maxsize=None)
def _ctx():
    return native.Context(native.Scene(_scenes.cbox(32, 24, "bdpt")), 0)


def _device_denoise(ctx, S, Q, n, N=None, P=None, A=None, **prm):
    H, W = S.shape[:2]
    t = [_dev(a) if a is not None else None for a in (S, Q, N, P, A)]
    out = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ptr = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
    ctx.film_denoise(t[0].data_ptr(), t[1].data_ptr(), W, H, n, out.data_ptr(), normal_ptr=ptr(t[2]),
                     position_ptr=ptr(t[3]), albedo_ptr=ptr(t[4]), **prm)
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(W, H):
    c = R.synthetic(W, H)
    for a in c:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


# 37x23, 5x3, 1x1: smaller than a tile or than the filter's reach; 70x33: more
# than one 16x16 tile each way, a multiple of neither; 5 levels = steps 1, 2
# (tile + halo in LDS) and 4, 8, 16 (direct loads)
@pytest.mark.parametrize("W,H", [(37, 23), (5, 3), (1, 1), (70, 33)])
def test_device_denoise_equals_the_cpu_loop_bit_for_bit(W, H):
    S, Q, n, N, P, A = _case(W, H)
    got = _device_denoise(_ctx(), S, Q, n, N, P, A, levels=5)
    _same_bits(got, native.film_denoise(S, Q, n, N, P, A, levels=5), f"{W}x{H}")


@pytest.mark.parametrize("levels", [1, 2, 8])
def test_device_denoise_other_level_counts(levels):
    """1: prepare then straight into `out`; 2: the last level on the LDS path; 8: step 128."""
    S, Q, n, N, P, A = _case(70, 33)
    prm = dict(levels=levels, normal_power=3, sigma_l=2.0)
    _same_bits(_device_denoise(_ctx(), S, Q, n, N, P, A, **prm), native.film_denoise(S, Q, n, N, P, A, **prm),
               f"{levels} levels")


@pytest.mark.parametrize("drop", ["normal", "position", "albedo", "all"])
def test_device_denoise_with_guides_missing(drop):
    S, Q, n, N, P, A = _case(70, 33)
    g = {"normal": (None, P, A), "position": (N, None, A), "albedo": (N, P, None), "all": (None, None, None)}[drop]
    _same_bits(_device_denoise(_ctx(), S, Q, n, *g), native.film_denoise(S, Q, n, *g), f"without {drop}")


def test_device_denoise_of_a_render():
    """cbox 64x48, PT at 16 spp: moments render + feature films + denoise, all on
    device films; against the CPU loop on the downloaded films.  The filter is
    a normalised average, but its weights are not symmetric: a pixel with a
    large variance (a firefly) takes in its dimmer neighbours while they, sure
    of themselves, refuse it, so energy leaves with the fireflies.  On these
    films the numpy restatement's sum is 0.9209 of the input's (7.91 % off,
    not within 2 %): the bound is that figure plus a quarter, 9.89 %."""
    W, H, spp = 64, 48, 16
    ctx = native.Context(native.Scene(_scenes.cbox(W, H)), 0)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda:0")  # noqa: E731
    film, sq, nrm, pos, alb, out = (z(H, W, 3) for _ in range(6))
    torch.cuda.synchronize()
    ctx.render_path_moments(W, H, spp, film_ptr=film.data_ptr(), film_sq_ptr=sq.data_ptr())
    ctx.render_features(W, H, native.FILM_PT, normal_ptr=nrm.data_ptr(), albedo_ptr=alb.data_ptr(),
                        position_ptr=pos.data_ptr())
    ctx.film_denoise(film.data_ptr(), sq.data_ptr(), W, H, spp, out.data_ptr(), normal_ptr=nrm.data_ptr(),
                     position_ptr=pos.data_ptr(), albedo_ptr=alb.data_ptr())
    h = [t.cpu().numpy() for t in (film, sq, nrm, pos, alb, out)]
    ctx.close()
    host = native.film_denoise(h[0], h[1], spp, h[2], h[3], h[4])
    _same_bits(h[5], host, "cbox 64x48 PT 16 spp")
    assert np.isfinite(h[5]).all()
    changed = float(np.mean(_bits(h[5]) != _bits(h[0])))
    ref = R.np_denoise(h[0], h[1], spp, h[2], h[3], h[4])
    s_in, s_out, s_ref = (float(a.astype(np.float64).sum()) for a in (h[0], h[5], ref))
    print("values changed", changed, "sum in", s_in, "out", s_out, "ratio", s_out / s_in, "restatement", s_ref / s_in)
    assert changed > 0.5
    assert abs(s_out / s_in - 1.0) <= 0.0791 * 1.25


def test_a_denoise_leaves_the_plain_render_alone():
    """The denoiser's buffers are its own: a plain render after one holds the
    same work buffers and renders the same film as before."""
    W, H = 32, 24
    ctx = native.Context(native.Scene(_scenes.cbox(W, H, "bdpt")), 0)
    before, st0 = ctx.render_bdpt(W, H, iterations=2, seed=9)
    S, Q, n, N, P, A = _case(70, 33)
    _device_denoise(ctx, S, Q, n, N, P, A)
    ctx.render_features(W, H, native.FILM_BDPT)
    after, st1 = ctx.render_bdpt(W, H, iterations=2, seed=9)
    ctx.close()
    assert (st1.work_bytes, st1.work_paths) == (st0.work_bytes, st0.work_paths)
    assert st0.work_bytes > 0
    assert_film_parity(after, before, case="bdpt_cbox32x24_after_denoise", kind="film_vs_before")


def test_multi_device_context_runs_on_its_first_device():
    W, H = 32, 24
    scene = native.Scene(_scenes.cbox(W, H, "bdpt"))
    one, two = native.Context(scene, 0), native.Context(scene, devices=[0, 0])
    f1, _ = one.render_features(W, H, native.FILM_BDPT)
    f2, st = two.render_features(W, H, native.FILM_BDPT)
    assert st.closest_rays == W * H
    for k in f1:
        _same_bits(f2[k], f1[k], f"two devices, {k}")
    S, Q, n, N, P, A = _case(70, 33)
    _same_bits(_device_denoise(two, S, Q, n, N, P, A), _device_denoise(one, S, Q, n, N, P, A), "two devices, denoise")
    one.close()
    two.close()


def _pfm(path):
    data = open(path, "rb").read()
    head = data.split(b"\n", 3)
    w, h = map(int, head[1].split())
    return np.frombuffer(head[3], np.float32).reshape(h, w, 3)[::-1]  # PFM rows run bottom-up


@pytest.mark.parametrize("flag,more", [("-p", []), ("-bpt", ["--iterations", "4"])])
def test_cli_writes_the_denoised_image(flag, more, tmp_path):
    W, H = 32, 24
    para = tmp_path / "p.para"
    para.write_text(f"7\n4\n8\n4\n{W}\n{H}\n5\n400\n")
    r = subprocess.run([os.path.join(native.PKG_DIR, "wr_tot"), _scenes.cbox(W, H, "bdpt"), str(tmp_path / "o.pfm"),
                        flag, "--params", str(para), "--denoise", str(tmp_path / "d.pfm"), *more],
                       capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    o, d = _pfm(tmp_path / "o.pfm"), _pfm(tmp_path / "d.pfm")
    assert o.shape == d.shape == (H, W, 3)
    assert np.isfinite(o).all() and np.isfinite(d).all()
    assert o.any() and d.any() and (_bits(o) != _bits(d)).any()
