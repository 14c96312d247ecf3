"""Device-resident ray batches on the GPU (include/winmad_rt.h wr_camera_rays /
wr_trace_closest_dev / wr_occluded_dev / wr_path_radiance_dev).

The host calls are pinned to the reference's own outputs (tests/test_gpu.py,
tests/test_gpu_bvh.py), and the _dev calls run the same kernels on the caller's
arrays, so the gate here is equality with the host calls: whole 40-byte wr_hit
records compared as uint32, misses included.  Radiance: the oracle at the
tolerance of test_path_radiance_per_ray_matches_oracle, and the host call.
"""
import ctypes as C
import os

import numpy as np
import pytest

import _oracle
import _scenes
from winmad_rt import native

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
SCENES = {"torus64": lambda: _scenes.torus(64, 64), "cbox64x48": lambda: _scenes.cbox(64, 48),
          "spheres64": lambda: _scenes.spheres(64, 64)}
MODES = {"default": None, "reference": native.TRACE_REFERENCE}

_ctx = {}


def ctx_of(name, mode="default"):
    if (name, mode) not in _ctx:
        s = native.Scene(SCENES[name]())
        _ctx[(name, mode)] = (s, native.Context(s, 0, trace=MODES[mode]))
    return _ctx[(name, mode)][1]


def normalize_f32(d):
    d = d.astype(F)
    l = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return (d / l[:, None]).astype(F)


def corpus(name, repeat=1):
    """The golden ray corpus: (closest-hit rays, occlusion rays, targets)."""
    rays = np.tile(np.fromfile(os.path.join(GOLD, f"rays_{name}.f32"), F).reshape(-1, 9), (repeat, 1))
    return (native.rays_from_arrays(rays[:, 0:3], normalize_f32(rays[:, 3:6])),  # the Ray ctor normalises
            native.rays_from_arrays(rays[:, 0:3], rays[:, 3:6]), np.ascontiguousarray(rays[:, 6:9]))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def records(host_hits):
    """wr_trace_closest's structured array as (n, 10) uint32 words."""
    return np.ascontiguousarray(host_hits).view(np.uint32).reshape(-1, 10)


def words(t):
    return t.cpu().numpy().view(np.uint32)


def same_records(got, want, what):
    bad = np.argwhere(words(got) != want)
    print(what, "words that differ:", len(bad), "of", want.size)
    assert len(bad) == 0, (what, bad[:5])


# ------------------------------------------------------------------ 1. corpus
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(SCENES))
def test_corpus_equals_the_host_calls(name, mode):
    c = ctx_of(name, mode)
    r8, ro, tg = corpus(name)
    want = c.trace_closest(r8)
    assert (want["prim"] >= 0).any() and (want["prim"] < 0).any()  # hits and misses are both compared
    hits = c.trace_closest_t(dev(r8))
    assert hits.dtype == torch.int32 and tuple(hits.shape) == (len(r8), 10) and hits.is_cuda
    same_records(hits, records(want), f"{name} {mode} closest")
    f = native.hit_fields(hits)
    assert np.array_equal(f["prim"].cpu().numpy(), want["prim"])
    assert np.array_equal(f["t"].cpu().numpy().view(np.uint32), want["t"].view(np.uint32))
    assert np.array_equal(f["n"].cpu().numpy().view(np.uint32), want["n"].view(np.uint32))
    occ = c.occluded_t(dev(ro), dev(tg))
    assert occ.dtype == torch.uint8 and tuple(occ.shape) == (len(ro),)
    want_occ = c.occluded(ro, tg)
    assert want_occ.any() and not want_occ.all()
    assert np.array_equal(occ.cpu().numpy(), want_occ)


# ------------------------------------------------------------------ 2. sizes
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4097]


@pytest.fixture(scope="module")
def sized():
    """The torus corpus (2048 rays) three times over, so that a prefix of 4097
    rays exists; the host's answers for all of it, computed once."""
    c = ctx_of("torus64")
    r8, ro, tg = corpus("torus64", repeat=3)
    return c, r8, ro, tg, records(c.trace_closest(r8)), c.occluded(ro, tg)


@pytest.mark.parametrize("n", SIZES)
def test_prefix_sizes_write_n_records_and_nothing_after(n, sized):
    c, r8, ro, tg, want, want_occ = sized
    big = torch.full((n + 3, 10), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    got = c.trace_closest_t(dev(r8[:n]), out=big[:n])
    assert tuple(got.shape) == (n, 10)
    assert got.untyped_storage().data_ptr() == big.untyped_storage().data_ptr()  # `out` itself, no copy
    same_records(big[:n], want[:n], f"n={n} closest")
    assert bool((big[n:] == 0x5A5A5A5A).all())
    obig = torch.full((n + 5,), 0xA5, dtype=torch.uint8, device=DEV)
    c.occluded_t(dev(ro[:n]), dev(tg[:n]), out=obig[:n])
    assert np.array_equal(obig[:n].cpu().numpy(), want_occ[:n])
    assert bool((obig[n:] == 0xA5).all())


# ------------------------------------------------------------------ 3. alignment
def test_records_need_only_four_byte_alignment(sized):
    c, r8, ro, tg, want, want_occ = sized
    n = 1000
    rays = torch.zeros((n + 1, 8), dtype=torch.float32, device=DEV)
    rays[1:] = dev(r8[:n])
    hits = torch.full((n + 1, 10), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    assert hits[1:].data_ptr() % 16 == 8  # one 40-byte record in: 8-byte aligned only
    c.trace_closest_t(rays[1:], out=hits[1:])
    same_records(hits[1:], want[:n], "closest, offset views")
    assert bool((hits[0] == 0x5A5A5A5A).all())
    orays = torch.zeros((n + 1, 8), dtype=torch.float32, device=DEV)
    orays[1:] = dev(ro[:n])
    targets = torch.zeros((n + 1, 3), dtype=torch.float32, device=DEV)
    targets[1:] = dev(tg[:n])
    assert targets[1:].data_ptr() % 8 == 4  # 12 bytes in: 4-byte aligned only
    occ = torch.full((n + 1,), 0xA5, dtype=torch.uint8, device=DEV)
    assert occ[1:].data_ptr() % 2 == 1
    c.occluded_t(orays[1:], targets[1:], out=occ[1:])
    assert np.array_equal(occ[1:].cpu().numpy(), want_occ[:n])
    assert int(occ[0]) == 0xA5


# ------------------------------------------------------------------ 4. ordering
def test_call_is_ordered_after_pending_default_stream_work():
    """The rays come out of a chain of torch ops on the default stream (a few
    matrix products, then elementwise work on 2^20 rays) that is still running
    when the call is issued: no synchronize in between.  Without the wait for
    the legacy null stream the call would read what `rays` held before: the
    unperturbed camera rays, valid rays with other answers."""
    c = ctx_of("torus64")
    W = 1024
    base = c.camera_rays_t(W, W)
    eye = torch.eye(4096, dtype=torch.float32, device=DEV)
    rays = base.clone()
    axis = torch.tensor([1.0, -0.5, 0.25], device=DEV)  # (made here: a host-to-device copy would wait for the stream)

    def produce():
        x = eye
        for _ in range(8):
            x = x @ eye  # stays the identity: x[0, 0] is exactly 1
        jitter = torch.sin(torch.arange(W * W, dtype=torch.float32, device=DEV)) * 0.01
        d = base[:, 3:6] + jitter[:, None] * (x[0, 0] - 1.0 + axis)
        d = d / torch.sqrt((d * d).sum(1, keepdim=True))
        rays.copy_(torch.cat([base[:, 0:3] + (x[1, 1] - 1.0), d, base[:, 6:8]], 1))

    produce()
    torch.cuda.synchronize()
    host_rays = rays.cpu().numpy()
    assert np.abs(host_rays[:, 3:6] - base.cpu().numpy()[:, 3:6]).max() > 1e-3
    want = dev(records(c.trace_closest(host_rays)).view(np.int32))
    stale = c.trace_closest_t(base)
    assert not bool(torch.equal(stale, want))  # reading `rays` too early would show
    rays.copy_(base)
    torch.cuda.synchronize()
    produce()
    hits = c.trace_closest_t(rays)  # no synchronize before
    assert bool(torch.equal(hits, want))  # ... and a torch op reads the result directly after
    assert int((native.hit_fields(hits)["prim"] >= 0).sum()) > 0


# ------------------------------------------------------------------ 5. camera rays
def oracle_camera_rays(path, W, H, layout):
    """The oracle's camera ray (cr_kat_camera: the reference's Camera::generateRay)
    at the raster point every value index of a W x H film in `layout` stands for."""
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


@pytest.mark.parametrize("layout", [native.FILM_PT, native.FILM_BDPT])
@pytest.mark.parametrize("W,H", [(32, 24), (30, 20)])  # 30 x 20: feat_index does not tile
def test_camera_rays(W, H, layout):
    path = _scenes.cbox(W, H, "bdpt" if layout == native.FILM_BDPT else "pt")
    scene = native.Scene(path)
    c = native.Context(scene, 0)
    host = c.camera_rays(W, H, layout)
    rays = c.camera_rays_t(W, H, layout)
    assert host.shape == (W * H, 8) and host.dtype == F
    assert rays.dtype == torch.float32 and tuple(rays.shape) == (W * H, 8) and rays.is_cuda
    assert np.array_equal(rays.cpu().numpy().view(np.uint32), host.view(np.uint32))
    # tracing them reproduces render_features' films: zeros where the ray misses
    f = native.hit_fields(c.trace_closest_t(rays))
    hit = (f["prim"] >= 0).cpu().numpy()
    assert hit.any()
    films, _ = c.render_features(W, H, layout)
    for film, got, shape in (("normal", f["n"], (-1, 3)), ("position", f["p"], (-1, 3)), ("depth", f["t"], (-1,))):
        got = got.cpu().numpy()
        got = np.where(hit[:, None] if got.ndim == 2 else hit, got, F(0))
        bad = np.argwhere(got.view(np.uint32) != films[film].reshape(shape).view(np.uint32))
        assert len(bad) == 0, (film, bad[:5])
    # ... and they are the oracle's camera rays
    want = oracle_camera_rays(path, W, H, layout)
    bad = np.argwhere(host.view(np.uint32) != want.view(np.uint32))
    print("camera rays off the oracle:", len(bad))
    assert len(bad) == 0, bad[:5]
    c.close()


# ------------------------------------------------------------------ 6. radiance
def test_radiance_accumulates_and_builds_the_moments_pair():
    """The ray recipe of test_path_radiance_per_ray_matches_oracle (camera rays
    through random points of the back wall plus random rays inside the box),
    n = 2000.  rgb_sq against the host's squares: 2.1e-5 relative = twice the
    1e-5 of a value for its square, plus three float roundings (two squares,
    one sum)."""
    path = _scenes.cbox(64, 48)
    c = ctx_of("cbox64x48")
    rng = np.random.default_rng(9)
    n = 2000
    cam = np.array([-0.0439815, -4.12529, 0.222539], F)
    tgt = np.stack([rng.uniform(-1.2, 1.2, n), np.full(n, 1.3), rng.uniform(-1.2, 1.2, n)], 1).astype(F)
    d = normalize_f32(tgt - cam)
    o = np.repeat(cam[None], n, 0)
    o[n // 2:] = rng.uniform(-1.0, 1.0, (n - n // 2, 3)).astype(F)
    d[n // 2:] = normalize_f32(rng.normal(size=(n - n // 2, 3)))
    rays8 = native.rays_from_arrays(o, d)
    rays = dev(rays8)
    ref, rst = _oracle.Scene(path).pt_radiance(np.concatenate([o, d], 1), 7, 77, sample=3)
    h3, hs3 = c.path_radiance(rays8, max_depth=7, seed=77, sample=3)
    h4, hs4 = c.path_radiance(rays8, max_depth=7, seed=77, sample=4)
    assert ref.sum() > 0

    def close(got, want, rel, floor):
        got, want = got.astype(np.float64), want.astype(np.float64)
        ok = np.abs(got - want) <= rel * np.abs(want) + floor
        print("values off:", int((~ok).sum()), "worst relative",
              float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))))
        return ok.all()

    # a new zeroed rgb: the host call's answer bit for bit
    plain, st = c.path_radiance_t(rays, max_depth=7, seed=77, sample=3)
    assert tuple(plain.shape) == (n, 3) and plain.dtype == torch.float32
    assert np.array_equal(plain.cpu().numpy().view(np.uint32), h3.view(np.uint32))
    assert (st.closest_rays, st.shadow_rays) == (hs3.closest_rays, hs3.shadow_rays)
    # two samples into one pair of films
    rgb = torch.zeros((n, 3), dtype=torch.float32, device=DEV)
    rgb_sq = torch.zeros((n, 3), dtype=torch.float32, device=DEV)
    out, st = c.path_radiance_t(rays, max_depth=7, seed=77, sample=3, rgb=rgb, rgb_sq=rgb_sq)
    assert out is rgb
    got = rgb.cpu().numpy()
    assert np.all(np.isfinite(got)) and got.min() >= 0
    assert close(got, ref, 1e-5, 1e-30)
    assert st.closest_rays == rst.closest_rays and st.shadow_rays == rst.shadow_rays
    _, st4 = c.path_radiance_t(rays, max_depth=7, seed=77, sample=4, rgb=rgb, rgb_sq=rgb_sq)
    assert (st4.closest_rays, st4.shadow_rays) == (hs4.closest_rays, hs4.shadow_rays)
    assert close(rgb.cpu().numpy(), h3.astype(np.float64) + h4, 1e-5, 1e-30)
    sq = h3.astype(np.float64) ** 2 + h4.astype(np.float64) ** 2
    assert close(rgb_sq.cpu().numpy(), sq, 2.1e-5, 0.0)
    info = c.film_error(rgb.data_ptr(), rgb_sq.data_ptr(), n, 1, 2)
    vals = [info.sum_stderr, info.sum_mean, info.rel_stderr, info.max_rel_stderr]
    print("film_error of the n x 1 film:", info.as_dict())
    assert np.all(np.isfinite(vals)) and info.sum_mean > 0 and info.values > 0


# ------------------------------------------------------------------ 7. arguments
def test_bad_arguments_are_refused_and_outputs_left_alone():
    c = ctx_of("torus64")
    L = native.lib()
    r8 = corpus("torus64")[0][:4]
    rays = dev(r8)
    tg = torch.zeros((4, 3), dtype=torch.float32, device=DEV)
    hits = torch.full((4, 10), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    occ = torch.full((4,), 0xA5, dtype=torch.uint8, device=DEV)
    rgb = torch.full((4, 3), -7.0, dtype=torch.float32, device=DEV)
    both = torch.full((64,), -7.0, dtype=torch.float32, device=DEV)  # rays and hits in one buffer
    pinned = torch.from_numpy(r8.copy()).pin_memory()  # device-readable host memory: cannot fault
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())
    big = (1 << 28) + 1
    cases = {
        "closest null rays": lambda: L.wr_trace_closest_dev(c.h, None, 4, p(hits)),
        "closest null hits": lambda: L.wr_trace_closest_dev(c.h, p(rays), 4, None),
        "closest n = -1": lambda: L.wr_trace_closest_dev(c.h, p(rays), -1, p(hits)),
        "closest n = 2^28 + 1": lambda: L.wr_trace_closest_dev(c.h, p(rays), big, p(hits)),
        "closest hits alias rays": lambda: L.wr_trace_closest_dev(c.h, p(both), 4, C.c_void_p(both.data_ptr() + 16)),
        "closest pinned rays": lambda: L.wr_trace_closest_dev(c.h, p(pinned), 4, p(hits)),
        "occluded null targets": lambda: L.wr_occluded_dev(c.h, p(rays), None, 4, p(occ)),
        "occluded null output": lambda: L.wr_occluded_dev(c.h, p(rays), p(tg), 4, None),
        "occluded n = -1": lambda: L.wr_occluded_dev(c.h, p(rays), p(tg), -1, p(occ)),
        "occluded n = 2^28 + 1": lambda: L.wr_occluded_dev(c.h, p(rays), p(tg), big, p(occ)),
        "occluded pinned rays": lambda: L.wr_occluded_dev(c.h, p(pinned), p(tg), 4, p(occ)),
        "radiance null rgb": lambda: L.wr_path_radiance_dev(c.h, p(rays), 4, 7, 1, 0, None, None, None),
        "radiance n = -1": lambda: L.wr_path_radiance_dev(c.h, p(rays), -1, 7, 1, 0, p(rgb), None, None),
        "radiance n = 2^26 + 1": lambda: L.wr_path_radiance_dev(c.h, p(rays), (1 << 26) + 1, 7, 1, 0, p(rgb), None, None),
        "radiance max_depth": lambda: L.wr_path_radiance_dev(c.h, p(rays), 4, 62, 1, 0, p(rgb), None, None),
        "radiance rgb_sq is rgb": lambda: L.wr_path_radiance_dev(c.h, p(rays), 4, 7, 1, 0, p(rgb), p(rgb), None),
        "radiance pinned rays": lambda: L.wr_path_radiance_dev(c.h, p(pinned), 4, 7, 1, 0, p(rgb), None, None),
        "camera rays pinned": lambda: L.wr_camera_rays(c.h, 2, 2, native.FILM_PT, p(pinned), 1),
    }
    for name, call in cases.items():
        assert call() == native.WR_E_ARG, name
        msg = L.wr_last_error().decode()
        assert msg, name
        if "pinned" in name and "camera" not in name:
            assert "wr_" + {"closest": "trace_closest", "occluded": "occluded", "radiance": "path_radiance"}[
                name.split()[0]] in msg, msg  # the message names the host call
    torch.cuda.synchronize()  # HIP's sticky error of a failed pointer query is cleared
    assert bool((hits == 0x5A5A5A5A).all()) and bool((occ == 0xA5).all())
    assert bool((rgb == -7.0).all()) and bool((both == -7.0).all())
    assert np.array_equal(pinned.numpy(), r8)
    with pytest.raises(ValueError):
        c.trace_closest_t(pinned)  # the wrapper refuses it first
    # the same buffers in a good call
    assert L.wr_trace_closest_dev(c.h, p(rays), 4, p(hits)) == native.WR_OK
    same_records(hits, records(c.trace_closest(r8)), "after the refusals")
    assert L.wr_trace_closest_dev(c.h, None, 0, None) == native.WR_OK  # n == 0 as the host call


# ------------------------------------------------------------------ 8. multi-device context
def test_multi_device_context_runs_on_its_first_device():
    s = native.Scene(SCENES["torus64"]())
    m = native.Context(s, devices=[0, 0])
    r8, ro, tg = corpus("torus64")
    assert len(r8) >= 1024  # the host call shares this many out; the device call does not
    one = ctx_of("torus64")
    same_records(m.trace_closest_t(dev(r8)), records(one.trace_closest(r8)), "multi-device closest")
    assert np.array_equal(m.occluded_t(dev(ro), dev(tg)).cpu().numpy(), one.occluded(ro, tg))
    m.close()
