"""Shading on device arrays on the GPU (include/winmad_rt.h wr_bsdf_eval_dev /
wr_bsdf_sample_dev / wr_light_illuminate_dev / wr_light_emit_dev /
wr_light_radiance_dev / wr_rng_uniform_dev).

The calls run the device functions of csrc/wr_devmath.h that the renders run,
so the gate is the one of tests/test_gpu_devkat.py: every field the reference
wrote, bit for bit -- against the reference's own answers (tests/golden/kat_*)
and against the oracle's hooks on the random zoo cases.  Where the reference
writes nothing (the -7 mark of the hooks) a record holds 0.  The script path
tracer of tests/_script_pt.py over these calls has to reproduce the oracle's
and the library's path tracer per ray.
"""
import ctypes as C

import numpy as np
import pytest

import _kat
import _oracle
import _scenes
import _script_pt
from _kat import F, same_bits
from winmad_rt import native

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
UNSET = F(-7)
SCENES = {"torus64": lambda: _scenes.torus(64, 64), "cbox64x48": lambda: _scenes.cbox(64, 48),
          "spheres64": lambda: _scenes.spheres(64, 64), "zoo": lambda: _scenes.zoo(24, 32)}
KAT_SCENES = {"kat_torus64": "torus64", "kat_cbox64x48": "cbox64x48", "kat_spheres64": "spheres64",
              "kat_zoo": "zoo", "kat_zoo_edges": "zoo"}

_ctx = {}


def ctx_of(name):
    if name not in _ctx:
        s = native.Scene(SCENES[name]())
        _ctx[name] = (s, native.Context(s, 0))
    return _ctx[name][1]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def hit_records(normal, mat, prim=0):
    """(n, 10) int32 wr_hit records from (n, mat): t = 1, p = 0, prim as given."""
    n = len(mat)
    rec = np.zeros((n, 10), np.int32)
    rec[:, 0] = np.ones(n, F).view(np.int32)
    rec[:, 4:7] = np.ascontiguousarray(normal, F).view(np.int32)
    rec[:, 7] = prim
    rec[:, 9] = mat
    return rec


def zeroed(want):
    """The expected values with the hooks' "not written" mark replaced by the records' 0."""
    want = want.copy()
    want[want == UNSET] = 0
    return want


def check_bsdf(c, b, what):
    """The BSDF cases `b` (mat, inp = n wi wo r3, valid, out: the 26-float layout
    of tests/_kat.py) through bsdf_eval_t and bsdf_sample_t."""
    inp = b["inp"]
    hits = dev(hit_records(inp[:, 0:3], b["mat"]))
    wi, wo, r3 = dev(inp[:, 3:6]), dev(inp[:, 6:9]), dev(inp[:, 9:12])
    info, ev = c.bsdf_eval_t(hits, wi, wo)
    info2, sm = c.bsdf_sample_t(hits, wi, r3)
    assert info.dtype == ev.dtype == sm.dtype == torch.int32
    assert tuple(info.shape) == (len(inp), 9) and tuple(ev.shape) == (len(inp), 8) and tuple(sm.shape) == (len(inp), 9)
    assert bool(torch.equal(info, info2))
    fi, fe, fs = (native.bsdf_info_fields(host(info)), native.bsdf_eval_fields(host(ev)),
                  native.bsdf_sample_fields(host(sm)))
    valid = b["valid"]
    assert np.array_equal(fi["valid"], valid), (what, "valid flags", int((fi["valid"] != valid).sum()))
    dead = valid == 0
    for rec in (host(info), host(ev), host(sm)):
        assert not rec[dead].any(), (what, "records of invalid BSDFs are all zero")
    want = zeroed(b["out"])
    n = 0
    got = np.concatenate([fi["is_delta"][:, None].astype(F), fi["cos_wi"][:, None], fi["continue_prob"][:, None],
                          fi["fresnel"][:, None], fi["prob"]], 1)
    n += same_bits(got, want[:, 0:8], what + " BSDF::init")
    got = np.concatenate([fe["f"], fe["cos_wo"][:, None], fe["dir_pdf"][:, None], fe["rev_pdf"][:, None],
                          fe["pdf"][:, None], fe["pdf_rev"][:, None]], 1)
    n += same_bits(got, want[:, 8:16], what + " BSDF::f / pdf")
    got = np.concatenate([fs["type"][:, None].astype(F), fs["f"], fs["wo"], fs["pdf"][:, None], fs["cos_wo"][:, None]], 1)
    n += same_bits(got, want[:, 16:25], what + " BSDF::sample")
    return n, int((b["out"][~dead] == UNSET).sum())


def check_light(c, li, what):
    """The light cases `li` (li, inp = pos r3 dir_r3 pos_r3 ray_d, out: the 27-float layout)."""
    inp, ids = li["inp"], dev(li["li"])
    want = zeroed(li["out"])
    il = host(c.light_illuminate_t(ids, dev(inp[:, 0:3]), dev(inp[:, 3:6])))
    em = host(c.light_emit_t(ids, dev(inp[:, 6:9]), dev(inp[:, 9:12])))
    hits = dev(hit_records(np.zeros((len(inp), 3), F), -li["li"] - 1))
    ra = host(c.light_radiance_t(hits, dev(inp[:, 12:15])))
    assert il.shape == (len(inp), 10) and em.shape == (len(inp), 12) and ra.shape == (len(inp), 5)
    n = same_bits(il.view(F), want[:, 0:10], what + " AreaLight::illuminance")
    n += same_bits(em.view(F), want[:, 10:22], what + " AreaLight::emit")
    n += same_bits(ra.view(F), want[:, 22:27], what + " AreaLight::getRadiance")
    f = native.light_fields(ra)
    assert np.array_equal(f["le"].view(np.uint32), want[:, 22:25].view(np.uint32))
    return n


# ------------------------------------------------------------------ 1. the reference's answers
@pytest.mark.parametrize("name", list(KAT_SCENES))
def test_calls_equal_the_reference_answers(name):
    k = _kat.parse(name)
    c = ctx_of(KAT_SCENES[name])
    nb, unwritten = check_bsdf(c, k["bsdf"], name)
    nl = check_light(c, k["light"], name)
    print(name, "bsdf values:", nb, "light values:", nl, "fields the reference left unwritten:", unwritten,
          "invalid BSDFs:", int((k["bsdf"]["valid"] == 0).sum()))
    assert nb > 0 and nl > 0


# ------------------------------------------------------------------ 2. the oracle on random cases
def test_calls_equal_the_oracle_on_random_cases():
    cases = _kat.zoo_random_cases()
    stats = _kat.check_zoo_random_cases(cases)
    c = ctx_of("zoo")
    nb, unwritten = check_bsdf(c, cases["bsdf"], "random")
    nl = check_light(c, cases["light"], "random")
    print("bsdf values:", nb, "light values:", nl, "unwritten fields:", unwritten, stats)
    assert unwritten > 0 and stats["bsdf_invalid"] > 0


# ------------------------------------------------------------------ 3. RNG
def test_rng_draws_equal_the_oracle_streams():
    c = ctx_of("torus64")
    L = _oracle.lib()
    n, seed, it, sub = 1000, 77, 3, 2
    rng = np.random.default_rng(5)
    path = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    path[:4] = (0, 1, 0x7FFFFFFF, 0xFFFFFFFF)
    want = np.zeros((n, 7), F)
    for i, p in enumerate(path.tolist()):
        key = L.cr_stream_key(seed, it, sub, p)
        for j in range(7):
            want[i, j] = F(L.cr_stream_u32(key, j) & 0xFFFFFF) / F(16777216.0)
    pt = dev(path.view(np.int32))
    got = c.rng_uniform_t(n, 7, seed, it, sub, path=pt)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 7)
    same_bits(host(got), want, "rng_uniform_t, 7 draws")
    # the same draws in two calls, the counter carried
    ctr = torch.zeros((n,), dtype=torch.int32, device=DEV)
    a = c.rng_uniform_t(n, 3, seed, it, sub, path=pt, ctr=ctr)
    assert bool((ctr == 3).all())
    b = c.rng_uniform_t(n, 4, seed, it, sub, path=pt, ctr=ctr)
    assert bool((ctr == 7).all())
    same_bits(np.concatenate([host(a), host(b)], 1), want, "rng_uniform_t, 3 + 4 draws")
    # path = None is path k = k
    ar = torch.arange(n, dtype=torch.int32, device=DEV)
    assert bool(torch.equal(c.rng_uniform_t(n, 7, seed, it, sub), c.rng_uniform_t(n, 7, seed, it, sub, path=ar)))
    key0 = L.cr_stream_key(seed, it, sub, 0)
    assert float(c.rng_uniform_t(1, 1, seed, it, sub)[0, 0]) == float(F(L.cr_stream_u32(key0, 0) & 0xFFFFFF) / F(2 ** 24))


# ------------------------------------------------------------------ 4. from real hits
@pytest.mark.parametrize("name", ["torus64", "cbox64x48", "spheres64"])
def test_shading_of_traced_camera_rays(name):
    c = ctx_of(name)
    sc = _oracle.Scene(SCENES[name]())
    W, H = (64, 48) if name == "cbox64x48" else (64, 64)
    rays = c.camera_rays_t(W, H, native.FILM_PT if name == "cbox64x48" else native.FILM_BDPT)
    hits = c.trace_closest_t(rays)
    d = rays[:, 3:6].contiguous()
    wi = -d
    f = native.hit_fields(host(hits))
    wo = dev(f["n"])  # evaluate towards the normal
    info, ev = c.bsdf_eval_t(hits, wi, wo)
    hit = f["prim"] >= 0
    assert hit.any()
    inp = np.concatenate([f["n"], host(wi), f["n"], np.zeros((len(hit), 3), F)], 1)[hit]
    want, valid = _kat.oracle_bsdf(sc, f["mat_id"][hit], inp)
    fi, fe = native.bsdf_info_fields(host(info)), native.bsdf_eval_fields(host(ev))
    assert not fi["valid"][~hit].any()
    assert np.array_equal(fi["valid"][hit], valid)
    assert not host(info)[fi["valid"] == 0].any() and not host(ev)[fi["valid"] == 0].any()
    want = zeroed(want)
    same_bits(np.concatenate([fi["cos_wi"][:, None], fi["continue_prob"][:, None], fi["fresnel"][:, None], fi["prob"]],
                             1)[hit], want[:, 1:8], name + " BSDF::init of the hits")
    same_bits(np.concatenate([fe["f"], fe["cos_wo"][:, None], fe["dir_pdf"][:, None], fe["rev_pdf"][:, None],
                              fe["pdf"][:, None], fe["pdf_rev"][:, None]], 1)[hit],
              want[:, 8:16], name + " BSDF::f / pdf of the hits")
    # emitters: radiance is non-zero exactly where the hit is on a light that faces the ray (cos > EPS)
    rad = host(c.light_radiance_t(hits, d)).view(F)
    em = hit & (f["mat_id"] < 0)
    assert not rad[~em].any()
    k = np.flatnonzero(em)
    if len(k):
        linp = np.zeros((len(k), 15), F)
        linp[:, 12:15] = host(d)[k]
        lw = zeroed(_kat.oracle_light(sc, -f["mat_id"][k] - 1, linp))[:, 22:27]
        same_bits(rad[k], lw, name + " getRadiance of the emitter hits")
        # (getRadiance returns Le where cmpf(cos) != 0 with cos clamped to [0, 1]: the oracle's rows say where)
        print(name, "emitter hits:", len(k), "lit:", int(rad[k, 0:3].any(1).sum()))
        assert np.array_equal(rad[k, 0:3].any(1), lw[:, 0:3].any(1))
    print(name, "hits:", int(hit.sum()), "invalid at a hit:", int((valid == 0).sum()), "emitter hits:", len(k))
    if name == "cbox64x48":
        assert len(k) > 0 and rad[k, 0:3].any()  # the luminaire is in view


# ------------------------------------------------------------------ 5. completeness
def test_script_path_tracer_over_the_calls_equals_the_path_tracers():
    """tests/_script_pt.py over the device calls: the 2,048 rays, scene and
    parameters of test_shading_host's oracle-backend test; the gate is the
    project's per-ray radiance gate 1e-5 |ref| + 1e-30 against the oracle's
    PathIntegrator::raytracing and against path_radiance_t, no ray exempt."""
    c = ctx_of("cbox64x48")
    o, d = _script_pt.cbox_rays(2048)
    ref, _ = _oracle.Scene(SCENES["cbox64x48"]()).pt_radiance(np.concatenate([o, d], 1), 7, 77, sample=3)
    assert ref.sum() > 0
    got = host(_script_pt.radiance(_script_pt.DeviceBackend(c, 77, 3), dev(o), dev(d), 7))
    lib, _ = c.path_radiance_t(dev(native.rays_from_arrays(o, d)), max_depth=7, seed=77, sample=3)
    lib = host(lib)
    assert got.dtype == np.float32 and np.all(np.isfinite(got))
    for want, what in ((ref, "oracle"), (lib, "path_radiance_t")):
        err = np.abs(got.astype(np.float64) - want)
        ok = np.all(err <= 1e-5 * np.abs(want) + 1e-30, axis=1)
        print("against", what, "rays off:", int((~ok).sum()), "of", len(ok), "bit-equal rays:",
              int((got.view(np.uint32) == want.view(np.uint32)).all(1).sum()))
        assert ok.all(), (what, np.argwhere(~ok)[:5].ravel())


# ------------------------------------------------------------------ 6. robustness
@pytest.fixture(scope="module")
def zoo_inputs():
    """1,000 random BSDF and light cases on the zoo, on the device, with the calls' answers."""
    c = ctx_of("zoo")
    cases = _kat.zoo_random_cases()
    n = 1000
    pick = np.random.default_rng(1).permutation(len(cases["bsdf"]["mat"]))[:n]
    b = cases["bsdf"]["inp"][pick]
    x = {"hits": dev(hit_records(b[:, 0:3], cases["bsdf"]["mat"][pick])), "wi": dev(b[:, 3:6]), "wo": dev(b[:, 6:9]),
         "r3": dev(b[:, 9:12])}
    pick = np.random.default_rng(2).permutation(len(cases["light"]["li"]))[:n]
    l = cases["light"]["inp"][pick]
    x.update(light=dev(cases["light"]["li"][pick]), pos=dev(l[:, 0:3]), lr3=dev(l[:, 3:6]), dr=dev(l[:, 6:9]),
             pr=dev(l[:, 9:12]), rd=dev(l[:, 12:15]))
    x["lhits"] = dev(hit_records(np.zeros((n, 3), F), -cases["light"]["li"][pick] - 1))
    x["info"], x["eval"] = c.bsdf_eval_t(x["hits"], x["wi"], x["wo"])
    _, x["sample"] = c.bsdf_sample_t(x["hits"], x["wi"], x["r3"])
    x["illum"] = c.light_illuminate_t(x["light"], x["pos"], x["lr3"])
    x["emit"] = c.light_emit_t(x["light"], x["dr"], x["pr"])
    x["rad"] = c.light_radiance_t(x["lhits"], x["rd"])
    assert bool(x["eval"].any()) and bool(x["sample"].any()) and bool(x["illum"].any()) and bool(x["rad"].any())
    return c, n, x


def shifted(t):
    """A copy of t one record into a larger buffer: a view with the alignment of one record."""
    big = torch.zeros((t.shape[0] + 1,) + tuple(t.shape[1:]), dtype=t.dtype, device=DEV)
    big[1:] = t
    return big[1:]


def test_records_need_only_four_byte_alignment(zoo_inputs):
    c, n, x = zoo_inputs
    s = {k: shifted(v) for k, v in x.items()}
    assert s["wi"].data_ptr() % 8 == 4 and s["hits"].data_ptr() % 16 == 8 and s["light"].data_ptr() % 8 == 4
    outs = {k: torch.full((n + 1, w), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
            for k, w in (("info", 9), ("eval", 8), ("sample", 9), ("illum", 10), ("emit", 12), ("rad", 5))}
    assert outs["info"][1:].data_ptr() % 8 == 4 and outs["rad"][1:].data_ptr() % 8 == 4
    c.bsdf_eval_t(s["hits"], s["wi"], s["wo"], info=outs["info"][1:], out=outs["eval"][1:])
    c.bsdf_sample_t(s["hits"], s["wi"], s["r3"], out=outs["sample"][1:])
    c.light_illuminate_t(s["light"], s["pos"], s["lr3"], out=outs["illum"][1:])
    c.light_emit_t(s["light"], s["dr"], s["pr"], out=outs["emit"][1:])
    c.light_radiance_t(s["lhits"], s["rd"], out=outs["rad"][1:])
    for k, o in outs.items():
        assert bool(torch.equal(o[1:], x[k])), k
        assert bool((o[0] == 0x5A5A5A5A).all()), k
    rbig = torch.full((n + 1, 3), -7.0, dtype=torch.float32, device=DEV)
    c.rng_uniform_t(n, 3, 1, 2, 3, path=shifted(torch.arange(n, dtype=torch.int32, device=DEV)), out=rbig[1:])
    assert bool(torch.equal(rbig[1:], c.rng_uniform_t(n, 3, 1, 2, 3))) and bool((rbig[0] == -7.0).all())


def test_n_zero(zoo_inputs):
    c, n, x = zoo_inputs
    e = lambda k: x[k][:0]
    info, ev = c.bsdf_eval_t(e("hits"), e("wi"), e("wo"))
    assert tuple(info.shape) == (0, 9) and tuple(ev.shape) == (0, 8)
    assert tuple(c.bsdf_sample_t(e("hits"), e("wi"), e("r3"))[1].shape) == (0, 9)
    assert tuple(c.light_illuminate_t(e("light"), e("pos"), e("lr3")).shape) == (0, 10)
    assert tuple(c.light_emit_t(e("light"), e("dr"), e("pr")).shape) == (0, 12)
    assert tuple(c.light_radiance_t(e("lhits"), e("rd")).shape) == (0, 5)
    assert tuple(c.rng_uniform_t(0, 3, 1, 2, 3).shape) == (0, 3)
    L = native.lib()
    assert L.wr_bsdf_eval_dev(c.h, None, None, None, 0, None, None) == native.WR_OK
    assert L.wr_rng_uniform_dev(c.h, 1, 2, 3, None, None, 3, 0, None) == native.WR_OK


def test_indices_outside_the_scene_give_zero_records(zoo_inputs):
    c, n, x = zoo_inputs
    info = c.scene.info()
    nl, nm = info["nlights"], info["nmaterials"]
    assert nl > 0 and nm == _kat.NMAT
    light = x["light"].clone()
    light[100], light[200] = -1, nl
    il = c.light_illuminate_t(light, x["pos"], x["lr3"])
    em = c.light_emit_t(light, x["dr"], x["pr"])
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[100] = keep[200] = False
    for got, k in ((il, "illum"), (em, "emit")):
        assert not bool(got[~keep].any()), k
        assert bool(x[k][~keep].any()), k  # (the good indices gave values there)
        assert bool(torch.equal(got[keep], x[k][keep])), k
    hits = x["hits"].clone()
    hits[100, 9], hits[200, 9] = nm, -nl - 1
    info_t, ev = c.bsdf_eval_t(hits, x["wi"], x["wo"])
    _, sm = c.bsdf_sample_t(hits, x["wi"], x["r3"])
    lh = x["lhits"].clone()
    lh[100, 9], lh[200, 9] = nm, -nl - 1
    ra = c.light_radiance_t(lh, x["rd"])
    for got, k in ((info_t, "info"), (ev, "eval"), (sm, "sample"), (ra, "rad")):
        assert not bool(got[~keep].any()), k
        assert bool(torch.equal(got[keep], x[k][keep])), k
    assert bool(x["info"][~keep].any())
    # the largest indices the scene has are fine
    hits[100, 9], hits[200, 9] = nm - 1, -nl
    assert bool(c.bsdf_eval_t(hits, x["wi"], x["wo"])[0][200, 0] == 1)


def test_scene_without_lights():
    """The light calls need a light (WR_E_SCENE); the BSDF calls do not, and an
    emitter id has nothing to point at: a zero record."""
    import _tiny_scenes
    c = native.Context(native.Scene(_tiny_scenes.tiny(1)), 0)
    assert c.scene.info()["nlights"] == 0
    n = 5
    v = torch.rand((n, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    up = torch.tensor([[0.0, 1.0, 0.0]], device=DEV).repeat(n, 1)
    light = torch.zeros((n,), dtype=torch.int32, device=DEV)
    rec = hit_records(host(up), np.array([1, 1, -1, 1, 1], np.int32))
    hits = dev(rec)
    for call in (lambda: c.light_illuminate_t(light, v, v), lambda: c.light_emit_t(light, v, v),
                 lambda: c.light_radiance_t(hits, v)):
        with pytest.raises(native.WrError) as e:
            call()
        assert e.value.code == native.WR_E_SCENE
    info, ev = c.bsdf_eval_t(hits, up, up)
    valid = host(native.bsdf_info_fields(info)["valid"])
    assert valid.tolist() == [1, 1, 0, 1, 1] and not bool(ev[2].any()) and bool(ev[0].any())
    c.close()


def test_call_is_ordered_after_pending_default_stream_work():
    """The pattern of test_gpu_device_rays' ordering test at 2^18 records: the
    positions come out of a chain of torch ops on the default stream that is
    still running when light_illuminate_t is issued, with no synchronize."""
    c = ctx_of("zoo")
    n = 1 << 18
    g = torch.Generator(device=DEV).manual_seed(3)
    base = torch.rand((n, 3), device=DEV, generator=g) * 2.6 - 1.3
    r3 = torch.rand((n, 3), device=DEV, generator=g)
    light = torch.zeros((n,), dtype=torch.int32, device=DEV)
    eye = torch.eye(4096, dtype=torch.float32, device=DEV)
    shift = torch.tensor([0.25, -0.125, 0.0625], device=DEV)
    pos = base.clone()

    def produce():
        x = eye
        for _ in range(8):
            x = x @ eye  # stays the identity
        pos.copy_(base + shift * x[0, 0])

    produce()
    torch.cuda.synchronize()
    want = c.light_illuminate_t(light, pos.clone(), r3)
    stale = c.light_illuminate_t(light, base, r3)
    assert not bool(torch.equal(stale, want))
    pos.copy_(base)
    torch.cuda.synchronize()
    produce()
    got = c.light_illuminate_t(light, pos, r3)  # no synchronize before
    assert bool(torch.equal(got, want))
    assert bool(got.any())


def test_bad_pointers_are_refused_and_hip_stays_clean(zoo_inputs):
    c, n, x = zoo_inputs
    L = native.lib()
    m = 8
    p = lambda t: C.c_void_p(t.data_ptr())
    hits, wi, wo, r3 = x["hits"][:m].clone(), x["wi"][:m].clone(), x["wo"][:m].clone(), x["r3"][:m].clone()
    light = x["light"][:m].clone()
    host_wi = np.zeros((m, 3), F)
    pinned = torch.zeros((m, 3), dtype=torch.float32).pin_memory()
    ev = torch.full((m, 8), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    il = torch.full((m, 12), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    both = torch.zeros((m * 16,), dtype=torch.float32, device=DEV)  # an input and an output in one buffer
    ctr = torch.zeros((m,), dtype=torch.int32, device=DEV)
    rout = torch.full((m, 3), -7.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    cases = {
        "eval host wi": lambda: L.wr_bsdf_eval_dev(c.h, p(hits), C.c_void_p(host_wi.ctypes.data), p(wo), m, None, p(ev)),
        "eval pinned wi": lambda: L.wr_bsdf_eval_dev(c.h, p(hits), p(pinned), p(wo), m, None, p(ev)),
        "eval out overlaps wo": lambda: L.wr_bsdf_eval_dev(c.h, p(hits), p(wi), p(both), m, None,
                                                           C.c_void_p(both.data_ptr() + 16)),
        "eval info is out": lambda: L.wr_bsdf_eval_dev(c.h, p(hits), p(wi), p(wo), m, p(il), p(il)),
        "eval null out": lambda: L.wr_bsdf_eval_dev(c.h, p(hits), p(wi), p(wo), m, None, None),
        "eval n = 2^28 + 1": lambda: L.wr_bsdf_eval_dev(c.h, p(hits), p(wi), p(wo), (1 << 28) + 1, None, p(ev)),
        "sample pinned r3": lambda: L.wr_bsdf_sample_dev(c.h, p(hits), p(wi), p(pinned), m, None, p(il)),
        "illuminate pinned pos": lambda: L.wr_light_illuminate_dev(c.h, p(light), p(pinned), p(r3), m, p(il)),
        "illuminate out overlaps light": lambda: L.wr_light_illuminate_dev(c.h, p(both), p(wi), p(r3), m,
                                                                           C.c_void_p(both.data_ptr() + 4)),
        "emit host r3": lambda: L.wr_light_emit_dev(c.h, p(light), C.c_void_p(host_wi.ctypes.data), p(r3), m, p(il)),
        "radiance pinned d": lambda: L.wr_light_radiance_dev(c.h, p(hits), p(pinned), m, p(il)),
        "rng draws = 0": lambda: L.wr_rng_uniform_dev(c.h, 1, 2, 3, None, p(ctr), 0, m, p(rout)),
        "rng draws = 65": lambda: L.wr_rng_uniform_dev(c.h, 1, 2, 3, None, p(ctr), 65, m, p(rout)),
        "rng out is ctr": lambda: L.wr_rng_uniform_dev(c.h, 1, 2, 3, None, p(ctr), 1, m, p(ctr)),
        "rng pinned out": lambda: L.wr_rng_uniform_dev(c.h, 1, 2, 3, None, None, 3, m, p(pinned)),
    }
    for name, call in cases.items():
        assert call() == native.WR_E_ARG, name
        msg = L.wr_last_error().decode()
        assert "wr_" + {"eval": "bsdf_eval", "sample": "bsdf_sample", "illuminate": "light_illuminate",
                        "emit": "light_emit", "radiance": "light_radiance", "rng": "rng_uniform"}[name.split()[0]] in msg, msg
    torch.cuda.synchronize()  # HIP's error state is clean: nothing sticky from the failed pointer queries
    assert bool((ev == 0x5A5A5A5A).all()) and bool((il == 0x5A5A5A5A).all()) and bool((rout == -7.0).all())
    assert not bool(ctr.any()) and not bool(pinned.any()) and not bool(both.any())
    # the same buffers in good calls
    assert L.wr_bsdf_eval_dev(c.h, p(hits), p(wi), p(wo), m, None, p(ev)) == native.WR_OK
    assert bool(torch.equal(ev, x["eval"][:m]))
    assert L.wr_rng_uniform_dev(c.h, 1, 2, 3, None, p(ctr), 3, m, p(rout)) == native.WR_OK
    assert bool((ctr == 3).all()) and bool(torch.equal(rout, c.rng_uniform_t(m, 3, 1, 2, 3)))


def test_wrappers_refuse_wrong_tensors(zoo_inputs):
    c, n, x = zoo_inputs
    hits, wi, wo = x["hits"], x["wi"], x["wo"]
    bad = {"dtype": wi.double(), "shape": wi[:, :2].contiguous(), "rows": wi[:-1], "device": wi.cpu(),
           "non-contiguous": torch.zeros((n, 6), dtype=torch.float32, device=DEV)[:, ::2]}
    for what, t in bad.items():
        for call in (lambda: c.bsdf_eval_t(hits, t, wo), lambda: c.bsdf_eval_t(hits, wi, t),
                     lambda: c.bsdf_sample_t(hits, wi, t), lambda: c.light_illuminate_t(x["light"], t, x["lr3"]),
                     lambda: c.light_emit_t(x["light"], x["dr"], t), lambda: c.light_radiance_t(x["lhits"], t)):
            with pytest.raises(ValueError):
                call()
    for t in (hits.to(torch.int64), hits[:, :9].contiguous(), hits.cpu(), hits.view(torch.float32)):
        with pytest.raises(ValueError):
            c.bsdf_eval_t(t, wi, wo)
    with pytest.raises(ValueError):
        c.light_illuminate_t(x["light"].to(torch.int64), x["pos"], x["lr3"])
    with pytest.raises(ValueError):
        c.bsdf_eval_t(hits, wi, wo, out=torch.zeros((n, 8), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        c.rng_uniform_t(n, 3, 1, 2, 3, out=torch.zeros((n, 4), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        c.rng_uniform_t(n, 3, 1, 2, 3, ctr=torch.zeros((n,), dtype=torch.int32))


# ------------------------------------------------------------------ 7. nothing else moved
def test_renders_are_unchanged_by_a_burst_of_shading_calls():
    """A 64 x 64 torus BDPT film and a cbox PT film rendered before and after a
    burst of shading calls on the same contexts are bit-equal."""
    ct, cb = ctx_of("torus64"), ctx_of("cbox64x48")
    before = (ct.render_bdpt(64, 64, iterations=1, seed=5489)[0], cb.render_path(64, 48, 1, max_depth=7, seed=5489)[0])
    for c in (ct, cb):
        rays = c.camera_rays_t(64, 48)
        hits = c.trace_closest_t(rays)
        d = rays[:, 3:6].contiguous()
        k = len(d)
        light = torch.zeros((k,), dtype=torch.int32, device=DEV)
        for rep in range(4):
            u = c.rng_uniform_t(k, 6, 5489, rep, 2)
            a, b = u[:, 0:3].contiguous(), u[:, 3:6].contiguous()
            c.bsdf_eval_t(hits, -d, a)
            c.bsdf_sample_t(hits, -d, a)
            c.light_illuminate_t(light, native.hit_fields(hits)["p"].contiguous(), b)
            c.light_emit_t(light, a, b)
            c.light_radiance_t(hits, d)
    after = (ct.render_bdpt(64, 64, iterations=1, seed=5489)[0], cb.render_path(64, 48, 1, max_depth=7, seed=5489)[0])
    for a, b, what in zip(before, after, ("torus BDPT", "cbox PT")):
        assert a.any()
        diff = int((a.view(np.uint32) != b.view(np.uint32)).sum())
        print(what, "values that differ:", diff, "of", a.size)
        assert diff == 0, what
