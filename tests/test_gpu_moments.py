"""Second-moment films on the GPU (include/winmad_rt.h).

A moments render accumulates film += sum_i F_i and film_sq += sum_i F_i o F_i,
F_i the complete film of pass i (a BDPT / VCM iteration, a PT sample index).
The oracle renders single passes (iter_begin / k_begin), so the references are
    ref    = sum_i oracle(pass i)
    ref_sq = sum_i oracle(pass i)^2     (squared and summed in float64)
and both films pass the film gates of tests/_parity.py at their defaults.  A
square's relative error is twice the film's plus one rounding, and the film's
(<= 8.2e-8 relative RMSE) is more than 10x inside the gates.
"""
import functools
import os
import subprocess
import types

import numpy as np
import pytest

import _oracle
import _scenes
from _parity import assert_film_parity, assert_ray_counts, assert_vcm_parity
from winmad_rt import native

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _sum_passes(render_pass, begin, count):
    """ref, ref_sq (float64) and the summed ray counts of the oracle's passes [begin, begin + count)."""
    ref = ref_sq = None
    rays = types.SimpleNamespace(closest_rays=0, shadow_rays=0)
    for i in range(begin, begin + count):
        f, st = render_pass(i)
        f = f.astype(np.float64)
        ref = f if ref is None else ref + f
        ref_sq = f * f if ref_sq is None else ref_sq + f * f
        rays.closest_rays += st.closest_rays
        rays.shadow_rays += st.shadow_rays
    ref.setflags(write=False)
    ref_sq.setflags(write=False)
    return ref, ref_sq, rays


BDPT_CASES = {  # name: scene, W, H, control_length, iterations, iter_begin, seed
    "cbox": (lambda: _scenes.cbox(32, 24, "bdpt"), 32, 24, 0, 4, 5, 7),
    "torus": (lambda: _scenes.torus(48, 48), 48, 48, 3, 4, 0, 11),  # splat-dominated, 16 % of the pixels lit
    "spheres": (lambda: _scenes.spheres(32, 32), 32, 32, 3, 4, 1, 5489),
}


@functools.lru_cache(maxsize=None)
def _bdpt_oracle(name, begin, count):
    maker, W, H, ctl, _, _, seed = BDPT_CASES[name]
    sc = _oracle.Scene(maker())
    return _sum_passes(lambda i: sc.bdpt(W, H, 1, seed, mode=1, control_length=ctl, iter_begin=i), begin, count)


def _dev_films(W, H):
    return (torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0"),
            torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0"))


@functools.lru_cache(maxsize=None)
def _bdpt_render(name):
    """The moments render of a case into device films (kept with their context
    for the wr_film_error test), and the plain render of the same call."""
    maker, W, H, ctl, it, begin, seed = BDPT_CASES[name]
    c = native.Context(native.Scene(maker()), 0)
    film, sq = _dev_films(W, H)
    torch.cuda.synchronize()
    _, _, st = c.render_bdpt_moments(W, H, iterations=it, seed=seed, iter_begin=begin, control_length=ctl,
                                     film_ptr=film.data_ptr(), film_sq_ptr=sq.data_ptr())
    plain, pst = c.render_bdpt(W, H, iterations=it, seed=seed, iter_begin=begin, control_length=ctl)
    return types.SimpleNamespace(ctx=c, film=film, sq=sq, st=st, plain=plain, pst=pst, W=W, H=H, n=it)


@pytest.mark.parametrize("name", list(BDPT_CASES))
def test_bdpt_moments_match_the_oracle_passes(name):
    r = _bdpt_render(name)
    _, _, _, ctl, it, begin, seed = BDPT_CASES[name]
    ref, ref_sq, rays = _bdpt_oracle(name, begin, it)
    case = f"moments_bdpt_{name}{r.W}x{r.H}_i{it}_b{begin}_s{seed}_ctl{ctl}"
    film, sq = r.film.cpu().numpy(), r.sq.cpu().numpy()
    assert_film_parity(film, ref, case=case)
    assert_film_parity(sq, ref_sq, case=case, kind="film_sq")
    assert_ray_counts(r.st, rays)
    # `film` is what the plain render of the same call adds
    assert_film_parity(film, r.plain, case=case, kind="film_vs_plain")
    assert_ray_counts(r.st, r.pst)
    # (cbox and spheres fill the default pools at this size, as their plain
    # renders do: both films then come through the redo as well)
    assert r.st.redone == r.pst.redone


def test_bdpt_moments_square_whole_passes_not_pieces(monkeypatch):
    """An iteration of 768 paths in three pieces of 256, the render on several
    pipelines: the square is still the complete iteration film's (squaring per
    piece would give a smaller film_sq wherever two pieces light one pixel)."""
    monkeypatch.setenv("WR_PIECE_MIN", "64")
    monkeypatch.setenv("WR_PIECE_CAP", "256")
    monkeypatch.setenv("WR_PIPES", "4")
    maker, W, H, ctl, it, begin, seed = BDPT_CASES["cbox"]
    c = native.Context(native.Scene(maker()), 0)
    film, sq, st = c.render_bdpt_moments(W, H, iterations=it, seed=seed, iter_begin=begin, control_length=ctl)
    c.close()
    assert st.pipelines > 1, st.pipelines
    ref, ref_sq, rays = _bdpt_oracle("cbox", begin, it)
    assert_film_parity(film, ref, case="moments_bdpt_cbox32x24_pieces")
    assert_film_parity(sq, ref_sq, case="moments_bdpt_cbox32x24_pieces", kind="film_sq")
    assert_ray_counts(st, rays)


def test_bdpt_moments_redo_puts_both_films_back(monkeypatch):
    """Tiny pools (the torus 96x64 case of tests/test_gpu_pools.py): the render
    overflows and is redone from both films as they were -- device films that
    already hold a first call's sums end as earlier + new."""
    monkeypatch.setenv("WR_BDPT_POOL_SCALE", "0.002")
    W, H, seed = 96, 64, 7
    path = _scenes.torus(W, H)
    c = native.Context(native.Scene(path), 0)
    film, sq = _dev_films(W, H)
    torch.cuda.synchronize()
    c.render_bdpt_moments(W, H, iterations=2, seed=seed, film_ptr=film.data_ptr(), film_sq_ptr=sq.data_ptr())
    torch.cuda.synchronize()
    early, early_sq = film.cpu().numpy().astype(np.float64), sq.cpu().numpy().astype(np.float64)
    _, _, st = c.render_bdpt_moments(W, H, iterations=2, seed=seed, iter_begin=2, film_ptr=film.data_ptr(),
                                     film_sq_ptr=sq.data_ptr())
    torch.cuda.synchronize()
    c.close()
    assert st.redone >= 1, st.redone
    sc = _oracle.Scene(path)
    old, old_sq, _ = _sum_passes(lambda i: sc.bdpt(W, H, 1, seed, mode=1, iter_begin=i), 0, 2)
    new, new_sq, rays = _sum_passes(lambda i: sc.bdpt(W, H, 1, seed, mode=1, iter_begin=i), 2, 2)
    assert_film_parity(early, old, case="moments_bdpt_torus96x64_redo_first")
    assert_film_parity(early_sq, old_sq, case="moments_bdpt_torus96x64_redo_first", kind="film_sq")
    assert_film_parity(film.cpu().numpy(), early + new, case="moments_bdpt_torus96x64_redo")
    assert_film_parity(sq.cpu().numpy(), early_sq + new_sq, case="moments_bdpt_torus96x64_redo", kind="film_sq")
    assert_ray_counts(st, rays)


def test_bdpt_moments_calls_over_disjoint_passes_add_up():
    """Iterations [0, 2) then [2, 4) into the same device films: one call over [0, 4)."""
    W, H, seed = 48, 48, 11
    c = native.Context(native.Scene(_scenes.torus(W, H)), 0)
    film, sq = _dev_films(W, H)
    torch.cuda.synchronize()
    _, _, s0 = c.render_bdpt_moments(W, H, iterations=2, seed=seed, film_ptr=film.data_ptr(), film_sq_ptr=sq.data_ptr())
    _, _, s1 = c.render_bdpt_moments(W, H, iterations=2, seed=seed, iter_begin=2, film_ptr=film.data_ptr(),
                                     film_sq_ptr=sq.data_ptr())
    one, one_sq, st = c.render_bdpt_moments(W, H, iterations=4, seed=seed)
    torch.cuda.synchronize()
    c.close()
    assert s0.closest_rays + s1.closest_rays == st.closest_rays
    assert s0.shadow_rays + s1.shadow_rays == st.shadow_rays
    assert_film_parity(film.cpu().numpy(), one, case="moments_bdpt_torus48x48_additive", kind="film_vs_one_call")
    assert_film_parity(sq.cpu().numpy(), one_sq, case="moments_bdpt_torus48x48_additive", kind="film_sq_vs_one_call")
    ref, ref_sq, rays = _bdpt_oracle("torus", 0, 4)
    assert_film_parity(one, ref, case="moments_bdpt_torus48x48_host")
    assert_film_parity(one_sq, ref_sq, case="moments_bdpt_torus48x48_host", kind="film_sq")
    assert_ray_counts(st, rays)


def test_vcm_moments_match_the_oracle_passes():
    """iter_begin = 2: the merge radius follows the global iteration index."""
    W, H, it, begin, seed = 32, 32, 3, 2, 19
    path = _scenes.spheres(W, H)
    c = native.Context(native.Scene(path), 0)
    film, sq, st = c.render_vcm_moments(W, H, iterations=it, seed=seed, iter_begin=begin)
    plain, pst = c.render_vcm(W, H, iterations=it, seed=seed, iter_begin=begin)
    c.close()
    sc = _oracle.Scene(path)
    ref, ref_sq, rays = _sum_passes(lambda i: sc.vcm(W, H, 1, seed, mode=1, iter_begin=i), begin, it)
    assert_vcm_parity(film, ref, case="moments_vcm_spheres32x32_i3_b2_s19")
    assert_vcm_parity(sq, ref_sq, case="moments_vcm_spheres32x32_i3_b2_s19_sq")
    assert_ray_counts(st, rays)
    assert_vcm_parity(film, plain, case="moments_vcm_spheres32x32_vs_plain")
    assert_ray_counts(st, pst)


def test_path_moments_match_the_oracle_samples():
    """spp = 5: a 2x2 grid plus one overshoot sample; then samples [2, 5) alone."""
    W, H, spp, depth, seed = 32, 24, 5, 7, 23
    path = _scenes.cbox(W, H)
    c = native.Context(native.Scene(path), 0)
    sc = _oracle.Scene(path)
    one = lambda k: sc.pt_samples(W, H, spp, k, 1, depth, seed, mode=1)  # noqa: E731
    for k0, n in ((0, 5), (2, 3)):
        film, sq, st = c.render_path_moments(W, H, spp, max_depth=depth, seed=seed, sample_begin=k0, sample_count=n)
        plain, pst = c.render_path(W, H, spp, max_depth=depth, seed=seed, sample_begin=k0, sample_count=n)
        ref, ref_sq, rays = _sum_passes(one, k0, n)
        case = f"moments_pt_cbox32x24_spp5_k{k0}_n{n}"
        assert_film_parity(film, ref, case=case)
        assert_film_parity(sq, ref_sq, case=case, kind="film_sq")
        assert_ray_counts(st, rays)
        assert_film_parity(film, plain, case=case, kind="film_vs_plain")
        assert_ray_counts(st, pst)
    c.close()


@pytest.mark.parametrize("name", list(BDPT_CASES))
def test_film_error_on_device_films_equals_the_host_path(name):
    """k_film_error on the device films of the BDPT cases: the host loop's
    numbers on the same arrays copied back (double arithmetic, another summation
    order: 1e-9), and the map is the numpy map stored as float (1e-6)."""
    r = _bdpt_render(name)
    se_dev = torch.full((r.H, r.W, 3), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    dev = r.ctx.film_error(r.film.data_ptr(), r.sq.data_ptr(), r.W, r.H, r.n, stderr_map_ptr=se_dev.data_ptr())
    nomap = r.ctx.film_error(r.film.data_ptr(), r.sq.data_ptr(), r.W, r.H, r.n)
    S, Q = r.film.cpu().numpy(), r.sq.cpu().numpy()
    host, se_host = native.film_error(S, Q, r.n, stderr_map=True)
    for k in ("sum_stderr", "sum_mean", "rel_stderr", "max_rel_stderr"):
        a, b, c = getattr(dev, k), getattr(host, k), getattr(nomap, k)
        print(name, k, a, b)
        assert b > 0 and abs(a - b) <= 1e-9 * b and abs(c - b) <= 1e-9 * b, (k, a, b, c)
    assert dev.values == host.values == nomap.values == int((S > 0).sum())
    s, q = S.astype(np.float64), Q.astype(np.float64)
    se = np.sqrt(np.maximum(0.0, (q - s * s / r.n) / (r.n - 1)) / r.n)
    got = se_dev.cpu().numpy()
    assert np.all(np.abs(got - se) <= 1e-6 * se), float(np.abs(got - se).max())
    assert np.all(np.abs(got - se_host) <= 1e-6 * se)
    with pytest.raises(native.WrError):
        r.ctx.film_error(r.film.data_ptr(), r.sq.data_ptr(), r.W, r.H, 1)


def test_moments_on_a_multi_device_context_are_refused():
    W, H = 32, 24
    c = native.Context(native.Scene(_scenes.cbox(W, H, "bdpt")), devices=[0, 0])
    for call in (lambda: c.render_bdpt_moments(W, H, iterations=2),
                 lambda: c.render_vcm_moments(W, H, iterations=2),
                 lambda: c.render_path_moments(W, H, 4)):
        with pytest.raises(native.WrError, match="multi-device") as e:
            call()
        assert e.value.code == native.WR_E_ARG
    film, _ = c.render_bdpt(W, H, iterations=1)  # the plain render still runs there
    assert film.any()
    c.close()


def _pfm(path):
    data = open(path, "rb").read()
    head = data.split(b"\n", 3)
    w, h = map(int, head[1].split())
    return np.frombuffer(head[3], np.float32).reshape(h, w, 3)[::-1]  # PFM rows run bottom-up


def test_cli_stops_at_the_error_target(tmp_path):
    """No threshold fixed in advance: the batches of 4 iterations the mirror
    renders are rendered here through Python, e_k = rel_stderr after k
    iterations, and the target is the geometric mean of e_8 and e_12 -- wr_tot
    must stop at 12 of 24 and scale its image by 1/12.  Target 0 is off."""
    W, H, seed, every, total = 32, 24, 31, 4, 24
    scene = _scenes.cbox(W, H, "bdpt")
    c = native.Context(native.Scene(scene), 0)
    film, sq = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
    e, films = {}, {}
    for k in range(0, total, every):
        c.render_bdpt_moments(W, H, iterations=every, seed=seed, iter_begin=k, film=film, film_sq=sq)
        e[k + every] = native.film_error(film, sq, k + every).rel_stderr
        films[k + every] = film.copy()
    c.close()
    print("rel_stderr by iterations:", e)
    assert e[4] > e[8] > e[12] > 0, e
    target = float(np.sqrt(e[8] * e[12]))
    para = tmp_path / "p.para"
    para.write_text(f"7\n1\n8\n4\n{W}\n{H}\n5\n400\n")
    exe = os.path.join(native.PKG_DIR, "wr_tot")
    base = [exe, scene, None, "-bpt", "--params", str(para), "--iterations", str(total), "--seed", str(seed)]

    def run(out, *more):
        r = subprocess.run([*base[:2], str(tmp_path / out), *base[3:], *more], capture_output=True, text=True,
                           cwd=tmp_path, timeout=120)
        assert r.returncode == 0, r.stderr
        return r.stdout

    out = run("stop.pfm", "--target-error", repr(target), "--error-every", str(every), "--error-out",
              str(tmp_path / "se.pfm"))
    line = [ln for ln in out.splitlines() if ln.startswith("error ")]
    assert len(line) == 1 and line[0].endswith(" after 12 iterations"), out
    shown = float(line[0].split()[1])
    assert shown == pytest.approx(e[12], rel=1e-4)
    img = _pfm(tmp_path / "stop.pfm")  # outputImage: the film times the float 1 / iterationsDone
    assert_film_parity(img, films[12] * (np.float32(1) / np.float32(12)), case="moments_cli_stop12")
    se = _pfm(tmp_path / "se.pfm").astype(np.float64)  # --error-out: rel_stderr is sum(se) / sum(mean)
    assert se.shape == (H, W, 3) and se.sum() / img.astype(np.float64).sum() == pytest.approx(shown, rel=1e-4)
    out = run("all.pfm", "--target-error", "0", "--error-every", str(every))
    assert not [ln for ln in out.splitlines() if ln.startswith("error ")], out
    assert_film_parity(_pfm(tmp_path / "all.pfm"), films[24] * (np.float32(1) / np.float32(24)),
                       case="moments_cli_all24")
