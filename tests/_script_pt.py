"""A path tracer written as a script over the library's device-array calls:
PathIntegrator::raytracing (pathIntegrator.cpp:29-148; csrc/wr_pt.h pt_shade_body /
pt_resolve_body restate it as kernels), once, over a small backend interface.

It is the worked example of "your own integrator"  and the
proof that the shading calls are complete: with them, and the ray calls, a
script reproduces the library's own path tracer ray for ray.

All arithmetic between the calls is float32, one operation per statement part,
in the order pt_shade_body uses, on whole arrays of the rays still alive.

backend interface (arrays are the backend's: numpy on the CPU, torch on the GPU):
  xp                          the array module (numpy / torch)
  nlights
  f32(x)                      a float32 scalar of the backend
  i32(a)                      float array -> int32 (truncation, as a C cast)
  copy(a)                     a new array with a's values
  trace(o, d)                 -> hit dict: prim, mat_id (int32), t, p, n (+ the backend's own record)
  occluded(o, d, target)      -> (k,) 0 / 1
  bsdf_eval(hit, wi, wo)      -> (info dict, eval dict)     [BSDF::init + BSDF::f]
  bsdf_sample(hit, wi, r3)    -> sample dict                [BSDF::sample]
  light_illuminate(id, p, r3) -> dict                       [AreaLight::illuminance]
  light_radiance(hit, d)      -> dict                       [AreaLight::getRadiance]
  rng(path, ctr, draws)       -> ((k, draws) floats, advanced ctr): stream (seed, sample, 2, path)
  take(hit, idx)              the rows idx of every array of a hit dict
The dict keys are the fields of the records in include/winmad_rt.h.
"""
import ctypes as C

import numpy as np

F = np.float32


def cbox_rays(n=2048, seed=9):
    """The ray recipe of test_path_radiance_per_ray_matches_oracle for the
    Cornell box: n / 2 camera rays towards random points of the back wall, n / 2
    random rays inside the box.  Returns (o, d) float32 (n, 3)."""
    rng = np.random.default_rng(seed)
    cam = np.array([-0.0439815, -4.12529, 0.222539], F)
    tgt = np.stack([rng.uniform(-1.2, 1.2, n), np.full(n, 1.3), rng.uniform(-1.2, 1.2, n)], 1).astype(F)

    def normalize_f32(v):
        v = v.astype(F)
        l = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        return (v / l[:, None]).astype(F)

    d = normalize_f32(tgt - cam)
    o = np.repeat(cam[None], n, 0)
    o[n // 2:] = rng.uniform(-1.0, 1.0, (n - n // 2, 3)).astype(F)
    d[n // 2:] = normalize_f32(rng.normal(size=(n - n // 2, 3)))
    return o, d


def radiance(be, o, d, max_depth):
    """PathIntegrator::raytracing(ray, 0) for rays (o, d) as given: (n, 3) radiance."""
    xp = be.xp
    EPS, ONE = be.f32(1e-3), be.f32(1.0)
    nl = be.nlights
    lpp = ONE / be.f32(float(nl))

    def gt(x):  # cmpf(x) > 0
        return x > EPS

    def lt(x):  # cmpf(x) < 0
        return x < -EPS

    def zero(x):  # cmpf(x) == 0
        return ~(gt(x) | lt(x))

    def black(c):
        return zero(c[:, 0]) & zero(c[:, 1]) & zero(c[:, 2])

    def rows(mask):
        return xp.nonzero(mask)[0] if xp is np else xp.nonzero(mask)[:, 0]

    o, d = be.copy(o), be.copy(d)  # updated in place from bounce to bounce
    res = xp.zeros_like(o)
    pw = xp.ones_like(o)
    last_pdf = xp.ones_like(o[:, 0])
    last_spec = last_pdf > be.f32(0.0)
    ctr = be.i32(xp.zeros_like(last_pdf))
    act = rows(last_spec)
    plen = 1
    while act.shape[0] > 0:
        h = be.trace(o[act], d[act])
        k = rows(h["prim"] >= 0)  # a miss ends the path (:46)
        act, h = act[k], be.take(h, k)
        if act.shape[0] == 0:
            break
        dd = d[act]
        wi = -dd
        info = be.bsdf_eval(h, wi, wi)[0]  # BSDF bsdf(-r.dir, inter, scene) (:50)
        k = rows(info["valid"] != 0)
        act, h, dd, wi = act[k], be.take(h, k), dd[k], wi[k]
        info = {f: v[k] for f, v in info.items()}
        # ---- emitters (:53-73): add Le with the MIS weight of the BSDF-sampled hit, end
        em = h["mat_id"] < 0
        k = rows(em)
        if k.shape[0] > 0:
            ia = act[k]
            rad = be.light_radiance(be.take(h, k), dd[k])
            c = rad["le"]
            mw = xp.ones_like(c[:, 0])
            if plen > 1:
                t = h["t"][k]
                dp = rad["direct_pdf_a"] * (t * t) / xp.abs(info["cos_wi"][k])  # pdfAtoW
                lp = last_pdf[ia]
                mw = xp.where(last_spec[ia], mw, lp / (lp + dp * lpp))
            add = (pw[ia] * c) * mw[:, None]
            j = rows(~black(c))
            res[ia[j]] = res[ia[j]] + add[j]
        # ---- surfaces that go on (:75-79)
        if plen > max_depth:
            break
        k = rows(~em & ~zero(info["continue_prob"]))
        act, h, dd, wi = act[k], be.take(h, k), dd[k], wi[k]
        info = {f: v[k] for f, v in info.items()}
        if act.shape[0] == 0:
            break
        cont, hp = info["continue_prob"], h["p"]
        # ---- next event estimation (:81-118)
        k = rows(info["is_delta"] == 0)
        if k.shape[0] > 0:
            ia = act[k]
            u, c = be.rng(ia, ctr[ia], 4)  # the light, then a point on it
            ctr[ia] = c
            lid = be.i32(u[:, 0] * be.f32(float(nl)))
            lid = xp.minimum(lid, xp.zeros_like(lid) + (nl - 1))
            il = be.light_illuminate(lid, hp[k], u[:, 1:4])
            j = rows(~black(il["le"]))
            k, ia = k[j], ia[j]
            il = {f: v[j] for f, v in il.items()}
            dtl, dist, hpl = il["dir"], il["dist"], hp[k]
            occ = be.occluded(hpl + dtl * EPS, dtl, hpl + dtl * (dist - EPS)[:, None])
            j = rows(occ == 0)
            k, ia = k[j], ia[j]
            il = {f: v[j] for f, v in il.items()}
            if k.shape[0] > 0:
                ev = be.bsdf_eval(be.take(h, k), wi[k], il["dir"])[1]
                bf, cw = ev["f"], ev["cos_wo"]
                bp = ev["dir_pdf"] * cont[k]
                dpdf = il["direct_pdf"]
                w = (dpdf * lpp) / ((dpdf * lpp) + bp)
                contrib = (il["le"] * bf) * (w * cw / (lpp * dpdf))[:, None]
                add = contrib * pw[ia]
                j = rows(~black(bf))
                res[ia[j]] = res[ia[j]] + add[j]
        # ---- the next direction and Russian roulette (:120-146)
        u, c = be.rng(act, ctr[act], 3)
        ctr[act] = c
        sm = be.bsdf_sample(h, wi, u)
        bf, pdf = sm["f"], sm["pdf"]
        lspec = (sm["type"] & 3) != 0
        lpdf = pdf * cont
        alive = ~black(bf)
        k = rows(alive & lt(cont - ONE))
        if k.shape[0] > 0:
            ia = act[k]
            u, c = be.rng(ia, ctr[ia], 1)
            ctr[ia] = c
            alive[k] = ~gt(u[:, 0] - cont[k])
            pdf[k] = pdf[k] * cont[k]
        k = rows(alive)
        act = act[k]
        pw[act] = (pw[act] * bf[k]) * (sm["cos_wo"][k] / pdf[k])[:, None]
        o[act] = hp[k] + sm["wo"][k] * EPS
        d[act] = sm["wo"][k]  # r.dir stays un-normalised (:144-145)
        last_spec[act] = lspec[k]
        last_pdf[act] = lpdf[k]
        plen += 1
    return res


# ------------------------------------------------------------------ the oracle on the CPU
class OracleBackend:
    """numpy over the oracle's primitives: Scene.trace and the known-answer
    hooks cr_kat_bsdf / cr_kat_light / cr_stream_key / cr_stream_u32 (tests/_kat.py).
    What a hook leaves unwritten (its -7 mark) reads 0, as in the device records."""
    xp = np

    def __init__(self, scene, seed, sample):
        import _kat
        self._kat = _kat
        self.sc = scene
        self.seed, self.sample = seed, sample
        self.nlights = scene.L.cr_scene_nlights(scene.h)

    @staticmethod
    def f32(x):
        return F(x)

    @staticmethod
    def i32(a):
        return a.astype(np.int32)

    @staticmethod
    def copy(a):
        return np.array(a, F)

    @staticmethod
    def take(h, idx):
        return {f: v[idx] for f, v in h.items()}

    def trace(self, o, d):
        oi, of, _, _ = self.sc.trace(np.concatenate([o, d, np.zeros_like(o)], 1))
        return {"prim": oi[:, 0].copy(), "mat_id": oi[:, 2].copy(), "t": of[:, 0].copy(), "p": of[:, 1:4].copy(),
                "n": of[:, 4:7].copy()}

    def occluded(self, o, d, target):
        return self.sc.trace(np.concatenate([o, d, target], 1))[2]

    def _bsdf(self, h, wi, wo, r3):
        n = len(wi)
        inp = np.concatenate([h["n"], wi, wo, r3], 1).astype(F)
        out = np.full((n, 26), F(-7))
        valid = np.zeros(n, np.int32)
        fn, sh = self.sc.L.cr_kat_bsdf, self.sc.h
        FP = C.POINTER(C.c_float)
        for i in range(n):
            p = inp.ctypes.data + i * inp.strides[0]
            valid[i] = fn(sh, int(h["mat_id"][i]), C.cast(p, FP), C.cast(p + 12, FP), C.cast(p + 24, FP),
                          C.cast(p + 36, FP), C.cast(out.ctypes.data + i * out.strides[0], FP))
        out[valid == 0] = 0
        out[out == F(-7)] = 0
        return out, valid

    def bsdf_eval(self, h, wi, wo):
        out, valid = self._bsdf(h, wi, wo, np.zeros_like(wi))
        info = {"valid": valid, "is_delta": out[:, 0].astype(np.int32), "cos_wi": out[:, 1], "continue_prob": out[:, 2],
                "fresnel": out[:, 3], "prob": out[:, 4:8]}
        ev = {"f": out[:, 8:11], "cos_wo": out[:, 11], "dir_pdf": out[:, 12], "rev_pdf": out[:, 13], "pdf": out[:, 14],
              "pdf_rev": out[:, 15]}
        return info, ev

    def bsdf_sample(self, h, wi, r3):
        out, _ = self._bsdf(h, wi, wi, r3)
        return {"type": out[:, 16].astype(np.int32), "f": out[:, 17:20], "wo": out[:, 20:23], "pdf": out[:, 23].copy(),
                "cos_wo": out[:, 24]}

    def _light(self, li, pos, r3, rd):
        n = len(li)
        z = np.zeros((n, 3), F)
        inp = np.concatenate([z if pos is None else pos, z if r3 is None else r3, z, z, z if rd is None else rd], 1)
        out = self._kat.oracle_light(self.sc, li, inp.astype(F))
        out[out == F(-7)] = 0
        return out

    def light_illuminate(self, lid, pos, r3):
        out = self._light(lid, pos, r3, None)
        return {"le": out[:, 0:3], "dir": out[:, 3:6], "dist": out[:, 6], "direct_pdf": out[:, 7],
                "emission_pdf": out[:, 8], "cos_light": out[:, 9]}

    def light_radiance(self, h, d):
        out = self._light(-h["mat_id"] - 1, None, None, d)
        return {"le": out[:, 22:25], "direct_pdf_a": out[:, 25], "emission_pdf": out[:, 26]}

    def rng(self, path, ctr, draws):
        L = self.sc.L
        out = np.zeros((len(path), draws), F)
        for i, (p, c) in enumerate(zip(path.tolist(), ctr.tolist())):
            key = L.cr_stream_key(self.seed, self.sample, 2, p)
            for j in range(draws):
                out[i, j] = F(L.cr_stream_u32(key, c + j) & 0xffffff) / F(16777216.0)
        return out, ctr + np.int32(draws)


# ------------------------------------------------------------------ the library on the GPU
class DeviceBackend:
    """torch over the device-array calls of winmad_rt.native.Context: nothing
    leaves the GPU between the first trace and the returned radiance."""

    def __init__(self, ctx, seed, sample):
        import torch
        from winmad_rt import native
        self.xp, self.native, self.ctx = torch, native, ctx
        self.seed, self.sample = seed, sample
        self.nlights = ctx.scene.info()["nlights"]
        self.dev = f"cuda:{ctx.devices()[0]}"

    def f32(self, x):
        return self.xp.tensor(float(x), dtype=self.xp.float32, device=self.dev)

    def i32(self, a):
        return a.to(self.xp.int32)

    @staticmethod
    def copy(a):
        return a.clone()

    @staticmethod
    def take(h, idx):
        return {f: v[idx] for f, v in h.items()}

    def _rays(self, o, d):
        t = self.xp
        lim = t.zeros((o.shape[0], 2), dtype=t.float32, device=self.dev)
        lim[:, 1] = 1e7
        return t.cat([o, d, lim], 1)

    def trace(self, o, d):
        rec = self.ctx.trace_closest_t(self._rays(o, d))
        f = self.native.hit_fields(rec)
        return {"rec": rec, "prim": f["prim"], "mat_id": f["mat_id"], "t": f["t"], "p": f["p"], "n": f["n"]}

    def occluded(self, o, d, target):
        return self.ctx.occluded_t(self._rays(o, d), target.contiguous())

    def bsdf_eval(self, h, wi, wo):
        info, ev = self.ctx.bsdf_eval_t(h["rec"].contiguous(), wi.contiguous(), wo.contiguous())
        return self.native.bsdf_info_fields(info), self.native.bsdf_eval_fields(ev)

    def bsdf_sample(self, h, wi, r3):
        _, sm = self.ctx.bsdf_sample_t(h["rec"].contiguous(), wi.contiguous(), r3.contiguous())
        f = self.native.bsdf_sample_fields(sm)
        return {**f, "pdf": f["pdf"].clone()}  # the script scales it in place

    def light_illuminate(self, lid, pos, r3):
        return self.native.light_fields(self.ctx.light_illuminate_t(lid.contiguous(), pos.contiguous(),
                                                                     r3.contiguous()))

    def light_radiance(self, h, d):
        return self.native.light_fields(self.ctx.light_radiance_t(h["rec"].contiguous(), d.contiguous()))

    def rng(self, path, ctr, draws):
        ctr = ctr.contiguous()
        out = self.ctx.rng_uniform_t(int(path.shape[0]), draws, self.seed, self.sample, 2,
                                     path=path.to(self.xp.int32), ctr=ctr)
        return out, ctr
