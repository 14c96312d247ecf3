"""The photon-mapping integrator (PhotonIntegrator, surfaceIntegrator/photonMap.cpp)
written as a script: the three definitions of DESIGN.md 15 -- photon pass,
estimate, camera pass -- in numpy float32 over the oracle's primitives
(_script_pt.OracleBackend: Scene.trace and the cr_kat_* hooks), the neighbours
by brute force (_points_ref.knn).  It is what csrc/wr_photon.h is tested
against; neither is written from the other.

All arithmetic between the calls is float32, one operation per statement part,
in the order the definitions state.
"""
import ctypes as C

import numpy as np

import _points_ref
import _script_photons

F = np.float32
EPS, ONE, PI = F(1e-3), F(1.0), F(np.pi)
NONE, CAUSTIC, INDIRECT = 0, 1, 2
PHOTON_SUBPATH = 3


def gt(x):  # cmp(x) > 0
    return x > EPS


def lt(x):  # cmp(x) < 0
    return x < -EPS


def black(c):
    return ~(gt(c[:, 0]) | lt(c[:, 0]) | gt(c[:, 1]) | lt(c[:, 1]) | gt(c[:, 2]) | lt(c[:, 2]))


def dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


class Backend(_script_photons.OraclePhotons):
    """OraclePhotons with the counter stream named per call: (seed, iteration, subpath, path)."""

    def stream(self, iteration, subpath, path, ctr, draws):
        L = self.sc.L
        out = np.zeros((len(path), draws), F)
        for i, (p, c) in enumerate(zip(np.asarray(path).tolist(), np.asarray(ctr).tolist())):
            key = L.cr_stream_key(self.seed, iteration, subpath, p)
            for j in range(draws):
                out[i, j] = F(L.cr_stream_u32(key, c + j) & 0xffffff) / F(16777216.0)
        return out, ctr + np.int32(draws)

    def _prims(self):
        """The scene's primitives from the oracle's dump: type (0 triangle, 1
        sphere), p0 / p1 / p2 (a sphere: centre in p0, radius in p1[0])."""
        if not hasattr(self, "_prim_cache"):
            import os
            import tempfile
            with tempfile.TemporaryDirectory() as d:
                text = self.sc.dump(os.path.join(d, "scene.txt"))
            kind, pts = [], []
            for line in text.splitlines():
                tok = line.split()
                if tok and tok[0] in ("tri", "sph"):
                    v = [float.fromhex(t) for t in tok[2:]]
                    kind.append(0 if tok[0] == "tri" else 1)
                    pts.append(v if tok[0] == "tri" else v + [0.0] * 5)
            self._prim_cache = (np.array(kind, np.int32), np.array(pts, F).reshape(-1, 3, 3))
        return self._prim_cache

    def trace(self, o, d):
        """Scene::intersect for the ray (o, d) with d AS GIVEN.  The oracle's
        trace call normalises every direction (the Ray constructor), but the
        reference traces a bounce ray it has re-aimed without one
        (photonMap.cpp:155, :358: `dir` is what BSDF::sample returned).  So the
        oracle names the primitive, and the hit on it is computed here from the
        direction as given, with the operations of Triangle::hit
        (triangle.cpp:22-87) and Sphere::hit (sphere.cpp:17-78) in float32 and
        in their order.  For a direction that is already normalised this gives
        the oracle's own answer (tests/test_photonmap_host.py checks that
        against the reference's hit points)."""
        h = super().trace(o, d)
        o, d = np.asarray(o, F), np.asarray(d, F)
        rows = np.nonzero(h["prim"] >= 0)[0]
        if rows.shape[0] == 0:
            return h
        kind, pts = self._prims()
        g = h["prim"][rows]
        p0, p1, p2 = pts[g, 0], pts[g, 1], pts[g, 2]
        ro, rd = o[rows], d[rows]
        with np.errstate(all="ignore"):
            # Triangle::hit
            A, B, Cc = p0[:, 0] - p1[:, 0], p0[:, 1] - p1[:, 1], p0[:, 2] - p1[:, 2]
            D, E, Ff = p0[:, 0] - p2[:, 0], p0[:, 1] - p2[:, 1], p0[:, 2] - p2[:, 2]
            G, H, I = rd[:, 0], rd[:, 1], rd[:, 2]
            J, K, L = p0[:, 0] - ro[:, 0], p0[:, 1] - ro[:, 1], p0[:, 2] - ro[:, 2]
            EIHF, GFDI, DHEG = E * I - H * Ff, G * Ff - D * I, D * H - E * G
            denom = A * EIHF + B * GFDI + Cc * DHEG
            AKJB, JCAL, BLKC = A * K - J * B, J * Cc - A * L, B * L - K * Cc
            t_tri = -(Ff * AKJB + E * JCAL + D * BLKC) / denom
            # Sphere::hit (the centre is p0, the radius p1.x)
            oc = p0 - ro
            rad = p1[:, 0]
            l_oc = oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1] + oc[:, 2] * oc[:, 2]
            t_ca = oc[:, 0] * rd[:, 0] + oc[:, 1] * rd[:, 1] + oc[:, 2] * rd[:, 2]
            t_hc = rad * rad - l_oc + t_ca * t_ca
            root = np.sqrt(t_hc)
            t1, t2 = t_ca - root, t_ca + root
            t_sph = np.where(t1 > EPS, t1, t2)  # cmp(t1) <= 0: the far root
            sph = kind[g] == 1
            t = np.where(sph, t_sph, t_tri).astype(F)
            p = (ro + rd * t[:, None]).astype(F)
            v = p - p0
            ln = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
            n = np.where(sph[:, None], v / ln[:, None], h["n"][rows]).astype(F)
        h["t"][rows], h["p"][rows], h["n"][rows] = t, p, n
        return h

    def light_emit(self, lid, dir_r3, pos_r3):
        z = np.zeros((len(lid), 3), F)
        out = self._kat.oracle_light(self.sc, lid, np.concatenate([z, z, dir_r3, pos_r3, z], 1).astype(F))
        out[out == F(-7)] = 0
        return {"le_cos": out[:, 10:13], "pos": out[:, 13:16], "dir": out[:, 16:19], "emission_pdf": out[:, 19],
                "cos_light": out[:, 21]}

    def intensity(self, lid):
        """AreaLight::getIntensity: what illuminance returns where the light faces the point."""
        n = len(lid)
        out = np.zeros((n, 3), F)
        for i, li in enumerate(np.asarray(lid).tolist()):
            out[i] = self._le(li)
        return out

    def _le(self, li):
        if not hasattr(self, "_le_cache"):
            self._le_cache = {}
        if li not in self._le_cache:
            # emit with the direction sample (0, 1, *): local direction (1 * 0, 0, 1) has cosine 1, le_cos = intensity
            em = self.light_emit(np.array([li], np.int32), np.array([[0, 1, 0]], F), np.array([[0.25, 0.25, 0]], F))
            self._le_cache[li] = (em["le_cos"][0] / em["cos_light"][0]).astype(F)
        return self._le_cache[li]


# ------------------------------------------------------------------ photon pass
def shoot(be, shot0, n, max_path_length):
    """Shots shot0 .. shot0 + n - 1 (buildPhotonMap's loop body, :66-160, per
    shot): every photon they would record, as arrays sorted by (shot, bounce):
    shot, nint (nIntersections), cls, pos, wi, alpha."""
    nl = be.nlights
    lpp = ONE / F(float(nl))
    shots = np.arange(shot0, shot0 + n, dtype=np.int64)
    ctr = np.zeros(n, np.int32)
    u, ctr = be.stream(0, PHOTON_SUBPATH, shots, ctr, 7)
    lid = np.minimum((u[:, 0] * F(float(nl))).astype(np.int32), nl - 1)
    em = be.light_emit(lid, u[:, 4:7], u[:, 1:4])  # the position sample is drawn first
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = ((em["le_cos"] * em["cos_light"][:, None]) / (em["emission_pdf"] * lpp)[:, None]).astype(F)
    o, d = np.array(em["pos"], F), np.array(em["dir"], F)  # Ray(lightPos, lightDir): no EPS offset
    d = (d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]).astype(F)  # Ray's constructor
    spec = np.ones(n, bool)
    act = np.nonzero(~black(alpha))[0]
    rec = {k: [] for k in ("shot", "nint", "cls", "pos", "wi", "alpha")}
    for b in range(max_path_length + 1):
        if act.shape[0] == 0:
            break
        nint = b + 1
        h = be.trace(o[act], d[act])
        k = np.nonzero((h["prim"] >= 0) & (h["mat_id"] > 0))[0]
        act, h = act[k], be.take(h, k)
        if act.shape[0] == 0:
            break
        wi = -d[act]
        info = be.bsdf_eval(h, wi, wi)[0]
        k = np.nonzero(info["valid"] != 0)[0]  # a grazing hit ends the path, nothing stored
        act, h, wi = act[k], be.take(h, k), wi[k]
        info = {f: v[k] for f, v in info.items()}
        if act.shape[0] == 0:
            break
        if nint > 1:
            k = np.nonzero(gt(info["prob"][:, 0]) | gt(info["prob"][:, 1]))[0]
            ia = act[k]
            rec["shot"].append(shots[ia])
            rec["nint"].append(np.full(len(ia), nint, np.int32))
            rec["cls"].append(np.where(spec[ia], CAUSTIC, INDIRECT).astype(np.int32))
            rec["pos"].append(h["p"][k].astype(F))
            rec["wi"].append(wi[k].astype(F))
            rec["alpha"].append(alpha[ia].copy())
        if nint > max_path_length:
            break
        u, c = be.stream(0, PHOTON_SUBPATH, shots[act], ctr[act], 3)
        ctr[act] = c
        sm = be.bsdf_sample(h, wi, u)
        bf, pdf, cont = sm["f"], sm["pdf"], info["continue_prob"]
        alive = ~black(bf)
        spec[act] = spec[act] & ~(alive & ((sm["type"] & 12) != 0))
        k = np.nonzero(alive & lt(cont - ONE))[0]
        if k.shape[0] > 0:
            ia = act[k]
            u, c = be.stream(0, PHOTON_SUBPATH, shots[ia], ctr[ia], 1)
            ctr[ia] = c
            alive[k] = ~gt(u[:, 0] - cont[k])
            pdf[k] = pdf[k] * cont[k]
        k = np.nonzero(alive)[0]
        act = act[k]
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha[act] = (alpha[act] * bf[k]) * (sm["cos_wo"][k] / pdf[k])[:, None]
        o[act] = h["p"][k] + sm["wo"][k] * EPS
        d[act] = sm["wo"][k]
    out = {}
    for f, parts in rec.items():
        shape = (0, 3) if f in ("pos", "wi", "alpha") else (0,)
        out[f] = np.concatenate(parts) if parts else np.zeros(shape, F if len(shape) == 2 else np.int64)
    order = np.lexsort((out["nint"], out["shot"]))
    return {f: v[order] for f, v in out.items()}


def select(rec, n_caustic, n_indirect, shots_run, max_shots):
    """The maps of the photons `rec` of shots 0 .. shots_run - 1, by prefix
    counts: the first n of each class, the shot counts of the definition.
    Returns None while neither the maps are full nor max_shots is reached."""
    maps, paths, full = {}, {}, {}
    for name, cls, cap in (("caustic", CAUSTIC, n_caustic), ("indirect", INDIRECT, n_indirect)):
        k = np.nonzero(rec["cls"] == cls)[0][:cap]
        maps[name] = {f: rec[f][k] for f in ("pos", "wi", "alpha", "shot")}
        full[name] = len(k) == cap
        paths[name] = int(rec["shot"][k[-1]]) + 1 if full[name] and cap else 0
    done = full["caustic"] and full["indirect"]
    if not done and shots_run < max_shots:
        return None
    shots = min(shots_run, max(paths["caustic"], paths["indirect"])) if done else shots_run
    for name, cap in (("caustic", n_caustic), ("indirect", n_indirect)):
        if not (full[name] and cap):
            paths[name] = shots
    return {"shots": shots, "caustic": maps["caustic"], "indirect": maps["indirect"],
            "caustic_paths": paths["caustic"], "indirect_paths": paths["indirect"]}


def serial_select(rec, n_caustic, n_indirect, shots_run):
    """buildPhotonMap's loop, literally, over the recorded photons of shots
    0 .. shots_run - 1 (the shots themselves are shoot()'s): one shot after
    another, push_back while a map is not done, stop after the shot at which
    both are."""
    cau, ind = [], []
    cdone, idone = n_caustic == 0, n_indirect == 0
    cpaths = ipaths = 0
    nshot = 0
    j, n = 0, len(rec["shot"])
    while not (cdone and idone) and nshot < shots_run:
        nshot += 1
        while j < n and rec["shot"][j] == nshot - 1:
            if rec["cls"][j] == CAUSTIC:
                if not cdone:
                    cau.append(j)
                    if len(cau) == n_caustic:
                        cdone, cpaths = True, nshot
            elif not idone:
                ind.append(j)
                if len(ind) == n_indirect:
                    idone, ipaths = True, nshot
            j += 1
    return {"shots": nshot, "caustic": np.array(cau, np.int64), "indirect": np.array(ind, np.int64),
            "caustic_paths": cpaths if cdone and n_caustic else nshot,
            "indirect_paths": ipaths if idone and n_indirect else nshot}


def build_maps(be, n_caustic, n_indirect, max_path_length, max_shots, chunk=1024):
    """The photon pass: shots in chunks until select() has its answer."""
    parts, run = [], 0
    while True:
        n = min(chunk, max_shots - run)
        parts.append(shoot(be, run, n, max_path_length))
        run += n
        rec = {f: np.concatenate([p[f] for p in parts]) for f in parts[0]}
        out = select(rec, n_caustic, n_indirect, run, max_shots)
        if out is not None:
            out["records"], out["shots_run"] = rec, run
            return out


# ------------------------------------------------------------------ estimate
def closed_form_msd(kth, max_sqr_dist):
    """max_sqr_dist * 2^j for the smallest j >= 0 with kth < it (strictly)."""
    msd = np.full(kth.shape, F(max_sqr_dist), F)
    with np.errstate(over="ignore"):
        for _ in range(300):
            grow = ~(kth < msd)
            if not grow.any():
                break
            msd = np.where(grow, msd * F(2.0), msd)
    return msd


def doubling_loop(q, pts, k, max_sqr_dist):
    """estimate's search loop (:176-186), literally, for one query over
    _points_ref.knn, stopping like the closed form when the map has fewer than
    k photons: (msd, indices)."""
    k_eff = min(k, len(pts))
    search = F(max_sqr_dist)
    msd, idx = search, np.zeros(0, np.int32)
    while True:
        msd = search
        i, _, c = _points_ref.knn(q[None], pts, k, msd) if len(pts) else (np.zeros((1, k), np.int32), None, [0])
        idx = i[0, :c[0]]
        if c[0] >= k_eff:
            return msd, idx
        search = F(search * F(2.0))


def estimate(be, photons, h, wo, k, max_sqr_dist):
    """estimate() (:164-231) at the hits h (dict of arrays: prim, mat_id, p, n,
    t) seen from wo.  Returns rgb (n, 3), msd (n,), found (n,)."""
    n = len(wo)
    rgb, msd, found = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, np.int32)
    pos = photons["pos"]
    if n == 0 or len(pos) == 0:
        return rgb, msd, found
    q = np.asarray(h["p"], F)
    idx, sqr, cnt = _points_ref.knn(q, pos, k, F(np.inf))
    found = np.where(h["prim"] >= 0, cnt, 0).astype(np.int32)
    rows = np.nonzero(found > 0)[0]
    if rows.shape[0] == 0:
        return rgb, msd, found
    kth = sqr[rows, found[rows] - 1]
    msd[rows] = closed_form_msd(kth, max_sqr_dist)
    hh = be.take(h, rows)
    w = np.asarray(wo, F)[rows]
    info = be.bsdf_eval(hh, w, w)[0]
    ok = (info["valid"] != 0) & (hh["mat_id"] > 0)  # (an emitter's BSDF::f is black)
    rows, hh, w = rows[ok], be.take(hh, np.nonzero(ok)[0]), w[ok]
    if rows.shape[0] == 0:
        return rgb, msd, found
    nn = hh["n"]
    nv = np.where(lt(dot(w, nn))[:, None], -nn, nn)
    scale = ONE / ((PI * msd[rows]) * found[rows].astype(F))
    est = np.zeros((len(rows), 3), F)
    for s in range(k):  # ascending (d2, index), one add per channel per term
        use = np.nonzero(found[rows] > s)[0]
        if use.shape[0] == 0:
            break
        i = idx[rows[use], s]
        wi = photons["wi"][i].copy()
        flip = ~gt(dot(nv[use], wi))
        wi[flip, 2] = wi[flip, 2] * F(-1.0)
        ev = be.bsdf_eval(be.take(hh, use), w[use], wi)[1]
        with np.errstate(divide="ignore", invalid="ignore"):
            term = (ev["f"] * photons["alpha"][i]) * ((ev["cos_wo"] * scale[use]) / ev["dir_pdf"])[:, None]
        term = np.where(black(ev["f"])[:, None], F(0.0), term).astype(F)
        est[use] = est[use] + term
    rgb[rows] = est
    return rgb, msd, found


# ------------------------------------------------------------------ camera pass
def camera_rays(be, width, height, sample, spp):
    """SurfaceIntegrator::render's ray of every pixel for sample `sample` of spp
    (surfaceIntegrator.cpp:26-34): stream (seed, sample, 2, pixel), three draws."""
    P = width * height
    path = np.arange(P, dtype=np.int64)
    u, ctr = be.stream(sample, 2, path, np.zeros(P, np.int32), 3)
    glen = int(np.sqrt(float(spp)))
    row, col = sample // glen, sample % glen
    a = (u[:, 0] + F(float(row))) / F(float(glen))
    b = (u[:, 1] + F(float(col))) / F(float(glen))
    jj, i = (path % width).astype(F), (path // width).astype(F)
    x = ((jj - F(0.5)) + ONE * a) + F(0.0) * b
    y = ((i - F(0.5)) + F(0.0) * a) + ONE * b
    out = np.zeros((P, 10), F)
    w3 = (C.c_float * 3)(0, 0, 0)
    for p in range(P):
        be.sc.L.cr_kat_camera(be.sc.h, float(x[p]), float(y[p]), w3, be._kat._at(out, p))
    return out[:, 0:3].copy(), out[:, 3:6].copy(), ctr


def render(be, maps, width, height, spp, knn, max_sqr_dist, sample_begin=0, sample_count=0):
    """PhotonIntegrator::raytracing as a loop with a throughput over depths
    0..2, summed over the samples.  Returns {direct_target: film} for 0 and 1:
    the two differ in the direct term alone, so one pass gives both."""
    nl = be.nlights
    P = width * height
    films = {0: np.zeros((P, 3), F), 1: np.zeros((P, 3), F)}
    k1 = sample_begin + sample_count if sample_count > 0 else spp
    for sample in range(sample_begin, k1):
        o, d, ctr = camera_rays(be, width, height, sample, spp)
        pw = np.ones((P, 3), F)
        act = np.arange(P)
        for depth in range(3):
            if act.shape[0] == 0:
                break
            h = be.trace(o[act], d[act])
            k = np.nonzero(h["prim"] >= 0)[0]
            act, h = act[k], be.take(h, k)
            k = np.nonzero(h["mat_id"] < 0)[0]  # an emitter: intensity * 100, the path ends
            if k.shape[0] > 0:
                add = pw[act[k]] * (be.intensity(-h["mat_id"][k] - 1) * F(100.0))
                for f in films.values():
                    f[act[k]] = f[act[k]] + add
            k = np.nonzero(h["mat_id"] > 0)[0]
            act, h = act[k], be.take(h, k)
            if act.shape[0] == 0:
                break
            wi = -d[act]
            info = be.bsdf_eval(h, wi, wi)[0]
            k = np.nonzero(info["valid"] != 0)[0]
            act, h, wi = act[k], be.take(h, k), wi[k]
            info = {f: v[k] for f, v in info.items()}
            if act.shape[0] == 0:
                break
            hp = h["p"]
            # ---- direct light (:233-270)
            u, c = be.stream(sample, 2, act, ctr[act], 4)
            ctr[act] = c
            lid = np.minimum((u[:, 0] * F(float(nl))).astype(np.int32), nl - 1)
            il = be.light_illuminate(lid, hp, u[:, 1:4])
            j = np.nonzero(il["direct_pdf"] > F(0.0))[0]  # (a light seen from behind adds nothing)
            if j.shape[0] > 0:
                dtl, dist = il["dir"][j], il["dist"][j]
                illu = il["le"][j] / (il["direct_pdf"][j] / F(float(nl)))[:, None]
                ev = be.bsdf_eval(be.take(h, j), wi[j], dtl)[1]
                with np.errstate(divide="ignore", invalid="ignore"):
                    val = pw[act[j]] * ((illu * ev["f"]) * (ev["cos_wo"] / ev["dir_pdf"])[:, None])
                lit = ~black(ev["f"])
                for target, f in films.items():
                    far = dist if target else h["t"][j]
                    occ = be.occluded(hp[j] + dtl * EPS, dtl, hp[j] + dtl * (far - EPS)[:, None])
                    m = np.nonzero(lit & (occ == 0))[0]
                    f[act[j[m]]] = f[act[j[m]]] + val[m]
            # ---- the two maps, indirect then caustic
            for name in ("indirect", "caustic"):
                est = estimate(be, maps[name], h, wi, knn, max_sqr_dist)[0]
                add = pw[act] * est
                for f in films.values():
                    f[act] = f[act] + add
            if depth == 2:
                break
            # ---- the next direction and Russian roulette (:336-359)
            u, c = be.stream(sample, 2, act, ctr[act], 3)
            ctr[act] = c
            sm = be.bsdf_sample(h, wi, u)
            bf, pdf, cont = sm["f"], sm["pdf"], info["continue_prob"]
            alive = ~black(bf)
            k = np.nonzero(alive & lt(cont - ONE))[0]
            if k.shape[0] > 0:
                ia = act[k]
                u, c = be.stream(sample, 2, ia, ctr[ia], 1)
                ctr[ia] = c
                alive[k] = ~gt(u[:, 0] - cont[k])
                pdf[k] = pdf[k] * cont[k]
            k = np.nonzero(alive)[0]
            act = act[k]
            with np.errstate(divide="ignore", invalid="ignore"):
                pw[act] = (pw[act] * bf[k]) * (sm["cos_wo"][k] / pdf[k])[:, None]
            o[act] = hp[k] + sm["wo"][k] * EPS
            d[act] = sm["wo"][k]
    return {t: f.reshape(height, width, 3) for t, f in films.items()}
