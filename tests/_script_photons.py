"""A one-bounce photon gather written as a script over the library's
device-array calls: an example of density estimation with the point-set index
(include/winmad_rt.h wr_points_*), not an integrator.

  emit N light particles   rng + light_emit            (AreaLight::emit)
  trace them               trace                       (Scene::intersect)
  keep hit position and carried power of those that land on a non-emitter surface
  build an index over the positions; the queries are the first hits of the camera rays
  estimate sum(power_j) / (pi * r2 * N) over the k nearest, r2 = the k-th sqr_dist
  (ClosePhotonQuery's gather radius), summed in the order the search returns

All arithmetic between the calls is float32 on whole arrays, one operation per
statement part, so two backends with the same neighbours in the same order give
the same bits.

backend interface (tests/_script_pt.py's, plus):
  light_emit(id, dir_r3, pos_r3) -> dict le_cos, pos, dir, emission_pdf  [AreaLight::emit]
  camera_rays(width, height)     -> (o, d), one ray per pixel (FILM_PT order)
  arange(n)                      -> int32 0 .. n - 1;  i64(a) -> int64
  knn(points, queries, k, max_sqr_dist) -> (index (nq, k), sqr_dist (nq, k), count (nq,))
"""
import ctypes as C

import numpy as np

import _points_ref
import _script_pt

F = np.float32


def estimate(be, n_particles, width, height, k, max_sqr_dist):
    """(width * height, 3) float32 estimate at the camera rays' first hits and
    the number of stored particles."""
    xp = be.xp
    EPS = be.f32(1e-3)
    nl = be.nlights
    lpp = be.f32(1.0) / be.f32(float(nl))
    path = be.arange(n_particles)
    u, _ = be.rng(path, path * 0, 7)  # particle p draws from stream p: the light, its direction and position samples
    lid = be.i32(u[:, 0] * be.f32(float(nl)))
    lid = xp.minimum(lid, xp.zeros_like(lid) + (nl - 1))
    em = be.light_emit(lid, u[:, 1:4], u[:, 4:7])
    pdf = em["emission_pdf"] * lpp
    ok = pdf > be.f32(0.0)
    one = xp.ones_like(pdf)
    power = em["le_cos"] / xp.where(ok, pdf, one)[:, None]
    d = em["dir"]
    h = be.trace(em["pos"] + d * EPS, d)
    keep = ok & (h["prim"] >= 0) & (h["mat_id"] > 0)  # a surface that is no emitter (and not the black material 0)
    rows = xp.nonzero(keep)[0] if xp is np else xp.nonzero(keep)[:, 0]
    pts, pw = be.copy(h["p"][rows]), power[rows]
    co, cd = be.camera_rays(width, height)
    ch = be.trace(co, cd)
    q, seen = be.copy(ch["p"]), ch["prim"] >= 0
    est = xp.zeros_like(q)
    if pts.shape[0] == 0:
        return est, 0
    idx, sqr, cnt = be.knn(pts, q, k, max_sqr_dist)
    for s in range(k):  # a fixed order: the search's
        use = cnt > s
        i = xp.where(use, idx[:, s], xp.zeros_like(idx[:, s]))
        est = est + xp.where(use[:, None], pw[be.i64(i)], xp.zeros_like(est))
    last = xp.where(cnt > 0, cnt - 1, xp.zeros_like(cnt))
    r2 = sqr[be.i64(be.arange(q.shape[0])), be.i64(last)]
    good = seen & (cnt > 0) & (r2 > be.f32(0.0))
    norm = (be.f32(np.pi) * xp.where(good, r2, xp.ones_like(r2))) * be.f32(float(n_particles))
    est = xp.where(good[:, None], est / norm[:, None], xp.zeros_like(est))
    return est, int(pts.shape[0])


# ------------------------------------------------------------------ the oracle on the CPU
class OraclePhotons(_script_pt.OracleBackend):
    """numpy over the oracle's primitives, the neighbours by brute force (tests/_points_ref.py)."""

    def __init__(self, scene, seed):
        super().__init__(scene, seed, 0)

    @staticmethod
    def i64(a):
        return a.astype(np.int64)

    @staticmethod
    def arange(n):
        return np.arange(n, dtype=np.int32)

    def light_emit(self, lid, dir_r3, pos_r3):
        z = np.zeros((len(lid), 3), F)
        out = self._kat.oracle_light(self.sc, lid, np.concatenate([z, z, dir_r3, pos_r3, z], 1).astype(F))
        out[out == F(-7)] = 0
        return {"le_cos": out[:, 10:13], "pos": out[:, 13:16], "dir": out[:, 16:19], "emission_pdf": out[:, 19]}

    def camera_rays(self, width, height):
        out = np.zeros((width * height, 10), F)
        w = (C.c_float * 3)(0, 0, 0)
        for i in range(height):
            for jj in range(width):
                self.sc.L.cr_kat_camera(self.sc.h, float(jj), float(i), w, self._kat._at(out, i * width + jj))
        return out[:, 0:3].copy(), out[:, 3:6].copy()

    @staticmethod
    def knn(points, queries, k, max_sqr_dist):
        return _points_ref.knn(queries, points, k, max_sqr_dist)


# ------------------------------------------------------------------ the library on the GPU
class DevicePhotons(_script_pt.DeviceBackend):
    """torch over the device-array calls; neighbours: "index" (PointsIndex.knn_t)
    or "brute" (a top-k over all pairs in torch, the same float32 expression)."""

    def __init__(self, ctx, seed, neighbours="index", cell=None):
        super().__init__(ctx, seed, 0)
        self.neighbours, self.cell = neighbours, cell

    def i64(self, a):
        return a.to(self.xp.int64)

    def arange(self, n):
        return self.xp.arange(n, dtype=self.xp.int32, device=self.dev)

    def light_emit(self, lid, dir_r3, pos_r3):
        f = self.native.light_fields(self.ctx.light_emit_t(lid.contiguous(), dir_r3.contiguous(), pos_r3.contiguous()))
        return {"le_cos": f["le_cos"], "pos": f["pos"], "dir": f["dir"], "emission_pdf": f["emission_pdf"]}

    def camera_rays(self, width, height):
        rays = self.ctx.camera_rays_t(width, height)
        return rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous()

    def knn(self, points, queries, k, max_sqr_dist):
        t = self.xp
        if self.neighbours == "index":
            cell = self.cell if self.cell is not None else float(np.sqrt(max_sqr_dist)) / 2
            with self.ctx.points_index_t(points.contiguous(), cell) as idx:
                return idx.knn_t(queries.contiguous(), k, max_sqr_dist)
        dx = queries[:, None, 0] - points[None, :, 0]
        dy = queries[:, None, 1] - points[None, :, 1]
        dz = queries[:, None, 2] - points[None, :, 2]
        d2 = dx * dx + dy * dy + dz * dz
        inf = t.full_like(d2, float("inf"))
        d2 = t.where(d2 < max_sqr_dist, d2, inf)
        if d2.shape[1] < k:
            d2 = t.cat([d2, inf[:, :1].expand(-1, k - d2.shape[1])], 1)
        val, order = t.sort(d2, dim=1, stable=True)  # equal d2: the lower index first
        val, order = val[:, :k], order[:, :k]
        have = val < float("inf")
        return (t.where(have, order, t.full_like(order, -1)).to(t.int32), t.where(have, val, t.zeros_like(val)),
                have.sum(1).to(t.int32))
