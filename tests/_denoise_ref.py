"""The film denoiser's definition (include/winmad_rt.h
wr_film_denoise) restated in numpy float32, and the synthetic films the host
and GPU denoise tests share.  Test infrastructure only.

The restatement evaluates whole images per tap; a tap outside the image adds
+0 to every sum, which leaves a float sum as it is, so it equals the library's
per-pixel loop (which skips those taps) bit for bit.
"""
import numpy as np

F = np.float32
DEFAULTS = dict(levels=5, normal_power=7, sigma_l=4.0, sigma_p=0.05, sigma_a=0.1)
B3 = (0.375, 0.25, 0.0625)


def _shift(a, oy, ox):
    """out[y, x] = a[y + oy, x + ox] where that lies in the image (else 0), and the mask of those."""
    H, W = a.shape[:2]
    out = np.zeros_like(a)
    m = np.zeros((H, W), bool)
    y0, y1 = max(0, -oy), min(H, H - oy)
    x0, x1 = max(0, -ox), min(W, W - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        m[y0:y1, x0:x1] = True
    return out, m


def _falloff(x):
    m = F(1.0) - F(0.25) * x
    m = np.where(m > 0, m, F(0.0))
    return (m * m) * (m * m)


def _lum(c):
    return F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1] + F(0.0722) * c[..., 2]


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def np_input(S, Q, n):
    s, q, n = S.astype(np.float64), Q.astype(np.float64), float(n)
    var = (q - s * s / n) / (n - 1.0)
    var = np.where(var > 0.0, var, 0.0) / n
    mu, se = s / n, np.sqrt(var)
    v = 0.2126 * (se[..., 0] * se[..., 0]) + 0.7152 * (se[..., 1] * se[..., 1]) + 0.0722 * (se[..., 2] * se[..., 2])
    return mu.astype(F), v.astype(F)


def _normal_weight(N, p_surf, Nq, power):
    """w_n and the mask of the pairs that are both surfaces."""
    q_surf = (Nq != 0).any(axis=2)
    both = p_surf & q_surf
    d = _dot(N, Nq)
    d = np.where(d > 0, d, F(0.0))
    for _i in range(power):
        d = d * d
    return np.where(both, d, np.where(p_surf == q_surf, F(1.0), F(0.0))), both


def np_level(c, v, N, P, A, s, prm):
    H, W = v.shape
    p_surf = (N != 0).any(axis=2) if N is not None else None
    pv, pk = np.zeros((H, W), F), np.zeros((H, W), F)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            vq, m = _shift(v, dy, dx)
            if N is not None and (dy != 0 or dx != 0):  # a tap whose w_n is exactly 0 is skipped
                m = m & (_normal_weight(N, p_surf, _shift(N, dy, dx)[0], prm["normal_power"])[0] != 0)
            pw = F((0.5 if dy == 0 else 0.25) * (0.5 if dx == 0 else 0.25))
            pv = pv + np.where(m, pw * vq, F(0.0))
            pk = pk + np.where(m, pw, F(0.0))
    vt = pv / pk
    l_den = F(prm["sigma_l"]) * np.sqrt(vt) + F(1e-12)
    lum_p = _lum(c)
    sw = np.zeros((H, W), F)
    sc = np.zeros((H, W, 3), F)
    sv = np.zeros((H, W), F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            cq, m = _shift(c, s * dy, s * dx)
            vq, _ = _shift(v, s * dy, s * dx)
            hk = F(F(B3[abs(dy)]) * F(B3[abs(dx)]))
            if dy == 0 and dx == 0:
                w = np.full((H, W), hk, F)
            else:
                w = hk * _falloff(np.abs(lum_p - _lum(cq)) / l_den)
                if N is not None:
                    Nq, _ = _shift(N, s * dy, s * dx)
                    wn, both = _normal_weight(N, p_surf, Nq, prm["normal_power"])
                    w = w * wn
                    if P is not None:
                        Pq, _ = _shift(P, s * dy, s * dx)
                        D = Pq - P
                        wp = _falloff(np.abs(_dot(N, D)) / (F(prm["sigma_p"]) * np.sqrt(_dot(D, D)) + F(1e-12)))
                        w = w * np.where(both, wp, F(1.0))
                if A is not None:
                    Aq, _ = _shift(A, s * dy, s * dx)
                    dA = np.abs(Aq - A)
                    w = w * _falloff((dA[..., 0] + dA[..., 1] + dA[..., 2]) / F(prm["sigma_a"]))
                w = np.where(m, w, F(0.0)).astype(F)
            sw = sw + w
            sc = sc + w[..., None] * cq
            sv = sv + (w * w) * vq
    return sc / sw[..., None], sv / (sw * sw)


def np_denoise(S, Q, n, normal=None, position=None, albedo=None, **params):
    prm = dict(DEFAULTS, **params)
    with np.errstate(all="ignore"):
        c, v = np_input(S, Q, n)
        for t in range(prm["levels"]):
            c, v = np_level(c, v, normal, position, albedo, 1 << t, prm)
        out = c * F(n)
    assert out.dtype == F
    return out


def regions(W):
    """Columns of region A, of the no-surface band and of region B."""
    a_end = max(1, (2 * W) // 5)
    band_end = a_end + max(1, W // 12) if W >= 3 else a_end
    return slice(0, a_end), slice(a_end, min(W, band_end)), slice(min(W, band_end), W)


def fold(passes):
    """The float32 sums a moments render accumulates pass by pass."""
    S = np.zeros(passes.shape[1:], F)
    Q = np.zeros(passes.shape[1:], F)
    for p in passes:
        S += p
        Q += p * p
    return S, Q


def synthetic_passes(W, H, n=6, seed=12):
    """Pass films of a W x H image: region A (normal +z, a plane z = 0), a band
    of no-surface pixels, region B (normal +x, a plane x = 0); different
    albedos; pixel (1, 1) is 0.75 in every pass, pixel (2, 3) is hot in one."""
    rng = np.random.default_rng(seed)
    A_, band, B_ = regions(W)
    passes = (rng.random((n, H, W, 3), dtype=F) * F(0.5) + F(0.25)).astype(F)
    passes[:, :, B_, :] += F(0.5)
    if H > 1 and W > 1:
        passes[:, 1, 1, :] = 0.75
    if H > 2 and W > 3:
        passes[:, 2, 3, :] = 0.1
        passes[n // 2, 2, 3, :] = 1000.0
    return passes


def synthetic_guides(W, H):
    A_, band, B_ = regions(W)
    yy, xx = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    N = np.zeros((H, W, 3), F)
    P = np.zeros((H, W, 3), F)
    Al = np.zeros((H, W, 3), F)
    N[:, A_] = (0, 0, 1)
    N[:, B_] = (1, 0, 0)
    P[..., 0], P[..., 1] = xx * F(0.1), yy * F(0.1)
    P[:, B_, 2] = P[:, B_, 0]
    P[:, B_, 0] = 0
    P[:, band] = 0
    Al[:, A_] = (0.7, 0.2, 0.2)
    Al[:, B_] = (0.2, 0.7, 0.25)
    if H > 4 and W > 2:  # a second material inside region A
        Al[H // 2:, 0:1] = (0.7, 0.2, 0.35)
    return N, P, Al


def synthetic(W, H, n=6, seed=12):
    """(S, Q, n, normal, position, albedo) of the synthetic image."""
    S, Q = fold(synthetic_passes(W, H, n, seed))
    return (S, Q, n) + synthetic_guides(W, H)
