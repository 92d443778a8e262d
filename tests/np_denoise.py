"""float32 numpy restatement of the diffuse denoiser (csrc/denoise.hip: k_dn_temporal, k_dn_variance, k_dn_atrous; include/vkrt.h
vkrt_denoise_diffuse) in the kernels' operation order.  Every array is float32 and every binary operation rounds like the
kernels' (built with -ffp-contract=off: no fused multiply-adds; / and sqrt correctly rounded); expf may differ from np.exp in the
last bit, which is what the GPU parity test's tolerance is for.

Inputs are the planes Renderer.gbuffer_raycast(view_matrix=...) + Renderer.hybrid_trace fill, as numpy arrays:
color / position / normal [H,W,4], roughMetal [H,W,2], nrdViewZ [H,W], nrdRadianceHitDist [H,W,4]."""
import numpy as np

F = np.float32
INVALID = np.uint32(0x80008000)  # oct word of a pixel without geometry
SIGMA_Z = F(1.0)
SIGMA_L = F(4.0)
B3 = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))


def _sign(v):
    return np.where(v >= 0, F(1), F(-1)).astype(F)


def oct_encode(nx, ny, nz):
    s = (np.abs(nx) + np.abs(ny)) + np.abs(nz)
    s = np.where(s > 0, s, F(1)).astype(F)
    vx, vy = nx / s, ny / s
    neg = ~(nz >= 0)
    wx = (F(1) - np.abs(vy)) * _sign(vx)
    wy = (F(1) - np.abs(vx)) * _sign(vy)
    vx, vy = np.where(neg, wx, vx).astype(F), np.where(neg, wy, vy).astype(F)
    qx = np.rint(np.clip(vx, F(-1), F(1)) * F(32767)).astype(np.int32)
    qy = np.rint(np.clip(vy, F(-1), F(1)) * F(32767)).astype(np.int32)
    return ((qx & 0xFFFF).astype(np.uint32) | ((qy & 0xFFFF).astype(np.uint32) << np.uint32(16))).astype(np.uint32)


def oct_decode(bits):
    bits = np.asarray(bits, np.uint32)
    x = (bits & np.uint32(0xFFFF)).astype(np.uint16).view(np.int16).astype(F) * F(1.0 / 32767.0)
    y = (bits >> np.uint32(16)).astype(np.uint16).view(np.int16).astype(F) * F(1.0 / 32767.0)
    z = (F(1) - np.abs(x)) - np.abs(y)
    t = np.maximum(-z, F(0))
    x = x + np.where(x >= 0, -t, t)
    y = y + np.where(y >= 0, -t, t)
    r = F(1) / np.sqrt((x * x + y * y) + z * z)
    return x * r, y * r, z * r


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def lum(r, g, b):
    return (F(0.25) * r + F(0.5) * g) + F(0.25) * b


def pow128(d):
    d = np.maximum(d, F(0))
    for _ in range(7):
        d = d * d
    return d


def e_z(zp, gx, gy, zq, ox, oy):
    """exponent of the depth weight w_z = exp(-e_z)"""
    return np.abs(zq - zp) / (SIGMA_Z * np.abs(gx * F(ox) + gy * F(oy)) + F(1e-3) * np.abs(zp))


def geom_valid(pos, nrm):
    return ~(np.all(pos[..., :3] == 0, axis=-1) & np.all(nrm[..., :3] == 0, axis=-1))


def albedo_factor(color, pos, nrm, rm):
    """curWeight of k_hybrid: albedo (floored at 1e-3 per channel) on the diffuse branch, 1 on the specular branch / black albedo"""
    ratio = rm[..., 1] * (F(1) - rm[..., 0])
    a = np.stack([color[..., 3], pos[..., 3], nrm[..., 3]], -1)
    amax = np.maximum(np.maximum(a[..., 0], a[..., 1]), a[..., 2])
    keep = ~(ratio < F(0.8)) | ~(amax >= F(1e-3))
    return np.where(keep[..., None], F(1), np.maximum(a, F(1e-3))).astype(F)


def project(M, X, W, H):
    """continuous pixel (px, py) of world points X [...,3] under column-major viewProj M[16]; ok = in front of the camera"""
    M = np.asarray(M, F).reshape(-1)
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    cx = ((M[0] * x + M[4] * y) + M[8] * z) + M[12]
    cy = ((M[1] * x + M[5] * y) + M[9] * z) + M[13]
    cw = ((M[3] * x + M[7] * y) + M[11] * z) + M[15]
    ok = cw > 0
    cws = np.where(ok, cw, F(1)).astype(F)
    px = ((cx / cws) * F(0.5) + F(0.5)) * F(W) - F(0.5)
    py = ((cy / cws) * F(0.5) + F(0.5)) * F(H) - F(0.5)
    return px, py, ok


def _min_abs(a, b):
    return np.where(np.abs(a) <= np.abs(b), a, b).astype(F)


def _shift(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx] where that lies inside the image, else fill; also returns the inside mask"""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((H, W), bool)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        b[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
        inside[ys:ye, xs:xe] = True
    return b, inside


class NpDenoiser:
    def __init__(self, width, height, sigma_l=SIGMA_L):
        """sigma_l: the luminance edge-stopping constant (the kernels' 4); np.inf switches w_l off (an experiment, not a kernel mode)"""
        self.W, self.H = int(width), int(height)
        self.sigma_l = F(sigma_l)
        self.reset()
        self.hist = np.zeros((self.H, self.W, 3), F)
        self.geom_pos = np.zeros((self.H, self.W, 3), F)
        self.geom_oct = np.full((self.H, self.W), INVALID, np.uint32)
        self.mom = np.zeros((self.H, self.W, 3), F)
        self.prev_vp = np.zeros(16, F)

    def reset(self):
        self.has_history = False

    # ---- k_dn_temporal ------------------------------------------------------------------------------------------------------
    def temporal(self, view_proj, g, max_history):
        W, H = self.W, self.H
        pos, nrm, col, rm = (np.asarray(g[k], F) for k in ("position", "normal", "color", "roughMetal"))
        vz = np.asarray(g["nrdViewZ"], F).reshape(H, W)
        rad = np.asarray(g["nrdRadianceHitDist"], F)
        valid = geom_valid(pos, nrm)
        # viewZ gradient: the smaller of the two one-sided differences (one-sided next to a pixel without geometry)
        zl, vl = _shift(vz, -1, 0, F(0)); zr, vr = _shift(vz, 1, 0, F(0))
        zu, vu = _shift(vz, 0, -1, F(0)); zd, vd = _shift(vz, 0, 1, F(0))
        vl &= _shift(valid, -1, 0, False)[0]; vr &= _shift(valid, 1, 0, False)[0]
        vu &= _shift(valid, 0, -1, False)[0]; vd &= _shift(valid, 0, 1, False)[0]
        zl, zr, zu, zd = (np.where(v, z, F(0)).astype(F) for v, z in ((vl, zl), (vr, zr), (vu, zu), (vd, zd)))
        gx = np.where(vl & vr, _min_abs(zr - vz, vz - zl), np.where(vr, zr - vz, np.where(vl, vz - zl, F(0)))).astype(F)
        gy = np.where(vu & vd, _min_abs(zd - vz, vz - zu), np.where(vd, zd - vz, np.where(vu, vz - zu, F(0)))).astype(F)
        octw = np.where(valid, oct_encode(nrm[..., 0], nrm[..., 1], nrm[..., 2]), INVALID).astype(np.uint32)
        self.rec = (np.where(valid, vz, F(0)).astype(F), np.where(valid, gx, F(0)).astype(F), np.where(valid, gy, F(0)).astype(F), octw)
        # current sample
        f = albedo_factor(col, pos, nrm, rm)
        t = rad[..., 0] - rad[..., 2]
        cr = np.maximum(t + rad[..., 1], F(0)) / f[..., 0]
        cg = np.maximum(rad[..., 0] + rad[..., 2], F(0)) / f[..., 1]
        cb = np.maximum(t - rad[..., 1], F(0)) / f[..., 2]
        Y = lum(cr, cg, cb)
        # history taps
        sw = np.zeros((H, W), F); hr = np.zeros((H, W), F); hg = np.zeros((H, W), F); hb = np.zeros((H, W), F)
        h1 = np.zeros((H, W), F); h2 = np.zeros((H, W), F); max_len = np.zeros((H, W), F)
        if self.has_history:
            X = pos[..., :3]
            pxp, pyp, okp = project(self.prev_vp, X, W, H)
            pxc, pyc, okc = project(view_proj, X, W, H)
            xs = np.arange(W, dtype=F)[None, :].repeat(H, 0)
            ys = np.arange(H, dtype=F)[:, None].repeat(W, 1)
            qx = xs + (pxp - pxc)
            qy = ys + (pyp - pyc)
            inside = okp & okc & valid & (qx > F(-1)) & (qx < F(W)) & (qy > F(-1)) & (qy < F(H))
            qx = np.where(inside, qx, F(0)).astype(F)
            qy = np.where(inside, qy, F(0)).astype(F)
            x0, y0 = np.floor(qx), np.floor(qy)
            fx, fy = qx - x0, qy - y0
            tol = F(0.01) * np.abs(vz)
            N = (nrm[..., 0], nrm[..., 1], nrm[..., 2])
            gdec = oct_decode(self.geom_oct)
            for j in (0, 1):
                for i in (0, 1):
                    w = (fx if i else F(1) - fx) * (fy if j else F(1) - fy)
                    tx = x0.astype(np.int64) + i
                    ty = y0.astype(np.int64) + j
                    ok = inside & (w > 0) & (tx >= 0) & (ty >= 0) & (tx < W) & (ty < H)
                    txc, tyc = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
                    ok &= self.geom_oct[tyc, txc] != INVALID
                    gp = self.geom_pos[tyc, txc]
                    d = (gp[..., 0] - pos[..., 0], gp[..., 1] - pos[..., 1], gp[..., 2] - pos[..., 2])
                    ok &= np.abs(dot3(N, d)) <= tol
                    ok &= dot3(N, tuple(c[tyc, txc] for c in gdec)) >= F(0.9)
                    m = self.mom[tyc, txc]
                    h = self.hist[tyc, txc]
                    w = np.where(ok, w, F(0)).astype(F)
                    sw = np.where(ok, sw + w, sw)
                    hr = np.where(ok, hr + w * h[..., 0], hr); hg = np.where(ok, hg + w * h[..., 1], hg); hb = np.where(ok, hb + w * h[..., 2], hb)
                    h1 = np.where(ok, h1 + w * m[..., 0], h1); h2 = np.where(ok, h2 + w * m[..., 1], h2)
                    max_len = np.where(ok, np.maximum(max_len, m[..., 2]), max_len)
        hist = sw > 0
        sws = np.where(hist, sw, F(1)).astype(F)
        length = np.where(hist, np.minimum(max_len, F(max_history - 1)) + F(1), F(1)).astype(F)
        a = F(1) / length
        blend = lambda s, c: np.where(hist, (s / sws) * (F(1) - a) + c * a, c).astype(F)  # noqa: E731
        c = np.stack([blend(hr, cr), blend(hg, cg), blend(hb, cb)], -1)
        m = np.stack([blend(h1, Y), blend(h2, Y * Y), length], -1)
        c = np.where(valid[..., None], c, F(0)).astype(F)
        m = np.where(valid[..., None], m, F(0)).astype(F)
        self.valid, self.factor = valid, f
        self.geom_pos = np.where(valid[..., None], pos[..., :3], F(0)).astype(F)
        self.geom_oct = octw
        self.mom = m
        return c, m

    # ---- k_dn_variance ------------------------------------------------------------------------------------------------------
    def variance(self, m):
        zp, gx, gy, octw = self.rec
        valid = self.valid
        var_long = np.maximum(m[..., 1] - m[..., 0] * m[..., 0], F(0))
        Np = oct_decode(octw)
        s1 = np.zeros(zp.shape, F); s2 = np.zeros(zp.shape, F); sw = np.zeros(zp.shape, F)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                zq, inside = _shift(zp, dx, dy, F(0))
                oq, _ = _shift(octw, dx, dy, INVALID)
                ok = inside & (oq != INVALID) & valid
                Nq = oct_decode(oq)
                w = np.exp(-e_z(zp, gx, gy, zq, dx, dy)) * pow128(dot3(Np, Nq))
                mq, _ = _shift(m, dx, dy, F(0))
                s1 = np.where(ok, s1 + w * mq[..., 0], s1)
                s2 = np.where(ok, s2 + w * mq[..., 1], s2)
                sw = np.where(ok, sw + w, sw)
        sws = np.where(sw > 0, sw, F(1)).astype(F)
        a, b = s1 / sws, s2 / sws
        length = np.where(m[..., 2] > 0, m[..., 2], F(1)).astype(F)
        var_short = np.maximum(b - a * a, F(0)) * (F(4) / length)
        return np.where(valid, np.where(m[..., 2] >= F(4), var_long, var_short), F(0)).astype(F)

    # ---- k_dn_atrous --------------------------------------------------------------------------------------------------------
    def atrous(self, c, var, step):
        zp, gx, gy, octw = self.rec
        valid = self.valid
        Np = oct_decode(octw)
        gv = np.zeros(zp.shape, F); gk = np.zeros(zp.shape, F)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                oq, inside = _shift(octw, dx, dy, INVALID)
                ok = inside & (oq != INVALID)
                k = (F(0.5) if dx == 0 else F(0.25)) * (F(0.5) if dy == 0 else F(0.25))
                vq, _ = _shift(var, dx, dy, F(0))
                gv = np.where(ok, gv + k * vq, gv)
                gk = np.where(ok, gk + k, gk)
        gks = np.where(gk > 0, gk, F(1)).astype(F)
        Yp = lum(c[..., 0], c[..., 1], c[..., 2])
        if np.isfinite(self.sigma_l):
            inv_l = F(1) / (self.sigma_l * np.sqrt(gv / gks) + F(1e-10))
        else:  # w_l switched off
            inv_l = np.zeros_like(gv)
        sr = np.zeros(zp.shape, F); sg = np.zeros(zp.shape, F); sb = np.zeros(zp.shape, F); sv = np.zeros(zp.shape, F)
        sw = np.zeros(zp.shape, F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = dx * step, dy * step
                zq, inside = _shift(zp, ox, oy, F(0))
                oq, _ = _shift(octw, ox, oy, INVALID)
                ok = inside & (oq != INVALID) & valid
                cq, _ = _shift(c, ox, oy, F(0))
                vq, _ = _shift(var, ox, oy, F(0))
                e = e_z(zp, gx, gy, zq, ox, oy) + np.abs(Yp - lum(cq[..., 0], cq[..., 1], cq[..., 2])) * inv_l  # w_z * w_l = exp(-e)
                wn = pow128(dot3(Np, oct_decode(oq)))
                w = ((B3[dx + 2] * B3[dy + 2]) * wn) * np.exp(-e)
                sr = np.where(ok, sr + w * cq[..., 0], sr); sg = np.where(ok, sg + w * cq[..., 1], sg)
                sb = np.where(ok, sb + w * cq[..., 2], sb)
                sv = np.where(ok, sv + (w * w) * vq, sv)
                sw = np.where(ok, sw + w, sw)
        sws = np.where(sw > 0, sw, F(1)).astype(F)
        out = np.stack([sr / sws, sg / sws, sb / sws], -1)
        outv = sv / (sws * sws)
        return np.where(valid[..., None], out, F(0)).astype(F), np.where(valid, outv, F(0)).astype(F)

    def denoise(self, view_proj, g, out=None, iterations=5, max_history=32):
        """One vkrt_denoise_diffuse call.  out [H,W,4] float32 (updated in place at valid pixels, .w untouched); returns out."""
        assert 0 <= iterations <= 5 and 1 <= max_history <= 255
        view_proj = np.asarray(view_proj, F).reshape(-1)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
            c, m = self.temporal(view_proj, g, max_history)
            if iterations == 0:
                self.hist = c
            else:
                var = self.variance(m)
                for i in range(iterations):
                    c, var = self.atrous(c, var, 1 << i)
                    if i == 0:
                        self.hist = c
        if out is None:
            out = np.zeros((self.H, self.W, 4), F)
        res = (c * self.factor).astype(F)
        v = self.valid
        out[..., :3][v] = res[v]
        self.prev_vp = view_proj.copy()
        self.has_history = True
        return out
