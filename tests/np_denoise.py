"""numpy restatement of the diffuse denoiser (csrc/denoise.hip: k_dn_temporal, k_dn_variance, k_dn_atrous; include/vkrt.h
vkrt_denoise_diffuse) in the kernels' operation order, in a chosen dtype.

float32 (the default): every array is float32 and every binary operation rounds like the kernels' (built with -ffp-contract=off:
no fused multiply-adds; / and sqrt correctly rounded); expf may differ from np.exp in the last bit, which is what the GPU parity
tests' tolerance is for.  float64: the same expression tree evaluated in binary64 on the same binary32 inputs and with the kernels'
binary32 constants (0.8f, 1e-3f, 1.0f / 32767.0f, ... widened exactly): the high-precision reference of the float32 one and of the
kernels.

Inputs are the planes Renderer.gbuffer_raycast(view_matrix=...) + Renderer.hybrid_trace fill, as numpy arrays:
color / position / normal [H,W,4], roughMetal [H,W,2], nrdViewZ [H,W], nrdRadianceHitDist [H,W,4]."""
import numpy as np

INVALID = np.uint32(0x80008000)  # oct word of a pixel without geometry

# The kernels' constants and the shape of their formulas where a test wants to depart from them (NpDenoiser(..., name=value)): the
# sensitivity tests run one departure at a time and ask that the comparison against the float64 twin sees it.
VARIANT = dict(
    b3_end=0.0625,       # B3 kernel (b3_end, 1/4, 3/8, 1/4, b3_end): its product gives the 5x5 a-trous weights
    g3=(0.5, 0.25),      # centre / edge weight of the 3x3 Gaussian over the variance
    squarings=7,         # w_n = max(0, dot)^(2^squarings)
    sigma_l=4.0,         # luminance edge-stopping constant; np.inf switches w_l off (an experiment, not a kernel mode)
    ez_eps=1e-3,         # the |zp| term of the depth weight's denominator
    short_scale=4.0,     # spatial variance estimate * short_scale / len
    long_len=4.0,        # temporal variance from this history length on
    central_grad=False,  # True: central difference of viewZ instead of the smaller one-sided difference
    swap_fxfy=False,     # True: the bilinear history weights use fy along x and fx along y
    plane_tol=0.01,      # history tap: |N . (X_prev - X)| <= plane_tol |viewZ|
    normal_cos=0.9,      # history tap: N . N_prev >= normal_cos
    len_min=False,       # True: the shortest of the accepted taps' history lengths instead of the longest
    fold_sign=True,      # False: the nz < 0 fold of the oct encoding without its sign factors
    spec=0.8,            # metal * (1 - rough) >= spec: specular branch, not demodulated
    amin=1e-3,           # albedo maximum below amin: black, not demodulated
    floor=True,          # False: no per-channel floor of the albedo at 1e-3
)


def _exp(x):
    """np.exp; a name of its own so that a test can pin the one operation whose last bit depends on the numpy build"""
    return np.exp(x)


def _c(F, v):
    """the kernels' binary32 constant v in dtype F"""
    return F(np.float32(v))


def _sign(v, F=np.float32):
    return np.where(v >= 0, F(1), F(-1)).astype(F)


def oct_encode(nx, ny, nz, F=np.float32, fold_sign=True):
    s = (np.abs(nx) + np.abs(ny)) + np.abs(nz)
    s = np.where(s > 0, s, F(1)).astype(F)
    vx, vy = nx / s, ny / s
    neg = ~(nz >= 0)
    wx = (F(1) - np.abs(vy)) * (_sign(vx, F) if fold_sign else F(1))
    wy = (F(1) - np.abs(vx)) * (_sign(vy, F) if fold_sign else F(1))
    vx, vy = np.where(neg, wx, vx).astype(F), np.where(neg, wy, vy).astype(F)
    qx = np.rint(np.clip(vx, F(-1), F(1)) * F(32767)).astype(np.int32)
    qy = np.rint(np.clip(vy, F(-1), F(1)) * F(32767)).astype(np.int32)
    return ((qx & 0xFFFF).astype(np.uint32) | ((qy & 0xFFFF).astype(np.uint32) << np.uint32(16))).astype(np.uint32)


def oct_decode(bits, F=np.float32):
    bits = np.asarray(bits, np.uint32)
    x = (bits & np.uint32(0xFFFF)).astype(np.uint16).view(np.int16).astype(F) * _c(F, 1.0 / 32767.0)
    y = (bits >> np.uint32(16)).astype(np.uint16).view(np.int16).astype(F) * _c(F, 1.0 / 32767.0)
    z = (F(1) - np.abs(x)) - np.abs(y)
    t = np.maximum(-z, F(0))
    x = x + np.where(x >= 0, -t, t)
    y = y + np.where(y >= 0, -t, t)
    r = F(1) / np.sqrt((x * x + y * y) + z * z)
    return x * r, y * r, z * r


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def lum(r, g, b, F=np.float32):
    return (F(0.25) * r + F(0.5) * g) + F(0.25) * b


def pow128(d, F=np.float32, squarings=7):
    d = np.maximum(d, F(0))
    for _ in range(squarings):
        d = d * d
    return d


def e_z(zp, gx, gy, zq, ox, oy, F=np.float32, eps=1e-3):
    """exponent of the depth weight w_z = exp(-e_z) (sigma_z = 1)"""
    return np.abs(zq - zp) / (F(1) * np.abs(gx * F(ox) + gy * F(oy)) + _c(F, eps) * np.abs(zp))


def geom_valid(pos, nrm):
    return ~(np.all(pos[..., :3] == 0, axis=-1) & np.all(nrm[..., :3] == 0, axis=-1))


def albedo_arms(color, pos, nrm, rm, F=np.float32, spec=0.8, amin=1e-3):
    """(specular, black) masks of dnAlbedo's two early returns; neither: the demodulating arm"""
    ratio = rm[..., 1] * (F(1) - rm[..., 0])
    amax = np.maximum(np.maximum(color[..., 3], pos[..., 3]), nrm[..., 3])
    specular = ~(ratio < _c(F, spec))
    return specular, ~specular & ~(amax >= _c(F, amin))


def albedo_factor(color, pos, nrm, rm, F=np.float32, spec=0.8, amin=1e-3, floor=True):
    """curWeight of k_hybrid: albedo (floored at 1e-3 per channel) on the diffuse branch, 1 on the specular branch / black albedo"""
    a = np.stack([color[..., 3], pos[..., 3], nrm[..., 3]], -1)
    specular, black = albedo_arms(color, pos, nrm, rm, F, spec, amin)
    keep = specular | black
    return np.where(keep[..., None], F(1), np.maximum(a, _c(F, 1e-3)) if floor else a).astype(F)


def project(M, X, W, H, F=np.float32):
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


def _min_abs(a, b, F=np.float32):
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
    def __init__(self, width, height, sigma_l=None, dtype=np.float32, **variant):
        """dtype: np.float32 (the kernels' arithmetic) or np.float64 (the reference).  variant: departures from VARIANT's values."""
        unknown = set(variant) - set(VARIANT)
        assert not unknown, unknown
        self.W, self.H = int(width), int(height)
        self.F = F = np.dtype(dtype).type
        self.v = dict(VARIANT, **variant)
        if sigma_l is not None:
            self.v["sigma_l"] = sigma_l
        self.sigma_l = F(np.float32(self.v["sigma_l"]))
        b = self.v["b3_end"]
        self.b3 = tuple(_c(F, k) for k in (b, 0.25, 0.375, 0.25, b))
        self.reset()
        self.hist = np.zeros((self.H, self.W, 3), F)
        self.geom_pos = np.zeros((self.H, self.W, 3), F)
        self.geom_oct = np.full((self.H, self.W), INVALID, np.uint32)
        self.mom = np.zeros((self.H, self.W, 3), F)
        self.prev_vp = np.zeros(16, F)
        self.cover = {}  # branch counts of the last call (pixels or history taps): what a test's inputs reached

    def reset(self):
        self.has_history = False

    # ---- k_dn_temporal ------------------------------------------------------------------------------------------------------
    def temporal(self, view_proj, g, max_history):
        W, H, F, v = self.W, self.H, self.F, self.v
        pos, nrm, col, rm = (np.asarray(g[k], F) for k in ("position", "normal", "color", "roughMetal"))
        vz = np.asarray(g["nrdViewZ"], F).reshape(H, W)
        rad = np.asarray(g["nrdRadianceHitDist"], F)
        valid = geom_valid(pos, nrm)
        # viewZ gradient: the smaller of the two one-sided differences (one-sided next to a pixel without geometry)
        zl, vl = _shift(vz, -1, 0, F(0)); zr, vr = _shift(vz, 1, 0, F(0))
        zu, vu = _shift(vz, 0, -1, F(0)); zd, vd = _shift(vz, 0, 1, F(0))
        vl &= _shift(valid, -1, 0, False)[0]; vr &= _shift(valid, 1, 0, False)[0]
        vu &= _shift(valid, 0, -1, False)[0]; vd &= _shift(valid, 0, 1, False)[0]
        zl, zr, zu, zd = (np.where(m, z, F(0)).astype(F) for m, z in ((vl, zl), (vr, zr), (vu, zu), (vd, zd)))
        if v["central_grad"]:
            two = lambda a, b: (a + b) * F(0.5)  # noqa: E731
        else:
            two = lambda a, b: _min_abs(a, b, F)  # noqa: E731
        gx = np.where(vl & vr, two(zr - vz, vz - zl), np.where(vr, zr - vz, np.where(vl, vz - zl, F(0)))).astype(F)
        gy = np.where(vu & vd, two(zd - vz, vz - zu), np.where(vd, zd - vz, np.where(vu, vz - zu, F(0)))).astype(F)
        octw = np.where(valid, oct_encode(nrm[..., 0], nrm[..., 1], nrm[..., 2], F, v["fold_sign"]), INVALID).astype(np.uint32)
        self.rec = (np.where(valid, vz, F(0)).astype(F), np.where(valid, gx, F(0)).astype(F), np.where(valid, gy, F(0)).astype(F), octw)
        # current sample.  fmax, as the kernel's fmaxf: a NaN sample counts as black
        f = albedo_factor(col, pos, nrm, rm, F, v["spec"], v["amin"], v["floor"])
        t = rad[..., 0] - rad[..., 2]
        cr = np.fmax(t + rad[..., 1], F(0)) / f[..., 0]
        cg = np.fmax(rad[..., 0] + rad[..., 2], F(0)) / f[..., 1]
        cb = np.fmax(t - rad[..., 1], F(0)) / f[..., 2]
        Y = lum(cr, cg, cb, F)
        specular, black = albedo_arms(col, pos, nrm, rm, F, v["spec"], v["amin"])
        floored = valid & ~specular & ~black & (np.minimum(np.minimum(col[..., 3], pos[..., 3]), nrm[..., 3]) < _c(F, 1e-3))
        cover = dict(valid=int(valid.sum()), nz_neg=int((valid & ~(nrm[..., 2] >= 0)).sum()), arm_specular=int((valid & specular).sum()),
                     arm_black=int((valid & black).sum()), arm_diffuse=int((valid & ~specular & ~black).sum()), floored=int(floored.sum()),
                     taps_accepted=0, taps_plane_only=0, taps_normal_only=0, behind_prev=0, q_outside=0)
        # history taps
        sw = np.zeros((H, W), F); hr = np.zeros((H, W), F); hg = np.zeros((H, W), F); hb = np.zeros((H, W), F)
        h1 = np.zeros((H, W), F); h2 = np.zeros((H, W), F)
        max_len = np.full((H, W), np.inf if v["len_min"] else 0, F)
        if self.has_history:
            X = pos[..., :3]
            pxp, pyp, okp = project(self.prev_vp, X, W, H, F)
            pxc, pyc, okc = project(view_proj, X, W, H, F)
            xs = np.arange(W, dtype=F)[None, :].repeat(H, 0)
            ys = np.arange(H, dtype=F)[:, None].repeat(W, 1)
            qx = xs + (pxp - pxc)
            qy = ys + (pyp - pyc)
            inside = okp & okc & valid & (qx > F(-1)) & (qx < F(W)) & (qy > F(-1)) & (qy < F(H))
            cover["behind_prev"] = int((valid & ~okp).sum())
            cover["q_outside"] = int((valid & okp & okc & ~inside).sum())
            qx = np.where(inside, qx, F(0)).astype(F)
            qy = np.where(inside, qy, F(0)).astype(F)
            x0, y0 = np.floor(qx), np.floor(qy)
            fx, fy = qx - x0, qy - y0
            if v["swap_fxfy"]:
                fx, fy = fy, fx
            tol = _c(F, v["plane_tol"]) * np.abs(vz)
            N = (nrm[..., 0], nrm[..., 1], nrm[..., 2])
            gdec = oct_decode(self.geom_oct, F)
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
                    plane = np.abs(dot3(N, d)) <= tol
                    facing = dot3(N, tuple(c[tyc, txc] for c in gdec)) >= _c(F, v["normal_cos"])
                    cover["taps_plane_only"] += int((ok & ~plane & facing).sum())
                    cover["taps_normal_only"] += int((ok & plane & ~facing).sum())
                    ok &= plane
                    ok &= facing
                    cover["taps_accepted"] += int(ok.sum())
                    m = self.mom[tyc, txc]
                    h = self.hist[tyc, txc]
                    w = np.where(ok, w, F(0)).astype(F)
                    sw = np.where(ok, sw + w, sw)
                    hr = np.where(ok, hr + w * h[..., 0], hr); hg = np.where(ok, hg + w * h[..., 1], hg); hb = np.where(ok, hb + w * h[..., 2], hb)
                    h1 = np.where(ok, h1 + w * m[..., 0], h1); h2 = np.where(ok, h2 + w * m[..., 1], h2)
                    max_len = np.where(ok, (np.minimum if v["len_min"] else np.maximum)(max_len, m[..., 2]), max_len)
        hist = sw > 0
        sws = np.where(hist, sw, F(1)).astype(F)
        length = np.where(hist, np.minimum(max_len, F(max_history - 1)) + F(1), F(1)).astype(F)
        a = F(1) / length
        blend = lambda s, c: np.where(hist, (s / sws) * (F(1) - a) + c * a, c).astype(F)  # noqa: E731
        c = np.stack([blend(hr, cr), blend(hg, cg), blend(hb, cb)], -1)
        m = np.stack([blend(h1, Y), blend(h2, Y * Y), length], -1)
        c = np.where(valid[..., None], c, F(0)).astype(F)
        m = np.where(valid[..., None], m, F(0)).astype(F)
        self.valid, self.factor, self.cover = valid, f, cover
        self.geom_pos = np.where(valid[..., None], pos[..., :3], F(0)).astype(F)
        self.geom_oct = octw
        self.mom = m
        return c, m

    # ---- k_dn_variance ------------------------------------------------------------------------------------------------------
    def variance(self, m):
        F, v = self.F, self.v
        zp, gx, gy, octw = self.rec
        valid = self.valid
        var_long = np.maximum(m[..., 1] - m[..., 0] * m[..., 0], F(0))
        Np = oct_decode(octw, F)
        s1 = np.zeros(zp.shape, F); s2 = np.zeros(zp.shape, F); sw = np.zeros(zp.shape, F)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                zq, inside = _shift(zp, dx, dy, F(0))
                oq, _ = _shift(octw, dx, dy, INVALID)
                ok = inside & (oq != INVALID) & valid
                Nq = oct_decode(oq, F)
                w = _exp(-e_z(zp, gx, gy, zq, dx, dy, F, v["ez_eps"])) * pow128(dot3(Np, Nq), F, v["squarings"])
                mq, _ = _shift(m, dx, dy, F(0))
                s1 = np.where(ok, s1 + w * mq[..., 0], s1)
                s2 = np.where(ok, s2 + w * mq[..., 1], s2)
                sw = np.where(ok, sw + w, sw)
        sws = np.where(sw > 0, sw, F(1)).astype(F)
        a, b = s1 / sws, s2 / sws
        length = np.where(m[..., 2] > 0, m[..., 2], F(1)).astype(F)
        var_short = np.maximum(b - a * a, F(0)) * (_c(F, v["short_scale"]) / length)
        long_path = m[..., 2] >= _c(F, v["long_len"])
        self.cover["var_long"] = int((valid & long_path).sum())
        self.cover["var_short"] = int((valid & ~long_path).sum())
        return np.where(valid, np.where(long_path, var_long, var_short), F(0)).astype(F)

    # ---- k_dn_atrous --------------------------------------------------------------------------------------------------------
    def atrous(self, c, var, step):
        F, v = self.F, self.v
        zp, gx, gy, octw = self.rec
        valid = self.valid
        Np = oct_decode(octw, F)
        gv = np.zeros(zp.shape, F); gk = np.zeros(zp.shape, F)
        g_mid, g_edge = _c(F, v["g3"][0]), _c(F, v["g3"][1])
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                oq, inside = _shift(octw, dx, dy, INVALID)
                ok = inside & (oq != INVALID)
                k = (g_mid if dx == 0 else g_edge) * (g_mid if dy == 0 else g_edge)
                vq, _ = _shift(var, dx, dy, F(0))
                gv = np.where(ok, gv + k * vq, gv)
                gk = np.where(ok, gk + k, gk)
        gks = np.where(gk > 0, gk, F(1)).astype(F)
        Yp = lum(c[..., 0], c[..., 1], c[..., 2], F)
        if np.isfinite(self.sigma_l):
            inv_l = F(1) / (self.sigma_l * np.sqrt(gv / gks) + _c(F, 1e-10))
        else:  # w_l switched off
            inv_l = np.zeros_like(gv)
        sr = np.zeros(zp.shape, F); sg = np.zeros(zp.shape, F); sb = np.zeros(zp.shape, F); sv = np.zeros(zp.shape, F)
        sw = np.zeros(zp.shape, F)
        B3 = self.b3
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = dx * step, dy * step
                zq, inside = _shift(zp, ox, oy, F(0))
                oq, _ = _shift(octw, ox, oy, INVALID)
                ok = inside & (oq != INVALID) & valid
                cq, _ = _shift(c, ox, oy, F(0))
                vq, _ = _shift(var, ox, oy, F(0))
                # w_z * w_l = exp(-e)
                e = e_z(zp, gx, gy, zq, ox, oy, F, v["ez_eps"]) + np.abs(Yp - lum(cq[..., 0], cq[..., 1], cq[..., 2], F)) * inv_l
                wn = pow128(dot3(Np, oct_decode(oq, F)), F, v["squarings"])
                w = ((B3[dx + 2] * B3[dy + 2]) * wn) * _exp(-e)
                sr = np.where(ok, sr + w * cq[..., 0], sr); sg = np.where(ok, sg + w * cq[..., 1], sg)
                sb = np.where(ok, sb + w * cq[..., 2], sb)
                sv = np.where(ok, sv + (w * w) * vq, sv)
                sw = np.where(ok, sw + w, sw)
        sws = np.where(sw > 0, sw, F(1)).astype(F)
        out = np.stack([sr / sws, sg / sws, sb / sws], -1)
        outv = sv / (sws * sws)
        return np.where(valid[..., None], out, F(0)).astype(F), np.where(valid, outv, F(0)).astype(F)

    def denoise(self, view_proj, g, out=None, iterations=5, max_history=32):
        """One vkrt_denoise_diffuse call.  out [H,W,4] of the denoiser's dtype (updated in place at valid pixels, .w untouched);
        returns out."""
        assert 0 <= iterations <= 5 and 1 <= max_history <= 255
        F = self.F
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
