"""numpy restatement of k_dn_motion_temporal (csrc/denoise.hip; include/vkrt.h vkrt_denoise_diffuse_motion): NpDenoiser whose temporal
stage looks the history up where the pixel's surface point was one call ago.  g["prevPosition"] [H,W,4] holds that point Xp (xyz) and a
flag w: w == 0 = the surface did not exist then, no history.  Xp replaces the pixel's position in two places -- the projection under the
previous call's viewProj and the plane test d = geomPrev[tap] - Xp -- and everything else is np_denoise.NpDenoiser.temporal, restated
here line by line in the same operation order (float32 like the kernel, or float64 as its twin).

A dict without "prevPosition" takes the parent's temporal stage, as Denoiser.denoise takes the plain entry point: the two may be mixed on
one instance.  MOTION_VARIANT lists three one-line departures for the sensitivity tests."""
import numpy as np

import np_denoise as nd
from np_denoise import INVALID, _c, _min_abs, _shift, albedo_arms, albedo_factor, dot3, geom_valid, lum, oct_decode, oct_encode, project

MOTION_VARIANT = dict(
    plane_on_pos=False,     # True: the plane test against the pixel's current position instead of Xp
    project_cur_vp=False,   # True: Xp projected under the current view-projection instead of the previous one
    ignore_w0=False,        # True: prevPosition.w == 0 does not switch the history off
)


class NpMotionDenoiser(nd.NpDenoiser):
    def __init__(self, width, height, sigma_l=None, dtype=np.float32, **variant):
        self.mv = dict(MOTION_VARIANT, **{k: variant.pop(k) for k in list(variant) if k in MOTION_VARIANT})
        super().__init__(width, height, sigma_l=sigma_l, dtype=dtype, **variant)

    def temporal(self, view_proj, g, max_history):
        if "prevPosition" not in g:
            return super().temporal(view_proj, g, max_history)
        W, H, F, v, mv = self.W, self.H, self.F, self.v, self.mv
        pos, nrm, col, rm = (np.asarray(g[k], F) for k in ("position", "normal", "color", "roughMetal"))
        prev = np.asarray(g["prevPosition"], F)
        vz = np.asarray(g["nrdViewZ"], F).reshape(H, W)
        rad = np.asarray(g["nrdRadianceHitDist"], F)
        valid = geom_valid(pos, nrm)
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
                     taps_accepted=0, taps_plane_only=0, taps_normal_only=0, behind_prev=0, q_outside=0, not_existed=0, xp_not_finite=0)
        sw = np.zeros((H, W), F); hr = np.zeros((H, W), F); hg = np.zeros((H, W), F); hb = np.zeros((H, W), F)
        h1 = np.zeros((H, W), F); h2 = np.zeros((H, W), F)
        max_len = np.full((H, W), np.inf if v["len_min"] else 0, F)
        if self.has_history:
            X = pos[..., :3]
            Xp = prev[..., :3]
            existed = np.ones((H, W), bool) if mv["ignore_w0"] else ~(prev[..., 3] == 0)
            pxp, pyp, okp = project(view_proj if mv["project_cur_vp"] else self.prev_vp, Xp, W, H, F)
            pxc, pyc, okc = project(view_proj, X, W, H, F)
            xs = np.arange(W, dtype=F)[None, :].repeat(H, 0)
            ys = np.arange(H, dtype=F)[:, None].repeat(W, 1)
            qx = xs + (pxp - pxc)
            qy = ys + (pyp - pyc)
            inside = existed & okp & okc & valid & (qx > F(-1)) & (qx < F(W)) & (qy > F(-1)) & (qy < F(H))
            cover["not_existed"] = int((valid & ~existed).sum())
            cover["xp_not_finite"] = int((valid & existed & ~np.isfinite(Xp).all(-1)).sum())
            cover["behind_prev"] = int((valid & existed & ~okp).sum())
            cover["q_outside"] = int((valid & existed & okp & okc & ~inside).sum())
            qx = np.where(inside, qx, F(0)).astype(F)
            qy = np.where(inside, qy, F(0)).astype(F)
            x0, y0 = np.floor(qx), np.floor(qy)
            fx, fy = qx - x0, qy - y0
            if v["swap_fxfy"]:
                fx, fy = fy, fx
            tol = _c(F, v["plane_tol"]) * np.abs(vz)
            N = (nrm[..., 0], nrm[..., 1], nrm[..., 2])
            gdec = oct_decode(self.geom_oct, F)
            A = X if mv["plane_on_pos"] else Xp  # the point the previous position plane is held against
            for j in (0, 1):
                for i in (0, 1):
                    w = (fx if i else F(1) - fx) * (fy if j else F(1) - fy)
                    tx = x0.astype(np.int64) + i
                    ty = y0.astype(np.int64) + j
                    ok = inside & (w > 0) & (tx >= 0) & (ty >= 0) & (tx < W) & (ty < H)
                    txc, tyc = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
                    ok &= self.geom_oct[tyc, txc] != INVALID
                    gp = self.geom_pos[tyc, txc]
                    d = (gp[..., 0] - A[..., 0], gp[..., 1] - A[..., 1], gp[..., 2] - A[..., 2])
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
