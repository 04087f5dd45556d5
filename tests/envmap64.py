"""A float64 restatement of emitter `envmap` (src/emitters/envmap.cpp) for the tests: the texels rounded to IEEE half as the reference's
TMIPMap<Spectrum, SpectrumHalf> keeps them (:100-190), the sampling tables built from them in float32 in the reference's order
(configure(), :260-320), and evalEnvironment (:380-415, level-0 evalBilinear of include/mitsuba/render/mipmap.h:573-596),
internalSampleDirection (:554-610, sampleReuse :657-662, warp::squareToTent) and internalPdfDirection (:612-645) in float64 on top of
those tables.  Vectorised over numpy arrays of directions / samples."""
import numpy as np

LUM = np.array([0.212671, 0.715160, 0.072169])          # include/mitsuba/core/spectrum.h:638
EPSILON = 1e-4                                           # include/mitsuba/core/constants.h (single precision)


class EnvMap64:
    def __init__(self, image, to_world=None, scale=1.0):
        img = np.asarray(image, np.float32)
        self.h, self.w = img.shape[:2]
        with np.errstate(over="ignore"):
            self.tex = img.astype(np.float16).astype(np.float64)               # level 0, half-rounded (beyond 65504: inf, as the reference's half)
        self.scale = float(scale)
        m = np.eye(4) if to_world is None else np.asarray(to_world, np.float64)
        self.R = np.asarray(m, np.float64)[:3, :3].astype(np.float32).astype(np.float64)
        self.Rinv = np.linalg.inv(self.R)
        self._tables()

    def _tables(self):
        W, H = self.w, self.h
        lum32 = (self.tex[..., 0].astype(np.float32) * np.float32(0.212671) + self.tex[..., 1].astype(np.float32) * np.float32(0.715160)
                 + self.tex[..., 2].astype(np.float32) * np.float32(0.072169))
        cols = np.zeros((H, W + 1), np.float32)
        rows = np.zeros(H + 1, np.float32)
        weights = np.zeros(H, np.float32)
        row_sum = np.float32(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            for y in range(H):
                col = np.cumsum(lum32[y], dtype=np.float32)                    # sequential float32 accumulation in x order
                cols[y, 1:] = col
                cols[y, 1:W] *= np.float32(1) / col[-1]
                cols[y, W] = 1
                wgt = np.float32(np.sin(float(np.float32(y) + np.float32(0.5)) * np.pi / H))
                weights[y] = wgt
                row_sum = np.float32(row_sum + np.float32(col[-1] * wgt))
                rows[y + 1] = row_sum
            rows[1:H] *= np.float32(1) / row_sum
        rows[H] = 1
        if row_sum == 0:
            raise ValueError("The environment map is completely black -- this is not allowed.")
        if not np.isfinite(row_sum):
            raise ValueError("The environment map contains an invalid floating point value (nan/inf) -- giving up.")
        self.cdf_cols, self.cdf_rows, self.row_weights = cols, rows, weights
        self.norm = float(np.float32(1.0 / (float(row_sum) * (2 * np.pi / W) * (np.pi / H))))
        self.pix = (2 * np.pi / W, np.pi / H)

    # ---- look-ups
    def texel(self, x, y):
        x = np.mod(x, self.w)
        y = np.clip(y, 0, self.h - 1)
        return self.tex[y, x]

    def _rows(self, fx, fy):
        x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
        dx1, dy1 = (fx - x0)[:, None], (fy - y0)[:, None]
        v1 = self.texel(x0, y0) * (1 - dx1) * (1 - dy1) + self.texel(x0 + 1, y0) * dx1 * (1 - dy1)
        v2 = self.texel(x0, y0 + 1) * (1 - dx1) * dy1 + self.texel(x0 + 1, y0 + 1) * dx1 * dy1
        return v1, v2, y0

    def _row_pdf(self, v1, v2, y0):
        w = self.row_weights.astype(np.float64)
        return (v1 @ LUM * w[np.clip(y0, 0, self.h - 1)] + v2 @ LUM * w[np.clip(y0 + 1, 0, self.h - 1)]) * self.norm

    def uv(self, dirs):
        """lat-long coordinates of world directions (not necessarily unit)"""
        v = np.asarray(dirs, np.float64) @ self.Rinv.T
        v = v / np.linalg.norm(v, axis=1, keepdims=True)
        return np.arctan2(v[:, 0], -v[:, 2]) / (2 * np.pi), np.arccos(np.clip(v[:, 1], -1, 1)) / np.pi, v

    def eval(self, dirs):
        """(value x scale, pdfDirect) at world directions"""
        u, t, v = self.uv(dirs)
        v1, v2, y0 = self._rows(u * self.w - 0.5, t * self.h - 0.5)
        sin_t = np.sqrt(np.maximum(1 - v[:, 1] ** 2, 0))
        return (v1 + v2) * self.scale, self._row_pdf(v1, v2, y0) / np.maximum(sin_t, EPSILON)

    def pdf(self, dirs):
        return self.eval(dirs)[1]

    @staticmethod
    def _reuse(cdf, rows, size, s):
        """sampleReuse: lower_bound over cdf[row, 0 .. size] (float32 tables, one per sample's row), index clamped to [0, size - 1], the
        sample rescaled.  Vectorised: row r's entries (all in [0, 1]) are shifted by 2 r, which keeps every comparison exact."""
        cdf = np.asarray(cdf, np.float32).reshape(-1, size + 1)
        keyed = (cdf.astype(np.float64) + 2.0 * np.arange(cdf.shape[0])[:, None]).ravel()
        q = np.asarray(s, np.float32).astype(np.float64) + 2.0 * rows
        idx = np.clip(np.searchsorted(keyed, q, side="left") - rows * (size + 1) - 1, 0, size - 1)
        lo = cdf[rows, idx].astype(np.float64); hi = cdf[rows, idx + 1].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return idx, (s - lo) / (hi - lo)

    @staticmethod
    def _tent(s):
        return np.where(s < 0.5, 1 - np.sqrt(2 * s), -(1 - np.sqrt(np.maximum(2 * (s - 0.5), 0))))

    def sample(self, u2):
        """sampleDirect: (row, col, world direction, value x scale / pdf, pdf) for samples u2 (n x 2)"""
        u2 = np.asarray(u2, np.float64)
        n = u2.shape[0]
        row, sy = self._reuse(self.cdf_rows, np.zeros(n, np.int64), self.h, u2[:, 1])
        col, sx = self._reuse(self.cdf_cols, row, self.w, u2[:, 0])
        px, py = col + self._tent(sx), row + self._tent(sy)
        v1, v2, y0 = self._rows(px, py)
        value = (v1 + v2) * self.scale
        phi, theta = self.pix[0] * (px + 0.5), self.pix[1] * (py + 0.5)
        d = np.stack([np.sin(phi) * np.sin(theta), np.cos(theta), -np.cos(phi) * np.sin(theta)], axis=1)
        pdf = self._row_pdf(v1, v2, y0) / np.maximum(np.abs(np.sin(theta)), EPSILON)
        with np.errstate(divide="ignore", invalid="ignore"):
            vop = np.where((pdf > 0)[:, None] & np.any(value != 0, axis=1)[:, None], value / pdf[:, None], 0.0)
        return row, col, d @ self.R.T, vop, np.where(pdf > 0, pdf, 0.0)


def sun_and_gradient(h=24, w=40):
    """a strongly non-uniform test map: a vertical colour gradient and a small bright 'sun'; non-power-of-two sides"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([0.2 + 0.8 * y / h, 0.3 + 0.4 * x / w, 1.0 - 0.7 * y / h], axis=2)
    img[h // 4:h // 4 + 2, (3 * w) // 5:(3 * w) // 5 + 3] = [60.0, 50.0, 30.0]
    return img.astype(np.float32)


def rot(axis, deg):
    """4x4 rotation about a unit axis"""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    t = np.radians(deg); K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4); m[:3, :3] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
    return m
