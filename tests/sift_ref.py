"""Float64 numpy restatement of the SIFT node extractor (OpenCV's algorithm with the
reference's settings, restated; lesion_gnn_amd/datasets/nodes/sift.py runs it in HIP).

One function per stage, so a test can start a stage from given inputs: `gray`, `pyramid`,
`candidates`, `refine`, `orient`, `select`, `descriptors`, and `extract` for the whole chain. The
scale space is float64 here and fp32 on the device; the stages after it read an fp32 pyramid (the
oracle's own rounded, or the device's) and compute in float64 in the order the kernels do.

Every discrete decision notes its relative margin to its threshold in a `Margins`; the cases are
chosen so that the smallest is far above float64 rounding (tests/test_sift_ref.py).
"""
from __future__ import annotations

import math

import numpy as np

LAYERS = 3            # nOctaveLayers
EDGE = 10.0           # edgeThreshold
BORDER = 5
STEPS = 5             # refinement steps
INIT_SIGMA = 0.5      # assumed blur of the input
ORI_BINS = 36
ORI_SIG = 1.5
ORI_RADIUS = 4.5
ORI_PEAK = 0.8
D_WIDTH, D_BINS = 4, 8
D_SCALE = 3.0
D_CLAMP = 0.2
D_FACTOR = 512.0
FLT_EPSILON = float(np.finfo(np.float32).eps)
SINGULAR = 100 * float(np.finfo(np.float64).eps)
INT_MAX_3 = float(2**31 - 1) / 3.0
DEG = 180.0 / math.pi
RAD = math.pi / 180.0


class Margins:
    """The smallest relative distance of any decision's value from its threshold."""

    def __init__(self):
        self.smallest = math.inf
        self.where = None

    def note(self, a: float, b: float, where: str) -> None:
        m = abs(a - b) / max(abs(a), abs(b), 1e-300)
        if m < self.smallest:
            self.smallest, self.where = m, where

    def note_round(self, v: float, where: str) -> None:
        """v is about to be rounded to an integer: its distance from the nearest half."""
        f = v - math.floor(v)
        m = abs(f - 0.5) / max(abs(v), 1.0)
        if m < self.smallest:
            self.smallest, self.where = m, where


def cv_round(v: float) -> int:
    return int(np.rint(v))  # half to even, as cvRound


# ---- steps 1-3: gray, base, octaves ---------------------------------------------------------------

def gray(image: np.ndarray) -> np.ndarray:
    """uint8 (H, W, 3) -> uint8 (H, W) with the integer weights of a BGR conversion applied to the
    RGB array the reference passes: channel 0 (red) gets the 0.114 weight. (H, W) is returned as
    it is."""
    if image.ndim == 2:
        return image.copy()
    c = image.astype(np.int64)
    return ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def kernel_size(sigma: float) -> int:
    return cv_round(8.0 * sigma + 1.0) | 1


def gaussian_kernel(sigma: float) -> np.ndarray:
    k = kernel_size(sigma)
    x = np.arange(k, dtype=np.float64) - (k - 1) // 2
    w = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return w / w.sum()


def reflect101(i: np.ndarray, n: int) -> np.ndarray:
    i = np.array(i, dtype=np.int64)
    for _ in range(8):  # bounded: every pass brings an index nearer to [0, n)
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * (n - 1) - i, i)
    assert ((i >= 0) & (i < n)).all()
    return i


def blur(img: np.ndarray, sigma: float) -> np.ndarray:
    w = gaussian_kernel(sigma)
    r = (len(w) - 1) // 2
    H, W = img.shape
    cols = reflect101(np.arange(W)[:, None] + np.arange(-r, r + 1)[None, :], W)
    rows = reflect101(np.arange(H)[:, None] + np.arange(-r, r + 1)[None, :], H)
    tmp = np.zeros_like(img)
    for t in range(len(w)):  # rows first, taps in order
        tmp = tmp + w[t] * img[:, cols[:, t]]
    out = np.zeros_like(img)
    for t in range(len(w)):
        out = out + w[t] * tmp[rows[:, t], :]
    return out


def double_image(g: np.ndarray) -> np.ndarray:
    H, W = g.shape

    def taps(n):
        s = (np.arange(2 * n, dtype=np.float64) + 0.5) / 2.0 - 0.5
        i0 = np.floor(s)
        f = s - i0
        i0 = i0.astype(np.int64)
        return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), f

    y0, y1, fy = taps(H)
    x0, x1, fx = taps(W)
    g = g.astype(np.float64)
    top = g[y0][:, x0] * (1 - fx) + g[y0][:, x1] * fx
    bot = g[y1][:, x0] * (1 - fx) + g[y1][:, x1] * fx
    return top * (1 - fy)[:, None] + bot * fy[:, None]


def octave_dims(H: int, W: int) -> list[tuple[int, int]]:
    """The (height, width) of every octave built for an (H, W) image."""
    h, w = 2 * H, 2 * W
    n = cv_round(math.log(min(h, w)) / math.log(2.0) - 2.0) + 1
    dims = []
    for _ in range(n):
        if min(h, w) <= 10:
            break
        dims.append((h, w))
        h, w = h // 2, w // 2
    return dims


def level_sigmas(sigma: float) -> list[float]:
    """The blur that takes level i - 1 to level i, i = 1..5."""
    k = 2.0 ** (1.0 / LAYERS)
    out = []
    for i in range(1, LAYERS + 3):
        prev = sigma * k ** (i - 1)
        out.append(math.sqrt((prev * k) ** 2 - prev ** 2))
    return out


def base_sigma(sigma: float) -> float:
    return math.sqrt(max(sigma * sigma - (2 * INIT_SIGMA) ** 2, 0.01))


def pyramid(g: np.ndarray, sigma: float):
    """gray uint8 (H, W) -> (gauss, dog): per octave float64 (6, h, w) and (5, h, w)."""
    dims = octave_dims(*g.shape)
    sig = level_sigmas(sigma)
    gauss, dog = [], []
    level = blur(double_image(g), base_sigma(sigma))
    for o, (h, w) in enumerate(dims):
        if o:
            level = gauss[-1][LAYERS][::2, ::2][:h, :w]
        assert level.shape == (h, w)
        levels = [level]
        for s in sig:
            levels.append(blur(levels[-1], s))
        gauss.append(np.stack(levels))
        dog.append(gauss[-1][1:] - gauss[-1][:-1])
    return gauss, dog


def level_bounds(H: int, W: int, sigma: float):
    """The absolute fp32 error bound of every Gaussian level (per octave, 6 values) and DoG level
    (5 values): every level is a convex combination of values in [0, 255]; one separable blur of
    ksize taps adds at most 2 * (ksize + 1) * 2^-24 * 255 (a rounded weight, a product and a sum
    per tap, rows and columns); the doubling is exact in fp32 (multiples of 1/16 below 256). The
    bound is carried from level to level and across octaves; a DoG level's is its two levels'."""
    unit = 2.0 ** -24 * 255.0
    sig = level_sigmas(sigma)
    gb, db = [], []
    b = 2 * (kernel_size(base_sigma(sigma)) + 1) * unit
    for o in range(len(octave_dims(H, W))):
        if o:
            b = gb[-1][LAYERS]
        lv = [b]
        for s in sig:
            lv.append(lv[-1] + 2 * (kernel_size(s) + 1) * unit)
        gb.append(lv)
        db.append([lv[i] + lv[i + 1] for i in range(LAYERS + 2)])
    return gb, db


def to_f32(levels):
    return [np.ascontiguousarray(a, dtype=np.float32) for a in levels]


# ---- step 4: candidates -------------------------------------------------------------------------

def candidates(dog) -> np.ndarray:
    """fp32 DoG octaves -> int32 (n, 4): (octave, layer, row, column) in that order."""
    out = []
    for o, d in enumerate(dog):
        _, h, w = d.shape
        if h <= 2 * BORDER or w <= 2 * BORDER:
            continue
        for layer in range(1, LAYERS + 1):
            v = d[layer, BORDER:h - BORDER, BORDER:w - BORDER]
            hi = np.ones(v.shape, bool)
            lo = np.ones(v.shape, bool)
            for dl in (-1, 0, 1):
                for dr in (-1, 0, 1):
                    for dc in (-1, 0, 1):
                        if dl == dr == dc == 0:
                            continue
                        nb = d[layer + dl, BORDER + dr:h - BORDER + dr, BORDER + dc:w - BORDER + dc]
                        hi &= v >= nb
                        lo &= v <= nb
            rr, cc = np.nonzero(((v > 0) & hi) | ((v < 0) & lo))
            out += [(o, layer, r + BORDER, c + BORDER) for r, c in zip(rr, cc)]
    return np.array(out, dtype=np.int32).reshape(-1, 4)


# ---- step 5: refinement ---------------------------------------------------------------------------

def solve3(A, b):
    """Gaussian elimination with partial pivoting; a singular system gives zeros."""
    A = [list(map(float, row)) for row in A]
    b = list(map(float, b))
    for i in range(3):
        k = i
        for j in range(i + 1, 3):
            if abs(A[j][i]) > abs(A[k][i]):
                k = j
        if abs(A[k][i]) < SINGULAR:
            return [0.0, 0.0, 0.0]
        if k != i:
            A[i], A[k] = A[k], A[i]
            b[i], b[k] = b[k], b[i]
        d = -1.0 / A[i][i]
        for j in range(i + 1, 3):
            alpha = A[j][i] * d
            for c in range(i + 1, 3):
                A[j][c] += alpha * A[i][c]
            b[j] += alpha * b[i]
    x = [0.0, 0.0, 0.0]
    for i in (2, 1, 0):
        s = b[i]
        for c in range(i + 1, 3):
            s -= A[i][c] * x[c]
        x[i] = s / A[i][i]
    return x


def _derivs(d, layer, r, c):
    scale = 1.0 / 255.0
    img, prv, nxt = (d[layer].astype(np.float64), d[layer - 1].astype(np.float64),
                     d[layer + 1].astype(np.float64))
    dD = [(img[r, c + 1] - img[r, c - 1]) * (scale * 0.5),
          (img[r + 1, c] - img[r - 1, c]) * (scale * 0.5),
          (nxt[r, c] - prv[r, c]) * (scale * 0.5)]
    v2 = img[r, c] * 2.0
    dxx = (img[r, c + 1] + img[r, c - 1] - v2) * scale
    dyy = (img[r + 1, c] + img[r - 1, c] - v2) * scale
    dss = (nxt[r, c] + prv[r, c] - v2) * scale
    dxy = (img[r + 1, c + 1] - img[r + 1, c - 1] - img[r - 1, c + 1] + img[r - 1, c - 1]) * (scale * 0.25)
    dxs = (nxt[r, c + 1] - nxt[r, c - 1] - prv[r, c + 1] + prv[r, c - 1]) * (scale * 0.25)
    dys = (nxt[r + 1, c] - nxt[r - 1, c] - prv[r + 1, c] + prv[r - 1, c]) * (scale * 0.25)
    return dD, dxx, dyy, dss, dxy, dxs, dys


def refine(dog, cand: np.ndarray, sigma: float, margins: Margins | None = None):
    """OpenCV's adjustLocalExtrema per candidate. Returns a list with one entry per candidate:
    None if rejected, else dict(octave, layer, r, c, x, y, size, response) with the four floats
    rounded to fp32 (not yet halved)."""
    m = margins or Margins()
    out = []
    for o, layer, r, c in cand.tolist():
        d = dog[o]
        _, h, w = d.shape
        ok = False
        xi = xr = xc = 0.0
        for _ in range(STEPS):
            dD, dxx, dyy, dss, dxy, dxs, dys = _derivs(d, layer, r, c)
            X = solve3([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]], dD)
            xc, xr, xi = -X[0], -X[1], -X[2]
            for v in (xc, xr, xi):
                m.note(abs(v), 0.5, "offset against 0.5")
            if abs(xi) < 0.5 and abs(xr) < 0.5 and abs(xc) < 0.5:
                ok = True
                break
            if abs(xi) > INT_MAX_3 or abs(xr) > INT_MAX_3 or abs(xc) > INT_MAX_3:
                break
            for v in (xc, xr, xi):
                m.note_round(v, "offset rounding")
            c += cv_round(xc)
            r += cv_round(xr)
            layer += cv_round(xi)
            if (layer < 1 or layer > LAYERS or c < BORDER or c >= w - BORDER or r < BORDER
                    or r >= h - BORDER):
                break
        if not ok:
            out.append(None)
            continue
        dD, dxx, dyy, dss, dxy, dxs, dys = _derivs(d, layer, r, c)
        t = dD[0] * xc + dD[1] * xr + dD[2] * xi
        contr = float(d[layer, r, c]) * (1.0 / 255.0) + t * 0.5
        tr = dxx + dyy
        det = dxx * dyy - dxy * dxy
        m.note(det, 0.0, "det against 0") if det != 0 else None
        m.note(tr * tr * EDGE, (EDGE + 1.0) * (EDGE + 1.0) * det, "edge test")
        if det <= 0 or tr * tr * EDGE >= (EDGE + 1.0) * (EDGE + 1.0) * det:
            out.append(None)
            continue
        s = float(1 << o)
        out.append(dict(
            octave=o, layer=layer, r=r, c=c,
            x=np.float32((c + xc) * s), y=np.float32((r + xr) * s),
            size=np.float32(sigma * math.pow(2.0, (layer + xi) / LAYERS) * s * 2.0),
            response=np.float32(abs(contr))))
    return out


# ---- step 6: orientation ----------------------------------------------------------------------------

def gradient_bin(dx: np.ndarray, dy: np.ndarray, margins: Margins | None = None) -> np.ndarray:
    """The 36-bin index of each gradient: round(atan2 in degrees / 10), with the exact ties
    |dx| == |dy| sent to the lower bin by a branch."""
    ori = np.arctan2(dy, dx) * DEG
    ori = np.where(ori < 0, ori + 360.0, ori)
    t = ori / (360.0 / ORI_BINS)
    b = np.rint(t).astype(np.int64)
    tie = np.abs(dx) == np.abs(dy)
    quad = np.where(dy > 0, np.where(dx > 0, 4, 13), np.where(dx < 0, 22, 31))
    quad = np.where((dx == 0) & (dy == 0), 0, quad)
    b = np.where(tie, quad, b)
    if margins is not None and (~tie).any():
        f = t[~tie] - np.floor(t[~tie])
        k = np.argmin(np.abs(f - 0.5))
        margins.note_round(float(t[~tie][k]), "orientation bin")
    return np.where(b >= ORI_BINS, b - ORI_BINS, b)


def orientation_hist(img: np.ndarray, c: int, r: int, radius: int, sigma: float,
                     margins: Margins | None = None) -> np.ndarray:
    h, w = img.shape
    img = img.astype(np.float64)
    ii, jj = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1),
                         indexing="ij")
    y, x = r + ii, c + jj
    keep = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    y, x, ii, jj = y[keep], x[keep], ii[keep], jj[keep]  # raster order
    dx = img[y, x + 1] - img[y, x - 1]
    dy = img[y - 1, x] - img[y + 1, x]
    wgt = np.exp((ii * ii + jj * jj).astype(np.float64) * (-1.0 / (2.0 * sigma * sigma)))
    mag = np.sqrt(dx * dx + dy * dy)
    raw = np.zeros(ORI_BINS)
    np.add.at(raw, gradient_bin(dx, dy, margins), wgt * mag)
    n = ORI_BINS
    hist = np.zeros(n)
    for i in range(n):
        hist[i] = ((raw[(i - 2) % n] + raw[(i + 2) % n]) * (1.0 / 16.0)
                   + (raw[(i - 1) % n] + raw[(i + 1) % n]) * (4.0 / 16.0)
                   + raw[i] * (6.0 / 16.0))
    return hist


def orient(gauss, refined, margins: Margins | None = None):
    """Refined candidates -> keypoints in canonical order, one per orientation peak:
    (kf float32 (n, 5): x, y, size, angle, response, not yet halved; ki int32 (n, 2): octave,
    layer; src int (n,): the candidate each came from)."""
    m = margins or Margins()
    kf, ki, src = [], [], []
    n = ORI_BINS
    for idx, k in enumerate(refined):
        if k is None:
            continue
        o = k["octave"]
        scl = float(k["size"]) * 0.5 / float(1 << o)
        m.note_round(ORI_RADIUS * scl, "orientation radius")
        hist = orientation_hist(gauss[o][k["layer"]], k["c"], k["r"], cv_round(ORI_RADIUS * scl),
                                ORI_SIG * scl, m)
        thr = float(hist.max()) * ORI_PEAK
        for j in range(n):
            left, right = hist[(j - 1) % n], hist[(j + 1) % n]
            if hist[j] > 0:
                m.note(hist[j], left, "orientation peak")
                m.note(hist[j], right, "orientation peak")
                if hist[j] > left and hist[j] > right:
                    m.note(hist[j], thr, "orientation peak ratio") if hist[j] != hist.max() else None
            if hist[j] > left and hist[j] > right and hist[j] >= thr:
                b = j + 0.5 * (left - right) / (left - 2.0 * hist[j] + right)
                b = n + b if b < 0 else b - n if b >= n else b
                angle = np.float32(360.0 - (360.0 / n) * b)
                if abs(float(angle) - 360.0) < FLT_EPSILON:
                    angle = np.float32(0.0)
                kf.append((k["x"], k["y"], k["size"], angle, k["response"]))
                ki.append((o, k["layer"]))
                src.append(idx)
    return (np.array(kf, dtype=np.float32).reshape(-1, 5),
            np.array(ki, dtype=np.int32).reshape(-1, 2), np.array(src, dtype=np.int64))


# ---- step 7: duplicates, selection, halving -------------------------------------------------------

def select(kf: np.ndarray, ki: np.ndarray, num_keypoints: int):
    """Drop keypoints equal in (pt, size, angle) to an earlier one, keep those whose response is
    at least the num_keypoints-th largest (ties kept), order by response descending then canonical
    order, and halve pt and size. Returns (kf, ki, order): order indexes the input rows."""
    n = len(kf)
    alive = np.ones(n, bool)
    seen = set()
    for i in range(n):
        key = kf[i, :4].tobytes()
        if key in seen:
            alive[i] = False
        seen.add(key)
    idx = np.nonzero(alive)[0]
    resp = kf[idx, 4]
    order = idx[np.argsort(-resp.astype(np.float64), kind="stable")]
    if len(order) > num_keypoints > 0:
        thr = kf[order[num_keypoints - 1], 4]
        order = order[kf[order, 4] >= thr]
    elif num_keypoints <= 0:
        order = order[:0]
    out = kf[order].copy()
    out[:, :3] *= np.float32(0.5)
    return out, ki[order].copy(), order


# ---- step 8: descriptors ----------------------------------------------------------------------------

def descriptor(img: np.ndarray, x: float, y: float, ori: float, scl: float,
               margins: Margins | None = None) -> np.ndarray:
    """OpenCV's calcSIFTDescriptor on one Gaussian level: (x, y) in the level's pixels, ori in
    degrees, scl = size / 2 in the level's pixels -> 128 values in 0..255."""
    m = margins or Margins()
    d, n = D_WIDTH, D_BINS
    h, w = img.shape
    img = img.astype(np.float64)
    m.note_round(x, "descriptor centre")
    m.note_round(y, "descriptor centre")
    px, py = cv_round(x), cv_round(y)
    cos_t, sin_t = math.cos(ori * RAD), math.sin(ori * RAD)
    bins_per_deg = n / 360.0
    exp_scale = -1.0 / (d * d * 0.5)
    hist_width = D_SCALE * scl
    rad = hist_width * 1.4142135623730951 * (d + 1) * 0.5
    m.note_round(rad, "descriptor radius")
    radius = min(cv_round(rad), int(math.sqrt(float(h) * h + float(w) * w)))
    cos_t /= hist_width
    sin_t /= hist_width
    ii, jj = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1),
                         indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()  # raster order
    c_rot = jj * cos_t - ii * sin_t
    r_rot = jj * sin_t + ii * cos_t
    rbin = r_rot + d // 2 - 0.5
    cbin = c_rot + d // 2 - 0.5
    r, c = py + ii, px + jj
    keep = ((rbin > -1) & (rbin < d) & (cbin > -1) & (cbin < d) & (r > 0) & (r < h - 1) & (c > 0)
            & (c < w - 1))
    rbin, cbin, r, c, c_rot, r_rot = rbin[keep], cbin[keep], r[keep], c[keep], c_rot[keep], r_rot[keep]
    dx = img[r, c + 1] - img[r, c - 1]
    dy = img[r - 1, c] - img[r + 1, c]
    wgt = np.exp((c_rot * c_rot + r_rot * r_rot) * exp_scale)
    a = np.arctan2(dy, dx) * DEG
    a = np.where(a < 0, a + 360.0, a)
    mag = np.sqrt(dx * dx + dy * dy) * wgt
    obin = (a - ori) * bins_per_deg
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
    rbin, cbin, obin = rbin - r0, cbin - c0, obin - o0
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
    o0 = np.where(o0 < 0, o0 + n, o0)
    o0 = np.where(o0 >= n, o0 - n, o0)
    v_r1 = mag * rbin
    v_r0 = mag - v_r1
    v_rc11 = v_r1 * cbin
    v_rc10 = v_r1 - v_rc11
    v_rc01 = v_r0 * cbin
    v_rc00 = v_r0 - v_rc01
    v111 = v_rc11 * obin
    v110 = v_rc11 - v111
    v101 = v_rc10 * obin
    v100 = v_rc10 - v101
    v011 = v_rc01 * obin
    v010 = v_rc01 - v011
    v001 = v_rc00 * obin
    v000 = v_rc00 - v001
    base = ((r0 + 1) * (d + 2) + c0 + 1) * (n + 2) + o0
    row, col = (d + 2) * (n + 2), n + 2
    idx = np.stack([base, base + 1, base + col, base + col + 1, base + row, base + row + 1,
                    base + row + col, base + row + col + 1], axis=1)
    val = np.stack([v000, v001, v010, v011, v100, v101, v110, v111], axis=1)
    hist = np.zeros((d + 2) * (d + 2) * (n + 2))
    np.add.at(hist, idx.ravel(), val.ravel())  # sample by sample, the eight corners in order
    hist = hist.reshape(d + 2, d + 2, n + 2)
    hist[:, :, 0] += hist[:, :, n]
    hist[:, :, 1] += hist[:, :, n + 1]
    dst = hist[1:d + 1, 1:d + 1, :n].reshape(-1)
    nrm2 = 0.0
    for v in dst:
        nrm2 += v * v
    thr = math.sqrt(nrm2) * D_CLAMP
    dst = np.minimum(dst, thr)
    nrm2 = 0.0
    for v in dst:
        nrm2 += v * v
    scale = D_FACTOR / max(math.sqrt(nrm2), FLT_EPSILON)
    return np.clip(np.rint(dst * scale), 0, 255).astype(np.float32)


def descriptors(gauss, kf: np.ndarray, ki: np.ndarray, margins: Margins | None = None):
    """Selected keypoints (halved kf, ki) -> float32 (n, 128)."""
    out = np.zeros((len(kf), D_WIDTH * D_WIDTH * D_BINS), dtype=np.float32)
    for i in range(len(kf)):
        o, layer = int(ki[i, 0]), int(ki[i, 1])
        # the halved fp32 values doubled and scaled by the octave: exact powers of two
        s = 2.0 / float(1 << o)
        angle = 360.0 - float(kf[i, 3])
        if abs(angle - 360.0) < FLT_EPSILON:
            angle = 0.0
        out[i] = descriptor(gauss[o][layer], float(kf[i, 0]) * s, float(kf[i, 1]) * s, angle,
                            float(kf[i, 2]) * s * 0.5, margins)
    return out


# ---- the chain ----------------------------------------------------------------------------------

def keypoints(gauss, dog, sigma: float, num_keypoints: int, margins: Margins | None = None,
              cand: np.ndarray | None = None):
    """Steps 4-7 on an fp32 pyramid -> (kf, ki) as `select` gives them."""
    if cand is None:
        cand = candidates(dog)
    kf, ki, _ = orient(gauss, refine(dog, cand, sigma, margins), margins)
    kf, ki, _ = select(kf, ki, num_keypoints)
    return kf, ki


def extract(image: np.ndarray, num_keypoints: int, sigma: float):
    """uint8 image -> dict(x (n, 128) fp32, pos (n, 2) fp64, score (n,) fp64, kf, ki, margin,
    margin_where, survivors: refined keypoints per octave before orientation, two_peaks: whether
    a candidate gave more than one keypoint)."""
    m = Margins()
    g64, d64 = pyramid(gray(image), sigma)
    gauss, dog = to_f32(g64), to_f32(d64)
    cand = candidates(dog)
    refined = refine(dog, cand, sigma, m)
    kf0, ki0, src = orient(gauss, refined, m)
    kf, ki, _ = select(kf0, ki0, num_keypoints)
    x = descriptors(gauss, kf, ki, m)
    survivors = np.bincount([k["octave"] for k in refined if k is not None],
                            minlength=len(gauss))
    return dict(x=x, pos=kf[:, :2].astype(np.float64), score=kf[:, 4].astype(np.float64), kf=kf,
                ki=ki, margin=m.smallest, margin_where=m.where, candidates=len(cand),
                survivors=survivors, two_peaks=bool(len(src) > len(set(src.tolist()))))
