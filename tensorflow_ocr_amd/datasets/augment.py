"""Training augmentation, host side: the POLICY.  The reference holds the EAST flow in datasets/icdar.py:576-615 and keeps
it disabled (`if (0)` and comments): random scale from [0.5, 1, 2, 3], crop_area (:138-199) that never cuts a text box,
background crops with probability 3/8, pad to a square, resize.  The PixelLink recipe adds rotations by multiples of 90
degrees with probability 0.2 and colour distortion.

Nothing here touches a pixel.  plan() draws the random numbers of one sample and returns what the device needs: the
inverse affine map in 16.16 fixed point and a colour matrix (one record of ocr_augment_u8_batch, include/ocr_hip.h) plus
the polygons moved through the same map.  The pixels are warped by the kernel, all images of a batch in one launch.

Coordinates.  A pixel index d names the sample at the continuous position d + 0.5; every step below is a matrix F on
continuous positions, so an index moves as d' = F(d + 0.5) - 0.5.  The kernel evaluates the inverse, source index
u = Finv(d' + 0.5) - 0.5, with the two halves folded into the constant terms.  Polygon vertices are pixel indices (the
reference rasterises them as such) and go through the forward form in float64.

NumPy only; never imports torch (the policy is testable, and usable, without a GPU)."""
import math

import numpy as np

# one record of the device table (include/ocr_hip.h: ocr_augment_desc), 112 bytes, naturally aligned
DESC_DTYPE = np.dtype([("src_off", "<i8"), ("H", "<i4"), ("W", "<i4"), ("A", "<i8", (6,)), ("col", "<f4", (3, 4))])
assert DESC_DTYPE.itemsize == 112

LUMA = (0.299, 0.587, 0.114)            # Rec.601


def crop_area(shape, polys, tags, rng, crop_background=False, max_tries=50, min_crop_side_ratio=0.1):
    """icdar.py:138-199 on coordinates alone: returns (xmin, ymin, xmax, ymax, polys, tags), the rectangle INCLUSIVE
    (the reference slices im[ymin:ymax+1, xmin:xmax+1]) and the kept polygons moved into it.  Same steps: projections
    of the rounded polygons onto padded axis arrays, two rng.choice draws per axis among the free positions, clip,
    minimum side ratio, a polygon is kept when all four vertices are inside, background mode returns the first text-free
    rectangle; the whole image with every polygon when no row or column is free or no try succeeds."""
    h, w = int(shape[0]), int(shape[1])
    pad_h, pad_w = h // 10, w // 10
    h_array = np.zeros(h + pad_h * 2, dtype=np.int32)
    w_array = np.zeros(w + pad_w * 2, dtype=np.int32)
    for poly in polys:
        poly = np.round(poly, decimals=0).astype(np.int32)
        minx, maxx = np.min(poly[:, 0]), np.max(poly[:, 0])
        w_array[minx + pad_w:maxx + pad_w] = 1
        miny, maxy = np.min(poly[:, 1]), np.max(poly[:, 1])
        h_array[miny + pad_h:maxy + pad_h] = 1
    h_axis = np.where(h_array == 0)[0]
    w_axis = np.where(w_array == 0)[0]
    whole = (0, 0, w - 1, h - 1, polys, tags)
    if len(h_axis) == 0 or len(w_axis) == 0:
        return whole
    for _ in range(max_tries):
        xx = rng.choice(w_axis, size=2)
        xmin = int(np.clip(np.min(xx) - pad_w, 0, w - 1))
        xmax = int(np.clip(np.max(xx) - pad_w, 0, w - 1))
        yy = rng.choice(h_axis, size=2)
        ymin = int(np.clip(np.min(yy) - pad_h, 0, h - 1))
        ymax = int(np.clip(np.max(yy) - pad_h, 0, h - 1))
        if xmax - xmin < min_crop_side_ratio * w or ymax - ymin < min_crop_side_ratio * h:
            continue
        if polys.shape[0] != 0:
            inside = ((polys[:, :, 0] >= xmin) & (polys[:, :, 0] <= xmax)
                      & (polys[:, :, 1] >= ymin) & (polys[:, :, 1] <= ymax))
            selected = np.where(np.sum(inside, axis=1) == 4)[0]
        else:
            selected = np.zeros(0, np.int64)
        if len(selected) == 0:
            if crop_background:
                return xmin, ymin, xmax, ymax, polys[selected], tags[selected]
            continue
        kept = polys[selected].copy()
        kept[:, :, 0] -= xmin
        kept[:, :, 1] -= ymin
        return xmin, ymin, xmax, ymax, kept, tags[selected]
    return whole


def _scale(sx, sy):
    return np.array([[sx, 0, 0], [0, sy, 0], [0, 0, 1]], np.float64)


def _shift(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)


def _rot90_matrix(S):
    """One np.rot90 step of an S x S image on continuous positions: out[i, j] = in[j, S-1-i]."""
    return np.array([[0, 1, 0], [-1, 0, S], [0, 0, 1]], np.float64)


def fixed_inverse(F):
    """The kernel's A for a forward matrix F on continuous positions: Finv with u = Finv(d + 0.5) - 0.5 folded into the
    constants, rounded to 16.16."""
    Fi = np.linalg.inv(F)
    a = np.array([Fi[0, 0], Fi[0, 1], Fi[0, 2] + 0.5 * (Fi[0, 0] + Fi[0, 1]) - 0.5,
                  Fi[1, 0], Fi[1, 1], Fi[1, 2] + 0.5 * (Fi[1, 0] + Fi[1, 1]) - 0.5], np.float64)
    return np.rint(a * 65536.0).astype(np.int64)


def rot90_fixed(A, S, k90):
    """A after k90 np.rot90 steps of the S x S output, in integers: out_k(dx, dy) = out_{k-1}(S-1-dy, dx), so the rotated
    output is an exact permutation of the unrotated one."""
    A = np.array(A, np.int64)
    for _ in range(k90 % 4):
        A = np.array([A[1], -A[0], A[2] + A[0] * (S - 1), A[4], -A[3], A[5] + A[3] * (S - 1)], np.int64)
    return A


def apply_forward(F, polys):
    """Pixel-index vertices through F: d' = F(d + 0.5) - 0.5, float64."""
    p = np.asarray(polys, np.float64).reshape(-1, 2) + 0.5
    q = p @ F[:2, :2].T + F[:2, 2]
    return (q - 0.5).reshape(-1, 4, 2)


def apply_fixed(A, pts):
    """Source positions (float64, in pixels) the fixed-point map A assigns to output positions pts [..., 2]."""
    pts = np.asarray(pts, np.float64)
    A = np.asarray(A, np.float64)
    x = (A[0] * pts[..., 0] + A[1] * pts[..., 1] + A[2]) / 65536.0
    y = (A[3] * pts[..., 0] + A[4] * pts[..., 1] + A[5]) / 65536.0
    return np.stack([x, y], axis=-1)


def colour_matrix(saturation=1.0, contrast=1.0, brightness=0.0):
    """[3,4] float32 on 0..255 values: saturation about the Rec.601 luma, then contrast about 128, then a brightness offset;
    composed in float64.  (1, 1, 0) is the identity bit for bit."""
    M = np.zeros((3, 4), np.float64)
    M[:, :3] = np.eye(3)
    if saturation != 1.0:
        M[:, :3] = saturation * np.eye(3) + (1.0 - saturation) * np.tile(np.array(LUMA, np.float64), (3, 1))
    if contrast != 1.0:
        M[:, :3] *= contrast
        M[:, 3] = 128.0 * (1.0 - contrast)
    if brightness != 0.0:
        M[:, 3] += brightness
    return M.astype(np.float32)


def pack_desc(src_offs, shapes, plans, slab_bytes):
    """The device table for a batch: src_offs[b] = byte offset of image b (uint8 [H,W,3]) in a slab of slab_bytes bytes,
    plans[b] = (A, col, ...).  Every image must lie inside the slab: the kernel trusts the table."""
    d = np.zeros(len(plans), DESC_DTYPE)
    for b, (off, shp, pl) in enumerate(zip(src_offs, shapes, plans)):
        H, W = int(shp[0]), int(shp[1])
        if len(shp) != 3 or shp[2] != 3 or H <= 0 or W <= 0 or off < 0 or off + 3 * H * W > slab_bytes:
            raise ValueError("image %d (%r at byte %d) does not lie inside the %d-byte slab" % (b, tuple(shp), off, slab_bytes))
        d[b]["src_off"], d[b]["H"], d[b]["W"] = off, H, W
        d[b]["A"] = np.asarray(pl[0], np.int64)
        d[b]["col"] = np.asarray(pl[1], np.float32)
    return d


def _num(text):
    text = text.strip()
    if "/" in text:
        a, b = text.split("/")
        return float(a) / float(b)
    return float(text)


def _flag(text):
    t = text.strip().lower()
    if t in ("1", "true", "yes", "on"):
        return True
    if t in ("0", "false", "no", "off"):
        return False
    raise ValueError("not a boolean: %r" % text)


class Augment:
    """The policy.  `log`: None, or a list the generator appends (im_fn, A, col, polys, tags) to for every sample it emits."""

    FIELDS = ("random_scale", "crop", "min_crop_side_ratio", "background_ratio", "rotate90_prob", "max_rotate_deg",
              "brightness", "contrast", "saturation")

    def __init__(self, random_scale=(0.5, 1, 2, 3), crop=True, min_crop_side_ratio=0.1, background_ratio=3 / 8,
                 rotate90_prob=0.0, max_rotate_deg=0.0, brightness=0.0, contrast=0.0, saturation=0.0):
        self.random_scale = tuple(float(s) for s in random_scale)
        if not self.random_scale or min(self.random_scale) <= 0:
            raise ValueError("random_scale needs positive factors")
        self.crop = bool(crop)
        self.min_crop_side_ratio = float(min_crop_side_ratio)
        self.background_ratio = float(background_ratio)
        self.rotate90_prob = float(rotate90_prob)
        self.max_rotate_deg = float(max_rotate_deg)
        self.brightness = float(brightness)
        self.contrast = float(contrast)
        self.saturation = float(saturation)
        for name in ("background_ratio", "rotate90_prob"):
            if not 0.0 <= getattr(self, name) <= 1.0:
                raise ValueError("%s is a probability" % name)
        for name in ("min_crop_side_ratio", "max_rotate_deg", "brightness", "contrast", "saturation"):
            if getattr(self, name) < 0:
                raise ValueError("%s must not be negative" % name)
        self.log = None

    PRESETS = {
        "east": {},
        "pixellink": dict(rotate90_prob=0.2, brightness=32 / 255, contrast=0.5, saturation=0.5),
    }

    @classmethod
    def parse(cls, text):
        """`none` -> None; `east` (the reference's disabled flow with its constants); `pixellink` (east + rotate90_prob=0.2,
        brightness=32/255, contrast=0.5, saturation=0.5); or `key=value,...` over the constructor's parameters, optionally
        after a preset name (`east,max_rotate_deg=10`).  random_scale is a `:` separated list; numbers may be fractions."""
        if text is None:
            return None
        items = [t.strip() for t in str(text).split(",") if t.strip()]
        if not items or items == ["none"]:
            return None
        kw = {}
        if "=" not in items[0]:
            if items[0] not in cls.PRESETS:
                raise ValueError("unknown augmentation preset %r (none, east, pixellink or key=value,...)" % items[0])
            kw.update(cls.PRESETS[items[0]])
            items = items[1:]
        for it in items:
            if "=" not in it:
                raise ValueError("expected key=value, got %r" % it)
            k, v = (s.strip() for s in it.split("=", 1))
            if k not in cls.FIELDS:
                raise ValueError("unknown augmentation parameter %r (one of %s)" % (k, ", ".join(cls.FIELDS)))
            if k == "random_scale":
                kw[k] = tuple(_num(s) for s in v.split(":"))
            elif k == "crop":
                kw[k] = _flag(v)
            else:
                kw[k] = _num(v)
        return cls(**kw)

    def spec(self):
        """The key=value text parse() turns back into an equal policy."""
        out = []
        for k in self.FIELDS:
            v = getattr(self, k)
            if k == "random_scale":
                out.append("%s=%s" % (k, ":".join(repr(s) for s in v)))
            elif k == "crop":
                out.append("%s=%s" % (k, "true" if v else "false"))
            else:
                out.append("%s=%r" % (k, v))
        return ",".join(out)

    def __eq__(self, other):
        return isinstance(other, Augment) and all(getattr(self, k) == getattr(other, k) for k in self.FIELDS)

    def __hash__(self):
        return hash(tuple(getattr(self, k) for k in self.FIELDS))

    def __repr__(self):
        return "Augment(%s)" % self.spec()

    def plan(self, rng, h, w, polys, tags, S):
        """One sample: image h x w, validated polygons float [k,4,2] in SOURCE pixels, tags bool [k], output S x S.
        None where the reference does `continue`; else (A int64 [6], col float32 [3,4], polys float32 [k',4,2], tags bool [k'])
        in the order of icdar.py:576-623.  All draws come from `rng` (a numpy RandomState)."""
        polys = np.asarray(polys, np.float64).reshape(-1, 4, 2)
        tags = np.asarray(tags, bool).reshape(-1)
        # 1. random scale: cv2.resize(im, dsize=None, fx=s, fy=s) makes a round(w*s) x round(h*s) image; nothing is resampled here
        s = float(rng.choice(self.random_scale))
        hs, ws = max(1, int(np.rint(h * s))), max(1, int(np.rint(w * s)))
        F = _scale(ws / float(w), hs / float(h))
        polys = apply_forward(F, polys)
        # 2. crop
        xmin, ymin, xmax, ymax = 0, 0, ws - 1, hs - 1
        if self.crop:
            background = rng.rand() < self.background_ratio
            xmin, ymin, xmax, ymax, polys, tags = crop_area((hs, ws), polys, tags, rng, crop_background=background,
                                                            min_crop_side_ratio=self.min_crop_side_ratio)
            if background and polys.shape[0] > 0:
                return None                   # "cannot find background"
            if not background and polys.shape[0] == 0:
                return None
        elif polys.shape[0] == 0:
            return None
        F = _shift(-xmin, -ymin) @ F
        # 3. pad to a square anchored top-left (zeros: taps outside the source), resize to S
        side = max(ymax - ymin + 1, xmax - xmin + 1, S)
        k = S / float(side)
        F = _scale(k, k) @ F
        polys = polys * k + (0.5 * k - 0.5)   # (d + 0.5) * k - 0.5
        # 4. / 5. rotations about the centre of the output square; they commute, and the quarter turns are applied to the
        #         integer map so that they stay an exact pixel permutation
        k90 = 0
        if self.rotate90_prob > 0 and rng.rand() < self.rotate90_prob:
            k90 = int(rng.randint(0, 4))
        if self.max_rotate_deg > 0:
            th = math.radians(float(rng.uniform(-self.max_rotate_deg, self.max_rotate_deg)))
            c, sn = math.cos(th), math.sin(th)
            R = _shift(S / 2.0, S / 2.0) @ np.array([[c, -sn, 0], [sn, c, 0], [0, 0, 1]], np.float64) @ _shift(-S / 2.0, -S / 2.0)
            F = R @ F
            polys = apply_forward(R, polys)
        A = rot90_fixed(fixed_inverse(F), S, k90)
        for _ in range(k90):
            polys = apply_forward(_rot90_matrix(S), polys)
        if self.max_rotate_deg > 0 and polys.shape[0]:
            out = (polys < 0) | (polys > S - 1)
            out = out[:, :, 0] | out[:, :, 1]
            keep = ~out.all(axis=1)           # every vertex outside: gone; some outside: don't-care (the rasteriser clips)
            tags = (tags | out.any(axis=1))[keep]
            polys = polys[keep]
        # 6. colour
        sat = float(rng.uniform(1 - self.saturation, 1 + self.saturation)) if self.saturation > 0 else 1.0
        con = float(rng.uniform(1 - self.contrast, 1 + self.contrast)) if self.contrast > 0 else 1.0
        bri = float(rng.uniform(-self.brightness, self.brightness)) * 255.0 if self.brightness > 0 else 0.0
        return A, colour_matrix(sat, con, bri), polys.astype(np.float32), tags.copy()
