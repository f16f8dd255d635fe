"""Augmentation of training samples: the reference's ``Mytransforms.RandomResized``, ``RandomRotate``, ``RandomCrop`` /
``SinglePersonCrop`` and ``RandomHorizontalFlip`` (utils/Mytransforms.py, composed in utils/utils.py:231-345) as ONE affine map
per sample.  The points (key points, person centre) go through the map on the host in float64, the pixels through its exact
inverse on the device in one bilinear resample (``ops.augment_image`` -> ``up_augment_image``), so labels and pixels cannot
drift apart.

What is the reference's and what is not.  The POINT arithmetic is the reference's, with its integer quirks: the resized image
is ``round(ratio * w)`` wide (OpenCV's documented ``dsize`` rule for ``cv2.resize(img, (0, 0), fx, fy)``), a source narrower
than 64 is padded to 64 first (Mytransforms.py:64-66), the rotation is ``cv2.getRotationMatrix2D`` about ``(w / 2, h / 2)`` of
the resized image on a canvas of ``int(h |sin| + w |cos|)`` by ``int(h |cos| + w |sin|)`` with the translation re-centred
(:201-210), the crop offsets are integers drawn as ``RandomCrop.get_params`` draws them (:434-441), the mirror is
``x -> W - 1 - x`` (:510).  The PIXELS are resampled once, not three times: the reference resizes with OpenCV's half-pixel
convention (``(x + 0.5) / ratio - 0.5``), warps, then crops; here the image map is by definition the inverse of the point
map, which differs from the reference's resize by 0.5 * |1 - ratio| pixels of the resized image and spares two rounds of
interpolation blur.  Everything outside the source is the border value (128), which is also what the reference pads, warps
and crops with."""
from __future__ import annotations

import math

import numpy as np

# rows exchanged by a mirror: Mytransforms.hflip (:513, the LSP loader's), hflip_BBC (:533), hflip_NTID (:554)
SWAP_PAIRS = {
    "LSP": ((0, 5), (1, 4), (2, 3), (6, 11), (7, 10), (8, 9)),
    "BBC": ((1, 2), (3, 4), (5, 6)),
    "NTID": ((0, 5), (1, 4), (2, 3), (6, 11), (7, 10), (8, 9)),
}
MIN_WIDTH = 64                 # Mytransforms.py:64-66


def _hw(out_size):
    if isinstance(out_size, (int, np.integer)):
        return int(out_size), int(out_size)
    return int(out_size[0]), int(out_size[1])


def rotation_matrix(cx: float, cy: float, degree: float):
    """``cv2.getRotationMatrix2D((cx, cy), degree, 1.0)`` by OpenCV's documented formula: [[a, b, (1 - a) cx - b cy],
    [-b, a, b cx + (1 - a) cy]] with a = cos, b = sin of the angle (positive = counter-clockwise, origin top-left)."""
    a, b = math.cos(math.radians(degree)), math.sin(math.radians(degree))
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], dtype=np.float64)


def resize_rotate(h: int, w: int, ratio: float, degree: float):
    """The first two steps -> (2x3 float64 map from a source pixel to the rotated canvas, (canvas height, canvas width))."""
    if not (ratio > 0 and math.isfinite(ratio) and math.isfinite(degree)):
        raise ValueError(f"augment: ratio {ratio!r}, degree {degree!r}")
    w1, h1 = int(round(ratio * max(int(w), MIN_WIDTH))), int(round(ratio * int(h)))     # dsize of cv2.resize
    m = rotation_matrix(w1 / 2.0, h1 / 2.0, degree)
    cos_val, sin_val = abs(m[0, 0]), abs(m[0, 1])
    new_w, new_h = int(h1 * sin_val + w1 * cos_val), int(h1 * cos_val + w1 * sin_val)
    m[0, 2] += new_w / 2.0 - w1 / 2.0
    m[1, 2] += new_h / 2.0 - h1 / 2.0
    m[:, :2] *= ratio                                                                   # points are multiplied by ratio first
    return m, (new_h, new_w)


def invert(forward):
    """exact inverse of a 2x3 affine map (float64)"""
    f = np.asarray(forward, dtype=np.float64)
    a, b, c, d = f[0, 0], f[0, 1], f[1, 0], f[1, 1]
    det = a * d - b * c
    if not (math.isfinite(det) and det != 0):
        raise ValueError("augment: a singular map")
    lin = np.array([[d, -b], [-c, a]], dtype=np.float64) / det
    return np.concatenate([lin, -(lin @ f[:, 2:3])], axis=1)


def compose(h: int, w: int, ratio: float, degree: float, crop_left: int, crop_up: int, out_size, flip: bool):
    """-> (forward, inv), both 2x3 float64: ``forward`` takes a source pixel (x, y, 1) of an h x w image to the output of
    resize(ratio) -> rotate(degree) -> crop(crop_left, crop_up, out_size) -> hflip (if ``flip``); ``inv`` is its exact inverse,
    the map ``ops.augment_image`` wants (output pixel -> source position).  out_size: an int or (height, width)."""
    _, wo = _hw(out_size)
    m, _ = resize_rotate(h, w, ratio, degree)
    m[0, 2] -= int(crop_left)
    m[1, 2] -= int(crop_up)
    if flip:
        m[0] = -m[0]
        m[0, 2] += wo - 1
    return m, invert(m)


def crop_offsets(center, out_size, perturb=(0.5, 0.5), center_perturb_max: float = 5):
    """``RandomCrop.get_params`` (Mytransforms.py:434-441) for the two uniform(0, 1) draws ``perturb``: (offset_left, offset_up).
    perturb = (0.5, 0.5) is ``SinglePersonCrop.get_params``."""
    ho, wo = _hw(out_size)
    x_offset = int((perturb[0] - 0.5) * 2 * center_perturb_max)
    y_offset = int((perturb[1] - 0.5) * 2 * center_perturb_max)
    return int(round(center[0] + x_offset - wo / 2)), int(round(center[1] + y_offset - ho / 2))


def apply(forward, pts):
    """a 2x3 map on (..., 2) points, float64"""
    p = np.asarray(pts, dtype=np.float64)
    f = np.asarray(forward, dtype=np.float64)
    return p @ f[:, :2].T + f[:, 2]


def transform_points(kpt, center, forward, flip: bool, dataset: str):
    """Key points (K, 2) and the person centre (2,) through ``forward``, in float64 on the host -> (kpt', center').
    A joint with a negative coordinate is this project's mark of an invisible joint (``SyntheticPoseData``, the LSP
    annotations): it keeps its coordinates, as the reference's rotate / crop skip ``kpt[i][2] == 0`` and its hflip mirrors only
    ``== 1``.  With ``flip`` the rows of the dataset's left / right pairs are exchanged (invisible rows too, as in the
    reference); a dataset for which the reference has no table is refused."""
    k = np.array(kpt, dtype=np.float64)
    if k.ndim != 2 or k.shape[1] != 2:
        raise ValueError(f"transform_points: key points (K, 2), got {k.shape}")
    seen = (k >= 0).all(axis=1)
    k[seen] = apply(forward, k[seen])
    c = apply(forward, np.asarray(center, dtype=np.float64).reshape(2))
    if flip:
        if dataset not in SWAP_PAIRS:
            raise ValueError(f"augment: the reference has no left / right table for {dataset!r}; no mirror for this dataset")
        for a, b in SWAP_PAIRS[dataset]:
            k[[a, b]] = k[[b, a]]
    return k, c


class Augmenter:
    """Draws the reference's random parameters per sample and turns them into maps and transformed annotations.

    Per sample (per CLIP when the annotations carry a frame axis, so the frames stay registered for the ConvLSTM):
    ``ratio = uniform(scale_min, scale_max) / scale`` (RandomResized.get_params), ``degree = uniform(-max_degree, max_degree)``
    (RandomRotate), two ``uniform(0, 1)`` perturbations of the crop centre (RandomCrop.get_params; the crop is centred on the
    transformed person centre, of a clip's first frame) and ``flip = uniform(0, 1) < flip_prob``.  ``numpy`` Generator seeded
    with ``seed``; ``params=`` in a call replaces the draws with explicit values."""

    def __init__(self, dataset: str, scale_min: float = 0.3, scale_max: float = 1.1, max_degree: float = 40, crop=368,
                 center_perturb_max: float = 5, flip_prob: float = 0.5, seed: int = 0):
        if flip_prob > 0 and dataset not in SWAP_PAIRS:
            raise ValueError(f"augment: the reference has no left / right table for {dataset!r}; use flip_prob=0")
        if not 0 < scale_min <= scale_max:
            raise ValueError(f"augment: scales {scale_min} .. {scale_max}")
        self.dataset, self.scale_min, self.scale_max, self.max_degree = dataset, float(scale_min), float(scale_max), float(max_degree)
        self.crop, self.perturb_max, self.flip_prob = _hw(crop), center_perturb_max, float(flip_prob)
        self.rng = np.random.default_rng(seed)

    def draw(self, n: int, scale=None):
        """-> dict of arrays, one entry per sample: ratio, degree, perturb (n, 2), flip"""
        s = np.ones(n) if scale is None else np.asarray(scale, dtype=np.float64).reshape(n)
        return {"ratio": self.rng.uniform(self.scale_min, self.scale_max, n) / s,
                "degree": self.rng.uniform(-self.max_degree, self.max_degree, n),
                "perturb": self.rng.uniform(0.0, 1.0, (n, 2)),
                "flip": self.rng.uniform(0.0, 1.0, n) < self.flip_prob}

    def __call__(self, hw, kpts, center, scale=None, params=None):
        """hw: (h, w) of every source image or (n, 2) per sample; kpts (n, K, 2) or (n, T, K, 2); center (n, 2) or (n, T, 2).
        -> (inv (n, 2, 3) for ``ops.augment_image``, kpts', center' in the shapes given, forward (n, 2, 3), params)."""
        k = np.asarray(kpts, dtype=np.float64)
        c = np.asarray(center, dtype=np.float64)
        n = k.shape[0]
        if k.ndim not in (3, 4) or c.shape != k.shape[:-2] + (2,):
            raise ValueError(f"augment: key points {k.shape} with centres {c.shape}")
        sizes = np.broadcast_to(np.asarray(hw, dtype=np.int64).reshape(-1, 2), (n, 2))
        p = self.draw(n, scale) if params is None else params
        fwd, inv = np.empty((n, 2, 3)), np.empty((n, 2, 3))
        k2, c2 = np.empty_like(k), np.empty_like(c)
        for i in range(n):
            h, w = int(sizes[i, 0]), int(sizes[i, 1])
            ratio, degree, flip = float(p["ratio"][i]), float(p["degree"][i]), bool(p["flip"][i])
            pre, _ = resize_rotate(h, w, ratio, degree)
            left, up = crop_offsets(apply(pre, c[i].reshape(-1, 2)[0]), self.crop, p["perturb"][i], self.perturb_max)
            fwd[i], inv[i] = compose(h, w, ratio, degree, left, up, self.crop, flip)
            if k.ndim == 3:
                k2[i], c2[i] = transform_points(k[i], c[i], fwd[i], flip, self.dataset)
            else:
                for t in range(k.shape[1]):
                    k2[i, t], c2[i, t] = transform_points(k[i, t], c[i, t], fwd[i], flip, self.dataset)
        return inv, k2, c2, fwd, p
