"""The host side of the evaluation protocol around the forward (utils/extra_utils, vendored from pytorch-pose): the channel
permutation of the flip test and the crop transform whose inverse ``up_final_preds`` applies on the device.

``flip_perm`` gives, for every OUTPUT channel of a model (background first, joint k in channel k + 1, the five box channels of
``bbox=True`` last), the channel whose mirrored map it is merged with.  ``get_transform`` / ``inverse_maps`` restate
transforms.py:79-116 in numpy float64, including the arithmetic the reference does in float32 when ``scale`` is a float32 tensor.
"""
from __future__ import annotations

import numpy as np
import torch

# left / right joint pairs, the reference's own lists
PAIRS = {
    "MPII": ([0, 5], [1, 4], [2, 3], [10, 15], [11, 14], [12, 13]),              # extra_utils/transforms.py:27-30
    "LSP": ([0, 5], [1, 4], [2, 3], [6, 11], [7, 10], [8, 9]),                   # Mytransforms.py:513 hflip
    "NTID": ([0, 5], [1, 4], [2, 3], [6, 11], [7, 10], [8, 9]),                  # Mytransforms.py:554 hflip_NTID
    "BBC": ([1, 2], [3, 4], [5, 6]),                                             # Mytransforms.py:533 hflip_BBC
}


def flip_perm(dataset, num_classes: int, bbox: bool = False, pairs=None):
    """The channel permutation of the flip test for all num_classes + 1 (+ 5) output channels, a list of ints: channel 0
    (background) is fixed, joint k is channel k + 1 and exchanges with its left / right partner; with `bbox` the five box channels
    follow in the order centre, tl, bl, tr, br (``up_persons_decode``): centre fixed, tl <-> tr, bl <-> br.  `pairs` overrides the
    dataset's list; a dataset the reference has no list for needs it (ValueError)."""
    if pairs is None:
        if dataset not in PAIRS:
            raise ValueError(f"flip_perm: the reference has no left / right pairs for dataset {dataset!r}: pass pairs=")
        pairs = PAIRS[dataset]
    perm = list(range(num_classes + 1 + (5 if bbox else 0)))
    for a, b in pairs:
        a, b = int(a), int(b)
        if not (0 <= a < num_classes and 0 <= b < num_classes):
            raise ValueError(f"flip_perm: pair ({a}, {b}) with {num_classes} joints")
        perm[a + 1], perm[b + 1] = perm[b + 1], perm[a + 1]
    if bbox:
        f = num_classes + 1
        perm[f + 1], perm[f + 3] = f + 3, f + 1          # tl <-> tr
        perm[f + 2], perm[f + 4] = f + 4, f + 2          # bl <-> br
    return perm


def _res(res):
    if np.ndim(res) == 0:
        return [int(res), int(res)]
    return [res[0], res[1]]


def get_transform(center, scale, res, rot=0):
    """transforms.py:79-108 for one sample: the (3, 3) float64 matrix from source pixels to the res[0] x res[1] crop.  A torch
    tensor `scale` keeps the reference's arithmetic in the tensor's dtype: ``200 * scale`` is a float32 product for a float32
    tensor, and python ``float / tensor`` is ``tensor.reciprocal() * float`` there, two roundings.  Anything else is float64."""
    res = _res(res)
    c0, c1 = float(center[0]), float(center[1])
    r0, r1 = res[0], res[1]
    if isinstance(scale, torch.Tensor):
        T = np.dtype(str(scale.dtype).replace("torch.", "")).type
        h = T(200) * T(float(scale))
        inv_h = T(1) / h
        div = lambda a: inv_h * T(a)
        t00, t11 = div(float(r1)), div(float(r0))
        t02 = T(r1) * (div(-c0) + T(.5))
        t12 = T(r0) * (div(-c1) + T(.5))
    else:
        h = 200 * np.float64(scale)
        t00, t11 = float(r1) / h, float(r0) / h
        t02 = r1 * (-c0 / h + .5)
        t12 = r0 * (-c1 / h + .5)
    t = np.zeros((3, 3))
    t[0, 0], t[1, 1], t[0, 2], t[1, 2], t[2, 2] = t00, t11, t02, t12, 1
    if not rot == 0:
        rot = -rot
        rot_mat = np.zeros((3, 3))
        rot_rad = rot * np.pi / 180
        sn, cs = np.sin(rot_rad), np.cos(rot_rad)
        rot_mat[0, :2] = [cs, -sn]
        rot_mat[1, :2] = [sn, cs]
        rot_mat[2, 2] = 1
        t_mat = np.eye(3)
        t_mat[0, 2] = -r1 / 2
        t_mat[1, 2] = -r0 / 2
        t_inv = t_mat.copy()
        t_inv[:2, 2] *= -1
        t = np.dot(t_inv, np.dot(rot_mat, np.dot(t_mat, t)))
    return t


def inverse_maps(center, scale, res):
    """What ``transform(..., invert=1)`` multiplies with (transforms.py:111-116), for a batch: (B, 2, 3) float64, the first two
    rows of ``np.linalg.inv(get_transform(center[i], scale[i], res))`` — the `inv` argument of ``up_final_preds``."""
    n = len(center)
    out = np.empty((n, 2, 3), dtype=np.float64)
    for i in range(n):
        out[i] = np.linalg.inv(get_transform(center[i], scale[i], res))[:2]
    return out


def crop_maps(center, scale, res, rot=0):
    """The crop in front of the network, for a batch: (B, 6) float64, the first two rows of
    ``np.linalg.inv(get_transform(center[i], scale[i], res, rot))`` flattened — the `inv` argument of ``up_crop_to_nhwc``: it takes
    an output pixel (u, v) of the network input to its position in the source frame.  `res` = [H, W] of the network input:
    get_transform's own order, where res[1] scales x — NOT the [W, H] that ``final_preds`` (and so ``inverse_maps`` on the way
    back) wants on non-square maps; ``up_final_preds``'s header records that quirk of the reference.  No +-1 shift: the
    reference's ``transform`` maps ``pt - 1`` and adds 1, so in 0-based pixels the matrix itself is the map.  `rot` in degrees, one
    value or one per sample."""
    n = len(center)
    rots = np.broadcast_to(np.asarray(rot, dtype=np.float64), (n,))
    out = np.empty((n, 6), dtype=np.float64)
    for i in range(n):
        out[i] = np.linalg.inv(get_transform(center[i], scale[i], res, float(rots[i])))[:2].reshape(6)
    return out
