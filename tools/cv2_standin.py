"""A shape-only stand-in for the `cv2` module, this project's own code: enough for the reference's utils/Mytransforms.py to be
loaded and its POINT arithmetic to run where OpenCV is not installed (tools/make_goldens.py g20).  getRotationMatrix2D is
OpenCV's documented formula; resize, warpAffine and copyMakeBorder return zero arrays of the size OpenCV documents for the
call — no pixel is resampled, so nothing an image function returns here may be recorded as a reference result."""
import math

import numpy as np

BORDER_CONSTANT = 0
INTER_LINEAR = 1
INTER_CUBIC = 2


def getRotationMatrix2D(center, angle, scale):
    a = scale * math.cos(math.radians(angle))
    b = scale * math.sin(math.radians(angle))
    return np.array([[a, b, (1 - a) * center[0] - b * center[1]], [-b, a, b * center[0] + (1 - a) * center[1]]], dtype=np.float64)


def _like(img, h, w):
    return np.zeros((int(h), int(w)) + tuple(img.shape[2:]), dtype=img.dtype)


def resize(img, dsize, fx=0, fy=0, interpolation=INTER_LINEAR):
    if dsize and dsize[0] and dsize[1]:
        return _like(img, dsize[1], dsize[0])
    return _like(img, round(fy * img.shape[0]), round(fx * img.shape[1]))      # dsize = Size(round(fx * cols), round(fy * rows))


def warpAffine(img, m, dsize, flags=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0):
    return _like(img, dsize[1], dsize[0])


def copyMakeBorder(img, top, bottom, left, right, borderType, value=0):
    return _like(img, img.shape[0] + top + bottom, img.shape[1] + left + right)
