"""CPU oracle for the UniPose / UniPose-LSTM forward+backward hot path.

TEST INFRASTRUCTURE ONLY.  Nothing under ``unipose_amd/`` may import this
module; only ``tests/``, ``__graft_entry__.smoke()`` and the ``cpu_baseline``
leg of ``bench.py`` use it, and only as the checker / baseline.

It is a functional restatement (plain ``torch.nn.functional`` calls on CPU
tensors, driven by a flat ``state_dict``) of the network the reference builds
out of ``nn.Module`` objects.  Each function cites the reference lines it
follows (paths relative to /root/reference).

Parity pin: ``tools/make_goldens.py`` imports the genuine reference ``model/``
package (possible only in the development container) and stores its outputs
under ``tests/golden/``; ``tests/test_oracle_golden.py`` checks this file
against those vectors.  The arithmetic itself lives in PyTorch (un-pinned in
the reference; 2.10.0 here): conv2d / batch_norm / max_pool2d / interpolate.
"""
from __future__ import annotations

import zlib
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

SD = Dict[str, torch.Tensor]

BN_EPS = 1e-5       # nn.BatchNorm2d default; the reference never overrides it
BN_MOMENTUM = 0.1


# --------------------------------------------------------------------------
# building blocks
# --------------------------------------------------------------------------
_RELU_MASKS = None      # iterator over externally supplied ReLU outputs (NHWC), see relu_masks_from()


class relu_masks_from:
    """Context manager for flip-free gradient comparisons.  ReLU is discontinuous: an activation within
    fp32 round-off of zero can land on either side in two otherwise equivalent implementations, and one
    flipped element changes a small-batch gradient by percents.  Inside this context every ReLU of the
    oracle uses the sign pattern of the corresponding ReLU OUTPUT recorded by the implementation under
    test (same call order, NHWC tensors), so both sides differentiate the same piecewise-linear function.
    The forward values are compared separately, without masks."""

    def __init__(self, outputs_nhwc):
        self.outs = list(outputs_nhwc)

    def __enter__(self):
        global _RELU_MASKS
        _RELU_MASKS = iter(self.outs)
        return self

    def __exit__(self, *a):
        global _RELU_MASKS
        left = sum(1 for _ in _RELU_MASKS)
        _RELU_MASKS = None
        if a[0] is None and left:
            raise AssertionError(f"{left} recorded ReLU outputs were not consumed: call order mismatch")


_RELU_RECORD = None     # list collecting the oracle's own ReLU PRE-activations (NCHW), see relu_record()


class relu_record:
    """Collect the pre-activation of every ReLU the oracle evaluates, in call order (NCHW tensors, detached): lets a test
    state HOW the sign patterns of the implementation under test differ from the oracle's own — how many elements, and
    that each of them sits within round-off of zero — instead of only replaying them (relu_masks_from)."""

    def __init__(self):
        self.pre = []

    def __enter__(self):
        global _RELU_RECORD
        _RELU_RECORD = self.pre
        return self

    def __exit__(self, *a):
        global _RELU_RECORD
        _RELU_RECORD = None


def _relu(x):
    if _RELU_RECORD is not None:
        _RELU_RECORD.append(x.detach())
    if _RELU_MASKS is None:
        return F.relu(x)
    z = next(_RELU_MASKS)
    m = (z[..., :x.shape[1]].permute(0, 3, 1, 2) > 0).to(x.dtype)
    assert m.shape == x.shape, (m.shape, x.shape)
    return x * m


def _bn(sd: SD, p: str, x, train: bool):
    """nn.BatchNorm2d as used at every bnX site (resnet.py:11,14,16,62)."""
    if train:
        nbt = sd.get(p + ".num_batches_tracked")
        if nbt is not None:
            nbt += 1
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"],
                        sd[p + ".weight"], sd[p + ".bias"],
                        training=train, momentum=BN_MOMENTUM, eps=BN_EPS)


def bottleneck(sd: SD, p: str, x, stride: int, dil: int, train: bool):
    """Bottleneck.forward, resnet.py:22-42 (ctor :8-20)."""
    y = _relu(_bn(sd, p + ".bn1", F.conv2d(x, sd[p + ".conv1.weight"]), train))
    y = F.conv2d(y, sd[p + ".conv2.weight"], stride=stride, padding=dil, dilation=dil)
    y = _relu(_bn(sd, p + ".bn2", y, train))
    y = _bn(sd, p + ".bn3", F.conv2d(y, sd[p + ".conv3.weight"]), train)
    if (p + ".downsample.0.weight") in sd:
        x = F.conv2d(x, sd[p + ".downsample.0.weight"], stride=stride)
        x = _bn(sd, p + ".downsample.1", x, train)
    return _relu(y + x)


# (blocks, stride of first block, per-block dilation) for output_stride 16:
# resnet.py:49-53 (strides [1,2,2,1], dilations [1,1,1,2]), :67-70, MG unit :94-111
_LAYERS_OS16 = (
    ("layer1", 3, 1, (1, 1, 1)),
    ("layer2", 4, 2, (1, 1, 1, 1)),
    ("layer3", 23, 2, (1,) * 23),
    ("layer4", 3, 1, (2, 4, 8)),
)


# output_stride 8: resnet.py:54-56 (strides [1,2,1,1], dilations [1,1,2,4]): layer3 keeps the 1/8 resolution at dilation 2,
# the multi-grid unit runs at dilation 4 x [1,2,4]
_LAYERS_OS8 = (
    ("layer1", 3, 1, (1, 1, 1)),
    ("layer2", 4, 2, (1, 1, 1, 1)),
    ("layer3", 23, 1, (2,) * 23),
    ("layer4", 3, 1, (4, 8, 16)),
)
# WASP dilations: wasp.py:39-44 ([24,18,12,6] at output stride 16, [48,36,24,12] at 8)
_WASP_DIL = {16: (24, 18, 12, 6), 8: (48, 36, 24, 12)}


def _layers(output_stride: int):
    if output_stride == 16:
        return _LAYERS_OS16
    if output_stride == 8:
        return _LAYERS_OS8
    raise NotImplementedError      # resnet.py:57-58


def backbone(sd: SD, x, train: bool, taps: Optional[dict] = None, prefix="backbone", output_stride: int = 16):
    """ResNet.forward, resnet.py:113-124."""
    x = F.conv2d(x, sd[prefix + ".conv1.weight"], stride=2, padding=3)
    x = _relu(_bn(sd, prefix + ".bn1", x, train))
    x = F.max_pool2d(x, 3, 2, 1)
    if taps is not None:
        taps["stem"] = x
    low = None
    for name, n, stride, dils in _layers(output_stride):
        for i in range(n):
            x = bottleneck(sd, f"{prefix}.{name}.{i}", x, stride if i == 0 else 1, dils[i], train)
        if name == "layer1":
            low = x
        if taps is not None:
            taps[name] = x
    return x, low


def _atrous(sd: SD, p: str, x, dil: int, k: int, train: bool):
    """_AtrousModule.forward, wasp.py:16-20."""
    pad = 0 if k == 1 else dil
    y = F.conv2d(x, sd[p + ".atrous_conv.weight"], padding=pad, dilation=dil)
    return _relu(_bn(sd, p + ".bn", y, train))


def wasp(sd: SD, x, train: bool, drop_masks: Optional[dict] = None,
         video: bool = False, taps: Optional[dict] = None, p_drop: float = 0.5, output_stride: int = 16):
    """wasp.forward, wasp.py:66-90 (video variant waspVideo.py:56-59: GAP branch has no BN)."""
    d1, d2, d3, d4 = _WASP_DIL[output_stride]
    x1 = _atrous(sd, "wasp.aspp1", x, d1, 1, train)
    x2 = _atrous(sd, "wasp.aspp2", x1, d2, 3, train)
    x3 = _atrous(sd, "wasp.aspp3", x2, d3, 3, train)
    x4 = _atrous(sd, "wasp.aspp4", x3, d4, 3, train)
    if taps is not None:
        taps.update(x1=x1, x2=x2, x3=x3, x4=x4)
    w2 = sd["wasp.conv2.weight"]
    xs = [F.conv2d(F.conv2d(t, w2), w2) for t in (x1, x2, x3, x4)]   # wasp.py:72-80
    g = F.adaptive_avg_pool2d(x, 1)
    g = F.conv2d(g, sd["wasp.global_avg_pool.1.weight"])
    if not video:
        g = _bn(sd, "wasp.global_avg_pool.2", g, train)
    g = _relu(g)
    g = F.interpolate(g, size=x4.shape[2:], mode="bilinear", align_corners=True)
    y = torch.cat(xs + [g], dim=1)
    y = _relu(_bn(sd, "wasp.bn1", F.conv2d(y, sd["wasp.conv1.weight"]), train))
    return _dropout(y, p_drop, train, drop_masks, "wasp")


def _dropout(x, p: float, train: bool, masks: Optional[dict], key: str):
    """nn.Dropout with an injectable keep-mask (masks[key] in {0,1}); masks=None, p>0
    and train=True falls back to torch's RNG like the reference does."""
    if not train or p == 0.0:
        return x
    if masks is not None and key in masks:
        return x * masks[key] / (1.0 - p)
    return F.dropout(x, p, True)


def decoder(sd: SD, x, low, train: bool, drop_masks: Optional[dict] = None,
            taps: Optional[dict] = None, p_drop=(0.5, 0.1)):
    """Decoder.forward, decoder.py:38-56."""
    low = _relu(_bn(sd, "decoder.bn1", F.conv2d(low, sd["decoder.conv1.weight"]), train))
    low = F.max_pool2d(low, 3, 2, 1)
    x = F.interpolate(x, size=low.shape[2:], mode="bilinear", align_corners=True)
    x = torch.cat((x, low), dim=1)
    x = F.conv2d(x, sd["decoder.last_conv.0.weight"], padding=1)
    x = _relu(_bn(sd, "decoder.last_conv.1", x, train))
    x = _dropout(x, p_drop[0], train, drop_masks, "dec0")
    x = F.conv2d(x, sd["decoder.last_conv.4.weight"], padding=1)
    x = _relu(_bn(sd, "decoder.last_conv.5", x, train))
    x = _dropout(x, p_drop[1], train, drop_masks, "dec1")
    if taps is not None:
        taps["dec_pre"] = x
    return F.conv2d(x, sd["decoder.last_conv.8.weight"], sd["decoder.last_conv.8.bias"])


def unipose_forward(sd: SD, x, train: bool = False, stride: int = 8,
                    drop_masks: Optional[dict] = None, taps: Optional[dict] = None,
                    p_drop=(0.5, 0.5, 0.1), output_stride: int = 16):
    """unipose.forward, model/unipose.py:27-38 (output_stride: ctor argument, model/unipose.py:9-25)."""
    if train and x.shape[0] == 1:
        raise ValueError("Expected more than 1 value per channel when training")  # wasp.py:51-54
    f, low = backbone(sd, x, train, taps, output_stride=output_stride)
    f = wasp(sd, f, train, drop_masks, False, taps, p_drop[0], output_stride=output_stride)
    if taps is not None:
        taps["wasp"] = f
    y = decoder(sd, f, low, train, drop_masks, taps, p_drop[1:])
    if stride != 8:
        y = F.interpolate(y, size=x.shape[2:], mode="bilinear", align_corners=True)
    return y


# --------------------------------------------------------------------------
# UniPose-LSTM
# --------------------------------------------------------------------------
def lstm0_cell(sd: SD, z):
    """LSTM_0.forward, model/uniposeLSTM.py:16-24 (cell = tanh(g*i), no forget gate)."""
    def c(n):
        return F.conv2d(z, sd[f"lstm_0.conv_{n}_lstm.weight"], sd[f"lstm_0.conv_{n}_lstm.bias"], padding=1)
    g, i, o = torch.tanh(c("g")), torch.sigmoid(c("i")), torch.sigmoid(c("o"))
    cell = torch.tanh(g * i)
    return cell, o * cell


def lstm_cell(sd: SD, z, h, c_prev):
    """LSTM.forward, model/uniposeLSTM.py:40-64."""
    def s(n):
        return (F.conv2d(z, sd[f"lstm.conv_{n}x_lstm.weight"], sd[f"lstm.conv_{n}x_lstm.bias"], padding=1)
                + F.conv2d(h, sd[f"lstm.conv_{n}h_lstm.weight"], sd[f"lstm.conv_{n}h_lstm.bias"], padding=1))
    g, o, i, f = torch.tanh(s("g")), torch.sigmoid(s("o")), torch.sigmoid(s("i")), torch.sigmoid(s("f"))
    cell = f * c_prev + i * g
    return cell, o * torch.tanh(cell)


def lstm_head(sd: SD, hide):
    """conv1..conv5 with ReLU after each, model/uniposeLSTM.py:120-124."""
    y = hide
    for n, pad in (("conv1", 5), ("conv2", 5), ("conv3", 5), ("conv4", 0), ("conv5", 0)):
        y = _relu(F.conv2d(y, sd[n + ".weight"], sd[n + ".bias"], padding=pad))
    return y


def unipose_lstm_forward(sd: SD, frames, centermap, it: int, prev_hide, prev_cell,
                         train: bool = False, drop_masks: Optional[dict] = None, p_drop=(0.5, 0.5, 0.1)):
    """uniposeLSTM.unipose.forward, model/uniposeLSTM.py:98-147, with the state generalised
    from the hard-wired batch 1 (:99-104) to (B,15,H/8,W/8).  `previous` is unused there.
    p_drop: the three dropout rates (waspVideo.py:48, decoder.py:24,28), like unipose_forward's — (0, 0, 0) for comparisons
    with a model whose dropouts are switched off (round 4: the training comparisons of the video model passed the default
    rates with no masks before, i.e. compared against an oracle that dropped activations at random)."""
    x = frames[:, it]
    f, low = backbone(sd, x, train)
    f = wasp(sd, f, train, drop_masks, video=True, p_drop=p_drop[0])
    y = decoder(sd, f, low, train, drop_masks, p_drop=p_drop[1:])
    c = F.avg_pool2d(centermap[:, it], 9, 8, 1)
    z = torch.cat((y, c), dim=1)
    if it == 0:
        cell, hide = lstm0_cell(sd, z)
    else:
        if prev_hide.dim() == 3:
            prev_hide, prev_cell = prev_hide[None], prev_cell[None]
        cell, hide = lstm_cell(sd, z, prev_hide, prev_cell)
    return lstm_head(sd, hide), cell, hide


# --------------------------------------------------------------------------
# heat-map argmax (numpy, like the reference)
# --------------------------------------------------------------------------
def get_max_preds(hm: np.ndarray):
    """utils/evaluate.py:32-54: first-max flat argmax per (n, joint); x = idx % W,
    y = floor(idx / W); both zeroed where max <= 0."""
    b, j, h, w = hm.shape
    flat = hm.reshape(b, j, -1)
    idx = flat.argmax(2)
    mx = flat.max(2)
    preds = np.stack((idx % w, idx // w), axis=2).astype(np.float32)
    preds *= (mx > 0.0)[:, :, None].astype(np.float32)
    return preds, mx[:, :, None]


def gaussian_kernel(size_w, size_h, center_x, center_y, sigma):
    """utils/utils.py:200-203 (`guassian_kernel`): exp(-D2 / 2 / sigma^2) on the integer pixel grid, float64."""
    ys, xs = np.mgrid[0:size_h, 0:size_w]
    return np.exp(-((xs - center_x) ** 2 + (ys - center_y) ** 2) / 2.0 / sigma / sigma)


def _clip_map(m):
    m = m.copy()
    m[m > 1] = 1
    m[m < 0.0099] = 0
    return m


def make_heatmap(kpt, height, width, stride, sigma):
    """lsp_lspet_data.py:224-236 (same in mpii_data.py:165-175): (K,2) pixel keypoints -> (K+1, h, w) float32 with
    h = int(height/stride); joint centres int(coordinate) * 1.0 / stride; channel 0 = 1 - max of the joint channels."""
    h, w = int(height / stride), int(width / stride)
    out = np.zeros((len(kpt) + 1, h, w), dtype=np.float32)
    for i, (kx, ky) in enumerate(kpt):
        out[i + 1] = _clip_map(gaussian_kernel(w, h, int(kx) * 1.0 / stride, int(ky) * 1.0 / stride, sigma))
    out[0] = 1.0 - np.max(out[1:], axis=0)
    return out


def make_centermap(center, height, width, sigma=3):
    """lsp_lspet_data.py:238-242: (1, height, width) float32 Gaussian around `center`."""
    return _clip_map(gaussian_kernel(width, height, center[0], center[1], sigma)).astype(np.float32)[None]


# joints the reference measures head length / torso size on, per dataset (utils/evaluate.py:92-107, 127-153)
DATASETS = ("LSP", "COCO", "Penn_Action", "NTID", "PoseTrack", "BBC", "MPII")


def _head_and_torso(t0: np.ndarray, dataset: str):
    """Head length (PCKh scale) and torso size (PCK scale) from the TARGET joints of sample 0 only
    (utils/evaluate.py:92-107 and :127-153).  All arithmetic stays float32 like the reference's
    np.linalg.norm on float32 coordinates."""
    n2 = lambda v: np.linalg.norm(np.asarray(v, dtype=np.float32))
    mid = lambda a, b: (t0[a] + t0[b]) / np.float32(2)
    if dataset == "LSP":
        return n2(t0[14] - t0[13]), n2(t0[13] - mid(3, 4))
    if dataset == "COCO":
        return n2(t0[4] - t0[5]), n2(t0[13] - mid(12, 13))
    if dataset == "Penn_Action":
        return n2(t0[0] - mid(1, 2)), n2(mid(1, 2) - mid(7, 8))
    if dataset == "NTID":
        return np.float32(2) * n2(t0[4] - t0[3]), n2(t0[3] - t0[1])
    if dataset == "PoseTrack":
        return np.float32(2) * n2(t0[1] - t0[2]), n2(mid(12, 13) - mid(6, 7))
    if dataset == "BBC":
        return n2(t0[1] - mid(6, 7)), n2(np.float32(3) * (t0[1, 0] - mid(6, 7)))
    if dataset == "MPII":
        return n2(t0[9] - t0[10]), n2(t0[7, 0] - t0[8, 0])
    raise ValueError(f"unknown dataset {dataset!r}")


def accuracy(output: np.ndarray, target: np.ndarray, thr_pck: float, thr_pckh: float, dataset: str, swap_norm: bool = False):
    """utils/evaluate.py:58-172 `accuracy(..., hm_type='gaussian')` restated with masks instead of loops:
    joints from the argmax of both heat-map stacks; distance of prediction and target after dividing x by H/10 and
    y by W/10 (:68-70, the reference's own order); a joint counts for a sample when both target coordinates exceed
    1 (:12); per-joint fraction below 0.5 / thr_pckh*head / thr_pck*torso (:22-29); entry 0 of each result is
    replaced by the mean over the joints that had any valid sample (:75-90, :110-123, :155-170).
    Returns (acc, PCK, PCKh, cnt, pred, visible) like the reference.  swap_norm=True is NOT the reference: it divides x by
    W/10 and y by H/10, so that the generator of the rectangular fixture (G18) can prove its inputs tell the two orders apart."""
    pred, _ = get_max_preds(output)
    tgt, _ = get_max_preds(target)
    b, j = pred.shape[:2]
    h, w = output.shape[2], output.shape[3]
    norm = np.ones((b, 2)) * np.array([w, h] if swap_norm else [h, w]) / 10                      # float64, as in the reference
    diff = pred.astype(np.float32) / norm[:, None, :] - tgt.astype(np.float32) / norm[:, None, :]
    dist = np.stack([[np.linalg.norm(diff[n, c]) for n in range(b)] for c in range(j)])      # (J, B) float64
    valid = ((tgt[:, :, 0] > 1) & (tgt[:, :, 1] > 1)).T                  # (J, B)
    nvalid = valid.sum(1)
    head, torso = _head_and_torso(tgt[0], dataset)

    def per_joint(threshold):
        below = (np.less(dist, threshold) & valid).sum(1)
        return np.where(nvalid > 0, below * 1.0 / np.maximum(nvalid, 1), -1.0)

    acc = per_joint(0.5)
    visible = (acc >= 0).astype(np.float64)
    cnt = int(visible.sum())
    out = []
    for frac in (acc, per_joint(thr_pck * torso), per_joint(thr_pckh * head)):
        total = 0
        for v in frac:                                                  # same summation order as the reference
            if v >= 0:
                total = total + v
        res = np.where(frac >= 0, frac, 0.0)
        if cnt != 0:
            res[0] = total / cnt
        out.append(res)
    return out[0], out[1], out[2], cnt, pred, visible


# first box channel (centre; then top-left, bottom-left, top-right, bottom-right) per dataset (utils/uniPose.py:20-49)
BOX_CHANNEL0 = {"LSP": 15, "MPII": 17, "PoseTrack": 18, "NTID": 20, "NTID_small": 20}


def local_peaks(m: np.ndarray):
    """utils/uniPose.py:52-70 for one map: negatives -> 0, `maximum_filter(3x3) == map` XOR the eroded zero background.
    scipy reflects the border for the maximum and counts it as background for the erosion, so both reduce to the
    in-bounds neighbours: a pixel is kept iff it is > 0 and >= each in-bounds neighbour.  Returns [[row, col], ...] in
    row-major order like the reference's double loop."""
    c = np.where(m < 0, 0, m).astype(m.dtype)
    h, w = c.shape
    pad = np.full((h + 2, w + 2), -np.inf, dtype=c.dtype)
    pad[1:-1, 1:-1] = c
    nb = np.max(np.stack([pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]), axis=0)
    keep = (c > 0) & (c == nb)
    return [[int(i), int(j)] for i, j in np.argwhere(keep)]


def unipose_kpts_multi(maps: np.ndarray, dataset: str):
    """utils/uniPose.py:14-200 `uniPose_kpts`: maps (1, C, H, W) with the box head's five extra channels.  For every
    centre peak idx: the 14 joint channels 1..14 (hard-wired `box[1:15]`, :161) are arg-maxed inside the box spanned by the
    idx-th top-left and bottom-right peaks; returns [[idx, x, y], ...] (14 joints, centre, four corners per person).
    Raises like the reference: IndexError when a corner list is shorter than the centre list, ValueError for an empty box."""
    if dataset not in BOX_CHANNEL0:
        raise ValueError(f"no box channels defined for dataset {dataset!r}")
    mapping = np.asarray(maps)[0]
    f = BOX_CHANNEL0[dataset]
    center, tl, bl, tr, br = (local_peaks(mapping[f + i]) for i in range(5))
    kpts = []
    for idx in range(len(center)):
        box = mapping[:, tl[idx][0]:br[idx][0], tl[idx][1]:br[idx][1]]
        for m in box[1:15]:
            h, w = np.unravel_index(m.argmax(), m.shape)
            kpts.append([idx, int(w + tl[idx][1]), int(h + tl[idx][0])])
        for lst in (center, tl, bl, tr, br):
            kpts.append([idx, lst[idx][1], lst[idx][0]])
    return kpts


def get_kpts(maps: np.ndarray, img_h: float = 368.0, img_w: float = 368.0):
    """utils/utils.py:94-106: per joint (channel 0 skipped), [x, y] ints in image pixels."""
    out = []
    for m in maps[0][1:]:
        r, c = np.unravel_index(m.argmax(), m.shape)
        out.append([int(c * img_w / m.shape[1]), int(r * img_h / m.shape[0])])
    return out


# --------------------------------------------------------------------------
# deterministic synthetic weights (same values here and on the GPU box)
# --------------------------------------------------------------------------
def _gen(name: str, seed: int):
    g = torch.Generator()
    g.manual_seed((zlib.crc32(name.encode()) ^ (seed * 2654435761)) & 0x7FFFFFFF)
    return g


def _conv_w(name, shape, seed, gain=1.0):
    fan_in = shape[1] * shape[2] * shape[3]
    return torch.randn(shape, generator=_gen(name, seed)) * (gain * (2.0 / fan_in) ** 0.5)


def _bn_entries(sd, p, c, seed):
    # the last BN of every residual branch gets a small gain (0.1..0.3) so that the eval-mode trunk, whose
    # running statistics are synthetic, keeps O(1)..O(10) activations through 33 residual adds instead of
    # growing geometrically (which saturates the ConvLSTM gates and makes every comparison ill-conditioned)
    lo, span = (0.1, 0.2) if p.endswith(".bn3") else (0.5, 1.0)
    sd[p + ".weight"] = lo + span * torch.rand(c, generator=_gen(p + ".weight", seed))
    sd[p + ".bias"] = 0.1 * torch.randn(c, generator=_gen(p + ".bias", seed))
    sd[p + ".running_mean"] = 0.1 * torch.randn(c, generator=_gen(p + ".rm", seed))
    sd[p + ".running_var"] = 0.5 + torch.rand(c, generator=_gen(p + ".rv", seed))
    sd[p + ".num_batches_tracked"] = torch.zeros((), dtype=torch.long)


_SD_CACHE: "collections.OrderedDict" = __import__("collections").OrderedDict()


def synth_state_dict(num_classes: int, seed: int = 0, lstm: bool = False) -> SD:
    """Every key of the reference state_dict (687 for K=14), He-scaled conv
    weights and non-trivial BN affine/running statistics, derived from (name, seed).
    The last few results are kept and handed out as fresh clones (the test suites ask for the same few dozens of times)."""
    key = (num_classes, seed, lstm, torch.get_default_dtype())
    if key not in _SD_CACHE:
        _SD_CACHE[key] = _synth_state_dict(num_classes, seed, lstm)
        while len(_SD_CACHE) > 4:
            _SD_CACHE.popitem(last=False)
    _SD_CACHE.move_to_end(key)
    return {k: v.clone() for k, v in _SD_CACHE[key].items()}


def _synth_state_dict(num_classes: int, seed: int, lstm: bool) -> SD:
    sd: SD = {}

    def conv(name, co, ci, k, bias=False, gain=1.0):
        sd[name + ".weight"] = _conv_w(name, (co, ci, k, k), seed, gain)
        if bias:
            sd[name + ".bias"] = 0.05 * torch.randn(co, generator=_gen(name + ".bias", seed))

    conv("backbone.conv1", 64, 3, 7)
    _bn_entries(sd, "backbone.bn1", 64, seed)
    inpl = 64
    for name, n, _, _ in _LAYERS_OS16:
        planes = {"layer1": 64, "layer2": 128, "layer3": 256, "layer4": 512}[name]
        for i in range(n):
            p = f"backbone.{name}.{i}"
            conv(p + ".conv1", planes, inpl if i == 0 else planes * 4, 1)
            _bn_entries(sd, p + ".bn1", planes, seed)
            conv(p + ".conv2", planes, planes, 3)
            _bn_entries(sd, p + ".bn2", planes, seed)
            conv(p + ".conv3", planes * 4, planes, 1, gain=0.5)
            _bn_entries(sd, p + ".bn3", planes * 4, seed)
            if i == 0:
                conv(p + ".downsample.0", planes * 4, inpl, 1)
                _bn_entries(sd, p + ".downsample.1", planes * 4, seed)
        inpl = planes * 4
    conv("wasp.aspp1.atrous_conv", 256, 2048, 1)
    _bn_entries(sd, "wasp.aspp1.bn", 256, seed)
    for i in (2, 3, 4):
        conv(f"wasp.aspp{i}.atrous_conv", 256, 256, 3)
        _bn_entries(sd, f"wasp.aspp{i}.bn", 256, seed)
    conv("wasp.global_avg_pool.1", 256, 2048, 1)
    if not lstm:
        _bn_entries(sd, "wasp.global_avg_pool.2", 256, seed)
    conv("wasp.conv1", 256, 1280, 1)
    conv("wasp.conv2", 256, 256, 1, gain=0.7)
    _bn_entries(sd, "wasp.bn1", 256, seed)
    conv("decoder.conv1", 48, 256, 1)
    _bn_entries(sd, "decoder.bn1", 48, seed)
    conv("decoder.conv2", 256, 2048, 1)          # defined, never used (decoder.py:20-21,43-45)
    _bn_entries(sd, "decoder.bn2", 256, seed)
    conv("decoder.last_conv.0", 256, 304, 3)
    _bn_entries(sd, "decoder.last_conv.1", 256, seed)
    conv("decoder.last_conv.4", 256, 256, 3)
    _bn_entries(sd, "decoder.last_conv.5", 256, seed)
    conv("decoder.last_conv.8", num_classes + 1, 256, 1, bias=True)
    if lstm:
        c = num_classes + 2
        for n in "gio":
            conv(f"lstm_0.conv_{n}_lstm", c, c, 3, bias=True)
        for n in "giof":
            conv(f"lstm.conv_{n}x_lstm", c, c, 3, bias=True)
            conv(f"lstm.conv_{n}h_lstm", c, c, 3, bias=True)
        conv("conv1", 128, c, 11, bias=True)
        conv("conv2", 128, 128, 11, bias=True)
        conv("conv3", 128, 128, 11, bias=True)
        conv("conv4", 128, 128, 1, bias=True)
        conv("conv5", num_classes + 1, 128, 1, bias=True)
    # state_dict ordering of the reference interleaves differently; order is irrelevant to
    # load_state_dict, which matches by key.
    return sd


def synth_input(shape, seed: int, kind: str = "randn"):
    g = torch.Generator()
    g.manual_seed(seed)
    if kind == "randn":
        return torch.randn(shape, generator=g)
    return torch.rand(shape, generator=g)


def clone_sd(sd: SD, requires_grad: bool = False) -> SD:
    out = {}
    for k, v in sd.items():
        t = v.clone()
        if requires_grad and t.is_floating_point() and "running_" not in k:
            t.requires_grad_(True)
        out[k] = t
    return out


def max_rel(a, b) -> float:
    """max|a-b| / max|b| — SURVEY §8c: relative-to-max, not elementwise."""
    a = torch.as_tensor(a, dtype=torch.float64)
    b = torch.as_tensor(b, dtype=torch.float64)
    d = (a - b).abs().max().item()
    s = b.abs().max().item()
    return d / s if s > 0 else d
