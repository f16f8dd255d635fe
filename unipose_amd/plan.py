"""``UniPosePlan`` — the image model's inference forward as ONE call into the C ABI (``up_unipose_forward``, ABI 9; at
``stride != 8`` ``up_unipose_forward_upsampled``; key points instead of heat-maps: ``up_unipose_keypoints``; the persons of the
box head: ``up_unipose_persons``).

The reference's validation / test loops run ``heat = model(input)`` per batch (unipose.py:150-160).  A plan is built once
from a model (any ``unipose`` with ``bbox`` or not, output stride 16 / 8): its BatchNorm layers are folded into the
convolutions (``checkpoint.fold_batchnorm``), the folded weights are packed into plan-owned device memory, the activation
workspace is one torch byte tensor.  ``plan(x)`` then issues the whole network from C — no autograd, no per-layer Python —
and returns the heat-maps (the two slices of ``unipose(bbox=True)`` when the model has the box head).

    model = unipose("MPII", num_classes=16).cuda().eval(); model.load_state_dict(...)
    plan = UniPosePlan(model, batch=8, height=368, width=368)
    heat = plan(images)                      # equal bits to checkpoint.load_folded(...)(images)
    preds, maxvals, idx = plan.keypoints(images)     # equal bits to ops.heatmap_argmax(heat), without the NCHW heat-maps
    kpts, count, status = plan.persons(images, "MPII")        # bbox=True models: ops.persons_decode of the maps, without them
    preds, coords, maxvals = plan.final_preds(images, center, scale, flip=True, dataset="MPII")   # flip test + pytorch-pose's final_preds
    preds, coords, maxvals = plan.frame_final_preds(frames_u8_hwc, center, scale, frame_of=[0] * 8, flip=True, dataset="MPII")   # the crop too

A model built with ``stride != 8`` (the reference's full-resolution mode, model/unipose.py:31-32) gives the heat-maps up-sampled
to the input size, as the module does; ``keypoints`` then decodes on that grid without ever writing the up-sampled maps
(``up_heatmap_decode``).

The launches are those of the drop-in module's folded forward, so the results agree bit for bit
(tests/test_plan_emu.py, tests/test_plan_gpu.py).  Weights are captured at construction: call ``refresh(model)`` after
changing them.  Inference only.

``UniPosePlan(..., storage="bf16")`` runs every method in bf16 STORAGE: the launches of the folded module under
``ops.set_conv_math("bf16s")`` — bf16 activations and weight images behind the fp32 stem, fp32 accumulation, fp32 maps out of the
last convolution — again with equal bits (tests/test_plan_bf16_*.py).  Inputs, results and ``refresh`` stay fp32; the plan neither
reads nor sets ``ops.CONV_MATH``, so plans of both storages can be alive and called in turn.

``UniPosePlan(..., flip="one_pass")`` (default ``"two_pass"``; ``plan.flip_mode`` reads it back) runs the flip test of
``flip_heatmaps``, ``final_preds(flip=True)``, ``frame_heatmaps(flip=True)`` and ``frame_final_preds(flip=True)`` as ONE trunk over
2 * batch images, the input and its mirror: a pass less, at the workspace of a forward of twice the batch.  Its identity:
``flip_heatmaps(x)`` has equal bits to ``ops.flip_merge(a, f, perm)`` with ``a, f`` the two halves of
``plan2B(torch.cat([x, x.flip(3)]))``, ``plan2B`` a two-pass plan of batch 2 * batch of the same model and storage — not to the
two-pass form, wherever a convolution picks its kernel by the number of rows.  Every other method is unchanged.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _C
from .checkpoint import fold_batchnorm


class _Config(C.Structure):
    """up_unipose_config"""
    _fields_ = [(n, C.c_int32) for n in ("batch", "height", "width", "output_stride", "out_channels")]


def _set_convs(plan, prefix, folded):
    """every convolution the plan lists, from the folded state dict (`prefix`: up_unipose_plan / up_unipose_lstm_plan)"""
    L = _C.lib()
    who = type(plan).__name__
    keep = []
    shape = (C.c_int32 * 4)()
    hb = C.c_int32()
    for i in range(getattr(L, prefix + "_num_convs")(plan._plan)):
        name = getattr(L, prefix + "_conv_name")(plan._plan, i).decode()
        _C.check(getattr(L, prefix + "_conv_shape")(plan._plan, i, shape, C.byref(hb)), prefix[3:] + "_conv_shape")
        w = folded[name + ".weight"].to(plan.device, torch.float32).contiguous()
        if tuple(w.shape) != tuple(shape):
            raise ValueError(f"{who}: {name}.weight is {tuple(w.shape)}, the plan expects {tuple(shape)}")
        b = folded.get(name + ".bias")
        if bool(hb.value) != (b is not None):
            raise ValueError(f"{who}: {name} {'needs' if hb.value else 'must not have'} a bias after folding")
        if b is not None:
            b = b.to(plan.device, torch.float32).contiguous()
        _C.check(getattr(L, prefix + "_set_conv")(plan._plan, i, w.data_ptr(), None if b is None else b.data_ptr(), plan._stream()),
                 prefix[3:] + "_set_conv")
        keep += [w, b]
    if plan.device.type == "cuda":
        torch.cuda.current_stream(plan.device).synchronize()       # the staging tensors in `keep` may go now
    del keep


def _check_out(who, name, t, shape, dev, dtype=torch.float32):
    if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{who}: `{name}` is {tuple(t.shape)} {t.dtype} on {t.device} (contiguous: {t.is_contiguous()}), "
                         f"the plan writes a contiguous {str(dtype).replace('torch.', '')} {shape} on {dev}")
    return t


class _Plan:
    """What the two plan classes share: device and stream, the aligned workspace, `out` tensors, the flip test's permutation and
    the end of the plan.  `_prefix` names the C functions of the plan; `out_channels` are the channels of its heat-maps."""
    _prefix = None
    bbox = False

    def _create(self, cfg, device, dtype=None, flip="two_pass"):
        """dtype: None for the plan's plain create entry, else the storage type code of its `_create_t` form; flip: "two_pass" or
        "one_pass" (UP_PLAN_FLIP_ONE_PASS through the `_create_ex` form)"""
        L = _C.lib()
        self.cfg, self.device, self.workspace, self.flip_mode = cfg, device, None, flip
        self._plan = C.c_void_p()
        if flip == "one_pass":
            _C.check(getattr(L, self._prefix + "_create_ex")(C.byref(cfg), dtype or 0, _C.PLAN_FLIP_ONE_PASS, C.byref(self._plan)),
                     self._prefix[3:] + "_create_ex")
        elif dtype is None:
            _C.check(getattr(L, self._prefix + "_create")(C.byref(cfg), C.byref(self._plan)), self._prefix[3:] + "_create")
        else:
            _C.check(getattr(L, self._prefix + "_create_t")(C.byref(cfg), dtype, C.byref(self._plan)), self._prefix[3:] + "_create_t")
        self._ws(getattr(L, self._prefix + "_workspace")(self._plan))

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream if self.device.type == "cuda" else 0

    def _ws(self, need=None):
        """the 256-byte aligned (pointer, bytes) of `self.workspace`, grown first where it is smaller than `need` bytes"""
        if need is not None and (self.workspace is None or self.workspace.numel() < max(need, 256) + 256):
            self.workspace = torch.empty(max(need, 256) + 256, dtype=torch.uint8, device=self.device)
        ws = self.workspace
        off = (-ws.data_ptr()) % 256
        return ws.data_ptr() + off, ws.numel() - off

    def _flip_ws(self):
        """the flip test keeps the first pass's heat-maps while the network runs again (one_pass: it runs at twice the batch): a
        larger workspace, made at the first call"""
        return self._ws(getattr(_C.lib(), self._prefix + "_flip_workspace")(self._plan))

    def _out(self, who, out, shape):
        """the caller's `out` tensor if it is what the plan writes, or a new one"""
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device)
        return _check_out(who, "out", out, shape, self.device)

    def _outs(self, who, out, names, shapes, dtypes=None, word="triple"):
        """the caller's `out` tuple if every tensor in it is what the plan writes, or new tensors"""
        dtypes = dtypes or (torch.float32,) * len(names)
        if out is None:
            return tuple(torch.empty(s, dtype=d, device=self.device) for s, d in zip(shapes, dtypes))
        if len(out) != len(names):
            raise ValueError(f"{who}: `out` is a ({', '.join(names)}) {word}")
        return tuple(_check_out(who, n, t, s, self.device, d) for n, t, s, d in zip(names, out, shapes, dtypes))

    def _perm(self, dataset, pairs):
        from . import ops, protocol
        return ops._perm_array(protocol.flip_perm(dataset, self.num_classes, self.bbox, pairs), self.out_channels)

    def _frame_ws(self, program):
        """a program from frames keeps the mirrored input through the first trunk (one_pass: it is half of the one input): its own
        need, made at the first call (`_flip_ws`)"""
        return self._ws(getattr(_C.lib(), self._prefix + "_program_workspace")(self._plan, _C.PROGRAM_FROM_FRAMES + program))

    def _frame_args(self, who, frames, center, scale, frame_of, rot, valid_hw, lead=None):
        """the arguments of up_crop_to_nhwc / up_clip_crop_to_nhwc as the entries from frames take them, and the tensors that must
        outlive the call.  lead: the samples' leading shape, (batch,) by default, (B, T) for a clip."""
        from . import protocol
        name = type(self).__name__
        lead = (self.batch,) if lead is None else tuple(lead)
        n = 1
        for d in lead:
            n *= d
        if (not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[3] != 3 or frames.device != self.device
                or frames.dtype not in (torch.uint8, torch.float32)):
            raise ValueError(f"{name}.{who}: frames (F, Hs, Ws, 3) uint8 or float32 on {self.device}, got "
                             f"{tuple(frames.shape)} {frames.dtype} on {frames.device}")
        x = frames.contiguous()
        nf, hs, ws = x.shape[:3]
        if len(lead) > 1 and center is not None and scale is not None:
            import numpy as np
            # a tensor stays one (protocol.get_transform keeps the reference's arithmetic in a tensor scale's dtype)
            c = center if isinstance(center, torch.Tensor) else np.asarray(center)
            sc = scale if isinstance(scale, torch.Tensor) else np.asarray(scale)
            if tuple(c.shape) != lead + (2,) or tuple(sc.shape) != lead:
                raise ValueError(f"{name}.{who}: center {tuple(c.shape)} / scale {tuple(sc.shape)}, one crop per frame is "
                                 f"{lead + (2,)} / {lead}")
            center, scale = c.reshape(n, 2), sc.reshape(n)
        if center is None or scale is None or len(center) != n or len(scale) != n:
            raise ValueError(f"{name}.{who}: one centre and one scale per sample of the batch of {n}")
        m = torch.from_numpy(protocol.crop_maps(center, scale, [self.height, self.width], rot)).to(self.device)
        fo = None
        if frame_of is not None:
            fo = torch.as_tensor(frame_of)
            if tuple(fo.shape) != lead:
                raise ValueError(f"{name}.{who}: frame_of {tuple(fo.shape)} for a batch of {lead}")
            fo = fo.to(device=self.device, dtype=torch.int32).contiguous()
        elif nf != n:
            raise ValueError(f"{name}.{who}: {nf} frames for a batch of {n} and no frame_of")
        valid = None
        if valid_hw is not None:
            valid = torch.as_tensor(valid_hw).to(device=self.device, dtype=torch.int32).contiguous()
            if tuple(valid.shape) != (nf, 2):
                raise ValueError(f"{name}.{who}: valid_hw {tuple(valid.shape)} for {nf} frames ((F, 2) expected)")
        args = (x.data_ptr(), 0 if x.dtype == torch.uint8 else 1, nf, hs, ws, None if fo is None else fo.data_ptr(),
                None if valid is None else valid.data_ptr(), m.data_ptr(), 128.0, 128.0, 256.0)
        return args, (x, m, fo, valid), (center, scale)

    def close(self):
        if self._plan:
            getattr(_C.lib(), self._prefix + "_destroy")(self._plan)
            self._plan = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001  (interpreter shutdown)
            pass


# storage="..." of UniPosePlan -> (what plan.storage reads back, UP_DT_* code): the names ops.set_conv_math takes for the two modes
_STORAGE = {"f32": ("f32", 0), "fp32": ("f32", 0), "bf16": ("bf16", 1), "bf16s": ("bf16", 1), "bf16_storage": ("bf16", 1)}


class UniPosePlan(_Plan):
    _prefix = "up_unipose_plan"

    def __init__(self, model, batch: int, height: int, width: int, storage: str = "f32", flip: str = "two_pass"):
        if not isinstance(flip, str) or flip not in ("two_pass", "one_pass"):
            raise ValueError(f"UniPosePlan: flip {flip!r}; 'two_pass' or 'one_pass'")
        if not isinstance(storage, str) or storage not in _STORAGE:
            raise ValueError(f"UniPosePlan: storage {storage!r}; one of {sorted(_STORAGE)}")
        self.storage, dtype = _STORAGE[storage]
        if model.training:
            raise ValueError("UniPosePlan captures the inference forward: call model.eval() first")
        if batch < 1 or height < 8 or width < 8:
            raise ValueError(f"UniPosePlan: batch {batch}, {height} x {width} input")
        self.upsampled = getattr(model, "stride", 8) != 8      # model/unipose.py:31-32: heat-maps at the input size
        w0 = model.backbone.conv1.weight
        if not w0.is_cuda and not _C._ALLOW_HOST_POINTERS:
            raise _C.UniPoseHipError("UniPosePlan needs a CUDA(HIP) model; there is no CPU fallback")
        self.bbox = bool(getattr(model, "bbox", False))
        self.num_classes = model.num_classes
        out_channels = model.decoder.last_conv[8].out_channels
        os_ = 16 if model.wasp.aspp2.atrous_conv.dilation[0] == 18 else 8
        # (the default goes through up_unipose_plan_create, as before the storage option)
        self._create(_Config(batch, height, width, os_, out_channels), w0.device, dtype if dtype else None, flip)
        self.batch, self.height, self.width, self.out_channels = batch, height, width, out_channels
        # heat-map size: three ceil-halvings (7x7 stride-2 stem, 3x3 stride-2 max-pool, layer2's stride 2), the arithmetic of
        # plan.hip's build(): ceil(H / 8), NOT H // 8 — the two differ whenever H % 8 != 0 (a 52 x 52 input gives 7 x 7 maps)
        self.map_height, self.map_width = (height - 1) // 8 + 1, (width - 1) // 8 + 1
        # what plan(x) writes: the maps themselves, or (stride != 8) the maps up-sampled to the input size
        self.out_height, self.out_width = (height, width) if self.upsampled else (self.map_height, self.map_width)
        self.refresh(model)

    def refresh(self, model):
        """(re)load the weights: BatchNorm folded in float64 and rounded once, like checkpoint.fold_batchnorm / load_folded; the
        plan packs them in its own storage type (bf16 images behind the stem in bf16 storage)"""
        _set_convs(self, "up_unipose_plan", fold_batchnorm(model))

    def _input(self, x):
        if tuple(x.shape) != (self.batch, 3, self.height, self.width) or x.dtype != torch.float32 or x.device != self.device:
            raise ValueError(f"UniPosePlan: input {tuple(x.shape)} {x.dtype} on {x.device}, planned for "
                             f"{(self.batch, 3, self.height, self.width)} float32 on {self.device}")
        return x.contiguous()

    def __call__(self, x: torch.Tensor, out: torch.Tensor = None):
        x = self._input(x)
        out = self._out("UniPosePlan", out, (self.batch, self.out_channels, self.out_height, self.out_width))
        ws, nbytes = self._ws()
        forward = _C.lib().up_unipose_forward_upsampled if self.upsampled else _C.lib().up_unipose_forward
        _C.check(forward(self._plan, x.data_ptr(), out.data_ptr(), ws, nbytes, self._stream()),
                 "unipose_forward_upsampled" if self.upsampled else "unipose_forward")
        if self.bbox:                   # model/unipose.py:34-35
            return out[:, 0:self.num_classes + 1], out[:, self.num_classes + 1:]
        return out

    def keypoints(self, x: torch.Tensor, full_resolution: bool = None, out=None):
        """get_max_preds (utils/evaluate.py:32-54) of the forward's heat-maps without writing them: (preds (B, C, 2) float32,
        maxvals (B, C, 1) float32, idx (B, C) int32) for all C output channels (with the box head the caller slices) — equal bits
        to ``ops.heatmap_argmax`` of the heat-maps.  full_resolution (default: the model's ``stride != 8``): on the grid of the
        maps up-sampled to the input size, else on the maps' own.  `out`: a (preds, maxvals, idx) triple to write into."""
        x = self._input(x)
        if full_resolution is None:
            full_resolution = self.upsampled
        B, C_ = self.batch, self.out_channels
        preds, maxvals, idx = self._outs("UniPosePlan.keypoints", out, ("preds", "maxvals", "idx"), ((B, C_, 2), (B, C_, 1), (B, C_)),
                                         (torch.float32, torch.float32, torch.int32))
        oh, ow = (self.height, self.width) if full_resolution else (self.map_height, self.map_width)
        ws, nbytes = self._ws()
        _C.check(_C.lib().up_unipose_keypoints(self._plan, x.data_ptr(), oh, ow, idx.data_ptr(), preds.data_ptr(), maxvals.data_ptr(),
                                               ws, nbytes, self._stream()), "unipose_keypoints")
        return preds, maxvals, idx

    def persons(self, x: torch.Tensor, dataset: str, max_persons: int = 16, out=None):
        """The multi-person decode of the forward's maps without writing them (``up_unipose_persons``): the device triple of
        ``ops.persons_decode(torch.cat(plan(x), 1), dataset, max_persons)`` — (kpts (B, max_persons, 19, 2), count (B,),
        status (B,)), all int32 — read straight from the NHWC output of the last convolution, on the maps' own grid (the one the
        reference decodes on, also for a model with stride != 8).  `out`: a (kpts, count, status) triple to write into."""
        from . import ops
        if not self.bbox:
            raise ValueError("UniPosePlan.persons: the model has no box head (unipose(..., bbox=True))")
        if dataset not in ops.BOX_CHANNEL0:
            raise ValueError(f"no box channels defined for dataset {dataset!r}")
        f = ops.BOX_CHANNEL0[dataset]
        if self.out_channels < f + 5:
            raise IndexError(f"index {f + 4} is out of bounds for axis 0 with size {self.out_channels}")
        if not 1 <= max_persons <= ops.PERSONS_CAP:
            raise ValueError(f"max_persons {max_persons}: 1..{ops.PERSONS_CAP}")
        x = self._input(x)
        B = self.batch
        if out is None:
            out = ops._persons_out(B, max_persons, 19, self.device)[:3]
        kpts, count, status = self._outs("UniPosePlan.persons", out, ("kpts", "count", "status"), ((B, max_persons, 19, 2), (B,), (B,)),
                                         (torch.int32,) * 3)
        ws, nbytes = self._ws()
        _C.check(_C.lib().up_unipose_persons(self._plan, x.data_ptr(), f, 1, 14, max_persons, count.data_ptr(), status.data_ptr(),
                                             kpts.data_ptr(), ws, nbytes, self._stream()), "unipose_persons")
        return kpts, count, status

    def flip_heatmaps(self, x: torch.Tensor, dataset: str = None, pairs=None, out: torch.Tensor = None):
        """The flip test in one call (``up_unipose_flip_forward``): the network on `x` and on the mirrored `x`, the second maps
        mirrored back with left / right channels exchanged (``protocol.flip_perm(dataset, num_classes, bbox, pairs)``), and the
        mean of the two — equal bits to ``ops.flip_merge(maps(x), maps(x.flip(3)), perm)``.  Returns ONE (B, out_channels, h, w)
        tensor on the maps' own grid ceil(H/8) x ceil(W/8), also for a model with ``stride != 8`` and with the box head."""
        x = self._input(x)
        perm = self._perm(dataset, pairs)
        out = self._out("UniPosePlan.flip_heatmaps", out, (self.batch, self.out_channels, self.map_height, self.map_width))
        ws, nbytes = self._flip_ws()
        _C.check(_C.lib().up_unipose_flip_forward(self._plan, x.data_ptr(), perm, out.data_ptr(), ws, nbytes, self._stream()),
                 "unipose_flip_forward")
        return out

    def final_preds(self, x: torch.Tensor, center=None, scale=None, res=None, flip: bool = False, dataset: str = None, pairs=None,
                    out=None):
        """``ops.final_preds`` of the forward's maps without writing them (``up_unipose_final_preds``): (preds (B, C, 2) in
        source-image pixels, coords (B, C, 2) on the heat-map grid, maxvals (B, C, 1)), float32, for all C output channels, read
        straight from the NHWC output of the last convolution.  `center` (B, 2) / `scale` (B,) as the loader gives them, `res`
        = [W, H] of the maps by default; ``center=None``: preds = coords.  flip: the flip test first (``flip_heatmaps``), with
        `dataset` / `pairs` naming the left / right channels.  Always on the maps' own grid ceil(H/8) x ceil(W/8), also for a
        model with ``stride != 8``.  `out`: a (preds, coords, maxvals) triple to write into."""
        from . import protocol
        x = self._input(x)
        perm = self._perm(dataset, pairs) if flip else None
        res = [self.map_width, self.map_height] if res is None else protocol._res(res)
        inv = None
        if center is not None:
            inv = torch.from_numpy(protocol.inverse_maps(center, scale, res))
            if tuple(inv.shape) != (self.batch, 2, 3):
                raise ValueError(f"UniPosePlan.final_preds: {inv.shape[0]} centres for a batch of {self.batch}")
            inv = inv.to(self.device)
        B, C_ = self.batch, self.out_channels
        preds, coords, maxvals = self._outs("UniPosePlan.final_preds", out, ("preds", "coords", "maxvals"),
                                            ((B, C_, 2), (B, C_, 2), (B, C_, 1)))
        ws, nbytes = self._flip_ws() if flip else self._ws()
        _C.check(_C.lib().up_unipose_final_preds(self._plan, x.data_ptr(), perm, None if inv is None else inv.data_ptr(), int(res[0]),
                                                 int(res[1]), preds.data_ptr(), coords.data_ptr(), maxvals.data_ptr(), ws, nbytes,
                                                 self._stream()), "unipose_final_preds")
        return preds, coords, maxvals

    # ---- from source frames: the crop (up_crop_to_nhwc) in front of the same programs ----------------------------------------------
    def frame_heatmaps(self, frames: torch.Tensor, center, scale, frame_of=None, rot=0, flip: bool = False, dataset: str = None,
                       pairs=None, valid_hw=None, out: torch.Tensor = None):
        """The heat-maps of persons in source frames in one call (``up_unipose_frame_heatmaps``): frames (F, Hs, Ws, 3) uint8 or
        float32 on the device as the camera gives them, `center` (B, 2) / `scale` (B,) one person per sample, frame_of (B,) the
        frame each person is in (None: sample b is in frame b).  The crop is ``protocol.crop_maps(center, scale, [H, W], rot)``
        sampled as ``ops.crop_to_nhwc`` does (border = mean = 128, std = 256): no NCHW input is staged and each person reads the
        frame once.  Returns ONE (B, out_channels, h, w) tensor on the maps' own grid: equal bits to the plan's maps of the
        cropped input, with `flip` to ``flip_heatmaps`` of it (`dataset` / `pairs` as there)."""
        args, keep, _ = self._frame_args("frame_heatmaps", frames, center, scale, frame_of, rot, valid_hw)
        perm = self._perm(dataset, pairs) if flip else None
        out = self._out("UniPosePlan.frame_heatmaps", out, (self.batch, self.out_channels, self.map_height, self.map_width))
        ws, nbytes = self._frame_ws(4 if flip else 0)
        _C.check(_C.lib().up_unipose_frame_heatmaps(self._plan, *args, perm, out.data_ptr(), ws, nbytes, self._stream()),
                 "unipose_frame_heatmaps")
        del keep
        return out

    def frame_final_preds(self, frames: torch.Tensor, center, scale, frame_of=None, rot=0, flip: bool = False, dataset: str = None,
                          pairs=None, valid_hw=None, out=None, res=None):
        """Frames, centres and scales in, joints in frame coordinates out (``up_unipose_frame_final_preds``): the crop of
        ``frame_heatmaps``, the network (with `flip` the flip test), then ``final_preds`` — (preds (B, C, 2) in source-frame
        pixels, coords (B, C, 2) on the heat-map grid, maxvals (B, C, 1)), equal bits to ``final_preds`` of the cropped input.
        The way back is ``protocol.inverse_maps(center, scale, res)`` with `res` = [W, H] of the maps by default, as in
        ``final_preds``; a rotation is not undone on the way back, as in pytorch-pose (``transform_preds`` passes rot = 0)."""
        from . import protocol
        args, keep, _ = self._frame_args("frame_final_preds", frames, center, scale, frame_of, rot, valid_hw)
        perm = self._perm(dataset, pairs) if flip else None
        res = [self.map_width, self.map_height] if res is None else protocol._res(res)
        inv = torch.from_numpy(protocol.inverse_maps(center, scale, res)).to(self.device)
        B, C_ = self.batch, self.out_channels
        preds, coords, maxvals = self._outs("UniPosePlan.frame_final_preds", out, ("preds", "coords", "maxvals"),
                                            ((B, C_, 2), (B, C_, 2), (B, C_, 1)))
        ws, nbytes = self._frame_ws(5 if flip else 6)
        _C.check(_C.lib().up_unipose_frame_final_preds(self._plan, *args, perm, inv.data_ptr(), int(res[0]), int(res[1]),
                                                       preds.data_ptr(), coords.data_ptr(), maxvals.data_ptr(), ws, nbytes,
                                                       self._stream()), "unipose_frame_final_preds")
        del keep
        return preds, coords, maxvals


class _LstmConfig(C.Structure):
    """up_unipose_lstm_config"""
    _fields_ = [(n, C.c_int32) for n in ("batch", "frames", "height", "width", "output_stride", "num_classes")]


class UniPoseLSTMPlan(_Plan):
    """The video model's inference forward through the C ABI (``up_unipose_lstm_step`` / ``up_unipose_lstm_clip``, ABI 10 additions).

    Built from an eval-mode ``unipose_lstm`` (BatchNorm folded like ``checkpoint.fold_batchnorm``).  Two forms, equal bits to the
    folded module (``checkpoint.load_folded``):

        plan = UniPoseLSTMPlan(model, batch=1, height=368, width=368, frames=5)
        heat, cell, hide = plan.step(x[:, 0], cm[:, 0])                    # the first frame (LSTM_0) ...
        heat, cell, hide = plan.step(x[:, 1], cm[:, 1], (hide, cell))      # ... a later one: the module's per-frame path
        heats, cell, hide = plan.clip(x, cm)     # (B, T, K+1, h, w) + the last frame's state: the module's whole-clip unroll
        preds, maxvals, idx, cell, hide = plan.clip_keypoints(x, cm)       # the joints, no NCHW heat-maps in between
        preds, coords, maxvals = plan.clip_final_preds(x, cm, center, scale, flip=True, pairs=[[1, 2], [3, 4]])
        state = plan.stream_state()                                        # a camera: one frame in, joints out
        preds, maxvals, idx = plan.stream(frame, centermap, state, first=True)
        preds, coords, maxvals = plan.clip_frame_final_preds(frames_u8_hwc, center, scale, frame_of=fo)    # the crop and the centre map too
        preds, coords, maxvals = plan.stream_frames(frames_u8_hwc, center, scale, state, first=True)
        pool = plan.stream_pool(32)                                        # many cameras: a batch whose samples start and restart on their own
        preds, maxvals, idx = plan.serve(frames, centermaps, pool, slot=[5, -1, 0], first=[1, 0, 0])      # (batch 3; -1: an idle lane)
        preds, coords, maxvals = plan.serve_frames(frames_u8_hwc, center, scale, pool, slot, first)

    The state is the caller's, NCHW (B, K+2, h, w) as the reference's signature has it; the (K+2, h, w) zeros of the reference's
    first call are accepted too (broadcast over the batch like ``unipose._state``, and ignored when ``first`` is set, as the
    module ignores them at iter == 0).  Weights are captured at construction: ``refresh(model)`` after changing them.  Inference only.

    ``UniPoseLSTMPlan(..., storage="bf16")`` runs every method with the launches of the folded module under
    ``ops.set_conv_math("bf16s")`` (unipose_amd/uniposeLSTM.py): a bf16 trunk that hands over fp32 heat-maps, fp32 ConvLSTM state
    and head, their convolutions of 32-aligned input width on bf16 operands — equal bits again (tests/test_lstm_plan_bf16_*.py).
    Frames, centre maps, states, results and ``refresh`` stay float32; a ``stream_state()`` buffer has the same size in both storages.

    ``UniPoseLSTMPlan(..., flip="one_pass")`` (default ``"two_pass"``; ``plan.flip_mode``) runs the flip test of
    ``clip_flip_heatmaps``, ``clip_final_preds(flip=True)``, ``clip_frame_heatmaps(flip=True)`` and
    ``clip_frame_final_preds(flip=True)`` as ONE pass over 2 * batch samples per frame, the clip and its mirror, each half with its own
    recurrent state.  Its identity: ``clip_flip_heatmaps(x, cm)`` has equal bits, frame by frame, to ``ops.flip_merge`` of the two
    batch halves of ``plan2B.clip(torch.cat([x, x.flip(-1)]), torch.cat([cm, cm.flip(-1)]))``, ``plan2B`` a two-pass plan of batch
    2 * batch — not to the two-pass form, wherever a convolution picks its kernel by the number of rows.  Every other method, the
    state buffer and ``plan.workspace`` of the plain methods are unchanged.
    """
    _prefix = "up_unipose_lstm_plan"

    def __init__(self, model, batch: int, height: int, width: int, frames: int = 1, storage: str = "f32", flip: str = "two_pass"):
        if not isinstance(flip, str) or flip not in ("two_pass", "one_pass"):
            raise ValueError(f"UniPoseLSTMPlan: flip {flip!r}; 'two_pass' or 'one_pass'")
        if not isinstance(storage, str) or storage not in _STORAGE:
            raise ValueError(f"UniPoseLSTMPlan: storage {storage!r}; one of {sorted(_STORAGE)}")
        self.storage, dtype = _STORAGE[storage]
        if model.training:
            raise ValueError("UniPoseLSTMPlan captures the inference forward: call model.eval() first")
        # model.stride is not looked at: the reference's video model stores it (model/uniposeLSTM.py:71) and never up-samples, and
        # neither does the drop-in module (unipose_amd/uniposeLSTM.py).  clip_keypoints / stream decode on either grid.
        if batch < 1 or frames < 1 or height < 8 or width < 8:
            raise ValueError(f"UniPoseLSTMPlan: batch {batch}, {frames} frames, {height} x {width} input")
        w0 = model.backbone.conv1.weight
        if not w0.is_cuda and not _C._ALLOW_HOST_POINTERS:
            raise _C.UniPoseHipError("UniPoseLSTMPlan needs a CUDA(HIP) model; there is no CPU fallback")
        self.num_classes = K = model.num_classes
        os_ = 16 if model.wasp.aspp2.atrous_conv.dilation[0] == 18 else 8
        # (the default goes through up_unipose_lstm_plan_create, as before the storage option)
        self._create(_LstmConfig(batch, frames, height, width, os_, K), w0.device, dtype if dtype else None, flip)
        self.batch, self.frames, self.height, self.width = batch, frames, height, width
        self.out_channels, self.out_height, self.out_width = K + 1, (height - 1) // 8 + 1, (width - 1) // 8 + 1
        self.refresh(model)

    def refresh(self, model):
        """(re)load the weights: BatchNorm folded in float64 and rounded once; the gate weights are stacked by the plan"""
        _set_convs(self, "up_unipose_lstm_plan", fold_batchnorm(model))

    def _input(self, t, shape, what):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != self.device:
            raise ValueError(f"UniPoseLSTMPlan: {what} {tuple(t.shape)} {t.dtype} on {t.device}, planned for {shape} float32 on "
                             f"{self.device}")
        return t.contiguous()

    def _state(self, t, what):
        c = (self.num_classes + 2, self.out_height, self.out_width)
        if t.dim() == 3 and tuple(t.shape) == c:
            t = t.unsqueeze(0).expand(self.batch, -1, -1, -1)
        return self._input(t, (self.batch,) + c, what)

    def step(self, frame: torch.Tensor, centermap: torch.Tensor, prev=None, first: bool = None, out=None):
        """One frame: frame (B, 3, H, W), centermap (B, 1, H, W), prev = None or (hide, cell) -> heat (B, K+1, h, w), cell, hide
        (B, K+2, h, w).  first (default: prev is None) selects LSTM_0, which reads no state."""
        B, H, W, h, w, K = self.batch, self.height, self.width, self.out_height, self.out_width, self.num_classes
        x = self._input(frame, (B, 3, H, W), "frame")
        cm = self._input(centermap, (B, 1, H, W), "centre map")
        if first is None:
            first = prev is None
        if not first and prev is None:
            raise ValueError("UniPoseLSTMPlan.step: a later frame needs the previous (hide, cell)")
        ph = pc = None
        if not first:
            ph, pc = self._state(prev[0], "previous hide"), self._state(prev[1], "previous cell")
        heat, cell, hide = self._outs("UniPoseLSTMPlan", out, ("heat", "cell", "hide"), [(B, K + 1, h, w), (B, K + 2, h, w), (B, K + 2, h, w)])
        ws, nbytes = self._ws()
        _C.check(_C.lib().up_unipose_lstm_step(self._plan, x.data_ptr(), cm.data_ptr(), None if first else ph.data_ptr(),
                                               None if first else pc.data_ptr(), heat.data_ptr(), cell.data_ptr(), hide.data_ptr(),
                                               ws, nbytes, self._stream()), "unipose_lstm_step")
        return heat, cell, hide

    def clip(self, frames: torch.Tensor, centermaps: torch.Tensor, out=None):
        """The whole clip: frames (B, T, 3, H, W), centermaps (B, T, 1, H, W) -> heats (B, T, K+1, h, w) and the last frame's cell,
        hide (B, K+2, h, w).  T is the plan's `frames`."""
        B, T, H, W, h, w, K = self.batch, self.frames, self.height, self.width, self.out_height, self.out_width, self.num_classes
        x = self._input(frames, (B, T, 3, H, W), "clip")
        cm = self._input(centermaps, (B, T, 1, H, W), "centre maps")
        heat, cell, hide = self._outs("UniPoseLSTMPlan", out, ("heat", "cell", "hide"),
                                      [(B, T, K + 1, h, w), (B, K + 2, h, w), (B, K + 2, h, w)])
        ws, nbytes = self._ws()
        _C.check(_C.lib().up_unipose_lstm_clip(self._plan, x.data_ptr(), cm.data_ptr(), heat.data_ptr(), cell.data_ptr(),
                                               hide.data_ptr(), ws, nbytes, self._stream()), "unipose_lstm_clip")
        return heat, cell, hide

    # ---- the evaluation entries: joints, flip test, final_preds, stream ---------------------------------------------------------
    def _clip_inputs(self, frames, centermaps):
        B, T, H, W = self.batch, self.frames, self.height, self.width
        return self._input(frames, (B, T, 3, H, W), "clip"), self._input(centermaps, (B, T, 1, H, W), "centre maps")

    def clip_keypoints(self, frames: torch.Tensor, centermaps: torch.Tensor, full_resolution: bool = False, out=None):
        """The joints of the whole clip without its NCHW heat-maps (``up_unipose_lstm_clip_keypoints``): (preds (B, T, K+1, 2),
        maxvals (B, T, K+1, 1), idx (B, T, K+1) int32, cell, hide (B, K+2, h, w) of the last frame) — equal bits to
        ``ops.heatmap_decode`` of ``clip(...)``'s heat-maps.  full_resolution: on the grid of the maps up-sampled to the input size,
        else on the maps' own.  `out`: such a 5-tuple to write into."""
        B, T, h, w, K = self.batch, self.frames, self.out_height, self.out_width, self.num_classes
        x, cm = self._clip_inputs(frames, centermaps)
        f32 = torch.float32
        preds, maxvals, idx, cell, hide = self._outs(
            "UniPoseLSTMPlan.clip_keypoints", out, ("preds", "maxvals", "idx", "cell", "hide"),
            ((B, T, K + 1, 2), (B, T, K + 1, 1), (B, T, K + 1), (B, K + 2, h, w), (B, K + 2, h, w)), (f32, f32, torch.int32, f32, f32),
            word="tuple")
        oh, ow = (self.height, self.width) if full_resolution else (h, w)
        ws, nbytes = self._ws()
        _C.check(_C.lib().up_unipose_lstm_clip_keypoints(self._plan, x.data_ptr(), cm.data_ptr(), oh, ow, idx.data_ptr(),
                                                         preds.data_ptr(), maxvals.data_ptr(), cell.data_ptr(), hide.data_ptr(), ws,
                                                         nbytes, self._stream()), "unipose_lstm_clip_keypoints")
        return preds, maxvals, idx, cell, hide

    def clip_flip_heatmaps(self, frames: torch.Tensor, centermaps: torch.Tensor, pairs=None, dataset: str = None,
                           out: torch.Tensor = None):
        """The flip test of a clip in one call (``up_unipose_lstm_clip_flip``; this project's extension, the reference's video
        drivers run none): the network on the clip and on the mirrored clip (frames and centre maps), each with its own recurrent
        state, the second maps mirrored back with left / right channels exchanged (``protocol.flip_perm(dataset, K, False,
        pairs)``; the reference has no list for Penn_Action: pass `pairs`), and the mean of the two — equal bits to
        ``ops.flip_merge`` of the two ``clip`` results frame by frame.  Returns (B, T, K+1, h, w)."""
        B, T, h, w, K = self.batch, self.frames, self.out_height, self.out_width, self.num_classes
        x, cm = self._clip_inputs(frames, centermaps)
        perm = self._perm(dataset, pairs)
        out = self._out("UniPoseLSTMPlan.clip_flip_heatmaps", out, (B, T, K + 1, h, w))
        ws, nbytes = self._flip_ws()
        _C.check(_C.lib().up_unipose_lstm_clip_flip(self._plan, x.data_ptr(), cm.data_ptr(), perm, out.data_ptr(), ws, nbytes,
                                                    self._stream()), "unipose_lstm_clip_flip")
        return out

    def clip_final_preds(self, frames: torch.Tensor, centermaps: torch.Tensor, center=None, scale=None, res=None, flip: bool = False,
                         pairs=None, dataset: str = None, out=None):
        """``ops.final_preds`` of the clip's maps without writing them (``up_unipose_lstm_clip_final_preds``): (preds (B, T, K+1, 2)
        in source-image pixels, coords (B, T, K+1, 2) on the heat-map grid, maxvals (B, T, K+1, 1)).  `center` (B, T, 2) / `scale`
        (B, T): one crop per frame (``protocol.inverse_maps``); ``center=None``: preds = coords.  `res` = [w, h] of the maps by
        default.  flip: the flip test first (``clip_flip_heatmaps``).  `out`: a (preds, coords, maxvals) triple to write into."""
        from . import protocol
        B, T, h, w, K = self.batch, self.frames, self.out_height, self.out_width, self.num_classes
        x, cm = self._clip_inputs(frames, centermaps)
        perm = self._perm(dataset, pairs) if flip else None
        res = [w, h] if res is None else protocol._res(res)
        if int(res[0]) <= 0 or int(res[1]) <= 0:
            raise ValueError(f"UniPoseLSTMPlan.clip_final_preds: res {list(res)}")
        inv = None
        if center is not None:
            import numpy as np
            # a tensor stays one (protocol.get_transform keeps the reference's arithmetic in a tensor scale's dtype)
            c = center if isinstance(center, torch.Tensor) else np.asarray(center)
            sc = scale if isinstance(scale, torch.Tensor) or scale is None else np.asarray(scale)
            if sc is None or tuple(c.shape) != (B, T, 2) or tuple(sc.shape) != (B, T):
                raise ValueError(f"UniPoseLSTMPlan.clip_final_preds: center {tuple(c.shape)} / scale "
                                 f"{None if sc is None else tuple(sc.shape)}, one crop per frame is {(B, T, 2)} / {(B, T)}")
            inv = torch.from_numpy(protocol.inverse_maps(c.reshape(B * T, 2), sc.reshape(B * T), res)).to(self.device)
        shapes = ((B, T, K + 1, 2), (B, T, K + 1, 2), (B, T, K + 1, 1))
        preds, coords, maxvals = self._outs("UniPoseLSTMPlan.clip_final_preds", out, ("preds", "coords", "maxvals"), shapes, word="tuple")
        ws, nbytes = self._flip_ws() if flip else self._ws()
        _C.check(_C.lib().up_unipose_lstm_clip_final_preds(self._plan, x.data_ptr(), cm.data_ptr(), perm,
                                                           None if inv is None else inv.data_ptr(), int(res[0]), int(res[1]),
                                                           preds.data_ptr(), coords.data_ptr(), maxvals.data_ptr(), ws, nbytes,
                                                           self._stream()), "unipose_lstm_clip_final_preds")
        return preds, coords, maxvals

    def stream_state(self):
        """A zeroed recurrent-state buffer for ``stream``: opaque bytes (the plan's own NHWC hide and cell), one per camera."""
        n = _C.lib().up_unipose_lstm_plan_state_bytes(self._plan)
        buf = torch.zeros(n + 256, dtype=torch.uint8, device=self.device)
        off = (-buf.data_ptr()) % 256
        return buf[off:off + n]

    def _check_state(self, who, state):
        n = _C.lib().up_unipose_lstm_plan_state_bytes(self._plan)
        if (not isinstance(state, torch.Tensor) or state.dtype != torch.uint8 or state.dim() != 1 or state.numel() != n
                or state.device != self.device or not state.is_contiguous() or state.data_ptr() % 256):
            raise ValueError(f"UniPoseLSTMPlan.{who}: `state` is not a buffer of stream_state() ({n} bytes, uint8, 256-byte aligned, "
                             f"on {self.device})")

    def stream(self, frame: torch.Tensor, centermap: torch.Tensor, state: torch.Tensor, first: bool = False,
               full_resolution: bool = False, heat: torch.Tensor = None):
        """One frame in, joints out (``up_unipose_lstm_stream_keypoints``): (preds (B, K+1, 2), maxvals (B, K+1, 1), idx (B, K+1)
        int32) — equal bits to ``ops.heatmap_decode`` of ``step``'s heat-maps — with hide and cell kept in `state`
        (``stream_state()``), updated in place.  first: the first frame of a stream (LSTM_0; `state` is not read).  `heat`: an
        optional (B, K+1, h, w) tensor that receives the NCHW heat-maps."""
        B, H, W, h, w, K = self.batch, self.height, self.width, self.out_height, self.out_width, self.num_classes
        x = self._input(frame, (B, 3, H, W), "frame")
        cm = self._input(centermap, (B, 1, H, W), "centre map")
        self._check_state("stream", state)
        if heat is not None:
            _check_out("UniPoseLSTMPlan.stream", "heat", heat, (B, K + 1, h, w), self.device)
        preds, maxvals, idx = self._outs("UniPoseLSTMPlan.stream", None, ("preds", "maxvals", "idx"),
                                         ((B, K + 1, 2), (B, K + 1, 1), (B, K + 1)), (torch.float32, torch.float32, torch.int32))
        oh, ow = (H, W) if full_resolution else (h, w)
        ws, nbytes = self._ws()
        _C.check(_C.lib().up_unipose_lstm_stream_keypoints(self._plan, x.data_ptr(), cm.data_ptr(), state.data_ptr(), int(bool(first)),
                                                           oh, ow, idx.data_ptr(), preds.data_ptr(), maxvals.data_ptr(),
                                                           None if heat is None else heat.data_ptr(), ws, nbytes, self._stream()),
                 "unipose_lstm_stream_keypoints")
        return preds, maxvals, idx

    # ---- from source frames: the clip crop and the centre pool in front of the same programs ----------------------------------------
    def _crop_center(self, who, crop_center, lead):
        """the centre of the centre map per sample, (lead, 2) float64 on the device: [int(W / 2), int(H / 2)] by default, where
        get_transform sends `center` (res / 2) and the reference's video loader puts it (penn_action_data.py:105-106,130)"""
        if crop_center is None:
            c = torch.tensor([float(int(self.width / 2)), float(int(self.height / 2))], dtype=torch.float64)
            return c.expand(*lead, 2).contiguous().to(self.device)
        if not isinstance(crop_center, torch.Tensor):
            import numpy as np
            crop_center = np.ascontiguousarray(crop_center, dtype=np.float64)
        c = torch.as_tensor(crop_center, dtype=torch.float64)
        if tuple(c.shape) == (2,):
            c = c.expand(*lead, 2)
        if tuple(c.shape) != tuple(lead) + (2,):
            raise ValueError(f"UniPoseLSTMPlan.{who}: crop_center {tuple(c.shape)}, (2,) or {tuple(lead) + (2,)} expected")
        return c.contiguous().to(self.device)

    def clip_frame_heatmaps(self, frames: torch.Tensor, center, scale, frame_of=None, rot=0, flip: bool = False, pairs=None,
                            dataset: str = None, valid_hw=None, crop_center=None, sigma: float = 3.0, out=None):
        """The heat-maps of a clip from source frames in one call (``up_unipose_lstm_clip_frame_heatmaps``): frames (F, Hs, Ws, 3)
        uint8 or float32 on the device, `center` (B, T, 2) / `scale` (B, T) one crop per frame of the clip, frame_of (B, T) the
        source frame each reads (None: sample (b, t) reads frame b * T + t).  The crop maps are ``protocol.crop_maps`` of the
        flattened (B * T) centres and scales, sampled as ``ops.clip_crop_to_nhwc`` does; the centre map is never built: its pooled
        form comes from `crop_center` ((B, T, 2) or (2,), in pixels of the network input; default [int(W / 2), int(H / 2)], where the
        crop puts `center`) and `sigma` (``ops.center_pool``).  Returns (heats (B, T, K+1, h, w), cell, hide (B, K+2, h, w) of the
        last frame) — equal bits to ``clip`` of the cropped clip and ``ops.make_centermaps(crop_center, H, W, sigma)`` — or with
        `flip` ONE (B, T, K+1, h, w) tensor, equal bits to ``clip_flip_heatmaps`` (`pairs` / `dataset` as there; `out` is then that
        tensor, else the triple)."""
        B, T, h, w, K = self.batch, self.frames, self.out_height, self.out_width, self.num_classes
        args, keep, _ = self._frame_args("clip_frame_heatmaps", frames, center, scale, frame_of, rot, valid_hw, (B, T))
        cc = self._crop_center("clip_frame_heatmaps", crop_center, (B, T))
        L = _C.lib()
        if flip:
            perm = self._perm(dataset, pairs)
            heat = self._out("UniPoseLSTMPlan.clip_frame_heatmaps", out, (B, T, K + 1, h, w))
            ws, nbytes = self._frame_ws(4)
            _C.check(L.up_unipose_lstm_clip_frame_heatmaps(self._plan, *args, cc.data_ptr(), float(sigma), perm, heat.data_ptr(), None,
                                                           None, ws, nbytes, self._stream()), "unipose_lstm_clip_frame_heatmaps")
            del keep
            return heat
        heat, cell, hide = self._outs("UniPoseLSTMPlan.clip_frame_heatmaps", out, ("heat", "cell", "hide"),
                                      [(B, T, K + 1, h, w), (B, K + 2, h, w), (B, K + 2, h, w)])
        ws, nbytes = self._frame_ws(2)
        _C.check(L.up_unipose_lstm_clip_frame_heatmaps(self._plan, *args, cc.data_ptr(), float(sigma), None, heat.data_ptr(),
                                                       cell.data_ptr(), hide.data_ptr(), ws, nbytes, self._stream()),
                 "unipose_lstm_clip_frame_heatmaps")
        del keep
        return heat, cell, hide

    def clip_frame_final_preds(self, frames: torch.Tensor, center, scale, frame_of=None, rot=0, flip: bool = False, pairs=None,
                               dataset: str = None, valid_hw=None, crop_center=None, sigma: float = 3.0, res=None, out=None):
        """Frames, centres and scales in, the clip's joints in frame pixels out (``up_unipose_lstm_clip_frame_final_preds``): the
        crop and the centre pool of ``clip_frame_heatmaps``, the network (with `flip` the flip test), then ``final_preds`` — (preds
        (B, T, K+1, 2) in source-frame pixels, coords (B, T, K+1, 2) on the heat-map grid, maxvals (B, T, K+1, 1)), equal bits to
        ``clip_final_preds`` of the cropped clip.  The way back is ``protocol.inverse_maps(center, scale, res)`` per frame with `res`
        = [w, h] of the maps by default, as in ``clip_final_preds``; a rotation is not undone on the way back."""
        from . import protocol
        B, T, h, w, K = self.batch, self.frames, self.out_height, self.out_width, self.num_classes
        args, keep, (c, sc) = self._frame_args("clip_frame_final_preds", frames, center, scale, frame_of, rot, valid_hw, (B, T))
        cc = self._crop_center("clip_frame_final_preds", crop_center, (B, T))
        perm = self._perm(dataset, pairs) if flip else None
        res = [w, h] if res is None else protocol._res(res)
        if int(res[0]) <= 0 or int(res[1]) <= 0:
            raise ValueError(f"UniPoseLSTMPlan.clip_frame_final_preds: res {list(res)}")
        inv = torch.from_numpy(protocol.inverse_maps(c, sc, res)).to(self.device)
        shapes = ((B, T, K + 1, 2), (B, T, K + 1, 2), (B, T, K + 1, 1))
        preds, coords, maxvals = self._outs("UniPoseLSTMPlan.clip_frame_final_preds", out, ("preds", "coords", "maxvals"), shapes,
                                            word="tuple")
        ws, nbytes = self._frame_ws(5 if flip else 6)
        _C.check(_C.lib().up_unipose_lstm_clip_frame_final_preds(self._plan, *args, cc.data_ptr(), float(sigma), perm, inv.data_ptr(),
                                                                 int(res[0]), int(res[1]), preds.data_ptr(), coords.data_ptr(),
                                                                 maxvals.data_ptr(), ws, nbytes, self._stream()),
                 "unipose_lstm_clip_frame_final_preds")
        del keep
        return preds, coords, maxvals

    def stream_frames(self, frames: torch.Tensor, center, scale, state: torch.Tensor, first: bool = False, frame_of=None, rot=0,
                      valid_hw=None, crop_center=None, sigma: float = 3.0, res=None, heat: torch.Tensor = None):
        """One camera frame in, joints in frame pixels out (``up_unipose_lstm_stream_frame_final_preds``): frames (F, Hs, Ws, 3),
        `center` (B, 2) / `scale` (B,) one person per sample, frame_of (B,) as in ``UniPosePlan.frame_final_preds``; the crop, the
        centre pool (`crop_center` (B, 2) or (2,), `sigma`), the step of ``stream`` with hide and cell kept in `state`
        (``stream_state()``; first: the first frame of a stream), then ``final_preds``: (preds (B, K+1, 2) in source-frame pixels,
        coords (B, K+1, 2), maxvals (B, K+1, 1)) — equal bits to ``ops.final_preds`` of ``stream``'s heat-maps of the cropped frame.
        `heat`: an optional (B, K+1, h, w) tensor that receives the NCHW heat-maps; it is then returned as a fourth item."""
        from . import protocol
        B, h, w, K = self.batch, self.out_height, self.out_width, self.num_classes
        args, keep, (c, sc) = self._frame_args("stream_frames", frames, center, scale, frame_of, rot, valid_hw)
        cc = self._crop_center("stream_frames", crop_center, (B,))
        self._check_state("stream_frames", state)
        if heat is not None:
            _check_out("UniPoseLSTMPlan.stream_frames", "heat", heat, (B, K + 1, h, w), self.device)
        res = [w, h] if res is None else protocol._res(res)
        if int(res[0]) <= 0 or int(res[1]) <= 0:
            raise ValueError(f"UniPoseLSTMPlan.stream_frames: res {list(res)}")
        inv = torch.from_numpy(protocol.inverse_maps(c, sc, res)).to(self.device)
        preds, coords, maxvals = self._outs("UniPoseLSTMPlan.stream_frames", None, ("preds", "coords", "maxvals"),
                                            ((B, K + 1, 2), (B, K + 1, 2), (B, K + 1, 1)))
        ws, nbytes = self._frame_ws(7 if first else 8)
        _C.check(_C.lib().up_unipose_lstm_stream_frame_final_preds(
            self._plan, *args, cc.data_ptr(), float(sigma), state.data_ptr(), int(bool(first)), inv.data_ptr(), int(res[0]), int(res[1]),
            preds.data_ptr(), coords.data_ptr(), maxvals.data_ptr(), None if heat is None else heat.data_ptr(), ws, nbytes,
            self._stream()), "unipose_lstm_stream_frame_final_preds")
        del keep
        return (preds, coords, maxvals) if heat is None else (preds, coords, maxvals, heat)

    # ---- many independent streams in one call: the state in a pool of per-stream records ---------------------------------------------
    def stream_pool(self, slots: int):
        """The recurrent state of `slots` streams for ``serve`` / ``serve_frames``: aligned uint8 bytes
        (``up_unipose_lstm_plan_pool_bytes``), one record per stream — hide (h, w, rup4(K+2)) then cell, float32, the record stride
        rounded up to 256 bytes (``pool_view``).  The content does not matter: a stream's first frame writes its whole record."""
        n = _C.lib().up_unipose_lstm_plan_pool_bytes(self._plan, int(slots))
        if n == 0:
            raise ValueError(f"UniPoseLSTMPlan.stream_pool: {slots} slots")
        buf = torch.empty(n + 256, dtype=torch.uint8, device=self.device)
        off = (-buf.data_ptr()) % 256
        return buf[off:off + n]

    def _pool_slots(self, who, pool):
        rec = _C.lib().up_unipose_lstm_plan_pool_bytes(self._plan, 1)
        if (not isinstance(pool, torch.Tensor) or pool.dtype != torch.uint8 or pool.dim() != 1 or pool.numel() < rec or pool.numel() % rec
                or pool.device != self.device or not pool.is_contiguous() or pool.data_ptr() % 256):
            raise ValueError(f"UniPoseLSTMPlan.{who}: `pool` is not a buffer of stream_pool() (records of {rec} bytes, uint8, 256-byte "
                             f"aligned, on {self.device})")
        return pool.numel() // rec

    def pool_view(self, pool: torch.Tensor):
        """A float32 view (slots, 2, h, w, rup4(K+2)) of a ``stream_pool()`` buffer: [s, 0] the hidden and [s, 1] the cell state of
        the stream in slot s, NHWC, the pad lanes zeros."""
        slots = self._pool_slots("pool_view", pool)
        h, w, ldo = self.out_height, self.out_width, (self.num_classes + 2 + 3) // 4 * 4
        return pool.view(torch.float32).view(slots, -1)[:, :2 * h * w * ldo].view(slots, 2, h, w, ldo)

    def _serve_tables(self, who, slot, first):
        from . import ops
        if len(slot) != self.batch or len(first) != self.batch:
            raise ValueError(f"UniPoseLSTMPlan.{who}: {len(slot)} slots and {len(first)} first flags for a batch of {self.batch}")
        return ops.serve_tables(slot, first)

    def serve(self, frame: torch.Tensor, centermap: torch.Tensor, pool: torch.Tensor, slot, first, full_resolution: bool = False,
              heat: torch.Tensor = None):
        """One frame of up to `batch` independent streams in ONE call (``up_unipose_lstm_serve_keypoints``): ``stream`` for a batch
        whose samples start, continue and restart on their own.  slot (B,): the record of `pool` (``stream_pool(slots)``) that holds
        sample b's stream, -1 for a lane with no stream (it is computed as a first frame and touches nothing of the pool); first (B,):
        truthy where the stream starts or restarts with this frame (LSTM_0, its record is not read).  Returns (preds (B, K+1, 2),
        maxvals (B, K+1, 1), idx (B, K+1) int32): lane b has equal bits to lane b of ``stream`` of the same batch with ``first=True``
        resp. with that stream's state in lane b, and the record becomes that lane of the new state.  `heat`: an optional
        (B, K+1, h, w) tensor that receives the NCHW heat-maps."""
        B, H, W, h, w, K = self.batch, self.height, self.width, self.out_height, self.out_width, self.num_classes
        x = self._input(frame, (B, 3, H, W), "frame")
        cm = self._input(centermap, (B, 1, H, W), "centre map")
        slots = self._pool_slots("serve", pool)
        st, ft = self._serve_tables("serve", slot, first)
        if heat is not None:
            _check_out("UniPoseLSTMPlan.serve", "heat", heat, (B, K + 1, h, w), self.device)
        preds, maxvals, idx = self._outs("UniPoseLSTMPlan.serve", None, ("preds", "maxvals", "idx"),
                                         ((B, K + 1, 2), (B, K + 1, 1), (B, K + 1)), (torch.float32, torch.float32, torch.int32))
        oh, ow = (H, W) if full_resolution else (h, w)
        ws, nbytes = self._ws(_C.lib().up_unipose_lstm_plan_program_workspace(self._plan, _C.PROGRAM_SERVE))
        _C.check(_C.lib().up_unipose_lstm_serve_keypoints(self._plan, x.data_ptr(), cm.data_ptr(), pool.data_ptr(), slots, st, ft, oh, ow,
                                                          idx.data_ptr(), preds.data_ptr(), maxvals.data_ptr(),
                                                          None if heat is None else heat.data_ptr(), ws, nbytes, self._stream()),
                 "unipose_lstm_serve_keypoints")
        return preds, maxvals, idx

    def serve_frames(self, frames: torch.Tensor, center, scale, pool: torch.Tensor, slot, first, frame_of=None, rot=0, valid_hw=None,
                     crop_center=None, sigma: float = 3.0, res=None, heat: torch.Tensor = None):
        """One camera frame of up to `batch` independent streams in, joints in frame pixels out
        (``up_unipose_lstm_serve_frame_final_preds``): ``stream_frames`` with the state in `pool` and the per-sample `slot` / `first`
        of ``serve``.  Returns (preds (B, K+1, 2) in source-frame pixels, coords (B, K+1, 2), maxvals (B, K+1, 1)) and, where given,
        `heat` as a fourth item — equal bits to ``serve`` of the cropped frames and ``ops.make_centermaps(crop_center)``, followed by
        ``ops.final_preds``."""
        from . import protocol
        B, h, w, K = self.batch, self.out_height, self.out_width, self.num_classes
        args, keep, (c, sc) = self._frame_args("serve_frames", frames, center, scale, frame_of, rot, valid_hw)
        cc = self._crop_center("serve_frames", crop_center, (B,))
        slots = self._pool_slots("serve_frames", pool)
        st, ft = self._serve_tables("serve_frames", slot, first)
        if heat is not None:
            _check_out("UniPoseLSTMPlan.serve_frames", "heat", heat, (B, K + 1, h, w), self.device)
        res = [w, h] if res is None else protocol._res(res)
        if int(res[0]) <= 0 or int(res[1]) <= 0:
            raise ValueError(f"UniPoseLSTMPlan.serve_frames: res {list(res)}")
        inv = torch.from_numpy(protocol.inverse_maps(c, sc, res)).to(self.device)
        preds, coords, maxvals = self._outs("UniPoseLSTMPlan.serve_frames", None, ("preds", "coords", "maxvals"),
                                            ((B, K + 1, 2), (B, K + 1, 2), (B, K + 1, 1)))
        ws, nbytes = self._ws(_C.lib().up_unipose_lstm_plan_program_workspace(self._plan, _C.PROGRAM_SERVE + 1))
        _C.check(_C.lib().up_unipose_lstm_serve_frame_final_preds(
            self._plan, *args, cc.data_ptr(), float(sigma), pool.data_ptr(), slots, st, ft, inv.data_ptr(), int(res[0]), int(res[1]),
            preds.data_ptr(), coords.data_ptr(), maxvals.data_ptr(), None if heat is None else heat.data_ptr(), ws, nbytes,
            self._stream()), "unipose_lstm_serve_frame_final_preds")
        del keep
        return (preds, coords, maxvals) if heat is None else (preds, coords, maxvals, heat)


class StreamSlots:
    """A free list over the records of a ``stream_pool(slots)``: ``acquire()`` hands out the lowest free slot when a stream starts,
    ``release(s)`` takes it back when the stream ends.  Host-only bookkeeping: it touches no device memory (a record needs no
    clearing: the stream's first frame writes all of it)."""

    def __init__(self, slots: int):
        if int(slots) < 1:
            raise ValueError(f"StreamSlots: {slots} slots")
        self.slots = int(slots)
        self._free = list(range(self.slots - 1, -1, -1))       # a stack, the lowest slot on top
        self._used = set()

    def acquire(self) -> int:
        if not self._free:
            raise RuntimeError(f"StreamSlots: all {self.slots} slots are in use")
        s = self._free.pop()
        self._used.add(s)
        return s

    def release(self, s: int):
        if s not in self._used:
            raise ValueError(f"StreamSlots: slot {s} is not in use")
        self._used.remove(s)
        self._free.append(s)
        self._free.sort(reverse=True)

    @property
    def free(self) -> int:
        return len(self._free)
