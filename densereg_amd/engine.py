"""Torch-facing engine: device memory and streams come from PyTorch-ROCm, all compute from the HIP
library behind the C ABI (``include/densereg.h``).  There is no eager / CPU fallback here: every
method hands raw device pointers to ``libdensereg_hip.so``.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Dict, Iterable, NamedTuple, Optional

import numpy as np
import torch

from . import _lib


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), 'engine tensors must be contiguous device tensors'
    return t.data_ptr()


def _f32(t: torch.Tensor) -> torch.Tensor:
    assert t.dtype == torch.float32
    return t


MAP_STRIDE = 4      # input side / map side for every accepted crop size (um_v1.py:109)


class VoteReport(NamedTuple):
    """What ``Engine.vote_report`` / ``infer_report`` fetch next to the joints (``struct dr_vote_report``): the reference's
    "interface to fetch output" (hourglass_um_crop_tiny.py:464-471, 521-526, 781-784).  Members that were not asked for are ``None``."""
    xyz_norm: Optional[torch.Tensor]        # (B,J,3)   normalised mean-shift centre
    uvd: Optional[torch.Tensor]             # (B,J,3)   self.uvd_pts: the joints projected into the crop
    can_idx: Optional[torch.Tensor]         # (B,J,5)   int32 map pixel of each candidate, top_k order
    can_score: Optional[torch.Tensor]       # (B,J,5)   refined heat at those pixels
    can_pts: Optional[torch.Tensor]         # (B,J,5,3) self.can_pts
    ori_pts: Optional[torch.Tensor]         # (B,J,5,3) self.ori_pts
    can_weight: Optional[torch.Tensor]      # (B,J,5)   _get_candidate_weights
    mass: Optional[torch.Tensor]            # (B,J)     mean-shift kernel mass at the final centre (extension: a confidence)
    hm_peak: Optional[torch.Tensor]         # (B,J,3)   (u, v, value) of the raw heat map's first maximum, map resolution

    @property
    def hm_uvd_pts(self) -> Optional[torch.Tensor]:
        """self.hm_uvd_pts (:471), (B,3J): the heat-map peak at input resolution with d = 1 (the reference passes ds = ones).  With the
        legacy bilinear resize every map pixel is an input pixel exactly, so the peak of the resized map is the map's peak scaled by
        in_hw / map_hw = 4 (the network's maps are a quarter of the input side, um_v1.py:109)."""
        if self.hm_peak is None:
            return None
        uv = self.hm_peak[..., :2] * float(MAP_STRIDE)
        return torch.cat([uv, torch.ones_like(uv[..., :1])], dim=-1).reshape(uv.shape[0], -1)


class LossReport(NamedTuple):
    """What ``Engine.loss_report`` fetches (``struct dr_loss_report``): the l2 losses of the most recent forward (hourglass_um_crop_tiny.py
    :353, :357, :363; last axis = hm, hm3, um) and the targets they were taken against (:336-346).  Members that were not asked
    for are ``None``."""
    total: Optional[torch.Tensor]           # (3)         summed over stacks: the first three terms of ``Engine.loss``
    stack_losses: Optional[torch.Tensor]    # (S,3)
    joint_losses: Optional[torch.Tensor]    # (S,J,3)
    crop_losses: Optional[torch.Tensor]     # (B,S,3)
    gt_hm: Optional[torch.Tensor]           # (B,h,w,J)   self.gt_hms
    gt_hm3: Optional[torch.Tensor]          # (B,h,w,J)   self.gt_hm3s
    gt_um: Optional[torch.Tensor]           # (B,h,w,3J)  self.gt_ums


class StepReport(NamedTuple):
    """What ``Engine.step_report`` fetches (``struct dr_step_report``): per trainable variable (``names``, flat order) the statistics
    of the weights, of the averaged and clipped gradient ``g`` and of the decrement ``u`` the next ``apply_adam`` would apply --
    the reference's per-variable histograms (train_single_gpu.py:91-95) and the counts that show a diverging or dead layer before
    the step is taken.  Members that were not asked for are ``None``."""
    param_stats: Optional[torch.Tensor]     # (V,4)   min, max, sum, sum of squares of theta
    grad_stats: Optional[torch.Tensor]      # (V,4)   the same of g
    raw_stats: Optional[torch.Tensor]       # (V,2)   max |a|, sum a^2 over the finite a = acc / div (before the clip)
    update_stats: Optional[torch.Tensor]    # (V,4)   min, max, sum, sum of squares of u
    grad_counts: Optional[torch.Tensor]     # (V,4)   int32: elements, non-finite acc, clipped, acc == 0
    global_: Optional[torch.Tensor]         # (6)     ||g||, ||a|| (finite a), ||theta||, ||u||, max |g|, max |u|   (member ``global``)
    global_counts: Optional[torch.Tensor]   # (3)     int32: non-finite, clipped, zero
    grad_hist: Optional[torch.Tensor]       # (V,E+1) int32 bucket counts of g: bucket = np.searchsorted(edges, x, side='right')
    param_hist: Optional[torch.Tensor]      # (V,E+1) int32 bucket counts of theta
    names: tuple                            # the V variable names
    edges: Optional[torch.Tensor]           # (E) the histogram edges on the device (may be passed back as ``edges``), or None

    def get(self, member: str):
        """Member by its name in ``_lib.STEP_REPORT_FIELDS`` (``global`` is a Python keyword: the attribute is ``global_``)."""
        return getattr(self, 'global_' if member == 'global' else member)


class Panel(NamedTuple):
    """One panel of ``Engine.render`` (``struct dr_panel``): channel ``channel`` of the float32 device tensor ``src`` (B,h,w,C) --
    dense NHWC or a channel-slice view of one -- coloured with ``kind`` ('jet', 'greys', or 'um_xy': the jet panel of _vis_um_xy of
    joint ``channel`` of an offset map), and optionally ``pts`` (B,N,3) drawn over it: ``pts_space`` 'uvd' (pixels of a
    ``pts_hw``-sided image) or 'xyz_mm' (projected with ``cfg`` (B,6)); ``skeleton`` None, 'icvl', 'nyu' or 'msra'."""
    src: torch.Tensor
    channel: int = 0
    kind: str = 'jet'
    pts: Optional[torch.Tensor] = None
    pts_space: str = 'uvd'
    pts_hw: int = 0
    skeleton: Optional[str] = None
    cfg: Optional[torch.Tensor] = None


PANEL_KINDS = {'jet': _lib.PANEL_JET, 'greys': _lib.PANEL_GREYS, 'um_xy': _lib.PANEL_UM_XY}
PTS_SPACES = {'uvd': _lib.PTS_UVD, 'xyz_mm': _lib.PTS_XYZ_MM}
SKELETONS = {None: _lib.SKEL_NONE, 'icvl': _lib.SKEL_ICVL, 'nyu': _lib.SKEL_NYU, 'msra': _lib.SKEL_MSRA}


def hist_edges(lo: float = 1e-12, hi: float = 1e20, ratio: float = 1.1) -> np.ndarray:
    """The symmetric geometric edge set ``-hi ... -lo, +lo ... +hi`` (float32, strictly ascending): ``2 * ceil(log(hi / lo) /
    log(ratio))`` edges, geometrically spaced from ``lo`` to ``hi`` on either side (buckets about ``ratio`` wide) and one bucket
    ``[-lo, +lo)`` around zero.  Buckets follow numpy (``Engine.step_report``)."""
    if not (0.0 < lo < hi and ratio > 1.0):
        raise ValueError('hist_edges: need 0 < lo < hi and ratio > 1')
    n = int(np.ceil(np.log(hi / lo) / np.log(ratio)))
    pos = np.geomspace(lo, hi, n).astype(np.float32)
    e = np.concatenate([-pos[::-1], pos])
    if e.size > _lib.STEP_REPORT_MAX_EDGES or not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
        raise ValueError('hist_edges(%g, %g, %g): %d edges; at most %d strictly ascending finite float32 values can be used'
                         % (lo, hi, ratio, e.size, _lib.STEP_REPORT_MAX_EDGES))
    return e


assert hist_edges().size <= _lib.STEP_REPORT_MAX_EDGES


class Engine:
    """One engine per (process, device).  Mirrors the call sites of the reference:

    * ``forward_eval`` / ``forward_train``  <->  ``um_v1.detect_net(dm, cfgs, coms, J, is_training)``
    * ``vote`` / ``infer``                  <->  ``JointDetectionModel._xyz_estimation`` / ``.test``
    * ``loss`` / ``backward`` / ``apply_adam`` <-> ``.loss`` and the step of ``train_single_gpu.train``
    """

    _holders = 0                # trainers bound to this engine (retain / release)
    _close_pending = False      # close() was asked for while a holder was bound

    def __init__(self, num_stack=2, num_fea=128, num_jnt=16, in_hw=128, kernel_size=3, max_batch=40,
                 device: int = 0, training: bool = False, pipeline: Optional[int] = None):
        """``pipeline`` (training engines): micro-steps in flight, ``dr_set_pipeline``.  2 lets the kernels of micro-step k+1 fill
        the launch boundaries and small-grid chains of micro-step k (measured on MI355X, B=40: S=2 F=128 fp32 2050 -> 2250 crops/s,
        bf16 3350 -> 4006, MSRA J=21 2021 -> 2215) and costs a second set of per-micro-step buffers.  Where every layer already
        runs many rounds of workgroups there is nothing to fill and two streams of big kernels only evict each other's L2 lines
        (S=4 F=256 on 256x256 crops, 163 840 pixels per layer: bf16 473 -> 394, fp32 222 -> 205), so the default (``None``;
        ``DR_PIPELINE=1|2`` overrides) is 2 up to 65 536 pixels per full-resolution layer (max_batch x map side squared) and 1
        above.  When the device cannot hold the second set the engine says so and runs at depth 1."""
        self.lib = _lib.load()
        self.device = torch.device('cuda', device)
        with torch.cuda.device(self.device):
            self.h = _lib.Handle(self.lib, num_stack, num_fea, num_jnt, in_hw, kernel_size, max_batch, device, training)
        self.pipeline = 1
        if training:
            auto = 2 if max_batch * (in_hw // 4) ** 2 <= 65536 else 1
            depth = int(os.environ.get('DR_PIPELINE', auto)) if pipeline is None else int(pipeline)
            if depth == 2:
                try:
                    with torch.cuda.device(self.device):
                        self.h.call('dr_set_pipeline', 2)
                    self.pipeline = 2
                except _lib.DenseRegError as e:
                    if e.code != -5:                                   # DR_E_NOMEM: a speed feature, not a correctness one
                        raise
                    sys.stderr.write('densereg_amd: no memory for a second micro-step slot, running one micro-step at a time (%s)\n' % e)
        self.num_stack, self.num_fea, self.num_jnt, self.in_hw = num_stack, num_fea, num_jnt, in_hw
        self.map_hw = in_hw // MAP_STRIDE
        self.max_batch = max_batch
        self.training = training
        self.groups = 1

    # ---- plumbing ---------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        """Destroy the native handle (weights, workspaces, streams).  While a holder is bound (``retain``: a
        ``DataParallelTrainer`` keeps a zero-copy view of the flat gradient buffer and launches on this engine) the
        handle stays alive and is destroyed when the last holder lets go: the holder's views never dangle and a
        micro-step it still owes runs instead of failing on a destroyed handle."""
        if self._holders > 0:
            self._close_pending = True
            return
        self.h.close()

    def retain(self):
        """A holder (an object that aliases this engine's device memory) binds itself; pair with ``release``."""
        self._holders += 1

    def release(self):
        self._holders -= 1
        if self._holders <= 0 and self._close_pending:
            self._close_pending = False
            self.h.close()

    def set_precision(self, precision: str):
        """'f32' (default) or 'bf16': matrix-core arithmetic of every k != 7 convolution of the handle (dr_set_precision) --
        eval forward / infer, and on a training engine the train-mode forward, the input gradients and the weight
        gradients; BatchReNorm, loss, Adam and the master weights stay fp32.  Call before load_params (it un-finalizes
        the handle and the packed weights follow the precision)."""
        self.h.call('dr_set_precision', {'f32': 0, 'bf16': 1}[precision])

    def set_fusion(self, on: bool):
        """Eval mode: the part of every hourglass below 16x16 pixels as one launch (``dr_set_fusion``; on by default).  Off keeps
        every layer's output in HBM (``read_activation``)."""
        self.h.call('dr_set_fusion', 1 if on else 0)

    def load_params(self, params: Dict[str, np.ndarray]):
        self.h.load_params(params)
        self.h.call('dr_finalize_params', self._stream())

    def read_params(self) -> Dict[str, np.ndarray]:
        torch.cuda.synchronize(self.device)
        return self.h.read_params()

    def param_infos(self):
        return self.h.param_infos()

    def new(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    # ---- the path ---------------------------------------------------------------------------
    def norm_dm(self, dm_mm: torch.Tensor, com: torch.Tensor) -> torch.Tensor:
        out = torch.empty_like(dm_mm)
        self.h.call('dr_norm_dm', dm_mm.shape[0], _p(_f32(dm_mm)), _p(_f32(com)), _p(out), self._stream())
        return out

    def forward_eval(self, dm_norm: torch.Tensor, want_maps: bool = True):
        B, J, m = dm_norm.shape[0], self.num_jnt, self.map_hw
        hm = hm3 = um = None
        if want_maps:
            hm, hm3, um = self.new(B, m, m, J), self.new(B, m, m, J), self.new(B, m, m, 3 * J)
        self.h.call('dr_forward_eval', B, _p(_f32(dm_norm)), _p(hm), _p(hm3), _p(um), self._stream())
        return hm, hm3, um

    def read_maps(self, B: int, stack: int):
        J, m = self.num_jnt, self.map_hw
        hm, hm3, um = self.new(B, m, m, J), self.new(B, m, m, J), self.new(B, m, m, 3 * J)
        self.h.call('dr_read_maps', B, stack, _p(hm), _p(hm3), _p(um), self._stream())
        return hm, hm3, um

    def vote(self, hm, hm3, um, dm_norm, cfg, com) -> torch.Tensor:
        B = dm_norm.shape[0]
        xyz = self.new(B, 3 * self.num_jnt)
        self.h.call('dr_vote', B, _p(hm), _p(hm3), _p(um), _p(dm_norm), _p(cfg), _p(com), _p(xyz), self._stream())
        return xyz

    def infer(self, dm_norm, cfg, com, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        B = dm_norm.shape[0]
        xyz = out if out is not None else self.new(B, 3 * self.num_jnt)
        self.h.call('dr_infer', B, _p(dm_norm), _p(cfg), _p(com), _p(xyz), self._stream())
        return xyz

    def _new_report(self, B: int, fields: Optional[Iterable[str]]):
        """Buffers of the requested members (``None`` = all) and the C struct that names them; the rest stay NULL."""
        want = tuple(_lib.VOTE_REPORT_FIELDS) if fields is None else tuple(fields)
        unknown = [f for f in want if f not in _lib.VOTE_REPORT_FIELDS]
        if unknown:
            raise ValueError('unknown vote report member(s) %s; known: %s' % (unknown, ', '.join(_lib.VOTE_REPORT_FIELDS)))
        bufs, c_rep = {}, _lib.DrVoteReport()
        for name, (tail, is_int) in _lib.VOTE_REPORT_FIELDS.items():
            bufs[name] = self.new(B, self.num_jnt, *tail, dtype=torch.int32 if is_int else torch.float32) if name in want else None
            setattr(c_rep, name + '_dev', _p(bufs[name]))
        return VoteReport(**bufs), c_rep

    def vote_report(self, hm, hm3, um, dm_norm, cfg, com, fields: Optional[Iterable[str]] = None):
        """``vote`` plus the report of the same launch (``dr_vote_report``): ``(xyz_mm, VoteReport)``.  ``fields`` names the
        members to fetch (default: all); the others are ``None`` and cost nothing."""
        B = dm_norm.shape[0]
        xyz = self.new(B, 3 * self.num_jnt)
        rep, c_rep = self._new_report(B, fields)
        self.h.call('dr_vote_report', B, _p(hm), _p(hm3), _p(um), _p(dm_norm), _p(cfg), _p(com), _p(xyz), C.byref(c_rep), self._stream())
        return xyz, rep

    def infer_report(self, dm_norm, cfg, com, fields: Optional[Iterable[str]] = None):
        """``infer`` plus the report (``dr_infer_report``): ``(xyz_mm, VoteReport)``."""
        B = dm_norm.shape[0]
        xyz = self.new(B, 3 * self.num_jnt)
        rep, c_rep = self._new_report(B, fields)
        self.h.call('dr_infer_report', B, _p(dm_norm), _p(cfg), _p(com), _p(xyz), C.byref(c_rep), self._stream())
        return xyz, rep

    def _new_loss_report(self, B: int, fields: Optional[Iterable[str]], known):
        """As ``_new_report``, for ``struct dr_loss_report``; ``known`` = the members this entry point offers."""
        want = tuple(known) if fields is None else tuple(fields)
        unknown = [f for f in want if f not in known]
        if unknown:
            raise ValueError('unknown loss report member(s) %s; known: %s' % (unknown, ', '.join(known)))
        bufs, c_rep = {}, _lib.DrLossReport()
        for name, shape in _lib.LOSS_REPORT_FIELDS.items():
            bufs[name] = self.new(*shape(B, self.num_stack, self.num_jnt, self.map_hw)) if name in want else None
            setattr(c_rep, name + '_dev', _p(bufs[name]))
        return LossReport(**bufs), c_rep

    def targets(self, dm_norm, pose_mm, cfg, com, fields: Optional[Iterable[str]] = None):
        """The training targets as maps (``dr_targets``): ``(gt_hm, gt_hm3, gt_um)``; needs no forward and no parameters.
        ``fields`` names the maps to build (default: all three); the others are ``None``."""
        B = dm_norm.shape[0]
        rep, c = self._new_loss_report(B, fields, ('gt_hm', 'gt_hm3', 'gt_um'))
        self.h.call('dr_targets', B, _p(_f32(dm_norm)), _p(_f32(pose_mm)), _p(_f32(cfg)), _p(_f32(com)), c.gt_hm_dev, c.gt_hm3_dev,
                    c.gt_um_dev, self._stream())
        return rep.gt_hm, rep.gt_hm3, rep.gt_um

    def loss_report(self, dm_norm, pose_mm, cfg, com, fields: Optional[Iterable[str]] = None) -> LossReport:
        """The loss terms of the most recent forward -- eval or train -- per stack, joint and crop, and the targets
        (``dr_loss_report``).  Changes nothing in the engine: a validation loss after ``forward_eval`` / ``infer``, or a closer look
        at a training micro-step between ``forward_train`` and ``backward``.  ``fields`` as in ``vote_report``."""
        B = dm_norm.shape[0]
        rep, c_rep = self._new_loss_report(B, fields, tuple(_lib.LOSS_REPORT_FIELDS))
        self.h.call('dr_loss_report', B, _p(_f32(dm_norm)), _p(_f32(pose_mm)), _p(_f32(cfg)), _p(_f32(com)), C.byref(c_rep),
                    self._stream())
        return rep

    # ---- image report ---------------------------------------------------------------------------
    def render(self, panels, out_hw: int = 128) -> torch.Tensor:
        """The image report (``dr_render_panels``): every ``Panel`` of every crop as RGB8, one launch, no host round trip of the
        maps.  Returns uint8 ``(B, P, out_hw, out_hw, 3)``; ``out_hw`` a multiple of 4 up to 512; at most 16 panels."""
        panels = list(panels)
        if not 1 <= len(panels) <= _lib.RENDER_MAX_PANELS:
            raise ValueError('render: %d panels (1..%d)' % (len(panels), _lib.RENDER_MAX_PANELS))
        B = panels[0].src.shape[0]
        arr, keep = (_lib.DrPanel * len(panels))(), []
        for c, pn in zip(arr, panels):
            src = _f32(pn.src if pn.src.dim() == 4 else pn.src.unsqueeze(-1))
            _, h, w, C_ = src.shape
            cs = src.stride(2)
            if not (src.is_cuda and src.shape[0] == B and src.stride(3) == 1 and src.stride(1) == w * cs and src.stride(0) == h * w * cs):
                raise ValueError('render: a panel source must be a (B,h,w,C) device tensor, NHWC-dense or a channel slice of one')
            if pn.kind not in PANEL_KINDS or not 0 <= (3 * pn.channel + 2 if pn.kind == 'um_xy' else pn.channel) < C_:
                raise ValueError('render: kind %r / channel %d of a %d-channel source' % (pn.kind, pn.channel, C_))
            c.src_dev, c.src_h, c.src_w, c.src_c, c.channel, c.kind = src.data_ptr(), h, w, cs, pn.channel, PANEL_KINDS[pn.kind]
            keep.append(src)
            if pn.pts is not None:
                pts = _f32(pn.pts).reshape(B, -1, 3)
                c.pts_dev, c.num_pts, c.pts_space, c.pts_hw = _p(pts), pts.shape[1], PTS_SPACES[pn.pts_space], int(pn.pts_hw)
                c.skeleton, c.cfg_dev = SKELETONS[pn.skeleton], _p(pn.cfg)
                keep.append(pts)
        out = self.new(B, len(panels), out_hw, out_hw, 3, dtype=torch.uint8)
        with torch.cuda.device(self.device):
            rc = self.lib.dr_render_panels(B, arr, len(panels), int(out_hw), _p(out), self._stream())
        if rc != _lib.DR_OK:
            raise _lib.DenseRegError(rc, 'dr_render_panels')
        return out

    def colormap(self, kind: str) -> np.ndarray:
        """The compiled-in colour table of 'jet' or 'greys' (``dr_colormap``): uint8 (256, 3)."""
        lut = np.empty((256, 3), np.uint8)
        rc = self.lib.dr_colormap(PANEL_KINDS[kind], lut.ctypes.data)
        if rc != _lib.DR_OK:
            raise _lib.DenseRegError(rc, 'dr_colormap')
        return lut

    def read_activation(self, scope: str, B: int, shape) -> np.ndarray:
        torch.cuda.synchronize(self.device)
        a = np.empty(shape, np.float32)
        self.h.call('dr_read_activation', scope.encode(), B, a.ctypes.data, a.size)
        return a

    # ---- training ---------------------------------------------------------------------------
    def forward_train(self, dm_norm, dropout_mode=_lib.DROPOUT_RNG, keep_mask: Optional[torch.Tensor] = None, seed: int = 0):
        self.h.call('dr_forward_train', dm_norm.shape[0], _p(_f32(dm_norm)), int(dropout_mode), _p(keep_mask),
                    C.c_uint64(seed), self._stream())

    def loss(self, dm_norm, pose_mm, cfg, com) -> torch.Tensor:
        """The four loss terms of the last ``forward_train``: a tensor of 4, or ``[groups, 4]`` (one row per micro-batch) after
        ``set_groups(G > 1)``."""
        out = self.new(4) if self.groups == 1 else self.new(self.groups, 4)
        self.h.call('dr_loss', dm_norm.shape[0], _p(dm_norm), _p(_f32(pose_mm)), _p(_f32(cfg)), _p(_f32(com)), _p(out),
                    self._stream())
        return out

    def backward(self, B: int):
        self.h.call('dr_backward', B, self._stream())

    def zero_grad(self):
        self.h.call('dr_zero_grad', self._stream())

    def set_pipeline(self, depth: int):
        """Micro-steps in flight (``dr_set_pipeline``): 1 or 2.  Going to 1 finishes what is in flight and folds the gradients."""
        self.h.call('dr_set_pipeline', int(depth))
        self.pipeline = int(depth)

    def set_groups(self, groups: int):
        """Micro-batch groups (``dr_set_groups``): the next ``forward_train`` / ``loss`` / ``backward`` take ``groups`` consecutive
        micro-batches of one accumulation window at once (per-micro-batch BatchReNorm statistics and state chain, summed
        gradient); 1 restores one micro-batch per call."""
        if int(groups) != self.groups:
            self.h.call('dr_set_groups', int(groups))
            self.groups = int(groups)

    def groups_supported(self, micro_batch: int, groups: int) -> bool:
        """Can ``groups`` micro-batches of ``micro_batch`` crops run as one pass on this engine?  (``dr_set_groups``: at most 8
        groups, whole 32-row tiles per micro-batch in the 2x2 layers = a multiple of 8 crops, and the buffers to hold them.)"""
        return (self.training and 1 <= groups <= 8 and micro_batch % 8 == 0 and micro_batch * groups <= self.max_batch)

    def sync_grads(self):
        """Order the current stream behind every micro-step in flight and make ``flat_view('grad')`` the sum of all slots'
        accumulated gradients (before an all-reduce, or before reading the view); nothing to do at pipeline depth 1."""
        self.h.call('dr_sync_grads', self._stream())

    def apply_adam(self, lr: float, div: float, step: int, clip: float = 0.2):
        self.h.call('dr_apply_adam', C.c_float(lr), C.c_float(div), C.c_float(clip), C.c_int64(step), self._stream())

    def trainable_names(self) -> tuple:
        """The trainable variables in flat order (the rows of every per-variable member of ``step_report``)."""
        if getattr(self, '_trainable_names', None) is None:
            self._trainable_names = tuple(n for n, _, tr in self.h.param_infos() if tr)
        return self._trainable_names

    def _device_edges(self, edges) -> Optional[torch.Tensor]:
        """Histogram edges checked on the host (strictly ascending, finite, at most 2048) and uploaded.  The tensor a previous
        report returned as ``StepReport.edges`` is taken as it is: it was checked then."""
        if edges is None:
            return None
        if edges is getattr(self, '_step_edges', None):
            return edges
        e = edges.detach().cpu().numpy() if isinstance(edges, torch.Tensor) else np.asarray(edges)
        e = np.ascontiguousarray(e, np.float32).reshape(-1)
        if e.size < 1 or e.size > _lib.STEP_REPORT_MAX_EDGES:
            raise ValueError('step report: %d histogram edges (1..%d)' % (e.size, _lib.STEP_REPORT_MAX_EDGES))
        if not np.all(np.isfinite(e)) or not np.all(e[1:] > e[:-1]):
            raise ValueError('step report: the histogram edges must be finite and strictly ascending')
        self._step_edges = torch.from_numpy(e).to(self.device)
        return self._step_edges

    def step_report(self, lr: float, div: float, step: int, clip: float = 0.2, fields: Optional[Iterable[str]] = None,
                    edges=None) -> StepReport:
        """The step ``apply_adam(lr, div, step, clip)`` would take now, described and not taken (``dr_step_report``): changes
        nothing in the engine.  ``fields`` names the members to fetch (``_lib.STEP_REPORT_FIELDS``; default: all, the two
        histograms only when ``edges`` are given); the others are ``None`` and cost nothing.  ``edges``: strictly ascending finite
        histogram edges (``hist_edges()``), a host array or the device tensor of an earlier report; element ``x`` is counted in
        bucket ``np.searchsorted(edges, x, side='right')``."""
        known = _lib.STEP_REPORT_FIELDS
        if fields is None:
            want = tuple(n for n in known if edges is not None or not n.endswith('_hist'))
        else:
            want = tuple(fields)
        unknown = [f for f in want if f not in known]
        if unknown:
            raise ValueError('unknown step report member(s) %s; known: %s' % (unknown, ', '.join(known)))
        if edges is None and any(n.endswith('_hist') for n in want):
            raise ValueError('step report: a histogram member needs edges')
        d_edges = self._device_edges(edges)
        names = self.trainable_names()
        V, E = len(names), 0 if d_edges is None else int(d_edges.numel())
        bufs, c_rep = {}, _lib.DrStepReport()
        c_rep.hist_edges_dev, c_rep.num_edges = _p(d_edges), E
        for name, (shape, is_int) in known.items():
            t = self.new(*shape(V, E), dtype=torch.int32 if is_int else torch.float32) if name in want else None
            bufs['global_' if name == 'global' else name] = t
            setattr(c_rep, name + '_dev', _p(t))
        self.h.call('dr_step_report', C.c_float(lr), C.c_float(div), C.c_float(clip), C.c_int64(step), C.byref(c_rep), self._stream())
        return StepReport(names=names, edges=d_edges, **bufs)

    def flat_view(self, which: str) -> torch.Tensor:
        """Zero-copy torch view of the flat fp32 gradient / parameter buffer (for RCCL all-reduce)."""
        ptr, n = self.h.flat(which)
        return _as_tensor(ptr, n, self.device)

    def conv_flops_per_crop(self) -> float:
        return self.h.conv_flops_per_crop()

    # ---- checkpoints (tf.train.Saver files of the reference, train_single_gpu.py:108-123,172) -----
    def _trainable_offsets(self):
        off, out = 0, {}
        for name, shape, trainable in self.h.param_infos():
            if trainable:
                n = int(np.prod(shape))
                out[name] = (off, n)
                off += n
        return out

    def adam_views(self):
        m, v, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        self.h.call('dr_flat_adam', C.byref(m), C.byref(v), C.byref(n))
        return _as_tensor(m.value, n.value, self.device), _as_tensor(v.value, n.value, self.device)

    def load_checkpoint(self, prefix: str, strict: bool = True) -> dict:
        """Restore from ``<prefix>.index`` / ``.data-*`` written by the reference (or by ``save_checkpoint``): model
        variables, BatchReNorm state incl. the zero-debias slots, and -- on a training engine -- Adam's moments.
        Returns the import report (``missing`` / ``unexpected`` names, ``scalars`` such as ``global_step``)."""
        from . import checkpoint
        torch.cuda.synchronize(self.device)
        rep = checkpoint.load_into(self.h, prefix, strict=strict)
        if self.training and (rep['adam_m'] or rep['adam_v']):
            m, v = self.adam_views()
            for src, dst in ((rep['adam_m'], m), (rep['adam_v'], v)):
                for name, (off, n) in self._trainable_offsets().items():
                    if name in src:
                        dst[off:off + n].copy_(torch.from_numpy(src[name].reshape(-1)))
        self.h.call('dr_finalize_params', self._stream())
        return rep

    def save_checkpoint(self, prefix: str, global_step: Optional[int] = None, beta_powers=None):
        """Write a checkpoint the reference's ``Saver.restore`` reads by name (variables, slots, Adam moments)."""
        from . import checkpoint
        torch.cuda.synchronize(self.device)
        extra = {}
        if self.training:
            m, v = (t.cpu().numpy() for t in self.adam_views())
            shapes = {n: s for n, s, _ in self.h.param_infos()}
            for name, (off, n) in self._trainable_offsets().items():
                extra[name + '/Adam'] = m[off:off + n].reshape(shapes[name])
                extra[name + '/Adam_1'] = v[off:off + n].reshape(shapes[name])
            # AdamOptimizer's non-slot variables: Saver(tf.global_variables()).restore needs them.  After t applied updates
            # they hold beta^(t+1) (TF initialises them to beta and multiplies once per apply_gradients).
            if beta_powers is None and global_step is not None:
                beta_powers = (0.5 ** (int(global_step) + 1), 0.999 ** (int(global_step) + 1))
            if beta_powers is not None:
                extra['beta1_power'] = np.array(beta_powers[0], np.float32)
                extra['beta2_power'] = np.array(beta_powers[1], np.float32)
        return checkpoint.export_from(self.h, prefix, global_step=global_step, extra=extra)


class _CudaArray:
    """``__cuda_array_interface__`` shim so torch can alias library-owned device memory."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {'shape': (n,), 'typestr': '<f4', 'data': (ptr, False), 'version': 2}


def _as_tensor(ptr: int, n: int, device) -> torch.Tensor:
    return torch.as_tensor(_CudaArray(ptr, n), device=device)
