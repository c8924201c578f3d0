"""ctypes mirror of include/idh_model.h — the whole-model C entry points (``idh_model_sizes`` / ``idh_model_pack`` / ``idh_model_fwd``) — and
``ModelEntry``, which describes a BDModel / DepthModel (drop-in, converted or reference modules, or a ``pipeline.HotPath``) to them.

``HotPath`` does NOT go through this: it keeps building its plans with ``nhwc.Plan``.  ``ModelEntry`` is what the parity tests and
tools/perf_model_entry.py call to show that a C host gets HotPath's numbers from one call, and the worked example of the binding a non-Python
host writes.  Reference: experiment_modules/bd_model.py:221-304, depth_model.py:378-433.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch
from torch import nn

from . import _lib
from .net_abi import BlockParams, ConvParams, conv_params, cvencoder_blocks, unetpp_blocks

MODEL_BD, MODEL_DEPTH = 0, 1
VOLUME_FEATURE_MLP, VOLUME_DOT, VOLUME_ZERO = 0, 1, 2
MATCH_FEATS_NCHW, MATCH_LAYER1_NCHW, MATCH_LAYER1_NHWC = 0, 1, 2
QUERY_PLANES, QUERY_SEARCH, QUERY_SEARCH_THR = 0, 1, 2
PRIOR_NONE, PRIOR_WARPED, PRIOR_INPUTS, PRIOR_CHAIN = 0, 1, 2, 3
UNETPP_BLOCKS = 49

f32p = C.c_void_p


class ModelParams(C.Structure):
    _fields_ = [("cv_blocks", BlockParams * 12), ("dec_blocks", BlockParams * UNETPP_BLOCKS), ("depth_heads", ConvParams * 4),
                ("match_head", ConvParams * 2), ("fv_w", f32p * 3), ("fv_b", f32p * 3), ("mlp_w", f32p * 3), ("mlp_b", f32p * 3),
                ("thr_bins", f32p), ("thr_values", f32p)]


class ModelDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("volume", C.c_int32), ("K", C.c_int32), ("C", C.c_int32), ("D", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("P", C.c_int32), ("use_prior", C.c_int32), ("matching_input", C.c_int32), ("query", C.c_int32), ("prior_mode", C.c_int32),
                ("n_thr_bins", C.c_int32), ("search_iters", C.c_int32), ("search_lo", C.c_float), ("search_hi", C.c_float),
                ("search_threshold", C.c_float), ("min_depth", C.c_float), ("max_depth", C.c_float), ("matching_scale", C.c_int32),
                ("math", C.c_int32), ("skip_decoder", C.c_int32), ("return_mask", C.c_int32), ("net", C.POINTER(ModelParams))]


class ModelInputs(C.Structure):
    _fields_ = [("matching_cur", f32p), ("matching_src", f32p), ("matching_layer1", f32p), ("pyramid", f32p * 5), ("src_cam_T_cur_cam", f32p),
                ("cur_cam_T_src_cam", f32p), ("src_K", f32p), ("cur_invK", f32p), ("rendered_depth", f32p), ("prior", f32p),
                ("prior_prediction", f32p), ("prior_channels", C.c_int32), ("prior_cam_T_world", f32p), ("world_T_cam", f32p),
                ("cam_T_world", f32p), ("K_s0", f32p), ("invK_s0", f32p)]


class ModelOutputs(C.Structure):
    _fields_ = [("pred_0", f32p), ("search_depths", f32p), ("prior_mask", f32p), ("log_depth", f32p * 4), ("depth", f32p * 4),
                ("lowest_cost", f32p), ("overall_mask", f32p), ("prior_out", f32p)]


class ModelSizes(C.Structure):
    _fields_ = [("weight_floats", C.c_size_t), ("workspace_floats", C.c_size_t), ("plan_key", C.c_uint64), ("conv_ops", C.c_int32),
                ("conv_launches", C.c_int32)]


def _sigs():
    P = C.POINTER
    i32 = C.c_int
    return {
        "idh_model_sizes": (i32, [P(ModelDesc), i32, P(ModelSizes)]),
        "idh_model_pack": (i32, [P(ModelDesc), P(ModelParams), i32, C.c_void_p, C.c_void_p]),
        "idh_model_fwd": (i32, [P(ModelDesc), C.c_void_p, C.c_size_t, C.c_uint64, i32, P(ModelInputs), P(ModelOutputs), C.c_void_p, C.c_size_t,
                                C.c_void_p]),
    }


SIGS = _sigs()


def _linear(lin: nn.Linear, keep: list):
    w, b = lin.weight.detach().contiguous(), lin.bias.detach().contiguous()
    keep += [w, b]
    return w.data_ptr(), b.data_ptr()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


class ModelEntry:
    """The whole-model C entry for one model.  ``ModelEntry.of(model)`` reads the structure off anything with the BDModel / DepthModel
    attribute names (``cost_volume``, ``cost_volume_net``, ``depth_decoder``, ``binary_mlp``, ``thresholder``) - a drop-in or converted
    model, the reference's modules, or a ``HotPath``; ``.sizes(B)`` / ``.pack(B)`` / ``__call__`` take HotPath.forward's argument names and return
    its output keys.  Blob and workspace are owned here (one per B) and the workspace is reused between calls, so a call allocates only its
    outputs - or nothing, when the caller passes ``out=`` (graph capture)."""

    def __init__(self, cost_volume, cost_volume_net, depth_decoder, binary_mlp=None, thresholder=None, min_depth=0.25, max_depth=5.0,
                 matching_model=None):
        name = type(cost_volume).__name__
        if name in ("FeatureVolumeManager", "FastFeatureVolumeManager"):
            self.volume = VOLUME_FEATURE_MLP
        elif name in ("CostVolumeManager", "EfficientCostVolumeManager"):
            self.volume = VOLUME_DOT
        elif name == "ZeroCostVolumeManager":
            self.volume = VOLUME_ZERO
        else:
            raise _lib.IdhError(f"unrecognised cost volume class {name}")
        self.cost_volume, self.cost_volume_net, self.depth_decoder, self.binary_mlp = cost_volume, cost_volume_net, depth_decoder, binary_mlp
        self.thresholder = thresholder
        self.matching_model = matching_model  # ResnetMatchingEncoder: its net[5:] head runs inside the call when matching_layer1 is passed
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        self.depth_head = bool(getattr(depth_decoder, "depth_head", False)) or len(depth_decoder.convs["output_0"]) == 2
        self._keep: list = []
        p = ModelParams()
        enc = cvencoder_blocks(cost_volume_net, self._keep)
        if len(enc) != 12:
            raise _lib.IdhError("the model entry covers CVEncoders of four levels")
        for i in range(12):
            p.cv_blocks[i] = enc[i]
        dec, heads = unetpp_blocks(depth_decoder, self._keep)
        for i in range(UNETPP_BLOCKS):
            p.dec_blocks[i] = dec[i]
        if heads is not None:
            for i in range(4):
                p.depth_heads[i] = heads[i]
        if self.volume == VOLUME_FEATURE_MLP:
            for j, k in enumerate((0, 2, 4)):
                p.fv_w[j], p.fv_b[j] = _linear(cost_volume.mlp.net[k], self._keep)
        if matching_model is not None:
            p.match_head[0] = conv_params(matching_model.net[5], self._keep)
            p.match_head[1] = conv_params(matching_model.net[8], self._keep)
        if binary_mlp is not None and not self.depth_head:
            seq = binary_mlp.mlps["s0"]
            for j, k in enumerate((0, 2, 4)):
                p.mlp_w[j], p.mlp_b[j] = _linear(seq[k], self._keep)
        self.params = p
        self._blobs: Dict[tuple, tuple] = {}
        self._ws: Dict[tuple, torch.Tensor] = {}

    @classmethod
    def of(cls, model, min_depth: Optional[float] = None, max_depth: Optional[float] = None) -> "ModelEntry":
        opts = getattr(model, "run_opts", None) or getattr(model, "opts", None)
        lo = min_depth if min_depth is not None else getattr(model, "min_depth", getattr(opts, "min_matching_depth", 0.25))
        hi = max_depth if max_depth is not None else getattr(model, "max_depth", getattr(opts, "max_matching_depth", 5.0))
        return cls(model.cost_volume, model.cost_volume_net, model.depth_decoder, getattr(model, "binary_mlp", None),
                   getattr(model, "thresholder", None), lo, hi, getattr(model, "matching_model", None))

    # ------------------------------------------------------------------------------------
    def desc(self, B, K, C_, H, W, P=0, use_prior=None, query=QUERY_PLANES, prior_mode=PRIOR_NONE, return_mask=False,
             matching_input=MATCH_FEATS_NCHW) -> ModelDesc:
        d = ModelDesc()
        d.kind = MODEL_DEPTH if self.depth_head else MODEL_BD
        d.volume, d.K, d.C, d.D, d.H, d.W, d.P = self.volume, K, C_, self.cost_volume.num_depth_bins, H, W, P
        d.use_prior = int(bool(getattr(self.binary_mlp, "use_prior", False)) if use_prior is None else use_prior)
        d.matching_input, d.query, d.prior_mode = matching_input, query, prior_mode
        d.n_thr_bins = self.thresholder.bins.numel() if (query == QUERY_SEARCH_THR and self.thresholder is not None) else 0
        d.search_iters, d.search_lo, d.search_hi, d.search_threshold = 12, 0.5, 8.0, 0.5
        d.min_depth, d.max_depth = self.min_depth, self.max_depth
        d.matching_scale, d.return_mask = 1, int(return_mask)
        d.math = 0 if (getattr(self.binary_mlp, "mlp_math", None) or "fp32") == "fp32" and (self.cost_volume.__dict__.get("mlp_math") or "fp32") == "fp32" else 1
        d.net = C.pointer(self.params)
        return d

    def sizes(self, d: ModelDesc, B: int) -> ModelSizes:
        s = ModelSizes()
        _lib.check(_lib.lib().idh_model_sizes(C.byref(d), B, C.byref(s)), "idh_model_sizes")
        return s

    def pack(self, d: ModelDesc, B: int, device="cuda"):
        """(blob, sizes) for (desc, B), packed once and cached until a parameter changes."""
        s = self.sizes(d, B)
        thr_src = ()
        if self.thresholder is not None and d.query == QUERY_SEARCH_THR:
            thr_src = (self.thresholder.bins, self.thresholder.thresholds)
        ver = (tuple(_lib.param_version(t) for t in self._keep if t is not None),
               tuple((t.data_ptr(), _lib.param_version(t)) for t in thr_src))
        ent = self._blobs.get(s.plan_key)
        if ent is not None and ent[2] == ver:
            return ent[0], s
        if thr_src:  # device copies live only as long as the pack that reads them (stream-ordered)
            bins, thr = (t.to(device=device, dtype=torch.float32).contiguous() for t in thr_src)
            self.params.thr_bins, self.params.thr_values = bins.data_ptr(), thr.data_ptr()
        raw = torch.empty(s.weight_floats + 64, device=device)
        blob = raw[(-raw.data_ptr() // 4) % 64:][: s.weight_floats]  # 256-byte aligned
        _lib.check(_lib.lib().idh_model_pack(C.byref(d), C.byref(self.params), B, blob.data_ptr(), _lib.stream_ptr()), "idh_model_pack")
        if thr_src:
            self.params.thr_bins = self.params.thr_values = None
        self._blobs[s.plan_key] = (blob, raw, ver)
        return blob, s

    def workspace(self, s: ModelSizes, device="cuda", fill: Optional[float] = None):
        w = self._ws.get(s.plan_key)
        if w is None or fill is not None:
            raw = torch.empty(s.workspace_floats + 64, device=device) if fill is None else torch.full((s.workspace_floats + 64,), fill, device=device)
            w = raw[(-raw.data_ptr() // 4) % 64:][: max(s.workspace_floats, 1)]
            self._ws[s.plan_key] = w
        return w

    # ------------------------------------------------------------------------------------
    def __call__(self, matching_cur_feats, matching_src_feats, cur_feats: List[torch.Tensor], src_cam_T_cur_cam, cur_cam_T_src_cam, src_K, cur_invK,
                 rendered_depth=None, prior=None, return_mask=False, prior_inputs=None, infer_depth=False, frame_chain=None,
                 matching_layer1=None, out: Optional[Dict[str, torch.Tensor]] = None, plan=None) -> Dict[str, torch.Tensor]:
        """HotPath.forward's arguments and output keys.  ``matching_layer1`` (B, K+1, 64, H, W), contiguous or channels-last per image (as
        HotPath takes it): the matching-encoder head runs inside the call, and the matching features must be None.  ``out``: preallocated
        outputs (as returned by an earlier call) written in place; ``plan``: (desc, blob, sizes, workspace) from ``prepare`` - what a captured
        graph replays with."""
        mi, l1 = MATCH_FEATS_NCHW, None
        if matching_layer1 is not None:
            if matching_cur_feats is not None or matching_src_feats is not None:
                raise _lib.IdhError("pass either finished matching features or matching_layer1, not both")
            if self.matching_model is None:
                raise _lib.IdhError("matching_layer1 needs a model with a matching_model")
            B, K1, hc, H, W = matching_layer1.shape
            K, C_ = K1 - 1, self.matching_model.net[8].out_channels
            l1 = matching_layer1.reshape(B * K1, hc, H, W)
            if l1.is_contiguous():
                mi = MATCH_LAYER1_NCHW
            elif l1.is_contiguous(memory_format=torch.channels_last):
                mi = MATCH_LAYER1_NHWC
            else:
                l1, mi = l1.contiguous(), MATCH_LAYER1_NCHW
        else:
            B, K, C_, H, W = matching_src_feats.shape
        ins = [matching_cur_feats, matching_src_feats, *cur_feats, src_cam_T_cur_cam, cur_cam_T_src_cam, src_K, cur_invK, rendered_depth, prior]
        _lib.require_cuda_f32(l1, *ins)
        for t in ins:
            if t is not None and not t.is_contiguous():
                raise _lib.IdhError("idh_model_fwd takes dense tensors")
        P = rendered_depth.shape[1] if rendered_depth is not None else 0
        query = QUERY_PLANES
        if infer_depth:
            query = QUERY_SEARCH_THR if self.thresholder is not None else QUERY_SEARCH
        pm, pin = PRIOR_NONE, frame_chain
        if frame_chain is not None:
            pm = PRIOR_CHAIN
        elif prior is not None:
            pm = PRIOR_WARPED
        elif prior_inputs is not None and prior_inputs.get("prior_prediction") is not None:
            pm, pin = PRIOR_INPUTS, prior_inputs
        if plan is None:
            plan = self.prepare(B, K, C_, H, W, P, query=query, prior_mode=pm, return_mask=return_mask, device=src_K.device, matching_input=mi)
        d, blob, s, ws = plan
        if (d.kind == MODEL_BD and (d.query != query or d.prior_mode != pm)) or d.matching_input != mi:
            raise _lib.IdhError("plan prepared for another query / prior mode / matching input")
        H0, W0 = 2 * H, 2 * W
        dev = src_K.device
        if out is None:
            out = {"lowest_cost_bhw": torch.empty(B, H, W, device=dev)}
            out["overall_mask_bhw"] = torch.empty(B, H, W, device=dev, dtype=torch.bool) if (return_mask and self.volume == VOLUME_FEATURE_MLP) else None
            if d.kind == MODEL_DEPTH:
                for i in range(4):
                    out[f"log_depth_pred_s{i}_b1hw"] = torch.empty(B, 1, H0 >> i, W0 >> i, device=dev)
                    out[f"depth_pred_s{i}_b1hw"] = torch.empty(B, 1, H0 >> i, W0 >> i, device=dev)
            else:
                if query != QUERY_PLANES:
                    out["search_depths"] = torch.empty(B, 1, H0, W0, device=dev)
                out["pred_0"] = torch.empty(B, 1 if query != QUERY_PLANES else P, H0, W0, device=dev)
                if pm == PRIOR_INPUTS or (pm == PRIOR_CHAIN and frame_chain.get("prior_prediction") is not None):
                    out["prior_mask"] = torch.empty(B, P, H0, W0, device=dev)
                if pm == PRIOR_CHAIN:
                    out["prior_out"] = torch.empty(1, P, H0, W0, device=dev)
        i = ModelInputs()
        i.matching_cur, i.matching_src, i.matching_layer1 = _ptr(matching_cur_feats), _ptr(matching_src_feats), _ptr(l1)
        for k, f in enumerate(cur_feats):
            i.pyramid[k] = f.data_ptr()
        i.src_cam_T_cur_cam, i.cur_cam_T_src_cam, i.src_K, i.cur_invK = (_ptr(t) for t in (src_cam_T_cur_cam, cur_cam_T_src_cam, src_K, cur_invK))
        i.rendered_depth, i.prior = _ptr(rendered_depth), _ptr(prior)
        if pin is not None:
            for k in pin.values():
                if k is not None:
                    _lib.require_cuda_f32(k)
                    if not k.is_contiguous():
                        raise _lib.IdhError("idh_model_fwd takes dense tensors")
            pp = pin.get("prior_prediction")
            i.prior_prediction, i.prior_channels = _ptr(pp), (pp.shape[1] if pp is not None else 0)
            i.prior_cam_T_world, i.world_T_cam, i.cam_T_world = _ptr(pin.get("prior_cam_T_world")), _ptr(pin.get("world_T_cam_b44")), _ptr(pin.get("cam_T_world_b44"))
            i.K_s0, i.invK_s0 = _ptr(pin.get("K_s0_b44")), _ptr(pin.get("invK_s0_b44"))
        o = ModelOutputs()
        o.pred_0, o.search_depths, o.prior_mask = _ptr(out.get("pred_0")), _ptr(out.get("search_depths")), _ptr(out.get("prior_mask"))
        for k in range(4):
            o.log_depth[k], o.depth[k] = _ptr(out.get(f"log_depth_pred_s{k}_b1hw")), _ptr(out.get(f"depth_pred_s{k}_b1hw"))
        o.lowest_cost, o.overall_mask, o.prior_out = _ptr(out["lowest_cost_bhw"]), _ptr(out.get("overall_mask_bhw")), _ptr(out.get("prior_out"))
        _lib.check(_lib.lib().idh_model_fwd(C.byref(d), blob.data_ptr(), s.weight_floats, s.plan_key, B, C.byref(i), C.byref(o), ws.data_ptr(),
                                            s.workspace_floats, _lib.stream_ptr()), "idh_model_fwd")
        return out

    def prepare(self, B, K, C_, H, W, P, query=QUERY_PLANES, prior_mode=PRIOR_NONE, return_mask=False, device="cuda", ws_fill=None,
                matching_input=MATCH_FEATS_NCHW):
        """(desc, blob, sizes, workspace) of one shape: everything a call needs besides its tensors."""
        d = self.desc(B, K, C_, H, W, P, query=query, prior_mode=prior_mode, return_mask=return_mask, matching_input=matching_input)
        blob, s = self.pack(d, B, device)
        return d, blob, s, self.workspace(s, device, ws_fill)
