"""The whole-model C entry (include/idh_model.h, csrc/model.hip) against HotPath on the same inputs: one idh_model_fwd call must produce
HotPath.forward's outputs bit for bit (same kernels, same kernel choices, same arguments), the frame chain must match HotPath's frame_chain
(sigmoid now in HIP), a captured graph must replay bit-identically, and a blob of another plan must be refused without a write.  The workspace
starts as NaN (as tests/test_net_abi_gpu.py::_alloc): a read of anything the pass did not write shows up."""
import types

import pytest
import torch

import implicit_depth_amd.synthetic as syn
import volume_geometry as vg
from hot_helpers import holder, rel_poses, to_cuda

pytestmark = pytest.mark.gpu


def _setup(K, volume, decoder, use_prior, B, img_h, img_w, P=2, D=64, seed=0, with_head=False):
    from implicit_depth_amd.model_abi import ModelEntry
    from implicit_depth_amd.pipeline import HotPath

    H, W = img_h // 4, img_w // 4
    h = holder(K, volume, H, W, D, use_prior=use_prior, decoder=decoder, with_mlp=decoder == "bd", with_head=with_head).cuda()
    hp = HotPath(h.cost_volume, h.cost_volume_net, h.depth_decoder, getattr(h, "binary_mlp", None),
                 matching_model=h.matching_model if with_head else None).cuda()
    ent = ModelEntry.of(hp)
    cur, src = frame_tuple(B, K, img_h, img_w, seed, P)
    cvi = to_cuda(syn.cost_volume_inputs(B, K, 16, H, W, seed))
    pyr = [t.cuda().contiguous() for t in syn.encoder_pyramid(B, img_h, img_w, seed=seed)]
    a, b = rel_poses(cur, src)
    args = dict(matching_cur_feats=cvi["cur_feats"].contiguous(), matching_src_feats=cvi["src_feats"].contiguous(), cur_feats=pyr,
                src_cam_T_cur_cam=a.contiguous(), cur_cam_T_src_cam=b.contiguous(), src_K=cur_src_K(src), cur_invK=cur["invK_s1_b44"])
    return hp, ent, cur, args


def frame_tuple(B, K, img_h, img_w, seed, P):
    cur, src = syn.frame_tuple(B, K, img_h, img_w, seed=seed, P=P)
    return to_cuda(cur), to_cuda(src)


def cur_src_K(src):
    return src["K_s1_b44"].contiguous()


def _prior_inputs(cur, B, img_h, img_w, seed=5):
    g = torch.Generator().manual_seed(seed)
    pp = torch.rand(B, 1, img_h // 2, img_w // 2, generator=g).cuda()
    shift = torch.eye(4).expand(B, 4, 4).clone()
    shift[:, 0, 3] = 0.05
    return {"prior_prediction": pp, "prior_cam_T_world": shift.cuda().contiguous(), "world_T_cam_b44": cur["world_T_cam_b44"].contiguous(),
            "K_s0_b44": cur["K_s0_b44"].contiguous(), "invK_s0_b44": cur["invK_s0_b44"].contiguous()}


def _same(got, ref, keys):
    for k in keys:
        assert ref.get(k) is not None and got.get(k) is not None, k
        assert got[k].shape == ref[k].shape, k
        assert torch.equal(got[k], ref[k]), (k, float((got[k].float() - ref[k].float()).abs().max()))


CASES = {
    # id: (K, volume, decoder, use_prior, B, img_h, img_w, mode)
    "bd_mlp_k7_b1_512x384": (7, "mlp", "bd", False, 1, 384, 512, "planes"),
    "bd_mlp_k7_b4_mask": (7, "mlp", "bd", False, 4, 64, 128, "planes_mask"),
    "bd_dot_k8_b4": (8, "dot", "bd", False, 4, 64, 128, "planes"),
    "depth_mlp_b4": (7, "mlp", "depth", False, 4, 64, 128, "depth"),
    "depth_dot_b1": (7, "dot", "depth", False, 1, 64, 128, "depth"),
    "search_b4": (7, "mlp", "bd", False, 4, 64, 128, "search"),
    "search_thr_b4": (7, "mlp", "bd", False, 4, 64, 128, "search_thr"),
    "prior_inputs_b4": (7, "mlp", "bd", True, 4, 64, 128, "prior_inputs"),
    "prior_search_b4": (7, "mlp", "bd", True, 4, 64, 128, "prior_search"),
    "prior_warped_b4": (7, "mlp", "bd", True, 4, 64, 128, "prior_warped"),
    # the matching-encoder head inside the call (HotPath(matching_layer1=...)): NCHW (1x1 conv reading it in place) and channels-last
    "layer1_nchw_mlp_b1_512x384": (7, "mlp", "bd", False, 1, 384, 512, "layer1_nchw"),
    "layer1_nchw_mlp_b4": (7, "mlp", "bd", False, 4, 64, 128, "layer1_nchw"),
    "layer1_cl_mlp_b4": (7, "mlp", "bd", False, 4, 64, 128, "layer1_cl"),
    "layer1_nchw_dot_k8_b4": (8, "dot", "bd", False, 4, 64, 128, "layer1_nchw"),
    "layer1_cl_depth_b1": (7, "mlp", "depth", False, 1, 64, 128, "layer1_cl"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_bit_identical_to_hotpath(case):
    K, volume, decoder, use_prior, B, img_h, img_w, mode = CASES[case]
    head = mode.startswith("layer1")
    hp, ent, cur, args = _setup(K, volume, decoder, use_prior, B, img_h, img_w, with_head=head)
    kw = {}
    mi = 0
    if head:
        l1 = syn.layer1_maps(B, K, img_h // 4, img_w // 4, seed=9).cuda()
        if mode == "layer1_cl":
            l1 = l1.view(-1, *l1.shape[2:]).contiguous(memory_format=torch.channels_last).view(l1.shape)
        args["matching_cur_feats"] = args["matching_src_feats"] = None
        kw["matching_layer1"] = l1
        mi = 1 if mode == "layer1_nchw" else 2
    keys = ["lowest_cost_bhw"]
    if decoder == "depth":
        keys += [f"{n}_pred_s{i}_b1hw" for i in range(4) for n in ("log_depth", "depth")]
    else:
        kw["rendered_depth"] = cur["rendered_depth"].contiguous()
        keys.append("pred_0")
    if mode == "planes_mask":
        kw["return_mask"] = True
        keys.append("overall_mask_bhw")
    if mode.startswith("search") or mode == "prior_search":
        kw["infer_depth"] = True
        keys.append("search_depths")
    if mode == "search_thr":
        t = types.SimpleNamespace(bins=torch.linspace(0.5, 8.0, 16).cuda(), thresholds=torch.linspace(0.3, 0.7, 16).cuda())
        hp.thresholder = t
        ent.thresholder = t
    if mode in ("prior_inputs", "prior_search"):
        kw["prior_inputs"] = _prior_inputs(cur, B, img_h, img_w)
        keys.append("prior_mask")
    if mode == "prior_warped":
        kw["prior"] = (torch.rand(B, 2, img_h // 2, img_w // 2, generator=torch.Generator().manual_seed(3)) * 2 - 1).cuda()
    with torch.inference_mode():
        ref = hp(**args, **kw)
        d, blob, s, ws = ent.prepare(B, K, 16, img_h // 4, img_w // 4, kw["rendered_depth"].shape[1] if "rendered_depth" in kw else 0,
                                     query={"search": 1, "search_thr": 2, "prior_search": 1}.get(mode, 0),
                                     prior_mode={"prior_inputs": 2, "prior_search": 2, "prior_warped": 1}.get(mode, 0),
                                     return_mask=mode == "planes_mask", ws_fill=float("nan"), matching_input=mi)
        got = ent(**args, **kw, plan=(d, blob, s, ws))
        got2 = ent(**args, **kw, plan=(d, blob, s, ws))  # a second call on the same (dirty) workspace
        torch.cuda.synchronize()
    _same(got, ref, keys)
    _same(got2, ref, keys)
    if "pred_0" in keys:
        assert bool(torch.isfinite(got["pred_0"]).all())


@pytest.mark.parametrize("volume,K", [("mlp", 7), ("dot", 8)])
def test_per_view_intrinsics_bit_identical_to_hotpath(volume, K):
    """idh_model_fwd with another src_K for every (b, k), another cur_invK for every b and general rotations (tests/volume_geometry.py): the
    cases above repeat one K and rotate about y alone.  A second call on the same plan with other matrices must follow them."""
    B, img_h, img_w = 3, 64, 128
    H, W = img_h // 4, img_w // 4
    hp, ent, cur, args = _setup(K, volume, "bd", False, B, img_h, img_w)
    rd = cur["rendered_depth"].contiguous()
    keys = ["lowest_cost_bhw", "pred_0"] + (["overall_mask_bhw"] if volume == "mlp" else [])
    with torch.inference_mode():
        plan = ent.prepare(B, K, 16, H, W, rd.shape[1], return_mask=volume == "mlp", ws_fill=float("nan"))
        lows = []
        for seed in (300, 301):
            c = to_cuda(vg.build_case("intrinsics", seed, B, K, 16, H, W))
            a = dict(args, matching_cur_feats=c["cur_feats"], matching_src_feats=c["src_feats"], src_cam_T_cur_cam=c["src_extrinsics"],
                     cur_cam_T_src_cam=c["src_poses"], src_K=c["src_Ks"], cur_invK=c["cur_invK"])
            ref = hp(**a, rendered_depth=rd, return_mask=volume == "mlp")
            got = ent(**a, rendered_depth=rd, return_mask=volume == "mlp", plan=plan)
            torch.cuda.synchronize()
            _same(got, ref, keys)
            assert bool(torch.isfinite(got["pred_0"]).all())
            lows.append(got["lowest_cost_bhw"].clone())
    assert not torch.equal(lows[0], lows[1])


def test_frame_chain_matches_hotpath():
    from implicit_depth_amd import model_abi as m

    B, K, img_h, img_w = 4, 7, 64, 128
    hp, ent, cur, args = _setup(K, "mlp", "bd", True, B, img_h, img_w, P=1)
    g = torch.Generator().manual_seed(11)
    wTc = torch.eye(4).expand(B, 4, 4).clone()
    wTc[:, 0, 3] = torch.arange(B) * 0.05
    wTc = wTc.cuda()
    fc = {"world_T_cam_b44": wTc.contiguous(), "cam_T_world_b44": torch.linalg.inv(wTc).contiguous(), "K_s0_b44": cur["K_s0_b44"].contiguous(),
          "invK_s0_b44": cur["invK_s0_b44"].contiguous(), "prior_prediction": torch.rand(1, 1, img_h // 2, img_w // 2, generator=g).cuda(),
          "prior_cam_T_world": torch.eye(4)[None].cuda().contiguous()}
    rd = torch.full((B, 1, img_h // 2, img_w // 2), 2.0, device="cuda")
    with torch.inference_mode():
        ref = hp(**args, rendered_depth=rd, frame_chain=fc)
        plan = ent.prepare(B, K, 16, img_h // 4, img_w // 4, 1, prior_mode=m.PRIOR_CHAIN, ws_fill=float("nan"))
        got = ent(**args, rendered_depth=rd, frame_chain=fc, plan=plan)
        torch.cuda.synchronize()
    _same(got, ref, ["lowest_cost_bhw"])
    # frame 0's prior is the caller's (no sigmoid involved): bit-identical; later frames read sigmoid(logits) computed in HIP
    assert torch.equal(got["pred_0"][:1], ref["pred_0"][:1])
    assert torch.equal(got["prior_mask"][:1], ref["prior_mask"][:1])
    scale = ref["pred_0"].abs().max()
    assert float((got["pred_0"] - ref["pred_0"]).abs().max() / scale) < 1e-5
    assert float((got["prior_mask"] - ref["prior_mask"]).abs().max()) < 1e-5
    assert float((got["prior_out"] - torch.sigmoid(got["pred_0"][-1:])).abs().max()) < 2e-7


def test_graph_capture_replays_bit_identically():
    B, K, img_h, img_w = 2, 7, 64, 128
    hp, ent, cur, args = _setup(K, "mlp", "bd", False, B, img_h, img_w)
    rd = cur["rendered_depth"].contiguous()
    plan = ent.prepare(B, K, 16, img_h // 4, img_w // 4, rd.shape[1])
    static = {k: (v.clone() if torch.is_tensor(v) else [t.clone() for t in v]) for k, v in args.items()}
    srd = rd.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = ent(**static, rendered_depth=srd, plan=plan)  # warm-up, and the outputs the graph writes
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ent(**static, rendered_depth=srd, plan=plan, out=out)
    for r in range(3):
        new_args = {k: (v * (1.0 + 0.1 * r) if k.startswith("matching") else v) for k, v in args.items()}
        new_args["cur_feats"] = [t.flip(-1).contiguous() if r % 2 else t for t in args["cur_feats"]]
        for k, v in new_args.items():
            if torch.is_tensor(v):
                static[k].copy_(v)
            else:
                for a, b in zip(static[k], v):
                    a.copy_(b)
        srd.copy_(rd + 0.1 * r)
        g.replay()
        torch.cuda.synchronize()
        eager = ent(**{k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in new_args.items()}, rendered_depth=(rd + 0.1 * r).contiguous())
        torch.cuda.synchronize()
        _same(out, eager, ["pred_0", "lowest_cost_bhw"])


def test_blob_of_another_plan_is_refused_without_a_write():
    import ctypes as C

    from implicit_depth_amd import _lib
    from implicit_depth_amd import model_abi as m

    B, K, img_h, img_w = 1, 7, 64, 128
    hp, ent, cur, args = _setup(K, "mlp", "bd", False, B, img_h, img_w)
    d, blob, s, ws = ent.prepare(B, K, 16, img_h // 4, img_w // 4, 2)
    rd = cur["rendered_depth"].contiguous()
    pred = torch.full((B, 2, img_h // 2, img_w // 2), 7.0, device="cuda")
    low = torch.full((B, img_h // 4, img_w // 4), 7.0, device="cuda")
    i, o = m.ModelInputs(), m.ModelOutputs()
    i.matching_cur, i.matching_src = args["matching_cur_feats"].data_ptr(), args["matching_src_feats"].data_ptr()
    for k, f in enumerate(args["cur_feats"]):
        i.pyramid[k] = f.data_ptr()
    i.src_cam_T_cur_cam, i.cur_cam_T_src_cam = args["src_cam_T_cur_cam"].data_ptr(), args["cur_cam_T_src_cam"].data_ptr()
    i.src_K, i.cur_invK, i.rendered_depth = args["src_K"].data_ptr(), args["cur_invK"].data_ptr(), rd.data_ptr()
    o.pred_0, o.lowest_cost = pred.data_ptr(), low.data_ptr()
    L = _lib.lib()
    other = ent.sizes(ent.desc(2, K, 16, img_h // 4, img_w // 4, 2), 2).plan_key  # the key of the same model at B = 2
    rc = L.idh_model_fwd(C.byref(d), blob.data_ptr(), s.weight_floats, other, B, C.byref(i), C.byref(o), ws.data_ptr(), s.workspace_floats,
                         _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1
    assert bool((pred == 7.0).all()) and bool((low == 7.0).all())
    # the right key runs
    _lib.check(L.idh_model_fwd(C.byref(d), blob.data_ptr(), s.weight_floats, s.plan_key, B, C.byref(i), C.byref(o), ws.data_ptr(), s.workspace_floats,
                               _lib.stream_ptr()), "idh_model_fwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pred).all()) and not bool((pred == 7.0).any())


def test_frame_chain_matches_single_frame_calls():
    """The 4-frame chain against 4 one-frame calls of the entry, each with IDH_PRIOR_INPUTS = the previous call's prior_out (or the start
    prior): the loop a host runs without the chain.  Different batch sizes take other conv tiles (another summation order), hence the
    scale-relative bar of tests/test_temporal_gpu.py."""
    from implicit_depth_amd import model_abi as m

    B, K, img_h, img_w = 4, 7, 64, 128
    hp, ent, cur, args = _setup(K, "mlp", "bd", True, B, img_h, img_w, P=1)
    g = torch.Generator().manual_seed(12)
    wTc = torch.eye(4).expand(B, 4, 4).clone()
    wTc[:, 0, 3] = torch.arange(B) * 0.05
    wTc = wTc.cuda()
    cTw = torch.linalg.inv(wTc).contiguous()
    fc = {"world_T_cam_b44": wTc.contiguous(), "cam_T_world_b44": cTw, "K_s0_b44": cur["K_s0_b44"].contiguous(),
          "invK_s0_b44": cur["invK_s0_b44"].contiguous(), "prior_prediction": torch.rand(1, 1, img_h // 2, img_w // 2, generator=g).cuda(),
          "prior_cam_T_world": torch.eye(4)[None].cuda().contiguous()}
    rd = torch.full((B, 1, img_h // 2, img_w // 2), 2.0, device="cuda")
    with torch.inference_mode():
        chain = ent(**args, rendered_depth=rd, frame_chain=fc)
        prev, prev_cTw = fc["prior_prediction"], fc["prior_cam_T_world"]
        for b in range(B):
            one = lambda t: t[b:b + 1].contiguous()
            a1 = {k: (one(v) if torch.is_tensor(v) else [one(t) for t in v]) for k, v in args.items()}
            pin = {"prior_prediction": prev, "prior_cam_T_world": prev_cTw, "world_T_cam_b44": one(fc["world_T_cam_b44"]),
                   "K_s0_b44": one(fc["K_s0_b44"]), "invK_s0_b44": one(fc["invK_s0_b44"])}
            o1 = ent(**a1, rendered_depth=one(rd), prior_inputs=pin)
            r = chain["pred_0"][b:b + 1]
            assert float((o1["pred_0"] - r).abs().max() / r.abs().max()) < 5e-5, b
            prev, prev_cTw = torch.sigmoid(o1["pred_0"]).contiguous(), one(cTw)
        torch.cuda.synchronize()
    # (sigmoid' <= 1/4: the logits' bar carries over, in units of their scale)
    assert float((chain["prior_out"] - prev).abs().max()) < 5e-5 * max(1.0, float(chain["pred_0"].abs().max()))


GOLDENS = ["g5_full_bdmodel_mlp", "g5_full_bdmodel_dot", "g9_full_depthmodel", "g5_full_temporal_d96"]


@pytest.mark.parametrize("name", GOLDENS)
def test_reference_goldens(name):
    """The reference's BDModel / DepthModel forward at full size (the goldens and tolerances of tests/test_bdmodel_gpu.py), through one
    idh_model_fwd call."""
    import numpy as np
    from torch import nn

    from conftest import TOL, load_golden, rel_err
    from implicit_depth_amd import cost_volume as cv
    from implicit_depth_amd import networks as net
    from implicit_depth_amd.model_abi import ModelEntry

    g = load_golden(name)
    temporal, depth = name.endswith("temporal_d96"), name.startswith("g9")
    if temporal or not depth:
        K, Hi, Wi, D, P = [int(v) for v in g["dims"]]
    else:
        K, Hi, Wi, D = [int(v) for v in g["dims"]]
        P = 1
    volume = "dot" if name.endswith("_dot") else "mlp"
    h = nn.Module()
    h.cost_volume = (cv.FeatureVolumeManager(Hi // 4, Wi // 4, D, num_source_views=K) if volume == "mlp" else cv.CostVolumeManager(Hi // 4, Wi // 4, D))
    h.cost_volume_net = net.CVEncoder(D, [48, 64, 160, 256], [64, 128, 256, 384])
    h.depth_decoder = (net.DepthDecoderPP if depth else net.BDDecoderPP)([24] + h.cost_volume_net.num_ch_enc)
    if not depth:
        h.binary_mlp = net.BinaryMLPNetwork(h.depth_decoder.num_ch_dec, mlp_size=128, use_prior=temporal)
    syn.fill_state_dict(h, seed=33 if depth else 30)
    assert sorted(h.state_dict()) == list(g["keys"])
    h.cuda()
    s0, s1 = (34, 75) if depth else (31, 71)
    cur, src = syn.frame_tuple(1, K, Hi, Wi, seed=s0, P=P)
    cur, src = to_cuda(cur), to_cuda(src)
    mc = syn.randn((1, 16, Hi // 4, Wi // 4), s1, "mc").cuda()
    ms = syn.randn((1, K, 16, Hi // 4, Wi // 4), s1 + 1, "ms").cuda()
    pyr = [t.cuda().contiguous() for t in syn.encoder_pyramid(1, Hi, Wi, seed=s1 + 2)]
    ent = ModelEntry.of(h)
    kw = {}
    if not depth:
        kw["rendered_depth"] = cur["rendered_depth"].contiguous()
    if temporal:
        kw["prior_inputs"] = {"prior_prediction": torch.sigmoid(syn.randn((1, 1, Hi // 2, Wi // 2), 74, "prior")).cuda(),
                              "prior_cam_T_world": torch.linalg.inv(syn.source_pose(1).float())[None].cuda().contiguous(),
                              "world_T_cam_b44": cur["world_T_cam_b44"].contiguous(), "K_s0_b44": cur["K_s0_b44"].contiguous(),
                              "invK_s0_b44": cur["invK_s0_b44"].contiguous()}
    with torch.inference_mode():
        out = ent(mc.contiguous(), ms.contiguous(), pyr, (src["cam_T_world_b44"] @ cur["world_T_cam_b44"].unsqueeze(1)).contiguous(),
                  (cur["cam_T_world_b44"].unsqueeze(1) @ src["world_T_cam_b44"]).contiguous(), src["K_s1_b44"].contiguous(),
                  cur["invK_s1_b44"].contiguous(), return_mask=True, **kw)
        torch.cuda.synchronize()
    if depth:
        for i in range(4):
            sl = (slice(None), slice(None), slice(None, None, 3), slice(None, None, 4)) if i >= 2 else (slice(None), slice(None), slice(None, None, 6), slice(None, None, 8))
            for nm, tol in ((f"log_depth_pred_s{i}_b1hw", TOL), (f"depth_pred_s{i}_b1hw", 5 * TOL)):
                y = out[nm].cpu()
                assert rel_err(y[sl], g[nm + "_slice"]) < tol, nm
                sd = y.double()
                np.testing.assert_allclose([sd.abs().sum().item(), (sd * sd).sum().item()], g[nm + "_chk"][1:], rtol=1e-3)
    elif temporal:
        pm = out["prior_mask"].cpu()
        assert ((pm[:, :, ::6, ::8] - torch.as_tensor(g["prior_mask_slice"])).abs() > 1e-6).float().mean().item() < 2e-3
        pred = out["pred_0"].cpu()
        dd = (pred[:, :, ::6, ::8] - torch.as_tensor(g["pred_slice"])).abs() / torch.as_tensor(g["pred_slice"]).abs().max()
        assert (dd > TOL).float().mean().item() < 2e-3
        sd = pred.double()
        np.testing.assert_allclose([sd.abs().sum().item(), (sd * sd).sum().item()], g["pred_chk"][1:], rtol=5e-4)
    else:
        pred = out["pred_0"].cpu()
        assert rel_err(pred[:, :, ::6, ::8], g["pred_slice"]) < TOL
        sd = pred.double()
        np.testing.assert_allclose([sd.abs().sum().item(), (sd * sd).sum().item()], g["pred_chk"][1:], rtol=2e-4)
    low = out["lowest_cost_bhw"].cpu()
    if "lowest_slice" in g:
        assert ((low[:, ::3, ::4] - torch.as_tensor(g["lowest_slice"])).abs() > 1e-5).float().mean().item() < 5e-3
    if volume == "mlp" and "mask_slice" in g:
        assert (out["overall_mask_bhw"].cpu()[:, ::3, ::4] != torch.as_tensor(g["mask_slice"])).float().mean().item() < 2e-3
