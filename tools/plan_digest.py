"""One digest line per plan of the two plan builders, to hold a builder change against its parent: run on both, each in a fresh process, and diff.
  python tools/plan_digest.py           csrc/networks.hip, host only (the parent: IDH_LIB=<its libidh.so>): the size queries of test_plan_audit_cpu's
      _net_plans and the model plans of test_model_plans_are_clean.  Hashed: the raw bytes of the scheduled idh_op array (size queries use
      made-up, deterministic addresses), order, n_first, workspace and blob floats, the sizes struct.
  python tools/plan_digest.py --python  nhwc.Plan, on the GPU (the parent: its tree): the six drop-in forwards and a HotPath plan at small test
      shapes.  Hashed: every op field (pointers by first appearance), levels, the build-index-to-position map, count_launches(), recycled."""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def digest(*parts) -> str:
    return hashlib.sha256(b"".join(p if isinstance(p, bytes) else repr(p).encode() for p in parts)).hexdigest()[:20]


def cpp_plans():
    import plan_audit as A
    from implicit_depth_amd import model_abi as m
    from test_model_abi_cpu import CONFIGS, _entry
    from test_plan_audit_cpu import _net_plans

    def line(label, plans, s):
        (p,) = plans
        d = digest(b"".join(bytes(op) for op in p.ops), p.order, p.n_first, p.ws[1], p.blob[1], [(f, getattr(s, f)) for f, _ in s._fields_])
        print(f"{label}: {len(p.ops)} ops, n_first {p.n_first}, ws {p.ws[1]}, blob {p.blob[1]}, digest {d}")

    *calls, keep = _net_plans()
    for label, call in calls:
        with A.observe() as plans:
            rc, s = call()
        assert rc == 0, (label, rc)
        line(label, plans, s)
    for volume, decoder, use_prior in CONFIGS:
        e = _entry(volume, decoder, use_prior, with_head=True)
        for B in (1, 4, 32):
            for mi in (m.MATCH_FEATS_NCHW, m.MATCH_LAYER1_NCHW):
                d = e.desc(B, 7, 16, 96, 128, P=2, prior_mode=m.PRIOR_INPUTS if use_prior else m.PRIOR_NONE, matching_input=mi)
                with A.observe() as plans:
                    s = e.sizes(d, B)
                line(f"model {volume}/{decoder}/prior={use_prior} B={B} matching_input={mi}", plans, s)


def canon(v, t, seen):
    """A ctypes value as plain lists; a pointer as the index of its first appearance in ``seen`` (the aliasing, not the address)."""
    if t is C.c_void_p:
        return ("ptr", seen.setdefault(v, len(seen)) if v else None)
    if issubclass(t, C.Array):
        return [canon(e, t._type_, seen) for e in v]
    if issubclass(t, C.Structure):
        return [canon(getattr(v, f), ft, seen) for f, ft in t._fields_]
    return v


def python_plans():
    import torch

    import implicit_depth_amd.synthetic as syn
    from implicit_depth_amd import networks as net
    from implicit_depth_amd import nhwc
    from implicit_depth_amd.layers import BasicBlock
    from test_matching_stem_gpu import _encoder
    from test_plan_audit_gpu import _pipeline

    def line(label, p):
        seen = {}
        d = digest([canon(op, type(op), seen) for op in p._array()], p.levels, p._pos, p.count_launches(), p.recycled)
        print(f"{label}: {len(p.ops)} ops, {p.count_launches()} launches, recycled {p.recycled}, digest {d}")

    r = lambda *shape: torch.randn(*shape, device="cuda")
    ch = [24, 64, 128, 256, 384]
    pyr = [t.cuda() for t in syn.encoder_pyramid(1, 96, 128, seed=11)]
    dec_in = [pyr[0]] + [r(1, c, 24 >> i, 32 >> i) for i, c in enumerate(ch[1:])]
    enc = _encoder()
    with torch.no_grad():
        for label, mod, run, tag in (("block_forward_nchw", BasicBlock(24, 40, 2), lambda m: m(r(2, 24, 12, 20)), "bb"),
                                     ("cv_encoder_forward_nchw", net.CVEncoder(16, [48, 64, 160, 256], ch[1:]), lambda m: m(r(1, 16, 24, 32), pyr[1:]), "cve"),
                                     ("decoder_forward_nchw", net.DepthDecoderPP(ch), lambda m: m(dec_in), "dec"),
                                     ("skip_regression_forward_nchw", net.SkipDecoderRegression(ch), lambda m: m(dec_in), "skipreg"),
                                     ("matching_head_forward", enc, lambda m: nhwc.matching_head_forward(m, r(3, 64, 24, 32)), "mh"),
                                     ("matching_encoder_forward", enc, lambda m: m(r(3, 3, 384, 512)), "stem")):
            run(mod.cuda())
            line(label, next(ent[0] for key, ent in mod.__dict__["_idh_plans"].d.items() if key[0] == tag))  # (the plan cached under that key)
        (ent,) = _pipeline(1, 2, 24, 32, 16, 2, False)._plans.values()
        line(f"HotPath (n_head_ops {ent['n_head_ops']})", ent["plan"])
        torch.cuda.synchronize()


if __name__ == "__main__":
    python_plans() if "--python" in sys.argv[1:] else cpp_plans()
