"""MI355X-native cost-volume hot path of nianticlabs/implicit-depth.

The heavy lifting lives in ``csrc/`` (hand-written gfx950 HIP kernels behind the C ABI of
``include/idh.h``); the Python modules here mirror the reference's ``nn.Module`` interface
for this path so they can be swapped into ``BDModel`` / ``DepthModel`` like the reference's
own ``to_fast()`` precedent (reference ``test_bd.py:80-81``).
"""
__version__ = "0.1.0"

_EXPORTS = {"MeshDepthRasterizer": "raster", "TSDFVolume": "fusion", "load_ply": "raster", "save_ply": "raster", "AssetRenderer": "raster", "TemporalEvaluator": "evaluation", "temporal_final_metrics": "evaluation",
            "FrameIngest": "ingest", "load_color": "ingest", "load_depth": "ingest", "intrinsics_pyramid": "ingest",
            "StreamingSession": "streaming", "FeatureBank": "feature_bank", "KeyframeBuffer": "keyframes"}


def __getattr__(name):  # lazily: these modules import torch and bind the library
    if name in _EXPORTS:
        import importlib

        return getattr(importlib.import_module("." + _EXPORTS[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
