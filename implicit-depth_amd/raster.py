"""Depth-only mesh rasterisation (csrc/raster.hip) with the surface of the reference's ``Pytorch3DRasterizer``
(utils/binary_metrics_utils.py:283-388), which needs pytorch3d's CUDA kernels.

``MeshDepthRasterizer`` renders the query plane of a ``temporal_eval`` window (test_bd.py:172-181) and the scene's ground-truth mesh
(:362), and samples a prediction at every projected ground-truth vertex (:360-388).  ``load_ply`` reads the mesh.  Semantics of the render:
include/idh_raster.h and DESIGN.md §4.8 — pixel (i, j) looks along the ray through (j + 0.5, i + 0.5), the nearest z > 0 wins, -1 where
nothing is hit, triangles crossing z = 0 are drawn for their part in front of the camera.

``render_shaded`` / ``AssetRenderer`` (csrc/raster_shade.hip) render an asset for the live AR loop with the same geometry:
the same depth bit for bit, plus lit RGBA from vertex colours, the visible face, its barycentrics and interpolated per-vertex attributes."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib

PLANE_SIZE = 1024      # vertices per side of the query plane (binary_metrics_utils.py:306)
PLANE_SPACING = 0.025  # metres between them
DEPTH_TOLERANCE = 0.05  # a vertex is visible when the visibility render is within this of its depth (:381)

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _ply_type(name, path):
    try:
        return _PLY_TYPES[name]
    except KeyError:
        raise ValueError(f"{path}: unknown PLY property type {name!r}") from None


def load_ply(path, return_colors: bool = False):
    """(verts float32 (V,3), faces int64 (F,3)) of an ASCII or binary-little-endian PLY file, as pytorch3d.io.load_ply returns them
    (binary_metrics_utils.py:299).  Extra vertex properties, scalar properties beside the face list (e.g. ``uchar flags``) and extra
    scalar-only elements are skipped; the face list may have any integer count and index type.  With ``return_colors`` a third value
    follows: the vertices' ``red``, ``green``, ``blue`` and ``alpha`` (255 when the file has none) as uint8 (V,4), as ScanNet meshes
    carry them and ``render_shaded`` takes them, or None when the file has no colours.  Triangles only.  Not supported (ValueError):
    big-endian files, list properties outside the face element, more than one list per face, colours that are not uchar."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data.index(b"\n", end) + 1
    fmt, elements = None, []  # elements: [name, count, [(name, type) or (name, count type, index type)]]
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"{path}: property before any element")
            if tok[1] == "list":
                elements[-1][2].append((tok[4], _ply_type(tok[2], path), _ply_type(tok[3], path)))
            else:
                elements[-1][2].append((tok[2], _ply_type(tok[1], path)))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported (ascii and binary_little_endian are)")
    tokens = data[body:].split() if fmt == "ascii" else None
    at = 0 if fmt == "ascii" else body
    verts = faces = colors = None
    for name, count, props in elements:
        lists = [p for p in props if len(p) == 3]
        if lists and (name != "face" or len(lists) > 1):
            raise ValueError(f"{path}: list properties are only supported as the one vertex list of the face element (element {name!r})")
        # every row has a fixed width once the list is known to hold three indices: a structured dtype / a token matrix reads the block
        fields, width = [], 0
        for p in props:
            if len(p) == 3:
                fields += [("#n", "<" + p[1]), ("#i", "<" + p[2], (3,))]
                width += 4
            else:
                fields.append((p[0], "<" + p[1]))
                width += 1
        if fmt == "ascii":
            block = tokens[at:at + count * width]
            at += count * width
            if lists and count:
                col = [len(q) == 3 for q in props].index(True)
                if len(block) != count * width or any(int(t) != 3 for t in block[col::width]):
                    raise ValueError(f"{path}: only triangle faces are supported")
            rows = np.array(block, dtype=np.float64).reshape(count, width)
            cols, j = {}, 0
            for p in props:
                if len(p) == 3:
                    cols["#n"], cols["#i"] = rows[:, j], rows[:, j + 1:j + 4]
                    j += 4
                else:
                    cols[p[0]] = rows[:, j]
                    j += 1
        else:
            dt = np.dtype(fields)
            if lists and count:
                off = sum(np.dtype(f[1]).itemsize for f in fields[:[f[0] for f in fields].index("#n")])
                first = int(np.frombuffer(data, dtype=dt.fields["#n"][0], count=1, offset=at + off)[0]) if at + dt.itemsize <= len(data) else -1
                if first != 3 or at + count * dt.itemsize > len(data):
                    raise ValueError(f"{path}: only triangle faces are supported")
            rows = np.frombuffer(data, dtype=dt, count=count, offset=at)
            at += count * dt.itemsize
            cols = {f[0]: rows[f[0]] for f in fields}
        if name == "vertex":
            if not all(k in cols for k in "xyz"):
                raise ValueError(f"{path}: vertex element without x, y, z")
            verts = np.stack([np.asarray(cols[k], dtype=np.float32) for k in "xyz"], 1)
            if return_colors and all(k in cols for k in ("red", "green", "blue")):
                names = ("red", "green", "blue") + (("alpha",) if "alpha" in cols else ())
                if any(t != "u1" for n, t in (q for q in props if len(q) == 2) if n in names):
                    raise ValueError(f"{path}: vertex colours must be uchar")
                colors = np.full((count, 4), 255, np.uint8)
                for j, k in enumerate(names):
                    colors[:, j] = np.asarray(cols[k]).astype(np.uint8)
        elif name == "face" and lists:
            if (np.asarray(cols["#n"]) != 3).any():
                raise ValueError(f"{path}: only triangle faces are supported")
            faces = np.asarray(cols["#i"]).astype(np.int64).reshape(count, 3)
    if verts is None:
        raise ValueError(f"{path}: no vertex element")
    if faces is None:
        faces = np.zeros((0, 3), np.int64)
    if faces.size and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError(f"{path}: face index outside the {len(verts)} vertices")
    pair = torch.from_numpy(np.ascontiguousarray(verts)), torch.from_numpy(np.ascontiguousarray(faces))
    if return_colors:
        return pair + (None if colors is None else torch.from_numpy(colors),)
    return pair


def save_ply(path, verts, faces, colors=None) -> None:
    """Write a triangle mesh as binary little-endian PLY that ``load_ply`` reads back exactly: ``verts`` (V,3) stored as float32,
    ``faces`` (F,3) of any integer type stored as ``uchar`` count + ``int`` indices, ``colors`` (V,3) or (V,4) uint8 stored as
    ``red green blue [alpha]`` uchar (the layout of ScanNet's meshes).  Tensors (GPU ones included) or arrays."""
    def host(t):
        return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    v, f = host(verts), host(faces)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
        raise ValueError(f"save_ply: verts {v.shape} must be (V,3) and faces {f.shape} {f.dtype} an integer (F,3)")
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"save_ply: face index outside the {len(v)} vertices")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    names = ()
    if colors is not None:
        c = host(colors)
        if c.dtype != np.uint8 or c.ndim != 2 or c.shape[0] != len(v) or c.shape[1] not in (3, 4):
            raise ValueError(f"save_ply: colors {c.shape} {c.dtype} must be uint8 ({len(v)},3) or ({len(v)},4)")
        names = ("red", "green", "blue", "alpha")[:c.shape[1]]
        fields += [(n, "u1") for n in names]
    vrec = np.empty(len(v), dtype=np.dtype(fields))
    for j, k in enumerate("xyz"):
        vrec[k] = v[:, j]
    for j, k in enumerate(names):
        vrec[k] = c[:, j]
    frec = np.empty(len(f), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    frec["n"], frec["i"] = 3, f
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
    header += [f"property uchar {n}" for n in names]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(vrec.tobytes())
        out.write(frec.tobytes())


def plane_faces(size: int = PLANE_SIZE) -> torch.Tensor:
    """The (2 (size-1)^2, 3) int64 faces of the size x size vertex grid in the order of the reference's double loop
    (binary_metrics_utils.py:315-323): for idx = h * size + w, (idx, idx + size + 1, idx + size) then (idx, idx + 1, idx + 1 + size)."""
    idx = (torch.arange(size - 1).view(-1, 1) * size + torch.arange(size - 1).view(1, -1)).reshape(-1, 1)
    off = torch.tensor([[0, size + 1, size], [0, 1, size + 1]])
    return (idx.view(-1, 1, 1) + off.view(1, 2, 3)).reshape(-1, 3)


def plane_vertices(world_T_cam_b44: torch.Tensor, distance) -> torch.Tensor:
    """(size^2, 3) vertices of the plane ``distance`` in front of the camera (binary_metrics_utils.py:306-314, :325), by the same
    operations: the float32 grid, z scaled by ``distance``, one matmul with the pose."""
    x = (torch.arange(PLANE_SIZE, dtype=torch.float64) - PLANE_SIZE // 2) * PLANE_SPACING
    ys, xs = torch.meshgrid(x, x, indexing="ij")  # np.meshgrid(x, x): xs varies along the row
    one = torch.ones_like(xs)
    points_14N = torch.stack((xs, ys, one, one), 0).float().view(1, 4, -1).to(world_T_cam_b44.device)
    points_14N[:, 2] *= distance
    return torch.matmul(world_T_cam_b44, points_14N)[0, :3].T


def _mesh(verts, faces, device=None):
    v = torch.as_tensor(verts).float()
    f = torch.as_tensor(faces)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or f.dtype.is_floating_point:
        raise _lib.IdhError(f"mesh: vertices {tuple(v.shape)} must be (V,3) floats and faces {tuple(f.shape)} (F,3) integers")
    if device is not None:
        v, f = v.to(device), f.to(device)
    return v.contiguous(), f.long().contiguous()


def render_depth(verts, faces, cam_T_world_b44, K_b44, height, width) -> torch.Tensor:
    """(B,1,height,width) depth of the mesh (``verts`` (V,3) float32, ``faces`` (F,3) integer, both on the GPU) in B cameras.  The kernel
    reads int32 faces: pass them as int32 to render the same mesh repeatedly without a conversion per call (MeshDepthRasterizer does)."""
    _lib.require_cuda_f32(verts, cam_T_world_b44, K_b44)
    if cam_T_world_b44.dim() != 3 or tuple(cam_T_world_b44.shape[1:]) != (4, 4) or tuple(K_b44.shape) != tuple(cam_T_world_b44.shape):
        raise _lib.IdhError(f"render_depth: cam_T_world {tuple(cam_T_world_b44.shape)} and K {tuple(K_b44.shape)} must both be (B,4,4)")
    if not faces.is_cuda:
        raise _lib.IdhError("render_depth: faces must be on the GPU; there is no CPU fallback")
    B, V, F = cam_T_world_b44.shape[0], verts.shape[0], faces.shape[0]
    f32 = faces.to(torch.int32).contiguous()  # no copy when they already are
    v, T, K = verts.contiguous(), cam_T_world_b44.contiguous(), K_b44.contiguous()
    out = torch.empty(B, 1, height, width, device=v.device)
    nbytes = _lib.lib().idh_raster_workspace_bytes(B, V, F)
    ws = torch.empty(max(nbytes, 256), device=v.device, dtype=torch.uint8)
    _lib.check(_lib.lib().idh_raster_depth_fwd(_lib.ptr(v) if V else None, V, _lib.ptr(f32) if F else None, F, T.data_ptr(), K.data_ptr(), B,
                                               height, width, out.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr()), "idh_raster_depth_fwd")
    return out


def render_shaded(verts, faces, cam_T_world_b44, K_b44, height, width, *, colors=None, attrs=None, ambient: float = 0.3,
                  empty_depth: float = -1.0, return_faces: bool = False, return_bary: bool = False) -> Dict[str, torch.Tensor]:
    """The mesh in B cameras with everything a compositor or a user's own shader needs, in one call (idh_raster_shaded_fwd, DESIGN.md
    §4.19).  ``verts`` (V,3) float32 and ``faces`` (F,3) integer as for ``render_depth`` (int32 faces are used as they are).  Returns

    * ``"depth"`` (B,1,height,width): ``render_depth``'s values bit for bit, ``empty_depth`` where nothing is hit;
    * ``"rgba"`` (B,height,width,4) uint8 when ``colors`` (V,4) uint8 is given: the vertex colours interpolated over the visible face
      and lit by a headlight at the camera on the face's own normal (``ambient`` in [0, 1]; 1 = unlit), alpha interpolated and 0 where
      nothing is hit: ``compositing.composite_mask(..., virtual_rgba=...)`` takes it as it is;
    * ``"attrs"`` (B,height,width,C) when ``attrs`` (V,C) float32, 1 <= C <= 16, is given: the user's own per-vertex quantities
      (normals, UVs, labels) interpolated perspective-correctly, zeros where nothing is hit;
    * ``"pix_to_face"`` (B,height,width) int32, -1 where nothing is hit (``return_faces``), and ``"bary"`` (B,height,width,3), the
      barycentric weights of the face's three vertices at the hit point (``return_bary``).

    Among faces at exactly the same depth the lowest index wins; two calls return the same bits.  There is no CPU fallback."""
    _lib.require_cuda_f32(verts, cam_T_world_b44, K_b44, attrs)
    if cam_T_world_b44.dim() != 3 or tuple(cam_T_world_b44.shape[1:]) != (4, 4) or tuple(K_b44.shape) != tuple(cam_T_world_b44.shape):
        raise _lib.IdhError(f"render_shaded: cam_T_world {tuple(cam_T_world_b44.shape)} and K {tuple(K_b44.shape)} must both be (B,4,4)")
    if not faces.is_cuda:
        raise _lib.IdhError("render_shaded: faces must be on the GPU; there is no CPU fallback")
    B, V, F = cam_T_world_b44.shape[0], verts.shape[0], faces.shape[0]
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point:
        raise _lib.IdhError(f"render_shaded: vertices {tuple(verts.shape)} must be (V,3) and faces {tuple(faces.shape)} (F,3) integers")
    if colors is not None and (not colors.is_cuda or colors.dtype != torch.uint8 or tuple(colors.shape) != (V, 4)):
        raise _lib.IdhError(f"render_shaded: colors must be a uint8 ({V},4) tensor on the GPU (got {colors.dtype} {tuple(colors.shape)} on {colors.device})")
    if attrs is not None and (attrs.dim() != 2 or attrs.shape[0] != V or not 1 <= attrs.shape[1] <= _lib.RASTER_MAX_ATTRS):
        raise _lib.IdhError(f"render_shaded: attrs {tuple(attrs.shape)} must be ({V},C) with 1 <= C <= {_lib.RASTER_MAX_ATTRS}")
    dev = verts.device
    f32 = faces.to(torch.int32).contiguous()  # no copy when they already are
    v, T, K = verts.contiguous(), cam_T_world_b44.contiguous(), K_b44.contiguous()
    col = None if colors is None else colors.contiguous()
    att = None if attrs is None else attrs.contiguous()
    C_ = 0 if att is None else att.shape[1]
    out = {"depth": torch.empty(B, 1, height, width, device=dev)}
    if col is not None:
        out["rgba"] = torch.empty(B, height, width, 4, device=dev, dtype=torch.uint8)
    if att is not None:
        out["attrs"] = torch.empty(B, height, width, C_, device=dev)
    if return_faces:
        out["pix_to_face"] = torch.empty(B, height, width, device=dev, dtype=torch.int32)
    if return_bary:
        out["bary"] = torch.empty(B, height, width, 3, device=dev)
    L = _lib.lib()
    nbytes = L.idh_raster_shaded_workspace_bytes(B, V, F, height, width)
    ws = torch.empty(max(nbytes, 256), device=dev, dtype=torch.uint8)
    a = _lib.RasterShadedArgs()
    a.verts_v3, a.faces_f3 = (_lib.ptr(v) if V else None), (_lib.ptr(f32) if F else None)
    a.cam_T_world_b44, a.K_b44, a.colors_v4, a.attrs_vc = T.data_ptr(), K.data_ptr(), _lib.ptr(col), _lib.ptr(att)
    a.depth_b1hw, a.pix_to_face_bhw, a.bary_bhw3 = out["depth"].data_ptr(), _lib.ptr(out.get("pix_to_face")), _lib.ptr(out.get("bary"))
    a.attr_out_bhwc, a.rgba_bhw4 = _lib.ptr(out.get("attrs")), _lib.ptr(out.get("rgba"))
    a.workspace, a.workspace_bytes, a.ambient, a.empty_depth = ws.data_ptr(), nbytes, float(ambient), float(empty_depth)
    a.V, a.F, a.B, a.H, a.W, a.C = V, F, B, int(height), int(width), C_
    _lib.check(L.idh_raster_shaded_fwd(C.byref(a), _lib.stream_ptr()), "idh_raster_shaded_fwd")
    return out


def _pose_f64(name, T) -> np.ndarray:
    T = np.asarray(T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else T, dtype=np.float64)
    if T.shape != (4, 4):
        raise _lib.IdhError(f"{name} {T.shape} must be (4,4)")
    return T


class AssetRenderer:
    """A virtual asset kept on the GPU and rendered into a moving camera: the producer of the ``asset_depth`` / ``asset_rgba`` pair of
    the live AR loop, which the reference reads from files rendered off line.  ``verts`` (V,3) in the asset's own
    frame, ``faces`` (F,3) (their int32 copy is made once), ``colors`` (V,4) uint8 or None (then only depth is rendered).
    ``world_T_asset`` places the asset in the world (default: identity); ``place`` moves it - e.g. onto the hit point of
    ``StreamingSession.raycast_view``.  The vertices are never rewritten: every render forms
    ``cam_T_mesh = float32(inv(world_T_cam) @ world_T_asset)`` in float64 on the host."""

    def __init__(self, verts, faces, colors=None, world_T_asset=None, ambient: float = 0.3, device="cuda"):
        self.verts, faces = _mesh(verts, faces, device)
        self.faces = faces.to(torch.int32)
        self.colors = None if colors is None else torch.as_tensor(colors).to(device=self.verts.device).contiguous()
        if self.colors is not None and (self.colors.dtype != torch.uint8 or tuple(self.colors.shape) != (self.verts.shape[0], 4)):
            raise _lib.IdhError(f"AssetRenderer: colors must be uint8 ({self.verts.shape[0]},4), got {self.colors.dtype} {tuple(self.colors.shape)}")
        self.ambient = float(ambient)
        self.world_T_asset = np.eye(4)
        if world_T_asset is not None:
            self.place(world_T_asset)

    def place(self, world_T_asset) -> None:
        """Move the asset: ``world_T_asset`` is a (4,4) array or tensor."""
        self.world_T_asset = _pose_f64("world_T_asset", world_T_asset)

    def cam_T_mesh(self, world_T_cam) -> torch.Tensor:
        """(1,4,4) float32 on the asset's device: the asset's frame to the camera at ``world_T_cam``, formed in float64."""
        T = np.linalg.inv(_pose_f64("world_T_cam", world_T_cam)) @ self.world_T_asset
        return torch.from_numpy(T.astype(np.float32))[None].to(self.verts.device)

    def render(self, world_T_cam, K, size, empty_depth: float = -1.0, **kw) -> Dict[str, torch.Tensor]:
        """``render_shaded`` of the asset in the one camera at ``world_T_cam`` ((4,4) array or tensor) with intrinsics ``K`` ((4,4) or
        (1,4,4), at ``size`` = (height, width)).  Keyword arguments (``attrs``, ``return_faces``, ``return_bary``) are passed on."""
        K = torch.as_tensor(K).to(device=self.verts.device, dtype=torch.float32)
        if K.dim() == 2:
            K = K[None]
        return render_shaded(self.verts, self.faces, self.cam_T_mesh(world_T_cam), K, int(size[0]), int(size[1]), colors=self.colors,
                             ambient=self.ambient, empty_depth=empty_depth, **kw)


def warp_depth(depth_m1hw, src_invK_m44, cam_T_src_bm44, K_b44, height, width, *, tear_ratio: float = 1.1, empty_depth: float = -1.0,
               return_source: bool = False) -> Dict[str, torch.Tensor]:
    """M depth maps ``depth_m1hw`` (M,1,h,w) - predictions of a ``DepthModel``, lidar frames, a ``BDModel``'s ``infer_depth`` result -
    warped into B cameras in one call (idh_depth_warp_fwd).  ``src_invK_m44`` (M,4,4): the sources' inverse intrinsics
    at h x w; ``cam_T_src_bm44`` (B,M,4,4): source camera frame to target camera frame (``relative_poses`` forms it in float64);
    ``K_b44`` (B,4,4): the targets' intrinsics at ``height`` x ``width``.  Every map is a triangulated surface over its pixel centres
    (include/idh_raster.h states the vertices and the two faces of a quad); a face whose three source depths are not all finite and
    positive, or whose largest exceeds ``tear_ratio`` (>= 1; ``inf`` never tears) times its smallest, is not drawn.  Returns

    * ``"depth"`` (B,1,height,width): the z in the target camera of the nearest surface any of the M sources remembers,
      ``empty_depth`` where none saw anything;
    * ``"source"`` (B,height,width) int32 with ``return_source``: ``m * 2 (h-1) (w-1) + face`` of the winner (``decode_source``), -1
      where empty; the lowest among exactly equal depths.

    Two calls return the same bits.  There is no CPU fallback."""
    _lib.require_cuda_f32(depth_m1hw, src_invK_m44, cam_T_src_bm44, K_b44)
    if depth_m1hw.dim() != 4 or depth_m1hw.shape[1] != 1:
        raise _lib.IdhError(f"warp_depth: depth {tuple(depth_m1hw.shape)} must be (M,1,h,w)")
    M, _, h, w = depth_m1hw.shape
    if tuple(src_invK_m44.shape) != (M, 4, 4):
        raise _lib.IdhError(f"warp_depth: src_invK {tuple(src_invK_m44.shape)} must be ({M},4,4)")
    if cam_T_src_bm44.dim() != 4 or tuple(cam_T_src_bm44.shape[1:]) != (M, 4, 4):
        raise _lib.IdhError(f"warp_depth: cam_T_src {tuple(cam_T_src_bm44.shape)} must be (B,{M},4,4)")
    B = cam_T_src_bm44.shape[0]
    if tuple(K_b44.shape) != (B, 4, 4):
        raise _lib.IdhError(f"warp_depth: K {tuple(K_b44.shape)} must be ({B},4,4)")
    height, width = int(height), int(width)
    d, iK, T, K = depth_m1hw.contiguous(), src_invK_m44.contiguous(), cam_T_src_bm44.contiguous(), K_b44.contiguous()
    L = _lib.lib()
    a = _lib.DepthWarpArgs()
    a.B, a.M, a.h, a.w, a.H, a.W = B, M, h, w, height, width
    a.tear_ratio, a.empty_depth = float(tear_ratio), float(empty_depth)
    nbytes = L.idh_depth_warp_workspace_bytes(B, M, h, w, height, width)
    if nbytes == 0:
        raise _lib.IdhError(f"warp_depth: B = {B}, M = {M}, height = {height} and width = {width} must be positive and the sources "
                            f"({h} x {w}) at least 2 x 2")
    out = {"depth": torch.empty(B, 1, height, width, device=d.device)}
    if return_source:
        out["source"] = torch.empty(B, height, width, device=d.device, dtype=torch.int32)
    ws = torch.empty(nbytes, device=d.device, dtype=torch.uint8)
    a.depth_m1hw, a.src_invK_m44, a.cam_T_src_bm44, a.K_b44 = d.data_ptr(), iK.data_ptr(), T.data_ptr(), K.data_ptr()
    a.depth_b1hw, a.source_bhw, a.workspace, a.workspace_bytes = out["depth"].data_ptr(), _lib.ptr(out.get("source")), ws.data_ptr(), nbytes
    _lib.check(L.idh_depth_warp_fwd(C.byref(a), _lib.stream_ptr()), "idh_depth_warp_fwd")
    return out


def decode_source(source, h: int, w: int):
    """``(m, i, j, upper)`` of ``warp_depth``'s ``"source"`` ids for sources of h x w pixels (a tensor gives int64 tensors, anything
    else int64 arrays): the source map, the quad's top-left vertex (row i, column j) and whether the face is the quad's second one,
    (v01, v10, v11), or its first, (v00, v10, v01).  All four are -1 where the id is -1 (nothing was hit)."""
    h, w = int(h), int(w)
    if h < 2 or w < 2:
        raise _lib.IdhError(f"decode_source: sources of {h} x {w} pixels have no faces")
    F = 2 * (h - 1) * (w - 1)
    s, where = (source.long(), torch.where) if isinstance(source, torch.Tensor) else (np.asarray(source, dtype=np.int64), np.where)
    empty = s < 0
    m, face = s // F, s % F
    q = face // 2
    parts = (m, q // (w - 1), q % (w - 1), face % 2)
    return tuple(where(empty, -1, p) for p in parts)


def relative_poses(world_T_cam_targets, world_T_src_sources) -> torch.Tensor:
    """(B,M,4,4) float32 on the host: ``float32(inv(world_T_cam[b]) @ world_T_src[m])`` formed in float64, as ``AssetRenderer.cam_T_mesh``
    does.  Both arguments are sequences of (4,4) arrays or tensors."""
    tgt = [np.linalg.inv(_pose_f64("world_T_cam", T)) for T in world_T_cam_targets]
    src = [_pose_f64("world_T_src", T) for T in world_T_src_sources]
    return torch.from_numpy(np.stack([np.stack([t @ s for s in src]) for t in tgt]).astype(np.float32))


def vertex_predictions(verts, cam_T_world_b44, K_b44, pred_11hw, depth_11hw, tolerance=DEPTH_TOLERANCE) -> torch.Tensor:
    """(V,) the prediction sampled at each projected vertex, -1 where the vertex is behind the camera, off the image, hidden
    (``depth_11hw`` is the mesh's own render) or the prediction is not positive (binary_metrics_utils.py:364-386)."""
    _lib.require_cuda_f32(verts, cam_T_world_b44, K_b44, pred_11hw, depth_11hw)
    H, W = depth_11hw.shape[-2:]
    if pred_11hw.numel() != H * W or depth_11hw.numel() != H * W or cam_T_world_b44.numel() != 16 or K_b44.numel() != 16:
        raise _lib.IdhError(f"vertex_predictions: one camera and (1,1,H,W) maps (got prediction {tuple(pred_11hw.shape)}, depth "
                            f"{tuple(depth_11hw.shape)}, cam_T_world {tuple(cam_T_world_b44.shape)})")
    v, T, K, p, d = (t.contiguous() for t in (verts, cam_T_world_b44, K_b44, pred_11hw, depth_11hw))
    out = torch.empty(v.shape[0], device=v.device)
    _lib.check(_lib.lib().idh_vertex_predictions_fwd(v.data_ptr(), v.shape[0], T.data_ptr(), K.data_ptr(), p.data_ptr(), d.data_ptr(), H, W,
                                                     float(tolerance), out.data_ptr(), _lib.stream_ptr()), "idh_vertex_predictions_fwd")
    return out


def vertex_occlusion_changes(history_tv: torch.Tensor) -> float:
    """sum over vertices and consecutive frames of |p[t+1] - p[t]| after the reference's quantisation (-1 -> unknown, > 0.5 -> 1,
    < 0.5 -> 0; binary_metrics_utils.py:273-279), counted on the GPU in integer units of 0.5.  Synchronises (it returns a host number,
    as the reference does)."""
    _lib.require_cuda_f32(history_tv)
    if history_tv.dim() != 2:
        raise _lib.IdhError(f"vertex_occlusion_changes: history {tuple(history_tv.shape)} must be (T,V)")
    h = history_tv.contiguous()
    out = torch.empty(1, device=h.device, dtype=torch.int64)
    _lib.check(_lib.lib().idh_vertex_occlusion_changes_fwd(h.data_ptr(), h.shape[0], h.shape[1], out.data_ptr(), _lib.stream_ptr()),
               "idh_vertex_occlusion_changes_fwd")
    return 0.5 * int(out.item())


class MeshDepthRasterizer:
    """The reference's ``Pytorch3DRasterizer(height, width)``.  ``mesh`` / ``gt_mesh`` are ``(verts (V,3) float32, faces (F,3) int64)``
    pairs in place of pytorch3d ``Meshes``.  The reference hard-codes 256 / 192 when it normalises the vertices' screen positions
    (:370-371); the instance's width / height are used here, which is the same at its default size."""

    def __init__(self, height: int = 192, width: int = 256):
        self.height, self.width = int(height), int(width)
        self.mesh: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self.faces: Optional[torch.Tensor] = None  # the plane's faces, built once
        self.gt_mesh: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self.gt_vertex_predictions: List[torch.Tensor] = []
        self._faces_i32 = self._gt_faces_i32 = None  # the kernel's int32 copies of faces / gt_mesh's faces, made once

    def load_gt_mesh(self, gt_mesh_path=None, verts=None, faces=None, device="cuda"):
        """The scene's ground-truth mesh from a PLY file (or from ``verts`` / ``faces`` directly)."""
        if gt_mesh_path is not None:
            verts, faces = load_ply(gt_mesh_path)
        self.gt_mesh = _mesh(verts, faces, device)
        self._gt_faces_i32 = self.gt_mesh[1].to(torch.int32)

    def create_plane_from_camera(self, world_T_cam_b44, distance=2.5):
        """The query plane: a 1024 x 1024 grid of 2.5 cm cells, fronto-parallel ``distance`` in front of the camera (the reference
        calls this argument cam_T_world_b44 and passes world_T_cam_b44, test_bd.py:174-176).  On the device of the pose."""
        vertices = plane_vertices(world_T_cam_b44, distance)
        if self.faces is None or self.faces.device != vertices.device:
            self.faces = plane_faces().to(vertices.device)
            self._faces_i32 = self.faces.to(torch.int32)
        self.mesh = (vertices.contiguous(), self.faces)

    def __call__(self, cam_T_world_b44, K_b44):
        if self.mesh is None:
            raise ValueError("Mesh has not been initialised for rendering!")
        return self.render_depth(cam_T_world_b44, K_b44)

    def render_depth(self, cam_T_world_b44, K_b44, mesh=None):
        """(B,1,height,width) depth of ``mesh`` (default: the plane) from the B cameras (binary_metrics_utils.py:336-358)."""
        verts, faces = self.mesh if mesh is None else mesh
        if faces is self.faces:
            faces = self._faces_i32
        elif self.gt_mesh is not None and faces is self.gt_mesh[1]:
            faces = self._gt_faces_i32
        return render_depth(verts, faces, cam_T_world_b44, K_b44, self.height, self.width)

    def update_gt_vertex_predictions(self, pred, cam_T_world_b44, K_b44):
        """Render the ground-truth mesh for visibility, sample ``pred`` (1,1,height,width) at its visible vertices and append the
        (V,) result to ``gt_vertex_predictions`` (binary_metrics_utils.py:360-388)."""
        if self.gt_mesh is None:
            raise ValueError("The ground-truth mesh has not been loaded!")
        rendered_depth = self.render_depth(cam_T_world_b44, K_b44, mesh=self.gt_mesh)
        self.gt_vertex_predictions.append(vertex_predictions(self.gt_mesh[0], cam_T_world_b44, K_b44, pred, rendered_depth))
