/*
 * idh_fusion.h — TSDF fusion of depth maps, the ray cast of the fused surface into live cameras, its extraction as a triangle mesh and
 * the alignment of a depth map's camera against it (additive: idh_version() stays as it is; every struct is versioned through its
 * struct_size; csrc/tsdf.hip, csrc/tsdf_mesh.hip, csrc/tsdf_align.hip).
 *
 * The depth warp of idh_raster.h draws remembered maps as separate sheets under one z-buffer: maps are not combined, holes stay holes
 * and the memory is as long as the ring.  Here every map is averaged into a truncated signed distance volume (Curless and Levoy) - the
 * step the reference's workflow takes off line with open3d ("for mesh fusion") before --temporal_eval - and a live camera ray-casts it.
 *
 * Conventions shared with the rest of the library: OpenCV intrinsics fx = K[0][0], fy = K[1][1], cx = K[0][2], cy = K[1][2]; pixel
 * (row i, column j) has its centre at (j + 0.5, i + 0.5), the convention of BackprojectDepth (utils/geometry_utils.py:39,60-61), so the
 * pixel that holds image point (px, py) is (floor(py), floor(px)); device pointers, dense fp32, caller-owned storage, `stream` a
 * hipStream_t, asynchronous, IDH_OK or a negative IDH_E* code.  Arguments are validated on the host before anything is launched.
 * All device arithmetic is fp32 without contraction, in the order written below.
 *
 * The volume
 *   dims (Nz, Ny, Nx), axis-aligned with the world; voxel (x, y, z) has its centre at origin + voxel_size * (x, y, z);
 *   values (Nz, Ny, Nx, 2) fp32, x fastest among voxels: the pair {T, W} - truncated signed distance in units of the truncation
 *   distance, in [-1, 1], and the number of observations.  An empty volume holds {1, 0} everywhere.
 *   trunc = trunc_voxels * voxel_size (one fp32 multiply).
 *   block_flags: one byte per 8 x 8 x 8 block of CELLS (cell (x, y, z) is the cube between voxels (x..x+1, y..y+1, z..z+1); an axis of
 *   N voxels has N - 1 cells and (N + 6) / 8 blocks, the last one partial), (NBz, NBy, NBx), x fastest.  The guarantee: a block whose
 *   byte is 0 has W == 0 at EVERY voxel any of its cells reads (its 8 x 8 x 8 cells read 9 x 9 x 9 voxels) - no sample inside it is
 *   known.  This is a superset of "some voxel there has W > 0 and T < 1": the ray cast's flag bits 2 and 4 count known samples, and
 *   observed free space (W > 0, T == 1) is known, so only blocks without any observation can be jumped without changing a bit.
 *   Bytes are set by idh_tsdf_integrate_fwd, rebuilt by idh_tsdf_flags_fwd (and by idh_tsdf_shift_fwd on the volume it writes), cleared
 *   by idh_tsdf_reset_fwd alone.
 */
#ifndef IDH_FUSION_H_
#define IDH_FUSION_H_

#include <stddef.h>
#include <stdint.h>

#include "idh.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define IDH_TSDF_MAX_MAPS 16      /* M of one integrate call: pipeline.MAX_RING_CAPACITY */
#define IDH_TSDF_MAX_CAMERAS 128  /* B of one ray cast */
#define IDH_TSDF_MAX_STEPS 65536  /* max_steps of one ray cast (the range clip of `skip` is exact up to this lattice length) */

#define IDH_TSDF_HIT 1          /* flags: a surface crossing was found */
#define IDH_TSDF_NONE_KNOWN 2   /* no sample up to the end was known */
#define IDH_TSDF_SOME_KNOWN 4   /* some but not all samples up to the end were known */
#define IDH_TSDF_NO_NORMAL 8    /* a hit whose cell is not known or whose gradient is zero (only with normals_b3hw) */

typedef struct idh_tsdf_volume {
    int64_t struct_size;       /* sizeof(idh_tsdf_volume) of the caller's header (must be >= the library's) */
    float *values;             /* (Nz,Ny,Nx,2) {T, W} */
    uint8_t *block_flags;      /* idh_tsdf_block_flag_bytes(Nz, Ny, Nx) bytes */
    int64_t block_flag_bytes;  /* what the caller allocated */
    float origin[3];           /* world (x, y, z) of the centre of voxel (0,0,0) */
    float voxel_size;          /* > 0, finite */
    float trunc_voxels;        /* > 0, finite */
    int32_t Nz, Ny, Nx;        /* each >= 2; Nz * Ny * Nx < 2^31 */
} idh_tsdf_volume;

typedef struct idh_tsdf_integrate_args {
    int64_t struct_size;
    idh_tsdf_volume volume;
    const float *depth_m1hw;       /* (M,1,h,w) */
    const float *K_m44;            /* (M,4,4) intrinsics at h x w, row-major */
    const float *cam_T_world_m44;  /* (M,4,4) */
    float max_weight;              /* >= 1, finite */
    int32_t M, h, w;
} idh_tsdf_integrate_args;

typedef struct idh_tsdf_raycast_args {
    int64_t struct_size;
    idh_tsdf_volume volume;
    const float *world_T_cam_b44;  /* (B,4,4) */
    const float *invK_b44;         /* (B,4,4) inverse intrinsics at H x W */
    float *depth_b1hw;             /* out (B,1,H,W) */
    uint8_t *flags_bhw;            /* out (B,H,W) */
    float *normals_b3hw;           /* out (B,3,H,W), or NULL */
    float near;                    /* >= 0, finite: t of sample 0 */
    float step_voxels;             /* in (0, 1] */
    float empty_depth;             /* written to depth where there is no hit */
    int32_t max_steps;             /* 1 .. IDH_TSDF_MAX_STEPS */
    int32_t world_normals;         /* 0: normals in the camera's frame, 1: in the world's */
    int32_t skip;                  /* 0: the plain march over every sample, 1: range clip and block jumps (same bits) */
    int32_t B, H, W;
} idh_tsdf_raycast_args;

/* sizeof(...) as compiled into the library (bindings assert their mirrors match). */
size_t idh_sizeof_tsdf_volume(void);
size_t idh_sizeof_tsdf_integrate_args(void);
size_t idh_sizeof_tsdf_raycast_args(void);

/* Bytes of the block flags of a (Nz, Ny, Nx) volume: ((Nz + 6) / 8) * ((Ny + 6) / 8) * ((Nx + 6) / 8).  0 if a dim is < 2. */
size_t idh_tsdf_block_flag_bytes(int Nz, int Ny, int Nx);

/* What every entry point below checks of its volume, in this order.
 * IDH_EINVAL: struct_size short, a dim < 2, voxel_size or trunc_voxels not finite and > 0, an origin component not finite, values NULL;
 * IDH_EUNSUPPORTED: Nz * Ny * Nx >= 2^31, Nz > 65535 or Ny > 262140 (the launch grid's limits);
 * IDH_EWORKSPACE: block_flags NULL or block_flag_bytes < idh_tsdf_block_flag_bytes(Nz, Ny, Nx) - the caller-owned side storage is
 * answered like a short workspace everywhere else in the library. */

/* Every voxel to {1, 0}, every block flag to 0.  IDH_EINVAL also for vol == NULL. */
int idh_tsdf_reset_fwd(const idh_tsdf_volume *vol, void *stream);

/* Rebuild the block flags from the values (for a pair tensor made elsewhere): a block's byte is 1 iff W > 0 at some voxel its cells read. */
int idh_tsdf_flags_fwd(const idh_tsdf_volume *vol, void *stream);

/* M depth maps into the volume, one launch, one lane per voxel.  Per voxel (x, y, z), for m = 0 .. M - 1 in this order:
 *   p = origin + voxel_size * (x, y, z)                                  (per component: one multiply, one add)
 *   c = R p + t from cam_T_world[m]: c.x = ((r00 p.x + r01 p.y) + r02 p.z) + t.x, likewise y, z;   skip unless c.z > 0
 *   px = fx * (c.x / c.z) + cx,  py = fy * (c.y / c.z) + cy;  tap (i, j) = (floor(py), floor(px));
 *   skip unless 0 <= px < w and 0 <= py < h and d = depth[m, i, j] is finite and > 0                (the validity rule of the warp)
 *   sdf = d - c.z   (projective, along the camera's z);  skip if sdf < -trunc;  s = min(1, sdf / trunc)
 *   T <- (W * T + s) / (W + 1);   W <- min(W + 1, max_weight)
 * The lane keeps {T, W} in registers over the M maps: it loads them when the first map touches the voxel and stores them once; a
 * voxel no map touches reads and writes nothing of the volume.  So two calls return the same bits, and one call with M maps equals M
 * calls with one map each, bit for bit.  Flags of the blocks a touched voxel belongs to are set to 1 (plain byte stores of one value).
 * IDH_EINVAL: args NULL, struct_size short, M, h or w <= 0, max_weight < 1 or not finite, a null input; the volume's conditions;
 * IDH_EUNSUPPORTED: M > IDH_TSDF_MAX_MAPS, h * w >= 2^31 / M. */
int idh_tsdf_integrate_fwd(const idh_tsdf_integrate_args *args, void *stream);

/* The fused surface in B cameras, one launch, one lane per pixel, 8 x 8-pixel tiles per wave.  Per pixel (i, j) of camera b:
 *   q = invK[:3,:3] (j + 0.5, i + 0.5, 1): q.x = (k00 u + k01 v) + k02, ...;  n = sqrt((q.x q.x + q.y q.y) + q.z q.z);  dc = q / n
 *   dir = R dc (as c above, without t), o = t from world_T_cam;   og = (o - origin) / voxel_size,  dg = dir / voxel_size  (per component)
 *   step = step_voxels * voxel_size;  sample k = 0 .. max_steps - 1:  t_k = near + (float)k * step,  g = og + t_k * dg,  cell = floor(g)
 *   the sample is KNOWN when 0 <= cell <= N - 2 on the three axes and the eight voxels cell + {0,1}^3 all have W > 0; then with
 *   r = g - cell:  along x  a_yz = T_yz0 + r.x * (T_yz1 - T_yz0),  then y  b_z = a_0z + r.y * (a_1z - a_0z),  then z  f = b_0 + r.z * (b_1 - b_0)
 *   HIT: the first k >= 1 with samples k - 1 and k known, f_{k-1} > 0 and f_k <= 0:
 *        t* = t_{k-1} + step * (f_{k-1} / (f_{k-1} - f_k));   depth = t* * dc.z   (the camera's z of the point; no further refinement)
 *   A ray that starts behind a surface, or enters one from unobserved space, does not hit there and marches on.
 *   flags: IDH_TSDF_HIT; with "the end" = the hit's k (samples 0 .. k) or max_steps (all samples): IDH_TSDF_NONE_KNOWN when none of them
 *   was known, IDH_TSDF_SOME_KNOWN when some but not all were; no hit and neither bit: the ray crossed observed free space only.
 *   depth = empty_depth when there is no hit.
 *   normals (optional): at a hit, g* = og + t* dg and its cell; if that cell is known, the gradient of the interpolant there,
 *        G.x = lerp_z(lerp_y(T001 - T000, T011 - T010), lerp_y(T101 - T100, T111 - T110))   (Tzyx; lerp(a, b) = a + r (b - a)),
 *        G.y = lerp_z(lerp_x(T010 - T000, T011 - T001), lerp_x(T110 - T100, T111 - T101)),
 *        G.z = lerp_y(lerp_x(T100 - T000, T101 - T001), lerp_x(T110 - T010, T111 - T011)),
 *        N = G / sqrt((G.x G.x + G.y G.y) + G.z G.z), negated if N . dir > 0 (towards the camera); world_normals == 0 stores R^T N.
 *        Zero, with IDH_TSDF_NO_NORMAL set, when the cell is not known or G is zero; zero where there is no hit.
 * skip: the lattice range is clipped to the volume's box and blocks whose flag is 0 are jumped to the first lattice sample that may
 * lie past them; every sample left out is one the plain march finds not known, so both marches return the same bits.
 * IDH_EINVAL: args NULL, struct_size short, B, H or W <= 0, max_steps <= 0, step_voxels outside (0, 1] or NaN, near < 0 or not finite,
 * empty_depth NaN, a null world_T_cam / invK / depth / flags; the volume's conditions;
 * IDH_EUNSUPPORTED: B > IDH_TSDF_MAX_CAMERAS, B * H * W >= 2^31, max_steps > IDH_TSDF_MAX_STEPS. */
int idh_tsdf_raycast_fwd(const idh_tsdf_raycast_args *args, void *stream);

/* ---- Mesh extraction: marching cubes over the volume to an indexed triangle mesh (csrc/tsdf_mesh.hip) ----------
 *
 * Voxel values are compared as stored; no arithmetic decides topology.
 *   A voxel is INSIDE when T <= 0 (the ray cast's f_{k-1} > 0, f_k <= 0) and KNOWN when W > min_weight (min_weight = 0: the ray cast's
 *   W > 0).  A cell is KNOWN when its eight voxels are, and EMITTED when it is known and its case is neither 0 nor 255.
 *   Corner c = dx + 2 dy + 4 dz of a cell; case bit c is set when corner c is inside.  Cube edge e = 4 * axis + j, axis 0/1/2 = x/y/z,
 *   j = first + 2 * second of the edge's lower corner's two other coordinates in x < y < z order.  The grid edge from voxel a to
 *   a + axis is OWNED by a.  The triangles of a case come from the table csrc/mc_table.h, generated by tools/gen_mc_table.py.
 * Vertices.  One on every owned edge with exactly one endpoint inside that at least one emitted cell contains (no orphans, none
 *   missing), ordered by ascending linear index of the owner ((z * Ny + y) * Nx + x), then axis.  With a the owner and b = a + axis:
 *     r = T_a / (T_a - T_b)                                     (the denominator cannot be zero)
 *     along the axis   origin + voxel_size * ((float)idx + r);   the other two   origin + voxel_size * (float)idx
 *     weights (optional)   W_a + r * (W_b - W_a)
 * Faces.  int32 triples of vertex indices, ordered by ascending linear index of the cell, then table order.  The right-hand normal
 *   (v1 - v0) x (v2 - v0) points to the positive (free-space) side: a closed surface around an inside region has positive signed volume.
 *   Degenerate triangles (a vertex at r = 0 or r = 1) are kept.
 * Order and bits are deterministic: two extractions return equal arrays.
 *
 * Two calls.  idh_tsdf_mesh_count_fwd classifies every cell, scans the per-voxel vertex and triangle counts (a three-phase scan:
 * per-workgroup sums, a scan of the sums, the bases added back; no workgroup waits on another) and leaves the totals {V, F} in
 * `totals` and what the second call needs in `workspace`.  The caller reads the totals, allocates, and idh_tsdf_mesh_emit_fwd - same
 * volume, min_weight and workspace - writes the first vert_capacity vertices and the first face_capacity faces: every store is guarded
 * by the capacities, so a stale total cannot write out of bounds.
 * use_block_flags: cells of a block whose flag is 0 are not read (none of them is known); the arrays are the same either way. */
typedef struct idh_tsdf_mesh_args {
    int64_t struct_size;
    idh_tsdf_volume volume;
    void *workspace;          /* idh_tsdf_mesh_workspace_bytes(Nz, Ny, Nx) bytes, 16-byte aligned */
    int64_t workspace_bytes;  /* what the caller allocated */
    int32_t *totals;          /* count: out, 2 x int32 {V, F} on the device; emit: not read */
    float *verts_v3;          /* emit: out (vert_capacity, 3); count: not read */
    int32_t *faces_f3;        /* emit: out (face_capacity, 3); count: not read */
    float *weights_v;         /* emit: out (vert_capacity), or NULL */
    int64_t vert_capacity;    /* >= 0 */
    int64_t face_capacity;    /* >= 0 */
    float min_weight;         /* >= 0 */
    int32_t use_block_flags;  /* 0: every cell is read; 1: blocks whose flag is 0 are skipped (same arrays) */
} idh_tsdf_mesh_args;

size_t idh_sizeof_tsdf_mesh_args(void);

/* With n = Nz * Ny * Nx rounded up to a multiple of 4 and p_1 = ceil(n / 1024), p_{k+1} = ceil(p_k / 1024) while p_k > 1024:
 * 8 n + 8 (p_1 + p_2 + ...) bytes - four bytes of {case, vertex on x, y, z} and a four-byte vertex base per voxel, and the scan's
 * partial sums.  0 if a dim is < 2 or Nz * Ny * Nx > 2^28. */
size_t idh_tsdf_mesh_workspace_bytes(int Nz, int Ny, int Nx);

/* Both calls - IDH_EINVAL: args NULL, struct_size short, min_weight negative or NaN, a null output (count: totals; emit: verts_v3 or
 * faces_f3), a negative capacity (emit); the volume's conditions; IDH_EUNSUPPORTED: Nz * Ny * Nx > 2^28 (int32 indices cannot overflow
 * at five triangles per cell); IDH_EWORKSPACE: workspace NULL or workspace_bytes < idh_tsdf_mesh_workspace_bytes(Nz, Ny, Nx);
 * IDH_EINVAL: workspace not 16-byte aligned. */
int idh_tsdf_mesh_count_fwd(const idh_tsdf_mesh_args *args, void *stream);
int idh_tsdf_mesh_emit_fwd(const idh_tsdf_mesh_args *args, void *stream);

/* ---- Colour: camera frames fused next to the depth, ray-cast and meshed with the surface (csrc/tsdf.hip, csrc/tsdf_mesh.hip) ----
 *
 * colors (Nz, Ny, Nx, 4) fp32, caller-owned and laid out like `values`: the quad {R, G, B, Wc} per voxel, 16 bytes, 16-byte aligned -
 * R, G, B in units of a uint8 channel (0 .. 255), Wc the number of colour observations.  The EMPTY state is all-zero bytes: a memset
 * (hipMemsetAsync, tensor.zero_()) resets it; idh_tsdf_reset_fwd does not know the tensor and leaves it alone.  No entry point above
 * reads or writes it: idh_tsdf_integrate_fwd on a coloured volume (lidar, depth-only maps) leaves `colors` as it is, so Wc <= W holds
 * at every voxel of a volume filled through these calls with one max_weight.
 * Frames are uint8 RGB (M, hc, wc, 3), the frame convention of idh_ingest.h and idh_composite.h, with intrinsics of their own. */
typedef struct idh_tsdf_integrate_color_args {
    int64_t struct_size;
    idh_tsdf_volume volume;
    const float *depth_m1hw;       /* (M,1,h,w) */
    const float *K_m44;            /* (M,4,4) intrinsics at h x w, row-major */
    const float *cam_T_world_m44;  /* (M,4,4) */
    float max_weight;              /* >= 1, finite: caps W and Wc */
    int32_t M, h, w;
    float *colors_zyx4;            /* (Nz,Ny,Nx,4) {R, G, B, Wc}, 16-byte aligned */
    const uint8_t *color_mhw3;     /* (M,hc,wc,3) RGB frames, frame m taken with depth map m */
    const float *color_K_m44;      /* (M,4,4) intrinsics at hc x wc */
    int32_t hc, wc;
} idh_tsdf_integrate_color_args;

typedef struct idh_tsdf_raycast_color_args {
    int64_t struct_size;
    idh_tsdf_volume volume;
    const float *world_T_cam_b44;  /* the fields of idh_tsdf_raycast_args, with their meaning */
    const float *invK_b44;
    float *depth_b1hw;
    uint8_t *flags_bhw;
    float *normals_b3hw;           /* or NULL */
    float near;
    float step_voxels;
    float empty_depth;
    int32_t max_steps;
    int32_t world_normals;
    int32_t skip;
    int32_t B, H, W;
    const float *colors_zyx4;      /* (Nz,Ny,Nx,4), 16-byte aligned */
    uint8_t *rgba_bhw4;            /* out (B,H,W,4): the layout of idh_raster_shaded_fwd's rgba */
} idh_tsdf_raycast_color_args;

typedef struct idh_tsdf_mesh_colors_args {
    int64_t struct_size;
    idh_tsdf_mesh_args mesh;       /* volume, min_weight and workspace of the count call before it; vert_capacity; the rest is not read */
    const float *colors_zyx4;      /* (Nz,Ny,Nx,4), 16-byte aligned */
    uint8_t *rgba_v4;              /* out (vert_capacity, 4) */
} idh_tsdf_mesh_colors_args;

size_t idh_sizeof_tsdf_integrate_color_args(void);
size_t idh_sizeof_tsdf_raycast_color_args(void);
size_t idh_sizeof_tsdf_mesh_colors_args(void);

/* idh_tsdf_integrate_fwd with a colour frame per map, one launch, one lane per voxel.  For m = 0 .. M - 1 the {T, W} update of the
 * voxel is exactly the one stated there; immediately after the voxel's {T, W} update for map m (so only where map m updated it):
 *   skip the colour unless sdf <= trunc                               (free space in front of the band carries no colour)
 *   qx = fxc * (c.x / c.z) + cxc,  qy = fyc * (c.y / c.z) + cyc       (color_K[m]; the quotients are those of px and py)
 *   skip unless 0 <= qx < wc and 0 <= qy < hc;   tap (floor(qy), floor(qx)),  c = its three bytes converted to float
 *   per channel   C <- (Wc * C + c) / (Wc + 1);   then   Wc <- min(Wc + 1, max_weight)
 * The lane keeps {R, G, B, Wc} in registers over the M maps: one 16-byte load at the first map that colours the voxel, one 16-byte
 * store at the end; a voxel no map colours reads and writes nothing of `colors`.
 * Promises: `values` and `block_flags` after this call equal, bit for bit, what idh_tsdf_integrate_fwd leaves for the same maps; two
 * calls return the same bits; one call with M maps equals M calls with one map each, bit for bit, colours included.
 * Codes: those of idh_tsdf_integrate_fwd, and with its IDH_EINVAL conditions (before the volume's) also a null colors_zyx4, color_mhw3
 * or color_K_m44, hc <= 0 or wc <= 0, colors_zyx4 not 16-byte aligned; with its IDH_EUNSUPPORTED conditions also hc * wc >= 2^31 / M. */
int idh_tsdf_integrate_color_fwd(const idh_tsdf_integrate_color_args *args, void *stream);

/* idh_tsdf_raycast_fwd with the surface's colour.  The march, depth, flags and normals are the ones stated there, bit for bit, with
 * skip 0 and 1.  Colour is formed once per pixel, at the hit:
 *   g* = og + t* dg, its cell and r = g* - cell, exactly as for the normals; if the cell is in range (0 <= cell <= N - 2 per axis),
 *   over its corners c = 0 .. 7 (c = dx + 2 dy + 4 dz) in this order, only those with Wc > 0:
 *     w = ((dx ? r.x : 1 - r.x) * (dy ? r.y : 1 - r.y)) * (dz ? r.z : 1 - r.z);   num += w * C (per channel);   den += w
 *   den > 0: each channel (uint8)(int)(min(max(num / den, 0), 255) + 0.5f), alpha 255
 *   no hit, a cell out of range or den == 0: the four bytes are 0.
 * The known rule W > 0 plays no part in the colour and there is no new flag bit: alpha says whether there is a colour.
 * Codes: those of idh_tsdf_raycast_fwd, and with its null checks (before the volume's conditions) IDH_EINVAL for a null colors_zyx4 or
 * rgba_bhw4 or colors_zyx4 not 16-byte aligned. */
int idh_tsdf_raycast_color_fwd(const idh_tsdf_raycast_color_args *args, void *stream);

/* The colours of the vertices idh_tsdf_mesh_emit_fwd writes, after idh_tsdf_mesh_count_fwd on the same volume, min_weight and
 * workspace (before or after the emit call; that call is not changed).  One pass over the workspace's chunks.  An owner a with a vertex
 * on `axis` has the index it has in emit; with b = a + axis:
 *   r = T_a / (T_a - T_b)                                             (the expression of emit)
 *   both endpoints with Wc > 0:  C = C_a + r * (C_b - C_a) per channel;   one endpoint with Wc > 0: that endpoint's colour;
 *   rounding and alpha as in the ray cast;   neither: four zero bytes.
 * Every store is guarded by mesh.vert_capacity.
 * Codes: IDH_EINVAL for args NULL or struct_size short; then those of the two mesh calls in their order, where the null outputs are
 * colors_zyx4 and rgba_v4 (verts_v3, faces_f3 and totals are not read) and the capacity is vert_capacity; IDH_EINVAL also for
 * colors_zyx4 not 16-byte aligned. */
int idh_tsdf_mesh_colors_fwd(const idh_tsdf_mesh_colors_args *args, void *stream);

/* ---- Per-observation weights (csrc/tsdf.hip) -----------------------------------------------------------------------
 *
 * idh_tsdf_integrate_color_fwd with a weight per depth sample: weight_m1hw (M,1,h,w) is tapped where the depth is, g = weight[m, i, j].
 *   skip the observation entirely - like a hole - unless g is finite and > 0
 *   T <- (W * T + g * s) / (W + g);   W <- min(W + g, max_weight)
 *   colour, under the conditions stated there, with the same g:   C <- (Wc * C + g * c) / (Wc + g);   Wc <- min(Wc + g, max_weight)
 * colors_zyx4, color_mhw3 and color_K_m44 may be NULL, all three together: geometry only, hc and wc are not read and `colors` is left
 * as it is (idh_tsdf_integrate_fwd with weights).
 * Promises: with every weight 1.0f, `values`, `block_flags` and `colors` equal, bit for bit, what the unweighted calls leave (1 * s == s
 * and the build does not contract); two calls return the same bits; one call with M maps equals M calls with one map each.
 * Codes: those of idh_tsdf_integrate_color_fwd in its order (the colour conditions only when a colour pointer is given, where a null
 * one among the three is IDH_EINVAL), and IDH_EINVAL for a null weight_m1hw. */
typedef struct idh_tsdf_integrate_weighted_args {
    int64_t struct_size;
    idh_tsdf_volume volume;
    const float *depth_m1hw;       /* the fields of idh_tsdf_integrate_color_args, with their meaning */
    const float *K_m44;
    const float *cam_T_world_m44;
    float max_weight;
    int32_t M, h, w;
    float *colors_zyx4;            /* or NULL (then all three) */
    const uint8_t *color_mhw3;
    const float *color_K_m44;
    int32_t hc, wc;
    const float *weight_m1hw;      /* (M,1,h,w) */
} idh_tsdf_integrate_weighted_args;

size_t idh_sizeof_tsdf_integrate_weighted_args(void);

int idh_tsdf_integrate_weighted_fwd(const idh_tsdf_integrate_weighted_args *args, void *stream);

/* ---- A volume that follows the camera: shift by whole voxels (csrc/tsdf.hip) -------------------------------------------
 *
 * The grid moves under its contents: `dst` is a second volume of the same dims, voxel_size and trunc_voxels whose origin lies
 * shift = (sx, sy, sz) voxels further along the world's axes, and every world lattice point both grids hold keeps what was fused there.
 * What `src` holds outside `dst` is dropped (the caller keeps it first if it wants it); what `dst` holds outside `src` is empty.
 * One launch after the clear of dst's flags, one lane per voxel of dst.  Per voxel (x, y, z) of dst:
 *   a = (x + sx, y + sy, z + sz)                                          (in 64-bit: no shift overflows)
 *   a inside src and W_src(a) > 0:   the pair {T, W} of dst is the pair of src at a, bit for bit, and the quad {R, G, B, Wc} likewise
 *   otherwise:                       the pair is {1, 0} and the quad sixteen zero bytes
 * A voxel of src with W == 0 (or NaN) therefore arrives in the EMPTY state whatever its T and its quad were: no consumer reads T or the
 * colour of such a voxel, and dst is a function of what the consumers can see of src.  shift = (0,0,0) is a normalising copy; |s| >= N on
 * an axis leaves dst empty.  Every byte of dst's values (and colours) is written, and dst's first idh_tsdf_block_flag_bytes(Nz, Ny, Nx)
 * flag bytes equal what idh_tsdf_flags_fwd would leave on dst's new values: 1 iff W > 0 at some voxel the block's cells read (cleared,
 * then plain byte stores of 1).  src is only read.  No allocation, no synchronisation, no host read-back; two calls return the same bits.
 * The colours are optional, both pointers or neither.
 * Codes, in this order.
 * IDH_EINVAL: args NULL, struct_size short; exactly one of src_colors_zyx4 and dst_colors_zyx4 NULL; a colour pointer not 16-byte aligned;
 * src's volume conditions, then dst's, with their codes;
 * IDH_EINVAL: Nz, Ny, Nx, voxel_size or trunc_voxels of the two differ (the floats compared as bits);
 *   dst.origin[i] is not, bit for bit, src.origin[i] + voxel_size * (float)shift[i] (one fp32 multiply, one fp32 add) - the data cannot
 *   move without the frame;
 *   one of src's byte ranges - values, the flag bytes named above, colours - overlaps one of dst's (ping-pong, never in place). */
typedef struct idh_tsdf_shift_args {
    int64_t struct_size;
    idh_tsdf_volume src;           /* read */
    idh_tsdf_volume dst;           /* written: values and block_flags, every byte of both */
    const float *src_colors_zyx4;  /* (Nz,Ny,Nx,4), 16-byte aligned, or NULL */
    float *dst_colors_zyx4;        /* (Nz,Ny,Nx,4), 16-byte aligned; NULL iff src_colors_zyx4 is NULL */
    int32_t shift[3];              /* (sx, sy, sz) voxels, any int32 */
} idh_tsdf_shift_args;

size_t idh_sizeof_tsdf_shift_args(void);

int idh_tsdf_shift_fwd(const idh_tsdf_shift_args *args, void *stream);

/* ---- Pose alignment: fit a depth map's camera to the fused volume (csrc/tsdf_align.hip) ---------------------------------
 *
 * Frame-to-model alignment on the signed distance field itself (Bylow et al. 2013): Gauss-Newton on the sum of f(T p)^2 over the map's
 * back-projected points, with the interpolant f and its gradient G of the ray cast above.  No data association, no rendered map.
 * The pose is kept in fp64 (R, t) in the workspace, initialised from world_T_cam_in_44; every iteration is two launches - a per-pixel
 * pass with a chunked fp64 reduction and a one-workgroup solve - and the call enqueues 2 * iters launches without any host
 * synchronisation or read-back.
 *
 * Per pixel (i, j) with i % stride == 0 and j % stride == 0, against the iteration's pose ROUNDED TO fp32 (R, t below are those floats):
 *   d = depth[i, j]: skip unless finite and > 0;  wm = weight[i, j]: skip unless finite and > 0 (wm = 1 without a weight map)
 *   q = invK[:3,:3] (j + 0.5, i + 0.5, 1) as in the ray cast, not normalised;   pc = q * d (per component)
 *   pw = R pc + t in the order of the integrate's c: pw.x = ((r00 pc.x + r01 pc.y) + r02 pc.z) + t.x, ...
 *   g = (pw - origin) / voxel_size (per component);  cell = floor(g);  skip unless the cell is KNOWN (the ray cast's rule)
 *   f and G by the ray cast's expressions with r = g - cell;   skip when (G.x G.x + G.y G.y) + G.z G.z == 0 (a saturated cell)
 *   r = f * trunc (metres);   n = G * trunc_voxels (per component);   a = pw - t (per component)
 *   J = (n.x, n.y, n.z, a.y n.z - a.z n.y, a.z n.x - a.x n.z, a.x n.y - a.y n.x): the derivative of r under
 *       pw' = t + v + exp(w^)(pw - t) at (v, w) = 0 - the increment translates the camera and rotates it about its own centre
 *   wgt = wm * (huber <= 0 || |r| <= huber ? 1 : huber / |r|)
 * The system, in fp64 from the eight floats widened: A_ab += (wgt J_a) J_b for a <= b (21 entries, row-major upper triangle),
 *   b_a += (wgt J_a) r,  cost += (wgt r) r,  count += 1.
 * Reduction: the selected pixels (ceil(h / stride) x ceil(w / stride) of them) are cut into 16 x 16 chunks, whatever the grid; a lane
 * holds one pixel, a wave an 8 x 8 quarter, summed by shuffles (offsets 32 .. 1) and then over the four waves in order; one record of
 * 29 doubles per chunk; the solve adds record c into slot c % 8 in ascending c and then the slots in ascending order.  No atomics:
 * the same bits for every max_workgroups and every call.
 * The solve, fp64:  status 1 if count < min_count.  Else A' = A + damping * diag(A), Cholesky A' = L L^T with pivots
 *   p_k = A'_kk - sum_{j<k} L_kj^2; status 2 unless every p_k > min_pivot_ratio * A'_kk (an exactly planar volume has p_0 == 0).
 *   Else xi = -(A')^-1 b = (v, w);  R <- E R with E = I + (sin th / th) w^ + ((1 - cos th) / th^2) w^ w^, th = |w| (E = I + w^ below
 *   th = 1e-12);  t <- t + v;  status 0.
 *   After a non-zero status, or a status-0 step with |v| < min_step and |w| < min_step, the remaining iterations return at once (a flag
 *   in the workspace); their records are zero but for status 3.
 * Outputs.  world_T_cam_out_44: the fp64 pose rounded once, bottom row 0 0 0 1 (the input's bits after status 1 or 2 at iteration 0).
 *   records (iters, 40) doubles: [0..20] A, [21..26] b, [27] cost, [28] count, [29] status, [30] |v|, [31] |w|, [32..37] xi, [38..39] 0.
 *   rows_hw8 (optional): (h, w, 8) fp32 (J[6], r, wgt) of iteration 0 - the input pose; all zero for a pixel skipped or not selected.
 * IDH_EINVAL: args NULL, struct_size short, h or w <= 0, iters outside 1 .. IDH_TSDF_ALIGN_MAX_ITERS, stride < 1, min_count < 6,
 *   max_workgroups < 0, huber NaN or infinite, damping or min_step negative or not finite, min_pivot_ratio outside [0, 1), a null
 *   depth / invK / pose in / pose out / records, workspace not 8-byte or rows_hw8 not 16-byte aligned; the volume's conditions;
 * IDH_EUNSUPPORTED: h * w >= 2^31;   IDH_EWORKSPACE: workspace NULL or workspace_bytes < idh_tsdf_align_workspace_bytes(h, w, stride, iters). */
#define IDH_TSDF_ALIGN_MAX_ITERS 64
#define IDH_TSDF_ALIGN_RECORD 40  /* doubles per iteration's record */

typedef struct idh_tsdf_align_args {
    int64_t struct_size;
    idh_tsdf_volume volume;
    const float *depth_11hw;          /* (1,1,h,w) */
    const float *invK_44;             /* inverse intrinsics at h x w */
    const float *weight_11hw;         /* (1,1,h,w), or NULL */
    const float *world_T_cam_in_44;   /* the pose to start from */
    float *world_T_cam_out_44;        /* out (4,4); may be the input's address */
    double *records_i40;              /* out (iters, 40) */
    float *rows_hw8;                  /* out (h,w,8), 16-byte aligned, or NULL */
    void *workspace;                  /* idh_tsdf_align_workspace_bytes(h, w, stride, iters) bytes, 8-byte aligned */
    int64_t workspace_bytes;          /* what the caller allocated */
    double damping;                   /* >= 0, finite */
    double min_step;                  /* >= 0, finite; metres and radians */
    double min_pivot_ratio;           /* in [0, 1); 1e-6 is the bindings' default */
    float huber;                      /* metres; <= 0: none */
    int32_t h, w;
    int32_t iters;                    /* 1 .. IDH_TSDF_ALIGN_MAX_ITERS */
    int32_t stride;                   /* >= 1 */
    int32_t min_count;                /* >= 6 */
    int32_t max_workgroups;           /* of the per-pixel pass; 0: one per chunk */
} idh_tsdf_align_args;

size_t idh_sizeof_tsdf_align_args(void);

/* 8 * (16 + 32 * chunks) bytes with chunks = ceil(ceil(h / stride) / 16) * ceil(ceil(w / stride) / 16): the pose state and one record per
 * chunk (reused by every iteration).  0 if h, w or stride < 1, iters outside 1 .. IDH_TSDF_ALIGN_MAX_ITERS or h * w >= 2^31. */
size_t idh_tsdf_align_workspace_bytes(int h, int w, int stride, int iters);

int idh_tsdf_align_fwd(const idh_tsdf_align_args *args, void *stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* IDH_FUSION_H_ */
