// Mesh extraction from the TSDF volume (include/idh_fusion.h): marching cubes to an indexed triangle mesh in a
// deterministic order, without an atomic counter.  The header states the semantics; the case table is csrc/mc_table.h (generated).
//
// Per voxel the workspace holds one 4-byte word {case, vertex on x, vertex on y, vertex on z} and one int32 vertex base.
//
//   count:  clear of the words
//           mesh_classify_k     A. one lane per cell, a wave along x.  The lane reads its eight voxels as four 16-byte loads (as the ray
//                               cast does); an emitted cell stores its case and stores the value 1 into the vertex byte of the owner
//                               of each of its crossed edges.  A crossed edge in a known cell makes that cell's case neither 0 nor
//                               255, so "crossed and in an emitted cell" is exactly what the up to four cells round an edge store,
//                               and since only the value 1 is ever stored between clears the concurrent byte stores need no atomic -
//                               the way integrate sets block flags.  (The alternative, a 3 x 3 x 3 neighbourhood of packed bits in
//                               LDS, needs a tile with an apron on three axes; the bytes replace it with stores only surface cells make.)
//           mesh_reduce_info_k  B1. per chunk of 1024 voxels: the sum of both counts, packed in one 64-bit word.
//           mesh_reduce_k       B1'. the same over 1024 sums, while there are more than 1024 of them.
//           mesh_scan_level_k   B2/B3. one workgroup scans the top level and writes the totals; the levels below are scanned per
//                               chunk with the chunk's base from the level above.
//           mesh_vbase_k        B3. per chunk: exclusive scan of the vertex counts plus the chunk's base -> the per-voxel vertex base.
//                               Chunks without a vertex are skipped (their bases are never read), and so does emit skip chunks
//                               without a vertex or a triangle: the scanned sums of two neighbouring chunks are equal there.
//   emit:   mesh_emit_k         C. per chunk: owners write their vertices; cells scan their triangle counts in the
//                               workgroup, add the chunk's base and write faces, whose indices are vertex_base[owner] + the rank of
//                               the axis among the owner's vertex bytes.  Every store is guarded by the capacities.
//
//   colours: mesh_colors_k      C'. the vertex half of C over again: the owner's and the far endpoint's {R, G, B, Wc} quads (16-byte
//                               loads) interpolated with the vertex's r and stored as one 4-byte word at the vertex's index.
//
// Every kernel is one pass over independent chunks: no workgroup waits on another.
#include "tsdf_common.h"

namespace {

#define IDH_MC_TABLE_ATTR __device__ const
#include "mc_table.h"

typedef unsigned long long u64;  // a pair of counts: vertices in the low 32 bits, triangles in the high 32 (neither sum reaches 2^31)

constexpr int kThreads = 256, kItems = 4, kChunk = kThreads * kItems;
constexpr int kMaxLevels = 4;
constexpr long long kMaxVoxels = 1ll << 28;

__device__ __forceinline__ u64 pack(unsigned v, unsigned f) { return (u64)v | ((u64)f << 32); }
__device__ __forceinline__ unsigned vertex_count(unsigned word) { return ((word >> 8) & 1u) + ((word >> 16) & 1u) + ((word >> 24) & 1u); }
__device__ __forceinline__ u64 counts_of(unsigned word) { return pack(vertex_count(word), mc_tri_count[word & 255u]); }

// exclusive prefix of `mine` over the workgroup's 256 threads, and the sum over all of them
__device__ __forceinline__ u64 block_scan(u64 mine, u64 &total) {
    __shared__ u64 wave_sum[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    u64 before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const u64 s = wave_sum[w];
        if (w < wave) before += s;
        total += s;
    }
    return before + (inc - mine);
}

struct ClassifyArgs {
    Vol V;
    unsigned char *info;  // 4 bytes per voxel
    float min_weight;
    int skip;
};

__global__ __launch_bounds__(256) void mesh_classify_k(const ClassifyArgs a) {
    const Vol &V = a.V;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, z = blockIdx.z;
    if (x >= V.Nx - 1 || y >= V.Ny - 1 || z >= V.Nz - 1) return;  // no cell: the word stays 0
    if (a.skip && !V.flags[((size_t)(z >> 3) * V.nby + (y >> 3)) * V.nbx + (x >> 3)]) return;  // no cell of the block is known
    const size_t row = (size_t)V.Nx, slice = row * V.Ny;
    const size_t i = (size_t)z * slice + (size_t)y * row + x;
    const float *p = V.values + 2 * i;
    const f4a8 c00 = *reinterpret_cast<const f4a8 *>(p);  // rows (y, z) = (0,0), (1,0), (0,1), (1,1); each {T_x0, W_x0, T_x1, W_x1}
    const f4a8 c10 = *reinterpret_cast<const f4a8 *>(p + 2 * row);
    const f4a8 c01 = *reinterpret_cast<const f4a8 *>(p + 2 * slice);
    const f4a8 c11 = *reinterpret_cast<const f4a8 *>(p + 2 * (slice + row));
    const float mw = a.min_weight;
    if (!(c00.y > mw && c00.w > mw && c10.y > mw && c10.w > mw && c01.y > mw && c01.w > mw && c11.y > mw && c11.w > mw)) return;
    const unsigned c = (unsigned)(c00.x <= 0.f) | (unsigned)(c00.z <= 0.f) << 1 | (unsigned)(c10.x <= 0.f) << 2 | (unsigned)(c10.z <= 0.f) << 3 |
                       (unsigned)(c01.x <= 0.f) << 4 | (unsigned)(c01.z <= 0.f) << 5 | (unsigned)(c11.x <= 0.f) << 6 | (unsigned)(c11.z <= 0.f) << 7;
    if (c == 0u || c == 255u) return;
    a.info[4 * i] = (unsigned char)c;
    // bit k of a mask: the edge that leaves corner k along the axis is crossed
    const unsigned mx = (c ^ (c >> 1)) & 0x55u, my = (c ^ (c >> 2)) & 0x33u, mz = (c ^ (c >> 4)) & 0x0fu;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        unsigned char *o = a.info + 4 * (i + (k & 1) + ((k >> 1) & 1) * row + (k >> 2) * slice);
        if ((mx >> k) & 1u) o[1] = 1;
        if ((my >> k) & 1u) o[2] = 1;
        if ((mz >> k) & 1u) o[3] = 1;
    }
}

// n4: the number of words, a multiple of 4 (the words past the last voxel are 0)
__global__ __launch_bounds__(256) void mesh_reduce_info_k(const uint4 *__restrict__ info, long long n4, u64 *__restrict__ out) {
    const long long i0 = blockIdx.x * (long long)kChunk + threadIdx.x * kItems;
    u64 mine = 0;
    if (i0 < n4) {
        const uint4 w = info[i0 >> 2];
        mine = counts_of(w.x) + counts_of(w.y) + counts_of(w.z) + counts_of(w.w);
    }
    u64 total;
    block_scan(mine, total);
    if (threadIdx.x == 0) out[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void mesh_reduce_k(const u64 *__restrict__ in, int count, u64 *__restrict__ out) {
    const int i0 = blockIdx.x * kChunk + threadIdx.x * kItems;
    u64 mine = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k)
        if (i0 + k < count) mine += in[i0 + k];
    u64 total;
    block_scan(mine, total);
    if (threadIdx.x == 0) out[blockIdx.x] = total;
}

// in place: data[i] <- the sum of what precedes it in its chunk, plus base[chunk]; the top level (one chunk) has no base and writes the totals
__global__ __launch_bounds__(256) void mesh_scan_level_k(u64 *__restrict__ data, int count, const u64 *__restrict__ base, int32_t *__restrict__ totals) {
    const int i0 = blockIdx.x * kChunk + threadIdx.x * kItems;
    u64 v0 = 0, v1 = 0, v2 = 0, v3 = 0;
    if (i0 < count) v0 = data[i0];
    if (i0 + 1 < count) v1 = data[i0 + 1];
    if (i0 + 2 < count) v2 = data[i0 + 2];
    if (i0 + 3 < count) v3 = data[i0 + 3];
    u64 total;
    u64 e = block_scan(v0 + v1 + v2 + v3, total);
    if (base) e += base[blockIdx.x];
    if (i0 < count) data[i0] = e;
    if (i0 + 1 < count) data[i0 + 1] = e + v0;
    if (i0 + 2 < count) data[i0 + 2] = e + v0 + v1;
    if (i0 + 3 < count) data[i0 + 3] = e + v0 + v1 + v2;
    if (totals && threadIdx.x == 0) totals[0] = (int32_t)(total & 0xffffffffull), totals[1] = (int32_t)(total >> 32);
}

__global__ __launch_bounds__(256) void mesh_vbase_k(const uint4 *__restrict__ info, long long n4, const u64 *__restrict__ base, int4 *__restrict__ vbase) {
    // a chunk without a vertex is left as it is: a base is only read at voxels that own one (the last chunk is never tested - its end
    // is not in the array)
    if (blockIdx.x + 1 < gridDim.x && (unsigned)base[blockIdx.x + 1] == (unsigned)base[blockIdx.x]) return;
    const long long i0 = blockIdx.x * (long long)kChunk + threadIdx.x * kItems;
    const bool live = i0 < n4;
    unsigned c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    if (live) {
        const uint4 w = info[i0 >> 2];
        c0 = vertex_count(w.x), c1 = vertex_count(w.y), c2 = vertex_count(w.z), c3 = vertex_count(w.w);
    }
    u64 total;
    const unsigned e = (unsigned)(block_scan(c0 + c1 + c2 + c3, total) + (base[blockIdx.x] & 0xffffffffull));
    if (live) vbase[i0 >> 2] = make_int4((int)e, (int)(e + c0), (int)(e + c0 + c1), (int)(e + c0 + c1 + c2));
}

struct EmitArgs {
    Vol V;
    const unsigned *info;
    const int32_t *vbase;
    const u64 *base;  // per chunk, after the scan: {vertices, triangles} before the chunk
    float *verts, *weights;
    int32_t *faces;
    long long n4, vcap, fcap;
};

// Four consecutive voxels per lane, as in the scan.  (Measured and dropped, profiles/mesh/README.md: one voxel per lane in workgroups
// of 1024, and issuing the fifteen gathers of a cell together instead of triangle by triangle - both slower.)
__global__ __launch_bounds__(256) void mesh_emit_k(const EmitArgs a) {
    const Vol &V = a.V;
    if (blockIdx.x + 1 < gridDim.x && a.base[blockIdx.x + 1] == a.base[blockIdx.x]) return;  // a chunk without a vertex or a triangle
    const long long i0 = blockIdx.x * (long long)kChunk + threadIdx.x * kItems;
    uint4 w = make_uint4(0, 0, 0, 0);
    if (i0 < a.n4) w = reinterpret_cast<const uint4 *>(a.info)[i0 >> 2];
    const unsigned tris = (unsigned)mc_tri_count[w.x & 255u] + mc_tri_count[w.y & 255u] + mc_tri_count[w.z & 255u] + mc_tri_count[w.w & 255u];
    u64 total;
    long long fi = (long long)block_scan(tris, total);
    if ((w.x | w.y | w.z | w.w) == 0u) return;  // nothing owned, nothing emitted (the words past the last voxel are 0)
    fi += (long long)(a.base[blockIdx.x] >> 32);
    const int4 vb = reinterpret_cast<const int4 *>(a.vbase)[i0 >> 2];
    const long long row = V.Nx, slice = row * V.Ny;
    int x = (int)(i0 % row), y = (int)((i0 / row) % V.Ny), z = (int)(i0 / slice);
    const float2 *values = reinterpret_cast<const float2 *>(V.values);
    for (int k = 0; k < kItems; ++k) {
        const unsigned word = k == 0 ? w.x : k == 1 ? w.y : k == 2 ? w.z : w.w;
        const long long i = i0 + k;
        if (word >> 8) {  // this voxel owns vertices
            const float2 ta = values[i];
            long long vi = k == 0 ? vb.x : k == 1 ? vb.y : k == 2 ? vb.z : vb.w;
            const float px = V.ox + V.v * (float)x, py = V.oy + V.v * (float)y, pz = V.oz + V.v * (float)z;
            for (int axis = 0; axis < 3; ++axis) {
                if (!((word >> (8 + 8 * axis)) & 1u)) continue;
                const float2 tb = values[i + (axis == 0 ? 1 : axis == 1 ? row : slice)];
                const float r = ta.x / (ta.x - tb.x);
                if (vi < a.vcap) {
                    float *o = a.verts + 3 * vi;
                    o[0] = axis == 0 ? V.ox + V.v * ((float)x + r) : px;
                    o[1] = axis == 1 ? V.oy + V.v * ((float)y + r) : py;
                    o[2] = axis == 2 ? V.oz + V.v * ((float)z + r) : pz;
                    if (a.weights) a.weights[vi] = ta.y + r * (tb.y - ta.y);
                }
                ++vi;
            }
        }
        const unsigned c = word & 255u;
        const int nt = mc_tri_count[c];
        for (int t = 0; t < nt; ++t, ++fi) {
            if (fi >= a.fcap) break;  // and every later face of the lane: fi only grows
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int e = mc_tri_edges[c][3 * t + q];
                const int axis = e >> 2, j0 = e & 1, j1 = (e >> 1) & 1;
                // the lower corner's two other coordinates, in x < y < z order
                const long long owner = i + (axis == 0 ? j0 * row + j1 * slice : axis == 1 ? j0 + j1 * slice : j0 + j1 * row);
                const unsigned ow = a.info[owner];
                const int rank = axis == 0 ? 0 : axis == 1 ? (int)((ow >> 8) & 1u) : (int)(((ow >> 8) & 1u) + ((ow >> 16) & 1u));
                a.faces[3 * fi + q] = a.vbase[owner] + rank;
            }
        }
        if (++x == V.Nx) {
            x = 0;
            if (++y == V.Ny) y = 0, ++z;
        }
    }
}

struct ColorsArgs {
    Vol V;
    const unsigned *info;
    const int32_t *vbase;
    const u64 *base;
    const float4 *colors;  // {R, G, B, Wc} per voxel
    unsigned *rgba;        // one word per vertex: bytes R, G, B, A in memory order
    long long n4, vcap;
};

__device__ __forceinline__ unsigned channel_byte(float c) { return (unsigned)(int)(fminf(fmaxf(c, 0.f), 255.f) + 0.5f); }
__device__ __forceinline__ unsigned pack_rgba(float r, float g, float b) { return channel_byte(r) | channel_byte(g) << 8 | channel_byte(b) << 16 | 255u << 24; }

// The vertex half of mesh_emit_k over again, for the colours: same chunks, same four voxels per lane, same vertex indices.
__global__ __launch_bounds__(256) void mesh_colors_k(const ColorsArgs a) {
    const Vol &V = a.V;
    if (blockIdx.x + 1 < gridDim.x && (unsigned)a.base[blockIdx.x + 1] == (unsigned)a.base[blockIdx.x]) return;  // a chunk without a vertex
    const long long i0 = blockIdx.x * (long long)kChunk + threadIdx.x * kItems;
    if (i0 >= a.n4) return;
    const uint4 w = reinterpret_cast<const uint4 *>(a.info)[i0 >> 2];
    if (((w.x | w.y | w.z | w.w) >> 8) == 0u) return;  // nothing owned
    const int4 vb = reinterpret_cast<const int4 *>(a.vbase)[i0 >> 2];
    const long long row = V.Nx, slice = row * V.Ny;
    const float2 *values = reinterpret_cast<const float2 *>(V.values);
    for (int k = 0; k < kItems; ++k) {
        const unsigned word = k == 0 ? w.x : k == 1 ? w.y : k == 2 ? w.z : w.w;
        if (!(word >> 8)) continue;
        const long long i = i0 + k;
        const float Ta = values[i].x;
        const float4 ca = a.colors[i];
        long long vi = k == 0 ? vb.x : k == 1 ? vb.y : k == 2 ? vb.z : vb.w;
        for (int axis = 0; axis < 3; ++axis) {
            if (!((word >> (8 + 8 * axis)) & 1u)) continue;
            const long long j = i + (axis == 0 ? 1 : axis == 1 ? row : slice);
            const float Tb = values[j].x;
            const float4 cb = a.colors[j];
            const float r = Ta / (Ta - Tb);
            unsigned out = 0u;
            if (ca.w > 0.f && cb.w > 0.f) out = pack_rgba(ca.x + r * (cb.x - ca.x), ca.y + r * (cb.y - ca.y), ca.z + r * (cb.z - ca.z));
            else if (ca.w > 0.f) out = pack_rgba(ca.x, ca.y, ca.z);
            else if (cb.w > 0.f) out = pack_rgba(cb.x, cb.y, cb.z);
            if (vi < a.vcap) a.rgba[vi] = out;
            ++vi;
        }
    }
}

struct MeshLayout {
    long long n, n4;
    int levels;              // levels of partial sums, >= 1; the last one has at most kChunk entries
    long long p[kMaxLevels];  // entries per level
    size_t info_off, vbase_off, level_off[kMaxLevels], bytes;
};

bool mesh_layout(int Nz, int Ny, int Nx, MeshLayout &L) {
    if (Nz < 2 || Ny < 2 || Nx < 2) return false;
    L.n = (long long)Nz * Ny * Nx;
    if (L.n > kMaxVoxels) return false;
    L.n4 = (L.n + 3) & ~3ll;
    L.info_off = 0, L.vbase_off = (size_t)L.n4 * 4;
    size_t off = (size_t)L.n4 * 8;
    L.levels = 0;
    long long p = L.n4;
    do {
        p = (p + kChunk - 1) / kChunk;
        L.p[L.levels] = p, L.level_off[L.levels] = off;
        off += (size_t)p * 8;
        ++L.levels;
    } while (p > kChunk && L.levels < kMaxLevels);
    L.bytes = off;
    return p <= kChunk;
}

// what the calls check, in the header's order; `outputs`: the call has its non-null outputs
int check_mesh(const idh_tsdf_mesh_args *args, bool outputs, bool bad_capacity, Vol &V, MeshLayout &L) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_tsdf_mesh_args)) return IDH_EINVAL;
    const idh_tsdf_mesh_args &e = *args;
    if (!(e.min_weight >= 0.f)) return IDH_EINVAL;  // also refuses NaN
    if (!outputs) return IDH_EINVAL;
    if (bad_capacity) return IDH_EINVAL;
    if (const int rc = check_volume(e.volume, V)) return rc;
    if (!mesh_layout(e.volume.Nz, e.volume.Ny, e.volume.Nx, L)) return IDH_EUNSUPPORTED;
    if (!e.workspace || e.workspace_bytes < 0 || (size_t)e.workspace_bytes < L.bytes) return IDH_EWORKSPACE;
    if ((uintptr_t)e.workspace & 15u) return IDH_EINVAL;
    return IDH_OK;
}

}  // namespace

extern "C" size_t idh_sizeof_tsdf_mesh_args(void) { return sizeof(idh_tsdf_mesh_args); }

extern "C" size_t idh_tsdf_mesh_workspace_bytes(int Nz, int Ny, int Nx) {
    MeshLayout L;
    return mesh_layout(Nz, Ny, Nx, L) ? L.bytes : 0;
}

extern "C" int idh_tsdf_mesh_count_fwd(const idh_tsdf_mesh_args *args, void *stream) {
    Vol V;
    MeshLayout L;
    if (const int rc = check_mesh(args, args && args->totals, false, V, L)) return rc;
    hipStream_t st = idh_stream(stream);
    char *ws = static_cast<char *>(args->workspace);
    if (hipMemsetAsync(ws + L.info_off, 0, (size_t)L.n4 * 4, st) != hipSuccess) return IDH_ELAUNCH;
    ClassifyArgs c;
    c.V = V, c.info = reinterpret_cast<unsigned char *>(ws + L.info_off), c.min_weight = args->min_weight, c.skip = args->use_block_flags != 0;
    hipLaunchKernelGGL(mesh_classify_k, dim3(idh_cdiv(V.Nx, 64), idh_cdiv(V.Ny, 4), V.Nz), dim3(64, 4), 0, st, c);
    IDH_CHECK_LAUNCH();
    const uint4 *info = reinterpret_cast<const uint4 *>(ws + L.info_off);
    u64 *level[kMaxLevels];
    for (int k = 0; k < L.levels; ++k) level[k] = reinterpret_cast<u64 *>(ws + L.level_off[k]);
    hipLaunchKernelGGL(mesh_reduce_info_k, dim3((unsigned)L.p[0]), dim3(kThreads), 0, st, info, L.n4, level[0]);
    IDH_CHECK_LAUNCH();
    for (int k = 1; k < L.levels; ++k) {
        hipLaunchKernelGGL(mesh_reduce_k, dim3((unsigned)L.p[k]), dim3(kThreads), 0, st, level[k - 1], (int)L.p[k - 1], level[k]);
        IDH_CHECK_LAUNCH();
    }
    const int top = L.levels - 1;
    hipLaunchKernelGGL(mesh_scan_level_k, dim3(1), dim3(kThreads), 0, st, level[top], (int)L.p[top], (const u64 *)nullptr, args->totals);
    IDH_CHECK_LAUNCH();
    for (int k = top - 1; k >= 0; --k) {
        hipLaunchKernelGGL(mesh_scan_level_k, dim3((unsigned)L.p[k + 1]), dim3(kThreads), 0, st, level[k], (int)L.p[k], (const u64 *)level[k + 1], (int32_t *)nullptr);
        IDH_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(mesh_vbase_k, dim3((unsigned)L.p[0]), dim3(kThreads), 0, st, info, L.n4, (const u64 *)level[0], reinterpret_cast<int4 *>(ws + L.vbase_off));
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" int idh_tsdf_mesh_emit_fwd(const idh_tsdf_mesh_args *args, void *stream) {
    Vol V;
    MeshLayout L;
    if (const int rc = check_mesh(args, args && args->verts_v3 && args->faces_f3, args && (args->vert_capacity < 0 || args->face_capacity < 0), V, L)) return rc;
    if (args->vert_capacity == 0 && args->face_capacity == 0) return IDH_OK;
    char *ws = static_cast<char *>(args->workspace);
    EmitArgs a;
    a.V = V, a.info = reinterpret_cast<const unsigned *>(ws + L.info_off), a.vbase = reinterpret_cast<const int32_t *>(ws + L.vbase_off);
    a.base = reinterpret_cast<const u64 *>(ws + L.level_off[0]);
    a.verts = args->verts_v3, a.weights = args->weights_v, a.faces = args->faces_f3;
    a.n4 = L.n4, a.vcap = args->vert_capacity, a.fcap = args->face_capacity;
    hipLaunchKernelGGL(mesh_emit_k, dim3((unsigned)L.p[0]), dim3(kThreads), 0, idh_stream(stream), a);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}

extern "C" size_t idh_sizeof_tsdf_mesh_colors_args(void) { return sizeof(idh_tsdf_mesh_colors_args); }

extern "C" int idh_tsdf_mesh_colors_fwd(const idh_tsdf_mesh_colors_args *args, void *stream) {
    if (!args || args->struct_size < (int64_t)sizeof(idh_tsdf_mesh_colors_args)) return IDH_EINVAL;
    const idh_tsdf_mesh_args &m = args->mesh;
    Vol V;
    MeshLayout L;
    if (const int rc = check_mesh(&m, args->colors_zyx4 && args->rgba_v4, m.vert_capacity < 0, V, L)) return rc;
    if ((uintptr_t)args->colors_zyx4 & 15u) return IDH_EINVAL;
    if (m.vert_capacity == 0) return IDH_OK;
    char *ws = static_cast<char *>(m.workspace);
    ColorsArgs a;
    a.V = V, a.info = reinterpret_cast<const unsigned *>(ws + L.info_off), a.vbase = reinterpret_cast<const int32_t *>(ws + L.vbase_off);
    a.base = reinterpret_cast<const u64 *>(ws + L.level_off[0]);
    a.colors = reinterpret_cast<const float4 *>(args->colors_zyx4), a.rgba = reinterpret_cast<unsigned *>(args->rgba_v4);
    a.n4 = L.n4, a.vcap = m.vert_capacity;
    hipLaunchKernelGGL(mesh_colors_k, dim3((unsigned)L.p[0]), dim3(kThreads), 0, idh_stream(stream), a);
    IDH_CHECK_LAUNCH();
    return IDH_OK;
}
