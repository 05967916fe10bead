// Surface meshes of label volumes and scalar fields, gfx950: marching tetrahedra on the Kuhn (6-tetrahedron) split of the
// cells of the padded grid, welded and closed (rule pinned in ctunet_amd/mesh.py; tests/mesh_ref.py restates it in numpy).
//
// A CELL ROW is the W+1 cells of one (cz, cy) of the padded grid; rows in C order are the blocks of the numbering, so
// "cells in C order" is "rows in order, then x".  The workspace keeps the rows at a stride of WCP = W+1 rounded up to 16
// cells (the pad cells hold code 0), so every lane's 16 cells are 16-byte aligned in every per-cell array.
//   1. count   one wave per cell row, a lane owns 16 cells along x per step: it reads the 16 voxels of each of the row's four
//              voxel rows as 16 inside bits per voxel row (mask16 of voxel_rows.h: 16-byte loads where the 16 voxels are
//              aligned, voxel by voxel otherwise), gets the 17th (the voxel left of its first) from the lane below, and
//              forms each cell's 8-bit inside code (bit dz*4 + dy*2 + dx).  Per cell it writes the
//              code (1 byte; the 7-bit crossing mask of the owned edges is a function of it, edge_mask()) and the packed
//              exclusive prefix of (vertices, triangles) within the row (uint32: low 16 / high 16 bits; a row has at most
//              7 * 1025 vertices and 12 * 1025 triangles), from a wave scan of the lanes' sums.  Per row: the packed total.
//   2. scan    one block of SB threads: exclusive int64 scan of the row totals in row order (block_exclusive_scan of scan.h,
//              a thread owns ceil(rows / SB) consecutive rows: the second level) -> int32 vertex and face base per row,
//              int64 totals (V, F) at the head of the workspace for the host to read.
//   3. emit    two launches, a thread owns the same 16 cells: vertices (owner cell: t and the position, contraction off) and
//              faces (vertex id = vbase[row'] + prefix[cell'] + popcount(mask[cell'] & ((1 << k) - 1)) through a table of
//              (owner offset, edge slot) per (tetrahedron, case, triangle, corner) that make_tables() derives at compile
//              time from the 16-case rule, winding included).
//   4. measure per-face area and signed volume term in float64, block sums in thread order, one fixed-order final sum;
//              optionally the unit normals.
// No atomics anywhere; every position is decided by the scan.  Measured: profiles/mesh.md.
//
// No reference counterpart: the reference writes NIfTI volumes only.
#include "common.h"
#include "scan.h"
#include "voxel_rows.h"

#pragma clang fp contract(off)

namespace {

using ctu_vox::MAX_SIDE;

constexpr int CB = 256;                         // count block: CB / 64 cell rows
constexpr int VPT = 16;                         // cells of a lane per step (and of a thread of the emit kernels)
constexpr int SB = CTU_MESH_SCAN_BLOCK;         // scan block
constexpr int EB = 256;                         // emit block
constexpr int MB = 256;                         // measure block
constexpr int MAX_MB = CTU_MESH_MEASURE_WS / 16;  // measure blocks: two doubles each

// owned edge slot k -> the cell corner (dz*4 + dy*2 + dx) at its far end, and back
constexpr int SLOT_CORNER[7] = {1, 2, 4, 3, 5, 6, 7};
constexpr int CORNER_SLOT[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
// the six tetrahedra: permutations (a, b, c) of the axes (z, y, x) = (0, 1, 2) in lexicographic order
constexpr int PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
constexpr int AXIS_BIT[3] = {4, 2, 1};

struct Tables {
    uint32_t tri[6][16][2];                     // bit 31: valid; corner j of the triangle: bits 6j..6j+5 = offset << 3 | slot
    uint8_t ntri[256];                          // triangles of a cell by its inside code
};

constexpr int popc4(int c) { return (c & 1) + ((c >> 1) & 1) + ((c >> 2) & 1) + ((c >> 3) & 1); }

// vertex on the lattice edge between path corners j1 and j2 of a tetrahedron: who owns it, and twice its position at
// t = 1/2 in (x, y, z)
struct EdgeRef { int code, x, y, z; };
constexpr EdgeRef edge_ref(const int corner[4], int j1, int j2) {
    const int lo = corner[j1 < j2 ? j1 : j2], hi = corner[j1 < j2 ? j2 : j1];
    return {lo << 3 | CORNER_SLOT[hi ^ lo], (lo & 1) + (hi & 1), ((lo >> 1) & 1) + ((hi >> 1) & 1), (lo >> 2) + (hi >> 2)};
}

// one triangle with its first corner kept and the other two ordered so that the right-hand normal, in (x, y, z), points
// from the inside corners of the tetrahedron to the outside ones
constexpr uint32_t wind(const int corner[4], int cs, EdgeRef a, EdgeRef b, EdgeRef c) {
    const int ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
    const int nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    int in[3] = {0, 0, 0}, out[3] = {0, 0, 0}, nin = 0;
    for (int j = 0; j < 4; ++j) {
        int* s = (cs >> j) & 1 ? in : out;
        s[0] += corner[j] & 1;
        s[1] += (corner[j] >> 1) & 1;
        s[2] += corner[j] >> 2;
        nin += (cs >> j) & 1;
    }
    // (centroid of the outside corners - centroid of the inside ones) * nin * nout
    const int nout = 4 - nin;
    const int dot = nx * (nin * out[0] - nout * in[0]) + ny * (nin * out[1] - nout * in[1]) + nz * (nin * out[2] - nout * in[2]);
    return dot > 0 ? (0x80000000u | a.code | b.code << 6 | c.code << 12) : (0x80000000u | a.code | c.code << 6 | b.code << 12);
}

constexpr Tables make_tables() {
    Tables t{};
    for (int p = 0; p < 6; ++p) {
        const int c1 = AXIS_BIT[PERM[p][0]];
        const int corner[4] = {0, c1, c1 | AXIS_BIT[PERM[p][1]], 7};
        for (int cs = 1; cs < 15; ++cs) {
            const int n = popc4(cs);
            if (n == 2) {
                int in[2] = {0, 0}, out[2] = {0, 0}, ni = 0, no = 0;
                for (int j = 0; j < 4; ++j) {
                    if ((cs >> j) & 1) in[ni++] = j;
                    else out[no++] = j;
                }
                const EdgeRef a = edge_ref(corner, in[0], out[0]), b = edge_ref(corner, in[0], out[1]),
                              c = edge_ref(corner, in[1], out[1]), d = edge_ref(corner, in[1], out[0]);
                t.tri[p][cs][0] = wind(corner, cs, a, b, c);
                t.tri[p][cs][1] = wind(corner, cs, a, c, d);
            } else {
                const int want = n == 1 ? 1 : 0;                // the lone corner is the inside one, or the outside one
                int lone = 0, o[3] = {0, 0, 0}, no = 0;
                for (int j = 0; j < 4; ++j) {
                    if (((cs >> j) & 1) == want) lone = j;
                    else o[no++] = j;
                }
                t.tri[p][cs][0] = wind(corner, cs, edge_ref(corner, lone, o[0]), edge_ref(corner, lone, o[1]),
                                       edge_ref(corner, lone, o[2]));
            }
        }
    }
    for (int code = 0; code < 256; ++code) {
        int n = 0;
        for (int p = 0; p < 6; ++p) {
            const int c1 = AXIS_BIT[PERM[p][0]], c2 = c1 | AXIS_BIT[PERM[p][1]];
            const int cs = (code & 1) | ((code >> c1) & 1) << 1 | ((code >> c2) & 1) << 2 | ((code >> 7) & 1) << 3;
            n += (t.tri[p][cs][0] >> 31) + (t.tri[p][cs][1] >> 31);
        }
        t.ntri[code] = (uint8_t)n;
    }
    return t;
}

__constant__ Tables TAB = make_tables();

// the owned edges whose two ends differ in insideness: bit k for slot k
__device__ __forceinline__ uint32_t edge_mask(uint32_t code) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) m |= (((code >> SLOT_CORNER[k]) ^ code) & 1u) << k;
    return m;
}

struct MeshArgs {
    int D, H, W;
    int Hc, Wc, Wcp, nrows;                     // cells: (D+1) x Hc x Wc, row stride Wcp
    int has_label;
    long long label;
    float level, fill;
    float sp[3], org[3];
    long long* totals;                          // (V, F)
    int* rowv;                                  // [nrows] vertex base of a row
    int* rowf;                                  // [nrows] face base of a row
    uint32_t* rowtot;                           // [nrows] vertices | triangles << 16 of a row
    uint8_t* code;                              // [nrows * Wcp]
    uint32_t* pre;                              // [nrows * Wcp] exclusive prefix within the row, packed like rowtot
};

struct Layout { size_t rowv, rowf, rowtot, code, pre, total; };
Layout layout(int D, int H, int W) {
    const size_t nrows = (size_t)(D + 1) * (H + 1), ncp = nrows * (size_t)((W + 1 + VPT - 1) / VPT * VPT);
    Layout l;
    size_t o = 256;                             // the totals
    l.rowv = o;   o += align256(nrows * 4);
    l.rowf = o;   o += align256(nrows * 4);
    l.rowtot = o; o += align256(nrows * 4);
    l.code = o;   o += align256(ncp);
    l.pre = o;    o += align256(ncp * 4);
    l.total = o;
    return l;
}

bool shape_ok(int D, int H, int W) {
    return ctu_vox::sides_ok(D, H, W) && (int64_t)(D + 1) * (H + 1) * (W + 1) < ((int64_t)1 << 31);
}

// ------------------------------------------------------------------------------------------------ 1. count
template <class T>
__global__ void __launch_bounds__(CB) mesh_count_kernel(MeshArgs a, const T* __restrict__ vol) {
    __shared__ uint8_t ntri[256];
    ntri[threadIdx.x] = TAB.ntri[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (CB / 64) + (threadIdx.x >> 6);
    if (row >= a.nrows) return;                                    // wave-uniform
    const int cz = row / a.Hc, cy = row - cz * a.Hc;
    // voxel row r = dz*2 + dy of the cell row: (cz - 1 + dz, cy - 1 + dy), absent outside the volume
    const T* vrow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int z = cz - 1 + (r >> 1), y = cy - 1 + (r & 1);
        vrow[r] = (z >= 0 && z < a.D && y >= 0 && y < a.H) ? vol + ((int64_t)z * a.H + y) * a.W : nullptr;
    }
    const ctu_vox::Inside inside{{a.has_label, a.label}, a.level};
    uint32_t carry[4] = {0, 0, 0, 0};                              // bit of the voxel left of lane 0's first
    uint32_t run = 0;                                              // packed (vertices, triangles) of the cells so far
    uint8_t* crow = a.code + (int64_t)row * a.Wcp;
    uint32_t* prow = a.pre + (int64_t)row * a.Wcp;
    for (int xb = 0; xb < a.Wcp; xb += 64 * VPT) {
        const int x0 = xb + lane * VPT;                            // first cell; its corner dx = 0 is voxel x0 - 1
        uint32_t ext[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            // inside bits of voxels x0 .. x0+15 of the voxel row (bit i for x0 + i; 0 outside the row)
            const uint32_t b = (vrow[r] && x0 < a.W) ? ctu_vox::mask16(vrow[r] + x0, min(a.W - x0, VPT), inside) : 0u;
            const uint32_t below = __shfl_up(b >> (VPT - 1), 1);
            ext[r] = b << 1 | (lane ? below : carry[r]);
            carry[r] = __shfl(b >> (VPT - 1), 63);
        }
        uint32_t codes[VPT / 4] = {0, 0, 0, 0};
        uint32_t cnt[VPT];
        uint32_t sum = 0;
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const uint32_t c = ((ext[0] >> i) & 3u) | ((ext[1] >> i) & 3u) << 2 | ((ext[2] >> i) & 3u) << 4 | ((ext[3] >> i) & 3u) << 6;
            codes[i >> 2] |= c << (8 * (i & 3));
            cnt[i] = sum;
            sum += (uint32_t)__popc(edge_mask(c)) | (uint32_t)ntri[c] << 16;
        }
        uint32_t s = sum;                                          // inclusive scan of the lanes' sums
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(s, o);
            if (lane >= o) s += y;
        }
        const uint32_t base = run + s - sum;
        run += __shfl(s, 63);
        if (x0 < a.Wcp) {
            *reinterpret_cast<uint4*>(crow + x0) = make_uint4(codes[0], codes[1], codes[2], codes[3]);
#pragma unroll
            for (int q = 0; q < VPT / 4; ++q)
                *reinterpret_cast<uint4*>(prow + x0 + 4 * q) =
                    make_uint4(base + cnt[4 * q], base + cnt[4 * q + 1], base + cnt[4 * q + 2], base + cnt[4 * q + 3]);
        }
    }
    if (lane == 0) a.rowtot[row] = run;
}

// ------------------------------------------------------------------------------------------------ 2. scan
__global__ void __launch_bounds__(SB) mesh_scan_kernel(MeshArgs a) {
    __shared__ long long lds[SB / 64];
    const int per = (a.nrows + SB - 1) / SB;
    const int r0 = min((int)threadIdx.x * per, a.nrows), r1 = min(r0 + per, a.nrows);
    long long sv = 0, sf = 0;
    for (int r = r0; r < r1; ++r) {
        const uint32_t t = a.rowtot[r];
        sv += t & 0xFFFFu;
        sf += t >> 16;
    }
    long long tv, tf;
    long long ov = block_exclusive_scan(sv, lds, tv);
    long long of = block_exclusive_scan(sf, lds, tf);
    for (int r = r0; r < r1; ++r) {
        const uint32_t t = a.rowtot[r];
        a.rowv[r] = (int)ov;                                       // meaningful while the totals are below 2^31: emit
        a.rowf[r] = (int)of;                                       // refuses anything else
        ov += t & 0xFFFFu;
        of += t >> 16;
    }
    if (threadIdx.x == 0) {
        a.totals[0] = tv;
        a.totals[1] = tf;
    }
}

// ------------------------------------------------------------------------------------------------ 3. emit
// value of the padded point (pz, py, px): the voxel (pz-1, py-1, px-1), or the fill value on the virtual layer
__device__ __forceinline__ float point_value(const float* __restrict__ vol, int pz, int py, int px, const MeshArgs& a) {
    const int z = pz - 1, y = py - 1, x = px - 1;
    if ((unsigned)z >= (unsigned)a.D || (unsigned)y >= (unsigned)a.H || (unsigned)x >= (unsigned)a.W) return a.fill;
    return vol[((int64_t)z * a.H + y) * a.W + x];
}

// FIELD: the corner values are the float32 volume's; otherwise 1 / 0 by the inside code (fill 0)
template <bool FIELD>
__global__ void __launch_bounds__(EB) mesh_vertices_kernel(MeshArgs a, const float* __restrict__ vol, float* __restrict__ vert) {
    const int64_t g = (int64_t)blockIdx.x * EB + threadIdx.x;
    const int64_t c0 = g * VPT;
    if (c0 >= (int64_t)a.nrows * a.Wcp) return;
    const uint4 cw = *reinterpret_cast<const uint4*>(a.code + c0);
    const uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
    bool any = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) any |= w[q] != 0u && w[q] != 0xFFFFFFFFu;
    if (!any) return;
    const int row = (int)(c0 / a.Wcp), x0 = (int)(c0 - (int64_t)row * a.Wcp);
    const int cz = row / a.Hc, cy = row - cz * a.Hc;
    const int vb = a.rowv[row];
    for (int i = 0; i < VPT; ++i) {
        const uint32_t code = a.code[c0 + i];
        if (code == 0u || code == 255u) continue;
        const uint32_t m = edge_mask(code);
        const int cx = x0 + i;
        float* out = vert + ((int64_t)vb + (a.pre[c0 + i] & 0xFFFFu)) * 3;
        const float v0 = FIELD ? point_value(vol, cz, cy, cx, a) : (float)(code & 1u);
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            if (!((m >> k) & 1u)) continue;
            const int cr = SLOT_CORNER[k], dz = cr >> 2, dy = (cr >> 1) & 1, dx = cr & 1;
            const float v1 = FIELD ? point_value(vol, cz + dz, cy + dy, cx + dx, a) : (float)((code >> cr) & 1u);
            const float num = a.level - v0, den = v1 - v0;
            const float t = num / den;
            const float fz = (float)(cz - 1) + t * (float)dz, fy = (float)(cy - 1) + t * (float)dy, fx = (float)(cx - 1) + t * (float)dx;
            const float sz = fz * a.sp[0], sy = fy * a.sp[1], sx = fx * a.sp[2];
            out[0] = a.org[0] + sz;
            out[1] = a.org[1] + sy;
            out[2] = a.org[2] + sx;
            out += 3;
        }
    }
}

__global__ void __launch_bounds__(EB) mesh_faces_kernel(MeshArgs a, int* __restrict__ faces) {
    __shared__ uint32_t tri[6 * 16 * 2];
    __shared__ int nbase[8][EB];                                   // vertex base of the cell at offset o, per thread
    __shared__ uint8_t nmask[8][EB];                               // and its crossing mask
    for (int i = threadIdx.x; i < 6 * 16 * 2; i += EB) tri[i] = (&TAB.tri[0][0][0])[i];
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * EB + threadIdx.x;
    const int64_t c0 = g * VPT;
    if (c0 >= (int64_t)a.nrows * a.Wcp) return;
    const uint4 cw = *reinterpret_cast<const uint4*>(a.code + c0);
    const uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
    bool any = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) any |= w[q] != 0u && w[q] != 0xFFFFFFFFu;
    if (!any) return;
    const int row = (int)(c0 / a.Wcp), x0 = (int)(c0 - (int64_t)row * a.Wcp);
    const int cz = row / a.Hc, cy = row - cz * a.Hc;
    const int fb = a.rowf[row];
    const int tid = threadIdx.x;
    for (int i = 0; i < VPT; ++i) {
        const uint32_t code = a.code[c0 + i];
        if (code == 0u || code == 255u) continue;
        const int cx = x0 + i;
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            const int nz = cz + (o >> 2), ny = cy + ((o >> 1) & 1), nx = cx + (o & 1);
            int base = 0;
            uint32_t m = 0;
            // a cell past the last one owns no crossing edge: both ends of such an edge are virtual points
            if (nz <= a.D && ny < a.Hc && nx < a.Wc) {
                const int nrow = nz * a.Hc + ny;
                const int64_t ci = (int64_t)nrow * a.Wcp + nx;
                base = a.rowv[nrow] + (int)(a.pre[ci] & 0xFFFFu);
                m = edge_mask(a.code[ci]);
            }
            nbase[o][tid] = base;
            nmask[o][tid] = (uint8_t)m;
        }
        int* out = faces + ((int64_t)fb + (a.pre[c0 + i] >> 16)) * 3;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const int c1 = AXIS_BIT[PERM[p][0]], c2 = c1 | AXIS_BIT[PERM[p][1]];
            const uint32_t cs = (code & 1u) | ((code >> c1) & 1u) << 1 | ((code >> c2) & 1u) << 2 | ((code >> 7) & 1u) << 3;
            if (cs == 0u || cs == 15u) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint32_t e = tri[(p * 16 + cs) * 2 + j];
                if (!(e >> 31)) continue;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const uint32_t r = (e >> (6 * q)) & 63u, o = r >> 3, k = r & 7u;
                    out[q] = nbase[o][tid] + __popc((uint32_t)nmask[o][tid] & ((1u << k) - 1u));
                }
                out += 3;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ 4. measure
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < MB / 64; ++i) t += lds[i];
    __syncthreads();
    return t;
}

// vertices are (z, y, x) columns; the geometry is taken in (x, y, z)
__global__ void __launch_bounds__(MB) mesh_measure_kernel(const float* __restrict__ vert, const int* __restrict__ faces, int64_t F,
                                                          double* __restrict__ part, float* __restrict__ normals) {
    __shared__ double lds[MB / 64];
    double area = 0.0, vol = 0.0;
    for (int64_t f = (int64_t)blockIdx.x * MB + threadIdx.x; f < F; f += (int64_t)gridDim.x * MB) {
        double p[3][3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float* v = vert + (int64_t)faces[f * 3 + q] * 3;
            p[q][0] = (double)v[2];
            p[q][1] = (double)v[1];
            p[q][2] = (double)v[0];
        }
        const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
        const double vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
        const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
        const double len = sqrt(nx * nx + ny * ny + nz * nz);
        area += 0.5 * len;
        const double cx = p[1][1] * p[2][2] - p[1][2] * p[2][1], cy = p[1][2] * p[2][0] - p[1][0] * p[2][2],
                     cz = p[1][0] * p[2][1] - p[1][1] * p[2][0];
        vol += (p[0][0] * cx + p[0][1] * cy + p[0][2] * cz) / 6.0;
        if (normals) {
            const double inv = len > 0.0 ? 1.0 / len : 0.0;
            normals[f * 3 + 0] = (float)(nz * inv);
            normals[f * 3 + 1] = (float)(ny * inv);
            normals[f * 3 + 2] = (float)(nx * inv);
        }
    }
    area = block_sum(area, lds);
    vol = block_sum(vol, lds);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = area;
        part[2 * blockIdx.x + 1] = vol;
    }
}

__global__ void __launch_bounds__(MB) mesh_measure_final_kernel(const double* __restrict__ part, int nb, double* __restrict__ out) {
    __shared__ double lds[MB / 64];
    double area = 0.0, vol = 0.0;
    for (int b = threadIdx.x; b < nb; b += MB) {
        area += part[2 * b];
        vol += part[2 * b + 1];
    }
    area = block_sum(area, lds);
    vol = block_sum(vol, lds);
    if (threadIdx.x == 0) {
        out[0] = area;
        out[1] = vol;
    }
}

MeshArgs make_args(int D, int H, int W, void* ws) {
    const Layout l = layout(D, H, W);
    MeshArgs a{};
    a.D = D; a.H = H; a.W = W;
    a.Hc = H + 1; a.Wc = W + 1; a.Wcp = (W + 1 + VPT - 1) / VPT * VPT;
    a.nrows = (D + 1) * (H + 1);
    unsigned char* b = (unsigned char*)ws;
    a.totals = (long long*)b;
    a.rowv = (int*)(b + l.rowv);
    a.rowf = (int*)(b + l.rowf);
    a.rowtot = (uint32_t*)(b + l.rowtot);
    a.code = b + l.code;
    a.pre = (uint32_t*)(b + l.pre);
    return a;
}

template <class T>
int launch_count(const MeshArgs& a, const void* vol, hipStream_t st) {
    const int grid = ceil_div(a.nrows, CB / 64);
    mesh_count_kernel<T><<<grid, CB, 0, st>>>(a, (const T*)vol);
    CTU_CHECK_LAUNCH("mesh count");
    return CTU_OK;
}

}  // namespace

extern "C" size_t ctu_mesh_ws_bytes(int D, int H, int W) { return shape_ok(D, H, W) ? layout(D, H, W).total : 0; }

extern "C" int ctu_mesh_count(const void* volume, int dtype, int D, int H, int W, int has_label, int64_t label, float level,
                              void* ws, void* stream) {
    CTU_REQUIRE(volume && ws, "mesh_count: null pointer");
    CTU_REQUIRE(shape_ok(D, H, W), "mesh_count: bad shape %dx%dx%d (every side in 1..%d, (D+1)(H+1)(W+1) < 2^31)", D, H, W, MAX_SIDE);
    CTU_REQUIRE((uintptr_t)ws % 16 == 0, "mesh_count: the workspace must be 16-byte aligned");
    CTU_REQUIRE(dtype == CTU_U8 || dtype == CTU_I64 || dtype == CTU_F32,
                "mesh_count: unsupported dtype %d (uint8, int64 or float32)", dtype);
    CTU_REQUIRE(dtype != CTU_F32 || !has_label, "mesh_count: a label belongs to uint8 / int64 volumes");
    CTU_REQUIRE(dtype != CTU_F32 || level == level, "mesh_count: level is NaN");
    hipStream_t st = (hipStream_t)stream;
    MeshArgs a = make_args(D, H, W, ws);
    a.has_label = has_label != 0;
    a.label = label;
    a.level = level;
    int rc;
    if (dtype == CTU_U8) rc = launch_count<uint8_t>(a, volume, st);
    else if (dtype == CTU_I64) rc = launch_count<long long>(a, volume, st);
    else rc = launch_count<float>(a, volume, st);
    if (rc != CTU_OK) return rc;
    mesh_scan_kernel<<<1, SB, 0, st>>>(a);
    CTU_CHECK_LAUNCH("mesh scan");
    return CTU_OK;
}

extern "C" int ctu_mesh_emit(const void* volume, int dtype, int D, int H, int W, float level, float fill_value,
                             const float* spacing, const float* origin, int64_t V, int64_t F, float* vertices, int32_t* faces,
                             void* ws, void* stream) {
    CTU_REQUIRE(ws, "mesh_emit: null workspace");
    CTU_REQUIRE(shape_ok(D, H, W), "mesh_emit: bad shape %dx%dx%d (every side in 1..%d, (D+1)(H+1)(W+1) < 2^31)", D, H, W, MAX_SIDE);
    CTU_REQUIRE(dtype == CTU_U8 || dtype == CTU_I64 || dtype == CTU_F32,
                "mesh_emit: unsupported dtype %d (uint8, int64 or float32)", dtype);
    CTU_REQUIRE(V >= 0 && F >= 0 && V < ((int64_t)1 << 31) && F < ((int64_t)1 << 31),
                "mesh_emit: the mesh has %lld vertices and %lld faces; both must stay below 2^31", (long long)V, (long long)F);
    CTU_REQUIRE((V == 0) == (F == 0), "mesh_emit: V = %lld and F = %lld are not the totals of one count", (long long)V, (long long)F);
    if (V == 0) return CTU_OK;
    CTU_REQUIRE(vertices && faces, "mesh_emit: null output");
    const bool field = dtype == CTU_F32;
    if (field) {
        CTU_REQUIRE(volume, "mesh_emit: null volume");
        CTU_REQUIRE(level == level && fill_value <= level, "mesh_emit: fill_value %g must not exceed level %g", (double)fill_value,
                    (double)level);
    }
    MeshArgs a = make_args(D, H, W, ws);
    a.level = field ? level : 0.5f;
    a.fill = field ? fill_value : 0.f;
    for (int i = 0; i < 3; ++i) {
        a.sp[i] = spacing ? spacing[i] : 1.f;
        a.org[i] = origin ? origin[i] : 0.f;
        CTU_REQUIRE(a.sp[i] > 0.f && a.sp[i] < __builtin_inff() && a.org[i] - a.org[i] == 0.f,
                    "mesh_emit: spacing must be positive and finite, origin finite");
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t nthreads = (int64_t)a.nrows * a.Wcp / VPT;
    const unsigned grid = (unsigned)ceil_div64(nthreads, EB);
    if (field) mesh_vertices_kernel<true><<<grid, EB, 0, st>>>(a, (const float*)volume, vertices);
    else mesh_vertices_kernel<false><<<grid, EB, 0, st>>>(a, nullptr, vertices);
    CTU_CHECK_LAUNCH("mesh vertices");
    mesh_faces_kernel<<<grid, EB, 0, st>>>(a, faces);
    CTU_CHECK_LAUNCH("mesh faces");
    return CTU_OK;
}

extern "C" int ctu_mesh_measure(const float* vertices, int64_t V, const int32_t* faces, int64_t F, double* out, float* normals,
                                void* ws, void* stream) {
    CTU_REQUIRE(out && ws, "mesh_measure: null pointer");
    CTU_REQUIRE(V >= 0 && F >= 0 && V < ((int64_t)1 << 31) && F < ((int64_t)1 << 31),
                "mesh_measure: V = %lld and F = %lld must lie in [0, 2^31)", (long long)V, (long long)F);
    CTU_REQUIRE(F == 0 || (vertices && faces && V > 0), "mesh_measure: faces without vertices");
    hipStream_t st = (hipStream_t)stream;
    int64_t nb = ceil_div64(F, MB);
    nb = nb < 1 ? 1 : (nb > MAX_MB ? MAX_MB : nb);
    mesh_measure_kernel<<<(unsigned)nb, MB, 0, st>>>(vertices, faces, F, (double*)ws, normals);
    CTU_CHECK_LAUNCH("mesh measure");
    mesh_measure_final_kernel<<<1, MB, 0, st>>>((const double*)ws, (int)nb, out);
    CTU_CHECK_LAUNCH("mesh measure final");
    return CTU_OK;
}
