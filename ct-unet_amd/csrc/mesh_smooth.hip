// Vertex adjacency (CSR) and Taubin / Laplacian smoothing of surface meshes, gfx950 (rule pinned in ctunet_amd/mesh.py;
// tests/mesh_smooth_ref.py restates it in numpy).
//
// Adjacency, over the 6F directed pairs (a -> b, a != b) of the faces; a face with an index outside [0, V) is skipped by
// every kernel and counted in the workspace head:
//   1. count    a thread per face: cnt[a] += 1 per pair (integer atomics: the final value does not depend on arrival order).
//   2. scan     exclusive scan of cnt over V in vertex order -> the cursor of every vertex's segment of `seg`.  Three
//               launches: the sum of every chunk of SCAN_CHUNK = 1024 threads x 4 vertices, one block that scans the chunk
//               sums in order (a thread owns ceil(chunks / 1024) consecutive chunks beyond 1024 chunks; int64), and the
//               chunks again with their bases (chunked_exclusive_scan of scan.h).
//   3. fill     a thread per face: seg[cursor[a]++] = b.  The order within a segment depends on arrival; step 4 removes it.
//               Afterwards cursor[a] is the segment's end, so the segment is [cursor[a] - cnt[a], cursor[a]).
//   4. sort     a thread per vertex: insertion of the segment's entries into its own sorted duplicate-free prefix, in
//               place (the prefix never overtakes the read position); cnt[a] = |N(a)|.  Valences of marching-tetrahedra
//               meshes are 4..10 (segments of 8..20 entries); any valence gives the right answer, in quadratic time.
//   5. scan     the same scan of the unique counts -> offsets [V+1], and E at the workspace head for the host.
//   6. emit     a thread per vertex copies its prefix to neighbours[offsets[i] ..], bounded by E.
// Smoothing: positions are staged as 16 bytes per vertex (x, y, z, pad) in two ping-pong buffers, so a neighbour is one
// 16-byte load; one launch per step, a thread per vertex, Jacobi; the last step writes the packed [V,3] result.  Every
// offset is compared against E and every neighbour against V before it is used.  Contraction is off: the sum in ascending
// neighbour order, the division, the subtraction, the product and the sum each round on their own, as numpy's do.
// Measured: profiles/mesh_smooth.md.
//
// No reference counterpart: the reference writes NIfTI volumes only.
#include "common.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace {

constexpr int FB = 256;                         // block of the per-face and per-vertex kernels
constexpr int SCAN_CHUNK = CSCAN_CHUNK;         // scan.h: 1024 threads x 4 vertices
static_assert(SCAN_CHUNK == CTU_MESH_ADJ_SCAN_CHUNK, "the header states the scan's single-block capacity");
constexpr int64_t LIMIT = (int64_t)1 << 31;

struct Head { long long E, bad, upper; };      // at the start of the workspace (256 bytes reserved)

struct Layout { size_t cnt, cursor, bsum, seg, total; };
Layout layout(int64_t V, int64_t F) {
    Layout l;
    size_t o = 256;
    l.cnt = o;    o += align256((size_t)V * 4);               // directly behind the head: one memset clears both
    l.cursor = o; o += align256((size_t)V * 4);
    l.bsum = o;   o += align256((size_t)ceil_div64(V, SCAN_CHUNK) * 8);
    l.seg = o;    o += align256((size_t)F * 24);
    l.total = o;
    return l;
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 0 && F >= 0 && V < LIMIT && F < LIMIT && 6 * F < LIMIT; }

// ------------------------------------------------------------------------------------------------ count / fill
template <bool FILL>
__global__ void __launch_bounds__(FB) adj_pairs_kernel(const int* __restrict__ faces, int64_t F, int V, int* __restrict__ cnt,
                                                       int* __restrict__ cursor, int* __restrict__ seg, Head* head) {
    const int64_t t = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (t >= F) return;
    const int v[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
    if ((unsigned)v[0] >= (unsigned)V || (unsigned)v[1] >= (unsigned)V || (unsigned)v[2] >= (unsigned)V) {
        if (!FILL) atomicAdd((unsigned long long*)&head->bad, 1ull);
        return;
    }
    const int64_t cap = 6 * F;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int a = v[q], b = v[q == 2 ? 0 : q + 1];
        if (a == b) continue;
        if (FILL) {
            const int pa = atomicAdd(cursor + a, 1), pb = atomicAdd(cursor + b, 1);
            if ((unsigned)pa < cap) seg[pa] = b;
            if ((unsigned)pb < cap) seg[pb] = a;
        } else {
            atomicAdd(cnt + a, 1);
            atomicAdd(cnt + b, 1);
        }
    }
}

// ------------------------------------------------------------------------------------------------ sort / emit
__global__ void __launch_bounds__(FB) adj_sort_kernel(int V, int64_t cap, int* __restrict__ cnt, const int* __restrict__ cursor,
                                                      int* __restrict__ seg) {
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i >= V) return;
    const int n = cnt[i];
    const int64_t s0 = (int64_t)cursor[i] - n;
    if (n <= 0 || s0 < 0 || s0 + n > cap) {                        // cannot happen after count / scan / fill of one call
        cnt[i] = 0;
        return;
    }
    int* s = seg + s0;
    int m = 0;                                                     // s[0 .. m) is sorted and duplicate-free, m <= k
    for (int k = 0; k < n; ++k) {
        const int x = s[k];
        int j = m;
        while (j > 0 && s[j - 1] > x) --j;
        if (j > 0 && s[j - 1] == x) continue;
        for (int t = m; t > j; --t) s[t] = s[t - 1];
        s[j] = x;
        ++m;
    }
    cnt[i] = m;
}

__global__ void __launch_bounds__(FB) adj_emit_kernel(int V, int64_t cap, int64_t E, const int* __restrict__ cnt,
                                                      const int* __restrict__ cursor, const int* __restrict__ seg,
                                                      const int* __restrict__ offsets, int* __restrict__ neighbours) {
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i >= V) return;
    const int m = cnt[i];
    const int64_t o = offsets[i];
    // the segment began at cursor - (its upper-bound count), which the sort overwrote; the next vertex's begins where this
    // one ended, so the begin is the previous cursor
    const int64_t s0 = i ? cursor[i - 1] : 0;
    if (m <= 0 || o < 0 || o + m > E || s0 < 0 || s0 + m > cap) return;
    for (int k = 0; k < m; ++k) neighbours[o + k] = seg[s0 + k];
}

// ------------------------------------------------------------------------------------------------ smoothing
__global__ void __launch_bounds__(FB) smooth_pack_kernel(const float* __restrict__ vert, int V, float4* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i >= V) return;
    dst[i] = make_float4(vert[3 * i], vert[3 * i + 1], vert[3 * i + 2], 0.f);
}

// one step with factor s; LAST: the packed [V,3] result instead of the staged one
template <bool LAST>
__global__ void __launch_bounds__(FB) smooth_step_kernel(const float4* __restrict__ src, int V, const int* __restrict__ offsets,
                                                         const int* __restrict__ neighbours, int64_t E,
                                                         const uint8_t* __restrict__ fixed, float s, float4* __restrict__ dst,
                                                         float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i >= V) return;
    float4 p = src[i];
    const int o0 = offsets[i], o1 = offsets[i + 1];
    if (o0 >= 0 && o1 > o0 && o1 <= E && !(fixed && fixed[i])) {
        // a neighbour outside [0, V) (a corrupted table) stands in as the vertex itself or is left out: wrong, never a fault
        int j = neighbours[o0];
        float4 a = (unsigned)j < (unsigned)V ? src[j] : p;
        for (int k = o0 + 1; k < o1; ++k) {
            j = neighbours[k];
            if ((unsigned)j >= (unsigned)V) continue;
            const float4 q = src[j];
            a.x = a.x + q.x;
            a.y = a.y + q.y;
            a.z = a.z + q.z;
        }
        const float d = (float)(o1 - o0);
        const float mx = a.x / d, my = a.y / d, mz = a.z / d;
        const float dx = mx - p.x, dy = my - p.y, dz = mz - p.z;
        const float tx = s * dx, ty = s * dy, tz = s * dz;
        p.x = p.x + tx;
        p.y = p.y + ty;
        p.z = p.z + tz;
    }
    if (LAST) {
        out[3 * i] = p.x;
        out[3 * i + 1] = p.y;
        out[3 * i + 2] = p.z;
    } else {
        dst[i] = p;
    }
}

int scan(const int* x, int64_t n, long long* bsum, int* y, long long* total, int* end, hipStream_t st) {
    return chunked_exclusive_scan(x, n, bsum, y, total, end, st, "mesh adjacency scan");
}

}  // namespace

extern "C" size_t ctu_mesh_adjacency_ws_bytes(int64_t V, int64_t F) { return sizes_ok(V, F) ? layout(V, F).total : 0; }

extern "C" int ctu_mesh_adjacency_build(const int32_t* faces, int64_t V, int64_t F, int32_t* offsets, void* ws, void* stream) {
    CTU_REQUIRE(sizes_ok(V, F), "mesh_adjacency_build: V and 6F must lie in [0, 2^31), got V = %lld, F = %lld", (long long)V, (long long)F);
    CTU_REQUIRE(F == 0 || V > 0, "mesh_adjacency_build: faces without vertices");
    if (V == 0 || F == 0) return CTU_OK;                           // the empty table: offsets all zero, E = 0; nothing is written
    CTU_REQUIRE(faces && offsets && ws, "mesh_adjacency_build: null pointer");
    CTU_REQUIRE((uintptr_t)ws % 16 == 0, "mesh_adjacency_build: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(V, F);
    unsigned char* b = (unsigned char*)ws;
    Head* head = (Head*)b;
    int* cnt = (int*)(b + l.cnt);
    int* cursor = (int*)(b + l.cursor);
    long long* bsum = (long long*)(b + l.bsum);
    int* seg = (int*)(b + l.seg);
    CTU_REQUIRE(hipMemsetAsync(ws, 0, l.cursor, st) == hipSuccess, "mesh_adjacency_build: cannot clear the workspace");
    const unsigned fgrid = (unsigned)ceil_div64(F, FB), vgrid = (unsigned)ceil_div64(V, FB);
    adj_pairs_kernel<false><<<fgrid, FB, 0, st>>>(faces, F, (int)V, cnt, cursor, seg, head);
    CTU_CHECK_LAUNCH("mesh adjacency count");
    int rc = scan(cnt, V, bsum, cursor, &head->upper, nullptr, st);
    if (rc != CTU_OK) return rc;
    adj_pairs_kernel<true><<<fgrid, FB, 0, st>>>(faces, F, (int)V, cnt, cursor, seg, head);
    CTU_CHECK_LAUNCH("mesh adjacency fill");
    adj_sort_kernel<<<vgrid, FB, 0, st>>>((int)V, 6 * F, cnt, cursor, seg);
    CTU_CHECK_LAUNCH("mesh adjacency sort");
    return scan(cnt, V, bsum, offsets, &head->E, offsets + V, st);
}

extern "C" int ctu_mesh_adjacency_emit(int64_t V, int64_t F, int64_t E, const int32_t* offsets, int32_t* neighbours, void* ws,
                                       void* stream) {
    CTU_REQUIRE(sizes_ok(V, F), "mesh_adjacency_emit: V and 6F must lie in [0, 2^31), got V = %lld, F = %lld", (long long)V, (long long)F);
    CTU_REQUIRE(E >= 0 && E <= 6 * F, "mesh_adjacency_emit: E = %lld is not the total of a build of %lld faces", (long long)E,
                (long long)F);
    if (V == 0 || E == 0) return CTU_OK;
    CTU_REQUIRE(offsets && neighbours && ws, "mesh_adjacency_emit: null pointer");
    CTU_REQUIRE((uintptr_t)ws % 16 == 0, "mesh_adjacency_emit: the workspace must be 16-byte aligned");
    const Layout l = layout(V, F);
    unsigned char* b = (unsigned char*)ws;
    adj_emit_kernel<<<(unsigned)ceil_div64(V, FB), FB, 0, (hipStream_t)stream>>>((int)V, 6 * F, E, (const int*)(b + l.cnt),
                                                                                (const int*)(b + l.cursor), (const int*)(b + l.seg),
                                                                                offsets, neighbours);
    CTU_CHECK_LAUNCH("mesh adjacency emit");
    return CTU_OK;
}

extern "C" size_t ctu_mesh_smooth_ws_bytes(int64_t V) { return V >= 0 && V < LIMIT ? 2 * align256((size_t)V * 16) : 0; }

extern "C" int ctu_mesh_smooth(const float* vertices, int64_t V, const int32_t* offsets, const int32_t* neighbours, int64_t E,
                               const uint8_t* fixed, int iterations, float lambda, int has_mu, float mu, float* out, void* ws,
                               void* stream) {
    CTU_REQUIRE(V >= 0 && V < LIMIT && E >= 0 && E < LIMIT, "mesh_smooth: V = %lld and E = %lld must lie in [0, 2^31)", (long long)V,
                (long long)E);
    CTU_REQUIRE(iterations >= 0 && iterations <= CTU_MESH_SMOOTH_MAX_ITERATIONS, "mesh_smooth: iterations must lie in 0..%d, got %d",
                CTU_MESH_SMOOTH_MAX_ITERATIONS, iterations);
    CTU_REQUIRE(lambda > 0.f && lambda <= 1.f, "mesh_smooth: lambda must lie in (0, 1], got %g", (double)lambda);
    CTU_REQUIRE(!has_mu || (mu - mu == 0.f && mu < -lambda), "mesh_smooth: mu must be finite and below -lambda = %g, got %g",
                (double)-lambda, (double)mu);
    if (V == 0) return CTU_OK;
    CTU_REQUIRE(vertices && out && offsets && ws, "mesh_smooth: null pointer");
    CTU_REQUIRE(E == 0 || neighbours, "mesh_smooth: null neighbours");
    CTU_REQUIRE((uintptr_t)ws % 16 == 0, "mesh_smooth: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int steps = iterations * (has_mu ? 2 : 1);
    if (steps == 0) {
        CTU_REQUIRE(hipMemcpyAsync(out, vertices, (size_t)V * 12, hipMemcpyDeviceToDevice, st) == hipSuccess,
                    "mesh_smooth: cannot copy the vertices");
        return CTU_OK;
    }
    float4* buf[2] = {(float4*)ws, (float4*)((unsigned char*)ws + align256((size_t)V * 16))};
    const unsigned grid = (unsigned)ceil_div64(V, FB);
    smooth_pack_kernel<<<grid, FB, 0, st>>>(vertices, (int)V, buf[0]);
    CTU_CHECK_LAUNCH("mesh smooth pack");
    for (int t = 0; t < steps; ++t) {
        const float s = has_mu && (t & 1) ? mu : lambda;
        if (t == steps - 1)
            smooth_step_kernel<true><<<grid, FB, 0, st>>>(buf[t & 1], (int)V, offsets, neighbours, E, fixed, s, nullptr, out);
        else
            smooth_step_kernel<false><<<grid, FB, 0, st>>>(buf[t & 1], (int)V, offsets, neighbours, E, fixed, s, buf[(t + 1) & 1], nullptr);
        CTU_CHECK_LAUNCH("mesh smooth step");
    }
    return CTU_OK;
}
