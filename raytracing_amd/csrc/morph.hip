// morph.hip -- the scene's triangles morphed ON THE DEVICE from one weight per morph target, alone or fused with the skin (rt_scene_set_morph / rt_scene_morph /
// rt_scene_morph_skin).
//
// A face, a muscle corrective or a cloth cache is 4 bytes per target and frame, not 160 bytes per triangle: the scene keeps its rest pose and the targets'
// deltas on the device, transposed into one row of 32-byte records per triangle; a kernel writes the morphed triangles into a staging area in rt_triangle
// layout, and the refit (refit.hip) runs on that as on any other triangle array.
//
//   k_morph_triangles        one thread per triangle, 256 per block: rest + row + records + weights -> staged (morph.h's arithmetic)
//   k_morph_skin_triangles   the same morph, then skin.h's blend per corner from the skin's influences and palette -> staged, in one pass
//
// The rest pose and the staging area are a moved::Stage (moved.hip makes the rest pose, once per rt_scene_set_morph).  Both kernels move the block's 256
// triangles (40 KB, contiguous) through LDS in 16-byte pieces as moved_tile.h describes, and a thread morphs its own triangle in place there: a record names
// its corner at run time, which is an LDS address, not an index into registers (no scratch).
// A thread streams its own records row[i] .. row[i + 1], each a 16-byte aligned 32-byte piece (the compiler emits a 16-byte and a 12-byte load: `pad` is
// never used); a block's records are contiguous, so its lines are shared through L1.
//   k_morph_triangles stages up to LDS_TARGETS weights (4 KB) in LDS once per block; more are gathered from global memory.  40 960 + 4 096 bytes: three
//     blocks per CU.  Both branches call the same morph.h function on the same values, so they agree bit for bit.
//   k_morph_skin_triangles spends its LDS on the tile and on a palette of up to skin::LDS_BONES matrices (6 KB) only: 47 104 bytes, three blocks per CU where
//     k_skin_triangles' 64 KB leave two.  The influences do not go through LDS: a thread reads its own 72 bytes as nine 8-byte loads (a block's 18 KB are
//     contiguous, every line is used whole through L1), and the weights are gathered through L1 beside the records that name them.
// -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <new>
#include <vector>
#include "morph.h"
#include "morph_host.h"
#include "skin_host.h"
#include "moved_tile.h"
#include "device_memory.h"

namespace morph
{
static_assert(sizeof(rt_morph_delta) == 32 && sizeof(Record) == RECORD_BYTES, "32-byte deltas and records");
static_assert(256 * 160 + LDS_TARGETS * WEIGHT_BYTES <= 163840 / 3, "k_morph_triangles' LDS: three blocks per CU");
static_assert(256 * 160 + skin::LDS_BONES * skin::MATRIX_BYTES <= 163840 / 3, "k_morph_skin_triangles' LDS: three blocks per CU");

// triangle i's row, never past row[nt] (i < nt) and never past the records
__device__ inline void row_of(const uint32_t* __restrict__ row, uint32_t i, uint32_t n_records, uint32_t& begin, uint32_t& count)
{
    const uint32_t r1 = row[i + 1u] < n_records ? row[i + 1u] : n_records;
    begin = row[i] < r1 ? row[i] : r1;
    count = r1 - begin;
}

__global__ __launch_bounds__(256) void k_morph_triangles(const float4* __restrict__ rest, const uint32_t* __restrict__ row, const Record* __restrict__ records,
    const float* __restrict__ weights, uint32_t nt, uint32_t n_targets, uint32_t n_records, float4* __restrict__ out)
{
    __shared__ float4 tile[256 * 10];
    __shared__ float staged_weights[LDS_TARGETS];
    const moved::Tile b = moved::block_tile(nt);
    moved::load_tile(b, rest, tile);
    const bool staged = n_targets <= (uint32_t)LDS_TARGETS;        // the same for every block of a launch
    if (staged)
        for (uint32_t k = threadIdx.x; k < n_targets; k += 256u) staged_weights[k] = weights[k];
    __syncthreads();
    if (threadIdx.x < b.n)
    {
        uint32_t begin, count;
        row_of(row, b.first + threadIdx.x, n_records, begin, count);
        rt_triangle& t = *reinterpret_cast<rt_triangle*>(&tile[threadIdx.x * 10u]);
        if (staged) morph_triangle(records + begin, count, staged_weights, n_targets, t);
        else morph_triangle(records + begin, count, weights, n_targets, t);
    }
    __syncthreads();
    moved::store_tile(b, tile, out);
}

__global__ __launch_bounds__(256) void k_morph_skin_triangles(const float4* __restrict__ rest, const uint32_t* __restrict__ row, const Record* __restrict__ records,
    const float* __restrict__ weights, uint32_t nt, uint32_t n_targets, uint32_t n_records, const uint2* __restrict__ influences, const float* __restrict__ palette,
    uint32_t n_bones, float4* __restrict__ out)
{
    __shared__ float4 tile[256 * 10];
    __shared__ float4 bones[skin::LDS_BONES * 3];
    const moved::Tile b = moved::block_tile(nt);
    moved::load_tile(b, rest, tile);
    const bool staged = n_bones <= (uint32_t)skin::LDS_BONES;      // the same for every block of a launch
    if (staged)
        for (uint32_t k = threadIdx.x; k < n_bones * 3u; k += 256u) bones[k] = reinterpret_cast<const float4*>(palette)[k];
    __syncthreads();
    if (threadIdx.x < b.n)
    {
        const uint32_t i = b.first + threadIdx.x;
        uint2 q[9];                                                // this triangle's influences: 72 bytes from an 8-byte aligned address (i * 72)
        for (uint32_t j = 0; j < 9u; ++j) q[j] = influences[(size_t)i * 9 + j];
        uint32_t begin, count;
        row_of(row, i, n_records, begin, count);
        rt_triangle& t = *reinterpret_cast<rt_triangle*>(&tile[threadIdx.x * 10u]);
        morph_triangle(records + begin, count, weights, n_targets, t);
        if (staged) skin::skin_triangle(reinterpret_cast<const float*>(bones), n_bones, q, t);
        else skin::skin_triangle(palette, n_bones, q, t);
    }
    __syncthreads();
    moved::store_tile(b, tile, out);
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------------------
Fault table_fault(const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t n_targets, uint32_t nt)
{
    if (target_offsets[0] != 0u) return FIRST_OFFSET;
    for (uint32_t t = 0; t < n_targets; ++t) if (target_offsets[t + 1] < target_offsets[t]) return DECREASING_OFFSET;
    const uint64_t corners = (uint64_t)nt * 3;
    std::vector<uint32_t> last;                                     // target + 1 of the corner's latest delta
    try { last.assign(corners, 0u); } catch (const std::bad_alloc&) { return NO_MEMORY; }
    for (uint32_t t = 0; t < n_targets; ++t)
        for (uint32_t k = target_offsets[t]; k < target_offsets[t + 1]; ++k)
        {
            const rt_morph_delta& d = deltas[k];
            if (d.corner >= corners) return BAD_CORNER;
            for (int j = 0; j < 3; ++j) if (!std::isfinite(d.position[j]) || !std::isfinite(d.normal[j])) return NOT_FINITE;
            if (d.pad != 0u) return BAD_PAD;
            if (last[d.corner] == t + 1u) return TWICE;
            last[d.corner] = t + 1u;
        }
    return TABLE_OK;
}

bool weights_finite(const float* weights, uint32_t n_targets)
{
    for (uint32_t k = 0; k < n_targets; ++k) if (!std::isfinite(weights[k])) return false;
    return true;
}

// a counting sort over the targets in order puts a row in ascending target order; inside one (triangle, target) the at most three corners are sorted after
bool transpose(const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t n_targets, uint32_t nt, std::vector<uint32_t>& row, std::vector<Record>& records)
{
    const uint32_t n = target_offsets[n_targets];
    std::vector<uint32_t> next;
    try { row.assign((size_t)nt + 1, 0u); records.resize(n); next.resize(nt); } catch (const std::bad_alloc&) { return false; }
    for (uint32_t k = 0; k < n; ++k) ++row[deltas[k].corner / 3u + 1u];
    for (uint32_t i = 0; i < nt; ++i) row[i + 1] += row[i];
    std::copy(row.begin(), row.end() - 1, next.begin());
    for (uint32_t t = 0; t < n_targets; ++t)
        for (uint32_t k = target_offsets[t]; k < target_offsets[t + 1]; ++k)
        {
            const rt_morph_delta& d = deltas[k];
            Record& r = records[next[d.corner / 3u]++];
            r.key = t << 2 | d.corner % 3u;
            for (int j = 0; j < 3; ++j) { r.dp[j] = d.position[j]; r.dn[j] = d.normal[j]; }
            r.pad = 0u;
        }
    for (uint32_t i = 0; i < nt; ++i)
        for (uint32_t a = row[i] + 1u; a < row[i + 1]; ++a)          // an insertion sort that only ever moves a record past its own target's
            for (uint32_t b = a; b > row[i] && records[b - 1].key > records[b].key; --b) std::swap(records[b - 1], records[b]);
    return true;
}

void release(State& st)
{
    st.stage.release(); dev::drop(st.row); dev::drop(st.records); dev::drop(st.weights);
    if (st.host_weights) (void)hipHostFree(st.host_weights);
    st = State();
}

bool arm(hipStream_t stream, State& st, const float4* tris_sh, const std::vector<uint32_t>& row, const std::vector<Record>& records, uint32_t nt, uint32_t n_targets)
{
    release(st);
    st.n_targets = n_targets; st.n_deltas = (uint32_t)records.size();
    const size_t row_bytes = ((size_t)nt + 1) * ROW_BYTES, record_bytes = records.size() * RECORD_BYTES;   // (no records: dev::alloc never asks for 0 bytes)
    st.bytes = (size_t)nt * (REST_BYTES + STAGED_BYTES) + row_bytes + record_bytes + (size_t)n_targets * WEIGHT_BYTES;
    bool ok = st.stage.arm(stream, tris_sh, nt) && dev::get(st.row, row_bytes) &&
              dev::get(st.records, record_bytes) && dev::get(st.weights, (size_t)n_targets * WEIGHT_BYTES) &&
              hipHostMalloc((void**)&st.host_weights, (size_t)n_targets * WEIGHT_BYTES) == hipSuccess &&
              hipMemcpyAsync(st.row, row.data(), row_bytes, hipMemcpyHostToDevice, stream) == hipSuccess &&
              (record_bytes == 0 || hipMemcpyAsync(st.records, records.data(), record_bytes, hipMemcpyHostToDevice, stream) == hipSuccess);
    ok = hipStreamSynchronize(stream) == hipSuccess && ok;          // row and records are the caller's vectors: read before they go
    if (!ok) { (void)hipGetLastError(); release(st); }
    return ok;
}

static bool upload_weights(hipStream_t stream, State& st, const float* weights)
{
    memcpy(st.host_weights, weights, (size_t)st.n_targets * WEIGHT_BYTES);
    return hipMemcpyAsync(st.weights, st.host_weights, (size_t)st.n_targets * WEIGHT_BYTES, hipMemcpyHostToDevice, stream) == hipSuccess;
}

bool run(hipStream_t stream, State& st, const float* weights)
{
    if (!upload_weights(stream, st, weights)) return false;
    hipLaunchKernelGGL(k_morph_triangles, dim3(dev::blocks_for(st.stage.n_tris, 256u)), dim3(256), 0, stream, (const float4*)st.stage.rest, (const uint32_t*)st.row,
        (const Record*)st.records, (const float*)st.weights, st.stage.n_tris, st.n_targets, st.n_deltas, (float4*)st.stage.staged);
    return dev::clean();
}

bool run_skin(hipStream_t stream, State& st, const float* weights, const rt_skin_influence* d_influences, const float* d_palette, uint32_t n_bones)
{
    if (!upload_weights(stream, st, weights)) return false;
    hipLaunchKernelGGL(k_morph_skin_triangles, dim3(dev::blocks_for(st.stage.n_tris, 256u)), dim3(256), 0, stream, (const float4*)st.stage.rest, (const uint32_t*)st.row,
        (const Record*)st.records, (const float*)st.weights, st.stage.n_tris, st.n_targets, st.n_deltas, (const uint2*)d_influences, d_palette, n_bones,
        (float4*)st.stage.staged);
    return dev::clean();
}

bool debug_host(const rt_triangle* rest, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t n_targets, uint32_t nt, const float* weights, rt_triangle* out)
{
    std::vector<uint32_t> row;
    std::vector<Record> records;
    if (!transpose(deltas, target_offsets, n_targets, nt, row, records)) return false;
    for (uint32_t i = 0; i < nt; ++i)
    {
        rt_triangle t = rest[i];
        morph_triangle(records.data() + row[i], row[i + 1] - row[i], weights, n_targets, t);
        out[i] = t;
    }
    return true;
}

// the uploaded copies both device forms share; false: an allocation or a copy failed
struct DebugCopies
{
    void *rest = nullptr, *row = nullptr, *records = nullptr, *weights = nullptr, *out = nullptr;
    uint32_t n_records = 0;
    bool fill(dev::Temps& tmp, const rt_triangle* h_rest, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t n_targets, uint32_t nt, const float* h_weights)
    {
        if (!transpose(deltas, target_offsets, n_targets, nt, h_row, h_records)) return false;
        n_records = (uint32_t)h_records.size();
        rest = tmp.get(h_rest, (size_t)nt * sizeof(rt_triangle));
        row = tmp.get(h_row.data(), h_row.size() * ROW_BYTES);
        records = tmp.get(h_records.data(), h_records.size() * RECORD_BYTES);
        weights = tmp.get(h_weights, (size_t)n_targets * WEIGHT_BYTES);
        out = tmp.get(nullptr, (size_t)nt * sizeof(rt_triangle));
        return rest && row && records && weights && out;
    }
    std::vector<uint32_t> h_row;                                    // live until the Temps' finish() has waited for the stream
    std::vector<Record> h_records;
};

bool debug_device(hipStream_t stream, const rt_triangle* rest, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t n_targets, uint32_t nt,
    const float* weights, rt_triangle* out)
{
    DebugCopies c;                                                  // before tmp: tmp's destructor waits for the stream while c's vectors still stand
    dev::Temps tmp(stream);
    const bool ok = c.fill(tmp, rest, deltas, target_offsets, n_targets, nt, weights);
    if (ok)
        hipLaunchKernelGGL(k_morph_triangles, dim3(dev::blocks_for(nt, 256u)), dim3(256), 0, stream, (const float4*)c.rest, (const uint32_t*)c.row, (const Record*)c.records,
            (const float*)c.weights, nt, n_targets, c.n_records, (float4*)c.out);
    return tmp.finish(ok && dev::clean(), out, c.out, (size_t)nt * sizeof(rt_triangle));
}

bool debug_skin_device(hipStream_t stream, const rt_triangle* rest, const rt_morph_delta* deltas, const uint32_t* target_offsets, uint32_t n_targets, uint32_t nt,
    const float* weights, const rt_skin_influence* per_corner, const float* matrices3x4, uint32_t n_bones, rt_triangle* out)
{
    DebugCopies c;
    dev::Temps tmp(stream);
    bool ok = c.fill(tmp, rest, deltas, target_offsets, n_targets, nt, weights);
    void* const d_infl = tmp.get(per_corner, (size_t)nt * skin::INFLUENCE_BYTES);
    void* const d_palette = tmp.get(matrices3x4, (size_t)n_bones * skin::MATRIX_BYTES);
    ok = ok && d_infl && d_palette;
    if (ok)
        hipLaunchKernelGGL(k_morph_skin_triangles, dim3(dev::blocks_for(nt, 256u)), dim3(256), 0, stream, (const float4*)c.rest, (const uint32_t*)c.row, (const Record*)c.records,
            (const float*)c.weights, nt, n_targets, c.n_records, (const uint2*)d_infl, (const float*)d_palette, n_bones, (float4*)c.out);
    return tmp.finish(ok && dev::clean(), out, c.out, (size_t)nt * sizeof(rt_triangle));
}
} // namespace morph
