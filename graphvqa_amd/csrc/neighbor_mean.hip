// Mean over in-neighbours of node rows, forward and backward (torch_scatter's scatter_mean(m[row], col, dim_size = N) with m a per-NODE
// tensor: the cell of the reference's RecurrentExecutionEngine, pipeline_model_gat.py:250-259, once its first MLP is applied per node).
//   forward : out[i, :F] = (sum over the CSR slots s of row i of g, in slot order, of x[csr_src[s], :F]) / max(deg_i, 1)
//   backward: dx[j, :F]  =  sum over the CSR slots s of row j of gt (the transposed handle), in slot order, of
//                           dout[d, :F] / max(deg_g(d), 1),  d = gt->csr_src[s],  deg_g(d) = g->rowptr[d + 1] - g->rowptr[d]
// Both are one gather-reduce over node rows: no [E, F] tensor, no float atomics, no workspace; the order of every sum is the slot order,
// so two runs give the same bits.  A node without in-edges (out-edges in the backward) gets a zero row.
//
// One kernel form.  Lanes run over columns: a row is owned by `tpr` consecutive threads of a 256-thread workgroup, thread c of them takes the
// units c, c + tpr, ... of the row (a unit = V channels: V = 4, 16-byte accesses, when F, the row strides and the base pointers allow; V = 1
// otherwise), and a workgroup takes 256 / tpr consecutive destination rows (F = 512: 2 rows, one kilobyte per wave-load; F = 300: 3 rows;
// F = 12: 85 rows).  tpr = min(units per row, 256), so at most tpr - 1 threads of a workgroup idle.  The slot loop is unrolled four times --
// four independent row loads in flight per thread, added in slot order -- which is what keeps a hub row (in-degree in the thousands) at a
// few hundred dependent round trips instead of thousands; such a row costs its own workgroup that long and nobody else.
#include "common.h"

namespace gvqa {
namespace {

template <int V> struct NmVec { float v[V]; };
template <int V> __device__ __forceinline__ NmVec<V> nm_load(const float* __restrict__ p) {
    NmVec<V> o;
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        o.v[0] = t.x; o.v[1] = t.y; o.v[2] = t.z; o.v[3] = t.w;
    } else {
        o.v[0] = *p;
    }
    return o;
}
template <int V> __device__ __forceinline__ void nm_store(float* __restrict__ p, const NmVec<V>& o) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(o.v[0], o.v[1], o.v[2], o.v[3]);
    else *p = o.v[0];
}

// weight of the row of slot source j: the backward divides every gathered row by its own in-degree in g
template <bool BWD> __device__ __forceinline__ float nm_weight(const int32_t* __restrict__ deg_rowptr, int j) {
    if constexpr (BWD) return 1.f / (float)max(deg_rowptr[j + 1] - deg_rowptr[j], 1);
    else return 1.f;
}

// rowptr / src: the CSR that is walked (g forward, gt backward); deg_rowptr: g->rowptr (backward only); Cq = F / V units per row
template <int V, bool BWD>
__global__ __launch_bounds__(256) void k_neighbor_mean(int64_t N, int Cq, int tpr, int rows_per_wg, const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ src, const int32_t* __restrict__ deg_rowptr,
                                                       const float* __restrict__ x, int64_t ldx, float* __restrict__ out, int64_t ldo) {
    const int r = (int)threadIdx.x / tpr, c = (int)threadIdx.x - r * tpr;
    const int64_t i = (int64_t)blockIdx.x * rows_per_wg + r;
    if (r >= rows_per_wg || i >= N) return;
    const int s0 = rowptr[i], s1 = rowptr[i + 1];
    float* __restrict__ orow = out + i * ldo;
    for (int q = c; q < Cq; q += tpr) {
        const int64_t col = (int64_t)q * V;
        NmVec<V> a;
#pragma unroll
        for (int k = 0; k < V; ++k) a.v[k] = 0.f;
        int s = s0;
        for (; s + 4 <= s1; s += 4) {
            int j[4];
            float w[4];
            NmVec<V> v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) j[u] = src[s + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = nm_load<V>(x + (int64_t)j[u] * ldx + col);
                w[u] = nm_weight<BWD>(deg_rowptr, j[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < V; ++k) a.v[k] += BWD ? v[u].v[k] * w[u] : v[u].v[k];
        }
        for (; s < s1; ++s) {
            const int j = src[s];
            const NmVec<V> v = nm_load<V>(x + (int64_t)j * ldx + col);
            const float w = nm_weight<BWD>(deg_rowptr, j);
#pragma unroll
            for (int k = 0; k < V; ++k) a.v[k] += BWD ? v.v[k] * w : v.v[k];
        }
        if constexpr (!BWD) {
            const float den = (float)max(s1 - s0, 1);
#pragma unroll
            for (int k = 0; k < V; ++k) a.v[k] /= den;
        }
        nm_store<V>(orow + col, a);
    }
}

int nm_checks(const char* who, const gvqa_graph* g, int64_t F, const void* in, int64_t ld_in, const void* out, int64_t ld_out) {
    GVQA_REQUIRE(g && g->valid && g->finalized, GVQA_E_INVALID, "%s: graph not built / not finalized", who);
    GVQA_REQUIRE(F >= 1 && F < (1ll << 30), GVQA_E_INVALID, "%s: F must be in [1, 2^30)", who);
    GVQA_REQUIRE(ld_in >= F && ld_out >= F, GVQA_E_INVALID, "%s: row strides below their width", who);
    GVQA_REQUIRE(g->num_nodes < (1ll << 31) && g->num_edges < (1ll << 31), GVQA_E_UNSUPPORTED, "%s: more than 2^31 - 1 nodes or edges", who);
    if (g->num_nodes > 0) GVQA_REQUIRE(in && out, GVQA_E_INVALID, "%s: null tensor", who);
    return GVQA_OK;
}

template <bool BWD>
int nm_launch(const gvqa_graph* walk, const int32_t* deg_rowptr, int64_t F, const float* x, int64_t ldx, float* out, int64_t ldo,
              hipStream_t stream) {
    const int64_t N = walk->num_nodes;
    const bool v4 = F % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && aligned16(x) && aligned16(out);
    const int64_t Cq = v4 ? F / 4 : F;
    const int tpr = (int)(Cq < 256 ? Cq : 256), rows = 256 / tpr;
    const int64_t grid = cdiv(N, rows);
    GVQA_REQUIRE(grid < (1ll << 31), GVQA_E_UNSUPPORTED, "graph_neighbor_mean: more than 2^31 - 1 workgroups");
    if (v4)
        hipLaunchKernelGGL((k_neighbor_mean<4, BWD>), dim3((unsigned)grid), dim3(256), 0, stream, N, (int)Cq, tpr, rows, walk->rowptr, walk->csr_src,
                           deg_rowptr, x, ldx, out, ldo);
    else
        hipLaunchKernelGGL((k_neighbor_mean<1, BWD>), dim3((unsigned)grid), dim3(256), 0, stream, N, (int)Cq, tpr, rows, walk->rowptr, walk->csr_src,
                           deg_rowptr, x, ldx, out, ldo);
    GVQA_LAUNCH_CHECK();
    return GVQA_OK;
}

}  // namespace
}  // namespace gvqa

extern "C" int gvqa_graph_neighbor_mean_forward(const gvqa_graph* g, int64_t F, const float* x, int64_t ld_x, float* out, int64_t ld_out,
                                                void* stream) {
    using namespace gvqa;
    if (int rc = nm_checks("graph_neighbor_mean_forward", g, F, x, ld_x, out, ld_out)) return rc;
    if (g->num_nodes == 0) return GVQA_OK;
    return nm_launch<false>(g, nullptr, F, x, ld_x, out, ld_out, static_cast<hipStream_t>(stream));
}

extern "C" int gvqa_graph_neighbor_mean_backward(const gvqa_graph* g, const gvqa_graph* gt, int64_t F, const float* dout, int64_t ld_dout,
                                                 float* dx, int64_t ld_dx, void* stream) {
    using namespace gvqa;
    if (int rc = nm_checks("graph_neighbor_mean_backward", g, F, dout, ld_dout, dx, ld_dx)) return rc;
    GVQA_REQUIRE(gt && gt->valid && gt->finalized, GVQA_E_INVALID, "graph_neighbor_mean_backward: transposed graph not built / not finalized");
    GVQA_REQUIRE(gt->num_nodes == g->num_nodes && gt->num_edges == g->num_edges, GVQA_E_INVALID,
                 "graph_neighbor_mean_backward: gt is not the transposed handle of g (node / edge counts differ)");
    if (g->num_nodes == 0) return GVQA_OK;
    return nm_launch<true>(gt, g->rowptr, F, dout, ld_dout, dx, ld_dx, static_cast<hipStream_t>(stream));
}
