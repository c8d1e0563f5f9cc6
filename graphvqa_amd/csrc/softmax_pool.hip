// Global attention pooling, forward and backward (torch_geometric.utils.softmax(gate, batch) followed by scatter_add(gate * x, batch):
// pipeline_model_gat.py:172-179 and :279-286, call site K13 of SURVEY 2.1).  Per graph b with scores s_i and rows x[i, :C]:
//   forward : m_b = max_i s_i (0 for an empty graph);  gate_i = exp(s_i - m_b) / (sum_j exp(s_j - m_b) + 1e-16);  out[b] = sum_i gate_i x[i]
//   backward: t_i = <dout[b], x[i]> (+ dgate_i);  r_b = sum_i gate_i t_i;  dscore_i = gate_i (t_i - r_b);  dx[i] = gate_i dout[b]
// The derivative is exact for the +1e-16 denominator with the max taken as a constant; the term PyG's autograd adds through the max is
// gate_i 1e-16 / (S + 1e-16) with S >= 1, below fp32 resolution.
//
// Two forms, picked per call by gsp_pick_form from the handle's statistics (max_graph_nodes x C):
//   (1) one 256-thread workgroup per graph.  Scores, max and sum once per graph; the gates of up to GSP_ROWS nodes in LDS; the four waves
//       stride over the node rows, a lane owns GSP_U units of V channels per column tile (C = 512: one tile, two 16-byte loads per row), the
//       waves' partial rows are added in wave order through LDS.  The backward holds dout[b] in registers when C fits one tile, takes t_i by a
//       wave reduction and writes dx[i] in the same pass: x is read once and dx written once.  Larger graphs loop over chunks of GSP_ROWS rows.
//   (2) split: a graph is cut into chunks of rows, one workgroup each.  Forward pass A leaves per chunk (max, sum, rows weighted with
//       exp(s - m_chunk)) in the workspace; pass B, grid (graph, chunk) again, combines them in chunk order -- every workgroup the graph's
//       (m_b, S) itself, then the gates of its own rows and its own slice of the output columns: sum_c exp(m_c - m_b) P_c / (S + 1e-16).
//       Backward pass A writes dx and leaves t_i in dscore and the chunk's sum of gate_i t_i in the workspace; pass B combines r_b and
//       finishes dscore in place.
// No float atomics; every sum has an order fixed by (thread, wave, chunk): the same bits in every run.
//
// Rows: x / dout / dx are [N, ld_*], out [B, ld_out], ld_* >= C elements; score [N] with stride ld_score >= 1; gate / dgate / dscore [N]
// dense.  16-byte accesses when C, every row stride and every row pointer allow it, scalar ones otherwise.
#include <algorithm>

#include "common.h"

namespace gvqa {
namespace {

constexpr int GSP_ROWS = 256;                  // node rows whose gates one pass of a workgroup holds in LDS
constexpr int GSP_U = 2;                       // units (V channels) a lane owns per column tile: a tile is 64 GSP_U V channels
constexpr int64_t GSP_CHUNK = 16384;           // elements per workgroup of the split form (C = 512: 32 rows, 64 KB)
constexpr int GSP_MAX_CHUNKS = 1024;           // chunks per graph at most (larger graphs get larger chunks): the combine holds their weights in LDS
constexpr int64_t GSP_MAX_GRID = 1 << 22;      // graphs x chunks of a split launch at most
constexpr int64_t GSP_MAX_PARTIAL = 1 << 24;   // floats of partial rows in the workspace at most (64 MB) -- or one row per graph, if that is more
constexpr int64_t GSP_SPLIT_MIN = 32768;       // auto rule: split form when max_graph_nodes x C > this (the last swept size at which form 1 is not slower)

template <int V> struct GspVec { float v[V]; };
template <int V> __device__ __forceinline__ GspVec<V> gsp_load(const float* __restrict__ p) {
    GspVec<V> o;
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        o.v[0] = t.x; o.v[1] = t.y; o.v[2] = t.z; o.v[3] = t.w;
    } else {
        o.v[0] = *p;
    }
    return o;
}
template <int V> __device__ __forceinline__ void gsp_store(float* __restrict__ p, const GspVec<V>& o) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(o.v[0], o.v[1], o.v[2], o.v[3]);
    else *p = o.v[0];
}

// over the 256 threads, the four waves combined in index order (red: 4 floats of LDS)
__device__ __forceinline__ float gsp_block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float gsp_block_max(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// max and sum of exp(s - max) over the rows [i0, i0 + n) (n >= 1), by the whole workgroup
__device__ __forceinline__ void gsp_max_sum(const float* __restrict__ score, int64_t lds, int64_t i0, int64_t n, float* red, float& m, float& S) {
    float v = -INFINITY;
    for (int64_t r = threadIdx.x; r < n; r += 256) v = fmaxf(v, score[(i0 + r) * lds]);
    m = gsp_block_max(v, red);
    float s = 0.f;
    for (int64_t r = threadIdx.x; r < n; r += 256) s += expf(score[(i0 + r) * lds] - m);
    S = gsp_block_sum(s, red);
}

// dst[:C] = sum over the rows [i0, i0 + n) (n >= 1) of w_i x[i, :C], w_i = exp(s_i - m) / den, by the whole workgroup; gate != NULL: gate[i] = w_i
// as well.  gl: GSP_ROWS floats, acc: 4 x 64 GSP_U V floats of LDS.  A wave adds its rows in index order, the waves are added in wave order.
template <int V>
__device__ __forceinline__ void gsp_weighted_rows(int Cq, const float* __restrict__ score, int64_t lds, const float* __restrict__ x, int64_t ldx,
                                                  int64_t i0, int64_t n, float m, float den, float* __restrict__ gate, float* __restrict__ dst,
                                                  float* gl, float* acc) {
    constexpr int TQ = 64 * GSP_U;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t0 = 0; t0 < Cq; t0 += TQ) {
        GspVec<V> a[GSP_U];
#pragma unroll
        for (int u = 0; u < GSP_U; ++u)
#pragma unroll
            for (int k = 0; k < V; ++k) a[u].v[k] = 0.f;
        for (int64_t c0 = 0; c0 < n; c0 += GSP_ROWS) {
            const int cn = (int)min<int64_t>(GSP_ROWS, n - c0);
            __syncthreads();
            if ((int)threadIdx.x < cn) {
                const float w = expf(score[(i0 + c0 + threadIdx.x) * lds] - m) / den;
                gl[threadIdx.x] = w;
                if (gate && t0 == 0) gate[i0 + c0 + threadIdx.x] = w;
            }
            __syncthreads();
#pragma unroll 2
            for (int r = wave; r < cn; r += 4) {
                const float w = gl[r];
                const float* __restrict__ xr = x + (i0 + c0 + r) * ldx;
#pragma unroll
                for (int u = 0; u < GSP_U; ++u) {
                    const int q = t0 + u * 64 + lane;
                    if (q < Cq) {
                        const GspVec<V> xv = gsp_load<V>(xr + (int64_t)q * V);
#pragma unroll
                        for (int k = 0; k < V; ++k) a[u].v[k] += w * xv.v[k];
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < GSP_U; ++u) gsp_store<V>(acc + ((wave * GSP_U + u) * 64 + lane) * V, a[u]);
        __syncthreads();
        if ((int)threadIdx.x < TQ && t0 + (int)threadIdx.x < Cq) {
            GspVec<V> o;
#pragma unroll
            for (int k = 0; k < V; ++k)
                o.v[k] = (acc[threadIdx.x * V + k] + acc[(TQ + threadIdx.x) * V + k]) + (acc[(2 * TQ + threadIdx.x) * V + k] + acc[(3 * TQ + threadIdx.x) * V + k]);
            gsp_store<V>(dst + (int64_t)(t0 + threadIdx.x) * V, o);
        }
    }
    __syncthreads();
}

// Backward over the rows [i0, i0 + n) (n >= 1) of graph row `dro` = dout[b]: dx[i] = gate_i dro (dx != NULL) and, with dscore != NULL,
// t_i = <dro, x[i]> (+ dgate_i).  Returns this thread's sum of gate_i t_i over the rows it owns (row c0 + threadIdx.x of every chunk c0).
// t_i goes to dscore[i] -- except, with keep0, the first chunk's, which stays in the register t0 (form 1: a workload graph never touches dscore twice).
template <int V>
__device__ __forceinline__ float gsp_bwd_rows(int Cq, const float* __restrict__ x, int64_t ldx, const float* __restrict__ dro,
                                              const float* __restrict__ gate, const float* __restrict__ dgate, int64_t i0, int64_t n,
                                              float* __restrict__ dscore, float* __restrict__ dx, int64_t lddx, bool keep0, float& t0, float* tl) {
    constexpr int TQ = 64 * GSP_U;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool one = Cq <= TQ;          // dout[b] in registers
    GspVec<V> dreg[GSP_U];
#pragma unroll
    for (int u = 0; u < GSP_U; ++u) {
        const int q = u * 64 + lane;
        if (one && q < Cq) dreg[u] = gsp_load<V>(dro + (int64_t)q * V);
        else
#pragma unroll
            for (int k = 0; k < V; ++k) dreg[u].v[k] = 0.f;
    }
    float racc = 0.f;
    for (int64_t c0 = 0; c0 < n; c0 += GSP_ROWS) {
        const int cn = (int)min<int64_t>(GSP_ROWS, n - c0);
        for (int r = wave; r < cn; r += 4) {
            const int64_t i = i0 + c0 + r;
            const float gi = gate[i];
            const float* __restrict__ xr = x + i * ldx;
            float* __restrict__ dxr = dx ? dx + i * lddx : nullptr;
            float dot = 0.f;
            for (int tq = 0; tq < Cq; tq += TQ) {
#pragma unroll
                for (int u = 0; u < GSP_U; ++u) {
                    const int q = tq + u * 64 + lane;
                    if (q < Cq) {
                        const GspVec<V> dv = one ? dreg[u] : gsp_load<V>(dro + (int64_t)q * V);
                        if (dscore) {
                            const GspVec<V> xv = gsp_load<V>(xr + (int64_t)q * V);
#pragma unroll
                            for (int k = 0; k < V; ++k) dot += xv.v[k] * dv.v[k];
                        }
                        if (dxr) {
                            GspVec<V> o;
#pragma unroll
                            for (int k = 0; k < V; ++k) o.v[k] = gi * dv.v[k];
                            gsp_store<V>(dxr + (int64_t)q * V, o);
                        }
                    }
                }
            }
            if (dscore) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
                if (lane == 0) tl[r] = dot;
            }
        }
        if (!dscore) continue;
        __syncthreads();
        if ((int)threadIdx.x < cn) {
            const int64_t i = i0 + c0 + threadIdx.x;
            const float ti = tl[threadIdx.x] + (dgate ? dgate[i] : 0.f);
            racc += gate[i] * ti;
            if (keep0 && c0 == 0) t0 = ti;
            else dscore[i] = ti;
        }
        __syncthreads();
    }
    return racc;
}

// ---- form 1: one workgroup per graph ----
template <int V>
__global__ __launch_bounds__(256) void k_gsp_fwd_wg(int C, const int32_t* __restrict__ graph_ptr, const float* __restrict__ score, int64_t lds,
                                                    const float* __restrict__ x, int64_t ldx, float* __restrict__ gate, float* __restrict__ out,
                                                    int64_t ldo) {
    __shared__ float red[4];
    __shared__ float gl[GSP_ROWS];
    __shared__ __attribute__((aligned(16))) float acc[4 * 64 * GSP_U * V];
    const int64_t b = blockIdx.x, n0 = graph_ptr[b], n = graph_ptr[b + 1] - n0;
    const int Cq = C / V;
    float* __restrict__ orow = out + b * ldo;
    if (n <= 0) {
        for (int c = threadIdx.x; c < C; c += 256) orow[c] = 0.f;
        return;
    }
    float m, S;
    gsp_max_sum(score, lds, n0, n, red, m, S);
    gsp_weighted_rows<V>(Cq, score, lds, x, ldx, n0, n, m, S + 1e-16f, gate, orow, gl, acc);
}

template <int V>
__global__ __launch_bounds__(256) void k_gsp_bwd_wg(int C, const int32_t* __restrict__ graph_ptr, const float* __restrict__ x, int64_t ldx,
                                                    const float* __restrict__ gate, const float* __restrict__ dout, int64_t ldd,
                                                    const float* __restrict__ dgate, float* __restrict__ dscore, float* __restrict__ dx, int64_t lddx) {
    __shared__ float red[4];
    __shared__ float tl[GSP_ROWS];
    const int64_t b = blockIdx.x, n0 = graph_ptr[b], n = graph_ptr[b + 1] - n0;
    if (n <= 0) return;
    float t0 = 0.f;
    const float racc = gsp_bwd_rows<V>(C / V, x, ldx, dout + b * ldd, gate, dgate, n0, n, dscore, dx, lddx, true, t0, tl);
    if (!dscore) return;
    const float rb = gsp_block_sum(racc, red);
    // (a thread reads back the t_i it stored itself)
    for (int64_t r = threadIdx.x; r < n; r += 256) {
        const float ti = r < GSP_ROWS ? t0 : dscore[n0 + r];
        dscore[n0 + r] = gate[n0 + r] * (ti - rb);
    }
}

// ---- form 2: split.  Grid (graph, chunk); chunk c of a graph = its rows [c R, (c + 1) R).  Workspace: MS[(b nch + c) 2 + k] = the chunk's (max, sum)
//      (the backward: k = 0 its sum of gate_i t_i), P[(b nch + c) Cp + :C] its weighted rows ----
template <int V>
__global__ __launch_bounds__(256) void k_gsp_fwd_split_a(int C, int64_t R, int nch, int64_t Cp, const int32_t* __restrict__ graph_ptr,
                                                         const float* __restrict__ score, int64_t lds, const float* __restrict__ x, int64_t ldx,
                                                         float* __restrict__ MS, float* __restrict__ P) {
    __shared__ float red[4];
    __shared__ float gl[GSP_ROWS];
    __shared__ __attribute__((aligned(16))) float acc[4 * 64 * GSP_U * V];
    const int64_t b = blockIdx.x, c = blockIdx.y, n0 = graph_ptr[b], n = graph_ptr[b + 1] - n0;
    const int64_t r0 = c * R, r1 = min(r0 + R, n);
    if (r0 >= n || c >= nch) return;
    float m, S;
    gsp_max_sum(score, lds, n0 + r0, r1 - r0, red, m, S);
    if (threadIdx.x == 0) { MS[(b * nch + c) * 2] = m; MS[(b * nch + c) * 2 + 1] = S; }
    gsp_weighted_rows<V>(C / V, score, lds, x, ldx, n0 + r0, r1 - r0, m, 1.f, nullptr, P + (b * nch + c) * Cp, gl, acc);
}

template <int V>
__global__ __launch_bounds__(256) void k_gsp_fwd_split_b(int C, int64_t R, int nch, int64_t Cp, const int32_t* __restrict__ graph_ptr,
                                                         const float* __restrict__ score, int64_t lds, const float* __restrict__ MS,
                                                         const float* __restrict__ P, float* __restrict__ gate, float* __restrict__ out, int64_t ldo) {
    __shared__ float red[4];
    __shared__ float wl[GSP_MAX_CHUNKS];
    const int64_t b = blockIdx.x, c = blockIdx.y, n0 = graph_ptr[b], n = graph_ptr[b + 1] - n0;
    float* __restrict__ orow = out + b * ldo;
    if (n <= 0) {
        if (c == 0) for (int k = threadIdx.x; k < C; k += 256) orow[k] = 0.f;
        return;
    }
    const int nc = (int)min<int64_t>((n + R - 1) / R, nch);      // (<= nch whenever the handle's max_graph_nodes holds)
    if (c >= nc) return;
    const float* __restrict__ MSb = MS + b * nch * 2;
    float v = -INFINITY;
    for (int k = threadIdx.x; k < nc; k += 256) v = fmaxf(v, MSb[2 * k]);
    const float m = gsp_block_max(v, red);
    float s = 0.f;
    for (int k = threadIdx.x; k < nc; k += 256) {
        const float w = expf(MSb[2 * k] - m);
        wl[k] = w;
        s += MSb[2 * k + 1] * w;
    }
    const float den = gsp_block_sum(s, red) + 1e-16f;            // (its barriers publish wl)
    const int64_t r0 = c * R, r1 = min(r0 + R, n);
    for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) gate[n0 + r] = expf(score[(n0 + r) * lds] - m) / den;
    // this workgroup's slice of the output columns: the chunks' rows added in chunk order
    const int Cq = C / V, per = (Cq + nc - 1) / nc;
    const int q1 = min(Cq, ((int)c + 1) * per);
    const float* __restrict__ Pb = P + b * nch * Cp;
    for (int q = (int)c * per + threadIdx.x; q < q1; q += 256) {
        GspVec<V> a;
#pragma unroll
        for (int k = 0; k < V; ++k) a.v[k] = 0.f;
        for (int j = 0; j < nc; ++j) {
            const GspVec<V> pv = gsp_load<V>(Pb + j * Cp + (int64_t)q * V);
            const float w = wl[j];
#pragma unroll
            for (int k = 0; k < V; ++k) a.v[k] += w * pv.v[k];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) a.v[k] /= den;
        gsp_store<V>(orow + (int64_t)q * V, a);
    }
}

template <int V>
__global__ __launch_bounds__(256) void k_gsp_bwd_split_a(int C, int64_t R, int nch, const int32_t* __restrict__ graph_ptr, const float* __restrict__ x,
                                                         int64_t ldx, const float* __restrict__ gate, const float* __restrict__ dout, int64_t ldd,
                                                         const float* __restrict__ dgate, float* __restrict__ dscore, float* __restrict__ dx,
                                                         int64_t lddx, float* __restrict__ MS) {
    __shared__ float red[4];
    __shared__ float tl[GSP_ROWS];
    const int64_t b = blockIdx.x, c = blockIdx.y, n0 = graph_ptr[b], n = graph_ptr[b + 1] - n0;
    const int64_t r0 = c * R, r1 = min(r0 + R, n);
    if (r0 >= n || c >= nch) return;
    float t0 = 0.f;
    const float racc = gsp_bwd_rows<V>(C / V, x, ldx, dout + b * ldd, gate, dgate, n0 + r0, r1 - r0, dscore, dx, lddx, false, t0, tl);
    if (!dscore) return;
    const float rc = gsp_block_sum(racc, red);
    if (threadIdx.x == 0) MS[(b * nch + c) * 2] = rc;
}

__global__ __launch_bounds__(256) void k_gsp_bwd_split_b(int64_t R, int nch, const int32_t* __restrict__ graph_ptr, const float* __restrict__ gate,
                                                         const float* __restrict__ MS, float* __restrict__ dscore) {
    __shared__ float red[4];
    const int64_t b = blockIdx.x, c = blockIdx.y, n0 = graph_ptr[b], n = graph_ptr[b + 1] - n0;
    if (n <= 0) return;
    const int nc = (int)min<int64_t>((n + R - 1) / R, nch);
    if (c >= nc) return;
    float s = 0.f;
    for (int k = threadIdx.x; k < nc; k += 256) s += MS[(b * nch + k) * 2];
    const float rb = gsp_block_sum(s, red);
    const int64_t r0 = c * R, r1 = min(r0 + R, n);
    for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) dscore[n0 + r] = gate[n0 + r] * (dscore[n0 + r] - rb);
}

// The auto rule, in one place: the split form when the largest graph has more than GSP_SPLIT_MIN elements (a forced form is taken as given)
int gsp_pick_form(const gvqa_graph* g, int64_t C, int form) {
    if (form == 1 || form == 2) return form;
    return (int64_t)g->max_graph_nodes * C > GSP_SPLIT_MIN ? 2 : 1;
}
// rows per chunk and chunks per graph of the split form, and the row stride of the partial rows in the workspace
void gsp_chunks(const gvqa_graph* g, int64_t C, int64_t* R, int* nch, int64_t* Cp) {
    const int64_t maxn = std::max<int64_t>(g->max_graph_nodes, 1), B = std::max<int64_t>(g->num_graphs, 1);
    *Cp = (int64_t)align_up((size_t)C, 4);
    // the grid is graphs x chunks for EVERY graph of the batch, and every chunk owns a row of Cp floats in the workspace
    const int64_t maxc = std::max<int64_t>(1, std::min<int64_t>(GSP_MAX_CHUNKS, std::min<int64_t>(GSP_MAX_GRID / B, GSP_MAX_PARTIAL / (B * *Cp))));
    int64_t r = std::max<int64_t>(1, GSP_CHUNK / C);
    if (cdiv(maxn, r) > maxc) r = cdiv(maxn, maxc);
    *R = r;
    *nch = (int)cdiv(maxn, r);
}
struct GspWs { float *MS, *P; bool ok; };
GspWs gsp_carve(const gvqa_graph* g, int nch, int64_t Cp, void* ws, size_t ws_bytes) {
    Carver cv(ws, ws_bytes);
    GspWs r;
    r.MS = cv.take<float>((size_t)g->num_graphs * nch * 2);
    r.P = cv.take<float>((size_t)g->num_graphs * nch * Cp);
    r.ok = ws != nullptr && cv.ok();
    return r;
}
int gsp_common_checks(const char* who, const gvqa_graph* g, int64_t C, int form) {
    GVQA_REQUIRE(g && g->valid && g->finalized, GVQA_E_INVALID, "%s: graph not built / not finalized", who);
    GVQA_REQUIRE(C >= 1 && C < (1ll << 30), GVQA_E_INVALID, "%s: C must be in [1, 2^30)", who);
    GVQA_REQUIRE(form >= 0 && form <= 2, GVQA_E_INVALID, "%s: form must be 0 (auto), 1 (workgroup per graph) or 2 (split)", who);
    GVQA_REQUIRE(g->num_graphs < (1ll << 31), GVQA_E_UNSUPPORTED, "%s: more than 2^31 - 1 graphs", who);
    return GVQA_OK;
}

}  // namespace
}  // namespace gvqa

extern "C" size_t gvqa_graph_softmax_pool_workspace_bytes(const gvqa_graph* g, int64_t C) {
    using namespace gvqa;
    if (!g || !g->finalized || C < 1 || C >= (1ll << 30) || g->num_graphs <= 0) return 0;
    int64_t R, Cp; int nch;
    gsp_chunks(g, C, &R, &nch, &Cp);
    return align_up((size_t)g->num_graphs * nch * 2 * sizeof(float), 256) + align_up((size_t)g->num_graphs * nch * Cp * sizeof(float), 256);
}

extern "C" int gvqa_graph_softmax_pool_form(const gvqa_graph* g, int64_t C) {
    using namespace gvqa;
    if (int rc = gsp_common_checks("graph_softmax_pool_form", g, C, 0)) return rc;
    return gsp_pick_form(g, C, 0);
}

extern "C" int gvqa_graph_softmax_pool_forward(const gvqa_graph* g, int64_t C, const float* score, int64_t ld_score, const float* x, int64_t ld_x,
                                               float* gate, float* out, int64_t ld_out, int form, void* ws, size_t ws_bytes, void* stream_) {
    using namespace gvqa;
    if (int rc = gsp_common_checks("graph_softmax_pool_forward", g, C, form)) return rc;
    GVQA_REQUIRE(ld_x >= C && ld_out >= C && ld_score >= 1, GVQA_E_INVALID, "graph_softmax_pool_forward: row strides below their width");
    if (g->num_graphs == 0 || g->num_nodes == 0) return GVQA_OK;
    GVQA_REQUIRE(score && x && gate && out, GVQA_E_INVALID, "graph_softmax_pool_forward: null tensor");
    int64_t R, Cp; int nch;
    gsp_chunks(g, C, &R, &nch, &Cp);
    const GspWs w_ = gsp_carve(g, nch, Cp, ws, ws_bytes);
    GVQA_REQUIRE(w_.ok, GVQA_E_WORKSPACE, "graph_softmax_pool_forward: workspace too small");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool v4 = C % 4 == 0 && ld_x % 4 == 0 && ld_out % 4 == 0 && aligned16(x) && aligned16(out) && aligned16(w_.P);
    const unsigned B = (unsigned)g->num_graphs;
    if (gsp_pick_form(g, C, form) == 1) {
        if (v4) hipLaunchKernelGGL(k_gsp_fwd_wg<4>, dim3(B), dim3(256), 0, stream, (int)C, g->graph_ptr, score, ld_score, x, ld_x, gate, out, ld_out);
        else hipLaunchKernelGGL(k_gsp_fwd_wg<1>, dim3(B), dim3(256), 0, stream, (int)C, g->graph_ptr, score, ld_score, x, ld_x, gate, out, ld_out);
    } else {
        const dim3 grid(B, (unsigned)nch);
        if (v4) {
            hipLaunchKernelGGL(k_gsp_fwd_split_a<4>, grid, dim3(256), 0, stream, (int)C, R, nch, Cp, g->graph_ptr, score, ld_score, x, ld_x, w_.MS, w_.P);
            hipLaunchKernelGGL(k_gsp_fwd_split_b<4>, grid, dim3(256), 0, stream, (int)C, R, nch, Cp, g->graph_ptr, score, ld_score, w_.MS, w_.P, gate, out, ld_out);
        } else {
            hipLaunchKernelGGL(k_gsp_fwd_split_a<1>, grid, dim3(256), 0, stream, (int)C, R, nch, Cp, g->graph_ptr, score, ld_score, x, ld_x, w_.MS, w_.P);
            hipLaunchKernelGGL(k_gsp_fwd_split_b<1>, grid, dim3(256), 0, stream, (int)C, R, nch, Cp, g->graph_ptr, score, ld_score, w_.MS, w_.P, gate, out, ld_out);
        }
    }
    GVQA_LAUNCH_CHECK();
    return GVQA_OK;
}

extern "C" int gvqa_graph_softmax_pool_backward(const gvqa_graph* g, int64_t C, const float* x, int64_t ld_x, const float* gate, const float* dout,
                                                int64_t ld_dout, const float* dgate, float* dscore, float* dx, int64_t ld_dx, int form, void* ws,
                                                size_t ws_bytes, void* stream_) {
    using namespace gvqa;
    if (int rc = gsp_common_checks("graph_softmax_pool_backward", g, C, form)) return rc;
    GVQA_REQUIRE(ld_x >= C && ld_dout >= C && (!dx || ld_dx >= C), GVQA_E_INVALID, "graph_softmax_pool_backward: row strides below their width");
    if (g->num_graphs == 0 || g->num_nodes == 0) return GVQA_OK;
    GVQA_REQUIRE(x && gate && dout, GVQA_E_INVALID, "graph_softmax_pool_backward: null tensor");
    int64_t R, Cp; int nch;
    gsp_chunks(g, C, &R, &nch, &Cp);
    const GspWs w_ = gsp_carve(g, nch, Cp, ws, ws_bytes);
    GVQA_REQUIRE(w_.ok, GVQA_E_WORKSPACE, "graph_softmax_pool_backward: workspace too small");
    if (!dscore && !dx) return GVQA_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool v4 = C % 4 == 0 && ld_x % 4 == 0 && ld_dout % 4 == 0 && (!dx || ld_dx % 4 == 0) && aligned16(x) && aligned16(dout) && aligned16(dx);
    const unsigned B = (unsigned)g->num_graphs;
    if (gsp_pick_form(g, C, form) == 1) {
        if (v4) hipLaunchKernelGGL(k_gsp_bwd_wg<4>, dim3(B), dim3(256), 0, stream, (int)C, g->graph_ptr, x, ld_x, gate, dout, ld_dout, dgate, dscore, dx, ld_dx);
        else hipLaunchKernelGGL(k_gsp_bwd_wg<1>, dim3(B), dim3(256), 0, stream, (int)C, g->graph_ptr, x, ld_x, gate, dout, ld_dout, dgate, dscore, dx, ld_dx);
    } else {
        const dim3 grid(B, (unsigned)nch);
        if (v4) hipLaunchKernelGGL(k_gsp_bwd_split_a<4>, grid, dim3(256), 0, stream, (int)C, R, nch, g->graph_ptr, x, ld_x, gate, dout, ld_dout, dgate, dscore, dx, ld_dx, w_.MS);
        else hipLaunchKernelGGL(k_gsp_bwd_split_a<1>, grid, dim3(256), 0, stream, (int)C, R, nch, g->graph_ptr, x, ld_x, gate, dout, ld_dout, dgate, dscore, dx, ld_dx, w_.MS);
        if (dscore) hipLaunchKernelGGL(k_gsp_bwd_split_b, grid, dim3(256), 0, stream, R, nch, g->graph_ptr, gate, w_.MS, dscore);
    }
    GVQA_LAUNCH_CHECK();
    return GVQA_OK;
}
