// Graph LayerNorm, forward and backward (graph_utils/my_graph_layernorm.py:52-78): one normalisation per graph over its nodes x channels,
// 1-element weight / bias, eps OUTSIDE the square root.  Per graph g with n_g nodes, M = max(n_g, 1) D:
//   forward : mu = sum x / M;  xc = x - mu;  sigma = sqrt(sum xc^2 / M) (the variance of the CENTRED values, never E[x^2] - mu^2);
//             out = xc / (sigma + eps) * w + b;  stats[g] = (mu, sigma)
//   backward: y = xc / (sigma + eps) recomputed from x and stats (nothing else is saved);  S1 = sum_g dout, S2 = sum_g dout y;
//             dx = (w dout - w S1 / M) / (sigma + eps) - y (w S2) / (M sigma);  dweight = sum over graphs of S2, dbias = of S1
// Every value is taken relative to the graph's PIVOT p = its first element before it is summed: x - p is exact (or nearly) for values near
// p, so a large common offset (|mean| >> sigma) costs one rounding of the mean instead of one per addition, and xc = (x - p) - mean(x - p).
//
// Degenerate graphs.  An empty graph is skipped; its stats row is (0, 0).  sigma == 0 (a constant graph): out = b, as the reference; in the
// backward the variance term is DROPPED, dx = (w dout - mean(w dout)) / eps -- the reference's autograd gives NaN there (d sqrt at 0), this
// is the limit of the formula with y = 0 and a deliberate difference.
//
// Two forms, picked per call by gln_pick_form from the handle's statistics (max_graph_nodes x D):
//   (1) one 256-thread workgroup per graph.  The passes re-read the graph's rows (a workload graph is 6-40 nodes x 300-512 channels, <= 80 KB) from
//       the caches behind the CU -- which level serves them is not measured: eight resident workgroups per CU hold more than an XCD's 4 MiB L2 at
//       the workload's shapes, so the 256 MiB Infinity Cache is the likely one.  No LDS image: 80 KB of the CU's 160 KiB per workgroup would
//       leave two workgroups per CU where this form runs eight.
//   (2) split: a graph is cut into chunks of GLN_CHUNK elements, one workgroup each; the chunks' partial sums go to the workspace and EVERY
//       workgroup of the next pass adds its graph's partials itself, in an order fixed by (thread, chunk): the same bits in every
//       workgroup and every run, no atomics, no extra reduction launch.  For large segments and batch = None (one segment).
// dweight / dbias: per-graph (S1, S2) in the workspace, then one workgroup adds them in a fixed order.  No float atomics anywhere.
//
// Rows: x / out / dout / dx are [N, ld_*] with ld_* >= D elements.  16-byte accesses when D, every row stride and every pointer allow it,
// scalar ones otherwise.  out must not alias x (the passes re-read x), dx must not alias x or dout.
#include <algorithm>

#include "common.h"

namespace gvqa {
namespace {

constexpr int64_t GLN_CHUNK = 8192;        // elements per workgroup of the split form (32 KB: 8 float4 per thread)
constexpr int GLN_MAX_CHUNKS = 1024;       // chunks per graph at most (larger segments get larger chunks): the in-kernel combine reads <= 4 per thread
constexpr int GLN_BLK = 8;                 // units per block sum of a thread's two-level sums
constexpr int64_t GLN_SPLIT_MIN = 65536;   // auto rule: split form when max_graph_nodes x D > this (the last measured size at which form 1 is not slower)
constexpr int64_t GLN_MAX_GRID = 1 << 22;  // graphs x chunks of a split launch at most (B > 4096: fewer, larger chunks per graph), which also bounds the workspace at 32 MB + 8 B

template <int V> struct GlnVec { float v[V]; };
template <int V> __device__ __forceinline__ GlnVec<V> gln_load(const float* __restrict__ p) {
    GlnVec<V> o;
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        o.v[0] = t.x; o.v[1] = t.y; o.v[2] = t.z; o.v[3] = t.w;
    } else {
        o.v[0] = *p;
    }
    return o;
}
template <int V> __device__ __forceinline__ void gln_store(float* __restrict__ p, const GlnVec<V>& o) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(o.v[0], o.v[1], o.v[2], o.v[3]);
    else *p = o.v[0];
}
// unit q (V consecutive channels) of a segment -> row within the segment and first channel.  flat: every row stride == D, the segment is one run
template <int V> __device__ __forceinline__ void gln_rc(int64_t q, int Dq, bool flat, int64_t& r, int64_t& c) {
    if (flat) { r = 0; c = q * V; }
    else { r = q / Dq; c = (q - r * Dq) * V; }
}

// sums over the 256 threads, the four waves added in index order (red: 8 floats of LDS)
__device__ __forceinline__ float gln_block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ void gln_block_sum2(float& a, float& b, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = a; red[4 + (threadIdx.x >> 6)] = b; }
    __syncthreads();
    a = (red[0] + red[1]) + (red[2] + red[3]);
    b = (red[4] + red[5]) + (red[6] + red[7]);
}

// ---- passes over the units [q0, q1) of the segment that starts at row n0 (shared by both forms) ----
// A thread's sum is two-level: GLN_BLK units into a block sum, block sums into the total.  One chain over the 3500 values a thread of form 1 owns in a
// 3000 x 300 segment loses 7e-6 of a sum of gradients that cancels to 164 out of 900 000 terms (fp64 reference); the two-level order 3e-7.
template <int V> __device__ __forceinline__ float gln_pass_sum(int64_t q0, int64_t q1, int Dq, bool flat, const float* __restrict__ x, int64_t n0,
                                                               int64_t ldx, float p) {
    float s = 0.f, blk = 0.f;
    int it = 0;
#pragma unroll 4
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
        int64_t r, c;
        gln_rc<V>(q, Dq, flat, r, c);
        const GlnVec<V> xv = gln_load<V>(x + (n0 + r) * ldx + c);
#pragma unroll
        for (int k = 0; k < V; ++k) blk += xv.v[k] - p;
        if ((++it & (GLN_BLK - 1)) == 0) { s += blk; blk = 0.f; }
    }
    return s + blk;
}
template <int V> __device__ __forceinline__ float gln_pass_sq(int64_t q0, int64_t q1, int Dq, bool flat, const float* __restrict__ x, int64_t n0,
                                                              int64_t ldx, float p, float ms) {
    float s = 0.f, blk = 0.f;
    int it = 0;
#pragma unroll 4
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
        int64_t r, c;
        gln_rc<V>(q, Dq, flat, r, c);
        const GlnVec<V> xv = gln_load<V>(x + (n0 + r) * ldx + c);
#pragma unroll
        for (int k = 0; k < V; ++k) { const float d = (xv.v[k] - p) - ms; blk += d * d; }
        if ((++it & (GLN_BLK - 1)) == 0) { s += blk; blk = 0.f; }
    }
    return s + blk;
}
template <int V> __device__ __forceinline__ void gln_pass_apply(int64_t q0, int64_t q1, int Dq, bool flat, const float* __restrict__ x, int64_t n0,
                                                                int64_t ldx, float p, float ms, float sd, float ww, float bb,
                                                                float* __restrict__ out, int64_t ldo) {
#pragma unroll 4
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
        int64_t r, c;
        gln_rc<V>(q, Dq, flat, r, c);
        const GlnVec<V> xv = gln_load<V>(x + (n0 + r) * ldx + c);
        GlnVec<V> o;
#pragma unroll
        for (int k = 0; k < V; ++k) o.v[k] = ((xv.v[k] - p) - ms) / sd * ww + bb;
        gln_store<V>(out + (n0 + r) * ldo + c, o);
    }
}
template <int V> __device__ __forceinline__ void gln_pass_bwd_sum(int64_t q0, int64_t q1, int Dq, bool flat, const float* __restrict__ x, int64_t n0,
                                                                  int64_t ldx, const float* __restrict__ dout, int64_t ldd, float mu, float sd,
                                                                  float& s1, float& s2) {
    float b1 = 0.f, b2 = 0.f;
    int it = 0;
#pragma unroll 4
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
        int64_t r, c;
        gln_rc<V>(q, Dq, flat, r, c);
        const GlnVec<V> xv = gln_load<V>(x + (n0 + r) * ldx + c), gv = gln_load<V>(dout + (n0 + r) * ldd + c);
#pragma unroll
        for (int k = 0; k < V; ++k) { b1 += gv.v[k]; b2 += gv.v[k] * ((xv.v[k] - mu) / sd); }
        if ((++it & (GLN_BLK - 1)) == 0) { s1 += b1; s2 += b2; b1 = b2 = 0.f; }
    }
    s1 += b1; s2 += b2;
}
// dx = (w dout - a) / sd - y bc, a = w S1 / M, bc = sigma > 0 ? w S2 / (M sigma) : 0
template <int V> __device__ __forceinline__ void gln_pass_bwd_apply(int64_t q0, int64_t q1, int Dq, bool flat, const float* __restrict__ x, int64_t n0,
                                                                    int64_t ldx, const float* __restrict__ dout, int64_t ldd, float mu, float sd,
                                                                    float ww, float a, float bc, float* __restrict__ dx, int64_t lddx) {
#pragma unroll 4
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
        int64_t r, c;
        gln_rc<V>(q, Dq, flat, r, c);
        const GlnVec<V> xv = gln_load<V>(x + (n0 + r) * ldx + c), gv = gln_load<V>(dout + (n0 + r) * ldd + c);
        GlnVec<V> o;
#pragma unroll
        for (int k = 0; k < V; ++k) o.v[k] = (ww * gv.v[k] - a) / sd - (xv.v[k] - mu) / sd * bc;
        gln_store<V>(dx + (n0 + r) * lddx + c, o);
    }
}

// ---- form 1: one workgroup per graph ----
template <int V>
__global__ __launch_bounds__(256) void k_gln_fwd_wg(int D, bool flat, const int32_t* __restrict__ graph_ptr, const float* __restrict__ x, int64_t ldx,
                                                    const float* __restrict__ w, const float* __restrict__ b, float eps, float* __restrict__ out,
                                                    int64_t ldo, float* __restrict__ stats) {
    __shared__ float red[8];
    const int64_t g = blockIdx.x, n0 = graph_ptr[g], n = graph_ptr[g + 1] - n0;
    if (n <= 0) {
        if (stats && threadIdx.x == 0) { stats[2 * g] = 0.f; stats[2 * g + 1] = 0.f; }
        return;
    }
    const int Dq = D / V;
    const int64_t Mq = n * Dq;
    const float norm = (float)(n * D), p = x[n0 * ldx];
    const float ww = w ? w[0] : 1.f, bb = b ? b[0] : 0.f;
    const float ms = gln_block_sum(gln_pass_sum<V>(0, Mq, Dq, flat, x, n0, ldx, p), red) / norm;
    const float sigma = sqrtf(gln_block_sum(gln_pass_sq<V>(0, Mq, Dq, flat, x, n0, ldx, p, ms), red) / norm);
    gln_pass_apply<V>(0, Mq, Dq, flat, x, n0, ldx, p, ms, sigma + eps, ww, bb, out, ldo);
    if (stats && threadIdx.x == 0) { stats[2 * g] = p + ms; stats[2 * g + 1] = sigma; }
}

template <int V>
__global__ __launch_bounds__(256) void k_gln_bwd_wg(int D, bool flat, const int32_t* __restrict__ graph_ptr, const float* __restrict__ x, int64_t ldx,
                                                    const float* __restrict__ dout, int64_t ldd, const float* __restrict__ w, float eps,
                                                    const float* __restrict__ stats, float* __restrict__ dx, int64_t lddx, float* __restrict__ G) {
    __shared__ float red[8];
    const int64_t g = blockIdx.x, n0 = graph_ptr[g], n = graph_ptr[g + 1] - n0;
    if (n <= 0) {
        if (threadIdx.x == 0) { G[2 * g] = 0.f; G[2 * g + 1] = 0.f; }
        return;
    }
    const int Dq = D / V;
    const int64_t Mq = n * Dq;
    const float norm = (float)(n * D), mu = stats[2 * g], sigma = stats[2 * g + 1], sd = sigma + eps;
    const float ww = w ? w[0] : 1.f;
    float s1 = 0.f, s2 = 0.f;
    gln_pass_bwd_sum<V>(0, Mq, Dq, flat, x, n0, ldx, dout, ldd, mu, sd, s1, s2);
    gln_block_sum2(s1, s2, red);
    if (threadIdx.x == 0) { G[2 * g] = s1; G[2 * g + 1] = s2; }
    if (!dx) return;
    gln_pass_bwd_apply<V>(0, Mq, Dq, flat, x, n0, ldx, dout, ldd, mu, sd, ww, ww * s1 / norm, sigma > 0.f ? ww * s2 / (norm * sigma) : 0.f, dx, lddx);
}

// ---- form 2: split.  Grid (graph, chunk); chunk c of a graph = units [c CHq, (c + 1) CHq) of its n Dq; P[(g nch + c) 2 + k] its partial sums ----
// sum of column k of a graph's nc chunk partials: thread t adds chunks t, t + 256, ..., then the block sum -- the same order in every workgroup
__device__ __forceinline__ float gln_combine(const float* __restrict__ Pg, int nc, int k, float* red) {
    float s = 0.f;
    for (int c = threadIdx.x; c < nc; c += 256) s += Pg[2 * c + k];
    return gln_block_sum(s, red);
}

template <int V, int PASS>      // PASS 0: P[.., 0] = sum (x - p);  1: P[.., 1] = sum of squared centred values;  2: out (and stats, by chunk 0)
__global__ __launch_bounds__(256) void k_gln_fwd_split(int D, bool flat, int64_t CHq, int nch, const int32_t* __restrict__ graph_ptr,
                                                       const float* __restrict__ x, int64_t ldx, const float* __restrict__ w, const float* __restrict__ b,
                                                       float eps, float* __restrict__ out, int64_t ldo, float* __restrict__ stats, float* __restrict__ P) {
    __shared__ float red[8];
    const int64_t g = blockIdx.x, c = blockIdx.y, n0 = graph_ptr[g], n = graph_ptr[g + 1] - n0;
    if (n <= 0) {
        if (PASS == 2 && c == 0 && stats && threadIdx.x == 0) { stats[2 * g] = 0.f; stats[2 * g + 1] = 0.f; }
        return;
    }
    const int Dq = D / V;
    const int64_t Mq = n * Dq, q0 = c * CHq, q1 = min(q0 + CHq, Mq);
    if (q0 >= Mq) return;
    const int nc = (int)min<int64_t>((Mq + CHq - 1) / CHq, nch);      // (<= nch whenever the handle's max_graph_nodes holds)
    float* Pg = P + g * nch * 2;
    const float norm = (float)(n * D), p = x[n0 * ldx];
    if (PASS == 0) {
        const float s = gln_block_sum(gln_pass_sum<V>(q0, q1, Dq, flat, x, n0, ldx, p), red);
        if (threadIdx.x == 0) Pg[2 * c] = s;
        return;
    }
    const float ms = gln_combine(Pg, nc, 0, red) / norm;
    if (PASS == 1) {
        const float s = gln_block_sum(gln_pass_sq<V>(q0, q1, Dq, flat, x, n0, ldx, p, ms), red);
        if (threadIdx.x == 0) Pg[2 * c + 1] = s;
        return;
    }
    const float sigma = sqrtf(gln_combine(Pg, nc, 1, red) / norm);
    gln_pass_apply<V>(q0, q1, Dq, flat, x, n0, ldx, p, ms, sigma + eps, w ? w[0] : 1.f, b ? b[0] : 0.f, out, ldo);
    if (c == 0 && stats && threadIdx.x == 0) { stats[2 * g] = p + ms; stats[2 * g + 1] = sigma; }
}

template <int V, int PASS>      // PASS 0: P[.., 0 / 1] = the chunk's (S1, S2);  1: G[g] = the graph's (S1, S2) (by chunk 0) and dx
__global__ __launch_bounds__(256) void k_gln_bwd_split(int D, bool flat, int64_t CHq, int nch, const int32_t* __restrict__ graph_ptr,
                                                       const float* __restrict__ x, int64_t ldx, const float* __restrict__ dout, int64_t ldd,
                                                       const float* __restrict__ w, float eps, const float* __restrict__ stats, float* __restrict__ dx,
                                                       int64_t lddx, float* __restrict__ P, float* __restrict__ G) {
    __shared__ float red[8];
    const int64_t g = blockIdx.x, c = blockIdx.y, n0 = graph_ptr[g], n = graph_ptr[g + 1] - n0;
    if (n <= 0) {
        if (PASS == 1 && c == 0 && threadIdx.x == 0) { G[2 * g] = 0.f; G[2 * g + 1] = 0.f; }
        return;
    }
    const int Dq = D / V;
    const int64_t Mq = n * Dq, q0 = c * CHq, q1 = min(q0 + CHq, Mq);
    if (q0 >= Mq) return;
    const int nc = (int)min<int64_t>((Mq + CHq - 1) / CHq, nch);      // (<= nch whenever the handle's max_graph_nodes holds)
    float* Pg = P + g * nch * 2;
    const float norm = (float)(n * D), mu = stats[2 * g], sigma = stats[2 * g + 1], sd = sigma + eps;
    if (PASS == 0) {
        float s1 = 0.f, s2 = 0.f;
        gln_pass_bwd_sum<V>(q0, q1, Dq, flat, x, n0, ldx, dout, ldd, mu, sd, s1, s2);
        gln_block_sum2(s1, s2, red);
        if (threadIdx.x == 0) { Pg[2 * c] = s1; Pg[2 * c + 1] = s2; }
        return;
    }
    const float s1 = gln_combine(Pg, nc, 0, red), s2 = gln_combine(Pg, nc, 1, red);
    if (c == 0 && threadIdx.x == 0) { G[2 * g] = s1; G[2 * g + 1] = s2; }
    if (!dx) return;
    const float ww = w ? w[0] : 1.f;
    gln_pass_bwd_apply<V>(q0, q1, Dq, flat, x, n0, ldx, dout, ldd, mu, sd, ww, ww * s1 / norm, sigma > 0.f ? ww * s2 / (norm * sigma) : 0.f, dx, lddx);
}

// dbias = sum_g G[g, 0], dweight = sum_g G[g, 1]: one workgroup, thread t adds graphs t, t + 1024, ..., the 16 waves in index order
__global__ __launch_bounds__(1024) void k_gln_param_finish(int64_t B, const float* __restrict__ G, float* __restrict__ dweight, float* __restrict__ dbias) {
    __shared__ float red[32];
    float s1 = 0.f, s2 = 0.f;
    for (int64_t g = threadIdx.x; g < B; g += 1024) { s1 += G[2 * g]; s2 += G[2 * g + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = s1; red[16 + (threadIdx.x >> 6)] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) { t1 += red[k]; t2 += red[16 + k]; }
        if (dbias) dbias[0] = t1;
        if (dweight) dweight[0] = t2;
    }
}

// The auto rule, in one place: the split form when the largest graph has more than GLN_SPLIT_MIN elements (a forced form is taken as given)
int gln_pick_form(const gvqa_graph* g, int64_t D, int form) {
    if (form == 1 || form == 2) return form;
    return (int64_t)g->max_graph_nodes * D > GLN_SPLIT_MIN ? 2 : 1;
}
// chunk size (elements, a multiple of 1024) and chunks per graph of the split form
void gln_chunks(const gvqa_graph* g, int64_t D, int64_t* CH, int* nch) {
    const int64_t maxM = std::max<int64_t>(g->max_graph_nodes, 1) * D;
    // the grid is graphs x chunks for EVERY graph of the batch (the small ones leave at once): one huge graph among very many small ones gets fewer chunks
    const int64_t maxc = std::min<int64_t>(GLN_MAX_CHUNKS, std::max<int64_t>(1, GLN_MAX_GRID / std::max<int64_t>(g->num_graphs, 1)));
    int64_t ch = GLN_CHUNK;
    if (cdiv(maxM, ch) > maxc) ch = (int64_t)align_up((size_t)cdiv(maxM, maxc), 1024);
    *CH = ch;
    *nch = (int)cdiv(maxM, ch);
}
struct GlnWs { float *P, *G; bool ok; };
GlnWs gln_carve(const gvqa_graph* g, int nch, void* ws, size_t ws_bytes) {
    Carver cv(ws, ws_bytes);
    GlnWs r;
    r.P = cv.take<float>((size_t)g->num_graphs * nch * 2);
    r.G = cv.take<float>((size_t)g->num_graphs * 2);
    r.ok = ws != nullptr && cv.ok();
    return r;
}
int gln_common_checks(const char* who, const gvqa_graph* g, int64_t D, int form) {
    GVQA_REQUIRE(g && g->valid && g->finalized, GVQA_E_INVALID, "%s: graph not built / not finalized", who);
    GVQA_REQUIRE(D >= 1 && D < (1ll << 31), GVQA_E_INVALID, "%s: D must be in [1, 2^31)", who);
    GVQA_REQUIRE(form >= 0 && form <= 2, GVQA_E_INVALID, "%s: form must be 0 (auto), 1 (workgroup per graph) or 2 (split)", who);
    GVQA_REQUIRE(g->num_graphs < (1ll << 31), GVQA_E_UNSUPPORTED, "%s: more than 2^31 - 1 graphs", who);
    return GVQA_OK;
}

}  // namespace
}  // namespace gvqa

extern "C" size_t gvqa_graph_layernorm_workspace_bytes(const gvqa_graph* g, int64_t D) {
    using namespace gvqa;
    if (!g || !g->finalized || D < 1 || g->num_graphs <= 0) return 0;
    int64_t CH; int nch;
    gln_chunks(g, D, &CH, &nch);
    return align_up((size_t)g->num_graphs * nch * 2 * sizeof(float), 256) + align_up((size_t)g->num_graphs * 2 * sizeof(float), 256);
}

extern "C" int gvqa_graph_layernorm_form(const gvqa_graph* g, int64_t D) {
    using namespace gvqa;
    if (int rc = gln_common_checks("graph_layernorm_form", g, D, 0)) return rc;
    return gln_pick_form(g, D, 0);
}

extern "C" int gvqa_graph_layernorm_forward(const gvqa_graph* g, int64_t D, const float* x, int64_t ld_x, const float* weight, const float* bias,
                                            float eps, float* out, int64_t ld_out, float* stats, int form, void* ws, size_t ws_bytes, void* stream_) {
    using namespace gvqa;
    if (int rc = gln_common_checks("graph_layernorm_forward", g, D, form)) return rc;
    GVQA_REQUIRE(ld_x >= D && ld_out >= D, GVQA_E_INVALID, "graph_layernorm_forward: row strides below D");
    if (g->num_graphs == 0 || g->num_nodes == 0) return GVQA_OK;
    GVQA_REQUIRE(x && out, GVQA_E_INVALID, "graph_layernorm_forward: null tensor");
    int64_t CH; int nch;
    gln_chunks(g, D, &CH, &nch);
    const GlnWs w_ = gln_carve(g, nch, ws, ws_bytes);
    GVQA_REQUIRE(w_.ok, GVQA_E_WORKSPACE, "graph_layernorm_forward: workspace too small");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool v4 = D % 4 == 0 && ld_x % 4 == 0 && ld_out % 4 == 0 && aligned16(x) && aligned16(out);
    const bool flat = ld_x == D && ld_out == D;
    const unsigned B = (unsigned)g->num_graphs;
    if (gln_pick_form(g, D, form) == 1) {
        if (v4) hipLaunchKernelGGL(k_gln_fwd_wg<4>, dim3(B), dim3(256), 0, stream, (int)D, flat, g->graph_ptr, x, ld_x, weight, bias, eps, out, ld_out, stats);
        else hipLaunchKernelGGL(k_gln_fwd_wg<1>, dim3(B), dim3(256), 0, stream, (int)D, flat, g->graph_ptr, x, ld_x, weight, bias, eps, out, ld_out, stats);
    } else {
        const dim3 grid(B, (unsigned)nch);
#define GLN_FWD(V, PASS) hipLaunchKernelGGL((k_gln_fwd_split<V, PASS>), grid, dim3(256), 0, stream, (int)D, flat, CH / V, nch, g->graph_ptr, x, ld_x, weight, bias, \
                                            eps, out, ld_out, stats, w_.P)
        if (v4) { GLN_FWD(4, 0); GLN_FWD(4, 1); GLN_FWD(4, 2); }
        else { GLN_FWD(1, 0); GLN_FWD(1, 1); GLN_FWD(1, 2); }
#undef GLN_FWD
    }
    GVQA_LAUNCH_CHECK();
    return GVQA_OK;
}

extern "C" int gvqa_graph_layernorm_backward(const gvqa_graph* g, int64_t D, const float* x, int64_t ld_x, const float* dout, int64_t ld_dout,
                                             const float* weight, float eps, const float* stats, float* dx, int64_t ld_dx, float* dweight, float* dbias,
                                             int form, void* ws, size_t ws_bytes, void* stream_) {
    using namespace gvqa;
    if (int rc = gln_common_checks("graph_layernorm_backward", g, D, form)) return rc;
    GVQA_REQUIRE(ld_x >= D && ld_dout >= D && (!dx || ld_dx >= D), GVQA_E_INVALID, "graph_layernorm_backward: row strides below D");
    if (g->num_graphs == 0 || g->num_nodes == 0) return GVQA_OK;
    GVQA_REQUIRE(x && dout && stats, GVQA_E_INVALID, "graph_layernorm_backward: null tensor");
    if (!dx && !dweight && !dbias) return GVQA_OK;
    int64_t CH; int nch;
    gln_chunks(g, D, &CH, &nch);
    const GlnWs w_ = gln_carve(g, nch, ws, ws_bytes);
    GVQA_REQUIRE(w_.ok, GVQA_E_WORKSPACE, "graph_layernorm_backward: workspace too small");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool v4 = D % 4 == 0 && ld_x % 4 == 0 && ld_dout % 4 == 0 && (!dx || ld_dx % 4 == 0) && aligned16(x) && aligned16(dout) && aligned16(dx);
    const bool flat = ld_x == D && ld_dout == D && (!dx || ld_dx == D);
    const unsigned B = (unsigned)g->num_graphs;
    if (gln_pick_form(g, D, form) == 1) {
        if (v4) hipLaunchKernelGGL(k_gln_bwd_wg<4>, dim3(B), dim3(256), 0, stream, (int)D, flat, g->graph_ptr, x, ld_x, dout, ld_dout, weight, eps, stats, dx, ld_dx, w_.G);
        else hipLaunchKernelGGL(k_gln_bwd_wg<1>, dim3(B), dim3(256), 0, stream, (int)D, flat, g->graph_ptr, x, ld_x, dout, ld_dout, weight, eps, stats, dx, ld_dx, w_.G);
    } else {
        // (without dx the second pass only combines: chunk 0 of every graph)
        const dim3 grid(B, (unsigned)nch), grid1(B, dx ? (unsigned)nch : 1u);
#define GLN_BWD(V, PASS, GRID) hipLaunchKernelGGL((k_gln_bwd_split<V, PASS>), GRID, dim3(256), 0, stream, (int)D, flat, CH / V, nch, g->graph_ptr, x, ld_x, dout, \
                                                  ld_dout, weight, eps, stats, dx, ld_dx, w_.P, w_.G)
        if (v4) { GLN_BWD(4, 0, grid); GLN_BWD(4, 1, grid1); }
        else { GLN_BWD(1, 0, grid); GLN_BWD(1, 1, grid1); }
#undef GLN_BWD
    }
    if (dweight || dbias) hipLaunchKernelGGL(k_gln_param_finish, dim3(1), dim3(1024), 0, stream, (int64_t)g->num_graphs, w_.G, dweight, dbias);
    GVQA_LAUNCH_CHECK();
    return GVQA_OK;
}
