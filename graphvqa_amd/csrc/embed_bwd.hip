// Table gradient of the token-embedding sums (gvqa_embed_sum, encoder.hip):
//     dtable[v, :] = sum over (r, t) with clamp(tokens[r, t]) == v, v != ignore, of sign(r) * dout[r, :].
//
// Deterministic and without a [rows T, D] array: the occurrences o = r T + t are put in token order by a STABLE counting sort, the
// sorted list is cut into fixed chunks that are summed in ascending o, and a token that spans chunks gets its per-chunk partial rows
// added in chunk order.  The order of every fp32 addition depends on `tokens` alone.
//   (a) k_eb_hist   one workgroup per slice of EB_SLICE occurrences: LDS histogram (integer atomics: the counts do not depend on
//                   arrival order) -> hist[token][slice]; ignored occurrences are dropped here and never seen again.
//       scan        graph.hip's three scan kernels over hist in (token, slice) order: the first sorted position of every
//                   (token, slice) pair; element [V ns] is M, the number of kept occurrences.
//       k_eb_place  one wave per slice walks it 64 occurrences at a time; the rank of an occurrence among the lanes of its token
//                   comes from ballots (lane order = occurrence order), the running position of each token from an LDS cursor
//                   -> sorted[pos] = {row, token}, ascending o inside every token.
//   (b) k_eb_sum    one wave per chunk of EB_CHUNK sorted positions, lanes along D (16 B per lane, W = 4).  The chunk's
//                   {row, token, sign} list sits in LDS, so the row addresses are known up front: four rows are in flight, no
//                   index-then-row chain.  A run that lies inside the chunk is written straight to dtable; a run that came in from
//                   the previous chunk / goes on into the next one leaves as the chunk's head / tail partial row.
//   (c) k_eb_combine  one wave per token: zero rows for tokens without occurrences, and for a token over chunks c0 < c1 the row
//                   tail[c0] + head[c0 + 1] + ... + head[c1].  Tokens inside one chunk were finished by (b).
// A token with 65 536 occurrences is 512 chunks on 512 waves, then 512 row adds by one wave.
#include "common.h"

namespace gvqa {

constexpr int EB_SLICE = GVQA_EMBED_BWD_SLICE;
constexpr int EB_CHUNK = GVQA_EMBED_BWD_CHUNK;
constexpr int EB_MAX_V = GVQA_EMBED_BWD_MAX_V;
constexpr int EB_WAVES = 4;          // chunks (k_eb_sum) / tokens (k_eb_combine) per workgroup

__device__ __forceinline__ int eb_clamp(int64_t id, int V) { return (int)(id < 0 ? 0 : (id >= V ? V - 1 : id)); }

__global__ __launch_bounds__(256) void k_eb_hist(int64_t n, int V, int ns, const int64_t* __restrict__ tok, int ignore,
                                                 int32_t* __restrict__ hist) {
    __shared__ int h[EB_MAX_V];
    const int slice = blockIdx.x;
    for (int v = threadIdx.x; v < V; v += 256) h[v] = 0;
    __syncthreads();
    const int64_t o0 = (int64_t)slice * EB_SLICE;
    for (int i = threadIdx.x; i < EB_SLICE; i += 256) {
        const int64_t o = o0 + i;
        if (o < n) {
            const int id = eb_clamp(tok[o], V);
            if (id != ignore) atomicAdd(&h[id], 1);
        }
    }
    __syncthreads();
    for (int v = threadIdx.x; v < V; v += 256) hist[(int64_t)v * ns + slice] = h[v];
    if (slice == 0 && threadIdx.x == 0) hist[(int64_t)V * ns] = 0;       // (its scan is M)
}

__global__ __launch_bounds__(64) void k_eb_place(int64_t n, int T, int V, int ns, const int64_t* __restrict__ tok, int ignore,
                                                 const int32_t* __restrict__ scan, int2* __restrict__ sorted) {
    __shared__ int cur[EB_MAX_V];
    const int slice = blockIdx.x, lane = threadIdx.x;
    for (int v = lane; v < V; v += 64) cur[v] = scan[(int64_t)v * ns + slice];
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t o0 = (int64_t)slice * EB_SLICE;
    for (int i0 = 0; i0 < EB_SLICE; i0 += 64) {
        const int64_t o = o0 + i0 + lane;
        int id = -1;
        if (o < n) id = eb_clamp(tok[o], V);
        const bool active = id >= 0 && id != ignore;
        // rank of this lane among the lanes with its token, and their number: one ballot per distinct token of the 64
        unsigned long long todo = __ballot(active);
        int rank = 0, cnt = 0;
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int t = __shfl(id, leader, 64);
            const bool mine = active && id == t;
            const unsigned long long m = __ballot(mine);
            if (mine) {
                rank = __popcll(m & below);
                cnt = __popcll(m);
            }
            todo &= ~m;
        }
        if (active) {
            const int base = cur[id];
            sorted[base + rank] = make_int2((int)((uint32_t)o / (uint32_t)T), id);
            if (rank == cnt - 1) cur[id] = base + cnt;
        }
        __syncthreads();
    }
}

// W floats per lane and column slot, NQ column slots per lane: one pass over the chunk covers 64 NQ W columns.
template <int W, int NQ>
__global__ __launch_bounds__(64 * EB_WAVES) void k_eb_sum(int V, int D, int ns, int64_t nc, const int32_t* __restrict__ scan,
                                                          const int2* __restrict__ sorted, const uint8_t* __restrict__ neg,
                                                          const float* __restrict__ dout, int64_t ldd, float* __restrict__ dtable,
                                                          float* __restrict__ partial) {
    __shared__ int s_r[EB_WAVES][EB_CHUNK];
    __shared__ int s_tok[EB_WAVES][EB_CHUNK];
    __shared__ float s_sg[EB_WAVES][EB_CHUNK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * EB_WAVES + wave;
    const int64_t M = scan[(int64_t)V * ns];
    const int64_t start = c * EB_CHUNK;
    int cnt = 0;
    if (c < nc && start < M) cnt = (int)(M - start < EB_CHUNK ? M - start : EB_CHUNK);
    for (int p = lane; p < cnt; p += 64) {
        const int2 e = sorted[start + p];
        s_r[wave][p] = e.x;
        s_tok[wave][p] = e.y;
        s_sg[wave][p] = (neg && neg[e.x]) ? -1.f : 1.f;
    }
    __syncthreads();
    if (cnt == 0) return;
    const int* rr = s_r[wave];
    const int* tt = s_tok[wave];
    const float* ss = s_sg[wave];
    const int DW = D / W;                              // column slots
    constexpr int U = 4;                               // rows in flight

    for (int cb = 0; cb < DW; cb += 64 * NQ) {
        int col[NQ];
        bool on[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int s = cb + q * 64 + lane;
            on[q] = s < DW;
            col[q] = (on[q] ? s : 0) * W;
        }
        float acc[NQ][W];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int j = 0; j < W; ++j) acc[q][j] = 0.f;
        int cur = tt[0], ps = 0;

        // a finished run [ps, pe) of token `tk`: to dtable when it lies inside the chunk, else the chunk's head / tail partial row
        auto flush = [&](int tk, int ps_, int pe) {
            float* dst = dtable + (int64_t)tk * D;
            if (ps_ == 0 && (int64_t)scan[(int64_t)tk * ns] < start) dst = partial + (c * 2) * D;
            else if (pe == cnt && (int64_t)scan[(int64_t)(tk + 1) * ns] > start + pe) dst = partial + (c * 2 + 1) * D;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (!on[q]) continue;
                if constexpr (W == 4) *reinterpret_cast<float4*>(dst + col[q]) = make_float4(acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
                else dst[col[q]] = acc[q][0];
            }
        };

        for (int p = 0; p < cnt; p += U) {
            float v[U][NQ][W];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int pi = p + u < cnt ? p + u : cnt - 1;
                const float* row = dout + (int64_t)rr[pi] * ldd;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    if constexpr (W == 4) {
                        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (on[q]) x = *reinterpret_cast<const float4*>(row + col[q]);
                        v[u][q][0] = x.x; v[u][q][1] = x.y; v[u][q][2] = x.z; v[u][q][3] = x.w;
                    } else {
                        v[u][q][0] = on[q] ? row[col[q]] : 0.f;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (p + u >= cnt) break;
                const int tk = tt[p + u];
                if (tk != cur) {
                    flush(cur, ps, p + u);
                    cur = tk;
                    ps = p + u;
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
#pragma unroll
                        for (int j = 0; j < W; ++j) acc[q][j] = 0.f;
                }
                const float sg = ss[p + u];
#pragma unroll
                for (int q = 0; q < NQ; ++q)
#pragma unroll
                    for (int j = 0; j < W; ++j) acc[q][j] += sg * v[u][q][j];
            }
        }
        flush(cur, ps, cnt);
    }
}

template <int W>
__global__ __launch_bounds__(64 * EB_WAVES) void k_eb_combine(int V, int D, int ns, const int32_t* __restrict__ scan,
                                                              const float* __restrict__ partial, float* __restrict__ dtable) {
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * EB_WAVES + (threadIdx.x >> 6);
    if (v >= V) return;
    const int64_t s = scan[(int64_t)v * ns], e = scan[(int64_t)(v + 1) * ns];
    const int64_t c0 = s / EB_CHUNK, c1 = e > s ? (e - 1) / EB_CHUNK : c0;
    if (e > s && c0 == c1) return;                     // k_eb_sum wrote the row
    const int DW = D / W;
    float* dst = dtable + (int64_t)v * D;
    for (int sl = lane; sl < DW; sl += 64) {
        const int col = sl * W;
        float acc[W];
#pragma unroll
        for (int j = 0; j < W; ++j) acc[j] = 0.f;
        if (e > s) {
            // tail of c0, then the heads of c0 + 1 .. c1, in that order (four rows in flight)
            const float* p0 = partial + (c0 * 2 + 1) * D + col;
            if constexpr (W == 4) {
                const float4 x = *reinterpret_cast<const float4*>(p0);
                acc[0] = x.x; acc[1] = x.y; acc[2] = x.z; acc[3] = x.w;
            } else {
                acc[0] = *p0;
            }
            for (int64_t cc = c0 + 1; cc <= c1; cc += 4) {
                float x[4][W];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t ci = cc + u <= c1 ? cc + u : c1;
                    const float* pp = partial + (ci * 2) * D + col;
                    if constexpr (W == 4) {
                        const float4 y = *reinterpret_cast<const float4*>(pp);
                        x[u][0] = y.x; x[u][1] = y.y; x[u][2] = y.z; x[u][3] = y.w;
                    } else {
                        x[u][0] = *pp;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (cc + u <= c1)
#pragma unroll
                        for (int j = 0; j < W; ++j) acc[j] += x[u][j];
            }
        }
        if constexpr (W == 4) *reinterpret_cast<float4*>(dst + col) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else dst[col] = acc[0];
    }
}

struct EbLayout {
    int64_t n, ns, nc, hn;      // occurrences, slices, chunks, histogram entries (V ns + 1)
    size_t hist, scan, tiles, sorted, partial, total;
    bool ok;
};

static EbLayout eb_layout(int64_t rows, int32_t T, int32_t V, int32_t D) {
    EbLayout L = {};
    if (rows < 0 || T <= 0 || V <= 0 || D <= 0 || V > EB_MAX_V) return L;
    if (rows > (int64_t)0x7fffffff / T) return L;
    L.n = rows * T;
    L.ns = cdiv(L.n, EB_SLICE);
    L.nc = cdiv(L.n, EB_CHUNK);
    L.hn = (int64_t)V * L.ns + 1;
    if (L.hn >= (int64_t)0x7fffffff) return L;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes, 256); return o; };
    L.hist = take((size_t)L.hn * 4);
    L.scan = take((size_t)L.hn * 4);
    L.tiles = take((size_t)(exclusive_scan_tiles(L.hn) + 1) * 4);
    L.sorted = take((size_t)L.n * sizeof(int2));
    L.partial = take((size_t)L.nc * 2 * (size_t)D * 4);
    L.total = off > 0 ? off : 256;
    L.ok = true;
    return L;
}

}  // namespace gvqa

using namespace gvqa;

extern "C" {

size_t gvqa_embed_sum_backward_workspace_bytes(int64_t rows, int32_t T, int32_t V, int32_t D) {
    const EbLayout L = eb_layout(rows, T, V, D);
    return L.ok ? L.total : 0;
}

int gvqa_embed_sum_backward(int64_t rows, int32_t T, int32_t V, int32_t D, const int64_t* tokens, const uint8_t* negate, int64_t ignore_index,
                            const float* dout, int64_t ldd, float* dtable, void* ws, size_t ws_bytes, void* stream_) {
    GVQA_REQUIRE(rows >= 0 && T > 0 && V > 0 && D > 0, GVQA_E_INVALID, "embed_sum_backward: bad dims");
    GVQA_REQUIRE(ignore_index >= -1 && ignore_index < V, GVQA_E_INVALID, "embed_sum_backward: ignore_index %lld outside [-1, %d)",
                 (long long)ignore_index, (int)V);
    const EbLayout L = eb_layout(rows, T, V, D);
    GVQA_REQUIRE(L.ok, GVQA_E_UNSUPPORTED, "embed_sum_backward: V = %d > %d or rows x T = %lld x %d past the kernels' int32 range", (int)V,
                 EB_MAX_V, (long long)rows, (int)T);
    GVQA_REQUIRE(dtable, GVQA_E_INVALID, "embed_sum_backward: null dtable");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (rows == 0) {
        GVQA_HIP_CHECK(hipMemsetAsync(dtable, 0, (size_t)V * D * sizeof(float), stream));
        return GVQA_OK;
    }
    GVQA_REQUIRE(tokens && dout, GVQA_E_INVALID, "embed_sum_backward: null tensor");
    GVQA_REQUIRE(ldd >= D, GVQA_E_INVALID, "embed_sum_backward: ldd %lld < D %d", (long long)ldd, (int)D);
    GVQA_REQUIRE(ws && ws_bytes >= L.total, GVQA_E_WORKSPACE, "embed_sum_backward: workspace %zu < %zu bytes", ws ? ws_bytes : (size_t)0, L.total);
    char* base = static_cast<char*>(ws);
    int32_t* hist = reinterpret_cast<int32_t*>(base + L.hist);
    int32_t* scan = reinterpret_cast<int32_t*>(base + L.scan);
    int32_t* tiles = reinterpret_cast<int32_t*>(base + L.tiles);
    int2* sorted = reinterpret_cast<int2*>(base + L.sorted);
    float* partial = reinterpret_cast<float*>(base + L.partial);
    const int ns = (int)L.ns, ign = (int)ignore_index;

    hipLaunchKernelGGL(k_eb_hist, dim3((unsigned)L.ns), dim3(256), 0, stream, L.n, (int)V, ns, tokens, ign, hist);
    const int rc = launch_exclusive_scan_i32(L.hn, hist, scan, tiles, stream);
    if (rc != GVQA_OK) return rc;
    hipLaunchKernelGGL(k_eb_place, dim3((unsigned)L.ns), dim3(64), 0, stream, L.n, (int)T, (int)V, ns, tokens, ign, (const int32_t*)scan, sorted);
    const bool v4 = D % 4 == 0 && ldd % 4 == 0 && aligned16(dout) && aligned16(dtable) && aligned16(ws);
    const dim3 gs((unsigned)cdiv(L.nc, EB_WAVES)), gc((unsigned)cdiv(V, EB_WAVES)), blk(64 * EB_WAVES);
    if (v4) {
        hipLaunchKernelGGL((k_eb_sum<4, 2>), gs, blk, 0, stream, (int)V, (int)D, ns, L.nc, (const int32_t*)scan, (const int2*)sorted, negate, dout, ldd,
                           dtable, partial);
        hipLaunchKernelGGL(k_eb_combine<4>, gc, blk, 0, stream, (int)V, (int)D, ns, (const int32_t*)scan, (const float*)partial, dtable);
    } else {
        hipLaunchKernelGGL((k_eb_sum<1, 4>), gs, blk, 0, stream, (int)V, (int)D, ns, L.nc, (const int32_t*)scan, (const int2*)sorted, negate, dout, ldd,
                           dtable, partial);
        hipLaunchKernelGGL(k_eb_combine<1>, gc, blk, 0, stream, (int)V, (int)D, ns, (const int32_t*)scan, (const float*)partial, dtable);
    }
    GVQA_LAUNCH_CHECK();
    return GVQA_OK;
}

}  // extern "C"
