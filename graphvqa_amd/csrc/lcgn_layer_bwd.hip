// gat_lcgn's attention for training (gfx950): the forward with a dropout mask, and its backward in two walks.
//
// Forward (k_lcgn_attention of lcgn_layer.hip, TR form), per head h, with g(n) the graph of node n and m the mask (or 1):
//   y[i]   = proj_cmd[g(i)] * x_r[i]                        z[e] = x_l[src_e] . y[dst_e]
//   alpha  = softmax over the in-edges of dst of leaky_relu(z)
//   v'[j]  = x_val[j] * cal_cmd[g(j)]                       o[i,h] = sum_{e -> i} alpha[e,h] m[e,h] v'[src_e,h,:]
// Backward, given G = dL/dout; G_h[i] = G[i, hC:(h+1)C] (concat) or G[i] / H (mean):
//   da[e]    = m[e] (G_h[dst_e] . v'[src_e])
//   dz[e]    = alpha[e] (da[e] - sum_{e' -> dst_e} alpha[e'] da[e']) (z[e] > 0 ? 1 : slope)
//   dy[i]    = sum_{e -> i}     dz[e] x_l[src_e]            d x_r[i]   = dy[i]  * proj_cmd[g(i)]
//   d x_l[j] = sum_{e: src = j} dz[e] y[dst_e]
//   dv'[j]   = sum_{e: src = j} alpha[e] m[e] G_h[dst_e]    d x_val[j] = dv'[j] * cal_cmd[g(j)]
//   d proj_cmd[b] = sum_{i in b} dy[i] * x_r[i]             d cal_cmd[b] = sum_{j in b} dv'[j] * x_val[j]
//
// k_lcgn_att_bwd_dst: one workgroup per destination, the forward's lane layout (a head's dot products reduce inside one wave);
// it walks the in-edges twice (da and the row sum, then z, dz and dy) and leaves dz [E, H] in the workspace.
// k_lcgn_att_bwd_src: one workgroup per source over the CSR of the transposed graph; nothing to reduce, one float4 column chunk
// per thread.  Both write the per-node rows dy * x_r and dv' * x_val to the workspace; gvqa_graph_segment_sum adds them per
// graph into dpc.  Every sum runs in CSR order: deterministic, no atomics.
#include "common.h"

namespace gvqa {

__device__ __forceinline__ float4 bld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void bst4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float bdot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float4 bmul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 bfma4(float s, float4 a, float4 c) {
    return make_float4(c.x + s * a.x, c.y + s * a.y, c.z + s * a.z, c.w + s * a.w);
}

constexpr int LCGN_BWD_ONE_WAVE_HC = 1024;       // as the forward: up to here one wave holds every head, else one wave per head

// Lane layout of k_lcgn_attention: the wave's hpw heads in aligned segments of LPH lanes, lane sl of head hl owns the float4 chunks
// sl, sl + LPH, ... (KC at most) of that head.  YL (KC = 16, one head of more than 2048 channels): y and G live in LDS
// (2 * 64 KC float4 per wave).  xg: the batch has edges across graphs (cal_cmd of the SOURCE's graph per edge; else it is folded into G
// once).  dz [E, H] (COO order) holds da between the two walks: the lane that wrote a value reads it back and hands it to its segment.
// rows [N, 2HC]: this kernel writes the left half (dy * x_r).
// YL runs one wave per workgroup (H = 1), so its launch bound is 64 threads: under 512 it spilled 20 registers.
template <int KC, bool YL>
__global__ __launch_bounds__(YL ? 64 : 512) void k_lcgn_att_bwd_dst(int H, int C, int hpw, int LPH, int concat, int xg, float slope,
                                                          const float* __restrict__ J, int64_t ldj, const float* __restrict__ pc,
                                                          int64_t ldpc, const float* __restrict__ alpha, const float* __restrict__ mask,
                                                          const float* __restrict__ dout, int64_t ldd, const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ csr_src, const int32_t* __restrict__ csr_eid,
                                                          const int32_t* __restrict__ node_graph, float* dz, float* __restrict__ dJ,
                                                          int64_t lddj, float* __restrict__ rows) {
    extern __shared__ float4 lcgn_bwd_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x;
    const int HC = H * C, Cq = C >> 2;
    const bool mean = !concat && H > 1;
    const int hl = lane / LPH, sl = lane - hl * LPH;
    const bool mine = hl < hpw;                  // this lane serves a head
    const bool lead = sl == 0 && mine;
    const int head = wave * hpw + hl;
    const int64_t hcol = (int64_t)head * C;
    const int g = node_graph[i];
    float4* ylds = lcgn_bwd_lds + wave * 2 * 64 * KC;
    const float fh = (float)H;
    bool ok[KC];
    float4 y[YL ? 1 : KC], gr[YL ? 1 : KC], dy[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int q = sl + k * LPH;
        ok[k] = mine && q < Cq;
        dy[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 yk = dy[k], gk = dy[k];
        if (ok[k]) {
            yk = bmul4(bld4(pc + (int64_t)g * ldpc + hcol + 4 * q), bld4(J + (int64_t)i * ldj + HC + hcol + 4 * q));
            gk = bld4(dout + (int64_t)i * ldd + (concat ? hcol : 0) + 4 * q);
            if (mean) gk = make_float4(gk.x / fh, gk.y / fh, gk.z / fh, gk.w / fh);
            if (!xg) gk = bmul4(gk, bld4(pc + (int64_t)g * ldpc + HC + hcol + 4 * q));   // every source shares the destination's cal_cmd row
        }
        if (YL) { ylds[k * 64 + lane] = yk; ylds[(KC + k) * 64 + lane] = gk; }
        else { y[YL ? 0 : k] = yk; gr[YL ? 0 : k] = gk; }
    }
    const float* xl_base = J + hcol;
    const float* xv_base = J + 2 * (int64_t)HC + hcol;
    const float* cc_base = pc + HC + hcol;
    const int lo = rowptr[i], hi = rowptr[i + 1];
    float S = 0.f;                               // sum over the in-edges of alpha * da
    for (int s = lo; s < hi; ++s) {
        const int src = csr_src[s];
        const int64_t ah = (int64_t)csr_eid[s] * H + head;
        const int gs = xg ? node_graph[src] : 0;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            if (!ok[k]) continue;
            const int64_t off = 4 * (int64_t)(sl + k * LPH);
            float4 xv = bld4(xv_base + (int64_t)src * ldj + off);
            if (xg) xv = bmul4(xv, bld4(cc_base + (int64_t)gs * ldpc + off));
            v += bdot4(xv, YL ? ylds[(KC + k) * 64 + lane] : gr[YL ? 0 : k]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            if (o < LPH) v += __shfl_xor(v, o, 64);
        const float da = mask && mine ? mask[ah] * v : v;
        S += (mine ? alpha[ah] : 0.f) * da;
        if (lead) dz[ah] = da;
    }
    for (int s = lo; s < hi; ++s) {
        const int src = csr_src[s];
        const int64_t ah = (int64_t)csr_eid[s] * H + head;
        float4 xl[YL ? 1 : KC];                  // YL: the x_l row is read again for dy instead of held (64 registers)
        float z = 0.f;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const float4 v = ok[k] ? bld4(xl_base + (int64_t)src * ldj + 4 * (sl + k * LPH)) : make_float4(0.f, 0.f, 0.f, 0.f);
            z += bdot4(v, YL ? ylds[k * 64 + lane] : y[YL ? 0 : k]);
            if (!YL) xl[YL ? 0 : k] = v;
        }
        if (YL) asm volatile("" ::: "memory");     // keeps the second read of the row a load of its own (else 64 registers held)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            if (o < LPH) z += __shfl_xor(z, o, 64);
        float da = lead ? dz[ah] : 0.f;
        da = __shfl(da, hl * LPH, 64);
        const float d = (mine ? alpha[ah] : 0.f) * (da - S) * (z > 0.f ? 1.f : slope);
        if (lead) dz[ah] = d;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            if (YL) {
                if (ok[k]) dy[k] = bfma4(d, bld4(xl_base + (int64_t)src * ldj + 4 * (sl + k * LPH)), dy[k]);
            } else {
                dy[k] = bfma4(d, xl[k], dy[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        if (!ok[k]) continue;
        const int64_t col = hcol + 4 * (sl + k * LPH);
        bst4(dJ + (int64_t)i * lddj + HC + col, bmul4(dy[k], bld4(pc + (int64_t)g * ldpc + col)));
        bst4(rows + (int64_t)i * 2 * HC + col, bmul4(dy[k], bld4(J + (int64_t)i * ldj + HC + col)));
    }
}

// One workgroup per source j over its out-edges (t_*: the CSR of the transposed graph: t_dst = its csr_src, t_eid the COO edge
// id); thread t owns the float4 column chunks t, t + blockDim, ... of the H C columns.  Writes d x_l, d x_val and the right half of
// rows (dv' * x_val).
__global__ __launch_bounds__(512) void k_lcgn_att_bwd_src(int H, int C, int concat, int xg, const float* __restrict__ J, int64_t ldj,
                                                          const float* __restrict__ pc, int64_t ldpc, const float* __restrict__ alpha,
                                                          const float* __restrict__ mask, const float* __restrict__ dout, int64_t ldd,
                                                          const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_dst,
                                                          const int32_t* __restrict__ t_eid, const int32_t* __restrict__ node_graph,
                                                          const float* __restrict__ dz, float* __restrict__ dJ, int64_t lddj,
                                                          float* __restrict__ rows) {
    const int j = blockIdx.x;
    const int HC = H * C, Cq = C >> 2, HCq = HC >> 2;
    const bool mean = !concat && H > 1;
    const float fh = (float)H;
    const int g = node_graph[j];
    const int lo = t_rowptr[j], hi = t_rowptr[j + 1];
    for (int c4 = threadIdx.x; c4 < HCq; c4 += blockDim.x) {
        const int h = c4 / Cq;
        const int64_t col = 4 * (int64_t)c4, gcol = concat ? col : 4 * (int64_t)(c4 - h * Cq);
        float4 al = make_float4(0.f, 0.f, 0.f, 0.f), av = al;
        for (int s = lo; s < hi; ++s) {
            const int d = t_dst[s];
            const int64_t ah = (int64_t)t_eid[s] * H + h;
            const float dzv = dz[ah];
            const float am = mask ? alpha[ah] * mask[ah] : alpha[ah];
            const int gd = xg ? node_graph[d] : g;
            const float4 yv = bmul4(bld4(pc + (int64_t)gd * ldpc + col), bld4(J + (int64_t)d * ldj + HC + col));
            float4 G = bld4(dout + (int64_t)d * ldd + gcol);
            if (mean) G = make_float4(G.x / fh, G.y / fh, G.z / fh, G.w / fh);
            al = bfma4(dzv, yv, al);
            av = bfma4(am, G, av);
        }
        bst4(dJ + (int64_t)j * lddj + col, al);
        bst4(dJ + (int64_t)j * lddj + 2 * HC + col, bmul4(av, bld4(pc + (int64_t)g * ldpc + HC + col)));
        bst4(rows + (int64_t)j * 2 * HC + HC + col, bmul4(av, bld4(J + (int64_t)j * ldj + 2 * HC + col)));
    }
}

// ---- the same two walks on a J stored as bf16 (gvqa_lcgn_attention_bf16_backward) -----------------------------------------------------
// The bf16 forward's lane layout: a lane's 16-byte load of J is 8 channels (a chunk), lane sl of a head owns the chunks sl, sl + LPH, ...
// of its C / 8 (KC <= 8 within H C <= 4096, so y, G and dy always fit the registers: no LDS form).  bf16 -> fp32 is a shift in
// registers; pc, alpha, mask, dout, dz, dJ, rows and every sum are fp32, the formulas and the order of the sums those above.
__device__ __forceinline__ uint4 bld16(const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void bbf8(uint4 r, float (&f)[8]) {
    f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xFFFF0000u);
    f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xFFFF0000u);
    f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xFFFF0000u);
    f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xFFFF0000u);
}
__device__ __forceinline__ void bld8f(const float* p, float (&f)[8]) {
    const float4 a = bld4(p), b = bld4(p + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
__device__ __forceinline__ void bst8f(float* p, const float (&f)[8]) {
    bst4(p, make_float4(f[0], f[1], f[2], f[3]));
    bst4(p + 4, make_float4(f[4], f[5], f[6], f[7]));
}

// KC = 8 is one head of more than 2048 channels (H = 1: one wave per workgroup), so its launch bound is 64 threads.
template <int KC>
__global__ __launch_bounds__(KC == 8 ? 64 : 512) void k_lcgn_att16_bwd_dst(int H, int C, int hpw, int LPH, int concat, int xg, float slope,
                                                          const uint16_t* __restrict__ J, int64_t ldj, const float* __restrict__ pc,
                                                          int64_t ldpc, const float* __restrict__ alpha, const float* __restrict__ mask,
                                                          const float* __restrict__ dout, int64_t ldd, const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ csr_src, const int32_t* __restrict__ csr_eid,
                                                          const int32_t* __restrict__ node_graph, float* dz, float* __restrict__ dJ,
                                                          int64_t lddj, float* __restrict__ rows) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x;
    const int HC = H * C, C8 = C >> 3;
    const bool mean = !concat && H > 1;
    const int hl = lane / LPH, sl = lane - hl * LPH;
    const bool mine = hl < hpw;                  // this lane serves a head
    const bool lead = sl == 0 && mine;
    const int head = wave * hpw + hl;
    const int64_t hcol = (int64_t)head * C;
    const int g = node_graph[i];
    const float fh = (float)H;
    bool ok[KC];
    float y[KC][8], gr[KC][8], dy[KC][8];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int q = sl + k * LPH;
        ok[k] = mine && q < C8;
#pragma unroll
        for (int j = 0; j < 8; ++j) y[k][j] = gr[k][j] = dy[k][j] = 0.f;
        if (ok[k]) {
            float a[8], b[8];
            bld8f(pc + (int64_t)g * ldpc + hcol + 8 * q, a);
            bbf8(bld16(J + (int64_t)i * ldj + HC + hcol + 8 * q), b);
            bld8f(dout + (int64_t)i * ldd + (concat ? hcol : 0) + 8 * q, gr[k]);
#pragma unroll
            for (int j = 0; j < 8; ++j) y[k][j] = a[j] * b[j];
            if (mean) {
#pragma unroll
                for (int j = 0; j < 8; ++j) gr[k][j] /= fh;
            }
            if (!xg) {                           // every source shares the destination's cal_cmd row
                bld8f(pc + (int64_t)g * ldpc + HC + hcol + 8 * q, a);
#pragma unroll
                for (int j = 0; j < 8; ++j) gr[k][j] *= a[j];
            }
        }
    }
    const uint16_t* xl_base = J + hcol;
    const uint16_t* xv_base = J + 2 * (int64_t)HC + hcol;
    const float* cc_base = pc + HC + hcol;
    const int lo = rowptr[i], hi = rowptr[i + 1];
    float S = 0.f;                               // sum over the in-edges of alpha * da
    for (int s = lo; s < hi; ++s) {
        const int src = csr_src[s];
        const int64_t ah = (int64_t)csr_eid[s] * H + head;
        const int gs = xg ? node_graph[src] : 0;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            if (!ok[k]) continue;
            const int64_t off = 8 * (int64_t)(sl + k * LPH);
            float xv[8];
            bbf8(bld16(xv_base + (int64_t)src * ldj + off), xv);
            if (xg) {
                float c[8];
                bld8f(cc_base + (int64_t)gs * ldpc + off, c);
#pragma unroll
                for (int j = 0; j < 8; ++j) xv[j] *= c[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) v += xv[j] * gr[k][j];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            if (o < LPH) v += __shfl_xor(v, o, 64);
        const float da = mask && mine ? mask[ah] * v : v;
        S += (mine ? alpha[ah] : 0.f) * da;
        if (lead) dz[ah] = da;
    }
    for (int s = lo; s < hi; ++s) {
        const int src = csr_src[s];
        const int64_t ah = (int64_t)csr_eid[s] * H + head;
        uint4 xl[KC];
        float z = 0.f;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            xl[k] = ok[k] ? bld16(xl_base + (int64_t)src * ldj + 8 * (sl + k * LPH)) : make_uint4(0u, 0u, 0u, 0u);
            float f[8];
            bbf8(xl[k], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) z += f[j] * y[k][j];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            if (o < LPH) z += __shfl_xor(z, o, 64);
        float da = lead ? dz[ah] : 0.f;
        da = __shfl(da, hl * LPH, 64);
        const float d = (mine ? alpha[ah] : 0.f) * (da - S) * (z > 0.f ? 1.f : slope);
        if (lead) dz[ah] = d;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            float f[8];
            bbf8(xl[k], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) dy[k][j] += d * f[j];
        }
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        if (!ok[k]) continue;
        const int64_t col = hcol + 8 * (sl + k * LPH);
        float a[8], b[8], r[8];
        bld8f(pc + (int64_t)g * ldpc + col, a);
        bbf8(bld16(J + (int64_t)i * ldj + HC + col), b);
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = dy[k][j] * a[j];
        bst8f(dJ + (int64_t)i * lddj + HC + col, r);
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = dy[k][j] * b[j];
        bst8f(rows + (int64_t)i * 2 * HC + col, r);
    }
}

// k_lcgn_att_bwd_src on a bf16 J: thread t owns the 8-channel chunks t, t + blockDim, ... of the H C columns.
__global__ __launch_bounds__(512) void k_lcgn_att16_bwd_src(int H, int C, int concat, int xg, const uint16_t* __restrict__ J, int64_t ldj,
                                                            const float* __restrict__ pc, int64_t ldpc, const float* __restrict__ alpha,
                                                            const float* __restrict__ mask, const float* __restrict__ dout, int64_t ldd,
                                                            const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_dst,
                                                            const int32_t* __restrict__ t_eid, const int32_t* __restrict__ node_graph,
                                                            const float* __restrict__ dz, float* __restrict__ dJ, int64_t lddj,
                                                            float* __restrict__ rows) {
    const int j = blockIdx.x;
    const int HC = H * C, C8 = C >> 3, HC8 = HC >> 3;
    const bool mean = !concat && H > 1;
    const float fh = (float)H;
    const int g = node_graph[j];
    const int lo = t_rowptr[j], hi = t_rowptr[j + 1];
    for (int c8 = threadIdx.x; c8 < HC8; c8 += blockDim.x) {
        const int h = c8 / C8;
        const int64_t col = 8 * (int64_t)c8, gcol = concat ? col : 8 * (int64_t)(c8 - h * C8);
        float al[8], av[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) al[k] = av[k] = 0.f;
        for (int s = lo; s < hi; ++s) {
            const int d = t_dst[s];
            const int64_t ah = (int64_t)t_eid[s] * H + h;
            const float dzv = dz[ah];
            const float am = mask ? alpha[ah] * mask[ah] : alpha[ah];
            const int gd = xg ? node_graph[d] : g;
            float p8[8], xr[8], G[8];
            bld8f(pc + (int64_t)gd * ldpc + col, p8);
            bbf8(bld16(J + (int64_t)d * ldj + HC + col), xr);
            bld8f(dout + (int64_t)d * ldd + gcol, G);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (mean) G[k] /= fh;
                al[k] += dzv * (p8[k] * xr[k]);
                av[k] += am * G[k];
            }
        }
        float c[8], xv[8], r[8];
        bld8f(pc + (int64_t)g * ldpc + HC + col, c);
        bbf8(bld16(J + (int64_t)j * ldj + 2 * HC + col), xv);
        bst8f(dJ + (int64_t)j * lddj + col, al);
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = av[k] * c[k];
        bst8f(dJ + (int64_t)j * lddj + 2 * HC + col, r);
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = av[k] * xv[k];
        bst8f(rows + (int64_t)j * 2 * HC + HC + col, r);
    }
}

struct LcgnBwdLayout {
    size_t dz, rows, total;
};
static LcgnBwdLayout lcgn_bwd_layout(int64_t N, int64_t E, int64_t H, int64_t HC) {
    LcgnBwdLayout L; size_t off = 0;
    auto take = [&](size_t bytes) { size_t r = off; off += align_up(bytes, 256); return r; };
    L.dz = take((size_t)E * H * sizeof(float));
    L.rows = take((size_t)N * 2 * HC * sizeof(float));       // [dy * x_r | dv' * x_val] per node
    L.total = off;
    return L;
}

}  // namespace gvqa

extern "C" {
using namespace gvqa;

int gvqa_lcgn_attention_train(const gvqa_graph* g, int32_t heads, int32_t C, int32_t concat, float negative_slope, const float* J,
                              int64_t ld_J, const float* pc, int64_t ld_pc, const float* bias, const float* mask, float* out,
                              int64_t ld_out, float* alpha_out, void* stream) {
    GVQA_REQUIRE(g, GVQA_E_INVALID, "lcgn_attention_train: null graph");
    int rc = lcgn_heads_limits(heads, C, "lcgn_attention_train");
    if (rc) return rc;
    GVQA_REQUIRE(g->finalized, GVQA_E_INVALID, "lcgn_attention_train: the graph is not finalized");
    const int64_t HC = (int64_t)heads * C, cout = concat ? HC : C;
    GVQA_REQUIRE(ld_J >= 3 * HC && ld_pc >= 2 * HC && ld_out >= cout, GVQA_E_INVALID,
                 "lcgn_attention_train: leading dimensions too small (ld_J %lld < %lld, ld_pc %lld < %lld or ld_out %lld < %lld)",
                 (long long)ld_J, (long long)(3 * HC), (long long)ld_pc, (long long)(2 * HC), (long long)ld_out, (long long)cout);
    if (g->num_nodes == 0) return GVQA_OK;
    GVQA_REQUIRE(J && pc && out, GVQA_E_INVALID, "lcgn_attention_train: null tensor");
    GVQA_REQUIRE(alpha_out || g->num_edges == 0, GVQA_E_INVALID, "lcgn_attention_train: alpha_out is required (the backward reads it)");
    GVQA_REQUIRE(ld_J % 4 == 0 && ld_pc % 4 == 0 && ld_out % 4 == 0 && aligned16(J) && aligned16(pc) && aligned16(out),
                 GVQA_E_UNSUPPORTED, "lcgn_attention_train: rows must be 16-byte aligned (pointers and leading dimensions)");
    return launch_lcgn_attention(g, heads, C, concat, negative_slope, J, ld_J, pc, ld_pc, bias, out, ld_out, alpha_out, true, mask,
                                 static_cast<hipStream_t>(stream));
}

size_t gvqa_lcgn_attention_backward_workspace_bytes(const gvqa_graph* g, int32_t heads, int32_t C) {
    if (!g || lcgn_heads_limits(heads, C, "lcgn_attention_backward") != GVQA_OK) return 0;
    return lcgn_bwd_layout(g->num_nodes, g->num_edges, heads, (int64_t)heads * C).total;
}

int gvqa_lcgn_attention_backward(const gvqa_graph* g, const gvqa_graph* gt, int32_t heads, int32_t C, int32_t concat,
                                 float negative_slope, const float* J, int64_t ld_J, const float* pc, int64_t ld_pc, const float* alpha,
                                 const float* mask, const float* dout, int64_t ld_dout, float* dJ, int64_t ld_dJ, float* dpc,
                                 int64_t ld_dpc, void* ws, size_t ws_bytes, void* stream_) {
    GVQA_REQUIRE(g && gt, GVQA_E_INVALID, "lcgn_attention_backward: null graph");
    int rc = lcgn_heads_limits(heads, C, "lcgn_attention_backward");
    if (rc) return rc;
    GVQA_REQUIRE(g->finalized && gt->finalized, GVQA_E_INVALID, "lcgn_attention_backward: the graph is not finalized");
    GVQA_REQUIRE(g->num_nodes == gt->num_nodes && g->num_edges == gt->num_edges && g->num_graphs == gt->num_graphs, GVQA_E_INVALID,
                 "lcgn_attention_backward: the transposed graph must be built from the flipped edge_index of the same batch "
                 "(nodes %lld / %lld, edges %lld / %lld)", (long long)g->num_nodes, (long long)gt->num_nodes, (long long)g->num_edges,
                 (long long)gt->num_edges);
    const int64_t N = g->num_nodes, E = g->num_edges, B = g->num_graphs, HC = (int64_t)heads * C, cout = concat ? HC : C;
    GVQA_REQUIRE(ld_J >= 3 * HC && ld_dJ >= 3 * HC && ld_pc >= 2 * HC && ld_dpc >= 2 * HC && ld_dout >= cout, GVQA_E_INVALID,
                 "lcgn_attention_backward: leading dimensions too small (ld_J %lld, ld_dJ %lld < %lld, ld_pc %lld, ld_dpc %lld < %lld or "
                 "ld_dout %lld < %lld)", (long long)ld_J, (long long)ld_dJ, (long long)(3 * HC), (long long)ld_pc, (long long)ld_dpc,
                 (long long)(2 * HC), (long long)ld_dout, (long long)cout);
    const LcgnBwdLayout L = lcgn_bwd_layout(N, E, heads, HC);
    GVQA_REQUIRE(ws_bytes >= L.total && (ws || L.total == 0), GVQA_E_WORKSPACE, "lcgn_attention_backward: workspace %zu < required %zu",
                 ws_bytes, L.total);
    if (B == 0) return GVQA_OK;
    GVQA_REQUIRE(dpc, GVQA_E_INVALID, "lcgn_attention_backward: null dpc");
    GVQA_REQUIRE(N == 0 || (J && pc && dout && dJ), GVQA_E_INVALID, "lcgn_attention_backward: null tensor");
    GVQA_REQUIRE(E == 0 || alpha, GVQA_E_INVALID, "lcgn_attention_backward: null alpha");
    GVQA_REQUIRE(ld_J % 4 == 0 && ld_pc % 4 == 0 && ld_dout % 4 == 0 && ld_dJ % 4 == 0 && aligned16(J) && aligned16(pc) &&
                     aligned16(dout) && aligned16(dJ),
                 GVQA_E_UNSUPPORTED, "lcgn_attention_backward: rows must be 16-byte aligned (pointers and leading dimensions)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    char* base = static_cast<char*>(ws);
    float* dz = reinterpret_cast<float*>(base + L.dz);
    float* rows = reinterpret_cast<float*>(base + L.rows);
    if (N > 0) {
        const bool one_wave = HC <= LCGN_BWD_ONE_WAVE_HC;
        const int waves = one_wave ? 1 : heads, hpw = one_wave ? heads : 1;
        int LPH = 64;
        while (LPH * hpw > 64) LPH >>= 1;
        const int need = (int)cdiv(C / 4, LPH);
        const int KC = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : 16;
        const int xg = !g->intra_graph;
        const size_t lds = KC == 16 ? (size_t)waves * 2 * 64 * KC * sizeof(float4) : 0;
        const dim3 grid((unsigned)N), block((unsigned)(64 * waves));
#define LCGN_BWD_DST(KC_)                                                                                                           \
    hipLaunchKernelGGL((k_lcgn_att_bwd_dst<KC_, (KC_ >= 16)>), grid, block, lds, stream, heads, C, hpw, LPH, concat, xg, negative_slope, \
                       J, ld_J, pc, ld_pc, alpha, mask, dout, ld_dout, g->rowptr, g->csr_src, g->csr_eid, g->node_graph, dz, dJ, ld_dJ,   \
                       rows)
        switch (KC) {
            case 1: LCGN_BWD_DST(1); break;
            case 2: LCGN_BWD_DST(2); break;
            case 4: LCGN_BWD_DST(4); break;
            case 8: LCGN_BWD_DST(8); break;
            default: LCGN_BWD_DST(16); break;
        }
#undef LCGN_BWD_DST
        GVQA_LAUNCH_CHECK();
        const int threads = (int)std::min<int64_t>(512, align_up((size_t)(HC / 4), 64));
        hipLaunchKernelGGL(k_lcgn_att_bwd_src, grid, dim3((unsigned)threads), 0, stream, heads, C, concat, xg, J, ld_J, pc, ld_pc, alpha,
                           mask, dout, ld_dout, gt->rowptr, gt->csr_src, gt->csr_eid, g->node_graph, dz, dJ, ld_dJ, rows);
        GVQA_LAUNCH_CHECK();
    }
    // dpc[b] = sum over the nodes of graph b of [dy * x_r | dv' * x_val] (a graph without nodes: a zero row)
    return gvqa_graph_segment_sum(g, 2 * HC, rows, 2 * HC, dpc, ld_dpc, stream_);
}

size_t gvqa_lcgn_attention_bf16_backward_workspace_bytes(const gvqa_graph* g, int32_t heads, int32_t C) {
    if (!g || lcgn_heads_limits(heads, C, "lcgn_attention_bf16_backward") != GVQA_OK || C % 8 != 0) return 0;
    return lcgn_bwd_layout(g->num_nodes, g->num_edges, heads, (int64_t)heads * C).total;
}

int gvqa_lcgn_attention_bf16_backward(const gvqa_graph* g, const gvqa_graph* gt, int32_t heads, int32_t C, int32_t concat,
                                      float negative_slope, const void* J_, int64_t ld_J, const float* pc, int64_t ld_pc,
                                      const float* alpha, const float* mask, const float* dout, int64_t ld_dout, float* dJ, int64_t ld_dJ,
                                      float* dpc, int64_t ld_dpc, void* ws, size_t ws_bytes, void* stream_) {
    GVQA_REQUIRE(g && gt, GVQA_E_INVALID, "lcgn_attention_bf16_backward: null graph");
    int rc = lcgn_heads_limits(heads, C, "lcgn_attention_bf16_backward");
    if (rc) return rc;
    GVQA_REQUIRE(C % 8 == 0, GVQA_E_UNSUPPORTED, "lcgn_attention_bf16_backward: C = %d must be a multiple of 8", C);
    GVQA_REQUIRE(g->finalized && gt->finalized, GVQA_E_INVALID, "lcgn_attention_bf16_backward: the graph is not finalized");
    GVQA_REQUIRE(g->num_nodes == gt->num_nodes && g->num_edges == gt->num_edges && g->num_graphs == gt->num_graphs, GVQA_E_INVALID,
                 "lcgn_attention_bf16_backward: the transposed graph must be built from the flipped edge_index of the same batch "
                 "(nodes %lld / %lld, edges %lld / %lld)", (long long)g->num_nodes, (long long)gt->num_nodes, (long long)g->num_edges,
                 (long long)gt->num_edges);
    const int64_t N = g->num_nodes, E = g->num_edges, B = g->num_graphs, HC = (int64_t)heads * C, cout = concat ? HC : C;
    GVQA_REQUIRE(ld_J >= 3 * HC && ld_dJ >= 3 * HC && ld_pc >= 2 * HC && ld_dpc >= 2 * HC && ld_dout >= cout, GVQA_E_INVALID,
                 "lcgn_attention_bf16_backward: leading dimensions too small (ld_J %lld, ld_dJ %lld < %lld, ld_pc %lld, ld_dpc %lld < %lld "
                 "or ld_dout %lld < %lld)", (long long)ld_J, (long long)ld_dJ, (long long)(3 * HC), (long long)ld_pc, (long long)ld_dpc,
                 (long long)(2 * HC), (long long)ld_dout, (long long)cout);
    const LcgnBwdLayout L = lcgn_bwd_layout(N, E, heads, HC);
    GVQA_REQUIRE(ws_bytes >= L.total && (ws || L.total == 0), GVQA_E_WORKSPACE,
                 "lcgn_attention_bf16_backward: workspace %zu < required %zu", ws_bytes, L.total);
    if (B == 0) return GVQA_OK;
    GVQA_REQUIRE(dpc, GVQA_E_INVALID, "lcgn_attention_bf16_backward: null dpc");
    GVQA_REQUIRE(N == 0 || (J_ && pc && dout && dJ), GVQA_E_INVALID, "lcgn_attention_bf16_backward: null tensor");
    GVQA_REQUIRE(E == 0 || alpha, GVQA_E_INVALID, "lcgn_attention_bf16_backward: null alpha");
    GVQA_REQUIRE(ld_J % 8 == 0 && ld_pc % 4 == 0 && ld_dout % 4 == 0 && ld_dJ % 4 == 0 && aligned16(J_) && aligned16(pc) &&
                     aligned16(dout) && aligned16(dJ),
                 GVQA_E_UNSUPPORTED, "lcgn_attention_bf16_backward: rows must be 16-byte aligned (pointers and leading dimensions)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const uint16_t* J = static_cast<const uint16_t*>(J_);
    char* base = static_cast<char*>(ws);
    float* dz = reinterpret_cast<float*>(base + L.dz);
    float* rows = reinterpret_cast<float*>(base + L.rows);
    if (N > 0) {
        const bool one_wave = HC <= LCGN_BWD_ONE_WAVE_HC;
        const int waves = one_wave ? 1 : heads, hpw = one_wave ? heads : 1;
        int LPH = 64;
        while (LPH * hpw > 64) LPH >>= 1;
        const int need = (int)cdiv(C / 8, LPH);              // 8-channel chunks per lane
        GVQA_REQUIRE(need <= 8, GVQA_E_UNSUPPORTED, "lcgn_attention_bf16_backward: %d chunks per lane (H %d, C %d)", need, heads, C);
        const int KC = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : 8;
        GVQA_REQUIRE(KC < 8 || waves == 1, GVQA_E_UNSUPPORTED, "lcgn_attention_bf16_backward: 8 chunks per lane need one wave (H %d, C %d)",
                     heads, C);
        const int xg = !g->intra_graph;
        const dim3 grid((unsigned)N), block((unsigned)(64 * waves));
#define LCGN_BWD16_DST(KC_)                                                                                                          \
    hipLaunchKernelGGL((k_lcgn_att16_bwd_dst<KC_>), grid, block, 0, stream, heads, C, hpw, LPH, concat, xg, negative_slope, J, ld_J, pc,  \
                       ld_pc, alpha, mask, dout, ld_dout, g->rowptr, g->csr_src, g->csr_eid, g->node_graph, dz, dJ, ld_dJ, rows)
        switch (KC) {
            case 1: LCGN_BWD16_DST(1); break;
            case 2: LCGN_BWD16_DST(2); break;
            case 4: LCGN_BWD16_DST(4); break;
            default: LCGN_BWD16_DST(8); break;
        }
#undef LCGN_BWD16_DST
        GVQA_LAUNCH_CHECK();
        const int threads = (int)std::min<int64_t>(512, align_up((size_t)(HC / 8), 64));
        hipLaunchKernelGGL(k_lcgn_att16_bwd_src, grid, dim3((unsigned)threads), 0, stream, heads, C, concat, xg, J, ld_J, pc, ld_pc, alpha,
                           mask, dout, ld_dout, gt->rowptr, gt->csr_src, gt->csr_eid, g->node_graph, dz, dJ, ld_dJ, rows);
        GVQA_LAUNCH_CHECK();
    }
    return gvqa_graph_segment_sum(g, 2 * HC, rows, 2 * HC, dpc, ld_dpc, stream_);
}

}  // extern "C"
