// gat_lcgn for any number of heads (gfx950): attention + aggregation in one launch, and the stand-alone layer.
//
// Reference: baseline_and_test_models/lcgn.py:120-238 (gat_lcgn.forward / message).  lcgn.hip keeps lcgn_seq's gat_heads = 1
// pipeline (edge-logit kernel + the GAT message-passing kernel); this file serves H = 1 .. 8 heads of width C:
//   logit[e,h] = x_l[src,h,:] . (proj_cmd[g(dst),h,:] * x_r[dst,h,:])             lcgn.py:144-154,207
//   alpha      = softmax over the destination's in-edges of leaky_relu(logit)     :208-211 (max-shifted, + 1e-16)
//   out[i]     = sum_e alpha[e,h] x_val[src,h,:] * cal_cmd[g(src),h,:]            :230-238
// with the heads side by side (concat) or averaged, + bias (:181-189).
//
// One workgroup per destination node.  H * C <= 1024: one wave holds every head; otherwise one wave per head, so that every
// head's dot product reduces inside one wave.  The destination's y = proj_cmd * x_r stays in registers; the in-edges are walked
// in CSR order (= COO order within a row: deterministic, no atomics) with an online softmax per head (running max and
// denominator, the accumulators rescaled when the max moves), 16 bytes per lane and up to two edges' x_l rows in flight.
#include "common.h"

namespace gvqa {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

constexpr int LCGN_ATT_MAX_HEADS = 8, LCGN_ATT_MAX_HC = 4096, LCGN_ATT_ONE_WAVE_HC = 1024;

// Lane layout: the wave's hpw heads sit in aligned segments of LPH lanes (a power of two, 64 / LPH >= hpw); lane sl of head hl owns
// the float4 chunks sl, sl + LPH, sl + 2 LPH, ... of that head (KC of them at most), so every lane serves one head, a head's dot
// product is a butterfly over its own segment, and the softmax state (running max, denominator) is one pair of registers per lane.
// XG: the batch has edges across graphs -> cal_cmd of the SOURCE's graph per edge (else the destination's, once at the end).
// YL: y lives in LDS instead of registers (KC = 16: one head of more than 2048 channels).
// J [N, ldj] = [x_l | x_r | x_val] (H C columns each), pc [B, ldpc] = [proj_cmd | cal_cmd] (H C each).  alpha (optional) [E, H]:
// the walk leaves the leaky-relu'd logits there (lane 0 of a head's segment writes that head), the same lane normalises them after
// the walk.  TR: the training forward (gvqa_lcgn_attention_train) -- alpha is required, mask (optional) [E, H] in COO order
// multiplies the weight of a message after the softmax (attention dropout, lcgn.py:212), never the denominator.  Dynamic LDS: H C floats when the heads are averaged (concat == 0, H > 1), + 64 KC float4 per wave with YL.
template <int KC, bool XG, bool YL, bool TR>
__global__ __launch_bounds__(512) void k_lcgn_attention(int H, int C, int hpw, int LPH, int concat, float slope, const float* __restrict__ J,
                                                        int64_t ldj, const float* __restrict__ pc, int64_t ldpc, const float* __restrict__ bias,
                                                        const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr_src,
                                                        const int32_t* __restrict__ csr_eid, const int32_t* __restrict__ node_graph,
                                                        float* __restrict__ out, int64_t ldo, float* __restrict__ alpha,
                                                        const float* __restrict__ mask) {
    extern __shared__ float4 lcgn_lds[];
    constexpr int NE = KC <= 4 ? 2 : 1;          // edges in flight (register budget)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x;
    const int HC = H * C, Cq = C >> 2;
    const bool mean = !concat && H > 1;
    const int hl = lane / LPH, sl = lane - hl * LPH;
    const bool lead = sl == 0 && hl < hpw;       // the lane that writes / normalises this head's alpha
    const int head = wave * hpw + hl;            // (>= H on lanes past the wave's heads)
    const int64_t hcol = (int64_t)head * C;
    const int g = node_graph[i];
    float4* ylds = lcgn_lds + (mean ? HC / 4 : 0) + wave * 64 * KC;
    bool ok[KC];
    float4 y[YL ? 1 : KC], acc[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int q = sl + k * LPH;
        ok[k] = hl < hpw && q < Cq;
        acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 yk = acc[k];
        if (ok[k]) {
            const float4 a = ld4(pc + (int64_t)g * ldpc + hcol + 4 * q), b = ld4(J + (int64_t)i * ldj + HC + hcol + 4 * q);
            yk = make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
        }
        if (YL) ylds[k * 64 + lane] = yk;
        else y[YL ? 0 : k] = yk;
    }
    const float* xl_base = J + hcol;
    const float* xv_base = J + 2 * (int64_t)HC + hcol;
    const float* cc_base = pc + HC + hcol;
    float m = -INFINITY, den = 0.f;
    const int lo = rowptr[i], hi = rowptr[i + 1];
    for (int s = lo; s < hi; s += NE) {
        const int ne = min(NE, hi - s);
        int src[NE];
        float4 xl[NE][KC];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            src[e] = e < ne ? csr_src[s + e] : 0;
#pragma unroll
            for (int k = 0; k < KC; ++k)
                xl[e][k] = e < ne && ok[k] ? ld4(xl_base + (int64_t)src[e] * ldj + 4 * (sl + k * LPH)) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float l[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < KC; ++k) v += dot4(xl[e][k], YL ? ylds[k * 64 + lane] : y[YL ? 0 : k]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
                if (o < LPH) v += __shfl_xor(v, o, 64);
            l[e] = v > 0.f ? v : v * slope;                                      // leaky_relu (lcgn.py:209)
        }
        // YL (64 float4 per lane and row): x_val's loads stay behind the dot product, whose x_l registers they reuse
        if (YL) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            if (e >= ne) break;
            const float mn = fmaxf(m, l[e]);
            const float sc = expf(m - mn), p = expf(l[e] - mn);
            den = den * sc + p;
            m = mn;
            const int64_t ah = TR ? (int64_t)csr_eid[s + e] * H + head : 0;
            if (TR) {
                if (lead) alpha[ah] = l[e];
            } else if (alpha && lead) {
                alpha[(int64_t)csr_eid[s + e] * H + head] = l[e];
            }
            const float w = TR && mask && hl < hpw ? p * mask[ah] : p;          // dropout scales the message, not the softmax
            const int gs = XG ? node_graph[src[e]] : 0;
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                if (!ok[k]) continue;
                const int64_t off = 4 * (int64_t)(sl + k * LPH);
                float4 v = ld4(xv_base + (int64_t)src[e] * ldj + off);
                if (XG) {
                    const float4 c = ld4(cc_base + (int64_t)gs * ldpc + off);
                    v = make_float4(v.x * c.x, v.y * c.y, v.z * c.z, v.w * c.w);
                }
                acc[k] = make_float4(acc[k].x * sc + w * v.x, acc[k].y * sc + w * v.y, acc[k].z * sc + w * v.z, acc[k].w * sc + w * v.w);
            }
        }
    }
    const float d = den + 1e-16f;                // a node without in-edges: 0 / 1e-16 = 0
    if (alpha && lead) {                         // the stored logits of this node's in-edges -> softmax weights (one destination per edge)
        for (int s = lo; s < hi; ++s) {
            const int64_t a = (int64_t)csr_eid[s] * H + head;
            alpha[a] = expf(alpha[a] - m) / d;
        }
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        if (!ok[k]) continue;
        const int q = sl + k * LPH;
        float4 r = make_float4(acc[k].x / d, acc[k].y / d, acc[k].z / d, acc[k].w / d);
        if (!XG) {          // every in-edge comes from the destination's graph: cal_cmd factors out of the sum
            const float4 c = ld4(cc_base + (int64_t)g * ldpc + 4 * q);
            r = make_float4(r.x * c.x, r.y * c.y, r.z * c.z, r.w * c.w);
        }
        if (mean) {
            lcgn_lds[head * Cq + q] = r;
        } else {
            if (bias) {
                const float* b = bias + hcol + 4 * q;
                r = make_float4(r.x + b[0], r.y + b[1], r.z + b[2], r.w + b[3]);
            }
            *reinterpret_cast<float4*>(out + (int64_t)i * ldo + hcol + 4 * q) = r;
        }
    }
    if (mean) {           // the heads' mean (lcgn.py:186), + bias
        __syncthreads();
        for (int c4 = threadIdx.x; c4 < Cq; c4 += blockDim.x) {
            float4 r = lcgn_lds[c4];
            for (int h = 1; h < H; ++h) {
                const float4 v = lcgn_lds[h * Cq + c4];
                r = make_float4(r.x + v.x, r.y + v.y, r.z + v.z, r.w + v.w);
            }
            const float fh = (float)H;
            r = make_float4(r.x / fh, r.y / fh, r.z / fh, r.w / fh);
            if (bias) {
                const float* b = bias + 4 * c4;
                r = make_float4(r.x + b[0], r.y + b[1], r.z + b[2], r.w + b[3]);
            }
            *reinterpret_cast<float4*>(out + (int64_t)i * ldo + 4 * c4) = r;
        }
    }
}


// argument checks shared by the entry points (lcgn_layer_bwd.hip too): limits -> GVQA_E_UNSUPPORTED (nothing enqueued)
int lcgn_heads_limits(int32_t heads, int32_t C, const char* who) {
    GVQA_REQUIRE(heads >= 1 && heads <= LCGN_ATT_MAX_HEADS, GVQA_E_UNSUPPORTED, "%s: heads = %d outside 1 .. %d", who, heads,
                 LCGN_ATT_MAX_HEADS);
    GVQA_REQUIRE(C > 0 && C % 4 == 0, GVQA_E_UNSUPPORTED, "%s: C = %d must be a positive multiple of 4", who, C);
    GVQA_REQUIRE((int64_t)heads * C <= LCGN_ATT_MAX_HC, GVQA_E_UNSUPPORTED, "%s: heads * C = %lld > %d", who,
                 (long long)heads * C, LCGN_ATT_MAX_HC);
    return GVQA_OK;
}

// train: the training forward (alpha required, mask NULL or [E, H]); else the inference form (alpha optional, no mask)
int launch_lcgn_attention(const gvqa_graph* g, int H, int C, int concat, float slope, const float* J, int64_t ldj, const float* pc,
                          int64_t ldpc, const float* bias, float* out, int64_t ldo, float* alpha, bool train, const float* mask,
                          hipStream_t stream) {
    const int64_t N = g->num_nodes;
    if (N == 0) return GVQA_OK;
    const int HC = H * C, Cq = C / 4;
    const bool one_wave = HC <= LCGN_ATT_ONE_WAVE_HC;
    const int waves = one_wave ? 1 : H, hpw = one_wave ? H : 1;
    int LPH = 64;
    while (LPH * hpw > 64) LPH >>= 1;                    // lanes per head: 64 / pow2ceil(heads of the wave)
    const int need = (int)cdiv(Cq, LPH);                 // float4 chunks per lane
    const int KC = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : 16;
    const bool xg = !g->intra_graph;
    const bool mean = !concat && H > 1;
    const size_t lds = (mean ? (size_t)HC * sizeof(float) : 0) + (KC == 16 ? (size_t)waves * 64 * KC * 16 : 0);
    const dim3 grid((unsigned)N), block((unsigned)(64 * waves));
#define LCGN_ATT(KC_, XG_, TR_)                                                                                                   \
    hipLaunchKernelGGL((k_lcgn_attention<KC_, XG_, (KC_ >= 16), TR_>), grid, block, lds, stream, H, C, hpw, LPH, concat, slope, J, ldj, \
                       pc, ldpc, bias, g->rowptr, g->csr_src, g->csr_eid, g->node_graph, out, ldo, alpha, mask)
#define LCGN_ATT_TR(KC_, XG_) do { if (train) LCGN_ATT(KC_, XG_, true); else LCGN_ATT(KC_, XG_, false); } while (0)
#define LCGN_ATT_XG(KC_) do { if (xg) LCGN_ATT_TR(KC_, true); else LCGN_ATT_TR(KC_, false); } while (0)
    switch (KC) {
        case 1: LCGN_ATT_XG(1); break;
        case 2: LCGN_ATT_XG(2); break;
        case 4: LCGN_ATT_XG(4); break;
        case 8: LCGN_ATT_XG(8); break;
        default: LCGN_ATT_XG(16); break;
    }
#undef LCGN_ATT_XG
#undef LCGN_ATT_TR
#undef LCGN_ATT
    GVQA_LAUNCH_CHECK();
    return GVQA_OK;
}

// ---- bf16 storage of the node tensors (lcgn_seq's node_feature_dtype = bfloat16 with gat_heads > 1) -----------------------------------
// k_lcgn_attention's inference form on a bf16 J: the same workgroup per destination, lane segments per head, segmented butterfly and
// online softmax in CSR order, but a lane's 16-byte load is 8 channels (a "chunk"), so lane sl of a head owns the chunks sl, sl + LPH,
// ... of its C / 8.  Within H C <= 4096 a lane holds at most 8 chunks (one wave: C / 8 <= 128 / H over 64 / pow2ceil(H) lanes -> 4;
// one wave per head: C / 8 <= 512 over 64 lanes -> 8), so y always fits the registers and there is no LDS form.  bf16 -> fp32 is a
// shift in registers; logits, softmax, accumulation, pc and bias are fp32.  O16: out is bf16 (rounded to nearest even after the
// head mean and the bias), else fp32.  Dynamic LDS: H C floats when the heads are averaged.
__device__ __forceinline__ uint4 ld16(const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void bf16x8_to_f32(uint4 r, float (&f)[8]) {
    f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xFFFF0000u);
    f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xFFFF0000u);
    f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xFFFF0000u);
    f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xFFFF0000u);
}
__device__ __forceinline__ void ld8f(const float* p, float (&f)[8]) {
    const float4 a = ld4(p), b = ld4(p + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) { return (unsigned)f32_to_bf16(lo) | ((unsigned)f32_to_bf16(hi) << 16); }

// The body of both bf16 kernels.  TR: the training forward with a mask (gvqa_lcgn_attention_bf16_train) -- alpha and mask are
// required, mask [E, H] in COO order multiplies the weight of a message after the softmax, never the denominator.  (Without a mask
// the training forward IS the inference form with fp32 out and alpha: the launcher sends it there, so the two are bit-identical
// whatever contraction the compiler picks for either instantiation.)
template <int KC, bool XG, bool O16, bool TR>
__device__ __forceinline__ void lcgn_att16_body(int H, int C, int hpw, int LPH, int concat, float slope, const uint16_t* __restrict__ J,
                                                int64_t ldj, const float* __restrict__ pc, int64_t ldpc, const float* __restrict__ bias,
                                                const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr_src,
                                                const int32_t* __restrict__ csr_eid, const int32_t* __restrict__ node_graph,
                                                void* __restrict__ out, int64_t ldo, float* __restrict__ alpha,
                                                const float* __restrict__ mask) {
    extern __shared__ float4 lcgn16_lds[];
    constexpr int NE = KC == 1 ? 4 : KC <= 4 ? 2 : 1;      // edges in flight (register budget)
    constexpr bool PV = KC <= 4;                          // x_val's rows are requested together with x_l's
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x;
    const int HC = H * C, C8 = C >> 3, Cq = C >> 2;
    const bool mean = !concat && H > 1;
    const int hl = lane / LPH, sl = lane - hl * LPH;
    const bool lead = sl == 0 && hl < hpw;
    const int head = wave * hpw + hl;
    const int64_t hcol = (int64_t)head * C;
    const int g = node_graph[i];
    bool ok[KC];
    float y[KC][8], acc[KC][8];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int q = sl + k * LPH;
        ok[k] = hl < hpw && q < C8;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] = y[k][j] = 0.f;
        if (ok[k]) {
            float a[8], b[8];
            ld8f(pc + (int64_t)g * ldpc + hcol + 8 * q, a);
            bf16x8_to_f32(ld16(J + (int64_t)i * ldj + HC + hcol + 8 * q), b);
#pragma unroll
            for (int j = 0; j < 8; ++j) y[k][j] = a[j] * b[j];
        }
    }
    const uint16_t* xl_base = J + hcol;
    const uint16_t* xv_base = J + 2 * (int64_t)HC + hcol;
    const float* cc_base = pc + HC + hcol;
    float m = -INFINITY, den = 0.f;
    const int lo = rowptr[i], hi = rowptr[i + 1];
    for (int s = lo; s < hi; s += NE) {
        const int ne = min(NE, hi - s);
        int src[NE];
        uint4 xl[NE][KC], xv[PV ? NE : 1][KC];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            src[e] = e < ne ? csr_src[s + e] : 0;
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const bool on = e < ne && ok[k];
                const int64_t off = (int64_t)src[e] * ldj + 8 * (sl + k * LPH);
                xl[e][k] = on ? ld16(xl_base + off) : make_uint4(0u, 0u, 0u, 0u);
                if (PV) xv[e][k] = on ? ld16(xv_base + off) : make_uint4(0u, 0u, 0u, 0u);
            }
        }
        float l[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                float f[8];
                bf16x8_to_f32(xl[e][k], f);
#pragma unroll
                for (int j = 0; j < 8; ++j) v += f[j] * y[k][j];
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
                if (o < LPH) v += __shfl_xor(v, o, 64);
            l[e] = v > 0.f ? v : v * slope;                                      // leaky_relu (lcgn.py:209)
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            if (e >= ne) break;
            const float mn = fmaxf(m, l[e]);
            const float sc = expf(m - mn), p = expf(l[e] - mn);
            den = den * sc + p;
            m = mn;
            float w = p;
            if (TR) {
                const int64_t ah = (int64_t)csr_eid[s + e] * H + head;
                if (lead) alpha[ah] = l[e];
                if (hl < hpw) w = p * mask[ah];                                  // dropout scales the message, not the softmax
            } else if (alpha && lead) {
                alpha[(int64_t)csr_eid[s + e] * H + head] = l[e];
            }
            const int gs = XG ? node_graph[src[e]] : 0;
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                if (!ok[k]) continue;
                const int64_t off = 8 * (int64_t)(sl + k * LPH);
                float v[8];
                bf16x8_to_f32(PV ? xv[PV ? e : 0][k] : ld16(xv_base + (int64_t)src[e] * ldj + off), v);
                if (XG) {
                    float c[8];
                    ld8f(cc_base + (int64_t)gs * ldpc + off, c);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] *= c[j];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[k][j] = acc[k][j] * sc + w * v[j];
            }
        }
    }
    const float d = den + 1e-16f;                // a node without in-edges: 0 / 1e-16 = 0
    if (alpha && lead) {
        for (int s = lo; s < hi; ++s) {
            const int64_t a = (int64_t)csr_eid[s] * H + head;
            alpha[a] = expf(alpha[a] - m) / d;
        }
    }
    float* lds = reinterpret_cast<float*>(lcgn16_lds);
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        if (!ok[k]) continue;
        const int q = sl + k * LPH;
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = acc[k][j] / d;
        if (!XG) {          // every in-edge comes from the destination's graph: cal_cmd factors out of the sum
            float c[8];
            ld8f(cc_base + (int64_t)g * ldpc + 8 * q, c);
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] *= c[j];
        }
        if (mean) {
            float4* dst = reinterpret_cast<float4*>(lds + hcol + 8 * q);
            dst[0] = make_float4(r[0], r[1], r[2], r[3]);
            dst[1] = make_float4(r[4], r[5], r[6], r[7]);
        } else {
            if (bias) {
                float b[8];
                ld8f(bias + hcol + 8 * q, b);
#pragma unroll
                for (int j = 0; j < 8; ++j) r[j] += b[j];
            }
            const int64_t o = (int64_t)i * ldo + hcol + 8 * q;
            if (O16) {
                *reinterpret_cast<uint4*>(static_cast<uint16_t*>(out) + o) =
                    make_uint4(pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]), pack_bf16x2(r[4], r[5]), pack_bf16x2(r[6], r[7]));
            } else {
                float4* dst = reinterpret_cast<float4*>(static_cast<float*>(out) + o);
                dst[0] = make_float4(r[0], r[1], r[2], r[3]);
                dst[1] = make_float4(r[4], r[5], r[6], r[7]);
            }
        }
    }
    if (mean) {           // the heads' mean (lcgn.py:186), + bias, one rounding
        __syncthreads();
        for (int c4 = threadIdx.x; c4 < Cq; c4 += blockDim.x) {
            float4 r = lcgn16_lds[c4];
            for (int h = 1; h < H; ++h) {
                const float4 v = lcgn16_lds[h * Cq + c4];
                r = make_float4(r.x + v.x, r.y + v.y, r.z + v.z, r.w + v.w);
            }
            const float fh = (float)H;
            r = make_float4(r.x / fh, r.y / fh, r.z / fh, r.w / fh);
            if (bias) {
                const float4 b = ld4(bias + 4 * c4);
                r = make_float4(r.x + b.x, r.y + b.y, r.z + b.z, r.w + b.w);
            }
            const int64_t o = (int64_t)i * ldo + 4 * c4;
            if (O16) *reinterpret_cast<uint2*>(static_cast<uint16_t*>(out) + o) = make_uint2(pack_bf16x2(r.x, r.y), pack_bf16x2(r.z, r.w));
            else *reinterpret_cast<float4*>(static_cast<float*>(out) + o) = r;
        }
    }
}

template <int KC, bool XG, bool O16>
__global__ __launch_bounds__(512) void k_lcgn_attention_bf16(int H, int C, int hpw, int LPH, int concat, float slope,
                                                             const uint16_t* __restrict__ J, int64_t ldj, const float* __restrict__ pc,
                                                             int64_t ldpc, const float* __restrict__ bias,
                                                             const int32_t* __restrict__ rowptr, const int32_t* __restrict__ csr_src,
                                                             const int32_t* __restrict__ csr_eid, const int32_t* __restrict__ node_graph,
                                                             void* __restrict__ out, int64_t ldo, float* __restrict__ alpha) {
    lcgn_att16_body<KC, XG, O16, false>(H, C, hpw, LPH, concat, slope, J, ldj, pc, ldpc, bias, rowptr, csr_src, csr_eid, node_graph, out, ldo,
                                        alpha, nullptr);
}

// The training forward on a bf16 J with a mask: fp32 out, alpha always written.
template <int KC, bool XG>
__global__ __launch_bounds__(512) void k_lcgn_att16_train(int H, int C, int hpw, int LPH, int concat, float slope,
                                                          const uint16_t* __restrict__ J, int64_t ldj, const float* __restrict__ pc,
                                                          int64_t ldpc, const float* __restrict__ bias, const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ csr_src, const int32_t* __restrict__ csr_eid,
                                                          const int32_t* __restrict__ node_graph, float* __restrict__ out, int64_t ldo,
                                                          float* __restrict__ alpha, const float* __restrict__ mask) {
    lcgn_att16_body<KC, XG, false, true>(H, C, hpw, LPH, concat, slope, J, ldj, pc, ldpc, bias, rowptr, csr_src, csr_eid, node_graph, out, ldo,
                                         alpha, mask);
}

// train: gvqa_lcgn_attention_bf16_train (fp32 out, alpha required, mask NULL -- the inference kernel -- or [E, H]); else the inference form
static int launch_lcgn_attention_bf16(const gvqa_graph* g, int H, int C, int concat, float slope, const uint16_t* J, int64_t ldj, const float* pc,
                               int64_t ldpc, const float* bias, void* out, int64_t ldo, bool out16, float* alpha, bool train,
                               const float* mask, hipStream_t stream) {
    const int64_t N = g->num_nodes;
    if (N == 0) return GVQA_OK;
    const int HC = H * C, C8 = C / 8;
    const bool one_wave = HC <= LCGN_ATT_ONE_WAVE_HC;
    const int waves = one_wave ? 1 : H, hpw = one_wave ? H : 1;
    int LPH = 64;
    while (LPH * hpw > 64) LPH >>= 1;
    const int need = (int)cdiv(C8, LPH);                 // 8-channel chunks per lane
    GVQA_REQUIRE(need <= 8, GVQA_E_UNSUPPORTED, "lcgn_attention_bf16: %d chunks per lane (H %d, C %d)", need, H, C);
    const int KC = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : 8;
    const bool xg = !g->intra_graph;
    const size_t lds = !concat && H > 1 ? (size_t)HC * sizeof(float) : 0;
    const dim3 grid((unsigned)N), block((unsigned)(64 * waves));
#define LCGN_ATT16(KC_, XG_, O16_)                                                                                                   \
    hipLaunchKernelGGL((k_lcgn_attention_bf16<KC_, XG_, O16_>), grid, block, lds, stream, H, C, hpw, LPH, concat, slope, J, ldj, pc, ldpc, \
                       bias, g->rowptr, g->csr_src, g->csr_eid, g->node_graph, out, ldo, alpha)
#define LCGN_ATT16_TR(KC_, XG_)                                                                                                       \
    hipLaunchKernelGGL((k_lcgn_att16_train<KC_, XG_>), grid, block, lds, stream, H, C, hpw, LPH, concat, slope, J, ldj, pc, ldpc, bias,     \
                       g->rowptr, g->csr_src, g->csr_eid, g->node_graph, static_cast<float*>(out), ldo, alpha, mask)
#define LCGN_ATT16_O(KC_, XG_)                                                                                                        \
    do {                                                                                                                              \
        if (train && mask) LCGN_ATT16_TR(KC_, XG_);                                                                                   \
        else if (out16) LCGN_ATT16(KC_, XG_, true);                                                                                   \
        else LCGN_ATT16(KC_, XG_, false);                                                                                             \
    } while (0)
#define LCGN_ATT16_XG(KC_) do { if (xg) LCGN_ATT16_O(KC_, true); else LCGN_ATT16_O(KC_, false); } while (0)
    switch (KC) {
        case 1: LCGN_ATT16_XG(1); break;
        case 2: LCGN_ATT16_XG(2); break;
        case 4: LCGN_ATT16_XG(4); break;
        default: LCGN_ATT16_XG(8); break;
    }
#undef LCGN_ATT16_XG
#undef LCGN_ATT16_O
#undef LCGN_ATT16_TR
#undef LCGN_ATT16
    GVQA_LAUNCH_CHECK();
    return GVQA_OK;
}

struct GatLcgnLayout {
    size_t Wst, Wpc, J, pc, scratch, total;
};
static GatLcgnLayout gat_lcgn_layout(int64_t N, int64_t B, int64_t in, int64_t HC, int64_t cmd_dim) {
    GatLcgnLayout L; size_t off = 0;
    auto take = [&](size_t bytes) { size_t r = off; off += align_up(bytes, 256); return r; };
    L.Wst = take((size_t)3 * HC * in * sizeof(float));        // [lin_l; lin_r; cal_x] when the caller's weights are not stacked already
    L.Wpc = take((size_t)2 * HC * cmd_dim * sizeof(float));   // [proj_cmd; cal_cmd] likewise
    L.J = take((size_t)N * 3 * HC * sizeof(float));
    L.pc = take((size_t)B * 2 * HC * sizeof(float));
    L.scratch = take(linear_auto_scratch_bytes(N, 3 * HC, in));
    L.total = off;
    return L;
}

}  // namespace gvqa

extern "C" {
using namespace gvqa;

int gvqa_lcgn_attention(const gvqa_graph* g, int32_t heads, int32_t C, int32_t concat, float negative_slope, const float* J,
                        int64_t ld_J, const float* pc, int64_t ld_pc, const float* bias, float* out, int64_t ld_out, float* alpha_out,
                        void* stream) {
    GVQA_REQUIRE(g, GVQA_E_INVALID, "lcgn_attention: null graph");
    int rc = lcgn_heads_limits(heads, C, "lcgn_attention");
    if (rc) return rc;
    GVQA_REQUIRE(g->finalized, GVQA_E_INVALID, "lcgn_attention: the graph is not finalized");
    const int64_t HC = (int64_t)heads * C, cout = concat ? HC : C;
    GVQA_REQUIRE(ld_J >= 3 * HC && ld_pc >= 2 * HC && ld_out >= cout, GVQA_E_INVALID,
                 "lcgn_attention: leading dimensions too small (ld_J %lld < %lld, ld_pc %lld < %lld or ld_out %lld < %lld)",
                 (long long)ld_J, (long long)(3 * HC), (long long)ld_pc, (long long)(2 * HC), (long long)ld_out, (long long)cout);
    if (g->num_nodes == 0) return GVQA_OK;
    GVQA_REQUIRE(J && pc && out, GVQA_E_INVALID, "lcgn_attention: null tensor");
    GVQA_REQUIRE(ld_J % 4 == 0 && ld_pc % 4 == 0 && ld_out % 4 == 0 && aligned16(J) && aligned16(pc) && aligned16(out),
                 GVQA_E_UNSUPPORTED, "lcgn_attention: rows must be 16-byte aligned (pointers and leading dimensions)");
    return launch_lcgn_attention(g, heads, C, concat, negative_slope, J, ld_J, pc, ld_pc, bias, out, ld_out, alpha_out, false,
                                 nullptr, static_cast<hipStream_t>(stream));
}

int gvqa_lcgn_attention_bf16(const gvqa_graph* g, int32_t heads, int32_t C, int32_t concat, float negative_slope, const void* J,
                             int64_t ld_J, const float* pc, int64_t ld_pc, const float* bias, void* out, int64_t ld_out, int32_t out_bf16,
                             float* alpha_out, void* stream) {
    GVQA_REQUIRE(g, GVQA_E_INVALID, "lcgn_attention_bf16: null graph");
    int rc = lcgn_heads_limits(heads, C, "lcgn_attention_bf16");
    if (rc) return rc;
    GVQA_REQUIRE(C % 8 == 0, GVQA_E_UNSUPPORTED, "lcgn_attention_bf16: C = %d must be a multiple of 8", C);
    GVQA_REQUIRE(g->finalized, GVQA_E_INVALID, "lcgn_attention_bf16: the graph is not finalized");
    const int64_t HC = (int64_t)heads * C, cout = concat ? HC : C;
    GVQA_REQUIRE(ld_J >= 3 * HC && ld_pc >= 2 * HC && ld_out >= cout, GVQA_E_INVALID,
                 "lcgn_attention_bf16: leading dimensions too small (ld_J %lld < %lld, ld_pc %lld < %lld or ld_out %lld < %lld)",
                 (long long)ld_J, (long long)(3 * HC), (long long)ld_pc, (long long)(2 * HC), (long long)ld_out, (long long)cout);
    if (g->num_nodes == 0) return GVQA_OK;
    GVQA_REQUIRE(J && pc && out, GVQA_E_INVALID, "lcgn_attention_bf16: null tensor");
    GVQA_REQUIRE(ld_J % 8 == 0 && ld_pc % 4 == 0 && ld_out % (out_bf16 ? 8 : 4) == 0 && aligned16(J) && aligned16(pc) && aligned16(out) &&
                     aligned16(bias),
                 GVQA_E_UNSUPPORTED, "lcgn_attention_bf16: rows must be 16-byte aligned (pointers and leading dimensions)");
    return launch_lcgn_attention_bf16(g, heads, C, concat, negative_slope, static_cast<const uint16_t*>(J), ld_J, pc, ld_pc, bias, out,
                                      ld_out, out_bf16 != 0, alpha_out, false, nullptr, static_cast<hipStream_t>(stream));
}

int gvqa_lcgn_attention_bf16_train(const gvqa_graph* g, int32_t heads, int32_t C, int32_t concat, float negative_slope, const void* J,
                                   int64_t ld_J, const float* pc, int64_t ld_pc, const float* bias, const float* mask, float* out,
                                   int64_t ld_out, float* alpha_out, void* stream) {
    GVQA_REQUIRE(g, GVQA_E_INVALID, "lcgn_attention_bf16_train: null graph");
    int rc = lcgn_heads_limits(heads, C, "lcgn_attention_bf16_train");
    if (rc) return rc;
    GVQA_REQUIRE(C % 8 == 0, GVQA_E_UNSUPPORTED, "lcgn_attention_bf16_train: C = %d must be a multiple of 8", C);
    GVQA_REQUIRE(g->finalized, GVQA_E_INVALID, "lcgn_attention_bf16_train: the graph is not finalized");
    const int64_t HC = (int64_t)heads * C, cout = concat ? HC : C;
    GVQA_REQUIRE(ld_J >= 3 * HC && ld_pc >= 2 * HC && ld_out >= cout, GVQA_E_INVALID,
                 "lcgn_attention_bf16_train: leading dimensions too small (ld_J %lld < %lld, ld_pc %lld < %lld or ld_out %lld < %lld)",
                 (long long)ld_J, (long long)(3 * HC), (long long)ld_pc, (long long)(2 * HC), (long long)ld_out, (long long)cout);
    if (g->num_nodes == 0) return GVQA_OK;
    GVQA_REQUIRE(J && pc && out, GVQA_E_INVALID, "lcgn_attention_bf16_train: null tensor");
    GVQA_REQUIRE(alpha_out || g->num_edges == 0, GVQA_E_INVALID,
                 "lcgn_attention_bf16_train: alpha_out is required (the backward reads it)");
    GVQA_REQUIRE(ld_J % 8 == 0 && ld_pc % 4 == 0 && ld_out % 4 == 0 && aligned16(J) && aligned16(pc) && aligned16(out) && aligned16(bias),
                 GVQA_E_UNSUPPORTED, "lcgn_attention_bf16_train: rows must be 16-byte aligned (pointers and leading dimensions)");
    return launch_lcgn_attention_bf16(g, heads, C, concat, negative_slope, static_cast<const uint16_t*>(J), ld_J, pc, ld_pc, bias, out,
                                      ld_out, false, alpha_out, true, mask, static_cast<hipStream_t>(stream));
}

size_t gvqa_gat_lcgn_workspace_bytes(const gvqa_graph* g, int32_t in_channels, int32_t C, int32_t heads, int32_t cmd_dim) {
    if (!g || in_channels < 1 || cmd_dim < 1 || lcgn_heads_limits(heads, C, "gat_lcgn") != GVQA_OK) return 0;
    return gat_lcgn_layout(g->num_nodes, g->num_graphs, in_channels, (int64_t)heads * C, cmd_dim).total;
}

int gvqa_gat_lcgn_forward(const gvqa_graph* g, int32_t in_channels, int32_t C, int32_t heads, int32_t cmd_dim, int32_t concat,
                          float negative_slope, const gvqa_lcgn_params* p, const float* x, const float* cmd, float* out,
                          float* alpha_out, void* ws, size_t ws_bytes, void* stream_) {
    GVQA_REQUIRE(g && p, GVQA_E_INVALID, "gat_lcgn: null argument");
    int rc = lcgn_heads_limits(heads, C, "gat_lcgn");
    if (rc) return rc;
    GVQA_REQUIRE(in_channels > 0 && cmd_dim > 0, GVQA_E_INVALID, "gat_lcgn: bad dims (in_channels %d, cmd_dim %d)", in_channels, cmd_dim);
    GVQA_REQUIRE(g->finalized, GVQA_E_INVALID, "gat_lcgn: the graph is not finalized");
    const int64_t N = g->num_nodes, B = g->num_graphs, HC = (int64_t)heads * C, K = in_channels;
    const GatLcgnLayout L = gat_lcgn_layout(N, B, K, HC, cmd_dim);
    GVQA_REQUIRE(ws && ws_bytes >= L.total, GVQA_E_WORKSPACE, "gat_lcgn: workspace %zu < required %zu", ws_bytes, L.total);
    if (N == 0) return GVQA_OK;
    GVQA_REQUIRE(p->lin_l_weight && p->lin_r_weight && p->cal_x_weight && p->proj_cmd_weight && p->cal_cmd_weight, GVQA_E_INVALID,
                 "gat_lcgn: null weight");
    GVQA_REQUIRE(x && cmd && out, GVQA_E_INVALID, "gat_lcgn: null tensor");
    GVQA_REQUIRE(aligned16(out), GVQA_E_UNSUPPORTED, "gat_lcgn: out must be 16-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    char* base = static_cast<char*>(ws);
    auto P = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    // the stacked weights: the caller's own memory when it already holds them back to back (the Python module caches them so),
    // else a copy in the workspace
    const float* Wst = p->lin_l_weight;
    if (p->lin_r_weight != Wst + HC * K || p->cal_x_weight != Wst + 2 * HC * K) {
        const size_t wb = (size_t)HC * K * sizeof(float);
        GVQA_HIP_CHECK(hipMemcpyAsync(P(L.Wst), p->lin_l_weight, wb, hipMemcpyDeviceToDevice, stream));
        GVQA_HIP_CHECK(hipMemcpyAsync(P(L.Wst) + HC * K, p->lin_r_weight, wb, hipMemcpyDeviceToDevice, stream));
        GVQA_HIP_CHECK(hipMemcpyAsync(P(L.Wst) + 2 * HC * K, p->cal_x_weight, wb, hipMemcpyDeviceToDevice, stream));
        Wst = P(L.Wst);
    }
    const float* Wpc = p->proj_cmd_weight;
    if (p->cal_cmd_weight != Wpc + HC * cmd_dim) {
        const size_t wb = (size_t)HC * cmd_dim * sizeof(float);
        GVQA_HIP_CHECK(hipMemcpyAsync(P(L.Wpc), p->proj_cmd_weight, wb, hipMemcpyDeviceToDevice, stream));
        GVQA_HIP_CHECK(hipMemcpyAsync(P(L.Wpc) + HC * cmd_dim, p->cal_cmd_weight, wb, hipMemcpyDeviceToDevice, stream));
        Wpc = P(L.Wpc);
    }
    const LinearEpilogue none{nullptr, nullptr, 0, nullptr, 0, 0};
    {   // J = x . [lin_l; lin_r; cal_x]^T: one product, the arithmetic GVQA_OPT_PROJECTION selects       lcgn.py:144-145,230
        StageTimer tp(GVQA_STAGE_PROJ, stream);
        rc = launch_linear_auto(N, 3 * HC, K, x, K, Wst, K, none, P(L.J), 3 * HC, base + L.scratch, L.total - L.scratch, stream);
        if (rc) return rc;
    }
    {   // pc = cmd . [proj_cmd; cal_cmd]^T, per graph                                                     :148-149
        StageTimer tq(GVQA_STAGE_GRAPH_TERM, stream);
        rc = launch_linear_t(B, 2 * HC, cmd_dim, cmd, cmd_dim, Wpc, cmd_dim, none, P(L.pc), 2 * HC, 1, 0, 0, 0, 0, stream);
        if (rc) return rc;
    }
    StageTimer tm(GVQA_STAGE_MP, stream);
    return launch_lcgn_attention(g, heads, C, concat, negative_slope, P(L.J), 3 * HC, P(L.pc), 2 * HC, p->bias, out,
                                 concat ? HC : C, alpha_out, false, nullptr, stream);
}

}  // extern "C"
