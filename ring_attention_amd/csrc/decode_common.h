// The decode row body shared by the dense (decode.hip) and paged
// (decode_paged.hip) partial kernels: which (b, head, query token) a wave
// owns, how one key row folds into its online softmax, and how the 64 lanes
// merge into the (out, lse) partial that decode_merge consumes.  The kernels
// keep what is their own: where a key row lives and which keys a row spans.
#pragma once

#include "attn_common.h"

namespace ring_attn {

struct DecodeRow {
    int b, h, hk, iq;       // batch, q head, its kv head, query token
    int bh;                 // b * H + h
};

// group-major wave->row mapping: consecutive waves (the 4 of a block,
// which land on ONE CU and one XCD L2) cover the query tokens and then
// the GQA group-mates of the SAME kv head, so their shared kv stream is
// fetched once per L2.  The natural (b,h,iq) order instead put 4
// DIFFERENT kv heads in each block and scattered a group's readers
// across the 8 XCDs' private L2s — each re-fetched the stream from HBM
// (measured: 32q/4kv nq=1 decode at 0.27 TB/s effective).  Output
// layout is unchanged; only the wave->row assignment differs.
__device__ __forceinline__ DecodeRow decode_row(int wave_global, int h, int hk, int nq) {
    DecodeRow row;
    const int G = h / hk;
    row.iq = wave_global % nq;
    int r = wave_global / nq;
    const int g = r % G;  r /= G;
    row.hk = r % hk;                   // reference tile GQA pairing
    row.b = r / hk;
    row.h = row.hk + g * hk;           // group-mate g of kv head hk
    row.bh = row.b * h + row.h;
    return row;
}

// One wave's running state over the keys it has seen: each lane handles keys
// lane, lane+64, ... of the row's span with its own (m, l, acc); finish()
// merges the 64 lanes.
template <int D>
struct DecodeState {
    float qreg[D];          // q in registers (fp32), replicated per lane
    float acc[D];
    float m, l;

    __device__ __forceinline__ void init(const __bf16* qp) {
        #pragma unroll
        for (int d = 0; d < D; ++d) qreg[d] = (float)qp[d];
        m = MASK_VALUE_F;
        l = 0.f;
        #pragma unroll
        for (int d = 0; d < D; ++d) acc[d] = 0.f;
    }

    // one bf16 key row: score and value pass fused online, 16-byte loads
    __device__ __forceinline__ void fold_bf16(const __bf16* krow, const __bf16* vrow,
                                              float scale) {
        float s = 0.f;
        #pragma unroll
        for (int d = 0; d < D; d += 8) {
            bf16x8 kv8 = *(const bf16x8*)(krow + d);
            #pragma unroll
            for (int e = 0; e < 8; ++e) s += qreg[d + e] * (float)kv8[e];
        }
        s *= scale;
        float m_new = fmaxf(m, s);
        float alpha = __expf(m - m_new);
        float w = __expf(s - m_new);
        l = l * alpha + w;
        #pragma unroll
        for (int d = 0; d < D; d += 8) {
            bf16x8 vv8 = *(const bf16x8*)(vrow + d);
            #pragma unroll
            for (int e = 0; e < 8; ++e) acc[d + e] = acc[d + e] * alpha + w * (float)vv8[e];
        }
        m = m_new;
    }

    // one e4m3 key row with ONE e8m0 scale per row (*ksc, *vsc): the k scale
    // folds into the score (s_true = 2^ek * dot(q, k8)) and the v scale into
    // the softmax weight (acc += (w * 2^ev) * v8) — the same fp32 math as the
    // bf16 row, only the loads halve
    __device__ __forceinline__ void fold_fp8(const unsigned char* krow,
                                             const unsigned char* vrow,
                                             const unsigned char* ksc,
                                             const unsigned char* vsc, float scale) {
        float s = 0.f;
        #pragma unroll
        for (int d = 0; d < D; d += 16) {
            uint4 k16 = *(const uint4*)(krow + d);
            const unsigned* kw = (const unsigned*)&k16;
            #pragma unroll
            for (int w4 = 0; w4 < 4; ++w4) {
                f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(kw[w4], false);
                f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(kw[w4], true);
                s += qreg[d + 4 * w4 + 0] * lo[0] + qreg[d + 4 * w4 + 1] * lo[1]
                   + qreg[d + 4 * w4 + 2] * hi[0] + qreg[d + 4 * w4 + 3] * hi[1];
            }
        }
        s *= scale * exp2f((float)*ksc - 127.f);
        float m_new = fmaxf(m, s);
        float alpha = __expf(m - m_new);
        float w = __expf(s - m_new) * exp2f((float)*vsc - 127.f);
        l = l * alpha + __expf(s - m_new);
        #pragma unroll
        for (int d = 0; d < D; d += 16) {
            uint4 v16 = *(const uint4*)(vrow + d);
            const unsigned* vw = (const unsigned*)&v16;
            #pragma unroll
            for (int w4 = 0; w4 < 4; ++w4) {
                f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(vw[w4], false);
                f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(vw[w4], true);
                // updated in the pairs the converts deliver: four scalar
                // updates get paired (lo[0], hi[0]) by the vectoriser, at
                // two v_mov per packed op
                int base = d + 4 * w4;
                f32x2 a01 = {acc[base + 0], acc[base + 1]};
                f32x2 a23 = {acc[base + 2], acc[base + 3]};
                a01 = a01 * alpha + w * lo;
                a23 = a23 * alpha + w * hi;
                acc[base + 0] = a01[0];  acc[base + 1] = a01[1];
                acc[base + 2] = a23[0];  acc[base + 3] = a23[1];
            }
        }
        m = m_new;
    }

    // cross-lane merge (all 64 lanes -> every lane holds the wave's stats),
    // then lane 0 writes the partial: out row (D floats) and its lse slot
    __device__ __forceinline__ void finish(int lane, float* op, float* lse_slot) {
        #pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            float m2 = __shfl_xor(m, off);
            float l2 = __shfl_xor(l, off);
            float m_new = fmaxf(m, m2);
            float a1 = __expf(m - m_new), a2 = __expf(m2 - m_new);
            l = l * a1 + l2 * a2;
            #pragma unroll
            for (int d = 0; d < D; ++d) {
                float o2 = __shfl_xor(acc[d], off);
                acc[d] = acc[d] * a1 + o2 * a2;
            }
            m = m_new;
        }
        // an empty chunk lands here with acc == 0, l == 0, m == MASK_VALUE_F and
        // writes out = 0, lse = MASK_VALUE_F (the partial buffers are not
        // zero-filled); decode_merge gives it weight exp(MASK - max) == 0
        float l_safe = fmaxf(l, 1e-38f);
        if (lane == 0) {
            float inv = 1.f / l_safe;
            #pragma unroll
            for (int d = 0; d < D; ++d) op[d] = acc[d] * inv;
            *lse_slot = __logf(l_safe) + m;
        }
    }
};

}  // namespace ring_attn
