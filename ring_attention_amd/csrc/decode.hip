// Single-query (decode) attention partial for tree-attention decoding.
//
// Capability counterpart of the reference's tree-decode local partial
// (/root/reference/ring_attention_pytorch/tree_attn_decoding.py:54-79).
// Memory-bound: one wave per (b, h); KV streamed with 16-byte loads; softmax
// via in-wave shuffle reduction; fp32 out + lse emitted for the cross-rank
// RCCL merge (done in Python with a packed all-reduce).

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "decode_common.h"

namespace ring_attn {

// FP8 = the KV cache is 8-bit (half the HBM bytes — decode is bandwidth-
// bound, measured 1.5-1.6 TB/s on the bf16 stream): k/v are e4m3 rows with
// one e8m0 scale per kv row (kscale/vscale); q stays bf16.
template <int D, bool FP8>
__global__ __launch_bounds__(256) void decode_partial_kernel(DecodeParams p) {
    // one wave per (b, q-head, query token); 4 waves per block; blockIdx.y
    // splits the KV range into `chunks` partials (merged on the host) so
    // long sequences use the whole chip.  Multi-query (speculative / tree
    // heads) and GQA share the kv stream through L2/L3: the extra waves of
    // one kv head re-read lines the first wave just fetched, so >= 2
    // queries/step cost far less than 2x one query.
    const int rows = p.b * p.h * p.nq;
    const int wave_global = (blockIdx.x * 4) + (threadIdx.x >> 6);
    if (wave_global >= rows) return;
    const DecodeRow r = decode_row(wave_global, p.h, p.hk, p.nq);
    const int lane = threadIdx.x & 63;
    const int chunk = blockIdx.y;
    const long per = (p.n + gridDim.y - 1) / gridDim.y;
    const long j_lo = chunk * per;
    const long j_hi = min(p.n, j_lo + per);
    const long kv0 = ((long)r.b * p.hk + r.hk) * p.n;   // first row of this kv head

    DecodeState<D> st;
    st.init((const __bf16*)p.q + ((long)r.bh * p.nq + r.iq) * D);
    for (long j = j_lo + lane; j < j_hi; j += 64) {
        const long row = kv0 + j;
        if constexpr (FP8) {
            st.fold_fp8((const unsigned char*)p.k + row * D,
                        (const unsigned char*)p.v + row * D,
                        (const unsigned char*)p.kscale + row,
                        (const unsigned char*)p.vscale + row, p.scale);
        } else {
            st.fold_bf16((const __bf16*)p.k + row * D, (const __bf16*)p.v + row * D,
                         p.scale);
        }
    }
    const long slot = (long)chunk * rows + (long)r.bh * p.nq + r.iq;
    st.finish(lane, p.out + slot * D, p.lse + slot);
}

template <bool FP8>
static void launch_decode_partial_t(const DecodeParams& p, int head_dim, hipStream_t stream) {
    int waves = p.b * p.h * p.nq;
    // the binding always sets p.chunks
    long chunks = p.chunks > 0 ? p.chunks : decode_default_chunks(p.n, waves);
    dim3 grid((waves + 3) / 4, (unsigned)chunks);
    dim3 block(256);
    if (head_dim == 64) {
        hipLaunchKernelGGL((decode_partial_kernel<64, FP8>), grid, block, 0, stream, p);
    } else if (head_dim == 128) {
        hipLaunchKernelGGL((decode_partial_kernel<128, FP8>), grid, block, 0, stream, p);
    } else {
        __builtin_trap();
    }
}

void launch_decode_partial(const DecodeParams& p, int head_dim, hipStream_t stream) {
    launch_decode_partial_t<false>(p, head_dim, stream);
}

void launch_decode_partial_fp8(const DecodeParams& p, int head_dim, hipStream_t stream) {
    launch_decode_partial_t<true>(p, head_dim, stream);
}


// ---------------------------------------------------------------------------
// Fused kv-chunk merge: combine the S per-chunk partials (out, lse) into one
// (out, lse) with the logsumexp weights.  The torch expression for this
// (max + exp + weighted sums over the S axis) costs ~50 us of reduce/
// elementwise dispatches per decode step at S = 256 — more than the decode
// kernel itself (30 us).  One wave per (b, h, nq) row; lanes parallel over d.
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void decode_merge_kernel(DecodeMergeParams p) {
    // one BLOCK per row: the 4 waves split the S chunks (a single wave
    // serially streaming S*D floats was latency-bound at decode's tiny
    // row counts), lanes parallel over d; LDS combines the 4 partials
    constexpr int DR = D / 64;
    const long row = blockIdx.x;
    const int wid = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;

    __shared__ float lm[4];
    __shared__ float lden[4];
    __shared__ float lacc[4][D];

    // global max over all S (each thread strides the whole range)
    float m = MASK_VALUE_F;
    for (int sC = (int)threadIdx.x; sC < p.s; sC += 256)
        m = fmaxf(m, p.lses[(long)sC * p.rows + row]);
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        m = fmaxf(m, __shfl_xor(m, off));
    if (lane == 0) lm[wid] = m;
    __syncthreads();
    m = fmaxf(fmaxf(lm[0], lm[1]), fmaxf(lm[2], lm[3]));

    // wave w accumulates chunks s = w, w+4, ...
    float den = 0.f;
    float acc[DR];
    #pragma unroll
    for (int r = 0; r < DR; ++r) acc[r] = 0.f;
    for (int sC = wid; sC < p.s; sC += 4) {
        float w = __expf(p.lses[(long)sC * p.rows + row] - m);
        den += w;
        const float* op = p.outs + ((long)sC * p.rows + row) * D;
        #pragma unroll
        for (int r = 0; r < DR; ++r)
            acc[r] += w * op[r * 64 + lane];
    }
    if (lane == 0) lden[wid] = den;
    #pragma unroll
    for (int r = 0; r < DR; ++r) lacc[wid][r * 64 + lane] = acc[r];
    __syncthreads();

    if (wid == 0) {
        float den_t = lden[0] + lden[1] + lden[2] + lden[3];
        float den_safe = fmaxf(den_t, 1e-38f);
        float inv = 1.f / den_safe;
        float* dst = p.out + row * D;
        #pragma unroll
        for (int r = 0; r < DR; ++r) {
            int d = r * 64 + lane;
            dst[d] = (lacc[0][d] + lacc[1][d] + lacc[2][d] + lacc[3][d]) * inv;
        }
        if (lane == 0) p.lse[row] = __logf(den_safe) + m;
    }
}

void launch_decode_merge(const DecodeMergeParams& p, int head_dim, hipStream_t stream) {
    dim3 grid((unsigned)p.rows);
    dim3 block(256);
    if (head_dim == 64) {
        hipLaunchKernelGGL(decode_merge_kernel<64>, grid, block, 0, stream, p);
    } else if (head_dim == 128) {
        hipLaunchKernelGGL(decode_merge_kernel<128>, grid, block, 0, stream, p);
    } else {
        __builtin_trap();
    }
}

}  // namespace ring_attn
