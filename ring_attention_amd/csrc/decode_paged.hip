// Paged KV-cache decode: block-table pages + per-sequence lengths.
//
// Serving counterpart of decode.hip.  The cache is a pool of fixed-size pages
// (num_pages, HK, page_size, D); sequence b's key j lives at page
// block_table[b][j >> log2(page_size)], row j & (page_size - 1).  A
// (page, kv head) block is page_size x D contiguous, so the 16-byte row loads
// of the dense kernels carry over unchanged; the only extra traffic is one
// 4-byte table read per page per wave.  Two kernels:
//   decode_partial_paged_kernel  reads the pool  (bf16 or e4m3 + e8m0 rows)
//   paged_kv_append_kernel       writes new tokens into it (fused fp8 quant)
// The partial contract (out fp32 (S,B,HQ,NQ,D), lse fp32 (S,B,HQ,NQ,1)) is the
// dense kernels', so decode_merge is reused as is.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "decode_common.h"
#include "fp8_quant.h"

namespace ring_attn {

template <int D, bool FP8, bool WIN>
__global__ __launch_bounds__(256) void decode_partial_paged_kernel(PagedDecodeParams p) {
    constexpr bool SOFTCLAMP = false;
#include "decode_paged_rows.inc"
}

// The same rows with logit capping (decode_common.h's SOFTCLAMP), built
// without packed f32 ops.
template <int D, bool FP8, bool WIN>
__global__ __launch_bounds__(256) RING_ATTN_NO_PACKED_F32
void decode_partial_paged_softclamp_kernel(PagedDecodeParams p) {
    constexpr bool SOFTCLAMP = true;
#include "decode_paged_rows.inc"
}

void launch_decode_partial_paged(const PagedDecodeParams& p, int head_dim, bool fp8,
                                 hipStream_t stream) {
    int waves = p.b * p.h * p.nq;
    // kv-split fallback (the binding always sets p.chunks), driven by the
    // host-known longest sequence (no device read on the step path);
    // with a window the longest ROW SPAN drives the split, not the longest
    // sequence: win + 1 keys, nq - 1 more over the query tokens, up to 63 of
    // alignment in front
    const long span = p.has_win ? min(p.max_seq_len, p.win + p.nq + 63) : p.max_seq_len;
    long chunks = p.chunks > 0 ? p.chunks : decode_default_chunks(span, waves);
    dim3 grid((waves + 3) / 4, (unsigned)chunks);
    dim3 block(256);
    // the window and the clamp are template switches: the instantiations
    // without them keep the code they had before either existed
#define LAUNCH_PAGED_DECODE_K(K_, D_, FP8_)                                        \
    do {                                                                           \
        if (p.has_win)                                                             \
            hipLaunchKernelGGL((K_<D_, FP8_, true>), grid, block, 0, stream, p);   \
        else                                                                       \
            hipLaunchKernelGGL((K_<D_, FP8_, false>), grid, block, 0, stream, p);  \
    } while (0)
#define LAUNCH_PAGED_DECODE(D_, FP8_)                                              \
    do {                                                                           \
        if (p.softclamp)                                                           \
            LAUNCH_PAGED_DECODE_K(decode_partial_paged_softclamp_kernel, D_, FP8_);\
        else                                                                       \
            LAUNCH_PAGED_DECODE_K(decode_partial_paged_kernel, D_, FP8_);          \
    } while (0)
    if (head_dim == 64 && !fp8) {
        LAUNCH_PAGED_DECODE(64, false);
    } else if (head_dim == 128 && !fp8) {
        LAUNCH_PAGED_DECODE(128, false);
    } else if (head_dim == 64) {
        LAUNCH_PAGED_DECODE(64, true);
    } else if (head_dim == 128) {
        LAUNCH_PAGED_DECODE(128, true);
    } else {
        __builtin_trap();
    }
#undef LAUNCH_PAGED_DECODE
#undef LAUNCH_PAGED_DECODE_K
}


// ---------------------------------------------------------------------------
// Append: token t < append_lens[b] of sequence b goes to position
// seq_lens[b] + t (seq_lens = lengths BEFORE the append; the host advances
// them).  One wave per (b, kv head, t): lanes 0-31 carry the K row, lanes
// 32-63 the V row.  bf16 mode is a 16-byte row copy.  fp8 mode quantises the
// row in flight to the quantize_kv_cache format: one e8m0 scale
// 2^ceil(log2(amax / 448)) per row, e4m3 data.  Nothing else in the pool is
// written.
// ---------------------------------------------------------------------------
template <int D, bool FP8>
__global__ __launch_bounds__(256) void paged_kv_append_kernel(PagedAppendParams p) {
    const long rows = (long)p.b * p.hk * p.t;
    const long wave_global = ((long)blockIdx.x * 4) + (threadIdx.x >> 6);
    if (wave_global >= rows) return;
    const int t = (int)(wave_global % p.t);
    long r = wave_global / p.t;
    const int hk = (int)(r % p.hk);
    const int b = (int)(r / p.hk);
    if (t >= p.append_lens[b]) return;                 // ragged: nothing to do

    const int shift = p.page_shift;
    const long pos = (long)p.seq_lens[b] + t;
    const long slot = pos >> shift;
    if (slot >= p.max_pages) return;                   // host checks; never write astray
    const int pg = p.block_table[(long)b * p.max_pages + slot];
    if ((unsigned)pg >= (unsigned)p.num_pages) return;
    const long drow = ((((long)pg * p.hk + hk) << shift) | (pos & ((1L << shift) - 1)));
    const long srow = wave_global;                     // (B, HK, T, D) row index

    const int lane = threadIdx.x & 63;
    const int is_v = lane >> 5;
    const int sl = lane & 31;
    const __bf16* src = (const __bf16*)(is_v ? p.v_new : p.k_new) + srow * D;

    if constexpr (!FP8) {
        if (sl < D / 8) {
            __bf16* dst = (__bf16*)(is_v ? p.v_pages : p.k_pages) + drow * D;
            *(bf16x8*)(dst + sl * 8) = *(const bf16x8*)(src + sl * 8);
        }
    } else {
        // 4 elements per lane: D/4 (16 or 32) lanes of each half-wave active
        const bool act = sl < D / 4;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (act) {
            bf16x4 x4 = *(const bf16x4*)(src + sl * 4);
            #pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = (float)x4[e];
        }
        float amax = fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3])));
        #pragma unroll
        for (int off = 16; off > 0; off >>= 1)         // stays inside the half-wave
            amax = fmaxf(amax, __shfl_xor(amax, off));
        // the project's one scale rule and exact scaling (fp8_quant.h)
        const int e = e8m0_exponent(amax);
        const unsigned u = e4m3_pack4(x[0], x[1], x[2], x[3], e);
        if (act) {
            unsigned char* dst = (unsigned char*)(is_v ? p.v_pages : p.k_pages) + drow * D;
            *(unsigned*)(dst + sl * 4) = u;
        }
        if (sl == 0) {
            unsigned char* sc = (unsigned char*)(is_v ? p.vscale : p.kscale);
            sc[drow] = (unsigned char)(e + 127);
        }
    }
}

void launch_paged_kv_append(const PagedAppendParams& p, int head_dim, bool fp8,
                            hipStream_t stream) {
    long waves = (long)p.b * p.hk * p.t;
    if (waves == 0) return;
    dim3 grid((unsigned)((waves + 3) / 4));
    dim3 block(256);
    if (head_dim == 64 && !fp8) {
        hipLaunchKernelGGL((paged_kv_append_kernel<64, false>), grid, block, 0, stream, p);
    } else if (head_dim == 128 && !fp8) {
        hipLaunchKernelGGL((paged_kv_append_kernel<128, false>), grid, block, 0, stream, p);
    } else if (head_dim == 64) {
        hipLaunchKernelGGL((paged_kv_append_kernel<64, true>), grid, block, 0, stream, p);
    } else if (head_dim == 128) {
        hipLaunchKernelGGL((paged_kv_append_kernel<128, true>), grid, block, 0, stream, p);
    } else {
        __builtin_trap();
    }
}

}  // namespace ring_attn
