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

namespace ring_attn {

template <int D, bool FP8, bool WIN>
__global__ __launch_bounds__(256) void decode_partial_paged_kernel(PagedDecodeParams p) {
    // one wave per (b, q-head, query token); 4 waves per block; grid.y is
    // the kv-split.  The wave->row mapping (decode_row) and the row body
    // (DecodeState) are decode_common.h's, shared with the dense kernels.
    const int rows = p.b * p.h * p.nq;
    // grid = (row blocks, S) like the dense kernels.  With ragged lengths the
    // hardware's round-robin of consecutive workgroup ids over the 8 XCDs
    // would pin each sequence's row blocks (blockIdx.x, the fast index) to
    // the same one or two XCDs — the longest sequence then streams through a
    // fraction of the chip (measured: ragged b=8 601 us vs 241 us).
    // chunk_major (set by the binding for b > 1) re-reads the linear
    // workgroup id with the kv chunk as the fast index, so every row's
    // chunks spread over all XCDs.
    const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y;
    const int row_block = p.chunk_major ? (int)(lin / gridDim.y) : (int)blockIdx.x;
    const int chunk = p.chunk_major ? (int)(lin % gridDim.y) : (int)blockIdx.y;
    const int wave_global = (row_block * 4) + (threadIdx.x >> 6);
    if (wave_global >= rows) return;
    const DecodeRow r = decode_row(wave_global, p.h, p.hk, p.nq);
    const int b = r.b, hk = r.hk, iq = r.iq;
    const int lane = threadIdx.x & 63;

    // per-row key limit: the sequence's own length (never past what the
    // table can address); with `causal` the last nq cached positions are the
    // queries' own tokens and query iq sees up to and including its own
    const int shift = p.page_shift;
    const long cap = (long)p.max_pages << shift;
    long limit = min((long)p.seq_lens[b], cap);
    if (p.causal) limit -= (p.nq - 1 - iq);
    limit = max(limit, 0L);
    // lookback window (WIN): the row's query sits at position
    // seq_len + kv_after - nq + iq in local key coordinates (kv_after =
    // tokens of the sequence held by later ranks) and attends only keys
    // j >= position - win, so its span is [lo, limit).  The unwindowed
    // instantiation keeps lo = base = 0 as constants.
    long lo = 0;
    if constexpr (WIN) {
        const long len = min((long)p.seq_lens[b], cap);
        const long after = p.kv_after ? (long)p.kv_after[b] : 0L;
        lo = min(max(len + after - p.nq + iq - p.win, 0L), limit);
    }
    const long base = lo & ~63L;
    // kv-split of THIS row's span: a slice of the batch-wide max range
    // would leave short sequences on chunk 0 only.  The span is cut from
    // its 64-aligned start and the per-chunk length is rounded up to 64 keys
    // so every loop pass of the wave starts 64-aligned (for page_size >= 64
    // its 64 keys then share one page).  Chunks past the row's end are
    // empty and still write their partial below; so does a row whose span
    // is empty (lo == limit), which touches neither the table nor the pool.
    long per = (limit - base + gridDim.y - 1) / gridDim.y;
    per = (per + 63) & ~63L;
    const long j_lo = base + chunk * per;
    const long j_hi = (!WIN || lo < limit) ? min(limit, j_lo + per) : j_lo;

    const int* bt = p.block_table + (long)b * p.max_pages;
    const long pmask = (1L << shift) - 1;
    const bool uniform_page = shift >= 6;

    DecodeState<D> st;
    st.init((const __bf16*)p.q + ((long)r.bh * p.nq + iq) * D);

    // each lane handles keys lane, lane+64, ...; the page id of the NEXT pass
    // is fetched before the current rows are consumed so the dependent
    // table -> row load chain overlaps the row math.  Table entries are read
    // only for j < limit, i.e. only valid entries are ever touched.
    // Keys in [base, lo) fall in the row's FIRST pass only (every later pass
    // starts at or beyond base + 64 > lo) and do no row math.  Their table
    // entries differ by page size:
    //   page_size < 64  such a key can sit in a released page (entry -1):
    //                   a lane reads its entry only when lo <= j;
    //   page_size >= 64 the pass lies in the page that holds lo, which the
    //                   host guard keeps live, and the id comes from the
    //                   first lane: the read is NOT predicated on lo (lane 0
    //                   would otherwise hand -1 to the whole wave) and only
    //                   the row math is masked.
    long j = j_lo + lane;
    int pg = (j < j_hi && (!WIN || uniform_page || j >= lo)) ? bt[j >> shift] : -1;
    while (j < j_hi) {
        const long jn = j + 64;
        const int pg_next = jn < j_hi ? bt[jn >> shift] : -1;
        // page_size >= 64: the wave's 64 keys share the page -> scalar id
        if (uniform_page) pg = __builtin_amdgcn_readfirstlane(pg);
        // a page id outside the pool is never dereferenced
        if ((unsigned)pg < (unsigned)p.num_pages && (!WIN || j >= lo)) {
            const long row = ((((long)pg * p.hk + hk) << shift) | (j & pmask));
            if constexpr (FP8) {
                st.fold_fp8((const unsigned char*)p.k_pages + row * D,
                            (const unsigned char*)p.v_pages + row * D,
                            (const unsigned char*)p.kscale + row,
                            (const unsigned char*)p.vscale + row, p.scale);
            } else {
                st.fold_bf16((const __bf16*)p.k_pages + row * D,
                             (const __bf16*)p.v_pages + row * D, p.scale);
            }
        }
        j = jn;
        pg = pg_next;
    }

    // an empty chunk still writes its partial (out = 0, lse = MASK_VALUE_F)
    const long slot = (long)chunk * rows + (long)r.bh * p.nq + iq;
    st.finish(lane, p.out + slot * D, p.lse + slot);
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
    // the window is a template switch: the unwindowed instantiations keep
    // the code they had before the window existed
#define LAUNCH_PAGED_DECODE(D_, FP8_)                                              \
    do {                                                                           \
        if (p.has_win)                                                             \
            hipLaunchKernelGGL((decode_partial_paged_kernel<D_, FP8_, true>),      \
                               grid, block, 0, stream, p);                         \
        else                                                                       \
            hipLaunchKernelGGL((decode_partial_paged_kernel<D_, FP8_, false>),     \
                               grid, block, 0, stream, p);                         \
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
        // e = ceil(log2(max(amax, 2^-126) / 448)), integer-exact: with
        // amax = mant * 2^ex (mant in [1, 2)) and 448 = 1.75 * 2^8 this is
        // ex - 8 when mant <= 1.75 and ex - 7 otherwise; zero / subnormal
        // amax clamps to 2^-126 and lands on the lower clamp below
        const unsigned bits = __float_as_uint(amax);
        const int ex = (int)((bits >> 23) & 0xffu);
        const unsigned mant = bits & 0x7fffffu;
        int e = ex == 0 ? -127 : ex - 127 - 8 + (mant > 0x600000u ? 1 : 0);
        e = min(max(e, -127), 127);
        #pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = ldexpf(x[i], -e);   // exact power-of-two scaling
        int u = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
        u = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], u, true);
        if (act) {
            unsigned char* dst = (unsigned char*)(is_v ? p.v_pages : p.k_pages) + drow * D;
            *(unsigned*)(dst + sl * 4) = (unsigned)u;
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
