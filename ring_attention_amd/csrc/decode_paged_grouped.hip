// Grouped paged decode: all (group-mate, draft) rows of one kv head share one
// pass over the cache, on the matrix cores, with a token-tree mask.
//
// decode_paged.hip runs one wave per (b, q head, query token) and every wave
// streams K/V for itself: a GQA group of G heads with nq drafts reads the same
// rows G * nq times.  Here the R = G * nq rows of a (b, kv head) are stacked
// into 32-row tiles (row r = g * nq + iq is q head hk + g * HK, draft iq) and
// K/V are read once per tile:
//   * grid (b * HK * row tiles, S); a workgroup is 4 waves and owns one row
//     tile and one kv chunk.  Its waves take the chunk's 32-key blocks
//     round-robin, so a key row is consumed by exactly one wave: K needs no
//     LDS and the loop has no workgroup barrier.  Each wave keeps (m, l, O)
//     for all 32 rows; the four states meet in LDS behind the one barrier of
//     the epilogue.
//   * scores: S^T = K Q^T with v_mfma_f32_32x32x16_bf16.  The K fragment is
//     the dense kernels' 16-byte row load (lane l: key row l & 31, elements
//     16 * step + 8 * (l >> 5)) and goes from global memory straight into the
//     MFMA; the Q^T fragments are loaded once per wave.  Softmax is the
//     forward's (exp2 domain, one permlane32 swap per reduction, l summed
//     from the unrounded exponentials).
//   * PV: O^T += V^T P^T.  P is packed to bf16 in registers in the order the
//     score tile delivers it (kperm_pair's k order).  V is the one operand
//     that needs a transpose: the wave's 32 x D block is staged row-major
//     into a wave-private LDS slice (16-byte chunks, XOR-swizzled) and read
//     back with ds_read_b64_tr_b16 in that k order.  The slice is
//     double-buffered: the loads of block i + 1 are issued before block i's
//     MFMAs and land in the other buffer after them.
//   * fp8 pools: raw e4m3 bytes and the row's e8m0 byte stay in the staging
//     registers and become bf16 right before the MFMA (K) or the LDS write
//     (V): e4m3 x 2^(scale - 127), exact for normal-range rows.
//   * paging: a 32-key block starts 32-aligned, so it lies in one page for
//     page_size >= 32 and in two for page_size 16.  Both halves' ids are
//     wave-uniform table reads (the same entry twice for page_size >= 32),
//     fetched one block ahead; a lane picks by its key row.  Only entries
//     below ceil(len / page_size) are read, an id outside the pool is never
//     dereferenced, and rows at or beyond the chunk's end are zero-filled
//     without forming an address (0 * NaN would poison the MFMA).
//   * window (WIN): row iq's query sits at qpos = len + kv_after[b] - nq + iq
//     and attends keys [lo, limit), lo = clamp(qpos - window, 0, limit)
//     (tree_decode.py's _window_spans; with tree_bits the mask is the chain,
//     host-checked, so limit = P0 + iq + 1).  lo never decreases in iq:
//     lo_min (row 0) and lo_max (row nq - 1) are wave-uniform.  The workgroup
//     splits [lo_min & ~127, len) instead of [0, len), so blocks stay
//     32-aligned and passes 128-aligned; a wave drops the blocks that end at
//     or below lo_min, and a block is open only from lo_max up: below it the
//     masked arm also tests key >= the lane's own lo.  Pages below the one
//     that holds lo_min may be released: a 16-key half with no key at or
//     above lo_min reads no table entry and is zero-filled (every element
//     there is masked anyway).  A sequence whose row 0 is dead has only dead
//     rows and touches neither the table nor the pool.
//   * mask: with tree_bits the last nq cached keys are the drafts' own
//     tokens; key P0 + t (P0 = len - nq) is visible to draft iq iff bit t of
//     tree_bits[b][iq] is set, keys below P0 to every row.  Only blocks that
//     reach beyond P0 test per element.  Without tree_bits P0 = len.
//   * SOFTCLAMP (logit capping, the training kernels' definition): every
//     score becomes x = c * log2e * tanh(s * scale / c) before the mask, in
//     both arms; the max is taken on x and the exponent is exp2(x - m), with
//     no scale left to fold.  scale / c and c * log2e are wave-uniform.
// The partial contract is decode_paged.hip's (out fp32 (S,B,HQ,NQ,D), lse fp32
// (S,B,HQ,NQ,1), out = 0 and lse = MASK_VALUE_F where a row saw no key), so
// decode_merge and the cross-rank merge are reused unchanged.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

#include "attn_common.h"

// Packed f32 ops are switched off for every function of this file: the
// softmax and rescale blocks sit beside MFMAs, where a v_pk_*_f32 costs more
// than the two scalar ops it replaces (attn_common.h, sub_f32).  A function
// with the feature off cannot inline one that has it on, so nothing here
// calls a HIP header function that is not always_inline: the barrier, the
// ballot, the bit cast and the vectors are the compiler's own.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace ring_attn {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int GWAVES = 4;       // waves per workgroup
constexpr int GTILE = 32;       // rows per tile and keys per block
constexpr int GPASS = GWAVES * GTILE;   // keys a workgroup consumes per pass

// 8 e4m3 bytes x 2^(sbyte - 127) -> 8 bf16 (attn_fwd_paged.hip's rule).  The
// e8m0 byte is the fp32 exponent field; byte 0 (2^-127) is the one subnormal.
__device__ __forceinline__ u32x4 grouped_dequant_e4m3x8(u32x2 raw, unsigned sbyte) {
    const float sc = __builtin_bit_cast(float, sbyte ? sbyte << 23 : 0x00400000u);
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(raw[0], false);
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8(raw[0], true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8(raw[1], false);
    const f32x2 d = __builtin_amdgcn_cvt_pk_f32_fp8(raw[1], true);
    return u32x4{pack_bf16x2(a[0] * sc, a[1] * sc), pack_bf16x2(b[0] * sc, b[1] * sc),
                 pack_bf16x2(c[0] * sc, c[1] * sc), pack_bf16x2(d[0] * sc, d[1] * sc)};
}

// 8 elements of one pool row as they wait in registers: bf16 bits, or raw
// e4m3 bytes plus the row's scale byte (converted at the point of use)
template <bool FP8> struct GroupedChunk;
template <> struct GroupedChunk<false> {
    u32x4 v;
    __device__ __forceinline__ u32x4 bf16_bits() const { return v; }
};
template <> struct GroupedChunk<true> {
    u32x2 raw;
    unsigned sbyte;
    __device__ __forceinline__ u32x4 bf16_bits() const {
        return grouped_dequant_e4m3x8(raw, sbyte);
    }
};

template <int D, bool FP8>
__device__ __forceinline__ GroupedChunk<FP8> grouped_pool_chunk(
        const void* pool, const void* scales, long row, int e0) {
    if constexpr (!FP8) {
        return {*(const u32x4*)((const __bf16*)pool + row * D + e0)};
    } else {
        return {*(const u32x2*)((const unsigned char*)pool + row * D + e0),
                ((const unsigned char*)scales)[row]};
    }
}

}  // namespace

template <int D, bool FP8, bool WIN, bool SOFTCLAMP>
__global__ __launch_bounds__(GWAVES * 64)
void decode_partial_paged_grouped_kernel(PagedGroupedDecodeParams p) {
    static_assert(D == 64 || D == 128);
    constexpr int KSTEPS = D / 16;          // QK^T k-steps
    constexpr int DBLK = D / 32;            // 32-d output blocks
    constexpr int CH = D / 8;               // 16-byte chunks per V row
    constexpr int VREGS = GTILE * CH / 64;  // V chunks per lane (== KSTEPS)
    constexpr int SLICE = 2 * GTILE * D;    // bf16 elements of one wave's slice

    // a wave's slice holds its two V buffers in the loop and its fp32 O^T
    // (D x 32 floats, the same 128 * D bytes) in the epilogue
    __shared__ __align__(16) __bf16 lds_v[GWAVES * SLICE];
    __shared__ float lds_ml[GWAVES][2][GTILE];

    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31;
    const int lhi = lane >> 5;

    // ---- which (b, kv head, row tile, chunk): chunk-major for b > 1, for
    // the reason given in decode_paged.hip
    const int G = p.h / p.hk;
    const int R = G * p.nq;
    const int tiles = (R + GTILE - 1) / GTILE;
    const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y;
    int rb = p.chunk_major ? (int)(lin / gridDim.y) : (int)blockIdx.x;
    const int chunk = p.chunk_major ? (int)(lin % gridDim.y) : (int)blockIdx.y;
    const int tile = rb % tiles;  rb /= tiles;
    const int hk = rb % p.hk;
    const int b = rb / p.hk;

    // ---- the sequence's span and this chunk's share of it (wave-uniform)
    const int shift = p.page_shift;
    const long pmask = (1L << shift) - 1;
    const long len = min(max((long)__builtin_amdgcn_readfirstlane(p.seq_lens[b]), 0L),
                         (long)p.max_pages << shift);
    const long P0 = p.tree_bits ? max(len - p.nq, 0L) : len;
    // window (WIN): qp0 = row 0's qpos - window; the rows' lower bounds run
    // from lo_min (row 0) to lo_max (row nq - 1).  Row 0 dead <=> every row
    // dead (the chain's limit and qpos both grow by one per row; without a
    // mask the limit is len for all).  The unwindowed instantiation keeps
    // base = 0 as a constant.
    long qp0 = 0, lo_min = 0, lo_max = 0;
    bool live = true;
    if constexpr (WIN) {
        const long after = p.kv_after
            ? (long)__builtin_amdgcn_readfirstlane(p.kv_after[b]) : 0L;
        qp0 = len + after - p.nq - p.window;
        const long lim0 = p.tree_bits ? min(len, P0 + 1) : len;
        lo_min = min(max(qp0, 0L), lim0);
        lo_max = min(max(qp0 + p.nq - 1, 0L), len);
        live = lo_min < lim0;
    }
    const long base = lo_min & ~(long)(GPASS - 1);
    long per = (len - base + gridDim.y - 1) / gridDim.y;
    per = (per + GPASS - 1) & ~(long)(GPASS - 1);
    const long j_lo = base + (long)chunk * per;
    const long j_hi = live ? min(len, j_lo + per) : j_lo;

    // ---- this lane's row: q fragments and mask word.  Rows past R run on
    // row 0 and are dropped in the epilogue.
    const int row = tile * GTILE + l31;
    const int row_c = row < R ? row : 0;
    const int g = row_c / p.nq, iq = row_c % p.nq;
    const int h = hk + g * p.hk;
    const __bf16* qrow = (const __bf16*)p.q + (((long)b * p.h + h) * p.nq + iq) * D;
    bf16x8 qf[KSTEPS];
    #pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) qf[ks] = *(const bf16x8*)(qrow + ks * 16 + lhi * 8);
    unsigned long long bits = 0;
    if (p.tree_bits) {
        const int* tb = p.tree_bits + ((long)b * p.nq + iq) * 2;
        bits = (unsigned long long)(unsigned)tb[0] | ((unsigned long long)(unsigned)tb[1] << 32);
    }
    // this row's lower bound as a draft index (key - P0); the draft test
    // below supplies the row's limit
    int tl = 0;
    if constexpr (WIN) tl = (int)(min(max(qp0 + iq, 0L), len) - P0);

    float m_run = MASK_VALUE_F;
    float l_run = 0.f;
    f32x16 o_acc[DBLK];
    #pragma unroll
    for (int db = 0; db < DBLK; ++db) o_acc[db] = f32x16{};

    // ---- staging
    using Chunk = GroupedChunk<FP8>;
    Chunk kst[KSTEPS], vst[VREGS];
    const int* bt = p.block_table + (long)b * p.max_pages;
    const long head_rows = (long)hk << shift;
    const long page_rows = (long)p.hk << shift;
    const int vrow0 = lane / CH, ve0 = (lane % CH) * 8;     // V chunk r: row vrow0 + r * (64 / CH)
    __bf16* slice = lds_v + wid * SLICE;

    // ids of the pages that hold keys [j0, j0 + 16) and [j0 + 16, j0 + 32)
    int pg_a = -1, pg_b = -1;
    // (WIN: a half that ends at or below lo_min may lie in a released page)
    auto table_id = [&](long j) {
        return j < j_hi && (!WIN || j + 16 > lo_min) ? bt[j >> shift] : -1;
    };
    auto load_block = [&](long j0, int id_a, int id_b) {
        auto pool_row = [&](long j, bool& ok) {
            // bit select: written as ?: the two ids become a table in
            // scratch indexed by the half
            const int second = -(int)((j >> 4) & 1);
            const int pg = (id_a & ~second) | (id_b & second);
            ok = j < j_hi && (unsigned)pg < (unsigned)p.num_pages;
            return (long)pg * page_rows + head_rows + (j & pmask);
        };
        bool ok;
        const long krow = pool_row(j0 + l31, ok);
        #pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks)
            kst[ks] = ok ? grouped_pool_chunk<D, FP8>(p.k_pages, p.kscale, krow, ks * 16 + lhi * 8)
                         : Chunk{};
        #pragma unroll
        for (int r = 0; r < VREGS; ++r) {
            const long vrow = pool_row(j0 + vrow0 + r * (64 / CH), ok);
            vst[r] = ok ? grouped_pool_chunk<D, FP8>(p.v_pages, p.vscale, vrow, ve0) : Chunk{};
        }
    };
    auto write_v = [&](int par) {
        #pragma unroll
        for (int r = 0; r < VREGS; ++r) {
            const int vr = vrow0 + r * (64 / CH);
            *(u32x4*)(slice + par * GTILE * D + vr * D + ((ve0 / 8) ^ (vr & 7)) * 8)
                = vst[r].bf16_bits();
        }
    };

    // transposed V reads (KERNELS.md "ds_read_b64_tr_b16"): lane f = lane & 15
    // of 16-lane group g16 addresses row 4 * lhi + (f >> 2) (+ 16 * half + 8 * u),
    // columns db * 32 + 16 * g16 + 4 * (f & 3) .. + 4, and receives
    // out[e] = V[row + e][db * 32 + (lane & 31)]
    typedef __attribute__((address_space(3))) bf16x4* lds_v4;
    const int f15 = lane & 15, g16 = (lane >> 4) & 1;
    const int trow = 4 * lhi + (f15 >> 2);
    int tr_off[DBLK];
    #pragma unroll
    for (int db = 0; db < DBLK; ++db) {
        const int col = db * 32 + 16 * g16 + 4 * (f15 & 3);
        tr_off[db] = trow * D + ((col / 8) ^ (trow & 7)) * 8 + (col % 8);
    }

    const float scale2 = p.scale * LOG2E;
    // SOFTCLAMP: s -> tanh argument, tanh -> exp2-domain score
    const float clamp_in = SOFTCLAMP ? p.scale * __builtin_amdgcn_rcpf(p.softclamp_value) : 0.f;
    const float clamp_out = p.softclamp_value * LOG2E;
    long j0 = j_lo + wid * GTILE;
    // lo_min < base + GPASS: only the first pass holds blocks below lo_min
    if constexpr (WIN) if (j0 + GTILE <= lo_min) j0 += GPASS;
    if (j0 < j_hi) {
        load_block(j0, table_id(j0), table_id(j0 + 16));
        pg_a = table_id(j0 + GPASS);
        pg_b = table_id(j0 + GPASS + 16);
        write_v(0);
    }
    for (int par = 0; j0 < j_hi; j0 += GPASS, par ^= 1) {
        // this block's K fragments leave the staging registers, which then
        // take the next block's loads
        Chunk kc[KSTEPS];
        #pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) kc[ks] = kst[ks];
        const bool more = j0 + GPASS < j_hi;
        if (more) {
            load_block(j0 + GPASS, pg_a, pg_b);
            pg_a = table_id(j0 + 2 * GPASS);
            pg_b = table_id(j0 + 2 * GPASS + 16);
        }

        // ---- S^T[kv][row]
        f32x16 s = f32x16{};
        #pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            union { u32x4 u; bf16x8 v; } kf;
            kf.u = kc[ks].bf16_bits();
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf.v, qf[ks], s, 0, 0, 0);
        }

        // ---- scale, mask.  A block below P0 is visible to every row and
        // keeps raw scores (the scale folds into the exp argument); clamped
        // scores are final in either arm.
        const bool open_block = j0 + GTILE <= P0 && (!WIN || j0 >= lo_max);
        float smax = MASK_VALUE_F;
        if (open_block) {
            if constexpr (SOFTCLAMP) {
                #pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[r] = clamp_out * fast_tanhf(s[r] * clamp_in);
                    smax = fmaxf(smax, s[r]);
                }
            } else {
                #pragma unroll
                for (int r = 0; r < 16; ++r) smax = fmaxf(smax, s[r]);
                smax *= scale2;
            }
        } else {
            const int t0 = (int)(j0 - P0) + 4 * lhi;   // draft index of reg 0's key
            const int nt = (int)(len - P0);            // drafts cached (0 without a mask)
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int t = t0 + (r & 3) + 8 * (r >> 2);
                const bool ok = (!WIN || t >= tl)
                                && (t < 0 || (t < nt && ((bits >> (t & 63)) & 1)));
                float x;
                if constexpr (SOFTCLAMP) {
                    // clamped before the test, as in the forward
                    x = clamp_out * fast_tanhf(s[r] * clamp_in);
                    if (!ok) x = MASK_VALUE_F;
                } else {
                    x = ok ? s[r] * scale2 : MASK_VALUE_F;
                }
                s[r] = x;
                smax = fmaxf(smax, x);
            }
        }
        smax = fmaxf(smax, cross_half(smax));

        // ---- online softmax (the forward's: exact skip of the rescale when
        // no row's max grew; an all-masked row keeps its exps at 0 through
        // the clamped subtrahend)
        const float m_new = fmaxf(m_run, smax);
        const bool any_growth = __builtin_amdgcn_ballot_w64(smax > m_run) != 0;
        const float m_exp = fmaxf(m_new, -1.7e38f);
        const float escale = (open_block && !SOFTCLAMP) ? scale2 : 1.f;
        alignas(16) uint32_t pk[8];
        float partial[8];
        #pragma unroll
        for (int x2 = 0; x2 < 8; ++x2) {
            const float e0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[2 * x2], escale, -m_exp));
            const float e1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[2 * x2 + 1], escale, -m_exp));
            partial[x2] = e0 + e1;
            pk[x2] = pack_bf16x2(e0, e1);
        }
        #pragma unroll
        for (int w = 4; w >= 1; w >>= 1)
            #pragma unroll
            for (int x2 = 0; x2 < w; ++x2) partial[x2] += partial[x2 + w];
        float rowsum = partial[0];
        rowsum += cross_half(rowsum);
        if (any_growth) {
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            l_run = l_run * alpha + rowsum;
            #pragma unroll
            for (int db = 0; db < DBLK; ++db)
                #pragma unroll
                for (int r = 0; r < 16; ++r) o_acc[db][r] *= alpha;
            m_run = m_new;
        } else {
            l_run += rowsum;
        }

        // ---- O^T[d][row] += V^T[d][kv] P^T[kv][row]; pk[4 * ks .. + 3] is the
        // B fragment of k-step ks, keys 16 * ks + 4 * lhi + {0..3, 8..11}
        const __bf16* vbuf = slice + par * GTILE * D;
        #pragma unroll
        for (int db = 0; db < DBLK; ++db)
            #pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (lds_v4)(vbuf + (16 * ks) * D + tr_off[db]));
                const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (lds_v4)(vbuf + (16 * ks + 8) * D + tr_off[db]));
                const bf16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                o_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    vf, *(const bf16x8*)(pk + 4 * ks), o_acc[db], 0, 0, 0);
            }

        if (more) write_v(par ^ 1);
    }

    // ---- epilogue: the four waves' states meet in LDS.  A wave's O^T goes
    // into its own slice (its V reads are done: LDS is in order per wave), so
    // one barrier is enough.
    asm volatile("" ::: "memory");
    float* oslice = (float*)slice;
    #pragma unroll
    for (int db = 0; db < DBLK; ++db)
        #pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = db * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
            oslice[d * GTILE + l31] = o_acc[db][r];
        }
    if (lhi == 0) {
        lds_ml[wid][0][l31] = m_run;
        lds_ml[wid][1][l31] = l_run;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

    // thread t finishes row t & 31, d in [dg * D / 8, (dg + 1) * D / 8)
    const int orow = tile * GTILE + (threadIdx.x & 31);
    if (orow >= R) return;
    const int dg = threadIdx.x >> 5;
    float mw[GWAVES], m = MASK_VALUE_F;
    #pragma unroll
    for (int w = 0; w < GWAVES; ++w) {
        mw[w] = lds_ml[w][0][threadIdx.x & 31];
        m = fmaxf(m, mw[w]);
    }
    float aw[GWAVES], l = 0.f;
    #pragma unroll
    for (int w = 0; w < GWAVES; ++w) {
        aw[w] = __builtin_amdgcn_exp2f(mw[w] - m);
        l += aw[w] * lds_ml[w][1][threadIdx.x & 31];
    }
    // a row that saw no key in this chunk: l == 0, every O is 0 -> out = 0
    const float inv = 1.f / fmaxf(l, 1e-38f);
    const int og = orow / p.nq, oiq = orow % p.nq;
    const long rows_all = (long)p.b * p.h * p.nq;
    const long slot = (long)chunk * rows_all + ((long)b * p.h + hk + og * p.hk) * p.nq + oiq;
    float* op = p.out + slot * D + dg * (D / 8);
    #pragma unroll
    for (int d4 = 0; d4 < D / 8; d4 += 4) {
        f32x4 o4;
        #pragma unroll
        for (int e = 0; e < 4; ++e) {
            float acc = 0.f;
            #pragma unroll
            for (int w = 0; w < GWAVES; ++w)
                acc += aw[w] * ((const float*)(lds_v + w * SLICE))
                                   [(dg * (D / 8) + d4 + e) * GTILE + (threadIdx.x & 31)];
            o4[e] = acc * inv;
        }
        *(f32x4*)(op + d4) = o4;
    }
    if (dg == 0) p.lse[slot] = l > 0.f ? __logf(l) + m * LN2 : MASK_VALUE_F;
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

long paged_grouped_chunks(const PagedGroupedDecodeParams& p) {
    const long tiles = ((long)(p.h / p.hk) * p.nq + GTILE - 1) / GTILE;
    // with a window the longest workgroup span drives the split: window + 1
    // keys, nq - 1 more over the rows, up to GPASS - 1 of alignment in front
    const long span = p.has_window ? std::min(p.max_seq_len, p.window + p.nq + GPASS - 1)
                                   : p.max_seq_len;
    return p.chunks > 0 ? p.chunks
                        : decode_default_chunks(span, GWAVES * p.b * p.hk * tiles);
}

void launch_decode_partial_paged_grouped(const PagedGroupedDecodeParams& p, int head_dim,
                                         bool fp8, hipStream_t stream) {
    const long tiles = ((long)(p.h / p.hk) * p.nq + GTILE - 1) / GTILE;
    dim3 grid((unsigned)(p.b * p.hk * tiles), (unsigned)paged_grouped_chunks(p));
    dim3 block(GWAVES * 64);
    // the window and the clamp are template switches: the instantiations
    // without them keep the code they had before either existed
#define LAUNCH_GROUPED_W(D_, FP8_, WIN_)                                                \
    do {                                                                                \
        if (p.softclamp)                                                                \
            hipLaunchKernelGGL((decode_partial_paged_grouped_kernel<D_, FP8_, WIN_, true>),  \
                               grid, block, 0, stream, p);                              \
        else                                                                            \
            hipLaunchKernelGGL((decode_partial_paged_grouped_kernel<D_, FP8_, WIN_, false>), \
                               grid, block, 0, stream, p);                              \
    } while (0)
#define LAUNCH_GROUPED(D_, FP8_)                                                        \
    do {                                                                                \
        if (p.has_window) LAUNCH_GROUPED_W(D_, FP8_, true);                             \
        else LAUNCH_GROUPED_W(D_, FP8_, false);                                         \
    } while (0)
    if (head_dim == 64 && !fp8)
        LAUNCH_GROUPED(64, false);
    else if (head_dim == 128 && !fp8)
        LAUNCH_GROUPED(128, false);
    else if (head_dim == 64)
        LAUNCH_GROUPED(64, true);
    else if (head_dim == 128)
        LAUNCH_GROUPED(128, true);
    else
        __builtin_trap();
#undef LAUNCH_GROUPED
#undef LAUNCH_GROUPED_W
}

}  // namespace ring_attn
