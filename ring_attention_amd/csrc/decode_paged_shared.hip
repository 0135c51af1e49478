// Shared-prefix paged decode: sequences whose block tables start with the
// same pages (PagedKVCache.share_prefix) stream those pages ONCE per kv head,
// for the rows of all of them, and up to two 32-row tiles share that stream
// inside one workgroup.
//
// decode_paged_grouped.hip stacks the G * nq rows of one (sequence, kv head)
// into 32-row tiles and reads K/V once per tile, but a batch of b sequences
// behind one prefix still reads the prefix b times.  Here the launch is a flat
// 1-D grid over a host-built table of WORK UNITS (tree_decode.py's
// plan_shared_units, from the cache's host mirrors; heaviest first), and a
// unit says whose rows meet which keys:
//   * a unit is PSU_INTS int32: kind, kv head, first row tile, tile count (1
//     or 2), key span [j_lo, j_hi), partial slot, member list (offset and
//     count into `members`), lower bound `lo` and the length `len`.
//   * rows: the members' rows are stacked as r = (m * G + g) * nq + iq (member
//     m, group-mate g, draft iq) and cut into 32-row tiles that run across
//     sequence boundaries.  Lane l's row resolves through the member list to
//     (b_m, q head hk + g * HK, iq): that is where its Q^T fragment comes from
//     and where its partial goes.  Rows past the last one run on row 0 and
//     are dropped in the epilogue.
//   * PREFIX unit: the members of one group over a span inside [0, P), P the
//     shared length.  Pages come from the FIRST member's table row (the others
//     hold the same ids there).  Every row sees every key, so only the open
//     arm runs, except in the block that holds j_hi: P is a multiple of the
//     page size, not of 32, and that block tests key < j_hi per element.
//   * SUFFIX unit: one sequence (a member list of one; rows g * nq + iq as in
//     decode_paged_grouped.hip) over a span inside [lo, len), lo = its shared
//     length P_s, or 0 for a sequence outside any group.  The spans of a
//     sequence are cut from lo & ~127, so blocks stay 32-aligned and passes
//     128-aligned; a wave drops the blocks that end at or below lo, and a
//     block that straddles lo masks key < lo per element: the mechanism of
//     decode_paged_grouped.hip's window with lo_min.  With tree_bits the last
//     nq keys are the drafts (P0 = len - nq, host-checked lo <= P0) and the
//     mask acts there as in that kernel.
//   * two tiles: a unit may hold two consecutive tiles of one kv head and
//     span.  Per 32-key block a wave loads its K fragment once (global memory
//     straight into the MFMA operand, fp8 converted once), stages its V block
//     once into its swizzled, double-buffered LDS slice and reads it back
//     once with ds_read_b64_tr_b16, then runs scores, mask, softmax, P pack
//     and PV for each tile: decode_grouped.hip's scheme under the paged
//     address rule.  With TILES == 2 the Q^T fragments come from a swizzled
//     LDS image written once by the workgroup (no registers to hold them).
//   * the per-tile arithmetic is decode_paged_grouped.hip's, step by step:
//     S^T = K Q^T with v_mfma_f32_32x32x16_bf16, exp2 softmax with one
//     permlane32 swap per reduction, l summed from the unrounded exponentials,
//     P packed in score-register order, fp8 bytes converted at the point of
//     use, wave-uniform page ids fetched one block ahead, SOFTCLAMP as a
//     template switch.
//   * bounds: a table entry is read only for a key below j_hi (the host keeps
//     j_hi <= len <= max_pages * page_size), an id outside the pool is never
//     dereferenced, and rows at or beyond j_hi are zero-filled without forming
//     an address.
// The partial contract is decode_paged.hip's (out fp32 (S,B,HQ,NQ,D), lse fp32
// (S,B,HQ,NQ,1)); the unit's slot is its S index.  Not every (slot, row) has a
// unit: the binding fills the partials with out = 0, lse = MASK_VALUE_F first,
// so decode_merge and the cross-rank merge are reused unchanged.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

#include "attn_common.h"

// Packed f32 ops are off for every function of this file, for the reason and
// under the rule given in decode_paged_grouped.hip: nothing here calls a HIP
// header function that is not always_inline.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace ring_attn {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int SH_WAVES = 4;                     // waves per workgroup
constexpr int SH_TILE = 32;                     // rows per tile and keys per block
constexpr int SH_PASS = SH_WAVES * SH_TILE;     // keys a workgroup consumes per pass

// 8 e4m3 bytes x 2^(sbyte - 127) -> 8 bf16 (decode_paged_grouped.hip's rule)
__device__ __forceinline__ u32x4 sh_dequant_e4m3x8(u32x2 raw, unsigned sbyte) {
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
template <bool FP8> struct SharedChunk;
template <> struct SharedChunk<false> {
    u32x4 v;
    __device__ __forceinline__ u32x4 bf16_bits() const { return v; }
};
template <> struct SharedChunk<true> {
    u32x2 raw;
    unsigned sbyte;
    __device__ __forceinline__ u32x4 bf16_bits() const { return sh_dequant_e4m3x8(raw, sbyte); }
};

template <int D, bool FP8>
__device__ __forceinline__ SharedChunk<FP8> shared_pool_chunk(
        const void* pool, const void* scales, long row, int e0) {
    if constexpr (!FP8) {
        return {*(const u32x4*)((const __bf16*)pool + row * D + e0)};
    } else {
        return {*(const u32x2*)((const unsigned char*)pool + row * D + e0),
                ((const unsigned char*)scales)[row]};
    }
}

}  // namespace

template <int D, bool FP8, int TILES, bool SOFTCLAMP>
__global__ __launch_bounds__(SH_WAVES * 64)
// d 64, two tiles: fits 2 waves per SIMD when asked to (no scratch); the other
// instantiations keep the allocator's own choice
__attribute__((amdgpu_waves_per_eu(D == 64 && TILES == 2 ? 2 : 1)))
void decode_partial_paged_shared_kernel(PagedSharedDecodeParams p) {
    static_assert(D == 64 || D == 128);
    static_assert(TILES == 1 || TILES == 2);
    constexpr int KSTEPS = D / 16;              // QK^T k-steps
    constexpr int DBLK = D / 32;                // 32-d output blocks
    constexpr int CH = D / 8;                   // 16-byte chunks per row
    constexpr int VREGS = SH_TILE * CH / 64;    // V chunks per lane (== KSTEPS)
    constexpr int SLICE = 2 * SH_TILE * D;      // bf16 elements of one wave's slice
    constexpr bool QLDS = TILES > 1;            // Q^T fragments from an LDS image
    // V^T fragments read once per block and held for both tiles; d 128 has no
    // registers for that and re-reads them per tile
    constexpr bool VHOLD = !(D == 128 && TILES > 1);
    constexpr int QLDS_ELEMS = QLDS ? TILES * SH_TILE * D : 8;

    // a wave's slice holds its two V buffers in the loop and one tile's fp32
    // O^T (D x 32 floats, the same 128 * D bytes) in the epilogue
    __shared__ __align__(16) __bf16 lds_v[SH_WAVES * SLICE];
    __shared__ __align__(16) __bf16 lds_q[QLDS_ELEMS];
    __shared__ float lds_ml[SH_WAVES][2][SH_TILE];

    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31;
    const int lhi = lane >> 5;

    // ---- the unit (wave-uniform)
    const int* unit = p.units + (long)blockIdx.x * PSU_INTS;
    auto field = [&](int f) { return __builtin_amdgcn_readfirstlane(unit[f]); };
    const bool prefix = field(PSU_KIND) == PSU_PREFIX;
    const int hk = field(PSU_HK);
    const int tile0 = field(PSU_TILE0);
    const int ntile = TILES == 1 ? 1 : field(PSU_NTILE);
    const long j_lo = field(PSU_JLO);
    const long j_hi = field(PSU_JHI);
    const int slot_s = field(PSU_SLOT);
    const int* members = p.members + field(PSU_MEM0);
    const int nmem = field(PSU_NMEM);
    const long lo = field(PSU_LO);
    const long len = field(PSU_LEN);

    // keys below P0 are visible to every row; nt drafts follow.  A prefix unit
    // has no drafts and ends its open range at j_hi.
    const long P0 = prefix ? j_hi : (p.tree_bits ? len - p.nq : len);
    const int nt = prefix ? 0 : (int)(len - P0);
    const int tl = (int)(lo - P0);              // the rows' lower bound as a draft index

    // ---- the rows of the tiles: q fragments and mask words
    const int G = p.h / p.hk;
    const int GN = G * p.nq;
    const int R = nmem * GN;
    auto q_row = [&](int row) {
        const int row_c = row < R ? row : 0;
        const int m = row_c / GN, rem = row_c % GN;
        const int g = rem / p.nq, iq = rem % p.nq;
        return ((long)members[m] * p.h + hk + g * p.hk) * p.nq + iq;
    };
    bf16x8 qf[QLDS ? 1 : KSTEPS];
    unsigned long long bits[TILES];
    #pragma unroll
    for (int t = 0; t < TILES; ++t) {
        const long qr = q_row((tile0 + t) * SH_TILE + l31);
        if constexpr (!QLDS) {
            #pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks)
                qf[ks] = *(const bf16x8*)((const __bf16*)p.q + qr * D + ks * 16 + lhi * 8);
        }
        bits[t] = 0;
        if (p.tree_bits) {
            const long hn = (long)p.h * p.nq;
            const int* tb = p.tree_bits + ((qr / hn) * p.nq + qr % p.nq) * 2;
            bits[t] = (unsigned long long)(unsigned)tb[0]
                      | ((unsigned long long)(unsigned)tb[1] << 32);
        }
    }
    if constexpr (QLDS) {
        // the workgroup's TILES * 32 q rows, row-major with the 16-byte chunk
        // index XORed by row & 7; written once, read once per (block, tile)
        #pragma unroll
        for (int c = 0; c < TILES * CH / 8; ++c) {
            const int idx = threadIdx.x + c * (SH_WAVES * 64);
            const int lr = idx / CH, ch = idx % CH;
            const long qr = q_row(tile0 * SH_TILE + lr);
            *(u32x4*)(lds_q + lr * D + ((ch ^ (lr & 7)) * 8))
                = *(const u32x4*)((const __bf16*)p.q + qr * D + ch * 8);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }

    float m_run[TILES], l_run[TILES];
    f32x16 o_acc[TILES][DBLK];
    #pragma unroll
    for (int t = 0; t < TILES; ++t) {
        m_run[t] = MASK_VALUE_F;
        l_run[t] = 0.f;
        #pragma unroll
        for (int db = 0; db < DBLK; ++db) o_acc[t][db] = f32x16{};
    }

    // ---- staging
    using Chunk = SharedChunk<FP8>;
    Chunk kst[KSTEPS], vst[VREGS];
    const int shift = p.page_shift;
    const long pmask = (1L << shift) - 1;
    const int* bt = p.block_table
                    + (long)__builtin_amdgcn_readfirstlane(members[0]) * p.max_pages;
    const long head_rows = (long)hk << shift;
    const long page_rows = (long)p.hk << shift;
    const int vrow0 = lane / CH, ve0 = (lane % CH) * 8;     // V chunk r: row vrow0 + r * (64 / CH)
    __bf16* slice = lds_v + wid * SLICE;

    // ids of the pages that hold keys [j0, j0 + 16) and [j0 + 16, j0 + 32)
    int pg_a = -1, pg_b = -1;
    auto table_id = [&](long j) { return j < j_hi ? bt[j >> shift] : -1; };
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
            kst[ks] = ok ? shared_pool_chunk<D, FP8>(p.k_pages, p.kscale, krow, ks * 16 + lhi * 8)
                         : Chunk{};
        #pragma unroll
        for (int r = 0; r < VREGS; ++r) {
            const long vrow = pool_row(j0 + vrow0 + r * (64 / CH), ok);
            vst[r] = ok ? shared_pool_chunk<D, FP8>(p.v_pages, p.vscale, vrow, ve0) : Chunk{};
        }
    };
    auto write_v = [&](int par) {
        #pragma unroll
        for (int r = 0; r < VREGS; ++r) {
            const int vr = vrow0 + r * (64 / CH);
            *(u32x4*)(slice + par * SH_TILE * D + vr * D + ((ve0 / 8) ^ (vr & 7)) * 8)
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
    long j0 = j_lo + wid * SH_TILE;
    // lo < (lo & ~127) + SH_PASS: only a span's first pass holds blocks below lo
    if (j0 + SH_TILE <= lo) j0 += SH_PASS;
    if (j0 < j_hi) {
        load_block(j0, table_id(j0), table_id(j0 + 16));
        pg_a = table_id(j0 + SH_PASS);
        pg_b = table_id(j0 + SH_PASS + 16);
        write_v(0);
    }
    for (int par = 0; j0 < j_hi; j0 += SH_PASS, par ^= 1) {
        // this block's K fragments leave the staging registers (fp8: as bf16),
        // which then take the next block's loads
        union { u32x4 u; bf16x8 v; } kf[KSTEPS];
        #pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) kf[ks].u = kst[ks].bf16_bits();
        const bool more = j0 + SH_PASS < j_hi;
        if (more) {
            load_block(j0 + SH_PASS, pg_a, pg_b);
            pg_a = table_id(j0 + 2 * SH_PASS);
            pg_b = table_id(j0 + 2 * SH_PASS + 16);
        }

        // this block's V^T fragments: vf[db][ks] is the A fragment of d block
        // db, keys 16 * ks + 4 * lhi + {0..3, 8..11}
        const __bf16* vbuf = slice + par * SH_TILE * D;
        auto read_vf = [&](int db, int ks) {
            const bf16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                (lds_v4)(vbuf + (16 * ks) * D + tr_off[db]));
            const bf16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                (lds_v4)(vbuf + (16 * ks + 8) * D + tr_off[db]));
            return (bf16x8)__builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
        };
        bf16x8 vf[VHOLD ? DBLK : 1][2];
        if constexpr (VHOLD) {
            #pragma unroll
            for (int db = 0; db < DBLK; ++db)
                #pragma unroll
                for (int ks = 0; ks < 2; ++ks) vf[db][ks] = read_vf(db, ks);
        }

        // a block inside [lo, P0) is visible to every row and keeps raw scores
        // (the scale folds into the exp argument); clamped scores are final in
        // either arm
        const bool open_block = j0 + SH_TILE <= P0 && j0 >= lo;
        const int t0 = (int)(j0 - P0) + 4 * lhi;    // draft index of reg 0's key
        const float escale = (open_block && !SOFTCLAMP) ? scale2 : 1.f;

        #pragma unroll
        for (int t = 0; t < TILES; ++t) {
            if (t >= ntile) break;
            // ---- S^T[kv][row] of tile t
            f32x16 s = f32x16{};
            #pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) {
                bf16x8 qv;
                if constexpr (QLDS) {
                    const int lr = t * SH_TILE + l31;
                    qv = *(const bf16x8*)(lds_q + lr * D + (((2 * ks + lhi) ^ (l31 & 7)) * 8));
                } else {
                    qv = qf[ks];
                }
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks].v, qv, s, 0, 0, 0);
            }

            // ---- scale, mask
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
                const unsigned long long bt_row = bits[t];
                #pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int td = t0 + (r & 3) + 8 * (r >> 2);
                    const bool ok = td >= tl
                                    && (td < 0 || (td < nt && ((bt_row >> (td & 63)) & 1)));
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

            // ---- online softmax (the forward's: exact skip of the rescale
            // when no row's max grew; an all-masked row keeps its exps at 0
            // through the clamped subtrahend)
            const float m_new = fmaxf(m_run[t], smax);
            const bool any_growth = __builtin_amdgcn_ballot_w64(smax > m_run[t]) != 0;
            const float m_exp = fmaxf(m_new, -1.7e38f);
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
                const float alpha = __builtin_amdgcn_exp2f(m_run[t] - m_new);
                l_run[t] = l_run[t] * alpha + rowsum;
                #pragma unroll
                for (int db = 0; db < DBLK; ++db)
                    #pragma unroll
                    for (int r = 0; r < 16; ++r) o_acc[t][db][r] *= alpha;
                m_run[t] = m_new;
            } else {
                l_run[t] += rowsum;
            }

            // ---- O^T[d][row] += V^T[d][kv] P^T[kv][row]; pk[4 * ks .. + 3] is
            // the B fragment of k-step ks
            #pragma unroll
            for (int db = 0; db < DBLK; ++db)
                #pragma unroll
                for (int ks = 0; ks < 2; ++ks)
                    o_acc[t][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        VHOLD ? vf[VHOLD ? db : 0][ks] : read_vf(db, ks),
                        *(const bf16x8*)(pk + 4 * ks), o_acc[t][db], 0, 0, 0);
        }

        if (more) write_v(par ^ 1);
    }

    // ---- epilogue, tile by tile: the four waves' states meet in LDS.  A
    // wave's O^T goes into its own slice (its V reads are done: LDS is in
    // order per wave), so one barrier is enough before the combine; the one at
    // the top of the next round keeps that round's writes behind these reads.
    asm volatile("" ::: "memory");
    float* oslice = (float*)slice;
    const int dg = threadIdx.x >> 5;
    #pragma unroll
    for (int t = 0; t < TILES; ++t) {
        if (t >= ntile) break;
        if (t > 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        #pragma unroll
        for (int db = 0; db < DBLK; ++db)
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int d = db * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                oslice[d * SH_TILE + l31] = o_acc[t][db][r];
            }
        if (lhi == 0) {
            lds_ml[wid][0][l31] = m_run[t];
            lds_ml[wid][1][l31] = l_run[t];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

        // thread x finishes row x & 31, d in [dg * D / 8, (dg + 1) * D / 8)
        const int orow = (tile0 + t) * SH_TILE + (threadIdx.x & 31);
        if (orow < R) {
            float mw[SH_WAVES], m = MASK_VALUE_F;
            #pragma unroll
            for (int w = 0; w < SH_WAVES; ++w) {
                mw[w] = lds_ml[w][0][threadIdx.x & 31];
                m = fmaxf(m, mw[w]);
            }
            float aw[SH_WAVES], l = 0.f;
            #pragma unroll
            for (int w = 0; w < SH_WAVES; ++w) {
                aw[w] = __builtin_amdgcn_exp2f(mw[w] - m);
                l += aw[w] * lds_ml[w][1][threadIdx.x & 31];
            }
            // a row that saw no key in this span: l == 0, every O is 0 -> out = 0
            const float inv = 1.f / fmaxf(l, 1e-38f);
            const long rows_all = (long)p.b * p.h * p.nq;
            const long slot = (long)slot_s * rows_all + q_row(orow);
            float* op = p.out + slot * D + dg * (D / 8);
            #pragma unroll
            for (int d4 = 0; d4 < D / 8; d4 += 4) {
                f32x4 o4;
                #pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float acc = 0.f;
                    #pragma unroll
                    for (int w = 0; w < SH_WAVES; ++w)
                        acc += aw[w] * ((const float*)(lds_v + w * SLICE))
                                           [(dg * (D / 8) + d4 + e) * SH_TILE + (threadIdx.x & 31)];
                    o4[e] = acc * inv;
                }
                *(f32x4*)(op + d4) = o4;
            }
            if (dg == 0) p.lse[slot] = l > 0.f ? __logf(l) + m * LN2 : MASK_VALUE_F;
        }
    }
}

// Holes of the partials: a (slot, row) without a unit reads out = 0 and
// lse = MASK_VALUE_F in the merge.  One thread per 16 bytes of out.
__global__ __launch_bounds__(256)
void paged_shared_fill_kernel(float* out, float* lse, long out_vec4, long lse_n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < out_vec4) ((f32x4*)out)[i] = f32x4{};
    if (i < lse_n) lse[i] = MASK_VALUE_F;
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// Most row tiles a unit may hold: two share one K/V stream at either head dim
int paged_shared_unit_tiles(int head_dim) {
    (void)head_dim;
    return 2;
}

void launch_decode_partial_paged_shared(const PagedSharedDecodeParams& p, int head_dim,
                                        bool fp8, hipStream_t stream) {
    // every slot first reads as "saw no key"; the units then write theirs
    const long rows = (long)p.n_slots * p.b * p.h * p.nq;
    const long vec4 = rows * head_dim / 4;
    hipLaunchKernelGGL(paged_shared_fill_kernel, dim3((unsigned)((vec4 + 255) / 256)),
                       dim3(256), 0, stream, p.out, p.lse, vec4, rows);
    if (p.n_units == 0) return;
    dim3 grid((unsigned)p.n_units);
    dim3 block(SH_WAVES * 64);
    // the two-tile variant runs only when some unit holds two tiles
#define LAUNCH_SH(D_, FP8_, T_)                                                         \
    do {                                                                                \
        if (p.softclamp)                                                                \
            hipLaunchKernelGGL((decode_partial_paged_shared_kernel<D_, FP8_, T_, true>),  \
                               grid, block, 0, stream, p);                              \
        else                                                                            \
            hipLaunchKernelGGL((decode_partial_paged_shared_kernel<D_, FP8_, T_, false>), \
                               grid, block, 0, stream, p);                              \
    } while (0)
#define LAUNCH_SH_FP8(D_, T_)                                                           \
    do { if (fp8) LAUNCH_SH(D_, true, T_); else LAUNCH_SH(D_, false, T_); } while (0)
    if (head_dim == 64 && p.unit_tiles == 1) LAUNCH_SH_FP8(64, 1);
    else if (head_dim == 64 && p.unit_tiles == 2) LAUNCH_SH_FP8(64, 2);
    else if (head_dim == 128 && p.unit_tiles == 1) LAUNCH_SH_FP8(128, 1);
    else if (head_dim == 128 && p.unit_tiles == 2) LAUNCH_SH_FP8(128, 2);
    else __builtin_trap();
#undef LAUNCH_SH_FP8
#undef LAUNCH_SH
}

}  // namespace ring_attn
