// Grouped decode over the DENSE KV cache: all (group-mate, draft) rows of one
// kv head share one pass over K/V, on the matrix cores, with a token-tree
// mask, and up to TILES 32-row tiles share that pass inside one workgroup.
//
// decode.hip runs one wave per (b, q head, query token) and every wave streams
// K/V for itself.  Here the R = G * nq rows of a (b, kv head) are stacked into
// T = ceil(R / 32) tiles (row r = g * nq + iq is q head hk + g * HK, draft iq),
// as in decode_paged_grouped.hip, whose per-tile arithmetic this file repeats
// step by step (scores, mask, softmax, P pack, PV).  What differs:
//   * layouts are decode.hip's: q (B, HQ, NQ, D) bf16, k / v (B, HK, N, D)
//     bf16 or e4m3 bytes with e8m0 row scales (B, HK, N).  A key row's address
//     is ((b * HK + hk) * N + j) * D: no table, no page, one length N.
//   * grid (B * HK * ceil(T / TILES), S); a workgroup is 4 waves and owns up to
//     TILES consecutive tiles of ONE kv head and one 128-key-aligned kv chunk.
//     Its waves take the chunk's 32-key blocks round-robin, so a key row is
//     consumed by exactly one wave of one workgroup per TILES tiles: K needs no
//     LDS and the loop has no workgroup barrier.
//   * per 32-key block a wave loads its K fragment once (global memory straight
//     into the MFMA operand, fp8 converted once), stages its V block once into
//     its swizzled, double-buffered LDS slice and reads it back once with
//     ds_read_b64_tr_b16 into registers (d 128 with TILES > 1 has no registers
//     to hold the fragments and re-reads them per tile); then it loops over
//     its tiles: scores for tile t, mask, tile t's own (m, l) update, P pack,
//     PV MFMAs into tile t's accumulators.  The global K/V traffic does not
//     grow with TILES; the MFMA and softmax work per tile is the paged
//     kernel's.
//   * registers: O is 32 * TILES (d 64) / 64 * TILES (d 128) accumulators per
//     lane.  The Q^T fragments (16 * TILES / 32 * TILES VGPRs) stay in
//     registers for TILES == 1, as in the paged kernel; for TILES > 1 they live
//     in a swizzled LDS image written once by the workgroup and read once per
//     (block, tile), which keeps every instantiation free of scratch.
//   * epilogue, tile by tile: each wave writes that tile's O^T into its own
//     slice, one barrier follows, 256 threads combine the four wave states and
//     write the partial; a second barrier separates the reads from the next
//     tile's writes.
//   * mask: with tree_bits the last nq keys are the drafts' own tokens; key
//     P0 + t (P0 = N - nq) is visible to draft iq iff bit t of
//     tree_bits[b][iq] is set, keys below P0 to every row.  Blocks that end at
//     or below P0 take the open arm.  Without tree_bits P0 = N.  Keys at or
//     beyond the chunk's end are zero-filled without forming an address.
//   * SOFTCLAMP: decode_paged_grouped.hip's, per tile: x = c * log2e *
//     tanh(s * scale / c) in both arms, max on x, exp2(x - m).
// No window, no kv_after: a dense cache can be sliced by the caller.
// The partial contract is decode.hip's (out fp32 (S,B,HQ,NQ,D), lse fp32
// (S,B,HQ,NQ,1), out = 0 and lse = MASK_VALUE_F where a row saw no key), so
// decode_merge and the cross-rank merge are reused unchanged.

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

constexpr int DG_WAVES = 4;                     // waves per workgroup
constexpr int DG_TILE = 32;                     // rows per tile and keys per block
constexpr int DG_PASS = DG_WAVES * DG_TILE;     // keys a workgroup consumes per pass

// 8 e4m3 bytes x 2^(sbyte - 127) -> 8 bf16 (decode_paged_grouped.hip's rule)
__device__ __forceinline__ u32x4 dg_dequant_e4m3x8(u32x2 raw, unsigned sbyte) {
    const float sc = __builtin_bit_cast(float, sbyte ? sbyte << 23 : 0x00400000u);
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(raw[0], false);
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8(raw[0], true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8(raw[1], false);
    const f32x2 d = __builtin_amdgcn_cvt_pk_f32_fp8(raw[1], true);
    return u32x4{pack_bf16x2(a[0] * sc, a[1] * sc), pack_bf16x2(b[0] * sc, b[1] * sc),
                 pack_bf16x2(c[0] * sc, c[1] * sc), pack_bf16x2(d[0] * sc, d[1] * sc)};
}

// 8 elements of one cache row as they wait in registers: bf16 bits, or raw
// e4m3 bytes plus the row's scale byte (converted at the point of use)
template <bool FP8> struct DenseChunk;
template <> struct DenseChunk<false> {
    u32x4 v;
    __device__ __forceinline__ u32x4 bf16_bits() const { return v; }
};
template <> struct DenseChunk<true> {
    u32x2 raw;
    unsigned sbyte;
    __device__ __forceinline__ u32x4 bf16_bits() const { return dg_dequant_e4m3x8(raw, sbyte); }
};

template <int D, bool FP8>
__device__ __forceinline__ DenseChunk<FP8> dense_chunk(const void* cache, const void* scales,
                                                       long row, int e0) {
    if constexpr (!FP8) {
        return {*(const u32x4*)((const __bf16*)cache + row * D + e0)};
    } else {
        return {*(const u32x2*)((const unsigned char*)cache + row * D + e0),
                ((const unsigned char*)scales)[row]};
    }
}

}  // namespace

template <int D, bool FP8, int TILES, bool SOFTCLAMP>
__global__ __launch_bounds__(DG_WAVES * 64)
// d 64, two tiles: fits 2 waves per SIMD when asked to (no scratch); the other
// instantiations keep the allocator's own choice
__attribute__((amdgpu_waves_per_eu(D == 64 && TILES == 2 ? 2 : 1)))
void decode_partial_grouped_kernel(GroupedDecodeParams p) {
    static_assert(D == 64 || D == 128);
    static_assert(TILES == 1 || TILES == 2 || TILES == 4);
    constexpr int KSTEPS = D / 16;              // QK^T k-steps
    constexpr int DBLK = D / 32;                // 32-d output blocks
    constexpr int CH = D / 8;                   // 16-byte chunks per row
    constexpr int VREGS = DG_TILE * CH / 64;    // V chunks per lane (== KSTEPS)
    constexpr int SLICE = 2 * DG_TILE * D;      // bf16 elements of one wave's slice
    constexpr bool QLDS = TILES > 1;            // Q^T fragments from an LDS image
    // V^T fragments read once per block and held for all tiles; d 128 with
    // more than one tile has no registers for that and re-reads them per tile
    constexpr bool VHOLD = !(D == 128 && TILES > 1);
    constexpr int QREG_TILES = QLDS ? 1 : TILES;
    constexpr int QLDS_ELEMS = QLDS ? TILES * DG_TILE * D : 8;

    // a wave's slice holds its two V buffers in the loop and one tile's fp32
    // O^T (D x 32 floats, the same 128 * D bytes) in the epilogue
    __shared__ __align__(16) __bf16 lds_v[DG_WAVES * SLICE];
    __shared__ __align__(16) __bf16 lds_q[QLDS_ELEMS];
    __shared__ float lds_ml[DG_WAVES][2][DG_TILE];

    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31;
    const int lhi = lane >> 5;

    // ---- which (b, kv head, tile group, chunk): chunk-major for b > 1, for
    // the reason given in decode_paged.hip
    const int G = p.h / p.hk;
    const int R = G * p.nq;
    const int tiles = (R + DG_TILE - 1) / DG_TILE;
    const int groups = (tiles + TILES - 1) / TILES;
    const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y;
    int rb = p.chunk_major ? (int)(lin / gridDim.y) : (int)blockIdx.x;
    const int chunk = p.chunk_major ? (int)(lin % gridDim.y) : (int)blockIdx.y;
    const int tile0 = (rb % groups) * TILES;  rb /= groups;
    const int ntile = min(TILES, tiles - tile0);    // tiles this workgroup owns
    const int hk = rb % p.hk;
    const int b = rb / p.hk;

    // ---- this chunk's share of [0, n) (wave-uniform)
    const long n = p.n;
    const long P0 = p.tree_bits ? n - p.nq : n;
    long per = (n + gridDim.y - 1) / gridDim.y;
    per = (per + DG_PASS - 1) & ~(long)(DG_PASS - 1);
    const long j_lo = (long)chunk * per;
    const long j_hi = min(n, j_lo + per);

    // ---- the rows of the tiles: q fragments and mask words.  Rows past R run
    // on row 0 and are dropped in the epilogue.
    auto q_row = [&](int row) {
        const int row_c = row < R ? row : 0;
        const int g = row_c / p.nq, iq = row_c % p.nq;
        return ((long)b * p.h + hk + g * p.hk) * p.nq + iq;
    };
    bf16x8 qf[QREG_TILES][KSTEPS];
    unsigned long long bits[TILES];
    #pragma unroll
    for (int t = 0; t < TILES; ++t) {
        const long qr = q_row((tile0 + t) * DG_TILE + l31);
        if constexpr (!QLDS) {
            #pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks)
                qf[t][ks] = *(const bf16x8*)((const __bf16*)p.q + qr * D + ks * 16 + lhi * 8);
        }
        bits[t] = 0;
        if (p.tree_bits) {
            const int* tb = p.tree_bits + ((long)b * p.nq + (int)(qr % p.nq)) * 2;
            bits[t] = (unsigned long long)(unsigned)tb[0]
                      | ((unsigned long long)(unsigned)tb[1] << 32);
        }
    }
    if constexpr (QLDS) {
        // the workgroup's TILES * 32 q rows, row-major with the 16-byte chunk
        // index XORed by row & 7; written once, read once per (block, tile)
        #pragma unroll
        for (int c = 0; c < TILES * CH / 8; ++c) {
            const int idx = threadIdx.x + c * (DG_WAVES * 64);
            const int lr = idx / CH, ch = idx % CH;
            const long qr = q_row(tile0 * DG_TILE + lr);
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
    using Chunk = DenseChunk<FP8>;
    Chunk kst[KSTEPS], vst[VREGS];
    const long head_row = ((long)b * p.hk + hk) * n;        // row of key 0
    const int vrow0 = lane / CH, ve0 = (lane % CH) * 8;     // V chunk r: row vrow0 + r * (64 / CH)
    __bf16* slice = lds_v + wid * SLICE;

    auto load_block = [&](long j0) {
        const bool kok = j0 + l31 < j_hi;
        #pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks)
            kst[ks] = kok ? dense_chunk<D, FP8>(p.k, p.kscale, head_row + j0 + l31,
                                                ks * 16 + lhi * 8)
                          : Chunk{};
        #pragma unroll
        for (int r = 0; r < VREGS; ++r) {
            const long j = j0 + vrow0 + r * (64 / CH);
            vst[r] = j < j_hi ? dense_chunk<D, FP8>(p.v, p.vscale, head_row + j, ve0) : Chunk{};
        }
    };
    auto write_v = [&](int par) {
        #pragma unroll
        for (int r = 0; r < VREGS; ++r) {
            const int vr = vrow0 + r * (64 / CH);
            *(u32x4*)(slice + par * DG_TILE * D + vr * D + ((ve0 / 8) ^ (vr & 7)) * 8)
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
    const int nt = (int)(n - P0);               // drafts cached (0 without a mask)
    long j0 = j_lo + wid * DG_TILE;
    if (j0 < j_hi) {
        load_block(j0);
        write_v(0);
    }
    for (int par = 0; j0 < j_hi; j0 += DG_PASS, par ^= 1) {
        // this block's K fragments leave the staging registers (fp8: as bf16),
        // which then take the next block's loads
        union { u32x4 u; bf16x8 v; } kf[KSTEPS];
        #pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) kf[ks].u = kst[ks].bf16_bits();
        const bool more = j0 + DG_PASS < j_hi;
        if (more) load_block(j0 + DG_PASS);

        // this block's V^T fragments: vf[db][ks] is the A fragment of d block
        // db, keys 16 * ks + 4 * lhi + {0..3, 8..11}
        const __bf16* vbuf = slice + par * DG_TILE * D;
        auto read_vf = [&](int db, int ks) {
            const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                (lds_v4)(vbuf + (16 * ks) * D + tr_off[db]));
            const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                (lds_v4)(vbuf + (16 * ks + 8) * D + tr_off[db]));
            return (bf16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        };
        bf16x8 vf[VHOLD ? DBLK : 1][2];
        if constexpr (VHOLD) {
            #pragma unroll
            for (int db = 0; db < DBLK; ++db)
                #pragma unroll
                for (int ks = 0; ks < 2; ++ks) vf[db][ks] = read_vf(db, ks);
        }

        // a block below P0 is visible to every row and keeps raw scores (the
        // scale folds into the exp argument); clamped scores are final in
        // either arm
        const bool open_block = j0 + DG_TILE <= P0;
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
                    const int lr = t * DG_TILE + l31;
                    qv = *(const bf16x8*)(lds_q + lr * D + (((2 * ks + lhi) ^ (l31 & 7)) * 8));
                } else {
                    qv = qf[t][ks];
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
                const unsigned long long bt = bits[t];
                #pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int td = t0 + (r & 3) + 8 * (r >> 2);
                    const bool ok = td < 0 || (td < nt && ((bt >> (td & 63)) & 1));
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
                oslice[d * DG_TILE + l31] = o_acc[t][db][r];
            }
        if (lhi == 0) {
            lds_ml[wid][0][l31] = m_run[t];
            lds_ml[wid][1][l31] = l_run[t];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

        // thread x finishes row x & 31, d in [dg * D / 8, (dg + 1) * D / 8)
        const int orow = (tile0 + t) * DG_TILE + (threadIdx.x & 31);
        if (orow < R) {
            float mw[DG_WAVES], m = MASK_VALUE_F;
            #pragma unroll
            for (int w = 0; w < DG_WAVES; ++w) {
                mw[w] = lds_ml[w][0][threadIdx.x & 31];
                m = fmaxf(m, mw[w]);
            }
            float aw[DG_WAVES], l = 0.f;
            #pragma unroll
            for (int w = 0; w < DG_WAVES; ++w) {
                aw[w] = __builtin_amdgcn_exp2f(mw[w] - m);
                l += aw[w] * lds_ml[w][1][threadIdx.x & 31];
            }
            // a row that saw no key in this chunk: l == 0, every O is 0 -> out = 0
            const float inv = 1.f / fmaxf(l, 1e-38f);
            const long rows_all = (long)p.b * p.h * p.nq;
            const long slot = (long)chunk * rows_all + q_row(orow);
            float* op = p.out + slot * D + dg * (D / 8);
            #pragma unroll
            for (int d4 = 0; d4 < D / 8; d4 += 4) {
                f32x4 o4;
                #pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float acc = 0.f;
                    #pragma unroll
                    for (int w = 0; w < DG_WAVES; ++w)
                        acc += aw[w] * ((const float*)(lds_v + w * SLICE))
                                           [(dg * (D / 8) + d4 + e) * DG_TILE + (threadIdx.x & 31)];
                    o4[e] = acc * inv;
                }
                *(f32x4*)(op + d4) = o4;
            }
            if (dg == 0) p.lse[slot] = l > 0.f ? __logf(l) + m * LN2 : MASK_VALUE_F;
        }
    }
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// Tiles per workgroup: the smallest built TILES that holds all T tiles of a
// kv head, else the largest, up to a limit.  The limit is 2 unless tiles_cap
// (RING_ATTN_GROUPED_TILES) sets another: at d 64 the 4-tile variant runs at
// one wave per SIMD and measured slower than one tile per workgroup
// (docs/KERNELS.md 3d), so it is reached only through the switch.
int grouped_decode_tiles(const GroupedDecodeParams& p, int head_dim) {
    const long tiles = ((long)(p.h / p.hk) * p.nq + DG_TILE - 1) / DG_TILE;
    const int largest = head_dim == 64 ? 4 : 2;
    const int limit = p.tiles_cap > 0 ? p.tiles_cap : 2;
    int t = 1;
    while (t < tiles && t < largest && 2 * t <= limit) t *= 2;
    return t;
}

long grouped_decode_chunks(const GroupedDecodeParams& p, int head_dim) {
    const long tiles = ((long)(p.h / p.hk) * p.nq + DG_TILE - 1) / DG_TILE;
    const long per_wg = grouped_decode_tiles(p, head_dim);
    const long groups = (tiles + per_wg - 1) / per_wg;
    return p.chunks > 0 ? p.chunks
                        : decode_default_chunks(p.n, DG_WAVES * p.b * p.hk * groups);
}

void launch_decode_partial_grouped(const GroupedDecodeParams& p, int head_dim, bool fp8,
                                   hipStream_t stream) {
    const long tiles = ((long)(p.h / p.hk) * p.nq + DG_TILE - 1) / DG_TILE;
    const int per_wg = grouped_decode_tiles(p, head_dim);
    const long groups = (tiles + per_wg - 1) / per_wg;
    dim3 grid((unsigned)(p.b * p.hk * groups), (unsigned)grouped_decode_chunks(p, head_dim));
    dim3 block(DG_WAVES * 64);
#define LAUNCH_DG(D_, FP8_, T_)                                                         \
    do {                                                                                \
        if (p.softclamp)                                                                \
            hipLaunchKernelGGL((decode_partial_grouped_kernel<D_, FP8_, T_, true>),     \
                               grid, block, 0, stream, p);                              \
        else                                                                            \
            hipLaunchKernelGGL((decode_partial_grouped_kernel<D_, FP8_, T_, false>),    \
                               grid, block, 0, stream, p);                              \
    } while (0)
#define LAUNCH_DG_FP8(D_, T_)                                                           \
    do { if (fp8) LAUNCH_DG(D_, true, T_); else LAUNCH_DG(D_, false, T_); } while (0)
    if (head_dim == 64 && per_wg == 1) LAUNCH_DG_FP8(64, 1);
    else if (head_dim == 64 && per_wg == 2) LAUNCH_DG_FP8(64, 2);
    else if (head_dim == 64 && per_wg == 4) LAUNCH_DG_FP8(64, 4);
    else if (head_dim == 128 && per_wg == 1) LAUNCH_DG_FP8(128, 1);
    else if (head_dim == 128 && per_wg == 2) LAUNCH_DG_FP8(128, 2);
    else __builtin_trap();
#undef LAUNCH_DG_FP8
#undef LAUNCH_DG
}

}  // namespace ring_attn
