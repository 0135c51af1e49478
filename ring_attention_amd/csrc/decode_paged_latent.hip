// MLA latent-cache paged decode: d_qk = 576 (512-d latent + 64-d rope part),
// d_v = 512, one pool row per token that is the key of EVERY query head and,
// in its first 512 columns, also the value.
//
// decode_paged_grouped.hip gives each wave its own 32-key blocks and keeps the
// whole O of a tile in that wave's registers; at d_v = 512 that is 256
// accumulators plus 144 fragment registers each for Q^T and K.  Here the four
// waves of a workgroup work on the SAME 32-key block and split it by column:
//   * rows: r = h * nq + iq of a sequence (one kv head), cut into 32-row
//     tiles; rows past R = H * nq run on row 0's q and are not written.
//   * grid (b * row tiles, S), chunk-major for b > 1; [0, len) is cut into S
//     128-key-aligned chunks, so a 32-key block straddles nothing but len.
//   * K image: the 32 x 576 bf16 block (nine 16-byte chunks per thread) is
//     loaded through the block table into staging registers ONE BLOCK AHEAD
//     and written row-major into LDS, chunk index XORed with row & 7.  Page
//     ids are wave-uniform table reads fetched one block before the load
//     (two per block for page_size 16, picked by bit masks); only entries
//     below ceil(len / page_size) are read, an id outside the pool is never
//     dereferenced, and rows at or past the chunk's end are zero-filled
//     without forming an address.
//   * scores: S^T = K Q^T is split over the REDUCTION dim: wave w owns
//     columns [144 w, 144 w + 144), 9 v_mfma_f32_32x32x16_bf16 per block with
//     16-byte LDS row reads as A fragments and 36 Q^T registers loaded once.
//     Each wave stores its partial 32 x 32 fp32 C fragment to LDS in lane /
//     register order; behind a barrier every wave sums the four partials in
//     one fixed order, so all waves hold bit-identical scores.
//   * softmax: every wave runs the same exp2-domain online softmax
//     redundantly (open and masked arms of the grouped kernel: a block that
//     ends at or below len - (nq - 1) is unmasked); (m, l) are identical in
//     all waves by construction, l is summed from the unrounded exponentials
//     and the skip of the rescale is exact.
//   * PV: wave w owns value columns [128 w, 128 w + 128): O^T[128][32] is 64
//     accumulators, 8 MFMAs per block.  P is packed to bf16 in score-register
//     order (kperm_pair's k order) and the V^T fragments are read with
//     ds_read_b64_tr_b16 from the SAME K image: V costs no second load and no
//     second LDS image.
//   * epilogue: a wave owns a disjoint column slice over all keys of the
//     chunk, so there is no cross-wave state to combine; it normalises and
//     writes its 128 columns.  An empty chunk or sequence writes out = 0,
//     lse = MASK_VALUE_F.
// 17 MFMAs per wave and block, against 44 if each wave recomputed the full
// 576-wide score tile.  LDS: one K image (36 864 B) + the partials (16 384 B)
// = 52 KB, single-buffered: the next block waits in the staging registers.
// Three barriers per block: image written | partials written | image and
// partials read.  They wait on LDS traffic only (lgkmcnt), never on the
// global prefetch in flight.
// The partial contract is decode_paged.hip's (out fp32 (S,B,H,NQ,512), lse
// fp32 (S,B,H,NQ,1)), so decode_merge<512> and the cross-rank merge apply.
//
// paged_latent_append_kernel writes new tokens into the pool: one wave per
// token, 72 16-byte chunks per row.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

#include "attn_common.h"

// Packed f32 ops off for the whole file, and no call to a HIP header function
// that is not always_inline (decode_paged_grouped.hip has the reasons).
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace ring_attn {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int LWAVES = 4;       // waves per workgroup
constexpr int LTILE = 32;       // rows per tile and keys per block
constexpr int LALIGN = 128;     // chunk alignment in keys

// workgroup barrier for LDS hand-offs: waits for this wave's LDS traffic
// only.  A workgroup-scope release fence would also drain vmcnt, and with it
// the next block's loads.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

}  // namespace

// Two waves per SIMD asked for: left alone the allocator spreads to 332
// registers (one wave per SIMD); held to 256 it needs no scratch.
template <int DK, int DV>
__global__ __launch_bounds__(LWAVES * 64) __attribute__((amdgpu_waves_per_eu(2)))
void decode_partial_latent_kernel(PagedLatentDecodeParams p) {
    static_assert(DK == 576 && DV == 512);
    constexpr int CH = DK / 8;                          // 16-byte chunks per row: 72
    constexpr int KREGS = LTILE * CH / (LWAVES * 64);   // chunks per thread: 9
    constexpr int KCOLS = DK / LWAVES;                  // reduction columns per wave: 144
    constexpr int KSTEPS = KCOLS / 16;                  // 9
    constexpr int VCOLS = DV / LWAVES;                  // value columns per wave: 128
    constexpr int DBLK = VCOLS / 32;                    // 4
    static_assert(KREGS * LWAVES * 64 == LTILE * CH && KSTEPS * 16 * LWAVES == DK);

    __shared__ __align__(16) __bf16 lds_k[LTILE * DK];
    __shared__ __align__(16) float lds_part[LWAVES * 4 * 64 * 4];

    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31;
    const int lhi = lane >> 5;

    // ---- which (b, row tile, chunk): chunk-major for b > 1, for the reason
    // given in decode_paged.hip
    const int R = p.h * p.nq;
    const int tiles = (R + LTILE - 1) / LTILE;
    const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y;
    const int rb = p.chunk_major ? (int)(lin / gridDim.y) : (int)blockIdx.x;
    const int chunk = p.chunk_major ? (int)(lin % gridDim.y) : (int)blockIdx.y;
    const int tile = rb % tiles;
    const int b = rb / tiles;

    // ---- the sequence's span and this chunk's share of it (wave-uniform)
    const int shift = p.page_shift;
    const long pmask = (1L << shift) - 1;
    const long len = min(max((long)__builtin_amdgcn_readfirstlane(p.seq_lens[b]), 0L),
                         (long)p.max_pages << shift);
    long per = (len + gridDim.y - 1) / gridDim.y;
    per = (per + LALIGN - 1) & ~(long)(LALIGN - 1);
    const long j_lo = (long)chunk * per;
    const long j_hi = min(len, j_lo + per);
    // blocks that end at or below `open_to` are visible to every row
    const long open_to = p.causal ? len - (p.nq - 1) : len;

    // ---- this lane's row: its slice of q and its key limit
    const int row = tile * LTILE + l31;
    const int row_c = row < R ? row : 0;
    const int iq = row_c % p.nq;
    const long limit = p.causal ? max(len - (p.nq - 1 - iq), 0L) : len;
    const __bf16* qrow = (const __bf16*)p.q + ((long)b * R + row_c) * DK + wid * KCOLS;
    bf16x8 qf[KSTEPS];
    #pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) qf[ks] = *(const bf16x8*)(qrow + ks * 16 + lhi * 8);

    float m_run = MASK_VALUE_F;
    float l_run = 0.f;
    f32x16 o_acc[DBLK];
    #pragma unroll
    for (int db = 0; db < DBLK; ++db) o_acc[db] = f32x16{};

    // ---- staging: thread x carries chunks x, x + 256, ... of the block, so a
    // wave's 64 loads cover 1 KB of consecutive row bytes
    u32x4 kst[KREGS];
    const int* bt = p.block_table + (long)b * p.max_pages;
    const __bf16* pool = (const __bf16*)p.pages;
    // ids of the pages that hold keys [j0, j0 + 16) and [j0 + 16, j0 + 32)
    int pg_a = -1, pg_b = -1;
    auto table_id = [&](long j) { return j < j_hi ? bt[j >> shift] : -1; };
    auto load_block = [&](long j0, int id_a, int id_b) {
        #pragma unroll
        for (int i = 0; i < KREGS; ++i) {
            const int c = (int)threadIdx.x + i * (LWAVES * 64);
            const int kr = c / CH, ch = c - kr * CH;
            const long j = j0 + kr;
            // bit select: written as ?: the two ids become a table in scratch
            const int second = -(kr >> 4);
            const int pg = (id_a & ~second) | (id_b & second);
            const bool ok = j < j_hi && (unsigned)pg < (unsigned)p.num_pages;
            const long prow = ((long)pg << shift) + (j & pmask);
            kst[i] = ok ? *(const u32x4*)(pool + prow * DK + ch * 8) : u32x4{};
        }
    };
    auto write_block = [&]() {
        #pragma unroll
        for (int i = 0; i < KREGS; ++i) {
            const int c = (int)threadIdx.x + i * (LWAVES * 64);
            const int kr = c / CH, ch = c - kr * CH;
            *(u32x4*)(lds_k + kr * DK + (ch ^ (kr & 7)) * 8) = kst[i];
        }
    };

    // A fragments of the scores: key row l31, 16-byte chunk 18 w + 2 ks + lhi
    const __bf16* arow = lds_k + l31 * DK;
    const int achunk0 = wid * (KCOLS / 8) + lhi;
    const int aswz = l31 & 7;

    // transposed V reads (KERNELS.md "ds_read_b64_tr_b16"): lane f = lane & 15
    // of 16-lane group g16 addresses row 4 * lhi + (f >> 2) (+ 16 * half + 8 * u),
    // columns 128 w + db * 32 + 16 * g16 + 4 * (f & 3) .. + 4
    typedef __attribute__((address_space(3))) bf16x4* lds_v4;
    const int f15 = lane & 15, g16 = (lane >> 4) & 1;
    const int trow = 4 * lhi + (f15 >> 2);
    int tr_off[DBLK];
    #pragma unroll
    for (int db = 0; db < DBLK; ++db) {
        const int col = wid * VCOLS + db * 32 + 16 * g16 + 4 * (f15 & 3);
        tr_off[db] = trow * DK + ((col / 8) ^ (trow & 7)) * 8 + (col % 8);
    }

    f32x4* part = (f32x4*)lds_part;
    const float scale2 = p.scale * LOG2E;

    if (j_lo < j_hi) {
        load_block(j_lo, table_id(j_lo), table_id(j_lo + 16));
        pg_a = table_id(j_lo + LTILE);
        pg_b = table_id(j_lo + LTILE + 16);
    }
    for (long j0 = j_lo; j0 < j_hi; j0 += LTILE) {
        // ---- this block becomes the LDS image; the staging registers take
        // the next block's loads
        write_block();
        lds_barrier();
        if (j0 + LTILE < j_hi) {
            load_block(j0 + LTILE, pg_a, pg_b);
            pg_a = table_id(j0 + 2 * LTILE);
            pg_b = table_id(j0 + 2 * LTILE + 16);
        }

        // ---- partial S^T[kv][row] over this wave's 144 columns
        f32x16 s = f32x16{};
        #pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const bf16x8 kf = *(const bf16x8*)(arow + ((achunk0 + 2 * ks) ^ aswz) * 8);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
        }
        #pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
            part[(wid * 4 + r4) * 64 + lane]
                = f32x4{s[4 * r4], s[4 * r4 + 1], s[4 * r4 + 2], s[4 * r4 + 3]};
        lds_barrier();
        // every wave sums the four partials in the same order
        #pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const f32x4 a = part[(0 * 4 + r4) * 64 + lane];
            const f32x4 c = part[(1 * 4 + r4) * 64 + lane];
            const f32x4 e = part[(2 * 4 + r4) * 64 + lane];
            const f32x4 g = part[(3 * 4 + r4) * 64 + lane];
            #pragma unroll
            for (int x = 0; x < 4; ++x) s[4 * r4 + x] = (a[x] + c[x]) + (e[x] + g[x]);
        }

        // ---- scale, mask.  An open block keeps raw scores (the scale folds
        // into the exp argument).
        const bool open_block = j0 + LTILE <= open_to;
        float smax = MASK_VALUE_F;
        if (open_block) {
            #pragma unroll
            for (int r = 0; r < 16; ++r) smax = fmaxf(smax, s[r]);
            smax *= scale2;
        } else {
            const long jr = j0 + 4 * lhi;               // key of register 0
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool ok = jr + (r & 3) + 8 * (r >> 2) < limit;
                const float x = ok ? s[r] * scale2 : MASK_VALUE_F;
                s[r] = x;
                smax = fmaxf(smax, x);
            }
        }
        smax = fmaxf(smax, cross_half(smax));

        // ---- online softmax (the grouped kernel's: exact skip of the rescale
        // when no row's max grew; an all-masked row keeps its exps at 0
        // through the clamped subtrahend)
        const float m_new = fmaxf(m_run, smax);
        const bool any_growth = __builtin_amdgcn_ballot_w64(smax > m_run) != 0;
        const float m_exp = fmaxf(m_new, -1.7e38f);
        const float escale = open_block ? scale2 : 1.f;
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

        // ---- O^T[d][row] += V^T[d][kv] P^T[kv][row] over this wave's 128
        // value columns; pk[4 * ks .. + 3] is the B fragment of k-step ks,
        // keys 16 * ks + 4 * lhi + {0..3, 8..11}
        #pragma unroll
        for (int db = 0; db < DBLK; ++db)
            #pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (lds_v4)(lds_k + (16 * ks) * DK + tr_off[db]));
                const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (lds_v4)(lds_k + (16 * ks + 8) * DK + tr_off[db]));
                const bf16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                o_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    vf, *(const bf16x8*)(pk + 4 * ks), o_acc[db], 0, 0, 0);
            }
        // the image and the partials are read: the next block may overwrite
        lds_barrier();
    }

    // ---- epilogue: lane (l31, lhi) of wave w holds row l31, columns
    // 128 w + 32 db + 8 (r >> 2) + 4 lhi + (r & 3)
    if (row >= R) return;
    // a row that saw no key in this chunk: l == 0, every O is 0 -> out = 0
    const float inv = 1.f / fmaxf(l_run, 1e-38f);
    const long rows_all = (long)p.b * R;
    const long slot = (long)chunk * rows_all + (long)b * R + row;
    float* op = p.out + slot * DV + wid * VCOLS + 4 * lhi;
    #pragma unroll
    for (int db = 0; db < DBLK; ++db)
        #pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
            *(f32x4*)(op + db * 32 + r4 * 8)
                = f32x4{o_acc[db][4 * r4] * inv, o_acc[db][4 * r4 + 1] * inv,
                        o_acc[db][4 * r4 + 2] * inv, o_acc[db][4 * r4 + 3] * inv};
    if (wid == 0 && lhi == 0)
        p.lse[slot] = l_run > 0.f ? __logf(l_run) + m_run * LN2 : MASK_VALUE_F;
}

// ---------------------------------------------------------------------------
// Append: token t < append_lens[b] of sequence b goes to position
// seq_lens[b] + t (lengths BEFORE the append; the host advances them).  One
// wave per (b, t): the row's 72 16-byte chunks go to lanes 0-63 and 0-7.
// ---------------------------------------------------------------------------
template <int DK>
__global__ __launch_bounds__(256) void paged_latent_append_kernel(PagedLatentAppendParams p) {
    constexpr int CH = DK / 8;
    const long rows = (long)p.b * p.t;
    const long wave_global = ((long)blockIdx.x * 4) + (threadIdx.x >> 6);
    if (wave_global >= rows) return;
    const int t = (int)(wave_global % p.t);
    const int b = (int)(wave_global / p.t);
    if (t >= p.append_lens[b]) return;                 // ragged: nothing to do

    const int shift = p.page_shift;
    const long pos = (long)p.seq_lens[b] + t;
    const long slot = pos >> shift;
    if (slot >= p.max_pages) return;                   // host checks; never write astray
    const int pg = p.block_table[(long)b * p.max_pages + slot];
    if ((unsigned)pg >= (unsigned)p.num_pages) return;
    const long drow = ((long)pg << shift) | (pos & ((1L << shift) - 1));
    const u32x4* src = (const u32x4*)((const __bf16*)p.ckv_new + wave_global * DK);
    u32x4* dst = (u32x4*)((__bf16*)p.pages + drow * DK);
    const int lane = threadIdx.x & 63;
    dst[lane] = src[lane];
    if (lane < CH - 64) dst[64 + lane] = src[64 + lane];
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

long paged_latent_chunks(const PagedLatentDecodeParams& p) {
    const long tiles = ((long)p.h * p.nq + LTILE - 1) / LTILE;
    return p.chunks > 0 ? p.chunks
                        : decode_default_chunks(p.max_seq_len, LWAVES * p.b * tiles);
}

void launch_decode_partial_latent(const PagedLatentDecodeParams& p, hipStream_t stream) {
    const long tiles = ((long)p.h * p.nq + LTILE - 1) / LTILE;
    dim3 grid((unsigned)(p.b * tiles), (unsigned)paged_latent_chunks(p));
    dim3 block(LWAVES * 64);
    hipLaunchKernelGGL((decode_partial_latent_kernel<576, 512>), grid, block, 0, stream, p);
}

void launch_paged_latent_append(const PagedLatentAppendParams& p, hipStream_t stream) {
    const long waves = (long)p.b * p.t;
    if (waves == 0) return;
    dim3 grid((unsigned)((waves + 3) / 4));
    dim3 block(256);
    hipLaunchKernelGGL(paged_latent_append_kernel<576>, grid, block, 0, stream, p);
}

}  // namespace ring_attn
