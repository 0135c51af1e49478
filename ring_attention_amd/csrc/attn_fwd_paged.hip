// Paged PREFILL attention: the dense forward's hot loop reading K/V through
// the block table of a PagedKVCache, with per-sequence geometry.
//
// Serving counterpart of attn_fwd.hip (chunked prefill, prefix reuse, ragged
// prompt batches).  q is (B, T, H, D); the chunk's own tokens are already in
// the cache (append first, then attend): query t < q_lens[b] of sequence b
// sits at position seq_lens[b] - q_lens[b] + t and attends keys
// [0, seq_lens[b]) under Mask{causal, has_win, diag = seq_len - q_len,
// q_stride = 1, win} — every workgroup builds its own Mask and its own nk from
// the two length vectors; the algebra stays in attn_mask.h.
//
// The tile loop from the barrier downward is a COPY of attn_fwd_body.inc
// without softclamp, bias, kmask, ticks and ablate.  attn_fwd.hip and its
// body are the headline kernel and their codegen is fragile against
// refactoring (see the body's header), so the copy is the accepted cost, as
// for the fp8 and v2 forwards.  What differs from the dense kernel:
//   * geometry per sequence (lengths read once, kept wave-uniform); a
//     workgroup whose first row is at or beyond q_lens[b] has an empty tile
//     range, never reaches a barrier and writes the dead-row convention
//     (out = 0, finite lse <= -1e30) for its rows < T
//   * staging: key j lives at page block_table[b][j >> shift], row
//     j & (ps - 1); a (page, kv head) block is ps x D contiguous, so the row
//     stride is D.  PAGE_TILE (ps >= KVBLK): a tile lies inside one page, the
//     id is scalar.  Otherwise the id is per staging row; a V pair
//     (2p, 2p+1) never straddles a page (ps is even).  Ids for the next
//     load_tile are fetched one tile ahead, so the dependent table -> row
//     chain stays out of the loads the MFMAs wait for.  Only table entries
//     below ceil(seq_len / ps) are read; rows at or beyond seq_len are
//     zero-filled without forming an address, and an id outside the pool is
//     never dereferenced.
//   * FP8 pools: e4m3 rows + one e8m0 scale per row are dequantised to bf16
//     at staging (e4m3 x 2^(scale-127) has 4 significant bits: exact in bf16
//     unless the product drops below the smallest normal); the staging
//     registers hold the raw bytes and the conversion runs at the LDS write.
//     LDS images and the MFMA path stay bf16.
//   * kv_split > 1: every row < T of every share writes a partial in the
//     dense layout (S, B, H, D, T) + m, l (dead rows and empty shares:
//     m = MASK, l = 0, o = 0); attn_fwd_merge finishes, unchanged.
// Causal pairing is not used: the per-sequence diagonals differ.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

#include "attn_common.h"

namespace ring_attn {

namespace {

constexpr int WAVES = 8;
constexpr int QROWS_WAVE = 32;
constexpr int QROWS_WG = ROWS_WG;
static_assert(QROWS_WG == WAVES * QROWS_WAVE);
constexpr int NTHREADS = WAVES * 64;

template <int D>
struct PagedFwdLds {
    static constexpr int KVB = kvblk(D);
    // double-buffered: K tile [kv][D] + V^T tile [d][kv], 16B-chunk swizzled
    __align__(16) __bf16 k[2][KVB * D];
    __align__(16) __bf16 vt[2][D * KVB];
};

// 8 e4m3 bytes x 2^(sbyte - 127) -> 8 bf16.  The e8m0 byte is the fp32
// exponent field; byte 0 (2^-127) is the one fp32 subnormal.
__device__ __forceinline__ uint4 dequant_e4m3x8(uint2 raw, unsigned sbyte) {
    const float sc = __uint_as_float(sbyte ? sbyte << 23 : 0x00400000u);
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(raw.x, false);
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8(raw.x, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8(raw.y, false);
    const f32x2 d = __builtin_amdgcn_cvt_pk_f32_fp8(raw.y, true);
    return uint4{pack_bf16x2(a[0] * sc, a[1] * sc), pack_bf16x2(b[0] * sc, b[1] * sc),
                 pack_bf16x2(c[0] * sc, c[1] * sc), pack_bf16x2(d[0] * sc, d[1] * sc)};
}

// One staged 8-element chunk as it sits in registers between load_tile and
// write_tile.  An fp8 chunk stays RAW (8 bytes + the row's scale byte) until
// the LDS write: converting at the load would wait for the load right where
// it is issued and undo the issue-early / write-late split (measured: +40%
// on the whole kernel).  A zero chunk dequantises to zeros.
template <bool FP8> struct StagedChunk;
template <> struct StagedChunk<false> {
    uint4 v;
    __device__ __forceinline__ uint4 bf16_bits() const { return v; }
};
template <> struct StagedChunk<true> {
    uint2 raw;
    unsigned sbyte;
    __device__ __forceinline__ uint4 bf16_bits() const { return dequant_e4m3x8(raw, sbyte); }
};

// elements [e0, e0 + 8) of pool row `row`
template <int D, bool FP8>
__device__ __forceinline__ StagedChunk<FP8> pool_chunk(const void* pool, const void* scales,
                                                       long row, int e0) {
    if constexpr (!FP8) {
        return {*(const uint4*)((const __bf16*)pool + row * D + e0)};
    } else {
        return {*(const uint2*)((const unsigned char*)pool + row * D + e0),
                ((const unsigned char*)scales)[row]};
    }
}

}  // namespace

template <int D, bool FP8, bool PAGE_TILE>
__global__ __launch_bounds__(NTHREADS, 1) void attn_fwd_paged_kernel(PagedPrefillParams p) {
    static_assert(D % 32 == 0);
    constexpr int DBLK = D / 32;     // 32-d output blocks
    constexpr int KSTEPS = D / 16;   // QK^T k-steps
    constexpr int KVBLK = kvblk(D);
    constexpr int NBLK = KVBLK / 32;

    __shared__ PagedFwdLds<D> lds;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int l31 = lane & 31;
    const int lhi = lane >> 5;        // 0 or 1

    const int qtile = blockIdx.x;
    const int bh = blockIdx.y;
    const int b = bh / p.h;
    const int h = bh % p.h;
    const int hk = h % p.hk;          // tile GQA: qh pairs qh % hk

    // ---- this sequence's geometry (wave-uniform).  The lengths are clamped
    // to what the table can address and to each other, so nothing below
    // depends on the host having checked them.
    const int shift = p.page_shift;
    const long pmask = (1L << shift) - 1;
    const long T = p.t;
    const long nk = min(max((long)__builtin_amdgcn_readfirstlane(p.seq_lens[b]), 0L),
                        (long)p.max_pages << shift);
    const long ql = min(max((long)__builtin_amdgcn_readfirstlane(p.q_lens[b]), 0L),
                        min(T, nk));
    const Mask M{p.causal, p.has_win, nk - ql, 1, p.win};

    const long irow0 = (long)qtile * QROWS_WG + wid * QROWS_WAVE;  // this wave's first q row
    const long i = irow0 + l31;                                     // this lane's q row
    const bool row_valid = i < ql;
    const long i_clamped = row_valid ? i : 0;
    const long wg_i_min = (long)qtile * QROWS_WG;
    const bool wg_live = wg_i_min < ql;     // else: empty tile range, no barrier

    // ---- load Q fragments (bf16x8 per k-step): q[b, i, h, ks*16 + lhi*8 .. +8]
    const __bf16* qbase = (const __bf16*)p.q + ((long)b * T + i_clamped) * p.h * D + (long)h * D;
    bf16x8 qf[KSTEPS];
    #pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
        qf[ks] = wg_live ? *(const bf16x8*)(qbase + ks * 16 + lhi * 8) : bf16x8{};

    // ---- accumulators
    float m_run = MASK_VALUE_F;   // running row max of scaled scores (lane's q row)
    float l_run = 0.f;            // running row sum
    f32x16 o_acc[DBLK];           // O^T[d][q]: j = l31 = q, rows = d pattern
    #pragma unroll
    for (int db = 0; db < DBLK; ++db) o_acc[db] = f32x16{};

    const bool split_mode = p.kv_split > 1;
    const int zsplit = blockIdx.z;

    // ---- tile bounds over this workgroup's VALID rows (attn_mask.h)
    const long wg_i_max = min((long)(qtile + 1) * QROWS_WG, ql) - 1;
    const long wg_q_min = M.qpos(wg_i_min);
    const long wg_q_max = M.qpos(wg_i_max);
    const long qpos_i = M.qpos(i);                    // this lane's q position
    TileRange tr{0, 0};
    if (wg_live) {
        tr = M.kv_tile_range(wg_i_min, wg_i_max, nk, KVBLK);
        if (split_mode) tr = split_share(tr, p.kv_split, zsplit);
    }
    const int t_lo = tr.lo, t_hi = tr.hi;

    // ---- per-thread staging registers and their tile-local rows
    constexpr int CH_PER_ROW = D * 2 / 16;
    constexpr int KCHUNKS = KVBLK * CH_PER_ROW;          // K-tile 16B chunks
    constexpr int KREGS = (KCHUNKS + NTHREADS - 1) / NTHREADS;
    constexpr int VPAIRS = (KVBLK / 2) * (D / 8);
    constexpr int VREGS = (VPAIRS + NTHREADS - 1) / NTHREADS;
    static_assert(KCHUNKS % NTHREADS == 0 && VPAIRS % NTHREADS == 0);
    constexpr int KROW_STEP = NTHREADS / CH_PER_ROW;     // K rows between a thread's regs
    constexpr int VD_STEP = (NTHREADS / (KVBLK / 2)) * 8;  // extra V regs advance along d
    const int krow0 = tid / CH_PER_ROW, ke0 = (tid % CH_PER_ROW) * 8;
    const int vrow0 = (tid % (KVBLK / 2)) * 2, ve0 = (tid / (KVBLK / 2)) * 8;

    using Staged = StagedChunk<FP8>;
    Staged kst[KREGS];
    Staged vsta[VREGS], vstb[VREGS];

    const int* bt = p.block_table + (long)b * p.max_pages;
    const long head_rows = (long)hk << shift;            // kv head's offset inside a page
    const long page_rows = (long)p.hk << shift;

    // page ids of the NEXT load_tile (fetched one tile ahead): PAGE_TILE uses
    // pgk[0] alone (the tile's one page); else one id per K staging row and
    // one for the V pair
    int pgk[KREGS], pgv = -1;
    long j0_next = (long)t_lo * KVBLK;
    auto fetch_ids = [&]() {
        const long j0 = j0_next;
        if constexpr (PAGE_TILE) {
            pgk[0] = j0 < nk ? bt[j0 >> shift] : -1;
        } else {
            #pragma unroll
            for (int r = 0; r < KREGS; ++r) {
                const long j = j0 + krow0 + r * KROW_STEP;
                pgk[r] = j < nk ? bt[j >> shift] : -1;
            }
            const long jv = j0 + vrow0;
            pgv = jv < nk ? bt[jv >> shift] : -1;
        }
    };

    auto load_tile = [&]() {
        const long j0 = j0_next;
        if constexpr (PAGE_TILE) {
            const int pg = __builtin_amdgcn_readfirstlane(pgk[0]);
            const bool pg_ok = (unsigned)pg < (unsigned)p.num_pages;
            const long row0 = (long)pg * page_rows + head_rows + (j0 & pmask);
            #pragma unroll
            for (int r = 0; r < KREGS; ++r) {
                const int kr = krow0 + r * KROW_STEP;
                kst[r] = (pg_ok && j0 + kr < nk)
                         ? pool_chunk<D, FP8>(p.k_pages, p.kscale, row0 + kr, ke0)
                         : Staged{};
            }
            const bool oka = pg_ok && j0 + vrow0 < nk;
            const bool okb = pg_ok && j0 + vrow0 + 1 < nk;
            #pragma unroll
            for (int r = 0; r < VREGS; ++r) {
                vsta[r] = oka ? pool_chunk<D, FP8>(p.v_pages, p.vscale, row0 + vrow0, ve0 + r * VD_STEP)
                              : Staged{};
                vstb[r] = okb ? pool_chunk<D, FP8>(p.v_pages, p.vscale, row0 + vrow0 + 1, ve0 + r * VD_STEP)
                              : Staged{};
            }
        } else {
            #pragma unroll
            for (int r = 0; r < KREGS; ++r) {
                const int kr = krow0 + r * KROW_STEP;
                const int pg = pgk[r];                 // -1 at or beyond nk
                const long row = (long)pg * page_rows + head_rows + ((j0 + kr) & pmask);
                kst[r] = (unsigned)pg < (unsigned)p.num_pages
                         ? pool_chunk<D, FP8>(p.k_pages, p.kscale, row, ke0)
                         : Staged{};
            }
            const bool oka = (unsigned)pgv < (unsigned)p.num_pages;
            const bool okb = oka && j0 + vrow0 + 1 < nk;
            const long rowa = (long)pgv * page_rows + head_rows + ((j0 + vrow0) & pmask);
            #pragma unroll
            for (int r = 0; r < VREGS; ++r) {
                vsta[r] = oka ? pool_chunk<D, FP8>(p.v_pages, p.vscale, rowa, ve0 + r * VD_STEP)
                              : Staged{};
                vstb[r] = okb ? pool_chunk<D, FP8>(p.v_pages, p.vscale, rowa + 1, ve0 + r * VD_STEP)
                              : Staged{};
            }
        }
        j0_next += KVBLK;
        fetch_ids();
    };

    auto write_tile = [&](int par) {
        #pragma unroll
        for (int r = 0; r < KREGS; ++r) {
            int c = tid + r * NTHREADS;
            int row = c / CH_PER_ROW, ch = c % CH_PER_ROW;
            *(uint4*)(lds.k[par] + row * D + swz<D / 8>(row, ch) * 8) = kst[r].bf16_bits();
        }
        #pragma unroll
        for (int r = 0; r < VREGS; ++r) {
            int c = tid + r * NTHREADS;
            // kv pairs land in the PV k order (kperm_pair): the packed P
            // pairs are then the B fragments with no lane exchange
            int jp = kperm_pair(c % (KVBLK / 2));
            int d0 = (c / (KVBLK / 2)) * 8;
            union { uint4 u; bf16x8 v; } va, vb;
            va.u = vsta[r].bf16_bits(); vb.u = vstb[r].bf16_bits();
            #pragma unroll
            for (int e = 0; e < 8; ++e) {
                int d = d0 + e;
                int byte_off = d * KVBLK * 2 + ((jp * 4) ^ ((d & 7) << 4));
                __bf16 pair[2] = {va.v[e], vb.v[e]};
                *(uint32_t*)((char*)lds.vt[par] + byte_off) = *(uint32_t*)pair;
            }
        }
    };

    // 3-deep pipeline over DOUBLE-buffered LDS: one barrier per tile; LDS
    // writes and the next-next tile's HBM loads fully overlap the MFMAs
    const float scale2 = p.scale * LOG2E;    // softmax runs in the exp2 domain
    if (t_lo < t_hi) {
        fetch_ids();
        load_tile();
        write_tile(t_lo & 1);
        if (t_lo + 1 < t_hi) load_tile();
    }

    for (int t = t_lo; t < t_hi; ++t) {
        const int par = t & 1;
        const long j0 = (long)t * KVBLK;
        const long jmax = min(j0 + KVBLK, nk) - 1;
        const bool full_tile =
            (jmax - j0 == KVBLK - 1) &&
            M.uncut(wg_q_min, wg_q_max, j0, jmax);

        __syncthreads();

        // ---- QK^T: S^T[kv][q] for the NBLK 32-row kv blocks
        f32x16 s[NBLK];
        #pragma unroll
        for (int kb = 0; kb < NBLK; ++kb) s[kb] = f32x16{};
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int kb = 0; kb < NBLK; ++kb) {
            int krow = kb * 32 + l31;
            #pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) {
                int chunk = ks * 2 + lhi;
                bf16x8 kf = *(const bf16x8*)(lds.k[par] + krow * D + swz<D / 8>(krow, chunk) * 8);
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[kb], 0, 0, 0);
            }
        }
        __builtin_amdgcn_s_setprio(0);

        // stage tile t+1 into the other buffer while the MFMAs above retire
        if (t + 1 < t_hi) write_tile(par ^ 1);
        if (t + 2 < t_hi) load_tile();

        // ---- scale (exp2 domain), mask in place.  The full-tile variant
        // must contain NO per-element conditions: a condition inside the
        // unrolled loop is PREDICATED (cndmask per element, executed on every
        // tile) rather than branched — hoist to one scalar branch.
        float smax = MASK_VALUE_F;
        if (full_tile) {
            // exp2+fma fold: fmax runs on RAW scores (scale2 > 0 is
            // monotone); the scale is folded into the exp argument as a
            // single v_fma below — saves one VALU per element
            #pragma unroll
            for (int kb = 0; kb < NBLK; ++kb)
                #pragma unroll
                for (int r = 0; r < 16; ++r)
                    smax = fmaxf(smax, s[kb][r]);
            smax *= scale2;
        } else {
            #pragma unroll
            for (int kb = 0; kb < NBLK; ++kb)
                #pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float x = s[kb][r] * scale2;
                    long j = j0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                    bool ok = M.attends(qpos_i, j, j <= jmax);
                    if (!ok) x = MASK_VALUE_F;
                    s[kb][r] = x;
                    smax = fmaxf(smax, x);
                }
        }
        smax = fmaxf(smax, cross_half(smax));

        // ---- online softmax update (defer-max THR=0: exact — skip the O
        // rescale whenever the running max did not grow on any lane)
        float m_new = fmaxf(m_run, smax);
        const bool any_growth = !__all(smax <= m_run);
        // all-masked rows: m_new == MASK -> exp2(x - m_new) would be 1 for
        // every masked element (out = mean(V) instead of 0).  Clamping the
        // exp-domain max keeps those exps at 0 while leaving real rows
        // (|scores| << 1e37) untouched.
        const float m_exp = fmaxf(m_new, -1.7e38f);
        // full tiles kept RAW scores: exp2(fma(s, scale2, -m))
        const float escale = full_tile ? scale2 : 1.f;
        alignas(16) uint32_t pk[NBLK * 8];                          // packed bf16 pairs
        float partial[NBLK * 8];
        #pragma unroll
        for (int x2 = 0; x2 < NBLK * 8; ++x2) {
            float e0 = __builtin_amdgcn_exp2f(
                __builtin_fmaf(s[x2 >> 3][(2 * x2) & 15], escale, -m_exp));
            float e1 = __builtin_amdgcn_exp2f(
                __builtin_fmaf(s[x2 >> 3][(2 * x2 + 1) & 15], escale, -m_exp));
            partial[x2] = e0 + e1;
            pk[x2] = pack_bf16x2(e0, e1);
        }
        // pairwise tree instead of a 32-deep serial dependency chain
        #pragma unroll
        for (int w = NBLK * 4; w >= 1; w >>= 1)
            #pragma unroll
            for (int x2 = 0; x2 < w; ++x2) partial[x2] += partial[x2 + w];
        float rowsum = partial[0];
        rowsum += cross_half(rowsum);
        if (any_growth) {
            float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            l_run = l_run * alpha + rowsum;
            #pragma unroll
            for (int db = 0; db < DBLK; ++db)
                #pragma unroll
                for (int r = 0; r < 16; ++r) o_acc[db][r] *= alpha;
            m_run = m_new;
        } else {
            l_run += rowsum;
        }

        // ---- PV: O^T[d][q] += V^T[d][kv] P^T[kv][q]; pk[4*ks .. 4*ks+3] is
        // the B fragment of k-step ks (the vt image is staged in that order)
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int db = 0; db < DBLK; ++db) {
            int drow = db * 32 + l31;
            #pragma unroll
            for (int ks = 0; ks < NBLK * 2; ++ks) {
                int chunk = ks * 2 + lhi;
                bf16x8 vf = *(const bf16x8*)(lds.vt[par] + drow * KVBLK + swz<KVBLK / 8>(drow, chunk) * 8);
                o_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    vf, *(const bf16x8*)(pk + 4 * ks), o_acc[db], 0, 0, 0);
            }
        }
        __builtin_amdgcn_s_setprio(0);
    }

    // ---- epilogue: every row < T is written.  A row at or beyond q_lens[b]
    // ran the loop on row 0's q: drop its state for the dead-row convention.
    if (i >= T) return;
    if (!row_valid) {
        m_run = MASK_VALUE_F;
        l_run = 0.f;
        #pragma unroll
        for (int db = 0; db < DBLK; ++db) o_acc[db] = f32x16{};
    }

    if (split_mode) {
        // this share's unnormalized partial (merged by attn_fwd_merge)
        const long part = (long)zsplit * p.b * p.h;
        float* mrow = p.m_part + (part + (long)b * p.h + h) * T;
        float* lrow = p.l_part + (part + (long)b * p.h + h) * T;
        if (lhi == 0) {
            mrow[i] = m_run == MASK_VALUE_F ? MASK_VALUE_F : m_run * LN2;
            lrow[i] = l_run;
        }
        float* oa = p.o_part + (part + (long)b * p.h + h) * D * T;
        #pragma unroll
        for (int db = 0; db < DBLK; ++db)
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                int d = db * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                oa[(long)d * T + i] = o_acc[db][r];
            }
        return;
    }

    float l_safe = fmaxf(l_run, 1e-38f);
    float inv_l = 1.f / l_safe;
    __bf16* ob = (__bf16*)p.out + ((long)b * T + i) * p.h * D + (long)h * D;
    #pragma unroll
    for (int db = 0; db < DBLK; ++db)
        #pragma unroll
        for (int g = 0; g < 4; ++g) {                            // groups of 4 contiguous d
            __bf16 four[4];
            #pragma unroll
            for (int e = 0; e < 4; ++e)
                four[e] = (__bf16)(o_acc[db][g * 4 + e] * inv_l);
            int d = db * 32 + 8 * g + 4 * lhi;
            *(uint2*)(ob + d) = *(uint2*)four;
        }
    if (lhi == 0) {
        float* lsep = p.lse + ((long)b * p.h + h) * T;
        lsep[i] = __logf(l_safe) + m_run * LN2;
    }
}

template <int D, bool FP8>
static void launch_paged_d(const PagedPrefillParams& p, dim3 grid, hipStream_t stream) {
    dim3 block(NTHREADS);
    if ((1 << p.page_shift) >= kvblk(D))
        hipLaunchKernelGGL((attn_fwd_paged_kernel<D, FP8, true>), grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL((attn_fwd_paged_kernel<D, FP8, false>), grid, block, 0, stream, p);
}

void launch_attn_fwd_paged(const PagedPrefillParams& p, int head_dim, bool fp8,
                           hipStream_t stream) {
    dim3 grid((unsigned)ceil_div(p.t, QROWS_WG), (unsigned)(p.b * p.h),
              (unsigned)(p.kv_split > 1 ? p.kv_split : 1));
    if (head_dim == 64 && !fp8) launch_paged_d<64, false>(p, grid, stream);
    else if (head_dim == 128 && !fp8) launch_paged_d<128, false>(p, grid, stream);
    else if (head_dim == 64) launch_paged_d<64, true>(p, grid, stream);
    else if (head_dim == 128) launch_paged_d<128, true>(p, grid, stream);
    else __builtin_trap();   // unsupported head dim is a host-side error (bindings)
}

}  // namespace ring_attn
