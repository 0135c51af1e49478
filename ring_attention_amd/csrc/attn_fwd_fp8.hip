// CDNA4 (gfx950) MX-FP8 flash-attention FORWARD kernel (serving fast path).
//
// MI355X-only capability beyond the reference (which is bf16/fp16 Triton,
// /root/reference/ring_attention_pytorch/triton_flash_attn.py): the gfx950
// block-scaled MFMA v_mfma_scale_f32_32x32x64_f8f6f4 runs e4m3 at ~4.7 PF/s
// (2x the bf16 rate, 4x the K per instruction), so QK^T and PV both drop to
// ONE scaled MFMA per 32x32x64 tile.  Softmax stays fp32 (exp2 domain) and
// the accumulator is fp32 — only the matmul operands are 8-bit.
//
// Numerics design (hardware semantics verified by csrc/tools/fp8_probe*.hip
// on MI355X):
//   * A/B fragment map (our loading convention): lane l, byte r ->
//     (i = l&31, k = 32*(l>>5) + r) for A; (k = 32*(l>>5) + r, j = l&31)
//     for B; C/D = the standard 32x32 map (dtype-independent on gfx950).
//     Any k bijection is self-consistent as long as A and B share it.
//   * scale operands: lane l's e8m0 byte (selected by opsel, we use byte 0)
//     scales (row l&31, k-block l>>5); passing the SAME byte on both lane
//     halves scales the whole 64-deep row uniformly, which sidesteps the
//     hardware's k-block interleave entirely.  Granularity used:
//       Q, K: one e8m0 per row (per 64-d chunk) = 2^ceil(log2(amax/448))
//       V:    one e8m0 per (d row, 64-kv chunk)
//       P:    fixed 2^-8 (exp2(x - m) <= 1; the shift moves the e4m3
//             subnormal cutoff from 2^-9 to 2^-17)
//   * e4m3 is OCP e4m3fn (torch.float8_e4m3fn matches bit-for-bit).
//   * the scaled MFMA's sum is NOT exact (csrc/tools/fp8_probe5.hip; recorded
//     results in tests/golden/mfma_scale_f8_dot.npz): inside every group of 8
//     consecutive k (8 consecutive d for QK^T, 8 consecutive keys for PV) the
//     products are aligned to the group's largest exponent sum e(a) + e(b)
//     (e4m3 exponent field, subnormals at -6) and truncated toward zero 13
//     bits below it; the 8 group sums and C then add with ~25 bits.  Scores
//     are therefore off the exact dot product by up to 2^-12.2 of the largest
//     product, which moves P bytes and lse (2e-3 on inputs with 2^+-2 row
//     gains).  tests/fp8_emulation.py::mfma_scores models it; with it the
//     kernel matches the CPU model to bf16 rounding on out and 7.6e-6 on lse.
//     PV's share is below 2^-10 of sum(P |V|).
//
// Causal: the PAIRED instantiation uses the bf16 kernels' mirrored-tile
// load balance (WG x runs q-tiles (x, T-1-x) — uniform T+1 kv-tile walks
// per WG instead of the 2:1 triangle imbalance).  GQA pairs q head qh with
// kv head qh % hk (reference tile convention).
//
// Mask: attn_mask.h's geometry (causal at qpos(i) = i * q_stride + diag, an
// optional window qpos(i) - j <= win), so a ring hop of any layout is one
// launch; the walk covers kv_tile_range only.  Rows that attend no key give
// out == 0 and the finite lse floor log(1e-38) + MASK_VALUE_F * ln 2: a masked
// score is MASK_VALUE_F, m_exp is clamped at -1.7e38, so exp2 sees -1.7e38
// (P = 0, never inf - inf), and alpha = exp2(MASK_VALUE_F - MASK_VALUE_F) = 1.
//
// Scope (asserted in the binding): no key-pad mask/bias/softclamp, single
// shot (no ring resume), D in {64, 128}.  Ragged lengths are handled by the
// PYTHON wrapper padding the quantized buffers to (nq%256, nk%128)
// alignment (zero rows, scale 2^-127 — never NaN bytes) while the kernel
// masks scores at the TRUE kv length; padded q rows are sliced off by the
// wrapper.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>
#include <type_traits>

#include "attn_common.h"

namespace ring_attn {

typedef int i32x8_ __attribute__((ext_vector_type(8)));

static constexpr int FP8_WAVES = 8;
static constexpr int FP8_QROWS_WAVE = 32;
static constexpr int FP8_QROWS_WG = ROWS_WG;                      // 256
static_assert(FP8_QROWS_WG == FP8_WAVES * FP8_QROWS_WAVE);
static constexpr int FP8_NTHREADS = FP8_WAVES * 64;               // 512
// FP8_KVBLK (128) comes from attn_mask.h
static constexpr int FP8_NBLK = FP8_KVBLK / 32;                   // 4

template <int D>
struct Fp8Lds {
    __align__(16) unsigned char k[2][FP8_KVBLK * D];     // [kv][d] bytes
    __align__(16) unsigned char vt[2][D * FP8_KVBLK];    // [d][kv] bytes
    unsigned char ks[2][FP8_KVBLK * (D / 64)];           // k (row, chunk) e8m0
};

// GEO selects the mask: false folds the standard mask (qpos(i) = i, no window)
// to constants, true reads diag / q_stride / win from the params.  Without
// GEO the kernel takes the core of the params alone, so its kernarg and the
// PAIRED frame's copy of it are what they were before the geometry existed.
template <bool GEO>
using Fp8Frame = std::conditional_t<GEO, Fp8FwdParams, Fp8FwdCore>;

template <int D, bool PAIRED, bool GEO>
__global__ __launch_bounds__(FP8_NTHREADS, 1)
void attn_fwd_fp8_kernel(Fp8Frame<GEO> p) {
    constexpr int DBLK = D / 32;
    constexpr int NDCH = D / 64;          // 64-deep MFMA k-chunks per head dim
    constexpr int KCH = D * 2 / 32;       // 16B LDS chunks per K row (D bytes)

    __shared__ Fp8Lds<D> lds;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int l31 = lane & 31;
    const int lhi = lane >> 5;

    const int bh = blockIdx.y;
    const int b = bh / p.h;
    const int h = bh % p.h;
    const int hk = h % p.hk;              // reference tile GQA pairing

    const int n_pit = PAIRED
        ? (p.paired - 1 - (int)blockIdx.x == (int)blockIdx.x ? 1 : 2) : 1;
    for (int pit = 0; pit < n_pit; ++pit) {
    const int qtile = PAIRED
        ? (pit == 0 ? (int)blockIdx.x : p.paired - 1 - (int)blockIdx.x)
        : (int)blockIdx.x;
    if (PAIRED && pit == 1) {
        __syncthreads();                  // LDS handoff between tiles
    }

    auto fp8_body = [&]() {
    const Fp8Frame<GEO> P = p;            // register-local (noinline frame)
    const long i = (long)qtile * FP8_QROWS_WG + wid * FP8_QROWS_WAVE + l31;

    // ---- Q fragments: per 64-d chunk, 32 e4m3 bytes (d = 64*dc + 32*lhi
    // .. +31) + per-chunk row scale
    const unsigned char* qrow = (const unsigned char*)P.q
        + ((long)b * P.nq + i) * P.h * D + (long)h * D + 32 * lhi;
    union { i32x8_ v; uint4 u4[2]; } qf[NDCH];
    int qs[NDCH];
    #pragma unroll
    for (int dc = 0; dc < NDCH; ++dc) {
        qf[dc].u4[0] = *(const uint4*)(qrow + dc * 64);
        qf[dc].u4[1] = *(const uint4*)(qrow + dc * 64 + 16);
        qs[dc] = ((const unsigned char*)P.qs)[
            (((long)b * P.nq + i) * P.h + h) * NDCH + dc];
    }

    // ---- accumulators
    float m_run = MASK_VALUE_F, l_run = 0.f;
    f32x16 o_acc[DBLK];
    #pragma unroll
    for (int db = 0; db < DBLK; ++db) o_acc[db] = f32x16{};

    // ---- kv tile range [t_lo, t_hi) of this workgroup (attn_mask.h; it
    // takes ROW indices and applies qpos itself).  nq and nk are padded to
    // whole tiles, so the walk covers the padded keys and masks them at
    // nk_true below.  An empty range falls straight to the epilogue.
    const Mask M = [&P] {
        if constexpr (GEO) return mask_of(P);
        else return Mask{P.causal, 0, 0, 1, 0};
    }();
    const long wg_q_min = (long)qtile * FP8_QROWS_WG;
    const long wg_q_max = wg_q_min + FP8_QROWS_WG - 1;
    const TileRange tr = M.kv_tile_range(wg_q_min, wg_q_max, P.nk, FP8_KVBLK);
    const int t_hi = tr.hi;
    const int t_lo = GEO ? tr.lo : 0;
    // the one 64-bit position of this lane's row; per tile it becomes a
    // 32-bit offset range (Mask::row_cut), never a position per element
    const long qp = M.qpos(i);

    // ---- staging (one uint4 per thread per image per tile)
    const unsigned char* kbase = (const unsigned char*)P.k
        + ((long)b * P.nk) * P.hk * D + (long)hk * D;
    const unsigned char* vtbase = (const unsigned char*)P.vt
        + (((long)b * P.hk + hk) * D) * P.nk;
    const unsigned char* ksbase = (const unsigned char*)P.ks
        + (((long)b * P.nk) * P.hk + hk) * NDCH;

    // per-tile staging: K = KVBLK*D bytes, V^T = D*KVBLK bytes — KREGS
    // uint4 per thread each; ks = KVBLK*NDCH bytes
    constexpr int KREGS = FP8_KVBLK * D / 16 / FP8_NTHREADS;
    constexpr int VCH = FP8_KVBLK / 16;   // 16B chunks per V^T row
    const long k_row_stride = (long)P.hk * D;
    const unsigned char* kptr = kbase + (tid / KCH) * k_row_stride + (tid % KCH) * 16;
    const unsigned char* vptr = vtbase + (long)(tid / VCH) * P.nk + (tid % VCH) * 16;
    const unsigned char* ksptr = ksbase + (long)(tid / NDCH) * P.hk * NDCH + (tid % NDCH);
    if constexpr (GEO) {                  // a window starts the walk at t_lo
        kptr += (long)t_lo * FP8_KVBLK * k_row_stride;
        vptr += (long)t_lo * FP8_KVBLK;
        ksptr += (long)t_lo * FP8_KVBLK * P.hk * NDCH;
    }

    uint4 kst[KREGS], vst[KREGS];
    unsigned char ksst = 0;

    auto load_tile = [&]() {
        #pragma unroll
        for (int r = 0; r < KREGS; ++r) {
            kst[r] = *(const uint4*)(kptr + (long)(r * (FP8_NTHREADS / KCH)) * k_row_stride);
            vst[r] = *(const uint4*)(vptr + (long)(r * (FP8_NTHREADS / VCH)) * P.nk);
        }
        if (tid < FP8_KVBLK * NDCH) ksst = *ksptr;
        kptr += (long)FP8_KVBLK * k_row_stride;
        vptr += FP8_KVBLK;
        ksptr += (long)FP8_KVBLK * P.hk * NDCH;
    };
    auto write_tile = [&](int par) {
        #pragma unroll
        for (int r = 0; r < KREGS; ++r) {
            {   // K: D-byte rows, KCH 16B chunks
                int c = tid + r * FP8_NTHREADS;
                int row = c / KCH, ch = c % KCH;
                *(uint4*)(lds.k[par] + row * D + swz<KCH>(row, ch) * 16) = kst[r];
            }
            {   // V^T: KVBLK-byte rows, VCH chunks
                int c = tid + r * FP8_NTHREADS;
                int row = c / VCH, ch = c % VCH;
                *(uint4*)(lds.vt[par] + row * FP8_KVBLK + swz<8>(row, ch) * 16) = vst[r];
            }
        }
        if (tid < FP8_KVBLK * NDCH) lds.ks[par][tid] = ksst;
    };

    const float scale2 = P.scale * LOG2E;

    if (t_hi > t_lo) {
        load_tile();
        write_tile(0);
        if (t_hi > t_lo + 1) load_tile();
    }

    for (int t = t_lo; t < t_hi; ++t) {
        const int par = (t - t_lo) & 1;
        const long j0 = (long)t * FP8_KVBLK;
        // uncut wants q POSITIONS (qpos is monotone in the row index)
        const bool full_tile = (j0 + FP8_KVBLK <= P.nk_true)
            && M.uncut(M.qpos(wg_q_min), M.qpos(wg_q_max), j0, j0 + FP8_KVBLK - 1);

        __syncthreads();

        // ---- QK^T: one scaled MFMA per (32-kv block, 64-d chunk); chunks
        // chain through the fp32 accumulator (each dequants its own scales)
        f32x16 s[FP8_NBLK];
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int kb = 0; kb < FP8_NBLK; ++kb) {
            int krow = kb * 32 + l31;
            f32x16 acc = {};
            #pragma unroll
            for (int dc = 0; dc < NDCH; ++dc) {
                union { i32x8_ v; uint4 u4[2]; } kf;
                kf.u4[0] = *(const uint4*)(lds.k[par] + krow * D
                               + swz<KCH>(krow, 4 * dc + 2 * lhi) * 16);
                kf.u4[1] = *(const uint4*)(lds.k[par] + krow * D
                               + swz<KCH>(krow, 4 * dc + 2 * lhi + 1) * 16);
                int sa = lds.ks[par][krow * NDCH + dc];
                acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
                    kf.v, qf[dc].v, acc, 0, 0, 0, sa, 0, qs[dc]);
            }
            s[kb] = acc;
        }
        __builtin_amdgcn_s_setprio(0);

        // stage tile t+1 while the MFMAs retire
        if (t + 1 < t_hi) write_tile(par ^ 1);
        if (t + 2 < t_hi) load_tile();

        // ---- softmax (exp2 domain; scores are true-scale fp32 — the MFMA
        // applied the e8m0 dequant in hardware).  Masked (diagonal) tiles
        // scale + mask in place and switch the exp fold to escale = 1.
        float smax = MASK_VALUE_F;
        if (full_tile) {
            #pragma unroll
            for (int kb = 0; kb < FP8_NBLK; ++kb)
                #pragma unroll
                for (int r = 0; r < 16; ++r) smax = fmaxf(smax, s[kb][r]);
            smax *= scale2;
        } else if constexpr (GEO) {
            // padded keys, causal and window as one offset range per row
            // (the lane half's 4 * lhi goes into the range, so that the
            // element offsets compared against it are compile-time constants)
            const RowCut rc = M.row_cut(qp, j0, FP8_KVBLK, P.nk_true);
            const int o_lo = rc.lo - 4 * lhi, o_hi = rc.hi - 4 * lhi;
            #pragma unroll
            for (int kb = 0; kb < FP8_NBLK; ++kb)
                #pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = kb * 32 + (r & 3) + 8 * (r >> 2);
                    float x = s[kb][r] * scale2;
                    if (o < o_lo || o > o_hi) x = MASK_VALUE_F;
                    s[kb][r] = x;
                    smax = fmaxf(smax, x);
                }
        } else {
            #pragma unroll
            for (int kb = 0; kb < FP8_NBLK; ++kb)
                #pragma unroll
                for (int r = 0; r < 16; ++r) {
                    long j = j0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                    float x = s[kb][r] * scale2;
                    // padded keys, then the mask at qpos(i) = i
                    if (!M.attends(qp, j, j < P.nk_true)) x = MASK_VALUE_F;
                    s[kb][r] = x;
                    smax = fmaxf(smax, x);
                }
        }
        smax = fmaxf(smax, cross_half(smax));

        float m_new = fmaxf(m_run, smax);
        const bool any_growth = !__all(smax <= m_run);
        const float m_exp = fmaxf(m_new, -1.7e38f);
        const float escale = full_tile ? scale2 : 1.f;

        // exp2 + pack to e4m3 at 2^8 (PV dequants via scale byte 119)
        // own_dw[kb][g] = bytes of kv rows (8g + 4*lhi .. +3) of block kb
        uint32_t own_dw[FP8_NBLK][4];
        float partial[FP8_NBLK * 8];
        #pragma unroll
        for (int kb = 0; kb < FP8_NBLK; ++kb) {
            #pragma unroll
            for (int g = 0; g < 4; ++g) {
                float e0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][4 * g + 0], escale, -m_exp));
                float e1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][4 * g + 1], escale, -m_exp));
                float e2 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][4 * g + 2], escale, -m_exp));
                float e3 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][4 * g + 3], escale, -m_exp));
                partial[kb * 8 + 2 * g] = e0 + e1;
                partial[kb * 8 + 2 * g + 1] = e2 + e3;
                int u = __builtin_amdgcn_cvt_pk_fp8_f32(e0 * 256.f, e1 * 256.f, 0, false);
                u = __builtin_amdgcn_cvt_pk_fp8_f32(e2 * 256.f, e3 * 256.f, u, true);
                own_dw[kb][g] = (uint32_t)u;
            }
        }
        #pragma unroll
        for (int w = FP8_NBLK * 4; w >= 1; w >>= 1)
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

        // ---- build P^T B-fragments per 64-kv chunk via permlane32_swap:
        // my frag slot 2g   <- block (2c + lhi) rows 8g+0..3
        //         slot 2g+1 <- block (2c + lhi) rows 8g+4..7
        // swap(own_dw[2c][g], own_dw[2c+1][g]):
        //   lanes<32: r0 = own [2c][g] (rows 8g+0-3), r1 = partner [2c][g]
        //             (rows 8g+4-7)            -> block 2c  = 2c+lhi
        //   lanes>=32: r0 = partner [2c+1][g] (rows 8g+0-3), r1 = own
        //             [2c+1][g] (rows 8g+4-7)  -> block 2c+1 = 2c+lhi
        #pragma unroll
        for (int c = 0; c < 2; ++c) {
            union { i32x8_ v; uint32_t dw[8]; } pf;
            #pragma unroll
            for (int g = 0; g < 4; ++g) {
                u32x2 r = __builtin_amdgcn_permlane32_swap(
                    own_dw[2 * c][g], own_dw[2 * c + 1][g], false, false);
                pf.dw[2 * g] = r[0];
                pf.dw[2 * g + 1] = r[1];
            }
            // ---- PV: O^T[d][q] += V^T[d][kv] P^T[kv][q], one scaled MFMA
            // per 32-d block (K = 64 kv)
            __builtin_amdgcn_s_setprio(1);
            #pragma unroll
            for (int db = 0; db < DBLK; ++db) {
                int drow = db * 32 + l31;
                union { i32x8_ v; uint4 u4[2]; } vf;
                vf.u4[0] = *(const uint4*)(lds.vt[par] + drow * FP8_KVBLK
                                           + swz<8>(drow, 4 * c + 2 * lhi) * 16);
                vf.u4[1] = *(const uint4*)(lds.vt[par] + drow * FP8_KVBLK
                                           + swz<8>(drow, 4 * c + 2 * lhi + 1) * 16);
                int sv = ((const unsigned char*)P.vs)[
                    (((long)b * P.hk + hk) * D + drow) * P.nvs + (t * 2 + c)];
                o_acc[db] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
                    vf.v, pf.v, o_acc[db], 0, 0, 0, sv, 0, 119);
            }
            __builtin_amdgcn_s_setprio(0);
        }
    }

    // ---- epilogue: normalize, emit bf16 out (B,Nq,H,D) + lse (B,H,Nq)
    float l_safe = fmaxf(l_run, 1e-38f);
    float inv_l = 1.f / l_safe;
    __bf16* ob = (__bf16*)P.out + ((long)b * P.nq + i) * P.h * D + (long)h * D;
    #pragma unroll
    for (int db = 0; db < DBLK; ++db)
        #pragma unroll
        for (int g = 0; g < 4; ++g) {
            __bf16 four[4];
            #pragma unroll
            for (int e = 0; e < 4; ++e)
                four[e] = (__bf16)(o_acc[db][g * 4 + e] * inv_l);
            int d = db * 32 + 8 * g + 4 * lhi;
            *(uint2*)(ob + d) = *(uint2*)four;
        }
    if (lhi == 0) {
        float* lsep = P.lse + ((long)b * P.h + h) * P.nq;
        lsep[i] = __logf(l_safe) + m_run * LN2;
    }
    };
    if constexpr (PAIRED) noinline_call(fp8_body);
    else fp8_body();
    }  // pair loop
}

template <int D, bool PAIRED, bool GEO>
static void launch_fp8_instance(const Fp8FwdParams& p, dim3 grid, hipStream_t stream) {
    const Fp8Frame<GEO> arg = p;          // without GEO: the core (slicing)
    hipLaunchKernelGGL((attn_fwd_fp8_kernel<D, PAIRED, GEO>), grid,
                       dim3(FP8_NTHREADS), 0, stream, arg);
}

// Which instantiation a launch runs:
//   A causal mask whose row 0 already sees the last true key (diag >=
//   nk_true - 1: a ring hop from an earlier rank) cuts nothing and is
//   launched as not causal.  Then
//   GEO    is off when the mask is the standard one: no window and either
//          not causal (diag / q_stride do not matter) or diag == 0 with
//          q_stride == 1.  Those launches keep the constant-folded mask.
//   PAIRED (WG x runs q tiles (x, T-1-x)) when the mask is causal, has no
//          window, q_stride == 1 and the diagonal cuts the hop: row 0 misses
//          a key (the rule above) and the last row sees one.  That covers
//          the standard causal call and every striped ring hop (diag 0 /
//          -1).  A window bounds every row's walk and a stride or a diagonal
//          outside the hop leaves no triangle to balance: those take the
//          plain grid.
void launch_attn_fwd_fp8(const Fp8FwdParams& p, int head_dim, hipStream_t stream) {
    const long T = p.nq / FP8_QROWS_WG;
    const bool causal = p.causal && p.diag < p.nk_true - 1;
    const bool geo = p.has_win || (causal && (p.diag != 0 || p.q_stride != 1));
    const bool cuts = p.nq - 1 + p.diag >= 0;
    const bool paired = causal && !p.has_win && p.q_stride == 1 && cuts;
    Fp8FwdParams pc = p;
    pc.causal = causal ? 1 : 0;
    pc.paired = (int)T;
    const dim3 grid((unsigned)(paired ? (T + 1) / 2 : T), (unsigned)(p.b * p.h));
    const bool d64 = head_dim == 64;
    // (the standard-mask instantiations are named first, in the order they
    // always had: the PAIRED frame functions are 4-byte aligned, so where
    // they land in the code object follows from what is emitted before them,
    // and a hot loop moved against the fetch window cost 0.2 - 0.6%)
    if (!geo) {
        if (paired) d64 ? launch_fp8_instance<64, true, false>(pc, grid, stream)
                        : launch_fp8_instance<128, true, false>(pc, grid, stream);
        else        d64 ? launch_fp8_instance<64, false, false>(pc, grid, stream)
                        : launch_fp8_instance<128, false, false>(pc, grid, stream);
    } else {
        if (paired) d64 ? launch_fp8_instance<64, true, true>(pc, grid, stream)
                        : launch_fp8_instance<128, true, true>(pc, grid, stream);
        else        d64 ? launch_fp8_instance<64, false, true>(pc, grid, stream)
                        : launch_fp8_instance<128, false, true>(pc, grid, stream);
    }
}

}  // namespace ring_attn
