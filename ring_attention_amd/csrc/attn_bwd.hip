// CDNA4 (gfx950) flash-attention BACKWARD kernels (recompute-based).
//
// Capability counterpart of the reference's Triton _bwd_kernel
// (/root/reference/ring_attention_pytorch/triton_flash_attn.py:509-1128),
// re-designed for wave64/MFMA; no code ported.  TWO kernels, each with the
// contraction laid out so every accumulator lives in registers and no
// cross-workgroup atomics exist at all:
//
//  * attn_bwd_dq_kernel — ROW-parallel (mirrors the forward kernel): each
//    wave owns 32 q rows, Q^T and dO^T fragments live in registers, K/V/K^T
//    tiles stream through LDS; ds^T is built in-register (lane = q) and
//    dq^T accumulates in registers; epilogue does ONE plain fp32 += per
//    element (each q row is owned by exactly one workgroup).
//  * attn_bwd_dkv_kernel — COLUMN-parallel: each wave owns 32 kv rows with
//    K/V fragments in registers across the whole q loop; Q/dO stream through
//    LDS (one row-major image each, read row-wise for S/dP and through
//    ds_read_b64_tr_b16 for dv/dk; d128: row-major + pair-staged
//    transpose); p/ds fragments are built
//    in-register (lane = kv); dk/dv accumulate in registers and are written
//    once.  GQA: the group's query heads are iterated with K/V resident, so
//    dk/dv need no cross-head reduction.
//
// The reference needed tl.debug_barrier() workarounds and an atomic-vs-
// serialized dq autotune choice (triton_flash_attn.py:648-776); this design
// removes the hazards structurally (profiled on MI355X: the single-kernel
// atomic variant was LDS/atomic-bound at 35% LDS-array cycles).
//
// causality/striping/lookback use the forward's mask geometry (attn_mask.h);
// softclamp backward applies the dtanh factor exactly as the oracle.
//
// Output layouts:
//   dq: fp32 (B, Nq, H, D)   — plain accumulate (+=) across hops
//   dk: fp32 (B, HK, Nk, D)  — plain writes (one WG owns each row)
//   dv: fp32 (B, HK, D, Nk)  — transposed scratch, coalesced from dv^T regs
// Single-pass launches may instead pass bf16 dq_bf (B, Nq, H, D) and
// dk_bf/dv_bf (B, Nk, HK, D): the epilogues round and store the final
// gradients themselves; attn_bwd_finalize_kernel does the same in one launch
// for the fp32 scratch of the accumulating modes.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

#include "attn_common.h"

namespace ring_attn {

// ---------------------------------------------------------------------------
// dq kernel: row-parallel, forward-like (same pipeline as attn_fwd_kernel:
// double-buffered LDS, one barrier per kv tile, running-pointer staging)
// ---------------------------------------------------------------------------
// Tile shapes come from attn_mask.h: ROWS_WG q rows (8 waves x 32) walk kv
// tiles of kvblk(D).
// The kt image is gone (K^T fragments come from the row-major k image via
// ds_read_b64_tr_b16 — the v2 forward's V recipe, hardware-verified in
// tools/hw_probe.hip), which frees a third of the LDS and the transpose
// staging.  d128 stays at KVB=64: the KVB=128 variant its freed LDS allows
// spills 280-336 B/lane into the hot loop and measured SLOWER (174 vs 204
// TF headline) — the round-1 "fwd KVBLK=128 at d128" trap again.
template <int D>
struct DqLds {
    static constexpr int KVB = kvblk(D);
    __align__(16) __bf16 k[2][KVB * D];    // [kv][d] swizzled
    __align__(16) __bf16 v[2][KVB * D];    // [kv][d] swizzled
    unsigned char kmask[2][KVB];
};

template <int D, bool SOFTCLAMP, bool PAIRED, bool BIAS = false>
__global__ __launch_bounds__(512, 2)   // 8-wave WGs need exactly 2 waves/SIMD:
void attn_bwd_dq_kernel(BwdParams p) { // cap 256 VGPR, stop the 220 B/thread
                                       // scratch spills seen at the 128 cap
    constexpr int DBLK = D / 32;
    constexpr int KSTEPS = D / 16;
    constexpr int DQ_KVBLK = kvblk(D);
    constexpr int DQ_NBLK = DQ_KVBLK / 32;

    __shared__ DqLds<D> lds;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int l31 = lane & 31;
    const int lhi = lane >> 5;

    const int bh = blockIdx.y;
    const int b = bh / p.h;
    const int h = bh % p.h;
    const int hk = h % p.hk;   // reference tile GQA pairing

    // causal pairing: WG x runs q-tiles (x, T-1-x) — uniform per-WG work
    const int n_pit = PAIRED
        ? (p.paired - 1 - (int)blockIdx.x == (int)blockIdx.x ? 1 : 2) : 1;
    for (int pit = 0; pit < n_pit; ++pit) {
    const int qtile = PAIRED
        ? (pit == 0 ? (int)blockIdx.x : p.paired - 1 - (int)blockIdx.x)
        : (p.desc ? p.desc[(long)blockIdx.x * 3] : (int)blockIdx.x);
    if (PAIRED && pit == 1) {
        __syncthreads();                       // LDS handoff between tiles
    }

    auto dq_body = [&]() {
    const BwdParams P = p;   // register-local copy (see noinline_call)
    const long i = (long)qtile * ROWS_WG + wid * 32 + l31;
    const bool row_valid = i < P.nq;
    const long ic = row_valid ? i : 0;

    // Q^T and dO^T fragments in registers (B-operand layout, lane = q)
    const __bf16* qbase = (const __bf16*)P.q + ((long)b * P.nq + ic) * P.h * D + (long)h * D;
    const __bf16* dobase = (const __bf16*)P.dout + ((long)b * P.nq + ic) * P.h * D + (long)h * D;
    bf16x8 qf[KSTEPS], dof[KSTEPS];
    #pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
        qf[ks] = *(const bf16x8*)(qbase + ks * 16 + lhi * 8);
        dof[ks] = *(const bf16x8*)(dobase + ks * 16 + lhi * 8);
    }
    const float lse_i = P.lse[((long)b * P.h + h) * P.nq + ic] * LOG2E;
    const float delta_i = P.delta[((long)b * P.h + h) * P.nq + ic];

    f32x16 dq_acc[DBLK];
    #pragma unroll
    for (int db = 0; db < DBLK; ++db) dq_acc[db] = f32x16{};

    // mask geometry (attn_mask.h): this workgroup's kv tile range
    const Mask M = mask_of(P);
    const long wg_i_min = (long)qtile * ROWS_WG;
    const long wg_i_max = min((long)(qtile + 1) * ROWS_WG, P.nq) - 1;
    const long wg_q_min = M.qpos(wg_i_min);
    const long wg_q_max = M.qpos(wg_i_max);
    const long qpos_i = M.qpos(i);
    TileRange tr = M.kv_tile_range(wg_i_min, wg_i_max, P.nk, DQ_KVBLK);
    if (P.split > 1) tr = split_share(tr, P.split, (int)blockIdx.z);
    if (!PAIRED && P.desc)       // descriptor mode: exact unit bounds
        tr = {P.desc[(long)blockIdx.x * 3 + 1], P.desc[(long)blockIdx.x * 3 + 2]};
    const int t_lo = tr.lo, t_hi = tr.hi;

    // staging: K + V row chunks, K^T pairs, running pointers
    constexpr int CH = D * 2 / 16;
    constexpr int KCHUNKS = DQ_KVBLK * CH;
    constexpr int KREGS = (KCHUNKS + 511) / 512;
    const __bf16* kbase = (const __bf16*)P.k + ((long)b * P.nk) * P.hk * D + (long)hk * D;
    const __bf16* vbase = (const __bf16*)P.v + ((long)b * P.nk) * P.hk * D + (long)hk * D;
    const unsigned char* mbase = P.kmask ? (const unsigned char*)P.kmask + (long)b * P.nk : nullptr;

    const long kv_row_stride = (long)P.hk * D;
    const long tile_stride = DQ_KVBLK * kv_row_stride;
    const __bf16* kptr = kbase + (long)t_lo * tile_stride
        + (tid / CH) * kv_row_stride + (tid % CH) * 8;
    const __bf16* vptr = vbase + (long)t_lo * tile_stride
        + (tid / CH) * kv_row_stride + (tid % CH) * 8;
    long j0_next = (long)t_lo * DQ_KVBLK;

    uint4 kst[KREGS], vst[KREGS];
    unsigned char mst = 1;

    auto load_tile = [&]() {
        const long j0 = j0_next;
        const long jmax = min(j0 + DQ_KVBLK, P.nk) - 1;
        const bool full = jmax - j0 == DQ_KVBLK - 1;
        #pragma unroll
        for (int r = 0; r < KREGS; ++r) {
            int c = tid + r * 512;
            if (c < KCHUNKS) {
                long off = (long)(r * (512 / CH)) * kv_row_stride;
                bool okr = full || (j0 + c / CH) <= jmax;
                kst[r] = okr ? *(const uint4*)(kptr + off) : uint4{0, 0, 0, 0};
                vst[r] = okr ? *(const uint4*)(vptr + off) : uint4{0, 0, 0, 0};
            }
        }
        if (mbase && tid < DQ_KVBLK)
            mst = (j0 + tid <= jmax) ? mbase[j0 + tid] : 0;
        kptr += tile_stride; vptr += tile_stride;
        j0_next += DQ_KVBLK;
    };

    auto write_tile = [&](int par) {
        #pragma unroll
        for (int r = 0; r < KREGS; ++r) {
            int c = tid + r * 512;
            if (c < KCHUNKS) {
                int row = c / CH, ch = c % CH;
                *(uint4*)(lds.k[par] + row * D + swz<D / 8>(row, ch) * 8) = kst[r];
                *(uint4*)(lds.v[par] + row * D + swz<D / 8>(row, ch) * 8) = vst[r];
            }
        }
        if (mbase && tid < DQ_KVBLK) lds.kmask[par][tid] = mst;
    };

    const float scale2 = P.scale * LOG2E;   // exp2 domain
    if (t_lo < t_hi) {
        load_tile();
        write_tile(t_lo & 1);
        if (t_lo + 1 < t_hi) load_tile();
    }

    for (int t = t_lo; t < t_hi; ++t) {
        const int par = t & 1;
        const long j0 = (long)t * DQ_KVBLK;
        const long jmax = min(j0 + DQ_KVBLK, P.nk) - 1;
        const bool full_tile = !BIAS &&
            (jmax - j0 == DQ_KVBLK - 1) &&
            M.uncut(wg_q_min, wg_q_max, j0, jmax) &&
            !P.kmask;

        __syncthreads();

        // s^T and dp^T computed PER 32-row BLOCK and packed immediately —
        // keeping all NBLK blocks' accumulators live (128 VGPRs) forced
        // scratch spills at the 256-register budget
        alignas(16) uint32_t pk[DQ_NBLK * 8];
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int kb = 0; kb < DQ_NBLK; ++kb) {
            f32x16 s = f32x16{}, dp = f32x16{};
            int krow = kb * 32 + l31;
            #pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) {
                int chunk = ks * 2 + lhi;
                bf16x8 kfr = *(const bf16x8*)(lds.k[par] + krow * D + swz<D / 8>(krow, chunk) * 8);
                bf16x8 vfr = *(const bf16x8*)(lds.v[par] + krow * D + swz<D / 8>(krow, chunk) * 8);
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr, qf[ks], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr, dof[ks], dp, 0, 0, 0);
            }
            if (full_tile && row_valid) {
                #pragma unroll
                for (int x2 = 0; x2 < 8; ++x2) {
                    float dse[2];
                    #pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        int r = 2 * x2 + e;
                        float x, dtanh = 1.f;
                        if constexpr (SOFTCLAMP) {
                            float inv_v = __builtin_amdgcn_rcpf(P.softclamp_value);
                            float th = fast_tanhf(s[r] * P.scale * inv_v);
                            x = P.softclamp_value * th * LOG2E;
                            dtanh = 1.f - th * th;
                        } else {
                            x = __builtin_fmaf(s[r], scale2, -lse_i);  // fold
                        }
                        float pv = __builtin_amdgcn_exp2f(SOFTCLAMP ? x - lse_i : x);
                        // the uniform softmax scale is applied once to the
                        // fp32 accumulators in the epilogue.  sub_f32 /
                        // mul_f32: single-issue, never v_pk_*_f32 beside
                        // the MFMAs (attn_common.h)
                        dse[e] = mul_f32(pv, sub_f32(dp[r], delta_i));
                        if constexpr (SOFTCLAMP) dse[e] = mul_f32(dse[e], dtanh);
                    }
                    pk[kb * 8 + x2] = pack_bf16x2(dse[0], dse[1]);
                }
            } else {
                #pragma unroll
                for (int x2 = 0; x2 < 8; ++x2) {
                    float dse[2];
                    #pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        int r = 2 * x2 + e;
                        long jj = j0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                        float x, dtanh = 1.f;
                        if constexpr (SOFTCLAMP) {
                            float inv_v = __builtin_amdgcn_rcpf(P.softclamp_value);
                            float th = fast_tanhf(s[r] * P.scale * inv_v);
                            x = P.softclamp_value * th * LOG2E;
                            dtanh = 1.f - th * th;
                        } else {
                            x = s[r] * scale2;
                        }
                        bool ok = row_valid && jj <= jmax;
                        if constexpr (BIAS) {
                            if (ok) {
                                const long bi = P.bias_mat
                                    ? (((long)b * P.h + h) * P.nq + ic) * P.nk + jj
                                    : ((long)b * P.h + h) * P.nk + jj;
                                x += P.bias[bi] * LOG2E;
                            }
                        }
                        ok = M.attends(qpos_i, jj, ok);
                        if (P.kmask) ok = ok && lds.kmask[par][jj - j0];
                        float pv = ok ? __builtin_amdgcn_exp2f(
                            SOFTCLAMP ? x - lse_i : x - lse_i) : 0.f;
                        dse[e] = mul_f32(pv, sub_f32(dp[r], delta_i));
                        if constexpr (SOFTCLAMP) dse[e] = mul_f32(dse[e], dtanh);
                    }
                    pk[kb * 8 + x2] = pack_bf16x2(dse[0], dse[1]);
                }
            }
        }
        __builtin_amdgcn_s_setprio(0);

        if (t + 1 < t_hi) write_tile(par ^ 1);
        if (t + 2 < t_hi) load_tile();

        // dq^T[d][q] += K^T[d][kv] x ds^T[kv][q].  The B fragment of k-step
        // ks (lane = q) is pk[4*ks .. 4*ks+3] as packed: its k order is
        // kv = ks*16 + 4*lhi + {0,1,2,3,8,9,10,11} (see kperm_pair), and the
        // K^T reads below pick their kv rows to match.  K^T A-fragments come
        // straight from the row-major swizzled k image via
        // ds_read_b64_tr_b16: lane f=l&15 of each 16-lane group fetches
        // K[kvq + (f>>2)][dg + 4*(f&3) ..+4] and the hardware
        // redistribution delivers out[l][j] = K[kvq + j][dg + (l&15)] —
        // i.e. lane l31 holds d column db*32 + l31, 4 kv per read.
        {
            const int f15 = lane & 15;
            const int g16 = (lane >> 4) & 1;
            const unsigned kb_lds = (unsigned)(uintptr_t)
                (__attribute__((address_space(3))) __bf16*)lds.k[par];
            __builtin_amdgcn_s_setprio(1);
            // issue ALL K^T tr-reads up front (asm loads cannot be software-
            // pipelined by the scheduler, so one batched wait beats a wait
            // per d-block), then run the whole MFMA stream.  The compiler-
            // visible form (__builtin_amdgcn_ds_read_tr16_b64_v4bf16, waits
            // placed by the scheduler) measured a tie with this one —
            // profiles/README.md "VALU diet" — so the batched form stays.
            unsigned long long ktr[DBLK][DQ_NBLK * 2][2];
            #pragma unroll
            for (int db = 0; db < DBLK; ++db) {
                const int dg = db * 32 + g16 * 16 + 4 * (f15 & 3);
                #pragma unroll
                for (int ks = 0; ks < DQ_NBLK * 2; ++ks) {
                    #pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        const int kv = ks * 16 + 4 * lhi + 8 * half + (f15 >> 2);
                        // swizzled element address of (kv, dg): 16B chunk
                        // c = dg/8 XORed with the row's swizzle key
                        const int c = (dg / 8) ^ (kv & (CH < 8 ? CH - 1 : 7));
                        const unsigned a = kb_lds
                            + (unsigned)(kv * (D * 2) + c * 16 + (dg % 8) * 2);
                        asm volatile("ds_read_b64_tr_b16 %0, %1"
                                     : "=&v"(ktr[db][ks][half]) : "v"(a) : "memory");
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            #pragma unroll
            for (int db = 0; db < DBLK; ++db)
                #pragma unroll
                for (int ks = 0; ks < DQ_NBLK * 2; ++ks) {
                    bf16x8 ktf;
                    *(unsigned long long*)&ktf = ktr[db][ks][0];
                    *((unsigned long long*)&ktf + 1) = ktr[db][ks][1];
                    dq_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        ktf, *(const bf16x8*)(pk + 4 * ks), dq_acc[db], 0, 0, 0);
                }
            __builtin_amdgcn_s_setprio(0);
        }
    }

    if (!row_valid) return;
    // the softmax scale, a uniform factor of ds, was left out of the hot
    // loop: apply it once to this launch's finished fp32 partial, ahead of
    // every output mode (exact for power-of-two scales)
    #pragma unroll
    for (int db = 0; db < DBLK; ++db)
        #pragma unroll
        for (int r = 0; r < 16; ++r) dq_acc[db][r] = mul_f32(dq_acc[db][r], P.scale);
    if (P.dq_bf) {
        // fused epilogue (single-pass only, enforced by the binding): this
        // lane is the unique writer of its row, so round the finished fp32
        // value (RNE) and store bf16 at its final address — regs 4g..4g+3
        // are 4 consecutive d, one 8-byte store each
        __bf16* dqb = (__bf16*)P.dq_bf + ((long)b * P.nq + i) * P.h * D + (long)h * D;
        #pragma unroll
        for (int db = 0; db < DBLK; ++db)
            #pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v4 = {dq_acc[db][4 * g], dq_acc[db][4 * g + 1],
                            dq_acc[db][4 * g + 2], dq_acc[db][4 * g + 3]};
                *(bf16x4*)(dqb + db * 32 + 8 * g + 4 * lhi) =
                    __builtin_convertvector(v4, bf16x4);
            }
        return;
    }
    // epilogue: dq (B, Nq, H, D) fp32; unique writer per row unless the kv
    // walk is split across grid.z (then fp32 atomics, contention = split)
    float* dqp = P.dq + ((long)b * P.nq + i) * P.h * D + (long)h * D;
    #pragma unroll
    for (int db = 0; db < DBLK; ++db)
        #pragma unroll
        for (int r = 0; r < 16; ++r) {
            int d = db * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
            if (P.split > 1 || P.desc) atomicAdd(dqp + d, dq_acc[db][r]);
            else if (P.accumulate) dqp[d] += dq_acc[db][r];
            else dqp[d] = dq_acc[db][r];
        }
    };
    // measured: the noinline frame REGRESSES d128-PAIRED dq (105 vs 123 TF)
    // unlike fwd/dkv, but the lambda restructure itself (register-local P
    // copy) lifts d128-plain (200 -> 207) — keep the body direct-called.
    dq_body();
    }  // pair loop
}

// ---------------------------------------------------------------------------
// dk/dv kernel: column-parallel, K/V resident in registers
// ---------------------------------------------------------------------------
static constexpr int KVROWS_WAVE = 32;   // 8 waves own the ROWS_WG kv rows
static_assert(ROWS_WG == 8 * KVROWS_WAVE);

// SINGLE_IMAGE (d32, d64): Q and dO are staged once, row-major; the dv/dk
// MFMAs take their transposed operands from the same images with
// ds_read_b64_tr_b16 (as dq takes K^T from its k image).  d128 keeps the
// second, pair-staged transposed pair of images.
template <int D, int QT, bool SINGLE_IMAGE>
struct DkvLds {
    // double-buffered q-tile images (one barrier per q tile; staging writes
    // and next-next tile's loads overlap the MFMAs, as in the forward kernel)
    __align__(16) __bf16 q[2][QT * D];      // [q][d]   swizzled rows
    __align__(16) __bf16 qt[2][D * QT];     // [d][q]   pair-staged transpose
    __align__(16) __bf16 do_[2][QT * D];    // [q][d]
    __align__(16) __bf16 dot[2][D * QT];    // [d][q]
    __align__(16) float lse[2][QT];
    __align__(16) float delta[2][QT];
};

template <int D, int QT>
struct DkvLds<D, QT, true> {
    __align__(16) __bf16 q[2][QT * D];      // [q][d]   swizzled rows
    __align__(16) __bf16 do_[2][QT * D];    // [q][d]
    __align__(16) float lse[2][QT];
    __align__(16) float delta[2][QT];
    // the bf16 epilogue stages 2 x ROWS_WG x D values through this
    // allocation, more than the images take: the difference stays allocated
    // (registers, not LDS, hold occupancy at one workgroup per CU)
    __align__(16) __bf16 epilogue_room[2 * ROWS_WG * D - 4 * QT * D];
    static_assert(2 * ROWS_WG * D > 4 * QT * D);
};


// staging registers of the transposed images' row pairs: the two-image form
// has them, the single-image form has none
template <int TREGS, bool TWO_IMAGE>
struct DkvTrStage {
    bf16x8 q_a[TREGS], q_b[TREGS], do_a[TREGS], do_b[TREGS];
};
template <int TREGS>
struct DkvTrStage<TREGS, false> {};

template <int D, int QT, bool SOFTCLAMP, bool PAIRED, bool BIAS = false>
__global__ __launch_bounds__(512, 2)   // see dq kernel note (552 B spills)
void attn_bwd_dkv_kernel(BwdParams p) {
    static_assert(D % 32 == 0 && QT % 32 == 0);
    constexpr int DBLK = D / 32;
    constexpr int KSTEPS = D / 16;
    constexpr int QBLKS = QT / 32;
    constexpr int TM = (QT / 8 - 1) < 7 ? (QT / 8 - 1) : 7;

    // d32 / d64 stage one row-major image per operand (see DkvLds); d128 has
    // not been measured in that form and keeps two
    constexpr bool SINGLE_IMAGE = (D != 128);
    __shared__ DkvLds<D, QT, SINGLE_IMAGE> lds;

    // the d64 body runs in a noinline frame (see the call below) and keeps
    // its wave-uniform state in SGPRs: it captures nothing
    constexpr bool FRAME = (D == 64);
    // explicit LDS operand prefetch in the tile loop: d64 only (d128 has no
    // registers for it, its tile loop already spills)
    constexpr bool PREFETCH = (D == 64);

    // causal pairing (mirrored): kv-tile x attends T-x q-tiles, so WG x
    // runs kv-tiles (x, T-1-x) for uniform per-WG work
    const int n_pit = PAIRED
        ? (p.paired - 1 - (int)blockIdx.x == (int)blockIdx.x ? 1 : 2) : 1;
    for (int pit = 0; pit < n_pit; ++pit) {
    const int kvtile_wg = PAIRED
        ? (pit == 0 ? (int)blockIdx.x : p.paired - 1 - (int)blockIdx.x)
        : (p.desc ? p.desc[(long)blockIdx.x * 3] : (int)blockIdx.x);
    if (PAIRED && pit == 1) {
        __syncthreads();                       // LDS handoff between tiles
    }

    auto dkv_body = [&](int kvtile_arg, unsigned long long kernarg) {
    // FRAME: the parameters come by scalar loads from the kernarg segment and
    // the workgroup / wave coordinates are re-derived here, so pointers, tile
    // bounds, loop counters and mask integers are scalar and the tile loop's
    // back-edge is a scalar branch.  Per-lane: tid, lane, l31, lhi and what derives from
    // them (j, jc, col_valid, kmask_own).
    const BwdParams P = [&] {
        if constexpr (FRAME) {
            BwdParams kp = kernarg_params<BwdParams>(kernarg);
            kp.q = as_global(kp.q);         kp.k = as_global(kp.k);
            kp.v = as_global(kp.v);         kp.dout = as_global(kp.dout);
            kp.kmask = as_global(kp.kmask); kp.lse = as_global(kp.lse);
            kp.delta = as_global(kp.delta); kp.dk = as_global(kp.dk);
            kp.dv = as_global(kp.dv);       kp.dk_bf = as_global(kp.dk_bf);
            kp.dv_bf = as_global(kp.dv_bf); kp.bias = as_global(kp.bias);
            kp.desc = as_global(kp.desc);
            return kp;
        } else {
            return p;            // register-local copy
        }
    }();
    const int kvtile = uniform<FRAME>(kvtile_arg);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = uniform<FRAME>(tid >> 6);
    const int l31 = lane & 31;
    const int lhi = lane >> 5;
    const int bhk = blockIdx.y;
    const int b = bhk / P.hk;
    const int hkh = bhk % P.hk;

    const long j0_wg = (long)kvtile * ROWS_WG;
    const long jmax = min(j0_wg + ROWS_WG, P.nk) - 1;
    const long j = j0_wg + wid * KVROWS_WAVE + l31;
    const bool col_valid = j <= jmax;
    const long jc = col_valid ? j : j0_wg;

    const __bf16* kb = (const __bf16*)P.k + ((long)b * P.nk + jc) * P.hk * D + (long)hkh * D;
    const __bf16* vb = (const __bf16*)P.v + ((long)b * P.nk + jc) * P.hk * D + (long)hkh * D;
    bf16x8 kf[KSTEPS], vf[KSTEPS];
    #pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
        kf[ks] = *(const bf16x8*)(kb + ks * 16 + lhi * 8);
        vf[ks] = *(const bf16x8*)(vb + ks * 16 + lhi * 8);
    }
    unsigned char kmask_own = 1;
    if (P.kmask) kmask_own = col_valid ? ((const unsigned char*)P.kmask)[(long)b * P.nk + j] : 0;

    f32x16 dv_acc[DBLK], dk_acc[DBLK];
    #pragma unroll
    for (int db = 0; db < DBLK; ++db) { dv_acc[db] = f32x16{}; dk_acc[db] = f32x16{}; }
    const float scale2 = P.scale * LOG2E;   // exp2 domain

    const Mask M = mask_of(P);

    // K/V fragments land here, once (vmcnt(0), other counters untouched).
    // Left in flight into the tile loop, the compiler's wait insertion sees
    // them pending on the path around the loop prologue and guards the S/dP
    // MFMAs, which read them, with counted vmcnt waits in EVERY iteration;
    // in steady state those counts hold the MFMAs back for the q-tile
    // global loads issued a few instructions earlier.
    if constexpr (FRAME) __builtin_amdgcn_s_waitcnt(0x0F70);

    for (int g = 0; g < P.group; ++g) {
        // group boundary barrier: the previous group's last tile is still
        // being read from LDS by slower waves when this group's prologue
        // write_qtile targets the same buffer (GQA-only race; widest at
        // split>1 where a chunk is a single tile)
        if (g > 0) __syncthreads();
        const int h = hkh + g * P.hk;   // reference tile GQA: group g's q head
        const float* lse_row = P.lse + ((long)b * P.h + h) * P.nq;
        const float* delta_row = P.delta + ((long)b * P.h + h) * P.nq;
        const __bf16* qg = (const __bf16*)P.q + ((long)b * P.nq) * P.h * D + (long)h * D;
        const __bf16* dog = (const __bf16*)P.dout + ((long)b * P.nq) * P.h * D + (long)h * D;

        // mask geometry (attn_mask.h): the q tiles this workgroup's keys
        // are attended from; grid.z takes a share of that walk
        TileRange tr = M.q_tile_range(j0_wg, jmax, P.nq, QT);
        if (P.split > 1) tr = split_share(tr, P.split, (int)blockIdx.z);
        if (!PAIRED && P.desc)     // descriptor mode: exact unit bounds
            tr = {uniform<FRAME>(P.desc[(long)blockIdx.x * 3 + 1]),
                  uniform<FRAME>(P.desc[(long)blockIdx.x * 3 + 2])};
        const int t0 = tr.lo, t1 = tr.hi;

        // ---- T14 pipeline: per-thread staging registers
        constexpr int CH = D * 2 / 16;
        constexpr int QCHUNKS = QT * CH;
        constexpr int QREGS = (QCHUNKS + 511) / 512;
        constexpr int TPAIRS = (QT / 2) * (D / 8);
        constexpr int TREGS = (TPAIRS + 511) / 512;
        uint4 qst[QREGS], dost[QREGS];
        DkvTrStage<TREGS, !SINGLE_IMAGE> trs;
        float lse_st = 0.f, delta_st = 0.f;
        long t_next = t0;

        // Global loads of a q tile.  Addresses are a scalar tile base plus a
        // 32-bit per-lane BYTE offset (the saddr + voffset form: one VGPR per
        // access pattern, not a 64-bit pointer per access).  Every load is
        // unconditional: a row past the end of a ragged last tile reads the
        // tile's last valid row instead and is zeroed when the tile is
        // written to LDS (write_qtile).  A `valid ? load : 0` here puts a
        // zero write to the staging register in front of each load, and that
        // write waits for EVERY global load in flight, once per tile, in
        // the tile loop; likewise the lse product waits for its own load, so
        // it is taken at write time too.
        const unsigned qrow_bytes = (unsigned)(P.h * D) * 2u;
        auto ld16 = [](const __bf16* base, unsigned boff) {
            return *(const uint4*)((const char*)base + boff);
        };
        auto ld8h = [](const __bf16* base, unsigned boff) {
            return *(const bf16x8*)((const char*)base + boff);
        };
        auto tile_rows = [&](long tile) {                      // valid q rows
            return (int)(min((tile + 1) * QT, P.nq) - tile * QT);
        };
        auto load_qtile = [&](int tid) {
            const long i0 = t_next * QT;
            const int last = tile_rows(t_next) - 1;
            const __bf16* qtile = qg + i0 * P.h * D;
            const __bf16* dotile = dog + i0 * P.h * D;
            #pragma unroll
            for (int r = 0; r < QREGS; ++r) {
                int c = tid + r * 512;
                if (c < QCHUNKS) {
                    int lr = min(c / CH, last);
                    int ch = c % CH;
                    unsigned off = (unsigned)lr * qrow_bytes + ch * 16;
                    qst[r] = ld16(qtile, off);
                    dost[r] = ld16(dotile, off);
                }
            }
            if constexpr (!SINGLE_IMAGE) {
                #pragma unroll
                for (int r = 0; r < TREGS; ++r) {
                    int c = tid + r * 512;
                    if (c < TPAIRS) {
                        int jp = c % (QT / 2);
                        int d0 = (c / (QT / 2)) * 8;
                        unsigned offa = (unsigned)min(jp * 2, last) * qrow_bytes + d0 * 2;
                        unsigned offb = (unsigned)min(jp * 2 + 1, last) * qrow_bytes + d0 * 2;
                        trs.q_a[r] = ld8h(qtile, offa);
                        trs.q_b[r] = ld8h(qtile, offb);
                        trs.do_a[r] = ld8h(dotile, offa);
                        trs.do_b[r] = ld8h(dotile, offb);
                    }
                }
            }
            if (tid < QT) {
                long gi = i0 + min(tid, last);
                lse_st = lse_row[gi];
                delta_st = delta_row[gi];
            }
            ++t_next;
        };

        // `tile` is the q tile held in the staging registers
        auto write_qtile = [&](int par, int tid, long tile) {
            const int rows = tile_rows(tile);
            if (rows < QT) {       // ragged last tile: rows past the end are 0
                #pragma unroll
                for (int r = 0; r < QREGS; ++r)
                    if ((tid + r * 512) / CH >= rows) {
                        qst[r] = uint4{0, 0, 0, 0};
                        dost[r] = uint4{0, 0, 0, 0};
                    }
                if constexpr (!SINGLE_IMAGE) {
                    #pragma unroll
                    for (int r = 0; r < TREGS; ++r) {
                        int la = ((tid + r * 512) % (QT / 2)) * 2;
                        if (la >= rows) { trs.q_a[r] = bf16x8{}; trs.do_a[r] = bf16x8{}; }
                        if (la + 1 >= rows) { trs.q_b[r] = bf16x8{}; trs.do_b[r] = bf16x8{}; }
                    }
                }
            }
            #pragma unroll
            for (int r = 0; r < QREGS; ++r) {
                int c = tid + r * 512;
                if (c < QCHUNKS) {
                    int row = c / CH, ch = c % CH;
                    *(uint4*)(lds.q[par] + row * D + swz<D / 8>(row, ch) * 8) = qst[r];
                    *(uint4*)(lds.do_[par] + row * D + swz<D / 8>(row, ch) * 8) = dost[r];
                }
            }
            if constexpr (!SINGLE_IMAGE) {
                #pragma unroll
                for (int r = 0; r < TREGS; ++r) {
                    int c = tid + r * 512;
                    if (c < TPAIRS) {
                        // q pairs land in the dv/dk k order (kperm_pair): the
                        // packed p/ds pairs are then the fragments as they stand
                        int jp = kperm_pair(c % (QT / 2));
                        int d0 = (c / (QT / 2)) * 8;
                        // element (d0 + e, pair jp) sits at byte
                        //   (d0 + e) * QT * 2 + ((jp * 4) ^ (((d0 + e) & TM) << 4))
                        // of image `par`.  d0 % 8 == 0, so the swizzle term is
                        // (e & TM) << 4; it is below the QT * 2 row size and the
                        // buffer and row-group offsets have those bits clear, so
                        // the XOR applies to the whole address: one base
                        // register and one v_xor per store instead of eight
                        // loop-invariant addresses held (and spilled) across
                        // the tile loop
                        static_assert((TM << 4) < QT * 2 && (D * QT * 2) % (QT * 2) == 0);
                        const unsigned base = par * (D * QT * 2) + d0 * QT * 2 + jp * 4;
                        #pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            unsigned byte_off = (base ^ ((e & TM) << 4)) + e * QT * 2;
                            __bf16 pq[2] = {trs.q_a[r][e], trs.q_b[r][e]};
                            __bf16 pd[2] = {trs.do_a[r][e], trs.do_b[r][e]};
                            *(uint32_t*)((char*)lds.qt[0] + byte_off) = *(uint32_t*)pq;
                            *(uint32_t*)((char*)lds.dot[0] + byte_off) = *(uint32_t*)pd;
                        }
                    }
                }
            }
            if (tid < QT) {
                const bool okl = tid < rows;
                // exp2-domain lse: one product per q row here, not one per
                // lane per element in the hot loop (same fp32 product)
                lds.lse[par][tid] = okl ? lse_st * LOG2E : 0.f;
                lds.delta[par][tid] = okl ? delta_st : 0.f;
            }
        };

        if (t0 < t1) {
            load_qtile(tid);
            write_qtile(t0 & 1, tid, t0);
            if (t0 + 1 < t1) load_qtile(tid);
        }

        for (int t = t0; t < t1; ++t) {
            const int par = t & 1;
            const long i0 = (long)t * QT;
            const long imax = min(i0 + QT, P.nq) - 1;
            const bool full_tile = !BIAS &&
                (imax - i0 == QT - 1) &&
                M.uncut(M.qpos(i0), M.qpos(imax), j0_wg, jmax) &&
                !P.kmask;

            // MFMA operand fragments of one 32-row q block: the S/dP pair
            // (rows of the q / dO images) and the dv/dk pair (SINGLE_IMAGE:
            // columns of the same images, read transposed; else rows of
            // the transposed images)
            bf16x8 qa[KSTEPS], da[KSTEPS], doa[2 * DBLK], qta[2 * DBLK];
            auto read_sdp = [&](int qb) {
                #pragma unroll
                for (int ks = 0; ks < KSTEPS; ++ks) {
                    int qrow = qb * 32 + l31;
                    int chunk = ks * 2 + lhi;
                    qa[ks] = *(const bf16x8*)(lds.q[par] + qrow * D + swz<D / 8>(qrow, chunk) * 8);
                    da[ks] = *(const bf16x8*)(lds.do_[par] + qrow * D + swz<D / 8>(qrow, chunk) * 8);
                }
            };
            // SINGLE_IMAGE: dO^T / Q^T fragments straight from the row-major
            // images.  Fragment db*2+half holds, for d column db*32 + l31,
            // q rows qb*32 + 16*half + 4*lhi + {0,1,2,3, 8,9,10,11} (the k
            // order of the packed p/ds pairs, kperm_pair): two transposed
            // reads of 4 consecutive rows, u = 0, 1.  Lane f = lane & 15 of
            // each 16-lane group g16 addresses row + (f >> 2), columns
            // db*32 + 16*g16 + 4*(f & 3) .. +4, and the hardware delivers
            // out[l][e] = image[row + e][db*32 + (l & 31)].  Every row
            // term but 4*lhi + (f >> 2) is a multiple of 8, so the swizzle
            // key (row & 7) is per lane and each read is a per-lane base
            // plus a compile-time offset (the base of db 1 is db 0's with
            // the 64-byte bit flipped).
            auto read_dvdk_tr = [&](int qb) {
                typedef __attribute__((address_space(3))) bf16x4* lds_v4;
                const int f15 = lane & 15;
                const int g16 = (lane >> 4) & 1;
                const int lrow = 4 * lhi + (f15 >> 2);
                const int key = lrow & (D / 8 < 8 ? D / 8 - 1 : 7);
                #pragma unroll
                for (int db = 0; db < DBLK; ++db) {
                    const int col = db * 32 + 16 * g16 + 4 * (f15 & 3);
                    const int lane_off = lrow * D + ((col / 8) ^ key) * 8 + (col % 8);
                    #pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        bf16x4 dv4[2], qv4[2];
                        #pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const int off = (qb * 32 + 16 * half + 8 * u) * D + lane_off;
                            dv4[u] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                                (lds_v4)(lds.do_[par] + off));
                            qv4[u] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                                (lds_v4)(lds.q[par] + off));
                        }
                        doa[db * 2 + half] = __builtin_shufflevector(
                            dv4[0], dv4[1], 0, 1, 2, 3, 4, 5, 6, 7);
                        qta[db * 2 + half] = __builtin_shufflevector(
                            qv4[0], qv4[1], 0, 1, 2, 3, 4, 5, 6, 7);
                    }
                }
            };
            auto read_dvdk = [&](int qb) {
                if constexpr (SINGLE_IMAGE) {
                    read_dvdk_tr(qb);
                } else {
                    #pragma unroll
                    for (int db = 0; db < DBLK; ++db)
                        #pragma unroll
                        for (int half = 0; half < 2; ++half) {
                            int qk = qb * 2 + half;
                            int drow = db * 32 + l31;
                            int ch = qk * 2 + lhi;
                            doa[db * 2 + half] = *(const bf16x8*)(lds.dot[par] + drow * QT +
                                                                  ((ch ^ (drow & TM))) * 8);
                            qta[db * 2 + half] = *(const bf16x8*)(lds.qt[par] + drow * QT +
                                                                  ((ch ^ (drow & TM))) * 8);
                        }
                }
            };

            // masked path: the lane's half offset and its one 64-bit q
            // position per tile.  Both are made opaque: left visible, the
            // per-register terms are folded back into 32 loop-invariant
            // per-lane products that live in scratch
            const int rows_m1 = (int)(imax - i0);            // last valid tile row
            int lhi4 = 4 * lhi;
            asm volatile("" : "+v"(lhi4));
            long qp_lane = M.qpos(i0 + lhi4);
            asm volatile("" : "+v"(qp_lane));

            __syncthreads();

            // PREFETCH: each batch of LDS reads is issued one block of work
            // ahead of the MFMAs that consume it, and pinned there (the
            // scheduler otherwise sinks every read to just above its MFMA,
            // where both waves of the SIMD wait out the round trip together):
            //   barrier | S/dP reads of q block 0 | staging of tile t+1
            //   per q block: S/dP MFMAs | dv/dk reads | softmax, ds
            //              | S/dP reads of the next q block | dv/dk MFMAs
            // Nothing is read from image `par` ahead of the barrier above.
            if constexpr (PREFETCH) {
                read_sdp(0);
                __builtin_amdgcn_sched_barrier(0);
            }

            // the staging addresses are a few VALU ops from tid.  Left
            // loop-invariant they are hoisted, spilled under the loop's
            // register pressure and reloaded from scratch just ahead of
            // their use, one exposed memory round trip each per tile; the
            // empty asm makes tid opaque so they are rebuilt in the loop
            int tid_l = tid;
            if constexpr (FRAME) asm volatile("" : "+v"(tid_l));
            if (t + 1 < t1) write_qtile(par ^ 1, tid_l, t + 1);
            if (t + 2 < t1) load_qtile(tid_l);

            #pragma unroll
            for (int qb = 0; qb < QBLKS; ++qb) {
                // S2[q][kv], dP[q][kv]: lane = kv, q rows in regs
                f32x16 s2 = f32x16{}, dp = f32x16{};
                if constexpr (!PREFETCH) read_sdp(qb);
                #pragma unroll
                for (int ks = 0; ks < KSTEPS; ++ks) {
                    s2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[ks], kf[ks], s2, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da[ks], vf[ks], dp, 0, 0, 0);
                }
                // the first row group's lse / delta go ahead of the dv/dk
                // batch: the softmax block starts on them
                f32x4 lse_g0 = f32x4{}, delta_g0 = f32x4{};
                if constexpr (PREFETCH) {
                    lse_g0 = *(const f32x4*)(lds.lse[par] + qb * 32 + 4 * lhi);
                    delta_g0 = *(const f32x4*)(lds.delta[par] + qb * 32 + 4 * lhi);
                    read_dvdk(qb);
                    __builtin_amdgcn_sched_barrier(0);
                }

                alignas(16) uint32_t p_pk[8], ds_pk[8];
                if (full_tile && col_valid) {
                    #pragma unroll
                    for (int x2 = 0; x2 < 8; ++x2) {
                        float pe[2], dse[2];
                        // per-group wide loads (8 live regs, not 32): regs
                        // 4g..4g+3 are consecutive qloc -> one b128 each
                        f32x4 lse4, delta4;
                        if (PREFETCH && (x2 >> 1) == 0) {
                            lse4 = lse_g0;
                            delta4 = delta_g0;
                        } else {
                            int base = qb * 32 + 8 * (x2 >> 1) + 4 * lhi;
                            lse4 = *(const f32x4*)(lds.lse[par] + base);
                            delta4 = *(const f32x4*)(lds.delta[par] + base);
                        }
                        #pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            int r = 2 * x2 + e;
                            float x, dtanh = 1.f;
                            if constexpr (SOFTCLAMP) {
                                float inv_v = __builtin_amdgcn_rcpf(P.softclamp_value);
                                float th = fast_tanhf(s2[r] * P.scale * inv_v);
                                x = P.softclamp_value * th * LOG2E;
                                dtanh = 1.f - th * th;
                            } else {
                                x = __builtin_fmaf(s2[r], scale2, -lse4[r & 3]);  // fold
                            }
                            float pv = __builtin_amdgcn_exp2f(SOFTCLAMP ? x - lse4[r & 3] : x);
                            pe[e] = pv;
                            // the uniform softmax scale is applied once to
                            // dk's fp32 accumulators in the epilogue
                            dse[e] = mul_f32(pv, sub_f32(dp[r], delta4[r & 3]));
                            if constexpr (SOFTCLAMP) dse[e] = mul_f32(dse[e], dtanh);
                        }
                        p_pk[x2] = pack_bf16x2(pe[0], pe[1]);
                        ds_pk[x2] = pack_bf16x2(dse[0], dse[1]);
                    }
                } else {
                    #pragma unroll
                    for (int x2 = 0; x2 < 8; ++x2) {
                        float pe[2], dse[2];
                        // per-group wide loads (8 live regs, not 32): regs
                        // 4g..4g+3 are consecutive qloc -> one b128 each
                        f32x4 lse4, delta4;
                        if (PREFETCH && (x2 >> 1) == 0) {
                            lse4 = lse_g0;
                            delta4 = delta_g0;
                        } else {
                            int base = qb * 32 + 8 * (x2 >> 1) + 4 * lhi;
                            lse4 = *(const f32x4*)(lds.lse[par] + base);
                            delta4 = *(const f32x4*)(lds.delta[par] + base);
                        }
                        #pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            int r = 2 * x2 + e;
                            // q row of register r: a compile-time row cr of
                            // the tile plus the lane's half offset.  The
                            // row test is 32-bit against the tile's row
                            // count and qpos(i) is the lane's one 64-bit
                            // base plus the SCALAR cr * q_stride: the same
                            // integers as qpos(i0 + qloc), without 32
                            // per-lane 64-bit products held (spilled)
                            // across the tile loop
                            const int cr = qb * 32 + (r & 3) + 8 * (r >> 2);
                            const int qloc = cr + lhi4;
                            float x, dtanh = 1.f;
                            if constexpr (SOFTCLAMP) {
                                float inv_v = __builtin_amdgcn_rcpf(P.softclamp_value);
                                float th = fast_tanhf(s2[r] * P.scale * inv_v);
                                x = P.softclamp_value * th * LOG2E;
                                dtanh = 1.f - th * th;
                            } else {
                                x = s2[r] * scale2;
                            }
                            bool ok = col_valid && qloc <= rows_m1;
                            if constexpr (BIAS) {
                                if (ok) {
                                    const long i = i0 + qloc;
                                    const long bi = P.bias_mat
                                        ? (((long)b * P.h + h) * P.nq + i) * P.nk + j
                                        : ((long)b * P.h + h) * P.nk + j;
                                    x += P.bias[bi] * LOG2E;
                                }
                            }
                            ok = M.attends(qp_lane + (long)cr * M.q_stride, j, ok);
                            if (P.kmask) ok = ok && kmask_own;
                            float pv = ok ? __builtin_amdgcn_exp2f(x - lse4[r & 3]) : 0.f;
                            pe[e] = pv;
                            dse[e] = mul_f32(pv, sub_f32(dp[r], delta4[r & 3]));
                            if constexpr (SOFTCLAMP) dse[e] = mul_f32(dse[e], dtanh);
                        }
                        p_pk[x2] = pack_bf16x2(pe[0], pe[1]);
                        ds_pk[x2] = pack_bf16x2(dse[0], dse[1]);
                    }
                }

                // dv^T[d][kv] += dO^T x p ; dk[kv][d] += ds^T x Q^T-read.
                // p_pk/ds_pk[4*half .. 4*half+3] (lane = kv) are the
                // fragments of k-step `half` as packed: q rows
                // 16*half + 4*lhi + {0,1,2,3,8,9,10,11}: the rows the
                // transposed reads pick (read_dvdk_tr) and the order the
                // qt/dot images of the two-image form are staged in
                // (kperm_pair)
                if constexpr (PREFETCH) {
                    if (qb + 1 < QBLKS) {
                        read_sdp(qb + 1);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                } else {
                    read_dvdk(qb);
                }
                #pragma unroll
                for (int db = 0; db < DBLK; ++db)
                    #pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        dv_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                            doa[db * 2 + half], *(const bf16x8*)(p_pk + 4 * half), dv_acc[db], 0, 0, 0);
                        dk_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                            *(const bf16x8*)(ds_pk + 4 * half), qta[db * 2 + half], dk_acc[db], 0, 0, 0);
                    }
            }
        }
    }

    // the softmax scale, a uniform factor of ds, was left out of the hot
    // loop: apply it once to this launch's finished fp32 dk partial, ahead
    // of every output mode (exact for power-of-two scales)
    #pragma unroll
    for (int db = 0; db < DBLK; ++db)
        #pragma unroll
        for (int r = 0; r < 16; ++r) dk_acc[db][r] = mul_f32(dk_acc[db][r], P.scale);

    if (P.dk_bf) {
        // fused epilogue (single-pass only, enforced by the binding): this
        // WG is the unique writer of its 256 kv rows, so round the finished
        // fp32 values (RNE) and store bf16 in the caller's (B,Nk,HK,D)
        // layout.  dk lanes own a d COLUMN (2-byte direct stores), so the
        // tile is transposed through the Q/dO LDS images, which are dead
        // once every wave has left the last q tile: [256][D] bf16 dk, then
        // [256][D] bf16 dv (2 x 32 KB at d64 of the 65 KB allocated), same
        // 16-byte-chunk XOR swizzle as the staged images.  Each wave writes
        // and reads back only its own 32 rows; rows leave as 16-byte stores.
        // (dv could leave straight from registers, 8 B per lane: measured
        // equal at the headline shape — docs/KERNELS.md §2 — so both
        // tensors share the one staged store loop.)
        constexpr int ECH = D / 8;
        __bf16* stg_dk = (__bf16*)&lds;
        __bf16* stg_dv = stg_dk + ROWS_WG * D;
        static_assert(sizeof(DkvLds<D, QT, SINGLE_IMAGE>) >= 2 * ROWS_WG * D * sizeof(__bf16));
        const int wrow0 = wid * KVROWS_WAVE;
        const long orow_stride = (long)P.hk * D;
        __bf16* dkb = (__bf16*)P.dk_bf + ((long)b * P.nk) * orow_stride + (long)hkh * D;
        __bf16* dvb = (__bf16*)P.dv_bf + ((long)b * P.nk) * orow_stride + (long)hkh * D;
        __syncthreads();                       // last tile's readers are done
        #pragma unroll
        for (int db = 0; db < DBLK; ++db)
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                int row = wrow0 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                int d = db * 32 + l31;
                stg_dk[row * D + swz<ECH>(row, d / 8) * 8 + (d & 7)] = (__bf16)dk_acc[db][r];
            }
        {
            // dv^T regs 4g..4g+3 are 4 consecutive d of this lane's kv row
            const int row = wrow0 + l31;
            #pragma unroll
            for (int db = 0; db < DBLK; ++db)
                #pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v4 = {dv_acc[db][4 * g], dv_acc[db][4 * g + 1],
                                dv_acc[db][4 * g + 2], dv_acc[db][4 * g + 3]};
                    *(bf16x4*)(stg_dv + row * D + swz<ECH>(row, db * 4 + g) * 8 + 4 * lhi) =
                        __builtin_convertvector(v4, bf16x4);
                }
        }
        __syncthreads();
        #pragma unroll
        for (int c = lane; c < KVROWS_WAVE * ECH; c += 64) {
            int row = wrow0 + c / ECH, ch = c % ECH;
            long kvrow = j0_wg + row;
            if (kvrow <= jmax) {
                int so = row * D + swz<ECH>(row, ch) * 8;
                *(uint4*)(dkb + kvrow * orow_stride + ch * 8) = *(const uint4*)(stg_dk + so);
                *(uint4*)(dvb + kvrow * orow_stride + ch * 8) = *(const uint4*)(stg_dv + so);
            }
        }
    } else {
        // write dk (B,HK,Nk,D) and dv^T (B,HK,D,Nk).  dk: the lane owns a d
        // COLUMN of all 32 kv rows of its wave, so only the row guard
        // applies (gating on the lane's own kv row left columns of a
        // partially valid wave unwritten when Nk % 32 != 0)
        float* dkb = P.dk + (((long)b * P.hk + hkh) * P.nk) * D;
        #pragma unroll
        for (int db = 0; db < DBLK; ++db)
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                long kvrow = j0_wg + wid * KVROWS_WAVE + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                int d = db * 32 + l31;
                if (kvrow <= jmax) {
                    float* dst = dkb + kvrow * D + d;
                    if (P.split > 1 || P.desc) atomicAdd(dst, dk_acc[db][r]);
                    else if (P.accumulate) *dst += dk_acc[db][r];
                    else *dst = dk_acc[db][r];
                }
            }
        float* dvb = P.dv + (((long)b * P.hk + hkh) * D) * P.nk;
        if (col_valid)
        #pragma unroll
        for (int db = 0; db < DBLK; ++db)
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                int d = db * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                float* dst = dvb + (long)d * P.nk + j;
                if (P.split > 1 || P.desc) atomicAdd(dst, dv_acc[db][r]);
                else if (P.accumulate) *dst += dv_acc[db][r];
                else *dst = dv_acc[db][r];
            }
    }
    };
    // the noinline frame confines register allocation to the body — at d64
    // it cuts the hot-loop spills roughly in half for BOTH instantiations
    // (measured headline +4%, causal +17-24%); d128 is better DIRECT for
    // both forms (paired: 125 -> 138 TF causal 8k — the same value-copy
    // preference as the d128 fwd/dq bodies), so only d64 takes the call
    if constexpr (FRAME) noinline_call(dkv_body, kvtile_wg, kernarg_address());
    else dkv_body(kvtile_wg, 0ull);
    }  // pair loop
}

void launch_attn_bwd_dq(const BwdParams& p, int head_dim, hipStream_t stream) {
    dim3 block(512);
    int z = p.split > 1 ? p.split : 1;
    long qt_ = ceil_div(p.nq, ROWS_WG);
    if (p.desc) qt_ = p.n_units;
    else if (p.paired) qt_ = (qt_ + 1) / 2;
    dim3 grid_dq(qt_, p.b * p.h, z);
    const bool pr = p.paired > 0;
    if (p.bias) {   // bias runs unpaired (bindings force paired=0)
        if (head_dim == 64) {
            if (p.softclamp) hipLaunchKernelGGL((attn_bwd_dq_kernel<64, true, false, true>), grid_dq, block, 0, stream, p);
            else hipLaunchKernelGGL((attn_bwd_dq_kernel<64, false, false, true>), grid_dq, block, 0, stream, p);
        } else if (head_dim == 128) {
            if (p.softclamp) hipLaunchKernelGGL((attn_bwd_dq_kernel<128, true, false, true>), grid_dq, block, 0, stream, p);
            else hipLaunchKernelGGL((attn_bwd_dq_kernel<128, false, false, true>), grid_dq, block, 0, stream, p);
        } else {
            if (p.softclamp) hipLaunchKernelGGL((attn_bwd_dq_kernel<32, true, false, true>), grid_dq, block, 0, stream, p);
            else hipLaunchKernelGGL((attn_bwd_dq_kernel<32, false, false, true>), grid_dq, block, 0, stream, p);
        }
        return;
    }
    if (head_dim == 64) {
        if (p.softclamp) if (pr) hipLaunchKernelGGL((attn_bwd_dq_kernel<64, true, true>), grid_dq, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_bwd_dq_kernel<64, true, false>), grid_dq, block, 0, stream, p);
        else if (pr) hipLaunchKernelGGL((attn_bwd_dq_kernel<64, false, true>), grid_dq, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_bwd_dq_kernel<64, false, false>), grid_dq, block, 0, stream, p);
    } else if (head_dim == 128) {
        if (p.softclamp) if (pr) hipLaunchKernelGGL((attn_bwd_dq_kernel<128, true, true>), grid_dq, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_bwd_dq_kernel<128, true, false>), grid_dq, block, 0, stream, p);
        else if (pr) hipLaunchKernelGGL((attn_bwd_dq_kernel<128, false, true>), grid_dq, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_bwd_dq_kernel<128, false, false>), grid_dq, block, 0, stream, p);
    } else if (head_dim == 32) {
        if (p.softclamp) if (pr) hipLaunchKernelGGL((attn_bwd_dq_kernel<32, true, true>), grid_dq, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_bwd_dq_kernel<32, true, false>), grid_dq, block, 0, stream, p);
        else if (pr) hipLaunchKernelGGL((attn_bwd_dq_kernel<32, false, true>), grid_dq, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_bwd_dq_kernel<32, false, false>), grid_dq, block, 0, stream, p);
    } else {
        __builtin_trap();
    }
}

void launch_attn_bwd_dkv(const BwdParams& p, int head_dim, hipStream_t stream) {
    dim3 block(512);
    int z = p.split > 1 ? p.split : 1;
    long kt_ = ceil_div(p.nk, ROWS_WG);
    if (p.desc) kt_ = p.n_units;
    else if (p.paired) kt_ = (kt_ + 1) / 2;
    dim3 grid_dkv(kt_, p.b * p.hk, z);
    const bool pr = p.paired > 0;
    if (p.bias) {   // bias runs unpaired (bindings force paired=0)
        if (head_dim == 64) {
            if (p.softclamp) hipLaunchKernelGGL((attn_bwd_dkv_kernel<64, DKV_QT, true, false, true>), grid_dkv, block, 0, stream, p);
            else hipLaunchKernelGGL((attn_bwd_dkv_kernel<64, DKV_QT, false, false, true>), grid_dkv, block, 0, stream, p);
        } else if (head_dim == 128) {
            if (p.softclamp) hipLaunchKernelGGL((attn_bwd_dkv_kernel<128, DKV_QT, true, false, true>), grid_dkv, block, 0, stream, p);
            else hipLaunchKernelGGL((attn_bwd_dkv_kernel<128, DKV_QT, false, false, true>), grid_dkv, block, 0, stream, p);
        } else {
            if (p.softclamp) hipLaunchKernelGGL((attn_bwd_dkv_kernel<32, DKV_QT, true, false, true>), grid_dkv, block, 0, stream, p);
            else hipLaunchKernelGGL((attn_bwd_dkv_kernel<32, DKV_QT, false, false, true>), grid_dkv, block, 0, stream, p);
        }
        return;
    }
    if (head_dim == 64) {
        if (p.softclamp) if (pr) hipLaunchKernelGGL((attn_bwd_dkv_kernel<64, DKV_QT, true, true>), grid_dkv, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_bwd_dkv_kernel<64, DKV_QT, true, false>), grid_dkv, block, 0, stream, p);
        else if (pr) hipLaunchKernelGGL((attn_bwd_dkv_kernel<64, DKV_QT, false, true>), grid_dkv, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_bwd_dkv_kernel<64, DKV_QT, false, false>), grid_dkv, block, 0, stream, p);
    } else if (head_dim == 128) {
        if (p.softclamp) if (pr) hipLaunchKernelGGL((attn_bwd_dkv_kernel<128, DKV_QT, true, true>), grid_dkv, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_bwd_dkv_kernel<128, DKV_QT, true, false>), grid_dkv, block, 0, stream, p);
        else if (pr) hipLaunchKernelGGL((attn_bwd_dkv_kernel<128, DKV_QT, false, true>), grid_dkv, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_bwd_dkv_kernel<128, DKV_QT, false, false>), grid_dkv, block, 0, stream, p);
    } else if (head_dim == 32) {
        if (p.softclamp) if (pr) hipLaunchKernelGGL((attn_bwd_dkv_kernel<32, DKV_QT, true, true>), grid_dkv, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_bwd_dkv_kernel<32, DKV_QT, true, false>), grid_dkv, block, 0, stream, p);
        else if (pr) hipLaunchKernelGGL((attn_bwd_dkv_kernel<32, DKV_QT, false, true>), grid_dkv, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_bwd_dkv_kernel<32, DKV_QT, false, false>), grid_dkv, block, 0, stream, p);
    } else {
        __builtin_trap();
    }
}

// ---------------------------------------------------------------------------
// delta = rowsum(dO * O) preprocess, fused over the bf16 inputs
// (replaces two f32 casts + mul + reduce torch kernels per backward)
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void attn_delta_kernel(DeltaParams p) {
    constexpr int LPR = D / 8;                 // lanes per row (16B each)
    constexpr int RPW = 64 / LPR;              // rows per wave
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * (blockDim.x >> 6)) + (threadIdx.x >> 6);
    const long row = (long)wave * RPW + lane / LPR;
    if (row >= p.rows) return;
    const int c = lane % LPR;

    const __bf16* dop = (const __bf16*)p.dout + row * D + c * 8;
    const __bf16* op = (const __bf16*)p.out + row * D + c * 8;
    bf16x8 a = *(const bf16x8*)dop;
    bf16x8 b = *(const bf16x8*)op;
    float s = 0.f;
    #pragma unroll
    for (int e = 0; e < 8; ++e) s += (float)a[e] * (float)b[e];
    #pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (c == 0) {
        // row = (bb * n + i) * h + hh  ->  delta[(bb * h + hh) * n + i]
        const long hh = row % p.h;
        const long bi = row / p.h;
        const long i = bi % p.n, bb = bi / p.n;
        p.delta[(bb * p.h + hh) * p.n + i] = s;
    }
}

void launch_attn_delta(const DeltaParams& p, int head_dim, hipStream_t stream) {
    dim3 block(256);
    if (head_dim == 64) {
        long waves = (p.rows + 7) / 8;
        hipLaunchKernelGGL(attn_delta_kernel<64>, dim3((waves + 3) / 4), block, 0, stream, p);
    } else if (head_dim == 128) {
        long waves = (p.rows + 3) / 4;
        hipLaunchKernelGGL(attn_delta_kernel<128>, dim3((waves + 3) / 4), block, 0, stream, p);
    } else if (head_dim == 32) {
        long waves = (p.rows + 15) / 16;
        hipLaunchKernelGGL(attn_delta_kernel<32>, dim3((waves + 3) / 4), block, 0, stream, p);
    } else {
        __builtin_trap();
    }
}

// ---------------------------------------------------------------------------
// finalize: ONE launch turning the fp32-accumulated scratch gradients into
// bf16 gradients in the caller's layout (replaces two permute-copies and
// three casts wherever fp32 accumulation is genuinely needed: grid.z splits,
// descriptor units, multi-hop ring, all-gather reduce-scatter).
//   grid = (ceil(Nk/64), B*HK, 3): z=0 dk, z=1 dv, z=2 dq (grid-stride cast)
//   dk fp32 (B,HK,Nk,D) -> bf16 (B,Nk,HK,D): rows are contiguous both sides
//   dv fp32 (B,HK,D,Nk) -> bf16 (B,Nk,HK,D): 64-kv tile transposed in LDS
//     (reads coalesced along kv, writes 16 B along d); any Nk
// Memory-bound: 6 B moved per gradient element.
// ---------------------------------------------------------------------------
static constexpr int FIN_ROWS = 64;

__device__ __forceinline__ uint4 fin_pack8(const float* s) {
    f32x4 a = {s[0], s[1], s[2], s[3]}, c = {s[4], s[5], s[6], s[7]};
    union { bf16x4 h[2]; uint4 u; } o;
    o.h[0] = __builtin_convertvector(a, bf16x4);
    o.h[1] = __builtin_convertvector(c, bf16x4);
    return o.u;
}

template <int D>
__global__ __launch_bounds__(256) void attn_bwd_finalize_kernel(BwdFinalizeParams p) {
    constexpr int CH = D / 8;
    constexpr int LDW = FIN_ROWS + 1;          // padded kv pitch (floats)
    __shared__ float tile[D * LDW];
    const int tid = threadIdx.x;
    const int which = blockIdx.z;

    if (which == 2) {
        if (!p.dq) return;
        const long nblk = (long)gridDim.x * gridDim.y;
        const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
        const long chunks = p.dq_elems / 8;
        for (long c = blk * 256 + tid; c < chunks; c += nblk * 256) {
            float s[8];
            *(f32x4*)s = *(const f32x4*)(p.dq + c * 8);
            *(f32x4*)(s + 4) = *(const f32x4*)(p.dq + c * 8 + 4);
            *(uint4*)((__bf16*)p.dq_bf + c * 8) = fin_pack8(s);
        }
        return;
    }
    if (!p.dk) return;

    const int bb = blockIdx.y / p.hk;
    const int hh = blockIdx.y % p.hk;
    const long n0 = (long)blockIdx.x * FIN_ROWS;
    const int rows = (int)min((long)FIN_ROWS, p.nk - n0);
    const long orow_stride = (long)p.hk * D;

    if (which == 0) {
        const float* src = p.dk + (((long)bb * p.hk + hh) * p.nk + n0) * D;
        __bf16* dst = (__bf16*)p.dk_bf + ((long)bb * p.nk + n0) * orow_stride + (long)hh * D;
        for (int c = tid; c < rows * CH; c += 256) {
            int row = c / CH, ch = c % CH;
            float s[8];
            *(f32x4*)s = *(const f32x4*)(src + (long)row * D + ch * 8);
            *(f32x4*)(s + 4) = *(const f32x4*)(src + (long)row * D + ch * 8 + 4);
            *(uint4*)(dst + row * orow_stride + ch * 8) = fin_pack8(s);
        }
        return;
    }

    // dv: source rows are d, kv contiguous — scalar loads (any Nk alignment)
    const float* src = p.dv + (((long)bb * p.hk + hh) * D) * p.nk + n0;
    for (int c = tid; c < D * FIN_ROWS; c += 256) {
        int d = c / FIN_ROWS, nn = c % FIN_ROWS;
        if (nn < rows) tile[d * LDW + nn] = src[(long)d * p.nk + nn];
    }
    __syncthreads();
    __bf16* dst = (__bf16*)p.dv_bf + ((long)bb * p.nk + n0) * orow_stride + (long)hh * D;
    for (int c = tid; c < rows * CH; c += 256) {
        int row = c / CH, ch = c % CH;
        float s[8];
        #pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = tile[(ch * 8 + e) * LDW + row];
        *(uint4*)(dst + row * orow_stride + ch * 8) = fin_pack8(s);
    }
}

void launch_attn_bwd_finalize(const BwdFinalizeParams& p, int head_dim, hipStream_t stream) {
    dim3 block(256);
    long nx = p.dk ? (p.nk + FIN_ROWS - 1) / FIN_ROWS : 256;
    int ny = p.dk ? p.b * p.hk : 1;
    dim3 grid(nx, ny, p.dq ? 3 : 2);
    if (head_dim == 64) hipLaunchKernelGGL(attn_bwd_finalize_kernel<64>, grid, block, 0, stream, p);
    else if (head_dim == 128) hipLaunchKernelGGL(attn_bwd_finalize_kernel<128>, grid, block, 0, stream, p);
    else if (head_dim == 32) hipLaunchKernelGGL(attn_bwd_finalize_kernel<32>, grid, block, 0, stream, p);
    else __builtin_trap();
}

}  // namespace ring_attn
