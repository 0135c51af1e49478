// CDNA4 (gfx950) flash-attention FORWARD kernel with online-softmax
// resume across ring passes.
//
// Brand-new MI355X design (capability counterpart of the reference's Triton
// _fwd_kernel, /root/reference/ring_attention_pytorch/triton_flash_attn.py:52-430,
// re-thought for wave64 + MFMA; no code ported):
//
//   * 8 waves / 512 threads per workgroup; each wave owns 32 Q rows
//     (256-row Q tile per workgroup), KV tile = KVBLK (128 at d64).
//   * swapped QK^T: S^T[kv][q] = mfma(A=K, B=Q^T) so each lane holds a full
//     slice of ONE q row's scores -> softmax is almost entirely in-register
//     (31 VALU max/sum + one cross-half __shfl_xor), no LDS round trip.
//   * P -> bf16 via one v_cvt_pk_bf16_f32 per pair; the packed pairs ARE the
//     PV B-operand fragments: the V^T image is staged in the k order the
//     score tile's C layout produces (kperm_pair in attn_common.h), so no
//     lane exchange is needed.
//   * K and V^T staged in LDS with an XOR-16B swizzle (conflict-free
//     ds_read_b128 column slices); 3-deep pipeline over DOUBLE-buffered LDS
//     (one barrier per tile; staging overlaps the MFMAs).
//   * causality, striping and lookback reduce to integers (attn_mask.h holds
//     the algebra): attend(i,j) <=> j <= qpos(i) AND qpos(i) - j <= win, with
//     qpos affine in i (host folds ring-rank offsets / layout strides; a
//     stride > 1 expresses a striped q shard against gathered global KV).
//   * resume contract: fp32 o_acc (B,H,D,Nq transposed scratch), m, l
//     (B,H,Nq) persist between ring hops; IS_FIRST initializes instead of
//     loading, IS_LAST normalizes and emits bf16 out (B,Nq,H,D) + lse.
//     Single-hop launches (IS_FIRST && IS_LAST) never touch o_acc at all.
//
// Verified fragment maps (csrc/tools/mfma_probe.hip, run on MI355X):
//   mfma_f32_32x32x16_bf16: A(i=l&31, k=8*(l>>5)+r)  B(k=8*(l>>5)+r, j=l&31)
//                           C(i=(r&3)+8*(r>>2)+4*(l>>5), j=l&31)
//   permlane32_swap: r0 = {lo: vdst.lo, hi: src.lo}, r1 = {lo: vdst.hi, hi: src.hi}

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>
#include <cstdlib>

#include "attn_common.h"

namespace ring_attn {

// ---------------------------------------------------------------------------
// geometry
// ---------------------------------------------------------------------------
// tile shapes come from attn_mask.h: 256 q rows per workgroup (8 waves x 32
// rows), kv tile kvblk(D)
static constexpr int WAVES = 8;          // 8-wave WGs: the 2-waves/SIMD paired
static constexpr int QROWS_WAVE = 32;    // regime (4-wave variant measured slower)
static constexpr int QROWS_WG = ROWS_WG;
static_assert(QROWS_WG == WAVES * QROWS_WAVE);
static constexpr int NTHREADS = WAVES * 64;

template <int D>
struct FwdLds {
    static constexpr int KVB = kvblk(D);
    // double-buffered: K tile [kv][D] + V^T tile [d][kv], 16B-chunk swizzled
    __align__(16) __bf16 k[2][KVB * D];
    __align__(16) __bf16 vt[2][D * KVB];
    unsigned char kmask[2][KVB];
};

// ---------------------------------------------------------------------------
// forward kernel
// ---------------------------------------------------------------------------
// How the per-q-tile body (attn_fwd_body.inc) is placed in the kernel.
enum BodyForm {
    BODY_DIRECT,   // at pit-loop scope, P aliases the kernel parameter
    BODY_LAMBDA,   // directly-called lambda with a VALUE copy of the params
    BODY_FRAME,    // the same lambda behind a noinline frame
};

// The form each instantiation keeps, chosen by measurement (fwd-only, same
// box, TF; profiles/README.md "Lean forward instantiations").
// Full-featured bodies keep what they had: PAIRED the frame (it confines
// register allocation to the body, the pair loop's liveness otherwise spills
// 532 B/lane); d128 plain the value copy (it frees the allocator from
// aliasing p through the kernarg segment, 498 vs 424); d64 / d32 plain direct
// (the lambda cost 264 B/lane of scratch and -3.5%, the frame -12%).
// Lean bodies are direct everywhere.  The frame and the value copy were
// remedies for register pressure the lean body does not have, and the frame
// now only costs (direct / lambda / frame): d64 plain 554 / 536 / 473, d128
// plain 699 / 683 / 570, d64 PAIRED 476 / 468 / 410, d128 PAIRED 607 / 611 /
// 505, d32 PAIRED 281 / 283 / 205, d32 plain 326 / 329 / 227.  Direct and
// lambda are within a run's spread at d128 PAIRED and d32; direct is the
// simpler form and the only one with no scratch in the plain kernels.
// To measure the forms again, build with -DFWD_LEAN_FORM=0|1|2 (BodyForm
// value): every lean instantiation then takes that form.  The figures above
// came from a build that chose the form per launch instead; the kernels are
// the same.
#ifndef FWD_LEAN_FORM
#define FWD_LEAN_FORM BODY_DIRECT
#endif
constexpr BodyForm fwd_body_form(int d, bool paired, bool lean) {
    if (lean) return (BodyForm)FWD_LEAN_FORM;
    return paired ? BODY_FRAME : d == 128 ? BODY_LAMBDA : BODY_DIRECT;
}

// LEAN: the body without ticks, ablate, key-pad mask and bias (see the
// header of attn_fwd_body.inc); launch_attn_fwd picks it when none is set.
template <int D, bool SOFTCLAMP, bool PAIRED, bool LEAN>
__global__ __launch_bounds__(NTHREADS, 1) void attn_fwd_kernel(FwdParams p) {
    static_assert(D % 32 == 0);
    constexpr int DBLK = D / 32;     // 32-d output blocks
    constexpr int KSTEPS = D / 16;   // QK^T k-steps
    constexpr int KVBLK = kvblk(D);
    constexpr int NBLK = KVBLK / 32;

    constexpr BodyForm FORM = fwd_body_form(D, PAIRED, LEAN);

    __shared__ FwdLds<D> lds;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int l31 = lane & 31;
    const int lhi = lane >> 5;        // 0 or 1

    const int bh = blockIdx.y;
    const int b = bh / p.h;
    const int h = bh % p.h;
    const int hk = h % p.hk;          // kv head (reference tile GQA: qh pairs qh % hk)

    // causal pairing: WG x runs q-tiles (x, T-1-x) — per-WG work is the
    // uniform T+1 tiles instead of the 2:1 triangle imbalance
    const int n_pit = PAIRED
        ? (p.paired - 1 - (int)blockIdx.x == (int)blockIdx.x ? 1 : 2) : 1;
    for (int pit = 0; pit < n_pit; ++pit) {
    const int qtile = PAIRED
        ? (pit == 0 ? (int)blockIdx.x : p.paired - 1 - (int)blockIdx.x)
        : (int)blockIdx.x;
    if (PAIRED && pit == 1) {
        __syncthreads();                       // LDS handoff between tiles
    }

    if constexpr (FORM == BODY_FRAME) {
        auto fwd_body = [&]() {
            const FwdParams P = p;   // register-local copy: the noinline
                                     // frame would otherwise re-read
                                     // fields through scratch
            #define FWD_EXIT return
            #include "attn_fwd_body.inc"
            #undef FWD_EXIT
        };
        noinline_call(fwd_body);
    } else if constexpr (FORM == BODY_LAMBDA) {
        auto fwd_body = [&]() {
            const FwdParams P = p;
            #define FWD_EXIT return
            #include "attn_fwd_body.inc"
            #undef FWD_EXIT
        };
        fwd_body();
    } else {
        const FwdParams& P = p;      // transparent alias: keeps the
                                     // original (spill-free) codegen
        #define FWD_EXIT continue
        #include "attn_fwd_body.inc"
        #undef FWD_EXIT
    }
    }  // pair loop
}

// ---------------------------------------------------------------------------
// split-merge: combine kv_split partials (and optionally the running ring
// accumulator) with the standard online-softmax merge; memory-bound.
// One thread per q row; d-loop vectorized along n across the wave.
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void attn_fwd_merge_kernel(FwdMergeParams p) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;   // global (b*h*n) row
    const long total = (long)p.b * p.h * p.nq;
    if (row >= total) return;
    const long bh = row / p.nq;
    const long n = row % p.nq;
    const long b = bh / p.h, h = bh % p.h;

    const long bhn = bh * p.nq + n;
    const long stride_bh = (long)p.b * p.h;

    float m_tot = MASK_VALUE_F;
    if (!p.is_first) m_tot = p.m[bhn];
    for (int s = 0; s < p.splits; ++s)
        m_tot = fmaxf(m_tot, p.m_part[s * stride_bh * p.nq + bhn]);

    float l_tot = 0.f;
    float alpha_prev = 0.f;
    if (!p.is_first) {
        alpha_prev = __expf(p.m[bhn] - m_tot);
        l_tot = p.l[bhn] * alpha_prev;
    }
    float alpha_s[16];                      // splits <= 16
    for (int s = 0; s < p.splits; ++s) {
        alpha_s[s] = __expf(p.m_part[s * stride_bh * p.nq + bhn] - m_tot);
        l_tot += p.l_part[s * stride_bh * p.nq + bhn] * alpha_s[s];
    }

    const long od_base = (bh * D) * p.nq + n;     // (b,h,d,n) index at d=0
    if (p.is_last) {
        float l_safe = fmaxf(l_tot, 1e-38f);
        float inv = 1.f / l_safe;
        __bf16* ob = (__bf16*)p.out + ((long)b * p.nq + n) * p.h * D + h * D;
        for (int d = 0; d < D; d += 4) {
            float acc[4];
            #pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = p.is_first ? 0.f : p.o_acc[od_base + (long)(d + e) * p.nq] * alpha_prev;
                for (int s = 0; s < p.splits; ++s)
                    v += p.o_part[s * stride_bh * D * p.nq + od_base + (long)(d + e) * p.nq]
                         * alpha_s[s];
                acc[e] = v * inv;
            }
            __bf16 four[4] = {(__bf16)acc[0], (__bf16)acc[1], (__bf16)acc[2], (__bf16)acc[3]};
            *(uint2*)(ob + d) = *(uint2*)four;
        }
        p.lse[bhn] = __logf(l_safe) + m_tot;
    } else {
        for (int d = 0; d < D; ++d) {
            float v = p.is_first ? 0.f : p.o_acc[od_base + (long)d * p.nq] * alpha_prev;
            for (int s = 0; s < p.splits; ++s)
                v += p.o_part[s * stride_bh * D * p.nq + od_base + (long)d * p.nq] * alpha_s[s];
            p.o_acc[od_base + (long)d * p.nq] = v;
        }
        p.m[bhn] = m_tot;
        p.l[bhn] = l_tot;
    }
}

void launch_attn_fwd_merge(const FwdMergeParams& p, int head_dim, hipStream_t stream) {
    long total = (long)p.b * p.h * p.nq;
    dim3 grid((total + 255) / 256);
    dim3 block(256);
    if (head_dim == 64) {
        hipLaunchKernelGGL(attn_fwd_merge_kernel<64>, grid, block, 0, stream, p);
    } else if (head_dim == 32) {
        hipLaunchKernelGGL(attn_fwd_merge_kernel<32>, grid, block, 0, stream, p);
    } else {
        hipLaunchKernelGGL(attn_fwd_merge_kernel<128>, grid, block, 0, stream, p);
    }
}

template <int D, bool LEAN>
static void launch_fwd_d(const FwdParams& p, dim3 grid, dim3 block, hipStream_t stream) {
    if (p.softclamp) {
        if (p.paired > 0) hipLaunchKernelGGL((attn_fwd_kernel<D, true, true, LEAN>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_fwd_kernel<D, true, false, LEAN>), grid, block, 0, stream, p);
    } else {
        if (p.paired > 0) hipLaunchKernelGGL((attn_fwd_kernel<D, false, true, LEAN>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_fwd_kernel<D, false, false, LEAN>), grid, block, 0, stream, p);
    }
}

void launch_attn_fwd(const FwdParams& p, int head_dim, hipStream_t stream) {
    // v2 (one-wave-per-SIMD pipeline) opt-in via RING_ATTN_FWD_V2=1;
    // RING_ATTN_FWD_V2=0 forces v1.  Default currently v1 (flip after the
    // promotion criterion: v2 beats v1 with full-flag oracle parity).
    static const char* v2env = std::getenv("RING_ATTN_FWD_V2");
    if (v2env && v2env[0] == '1') {
        if (launch_attn_fwd_v2(p, head_dim, stream)) return;
    }
    long qtiles = ceil_div(p.nq, QROWS_WG);
    dim3 grid(p.paired ? (qtiles + 1) / 2 : qtiles, p.b * p.h,
              p.kv_split > 1 ? p.kv_split : 1);
    dim3 block(NTHREADS);
    // lean exactly when none of the four cold features is asked for
    const bool lean = !p.kmask && !p.bias && !p.ticks && p.ablate == 0;
    if (head_dim == 64) {
        if (lean) launch_fwd_d<64, true>(p, grid, block, stream);
        else launch_fwd_d<64, false>(p, grid, block, stream);
    } else if (head_dim == 128) {
        if (lean) launch_fwd_d<128, true>(p, grid, block, stream);
        else launch_fwd_d<128, false>(p, grid, block, stream);
    } else if (head_dim == 32) {
        if (lean) launch_fwd_d<32, true>(p, grid, block, stream);
        else launch_fwd_d<32, false>(p, grid, block, stream);
    } else {
        // unsupported head dim is a host-side error (checked in bindings)
        __builtin_trap();
    }
}

}  // namespace ring_attn
