// Shared types for the ring_attention_amd CDNA4 kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_bf16.h>
#endif

#include "attn_mask.h"

namespace ring_attn {

#ifdef __HIPCC__
typedef __bf16 bf16_t;
typedef bf16_t bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef bf16_t bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef bf16_t bf16x2 __attribute__((ext_vector_type(2)));

// two fp32 -> one packed bf16 pair (lo = a, hi = b), round-to-nearest-even.
// The vector convert lowers to ONE v_cvt_pk_bf16_f32; the
// __float22bfloat162_rn route costs two converts plus a shift and an or.
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
    union { bf16x2 h; uint32_t u; } c;
    c.h = __builtin_convertvector(f32x2{a, b}, bf16x2);
    return c.u;
}

// Second-GEMM k order.  An MFMA sums over k, so any permutation of the k
// slots shared by A and B leaves the product unchanged.  The score tile's C
// layout gives lane half lhi rows (r&3) + 8*(r>>2) + 4*lhi, so the packed
// pairs x2 = 4*half .. 4*half+3 of a 32-row block are rows
// 16*half + 4*lhi + {0,1,2,3,8,9,10,11}.  Taking that as the k order of
// k-step `half` makes the packed pairs the P/dS fragment as they stand; the
// OTHER operand is staged to match: a transposed LDS image stores row pair
// (b2 b1 b0) of each 16-row group at pair slot (b1 b2 b0), so the 16-byte
// chunk lhi of the group holds exactly those rows.
__device__ __forceinline__ int kperm_pair(int jp) {
    return (jp & ~6) | ((jp & 4) >> 1) | ((jp & 2) << 1);
}

// XOR swizzle of a 16-byte chunk index within a row of CH chunks:
// chunk' = chunk ^ (row & 7).  Applied identically on the staging write and
// the fragment read, so the LDS image is consistent (both-sides rule).
template <int CH>
__device__ __forceinline__ int swz(int row, int chunk) {
    // swizzle mask must stay inside the row: CH chunks per row (CH-1 when
    // CH <= 8; wider rows keep the measured 8-slot spread)
    return chunk ^ (row & (CH < 8 ? CH - 1 : 7));
}

// Single-issue f32 subtract / multiply for the softmax and ds blocks of the
// backward tile loops.  Written in C++, neighbouring register pairs of these
// ops are SLP-packed into v_pk_add_f32 / v_pk_mul_f32 under plain -O3, and a
// packed f32 op issued beside MFMAs costs more than the two scalar ops it
// replaces.  The helpers are the same IEEE operation per element (bitwise
// equal results): the op itself stays C++ and its RESULT passes through an
// empty asm, which the vectorizer cannot look through, so no pair of them
// is ever joined.  Not volatile and no clobbers: the scheduler places them
// like any other VALU op.
// The op must NOT be written as asm ("v_sub_f32 %0, %1, %2"): these operands
// are MFMA results, the wait states between an MFMA and a VALU read of its
// result are inserted by the compiler, and it inserts none in front of
// inline asm.  That form read accumulators ahead of the MFMA's write (dq
// wrong by orders of magnitude on the GPU).
// (-fno-slp-vectorize for the translation unit was the alternative: it also
// changes staging and epilogue code, moves scratch up in four
// instantiations, and leaves the vector-typed epilogue scaling packed.)
__device__ __forceinline__ float sub_f32(float a, float b) {
    float r = a - b;
    asm("" : "+v"(r));
    return r;
}
__device__ __forceinline__ float mul_f32(float a, float b) {
    float r = a * b;
    asm("" : "+v"(r));
    return r;
}

// fast tanh from builtins: tanh(x) = 1 - 2/(exp2(2x*log2e) + 1); avoids the
// libm tanhf whose inlined body injects v_div_* sequences into the hot loop
__device__ __forceinline__ float fast_tanhf(float x) {
    float e = __builtin_amdgcn_exp2f(x * 2.885390081777927f);   // 2*log2(e)
    return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}

// cross-half (lane <-> lane^32) exchange via v_permlane32_swap — pure VALU,
// no LDS round trip (a __shfl_xor(x, 32) lowers to ds_bpermute + addressing)
__device__ __forceinline__ float cross_half(float x) {
    union { float f; unsigned u; } c; c.f = x;
    u32x2 r = __builtin_amdgcn_permlane32_swap(c.u, c.u, false, false);
    // r0 = {lo: own lo, hi: own lo}; r1 = {lo: own hi, hi: own hi}
    union { unsigned u; float f; } lo, hi; lo.u = r[0]; hi.u = r[1];
    // lanes < 32 want the partner's value = own hi-half's value = r1.lo;
    // lanes >= 32 want r0.hi = own lo-half's value — both are "the other
    // half's x" exactly when we select r1 on lo lanes and r0 on hi lanes
    return (threadIdx.x & 32) ? lo.f : hi.f;
}

// a noinline frame confines register allocation to the body it wraps
template <class F>
__device__ __attribute__((noinline)) void noinline_call(F&& f) { f(); }

// The same frame for a body that captures nothing.  A lambda called through a
// noinline frame reads everything it captures by reference back from memory
// into VGPRs, and the compiler then treats values that are the same in every
// lane as per-lane: loop bounds, pointers and mask integers become 64-bit
// VALU compares and exec-masked branches.  Such a body instead takes its one
// varying scalar and the address of the kernel's parameters as arguments,
// re-derives the rest from blockIdx / threadIdx and reads the parameters with
// kernarg_params().
// not_tail_called: a call that passes no pointer into the caller's frame gets
// the IR `tail` marker, and a function with such a call site loses the
// local-function exemption from saving callee-saved registers — the frame
// would open and close with ~110 scratch stores and loads.
template <class F>
__device__ __attribute__((noinline, not_tail_called))
void noinline_call(F&& f, int x, unsigned long long kernarg) { f(x, kernarg); }

// wave-uniform value -> SGPR (the caller vouches that every lane holds x)
template <bool ON>
__device__ __forceinline__ int uniform(int x) {
    if constexpr (ON) return __builtin_amdgcn_readfirstlane(x);
    else return x;
}

// Address of the kernarg segment.  KERNELS ONLY: in a called function the
// builtin is lowered to a null pointer, so the kernel takes the address and
// hands it to the frame.
__device__ __forceinline__ unsigned long long kernarg_address() {
    return (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
}

// The kernel's parameter struct, read from the kernarg segment at `kernarg`
// (kernarg_address() of a kernel whose ONLY parameter is a T by value).  The
// address goes through readfirstlane and the loads through the constant
// address space, so they are scalar loads and every field arrives
// wave-uniform in SGPRs.
template <class T>
__device__ __forceinline__ T kernarg_params(unsigned long long kernarg) {
    static_assert(sizeof(T) % 4 == 0);
    typedef const __attribute__((address_space(4))) unsigned int* const_words;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)kernarg);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(kernarg >> 32));
    const_words src = (const_words)(((unsigned long long)hi << 32) | lo);
    union { T t; unsigned w[sizeof(T) / 4]; } u;
    #pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; ++i) u.w[i] = src[i];
    return u.t;
}

// A pointer rebuilt from kernarg words has no address space the compiler can
// see, and is accessed with flat instructions; those also count on lgkmcnt,
// the counter the LDS operand waits are counted on.  Kernel parameters point
// to global memory (or are null): rebuilding p as a global-address-space
// pointer says so, and the compiler carries it to every access derived from
// p.  (Through the integer: a direct generic -> global -> generic pointer
// cast pair is folded away.)
template <class T>
__device__ __forceinline__ T* as_global(T* p) {
    return (T*)(__attribute__((address_space(1))) T*)(unsigned long long)p;
}

static constexpr float LOG2E = 1.4426950408889634f;
static constexpr float LN2 = 0.6931471805599453f;
#endif

// Must match ring_attention_amd.ops.reference.MASK_VALUE (torch.finfo(f32).min)
static constexpr float MASK_VALUE_F = -3.4028234663852886e38f;

struct FwdParams {
    const void* q;          // bf16 (B, Nq, H, D)
    const void* k;          // bf16 (B, Nk, HK, D)
    const void* v;          // bf16 (B, Nk, HK, D)
    const void* kmask;      // uint8 (B, Nk) or nullptr; 1 = attend
    float* o_acc;           // fp32 (B, H, D, Nq) scratch (nullptr for single-pass)
    float* m;               // fp32 (B, H, Nq)
    float* l;               // fp32 (B, H, Nq)
    void* out;              // bf16 (B, Nq, H, D) (written when is_last)
    float* lse;             // fp32 (B, H, Nq)    (written when is_last)
    int b, h, hk, group;    // group = H / HK
    long nq, nk;
    float scale;
    float softclamp_value;
    int softclamp;          // bool
    int causal;             // bool
    long diag;              // q position base: qpos(i) = i*q_stride + diag
    long q_stride;          // attend iff j <= qpos(i) (causal)
    long win;               // attend iff qpos(i) - j <= win (when has_win)
    int has_win;            // lookback window enabled
    int is_first;           // initialize m/l/o instead of loading
    int is_last;            // normalize + write out/lse instead of o_acc/m/l
    int kv_split;           // >1: grid.z splits the kv range; o_acc/m/l hold
                            // kv_split partials (merged by attn_fwd_merge)
    int ablate;             // diagnostics: 1 = stage first tile only
    int paired;             // causal load balance: >0 = total q-tiles T;
                            // grid.x = ceil(T/2), each WG runs tiles
                            // (x, T-1-x) so per-WG causal work is uniform
    unsigned long long* ticks;  // diagnostics: per-tile segment s_memtime
                                // stamps from block(0,0,0) wave 0 (or null)
    const float* bias;      // additive attention bias (natural-log domain)
                            // or null; (B,H,Nk) vector / (B,H,Nq,Nk) matrix
                            // (reference triton_flash_attn.py:1047-1063)
    int bias_mat;           // 1 = matrix (per-row) bias
};

struct FwdMergeParams {
    const float* o_part;    // fp32 (S, B, H, D, Nq) unnormalized partials
    const float* m_part;    // fp32 (S, B, H, Nq)
    const float* l_part;    // fp32 (S, B, H, Nq)
    float* o_acc;           // fp32 (B, H, D, Nq) running accumulator (ring)
    float* m;               // fp32 (B, H, Nq)
    float* l;               // fp32 (B, H, Nq)
    void* out;              // bf16 (B, Nq, H, D) written when is_last
    float* lse;             // fp32 (B, H, Nq)
    int splits;
    int b, h;
    long nq;
    int is_first;           // no running state to fold in
    int is_last;            // normalize + emit out/lse
};

void launch_attn_fwd_merge(const FwdMergeParams& p, int head_dim, hipStream_t stream);

void launch_attn_fwd(const FwdParams& p, int head_dim, hipStream_t stream);

// v2: one-wave-per-SIMD pipelined forward (attn_fwd_v2.hip); returns false
// when the config is not covered (caller falls back to v1)
bool launch_attn_fwd_v2(const FwdParams& p, int head_dim, hipStream_t stream);

struct BwdParams {
    const void* q;          // bf16 (B, Nq, H, D)
    const void* k;          // bf16 (B, Nk, HK, D)
    const void* v;          // bf16 (B, Nk, HK, D)
    const void* dout;       // bf16 (B, Nq, H, D)
    const void* kmask;      // uint8 (B, Nk) or nullptr
    const float* lse;       // fp32 (B, H, Nq)
    const float* delta;     // fp32 (B, H, Nq)  rowsum(do*o)
    float* dq;              // fp32 (B, Nq, H, D)  plain write / += / atomics
    float* dk;              // fp32 (B, HK, Nk, D) kernel scratch layout
    float* dv;              // fp32 (B, HK, D, Nk) transposed scratch layout
    // fused epilogue (single-pass launches only: split <= 1, no desc, no
    // accumulate — the kernel is then the unique writer of every element).
    // When set, the epilogue rounds its fp32 accumulator to bf16 (RNE) and
    // stores it HERE in the caller's final layout; the matching fp32 buffer
    // above is not touched and may be null.
    void* dq_bf;            // bf16 (B, Nq, H, D) or null
    void* dk_bf;            // bf16 (B, Nk, HK, D) or null
    void* dv_bf;            // bf16 (B, Nk, HK, D) or null
    int b, h, hk, group;
    long nq, nk;
    float scale;
    float softclamp_value;
    int softclamp;
    int causal;
    long diag;
    long q_stride;
    long win;
    int has_win;
    int accumulate;         // dk/dv + dq: 0 = overwrite, 1 = add to existing
    int split;              // >1: grid.z splits the contraction range; dq/dk/dv
                            // accumulated with fp32 atomics instead of plain ops
    int paired;             // causal balance: >0 = total walk-parallel tiles T;
                            // grid.x = ceil(T/2), WG x runs tiles (x, T-1-x)
    const float* bias;      // additive bias (see FwdParams) or null
    int bias_mat;
    const int* desc;        // descriptor scheduling (or null): grid.x units,
                            // desc[3u] = tile, desc[3u+1] = t_lo,
                            // desc[3u+2] = t_hi — constant work per unit;
                            // outputs accumulate with fp32 atomics
    long n_units;           // rows in desc (grid.x when desc mode)
};

void launch_attn_bwd_dq(const BwdParams& p, int head_dim, hipStream_t stream);
void launch_attn_bwd_dkv(const BwdParams& p, int head_dim, hipStream_t stream);

// One-launch finish for the fp32-accumulating backward paths (grid.z splits,
// descriptor units, multi-hop ring, all-gather reduce-scatter): fp32 scratch
// layouts -> bf16 gradients in the caller's (B, N, HK, D) layout.
struct BwdFinalizeParams {
    const float* dk;        // fp32 (B, HK, Nk, D) or null
    const float* dv;        // fp32 (B, HK, D, Nk) or null (with dk)
    const float* dq;        // fp32, dq_elems values (flat cast) or null
    void* dk_bf;            // bf16 (B, Nk, HK, D)
    void* dv_bf;            // bf16 (B, Nk, HK, D)
    void* dq_bf;            // bf16, dq_elems values
    int b, hk;
    long nk;
    long dq_elems;          // multiple of 8
};

void launch_attn_bwd_finalize(const BwdFinalizeParams& p, int head_dim, hipStream_t stream);

struct DeltaParams {
    const void* dout;       // bf16 (B, N, H, D)
    const void* out;        // bf16 (B, N, H, D)
    float* delta;           // fp32 (B, H, N)
    long rows;              // B*N*H
    long n;
    int h;
};

void launch_attn_delta(const DeltaParams& p, int head_dim, hipStream_t stream);

struct DecodeParams {
    const void* q;          // bf16 (B, HQ, NQ, D): NQ query tokens per head
                            // (speculative / tree-decode heads)
    const void* k;          // bf16 (B, HK, N, D)
    const void* v;          // bf16 (B, HK, N, D)
    float* out;             // fp32 (S, B, HQ, NQ, D) per-chunk partials
    float* lse;             // fp32 (S, B, HQ, NQ, 1)
    int b, h;               // h = HQ (query heads)
    int hk;                 // kv heads; q head qh reads kv head qh % hk
    int nq;                 // query tokens per head (>= 1)
    long n;
    float scale;
    long chunks;            // kv-split S (0 = auto)
    const void* kscale;     // fp8 mode: e8m0 per kv row (B, HK, N)
    const void* vscale;     // fp8 mode: e8m0 per kv row (B, HK, N)
};

// Default kv-split S of every decode partial: ~512 keys per wave over the
// longest key span a row covers, total waves capped near 8192, S capped at 256
// (the chunk merge grows with S).  GPU-swept; the figures are at bindings.cpp's
// decode_partials.
inline long decode_default_chunks(long span, long waves) {
    return std::max(1L, std::min(std::min(span / 512 + 1, 256L),
                                 8192L / std::max(waves, 1L)));
}

void launch_decode_partial(const DecodeParams& p, int head_dim, hipStream_t stream);
void launch_decode_partial_fp8(const DecodeParams& p, int head_dim, hipStream_t stream);

struct DecodeMergeParams {
    const float* outs;   // (S, rows, D)
    const float* lses;   // (S, rows)
    float* out;          // (rows, D)
    float* lse;          // (rows)
    long rows;           // B * H * NQ
    int s;               // chunk count S
};

void launch_decode_merge(const DecodeMergeParams& p, int head_dim, hipStream_t stream);

// Paged KV cache (decode_paged.hip).  Pool pages are (P, HK, PS, D) with
// PS = 1 << page_shift; key j of sequence b lives at page
// block_table[b][j >> page_shift], row j & (PS - 1).
struct PagedDecodeParams {
    const void* q;          // bf16 (B, HQ, NQ, D)
    const void* k_pages;    // bf16 or e4m3 bytes (P, HK, PS, D)
    const void* v_pages;    // bf16 or e4m3 bytes (P, HK, PS, D)
    const void* kscale;     // fp8 mode: e8m0 per row (P, HK, PS)
    const void* vscale;     // fp8 mode: e8m0 per row (P, HK, PS)
    const int* block_table; // int32 (B, max_pages); entries at or beyond
                            // ceil(seq_len / PS) are never read
    const int* seq_lens;    // int32 (B): tokens held per sequence (0 legal)
    float* out;             // fp32 (S, B, HQ, NQ, D) per-chunk partials
    float* lse;             // fp32 (S, B, HQ, NQ, 1)
    int b, h;               // h = HQ (query heads)
    int hk;                 // kv heads; q head qh reads kv head qh % hk
    int nq;                 // query tokens per head (>= 1)
    int page_shift;         // log2(page size)
    int max_pages;          // block_table row stride
    int num_pages;          // P: ids outside [0, P) are never dereferenced
    int causal;             // query iq sees keys [0, seq_len - (nq-1-iq))
    int chunk_major;        // 1 = kv chunk is the fast workgroup index
    float scale;
    long chunks;            // kv-split S (0 = auto from max_seq_len)
    long max_seq_len;       // host-known upper bound of seq_lens
    // lookback window: the query of row (b, iq) sits at position
    // seq_len + kv_after[b] - nq + iq (local key coordinates) and attends
    // keys [clamp(position - win, 0, limit), limit)
    int has_win;            // 0 = no window (win and kv_after unused)
    long win;               // >= 0
    const int* kv_after;    // int32 (B): tokens held by LATER ranks, or null (0)
};

void launch_decode_partial_paged(const PagedDecodeParams& p, int head_dim, bool fp8,
                                 hipStream_t stream);

struct PagedAppendParams {
    const void* k_new;      // bf16 (B, HK, T, D)
    const void* v_new;      // bf16 (B, HK, T, D)
    void* k_pages;          // bf16 or e4m3 bytes (P, HK, PS, D)
    void* v_pages;
    void* kscale;           // fp8 mode: e8m0 per row (P, HK, PS)
    void* vscale;
    const int* block_table; // int32 (B, max_pages)
    const int* seq_lens;    // int32 (B): lengths BEFORE the append
    const int* append_lens; // int32 (B): 0 <= append_lens[b] <= T
    int b, hk, t;
    int page_shift, max_pages, num_pages;
};

void launch_paged_kv_append(const PagedAppendParams& p, int head_dim, bool fp8,
                            hipStream_t stream);

// Paged prefill (attn_fwd_paged.hip): the dense forward over pool pages with
// per-sequence geometry.  Query t < q_lens[b] sits at position
// seq_lens[b] - q_lens[b] + t (its tokens are already cached) and attends
// keys [0, seq_lens[b]) under Mask{causal, has_win, diag = seq_len - q_len,
// q_stride = 1, win}.
struct PagedPrefillParams {
    const void* q;          // bf16 (B, T, H, D)
    const void* k_pages;    // bf16 or e4m3 bytes (P, HK, PS, D)
    const void* v_pages;
    const void* kscale;     // fp8 mode: e8m0 per row (P, HK, PS)
    const void* vscale;
    const int* block_table; // int32 (B, max_pages); entries at or beyond
                            // ceil(seq_len / PS) are never read
    const int* seq_lens;    // int32 (B)
    const int* q_lens;      // int32 (B): 0 <= q_lens[b] <= min(T, seq_lens[b])
    float* o_part;          // kv_split > 1: fp32 (S, B, H, D, T) partials
    float* m_part;          // fp32 (S, B, H, T)
    float* l_part;          // fp32 (S, B, H, T)
    void* out;              // kv_split <= 1: bf16 (B, T, H, D)
    float* lse;             // fp32 (B, H, T)
    int b, h, hk;
    int t;                  // T: q rows per sequence in the buffers
    int page_shift, max_pages, num_pages;
    int causal, has_win;
    long win;
    float scale;
    int kv_split;           // grid.z shares of each workgroup's own tile range
};

void launch_attn_fwd_paged(const PagedPrefillParams& p, int head_dim, bool fp8,
                           hipStream_t stream);

// Fp8FwdCore is all a launch with the standard mask reads, and all that the
// instantiations with the constant mask take as their kernel argument (the
// PAIRED kernels keep a copy in a stack frame); the launcher hands the
// geometry of Fp8FwdParams only to the instantiations that read it.
struct Fp8FwdCore {
    const void* q;      // e4m3 bytes (B, Nq, H, D)
    const void* k;      // e4m3 bytes (B, Nk, H, D)
    const void* vt;     // e4m3 bytes (B, H, D, Nk)  — host-pre-transposed V
    const void* qs;     // e8m0 bytes (B, Nq, H, D/64): per (row, 64-d chunk)
    const void* ks;     // e8m0 bytes (B, Nk, HK, D/64)
    const void* vs;     // e8m0 bytes (B, HK, D, Nvs): per (d row, 64-kv chunk)
    void* out;          // bf16 (B, Nq, H, D)
    float* lse;         // fp32 (B, H, Nq)
    int b, h, hk;       // GQA: kv heads (qh pairs qh % hk)
    long nq, nk;        // PADDED sizes (nq % 256 == 0, nk % 128 == 0) — the
                        // wrapper pads the quantized buffers; strides use these
    long nk_true;       // true kv length: keys j >= nk_true are masked out
    int nvs;            // Nk / 64
    float scale;
    int causal;         // j <= qpos(i)
    int paired;         // total q tiles T (PAIRED launches)
};

struct Fp8FwdParams : Fp8FwdCore {
    // mask geometry (attn_mask.h): qpos(i) = i * q_stride + diag, window
    // qpos(i) - j <= win when has_win.  diag 0, q_stride 1, no window is the
    // standard mask and runs the instantiations with the constant mask.
    int has_win;
    long diag, q_stride, win;
};

void launch_attn_fwd_fp8(const Fp8FwdParams& p, int head_dim, hipStream_t stream);

struct RotaryParams {
    const void* x;      // bf16 (B, N, H, D)
    const float* cos_t; // fp32 (N, D/2) host-precomputed table
    const float* sin_t; // fp32 (N, D/2)
    void* out;          // bf16 (B, N, H, D)
    long rows;          // B * N * H
    int n, h, d;
    float sin_sign;     // +1 forward, -1 inverse (backward)
};

void launch_rotary(const RotaryParams& p, int head_dim, hipStream_t stream);

}  // namespace ring_attn
