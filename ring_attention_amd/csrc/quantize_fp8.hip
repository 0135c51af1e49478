// MX-FP8 operand quantisation: bf16/fp16 q, k, v -> the e4m3 + e8m0 operands
// of attn_fwd_fp8 in ONE launch, and the per-row KV-cache form of the fp8
// decode kernels in one more.  Every input element is read once from HBM and
// every output byte written once; padding (rows beyond n, columns beyond the
// true head dim) is produced in registers as zeros, which the ordinary rule
// turns into data byte 0 and scale byte 0.
//
// The grid is cut by workgroup index into three uniform parts:
//   [0, b * hk * v_tiles)         V tiles        (none in the cache form)
//   [.., + row[0].blocks)         row job on q   (cache form: k)
//   [.., + row[1].blocks)         row job on k   (cache form: v)
//
// Row job.  A group of 8 lanes owns one (row, 64-column chunk): a 16-byte load
// per lane, amax by three DPP xor steps inside the group, four packed e4m3
// converts and one 8-byte store per lane — the chunk leaves as 64 contiguous
// bytes and a wave covers 8 chunks per pass.  Groups are numbered in output
// order, so data byte offset and scale index are linear in the group number
// and only the strided input needs the (b, i, head) decomposition.  Each
// thread issues the loads of its four passes before it reduces the first.
// The cache form widens the group to the whole row (D/8 lanes, a fourth xor
// step at D = 128).
//
// V job.  A workgroup owns (b, kv head, 16384/D keys) for all D columns:
// coalesced 16-byte row loads go to a row-major [key][D] LDS image (32 KB),
// one barrier, then thread (chunk, column) walks ITS 64 keys down the image.
// A wave's 64 lanes read 64 consecutive columns of one image row per step, so
// the transposed read is bank-conflict-free without swizzle or padding, the
// chunk's amax never leaves the lane, and the lane stores its 64 bytes of row
// `column` of v8t as four 16-byte stores.

#include <hip/hip_runtime.h>
#include <cstdint>

#include "attn_common.h"

// New code is built without packed f32 ops (v_pk_mul_f32 and kin); see
// decode_paged_grouped.hip for the rule that follows: only compiler builtins
// and always_inline helpers are called from here.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "fp8_quant.h"

namespace ring_attn {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int QTHREADS = 256;
constexpr int ROW_PASSES = 4;           // groups per thread in the row job
constexpr int V_TILE_ELEMS = 16384;     // keys x D per V tile (32 KB of LDS)

// 16-bit input element -> f32
template <bool HALF>
__device__ __forceinline__ float in_to_f32(unsigned bits16) {
    if constexpr (HALF) {
        return (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
    } else {
        return __builtin_bit_cast(float, bits16 << 16);
    }
}

// max with the lane the DPP control selects (all lanes stay active)
template <int CTRL>
__device__ __forceinline__ float dpp_max(float x) {
    const int xi = __builtin_bit_cast(int, x);
    const int o = __builtin_amdgcn_update_dpp(xi, xi, CTRL, 0xf, 0xf, false);
    return __builtin_fmaxf(x, __builtin_bit_cast(float, o));
}

template <int D, bool HALF, bool ROWSCALE>
__device__ __forceinline__ void quant_rows(const QuantRowSeg& s, unsigned blk, int d_true) {
    constexpr int LPG = ROWSCALE ? D / 8 : 8;        // lanes per scale group
    constexpr int GPR = ROWSCALE ? 1 : D / 64;       // groups per row
    constexpr int GPP = QTHREADS / LPG;              // groups per pass
    const unsigned total = (unsigned)s.b * (unsigned)s.n_pad * (unsigned)s.h * GPR;
    const int l = threadIdx.x % LPG;
    const unsigned g0 = blk * (GPP * ROW_PASSES) + threadIdx.x / LPG;

    u32x4 raw[ROW_PASSES];
    #pragma unroll
    for (int it = 0; it < ROW_PASSES; ++it) {
        const unsigned g = g0 + it * GPP;
        const unsigned r = g / GPR;
        const int col = (int)(g % GPR) * 64 + l * 8;
        const unsigned t = r / (unsigned)s.h;
        const unsigned hh = r - t * (unsigned)s.h;
        const unsigned bb = t / (unsigned)s.n_pad;
        const unsigned i = t - bb * (unsigned)s.n_pad;
        raw[it] = u32x4{0u, 0u, 0u, 0u};
        if (g < total && i < (unsigned)s.n && col < d_true) {
            const unsigned short* src = (const unsigned short*)s.x
                + (long)bb * s.sb + (long)i * s.sn + (long)hh * s.sh + col;
            raw[it] = *(const u32x4*)src;
        }
    }
    #pragma unroll
    for (int it = 0; it < ROW_PASSES; ++it) {
        const unsigned g = g0 + it * GPP;
        float x[8];
        #pragma unroll
        for (int w = 0; w < 4; ++w) {
            x[2 * w] = in_to_f32<HALF>(raw[it][w] & 0xffffu);
            x[2 * w + 1] = in_to_f32<HALF>(raw[it][w] >> 16);
        }
        float amax = 0.f;
        #pragma unroll
        for (int e = 0; e < 8; ++e) amax = __builtin_fmaxf(amax, __builtin_fabsf(x[e]));
        amax = dpp_max<0xB1>(amax);                  // quad_perm [1,0,3,2]: lane ^ 1
        amax = dpp_max<0x4E>(amax);                  // quad_perm [2,3,0,1]: lane ^ 2
        amax = dpp_max<0x141>(amax);                 // row_half_mirror: the other quad
        if constexpr (LPG == 16) amax = dpp_max<0x140>(amax);   // row_mirror: other 8
        const int e = e8m0_exponent(amax);
        u32x2 o;
        o[0] = e4m3_pack4(x[0], x[1], x[2], x[3], e);
        o[1] = e4m3_pack4(x[4], x[5], x[6], x[7], e);
        if (g < total) {
            *(u32x2*)((unsigned char*)s.out8 + (long)g * (LPG * 8) + l * 8) = o;
            if (l == 0) ((unsigned char*)s.scales)[g] = (unsigned char)(e + 127);
        }
    }
}

template <int D, bool HALF>
__device__ __forceinline__ void quant_v_tile(const QuantFp8Params& p, unsigned vb,
                                             unsigned short* img) {
    constexpr int TK = V_TILE_ELEMS / D;             // keys per tile
    constexpr int CPR = D / 8;                       // 16-byte chunks per row
    constexpr int LOADS = TK * CPR / QTHREADS;       // per thread: 8
    const unsigned tile = vb % p.v_tiles;
    const unsigned bh = vb / p.v_tiles;
    const unsigned hh = bh % (unsigned)p.hk;
    const unsigned bb = bh / (unsigned)p.hk;
    const int k0 = (int)tile * TK;
    const unsigned short* src = (const unsigned short*)p.v + (long)bb * p.vsb + (long)hh * p.vsh;

    u32x4 raw[LOADS];
    #pragma unroll
    for (int u = 0; u < LOADS; ++u) {
        const int idx = u * QTHREADS + threadIdx.x;
        const int row = idx / CPR, c = idx % CPR;
        raw[u] = u32x4{0u, 0u, 0u, 0u};
        if (k0 + row < p.nk && c * 8 < p.d)
            raw[u] = *(const u32x4*)(src + (long)(k0 + row) * p.vsn + c * 8);
    }
    #pragma unroll
    for (int u = 0; u < LOADS; ++u)
        *(u32x4*)(img + (u * QTHREADS + threadIdx.x) * 8) = raw[u];

    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

    const int dcol = threadIdx.x % D;
    const int ch = threadIdx.x / D;                  // 64-key chunk of the tile
    const int key0 = k0 + ch * 64;
    if (key0 >= p.nk_pad) return;                    // the last tile may be short
    float x[64];
    float amax = 0.f;
    #pragma unroll
    for (int i = 0; i < 64; ++i) {
        x[i] = in_to_f32<HALF>(img[(ch * 64 + i) * D + dcol]);
        amax = __builtin_fmaxf(amax, __builtin_fabsf(x[i]));
    }
    const int e = e8m0_exponent(amax);
    const long orow = ((long)bb * p.hk + hh) * D + dcol;
    unsigned char* dst = (unsigned char*)p.v8t + orow * p.nk_pad + key0;
    #pragma unroll
    for (int q = 0; q < 4; ++q) {
        u32x4 o;
        #pragma unroll
        for (int w = 0; w < 4; ++w)
            o[w] = e4m3_pack4(x[q * 16 + w * 4], x[q * 16 + w * 4 + 1],
                              x[q * 16 + w * 4 + 2], x[q * 16 + w * 4 + 3], e);
        *(u32x4*)(dst + q * 16) = o;
    }
    ((unsigned char*)p.vs)[orow * (p.nk_pad / 64) + key0 / 64] = (unsigned char)(e + 127);
}

template <int D, bool HALF, bool ROWSCALE>
__global__ __launch_bounds__(QTHREADS) void quantize_fp8_kernel(QuantFp8Params p) {
    unsigned blk = blockIdx.x;
    if constexpr (!ROWSCALE) {
        // V tiles carry the most work per workgroup (32 KB in, a barrier, 64
        // LDS steps), so they are dispatched first and the row blocks fill in
        // behind them
        const unsigned v_blocks = (unsigned)p.b * (unsigned)p.hk * p.v_tiles;
        if (blk < v_blocks) {
            __shared__ __attribute__((aligned(16))) unsigned short img[V_TILE_ELEMS];
            quant_v_tile<D, HALF>(p, blk, img);
            return;
        }
        blk -= v_blocks;
    }
    if (blk < p.row[0].blocks)
        quant_rows<D, HALF, ROWSCALE>(p.row[0], blk, p.d);
    else if (blk - p.row[0].blocks < p.row[1].blocks)
        quant_rows<D, HALF, ROWSCALE>(p.row[1], blk - p.row[0].blocks, p.d);
}

template <int D, bool HALF, bool ROWSCALE>
void launch_one(const QuantFp8Params& p, unsigned blocks, hipStream_t stream) {
    hipLaunchKernelGGL((quantize_fp8_kernel<D, HALF, ROWSCALE>), dim3(blocks),
                       dim3(QTHREADS), 0, stream, p);
}

}  // namespace

void launch_quantize_fp8(QuantFp8Params p, int head_dim, bool fp16, bool row_scale,
                         hipStream_t stream) {
    if (head_dim != 64 && head_dim != 128) __builtin_trap();
    const long lpg = row_scale ? head_dim / 8 : 8;
    const long gpr = row_scale ? 1 : head_dim / 64;
    const long per_block = (QTHREADS / lpg) * ROW_PASSES;
    for (QuantRowSeg& s : p.row) {
        const long groups = (long)s.b * s.n_pad * s.h * gpr;
        s.blocks = (unsigned)((groups + per_block - 1) / per_block);
    }
    const long tk = V_TILE_ELEMS / head_dim;
    p.v_tiles = row_scale ? 0u : (unsigned)((p.nk_pad + tk - 1) / tk);
    const unsigned blocks = p.row[0].blocks + p.row[1].blocks
                            + (row_scale ? 0u : (unsigned)p.b * p.hk * p.v_tiles);
    if (blocks == 0) return;
#define LAUNCH_QUANT(D_)                                                         \
    do {                                                                         \
        if (row_scale) {                                                         \
            if (fp16) launch_one<D_, true, true>(p, blocks, stream);             \
            else launch_one<D_, false, true>(p, blocks, stream);                 \
        } else {                                                                 \
            if (fp16) launch_one<D_, true, false>(p, blocks, stream);            \
            else launch_one<D_, false, false>(p, blocks, stream);                \
        }                                                                        \
    } while (0)
    if (head_dim == 64) LAUNCH_QUANT(64);
    else LAUNCH_QUANT(128);
#undef LAUNCH_QUANT
}

}  // namespace ring_attn

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif
