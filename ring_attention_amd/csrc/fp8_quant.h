// MX-FP8 quantisation rule, shared by every kernel that writes e4m3 + e8m0
// (quantize_fp8.hip, paged_kv_append_kernel): the block exponent from the
// float's own bits and the exact power-of-two scaling into packed e4m3.
// Compiler builtins only, so files that switch packed f32 ops off can inline it.
#pragma once

#include <hip/hip_runtime.h>

namespace ring_attn {

// e = clamp(ceil(log2(max(amax, 2^-126) / 448)), -127, 127), integer-exact:
// with amax = mant * 2^ex (mant in [1, 2)) and 448 = 1.75 * 2^8 this is
// ex - 8 when mant <= 1.75 and ex - 7 otherwise; zero / subnormal amax
// clamps to 2^-126 and lands on the lower clamp.  The e8m0 byte is e + 127.
__device__ __forceinline__ int e8m0_exponent(float amax) {
    const unsigned bits = __builtin_bit_cast(unsigned, amax);
    const int ex = (int)((bits >> 23) & 0xffu);
    const unsigned mant = bits & 0x7fffffu;
    const int e = ex == 0 ? -127 : ex - 127 - 8 + (mant > 0x600000u ? 1 : 0);
    return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// four floats * 2^-e (exact) -> four e4m3 bytes, round-to-nearest-even,
// x0 in the low byte
__device__ __forceinline__ unsigned e4m3_pack4(float x0, float x1, float x2, float x3, int e) {
    int u = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_ldexpf(x0, -e), __builtin_ldexpf(x1, -e),
                                            0, false);
    u = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_ldexpf(x2, -e), __builtin_ldexpf(x3, -e),
                                        u, true);
    return (unsigned)u;
}

}  // namespace ring_attn
