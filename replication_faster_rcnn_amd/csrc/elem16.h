// Element types of the network's predictions (DESIGN.md §3 "Predictions in
// 16-bit types"): fp32, or float16 / bfloat16 held as their raw 16-bit patterns.
// A 16-bit value is widened exactly at the load (neither type has a value fp32
// lacks; subnormals are kept) and every result is rounded to nearest even once,
// at the store, as torch's .to(dtype) does: float16 overflows to +-inf, a
// bfloat16 NaN becomes the quiet 0x7FC0.  Nothing is computed in 16 bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/frcnn_capi.h"

namespace frcnn {

struct ElemF32 {
    using raw = float;
    static __device__ __forceinline__ float widen(float r) { return r; }
    static __device__ __forceinline__ float narrow(float v) { return v; }
};

struct ElemF16 {
    using raw = uint16_t;
    static __device__ __forceinline__ float widen(uint16_t r) {
        return static_cast<float>(__builtin_bit_cast(_Float16, r));  // v_cvt_f32_f16
    }
    static __device__ __forceinline__ uint16_t narrow(float v) {
        // The empty asm pins the finished fp32 value in a register.  Without it the compiler folds
        // the multiply that produced v into the conversion (v_fma_mixlo_f16: the exact product
        // rounded straight to 16 bits), which is not the fp32 result rounded once.
        asm volatile("" : "+v"(v));
        return __builtin_bit_cast(uint16_t, static_cast<_Float16>(v));  // nearest even, overflow to +-inf
    }
};

struct ElemBF16 {
    using raw = uint16_t;
    static __device__ __forceinline__ float widen(uint16_t r) { return __uint_as_float(static_cast<uint32_t>(r) << 16); }
    static __device__ __forceinline__ uint16_t narrow(float v) {
        if (v != v) return 0x7FC0u;
        uint32_t u = __float_as_uint(v);
        u += 0x7FFFu + ((u >> 16) & 1u);  // nearest even; a carry out of the exponent is +-inf
        return static_cast<uint16_t>(u >> 16);
    }
};

inline bool dtype_code_ok(int dtype) { return dtype == FRCNN_F32 || dtype == FRCNN_F16 || dtype == FRCNN_BF16; }
inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace frcnn
