// Integer sort keys for floats, and the wave-level fence of an LDS sorting network (sliced_w2.hip, dad.hip).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned ord_f32(float f) {  // order-preserving float -> unsigned (-0 sorts below +0: add 0.f first)
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord_f32(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// orders this wave's LDS accesses across a step of the network that no other wave takes part in (compiler fence + wave barrier)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
