// Moving average of ALL teacher parameters of a BYOL wrapper in one launch, in place.
//
// The reference updates the teacher with `params_t.data = params_t.data * d + params_s.data * (1 - d)` in a Python loop
// (trainer/byol_wrapper.py:38-40, called from trainer/byol_trainer.py:22): three elementwise launches and a fresh allocation for
// each of the ~110 parameter tensors of PNA + Net3D, and a new storage for every teacher tensor every step.  This kernel walks a
// device-resident table of <= 4 K-element chunks built once per wrapper (as adam.hip does) and writes the teacher where it is.
//
// Arithmetic: the reference's three roundings per element and nothing else -  fl(fl(t * d) + fl(s * (1 - d)))  with d and 1 - d
// the fp32 values torch makes of the Python scalars (the caller forms 1 - d in double and rounds once).  hipcc contracts a * b + c
// into one fused multiply-add by default, which rounds once where the reference rounds twice: the products and the sum go through
// the non-contracting intrinsics, so the teacher follows the reference's trajectory bit for bit.
#include "common.h"

namespace i3d {

struct EmaChunk {       // device table entry: one <= 4096-element piece of a (teacher, student) parameter pair
    float* t;
    const float* s;
    int n;
    int pad;
};

constexpr int EMA_CHUNK = 4096;

__device__ __forceinline__ float ema_update(float t, float s, float decay, float one_minus_decay) {
    return __fadd_rn(__fmul_rn(t, decay), __fmul_rn(s, one_minus_decay));
}

__global__ void __launch_bounds__(256)
ema_kernel(const EmaChunk* __restrict__ table, int n_chunks, float decay, float one_minus_decay) {
    I3D_CHAIN_PRIO();
    if ((int)blockIdx.x >= n_chunks) return;
    const EmaChunk c = table[blockIdx.x];
    const bool vec = ((((uintptr_t)c.t | (uintptr_t)c.s) & 15) == 0);
    int done = 0;
    if (vec) {
        const int n4 = c.n / 4;
        for (int i = threadIdx.x; i < n4; i += 256) {
            float4 t = reinterpret_cast<float4*>(c.t)[i];
            const float4 s = reinterpret_cast<const float4*>(c.s)[i];
            t.x = ema_update(t.x, s.x, decay, one_minus_decay);
            t.y = ema_update(t.y, s.y, decay, one_minus_decay);
            t.z = ema_update(t.z, s.z, decay, one_minus_decay);
            t.w = ema_update(t.w, s.w, decay, one_minus_decay);
            reinterpret_cast<float4*>(c.t)[i] = t;
        }
        done = n4 * 4;
    }
    for (int i = done + threadIdx.x; i < c.n; i += 256) c.t[i] = ema_update(c.t[i], c.s[i], decay, one_minus_decay);
}

}  // namespace i3d

using namespace i3d;

extern "C" int i3d_ema_chunk_elems(void) { return EMA_CHUNK; }
extern "C" int i3d_ema_chunk_bytes(void) { return (int)sizeof(EmaChunk); }

extern "C" int i3d_ema_update(const void* chunk_table, int n_chunks, float decay, float one_minus_decay, void* stream) {
    I3D_CHECK_ARG(chunk_table != nullptr && n_chunks > 0, "bad arguments");
    hipLaunchKernelGGL(ema_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const EmaChunk*)chunk_table, n_chunks, decay,
                       one_minus_decay);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
