// The two block reductions of the small kernels (binhip_loss.hip, binhip_convlstm.hip), for blocks of exactly 256 threads.  Both
// combine in a fixed order, so a result does not depend on the device or the run; the bit pin of tests/small_kernel_bit_cases.py holds
// the pairing to what it was when these were spelled out per kernel.
// (binhip_metrics.hip and bingrad_norm.hip reduce six sums at once and shuffle doubles: other shapes, not these.)
#pragma once
#include <hip/hip_runtime.h>

// One value per thread -> one per block: shuffle within each wave (v = op(v, lane + 32), + 16, ... + 1), one LDS slot per wave,
// op(op(s0, s1), op(s2, s3)).  Every thread must call it, once per kernel (the four slots are not fenced for a second use); every
// thread gets the result.
template <class Op>
__device__ __forceinline__ float block_reduce_waves(float v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_down(v, o, 64));
    __shared__ float sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return op(op(sm[0], sm[1]), op(sm[2], sm[3]));
}

// `n` values -> one per block: thread t combines load(t), load(t + 256), ... onto `init` in that order, the 256 results go through
// an LDS tree with stride 128, 64, ... 1.  Every thread must call it and gets the result; it may be called again (a loop over terms).
template <class T, class Load, class Op>
__device__ __forceinline__ T block_reduce_strided(int n, T init, Load load, Op op) {
    __shared__ T sm[256];
    T acc = init;
    for (int i = threadIdx.x; i < n; i += 256) acc = op(acc, load(i));
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] = op(sm[threadIdx.x], sm[threadIdx.x + o]);
        __syncthreads();
    }
    const T r = sm[0];
    __syncthreads();
    return r;
}

struct BhAdd {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct BhMax {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
};
