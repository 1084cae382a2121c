// binhip_multi_tensor.h — the one multi-tensor core of the elementwise kernels that walk a table of tensors passed BY VALUE:
// adam_step_kernel (binopt_adam.hip), grad_sumsq_kernel / grad_scale_kernel (bingrad_norm.hip) and ema_step_kernel (binema_step.hip).
// Internal: nothing here is exported, and each of the three libraries compiles its own copy.  A .hip file keeps its arithmetic, its
// argument checks and its entry points; what it shares with the others lives here, once:
//   RowTable, find_row   the by-value table {rows, first workgroup of every row, n} and a workgroup's binary search for its row
//                        (wave-uniform: scalar loads from the kernel arguments).  No device-side table, no copy, no allocation.
//   Launches             the host side: every row checked before anything is launched, rows packed into launches of at most
//                        MAX_ROWS rows and MAX_BLOCKS workgroups, one loop that issues them.
//   walk_chunk           the device side.  A workgroup owns one CHUNK = THREADS * UNROLL * 4 element chunk of one row.  A whole
//                        chunk of a row whose N pointers are all 16-byte aligned moves 16 B per lane, nothing predicated; the last,
//                        partial chunk of every row, and every row with a misaligned pointer (the gradients of FlatGradAllReduce
//                        are views at any 4-byte offset), take 4 B per lane, consecutive lanes on consecutive floats.  Both paths
//                        load all operands of everything a lane owns, then compute, then store ("Epilogues and
//                        vmcnt"), and both hand every element to the one functor, so they agree bit for bit.
//   shortest_decimal     the decimal a caller wrote for a float coefficient.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <math.h>

namespace multi_tensor {
constexpr int E_ARG = -1, E_SHAPE = -2;                          // BINOPT_ / BINGRAD_ / BINEMA_E_ARG and _E_SHAPE

template <typename Row, int MAX_ROWS>
struct RowTable {
    Row row[MAX_ROWS];
    int first_block[MAX_ROWS + 1];                               // row r owns workgroups first_block[r] .. first_block[r + 1] - 1
    int n;
};

// the row of this workgroup: largest r with first_block[r] <= blockIdx.x  (first_block[0] = 0, first_block[n] = gridDim.x)
template <typename Row, int MAX_ROWS>
__device__ __forceinline__ int find_row(const RowTable<Row, MAX_ROWS>& tab) {
    int lo = 0, hi = tab.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab.first_block[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    return lo;
}

// Host side of a kernel whose workgroups take CHUNK elements each, at most MAX_BLOCKS workgroups per launch.  A row is any struct
// with an int64_t numel.
template <int CHUNK, int64_t MAX_BLOCKS>
struct Launches {
    static int64_t chunks_of(int64_t numel) { return (numel - 1) / CHUNK + 1; }

    // E_ARG / E_SHAPE for a bad table, else the number of workgroups all rows take.  `valid_row`: the row's pointers are non-null.
    template <typename Row, typename Valid>
    static int64_t check_rows(const Row* items, int n, Valid valid_row) {
        if (n < 0 || (n > 0 && !items)) return E_ARG;
        int64_t total = 0;
        for (int i = 0; i < n; ++i) {
            if (!valid_row(items[i]) || items[i].numel < 1) return E_ARG;
            if (chunks_of(items[i].numel) > MAX_BLOCKS) return E_SHAPE;
            total += chunks_of(items[i].numel);
        }
        return total;
    }

    // rows [i, i + k) into `tab`, as many as one launch takes; returns k and the launch's workgroup count
    template <typename Row, int MAX_ROWS>
    static int fill_table(RowTable<Row, MAX_ROWS>& tab, const Row* items, int i, int n, int64_t& blocks) {
        blocks = 0;
        int k = 0;
        for (; k < MAX_ROWS && i + k < n; ++k) {
            const int64_t nb = chunks_of(items[i + k].numel);
            if (blocks + nb > MAX_BLOCKS) break;                 // the rest goes into the next launch
            tab.row[k] = items[i + k];
            tab.first_block[k] = (int)blocks;
            blocks += nb;
        }
        for (int j = k; j <= MAX_ROWS; ++j) tab.first_block[j] = (int)blocks;
        for (int j = k; j < MAX_ROWS; ++j) tab.row[j] = Row{};
        tab.n = k;
        return k;
    }

    // `launch(tab, blocks)` (one hipLaunchKernelGGL) for every launch that rows which passed check_rows take; 0 or the hipError_t
    template <typename Table, typename Row, typename Launch>
    static int for_each_launch(const Row* items, int n, Launch launch) {
        for (int i = 0; i < n;) {
            Table tab;
            int64_t blocks = 0;
            i += fill_table(tab, items, i, n, blocks);
            launch(tab, (unsigned)blocks);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return (int)e;
        }
        return 0;
    }
};

// One workgroup's chunk, starting at element `base` of a row of `numel` (>= 1) elements behind the pointers `row_ptr...` (float* or
// const float*, N of them, no two overlapping).  Every element goes through `f(x, valid)`: x[j] is the element's value behind the
// j-th pointer, which f may change; bit j of WRITES says that the j-th pointer is written back (0: nothing is, as in a reduction).
// `valid` is false for what a lane past the end of the row holds — a reduction drops it by a select, never a branch; on the 16-byte
// path it is the constant true.
template <int THREADS, int UNROLL, unsigned WRITES, typename F, typename... P>
__device__ __forceinline__ void walk_chunk(int64_t numel, int64_t base, F f, P* __restrict__... row_ptr) {
    constexpr int CHUNK = THREADS * UNROLL * 4, N = sizeof...(P);
    static_assert((WRITES >> N) == 0, "a WRITES bit per pointer");
    const float* const ptr[N] = {row_ptr...};                    // the one place that writes casts the const of a written pointer away
    const int t = threadIdx.x;
    uintptr_t low_bits = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) low_bits |= (uintptr_t)ptr[j];
    constexpr int U = UNROLL * 4;                                // elements a lane owns
    if ((low_bits & 15) == 0 && base + CHUNK <= numel) {         // a whole chunk of an aligned row: 16 B per lane, nothing predicated
        float x[U][N];
#pragma unroll
        for (int k = 0; k < UNROLL; ++k)
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float4 q = *(const float4*)(ptr[j] + base + 4 * (k * THREADS + t));
                x[4 * k][j] = q.x; x[4 * k + 1][j] = q.y; x[4 * k + 2][j] = q.z; x[4 * k + 3][j] = q.w;
            }
#pragma unroll
        for (int k = 0; k < U; ++k) f(x[k], true);
#pragma unroll
        for (int k = 0; k < UNROLL; ++k)
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (WRITES >> j & 1)
                    *(float4*)const_cast<float*>(ptr[j] + base + 4 * (k * THREADS + t)) =
                        make_float4(x[4 * k][j], x[4 * k + 1][j], x[4 * k + 2][j], x[4 * k + 3][j]);
    } else {
        // 4 B per lane.  The loads are not predicated (a lane past the end re-reads the row's last element, numel >= 1), so all of
        // them are in flight at once; only the stores are.
        float x[U][N];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int64_t e = min(base + k * THREADS + t, numel - 1);
#pragma unroll
            for (int j = 0; j < N; ++j) x[k][j] = ptr[j][e];
        }
#pragma unroll
        for (int k = 0; k < U; ++k) f(x[k], base + k * THREADS + t < numel);
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int64_t e = base + k * THREADS + t;
            if (e < numel) {
#pragma unroll
                for (int j = 0; j < N; ++j)
                    if (WRITES >> j & 1) const_cast<float*>(ptr[j])[e] = x[k][j];
            }
        }
    }
}

// The shortest decimal that rounds to the float `b` (what printing a float32 shows), as a double.  A caller's beta2 = 0.999 arrives as
// the float 0.99900001287…, and 1 - that is off from 0.001 by 1.3e-5 relative — far outside fp32 rounding of the update; the decimal
// the caller wrote is recovered instead, so that 1 - b carries full fp32 precision (torch casts its double 1 - beta2 the same way).
// For a float that is no short decimal this returns a double within half a float ulp of it.
inline double shortest_decimal(float b) {
    double scale = 1.0;
    for (int k = 1; k <= 9; ++k) {
        scale *= 10.0;                                           // exact in double
        const double d = nearbyint((double)b * scale) / scale;  // an integer over an exact power of ten: correctly rounded
        if ((float)d == b) return d;
    }
    return (double)b;
}
}  // namespace multi_tensor
