// tune_handoff.hip -- does a consumer launch find its producer's outputs in the Infinity Cache when it walks the other way?
// Writer: 3 reads, 3 writes (shaped like the fused split: a, b, coefficients -> 3 shares).  Reader: 3 reads, 1 write (shaped
// like the recombination: 3 shares -> y), launched right after the writer on the same stream and reading its three rows.
// 80 MB rows, 16 B per lane, non-temporal loads, uncapped grid; four rotating buffer sets, so every writer starts cold.
// The reader walks its blocks ascending (as the writer does) or descending (whole blocks reversed, lanes ascending);
// the writer stores non-temporally (as the library does) or with the default policy.  Times: events around each launch.
//   hipcc --offload-arch=gfx950 -O3 tools/tune_handoff.hip -o build/tune_handoff
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define CK(x)                                                                                      \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));      \
            exit(1);                                                                               \
        }                                                                                          \
    } while (0)

template <bool NT_STORE>
__global__ __launch_bounds__(256) void k_writer(const u32x4* __restrict__ in, u32x4* __restrict__ sh, size_t n, size_t stride) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u32x4 a = __builtin_nontemporal_load(in + i);
    const u32x4 b = __builtin_nontemporal_load(in + stride + i);
    const u32x4 c = __builtin_nontemporal_load(in + 2 * stride + i);
    const u32x4 s0 = a * b + c, s1 = s0 + c, s2 = s1 + c;
    if (NT_STORE) {
        __builtin_nontemporal_store(s0, sh + i);
        __builtin_nontemporal_store(s1, sh + stride + i);
        __builtin_nontemporal_store(s2, sh + 2 * stride + i);
    } else {
        sh[i] = s0;
        sh[stride + i] = s1;
        sh[2 * stride + i] = s2;
    }
}

__global__ __launch_bounds__(256) void k_reader(const u32x4* __restrict__ sh, u32x4* __restrict__ out, size_t n, size_t stride,
                                                int desc) {
    const size_t blk = desc ? (size_t)(gridDim.x - 1 - blockIdx.x) : (size_t)blockIdx.x;
    const size_t i = blk * 256 + threadIdx.x;
    if (i >= n) return;
    const u32x4 s0 = __builtin_nontemporal_load(sh + i);
    const u32x4 s1 = __builtin_nontemporal_load(sh + stride + i);
    const u32x4 s2 = __builtin_nontemporal_load(sh + 2 * stride + i);
    __builtin_nontemporal_store(s0 * 3u + s1 * 5u + s2 * 7u, out + i);
}

int main() {
    const size_t n = 5000000;           // 80 MB per row (10^7 eight-byte elements)
    const size_t stride = n + 17 * 16;  // skewed pitch as the library does
    const int SETS = 4;                 // 7 rows per set: 3 inputs, 3 shares, 1 output
    std::vector<u32x4*> in(SETS), sh(SETS), out(SETS);
    for (int s = 0; s < SETS; ++s) {
        CK(hipMalloc(&in[s], 3 * stride * 16));
        CK(hipMalloc(&sh[s], 3 * stride * 16));
        CK(hipMalloc(&out[s], stride * 16));
        CK(hipMemset(in[s], 1 + s, 3 * stride * 16));
        CK(hipMemset(sh[s], 0, 3 * stride * 16));
        CK(hipMemset(out[s], 0, stride * 16));
    }
    const unsigned grid = (unsigned)((n + 255) / 256);
    const int reps = 40;
    std::vector<hipEvent_t> ev(3 * reps);
    for (auto& e : ev) CK(hipEventCreate(&e));
    // cold: the reader reads the shares of the set written SETS-1 launch pairs ago (no hand-off, the yardstick)
    auto run = [&](const char* name, bool nt_store, int desc, bool cold) {
        std::vector<double> tw, tr;
        for (int pass = 0; pass < 2; ++pass) {  // pass 0 warms up
            for (int r = 0; r < reps; ++r) {
                const int s = r % SETS, sr = cold ? (r + 1) % SETS : s;
                CK(hipEventRecord(ev[3 * r]));
                if (nt_store)
                    hipLaunchKernelGGL(k_writer<true>, dim3(grid), dim3(256), 0, 0, in[s], sh[s], n, stride);
                else
                    hipLaunchKernelGGL(k_writer<false>, dim3(grid), dim3(256), 0, 0, in[s], sh[s], n, stride);
                CK(hipEventRecord(ev[3 * r + 1]));
                hipLaunchKernelGGL(k_reader, dim3(grid), dim3(256), 0, 0, sh[sr], out[s], n, stride, desc);
                CK(hipEventRecord(ev[3 * r + 2]));
            }
            CK(hipGetLastError());
            CK(hipDeviceSynchronize());
        }
        for (int r = 0; r < reps; ++r) {
            float a, b;
            CK(hipEventElapsedTime(&a, ev[3 * r], ev[3 * r + 1]));
            CK(hipEventElapsedTime(&b, ev[3 * r + 1], ev[3 * r + 2]));
            tw.push_back(a * 1e3);
            tr.push_back(b * 1e3);
        }
        std::sort(tw.begin(), tw.end());
        std::sort(tr.begin(), tr.end());
        const double w = tw[reps / 2], rd = tr[reps / 2];
        printf("%-34s writer %6.1f us (%5.0f GB/s)  reader %6.1f us [%5.1f..%5.1f] (%5.0f GB/s)  pair %6.1f us\n", name, w,
               6.0 * n * 16 / (w * 1e-6) / 1e9, rd, tr[reps / 10], tr[reps - 1 - reps / 10], 4.0 * n * 16 / (rd * 1e-6) / 1e9,
               w + rd);
        fflush(stdout);
    };
    for (int round = 0; round < 2; ++round) {
        printf("-- round %d\n", round);
        run("nt stores, reader cold asc", true, 0, true);
        run("nt stores, reader cold desc", true, 1, true);
        run("nt stores, reader asc", true, 0, false);
        run("nt stores, reader desc", true, 1, false);
        run("default stores, reader cold asc", false, 0, true);
        run("default stores, reader asc", false, 0, false);
        run("default stores, reader desc", false, 1, false);
    }
    return 0;
}
