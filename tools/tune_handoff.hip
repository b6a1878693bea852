// tune_handoff.hip -- does a consumer launch find its producer's outputs in the Infinity Cache when it walks the other way?
// Writer: 3 reads, 3 writes (shaped like the fused split: a, b, coefficients -> 3 shares).  Reader: 3 reads, 1 write (shaped
// like the recombination: 3 shares -> y), launched right after the writer on the same stream and reading its three rows.
// 80 MB rows, 16 B per lane, non-temporal loads, uncapped grid; four rotating buffer sets, so every writer starts cold.
// The reader walks its blocks ascending (as the writer does) or descending (whole blocks reversed, lanes ascending);
// the writer stores non-temporally (as the library does) or with the default policy.  Times: events around each launch.
// Second part (profiles/r19_handoff_account.md): the pair with a cache hint of its own on each side -- the writer's cold
// loads nt / plain / sc1 / sc0 sc1, its kept stores plain / sc1, the reader's loads of the handed rows nt / plain, the reader
// ascending / whole blocks reversed -- through the buffer builtins, whose aux argument carries the hint (the first line of
// that part, nt / plain / nt / asc, is the first part's "default stores, reader asc" again: the two must time the same).
//   hipcc --offload-arch=gfx950 -O3 tools/tune_handoff.hip -o build/tune_handoff
//   tune_handoff            both parts, two rounds
//   tune_handoff counters   one round of "nt stores, reader cold asc" and of the second part, after two calibrations (a
//                           copy of one row; one row read twice back to back), for a run under
//                           rocprofv3 --kernel-trace --pmc FETCH_SIZE (or WRITE_SIZE); every line is 160 launches, writer and
//                           reader alternating, the last 80 of them timed (tools/handoff_account.py summarize-probe)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
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

// ---- the pair with per-side cache hints (aux of the buffer builtins on gfx950: sc0 = 1, nt = 2, sc1 = 16) ----------------
enum { H_PLAIN = 0, H_NT = 2, H_SC1 = 16, H_SC0SC1 = 17 };
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rows_of(const void* p, size_t stride) {      // three rows: < 2^31 bytes
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)(3 * stride * 16), 0x00020000);
}
template <int LD, int ST>
__global__ __launch_bounds__(256) void k_writer_h(const u32x4* __restrict__ in, u32x4* __restrict__ sh, size_t n, size_t stride) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const __amdgpu_buffer_rsrc_t ri = rows_of(in, stride), ro = rows_of(sh, stride);
    const int off = (int)(i * 16), row = (int)(stride * 16);
    const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(ri, off, 0, LD);
    const u32x4 b = __builtin_amdgcn_raw_buffer_load_b128(ri, off, row, LD);
    const u32x4 c = __builtin_amdgcn_raw_buffer_load_b128(ri, off, 2 * row, LD);
    const u32x4 s0 = a * b + c, s1 = s0 + c, s2 = s1 + c;
    __builtin_amdgcn_raw_buffer_store_b128(s0, ro, off, 0, ST);
    __builtin_amdgcn_raw_buffer_store_b128(s1, ro, off, row, ST);
    __builtin_amdgcn_raw_buffer_store_b128(s2, ro, off, 2 * row, ST);
}
template <int LD>
__global__ __launch_bounds__(256) void k_reader_h(const u32x4* __restrict__ sh, u32x4* __restrict__ out, size_t n, size_t stride,
                                                  int desc) {
    const size_t blk = desc ? (size_t)(gridDim.x - 1 - blockIdx.x) : (size_t)blockIdx.x;
    const size_t i = blk * 256 + threadIdx.x;
    if (i >= n) return;
    const __amdgpu_buffer_rsrc_t ri = rows_of(sh, stride);
    const int off = (int)(i * 16), row = (int)(stride * 16);
    const u32x4 s0 = __builtin_amdgcn_raw_buffer_load_b128(ri, off, 0, LD);
    const u32x4 s1 = __builtin_amdgcn_raw_buffer_load_b128(ri, off, row, LD);
    const u32x4 s2 = __builtin_amdgcn_raw_buffer_load_b128(ri, off, 2 * row, LD);
    __builtin_nontemporal_store(s0 * 3u + s1 * 5u + s2 * 7u, out + i);
}
typedef void (*writer_fn)(const u32x4*, u32x4*, size_t, size_t);
typedef void (*reader_fn)(const u32x4*, u32x4*, size_t, size_t, int);
struct Hint {
    const char* name;
    int aux;
};
static const Hint LOADS_W[4] = {{"nt", H_NT}, {"plain", H_PLAIN}, {"sc1", H_SC1}, {"sc0sc1", H_SC0SC1}};
static const Hint STORES_W[2] = {{"plain", H_PLAIN}, {"sc1", H_SC1}};
static const Hint LOADS_R[2] = {{"nt", H_NT}, {"plain", H_PLAIN}};
static writer_fn writer_of(int ld, int st) {
#define W_(L, S) if (ld == L && st == S) return k_writer_h<L, S>;
#define WL_(L) W_(L, H_PLAIN) W_(L, H_SC1)
    WL_(H_NT) WL_(H_PLAIN) WL_(H_SC1) WL_(H_SC0SC1)
#undef WL_
#undef W_
    return nullptr;
}
static reader_fn reader_of(int ld) { return ld == H_NT ? k_reader_h<H_NT> : k_reader_h<H_PLAIN>; }

// calibrations of the counter runs: exactly one row in and one row out; one row in, nothing out
__global__ __launch_bounds__(256) void k_calib_copy(const u32x4* __restrict__ in, u32x4* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) __builtin_nontemporal_store(__builtin_nontemporal_load(in + i), out + i);
}
__global__ __launch_bounds__(256) void k_calib_read(const u32x4* __restrict__ in, u32x4* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u32x4 v = in[i];                                                    // default policy: the row may stay cached
    if (v.x == 0x12345678u && v.y == 0x9abcdef0u) out[i] = v;                 // never true: keeps the load alive
}

int main(int argc, char** argv) {
    const bool counters = argc > 1 && !strcmp(argv[1], "counters");
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
    // wk / rk: the pair with per-side hints; without them the first part's kernels
    auto run = [&](const char* name, bool nt_store, int desc, bool cold, writer_fn wk = nullptr, reader_fn rk = nullptr) {
        std::vector<double> tw, tr;
        for (int pass = 0; pass < 2; ++pass) {  // pass 0 warms up
            for (int r = 0; r < reps; ++r) {
                const int s = r % SETS, sr = cold ? (r + 1) % SETS : s;
                CK(hipEventRecord(ev[3 * r]));
                if (wk)
                    hipLaunchKernelGGL(wk, dim3(grid), dim3(256), 0, 0, in[s], sh[s], n, stride);
                else if (nt_store)
                    hipLaunchKernelGGL(k_writer<true>, dim3(grid), dim3(256), 0, 0, in[s], sh[s], n, stride);
                else
                    hipLaunchKernelGGL(k_writer<false>, dim3(grid), dim3(256), 0, 0, in[s], sh[s], n, stride);
                CK(hipEventRecord(ev[3 * r + 1]));
                if (rk)
                    hipLaunchKernelGGL(rk, dim3(grid), dim3(256), 0, 0, sh[sr], out[s], n, stride, desc);
                else
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
        printf("%-44s writer %6.1f us (%5.0f GB/s)  reader %6.1f us [%5.1f..%5.1f] (%5.0f GB/s)  pair %6.1f us\n", name, w,
               6.0 * n * 16 / (w * 1e-6) / 1e9, rd, tr[reps / 10], tr[reps - 1 - reps / 10], 4.0 * n * 16 / (rd * 1e-6) / 1e9,
               w + rd);
        fflush(stdout);
    };
    // writer loads / writer stores / reader loads / reader walk
    auto hinted = [&]() {
        for (const Hint& lw : LOADS_W)
            for (const Hint& sw : STORES_W)
                for (const Hint& lr : LOADS_R)
                    for (int desc = 0; desc < 2; ++desc) {
                        char name[64];
                        snprintf(name, sizeof name, "hints %s / %s / %s / %s", lw.name, sw.name, lr.name, desc ? "rev" : "asc");
                        run(name, false, desc, false, writer_of(lw.aux, sw.aux), reader_of(lr.aux));
                    }
    };
    if (counters) {
        hipLaunchKernelGGL(k_calib_copy, dim3(grid), dim3(256), 0, 0, in[0], out[0], n);
        // 3 x 240 MB of other rows first, so that the row starts cold; then twice back to back
        for (int s = 1; s < SETS; ++s)
            hipLaunchKernelGGL(k_calib_copy, dim3((unsigned)((3 * stride + 255) / 256)), dim3(256), 0, 0, in[s], sh[s], 3 * stride);
        hipLaunchKernelGGL(k_calib_read, dim3(grid), dim3(256), 0, 0, in[0], out[0], n);
        hipLaunchKernelGGL(k_calib_read, dim3(grid), dim3(256), 0, 0, in[0], out[0], n);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        printf("-- counters\n");
        run("nt stores, reader cold asc", true, 0, true);
        hinted();
        return 0;
    }
    for (int round = 0; round < 2; ++round) {
        printf("-- round %d\n", round);
        run("nt stores, reader cold asc", true, 0, true);
        run("nt stores, reader cold desc", true, 1, true);
        run("nt stores, reader asc", true, 0, false);
        run("nt stores, reader desc", true, 1, false);
        run("default stores, reader cold asc", false, 0, true);
        run("default stores, reader asc", false, 0, false);
        run("default stores, reader desc", false, 1, false);
        hinted();
    }
    return 0;
}
