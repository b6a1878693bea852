// api.hip -- the extern "C" boundary of libffgpu.so (declared in include/ffgpu.h).
// Host-side only: classifies the modulus, builds the field policy, dispatches
// to the per-policy launcher tables (ops_*.hip).  No arithmetic on array data
// happens on the host: if the GPU path cannot run, the call returns an error.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <mutex>
#include <new>

#include "../../include/ffgpu.h"
#include "../../include/ffgpu_math.h"
#include "handoff.hpp"
#include "hostint.hpp"
#include "operands.hpp"
#include "kernels.hpp"
#include "policy_build.hpp"
#include "keccak_geom.hpp"

using namespace ffgpu;

// per-policy launcher tables (one translation unit each, see ops_*.hip)
const FieldOps* ffgpu_ops_pm64_mersenne();   // PM64<false,true>
const FieldOps* ffgpu_ops_pm64_k64();        // PM64<true,false>
const FieldOps* ffgpu_ops_pm64_gen();        // PM64<false,false>
const FieldOps* ffgpu_ops_rc64();
const FieldOps* ffgpu_ops_rc32();
const FieldOps* ffgpu_ops_pm128_k128();      // PM128<true>
const FieldOps* ffgpu_ops_pm128_gen();       // PM128<false>
const FieldOps* ffgpu_ops_pm96();            // PM96
const FieldOps* ffgpu_ops_pm192();           // PM192
const FieldOps* ffgpu_ops_mont192();         // MONT192
const FieldOps* ffgpu_ops_mont128();
const FieldOps* ffgpu_ops_gf2p8();
const FieldOps* ffgpu_ops_gf2w32();
const FieldOps* ffgpu_ops_gf2w64();
const FieldOps* ffgpu_ops_gf2w128();

static thread_local char g_hip_err[256] = "";

static int hip_fail(hipError_t e, const char* what) {
    snprintf(g_hip_err, sizeof(g_hip_err), "%s: %s", what, hipGetErrorString(e));
    return FFGPU_EHIP;
}
#define HIPCHK(call)                                     \
    do {                                                 \
        hipError_t e_ = (call);                          \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

// what a launcher reported -> the status of the entry point (and the text of ffgpu_last_hip_error)
static int status_of(const LaunchStatus& s) {
    switch (s.code) {
        case L_OK: return FFGPU_OK;
        case L_NOT_SUPPORTED:
        case L_DECLINED: return FFGPU_ENOTSUP;      // (declined: only where no other route is left)
        case L_HIP_ERROR: return hip_fail(s.hip, "kernel launch");
        default: return FFGPU_EINVAL;               // bad argument, plan refused, workspace too small
    }
}

struct DeviceGuard {
    int prev;
    bool switched;
    explicit DeviceGuard(int dev) : prev(-1), switched(false) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) {
            if (hipSetDevice(dev) == hipSuccess) switched = true;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

// grow-only device scratch of ffgpu_matmul (digit planes, split-K slabs), ONE BUFFER PER STREAM: launches on
// different streams never share scratch, and a buffer is only freed after its own stream has drained
struct ScratchSlots {
    struct Slot {
        hipStream_t stream = nullptr;
        void* ptr = nullptr;
        size_t bytes = 0;
        int used = 0;
    } slots[8];
    std::mutex mu;
    // the buffer of `st`, at least `want` bytes unless the device has none to give (*ptr may then be smaller or null: the
    // VALU kernels need no scratch)
    int get(hipStream_t st, size_t want, void** ptr, size_t* bytes) {
        std::lock_guard<std::mutex> lk(mu);
        Slot* slot = nullptr;
        for (auto& sc : slots)
            if (sc.used && sc.stream == st) slot = &sc;
        if (!slot) {
            for (auto& sc : slots)
                if (!sc.used && !slot) slot = &sc;
            if (!slot) {                                     // more streams than slots: recycle the smallest buffer
                slot = &slots[0];
                for (auto& sc : slots)
                    if (sc.bytes < slot->bytes) slot = &sc;
                HIPCHK(hipStreamSynchronize(slot->stream));
                if (slot->ptr) (void)hipFree(slot->ptr);
                slot->ptr = nullptr;
                slot->bytes = 0;
            }
            slot->used = 1;
            slot->stream = st;
        }
        if (slot->bytes < want) {
            HIPCHK(hipStreamSynchronize(st));                // queued work may still read the old buffer
            if (slot->ptr) (void)hipFree(slot->ptr);
            slot->ptr = nullptr;
            slot->bytes = 0;
            if (hipMalloc(&slot->ptr, want) == hipSuccess) slot->bytes = want;
            else (void)hipGetLastError();                    // no scratch: the VALU kernels need none
        }
        *ptr = slot->ptr;
        *bytes = slot->bytes;
        return FFGPU_OK;
    }
    void release() {                                         // (the context's destructor, under its device guard)
        for (auto& sc : slots)
            if (sc.ptr) (void)hipFree(sc.ptr);
    }
};

// Every member starts at zero (several are read before they are first written).
struct ffgpu_ctx {
    int kind = 0;
    int reduction = 0;
    int device = 0;
    int elem_bytes = 0;
    int policy_kind = 0;
    const FieldOps* ops = nullptr;
    uint64_t rng_r[2] = {};  // 2^W mod p for the keystream sampler
    ffgpu::LaunchCfg lc = {}; // launch shape and run-time switches, filled when the context is created
    int gf8_tab_min = 0;    // GF(2^n<=8): arrays of at least this many elements multiply through LDS tables
    alignas(16) unsigned char gf8_tables[1536] = {};
    int gf2w_limbs = 0;     // GF(2^n), 9 <= n <= 128: 1 or 2 limbs -> windowed multiplication kernel
    alignas(16) unsigned char gf2w_rtable[256] = {};
    // last S-box table built for this context (depends only on rows8, b); guarded by sbox_mu
    uint8_t sbox_key[9] = {};
    int sbox_valid = 0;
    uint8_t sbox_lut[256] = {};
    std::mutex sbox_mu;
    alignas(16) unsigned char policy[128] = {};
    uint64_t modulus[3] = {};
    ScratchSlots scratch;
    // which outputs feed the next launch on their stream (handoff.hpp); guarded by handoff_mu
    HandoffTracker handoff = {};
    std::mutex handoff_mu;
    void* gf8_tables_dev = nullptr;   // device copy of gf8_tables (lazily, for the fused GF(2^n<=8) product); guarded by gf8_mu
    std::mutex gf8_mu;
    // tables of the fused S-box layer (ffgpu_gf256_sbox_layer) for the last affine map used with this context; guarded by sbl_mu
    void* sbl_tables_dev = nullptr;
    unsigned char sbl_key[72] = {};
    int sbl_valid = 0;
    std::mutex sbl_mu;
    // opt-in timing of the most recent compute call (ffgpu_ctx_set_timing / ffgpu_last_kernel_ms)
    int timing = 0, timed = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // timing mode 2 (ffgpu_busy_ms): one event pair per compute call, harvested into acc_ms
    enum { ACC_MAX = 256 };
    hipEvent_t acc_ev[2 * ACC_MAX] = {};
    int acc_made = 0, acc_n = 0;
    double acc_ms = 0.0;
    unsigned long long acc_calls = 0;

    ~ffgpu_ctx() {
        DeviceGuard g(device);
        scratch.release();
        if (gf8_tables_dev) (void)hipFree(gf8_tables_dev);
        if (sbl_tables_dev) (void)hipFree(sbl_tables_dev);
        for (int i = 0; i < 2 * acc_made; ++i) (void)hipEventDestroy(acc_ev[i]);
        if (ev0) {
            (void)hipEventDestroy(ev0);
            (void)hipEventDestroy(ev1);
        }
    }
};

// sum the elapsed time of the recorded event pairs of accumulate mode into acc_ms (waits for the last one)
static void acc_harvest(ffgpu_ctx* c) {
    if (c->acc_n == 0) return;
    (void)hipEventSynchronize(c->acc_ev[2 * (c->acc_n - 1) + 1]);
    for (int i = 0; i < c->acc_n; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->acc_ev[2 * i], c->acc_ev[2 * i + 1]) == hipSuccess) c->acc_ms += ms;
    }
    c->acc_calls += (unsigned long long)c->acc_n;
    c->acc_n = 0;
}

// brackets the launches of one API call with two events when the context has timing switched on
struct LaunchTimer {
    ffgpu_ctx* c;
    hipStream_t st;
    int slot;
    LaunchTimer(ffgpu_ctx* ctx, hipStream_t s) : c(ctx && ctx->timing ? ctx : nullptr), st(s), slot(-1) {
        if (!c) return;
        if (c->timing == 2) {
            if (c->acc_n == ffgpu_ctx::ACC_MAX) acc_harvest(c);
            if (c->acc_n == c->acc_made) {
                if (hipEventCreate(&c->acc_ev[2 * c->acc_made]) != hipSuccess ||
                    hipEventCreate(&c->acc_ev[2 * c->acc_made + 1]) != hipSuccess) {
                    c = nullptr;
                    return;
                }
                ++c->acc_made;
            }
            slot = c->acc_n++;
            (void)hipEventRecord(c->acc_ev[2 * slot], st);
        } else {
            (void)hipEventRecord(c->ev0, st);
        }
    }
    ~LaunchTimer() {
        if (!c) return;
        if (slot >= 0) {
            (void)hipEventRecord(c->acc_ev[2 * slot + 1], st);
        } else {
            (void)hipEventRecord(c->ev1, st);
            c->timed = 1;
        }
    }
};

// The scope of one compute call, opened once its arguments have been checked: the context's device is current, the
// call's launches are timed when timing is on, `st` is its stream and `lc` its launch shape.  A tracked call (one whose
// arrays take part in the hand-off, handoff.hpp) names its kind and byte ranges: lc.policy (CachePolicy, kernels.hpp) then
// says to keep the outputs when the tracker predicts that the next launch on the stream reads them -- write-through for
// share generation, the flavour measured for it, the default policy for the other kinds -- and whether the call reads what
// the call before it kept; what the call reads settles the prediction for the call before it.
struct CallScope {
    DeviceGuard dev;
    LaunchTimer timer;
    hipStream_t st;
    LaunchCfg lc;
    CallScope(ffgpu_ctx* ctx, void* stream)
        : dev(ctx->device), timer(ctx, (hipStream_t)stream), st((hipStream_t)stream), lc(ctx->lc) {}
    CallScope(ffgpu_ctx* ctx, void* stream, int kind, const ByteRange* in, int nin, const ByteRange& out) : CallScope(ctx, stream) {
        if (lc.handoff) {
            std::lock_guard<std::mutex> lk(ctx->handoff_mu);
            int fed = 0;
            const int keep = ctx->handoff.launch(stream, kind, in, nin, &out, 1, &fed);
            lc.policy = (keep ? (kind == HK_SPLIT ? CP_ST_SC1 : CP_ST_PLAIN) : CP_ST_NT) | (fed ? CP_FED : 0);
        }
    }
};

static const FieldOps* ops_for(int kind) {
    switch (kind) {
        case POL_PM64_MERSENNE: return ffgpu_ops_pm64_mersenne();
        case POL_PM64_K64: return ffgpu_ops_pm64_k64();
        case POL_PM64_GEN: return ffgpu_ops_pm64_gen();
        case POL_RC64: return ffgpu_ops_rc64();
        case POL_RC32: return ffgpu_ops_rc32();
        case POL_PM128_K128: return ffgpu_ops_pm128_k128();
        case POL_PM128_GEN: return ffgpu_ops_pm128_gen();
        case POL_PM96: return ffgpu_ops_pm96();
        case POL_PM192: return ffgpu_ops_pm192();
        case POL_MONT192: return ffgpu_ops_mont192();
        case POL_MONT128: return ffgpu_ops_mont128();
        case POL_GF2P8: return ffgpu_ops_gf2p8();
        case POL_GF2W32: return ffgpu_ops_gf2w32();
        case POL_GF2W64: return ffgpu_ops_gf2w64();
        case POL_GF2W128: return ffgpu_ops_gf2w128();
        default: return nullptr;
    }
}

extern "C" {

int ffgpu_abi_version(void) { return FFGPU_ABI_VERSION; }

const char* ffgpu_strerror(int status) {
    switch (status) {
        case FFGPU_OK: return "ok";
        case FFGPU_EINVAL: return "invalid argument";
        case FFGPU_ENOTSUP: return "field or size not supported by this build";
        case FFGPU_EHIP: return "HIP runtime error";
        case FFGPU_ESTALE: return "interprocess mapping does not show the exported row (stale mapping)";
        case FFGPU_EMODULUS: return "unusable modulus";
        case FFGPU_ENOMEM: return "out of device memory";
        default: return "unknown status";
    }
}

const char* ffgpu_last_hip_error(void) { return g_hip_err; }

int ffgpu_device_count(int* count) {
    if (!count) return FFGPU_EINVAL;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return hip_fail(e, "hipGetDeviceCount");
    }
    *count = n;
    return FFGPU_OK;
}

int ffgpu_device_pci_bus_id(int device, char* buf, int len) {
    if (!buf || len < 16 || device < 0) return FFGPU_EINVAL;
    buf[0] = 0;
    hipError_t e = hipDeviceGetPCIBusId(buf, len, device);
    if (e != hipSuccess) return hip_fail(e, "hipDeviceGetPCIBusId");
    return FFGPU_OK;
}

// The library's switches (INTEGRATION.md section 6 lists the same names): an integer outside [lowest, highest] counts as
// not set.  The on/off switches take any integer, 0 is off.
struct Switch {
    const char* name;
    int LaunchCfg::*field;
    double LaunchCfg::*real;      // the one switch that is not an integer
    double def;
    int lowest, highest;
};
static const Switch SWITCHES[] = {
    {"FFGPU_BLOCKS_PER_CU", &LaunchCfg::blocks_per_cu, nullptr, 0, 0, INT_MAX},     // 0: uncapped
    {"FFGPU_MM_MFMA", &LaunchCfg::mm_mfma, nullptr, 1, INT_MIN, INT_MAX},
    {"FFGPU_MM_MFMA_MIN", nullptr, &LaunchCfg::mm_mfma_min, 8e7, 0, 0},
    {"FFGPU_MM_STACK_LOOP_MIN", &LaunchCfg::mm_stack_loop_min, nullptr, 1 << 22, 0, INT_MAX},
    {"FFGPU_GF2W_BITSLICED", &LaunchCfg::gf2w_bitsliced, nullptr, 1, INT_MIN, INT_MAX},
    {"FFGPU_HANDOFF", &LaunchCfg::handoff, nullptr, 1, INT_MIN, INT_MAX},
    {"FFGPU_CONV_WIDE_PER_CU", &LaunchCfg::conv_wide_per_cu, nullptr, 2, 0, INT_MAX},
    {"FFGPU_SCAN_GEOM", &LaunchCfg::scan_geom, nullptr, 0, 0, 2},
    {"FFGPU_SCAN_TILE_THREADS", &LaunchCfg::scan_tile_threads, nullptr, 256, 1, 256},
};

int ffgpu_ctx_create(int kind, const uint64_t* modulus, int nlimbs, int device, ffgpu_ctx** out) {
    if (!modulus || !out || nlimbs < 1 || nlimbs > 3 || device < 0) return FFGPU_EINVAL;
    PolicyBlob pb;
    memset(&pb, 0, sizeof(pb));
    int rc;
    if (kind == FFGPU_PRIME) {
        rc = build_prime_policy3(&pb, modulus, nlimbs);
    } else if (kind == FFGPU_BINARY) {
        rc = build_binary_policy(&pb, modulus, nlimbs);
    } else {
        rc = FFGPU_EINVAL;
    }
    if (rc != FFGPU_OK) return rc;
    // (the secure steps' table goes with the kind: PRIME_CTX is then all an entry needs before it calls through ops->secure)
    const FieldOps* ops = ops_for(pb.kind);
    if (!ops || (ops->secure != nullptr) != (kind == FFGPU_PRIME)) return FFGPU_ENOTSUP;
    ffgpu_ctx* c = new (std::nothrow) ffgpu_ctx();
    if (!c) return FFGPU_ENOMEM;
    c->ops = ops;
    c->kind = kind;
    c->device = device;
    for (int i = 0; i < nlimbs; ++i) c->modulus[i] = modulus[i];
    memcpy(c->policy, pb.bytes, sizeof(c->policy));
    c->reduction = pb.reduction;
    c->elem_bytes = pb.elem_bytes;
    c->policy_kind = pb.kind;
    rng_const(pb, c->rng_r);
    {   // the launch shape and the library's switches: read here, once per context -- no call path looks at the
        // environment or queries the device
        int cus = 256;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
        c->lc.num_cu = cus;
        for (const Switch& sw : SWITCHES) {
            const char* e = getenv(sw.name);
            if (sw.real) {
                c->lc.*sw.real = e ? atof(e) : sw.def;
                continue;
            }
            const int v = e ? atoi(e) : (int)sw.def;
            c->lc.*sw.field = v >= sw.lowest && v <= sw.highest ? v : (int)sw.def;
        }
    }
    if (pb.kind == POL_GF2W64 || pb.kind == POL_GF2W128) {
        // sparse moduli (all MPyC defaults) multiply in registers through the integer multiplier
        // (fields.hpp ff_clmul*); dense moduli use the 4-bit window kernel with LDS tables
        bool in_regs;
        if (pb.kind == POL_GF2W128) {
            GF2W128 f;
            memcpy(&f, pb.bytes, sizeof(f));
            in_regs = (f.fast & 1) != 0;
        } else {
            GF2W64 f;
            memcpy(&f, pb.bytes, sizeof(f));
            in_regs = (f.fast & 1) != 0;
        }
        if (!in_regs) {
            c->gf2w_limbs = pb.kind == POL_GF2W128 ? 2 : 1;
            ffgpu_gf2w_build_rtable(c->policy, c->gf2w_limbs, c->gf2w_rtable);
        }
    }
    if (pb.kind == POL_GF2P8 && ffgpu_gf8_build_tables(c->policy, c->gf8_tables)) {
        c->gf8_tab_min = 1 << 18;   // below this the shift-xor kernel has lower latency
    }
    *out = c;
    return FFGPU_OK;
}

// device copy of the GF(2^n<=8) log/antilog tables for the fused share-generation kernel (made on first use:
// contexts can be created and classified on machines without a GPU)
static const void* gf8_tables_on_device(ffgpu_ctx* ctx) {
    if (!ctx->gf8_tab_min) return nullptr;                 // not a GF(2^n<=8) context with tables
    std::lock_guard<std::mutex> g(ctx->gf8_mu);
    if (!ctx->gf8_tables_dev) {
        void* d = nullptr;
        if (hipMalloc(&d, sizeof(ctx->gf8_tables)) != hipSuccess) return nullptr;
        if (hipMemcpy(d, ctx->gf8_tables, sizeof(ctx->gf8_tables), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d);
            return nullptr;
        }
        ctx->gf8_tables_dev = d;
    }
    return ctx->gf8_tables_dev;
}

int ffgpu_ctx_destroy(ffgpu_ctx* ctx) {
    delete ctx;
    return FFGPU_OK;
}
int ffgpu_ctx_set_timing(ffgpu_ctx* ctx, int enable) {
    if (!ctx) return FFGPU_EINVAL;
    if (enable && !ctx->ev0) {
        DeviceGuard g(ctx->device);
        HIPCHK(hipEventCreate(&ctx->ev0));
        HIPCHK(hipEventCreate(&ctx->ev1));
    }
    if (ctx->timing == 2 && enable != 2) {
        DeviceGuard g(ctx->device);
        acc_harvest(ctx);
    }
    ctx->timing = enable == 2 ? 2 : (enable ? 1 : 0);
    ctx->timed = 0;
    return FFGPU_OK;
}
int ffgpu_busy_ms(ffgpu_ctx* ctx, double* ms, unsigned long long* calls, int reset) {
    if (!ctx) return FFGPU_EINVAL;
    DeviceGuard g(ctx->device);
    acc_harvest(ctx);
    if (ms) *ms = ctx->acc_ms;
    if (calls) *calls = ctx->acc_calls;
    if (reset) {
        ctx->acc_ms = 0.0;
        ctx->acc_calls = 0;
    }
    return FFGPU_OK;
}
int ffgpu_last_kernel_ms(ffgpu_ctx* ctx, float* ms) {
    if (!ctx || !ms || !ctx->timed) return FFGPU_EINVAL;
    DeviceGuard g(ctx->device);
    HIPCHK(hipEventSynchronize(ctx->ev1));
    HIPCHK(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return FFGPU_OK;
}
int ffgpu_ctx_elem_bytes(const ffgpu_ctx* ctx) { return ctx ? ctx->elem_bytes : -1; }
int ffgpu_ctx_reduction(const ffgpu_ctx* ctx) { return ctx ? ctx->reduction : -1; }
int ffgpu_ctx_device(const ffgpu_ctx* ctx) { return ctx ? ctx->device : -1; }

int ffgpu_malloc(ffgpu_ctx* ctx, size_t bytes, void** dptr) {
    if (!ctx || !dptr) return FFGPU_EINVAL;
    DeviceGuard g(ctx->device);
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 16);
    if (e == hipErrorOutOfMemory) return FFGPU_ENOMEM;
    if (e != hipSuccess) return hip_fail(e, "hipMalloc");
    return FFGPU_OK;
}
int ffgpu_free(ffgpu_ctx* ctx, void* dptr) {
    if (!ctx) return FFGPU_EINVAL;
    DeviceGuard g(ctx->device);
    HIPCHK(hipFree(dptr));
    return FFGPU_OK;
}
int ffgpu_h2d(ffgpu_ctx* ctx, void* dst, const void* host_src, size_t bytes, void* stream) {
    if (!ctx || (bytes && (!dst || !host_src))) return FFGPU_EINVAL;
    DeviceGuard g(ctx->device);
    HIPCHK(hipMemcpyAsync(dst, host_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return FFGPU_OK;
}
int ffgpu_d2h(ffgpu_ctx* ctx, void* host_dst, const void* src, size_t bytes, void* stream) {
    if (!ctx || (bytes && (!host_dst || !src))) return FFGPU_EINVAL;
    DeviceGuard g(ctx->device);
    HIPCHK(hipMemcpyAsync(host_dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return FFGPU_OK;
}
// ---- device buffers across co-located party processes (include/ffgpu.h "device-side wire") ----
// first and last 16 bytes of a row in one small synchronous copy (2 rows of 16 bytes, pitch = bytes - 16)
static int ipc_canary(const void* row, size_t bytes, unsigned char* out32) {
    if (bytes < 32) return FFGPU_EINVAL;
    HIPCHK(hipMemcpy2D(out32, 16, row, bytes - 16, 16, 2, hipMemcpyDeviceToHost));
    return FFGPU_OK;
}
int ffgpu_ipc_export(ffgpu_ctx* ctx, const void* ptr, size_t bytes, unsigned char* handle, unsigned long long* offset,
                     unsigned char* canary32, void* stream) {
    if (!ctx || !ptr || !handle || !offset) return FFGPU_EINVAL;
    static_assert(sizeof(hipIpcMemHandle_t) == FFGPU_IPC_HANDLE_BYTES, "handle size");
    DeviceGuard g(ctx->device);
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));          // the row is complete before anybody can open it
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    HIPCHK(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr));
    hipIpcMemHandle_t h;
    HIPCHK(hipIpcGetMemHandle(&h, base));
    memcpy(handle, &h, sizeof(h));
    *offset = (unsigned long long)((const char*)ptr - (const char*)base);
    if (canary32) return ipc_canary(ptr, bytes, canary32);
    return FFGPU_OK;
}
int ffgpu_ipc_open(ffgpu_ctx* ctx, const unsigned char* handle, void** base) {
    if (!ctx || !handle || !base) return FFGPU_EINVAL;
    DeviceGuard g(ctx->device);
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof(h));
    void* p = nullptr;
    HIPCHK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
    *base = p;
    return FFGPU_OK;
}
int ffgpu_ipc_read(ffgpu_ctx* ctx, const void* base, unsigned long long offset, void* dst, size_t bytes,
                   const unsigned char* expect_canary32, void* stream) {
    if (!ctx || (bytes && (!base || !dst))) return FFGPU_EINVAL;
    DeviceGuard g(ctx->device);
    const char* src = (const char*)base + offset;
    if (expect_canary32) {
        unsigned char got[32];
        int rc = ipc_canary(src, bytes, got);
        if (rc != FFGPU_OK) return rc;
        if (memcmp(got, expect_canary32, 32) != 0) return FFGPU_ESTALE;
    }
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));          // the copy HAS run when the caller acknowledges the row
    return FFGPU_OK;
}
int ffgpu_ipc_read_reduced(ffgpu_ctx* ctx, const void* base, unsigned long long offset, void* dst, size_t n,
                           const unsigned char* expect_canary32, void* stream) {
    if (!ctx || (n && (!base || !dst))) return FFGPU_EINVAL;
    const char* src = (const char*)base + offset;
    if (expect_canary32) {
        DeviceGuard g(ctx->device);
        unsigned char got[32];
        int rc = ipc_canary(src, n * (size_t)ctx->elem_bytes, got);
        if (rc != FFGPU_OK) return rc;
        if (memcmp(got, expect_canary32, 32) != 0) return FFGPU_ESTALE;
    }
    int rc = ffgpu_reduce(ctx, src, dst, n, stream);            // ONE pass: the peer's row is read through the mapping
    if (rc != FFGPU_OK) return rc;
    DeviceGuard g(ctx->device);
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return FFGPU_OK;
}
int ffgpu_ipc_close(ffgpu_ctx* ctx, void* base) {
    if (!ctx || !base) return FFGPU_EINVAL;
    DeviceGuard g(ctx->device);
    HIPCHK(hipIpcCloseMemHandle(base));
    return FFGPU_OK;
}

int ffgpu_stream_sync(ffgpu_ctx* ctx, void* stream) {
    if (!ctx) return FFGPU_EINVAL;
    DeviceGuard g(ctx->device);
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return FFGPU_OK;
}

#define ARGCHK(cond) \
    do {             \
        if (!(cond)) return FFGPU_EINVAL; \
    } while (0)
// the first line of an entry of the secure rounds: a context (FFGPU_EINVAL), over a prime field (FFGPU_ENOTSUP)
#define PRIME_CTX(ctx) \
    do {               \
        ARGCHK(ctx);   \
        if ((ctx)->kind != FFGPU_PRIME) return FFGPU_ENOTSUP; \
    } while (0)
// what an entry with an X_args function does before it looks at a pointer: `call` is X_args(..., &work); the entry returns
// what X_args refused, and FFGPU_OK when there is nothing to do
#define ARGS_OR_RETURN(call) \
    do {                     \
        bool work;           \
        const int rc = (call); \
        if (rc != FFGPU_OK || !work) return rc; \
    } while (0)

// bytes of `rows` rows of n elements, `stride` elements apart
static size_t rows_bytes(const ffgpu_ctx* ctx, size_t rows, size_t stride, size_t n) {
    return ((rows > 0 ? rows - 1 : 0) * stride + n) * (size_t)ctx->elem_bytes;
}

static int do_ew2(ffgpu_ctx* ctx, int op, const void* a, const void* b, void* out, size_t n, void* stream) {
    ARGCHK(ctx);
    if (n == 0) return FFGPU_OK;
    ARGCHK(a && b && out);
    const size_t nb = rows_bytes(ctx, 1, 0, n);
    const ByteRange in[2] = {byte_range(a, nb), byte_range(b, nb)};
    CallScope cs(ctx, stream, HK_EW, in, 2, byte_range(out, nb));
    return status_of(ctx->ops->ew2(ctx->policy, cs.lc, op, a, b, out, n, cs.st));
}
static int do_ew1(ffgpu_ctx* ctx, int op, const void* a, const uint64_t* s, void* out, size_t n, void* stream) {
    ARGCHK(ctx);
    if (n == 0) return FFGPU_OK;
    ARGCHK(a && out);
    const size_t nb = rows_bytes(ctx, 1, 0, n);
    const ByteRange in = byte_range(a, nb);
    CallScope cs(ctx, stream, HK_EW, &in, 1, byte_range(out, nb));
    return status_of(ctx->ops->ew1(ctx->policy, cs.lc, op, a, s, out, n, cs.st));
}

int ffgpu_reduce(ffgpu_ctx* ctx, const void* raw, void* out, size_t n, void* stream) {
    return do_ew1(ctx, OP_REDUCE, raw, nullptr, out, n, stream);
}
int ffgpu_add(ffgpu_ctx* ctx, const void* a, const void* b, void* out, size_t n, void* stream) {
    return do_ew2(ctx, OP_ADD, a, b, out, n, stream);
}
int ffgpu_sub(ffgpu_ctx* ctx, const void* a, const void* b, void* out, size_t n, void* stream) {
    return do_ew2(ctx, OP_SUB, a, b, out, n, stream);
}
int ffgpu_mul(ffgpu_ctx* ctx, const void* a, const void* b, void* out, size_t n, void* stream) {
    const bool tables = ctx && ctx->gf8_tab_min && n >= (size_t)ctx->gf8_tab_min;
    const bool bitsliced = ctx && ctx->policy_kind == POL_GF2W64 && ctx->lc.gf2w_bitsliced && n >= ((size_t)1 << 21);
    if (!ctx || n == 0 || !a || !b || !out || !(tables || ctx->gf2w_limbs || bitsliced)) return do_ew2(ctx, OP_MUL, a, b, out, n, stream);
    // one scope and one hand-off step for the call, whichever kernels serve it (only the element-wise kernel takes
    // the policy word; ffgpu_last_kernel_ms reports the call, not its tail)
    const size_t nb = rows_bytes(ctx, 1, 0, n);
    const ByteRange in[2] = {byte_range(a, nb), byte_range(b, nb)};
    CallScope cs(ctx, stream, HK_EW, in, 2, byte_range(out, nb));
    if (tables) return status_of(ffgpu_launch_gf8_mul_tab(ctx->gf8_tables, cs.lc, a, b, out, n, cs.st));
    if (ctx->gf2w_limbs)
        return status_of(ffgpu_launch_gf2w_mul_win(ctx->policy, ctx->gf2w_limbs, ctx->gf2w_rtable, cs.lc, a, b, out, n, cs.st));
    // GF(2^64) with the default modulus: bit-sliced product for all whole pairs of elements, the element-wise kernel for
    // the odd last one (and for everything when the launcher declines: another modulus, unaligned arrays)
    size_t done = 0;
    const LaunchStatus ls = ffgpu_launch_gf2w64_mul_bitsliced(ctx->policy, cs.lc, a, b, out, n, cs.st, &done);
    if (ls.code != L_DECLINED && !ls.ok()) return status_of(ls);
    if (done == n) return FFGPU_OK;
    return status_of(ctx->ops->ew2(ctx->policy, cs.lc, OP_MUL, (const char*)a + 8 * done, (const char*)b + 8 * done,
                                   (char*)out + 8 * done, n - done, cs.st));
}
int ffgpu_neg(ffgpu_ctx* ctx, const void* a, void* out, size_t n, void* stream) {
    return do_ew1(ctx, OP_NEG, a, nullptr, out, n, stream);
}
int ffgpu_add_scalar(ffgpu_ctx* ctx, const void* a, const uint64_t* s, void* out, size_t n, void* stream) {
    ARGCHK(s);
    return do_ew1(ctx, OP_ADD, a, s, out, n, stream);
}
int ffgpu_mul_scalar(ffgpu_ctx* ctx, const void* a, const uint64_t* s, void* out, size_t n, void* stream) {
    ARGCHK(s);
    return do_ew1(ctx, OP_MUL, a, s, out, n, stream);
}
int ffgpu_rsub_scalar(ffgpu_ctx* ctx, const void* a, const uint64_t* s, void* out, size_t n, void* stream) {
    ARGCHK(s);
    return do_ew1(ctx, OP_RSUB, a, s, out, n, stream);
}
int ffgpu_muladd(ffgpu_ctx* ctx, const void* a, const void* b, const void* c, void* out, size_t n,
                 void* stream) {
    ARGCHK(ctx);
    if (n == 0) return FFGPU_OK;
    ARGCHK(a && b && c && out);
    const size_t nb = rows_bytes(ctx, 1, 0, n);
    const ByteRange in[3] = {byte_range(a, nb), byte_range(b, nb), byte_range(c, nb)};
    CallScope cs(ctx, stream, HK_EW, in, 3, byte_range(out, nb));
    return status_of(ctx->ops->muladd(ctx->policy, cs.lc, a, b, c, out, n, cs.st));
}

// the modulus of a context (its limbs are zero-padded to three) and its bit length
static U192 modulus_of(const ffgpu_ctx* ctx) { return U192(ctx->modulus, 3); }
static int modulus_bits(const ffgpu_ctx* ctx) { return modulus_of(ctx).bits(); }

static void set_exp(const U192& e, ExpArgs* ex) {
    ex->post = 0;
    e.store(ex->e, 3);
    ex->nbits = e.bits();
}
static int make_exp(const uint64_t* e, int limbs, ExpArgs* ex) {
    if (!e || limbs < 1 || limbs > 3) return FFGPU_EINVAL;
    set_exp(U192(e, limbs), ex);
    return FFGPU_OK;
}

// products (squarings + multiplications) of ff_pow_chain<true> for this exponent: the same decisions, on the host
static int exp_chain_cost(const ExpArgs& ex) {
    auto bit = [&](int i) -> int { return (int)((ex.e[i >> 6] >> (i & 63)) & 1u); };
    if (ex.nbits <= 1) return 0;
    int run = 0;
    for (int i = ex.nbits - 1; i >= 0 && bit(i); --i) ++run;
    int cost = 0, i = ex.nbits - 2;
    if (run >= 12) {
        int have = 1;
        for (int b = 30 - __builtin_clz((unsigned)run); b >= 0; --b) {
            cost += have + 1;
            have *= 2;
            if ((run >> b) & 1) {
                cost += 2;
                ++have;
            }
        }
        i = ex.nbits - 1 - run;
    }
    int ones = 0;
    for (int b = i; b >= 0; --b) ones += bit(b);
    if (i < 4 || ones <= 8 + (i + 1) / 8) return cost + (i + 1) + ones;
    cost += 8;                                              // a^2 and the seven odd powers
    while (i >= 0) {
        if (!bit(i)) {
            ++cost;
            --i;
            continue;
        }
        int j = i - 3 > 0 ? i - 3 : 0;
        while (!bit(j)) ++j;
        cost += (i - j + 1) + 1;
        i = j - 1;
    }
    return cost;
}
// e = 3 e' + 1 with a shorter chain for e' (+ 3 products for r^3 * a): hand over (e', post = 1)
static void exp_try_cube_form(ExpArgs* ex) {
    if (ex->nbits < 16) return;
    unsigned rem;
    const U192 q = U192(ex->e, 3).div3(&rem);
    if (rem != 1) return;
    ExpArgs alt;
    set_exp(q, &alt);
    if (alt.nbits == 0) return;
    if (exp_chain_cost(alt) + 3 < exp_chain_cost(*ex)) {
        alt.post = 1;
        *ex = alt;
    }
}

int ffgpu_pow(ffgpu_ctx* ctx, const void* a, const uint64_t* host_exp, int exp_limbs, void* out, size_t n,
              void* stream) {
    ARGCHK(ctx);
    ExpArgs ex;
    int rc = make_exp(host_exp, exp_limbs, &ex);
    if (rc != FFGPU_OK) return rc;
    exp_try_cube_form(&ex);
    if (n == 0) return FFGPU_OK;
    ARGCHK(a && out);
    CallScope cs(ctx, stream);
    if (ex.nbits == 0) {
        // a^0 = 1 (also for a = 0, as pow(0, 0, p) = 1): 0*a + 1
        uint64_t zero[3] = {0, 0, 0}, one[3] = {1, 0, 0};
        rc = status_of(ctx->ops->ew1(ctx->policy, cs.lc, OP_MUL, a, zero, out, n, cs.st));
        if (rc != FFGPU_OK) return rc;
        return status_of(ctx->ops->ew1(ctx->policy, cs.lc, OP_ADD, out, one, out, n, cs.st));
    }
    return status_of(ctx->ops->pow(ctx->policy, cs.lc, a, &ex, out, n, cs.st));
}

// exponent q - 2 (order of the multiplicative group minus one) for x^-1 = x^(q-2); false for the two-element fields
// GF(2) and GF(2^1), where q - 2 = 0 and x^-1 = x: exponent 1
static bool inverse_exponent(const ffgpu_ctx* ctx, ExpArgs* ex) {
    // (a binary context's modulus is the bit pattern of a polynomial of degree bits - 1)
    const U192 q = ctx->kind == FFGPU_PRIME ? modulus_of(ctx) : U192::pow2(modulus_bits(ctx) - 1);
    set_exp(p_minus_2(q), ex);
    if (ex->nbits == 0) {
        set_exp(1, ex);
        return false;
    }
    return true;
}

// the Legendre exponent (p - 1) / 2 of an odd prime field
static void legendre_exponent(const ffgpu_ctx* ctx, ExpArgs* ex) { set_exp(half_below(modulus_of(ctx)), ex); }

int ffgpu_sqrt_cl(ffgpu_ctx* ctx, const void* a, void* out, size_t n, void* stream) {
    ARGCHK(ctx);
    if (ctx->kind != FFGPU_PRIME || (ctx->modulus[0] & 3) != 1) return FFGPU_ENOTSUP;
    if (n == 0) return FFGPU_OK;
    ARGCHK(a && out);
    ExpArgs eleg, elad;
    legendre_exponent(ctx, &eleg);
    set_exp(half_above(modulus_of(ctx)), &elad);
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->sqrt_cl(ctx->policy, cs.lc, a, &eleg, &elad, out, n, cs.st));
}

int ffgpu_gauss(ffgpu_ctx* ctx, void* a, int n, int ncols, size_t batch, int mode, void* det_out,
                void* dev_singular, void* stream) {
    ARGCHK(ctx && n >= 0 && ncols >= n && (mode == 0 || mode == 1));
    if (batch == 0) return FFGPU_OK;
    ARGCHK(dev_singular && (mode == 0 || det_out));
    if (n == 0) return FFGPU_OK;
    ARGCHK(a);
    CallScope cs(ctx, stream);
    ExpArgs ex;
    inverse_exponent(ctx, &ex);
    HIPCHK(hipMemsetAsync(dev_singular, 0, batch * sizeof(int), cs.st));
    return status_of(ctx->ops->gauss(ctx->policy, cs.lc, a, n, ncols, batch, mode, &ex,
                                     mode ? det_out : nullptr, (int*)dev_singular, cs.st));
}

int ffgpu_inv(ffgpu_ctx* ctx, const void* a, void* out, size_t n, void* dev_zero_flag, void* stream) {
    ARGCHK(ctx);
    if (n == 0) return FFGPU_OK;
    ARGCHK(a && out);
    ExpArgs ex;
    inverse_exponent(ctx, &ex);
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->inv(ctx->policy, cs.lc, a, &ex, out, n, (int*)dev_zero_flag, cs.st));
}

int ffgpu_beaver_combine(ffgpu_ctx* ctx, const void* z, const void* x, const void* y, const void* d, const void* e,
                         int add_de, void* out, size_t n, void* stream) {
    ARGCHK(ctx);
    if (n == 0) return FFGPU_OK;
    ARGCHK(z && x && y && d && e && out);
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->beaver(ctx->policy, cs.lc, z, x, y, d, e, out, add_de ? 1 : 0, n,
                                      cs.st));
}

// what a share-generation call reads: a, then b and t rows of coefficients where present; returns how many ranges
static int split_inputs(const ffgpu_ctx* ctx, const void* a, const void* b, const void* coeffs, int t, size_t coeff_stride, size_t n,
                        ByteRange in[3]) {
    int nin = 0;
    in[nin++] = byte_range(a, rows_bytes(ctx, 1, 0, n));
    if (b) in[nin++] = byte_range(b, rows_bytes(ctx, 1, 0, n));
    if (coeffs) in[nin++] = byte_range(coeffs, rows_bytes(ctx, (size_t)t, coeff_stride, n));
    return nin;
}

static int do_split(ffgpu_ctx* ctx, const void* a, const void* b, bool fused, const void* coeffs,
                    size_t coeff_stride, int t, int m, void* shares, size_t share_stride, size_t n,
                    void* stream) {
    ARGCHK(ctx);
    ARGCHK(m >= 1 && t >= 0 && t < m);  // thresha.py:26 "0 <= t < m"
    if (n == 0) return FFGPU_OK;
    ARGCHK(a && shares && (!fused || b) && (t == 0 || coeffs));
    ARGCHK((m == 1 || share_stride >= n) && (t <= 1 || coeff_stride >= n));
    ByteRange in[3];
    const int nin = split_inputs(ctx, a, fused ? b : nullptr, t > 0 ? coeffs : nullptr, t, coeff_stride, n, in);
    CallScope cs(ctx, stream, HK_SPLIT, in, nin, byte_range(shares, rows_bytes(ctx, (size_t)m, share_stride, n)));
    return status_of(ctx->ops->split(ctx->policy, cs.lc, a, fused ? b : nullptr, coeffs,
                                     coeff_stride, t, m, shares, share_stride, n, cs.st,
                                     nullptr));
}

static int make_rng(const ffgpu_ctx* ctx, const uint8_t* key32, uint64_t nonce, int rounds, RngArgs* ra) {
    if (!key32) return FFGPU_EINVAL;
    if (rounds == 0) rounds = 20;
    if (rounds != 20 && rounds != 12 && rounds != 8) return FFGPU_EINVAL;
    memset(ra, 0, sizeof(*ra));
    memcpy(ra->rk.key, key32, 32);  // little-endian words, as RFC 8439
    ra->rk.nonce[0] = (uint32_t)nonce;
    ra->rk.nonce[1] = (uint32_t)(nonce >> 32);
    ra->rk.rounds = (uint32_t)rounds;
    ra->r0 = ctx->rng_r[0];
    ra->r1 = ctx->rng_r[1];
    return FFGPU_OK;
}

// the generator of a call whose key and nonce live on the device (ffgpu_rng_state_init); sampler: fill in the constant of
// the keystream sampler (the S-box layer draws bytes and leaves it zero)
static RngArgs make_dev_rng(const ffgpu_ctx* ctx, void* dev_state, uint64_t nonce_off, int defer_advance, bool sampler) {
    RngArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.rk.rounds = 20;
    if (sampler) {
        ra.r0 = ctx->rng_r[0];
        ra.r1 = ctx->rng_r[1];
    }
    ra.dev_key = (const RngKey*)dev_state;
    ra.nonce_off = (uint32_t)nonce_off;
    ra.no_advance = defer_advance ? 1 : 0;
    return ra;
}

static int do_split_rng(ffgpu_ctx* ctx, const void* a, const void* b, bool fused, const uint8_t* key32,
                        uint64_t nonce, int rounds, int t, int m, void* shares, size_t share_stride, size_t n,
                        void* stream) {
    ARGCHK(ctx);
    ARGCHK(m >= 1 && t >= 0 && t < m);
    RngArgs ra;
    int rc = make_rng(ctx, key32, nonce, rounds, &ra);
    if (rc != FFGPU_OK) return rc;
    if (n == 0) return FFGPU_OK;
    ARGCHK(a && shares && (!fused || b));
    ARGCHK(m == 1 || share_stride >= n);
    ByteRange in[3];
    const int nin = split_inputs(ctx, a, fused ? b : nullptr, nullptr, 0, 0, n, in);
    CallScope cs(ctx, stream, HK_SPLIT, in, nin, byte_range(shares, rows_bytes(ctx, (size_t)m, share_stride, n)));
    if (fused && t > 0) ra.aux = gf8_tables_on_device(ctx);
    return status_of(ctx->ops->split(ctx->policy, cs.lc, a, fused ? b : nullptr, nullptr, 0, t, m,
                                     shares, share_stride, n, cs.st, t > 0 ? &ra : nullptr));
}
int ffgpu_ctx_scalar_limbs(const ffgpu_ctx* ctx) { return (ctx && ctx->elem_bytes == 24) ? 3 : 2; }

size_t ffgpu_rng_state_bytes(void) { return sizeof(RngKey); }

int ffgpu_rng_state_init(ffgpu_ctx* ctx, void* dev_state, const uint8_t* host_key32, uint64_t nonce, int rounds,
                         void* stream) {
    ARGCHK(ctx && dev_state);
    RngArgs ra;
    int rc = make_rng(ctx, host_key32, nonce, rounds, &ra);
    if (rc != FFGPU_OK) return rc;
    CallScope cs(ctx, stream);
    HIPCHK(hipMemcpyAsync(dev_state, &ra.rk, sizeof(RngKey), hipMemcpyHostToDevice, cs.st));
    HIPCHK(hipStreamSynchronize(cs.st));     // the source is on this stack frame
    return FFGPU_OK;
}

int ffgpu_split_rng_state(ffgpu_ctx* ctx, const void* secrets, const void* mul_by, void* dev_state, int t, int m,
                          void* shares, size_t share_stride, size_t n, void* stream) {
    ARGCHK(ctx && dev_state);
    ARGCHK(m >= 1 && t >= 0 && t < m);
    if (n == 0) return FFGPU_OK;
    ARGCHK(secrets && shares && (m == 1 || share_stride >= n));
    RngArgs ra = make_dev_rng(ctx, dev_state, 0, 0, true);
    ByteRange in[3];
    const int nin = split_inputs(ctx, secrets, mul_by, nullptr, 0, 0, n, in);
    CallScope cs(ctx, stream, HK_SPLIT, in, nin, byte_range(shares, rows_bytes(ctx, (size_t)m, share_stride, n)));
    if (mul_by && t > 0) ra.aux = gf8_tables_on_device(ctx);
    // (the kernel's last workgroup advances the nonce, or rng_advance after it: launch.hpp, plan_rng)
    return status_of(ctx->ops->split(ctx->policy, cs.lc, secrets, mul_by, nullptr, 0, t, m, shares, share_stride, n, cs.st,
                                     t > 0 ? &ra : nullptr));
}

int ffgpu_gate_rng(ffgpu_ctx* ctx, const void* const* host_rows_a, const uint64_t* host_lambda_a, int ka,
                   const void* const* host_rows_b, const uint64_t* host_lambda_b, int kb, const uint8_t* host_key32,
                   uint64_t nonce, int rounds, void* dev_state, int t, int m, void* shares, size_t share_stride,
                   size_t n, void* stream) {
    return ffgpu_gate_rng_batch(ctx, host_rows_a, host_lambda_a, ka, 0, host_rows_b, host_lambda_b, kb, 0, host_key32,
                                dev_state ? 0 : nonce, rounds, dev_state, 0, t, m, shares, share_stride, 0, n, 1, stream);
}

int ffgpu_rng_state_advance(ffgpu_ctx* ctx, void* dev_state, uint32_t by, void* stream) {
    ARGCHK(ctx && dev_state);
    if (by == 0) return FFGPU_OK;
    DeviceGuard g(ctx->device);
    hipLaunchKernelGGL((k_rng_advance<0>), dim3(1), dim3(1), 0, (hipStream_t)stream, (RngKey*)dev_state, by);
    return status_of(launched());
}

int ffgpu_gate_rng_batch(ffgpu_ctx* ctx, const void* const* host_rows_a, const uint64_t* host_lambda_a, int ka,
                         size_t batch_stride_a, const void* const* host_rows_b, const uint64_t* host_lambda_b, int kb,
                         size_t batch_stride_b, const uint8_t* host_key32, uint64_t nonce, int rounds, void* dev_state,
                         int defer_advance, int t, int m, void* shares, size_t share_stride, size_t batch_stride_out,
                         size_t n, int nbatch, void* stream) {
    ARGCHK(ctx);
    ARGCHK(nbatch >= 1 && nbatch <= 255);
    ARGCHK(!dev_state || nonce <= 0xffffffffull);
    // host-key path: the batch row goes into bits 40..47 of the 64-bit nonce (bits 8..15 of nonce word 1); a caller
    // nonce that reaches those bits would alias another row's generator stream under a reused key
    ARGCHK(dev_state || nbatch == 1 || nonce < (1ull << 40));
    ARGCHK(m >= 1 && t >= 1 && t < m && ka >= 1 && kb >= 0);
    if (t > 3 || ka > 7 || kb > 7) return FFGPU_ENOTSUP;
    ARGCHK(host_rows_a && host_lambda_a && (kb == 0 || (host_rows_b && host_lambda_b)));
    RngArgs ra;
    if (dev_state) {
        ra = make_dev_rng(ctx, dev_state, nonce, defer_advance, true);
    } else {
        int rc = make_rng(ctx, host_key32, nonce, rounds, &ra);
        if (rc != FFGPU_OK) return rc;
    }
    if (n == 0) return FFGPU_OK;
    ARGCHK(shares && (m == 1 || share_stride >= n));
    for (int j = 0; j < ka; ++j) ARGCHK(host_rows_a[j]);
    for (int j = 0; j < kb; ++j) ARGCHK(host_rows_b[j]);
    ByteRange in[14];
    int nin = 0;
    for (int j = 0; j < ka; ++j) in[nin++] = byte_range(host_rows_a[j], rows_bytes(ctx, (size_t)nbatch, batch_stride_a, n));
    for (int j = 0; j < kb; ++j) in[nin++] = byte_range(host_rows_b[j], rows_bytes(ctx, (size_t)nbatch, batch_stride_b, n));
    const size_t oelems = ((size_t)nbatch - 1) * batch_stride_out + ((size_t)m - 1) * share_stride + n;
    CallScope cs(ctx, stream, HK_SPLIT, in, nin, byte_range(shares, oelems * (size_t)ctx->elem_bytes));
    ra.aux = gf8_tables_on_device(ctx);
    return status_of(ctx->ops->gate(ctx->policy, cs.lc, host_rows_a, host_lambda_a, ka, host_rows_b,
                                    host_lambda_b, kb, t, m, shares, share_stride, n, cs.st, &ra,
                                    nbatch, batch_stride_a, batch_stride_b, batch_stride_out));
}

int ffgpu_split(ffgpu_ctx* ctx, const void* secrets, const void* coeffs, size_t coeff_stride, int t, int m,
                void* shares, size_t share_stride, size_t n, void* stream) {
    return do_split(ctx, secrets, nullptr, false, coeffs, coeff_stride, t, m, shares, share_stride, n, stream);
}
int ffgpu_mul_split(ffgpu_ctx* ctx, const void* a, const void* b, const void* coeffs, size_t coeff_stride,
                    int t, int m, void* shares, size_t share_stride, size_t n, void* stream) {
    return do_split(ctx, a, b, true, coeffs, coeff_stride, t, m, shares, share_stride, n, stream);
}

int ffgpu_rng_coeffs(ffgpu_ctx* ctx, const uint8_t* host_key32, uint64_t nonce, int rounds, int t, void* coeffs,
                     size_t coeff_stride, size_t n, void* stream) {
    ARGCHK(ctx);
    ARGCHK(t >= 1);
    RngArgs ra;
    int rc = make_rng(ctx, host_key32, nonce, rounds, &ra);
    if (rc != FFGPU_OK) return rc;
    if (n == 0) return FFGPU_OK;
    ARGCHK(coeffs && (t == 1 || coeff_stride >= n));
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->rng_coeffs(ctx->policy, cs.lc, coeffs, coeff_stride, t, n,
                                          cs.st, &ra));
}
int ffgpu_split_rng(ffgpu_ctx* ctx, const void* secrets, const uint8_t* host_key32, uint64_t nonce, int rounds,
                    int t, int m, void* shares, size_t share_stride, size_t n, void* stream) {
    return do_split_rng(ctx, secrets, nullptr, false, host_key32, nonce, rounds, t, m, shares, share_stride, n,
                        stream);
}
int ffgpu_mul_split_rng(ffgpu_ctx* ctx, const void* a, const void* b, const uint8_t* host_key32, uint64_t nonce,
                        int rounds, int t, int m, void* shares, size_t share_stride, size_t n, void* stream) {
    return do_split_rng(ctx, a, b, true, host_key32, nonce, rounds, t, m, shares, share_stride, n, stream);
}

int ffgpu_recombine(ffgpu_ctx* ctx, const void* const* host_rows, const uint64_t* host_lambda, int k, int w,
                    void* out, size_t out_stride, size_t n, void* stream) {
    ARGCHK(ctx);
    ARGCHK(k >= 1 && w >= 1);
    if (n == 0) return FFGPU_OK;
    ARGCHK(host_rows && host_lambda && out && (w == 1 || out_stride >= n));
    for (int j = 0; j < k; ++j) ARGCHK(host_rows[j]);
    ByteRange in[MAXK_ANY];
    const int nin = k < (int)MAXK_ANY ? k : (int)MAXK_ANY;     // (more rows than that: the launcher refuses them)
    for (int j = 0; j < nin; ++j) in[j] = byte_range(host_rows[j], rows_bytes(ctx, 1, 0, n));
    CallScope cs(ctx, stream, HK_REC, in, nin, byte_range(out, rows_bytes(ctx, (size_t)w, out_stride, n)));
    // GF(2^n), 9 <= n <= 128 with a sparse modulus: shared nibble tables of the (uniform) Lagrange
    // coefficients in LDS instead of one full field multiplication per row and element
    if ((ctx->policy_kind == POL_GF2W64 || ctx->policy_kind == POL_GF2W128) && !ctx->gf2w_limbs && k <= 9 &&
        n >= 65536) {
        const int limbs = ctx->policy_kind == POL_GF2W128 ? 2 : 1;
        LaunchStatus ls;
        for (int r = 0; r < w && ls.ok(); ++r)
            ls = ffgpu_launch_gf2w_recombine(ctx->policy, limbs, cs.lc, host_rows, host_lambda + 2 * (size_t)r * k,
                                             k, (char*)out + (size_t)r * out_stride * ctx->elem_bytes, n, cs.st);
        if (ls.code != L_DECLINED) return status_of(ls);      // declined: the generic kernel below
    }
    return status_of(ctx->ops->recombine(ctx->policy, cs.lc, host_rows, host_lambda, k, w, out,
                                         out_stride, n, cs.st));
}

// one product through Launchers::matmul with the scratch of the call's stream (ffgpu_matmul, and ffgpu_matmul_stack for
// matrices that take the matrix-core, skinny or split-K routes)
static int matmul_one(ffgpu_ctx* ctx, const CallScope& cs, const void* A, size_t lda, const void* B, size_t ldb, void* C, size_t ldc,
                      size_t M, size_t K, size_t N) {
    // (restated in tests/matmul_contract.py, plan() -- move the two together)
    // scratch: int8 digit planes for the matrix-core product plus 64 MiB of split-K slabs (up to 8 GiB), else 64 MiB of
    // split-K partial sums.  (Asked for in whole 8 / 16 planes per operand: more than the 4 and 12 digits of 4- and
    // 12-byte elements need, and the split-K plans of the launcher see the size.)
    size_t want = 0;
    if (ctx->kind == FFGPU_PRIME) want = mfma_plane_bytes(cs.lc, ctx->elem_bytes <= 8 ? 8 : 16, M, K, N);
    if (want) want += (size_t)64 << 20;
    if (want > ((size_t)8 << 30)) want = 0;
    if (!want && K >= 64 && ((M + 31) / 32) * ((N + 31) / 32) < 2048) want = (size_t)64 << 20;
    void* ws = nullptr;
    size_t ws_bytes = 0;
    if (want) {
        const int rc = ctx->scratch.get(cs.st, want, &ws, &ws_bytes);
        if (rc != FFGPU_OK) return rc;
    }
    return status_of(ctx->ops->matmul(ctx->policy, cs.lc, A, lda, B, ldb, C, ldc, (int)M, (int)K, (int)N, ws, ws_bytes, cs.st));
}

int ffgpu_matmul(ffgpu_ctx* ctx, const void* A, size_t lda, const void* B, size_t ldb, void* C, size_t ldc,
                 size_t M, size_t K, size_t N, void* stream) {
    ARGCHK(ctx);
    if (M == 0 || N == 0) return FFGPU_OK;
    ARGCHK(C && ldc >= N && M < (1u << 30) && N < (1u << 30) && K < (1u << 30));
    ARGCHK(K == 0 || (A && B && lda >= K && ldb >= N));
    CallScope cs(ctx, stream);
    return matmul_one(ctx, cs, A, lda, B, ldb, C, ldc, M, K, N);
}

// bytes that `batch` matrices of `rows` rows of `cols` elements span, leading dimension ld and batch stride `stride`
// (0: one matrix); false when the sizes overflow
static bool stack_span(size_t batch, size_t stride, size_t rows, size_t ld, size_t cols, size_t eb, size_t* matrix, size_t* bytes) {
    size_t m, t;
    if (__builtin_mul_overflow(rows - 1, ld, &m) || __builtin_add_overflow(m, cols, &m)) return false;
    if (__builtin_mul_overflow(batch - 1, stride, &t) || __builtin_add_overflow(t, m, &t)) return false;
    if (!geom_bytes_ok(t, eb)) return false;
    *bytes = t * eb;
    *matrix = m;
    return true;
}

int ffgpu_matmul_stack(ffgpu_ctx* ctx, const void* A, size_t lda, size_t stride_a, const void* B, size_t ldb, size_t stride_b,
                       void* C, size_t ldc, size_t stride_c, size_t M, size_t K, size_t N, size_t batch, void* stream) {
    ARGCHK(ctx);
    if (batch == 0 || M == 0 || N == 0) return FFGPU_OK;
    ARGCHK(C && ldc >= N && M < (1u << 30) && N < (1u << 30) && K < (1u << 30));
    ARGCHK(K == 0 || (A && B && lda >= K && ldb >= N));
    const size_t eb = (size_t)ctx->elem_bytes;
    size_t mc, bytes_c;
    ARGCHK(stack_span(batch, stride_c, M, ldc, N, eb, &mc, &bytes_c));
    ARGCHK(stride_c >= mc || (stride_c == 0 && batch == 1));
    if (K > 0) {
        size_t ma, mb, bytes_a, bytes_b;
        ARGCHK(stack_span(batch, stride_a, M, lda, K, eb, &ma, &bytes_a) && stack_span(batch, stride_b, K, ldb, N, eb, &mb, &bytes_b));
        ARGCHK((stride_a == 0 || stride_a >= ma) && (stride_b == 0 || stride_b >= mb));
        const ByteRange o = byte_range(C, bytes_c);      // tiles and matrices are written while others are still read
        ARGCHK(!overlaps(o, byte_range(A, bytes_a)) && !overlaps(o, byte_range(B, bytes_b)));
    }
    // Matrices that Launchers::matmul would give to the matrix cores, or that are large enough for its skinny and split-K
    // routes to matter (FFGPU_MM_STACK_LOOP_MIN; default: just above the largest matrix the stack kernels were measured on and won, profiles/r12_matmul_stack.md), go through it one by one; the
    // others are one launch of the stack kernels, whose plan must hold the whole stack in one grid
    const bool loop = (double)M * (double)N * (double)K >= (double)ctx->lc.mm_stack_loop_min ||
                      (ctx->kind == FFGPU_PRIME && mfma_plane_bytes(ctx->lc, eb <= 8 ? 8 : 16, M, K, N) != 0);
    if (!loop)
        ARGCHK(stack_plan(M, K, N, batch, (int)eb, ctx->lc.num_cu, ctx->ops->stack_slot, stride_a == 0, stride_b == 0).ok);
    CallScope cs(ctx, stream);
    if (!loop)
        return status_of(ctx->ops->matmul_stack(ctx->policy, cs.lc, A, lda, stride_a, B, ldb, stride_b, C, ldc, stride_c, (int)M,
                                                (int)K, (int)N, batch, cs.st));
    for (size_t b = 0; b < batch; ++b) {
        const int rc = matmul_one(ctx, cs, (const char*)A + b * stride_a * eb, lda, (const char*)B + b * stride_b * eb, ldb,
                                  (char*)C + b * stride_c * eb, ldc, M, K, N);
        if (rc != FFGPU_OK) return rc;
    }
    return FFGPU_OK;
}

int ffgpu_convolve(ffgpu_ctx* ctx, const void* a, size_t na, const void* v, size_t nv, void* out, void* stream) {
    ARGCHK(ctx && a && v && out && na >= 1 && nv >= 1);
    ARGCHK(na < ((size_t)1 << 40) && nv < ((size_t)1 << 40));
    if (na < nv) {                                   // the shorter operand is the tap vector
        std::swap(a, v);
        std::swap(na, nv);
    }
    const size_t eb = (size_t)ctx->elem_bytes;
    const ByteRange o = byte_range(out, (na + nv - 1) * eb);
    ARGCHK(!overlaps(o, byte_range(a, na * eb)) && !overlaps(o, byte_range(v, nv * eb)));   // tiles read while others write
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->convolve(ctx->policy, cs.lc, a, na, v, nv, out, cs.st));
}

// the plan of a scan call, whichever alignment its pointers turn out to have: the larger workspace of the two
static size_t scan_ws_elems(const ffgpu_ctx* ctx, size_t outer, size_t k, size_t inner) {
    size_t need = 0;
    for (int aligned = 0; aligned < 2; ++aligned) {
        const ScanPlan p = scan_plan(outer, k, inner, (size_t)ctx->elem_bytes, aligned != 0, ctx->lc.num_cu, ctx->lc.scan_geom,
                                     ctx->lc.scan_tile_threads, 1);
        if (!p.ok) return 0;
        if (p.ws_elems > need) need = p.ws_elems;
    }
    return need;
}
size_t ffgpu_scan_workspace_bytes(ffgpu_ctx* ctx, size_t outer, size_t k, size_t inner) {
    if (!ctx) return 0;
    return scan_ws_elems(ctx, outer, k, inner) * (size_t)ctx->elem_bytes;
}
static int do_scan(ffgpu_ctx* ctx, bool reduce, int op, const void* a, void* out, size_t outer, size_t k, size_t inner,
                   int with_initial, void* workspace, size_t workspace_bytes, void* stream) {
    ARGCHK(ctx && a && out && (op == FFGPU_SCAN_ADD || op == FFGPU_SCAN_MUL));
    ARGCHK(k >= 1 && outer >= 1 && inner >= 1);
    const size_t eb = (size_t)ctx->elem_bytes;
    const uintptr_t amask = eb == 12 ? 3u : 15u;     // what the launcher asks of a pointer for 16-byte packs
    const bool aligned = (((uintptr_t)a | (uintptr_t)out) & amask) == 0;
    const ScanPlan p = scan_plan(outer, k, inner, eb, aligned, ctx->lc.num_cu, ctx->lc.scan_geom, ctx->lc.scan_tile_threads,
                                 with_initial ? 1 : 0);
    ARGCHK(p.ok);                                    // overflowing products, more tiles than a grid
    const size_t nin = p.lines * k, nout = reduce ? p.lines : p.lines * (k + (with_initial ? 1 : 0));
    const ByteRange in = byte_range(a, nin * eb), o = byte_range(out, nout * eb);
    // in place is safe (a thread or a workgroup reads its own elements before it writes them); any other overlap is not
    ARGCHK((!reduce && !with_initial && a == out) || !overlaps(o, in));
    ARGCHK(!workspace || ((uintptr_t)workspace & 15u) == 0);
    if (workspace && workspace_bytes) {
        const ByteRange w = byte_range(workspace, workspace_bytes);
        ARGCHK(!overlaps(w, in) && !overlaps(w, o));
    }
    CallScope cs(ctx, stream);
    return status_of(reduce ? ctx->ops->axis_reduce(ctx->policy, cs.lc, op, a, out, outer, k, inner, workspace, workspace_bytes, cs.st)
                            : ctx->ops->scan(ctx->policy, cs.lc, op, a, out, outer, k, inner, with_initial, workspace,
                                             workspace_bytes, cs.st));
}
int ffgpu_scan(ffgpu_ctx* ctx, int op, const void* a, void* out, size_t outer, size_t k, size_t inner, int with_initial,
               void* workspace, size_t workspace_bytes, void* stream) {
    return do_scan(ctx, false, op, a, out, outer, k, inner, with_initial, workspace, workspace_bytes, stream);
}
int ffgpu_axis_reduce(ffgpu_ctx* ctx, int op, const void* a, void* out, size_t outer, size_t k, size_t inner, void* workspace,
                      size_t workspace_bytes, void* stream) {
    return do_scan(ctx, true, op, a, out, outer, k, inner, 0, workspace, workspace_bytes, stream);
}

// ---- secure comparison: the local steps of np_sgn (sgn.hpp) -------------------------------------------------------------
// 2^l, 2^(l-1) and 2^-l mod p as host scalars of the context's limb count; false unless 1 <= l <= 64 and
// l <= bit_length(p) - 2 (the three constants are then field elements, 2^l < p / 2)
static bool sgn_consts(const ffgpu_ctx* ctx, int l, uint64_t out[9]) {
    return l <= SGN_MAX_L && pow2_consts(modulus_of(ctx), l, ffgpu_ctx_scalar_limbs(ctx), out);
}
// the first sub-share rows of an apply entry, which the entry looks at (more rows than MAXK: the entry itself or launch_rows
// refuses them, so a call with that many still gets that answer whatever lies past row MAXK)
static int rows_seen(int nrows) { return nrows < (int)MAXK ? nrows : (int)MAXK; }
static_assert((int)Operands::MAX_IN >= 3 * (int)CONV2D_MAX_SENDERS + 2 && (int)Operands::MAX_IN >= 2 * (int)RBITS_MAX_ROWS + 2 &&
              (int)Operands::MAX_OUT >= (int)CONV2D_MAX_SENDERS && (int)Operands::MAX_OUT >= (int)BSGN_MAX_PARTIES + 2 &&
              (int)Operands::MAX_OUT >= (int)RBITS_MAX_ROWS + 2, "operands.hpp holds the arrays of the largest callers");

int ffgpu_sgn_mask(ffgpu_ctx* ctx, const void* a, const void* rbits, const void* rdivl, int l, void* masked, size_t n,
                   void* stream) {
    PRIME_CTX(ctx);
    uint64_t consts[9];
    ARGCHK(sgn_consts(ctx, l, consts));
    if (n == 0) return FFGPU_OK;
    const size_t eb = (size_t)ctx->elem_bytes;
    const SgnPlan p = sgn_plan(n, l, eb);
    ARGCHK(p.ok);
    ARGCHK(Operands().in(a, n * eb).in(rbits, p.nl * eb).in(rdivl, n * eb).out(masked, n * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->sgn_mask(ctx->policy, cs.lc, a, rbits, rdivl, l, consts, masked, n, cs.st));
}

int ffgpu_sgn_expand(ffgpu_ctx* ctx, const void* c, const void* a, const void* rbits, const void* sbit, int l, void* e_out,
                     void* nx_out, void* z_out, size_t n, void* stream) {
    PRIME_CTX(ctx);
    uint64_t consts[9];
    ARGCHK(sgn_consts(ctx, l, consts));
    ARGCHK(e_out || nx_out || z_out);
    ARGCHK(sbit || !e_out);
    if (n == 0) return FFGPU_OK;
    const size_t eb = (size_t)ctx->elem_bytes;
    const SgnPlan p = sgn_plan(n, l, eb);
    ARGCHK(p.ok);
    Operands io;
    io.in(c, n * eb).in(a, n * eb).in(rbits, p.nl * eb).in_opt(sbit, n * eb);
    io.out_opt(e_out, (p.nl + n) * eb).out_opt(nx_out, p.nl * eb).out_opt(z_out, n * eb);
    ARGCHK(io.ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->sgn_expand(ctx->policy, cs.lc, c, a, rbits, e_out ? sbit : nullptr, l, consts, e_out, nx_out, z_out,
                                          n, cs.st));
}

int ffgpu_sgn_finish(ffgpu_ctx* ctx, const void* w, const void* sbit, const void* z, int l, void* lt_out, size_t n, void* stream) {
    PRIME_CTX(ctx);
    uint64_t consts[9];
    ARGCHK(sgn_consts(ctx, l, consts));
    if (n == 0) return FFGPU_OK;
    const size_t eb = (size_t)ctx->elem_bytes;
    ARGCHK(geom_bytes_ok(n, eb));                        // n * eb cannot overflow
    ARGCHK(Operands().in(w, n * eb).in(sbit, n * eb).in(z, n * eb).out(lt_out, n * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->sgn_finish(ctx->policy, cs.lc, w, sbit, z, l, consts, lt_out, n, cs.st));
}

// ---- sorting network: the two ends of a compare-exchange stage (sort.hpp) ------------------------------------------------
size_t ffgpu_cx_pairs(size_t k, size_t p, size_t d, size_t r) { return cx_pairs(k, p, d, r); }

// what both entries check before they look at a pointer: FFGPU_OK with *work == false when there is nothing to do
static int cx_args(const ffgpu_ctx* ctx, size_t outer, size_t k, size_t inner, size_t p, size_t d, size_t r, CxPlan* pl, bool* work) {
    ARGCHK(k >= 2 && cx_stage_valid(k, p, d, r));
    *work = false;
    if (outer == 0 || inner == 0) return FFGPU_OK;
    *pl = cx_plan(outer, k, inner, p, d, r, (size_t)ctx->elem_bytes, false);
    ARGCHK(pl->ok);                                      // the byte count of `a` overflows
    *work = pl->pairs != 0;
    return FFGPU_OK;
}

int ffgpu_cx_diff(ffgpu_ctx* ctx, const void* a, void* out, size_t outer, size_t k, size_t inner, size_t p, size_t d, size_t r,
                  void* stream) {
    PRIME_CTX(ctx);
    CxPlan pl;
    ARGS_OR_RETURN(cx_args(ctx, outer, k, inner, p, d, r, &pl, &work));
    const size_t eb = (size_t)ctx->elem_bytes;
    ARGCHK(Operands().in(a, outer * k * inner * eb).out(out, outer * pl.row_elems * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->cx_diff(ctx->policy, cs.lc, a, out, outer, k, inner, p, d, r, cs.st));
}

int ffgpu_cx_apply(ffgpu_ctx* ctx, void* a, const void* const* host_rows, const uint64_t* host_lambda, int nrows, size_t outer,
                   size_t k, size_t inner, size_t p, size_t d, size_t r, void* stream) {
    PRIME_CTX(ctx);
    ARGCHK(nrows >= 1);
    CxPlan pl;
    ARGS_OR_RETURN(cx_args(ctx, outer, k, inner, p, d, r, &pl, &work));
    const size_t eb = (size_t)ctx->elem_bytes;
    ARGCHK(Operands().inout(a, outer * k * inner * eb).in_rows(host_rows, rows_seen(nrows), outer * pl.row_elems * eb).host(host_lambda).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->cx_apply(ctx->policy, cs.lc, a, host_rows, host_lambda, nrows, outer, k, inner, p, d, r, cs.st));
}

// ---- tournament along an axis: the ends of a round (tour.hpp) -------------------------------------------------------------
static_assert((int)TOUR_HALVES == FFGPU_TOUR_HALVES && (int)TOUR_ODD_EVEN == FFGPU_TOUR_ODD_EVEN, "tour_geom.hpp and ffgpu.h name the pairings alike");
// what the four entries check before they look at a pointer: FFGPU_OK with *work == false when there is nothing to do
static int tour_args(const ffgpu_ctx* ctx, size_t outer, size_t k, size_t inner, int mode, TourPlan* pl, bool* work) {
    ARGCHK(k >= 2 && tour_mode_valid(mode));
    *work = false;
    if (outer == 0 || inner == 0) return FFGPU_OK;
    *pl = tour_plan(outer, k, inner, mode, (size_t)ctx->elem_bytes, false);
    ARGCHK(pl->ok);                                      // the byte count of the full level overflows
    *work = true;
    return FFGPU_OK;
}

int ffgpu_tour_diff(ffgpu_ctx* ctx, const void* a, void* out, size_t outer, size_t k, size_t inner, int mode, int neg, void* stream) {
    PRIME_CTX(ctx);
    TourPlan pl;
    ARGS_OR_RETURN(tour_args(ctx, outer, k, inner, mode, &pl, &work));
    const size_t eb = (size_t)ctx->elem_bytes;
    ARGCHK(Operands().in(a, outer * k * inner * eb).out(out, outer * pl.row_elems * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->tour_diff(ctx->policy, cs.lc, a, out, outer, k, inner, mode, neg, cs.st));
}

int ffgpu_tour_select(ffgpu_ctx* ctx, const void* a, const void* const* host_rows, const uint64_t* host_lambda, int nrows, void* out,
                      size_t outer, size_t k, size_t inner, int mode, int neg, void* stream) {
    PRIME_CTX(ctx);
    ARGCHK(nrows >= 1);
    TourPlan pl;
    ARGS_OR_RETURN(tour_args(ctx, outer, k, inner, mode, &pl, &work));
    const size_t eb = (size_t)ctx->elem_bytes;
    Operands io;
    io.in(a, outer * k * inner * eb).in_rows(host_rows, rows_seen(nrows), outer * pl.row_elems * eb).host(host_lambda);
    ARGCHK(io.out(out, outer * pl.next * inner * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->tour_select(ctx->policy, cs.lc, a, host_rows, host_lambda, nrows, out, outer, k, inner, mode, neg, cs.st));
}

int ffgpu_tour_unit_prod(ffgpu_ctx* ctx, const void* u, const void* c, void* out, size_t outer, size_t k, size_t inner, void* stream) {
    PRIME_CTX(ctx);
    TourPlan pl;
    ARGS_OR_RETURN(tour_args(ctx, outer, k, inner, TOUR_HALVES, &pl, &work));
    const size_t eb = (size_t)ctx->elem_bytes;
    ARGCHK(Operands().in(u, outer * pl.next * inner * eb).in(c, outer * pl.row_elems * eb).out(out, outer * pl.row_elems * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->tour_unit_prod(ctx->policy, cs.lc, u, c, out, outer, k, inner, cs.st));
}

int ffgpu_tour_unit_expand(ffgpu_ctx* ctx, const void* u, const void* const* host_rows, const uint64_t* host_lambda, int nrows,
                           void* out, size_t outer, size_t k, size_t inner, void* stream) {
    PRIME_CTX(ctx);
    ARGCHK(nrows >= 1);
    TourPlan pl;
    ARGS_OR_RETURN(tour_args(ctx, outer, k, inner, TOUR_ODD_EVEN, &pl, &work));
    const size_t eb = (size_t)ctx->elem_bytes;
    Operands io;
    io.in(u, outer * pl.next * inner * eb).in_rows(host_rows, rows_seen(nrows), outer * pl.row_elems * eb).host(host_lambda);
    ARGCHK(io.out(out, outer * k * inner * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->tour_unit_expand(ctx->policy, cs.lc, u, host_rows, host_lambda, nrows, out, outer, k, inner, cs.st));
}

// ---- first-occurrence search along an axis: the ends of a round (find.hpp) -------------------------------------------------
// what the three entries check before they look at a pointer: FFGPU_OK with *work == false when there is nothing to do.
// leaf: the bits are (outer, k, inner) and the round runs over k + virt positions; else a stored level (ncomp, outer, k, inner)
static int find_args(const ffgpu_ctx* ctx, size_t outer, size_t k, size_t inner, int ncomp, bool leaf, int flip, int virt, FindPlan* pl,
                     bool* work) {
    ARGCHK(find_comp_valid(ncomp) && (flip == 0 || flip == 1) && (virt == 0 || virt == 1));
    ARGCHK(k >= 1 && k <= ((size_t)1 << 62) && k + (size_t)virt >= 2);
    *work = false;
    if (outer == 0 || inner == 0) return FFGPU_OK;
    *pl = leaf ? find_leaf_plan(outer, k, inner, ncomp, virt, (size_t)ctx->elem_bytes, false)
               : find_plan(outer, k, inner, ncomp, (size_t)ctx->elem_bytes, false);
    ARGCHK(pl->t.ok);                                    // the byte count of a level overflows
    *work = true;
    return FFGPU_OK;
}

int ffgpu_find_leaf_prod(ffgpu_ctx* ctx, const void* bits, const void* tab, void* out, size_t outer, size_t k, size_t inner, int ncomp,
                         int flip, int virt, void* stream) {
    PRIME_CTX(ctx);
    FindPlan pl;
    ARGS_OR_RETURN(find_args(ctx, outer, k, inner, ncomp, true, flip, virt, &pl, &work));
    const size_t eb = (size_t)ctx->elem_bytes;
    Operands io;
    io.in(bits, outer * k * inner * eb).in(tab, (size_t)(ncomp - 1) * 2 * pl.kv * eb);
    ARGCHK(io.out(out, (size_t)ncomp * outer * pl.t.row_elems * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->find_leaf_prod(ctx->policy, cs.lc, bits, tab, out, outer, k, inner, ncomp, flip, virt, cs.st));
}

int ffgpu_find_leaf_apply(ffgpu_ctx* ctx, const void* bits, const void* tab, const void* const* host_rows, const uint64_t* host_lambda,
                          int nrows, void* out, size_t outer, size_t k, size_t inner, int ncomp, int flip, int virt, void* stream) {
    PRIME_CTX(ctx);
    if (nrows < 1 || nrows > (int)MAXK) return FFGPU_ENOTSUP;
    FindPlan pl;
    ARGS_OR_RETURN(find_args(ctx, outer, k, inner, ncomp, true, flip, virt, &pl, &work));
    const size_t eb = (size_t)ctx->elem_bytes;
    Operands io;
    io.in(bits, outer * k * inner * eb).in(tab, (size_t)(ncomp - 1) * 2 * pl.kv * eb);
    io.in_rows(host_rows, nrows, (size_t)ncomp * outer * pl.t.row_elems * eb).host(host_lambda);
    ARGCHK(io.out(out, (size_t)ncomp * outer * pl.t.next * inner * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->find_leaf_apply(ctx->policy, cs.lc, bits, tab, host_rows, host_lambda, nrows, out, outer, k, inner, ncomp,
                                               flip, virt, cs.st));
}

int ffgpu_find_prod(ffgpu_ctx* ctx, const void* level, void* out, size_t outer, size_t k, size_t inner, int ncomp, void* stream) {
    PRIME_CTX(ctx);
    FindPlan pl;
    ARGS_OR_RETURN(find_args(ctx, outer, k, inner, ncomp, false, 0, 0, &pl, &work));
    const size_t eb = (size_t)ctx->elem_bytes;
    ARGCHK(Operands().in(level, (size_t)ncomp * outer * k * inner * eb).out(out, (size_t)ncomp * outer * pl.t.row_elems * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->find_prod(ctx->policy, cs.lc, level, out, outer, k, inner, ncomp, cs.st));
}

// ---- bit decomposition over a prime field: the local steps of np_to_bits (bits.hpp) --------------------------------------
int ffgpu_carry_rounds(int l) { return bits_rounds(l); }
int ffgpu_carry_rows(int l, int round, int* rc, int* rd) {
    BitsLevel lv;
    ARGCHK(rc && rd && bits_level(l, round, lv));
    *rc = lv.rc;
    *rd = lv.rd;
    return FFGPU_OK;
}
int ffgpu_carry_level(int l, int round, uint8_t* k_out, uint8_t* q_out) {
    BitsLevel lv;
    ARGCHK(k_out && q_out && bits_level(l, round, lv));
    for (int j = 0; j < lv.rc + lv.rd; ++j) {
        k_out[j] = lv.k[j];
        q_out[j] = lv.q[j];
    }
    return FFGPU_OK;
}

// l as for the secure comparison (1 <= l <= 64, l <= bit_length(p) - 2: 2^l is a field element); 2^l as a host scalar
static bool bits_two_l(const ffgpu_ctx* ctx, int l, uint64_t out[3]) {
    uint64_t consts[9];
    if (!sgn_consts(ctx, l, consts)) return false;
    U192::pow2(l).store(out, 3);
    return true;
}
// the two scalars of a mask entry, 2^l and the caller's offset, as the launcher reads them; false as bits_two_l, or without offset
static bool mask_consts(const ffgpu_ctx* ctx, int l, const uint64_t* host_offset, uint64_t consts[6]) {
    uint64_t two_l[3];
    if (!bits_two_l(ctx, l, two_l) || !host_offset) return false;
    const int sl = ffgpu_ctx_scalar_limbs(ctx);
    for (int j = 0; j < 6; ++j) consts[j] = 0;
    U192(two_l, 3).store(consts, sl);
    U192(host_offset, sl).store(consts + sl, sl);
    return true;
}

int ffgpu_bits_mask(ffgpu_ctx* ctx, const void* a, const void* rbits, const void* rdivl, const uint64_t* host_offset, int l,
                    void* masked, size_t n, void* stream) {
    PRIME_CTX(ctx);
    uint64_t consts[6];
    ARGCHK(mask_consts(ctx, l, host_offset, consts));
    if (n == 0) return FFGPU_OK;
    const size_t eb = (size_t)ctx->elem_bytes;
    const SgnPlan p = sgn_plan(n, l, eb);
    ARGCHK(p.ok);
    ARGCHK(Operands().in(a, n * eb).in(rbits, p.nl * eb).in(rdivl, n * eb).out(masked, n * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->bits_mask(ctx->policy, cs.lc, a, rbits, rdivl, l, consts, masked, n, cs.st));
}

int ffgpu_bits_expand(ffgpu_ctx* ctx, const void* c, const void* rbits, int l, void* g_out, void* p_out, size_t n, void* stream) {
    PRIME_CTX(ctx);
    uint64_t two_l[3];
    ARGCHK(bits_two_l(ctx, l, two_l));
    if (n == 0) return FFGPU_OK;
    const size_t eb = (size_t)ctx->elem_bytes;
    const SgnPlan p = sgn_plan(n, l, eb);
    ARGCHK(p.ok);
    ARGCHK(Operands().in(c, n * eb).in(rbits, p.nl * eb).out(g_out, p.nl * eb).out(p_out, p.nl * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->bits_expand(ctx->policy, cs.lc, c, rbits, l, g_out, p_out, n, cs.st));
}

int ffgpu_bits_finish(ffgpu_ctx* ctx, const void* c, const void* rbits, const void* g, int l, void* out, size_t n, void* stream) {
    PRIME_CTX(ctx);
    uint64_t two_l[3];
    ARGCHK(bits_two_l(ctx, l, two_l));
    if (n == 0) return FFGPU_OK;
    const size_t eb = (size_t)ctx->elem_bytes;
    const SgnPlan p = sgn_plan(n, l, eb);
    ARGCHK(p.ok);
    ARGCHK(Operands().in(c, n * eb).in(rbits, p.nl * eb).in(g, p.nl * eb).out(out, p.nl * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->bits_finish(ctx->policy, cs.lc, c, rbits, g, l, out, n, cs.st));
}

// what both level entries check before they look at a pointer: FFGPU_OK with *work == false when there is nothing to do
static int carry_args(const ffgpu_ctx* ctx, int l, int round, size_t n, BitsLevel* lv, bool* work) {
    uint64_t two_l[3];
    ARGCHK(bits_two_l(ctx, l, two_l) && bits_level(l, round, *lv));
    *work = false;
    if (n == 0) return FFGPU_OK;
    ARGCHK(sgn_plan(n, l, (size_t)ctx->elem_bytes).ok);  // n * l or its byte size overflows
    *work = lv->rc + lv->rd != 0;
    return FFGPU_OK;
}

int ffgpu_carry_prod(ffgpu_ctx* ctx, const void* g, const void* p, int l, int round, void* out, size_t n, void* stream) {
    PRIME_CTX(ctx);
    BitsLevel lv;
    ARGS_OR_RETURN(carry_args(ctx, l, round, n, &lv, &work));
    const size_t eb = (size_t)ctx->elem_bytes, nl = n * (size_t)l;
    ARGCHK(Operands().in(g, nl * eb).in(p, nl * eb).out(out, (size_t)(lv.rc + lv.rd) * n * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->carry_prod(ctx->policy, cs.lc, g, p, l, lv, out, n, cs.st));
}

int ffgpu_carry_apply(ffgpu_ctx* ctx, void* g, void* p, const void* const* host_rows, const uint64_t* host_lambda, int nrows, int l,
                      int round, size_t n, void* stream) {
    PRIME_CTX(ctx);
    ARGCHK(nrows >= 1);
    BitsLevel lv;
    ARGS_OR_RETURN(carry_args(ctx, l, round, n, &lv, &work));
    const size_t eb = (size_t)ctx->elem_bytes, nl = n * (size_t)l;
    Operands io;
    io.inout(g, nl * eb).inout(p, nl * eb).in_rows(host_rows, rows_seen(nrows), (size_t)(lv.rc + lv.rd) * n * eb).host(host_lambda);
    ARGCHK(io.ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->carry_apply(ctx->policy, cs.lc, g, p, host_rows, host_lambda, nrows, l, lv, n, cs.st));
}

// ---- fixed point over a prime field: the local steps of np_trunc and of _norm (fxp.hpp) -------------------------------------
int ffgpu_trunc_mask(ffgpu_ctx* ctx, const void* a, const void* rbits, const void* rdivf, const uint64_t* host_offset, int f,
                     void* ar_out, void* masked_out, size_t n, void* stream) {
    PRIME_CTX(ctx);
    uint64_t consts[6];
    ARGCHK(mask_consts(ctx, f, host_offset, consts));
    if (n == 0) return FFGPU_OK;
    const size_t eb = (size_t)ctx->elem_bytes;
    const SgnPlan p = sgn_plan(n, f, eb);
    ARGCHK(p.ok);
    ARGCHK(Operands().in(a, n * eb).in(rbits, p.nl * eb).in(rdivf, n * eb).out(ar_out, n * eb).out(masked_out, n * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->trunc_mask(ctx->policy, cs.lc, a, rbits, rdivf, f, consts, ar_out, masked_out, n, cs.st));
}

int ffgpu_trunc_finish(ffgpu_ctx* ctx, const void* const* host_rows, const uint64_t* host_lambda, int nrows, const void* ar, int f,
                       void* out, size_t n, void* stream) {
    PRIME_CTX(ctx);
    ARGCHK(nrows >= 1);
    if (nrows > (int)MAXK) return FFGPU_ENOTSUP;
    uint64_t consts[9];
    ARGCHK(sgn_consts(ctx, f, consts));                  // 1 <= f <= 64, f <= bit_length(p) - 2; scalar 2: 2^-f
    if (n == 0) return FFGPU_OK;
    const size_t eb = (size_t)ctx->elem_bytes;
    ARGCHK(sgn_plan(n, f, eb).ok);
    ARGCHK(Operands().in_rows(host_rows, nrows, n * eb).host(host_lambda).in(ar, n * eb).out(out, n * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->trunc_finish(ctx->policy, cs.lc, host_rows, host_lambda, nrows, ar, f,
                                            consts + 2 * ffgpu_ctx_scalar_limbs(ctx), out, n, cs.st));
}

// what both norm entries check before they look at a pointer: FFGPU_OK with *work == false when there is nothing to do
static int norm_args(const ffgpu_ctx* ctx, int l, size_t n, RevPlan* pl, bool* work) {
    ARGCHK(fxp_norm_l_valid(l));
    *work = false;
    if (n == 0) return FFGPU_OK;
    *pl = fxp_norm_plan(n, l, (size_t)ctx->elem_bytes, false);
    ARGCHK(pl->ok);                                      // n * l or its byte size overflows
    *work = true;
    return FFGPU_OK;
}

int ffgpu_norm_prod(ffgpu_ctx* ctx, const void* bits, int l, void* out, void* sign_out, size_t n, void* stream) {
    PRIME_CTX(ctx);
    RevPlan pl;
    ARGS_OR_RETURN(norm_args(ctx, l, n, &pl, &work));
    const size_t eb = (size_t)ctx->elem_bytes;
    ARGCHK(Operands().in(bits, n * pl.l * eb).out(out, pl.elems * eb).out_opt(sign_out, n * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->norm_prod(ctx->policy, cs.lc, bits, l, out, sign_out, n, cs.st));
}

int ffgpu_norm_apply(ffgpu_ctx* ctx, const void* bits, const void* const* host_rows, const uint64_t* host_lambda, int nrows, int l,
                     void* out, size_t n, void* stream) {
    PRIME_CTX(ctx);
    ARGCHK(nrows >= 1);
    if (nrows > (int)MAXK) return FFGPU_ENOTSUP;
    RevPlan pl;
    ARGS_OR_RETURN(norm_args(ctx, l, n, &pl, &work));
    const size_t eb = (size_t)ctx->elem_bytes;
    ARGCHK(Operands().in(bits, n * pl.l * eb).in_rows(host_rows, nrows, pl.elems * eb).host(host_lambda).out(out, pl.elems * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->norm_apply(ctx->policy, cs.lc, bits, host_rows, host_lambda, nrows, l, out, n, cs.st));
}

// ---- logarithm and exponential of fixed-point numbers over a prime field: the local steps no other entry serves (explog.hpp;
// include/ffgpu_math.h) -------------------------------------------------------------------------------------------------------
int ffgm_powers_prod(ffgpu_ctx* ctx, const void* P, size_t stride, int h, int w, void* out, size_t n, void* stream) {
    PRIME_CTX(ctx);
    ARGCHK(explog_prod_valid(h, w));
    if (n == 0) return FFGPU_OK;
    const size_t eb = (size_t)ctx->elem_bytes;
    const RowsPlan pl = rows_plan(n, (size_t)h, stride, eb, false);
    size_t wn;
    ARGCHK(pl.ok && geom_mul_ok((size_t)w, n, wn) && geom_bytes_ok(wn, eb));
    ARGCHK(Operands().in(P, pl.span * eb).out(out, wn * eb).ok());                // (rows h.. of P's allocation lie past the span)
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->powers_prod(ctx->policy, cs.lc, P, stride, h, w, out, n, cs.st));
}

int ffgm_poly_dot(ffgpu_ctx* ctx, const void* P, size_t stride, int theta, const void* tab, const uint64_t* host_c0, void* out, size_t n,
                  void* stream) {
    PRIME_CTX(ctx);
    ARGCHK(explog_poly_valid(theta) && host_c0);
    if (n == 0) return FFGPU_OK;
    const size_t eb = (size_t)ctx->elem_bytes;
    const RowsPlan pl = rows_plan(n, (size_t)theta, stride, eb, false);
    ARGCHK(pl.ok);
    ARGCHK(Operands().in(P, pl.span * eb).in(tab, (size_t)theta * eb).out(out, n * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->poly_dot(ctx->policy, cs.lc, P, stride, theta, tab, host_c0, out, n, cs.st));
}

int ffgm_pow_base(ffgpu_ctx* ctx, const void* x, int shift, int ebits, const void* tab, void* out, size_t n, void* stream) {
    PRIME_CTX(ctx);
    const size_t eb = (size_t)ctx->elem_bytes;
    const int pbits = modulus_bits(ctx);
    ARGCHK(pow_base_plan(0, shift, ebits, pbits, eb).ok);
    if (n == 0) return FFGPU_OK;
    const PowBasePlan pl = pow_base_plan(n, shift, ebits, pbits, eb);
    ARGCHK(pl.ok);
    ARGCHK(Operands().in(x, n * eb).in(tab, (size_t)pl.tab_elems * eb).out(out, n * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->pow_base(ctx->policy, cs.lc, x, shift, ebits, pbits, tab, out, n, cs.st));
}

int ffgm_bits_reverse(ffgpu_ctx* ctx, const void* bits, int l, void* out, size_t n, void* stream) {
    PRIME_CTX(ctx);
    ARGCHK(explog_rev_l_valid(l));
    if (n == 0) return FFGPU_OK;
    const size_t eb = (size_t)ctx->elem_bytes;
    const RevPlan pl = explog_rev_plan(n, l, eb, false);
    ARGCHK(pl.ok);
    ARGCHK(Operands().in(bits, pl.elems * eb).out(out, pl.elems * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->bits_reverse(ctx->policy, cs.lc, bits, l, out, n, cs.st));
}

// ---- the Legendre zero test over a Blum prime: the local steps of runtime._np_is_zero (iszero.hpp; include/ffgpu_math.h) ----
int ffgm_iszero_mask(ffgpu_ctx* ctx, const void* a, const void* r, const void* z, const void* u2, int k, void* out, size_t n,
                     void* stream) {
    PRIME_CTX(ctx);
    const size_t eb = (size_t)ctx->elem_bytes;
    ARGCHK(iszero_mask_plan(n, k, eb, false).ok);
    if (n == 0) return FFGPU_OK;
    const size_t kn = iszero_mask_plan(n, k, eb, false).span * eb;
    ARGCHK(Operands().in(a, n * eb).in(r, kn).in(z, kn).in(u2, kn).out(out, kn).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->iszero_mask(ctx->policy, cs.lc, a, r, z, u2, k, out, n, cs.st));
}

int ffgm_legendre_code(ffgpu_ctx* ctx, const void* c, uint8_t* code, size_t count, void* stream) {
    PRIME_CTX(ctx);
    if (!ctx->modulus[2] && !ctx->modulus[1] && ctx->modulus[0] == 2) return FFGPU_ENOTSUP;
    const size_t eb = (size_t)ctx->elem_bytes;
    ARGCHK(stream_plan(count, eb, false).ok);
    if (count == 0) return FFGPU_OK;
    ARGCHK(Operands().in(c, count * eb).out(code, count).ok());
    ExpArgs ex;
    legendre_exponent(ctx, &ex);
    exp_try_cube_form(&ex);                                // (the choices of ffgpu_pow for this exponent)
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->legendre_code(ctx->policy, cs.lc, c, &ex, code, count, cs.st));
}

int ffgm_iszero_finish(ffgpu_ctx* ctx, const uint8_t* code, const void* z, void* out, size_t count, void* stream) {
    PRIME_CTX(ctx);
    const size_t eb = (size_t)ctx->elem_bytes;
    ARGCHK(flat_plan(count, eb, false).ok);
    if (count == 0) return FFGPU_OK;
    ARGCHK(Operands().in(code, count).in(z, count * eb).out(out, count * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->iszero_finish(ctx->policy, cs.lc, code, z, out, count, cs.st));
}

// ---- secure random bits over a prime field: the local steps of runtime.np_random_bits (rbits.hpp; include/ffgpu_math.h) ----
int ffgm_rbits_open(ffgpu_ctx* ctx, const void* const* host_r, const void* const* host_z, const uint64_t* host_lambda, int k, void* out,
                    int32_t* zeros, size_t n, void* stream) {
    PRIME_CTX(ctx);
    ARGCHK(k >= 1);
    if (k > (int)RBITS_MAX_ROWS) return FFGPU_ENOTSUP;
    const size_t eb = (size_t)ctx->elem_bytes;
    ARGCHK(rbits_open_plan(n, k, eb, false).ok);
    if (n == 0) return FFGPU_OK;
    Operands io;
    io.in_rows(host_r, k, n * eb).in_rows(host_z, k, n * eb).host(host_lambda);
    ARGCHK(io.out(out, n * eb).out_opt(zeros, sizeof(int32_t)).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->rbits_open(ctx->policy, cs.lc, host_r, host_z, host_lambda, k, out, zeros, n, cs.st));
}

int ffgm_rbits_finish(ffgpu_ctx* ctx, const void* c, const void* const* host_r, void* const* host_b, int m, int is_signed, int f, size_t n,
                      void* stream) {
    PRIME_CTX(ctx);
    if ((ctx->modulus[0] & 3) != 3) return FFGPU_ENOTSUP;
    ARGCHK(m >= 1 && f >= 0 && f < 192);
    if (m > (int)RBITS_MAX_ROWS) return FFGPU_ENOTSUP;
    const size_t eb = (size_t)ctx->elem_bytes;
    ARGCHK(rbits_finish_plan(n, m, eb, false).ok);
    if (n == 0) return FFGPU_OK;
    Operands io;
    int r0;
    io.in(c, n * eb).in_rows(host_r, m, n * eb, &r0);
    ARGCHK(io.out_rows(host_b, m, n * eb, r0).ok());       // (in place, host_b[i] == host_r[i]: the one overlap allowed)
    const U192 p = modulus_of(ctx);
    ExpArgs ex;
    set_exp(three_p_minus_5_over_4(p), &ex);
    exp_try_cube_form(&ex);                                // (the choices of ffgpu_pow for this exponent)
    // A = 2^f, B = 0 (signed), or A = B = (p + 1) / 2 2^f
    const U192 A = (is_signed ? U192(1) : half_above(p)).times_pow2_mod(f, p), B = is_signed ? U192(0) : A;
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->rbits_finish(ctx->policy, cs.lc, c, &ex, host_r, host_b, m, A.w, B.w, n, cs.st));
}

// ---- the secure binary sign by Legendre symbols: the local steps of the demo's bsgn (bsgn.hpp; include/ffgpu_math.h) ----
int ffgm_bsgn_mask(ffgpu_ctx* ctx, const void* a, const void* z, const uint64_t* host_alpha, const uint64_t* host_beta, int w, void* out,
                   size_t n, void* stream) {
    PRIME_CTX(ctx);
    ARGCHK(bsgn_w_valid(w));
    const size_t eb = (size_t)ctx->elem_bytes;
    const RowsPlan pl = bsgn_rows_plan(n, w, eb, false);
    ARGCHK(pl.ok);
    if (n == 0) return FFGPU_OK;
    const size_t wn = pl.span * eb;
    ARGCHK(Operands().in(a, n * eb).in(z, wn).host(host_alpha).host(host_beta).out(out, wn).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->bsgn_mask(ctx->policy, cs.lc, a, z, host_alpha, host_beta, w, out, n, cs.st));
}

int ffgm_bsgn_finish(ffgpu_ctx* ctx, const void* c, const void* const* host_s, void* const* host_out, int m, int w, int sum, size_t n,
                     void* stream) {
    PRIME_CTX(ctx);
    if (!ctx->modulus[2] && !ctx->modulus[1] && ctx->modulus[0] == 2) return FFGPU_ENOTSUP;
    ARGCHK(m >= 1 && bsgn_w_valid(w) && (sum == 0 || sum == 1));
    if (m > (int)BSGN_MAX_PARTIES) return FFGPU_ENOTSUP;
    const size_t eb = (size_t)ctx->elem_bytes;
    const RowsPlan pl = bsgn_rows_plan(n, w, eb, false);
    ARGCHK(pl.ok && bsgn_flat_plan(n, w, eb, false).ok);
    if (n == 0) return FFGPU_OK;
    const size_t wn = pl.span * eb, on = sum ? n * eb : wn;
    ARGCHK(Operands().in(c, wn).in_rows(host_s, m, wn).out_rows(host_out, m, on).ok());
    ExpArgs ex;
    legendre_exponent(ctx, &ex);
    exp_try_cube_form(&ex);                                // (the choices of ffgpu_pow for this exponent)
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->bsgn_finish(ctx->policy, cs.lc, c, &ex, host_s, host_out, m, w, sum, n, cs.st));
}

// ---- secure unit vectors and table lookup at secret indices: the local steps under runtime.np_unit_vector and
// runtime.unit_vector (unitvec.hpp; include/ffgpu_math.h) ----
int ffgm_unit_prod(ffgpu_ctx* ctx, const void* x, size_t xstride, const void* U, size_t h, void* out, size_t n, void* stream) {
    PRIME_CTX(ctx);
    ARGCHK(h >= 1 && xstride >= 1);
    const size_t eb = (size_t)ctx->elem_bytes;
    const RowsPlan pl = unit_rows_plan(n, h, eb, false);
    size_t xspan;
    ARGCHK(pl.ok && unit_x_span(n, xstride, eb, xspan));
    if (n == 0) return FFGPU_OK;
    ARGCHK(Operands().in(x, xspan * eb).in(U, pl.span * eb).out(out, pl.span * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->unit_prod(ctx->policy, cs.lc, x, xstride, U, h, out, n, cs.st));
}

int ffgm_unit_roll(ffgpu_ctx* ctx, const void* U, const void* c, int kbits, size_t K, void* out, size_t n, void* stream) {
    PRIME_CTX(ctx);
    ARGCHK(unit_roll_valid(kbits, K));
    const size_t eb = (size_t)ctx->elem_bytes;
    const RowsPlan pl = unit_rows_plan(n, (size_t)1 << kbits, eb, false);
    ARGCHK(pl.ok);
    if (n == 0) return FFGPU_OK;
    ARGCHK(Operands().in(U, pl.span * eb).in(c, n * eb).out(out, K * n * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->unit_roll(ctx->policy, cs.lc, U, c, kbits, K, out, n, cs.st));
}

int ffgm_unit_dot(ffgpu_ctx* ctx, const void* U, size_t rows, const void* c, int kbits, const void* tab, size_t tlen, void* out, size_t n,
                  void* stream) {
    PRIME_CTX(ctx);
    const size_t eb = (size_t)ctx->elem_bytes;
    const UnitDotPlan dp = unit_dot_plan(rows, c != nullptr, kbits, tlen, eb);
    ARGCHK(dp.ok);
    const RowsPlan pl = unit_rows_plan(n, rows, eb, false);
    ARGCHK(pl.ok);
    if (!dp.fits) return FFGPU_ENOTSUP;
    if (n == 0) return FFGPU_OK;
    ARGCHK(Operands().in(U, pl.span * eb).in(tab, tlen * eb).in_opt(c, n * eb).out(out, n * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->unit_dot(ctx->policy, cs.lc, U, rows, c, kbits, tab, tlen, out, n, cs.st));
}

// ---- secure 2-D convolution layers: the local correlation of the demo's convolvetensor for all senders (conv2d.hpp;
// include/ffgpu_math.h) ----
int ffgm_conv2d_plan(ffgpu_ctx* ctx, size_t k, size_t r, size_t m, size_t n, size_t v, int s, int nsend, ffgm_conv2d_plan_t* host_plan) {
    PRIME_CTX(ctx);
    ARGCHK(host_plan && nsend >= 1);
    if (nsend > (int)CONV2D_MAX_SENDERS) return FFGPU_ENOTSUP;
    const Conv2dPlan pl = ctx->ops->secure->conv2d_plan(ctx->lc, k, r, m, n, v, s, nsend);
    ARGCHK(pl.ok);
    if (!pl.grid_ok) return FFGPU_ENOTSUP;
    host_plan->tile_rows = pl.g.TH;
    host_plan->tile_cols = pl.g.TW;
    host_plan->out_channels = pl.g.VB;
    host_plan->in_channels_step = pl.g.CH;
    host_plan->flush_rows = pl.flush_rows;
    host_plan->wide = pl.wide;
    host_plan->grid_x = pl.empty ? 0 : (size_t)pl.grid_x;
    host_plan->grid_y = pl.empty ? 0 : (size_t)pl.grid_y;
    host_plan->lds_bytes = pl.lds_bytes;
    return FFGPU_OK;
}

int ffgm_conv2d(ffgpu_ctx* ctx, const void* const* host_x, const void* const* host_w, const void* const* host_b, void* const* host_out,
                int nsend, size_t k, size_t r, size_t m, size_t n, size_t v, int s, void* stream) {
    PRIME_CTX(ctx);
    ARGCHK(nsend >= 1);
    if (nsend > (int)CONV2D_MAX_SENDERS) return FFGPU_ENOTSUP;
    const size_t eb = (size_t)ctx->elem_bytes;
    const Conv2dPlan pl = ctx->ops->secure->conv2d_plan(ctx->lc, k, r, m, n, v, s, nsend);
    ARGCHK(pl.ok);
    if (pl.empty) return FFGPU_OK;
    if (!pl.grid_ok) return FFGPU_ENOTSUP;
    size_t nx, nw, ny;
    ARGCHK(conv2d_sizes(k, r, m, n, v, s, eb, &nx, &nw, &ny));
    Operands io;                                            // tiles read while others write: no output meets an input or another output
    io.in_rows(host_x, nsend, nx * eb).in_rows(host_w, nsend, nw * eb);
    if (host_b) io.in_rows(host_b, nsend, v * eb);
    ARGCHK(io.out_rows(host_out, nsend, ny * eb).ok());
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->secure->conv2d(ctx->policy, cs.lc, host_x, host_w, host_b, host_out, nsend, k, r, m, n, v, s, cs.st));
}

int ffgpu_group_matvec(ffgpu_ctx* ctx, const uint64_t* host_matrix, const uint64_t* host_bias, int r, int g,
                       const void* in, void* out, size_t ngroups, void* stream) {
    ARGCHK(ctx && host_matrix && r >= 1 && g >= 1);
    if (r > 16 || g > 16) return FFGPU_ENOTSUP;
    if (ngroups == 0) return FFGPU_OK;
    ARGCHK(in && out);
    CallScope cs(ctx, stream);
    if (ctx->kind == FFGPU_BINARY && ctx->elem_bytes == 1 && g == 8 && (((uintptr_t)in) & 7u) == 0) {
        // groups of 8 bytes: packed-byte kernel (misc.hip)
        if (r == 8 && (((uintptr_t)out) & 7u) == 0)
            return status_of(ffgpu_launch_gf8_group8(ctx->policy, cs.lc, host_matrix, host_bias, 0, in, out,
                                                     ngroups, cs.st));
        bool pow2 = (r == 1);
        for (int c = 0; pow2 && c < 8; ++c) pow2 = (host_matrix[2 * c] == (1ull << c));
        if (pow2 && (!host_bias || (host_bias[0] & 0xffu) == 0)) {   // np_from_bits: identity, then fold by 2^r
            uint64_t eye[128];
            memset(eye, 0, sizeof(eye));
            for (int c = 0; c < 8; ++c) eye[2 * (c * 8 + c)] = 1;
            return status_of(ffgpu_launch_gf8_group8(ctx->policy, cs.lc, eye, nullptr, 1, in, out, ngroups,
                                                     cs.st));
        }
    }
    return status_of(ctx->ops->group_matvec(ctx->policy, cs.lc, host_matrix, host_bias, r, g, in, out,
                                            ngroups, cs.st));
}

int ffgpu_gf256_bit_affine(ffgpu_ctx* ctx, const uint64_t* host_matrix, const uint64_t* host_bias, int from_bits,
                           const void* in, void* out, size_t n, void* stream) {
    ARGCHK(ctx && host_matrix);
    if (ctx->kind != FFGPU_BINARY || ctx->elem_bytes != 1) return FFGPU_ENOTSUP;
    if (n == 0) return FFGPU_OK;
    ARGCHK(in && out);
    if ((((uintptr_t)in) & 7u) || (!from_bits && (((uintptr_t)out) & 7u))) return FFGPU_EINVAL;
    CallScope cs(ctx, stream);
    return status_of(ffgpu_launch_gf8_group8(ctx->policy, cs.lc, host_matrix, host_bias, from_bits ? 1 : 0, in,
                                             out, n, cs.st));
}

static_assert((size_t)DOT_WORKSPACE_BYTES == (size_t)FFGPU_REDUCE_WORKSPACE_BYTES,
              "kernels.hpp bounds the grid of dot / sum by the workspace size that ffgpu.h names");
static int do_dot(ffgpu_ctx* ctx, const void* a, const void* b, void* out, void* workspace, size_t n, void* stream) {
    ARGCHK(ctx && out);
    CallScope cs(ctx, stream);
    if (n == 0) {   // empty sum = 0
        HIPCHK(hipMemsetAsync(out, 0, (size_t)ctx->elem_bytes, cs.st));
        return FFGPU_OK;
    }
    ARGCHK(a && workspace);
    return status_of(ctx->ops->dot(ctx->policy, cs.lc, a, b, out, workspace, n, cs.st));
}
int ffgpu_dot(ffgpu_ctx* ctx, const void* a, const void* b, void* out, void* workspace, size_t n, void* stream) {
    ARGCHK(n == 0 || b);
    return do_dot(ctx, a, b, out, workspace, n, stream);
}
int ffgpu_sum(ffgpu_ctx* ctx, const void* a, void* out, void* workspace, size_t n, void* stream) {
    return do_dot(ctx, a, nullptr, out, workspace, n, stream);
}

// a masked draw is a field element as it stands only when 2^mask_bits <= order: the modulus (a prime, or the bit pattern
// of a polynomial of degree n, order 2^n) has more than mask_bits bits
static bool prss_mask_fits(const ffgpu_ctx* ctx, int mask_bits) {
    return mask_bits < modulus_bits(ctx);
}

int ffgpu_prss_combine(ffgpu_ctx* ctx, const void* const* host_streams, int ks, int d, int l, int mask_bits,
                       const uint64_t* host_weights, int accumulate, void* out, size_t n, void* stream) {
    ARGCHK(ctx);
    ARGCHK(ks >= 1 && d >= 1 && l >= 1 && l <= 64 && mask_bits >= 0 && mask_bits <= 192);
    ARGCHK(prss_mask_fits(ctx, mask_bits));
    if (n == 0) return FFGPU_OK;
    ARGCHK(host_streams && host_weights && out);
    for (int s = 0; s < ks; ++s) ARGCHK(host_streams[s]);
    // limb radix constant for the wide reduction: 2^(8*elem_bytes) mod p (prime policies)
    uint64_t r2[2] = {ctx->rng_r[0], ctx->rng_r[1]};
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->prss(ctx->policy, cs.lc, host_streams, ks, d, l, mask_bits, host_weights,
                                    r2, accumulate, out, n, cs.st));
}

int ffgpu_prss_chacha(ffgpu_ctx* ctx, const uint8_t* host_keys, int ks, int d, int l, int mask_bits, int rounds,
                      const uint64_t* host_weights, int accumulate, void* out, size_t n, void* stream) {
    ARGCHK(ctx);
    ARGCHK(ks >= 1 && d >= 1 && l >= 1 && l <= 64 && mask_bits >= 0 && mask_bits <= 192);
    ARGCHK(rounds == 20 || rounds == 12 || rounds == 8);
    ARGCHK(prss_mask_fits(ctx, mask_bits));
    if (n == 0) return FFGPU_OK;
    ARGCHK(host_keys && host_weights && out);
    uint64_t r2[2] = {ctx->rng_r[0], ctx->rng_r[1]};
    CallScope cs(ctx, stream);
    return status_of(ctx->ops->prss_chacha(ctx->policy, cs.lc, host_keys, ks, d, l, mask_bits, rounds, host_weights,
                                           r2, accumulate, out, n, cs.st));
}
int ffgpu_prss_chacha_layout(int l, int* tb, int* dpt) {
    ARGCHK(l >= 1 && l <= 64 && tb && dpt);
    ffgpu::prss_cc_layout(l, tb, dpt);
    return FFGPU_OK;
}

int ffgpu_gf256_to_bits(ffgpu_ctx* ctx, const void* in, const void* addend, void* out, size_t n, void* stream) {
    ARGCHK(ctx);
    if (ctx->kind != FFGPU_BINARY || ctx->elem_bytes != 1) return FFGPU_ENOTSUP;
    if (n == 0) return FFGPU_OK;
    ARGCHK(in && out);
    CallScope cs(ctx, stream);
    return status_of(ffgpu_launch_gf8_to_bits(cs.lc, in, addend, out, n, cs.st));
}

int ffgpu_gf256_mask_open(ffgpu_ctx* ctx, const void* const* host_rows, const uint64_t* host_coef, int nrows,
                          const void* const* host_rbits, const uint64_t* host_mu, int np, void* out, size_t n, void* stream) {
    ARGCHK(ctx);
    if (ctx->kind != FFGPU_BINARY || ctx->elem_bytes != 1) return FFGPU_ENOTSUP;
    ARGCHK(nrows >= 0 && np >= 0 && nrows + np >= 1);
    if (nrows > 32 || np > 8) return FFGPU_ENOTSUP;
    if (n == 0) return FFGPU_OK;
    ARGCHK(out && (nrows == 0 || (host_rows && host_coef)) && (np == 0 || (host_rbits && host_mu)));
    for (int r = 0; r < nrows; ++r) ARGCHK(host_rows[r]);
    for (int p = 0; p < np; ++p) ARGCHK(host_rbits[p]);
    CallScope cs(ctx, stream);
    return status_of(ffgpu_launch_gf8_mask_open(ctx->policy, cs.lc, host_rows, host_coef, nrows, host_rbits, host_mu,
                                                np, out, n, cs.st));
}

int ffgpu_gf256_bits_affine_fold(ffgpu_ctx* ctx, const uint64_t* host_matrix, const uint64_t* host_bias, const void* c,
                                 const void* rbits, size_t rbits_batch_stride, void* out, size_t out_batch_stride, size_t n,
                                 int nbatch, void* stream) {
    ARGCHK(ctx && host_matrix);
    if (ctx->kind != FFGPU_BINARY || ctx->elem_bytes != 1) return FFGPU_ENOTSUP;
    ARGCHK(nbatch >= 1 && nbatch <= 65535);
    if (n == 0) return FFGPU_OK;
    ARGCHK(c && rbits && out);
    ARGCHK(nbatch == 1 || (rbits_batch_stride >= 8 * n && out_batch_stride >= n));
    CallScope cs(ctx, stream);
    return status_of(ffgpu_launch_gf8_bits_affine_fold(ctx->policy, cs.lc, host_matrix, host_bias, c, rbits,
                                                       rbits_batch_stride, out, out_batch_stride, n, nbatch,
                                                       cs.st));
}

}  // extern "C"

// tables of the fused S-box layer: log / antilog of the field, np_from_bits, affine fold -- cached on the device per
// (matrix, bias).  The caller holds the context's device.
static int sbox_layer_tables_on_device(ffgpu_ctx* ctx, const uint64_t* host_matrix, const uint64_t* host_bias) {
    unsigned char key[72];
    for (int i = 0; i < 64; ++i) key[i] = (unsigned char)(host_matrix[2 * i] & 0xffu);
    for (int i = 0; i < 8; ++i) key[64 + i] = host_bias ? (unsigned char)(host_bias[2 * i] & 0xffu) : 0;
    std::lock_guard<std::mutex> lk(ctx->sbl_mu);
    if (!ctx->sbl_tables_dev) {
        void* d = nullptr;
        if (hipMalloc(&d, 1536 + 2304 + 2304) != hipSuccess) return FFGPU_ENOMEM;
        ctx->sbl_tables_dev = d;
        ctx->sbl_valid = 0;
    }
    if (!ctx->sbl_valid || memcmp(key, ctx->sbl_key, sizeof(key)) != 0) {
        unsigned char host_tables[1536 + 2304 + 2304];
        ffgpu_gf8_sbox_layer_tables(ctx->policy, ctx->gf8_tables, host_matrix, host_bias, host_tables);
        // a DIFFERENT affine map than the cached one: launches that still read the old tables (on any stream) finish first
        if (ctx->sbl_valid) HIPCHK(hipDeviceSynchronize());
        // (synchronous copy: not inside a stream capture -- engine.CapturedLaunches warms the call up first)
        HIPCHK(hipMemcpy(ctx->sbl_tables_dev, host_tables, sizeof(host_tables), hipMemcpyHostToDevice));
        memcpy(ctx->sbl_key, key, sizeof(key));
        ctx->sbl_valid = 1;
    }
    return FFGPU_OK;
}

extern "C" {

int ffgpu_gf256_sbox_layer(ffgpu_ctx* ctx, const uint64_t* host_matrix, const uint64_t* host_bias, const uint64_t* host_lambda,
                           const uint64_t* host_mu, int t, int m, const void* x, size_t x_stride, const void* rbits,
                           size_t rbits_stride, void* out, size_t out_stride, size_t n, const uint8_t* host_key32, uint64_t nonce,
                           int rounds, void* dev_state, int defer_advance, void* stream) {
    ARGCHK(ctx && host_matrix && host_lambda && host_mu);
    if (ctx->kind != FFGPU_BINARY || ctx->elem_bytes != 1 || !ctx->gf8_tab_min) return FFGPU_ENOTSUP;
    ARGCHK(t >= 1 && m >= 2 * t + 1);
    if (t > 3 || m > 7) return FFGPU_ENOTSUP;
    ARGCHK(!dev_state || nonce <= 0xffffffffull);
    RngArgs ra;
    if (dev_state) {
        ra = make_dev_rng(ctx, dev_state, nonce, defer_advance, false);
    } else {
        int rc = make_rng(ctx, host_key32, nonce, rounds, &ra);
        if (rc != FFGPU_OK) return rc;
    }
    if (n == 0) return FFGPU_OK;
    ARGCHK(x && rbits && out && x_stride >= n && out_stride >= n && rbits_stride >= 8 * n);
    {   // (the tables go up before the scope opens: an upload is not part of the call's timed launches)
        DeviceGuard g(ctx->device);
        const int rc = sbox_layer_tables_on_device(ctx, host_matrix, host_bias);
        if (rc != FFGPU_OK) return rc;
    }
    CallScope cs(ctx, stream);
    return status_of(ffgpu_launch_gf8_sbox_layer(ctx->policy, cs.lc, x, x_stride, rbits, rbits_stride, out, out_stride,
                                                 ctx->sbl_tables_dev, host_lambda, host_mu, t, m, n, cs.st, &ra));
}

// what both Keccak entry points refuse before anything is launched
static int keccak_args_ok(const ffgpu_ctx* ctx, const void* const* host_rows, const uint64_t* host_lambda, int k, int iota_round) {
    ARGCHK(ctx && host_rows && host_lambda && k >= 1);
    if (ctx->kind != FFGPU_BINARY || ctx->elem_bytes != 1) return FFGPU_ENOTSUP;
    if (k > 7 || iota_round < -1 || iota_round > 23) return FFGPU_ENOTSUP;
    for (int s = 0; s < k; ++s) ARGCHK(host_rows[s]);
    return FFGPU_OK;
}

int ffgm_gf2_keccak_local(ffgpu_ctx* ctx, const void* const* host_rows, const uint64_t* host_lambda, int k, size_t batch_stride_in,
                           int nbatch, int iota_round, int apply_round, void* out, size_t batch_stride_out, size_t nstates,
                           void* stream) {
    const int rc = keccak_args_ok(ctx, host_rows, host_lambda, k, iota_round);
    if (rc != FFGPU_OK) return rc;
    ARGCHK(nbatch >= 1 && nbatch <= 255);
    if (nstates == 0) return FFGPU_OK;
    ARGCHK(out && (nbatch == 1 || (batch_stride_in >= 1600 * nstates && batch_stride_out >= 1600 * nstates)));
    CallScope cs(ctx, stream);
    return status_of(ffgpu_launch_keccak_local(ctx->policy, host_rows, host_lambda, k, batch_stride_in, nbatch, iota_round,
                                               apply_round, out, batch_stride_out, nstates, cs.st));
}

int ffgm_gf2_keccak_round(ffgpu_ctx* ctx, const void* const* host_rows, const uint64_t* host_lambda, int k, size_t batch_stride_in,
                           int iota_round, const uint8_t* host_key32, uint64_t nonce, int rounds, void* dev_state,
                           int defer_advance, int t, int m, void* shares, size_t share_stride, size_t batch_stride_out,
                           size_t nstates, void* stream) {
    const int rc0 = keccak_args_ok(ctx, host_rows, host_lambda, k, iota_round);
    if (rc0 != FFGPU_OK) return rc0;
    ARGCHK(m >= 1 && t >= 0 && t < m);
    if (!kk_pair_ok(m, t)) return FFGPU_ENOTSUP;
    ARGCHK(!dev_state || nonce <= 0xffffffffull);
    // host-key path: the sender goes into bits 40..47 of the 64-bit nonce, as the batch row of ffgpu_gate_rng_batch
    ARGCHK(dev_state || t == 0 || nonce < (1ull << 40));
    RngArgs ra;
    memset(&ra, 0, sizeof(ra));
    if (t > 0) {
        if (dev_state) {
            ra = make_dev_rng(ctx, dev_state, nonce, defer_advance, false);
        } else {
            const int rc = make_rng(ctx, host_key32, nonce, rounds, &ra);
            if (rc != FFGPU_OK) return rc;
        }
    }
    if (nstates == 0) return FFGPU_OK;
    ARGCHK(shares && (m == 1 || share_stride >= 1600 * nstates) && (t == 0 || (batch_stride_in >= 1600 * nstates && batch_stride_out >= 1600 * nstates)));
    CallScope cs(ctx, stream);
    return status_of(ffgpu_launch_keccak_round(ctx->policy, host_rows, host_lambda, k, batch_stride_in, iota_round, t, m, shares,
                                               share_stride, batch_stride_out, nstates, cs.st, &ra));
}

int ffgpu_gf256_sbox(ffgpu_ctx* ctx, const void* in, const uint8_t* host_rows8, uint8_t b, void* out,
                     size_t n, void* stream) {
    ARGCHK(ctx && host_rows8);
    if (ctx->kind != FFGPU_BINARY || ctx->elem_bytes != 1) return FFGPU_ENOTSUP;
    GF2P8 f;
    memcpy(&f, ctx->policy, sizeof(f));
    if (f.n != 8) return FFGPU_ENOTSUP;
    if (n == 0) return FFGPU_OK;
    ARGCHK(in && out);
    uint8_t lut[256];
    {
        std::lock_guard<std::mutex> lk(ctx->sbox_mu);
        uint8_t key[9];
        memcpy(key, host_rows8, 8);
        key[8] = b;
        if (!ctx->sbox_valid || memcmp(key, ctx->sbox_key, 9) != 0) {
            ffgpu_sbox_build_lut(ctx->policy, host_rows8, b, ctx->sbox_lut);
            memcpy(ctx->sbox_key, key, 9);
            ctx->sbox_valid = 1;
        }
        memcpy(lut, ctx->sbox_lut, 256);
    }
    CallScope cs(ctx, stream);
    return status_of(ffgpu_launch_sbox(lut, cs.lc, in, out, n, cs.st));
}

}  // extern "C"

// ---- timing helpers: HIP events on the launch stream ------------------------
template <class Fn>
static int time_loop(ffgpu_ctx* ctx, int reps, void* stream, float* ms, Fn fn) {
    ARGCHK(ctx && ms && reps >= 1);
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    int rc = FFGPU_OK;
    hipError_t he = hipEventRecord(e0, st);
    for (int i = 0; i < reps && rc == FFGPU_OK && he == hipSuccess; ++i) rc = fn();
    if (he == hipSuccess) he = hipEventRecord(e1, st);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    float t = 0.f;
    if (he == hipSuccess) he = hipEventElapsedTime(&t, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc != FFGPU_OK) return rc;
    if (he != hipSuccess) return hip_fail(he, "event timing");
    *ms = t / (float)reps;
    return FFGPU_OK;
}

extern "C" {

int ffgpu_time_mul(ffgpu_ctx* ctx, const void* a, const void* b, void* out, size_t n, int reps, void* stream,
                   float* ms) {
    return time_loop(ctx, reps, stream, ms, [&]() { return ffgpu_mul(ctx, a, b, out, n, stream); });
}
int ffgpu_time_split(ffgpu_ctx* ctx, const void* secrets, const void* coeffs, size_t coeff_stride, int t,
                     int m, void* shares, size_t share_stride, size_t n, int reps, void* stream, float* ms) {
    return time_loop(ctx, reps, stream, ms, [&]() {
        return ffgpu_split(ctx, secrets, coeffs, coeff_stride, t, m, shares, share_stride, n, stream);
    });
}
int ffgpu_time_recombine(ffgpu_ctx* ctx, const void* const* host_rows, const uint64_t* host_lambda, int k,
                         int w, void* out, size_t out_stride, size_t n, int reps, void* stream, float* ms) {
    return time_loop(ctx, reps, stream, ms, [&]() {
        return ffgpu_recombine(ctx, host_rows, host_lambda, k, w, out, out_stride, n, stream);
    });
}
int ffgpu_copy(ffgpu_ctx* ctx, const void* src, void* dst, size_t bytes, void* stream) {
    ARGCHK(ctx);
    if (bytes == 0) return FFGPU_OK;
    ARGCHK(src && dst);
    const ByteRange in = byte_range(src, bytes);
    CallScope cs(ctx, stream, HK_COPY, &in, 1, byte_range(dst, bytes));
    return status_of(ffgpu_launch_copy(cs.lc, src, dst, bytes, cs.st));
}
int ffgpu_valu_probe(ffgpu_ctx* ctx, int op, int iters, int waves_per_simd, void* scratch32, double* out3, void* stream) {
    ARGCHK(ctx && scratch32 && out3);
    ARGCHK(op >= 0 && op <= 13 && iters >= 1 && waves_per_simd >= 1 && waves_per_simd <= 8);
    DeviceGuard g(ctx->device);
    return status_of(ffgpu_launch_valu_probe(ctx->lc, op, iters, waves_per_simd, scratch32, out3, (hipStream_t)stream));
}
int ffgpu_time_copy(ffgpu_ctx* ctx, const void* src, void* dst, size_t bytes, int reps, void* stream,
                    float* ms) {
    ARGCHK(ctx && src && dst);
    return time_loop(ctx, reps, stream, ms, [&]() {
        return status_of(ffgpu_launch_copy(ctx->lc, src, dst, bytes, (hipStream_t)stream));
    });
}

}  // extern "C"
